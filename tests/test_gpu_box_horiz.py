"""BoxHorizSolve.momentum_rhs and advection_rhs (mimsem_amd/horizsolve.py; box/HorizSolve.cpp:412-526, :214-324) against their numpy
restatements in tests/box_strang_case.py on its uniform-layer p = 3, ne = 3, nk = 4 periodic box, per level at MOMENTUM_TOL = 1e-10 (the bar
tests/test_gpu_horiz_rhs2.py holds the sphere's routines to), with the element-local forcing composed (fused_forcing = False) and by
mimsem_horiz_momentum_forcing (True); viscosity on and off; with and without Fk, k2i relative to the sum of the magnitudes of its terms at
the same bar.  And the sphere's HorizSolve.momentum_rhs with the same switch against tests/strang2_case.py."""
import numpy as np
import pytest
import torch

from tests import box_strang_case as bc
from tests import strang2_case as s2c
from tests import strang_case as sc
from tests import vort_diag_case as vc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
MOMENTUM_TOL = 1e-10
VORT = 1.0e3
ARGS = ("theta_i", "dudz1", "dudz2", "velz1", "velz2", "Pi", "u1", "u2")


@pytest.fixture(scope="module")
def case(oracle):
    """fields of the sizes a step hands the routines: the state of the case, its second velocities perturbations of the first, the
    vorticities and the vertical mass flux diagnosed from it by the restatement"""
    from mimsem_amd.device import DeviceMesh, Engine
    c = bc.make_case(oracle)
    gd, nk = c["gd"], c["nk"]
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global"))
    velx, velz_v, rho, rt, exner = c["state"]
    r = np.random.default_rng(23)
    F = dict(u1=velx, u2=velx * (1 + 0.05 * r.standard_normal(velx.shape)), h1=rho, h2=rho * (1 + 1e-3 * r.standard_normal(rho.shape)))
    # (the state's exner is horizontally uniform to 1e-6: its gradient would be the difference of nearly equal numbers on both sides and
    #  agree to 1e-10 only, which is the conditioning of that input and says nothing about the routine)
    F["Pi"] = exner * (1 + 1e-2 * r.standard_normal(exner.shape))
    F["velz1"] = sc.to_horiz(c, velz_v, nk - 1); F["velz2"] = F["velz1"] * (1 + 0.05 * r.standard_normal(F["velz1"].shape))
    F["theta_i"] = s2c.to_horiz(c, bc.theta_up(c, sc.to_vert(c, rho), sc.to_vert(c, rt), velz_v, bc.DT), nk + 1)
    # (the vorticities of this state times VORT: beside the pressure gradient of that exner the second vorticity term would be 4e-9 of the result)
    F["dudz1"] = VORT * vc.horiz_pot_vort(gd, velx, rho)[0]; F["dudz2"] = F["dudz1"] * 1.1
    F["dwdx1"] = VORT * vc.vert_vort(gd, F["velz1"], rho)[0]; F["dwdx2"] = F["dwdx1"] * 0.9
    F["Fz"] = vc.vert_mass_flux(gd, F["velz1"], F["velz2"], F["h1"], F["h2"])
    c["F"] = F
    c["ref"] = {}
    for visc in (False, True):
        hz = bc.BoxOracle(gd, c["lx"], do_visc=visc)
        if not visc:
            c["adv"] = bc.advection_rhs(hz, F["u1"], F["u2"], F["h1"], F["h2"], F["theta_i"])
        a = [F[n] for n in ARGS]
        full = bc.momentum_rhs_all(hz, *a, Fz=F["Fz"], dwdx1=F["dwdx1"], dwdx2=F["dwdx2"], Fk=c["adv"][2])
        c["ref"][visc] = dict(full=full[0], k2i=full[1], k2i_abs=full[2], plain=bc.momentum_rhs_all(hz, *a))
    return c


def _hs(c, fused, visc):
    from mimsem_amd.horizsolve import BoxHorizSolve
    hs = BoxHorizSolve(c["eng"], lx=c["lx"], do_visc=visc)
    assert hs.fused_forcing is False and hs.fg is None and hs.thickness == bc.DZ
    assert abs(hs.del2 - bc.BoxOracle(c["gd"], c["lx"]).del2) < 1e-14 * abs(hs.del2)
    hs.fused_forcing = fused
    return hs


def _levels(label, got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (label, got.shape, want.shape)
    errs = [rel_l2(got[k], want[k]) for k in range(want.shape[0])]
    print("%s: relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
    assert np.all(np.isfinite(got)) and max(errs) < MOMENTUM_TOL, (label, errs)


def test_advection_rhs_against_the_restatement(case):
    F, t = case["F"], lambda a: case["eng"].tensor(np.array(a))         # (the case's arrays are read-only: copies)
    hs = _hs(case, False, False)
    got = hs.advection_rhs(t(F["u1"]), t(F["u2"]), t(F["h1"]), t(F["h2"]), t(F["theta_i"]))
    for name, g, w in zip(("dF", "dG", "Fk", "Gk"), got, case["adv"]):
        _levels("box advection_rhs %s" % name, g, w)
    assert hs.Fk is got[2] and hs.verify()
    for fn in (hs.momentum_rhs_ec, hs.advection_rhs_ec, hs.diagnose_q):                  # no box twin
        with pytest.raises(NotImplementedError):
            fn()


@pytest.mark.parametrize("visc", (False, True), ids=("no_visc", "visc"))
@pytest.mark.parametrize("fused", (False, True), ids=("composed", "fused"))
def test_momentum_rhs_against_the_restatement(case, fused, visc):
    F, t = case["F"], lambda a: case["eng"].tensor(np.array(a))         # (the case's arrays are read-only: copies)
    ref = case["ref"][visc]
    hs = _hs(case, fused, visc)
    args = [t(F[n]) for n in ARGS] + [None, None]                                        # (rho1, rho2: the box rotational term takes none)
    got = hs.momentum_rhs(*args, Fz=t(F["Fz"]), dwdx1=t(F["dwdx1"]), dwdx2=t(F["dwdx2"]), Fk=t(case["adv"][2]))
    _levels("box momentum_rhs, fused_forcing = %s, do_visc = %s" % (fused, visc), got, ref["full"])
    e = abs(hs.k2i - ref["k2i"]) / ref["k2i_abs"]
    print("k2i %.6e, restated %.6e, |difference| / sum of magnitudes %.2e" % (hs.k2i, ref["k2i"], e))
    assert ref["k2i"] != 0.0 and ref["k2i_abs"] > 0 and e < MOMENTUM_TOL
    hs.k2i_dev = None
    _levels("box momentum_rhs without dwdx / Fz / Fk, fused_forcing = %s, do_visc = %s" % (fused, visc), hs.momentum_rhs(*args), ref["plain"])
    assert hs.k2i == 0.0 and hs.verify()                                                 # without Fk no k2i is formed
    assert rel_l2(ref["full"], ref["plain"]) > 1e-6                                      # the optional terms are felt
    if visc:
        assert rel_l2(ref["full"], case["ref"][False]["full"]) > 1e-6                    # and so is the viscosity


def test_sphere_momentum_rhs_with_the_fused_forcing(oracle):
    """HorizSolve.momentum_rhs takes the same switch (default off): the p = 3 sphere of tests/test_gpu_horiz_rhs2.py, a full Jacobian, the
    Coriolis term and the mass-flux solve in the rotational operands"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.horizsolve import HorizSolve
    c = vc.make_case()
    F, gd, nk = c["F"], c["gd"], vc.NK
    dm = DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global")
    eng = Engine(dm)
    r = np.random.default_rng(17)
    F["theta_i"] = r.uniform(290, 310, (nk + 1, gd.N2)) * F["area"]
    F["dudz1"] = r.standard_normal((nk - 1, gd.N1)) * 1e-3 * F["ln"]; F["dudz2"] = F["dudz1"] * 1.1
    F["dwdx1"] = r.standard_normal((nk - 1, gd.N1)) * 1e-4 * F["ln"]; F["dwdx2"] = F["dwdx1"] * 0.9
    hz = c["ho"].HorizOracle(gd)
    Fk = s2c.advection_rhs(hz, F["u1"], F["u2"], F["h1"], F["h2"], F["theta_i"])[2]
    names = ("theta_i", "dudz1", "dudz2", "velz1", "velz2", "Pi", "u1", "u2", "h1", "h2")
    mom = [s2c.momentum_rhs(hz, k, F["theta_i"], F["dudz1"], F["dudz2"], F["velz1"], F["velz2"], F["Pi"][k], F["u1"][k], F["u2"][k], F["h1"][k],
                            F["h2"][k], dwdx1=F["dwdx1"], dwdx2=F["dwdx2"], Fk=Fk[k]) for k in range(nk)]
    outs = {}
    for fused in (False, True):
        hs = HorizSolve(eng, quad_coords=gd.xq[dm.gidq])
        assert hs.fused_forcing is False
        hs.fused_forcing = fused
        outs[fused] = hs.momentum_rhs(*[eng.tensor(F[n]) for n in names], dwdx1=eng.tensor(F["dwdx1"]), dwdx2=eng.tensor(F["dwdx2"]), Fk=eng.tensor(Fk))
        _levels("sphere momentum_rhs, fused_forcing = %s" % fused, outs[fused], np.stack([m[0] for m in mom]))
        e = abs(hs.k2i - sum(m[1] for m in mom)) / sum(m[2] for m in mom)
        assert e < MOMENTUM_TOL, e
    assert not torch.equal(outs[True], outs[False])                                      # two routes, not one
