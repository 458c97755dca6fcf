"""HorizSolve.advection_rhs, momentum_rhs and diagnose_fluxes(theta_in_Wt=True) (mimsem_amd/horizsolve.py; eul/HorizSolve.cpp:330-375,
:496-635, :313-317) against their numpy restatements in tests/strang2_case.py on the p = 3, ne = 2, nk = 3 sphere of tests/vort_diag_case.py,
per level at MOMENTUM_TOL = 1e-10 (the project's bar for these quantities: tests/test_gpu_next_rows.py), with the mass-flux right-hand side
by the fused kernel (fused_hu = True) and by the four composed applies (False); k2i relative to the sum of the magnitudes of its terms at the
same bar; and the _ec methods, which do not consult fused_hu, give the same bits either way."""
import numpy as np
import pytest
import torch

from tests import strang2_case as s2c
from tests import vort_diag_case as vc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
MOMENTUM_TOL = 1e-10


@pytest.fixture(scope="module")
def case(oracle):
    from mimsem_amd.device import DeviceMesh, Engine
    c = vc.make_case()
    F, gd, nk = c["F"], c["gd"], vc.NK
    dm = DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global")
    c["eng"], c["xq"] = Engine(dm), gd.xq[dm.gidq]
    r = np.random.default_rng(17)
    F["theta_i"] = r.uniform(290, 310, (nk + 1, gd.N2)) * F["area"]                   # theta on the nk+1 interfaces (no thickness)
    F["dudz1"] = r.standard_normal((nk - 1, gd.N1)) * 1e-3 * F["ln"]; F["dudz2"] = F["dudz1"] * 1.1
    F["dwdx1"] = r.standard_normal((nk - 1, gd.N1)) * 1e-4 * F["ln"]; F["dwdx2"] = F["dwdx1"] * 0.9
    hz = c["ho"].HorizOracle(gd)
    c["adv"] = s2c.advection_rhs(hz, F["u1"], F["u2"], F["h1"], F["h2"], F["theta_i"])
    Fk = c["adv"][2]
    margs = lambda k: (F["theta_i"], F["dudz1"], F["dudz2"], F["velz1"], F["velz2"], F["Pi"][k], F["u1"][k], F["u2"][k], F["h1"][k], F["h2"][k])
    mom = [s2c.momentum_rhs(hz, k, *margs(k), dwdx1=F["dwdx1"], dwdx2=F["dwdx2"], Fk=Fk[k]) for k in range(nk)]
    c["mom"] = np.stack([m[0] for m in mom])
    c["k2i"], c["k2i_abs"] = sum(m[1] for m in mom), sum(m[2] for m in mom)
    c["mom_plain"] = np.stack([s2c.momentum_rhs(hz, k, *margs(k)) for k in range(nk)])    # no dwdx, no Fk, velz for Fz
    return c


def _hs(c, fused):
    from mimsem_amd.horizsolve import HorizSolve
    hs = HorizSolve(c["eng"], quad_coords=c["xq"])
    assert hs.fused_hu is False
    hs.fused_hu = fused
    return hs


def _levels(label, got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (label, got.shape, want.shape)
    errs = [rel_l2(got[k], want[k]) for k in range(want.shape[0])]
    print("%s: relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
    assert np.all(np.isfinite(got)) and max(errs) < MOMENTUM_TOL, (label, errs)


@pytest.mark.parametrize("fused", (True, False))
def test_advection_rhs_against_the_restatement(case, fused):
    F, t = case["F"], case["eng"].tensor
    hs = _hs(case, fused)
    got = hs.advection_rhs(t(F["u1"]), t(F["u2"]), t(F["h1"]), t(F["h2"]), t(F["theta_i"]))
    for name, g, w in zip(("dF", "dG", "Fk", "Gk"), got, case["adv"]):
        _levels("advection_rhs %s, fused_hu = %s" % (name, fused), g, w)
    assert hs.Fk is got[2] and hs.Gk is got[3]
    assert hs.verify()
    # diagnose_fluxes: the default keeps the _ec form (theta in the levels) whatever fused_hu says
    Fd, Gd = hs.diagnose_fluxes(t(F["u1"]), t(F["u2"]), t(F["h1"]), t(F["h2"]), t(F["th"]))
    hs.fused_hu = not fused
    F0, G0 = hs.diagnose_fluxes(t(F["u1"]), t(F["u2"]), t(F["h1"]), t(F["h2"]), t(F["th"]))
    assert torch.equal(Fd, F0) and torch.equal(Gd, G0)


@pytest.mark.parametrize("fused", (True, False))
def test_momentum_rhs_against_the_restatement(case, fused):
    F, t = case["F"], case["eng"].tensor
    hs = _hs(case, fused)
    args = [t(F[n]) for n in ("theta_i", "dudz1", "dudz2", "velz1", "velz2", "Pi", "u1", "u2", "h1", "h2")]
    got = hs.momentum_rhs(*args, dwdx1=t(F["dwdx1"]), dwdx2=t(F["dwdx2"]), Fk=t(case["adv"][2]))
    _levels("momentum_rhs, fused_hu = %s" % fused, got, case["mom"])
    e = abs(hs.k2i - case["k2i"]) / case["k2i_abs"]
    print("k2i %.6e, restated %.6e, |difference| / sum of magnitudes %.2e" % (hs.k2i, case["k2i"], e))
    assert case["k2i"] != 0.0 and case["k2i_abs"] > 0 and e < MOMENTUM_TOL
    _levels("momentum_rhs without dwdx / Fz / Fk, fused_hu = %s" % fused, hs.momentum_rhs(*args), case["mom_plain"])
    assert hs.verify()
    assert rel_l2(case["mom"], case["mom_plain"]) > 1e-6                          # the optional terms are felt


def test_the_ec_methods_do_not_look_at_fused_hu(case):
    F, t = case["F"], case["eng"].tensor
    outs = {}
    for fused in (True, False):
        hs = _hs(case, fused)
        adv = hs.advection_rhs_ec(t(F["u1"]), t(F["u2"]), t(F["h1"]), t(F["h2"]), t(F["th"]))
        mom = hs.momentum_rhs_ec(*[t(F[n]) for n in ("th", "dudz1", "dudz2", "velz1", "velz2", "Pi", "u1", "u2", "h1", "h2")])
        outs[fused] = tuple(adv) + (mom,)
        assert hs.verify()
    assert all(torch.equal(a, b) for a, b in zip(outs[True], outs[False]))
