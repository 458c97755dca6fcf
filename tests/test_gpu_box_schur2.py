"""GPU parity of the box twin's vertical Newton loop (box/VertSolve.cpp:1264-1458): mimsem_column_diag_theta_wup (csrc/column_newton.inc:
diagTheta2 with test functions upwinded by the vertical velocity, box/VertSolve.cpp:499-531), VortDiag.vert_mom_vort (AssembleVertMomVort,
:1460-1499) and VertSolve.solve_schur_2(theta_up=True, vert_mom_vort=...), against the numpy restatement tests/box_schur2_case.py (pinned on
the CPU by tests/test_box_schur2_cpu.py).  The bar is the project's 1e-10 (tests/test_gpu_schur2.py): relative L2, worst column and worst
interface."""
import types

import numpy as np
import pytest
import torch

from tests import box_schur2_case as bc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-10
ERR_ARG, ERR_UNSUPPORTED = -1, -2
FIELDS = ("velz", "rho", "rt", "exner")
# (p, ne, nk): nk = 2 is the smallest column (both levels miss a neighbour); p = 4 fills the 16-lane row; ne = 3 gives 9 columns, a partial
# wavefront of the one-column-per-row kernel
THETA_BOXES = [(1, 2, 2), (2, 2, 3), (3, 2, 5), (4, 2, 4), (2, 3, 3)]
SPHERE = (3, 2, 4)
LOOP_BOXES = [(3, 2, 5), (4, 2, 4)]
_CASES = {}
ids = lambda s: "p%d_ne%d_nk%d" % s


def _case(oracle, shape, sphere=False):
    """the case of tests/box_schur2_case.py, its engine and its device arrays: built once, never changed"""
    key = shape + (sphere,)
    if key not in _CASES:
        from mimsem_amd.device import DeviceMesh, Engine
        c = (bc.make_sphere if sphere else bc.make_box)(oracle, *shape)
        c["eng"] = Engine(DeviceMesh([c["topo"]], [c["geom"]], nk=shape[2], numbering="local" if sphere else "global"))
        c["dev"] = {k: c["eng"].tensor(v) for k, v in c["st"].items()}
        _CASES[key] = c
    return _CASES[key]


def worst(got, want, nEl, slots):
    """relative L2 of the worst column and of the worst interface / level"""
    g, w = np.asarray(got).reshape(nEl, slots, -1), np.asarray(want).reshape(nEl, slots, -1)
    col = np.linalg.norm((g - w).reshape(nEl, -1), axis=1) / np.linalg.norm(w.reshape(nEl, -1), axis=1)
    ifc = np.linalg.norm((g - w).transpose(1, 0, 2).reshape(slots, -1), axis=1) / np.linalg.norm(w.transpose(1, 0, 2).reshape(slots, -1), axis=1)
    return float(max(col.max(), ifc.max()))


def _theta(c, velz=None, **kw):
    d = c["dev"]
    return c["eng"].diag_theta_wup(bc.DTW, d["rho"], d["rt"], d["velz"] if velz is None else velz, **kw)


# ---- 1. the column entry against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sphere", [(s, False) for s in THETA_BOXES] + [(SPHERE, True)],
                         ids=[ids(s) for s in THETA_BOXES] + ["sphere_" + ids(SPHERE)])
def test_diag_theta_wup_matches_the_restatement(oracle, shape, sphere):
    c = _case(oracle, shape, sphere)
    P, st = c["P"], c["st"]
    want = bc.diag_theta2_up_all(P, st["rho"], st["rt"], st["velz"], bc.DTW)
    got = _theta(c).cpu().numpy()
    err = worst(got, want, P.nEl, P.nk + 1)
    print("diag_theta_wup %s: worst column / interface %.3e" % (ids(shape), err))
    assert np.isfinite(got).all() and err < TOL


# ---- 2. properties of the entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 2), (4, 2, 4)], ids=ids)
def test_zero_velocity_is_the_lumped_diagnosis(oracle, shape):
    c = _case(oracle, shape)
    P, d = c["P"], c["dev"]
    got = _theta(c, velz=torch.zeros_like(d["velz"])).cpu().numpy()
    want = c["eng"].diag_theta(1, d["rho"], d["rt"]).cpu().numpy()
    err = worst(got, want, P.nEl, P.nk + 1)
    print("velz = 0 against diag_theta(1) %s: %.3e" % (ids(shape), err))
    assert err < TOL


@pytest.mark.parametrize("shape", [(2, 3, 3), (4, 2, 4)], ids=ids)
def test_blend_determinism_and_capture(oracle, shape):
    c = _case(oracle, shape)
    eng, P = c["eng"], c["P"]
    plain = _theta(c)
    blend = eng.tensor(np.random.default_rng(5).uniform(250.0, 350.0, tuple(plain.shape)) * float(plain.abs().mean()) / 300.0)
    wa, wb = 0.375, 0.625
    got = _theta(c, blend2=blend, wa=wa, wb=wb)
    want = wa * plain + wb * blend
    err = float(((got - want).abs() / want.abs()).max())
    print("blended against wa plain + wb blend2 %s: %.3e" % (ids(shape), err))
    assert err < 1e-14                                   # one rounding of a fused multiply-add
    assert torch.equal(_theta(c), plain) and torch.equal(_theta(c, blend2=blend, wa=wa, wb=wb), got)
    g, out = eng.capture(lambda: [_theta(c, blend2=blend, wa=wa, wb=wb)])
    out[0].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], got)


def test_errors_leave_the_output_alone(oracle):
    from mimsem_amd.device import DeviceMesh, Engine, _ptr as p
    from tests.helpers import make_patch
    c = _case(oracle, (2, 2, 3))
    eng, d = c["eng"], c["dev"]
    out = torch.full((c["P"].nEl, 4 * c["P"].n2e), -7.0, dtype=torch.float64, device=eng.device)
    good = [p(d["rho"]), p(d["rt"]), p(d["velz"]), p(out)]
    for null in range(4):
        a = [None if i == null else x for i, x in enumerate(good)]
        assert eng.L.mimsem_column_diag_theta_wup(eng.ctx, bc.DTW, *a, None, 1.0, 0.0) == ERR_ARG, null
    assert eng.L.mimsem_column_diag_theta_wup(None, bc.DTW, *good, None, 1.0, 0.0) == ERR_ARG
    # nk = 1: no interface inside the column
    cs, topo, geom, P1, _ = make_patch(oracle, 2, 1, 6, 0, nk=1, seed=1)
    e1 = Engine(DeviceMesh([topo], [geom], nk=1, numbering="local"))
    z = lambda n: torch.ones(P1.nEl, max(n, 1) * P1.n2e, dtype=torch.float64, device=e1.device)
    o1 = torch.full((P1.nEl, 2 * P1.n2e), -7.0, dtype=torch.float64, device=e1.device)
    assert e1.L.mimsem_column_diag_theta_wup(e1.ctx, bc.DTW, p(z(1)), p(z(1)), p(z(0)), p(o1), None, 1.0, 0.0) == ERR_ARG
    # order 5
    cs, topo, geom, P5, _ = make_patch(oracle, 5, 1, 6, 0, nk=2, seed=1)
    e5 = Engine(DeviceMesh([topo], [geom], nk=2, numbering="local"))
    z = lambda n: torch.ones(P5.nEl, n * P5.n2e, dtype=torch.float64, device=e5.device)
    o5 = torch.full((P5.nEl, 3 * P5.n2e), -7.0, dtype=torch.float64, device=e5.device)
    assert e5.L.mimsem_column_diag_theta_wup(e5.ctx, bc.DTW, p(z(2)), p(z(2)), p(z(1)), p(o5), None, 1.0, 0.0) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for o in (out, o1, o5):
        assert bool((o == -7.0).all())


# ---- 3. AssembleVertMomVort -------------------------------------------------------------------------------------------------------
def _vort_diag(c):
    from mimsem_amd.vortdiag import VortDiag
    if "vd" not in c:
        c["vd"] = VortDiag(c["eng"], types.SimpleNamespace(eng=c["eng"]))       # (vert_mom_vort uses nothing of the HorizSolve)
        c["ul_dev"] = c["eng"].tensor(c["ul"])
    eng, nk = c["eng"], c["P"].nk
    return c["vd"], lambda velz_v: c["vd"].vert_mom_vort(c["ul_dev"], eng.l2_vert_to_horiz(velz_v.contiguous(), nk - 1))


@pytest.mark.parametrize("shape", [(3, 3, 3), (4, 2, 2)], ids=ids)
def test_vert_mom_vort_matches_the_restatement(oracle, shape):
    c = _case(oracle, shape)
    P = c["P"]
    vd, uuz = _vort_diag(c)
    want = bc.vert_mom_vort(c, bc.box_dense(c), c["ul"], c["st"]["velz"])
    got = uuz(c["dev"]["velz"])
    assert tuple(got.shape) == (P.nEl, (P.nk - 1) * P.n2e)
    err = worst(got.cpu().numpy(), want, P.nEl, P.nk - 1)
    print("vert_mom_vort %s: %.3e, %s mass-solve steps" % (ids(shape), err, vd.its["unit_mass"]))
    assert err < TOL
    assert vd.logged == 1 and vd.check() and vd.missed == 0 and vd.unit_mass.chebyshev          # the true residual, logged on the device
    assert vd.unit_mass.verify() and vd.unit_mass.solves_checked > 0 and vd.unit_mass.solves_missed == 0
    # a solve cut to two steps is reported (by the true residual: the preconditioner is exact on a uniform box, see vert_mom_vort)
    vd.unit_mass._chebyshev().set_steps(2)
    uuz(c["dev"]["velz"])
    assert not vd.check() and vd.missed == 1 and not vd.unit_mass.chebyshev
    c.pop("vd")                                          # (the solver has left the fixed-length mode: the loop tests make their own)


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------
def _run(c, fused, **kw):
    from mimsem_amd.vertsolve import VertSolve
    d = c["dev"]
    vs = VertSolve(c["eng"], bc.DT, rayleigh=0.0)
    out = vs.solve_schur_2(d["velz"], d["rho"], d["rt"], d["exner"], d["zv"], maxit=3, tol=0.0, schur3_flags=3, fused=fused, **kw)
    return vs, out


@pytest.mark.parametrize("shape", LOOP_BOXES, ids=ids)
def test_box_loop_matches_the_restatement(oracle, shape):
    """three iterations, theta_up with vert_mom_vort and a seeded udwdx: fused and composed against the restatement and against each other"""
    c = _case(oracle, shape)
    P, st = c["P"], c["st"]
    gd = bc.box_dense(c)
    want = bc.solve_schur_2_box(P, bc.DT, st["velz"], st["rho"], st["rt"], st["exner"], st["zv"], 3, udwdx=c["udwdx"],
                                uuz=lambda v: bc.vert_mom_vort(c, gd, c["ul"], v))
    vd, uuz = _vort_diag(c)
    udwdx = c["eng"].tensor(c["udwdx"])
    res = {}
    for fused in (True, False):
        vs, out = _run(c, fused, udwdx=udwdx, theta_up=True, vert_mom_vort=uuz)
        assert vd.check() and vd.unit_mass.verify()
        res[fused] = dict(zip(FIELDS, out), theta_h=vs.theta_h, exner_h=vs.exner_h)
        for name, a in res[fused].items():
            slots = {"velz": P.nk - 1, "theta_h": P.nk + 1}.get(name, P.nk)
            err = worst(a.cpu().numpy(), want[name], P.nEl, slots)
            print("box loop %s %s %s: %.3e" % (ids(shape), "fused" if fused else "composed", name, err))
            assert err < TOL, (fused, name, err)
        assert len(vs.history) == 3
    for name in res[True]:
        err = rel_l2(res[True][name].cpu().numpy(), res[False][name].cpu().numpy())
        print("box loop %s fused against composed %s: %.3e" % (ids(shape), name, err))
        assert err < TOL, name


@pytest.mark.parametrize("shape", LOOP_BOXES[:1], ids=ids)
def test_default_arguments_change_no_bit(oracle, shape):
    c = _case(oracle, shape)
    udwdx = c["eng"].tensor(c["udwdx"])
    for fused in (True, False):
        va, a = _run(c, fused, udwdx=udwdx)
        vb, b = _run(c, fused, udwdx=udwdx, theta_up=False, vert_mom_vort=None)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(va.theta_h, vb.theta_h)
        # ... and a callable without udwdx adds nothing, as the reference's `if(udwdx)` (box/VertSolve.cpp:1343, :1403)
        vc, cc = _run(c, fused, vert_mom_vort=lambda v: 1 / 0)
        vd, dd = _run(c, fused)
        assert all(torch.equal(x, y) for x, y in zip(cc, dd))
