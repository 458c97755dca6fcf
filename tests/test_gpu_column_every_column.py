"""Every column of the small shapes of tests/column_cases.py against the CPU oracle, orders 1 to 6, column by column.

tests/test_gpu_column.py compares the per-column entries with the oracle on square one-patch meshes at orders 2 to 4.  The kernels behind them
carry several columns, or several (column, level) tasks, in the 16-lane DPP rows of one wavefront, and handle a partial wavefront by clamping
and "redo the last task, store nothing".  Here the column counts are chosen against those mappings (3, 5, 6, 9, 18: partial wavefronts with
one to three live rows, task tails, the last full column of a wave-per-column sweep), every sphere shape runs at an even and an odd level
count (two-sided / one-sided Thomas and pentadiagonal kernels), and orders 1, 5 and 6 reach the n2e = 1 instantiations, the workgroup Thomas
sweep, the thread-per-matrix LDS inverse and the wide Schur pipeline.  The error of each column is asserted on its own norm
(column_cases.assert_columns names the failing columns), so a small column cannot hide in a whole-array norm.

Tolerances are the project's: 1e-10 per column, for the solves the conditioning-aware budget of helpers.solve_error_budget beside the hard
1e-9, bit equality where two calls run the same kernel.  Each test prints one line: entry, shape, order, the worst column's error."""
import numpy as np
import pytest
import torch

from tests import column_cases as cc
from tests.column_cases import HARD, TOL, assert_columns
from tests.helpers import dense_from_band, rel_l2, solve_error_budget
from tests.test_gpu_column import COLCASES, HSCASES, _dense_from_blocks

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED = -2
FUSED_MAX_ORDER = 4                                      # mimsem_column_diag_theta_blend: orders 1..4 (include/mimsem_hip.h)
GEOMETRY_ONLY = ("CONST", "CONST_INV", "LINEAR", "LINEAR_INV", "RAYLEIGH", "LINCON", "LINCON2", "CONLIN")
INVERSE_OF = dict(LINEAR_INV="LINEAR", CONST_INV="CONST")
CASES = cc.all_cases()
HS_CASES = [c for c in CASES if c[0] in cc.ONE_PATCH]


def _with_engine(oracle, param):
    from mimsem_amd.device import Engine
    c = cc.build_case(oracle, *param)
    c.eng = Engine(c.dm)
    return c


@pytest.fixture(scope="module", params=CASES, ids=cc.case_id)
def case(request, oracle):
    return _with_engine(oracle, request.param)


@pytest.fixture(scope="module", params=HS_CASES, ids=cc.case_id)
def hs_case(request, oracle):
    """the one-patch shapes: uh of the upwinded entries is a 1-form row in the patch's own numbering"""
    return _with_engine(oracle, request.param)


def _t(eng):
    return lambda a: eng.tensor(a) if a is not None else None


def _per_column(case, fn):
    """fn(P, ex, ey, e) of the oracle for every context column, stacked"""
    return np.stack([fn(*case.col(e), e) for e in range(case.nEl)])


def _row(a, e):
    return None if a is None else a[e]


# ---- assembled operators and their applies --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colop,k1,k2,flag", COLCASES, ids=[f"{c[0]}_{c[3]}" for c in COLCASES])
def test_colop_blocks_and_apply(case, colop, k1, k2, flag):
    eng, P0, n2 = case.eng, case.P0, case.n2e
    F = case.fields()
    f1 = F[k1] if k1 else None; f2 = F[k2] if k2 else None
    t = _t(eng)
    blk = eng.colop_blocks(colop, f1=t(f1), f2=t(f2), flags=flag).cpu().numpy()
    rows, cols = P0.colop_dims(colop)
    r = np.random.default_rng(5)
    x = r.standard_normal((case.nEl, cols)); xt = r.standard_normal((case.nEl, rows))
    y = eng.colop_apply(colop, t(x), f1=t(f1), f2=t(f2), flags=flag, nout_slots=rows // n2).cpu().numpy()
    yt = eng.colop_apply(colop, t(xt), f1=t(f1), f2=t(f2), flags=flag, transpose=True, nout_slots=cols // n2).cpu().numpy()
    want = _per_column(case, lambda P, ex, ey, e: P.colop_dense(colop, ex, ey, flag=flag, f1=_row(f1, e), f2=_row(f2, e)))
    got = np.stack([_dense_from_blocks(P0, colop, blk[e]) for e in range(case.nEl)])
    errs = (assert_columns(colop + " blocks", got, want),
            assert_columns(colop + " apply", y, np.einsum("eij,ej->ei", want, x)),
            assert_columns(colop + "^T apply", yt, np.einsum("eji,ej->ei", want, xt)))
    print("colop %s flag %d on %s: blocks %.2e apply %.2e transposed %.2e" % ((colop, flag, case.label) + errs))


@pytest.mark.parametrize("colop", GEOMETRY_ONLY)
def test_colop_apply_blocks(case, colop):
    """mimsem_colop_apply_blocks, what both hosts use for the geometry-only operators they assemble once: blocks from colop_blocks, applied
    normal and transposed, against the oracle's dense matrix; the two inverses also against a solve with the oracle's LINEAR / CONST, so the
    inverse is held to the operator and not only to the oracle's own inverse"""
    eng, P0, n2 = case.eng, case.P0, case.n2e
    rows, cols = P0.colop_dims(colop)
    r = np.random.default_rng(35)
    x = r.standard_normal((case.nEl, cols)); xt = r.standard_normal((case.nEl, rows))
    blk = eng.colop_blocks(colop)
    y = eng.colop_apply_blocks(colop, blk, eng.tensor(x), rows // n2).cpu().numpy()
    yt = eng.colop_apply_blocks(colop, blk, eng.tensor(xt), cols // n2, transpose=True).cpu().numpy()
    want = _per_column(case, lambda P, ex, ey, e: P.colop_dense(colop, ex, ey))
    errs = [assert_columns(colop + " apply_blocks", y, np.einsum("eij,ej->ei", want, x)),
            assert_columns(colop + "^T apply_blocks", yt, np.einsum("eji,ej->ei", want, xt))]
    if colop in INVERSE_OF:
        A = _per_column(case, lambda P, ex, ey, e: P.colop_dense(INVERSE_OF[colop], ex, ey))
        errs.append(assert_columns(colop + " against the operator", y, np.stack([np.linalg.solve(A[e], x[e]) for e in range(case.nEl)])))
        errs.append(assert_columns(colop + "^T against the operator", yt, np.stack([np.linalg.solve(A[e].T, xt[e]) for e in range(case.nEl)])))
    print("colop_apply_blocks %s on %s: %s" % (colop, case.label, " ".join("%.2e" % v for v in errs)))


# ---- EOS vectors and theta diagnoses ---------------------------------------------------------------------------------------------------------
def test_eos_vectors(case):
    eng = case.eng
    F = case.fields()
    t = eng.tensor
    fac, expo = 1004.5 * (287.0 / 1e5) ** (287.0 / 717.5), 287.0 / 717.5
    got = [eng.column_eos(0, t(F["rt"]), t(F["pi"])), eng.column_eos(1, t(F["rt"]), None, fac, expo),
           eng.column_eos(2, t(F["thetaL"]), None), eng.column_eos(2, t(F["thetaL"]), t(F["eta"])), eng.column_eos(3, t(F["rho"]), t(F["eta"] * 1e-3))]
    want = [_per_column(case, lambda P, ex, ey, e: P.eos_residual(ex, ey, F["rt"][e], F["pi"][e])),
            _per_column(case, lambda P, ex, ey, e: P.eos_rhs(ex, ey, F["rt"][e], fac, expo)),
            _per_column(case, lambda P, ex, ey, e: P.const_log_theta_plus_eta(ex, ey, F["thetaL"][e])),
            _per_column(case, lambda P, ex, ey, e: P.const_log_theta_plus_eta(ex, ey, F["thetaL"][e], F["eta"][e])),
            _per_column(case, lambda P, ex, ey, e: P.const_rho_exp_eta(ex, ey, F["rho"][e], F["eta"][e] * 1e-3))]
    names = ("eos 0 residual", "eos 1 rhs", "eos 2 log theta", "eos 2 log theta + eta", "eos 3 rho exp eta")
    errs = [assert_columns(n, g.cpu().numpy(), w) for n, g, w in zip(names, got, want)]
    print("column_eos 0 1 2 2+eta 3 on %s: %s" % (case.label, " ".join("%.2e" % v for v in errs)))


def _oracle_thetas(case, F):
    return (_per_column(case, lambda P, ex, ey, e: P.diag_theta2(ex, ey, F["rho"][e], F["rt"][e])),
            _per_column(case, lambda P, ex, ey, e: P.diag_theta_L2(ex, ey, F["rho"][e], F["rt"][e])))


def test_diag_theta(case):
    eng = case.eng
    F = case.fields()
    want2, wantL = _oracle_thetas(case, F)
    thL = eng.diag_theta(0, eng.tensor(F["rho"]), eng.tensor(F["rt"])).cpu().numpy()
    th2 = eng.diag_theta(1, eng.tensor(F["rho"]), eng.tensor(F["rt"])).cpu().numpy()
    errs = (assert_columns("diag_theta(0)", thL, wantL), assert_columns("diag_theta(1)", th2, want2))
    print("diag_theta L2 / interfaces on %s: %.2e %.2e" % ((case.label,) + errs))


def test_diag_theta_blend(case):
    """mimsem_column_diag_theta_blend: both diagnoses in one launch, each alone and together, without blend fields and as
    wa theta + wb blend.  Orders 1..4 run k_diag_theta, the kernel mimsem_column_diag_theta itself launches there with one output and no
    blend field: the same instructions on the same inputs, so those outputs are asserted bit-equal.  Above order 4 the entry is documented
    as MIMSEM_ERR_UNSUPPORTED (the composed diag_theta is the route): that code, and the outputs untouched"""
    from mimsem_amd.device import _ptr
    eng, nk, n2 = case.eng, case.nk, case.n2e
    F = case.fields()
    rho, rt = eng.tensor(F["rho"]), eng.tensor(F["rt"])
    if case.pn > FUSED_MAX_ORDER:
        sent = -7.25
        th2 = torch.full((case.nEl, (nk + 1) * n2), sent, dtype=torch.float64, device=eng.device)
        thL = torch.full((case.nEl, nk * n2), sent, dtype=torch.float64, device=eng.device)
        for a, b in ((th2, thL), (th2, None), (None, thL)):
            rc = eng.L.mimsem_column_diag_theta_blend(eng.ctx, _ptr(rho), _ptr(rt), _ptr(a), None, _ptr(b), None, 1.0, 0.0)
            assert rc == ERR_UNSUPPORTED, rc
        eng.sync()
        assert bool((th2 == sent).all()) and bool((thL == sent).all())
        print("diag_theta_blend on %s: MIMSEM_ERR_UNSUPPORTED, outputs untouched" % case.label)
        return
    want2, wantL = _oracle_thetas(case, F)
    both2, bothL = eng.diag_theta_blend(rho, rt)
    only2, none = eng.diag_theta_blend(rho, rt, wantL=False)
    assert none is None
    none, onlyL = eng.diag_theta_blend(rho, rt, want2=False)
    assert none is None
    errs = [assert_columns("blend: theta2", both2.cpu().numpy(), want2), assert_columns("blend: thetaL", bothL.cpu().numpy(), wantL)]
    assert torch.equal(only2, both2) and torch.equal(onlyL, bothL)
    assert torch.equal(both2, eng.diag_theta(1, rho, rt)) and torch.equal(bothL, eng.diag_theta(0, rho, rt))
    r = np.random.default_rng(45)
    wa, wb = 0.25, 0.75
    b2 = r.uniform(0.5, 1.5, want2.shape) * np.abs(want2).mean(); bL = r.uniform(0.5, 1.5, wantL.shape) * np.abs(wantL).mean()
    m2, mL = eng.diag_theta_blend(rho, rt, blend2=eng.tensor(b2), blendL=eng.tensor(bL), wa=wa, wb=wb)
    errs += [assert_columns("blend: wa theta2 + wb blend2", m2.cpu().numpy(), wa * want2 + wb * b2),
             assert_columns("blend: wa thetaL + wb blendL", mL.cpu().numpy(), wa * wantL + wb * bL)]
    a2, none = eng.diag_theta_blend(rho, rt, blend2=eng.tensor(b2), wa=wa, wb=wb, wantL=False)
    none, aL = eng.diag_theta_blend(rho, rt, blendL=eng.tensor(bL), wa=wa, wb=wb, want2=False)
    assert torch.equal(a2, m2) and torch.equal(aL, mL)
    print("diag_theta_blend plain 2 / L, blended 2 / L on %s: %s" % (case.label, " ".join("%.2e" % v for v in errs)))


# ---- the two column solves -------------------------------------------------------------------------------------------------------------------
def _check_status(case):
    """status 0 for every column at orders <= 4; above, the path keeps no status: the documented n_unconverged == -1"""
    n, st, ratio = case.eng.solve_status()
    if case.pn <= 4:
        assert n == 0 and (st == 0).all(), (n, st.tolist(), ratio.tolist())
    else:
        assert n == -1, n


def _check_solve(case, e, Ld, rhs_dev, d_dev, ref, kL, kF, kd, others):
    """the assertions of test_gpu_column.test_schur_column_solve / _3_pentadiagonal for column e; returns the budget"""
    assert rel_l2(Ld, ref[kL]) < TOL, (case.label, e, rel_l2(Ld, ref[kL]))
    b = solve_error_budget(Ld, rhs_dev[e], d_dev[e], ref[kL], ref[kF], ref[kd])
    assert b["hip_vs_own_system"] < TOL, (e, b)
    bound = max(TOL, 4.0 * b["diff_of_exact_solutions"] + b["hip_vs_own_system"] + b["oracle_vs_own_system"])
    assert b["diff"] < bound, (e, b)
    assert b["diff"] < HARD, (e, b)
    for name, got in others:
        assert rel_l2(got[e], ref[name]) < min(max(TOL, 50.0 * bound), 50.0 * HARD), (name, e, b)
    return b


def _worst(budgets):
    return " ".join("%s %.2e" % (k, max(b[k] for b in budgets)) for k in ("rel_L", "hip_vs_own_system", "diff", "cond"))


def _schur_eta_against_the_oracle(case, keeps_status=True):
    """helmholtz_blocks and solve_schur_eta on the route the environment selects, every column against the oracle's; returns the solutions"""
    eng, nk, n2 = case.eng, case.nk, case.n2e
    F = case.fields()
    Fs = case.rhs(9)
    t = eng.tensor
    args = (75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]))
    L = eng.helmholtz_blocks(*args).cpu().numpy()
    dF = [t(f) for f in Fs]
    d = eng.solve_schur_eta(*args, *dF)
    if keeps_status:
        _check_status(case)
    else:
        assert eng.solve_status()[0] == -1
    d = [a.cpu().numpy() for a in d]; dF = [a.cpu().numpy() for a in dF]
    budgets = []
    for e in range(case.nEl):
        P, ex, ey = case.col(e)
        ref = P.solve_schur_column_eta(ex, ey, 75.0, F["thetaL"][e], F["rho"][e], F["eta"][e], F["pi"][e], *[f[e] for f in Fs])
        others = (("d_u", d[0]), ("d_eta", d[2]), ("d_rho", d[1]), ("F_u", dF[0]), ("F_rho", dF[1]), ("F_eta", dF[2]), ("F_pi", dF[3]))
        budgets.append(_check_solve(case, e, dense_from_band(L[e], nk, n2, lo=1), dF[3], d[3], ref, "L_pi", "F_pi", "d_pi", others))
    print("solve_schur_eta on %s: worst column %s" % (case.label, _worst(budgets)))
    return d


def test_schur_column_solve(case):
    _schur_eta_against_the_oracle(case)


def test_schur_column_solve_order_one_chain(oracle, monkeypatch):
    """order 1 with MIMSEM_SCHUR_FUSED=0: the chain of wide kernels ends in the wave-per-column Thomas sweep at n2e = 1, which no other
    setting of the default library launches (order 1 otherwise takes the fused sweep, and the chain of orders 2 to 4 the row-per-lane
    Thomas kernel).  The four columns of the smallest box against the oracle like every other route, then against the fused route"""
    case = _with_engine(oracle, ("B4", 1, 4))
    fused = _schur_eta_against_the_oracle(case)
    monkeypatch.setenv("MIMSEM_SCHUR_FUSED", "0")
    chain = _schur_eta_against_the_oracle(case, keeps_status=False)
    for name, a, b in zip(("d_u", "d_rho", "d_eta", "d_pi"), chain, fused):
        assert_columns("chain against fused " + name, a, b)


@pytest.mark.parametrize("flags", [0, 3], ids=["eul", "box"])
def test_schur_column_3_pentadiagonal(case, flags):
    eng, nk, n2 = case.eng, case.nk, case.n2e
    F = case.fields()
    Fs = case.rhs(29)
    t = eng.tensor
    dF = [t(f) for f in Fs]
    out = eng.solve_schur_3(75.0, t(F["theta"]), t(F["velz"]), t(F["rho"]), t(F["rt"]), t(F["pi"]), *dF, want_L=True, flags=flags)
    _check_status(case)
    d = [a.cpu().numpy() for a in out[:4]]; L = out[4].cpu().numpy(); dF = [a.cpu().numpy() for a in dF]
    budgets = []
    for e in range(case.nEl):
        P, ex, ey = case.col(e)
        ref = P.solve_schur_column_3(ex, ey, 75.0, F["theta"][e], F["velz"][e], F["rho"][e], F["rt"][e], F["pi"][e], *[f[e] for f in Fs], flags=flags)
        others = (("d_u", d[0]), ("d_pi", d[3]), ("d_rho", d[1]), ("F_u", dF[0]), ("F_rho", dF[1]), ("F_rt", dF[2]), ("F_pi", dF[3]))
        budgets.append(_check_solve(case, e, dense_from_band(L[e], nk, n2, lo=2), dF[2], d[2], ref, "L", "F_rt", "d_rt", others))
    print("solve_schur_3 flags %d on %s: worst column %s" % (flags, case.label, _worst(budgets)))


# ---- the Strang / Held-Suarez entries: one-patch shapes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("colop,k1,k2,param,up", HSCASES, ids=[f"{c[0]}_{c[2]}" for c in HSCASES])
def test_hs_colops(hs_case, colop, k1, k2, param, up):
    case = hs_case
    eng, P, n2 = case.eng, case.P0, case.n2e
    if up and P.n > 7:
        pytest.skip("edge-function scratch sized for p <= 7")
    F = case.fields()
    r = np.random.default_rng(15)
    f1 = F[k1] if k1 else None; f2 = F[k2] if k2 else None
    uh = case.uh(r, param) if up else None
    t = _t(eng)
    blk = eng.colop_blocks_ex(colop, param=param, f1=t(f1), f2=t(f2), uh=t(uh)).cpu().numpy()
    rows, cols = P.colop_dims(colop)
    x = r.standard_normal((case.nEl, cols))
    y = eng.colop_apply_ex(colop, t(x), rows // n2, param=param, f1=t(f1), f2=t(f2), uh=t(uh)).cpu().numpy()
    want = _per_column(case, lambda P, ex, ey, e: P.colop_dense_ex(colop, ex, ey, param=param, f1=_row(f1, e), f2=_row(f2, e), uh=uh))
    got = np.stack([_dense_from_blocks(P, colop, blk[e]) for e in range(case.nEl)])
    errs = (assert_columns(colop + " blocks_ex", got, want), assert_columns(colop + " apply_ex", y, np.einsum("eij,ej->ei", want, x)))
    print("colop_ex %s (f2 %s) on %s: blocks %.2e apply %.2e" % ((colop, k2, case.label) + errs))


def test_diag_theta_up_and_temp_forcing(hs_case):
    """diagTheta_up and AssembleTempForcing_HS on every column of the one-patch shapes, at the project's 1e-10.  The velocities shift the
    departure points by 0.3 of the smallest GLL sub-cell (Case.uh): with test_gpu_column._uh's 0.3 of the whole element the upwinded VA2
    has blocks of cond 4e9 ... 7e14 at orders 5 and 6 and the oracle's own solve is 5e-10 / 2e-6 off an extended-precision solution of its
    system, so it could not referee 1e-10 (a first version of this test did that and measured device vs oracle 1.1e-9 / 1.0e-9 / 1.3e-6 /
    4.4e-6 on S1 p5 nk4, p5 nk5, p6 nk4, p6 nk5, with the device 6.2e-10 and the oracle 4.8e-10 off the extended-precision solution at
    p5 nk4).  tests/test_column_cases_cpu.py holds the inputs to: oracle within 1e-12 of the extended-precision solution, cond < 1e8.  At
    orders 5 and 6 the oracle's and the device's distance from that solution are printed before anything is asserted."""
    case = hs_case
    eng, P, nk, n2 = case.eng, case.P0, case.nk, case.n2e
    F = case.fields()
    r = np.random.default_rng(21)
    dt = 60.0
    uh = case.uh(r, dt)
    t = eng.tensor
    th = eng.diag_theta_up(dt, t(F["rho"]), t(F["rt"]), t(uh)).cpu().numpy()
    lat = case.latitudes()                                            # the sphere's own; on the box seeded, and written into the oracle patch
    # Exner pressures cp*sigma^(R/cp) as column 2-forms: value * area * thickness, so that sigma > 0.7 and < 0.7 both occur
    area = P.det.mean() * 4.0 / n2
    sig = np.linspace(1.0, 0.3, nk)[None, :, None] * r.uniform(0.97, 1.0, (case.nEl, 1, n2))
    exner = (1004.5 * sig ** (287.0 / 1004.5) * area * P.thick.mean(axis=1)[None, :, None]).reshape(case.nEl, -1)
    got = eng.temp_forcing_hs(t(lat), t(exner), t(F["theta"]), t(F["rho"])).cpu().numpy()
    want_th = _per_column(case, lambda P, ex, ey, e: P.diag_theta_up(ex, ey, dt, F["rho"][e], F["rt"][e], uh))
    want_tf = _per_column(case, lambda P, ex, ey, e: P.temp_forcing_hs(ex, ey, exner[e], F["theta"][e], F["rho"][e]))
    if case.pn >= 5:                                                  # the oracle's own error beside the device's, before anything is asserted
        from tests.helpers import _rel_ld, ld_solve
        for e in range(case.nEl):
            Pe, ex, ey = case.col(e)
            A = Pe.colop_dense_ex("LINEAR_RHO2_UP", ex, ey, param=dt, f1=F["rho"][e], uh=uh)
            b = Pe.colop_dense_ex("LINCON2_UP", ex, ey, param=dt, uh=uh) @ F["rt"][e]
            x = ld_solve(A, b)
            cond = max(np.linalg.cond(A[k * n2:(k + 1) * n2, k * n2:(k + 1) * n2]) for k in range(nk + 1))
            print("diag_theta_up on %s column %d: cond of the worst VA2_up block %.2e; device vs oracle %.3e, oracle vs extended precision "
                  "%.3e, device vs extended precision %.3e" % (case.label, e, cond, rel_l2(th[e], want_th[e]), _rel_ld(want_th[e], x), _rel_ld(th[e], x)))
    errs = (assert_columns("temp_forcing_hs", got, want_tf), assert_columns("diag_theta_up", th, want_th))[::-1]
    print("diag_theta_up / temp_forcing_hs on %s: %.2e %.2e" % ((case.label,) + errs))
