"""GPU parity for the vertical (column) operators and the column Schur solve, rows C1..C9."""
import numpy as np
import torch
import pytest

from tests.helpers import dense_from_band, make_patch, rel_l2, solve_error_budget

pytestmark = pytest.mark.gpu
TOL = 1e-10
HARD = 1e-9       # unconditional ceiling beside the conditioning-aware budget of the Schur solves (round-4 verdict: a budget alone floats)


@pytest.fixture(scope="module", params=[(3, 2, 6, 1, 6), (4, 1, 6, 0, 5), (2, 2, 6, 3, 4), (3, 3, 6, 2, 8)], ids=lambda p: "p%d_ne%d_np%d_pi%d_nk%d" % p)
def setup(request, oracle):
    from mimsem_amd.device import DeviceMesh, Engine
    pn, ne, nprocs, pi, nk = request.param
    cs, topo, geom, P, rng = make_patch(oracle, pn, ne, nprocs, pi, nk=nk, seed=7 * pn + nk)
    eng = Engine(DeviceMesh([topo], [geom], nk=nk, numbering="local"))
    return eng, P


def _col_fields(P, seed=3):
    """physically scaled column fields: 2-form dofs are cell integrals ~ value * det * thick"""
    r = np.random.default_rng(seed)
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    area = P.det.mean() * 4.0 / n2              # ~ dof scale of a unit density (sum_q w_q = 4)
    dz = P.thick.mean()
    lev = lambda nl, lo, hi: r.uniform(lo, hi, (nEl, nl * n2)) * area * dz
    return dict(rho=lev(nk, 0.5, 1.2), rt=lev(nk, 250.0, 400.0), theta=lev(nk + 1, 280.0, 320.0) / dz,
                pi=lev(nk, 700.0, 1000.0), eta=lev(nk, 5.0, 6.0), velz=lev(nk - 1, -1.0, 1.0) / dz,
                thetaL=lev(nk, 280.0, 320.0))


def _dense_from_blocks(P, colop, blk):
    """stored blocks of one column -> dense matrix in the oracle's layout"""
    nk, n2 = P.nk, P.n2e
    rows, cols = P.colop_dims(colop)
    M = np.zeros((rows, cols))
    nb = blk.shape[0]
    if colop in ("LINCON", "LINCON2", "LINCON2_UP", "CONLIN", "CONLIN_W", "CONLIN_RHODPI"):
        off = 0 if colop == "LINCON" else -1
        for r in range(nb // 2):
            for w in range(2):
                c = r + off + w
                if 0 <= c < cols // n2 and r < rows // n2:
                    M[r*n2:(r+1)*n2, c*n2:(c+1)*n2] = blk[2*r + w]
    else:
        for r in range(nb):
            M[r*n2:(r+1)*n2, r*n2:(r+1)*n2] = blk[r]
    return M


COLCASES = [("CONST", None, None, 0), ("CONST_INV", None, None, 0), ("CONST_RHO", "rho", None, 0), ("CONST_RHO_INV", "rho", None, 0),
            ("CONST_THETA", "theta", None, 0), ("EOS_BLOCK", "rt", None, 0), ("LINEAR", None, None, 0), ("LINEAR_INV", None, None, 0),
            ("LINEAR_RT", "rt", None, 1), ("LINEAR_RT", "rt", None, 0), ("LINEAR_THETA", "theta", None, 0), ("LINEAR_RHO2", "rho", None, 0),
            ("RAYLEIGH", None, None, 0), ("LINCON", None, None, 0), ("LINCON2", None, None, 0), ("CONLIN", None, None, 0),
            ("CONLIN_W", "velz", None, 0), ("CONLIN_RHODPI", "thetaL", "velz", 0)]


@pytest.mark.parametrize("colop,k1,k2,flag", COLCASES, ids=[f"{c[0]}_{c[3]}" for c in COLCASES])
def test_colop_blocks_and_apply(setup, colop, k1, k2, flag):
    eng, P = setup
    F = _col_fields(P)
    f1 = F[k1] if k1 else None; f2 = F[k2] if k2 else None
    t = lambda a: eng.tensor(a) if a is not None else None
    blk = eng.colop_blocks(colop, f1=t(f1), f2=t(f2), flags=flag).cpu().numpy()
    rows, cols = P.colop_dims(colop)
    r = np.random.default_rng(5)
    x = r.standard_normal((P.nEl, cols)); xt = r.standard_normal((P.nEl, rows))
    y = eng.colop_apply(colop, eng.tensor(x), f1=t(f1), f2=t(f2), flags=flag, nout_slots=rows // P.n2e).cpu().numpy()
    yt = eng.colop_apply(colop, eng.tensor(xt), f1=t(f1), f2=t(f2), flags=flag, transpose=True, nout_slots=cols // P.n2e).cpu().numpy()
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        want = P.colop_dense(colop, ex, ey, flag=flag, f1=None if f1 is None else f1[e], f2=None if f2 is None else f2[e])
        got = _dense_from_blocks(P, colop, blk[e])
        assert rel_l2(got, want) < TOL, colop
        assert rel_l2(y[e], want @ x[e]) < TOL, colop
        assert rel_l2(yt[e], want.T @ xt[e]) < TOL, colop


def test_l2_transpose_roundtrip_and_layout(setup):
    import torch
    eng, P = setup
    vh = np.random.default_rng(1).standard_normal((P.nk, P.n2))
    vz = eng.l2_horiz_to_vert(eng.tensor(vh))
    assert np.array_equal(vz.cpu().numpy(), P.horiz_to_vert(vh))            # pure data movement: bit-exact
    back = eng.l2_vert_to_horiz(vz, P.nk)
    assert torch.equal(back, eng.tensor(vh))                                # VertToHoriz o HorizToVert = id


def test_eos_vectors(setup):
    eng, P = setup
    F = _col_fields(P)
    t = eng.tensor
    got = [eng.column_eos(0, t(F["rt"]), t(F["pi"])), eng.column_eos(1, t(F["rt"]), None, 1004.5 * (287.0 / 1e5) ** (287.0 / 717.5), 287.0 / 717.5),
           eng.column_eos(2, t(F["thetaL"]), None), eng.column_eos(2, t(F["thetaL"]), t(F["eta"])), eng.column_eos(3, t(F["rho"]), t(F["eta"] * 1e-3))]
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        want = [P.eos_residual(ex, ey, F["rt"][e], F["pi"][e]),
                P.eos_rhs(ex, ey, F["rt"][e], 1004.5 * (287.0 / 1e5) ** (287.0 / 717.5), 287.0 / 717.5),
                P.const_log_theta_plus_eta(ex, ey, F["thetaL"][e]), P.const_log_theta_plus_eta(ex, ey, F["thetaL"][e], F["eta"][e]),
                P.const_rho_exp_eta(ex, ey, F["rho"][e], F["eta"][e] * 1e-3)]
        for g, w in zip(got, want):
            assert rel_l2(g[e].cpu().numpy(), w) < TOL


def test_diag_theta(setup):
    eng, P = setup
    F = _col_fields(P)
    th0 = eng.diag_theta(0, eng.tensor(F["rho"]), eng.tensor(F["rt"])).cpu().numpy()
    th1 = eng.diag_theta(1, eng.tensor(F["rho"]), eng.tensor(F["rt"])).cpu().numpy()
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        assert rel_l2(th0[e], P.diag_theta_L2(ex, ey, F["rho"][e], F["rt"][e])) < TOL
        assert rel_l2(th1[e], P.diag_theta2(ex, ey, F["rho"][e], F["rt"][e])) < TOL


def test_schur_column_solve(setup):
    """solve_schur_column_eta: analytically assembled block-tridiagonal L_pi + block Thomas vs the oracle's dense
    restatement of the reference's MatMatMult chain + LU (eul/VertSolve.cpp:677-823)"""
    eng, P = setup
    F = _col_fields(P)
    r = np.random.default_rng(9)
    nEl, N, Nm = P.nEl, P.nk * P.n2e, (P.nk - 1) * P.n2e
    dt = 75.0
    Fu, Frho, Feta, Fpi = (r.standard_normal((nEl, n)) * 1e8 for n in (Nm, N, N, N))
    t = eng.tensor
    L = eng.helmholtz_blocks(dt, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"])).cpu().numpy()
    dFu, dFrho, dFeta, dFpi = t(Fu), t(Frho), t(Feta), t(Fpi)
    d_u, d_rho, d_eta, d_pi = eng.solve_schur_eta(dt, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]), dFu, dFrho, dFeta, dFpi)
    n2, nk = P.n2e, P.nk
    for e in range(nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        ref = P.solve_schur_column_eta(ex, ey, dt, F["thetaL"][e], F["rho"][e], F["eta"][e], F["pi"][e], Fu[e], Frho[e], Feta[e], Fpi[e])
        Ld = dense_from_band(L[e], nk, n2, lo=1)
        # the operator itself (incl. exact zeros outside the three block diagonals of the reference's product)
        assert rel_l2(Ld, ref["L_pi"]) < TOL
        # error budget against an extended-precision solve of each side's own system (tests/helpers.py): the device sweep is held
        # to 1e-10 on ITS system; the two solutions may differ by cond(L_pi) x the round-off difference of the two operators
        b = solve_error_budget(Ld, dFpi[e].cpu().numpy(), d_pi[e].cpu().numpy(), ref["L_pi"], ref["F_pi"], ref["d_pi"])
        assert b["hip_vs_own_system"] < TOL, b
        bound = max(TOL, 4.0 * b["diff_of_exact_solutions"] + b["hip_vs_own_system"] + b["oracle_vs_own_system"])
        assert b["diff"] < bound, b
        assert b["diff"] < HARD, b                                      # the budget explains a difference, it does not license any: hard ceiling
        for name, got in (("d_u", d_u), ("d_eta", d_eta), ("d_rho", d_rho), ("F_u", dFu), ("F_rho", dFrho), ("F_eta", dFeta), ("F_pi", dFpi)):
            assert rel_l2(got[e].cpu().numpy(), ref[name]) < min(max(TOL, 50.0 * bound), 50.0 * HARD), (name, b)


def test_two_sided_thomas_sweep_equals_the_one_sided(setup):
    """Round 3: for even nk the Helmholtz system is solved by the two-sided (twisted) block-Thomas sweep -- top and bottom halves of a
    column in two DPP rows at once -- instead of the one-sided chain (MIMSEM_THOMAS2=0): same system, same refinement rule, solutions
    equal to the round-off the conditioning allows, identical status"""
    import os
    eng, P = setup
    if P.nk % 2 or P.nk < 4 or P.n2e > 16:
        pytest.skip("two-sided sweep: even nk >= 4, orders <= 4")
    F = _col_fields(P)
    r = np.random.default_rng(21)
    nEl, N, Nm = P.nEl, P.nk * P.n2e, (P.nk - 1) * P.n2e
    rhs = [r.standard_normal((nEl, n)) * 1e8 for n in (Nm, N, N, N)]
    t = eng.tensor
    args = lambda: (75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]), *[t(x) for x in rhs])
    two = eng.solve_schur_eta(*args()); st2 = eng.solve_status()
    os.environ["MIMSEM_THOMAS2"] = "0"
    try:
        one = eng.solve_schur_eta(*args()); st1 = eng.solve_status()
    finally:
        del os.environ["MIMSEM_THOMAS2"]
    assert st1[0] == 0 and st2[0] == 0 and (st1[1] == 0).all() and (st2[1] == 0).all() and st2[2].max() <= 1e-10
    for a, b, name in zip(two, one, ("d_u", "d_rho", "d_eta", "d_pi")):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < TOL, name


@pytest.mark.parametrize("nk,pn", [(4, 3), (8, 3), (10, 3), (14, 3), (16, 3), (22, 3), (8, 4), (10, 4)],
                         ids=lambda v: str(v))
def test_two_sided_thomas_sweep_at_other_level_counts(oracle, nk, pn):
    """the rotating prefetch / batched loads of k_thomas_dpp2 with half-lengths m = nk/2 that are not multiples of its batch sizes (3, 4):
    two-sided against one-sided on the same columns, and the residual of the block-tridiagonal system itself"""
    import os
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    cs, topo, geom, P, rng = make_patch(oracle, pn, 2 if pn == 3 else 1, 6, 1, nk=nk, seed=100 + nk)
    eng = Engine(DeviceMesh([topo], [geom], nk=nk, numbering="local"))
    F = _col_fields(P, seed=nk)
    r = np.random.default_rng(nk)
    nEl, n2 = P.nEl, P.n2e
    rhs = [r.standard_normal((nEl, n * n2)) * 1e8 for n in (nk - 1, nk, nk, nk)]
    t = eng.tensor
    args = lambda: (75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]), *[t(x) for x in rhs])
    a2 = args(); two = eng.solve_schur_eta(*a2); st2 = eng.solve_status()
    os.environ["MIMSEM_THOMAS2"] = "0"
    try:
        one = eng.solve_schur_eta(*args()); st1 = eng.solve_status()
    finally:
        del os.environ["MIMSEM_THOMAS2"]
    assert st1[0] == 0 and st2[0] == 0
    for a, b, name in zip(two, one, ("d_u", "d_rho", "d_eta", "d_pi")):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < TOL, (name, nk)
    L = eng.helmholtz_blocks(75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"])).view(nEl, nk, 3, n2, n2)
    d = two[3].view(nEl, nk, n2); f = a2[8].view(nEl, nk, n2)                 # F_pi after the in-place update = the solve's right-hand side
    Ld = torch.einsum("ekij,ekj->eki", L[:, :, 1], d)
    Ld[:, 1:] += torch.einsum("ekij,ekj->eki", L[:, 1:, 0], d[:, :-1])
    Ld[:, :-1] += torch.einsum("ekij,ekj->eki", L[:, :-1, 2], d[:, 1:])
    Ln = torch.sqrt((L * L).sum(dim=(1, 2, 3, 4)))
    bwd = torch.linalg.vector_norm(Ld - f, dim=(1, 2)) / (Ln * torch.linalg.vector_norm(d, dim=(1, 2)) + torch.linalg.vector_norm(f, dim=(1, 2)))
    assert float(bwd.max()) < 1e-13, (nk, float(bwd.max()))


def test_residual_compositions(setup):
    """C8: diagnose_F_z / diagnose_Phi_z / assemble_residual_ec (eul/VertSolve.cpp:237-286, 432-502) issued for all
    columns through the ABI vs the same chain written with the oracle's dense column matrices"""
    from mimsem_amd.vertsolve import RAYLEIGH, VertSolve
    eng, P = setup
    if P.nk < 4:
        pytest.skip("Rayleigh layer needs nk >= 4")
    F = _col_fields(P)
    r = np.random.default_rng(13)
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    velz1, velz2 = F["velz"], F["velz"] * (1.0 + 0.1 * r.standard_normal(F["velz"].shape))
    rho1, rho2 = F["rho"], F["rho"] * (1.0 + 0.01 * r.standard_normal(F["rho"].shape))
    theta, Pi = F["thetaL"], F["pi"]
    zv = r.standard_normal((nEl, nk * n2)) * 1e8
    dt = 75.0
    t = eng.tensor
    vs = VertSolve(eng, dt)
    fw, Fz, G, ftc = vs.assemble_residual_ec(t(theta), t(Pi), t(velz1), t(velz2), t(rho1), t(rho2), t(zv))
    N, Nm = nk * n2, (nk - 1) * n2
    V10 = np.zeros((N, Nm))
    for k in range(nk):
        for i in range(n2):
            if k > 0: V10[k*n2+i, (k-1)*n2+i] = -1.0
            if k < nk - 1: V10[k*n2+i, k*n2+i] = +1.0
    V01 = -V10.T
    for e in range(nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        D = lambda op, **kw: P.colop_dense(op, ex, ey, **kw)
        VAinv = D("LINEAR_INV")
        F_ref = VAinv @ D("LINEAR_RT", flag=1, f1=rho1[e]) @ (velz1[e] / 3 + velz2[e] / 6) + \
            VAinv @ D("LINEAR_RT", flag=1, f1=rho2[e]) @ (velz1[e] / 6 + velz2[e] / 3)
        W1, W2 = D("CONLIN_W", f1=velz1[e]), D("CONLIN_W", f1=velz2[e])
        Phi = (W1 @ velz1[e] + W1 @ velz2[e] + W2 @ velz2[e]) / 6 + zv[e]
        VA, VB = D("LINEAR"), D("CONST")
        fw_ref = VA @ velz2[e] - VA @ velz1[e] + dt * V01 @ Phi
        tA2 = VAinv @ (V01 @ (VB @ Pi[e]))
        VAt = D("LINEAR_RT", flag=1, f1=theta[e])
        tA1 = VAt @ tA2
        fw_ref += 0.5 * dt * tA1
        G_ref = VAinv @ (VAt @ F_ref)
        VR = D("RAYLEIGH")
        fw_ref += 0.5 * dt * RAYLEIGH * (VR @ velz2[e] + VR @ velz1[e])
        tA2 = VAinv @ (V01 @ (VB @ theta[e]))
        VBr = D("CONST_RHO", f1=theta[e]); VBA = D("CONLIN_W", f1=tA2)
        fw_ref += 0.5 * dt * V01 @ (VBr @ Pi[e]) - 0.5 * dt * VBA.T @ Pi[e]
        ftc_ref = 0.5 * dt * VBr @ (V10 @ F_ref) + 0.5 * dt * VBA @ F_ref
        assert rel_l2(Fz[e].cpu().numpy(), F_ref) < TOL
        assert rel_l2(G[e].cpu().numpy(), G_ref) < TOL
        assert rel_l2(fw[e].cpu().numpy(), fw_ref) < TOL
        assert rel_l2(ftc[e].cpu().numpy(), ftc_ref) < TOL


def _uh(P, r, dt):
    """horizontal velocities [nk][n1] whose departure shift is ~0.3 of the reference element"""
    vs = P.det.mean() / P.thickInv.mean(axis=1) * 0.3 / dt            # per level: the stretched grid's thickness varies a lot
    return r.uniform(-1, 1, (P.nk, P.n1)) * vs[:, None]


HSCASES = [("LINEAR_RAYLEIGH_INV", None, None, 3.7e-2, False), ("EOS_BLOCK_INV", "pi", None, 0.0, False),
           ("EOS_BLOCK_INV", "pi", "theta", 0.0, False), ("LINEAR_RHO2_UP", "rho", None, 75.0, True), ("LINCON2_UP", None, None, 75.0, True)]


@pytest.mark.parametrize("colop,k1,k2,param,up", HSCASES, ids=[f"{c[0]}_{c[2]}" for c in HSCASES])
def test_hs_colops(setup, colop, k1, k2, param, up):
    """C2-C4 remainder: AssembleLinearWithRayleighInv, Assemble_EOS_BlockInv, AssembleLinearWithRho2_up, AssembleLinCon2_up"""
    eng, P = setup
    if up and P.n > 7:
        pytest.skip("edge-function scratch sized for p <= 7")
    F = _col_fields(P)
    r = np.random.default_rng(15)
    f1 = F[k1] if k1 else None; f2 = F[k2] if k2 else None
    uh = _uh(P, r, param) if up else None
    t = lambda a: eng.tensor(a) if a is not None else None
    blk = eng.colop_blocks_ex(colop, param=param, f1=t(f1), f2=t(f2), uh=t(uh)).cpu().numpy()
    rows, cols = P.colop_dims(colop)
    x = r.standard_normal((P.nEl, cols))
    y = eng.colop_apply_ex(colop, eng.tensor(x), rows // P.n2e, param=param, f1=t(f1), f2=t(f2), uh=t(uh)).cpu().numpy()
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        want = P.colop_dense_ex(colop, ex, ey, param=param, f1=None if f1 is None else f1[e], f2=None if f2 is None else f2[e], uh=uh)
        got = _dense_from_blocks(P, colop, blk[e])
        assert rel_l2(got, want) < TOL, colop
        assert rel_l2(y[e], want @ x[e]) < TOL, colop


def test_diag_theta_up_and_temp_forcing(setup):
    """C6 diagTheta_up (eul/VertSolve.cpp:354-384) and AssembleTempForcing_HS (eul/VertOps.cpp:1563-1633)"""
    eng, P = setup
    F = _col_fields(P)
    r = np.random.default_rng(21)
    dt = 60.0
    uh = _uh(P, r, dt)
    t = eng.tensor
    th = eng.diag_theta_up(dt, t(F["rho"]), t(F["rt"]), t(uh)).cpu().numpy()
    iq = P.elinds("q")
    lat = np.ascontiguousarray(P.sq[:, 1][iq])                        # Geom::s[elInds0_l][1]
    # Exner pressures cp*sigma^(R/cp) as column 2-forms: value * area * thickness, so that sigma > 0.7 and < 0.7 both occur
    area = P.det.mean() * 4.0 / P.n2e
    sig = np.linspace(1.0, 0.3, P.nk)[None, :, None] * r.uniform(0.97, 1.0, (P.nEl, 1, P.n2e))
    exner = (1004.5 * sig ** (287.0 / 1004.5) * area * P.thick.mean(axis=1)[None, :, None]).reshape(P.nEl, -1)
    got = eng.temp_forcing_hs(t(lat), t(exner), t(F["theta"]), t(F["rho"])).cpu().numpy()
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        assert rel_l2(th[e], P.diag_theta_up(ex, ey, dt, F["rho"][e], F["rt"][e], uh)) < TOL
        assert rel_l2(got[e], P.temp_forcing_hs(ex, ey, exner[e], F["theta"][e], F["rho"][e])) < TOL


@pytest.mark.parametrize("flags", [0, 3], ids=["eul", "box"])
def test_schur_column_3_pentadiagonal(setup, flags):
    """solve_schur_column_3 (eul/VertSolve.cpp:504-675): banded assembly of the block-pentadiagonal L_rt_rt, 2x2 super-block
    Thomas solve and back substitution vs the oracle's dense restatement of the MatMatMult chain + LU"""
    eng, P = setup
    F = _col_fields(P)
    r = np.random.default_rng(29)
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    N, Nm = nk * n2, (nk - 1) * n2
    dt = 75.0
    Fu, Frho, Frt, Fpi = (r.standard_normal((nEl, n)) * 1e8 for n in (Nm, N, N, N))
    t = eng.tensor
    dFu, dFrho, dFrt, dFpi = t(Fu), t(Frho), t(Frt), t(Fpi)
    d_u, d_rho, d_rt, d_pi, L = eng.solve_schur_3(dt, t(F["theta"]), t(F["velz"]), t(F["rho"]), t(F["rt"]), t(F["pi"]),
                                                  dFu, dFrho, dFrt, dFpi, want_L=True, flags=flags)
    L = L.cpu().numpy()
    for e in range(nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        ref = P.solve_schur_column_3(ex, ey, dt, F["theta"][e], F["velz"][e], F["rho"][e], F["rt"][e], F["pi"][e],
                                     Fu[e], Frho[e], Frt[e], Fpi[e], flags=flags)
        Ld = dense_from_band(L[e], nk, n2, lo=2)
        assert rel_l2(Ld, ref["L"]) < TOL                       # incl. exact zeros outside the five block diagonals
        b = solve_error_budget(Ld, dFrt[e].cpu().numpy(), d_rt[e].cpu().numpy(), ref["L"], ref["F_rt"], ref["d_rt"])
        assert b["hip_vs_own_system"] < TOL, b
        bound = max(TOL, 4.0 * b["diff_of_exact_solutions"] + b["hip_vs_own_system"] + b["oracle_vs_own_system"])
        assert b["diff"] < bound, b
        assert b["diff"] < HARD, b
        for name, got in (("d_u", d_u), ("d_pi", d_pi), ("d_rho", d_rho), ("F_u", dFu), ("F_rho", dFrho), ("F_rt", dFrt), ("F_pi", dFpi)):
            assert rel_l2(got[e].cpu().numpy(), ref[name]) < min(max(TOL, 50.0 * bound), 50.0 * HARD), (name, b)


def test_vertical_incidence(setup):
    """C1 VertOps::vertOps (eul/VertOps.cpp:134-182): V10, V01 = -V10^T, V10_full as bit-exact +-1 stencils"""
    eng, P = setup
    nk, n2, nEl = P.nk, P.n2e, P.nEl
    V10 = np.zeros((nk * n2, (nk - 1) * n2)); V10f = np.zeros((nk * n2, (nk + 1) * n2))
    for k in range(nk):
        for i in range(n2):
            if k > 0: V10[k*n2+i, (k-1)*n2+i] = -1.0
            if k < nk - 1: V10[k*n2+i, k*n2+i] = +1.0
            V10f[k*n2+i, k*n2+i] = -1.0; V10f[k*n2+i, (k+1)*n2+i] = +1.0
    r = np.random.default_rng(2)
    xm, xk, xp = (r.integers(-50, 50, (nEl, m * n2)).astype(np.float64) for m in (nk - 1, nk, nk + 1))
    assert np.array_equal(eng.column_incidence("V10", eng.tensor(xm)).cpu().numpy(), xm @ V10.T)
    assert np.array_equal(eng.column_incidence("V01", eng.tensor(xk)).cpu().numpy(), xk @ (-V10))
    assert np.array_equal(eng.column_incidence("V10_full", eng.tensor(xp)).cpu().numpy(), xp @ V10f.T)


@pytest.mark.parametrize("mode", ["rows", "wave", "0"])
def test_fused_schur_assembly_matches_default(setup, monkeypatch, mode):
    """the fused assembly of the Schur factors -- row-per-lane (16 lanes per (column, level) / (column, interface) task) or the
    earlier one-wave-per-task kernels -- and the unfused pipeline ("0") give the same Helmholtz operator and solution"""
    eng, P = setup
    if P.n2e not in (4, 9, 16):
        pytest.skip("fused kernels are built for 2x2, 3x3, 4x4 blocks")
    F = _col_fields(P)
    r = np.random.default_rng(9)
    nEl, N, Nm = P.nEl, P.nk * P.n2e, (P.nk - 1) * P.n2e
    Fs = [r.standard_normal((nEl, n)) * 1e8 for n in (Nm, N, N, N)]
    t = eng.tensor
    args = (75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]))
    base = eng.solve_schur_eta(*args, *[t(f) for f in Fs])
    L0 = eng.helmholtz_blocks(*args)
    monkeypatch.setenv("MIMSEM_SCHUR_FUSED", mode)
    alt = eng.solve_schur_eta(*args, *[t(f) for f in Fs])
    L1 = eng.helmholtz_blocks(*args)
    assert rel_l2(L1.cpu().numpy(), L0.cpu().numpy()) < TOL
    for a, b in zip(alt, base):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < TOL


@pytest.mark.parametrize("var", ["MIMSEM_THOMAS_WAVE", "MIMSEM_THOMAS_WG", "MIMSEM_EOS_WIDE", "MIMSEM_BAND_NAIVE"])
def test_selectable_kernel_variants_agree(setup, monkeypatch, var):
    """every kernel alternative behind an environment switch gives the default result: block-Thomas per wave / per
    workgroup, the wide EOS pipeline, the entry-per-thread band product"""
    eng, P = setup
    if P.nk < 4:
        pytest.skip("solve_schur_column_3 needs nk >= 4")
    F = _col_fields(P)
    r = np.random.default_rng(19)
    nEl, N, Nm = P.nEl, P.nk * P.n2e, (P.nk - 1) * P.n2e
    Fs = [r.standard_normal((nEl, n)) * 1e8 for n in (Nm, N, N, N)]
    t = eng.tensor
    a_eta = (75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]))
    a_3 = (75.0, t(F["theta"]), t(F["velz"]), t(F["rho"]), t(F["rt"]), t(F["pi"]))
    base_eta = eng.solve_schur_eta(*a_eta, *[t(f) for f in Fs])
    base_3 = eng.solve_schur_3(*a_3, *[t(f) for f in Fs])
    monkeypatch.setenv(var, "1")
    alt_eta = eng.solve_schur_eta(*a_eta, *[t(f) for f in Fs])
    alt_3 = eng.solve_schur_3(*a_3, *[t(f) for f in Fs])
    for a, b in list(zip(alt_eta, base_eta)) + list(zip(alt_3, base_3)):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < TOL, var


def _newton_start(eng, P, vs, seed=29):
    """the start state of the vertical Newton loop tests: zv from VertSolve::initGZ (device and formula), an EOS-consistent column at rest
    plus 1e-4 perturbations, the latitudes of the quadrature points and a small u dw/dx term"""
    from mimsem_amd.vertsolve import SCALE as VSCALE
    r = np.random.default_rng(seed)
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    levs = eng.mesh.geoms[0].levs
    zv_d = vs.init_gz(levs)
    W, Q = P.arr("W", (P.mp12, n2)), P.arr("Q", (P.mp12,))
    inds0 = eng.mesh.geoms[0].all_inds0_l()
    zv = np.zeros((nEl, nk * n2))
    for e in range(nEl):
        for k in range(nk):
            gz = 9.80616 * (levs[k, inds0[e]] + levs[k + 1, inds0[e]])
            zv[e, k * n2:(k + 1) * n2] = W.T @ (VSCALE * 0.5 * Q * gz)
    # an EOS-consistent column at rest plus small perturbations: Newton steps stay in the physical range of log / exp / pow.  A
    # constant value v is the 2-form with DoF_j = v * (area of sub-cell j) * det * thickness (the edge functions histopolate)
    wd = np.diff(P.arr("qx", (P.mp1,)))
    wj = np.outer(wd, wd).ravel()
    detm = P.det.mean(axis=1)
    thm = np.stack([[P.thick[k, inds0[e]].mean() for k in range(nk)] for e in range(nEl)])
    rho_v, th_v = np.linspace(1.2, 0.5, nk), np.linspace(290.0, 330.0, nk)
    pi_v = 1004.5 * (287.0 * rho_v * th_v / 1.0e5) ** (287.0 / 717.5)

    def col(v):
        out = np.zeros((nEl, nk * n2))
        for e in range(nEl):
            for k in range(nk):
                out[e, k * n2:(k + 1) * n2] = v[k] * wj * detm[e] * thm[e, k]
        return out
    pert = lambda: 1.0 + 1e-4 * r.standard_normal((nEl, nk * n2))
    rho, rt, exner = col(rho_v) * pert(), col(rho_v * th_v) * pert(), col(pi_v) * pert()
    velz = np.zeros((nEl, (nk - 1) * n2))
    lat = np.ascontiguousarray(P.sq[:, 1][P.elinds("q")])              # Geom::s[elInds0_l][1]: latitude of the quadrature points
    udwdx = 1e-3 * r.standard_normal((nEl, (nk - 1) * n2)) * float(np.abs(zv).mean()) / 9.80616 / 1.5e4
    return dict(zv_d=zv_d, zv=zv, velz=velz, rho=rho, rt=rt, exner=exner, lat=lat, udwdx=udwdx)


def test_vertical_newton_loop_matches_oracle(setup):
    """the caller of the column path: VertSolve::solve_schur_eta (eul/VertSolve.cpp:1721-1973) for all columns at once
    (mimsem_amd/vertsolve.py) against the column-by-column numpy restatement oracle/vert_oracle.py -- three Newton iterations,
    no horizontal wind; state and max-norm history.  Also VertSolve::initGZ (:89-175) against its formula."""
    from mimsem_amd.vertsolve import VertSolve
    from oracle import vert_oracle
    eng, P = setup
    if P.nk < 4:
        pytest.skip("Rayleigh layer needs nk >= 4")
    dt = 0.5
    t = eng.tensor
    vs = VertSolve(eng, dt)
    S = _newton_start(eng, P, vs)
    zv_d, zv, velz, rho, rt, exner, udwdx = (S[k] for k in ("zv_d", "zv", "velz", "rho", "rt", "exner", "udwdx"))
    assert rel_l2(zv_d.cpu().numpy(), zv) < 1e-13
    got = vs.solve_schur_eta(t(velz), t(rho), t(rt), t(exner), zv_d, maxit=3, tol=0.0)
    want = vert_oracle.solve_schur_eta(P, dt, velz, rho, rt, exner, zv, 3)
    for a, b, name in zip(got, want[:4], ("velz", "rho", "rt", "exner")):
        assert np.all(np.isfinite(b)), name
        assert rel_l2(a.cpu().numpy(), b) < TOL, name
    for hd, ho in zip(vs.history, want[4]):
        for k in ("exner", "w", "rho", "eta"):
            assert abs(hd[k] - ho[k]) <= 1e-5 * ho[k] + 1e-15, (k, hd[k], ho[k])
    # with the Held-Suarez temperature forcing and the u dw/dx term switched on
    got = vs.solve_schur_eta(t(velz), t(rho), t(rt), t(exner), zv_d, maxit=2, tol=0.0, hs_lat=t(S["lat"]), udwdx=t(udwdx))
    want = vert_oracle.solve_schur_eta(P, dt, velz, rho, rt, exner, zv, 2, hs_forcing=True, udwdx=udwdx)
    for a, b, name in zip(got, want[:4], ("velz", "rho", "rt", "exner")):
        assert np.all(np.isfinite(b)) and rel_l2(a.cpu().numpy(), b) < TOL, name


@pytest.mark.parametrize("pn,ne,nk", [(3, 2, 5), (2, 2, 4), (4, 1, 6), (5, 1, 4)], ids=lambda v: str(v))
def test_composed_eta_loop_matches_the_restatement_and_the_fused_loop(oracle, pn, ne, nk):
    """the COMPOSED solve_schur_eta loop (single-operator calls: the only route above order 4, and what MIMSEM_NEWTON_FUSED=0 selects)
    against oracle/vert_oracle.py and, at the orders that have one, against the fused loop: three iterations without forcing, two with
    the Held-Suarez forcing and u dw/dx; state, history and the published theta_h / theta_l2_h / exner_h.  An odd level count, the
    smallest the Rayleigh layer takes, the half-row layout of order 4, and an order with no fused route"""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.vertsolve import VertSolve
    from oracle import vert_oracle
    cs, topo, geom, P, rng = make_patch(oracle, pn, ne, 6, 1, nk=nk, seed=500 + 7 * nk + pn)
    eng = Engine(DeviceMesh([topo], [geom], nk=nk, numbering="local"))
    dt = 0.5
    t = eng.tensor
    vs = VertSolve(eng, dt)
    vs.fused = False
    S = _newton_start(eng, P, vs)
    zv_d, zv, velz, rho, rt, exner, udwdx = (S[k] for k in ("zv_d", "zv", "velz", "rho", "rt", "exner", "udwdx"))
    names = ("velz", "rho", "rt", "exner")
    halves = ("theta_h", "theta_l2_h", "exner_h")
    fz = VertSolve(eng, dt)
    fz.fused = True
    for nits, kw, okw in ((3, {}, {}), (2, dict(hs_lat=t(S["lat"]), udwdx=t(udwdx)), dict(hs_forcing=True, udwdx=udwdx))):
        got = vs.solve_schur_eta(t(velz), t(rho), t(rt), t(exner), zv_d, maxit=nits, tol=0.0, **kw)
        want = vert_oracle.solve_schur_eta(P, dt, velz, rho, rt, exner, zv, nits, **okw)
        assert len(vs.history) == nits
        for a, b, name in zip(got, want[:4], names):
            assert np.all(np.isfinite(b)), name
            assert rel_l2(a.cpu().numpy(), b) < TOL, (name, nits)
        for hd, ho in zip(vs.history, want[4]):
            for k in ("exner", "w", "rho", "eta"):
                assert abs(hd[k] - ho[k]) <= 1e-5 * ho[k] + 1e-15, (k, hd[k], ho[k])
        if pn <= 4:
            fus = fz.solve_schur_eta(t(velz), t(rho), t(rt), t(exner), zv_d, maxit=nits, tol=0.0, **kw)
            for a, b, name in zip(got, fus, names):
                assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < TOL, (name, nits)
            for name in halves:
                assert rel_l2(getattr(vs, name).cpu().numpy(), getattr(fz, name).cpu().numpy()) < TOL, (name, nits)


def test_max_norms_against_the_composed_reduction(setup):
    """mimsem_column_max_norms (VertSolve::MaxNorm, eul/VertSolve.cpp:228, on the squares newton_update leaves) against the torch composition
    it replaced; a NaN ratio wins the maximum, as a comparison on the host would see it"""
    import torch
    eng, P = setup
    r = np.random.default_rng(5)
    nrm = eng.tensor(r.uniform(0.1, 2.0, (8, P.nEl, P.nk * P.n2e)))
    got = eng.max_norms(nrm).cpu().numpy()
    cs = nrm.sum(dim=2)
    want = torch.sqrt(cs[0::2] / cs[1::2]).amax(dim=1).cpu().numpy()
    assert np.allclose(got, want, rtol=1e-13, atol=0.0)
    nrm[2, P.nEl // 2] = float("nan")
    got = eng.max_norms(nrm).cpu().numpy()
    assert np.isnan(got[1]) and np.allclose(got[[0, 2, 3]], want[[0, 2, 3]], rtol=1e-13)


@pytest.mark.parametrize("n", [1, 4, 9, 16, 24, 33, 40, 56, 64, 65])      # (65: past the one-wavefront kernel, thread per block in LDS)
def test_block_inverse_against_the_oracle_inv(oracle, n):
    """A5 as an entry point (mimsem_block_inverse: the PCBJACOBI blocks and WmatInv / the column inverses run through it): the batched
    Gauss-Jordan against the oracle's restatement of LinAlg::Inv (eul/LinAlg.cpp:186-269, pinned bit-for-bit against the compiled
    reference in tests/test_oracle_pins.py) on SPD mass-like blocks, on non-symmetric well-conditioned blocks that need the pivoting
    fall-back, and -- mimsem_block_inverse_status -- with ONE singular block among them: the count comes back instead of being dropped"""
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    cs, topo, geom, P, rng = make_patch(oracle, 2, 1, 6, 0, nk=2, seed=5)
    eng = Engine(DeviceMesh([topo], [geom], nk=2, numbering="local"))
    r = np.random.default_rng(100 + n)
    nb = 37
    G = r.standard_normal((nb, n, n))
    spd = np.einsum("bij,bkj->bik", G, G) + n * np.eye(n)[None]
    gen = r.standard_normal((nb, n, n)) + 0.1 * np.eye(n)[None]           # zero-ish diagonal entries now and then: row pivoting needed
    if n > 1:
        gen[::5, 0, 0] = 0.0
    for name, B in (("spd", spd), ("general", gen)):
        want = np.stack([oracle.inv(b)[0] for b in B])
        got, nsing = eng.block_inverse_status(eng.tensor(B))
        got = got.cpu().numpy()
        assert nsing == 0, (name, nsing)
        cond = np.array([np.linalg.cond(b) for b in B])
        err = np.array([rel_l2(got[i], want[i]) for i in range(nb)])
        assert (err < 1e-10 * np.maximum(1.0, cond / 1e3)).all(), (name, float(err.max()), float(cond.max()))
        assert max(np.abs(got[i] @ B[i] - np.eye(n)).max() for i in range(nb)) < 1e-9 * cond.max()
        if n > 16:
            # round 5: one wavefront per block (k_block_inverse_wave) -- the same pivots, the same operations per entry as the
            # thread-per-block kernel it replaces (MIMSEM_INV_THREAD=1): the same bits
            import os
            os.environ["MIMSEM_INV_THREAD"] = "1"
            try:
                old, _ = eng.block_inverse_status(eng.tensor(B))
            finally:
                del os.environ["MIMSEM_INV_THREAD"]
            assert torch.equal(old.cpu(), torch.as_tensor(got)), name
    if n > 1:
        S = spd.copy()
        S[11, :, -1] = S[11, :, 0]; S[11, -1, :] = S[11, 0, :]             # two equal rows and columns: exactly singular
        _, err = oracle.inv(S[11])
        got, nsing = eng.block_inverse_status(eng.tensor(S))
        assert err != 0 and nsing == 1, (err, nsing)
        ok = [i for i in range(nb) if i != 11]
        want = np.stack([oracle.inv(S[i])[0] for i in ok])
        assert max(rel_l2(got[i].cpu().numpy(), w) for i, w in zip(ok, want)) < 1e-10 * max(1.0, np.linalg.cond(S[ok[0]]) / 1e3)


@pytest.mark.parametrize("pn,ne,nk", [(3, 2, 4), (3, 2, 5), (3, 2, 7), (3, 2, 9), (3, 1, 12), (2, 2, 5), (2, 1, 11), (3, 3, 6), (4, 1, 5), (4, 1, 8), (4, 2, 6), (4, 2, 9), (4, 3, 6)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("flags", [0, 3], ids=["eul", "box"])
def test_fused_schur_3_walk_at_other_level_counts(oracle, pn, ne, nk, flags):
    """Round 4's three-launch solve_schur_column_3 (k_s3_sweep + k_penta_dpp + k_s3_backsub) against round 2's chain + 2 x 2 super-block
    sweep (MIMSEM_SCHUR3_CHAIN=1 MIMSEM_SCHUR3_SUPERBLOCKS=1: itself held to the oracle in test_schur_column_3_pentadiagonal) at level
    counts that are odd (one-sided pentadiagonal elimination), not multiples of anything, and on meshes so small that a column is split
    over several tasks (the walk's warm-up steps, the dump blocks, the peeled last step); bands, every right-hand side, every solution;
    the per-column status is valid and clean after it"""
    import os
    from mimsem_amd.device import DeviceMesh, Engine
    cs, topo, geom, P, rng = make_patch(oracle, pn, ne, 6, 1, nk=nk, seed=300 + 7 * nk + pn)
    eng = Engine(DeviceMesh([topo], [geom], nk=nk, numbering="local"))
    F = _col_fields(P, seed=nk + pn)
    r = np.random.default_rng(41 + nk)
    nEl, n2 = P.nEl, P.n2e
    rhs = [r.standard_normal((nEl, n * n2)) * 1e8 for n in (nk - 1, nk, nk, nk)]
    t = eng.tensor
    run = lambda: eng.solve_schur_3(75.0, t(F["theta"]), t(F["velz"]), t(F["rho"]), t(F["rt"]), t(F["pi"]), *[t(x) for x in rhs],
                                    want_L=True, flags=flags)
    new = run()
    nbad, st, ratio = eng.solve_status()
    assert nbad == 0 and (st == 0).all() and ratio.max() <= 1e-10, (nbad, float(ratio.max()))
    lane_major = eng.solve_schur_3(75.0, t(F["theta"]), t(F["velz"]), t(F["rho"]), t(F["rt"]), t(F["pi"]), *[t(x) for x in rhs], flags=flags)
    again = run()                                                       # run-to-run: the same bits (a spill lost in a divergent region showed here first)
    for a, b in zip(new, again):
        assert torch.equal(a, b)
    os.environ["MIMSEM_SCHUR3_CHAIN"] = "1"
    if pn < 4:
        os.environ["MIMSEM_SCHUR3_SUPERBLOCKS"] = "1"                   # (order 4: the chain's bands + k_penta_dpp, held to the oracle on config 5's columns)
    try:
        old = run()
    finally:
        del os.environ["MIMSEM_SCHUR3_CHAIN"]
        os.environ.pop("MIMSEM_SCHUR3_SUPERBLOCKS", None)
    if pn < 4:
        assert eng.solve_status()[0] == -1                              # the round-2 path keeps no status
    names = ("d_u", "d_rho", "d_rt", "d_pi", "L")
    for a, b, name in zip(new, old, names):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < (1e-12 if name == "L" else TOL), (name, pn, nk)
    # the solve that keeps its bands in the internal lane-major layout (no L_out) gives the same solutions
    for a, b, name in zip(lane_major, new, names[:4]):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-12, name


@pytest.mark.parametrize("pn,ne,nk", [(2, 2, 6), (3, 2, 6), (3, 2, 5), (4, 1, 6)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["eta", "s3_eul", "s3_box"])
def test_pivoted_band_lu_solves_every_column(oracle, pn, ne, nk, kind):
    """Round 4: mimsem_column_set_pivot_fallback(2) sends EVERY column of solve_schur_column_eta / _3 through the unblocked band LU with
    partial pivoting of column_pivot.inc (what the reference's PCLU does, eul/VertSolve.cpp:645-653, :806-812) instead of the unpivoted
    block sweep: status 3 for all columns, each solution held to an extended-precision pivoted solve of the bands the call returns, and
    every output of the call equal to the default path's up to the conditioning; switching the mode off restores the default bit for bit"""
    from mimsem_amd.device import DeviceMesh, Engine
    from tests.helpers import _ld_lu_solve
    cs, topo, geom, P, rng = make_patch(oracle, pn, ne, 6, 1, nk=nk, seed=500 + 11 * nk + pn)
    eng = Engine(DeviceMesh([topo], [geom], nk=nk, numbering="local"))
    F = _col_fields(P, seed=2 * nk + pn)
    r = np.random.default_rng(17 + nk)
    nEl, n2 = P.nEl, P.n2e
    rhs = [r.standard_normal((nEl, n * n2)) * 1e8 for n in (nk - 1, nk, nk, nk)]
    t = eng.tensor
    if kind == "eta":
        lo, sol = 1, 3                                                   # block-tridiagonal, solved for d_pi from F_pi
        bands = lambda: eng.helmholtz_blocks(75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"])).cpu().numpy()

        def run():
            Fs = [t(x) for x in rhs]
            out = eng.solve_schur_eta(75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]), *Fs)
            return list(out), Fs, None
    else:
        lo, sol = 2, 2                                                   # block-pentadiagonal, solved for d_rt from F_rt
        flags = 3 if kind == "s3_box" else 0

        def run():
            Fs = [t(x) for x in rhs]
            out = eng.solve_schur_3(75.0, t(F["theta"]), t(F["velz"]), t(F["rho"]), t(F["rt"]), t(F["pi"]), *Fs, want_L=True, flags=flags)
            return list(out[:4]), Fs, out[4].cpu().numpy()
    ref_out, ref_F, L = run()
    n0, st0, _ = eng.solve_status()
    assert n0 == 0 and (st0 == 0).all()                                  # (well-conditioned columns: the default path converges on all of them)
    if L is None:
        L = bands()
    eng.set_pivot_fallback(2)
    try:
        out, Fs, _ = run()
        nbad, st, ratio = eng.solve_status()
    finally:
        eng.set_pivot_fallback(1)                                       # (the default)
    assert nbad == 0 and (st == 3).all() and (ratio < 1e-10).all(), (nbad, np.unique(st), float(ratio.max()))
    f_key = 3 if kind == "eta" else 2
    for e in range(nEl):
        A = dense_from_band(L[e], nk, n2, lo=lo)
        b = Fs[f_key][e].cpu().numpy()
        want = np.asarray(_ld_lu_solve(A, b, (lo + 1) * n2 - 1), dtype=np.float64)
        got = out[sol][e].cpu().numpy()
        assert rel_l2(got, want) < 1e-15 * max(1e4, np.linalg.cond(A)), (e, rel_l2(got, want), np.linalg.cond(A))
    for a, b, name in zip(out + Fs, ref_out + ref_F, ("d_u", "d_rho", "d_rt|d_eta", "d_pi", "F_u", "F_rho", "F_rt|F_eta", "F_pi")):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < TOL, name       # back substitution from either solve: the same numbers to 1e-10
    again, _, _ = run()                                                   # the mode is off again: the default path, bit for bit
    for a, b in zip(again, ref_out):
        assert torch.equal(a, b)
    assert (eng.solve_status()[1] == 0).all()
