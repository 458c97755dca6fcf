"""The fixed-length mode of the C ABI's batched PCG (mimsem_ksp_set_fixed_iterations, csrc/ksp.hip) and its check log
(mimsem_krylov_ratio_max, csrc/krylov_kernels.hip): what a C++ host needs to run the density-dependent interface solves of
Euler::HorizPotVort / HorizSolve::diagVertVort (mimsem_amd/vortdiag.py: pcg_engine(fixed_its = m) and the log of VortDiag._solve) without
a host read.

Case: tests/strang_case.make_case() (p = 3, ne = 2, nk = 4), the operator of HorizPotVort -- UTMAT_H with the three interface densities
rho_i = 1/2 rho_i + 1/2 rho_{i+1} -- with the element-block preconditioner mimsem_ksp_set_pc_bjacobi builds from it.  The fixed mode is
the adaptive loop without its looks at the residual, so its result is compared BIT FOR BIT with the adaptive solve forced to the same
length (rtol = atol = 0, maxit = m); the recording through mimsem_graph_* shows that nothing is read back (a copy to the host or a stream
synchronisation inside a capture fails)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import strang_case as sc

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def case(oracle):
    from mimsem_amd.device import DeviceMesh, Engine
    c = sc.make_case()
    eng = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    rho = eng.tensor(c["rho"])
    rb = eng.combine(rho[:-1], 0.5, beta=0.5, c=rho[1:])                     # VortDiag.rho_bar
    ni, n1 = c["nk"] - 1, eng.mesh.n1
    rng = np.random.default_rng(7)
    A = lambda v: eng.apply("UTMAT_H", v, f=rb, lev0=0, scale=sc.SCALE)
    bs = [A(eng.tensor(rng.standard_normal((ni, n1)))) for _ in range(3)]
    torch.cuda.synchronize()
    return dict(eng=eng, rb=rb, ni=ni, n1=n1, A=A, b=bs[0], bs=bs)


def make_ksp(c, kind="cg"):
    from mimsem_amd.krylov import KSP
    k = KSP(c["eng"], kind)
    k.set_operator("UTMAT_H", c["ni"], lev0=0, scale=sc.SCALE, flags=0, f=c["rb"])
    if kind == "cg":
        k.set_pc("bjacobi")
    return k


def fixed_solve(c, m, b, log=None):
    k = make_ksp(c).set_fixed_iterations(m, log)
    x = k.solve(b)
    torch.cuda.synchronize()
    return k, x


def ratio(c, x, b):
    eng = c["eng"]
    r = eng.combine(c["A"](x), -1.0, beta=1.0, c=b)
    return (eng.rowdot(r, r) / eng.rowdot(b, b)).cpu().numpy()


@pytest.mark.parametrize("m", [1, 6])
def test_fixed_length_gives_the_bits_of_the_adaptive_loop_cut_at_m(case, m):
    ka = make_ksp(case).set_tolerances(rtol=0.0, atol=0.0, maxit=m, check_every=2)
    xa = ka.solve(case["b"])
    assert ka.iterations == m
    log = case["eng"].zeros(case["ni"])
    kf, xf = fixed_solve(case, m, case["b"], log)
    assert torch.equal(xf, xa)
    assert (kf.iterations, kf.rnorm, kf.reason) == (m, 0.0, "fixed_its")
    # the log is the true residual of every row
    got, want = log.cpu().numpy(), ratio(case, xf, case["b"])
    print("m = %d  log %s  recomputed %s" % (m, got, want))
    assert np.all(want > 0) and np.all(np.abs(got - want) <= 1e-12 * want)
    # no log: the same solution
    assert torch.equal(fixed_solve(case, m, case["b"])[1], xa)


def test_log_keeps_a_larger_value_and_grows_to_a_larger_ratio(case):
    log = case["eng"].zeros(case["ni"])
    log[1] = 1.0e10
    k, x = fixed_solve(case, 1, case["b"], log)
    want = ratio(case, x, case["b"])
    got = log.cpu().numpy()
    assert got[1] == 1.0e10 and all(abs(got[i] - want[i]) <= 1e-12 * want[i] for i in (0, 2))
    k.set_fixed_iterations(6, log)                                            # a better solve: nothing in the log goes down
    k.solve(case["b"])
    torch.cuda.synchronize()
    assert np.array_equal(log.cpu().numpy(), got)


def test_zero_row_gives_zero_solution_and_zero_log(case):
    b = case["b"].clone()
    b[1] = 0.0
    log = case["eng"].zeros(case["ni"])
    log[1] = -1.0                                                             # (so that the 0 below was written)
    _, x = fixed_solve(case, 6, b, log)
    _, clean = fixed_solve(case, 6, case["b"])
    assert bool((x[1] == 0.0).all()) and float(log[1]) == 0.0
    assert torch.equal(x[0], clean[0]) and torch.equal(x[2], clean[2])
    # every row zero: no early exit is needed for x = 0
    logz = case["eng"].zeros(case["ni"])
    _, xz = fixed_solve(case, 6, torch.zeros_like(b), logz)
    assert bool((xz == 0.0).all()) and bool((logz == 0.0).all())


def test_nan_row_is_logged_and_stays_in_its_row(case):
    b = case["b"].clone()
    b[2, 5] = float("nan")
    log = case["eng"].zeros(case["ni"])
    _, x = fixed_solve(case, 6, b, log)
    logc = case["eng"].zeros(case["ni"])
    _, clean = fixed_solve(case, 6, case["b"], logc)
    got, want = log.cpu().numpy(), logc.cpu().numpy()
    assert np.isnan(got[2]) and np.array_equal(got[:2], want[:2]) and np.all(np.isfinite(got[:2]))
    assert torch.equal(x[:2], clean[:2])


def test_recorded_solve_replays_the_bits_of_eager_solves(case):
    from mimsem_amd._lib import check
    eng, L = case["eng"], case["eng"].L
    m = 6
    log = eng.zeros(case["ni"])
    k = make_ksp(case).set_fixed_iterations(m, log)
    bbuf, xbuf = case["bs"][0].clone(), eng.zeros(case["ni"], case["n1"])
    torch.cuda.synchronize()
    check(L.mimsem_ctx_use_own_stream(eng.ctx), "use_own_stream")
    try:
        want = []
        for b in case["bs"]:                                                  # eager (the first one allocates the workspace)
            x = eng.zeros(case["ni"], case["n1"])
            log.zero_(); torch.cuda.synchronize()                             # (torch's stream is not the context's any more)
            k.solve(b, x=x); torch.cuda.synchronize()
            want.append((x, log.clone()))
        g = C.c_void_p()
        check(L.mimsem_graph_begin(eng.ctx), "graph_begin")
        try:
            k.solve(bbuf, x=xbuf)
        finally:
            rc = L.mimsem_graph_end(eng.ctx, C.byref(g))
        check(rc, "graph_end")
        assert L.mimsem_graph_num_nodes(g) > 6 * m
        for i in (1, 2):                                                      # changed right-hand sides
            bbuf.copy_(case["bs"][i]); xbuf.fill_(7.0); log.zero_(); torch.cuda.synchronize()
            check(L.mimsem_graph_launch(g), "graph_launch")
            torch.cuda.synchronize()
            assert torch.equal(xbuf, want[i][0]) and torch.equal(log, want[i][1])
        L.mimsem_graph_destroy(g)
    finally:
        torch.cuda.synchronize()
        eng.use_stream(torch.cuda.current_stream(eng.device))


def test_zero_restores_the_adaptive_solve(case):
    k0 = make_ksp(case).set_tolerances(rtol=1e-14, atol=1e-50, maxit=1000, check_every=2)
    x0 = k0.solve(case["b"])
    info0 = (k0.iterations, k0.rnorm, k0.reason)
    assert info0[2] in ("rtol", "atol") and info0[0] > 3
    log = case["eng"].zeros(case["ni"])
    k = make_ksp(case).set_tolerances(rtol=1e-14, atol=1e-50, maxit=1000, check_every=2).set_fixed_iterations(3, log)
    k.solve(case["b"])
    assert k.reason == "fixed_its"
    x = k.set_fixed_iterations(0).solve(case["b"])
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and (k.iterations, k.rnorm, k.reason) == info0
    # the log is let go with the mode: an adaptive solve writes none
    before = log.clone()
    k.solve(case["b"])
    torch.cuda.synchronize()
    assert torch.equal(log, before)


def test_argument_errors(case):
    eng, L = case["eng"], case["eng"].L
    k, kg = make_ksp(case), make_ksp(case, "gmres")
    log = eng.zeros(case["ni"])
    assert L.mimsem_ksp_set_fixed_iterations(None, 3, log.data_ptr()) == ERR_ARG
    assert L.mimsem_ksp_set_fixed_iterations(k.h, -1, log.data_ptr()) == ERR_ARG
    assert L.mimsem_ksp_set_fixed_iterations(kg.h, 3, log.data_ptr()) == ERR_UNSUPPORTED
    assert L.mimsem_ksp_set_fixed_iterations(k.h, 3, None) == 0 and L.mimsem_ksp_set_fixed_iterations(k.h, 0, None) == 0
    p = log.data_ptr()
    assert L.mimsem_krylov_ratio_max(None, 3, p, p + 8, p + 16) == ERR_ARG
    assert L.mimsem_krylov_ratio_max(eng.ctx, -1, p, p + 8, p + 16) == ERR_ARG
    for a in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.mimsem_krylov_ratio_max(eng.ctx, 1, *a) == ERR_ARG
    assert L.mimsem_krylov_ratio_max(eng.ctx, 0, p, p, p + 8) == 0
    from mimsem_amd._lib import MimsemError
    with pytest.raises(MimsemError):                                          # the wrapper checks the length of the log
        k.set_fixed_iterations(3, eng.zeros(case["ni"] - 1))
    with pytest.raises(MimsemError):
        eng.ratio_max(eng.zeros(2), eng.zeros(3), eng.zeros(3))


def test_ratio_max_kernel(case):
    """more than one block; the clamp of the denominator, and a NaN in the numerator, the denominator or the log itself"""
    eng = case["eng"]
    n = 300
    rng = np.random.default_rng(11)
    num, den, log = np.abs(rng.standard_normal(n)), np.abs(rng.standard_normal(n)), np.abs(rng.standard_normal(n))
    den[3] = 0.0; num[3] = 0.0                     # 0 / max(0, 1e-300) = 0
    den[4] = 0.0; num[4] = 1.0e-310                # a denormal over the clamp
    den[5] = 1.0e-305                              # below the clamp
    num[6] = np.nan; den[7] = np.nan; log[8] = np.nan
    num[299] = 1.0e6; log[298] = 1.0e9
    tn, td, tl = eng.tensor(num), eng.tensor(den), eng.tensor(log)
    want = torch.maximum(tl, tn / td.clamp_min(1e-300))
    got = eng.ratio_max(tn, td, tl)
    assert got is tl and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert [i for i in range(n) if np.isnan(got.cpu().numpy()[i])] == [6, 7, 8]
