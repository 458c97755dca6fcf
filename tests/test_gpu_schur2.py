"""GPU parity of VertSolve.solve_schur_2 (mimsem_amd/vertsolve.py: VertSolve::solve_schur_2, eul/VertSolve.cpp:1059-1246, the Newton loop
around solve_schur_column_3) and of its fused entry points mimsem_column_newton2_residual / _update, against the column-by-column numpy
restatement tests/schur2_case.py.  The bar is the project's 1e-10 relative L2: the loop is well conditioned on these states (1e-15 relative
noise in the start state moves the result of three iterations by at most 5.4e-15), which leaves about five orders of margin."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import schur2_case as sc
from tests.helpers import make_patch, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("velz", "rho", "rt", "exner")

# (p, ne, nk): an odd level count; the minimum solve_schur_3 accepts; the half-row layout of order 4; more columns than a block's tasks;
# order 5 (composed route only)
SHAPES = [(3, 2, 5), (2, 2, 4), (4, 1, 6), (3, 3, 8), (5, 1, 4)]
_CASES = {}


def _case(oracle, shape):
    """engine, patch, start state (host and device) of a shape, and the restated three iterations at dt = 0.5: built once, never changed"""
    if shape not in _CASES:
        from mimsem_amd.device import DeviceMesh, Engine
        pn, ne, nk = shape
        cs, topo, geom, P, rng = make_patch(oracle, pn, ne, 6, 1, nk=nk, seed=7 * pn + nk)
        eng = Engine(DeviceMesh([topo], [geom], nk=nk, numbering="local"))
        st = sc.state_at_rest(P, geom)
        dev = {k: eng.tensor(v) for k, v in st.items()}
        want = sc.solve_schur_2(P, 0.5, st["velz"], st["rho"], st["rt"], st["exner"], st["zv"], 3)
        _CASES[shape] = (eng, P, st, dev, want)
    return _CASES[shape]


def _run(eng, dev, dt, fused, maxit=3, tol=0.0, **kw):
    from mimsem_amd.vertsolve import VertSolve
    vs = VertSolve(eng, dt)
    out = vs.solve_schur_2(dev["velz"], dev["rho"], dev["rt"], dev["exner"], dev["zv"], maxit=maxit, tol=tol, fused=fused, **kw)
    return vs, out


def _compare(vs, got, want, what):
    for a, name in zip(got, FIELDS):
        assert np.all(np.isfinite(want[name])), (what, name)
        err = rel_l2(a.cpu().numpy(), want[name])
        print("%s %s: %.3e" % (what, name, err))
        assert err < TOL, (what, name, err)
    for a, name in ((vs.theta_h, "theta_h"), (vs.exner_h, "exner_h")):
        err = rel_l2(a.cpu().numpy(), want[name])
        print("%s %s: %.3e" % (what, name, err))
        assert err < TOL, (what, name, err)
    # k2i_z is a sum with cancellation: its round-off scales with the sum of the magnitudes of its terms
    print("%s k2i_z: %.6e against %.6e (sum of magnitudes %.3e)" % (what, vs.k2i_z, want["k2i_z"], want["k2i_abs"]))
    assert abs(vs.k2i_z - want["k2i_z"]) <= TOL * want["k2i_abs"], (what, vs.k2i_z, want["k2i_z"])
    assert len(vs.history) == len(want["history"])
    for hd, ho in zip(vs.history, want["history"]):
        for k in ("exner", "w", "rho", "rt"):
            assert abs(hd[k] - ho[k]) <= 1e-5 * ho[k] + 1e-15, (what, k, hd[k], ho[k])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "p%d_ne%d_nk%d" % s)
def test_composed_loop_matches_the_restatement(oracle, shape):
    """the composed route (single-operator entry points only, every order): three iterations at dt = 0.5; state, theta_h, exner_h, k2i_z, history"""
    eng, P, st, dev, want = _case(oracle, shape)
    vs, got = _run(eng, dev, 0.5, fused=False)
    _compare(vs, got, want, "composed")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] <= 4], ids=lambda s: "p%d_ne%d_nk%d" % s)
def test_fused_loop_matches_the_restatement_and_the_composed_loop(oracle, shape):
    """the fused route (mimsem_column_newton2_residual / _update, max_norms, diag_theta_blend): the same cases at orders <= 4"""
    eng, P, st, dev, want = _case(oracle, shape)
    vs, got = _run(eng, dev, 0.5, fused=True)
    _compare(vs, got, want, "fused")
    vc, comp = _run(eng, dev, 0.5, fused=False)
    for a, b, name in zip(got, comp, FIELDS):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < TOL, name
    assert rel_l2(vs.theta_h.cpu().numpy(), vc.theta_h.cpu().numpy()) < TOL


@pytest.mark.parametrize("shape", [(3, 2, 5), (3, 3, 8)], ids=lambda s: "p%d_ne%d_nk%d" % s)
def test_all_optional_inputs(oracle, shape):
    """Held-Suarez forcing, u dw/dx and a seeded random horizontal forcing, dt = 30, three iterations, both routes.  At dt = 0.5 the
    forcings move the state by less than the bar, so a missing term would pass; at dt = 30 each moves every field by more than 100 x TOL
    (asserted on the restatement itself)"""
    eng, P, st, dev, _ = _case(oracle, shape)
    dt = 30.0
    ex = sc.extras(P, st, dt)
    args = (P, dt, st["velz"], st["rho"], st["rt"], st["exner"], st["zv"], 3)
    base = sc.solve_schur_2(*args)
    for name, kw in (("hs", dict(hs_forcing=True)), ("udwdx", dict(udwdx=ex["udwdx"])), ("horiz", dict(dFx=ex["dFx"], dGx=ex["dGx"]))):
        one = sc.solve_schur_2(*args, **kw)
        moved = [rel_l2(one[k], base[k]) for k in FIELDS]
        print(name, moved)
        assert min(moved) > 100 * TOL, (name, moved)
    seen = []

    def forcing_ref(rho_i, rho_j, theta_h):
        seen.append(theta_h.shape)
        return ex["dFx"], ex["dGx"]
    want = sc.solve_schur_2(*args, hs_forcing=True, udwdx=ex["udwdx"], dFx=forcing_ref)
    assert seen == [(P.nEl, (P.nk + 1) * P.n2e)] * 3                  # the forcing gets theta_h on the nk+1 interfaces
    t = eng.tensor
    dFx, dGx = t(ex["dFx"]), t(ex["dGx"])
    calls = []

    def forcing(rho_i, rho_j, theta_h):
        calls.append(tuple(theta_h.shape))
        return dFx, dGx
    for fused in (False, True):
        calls.clear()
        vs, got = _run(eng, dev, dt, fused=fused, horiz_forcing=forcing, udwdx=t(ex["udwdx"]), hs_lat=t(ex["lat"]))
        assert calls == [(P.nEl, (P.nk + 1) * P.n2e)] * 3
        _compare(vs, got, want, "all inputs, %s" % ("fused" if fused else "composed"))


@pytest.mark.parametrize("shape", [(3, 2, 5), (4, 1, 6)], ids=lambda s: "p%d_ne%d_nk%d" % s)
def test_entry_points_alone(oracle, shape):
    """newton2_residual against the composed pieces on one iterate (the second: velz_j != 0, x_h != x_i), with each nullable input null and
    then present; newton2_update bit-equal to the torch expressions, its norm_squares through max_norms"""
    from mimsem_amd.vertsolve import VertSolve
    eng, P, st, dev, _ = _case(oracle, shape)
    nk, dt = P.nk, 30.0
    ex = sc.extras(P, st, dt)
    t = eng.tensor
    vs = VertSolve(eng, dt)
    vi, ri, ti, ei, zv = (dev[k] for k in ("velz", "rho", "rt", "exner", "zv"))
    vj, rj, tj, ej = vs.solve_schur_2(vi, ri, ti, ei, zv, maxit=1, tol=0.0, fused=False)
    theta_h, exner_h = vs.theta_h, vs.exner_h
    udwdx, dFx, dGx = t(ex["udwdx"]), t(ex["dFx"]), t(ex["dGx"])
    hs = eng.temp_forcing_hs(t(ex["lat"]), exner_h, theta_h, 0.5 * ri + 0.5 * rj)
    F_w0, F_z, G_z = vs.assemble_residual(theta_h, exner_h, vi, vj, ri, rj, zv)
    k2i0 = vs._k2i
    F_ex0 = eng.column_eos(0, tj, ej)
    for on in ((), ("w",), ("rho",), ("rt",), ("hs",), ("w", "rho", "rt", "hs")):
        a = dict(add_w=udwdx if "w" in on else None, add_rho_pre=dFx if "rho" in on else None, add_rt_pre=dGx if "rt" in on else None,
                 add_rt_post=hs if "hs" in on else None)
        F_w, F_rho, F_rt, F_ex, k2i = eng.newton2_residual(dt, vs.rayleigh, theta_h, exner_h, vi, vj, ri, rj, zv, ti, tj, ej, **a)
        w_F_w = F_w0 + dt * udwdx if "w" in on else F_w0
        dF = rj + dt * vs.V10(F_z) - ri + (dt * dFx if "rho" in on else 0.0)
        dG = tj + dt * vs.V10(G_z) - ti + (dt * dGx if "rt" in on else 0.0)
        w_F_rho = vs._mv("CONST", dF, rows=nk)
        w_F_rt = vs._mv("CONST", dG, rows=nk) + (dt * hs if "hs" in on else 0.0)
        for got, want, name in ((F_w, w_F_w, "F_w"), (F_rho, w_F_rho, "F_rho"), (F_rt, w_F_rt, "F_rt"), (F_ex, F_ex0, "F_exner"), (k2i, k2i0, "k2i")):
            err = rel_l2(got.cpu().numpy(), want.cpu().numpy())
            print(on, name, "%.3e" % err)
            assert err < TOL, (on, name, err)
    # rayleigh = 0 (the box twin): the friction term is gone, nothing else moves
    F_w, *_ = eng.newton2_residual(dt, 0.0, theta_h, exner_h, vi, vj, ri, rj, zv, ti, tj, ej)
    vs0 = VertSolve(eng, dt, rayleigh=0.0)
    assert rel_l2(F_w.cpu().numpy(), vs0.assemble_residual(theta_h, exner_h, vi, vj, ri, rj, zv)[0].cpu().numpy()) < TOL
    # the update
    r = np.random.default_rng(3)
    d = [t(1e-3 * r.standard_normal(tuple(x.shape)) * np.abs(x.cpu().numpy()).mean()) for x in (ri, ri, ti, ei)]
    d[0] = t(r.standard_normal(tuple(vi.shape)))
    xi = (vi, ri, ti, ei)
    xj = [x.clone() for x in (vj, rj, tj, ej)]
    want_j = [x + dx for x, dx in zip(xj, d)]
    want_h = [0.5 * a + 0.5 * b for a, b in zip(xi, want_j)]
    *got_h, nrm = eng.newton2_update(*d, *xi, *xj)
    for a, b in zip(xj + got_h, want_j + want_h):
        assert torch.equal(a, b)
    n2 = P.n2e
    pad = lambda x: torch.cat([x, torch.zeros(P.nEl, n2, dtype=torch.float64, device=x.device)], dim=1)
    want_nrm = torch.stack([d[3] * d[3], want_j[3] * want_j[3], pad(d[0] * d[0]), pad(want_j[0] * want_j[0]),
                            d[1] * d[1], want_j[1] * want_j[1], d[2] * d[2], want_j[2] * want_j[2]])
    assert torch.equal(nrm, want_nrm)
    col = lambda dx, x: float((torch.linalg.vector_norm(dx, dim=1) / torch.linalg.vector_norm(x, dim=1)).max())
    want_mx = [col(d[3], want_j[3]), col(d[0], want_j[0]), col(d[1], want_j[1]), col(d[2], want_j[2])]
    assert np.allclose(eng.max_norms(nrm).cpu().numpy(), want_mx, rtol=1e-13, atol=0.0)


def test_convergence_and_the_three_norm_stop(oracle):
    """maxit = 40, tol = 1e-12 at (3, 2, 5), dt = 0.5: stops when exner, rho AND rt are below tol, within one iteration of the restatement"""
    eng, P, st, dev, _ = _case(oracle, (3, 2, 5))
    want = sc.solve_schur_2(P, 0.5, st["velz"], st["rho"], st["rt"], st["exner"], st["zv"], 40, tol=1e-12)
    for fused in (False, True):
        vs, got = _run(eng, dev, 0.5, fused=fused, maxit=40, tol=1e-12)
        h = vs.history
        print(fused, len(h), len(want["history"]), h[-1])
        assert len(h) < 40 and abs(len(h) - len(want["history"])) <= 1
        assert all(h[-1][k] < 1e-12 for k in ("exner", "rho", "rt"))
        assert all(not all(x[k] < 1e-12 for k in ("exner", "rho", "rt")) for x in h[:-1])
        for a, name in zip(got, FIELDS):
            assert rel_l2(a.cpu().numpy(), want[name]) < TOL, (fused, name)


def test_determinism_and_capture(oracle):
    """two runs give the same bits; residual + update replayed from a captured graph give the bits of the eager calls"""
    eng, P, st, dev, _ = _case(oracle, (3, 3, 8))
    for fused in (False, True):
        _, a = _run(eng, dev, 0.5, fused=fused)
        _, b = _run(eng, dev, 0.5, fused=fused)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), fused
    from mimsem_amd.vertsolve import VertSolve
    dt = 0.5
    vs = VertSolve(eng, dt)
    vi, ri, ti, ei, zv = (dev[k] for k in ("velz", "rho", "rt", "exner", "zv"))
    xj0 = vs.solve_schur_2(vi, ri, ti, ei, zv, maxit=1, tol=0.0, fused=True)
    theta_h, exner_h = vs.theta_h, vs.exner_h
    r = np.random.default_rng(5)
    d = [eng.tensor(1e-4 * r.standard_normal(tuple(x.shape)) * np.abs(x.cpu().numpy()).mean()) for x in (ri, ri, ti, ei)]
    d[0] = eng.tensor(1e-3 * r.standard_normal(tuple(vi.shape)))

    def step(xj):
        F = eng.newton2_residual(dt, vs.rayleigh, theta_h, exner_h, vi, xj[0], ri, xj[1], zv, ti, xj[2], xj[3])
        U = eng.newton2_update(*d, vi, ri, ti, ei, *xj)
        return list(F) + list(U)
    eager_j = [x.clone() for x in xj0]
    eager = step(eager_j)
    work = [x.clone() for x in xj0]
    g, out = eng.capture(lambda: step(work))          # (the warm-up and the capture pass have already updated `work` in place)
    for w, x in zip(work, xj0):
        w.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out + work, eager + eager_j):
        assert torch.equal(a, b)


def test_errors(oracle):
    """order 5: the entries return MIMSEM_ERR_UNSUPPORTED and the loop runs composed without raising; null outputs and nk = 3 are refused"""
    from mimsem_amd import _lib
    from mimsem_amd.device import DeviceMesh, Engine, _ptr
    eng, P, st, dev, want = _case(oracle, (5, 1, 4))
    vi, ri, ti, ei, zv = (dev[k] for k in ("velz", "rho", "rt", "exner", "zv"))
    th = eng.diag_theta(1, ri, ti)
    with pytest.raises(_lib.MimsemError, match="code -2"):
        eng.newton2_residual(0.5, 0.0, th, ei, vi, vi, ri, ri, zv, ti, ti, ei)
    with pytest.raises(_lib.MimsemError, match="code -2"):
        eng.newton2_update(vi, ri, ti, ei, vi, ri, ti, ei, vi.clone(), ri.clone(), ti.clone(), ei.clone())
    vs, got = _run(eng, dev, 0.5, fused=True)                          # asked for, unsupported at this order: composed
    _compare(vs, got, want, "order 5, fused asked")
    # null outputs
    eng3, P3, st3, dev3, _ = _case(oracle, (3, 2, 5))
    vi, ri, ti, ei, zv = (dev3[k] for k in ("velz", "rho", "rt", "exner", "zv"))
    th = eng3.diag_theta(1, ri, ti)
    p = _ptr
    outs = [torch.empty_like(x) for x in (vi, ri, ri, ri, vi)]
    for null in range(5):
        o = [None if i == null else p(x) for i, x in enumerate(outs)]
        rc = eng3.L.mimsem_column_newton2_residual(eng3.ctx, 0.5, 0.0, p(th), p(ei), p(vi), p(vi), p(ri), p(ri), p(zv), p(ti), p(ti), p(ei),
                                                   None, None, None, None, *o)
        assert rc == -1, null
    xj = [x.clone() for x in (vi, ri, ti, ei)]
    xh = [torch.empty_like(x) for x in xj]
    nrm = torch.empty(8, P3.nEl, P3.nk * P3.n2e, dtype=torch.float64, device=vi.device)
    for null in range(5):
        o = [None if i == null else p(x) for i, x in enumerate(xh + [nrm])]
        rc = eng3.L.mimsem_column_newton2_update(eng3.ctx, p(vi), p(ri), p(ti), p(ei), p(vi), p(ri), p(ti), p(ei), *[p(x) for x in xj], *o)
        assert rc == -1, null
    assert all(torch.equal(a, b) for a, b in zip(xj, (vi, ri, ti, ei)))          # a refused call writes nothing
    # nk = 3: refused as mimsem_column_solve_schur_3 refuses it
    cs, topo, geom, Pk, rng = make_patch(oracle, 2, 1, 6, 0, nk=3, seed=1)
    e = Engine(DeviceMesh([topo], [geom], nk=3, numbering="local"))
    z = lambda sl: torch.ones(Pk.nEl, sl * Pk.n2e, dtype=torch.float64, device=e.device)
    with pytest.raises(_lib.MimsemError, match="code -1"):
        e.newton2_residual(0.5, 0.0, z(4), z(3), z(2), z(2), z(3), z(3), z(3), z(3), z(3), z(3))
    with pytest.raises(_lib.MimsemError, match="code -1"):
        e.newton2_update(z(2), z(3), z(3), z(3), z(2), z(3), z(3), z(3), z(2), z(3), z(3), z(3))
    with pytest.raises(_lib.MimsemError, match="code -1"):
        e.solve_schur_3(0.5, z(4), z(2), z(3), z(3), z(3), z(2), z(3), z(3), z(3))


def test_loop_driven_from_cpp(tmp_path, oracle):
    """mimsem_host::VertSolve2 (mimsem_amd/host/mimsem_vertsolve.hpp) built and run as tests/test_gpu_cpp_shim.py runs test_vert.cpp: three
    iterations without and with every optional input at dt = 30, and the loop run to its three-norm stop, against the Python loop at TOL"""
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    eng, P, st, dev, _ = _case(oracle, (3, 2, 5))
    dt = 30.0
    ex = sc.extras(P, st, dt)
    arrays = mesh_arrays(eng.mesh)
    arrays.update(dt=np.array([dt]), zv=st["zv"], velz=st["velz"], rho=st["rho"], rt=st["rt"], exner=st["exner"], lat=ex["lat"],
                  udwdx=ex["udwdx"], dFx=ex["dFx"], dGx=ex["dGx"])
    fin, fout = str(tmp_path / "vert2_in.arr"), str(tmp_path / "vert2_out.bin")
    write_arrays(fin, arrays)
    exe = os.path.join(str(tmp_path), "test_vert2")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_vert2.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "DONE" in out.stdout
    res = np.fromfile(fout, dtype=np.float64)
    pos = [0]

    def take(shape):
        n = int(np.prod(shape)); a = res[pos[0]:pos[0] + n].reshape(shape); pos[0] += n
        return a
    t = eng.tensor
    dFx, dGx = t(ex["dFx"]), t(ex["dGx"])
    runs = (dict(maxit=3, tol=0.0), dict(maxit=3, tol=0.0, horiz_forcing=lambda a, b, c: (dFx, dGx), udwdx=t(ex["udwdx"]), hs_lat=t(ex["lat"])),
            dict(maxit=40, tol=1e-12))
    nt = (P.nEl, (P.nk + 1) * P.n2e)
    for run, kw in enumerate(runs):
        got = [take(st[k].shape) for k in FIELDS] + [take(nt), take(st["rho"].shape)]
        its, k2i_z = take((2,))
        hist = take((int(its), 4))
        vs, py = _run(eng, dev, dt, fused=True, **kw)
        for a, b, name in zip(got, list(py) + [vs.theta_h, vs.exner_h], FIELDS + ("theta_h", "exner_h")):
            assert rel_l2(a, b.cpu().numpy()) < TOL, (run, name)
        assert int(its) == len(vs.history) and (run < 2 or int(its) < 40)
        assert abs(k2i_z - vs.k2i_z) <= 1e-9 * abs(vs.k2i_z) + 1e-300
        for hd, ho in zip(hist, vs.history):
            for j, k in enumerate(("exner", "w", "rho", "rt")):
                assert abs(hd[j] - ho[k]) <= 1e-5 * ho[k] + 1e-15, (run, k)
        if run == 2:
            assert all(hist[-1][j] < 1e-12 for j in (0, 2, 3)) and all(not all(h[j] < 1e-12 for j in (0, 2, 3)) for h in hist[:-1])
    assert pos[0] == res.size
