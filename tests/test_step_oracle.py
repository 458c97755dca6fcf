"""CPU checks of what the benchmark-size parity tests (tests/test_gpu_step_parity.py) stand on: the sparse mode of the numpy oracles
is the same oracle as the dense mode, the committed config-2 fixture is what that oracle computes, and the sketch that stands in for
the full HorizSolve outputs sees an error of the size the tests bound."""
import os

import numpy as np
import pytest

from tests.helpers import _splitmix64, hash_uniform, rel_l2, sketch, sketch_rel_err, z_levels

SAME = 1e-13          # sparse vs dense mode, and the fixture vs a fresh run: both are the same arithmetic up to summation order


@pytest.fixture(scope="module")
def sw_pair(oracle):
    pytest.importorskip("scipy")
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from oracle import sw_oracle
    pn, ne = 3, 2
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, 1) for p in range(6)]
    geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
    D = sw_oracle.SWOracle(cs, topos, geoms, coords)
    S = sw_oracle.SWOracle(cs, topos, geoms, coords, sparse=True)
    # the perturbed Williamson-2 state of tests/test_gpu_sweqn.py
    th = np.arcsin(D.xq[:, 2] / 6371220.0); lam = np.arctan2(D.xq[:, 1], D.xq[:, 0])
    U0, H0 = 38.61068276698372, 2998.1154702758267
    uq = np.stack([U0 * np.cos(th) + 3.0 * np.sin(2 * lam) * np.cos(th), 2.0 * np.cos(lam) * np.cos(th) ** 2], axis=1)
    hq = H0 - (6371220.0 * 7.292e-5 * U0 + 0.5 * U0 * U0) * np.sin(th) ** 2 / 9.80616 + 40.0 * np.cos(th) * np.sin(lam)
    return D, S, uq, hq


def test_sparse_sw_oracle_matches_dense(sw_pair):
    D, S, uq, hq = sw_pair
    import scipy.sparse as sp
    assert sp.issparse(S.M1) and sp.issparse(S.E21) and sp.issparse(S.assemble_operator(360.0))
    for k in ("E21", "E10"):                                         # the incidences are small integers: the same bits
        assert np.array_equal(getattr(S, k).toarray(), getattr(D, k)), k
    for k in ("M0", "M1", "M2"):
        assert rel_l2(getattr(S, k).toarray(), getattr(D, k)) < SAME, k
    assert rel_l2(S.fg, D.fg) < SAME
    u0, h0 = D.init1(uq), D.init2(hq)
    e_init = (rel_l2(S.init1(uq), u0), rel_l2(S.init2(hq), h0))
    r = np.random.default_rng(5)
    u1 = u0 * (1 + 1e-2 * r.standard_normal(u0.size)); h1 = h0 * (1 + 1e-3 * r.standard_normal(h0.size))
    print("sparse vs dense SW oracle: init1 %.1e  init2 %.1e" % e_init)
    assert max(e_init) < SAME
    for qe in (False, True):
        fu_d, fh_d = D.assemble_residual(u0, h0, u1, h1, 360.0, q_exact=qe)
        fu_s, fh_s = S.assemble_residual(u0, h0, u1, h1, 360.0, q_exact=qe)
        # the residual is M (x_j - x_i) + dt f: a difference of terms ~1e3 times its own size, whose round-off (the two modes sum the
        # element blocks in different orders) is relative to those terms -- measure it there
        su, sh = np.linalg.norm(D.M1 @ u1), np.linalg.norm(D.M2 @ h1)
        eu, eh = np.linalg.norm(fu_s - fu_d) / su, np.linalg.norm(fh_s - fh_d) / sh
        print("  assemble_residual q_exact=%s: f_u %.1e  f_h %.1e  (of |M1 u_j|, |M2 h_j|)" % (qe, eu, eh))
        assert eu < SAME and eh < SAME
        assert np.linalg.norm(fu_d) > 1e-4 * su and np.linalg.norm(fh_d) > 1e-4 * sh      # (the residual is not round-off itself)
    for qe, nits, dt in ((False, 2, 360.0), (True, 4, 600.0)):
        ud, hd = D.solve(u0, h0, dt, nits=nits, q_exact=qe); hist_d = np.array(D.history)
        us, hs = S.solve(u0, h0, dt, nits=nits, q_exact=qe); hist_s = np.array(S.history)
        print("  solve q_exact=%s: u %.1e  h %.1e  history %.1e" % (qe, rel_l2(us, ud), rel_l2(hs, hd), np.abs(hist_s / hist_d - 1).max()))
        assert rel_l2(us, ud) < SAME and rel_l2(hs, hd) < SAME and len(hist_s) == nits
        assert np.allclose(hist_s, hist_d, rtol=1e-8, atol=0)


def test_sparse_horiz_oracle_matches_dense(oracle):
    pytest.importorskip("scipy")
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from oracle import horiz_oracle as ho
    pn, ne, nk = 3, 2, 3
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    levs = z_levels(nk, geoms[0].n0)
    for g in geoms:
        g.set_levels(levs)
    D = ho.HorizOracle(ho.GlobalDense(cs, topos, geoms, coords, levs))
    S = ho.HorizOracle(ho.GlobalDense(cs, topos, geoms, coords, levs, sparse=True))
    from tests.golden.make_step_fixtures import horiz_inputs
    area = np.mean([P.det.mean() for P in D.g.P]) * 4.0 / (pn * pn); dz = np.mean([P.thick.mean() for P in D.g.P])
    f = horiz_inputs(nk, D.g.N1, D.g.N2, area, dz)
    args = (f["u1"], f["u2"], f["h1"], f["h2"], f["theta"])
    errs = {}
    for name, a, b in zip(("dF", "dG", "Fk", "Gk"), S.advection_rhs_ec(*args), D.advection_rhs_ec(*args)):
        errs[name] = rel_l2(a, b)
    Fk = D.advection_rhs_ec(*args)[2]
    errs["q"] = max(rel_l2(S.diagnose_q(lev, f["h1"][lev], f["u1"][lev]), D.diagnose_q(lev, f["h1"][lev], f["u1"][lev])) for lev in range(nk))
    for use_F, use_w in ((False, False), (True, False), (True, True)):
        for lev in range(nk):
            kw = dict(Fx=Fk[lev] if use_F else None, Fz=f["Fz"] if use_F else None, Fk=Fk[lev],
                      dwdx1=f["dwdx1"] if use_w else None, dwdx2=f["dwdx2"] if use_w else None)
            a = (lev, f["theta"][lev], f["dudz1"], f["dudz2"], f["velz1"], f["velz2"], f["Pi"][lev], f["u1"][lev], f["u2"][lev],
                 f["h1"][lev], f["h2"][lev])
            (ys, ks), (yd, kd) = S.momentum_rhs_ec(*a, **kw), D.momentum_rhs_ec(*a, **kw)
            key = "fu(F=%d,w=%d)" % (use_F, use_w)
            errs[key] = max(errs.get(key, 0.0), rel_l2(ys, yd), abs(ks - kd) / abs(kd))
    print("sparse vs dense HorizSolve oracle: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < SAME, errs


def test_config2_fixture_is_the_sparse_oracle(oracle, golden_dir):
    """re-run bench.py's config-2 step (Williamson-2, 16x16x6, dt 600 s, 4 Picard iterations) through the committed sparse oracle:
    the committed fixture's sketches are what it computes (about 10 s: the oracle assembles and factors 41 472-row systems)"""
    pytest.importorskip("scipy")
    from tests.golden.make_step_fixtures import SW_CASES, SW_FIELDS, sw_step
    fname, ne, dt, nits, q_exact, ic = SW_CASES["sw2"]
    want = np.load(os.path.join(golden_dir, fname))
    got = sw_step(ne, dt, nits, q_exact, ic)
    errs = {k: sketch_rel_err(got[k], want["S_" + k], float(want["norm_" + k])) for k in SW_FIELDS}
    errs.update(norms=max(abs(np.linalg.norm(got[k]) / float(want["norm_" + k]) - 1.0) for k in SW_FIELDS),
                history=rel_l2(got["history"], want["history"]))
    print("config-2 fixture vs a fresh sparse-oracle run: " + "  ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < SAME, errs
    assert int(want["nits"]) == nits and float(want["dt"]) == dt and bool(want["q_exact"]) == q_exact


def test_hash_and_sketch_helpers():
    # splitmix64 pinned to its published first outputs (seed 0: state += golden gamma, then the mix), so a changed hash cannot pass
    # silently while the GPU tests rebuild the wrong inputs
    assert int(_splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(_splitmix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4
    u = hash_uniform(3, (1000,), -2.0, 5.0)
    assert np.array_equal(u, hash_uniform(3, (1000,), -2.0, 5.0)) and not np.array_equal(u, hash_uniform(4, (1000,), -2.0, 5.0))
    assert u.min() >= -2.0 and u.max() < 5.0 and abs(u.mean() - 1.5) < 0.2
    n = 622080                                                          # the HorizSolve fixture's nk * n1
    y = hash_uniform(11, (n,), -1.0, 1.0) * np.exp(hash_uniform(12, (n,), -3.0, 3.0))
    s, ny = sketch(y), np.linalg.norm(y)
    assert sketch_rel_err(y, s, ny) == 0.0
    # a single wrong entry of 1e-9 |y|: every column of S has norm 1, so the sketch sees exactly that
    for i in (0, 12345, n - 1):
        yb = y.copy(); yb[i] += 1e-9 * ny
        e = sketch_rel_err(yb, s, ny)
        assert 0.9e-9 < e < 1.1e-9 and e > 1e-10, (i, e)
    # round-off: every entry perturbed by 1e-15 relative stays far below the tolerances the tests use
    yr = y * (1.0 + 1e-15 * hash_uniform(13, (n,), -1.0, 1.0))
    e = sketch_rel_err(yr, s, ny)
    assert e < 1e-12, e
    # an error spread over every entry is seen at its size too (within the Johnson-Lindenstrauss spread of K = 64 rows)
    d = 1e-9 * ny * hash_uniform(14, (n,), -1.0, 1.0) / np.linalg.norm(hash_uniform(14, (n,), -1.0, 1.0))
    assert 0.5e-9 < sketch_rel_err(y + d, s, ny) < 1.5e-9
