"""The passes whose work item is one element and a chunk of `lch` consecutive levels -- the two-pass element kernel (body_elem_apply), the
register-resident and the LDS-resident shared-block applies (k_blocks_apply_reg, k_blocks_apply_levels) and the owned-block pass
(k_owned_pass<ND, LC, KIND>) -- with several levels per work item on meshes a unit test can afford.  The library's rule gives one level per
item there, so the chunk loops (level-invariant data in registers, the next level prefetched, the ragged last chunk, a wavefront whose
elements have different level ranges) would otherwise run at full size only; mimsem_ctx_set_level_chunk asks for 1 .. 8 levels instead, in
the default build.

Shapes: patches of 3 x 3 = 9 elements (no multiple of the 4, 2 or 1-per-wave / 4-per-workgroup elements that share a wavefront or workgroup)
and the closed 2 x 2 x 6 sphere of 24 elements, both with 11 levels: 8 + 3 at lch = 8, 4 + 4 + 3 at 4, 3 + 3 + 3 + 2 at 3, 2 x 5 + 1 at 2.
Orders 2 .. 7; order 1 has no sphere coordinates (mesh.sphere_coords raises), so it is left out.

Every level has its own random inputs.  Inputs carry one extra row of NaN behind the call's last level (a value prefetched from past the call
would poison the result) and results one extra sentinel row (nothing writes past the ragged chunk); results start as NaN where the call
overwrites them, so a slot that is never written shows as well.

Every test builds engines of its own and sets the chunk back to 0 in a `finally`: no engine of another module ever carries a request."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import SCALE, make_patch, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-10                  # BASELINE north_star, as tests/test_gpu_horizontal.py: relative L2 per level against the oracle
NK = 11
PATCH_PI = {2: 5, 3: 0, 4: 3, 5: 2, 6: 1, 7: 4}      # a different patch of the cube per order, as tests/test_gpu_horizontal.py
SENTINEL = -7.25e77
CHUNKS = (2, 3, 4, 8)
FLAG_ACCUM, FLAG_TRANSPOSE = 2, 4
COEF = [(1.2, 0.0)] + [(1.0, 0.05)] * 7       # as test_owned_chebyshev_several_levels_per_work_item


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
def _pad(a):
    """the rows of `a` on the device with one row of NaN behind them: (the view of the rows, the whole buffer)"""
    import torch
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    buf = torch.full((a.shape[0] + 1, a.shape[1]), float("nan"), dtype=torch.float64, device="cuda")
    buf[:-1] = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    return buf[:-1]


def _result(nlev, n, base=None):
    """a result of nlev rows (NaN, or `base` for a call that accumulates or updates in place) with the sentinel row behind it"""
    import torch
    buf = torch.full((nlev + 1, n), float("nan"), dtype=torch.float64, device="cuda")
    buf[-1] = SENTINEL
    if base is not None:
        buf[:-1] = base
    return buf


def _checked(buf, what):
    """the rows of a result buffer after the call: the sentinel row untouched, every row finite"""
    import torch
    assert bool((buf[-1] == SENTINEL).all()), "%s: the row behind the call's last level was written" % (what,)
    assert bool(torch.isfinite(buf[:-1]).all()), "%s: a result is not finite" % (what,)
    return buf[:-1]


def _engage(eng, lch, nlev):
    """ask for lch levels per work item and prove that the setting engaged"""
    eng.set_level_chunk(lch)
    assert eng.L.mimsem_op_level_chunk(eng.ctx, nlev) == min(lch, nlev), (lch, nlev)


# ---- (a), (b): the element pass ---------------------------------------------------------------------------------------------------------
class Call:
    """one call of the element pass: run(eng, y) writes the rows of y, want[k] is the oracle's row k"""

    def __init__(self, name, nlev, nout, run, want, base=None, lch_a=3):
        self.name, self.nlev, self.nout, self.run, self.want, self.base, self.lch_a = name, nlev, nout, run, want, base, lch_a

    def __call__(self, eng):
        buf = _result(self.nlev, self.nout, self.base)
        self.run(eng, buf[:-1])
        return _checked(buf, self.name)


_PATCHES = {}


def _patch(oracle, pn):
    """the 9-element patch of order pn, its oracle and the calls of tests (a) and (b) with their oracle rows: built once, never changed"""
    if pn in _PATCHES:
        return _PATCHES[pn]
    import torch
    from mimsem_amd.device import DeviceMesh
    from tests.hmomentum_case import _exner_fields
    cs, topo, geom, P, rng = make_patch(oracle, pn, ne=3, nprocs=6, pi=PATCH_PI[pn], nk=NK, seed=pn * 100 + PATCH_PI[pn])
    assert P.nEl == 9
    dm = DeviceMesh([topo], [geom], nk=NK, numbering="local")
    r = np.random.default_rng(1000 + pn)
    n0, n1, n2, nq = P.n0, P.n1, P.n2, P.n0q
    F = dict(h2=r.uniform(0.5, 1.5, (NK, n2)) * 1e6, u1=r.standard_normal((NK, n1)) * 1e3, q0=r.standard_normal((NK, n0)) * 1e-4,
             x0=r.standard_normal((NK, n0)), x1=r.standard_normal((NK, n1)), x2=r.standard_normal((NK, n2)))
    D = {k: _pad(v) for k, v in F.items()}
    nout = {0: n0, 1: n1, 2: n2}
    calls = []

    def add(name, nlev, n, run, want, **kw):
        want = np.stack(want)
        assert want.shape == (nlev, n) and np.isfinite(want).all(), name
        calls.append(Call(name, nlev, n, run, want, **kw))

    # the operators of tests/test_gpu_horizontal.py::CASES (the two inverses go through the column path: not here)
    from tests.test_gpu_horizontal import CASES
    from mimsem_amd.device import Engine
    spaces = Engine._SPACES
    for op, flag, fkey, xkey in CASES:
        if op in ("WMATINV", "WHMATINV"):
            continue
        nlev = NK - 1 if op in ("UTMAT", "UTMAT_H") else NK          # (they read thick[lev + 1])
        x, f = _pad(F[xkey][:nlev]), (None if fkey is None else _pad(F[fkey][:nlev]))
        add("%s_%d" % (op, flag), nlev, nout[spaces[op][2]],
            lambda eng, y, op=op, flag=flag, x=x, f=f: eng.apply(op, x, f=f, lev0=0, scale=SCALE, flags=flag, out=y),
            [P.apply(op, F[xkey][k], lev=k, scale=SCALE, flag=flag, f1=None if fkey is None else F[fkey][k]) for k in range(nlev)])
    # accumulate with alpha != 1 on a 1-form and on a 2-form result
    for op, xkey, fkey, alpha in (("UHMAT", "x1", "h2", 0.25), ("WMAT", "x2", None, -0.5)):
        ax = [P.apply(op, F[xkey][k], lev=k, scale=SCALE, flag=1, f1=None if fkey is None else F[fkey][k]) for k in range(NK)]
        base = r.standard_normal(np.shape(ax)) * np.abs(ax).mean()
        add(op + "_accum", NK, np.shape(ax)[1],
            lambda eng, y, op=op, x=D[xkey], f=None if fkey is None else D[fkey], alpha=alpha:
                eng.apply(op, x, f=f, lev0=0, scale=SCALE, flags=1 | FLAG_ACCUM, alpha=alpha, out=y),
            [base[k] + alpha * ax[k] for k in range(NK)], base=torch.as_tensor(base, device="cuda"))
    # mimsem_pvec, without and with the depth
    for name, h in (("PVEC", None), ("PHVEC", D["h2"])):
        add(name, NK, n0,
            lambda eng, y, h=h: _check_rc(eng.L.mimsem_pvec(eng.ctx, 0, NK, SCALE, None if h is None else h.data_ptr(), 0 if h is None else h.stride(0),
                                                            y.data_ptr(), y.stride(0))),
            [P.pvec(k, SCALE) if h is None else P.phvec(k, SCALE, F["h2"][k]) for k in range(NK)])
    # the upwinded shallow-water operators: departure points ~0.2 of the reference element away
    fac, dt = 0.5, 600.0
    ul = r.uniform(-1, 1, (NK, n1)) * P.det.mean() * 0.2 / (fac * dt)
    hs, qs = r.uniform(0.5, 1.5, (NK, n2)) * 1e4, r.standard_normal((NK, n0)) * 1e-4
    for which, op, xk, f1 in ((0, "PHMAT_UP", "x0", hs), (1, "ROTMAT_UP", "x1", qs)):
        add(op, NK, nout[spaces[op][2]],
            lambda eng, y, op=op, x=D[xk], f=_pad(f1), u=_pad(ul): eng.apply_up(op, x, f, u, fac, dt, lev0=0, out=y),
            [P.apply_up(which, F[xk][k], fac, dt, f1[k], ul[k])[0] for k in range(NK)])
    # the upwinded test functions: shifts ~0.3 of the reference element, from each level's own thickness
    tau = 75.0
    vs = np.array([P.det.mean() / P.thickInv[k].mean() * 0.3 / tau for k in range(NK)])[:, None]
    v1, v2 = r.uniform(-1, 1, (NK, n1)) * vs, r.uniform(-1, 1, (NK, n1)) * vs
    dv1, dv2 = _pad(v1), _pad(v2)
    for tr in (False, True):
        fl = FLAG_TRANSPOSE if tr else 0
        add("UMAT_UP" + "_T" * tr, NK, n1,
            lambda eng, y, fl=fl: eng.apply_up("UMAT_UP", D["x1"], dv1, dv2, lev0=0, scale=SCALE, tau=tau, flags=fl, out=y),
            [P.apply_testup(0, F["x1"][k], k, SCALE, tau, v1[k], v2[k], transpose=tr) for k in range(NK)])
        add("UHMAT_UP" + "_T" * tr, NK, n1,
            lambda eng, y, fl=fl: eng.apply_up("UHMAT_UP", D["x1"], D["h2"], dv1, lev0=0, scale=SCALE, tau=tau, flags=fl, out=y),
            [P.apply_testup(1, F["x1"][k], k, SCALE, tau, F["h2"][k], v1[k], transpose=tr) for k in range(NK)])
    add("UVEC_HU_UP", NK, n1,
        lambda eng, y: eng.apply_up("UVEC_HU_UP", dv1, D["h2"], dv2, lev0=0, scale=SCALE, tau=tau, alpha=1.0 / 3.0, out=y),
        [P.uvec_hu_up(k, SCALE, v1[k], F["h2"][k], 1.0 / 3.0, tau, v2[k]) for k in range(NK)])
    # Held-Suarez friction: Umat_ray (the surface field is one row: u_stride = 0), and Umat + Umat_ray in one pass
    ek = [_exner_fields(P, r, k)[0] for k in range(NK)]
    es = _exner_fields(P, r, 0)[1]
    dek, des = _pad(ek), torch.as_tensor(es, device="cuda")
    ray = [P.umat_ray(F["x1"][k], k, SCALE, 120.0, ek[k], es) for k in range(NK)]
    assert all(np.abs(em).max() > 0 for _, em in ray)                         # sigma > 0.7 somewhere on every level
    add("UMAT_RAY", NK, n1, lambda eng, y: eng.apply_ray(D["x1"], dek, des, 120.0, lev0=0, scale=SCALE, out=y), [w for w, _ in ray])
    add("UMAT_FRIC", NK, n1, lambda eng, y: eng.apply_fric(D["x1"], dek, des, 120.0, lev0=0, scale=SCALE, out=y),
        [P.apply("UMAT", F["x1"][k], lev=k, scale=SCALE, flag=1) + ray[k][0] for k in range(NK)])
    # the quad-grid projections, over several rows
    for which, op in ((0, "WTQ"), (1, "PTQ"), (2, "UTQ")):
        xq = r.standard_normal((NK, nq * (2 if which == 2 else 1)))
        add(op, NK, nout[spaces[op][2]], lambda eng, y, op=op, x=_pad(xq): eng.apply(op, x, lev0=0, scale=1.0, out=y),
            [P.project_from_quad(which, xq[k]) for k in range(NK)])
    # mimsem_op_apply_levels with step 0: every row at geometry level 4
    for op, xkey, fkey in (("WMAT", "x2", None), ("UHMAT", "x1", "h2")):
        add(op + "_step0", NK, nout[spaces[op][2]],
            lambda eng, y, op=op, x=D[xkey], f=None if fkey is None else D[fkey]: eng.apply_levels(op, x, 0, f=f, lev0=4, scale=SCALE, flags=1, out=y),
            [P.apply(op, F[xkey][k], lev=4, scale=SCALE, flag=1, f1=None if fkey is None else F[fkey][k]) for k in range(NK)])
    # a sub-range of the levels: 2 .. 6, two levels per work item in test (a)
    for op, flag, fkey, xkey in (("UHMAT", 1, "h2", "x1"), ("PHMAT", 0, "h2", "x0"), ("WHMAT", 1, "h2", "x2"), ("WTQUMAT", 0, "u1", "x1")):
        add(op + "_lev2to6", 5, nout[spaces[op][2]],
            lambda eng, y, op=op, flag=flag, x=_pad(F[xkey][2:7]), f=_pad(F[fkey][2:7]): eng.apply(op, x, f=f, lev0=2, scale=SCALE, flags=flag, out=y),
            [P.apply(op, F[xkey][k], lev=k, scale=SCALE, flag=flag, f1=F[fkey][k]) for k in range(2, 7)], lch_a=2)
    _PATCHES[pn] = (dm, P, calls)
    return _PATCHES[pn]


def _check_rc(rc):
    assert rc == 0, rc


@pytest.mark.parametrize("pn", sorted(PATCH_PI))
def test_element_pass_every_level_matches_oracle(oracle, pn):
    """(a) three levels per work item (two for the sub-range calls), one call over all levels, every level against the oracle"""
    from mimsem_amd.device import Engine
    dm, P, calls = _patch(oracle, pn)
    eng = Engine(dm)
    worst = ("", -1, 0.0)
    try:
        for c in calls:
            _engage(eng, c.lch_a, c.nlev)
            y = c(eng).cpu().numpy()
            for k in range(c.nlev):
                err = rel_l2(y[k], c.want[k])
                if err > worst[2]:
                    worst = (c.name, k, err)
                assert err < TOL, (c.name, k, err)
    finally:
        eng.set_level_chunk(0)
        print("p = %d: worst relative error against the oracle %.2e (%s, row %d) over %d calls" % (pn, worst[2], worst[0], worst[1], len(calls)))


@pytest.mark.parametrize("pn", sorted(PATCH_PI))
def test_element_pass_same_bits_at_every_chunk_size(oracle, pn):
    """(b) the calls of (a) with 2, 3, 4 and 8 levels per work item: the bits of one level per work item"""
    import torch
    from mimsem_amd.device import Engine
    dm, P, calls = _patch(oracle, pn)
    eng = Engine(dm)
    try:
        _engage(eng, 1, NK)
        one = [c(eng).clone() for c in calls]
        for c, y1 in zip(calls, one):                                            # (and lch = 1 itself is right: the oracle again)
            assert max(rel_l2(y1[k].cpu().numpy(), c.want[k]) for k in range(c.nlev)) < TOL, c.name
        for lch in CHUNKS:
            for c, y1 in zip(calls, one):
                _engage(eng, lch, c.nlev)
                y = c(eng)
                assert torch.equal(y, y1), (c.name, lch, float((y - y1).abs().max()))
    finally:
        eng.set_level_chunk(0)


# ---- (c): sweeps and fixed-length solves on the closed sphere --------------------------------------------------------------------------
_SPHERES = {}


def _sphere_mesh(pn):
    """the closed 2 x 2 x 6 sphere of order pn with 11 stretched levels: 24 elements, global numbering, every slot owned"""
    if pn not in _SPHERES:
        from tests.test_gpu_pc_bjacobi_owned import _sphere
        *_, dm, eng = _sphere(pn, ne=2, nk=NK, seed=40 + pn)
        del eng
        assert dm.nEl == 24
        _SPHERES[pn] = dm
    return _SPHERES[pn]


def _sphere_exner(dm, r):
    """_exner_fields of tests/test_gpu_horizontal.py from the mesh's own metric: 2-form DoFs whose point values (after / det * thickInv) are
    Exner pressures cp sigma^(R/cp), sigma in [0.5, 1] per element and level, [0.98, 1.02] for the surface row"""
    from mimsem_amd.geom import gll_points
    n = dm.n
    dx = np.diff(gll_points(n))
    cell = np.outer(dx, dx).reshape(-1)

    def row(k, lo, hi):
        f = np.zeros(dm.n2)
        for e in range(dm.nEl):
            val = 1004.5 * r.uniform(lo, hi) ** (287.0 / 1004.5)
            f[dm.inds2[e]] = val * cell * (dm.det[e].mean() / dm.thickInv[k, e].mean()) * (1.0 + 1e-3 * r.standard_normal(n * n))
        return f
    return np.stack([row(k, 0.5, 1.0) for k in range(NK)]), row(0, 0.98, 1.02)


def _sweeps(eng, S):
    """every sweep and solve of test (c) on fresh buffers: {name: rows of the result}"""
    import torch
    out = {}

    def buf(name, base=None, n=None):
        out[name] = _result(NK, eng.sizes[1] if n is None else n, base)
        return out[name][:-1]

    n0 = eng.sizes[0]
    # Richardson and Chebyshev sweeps on the upwinded lumped 0-form operator and on the 1-form mass operator
    x = buf("rich0_x", S["x0"], n0); u = buf("rich0_upd", None, n0)
    eng.richardson_sweep("PHMAT_UP", x, S["b0"], S["dinv0"], f=S["h"], u=S["ul"], tau=S["tau"], upd=u)
    x = buf("cheb0_x", S["x0"], n0); p = buf("cheb0_p", S["p0"], n0); u = buf("cheb0_upd", None, n0)
    eng.chebyshev_sweep("PHMAT_UP", x, S["b0"], S["dinv0"], p, 0.9, 0.3, f=S["h"], u=S["ul"], tau=S["tau"], upd=u)
    x = buf("rich1_x", S["x1"]); u = buf("rich1_upd")
    eng.richardson_sweep("UMAT", x, S["b1"], S["dinv1"], scale=SCALE, flags=1, upd=u)
    x = buf("cheb1_x", S["x1"]); p = buf("cheb1_p", S["p1"]); u = buf("cheb1_upd")
    eng.chebyshev_sweep("UMAT", x, S["b1"], S["dinv1"], p, 0.9, 0.3, scale=SCALE, flags=1, upd=u)
    # one block-Chebyshev sweep from a given iterate
    x = buf("bcheb_x", S["x1"]); p = buf("bcheb_p", S["p1"]); u = buf("bcheb_upd")
    eng.block_chebyshev_sweep("UMAT", S["cm"], x, S["b1"], p, 1.9, 0.37, elem_scale=S["esc"], scale=SCALE, flags=1, upd=u)
    # the whole fixed-length solve, and the same steps as sweeps from x = 0
    x = buf("solve_x"); pb = buf("solve_pb"); u = buf("solve_upd")
    eng.block_chebyshev_solve("UMAT", S["cm"], S["b1"], COEF, x=x, elem_scale=S["esc"], scale=SCALE, flags=1, pb=pb, upd=u)
    x = buf("steps_x", 0.0); p = buf("steps_p", 7.0); first = buf("steps_first"); last = buf("steps_last")
    for k, (al, be) in enumerate(COEF):
        eng.block_chebyshev_sweep("UMAT", S["cm"], x, S["b1"], p, al, be, elem_scale=S["esc"], scale=SCALE, flags=1,
                                  upd=first if k == 0 else (last if k == len(COEF) - 1 else None))
    # ... and with Held-Suarez friction in the operator
    x = buf("fric_x"); pb = buf("fric_pb"); u = buf("fric_upd")
    eng.fric_chebyshev_solve(S["cm"], S["b1"], COEF, 240.0, S["ex"], S["exs"], x=x, elem_scale=S["esc"], scale=SCALE, flags=1, pb=pb, upd=u)
    return {k: _checked(v, k) for k, v in out.items()}


@pytest.mark.parametrize("pn", [2, 3, 4, 5])
def test_sweeps_and_solves_same_bits_at_every_chunk_size(pn):
    """(c) mimsem_op_richardson_sweep / _chebyshev_sweep (PHMAT_UP, UMAT), mimsem_block_chebyshev_sweep, mimsem_block_chebyshev_solve (8 steps,
    pb and upd given) and mimsem_fric_chebyshev_solve with 2, 3 and 8 levels per work item: the bits of one level per work item; and the whole
    solve has the bits of its steps as sweeps from x = 0, at every chunk size"""
    import torch
    from mimsem_amd.device import Engine
    dm = _sphere_mesh(pn)
    eng = Engine(dm)
    r = np.random.default_rng(300 + pn)
    n0, n1, n2 = eng.sizes[0], eng.sizes[1], eng.sizes[2]
    tau = 0.5 * 600.0
    S = dict(tau=tau, x0=_pad(r.standard_normal((NK, n0))), p0=_pad(r.standard_normal((NK, n0))), b0=_pad(r.standard_normal((NK, n0))),
             x1=_pad(r.standard_normal((NK, n1))), p1=_pad(r.standard_normal((NK, n1))), b1=_pad(r.standard_normal((NK, n1)) * 1e3),
             h=_pad(r.uniform(0.5, 1.5, (NK, n2)) * 1e4), ul=_pad(r.uniform(-1, 1, (NK, n1)) * np.abs(dm.det).mean() * 0.2 / tau),
             esc=_pad(r.uniform(0.8, 1.2, (NK, eng.nEl)) / dm.thickInv.mean(axis=2)))       # ~ MassSolver's 1 / mean(thickInv) per level and element
    ex, exs = _sphere_exner(dm, r)
    S["ex"], S["exs"] = _pad(ex), torch.as_tensor(exs, device="cuda")
    try:
        # the diagonal scalings and the blocks need not be good preconditioners here, only of the operators' size: made once, at the library's rule
        y0 = eng.apply_up("PHMAT_UP", S["x0"], S["h"], S["ul"], tau=tau, lev0=0)
        y1 = eng.apply("UMAT", S["x1"], lev0=0, scale=SCALE, flags=1)
        assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(y1).all())
        for key, y, x in (("dinv0", y0, S["x0"]), ("dinv1", y1, S["x1"])):
            s = (torch.linalg.vector_norm(x, dim=1) / torch.linalg.vector_norm(y, dim=1)).cpu().numpy()
            S[key] = _pad(r.uniform(0.5, 1.0, tuple(x.shape)) * s[:, None])
        S["cm"] = eng.elem_block_pc("UMAT", lev=0, scale=SCALE, flags=0).transpose(1, 2).contiguous()     # (without the thickness: esc carries it)
        _engage(eng, 1, NK)
        one = _sweeps(eng, S)
        assert not torch.equal(one["fric_x"], one["solve_x"])                        # the friction is in the operator
        for lch in (1, 2, 3, 8):
            _engage(eng, lch, NK)
            got = one if lch == 1 else _sweeps(eng, S)
            for name in one:
                assert torch.equal(got[name], one[name]), (name, lch, float((got[name] - one[name]).abs().max()))
            for a, b in (("solve_x", "steps_x"), ("solve_pb", "steps_first"), ("solve_upd", "steps_last")):
                assert torch.equal(got[a], got[b]), (a, lch)
    finally:
        eng.set_level_chunk(0)


# ---- (d): block applies with shared blocks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", sorted(PATCH_PI))
def test_shared_block_applies(oracle, pn):
    """(d) mimsem_elem_blocks_apply with one set of blocks for all levels (register-resident rows up to 64 rows, LDS-resident blocks above:
    the 1-form blocks of orders 6 and 7): forms 0, 1, 2, plain and transposed, with and without elem_scale, alpha = 0.5, accumulate on form 2 --
    against the dense numpy loop of test_element_blocks_apply_level_sweep at its bound, at 1, 2, 3 and 8 levels per work item, and the same
    bits at every chunk size"""
    import torch
    from mimsem_amd.device import Engine
    dm, P, _ = _patch(oracle, pn)
    eng = Engine(dm)
    r = np.random.default_rng(640 + pn)
    idx = {0: P.elinds("n0"), 2: P.elinds("n2"), 1: np.concatenate([P.elinds("n1x"), P.elinds("n1y")], axis=1)}
    cases = []
    for form, nd, nv in ((0, P.n0e, P.n0), (1, 2 * P.n1e, P.n1), (2, P.n2e, P.n2)):
        B = r.standard_normal((P.nEl, nd, nd)); xv = r.standard_normal((NK, nv)); sc = r.uniform(0.5, 2.0, (NK, P.nEl))
        base = r.standard_normal((NK, nv)) * nd ** 0.5
        dB, dx, dsc = torch.as_tensor(B, device="cuda"), _pad(xv), _pad(sc)
        for tr in (False, True):
            for scale in (None, sc):
                for alpha, accum in ((1.0, False), (0.5, False)) + (((0.5, True),) if form == 2 else ()):
                    ref = np.zeros((NK, nv))
                    for lev in range(NK):
                        for e in range(P.nEl):
                            Be = (B[e].T if tr else B[e]) * (1.0 if scale is None else scale[lev, e])
                            ref[lev, idx[form][e]] += Be @ xv[lev, idx[form][e]]
                    ref = alpha * ref + (base if accum else 0.0)
                    cases.append(((form, tr, scale is not None, alpha, accum), nv, ref, torch.as_tensor(base, device="cuda") if accum else None,
                                  dict(form=form, blocks=dB, x=dx, transpose=tr, alpha=alpha, accum=accum, elem_scale=None if scale is None else dsc)))
    try:
        one = {}
        for lch in (1, 2, 3, 8):
            _engage(eng, lch, NK)
            for key, nv, ref, base, kw in cases:
                buf = _result(NK, nv, base)
                eng.blocks_apply(out=buf[:-1], **kw)
                y = _checked(buf, key)
                assert rel_l2(y.cpu().numpy(), ref) < 1e-12, (key, lch)
                if lch == 1:
                    one[key] = y.clone()
                else:
                    assert torch.equal(y, one[key]), (key, lch, float((y - one[key]).abs().max()))
    finally:
        eng.set_level_chunk(0)


# ---- (e): the owned-block pass ------------------------------------------------------------------------------------------------------------
def _row_err(a, b):
    import torch
    return float((torch.linalg.vector_norm(a - b, dim=1) / torch.linalg.vector_norm(b, dim=1)).max())


@pytest.mark.parametrize("pn", sorted(PATCH_PI))
def test_owned_block_pass(pn):
    """(e) mimsem_owned_blocks_apply with shared inverse blocks at requests of 1, 2, 4 and 8 levels per work item (the compile-time level
    counts of k_owned_pass, blocks of 8 .. 98 rows; the rows of orders 6 and 7 are read from memory, not kept in registers): against an fp64
    einsum with numpy's inverses of the assembled blocks at 1e-12 per level, and against the call with a set of blocks per level (one level per
    work item) at 1e-14 per row; mimsem_owned_block_chebyshev_solve (orders <= 5: its first-step and later-step passes) the same way at 1e-13.
    The kernels differ in their compile-time level count: tolerances, not bit equality.  A closed sphere has no slot outside every block:
    results start as NaN and must be finite."""
    import torch
    from mimsem_amd.device import Engine
    dm = _sphere_mesh(pn)
    eng = Engine(dm)
    nd, n1 = 2 * pn * pn, eng.sizes[1]
    assert eng.owned_covers_all(1) and n1 == eng.nEl * nd
    r = np.random.default_rng(500 + pn)
    try:
        B = eng.owned_blocks("UMAT")[0]
        Binv = eng.owned_blocks("UMAT", invert=True)[0].contiguous()
        Blev = Binv.expand(NK, *Binv.shape).contiguous()
        xv = r.standard_normal((NK, n1))
        want = np.einsum("kij,lkj->lki", np.linalg.inv(B.cpu().numpy()), xv.reshape(NK, -1, nd)).reshape(NK, -1)   # chunk k = block k's rows
        x, b = _pad(xv), _pad(r.standard_normal((NK, n1)))
        buf = _result(NK, n1)
        eng.owned_blocks_apply(1, Blev, x, out=buf[:-1])
        y_lev = _checked(buf, "per-level blocks").clone()
        solve = pn <= 5
        if solve:
            bufs = [_result(NK, n1) for _ in range(3)]
            eng.owned_block_chebyshev_solve(Blev, b, COEF, x=bufs[0][:-1], pb=bufs[1][:-1], upd=bufs[2][:-1])
            s_lev = [_checked(t, "solve, per-level blocks").clone() for t in bufs]
        for req in (1, 2, 4, 8):
            _engage(eng, req, NK)
            buf = _result(NK, n1)
            eng.owned_blocks_apply(1, Binv, x, out=buf[:-1])
            y = _checked(buf, ("apply", req))
            yc = y.cpu().numpy()
            for lev in range(NK):
                assert rel_l2(yc[lev], want[lev]) < 1e-12, (req, lev)
            assert _row_err(y, y_lev) < 1e-14, req
            if solve:
                bufs = [_result(NK, n1) for _ in range(3)]
                eng.owned_block_chebyshev_solve(Binv, b, COEF, x=bufs[0][:-1], pb=bufs[1][:-1], upd=bufs[2][:-1])
                for t, ref, name in zip(bufs, s_lev, ("x", "pb", "upd")):
                    assert _row_err(_checked(t, ("solve", req, name)), ref) < 1e-13, (req, name)
    finally:
        eng.set_level_chunk(0)


# ---- (f): the setting itself ------------------------------------------------------------------------------------------------------------
def test_level_chunk_setting(oracle):
    import torch
    from mimsem_amd import _lib
    from mimsem_amd.device import Engine, check
    dm, P, calls = _patch(oracle, 3)
    eng = Engine(dm)
    L = eng.L
    chunk = lambda nlev=NK: L.mimsem_op_level_chunk(eng.ctx, nlev)
    own = [chunk(n) for n in range(1, NK + 1)]                   # the library's own values, before any request
    try:
        assert own == [1] * NK                                                       # nine elements: one level per work item
        assert L.mimsem_ctx_set_level_chunk(eng.ctx, 5) == 0 and chunk() == 5
        for bad in (-1, 9):
            assert L.mimsem_ctx_set_level_chunk(eng.ctx, bad) == -1 and chunk() == 5    # MIMSEM_ERR_ARG, nothing changed
            with pytest.raises(_lib.MimsemError):
                eng.set_level_chunk(bad)
            assert chunk() == 5
        assert L.mimsem_ctx_set_level_chunk(None, 2) == -1
        for lch in range(1, 9):
            eng.set_level_chunk(lch)
            assert [chunk(n) for n in range(1, NK + 1)] == [min(lch, n) for n in range(1, NK + 1)]     # a request is clamped to the call's levels
        eng.set_level_chunk(0)
        assert [chunk(n) for n in range(1, NK + 1)] == own                         # 0: the library's rule again
        # not inside a recording
        c = next(c for c in calls if c.name == "WMAT_1")
        y = _result(c.nlev, c.nout)
        c.run(eng, y[:-1])                                                          # (workspaces reach their size outside the capture)
        eng.sync(); torch.cuda.synchronize()
        g = C.c_void_p()
        check(L.mimsem_graph_begin(eng.ctx), "graph_begin")
        try:
            rc = L.mimsem_ctx_set_level_chunk(eng.ctx, 4)
            seen = chunk()
            c.run(eng, y[:-1])
        finally:
            rc_end = L.mimsem_graph_end(eng.ctx, C.byref(g))
        check(rc_end, "graph_end")
        L.mimsem_graph_destroy(g)
        torch.cuda.synchronize()
        assert rc == -4 and seen == 1                                               # MIMSEM_ERR_STATE, nothing changed
        assert chunk() == 1
    finally:
        eng.set_level_chunk(0)
