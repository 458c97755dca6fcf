"""Every C-ABI entry that takes a row stride, called with a DISTINCT stride per operand (include/mimsem_hip.h: a multi-level field is
base + k*stride, each operand with a stride of its own).  The Python wrappers hand the library one contiguous block per operand, so in the
rest of the suite all strides of a call are equal and a kernel that walks x with y's stride passes.  Here every entry runs through
tests/stride_case.py: contiguous, then "even" (distinct strides, 16-byte alignment kept) and "odd" (odd strides, bases 8 bytes off a
16-byte boundary), and the strided runs must give the BITS of the contiguous one, leave every word around their rows alone and their
inputs unchanged.  The contiguous result is compared with the entry's reference (the one its existing test uses, with that test's
tolerance); bit equality carries that comparison over to the strided runs.

tests/test_abi_stride_coverage.py holds COVERED | EXCLUDED against the header: a new strided entry point fails there until it has a case.

Run the layouts apart on the GPU:  pytest -m gpu tests/test_gpu_abi_strides.py -k even   /   -k odd."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import stride_case as sc
from tests.helpers import SCALE, make_patch, rel_l2, z_levels
from tests.stride_case import Case, Operand

pytestmark = pytest.mark.gpu

TOL = 1e-10                               # tests/test_gpu_horizontal.py, tests/test_gpu_column.py (TOL), tests/test_gpu_wave.py (oracle)
NK_A = 12
OPS = dict(UMAT=0, WMAT=1, UHMAT=2, PMAT=3, PHMAT=4, WTQUMAT=5, ROTMAT=6, WHMAT=7, UTMAT=8, UTMAT_H=9, UTQWMAT=10, WTQDUDZ=11,
           PHMAT_UP=14, ROTMAT_UP=15, UMAT_UP=19, UHMAT_UP=20, UVEC_HU_UP=21, UMAT_RAY=22, UMAT_FRIC=23)
SPACES = dict(UMAT=(1, None, 1), UTMAT=(1, None, 1), UHMAT=(1, 2, 1), UTMAT_H=(1, 2, 1), ROTMAT=(1, 0, 1), WMAT=(2, None, 2), WHMAT=(2, 2, 2),
              PMAT=(0, None, 0), PHMAT=(0, 2, 0), WTQUMAT=(1, 1, 2), WTQDUDZ=(1, 1, 2), UTQWMAT=(2, 1, 1))

# entries without a case here, each with its reason (tests/test_abi_stride_coverage.py allows these eight names and no others)
EXCLUDED = {
    "mimsem_ksp_set_operator": "solver object: driven from tests/cpp/test_ksp*.cpp",
    "mimsem_ksp_set_operator_sw": "solver object: driven from tests/cpp/test_ksp*.cpp",
    "mimsem_ksp_set_pc_jacobi": "solver object: driven from tests/cpp/test_ksp*.cpp",
    "mimsem_ksp_set_pc_elem_blocks": "solver object: driven from tests/cpp/test_ksp*.cpp",
    "mimsem_ksp_solve": "solver object: driven from tests/cpp/test_ksp*.cpp",
    "mimsem_halo_begin": "needs a transport between peers",
    "mimsem_sw_chebyshev_step2": "chain protocol with one v_stride shared by six vectors",
    "mimsem_sw_chebyshev_flush": "chain protocol with one v_stride shared by its vectors",
}

CASES = {}                                # case id -> (entry, builder(W) -> (engine, Case))


def _reg(entry, cid, fn, *a, **kw):
    assert cid not in CASES, cid
    CASES[cid] = (entry, lambda W: fn(W, *a, **kw))


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _field(r, form, shape):
    """coefficient fields at the magnitudes of tests/test_gpu_fullsize_oracle.py"""
    if form == 0:
        return r.standard_normal(shape) * 1e-4
    if form == 1:
        return r.standard_normal(shape) * 1e3
    return r.uniform(0.5, 1.5, shape) * 1e6


# ---- meshes, engines and oracles, built once ---------------------------------------------------------------------------------------
class World:
    def __init__(self, oracle):
        self.oracle, self._m, self._e, self._c = oracle, {}, {}, {}

    def cached(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def mesh(self, name):
        """A: the sphere of tests/test_gpu_wave_own4.py (p = 3, ne = 4, 6 patches, global numbering) with nk = 12; B, C: one patch in the
        local layout (orders 4 and 5); D: the first column mesh of tests/test_gpu_column.py; S: the shallow-water sphere"""
        if name in self._m:
            return self._m[name]
        from mimsem_amd.device import DeviceMesh
        if name == "A":
            from mimsem_amd.geom import Geom
            from mimsem_amd.mesh import CubedSphere, sphere_coords
            from mimsem_amd.topo import Topo
            from tests.test_gpu_fullsize_oracle import PatchView, _oracle_patch
            cs = CubedSphere(3, 4, 6); coords = sphere_coords(3, 4)
            topos = [Topo(cs, p, NK_A) for p in range(6)]
            geoms = [Geom(t, cs, coords, NK_A) for t in topos]
            for g in geoms:
                g.set_levels(z_levels(NK_A, g.n0))
            dm = DeviceMesh(topos, geoms, nk=NK_A, numbering="global")
            patches = []
            for pi in range(6):
                patches.append((PatchView(dm, topos, pi), _oracle_patch(self.oracle, cs, coords, geoms[pi], pi, NK_A)))
            m = dict(dm=dm, patches=patches)
        elif name == "S":               # the shallow-water sphere of tests/test_gpu_sweqn.py: one level of unit thickness (the src/ flavour has no vertical)
            from mimsem_amd.geom import Geom
            from mimsem_amd.mesh import CubedSphere, sphere_coords
            from mimsem_amd.topo import Topo
            cs = CubedSphere(3, 2, 6); coords = sphere_coords(3, 2)
            topos = [Topo(cs, p, 1) for p in range(6)]
            geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
            for g in geoms:
                g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
            m = dict(dm=DeviceMesh(topos, geoms, nk=1, numbering="global"))
        else:
            pn, ne, npr, pi, nk = {"B": (4, 2, 6, 3, 3), "C": (5, 1, 6, 2, 3), "D": (3, 2, 6, 1, 6)}[name]
            cs, topo, geom, P, rng = make_patch(self.oracle, pn, ne, npr, pi, nk=nk)
            m = dict(dm=DeviceMesh([topo], [geom], nk=nk, numbering="local"), P=P)
        self._m[name] = m
        return m

    def eng(self, mesh="A", key="default"):
        """engines by the switches of their creation: default, own1 / own0 (MIMSEM_WAVE_OWN), wave0 (MIMSEM_WAVE=0), balance (default +
        set_wave_balance(5, 2): a chip of tests/test_gpu_wave_balance.py CHIPS), halo (default + marked halo slots, for split applies)"""
        if (mesh, key) not in self._e:
            from tests.test_gpu_wave_own4 import _engine
            env = dict(MIMSEM_WAVE=None, MIMSEM_WAVE_OWN=None, MIMSEM_WAVE_BALANCE=None)
            env.update({"own1": {"MIMSEM_WAVE_OWN": "1"}, "own0": {"MIMSEM_WAVE_OWN": "0"}, "wave0": {"MIMSEM_WAVE": "0"}}.get(key, {}))
            e = _engine(self.mesh(mesh)["dm"], **env)
            if key == "balance":
                e.set_wave_balance(5, 2)
            if key == "halo":
                e.set_halo_slots(1, np.arange(0, e.sizes[1], 7))
            self._e[(mesh, key)] = e
        return self._e[(mesh, key)]

    def pool(self, mesh, op, rows=9):
        """x, f and the initial y of an operator, the same for every case of that operator (their oracle results are shared)"""
        def make():
            e = self.eng(mesh)
            sin, sf, sout = SPACES[op]
            r = np.random.default_rng(_seed(mesh, op))
            return dict(x=r.standard_normal((rows, e.sizes[sin])), f=None if sf is None else _field(r, sf, (rows, e.sizes[sf])),
                        y=r.standard_normal((rows, e.sizes[sout])))
        return self.cached(("pool", mesh, op), make)

    def oracle_apply(self, mesh, op, fl, lev, k):
        """[(slots, mask, want)] of P.apply on row k of the pool at geometry level lev: one entry for a local mesh, one per patch on mesh A"""
        def make():
            sin, sf, sout = SPACES[op]
            p = self.pool(mesh, op)
            m = self.mesh(mesh)
            if mesh != "A":
                want = m["P"].apply(op, p["x"][k], lev=lev, scale=SCALE, flag=fl, f1=None if sf is None else p["f"][k])
                return [(slice(None), slice(None), want)]
            out = []
            for v, P in m["patches"]:
                want = P.apply(op, p["x"][k][v.slots[sin]], lev=lev, scale=SCALE, flag=fl, f1=None if sf is None else p["f"][k][v.slots[sf]])
                out.append((v.slots[sout], v.mask[sout], want))
            return out
        return self.cached(("want", mesh, op, fl, lev, k), make)


_WORLD = {}


@pytest.fixture(scope="module")
def world(oracle):
    if "w" not in _WORLD:
        _WORLD["w"] = World(oracle)
    yield _WORLD["w"]
    _WORLD.clear(); _BASE.clear()


# ---- element applies --------------------------------------------------------------------------------------------------------------
def apply_case(W, mesh, engkey, op, nlev, lev0, fl, accum=False, how="apply"):
    """mimsem_op_apply / _part (BOUNDARY then INTERIOR) / _levels (step 0) against the CPU oracle's P.apply at TOL (tests/test_gpu_horizontal.py;
    on the global mesh A patch by patch on the slots no other patch contributes to, as tests/test_gpu_wave.py does)"""
    eng = W.eng(mesh, engkey)
    sin, sf, sout = SPACES[op]
    p = W.pool(mesh, op)
    alpha = 0.25 if accum else 1.0
    flags = fl | (2 if accum else 0)
    ops = ([Operand("f", p["f"][:nlev])] if sf is not None else []) + [Operand("x", p["x"][:nlev]), Operand("y", p["y"][:nlev], "inout" if accum else "out")]
    code = OPS[op]

    def call(eng, a):
        L, c = eng.L, eng.ctx
        if how == "part":
            rc = L.mimsem_op_apply_part(c, code, lev0, nlev, SCALE, flags, *a["f"], *a["x"], *a["y"], alpha, 1)
            return rc or L.mimsem_op_apply_part(c, code, lev0, nlev, SCALE, flags, *a["f"], *a["x"], *a["y"], alpha, 2)
        if how == "levels":
            return L.mimsem_op_apply_levels(c, code, lev0, 0, nlev, SCALE, flags, *a["f"], *a["x"], *a["y"], alpha)
        n0 = int(L.mimsem_ctx_wave_balance_launches(c))
        rc = L.mimsem_op_apply(c, code, lev0, nlev, SCALE, flags, *a["f"], *a["x"], *a["y"], alpha)
        if engkey == "balance":
            # 24 groups on a pretended chip of 5 CUs x 2: the planner engages at 9 levels (12 workgroups of the default rule, not a multiple of
            # 5); at 2 and 5 levels it cannot fill 10 workgroups and the default rule stays (tests/test_wave_balance_cpu.py restates both)
            assert int(L.mimsem_ctx_wave_balance_launches(c)) - n0 == (1 if nlev == 9 else 0), "the planned-list kernel did not run"
        return rc

    def ref(ins, outs):
        for k in range(nlev):
            for slots, mask, want in W.oracle_apply(mesh, op, fl, lev0 if how == "levels" else lev0 + k, k):
                want = alpha * want + (ins["y"][k][slots] if accum else 0.0)
                assert rel_l2(outs["y"][k][slots][mask], want[mask]) < TOL, (op, k)

    entry = {"apply": "mimsem_op_apply", "part": "mimsem_op_apply_part", "levels": "mimsem_op_apply_levels"}[how]
    return eng, Case(entry, ops, call, ref)


for _ek in ("default", "own1", "own0", "wave0", "balance"):
    for _fl in (0, 1):
        for _acc in (False, True):
            for _nl in (2, 5, 9):
                for _l0 in (0, 1):
                    _reg("mimsem_op_apply", "apply_A_%s_UMAT_fl%d%s_n%d_l%d" % (_ek, _fl, "_acc" if _acc else "", _nl, _l0), apply_case, "A", _ek, "UMAT",
                         _nl, _l0, _fl, _acc)
for _ek in ("default", "wave0"):
    for _op, _fl in (("UHMAT", 1), ("ROTMAT", 0), ("UTMAT", 0), ("UTMAT_H", 0), ("WHMAT", 1), ("WTQUMAT", 0), ("WTQDUDZ", 0)):
        _reg("mimsem_op_apply", "apply_A_%s_%s" % (_ek, _op), apply_case, "A", _ek, _op, 5, 1, _fl)
for _op, _fl in (("WMAT", 1), ("UTQWMAT", 0), ("PMAT", 0), ("PHMAT", 0)):
    _reg("mimsem_op_apply", "apply_A_default_%s" % _op, apply_case, "A", "default", _op, 5, 1, _fl)
for _m in ("B", "C"):
    for _op in ("UMAT", "UHMAT", "WMAT"):
        _reg("mimsem_op_apply", "apply_%s_%s" % (_m, _op), apply_case, _m, "default", _op, 3, 0, 1)
for _op in ("UMAT", "UHMAT"):
    _reg("mimsem_op_apply_part", "part_A_%s" % _op, apply_case, "A", "halo", _op, 5, 1, 1, False, "part")
for _op in ("WMAT", "UHMAT"):
    _reg("mimsem_op_apply_levels", "levels_A_%s" % _op, apply_case, "A", "default", _op, 3, 2, 1, False, "levels")


def _exner(W, r, levs):
    """Exner rows of the levels `levs` and the row of level 0 on mesh A, patch by patch with _exner_fields of tests/test_gpu_horizontal.py"""
    from tests.test_gpu_horizontal import _exner_fields
    dm = W.mesh("A")["dm"]
    ek, es = np.zeros((len(levs), dm.n2)), np.zeros((1, dm.n2))
    for v, P in W.mesh("A")["patches"]:
        for k, lev in enumerate(levs):
            ek[k][v.s2], es[0][v.s2] = _exner_fields(P, r, lev)
    return ek, es


def apply_up_case(W, op):
    """mimsem_op_apply_up on mesh A, four operands; the oracle calls and TOL of tests/test_gpu_horizontal.py (test_upwinded_sw_operators,
    test_eul_upwinded_test_functions, test_umat_ray_held_suarez_friction), patch by patch as in apply_case"""
    eng = W.eng("A")
    dm, patches = W.mesh("A")["dm"], W.mesh("A")["patches"]
    P0 = patches[0][1]
    r = np.random.default_rng(_seed("up", op))
    nlev, alpha, bc = 3, 1.0, False
    n0, n1, n2 = dm.n0, dm.n1, dm.n2
    if op in ("PHMAT_UP", "ROTMAT_UP"):
        lev0, scale, fac, dt = 0, 1.0, 0.5, 600.0
        tau = 1.0 / (1.0 / (fac * dt))
        u = r.uniform(-1, 1, (nlev, n1)) * P0.det.mean() * 0.2 / (fac * dt)
        f, x = (r.uniform(0.5, 1.5, (nlev, n2)) * 1e4, r.standard_normal((nlev, n0))) if op == "PHMAT_UP" else \
               (r.standard_normal((nlev, n0)) * 1e-4, r.standard_normal((nlev, n1)))
        sout = 0 if op == "PHMAT_UP" else 1
        want = lambda v, P, k: P.apply_up(0 if op == "PHMAT_UP" else 1, x[k][v.slots[sout]], fac, dt, f[k][v.s2 if op == "PHMAT_UP" else v.s0], u[k][v.s1])[0]
    elif op in ("UMAT_UP", "UHMAT_UP", "UVEC_HU_UP"):
        lev0, scale, tau, sout = 1, SCALE, 75.0, 1
        vs = np.array([P0.det.mean() / P0.thickInv[lev0 + k].mean() * 0.3 / tau for k in range(nlev)])[:, None]
        u1, u2 = r.uniform(-1, 1, (nlev, n1)) * vs, r.uniform(-1, 1, (nlev, n1)) * vs
        h = r.uniform(0.5, 1.5, (nlev, n2)) * 1e6
        if op == "UMAT_UP":
            f, u, x = u1, u2, r.standard_normal((nlev, n1))
            want = lambda v, P, k: P.apply_testup(0, x[k][v.s1], lev0 + k, SCALE, tau, f[k][v.s1], u[k][v.s1])
        elif op == "UHMAT_UP":
            f, u, x = h, u1, r.standard_normal((nlev, n1))
            want = lambda v, P, k: P.apply_testup(1, x[k][v.s1], lev0 + k, SCALE, tau, f[k][v.s2], u[k][v.s1])
        else:
            f, u, x, alpha = h, u2, u1, 1.0 / 3.0
            want = lambda v, P, k: P.uvec_hu_up(lev0 + k, SCALE, x[k][v.s1], f[k][v.s2], 1.0, tau, u[k][v.s1])
    else:
        lev0, scale, tau, sout, bc = 2, SCALE, 120.0, 1, True
        f, u = _exner(W, r, [lev0 + k for k in range(nlev)])
        x = r.standard_normal((nlev, n1))

        def want(v, P, k):
            w = P.umat_ray(x[k][v.s1], lev0 + k, SCALE, tau, f[k][v.s2], u[0][v.s2])[0]
            return w + P.apply("UMAT", x[k][v.s1], lev=lev0 + k, scale=SCALE, flag=1) if op == "UMAT_FRIC" else w
    y0 = r.standard_normal((nlev, (n0, n1)[sout]))
    ops = [Operand("f", f), Operand("u", u, broadcast=bc), Operand("x", x), Operand("y", y0, "out")]

    def call(eng, a):
        return eng.L.mimsem_op_apply_up(eng.ctx, OPS[op], lev0, nlev, scale, tau, 0, *a["f"], *a["u"], *a["x"], *a["y"], alpha)

    def ref(ins, outs):
        for k in range(nlev):
            for v, P in patches:
                w, m = alpha * want(v, P, k), v.mask[sout]
                assert rel_l2(outs["y"][k][v.slots[sout]][m], w[m]) < TOL, (op, k)
    return eng, Case("mimsem_op_apply_up", ops, call, ref)


for _op in ("PHMAT_UP", "ROTMAT_UP", "UMAT_UP", "UHMAT_UP", "UVEC_HU_UP", "UMAT_RAY", "UMAT_FRIC"):
    _reg("mimsem_op_apply_up", "up_A_%s" % _op, apply_up_case, _op)


# ---- other element-level entries --------------------------------------------------------------------------------------------------
def _elem_idx(dm, form):
    return {0: dm.inds0, 1: np.concatenate([dm.inds1x, dm.inds1y], axis=1), 2: dm.inds2}[form]


def blocks_apply_case(W, form, per_level, transpose):
    """both block layouts: a set per level (blocks_level_stride a stride of its own) / one set with elem_scale rows at a stride != nEl.
    Reference and 1e-12: the loops of tests/test_gpu_horizontal.py test_element_blocks_apply(_level_sweep)"""
    eng = W.eng("B")
    dm = eng.mesh
    r = np.random.default_rng(_seed("blocks", form, per_level))
    nlev, nd, nv, nEl = 3, {0: eng.n0e, 1: 2 * eng.n1e, 2: eng.n2e}[form], eng.sizes[form], eng.nEl
    B = r.standard_normal((nlev if per_level else 1, nEl * nd * nd))
    sc_ = r.uniform(0.5, 2.0, (nlev, nEl))
    x, y0 = r.standard_normal((nlev, nv)), r.standard_normal((nlev, nv))
    ops = [Operand("blocks", B, flat=not per_level)] + ([] if per_level else [Operand("elem_scale", sc_)]) + [Operand("x", x), Operand("y", y0, "out")]
    flags, alpha = (4 if transpose else 0), 0.5

    def call(eng, a):
        return eng.L.mimsem_elem_blocks_apply(eng.ctx, form, nlev, flags, a("blocks"), a["blocks"][1] if per_level else 0, *a["elem_scale"],
                                              *a["x"], *a["y"], alpha)

    def ref(ins, outs):
        idx = _elem_idx(dm, form)
        want = np.zeros((nlev, nv))
        for lev in range(nlev):
            Bl = B[lev if per_level else 0].reshape(nEl, nd, nd)
            for e in range(nEl):
                Be = (Bl[e].T if transpose else Bl[e]) * (1.0 if per_level else sc_[lev, e])
                want[lev, idx[e]] += Be @ x[lev, idx[e]]
        assert rel_l2(outs["y"], alpha * want) < 1e-12
    return eng, Case("mimsem_elem_blocks_apply", ops, call, ref)


_reg("mimsem_elem_blocks_apply", "blocks_apply_per_level", blocks_apply_case, 1, True, False)
_reg("mimsem_elem_blocks_apply", "blocks_apply_one_set_scaled", blocks_apply_case, 1, False, True)
_reg("mimsem_elem_blocks_apply", "blocks_apply_faces_scaled", blocks_apply_case, 2, False, False)


def pvec_case(W):
    """Phvec::assemble against the oracle at TOL (tests/test_gpu_horizontal.py test_pvec_phvec)"""
    eng, P = W.eng("B"), W.mesh("B")["P"]
    r = np.random.default_rng(_seed("pvec"))
    h = r.uniform(1, 2, (2, P.n2)) * 1e6
    ops = [Operand("h2", h), Operand("y", r.standard_normal((2, P.n0)), "out")]

    def ref(ins, outs):
        for k in range(2):
            assert rel_l2(outs["y"][k], P.phvec(1 + k, SCALE, h[k])) < TOL
    return eng, Case("mimsem_pvec", ops, lambda eng, a: eng.L.mimsem_pvec(eng.ctx, 1, 2, SCALE, *a["h2"], *a["y"]), ref)


_reg("mimsem_pvec", "pvec", pvec_case)


def incidence_case(W, which):
    """E10, E21 bit for bit against the oracle; E12 = -E21^T, E01 = -E10^T within the 1e-12 of tests/test_gpu_horizontal.py test_incidence"""
    eng, P = W.eng("B"), W.mesh("B")["P"]
    r = np.random.default_rng(_seed("inc", which))
    nin, nout = (P.n0, P.n1, P.n2, P.n1)[which], (P.n1, P.n2, P.n1, P.n0)[which]
    x = r.standard_normal((3, nin))
    ops = [Operand("x", x), Operand("y", r.standard_normal((3, nout)), "out")]

    def ref(ins, outs):
        if which < 2:
            for k in range(3):
                assert np.array_equal(outs["y"][k], (P.e10, P.e21)[which](x[k]))
            return
        fwd, n = (P.e21, P.n1) if which == 2 else (P.e10, P.n0)
        E = np.stack([fwd(col) for col in np.eye(n)], axis=1)                     # dense E21 / E10
        want = -(x @ E)
        assert bool((np.abs(outs["y"] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all())
    return eng, Case("mimsem_incidence_apply", ops, lambda eng, a: eng.L.mimsem_incidence_apply(eng.ctx, which, 3, *a["x"], *a["y"]), ref)


for _w in range(4):
    _reg("mimsem_incidence_apply", "incidence_%s" % ("E10", "E21", "E12", "E01")[_w], incidence_case, _w)


def interp_case(W, kind, form, push):
    """tests/test_gpu_horizontal.py test_interp_quad_matches_oracle_points: the oracle point by point, 1e-13"""
    eng, P = W.eng("B"), W.mesh("B")["P"]
    r = np.random.default_rng(_seed("interp", kind))
    nc, mp1, nex = (2 if form == 1 else 1), eng.mesh.m + 1, P.nElsX
    x = r.standard_normal((2, eng.sizes[form]))
    nout = eng.nEl * eng.mp12 * nc
    ops = [Operand("x", x), Operand("out", r.standard_normal((2, nout)), "out")]

    def ref(ins, outs):
        want = np.zeros((2, nex * nex, mp1 * mp1, nc))
        for lev in range(2):
            for ey in range(nex):
                for ex in range(nex):
                    for q in range(mp1 * mp1):
                        want[lev, ey * nex + ex, q] = P.interp(kind, ex, ey, q % mp1, q // mp1, x[lev])[:nc]
        assert rel_l2(outs["out"].reshape(want.shape), want) < 1e-13
    return eng, Case("mimsem_interp_quad", ops, lambda eng, a: eng.L.mimsem_interp_quad(eng.ctx, form, 1 if push else 0, 2, *a["x"], *a["out"]), ref)


_reg("mimsem_interp_quad", "interp_1g", interp_case, "1g", 1, True)
_reg("mimsem_interp_quad", "interp_2l", interp_case, "2l", 2, False)


def _owned_slots(dm):
    """[nEl, 2 n^2]: the slots each element owns in ascending order (the rule of include/mimsem_hip.h, as Engine.owned_covers_all reads it)"""
    n = dm.n
    l = np.arange(n * (n + 1))
    own = np.concatenate([np.asarray(dm.inds1x)[:, l % (n + 1) < n], np.asarray(dm.inds1y)[:, l // n < n]], axis=1)
    return np.sort(own, axis=1)


def owned_build_case(W):
    """f_stride of mimsem_owned_blocks_build (UHMAT, two levels).  Reference: the one-level builds of the same engine, bit for bit (two
    builds give the same bits, tests/test_gpu_pc_bjacobi_owned.py; the one-level build is what that file holds against the oracle's
    assembled chunks)"""
    import torch
    eng = W.eng("A")
    r = np.random.default_rng(_seed("owned_build"))
    nd = eng.owned_rows(1)
    h = r.uniform(0.5, 1.5, (2, eng.sizes[2])) * 1e6
    ops = [Operand("f", h), Operand("out", r.standard_normal((1, 2 * eng.nEl * nd * nd)), "out", flat=True)]

    def ref(ins, outs):
        got = outs["out"].reshape(2, eng.nEl, nd, nd)
        for k in range(2):
            one = eng.owned_blocks("UHMAT", f=eng.tensor(h[k:k + 1]), lev0=1 + k, nlev=1, scale=SCALE, flags=1)[0]
            assert torch.equal(one.cpu(), torch.from_numpy(got[k]))
    return eng, Case("mimsem_owned_blocks_build", ops,
                     lambda eng, a: eng.L.mimsem_owned_blocks_build(eng.ctx, OPS["UHMAT"], 1, 2, SCALE, 1, *a["f"], a("out")), ref)


_reg("mimsem_owned_blocks_build", "owned_blocks_build", owned_build_case)


def _owned_inverse(W):
    return W.cached("owned_inv", lambda: W.eng("A").owned_blocks("UMAT", lev0=0, nlev=3, scale=SCALE, flags=1, invert=True).cpu().numpy())


def owned_apply_case(W):
    """a set of blocks per level (blocks_level_stride, x_stride, y_stride all distinct); block-wise numpy products, the 1e-12 per level of
    tests/test_gpu_pc_bjacobi_owned.py test_owned_blocks_apply"""
    eng = W.eng("A")
    r = np.random.default_rng(_seed("owned_apply"))
    Binv = _owned_inverse(W)
    nd, n1 = Binv.shape[-1], eng.sizes[1]
    x = r.standard_normal((3, n1))
    ops = [Operand("blocks", Binv.reshape(3, -1)), Operand("x", x), Operand("y", r.standard_normal((3, n1)), "out")]

    def ref(ins, outs):
        own = _owned_slots(eng.mesh)
        for lev in range(3):
            want = np.zeros(n1)
            want[own] = np.einsum("kij,kj->ki", Binv[lev], x[lev][own])
            assert np.linalg.norm(outs["y"][lev] - want) / np.linalg.norm(want) < 1e-12
    return eng, Case("mimsem_owned_blocks_apply", ops,
                     lambda eng, a: eng.L.mimsem_owned_blocks_apply(eng.ctx, 1, 3, *a["blocks"], *a["x"], *a["y"]), ref)


_reg("mimsem_owned_blocks_apply", "owned_blocks_apply", owned_apply_case)


def pc_levels_case(W):
    """tests/test_gpu_vort_diag.py test_build_levels_rows_are_the_single_level_blocks: row r is the one-level build, bit for bit"""
    import torch
    eng = W.eng("B")
    r = np.random.default_rng(_seed("pc_levels"))
    nd = 2 * eng.n1e
    h = r.uniform(0.5, 1.5, (2, eng.sizes[2])) * 1e6
    ops = [Operand("f", h), Operand("out", r.standard_normal((1, 2 * eng.nEl * nd * nd)), "out", flat=True)]

    def ref(ins, outs):
        got = outs["out"].reshape(2, eng.nEl, nd, nd)
        for k in range(2):
            assert torch.equal(eng.elem_block_pc("UHMAT", f=eng.tensor(h[k]), lev=k, scale=SCALE).cpu(), torch.from_numpy(got[k]))
    return eng, Case("mimsem_elem_block_pc_build_levels", ops,
                     lambda eng, a: eng.L.mimsem_elem_block_pc_build_levels(eng.ctx, OPS["UHMAT"], 0, 1, 2, SCALE, 0, *a["f"], a("out")), ref)


_reg("mimsem_elem_block_pc_build_levels", "elem_block_pc_build_levels", pc_levels_case)

SW = dict(a=180.0, grav=9.80616, H=1.0e4)


def _sw_data(W, r, nlev=3):
    eng = W.eng("S")
    n1, n2 = eng.sizes[1], eng.sizes[2]
    x = np.concatenate([r.standard_normal((nlev, n1)), 50.0 * r.standard_normal((nlev, n2))], axis=1)
    return eng, n1, n2, x, r.standard_normal((nlev, eng.sizes[0])) * 1e-4


def _sw_blocks(W):
    def make():
        eng = W.eng("S")
        nd = 2 * eng.n1e + eng.n2e
        return np.random.default_rng(_seed("swblocks")).standard_normal((1, eng.nEl * nd * nd)) / nd
    return W.cached("swblocks", make)


def _sw_composed(eng, x, f0, n1):
    """the operator from the individual engine operators on contiguous tensors (SWEqn.apply_A_composed, the reference of
    tests/test_gpu_sweqn.py test_sw_fused_operator_matches_composition_and_oracle)"""
    import torch
    a, rows = SW["a"], []
    for k in range(x.shape[0]):                                            # (one geometry level: row by row)
        xt, ft = eng.tensor(x[k:k + 1]), eng.tensor(f0[k:k + 1])
        u, h = xt[:, :n1].contiguous(), xt[:, n1:].contiguous()
        yu = eng.apply("UMAT", u)
        eng.apply("ROTMAT", u, f=ft, alpha=a, flags=2, out=yu)
        yu += (a * SW["grav"]) * eng.incidence("E12", eng.apply("WMAT", h))
        w = eng.incidence("E21", u) * (a * SW["H"]) + h
        rows.append(torch.cat([yu, eng.apply("WMAT", w.contiguous())], dim=1))
    return torch.cat(rows, dim=0)


def _sw_precond(eng, r, blocks):
    """tests/test_gpu_sweqn.py test_sw_coupled_block_preconditioner: gather, batched mat-vec on the column-major blocks, scatter-add"""
    import torch
    dm = eng.mesh
    nd = 2 * eng.n1e + eng.n2e
    Cb = eng.tensor(blocks).view(eng.nEl, nd, nd)
    idx = torch.cat([torch.as_tensor(dm.inds1x), torch.as_tensor(dm.inds1y), torch.as_tensor(dm.inds2) + dm.n1], dim=1).long().to(eng.device)
    out = torch.zeros_like(r)
    for k in range(r.shape[0]):
        out[k].index_add_(0, idx.reshape(-1), torch.einsum("ecr,ec->er", Cb, r[k][idx]).reshape(-1))
    return out


def sw_case(W, which, broadcast=False):
    """the packed [u | h] entries on the shallow-water sphere of tests/test_gpu_sweqn.py.  which: apply | blocks | precond | cheb, against
    the compositions and the 1e-14 of tests/test_gpu_sweqn.py"""
    r = np.random.default_rng(_seed("sw", which, broadcast))
    eng, n1, n2, x, f0 = _sw_data(W, r)
    blocks = _sw_blocks(W)
    n = n1 + n2
    if broadcast:
        f0 = f0[:1]
    F0 = Operand("f0", f0, broadcast=broadcast)
    L = lambda eng: eng.L
    full_f0 = np.repeat(f0, 3, axis=0) if broadcast else f0
    tol = 1e-14
    if which == "apply":
        ops = [F0, Operand("x", x), Operand("y", r.standard_normal((3, n)), "out")]
        call = lambda eng, a: eng.L.mimsem_sw_operator_apply(eng.ctx, 3, SW["a"], SW["grav"], SW["H"], *a["f0"], *a["x"], *a["y"])
        ref = lambda ins, outs: _assert_rel(outs["y"], _sw_composed(eng, x, full_f0, n1), tol)
        entry = "mimsem_sw_operator_apply"
    elif which == "blocks":
        ops = [Operand("blocks", blocks, flat=True), Operand("x", x), Operand("y", r.standard_normal((3, n)), "out")]
        call = lambda eng, a: eng.L.mimsem_sw_blocks_apply(eng.ctx, 3, a("blocks"), *a["x"], *a["y"])
        ref = lambda ins, outs: _assert_rel(outs["y"], _sw_precond(eng, eng.tensor(x), blocks), tol)
        entry = "mimsem_sw_blocks_apply"
    elif which == "precond":
        ops = [F0, Operand("blocks", blocks, flat=True), Operand("x", x), Operand("z", r.standard_normal((3, n)), "out")]
        call = lambda eng, a: eng.L.mimsem_sw_operator_precond_apply(eng.ctx, 3, SW["a"], SW["grav"], SW["H"], *a["f0"], a("blocks"), *a["x"], *a["z"])
        ref = lambda ins, outs: _assert_rel(outs["z"], _sw_precond(eng, _sw_composed(eng, x, full_f0, n1), blocks), tol)
        entry = "mimsem_sw_operator_precond_apply"
    else:
        ca, cb = 0.37, 1.9
        res, d = np.concatenate([r.standard_normal((3, n1)), 50.0 * r.standard_normal((3, n2))], axis=1), \
            np.concatenate([r.standard_normal((3, n1)), 50.0 * r.standard_normal((3, n2))], axis=1)
        ops = [F0, Operand("blocks", blocks, flat=True), Operand("x", x, "inout"), Operand("r", res, "inout"), Operand("d", d, "inout")]
        call = lambda eng, a: eng.L.mimsem_sw_operator_precond_chebyshev(eng.ctx, 3, SW["a"], SW["grav"], SW["H"], *a["f0"], a("blocks"), ca, cb,
                                                                         *a["x"], *a["r"], *a["d"])

        def ref(ins, outs):
            Bd = _sw_precond(eng, _sw_composed(eng, d, full_f0, n1), blocks).cpu().numpy()
            r_ref = res - Bd
            for got, want in ((outs["x"], x + d), (outs["r"], r_ref), (outs["d"], ca * d + cb * r_ref)):
                assert rel_l2(got, want) < tol
        entry = "mimsem_sw_operator_precond_chebyshev"
    return eng, Case(entry, ops, call, ref)


def _assert_rel(got, want, tol):
    want = want.cpu().numpy() if hasattr(want, "cpu") else want
    assert rel_l2(got, want) < tol, rel_l2(got, want)


_reg("mimsem_sw_operator_apply", "sw_operator_apply", sw_case, "apply")
_reg("mimsem_sw_operator_apply", "sw_operator_apply_f0_broadcast", sw_case, "apply", True)
_reg("mimsem_sw_blocks_apply", "sw_blocks_apply", sw_case, "blocks")
_reg("mimsem_sw_operator_precond_apply", "sw_operator_precond_apply", sw_case, "precond")
_reg("mimsem_sw_operator_precond_chebyshev", "sw_operator_precond_chebyshev", sw_case, "cheb")


def sw_orth_case(W):
    """ldv > n.  tests/test_gpu_sweqn.py test_sw_body_with_the_gather_folded_into_the_first_gram_schmidt_pass: the same bits as
    mimsem_sw_operator_precond_apply followed by mimsem_krylov_orthogonalize"""
    import torch
    r = np.random.default_rng(_seed("sworth"))
    eng, n1, n2, x, f0 = _sw_data(W, r, 1)
    blocks = _sw_blocks(W)
    n, k = n1 + n2, 3
    Q, _ = np.linalg.qr(r.standard_normal((n, k)))
    V = np.ascontiguousarray(Q.T)
    ops = [Operand("f0", f0, flat=True), Operand("blocks", blocks, flat=True), Operand("x", x, flat=True), Operand("w", r.standard_normal((1, n)), "out", flat=True),
           Operand("V", V), Operand("h", r.standard_normal((1, k)), "out", flat=True)]

    def call(eng, a):
        return eng.L.mimsem_sw_operator_precond_orthogonalize(eng.ctx, SW["a"], SW["grav"], SW["H"], a("f0"), a("blocks"), a("x"), a("w"), k, *a["V"], -1.0, a("h"))

    def ref(ins, outs):
        nd = 2 * eng.n1e + eng.n2e
        w = eng.sw_operator_precond(SW["a"], SW["grav"], SW["H"], eng.tensor(f0[0]), eng.tensor(blocks).view(eng.nEl, nd, nd), eng.tensor(x)).reshape(-1).contiguous()
        h = eng.zeros(k)
        eng.orthogonalize(eng.tensor(V), w, h, k=k)
        assert torch.equal(w.cpu(), torch.from_numpy(outs["w"][0])) and torch.equal(h.cpu(), torch.from_numpy(outs["h"][0]))
    return eng, Case("mimsem_sw_operator_precond_orthogonalize", ops, call, ref)


_reg("mimsem_sw_operator_precond_orthogonalize", "sw_operator_precond_orthogonalize", sw_orth_case)


def _ap(eng, op, x, f=None, flags=0, alpha=1.0, out=None):
    return eng.apply(op, x, f=f, lev0=0, scale=SCALE, flags=flags, alpha=alpha, out=out)


def bernoulli_case(W):
    """velx1 / velx2 share ldu and velz1 / velz2 share ldz (one argument each), in buffers of their own; the composed route of
    HorizSolve.diagnose_Phi at the 1e-10 per level of tests/test_gpu_bernoulli.py"""
    eng = W.eng("A")
    r = np.random.default_rng(_seed("bernoulli"))
    nk, n1, n2 = 4, eng.sizes[1], eng.sizes[2]
    u1 = r.standard_normal((nk, n1)) * 1e3; u2 = u1 * (1 + 0.05 * r.standard_normal(u1.shape))
    z1 = r.standard_normal((nk - 1, n2)) * 1e3; z2 = z1 * (1 + 0.05 * r.standard_normal(z1.shape))
    ops = [Operand("velx1", u1, share="u"), Operand("velx2", u2, share="u"), Operand("velz1", z1, share="z"), Operand("velz2", z2, share="z"),
           Operand("out", r.standard_normal((nk, n2)), "out")]

    def call(eng, a):
        return eng.L.mimsem_horiz_bernoulli(eng.ctx, nk, a("velx1"), *a["velx2"], a("velz1"), *a["velz2"], SCALE, *a["out"])

    def ref(ins, outs):
        t = eng.tensor
        Phi = _ap(eng, "WTQUMAT", t(u1), f=t(u1), alpha=1.0 / 3.0)
        _ap(eng, "WTQUMAT", t(u2), f=t(u1), flags=2, alpha=1.0 / 3.0, out=Phi)
        _ap(eng, "WTQUMAT", t(u2), f=t(u2), flags=2, alpha=1.0 / 3.0, out=Phi)
        a1, a2 = eng.interface_average(t(z1), nk), eng.interface_average(t(z2), nk)
        _ap(eng, "WHMAT", a1, f=a1, flags=2, alpha=1.0 / 6.0, out=Phi)
        _ap(eng, "WHMAT", a2, f=a1, flags=2, alpha=1.0 / 6.0, out=Phi)
        _ap(eng, "WHMAT", a2, f=a2, flags=2, alpha=1.0 / 6.0, out=Phi)
        want = Phi.cpu().numpy()
        assert max(rel_l2(outs["out"][k], want[k]) for k in range(nk)) < TOL
    return eng, Case("mimsem_horiz_bernoulli", ops, call, ref)


def flux_rhs_case(W):
    """HorizSolve._uvec_hu4 (four accumulated Uhmat applies), 1e-10 per level (tests/test_gpu_flux_rhs.py)"""
    eng = W.eng("A")
    r = np.random.default_rng(_seed("flux"))
    nk, n1, n2 = 3, eng.sizes[1], eng.sizes[2]
    u1 = r.standard_normal((nk, n1)) * 1e3; u2 = u1 * (1 + 0.05 * r.standard_normal(u1.shape))
    h1 = r.uniform(0.5, 1.5, (nk, n2)) * 1e6; h2 = h1 * (1 + 0.01 * r.standard_normal(h1.shape))
    ops = [Operand("u1", u1, share="u"), Operand("u2", u2, share="u"), Operand("h1", h1, share="h"), Operand("h2", h2, share="h"),
           Operand("out", r.standard_normal((nk, n1)), "out")]

    def call(eng, a):
        return eng.L.mimsem_horiz_flux_rhs(eng.ctx, nk, a("u1"), *a["u2"], a("h1"), *a["h2"], SCALE, *a["out"])

    def ref(ins, outs):
        t = eng.tensor
        hu = _ap(eng, "UHMAT", t(u1), f=t(h1), flags=1, alpha=1.0 / 3.0)
        _ap(eng, "UHMAT", t(u1), f=t(h2), flags=3, alpha=1.0 / 6.0, out=hu)
        _ap(eng, "UHMAT", t(u2), f=t(h1), flags=3, alpha=1.0 / 6.0, out=hu)
        _ap(eng, "UHMAT", t(u2), f=t(h2), flags=3, alpha=1.0 / 3.0, out=hu)
        want = hu.cpu().numpy()
        assert max(rel_l2(outs["out"][k], want[k]) for k in range(nk)) < TOL
    return eng, Case("mimsem_horiz_flux_rhs", ops, call, ref)


def energetics_case(W):
    """five distinct strides; route_two of tests/test_gpu_energetics.py (applies, rowdot, interp_quad) with its bar: |difference| <= 1e-10 of
    the sum of the absolute values of the terms"""
    eng = W.eng("A")
    r = np.random.default_rng(_seed("energetics"))
    nlev, n1, n2 = 3, eng.sizes[1], eng.sizes[2]
    velx = r.standard_normal((nlev, n1)) * 1e3
    rho, rt, ex, th = (r.uniform(0.5, 1.5, (nlev, n2)) * s for s in (1e6, 3e8, 1e9, 3e2))
    ops = [Operand("velx", velx), Operand("rho", rho), Operand("rt", rt), Operand("exner", ex), Operand("theta", th),
           Operand("out", r.standard_normal((1, 4)), "out", flat=True)]

    def call(eng, a):
        return eng.L.mimsem_euler_energetics_horiz(eng.ctx, nlev, *a["velx"], *a["rho"], *a["rt"], *a["exner"], *a["theta"], a("out"))

    def ref(ins, outs):
        from mimsem_amd.geom import gll_weights
        from tests import energetics_case as ec
        t = eng.tensor
        ap = lambda op, x, f=None: eng.apply(op, x, f=f, lev0=0, scale=SCALE, flags=1)
        w = gll_weights(eng.mesh.n)
        wd = eng.tensor(eng.mesh.det * np.outer(w, w).ravel()[None, :])
        terms = [(0.5 / SCALE) * ap("UHMAT", t(velx), t(rho)) * t(velx), (ec.CV / ec.CP / SCALE) * t(rt) * ap("WMAT", t(ex)),
                 (0.5 / SCALE) * ap("WMAT", t(rt)) * t(th), eng.interp_quad(2, t(rho)) * wd[None]]
        for i, term in enumerate(terms):
            assert abs(outs["out"][0][i] - float(term.sum())) <= 1e-10 * float(term.abs().sum()), i
    return eng, Case("mimsem_euler_energetics_horiz", ops, call, ref)


_reg("mimsem_horiz_bernoulli", "horiz_bernoulli", bernoulli_case)
_reg("mimsem_horiz_flux_rhs", "horiz_flux_rhs", flux_rhs_case)
_reg("mimsem_euler_energetics_horiz", "euler_energetics_horiz", energetics_case)


# ---- sweeps and fixed-length solves on mesh A: 3 levels, 3 steps ------------------------------------------------------------------
# Reference: the same update composed in torch float64 from eng.apply and the preconditioner on contiguous tensors, relative 1e-13
# (tests/test_gpu_next_rows.py test_chebyshev_mass_solver).
SWEEP_TOL = 1e-13
COEF = [(1.0, 0.0), (0.9, 0.2), (0.8, 0.3)]


def _mass(W):
    from mimsem_amd.krylov import MassSolver
    return W.cached("mass", lambda: MassSolver(W.eng("A"), SCALE, True))


def _cm(W):
    return W.cached("cm", lambda: _mass(W).blocks.transpose(1, 2).contiguous().cpu().numpy().reshape(1, -1))


def _vnorm(got, want, what):
    import torch
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < SWEEP_TOL, (what, np.linalg.norm(got - want) / np.linalg.norm(want))


def _up_fields(W, r, nlev, lev0, tau):
    P0 = W.mesh("A")["patches"][0][1]
    eng = W.eng("A")
    vs = np.array([P0.det.mean() / P0.thickInv[lev0 + k].mean() * 0.3 / tau for k in range(nlev)])[:, None]
    return r.uniform(0.5, 1.5, (nlev, eng.sizes[2])), r.uniform(-1, 1, (nlev, eng.sizes[1])) * vs


def op_sweep_case(W, cheb):
    """mimsem_op_richardson_sweep / mimsem_op_chebyshev_sweep on UHMAT_UP (field, velocity, b, dinv, [p,] x, upd: six / seven strides)"""
    eng = W.eng("A")
    r = np.random.default_rng(_seed("opsweep", cheb))
    nlev, lev0, tau, n1 = 3, 1, 75.0, eng.sizes[1]
    h, u = _up_fields(W, r, nlev, lev0, tau)
    x0, b, p0 = r.standard_normal((nlev, n1)), r.standard_normal((nlev, n1)), r.standard_normal((nlev, n1))
    t = eng.tensor
    A = lambda v: eng.apply_up("UHMAT_UP", v, t(h), t(u), lev0=lev0, scale=SCALE, tau=tau)
    y = A(t(x0))
    dinv = r.uniform(0.5, 1.0, (nlev, n1)) * 0.1 * float(t(x0).abs().max() / y.abs().max())       # |dinv A| ~ 0.1: three steps stay well scaled
    b = b * float(y.abs().max())
    ops = [Operand("f", h), Operand("u", u), Operand("b", b), Operand("dinv", dinv)] + ([Operand("p", p0, "inout")] if cheb else []) + \
          [Operand("x", x0, "inout"), Operand("upd", r.standard_normal((nlev, n1)), "out")]

    def call(eng, a):
        rc = 0
        for al, be in COEF:
            if cheb:
                rc = rc or eng.L.mimsem_op_chebyshev_sweep(eng.ctx, OPS["UHMAT_UP"], lev0, nlev, SCALE, tau, 0, *a["f"], *a["u"], *a["b"], *a["dinv"], al, be,
                                                           *a["p"], *a["x"], *a["upd"])
            else:
                rc = rc or eng.L.mimsem_op_richardson_sweep(eng.ctx, OPS["UHMAT_UP"], lev0, nlev, SCALE, tau, 0, *a["f"], *a["u"], *a["b"], *a["dinv"],
                                                            *a["x"], *a["upd"])
        return rc

    def ref(ins, outs):
        x, p = t(x0), t(p0)
        for al, be in COEF:
            z = t(dinv) * (t(b) - A(x))
            if cheb:
                p = z + be * p; x = x + al * p
            else:
                x = x + z
        _vnorm(outs["x"], x, "x"); _vnorm(outs["upd"], z, "upd")
        if cheb:
            _vnorm(outs["p"], p, "p")
    return eng, Case("mimsem_op_chebyshev_sweep" if cheb else "mimsem_op_richardson_sweep", ops, call, ref)


_reg("mimsem_op_richardson_sweep", "op_richardson_sweep", op_sweep_case, False)
_reg("mimsem_op_chebyshev_sweep", "op_chebyshev_sweep", op_sweep_case, True)


def block_sweep_case(W, cheb):
    """mimsem_block_richardson_sweep (UHMAT without the thickness flag, the blocks alone) / mimsem_block_chebyshev_sweep (UHMAT with it,
    elem_scale rows at a stride of their own)"""
    eng, ms = W.eng("A"), _mass(W)
    r = np.random.default_rng(_seed("blocksweep", cheb))
    nlev, lev0, n1 = 3, 1, eng.sizes[1]
    fl = 1 if cheb else 0
    h = r.uniform(0.5, 1.5, (nlev, eng.sizes[2]))
    esc = ms.escale[lev0:lev0 + nlev].cpu().numpy()
    x0, b, p0 = r.standard_normal((nlev, n1)), r.standard_normal((nlev, n1)) * 1e9, r.standard_normal((nlev, n1))
    t = eng.tensor
    A = lambda v: eng.apply("UHMAT", v, f=t(h), lev0=lev0, scale=SCALE, flags=fl)
    Pc = lambda v: eng.blocks_apply(1, ms.blocks, v, transpose=True, elem_scale=t(esc) if cheb else None)
    if not cheb:                                                           # (blocks of the thickness-free Umat: bring b to the size of A x)
        b = b * float(A(t(x0)).abs().max()) / 1e9
    ops = [Operand("f", h), Operand("blocks", _cm(W), flat=True)] + ([Operand("elem_scale", esc)] if cheb else []) + [Operand("b", b)] + \
          ([Operand("p", p0, "inout")] if cheb else []) + [Operand("x", x0, "inout"), Operand("upd", r.standard_normal((nlev, n1)), "out")]

    def call(eng, a):
        rc = 0
        for al, be in COEF:
            if cheb:
                rc = rc or eng.L.mimsem_block_chebyshev_sweep(eng.ctx, OPS["UHMAT"], lev0, nlev, SCALE, fl, *a["f"], a("blocks"), *a["elem_scale"], *a["b"],
                                                              al, be, *a["p"], *a["x"], *a["upd"])
            else:
                rc = rc or eng.L.mimsem_block_richardson_sweep(eng.ctx, OPS["UHMAT"], lev0, nlev, SCALE, fl, *a["f"], a("blocks"), *a["b"], *a["x"], *a["upd"])
        return rc

    def ref(ins, outs):
        x, p = t(x0), t(p0)
        for al, be in COEF:
            z = Pc(t(b) - A(x))
            if cheb:
                p = z + be * p; x = x + al * p
            else:
                x = x + z
        _vnorm(outs["x"], x, "x"); _vnorm(outs["upd"], z, "upd")
        if cheb:
            _vnorm(outs["p"], p, "p")
    return eng, Case("mimsem_block_chebyshev_sweep" if cheb else "mimsem_block_richardson_sweep", ops, call, ref)


_reg("mimsem_block_richardson_sweep", "block_richardson_sweep", block_sweep_case, False)
_reg("mimsem_block_chebyshev_sweep", "block_chebyshev_sweep", block_sweep_case, True)


def solve_case(W, kind):
    """mimsem_block_chebyshev_solve (with pb, upd), mimsem_fric_chebyshev_solve (exner_stride), mimsem_owned_block_chebyshev_solve: three steps
    from x = 0 against the composed recurrence"""
    eng, ms = W.eng("A"), _mass(W)
    r = np.random.default_rng(_seed("solve", kind))
    nlev, lev0, n1, tau = 3, (0 if kind == "owned" else 2), eng.sizes[1], 120.0
    b = r.standard_normal((nlev, n1)) * 1e3
    t = eng.tensor
    esc = ms.escale[lev0:lev0 + nlev].cpu().numpy()
    outs3 = [Operand(nm, r.standard_normal((nlev, n1)), "out") for nm in ("x", "pb", "upd")]
    coef = (C.c_double * 6)(*[v for ab in COEF for v in ab])
    if kind == "owned":
        Binv = _owned_inverse(W)
        ops = [Operand("blocks", Binv.reshape(3, -1)), Operand("b", b)] + outs3
        call = lambda eng, a: eng.L.mimsem_owned_block_chebyshev_solve(eng.ctx, 0, lev0, nlev, SCALE, 1, *a["blocks"], *a["b"], 3, coef, *a["x"], *a["pb"], *a["upd"])
        A = lambda v: eng.apply("UMAT", v, lev0=lev0, scale=SCALE, flags=1)
        Pc = lambda v: eng.owned_blocks_apply(1, t(Binv), v)
        entry = "mimsem_owned_block_chebyshev_solve"
    else:
        Pc = lambda v: eng.blocks_apply(1, ms.blocks, v, transpose=True, elem_scale=t(esc))
        pre = [Operand("blocks", _cm(W), flat=True), Operand("elem_scale", esc), Operand("b", b)] + outs3
        if kind == "block":
            ops = pre
            call = lambda eng, a: eng.L.mimsem_block_chebyshev_solve(eng.ctx, 0, lev0, nlev, SCALE, 1, None, 0, a("blocks"), *a["elem_scale"], *a["b"], 3, coef,
                                                                     *a["x"], *a["pb"], *a["upd"])
            A = lambda v: eng.apply("UMAT", v, lev0=lev0, scale=SCALE, flags=1)
            entry = "mimsem_block_chebyshev_solve"
        else:
            ek, es = _exner(W, r, [lev0 + k for k in range(nlev)])
            ops = pre + [Operand("exner", ek), Operand("exner_s", es, flat=True)]
            call = lambda eng, a: eng.L.mimsem_fric_chebyshev_solve(eng.ctx, 0, lev0, nlev, SCALE, 1, None, 0, a("blocks"), *a["elem_scale"], *a["b"], 3, coef,
                                                                    *a["x"], *a["pb"], *a["upd"], tau, *a["exner"], a("exner_s"))
            A = lambda v: eng.apply_fric(v, t(ek), t(es[0]), tau, lev0=lev0, scale=SCALE)
            entry = "mimsem_fric_chebyshev_solve"

    def ref(ins, outs):
        import torch
        x = torch.zeros_like(t(b)); p = torch.zeros_like(x)
        for k, (al, be) in enumerate(COEF):
            z = Pc(t(b) - A(x)) if k else Pc(t(b))
            if k == 0:
                _vnorm(outs["pb"], z, "pb")
            p = z + be * p; x = x + al * p
        _vnorm(outs["x"], x, "x"); _vnorm(outs["upd"], z, "upd")
    return eng, Case(entry, ops, call, ref)


_reg("mimsem_block_chebyshev_solve", "block_chebyshev_solve", solve_case, "block")
_reg("mimsem_fric_chebyshev_solve", "fric_chebyshev_solve", solve_case, "fric")
_reg("mimsem_owned_block_chebyshev_solve", "owned_block_chebyshev_solve", solve_case, "owned")


# ---- vector algebra ---------------------------------------------------------------------------------------------------------------
# Reference: numpy in longdouble, rounded to float64.  Reductions (inner products, and the sums over k basis vectors that follow them):
# within 1e-14 * sum |a||b|, as tests/test_gpu_next_rows.py test_rowdot_short_and_long_rows has it.  Element-wise results: within 2 ulp --
# the kernels use fma, so a result differs from the correctly rounded one by the roundings of its one or two intermediate values; the
# inputs are positive (and the coefficients signed so that every term adds), which keeps cancellation from magnifying those roundings.
LD = np.longdouble
NS = (7, 1000, 5003)


def _ulp2(got, want, what):
    want64 = np.asarray(want, dtype=np.float64)
    assert bool((np.abs(got.astype(LD) - want) <= 2 * np.spacing(np.abs(want64))).all()), (what, float(np.max(np.abs(got.astype(LD) - want) / np.spacing(np.abs(want64)))))


def _red(got, want, scale, what, tol=1e-14):
    assert bool((np.abs(got.astype(LD) - want) <= tol * scale + 1e-300).all()), (what, float(np.max(np.abs(got.astype(LD) - want) / (scale + 1e-300))))


def _pos(r, shape):
    return r.uniform(0.5, 2.0, shape)


def gs_case(W, which, n):
    """mimsem_krylov_mdot / maxpy / orthogonalize (any V) and reorthonormalize / _ex / cgs2 (V orthonormal, as
    test_krylov_cgs2_three_launches has it, with its tolerances: w 1e-13 and col 1e-12 of |w0|_max, v 1e-12), ldv = n + pad"""
    import torch
    eng = W.eng("B")
    r = np.random.default_rng(_seed("gs", which, n))
    k = 3
    ortho = which in ("reorth", "reorth_ex", "cgs2")
    V = np.ascontiguousarray(np.linalg.qr(r.standard_normal((n, k)))[0].T) if ortho else r.standard_normal((k, n))
    w0, h0 = r.standard_normal((1, n)), r.standard_normal((1, k))
    Vl, wl = V.astype(LD), w0[0].astype(LD)
    absdot = np.abs(Vl) @ np.abs(wl)
    OV, Ow = Operand("V", V), Operand("w", w0, "in" if which == "mdot" else "inout", flat=True)
    f = lambda name, m, role="out": Operand(name, r.standard_normal((1, m)), role, flat=True)
    ns = k + 1
    flagw = torch.zeros(1, dtype=torch.int32, device=eng.device)          # the caller's flag word of the _ex / cgs2 forms
    if which == "mdot":
        ops = [OV, Ow, f("h", k)]
        call = lambda eng, a: eng.L.mimsem_krylov_mdot(eng.ctx, k, n, *a["V"], a("w"), a("h"))
        ref = lambda ins, outs: _red(outs["h"][0], Vl @ wl, absdot, "h")
    elif which == "maxpy":
        ops = [OV, Operand("h", h0, flat=True), Ow]
        call = lambda eng, a: eng.L.mimsem_krylov_maxpy(eng.ctx, k, n, *a["V"], a("h"), 0.75, a("w"))
        ref = lambda ins, outs: _red(outs["w"][0], wl + LD(0.75) * (h0[0].astype(LD) @ Vl), np.abs(wl) + 0.75 * (np.abs(h0[0]) @ np.abs(V)), "w")
    elif which == "orth":
        ops = [OV, Ow, f("h", k)]
        call = lambda eng, a: eng.L.mimsem_krylov_orthogonalize(eng.ctx, k, n, *a["V"], -1.0, a("w"), a("h"))

        def ref(ins, outs):
            h = Vl @ wl
            _red(outs["h"][0], h, absdot, "h")
            _red(outs["w"][0], wl - h @ Vl, np.abs(wl) + np.abs(h) @ np.abs(Vl) + absdot @ np.abs(Vl) * 1.0, "w")
    else:
        cgs2 = which == "cgs2"
        ops = [OV, Ow, f("v", n), Operand("h1", h0, "out" if cgs2 else "in", flat=True), f("h2", k), f("col", k + 2)]
        if which == "reorth":
            call = lambda eng, a: eng.L.mimsem_krylov_reorthonormalize(eng.ctx, k, n, *a["V"], a("w"), a("v"), a("h1"), a("h2"), a("col"), ns)
        elif which == "reorth_ex":
            call = lambda eng, a: eng.L.mimsem_krylov_reorthonormalize_ex(eng.ctx, k, n, *a["V"], a("w"), a("v"), a("h1"), a("h2"), a("col"), ns, 1, flagw.data_ptr())
        else:
            call = lambda eng, a: eng.L.mimsem_krylov_cgs2(eng.ctx, k, n, *a["V"], a("w"), a("v"), a("h1"), a("h2"), a("col"), ns, flagw.data_ptr())

        def ref(ins, outs):
            scale = float(np.abs(w0).max())
            w, h1 = wl, h0[0].astype(LD)
            if cgs2:
                h1 = Vl @ w; w = w - h1 @ Vl
            h2 = Vl @ w; w = w - h2 @ Vl
            nrm = np.sqrt(w @ w)
            assert float(np.abs(outs["w"][0] - w).max()) < 1e-13 * scale and float(np.abs(outs["v"][0] - w / nrm).max()) < 1e-12
            assert float(np.abs(outs["col"][0][:k] - (h1 + h2)).max()) < 1e-12 * scale and abs(float(outs["col"][0][ns] - nrm)) < 1e-12 * float(nrm)
            assert outs["col"][0][k] == ins["col"][0][k]                                   # (the word between the column and the norm slot)
    entry = dict(mdot="mimsem_krylov_mdot", maxpy="mimsem_krylov_maxpy", orth="mimsem_krylov_orthogonalize", reorth="mimsem_krylov_reorthonormalize",
                 reorth_ex="mimsem_krylov_reorthonormalize_ex", cgs2="mimsem_krylov_cgs2")[which]
    return eng, Case(entry, ops, call, ref)


def rows_case(W, which, n):
    """the row-wise kernels, 3 rows, every operand at a stride of its own"""
    eng = W.eng("B")
    r = np.random.default_rng(_seed("rows", which, n))
    R = 3
    P = lambda: _pos(r, (R, n))
    I = lambda name, role="in", d=None: Operand(name, P() if d is None else d, role)
    ld = lambda x: np.asarray(x).astype(LD)
    flat = lambda name, d: Operand(name, d, flat=True)
    if which == "rowdot":
        A, B = r.standard_normal((R, n)), r.standard_normal((R, n))
        ops = [I("A", d=A), I("B", d=B), Operand("out", r.standard_normal((1, R)), "out", flat=True)]
        call = lambda eng, a: eng.L.mimsem_krylov_rowdot(eng.ctx, R, n, *a["A"], *a["B"], a("out"))
        ref = lambda ins, outs: _red(outs["out"][0], (ld(A) * ld(B)).sum(axis=1), (np.abs(A) * np.abs(B)).sum(axis=1), "out")
        entry = "mimsem_krylov_rowdot"
    elif which == "cg_update":
        num, den = _pos(r, (1, R)), _pos(r, (1, R))
        p, Ap, x, res = P(), -P(), P(), P()                                   # (Ap < 0: r - a Ap adds)
        ops = [flat("num", num), flat("den", den), I("p", d=p), I("Ap", d=Ap), I("x", "inout", x), I("r", "inout", res)]
        call = lambda eng, a: eng.L.mimsem_krylov_cg_update(eng.ctx, R, n, a("num"), a("den"), *a["p"], *a["Ap"], *a["x"], *a["r"])

        def ref(ins, outs):
            al = ld(num[0] / den[0])[:, None]                                 # (the quotient is one correctly rounded float64 division)
            _ulp2(outs["x"], ld(x) + al * ld(p), "x"); _ulp2(outs["r"], ld(res) - al * ld(Ap), "r")
        entry = "mimsem_krylov_cg_update"
    elif which == "cg_direction":
        num, den, z, p = _pos(r, (1, R)), _pos(r, (1, R)), P(), P()
        ops = [flat("num", num), flat("den", den), I("z", d=z), I("p", "inout", p)]
        call = lambda eng, a: eng.L.mimsem_krylov_cg_direction(eng.ctx, R, n, a("num"), a("den"), *a["z"], *a["p"])
        ref = lambda ins, outs: _ulp2(outs["p"], ld(z) + ld(num[0] / den[0])[:, None] * ld(p), "p")
        entry = "mimsem_krylov_cg_direction"
    elif which == "cheb_start":
        c, s, th = P(), 0.7, 1.3
        ops = [I("c", d=c), I("r", "out"), I("d", "out"), I("x", "out")]
        call = lambda eng, a: eng.L.mimsem_krylov_chebyshev_start(eng.ctx, R, n, s, th, *a["c"], *a["r"], *a["d"], *a["x"])

        def ref(ins, outs):
            _ulp2(outs["r"], LD(s) * ld(c), "r"); _ulp2(outs["d"], LD(s) * ld(c) / LD(th), "d")
            assert not outs["x"].any()
        entry = "mimsem_krylov_chebyshev_start"
    elif which in ("cheb_px", "cheb_px_plain"):
        y, b, dinv, p, x = P(), P() + 2.0, P(), P(), P()                      # (b > y)
        al, be = 1.9, 0.37
        with_d = which == "cheb_px"
        ops = [I("y", d=y)] + ([I("b", d=b), I("dinv", d=dinv)] if with_d else []) + [I("p", "inout", p), I("x", "inout", x), I("upd", "out")]
        call = lambda eng, a: eng.L.mimsem_krylov_chebyshev_px(eng.ctx, R, n, al, be, *a["y"], *a["b"], *a["dinv"], *a["p"], *a["x"], *a["upd"])

        def ref(ins, outs):
            z = ld(dinv) * (ld(b) - ld(y)) if with_d else ld(y)
            pn = z + LD(be) * ld(p)
            _ulp2(outs["upd"], z, "upd"); _ulp2(outs["p"], pn, "p"); _ulp2(outs["x"], ld(x) + LD(al) * pn, "x")
        entry = "mimsem_krylov_chebyshev_px"
    elif which == "cheb_update":
        Bd, x, res, d = -P(), P(), P(), P()                                   # (Bd < 0: r - Bd adds)
        ca, cb = 0.37, 1.9
        ops = [I("Bd", d=Bd), I("x", "inout", x), I("r", "inout", res), I("d", "inout", d)]
        call = lambda eng, a: eng.L.mimsem_krylov_chebyshev_update(eng.ctx, R, n, ca, cb, *a["Bd"], *a["x"], *a["r"], *a["d"])

        def ref(ins, outs):
            rn = ld(res) - ld(Bd)
            _ulp2(outs["x"], ld(x) + ld(d), "x"); _ulp2(outs["r"], rn, "r"); _ulp2(outs["d"], LD(ca) * ld(d) + LD(cb) * rn, "d")
        entry = "mimsem_krylov_chebyshev_update"
    elif which.startswith("combine"):
        opc = int(which[-1])
        a_, b_, c_ = P(), P(), P()
        al, be = 2.0, 0.75
        ops = [I("a", d=a_)] + ([I("b", d=b_)] if opc else []) + [I("c", "inout", c_)]           # out aliases c (the documented aliasing)
        call = lambda eng, a: eng.L.mimsem_vec_combine(eng.ctx, R, n, al, *a["a"], opc, *a["b"], be, *a["c"], *a["c"])

        def ref(ins, outs):
            t = ld(a_) if opc == 0 else (ld(a_) * ld(b_) if opc == 1 else ld(a_) / ld(b_))
            _ulp2(outs["c"], LD(al) * t + LD(be) * ld(c_), "out")
        entry = "mimsem_vec_combine"
    else:
        nk = 4
        a_ = _pos(r, (nk - 1, n))
        ops = [I("a", d=a_), Operand("out", _pos(r, (nk, n)), "out")]
        call = lambda eng, a: eng.L.mimsem_interface_average(eng.ctx, nk, n, *a["a"], *a["out"])

        def ref(ins, outs):
            want = np.zeros((nk, n), dtype=LD)
            want[1:] += LD(0.5) * ld(a_); want[:-1] += LD(0.5) * ld(a_)
            _ulp2(outs["out"], want, "out")
        entry = "mimsem_interface_average"
    return eng, Case(entry, ops, call, ref)


for _n in NS:
    for _w, _e in (("mdot", "mimsem_krylov_mdot"), ("maxpy", "mimsem_krylov_maxpy"), ("orth", "mimsem_krylov_orthogonalize"),
                   ("reorth", "mimsem_krylov_reorthonormalize"), ("reorth_ex", "mimsem_krylov_reorthonormalize_ex"), ("cgs2", "mimsem_krylov_cgs2")):
        _reg(_e, "krylov_%s_n%d" % (_w, _n), gs_case, _w, _n)
    for _w, _e in (("rowdot", "mimsem_krylov_rowdot"), ("cg_update", "mimsem_krylov_cg_update"), ("cg_direction", "mimsem_krylov_cg_direction"),
                   ("cheb_start", "mimsem_krylov_chebyshev_start"), ("cheb_px", "mimsem_krylov_chebyshev_px"), ("cheb_px_plain", "mimsem_krylov_chebyshev_px"),
                   ("cheb_update", "mimsem_krylov_chebyshev_update"), ("combine0", "mimsem_vec_combine"), ("combine1", "mimsem_vec_combine"),
                   ("combine2", "mimsem_vec_combine"), ("iface", "mimsem_interface_average")):
        _reg(_e, "rows_%s_n%d" % (_w, _n), rows_case, _w, _n)


# ---- column and halo entries with a stride -----------------------------------------------------------------------------------------
def l2_case(W, direction):
    """pure data movement, bit for bit against the oracle (tests/test_gpu_column.py test_l2_transpose_roundtrip_and_layout)"""
    eng, P = W.eng("D"), W.mesh("D")["P"]
    r = np.random.default_rng(_seed("l2", direction))
    vh = r.standard_normal((P.nk, P.n2))
    vz = P.horiz_to_vert(vh).reshape(1, -1)
    if direction == 0:
        ops = [Operand("vh", vh), Operand("vz", r.standard_normal(vz.shape), "out", flat=True)]
        ref = lambda ins, outs: _same(outs["vz"], vz)
    else:
        ops = [Operand("vh", r.standard_normal(vh.shape), "out"), Operand("vz", vz, flat=True)]
        ref = lambda ins, outs: _same(outs["vh"], vh)
    return eng, Case("mimsem_l2_transpose", ops, lambda eng, a: eng.L.mimsem_l2_transpose(eng.ctx, direction, P.nk, *a["vh"], a("vz")), ref)


def _same(got, want):
    assert np.array_equal(got, want)


def column_up_case(W, which):
    """uh_stride of mimsem_column_diag_theta_up, mimsem_colop_blocks_ex, mimsem_colop_apply_ex (LINEAR_RHO2_UP): the oracle columns and TOL of
    tests/test_gpu_column.py test_diag_theta_up_and_temp_forcing / test_hs_colops"""
    from mimsem_amd._lib import COLOPS
    from tests.test_gpu_column import _col_fields, _dense_from_blocks, _uh
    eng, P = W.eng("D"), W.mesh("D")["P"]
    F = _col_fields(P)
    r = np.random.default_rng(_seed("colup", which))
    dt = 60.0 if which == "theta" else 75.0
    uh = _uh(P, r, dt)
    flat = lambda name, d, role="in": Operand(name, np.asarray(d).reshape(1, -1), role, flat=True)
    colop = "LINEAR_RHO2_UP"
    cols = [(0, 0), (P.nElsX - 1, P.nElsX - 1)]
    if which == "theta":
        ops = [flat("rho", F["rho"]), flat("rt", F["rt"]), Operand("uh", uh), flat("theta", r.standard_normal((P.nEl, (P.nk + 1) * P.n2e)), "out")]
        call = lambda eng, a: eng.L.mimsem_column_diag_theta_up(eng.ctx, dt, a("rho"), a("rt"), *a["uh"], a("theta"))

        def ref(ins, outs):
            th = outs["theta"].reshape(P.nEl, -1)
            for ex, ey in cols:
                e = ey * P.nElsX + ex
                assert rel_l2(th[e], P.diag_theta_up(ex, ey, dt, F["rho"][e], F["rt"][e], uh)) < TOL
        entry = "mimsem_column_diag_theta_up"
    elif which == "blocks":
        nb = eng.L.mimsem_colop_nblocks(eng.ctx, COLOPS[colop])
        ops = [flat("f1", F["rho"]), Operand("uh", uh), flat("out", r.standard_normal((P.nEl, nb * P.n2e * P.n2e)), "out")]
        call = lambda eng, a: eng.L.mimsem_colop_blocks_ex(eng.ctx, COLOPS[colop], 0, dt, a("f1"), None, *a["uh"], a("out"))

        def ref(ins, outs):
            blk = outs["out"].reshape(P.nEl, nb, P.n2e, P.n2e)
            for ex, ey in cols:
                e = ey * P.nElsX + ex
                assert rel_l2(_dense_from_blocks(P, colop, blk[e]), P.colop_dense_ex(colop, ex, ey, param=dt, f1=F["rho"][e], uh=uh)) < TOL
        entry = "mimsem_colop_blocks_ex"
    else:
        rows, ncol = P.colop_dims(colop)
        x = r.standard_normal((P.nEl, ncol))
        ops = [flat("f1", F["rho"]), Operand("uh", uh), flat("x", x), flat("y", r.standard_normal((P.nEl, rows)), "out")]
        call = lambda eng, a: eng.L.mimsem_colop_apply_ex(eng.ctx, COLOPS[colop], 0, 0, dt, a("f1"), None, *a["uh"], a("x"), a("y"))

        def ref(ins, outs):
            y = outs["y"].reshape(P.nEl, rows)
            for ex, ey in cols:
                e = ey * P.nElsX + ex
                assert rel_l2(y[e], P.colop_dense_ex(colop, ex, ey, param=dt, f1=F["rho"][e], uh=uh) @ x[e]) < TOL
        entry = "mimsem_colop_apply_ex"
    return eng, Case(entry, ops, call, ref)


_reg("mimsem_l2_transpose", "l2_horiz_to_vert", l2_case, 0)
_reg("mimsem_l2_transpose", "l2_vert_to_horiz", l2_case, 1)
_reg("mimsem_column_diag_theta_up", "column_diag_theta_up", column_up_case, "theta")
_reg("mimsem_colop_blocks_ex", "colop_blocks_ex", column_up_case, "blocks")
_reg("mimsem_colop_apply_ex", "colop_apply_ex", column_up_case, "apply")


def halo_case(W, which):
    """v_stride of mimsem_halo_pack / _unpack (insert, add) / _segments (pack, add): plain indexing, bit for bit (copies and one addition per
    slot; what tests/test_gpu_halo_abi.py and tests/test_gpu_sharded.py exchange)"""
    import torch
    eng = W.eng("B")
    r = np.random.default_rng(_seed("halo", which))
    n1, nlev = eng.sizes[1], 3
    idx = r.permutation(n1)[:41].astype(np.int32)                         # distinct slots
    off = np.array([0, 5, 17, 41], dtype=np.int32)                        # three neighbours
    v, buf = r.standard_normal((nlev, n1)), r.standard_normal((1, nlev * idx.size))
    didx = W.cached(("haloidx", which), lambda: torch.as_tensor(idx, device=eng.device))
    flat = lambda name, d, role="in": Operand(name, d, role, flat=True)
    b3 = buf.reshape(nlev, idx.size)
    seg = np.concatenate([buf[0][off[s] * nlev:off[s + 1] * nlev].reshape(nlev, -1) for s in range(3)], axis=1)      # [lev, slot] of the segment-major buffer
    if which == "pack":
        ops = [Operand("v", v), flat("buf", buf, "out")]
        call = lambda eng, a: eng.L.mimsem_halo_pack(eng.ctx, didx.data_ptr(), idx.size, nlev, *a["v"], a("buf"))
        ref = lambda ins, outs: _same(outs["buf"].reshape(nlev, -1), v[:, idx])
        entry = "mimsem_halo_pack"
    elif which in ("unpack_insert", "unpack_add"):
        mode = int(which == "unpack_add")
        ops = [flat("buf", buf), Operand("v", v, "inout")]
        call = lambda eng, a: eng.L.mimsem_halo_unpack(eng.ctx, didx.data_ptr(), idx.size, nlev, mode, a("buf"), *a["v"])

        def ref(ins, outs):
            want = v.copy()
            want[:, idx] = want[:, idx] + b3 if mode else b3
            _same(outs["v"], want)
        entry = "mimsem_halo_unpack"
    else:
        mode = {"seg_pack": 0, "seg_insert": 1, "seg_add": 2}[which]
        ops = [flat("buf", buf, "out" if mode == 0 else "in"), Operand("v", v, "in" if mode == 0 else "inout")]
        call = lambda eng, a: eng.L.mimsem_halo_segments(eng.ctx, didx.data_ptr(), 3, off.ctypes.data, 0, 3, nlev, mode, a("buf"), *a["v"])

        def ref(ins, outs):
            if mode == 0:
                got = np.concatenate([outs["buf"][0][off[s] * nlev:off[s + 1] * nlev].reshape(nlev, -1) for s in range(3)], axis=1)
                return _same(got, v[:, idx])
            want = v.copy()
            want[:, idx] = want[:, idx] + seg if mode == 2 else seg
            _same(outs["v"], want)
        entry = "mimsem_halo_segments"
    return eng, Case(entry, ops, call, ref)


for _w, _e in (("pack", "mimsem_halo_pack"), ("unpack_insert", "mimsem_halo_unpack"), ("unpack_add", "mimsem_halo_unpack"),
               ("seg_pack", "mimsem_halo_segments"), ("seg_insert", "mimsem_halo_segments"), ("seg_add", "mimsem_halo_segments")):
    _reg(_e, "halo_%s" % _w, halo_case, _w)

COVERED = {entry for entry, _ in CASES.values()}


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
_BASE = {}


def _base(W, cid):
    """(engine, case, its contiguous run -- compared with the entry's reference once)"""
    if cid not in _BASE:
        eng, case = CASES[cid][1](W)
        assert case.entry == CASES[cid][0]
        run = sc.run_case(eng, case, "contiguous")
        assert run.rc == 0, (cid, run.rc)
        sc.check_strided(case, run, run)                   # (the guard words and the inputs of the contiguous run itself)
        sc.check_reference(case, run)
        _BASE[cid] = (eng, case, run)
    return _BASE[cid]


@pytest.mark.parametrize("mode", ["even", "odd"])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_strided_call(world, cid, mode):
    eng, case, base = _base(world, cid)
    sc.check_strided(case, base, sc.run_case(eng, case, mode))


def test_umat_engines_take_their_routes(world):
    """which form each engine of the UMAT cases runs: the wave-level form is on for all but MIMSEM_WAVE=0, the owner form holds a whole call
    in one work item where the two-launch form (MIMSEM_WAVE_OWN=0) cuts it into chunks of 8 levels; printed for the record"""
    st = (C.c_int * 5)()
    got = {}
    for key in ("default", "own1", "own0", "wave0", "balance"):
        e = world.eng("A", key)
        rc = e.L.mimsem_op_wave_stats(e.ctx, 9, st)
        got[key] = (rc, list(st))
        print("%-8s wave_stats(9 levels): on=%d %s  planned-list launches so far: %d" % (key, rc, list(st), e.L.mimsem_ctx_wave_balance_launches(e.ctx)))
    assert got["wave0"][0] == 0 and all(got[k][0] == 1 and got[k][1][0] > 0 for k in ("default", "own1", "own0", "balance"))
    assert all(world.eng("A", k).L.mimsem_ctx_wave_balance_launches(world.eng("A", k).ctx) == 0 for k in ("default", "own1", "own0", "wave0"))
