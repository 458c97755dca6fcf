"""tests/column_cases.py -- the small meshes of tests/test_gpu_column_every_column.py, the map from a context column to (oracle patch, element),
the inputs, and the per-column comparison.  TEST INFRASTRUCTURE ONLY; no GPU is touched here (tests/test_column_cases_cpu.py checks all of it
on the CPU).

The column counts are chosen against the kernels' mappings, not against a workload: the block-Thomas and pentadiagonal kernels put four columns
in one wavefront (two in their two-sided forms, taken for even nk), the row-per-lane assembly four (column, level) tasks, the wave-per-column
sweep 64 / n2e columns (16, 7, 4 at orders 2, 3, 4).  Several one-element patches in ONE context are the only way to column counts that are not
squares; such a context takes the global numbering and one oracle.Patch per patch.

    name  mesh                                                 columns  what it reaches
    S1    CubedSphere(pn, 1, 6), patch 1, local                   1     the one-patch shape of orders 5 and 6 (uh is a row of the patch)
    S3    CubedSphere(pn, 1, 6), patches 1, 3, 4, global          3     one partial wavefront with three live rows
    S5    same, patches 0..4                                      5     4 + 1 columns; 2 + 2 + 1 two-sided; 25 / 20 tasks at nk = 5
    S6    same, all six                                           6     4 + 2 columns; 24 / 18 tasks at nk = 4 (a task tail of two rows)
    S9    CubedSphere(pn, 3, 6), patch 4, local                   9     7 + 2 in the order-3 sweep; two full wavefronts + 1 in the row kernels
    S18   CubedSphere(2, 3, 6), patches 1 and 4, global          18     16 + 2 in the order-2 sweep
    B9    PeriodicBox(1, 3, 1), local                             9     n2e = 1 (the sphere has no coordinates at order 1), odd nk
    B4    PeriodicBox(1, 2, 1), local                             4     n2e = 1, even nk
"""
import types

import numpy as np

from tests.helpers import rel_l2, z_levels

TOL = 1e-10
HARD = 1e-9

SPHERES = dict(S1=(1, (1,), "local"), S3=(1, (1, 3, 4), "global"), S5=(1, (0, 1, 2, 3, 4), "global"), S6=(1, (0, 1, 2, 3, 4, 5), "global"),
               S9=(3, (4,), "local"), S18=(3, (1, 4), "global"))
BOXES = dict(B9=(3, 5), B4=(2, 4))                       # name -> (ne, nk); order 1
ONE_PATCH = ("S1", "S9", "B9", "B4")                     # shapes whose 1-form rows are rows of the one patch: the entries that take uh


def all_cases():
    """(shape, order, nk) of every case: orders 2..4 on S3 S5 S6 S9 (order 2 also S18), orders 5 and 6 on S3 S5 (their kernels map one column
    to a workgroup: no position inside a wavefront) and on the one-patch S1, order 1 on the boxes; every sphere at an even and an odd nk
    (two-sided / one-sided Thomas and pentadiagonal kernels; 4 is the smallest count the Rayleigh layer and solve_schur_column_3 take)"""
    out = []
    for pn in (2, 3, 4):
        for name in ("S3", "S5", "S6", "S9") + (("S18",) if pn == 2 else ()):
            out += [(name, pn, nk) for nk in (4, 5)]
    for pn in (5, 6):
        for name in ("S1", "S3", "S5"):
            out += [(name, pn, nk) for nk in (4, 5)]
    out += [(name, 1, nk) for name, (_, nk) in BOXES.items()]
    return out


case_id = lambda c: "%s_p%d_nk%d" % c


class Case:
    """one context's worth of columns: `topos`, `geoms`, `dm` (the DeviceMesh), `patches` (one oracle.Patch per patch, in list order) and
    `where[e] = (patch position, element of that patch)`; P0 = patches[0] answers the questions that do not depend on the patch (dims)"""

    def __init__(self, name, pn, nk, topos, geoms, patches, numbering):
        from mimsem_amd.device import DeviceMesh
        self.name, self.pn, self.nk, self.numbering = name, pn, nk, numbering
        self.topos, self.geoms, self.patches = topos, geoms, patches
        self.dm = DeviceMesh(topos, geoms, nk=nk, numbering=numbering)
        self.P0 = patches[0]
        self.n2e, self.nEl = pn * pn, self.dm.nEl
        self.where, self.el0 = [], []
        for i, t in enumerate(topos):                    # patches are laid out in list order (PatchView.el0 of test_gpu_fullsize_oracle.py)
            self.el0.append(len(self.where))
            self.where += [(i, le) for le in range(t.nElsX ** 2)]
        assert len(self.where) == self.nEl
        self.one_patch = len(topos) == 1
        self.label = "%s p=%d nk=%d (%d columns)" % (name, pn, nk, self.nEl)

    def col(self, e):
        """(oracle patch, ex, ey) of context column e"""
        i, le = self.where[e]
        P = self.patches[i]
        return P, le % P.nElsX, le // P.nElsX

    def shape_ns(self):
        """what test_gpu_column._col_fields / _uh read of a patch, for the whole context"""
        return types.SimpleNamespace(nEl=self.nEl, nk=self.nk, n2e=self.n2e, det=self.dm.det, thick=self.dm.thick, thickInv=self.dm.thickInv,
                                     n1=self.dm.n1)

    def fields(self, seed=3):
        """the physically scaled column fields of test_gpu_column._col_fields, one row per context column"""
        from tests.test_gpu_column import _col_fields
        return _col_fields(self.shape_ns(), seed=seed)

    def rhs(self, seed):
        """the four right-hand sides of the column solves, standard_normal * 1e8 as in tests/test_gpu_column.py"""
        r = np.random.default_rng(seed)
        return [r.standard_normal((self.nEl, n * self.n2e)) * 1e8 for n in (self.nk - 1, self.nk, self.nk, self.nk)]

    def uh(self, r, dt):
        """horizontal velocities [nk][n1] of the one patch whose departure shift is ~0.3 of the SMALLEST GLL SUB-CELL of the reference element
        (0.3, 0.15, 0.083, 0.052, 0.035, 0.025 of the element at orders 1..6): what a stable advection step moves.  test_gpu_column._uh shifts by
        0.3 of the whole element at every order; at orders 5 and 6 that is 2.5 and 3.5 sub-cells, the blocks of the upwinded VA2 of
        diagTheta_up then have cond 4e9 ... 7e14 (whatever the density: also with rho constant) and the oracle's own double-precision solve
        is 5e-10 / 2e-6 off the extended-precision solution of its system -- no reference for a 1e-10 comparison.  The scale is held by a
        condition on the inputs, not by the device: tests/test_column_cases_cpu.py::test_the_upwinded_theta_system_is_well_posed"""
        from mimsem_amd.geom import gll_points
        assert self.one_patch
        P = self.P0
        x = gll_points(self.pn)
        vs = P.det.mean() / P.thickInv.mean(axis=1) * 0.3 * 0.5 * float(x[1] - x[0]) / dt
        return r.uniform(-1, 1, (P.nk, P.n1)) * vs[:, None]

    def latitudes(self, seed=77):
        """[nEl, mp12] latitude of the quadrature points, the array AssembleTempForcing_HS reads.  The sphere has its own (Geom::s); the box
        has none, so seeded values in (-pi/2, pi/2) are written into the oracle patch and the same array goes to the device"""
        assert self.one_patch
        P = self.P0
        if self.name in BOXES:
            P.sq[:, 1] = np.random.default_rng(seed).uniform(-1.5, 1.5, P.n0q)
        return np.ascontiguousarray(P.sq[:, 1][P.elinds("q")])


def build_case(oracle, name, pn, nk):
    """the meshes of the table above, with perturbed (seeded) levels, and their oracle patches"""
    from mimsem_amd.topo import Topo
    seed = 1000 * pn + 10 * nk + sum(map(ord, name))
    if name in BOXES:
        from mimsem_amd.geom import BoxGeom
        from mimsem_amd.mesh import PeriodicBox, box_coords
        ne = BOXES[name][0]
        assert pn == 1 and nk == BOXES[name][1]
        lx = 2.0 * ne                                    # det = 1, as tests/box_schur2_case.make_box
        bx = PeriodicBox(pn, ne, 1); coords = box_coords(pn, ne, lx)
        t = Topo(bx, 0, nk)
        g = BoxGeom(t, bx, coords, nk, lx)
        g.set_levels(z_levels(nk, g.n0, np.random.default_rng(seed), ztop=300.0 * nk))
        P = oracle.Patch(pn, pn, bx.nel, nk)
        P.set_metric(g.det, g.J); P.set_levels(g.levs)
        return Case(name, pn, nk, [t], [g], [P], "local")
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    ne, pis, numbering = SPHERES[name]
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    rng = np.random.default_rng(seed)
    topos = [Topo(cs, pi, nk) for pi in pis]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    patches = []
    for t, g, pi in zip(topos, geoms, pis):
        g.set_levels(z_levels(nk, g.n0, rng))            # every patch its own draw: no two columns of a case share a level set
        P = oracle.Patch(pn, pn, cs.nel, nk)
        P.set_sphere_geometry(coords[cs.patches[pi].loc0])
        P.set_levels(g.levs)
        patches.append(P)
    return Case(name, pn, nk, topos, geoms, patches, numbering)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------
def column_errors(got, want):
    """relative L2 error of every column on its own: got, want [nEl, ...]"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.array([rel_l2(got[e], want[e]) for e in range(want.shape[0])])


def failing_columns(got, want, tol=TOL):
    """(indices of the columns whose own relative L2 error is not below tol -- a NaN fails --, the errors)"""
    err = column_errors(got, want)
    return [int(e) for e in np.nonzero(~(err < tol))[0]], err


def assert_columns(what, got, want, tol=TOL):
    """every column below tol on its own norm: a small-magnitude column cannot hide in a whole-array norm.  Returns the worst error;
    the failure names the columns by index"""
    bad, err = failing_columns(got, want, tol)
    assert not bad, "%s: column%s %s above %.1e: %s (worst column %d)" % (
        what, "s" if len(bad) > 1 else "", ", ".join(str(e) for e in bad), tol, ", ".join("%.3e" % err[e] for e in bad), int(np.nanargmax(err)))
    return float(err.max())
