"""The small cubed sphere of the horizontal momentum update's tests (tests/test_hmomentum_cpu.py, tests/test_gpu_hmomentum.py): 6 x 2 x 2
elements, 3 levels, and on it the dense M1 (Umat with the vertical flag) and M1ray(tau) (Umat_ray) of a level, assembled from the oracle's
element matrices in the slot numbering the device uses (DeviceMesh, numbering="global": 1-forms by global id, 2-forms element by element)."""
import numpy as np

from mimsem_amd.workloads import SCALE, z_levels

K_F = 1.1574074074074073e-05        # compute_k_v's k_f, eul/Assembly.cpp:1846-1856
NE, NK = 2, 3


def _exner_fields(P, r, lev, lo=0.5, hi=1.0):
    """_exner_fields of tests/test_gpu_horizontal.py, restated (the sigma range of the level is a parameter here): 2-form DoFs whose point
    values (after /det * thickInv) are Exner pressures cp*sigma^(R/cp), sigma in [lo, hi] per element at the level, [0.98, 1.02] at level 0"""
    n = P.n
    dx = np.diff(P.arr("nx", (n + 1,)))
    cell = np.outer(dx, dx).reshape(-1)                                       # integral of 1 over each face of the reference element
    i2 = P.elinds("n2")
    iq = P.elinds("q")
    out = []
    for (k, a, b) in ((lev, lo, hi), (0, 0.98, 1.02)):
        f = np.zeros(P.n2)
        for e in range(P.nEl):
            sig = r.uniform(a, b)
            val = 1004.5 * sig ** (287.0 / 1004.5)
            scale_e = P.det[e].mean() / P.thickInv[k][iq[e]].mean()
            f[i2[e]] = val * cell * scale_e * (1.0 + 1e-3 * r.standard_normal(n * n))
        out.append(f)
    return out


class Sphere:
    def __init__(self, oracle, pn):
        from mimsem_amd.device import DeviceMesh
        from mimsem_amd.geom import Geom
        from mimsem_amd.mesh import CubedSphere, sphere_coords
        from mimsem_amd.topo import Topo
        self.pn = pn
        cs = CubedSphere(pn, NE, 6); coords = sphere_coords(pn, NE)
        self.topos = [Topo(cs, p, NK) for p in range(6)]
        self.geoms = [Geom(t, cs, coords, NK) for t in self.topos]
        levs = z_levels(NK, self.geoms[0].n0)
        for g in self.geoms:
            g.set_levels(levs)
        self.dm = DeviceMesh(self.topos, self.geoms, nk=NK, numbering="global")
        self.patches = []
        for t in self.topos:
            P = oracle.Patch(pn, pn, cs.nel, NK)
            P.set_sphere_geometry(coords[cs.patches[t.pi].loc0]); P.set_levels(levs)
            self.patches.append(P)
        P = self.patches[0]
        self.nElp, self.n1e, self.n2e = P.nEl, P.n1e, P.n2e
        self.n1, self.n2 = self.dm.n1, self.dm.n2
        self.idx = np.concatenate([self.dm.inds1x, self.dm.inds1y], axis=1)           # [nEl, 2 n1e]: x edges, then y edges
        self._i2 = [Q.elinds("n2") for Q in self.patches]
        self._m1 = {}

    # ---- 2-form fields: patch-local for the oracle, element by element for the device ----
    def exner(self, r, lev, lo=0.5, hi=1.0):
        """(exner at `lev`, exner at level 0) as lists of the six patch-local vectors"""
        both = [_exner_fields(P, r, lev, lo, hi) for P in self.patches]
        return [b[0] for b in both], [b[1] for b in both]

    def to_device(self, loc):
        return np.concatenate([f[i2].reshape(-1) for f, i2 in zip(loc, self._i2)])

    # ---- element matrices [nEl, 2 n1e, 2 n1e] and their assembly ----
    def _blocks(self, em):
        n = self.n1e
        return em.reshape(-1, 2, 2, n, n).transpose(0, 1, 3, 2, 4).reshape(-1, 2 * n, 2 * n)

    def m1_elmats(self, k, flag=1):
        return self._blocks(np.concatenate([P.op_elmats("UMAT", k, SCALE, flag) for P in self.patches]))

    def ray_elmats(self, k, tau, ek, es):
        return self._blocks(np.concatenate([P.umat_ray(np.zeros(P.n1), k, SCALE, tau, a, b)[1] for P, a, b in zip(self.patches, ek, es)]))

    def assemble(self, blocks):
        M = np.zeros((self.n1, self.n1))
        for e in range(blocks.shape[0]):
            M[np.ix_(self.idx[e], self.idx[e])] += blocks[e]
        return M

    def m1(self, k):
        if k not in self._m1:
            self._m1[k] = self.assemble(self.m1_elmats(k))
        return self._m1[k]

    def m1ray(self, k, tau, ek, es):
        return self.assemble(self.ray_elmats(k, tau, ek, es))

    def precond(self, k):
        """MassSolver's element-block preconditioner of level k: P = sum_e R_e^T D_e (M1_e)^-1 D_e R_e, D_e = 1/multiplicity of the edge"""
        mult = np.bincount(self.idx.reshape(-1), minlength=self.n1).astype(np.float64)
        P = np.zeros((self.n1, self.n1))
        for e, B in enumerate(self.m1_elmats(k)):
            d = 1.0 / mult[self.idx[e]]
            P[np.ix_(self.idx[e], self.idx[e])] += d[:, None] * np.linalg.inv(B) * d[None, :]
        return P
