"""Shared builders for the parity tests: the same patch handed to the oracle (CPU checker) and to the
HIP engine, on real cubed-sphere geometry with a stretched level set."""
import numpy as np

from mimsem_amd.geom import Geom
from mimsem_amd.mesh import CubedSphere, sphere_coords
from mimsem_amd.topo import Topo

from mimsem_amd.workloads import SCALE, z_levels  # noqa: F401  (kept importable from here for the tests)


def make_patch(oracle, pn=3, ne=4, nprocs=6, pi=0, nk=3, seed=0):
    rng = np.random.default_rng(seed)
    cs = CubedSphere(pn, ne, nprocs)
    coords = sphere_coords(pn, ne)
    topo = Topo(cs, pi, nk)
    geom = Geom(topo, cs, coords, nk)
    geom.set_levels(z_levels(nk, geom.n0, rng))
    P = oracle.Patch(pn, pn, cs.nel, nk)
    P.set_sphere_geometry(coords[cs.patches[pi].loc0])
    P.set_levels(geom.levs)
    return cs, topo, geom, P, rng


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel(); b = np.asarray(b, dtype=np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---- extended-precision reference for the column Schur solves (round-1 VERDICT "What's weak" 2) -------------------------------
def dense_from_band(blocks, nk, n2, lo):
    """[nk][2*lo+1][n2][n2] block bands (block column = row - lo + b) -> dense (nk*n2)^2"""
    N = nk * n2
    M = np.zeros((N, N))
    for k in range(nk):
        for b in range(2 * lo + 1):
            c = k - lo + b
            if 0 <= c < nk:
                M[k*n2:(k+1)*n2, c*n2:(c+1)*n2] = blocks[k, b]
    return M


def _ld_lu_solve(A, b, bw):
    LU = np.array(A, dtype=np.longdouble); x = np.array(b, dtype=np.longdouble)
    N = LU.shape[0]
    for i in range(N):
        r1 = min(N, i + 1 + bw); c1 = min(N, i + 1 + 2 * bw)
        p = i + int(np.argmax(np.abs(LU[i:r1, i])))
        if p != i:
            LU[[i, p]] = LU[[p, i]]; x[[i, p]] = x[[p, i]]
        f = LU[i+1:r1, i] / LU[i, i]
        LU[i+1:r1, i+1:c1] -= np.outer(f, LU[i, i+1:c1])
        x[i+1:r1] -= f * x[i]
    for i in range(N - 1, -1, -1):
        c1 = min(N, i + 1 + 2 * bw)
        x[i] = (x[i] - LU[i, i+1:c1] @ x[i+1:c1]) / LU[i, i]
    return x


def ld_solve(A, b):
    """A x = b by banded LU with partial pivoting in numpy.longdouble (x87 80-bit on the x86 hosts: eps 1.1e-19) plus one
    refinement step -- the 'exact' solution of a system whose entries are given in double"""
    A = np.asarray(A, dtype=np.float64)
    nz = np.nonzero(A)
    bw = int(np.abs(nz[0] - nz[1]).max()) if nz[0].size else 0
    Al = A.astype(np.longdouble); bl = np.asarray(b, dtype=np.longdouble)
    x = _ld_lu_solve(A, b, bw)
    x = x + _ld_lu_solve(A, bl - Al @ x, bw)
    return x


def _rel_ld(a, b):
    a = np.asarray(a, dtype=np.longdouble); b = np.asarray(b, dtype=np.longdouble)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), np.longdouble(1e-300)))


def solve_error_budget(L_hip, rhs_hip, d_hip, L_orc, rhs_orc, d_orc):
    """Where does |d_hip - d_orc| come from?  Each side is compared with the extended-precision solution of ITS OWN system
    (solver error: block-Thomas + refinement on the device, dense LU in the oracle); the two extended-precision solutions differ
    by what cond(L) makes of the round-off difference between the two assembled operators / right-hand sides.  All relative L2."""
    x_h, x_o = ld_solve(L_hip, rhs_hip), ld_solve(L_orc, rhs_orc)
    return {"rel_L": rel_l2(L_hip, L_orc), "rel_rhs": rel_l2(rhs_hip, rhs_orc), "cond": float(np.linalg.cond(L_orc)),
            "hip_vs_own_system": _rel_ld(d_hip, x_h), "oracle_vs_own_system": _rel_ld(d_orc, x_o),
            "diff_of_exact_solutions": _rel_ld(x_h, x_o), "diff": rel_l2(d_hip, d_orc)}


# ---- hashed inputs and sketched outputs for the benchmark-size fixtures (tests/golden/make_step_fixtures.py) ---------------------
# An integer hash, not numpy's rng: the GPU-side test rebuilds the inputs and the probe matrix bit for bit from (seed, index) alone,
# so neither has to be stored; only K numbers per output are.
SKETCH_K = 64


def _splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_uniform(seed, shape, lo=0.0, hi=1.0):
    """uniform numbers in [lo, hi): splitmix64 of (seed << 40) + i for the flat index i, top 53 bits"""
    n = int(np.prod(shape))
    z = _splitmix64((np.uint64(seed) << np.uint64(40)) + np.arange(n, dtype=np.uint64))
    u = (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return (lo + (hi - lo) * u).reshape(shape)


_PROBES = {}


def probe_matrix(n, K=SKETCH_K):
    """the K x n sketching matrix S: S[j, i] = +-1/sqrt(K) from the low bit of splitmix64(j*n + i) (kept as int8 signs; 1/sqrt(K) applied
    by sketch())"""
    if (K, n) not in _PROBES:
        S = np.empty((K, n), dtype=np.int8)
        i = np.arange(n, dtype=np.uint64)
        for j in range(K):
            S[j] = 1 - 2 * (_splitmix64(np.uint64(j) * np.uint64(n) + i) & np.uint64(1)).astype(np.int8)
        _PROBES[(K, n)] = S
    return _PROBES[(K, n)]


def sketch(y, K=SKETCH_K):
    """S y for the flattened y: a random projection that keeps |S e| close to |e| for any error e fixed before S is drawn
    (a single-entry error exactly: every column of S has norm 1)"""
    y = np.asarray(y, dtype=np.float64).ravel()
    S = probe_matrix(y.size, K)
    return np.array([np.dot(S[j].astype(np.float64), y) for j in range(K)]) / np.sqrt(K)


def sketch_rel_err(y, s_ref, norm_ref):
    """|S y - S y_ref| / |y_ref| from the stored sketch S y_ref and norm |y_ref|"""
    return float(np.linalg.norm(sketch(y, len(s_ref)) - s_ref) / norm_ref)
