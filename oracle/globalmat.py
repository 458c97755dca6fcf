"""Global matrices of the numpy oracles (oracle/sw_oracle.py, oracle/horiz_oracle.py) -- TEST INFRASTRUCTURE ONLY.

One assembly pattern, two storages: MatSetValues(ADD_VALUES) of element blocks into a dense numpy array (small spheres, the
matrices the tests read directly), or the same blocks as COO triplets summed into a scipy.sparse CSR matrix (the benchmark
spheres: config 3's M1 has 62 208 rows).  Likewise every KSPSolve is a dense LU, or a sparse LU (SuperLU) cached per fixed
matrix.  scipy is imported in sparse mode only."""
import numpy as np


class GlobalMat:
    """a global matrix under assembly"""

    def __init__(self, shape, sparse):
        self.shape, self.sparse = shape, sparse
        self.last_wins = False
        if sparse:
            self.r, self.c, self.v = [], [], []
        else:
            self.M = np.zeros(shape)

    def add(self, rows, cols, blocks):
        """M[rows[e], cols[e]] += blocks[e] for every element e (rows [nEl, a], cols [nEl, b], blocks [nEl, a, b])"""
        rows, cols = np.asarray(rows), np.asarray(cols)
        blocks = np.asarray(blocks).reshape(rows.shape[0], rows.shape[1], cols.shape[1])
        if self.sparse:
            self.r.append(np.broadcast_to(rows[:, :, None], blocks.shape).ravel())
            self.c.append(np.broadcast_to(cols[:, None, :], blocks.shape).ravel())
            self.v.append(blocks.ravel())
        else:
            for e in range(rows.shape[0]):
                self.M[np.ix_(rows[e], cols[e])] += blocks[e]

    def insert(self, rows, cols, vals):
        """M[rows, cols] = vals (plain insert: an entry written twice keeps its last value)"""
        if self.sparse:
            rows, cols, vals = np.broadcast_arrays(np.asarray(rows), np.asarray(cols), np.asarray(vals, dtype=np.float64))
            self.r.append(rows.ravel()); self.c.append(cols.ravel()); self.v.append(vals.ravel())
            self.last_wins = True
        else:
            self.M[rows, cols] = vals

    def done(self):
        if not self.sparse:
            return self.M
        import scipy.sparse as sp
        r = np.concatenate(self.r) if self.r else np.zeros(0, np.int64)
        c = np.concatenate(self.c) if self.c else np.zeros(0, np.int64)
        v = np.concatenate(self.v) if self.v else np.zeros(0)
        if self.last_wins:
            key = r.astype(np.int64) * self.shape[1] + c
            _, first_of_reversed = np.unique(key[::-1], return_index=True)
            keep = key.size - 1 - first_of_reversed
            r, c, v = r[keep], c[keep], v[keep]
        return sp.coo_matrix((v, (r, c)), shape=self.shape).tocsr()


class Solver:
    """the oracles' KSPSolve: dense LU, or sparse LU with the factors of fixed matrices kept under a key"""

    def __init__(self, sparse):
        self.sparse, self.lu = sparse, {}

    def __call__(self, M, b, key=None):
        if not self.sparse:
            return np.linalg.solve(M, b)
        lu = self.lu.get(key) if key is not None else None
        if lu is None:
            from scipy.sparse.linalg import splu
            lu = splu(M.tocsc())
            if key is not None:
                self.lu[key] = lu
        return lu.solve(np.ascontiguousarray(b, dtype=np.float64))


def block2x2(A11, A12, A21, A22, sparse):
    if sparse:
        import scipy.sparse as sp
        return sp.bmat([[A11, A12], [A21, A22]], format="csr")
    n1, n2 = A11.shape[0], A22.shape[0]
    A = np.zeros((n1 + n2, n1 + n2))
    A[:n1, :n1] = A11; A[:n1, n1:] = A12; A[n1:, :n1] = A21; A[n1:, n1:] = A22
    return A
