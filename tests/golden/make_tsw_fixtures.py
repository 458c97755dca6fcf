#!/usr/bin/env python3
"""Generate tests/golden/tsw_galewsky_p3_ne24.npz with the SPARSE mode of the thermal shallow-water oracle (tests/tsw_oracle.py:
ThermalSW_EEC_2::solve_rk restated over the scipy.sparse matrices of oracle/sw_oracle.py, sparse LU for every solve).

  tsw_galewsky_p3_ne24.npz : config 3 -- the GalewskyTSW_2 state (src/GalewskyTSW_2.cpp:118-126) on the 24x24x6 p = 3 sphere,
      one solve_rk(30 s).  u, h, S before (u0, h0, S0: the oracle's projections of the analytic fields) and after (u1, h1, S1) as
      sketches S y (K = 64) and norms |y|, and the six invariants (mass, buoyancy, energy, enstrophy, vorticity, entropy) before
      (inv0) and after (inv1), in that order.  (The full states would be 1.7 MB.)

Runtime: about 25 s; the file is ~5 KB.  The output is the same bits on every run: the arrays are deterministic and the archive members
carry a fixed timestamp (make_step_fixtures.save_npz).
Usage: python tests/golden/make_tsw_fixtures.py [out_dir]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FILE, NE, PN, DT = "tsw_galewsky_p3_ne24.npz", 24, 3, 30.0
INVARIANTS = ("mass", "buoyancy", "energy", "enstrophy", "vorticity", "entropy")


def build(out_dir=HERE):
    from oracle import pyoracle
    pyoracle.build(ref=False)
    from tests.golden.make_step_fixtures import save_npz
    from tests.helpers import sketch
    from tests.test_tsw_oracle import galewsky_state, tsw_sphere
    t0 = time.time()
    *_, O = tsw_sphere(PN, NE, sparse=True)
    x0 = galewsky_state(O)
    i0 = O.invariants(*x0)
    x1 = O.solve_rk(*x0, DT)
    i1 = O.invariants(*x1)
    arrays = dict(dt=np.float64(DT), inv0=np.array([i0[k] for k in INVARIANTS]), inv1=np.array([i1[k] for k in INVARIANTS]))
    for name, a in zip(("u0", "h0", "S0", "u1", "h1", "S1"), (*x0, *x1)):
        arrays[name + "_sketch"] = sketch(a)
        arrays[name + "_norm"] = np.float64(np.linalg.norm(a))
    path = os.path.join(out_dir, FILE)
    save_npz(path, **arrays)
    print("%s: %.1f s, %d bytes" % (path, time.time() - t0, os.path.getsize(path)))
    return path


if __name__ == "__main__":
    build(sys.argv[1] if len(sys.argv) > 1 else HERE)
