#!/usr/bin/env python3
"""Generate the benchmark-size parity fixtures under tests/golden/ with the SPARSE mode of the numpy oracles
(oracle/sw_oracle.py, oracle/horiz_oracle.py: the C oracle's element blocks into scipy.sparse matrices, sparse LU for every solve).
Needs the repository and scipy only; the GPU-side tests read the .npz files and need neither.

  sw_config2_p3_ne16.npz  : bench.py's config 2 -- Williamson-2 (alpha = 0) on the 16x16x6 sphere, dt = 600 s, q from the mean
                            state, 4 Picard iterations.
  sw_config3_p3_ne24.npz  : bench.py's config 3 -- the Galewsky jet on the 24x24x6 sphere, dt = 360 s, upwinded q, 2 Picard
                            iterations (the step bench.py times).
      each: the Coriolis 0-form fg, the start state (u0, h0: the oracle's init1 / init2 of the analytic fields), the state after
      one step (u1, h1) and the step's increments (du, dh) as sketches S y (K = 64) and norms |y|, and the oracle's Picard history
      |dx| / |x| in full.  (The full states would be 0.4 MB for config 2 and 1.2 MB for config 3.)  The tests build the start state
      on the device from the same analytic fields, check it against the sketch, and step from there.
  horiz_p3_ne24_nk10.npz  : HorizSolve's right-hand sides on the config-4 sphere with 10 levels (nk * n1 = 622 080: past both
      thresholds of the C++ host's check-norm row reductions).  Inputs come from tests/helpers.py::hash_uniform times the stored
      physical scales, so the tests rebuild them bit for bit; every output y is stored as its sketch S y (K = 64) and |y|.

The SW fixtures hold one step at dt: tests/cpp/test_sw.cpp takes them with its "no-half-step" argument.
Runtime: about 2 minutes (config 2 ~11 s, config 3 ~30 s, HorizSolve ~90 s); the three files are ~20 KB together.  The output is the same bits on every run: the arrays
are deterministic and the archive members carry a fixed timestamp.
Usage: python tests/golden/make_step_fixtures.py [sw2] [sw3] [horiz]    (default: all three)
"""
import io
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

# (file, ne, dt, Picard iterations, q_exact, initial condition)
SW_CASES = {"sw2": ("sw_config2_p3_ne16.npz", 16, 600.0, 4, True, "williamson2"),
            "sw3": ("sw_config3_p3_ne24.npz", 24, 360.0, 2, False, "galewsky")}
HORIZ_FILE, HORIZ_NE, HORIZ_NK = "horiz_p3_ne24_nk10.npz", 24, 10
PN = 3


def save_npz(path, **arrays):
    """np.savez_compressed without the wall-clock timestamps: regenerating a fixture gives the same file"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def sw_sphere(ne):
    """the src/-flavour sphere of tests/test_gpu_sweqn.py and bench.py's sw_extras: unit thickness, signed Jacobian determinant"""
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(PN, ne, 6); coords = sphere_coords(PN, ne)
    topos = [Topo(cs, p, 1) for p in range(6)]
    geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
    return cs, coords, topos, geoms


def sw_initial_fields(xq, ic):
    """(u, v) and h of the case's analytic start at the points xq (a torch [n, 3] tensor, on the host or the device)"""
    from mimsem_amd.sweqn import galewsky, williamson2
    return williamson2(xq, alpha=0.0) if ic == "williamson2" else galewsky(xq)


SW_FIELDS = ("fg", "u0", "h0", "u1", "h1", "du", "dh")


def sw_step(ne, dt, nits, q_exact, ic):
    """the oracle's start state and one SWEqn::solve step from it, in full"""
    import torch
    from oracle import sw_oracle
    cs, coords, topos, geoms = sw_sphere(ne)
    O = sw_oracle.SWOracle(cs, topos, geoms, coords, sparse=True)
    uq, hq = sw_initial_fields(torch.as_tensor(O.xq), ic)
    u0, h0 = O.init1(uq.numpy()), O.init2(hq.numpy())
    u1, h1 = O.solve(u0, h0, dt, nits=nits, q_exact=q_exact)
    return dict(u0=u0, h0=h0, fg=O.fg, u1=u1, h1=h1, du=u1 - u0, dh=h1 - h0, history=np.array(O.history))


def sw_fixture(full, ne, dt, nits, q_exact):
    """what the SW fixture keeps of sw_step's arrays: a sketch and the norm of each field, the history in full"""
    from tests.helpers import sketch
    res = dict(history=full["history"], dt=np.float64(dt), nits=np.int32(nits), q_exact=np.int32(q_exact), ne=np.int32(ne), pn=np.int32(PN))
    for name in SW_FIELDS:
        res["S_" + name] = sketch(full[name]); res["norm_" + name] = np.float64(np.linalg.norm(full[name]))
    return res


def horiz_sphere(ne, nk):
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import z_levels
    cs = CubedSphere(PN, ne, 6); coords = sphere_coords(PN, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    levs = z_levels(nk, geoms[0].n0)
    for g in geoms:
        g.set_levels(levs)
    return cs, coords, topos, geoms, levs


def horiz_inputs(nk, n1, n2, area, dz):
    """the fields of tests/test_gpu_next_rows.py::test_horizsolve_right_hand_sides (same physical scaling: 2-form dofs ~ value * area *
    thickness, 1-form dofs ~ value * edge length * thickness), drawn from hash_uniform instead of numpy's rng"""
    from tests.helpers import hash_uniform as hu
    ln = np.sqrt(area)
    f = {}
    f["u1"] = hu(1, (nk, n1), -1.7, 1.7) * 20.0 * ln * dz
    f["u2"] = f["u1"] * (1 + 0.05 * hu(2, (nk, n1), -1.7, 1.7))
    f["h1"] = hu(3, (nk, n2), 0.8, 1.2) * area * dz
    f["h2"] = f["h1"] * (1 + 0.01 * hu(4, (nk, n2), -1.7, 1.7))
    f["theta"] = hu(5, (nk, n2), 290.0, 310.0) * area * dz
    f["Pi"] = hu(6, (nk, n2), 900.0, 1000.0) * area * dz
    f["velz1"] = hu(7, (nk - 1, n2), -1.7, 1.7) * area
    f["velz2"] = f["velz1"] * (1 + 0.05 * hu(8, (nk - 1, n2), -1.7, 1.7))
    f["dudz1"] = hu(9, (nk - 1, n1), -1.7, 1.7) * 1e-3 * ln
    f["dudz2"] = f["dudz1"] * 1.1
    f["Fz"] = f["velz1"] * 0.7
    f["dwdx1"] = hu(10, (nk - 1, n1), -1.7, 1.7) * 2e-4 * ln
    f["dwdx2"] = f["dwdx1"] * 0.9
    return f


# the three momentum_rhs_ec argument combinations of the existing tests: (name, Fx and Fz given, dwdx given)
MOMENTUM_CASES = (("fuA", False, False), ("fuB", True, False), ("fuC", True, True))


def horiz_rhs(ne, nk):
    from oracle import horiz_oracle as ho
    from tests.helpers import sketch
    cs, coords, topos, geoms, levs = horiz_sphere(ne, nk)
    gd = ho.GlobalDense(cs, topos, geoms, coords, levs, sparse=True)
    H = ho.HorizOracle(gd)
    area = np.mean([P.det.mean() for P in gd.P]) * 4.0 / (PN * PN); dz = np.mean([P.thick.mean() for P in gd.P])
    f = horiz_inputs(nk, gd.N1, gd.N2, area, dz)
    u1, u2, h1, h2, th, Pi = f["u1"], f["u2"], f["h1"], f["h2"], f["theta"], f["Pi"]
    velz, velz2, dudz, dudz2 = f["velz1"], f["velz2"], f["dudz1"], f["dudz2"]
    out = {}
    dF, dG, Fk, Gk = H.advection_rhs_ec(u1, u2, h1, h2, th)
    out.update(dF=dF, dG=dG, Fk=Fk, Gk=Gk, fg=H.fg)
    out["Phi"] = np.stack([H.diagnose_Phi(lev, u1[lev], u2[lev], velz, velz2) for lev in range(nk)])
    out["q"] = np.stack([H.diagnose_q(lev, h1[lev], u1[lev]) for lev in range(nk)])
    k2i = {}
    for name, use_F, use_w in MOMENTUM_CASES:
        fu, k2i[name] = [], 0.0
        for lev in range(nk):
            y, k = H.momentum_rhs_ec(lev, th[lev], dudz, dudz2, velz, velz2, Pi[lev], u1[lev], u2[lev], h1[lev], h2[lev],
                                     Fx=Fk[lev] if use_F else None, Fz=f["Fz"] if use_F else None, Fk=Fk[lev],
                                     dwdx1=f["dwdx1"] if use_w else None, dwdx2=f["dwdx2"] if use_w else None)
            fu.append(y); k2i[name] += k
        out[name] = np.stack(fu)
    res = dict(area=np.float64(area), dz=np.float64(dz), nk=np.int32(nk), ne=np.int32(ne), pn=np.int32(PN), del2=np.float64(H.del2),
               k2i_fuA=np.float64(k2i["fuA"]), k2i_fuB=np.float64(k2i["fuB"]), k2i_fuC=np.float64(k2i["fuC"]))
    for name, y in out.items():
        res["S_" + name] = sketch(y); res["norm_" + name] = np.float64(np.linalg.norm(y))
    return res


def main(which):
    from oracle import pyoracle
    pyoracle.build(ref=False)
    for key in which:
        t0 = time.time()
        if key in SW_CASES:
            fname, ne, dt, nits, q_exact, ic = SW_CASES[key]
            save_npz(os.path.join(HERE, fname), **sw_fixture(sw_step(ne, dt, nits, q_exact, ic), ne, dt, nits, q_exact))
        else:
            fname = HORIZ_FILE
            save_npz(os.path.join(HERE, fname), **horiz_rhs(HORIZ_NE, HORIZ_NK))
        print("%s: %.1f s" % (fname, time.time() - t0), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["sw2", "sw3", "horiz"])
