"""Energetics.column on the bench mesh (p = 3, 24 x 24 x 6 cubed sphere, 30 levels: 3 456 columns): the fused kernel route
(mimsem_euler_energetics_column) against the composed route (Energetics.column_composed), timed beside each other in one process.

Device events around batches of CALLS calls (one call is tens of microseconds: a batch is timed, not a call), warm-up first, the two routes
alternating batch by batch, the median and the spread (min .. max) of SAMPLES batches per route.  The outputs of the two routes are compared
first (relative to the larger of |a|, |b|).  Writes profiles/energetics_column.txt (or the path given)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PN, NE, NPATCH, NK = 3, 24, 24, 30
WARMUP, CALLS, SAMPLES = 20, 50, 21


def main(path):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.vertsolve import VertSolve
    from mimsem_amd.workloads import z_levels
    if not torch.cuda.is_available():
        raise SystemExit("prof_energetics_column: no GPU (a timing needs one)")
    cs = CubedSphere(PN, NE, NPATCH); coords = sphere_coords(PN, NE)
    topos = [Topo(cs, p, NK) for p in range(NPATCH)]
    geoms = [Geom(t, cs, coords, NK) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(NK, g.n0))
    eng = Engine(DeviceMesh(topos, geoms, nk=NK, numbering="global"))
    vs = VertSolve(eng, 0.0)
    en = Energetics(eng, vs)
    r = np.random.default_rng(7)
    n2 = eng.n2e
    velz = eng.tensor(r.standard_normal((eng.nEl, (NK - 1) * n2)))
    rho = eng.tensor(r.uniform(0.8, 1.2, (eng.nEl, NK * n2)))
    levs = np.zeros((NK + 1, eng.mesh.nq))
    for g in geoms:
        levs[:, np.searchsorted(eng.mesh.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    zv = vs.init_gz(levs)
    en.set_geopotential(zv)
    routes = {"fused": lambda: eng.energetics_column(velz, rho, zv), "composed": lambda: en.column_composed(velz, rho, zv)}
    a, b = routes["fused"]().tolist(), routes["composed"]().tolist()
    diff = [abs(x - y) / max(abs(x), abs(y)) for x, y in zip(a, b)]
    for fn in routes.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(SAMPLES):
        for k, fn in routes.items():                      # alternating: both routes see the same drift of the machine
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(CALLS):
                fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / CALLS)
    lines = ["Energetics.column, p = %d, %d x %d x 6 sphere, %d levels: %d columns; %s" % (PN, NE, NE, NK, eng.nEl, torch.cuda.get_device_name(0)),
             "device events around batches of %d calls, %d warm-up calls, %d batches per route, routes alternating" % (CALLS, WARMUP, SAMPLES),
             "fused vs composed output, relative: kev %.2e  k2p %.2e  p2k %.2e  pe %.2e" % tuple(diff)]
    for k in routes:
        v = np.array(ms[k]) * 1e3
        lines.append("%-9s us per call: median %8.2f   min %8.2f   max %8.2f" % (k, np.median(v), v.min(), v.max()))
    lines.append("composed / fused (medians): %.2f" % (np.median(ms["composed"]) / np.median(ms["fused"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "energetics_column.txt"))
