#!/usr/bin/env python3
"""One Newton iteration of VertSolve.solve_schur_2 (VertSolve::solve_schur_2, eul/VertSolve.cpp:1059-1246) without horizontal forcing, the
fused route (mimsem_column_newton2_*) against the composed one (single-operator entry points: the kernels the loop had before the fused
entries existed), on
  bench : p = 3, 24 x 24 x 6 elements x 30 levels (the benchmark mesh), dt = 30, Rayleigh layer on
  box   : p = 4, 32 x 32 periodic box x 64 levels (BASELINE config 5), dt = 0.5, schur3_flags = 3, rayleigh = 0
Both routes are warmed up, then timed ALTERNATELY: device events around batches of `--its` iterations (tol = 0: every batch runs them all,
the per-iteration read-back of the norms included -- it belongs to the loop), `--reps` batches each; medians with min and max.  Device
activities per iteration (kernel launches and the read-back copy of the four norms) are counted from a trace of the process (batches of 3
and of 1 iterations, difference / 2).
  usage: prof_schur2.py [--mesh bench|box|both] [--bench-orders 3] [--its 4] [--reps 9] [--out profiles/schur2_newton.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mimsem_amd.vertsolve import VertSolve  # noqa: E402


def bench_case(rng, pn=3):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom, gll_points
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import z_levels
    nk = bench.NK
    cs = CubedSphere(pn, 24, 24); coords = sphere_coords(pn, 24)
    topos = [Topo(cs, p, nk) for p in range(24)]; geoms = [Geom(t, cs, coords, nk) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(nk, g.n0))
    dm = DeviceMesh(topos, geoms, nk=nk); eng = Engine(dm)
    nEl, n2 = dm.nEl, eng.n2e
    # the state of bench.py's vertical Newton iteration: a hydrostatic column (theta = 300 K + 4 K/km) with 1e-4 relative noise, at rest
    wd = np.diff(gll_points(pn)); wj = np.outer(wd, wd).ravel()
    cell = dm.det.mean(axis=1)[:, None, None] * dm.thick.mean(axis=2).T[:, :, None] * wj[None, None, :]
    zl = np.mean([g.levs.mean(axis=1) for g in dm.geoms], axis=0)
    zm = 0.5 * (zl[:-1] + zl[1:])
    th_v = 300.0 + 0.004 * zm
    pi_v = 1004.5 - (9.80616 / 0.004) * np.log(th_v / 300.0)
    rho_v = (1.0e5 / 287.0) * (pi_v / 1004.5) ** (717.5 / 287.0) / th_v
    colv = lambda v: eng.tensor((cell * v[None, :, None]).reshape(nEl, nk * n2) * (1.0 + 1e-4 * rng.standard_normal((nEl, nk * n2))))
    vs = VertSolve(eng, 30.0)
    levs = np.zeros((nk + 1, dm.nq))
    for g in dm.geoms:
        levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    st = (eng.zeros(nEl, (nk - 1) * n2), colv(rho_v), colv(rho_v * th_v), colv(pi_v), vs.init_gz(levs))
    return "bench: p=%d, 24x24x6 x %d levels, %d columns, dt 30" % (pn, nk, nEl), eng, vs, st, 0


def box_case(rng):
    engb, dmb, levs, fld, F, _ = bench.box_column_workload(0, rng)
    nEl, n2 = dmb.nEl, engb.n2e
    nkb = fld["rho"].shape[1] // n2
    vs = VertSolve(engb, 0.5, rayleigh=0.0)
    lq = np.zeros((nkb + 1, dmb.nq))
    for g in dmb.geoms:
        lq[:, np.searchsorted(dmb.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    st = (engb.zeros(nEl, (nkb - 1) * n2), fld["rho"], fld["rt"], fld["pi"], vs.init_gz(lq))
    return "box: p=4, 32x32 periodic box x %d levels, %d columns, dt 0.5, schur3_flags 3, rayleigh 0" % (nkb, nEl), engb, vs, st, 3


def launches_per_iteration(run):
    """kernel launches of one iteration from a kernel trace of this process; None where the tracer is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile

        def count(its):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                run(its); torch.cuda.synchronize()
            return sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower()
                       and "memset" not in ev.name.lower())
        n3, n1 = count(3), count(1)
        return (n3 - n1) / 2.0 if n3 > n1 else None
    except Exception as e:                                   # noqa: BLE001
        print("launch count not available:", repr(e)[:200])
        return None


def measure(title, eng, vs, st, flags, its, reps, lines):
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    run = {r: (lambda n, f=(r == "fused"): vs.solve_schur_2(*st, maxit=n, tol=0.0, schur3_flags=flags, fused=f)) for r in ("composed", "fused")}
    outs = {r: run[r](2) for r in run}                        # warm-up of both routes: code objects, workspaces, cached blocks
    torch.cuda.synchronize()
    rel = max(float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)) for a, b in zip(outs["fused"], outs["composed"]))
    ms = {r: [] for r in run}
    for _ in range(reps):
        for r in ("composed", "fused"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run[r](its); e1.record(); torch.cuda.synchronize()
            ms[r].append(e0.elapsed_time(e1) / its)
    n = {r: launches_per_iteration(run[r]) for r in run}
    lines.append(title)
    lines.append("  fused against composed after 2 iterations: relative L2 difference of the state %.2e; last norms %s" % (rel, vs.history[-1]))
    for r in ("composed", "fused"):
        lines.append("  %-8s  ms per iteration: median %.3f  min %.3f  max %.3f  (%d batches of %d)   device activities per iteration: %s"
                     % (r, statistics.median(ms[r]), min(ms[r]), max(ms[r]), reps, its, "not counted" if n[r] is None else "%g" % n[r]))
    lines.append("  fused / composed (medians): %.3f" % (statistics.median(ms["fused"]) / statistics.median(ms["composed"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="both", choices=("bench", "box", "both"))
    ap.add_argument("--bench-orders", default="3", help="element orders of the bench mesh, comma separated (the benchmark's own is 3)")
    ap.add_argument("--its", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur2_newton.txt"))
    a = ap.parse_args()
    lines = ["VertSolve.solve_schur_2: one Newton iteration, no horizontal forcing (scripts/prof_schur2.py); device: %s"
             % (torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none")]
    cases = [("bench", lambda rng, pn=int(o): bench_case(rng, pn)) for o in a.bench_orders.split(",")] + [("box", box_case)]
    for name, case in cases:
        if a.mesh in (name, "both"):
            title, eng, vs, st, flags = case(np.random.default_rng(0))
            measure(title, eng, vs, st, flags, a.its, a.reps, lines)
            del eng, vs, st
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
