#!/usr/bin/env python3
"""The box twin's theta diagnosis and Newton iteration on the config-5 grid (p = 4, 32 x 32 periodic box x 64 levels; the column workload of
bench.py), timed with device events, the two sides of each comparison ALTERNATELY in batches, medians with min and max:
  1. Engine.diag_theta_wup (mimsem_column_diag_theta_wup: block-tridiagonal, one column per 16-lane row) beside Engine.diag_theta_blend
     (mimsem_column_diag_theta_blend: block diagonal, one interface per row) on the same fields, both with the half-time blend;
  2. the FIRST Newton iteration of VertSolve.solve_schur_2 (maxit = 1 calls, each with its initial theta diagnosis) with theta_up=True beside
     theta_up=False (fused route, schur3_flags = 3, rayleigh = 0, no horizontal forcing, no vert_mom_vort: the column half alone).  Only the
     first: the benchmark's box state is not in balance, its first iteration takes |dtw w_j| to ~ 5 -- outside the condition of use of
     diag_theta_wup -- and later iterations of the box mode are not finite on it (the eul mode converges);
  3. the byte model of the new kernel over its time.
The vertical velocity is seeded with |dtw velz| <= 0.05 per dof (the entry's condition of use), dt = 0.01.
  usage: prof_box_schur2.py [--its 4] [--reps 9] [--out profiles/box_schur2.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from prof_schur2 import box_case  # noqa: E402
from mimsem_amd.vertsolve import VertSolve  # noqa: E402

DT = 0.01


def alternate(sides, reps, per):
    """sides: {name: callable running `per` units}; -> {name: [ms per unit]}"""
    for f in sides.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, f in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / per)
    return ms


def line(name, v, reps, per):
    return "  %-28s ms: median %.4f  min %.4f  max %.4f  (%d batches of %d)" % (name, statistics.median(v), min(v), max(v), reps, per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--its", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_schur2.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    rng = np.random.default_rng(0)
    title, eng, _, st, flags = box_case(rng)
    vs = VertSolve(eng, DT, rayleigh=0.0)
    velz0, rho, rt, exner, zv = st
    nEl, nk, n2 = eng.nEl, eng.nk, eng.n2e
    dtw = 0.25 * DT
    velz = eng.tensor((0.05 / dtw) * rng.uniform(-1.0, 1.0, tuple(velz0.shape)))
    lines = ["box twin: theta diagnosis and Newton iteration (scripts/prof_box_schur2.py); device: %s" % torch.cuda.get_device_name(0),
             title.replace("dt 0.5", "dt %g" % DT)]
    # 1. the two diagnoses
    blend = eng.diag_theta(1, rho, rt)
    per = 20
    sides = {"diag_theta_wup": lambda: [eng.diag_theta_wup(dtw, rho, rt, velz, blend2=blend, wa=0.5, wb=0.5) for _ in range(per)],
             "diag_theta_blend (theta2)": lambda: [eng.diag_theta_blend(rho, rt, blend2=blend, wa=0.5, wb=0.5, wantL=False) for _ in range(per)]}
    ms = alternate(sides, a.reps, per)
    up = eng.diag_theta_wup(dtw, rho, rt, velz)
    lines.append("theta on the %d interfaces of %d columns, blended; upwinded against lumped: relative L2 difference %.2e, all finite: %s"
                 % (nk + 1, nEl, float(torch.linalg.vector_norm(up - blend) / torch.linalg.vector_norm(blend)), bool(torch.isfinite(up).all())))
    for k in sides:
        lines.append(line(k, ms[k], a.reps, per))
    t_up = statistics.median(ms["diag_theta_wup"])
    lines.append("  wup / blend (medians): %.2f" % (t_up / statistics.median(ms["diag_theta_blend (theta2)"])))
    # 3. byte model: fields in and out once, the factors G and the forward vector y written and read back once
    nn = n2 * n2
    doubles = nEl * (2 * nk * n2 + (nk - 1) * n2 + 2 * (nk + 1) * n2 + 2 * nk * nn + 2 * (nk + 1) * n2)
    lines.append("  byte model of k_diag_theta_wup: %.1f MB (of which the factors G, written and read: %.1f MB) -> %.0f GB/s at the median"
                 % (8e-6 * doubles, 8e-6 * nEl * 2 * nk * nn, 8e-9 * doubles / (1e-3 * t_up)))
    # 2. one Newton iteration, box mode beside eul mode
    one = lambda up: vs.solve_schur_2(velz, rho, rt, exner, zv, maxit=1, tol=0.0, schur3_flags=flags, fused=True, theta_up=up)
    run = {m: (lambda up=(m == "theta_up=True"): [one(up) for _ in range(a.its)][-1]) for m in ("theta_up=True", "theta_up=False")}
    ms = alternate(run, a.reps, a.its)
    out = run["theta_up=True"]()
    lines.append("first Newton iteration with its initial theta diagnosis (fused route), norms of the box mode %s, state finite: %s"
                 % (vs.history[-1], all(bool(torch.isfinite(x).all()) for x in out)))
    for k in run:
        lines.append(line(k, ms[k], a.reps, a.its))
    lines.append("  box / eul (medians): %.3f" % (statistics.median(ms["theta_up=True"]) / statistics.median(ms["theta_up=False"])))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
