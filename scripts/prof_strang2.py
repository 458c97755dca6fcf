"""Euler.strang on the bench mesh (p = 3, 24 x 24 x 6 cubed sphere, 30 levels: 3 456 elements), two measurements in one process, on the
mesh and state of scripts/prof_strang.py:

1. The mass-flux right-hand side, Engine.flux_rhs (mimsem_horiz_flux_rhs: two launches) against HorizSolve._uvec_hu4 (four accumulated
   Uhmat applies): device events around batches of CALLS calls, warm-up first, the two routes alternating batch by batch, the median and the
   spread (min .. max) of SAMPLES batches per route; the output difference; the byte model of the call (element pass 162 doubles read + 24
   written per (level, element) at p = 3, gather 24 read per unit + the n1 slots of every level written) over the call time.
2. One strang step split by stage (host clock between device synchronisations at the stage boundaries; NEWTON Newton iterations, no
   convergence test), the median of STEPS steps after one warm-up step, with the kernel launches of a step counted by the profiler of
   torch -- and the same for strang_ec from the same process.

Writes profiles/strang.txt (or the path given)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import prof_strang as ps          # noqa: E402  (the mesh, the state and the batch sizes)

PEAK = 8.0e12


def by_stage(eu, step, solve, st, steps):
    """rows [stage 1, stage 2, stage 3, diagnostics + checks, whole step] in ms of `steps` steps after one warm-up step, the state after
    them and the kernel launches of one more step"""
    marks = []

    def mark_after(obj, name):
        inner = getattr(obj, name)

        def wrapped(*a, **kw):
            out = inner(*a, **kw)
            torch.cuda.synchronize(); marks.append(time.perf_counter())
            return out
        setattr(obj, name, wrapped)
        return lambda: setattr(obj, name, inner)
    undo = [mark_after(eu.hmom, "predictor"), mark_after(eu.vert, solve), mark_after(eu.hmom, "corrector")]
    one = getattr(eu, step)
    st = one(*st)[:5]                                      # warm-up: the first step finds the solvers' fixed lengths
    rows = []
    for _ in range(steps):
        del marks[:]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = one(*st)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        st = out[:5]
        m = marks[-3:]                                    # (a redone step leaves six marks: the last three belong to the evaluation that counted)
        rows.append([m[0] - t0, m[1] - m[0], m[2] - m[1], t1 - m[2], t1 - t0])
    for u in undo:
        u()
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            one(*st)
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                       and "memset" not in e.name.lower())
    except Exception as exc:                              # the count is an extra: the timings stand without it
        launches = "not counted (%s)" % type(exc).__name__
    return np.array(rows) * 1e3, st, launches


def main(path):
    s = ps.setup("prof_strang2")
    eng, hs, nEl = s.eng, s.hs, s.nEl
    rho2 = s.rho * 1.01

    # ---- 1. the mass-flux right-hand side: fused against composed -----------------------------------------------------------------------
    routes = {"fused": lambda: eng.flux_rhs(s.velx, s.velx2, s.rho, rho2, scale=1.0e8),
              "composed": lambda: hs._uvec_hu4(s.velx, s.velx2, s.rho, rho2)}
    a, b = routes["fused"](), routes["composed"]()
    diff = float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))
    for fn in routes.values():
        for _ in range(ps.WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(ps.SAMPLES):
        for k, fn in routes.items():                      # alternating: both routes see the same drift of the machine
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(ps.CALLS):
                fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / ps.CALLS)
    lines = ["Euler.strang, p = %d, %d x %d x 6 sphere, %d levels: %d elements; %s" % (ps.PN, ps.NE, ps.NE, ps.NK, nEl, torch.cuda.get_device_name(0)),
             "",
             "1. the mass-flux right-hand side, every level: mimsem_horiz_flux_rhs (2 launches) against HorizSolve._uvec_hu4 (4 accumulated applies)",
             "device events around batches of %d calls, %d warm-up calls, %d batches per route, routes alternating" % (ps.CALLS, ps.WARMUP, ps.SAMPLES),
             "fused vs composed output, relative L2: %.2e" % diff]
    for k in routes:
        v = np.array(ms[k]) * 1e3
        lines.append("%-9s us per call: median %8.2f   min %8.2f   max %8.2f" % (k, np.median(v), v.min(), v.max()))
    lines.append("composed / fused (medians): %.2f" % float(np.median(ms["composed"]) / np.median(ms["fused"])))
    n1e = eng.mesh.n * (eng.mesh.n + 1)
    unit = (2 * 2 * n1e + 2 * eng.n2e + 6 * eng.mp12 + 2 * n1e) * 8.0             # the element pass: reads + writes of one (level, element)
    model = (unit + 2 * n1e * 8.0) * nEl * ps.NK + eng.sizes[1] * 8.0 * ps.NK      # + the gather: element-local results read, slots written
    tf = float(np.median(ms["fused"])) * 1e-3
    lines.append("byte model over the call time (not a bandwidth measurement): %.0f bytes per (level, element) in the element pass, %.2f MB per"
                 % (unit, model / 1e6))
    lines.append("call with the gather: %.2f TB/s at the median (both launches included) = %.1f %% of 8 TB/s" % (model / tf / 1e12, 100.0 * model / tf / PEAK))

    # ---- 2. one step of each integrator, by stage ----------------------------------------------------------------------------------------
    st0 = (s.velx, s.velz, s.rho, s.rt, s.exner)
    for step, solve, note in (("strang", "solve_schur_2", "FUSED_HU = %s" % s.Euler.FUSED_HU), ("strang_ec", "solve_schur_eta", "")):
        eu = s.eu
        eu.first_step, eu.u_prev, eu.u_curr, eu.uz, eu.uz_prev = True, None, None, None, None       # each integrator starts from the same state
        n0, r0 = eu.steps, eu.redone
        rows, st, launches = by_stage(eu, step, solve, st0, ps.STEPS)
        finite = all(bool(torch.isfinite(x).all()) for x in st)
        lines += ["",
                  "2%s. one %s step (dt = %g, %d Newton iterations, no convergence test, diagnostics on, FUSED_PHI = %s%s), host clock between"
                  % ("a" if step == "strang" else "b", step, ps.DT, ps.NEWTON, s.Euler.FUSED_PHI, ", " + note if note else ""),
                  "device synchronisations at the stage boundaries; median (min .. max) of %d steps after one warm-up step, ms" % ps.STEPS]
        for i, name in enumerate(("stage 1 (predictor)", "stage 2 (vertical Newton + transport)", "stage 3 (corrector)", "diagnostics + checks", "whole step")):
            lines.append("%-38s %8.2f  (%8.2f .. %8.2f)" % (name, np.median(rows[:, i]), rows[:, i].min(), rows[:, i].max()))
        lines.append("steps redone after a missed check: %d; state finite after %d steps: %s" % (eu.redone - r0, eu.steps - n0, finite))
        lines.append("kernel launches of one step: %s" % launches)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strang.txt"))
