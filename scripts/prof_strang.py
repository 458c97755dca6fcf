"""Euler.strang_ec on the bench mesh (p = 3, 24 x 24 x 6 cubed sphere, 30 levels: 3 456 elements), two measurements in one process:

1. HorizSolve.diagnose_Phi, the one-launch kernel (mimsem_horiz_bernoulli, fused_phi = True) against the composed route (eight launches):
   device events around batches of CALLS calls, warm-up first, the two routes alternating batch by batch, the median and the spread
   (min .. max) of SAMPLES batches per route; the kernel's time beside its byte model (1 512 bytes per (level, element) at p = 3) as a
   fraction of 8 TB/s.  The outputs of the two routes are compared first.
2. One strang_ec step split by stage (host clock between device synchronisations at the stage boundaries; NEWTON Newton iterations,
   no convergence test), the median of STEPS steps after one warm-up step, with the number of kernel launches of a step counted by the
   profiler of torch.

State: the hydrostatic column at rest and the weak zonal-gradient wind of
tests/test_gpu_next_rows.py::test_vertical_newton_loop_with_horizontal_transport.  Writes profiles/strang_ec.txt (or the path given)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PN, NE, NPATCH, NK = 3, 24, 24, 30
WARMUP, CALLS, SAMPLES = 20, 50, 21
DT, NEWTON, STEPS = 30.0, 3, 5
BYTES_PER_UNIT, PEAK = 1512.0, 8.0e12


def setup(what="prof_strang"):
    """the bench mesh, its engine, an Euler object and the state of the measurements (see the module docstring) as a namespace"""
    import types
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.euler import Euler
    from mimsem_amd.geom import Geom, gll_points
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import z_levels
    if not torch.cuda.is_available():
        raise SystemExit("%s: no GPU (a timing needs one)" % what)
    cs = CubedSphere(PN, NE, NPATCH); coords = sphere_coords(PN, NE)
    topos = [Topo(cs, p, NK) for p in range(NPATCH)]
    geoms = [Geom(t, cs, coords, NK) for t in topos]
    for g in geoms:
        g.set_levels(z_levels(NK, g.n0))
    dm = DeviceMesh(topos, geoms, nk=NK, numbering="global")
    eng = Engine(dm)
    nEl, n2 = dm.nEl, eng.n2e
    levs = np.zeros((NK + 1, dm.nq))
    for g in geoms:
        levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
    xq = coords[dm.gidq]
    eu = Euler(eng, DT, levs, xq, newton_maxit=NEWTON, newton_tol=0.0)
    hs = eu.horiz
    # the column at rest and the weak wind
    wd = np.diff(gll_points(PN)); wj = np.outer(wd, wd).ravel()
    cell = dm.det.mean(axis=1)[:, None, None] * dm.thick.mean(axis=2).T[:, :, None] * wj[None, None, :]
    zl = np.mean([g.levs.mean(axis=1) for g in geoms], axis=0); zm = 0.5 * (zl[:-1] + zl[1:])
    th_v = 300.0 + 0.004 * zm
    pi_v = 1004.5 - (9.80616 / 0.004) * np.log(th_v / 300.0)
    rho_v = (1.0e5 / 287.0) * (pi_v / 1004.5) ** (717.5 / 287.0) / th_v
    colh = lambda v: eng.l2_vert_to_horiz(eng.tensor((cell * v[None, :, None]).reshape(nEl, NK * n2)), NK)
    rho, rt, exner = colh(rho_v), colh(rho_v * th_v), colh(pi_v)
    phi_q = torch.as_tensor(xq[:, 2] / 6371220.0, device=eng.device).repeat(NK, 1).contiguous()
    phi = eng.apply("WTQ", phi_q)
    velx = hs.grad(phi / float(phi.abs().max()) * float(rho.abs().mean()) * 1e-6)
    r = np.random.default_rng(7)
    velz = eng.tensor(1e-3 * r.standard_normal((nEl, (NK - 1) * n2)) * float(dm.det.mean()) * 4.0 / (PN * PN))
    velz_h = eng.l2_vert_to_horiz(velz, NK - 1)
    velx2 = velx * 1.05
    return types.SimpleNamespace(eng=eng, dm=dm, eu=eu, hs=hs, Euler=Euler, nEl=nEl, velx=velx, velx2=velx2, velz=velz, velz_h=velz_h,
                                 rho=rho, rt=rt, exner=exner)


def main(path):
    s = setup()
    eng, eu, hs, Euler, nEl = s.eng, s.eu, s.hs, s.Euler, s.nEl
    velx, velx2, velz, velz_h, rho, rt, exner = s.velx, s.velx2, s.velz, s.velz_h, s.rho, s.rt, s.exner
    # ---- 1. diagnose_Phi: fused against composed ------------------------------------------------------------------------------------
    def route(fused):
        def fn():
            hs.fused_phi = fused
            return hs.diagnose_Phi(velx, velx2, velz_h, velz_h)
        return fn
    routes = {"fused": route(True), "composed": route(False)}
    a, b = routes["fused"](), routes["composed"]()
    diff = float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))
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
    lines = ["Euler.strang_ec, p = %d, %d x %d x 6 sphere, %d levels: %d elements; %s" % (PN, NE, NE, NK, nEl, torch.cuda.get_device_name(0)),
             "",
             "1. HorizSolve.diagnose_Phi, every level: mimsem_horiz_bernoulli (1 launch) against the composed route (8 launches)",
             "device events around batches of %d calls, %d warm-up calls, %d batches per route, routes alternating" % (CALLS, WARMUP, SAMPLES),
             "fused vs composed output, relative L2: %.2e" % diff]
    for k in routes:
        v = np.array(ms[k]) * 1e3
        lines.append("%-9s us per call: median %8.2f   min %8.2f   max %8.2f" % (k, np.median(v), v.min(), v.max()))
    ratio = float(np.median(ms["composed"]) / np.median(ms["fused"]))
    lines.append("composed / fused (medians): %.2f" % ratio)
    model = BYTES_PER_UNIT * nEl * NK
    tf = float(np.median(ms["fused"])) * 1e-3
    lines.append("byte model %.0f bytes per (level, element) x %d = %.2f MB per call: %.2f TB/s at the median (call time, launch included) = %.1f %% of 8 TB/s"
                 % (BYTES_PER_UNIT, nEl * NK, model / 1e6, model / tf / 1e12, 100.0 * model / tf / PEAK))

    # ---- 2. one step, by stage ---------------------------------------------------------------------------------------------------------
    hs.fused_phi = Euler.FUSED_PHI
    marks = []

    def mark_after(obj, name):
        inner = getattr(obj, name)

        def wrapped(*a, **kw):
            out = inner(*a, **kw)
            torch.cuda.synchronize(); marks.append(time.perf_counter())
            return out
        setattr(obj, name, wrapped)
    mark_after(eu.hmom, "predictor"); mark_after(eu.vert, "solve_schur_eta"); mark_after(eu.hmom, "corrector")
    st = (velx, velz, rho, rt, exner)
    st = eu.strang_ec(*st)[:5]                             # warm-up: the first step finds the solvers' fixed lengths
    rows = []
    for _ in range(STEPS):
        del marks[:]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = eu.strang_ec(*st)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        st = out[:5]
        m = marks[-3:]                                    # (a redone step leaves six marks: the last three belong to the evaluation that counted)
        rows.append([m[0] - t0, m[1] - m[0], m[2] - m[1], t1 - m[2], t1 - t0])
    rows = np.array(rows) * 1e3
    finite = all(bool(torch.isfinite(x).all()) for x in st)
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            eu.strang_ec(*st)
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                       and "memset" not in e.name.lower())
    except Exception as exc:                              # the count is an extra: the timings stand without it
        launches = "not counted (%s)" % type(exc).__name__
    lines += ["",
              "2. one strang_ec step (dt = %g, %d Newton iterations, no convergence test, diagnostics on, fused_phi = %s), host clock between"
              % (DT, NEWTON, Euler.FUSED_PHI),
              "device synchronisations at the stage boundaries; median (min .. max) of %d steps after one warm-up step, ms" % STEPS]
    for i, name in enumerate(("stage 1 (predictor)", "stage 2 (vertical Newton + transport)", "stage 3 (corrector)", "diagnostics + checks", "whole step")):
        lines.append("%-38s %8.2f  (%8.2f .. %8.2f)" % (name, np.median(rows[:, i]), rows[:, i].min(), rows[:, i].max()))
    lines.append("steps redone after a missed check: %d; state finite after %d steps: %s" % (eu.redone, eu.steps, finite))
    lines.append("kernel launches of one step: %s" % launches)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strang_ec.txt"))
