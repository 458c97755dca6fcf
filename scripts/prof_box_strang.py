"""BoxEuler.strang on the config-5 grid (p = 4, 32 x 32 elements, 64 levels: 1 024 elements) with the rising-bubble state, do_visc = False,
two measurements in one process:

1. One BoxHorizSolve.momentum_rhs evaluation with the element-local forcing composed (fused_forcing = False: a RotMat, a Uhmat and a UtQWmat
   apply with their combines) and by mimsem_horiz_momentum_forcing (True: two launches): device events around batches of CALLS evaluations,
   warm-up first, the two routes alternating, the median and the spread of REPEATS batches per route; the output difference.  And the forcing
   alone (the kernel against the composed applies on the same operands), with its byte model over the call time.
2. One whole step both ways (NEWTON Newton iterations, no convergence test, diagnostics on): host clock between device synchronisations,
   the median of REPEATS steps per route after one warm-up step each, the routes alternating, both from the same state.

Writes profiles/box_strang.txt (or the path given)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import run_bubble as rb          # noqa: E402

PN, NE, NK, DT = 4, 32, 64, 0.01
NEWTON, CALLS, WARMUP, REPEATS = 3, 10, 3, 3
SCALE = 1.0e8
PEAK = 8.0e12


def batches(routes, calls):
    """ms per call: REPEATS batches per route, alternating, after WARMUP calls of each"""
    for fn in routes.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, fn in routes.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / calls)
    return ms


def report(lines, ms, unit="us"):
    f = 1e3 if unit == "us" else 1.0
    for k, v in ms.items():
        v = np.array(v) * f
        lines.append("%-9s %s per call: median %9.2f   min %9.2f   max %9.2f" % (k, unit, np.median(v), v.min(), v.max()))
    lines.append("composed / fused (medians): %.3f" % float(np.median(ms["composed"]) / np.median(ms["fused"])))


def main(path):
    eng, eu = rb.make_box_euler(PN, NE, NK, DT, newton_maxit=NEWTON, do_visc=False)
    eu.newton_tol = 0.0
    hs, vort, nk = eu.horiz, eu.vort, NK
    state = eu.initial_state()
    velx, velz, rho, rt, exner = state
    # a bubble at rest has no velocity: one step gives every operand of momentum_rhs a field of the run's own size
    state = eu.strang(*state, diagnostics=False)[:5]
    eu.first_step, eu.u_prev, eu.u_curr, eu.uz, eu.uz_prev = True, None, None, None, None
    velx, velz, rho, rt, exner = state
    to_v, to_h = eng.l2_horiz_to_vert, lambda a, rows: eng.l2_vert_to_horiz(a.contiguous(), rows)
    velz_h = to_h(velz, nk - 1)
    theta = to_h(eng.diag_theta_wup(0.25 * DT, to_v(rho), to_v(rt), velz), nk + 1)
    uz, dwdx, Fz = vort.horiz_pot_vort(velx, rho), vort.vert_vort(velz_h, rho), vort.vert_mass_flux(velz_h, velz_h, rho, rho)
    Fk = hs.advection_rhs(velx, velx, rho, rho, theta)[2]
    vort.check(); hs.verify()

    def mom(fused):
        def call():
            hs.fused_forcing = fused
            return hs.momentum_rhs(theta, uz, uz, velz_h, velz_h, exner, velx, velx, None, None, Fz=Fz, dwdx1=dwdx, dwdx2=dwdx, Fk=Fk)
        return call
    routes = {"fused": mom(True), "composed": mom(False)}
    a, b = routes["fused"](), routes["composed"]()
    diff = float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))
    lines = ["BoxEuler.strang, rising bubble, p = %d, %d x %d box, %d levels: %d elements, dt = %g, do_visc = False; %s"
             % (PN, NE, NE, NK, eng.nEl, DT, torch.cuda.get_device_name(0)), "",
             "1a. one BoxHorizSolve.momentum_rhs evaluation (with Fz, dwdx and Fk), the element-local forcing fused against composed",
             "device events around batches of %d evaluations, %d warm-up evaluations, %d batches per route, routes alternating" % (CALLS, WARMUP, REPEATS),
             "fused vs composed output, relative L2: %.2e" % diff]
    ms_mom = batches(routes, CALLS)
    report(lines, ms_mom)

    # the forcing alone, on the operands of that evaluation
    uh = velx
    q, th_h, dPi = hs.curl(uh), hs._theta_levels(theta), hs.grad(exner)
    dz, v = hs._vorticity_operands(uz, uz, velz_h, velz_h, Fz, dwdx, dwdx)
    base = eng.incidence("E12", hs.diagnose_Phi(velx, velx, velz_h, velz_h))
    out = base.clone()

    def fused():
        out.copy_(base)
        return eng.momentum_forcing(rot=(q, uh), pgf=(th_h, dPi), vor=(dz, v), scale=SCALE, flags=2, out=out)

    def composed():
        out.copy_(base)
        hs._ap("ROTMAT", uh, f=q, flags=2, out=out)
        dp = hs._ap("UHMAT", dPi, f=th_h, flags=0)
        eng.combine(dp, 1.0, beta=1.0, c=out, out=out)
        t = eng.apply("UTQWMAT", v, f=dz, lev0=0, scale=SCALE)
        eng.combine(t, 0.5, beta=1.0, c=out[1:], out=out[1:])
        eng.combine(t, 0.5, beta=1.0, c=out[:-1], out=out[:-1])
        return out
    lines += ["", "1b. the forcing alone (the copy of the E12 Phi it accumulates onto included on both sides): mimsem_horiz_momentum_forcing (2 launches)",
              "against the ROTMAT, UHMAT and UTQWMAT applies with their three combines"]
    ms_f = batches({"fused": fused, "composed": composed}, CALLS)
    report(lines, ms_f)
    n = eng.mesh.n
    n1e, n2e, mp12 = n * (n + 1), n * n, (n + 1) ** 2
    unit = (4 * 2 * n1e + 3 * n2e + mp12 + 6 * mp12 + 2 * n1e) * 8.0
    model = (unit + 2 * n1e * 8.0) * eng.nEl * NK + 2 * eng.sizes[1] * 8.0 * NK
    tf = float(np.median(ms_f["fused"])) * 1e-3
    lines.append("byte model over the call time (not a bandwidth measurement): %.0f bytes per (level, element) in the element pass, %.2f MB per call"
                 % (unit, model / 1e6))
    lines.append("with the accumulating gather: %.2f TB/s at the median (both launches and the copy included) = %.1f %% of 8 TB/s"
                 % (model / tf / 1e12, 100.0 * model / tf / PEAK))

    # ---- 2. the whole step ------------------------------------------------------------------------------------------------------------------
    def step(fused):
        def call():
            hs.fused_forcing = fused
            eu.first_step, eu.u_prev, eu.u_curr, eu.uz, eu.uz_prev = True, None, None, None, None      # every step the same first step
            return eu.strang(*state)
        return call
    steps = {"fused": step(True), "composed": step(False)}
    r0 = eu.redone
    for fn in steps.values():
        fn()
    ms_s = {k: [] for k in steps}
    for _ in range(REPEATS):
        for k, fn in steps.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out5 = fn()
            torch.cuda.synchronize(); ms_s[k].append((time.perf_counter() - t0) * 1e3)
    finite = all(bool(torch.isfinite(x).all()) for x in out5[:5])
    lines += ["", "2. one whole step (a first step from the same state every time, %d Newton iterations, no convergence test, diagnostics on), host clock"
              % NEWTON, "between device synchronisations; %d steps per route after one warm-up step each, routes alternating" % REPEATS]
    report(lines, ms_s, unit="ms")
    lines.append("steps redone after a missed check: %d; state finite: %s" % (eu.redone - r0, finite))
    faster = float(np.median(ms_mom["fused"])) < float(np.median(ms_mom["composed"]))
    lines += ["", "BoxEuler.FUSED_FORCING: the fused evaluation (1a) is %s than the composed one at the medians" % ("faster" if faster else "NOT faster")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "box_strang.txt"))
