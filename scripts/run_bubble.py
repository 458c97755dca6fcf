#!/usr/bin/env python3
"""The rising-bubble run of box/Bubble.cpp:123-215 on one GPU: the doubly periodic box with uniform layers, BoxEuler.initial_state (or
BoxEuler.load of dump index --start-step, the restart branch) and BoxEuler.run with do_visc = False (:160-161).

  python scripts/run_bubble.py --pn 3 --ne 8 --nk 30 --dt 0.01 --nsteps 20 --dump-every 10 --start-step 0 --outdir output

Writes outdir/energetics.dat; prints per step the Newton iterations of the vertical solve with their last norms and the steps redone so far,
at the end steps per second (host clock between device synchronisations around every step, the first step left out as warm-up) and the
relative drift of mass.  --profile PATH writes that summary to a file as well.

The work runs in a child process under a time limit of its own (--time-limit seconds, default 1200; exit status 124 when it runs out): this
process never opens the GPU."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv):
    from mimsem_amd import bubble as bb
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pn", type=int, default=3)
    ap.add_argument("--ne", type=int, default=8, help="elements per side of the box")
    ap.add_argument("--nk", type=int, default=30)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--nsteps", type=int, default=20)
    ap.add_argument("--dump-every", type=int, default=0)
    ap.add_argument("--start-step", type=int, default=0)
    ap.add_argument("--outdir", default="output")
    ap.add_argument("--ztop", type=float, default=bb.ZTOP)
    ap.add_argument("--lx", type=float, default=bb.LX)
    ap.add_argument("--theta-0", type=float, default=bb.THETA_0)
    ap.add_argument("--newton-maxit", type=int, default=20)
    ap.add_argument("--fused-forcing", action="store_true", help="momentum_rhs through mimsem_horiz_momentum_forcing")
    ap.add_argument("--profile", default=None, help="write the summary to this file as well")
    ap.add_argument("--write-case", default=None, metavar="PATH",
                    help="write the initial state as a case for the C++ host (mimsem_amd/host/euler_call.cpp, workloads.write_euler_case) and stop")
    ap.add_argument("--time-limit", type=float, default=1200.0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def make_box_euler(pn, ne, nk, dt, ztop=None, lx=None, newton_maxit=20, do_visc=False, fused_forcing=None):
    """the mesh of box/Bubble.cpp:151-155 (one patch, uniform layers of ztop / nk), its engine and its BoxEuler"""
    from mimsem_amd import bubble as bb
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.euler import BoxEuler
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    ztop = bb.ZTOP if ztop is None else ztop
    lx = bb.LX if lx is None else lx
    bx = PeriodicBox(pn, ne, 1); coords = box_coords(pn, ne, lx)
    topo = Topo(bx, 0, nk)
    geom = BoxGeom(topo, bx, coords, nk, lx)
    geom.set_levels(bb.levels(nk, coords[geom.loc0], ztop))
    eng = Engine(DeviceMesh([topo], [geom], nk=nk, numbering="global"))
    xq = coords[eng.mesh.gidq]
    eu = BoxEuler(eng, dt, bb.levels(nk, xq, ztop), xq, lx=lx, newton_maxit=newton_maxit, do_visc=do_visc)
    if fused_forcing is not None:
        eu.horiz.fused_forcing = fused_forcing
    return eng, eu


def work(a):
    import numpy as np
    import torch
    from mimsem_amd.energetics import FIELDS
    if not torch.cuda.is_available():
        raise SystemExit("run_bubble: no GPU (the step has no CPU path)")
    if a.start_step and not a.dump_every:
        raise SystemExit("run_bubble: --start-step counts dumps and needs --dump-every")
    t0 = time.perf_counter()
    eng, eu = make_box_euler(a.pn, a.ne, a.nk, a.dt, a.ztop, a.lx, a.newton_maxit, do_visc=False, fused_forcing=True if a.fused_forcing else None)
    head = "rising bubble, p = %d, %d x %d box (%d elements), %d levels, dt = %g s, BoxEuler.strang, fused_forcing %s; %s" \
        % (a.pn, a.ne, a.ne, eng.nEl, a.nk, a.dt, eu.horiz.fused_forcing, torch.cuda.get_device_name(0))
    print(head, flush=True)
    state = eu.load(a.start_step, a.outdir) if a.start_step else eu.initial_state(theta_0=a.theta_0, ztop=a.ztop)
    torch.cuda.synchronize()
    print("mesh, engine and %s: %.1f s (init1 solves redone: %d)" % ("restart" if a.start_step else "initial state", time.perf_counter() - t0, eu.init1_redone),
          flush=True)
    if a.write_case:
        from mimsem_amd import bubble as bb
        from mimsem_amd.workloads import write_euler_case
        write_euler_case(a.write_case, eng.mesh, bb.levels(a.nk, eu.xq, a.ztop), None, state, a.dt, a.nsteps, newton_maxit=a.newton_maxit,
                         do_visc=False, eng=eng, box_lx=a.lx)
        print("case for the C++ host written to %s" % a.write_case, flush=True)
        return 0
    ms, newton, lines = [], [], []
    inner = eu.strang

    def timed(*args, **kw):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = inner(*args, **kw)
        torch.cuda.synchronize(); ms.append((time.perf_counter() - t) * 1e3)
        return out
    eu.strang = timed

    def on_step(step, values):
        h = eu.vert.history
        newton.append(len(h)); lines.append(values)
        print("step %d (t = %g s): Newton iterations %d, last |d_exner|/|exner| %.3e |d_rho|/|rho| %.3e, steps redone %d, %.1f ms"
              % (step, step * a.dt, len(h), h[-1]["exner"], h[-1]["rho"], eu.redone, ms[-1]))
        print("  " + "\t".join("%s %.16g" % kv for kv in zip(FIELDS, values)), flush=True)
    state = eu.run(state, a.nsteps, dump_every=a.dump_every, outdir=a.outdir, start_step=a.start_step, on_step=on_step)
    finite = all(bool(torch.isfinite(x).all()) for x in state)
    out = [head, ""]
    if len(ms) > 1:
        rest = np.array(ms[1:])
        out.append("steps per second: %.2f  (%.1f ms per step: mean of %d steps after one warm-up step of %.1f ms; median %.1f, min %.1f, max %.1f)"
                   % (1e3 / rest.mean(), rest.mean(), rest.size, ms[0], np.median(rest), rest.min(), rest.max()))
    if newton:
        out.append("Newton iterations per step (maxit %d, tol %.0e): %s" % (a.newton_maxit, eu.newton_tol, " ".join(str(n) for n in newton)))
    out.append("steps redone after a missed check: %d of %d; init1 solves redone: %d; state finite: %s" % (eu.redone, eu.steps, eu.init1_redone, finite))
    if len(lines) > 1:
        im = FIELDS.index("mass")
        out.append("relative drift of mass over %d steps: %.3e; max |velz| of the final state: %.3e"
                   % (len(lines) - 1, (lines[-1][im] - lines[0][im]) / lines[0][im], float(state[1].abs().max())))
    text = "\n".join(out) + "\n"
    print("\n" + text, end="", flush=True)
    if a.profile:
        os.makedirs(os.path.dirname(os.path.abspath(a.profile)), exist_ok=True)
        with open(a.profile, "w") as f:
            f.write(text)
    return 0 if finite else 1


def main(argv):
    a = parse(argv)
    if a.child:
        return work(a)
    try:
        return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + list(argv), timeout=a.time_limit).returncode
    except subprocess.TimeoutExpired:
        print("run_bubble: the run did not end within %g s and was stopped" % a.time_limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
