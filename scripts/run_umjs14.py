#!/usr/bin/env python3
"""The baroclinic-wave run of eul/UMJS14.cpp:269-353 on one GPU: the cubed sphere and the stretched levels, Euler.initial_state (or Euler.load
of dump index --start-step, the restart branch) and Euler.run.

  python scripts/run_umjs14.py --pn 3 --ne 24 --nk 30 --dt 75 --nsteps 20 --dump-every 10 --start-step 0 --outdir output
  (--integrator strang: Euler.strang in place of Euler.strang_ec; --hs-forcing: the Held-Suarez forcing on the same initial state)

--case held-suarez is the run of eul/HeldSuarez.cpp:269-355 (mimsem_amd/heldsuarez.py): nk 16, dt 120, Euler.strang, Held-Suarez forcing, the
wind perturbation not cut beyond D0, a dump every 1 440 steps unless --dump-every says otherwise:

  python scripts/run_umjs14.py --case held-suarez --nsteps 72000 --zonal-stats 64 --stats-from 14400

--zonal-stats NB samples the zonal-mean statistics (mimsem_amd/zonalstats.py) in NB latitude bands on the device, from step --stats-from
(default 1) every --stats-every steps (default 1); outdir/zonal_stats.npz is written at every dump and at the end, and a run restarted with
--start-step > 0 reads it back when it is there and continues the sums.

Prints per step the Newton iterations of the vertical solve with their last norms, the steps redone so far and the energetics line; at the end
steps per second (host clock between device synchronisations around every step, the first step left out as warm-up: it finds the solvers' fixed
lengths), the time of a dump, the fixed lengths the solvers settled on and the relative drift of mass and of total energy
(keh + kev + pe + ie) from the first line to the last.  --profile PATH writes that summary to a file as well.

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
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pn", type=int, default=3)
    ap.add_argument("--ne", type=int, default=24)
    ap.add_argument("--case", choices=("umjs14", "held-suarez"), default="umjs14",
                    help="held-suarez: eul/HeldSuarez.cpp -- nk 16, dt 120, --integrator strang, --hs-forcing, uncut perturbation, --dump-every 1440")
    ap.add_argument("--nk", type=int, default=None, help="levels (default: 30, held-suarez: 16)")
    ap.add_argument("--dt", type=float, default=None, help="time step in seconds (default: 75, held-suarez: 120)")
    ap.add_argument("--nsteps", type=int, default=20)
    ap.add_argument("--dump-every", type=int, default=None, help="steps between dumps (default: 0, none; held-suarez: 1440)")
    ap.add_argument("--zonal-stats", type=int, default=0, metavar="NB", help="sample zonal-mean statistics in NB latitude bands (ZonalStats)")
    ap.add_argument("--stats-from", type=int, default=1, metavar="STEP", help="first step that is sampled")
    ap.add_argument("--stats-every", type=int, default=1, metavar="N", help="sample every N-th step")
    ap.add_argument("--start-step", type=int, default=0)
    ap.add_argument("--outdir", default="output")
    ap.add_argument("--vp", type=float, default=None, help="amplitude of the wind perturbation (default: umjs14.VP; 0: the steady state)")
    ap.add_argument("--newton-maxit", type=int, default=20)
    ap.add_argument("--integrator", choices=("strang_ec", "strang"), default=None,
                    help="Euler.strang_ec (eul/UMJS14.cpp) or Euler.strang (the integrator of eul/HeldSuarez.cpp)")
    ap.add_argument("--hs-forcing", action="store_true", help="Held-Suarez friction and temperature forcing (Euler's hs_forcing)")
    ap.add_argument("--patches", type=int, default=0, help="patches of the mesh (default: 24 for an even ne >= 8, else 6)")
    ap.add_argument("--profile", default=None, help="write the summary to this file as well")
    ap.add_argument("--write-case", default=None, metavar="PATH",
                    help="write the initial state as a case for the C++ host (mimsem_amd/host/euler_call.cpp, workloads.write_euler_case) and stop")
    ap.add_argument("--time-limit", type=float, default=1200.0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    hs = a.case == "held-suarez"
    if hs:
        from mimsem_amd import heldsuarez as case
        a.hs_forcing = True
    defaults = dict(nk=case.NK, dt=case.DT, dump_every=case.DUMP_EVERY, integrator=case.INTEGRATOR) if hs \
        else dict(nk=30, dt=75.0, dump_every=0, integrator="strang_ec")
    for name, value in defaults.items():                 # what the command line left open
        if getattr(a, name) is None:
            setattr(a, name, value)
    return a


def work(a):
    import numpy as np
    import torch
    from mimsem_amd import umjs14 as um
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import FIELDS
    from mimsem_amd.euler import Euler
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    if not torch.cuda.is_available():
        raise SystemExit("run_umjs14: no GPU (the step has no CPU path)")
    if a.start_step and not a.dump_every:
        raise SystemExit("run_umjs14: --start-step counts dumps and needs --dump-every")
    if a.zonal_stats < 0 or a.stats_every < 1:
        raise SystemExit("run_umjs14: --zonal-stats takes a number of bands, --stats-every a positive step count")
    hs = a.case == "held-suarez"
    npatch = a.patches or (24 if a.ne >= 8 and a.ne % 2 == 0 else 6)
    t0 = time.perf_counter()
    cs = CubedSphere(a.pn, a.ne, npatch); coords = sphere_coords(a.pn, a.ne)
    topos = [Topo(cs, p, a.nk) for p in range(npatch)]
    geoms = [Geom(t, cs, coords, a.nk) for t in topos]
    for g in geoms:
        g.set_levels(um.levels(a.nk, coords[g.loc0]))
    eng = Engine(DeviceMesh(topos, geoms, nk=a.nk, numbering="global"))
    xq = coords[eng.mesh.gidq]
    hs_lat = None
    if a.hs_forcing or a.zonal_stats:                    # latitude of the quadrature points [nEl, mp12]
        hs_lat = eng.tensor(np.ascontiguousarray(np.arcsin(xq[:, 2] / np.linalg.norm(xq, axis=1))[np.asarray(eng.mesh.indsq)]))
    eu = Euler(eng, a.dt, um.levels(a.nk, xq), xq, newton_maxit=a.newton_maxit, hs_forcing=a.hs_forcing, hs_lat=hs_lat if a.hs_forcing else None)
    head = ("Held-Suarez case" if hs else "UMJS14 baroclinic wave") + ", p = %d, %d x %d x 6 sphere (%d elements), %d levels, dt = %g s, Euler.%s%s; %s" \
        % (a.pn, a.ne, a.ne, eng.nEl, a.nk, a.dt, a.integrator, ", Held-Suarez forcing" if a.hs_forcing else "", torch.cuda.get_device_name(0))
    print(head, flush=True)
    state = eu.load(a.start_step, a.outdir) if a.start_step else eu.initial_state(um.VP if a.vp is None else a.vp, cut=not hs)
    torch.cuda.synchronize()
    t_init = time.perf_counter() - t0
    print("mesh, engine and %s: %.1f s (init1 solves redone: %d)" % ("restart" if a.start_step else "initial state", t_init, eu.init1_redone), flush=True)

    if a.write_case:
        from mimsem_amd.workloads import write_euler_case
        write_euler_case(a.write_case, eng.mesh, um.levels(a.nk, xq), xq, state, a.dt, a.nsteps, hs_lat=hs_lat, newton_maxit=a.newton_maxit, eng=eng)
        print("case for the C++ host written to %s" % a.write_case, flush=True)
        return 0

    ms, dump_ms, newton, lines = [], [], [], []

    def timed(name, sink):
        inner = getattr(eu, name)

        def wrapped(*args, **kw):
            torch.cuda.synchronize(); t = time.perf_counter()
            out = inner(*args, **kw)
            torch.cuda.synchronize(); sink.append((time.perf_counter() - t) * 1e3)
            return out
        setattr(eu, name, wrapped)
    timed(a.integrator, ms); timed("dump", dump_ms)

    def on_step(step, values):
        h = eu.vert.history
        newton.append(len(h)); lines.append(values)
        print("step %d (day %.4f): Newton iterations %d, last |d_exner|/|exner| %.3e |d_rho|/|rho| %.3e, steps redone %d, %.1f ms"
              % (step, step * a.dt / 86400.0, len(h), h[-1]["exner"], h[-1]["rho"], eu.redone, ms[-1]))
        if len(h) >= a.newton_maxit:
            print("  no convergence in %d iterations; norms per iteration:" % len(h))
            for i, n in enumerate(h):
                print("    %2d  %s" % (i + 1, "  ".join("%s %.3e" % kv for kv in n.items())))
        print("  " + "\t".join("%s %.16g" % kv for kv in zip(FIELDS, values)), flush=True)
    stats, stats_path, sample_ms = None, os.path.join(a.outdir, "zonal_stats.npz"), []
    on_state = None
    if a.zonal_stats:
        from mimsem_amd.zonalstats import ZonalStats
        stats = ZonalStats(eng, hs_lat, a.zonal_stats)
        if a.start_step and os.path.exists(stats_path):
            stats.load(stats_path)
            print("zonal statistics: %d samples read back from %s" % (stats.count, stats_path), flush=True)

        def on_state(step, new):
            if step >= a.stats_from and (step - a.stats_from) % a.stats_every == 0:
                torch.cuda.synchronize(); t = time.perf_counter()
                stats.sample(new)
                torch.cuda.synchronize(); sample_ms.append((time.perf_counter() - t) * 1e3)
            if a.dump_every and step % a.dump_every == 0:
                stats.save(stats_path)
    state = eu.run(state, a.nsteps, dump_every=a.dump_every, outdir=a.outdir, start_step=a.start_step, on_step=on_step, integrator=a.integrator,
                   on_state=on_state)
    if stats is not None:
        os.makedirs(a.outdir, exist_ok=True)
        stats.save(stats_path)
    finite = all(bool(torch.isfinite(x).all()) for x in state)

    out = [head, ""]
    if len(ms) > 1:
        rest = np.array(ms[1:])
        out.append("steps per second: %.2f  (%.1f ms per step: mean of %d steps after one warm-up step of %.1f ms; median %.1f, min %.1f, max %.1f)"
                   % (1e3 / rest.mean(), rest.mean(), rest.size, ms[0], np.median(rest), rest.min(), rest.max()))
    if newton:
        out.append("Newton iterations per step (maxit %d, tol %.0e): %s" % (a.newton_maxit, eu.newton_tol, " ".join(str(n) for n in newton)))
    out.append("steps redone after a missed check: %d of %d; init1 solves redone: %d; state finite: %s" % (eu.redone, eu.steps, eu.init1_redone, finite))
    m1, vd = eu.horiz.m1, eu.vort
    cal = getattr(m1, "cheb_calibration", None)
    out.append("1-form mass solver: %s; solves checked %d, missed %d, worst check %.2e"
               % ("fixed-length Chebyshev, %d steps (bound %d)" % (cal["steps"], cal["bound_steps"]) if m1.chebyshev and cal else "adaptive PCG",
                  m1.solves_checked, m1.solves_missed, m1.worst_check))
    out.append("density-weighted solves (HorizPotVort, diagVertVort): fixed PCG lengths %s (0: adaptive), checks missed %d" % (dict(vd._its), vd.missed))
    if stats is not None:
        out.append("zonal statistics: %d bands, %d samples in %s (%d taken in this run%s)"
                   % (stats.nbands, stats.count, stats_path, len(sample_ms),
                      ", %.3f ms per sample: median of the host clock around each, first %.3f" % (np.median(sample_ms), sample_ms[0]) if sample_ms else ""))
    if dump_ms:
        out.append("one dump (.vec of six fields, .npy of eight on the quadrature grid): %s ms" % " ".join("%.0f" % v for v in dump_ms))
    if len(lines) > 1:
        tot = lambda v: sum(v[FIELDS.index(n)] for n in ("keh", "kev", "pe", "ie"))
        im = FIELDS.index("mass")
        out.append("relative drift over %d steps (line 1 to line %d): mass %.3e, total energy %.3e"
                   % (len(lines) - 1, len(lines), (lines[-1][im] - lines[0][im]) / lines[0][im], (tot(lines[-1]) - tot(lines[0])) / tot(lines[0])))
        out.append("max |velz| of the final state: %.3e" % float(state[1].abs().max()))
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
        print("run_umjs14: the run did not end within %g s and was stopped" % a.time_limit, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
