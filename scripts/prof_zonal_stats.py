"""The zonal-mean statistics (mimsem_amd/zonalstats.py) on the 24 x 24 x 6, p = 3 sphere with a UMJS14 state after one Euler.strang step
under Held-Suarez forcing, NB = 64 latitude bands, three measurements in one process:

1. One sample by the kernel (Engine.zonal_moments: one launch) against ZonalStats.composed added to the running sums (four interp_quad
   launches, torch's element-wise kernels and index_add_), for nk = 16 (dt = 120, the Held-Suarez case) and nk = 30 (dt = 75): device
   events around batches of CALLS samples, WARMUP samples of each first, the two routes alternating, the median and min .. max of REPEATS
   batches per route; the difference of the two samples.
2. The kernel's time against its byte model: the compulsory bytes of a sample (every state array, J, det and thickInv once) and the bytes
   the design requests (per point and level 2 N velx DoFs, 3 N^2 2-form DoFs, J, det, thickInv, 2 N edge indices and the list entry).
3. nk = 16: one strang step under hs_forcing with a sample after it and with none -- a first step from the same state every time, host
   clock between device synchronisations, the median of REPEATS steps per route after one warm-up step each, the routes alternating.

The rule, stated before the measurement: ZonalStats.FUSED = True if the kernel's median (1) is not above the composed route's at both
level counts.  Writes profiles/zonal_stats.txt (or the path given)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PN, NE, NPATCH, NB = 3, 24, 24, 64
CASES = ((16, 120.0), (30, 75.0))
CALLS, WARMUP, REPEATS = 20, 3, 3
HBM = 6.3e12                     # achievable HBM rate, bytes per second


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
        lines.append("%-9s %s per call: median %9.2f   min %9.2f .. max %9.2f" % (k, unit, np.median(v), v.min(), v.max()))


def make(nk, dt):
    from mimsem_amd import heldsuarez as hs
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.euler import Euler
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(PN, NE, NPATCH); coords = sphere_coords(PN, NE)
    topos = [Topo(cs, p, nk) for p in range(NPATCH)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    for g in geoms:
        g.set_levels(hs.levels(nk, coords[g.loc0]))
    eng = Engine(DeviceMesh(topos, geoms, nk=nk, numbering="global"))
    xq = coords[eng.mesh.gidq]
    lat = eng.tensor(np.ascontiguousarray(np.arcsin(xq[:, 2] / np.linalg.norm(xq, axis=1))[np.asarray(eng.mesh.indsq)]))
    eu = Euler(eng, dt, hs.levels(nk, xq), xq, hs_forcing=True, hs_lat=lat)
    return eng, eu, lat


def main(path):
    from mimsem_amd.zonalstats import ZonalStats
    lines = ["zonal-mean statistics, p = %d, %d x %d x 6 sphere, NB = %d latitude bands, UMJS14 state after one Euler.strang step under Held-Suarez forcing; %s"
             % (PN, NE, NE, NB, torch.cuda.get_device_name(0)),
             "device events around batches of %d samples, %d warm-up samples, %d batches per route, routes alternating" % (CALLS, WARMUP, REPEATS)]
    fused_ok = True
    for nk, dt in CASES:
        eng, eu, lat = make(nk, dt)
        first = eu.initial_state(cut=False)
        state = eu.strang(*first, diagnostics=False)[:5]
        stats = ZonalStats(eng, lat, NB)
        velx, _, rho, rt, exner = state
        acc_f, acc_c = eng.zeros(9, nk, NB), eng.zeros(9, nk, NB)
        a = eng.zonal_moments(velx, rho, rt, exner, eng.zeros(9, nk, NB)).clone()
        b, scale = stats.composed(state), stats.composed(state, absolute=True)
        full = scale > 0
        diff = float(((a - b).abs()[full] / scale[full]).max())
        routes = {"fused": lambda: eng.zonal_moments(velx, rho, rt, exner, acc_f), "composed": lambda: acc_c.add_(stats.composed(state))}
        ms = batches(routes, CALLS)
        lines += ["", "1. nk = %d (%d elements, %d points a level, %d of %d bands hold points): one sample, kernel against composed"
                  % (nk, eng.nEl, eng.nEl * eng.mp12, int(full[0, 0].sum()), NB),
                  "kernel vs composed sample, max |difference| / S_abs over the entries: %.2e" % diff]
        report(lines, ms)
        mf, mc = float(np.median(ms["fused"])), float(np.median(ms["composed"]))
        lines.append("composed / fused (medians): %.2f" % (mc / mf))
        fused_ok = fused_ok and mf <= mc
        n = eng.mesh.n
        pts = eng.nEl * eng.mp12
        compulsory = 8.0 * (nk * (eng.sizes[1] + 3 * eng.sizes[2]) + 5 * pts + nk * pts)
        requested = nk * pts * (8.0 * (2 * n + 3 * n * n + 6) + 4.0 * (2 * n + 1))
        lines += ["2. byte model over the kernel's median (not a bandwidth measurement): compulsory %.1f MB a sample = %.1f us at %.1f TB/s, %.0f %% of it reached;"
                  % (compulsory / 1e6, compulsory / HBM * 1e6, HBM / 1e12, 100.0 * compulsory / HBM / (mf * 1e-3)),
                  "   requested by the design %.0f MB (%.0f bytes per point and level): %.1f TB/s through the vector L1"
                  % (requested / 1e6, requested / nk / pts, requested / (mf * 1e-3) / 1e12)]
        if nk != CASES[0][0]:
            continue

        def step(sample):
            def call():
                eu.first_step, eu.u_prev, eu.u_curr, eu.uz, eu.uz_prev = True, None, None, None, None      # every step the same first step
                new = eu.strang(*first, diagnostics=False)[:5]
                if sample:
                    stats.sample(new)
                return new
            return call
        steps = {"sampled": step(True), "plain": step(False)}
        r0 = eu.redone
        for fn in steps.values():
            fn()
        ms_s = {k: [] for k in steps}
        for _ in range(REPEATS):
            for k, fn in steps.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(); ms_s[k].append((time.perf_counter() - t0) * 1e3)
        lines += ["3. nk = %d: one strang step under hs_forcing (a first step from the same state every time, no diagnostics), a sample after it or none;"
                  % nk, "   host clock between device synchronisations, %d steps per route after one warm-up step each, routes alternating" % REPEATS]
        report(lines, ms_s, unit="ms")
        lines.append("sampled - plain (medians): %.3f ms; steps redone after a missed check: %d"
                     % (float(np.median(ms_s["sampled"]) - np.median(ms_s["plain"])), eu.redone - r0))
        del steps
    lines += ["", "ZonalStats.FUSED: the kernel's median is %s the composed route's at both level counts -> %s"
              % ("not above" if fused_ok else "ABOVE", fused_ok)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "zonal_stats.txt"))
