"""Times of the horizontal momentum update's friction pieces on the bench mesh: p = 3, 24 x 24 x 6 elements, 30 levels.
 (a) apply_fric (MIMSEM_OP_UMAT_FRIC, one element pass) against the pair it replaces: the Umat apply followed by the accumulating Umat_ray
     apply, alternated in the same process; and the largest relative difference of the two results
 (b) MassSolver.solve_fric (mimsem_fric_chebyshev_solve) at tau = 2 dt against the plain mimsem_block_chebyshev_solve of the same b, both
     through the class (check norms included), alternated
 (c) the step counts of the two solves, and of solve_fric at tau = 1/K_F
HIP events around REPS repetitions after a warm-up; SAMPLES samples of each, reported as median and [min, max] (the run-to-run spread inside
this process).  Output on stdout (profiles/hmomentum.txt keeps a run)."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mimsem_amd._lib import FLAG_ACCUM
from mimsem_amd.device import DeviceMesh, Engine
from mimsem_amd.geom import Geom, gll_points
from mimsem_amd.horizsolve import SCALE
from mimsem_amd.krylov import K_F, MassSolver
from mimsem_amd.mesh import CubedSphere, sphere_coords
from mimsem_amd.topo import Topo
from mimsem_amd.workloads import z_levels

PN, NE, NK = 3, int(os.environ.get("NE", "24")), int(os.environ.get("NK", "30"))
REPS, SAMPLES = int(os.environ.get("REPS", "50")), int(os.environ.get("SAMPLES", "7"))
DT = 120.0
NP = 24 if NE % 2 == 0 and NE >= 4 else 6
cs = CubedSphere(PN, NE, NP); coords = sphere_coords(PN, NE)
topos = [Topo(cs, p, NK) for p in range(NP)]
geoms = [Geom(t, cs, coords, NK) for t in topos]
for g in geoms:
    g.set_levels(z_levels(NK, g.n0, rng=np.random.default_rng(5)))
dm = DeviceMesh(topos, geoms, nk=NK, numbering="global")
eng = Engine(dm)
rng = np.random.default_rng(1)
# exner rows whose point values (after /det * thickInv) are cp sigma^(R/cp): sigma falls from 1 at level 0 to 0.3 at the top, with a
# per-element spread, so that the lowest levels carry friction (sigma > 0.7) and the upper ones take the k_v = 0 branch
n2e = PN * PN
dx = np.diff(gll_points(PN))                                            # integral of 1 over each face of the reference element
cell = np.outer(dx, dx).reshape(-1)
ex = np.zeros((NK, dm.nEl, n2e))
for k in range(NK):
    sig = (1.0 - 0.7 * k / max(NK - 1, 1)) * rng.uniform(0.97, 1.03, dm.nEl)
    scale_e = dm.det.mean(axis=1) / dm.thickInv[k].mean(axis=1)
    ex[k] = (1004.5 * sig ** (287.0 / 1004.5) * scale_e)[:, None] * cell[None, :]
exner = eng.tensor(ex.reshape(NK, dm.n2)); exner_s = exner[0].contiguous()
x = eng.tensor(rng.standard_normal((NK, dm.n1)))
y = eng.zeros(NK, dm.n1); y2 = eng.zeros(NK, dm.n1)


def timed(fns, reps=REPS):
    """ms per call of each fn: SAMPLES samples of `reps` calls between two events, the fns alternated sample by sample, after a warm-up"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    v = [[] for _ in fns]
    for _ in range(SAMPLES):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); e1.synchronize()
            v[i].append(e0.elapsed_time(e1) / reps)
    return [(float(np.median(s)), min(s), max(s)) for s in v]


def row(name, t):
    print("%-58s median %8.4f ms  [%8.4f, %8.4f]" % ((name,) + t))


print("mesh: p = %d, %d elements, %d levels; %d samples of %d calls" % (PN, eng.nEl, NK, SAMPLES, REPS))
tau = 2.0 * DT


def pair():
    eng.apply("UMAT", x, lev0=0, scale=SCALE, flags=1, out=y2)
    eng.apply_ray(x, exner, exner_s, tau, lev0=0, scale=SCALE, flags=FLAG_ACCUM, out=y2)


fric = lambda: eng.apply_fric(x, exner, exner_s, tau, lev0=0, scale=SCALE, out=y)
fric(); pair(); torch.cuda.synchronize()
ray = eng.apply_ray(x, exner, exner_s, tau, lev0=0, scale=SCALE)
print("levels with friction: %d of %d; |fric - pair| / |pair| = %.2e" % (int((ray.abs().amax(dim=1) > 0).sum()), NK,
                                                                          float(torch.linalg.vector_norm(y - y2) / torch.linalg.vector_norm(y2))))
ta, tp, tu = timed([fric, pair, lambda: eng.apply("UMAT", x, lev0=0, scale=SCALE, flags=1, out=y2)])
row("(a) apply_fric, one element pass", ta)
row("(a) UMAT apply + UMAT_RAY accumulate", tp)
row("(a) UMAT apply alone", tu)
print("(a) fric / pair = %.3f" % (ta[0] / tp[0]))

ms = MassSolver(eng, SCALE, True)
b = ms.apply_fric(eng.tensor(rng.standard_normal((NK, dm.n1))), tau, exner, exner_s)
out = torch.empty_like(b)
x0, n0 = ms.solve(b)                       # (Ritz bounds and the one-time calibration of the plain solve's count)
x0, n0 = ms.solve(b)
bound = ms.cheb_calibration["bound_steps"] if getattr(ms, "cheb_calibration", None) else n0
x1, n1 = ms.solve_fric(b, tau, exner, exner_s, out=out)
_, nbig = ms.solve_fric(b, 1.0 / K_F, exner, exner_s)
res = float((torch.linalg.vector_norm(b - ms.apply_fric(x1, tau, exner, exner_s), dim=1) / torch.linalg.vector_norm(b, dim=1)).max())
print("(c) steps: plain solve %d (bound-based %d), solve_fric(tau = %g) %d, solve_fric(tau = 1/K_F) %d; verify() %s; true residual of solve_fric %.2e"
      % (n0, bound, tau, n1, nbig, ms.verify(), res))
ts, tb = timed([lambda: ms.solve_fric(b, tau, exner, exner_s, out=out), lambda: ms.solve(b)], max(1, REPS // 5))
ms.verify()
row("(b) solve_fric, %d steps" % n1, ts)
row("(b) plain block_chebyshev_solve, %d steps" % n0, tb)
print("(b) per step: solve_fric %.4f ms, plain %.4f ms" % (ts[0] / n1, tb[0] / n0))
