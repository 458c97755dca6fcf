"""Times of the interface diagnoses (mimsem_amd/vortdiag.py) on the bench mesh: p = 3, 24 x 24 x 6 elements, 30 levels, 29 interfaces.
 (i)   one mimsem_elem_block_pc_build_levels call for UTMAT_H and for UHMAT (all 29 interfaces in one launch)
 (ii)  29 single-level mimsem_elem_block_pc_build calls for UHMAT (the form available before the batched entry)
 (iii) whole horiz_pot_vort and vert_vort calls in fixed-length mode, with their iteration counts
HIP events around REPS repetitions after a warm-up; SAMPLES samples of each, reported as median and [min, max] (the run-to-run spread
inside this process).  Output on stdout (profiles/vort_diag.txt keeps a run)."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mimsem_amd.device import DeviceMesh, Engine
from mimsem_amd.geom import Geom
from mimsem_amd.horizsolve import SCALE, HorizSolve
from mimsem_amd.mesh import CubedSphere, sphere_coords
from mimsem_amd.topo import Topo
from mimsem_amd.vortdiag import VortDiag
from mimsem_amd.workloads import z_levels

PN, NE, NK = 3, int(os.environ.get("NE", "24")), int(os.environ.get("NK", "30"))
REPS, SAMPLES = int(os.environ.get("REPS", "20")), int(os.environ.get("SAMPLES", "7"))
NP = 24 if NE % 2 == 0 and NE >= 4 else 6
cs = CubedSphere(PN, NE, NP); coords = sphere_coords(PN, NE)
topos = [Topo(cs, p, NK) for p in range(NP)]
geoms = [Geom(t, cs, coords, NK) for t in topos]
for g in geoms:
    g.set_levels(z_levels(NK, g.n0, rng=np.random.default_rng(5)))
dm = DeviceMesh(topos, geoms, nk=NK, numbering="global")
eng = Engine(dm)
rng = np.random.default_rng(1)
xq = np.zeros((dm.nq, 3))
for g in geoms:
    xq[g.loc0] = coords[g.loc0]
hs = HorizSolve(eng, quad_coords=xq[dm.gidq])
vd = VortDiag(eng, hs)
area = float(dm.det.mean()) * 4.0 / 9; dz = float(dm.thick.mean()); ln = area ** 0.5
velx = eng.tensor(rng.standard_normal((NK, dm.n1)) * 20.0 * ln * dz)
rho = eng.tensor(rng.uniform(0.8, 1.2, (NK, dm.n2)) * area * dz)
velz = eng.tensor(rng.standard_normal((NK - 1, dm.n2)) * area)
NI = NK - 1
rb = vd.rho_bar(rho)
nd = 2 * eng.n1e
out = torch.empty(NI, eng.nEl, nd, nd, dtype=torch.float64, device=eng.device)


def timed(fn, reps=REPS):
    """ms per call: SAMPLES samples of `reps` calls between two events, after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    v = []
    for _ in range(SAMPLES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); e1.synchronize()
        v.append(e0.elapsed_time(e1) / reps)
    return float(np.median(v)), min(v), max(v)


def loop_single():
    for i in range(NI):
        eng.elem_block_pc("UHMAT", f=rb[i], lev=0, scale=SCALE, out=out[i])


print("mesh: p = %d, %d elements, %d levels, %d interfaces; %d samples of %d calls" % (PN, eng.nEl, NK, NI, SAMPLES, REPS))
rows = [("(i)  build_levels UTMAT_H, one launch", lambda: eng.elem_block_pc_levels("UTMAT_H", NI, f=rb, lev0=0, lev_step=1, scale=SCALE, out=out)),
        ("(i)  build_levels UHMAT (level step 0), one launch", lambda: eng.elem_block_pc_levels("UHMAT", NI, f=rb, lev0=0, lev_step=0, scale=SCALE, out=out)),
        ("(ii) %d single-level builds UHMAT" % NI, loop_single)]
res = {}
for name, fn in rows:
    res[name] = timed(fn)
    print("%-52s median %8.4f ms  [%8.4f, %8.4f]" % ((name,) + res[name]))
(b_med, b_lo, b_hi), (s_med, s_lo, s_hi) = res[rows[1][0]], res[rows[2][0]]
print("batched / loop of single-level builds (UHMAT): %.3f   (spreads: batched %.1f %%, loop %.1f %%)" %
      (b_med / s_med, 100.0 * (b_hi - b_lo) / b_med, 100.0 * (s_hi - s_lo) / s_med))
# (iii) the first call of each solve finds its count adaptively; the timed calls run fixed-length
vd.horiz_pot_vort(velx, rho); vd.vert_vort(velz, rho)
print("adaptive first calls: iterations %s -> fixed lengths %s" % (vd.its, vd._its))
for name, fn in (("(iii) horiz_pot_vort, fixed length", lambda: vd.horiz_pot_vort(velx, rho)), ("(iii) vert_vort, fixed length", lambda: vd.vert_vort(velz, rho))):
    print("%-52s median %8.4f ms  [%8.4f, %8.4f]" % ((name,) + timed(fn, max(1, REPS // 10))))
print("fixed_its %s  check() %s" % (vd.fixed_its, vd.check()))
