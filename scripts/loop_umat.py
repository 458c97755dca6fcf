#!/usr/bin/env python3
"""The loop of profiles/umat_balance_ab.txt and profiles/umat_store_policy_ab.txt: the bench.py step (Umat apply over the 24 x 24 x 6
sphere x 30 levels) 2 000 times back to back, the host clock around one synchronise, three samples; prints us per step, the plan's
stats and a hash of y after the first call.  One library per process: MIMSEM_LIB=build_ab/libmimsem_hip_NAME.so TAG=NAME; alternate the
processes (parent, new, three times).  WARM = calls before the first sample (50).  SPLIT = levels per requested part (the default
rule otherwise; MIMSEM_WAVE_BALANCE=k selects the planned list as everywhere)."""
import ctypes as C
import hashlib
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from mimsem_amd.device import DeviceMesh, Engine
from mimsem_amd.geom import Geom
from mimsem_amd.mesh import CubedSphere, sphere_coords
from mimsem_amd.topo import Topo
from mimsem_amd.workloads import z_levels

PN, NE, NK = 3, 24, 30
cs = CubedSphere(PN, NE, 24); coords = sphere_coords(PN, NE)
topos = [Topo(cs, p, NK) for p in range(24)]
geoms = [Geom(t, cs, coords, NK) for t in topos]
for g in geoms:
    g.set_levels(z_levels(NK, g.n0))
dm = DeviceMesh(topos, geoms, nk=NK, numbering="global")
rng = np.random.default_rng(1)
eng = Engine(dm, device=0)
if os.environ.get("SPLIT"):                            # SPLIT=10: requested parts of 10 levels (mimsem_ctx_set_wave_split, the order as it is)
    assert eng.L.mimsem_ctx_set_wave_split(eng.ctx, int(os.environ["SPLIT"]), -1) == 0
x = eng.tensor(rng.standard_normal((NK, dm.n1))); y = eng.zeros(NK, dm.n1)
call, _ = eng.prepare_apply("UMAT", x, lev0=0, scale=1e8, flags=1, out=y)
call()
torch.cuda.synchronize()
sha = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()[:12]
for _ in range(int(os.environ.get("WARM", "50"))):     # WARM=2000: a whole sample's worth, so that the first sample is not the clocks' ramp
    call()
torch.cuda.synchronize()
s = []
for _ in range(3):
    t = time.perf_counter()
    for _ in range(2000):
        call()
    torch.cuda.synchronize()
    s.append((time.perf_counter() - t)/2000*1e6)
st = (C.c_int*5)()
eng.L.mimsem_op_wave_stats(eng.ctx, NK, st)
print("%-8s sha %s median %.2f (%s) us/step  stats %s" % (os.environ.get("TAG", "?"), sha, sorted(s)[1], " ".join("%.2f" % v for v in s), list(st)), flush=True)
