"""BoxEuler.entropy on the config-5 grid (p = 4, 32 x 32 elements, 64 levels: 1 024 elements, 65 interfaces) with the rising-bubble state:
the kernel (FUSED_ENTROPY = True: mimsem_euler_log_entropy, two launches) against the composed route (False: Engine.interp_quad, torch.log
and a weighted torch sum) on stage 1's theta_0 = diag_theta_wup of the initial state.  Device events around batches of CALLS evaluations,
WARMUP evaluations of each route first, the two routes alternating, the median and the spread of REPEATS batches per route; the two values
and their difference; the kernel's byte model over the call time.

Writes profiles/box_entropy.txt (or the path given)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import run_bubble as rb          # noqa: E402
from prof_box_strang import PEAK, batches, report          # noqa: E402

PN, NE, NK, DT = 4, 32, 64, 0.01
CALLS, WARMUP, REPEATS = 50, 3, 3


def main(path):
    eng, eu = rb.make_box_euler(PN, NE, NK, DT, newton_maxit=3, do_visc=False)
    velx, velz, rho, rt, exner = eu.initial_state()
    theta = eng.l2_vert_to_horiz(eng.diag_theta_wup(0.25 * DT, eng.l2_horiz_to_vert(rho), eng.l2_horiz_to_vert(rt), velz).contiguous(), NK + 1)

    def route(fused):
        def call():
            eu.FUSED_ENTROPY = fused
            return eu.entropy(theta)
        return call
    routes = {"fused": route(True), "composed": route(False)}
    a, b = float(routes["fused"]()), float(routes["composed"]())
    lines = ["BoxEuler.entropy, rising bubble, p = %d, %d x %d box, %d levels: %d elements, %d rows of theta; %s"
             % (PN, NE, NE, NK, eng.nEl, theta.shape[0], torch.cuda.get_device_name(0)), "",
             "mimsem_euler_log_entropy (2 launches) against interp_quad + torch.log + the weighted sum",
             "device events around batches of %d evaluations, %d warm-up evaluations, %d batches per route, routes alternating" % (CALLS, WARMUP, REPEATS),
             "fused % .16e   composed % .16e   |difference| / |composed| = %.2e" % (a, b, abs(a - b) / abs(b))]
    ms = batches(routes, CALLS)
    report(lines, ms)
    model = theta.numel() * 8.0 + theta.shape[0] * 8.0
    tf = float(np.median(ms["fused"])) * 1e-3
    lines.append("byte model over the call time (not a bandwidth measurement): theta and lz once, %.2f MB per call: %.2f TB/s at the median"
                 " (both launches included) = %.1f %% of 8 TB/s" % (model / 1e6, model / tf / 1e12, 100.0 * model / tf / PEAK))
    not_slower = float(np.median(ms["fused"])) <= float(np.median(ms["composed"]))
    lines += ["", "BoxEuler.FUSED_ENTROPY: the kernel's median is %s the composed route's" % ("not above" if not_slower else "ABOVE")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "box_entropy.txt"))
