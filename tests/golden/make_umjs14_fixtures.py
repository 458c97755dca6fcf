#!/usr/bin/env python3
"""Generate tests/golden/umjs14_ic_nk30.npz: recorded results of the reference's own analytic functions of the baroclinic-wave case
(eul/UMJS14.cpp:24-232, NK = 30) at about 40 points, for tests/test_umjs14_cpu.py to hold mimsem_amd/umjs14.py against.

Authoring container only (the reference does not travel; the .npz does).  The generator reads lines 24-232 of the reference's
eul/UMJS14.cpp -- the macros and the functions, pure <cmath> -- into a temporary directory, compiles them with g++ behind a main of its own
that reads the points and prints every function at every level, and stores the numbers.  No reference text enters the repository: the
fixture holds the points and the recorded results only.

Points: the perturbation centre and its antipode; two points 1e-5 m and 1e-3 m north of the centre; points at 0.5, 1 - 1e-6, 1 + 1e-6 and
1.5 times D0 north of the centre (inside, either side of, and outside the disc of the perturbation); both poles; four points on the equator;
a seeded spread over the sphere.  (At the two near-centre points the guard of the reference is decided by the rounding of acos near 1 and not
by the distance itself: 1 - cos(1e-3 m / a) is 1e-20, far below 2^-53, so gc_dist returns either 0 or a * acos(1 - 2^-53) = 0.095 m.  The
fixture records what the reference returned there.)

The archive members carry a fixed timestamp (save_npz of make_step_fixtures.py): the same bits on every run.
Usage: python tests/golden/make_umjs14_fixtures.py [reference root, default /root/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

FIRST, LAST, NK = 24, 232, 30
RAD_EARTH = 6371220.0
INTERFACE = ("z_at_level", "z_taper", "u_pert", "v_pert", "theta_init")       # ki = 0 .. NK
LAYER = ("u_init", "v_init", "rho_init", "rt_init", "exner_init")             # ki = 0 .. NK-1
POINT = ("gc_dist",)

MAIN = r"""
#include <cstdio>
#include <cmath>
#include "case.inc"
int main(int argc, char** argv) {
    int n, ii, ki;
    double x[3];
    FILE* f = fopen(argv[1], "r");
    if(!f || fscanf(f, "%d", &n) != 1) return 1;
    for(ii = 0; ii < n; ii++) {
        if(fscanf(f, "%la %la %la", &x[0], &x[1], &x[2]) != 3) return 2;
        printf("%a\n", gc_dist(x));
        for(ki = 0; ki <= NK; ki++) printf("%a %a %a %a %a\n", z_at_level(x, ki), z_taper(x, ki), u_pert(x, ki), v_pert(x, ki), theta_init(x, ki));
        for(ki = 0; ki <  NK; ki++) printf("%a %a %a %a %a\n", u_init(x, ki), v_init(x, ki), rho_init(x, ki), rt_init(x, ki), exner_init(x, ki));
    }
    fclose(f);
    return 0;
}
"""


def on_sphere(lon, lat):
    return RAD_EARTH * np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])


def points():
    lam_c, phi_c, d0 = np.pi / 9.0, 2.0 * np.pi / 9.0, RAD_EARTH / 6.0
    centre = on_sphere(lam_c, phi_c)
    pts = [centre, -centre]
    pts += [on_sphere(lam_c, phi_c + d / RAD_EARTH) for d in (1.0e-5, 1.0e-3)]
    pts += [on_sphere(lam_c, phi_c + f * d0 / RAD_EARTH) for f in (0.5, 1.0 - 1.0e-6, 1.0 + 1.0e-6, 1.5)]
    pts += [np.array([0.0, 0.0, RAD_EARTH]), np.array([0.0, 0.0, -RAD_EARTH])]
    pts += [on_sphere(l, 0.0) for l in (0.0, 0.5 * np.pi, np.pi, -0.5 * np.pi)]
    r = np.random.default_rng(2014)
    v = r.standard_normal((26, 3))
    pts += list(RAD_EARTH * v / np.linalg.norm(v, axis=1)[:, None])
    return np.array(pts)


def main(ref):
    from make_step_fixtures import save_npz
    src = os.path.join(ref, "eul", "UMJS14.cpp")
    x = points()
    with tempfile.TemporaryDirectory() as tmp:
        with open(src) as f:
            text = f.readlines()[FIRST - 1:LAST]
        with open(os.path.join(tmp, "case.inc"), "w") as f:
            f.writelines(text)
        with open(os.path.join(tmp, "main.cpp"), "w") as f:
            f.write(MAIN)
        with open(os.path.join(tmp, "points.txt"), "w") as f:
            f.write("%d\n" % len(x))
            for p in x:
                f.write(" ".join(float(c).hex() for c in p) + "\n")
        exe = os.path.join(tmp, "case")
        subprocess.run(["g++", "-O0", "-ffp-contract=off", "-o", exe, os.path.join(tmp, "main.cpp"), "-lm"], check=True, cwd=tmp)
        out = subprocess.run([exe, os.path.join(tmp, "points.txt")], check=True, capture_output=True, text=True).stdout
    vals = iter(out.split())
    nxt = lambda: float.fromhex(next(vals))
    rec = {n: np.zeros((NK + 1, len(x))) for n in INTERFACE}
    rec.update({n: np.zeros((NK, len(x))) for n in LAYER})
    rec["gc_dist"] = np.zeros(len(x))
    for i in range(len(x)):
        rec["gc_dist"][i] = nxt()
        for ki in range(NK + 1):
            for n in INTERFACE:
                rec[n][ki, i] = nxt()
        for ki in range(NK):
            for n in LAYER:
                rec[n][ki, i] = nxt()
    path = os.path.join(HERE, "umjs14_ic_nk%d.npz" % NK)
    save_npz(path, x=x, nk=np.array(NK), **rec)
    print("%s: %d points, %d bytes; NaN in the reference's results: %s" % (path, len(x), os.path.getsize(path),
          {n: int(np.isnan(a).sum()) for n, a in rec.items() if np.isnan(a).any()}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
