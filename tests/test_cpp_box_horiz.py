"""The box mode of mimsem_host::HorizSolve (mimsem_amd/host/mimsem_horizsolve.hpp; box/HorizSolve.cpp:214-324, :382-526), driven from C++
(tests/cpp/test_horiz2_box.cpp), against the numpy restatements of tests/box_strang_case.py on its uniform-layer p = 3, 3 x 3, nk = 4 box:
the case, the references and the bar of the Python host's test, tests/test_gpu_box_horiz.py -- relative L2 per level below
MOMENTUM_TOL = 1e-10, k2i relative to the sum of the magnitudes of its terms at the same bar, do_visc off and on, the element-local forcing
composed and fused; every observed value is printed.  The driver also checks that the _ec routines and diagnose_q throw and that a mesh
whose layers differ is refused.

CPU: the driver compiles with plain g++ -std=c++17 -Wall -Werror, no HIP headers, and links against the C ABI."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENTUM_TOL = 1e-10


def _build(tmp):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = os.path.join(tmp, "test_horiz2_box")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_horiz2_box.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_box_right_hand_sides_driven_from_cpp(tmp_path, oracle):
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    from tests import box_strang_case as bc
    from mimsem_amd.device import DeviceMesh
    from tests import strang2_case as s2c
    from tests import strang_case as sc
    from tests import vort_diag_case as vc
    from tests.test_gpu_box_horiz import ARGS, VORT
    # the fields of tests/test_gpu_box_horiz.py's case (same seed, same order of draws; why each is scaled as it is, is said there)
    c = bc.make_case(oracle)
    gd, nk = c["gd"], c["nk"]
    dm = DeviceMesh(c["topos"], c["geoms"], nk=nk, numbering="global")
    velx, velz_v, rho, rt, exner = c["state"]
    r = np.random.default_rng(23)
    F = dict(u1=velx, u2=velx * (1 + 0.05 * r.standard_normal(velx.shape)), h1=rho, h2=rho * (1 + 1e-3 * r.standard_normal(rho.shape)))
    F["Pi"] = exner * (1 + 1e-2 * r.standard_normal(exner.shape))
    F["velz1"] = sc.to_horiz(c, velz_v, nk - 1); F["velz2"] = F["velz1"] * (1 + 0.05 * r.standard_normal(F["velz1"].shape))
    F["theta_i"] = s2c.to_horiz(c, bc.theta_up(c, sc.to_vert(c, rho), sc.to_vert(c, rt), velz_v, bc.DT), nk + 1)
    F["dudz1"] = VORT * vc.horiz_pot_vort(gd, velx, rho)[0]; F["dudz2"] = F["dudz1"] * 1.1
    F["dwdx1"] = VORT * vc.vert_vort(gd, F["velz1"], rho)[0]; F["dwdx2"] = F["dwdx1"] * 0.9
    F["Fz"] = vc.vert_mass_flux(gd, F["velz1"], F["velz2"], F["h1"], F["h2"])
    c["ref"] = {}
    for visc in (False, True):
        hz = bc.BoxOracle(gd, c["lx"], do_visc=visc)
        if not visc:
            c["adv"] = bc.advection_rhs(hz, F["u1"], F["u2"], F["h1"], F["h2"], F["theta_i"])
        a = [F[n] for n in ARGS]
        full = bc.momentum_rhs_all(hz, *a, Fz=F["Fz"], dwdx1=F["dwdx1"], dwdx2=F["dwdx2"], Fk=c["adv"][2])
        c["ref"][visc] = dict(full=full[0], k2i=full[1], k2i_abs=full[2], plain=bc.momentum_rhs_all(hz, *a))
    arrays = mesh_arrays(dm)
    arrays.update({n: np.array(F[n]) for n in ARGS + ("h1", "h2", "Fz", "dwdx1", "dwdx2")})
    arrays.update(lx=np.array([c["lx"]]), thick=np.asarray(dm.thick, dtype=np.float64))
    fin, fout = str(tmp_path / "horiz2_box_in.arr"), str(tmp_path / "horiz2_box_out.bin")
    write_arrays(fin, arrays)
    out = subprocess.run([_build(str(tmp_path)), fin, fout], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "DONE" in out.stdout and "refused: HorizSolve (box): uniform layers only" in out.stdout
    res = np.fromfile(fout, dtype=np.float64)
    pos = [0]

    def take(rows, n):
        a = res[pos[0]:pos[0] + rows * n].reshape(rows, n); pos[0] += rows * n
        return a

    def levels(label, got, want):
        errs = [rel_l2(got[k], want[k]) for k in range(nk)]
        print("C++ box %-44s relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
        assert np.all(np.isfinite(got)) and max(errs) < MOMENTUM_TOL, (label, errs)
    N1, N2 = gd.N1, gd.N2
    for visc in (False, True):
        ref = c["ref"][visc]
        if not visc:
            del2 = take(1, 1)[0, 0]
            want = bc.BoxOracle(gd, c["lx"]).del2
            assert abs(del2 - want) < 1e-14 * abs(want)
            for name, n, w in zip(("dF", "dG", "Fk", "Gk"), (N2, N2, N1, N1), c["adv"]):
                levels("advection_rhs %s" % name, take(nk, n), w)
        for fused in (False, True):
            tag = "do_visc = %s, fused_forcing = %s" % (visc, fused)
            levels("momentum_rhs, " + tag, take(nk, N1), ref["full"])
            levels("plain, " + tag, take(nk, N1), ref["plain"])
            e = abs(take(1, 1)[0, 0] - ref["k2i"]) / ref["k2i_abs"]
            print("C++ box k2i, %s: |difference| / sum of magnitudes %.2e" % (tag, e))
            assert ref["k2i"] != 0.0 and e < MOMENTUM_TOL
    assert pos[0] == res.size
    assert rel_l2(c["ref"][True]["full"], c["ref"][False]["full"]) > 1e-6             # the viscosity is felt
