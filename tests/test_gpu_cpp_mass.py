"""The pieces the C++ hosts share (mimsem_amd/host/mimsem_mass.hpp: FixedMassSolve, CheckLog, cheb::accepted) on their own, driven by
tests/cpp/test_mass.cpp on the smallest spheres (ne = 2) that take each path: the SWEqn / ThermalSW flavour (one level, unit thickness), the
HorizSolve flavour (three levels of non-uniform thickness, MIMSEM_FLAG_VERT, scale 1e8) and order 5.  The executable asserts: whole solve
and sweep calls give the same bits in x and in both logged norms, both within 1e-11 of the library's CG, the log accepts them, rejects a
four-step solve and rejects a NaN reference norm."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    out = str(tmp_path_factory.mktemp("mass") / "test_mass")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_mass.cpp"), "-o", out,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("pn,nk,scale", [(3, 1, 1.0), (3, 3, 1.0e8), (5, 1, 1.0)], ids=["sw_flavour", "horiz_flavour", "order_5"])
def test_fixed_mass_solve_and_check_log(exe, tmp_path, pn, nk, scale):
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import mesh_arrays, write_arrays, z_levels
    ne = 2
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk, signed_det=(nk == 1)) for t in topos]
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]) if nk == 1 else z_levels(nk, g.n0))
    case = str(tmp_path / "mesh.arr")
    write_arrays(case, mesh_arrays(DeviceMesh(topos, geoms, nk=nk, numbering="global")))
    out = subprocess.run([exe, case, repr(scale), "1" if nk > 1 else "0"], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK")
    if pn == 3:
        assert "whole solve and sweeps" in out.stdout              # (order 3 has the whole-solve entry)
