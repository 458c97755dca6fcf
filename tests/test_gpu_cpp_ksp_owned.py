"""The reference's ksp1 call sequence with the reference's PCBJACOBI (KSP::setPCBJacobiOwned of mimsem_amd/host/mimsem_shim.hpp) compiled
with g++ against the C ABI (tests/cpp/test_ksp_owned.cpp) and run on the p = 3, 2 x 2 x 6 sphere, against the dense solve of the oracle's
assembled M1."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    exe = os.path.join(tmp, "test_ksp_owned")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "test_ksp_owned.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_ksp_owned_program_compiles(tmp_path):
    """CPU: the call sequence compiles with plain g++ against the shim and links against the C ABI"""
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_ksp1_sequence_with_owned_blocks_matches_dense_solve(tmp_path):
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    from oracle import sw_oracle
    pn, ne = 3, 2
    cs = CubedSphere(pn, ne, 6); coords = sphere_coords(pn, ne)
    topos = [Topo(cs, p, 1) for p in range(6)]
    geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
    for g in geoms:
        g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
    dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
    O = sw_oracle.SWOracle(cs, topos, geoms, coords)
    b = np.random.default_rng(21).standard_normal(O.N1)
    arrays = mesh_arrays(dm)
    arrays["b"] = b
    arrays["x_dense"] = np.linalg.solve(np.asarray(O.M1), b)
    path = os.path.join(str(tmp_path), "case.arr")
    write_arrays(path, arrays)
    out = subprocess.run([_build(str(tmp_path)), path], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "OK" in out.stdout
