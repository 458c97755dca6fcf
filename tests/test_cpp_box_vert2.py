"""mimsem_host::VertSolve2 with the box twin's options (mimsem_amd/host/mimsem_vertsolve.hpp: theta_up, vert_mom_vort, schur3_flags = 3,
rayleigh = 0; box/VertSolve.cpp:1264-1458) against the Python loop VertSolve.solve_schur_2(theta_up=True, vert_mom_vort=...), which
tests/test_gpu_box_schur2.py holds to the numpy restatement.

CPU: tests/cpp/test_vert2_box.cpp compiles with plain g++ -std=c++17 -Wall -Werror, no HIP headers, and links against the C ABI.
GPU: the driver runs three solves of three iterations on the p = 3, 2 x 2, nk = 5 box of tests/box_schur2_case.py in a process of its own.
Both hosts call the same entries on the same inputs (the time-centred term 1/2 udwdx + 1/2 uuz_j has exact halves, so one rounding on
either side); the bar is TOL = 1e-10 relative L2 per field, the bar between the two hosts of tests/test_gpu_schur2.py, and the observed
value of every field is printed.  The callback is the stand-in uuz_j = cc velz_j on both sides (cc scales it to the norm of udwdx): the
check is when the loop calls it, on which iterate, and how the term enters F_w; AssembleVertMomVort itself is tests/test_gpu_box_schur2.py's."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
FIELDS = ("velz", "rho", "rt", "exner")
SHAPE = (3, 2, 5)


def _build(tmp):
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = os.path.join(tmp, "test_vert2_box")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_vert2_box.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_driver_compiles_and_links(tmp_path):
    assert os.path.exists(_build(str(tmp_path)))
    text = open(os.path.join(ROOT, "mimsem_amd", "host", "mimsem_vertsolve.hpp")).read()
    assert "hip/hip_runtime" not in text and "mimsem_column_diag_theta_wup" in text


@pytest.mark.gpu
def test_box_loop_driven_from_cpp(tmp_path, oracle):
    from mimsem_amd.vertsolve import VertSolve
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    from tests import box_schur2_case as bc
    from tests.test_gpu_box_schur2 import _case
    c = _case(oracle, SHAPE)
    eng, P, st, d = c["eng"], c["P"], c["st"], c["dev"]
    cc = float(np.linalg.norm(c["udwdx"]) / np.linalg.norm(st["velz"]))
    arrays = mesh_arrays(eng.mesh)
    arrays.update(dt=np.array([bc.DT]), cc=np.array([cc]), zv=st["zv"], velz=st["velz"], rho=st["rho"], rt=st["rt"], exner=st["exner"],
                  udwdx=c["udwdx"])
    fin, fout = str(tmp_path / "vert2_box_in.arr"), str(tmp_path / "vert2_box_out.bin")
    write_arrays(fin, arrays)
    out = subprocess.run([_build(str(tmp_path)), fin, fout], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "DONE" in out.stdout
    res = np.fromfile(fout, dtype=np.float64)
    pos = [0]

    def take(shape):
        n = int(np.prod(shape)); a = res[pos[0]:pos[0] + n].reshape(shape); pos[0] += n
        return a
    udwdx = eng.tensor(c["udwdx"])
    calls = []

    def uuz(velz_j):
        calls.append(velz_j.clone())
        return cc * velz_j
    runs = (dict(udwdx=udwdx, vert_mom_vort=uuz), dict(vert_mom_vort=uuz), dict(udwdx=udwdx))
    nt = (P.nEl, (P.nk + 1) * P.n2e)
    finals = []
    for run, kw in enumerate(runs):
        got = [take(st[k].shape) for k in FIELDS] + [take(nt), take(st["rho"].shape)]
        its, k2i_z = take((2,))
        hist = take((int(its), 4))
        del calls[:]
        vs = VertSolve(eng, bc.DT, rayleigh=0.0)
        py = vs.solve_schur_2(d["velz"], d["rho"], d["rt"], d["exner"], d["zv"], maxit=3, tol=0.0, schur3_flags=3, fused=True, theta_up=True, **kw)
        assert len(calls) == (3 if run == 0 else 0)
        for a, b, name in zip(got, list(py) + [vs.theta_h, vs.exner_h], FIELDS + ("theta_h", "exner_h")):
            err = rel_l2(a, b.cpu().numpy())
            print("box loop from C++, run %d, %-8s |C++ - Python| / |Python| = %.2e" % (run, name, err))
            assert np.all(np.isfinite(a)) and err < TOL, (run, name, err)
        assert int(its) == 3 == len(vs.history)
        assert abs(k2i_z - vs.k2i_z) <= 1e-9 * abs(vs.k2i_z) + 1e-300
        for hd, ho in zip(hist, vs.history):
            for j, k in enumerate(("exner", "w", "rho", "rt")):
                assert abs(hd[j] - ho[k]) <= 1e-5 * ho[k] + 1e-15, (run, k)
        finals.append(got[0])
    assert pos[0] == res.size
    # the three solves differ where they should: the centred term against the forward one, and against none at all
    d02, d12 = rel_l2(finals[0], finals[2]), rel_l2(finals[1], finals[2])
    print("velz: centred against forward term %.2e, no term against forward term %.2e" % (d02, d12))
    assert d02 > 10 * TOL and d12 > 10 * TOL
