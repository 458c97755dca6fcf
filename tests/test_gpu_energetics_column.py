"""The fused column energetics kernel (mimsem_euler_energetics_column, csrc/energetics.inc; Engine.energetics_column, Energetics.column with
fused = True) against the composed route it stands beside (Energetics.column_composed) and against the oracle restatement of
tests/energetics_case.py, relative to S_abs (k2p and p2k are signed and may cancel), at the project's parity bar."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import energetics_case as ec

pytestmark = pytest.mark.gpu
PARITY = 1e-10           # README "N3 parity bar", SURVEY 8(c)
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def _rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


def build(c):
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.vertsolve import VertSolve
    eng = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    c["eng"], c["en"] = eng, Energetics(eng, VertSolve(eng, 0.0))
    c["t"] = {k: eng.tensor(c[k]) for k in ("velz_v", "rho_v", "zv_v")}
    c["ref_c"] = ec.restate_column(c)
    return c


@pytest.fixture(scope="module")
def sphere(oracle):
    return build(ec.make_case())


@pytest.fixture(scope="module")
def box(oracle):
    return build(ec.make_box_case(oracle))


@pytest.fixture(scope="module")
def p1(oracle):
    return build(ec.make_box_case(oracle, pn=1, ne=2, nk=5, seed=17))


def _check_column(label, c):
    t, en = c["t"], c["en"]
    assert c["eng"].mesh.n <= en.FUSED_MAX_ORDER
    en.fused = True
    fused = en.column(t["velz_v"], t["rho_v"], t["zv_v"])
    comp = en.column_composed(t["velz_v"], t["rho_v"], t["zv_v"])
    ref = c["ref_c"]
    e_ref = {n: abs(float(g) - ref[n][0]) / ref[n][1] for n, g in zip(ec.COLUMN, fused.tolist())}
    e_cmp = {n: abs(float(g) - float(w)) / ref[n][1] for n, g, w in zip(ec.COLUMN, fused.tolist(), comp.tolist())}
    print("%s: fused column kernel / S_abs  vs restatement %s   vs composed %s" % (
        label, " ".join("%s %.2e" % (n, e_ref[n]) for n in ec.COLUMN), " ".join("%s %.2e" % (n, e_cmp[n]) for n in ec.COLUMN)))
    for n, g in zip(ec.COLUMN, fused.tolist()):
        assert np.isfinite(g) and ref[n][1] > 0, n
        assert e_ref[n] <= PARITY and e_cmp[n] <= PARITY, (n, g, ref[n], e_ref[n], e_cmp[n])
    assert torch.equal(fused, en.column(t["velz_v"], t["rho_v"], t["zv_v"]))                 # two calls: the same bits
    assert torch.equal(fused, c["eng"].energetics_column(t["velz_v"], t["rho_v"], t["zv_v"]))


# ---- 1. the column kernel against the composed route and the restatement ---------------------------------------------------------------
def test_column_kernel_p3_sphere(sphere):
    """24 columns of 16 lanes in 6 full one-wave blocks; two interfaces"""
    _check_column("p3 ne2 nk3 sphere", sphere)


def test_column_kernel_p4_box(box):
    """32 lanes per column (25 points, 16 DoFs), 9 columns in 5 blocks (the last one half empty); ONE interface: it is both the first and the last"""
    _check_column("p4 ne3 nk2 box", box)


def test_column_kernel_p1_box(p1):
    """4 lanes per column, one DoF per level, four interfaces; 4 columns fill a quarter of the one block (the sphere has no order 1)"""
    _check_column("p1 ne2 nk5 box", p1)


def test_column_kernel_replayed(sphere):
    eng, t, en = sphere["eng"], sphere["t"], sphere["en"]
    en.fused = True
    eager = en.column(t["velz_v"], t["rho_v"], t["zv_v"]).clone()
    g, out = eng.capture(lambda: en.column(t["velz_v"], t["rho_v"], t["zv_v"]))
    out.zero_()
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_column_kernel_argument_errors_write_nothing(sphere):
    eng, t = sphere["eng"], sphere["t"]
    fn = eng.L.mimsem_euler_energetics_column
    eng.energetics_column(t["velz_v"], t["rho_v"], t["zv_v"])                               # (makes the LINEAR_INV blocks)
    out = torch.full((4,), 7.0, dtype=torch.float64, device=eng.device)
    good = dict(velz=t["velz_v"].data_ptr(), rho=t["rho_v"].data_ptr(), zv=t["zv_v"].data_ptr(), inv=eng._linear_inv.data_ptr(), out=out.data_ptr())

    def call(ctx=eng.ctx, **kw):
        a = dict(good); a.update(kw)
        return fn(ctx, *[None if a[k] is None else C.c_void_p(a[k]) for k in ("velz", "rho", "zv", "inv", "out")])
    assert call(ctx=None) == ERR_ARG
    for k in good:
        assert call(**{k: None}) == ERR_ARG, k
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))                                       # nothing written
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[3]) > 0
    from mimsem_amd._lib import MimsemError
    with pytest.raises(MimsemError):
        eng.energetics_column(t["velz_v"], t["rho_v"][:, :-1], t["zv_v"])                   # a short array: caught before the C call


def test_column_kernel_needs_an_interface_and_order_at_most_4():
    """nk = 1: MIMSEM_ERR_ARG; order 5: MIMSEM_ERR_UNSUPPORTED from the entry, and Energetics.column takes the composed route"""
    from mimsem_amd._lib import MimsemError
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.vertsolve import VertSolve
    from tests.helpers import z_levels

    def engine(pn, nk):
        cs = CubedSphere(pn, 1, 6); coords = sphere_coords(pn, 1)
        topos = [Topo(cs, p, nk) for p in range(6)]
        geoms = [Geom(t, cs, coords, nk) for t in topos]
        levs = z_levels(nk, geoms[0].n0, np.random.default_rng(5))
        for g in geoms:
            g.set_levels(levs)
        return Engine(DeviceMesh(topos, geoms, nk=nk, numbering="global"))
    eng = engine(3, 1)
    buf = torch.full((64,), 7.0, dtype=torch.float64, device=eng.device)
    p = C.c_void_p(buf.data_ptr())
    assert eng.L.mimsem_euler_energetics_column(eng.ctx, p, p, p, p, p) == ERR_ARG
    eng = engine(5, 2)
    assert eng.L.mimsem_euler_energetics_column(eng.ctx, p, p, p, p, p) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.full_like(buf, 7.0))
    r = np.random.default_rng(3)
    n2 = eng.n2e
    velz, rho, zv = (eng.tensor(r.uniform(0.5, 1.5, (eng.nEl, s * n2))) for s in (1, 2, 2))
    with pytest.raises(MimsemError):
        eng.energetics_column(velz, rho, zv)
    en = Energetics(eng, VertSolve(eng, 0.0))
    en.fused = True                                                                          # order 5: the composed route all the same
    assert torch.equal(en.column(velz, rho, zv), en.column_composed(velz, rho, zv))


def test_column_kernel_blocks_walk_several_columns(oracle):
    """More columns than the grid's 2 048 blocks hold at once: p = 4 has 2 columns per block, so the 65 x 65 = 4 225 columns of this periodic box
    send blocks 0 .. 128 round the fixed-stride walk twice (the second time with a half-empty group in block 64).  No dense restatement at
    this size: the composed device route is the reference and S_abs comes from its per-column terms."""
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.energetics import Energetics
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.vertsolve import FLAG_VERT, SCALE, VertSolve
    from tests.helpers import z_levels
    pn, ne, nk = 4, 65, 2
    bx = PeriodicBox(pn, ne, 1); coords = box_coords(pn, ne, 1000.0)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, coords, nk, 1000.0)
    r = np.random.default_rng(11)
    g.set_levels(z_levels(nk, g.n0, r, ztop=1500.0))
    eng = Engine(DeviceMesh([t], [g], nk=nk, numbering="global"))
    assert eng.nEl == ne * ne and eng.nEl > 2048 * 2
    vs = VertSolve(eng, 0.0)
    en = Energetics(eng, vs)
    n2 = eng.n2e
    velz = eng.tensor(r.standard_normal((eng.nEl, (nk - 1) * n2)))
    rho, zv = (eng.tensor(r.uniform(0.8, 1.2, (eng.nEl, nk * n2))) for _ in range(2))
    got, want = eng.energetics_column(velz, rho, zv), en.column_composed(velz, rho, zv)
    assert torch.equal(got, eng.energetics_column(velz, rho, zv))
    gi = vs._mv("LINEAR_INV", vs._mv("LINEAR_RT", velz, f1=rho, flags=FLAG_VERT, rows=nk - 1), rows=nk - 1)
    col = lambda a, b: float((a * b).sum(dim=1).abs().sum()) / SCALE                        # sum over columns of |the column's term|
    s_abs = [0.5 * col(rho, vs._mv("CONLIN_W", velz, f1=velz, rows=nk)), col(gi, vs.V01(zv)), col(vs.V10(gi), zv), col(zv, rho)]
    errs = [abs(float(a) - float(b)) / s for a, b, s in zip(got.tolist(), want.tolist(), s_abs)]
    print("p4 ne65 nk2 box, fused vs composed / S_abs: %s" % "  ".join("%s %.2e" % (n, e) for n, e in zip(ec.COLUMN, errs)))
    assert all(s > 0 for s in s_abs) and max(errs) <= PARITY


def test_shim_entry_called_from_cpp(tmp_path, sphere):
    """mimsem_host::Euler::energetics_column (mimsem_amd/host/mimsem_shim.hpp) compiled with g++ and called once on the p = 3 sphere
    (tests/cpp/test_energetics_column.cpp); velz, rho and zv are distinct arrays, so a swapped argument cannot pass"""
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    from tests.test_gpu_cpp_shim import _build
    c = sphere
    arrays = mesh_arrays(c["eng"].mesh)
    arrays.update(velz=c["velz_v"], rho=c["rho_v"], zv=c["zv_v"], dims=np.array([float(c["eng"].nEl), float(c["eng"].n2e)]))
    fin, fout = str(tmp_path / "en_in.arr"), str(tmp_path / "en_out.bin")
    write_arrays(fin, arrays)
    out = subprocess.run([_build(str(tmp_path), "test_energetics_column"), fin, fout], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "DONE" in out.stdout
    got = np.fromfile(fout, dtype=np.float64)
    assert got.shape == (4,)
    ref = c["ref_c"]
    for n, v in zip(ec.COLUMN, got):
        assert abs(v - ref[n][0]) / ref[n][1] <= PARITY, (n, v, ref[n])
