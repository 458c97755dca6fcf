#!/usr/bin/env python3
"""Every output of the two fused Newton residual entries and of three fused iterations of both vertical Newton loops, written as .npy files:
what two builds of the library (MIMSEM_LIB=... against the default) must agree on byte for byte.  On the one-column meshes of
tests/test_gpu_column_call_order.py, orders 1-4, nk = 4 and 5:
  newton_residual / newton2_residual   on that test's smooth fields, once with every optional input set and once with all of them null
  solve_schur_eta, solve_schur_2       three fused iterations (tol = 0) from a column at rest (order 2: on the one-element box, see below), with
                                       hs_lat, udwdx and a fixed horizontal forcing:
                                       the state, theta_h, theta_l2_h (the eta loop's alone), exner_h, the history and k2i_z
  usage: dump_newton.py OUTDIR      then: cmp the files of two OUTDIRs (scripts/dump_newton.py writes nothing else)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from mimsem_amd.device import Engine  # noqa: E402
from mimsem_amd.geom import gll_points  # noqa: E402
from mimsem_amd.vertsolve import VertSolve  # noqa: E402
from tests.test_gpu_column_call_order import _fields, _mesh  # noqa: E402

DT = 0.5


def _box_mesh(pn, nk):
    """the one-element periodic box of tests/test_gpu_column_call_order.py::_mesh (its order-1 case), at order pn"""
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import z_levels
    bx = PeriodicBox(pn, 1, 1)
    topo = Topo(bx, 0, nk)
    geom = BoxGeom(topo, bx, box_coords(pn, 1, 1000.0), nk, 1000.0)
    geom.set_levels(z_levels(nk, geom.n0, np.random.default_rng(40 + pn)))
    return DeviceMesh([topo], [geom], nk=nk, numbering="global")


def main(out):
    os.makedirs(out, exist_ok=True)
    nfiles = 0

    def save(name, arrays):
        nonlocal nfiles
        for i, a in enumerate(arrays):
            a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
            if not np.all(np.isfinite(a)):
                raise SystemExit("%s[%d] is not finite: equal bits of NaNs would say nothing" % (name, i))
            np.save(os.path.join(out, "%s_%d.npy" % (name, i)), a)
            nfiles += 1

    for pn in (1, 2, 3, 4):
        for nk in (4, 5):
            dm = _mesh(pn, nk)
            S = _fields(dm, pn, nk, seed=7 * pn + nk)["s"]
            eng = Engine(dm)
            t = eng.tensor
            tag = "p%d_nk%d" % (pn, nk)
            add_w, add_rho, add_rt, add_hs = 1e-3 * S["velz2"], 1e-3 * S["rho2"], 1e-3 * S["rt2"], 1e-4 * S["rt"]
            for opt in (True, False):
                o = (lambda x: t(x)) if opt else (lambda x: None)
                save("%s_newton_residual_%s" % (tag, "opt" if opt else "null"), eng.newton_residual(
                    75.0, 0.1, t(S["thetaL"]), t(S["pi"]), t(S["velz"]), t(S["velz2"]), t(S["rho"]), t(S["rho2"]), t(S["zv"]), t(S["rt"]), t(S["rt2"]),
                    t(S["rho"]), t(S["rt"]), t(S["pi"]), add_w=o(add_w), add_rho=o(add_rho), add_rt=o(add_rt)))
                save("%s_newton2_residual_%s" % (tag, "opt" if opt else "null"), eng.newton2_residual(
                    75.0, 0.1, t(S["theta"]), t(S["pi"]), t(S["velz"]), t(S["velz2"]), t(S["rho"]), t(S["rho2"]), t(S["zv"]), t(S["rt"]), t(S["rt2"]),
                    t(S["pi"]), add_w=o(add_w), add_rho_pre=o(add_rho), add_rt_pre=o(add_rt), add_rt_post=o(add_hs)))
            # the loops take logarithms and powers of their own iterates: they start from the column at rest of
            # tests/test_gpu_column.py::_newton_start (EOS-consistent, 1e-4 noise, zv from initGZ), not from the smooth fields.  At order 2
            # one element per face of the sphere is too coarse for that column (det varies fivefold over the element: the iteration
            # leaves the domain of the logarithm in its third step, on either route), so order 2 takes order 1's one-element box
            if pn == 2:
                dm = _box_mesh(pn, nk)
                eng = Engine(dm)
                t = eng.tensor
            r = np.random.default_rng(100 * pn + nk)
            wd = np.diff(gll_points(pn)); wj = np.outer(wd, wd).ravel()
            cell = dm.det.mean(axis=1)[:, None, None] * dm.thick.mean(axis=2).T[:, :, None] * wj[None, None, :]       # [nEl, nk, n2]
            rho_v, th_v = np.linspace(1.2, 0.5, nk), np.linspace(290.0, 330.0, nk)
            pi_v = 1004.5 * (287.0 * rho_v * th_v / 1.0e5) ** (287.0 / 717.5)
            n2 = pn * pn
            colv = lambda v: t((cell * v[None, :, None]).reshape(dm.nEl, nk * n2) * (1.0 + 1e-4 * r.standard_normal((dm.nEl, nk * n2))))
            g = dm.geoms[0]
            levs = g.levs                                               # (local numbering: the patch's own order)
            if dm.gidq is not None:
                levs = np.zeros((nk + 1, dm.nq))
                levs[:, np.searchsorted(dm.gidq, g.loc0[np.arange(g.n0)])] = g.levs
            vs = VertSolve(eng, DT)
            st = (eng.zeros(dm.nEl, (nk - 1) * n2), colv(rho_v), colv(rho_v * th_v), colv(pi_v), vs.init_gz(levs))
            lat = t(np.linspace(-1.2, 1.2, dm.nEl * eng.mp12).reshape(dm.nEl, eng.mp12))
            # a fixed forcing, small against what it joins: the eta loop adds it AFTER the VB product, the schur-2 loop before it
            fx, gx = 1e-5 * st[1], 1e-5 * st[2]
            vfx, vgx = eng.colop_apply("CONST", fx, nout_slots=nk), eng.colop_apply("CONST", gx, nout_slots=nk)
            udwdx = t(1e-3 * r.standard_normal((dm.nEl, (nk - 1) * n2)) * float(st[4].abs().mean()) / 9.80616 / 1.5e4)
            vs.fused = True
            got = vs.solve_schur_eta(*st, horiz_forcing=lambda *a: (vfx, vgx), udwdx=udwdx, hs_lat=lat, maxit=3, tol=0.0)
            hist = np.array([[h[k] for k in ("exner", "w", "rho", "eta")] for h in vs.history])
            save("%s_solve_schur_eta" % tag, list(got) + [vs.theta_h, vs.theta_l2_h, vs.exner_h, hist, np.array([vs.k2i_z])])
            vs = VertSolve(eng, DT)
            got = vs.solve_schur_2(*st, horiz_forcing=lambda *a: (fx, gx), udwdx=udwdx, hs_lat=lat, maxit=3, tol=0.0, fused=True)
            hist = np.array([[h[k] for k in ("exner", "w", "rho", "rt")] for h in vs.history])
            save("%s_solve_schur_2" % tag, list(got) + [vs.theta_h, vs.exner_h, hist, np.array([vs.k2i_z])])
    print("dump_newton: %d arrays in %s (library: %s)" % (nfiles, out, os.environ.get("MIMSEM_LIB", "default")))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
