"""A call sizes the column workspace (d_col) to exactly what its plan takes (csrc/col_workspace.hpp), so the buffer a call finds depends
on the calls before it; its result must not.  On a one-element-per-face patch of the sphere (order 1, for which the sphere has no
coordinates, on a one-element periodic box), for every column entry that uses the workspace: engine A
makes the call as its first column call, engine B after every other column call of the shape (the largest among them), engine C first
and again after them -- the same bits from all four, and the same status read-back after the solves.  The patch has one column, a
context of it is made in milliseconds: a case (up to nine entries, three contexts each) takes under half a second on an MI355X."""
import numpy as np
import pytest
import torch

from mimsem_amd.workloads import z_levels

pytestmark = pytest.mark.gpu

# orders 1-4 with nk = 2 (the Helmholtz entries only: the _3 solve and its Newton residual take nk >= 4), 4 and 5 (odd: the one-sided
# Thomas and penta kernels); order 5 on the wide paths
CASES = [(pn, nk) for pn in (1, 2, 3, 4) for nk in (2, 4, 5)] + [(5, 4)]


def _mesh(pn, nk):
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.geom import BoxGeom, Geom
    from mimsem_amd.mesh import CubedSphere, PeriodicBox, box_coords, sphere_coords
    from mimsem_amd.topo import Topo
    if pn == 1:                                          # (the sphere's coordinates exist for orders 2-7: order 1 on a one-element periodic box)
        bx = PeriodicBox(pn, 1, 1)
        topo = Topo(bx, 0, nk)
        geom = BoxGeom(topo, bx, box_coords(pn, 1, 1000.0), nk, 1000.0)
    else:
        cs = CubedSphere(pn, 1, 6)
        topo = Topo(cs, 1, nk)
        geom = Geom(topo, cs, sphere_coords(pn, 1), nk)
    geom.set_levels(z_levels(nk, geom.n0, np.random.default_rng(40 + pn)))
    return DeviceMesh([topo], [geom], nk=nk, numbering="global" if pn == 1 else "local")


def _fields(dm, pn, nk, seed):
    """physically scaled column fields, as tests/test_gpu_column.py::_col_fields: 2-form dofs are cell integrals ~ value * det * thick"""
    r = np.random.default_rng(seed)
    nEl, n2 = dm.nEl, pn * pn
    area = float(dm.det.mean()) * 4.0 / n2; dz = float(dm.thick.mean())
    lev = lambda nl, lo, hi: r.uniform(lo, hi, (nEl, nl * n2)) * area * dz
    F = dict(rho=lev(nk, 0.5, 1.2), rt=lev(nk, 250.0, 400.0), theta=lev(nk + 1, 280.0, 320.0) / dz, pi=lev(nk, 700.0, 1000.0),
             eta=lev(nk, 5.0, 6.0), velz=lev(nk - 1, -1.0, 1.0) / dz, thetaL=lev(nk, 280.0, 320.0),
             x=r.standard_normal((nEl, nk * n2)))
    F["rhs"] = [r.standard_normal((nEl, n * n2)) * 1e8 for n in (nk - 1, nk, nk, nk)]
    # the Newton residuals take logarithms of reconstructed fields: a smooth state for them, each dof the integral of a near-constant value over
    # its own GLL sub-cell (share wj of the element's area), as tests/test_gpu_fullsize_oracle.py::_hydrostatic_fields scales it
    from mimsem_amd.geom import gll_points
    wd = np.diff(gll_points(pn)); wj = np.outer(wd, wd).ravel() * float(dm.det.mean())
    smooth = lambda nl, v: np.tile(wj, nl)[None, :] * v * r.uniform(0.995, 1.005, (nEl, nl * n2))
    F["s"] = dict(rho=smooth(nk, 1.0) * dz, rho2=smooth(nk, 1.0) * dz, rt=smooth(nk, 300.0) * dz, rt2=smooth(nk, 300.0) * dz, pi=smooth(nk, 900.0) * dz,
                  thetaL=smooth(nk, 300.0) * dz, theta=smooth(nk + 1, 300.0), velz=smooth(nk - 1, 0.1), velz2=smooth(nk - 1, 0.2), zv=smooth(nk, 1.0e4) * dz)
    return F


def _calls(pn, nk):
    """name -> f(eng, F) returning the tensors the call produces or updates (and the status read-back after a solve)"""
    def status(eng):
        n, st, ratio = eng.solve_status()
        return [torch.tensor([n]), torch.from_numpy(st.copy()), torch.from_numpy(ratio.copy())]

    def eta(eng, F):
        t = eng.tensor
        rhs = [t(x) for x in F["rhs"]]
        d = eng.solve_schur_eta(75.0, t(F["thetaL"]), t(F["rho"]), t(F["eta"]), t(F["pi"]), *rhs)
        return list(d) + rhs + status(eng)

    def schur3(flags):
        def f(eng, F):
            t = eng.tensor
            rhs = [t(x) for x in F["rhs"]]
            d = eng.solve_schur_3(75.0, t(F["theta"]), t(F["velz"]), t(F["rho"]), t(F["rt"]), t(F["pi"]), *rhs, want_L=True, flags=flags)
            return list(d) + rhs + status(eng)
        return f

    def newton(eng, F):
        t, S = eng.tensor, F["s"]
        return list(eng.newton_residual(75.0, 0.1, t(S["thetaL"]), t(S["pi"]), t(S["velz"]), t(S["velz2"]), t(S["rho"]), t(S["rho2"]),
                                        t(S["zv"]), t(S["rt"]), t(S["rt2"]), t(S["rho"]), t(S["rt"]), t(S["pi"])))

    def newton2(eng, F):
        t, S = eng.tensor, F["s"]
        return list(eng.newton2_residual(75.0, 0.1, t(S["theta"]), t(S["pi"]), t(S["velz"]), t(S["velz2"]), t(S["rho"]), t(S["rho2"]),
                                         t(S["zv"]), t(S["rt"]), t(S["rt2"]), t(S["pi"])))

    calls = {"solve_schur_eta": eta,
             "helmholtz_blocks": lambda eng, F: [eng.helmholtz_blocks(75.0, *[eng.tensor(F[k]) for k in ("thetaL", "rho", "eta", "pi")])]}
    if nk >= 4:
        calls["colop_apply"] = lambda eng, F: [eng.colop_apply("EOS_BLOCK_INV", eng.tensor(F["x"]), f1=eng.tensor(F["pi"]), nout_slots=nk)]
        calls["diag_theta_L2"] = lambda eng, F: [eng.diag_theta(0, eng.tensor(F["rho"]), eng.tensor(F["rt"]))]
        calls["diag_theta_2"] = lambda eng, F: [eng.diag_theta(1, eng.tensor(F["rho"]), eng.tensor(F["rt"]))]
        calls["solve_schur_3"] = schur3(0)
        calls["solve_schur_3_box"] = schur3(3)
        if pn <= 4:                                      # the fused Newton residuals exist for orders 1-4
            calls["newton_residual"] = newton
            calls["newton2_residual"] = newton2
    return calls


def _same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and
                                    torch.equal(x.cpu().contiguous().view(torch.uint8), y.cpu().contiguous().view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("pn,nk", CASES, ids=["p%d_nk%d" % c for c in CASES])
def test_a_column_call_gives_the_same_bits_wherever_it_comes_in_the_sequence(pn, nk):
    from mimsem_amd.device import Engine
    calls = _calls(pn, nk)
    dm = _mesh(pn, nk)
    F = _fields(dm, pn, nk, seed=7 * pn + nk)
    for name, call in calls.items():
        others = [f for n, f in calls.items() if n != name]
        first = call(Engine(dm), F)                      # engine A: the first column call of its context
        eng_b = Engine(dm)                               # engine B: after every other call, the largest request of the shape among them
        for f in others:
            f(eng_b, F)
        after = call(eng_b, F)
        eng_c = Engine(dm)                               # engine C: first, and again after the others
        c_first = call(eng_c, F)
        for f in others:
            f(eng_c, F)
        c_again = call(eng_c, F)
        assert all(bool(torch.isfinite(x).all()) for x in first if x.dtype.is_floating_point), name      # (equal bits of NaNs would say nothing)
        assert _same_bits(first, after), (name, "first call against the call after the largest")
        assert _same_bits(first, c_first) and _same_bits(first, c_again), (name, "within one context")
