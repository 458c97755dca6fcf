"""CPU checks of the zonal-mean statistics and of the Held-Suarez case (no GPU): the band rule of mimsem_amd/zonalstats.py, the numpy
restatement of tests/zonal_case.py against the restated quadrature dumps of tests/umjs14_case.py, a constant temperature, the position of the
jet, mimsem_amd/heldsuarez.py against mimsem_amd/umjs14.py and the recorded values of the latter from before it took `cut`, the .npz
round trip, and a C++ translation unit that calls the two new methods of mimsem_host::Euler."""
import os
import subprocess

import numpy as np
import pytest

from mimsem_amd import heldsuarez as hs
from mimsem_amd import umjs14 as um
from mimsem_amd.zonalstats import MOMENTS, ZonalStats, band_edges, band_index
from tests import zonal_case as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the band rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2, 6, 7, 64])
def test_band_rule(nb):
    r = np.random.default_rng(nb)
    half = 0.5 * np.pi
    lat = np.concatenate([r.uniform(-half, half, 500), [half, -half, 0.0, -0.0, np.nextafter(half, 4.0), np.nextafter(-half, -4.0)], band_edges(nb)])
    b = band_index(lat, nb)
    assert b.dtype == np.int32 and b.shape == lat.shape and b.min() >= 0 and b.max() < nb       # exactly one band each, none outside
    e = band_edges(nb)
    inside = np.abs(lat) < half
    assert np.all(e[b[inside]] <= lat[inside]) and np.all(lat[inside] < e[b[inside] + 1])      # the band's half-open interval
    assert b[500] == nb - 1 and b[501] == 0 and b[504] == nb - 1 and b[505] == 0              # the poles, and beyond them by rounding, are kept
    if nb % 2 == 0:
        assert b[502] == b[503] == nb // 2                                                      # lat = +-0 on an inner edge: one band
    assert np.array_equal(band_index(lat[:500].reshape(20, 25), nb), b[:500].reshape(20, 25))    # [nEl, mp12] in, [nEl, mp12] out


# ---- point values against the quadrature dumps ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere(oracle):
    """the p = 3, ne = 2, nk = 4 sphere of tests/umjs14_case.py with a physically scaled random state"""
    from tests import umjs14_case as uc
    from tests.energetics_case import state_fields
    c = uc.add_dense(uc.make_mesh())
    r = np.random.default_rng(7)
    P0 = c["gd"].P[0]
    F = state_fields(P0, r, uc.PN, c["nk"], c["gd"].N1, c["gd"].N2)
    c["state"] = (F["u1"], None, F["h1"], F["th"], F["Pi"])
    c["fields"], c["weight"] = zc.point_fields(c["patches"], F["u1"], F["h1"], F["th"], F["Pi"])
    return c


def test_point_values_are_those_of_the_dumps(sphere):
    """u, v, r, Theta, Pi of the restatement against restate_quad_fields (Geom::write1 / write2) at every global quadrature point, read at
    the element whose value the dump keeps there: ties the statistics to the dumps"""
    from tests import umjs14_case as uc
    c, nk = sphere, sphere["nk"]
    velx, _, rho, rt, exner = c["state"]
    r = np.random.default_rng(8)
    quad = uc.restate_quad_fields(c, c["state"], r.standard_normal((nk + 1, c["gd"].N2)), r.standard_normal((nk - 1, c["gd"].N2)))
    last = uc.restate_last_writer(c["topos"], c["geoms"])
    for mine, theirs in (("u", "velocity_h_x"), ("v", "velocity_h_y"), ("r", "density"), ("Theta", "rhoTheta"), ("Pi", "exner")):
        got = c["fields"][mine].reshape(nk, -1)[:, last]
        err = float(np.max(np.abs(got - quad[theirs]) / np.max(np.abs(quad[theirs]))))
        print("%s against %s: %.2e" % (mine, theirs, err))
        assert err <= 1e-14, (mine, err)


def test_weights_sum_to_the_sphere(sphere):
    """a = Q det summed over every element's points is the area of the sphere as the quadrature sees it, and the moment m = 0 of any band
    table that keeps every point sums to it on every level"""
    c = sphere
    lat = zc.latitudes(c)
    S, A = zc.moments(c["fields"], c["weight"], band_index(lat, 6), 6)
    area = 4.0 * np.pi * um.RAD_EARTH ** 2
    assert abs(c["weight"].sum() / area - 1.0) < 1e-3
    assert np.allclose(S[0].sum(axis=1), c["weight"].sum(), rtol=1e-13, atol=0.0)
    assert np.array_equal(S[0], A[0]) and (A >= np.abs(S)).all()


# ---- a constant temperature -------------------------------------------------------------------------------------------------------------
def test_constant_field(oracle):
    """a p = 3, 3 x 3 periodic box with uniform layers: its metric and thickness are constant, so a constant IS in the 2-form space and the
    projection reproduces it at every point.  r = 1.2, Pi = 950, Theta = 300 CP r / Pi: T = 300 at every point; velx = 0"""
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    pn, ne, nk, nb = 3, 3, 2, 4
    bx = PeriodicBox(pn, ne, 1)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, box_coords(pn, ne, 1000.0), nk, 1000.0)
    levs = np.stack([np.full(g.n0, 400.0 * k) for k in range(nk + 1)])
    g.set_levels(levs)
    P = oracle.Patch(pn, pn, bx.nel, nk)
    P.set_metric(g.det, g.J); P.set_levels(levs)
    W, iq, i2 = P.arr("W", (P.mp12, P.n2e)), P.elinds("q"), t.all_inds2_g()
    r0, pi0 = 1.2, 950.0
    consts = (r0, 300.0 * zc.CP * r0 / pi0, pi0)
    fields2 = [np.zeros((nk, bx.nDofs2G)) for _ in consts]
    for k in range(nk):
        for e in range(P.nEl):
            for f, cst in zip(fields2, consts):                                  # W h = c det thick at the points: the projection of the constant
                h, res, _, _ = np.linalg.lstsq(W, cst * P.det[e] * P.thick[k, iq[e]], rcond=None)
                f[k, i2[e]] = h
    velx = np.zeros((nk, bx.nDofs1G))
    band = np.random.default_rng(3).integers(-1, nb - 1, (P.nEl, P.mp12))        # some points left out, band nb - 1 empty
    S, A = zc.restate([(t, g, P)], velx, *fields2, band, nb)
    m = ZonalStats.means_of(S, band_edges(nb))
    full = np.array([(band == b).any() for b in range(nb)])
    assert full[:-1].all() and not full[-1]
    assert np.max(np.abs(m["T"][:, full] / 300.0 - 1.0)) < 1e-12
    assert np.max(np.abs(m["TT"][:, full])) < 1e-9
    assert not m["u"][:, full].any() and not m["v"][:, full].any() and not m["eke"][:, full].any()
    assert np.isnan(m["T"][:, ~full]).all() and np.isnan(m["u"][:, ~full]).all()               # an empty band reads NaN
    assert m["lat"].shape == (nb,) and np.array_equal(m["area"], S[0])


# ---- the jet ----------------------------------------------------------------------------------------------------------------------------
def test_jet_position(oracle):
    """the vp = 0 UMJS14 state on ne = 4, p = 3, nk = 4 in six bands of 30 degrees: u_mean ~ cos^2 sin^2 of the latitude peaks at 45 degrees, so at the
    lowest level the largest zonal-mean u of each hemisphere lies in its band [30, 60] -- with the components swapped, or u taken along a
    cube face's axes, it would not"""
    from tests import umjs14_case as uc
    c = uc.add_dense(uc.make_mesh(ne=4))
    nk, xq = c["nk"], c["coords"]
    uq, rho, rt, exner = um.layer_fields(nk, xq, vp=0.0)
    velx = uc.restate_init1(c, uq)
    fields, weight = zc.point_fields(c["patches"], velx, *(uc.restate_init2(c, f) for f in (rho, rt, exner)))
    S, _ = zc.moments(fields, weight, band_index(zc.latitudes(c), 6), 6)
    m = ZonalStats.means_of(S, band_edges(6))
    u0 = m["u"][0]
    print("zonal-mean u at the lowest level, bands south to north:", " ".join("%.3f" % v for v in u0))
    assert int(np.argmax(u0[:3])) == 1 and int(np.argmax(u0[3:])) == 1 and u0[1] > 1.0 and u0[4] > 1.0
    assert np.max(np.abs(m["v"][0])) < 0.05 * u0[1]                              # the steady jet has no meridional wind
    assert 150.0 < m["T"].min() and m["T"].max() < 350.0


# ---- the Held-Suarez case ---------------------------------------------------------------------------------------------------------------
def test_heldsuarez_against_umjs14(golden_dir):
    d = np.load(os.path.join(golden_dir, "umjs14_ic_nk30.npz"))
    x = d["x"]
    assert (hs.NK, hs.DT, hs.NSTEPS, hs.DUMP_EVERY, hs.INTEGRATOR) == (16, 120.0, 72000, 1440, "strang")      # eul/HeldSuarez.cpp:25, :275-277, :352
    assert hs.NSTEPS == 100 * 24 * 30 and hs.DUMP_EVERY == 2 * 24 * 30
    for name in ("D0", "ZT", "ZTOP", "VP", "rho_init", "rt_init", "exner_init", "theta_init"):
        assert getattr(hs, name) is getattr(um, name), name                      # :26-43 and the thermodynamic fields are UMJS14's
    gc = um.gc_dist(x)
    near, far = gc <= um.D0, gc > um.D0
    assert near.sum() >= 4 and far.sum() >= 2
    a, b = hs.layer_fields(hs.NK, x), um.layer_fields(16, x)
    assert a[0].shape == (16, x.shape[0], 2)
    assert np.array_equal(a[0][:, near], b[0][:, near])                          # inside the disc: bit for bit
    for i in (1, 2, 3):
        assert np.array_equal(a[i], b[i])                                        # rho, rt, exner: everywhere
    below = np.array([0.5 * (um.z_at_level(x, k, 16)[0] + um.z_at_level(x, k + 1, 16)[0]) < um.ZT for k in range(16)])
    assert below.any() and not below.all()
    assert (a[0][below][:, far] != b[0][below][:, far]).any()                   # outside it, below ZT: the uncut perturbation is there
    assert not um.v_init(x, 0, 16)[far].any() and hs.v_init(x, 0)[far].any()
    # layers whose two interfaces lie above ZT: the taper is 0 with or without the cut
    above = np.array([um.z_at_level(x, k, 16)[0] > um.ZT and um.z_at_level(x, k + 1, 16)[0] > um.ZT for k in range(16)])
    assert above.any() and np.array_equal(a[0][above], b[0][above])
    assert np.array_equal(hs.levels(16, x), um.levels(16, x))
    for k in (0, 5):
        assert np.array_equal(hs.u_init(x, k), um.u_init(x, k, 16, cut=False)) and np.array_equal(hs.u_pert(x, k), um.u_pert(x, k, 16, cut=False))
        assert np.array_equal(hs.v_pert(x, k), um.v_pert(x, k, 16, cut=False))


def test_umjs14_defaults_keep_every_bit(golden_dir):
    """tests/golden/umjs14_layer_fields_before_cut.npz: layer_fields, u_pert and v_pert of mimsem_amd/umjs14.py as they were before the `cut`
    keyword, on the points of umjs14_ic_nk30.npz -- the default (and cut=True) give the same bits"""
    x = np.load(os.path.join(golden_dir, "umjs14_ic_nk30.npz"))["x"]
    was = np.load(os.path.join(golden_dir, "umjs14_layer_fields_before_cut.npz"))
    for nk in (4, 16):
        for kw in ({}, {"cut": True}):
            uq, rho, rt, exner = um.layer_fields(nk, x, **kw)
            for name, got in (("uq", uq), ("rho", rho), ("rt", rt), ("exner", exner)):
                assert np.array_equal(got, was["%s_nk%d" % (name, nk)]), (name, nk, kw)
            assert np.array_equal(np.stack([um.u_pert(x, k, nk, **kw) for k in range(nk + 1)]), was["u_pert_nk%d" % nk])
            assert np.array_equal(np.stack([um.v_pert(x, k, nk, **kw) for k in range(nk + 1)]), was["v_pert_nk%d" % nk])


# ---- save / load ------------------------------------------------------------------------------------------------------------------------
class _HostEngine:
    """what ZonalStats needs of an engine, on host tensors: the sums and their file need no device"""
    nEl, mp12, nk = 6, 16, 3

    def zonal_plan(self, band, nb):
        assert band.shape == (self.nEl, self.mp12) and band.min() >= 0 and band.max() < nb
        self.nb = nb

    def zeros(self, *shape):
        import torch
        return torch.zeros(*shape, dtype=torch.float64)

    def tensor(self, a):
        import torch
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)


def test_save_load_round_trip(tmp_path):
    import torch
    r = np.random.default_rng(11)
    lat = r.uniform(-0.5 * np.pi, 0.5 * np.pi, (6, 16))
    a = ZonalStats(_HostEngine(), lat, 5)
    assert a.eng.nb == 5 and tuple(a.acc.shape) == (len(MOMENTS), 3, 5) and a.count == 0
    a.acc.copy_(torch.as_tensor(r.standard_normal((9, 3, 5)))); a.count = 17
    path = str(tmp_path / "zonal_stats.npz")
    a.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["acc", "count", "edges", "nbands"] and int(z["count"]) == 17 and int(z["nbands"]) == 5
        assert np.array_equal(z["edges"], band_edges(5)) and np.array_equal(z["acc"], a.moments())
    b = ZonalStats(_HostEngine(), lat, 5)
    b.load(path)
    assert b.count == 17 and torch.equal(b.acc, a.acc)                           # a restarted run continues the sums
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a.means().values(), b.means().values()))
    b.reset()
    assert b.count == 0 and not b.acc.any()
    with pytest.raises(ValueError):
        ZonalStats(_HostEngine(), lat, 4).load(path)                             # other bands: refused
    with pytest.raises(ValueError):
        ZonalStats(_HostEngine(), lat[:5], 5)
    sharded = _HostEngine(); sharded.halo = object()
    with pytest.raises(NotImplementedError, match="sharded engines are not supported"):
        ZonalStats(sharded, lat, 5)


# ---- the C++ host -----------------------------------------------------------------------------------------------------------------------
def test_shim_methods_compile_and_link(tmp_path):
    """a translation unit that calls mimsem_host::Euler::zonal_plan / zonal_moments compiles with plain g++ -std=c++17 -Wall -Werror against
    the header and links against the built library (tests/test_euler_cpp_build.py builds the step's host the same way)"""
    from mimsem_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    src = tmp_path / "zonal_call.cpp"
    src.write_text('#include "%s"\n'
                   "int sample(mimsem_host::Euler& eu, const int* band, int nb, int nk, const double* velx, const double* rho, const double* rt,\n"
                   "           const double* exner, double* acc) {\n"
                   "    eu.zonal_plan(band, nb);\n"
                   "    eu.zonal_moments(nk, velx, rho, rt, exner, acc);\n"
                   "    return 0;\n"
                   "}\n"
                   "int main() { return 0; }\n" % os.path.join(ROOT, "mimsem_amd", "host", "mimsem_shim.hpp"))
    exe = str(tmp_path / "zonal_call")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(src), "-o", exe, "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
    for name in ("mimsem_zonal_plan_build", "mimsem_euler_zonal_moments"):
        assert name in _lib.exported_symbols()
