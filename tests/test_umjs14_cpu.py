"""mimsem_amd/umjs14.py against recorded results of the reference's own functions (tests/golden/umjs14_ic_nk30.npz, written by
tests/golden/make_umjs14_fixtures.py from eul/UMJS14.cpp:24-232), the levels, the last-writer table of the quadrature dumps and the .vec files
of the two new level counts.  No GPU.

Error measure: max |numpy - reference| over all points and levels of a function, relative to max |reference| of that function.  (Point by
point the quotient is not a measure of the restatement: u_mean cancels to 1e-10 of the jet's scale at the poles, u_pert / v_pert pass through
zero.)  Bar per function: the observed value x 10, rounded up to a power of ten, none above 1e-12 (CAP).  Observed:
    z_at_level 0          z_taper    0          gc_dist    9.31e-17
    u_pert     4.33e-16   v_pert     3.76e-16   theta_init 1.70e-16
    u_init     2.04e-15   v_init     3.76e-16   rho_init   3.07e-16   rt_init 4.91e-16   exner_init 1.13e-16
z_at_level and z_taper reproduce the reference's bits (sqrt and IEEE arithmetic in the same order), so their bar is 0.  Exact zeros of the
reference are exact zeros here: both guards, and v_pert / u_pert outside the disc."""
import os

import numpy as np
import pytest

from mimsem_amd import io
from mimsem_amd import umjs14 as um

CAP = 1e-12
BARS = dict(z_at_level=0.0, z_taper=0.0, gc_dist=1e-15, u_pert=1e-14, v_pert=1e-14, theta_init=1e-14,
            u_init=1e-13, v_init=1e-14, rho_init=1e-14, rt_init=1e-14, exner_init=1e-14)
INTERFACE = ("z_at_level", "z_taper", "u_pert", "v_pert", "theta_init")
LAYER = ("u_init", "v_init", "rho_init", "rt_init", "exner_init")


@pytest.fixture(scope="module")
def recorded(golden_dir):
    d = np.load(os.path.join(golden_dir, "umjs14_ic_nk30.npz"))
    nk, x = int(d["nk"]), d["x"]
    got = {n: np.stack([getattr(um, n)(x, k, nk) for k in range(nk + 1)]) for n in INTERFACE}
    got.update({n: np.stack([getattr(um, n)(x, k, nk) for k in range(nk)]) for n in LAYER})
    got["gc_dist"] = um.gc_dist(x)
    return d, got


@pytest.mark.parametrize("name", sorted(BARS))
def test_functions_match_the_reference(recorded, name):
    d, got = recorded
    ref = d[name]
    assert got[name].shape == ref.shape and np.isfinite(ref).all()
    err = float(np.abs(got[name] - ref).max() / np.abs(ref).max())
    print("%s: max |numpy - reference| / max |reference| = %.2e (bar %.0e)" % (name, err, BARS[name]))
    assert BARS[name] <= CAP and err <= BARS[name]
    assert np.array_equal(got[name] == 0.0, ref == 0.0)                      # the reference's exact zeros, and no others


def test_guards_and_the_disc(recorded):
    """points 0-3 of the fixture: the centre, its antipode and the two points near the centre, where the reference returns 0 from its guards;
    points 6, 7: outside the disc (gc > D0); point 4: inside.  Above ZT the taper is 0 at every point"""
    d, got = recorded
    nk, gc = int(d["nk"]), got["gc_dist"]
    assert gc[0] == 0.0 and abs(gc[1] - um.RAD_EARTH * np.pi) < um.GUARD
    assert gc[4] < gc[5] < um.D0 < gc[6] < gc[7]
    for n in ("u_pert", "v_pert"):
        assert not got[n][:, [0, 1, 2, 3, 6, 7]].any(), n
        assert not d[n][:, [0, 1, 2, 3, 6, 7]].any(), n
    assert got["u_pert"][0, 4] != 0.0 and got["u_pert"][0, 5] != 0.0
    assert not got["v_init"][:, [0, 1, 2, 3, 6, 7]].any()
    above = np.array([um.z_at_level(d["x"], k, nk)[0] > um.ZT for k in range(nk + 1)])
    assert above.any() and not got["z_taper"][above].any() and not got["u_pert"][above].any()


def test_no_nan_or_inf_at_the_guard_points(recorded):
    d, got = recorded
    for n, a in got.items():
        assert np.isfinite(a).all(), n
    # the centre itself and its antipode for another level count, and the steady state
    x = d["x"][:4]
    with np.errstate(all="raise"):
        for k in range(4):
            for f in (um.u_init, um.v_init):
                assert np.isfinite(f(x, k, 4)).all() and np.isfinite(f(x, k, 4, vp=0.0)).all()
    assert not um.v_init(d["x"], 0, 30, vp=0.0).any()
    assert np.array_equal(um.u_init(d["x"], 0, 30, vp=0.0), um.u_mean(d["x"], um._z_mid(d["x"], 0, 30) + um.RAD_EARTH))


@pytest.mark.parametrize("nk", [4, 8, 30])
def test_levels(recorded, nk):
    d, _ = recorded
    lv = um.levels(nk, d["x"])
    assert lv.shape == (nk + 1, d["x"].shape[0])
    assert not lv[0].any() and np.array_equal(lv[nk], np.full(d["x"].shape[0], um.ZTOP))
    assert (np.diff(lv, axis=0) > 0.0).all()
    assert (np.diff(lv, n=2, axis=0) > 0.0).all()                           # stretched: every layer thicker than the one below
    if nk == 30:
        # Geom::initTopog stores (top - topog) z / top + topog (eul/Geom.cpp:755): z_at_level up to the rounding of top z / top
        assert (np.abs(lv - d["z_at_level"]) <= np.spacing(d["z_at_level"])).all()


def test_layer_fields_are_the_driver_s_arguments(recorded):
    d, got = recorded
    uq, rho, rt, exner = um.layer_fields(30, d["x"])
    assert uq.shape == (30, d["x"].shape[0], 2)
    assert np.array_equal(uq[..., 0], got["u_init"]) and np.array_equal(uq[..., 1], got["v_init"])
    assert np.array_equal(rho, got["rho_init"]) and np.array_equal(rt, got["rt_init"]) and np.array_equal(exner, got["exner_init"])


def test_last_writer_table_is_the_reference_s_visiting_order():
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.euler import last_writer_table
    from tests import umjs14_case as uc
    c = uc.make_mesh()
    dm = DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global")
    assert np.array_equal(dm.gidq, np.arange(dm.nq))
    got = last_writer_table(dm.indsq, dm.nq)
    want = uc.restate_last_writer(c["topos"], c["geoms"])
    assert got.shape == want.shape == (dm.nq,) and (want >= 0).all()
    assert np.array_equal(got, want)
    assert np.array_equal(dm.indsq.reshape(-1)[got], np.arange(dm.nq))        # the chosen point is a copy of the global point
    shared = np.bincount(dm.indsq.reshape(-1), minlength=dm.nq) > 1
    first = np.full(dm.nq, -1); first[dm.indsq.reshape(-1)[::-1]] = np.arange(dm.indsq.size)[::-1]
    assert shared.any() and (got[shared] > first[shared]).all() and np.array_equal(got[~shared], first[~shared])
    with pytest.raises(ValueError):
        last_writer_table(dm.indsq, dm.nq + 1)


@pytest.mark.parametrize("field,dlev", [("velocity_z", -1), ("theta", 1)])
def test_vec_files_of_the_new_level_counts(tmp_path, field, dlev):
    nk, n2, step = 4, 54, 7
    a = np.random.default_rng(5).standard_normal((nk + dlev, n2))
    out = str(tmp_path / "output")
    io.save_levels(field, step, a, out)
    assert sorted(os.listdir(out)) == ["%s_%.3u_%.4u.vec" % (field, k, step) for k in range(nk + dlev)]
    assert os.path.basename(io.vec_filename(field, step, nk + dlev - 1, out)) == "%s_%03d_0007.vec" % (field, nk + dlev - 1)
    back = io.load_levels(field, step, nk + dlev, out)
    assert back.dtype == np.float64 and np.array_equal(back, a)
    with pytest.raises(OSError):
        io.load_levels(field, step, nk + dlev + 1, out)
