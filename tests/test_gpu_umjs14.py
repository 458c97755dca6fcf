"""The baroclinic-wave driver on the device (mimsem_amd/euler.py: init1, init2, initial_state, run, dump, load) against the numpy restatements
of tests/umjs14_case.py, on the p = 3, ne = 2, nk = 4 sphere of tests/strang_case.py with the levels umjs14.levels(4, xq).

Bars: init1, init2 and the quadrature dumps are single operator chains held to the project's parity bar, 1e-10 relative L2 per level,
against LU-solved restatements.  run / dump / load are held to bit equality: run is strang_ec repeated, the .vec files carry the float64
bits, and two objects with the same history of solves settle on the same fixed lengths.  (A second Euler therefore builds its own initial
state before it steps: the first 1-form mass solve of an object calibrates its fixed length on that solve's right-hand side.)

Observed on an MI355X (relative L2 per level, the worst level):
    init2(rho_init) 3.1e-16      init1(u_init, v_init) 6.0e-16      init1 after a forced miss (adaptive rerun) 4.1e-16
    .npy against the restatement: vorticity 1.2e-15, velocity_h_x 1.8e-16, velocity_h_y 1.9e-15, density 2.6e-16, rhoTheta 2.6e-16,
    exner 2.4e-16, theta 8.1e-16, velocity_z 2.3e-16; the dumped theta .vec against the restated diagTheta2 4.6e-16
"""
import os

import numpy as np
import pytest
import torch

from mimsem_amd import io
from mimsem_amd import umjs14 as um
from tests import umjs14_case as uc
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
PARITY = 1e-10
MASS_BAR = 1e-13         # test_a_physical_step: how the figure was arrived at
DT = 75.0
STEP_KW = dict(newton_maxit=3, newton_tol=0.0)         # the fixed Newton count of tests/strang_case.py: the small sphere is not a physical run


def per_level(label, got, want, bar=PARITY):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape, (label, got.shape, want.shape)
    errs = [rel_l2(g, w) for g, w in zip(got, want)]
    print("%s: relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
    assert np.isfinite(got).all() and max(errs) < bar, (label, errs)
    return errs


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def case(oracle):
    c = uc.add_engine(uc.add_dense(uc.make_mesh()))
    c["uq"], c["rho_q"], c["rt_q"], c["exner_q"] = um.layer_fields(c["nk"], c["xq"])
    return c


@pytest.fixture(scope="module")
def ran(case, tmp_path_factory):
    """run(state, 3, dump_every=2) from initial_state() beside three strang_ec calls on a second Euler"""
    out = str(tmp_path_factory.mktemp("umjs14") / "output")
    eu = uc.make_euler(case, DT, **STEP_KW)
    st0 = eu.initial_state()
    seen = []
    final = eu.run(st0, 3, dump_every=2, outdir=out, on_step=lambda step, values: seen.append((step, values)))
    eu2 = uc.make_euler(case, DT, **STEP_KW)
    st, steps = eu2.initial_state(), []
    assert same_bits(st, st0)
    for _ in range(3):
        o = eu2.strang_ec(*st)
        st = o[:5]
        steps.append(o)
    return dict(eu=eu, eu2=eu2, st0=st0, final=final, seen=seen, steps=steps, out=out)


def test_init2_matches_the_element_wise_lu(case):
    eu = uc.make_euler(case, DT)
    per_level("init2(rho_init)", eu.init2(case["rho_q"]), uc.restate_init2(case, case["rho_q"]))
    assert eu._m2_inverse() is eu._m2_inverse()                          # built once
    with pytest.raises(ValueError):
        eu.init2(case["rho_q"][:-1])


def test_init1_matches_the_dense_lu_and_reruns_after_a_missed_check(case):
    eu = uc.make_euler(case, DT)
    want = uc.restate_init1(case, case["uq"])
    per_level("init1(u_init, v_init)", eu.init1(case["uq"]), want)
    m1 = eu.horiz.m1
    assert m1.chebyshev and eu.init1_redone == 0 and m1.solves_missed == 0 and m1.solves_checked >= 1
    m1._chebyshev().set_steps(1)                                         # one Chebyshev step: the check of the solve must fail
    per_level("init1 after a forced miss", eu.init1(case["uq"]), want)
    assert eu.init1_redone == 1 and m1.solves_missed == 1 and not m1.chebyshev
    assert eu.horiz.verify()                                             # nothing left in the log


def _projection_error(c):
    eu = uc.make_euler(c, DT)
    eng, dm = c["eng"], c["eng"].mesh
    rho_q = um.layer_fields(c["nk"], c["xq"])[1]
    dens = (eng.interp_quad(2, eu.init2(rho_q)) / eng.tensor(dm.thick)).cpu().numpy()
    want = rho_q[:, dm.indsq]
    assert np.isfinite(dens).all()
    return rel_l2(dens, want)


def test_projection_error_falls_with_resolution(case):
    """observed: ne = 2 1.627e-02, ne = 4 2.330e-03 (no value is fixed here: the error falls, and both are finite)"""
    e2 = _projection_error(case)
    e4 = _projection_error(uc.add_engine(uc.make_mesh(ne=4)))
    print("density on the quadrature grid against rho_init, relative L2: ne = 2 %.3e, ne = 4 %.3e" % (e2, e4))
    assert np.isfinite(e2) and np.isfinite(e4) and e4 < e2


def test_run_is_the_step_repeated(case, ran):
    from mimsem_amd.energetics import FIELDS, Energetics
    eu, eu2 = ran["eu"], ran["eu2"]
    assert same_bits(ran["final"], ran["steps"][2][:5])
    assert eu.steps == eu2.steps == 3 and eu.redone == eu2.redone and eu.step == 1 and not eu.first_step
    assert not ran["st0"][1].any()                                       # velz = 0 (eul/UMJS14.cpp:313-316)
    assert [s for s, _ in ran["seen"]] == [1, 2, 3]
    with open(os.path.join(ran["out"], "energetics.dat")) as f:
        lines = f.read().splitlines(keepends=True)
    assert len(lines) == 3
    for i, line in enumerate(lines):
        vals = ran["steps"][i][5]
        assert len(vals) == len(FIELDS) and vals == ran["seen"][i][1]
        p = os.path.join(ran["out"], "line_%d.dat" % i)
        Energetics.write_line(p, vals)
        with open(p) as f:
            assert f.read() == line
        os.remove(p)


def test_one_dump_under_step_index_one(case, ran):
    nk, out = case["nk"], ran["out"]
    names = {"energetics.dat"}
    names |= {"%s_%.3u_0001.vec" % (f, k) for f, d in uc.VEC_FIELDS for k in range(nk + d)}
    names |= {"%s_0001.npy" % f for f, _, _ in uc.QUAD_FIELDS}
    assert set(os.listdir(out)) == names
    after2 = ran["steps"][1][:5]
    eng = case["eng"]
    dev = {"velocity_h": after2[0], "density": after2[2], "rhoTheta": after2[3], "exner": after2[4],
           "velocity_z": eng.l2_vert_to_horiz(after2[1].contiguous(), nk - 1),
           "theta": eng.l2_vert_to_horiz(eng.diag_theta(1, eng.l2_horiz_to_vert(after2[2]), eng.l2_horiz_to_vert(after2[3])), nk + 1)}
    for f, d in uc.VEC_FIELDS:
        got = io.load_levels(f, 1, nk + d, out)
        assert got.shape == tuple(dev[f].shape) and np.array_equal(got, dev[f].cpu().numpy()), f
    assert dev["velocity_z"].any()                                       # the step has set the air moving


def test_restart(case, ran):
    after2 = ran["steps"][1][:5]
    eu3 = uc.make_euler(case, DT, **STEP_KW)
    st = eu3.load(1, ran["out"])
    assert same_bits(st, after2) and eu3.first_step and eu3.u_prev is None and eu3.uz_prev is None
    was_first = eu3.first_step
    o3 = eu3.strang_ec(*st)
    o4 = uc.make_euler(case, DT, **STEP_KW).strang_ec(*after2)
    assert was_first and not eu3.first_step
    assert same_bits(o3[:5], o4[:5]) and o3[5] == o4[5]
    assert not same_bits(o3[:5], ran["steps"][2][:5])                    # the restarted run is not the continued run (no u_prev, uz_prev in the dumps)
    # load on an object that has stepped puts it back to a first step
    eu3.load(1, ran["out"])
    assert eu3.first_step and eu3.u_curr is None


def test_quadrature_dumps(case, ran, tmp_path):
    nk, out = case["nk"], ran["out"]
    vec = {f: io.load_levels(f, 1, nk + d, out) for f, d in uc.VEC_FIELDS}
    state = (vec["velocity_h"], None, vec["density"], vec["rhoTheta"], vec["exner"])
    theta = uc.restate_theta2(case, vec["density"], vec["rhoTheta"])
    per_level("theta .vec", vec["theta"], theta)
    want = uc.restate_quad_fields(case, state, theta, vec["velocity_z"])
    for f, d, _ in uc.QUAD_FIELDS:
        got = np.load(os.path.join(out, "%s_0001.npy" % f))
        assert got.shape == (nk + d, case["eng"].sizes["q"]) and got.dtype == np.float64
        per_level(f + " .npy", got, want[f])
    # two dumps of the same state are the same bits
    eu, again = ran["eu"], str(tmp_path / "again")
    eu.dump(ran["steps"][1][:5], 1, again)
    for name in sorted(os.listdir(again)):
        with open(os.path.join(again, name), "rb") as a, open(os.path.join(out, name), "rb") as b:
            assert a.read() == b.read(), name
    assert len(os.listdir(again)) == len(os.listdir(out)) - 1           # (energetics.dat belongs to run)


def test_a_physical_step():
    """nk = 8 on the ne = 4 sphere, dt = 75, newton_maxit = 20, two steps from initial_state().
    Observed on an MI355X: the first step is redone once (velz = 0 makes stage 1's diagVertVort a solve with a zero right-hand side; the
    fixed length it leaves is too short for stage 3) and passes; on this coarse mesh the Newton loop uses all 20 iterations in both steps
    and ends at |d_exner|/|exner| 9.1e-12 / 1.1e-11, |d_rho|/|rho| 5.7e-12 / 6.9e-12 (tol 1e-12; the bench mesh converges in 11 .. 13,
    profiles/umjs14_run.txt); max|velz| 4.325e+12 / 2.581e+12 (degrees of freedom: velocity times face area).  Not asserted against numbers.
    mass: the relative change from the initial mass is 0 after both steps on the device; the same two steps through
    strang_case.Restatement on the CPU (6 Newton iterations, max|velz| 4.324e+12 / 2.581e+12) change it by 1.8e-15 and 0.  MASS_BAR is
    the larger observation, the restatement's, x 10 rounded up to a power of ten: 1e-13 (the cap is 1e-10)."""
    from mimsem_amd.energetics import FIELDS
    c = uc.add_engine(uc.make_mesh(ne=4, nk=8))
    eu = uc.make_euler(c, DT, newton_maxit=20)
    st = eu.initial_state()
    im = FIELDS.index("mass")
    mass0 = eu.energetics.diagnostics(*st)[im]
    assert np.isfinite(mass0) and mass0 > 0.0
    for i in range(2):
        o = eu.strang_ec(*st)                                            # (raises if a redone step misses its checks again)
        st = o[:5]
        for name, a in zip(("velx", "velz", "rho", "rt", "exner"), st):
            assert bool(torch.isfinite(a).all()), (i, name)
        change = abs(o[5][im] - mass0) / mass0
        print("step %d: Newton iterations %d, last norms %s, steps redone so far %d, max|velz| %.3e, mass %.16e, relative change %.2e"
              % (i + 1, len(eu.vert.history), eu.vert.history[-1], eu.redone, float(st[1].abs().max()), o[5][im], change))
        assert all(np.isfinite(v) for v in o[5])
        assert MASS_BAR <= 1e-10 and change <= MASS_BAR, (i, change)
    assert eu.steps == 2 and eu.redone <= 2


