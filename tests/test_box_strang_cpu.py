"""CPU checks behind the box twin's step (tests/box_strang_case.py): the point-wise form of the element-local momentum forcing against the
oracle's dense matrices -- on a sphere with a full Jacobian and on a periodic box, term by term and summed."""
import numpy as np
import pytest

from tests import box_strang_case as bc
from tests.helpers import rel_l2

POINTWISE_TOL = 1e-12            # two float64 evaluations of one sum in different orders (the bar of tests/test_euler_fused_cases_cpu.py)


def _levels(label, got, want):
    errs = [rel_l2(got[k], want[k]) for k in range(want.shape[0])]
    print("%s: relative L2 per level  %s" % (label, "  ".join("%.2e" % e for e in errs)))
    assert np.isfinite(got).all() and all(np.linalg.norm(w) > 0 for w in want) and max(errs) < POINTWISE_TOL, (label, errs)


@pytest.fixture(scope="module")
def sphere(oracle):
    return bc.sphere_forcing_case()


@pytest.fixture(scope="module")
def box(oracle):
    return bc.box_forcing_case(oracle)


@pytest.mark.parametrize("terms", [("rot",), ("pgf",), ("vor",), bc.TERMS], ids=lambda t: "+".join(t))
@pytest.mark.parametrize("which", ["sphere", "box"])
def test_pointwise_forcing_against_the_dense_matrices(which, terms, sphere, box):
    c = sphere if which == "sphere" else box
    for vert in ((False, True) if "pgf" in terms else (False,)):
        _levels("%s %s vert=%d" % (which, "+".join(terms), vert), bc.forcing_assembled(c["gd"], c["FF"], terms, vert),
                bc.forcing_dense(c["gd"], c["FF"], terms, vert))


def test_the_sphere_has_a_full_jacobian_and_the_terms_are_balanced(sphere, box):
    from tests.euler_fused_cases import JACOBIAN_MIN, jacobian_ratio
    assert max(jacobian_ratio(P) for P in sphere["gd"].P) >= JACOBIAN_MIN
    assert jacobian_ratio(box["gd"].P[0]) == 0.0
    for c in (sphere, box):
        n = [np.linalg.norm(bc.forcing_dense(c["gd"], c["FF"], (t,))) for t in bc.TERMS]
        assert max(n) / min(n) < 1.0 + 1e-9, n


# ---- BoxHorizSolve's host-side pieces ----------------------------------------------------------------------------------------------------
def test_viscosity_closed_form():
    """box/HorizSolve.cpp:106-114: del2 = -sqrt(2 * 0.072 dx^3.2), dx = sqrt(LX^2 / nDofs0G)"""
    from mimsem_amd.horizsolve import LX, BoxHorizSolve
    from mimsem_amd.mesh import PeriodicBox
    assert LX == 1000.0
    for pn, ne in ((3, 3), (4, 32)):
        n0g = PeriodicBox(pn, ne, 1).nDofs0G
        assert n0g == (pn * ne) ** 2
        dx = 1000.0 / (pn * ne)
        want = -((2.0 * 0.072 * dx ** 3.2) ** 0.5)
        got = BoxHorizSolve.viscosity(LX, n0g)
        assert got < 0 and abs(got - want) <= 4e-16 * abs(want), (got, want)
    assert abs(BoxHorizSolve.viscosity(500.0, 81) - BoxHorizSolve.viscosity(1000.0, 324)) < 1e-14     # only lx^2 / n0g counts


def test_uniform_layer_check(oracle):
    from mimsem_amd.device import DeviceMesh
    from mimsem_amd.horizsolve import uniform_thickness
    c = bc.make_case(oracle)
    assert uniform_thickness(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"]).thick) == bc.DZ
    p = bc.make_case(oracle, uniform=False)                                  # box_schur2_case.make_box: levels perturbed per point
    with pytest.raises(ValueError, match="uniform layers only"):
        uniform_thickness(DeviceMesh([p["topo"]], [p["geom"]], nk=p["P"].nk).thick)
    with pytest.raises(ValueError):
        uniform_thickness(np.array([10.0, 10.0 * (1.0 + 3e-14)]))
    assert uniform_thickness(np.array([10.0, 10.0 * (1.0 + 2e-16)])) > 0


# ---- mimsem_amd/bubble.py ----------------------------------------------------------------------------------------------------------------
def test_bubble_fields():
    from mimsem_amd import bubble as bb
    nk = 30
    x = np.array([[500.0, 500.0, 0.0], [500.0, 260.0, 0.0], [10.0, 990.0, 0.0], [500.0, 749.9, 0.0]])
    ks = np.arange(nk + 1)
    z = np.array([bb.z_at_level(x, k, nk)[0] for k in ks])
    assert z[0] == 0.0 and z[-1] == bb.ZTOP and np.allclose(np.diff(z), bb.ZTOP / nk, rtol=1e-14)
    assert bb.NK == 150 and bb.ZTOP == 1500.0 and bb.LX == 1000.0 and bb.THETA_0 == 300.0
    # Exner is hydrostatic: theta_0 dPi/dz = -g (Pi is linear in z, so differences are exact to round-off)
    Pi = np.array([bb.exner_init(x, k, nk)[0] for k in ks])
    dPidz = np.diff(Pi) / np.diff(z)
    assert np.max(np.abs(bb.THETA_0 * dPidz + bb.GRAVITY)) < 1e-10 * bb.GRAVITY
    # the unperturbed column satisfies the equation of state of column_eos: Pi = cp (R rho theta / p0)^(R / cv)
    rho = np.array([bb.rho_init(x, k, nk)[0] for k in ks])
    assert np.max(np.abs(bb.CP * (bb.RD * rho * bb.THETA_0 / bb.P0) ** (bb.RD / bb.CV) / Pi - 1.0)) < 1e-14
    # the perturbation: 0.5 K at the centre (z = 350 m is level 7 of 30), exactly 0 for r >= 250
    assert z[7] == 350.0
    th = np.stack([bb.theta_init(x, k, nk) for k in ks])
    assert abs(th[7, 0] - (bb.THETA_0 + 0.5)) < 1e-13
    assert np.all(th[:, 2] == bb.THETA_0) and np.all(th[[0, 1, 2, 12, 13, 30], 0] == bb.THETA_0)      # |z - 350| >= 250 at levels <= 2 and >= 12
    assert th[7, 1] > bb.THETA_0 and th[7, 3] > bb.THETA_0 and np.all(th[7] <= bb.THETA_0 + 0.5)
    edge = np.array([[500.0 + 250.0, 500.0, 0.0]])
    assert bb.theta_init(edge, 7, nk)[0] == bb.THETA_0                        # r = 250 exactly
    for k in (0, 7, 29):
        assert np.array_equal(bb.rt_init(x, k, nk), bb.rho_init(x, k, nk) * bb.theta_init(x, k, nk))
    uq, r2, t2, e2 = bb.layer_fields(nk, x)
    assert uq.shape == (nk, 4, 2) and not uq.any() and r2.shape == t2.shape == e2.shape == (nk, 4)
    assert np.array_equal(t2[7], bb.rt_init(x, 7, nk)) and np.array_equal(e2[3], bb.exner_init(x, 3, nk))
    lev = bb.levels(nk, x)
    assert lev.shape == (nk + 1, 4) and np.array_equal(lev[:, 0], z)
    # other parameters than the reference's
    assert bb.z_at_level(x, 4, nk=6, ztop=1200.0)[0] == 800.0 and bb.theta_init(np.array([[30.0, 30.0, 0.0]]), 1, nk=4, ztop=1400.0, lx=60.0)[0] == 300.5


# ---- the restated step: what each box feature is worth -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def steps(oracle):
    c = bc.make_case(oracle)

    def run(lose):
        R, st, out = bc.BoxRestatement(c, lose=lose), c["state"], []
        for _ in range(2):
            st = R.step(*st)
            out.append(st)
        return out, R
    c["run"] = run
    c["ref"], c["R"] = run(None)
    return c


def test_restated_step_is_sane(steps):
    """36 units of 16 lanes (the last block partial), the seeded upwinding at UPWIND, finite fields that stay in the range of the upwinding"""
    from tests import box_schur2_case as bs
    c, P = steps, steps["P"]
    assert P.nEl * c["nk"] == 36 and abs(bs.max_upwind(P, c["state"][1], 0.25 * bc.DT) - bc.UPWIND) < 1e-12
    for st in c["ref"]:
        assert all(np.isfinite(a).all() for a in st) and bs.max_upwind(P, st[1], 0.25 * bc.DT) < 0.5
    d = c["R"].diagnostics(c["ref"][1])
    assert set(d) == {"keh", "kev", "pe", "ie", "k2p", "p2k", "k2i", "i2k", "k2i_z", "i2k_z", "mass", "entr"}
    assert all(np.isfinite(v[0]) for v in d.values()) and d["k2i"][0] != 0.0 and d["k2i_z"][0] != 0.0
    # the entropy is that of stage 1's theta_0, not of the new state
    th_new = bc.theta_up(c, *(bc.sc.to_vert(c, a) for a in c["ref"][1][2:4]), c["ref"][1][1], bc.DT)
    assert abs(bc.entropy(c, th_new)[0] - d["entr"][0]) > 1e-12 * d["entr"][1]


@pytest.mark.parametrize("lose,step,field", [("uuz_first", 1, "velz"), ("leapfrog", 2, "velx"), ("dwdx", 1, "velx"), ("theta_up", 1, "velz"),
                                             ("kinetic", 1, "velx")])
def test_each_box_feature_moves_its_field(steps, lose, step, field):
    """the restatement without ONE feature of the box step differs from the full one, in the field that feature acts on first, by at least
    100 x the bar the device step is held to in that field"""
    got, _ = steps["run"](lose)
    i = bc.FIELDS.index(field)
    moved = {n: rel_l2(g, w) for n, g, w in zip(bc.FIELDS, got[step - 1], steps["ref"][step - 1])}
    print("without %s, step %d: %s" % (lose, step, "  ".join("%s %.2e" % kv for kv in moved.items())))
    assert moved[field] >= 100.0 * bc.BARS[step][field], (lose, field, moved[field], bc.BARS[step][field])
    if lose == "leapfrog":                                                   # the first step has no leapfrog to lose
        assert all(np.array_equal(g, w) for g, w in zip(got[0], steps["ref"][0]))
