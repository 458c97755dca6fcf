"""tests/box_strang_case.py -- the cases and the numpy restatements behind the box twin's step: the point-wise form of the element-local momentum
forcing that csrc/momentum_forcing.inc is written from, and the box HorizSolve / Euler::Strang restated on the oracle's dense matrices.
TEST INFRASTRUCTURE ONLY: shared by tests/test_box_strang_cpu.py, tests/test_gpu_momentum_forcing.py, tests/test_gpu_box_horiz.py and
tests/test_gpu_box_strang.py; nothing in the product imports it.

Part 1, the forcing (mimsem_horiz_momentum_forcing):
    momentum_forcing_pointwise   one patch, one level, patch-local vectors: the three integrands summed at the quadrature point, ONE projection
    forcing_assembled            every patch and level of a case, scattered with ADD into the global slots
    forcing_dense                the same sum from GlobalDense.mat("ROTMAT" / "UHMAT" / "UTQWMAT", ...), term by term
    forcing_fields               seeded operands, each term scaled to the norm of the rotational one so that none hides in the sum

Part 2, the step (BoxHorizSolve, BoxEuler.strang):
    make_case        a uniform-layer one-patch periodic box, p = 3, ne = 3, nk = 4 (36 units of 16 lanes, 16 to a block: the last block is
                     partial) with the seeded state box_schur2_case.make_box draws: max |0.25 dt w| = UPWIND
    BoxOracle        box/HorizSolve.cpp on box_schur2_case.box_dense: viscosity, curl without Coriolis, diagnose_Phi (the intent: with the
                     kinetic term), and momentum_rhs / advection_rhs as functions beside it.  Dense LU stands for every KSPSolve
    newton2_box      the loop of box/VertSolve.cpp:1264-1458 with the horizontal forcing re-evaluated per iteration (:1333), written after
                     box_schur2_case.solve_schur_2_box (which has no forcing hook)
    BoxRestatement   Euler::Strang (box/Euler_2.cpp:1306-1477) stage by stage: the first-step uuz = 0, the leapfrog predictor, the entropy of
                     theta_0.  Both sides run a fixed NITS = 3 Newton iterations, no convergence test.  `lose` drops ONE box feature for the
                     sensitivity checks of tests/test_box_strang_cpu.py
"""
import numpy as np

from oracle.globalmat import Solver
from oracle.horiz_oracle import HorizOracle
from oracle.vert_oracle import _v10
from tests import box_schur2_case as bs
from tests import energetics_case as ec
from tests import schur2_case as s2
from tests import strang2_case as s2c
from tests import strang_case as sc
from tests import vort_diag_case as vc

SCALE = ec.SCALE
TERMS = ("rot", "pgf", "vor")


# ---- part 1: the element-local forcing ---------------------------------------------------------------------------------------------------
def momentum_forcing_pointwise(P, lev, nk, rot=None, pgf=None, vor=None, vert=False, scale=SCALE):
    """the point-wise form of
        R(q; lev, scale) a + F(th; lev, const_vert = vert) g + 1/2 sum_{i in {lev-1, lev}, 0 <= i <= nk-2} Rh(dz_i; scale) v_i
    (RotMat::assemble eul/Assembly.cpp:1051-1065, Uhmat::assemble :432-448, UtQWmat::assemble :1504-1517) on one patch: with t = thickInv,
    d = det, J the Jacobian, Q the weight, m = scale Q / d, G = J^T J, D = det J, (a_x, a_y), (g_x, g_y), (z_x, z_y)_i the local interpolants
    of a, g, dz_i (interp1_l), q the value of the 0-form at the point (interp0), h = interp2_g(th) (which holds the 1/d) and w_i the local
    interpolant of v_i (interp2_l),
        c = m t^2 q D (-a_y, a_x)  +  m t h (t if vert) G (g_x, g_y)  +  sum_i 1/2 m w_i / d  G (z_x, z_y)_i
        out_x[e] = Ut c_x, out_y[e] = Vt c_y, summed over the elements of the patch.
    rot = (q, a), pgf = (th, g): this level's patch-local vectors; vor = (dz [nk-1, n1], v [nk-1, n2]): the interface arrays, patch-local
    rows.  A term left None is absent.  Returns the patch-local 1-form vector"""
    U, V, Q = P.arr("U", (P.mp12, P.n1e)), P.arr("V", (P.mp12, P.n1e)), P.arr("Q", (P.mp12,))
    iq, ix, iy = P.elinds("q"), P.elinds("n1x"), P.elinds("n1y")
    ifc = [i for i in (lev - 1, lev) if 0 <= i <= nk - 2] if vor is not None else []
    out = np.zeros(P.n1)
    for e in range(P.nEl):
        ex, ey = e % P.nElsX, e // P.nElsX
        cx, cy = np.zeros(P.mp12), np.zeros(P.mp12)
        for q in range(P.mp12):
            px, py = q % P.mp1, q // P.mp1
            J = np.array(P.J[e, q]).reshape(2, 2); d = P.det[e, q]; ti = P.thickInv[lev, iq[e, q]]
            G = J.T @ J
            D = J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
            m = scale * Q[q] / d
            c = np.zeros(2)
            if rot is not None:
                qv = P.interp("0", ex, ey, px, py, rot[0])[0]
                a = P.interp("1l", ex, ey, px, py, rot[1])
                c += (m * ti * ti * qv * D) * np.array([-a[1], a[0]])
            if pgf is not None:
                h = P.interp("2g", ex, ey, px, py, pgf[0])[0]
                g = np.array(P.interp("1l", ex, ey, px, py, pgf[1]))
                c += (m * ti * h * (ti if vert else 1.0)) * (G @ g)
            for i in ifc:
                w = P.interp("2l", ex, ey, px, py, vor[1][i])[0]
                z = np.array(P.interp("1l", ex, ey, px, py, vor[0][i]))
                c += (0.5 * m * w / d) * (G @ z)
            cx[q], cy[q] = c
        np.add.at(out, ix[e], U.T @ cx)
        np.add.at(out, iy[e], V.T @ cy)
    return out


def _pick(F, terms):
    return {t: (F.get(t) if t in terms else None) for t in TERMS}


def forcing_assembled(gd, F, terms=TERMS, vert=False):
    """momentum_forcing_pointwise of every patch and level of a case, scattered with ADD into the global slots -> [nk, N1]; F: the dict of
    forcing_fields (global vectors)"""
    nk = F["nk"]
    S = _pick(F, terms)
    out = np.zeros((nk, gd.N1))
    for t, P in zip(gd.topos, gd.P):
        vor = None if S["vor"] is None else (np.stack([gd.l1(t, r) for r in S["vor"][0]]), np.stack([gd.l2(t, r) for r in S["vor"][1]]))
        for k in range(nk):
            rot = None if S["rot"] is None else (gd.l0(t, S["rot"][0][k]), gd.l1(t, S["rot"][1][k]))
            pgf = None if S["pgf"] is None else (gd.l2(t, S["pgf"][0][k]), gd.l1(t, S["pgf"][1][k]))
            np.add.at(out[k], t.loc1, momentum_forcing_pointwise(P, k, nk, rot, pgf, vor, vert))
    return out


def forcing_dense(gd, F, terms=TERMS, vert=False):
    """the same sum from the oracle's dense global matrices, as the reference's momentum_rhs applies them -> [nk, N1]"""
    nk = F["nk"]
    S = _pick(F, terms)
    out = np.zeros((nk, gd.N1))
    for k in range(nk):
        if S["rot"] is not None:
            out[k] += gd.mat("ROTMAT", k, 0, S["rot"][0][k]) @ S["rot"][1][k]
        if S["pgf"] is not None:
            out[k] += gd.mat("UHMAT", k, 1 if vert else 0, S["pgf"][0][k]) @ S["pgf"][1][k]
        if S["vor"] is not None:
            for i in (k - 1, k):
                if 0 <= i <= nk - 2:
                    out[k] += 0.5 * (gd.mat("UTQWMAT", 0, 0, S["vor"][0][i]) @ S["vor"][1][i])
    return out


def forcing_fields(gd, nk, seed, like):
    """seeded operands of the forcing on the global vectors of gd: rot = (q [nk, N0], a [nk, N1]), pgf = (th [nk, N2], g [nk, N1]),
    vor = (dz [nk-1, N1], v [nk-1, N2]), every row its own draw (a wrong level or interface index must show).  `like`: the case's physically
    scaled fields (u1, th, velz1 of energetics_case.state_fields).  q, th and dz are then scaled so that each term alone has the norm of the
    rotational one (from the dense matrices: the reference, not the code under test): no term is round-off of another in the summed checks"""
    r = np.random.default_rng(seed)
    u1, th, vz = like["u1"][:nk], like["th"][:nk], like["velz1"][:max(nk - 1, 0)]
    F = dict(nk=nk)
    F["rot"] = (1e-4 * r.uniform(0.5, 1.5, (nk, gd.N0)) * np.sign(r.standard_normal((nk, gd.N0))), u1 * (1 + 0.1 * r.standard_normal(u1.shape)))
    F["pgf"] = (th * (1 + 0.01 * r.standard_normal(th.shape)), r.standard_normal(u1.shape) * np.abs(u1).mean())
    if nk > 1:
        F["vor"] = (r.standard_normal((nk - 1, gd.N1)) * np.abs(u1).mean(), vz * (1 + 0.1 * r.standard_normal(vz.shape)))
        norms = {t: np.linalg.norm(forcing_dense(gd, F, (t,))) for t in TERMS}
        F["vor"] = (F["vor"][0] * (norms["rot"] / norms["vor"]), F["vor"][1])
    else:
        norms = {t: np.linalg.norm(forcing_dense(gd, F, (t,))) for t in ("rot", "pgf")}
    F["pgf"] = (F["pgf"][0] * (norms["rot"] / norms["pgf"]), F["pgf"][1])
    for pair in (F[t] for t in TERMS if t in F):
        for x in pair:
            x.setflags(write=False)
    return F


def sub_levels(F, nk):
    """the first nk levels (nk - 1 interfaces) of a field set"""
    G = dict(nk=nk, rot=tuple(x[:nk] for x in F["rot"]), pgf=tuple(x[:nk] for x in F["pgf"]))
    if nk > 1:
        G["vor"] = tuple(x[:nk - 1] for x in F["vor"])
    return G


def sphere_forcing_case(seed=71):
    """vort_diag_case.make_case(): p = 3, ne = 2, nk = 3 cubed sphere, a FULL Jacobian, thickness varying by point and level; 72 units of 16
    lanes, 16 to a block: the last block is partial"""
    c = vc.make_case()
    c["nk"] = vc.NK
    c["FF"] = forcing_fields(c["gd"], vc.NK, seed, c["F"])
    return c


def box_dense_of(c, pn, ne):
    """GlobalDense of a one-patch periodic box case of energetics_case.make_box_case (box_schur2_case.box_dense wants its own dict)"""
    from mimsem_amd.mesh import PeriodicBox
    (t, g, P), = c["patches"]
    return bs.box_dense(dict(bx=PeriodicBox(pn, ne, 1), topo=t, geom=g, P=P))


def box_forcing_case(oracle, pn=4, ne=3, nk=2, seed=72):
    """energetics_case.make_box_case: a doubly periodic box (diagonal Jacobian, edges that wrap around), levels perturbed per point.  The
    default p = 4 puts 25 points on 32 lanes; nk = 2 has one interface feeding both levels.  ne = 2: an element's two neighbours in a
    direction are the same element"""
    c = ec.make_box_case(oracle, pn=pn, ne=ne, nk=nk, seed=seed)
    c["gd"] = box_dense_of(c, pn, ne)
    c["FF"] = forcing_fields(c["gd"], nk, seed + 1, c["F"])
    return c


# ---- part 2: the step --------------------------------------------------------------------------------------------------------------------
PN, NE, NK = 3, 3, 4
DT, UPWIND, NITS = 0.01, bs.UPWIND, 3   # DT: that of box/Bubble.cpp:135; the horizontal sound-wave CFL number is 0.5 on make_case's sub-cells
DZ = 300.0                              # the one layer thickness (box_schur2_case.make_box: ztop = 300 nk, there perturbed)
LX = 120.0                              # make_case: the side of the box; det = (LX / (2 NE))^2 = 400
PERT, STRAT, U0 = 1.0e-4, 1.0e-2, 0.1   # relative noise of the hydrostatic state, rise of theta over the column, horizontal velocity in m/s
FIELDS = ("velx", "velz", "rho", "rt", "exner")
CAP = 1e-8
# the bars of a device step against BoxRestatement per field (tests/test_gpu_box_strang.py: relative L2; the error observed on an MI355X x 10,
# rounded up to a power of ten, none above CAP); the sensitivity conditions of tests/test_box_strang_cpu.py are stated against them.
# Observed (FUSED_FORCING True and False alike to the digits shown):
#              velx      velz      rho       rt        exner
#    step 1    1.16e-12  1.70e-13  1.43e-16  1.47e-16  4.08e-16
#    step 2    2.10e-12  2.48e-13  5.43e-16  5.55e-16  4.55e-16
# (velx: the horizontal pressure gradient of an exner field that is uniform to PERT is a difference of nearly equal numbers on both sides)
BARS = {1: dict(velx=1e-10, velz=1e-11, rho=1e-14, rt=1e-14, exner=1e-14),
        2: dict(velx=1e-10, velz=1e-11, rho=1e-14, rt=1e-14, exner=1e-14)}
LOSSES = ("uuz_first", "leapfrog", "dwdx", "theta_up", "kinetic")


def make_case(oracle, pn=PN, ne=NE, nk=NK, seed=None, uniform=True):
    """box_schur2_case.make_box with layers of ONE thickness (uniform=False: that very box with its perturbed levels, for the check that
    refuses them): a one-patch periodic box, a seeded vertical velocity of max_q |0.25 DT w| = UPWIND over the dofs (the reference upwinds
    with w NOT divided by det) and a seeded horizontal velocity; beside it the dense matrices and the state in strang()'s layouts.

    What differs from box_schur2_case.finish_case, whose state only ever met the vertical loop, and why.  That box has 0.2 m sub-cells
    (lx = 2 ne) and DT = 0.1: a horizontal sound-wave CFL number of ~150 for a step that is explicit in the horizontal, and a column out of
    hydrostatic balance -- the restated step ends in NaN within two steps.  Here: DT = 0.01 and lx = LX (7 m sub-cells: CFL 0.5; det = 400, so
    w ~ 0.3 m/s at UPWIND); schur2_case.hydrostatic_state (theta_0 = 300 K) with PERT relative noise and a potential temperature rising by
    STRAT over the column (an isentropic column would hide the upwinding of theta); 1-form dofs of U0 m/s (they carry the layer thickness:
    M1 has vert_scale)"""
    from mimsem_amd.geom import BoxGeom
    from mimsem_amd.mesh import PeriodicBox, box_coords
    from mimsem_amd.topo import Topo
    if not uniform:
        return bs.make_box(oracle, pn, ne, nk, seed)
    seed = 1000 + 100 * pn + 10 * ne + nk if seed is None else seed
    lx = LX
    bx = PeriodicBox(pn, ne, 1); coords = box_coords(pn, ne, lx)
    t = Topo(bx, 0, nk)
    g = BoxGeom(t, bx, coords, nk, lx)
    r = np.random.default_rng(seed)
    levs = np.outer(DZ * np.arange(nk + 1), np.ones(g.n0))
    g.set_levels(levs)
    P = oracle.Patch(pn, pn, bx.nel, nk)
    P.set_metric(g.det, g.J); P.set_levels(levs)
    st = s2.hydrostatic_state(P, g, theta0=300.0)
    n2 = P.n2e
    for n in ("rho", "rt", "exner"):
        st[n] = st[n] * (1.0 + PERT * r.standard_normal(st[n].shape))
    st["rt"] = st["rt"] * np.repeat(1.0 + STRAT * np.arange(nk) / nk, n2)[None, :]
    w = r.standard_normal(st["velz"].shape)
    st["velz"] = w * (UPWIND / bs.max_upwind(P, w, 0.25 * DT))
    c = dict(bx=bx, topo=t, geom=g, P=P, N1=bx.nDofs1G, st=st)
    c["ul"] = U0 * DZ * np.sqrt(P.det.mean()) * r.standard_normal((nk, bx.nDofs1G))
    gd = bs.box_dense(c)
    gd.E10 = gd._e10(); gd.E01 = -gd.E10.T                                             # (box_dense leaves the curl's incidence out)
    c.update(gd=gd, patches=[(t, g, P)], topos=[t], geoms=[g], nk=nk, levs=levs, lx=lx, coords=coords, zv_v=st["zv"])
    c["state"] = (c["ul"], st["velz"]) + tuple(s2c.to_horiz(c, st[n], nk) for n in ("rho", "rt", "exner"))
    for a in c["state"]:
        a.setflags(write=False)
    return c


class BoxOracle(HorizOracle):
    """box/HorizSolve.cpp on the dense global matrices of a one-patch box: HorizOracle's grad / curl / laplacian (no Coriolis term is ever added)
    with the box viscosity (:106-114) and without the Coriolis set-up.  M1, M2, M0 per level: on uniform layers the level-0 matrices the
    reference assembles once"""

    def __init__(self, gd, lx, do_visc=True, kinetic=True):
        self.g, self.nk, self.do_visc, self.kinetic = gd, gd.nk, do_visc, kinetic
        self._solve = Solver(False)
        self.del2 = -np.sqrt(2.0 * 0.072 * np.sqrt(lx * lx / gd.N0) ** 3.2)
        self.M1 = [gd.mat("UMAT", k, 1) for k in range(self.nk)]
        self.M2 = [gd.mat("WMAT", k, 1) for k in range(self.nk)]
        self.M0 = [gd.mat("PMAT", k, 0) for k in range(self.nk)]
        self.fg = None

    def diagnose_Phi(self, lev, u1, u2, velz1, velz2):
        """:326-380 with the evident intent of its kinetic part (the commented-out K->assemble form :336-349 = the sphere's); kinetic=False:
        the reference as written, whose Wvec::assemble_K multiplies a zeroed table (box/Assembly.cpp:2994-3005)"""
        full = super().diagnose_Phi(lev, u1, u2, velz1, velz2)
        if self.kinetic:
            return full
        g = self.g
        K1 = g.mat("WTQUMAT", lev, 0, u1)
        return full - ((1.0 / 3.0) * (K1 @ u1) + (1.0 / 3.0) * (K1 @ u2) + (1.0 / 3.0) * (g.mat("WTQUMAT", lev, 0, u2) @ u2))


def momentum_rhs(hz, lev, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, Fz=None, dwdx1=None, dwdx2=None, Fk=None):
    """box/HorizSolve.cpp:412-526; theta [nk+1, N2] on the interfaces, Pi and the velocities this level's vectors, the rest [nk-1, .]
    interface arrays.  Returns fu, or with Fk (this level's mass flux) given (fu, k2i term, sum of |Fk . dp| entries / SCALE)"""
    g = hz.g
    theta_h = 0.5 * theta[lev] + 0.5 * theta[lev + 1]                                   # :428-430
    Phi = hz.diagnose_Phi(lev, velx1, velx2, velz1, velz2)
    dPi = hz.grad(Pi, lev)
    w = 0.5 * (hz.curl(velx1, lev) + hz.curl(velx2, lev))                               # diagnose_wxu :391-394
    uh = 0.5 * velx1 + 0.5 * velx2
    fu = g.E12 @ Phi + g.mat("ROTMAT", lev, 0, w) @ uh                                  # :439-440
    dp = g.mat("UHMAT", lev, 0, theta_h) @ dPi                                          # :443-445
    fu = fu + dp
    for il in ((lev - 1,) if lev > 0 else ()) + ((lev,) if lev < hz.nk - 1 else ()):    # :454-501
        v = Fz[il] if Fz is not None else 0.5 * velz1[il] + 0.5 * velz2[il]
        t = g.mat("UTQWMAT", 0, 0, 0.5 * dudz1[il] + 0.5 * dudz2[il]) @ v
        if Fz is not None and dwdx1 is not None:
            t = t - g.mat("UTQWMAT", 0, 0, 0.5 * dwdx1[il] + 0.5 * dwdx2[il]) @ v
        fu = fu + 0.5 * t
    if hz.do_visc:
        fu = fu + hz.M1[lev] @ hz.laplacian(hz.laplacian(uh, lev), lev)                 # :503-513
    if Fk is None:
        return fu
    return fu, float(Fk @ dp) / SCALE, float(np.abs(Fk * dp).sum()) / SCALE


def momentum_rhs_all(hz, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, Fz=None, dwdx1=None, dwdx2=None, Fk=None):
    """every level -> fu [nk, N1], or with Fk (fu, k2i, S_abs of k2i)"""
    out = [momentum_rhs(hz, k, theta, dudz1, dudz2, velz1, velz2, Pi[k], velx1[k], velx2[k], Fz, dwdx1, dwdx2, None if Fk is None else Fk[k])
           for k in range(hz.nk)]
    if Fk is None:
        return np.stack(out)
    return np.stack([o[0] for o in out]), sum(o[1] for o in out), sum(o[2] for o in out)


advection_rhs = s2c.advection_rhs        # :214-324 is the sphere's theta_in_Wt branch: (hz, u1, u2, h1, h2, theta) -> dF, dG, Fk, Gk


def theta_up(c, rho_v, rt_v, velz_v, dt):
    """Euler::diagTheta (box/Euler_2.cpp:543-565): the upwinded diagnosis over 0.25 dt -> [nEl, (nk+1) n2e]"""
    return bs.diag_theta2_up_all(c["P"], rho_v, rt_v, velz_v, 0.25 * dt)


def theta_lumped(c, rho_v, rt_v):
    P = c["P"]
    return np.stack([P.diag_theta2(e % P.nElsX, e // P.nElsX, rho_v[e], rt_v[e]) for e in range(P.nEl)])


def newton2_box(c, dt, velz_i, rho_i, rt_i, exner_i, zv, nits, forcing=None, udwdx=None, uuz=None, upwind=True):
    """`nits` iterations of box/VertSolve.cpp:1328-1418 for every column: box_schur2_case.solve_schur_2_box with forcing(rho_i, rho_j, theta_h)
    -> (dFx, dGx) in the vertical layout, HorizSolve::advection_rhs at the head of every iteration (:1333), added to dF_z / dG_z before the VB
    product.  Returns (velz, rho, rt, exner), theta_h, exner_h and (k2i_z, its S_abs) of the last iteration"""
    P = c["P"]
    nEl, nk, n2 = P.nEl, P.nk, P.n2e
    V10 = _v10(nk, n2)
    velz_j, rho_j, rt_j, exner_j = velz_i.copy(), rho_i.copy(), rt_i.copy(), exner_i.copy()
    theta = (lambda rho, rt, velz: theta_up(c, rho, rt, velz, dt)) if upwind else (lambda rho, rt, velz: theta_lumped(c, rho, rt))
    theta_i = theta(rho_i, rt_i, velz_i)
    theta_h = theta_i.copy()
    exner_h, velz_h, rho_h, rt_h = exner_i.copy(), velz_i.copy(), rho_i.copy(), rt_i.copy()
    uuz_j = None if udwdx is None else udwdx.copy()
    k2i = (0.0, 0.0)
    for _ in range(nits):
        dFx, dGx = forcing(rho_i, rho_j, theta_h) if forcing is not None else (None, None)
        ks, ka = 0.0, 0.0
        for e in range(nEl):
            ex, ey = e % P.nElsX, e // P.nElsX
            F_w, F_z, G_z, _, kk = s2.assemble_residual(P, ex, ey, dt, theta_h[e], exner_h[e], velz_i[e], velz_j[e], rho_i[e], rho_j[e], zv[e], V10, 0.0)
            ks += float(kk.sum()) / SCALE; ka += float(np.abs(kk).sum()) / SCALE
            if udwdx is not None:
                F_w = F_w + 0.5 * dt * udwdx[e] + 0.5 * dt * uuz_j[e]
            F_exner = P.eos_residual(ex, ey, rt_j[e], exner_j[e])
            VB = P.colop_dense("CONST", ex, ey)
            dF_z = rho_j[e] + dt * (V10 @ F_z) - rho_i[e]
            dG_z = rt_j[e] + dt * (V10 @ G_z) - rt_i[e]
            if dFx is not None:
                dF_z = dF_z + dt * dFx[e]
                dG_z = dG_z + dt * dGx[e]
            sol = P.solve_schur_column_3(ex, ey, dt, theta_h[e], velz_h[e], rho_h[e], rt_h[e], exner_h[e], F_w, VB @ dF_z, VB @ dG_z, F_exner, flags=3)
            velz_j[e] += sol["d_u"]; rho_j[e] += sol["d_rho"]; rt_j[e] += sol["d_rt"]; exner_j[e] += sol["d_pi"]
            exner_h[e] = 0.5 * exner_i[e] + 0.5 * exner_j[e]; velz_h[e] = 0.5 * velz_i[e] + 0.5 * velz_j[e]
            rho_h[e] = 0.5 * rho_i[e] + 0.5 * rho_j[e]; rt_h[e] = 0.5 * rt_i[e] + 0.5 * rt_j[e]
        k2i = (ks, ka)
        theta_h = 0.5 * theta(rho_j, rt_j, velz_j) + 0.5 * theta_i
        if udwdx is not None and uuz is not None:
            uuz_j = uuz(velz_j)
    return (velz_j, rho_j, rt_j, exner_j), theta_h, exner_h, k2i


def entropy(c, theta_v):
    """box/Euler_2.cpp:979-997 of theta [nEl, (nk+1) n2e] -> (CP sum_e sum_k lz_k sum_q Q_q log((W theta_k)_q), the sum of the magnitudes)"""
    P = c["P"]
    nk, n2 = P.nk, P.n2e
    W, Q = P.arr("W", (P.mp12, n2)), P.arr("Q", (P.mp12,))
    lz0 = P.thick[0, 0]                                                                 # geom->thick[0][0] :988
    terms = []
    for e in range(P.nEl):
        for k in range(nk + 1):
            lz = 0.5 * lz0 if k in (0, nk) else lz0
            terms.append(lz * (Q * np.log(W @ theta_v[e, k * n2:(k + 1) * n2])))
    terms = ec.CP * np.concatenate(terms)
    return float(terms.sum()), float(np.abs(terms).sum())


class BoxRestatement:
    """Euler::Strang of the box twin, stage by stage; carries first_step, u_prev / u_curr and uz / uz_prev between steps as the reference does.
    lose: one of LOSSES -- the restatement WITHOUT that feature of the box step:
      uuz_first  uuz = vert_mom_vort(velx, velz_0) on the first step too (the reference's is zero there)
      leapfrog   the forward predictor on every step
      dwdx       momentum_rhs without the dwdx part of the Rh coefficient
      theta_up   the lumped diagTheta2 of the eul/ step in stage 1 and in the Newton loop
      kinetic    diagnose_Phi as the reference is written: no kinetic term"""

    def __init__(self, c, dt=DT, nits=NITS, do_visc=False, lose=None):
        assert lose is None or lose in LOSSES
        self.c, self.gd, self.dt, self.nits, self.lose = c, c["gd"], dt, nits, lose
        self.hz = BoxOracle(c["gd"], c["lx"], do_visc=do_visc, kinetic=lose != "kinetic")
        self.first_step, self.u_prev, self.u_curr, self.uz, self.uz_prev = True, None, None, None, None

    def _mom(self, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, Fz, dwdx1, dwdx2, Fk=None):
        if self.lose == "dwdx":
            dwdx1 = dwdx2 = None
        return momentum_rhs_all(self.hz, theta, dudz1, dudz2, velz1, velz2, Pi, velx1, velx2, Fz, dwdx1, dwdx2, Fk)

    def _theta(self, rho_v, rt_v, velz_v):
        return theta_up(self.c, rho_v, rt_v, velz_v, self.dt) if self.lose != "theta_up" else theta_lumped(self.c, rho_v, rt_v)

    def stage1(self, velx, velz_v, velz_h0, rho, rt, exner):
        """:1337-1383 -> predictor velx; leaves theta_0 (vertical layout), uuz, Fu_1, dwdx1 and the carried vectors of this step"""
        c, gd, nk = self.c, self.gd, self.c["nk"]
        zero_uuz = self.first_step and self.lose != "uuz_first"
        self.uuz = np.zeros_like(velz_v) if zero_uuz else bs.vert_mom_vort(c, gd, velx, velz_v)       # :1337 (ul is zero on the first step)
        if not self.first_step:
            self.uz_prev = self.uz.copy()                                              # :1347-1349
        self.u_prev, self.u_curr = self.u_curr, velx.copy()                            # :1355-1356
        self.theta_0 = self._theta(sc.to_vert(c, rho), sc.to_vert(c, rt), velz_v)       # :1361
        theta_0 = s2c.to_horiz(c, self.theta_0, nk + 1)
        self.uz = vc.horiz_pot_vort(gd, velx, rho)[0]                                   # :1364
        self.dwdx1 = vc.vert_vort(gd, velz_h0, rho)[0]                                  # :1365
        if self.first_step:
            self.uz_prev = self.uz.copy()                                              # :1366
        Fz = vc.vert_mass_flux(gd, velz_h0, velz_h0, rho, rho)                          # :1367
        self.Fu_1 = self._mom(theta_0, self.uz, self.uz, velz_h0, velz_h0, exner, velx, velx, Fz, self.dwdx1, self.dwdx1)
        if self.first_step or self.lose == "leapfrog":
            return sc.momentum_update(None, self.hz.M1, self.dt, velx, self.Fu_1, 1.0)                # :1372-1374
        return sc.momentum_update(None, self.hz.M1, self.dt, self.u_prev, self.Fu_1, 2.0)             # :1375-1378 (leapfrog)

    def stage2(self, velx_0, velx_p, velz_v, rho, rt, exner):
        """:1392 -> (velz, rho, rt, exner) of the new time level in the vertical layout; leaves theta_h [nk+1, N2], exner_h (horizontal), k2i_z"""
        c, gd, nk = self.c, self.gd, self.c["nk"]
        self.Fk = None

        def forcing(rho_i, rho_j, theta_h):
            dF, dG, self.Fk, _ = advection_rhs(self.hz, velx_0, velx_p, rho, sc.to_horiz(c, rho_j, nk), s2c.to_horiz(c, theta_h, nk + 1))
            return sc.to_vert(c, dF), sc.to_vert(c, dG)
        new, th, eh, self.k2i_z = newton2_box(c, self.dt, velz_v, sc.to_vert(c, rho), sc.to_vert(c, rt), sc.to_vert(c, exner), c["zv_v"], self.nits,
                                              forcing=forcing, udwdx=self.uuz, uuz=lambda velz_j: bs.vert_mom_vort(c, gd, velx_p, velz_j),
                                              upwind=self.lose != "theta_up")
        self.theta_h, self.exner_h = s2c.to_horiz(c, th, nk + 1), sc.to_horiz(c, eh, nk)
        return new

    def stage3(self, velx_0, velx_p, velz_h0, velz_hn, rho_0, rho_n):
        """:1399-1413 -> the corrected velx; leaves k2i"""
        gd = self.gd
        self.uz = vc.horiz_pot_vort(gd, velx_p, rho_n)[0]                               # :1399
        Fz = vc.vert_mass_flux(gd, velz_h0, velz_hn, rho_0, rho_n)                      # :1400
        dwdx2 = vc.vert_vort(gd, velz_hn, rho_n)[0]                                     # :1401
        self.Fu_3, k2i, k2i_abs = self._mom(self.theta_h, self.uz, self.uz_prev, velz_hn, velz_h0, self.exner_h, velx_0, velx_p,
                                            Fz, self.dwdx1, dwdx2, Fk=self.Fk)
        self.k2i = (k2i, k2i_abs)
        return sc.momentum_update(None, self.hz.M1, self.dt, velx_0, self.Fu_3, 1.0)

    def step(self, velx, velz_v, rho, rt, exner):
        c, nk = self.c, self.c["nk"]
        velz_h0 = sc.to_horiz(c, velz_v, nk - 1)
        self.velx_p = self.stage1(velx, velz_v, velz_h0, rho, rt, exner)
        velz_n, rho_nv, rt_nv, exner_nv = self.stage2(velx, self.velx_p, velz_v, rho, rt, exner)
        rho_n, rt_n, exner_n = (sc.to_horiz(c, a, nk) for a in (rho_nv, rt_nv, exner_nv))
        velx_n = self.stage3(velx, self.velx_p, velz_h0, sc.to_horiz(c, velz_n, nk - 1), rho, rho_n)
        self.first_step = False
        return velx_n, velz_n, rho_n, rt_n, exner_n

    def diagnostics(self, state):
        """{name: (value, S_abs)} of the twelve numbers of box/Euler_2.cpp:887-1026 after a step that ended in `state`: the eight sums of
        tests/energetics_case.py, k2i and k2i_z of the step, i2k = i2k_z = 0 and the box entropy of stage 1's theta_0"""
        out = sc.energetics(self.c, state)
        out.update(k2i=self.k2i, k2i_z=self.k2i_z, i2k=(0.0, 0.0), i2k_z=(0.0, 0.0), entr=entropy(self.c, self.theta_0))
        return out
