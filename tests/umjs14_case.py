"""The case and the numpy restatements shared by tests/test_umjs14_cpu.py and tests/test_gpu_umjs14.py: the baroclinic-wave driver around
Euler.strang_ec (mimsem_amd/euler.py: init1, init2, initial_state, run, dump, load; mimsem_amd/umjs14.py).

Case: the p = 3 cubed sphere of tests/strang_case.py (ne = 2, six patches, 24 elements, nk = 4: the Rayleigh layer needs four levels) with the
stretched levels umjs14.levels(nk, xq) in place of tests/helpers.py::z_levels; ne = 4 (96 elements) for the projection quality and the
physical step, where no dense matrix is built.

Restatements (global numbering, numpy):
  init2            h_k = M2(k, SCALE, true)^-1 SCALE WtQ f_k, element by element: the oracle's WtQmat (Patch.project_from_quad) and dense LU of
                   the oracle's WMAT element matrices (eul/Euler_2.cpp:489-529)
  init1            u_k = M1(k, SCALE, true)^-1 SCALE UtQ uq_k with the dense M1 of tests/hmomentum_case.py (strang_case.DenseM1) and LU (:429-487)
  last_writer      the visiting order of Geom::write0 / write1 / write2 as a plain loop: patch by patch, ey, ex ascending, INSERT_VALUES
  quad_fields      Geom::write0 / write1 / write2 (eul/Geom.cpp:419-631): the oracle's interp0 / interp1_g / interp2_g point by point, the
                   thickness rule per field, the last value stored at a shared point wins"""
import numpy as np

from mimsem_amd import umjs14 as um

PN, NE, NK = 3, 2, 4
SCALE = 1.0e8
# (field of the dump, number of levels relative to nk, divided by the layer thickness)
QUAD_FIELDS = (("vorticity", 0, True), ("velocity_h_x", 0, True), ("velocity_h_y", 0, True), ("density", 0, True), ("rhoTheta", 0, True),
               ("exner", 0, True), ("theta", 1, False), ("velocity_z", -1, False))
VEC_FIELDS = (("velocity_h", 0), ("density", 0), ("rhoTheta", 0), ("exner", 0), ("velocity_z", -1), ("theta", 1))


def make_mesh(ne=NE, nk=NK):
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    cs = CubedSphere(PN, ne, 6); coords = sphere_coords(PN, ne)
    topos = [Topo(cs, p, nk) for p in range(6)]
    geoms = [Geom(t, cs, coords, nk) for t in topos]
    for g in geoms:
        g.set_levels(um.levels(nk, coords[g.loc0]))
    return dict(cs=cs, coords=coords, topos=topos, geoms=geoms, nk=nk, ne=ne)


def add_dense(c):
    """the oracle's patches and dense global matrices (the `oracle` fixture must have built the library)"""
    from oracle import horiz_oracle as ho
    levs = um.levels(c["nk"], c["coords"][c["geoms"][0].loc0])              # (no topography: the same heights at every point)
    c["gd"] = ho.GlobalDense(c["cs"], c["topos"], c["geoms"], c["coords"], levs)
    c["ho"] = ho
    c["patches"] = list(zip(c["topos"], c["geoms"], c["gd"].P))
    return c


def add_engine(c):
    from mimsem_amd.device import DeviceMesh, Engine
    c["eng"] = Engine(DeviceMesh(c["topos"], c["geoms"], nk=c["nk"], numbering="global"))
    dm = c["eng"].mesh
    assert np.array_equal(dm.gidq, np.arange(dm.nq))                        # every patch is there: slot = global quadrature id
    c["xq"] = c["coords"][dm.gidq]
    return c


def make_euler(c, dt, **kw):
    from mimsem_amd.euler import Euler
    return Euler(c["eng"], dt, um.levels(c["nk"], c["xq"]), c["xq"], **kw)


def _own(t):
    return t.pi * t.n2 + np.arange(t.n2)


def restate_init2(c, fq):
    """fq [nk, NQ] -> [nk, N2]"""
    out = np.zeros((c["nk"], c["gd"].N2))
    for t, g, P in c["patches"]:
        i2 = P.elinds("n2")
        for k in range(c["nk"]):
            b = SCALE * P.project_from_quad(0, np.ascontiguousarray(fq[k][g.loc0]))
            em = P.op_elmats("WMAT", k, SCALE, 1).reshape(P.nEl, P.n2e, P.n2e)
            h = np.zeros(P.n2)
            for e in range(P.nEl):
                h[i2[e]] = np.linalg.solve(em[e], b[i2[e]])
            out[k, _own(t)] = h
    return out


def restate_init1(c, uq):
    """uq [nk, NQ, 2] -> [nk, N1]"""
    from tests.strang_case import DenseM1
    dense = DenseM1(c)
    out = np.zeros((c["nk"], c["gd"].N1))
    for k in range(c["nk"]):
        b = np.zeros(c["gd"].N1)
        for t, g, P in c["patches"]:
            np.add.at(b, t.loc1, P.project_from_quad(2, np.ascontiguousarray(uq[k][g.loc0]).reshape(-1)))
        out[k] = np.linalg.solve(dense.m1(k), SCALE * b)
    return out


def restate_last_writer(topos, geoms):
    """the element-local point (flat index over elements patch by patch, then the element's points) whose value stays at every global
    quadrature point: a plain loop in the reference's visiting order, later stores overwriting earlier ones"""
    nq = int(max(g.loc0.max() for g in geoms)) + 1
    last, flat = np.full(nq, -1, dtype=np.int64), 0
    for t, g in zip(topos, geoms):
        inds = g.all_inds0_l()
        for ey in range(t.nElsX):
            for ex in range(t.nElsX):
                for ii in range(inds.shape[1]):
                    last[g.loc0[inds[ey * t.nElsX + ex, ii]]] = flat
                    flat += 1
    return last


def restate_quad_fields(c, state, theta, velz_h):
    """the fields of Euler.quad_fields from global numpy vectors: state = (velx [nk, N1], -, rho, rt, exner [nk, N2]), theta [nk+1, N2],
    velz_h [nk-1, N2].  Returns {name: [nlev, NQ]}"""
    gd, nk = c["gd"], c["nk"]
    hz = c["ho"].HorizOracle(gd)
    velx, _, rho, rt, exner = state
    vort = np.stack([hz.curl(velx[k], k) for k in range(nk)])
    src = {"vorticity": ("0", vort, 0, gd.l0), "velocity_h_x": ("1g", velx, 0, gd.l1), "velocity_h_y": ("1g", velx, 1, gd.l1),
           "density": ("2g", rho, 0, gd.l2), "rhoTheta": ("2g", rt, 0, gd.l2), "exner": ("2g", exner, 0, gd.l2),
           "theta": ("2g", theta, 0, gd.l2), "velocity_z": ("2g", velz_h, 0, gd.l2)}
    out = {}
    for name, _, thick in QUAD_FIELDS:
        kind, a, comp, loc = src[name]
        f = np.zeros((a.shape[0], gd.NQ))
        for t, g, P in c["patches"]:
            iq = P.elinds("q")
            for k in range(a.shape[0]):
                v = loc(t, a[k])
                for ey in range(P.nElsX):
                    for ex in range(P.nElsX):
                        for ii in range(P.mp12):
                            q = iq[ey * P.nElsX + ex, ii]
                            val = P.interp(kind, ex, ey, ii % P.mp1, ii // P.mp1, v)[comp]
                            if thick:
                                val *= 1.0 / P.thick[k, q]
                            f[k, g.loc0[q]] = val
        out[name] = f
    return out


def restate_theta2(c, rho, rt):
    """VertSolve::diagTheta2 of every column in the horizontal layout [nk+1, N2] (HorizToVert, per column, VertToHoriz:
    eul/Euler_2.cpp:1507-1509); the oracle's layout change takes nk rows, so the top interface comes from a second call on rows 1 .. nk"""
    nk = c["nk"]
    out = np.zeros((nk + 1, c["gd"].N2))
    for t, g, P in c["patches"]:
        own, n = _own(t), P.n2e
        rv, tv = P.horiz_to_vert(np.ascontiguousarray(rho[:, own])), P.horiz_to_vert(np.ascontiguousarray(rt[:, own]))
        th = np.stack([P.diag_theta2(e % P.nElsX, e // P.nElsX, rv[e], tv[e]) for e in range(P.nEl)])
        out[:nk, own] = P.vert_to_horiz(np.ascontiguousarray(th[:, :nk * n]))
        out[nk, own] = P.vert_to_horiz(np.ascontiguousarray(th[:, n:]))[-1]
    return out
