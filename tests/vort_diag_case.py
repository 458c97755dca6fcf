"""The case and the dense restatement shared by tests/test_vort_diag_cpu.py and tests/test_gpu_vort_diag.py: the p = 3, ne = 2, nk = 3 cubed
sphere of test_horizsolve_right_hand_sides (tests/test_gpu_next_rows.py) with the z_levels of tests/helpers.py (thickness varies
horizontally and by level), its physically scaled random fields, and Euler::HorizPotVort (eul/Euler_2.cpp:1051-1101),
HorizSolve::diagVertVort (eul/HorizSolve.cpp:823-861) and Euler::VertMassFlux (eul/Euler_2.cpp:1559-1572) restated on the oracle's dense
global matrices (oracle/horiz_oracle.py GlobalDense) and dense column matrices (the diagnose_F_z line of oracle/vert_oracle.py)."""
import numpy as np

from tests.helpers import z_levels

PN, NE, NK = 3, 2, 3


def make_case(seed=31):
    """mesh, dense global matrices and fields (numpy, global numbering); the oracle library must be built (the `oracle` fixture)"""
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.topo import Topo
    from oracle import horiz_oracle as ho
    cs = CubedSphere(PN, NE, 6); coords = sphere_coords(PN, NE)
    topos = [Topo(cs, p, NK) for p in range(6)]
    geoms = [Geom(t, cs, coords, NK) for t in topos]
    levs = z_levels(NK, geoms[0].n0)
    for g in geoms:
        g.set_levels(levs)
    gd = ho.GlobalDense(cs, topos, geoms, coords, levs)
    r = np.random.default_rng(seed)
    area = np.mean([P.det.mean() for P in gd.P]) * 4.0 / (PN * PN); dz = np.mean([P.thick.mean() for P in gd.P]); ln = np.sqrt(area)
    N1, N2 = gd.N1, gd.N2
    F = dict(area=area, dz=dz, ln=ln)
    F["u1"] = r.standard_normal((NK, N1)) * 20.0 * ln * dz; F["u2"] = F["u1"] * (1 + 0.05 * r.standard_normal((NK, N1)))
    F["h1"] = r.uniform(0.8, 1.2, (NK, N2)) * area * dz; F["h2"] = F["h1"] * (1 + 0.01 * r.standard_normal((NK, N2)))
    F["th"] = r.uniform(290, 310, (NK, N2)) * area * dz; F["Pi"] = r.uniform(900, 1000, (NK, N2)) * area * dz
    F["velz1"] = r.standard_normal((NK - 1, N2)) * area; F["velz2"] = F["velz1"] * (1 + 0.05 * r.standard_normal((NK - 1, N2)))
    return dict(cs=cs, coords=coords, topos=topos, geoms=geoms, levs=levs, gd=gd, ho=ho, F=F)


def rho_bar(rho):
    """rho_h of every interface, 0.5 a + 0.5 b"""
    return 0.5 * rho[:-1] + 0.5 * rho[1:]


def rho_bar_two_axpy(rho):
    """VecZeroEntries(rho_h); VecAXPY(rho_h, 0.5, rho[i]); VecAXPY(rho_h, 0.5, rho[i+1])"""
    out = np.zeros((rho.shape[0] - 1, rho.shape[1]))
    for i in range(rho.shape[0] - 1):
        out[i] += 0.5 * rho[i]
        out[i] += 0.5 * rho[i + 1]
    return out


def horiz_pot_vort(gd, velx, rho):
    """-> uz [nk-1, N1] and the relative residual of every solve"""
    nk = velx.shape[0]
    Mu = [gd.mat("UMAT", k, flag=1) @ velx[k] for k in range(nk)]            # M1->assemble(k, SCALE, true)
    rb = rho_bar(rho)
    uz, res = np.zeros((nk - 1, gd.N1)), []
    for i in range(nk - 1):
        du = Mu[i + 1] - Mu[i]
        A = gd.mat("UTMAT_H", i, field=rb[i])                                 # M1t->assemble_h(i, SCALE, rho_h)
        uz[i] = np.linalg.solve(A, du)
        res.append(np.linalg.norm(A @ uz[i] - du) / np.linalg.norm(du))
    return uz, res


def vert_vort(gd, velz, rho):
    """-> dwdx [nk-1, N1] and the relative residual of every solve; M2 and F at level 0 for every interface, as the reference has it"""
    ni = velz.shape[0]
    M2 = gd.mat("WMAT", 0, flag=1)                                            # M2->assemble(0, SCALE, true)
    rb = rho_bar(rho)
    dwdx, res = np.zeros((ni, gd.N1)), []
    for i in range(ni):
        A = gd.mat("UHMAT", 0, flag=0, field=rb[i])                           # F->assemble(rho_h, 0, false, SCALE)
        rhs = gd.E12 @ (M2 @ velz[i])
        dwdx[i] = np.linalg.solve(A, rhs)
        res.append(np.linalg.norm(A @ dwdx[i] - rhs) / np.linalg.norm(rhs))
    return dwdx, res


def vert_mass_flux(gd, velz1, velz2, rho1, rho2):
    """-> Fz [nk-1, N2]: per patch HorizToVert, per column the diagnose_F_z of oracle/vert_oracle.py (eul/VertSolve.cpp:237-260),
    VertToHoriz (interface fields ride in the first nk - 1 rows of an nk-row array)"""
    nk = rho1.shape[0]
    Fz = np.zeros((nk - 1, gd.N2))
    for t, P in zip(gd.topos, gd.P):
        own = t.pi * t.n2 + np.arange(t.n2)
        m = (nk - 1) * P.n2e
        lev = lambda a: P.horiz_to_vert(np.ascontiguousarray(a[:, own]))
        ifc = lambda a: P.horiz_to_vert(np.ascontiguousarray(np.vstack([a[:, own], np.zeros((1, t.n2))])))[:, :m]
        w1, w2, r1, r2 = ifc(velz1), ifc(velz2), lev(rho1), lev(rho2)
        Fv = np.zeros((P.nEl, nk * P.n2e))
        for e in range(P.nEl):
            ex, ey = e % P.nElsX, e // P.nElsX
            VAinv = P.colop_dense("LINEAR_INV", ex, ey)
            Fv[e, :m] = VAinv @ P.colop_dense("LINEAR_RT", ex, ey, flag=1, f1=r1[e]) @ (w1[e] / 3 + w2[e] / 6) + \
                VAinv @ P.colop_dense("LINEAR_RT", ex, ey, flag=1, f1=r2[e]) @ (w1[e] / 6 + w2[e] / 3)
        Fz[:, own] = P.vert_to_horiz(Fv)[:nk - 1]
    return Fz
