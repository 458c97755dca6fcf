"""The numpy restatement of the zonal-mean statistics (mimsem_amd/zonalstats.py, csrc/zonal_stats.inc) shared by
tests/test_zonal_stats_cpu.py and tests/test_gpu_zonal_stats.py.

point_fields()   the fields at every element's own quadrature points from the oracle's Geom::interp1_g / interp2_g, point by point, each
                 times 1 / thick of the level as Geom::write1 / write2(vert_scale = true) have it (tests/umjs14_case.py restate_quad_fields
                 states the dumps the same way): u, v, r, Theta, Pi [nk, nEl, mp12], elements patch by patch in the loop order ey, ex --
                 DeviceMesh's order -- and the weight a = Q_q det[e][q] [nEl, mp12]
moments()        T = Theta Pi / (CP r); the nine weighted products a {1, u, v, T, uu, vv, uv, vT, TT}; every (moment, level, band) entry
                 summed with math.fsum: the expected value is the correctly rounded sum of its terms and has no summation order of its own.
                 Returns beside it S_abs, the sum of the absolute values of the entry's terms: errors are taken relative to it.

`patches` is a list of (Topo, Geom, oracle Patch); vectors are global numpy arrays velx [nk, N1], rho, rt, exner [nk, N2]."""
import math

import numpy as np

from tests.energetics_case import _own, _patch_local_1form

CP = 1004.5                              # eul/Euler_2.cpp:29
MOMENTS = ("1", "u", "v", "T", "uu", "vv", "uv", "vT", "TT")
FIELDS = ("u", "v", "r", "Theta", "Pi")


def point_fields(patches, velx, rho, rt, exner):
    """-> ({name: [nk, nEl, mp12]} for FIELDS, weight [nEl, mp12])"""
    nk = velx.shape[0]
    vals, weight = [], []
    for t, g, P in patches:
        iq, own, Q = P.elinds("q"), _own(t), P.arr("Q", (P.mp12,))
        f = np.zeros((5, nk, P.nEl, P.mp12))
        for k in range(nk):
            ul = _patch_local_1form(t, P, velx[k])
            l2 = [np.ascontiguousarray(a[k, own]) for a in (rho, rt, exner)]
            for e in range(P.nEl):
                ex, ey = e % P.nElsX, e // P.nElsX
                for ii in range(P.mp12):
                    px, py = ii % P.mp1, ii // P.mp1
                    s = 1.0 / P.thick[k, iq[e, ii]]
                    uv = P.interp("1g", ex, ey, px, py, ul)
                    f[0, k, e, ii], f[1, k, e, ii] = uv[0] * s, uv[1] * s
                    for j, l in enumerate(l2):
                        f[2 + j, k, e, ii] = P.interp("2g", ex, ey, px, py, l)[0] * s
        vals.append(f)
        weight.append(Q[None, :] * np.array(P.det))
    f = np.concatenate(vals, axis=2)
    return {n: f[i] for i, n in enumerate(FIELDS)}, np.concatenate(weight)


def products(fields, weight):
    """the nine weighted products [9, nk, nEl, mp12]"""
    u, v = fields["u"], fields["v"]
    T = fields["Theta"] * fields["Pi"] / (CP * fields["r"])
    a = np.broadcast_to(weight, u.shape)
    return np.stack([a, a * u, a * v, a * T, a * (u * u), a * (v * v), a * (u * v), a * (v * T), a * (T * T)])


def moments(fields, weight, band, nb):
    """band [nEl, mp12] in [-1, nb) -> (S [9, nk, nb], S_abs [9, nk, nb]), every entry an fsum over the band's points"""
    prod = products(fields, weight)
    nm, nk = prod.shape[:2]
    flat = prod.reshape(nm, nk, -1)
    S, A = np.zeros((nm, nk, nb)), np.zeros((nm, nk, nb))
    for b in range(nb):
        idx = np.flatnonzero(np.asarray(band).reshape(-1) == b)
        for m in range(nm):
            for k in range(nk):
                terms = flat[m, k, idx].tolist()
                S[m, k, b] = math.fsum(terms)
                A[m, k, b] = math.fsum(abs(x) for x in terms)
    return S, A


def restate(patches, velx, rho, rt, exner, band, nb):
    fields, weight = point_fields(patches, velx, rho, rt, exner)
    return moments(fields, weight, band, nb)


def rel_err(got, want, s_abs):
    """max over the entries of |got - want| / S_abs (entries of empty bands, S_abs = 0, must match exactly and count as 0)"""
    got, want, s_abs = np.asarray(got), np.asarray(want), np.asarray(s_abs)
    empty = s_abs == 0.0
    assert np.array_equal(got[empty], want[empty]), "entries without terms differ"
    return float(np.max(np.abs(got - want)[~empty] / s_abs[~empty])) if (~empty).any() else 0.0


def latitudes(c):
    """latitude of every element's own quadrature points [nEl, mp12] of a case with "coords" and "geoms": what Euler takes as hs_lat"""
    out = []
    for g in c["geoms"]:
        x = c["coords"][g.loc0][g.all_inds0_l()]                                 # [nEl, mp12, 3]
        out.append(np.arcsin(x[..., 2] / np.linalg.norm(x, axis=-1)))
    return np.concatenate(out)
