"""The analytic baroclinic-wave case of eul/UMJS14.cpp:24-236 (Ullrich, Melvin, Jablonowski & Staniforth 2014, the deep-atmosphere
test without the deep terms the reference leaves out): the balanced zonal jet, its temperature and pressure, and the localised stream-function
perturbation of the wind, as numpy functions over points x [n, 3] (Cartesian, on the sphere of radius RAD_EARTH).

The reference fixes the level count in a macro (NK 30, :25); here `nk` is a parameter of every function that takes a level index `ki`.
Level indices are integers: interfaces 0 .. nk for z_at_level / z_taper / u_pert / v_pert / theta_init, layers 0 .. nk-1 for the midpoint
forms u_init / v_init / rho_init / rt_init / exner_init.  `vp` is the amplitude of the perturbation (VP, :42); vp = 0 is the steady state.

Guards kept from the reference (:157-160, :174-177): u_pert / v_pert are exactly 0 within 1e-4 m of the perturbation centre and of its
antipode and where the great-circle distance exceeds D0; z_taper is exactly 0 above ZT (:135).  The vectorised forms evaluate the quotient
by sin(gc / a) on a masked denominator, so the guarded points give 0 and not 0/0; the argument of acos in gc_dist is clipped to [-1, 1]
(at the centre it rounds to 1 + 2^-52, where the scalar acos of the reference returns NaN and every guard compares false)."""
import numpy as np

RAD_EARTH = 6371220.0          # eul/UMJS14.cpp:24
NK = 30                        # :25 (the default of `nk`)
P0 = 100000.0                  # :26
RD = 287.0                     # :27
GAMMA = 0.005                  # :28 (again :37)
GRAVITY = 9.80616              # :29
OMEGA = 7.29212e-5             # :30
CP = 1004.5                    # :31
CV = 717.5                     # :32
TE = 310.0                     # :33
TP = 240.0                     # :34
T0 = 0.5 * (TE + TP)           # :35
KP = 3.0                       # :36
ZT = 15000.0                   # :38
ZTOP = 30000.0                 # :39
LAMBDA_C = np.pi / 9.0         # :40
PHI_C = 2.0 * np.pi / 9.0      # :41
VP = 1.0                       # :42
D0 = RAD_EARTH / 6.0           # :43
MU = 15.0                      # :125 (mu of z_at_level)
GUARD = 1.0e-4                 # :157-158, :174-175


def _x(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(1, 3) if x.ndim == 1 else x


def _fac(r):
    """(r - a) / (b H) and its square (:48-51)"""
    H = RD * T0 / GRAVITY
    fac = (r - RAD_EARTH) / (2.0 * H)
    return fac * fac


def torr_1(r):
    """:45-54"""
    A, B, fac2 = 1.0 / GAMMA, (TE - TP) / ((TE + TP) * TP), _fac(r)
    return (A * GAMMA / T0) * np.exp(GAMMA * (r - RAD_EARTH) / T0) + B * (1.0 - 2.0 * fac2) * np.exp(-fac2)


def torr_2(r):
    """:56-64"""
    C, fac2 = 0.5 * (KP + 2.0) * (TE - TP) / (TE * TP), _fac(r)
    return C * (1.0 - 2.0 * fac2) * np.exp(-fac2)


def int_torr_1(r):
    """:66-75"""
    A, B, fac2 = 1.0 / GAMMA, (TE - TP) / ((TE + TP) * TP), _fac(r)
    return A * (np.exp(GAMMA * (r - RAD_EARTH) / T0) - 1.0) + B * (r - RAD_EARTH) * np.exp(-fac2)


def int_torr_2(r):
    """:77-85"""
    C, fac2 = 0.5 * (KP + 2.0) * (TE - TP) / (TE * TP), _fac(r)
    return C * (r - RAD_EARTH) * np.exp(-fac2)


def _lat(x):
    return np.arcsin(_x(x)[:, 2] / RAD_EARTH)


def _lon(x):
    x = _x(x)
    return np.arctan2(x[:, 1], x[:, 0])


def _cos_fac(cp):
    """cos^K - K / (K + 2) cos^(K+2) (:92-94, :105-107)"""
    return np.power(cp, KP) - (KP / (KP + 2.0)) * np.power(cp, KP + 2.0)


def temp(x, r):
    """:87-98; r: distance from the centre of the sphere, scalar or [n]"""
    Tinv = torr_1(r) - torr_2(r) * _cos_fac(np.cos(_lat(x)))
    return 1.0 / Tinv


def pres(x, r):
    """:100-110"""
    fac = _cos_fac(np.cos(_lat(x)))
    return P0 * np.exp(-GRAVITY * int_torr_1(r) / RD + GRAVITY * int_torr_2(r) * fac / RD)


def u_mean(x, r):
    """:112-122"""
    cp = np.cos(_lat(x))
    U = (GRAVITY * KP / RAD_EARTH) * int_torr_2(r) * (np.power(cp, KP - 1.0) - np.power(cp, KP + 1.0)) * temp(x, r)
    return -OMEGA * RAD_EARTH * cp + np.sqrt(OMEGA * OMEGA * RAD_EARTH * RAD_EARTH * cp * cp + RAD_EARTH * cp * U)


def z_at_level(x, ki, nk=NK):
    """:124-129: the height of interface ki, the same at every point"""
    frac = (1.0 * ki) / nk
    z = ZTOP * (np.sqrt(MU * frac * frac + 1.0) - 1.0) / (np.sqrt(MU + 1.0) - 1.0)
    return np.full(_x(x).shape[0], z)


def z_taper(x, ki, nk=NK):
    """:131-138"""
    z = z_at_level(x, ki, nk)
    frac = z / ZT
    return np.where(z > ZT, 0.0, 1.0 - 3.0 * frac * frac + 2.0 * frac * frac * frac)


def gc_dist(x):
    """:140-145: great-circle distance from the perturbation centre"""
    phi, lam = _lat(x), _lon(x)
    c = np.sin(PHI_C) * np.sin(phi) + np.cos(PHI_C) * np.cos(phi) * np.cos(lam - LAMBDA_C)
    return RAD_EARTH * np.arccos(np.clip(c, -1.0, 1.0))


def _pert(x, ki, nk, vp, fac, sign, cut=True):
    """cut: the guard `if(gc > D0) return 0.0` (:160, :177), which eul/HeldSuarez.cpp has commented out (mimsem_amd/heldsuarez.py: cut=False)"""
    gc = gc_dist(x)
    theta = 0.5 * np.pi * gc / D0
    ct, st = np.cos(theta), np.sin(theta)
    zero = (np.abs(gc - 0.0) < GUARD) | (np.abs(gc - RAD_EARTH * np.pi) < GUARD)
    if cut:
        zero = zero | (gc > D0)
    s = np.where(zero, 1.0, np.sin(gc / RAD_EARTH))
    val = sign * 16.0 * vp * z_taper(x, ki, nk) / (3.0 * np.sqrt(3.0)) * ct * ct * ct * st * fac / s
    return np.where(zero, 0.0, val)


def u_pert(x, ki, nk=NK, vp=VP, cut=True):
    """:147-163"""
    phi, lam = _lat(x), _lon(x)
    fac = -np.sin(PHI_C) * np.cos(phi) + np.cos(PHI_C) * np.sin(phi) * np.cos(lam - LAMBDA_C)
    return _pert(x, ki, nk, vp, fac, -1.0, cut)


def v_pert(x, ki, nk=NK, vp=VP, cut=True):
    """:165-180"""
    fac = np.cos(PHI_C) * np.sin(_lon(x) - LAMBDA_C)
    return _pert(x, ki, nk, vp, fac, +1.0, cut)


def _z_mid(x, ki, nk):
    return 0.5 * (z_at_level(x, ki, nk) + z_at_level(x, ki + 1, nk))


def u_init(x, ki, nk=NK, vp=VP, cut=True):
    """:182-188: the jet at the mean height of layer ki plus the mean of the two interface perturbations"""
    um = u_mean(x, _z_mid(x, ki, nk) + RAD_EARTH)
    return um + 0.5 * (u_pert(x, ki, nk, vp, cut) + u_pert(x, ki + 1, nk, vp, cut))


def v_init(x, ki, nk=NK, vp=VP, cut=True):
    """:190-194"""
    return 0.5 * (v_pert(x, ki, nk, vp, cut) + v_pert(x, ki + 1, nk, vp, cut))


def theta_init(x, ki, nk=NK):
    """:196-202: potential temperature at interface ki"""
    r = z_at_level(x, ki, nk) + RAD_EARTH
    return temp(x, r) * np.power(P0 / pres(x, r), RD / CP)


def rho_init(x, ki, nk=NK):
    """:204-210: density at the mean height of layer ki"""
    r = _z_mid(x, ki, nk) + RAD_EARTH
    return pres(x, r) / (RD * temp(x, r))


def rt_init(x, ki, nk=NK):
    """:212-217: rho times the mean of the two interface values of theta"""
    return rho_init(x, ki, nk) * (0.5 * (theta_init(x, ki, nk) + theta_init(x, ki + 1, nk)))


def exner_init(x, ki, nk=NK):
    """:219-224"""
    r = _z_mid(x, ki, nk) + RAD_EARTH
    return CP * np.power(pres(x, r) / P0, RD / CP)


def f_topog(x):
    """:234-236"""
    return np.zeros(_x(x).shape[0])


def levels(nk, xq):
    """the interface heights Geom::initTopog(f_topog, z_at_level) leaves in Geom::levs (eul/Geom.cpp:743-757) with the zero topography
    of this case: [nk+1, nq]"""
    xq = _x(xq)
    top, topog = z_at_level(xq[:1], nk, nk)[0], f_topog(xq)
    return np.stack([(top - topog) * z_at_level(xq, ki, nk) / top + topog for ki in range(nk + 1)])


def layer_fields(nk, xq, vp=VP, cut=True):
    """what the driver hands Euler::init1 / init2 (:319-322): uq [nk, nq, 2] (u_init, v_init interleaved per point, eul/Euler_2.cpp:454-455)
    and rho, rt, exner [nk, nq] on the points xq"""
    lay = range(nk)
    uq = np.stack([np.stack([u_init(xq, k, nk, vp, cut), v_init(xq, k, nk, vp, cut)], axis=-1) for k in lay])
    return (uq, np.stack([rho_init(xq, k, nk) for k in lay]), np.stack([rt_init(xq, k, nk) for k in lay]),
            np.stack([exner_init(xq, k, nk) for k in lay]))
