"""The analytic rising-bubble case of box/Bubble.cpp:24-90: a neutrally stratified atmosphere at rest in a doubly periodic box with a
warm sphere of 250 m radius, as numpy functions over points x [n, 3] (x, y in the box of side lx; the third coordinate is not used: the
height comes from the level index).

The reference fixes NK, ZTOP, _LX and THETA_0 in macros (:24-32); here they are the parameters `nk`, `ztop`, `lx` and `theta_0` with the
reference's values as defaults.  Level indices are integers.  Every function takes the index `ki` as z_at_level does -- the reference hands
init2 the LAYER index, so the layer fields rho, rt and exner are evaluated at the height of the layer's lower interface, ki ztop / nk
(:181-183 with Euler::init2, box/Euler_2.cpp:800); that is kept.

The layers have one thickness, ztop / nk, which is what BoxHorizSolve demands.  ki (ztop / nk) is formed as the reference forms it; where
ztop / nk is not a binary fraction the differences of neighbouring levels round differently and the uniform-layer check (1e-14 relative) can
refuse the mesh: choose nk so that ztop / nk is exact (the defaults are: 10 m)."""
import numpy as np

NK = 150                       # box/Bubble.cpp:24
ZTOP = 1500.0                  # :25
GRAVITY = 9.80616              # :26
CP = 1004.5                    # :27
CV = 717.5                     # :28
RD = 287.0                     # :29
P0 = 100000.0                  # :30
LX = 1000.0                    # :31
THETA_0 = 300.0                # :32
RADIUS = 250.0                 # :59
Z_CENTRE = 350.0               # :54
AMPLITUDE = 0.25               # :59: theta' = AMPLITUDE (1 + cos(pi r / RADIUS)), 0.5 K at the centre


def _x(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(1, -1) if x.ndim == 1 else x


def z_at_level(x, ki, nk=NK, ztop=ZTOP):
    """:40-42: the height of interface ki, the same at every point"""
    return np.full(_x(x).shape[0], ki * (ztop / nk))


def pres(x, ki, nk=NK, ztop=ZTOP, theta_0=THETA_0):
    """:44-48: the hydrostatic pressure of the atmosphere of constant potential temperature theta_0"""
    z = z_at_level(x, ki, nk, ztop)
    return P0 * np.power(1.0 - GRAVITY * z / (CP * theta_0), CP / RD)


def theta_init(x, ki, nk=NK, ztop=ZTOP, lx=LX, theta_0=THETA_0):
    """:50-62: theta_0 plus the bubble, exactly theta_0 where r >= RADIUS"""
    x = _x(x)
    xi, yi, zi = x[:, 0] - 0.5 * lx, x[:, 1] - 0.5 * lx, z_at_level(x, ki, nk, ztop) - Z_CENTRE
    r = np.sqrt(xi * xi + yi * yi + zi * zi)
    return np.where(r < RADIUS, theta_0 + AMPLITUDE * (1.0 + np.cos(np.pi * r / RADIUS)), theta_0)


def u_init(x, ki, nk=NK):
    """:64-66"""
    return np.zeros(_x(x).shape[0])


def v_init(x, ki, nk=NK):
    """:68-70"""
    return np.zeros(_x(x).shape[0])


def exner_init(x, ki, nk=NK, ztop=ZTOP, theta_0=THETA_0):
    """:72-76"""
    return CP * np.power(pres(x, ki, nk, ztop, theta_0) / P0, RD / CP)


def rho_init(x, ki, nk=NK, ztop=ZTOP, theta_0=THETA_0):
    """:78-82: the density of the UNPERTURBED column from the equation of state"""
    return (P0 / (RD * theta_0)) * np.power(exner_init(x, ki, nk, ztop, theta_0) / CP, CV / RD)


def rt_init(x, ki, nk=NK, ztop=ZTOP, lx=LX, theta_0=THETA_0):
    """:84-86"""
    return rho_init(x, ki, nk, ztop, theta_0) * theta_init(x, ki, nk, ztop, lx, theta_0)


def f_topog(x):
    """:88-90"""
    return np.zeros(_x(x).shape[0])


def levels(nk, xq, ztop=ZTOP):
    """the interface heights Geom::initTopog(f_topog, z_at_level) leaves with the zero topography of this case: [nk+1, nq]"""
    xq = _x(xq)
    top, topog = z_at_level(xq[:1], nk, nk, ztop)[0], f_topog(xq)
    return np.stack([(top - topog) * z_at_level(xq, ki, nk, ztop) / top + topog for ki in range(nk + 1)])


def layer_fields(nk, xq, ztop=ZTOP, lx=LX, theta_0=THETA_0):
    """what the driver hands Euler::init1 / init2 (:180-183), in the shape of umjs14.layer_fields: uq [nk, nq, 2] (u_init, v_init
    interleaved per point) and rho, rt, exner [nk, nq] on the points xq"""
    lay = range(nk)
    uq = np.stack([np.stack([u_init(xq, k, nk), v_init(xq, k, nk)], axis=-1) for k in lay])
    return (uq, np.stack([rho_init(xq, k, nk, ztop, theta_0) for k in lay]), np.stack([rt_init(xq, k, nk, ztop, lx, theta_0) for k in lay]),
            np.stack([exner_init(xq, k, nk, ztop, theta_0) for k in lay]))
