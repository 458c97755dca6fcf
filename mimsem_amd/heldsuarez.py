"""The Held-Suarez case of eul/HeldSuarez.cpp (Held & Suarez 1994 forcing on the UMJS14 jet): the analytic state the driver hands
Euler::init1 / init2 (:313-322) and the run's constants.  The file is eul/UMJS14.cpp with these differences, and nothing else:

  :25        NK 16 (UMJS14: 30)
  :160, :177 the guard `if(gc > D0) return 0.0` of u_pert / v_pert is commented out: the wind perturbation is NOT cut beyond D0 (it decays
             with cos^3 of the scaled distance and changes sign there); the two 1e-4 m guards at the centre and its antipode stay (:157-158, :174-175)
  :275-277   dt = 120, nSteps = 100*24*30, dumpEvery = 2*24*30 -- 1 440 steps, two days; the comment there says 12 hours, the code counts
  :298       pe->hs_forcing = true (Euler(hs_forcing=True): temperature relaxation in solve_schur_2, M1 + M1ray friction)
  :352       pe->Strang (Euler.strang), where UMJS14 steps with Strang_ec

Every other function (:45-236: the jet, temperature, pressure, levels, theta / rho / rt / exner) is umjs14's line for line, so this module
binds umjs14's functions with cut=False and its own NK."""
from . import umjs14
from .umjs14 import D0, VP, ZT, ZTOP, exner_init, f_topog, rho_init, rt_init, theta_init  # noqa: F401  (the shared part of the case)

NK = 16                        # eul/HeldSuarez.cpp:25
DT = 120.0                     # :275
NSTEPS = 100 * 24 * 30         # :276  (72 000 steps: 100 days)
DUMP_EVERY = 2 * 24 * 30       # :277  (1 440 steps)
INTEGRATOR = "strang"          # :352


def u_pert(x, ki, nk=NK, vp=VP):
    """:147-163, without the cut at D0 (:160)"""
    return umjs14.u_pert(x, ki, nk, vp, cut=False)


def v_pert(x, ki, nk=NK, vp=VP):
    """:165-180, without the cut at D0 (:177)"""
    return umjs14.v_pert(x, ki, nk, vp, cut=False)


def u_init(x, ki, nk=NK, vp=VP):
    """:182-188"""
    return umjs14.u_init(x, ki, nk, vp, cut=False)


def v_init(x, ki, nk=NK, vp=VP):
    """:190-194"""
    return umjs14.v_init(x, ki, nk, vp, cut=False)


def levels(nk, xq):
    """umjs14.levels: :124-129 and Geom::initTopog with the zero topography (:234-236)"""
    return umjs14.levels(nk, xq)


def layer_fields(nk, xq, vp=VP):
    """what the driver hands Euler::init1 / init2 (:319-322), as umjs14.layer_fields with the uncut perturbation"""
    return umjs14.layer_fields(nk, xq, vp, cut=False)
