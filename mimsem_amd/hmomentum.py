"""The explicit horizontal momentum update that ends stages 1 and 3 of Euler::Strang_ec (eul/Euler_2.cpp:1431-1456, :1477-1492), every
level in one call of each kernel (the reference loops `for(kk...)` around assemble + MatMult + KSPSolve):

    M1->assemble(kk); bu = M1 u_a - c dt Fu;  if(hs_forcing) M1 += M1ray(kk, c dt, exner[kk], exner[0]);  KSPSolve(ksp1, bu, velx[kk])

With Held-Suarez forcing the system matrix M1 + M1ray(c dt) is ONE operator on the device (MIMSEM_OP_UMAT_FRIC) and the solve is
MassSolver.solve_fric; without it the solve is MassSolver.solve.  Single GPU, field layout as horizsolve.py: 1-forms [nk, n1], 2-forms [nk, n2]."""
from .horizsolve import ACCUM, SCALE, VERT


class HorizMomentum:
    def __init__(self, eng, horiz, dt, hs_forcing=False):
        """horiz: the HorizSolve whose 1-form mass solver (blocks, spectral bounds, check log) the update shares"""
        self.eng, self.m1, self.dt, self.hs_forcing = eng, horiz.m1, dt, hs_forcing
        if hasattr(eng, "halo"):
            raise NotImplementedError("HorizMomentum: sharded engines are not supported")

    def update(self, u_a, Fu, c, exner=None):
        """velx of  (M1 [+ M1ray(c dt, exner[k], exner[0])]) velx = M1 u_a - c dt Fu  on all levels; u_a, Fu [nk, n1], exner [nk, n2]"""
        eng, tau = self.eng, c * self.dt
        b = eng.combine(Fu, -tau)
        eng.apply("UMAT", u_a, lev0=0, scale=SCALE, flags=VERT | ACCUM, out=b)
        if not self.hs_forcing:
            return self.m1.solve(b)[0]
        if exner is None:
            raise ValueError("HorizMomentum.update: Held-Suarez forcing needs the exner field")
        return self.m1.solve_fric(b, tau, exner, exner[0])[0]

    def predictor(self, velx, u_prev, Fu, exner, first_step):
        """stage 1 (:1433-1445): c = 1, u_a = velx on the first step, else c = 2, u_a = u_prev (leapfrog); exner = exner_0"""
        return self.update(velx, Fu, 1.0, exner) if first_step else self.update(u_prev, Fu, 2.0, exner)

    def corrector(self, velx_0, Fu, exner_h):
        """stage 3 (:1477-1489): c = 1, u_a = velx_0; exner = exner_h, the field the vertical solve left"""
        return self.update(velx_0, Fu, 1.0, exner_h)

    def verify(self):
        """MassSolver.verify: every fixed-length solve since the last call met its check"""
        return self.m1.verify()
