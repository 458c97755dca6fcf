"""Euler::diagnostics (eul/Euler_2.cpp:600-744): the energy budget of a 3-D state, the line the reference appends to output/energetics.dat
after every step -- its only verification of the Euler stack.  Twelve numbers in the file's order (FIELDS):

  keh kev pe ie k2p p2k k2i i2k k2i_z i2k_z mass entr

  horizontal()   keh, ie, entr, mass: the four element-local quadrature sums over all levels in one element pass plus a fixed-order final
                 pass (mimsem_euler_energetics_horiz, csrc/energetics.inc)
  column()       kev, k2p, p2k, pe (:638-664, :675-684): at orders <= 4 one pass over velz, rho, zv (mimsem_euler_energetics_column,
                 csrc/energetics.inc: the LINEAR_INV blocks are read, every other factor is a quadrature sum formed in registers) and the
                 final pass of horizontal(); at higher orders, and as column_composed() at every order, composed from the column operators,
                   kev = 1/2 sum_e rho_e . CONLIN_W(velz_e) velz_e / SCALE         k2p = sum_e gi_e . gv_e / SCALE
                   p2k = sum_e (V10 gi_e) . zv_e / SCALE                           pe  = sum_e zv_e . rho_e / SCALE
                 with gi = LINEAR_INV LINEAR_RT(rho, vert) velz and gv = V01 zv (initGZ's GRAD gz, eul/VertSolve.cpp:148-162; computed once per
                 zv and kept); the four dot products are ONE rowdot of four rows over the flattened column arrays
  diagnostics()  diagTheta_L2, the two halves, k2i from HorizSolve.k2i_dev and k2i_z from VertSolve.k2i_z, i2k = i2k_z = 0 as in the reference;
                 exactly one device-to-host read
  write_line()   the reference's format (:716-734): every value as %.16g followed by a tab, then a newline

Nothing here synchronises with the host except the one read of diagnostics(): diagnostics(..., read=False) returns the device tensor of 12 and
can be recorded by Engine.capture.  Single context, global numbering, as VortDiag; sharded runs are out of scope."""
import torch

from .vertsolve import FLAG_VERT, SCALE

FIELDS = ("keh", "kev", "pe", "ie", "k2p", "p2k", "k2i", "i2k", "k2i_z", "i2k_z", "mass", "entr")


class Energetics:
    FUSED_MAX_ORDER = 4                      # the orders mimsem_euler_energetics_column is instantiated for (those of the fused Newton entries)

    def __init__(self, eng, vert, horiz=None):
        """eng: Engine with nk >= 2 levels; vert: its VertSolve (column operators, k2i_z); horiz: the HorizSolve whose momentum_rhs_ec left k2i
        (None: k2i = 0)"""
        if vert.eng is not eng or (horiz is not None and horiz.eng is not eng):
            raise ValueError("Energetics: vert / horiz belong to another engine")
        if eng.nk < 2:
            raise ValueError("Energetics needs at least one interface (nk >= 2)")
        self.eng, self.vert, self.horiz = eng, vert, horiz
        self.nk = eng.nk
        self.zv = None                       # the geopotential diagnostics() uses: set_geopotential
        self.fused = True                    # column(): the one-pass kernel where it exists, 2.9x the composed route's speed at the bench mesh
                                             # (profiles/energetics_column.txt); False: column_composed everywhere
        self._gv_of, self._gv = None, None
        n = eng.nEl * eng.nk * eng.n2e
        # rows of the one rowdot: kev, k2p, p2k, pe.  The interface arrays of k2p are shorter than a level array: their tails stay zero
        self._A = torch.zeros(4, n, dtype=torch.float64, device=eng.device)
        self._B = torch.zeros(4, n, dtype=torch.float64, device=eng.device)
        # FIELDS from [keh ie entr mass | kev k2p p2k pe | k2i k2i_z 0]
        self._order = torch.tensor([0, 4, 7, 1, 5, 6, 8, 10, 9, 10, 3, 2], dtype=torch.int64, device=eng.device)
        self._factor = torch.tensor([0.5 / SCALE, 1.0 / SCALE, 1.0 / SCALE, 1.0 / SCALE], dtype=torch.float64, device=eng.device)

    def set_geopotential(self, zv):
        """zv: VertSolve.init_gz(levs), vertical layout [nEl, nk n2e]; its gradient gv = V01 zv is formed here, once"""
        self.eng._col(zv, self.nk, "zv")
        self.zv = zv
        self._gv_of, self._gv = zv, self.vert.V01(zv)
        return self

    def _grad(self, zv):
        if self._gv_of is not zv:
            self._gv_of, self._gv = zv, self.vert.V01(zv)
        return self._gv

    def horizontal(self, velx, rho, rt, exner, theta, out=None):
        """[keh, ie, entr, mass] (device) from velx [nk, n1] and rho, rt, exner, theta [nk, n2] in the horizontal layout"""
        return self.eng.energetics_horiz(velx, rho, rt, exner, theta, out=out)

    def column(self, velz, rho, zv=None):
        """[kev, k2p, p2k, pe] (device) from velz [nEl, (nk-1) n2e], rho and zv [nEl, nk n2e] in the vertical layout: ONE pass over the three
        inputs (Engine.energetics_column, k_energetics_column) at orders <= 4 when self.fused, the composed route otherwise"""
        if not self.fused or self.eng.mesh.n > self.FUSED_MAX_ORDER:
            return self.column_composed(velz, rho, zv)
        zv = self.zv if zv is None else zv
        if zv is None:
            raise ValueError("Energetics.column: no geopotential (pass zv or call set_geopotential)")
        return self.eng.energetics_column(velz, rho, zv)

    def column_composed(self, velz, rho, zv=None):
        """column() composed from the single column operators (five operator launches, one V10, seven copies into padded rows, one rowdot):
        every order; kept beside the fused kernel for comparison -- the two differ in summation order only"""
        eng, vert, nk = self.eng, self.vert, self.nk
        zv = self.zv if zv is None else zv
        if zv is None:
            raise ValueError("Energetics.column: no geopotential (pass zv or call set_geopotential)")
        eng._col(velz, nk - 1, "velz"); eng._col(rho, nk, "rho"); eng._col(zv, nk, "zv")
        gv = self._grad(zv)
        w2 = vert._mv("CONLIN_W", velz, f1=velz, rows=nk)                                    # AssembleConLinWithW(velz) velz :644-645
        gi = vert._mv("LINEAR_INV", vert._mv("LINEAR_RT", velz, f1=rho, flags=FLAG_VERT, rows=nk - 1), rows=nk - 1)      # :650-653
        dg = vert.V10(gi)                                                                    # :657
        A, B, m = self._A, self._B, gi.numel()
        A[0].copy_(rho.reshape(-1)); B[0].copy_(w2.reshape(-1))
        A[1, :m].copy_(gi.reshape(-1)); B[1, :m].copy_(gv.reshape(-1))
        A[2].copy_(dg.reshape(-1)); B[2].copy_(zv.reshape(-1))
        A[3].copy_(zv.reshape(-1)); B[3].copy_(rho.reshape(-1))
        return eng.rowdot(A, B) * self._factor

    def diagnostics(self, velx, velz, rho, rt, exner, read=True):
        """Euler::diagnostics: velx [nk, n1], rho, rt, exner [nk, n2] in the horizontal layout, velz [nEl, (nk-1) n2e] in the vertical one (the
        reference's velz[ei]).  Returns the 12 numbers of FIELDS as a list of floats (ONE device-to-host read); read=False: as a device
        tensor, without any host synchronisation (k2i_z is the host number VertSolve holds at the time of the call)."""
        eng, nk = self.eng, self.nk
        rho_v, rt_v = eng.l2_horiz_to_vert(rho), eng.l2_horiz_to_vert(rt)                    # l2_rho / l2_rt ->HorizToVert :626-627, :701-702
        theta = eng.l2_vert_to_horiz(eng.diag_theta(0, rho_v, rt_v), nk)                     # diagTheta_L2, VertToHoriz :703-704
        h = self.horizontal(velx, rho, rt, exner, theta)                                     # keh ie entr mass
        c = self.column(velz, rho_v)                                                         # kev k2p p2k pe
        one = lambda v: torch.full((1,), float(v), dtype=torch.float64, device=eng.device)
        k2i = self.horiz.k2i_dev if self.horiz is not None else None                         # vert->horiz->k2i :694 (stays on the device)
        k2i = one(0.0) if k2i is None else k2i.reshape(1).to(torch.float64)
        out = torch.cat([h, c, k2i, one(self.vert.k2i_z), one(0.0)])[self._order]            # vert->k2i_z :693; i2k = i2k_z = 0 :695
        return out.tolist() if read else out

    @staticmethod
    def write_line(path, values):
        """append one line in the reference's format (file.precision(16); value, tab, ..., endl :716-734)"""
        if len(values) != len(FIELDS):
            raise ValueError("write_line: %d values expected" % len(FIELDS))
        with open(path, "a") as f:
            f.write("".join("%.16g\t" % float(v) for v in values) + "\n")
