"""Every fixed-length solve is checked: its check norms go to a device log, the host reads the log once per step / evaluation, and a miss
switches the solver to its adaptive form and redoes the step.  This module is the Python hosts' one implementation of that -- the
counterpart of CheckLog and cheb::accepted / interval_steps / rate_steps of mimsem_amd/host/mimsem_mass.hpp, same names, same rule."""
import math
from itertools import accumulate

import numpy as np
import torch

from ._lib import MimsemError


def accepted(r2, ref2, bound):
    """THE acceptance rule of a check (cheb::relative / cheb::accepted), vectorised: rel = |r| / |ref| of logged pairs {|r|^2, |ref|^2} -- 0 where
    both are exactly zero (a slot not written, a zero right-hand side), NaN where the reference is no positive number; accepted iff
    rel <= bound (NaN compares false: a miss).  A logged ratio |r|^2 / |ref|^2 is accepted(ratio, 1.0, bound).  Returns (ok, rel).
    Two Python floats take the same rule without numpy (a host that judges a handful of slots per replayed iteration: 0.3 against 18 us)."""
    if type(r2) is float and type(ref2) is float:
        rel = 0.0 if r2 == 0.0 and ref2 == 0.0 else (math.sqrt(r2 / ref2) if ref2 > 0.0 and r2 >= 0.0 else math.nan)
        return rel <= bound, rel
    r2, ref2 = np.asarray(r2, dtype=np.float64), np.asarray(ref2, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where((r2 == 0.0) & (ref2 == 0.0), 0.0, np.where(ref2 > 0.0, np.sqrt(r2 / np.where(ref2 > 0.0, ref2, 1.0)), np.nan))
        return rel <= bound, rel


def interval_rate(lmin, lmax):
    """contraction per step of the Chebyshev iteration on a real interval [lmin, lmax]"""
    s = math.sqrt(lmax / lmin)
    return (s - 1.0) / (s + 1.0)


def interval_steps(l1, l2, rtol):
    """steps of the M1 iteration on [l1, l2] until the last sweep sees a residual of rtol"""
    return max(2, int(math.ceil(math.log(2.0 / rtol) / math.log(1.0 / interval_rate(l1, l2)))))


def rate_steps(rate, rtol):
    """steps of an iteration that contracts by `rate` whose RESULT reaches rtol (the [u|h] system, the upwinded 0-form mass)"""
    return max(2, int(math.ceil(math.log(0.5 * rtol) / math.log(rate))) + 1)


class CheckLog:
    """{|r|^2, |ref|^2} pairs of the checked solves in one device array [capacity, 2 width] (width systems per solve: first their |r|^2, then
    their |ref|^2), read with one copy.  A slot is claimed on the host when the solve is issued -- or recorded: its address is then part of the
    graph, and a body that is recorded more than once rewinds first so that every replay lands in the same slots."""

    def __init__(self, eng, capacity, width=1, reuse_last=False):
        """reuse_last: a log that is read at the caller's leisure (MassSolver) keeps taking solves when it is full -- they overwrite the last
        slot, and `shared` counts them; otherwise a claim past the capacity raises MimsemError"""
        self.eng, self.capacity, self.width, self.reuse_last = eng, capacity, width, reuse_last
        self.dist = hasattr(eng, "halo")
        self.dev = torch.zeros(capacity, 2 * width, dtype=torch.float64, device=eng.device)
        self.kinds = [None] * capacity
        self.size = self.shared = 0

    def kind(self, k):
        return self.kinds[k]

    def rewind(self):
        self.size = self.shared = 0

    def clear(self):
        self.dev.zero_()
        self.rewind()

    def claim(self, kind=None):
        """the next slot: the device view a caller fills with launches of its own"""
        if self.size < self.capacity:
            k = self.size
            self.size += 1
        elif self.reuse_last:
            k = self.capacity - 1
            self.shared += 1
        else:
            raise MimsemError("CheckLog: check-norm slots exhausted (%d)" % self.capacity)
        self.kinds[k] = kind
        return self.dev[k]

    def pair(self, both, kind=None, space=None):
        """both = (r | ref) side by side, [2 width, n]: every norm with ONE two-row-block dot (sharded: this rank's ownership-weighted part)"""
        self.eng.rowdot_local(both, both, out=self.claim(kind), space=space)

    def two(self, res, ref, kind=None, space=None):
        s = self.claim(kind)
        res, ref = res.reshape(1, -1), ref.reshape(1, -1)
        self.eng.rowdot_local(res, res, out=s[0:1], space=space)
        self.eng.rowdot_local(ref, ref, out=s[1:2], space=space)

    @staticmethod
    def read(*logs):
        """ONE device-to-host transfer for any number of logs and ratio rows (plain tensors) together, None entries passed through; a sharded
        engine reduces them in one all-reduce first (with the halo time-outs folded in: DistEngine.allreduce_checked).  Returns the host
        arrays, each in its log's shape.  The only place a check log leaves the device."""
        dev = [l.dev if isinstance(l, CheckLog) else l for l in logs]
        live = [t for t in dev if t is not None]
        flat = live[0] if len(live) == 1 else torch.cat([t.reshape(-1) for t in live])
        for l in logs:
            if isinstance(l, CheckLog) and l.dist:
                l.eng.allreduce_checked(flat)
                break
        host = flat.cpu().numpy().reshape(-1)
        ends = accumulate(0 if t is None else t.numel() for t in dev)
        return [None if t is None else host[e - t.numel():e].reshape(t.shape) for t, e in zip(dev, ends)]


def log_true_residual(eng, A, x, b, row):
    """the check of a fixed-length PCG: row[i] = max(row[i], |b_i - A x_i|^2 / |b_i|^2), a NaN kept (one launch after the two dots); judged
    by accepted(row, 1.0, bound)"""
    r = eng.combine(A(x), -1.0, beta=1.0, c=b)
    return eng.ratio_max(eng.rowdot(r, r), eng.rowdot(b, b), row)
