"""Device-resident mesh + operator engine: thin Python layer over the C ABI (include/mimsem_hip.h).
PyTorch supplies device memory, streams and torch.distributed -- plumbing, not the product."""
import contextlib
import ctypes as C
import gc

import numpy as np
import torch

from . import _lib
from ._lib import COLOPS, FLAG_ACCUM, FLAG_VERT, OPS, MeshDesc, check

_F64, _I32 = torch.float64, torch.int32


def _ptr(t):
    if t is None:
        return None
    if not (t.dtype in (torch.float64, torch.int32) and t.is_contiguous() and t.is_cuda):
        raise _lib.MimsemError("device float64/int32 contiguous tensor required, got %s %s contiguous=%s" % (t.device, t.dtype, t.is_contiguous()))
    return t.data_ptr()


def _need(cond, what):
    """argument validation that survives python -O: the C ABI takes raw pointers, a wrong-sized tensor would be an out-of-bounds
    device access (a GPU memory fault), so sizes are checked here and reported as MimsemError"""
    if not cond:
        raise _lib.MimsemError("invalid argument: " + what)


def _ps(t2):
    """(address, row stride) of a 2-D view that Engine._rows has checked; (None, 0) for an absent optional operand"""
    return (None, 0) if t2 is None else (t2.data_ptr(), t2.stride(0))


def _host(a, dtype):
    """a host numpy array as the ABI reads it: (the contiguous array -- the caller keeps it alive over the call --, its address)"""
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data


def _coef(coef):
    """[(alpha, beta)] of a fixed-length Chebyshev solve as the flat array of doubles the ABI takes"""
    return (C.c_double * (2 * len(coef)))(*[v for ab in coef for v in ab])


class no_gc:
    """Python's cyclic garbage collector must not run inside a stream capture: a collected device tensor is freed by the caching
    allocator with calls that are illegal on a capturing stream, the error is raised inside a destructor and the process aborts
    (seen as 'Fatal Python error: Aborted ... Garbage-collecting' in the middle of a GraphedGMRES capture)."""

    def __enter__(self):
        self.was = gc.isenabled()
        gc.disable()                     # (torch.cuda.graph collects once on entry by itself)

    def __exit__(self, *exc):
        if self.was:
            gc.enable()
        return False


class DeviceMesh:
    """Flattens any set of patches (Topo+Geom pairs) into the element->slot tables of mimsem_mesh_desc.

    numbering="local": exactly one patch, vectors have the reference's per-rank LOCAL (ghosted) layout
                       (Topo::elInds*_l) -- what VecGetArray on the reference's `*l` vectors gives.
    numbering="global": any number of patches; vector slots are the compacted global ids touched by the
                        patches (all of them => the concatenated PETSc global Vec)."""

    def __init__(self, topos, geoms, nk=1, numbering="global"):
        t0 = topos[0]
        self.n, self.m, self.nk = t0.elOrd, geoms[0].quad_ord, nk
        self.topos, self.geoms = topos, geoms
        n2e = self.n * self.n
        if numbering == "local":
            _need(len(topos) == 1, "numbering=\"local\" takes exactly one patch")
            self.inds0, self.inds1x, self.inds1y = t0.all_inds0_l(), t0.all_inds1x_l(), t0.all_inds1y_l()
            self.n0, self.n1, self.n2 = t0.n0, t0.n1, t0.n2
            self.gid0 = self.gid1 = self.gid2 = self.gidq = None
            self.indsq, self.nq = geoms[0].all_inds0_l(), geoms[0].n0
        else:
            g0 = np.concatenate([t.all_inds0_g() for t in topos])
            g1x = np.concatenate([t.all_inds1x_g() for t in topos])
            g1y = np.concatenate([t.all_inds1y_g() for t in topos])
            self.gid0, inv0 = np.unique(g0, return_inverse=True)
            self.gid1, inv1 = np.unique(np.concatenate([g1x.ravel(), g1y.ravel()]), return_inverse=True)
            self.inds0 = inv0.reshape(g0.shape).astype(np.int32)
            self.inds1x = inv1[:g1x.size].reshape(g1x.shape).astype(np.int32)
            self.inds1y = inv1[g1x.size:].reshape(g1y.shape).astype(np.int32)
            self.gid2 = np.concatenate([t.all_inds2_g().ravel() for t in topos])
            gq = np.concatenate([g.loc0[g.all_inds0_l()] for g in geoms])
            self.gidq, invq = np.unique(gq, return_inverse=True)
            self.indsq, self.nq = invq.reshape(gq.shape).astype(np.int32), self.gidq.size
            self.n0, self.n1 = self.gid0.size, self.gid1.size
            self.n2 = self.gid2.size
        self.nEl = self.inds0.shape[0]
        self.inds2 = np.arange(self.nEl * n2e, dtype=np.int32).reshape(self.nEl, n2e)
        self.det = np.ascontiguousarray(np.concatenate([g.det for g in geoms]))
        self.J = np.ascontiguousarray(np.concatenate([g.J for g in geoms]))
        th = [g.thick_at_elements() for g in geoms]
        self.thick = np.ascontiguousarray(np.concatenate([a for a, _ in th], axis=1))
        self.thickInv = np.ascontiguousarray(np.concatenate([b for _, b in th], axis=1))

    def desc(self):
        d = MeshDesc()
        d.elOrd, d.quadOrd, d.nEl, d.nk = self.n, self.m, self.nEl, self.nk
        d.n0, d.n1, d.n2 = self.n0, self.n1, self.n2
        keep = []
        d.nq = self.nq
        for name in ("inds0", "inds1x", "inds1y", "inds2", "indsq"):
            a, p = _host(getattr(self, name), np.int32); keep.append(a)
            setattr(d, name, p)
        for name in ("det", "J", "thick", "thickInv"):
            a, p = _host(getattr(self, name), np.float64); keep.append(a)
            setattr(d, name, p)
        d._keep = keep
        return d


class Engine:
    """One mimsem_ctx on one GPU."""

    def __init__(self, dmesh, device=0):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.MimsemError("no GPU visible: the operator engine has no CPU fallback")
        self.mesh = dmesh
        self.device = torch.device("cuda", device)
        self.ctx = C.c_void_p()
        d = dmesh.desc()
        torch.cuda.set_device(self.device)
        check(self.L.mimsem_ctx_create(C.byref(d), device, C.byref(self.ctx)), "mimsem_ctx_create")
        self.use_stream(torch.cuda.current_stream(self.device))
        n = dmesh.n
        self.n0e, self.n1e, self.n2e, self.mp12 = (n + 1) ** 2, (n + 1) * n, n * n, (n + 1) ** 2
        self.nEl, self.nk = dmesh.nEl, dmesh.nk
        self.sizes = {0: dmesh.n0, 1: dmesh.n1, 2: dmesh.n2, "q": dmesh.nq, "q2": 2 * dmesh.nq}
        self._linear_inv = None              # the LINEAR_INV column blocks energetics_column reads (made on its first call)
        self._zonal_nb = 0                   # bands of the context's zonal plan (zonal_plan; 0: none)

    def __del__(self):
        try:
            if self.ctx:
                self.L.mimsem_ctx_destroy(self.ctx); self.ctx = C.c_void_p()
        except Exception:
            pass

    def use_stream(self, stream):
        self._stream = stream
        check(self.L.mimsem_ctx_set_stream(self.ctx, C.c_void_p(stream.cuda_stream)), "set_stream")

    def on_current_stream(self):
        """context manager: launch the engine's kernels on torch's CURRENT stream (hipGraph capture, side streams), then
        go back to the stream the engine used before"""
        eng = self

        class _Bind:
            def __enter__(self_b):
                self_b.prev = getattr(eng, "_stream", None)
                eng.use_stream(torch.cuda.current_stream(eng.device))

            def __exit__(self_b, *exc):
                if self_b.prev is not None:
                    eng.use_stream(self_b.prev)
                return False
        return _Bind()

    def capture(self, fn):
        """Capture fn() -- engine calls and torch ops on fixed buffers, no host synchronisation -- in a hipGraph.  Returns
        (graph, outputs): graph.replay() re-runs the whole launch sequence with one submission; outputs are the static
        tensors fn returned (overwritten by every replay)."""
        dev = self.device
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s), self.on_current_stream():
            fn()                                        # warm-up: workspaces reach their final size outside the capture
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(g), self.on_current_stream():
            out = fn()
        torch.cuda.synchronize(dev)
        return g, out

    def sync(self):
        check(self.L.mimsem_ctx_sync(self.ctx), "sync")

    def set_profiling(self, every):
        """0 = off; n > 0 = time every n-th op_apply with hipExtLaunchKernelGGL start/stop events"""
        check(self.L.mimsem_ctx_set_profiling(self.ctx, int(every)), "set_profiling")

    def set_wave_balance(self, ncu=0, wgs_per_cu=2):
        """balanced level ranges of the one-launch Umat form: deal wgs_per_cu x ncu workgroups of equal work (ncu = 0: the device's CUs,
        < 0: off, > 0: a pretended chip); mimsem_ctx_set_wave_balance"""
        _need(int(ncu) < 0 or 1 <= int(wgs_per_cu) <= 3, "set_wave_balance: 1 .. 3 workgroups per CU")
        check(self.L.mimsem_ctx_set_wave_balance(self.ctx, int(ncu), int(wgs_per_cu)), "set_wave_balance")

    def set_level_chunk(self, lch):
        """levels per work item of the element kernel, the shared-block applies and the owned-block pass: 1 .. 8 is a request, 0 the library's
        own rules (tuning and tests only; results do not depend on it); mimsem_ctx_set_level_chunk"""
        _need(0 <= int(lch) <= 8, "set_level_chunk: 0 (the library's rules) or 1 .. 8 levels per work item")
        check(self.L.mimsem_ctx_set_level_chunk(self.ctx, int(lch)), "set_level_chunk")

    def profile_read(self):
        """(ms in element kernels, ms in gather-sum kernels, launches) since the last read"""
        a, b, n = C.c_double(), C.c_double(), C.c_longlong()
        check(self.L.mimsem_ctx_profile_read(self.ctx, C.byref(a), C.byref(b), C.byref(n)), "profile_read")
        return a.value, b.value, n.value

    def tensor(self, a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(self.device).contiguous()

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float64, device=self.device)

    # ---- argument checks ----------------------------------------------------------------------
    # The C ABI takes raw addresses and cannot check a length, so every wrapper below takes its addresses from _rows / _like / _out
    # (with _ps), _vec, _word, _blocks or _col (with _ptr) -- nowhere else -- and every failure is a MimsemError through _need.
    def _rows(self, t, n, name, rows=None, min_rows=0, optional=False, strided=False, dtype=_F64):
        """the 2-D view of a row array [nrows, n] (a [n] tensor: one row), checked for what keeps the library in bounds: float64 (int32
        where the ABI wants indices) on this engine's device, rows of length n (None: as they come), `rows` rows or at least min_rows.
        strided=False: one contiguous block, as _ptr demands; "r" / "w": rows with unit inner stride that lie at least n apart (slices of
        a wider array; "r", read only: also the same row for every level, as expand() makes)"""
        if t is None:
            _need(optional, name + " is required")
            return None
        d = t.dim()
        t2 = t if d == 2 else t.unsqueeze(0)
        if (d == 2 or d == 1) and t2.dtype is dtype and t2.device == self.device:
            r, w = t2.shape
            if (n is None or w == n) and (rows is None or r == rows) and r >= min_rows:
                if t2.is_contiguous() if not strided else (t2.stride(1) == 1 and (r <= 1 or t2.stride(0) >= w or (strided == "r" and t2.stride(0) == 0))):
                    return t2
        _need(False, "%s: %s %s rows of length %s on %s required (%s), got %s %s on %s with strides %s" % (
            name, dtype, rows if rows is not None else ">= %d" % min_rows, n, self.device, "one contiguous block" if not strided else "contiguous rows",
            t.dtype, tuple(t.shape), t.device, t.stride()))

    def _like(self, n, rows, strided=False, **named):
        """_rows for several operands of one shape [rows, n], in the order given; None stays None (the library refuses a missing operand)"""
        return [self._rows(t, n, name, rows=rows, optional=True, strided=strided) for name, t in named.items()]

    def _out(self, out, rows, n, exact=False, strided=False, zero=False):
        """(result, its 2-D view) of a row wrapper: `out` when given -- rows of length n, at least `rows` of them (exact: just `rows`) --,
        else a new [rows, n] tensor"""
        if out is None:
            out = (torch.zeros if zero else torch.empty)(rows, n, dtype=_F64, device=self.device)
            return out, out
        return out, self._rows(out, n, "out", rows if exact else None, rows, False, strided)

    def _vec(self, t, n, name, atleast=False, optional=False, dtype=_F64, pinned=False):
        """address of a flat array: one contiguous block of n entries (atleast: n or more; n None: as it comes) of any shape, float64 or
        int32, on this engine's device (pinned: see _word)"""
        if t is None:
            _need(optional, name + " is required")
            return None
        if t.dtype == dtype and t.is_contiguous() and (n is None or (t.numel() >= n if atleast else t.numel() == n)) \
                and (t.device == self.device or (pinned and t.is_pinned())):
            return t.data_ptr()
        _need(False, "%s: a contiguous %s array of %s%s entries on %s required, got %s %s on %s" % (
            name, dtype, "at least " if atleast else "", n, self.device, t.dtype, tuple(t.shape), t.device))

    def _word(self, t, n, name, dtype=_F64):
        """the col / flag words of cgs2, reorthonormalize and normalize, the one exception to "on this engine's device": they may lie in
        PINNED host memory, which the kernels write directly; dtype, contiguity and length (at least n) are checked as everywhere"""
        return self._vec(t, n, name, atleast=True, optional=True, dtype=dtype, pinned=True)

    def _blocks(self, t, nd, name, nlev=None):
        """(address, level stride) of element blocks: one contiguous float64 [nEl, nd, nd] set (stride 0) or, where nlev is given, also
        [nlev, nEl, nd, nd]"""
        if not (t is not None and t.dtype == _F64 and t.device == self.device and t.is_contiguous() and t.shape[-3:] == (self.nEl, nd, nd)
                and (t.dim() == 3 or (nlev is not None and t.dim() == 4 and t.shape[0] == nlev))):
            _need(False, "%s: contiguous float64 blocks [%snEl=%d, %d, %d] on %s required, got %s" % (
                name, "" if nlev is None else "(nlev=%d, ) " % nlev, self.nEl, nd, nd, self.device,
                None if t is None else (t.dtype, tuple(t.shape), t.device, t.stride())))
        return t.data_ptr(), t.stride(0) if t.dim() == 4 else 0

    def _new(self, *shape):
        return torch.empty(*shape, dtype=_F64, device=self.device)

    # ---- horizontal operators ---------------------------------------------------------------
    _SPACES = dict(UMAT=(1, None, 1), UTMAT=(1, None, 1), UHMAT=(1, 2, 1), UTMAT_H=(1, 2, 1), ROTMAT=(1, 0, 1),
                   WMAT=(2, None, 2), WMATINV=(2, None, 2), WHMAT=(2, 2, 2), WHMATINV=(2, 2, 2), PMAT=(0, None, 0),
                   PHMAT=(0, 2, 0), WTQUMAT=(1, 1, 2), WTQDUDZ=(1, 1, 2), UTQWMAT=(2, 1, 1),
                   PHMAT_UP=(0, 2, 0), ROTMAT_UP=(1, 0, 1), UMAT_UP=(1, 1, 1), UHMAT_UP=(1, 2, 1), UVEC_HU_UP=(1, 2, 1), WTQ=("q", None, 2), PTQ=("q", None, 0), UTQ=("q2", None, 1))

    def _op_args(self, op, x, f, out, exact=False):
        """the _SPACES-driven check shared by apply, apply_part, apply_levels, apply_up and prepare_apply: the 2-D views of x and of the
        operator's field (None for an operator that takes none), the result (given or new) and its 2-D view"""
        sin, sf, sout = self._SPACES[op]
        x2 = self._rows(x, self.sizes[sin], "x")
        f2 = None if sf is None else self._rows(f, self.sizes[sf], "f", x2.shape[0])
        return (x2, f2) + self._out(out, x2.shape[0], self.sizes[sout], exact)

    def _fsize(self, op):
        """length of the operator's field rows; None (not checked) for an operator that takes none"""
        sf = self._SPACES.get(op, (None, None, None))[1]
        return None if sf is None else self.sizes[sf]

    def apply(self, op, x, f=None, lev0=0, scale=1.0, flags=0, alpha=1.0, out=None):
        """y_k = A_op(level lev0+k, f_k) x_k ; x: [nlev, n_in] (or [n_in]) device tensor"""
        x2, f2, y, y2 = self._op_args(op, x, f, out)
        check(self.L.mimsem_op_apply(self.ctx, OPS[op], lev0, x2.shape[0], scale, flags, *_ps(f2), *_ps(x2), *_ps(y2), alpha), "mimsem_op_apply(%s)" % op)
        return y if x.dim() == 2 else y2[0]

    def apply_levels(self, op, x, lev_step, f=None, lev0=0, scale=1.0, flags=0, alpha=1.0, out=None):
        """mimsem_op_apply_levels: apply() with row r at geometry level lev0 + r lev_step; lev_step 0 (WMAT, UHMAT) evaluates every row
        at lev0, as HorizSolve::diagVertVort assembles M2 and F"""
        x2, f2, y, y2 = self._op_args(op, x, f, out)
        check(self.L.mimsem_op_apply_levels(self.ctx, OPS[op], lev0, lev_step, x2.shape[0], scale, flags, *_ps(f2), *_ps(x2), *_ps(y2), alpha),
              "mimsem_op_apply_levels(%s)" % op)
        return y

    def set_halo_slots(self, form, slots):
        """mark the 1-form slots that take part in a halo exchange: their element groups move to the front of the plan, so that
        apply_part(..., "boundary") completes exactly those slots (mimsem_ctx_set_halo_slots)"""
        sl, p = _host(slots, np.int32)
        check(self.L.mimsem_ctx_set_halo_slots(self.ctx, form, p, sl.size), "ctx_set_halo_slots")

    def reset_parts(self):
        """forget a BOUNDARY part whose INTERIOR part will not come (error path of a split apply; mimsem_op_apply_part_reset)"""
        check(self.L.mimsem_op_apply_part_reset(self.ctx), "op_apply_part_reset")

    def apply_part(self, op, part, x, f=None, lev0=0, scale=1.0, flags=0, alpha=1.0, out=None):
        """the boundary or the interior part of apply(): part "boundary" first (all marked slots of `out` complete afterwards), then
        "interior" into the SAME out with the same arguments.  The pending boundary part keeps its partial sums in a buffer of its own:
        other calls may run in between, but a second boundary part or a non-matching interior part is refused (MIMSEM_ERR_STATE)"""
        _need(out is not None, "apply_part: out [nlev, n_out] is required")
        x2, f2, y, y2 = self._op_args(op, x, f, out, exact=True)
        check(self.L.mimsem_op_apply_part(self.ctx, OPS[op], lev0, x2.shape[0], scale, flags, *_ps(f2), *_ps(x2), *_ps(y2), alpha,
                                          {"all": 0, "boundary": 1, "interior": 2}[part]), "mimsem_op_apply_part(%s)" % op)
        return out

    def apply_up(self, op, x, f, u, fac=None, dt=None, lev0=0, alpha=1.0, flags=0, out=None, scale=1.0, tau=None):
        """upwinded operators: f = the op's field, u = second (velocity) field.  SW ops (PHMAT_UP / ROTMAT_UP) pass fac, dt
        (tau = 1/(1/(fac*dt)), src/Assembly.cpp:541); the eul ops (UMAT_UP / UHMAT_UP / UVEC_HU_UP) pass scale and tau."""
        if tau is None:
            tau = 1.0 / (1.0 / (fac * dt))
        x2, f2, y, y2 = self._op_args(op, x, f, out)
        u2 = self._rows(u, self.sizes[1], "u", rows=x2.shape[0])
        check(self.L.mimsem_op_apply_up(self.ctx, OPS[op], lev0, x2.shape[0], scale, tau, flags, *_ps(f2), *_ps(u2), *_ps(x2), *_ps(y2), alpha),
              "mimsem_op_apply_up(%s)" % op)
        return y if x.dim() == 2 else y2[0]

    def _sweep_rows(self, op, x, f, u, form=None, **like):
        """operands of an in-place sweep: the views of x [nlev, n], the operator's field rows, the velocity rows and x's like-shaped
        companions (None stays None).  form None: n from the operator, which must be square"""
        sin, sf, sout = self._SPACES[op]
        _need(form is not None or sin == sout, "%s is not a square operator" % op)
        n = self.sizes[sin if form is None else form]
        x2 = self._rows(x, n, "x")
        nlev = x2.shape[0]
        return (x2, self._rows(f, self._fsize(op), "f", rows=nlev, optional=True), self._rows(u, self.sizes[1], "u", rows=nlev, optional=True),
                self._like(n, nlev, **like))

    def richardson_sweep(self, op, x, b, dinv, f=None, u=None, tau=0.0, lev0=0, scale=1.0, flags=0, upd=None):
        """x += dinv * (b - Op x) in place (mimsem_op_richardson_sweep: element pass + gather with the update epilogue);
        upd (optional, same shape) receives the update.  [nlev, n] tensors."""
        x2, f2, u2, (b2, d2, upd2) = self._sweep_rows(op, x, f, u, b=b, dinv=dinv, upd=upd)
        check(self.L.mimsem_op_richardson_sweep(self.ctx, OPS[op], lev0, x2.shape[0], scale, tau, flags, *_ps(f2), *_ps(u2), *_ps(b2), *_ps(d2),
                                                *_ps(x2), *_ps(upd2)), "richardson_sweep(%s)" % op)
        return x

    def chebyshev_sweep(self, op, x, b, dinv, p, alpha, beta, f=None, u=None, tau=0.0, lev0=0, scale=1.0, flags=0, upd=None):
        """z = dinv * (b - Op x); p = z + beta p; x += alpha p in place (mimsem_op_chebyshev_sweep: two launches); upd receives z"""
        x2, f2, u2, (b2, d2, p2, upd2) = self._sweep_rows(op, x, f, u, b=b, dinv=dinv, p=p, upd=upd)
        check(self.L.mimsem_op_chebyshev_sweep(self.ctx, OPS[op], lev0, x2.shape[0], scale, tau, flags, *_ps(f2), *_ps(u2), *_ps(b2), *_ps(d2),
                                               float(alpha), float(beta), *_ps(p2), *_ps(x2), *_ps(upd2)), "chebyshev_sweep(%s)" % op)
        return x

    def block_richardson_sweep(self, op, blocks, x, b, f=None, lev0=0, scale=1.0, flags=0, upd=None):
        """x += sum_e R_e^T B_e R_e (b - Op x) in place on 1-forms; blocks [nEl, 2 n1e, 2 n1e] column-major per element
        (mimsem_block_richardson_sweep: element pass, block pass with on-the-fly gathered residual, gather with update)"""
        x2, f2, _, (b2, upd2) = self._sweep_rows(op, x, f, None, form=1, b=b, upd=upd)
        check(self.L.mimsem_block_richardson_sweep(self.ctx, OPS[op], lev0, x2.shape[0], scale, flags, *_ps(f2),
                                                   self._blocks(blocks, 2 * self.n1e, "blocks")[0], *_ps(b2), *_ps(x2), *_ps(upd2)),
              "block_richardson_sweep(%s)" % op)
        return x

    def _elem_scale(self, elem_scale, nlev):
        return self._rows(elem_scale, self.nEl, "elem_scale", rows=nlev, optional=True)

    def block_chebyshev_sweep(self, op, blocks, x, b, p, alpha, beta, f=None, elem_scale=None, lev0=0, scale=1.0, flags=0, upd=None):
        """z = P (b - Op x) with P = sum_e R_e^T (elem_scale[lev, e] B_e) R_e; p = z + beta p; x += alpha p -- in place, three
        launches (mimsem_block_chebyshev_sweep).  blocks [nEl, 2 n1e, 2 n1e] column-major per element."""
        x2, f2, _, (b2, p2, upd2) = self._sweep_rows(op, x, f, None, form=1, b=b, p=p, upd=upd)
        check(self.L.mimsem_block_chebyshev_sweep(self.ctx, OPS[op], lev0, x2.shape[0], scale, flags, *_ps(f2),
                                                  self._blocks(blocks, 2 * self.n1e, "blocks")[0], *_ps(self._elem_scale(elem_scale, x2.shape[0])),
                                                  *_ps(b2), alpha, beta, *_ps(p2), *_ps(x2), *_ps(upd2)), "block_chebyshev_sweep(%s)" % op)
        return x

    def _solve_rows(self, b, x, pb, upd):
        """operands of a fixed-length 1-form solve from x = 0: (x -- new when not given --, nlev, the (address, stride) pairs of b, x, pb, upd)"""
        b2 = self._rows(b, self.sizes[1], "b")
        x = torch.empty_like(b) if x is None else x
        return (x, b2.shape[0], _ps(b2)) + tuple(_ps(t2) for t2 in self._like(self.sizes[1], b2.shape[0], x=x, pb=pb, upd=upd))

    def block_chebyshev_solve(self, op, blocks, b, coef, x=None, elem_scale=None, lev0=0, scale=1.0, flags=0, pb=None, upd=None):
        """the whole fixed-length solve from x = 0 as ONE call: len(coef) steps of block_chebyshev_sweep, the first without its operator pass
        and without cleared x / p (mimsem_block_chebyshev_solve; the same bits).  coef: [(alpha, beta)]; pb / upd receive the first / last
        preconditioned residual."""
        x, nlev, pb_, px, ppb, pupd = self._solve_rows(b, x, pb, upd)
        check(self.L.mimsem_block_chebyshev_solve(self.ctx, OPS[op], lev0, nlev, scale, flags, None, 0, self._blocks(blocks, 2 * self.n1e, "blocks")[0],
                                                  *_ps(self._elem_scale(elem_scale, nlev)), *pb_, len(coef), _coef(coef), *px, *ppb, *pupd),
              "block_chebyshev_solve(%s)" % op)
        return x

    def fric_chebyshev_solve(self, blocks, b, coef, tau, exner, exner_s, x=None, elem_scale=None, lev0=0, scale=1.0, flags=1, pb=None, upd=None):
        """block_chebyshev_solve for (M1 + M1ray(tau)) x = b (mimsem_fric_chebyshev_solve): the element pass of every step is UMAT_FRIC.  exner
        [nlev, n2]: the levels lev0.., exner_s [n2]: level 0; tau = 0 or exner = None: block_chebyshev_solve("UMAT", ...) itself."""
        x, nlev, pb_, px, ppb, pupd = self._solve_rows(b, x, pb, upd)
        ex2 = self._rows(exner, self.sizes[2], "exner", rows=nlev, optional=True)
        check(self.L.mimsem_fric_chebyshev_solve(self.ctx, OPS["UMAT"], lev0, nlev, scale, flags, None, 0, self._blocks(blocks, 2 * self.n1e, "blocks")[0],
                                                 *_ps(self._elem_scale(elem_scale, nlev)), *pb_, len(coef), _coef(coef), *px, *ppb, *pupd,
                                                 float(tau), *_ps(ex2), self._vec(exner_s, self.sizes[2], "exner_s", optional=ex2 is None)),
              "fric_chebyshev_solve")
        return x

    _OWNED_FORM = {"UMAT": 1, "UHMAT": 1, "UTMAT": 1, "UTMAT_H": 1, "WMAT": 2, "WHMAT": 2}

    def owned_rows(self, form):
        """rows of an owned block (mimsem_owned_blocks_*): the 2 n^2 edges (1-forms) or n^2 faces (2-forms) an element owns"""
        return {1: 2 * self.mesh.n * self.mesh.n, 2: self.n2e}[form]

    def owned_covers_all(self, form=1):
        """True when every slot of the form lies in an owned block (the rule of mimsem_owned_blocks_*: an element owns its x-edges of columns
        0..n-1 and y-edges of rows 0..n-1; 2-forms: its faces).  Spheres and periodic boxes as a whole: True; a rank-local layout's ghosts: False."""
        dm, n = self.mesh, self.mesh.n
        if form == 2:
            return np.unique(dm.inds2).size == self.sizes[2]
        l = np.arange(n * (n + 1))
        own = np.concatenate([np.asarray(dm.inds1x)[:, l % (n + 1) < n], np.asarray(dm.inds1y)[:, l // n < n]], axis=1)
        return np.unique(own).size == self.sizes[1]

    def owned_blocks(self, op, f=None, lev0=0, nlev=1, scale=1.0, flags=0, invert=False):
        """the reference's PCBJACOBI blocks (PCBJacobiSetTotalBlocks(size*nElsX*nElsX)): the ASSEMBLED diagonal block of the slots each element
        owns, [nlev, nEl, nd, nd] row-major for geometry levels lev0.. (mimsem_owned_blocks_build; f: [nlev, n_field] rows); invert: their exact
        inverses (mimsem_block_inverse), what owned_blocks_apply and owned_block_chebyshev_solve take"""
        nd = self.owned_rows(self._OWNED_FORM[op])
        out = self._new(nlev, self.nEl, nd, nd)
        check(self.L.mimsem_owned_blocks_build(self.ctx, OPS[op], lev0, nlev, scale, flags, *_ps(self._rows(f, self._fsize(op), "f", rows=nlev, optional=True)), _ptr(out)),
              "mimsem_owned_blocks_build(%s)" % op)
        if invert:
            check(self.L.mimsem_block_inverse(self.ctx, nlev * self.nEl, nd, _ptr(out)), "block_inverse")
        return out

    def owned_blocks_apply(self, form, blocks, x, out=None):
        """y[slots of block k] = B_k x[slots of block k] for every owned block and every row of x (mimsem_owned_blocks_apply, one launch); blocks
        [nEl, nd, nd] (one set for all rows) or [nlev, nEl, nd, nd].  Slots outside every block keep what `out` held (zeros when not given)."""
        x2 = self._rows(x, self.sizes[form], "x")
        y, y2 = self._out(out, x2.shape[0], self.sizes[form], exact=True, zero=True)
        check(self.L.mimsem_owned_blocks_apply(self.ctx, form, x2.shape[0], *self._blocks(blocks, self.owned_rows(form), "blocks", nlev=x2.shape[0]),
                                               *_ps(x2), *_ps(y2)), "mimsem_owned_blocks_apply")
        return y if x.dim() == 2 else y2[0]

    def owned_block_chebyshev_solve(self, blocks, b, coef, x=None, lev0=0, scale=1.0, flags=0, pb=None, upd=None):
        """block_chebyshev_solve with the owned-block preconditioner (mimsem_owned_block_chebyshev_solve): len(coef) steps of {element pass,
        owned-block pass} from x = 0 on Umat; blocks: the inverses, [nEl, nd, nd] or [nlev, nEl, nd, nd]"""
        x, nlev, pb_, px, ppb, pupd = self._solve_rows(b, x, pb, upd)
        check(self.L.mimsem_owned_block_chebyshev_solve(self.ctx, OPS["UMAT"], lev0, nlev, scale, flags, *self._blocks(blocks, self.owned_rows(1), "blocks", nlev=nlev),
                                                        *pb_, len(coef), _coef(coef), *px, *ppb, *pupd), "owned_block_chebyshev_solve")
        return x

    def sw_dual_chebyshev(self, coefA, blocks, b1, p1, x1, upd1, coefB, tau, h, u, b0, dinv, p0, x0, upd0, pb1=None, pb0=None):
        """the 1-form mass solve (len(coefA) block-Chebyshev steps on Umat) and the upwinded lumped 0-form mass solve (len(coefB) Chebyshev steps
        on Phmat_up) of one shallow-water Picard iteration, both from x = 0, in SHARED launches (mimsem_sw_dual_chebyshev): the same bits as the
        two sequences of block_chebyshev_sweep / chebyshev_sweep calls on zero iterates.  [1, n] tensors; x1, p1, x0, p0 are outputs / workspaces
        (need not be cleared); upd1 / upd0 receive the last step's preconditioned residual, pb1 / pb0 the first's (P b1, dinv b0)."""
        n0, n1, n2 = self.sizes[0], self.sizes[1], self.sizes[2]
        v = lambda t, n, name, optional=False: self._vec(t, n, name, optional=optional)
        ca, pca = _host(np.asarray(coefA, dtype=np.float64).reshape(-1, 2), np.float64)
        cb, pcb = _host(np.asarray(coefB, dtype=np.float64).reshape(-1, 2), np.float64)
        check(self.L.mimsem_sw_dual_chebyshev(self.ctx, ca.shape[0], pca, self._blocks(blocks, 2 * self.n1e, "blocks")[0], v(b1, n1, "b1"), v(p1, n1, "p1"),
                                              v(x1, n1, "x1"), v(upd1, n1, "upd1", True), v(pb1, n1, "pb1", True), cb.shape[0], pcb, float(tau), v(h, n2, "h"),
                                              v(u, n1, "u"), v(b0, n0, "b0"), v(dinv, n0, "dinv"), v(p0, n0, "p0"), v(x0, n0, "x0"), v(upd0, n0, "upd0", True),
                                              v(pb0, n0, "pb0", True)), "sw_dual_chebyshev")

    def _apply_exner(self, op, x, exner, exner_s, tau, lev0, scale, alpha, flags, out):
        """the one body of apply_ray and apply_fric: mimsem_op_apply_up with exner as the field and exner_s [n2] (one row) in the velocity's place"""
        x2 = self._rows(x, self.sizes[1], "x")
        f2 = self._rows(exner, self.sizes[2], "exner", rows=x2.shape[0])
        y, y2 = self._out(out, x2.shape[0], self.sizes[1])
        check(self.L.mimsem_op_apply_up(self.ctx, OPS[op], lev0, x2.shape[0], scale, tau, flags, *_ps(f2), self._vec(exner_s, self.sizes[2], "exner_s"), 0,
                                        *_ps(x2), *_ps(y2), alpha), "mimsem_op_apply_up(%s)" % op)
        return y if x.dim() == 2 else y2[0]

    def apply_ray(self, x, exner, exner_s, dt, lev0=0, scale=1.0, alpha=1.0, flags=0, out=None):
        """Umat_ray (Held-Suarez friction): x [nlev, n1], exner [nlev, n2] (levels lev0..), exner_s [n2] = level 0."""
        return self._apply_exner("UMAT_RAY", x, exner, exner_s, dt, lev0, scale, alpha, flags, out)

    def apply_fric(self, x, exner, exner_s, tau, lev0=0, scale=1.0, alpha=1.0, flags=0, out=None):
        """M1 + M1ray(tau) in one element pass (MIMSEM_OP_UMAT_FRIC; eul/Euler_2.cpp:1431-1451): Umat with the vertical flag whose point weights
        carry 1 + tau k_v.  Arguments as apply_ray; flags: FLAG_ACCUM or 0."""
        return self._apply_exner("UMAT_FRIC", x, exner, exner_s, tau, lev0, scale, alpha, flags, out)

    def prepare_apply(self, op, x, f=None, lev0=0, scale=1.0, flags=0, alpha=1.0, out=None):
        """Validate once, return (call, y): `call()` re-issues the same mimsem_op_apply with pre-marshalled
        arguments (the buffers are fixed) -- the host-side fast path for time-step loops and bench.py."""
        x2, f2, y, y2 = self._op_args(op, x, f, out)
        (pf, sf), (px, sx), (py, sy) = _ps(f2), _ps(x2), _ps(y2)
        fn = self.L.mimsem_op_apply
        args = (self.ctx, C.c_int(OPS[op]), C.c_int(lev0), C.c_int(x2.shape[0]), C.c_double(scale), C.c_uint(flags), C.c_void_p(pf), C.c_longlong(sf),
                C.c_void_p(px), C.c_longlong(sx), C.c_void_p(py), C.c_longlong(sy), C.c_double(alpha))
        keep = (x2, f2, y2)

        def call(_fn=fn, _args=args, _keep=keep):
            rc = _fn(*_args)
            if rc:
                check(rc, "mimsem_op_apply(%s)" % op)
        return call, y

    def element_matrices(self, op, f=None, lev=0, scale=1.0, flags=0):
        out = self._new(self.nEl, self.L.mimsem_op_elmat_size(self.ctx, OPS[op]))
        check(self.L.mimsem_op_element_matrices(self.ctx, OPS[op], lev, scale, flags, self._vec(f, self._fsize(op), "f", optional=True), _ptr(out)),
              "mimsem_op_element_matrices(%s)" % op)
        return out

    def _elmats_exner(self, op, exner, exner_s, tau, lev, scale):
        """the one body of element_matrices_ray and element_matrices_fric: exner [n2] at the level, exner_s [n2] at level 0"""
        out = self._new(self.nEl, self.L.mimsem_op_elmat_size(self.ctx, OPS[op]))
        check(self.L.mimsem_op_element_matrices_ex(self.ctx, OPS[op], lev, scale, tau, 0, self._vec(exner, self.sizes[2], "exner"),
                                                   self._vec(exner_s, self.sizes[2], "exner_s"), _ptr(out)), "mimsem_op_element_matrices_ex(%s)" % op)
        return out

    def element_matrices_ray(self, exner, exner_s, dt, lev=0, scale=1.0):
        return self._elmats_exner("UMAT_RAY", exner, exner_s, dt, lev, scale)

    def element_matrices_fric(self, exner, exner_s, tau, lev=0, scale=1.0):
        """the element blocks of M1 + M1ray(tau) at one level (what MatAXPY(M1->M, 1.0, M1ray->M) leaves in M1, eul/Euler_2.cpp:1448)"""
        return self._elmats_exner("UMAT_FRIC", exner, exner_s, tau, lev, scale)

    def elem_block_pc(self, op, f=None, lev=0, scale=1.0, flags=0, out=None):
        """mimsem_elem_block_pc_build: D_e (A_e)^-1 D_e of a 1-form mass operator (UMAT, UHMAT with f = the depth row) in one launch,
        [nEl, 2 n1e, 2 n1e] -- the blocks mimsem_ksp_set_pc_bjacobi builds, for blocks_apply(1, ..., transpose=True)"""
        nd = 2 * self.n1e
        out = self._new(self.nEl, nd, nd) if out is None else out
        check(self.L.mimsem_elem_block_pc_build(self.ctx, OPS[op], lev, scale, flags, self._vec(f, self._fsize(op), "f", optional=True), self._blocks(out, nd, "out")[0]),
              "mimsem_elem_block_pc_build(%s)" % op)
        return out

    def elem_block_pc_levels(self, op, nlev, f=None, lev0=0, lev_step=1, scale=1.0, flags=0, out=None):
        """mimsem_elem_block_pc_build_levels: the blocks of elem_block_pc for nlev rows in one launch, [nlev, nEl, 2 n1e, 2 n1e]; row r at
        geometry level lev0 + r lev_step with the field row f[r] (UMAT, UHMAT, UTMAT_H)"""
        nd = 2 * self.n1e
        out = self._new(nlev, self.nEl, nd, nd) if out is None else out
        _need(out.dim() == 4, "out: a contiguous [nlev, nEl, 2 n1e, 2 n1e] tensor")
        check(self.L.mimsem_elem_block_pc_build_levels(self.ctx, OPS[op], lev0, lev_step, nlev, scale, flags,
                                                       *_ps(self._rows(f, self.sizes[2], "f", rows=nlev, optional=True)), self._blocks(out, nd, "out", nlev=nlev)[0]),
              "mimsem_elem_block_pc_build_levels(%s)" % op)
        return out

    def blocks_apply(self, form, blocks, x, transpose=False, alpha=1.0, accum=False, out=None, elem_scale=None):
        """y = alpha * sum_e P_e^T B_e P_e x with caller-supplied element blocks [nEl, nd, nd] (same on every level, optionally
        times elem_scale[lev, e]) or [nlev, nEl, nd, nd]; form 0/1/2 (1-forms: nd = 2*n1e, x-edges then y-edges)."""
        x2 = self._rows(x, self.sizes[form], "x")
        nlev = x2.shape[0]
        pb, bstride = self._blocks(blocks, {0: self.n0e, 1: 2 * self.n1e, 2: self.n2e}[form], "blocks", nlev=nlev)
        _need(elem_scale is None or blocks.dim() == 3, "elem_scale goes with one set of blocks [nEl, nd, nd]")
        y, y2 = self._out(out, nlev, self.sizes[form])
        check(self.L.mimsem_elem_blocks_apply(self.ctx, form, nlev, (4 if transpose else 0) | (2 if accum else 0), pb, bstride,
                                              *_ps(self._elem_scale(elem_scale, nlev)), *_ps(x2), *_ps(y2), alpha), "mimsem_elem_blocks_apply")
        return y if x.dim() == 2 else y2[0]

    def tsw_diagnose(self, h, S, u, m2inv, s=None, Phi=None, h2=None):
        """mimsem_tsw_diagnose: s = M2h(h)^-1 M2 S, Phi = K(u) u + 1/2 M2 S + 1/4 M2h(s) h, h2 = M2^-1 M2h(h) h in one launch
        (src/ThermalSW_EEC_2.cpp diagnose_s, diagnose_Phi, rhs_u).  h, S: 2-form rows, u: a 1-form row, m2inv: the WMATINV element
        matrices [nEl, n2e * n2e]."""
        n1, n2 = self.sizes[1], self.sizes[2]
        v = lambda t, n, name: self._vec(t, n, name)
        s = torch.empty_like(h) if s is None else s
        Phi = torch.empty_like(h) if Phi is None else Phi
        h2 = torch.empty_like(h) if h2 is None else h2
        check(self.L.mimsem_tsw_diagnose(self.ctx, v(h, n2, "h"), v(S, n2, "S"), v(u, n1, "u"), v(m2inv, self.nEl * self.n2e * self.n2e, "m2inv"),
                                         v(s, n2, "s"), v(Phi, n2, "Phi"), v(h2, n2, "h2")), "mimsem_tsw_diagnose")
        return s, Phi, h2

    def tsw_update(self, F, G, grad_s, s, m2inv, h_i, S_i, h_j, S_j, alpha, beta, dt):
        """mimsem_tsw_update: h_j <- alpha h_i + beta (h_j - dt E21 F), S_j <- alpha S_i + beta S_j - beta dt M2^-1 fS with
        fS = 1/2 M2 E21 G + 1/2 M2h(s) E21 F + K(grad_s) F (src/ThermalSW_EEC_2.cpp solve_rk, rhs_S), h_j and S_j in place"""
        n1, n2 = self.sizes[1], self.sizes[2]
        v = lambda t, n, name: self._vec(t, n, name)
        check(self.L.mimsem_tsw_update(self.ctx, v(F, n1, "F"), v(G, n1, "G"), v(grad_s, n1, "grad_s"), v(s, n2, "s"),
                                       v(m2inv, self.nEl * self.n2e * self.n2e, "m2inv"), v(h_i, n2, "h_i"), v(S_i, n2, "S_i"), v(h_j, n2, "h_j"),
                                       v(S_j, n2, "S_j"), alpha, beta, dt), "mimsem_tsw_update")
        return h_j, S_j

    def wvec(self, rho, lev0=0, scale=1.0, vert_scale=True, out=None):
        """Wvec::assemble(lev, scale, vert_scale, rho) (eul/Assembly.cpp:2457-2495; row B18): the matrix-free 2-form right-hand side
        W^T diag(w s/det [thickInv]) W rho -- Wmat applied to rho.  (The reference leaves its Wt table unfilled and has every call
        commented out; this is the evident intent, see oracle/o_assembly.c.)"""
        return self.apply("WMAT", rho, lev0=lev0, scale=scale, flags=FLAG_VERT if vert_scale else 0, out=out)

    def wvec_K(self, vel1, vel2, lev0=0, scale=1.0, out=None):
        """Wvec::assemble_K(lev, scale, vel1, vel2) (eul/Assembly.cpp:2497-2545): the kinetic-energy 2-form 1/2 <vel2, vel1> as a
        vector -- WtQUmat(vel2) applied to vel1"""
        return self.apply("WTQUMAT", vel1, f=vel2, lev0=lev0, scale=scale, out=out)

    def pvec(self, lev0=0, nlev=1, scale=1.0, h2=None):
        y = self._new(nlev, self.sizes[0])
        check(self.L.mimsem_pvec(self.ctx, lev0, nlev, scale, *_ps(self._rows(h2, self.sizes[2], "h2", min_rows=nlev, optional=True)), *_ps(y)), "mimsem_pvec")
        return y

    def incidence(self, which, x):
        """which: 'E10','E21','E12','E01'"""
        w = dict(E10=0, E21=1, E12=2, E01=3)[which]
        x2 = self._rows(x, self.sizes[(0, 1, 2, 1)[w]], "x of " + which)
        y = self._new(x2.shape[0], self.sizes[(1, 2, 1, 0)[w]])      # (every entry is written: faces directly, edges / nodes by the gather pass over all slots)
        check(self.L.mimsem_incidence_apply(self.ctx, w, x2.shape[0], *_ps(x2), *_ps(y)), "incidence")
        return y if x.dim() == 2 else y[0]

    def interp_quad(self, form, x, push_forward=True):
        """Row A7, Geom::interp0 / interp1_l|_g / interp2_l|_g (eul/Geom.cpp:328-417) at every quadrature point:
        x [nlev, n_form] (or [n_form]) -> [nlev, nEl, mp12] (forms 0, 2) or [nlev, nEl, mp12, 2] (1-forms)."""
        x2 = self._rows(x, self.sizes[form], "x")
        out = self._new(x2.shape[0], self.nEl * self.mp12 * (2 if form == 1 else 1))
        check(self.L.mimsem_interp_quad(self.ctx, form, 1 if push_forward else 0, x2.shape[0], *_ps(x2), *_ps(out)), "interp_quad")
        out = out.view(x2.shape[0], self.nEl, self.mp12, 2) if form == 1 else out.view(x2.shape[0], self.nEl, self.mp12)
        return out if x.dim() == 2 else out[0]

    def energetics_horiz(self, velx, rho, rt, exner, theta, out=None):
        """mimsem_euler_energetics_horiz: [keh, ie, entr, mass] of Euler::diagnostics (eul/Euler_2.cpp:600-744) over the rows' levels
        0 .. nlev-1 as a device tensor of 4; velx [nlev, n1], the others [nlev, n2] (rows contiguous, any row stride)"""
        vx = self._rows(velx, self.sizes[1], "velx", strided="r")
        nlev = vx.shape[0]
        r2, t2, e2, th2 = self._like(self.sizes[2], nlev, strided="r", rho=rho, rt=rt, exner=exner, theta=theta)
        out = self._new(4) if out is None else out
        ps = _ps if nlev > 1 else (lambda v2: (_ps(v2)[0], 0))                       # (one level: row stride 0)
        check(self.L.mimsem_euler_energetics_horiz(self.ctx, nlev, *ps(vx), *ps(r2), *ps(t2), *ps(e2), *ps(th2), self._vec(out, 4, "out")),
              "euler_energetics_horiz")
        return out

    def energetics_column(self, velz, rho, zv, out=None):
        """mimsem_euler_energetics_column: [kev, k2p, p2k, pe] of Euler::diagnostics (eul/Euler_2.cpp:638-664, :675-684) as a device tensor
        of 4; velz [nEl, (nk-1) n2e], rho and zv [nEl, nk n2e] in the vertical layout.  Orders 1..4.  The LINEAR_INV blocks the kernel reads
        are made on the first call and kept: they depend on the geometry only, and a context's geometry (its levels included) is fixed when
        the DeviceMesh is made"""
        _need(self.nk >= 2, "energetics_column needs at least one interface (nk >= 2)")
        self._col(velz, self.nk - 1, "velz"); self._col(rho, self.nk, "rho"); self._col(zv, self.nk, "zv")
        out = self._new(4) if out is None else out
        if self._linear_inv is None:                        # (first call: one allocation and the launches of colop_blocks -- warm up before recording)
            self._linear_inv = self.colop_blocks("LINEAR_INV")
        check(self.L.mimsem_euler_energetics_column(self.ctx, _ptr(velz), _ptr(rho), _ptr(zv), _ptr(self._linear_inv), self._vec(out, 4, "out")),
              "euler_energetics_column")
        return out

    def log_entropy(self, theta, lz, factor=1.0, out=None):
        """mimsem_euler_log_entropy: factor sum_r lz[r] sum_e sum_q Q_q log((W theta_r)_q), the entropy of the box's energetics line
        (box/Euler_2.cpp:979-997), as a device tensor of 1; theta [nrows, n2] (rows contiguous, any row stride; nrows is not bound by the
        context's nk), lz [nrows]"""
        th = self._rows(theta, self.sizes[2], "theta", min_rows=1, strided="r")
        nrows = th.shape[0]
        out = self._new(1) if out is None else out
        ps = _ps if nrows > 1 else (lambda v2: (_ps(v2)[0], 0))                      # (one row: row stride 0)
        check(self.L.mimsem_euler_log_entropy(self.ctx, nrows, *ps(th), self._vec(lz, nrows, "lz"), float(factor), self._vec(out, 1, "out")),
              "euler_log_entropy")
        return out

    def bernoulli(self, velx1, velx2, velz1, velz2, scale=1.0, out=None):
        """mimsem_horiz_bernoulli: HorizSolve::diagnose_Phi (eul/HorizSolve.cpp:419-470) of every level in one launch; velx1, velx2 [nk, n1],
        velz1, velz2 [nk-1, n2] (horizontal layout) -> Phi [nk, n2].  Rows contiguous, any row stride (the two of a pair share it); velx1 is
        velx2 and velz1 is velz2 are allowed"""
        x1 = self._rows(velx1, self.sizes[1], "velx1", min_rows=2, strided="r")          # (at least one interface: nk >= 2)
        nk = x1.shape[0]
        x2 = self._rows(velx2, self.sizes[1], "velx2", rows=nk, strided="r")
        z1, z2 = self._like(self.sizes[2], nk - 1, strided="r", velz1=velz1, velz2=velz2)
        _need(x1.stride(0) == x2.stride(0), "velx1, velx2: one row stride")
        _need(z1 is not None and z2 is not None and (nk == 2 or z1.stride(0) == z2.stride(0)), "velz1, velz2: [nk-1, n2] with one row stride")
        out, o2 = self._out(out, nk, self.sizes[2], exact=True, strided="w")
        check(self.L.mimsem_horiz_bernoulli(self.ctx, nk, _ps(x1)[0], *_ps(x2), _ps(z1)[0], _ps(z2)[0], z1.stride(0) if nk > 2 else 0, scale, *_ps(o2)),
              "horiz_bernoulli")
        return out

    def flux_rhs(self, u1, u2, h1, h2, scale=1.0, out=None):
        """mimsem_horiz_flux_rhs: the assembled mass-flux right-hand side sum_ab c_ab Uvec::assemble_hu(u_a, h_b) of HorizSolve::diagnose_fluxes
        and momentum_rhs (eul/HorizSolve.cpp:298-306, :538-547) of every level in two launches; u1, u2 [nk, n1], h1, h2 [nk, n2] -> [nk, n1].
        Rows contiguous, any row stride (the two of a pair share it); u1 is u2 and h1 is h2 are allowed, out must not overlap an input"""
        x1 = self._rows(u1, self.sizes[1], "u1", min_rows=1, strided="r")
        nk = x1.shape[0]
        x2 = self._rows(u2, self.sizes[1], "u2", rows=nk, strided="r")
        r1, r2 = self._like(self.sizes[2], nk, strided="r", h1=h1, h2=h2)
        _need(nk <= self.nk, "u1: at most the context's %d levels" % self.nk)
        _need(nk == 1 or x1.stride(0) == x2.stride(0), "u1, u2: one row stride")
        _need(r1 is not None and r2 is not None and (nk == 1 or r1.stride(0) == r2.stride(0)), "h1, h2: [nk, n2] with one row stride")
        out, o2 = self._out(out, nk, self.sizes[1], exact=True, strided="w")
        ins = [_ps(t)[0] for t in (x1, x2, r1, r2)]
        _need(_ps(o2)[0] not in ins, "out: must not be an input")
        ld = (lambda t: t.stride(0)) if nk > 1 else (lambda t: 0)                    # (one level: row stride 0)
        check(self.L.mimsem_horiz_flux_rhs(self.ctx, nk, ins[0], ins[1], ld(x2), ins[2], ins[3], ld(r2), scale, _ps(o2)[0], ld(o2)), "horiz_flux_rhs")
        return out

    def momentum_forcing(self, rot=None, pgf=None, vor=None, scale=1.0, flags=0, out=None):
        """mimsem_horiz_momentum_forcing: the element-local forcing of HorizSolve::momentum_rhs (eul/HorizSolve.cpp:496-635,
        box/HorizSolve.cpp:412-526) of every level in two launches:
            out_k (+)= R(q_k) a_k + F(th_k; const_vert per FLAG_VERT) g_k + 1/2 sum_{i in {k-1, k}, 0 <= i <= nk-2} Rh(dz_i) v_i
        rot = (q [nk, n0], a [nk, n1]), pgf = (th [nk, n2], g [nk, n1]), vor = (dz [nk-1, n1], v [nk-1, n2]); a pair left None is an absent
        term (vor must be None with one level).  flags: FLAG_ACCUM adds onto `out` (then required), FLAG_VERT.  The library takes packed
        rows only: a strided view is made contiguous here.  out [nk, n1] is one contiguous block and must not be an input"""
        s = self.sizes
        _need(not (flags & ~(FLAG_VERT | FLAG_ACCUM)), "flags: FLAG_VERT and FLAG_ACCUM only")
        pairs = []
        for name, pair in (("rot", rot), ("pgf", pgf), ("vor", vor)):
            _need(pair is None or (len(pair) == 2 and pair[0] is not None and pair[1] is not None), name + ": a pair of two tensors or None")
            pairs.append((None, None) if pair is None else tuple(t if t.is_contiguous() else t.contiguous() for t in pair))
        (q, a), (th, g), (dz, v) = pairs
        nrows = lambda t: t.shape[0] if t.dim() == 2 else 1
        if a is not None or g is not None:                                       # the level count: from the first term given, else from out
            nk = nrows(a if a is not None else g)
        elif dz is not None:
            nk = nrows(dz) + 1
        else:
            _need(out is not None, "all three terms absent and no out")
            nk = nrows(out)
        _need(1 <= nk <= self.nk, "at most the context's %d levels" % self.nk)
        _need(dz is None or nk >= 2, "vor: one level has no interface")
        q2, a2 = self._rows(q, s[0], "rot[0]", rows=nk, optional=True), self._rows(a, s[1], "rot[1]", rows=nk, optional=True)
        t2, g2 = self._rows(th, s[2], "pgf[0]", rows=nk, optional=True), self._rows(g, s[1], "pgf[1]", rows=nk, optional=True)
        d2, v2 = self._rows(dz, s[1], "vor[0]", rows=nk - 1, optional=True), self._rows(v, s[2], "vor[1]", rows=nk - 1, optional=True)
        _need(out is not None or not (flags & FLAG_ACCUM), "FLAG_ACCUM needs out")
        out, o2 = self._out(out, nk, s[1], exact=True)
        ins = [_ps(t)[0] for t in (q2, a2, t2, g2, d2, v2)]
        _need(_ps(o2)[0] not in ins, "out: must not be an input")
        check(self.L.mimsem_horiz_momentum_forcing(self.ctx, nk, flags, scale, *ins, _ps(o2)[0]), "horiz_momentum_forcing")
        return out

    def zonal_plan(self, band, nb=None):
        """mimsem_zonal_plan_build: band [nEl, mp12] (host integers) names the band in [0, nb) of every quadrature point of every element,
        -1 leaves a point out; nb: the number of bands (default: the largest value + 1).  The library validates the table and keeps the
        sorted point list on the device; a second call replaces it.  Returns nb"""
        b, addr = _host(np.asarray(band), np.int32)
        _need(b.shape == (self.nEl, self.mp12), "band: [nEl=%d, mp12=%d] integers, got %s" % (self.nEl, self.mp12, b.shape))
        nb = int(b.max()) + 1 if nb is None else int(nb)
        _need(nb >= 1 and int(b.min()) >= -1 and int(b.max()) < nb, "band: values in [-1, nb), nb >= 1")
        check(self.L.mimsem_zonal_plan_build(self.ctx, addr, nb), "zonal_plan_build")
        self._zonal_nb = nb
        return nb

    def zonal_moments(self, velx, rho, rt, exner, acc):
        """mimsem_euler_zonal_moments: acc [9, nlev, nb] += the band sums of a {1, u, v, T, uu, vv, uv, vT, TT} of the physical fields of
        velx [nlev, n1], rho, rt, exner [nlev, n2] over the bands of zonal_plan, in one launch.  The library takes packed rows only: a
        strided view is made contiguous here.  acc is one contiguous block and must not be an input"""
        nb = self._zonal_nb
        _need(nb > 0, "zonal_moments: no plan (Engine.zonal_plan)")
        ins = [t if t is None or t.is_contiguous() else t.contiguous() for t in (velx, rho, rt, exner)]
        vx = self._rows(ins[0], self.sizes[1], "velx", min_rows=1)
        nlev = vx.shape[0]
        _need(nlev <= self.nk, "velx: at most the context's %d levels" % self.nk)
        r2, t2, e2 = self._like(self.sizes[2], nlev, rho=ins[1], rt=ins[2], exner=ins[3])
        _need(r2 is not None and t2 is not None and e2 is not None, "rho, rt, exner: [nlev, n2] required")
        _need(acc is not None and tuple(acc.shape) == (9, nlev, nb), "acc: [9, nlev=%d, nb=%d] required" % (nlev, nb))
        pa = self._vec(acc, 9 * nlev * nb, "acc")
        ptrs = [_ps(t)[0] for t in (vx, r2, t2, e2)]
        _need(pa not in ptrs, "acc: must not be an input")
        check(self.L.mimsem_euler_zonal_moments(self.ctx, nlev, *ptrs, pa), "euler_zonal_moments")
        return acc

    def _sw_rows(self, x, out):
        """packed rows [u | h] of the sw_operator family (contiguous rows, any row stride): the view of x, the result and its view"""
        x2 = self._rows(x, self.sizes[1] + self.sizes[2], "x", strided="r")
        return (x2,) + self._out(out, x2.shape[0], x2.shape[1], strided="w")

    def _sw_f0(self, f0, nlev):
        """(address, stride) of the Coriolis rows f0 [n0] or [1, n0] (one row for all: stride 0) or [nlev, n0]"""
        f2 = self._rows(f0, self.sizes[0], "f0", strided="r")
        _need(f2.shape[0] in (1, nlev), "f0: one row, or one per row of x")
        return _ps(f2)[0], 0 if f2.shape[0] == 1 else f2.stride(0)

    def sw_operator(self, a, grav, H, f0, x, out=None):
        """SWEqn::assemble_operator + MatMult (src/SWEqn_Picard.cpp:622-725) in one element pass: x, y packed rows [u | h]"""
        x2, y, y2 = self._sw_rows(x, out)
        check(self.L.mimsem_sw_operator_apply(self.ctx, x2.shape[0], a, grav, H, *self._sw_f0(f0, x2.shape[0]), *_ps(x2), *_ps(y2)), "sw_operator")
        return y if (x.dim() == 2 or out is not None) else y[0]

    def sw_operator_precond(self, a, grav, H, f0, blocks, x, out=None):
        """z = P (A x) in three launches (mimsem_sw_operator_precond_apply): the Krylov body of the shallow-water solve"""
        x2, z, z2 = self._sw_rows(x, out)
        check(self.L.mimsem_sw_operator_precond_apply(self.ctx, x2.shape[0], a, grav, H, *self._sw_f0(f0, x2.shape[0]),
                                                      self._blocks(blocks, 2 * self.n1e + self.n2e, "blocks")[0], *_ps(x2), *_ps(z2)), "sw_operator_precond")
        return z if (x.dim() == 2 or out is not None) else z[0]

    def sw_operator_precond_chebyshev(self, a, grav, H, f0, blocks, ca, cb, x, r, d):
        """one Chebyshev step on B = P A in three launches (mimsem_sw_operator_precond_chebyshev): x += d; r -= P A d; d = ca d + cb r, in place"""
        x2 = self._rows(x, self.sizes[1] + self.sizes[2], "x")
        r2, d2 = self._like(x2.shape[1], x2.shape[0], r=r, d=d)
        check(self.L.mimsem_sw_operator_precond_chebyshev(self.ctx, x2.shape[0], a, grav, H, *self._sw_f0(f0, x2.shape[0]),
                                                          self._blocks(blocks, 2 * self.n1e + self.n2e, "blocks")[0], float(ca), float(cb),
                                                          *_ps(x2), *_ps(r2), *_ps(d2)), "sw_operator_precond_chebyshev")

    def sw_operator_precond_orthogonalize(self, a, grav, H, f0, blocks, x, V, k, h, out, alpha=-1.0):
        """out = P (A x); h[:k] = V[:k] out; out += alpha V[:k]^T h -- the Krylov body and the first Gram-Schmidt pass of the Arnoldi step in four
        launches (mimsem_sw_operator_precond_orthogonalize; bit-identical to sw_operator_precond + orthogonalize, which take five)"""
        n = self.sizes[1] + self.sizes[2]
        _need(k >= 0, "k >= 0")
        check(self.L.mimsem_sw_operator_precond_orthogonalize(self.ctx, a, grav, H, self._vec(f0, self.sizes[0], "f0"),
                                                              self._blocks(blocks, 2 * self.n1e + self.n2e, "blocks")[0], self._vec(x, n, "x"), self._vec(out, n, "out"),
                                                              k, *_ps(self._rows(V, n, "V", min_rows=k)), alpha, self._vec(h, k, "h", atleast=True)),
              "sw_operator_precond_orthogonalize")
        return out

    def sw_blocks_apply(self, blocks, x, out=None):
        """z = sum_e R_e^T B_e R_e x on packed rows [u | h]; blocks [nEl, ND, ND] stored column-major per element (mimsem_sw_blocks_apply)"""
        x2, y, y2 = self._sw_rows(x, out)
        check(self.L.mimsem_sw_blocks_apply(self.ctx, x2.shape[0], self._blocks(blocks, 2 * self.n1e + self.n2e, "blocks")[0], *_ps(x2), *_ps(y2)), "sw_blocks_apply")
        return y if (x.dim() == 2 or out is not None) else y[0]

    # ---- column operators -------------------------------------------------------------------
    def _col(self, t, slots, name, optional=False):
        """a "vertical" array [nEl, slots*n2e] (L2Vecs::vz of every column)"""
        if t is None:
            _need(optional, name + " is required")
            return
        if not (t.dim() == 2 and t.shape[0] == self.nEl and t.shape[1] == slots * self.n2e):
            _need(False, "%s must be [nEl=%d, %d*n2e=%d], got %s" % (name, self.nEl, slots, slots * self.n2e, tuple(t.shape)))

    def _cols(self, slots):
        """a new vertical array [nEl, slots*n2e]"""
        return self._new(self.nEl, slots * self.n2e)

    def _colop_slots(self, colop, transpose=False):
        """(input slots, output slots) of a column operator in units of n2e (eul/VertOps.cpp: rows x cols of each Assemble*)"""
        nk = self.nk
        rc = dict(CONST=(nk, nk), CONST_INV=(nk, nk), CONST_RHO=(nk, nk), CONST_RHO_INV=(nk, nk), CONST_THETA=(nk, nk), EOS_BLOCK=(nk, nk),
                  EOS_BLOCK_INV=(nk, nk), LINEAR=(nk - 1, nk - 1), LINEAR_INV=(nk - 1, nk - 1), LINEAR_RT=(nk - 1, nk - 1),
                  LINEAR_THETA=(nk - 1, nk - 1), RAYLEIGH=(nk - 1, nk - 1), LINEAR_RAYLEIGH_INV=(nk - 1, nk - 1),
                  LINEAR_RHO2=(nk + 1, nk + 1), LINEAR_RHO2_UP=(nk + 1, nk + 1), LINCON=(nk - 1, nk), LINCON2=(nk + 1, nk), LINCON2_UP=(nk + 1, nk),
                  CONLIN=(nk, nk - 1), CONLIN_W=(nk, nk - 1), CONLIN_RHODPI=(nk, nk - 1))[colop]
        rows, cols = rc
        return (rows, cols) if transpose else (cols, rows)

    _COLOP_F1 = dict(CONST_RHO="nk", CONST_RHO_INV="nk", CONST_THETA="nk+1", EOS_BLOCK="nk", EOS_BLOCK_INV="nk", LINEAR_RT="nk", LINEAR_THETA="nk+1",
                     LINEAR_RHO2="nk", LINEAR_RHO2_UP="nk", CONLIN_W="nk-1", CONLIN_RHODPI="nk")

    def _check_colop(self, colop, f1, f2, x=None, nout_slots=None, transpose=False, uh=None):
        _need(colop in COLOPS, "unknown column operator %r" % (colop,))
        nk = self.nk
        if colop in self._COLOP_F1:
            self._col(f1, eval(self._COLOP_F1[colop], {"nk": nk}), "f1 of " + colop)
        if colop == "CONLIN_RHODPI":
            self._col(f2, nk - 1, "f2 of CONLIN_RHODPI")
        if colop == "EOS_BLOCK_INV" and f2 is not None:
            self._col(f2, nk + 1, "f2 (theta) of EOS_BLOCK_INV")
        if colop in ("LINEAR_RHO2_UP", "LINCON2_UP"):
            _need(uh is not None and uh.dim() == 2 and uh.shape == (nk, self.sizes[1]), "uh of %s must be [nk, n1]" % colop)
        if x is not None:
            sin, sout = self._colop_slots(colop, transpose)
            self._col(x, sin, "x of " + colop)
            _need(nout_slots == sout, "%s%s maps %d -> %d slots; nout_slots=%r" % (colop, "^T" if transpose else "", sin, sout, nout_slots))

    def l2_horiz_to_vert(self, vh):
        _need(vh.dim() == 2 and vh.shape[1] == self.sizes[2] and vh.shape[0] in (self.nk - 1, self.nk, self.nk + 1), "vh must be [nk-1|nk|nk+1, n2], got %s" % (tuple(vh.shape),))
        nkv = vh.shape[0]
        vz = self._cols(nkv)
        check(self.L.mimsem_l2_transpose(self.ctx, 0, nkv, _ptr(vh), vh.stride(0), _ptr(vz)), "l2_transpose")
        return vz

    def l2_vert_to_horiz(self, vz, nkv):
        self._col(vz, nkv, "vz")
        vh = self._new(nkv, self.sizes[2])
        check(self.L.mimsem_l2_transpose(self.ctx, 1, nkv, _ptr(vh), vh.stride(0), _ptr(vz)), "l2_transpose")
        return vh

    def colop_blocks(self, colop, f1=None, f2=None, flags=0):
        self._check_colop(colop, f1, f2)
        out = self._new(self.nEl, self.L.mimsem_colop_nblocks(self.ctx, COLOPS[colop]), self.n2e, self.n2e)
        check(self.L.mimsem_colop_blocks(self.ctx, COLOPS[colop], flags, _ptr(f1), _ptr(f2), _ptr(out)), "colop_blocks(%s)" % colop)
        return out

    def colop_apply(self, colop, x, f1=None, f2=None, flags=0, transpose=False, nout_slots=None):
        """nout_slots: rows of the operator in units of n2e (required; checked against the operator's shape)"""
        self._check_colop(colop, f1, f2, x, nout_slots, transpose)
        y = self._cols(nout_slots)
        check(self.L.mimsem_colop_apply(self.ctx, COLOPS[colop], flags, int(transpose), _ptr(f1), _ptr(f2), _ptr(x), _ptr(y)),
              "colop_apply(%s)" % colop)
        return y

    def colop_apply_blocks(self, colop, blocks, x, nout_slots, transpose=False):
        """MatMult with blocks from colop_blocks (geometry-only operators assembled once)"""
        self._check_colop(colop, None, None, x, nout_slots, transpose)
        _need(blocks.dim() == 4 and blocks.shape[0] == self.nEl and blocks.shape[1] == self.L.mimsem_colop_nblocks(self.ctx, COLOPS[colop])
              and blocks.shape[2:] == (self.n2e, self.n2e), "blocks of %s have shape %s" % (colop, tuple(blocks.shape)))
        y = self._cols(nout_slots)
        check(self.L.mimsem_colop_apply_blocks(self.ctx, COLOPS[colop], int(transpose), _ptr(blocks), _ptr(x), _ptr(y)),
              "colop_apply_blocks(%s)" % colop)
        return y

    def colop_blocks_ex(self, colop, param=0.0, f1=None, f2=None, uh=None, flags=0):
        """the Strang / Held-Suarez colops: param = dt_fric or dt, uh = [nk, n1] horizontal velocity (local 1-forms)"""
        self._check_colop(colop, f1, f2, uh=uh)
        out = self._new(self.nEl, self.L.mimsem_colop_nblocks(self.ctx, COLOPS[colop]), self.n2e, self.n2e)
        check(self.L.mimsem_colop_blocks_ex(self.ctx, COLOPS[colop], flags, param, _ptr(f1), _ptr(f2), _ptr(uh),
                                            uh.stride(0) if uh is not None else 0, _ptr(out)), "colop_blocks_ex(%s)" % colop)
        return out

    def colop_apply_ex(self, colop, x, nout_slots, param=0.0, f1=None, f2=None, uh=None, flags=0, transpose=False):
        self._check_colop(colop, f1, f2, x, nout_slots, transpose, uh=uh)
        y = self._cols(nout_slots)
        check(self.L.mimsem_colop_apply_ex(self.ctx, COLOPS[colop], flags, int(transpose), param, _ptr(f1), _ptr(f2), _ptr(uh),
                                           uh.stride(0) if uh is not None else 0, _ptr(x), _ptr(y)), "colop_apply_ex(%s)" % colop)
        return y

    def column_incidence(self, which, x):
        """'V10' | 'V01' | 'V10_full' applied to every column (VertOps::vertOps)"""
        w = dict(V10=0, V01=1, V10_full=2)[which]
        self._col(x, (self.nk - 1, self.nk, self.nk + 1)[w], "x of " + which)
        y = self._cols(self.nk - 1 if w == 1 else self.nk)
        check(self.L.mimsem_column_incidence(self.ctx, w, _ptr(x), _ptr(y)), "column_incidence")
        return y

    def diag_theta_up(self, dt, rho, rt, uh):
        self._col(rho, self.nk, "rho"); self._col(rt, self.nk, "rt")
        _need(uh.dim() == 2 and uh.shape == (self.nk, self.sizes[1]), "uh must be [nk, n1]")
        th = self._cols(self.nk + 1)
        check(self.L.mimsem_column_diag_theta_up(self.ctx, dt, _ptr(rho), _ptr(rt), _ptr(uh), uh.stride(0), _ptr(th)), "diag_theta_up")
        return th

    def temp_forcing_hs(self, lat, exner, theta, rho):
        _need(lat.dim() == 2 and lat.shape == (self.nEl, self.mp12), "lat must be [nEl, mp12] (latitude of the quadrature points)")
        self._col(exner, self.nk, "exner"); self._col(theta, self.nk + 1, "theta"); self._col(rho, self.nk, "rho")
        out = self._cols(self.nk)
        check(self.L.mimsem_column_temp_forcing_hs(self.ctx, _ptr(lat), _ptr(exner), _ptr(theta), _ptr(rho), _ptr(out)), "temp_forcing_hs")
        return out

    def _col_ptrs(self, *named):
        """the addresses of vertical arrays given as (tensor, slots, name) triples, each checked by _col (and _ptr)"""
        for t, slots, name in named:
            self._col(t, slots, name)
        return [_ptr(t) for t, _, _ in named]

    def solve_schur_3(self, dt, theta, velz, rho, rt, pi, F_u, F_rho, F_rt, F_pi, want_L=False, flags=0):
        """solve_schur_column_3 for every column; F_* updated in place; returns d_u, d_rho, d_rt, d_pi (, L [nEl,nk,5,n2e,n2e]);
        flags = 3 reproduces the box twin (box/VertSolve.cpp:879-1058)"""
        nk = self.nk
        ins = self._col_ptrs((theta, nk + 1, "theta"), (velz, nk - 1, "velz"), (rho, nk, "rho"), (rt, nk, "rt"), (pi, nk, "pi"),
                             (F_u, nk - 1, "F_u"), (F_rho, nk, "F_rho"), (F_rt, nk, "F_rt"), (F_pi, nk, "F_pi"))
        d_u, d_rho, d_rt, d_pi = self._cols(nk - 1), self._cols(nk), self._cols(nk), self._cols(nk)
        L = self._new(self.nEl, self.nk, 5, self.n2e, self.n2e) if want_L else None
        check(self.L.mimsem_column_solve_schur_3(self.ctx, dt, flags, *ins, _ptr(d_u), _ptr(d_rho), _ptr(d_rt), _ptr(d_pi), _ptr(L)), "solve_schur_3")
        return (d_u, d_rho, d_rt, d_pi, L) if want_L else (d_u, d_rho, d_rt, d_pi)

    def column_eos(self, which, a, b=None, p0=0.0, p1=0.0):
        _need(which in (0, 1, 2, 3), "column_eos which = 0..3")
        self._col(a, self.nk, "a"); self._col(b, self.nk, "b", optional=which in (1, 2))
        out = self._cols(self.nk)
        check(self.L.mimsem_column_eos(self.ctx, which, _ptr(a), _ptr(b), p0, p1, _ptr(out)), "column_eos")
        return out

    def diag_theta(self, which, rho, rt):
        _need(which in (0, 1), "diag_theta which = 0 (diagTheta_L2) | 1 (diagTheta2)")
        self._col(rho, self.nk, "rho"); self._col(rt, self.nk, "rt")
        th = self._cols(self.nk + (1 if which == 1 else 0))
        check(self.L.mimsem_column_diag_theta(self.ctx, which, _ptr(rho), _ptr(rt), _ptr(th)), "diag_theta")
        return th

    def diag_theta_blend(self, rho, rt, blend2=None, blendL=None, wa=1.0, wb=0.0, want2=True, wantL=True):
        """diagTheta2 and diagTheta_L2 in ONE launch, optionally blended with earlier fields: wa * theta(rho, rt) + wb * blend
        (mimsem_column_diag_theta_blend).  Returns (theta2 [nEl, (nk+1) n2e] | None, thetaL [nEl, nk n2e] | None)."""
        self._col(rho, self.nk, "rho"); self._col(rt, self.nk, "rt")
        self._col(blend2, self.nk + 1, "blend2", optional=True); self._col(blendL, self.nk, "blendL", optional=True)
        th2 = self._cols(self.nk + 1) if want2 else None
        thL = self._cols(self.nk) if wantL else None
        check(self.L.mimsem_column_diag_theta_blend(self.ctx, _ptr(rho), _ptr(rt), _ptr(th2), _ptr(blend2), _ptr(thL), _ptr(blendL), wa, wb),
              "diag_theta_blend")
        return th2, thL

    def diag_theta_wup(self, dtw, rho, rt, velz, blend2=None, wa=1.0, wb=0.0):
        """diagTheta2 of the box twin (box/VertSolve.cpp:499-531): theta on the nk+1 interfaces with the test functions upwinded by the
        vertical velocity velz [nEl, (nk-1) n2e] over dtw, optionally blended: wa * theta(rho, rt, velz) + wb * blend2
        (mimsem_column_diag_theta_wup; |dtw w| < 1 is the caller's to keep)"""
        self._col(rho, self.nk, "rho"); self._col(rt, self.nk, "rt"); self._col(velz, self.nk - 1, "velz")
        self._col(blend2, self.nk + 1, "blend2", optional=True)
        th2 = self._cols(self.nk + 1)
        check(self.L.mimsem_column_diag_theta_wup(self.ctx, dtw, _ptr(rho), _ptr(rt), _ptr(velz), _ptr(th2), _ptr(blend2), wa, wb),
              "diag_theta_wup")
        return th2

    def newton_residual(self, dt, rayleigh, theta, Pi, velz_i, velz_j, rho_i, rho_j, zv, rt_i, rt_j, rho_h, rt_h, exner_j,
                        add_w=None, add_rho=None, add_rt=None):
        """mimsem_column_newton_residual: (F_w, F_rho, F_eta, F_exner, th_w3, eta, k2i) for every column (VertSolve.cpp:1806-1851)"""
        nk = self.nk
        ins = self._col_ptrs((theta, nk, "theta"), (Pi, nk, "Pi"), (velz_i, nk - 1, "velz_i"), (velz_j, nk - 1, "velz_j"), (rho_i, nk, "rho_i"),
                             (rho_j, nk, "rho_j"), (zv, nk, "zv"), (rt_i, nk, "rt_i"), (rt_j, nk, "rt_j"), (rho_h, nk, "rho_h"), (rt_h, nk, "rt_h"),
                             (exner_j, nk, "exner_j"))
        self._col(add_w, nk - 1, "add_w", optional=True); self._col(add_rho, nk, "add_rho", optional=True); self._col(add_rt, nk, "add_rt", optional=True)
        outs = [self._cols(s) for s in (nk - 1, nk, nk, nk, nk, nk, nk - 1)]          # F_w, F_rho, F_eta, F_exner, th_w3, eta, k2i
        check(self.L.mimsem_column_newton_residual(self.ctx, dt, rayleigh, *ins, _ptr(add_w), _ptr(add_rho), _ptr(add_rt), *[_ptr(t) for t in outs]),
              "newton_residual")
        return tuple(outs)

    def _newton_update(self, fn, what, d3, d_w, d_rho, d_3, d_exner, velz_i, rho_i, rt_i, exner_i, velz_j, rho_j, rt_j, exner_j):
        """the one body of newton_update and newton2_update (d3: the name of the third correction, d_eta or d_rt)"""
        nk = self.nk
        ins = self._col_ptrs((d_w, nk - 1, "d_w"), (d_rho, nk, "d_rho"), (d_3, nk, d3), (d_exner, nk, "d_exner"), (velz_i, nk - 1, "velz_i"),
                             (rho_i, nk, "rho_i"), (rt_i, nk, "rt_i"), (exner_i, nk, "exner_i"), (velz_j, nk - 1, "velz_j"), (rho_j, nk, "rho_j"),
                             (rt_j, nk, "rt_j"), (exner_j, nk, "exner_j"))
        velz_h, rho_h, rt_h, exner_h = self._cols(nk - 1), self._cols(nk), self._cols(nk), self._cols(nk)
        nrm = self._new(8, self.nEl, nk * self.n2e)
        check(fn(self.ctx, *ins, _ptr(velz_h), _ptr(rho_h), _ptr(rt_h), _ptr(exner_h), _ptr(nrm)), what)
        return velz_h, rho_h, rt_h, exner_h, nrm

    def newton_update(self, d_w, d_rho, d_eta, d_exner, velz_i, rho_i, rt_i, exner_i, velz_j, rho_j, rt_j, exner_j):
        """mimsem_column_newton_update: velz_j / rho_j / rt_j / exner_j are updated IN PLACE; returns (velz_h, rho_h, rt_h, exner_h, norm_squares
        [8, nEl, nk n2e]) (VertSolve.cpp:1858-1912)"""
        return self._newton_update(self.L.mimsem_column_newton_update, "newton_update", "d_eta", d_w, d_rho, d_eta, d_exner, velz_i, rho_i, rt_i, exner_i,
                                   velz_j, rho_j, rt_j, exner_j)

    def newton2_residual(self, dt, rayleigh, theta_h, Pi, velz_i, velz_j, rho_i, rho_j, zv, rt_i, rt_j, exner_j,
                         add_w=None, add_rho_pre=None, add_rt_pre=None, add_rt_post=None):
        """mimsem_column_newton2_residual: (F_w, F_rho, F_rt, F_exner, k2i) of VertSolve::solve_schur_2 for every column
        (VertSolve.cpp:1131-1154); theta_h on the nk+1 interfaces; the additions each enter times dt"""
        nk = self.nk
        ins = self._col_ptrs((theta_h, nk + 1, "theta_h"), (Pi, nk, "Pi"), (velz_i, nk - 1, "velz_i"), (velz_j, nk - 1, "velz_j"), (rho_i, nk, "rho_i"),
                             (rho_j, nk, "rho_j"), (zv, nk, "zv"), (rt_i, nk, "rt_i"), (rt_j, nk, "rt_j"), (exner_j, nk, "exner_j"))
        self._col(add_w, nk - 1, "add_w", optional=True); self._col(add_rho_pre, nk, "add_rho_pre", optional=True)
        self._col(add_rt_pre, nk, "add_rt_pre", optional=True); self._col(add_rt_post, nk, "add_rt_post", optional=True)
        outs = [self._cols(s) for s in (nk - 1, nk, nk, nk, nk - 1)]                  # F_w, F_rho, F_rt, F_exner, k2i
        check(self.L.mimsem_column_newton2_residual(self.ctx, dt, rayleigh, *ins, _ptr(add_w), _ptr(add_rho_pre), _ptr(add_rt_pre), _ptr(add_rt_post),
                                                    *[_ptr(t) for t in outs]), "newton2_residual")
        return tuple(outs)

    def newton2_update(self, d_w, d_rho, d_rt, d_exner, velz_i, rho_i, rt_i, exner_i, velz_j, rho_j, rt_j, exner_j):
        """mimsem_column_newton2_update: velz_j / rho_j / rt_j / exner_j are updated IN PLACE; returns (velz_h, rho_h, rt_h, exner_h, norm_squares
        [8, nEl, nk n2e]) (VertSolve.cpp:1159-1183)"""
        return self._newton_update(self.L.mimsem_column_newton2_update, "newton2_update", "d_rt", d_w, d_rho, d_rt, d_exner, velz_i, rho_i, rt_i, exner_i,
                                   velz_j, rho_j, rt_j, exner_j)

    def max_norms(self, nrm):
        """mimsem_column_max_norms: VertSolve::MaxNorm for the four pairs of newton_update's norm squares -> device tensor [4] (exner, w, rho, eta)"""
        ws, out = self._new(4, self.nEl), self._new(4)
        check(self.L.mimsem_column_max_norms(self.ctx, self._vec(nrm, 8 * self.nEl * self.nk * self.n2e, "nrm"), _ptr(ws), _ptr(out)), "column_max_norms")
        return out

    def helmholtz_blocks(self, dt, theta, rho, eta, pi):
        nk = self.nk
        ins = self._col_ptrs((theta, nk, "theta"), (rho, nk, "rho"), (eta, nk, "eta"), (pi, nk, "pi"))
        out = self._new(self.nEl, self.nk, 3, self.n2e, self.n2e)
        check(self.L.mimsem_column_helmholtz_blocks(self.ctx, dt, *ins, _ptr(out)), "helmholtz_blocks")
        return out

    def solve_schur_eta(self, dt, theta, rho, eta, pi, F_u, F_rho, F_eta, F_pi):
        """F_* are updated in place (as the reference does); returns d_u, d_rho, d_eta, d_pi"""
        nk = self.nk
        ins = self._col_ptrs((theta, nk, "theta"), (rho, nk, "rho"), (eta, nk, "eta"), (pi, nk, "pi"),
                             (F_u, nk - 1, "F_u"), (F_rho, nk, "F_rho"), (F_eta, nk, "F_eta"), (F_pi, nk, "F_pi"))
        d_u, d_rho, d_eta, d_pi = self._cols(nk - 1), self._cols(nk), self._cols(nk), self._cols(nk)
        check(self.L.mimsem_column_solve_schur_eta(self.ctx, dt, *ins, _ptr(d_u), _ptr(d_rho), _ptr(d_eta), _ptr(d_pi)), "solve_schur_eta")
        return d_u, d_rho, d_eta, d_pi

    def solve_status(self):
        """(columns whose refinement did not converge in the last solve_schur_eta, or -1 when that path keeps no status; per-column status
        array: 0 converged, 1 not converged, 2 refinement off, 3 re-solved by the pivoted fallback, 4 flagged for its conditioning only and accepted on its backward error (set_pivot_fallback); per-column |last correction| / |solution|) -- mimsem_column_solve_status"""
        n = C.c_int(-1)
        st, pst = _host(np.zeros(max(self.nEl, 1), dtype=np.int32), np.int32)
        ratio, pratio = _host(np.zeros(max(self.nEl, 1)), np.float64)
        check(self.L.mimsem_column_solve_status(self.ctx, C.byref(n), pst, pratio), "column_solve_status")
        return n.value, st[:self.nEl], ratio[:self.nEl]

    def flag_columns_for_test(self, columns):
        """test hook: the next column solve treats these columns as flagged by its block sweep (mimsem_column_flag_for_test)"""
        cols, p = _host(columns, np.int32)
        check(self.L.mimsem_column_flag_for_test(self.ctx, p, int(cols.size)), "column_flag_for_test")

    def set_pivot_fallback(self, on=True):
        """(on by default) solve_schur_eta / solve_schur_3 re-solve the columns their unpivoted sweep flags by an LU with partial pivoting over
        the band (what the reference's PCLU does for every column); verified re-solves report status 3; 0 switches it off --
        mimsem_column_set_pivot_fallback"""
        check(self.L.mimsem_column_set_pivot_fallback(self.ctx, int(on)), "column_set_pivot_fallback")      # (2: every column, validation mode)

    # ---- Krylov building blocks ----------------------------------------------------------------
    def _basis(self, V, w, k):
        """(k, n, address and row stride of V, address of w) as the Gram-Schmidt kernels take them: w one contiguous block of n entries, V at
        least k rows of length n (k None: all of them)"""
        k = V.shape[0] if k is None else k
        _need(k >= 0, "k >= 0")
        return (k, w.numel()) + _ps(self._rows(V, w.numel(), "V", min_rows=k)) + (self._vec(w, w.numel(), "w"),)

    def mdot(self, V, w, k=None, out=None):
        """h[i] = <V[i], w> for i < k; V: [m, n] contiguous rows"""
        k, n, pV, ldv, pw = self._basis(V, w, k)
        h = out if out is not None else self._new(k)
        check(self.L.mimsem_krylov_mdot(self.ctx, k, n, pV, ldv, pw, self._vec(h, k, "out", atleast=True)), "krylov_mdot")
        return h

    def maxpy(self, V, h, w, alpha=1.0, k=None):
        """w += alpha * sum_{i<k} h[i] V[i]  (in place)"""
        k, n, pV, ldv, pw = self._basis(V, w, k)
        check(self.L.mimsem_krylov_maxpy(self.ctx, k, n, pV, ldv, self._vec(h, k, "h", atleast=True), alpha, pw), "krylov_maxpy")
        return w

    def orthogonalize(self, V, w, h, k=None, alpha=-1.0):
        """one classical Gram-Schmidt pass in two launches: h[:k] = V[:k] w, then w += alpha V[:k]^T h (in place)"""
        k, n, pV, ldv, pw = self._basis(V, w, k)
        check(self.L.mimsem_krylov_orthogonalize(self.ctx, k, n, pV, ldv, alpha, pw, self._vec(h, k, "h", atleast=True)), "krylov_orthogonalize")
        return w

    def _gs_args(self, V, w, v, k, h1, h2, col, norm_slot):
        """the arguments cgs2 and reorthonormalize share: V, w as in _basis, v like w, h1 / h2 at least k entries, col (a _word) long enough
        for its k entries and for norm_slot"""
        _need(norm_slot >= 0, "norm_slot >= 0")
        return self._basis(V, w, k) + (self._vec(v, w.numel(), "v"), self._vec(h1, k, "h1", atleast=True), self._vec(h2, k, "h2", atleast=True),
                                       self._word(col, max(k, norm_slot + 1), "col"), norm_slot)

    def cgs2(self, V, w, v, k, h1, h2, col, norm_slot, flag=None):
        """both Gram-Schmidt passes of an Arnoldi step + normalisation + Hessenberg column in three launches (mimsem_krylov_cgs2)"""
        check(self.L.mimsem_krylov_cgs2(self.ctx, *self._gs_args(V, w, v, k, h1, h2, col, norm_slot), self._word(flag, 1, "flag", _I32)), "krylov_cgs2")

    def reorthonormalize(self, V, w, v, k, h1, h2, col, norm_slot, fused=None, flag=None):
        """second Gram-Schmidt pass + normalisation in two launches: h2[:k] = V[:k] w; w -= V[:k]^T h2; v = w/|w|;
        col[:k] = h1 + h2; col[norm_slot] = |w| (col: device or pinned host tensor).  fused / flag given: the explicit form
        (mimsem_krylov_reorthonormalize_ex: the caller's own flag word, nothing shared through the context)"""
        args = self._gs_args(V, w, v, k, h1, h2, col, norm_slot)
        if fused is not None:
            check(self.L.mimsem_krylov_reorthonormalize_ex(self.ctx, *args, 1 if fused else 0, self._word(flag, 1, "flag", _I32)), "krylov_reorthonormalize_ex")
            return
        check(self.L.mimsem_krylov_reorthonormalize(self.ctx, *args), "krylov_reorthonormalize")
        return v

    def normalize(self, w, v, k, h1, h2, col, norm_slot):
        """v = w/|w|; col[:k] = h1 + h2; col[norm_slot] = |w|.  col: device tensor or PINNED host tensor (written by the kernel)"""
        n = w.numel()
        _need(norm_slot >= 0, "norm_slot >= 0")
        check(self.L.mimsem_krylov_normalize(self.ctx, n, self._vec(w, n, "w"), self._vec(v, n, "v"), k, self._vec(h1, k, "h1", atleast=True, optional=True),
                                             self._vec(h2, k, "h2", atleast=True, optional=True), self._word(col, max(k, norm_slot + 1), "col"), norm_slot),
              "krylov_normalize")
        return v

    def _rowwise(self, **named):
        """operands of a row-wise update: [nrows, n] tensors of one shape -- that of the first --, each one contiguous block (None: an absent
        optional one); (nrows, n, their (address, stride) pairs in the order given)"""
        name, t = next(iter(named.items()))
        nrows, n = self._rows(t, None, name).shape
        return (nrows, n) + tuple(_ps(t2) for t2 in self._like(n, nrows, **named))

    def rowdot(self, A, B, out=None):
        """out[i] = <A[i], B[i]> for [nrows, n] tensors (rows contiguous)"""
        nrows, n, pA, pB = self._rowwise(A=A, B=B)
        out = out if out is not None else self._new(nrows)
        check(self.L.mimsem_krylov_rowdot(self.ctx, nrows, n, *pA, *pB, self._vec(out, nrows, "out", atleast=True)), "rowdot")
        return out

    def rowdot_local(self, A, B, out=None, space=None):
        """the rank's part of rowdot (one rank: all of it); DistEngine weights by ownership and leaves the all-reduce to the caller"""
        return self.rowdot(A, B, out=out)

    def cg_update(self, num, den, p, Ap, x, r):
        """x += (num/den) p ; r -= (num/den) Ap  row-wise, in place"""
        nrows, n, pp, pAp, px, pr = self._rowwise(p=p, Ap=Ap, x=x, r=r)
        check(self.L.mimsem_krylov_cg_update(self.ctx, nrows, n, self._vec(num, nrows, "num", atleast=True), self._vec(den, nrows, "den", atleast=True),
                                             *pp, *pAp, *px, *pr), "cg_update")

    def chebyshev_start(self, c, s, theta, r, d, x):
        """r = s c ; d = r / theta ; x = 0 row-wise (one launch: mimsem_krylov_chebyshev_start); r may be c"""
        nrows, n, px, pc, pr, pd = self._rowwise(x=x, c=c, r=r, d=d)
        check(self.L.mimsem_krylov_chebyshev_start(self.ctx, nrows, n, float(s), float(theta), *pc, *pr, *pd, *px), "chebyshev_start")

    def chebyshev_px(self, alpha, beta, y, p, x, b=None, dinv=None, upd=None):
        """z = dinv (b - y) (or y when dinv is None); p = z + beta p; x += alpha p; upd = z -- row-wise, one launch (mimsem_krylov_chebyshev_px: the
        vector algebra of a Chebyshev step on a sharded mesh, where the operator result is completed over the halo between the passes)"""
        nrows, n, px, py, pb, pdinv, pp, pupd = self._rowwise(x=x, y=y, b=b, dinv=dinv, p=p, upd=upd)
        check(self.L.mimsem_krylov_chebyshev_px(self.ctx, nrows, n, float(alpha), float(beta), *py, *pb, *pdinv, *pp, *px, *pupd), "chebyshev_px")

    def axpy_dots(self, dx, x, out):
        """x += dx ; out[0] = dx . dx ; out[1] = x . x over ALL entries of the (contiguous) tensors (one launch: mimsem_krylov_axpy_dots)"""
        check(self.L.mimsem_krylov_axpy_dots(self.ctx, x.numel(), self._vec(dx, x.numel(), "dx"), self._vec(x, x.numel(), "x"), self._vec(out, 2, "out")),
              "axpy_dots")

    def chebyshev_update(self, a, b, Bd, x, r, d):
        """x += d ; r -= Bd ; d = a d + b r  row-wise, in place (one launch: mimsem_krylov_chebyshev_update)"""
        nrows, n, px, pBd, pr, pd = self._rowwise(x=x, Bd=Bd, r=r, d=d)
        check(self.L.mimsem_krylov_chebyshev_update(self.ctx, nrows, n, float(a), float(b), *pBd, *px, *pr, *pd), "chebyshev_update")

    def cg_direction(self, num, den, z, p):
        """p = z + (num/den) p  row-wise, in place"""
        nrows, n, pp, pz = self._rowwise(p=p, z=z)
        check(self.L.mimsem_krylov_cg_direction(self.ctx, nrows, n, self._vec(num, nrows, "num", atleast=True), self._vec(den, nrows, "den", atleast=True),
                                                *pz, *pp), "cg_direction")

    def ratio_max(self, num, den, log):
        """log[i] = max(log[i], num[i] / max(den[i], 1e-300)), a NaN on either side kept: the check log of a fixed-length solve, in place
        (one launch: mimsem_krylov_ratio_max)"""
        nrows = log.numel()
        check(self.L.mimsem_krylov_ratio_max(self.ctx, nrows, self._vec(num, nrows, "num"), self._vec(den, nrows, "den"), self._vec(log, nrows, "log")),
              "ratio_max")
        return log

    def combine(self, a, alpha=1.0, op=None, b=None, beta=0.0, c=None, out=None):
        """out = alpha * (a, a*b or a/b) + beta * c, row by row ([nrows, n] tensors whose rows are contiguous; slices along the first
        dimension are fine); out may be a or c (mimsem_vec_combine)"""
        a2 = self._rows(a, None, "a", strided="r")
        nrows, n = a2.shape
        out = torch.empty_like(a2) if out is None else out
        opc = {None: 0, "mul": 1, "div": 2}[op]
        _need(not opc or b is not None, "combine: op needs b")
        b2, c2 = self._like(n, nrows, strided="r", b=b, c=c)
        check(self.L.mimsem_vec_combine(self.ctx, nrows, n, float(alpha), *_ps(a2), opc, *_ps(b2), float(beta), *_ps(c2),
                                        *_ps(self._rows(out, n, "out", rows=nrows, strided="w"))), "vec_combine")
        return out

    def interface_average(self, a, nk):
        """[nk-1, n] interface field -> [nk, n] level field, 0.5*(k-1) + 0.5*(k) with the missing boundary interfaces left out"""
        a2 = self._rows(a, None, "a", min_rows=nk - 1, strided="r")
        out = self._new(nk, a2.shape[1])
        check(self.L.mimsem_interface_average(self.ctx, nk, a2.shape[1], *_ps(a2), *_ps(out)), "interface_average")
        return out

    def _block_inverse(self, blocks, status):
        """the one body of block_inverse and block_inverse_status: (the inverses as a new tensor, the library's count of bad pivots)"""
        _need(blocks.dim() == 3 and blocks.shape[1] == blocks.shape[2] and blocks.dtype == _F64, "block_inverse: [nblocks, n, n] float64 tensor required")
        out = blocks.contiguous().clone()
        ns = C.c_int(0)
        if status:
            check(self.L.mimsem_block_inverse_status(self.ctx, out.shape[0], out.shape[1], _ptr(out), C.byref(ns)), "block_inverse_status")
        else:
            check(self.L.mimsem_block_inverse(self.ctx, out.shape[0], out.shape[1], _ptr(out)), "block_inverse")
        return out, ns.value

    def block_inverse(self, blocks):
        """inverse of every [n, n] block of a [nblocks, n, n] tensor by the library's batched Gauss-Jordan (mimsem_block_inverse);
        returns a new tensor"""
        return self._block_inverse(blocks, False)[0]

    def block_inverse_status(self, blocks):
        """block_inverse plus the number of blocks for which the reference's LinAlg::Inv reports a (near-)singular pivot
        (mimsem_block_inverse_status; eul/LinAlg.cpp:243-246)"""
        return self._block_inverse(blocks, True)

    def norm(self, x):
        """2-norm of a whole (single-rank) vector by the library's two-stage row-dot; DistEngine overrides with the ownership-weighted,
        all-reduced version"""
        v = x.reshape(1, -1)
        if not v.is_contiguous():
            v = v.contiguous()
        return float(torch.sqrt(self.rowdot(v, v))[0])

    def complete(self, form, y):
        """single rank: results are already complete (DistEngine reduces the halo here)"""
        return y

    def wsum(self, form, t):
        """sum over the GLOBAL vector of one form (every DoF once); DistEngine weights by ownership and all-reduces"""
        return t.sum()

    def allreduce(self, t, op="sum"):
        """sum / max over the ranks of a DistEngine; the identity on one rank"""
        return t

    def space(self, key):
        """context manager naming the vector space of the inner products inside (0, 1, 2 or "uh" = packed [1-form, 2-form]);
        a no-op on one rank, the ownership weights on a DistEngine"""
        return contextlib.nullcontext()

    # ---- halo pack / unpack ---------------------------------------------------------------------
    def halo_segments(self, idx, seg_off, s_begin, s_end, mode, buf, v):
        """all neighbours in one launch (mimsem_halo_segments): mode 0 pack, 1 insert, 2 add; seg_off: host int32 array"""
        _need(isinstance(seg_off, np.ndarray) and seg_off.dtype == np.int32 and seg_off.ndim == 1 and seg_off.size >= 1, "seg_off: a host int32 array")
        off, poff = _host(seg_off, np.int32)
        v2 = self._rows(v, None, "v")
        total = int(off[-1])                                # (buf: segment-major [neighbour][level][slot], idx: the slots of all neighbours)
        check(self.L.mimsem_halo_segments(self.ctx, self._vec(idx, total, "idx", atleast=True, dtype=_I32), off.size - 1, poff, s_begin, s_end, v2.shape[0], mode,
                                          self._vec(buf, total * v2.shape[0], "buf", atleast=True), *_ps(v2)), "halo_segments")

    def halo_pack(self, idx, v):
        v2 = self._rows(v, None, "v")
        buf = self._new(v2.shape[0], idx.numel())
        check(self.L.mimsem_halo_pack(self.ctx, self._vec(idx, None, "idx", dtype=_I32), idx.numel(), v2.shape[0], *_ps(v2), _ptr(buf)), "halo_pack")
        return buf

    def halo_unpack(self, idx, buf, v, add):
        v2 = self._rows(v, None, "v")
        check(self.L.mimsem_halo_unpack(self.ctx, self._vec(idx, None, "idx", dtype=_I32), idx.numel(), v2.shape[0], int(add),
                                        self._vec(buf, v2.shape[0] * idx.numel(), "buf"), *_ps(v2)), "halo_unpack")
