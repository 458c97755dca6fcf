"""Synthetic inputs shared by bench.py, scripts/ and the parity tests (SURVEY 8(d) "synthetic inputs"): part of the
host-side mirror, no checker code in here."""
import numpy as np

SCALE = 1.0e8      # eul/Assembly.cpp:20


def z_levels(nk, n0q, rng=None, ztop=30000.0, mu=15.0):
    """UMJS14-like stretched levels (eul/UMJS14.cpp:124-129 shape), with a small per-point perturbation
    so that thickness really varies over the quad-point grid."""
    k = np.arange(nk + 1) / nk
    z = ztop * (np.sqrt(mu * k * k + 1.0) - 1.0) / (np.sqrt(mu + 1.0) - 1.0)
    levs = np.repeat(z[:, None], n0q, axis=1)
    if rng is not None:
        levs[1:-1] *= 1.0 + 0.01 * rng.uniform(-1, 1, (nk - 1, n0q))
    return levs


def write_sw_case(path, dm, fg, u, h, dt, nsteps, nits, q_exact, bot=None):
    """A shallow-water case for the C++ hosts (mimsem_amd/host/sw_io.hpp: tests/cpp/test_sw.cpp, mimsem_amd/host/sw_call.cpp): the tables of
    a DeviceMesh (nk = 1) as mimsem_mesh_desc takes them, the Coriolis 0-form, a start state (host arrays), the step parameters and
    (optional) the bottom topography 2-form."""
    import numpy as np
    with open(path, "wb") as f:
        np.array([dm.n, dm.m, dm.nEl, 1, dm.n0, dm.n1, dm.n2, dm.nq, nsteps, nits, int(q_exact), 0 if bot is None else 1], dtype=np.int32).tofile(f)
        for a in (dm.inds0, dm.inds1x, dm.inds1y, dm.inds2, dm.indsq):
            np.ascontiguousarray(a, dtype=np.int32).tofile(f)
        for a in (dm.det, dm.J, dm.thick[:1], dm.thickInv[:1], fg, u, h, np.array([dt])) + (() if bot is None else (bot,)):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def write_arrays(path, arrays):
    """named int32 / float64 arrays for the C++ hosts (mimsem_amd/host/sw_io.hpp::read_arrays)"""
    import struct

    import numpy as np
    with open(path, "wb") as f:
        f.write(b"MSEMARR1"); f.write(struct.pack("<i", len(arrays)))
        for name, a in arrays.items():
            a = np.asarray(a)
            kind = 0 if np.issubdtype(a.dtype, np.integer) else 1
            a = np.ascontiguousarray(a, dtype=np.int32 if kind == 0 else np.float64)
            nb = name.encode()
            f.write(struct.pack("<i", len(nb))); f.write(nb); f.write(struct.pack("<iq", kind, a.size))
            a.tofile(f)


def read_arrays(path):
    """the named arrays of write_arrays (also what tests/cpp/test_tsw.cpp writes back): {name: numpy array}"""
    import struct

    import numpy as np
    out = {}
    with open(path, "rb") as f:
        if f.read(8) != b"MSEMARR1":
            raise ValueError("%s: not an array file" % path)
        (count,) = struct.unpack("<i", f.read(4))
        for _ in range(count):
            (nl,) = struct.unpack("<i", f.read(4))
            name = f.read(nl).decode()
            kind, n = struct.unpack("<iq", f.read(12))
            out[name] = np.fromfile(f, dtype=np.int32 if kind == 0 else np.float64, count=n)
    return out


def write_tsw_case(path, dm, fg, dt, nsteps, use_graph=True, m1h_its=16, quad=None, state=None):
    """A thermal shallow-water case for the C++ host (tests/cpp/test_tsw.cpp, mimsem_amd/host/tsw_call.cpp over mimsem_thermalsw.hpp): the
    tables of a DeviceMesh (nk = 1), the Coriolis 0-form, dt, and either the quadrature-grid fields (uq [nq, 2], hq, sq) that init() projects
    or a start state (u, h, S) in the mesh's numbering"""
    import numpy as np
    a = mesh_arrays(dm)
    a.update(fg=np.asarray(fg, dtype=np.float64).ravel(), dt=np.array([dt], dtype=np.float64),
             opts=np.array([nsteps, int(use_graph), m1h_its, 1 if quad is not None else 0], dtype=np.int32))
    if quad is not None:
        for k, v in zip(("uq", "hq", "sq"), quad):
            a[k] = np.asarray(v, dtype=np.float64).ravel()
    else:
        for k, v in zip(("u0", "h0", "S0"), state):
            a[k] = np.asarray(v, dtype=np.float64).ravel()
    write_arrays(path, a)


def write_euler_case(path, mesh, levs, quad_coords, state, dt, nsteps, hs_lat=None, newton_maxit=20, newton_tol=1.0e-12, vort_its=0,
                     do_visc=True, m1_steps=0, eng=None, box_lx=None):
    """A 3-D Euler case for the C++ host (tests/cpp/test_euler.cpp, mimsem_amd/host/euler_call.cpp over mimsem_euler.hpp): the tables of a
    DeviceMesh (global numbering, nk >= 2), what the host does not diagnose itself -- the Coriolis 0-form fg [nk, n0] of HorizSolve.coriolis
    from quad_coords [nq, 3] and the geopotential zv [nEl, nk n2e] of VertSolve.init_gz from levs [nk+1, nq], both made here on the device
    (eng: an Engine of the mesh, made when None) --, the start state (velx, velz, rho, rt, exner) in Euler.strang_ec's layouts (host arrays or
    tensors) and the step parameters.  hs_lat [nEl, mp12]: Held-Suarez forcing with that latitude field; vort_its > 0: the count VortDiag's
    fixed-length solves start with (tests: 1 must miss its check), 0: found adaptively; m1_steps > 0: the Chebyshev solves of M1 cut to that
    many steps (tests: 4 must miss).  box_lx: the case is the doubly periodic box of that side (tests/cpp/test_box_euler.cpp, euler_call's box
    case over box::Euler): no Coriolis form is written, `lx` [1] is; the mesh is one patch with uniform layers, quad_coords is not read"""
    import numpy as np
    from .device import Engine
    from .horizsolve import HorizSolve
    from .vertsolve import VertSolve
    eng = Engine(mesh) if eng is None else eng
    host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)
    a = mesh_arrays(mesh)
    if box_lx is None:
        a["fg"] = host(HorizSolve(eng, del2=0.0, quad_coords=quad_coords).fg.expand(eng.nk, -1)).ravel()
    else:
        a["lx"] = np.array([box_lx], dtype=np.float64)
    a.update(zv=host(VertSolve(eng, dt).init_gz(levs)).ravel(),
             dt=np.array([dt], dtype=np.float64), newton_tol=np.array([newton_tol], dtype=np.float64),
             opts=np.array([nsteps, 0 if hs_lat is None else 1, newton_maxit, vort_its, int(do_visc), m1_steps], dtype=np.int32))
    for k, v in zip(("velx", "velz", "rho", "rt", "exner"), state):
        a[k] = host(v).ravel()
    if hs_lat is not None:
        a["hs_lat"] = host(hs_lat).ravel()
    write_arrays(path, a)


def mesh_arrays(dm):
    """the tables of a DeviceMesh under their mimsem_mesh_desc names (sw_io.hpp::desc_of)"""
    import numpy as np
    d = {"sizes": np.array([dm.n, dm.m, dm.nEl, dm.nk, dm.n0, dm.n1, dm.n2, dm.nq], dtype=np.int32)}
    for k in ("inds0", "inds1x", "inds1y", "inds2", "indsq", "det", "J", "thick", "thickInv"):
        d[k] = getattr(dm, k)
    return d
