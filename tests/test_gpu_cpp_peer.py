"""C++ ranks on the ONE-SIDED halo transport (Shard::use_peer, mimsem_amd/host/mimsem_shard.hpp): every rank a separate process of one driver
binary (tests/cpp/process_ranks.hpp), the sharded Picard iteration of src::SWEqn recorded as one hipGraph per rank, the transport's status
folded into the one all-reduce of an iteration.  Checked against the one-context run of the Python host and, bit for bit, against the
thread/callback C++ drivers on the same case files; the status path through mimsem_halo_peer_mark_for_test on both hosts.

Every rank process runs under its own time limit; an abort, a segmentation fault or a time limit (134 / 139 / 124 / 137) ends the module's
GPU work: the later tests fail without starting anything."""
import os
import re
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_LIMIT_S = 300
EXIT_HALO_TIMEOUT = 3                     # process_ranks::EXIT_HALO_TIMEOUT
RENDEZVOUS_BYTES = 1 << 20                # >= sizeof(process_ranks::Layout)
FATAL = (124, 134, 137, 139, -6, -9, -11)
_fatal = []                               # (what, exit statuses) of a run that faulted, hung or aborted


def _guard():
    if _fatal:
        pytest.fail("not started: an earlier GPU run of this module ended with %s" % (_fatal[0],))


def _build(tmp, name, extra=()):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "mimsem_amd"), "-lmimsem_hip", "-Wl,-rpath," + os.path.join(ROOT, "mimsem_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _check_statuses(what, codes):
    bad = [c for c in codes if c in FATAL]
    if bad:
        _fatal.append((what, codes))
        pytest.fail("%s: a rank ended with %s (fault, abort or time limit): nothing more is started" % (what, codes))


def _run_ranks(tmp, what, argv_of_rank, world, env=None):
    """start `world` rank processes (each under its own time limit), wait for all, return [(exit status, stdout + stderr)]"""
    procs, logs = [], []
    for r in range(world):
        log = open(os.path.join(str(tmp), "%s_rank%d.log" % (what, r)), "w+")
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(RANK_LIMIT_S)] + argv_of_rank(r), stdout=log, stderr=subprocess.STDOUT, cwd=ROOT, env=env))
        logs.append(log)
    out = []
    for p, log in zip(procs, logs):
        try:
            rc = p.wait(timeout=RANK_LIMIT_S + 30)
        except subprocess.TimeoutExpired:
            p.kill(); rc = p.wait()
            rc = 137
        log.seek(0)
        out.append((rc, log.read()))
        log.close()
    for rc, text in out:
        print(text)
    _check_statuses(what, [rc for rc, _ in out])
    return out


def _run_one(what, argv):
    try:
        p = subprocess.run(["timeout", "-k", "10", str(RANK_LIMIT_S)] + argv, capture_output=True, text=True, timeout=RANK_LIMIT_S + 30, cwd=ROOT)
        rc, text = p.returncode, p.stdout + p.stderr
    except subprocess.TimeoutExpired:
        rc, text = 137, ""
    print(text)
    _check_statuses(what, [rc])
    return rc, text


def _rendezvous(tmp, name):
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(b"\0" * RENDEZVOUS_BYTES)
    return path


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _field(text, pattern, cast=float):
    return [cast(m) for m in re.findall(pattern, text)]


# ---- the shallow-water case of test_gpu_cpp_shim.py::test_sharded_sw_step_driven_from_cpp ----------------------------------------------------
def _sw_cases(tmp_path, world, nsteps):
    """writes rank<r>.arr for every rank; returns (per-rank DeviceMesh, one-context u, h after nsteps, u, h at the start, global sizes)"""
    import numpy as np
    import torch
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.partition import build_plans, patches_of_rank
    from mimsem_amd.sweqn import SWEqn, williamson2
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import mesh_arrays, write_arrays
    pn, ne, npatch = 3, 4, 6
    cs = CubedSphere(pn, ne, npatch); coords = sphere_coords(pn, ne)

    def build(pids):
        topos = [Topo(cs, p, 1) for p in pids]
        geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
        for g in geoms:
            g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
        dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
        xq = np.zeros((int(max(g.loc0.max() for g in geoms)) + 1, 3))
        for g in geoms:
            xq[g.loc0] = coords[g.loc0]
        return dm, xq[dm.gidq]
    dm1, xq1 = build(list(range(npatch)))
    eng1 = Engine(dm1)
    S1 = SWEqn(eng1, xq1)
    uq, hq = williamson2(torch.as_tensor(xq1, device=eng1.device), alpha=0.0)
    lam = torch.atan2(torch.as_tensor(xq1[:, 1]), torch.as_tensor(xq1[:, 0])).to(eng1.device)
    uq = uq + torch.stack([3.0 * torch.sin(2 * lam), 2.0 * torch.cos(lam)], dim=1)            # perturbed: every term active
    u0, h0 = S1.init1(uq), S1.init2(hq)
    u, h = u0, h0
    for _ in range(nsteps):
        u, h = S1.solve(u, h, 360.0, nits=2, q_exact=False)
    assert S1.fixed_iterations == 2 * nsteps
    fg = S1.fg[0].cpu().numpy(); ug0 = u0[0].cpu().numpy(); hg0 = h0[0].cpu().numpy()
    want_u, want_h = u[0].cpu().numpy(), h[0].cpu().numpy()
    dms = []
    for rank in range(world):
        dm, _ = build(patches_of_rank(npatch, world, rank))
        p0, p1 = build_plans(cs, world, rank, dm.gid0, dm.gid1)
        ranks = p1.neighbours()
        assert ranks == p0.neighbours() and len(ranks) == world - 1
        empty = np.zeros(0, np.int32)

        def lists(by_rank):
            off = np.zeros(len(ranks) + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(by_rank.get(r, empty)) for r in ranks])
            return np.concatenate([by_rank.get(r, empty) for r in ranks]).astype(np.int32), off
        arr = mesh_arrays(dm)
        g1, g1o = lists(p1.ghost_slots); m1, m1o = lists(p1.mirror_slots); g0, g0o = lists(p0.ghost_slots); m0, m0o = lists(p0.mirror_slots)
        arr.update(ranks=np.asarray(ranks, np.int32), ghost1=g1, ghost1_off=g1o, mirror1=m1, mirror1_off=m1o, ghost0=g0, ghost0_off=g0o, mirror0=m0,
                   mirror0_off=m0o, own0=p0.owned.astype(np.float64), own1=p1.owned.astype(np.float64), fg=fg[dm.gid0], u=ug0[dm.gid1], h=hg0[dm.gid2],
                   params=np.array([360.0, 2.0, 0.0]))
        write_arrays(str(tmp_path / ("rank%d.arr" % rank)), arr)
        dms.append(dm)
    return dms, want_u, want_h, ug0, (cs.nDofs1G, cs.nDofs2G)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sw_step_cpp_ranks_one_sided_recorded(tmp_path, world):
    """src::SWEqn on `world` C++ rank PROCESSES over the one-sided transport, the Picard iteration recorded: three Galewsky-style steps equal the
    one-context run to 1e-10 and the thread/callback C++ driver (eager) bit for bit, with the same step counts; graphs recorded and replayed;
    no time-out; every receive buffer uncached"""
    import numpy as np
    _guard()
    nsteps = 3
    dms, want_u, want_h, ug0, (N1, N2) = _sw_cases(tmp_path, world, nsteps)
    exe = _build(tmp_path, "test_sw_sharded_peer")
    rdv = _rendezvous(tmp_path, "rendezvous")
    runs = _run_ranks(tmp_path, "sw_peer", lambda r: [exe, str(world), str(r), rdv, str(tmp_path / "rank"), str(tmp_path / "peer"), str(nsteps)], world)
    assert all(rc == 0 for rc, _ in runs), [rc for rc, _ in runs]
    # the same case files through the thread/callback driver: eager launches, host-staged exchanges
    rc, cb_text = _run_one("sw_callback", [_build(tmp_path, "test_sw_sharded", ["-pthread"]), str(world), str(tmp_path / "rank"), str(tmp_path / "cb"), str(nsteps)])
    assert rc == 0 and "DONE" in cb_text
    got_u = np.full(N1, np.nan); got_h = np.full(N2, np.nan)
    same_bits = True
    for rank, dm in enumerate(dms):
        peer = open(str(tmp_path / ("peer%d.bin" % rank)), "rb").read()
        cb = open(str(tmp_path / ("cb%d.bin" % rank)), "rb").read()
        same_bits = same_bits and peer == cb
        res = np.frombuffer(peer, dtype=np.float64)
        ul, hl = res[:dm.n1], res[dm.n1:]
        assert np.linalg.norm(ul - want_u[dm.gid1]) <= 1e-10 * np.linalg.norm(want_u[dm.gid1]), rank          # ghosts included
        got_u[dm.gid1] = ul; got_h[dm.gid2] = hl
    eu = np.linalg.norm(got_u - want_u) / np.linalg.norm(want_u); eh = np.linalg.norm(got_h - want_h) / np.linalg.norm(want_h)
    text = "\n".join(t for _, t in runs)
    steps = re.findall(r"chebyshev steps \[(\d+), (\d+), (\d+)\]", text)
    cb_steps = re.findall(r"chebyshev steps \[(\d+), (\d+), (\d+)\]", cb_text)
    nodes_first = _field(text, r"graph_nodes first (\d+)", int); nodes_later = _field(text, r"later (\d+), replays", int)
    replays = _field(text, r"replays (\d+)", int); iters = _field(text, r"Picard iterations (\d+)", int)
    exch = re.findall(r"exchanges per iteration first (\d+) later (\d+)", text)
    unc = _field(text, r"uncached (\d)", int); tmo = _field(text, r"peer_timeouts (\d+)", int); sps = _field(text, r"steps/s ([0-9.]+)")
    print("C++ one-sided SW step, world %d: |u - u_1ctx| = %.2e  |h - h_1ctx| = %.2e  bit-equal to the thread/callback driver: %s  graph nodes %s / %s  "
          "replays %s of %s iterations  exchanges per iteration %s  uncached %s  steps/s %s"
          % (world, eu, eh, same_bits, nodes_first, nodes_later, replays, iters, exch, unc, sps))
    assert eu < 1e-10 and eh < 1e-11 and np.linalg.norm(want_u - ug0) > 0
    assert same_bits, "the one-sided recorded run differs from the thread/callback run in some bit"
    assert len(steps) == world and len(set(steps)) == 1 and steps == cb_steps[:world] and set(cb_steps) == set(steps)
    assert len(nodes_first) == world and min(nodes_first) > 0 and min(nodes_later) > 0
    assert all(it == 2 * nsteps for it in iters) and all(rp == it - 2 for rp, it in zip(replays, iters))        # the first of each kind eager
    assert tmo == [0] * world
    assert unc == [1] * world, "a receive buffer of the one-sided transport is not uncached device memory"


@pytest.mark.gpu
def test_horizsolve_cpp_ranks_one_sided(tmp_path):
    """HorizSolve on 2 C++ rank PROCESSES over the one-sided transport (eager): advection_rhs_ec + momentum_rhs_ec bit-equal to the
    thread/callback driver and within 1e-9 of the one-context evaluation"""
    import numpy as np
    import torch  # noqa: F401
    from mimsem_amd.device import DeviceMesh, Engine
    from mimsem_amd.geom import Geom
    from mimsem_amd.horizsolve import HorizSolve
    from mimsem_amd.mesh import CubedSphere, sphere_coords
    from mimsem_amd.partition import build_plans, patches_of_rank
    from mimsem_amd.topo import Topo
    from mimsem_amd.workloads import mesh_arrays, write_arrays, z_levels
    _guard()
    world = 2
    pn, ne, npatch, nk = 3, 4, 6, 3
    cs = CubedSphere(pn, ne, npatch); coords = sphere_coords(pn, ne)

    def build(pids):
        topos = [Topo(cs, p, nk) for p in pids]
        geoms = [Geom(t, cs, coords, nk) for t in topos]
        for g in geoms:
            g.set_levels(z_levels(nk, g.n0))
        dm = DeviceMesh(topos, geoms, nk=nk, numbering="global")
        xq = np.zeros((int(max(g.loc0.max() for g in geoms)) + 1, 3))
        for g in geoms:
            xq[g.loc0] = coords[g.loc0]
        return dm, xq[dm.gidq]
    dm1, xq1 = build(list(range(npatch)))
    eng1 = Engine(dm1)
    hs1 = HorizSolve(eng1, quad_coords=xq1)
    r = np.random.default_rng(31)
    N0, N1, N2 = cs.nDofs0G, cs.nDofs1G, cs.nDofs2G
    area = float(dm1.det.mean()) * 4.0 / (pn * pn); dz = float(dm1.thick.mean()); ln = area ** 0.5
    G = dict(u1=r.standard_normal((nk, N1)) * 20.0 * ln * dz, h1=r.uniform(0.8, 1.2, (nk, N2)) * area * dz, theta=r.uniform(290, 310, (nk, N2)) * area * dz,
             Pi=r.uniform(900, 1000, (nk, N2)) * area * dz, velz=r.standard_normal((nk - 1, N2)) * area, dudz=r.standard_normal((nk - 1, N1)) * 1e-3 * ln)
    G["u2"] = G["u1"] * 1.03; G["h2"] = G["h1"] * 1.01
    t = lambda k: eng1.tensor(G[k])
    dF, dG, Fk, Gk = hs1.advection_rhs_ec(t("u1"), t("u2"), t("h1"), t("h2"), t("theta"))
    fu = hs1.momentum_rhs_ec(t("theta"), t("dudz"), t("dudz"), t("velz"), t("velz"), t("Pi"), t("u1"), t("u2"), t("h1"), t("h2"), Fx=Fk, Fk=Fk, dTheta=hs1.dTheta)
    want_fu, want_dG = fu.cpu().numpy(), dG.cpu().numpy()
    fg = hs1.fg.cpu().numpy()
    fg = fg if fg.shape[0] == nk else np.broadcast_to(fg, (nk, N0))
    dms = []
    for rank in range(world):
        dm, _ = build(patches_of_rank(npatch, world, rank))
        p0, p1 = build_plans(cs, world, rank, dm.gid0, dm.gid1)
        ranks = p1.neighbours()
        assert ranks == p0.neighbours() and len(ranks) == world - 1
        empty = np.zeros(0, np.int32)

        def lists(by_rank):
            off = np.zeros(len(ranks) + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(by_rank.get(q, empty)) for q in ranks])
            return np.concatenate([by_rank.get(q, empty) for q in ranks]).astype(np.int32), off
        arr = mesh_arrays(dm)
        g1, g1o = lists(p1.ghost_slots); m1, m1o = lists(p1.mirror_slots); g0, g0o = lists(p0.ghost_slots); m0, m0o = lists(p0.mirror_slots)
        arr.update(ranks=np.asarray(ranks, np.int32), ghost1=g1, ghost1_off=g1o, mirror1=m1, mirror1_off=m1o, ghost0=g0, ghost0_off=g0o, mirror0=m0,
                   mirror0_off=m0o, own0=p0.owned.astype(np.float64), own1=p1.owned.astype(np.float64), fg=np.ascontiguousarray(fg[:, dm.gid0]),
                   params=np.array([float(N0)]))
        for k, gid in (("u1", dm.gid1), ("u2", dm.gid1), ("dudz", dm.gid1), ("h1", dm.gid2), ("h2", dm.gid2), ("theta", dm.gid2), ("Pi", dm.gid2), ("velz", dm.gid2)):
            arr[k] = np.ascontiguousarray(G[k][:, gid])
        write_arrays(str(tmp_path / ("rank%d.arr" % rank)), arr)
        dms.append(dm)
    exe = _build(tmp_path, "test_horiz_sharded_peer")
    rdv = _rendezvous(tmp_path, "rendezvous")
    runs = _run_ranks(tmp_path, "horiz_peer", lambda q: [exe, str(world), str(q), rdv, str(tmp_path / "rank"), str(tmp_path / "peer")], world)
    assert all(rc == 0 for rc, _ in runs), [rc for rc, _ in runs]
    rc, cb_text = _run_one("horiz_callback", [_build(tmp_path, "test_horiz_sharded", ["-pthread"]), str(world), str(tmp_path / "rank"), str(tmp_path / "cb")])
    assert rc == 0 and "DONE" in cb_text
    got_fu = np.full((nk, N1), np.nan); got_dG = np.full((nk, N2), np.nan)
    same_bits = True
    for rank, dm in enumerate(dms):
        peer = open(str(tmp_path / ("peer%d.bin" % rank)), "rb").read()
        same_bits = same_bits and peer == open(str(tmp_path / ("cb%d.bin" % rank)), "rb").read()
        res = np.frombuffer(peer, dtype=np.float64)
        s1, s2 = nk * dm.n1, nk * dm.n2
        got_fu[:, dm.gid1] = res[:s1].reshape(nk, dm.n1); got_dG[:, dm.gid2] = res[s1:s1 + s2].reshape(nk, dm.n2)
    e1 = np.linalg.norm(got_fu - want_fu) / np.linalg.norm(want_fu); e2 = np.linalg.norm(got_dG - want_dG) / np.linalg.norm(want_dG)
    text = "\n".join(t for _, t in runs)
    unc = _field(text, r"uncached (\d)", int); tmo = _field(text, r"peer_timeouts (\d+)", int); eps = _field(text, r"evaluations/s ([0-9.]+)")
    print("C++ one-sided HorizSolve, world %d: |fu - fu_1ctx| = %.2e  |dG - dG_1ctx| = %.2e  bit-equal to the thread/callback driver: %s  uncached %s  "
          "evaluations/s %s" % (world, e1, e2, same_bits, unc, eps))
    assert same_bits, "the one-sided run differs from the thread/callback run in some bit"
    assert e1 < 1e-9 and e2 < 1e-9
    assert tmo == [0] * world and unc == [1] * world


@pytest.mark.gpu
def test_halo_timeout_stops_every_cpp_rank(tmp_path):
    """the status path of the C++ host: rank 1 marks its pair plan's error word after its first step (mimsem_halo_peer_mark_for_test); EVERY rank
    must leave with HaloTimeout after the next Picard iteration's all-reduce, with the driver's agreed exit code, within the time limit"""
    _guard()
    world = 2
    _sw_cases(tmp_path, world, 1)
    exe = _build(tmp_path, "test_sw_sharded_peer")
    rdv = _rendezvous(tmp_path, "rendezvous")
    runs = _run_ranks(tmp_path, "sw_peer_mark", lambda r: [exe, str(world), str(r), rdv, str(tmp_path / "rank"), str(tmp_path / "peer"), "3", "mark"], world)
    print("C++ status path: exit statuses %s" % [rc for rc, _ in runs])
    for rank, (rc, text) in enumerate(runs):
        assert rc == EXIT_HALO_TIMEOUT and "HaloTimeout" in text and "halo is stale" in text, (rank, rc, text)


def _py_status_worker(rank, world, port):
    """one rank of the Python-host status check: SWEqn over a DistEngine on the one-sided transport, one step, rank 1 marks its pair plan,
    the next step must raise HaloTimeout (exit EXIT_HALO_TIMEOUT; 1 = it did not)"""
    import numpy as np
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    code = 1
    try:
        from mimsem_amd.device import DeviceMesh, Engine
        from mimsem_amd.distributed import DistEngine, HaloTimeout
        from mimsem_amd.geom import Geom
        from mimsem_amd.mesh import CubedSphere, sphere_coords
        from mimsem_amd.partition import patches_of_rank
        from mimsem_amd.sweqn import SWEqn, williamson2
        from mimsem_amd.topo import Topo
        pn, ne, npatch = 3, 4, 6
        cs = CubedSphere(pn, ne, npatch); coords = sphere_coords(pn, ne)
        pids = patches_of_rank(npatch, world, rank)
        topos = [Topo(cs, p, 1) for p in pids]
        geoms = [Geom(t, cs, coords, 1, signed_det=True) for t in topos]
        for g in geoms:
            g.set_levels(np.stack([np.zeros(g.n0), np.ones(g.n0)]))
        dm = DeviceMesh(topos, geoms, nk=1, numbering="global")
        xq = np.zeros((int(max(g.loc0.max() for g in geoms)) + 1, 3))
        for g in geoms:
            xq[g.loc0] = coords[g.loc0]
        xq = xq[dm.gidq]
        eng = Engine(dm)
        deng = DistEngine(eng, cs, world, rank, overlap=True, transport="peer")
        S = SWEqn(deng, xq)
        uq, hq = williamson2(torch.as_tensor(xq, device=eng.device), alpha=0.0)
        u, h = S.solve(S.init1(uq), S.init2(hq), 360.0, nits=2, q_exact=False)
        ok_first = deng.peer_timeouts() == 0 and S.fixed_iterations == 2
        if rank == 1:
            deng.chalo.mark_for_test("pair")
        try:
            S.solve(u, h, 360.0, nits=2, q_exact=False)
            print("rank %d: no HaloTimeout" % rank, flush=True)
        except HaloTimeout as e:
            print("rank %d: HaloTimeout: %s (first step clean: %s)" % (rank, e, ok_first), flush=True)
            code = EXIT_HALO_TIMEOUT if ok_first else 1
    finally:
        dist.destroy_process_group()
    sys.stdout.flush()
    os._exit(code)


@pytest.mark.gpu
def test_halo_timeout_stops_every_python_rank(tmp_path):
    """the status path of the Python host: a 2-process DistEngine SW step on the one-sided transport raises HaloTimeout on both ranks after
    rank 1 marked its pair plan"""
    _guard()
    world, port = 2, _free_port()
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    code = "from tests.test_gpu_cpp_peer import _py_status_worker as w; w(%d, %d, %d)"
    runs = _run_ranks(tmp_path, "py_peer_mark", lambda r: [sys.executable, "-c", code % (r, world, port)], world, env=env)
    print("Python status path: exit statuses %s" % [rc for rc, _ in runs])
    for rank, (rc, text) in enumerate(runs):
        assert rc == EXIT_HALO_TIMEOUT and "HaloTimeout" in text and "halo is stale" in text, (rank, rc, text)
