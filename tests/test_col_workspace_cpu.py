"""The plans of the column workspace (csrc/col_workspace.hpp: one struct per user of mimsem_ctx::d_col, whose carve() both counts the
request and places every buffer) through tests/cpp/col_workspace_cli.cpp, a plain C++ program.  For every plan and path flag: the plan
is counted, carved on a host buffer of exactly that many doubles, and every member the path uses is non-null, inside the buffer, as
large as its block shape says, and disjoint from every other member -- but for the members documented as deliberate re-use, which
must BE the member they name.  No call asks for more than the formula it used before the plans existed (restated below), and the
program runs clean under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "col_workspace_cli.cpp")

N2 = (1, 4, 9, 16, 25, 49)
NK = (2, 3, 4, 5, 30)
NEL = (1, 6, 3456)
SHAPES = [(nEl, nk, n2) for n2 in N2 for nk in NK for nEl in NEL]


def mp12_of(n2):
    n = round(n2 ** 0.5)
    assert n * n == n2
    return (n + 1) ** 2                                  # quadrature order = element order


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cli(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("col_workspace") / ("col_workspace_cli_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + [SRC, "-o", exe])
    return exe


def plans(cli, nEl, nk, n2):
    """{(plan, path): (count, {member: (offset, need, alias)})}; a sanitizer report fails the run (non-zero exit, stderr)"""
    r = subprocess.run([cli] + [str(v) for v in (nEl, nk, n2, mp12_of(n2))], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out, cur = {}, None
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "plan":
            cur = out[(t[1], t[2])] = (int(t[3]), {})
        else:
            assert t[0] == "m" and t[1] not in cur[1], line
            cur[1][t[1]] = (int(t[2]), int(t[3]), t[4])
    return out


# ---- what a call asked of ensure_col before the plans: the formulas of the parent commit, restated ----
def colop_ws(nEl, nk, n2, mp12):
    return nEl * (nk + 1) * 2 * (mp12 + 3 * n2 * n2)


def sweep_ws(nEl, nk, n2, mp12):
    nn = n2 * n2
    return nEl * nk * (3 * nn + 2 * nn + 2 * n2) + 3 * nEl * nk * n2


def schur3_ws(nEl, nk, n2, mp12):
    nn, k1 = n2 * n2, nk + 1
    return nEl * k1 * (80 * nn + 2 * mp12 + 4 * nn + 16 * n2) + nEl * ((k1 + 2) // 2) * (4 * 4 * nn + 2 * 2 * n2 + 4 * nn + 4 * nn)


def parent_doubles(plan, path, nEl, nk, n2, mp12):
    nn, per = n2 * n2, nEl * nk * n2
    if plan == "colop":                                  # colop_blocks / colop_apply; the theta diagnoses added the right-hand side's share
        return colop_ws(nEl, nk, n2, mp12) + (nEl * (nk + 1) * (3 * nn + 2 * n2) if path == "1" else 0)
    if plan == "quad":
        return nEl * nk * mp12
    if plan == "blockinv":
        return nEl * (1 if path == "0" else nk) * (mp12 + nn)
    if plan == "schur":
        return nEl * (nk + 1) * (30 * nn + 8 * n2 + 4 * mp12) + colop_ws(nEl, nk, n2, mp12)
    if plan == "sweep":
        return sweep_ws(nEl, nk, n2, mp12)
    if plan == "newton":
        return max(sweep_ws(nEl, nk, n2, mp12), (5 if path == "1" else 4) * per)
    if plan == "s3fused":
        return nEl * nk * ((5 + 4 + 6) * nn + 2 * n2) + ((nEl + 3) * (nk // 2 + 1) + 8) * nn
    if plan == "schur3":
        return schur3_ws(nEl, nk, n2, mp12)
    raise KeyError(plan)


# ---- the members a path leaves null ----
S3_CHAIN_ONLY = {"Brtinv", "Cv"}
S3_BANDS_ONLY = {"VAB", "t_a", "G_rt", "DTV1", "AinvDTV1", "G_pi", "DX", "D_rt", "t_d", "Q", "GNN", "QMD", "DD", "DGG"}


def unused(plan, path):
    if plan == "colop":
        return set() if path == "1" else {"frt"}
    if plan == "newton":
        return set() if path == "1" else {"wF"}
    if plan == "schur3":
        dpp, own_cv, penta, rows = (ch == "1" for ch in path)
        tail = {"fpad", "dpad", "Gws", "Dinv"} if penta else ({"Fac"} | (set() if rows else {"Dinv"}))
        return (S3_BANDS_ONLY if dpp else S3_CHAIN_ONLY) | tail
    return set()


def vector_doubles(plan, path, m, nEl, nk, n2, mp12):
    """what the kernels index of a plain vector member (the program reports the block arrays' and bands' from their shapes)"""
    nn, lev, K, sm = n2 * n2, nEl * nk, (nk + 1) // 2, 2 * n2
    if m in ("cq", "tmpM") and plan in ("colop", "schur", "schur3"):      # coefficients and temporaries of colop_blocks_into
        return nEl * (nk + 1) * 2 * (mp12 if m == "cq" else 2 * nn)
    if plan == "colop":
        return {"M": nEl * (nk + 1) * 2 * nn, "frt": nEl * (nk + 1) * n2}[m]
    if plan == "quad":
        return lev * mp12
    if plan == "blockinv":
        return nEl * (1 if path == "0" else nk) * (mp12 if m == "cq" else nn)
    if plan == "schur":
        return nEl * (nk - 1) * n2 if m in ("gpi", "geta", "rlump") else lev * n2
    if plan == "sweep":
        return lev * {"L": 3 * nn, "G": nn, "D": nn}.get(m, n2)
    if plan == "newton":
        return lev * n2
    if plan == "s3fused":
        return ((nEl + 3) * (nk // 2 + 1) + 8) * nn if m == "dump" else lev * {"L": 5 * nn, "Fac": 4 * nn, "yws": n2, "fu2": n2}.get(m, nn)
    if plan == "schur3":
        penta = path[2] == "1"
        return {"Tm": nEl * K * 3 * sm * sm, "Fac": lev * 4 * nn, "yws": lev * n2 if penta else nEl * K * sm, "fpad": nEl * K * sm,
                "dpad": nEl * K * sm, "Gws": nEl * K * sm * sm, "Dinv": nEl * K * sm * sm}.get(m, lev * n2)
    raise KeyError(plan)


def check(plan, path, count, members, dims):
    null = {m for m, (off, _, _) in members.items() if off < 0}
    assert null == unused(plan, path), (plan, path, sorted(null ^ unused(plan, path)))
    own = {m: v for m, v in members.items() if v[0] >= 0 and v[2] == "-"}
    # deliberate re-use: the member IS the one it names, which owns its memory
    for m, (off, need, alias) in members.items():
        if off >= 0 and alias != "-":
            assert alias in own and own[alias][0] == off and (need < 0 or need == own[alias][1]), (plan, path, m, alias)
    # every other member: inside the buffer, disjoint from the rest (each owns the stretch up to the next member; the stretches tile the
    # buffer, none is empty), and that stretch is exactly what its block shape indexes -- a take that no member holds would lengthen one
    order = sorted(own, key=lambda m: own[m][0])
    offs = [own[m][0] for m in order] + [count]
    assert offs[0] == 0 and all(b > a for a, b in zip(offs, offs[1:])), (plan, path, "members overlap or lie outside", offs)
    for m, a, b in zip(order, offs, offs[1:]):
        need = own[m][1] if own[m][1] >= 0 else vector_doubles(plan, path, m, *dims)
        assert need == b - a, (plan, path, m, need, b - a)
    assert count <= parent_doubles(plan, path, *dims), (plan, path, count, parent_doubles(plan, path, *dims))


@pytest.mark.parametrize("nEl,nk,n2", SHAPES, ids=["%dx%d_n2_%d" % s for s in SHAPES])
def test_every_plan_fills_its_count_and_stays_within_the_parent_request(cli, nEl, nk, n2):
    got = plans(cli, nEl, nk, n2)
    want = {("colop", "0"), ("colop", "1"), ("quad", "-"), ("blockinv", "0"), ("blockinv", "1"), ("schur", "-"), ("sweep", "-"),
            ("newton", "0"), ("newton", "1")}
    if nk >= 4:                                          # the _3 solve takes nk >= 4
        want |= {("s3fused", "-")} | {("schur3", "%d%d%d%d" % (a, b, c, d)) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)}
    assert set(got) == want
    for (plan, path), (count, members) in got.items():
        assert count > 0
        check(plan, path, count, members, (nEl, nk, n2, mp12_of(n2)))


def test_the_3_solve_still_asks_for_more_than_colop_apply(cli):
    """tests/test_gpu_graph_workspaces.py grows d_col by a solve_schur_3 after a colop_apply: order 3, two elements per face edge, four levels"""
    got = plans(cli, 6 * 2 * 2, 4, 9)
    assert got[("s3fused", "-")][0] > got[("colop", "0")][0]


def test_the_checker_notices_an_overlap_a_gap_and_a_short_member(cli):
    count, members = plans(cli, 6, 4, 9)[("schur3", "1110")]
    dims = (6, 4, 9, 16)
    check("schur3", "1110", count, members, dims)
    off, need, alias = members["GG"]
    for spoilt in ({**members, "GG": (members["GN"][0], need, alias)},              # two members in one place
                   {**members, "GG": (off + 1, need, alias)},                       # GN one double too long, GG one short
                   {**members, "Cv": (-1, -1, "-")},                                # a take that no member holds
                   {**members, "Mrt": (members["Ainv"][0], members["Mrt"][1], "B")}):     # re-use that is not the member it names
        with pytest.raises(AssertionError):
            check("schur3", "1110", count, spoilt, dims)
    with pytest.raises(AssertionError):
        check("schur3", "1110", count - 1, members, dims)                    # a buffer one double short of the plan


def test_an_offset_that_cannot_be_held_is_reported(cli):
    r = subprocess.run([cli, "overflow"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.split() == ["overflow", "1"], (r.returncode, r.stdout, r.stderr[-2000:])
