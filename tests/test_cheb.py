"""namespace cheb of mimsem_amd/host/mimsem_mass.hpp (host-only C++: coefficients, safety margins, step count and the acceptance rule of the
fixed-length solves, shared by every C++ host) against the Python hosts' arithmetic in mimsem_amd/krylov.py, through tests/cpp/cheb_cli.cpp.
The same sequence of double operations in both languages: coefficients to 1e-15 (and whether they came out bit-equal is printed), margins and
step counts exactly.  No GPU, no library."""
import math
import os
import subprocess

import pytest

from mimsem_amd.krylov import chebyshev_ellipse_coefs, ritz_margins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cheb") / "cheb_cli")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "cheb_cli.cpp"), "-o", exe])
    return exe


def _run(cli, *args):
    out = subprocess.run([cli] + [a if isinstance(a, str) else repr(float(a)) for a in args], capture_output=True, text=True, check=True).stdout
    return [[float(x) for x in line.split()] for line in out.splitlines()]


@pytest.mark.parametrize("d,c2,steps", [(1.0, 0.04, 20), (1.0, -0.07, 17)], ids=["real_interval", "imaginary_foci"])
def test_coefficients_match_python(cli, d, c2, steps):
    got = _run(cli, "ellipse", d, c2, str(steps))
    want = chebyshev_ellipse_coefs(d, c2, steps)
    assert len(got) == len(want) == steps
    print("coefficients bit-equal: %s" % all(g[0] == w[0] and g[1] == w[1] for g, w in zip(got, want)))
    for (ga, gb), (wa, wb) in zip(got, want):
        assert abs(ga - wa) <= 1e-15 * abs(wa) and abs(gb - wb) <= 1e-15 * abs(wb)


def test_margins_match_python(cli):
    """Movement of the ends between the two estimates below the 1 % floor, between floor and cap, and above the cap, at widen 1 and 2.5, for
    the caps of SWEqn / ThermalSW (0.4 / none: krylov.ritz_margins as sweqn.py calls it) and of HorizSolve (0.10 / 0.05: at widen 1
    krylov.ritz_margins as MassSolver calls it, with the capped movement; HorizSolve never widens, so at widen 2.5 the reference is
    ritz_margins' own line with these caps in the place of its 0.4 / none)."""
    lo, hi = 0.8, 1.25
    for widen in (1.0, 2.5):
        for f in (0.001, 0.01, 0.02, 0.2):                      # 3 f = 0.3 %, 3 %, 6 %, 60 %
            lo_p, hi_p = lo * (1.0 + f), hi * (1.0 - f)
            e_lo, e_hi = 3.0 * abs(lo - lo_p) / lo, 3.0 * abs(hi - hi_p) / hi
            (got,) = _run(cli, "margins", lo, hi, lo_p, hi_p, 0.4, "inf", widen)
            assert tuple(got) == ritz_margins(lo, hi, e_lo, e_hi, widen), (widen, f)
            (got,) = _run(cli, "margins", lo, hi, lo_p, hi_p, 0.10, 0.05, widen)
            want = (1.0 - min(0.10, max(0.01, e_lo, 0.1 * (widen - 1.0))), 1.0 + min(0.05, max(0.01, e_hi, 0.05 * (widen - 1.0))))
            assert tuple(got) == want, (widen, f)
            if widen == 1.0:
                assert want == ritz_margins(lo, hi, min(0.10, e_lo), min(0.05, e_hi)), f


def test_step_count_matches_python(cli):
    l1, l2, rtol = 0.8, 1.25, 1e-14
    sg = (math.sqrt(l2 / l1) - 1.0) / (math.sqrt(l2 / l1) + 1.0)                    # krylov.ChebyshevMass
    want = max(2, int(math.ceil(math.log(2.0 / rtol) / math.log(1.0 / sg))))
    assert _run(cli, "steps", l1, l2, rtol) == [[want]]


@pytest.mark.parametrize("r2,ref2,bound,accept", [(0.0, 0.0, 3e-13, True), (1e-30, 1.0, 3e-13, True), (1e-20, 1.0, 3e-13, False), (1.0, 0.0, 3e-13, False),
                                                  ("nan", 1.0, 3e-13, False), (1.0, "nan", 3e-13, False), (0.0, "nan", 3e-13, False)])
def test_acceptance_rule(cli, r2, ref2, bound, accept):
    assert _run(cli, "accepted", r2, ref2, bound) == [[1.0 if accept else 0.0]]
