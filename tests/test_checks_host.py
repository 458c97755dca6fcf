"""mimsem_amd.checks on the host: THE acceptance rule of a check (cheb::relative / cheb::accepted of mimsem_amd/host/mimsem_mass.hpp) and the
two step-count rules against the formulas the hosts carried inline before the module existed."""
import math

import numpy as np
import pytest

from mimsem_amd.checks import accepted, interval_rate, interval_steps, rate_steps

BOUND = 3.0e-13
NAN = float("nan")


def _one(r2, ref2, bound=BOUND):
    """one pair through the rule -- as two Python floats and as arrays, which must agree"""
    ok, rel = accepted(float(r2), float(ref2), bound)
    oka, rela = accepted(np.array([r2, r2]), np.array([ref2, ref2]), bound)
    assert type(ok) is bool and oka.tolist() == [ok, ok] and (rela.tolist() == [rel, rel] or (math.isnan(rel) and np.isnan(rela).all()))
    return ok, float(rel)


def test_accepted_table():
    assert _one(0.0, 0.0) == (True, 0.0)                                   # a slot not written, a zero right-hand side
    ok, rel = _one(1e-3, 0.0)
    assert not ok and math.isnan(rel)                                      # a residual against a zero reference
    for r2 in (0.0, 1e-40, 1.0):
        assert not _one(r2, -1.0)[0]                                       # a negative reference
    for r2, ref2 in ((NAN, 1.0), (1.0, NAN), (NAN, NAN), (NAN, 0.0), (0.0, NAN)):
        assert not _one(r2, ref2)[0], (r2, ref2)
    assert not _one(-1e-30, 1.0)[0]                                        # (a negative |r|^2 is no number either)
    assert _one(1e-30, 1.0) == (True, math.sqrt(1e-30))


@pytest.mark.parametrize("r2,ref2", [(2.0 ** -80, 1.0), (9.0e-26, 4.0), (1.7e-27, 1.0), (3.3e-9, 2.5e17)])
def test_accepted_at_the_bound(r2, ref2):
    """rel exactly at the bound is accepted, the next double above the bound is a miss -- as a pair and in the ratio form"""
    rel = math.sqrt(r2 / ref2)
    below = float(np.nextafter(rel, 0.0))                                         # the bound whose next double above is rel
    for a, b in ((r2, ref2), (r2 / ref2, 1.0)):
        assert _one(a, b, rel) == (True, rel)
        assert _one(a, b, below) == (False, rel)
        assert _one(a, b, float(np.nextafter(rel, 1.0)))[0]


def test_accepted_is_vectorised_and_the_ratio_form_takes_the_same_cases():
    r2 = np.array([0.0, 1e-3, 1.0, NAN, 1.0, 4e-28, 1e-20])
    ref2 = np.array([0.0, 0.0, -1.0, 1.0, NAN, 1.0, 1.0])
    ok, rel = accepted(r2, ref2, 2.5e-14)
    assert ok.tolist() == [True, False, False, False, False, True, False]
    assert rel[0] == 0.0 and rel[5] == math.sqrt(4e-28) and rel[6] == math.sqrt(1e-20) and np.isnan(rel[1:5]).all()
    # a logged ratio |r|^2 / |ref|^2 (the device forms it as num / max(den, 1e-300) and keeps a NaN): accepted(ratio, 1, bound)
    ratio = np.array([[0.0, 1e-3 / 1e-300, NAN], [4e-28, 1e-20, float("inf")]])
    ok, rel = accepted(ratio, 1.0, 2.5e-14)
    assert ok.tolist() == [[True, False, False], [True, False, False]] and rel.shape == ratio.shape


def test_step_counts_equal_the_inline_formulas():
    for lmin in (0.3, 0.8):
        for lmax in (1.05, 1.2, 3.0):
            kappa = lmax / lmin
            sg = (math.sqrt(kappa) - 1.0) / (math.sqrt(kappa) + 1.0)
            assert interval_rate(lmin, lmax) == sg
            for rtol in (1e-10, 1e-14, 1e-15):
                # ChebyshevMass.__init__ ...
                assert interval_steps(lmin, lmax, rtol) == max(2, int(math.ceil(math.log(2.0 / rtol) / math.log(1.0 / sg)))), (lmin, lmax, rtol)
                # ... and GraphedChebyshev.__init__, whose rate is that of its interval
                assert rate_steps(interval_rate(lmin, lmax), rtol) == max(2, int(math.ceil(math.log(0.5 * rtol) / math.log(sg))) + 1)
    for rate in (0.05, 0.3, 0.59):
        for rtol in (1e-10, 1e-14, 1e-15):
            # the nq = ... line of the shallow-water host's upwinded 0-form mass
            assert rate_steps(rate, rtol) == max(2, int(math.ceil(math.log(0.5 * rtol) / math.log(rate))) + 1), (rate, rtol)
    assert interval_steps(0.999999, 1.000001, 1e-1) == 2 and rate_steps(1e-9, 1e-1) == 2          # the floor of two steps
