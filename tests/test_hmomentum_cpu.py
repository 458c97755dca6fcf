"""The spectral bound behind MassSolver.solve_fric (mimsem_amd/krylov.py friction_interval), checked on dense matrices without a GPU: with the
element-block preconditioner P of the 1-form mass solve, every eigenvalue of P (M1 + M1ray(tau)) lies in
friction_interval(lmin(P M1), lmax(P M1), tau) -- and the widening is needed: an exaggerated tau pushes eigenvalues well past lmax(P M1)."""
import numpy as np
import pytest

from tests.hmomentum_case import K_F, Sphere

LEV = 2


@pytest.fixture(scope="module")
def spectra(oracle):
    S = Sphere(oracle, 3)
    ek, es = S.exner(np.random.default_rng(97), LEV)               # sigma in [0.5, 1] per element: both branches of compute_k_v
    Lc = np.linalg.cholesky(S.precond(LEV))                        # P = Lc Lc^T: spec(P A) = spec(Lc^T A Lc), a symmetric problem
    M1 = S.m1(LEV)
    ev = lambda A: np.linalg.eigvalsh(Lc.T @ A @ Lc)
    return S, ek, es, M1, ev, ev(M1)


@pytest.mark.parametrize("tau", [240.0, 1.0 / K_F], ids=["tau240", "tau1overKF"])
def test_spectrum_lies_in_the_friction_interval(spectra, tau):
    from mimsem_amd.krylov import friction_interval
    S, ek, es, M1, ev, ev0 = spectra
    Mray = S.m1ray(LEV, tau, ek, es)
    assert np.abs(Mray).max() > 0                                  # sigma > 0.7 somewhere on this level
    lo, hi = friction_interval(ev0[0], ev0[-1], tau)
    assert lo == ev0[0] and hi == ev0[-1] * (1.0 + tau * K_F)
    lam = ev(M1 + Mray)
    print("tau %g: spec(P M1) [%.6f, %.6f], spec(P (M1 + M1ray)) [%.6f, %.6f], interval [%.6f, %.6f]" % (tau, ev0[0], ev0[-1], lam[0], lam[-1], lo, hi))
    assert lam[0] >= lo * (1.0 - 1e-12) and lam[-1] <= hi * (1.0 + 1e-12)


def test_the_widening_is_needed(spectra):
    """tau = 1/K_F doubles the interval; the spectrum follows it past lmax(P M1)"""
    S, ek, es, M1, ev, ev0 = spectra
    lam = ev(M1 + S.m1ray(LEV, 1.0 / K_F, ek, es))
    assert lam[-1] > 1.05 * ev0[-1], (lam[-1], ev0[-1])
