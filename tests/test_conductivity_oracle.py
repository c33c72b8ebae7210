"""The numpy restatement of the conductivity integrand (tests/cond_reference.py) against the COMPILED REFERENCE's
calculate_gamma_nm + calculate_conductivity_tensor (tests/golden/cond_integrand_L*.npz, tools/cond_fixture), and the factorised
form the GPU kernel computes against the direct Gamma sum.  CPU only."""
import numpy as np
import pytest

import cond_reference as R
from helpers import load_golden

CASES = ["cond_integrand_L7", "cond_integrand_L24"]


def fixture(name):
    z = load_golden(name)
    L, nvec = int(z["cond_ll"]), int(z["nvec"])
    mu = np.zeros((18, 18, L, L, nvec), np.complex128)
    mu[np.arange(18), np.arange(18)] = z["mu_diag"]
    return z, L, mu, float(z["energy_min"]), float(z["energy_max"])


@pytest.mark.parametrize("name", CASES)
def test_gamma_matches_reference(name):
    z, L, mu, emin, emax = fixture(name)
    assert np.array_equal(z["ene"], R.energy_mesh(emin, emax, int(z["channels_ldos"])))
    G = R.gamma_nm(z["ene"], emin, emax, L)[z["gamma_rows"]]
    ref = z["gamma_nm"]
    scale = np.abs(ref).max(axis=(1, 2))[:, None, None]            # per energy: Gamma(i, n, m) cancels to ~0 for some (n, m)
    assert (np.abs(G - ref) / scale).max() <= 1e-14


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("calctype", ["per_type", "random_vec"])
def test_integrand_matches_reference_fort123(name, calctype):
    z, L, mu, emin, emax = fixture(name)
    I = R.integrand_direct(R.gamma_nm(z["ene"], emin, emax, L), mu, emin, emax)
    mine, ref = R.fort123(I, z["ene"], emin, emax, float(z["fermi"])), z["fort123_" + calctype]
    assert mine.shape == ref.shape
    # es16.6: seven significant digits; a printed value is within half a unit of its last digit
    ulp = 10.0 ** np.floor(np.log10(np.maximum(np.abs(ref), 1e-300))) * 1e-6
    assert np.all(np.abs(mine - ref) <= 0.5 * ulp * 1.02 + 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_factorised_form_equals_direct_sum(name):
    z, L, mu, emin, emax = fixture(name)
    direct = R.integrand_direct(R.gamma_nm(z["ene"], emin, emax, L), mu, emin, emax)
    fact = R.integrand_factorised(mu, z["ene"], emin, emax)
    assert np.abs(fact - direct).max() <= 1e-13 * np.abs(direct).max()


@pytest.mark.parametrize("L", [1, 2, 5, 17])
def test_factorised_form_on_full_random_moments(L):
    """Off-diagonal blocks present (the reference reads only mu(l, l, ...)), L = 1 included, energies reaching past energy_max."""
    rng = np.random.default_rng(L)
    mu = rng.standard_normal((18, 18, L, L, 3)) + 1j * rng.standard_normal((18, 18, L, L, 3))
    ene = R.energy_mesh(-1.3, 0.4, 120)            # (fewer channels put the last of the 10 extra points past |x| = 1)
    direct = R.integrand_direct(R.gamma_nm(ene, -1.3, 0.4, L), mu, -1.3, 0.4)
    fact = R.integrand_factorised(mu, ene, -1.3, 0.4)
    assert np.abs(fact - direct).max() <= 1e-13 * np.abs(direct).max()
