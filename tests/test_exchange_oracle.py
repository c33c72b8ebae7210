"""The numpy restatement of the exchange workflow (exchange_reference.py) against the compiled reference's own calculate_intersite_gf /
_twoindex and calculate_exchange / _twoindex (tests/golden/exchange_*.npz, tools/exchange_fixture): block, Chebyshev and Chebyshev +
hoh pair chains with an i == j pair, g0 from the C oracle."""
import numpy as np
import pytest

from exchange_reference import exchange_pair, fixture_g0
from helpers import load_golden

CASES = ["exchange_block", "exchange_cheb", "exchange_cheb_hoh"]


def rel(mine, ref, floor):
    return np.abs(np.asarray(mine) - np.asarray(ref)).max() / max(np.abs(ref).max(), floor)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_compiled_reference(name, oracle_lib):
    z = load_golden(name)
    ene, fermi, nv1 = z["ene"], float(z["fermi"]), int(z["nv1"])
    for p in range(len(z["pairs"])):
        xc, so, fo, parts, jcum, _ = exchange_pair(fixture_g0(z, p), bool(z["same"][p]), z["dpar"][..., p], ene, fermi, nv1)
        floor = max(np.abs(z["xc"][:, p]).max(), np.abs(z["fo"][:, p]).max(), np.abs(z["parts"][:, p]).max()) * 1e-2
        assert rel(xc, z["xc"][:, p], floor) <= 1e-12, (name, p)
        assert rel(fo, z["fo"][:, p], floor) <= 1e-12, (name, p)
        assert rel(parts, z["parts"][:, p], floor) <= 1e-12, (name, p)
        # the second-order row as printed (es16.6, 7 significant digits): within one unit of the last printed digit, values that vanish
        # by symmetry judged on the pair's scale
        ref = z["so_printed"][:, p]
        ulp = 10.0 ** (np.floor(np.log10(np.maximum(np.abs(ref), 1e-300))) - 6)
        assert np.all(np.abs(so - ref) <= np.maximum(ulp, 1e-12 * floor)), (name, p, so, ref)
        # fort.150: ene(nv) - fermi and the cumulative J at Ef = ene(nv)
        f150 = z["fort150"][..., p]
        assert np.allclose(f150[:, 0], ene - fermi, rtol=0, atol=1e-15)
        assert rel(jcum, f150[:, 1], 0.0) <= 1e-12, (name, p)
        assert np.abs(xc).max() > 0 and np.abs(jcum).max() > 0
