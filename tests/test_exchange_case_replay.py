"""The drop-in exchange cases (tests/golden/exchange_dropin/<case>.npz, tools/exchange_case_fixture) replayed without any reference code:
the case's recursion problem through Recursion.recur_b_ij / chebyshev_recur_ij, then Exchange.compute on the chains left on the device
(i == j pairs: one compacted chain), against the compiled reference's own exchange routines on its own chains.

xc, fo, parts and the cumulative J of fort.150 are compared at 1e-10 relative.  The values that vanish by symmetry (D, the off-diagonal
I) are roundoff residuals of terms of J's size, so they get an absolute floor of 1e-12 of the case's largest |J|.  The second-order
images are compared with the reference's printed rows (7 digits; the routine keeps its full-precision values local)."""
import os

import numpy as np
import pytest

from helpers import objects_from
from rslmtoasa_amd.exchange import Exchange
from rslmtoasa_amd.green import Green
from rslmtoasa_amd.recursion import Recursion

pytestmark = pytest.mark.gpu
CASES_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exchange_dropin")
CASES = ["Example_exchange_bccFe", "Example_exchange_bccFe_hoh", "Generated_exchange_bccFe_chebyshev"]      # the manifest cases that have a fixture


def load_case(name):
    with np.load(os.path.join(CASES_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def replay(z):
    p = {k: z[k] for k in ("nn", "iz", "ee", "lsham", "eeo", "enim") if k in z}
    p.update(nmax=0, hoh=int(z["hoh"]), nsp=int(z["nsp"]))
    ham, lat, ctl, en = objects_from(p, [1], int(z["lld"]), nsp=int(z["nsp"]), emin=float(z["emin"]), emax=float(z["emax"]))
    lat.ijpair = np.asarray(z["pairs"], np.int32)
    rec = Recursion(ham, lat, ctl, en)
    try:
        kind = str(z["kind"])
        if kind == "block":
            rec.recur_b_ij()
        else:
            rec.chebyshev_recur_ij()
        g = Green(rec, np.asarray(z["ene"], np.float64))
        return Exchange(rec, g).compute(float(z["fermi"]), int(z["nv1"]), z["dpar"], kind=kind, cumulative=True, resident=True)
    finally:
        rec.close()


def printed_unit(v, digits=7):
    """Half a unit in the last digit of v printed with `digits` significant digits (es16.6)."""
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log10(np.where(v > 0, v, 1.0)))
    return 0.5 * 10.0 ** (e - (digits - 1))


@pytest.mark.parametrize("name", CASES)
def test_exchange_case_replay_matches_reference(name):
    z = load_case(name)
    xc, so, fo, parts, jcum = replay(z)
    floor = 1e-12 * np.abs(z["xc"][0]).max()
    for what, mine, ref in (("xc", xc, z["xc"]), ("fo", fo, z["fo"]), ("parts", parts, z["parts"])):
        assert mine.shape == ref.shape, what
        err = np.abs(mine - ref)
        bad = err > 1e-10 * np.abs(ref) + floor
        assert not bad.any(), (what, np.argwhere(bad)[:5], mine[bad][:5], ref[bad][:5])
    # printed at 7 digits: both roundings plus the reference's own digits
    ref = z["so_printed"]
    bad = np.abs(so - ref) > printed_unit(ref) + 1e-9 * np.abs(ref) + floor
    assert not bad.any(), ("so", np.argwhere(bad)[:5], so[bad][:5], ref[bad][:5])
    f150 = z["fort150"]                                    # (nen, 2, len(f150_pairs)): ene - fermi, cumulative J
    for k, p in enumerate(z["f150_pairs"]):
        assert np.allclose(f150[:, 0, k], z["ene"] - z["fermi"], rtol=0, atol=1e-14)
        err = np.abs(jcum[:, p] - f150[:, 1, k])
        assert err.max() <= 1e-10 * np.abs(f150[:, 1, k]).max(), (p, err.max())
