"""The two recursion drivers share one call setup (RecursionCall in rsrec.hip: kernel choice, reservations, batch prologue, the H|psi>
step, the side-stream hand-off): block Lanczos and Chebyshev interleaved on one handle must not see each other."""
import numpy as np
import pytest

from helpers import RTOL, objects_from, rel_err, supercell_problem
from rslmtoasa_amd.recursion import Recursion, chebyshev_scaling

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hoh", [False, True])
@pytest.mark.parametrize("spmm5", [1, 2])
def test_interleaved_recursions_leak_no_state(hoh, spmm5, oracle_lib):
    """recur_b, chebyshev_recur, recur_b, chebyshev_recur on one handle, then both once more without the side stream: every repeat gives
    the bits of the first call (work vectors, partials, seeds, the status word and the side-stream events are shared between the two), and
    those agree with the CPU oracle.  Three sites in batches of two: the second batch is short.  (The 4 x 4 x 8 cell has 128 atoms; the
    third site is its last atom.)  No tolerance on the repeats."""
    lld, batch = 8, 2
    p = supercell_problem((4, 4, 8), hoh=hoh)
    sites = np.array([1, 77, p["nn"].shape[0]], dtype=np.int32)
    nbatches = (len(sites) + batch - 1) // batch
    rec = Recursion(*objects_from(p, sites, lld, emin=-3.0, emax=1.8), device=0)
    for key, val in (("batch", batch), ("spmm5", spmm5), ("graph", 1)):
        rec.set_option(key, val)

    def lanczos():
        rec.a_b[:] = 0
        rec.b2_b[:] = 0
        rec.recur_b()
        return rec.a_b.copy(), rec.b2_b.copy()

    def chebyshev():
        rec.mu_n[:] = 0
        rec.chebyshev_recur()
        return rec.mu_n.copy()

    a0, b0 = lanczos()
    m0 = chebyshev()
    a1, b1 = lanczos()
    m1 = chebyshev()
    rec.set_option("side_stream", 0)
    a2, b2 = lanczos()
    m2 = chebyshev()
    # the H|psi> launches the call counts: one per level, two with hoh, in every batch (the launch-per-kernel path)
    rec.set_option("graph", 0)
    a3, b3 = lanczos()
    hops = rec.timing()["hop_launches"]
    rec.close()
    for a, b, m in ((a1, b1, m1), (a2, b2, m2), (a3, b3, m0)):
        assert np.array_equal(a, a0) and np.array_equal(b, b0) and np.array_equal(m, m0)
    assert hops == (lld - 1) * (2 if hoh else 1) * nbatches
    o = oracle_lib.Oracle(p)
    a_o, b_o = o.block_lanczos(sites, lld)
    mu_o, rc = o.chebyshev(sites, lld, *chebyshev_scaling(-3.0, 1.8))
    assert rc == 0
    assert rel_err(a0, a_o) < RTOL and rel_err(b0, b_o) < RTOL and rel_err(m0, mu_o) < RTOL
