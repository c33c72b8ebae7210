"""A chain's results do not depend on which other chains share its call: every chain ALONE against the same chain inside joint calls, bit for
bit, for the block-Lanczos and Chebyshev drivers and every form of the post-hop pass.

The lattice (tests/piece_lattices.py, conditions in tests/test_piece_lattices.py) has four disconnected pieces of 384, 771, 1203 and 1603 atoms;
a chain seeded in a piece saturates at 12, 25, 38 or 51 workgroups (seeds s12, s25, s38, s51), so the chains of one call differ in size and the
launch of a level is sized by the largest.  The partial sums of a level are summed in blocks of 16 and then over the blocks
(kernels_mfma.hpp, sum_partials16): the order depends on the chain's own partial count only.  [s25, s51] is the call that tells: alone, s25 has
25 partials in a launch of 25 workgroups (single-stage sum); beside s51 the launch has 51 and the two-stage sum (k_presum16) runs.  With a
sequential single-stage sum, ((p0 + p1) + ...) + p24, against (p0 + ... + p15) + (p16 + ... + p24), the two differ in the last bits.  [s12, s25]
(neither side presums) and s38 / s51 (both sides presum) are controls.

Every joint result is also held to the CPU oracle, so that "the same bits" cannot be "the same wrong bits"; and a handle that ran the largest
chain gives the smallest chain the bits of a fresh handle (zero block and the regions outside the chain's own in the rotating work vectors)."""
import numpy as np
import pytest

import piece_lattices as PL
from helpers import RTOL, objects_from, rel_err
from rslmtoasa_amd.recursion import Recursion, chebyshev_scaling

pytestmark = pytest.mark.gpu

SEEDS = PL.BATCH_SEEDS
JOINT = (("s25", "s51"), ("s12", "s25"), ("s12", "s25", "s38", "s51"), ("s51", "s25"))
FORMS = {"oop": {"orth3": 1, "orth_oop": 1}, "inplace": {"orth3": 1, "orth_oop": 0}, "lds": {"orth3": 2}}
CI, RM = {"kernels": 2, "spmm5": 2}, {"kernels": 2, "spmm5": 1}
DRIVERS = {   # name -> (driver, hoh, options)
    "lanczos_ci": ("lanczos", False, CI),
    "lanczos_rm": ("lanczos", False, RM),
    "lanczos_ci_hoh": ("lanczos", True, CI),
    "lanczos_rm_hoh": ("lanczos", True, RM),
    "cheb_fused": ("cheb", False, dict(CI, cheb_fused=1)),
    "cheb_unfused": ("cheb", False, dict(CI, cheb_fused=0)),
    "cheb_fused_hoh": ("cheb", True, dict(CI, cheb_fused=1)),
    "cheb_unfused_hoh": ("cheb", True, dict(CI, cheb_fused=0)),
    "lanczos_form_oop": ("lanczos", False, dict(CI, **FORMS["oop"])),
    "lanczos_form_inplace": ("lanczos", False, dict(CI, **FORMS["inplace"])),
    "lanczos_form_lds": ("lanczos", False, dict(CI, **FORMS["lds"])),
    "lanczos_valu": ("lanczos", False, {"kernels": 1}),
}
SETTINGS = {"default": {}, "nblk128": {"nblk": 128}, "nblk16": {"nblk": 16}, "graph0": {"graph": 0}, "graph2": {"graph": 2},
            "side0": {"side_stream": 0}, "side1": {"side_stream": 1}}
CASES = [(d, s) for d in DRIVERS for s in SETTINGS if d != "lanczos_valu" or s.startswith("nblk")]   # the VALU set's grid is fixed per chain once nblk is pinned


@pytest.fixture(scope="module")
def problems():
    return {hoh: PL.batch_problem(hoh) for hoh in (False, True)}


@pytest.fixture(scope="module")
def oracle_results(oracle_lib, problems):
    """(driver, hoh) -> {seed name: oracle arrays of that chain}, computed once and left unchanged."""
    cache = {}

    def get(driver, hoh):
        if (driver, hoh) not in cache:
            names = sorted(SEEDS)
            irec = np.array([SEEDS[n] for n in names], np.int32)
            o = oracle_lib.Oracle(problems[hoh])
            if driver == "lanczos":
                arrays = o.block_lanczos(irec, PL.BATCH_LLD)
            else:
                mu, div = o.chebyshev(irec, PL.BATCH_LLD, *chebyshev_scaling(PL.EMIN, PL.EMAX))
                assert div == 0
                arrays = (mu,)
            for x in arrays:
                x.setflags(write=False)
            cache[(driver, hoh)] = {n: tuple(x[..., i] for x in arrays) for i, n in enumerate(names)}
        return cache[(driver, hoh)]
    return get


def engine(p, options):
    rec = Recursion(*objects_from(p, [1], PL.BATCH_LLD, emin=PL.EMIN, emax=PL.EMAX), device=0)
    for k, v in options.items():
        rec.set_option(k, v)
    return rec


def run(rec, driver, names):
    """One call with the chains `names`: {name: (a_b, b2_b) or (mu_n,) of that chain}."""
    rec.lattice.irec = np.array([SEEDS[n] for n in names], np.int32)
    rec.restore_to_default()
    if driver == "lanczos":
        rec.recur_b()
        arrays = (rec.a_b, rec.b2_b)
    else:
        rec.chebyshev_recur()
        arrays = (rec.mu_n,)
    assert all(np.isfinite(x).all() for x in arrays)
    return {n: tuple(x[..., i].copy() for x in arrays) for i, n in enumerate(names)}


def ulp_distance(x, y):
    """Largest distance of two arrays in units of the last place of the larger entry (real and imaginary parts on their own)."""
    x, y = np.ascontiguousarray(x).view(np.float64), np.ascontiguousarray(y).view(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(x - y) / np.spacing(np.maximum(np.abs(x), np.abs(y)))
    return float(np.nanmax(np.where(x == y, 0.0, d)))


@pytest.mark.parametrize("driver_name,setting", CASES)
def test_alone_equals_joint_bitwise(driver_name, setting, problems, oracle_results):
    driver, hoh, options = DRIVERS[driver_name]
    rec = engine(problems[hoh], dict(options, **SETTINGS[setting]))
    want = oracle_results(driver, hoh)
    differ, off = [], []
    try:
        alone = {n: run(rec, driver, (n,))[n] for n in sorted(SEEDS)}
        for names in JOINT:
            joint = run(rec, driver, names)
            for n in names:
                for k, (x, y, o) in enumerate(zip(joint[n], alone[n], want[n])):
                    err = rel_err(x, o)
                    if not err < RTOL:
                        off.append(("+".join(names), n, k, err))
                    if not np.array_equal(x, y):
                        differ.append(("+".join(names), n, k, ulp_distance(x, y), rel_err(x, y)))
    finally:
        rec.close()
    assert not off, off
    for d in differ:
        print("%s %s: call [%s], chain %s, array %d: %.0f ulp apart (%.1e relative)" % ((driver_name, setting) + d))
    assert not differ, differ


@pytest.mark.parametrize("form", sorted(FORMS))
def test_small_chain_after_large_chain_on_one_handle(form, problems):
    """[s51], then [s12] on the same handle: the work vectors, the zero block and the third u vector hold the large chain's leftovers wherever
    the second call does not clear or overwrite them.  The bits must be those of a handle that never ran anything else."""
    options = dict(CI, **FORMS[form])
    rec = engine(problems[False], options)
    run(rec, "lanczos", ("s51",))
    used = run(rec, "lanczos", ("s12",))["s12"]
    rec.close()
    rec = engine(problems[False], options)
    fresh = run(rec, "lanczos", ("s12",))["s12"]
    rec.close()
    assert np.abs(fresh[0]).max() > 0
    assert np.array_equal(used[0], fresh[0]) and np.array_equal(used[1], fresh[1])
