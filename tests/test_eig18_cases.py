"""The inputs and bars of tests/test_gpu_eig18.py and tests/test_gpu_prescribed_chain.py, proven sound on the CPU before a GPU sees them:
the integer family squares exactly, the fixture's roots square back to its inputs in integer arithmetic, and the CPU oracle (a cyclic
Jacobi in plain C, oracle/rsrec_oracle.c) stays inside every bar the device is held to when it plays the device itself.

Measured with the oracle (forward error to the exact root, relative Frobenius): 2e-16 .. 1.3e-14 on the well-conditioned classes,
2.8e-12 on the real integer case (cond(B) = 7e5), 1.4e-13 / 8e-12 on the graded spectra 1e-8 / 1e-12; backward error <= 1.5e-14,
asymmetry <= 1.6e-16.  Chains: eig(b2_b) within 42 eps and eig(a_b) within 29 eps of the prescribed spectra (bar: 1e-13 = 450 eps)."""
import numpy as np
import pytest

import eig18_cases as EC

EPS = 2.0 ** -52


def stack(cases):
    return np.asfortranarray(np.stack([c[1] for c in cases], axis=2))


@pytest.fixture(scope="module")
def families():
    fam = {"exact": EC.exact_cases(), "diagonal": EC.diagonal_cases(), "spectrum": EC.spectrum_cases_with_roots(), "perturbed": EC.perturbed_cases()}
    for cases in fam.values():
        for _, S, B in cases:
            S.setflags(write=False)
            B.setflags(write=False)
    return fam


def test_integer_family_squares_exactly(families):
    names = [n for n, _, _ in families["exact"]]
    assert names == ["dense0", "dense1", "spin_diagonal", "real", "seven_identity", "kron3x6_mixed", "kron9x2"]
    for name, S, B in families["exact"]:
        assert np.array_equal(B, B.conj().T) and np.array_equal(S, S.conj().T)
        assert np.array_equal(B, np.round(B.real) + 1j * np.round(B.imag)) and np.abs(S).max() < 2.0 ** 40
        assert np.array_equal(B @ B, S)                                   # every partial sum is an integer below 2^53
        assert np.linalg.eigvalsh(B).min() > 0
    by = {n: B for n, _, B in families["exact"]}
    assert np.abs(by["spin_diagonal"][:9, 9:]).max() == 0 and np.abs(by["real"].imag).max() == 0
    assert 1e5 < np.linalg.cond(by["real"]) <= 1e6
    for name, mult in (("kron3x6_mixed", 6), ("kron9x2", 9)):             # the degeneracies are exact
        ev = np.linalg.eigvalsh(by[name])
        groups = ev.reshape(-1, mult)
        assert (np.ptp(groups, axis=1) < 1e-12 * ev.max()).all() and (np.diff(groups[:, 0]) > 1e-3).all()
    for name, S, B in families["diagonal"]:
        assert np.array_equal(S, np.diag(np.diagonal(S))) and np.array_equal(B, np.diag(np.sqrt(np.diagonal(S).real)))


def as_integers(a):
    """The complex double matrix `a` as (re, im, e): integer object arrays with a = (re + i im) 2^e exactly."""
    parts = [np.asarray(a.real, dtype=np.float64), np.asarray(a.imag, dtype=np.float64)]
    e = min(int(np.frexp(x[x != 0])[1].min()) for x in parts if x.any()) - 53
    conv = np.vectorize(lambda v: int(np.ldexp(v, -e)), otypes=[object])
    for x in parts:
        assert np.array_equal(np.ldexp(np.ldexp(x, -e), e), x)
    return conv(parts[0]), conv(parts[1]), e


def test_fixture_roots_square_back_to_the_inputs(families):
    """(root_hi + root_lo)^2 = S to 1e-30 ||S||, in exact integer arithmetic: no high-precision library on the test's side."""
    roots = EC.load_roots()
    assert len(roots) == 20
    for name, S in EC.spectrum_cases():
        S0, hi, lo = roots[name]
        assert EC.same_bits(S, S0)
        assert np.abs(lo).max() <= 2.0 ** -52 * np.abs(hi).max() and np.array_equal(hi, hi.conj().T)
        hr, hi_, eh = as_integers(hi)
        lr, li, el = as_integers(lo)
        e = min(eh, el)
        rr = hr * 2 ** (eh - e) + lr * 2 ** (el - e)
        ri = hi_ * 2 ** (eh - e) + li * 2 ** (el - e)
        sr, si, es = as_integers(S)
        pr, pi = rr.dot(rr) - ri.dot(ri), rr.dot(ri) + ri.dot(rr)               # (root)^2 2^(-2e), exact
        sh = es - 2 * e
        assert sh >= 0
        dr, di = pr - sr * 2 ** sh, pi - si * 2 ** sh
        num = sum(int(x) ** 2 for x in dr.ravel()) + sum(int(x) ** 2 for x in di.ravel())
        den = sum(int(x) ** 2 for x in sr.ravel()) + sum(int(x) ** 2 for x in si.ravel())
        # num / (den 4^sh) <= 1e-60, in integers
        assert num * 10 ** 60 <= den * 4 ** sh, (name, num, den)
        # and root_hi alone is the exact root rounded to double: it squares back to a few eps
        assert EC.fro(hi @ hi - S) <= 20 * EPS * EC.fro(S)


def test_oracle_stays_inside_the_device_bars(families, oracle_lib):
    worst = {}
    for fam, cases in families.items():
        R = oracle_lib.zsqr(stack(cases))
        for i, (name, S, B) in enumerate(cases):
            r = R[:, :, i]
            assert np.isfinite(r).all()
            if name == "zero":
                assert not r.any()
                continue
            err = EC.forward_error(r, B)
            assert np.isfinite(err) and err <= EC.forward_bar(err)
            if fam == "diagonal" or name == "seven_identity":
                assert EC.same_bits(r, B)                                    # the exit before the first sweep
            else:
                assert err > 0                                               # 16 x this is a bar that means something
            back, asym, neg = EC.structure_errors(r, S)
            print("oracle %-10s %-24s forward %.2e backward %.2e asymmetry %.2e" % (fam, name, err, back, asym))
            assert back <= EC.BACKWARD and asym <= EC.BACKWARD and neg <= EC.BACKWARD
            worst[fam] = max(worst.get(fam, 0.0), err)
    # well-conditioned classes: the oracle itself is far inside the absolute bar
    assert worst["exact"] < 1e-11 and worst["spectrum"] < 1e-10


def test_oracle_is_covariant_under_powers_of_two(oracle_lib):
    for name, S, B in EC.scale_bases():
        r0 = oracle_lib.zsqr(stack([(name, S)]))[:, :, 0]
        ks = EC.SCALE_IN + EC.SCALE_OUT
        R = oracle_lib.zsqr(np.asfortranarray(np.stack([EC.scaled(S, k) for k in ks], axis=2)))
        for i, k in enumerate(ks):
            assert EC.same_bits(R[:, :, i], EC.scaled(r0, k // 2)), (name, k)


CHAIN_BAR = 1e-13


@pytest.mark.parametrize("kind", ["uniform", "deg3x6", "equal"])
def test_oracle_meets_the_prescribed_chain_spectra(kind, oracle_lib):
    p, sig2, E = EC.prescribed_chain(EC.chain_sigmas(kind, 5, 7), 11)
    a_b, b2_b = oracle_lib.Oracle(p).block_lanczos(np.array([1], np.int32), 6)
    eb, ea = EC.chain_spectrum_errors(a_b[:, :, :, 0], b2_b[:, :, :, 0], sig2, E)
    print("oracle chain %-8s eig(b2_b) %s eps, eig(a_b) %s eps" % (kind, np.round(eb / EPS, 1), np.round(ea / EPS, 1)))
    assert (eb <= CHAIN_BAR).all() and (ea <= CHAIN_BAR).all()
    assert np.array_equal(b2_b[:, :, 0, 0], np.eye(18)) and not a_b[:, :, 5, 0].any()


@pytest.mark.parametrize("kind", ["kappa1e4", "kappa1e8", "one_small"])
def test_oracle_on_one_ill_conditioned_level(kind, oracle_lib):
    """The bars of the device are 16 x these distances: they must be finite and non-zero.  Measured: eig(b2_b[1]) 6 / 2 / 7.6 eps,
    eig(a_b[1]) 184 / 1.8e6 / 3.2e5 eps, eig(b2_b[2]) 137 / 1.8e6 / 6.3e5 eps (kappa 1e4 / kappa 1e8 / one sigma = 1e-4)."""
    p, sig2, E = EC.prescribed_chain(EC.graded_sigmas(kind, 8), 12)
    a_b, b2_b = oracle_lib.Oracle(p).block_lanczos(np.array([1], np.int32), 3)
    eb, ea = EC.chain_spectrum_errors(a_b[:, :, :, 0], b2_b[:, :, :, 0], sig2, E)
    print("oracle chain %-8s eig(b2_b) %s eps, eig(a_b) %s eps" % (kind, eb / EPS, ea / EPS))
    for x in (eb[0], ea[1], eb[1]):
        assert np.isfinite(x) and 0 < x < 1e-8
    assert eb[0] <= CHAIN_BAR                     # the graded B_1^2 itself is a plain Gram matrix: as accurate as any
