"""exchange_gpu's calculate_gilbert_damping and its wrappers around the inherited readers of green%gij / gji, through
oracle/_ref/damping_gpu.x (tests/fortran/damping_gpu_driver.f90 on the object set of the zero-edit drop-in): the reference's bcc Fe
exchange example (tests/golden/exchange_dropin, block, lld 20, nsp 2, two pairs) up to the pair recursion, then the routine.

Case 1: alldampings.out and damping-energy.out against the numpy restatement (damping_reference.py) applied to that run's own g0,
tmat and moments, which the driver dumps; spin_i from zero per pair, damping-energy.out with the last pair's factor.
Case 2: calculate_jij_auxgreen on the exchange_gpu object against the same routine on the reference's plain type(exchange)."""
import os
import re

import numpy as np
import pytest

from damping_reference import damping_rows, factor, total_damping
from helpers import program_built
from rslmtoasa_amd._proc import run_with_unlimited_stack
from test_exchange_dropin import prepare
from test_fortran_dropin import ROOT, fortran_float

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "oracle", "_ref", "damping_gpu.x")
CASE = "Example_exchange_bccFe"
TOL = 1e-12                      # kernel against restatement, relative to the pair's largest row (test_gpu_damping.py)
HALF_UNIT = 0.5e-9               # half a unit in the last digit of an F14.9 field


def run(mode, work):
    prepare(CASE, work)
    r = run_with_unlimited_stack([DRIVER], cwd=work, env={"OMP_NUM_THREADS": "8", "RSREC_REPORT": "1", "DAMPING_DRIVER_MODE": mode}, timeout=1200,
                                 scrub=False)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "fatal" not in log.lower(), log[-3000:]
    return log


def read_dump(path):
    b = open(path, "rb").read()
    o = 0

    def take(dtype, n):
        nonlocal o
        a = np.frombuffer(b, dtype=dtype, count=n, offset=o)
        o += a.nbytes
        return a
    nen, npairs, ntype = (int(x) for x in take(np.int32, 3))
    ene = take(np.float64, nen).copy()
    fermi = float(take(np.float64, 1)[0])
    pairs, types, lmax, ql = [], [], [], []
    for _ in range(npairs):
        pairs.append(tuple(int(x) for x in take(np.int32, 2)))
        t = take(np.int32, 4)
        types.append((int(t[0]), int(t[2])))
        lmax.append(int(t[1]))
        ql.append(take(np.float64, 6).reshape(3, 2, order="F").copy())
    tmat = take(np.complex128, 18 * 18 * 3 * ntype).reshape(18, 18, 3, ntype, order="F")
    g0 = [take(np.complex128, 18 * 18 * nen * 4).reshape(18, 18, nen, 4, order="F") for _ in range(npairs)]
    assert o == len(b)
    return dict(nen=nen, ene=ene, fermi=fermi, pairs=pairs, types=types, lmax=lmax, ql=ql, tmat=tmat, g0=g0)


def split_file(path):
    """(header text, data lines): the header is written list-directed, which the compiler may wrap over several lines."""
    lines = [l for l in path.read_text().splitlines() if l.strip()]
    return " ".join(l for l in lines if l.lstrip().startswith("#")), [l for l in lines if not l.lstrip().startswith("#")]


def numbers(line):
    return [fortran_float(t) for t in line.split()]


def test_damping_files_match_the_restatement(tmp_path):
    if not program_built(DRIVER):
        return
    work = tmp_path / "run"
    log = run("damping", work)
    assert "damping-gpu" in log, log[-3000:]                          # the g_timer label of the override: the stage ran on the device
    assert "host_intersite_allocated=F" in log, log[-3000:]           # green's 24 intersite arrays were never allocated
    d = read_dump(work / "damping_dump.bin")
    npairs = len(d["pairs"])
    m = re.search(r"rsrec report: library_calls=(\d+)", log)
    # the seeded pair recursion, rsrec_damping, and the driver's own dump of g0 afterwards (per pair at most a terminator and four Green
    # calls); a host intersite stage would add as many again
    assert m and 2 <= int(m.group(1)) <= 2 + 5 * npairs, log[-2000:]
    print("library_calls", m.group(1))

    # the reference's search for the energy nearest the Fermi level (:696-702): the first strict minimum
    ief, diff = 0, 1000.0
    for nv in range(d["nen"]):
        if abs(d["ene"][nv] - d["fermi"]) < diff:
            diff, ief = abs(d["ene"][nv] - d["fermi"]), nv
    rows, facs = [], []
    for q, (i, j) in enumerate(d["pairs"]):
        tm = np.stack([d["tmat"][:, :, :, d["types"][q][0] - 1], d["tmat"][:, :, :, d["types"][q][1] - 1]], axis=3)
        rows.append(damping_rows(d["g0"][q], i == j, tm))
        n = d["lmax"][q] + 1
        facs.append(factor(d["ql"][q][:n, 0], d["ql"][q][:n, 1]))

    head, lines = split_file(work / "alldampings.out")
    assert len(lines) == npairs and "#xx" in head and "#rij" in head
    for q, (i, j) in enumerate(d["pairs"]):
        got = numbers(lines[q])
        assert (int(got[0]), int(got[1])) == (i, j) and len(got) == 16
        f, r = facs[q], rows[q]
        exp = list(f * r[:9, ief]) + [0.5 * f * (r[0, ief] + r[4, ief])]
        tol = HALF_UNIT + TOL * abs(f) * np.abs(r).max()
        dev = np.abs(np.array(got[2:12]) - np.array(exp))
        print("pair", (i, j), "factor %.6f" % f, "xx yy zz", exp[0], exp[4], exp[8], "worst deviation %.2e (bound %.2e)" % (dev.max(), tol))
        assert np.all(dev <= tol), (q, got[2:12], exp)
        assert np.abs(np.array(exp)).max() > 100 * HALF_UNIT          # the comparison sees digits

    total = total_damping(rows)
    head, lines = split_file(work / "damping-energy.out")
    assert len(lines) == d["nen"] and "#Energy" in head and "#zz" in head
    got = np.array([numbers(l) for l in lines])
    assert got.shape == (d["nen"], 10)
    f = facs[-1]                                                       # the last pair's factor, as the reference's code uses it
    tol = HALF_UNIT + TOL * abs(f) * sum(np.abs(r).max() for r in rows)
    assert np.abs(got[:, 0] - (d["ene"] - d["fermi"])).max() <= HALF_UNIT + 1e-15
    dev = np.abs(got[:, 1:] - (f * total).T).max()
    print("damping-energy.out: worst deviation %.2e (bound %.2e), largest value %.3e" % (dev, tol, np.abs(f * total).max()))
    assert dev <= tol


def aux_values(log):
    """Every number calculate_jij_auxgreen prints: the 9 tensor components (3F14.9) and Dij_zz_aux, or J0_aux, per pair."""
    out, lines = [], log.splitlines()
    for k, line in enumerate(lines):
        if "Jij_aux tensor between pair" in line:
            out += [x for l in lines[k + 1:k + 4] for x in numbers(l)]
        elif "Dij_zz_aux between pair" in line or "J0_aux is" in line:
            out.append(fortran_float(line.split()[-1]))
    return out


def test_jij_auxgreen_matches_the_plain_type(tmp_path):
    """An inherited reader of green%gij / gji on the exchange_gpu object: fetch_intersite makes the arrays exist first.  Its output is
    that of the reference's own type(exchange) in the same driver, where the host intersite stage fills them."""
    if not program_built(DRIVER):
        return
    gpu = run("auxgreen", tmp_path / "gpu")
    plain = run("auxgreen_plain", tmp_path / "plain")
    assert "fetch-intersite" in gpu and "fetch-intersite" not in plain
    assert "host_intersite_allocated=T" in gpu and "host_intersite_allocated=T" in plain
    a, b = aux_values(gpu), aux_values(plain)
    print("gpu  ", a)
    print("plain", b)
    assert len(a) == len(b) == 2 * 10 and np.isfinite(a).all() and np.abs(a).max() > 0
    # same host routine on the same coefficients: the same printed digits (the list-directed Dij_zz_aux line carries every digit)
    assert a == b
