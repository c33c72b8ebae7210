"""The exchange post-processing (`post_processing = 'exchange'`, calculation.f90:816-950) through the zero-edit drop-in
oracle/_ref/rslmto_dropin.x, whose type(exchange) is fortran/exchange_gpu.f90: green's intersite arrays are never allocated and
Jij / Dij / Iij come from rsrec_exchange on the chains the pair recursion left on the device.

Cases (tests/golden/exchange_dropin/manifest.json): the reference's own examples Example_exchange_bccFe and _hoh (block, lld 20,
nsp 2), with its committed expected values; a Chebyshev variant of the same input; and a many-pair variant, atom 1 against the 136
atoms of its first nine neighbour shells and against itself (the i == j pair: one resident chain).

The comparison rule against ref.json is the reference's (tests/run_test.py): a value fails only if both the absolute and the relative
difference exceed the tolerance (a NaN in ref.json -- the _hoh case's dij.out -- passes whatever is printed).  A plain host run of the
reference is no yardstick for the Simpson-integrated files: simpson_f reads one element past its arrays."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import program_built
from oracle.make_fixtures import patch_namelist
from rslmtoasa_amd._proc import run_with_unlimited_stack
from test_fortran_dropin import DROPIN, ROOT, close, fortran_float

pytestmark = pytest.mark.gpu
CASES_DIR = os.path.join(ROOT, "tests", "golden", "exchange_dropin")
MANIFEST = json.load(open(os.path.join(CASES_DIR, "manifest.json")))
NEN = 2510                      # channels_ldos + 10
FIXTURES = ["Example_exchange_bccFe", "Example_exchange_bccFe_hoh", "Generated_exchange_bccFe_chebyshev"]     # cases with a reference fixture (tools/exchange_case_fixture)
# the eleven files of calculate_exchange_twoindex and the four of calculate_exchange (jtens*.out are opened and left empty)
TWOINDEX = ["jijso.out", "jijfo.out", "dijso.out", "dijfo.out", "aijso.out", "aijfo.out", "jijparts.out", "dijparts.out", "aijparts.out"]
EMPTY = ["jtens.out", "jtensso.out", "jtensfo.out"]
# ru_maxrss of the drop-in, read in a fresh Python child per run (RUSAGE_CHILDREN of that child = the program alone)
RSS_CHILD = r"""
import json, resource, sys
sys.path.insert(0, sys.argv[1])
from rslmtoasa_amd._proc import run_with_unlimited_stack
r = run_with_unlimited_stack([sys.argv[2]], cwd=sys.argv[3], env={"OMP_NUM_THREADS": "8", "RSREC_REPORT": "1"}, timeout=1200, scrub=False)
open(sys.argv[3] + "/run.log", "w").write(r.stdout + r.stderr)
print(json.dumps({"rc": r.returncode, "maxrss_kb": resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss}))
"""


def prepare(name, work):
    case = MANIFEST[name]
    shutil.copytree(os.path.join(CASES_DIR, case["inputs"]), work, copy_function=shutil.copyfile)
    inp = work / "input.nml"
    inp.write_text(patch_namelist(inp.read_text(), case["patch"]))


def check_log(log):
    assert "fatal" not in log.lower(), log[-3000:]
    assert "exchange-gpu" in log, log[-3000:]                    # the exchange stage ran on the device (g_timer label of exchange_gpu)
    m = re.search(r"rsrec report: library_calls=(\d+)", log)
    # exactly the seeded pair recursion and rsrec_exchange (the host intersite stage would add a terminator and Green call per pair)
    assert m and int(m.group(1)) == 2, log[-2000:]


def run_case(name, work):
    prepare(name, work)
    r = run_with_unlimited_stack([DROPIN], cwd=work, env={"OMP_NUM_THREADS": "8", "RSREC_REPORT": "1"}, timeout=1200, scrub=False)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    check_log(log)
    return log


def run_case_rss(name, work):
    """The case in a fresh child; (log, peak RSS of the program in kB)."""
    prepare(name, work)
    r = subprocess.run([sys.executable, "-c", RSS_CHILD, ROOT, DROPIN, str(work)], capture_output=True, text=True, timeout=1300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    log = (work / "run.log").read_text()
    assert res["rc"] == 0, log[-3000:]
    check_log(log)
    return log, res["maxrss_kb"]


def table(path):
    return [[fortran_float(t) for t in line.split()] for line in path.read_text().splitlines() if line.strip()]


def stdout_pairs(log):
    """Full-precision J and D per pair from the rank-0 stdout lines of calculate_exchange (list-directed: every digit)."""
    num = r"([-+0-9.EeDd]+)"
    jij = [(int(a), int(b), float(v)) for a, b, v in re.findall(r"Jij between pair\s+(\d+)\s+and\s+(\d+)\s+is\s+" + num, log)]
    dij = [(int(a), int(b), tuple(float(x) for x in (u, v, w)))
           for a, b, u, v, w in re.findall(r"Dij between pair\s+(\d+)\s+and\s+(\d+)\s+is\s+" + num + r"\s+" + num + r"\s+" + num, log)]
    return jij, dij


def load_fixture(name):
    with np.load(os.path.join(CASES_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def half_unit(tok):
    """Half a unit in the last printed digit of a Fortran field (f12.6, es16.6, e20.11)."""
    t = tok.replace("D", "E").replace("d", "e")
    m = re.fullmatch(r"[-+]?(\d*)\.(\d*)(?:[eE]?([-+]\d+))?", t)
    return 0.5 * 10.0 ** (int(m.group(3) or 0) - len(m.group(2)))


def compare_with_fixture(work, z, npairs):
    """Every number the two routines print, against the reference's full-precision values of the case fixture
    (tools/exchange_case_fixture): half a unit in the last printed digit + 1e-9 relative, with an absolute floor of 1e-12 of the
    case's largest |J| for the values that vanish by symmetry (roundoff residuals of terms of J's size, which the drop-in's own
    chains reproduce only to that level).  The second-order rows: against the reference's printed digits."""
    floor = 1e-12 * np.abs(z["xc"][0]).max()
    cols = {"jij.out": (z["xc"][0:1], 5), "dij.out": (z["xc"][1:4], 5), "aij.out": (z["xc"][4:13], 5),
            "jijfo.out": (z["fo"][0:1], 5), "dijfo.out": (z["fo"][1:4], 5), "aijfo.out": (z["fo"][4:13], 5),
            "jijparts.out": (z["parts"][0:4], 5), "dijparts.out": (z["parts"][4:10], 5), "aijparts.out": (z["parts"][10:28], 5),
            "jijso.out": (z["so_printed"][0:1], 5), "dijso.out": (z["so_printed"][1:4], 5), "aijso.out": (z["so_printed"][4:13], 5)}
    bad = []
    for fn, (ref, c0) in cols.items():
        lines = [l.split() for l in (work / fn).read_text().splitlines() if l.strip()]
        assert len(lines) == npairs, fn
        for p, toks in enumerate(lines):
            for k in range(ref.shape[0]):
                tok = toks[c0 + k]
                got, exp = fortran_float(tok), ref[k, p]
                tol = half_unit(tok) * (2 if fn.endswith("so.out") else 1) + 1e-9 * abs(exp) + floor
                if not abs(got - exp) <= tol:
                    bad.append((fn, p, k, got, exp))
    assert not bad, bad[:10]
    f150 = np.array(table(work / "fort.150"))
    for k, p in enumerate(z["f150_pairs"]):
        got = f150[p * NEN:(p + 1) * NEN]
        ref = z["fort150"][:, :, k]
        assert np.abs(got[:, 0] - ref[:, 0]).max() <= 1e-14
        assert np.abs(got[:, 1] - ref[:, 1]).max() <= 1e-9 * np.abs(ref[:, 1]).max(), (p, np.abs(got[:, 1] - ref[:, 1]).max())


def check_files(work, npairs):
    """Every file of both routines, with a row per pair (fort.150: a line per pair and energy), all finite."""
    for fn in ["jij.out", "dij.out", "aij.out"] + TWOINDEX:
        rows = table(work / fn)
        assert len(rows) == npairs, fn
        assert np.isfinite(np.array(rows)).all() or fn.startswith("dij") or fn.startswith("aij"), fn
    for fn in EMPTY:
        assert (work / fn).exists() and (work / fn).read_text().strip() == "", fn
    f150 = np.array(table(work / "fort.150"))
    assert f150.shape == (NEN * npairs, 2), f150.shape
    assert np.isfinite(f150).all()
    return f150


@pytest.mark.parametrize("name", ["Example_exchange_bccFe", "Example_exchange_bccFe_hoh", "Generated_exchange_bccFe_chebyshev"])
def test_exchange_case_through_drop_in(name, tmp_path):
    if not program_built(DROPIN):       # (warns: the program holds reference object code, test_fortran_dropin.py)
        return
    work = tmp_path / "run"
    log = run_case(name, work)
    f150 = check_files(work, 2)
    # fort.150: ene(nv) - fermi and the cumulative second-order J, per pair; at the mesh point on the Fermi level it is close to
    # jijso.out (not equal: simpson_f integrates to fermi itself there, a few 1e-5 apart)
    so = table(work / "jijso.out")
    for p in range(2):
        e, jc = f150[p * NEN:(p + 1) * NEN].T
        k = int(np.argmin(np.abs(e)))
        assert abs(e[k]) < 1e-5 and abs(jc[k] - so[p][5]) <= 1e-3 * abs(so[p][5]) + 1e-6, (p, e[k], jc[k], so[p][5])
    jij, dij = stdout_pairs(log)
    assert [(a, b) for a, b, _ in jij] == [(1, 2634), (1, 2635)]
    # jij.out's J is the stdout J rounded to f12.6
    for row, (_, _, v) in zip(table(work / "jij.out"), jij):
        assert abs(row[5] - v) <= 5e-7 + 1e-12, (row, v)
    case = MANIFEST[name]
    bad = []
    for fn, rows in case["expected"].get("text", {}).items():
        lines = (work / fn).read_text().splitlines()
        for row, cols in rows.items():
            vals = lines[int(row) - 1].split()
            for col, e in cols.items():
                got = fortran_float(vals[int(col) - 1])
                if not np.isnan(e) and not close(got, e, case["abs_tol"], case["rel_tol"]):
                    bad.append((fn, row, col, got, e))
    assert not bad, bad
    if name in FIXTURES:
        compare_with_fixture(work, load_fixture(name), 2)
    print(name, "J:", [v for _, _, v in jij], "D:", [v for _, _, v in dij])


def test_exchange_many_pairs_memory_and_symmetry(tmp_path):
    """atom 1 against 136 neighbours and itself: the peak RSS does not grow with the pairs (the reference's intersite arrays would
    add about 0.1 GB per pair; measured rise 0.29 GB), the pairs of one neighbour shell agree, and the two pairs shared with the 2-pair
    case give the same rows."""
    if not program_built(DROPIN):
        return
    log2, rss2 = run_case_rss("Example_exchange_bccFe", tmp_path / "two")
    logn, rssn = run_case_rss("Generated_exchange_bccFe_pairs", tmp_path / "many")
    npairs = 137
    check_files(tmp_path / "many", npairs)
    rise_gb = (rssn - rss2) / 1024.0 ** 2
    print("peak RSS: 2 pairs %.3f GB, %d pairs %.3f GB (rise %.3f GB)" % (rss2 / 1024.0 ** 2, npairs, rssn / 1024.0 ** 2, rise_gb))
    assert rise_gb < 1.0, rise_gb
    for line in logn.splitlines():
        if "exchange-gpu" in line:
            print(line)

    # the pairs the two runs share: the printed J / D / I rows are the same text, and the full-precision J agrees to 1e-12.  Not bit for
    # bit: the recursion picks its SpMM kernel by launch size (8 chains vs 545), so the chains differ in the last bits, and D, which
    # vanishes by symmetry, is a roundoff residual of ~1e-8 whose last printed digits move (dijso.out: 7.302979E-09 vs 7.302981E-09)
    for fn in ["jij.out", "dij.out", "aij.out"]:
        a = (tmp_path / "two" / fn).read_text().splitlines()
        b = (tmp_path / "many" / fn).read_text().splitlines()
        assert a == b[:2], fn
    j2, d2 = stdout_pairs(log2)
    jn, dn = stdout_pairs(logn)
    for (a, b, v), (a2, b2, w) in zip(j2, jn[:2]):
        assert (a, b) == (a2, b2) and abs(v - w) <= 1e-12 * abs(v), (v, w)
    for (_, _, v), (_, _, w) in zip(d2, dn[:2]):
        assert max(abs(x - y) for x, y in zip(v, w)) <= 1e-12, (v, w)
    for fn in TWOINDEX:
        a = np.array(table(tmp_path / "two" / fn))
        b = np.array(table(tmp_path / "many" / fn))[:2]
        assert np.all(np.abs(a - b) <= 2e-6 * np.abs(a) + 1e-12), fn
    f2 = np.array(table(tmp_path / "two" / "fort.150"))
    fm = np.array(table(tmp_path / "many" / "fort.150"))[:2 * NEN]
    assert np.all(np.abs(f2 - fm) <= 1e-9 * np.abs(f2).max()), np.abs(f2 - fm).max()

    # classes of equivalent pairs.  The moment lies along z and the Hamiltonian carries spin-orbit coupling, so only the operations of
    # the cubic group that keep the z axis (x <-> y, sign changes) map a pair onto an equivalent one: a class is (|dz|, {|dx|, |dy|}).
    # Pairs of one neighbour shell but of different classes really differ (a first run: 9e-4 relative in the second shell, 6e-2 in
    # the eighth, where J is small).  Within a class the spread is not roundoff either: the cluster this input builds (5984 atoms,
    # radius 8.9 alat) is not symmetric about atom 1 -- one surface atom, at (-2.5, 5.5, 6.5), has no mirror image -- and chains of
    # depth 20 reach the surface.  A run on MI355X gave up to 3.5e-4 relative (classes of small J) and |D| up to 6.4e-6 mRy, so the
    # 1e-8 one might expect does not hold; the bounds are that run's, times 10.
    assert len(jn) == npairs and jn[-1][:2] == (1, 1)
    rows = np.array(table(tmp_path / "many" / "jij.out"))[:-1]
    J = np.array([v for _, _, v in jn])[:-1]
    D = np.array([v for _, _, v in dn])[:-1]
    keys = [(round(abs(r[4]), 5), tuple(sorted((round(abs(r[2]), 5), round(abs(r[3]), 5))))) for r in rows]
    classes = {}
    for k, key in enumerate(keys):
        classes.setdefault(key, []).append(k)
    assert sum(len(v) for v in classes.values()) == 136 and len(classes) >= 9
    worst_j = worst_d = 0.0
    for key, idx in sorted(classes.items(), key=lambda kv: sum(x * x for x in (kv[0][0],) + kv[0][1])):
        spread = (J[idx].max() - J[idx].min()) / np.abs(J[idx]).max()
        dmax = np.abs(D[idx]).max()
        worst_j, worst_d = max(worst_j, spread), max(worst_d, dmax)
        print("class |dz| %.2f {|dx|,|dy|} %s: %2d pairs  J %.9f  spread %.2e  max|D| %.2e" % (key[0], key[1], len(idx), J[idx].mean(), spread, dmax))
    print("worst J spread %.2e, worst |D| %.2e" % (worst_j, worst_d))
    assert worst_j <= 4e-3 and worst_d <= 1e-4, (worst_j, worst_d)
