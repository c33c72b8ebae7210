"""The region planner of the host library (rslmtoasa_amd/csrc/region_plan.hpp) without a GPU: every list the kernels walk, the `cum` tables,
the level statistics that size the grids and steer the forms of the H|psi> launch, and the counters of rsrec_get_timing, held EXACTLY to a
restatement of the rule in plain numpy -- and, for where the lists lie inside a row, to the arrays the planner produced before it was
restructured (tests/golden/region_plan.npz).

Every case writes a problem file, runs build/region_plan_dump_san (region_plan_dump.cpp: its own main, built with ASan + UBSan) on it as a
stand-alone program and requires exit status 0 with nothing on stderr.
"""
import os
import subprocess

import numpy as np
import pytest

import piece_lattices as PL
from helpers import GOLD, random_problem, supercell_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "build", "region_plan_dump_san")
GROUP = 8


def run_dump(*args):
    r = subprocess.run([DUMP] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return r.stdout


def tables_from(nn):
    """nn(kk, nncols) of the reference (1-based, column 0 the count, 0 = absent) as rsrec_set_lattice converts it: nbr[kk][nslots] 0-based,
    -1 absent, slot 0 the atom itself."""
    nn = np.asarray(nn)
    kk, nslots = nn.shape[0], max(1, int(nn[:, 0].max()))
    nbr = np.full((kk, nslots), -1, np.int64)
    nbr[:, 0] = np.arange(kk)
    for i in range(kk):
        for j in range(1, int(nn[i, 0])):
            if nn[i, j]:
                nbr[i, j] = nn[i, j] - 1
    return nbr


def plan(tmp_path, c):
    """Run the planner on case `c`; every output array by name."""
    nbr, kk = c["nbr"], c["nbr"].shape[0]
    seeds = np.asarray(c["seeds"]).reshape(c["nb"], c["nseed"])
    head = [kk, nbr.shape[1], c["nmax"], c["ntype"], c["nb"], c["nseed"], c["nlev"], c["napply"], int(c["two_pass"]), int(c["grouped"]), c["sat_pct"]]
    keymode = 1 if "cr" in c else (0 if "key" in c else 2)
    parts = [head, [keymode], nbr.ravel(), c["iz0"]]
    text = "\n".join(" ".join(str(int(x)) for x in p) for p in parts) + "\n"
    if keymode == 0:
        text += " ".join(str(int(x)) for x in c["key"]) + "\n"
    if keymode == 1:
        text += " ".join(repr(float(x)) for x in np.asarray(c["cr"]).ravel()) + "\n"
    text += " ".join(str(int(x)) for x in seeds.ravel()) + "\n"
    path = tmp_path / "problem.txt"
    path.write_text(text)
    lines = run_dump(path).split("\n")
    out = {}
    for k in range(0, len(lines) - 1, 2):
        name, n = lines[k].split()
        floats = name in ("atom_steps", "block_mults", "level_groups", "mult_hist")
        out[name] = np.array(lines[k + 1].split(), dtype=np.float64 if floats else np.int64)
        assert out[name].size == int(n), name
    return out


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------
def joining_levels(nbr, seeds, nlev):
    """active_region_sizes' rule (rslmtoasa_amd/lattice.py) from a set of seeds: an atom joins when one of its own slots holds an atom already
    inside.  dist[i] = level at which atom i joins, -1: not within levels 0 .. nlev - 1."""
    kk = nbr.shape[0]
    active = np.zeros(kk + 1, bool)                      # index kk (from the -1 entries): never active
    active[np.asarray(seeds)] = True
    dist = np.where(active[:kk], 0, -1)
    for lev in range(1, nlev):
        hit = active[nbr[:, 1:]].any(axis=1) & ~active[:kk]
        dist[hit] = lev
        active[:kk] |= hit
    return dist


def check_plan(c, P):
    """Every condition on the plan P of case c."""
    nbr, iz0, nmax, ntype = c["nbr"], np.asarray(c["iz0"]), c["nmax"], c["ntype"]
    kk, ns = nbr.shape
    nb, nlev, napply, two_pass, grouped = c["nb"], c["nlev"], c["napply"], c["two_pass"], c["grouped"]
    key = P["key"]
    tau = np.where(np.arange(kk) < nmax, np.arange(kk), nmax + iz0)          # operator class
    ntau, nfs = nmax + ntype, ns + 1
    rank = (tau if grouped else np.zeros(kk, np.int64)), key, np.arange(kk)   # the order of every list: (class, key, atom)

    def in_order(atoms):
        atoms = np.asarray(atoms, np.int64)
        return atoms[np.lexsort((rank[2][atoms], rank[1][atoms], rank[0][atoms]))]

    def check_groups(lst, off):
        if not grouped:
            assert (lst >= 0).all()                                          # no padding at all
            return
        assert lst.size % GROUP == 0 and off % GROUP == 0
        g = lst.reshape(-1, GROUP)
        assert (g[:, 0] >= 0).all()                                          # every group starts with an atom
        assert (np.diff((g < 0).astype(int), axis=1) >= 0).all()             # -1 only at the tail
        cls = np.where(g >= 0, tau[np.maximum(g, 0)], tau[g[:, :1]])
        assert (cls == cls[:, :1]).all()                                     # one operator class per group

    def groups_by_class(lst, off):
        """what level_groups counts: grouped, the groups by the class of their first atom; ungrouped lists have no groups -- the counter then
        holds, under class 0, the entries whose offset in the row is a multiple of 8 (nothing reads it on that path)"""
        G = np.zeros(ntau)
        if grouped:
            np.add.at(G, tau[lst[::GROUP]], 1.0)
        else:
            G[0] = np.count_nonzero((off + np.arange(lst.size)) % GROUP == 0)
        return G

    ostride, sat_base = int(P["ostride"][0]), int(P["sat_base"][0])
    order = P["order"].reshape(nb, ostride)
    cnt, off, cnt2, off2 = P["cum"].reshape(4, nb, nlev)
    sat_from = (c["sat_pct"] * kk + 99) // 100
    all_sorted = in_order(np.arange(kk))
    level_max, hop_min, hop_max = np.zeros(nlev, np.int64), np.full(nlev, 2**31 - 1, np.int64), np.zeros(nlev, np.int64)
    level_sat, level_groups = np.zeros(nlev, np.int64), np.zeros((nlev, ntau))
    atom_steps, hist = 0.0, np.zeros((2, ntau, nfs))
    sat_count = None
    for ch in range(nb):
        row = order[ch]
        dist = joining_levels(nbr, np.asarray(c["seeds"]).reshape(nb, -1)[ch], nlev)
        spans = set()
        prev2 = 0
        for L in range(nlev):
            region = np.flatnonzero((dist >= 0) & (dist <= L))
            stalled = L > 0 and not np.any(dist == L)
            assert 0 <= off[ch, L] and off[ch, L] + cnt[ch, L] <= ostride and 0 <= off2[ch, L] and off2[ch, L] + cnt2[ch, L] <= ostride
            lst = row[off[ch, L]:off[ch, L] + cnt[ch, L]]
            if region.size >= sat_from:
                assert off[ch, L] == off2[ch, L] == sat_base and cnt[ch, L] == cnt2[ch, L]
                assert np.array_equal(lst[lst >= 0], all_sorted)             # every atom once, by (class, key, atom)
                sat_count = int(cnt[ch, L])
                level_sat[L] += 1
            else:
                assert np.array_equal(lst[lst >= 0], in_order(region))       # exactly the atoms with dist <= L, each once
                lst2 = row[off2[ch, L]:off2[ch, L] + cnt2[ch, L]]
                assert off2[ch, L] == 0 and np.array_equal(np.sort(lst2[lst2 >= 0]), region)
                shell = row[prev2:cnt2[ch, L]]                               # level-major list: this shell behind the earlier ones
                assert np.array_equal(shell[shell >= 0], in_order(np.flatnonzero(dist == L)))
                check_groups(shell, prev2)
                prev2 = int(cnt2[ch, L])
                if stalled:
                    assert off[ch, L] == off[ch, L - 1] and cnt[ch, L] == cnt[ch, L - 1]
                spans.add((int(off[ch, L]), int(cnt[ch, L])))
            check_groups(lst, int(off[ch, L]))
            if region.size >= sat_from and not grouped:                      # ... and on the list of all atoms every eighth entry under its class
                np.add.at(level_groups[L], tau[lst[::GROUP][:kk // GROUP]], 1.0)
            else:
                level_groups[L] += groups_by_class(lst, int(off[ch, L]))
            level_max[L] = max(level_max[L], cnt[ch, L], cnt2[ch, L])
            hop_min[L], hop_max[L] = min(hop_min[L], cnt[ch, L]), max(hop_max[L], cnt[ch, L])
        # the lists of the chain lie inside its row and do not overlap (a stalled level points at the previous level's list: one span)
        spans = sorted(spans) + [(sat_base, ostride - sat_base)]
        edge = prev2                                                         # the level-major list comes first
        for lo, n in spans:
            assert lo >= edge and lo + n <= ostride
            edge = lo + n
        sat_list = row[sat_base:]
        sat_list = sat_list[:np.flatnonzero(sat_list >= 0)[-1] + 1]
        assert np.array_equal(sat_list[sat_list >= 0], all_sorted)           # the list of all atoms is in every row
        if sat_count is not None:
            assert -(-sat_list.size // GROUP) * GROUP == sat_count if grouped else sat_list.size == sat_count == kk
        # bookkeeping in the reference's terms
        size = [np.count_nonzero((dist >= 0) & (dist <= L)) for L in range(nlev)]
        for t in range(1, napply + 1):
            atom_steps += size[min(2 * t if two_pass else t, nlev - 1)]
            src = np.where(nbr >= 0, dist[np.maximum(nbr, 0)], -1)           # [atom][slot]: joining level of the source
            for p, before in enumerate(((2 * (t - 1), 2 * t - 1) if two_pass else (t - 1,))):
                i, s = np.nonzero((src >= 0) & (src <= before))
                np.add.at(hist[p], (tau[i], s), 1.0)
            if two_pass:                                                     # the on-site term of the second pass
                i = np.flatnonzero((dist >= 0) & (dist <= 2 * (t - 1)))
                np.add.at(hist[1], (tau[i], ns), 1.0)
    assert np.array_equal(P["level_max"], level_max)
    assert np.array_equal(P["hop_min"], hop_min) and np.array_equal(P["hop_max"], hop_max)
    assert np.array_equal(P["level_sat"], level_sat)
    assert np.array_equal(P["level_groups"].reshape(nlev, ntau), level_groups)
    runs = []
    if grouped:                                                              # maximal class runs of the list of all atoms, in groups
        heads = tau[[a for a in order[0, sat_base:][::GROUP] if a >= 0]]
        for g, t in enumerate(heads):
            if runs and runs[-1][0] == t:
                runs[-1][2] = g + 1
            else:
                runs.append([int(t), g, g + 1])
    assert np.array_equal(P["sat_runs"].reshape(-1, 3), np.array(runs, np.int64).reshape(-1, 3))
    assert P["atom_steps"][0] == atom_steps
    assert np.array_equal(P["mult_hist"].reshape(2, ntau, nfs), hist)
    assert P["block_mults"][0] == hist.sum() + hist[1, :, ns].sum()          # the reference multiplies enim and lsham separately


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def case(nn, iz, seeds, nseed=1, nlev=None, napply=None, two_pass=False, grouped=True, sat_pct=100, nmax=0, ntype=None, key=None):
    seeds = np.asarray(seeds, np.int64).reshape(-1, nseed) - 1
    if napply is None:
        napply = (nlev - 1) // (2 if two_pass else 1)
    c = dict(nbr=tables_from(nn), iz0=np.asarray(iz, np.int64) - 1, seeds=seeds, nb=seeds.shape[0], nseed=nseed, nlev=nlev, napply=napply,
             two_pass=two_pass, grouped=grouped, sat_pct=sat_pct, nmax=nmax, ntype=int(ntype or np.max(iz)))
    if key is not None:
        c["key"] = key
    return c


def ring(n):
    nn = np.zeros((n, 4), np.int32)
    nn[:, 0] = 3
    nn[:, 1] = (np.arange(n) + 1) % n + 1
    nn[:, 2] = (np.arange(n) - 1) % n + 1
    return nn


def build_cases():
    C = {}
    sc = supercell_problem((4, 4, 8))["nn"]
    kk = sc.shape[0]
    one = np.ones(kk, np.int64)
    C["sc448"] = case(sc, one, [1, 77, 128], nlev=12)                                     # keys from the neighbour graph, as without positions
    two = 1 + (np.arange(kk) // 5) % 2
    C["sc448_classes"] = case(sc, two, [1, 77, 128], nlev=12, nmax=3)
    C["sc448_two_pass"] = case(sc, two, [1, 77], nlev=11, two_pass=True, nmax=3)
    C["sc448_ungrouped"] = case(sc, two, [1, 77, 128], nlev=12, grouped=False, nmax=3)
    C["sc448_pair"] = case(sc, two, [1, 77, 5, 9, 128, 128], nseed=2, nlev=9, nmax=3)
    for grouped in (True, False):
        C["whole_lattice_%d" % grouped] = case(sc, two, np.arange(1, kk + 1), nseed=kk, nlev=1, napply=1, grouped=grouped, nmax=3)
    tp = PL.two_piece_problem()
    for pct in (40, 77, 80, 100):
        C["two_piece_%d" % pct] = case(tp["nn"], tp["iz"], PL.two_piece_seeds(), nlev=PL.TWO_PIECE_LLD + 2, sat_pct=pct)
    rng = np.random.default_rng(9001)
    rp = random_problem(rng, 90, 7, 3, 9, False, True)
    keys = rng.integers(0, 30, 90)                                                        # many ties: the atom number decides
    C["ragged"] = case(rp["nn"], rp["iz"], [1, 45, 90], nlev=8, nmax=9, ntype=3, key=keys)
    C["ragged_ungrouped_sat80"] = case(rp["nn"], rp["iz"], [1, 45, 90], nlev=8, nmax=9, ntype=3, key=keys, grouped=False, sat_pct=80)
    C["ragged_two_pass_sat80"] = case(rp["nn"], rp["iz"], [2, 60], nlev=9, two_pass=True, nmax=9, ntype=3, key=keys, sat_pct=80)
    # a ring of 17 atoms, diameter 8, at 14 levels: alone it ends on the list of all atoms; beside a second ring of 5 its region stops growing
    # short of the lattice, and the levels behind stall
    C["ring17"] = case(ring(17), np.ones(17, np.int64), [1, 9], nlev=14)
    rings = np.concatenate([ring(17), np.where(ring(5) > 0, ring(5) + [[0, 17, 17, 0]], 0)])
    C["ring17_and_5"] = case(rings, np.ones(22, np.int64), [1, 9, 20], nlev=14)
    return C


CASES = build_cases()


def coverage(c):
    """(chain, level) pairs of case c on the list of all atoms, stalled below it, and with a class border inside a grouped list of their own."""
    kk = c["nbr"].shape[0]
    tau = np.where(np.arange(kk) < c["nmax"], np.arange(kk), c["nmax"] + c["iz0"])
    sat = stalled = border = 0
    for seeds in c["seeds"]:
        dist = joining_levels(c["nbr"], seeds, c["nlev"])
        for L in range(c["nlev"]):
            region = np.flatnonzero((dist >= 0) & (dist <= L))
            if region.size >= (c["sat_pct"] * kk + 99) // 100:
                sat += 1
                continue
            stalled += int(L > 0 and not np.any(dist == L))
            border += int(c["grouped"] and np.unique(tau[region]).size > 1)
    return sat, stalled, border


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLD, "region_plan.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_holds_the_rule_and_the_recorded_lists(name, tmp_path, golden):
    c = CASES[name]
    P = plan(tmp_path, c)
    check_plan(c, P)
    for field in ("order", "cum", "ostride", "sat_base"):                                 # where the lists lie in the row: the recorded plan
        assert np.array_equal(P[field], golden[name + "_" + field]), field


def test_the_table_reaches_every_branch():
    cover = {name: coverage(c) for name, c in CASES.items()}
    for k, what in enumerate(("on the list of all atoms", "stalled", "class border")):
        assert sum(cv[k] for cv in cover.values()) > 0, what
    # the two pieces: the larger one holds 200 of 260 atoms, 76.9 % -- its chains saturate at 40 and are one atom short at 77
    assert cover["two_piece_40"][0] > 0 and cover["two_piece_77"][0] == cover["two_piece_80"][0] == cover["two_piece_100"][0] == 0
    assert cover["ring17"][1] == 0 and cover["ring17_and_5"][1] == 2 * 5 + 11 and cover["sc448"][0] > 0 and cover["ragged"][2] > 0


def test_keys_from_positions_are_morton_codes(tmp_path):
    """2 x 2 x 2 corners of a box of sides (2, 1, 0.5): the largest span (2) scales every axis; q = floor((x - lo) / span * 1023) per axis, and the
    key interleaves the bits of (qx, qy, qz), x lowest."""
    cr = np.array([[x, y, z] for z in (0.0, 0.5) for y in (3.0, 4.0) for x in (-1.0, 1.0)])
    nn = np.zeros((8, 2), np.int32)
    nn[:, 0] = 1
    c = case(nn, np.ones(8, np.int64), [1], nlev=1, napply=1)
    c["cr"] = cr
    # q per axis: x in {0, 1023}, y in {0, 511}, z in {0, 255}
    sx, sy, sz = 0o1111111111, 0o0111111111 << 1, 0o0011111111 << 2                       # every third bit: 10, 9 and 8 of them
    want = [bx * sx + by * sy + bz * sz for bz in (0, 1) for by in (0, 1) for bx in (0, 1)]
    assert want[1] == 0x09249249 and want[2] == 0x02492492 and want[4] == 0x00924924
    assert plan(tmp_path, c)["key"].tolist() == want


def test_region_keys_compare_field_by_field():
    base = [3, 1, 12, 11, 0, 1, 100]

    def match(a, b):
        return run_dump("--match", ",".join(map(str, a)), ",".join(map(str, b))).strip() == "1"

    assert match(base, base)
    for field, value in enumerate([4, 2, 13, 10, 1, 0, 80]):
        other = list(base)
        other[field] = value
        assert not match(base, other), field
    # nseed = 4 194 304 is where a key packed as nseed << 9 wrapped to a negative int: just another value
    big = [1, 4194304, 1, 1, 0, 1, 100]
    assert match(big, big)
    assert not match(big, [1, 4194305, 1, 1, 0, 1, 100]) and not match(big, [1, 0, 1, 1, 0, 1, 100])
    assert not match(big, [1, 4194304, 1, 1, 0, 1, 80])
