"""Device time of the pair moments: four chains per pair (chebyshev_recur_ij) against one chain per atom
(rsrec_chebyshev_pairs_direct, both modes), in ONE process on one handle per cell.

    python tools/time_pair_direct.py [--lld 50] [--rounds 3] [--cells 4x4x8 22x22x22] [--stars 1 8 32 136] [--disjoint 32]
                                     [--out profiles/pair_direct_v1.json]

Pair lists: a star of P pairs (1, j) around atom 1, j running through the atoms nearest to atom 1 in the neighbour graph (a J_ij map;
capped at the cell's other atoms), and `--disjoint` pairs that share no atom.  Per list and route: device ms (rsrec_get_timing out[0])
and H|psi> launches (out[2]) of `--rounds` rounds, the routes alternating inside a round, after one warm-up call each; reported as
min-max.  Chain applications per call: 4 P (lld + 1) for the four-chain route, (2 lld + 1) times the distinct first atoms (mode 1) or the
distinct atoms (mode both) for the direct one.  One JSON line per row on stdout; the whole table goes to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def nearest_atoms(nn, start, n):
    """The n atoms nearest to `start` (1-based) in the neighbour graph, breadth first, ascending inside a shell; `start` itself left out."""
    seen, order, frontier = {start}, [], [start]
    while frontier and len(order) < n:
        nxt = sorted({int(j) for i in frontier for j in nn[i - 1, 1:int(nn[i - 1, 0])] if j and int(j) not in seen})
        seen.update(nxt)
        order += nxt
        frontier = nxt
    return order[:n]


def main():
    from helpers import objects_from, supercell_problem
    from rslmtoasa_amd.recursion import Recursion
    ap = argparse.ArgumentParser()
    ap.add_argument("--lld", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", nargs="+", default=["4x4x8", "22x22x22"])
    ap.add_argument("--stars", type=int, nargs="+", default=[1, 8, 32, 136])
    ap.add_argument("--disjoint", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_direct_v1.json"))
    args = ap.parse_args()
    rows = []
    for cell in args.cells:
        dims = tuple(int(v) for v in cell.split("x"))
        p = supercell_problem(dims)
        kk = p["nn"].shape[0]
        ham, lat, ctl, en = objects_from(p, [1], args.lld, emin=-3.0, emax=1.8)
        lists = []
        for n in args.stars:
            js = nearest_atoms(p["nn"], 1, min(n, kk - 1))
            lists.append(("star", np.array([(1, j) for j in js], np.int32)))
        nd = min(args.disjoint, kk // 2)
        atoms = np.linspace(1, kk, 2 * nd).astype(np.int64)
        assert len(set(atoms.tolist())) == 2 * nd
        lists.append(("disjoint", atoms.reshape(nd, 2).astype(np.int32)))
        lat.ijpair = lists[0][1]
        rec = Recursion(ham, lat, ctl, en)
        routes = {"four_chain": lambda: rec.chebyshev_recur_ij(), "direct_1": lambda: rec.chebyshev_recur_ij_direct(False),
                  "direct_both": lambda: rec.chebyshev_recur_ij_direct(True)}
        for shape, pairs in lists:
            rec.lattice.ijpair = pairs
            rec.restore_to_default()
            npairs = len(pairs)
            apps = {"four_chain": 4 * npairs * (args.lld + 1), "direct_1": (2 * args.lld + 1) * len(set(pairs[:, 0].tolist())),
                    "direct_both": (2 * args.lld + 1) * len(set(pairs.ravel().tolist()))}
            ms = {k: [] for k in routes}
            launches = {k: [] for k in routes}
            for fn in routes.values():
                fn()                                             # warm-up: buffers, region lists, code objects
            for _ in range(args.rounds):
                for k, fn in routes.items():
                    fn()
                    t = rec.timing()
                    ms[k].append(t["total_ms"])
                    launches[k].append(int(t["hop_launches"]))
            row = dict(cell=cell, atoms=kk, lld=args.lld, pairs=shape, npairs=npairs, rounds=args.rounds)
            for k in routes:
                row[k] = dict(device_ms_min=min(ms[k]), device_ms_max=max(ms[k]), spmm_launches=sorted(set(launches[k])), chain_applications=apps[k])
            for k in ("direct_1", "direct_both"):
                row["four_chain_over_" + k] = [min(ms["four_chain"]) / max(ms[k]), max(ms["four_chain"]) / min(ms[k])]
            rows.append(row)
            print(json.dumps(row), flush=True)
        rec.close()
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/time_pair_direct.py", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
