"""Device time of the k-resolved moments (rsrec_chebyshev_bloch) against the bare chain and against the route without it, in ONE
process on one handle per cell.

    python tools/time_bloch.py [--lld 50] [--rounds 3] [--cells 22x22x22 46x46x46] [--nk 16 64 256] [--out profiles/bloch_v1.json]

Per cell and nk, one source, one group: `--rounds` rounds after one warm-up call each, the routes alternating inside a round, reported
as min-max.
  bloch : rsrec_chebyshev_bloch without a download.  rsrec_get_timing out[0] (device ms), out[1] (ms in the H|psi> launches), out[5] (ms
          in the phase table and the Bloch passes).  The passes' matrix flops are 2592 nk sum_n N_act(n) (N_act(n): atoms of the chain's
          region at order n), quoted over out[5] as a share of the 78.6 TF FP64 matrix peak; the vector bytes they must read are
          5184 sum_n N_act(n) per 32 k-points (a wave keeps 64 rows of W per pass over the vector), quoted over out[5] as well.
  bare  : rsrec_chebyshev_pairs_direct with the one pair (source, source): the same chain with one gathered block per order.
On the 4x4x8 cell also the route without the call: a pairs_direct star of all 127 other atoms (plus the atom itself) and the phase sum
in numpy, wall time with the host's share, against the wall time of the Bloch call with its download.
One JSON line per row on stdout; the whole table goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TF = 78.6


def spread(v):
    return [min(v), max(v)]


def main():
    from bloch_reference import commensurate_k, supercell_cell
    from helpers import objects_from, supercell_problem
    from rslmtoasa_amd.lattice import active_region_sizes, supercell_positions
    from rslmtoasa_amd.recursion import Recursion
    ap = argparse.ArgumentParser()
    ap.add_argument("--lld", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", nargs="+", default=["22x22x22", "46x46x46"])
    ap.add_argument("--nk", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloch_v1.json"))
    args = ap.parse_args()
    rows = []
    rng = np.random.default_rng(1)
    for cell in args.cells + ["4x4x8"]:
        dims = tuple(int(v) for v in cell.split("x"))
        p = supercell_problem(dims)
        kk = p["nn"].shape[0]
        ham, lat, ctl, en = objects_from(p, [1], args.lld, emin=-3.0, emax=1.8)
        src = kk // 2 + 1
        star = np.array([(src, j) for j in range(1, kk + 1)], np.int32)
        lat.ijpair = star if cell == "4x4x8" else np.array([(src, src)], np.int32)      # (sizes the moment array of the pair calls)
        cr, cvec = supercell_positions(dims), supercell_cell(dims)
        rec = Recursion(ham, lat, ctl, en)
        napply = 2 * args.lld + 1
        nact = float(1 + sum(active_region_sizes(p["nn"], src, napply)))         # sum over the orders 0 .. 2 lld + 1
        if cell == "4x4x8":                                      # the route without the call, wall time
            k = commensurate_k(dims, rng.integers(0, 8, (64, 3)))

            def today():
                m_pair = rec.chebyshev_recur_ij_direct(False)
                w = np.exp(-1j * (k.T @ (cr - cr[:, src - 1:src])))
                return np.einsum("qj,abnj->abnq", w, m_pair[:, :, :, 1, :])

            def bloch():
                return rec.chebyshev_bloch([src], k, cr, cell=cvec)[..., 0, 0]
            a, b = today(), bloch()
            dev = float(np.abs(a - b).max() / np.abs(a).max())
            wall = {"star_and_numpy": [], "bloch": []}
            for _ in range(args.rounds):
                for name, fn in (("star_and_numpy", today), ("bloch", bloch)):
                    t0 = time.perf_counter()
                    fn()
                    wall[name].append(1e3 * (time.perf_counter() - t0))
            row = dict(cell=cell, atoms=kk, lld=args.lld, nk=64, rounds=args.rounds, deviation=dev,
                       wall_ms={n: spread(v) for n, v in wall.items()})
            rows.append(row)
            print(json.dumps(row), flush=True)
            rec.close()
            continue
        for nk in args.nk:
            k = commensurate_k(dims, rng.integers(0, dims[0], (nk, 3)))
            routes = {"bloch": lambda: rec.chebyshev_bloch([src], k, cr, cell=cvec, download=False),
                      "bare": lambda: rec.chebyshev_recur_ij_direct(False)}
            t = {n: {"total_ms": [], "hop_ms": [], "rest_ms": []} for n in routes}
            for fn in routes.values():
                fn()                                             # warm-up: buffers, region lists, code objects
            for _ in range(args.rounds):
                for n, fn in routes.items():
                    fn()
                    tm = rec.timing()
                    for key in t[n]:
                        t[n][key].append(tm[key])
            flop, vbytes = 2592.0 * nk * nact, 5184.0 * nact * ((2 * nk + 63) // 64)
            pass_ms = t["bloch"]["rest_ms"]
            row = dict(cell=cell, atoms=kk, lld=args.lld, nk=nk, rounds=args.rounds, sum_n_act=nact,
                       bloch=dict(device_ms=spread(t["bloch"]["total_ms"]), hop_ms=spread(t["bloch"]["hop_ms"]), pass_ms=spread(pass_ms),
                                  pass_tflops=spread([flop / (1e9 * m) for m in pass_ms]),
                                  pass_share_of_peak=spread([flop / (1e9 * m) / PEAK_TF for m in pass_ms]),
                                  pass_vector_tb_per_s=spread([vbytes / (1e9 * m) for m in pass_ms])),
                       bare=dict(device_ms=spread(t["bare"]["total_ms"]), hop_ms=spread(t["bare"]["hop_ms"])),
                       pass_over_hop=spread([m / h for m, h in zip(pass_ms, t["bloch"]["hop_ms"])]),
                       bloch_over_bare=[min(t["bloch"]["total_ms"]) / max(t["bare"]["total_ms"]), max(t["bloch"]["total_ms"]) / min(t["bare"]["total_ms"])])
            rows.append(row)
            print(json.dumps(row), flush=True)
        rec.close()
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/time_bloch.py", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
