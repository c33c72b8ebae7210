"""Device time of constant-energy maps (rsrec_chebyshev_bloch_map) against the route through the moments, in ONE process on one handle per cell.

    python tools/time_bloch_map.py [--lld 50] [--rounds 3] [--cells 22x22x22 46x46x46] [--nk 256 4096 65536] [--ne 1 4 8]
                                   [--baseline-nk-max 65536] [--out profiles/bloch_map_v1.json]

Per cell, nk (a commensurate plane of sqrt(nk) x sqrt(nk) points) and ne, one source, one group: `--rounds` rounds after one warm-up call
each, the routes alternating inside a round, device ms reported as min-max.
  map      : rsrec_chebyshev_bloch_map, a_k alone into a device array (nothing is downloaded), with two orders per accumulation pass and
             with one (option blochmap_orders).  rsrec_get_timing out[0] (device ms), out[1] (ms in the H|psi> launches), out[14..16] (ms
             in the accumulation passes, the phase tables, the final sums).  The accumulation is quoted in TB/s, counted as
             (1 + 2 ne) 5184 B per atom of every order's level -- what the one-order form moves; the two-order form moves (2 + 2 ne) 5184 B
             per atom and pair of orders, quoted as well --, the final sums as a share of the 78.6 TF FP64 matrix peak (2592 ne nk N flops).
  baseline : the route a user had: rsrec_chebyshev_bloch without a download + rsrec_chebyshev_ldos on the same ne energies, in calls of at
             most 4096 k-points, device ms summed over the calls.  Skipped above --baseline-nk-max points (`null` in the table).
  bare     : rsrec_chebyshev_pairs_direct with the one pair (source, source).
  streams  : what the projection pass of rsrec_chebyshev_lattice streams in this process on the same cell (one block stream of every atom per
             order); k_mfma_orth3 has no timer of its own in the library: its rate is the one on record (README: 5.35 TB/s), quoted beside.
`agreement`: the largest deviation of the map's a_k from the baseline's dosial at the shared points, relative to the largest value.
One JSON line per row on stdout; the whole table goes to --out."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TF = 78.6
ORTH3_TB_S = 5.35               # k_mfma_orth3's stream rate on record (README, rocprofv3 kernel trace)
NK_CALL = 4096                  # RSREC_BLOCH_NK_MAX: the baseline's call size


def spread(v):
    return [min(v), max(v)]


def main():
    import torch
    from bloch_reference import commensurate_k, supercell_cell
    from helpers import objects_from, supercell_problem
    from rslmtoasa_amd.green import Green
    from rslmtoasa_amd.lattice import active_region_sizes, supercell_positions
    from rslmtoasa_amd.recursion import Recursion, chebyshev_scaling
    ap = argparse.ArgumentParser()
    ap.add_argument("--lld", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", nargs="+", default=["22x22x22", "46x46x46"])
    ap.add_argument("--nk", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--ne", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--baseline-nk-max", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloch_map_v1.json"))
    args = ap.parse_args()
    rows, streams = [], []
    for cell in args.cells:
        dims = tuple(int(v) for v in cell.split("x"))
        p = supercell_problem(dims)
        kk = p["nn"].shape[0]
        src = kk // 2 + 1
        ham, lat, ctl, en = objects_from(p, [1], args.lld, emin=-3.0, emax=1.8)
        lat.ijpair = np.array([(src, src)], np.int32)
        cr, cvec = supercell_positions(dims), supercell_cell(dims)
        rec = Recursion(ham, lat, ctl, en)
        napply = 2 * args.lld + 1
        sizes = [1] + list(active_region_sizes(p["nn"], src, napply))               # atoms of the region at the orders 0 .. 2 lld + 1
        nact, npair = float(sum(sizes)), float(sum(sizes[1::2]))                      # (the two-order form runs at the odd orders)
        a, b = chebyshev_scaling(en.energy_min, en.energy_max)
        P = lambda x: x.ctypes.data_as(C.c_void_p)
        srcs = np.array([src], np.int32)
        t_proj = []                                              # the projection pass of rsrec_chebyshev_lattice on this cell, in this process
        one = np.ones((1, kk), np.complex128) / np.sqrt(kk)
        for r in range(args.rounds + 1):
            rec.chebyshev_lattice(np.arange(1, kk + 1, dtype=np.int32)[None, :], one, download=False)
            if r:
                t_proj.append(rec.timing()["rest_ms"])
        srow = dict(cell=cell, atoms=kk, orth3_tb_per_s_on_record=ORTH3_TB_S, projection_ms=spread(t_proj), projection_tb_per_s=spread([5184.0 * kk * (2 * args.lld + 2) / (1e9 * m) for m in t_proj]))
        streams.append(srow)
        print(json.dumps(srow), flush=True)
        for nk in args.nk:
            side = int(round(np.sqrt(nk)))
            assert side * side == nk, "nk must be a square: the grid is a plane"
            i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
            k = commensurate_k(dims, np.stack([i.ravel(), j.ravel(), np.zeros(nk, int)], axis=1))
            for ne in args.ne:
                ene = np.linspace(-1.5, 0.9, ne) if ne > 1 else np.array([-0.3])
                w = rec.chebyshev_green_weights(ene)
                out = torch.zeros(18 * ne * nk, dtype=torch.float64, device="cuda")

                def new_call(orders):
                    rec.set_option("blochmap_orders", orders)
                    rec._check(rec._L.rsrec_chebyshev_bloch_map(rec._h, 1, P(srcs), args.lld, a, b, P(cr), P(cvec), nk, P(k), 1, None, ne, P(w), None,
                                                                C.c_void_p(out.data_ptr())))
                    return rec.timing()

                gr = Green(rec, ene)
                with_base = nk <= args.baseline_nk_max

                def baseline(keep=False):
                    ms, parts = 0.0, []
                    for q0 in range(0, nk, NK_CALL):
                        kc = np.asfortranarray(k[:, q0:q0 + NK_CALL])
                        rec.chebyshev_bloch([src], kc, cr, cell=cvec, download=False)
                        ms += rec.timing()["total_ms"]
                        img = gr.chebyshev_ldos(nsites_total=kc.shape[1])
                        ms += rec.timing()["total_ms"]
                        if keep:
                            parts.append(img["dosial"].copy())
                    return ms, parts

                t = {o: {"total_ms": [], "hop_ms": [], "map_accum_ms": [], "map_phase_ms": [], "map_final_ms": []} for o in (2, 1)}
                t_base, t_bare = [], []
                for o in (2, 1):
                    new_call(o)                                  # warm-up: buffers, region lists, code objects
                row = dict(cell=cell, atoms=kk, lld=args.lld, nk=nk, ne=ne, rounds=args.rounds, sum_n_act=nact)
                if with_base:
                    a_map = out.cpu().numpy().reshape((18, ne, nk), order="F")
                    ref = np.concatenate(baseline(keep=True)[1], axis=0)              # dosial (image = k-point, 18, nen)
                    row["agreement"] = float(np.abs(a_map - ref.transpose(1, 2, 0)).max() / np.abs(ref).max())
                rec.chebyshev_recur_ij_direct(False)
                for _ in range(args.rounds):
                    for o in (2, 1):
                        tm = new_call(o)
                        for key in t[o]:
                            t[o][key].append(tm[key])
                    if with_base:
                        t_base.append(baseline()[0])
                    rec.chebyshev_recur_ij_direct(False)
                    t_bare.append(rec.timing()["total_ms"])
                rec.set_option("blochmap_orders", 2)
                counted = (1 + 2 * ne) * 5184.0 * nact
                moved = {1: counted, 2: (2 + 2 * ne) * 5184.0 * npair}
                flop = 2592.0 * ne * nk * sizes[-1]
                for o, name in ((2, "map_two_orders"), (1, "map_one_order")):
                    v = t[o]
                    row[name] = dict(device_ms=spread(v["total_ms"]), hop_ms=spread(v["hop_ms"]), accum_ms=spread(v["map_accum_ms"]), phase_ms=spread(v["map_phase_ms"]),
                                     final_ms=spread(v["map_final_ms"]), accum_counted_tb_per_s=spread([counted / (1e9 * m) for m in v["map_accum_ms"]]),
                                     accum_moved_tb_per_s=spread([moved[o] / (1e9 * m) for m in v["map_accum_ms"]]),
                                     final_share_of_peak=spread([flop / (1e9 * m) / PEAK_TF for m in v["map_final_ms"]]))
                row["bare_device_ms"] = spread(t_bare)
                row["baseline_device_ms"] = spread(t_base) if with_base else None
                best = min(row["map_two_orders"]["device_ms"][1], row["map_one_order"]["device_ms"][1])
                row["baseline_over_map"] = [min(t_base) / best, max(t_base) / min(t[2]["total_ms"] + t[1]["total_ms"])] if with_base else None
                rows.append(row)
                print(json.dumps(row), flush=True)
        rec.close()
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/time_bloch_map.py", streams=streams, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
