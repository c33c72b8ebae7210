"""Device time of rsrec_kubo_single_shot (kernels_shot.hpp) against the moment route, in one process.

    python tools/time_kubo_shot.py [--cells 20 46] [--cond-ll 50 500 2000] [--vectors 1 4] [--ne 2 16] [--orders 1 2 4 8 16]
                                   [--rounds 3] [--baseline-max-ll 4096] [--out profiles/kubo_shot_v1.json] [--append]

Cells: periodic fcc Pt supercells n^3 (20: 8 000 atoms, 46: 97 336) with the blocks and velocity operators of tests/golden/fccPt_kubo.npz,
built as ``bench.py --workload kubo`` builds its cell.  Per (cell, cond_ll, vectors, ne, shot_orders), after one warm-up call, --rounds
calls with random weights: device ms of the call (rsrec_get_timing out[0]), ms in the SpMM launches (out[1]), in the accumulation passes
(out[17]) with the GB/s of the bytes they move -- per pass and chain (orders of the pass + 2 ne) block streams of kk * 5 184 B --, and in
the final stage (out[18]), each as min and max over the rounds.  The existing route, rsrec_kubo_moments_diag + rsrec_kubo_integrand_diag
on 8 energies, runs in the same process with the same cond_ll and vectors wherever it runs at all (cond_ll <= RSREC_COND_LL_MAX = 4 096; a
smaller --baseline-max-ll records it as not run beyond that), with option kubo_lchunk at 0, and the row records how the library planned
it: the left chunks it formed over the call's vector batches and the left vectors per chunk (rsrec_get_timing out[19], out[20]).  Every row is printed as it is measured and the file is rewritten
after every row, so a run that is cut short keeps what it measured.  No pass/fail ratio."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FCC_PRIMITIVE = [[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]


def span(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def make_cell(n, z):
    from rslmtoasa_amd.lattice import bcc_supercell
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion
    nn = bcc_supercell((n, n, n), z["slot_vec"], primitive=np.array(FCC_PRIMITIVE))
    kk = nn.shape[0]
    ham = Hamiltonian(ee=z["ee"], lsham=z["lsham"], hoh=False)
    lat = Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=np.array([1], np.int32), nmax=0, ntype=1)
    return Recursion(ham, lat, Control(lld=50, nsp=2), Energy(), device=0), kk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[20, 46])
    ap.add_argument("--cond-ll", type=int, nargs="+", default=[50, 500, 2000])
    ap.add_argument("--vectors", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--ne", type=int, nargs="+", default=[2, 16])
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-max-ll", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds (a sweep made in several runs)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    import rslmtoasa_amd.recursion as R
    from cond_reference import energy_mesh
    from helpers import load_golden
    from rslmtoasa_amd.conductivity import Conductivity
    z = load_golden("fccPt_kubo")
    a, b = float(z["acheb"]), float(z["bcheb"])
    R.chebyshev_scaling = lambda emin, emax: (a, b)    # the fixture's window, as bench.py pins it
    result = dict(tool="tools/time_kubo_shot.py", device=torch.cuda.get_device_name(0), rounds=args.rounds, rows=[], baseline=[])
    if args.append and args.out and os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        result["rows"], result["baseline"] = old["rows"], old["baseline"]

    def write():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    rng = np.random.default_rng(7)
    for n in args.cells:
        rec, kk = make_cell(n, z)
        cond = Conductivity(rec)
        for cond_ll in args.cond_ll:
            for nvec in args.vectors:
                atlist = np.arange(1, nvec + 1, dtype=np.int32)
                for ne in args.ne:
                    w = (rng.standard_normal((2, cond_ll, ne)) + 1j * rng.standard_normal((2, cond_ll, ne))) / cond_ll
                    for P in args.orders:
                        rec.set_option("shot_orders", P)
                        t = {k: [] for k in ("total_ms", "hop_ms", "shot_accum_ms", "shot_final_ms")}
                        for r in range(args.rounds + 1):
                            rec.kubo_single_shot(z["v_a"], z["v_b"], w[0], w[1], atlist=atlist)
                            tm = rec.timing()
                            if r:                      # (round 0: warm-up -- buffers, code objects)
                                for k in t:
                                    t[k].append(tm[k])
                        nbatch_chains = 2 * nvec      # chains over all batches of the call
                        passes = -(-cond_ll // P)
                        gbytes = nbatch_chains * kk * 5184.0 * (cond_ll + 2.0 * ne * passes) * 1e-9
                        row = dict(cells=n, atoms=kk, cond_ll=cond_ll, vectors=nvec, ne=ne, shot_orders=P, hop_launches=int(tm["hop_launches"]),
                                   device_ms=span(t["total_ms"]), spmm_ms=span(t["hop_ms"]), accum_ms=span(t["shot_accum_ms"]),
                                   accum_gb=round(gbytes, 3), accum_gb_per_s=span([gbytes / (x * 1e-3) for x in t["shot_accum_ms"]]),
                                   final_ms=span(t["shot_final_ms"]))
                        print(json.dumps(row), flush=True)
                        result["rows"].append(row)
                        write()
                    rec.set_option("shot_orders", 0)
                base = dict(cells=n, atoms=kk, cond_ll=cond_ll, vectors=nvec, energies=8, kubo_lchunk_option=0)
                if cond_ll <= args.baseline_max_ll:
                    ene = energy_mesh(rec.en.energy_min, rec.en.energy_max, 2500)[600:2200:200]
                    tm_m, tm_i = [], []
                    for r in range(args.rounds + 1):
                        rec.compute_moments_stochastic(z["v_a"], z["v_b"], cond_ll, atlist=atlist, diag=True, resident_only=True)
                        m = rec.timing()
                        cond.integrand(None, ene)
                        if r:
                            tm_m.append(m)
                            tm_i.append(cond.timing()[0])
                    base.update(moments_device_ms=span([m["total_ms"] for m in tm_m]), moments_spmm_ms=span([m["hop_ms"] for m in tm_m]),
                                moments_contraction_ms=span([m["rest_ms"] for m in tm_m]), moments_hop_launches=int(tm_m[-1]["hop_launches"]),
                                integrand_device_ms=span(tm_i))
                    base.update(left_chunks=int(tm_m[-1]["kubo_left_chunks"]), kubo_lchunk_planned=int(tm_m[-1]["kubo_lchunk_planned"]))
                else:
                    base.update(not_run="cond_ll above --baseline-max-ll = %d" % args.baseline_max_ll)
                print(json.dumps(base), flush=True)
                result["baseline"].append(base)
                write()
        rec.close()


if __name__ == "__main__":
    main()
