"""Three responses to one applied field: one rsrec_kubo_moments_diag_multi call against three rsrec_kubo_moments_diag calls, in one
process, on the periodic fcc Pt cell the README numbers are quoted on.

    python tools/time_kubo_multi.py [--cells 20] [--ll 50 500] [--nvec 1 8] [--reps 3] [--out DIR]

For every (cond_ll, nvec), without and with hoh: the output operators are the fixture's v_a, its v_b and their mean (nout = 3), the
input operator its v_b; nothing is downloaded (the moments stay resident, as the drop-in and Conductivity.integrand(None, ...) use
them).  One warm-up call of each kind, then --reps rounds of the multi call followed by the three single-response calls; per side
the median over the rounds of the device ms, the SpMM ms, the contraction ms (rsrec_get_timing; the single side: the sum of its
three calls) and the SpMM launches.  A last round downloads both sides and records the largest deviation of a set from its
single-response call, relative to the set's largest moment.  One JSON line per (hoh, cond_ll, nvec); with --out
DIR/kubo_multi_l<cond_ll>_v<nvec>.json holds the configuration's line with both hoh settings."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FCC_PRIMITIVE = [[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]
KEYS = (("device_ms", "total_ms"), ("spmm_ms", "hop_ms"), ("contract_ms", "rest_ms"), ("spmm_launches", "hop_launches"))


def main():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    from helpers import load_golden
    import rslmtoasa_amd.recursion as R
    from rslmtoasa_amd.lattice import bcc_supercell
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=20)
    ap.add_argument("--ll", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--nvec", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.cells
    results = {}
    for hoh in (False, True):
        z = load_golden("fccPt_kubo_hoh" if hoh else "fccPt_kubo")
        nn = bcc_supercell((n, n, n), z["slot_vec"], primitive=np.array(FCC_PRIMITIVE))
        kk = nn.shape[0]
        a, b = float(z["acheb"]), float(z["bcheb"])
        half = a * float(np.float32(2) - np.float32(0.3)) / 2
        ham = Hamiltonian(ee=z["ee"], lsham=z["lsham"], eeo=z["eeo"], enim=z["enim"], hoh=True) if hoh else Hamiltonian(ee=z["ee"], lsham=z["lsham"])
        lat = Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=np.array([1], np.int32), nmax=0, ntype=1)
        rec = Recursion(ham, lat, Control(lld=max(args.ll), nsp=2), Energy(b - half, b + half), device=0)
        R.chebyshev_scaling = lambda emin, emax, a=a, b=b: (a, b)
        v_outs = [z["v_a"], z["v_b"], 0.5 * (z["v_a"] + z["v_b"])]
        vo_outs = [z["vo_a"], z["vo_b"], 0.5 * (z["vo_a"] + z["vo_b"])] if hoh else [None] * 3
        v_out = np.stack(v_outs, axis=-1)
        vo_out = np.stack(vo_outs, axis=-1) if hoh else None
        vo_b = z["vo_b"] if hoh else None

        def timing():
            t = rec.timing()
            return np.array([t[k] for _, k in KEYS])

        for L in args.ll:
            for nvec in args.nvec:
                atl = np.arange(1, nvec + 1, dtype=np.int32)

                def multi(resident_only=True):
                    return rec.compute_moments_stochastic_multi(v_out, z["v_b"], L, vo_out=vo_out, vo_b=vo_b, atlist=atl, resident_only=resident_only)

                def single(j, resident_only=True):
                    return rec.compute_moments_stochastic(v_outs[j], z["v_b"], L, vo_a=vo_outs[j], vo_b=vo_b, atlist=atl, diag=True,
                                                          resident_only=resident_only)
                multi()
                single(0)
                rows_m, rows_s = [], []
                for _ in range(args.reps):
                    multi()
                    rows_m.append(timing())
                    s = np.zeros(len(KEYS))
                    for j in range(3):
                        single(j)
                        s += timing()
                    rows_s.append(s)
                mu = multi(resident_only=False)
                dev = 0.0
                for j in range(3):
                    one = single(j, resident_only=False)
                    dev = max(dev, float(np.abs(mu[..., j] - one).max() / np.abs(one).max()))
                    del one
                del mu
                side = lambda rows: {k: round(float(x), 3) for (k, _), x in zip(KEYS, np.median(np.array(rows), axis=0))}   # noqa: E731
                res = dict(multi=side(rows_m), three_single_calls=side(rows_s), largest_deviation_rel=dev)
                for k in ("device_ms", "spmm_ms"):
                    res["multi_over_single_" + k] = round(res["multi"][k] / res["three_single_calls"][k], 3)
                both = results.setdefault((L, nvec), dict(atoms=kk, cond_ll=L, nvec=nvec, nout=3, reps=args.reps))
                both["hoh" if hoh else "no_hoh"] = res
                line = json.dumps(both)
                print(line, flush=True)
                if args.out:                           # (rewritten with both settings once the hoh pass reaches the configuration)
                    os.makedirs(args.out, exist_ok=True)
                    with open(os.path.join(args.out, "kubo_multi_l%d_v%d.json" % (L, nvec)), "w") as f:
                        f.write(line + "\n")
        rec.close()


if __name__ == "__main__":
    main()
