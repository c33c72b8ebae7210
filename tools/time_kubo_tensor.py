"""Three responses to three applied fields: one rsrec_kubo_moments_diag_tensor call against three rsrec_kubo_moments_diag_multi calls,
and the grouped contraction (option kubo_setgroup) against the per-set one, in one process, on the periodic fcc Pt cell the README
numbers are quoted on.

    python tools/time_kubo_tensor.py [--cells 20] [--ll 50 500] [--nvec 1 8] [--reps 3] [--out DIR]

For every (cond_ll, nvec), without and with hoh: the operators on both sides are the fixture's v_a, its v_b and their mean (nin = nout
= 3); nothing is downloaded (the moments stay resident).  Legs: the tensor call under kubo_setgroup = 1, 2 and 3, and the three multi
calls (one per input).  Every leg gets one warm-up and then --reps rounds; per leg the median and the min - max over the rounds of the
device ms, the SpMM ms, the contraction ms (rsrec_get_timing; the multi side: the sum of its three calls) and the SpMM launches.  A last
round downloads the tensor call's moments at every group width and records the largest deviation of a set from its single call
(rsrec_kubo_moments_diag; the groups of 2 and 3 through the per-set route's array), which must be 0.0.  Ratios: the tensor call at the
library's default (kubo_setgroup = 0) over the three multi calls, and the contraction of the groups of 2 and 3 over the per-set one
with the verdict "faster by more than the spread".  One JSON line per (hoh, cond_ll, nvec); with --out
DIR/kubo_tensor_l<cond_ll>_v<nvec>.json holds the configuration's line with both hoh settings."""
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
DEFAULT_SETGROUP = 2                                   # what kubo_setgroup = 0 means in the library


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
        v_ops = [z["v_a"], z["v_b"], 0.5 * (z["v_a"] + z["v_b"])]
        vo_ops = [z["vo_a"], z["vo_b"], 0.5 * (z["vo_a"] + z["vo_b"])] if hoh else [None] * 3
        v_all = np.stack(v_ops, axis=-1)
        vo_all = np.stack(vo_ops, axis=-1) if hoh else None

        def timing():
            t = rec.timing()
            return np.array([t[k] for _, k in KEYS])

        for L in args.ll:
            for nvec in args.nvec:
                atl = np.arange(1, nvec + 1, dtype=np.int32)

                def tensor(group, resident_only=True):
                    rec.set_option("kubo_setgroup", group)
                    try:
                        return rec.compute_moments_stochastic_tensor(v_all, v_all, L, vo_out=vo_all, vo_in=vo_all, atlist=atl, resident_only=resident_only)
                    finally:
                        rec.set_option("kubo_setgroup", 0)

                def multi(i):
                    rec.compute_moments_stochastic_multi(v_all, v_ops[i], L, vo_out=vo_all, vo_b=vo_ops[i], atlist=atl, resident_only=True)

                def three_multi():
                    s = np.zeros(len(KEYS))
                    for i in range(3):
                        multi(i)
                        s += timing()
                    return s

                def leg(call):
                    print("leg: hoh=%d cond_ll=%d nvec=%d" % (hoh, L, nvec), file=sys.stderr, flush=True)    # (a leg at cond_ll = 500 with 8 vectors takes a minute)
                    call()                                                   # warm-up: the buffers of this leg's shape
                    rows = np.array([call() for _ in range(args.reps)])
                    return {k: dict(median=round(float(np.median(rows[:, q])), 3), min=round(float(rows[:, q].min()), 3), max=round(float(rows[:, q].max()), 3))
                            for q, (k, _) in enumerate(KEYS)}

                legs = {"tensor_setgroup_%d" % g: leg(lambda g=g: (tensor(g), timing())[1]) for g in (1, 2, 3)}
                legs["three_multi_calls"] = leg(three_multi)
                dev = 0.0
                mu = tensor(1, resident_only=False)
                for i in range(3):
                    for j in range(3):
                        one = rec.compute_moments_stochastic(v_ops[j], v_ops[i], L, vo_a=vo_ops[j], vo_b=vo_ops[i], atlist=atl, diag=True)
                        dev = max(dev, float(np.abs(mu[..., j, i] - one).max() / np.abs(one).max()))
                        del one
                for g in (2, 3):                                             # the grouped routes against the per-set one, set by set
                    other = tensor(g, resident_only=False)
                    for s in range(9):
                        dev = max(dev, float(np.abs(other[..., s % 3, s // 3] - mu[..., s % 3, s // 3]).max() / np.abs(mu[..., s % 3, s // 3]).max()))
                    del other
                del mu
                res = dict(legs, largest_deviation_rel=dev)
                default = legs["tensor_setgroup_%d" % DEFAULT_SETGROUP]
                for k in ("device_ms", "spmm_ms"):
                    res["tensor_over_three_multi_" + k] = round(default[k]["median"] / legs["three_multi_calls"][k]["median"], 3)
                res["tensor_faster_than_three_multi"] = bool(default["device_ms"]["median"] < legs["three_multi_calls"]["device_ms"]["median"])
                c1 = legs["tensor_setgroup_1"]["contract_ms"]
                for g in (2, 3):
                    cg = legs["tensor_setgroup_%d" % g]["contract_ms"]
                    res["setgroup_%d_over_1_contract_ms" % g] = round(cg["median"] / c1["median"], 3)
                    # "beats by more than the spread": the medians differ by more than the min - max spread of either leg's rounds
                    res["setgroup_%d_beats_1_beyond_spread" % g] = bool(c1["median"] - cg["median"] > max(c1["max"] - c1["min"], cg["max"] - cg["min"]))
                both = results.setdefault((L, nvec), dict(atoms=kk, cond_ll=L, nvec=nvec, nin=3, nout=3, reps=args.reps, default_setgroup=DEFAULT_SETGROUP))
                both["hoh" if hoh else "no_hoh"] = res
                line = json.dumps(both)
                print(line, flush=True)
                if args.out:                           # (rewritten with both settings once the hoh pass reaches the configuration)
                    os.makedirs(args.out, exist_ok=True)
                    with open(os.path.join(args.out, "kubo_tensor_l%d_v%d.json" % (L, nvec)), "w") as f:
                        f.write(line + "\n")
        rec.close()


if __name__ == "__main__":
    main()
