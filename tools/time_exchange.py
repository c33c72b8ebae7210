"""Device time of rsrec_exchange (kernels_exchange.hpp) at nE = 2510 on chains already in GPU memory, and the ratio to
rsrec_block_green's kernels for the same 4P chains (the continued fraction alone, g0 written to device memory, not reduced).

    python tools/time_exchange.py [--lld 20 50] [--pairs 8 64 512] [--reps 3]

Prints one JSON line per (lld, pairs): median device ms of the exchange call and per pair, and -- where the g0 of the chains fits a
host buffer (pairs <= 64) -- the median ms of rsrec_block_green's Green kernels and the ratio exchange / block_green."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    import pair_cases as T
    from rslmtoasa_amd.exchange import Exchange
    ap = argparse.ArgumentParser()
    ap.add_argument("--lld", type=int, nargs="+", default=[20, 50])
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for lld in args.lld:
        base = np.array([(1, 2), (1, 9), (3, 17), (5, 60)], np.int32)
        rec, g, ene, nv1, dpar = T.setup(base, lld=lld, channels=2501)
        rec.zsqr()
        a_inf, b_inf, _, _ = g.terminator(nsites=16)
        x = Exchange(rec, g)
        for n in args.pairs:
            reps = (n + 3) // 4
            ta = torch.from_numpy(np.ascontiguousarray(rec.a_b[..., :16].transpose(3, 2, 1, 0))).cuda().repeat(reps, 1, 1, 1)[:4 * n].contiguous()
            tb = torch.from_numpy(np.ascontiguousarray(rec.b2_b[..., :16].transpose(3, 2, 1, 0))).cuda().repeat(reps, 1, 1, 1)[:4 * n].contiguous()
            ai, bi = np.tile(a_inf, (1, 1, reps))[..., :4 * n], np.tile(b_inf, (1, 1, reps))[..., :4 * n]
            rec.lattice.ijpair = np.tile(base, (reps, 1))[:n]
            dp = np.tile(dpar, (1, 1, 1, reps))[..., :n]
            t_x = []
            for _ in range(args.reps):
                x.compute(-0.05, nv1, dp, coef=(ta, tb), a_inf=ai, b_inf=bi)
                t_x.append(x.timing()[1])
            row = dict(lld=lld, pairs=n, nen=len(ene), exchange_ms=float(np.median(t_x)), ms_per_pair=float(np.median(t_x)) / n)
            if n <= 64:
                a_h = np.asfortranarray(np.tile(rec.a_b[..., :16], (1, 1, 1, reps))[..., :4 * n])
                b_h = np.asfortranarray(np.tile(rec.b2_b[..., :16], (1, 1, 1, reps))[..., :4 * n])
                g0 = np.zeros((18, 18, len(ene), 4 * n), np.complex128, order="F")
                import ctypes as C
                P = lambda a: a.ctypes.data_as(C.c_void_p)
                t_g = []
                for _ in range(args.reps):
                    rec._check(rec._L.rsrec_block_green(rec._h, 4 * n, lld, len(ene), P(g.ene), 0.0, 0.0, 0, P(np.asfortranarray(ai)), P(np.asfortranarray(bi)),
                                                        P(a_h), P(b_h), P(g0)))
                    t_g.append(rec.timing()["hop_ms"])
                row.update(block_green_ms=float(np.median(t_g)), ratio=float(np.median(t_x)) / float(np.median(t_g)))
            print(json.dumps(row), flush=True)
        rec.close()


if __name__ == "__main__":
    main()
