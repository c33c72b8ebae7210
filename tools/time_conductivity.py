"""Device time of rsrec_kubo_integrand (the conductivity integrand, kernels_cond.hpp) at nE = 2510 on moments already in GPU memory.

    python tools/time_conductivity.py [--ll 50 500] [--nvec 1 3 8] [--reps 5]

Prints one JSON line per (cond_ll, nvec): the median device ms of the call and of its contraction kernels, and the contraction rate
in the flops the factorised form needs (4 real GEMMs of nE x L x L per orbital and vector: 8 nE L^2 x 18 x nvec) as a fraction of
the 78.6 TFLOP/s FP64 matrix peak."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TF = 78.6


def main():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    from helpers import load_golden
    from cond_reference import energy_mesh
    from rslmtoasa_amd.conductivity import Conductivity
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion
    ap = argparse.ArgumentParser()
    ap.add_argument("--ll", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--nvec", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    z = load_golden("fccPt_kubo")
    ham = Hamiltonian(ee=z["ee"], lsham=z["lsham"])
    lat = Lattice(nn=z["nn"], iz=z["iz"], irec=np.asarray(z["atlist"], np.int32), ntype=1)
    en = Energy(-0.8, 0.6)
    rec = Recursion(ham, lat, Control(), en, device=0)
    cond = Conductivity(rec)
    ene = energy_mesh(en.energy_min, en.energy_max, 2500)
    for L in args.ll:
        for nvec in args.nvec:
            mu = torch.randn((nvec, L, L, 18, 18), dtype=torch.complex128, device="cuda")
            cond.integrand(mu, ene)                                       # warm-up: buffers, code objects
            tot, con = [], []
            for _ in range(args.reps):
                cond.integrand(mu, ene)
                t = cond.timing()
                tot.append(t[0]); con.append(t[1])
            flop = 8.0 * ene.size * L * L * 18 * nvec
            c = float(np.median(con))
            print(json.dumps(dict(cond_ll=L, nvec=nvec, nen=int(ene.size), call_ms=round(float(np.median(tot)), 3), contract_ms=round(c, 3),
                                  gflop=round(flop / 1e9, 2), tflops=round(flop / c / 1e9, 2), frac_peak=round(flop / c / 1e9 / PEAK_TF, 3))), flush=True)
            del mu
            torch.cuda.empty_cache()
    rec.close()


if __name__ == "__main__":
    main()
