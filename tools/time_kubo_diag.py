"""Full against orbital-diagonal Kubo moments, in one process, on the periodic fcc Pt cell the README numbers are quoted on.

    python tools/time_kubo_diag.py [--cells 20] [--ll 50 500] [--nvec 1 8] [--reps 3] [--out DIR]

For every (cond_ll, nvec): rsrec_kubo_moments (the full route: every element of the 18 x 18 blocks, downloaded into the host array)
and rsrec_kubo_moments_diag (the 18 diagonals, downloaded; and resident only), then the integrand at nE = 2510 from the full host
moments (rsrec_kubo_integrand: the host loop picks the diagonals and uploads them) against the resident diagonals
(rsrec_kubo_integrand_diag with NULL).  One warm-up call of each, then the median of --reps calls: device ms of the call, of its SpMMs
and of its contractions (rsrec_get_timing), and the wall ms around the call, which includes the download.  One JSON line per
configuration, also written to DIR/kubo_diag_l<cond_ll>_v<nvec>.json with --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FCC_PRIMITIVE = [[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]


def main():
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    from cond_reference import energy_mesh
    from helpers import load_golden
    import rslmtoasa_amd.recursion as R
    from rslmtoasa_amd.conductivity import Conductivity
    from rslmtoasa_amd.lattice import bcc_supercell
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=20)
    ap.add_argument("--ll", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--nvec", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    z = load_golden("fccPt_kubo")
    n = args.cells
    nn = bcc_supercell((n, n, n), z["slot_vec"], primitive=np.array(FCC_PRIMITIVE))
    kk = nn.shape[0]
    a, b = float(z["acheb"]), float(z["bcheb"])
    half = a * float(np.float32(2) - np.float32(0.3)) / 2
    en = Energy(b - half, b + half)
    ham = Hamiltonian(ee=z["ee"], lsham=z["lsham"])
    lat = Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=np.array([1], np.int32), nmax=0, ntype=1)
    rec = Recursion(ham, lat, Control(lld=max(args.ll), nsp=2), en, device=0)
    R.chebyshev_scaling = lambda emin, emax: (a, b)
    cond = Conductivity(rec)
    ene = energy_mesh(en.energy_min, en.energy_max, 2500)

    def timed(fn):
        """median over the repeats of (wall ms, device ms, SpMM ms, contraction ms) after one warm-up call; the last result"""
        out = fn()
        rows = []
        for _ in range(args.reps):
            del out
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            wall = (time.perf_counter() - t0) * 1e3
            t = rec.timing()
            rows.append((wall, t["total_ms"], t["hop_ms"], t["rest_ms"]))
        med = np.median(np.array(rows), axis=0)
        return dict(zip(("wall_ms", "device_ms", "spmm_ms", "contract_ms"), (round(float(x), 3) for x in med))), out

    for L in args.ll:
        for nvec in args.nvec:
            atl = np.arange(1, nvec + 1, dtype=np.int32)
            mom = lambda **kw: rec.compute_moments_stochastic(z["v_a"], z["v_b"], L, atlist=atl, **kw)   # noqa: E731
            res = dict(atoms=kk, cond_ll=L, nvec=nvec, reps=args.reps, nen=int(ene.size))
            res["full"], mu = timed(lambda: mom())
            res["integrand_from_host_full"], i_full = timed(lambda: cond.integrand(mu, ene))
            d_full = mu[np.arange(18), np.arange(18)]
            del mu
            res["diag"], d = timed(lambda: mom(diag=True))
            res["diag_vs_full_rel"] = float(max(np.abs(d[..., v] - d_full[..., v]).max() / np.abs(d_full[..., v]).max() for v in range(nvec)))
            res["diag_resident_only"], _ = timed(lambda: mom(diag=True, resident_only=True))
            res["integrand_from_resident_diag"], i_res = timed(lambda: cond.integrand(None, ene))
            res["integrand_rel"] = float(np.abs(i_res - i_full).max() / np.abs(i_full).max())
            for k in ("wall_ms", "device_ms", "contract_ms"):
                res["speedup_" + k] = round(res["full"][k] / res["diag"][k], 2)
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                with open(os.path.join(args.out, "kubo_diag_l%d_v%d.json" % (L, nvec)), "w") as f:
                    f.write(line + "\n")
            del d, d_full
    rec.close()


if __name__ == "__main__":
    main()
