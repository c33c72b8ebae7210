#!/usr/bin/env python3
"""Wall time of the density-of-states stage behind the Chebyshev recursion, for the problem of bench.py --full's `ldos` leg (bcc Fe
22^3 cell, 64 sites, LL = 50, the reference's 2510-point mesh) with --recur chebyshev:

  --route ldos   Green.chebyshev_ldos(): rsrec_chebyshev_ldos on the moments the recursion left on the device
  --route g0     the route it replaces: Green.chebyshev_green() with host arrays (moments up, g0(18,18,nE,site) down), then the
                 reduction of bands.f90:258-268 in numpy.  Needs nothing the library did not have before rsrec_chebyshev_ldos, so
                 RSREC_LIB may point at an older build of librsrec.so.

Wall time around the call, `--warmup` calls first, median of `--reps`; one JSON line.

    python tools/time_cheb_ldos.py --route ldos --reps 5 --warmup 2
    python tools/time_cheb_ldos.py --route g0 --reps 5 --warmup 2
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--route", choices=("ldos", "g0"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=22)
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--lld", type=int, default=50)
    args = ap.parse_args()

    import numpy as np
    import bench
    from rslmtoasa_amd import _lib
    from rslmtoasa_amd.green import Green
    from rslmtoasa_amd.lattice import bcc_supercell, spread_sites, supercell_positions
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

    st = bench.load_stencil(False)
    n = args.cells
    nn = bcc_supercell((n, n, n), st["slot_vec"])
    kk = nn.shape[0]
    lat = Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=spread_sites(kk, args.sites), nmax=0, ntype=1, cr=supercell_positions((n, n, n)))
    ham = Hamiltonian(ee=st["ee"], lsham=st["lsham"], eeo=None, enim=None, hall=None, hallo=None, hoh=False)
    rec = Recursion(ham, lat, Control(lld=args.lld, nsp=2, recur="chebyshev"), Energy(energy_min=-3.0, energy_max=1.8), device=0)
    gz = np.load(os.path.join(ROOT, "tests", "golden", "bccFe_nsp2_block_green.npz"), allow_pickle=False)
    ene = float(gz["ene_full_first"]) + float(gz["ene_full_step"]) * np.arange(int(gz["nen_full"]))     # bench.py's mesh of the ldos leg
    gr = Green(rec, ene)
    t0 = time.perf_counter()
    rec.chebyshev_recur()
    t_rec = time.perf_counter() - t0

    d = np.arange(18)

    def ldos():
        return gr.chebyshev_ldos()["dosial"]

    def g0():
        g = gr.chebyshev_green(nsites=args.sites)
        gim = g[d, d].imag                                                  # bands.f90:258-268 (as tests/test_gpu_ldos.py ldos_from_g0)
        dosial = (-gim / np.pi).transpose(2, 0, 1)
        dosia = (-(gim[:9] + gim[9:]) / np.pi).sum(axis=0).T
        dosia.sum(axis=0)
        return dosial

    call = ldos if args.route == "ldos" else g0
    times, device_ms, kernel_ms = [], [], []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        out = call()
        t = time.perf_counter() - t0
        if k >= args.warmup:
            tm = rec.timing()
            times.append(t * 1e3); device_ms.append(tm["total_ms"]); kernel_ms.append(tm["hop_ms"])
    assert np.isfinite(out).all() and out.shape == (args.sites, 18, len(ene))
    rec.close()
    print(json.dumps({"route": args.route, "library": _lib.LIB_PATH, "cells": n, "sites": args.sites, "lld": args.lld, "energies": len(ene),
                      "warmup": args.warmup, "reps": args.reps, "wall_ms_median": statistics.median(times), "wall_ms": times,
                      "device_ms_median": statistics.median(device_ms), "kernel_ms_median": statistics.median(kernel_ms),
                      "recursion_wall_s": t_rec, "checksum": float(np.abs(out).sum())}))


if __name__ == "__main__":
    main()
