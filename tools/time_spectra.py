#!/usr/bin/env python3
"""Wall time of the SCF moment spectra (the 15 functionals Im Tr(O g0) behind bands%calculate_magnetic_moments, calculate_orbital_moments
and calculate_moments) behind the on-site recursion: bcc Fe 22^3 cell, 64 sites, LL = 50, the reference's 2510-point mesh.

  --route spectra  Green.block_spectra() / chebyshev_spectra(): one library call on the chains the recursion left on the device.
  --route g0       what it replaces: terminators and rsrec_block_green (or rsrec_chebyshev_green) of the 64 sites into host memory
                   (g0(18,18,nE,64), 833 MB), then the same 15 traces in numpy, batched over the energies.  Uses nothing newer than
                   rsrec_block_green, so it runs unchanged in a checkout of an older commit with that commit's library; the operators
                   come from --bands-file (rslmtoasa_amd/bands.py of this tree: plain numpy), loaded by path.
  --recur          block (default) or chebyshev.

Wall time around the call, `--warmup` calls first, median and min-max of `--reps`, plus rsrec_get_timing; one JSON line with a checksum
(sum of |spec|) that the two routes must share to rounding.

    python tools/time_spectra.py --route spectra --reps 5 --warmup 2
    python tools/time_spectra.py --route g0 --reps 5 --warmup 2
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--route", choices=("spectra", "g0"), required=True)
    ap.add_argument("--recur", choices=("block", "chebyshev"), default="block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=22)
    ap.add_argument("--sites", type=int, default=64)
    ap.add_argument("--lld", type=int, default=50)
    ap.add_argument("--bands-file", default=os.path.join(ROOT, "rslmtoasa_amd", "bands.py"))
    args = ap.parse_args()

    import numpy as np
    import bench
    from rslmtoasa_amd import _lib
    from rslmtoasa_amd.green import Green
    from rslmtoasa_amd.lattice import bcc_supercell, spread_sites
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

    spec_ = importlib.util.spec_from_file_location("bands_ops", args.bands_file)
    bands = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(bands)
    ops = bands.stack(bands.SCF_OPERATORS)

    st = bench.load_stencil(False)
    n = args.cells
    nn = bcc_supercell((n, n, n), st["slot_vec"])
    kk = nn.shape[0]
    lat = Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=spread_sites(kk, args.sites), nmax=0, ntype=1)
    ham = Hamiltonian(ee=st["ee"], lsham=st["lsham"], eeo=None, enim=None, hall=None, hallo=None, hoh=False)
    rec = Recursion(ham, lat, Control(lld=args.lld, nsp=2, recur=args.recur), Energy(energy_min=-3.0, energy_max=1.8), device=0)
    gz = np.load(os.path.join(ROOT, "tests", "golden", "bccFe_nsp2_block_green.npz"), allow_pickle=False)
    ene = float(gz["ene_full_first"]) + float(gz["ene_full_step"]) * np.arange(int(gz["nen_full"]))     # bench.py's mesh of the ldos leg
    if args.recur == "chebyshev":
        ene = np.linspace(-2.6, 1.4, len(ene))                  # inside (b - a, b + a), where the Chebyshev Green function is finite
    gr = Green(rec, ene)
    t0 = time.perf_counter()
    rec.recur_b() if args.recur == "block" else rec.chebyshev_recur()
    t_rec = time.perf_counter() - t0

    if args.route == "spectra":
        def call():
            return gr.block_spectra(ops) if args.recur == "block" else gr.chebyshev_spectra(ops)
    elif args.recur == "block":
        rec.zsqr()                                              # (once, outside the timed call; the spectra route roots inside it)

        def call():
            a_inf, b_inf, _, _ = gr.terminator(nsites=args.sites)
            g0 = gr.block_green(a_inf, b_inf, nsites=args.sites)
            return np.einsum("kji,ijes->kes", ops, g0).imag
    else:
        def call():
            g0 = gr.chebyshev_green(nsites=args.sites)
            return np.einsum("kji,ijes->kes", ops, g0).imag

    times, device_ms, kernel_ms = [], [], []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        out = call()
        t = time.perf_counter() - t0
        if k >= args.warmup:
            tm = rec.timing()
            times.append(t * 1e3); device_ms.append(tm["total_ms"]); kernel_ms.append(tm["hop_ms"])
    assert np.isfinite(out).all() and out.shape == (len(ops), len(ene), args.sites)
    rec.close()
    print(json.dumps({"route": args.route, "recur": args.recur, "library": _lib.LIB_PATH, "cells": n, "sites": args.sites, "lld": args.lld,
                      "energies": len(ene), "operators": len(ops), "warmup": args.warmup, "reps": args.reps,
                      "wall_ms_median": statistics.median(times), "wall_ms_min": min(times), "wall_ms_max": max(times), "wall_ms": times,
                      "device_ms_median": statistics.median(device_ms), "kernel_ms_median": statistics.median(kernel_ms),
                      "recursion_wall_s": t_rec, "checksum": float(np.abs(out).sum())}))


if __name__ == "__main__":
    main()
