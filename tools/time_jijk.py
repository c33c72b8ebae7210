"""Device time of the auxiliary-GF exchange tensor per pair and of the spin-lattice Jijk per trio, at lld 20 and the 2 510 energies of
bench.py's LDOS leg, on the chains the pair recursion left on the device (Exchange.aux: rsrec_exchange_aux; Exchange.spin_lattice:
rsrec_spin_lattice).  Prints one JSON line: median device ms of the call (rsrec_get_timing out[0]) and of its kernel stage (out[5]),
per pair / per trio, and the device memory the process held after the call.  The host route to compare with is the reference's own
type(exchange) over the same objects: oracle/_ref/jijk_gpu.x with JIJK_DRIVER_MODE=plain (tests/fortran/jijk_gpu_driver.f90), whose
g_timer report carries the region `jijk-plain` (the routine) and `fetch-intersite` / the host intersite stage before it; with
JIJK_DRIVER_MODE=gpu the region is `jijk-gpu`.  Run both in the same session on an input with trios at lld 20 and channels_ldos 2500.

    python tools/time_jijk.py --reps 5 --warmup 2
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=22)
    ap.add_argument("--trios", type=int, default=21)
    ap.add_argument("--lld", type=int, default=20)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from rslmtoasa_amd.exchange import Exchange, disp_matrix, trio_pairs
    from rslmtoasa_amd.green import Green
    from rslmtoasa_amd.lattice import bcc_supercell, spread_sites, supercell_positions
    from rslmtoasa_amd.recursion import Control, Energy, Hamiltonian, Lattice, Recursion

    st = bench.load_stencil(False)
    n = args.cells
    nn = bcc_supercell((n, n, n), st["slot_vec"])
    kk = nn.shape[0]
    first = spread_sites(kk, args.trios)
    t = np.arange(args.trios)
    trios = np.stack([first, nn[first - 1, 1 + t % 14], nn[first - 1, 1 + (t + 5) % 14]], axis=1).astype(np.int32)   # i and two of its neighbours
    pairs = trio_pairs(trios)
    lat = Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=first, nmax=0, ntype=1, cr=supercell_positions((n, n, n)))
    lat.ijpair = pairs
    ham = Hamiltonian(ee=st["ee"], lsham=st["lsham"], eeo=None, enim=None, hall=None, hallo=None, hoh=False)
    rec = Recursion(ham, lat, Control(lld=args.lld, nsp=2, recur="block"), Energy(energy_min=-3.0, energy_max=1.8), device=0)
    gz = np.load(os.path.join(ROOT, "tests", "golden", "bccFe_nsp2_block_green.npz"), allow_pickle=False)
    ene = float(gz["ene_full_first"]) + float(gz["ene_full_step"]) * np.arange(int(gz["nen_full"]))
    gr = Green(rec, ene)
    rec.recur_b_ij()
    rng = np.random.default_rng(1)
    aa = np.zeros((2, 3, 2, 2, len(pairs)), order="F")
    aa[0], aa[1] = rng.uniform(-0.15, 0.4, aa[0].shape), rng.uniform(0.04, 0.22, aa[1].shape)
    at = np.zeros((3, 3, 2, 3, len(trios)), order="F")
    at[0], at[1], at[2] = rng.uniform(-0.15, 0.4, at[0].shape), rng.uniform(0.04, 0.22, at[1].shape), rng.uniform(0.01, 0.45, at[2].shape)
    dm = np.asfortranarray(np.stack([disp_matrix(rng.normal(size=3), 2.6) for _ in trios], axis=-1))
    nv1 = len(ene) - 9
    fermi = float(ene[len(ene) // 2])
    x = Exchange(rec, gr)
    out = {"lld": args.lld, "nen": len(ene), "pairs": len(pairs), "trios": len(trios)}
    for name, call, units in (("aux", lambda: x.aux(fermi, nv1, aa, resident=True), len(pairs)),
                              ("jijk", lambda: x.spin_lattice(fermi, nv1, at, dm, resident=True), len(trios))):
        tot, ker = [], []
        for r in range(args.warmup + args.reps):
            call()
            if r >= args.warmup:
                a, b = x.timing()
                tot.append(a)
                ker.append(b)
        free, total = torch.cuda.mem_get_info(0)
        out[name] = {"device_ms_per_unit": statistics.median(tot) / units, "kernel_ms_per_unit": statistics.median(ker) / units,
                     "device_ms_min_max": [min(tot), max(tot)], "device_mem_in_use_MiB": (total - free) / 2 ** 20}
    rec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
