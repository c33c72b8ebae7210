"""Device time of the per-atom blocks from whole-lattice seeds (rsrec_chebyshev_site_map, kernels_sitemap.hpp), its yardstick and the
route without the call, one process per cell on one MI355X.

    python tools/time_site_map.py [--cells 22 46] [--lld 50] [--rounds 3] [--vectors 8 64] [--ne 1 4 16] [--shapes 1x16 2x8 4x4 8x2]
                                  [--out profiles/site_map_v1.json] [--append]

The parent starts one child per cell (``--cell N``) and never opens the device itself.  Cells: periodic bcc Fe supercells n^3 (22: 10 648
atoms, 46: 97 336).  Per (vectors, ne, VTxPT), random-phase vectors and random weights, after one warm-up call --rounds calls without
d_full: device ms of the call (rsrec_get_timing out[0]), ms in the H|psi> launches (out[1]), ms in the accumulation passes (out[21]) and
their rate in bytes moved, (VT PT + 2 ne) 16 B per element and tile-pass with full tiles and passes counted as such, each as min and max.
The yardstick of the pass is not this code: k_shot_accum in the same process, rsrec_kubo_single_shot's accumulation time (out[17]) with
identity operators at the same ne, vectors and number of orders; both are also given as microseconds per vector and order (the single
shot advances two chains per vector).  The route without the call: rsrec_chebyshev on 64 spread sites plus rsrec_chebyshev_green on the
same ne energies, measured, and its EXTRAPOLATION to all atoms, kk / 64 times that.  Every row is printed as it is measured and the file is
rewritten after every row.  No pass/fail ratio."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def span(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def load(path):
    if path and os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return dict(tool="tools/time_site_map.py", rows=[], yardstick=[], route=[])


def child(args):
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    from helpers import objects_from, random_vec_coefficients, supercell_problem
    from rslmtoasa_amd.green import Green
    from rslmtoasa_amd.lattice import spread_sites
    from rslmtoasa_amd.recursion import Recursion
    n, lld, nmom = args.cell, args.lld, 2 * args.lld + 2
    p = supercell_problem((n, n, n))
    kk = p["nn"].shape[0]
    emin, emax = -3.0, 1.8
    rec = Recursion(*objects_from(p, spread_sites(kk, 64), lld, emin=emin, emax=emax), device=0)
    result = load(args.out)
    result["device"] = torch.cuda.get_device_name(0)

    def write():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    rng = np.random.default_rng(7)
    ident = np.zeros(p["ee"].shape, np.complex128, order="F")
    ident[:, :, 0, :] = np.eye(18)[:, :, None]
    for nvec in args.vectors:
        seeds, coefs = random_vec_coefficients(rng.random((kk, nvec)))
        for ne in args.ne:
            w = np.asfortranarray((rng.standard_normal((nmom, ne)) + 1j * rng.standard_normal((nmom, ne))) / nmom)
            for shape in args.shapes:
                vt, pt = (int(x) for x in shape.split("x"))
                rec.set_option("sitemap_vtile", vt)
                rec.set_option("sitemap_orders", pt)
                t = {k: [] for k in ("total_ms", "hop_ms", "site_accum_ms", "site_out_ms")}
                for r in range(args.rounds + 1):
                    rec.site_map(seeds, coefs, weights=w, blocks=False)
                    tm = rec.timing()
                    if r:                              # (round 0: warm-up -- buffers, code objects)
                        for k in t:
                            t[k].append(tm[k])
                nbatch = -(-nvec // 8)
                tiles = sum(-(-min(8, nvec - 8 * q) // vt) for q in range(nbatch))
                gbytes = tiles * (-(-nmom // pt)) * kk * 324.0 * 16.0 * (vt * pt + 2 * ne) * 1e-9
                row = dict(cells=n, atoms=kk, lld=lld, vectors=nvec, ne=ne, vtile=vt, orders=pt, hop_launches=int(tm["hop_launches"]),
                           device_ms=span(t["total_ms"]), hop_ms=span(t["hop_ms"]), accum_ms=span(t["site_accum_ms"]), out_ms=span(t["site_out_ms"]),
                           accum_gb=round(gbytes, 3), accum_gb_per_s=span([gbytes / (x * 1e-3) for x in t["site_accum_ms"]]),
                           accum_us_per_vector_order=span([1e3 * x / (nvec * nmom) for x in t["site_accum_ms"]]))
                print(json.dumps(row), flush=True)
                result["rows"].append(row)
                write()
            rec.set_option("sitemap_vtile", 0)
            rec.set_option("sitemap_orders", 0)
            # the yardstick: k_shot_accum on the same vectors, ne columns and nmom orders
            ta, tt = [], []
            for r in range(args.rounds + 1):
                rec.kubo_single_shot(ident, ident, w, w, seeds=seeds, coefs=coefs)
                tm = rec.timing()
                if r:
                    ta.append(tm["shot_accum_ms"])
                    tt.append(tm["total_ms"])
            gbytes = 2 * nvec * kk * 5184.0 * (nmom + 2.0 * ne * (-(-nmom // 16))) * 1e-9
            row = dict(cells=n, atoms=kk, cond_ll=nmom, vectors=nvec, ne=ne, shot_orders=16, device_ms=span(tt), accum_ms=span(ta), accum_gb=round(gbytes, 3),
                       accum_gb_per_s=span([gbytes / (x * 1e-3) for x in ta]), accum_us_per_vector_order=span([1e3 * x / (nvec * nmom) for x in ta]),
                       accum_us_per_chain_order=span([1e3 * x / (2 * nvec * nmom) for x in ta]))
            print(json.dumps(row), flush=True)
            result["yardstick"].append(row)
            write()
            # the route without the call: one chain per atom, here on 64 spread sites, and the Green function at the same energies
            ene = np.linspace(emin + 0.4, emax - 0.4, ne)
            tc, tg = [], []
            for r in range(args.rounds + 1):
                rec.chebyshev_recur()
                ms = rec.timing()["total_ms"]
                t0 = time.perf_counter()
                Green(rec, ene).chebyshev_green()
                if r:
                    tc.append(ms)
                    tg.append(1e3 * (time.perf_counter() - t0))
            both = [x + y for x, y in zip(tc, tg)]
            row = dict(cells=n, atoms=kk, lld=lld, sites=64, ne=ne, measured_with_vectors=nvec, chebyshev_device_ms=span(tc), green_wall_ms=span(tg),
                       ms_per_site=span([x / 64.0 for x in both]), extrapolated_to_all_atoms_s=span([x / 64.0 * kk * 1e-3 for x in both]))
            print(json.dumps(row), flush=True)
            result["route"].append(row)
            write()
    rec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[22, 46])
    ap.add_argument("--cell", type=int, default=None, help="run this one cell in this process (what the parent starts)")
    ap.add_argument("--lld", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vectors", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--ne", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--shapes", nargs="+", default=["1x16", "2x8", "4x4", "8x2"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_map_v1.json"))
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds (a sweep made in several runs)")
    args = ap.parse_args()
    if args.cell is not None:
        child(args)
        return
    if not args.append and args.out and os.path.exists(args.out):
        os.remove(args.out)
    for n in args.cells:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(n), "--lld", str(args.lld), "--rounds", str(args.rounds), "--out", args.out,
               "--vectors"] + [str(v) for v in args.vectors] + ["--ne"] + [str(v) for v in args.ne] + ["--shapes"] + list(args.shapes)
        rc = subprocess.call(cmd)
        if rc != 0:                                    # nothing more is started on the device behind a child that failed
            sys.exit(rc)


if __name__ == "__main__":
    main()
