"""Device time of the Chebyshev moments from whole-lattice seeds (rsrec_chebyshev_lattice), and the routes without the call, in ONE
process on one handle per cell.

    python tools/time_lattice.py [--lld 50] [--rounds 3] [--cells 22x22x22 46x46x46] [--nk 1 8 64] [--ngroup 1 4 16] [--out profiles/lattice_v1.json]

Per cell, nk plane-wave chains and ngroup (every atom in a group, groups by atom number modulo ngroup): `--rounds` calls without a
download after one warm-up call, reported as min-max.  rsrec_get_timing out[0] (device ms), out[1] (ms in the H|psi> launches), out[5] (ms
in the projection kernels).  The projection must read 5 184 B per grouped atom, order and chain; that over out[5] is its rate, quoted
next to the 6.08 TB/s k_mfma_adot reaches on two streams (profiles/).  A cell whose call fails for want of memory is recorded as such.
The routes without the call:
  4x4x8 alloy, 64 k-points, lld 5, two groups by type: rsrec_chebyshev_bloch with all 128 sources, download and host mean, wall time,
      against one bloch_average call (wall time, download included);
  22^3, 3 random vectors, 102 moments: rsrec_kubo_moments_diag with identity operators and cond_ll = 102, its m = 1 column, against
      cell_moments at lld 50 (wall time and device ms of both).
One JSON line per row on stdout; the whole table goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ADOT_TB_S = 6.08


def spread(v):
    return [min(v), max(v)]


def grid_rows(args, rng):
    from bloch_reference import commensurate_k
    from helpers import objects_from, supercell_problem
    from rslmtoasa_amd import _lib
    from rslmtoasa_amd.lattice import supercell_positions
    from rslmtoasa_amd.recursion import Recursion
    rows = []
    for cell in args.cells:
        dims = tuple(int(v) for v in cell.split("x"))
        p = supercell_problem(dims)
        kk = p["nn"].shape[0]
        rec = Recursion(*objects_from(p, [1], args.lld, emin=-3.0, emax=1.8))
        cr = supercell_positions(dims)
        for nk in args.nk:
            k = commensurate_k(dims, rng.integers(0, dims[0], (nk, 3)))
            for ng in args.ngroup:
                group = (np.arange(kk) % ng + 1).astype(np.int32)
                row = dict(cell=cell, atoms=kk, lld=args.lld, nk=nk, ngroup=ng, rounds=args.rounds)
                t = {"total_ms": [], "hop_ms": [], "rest_ms": []}
                try:
                    for r in range(args.rounds + 1):                 # the first call warms up: buffers, the list of all atoms, code objects
                        rec.bloch_average(k, cr, group=group, download=False)
                        tm = rec.timing()
                        if r:
                            for key in t:
                                t[key].append(tm[key])
                except _lib.RsrecError as e:
                    row["failed"] = str(e)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    continue
                nbytes = 5184.0 * kk * (2 * args.lld + 2) * nk
                rate = [nbytes / (1e9 * m) for m in t["rest_ms"]]
                row.update(device_ms=spread(t["total_ms"]), hop_ms=spread(t["hop_ms"]), projection_ms=spread(t["rest_ms"]),
                           projection_tb_per_s=spread(rate), projection_over_adot_rate=spread([v / ADOT_TB_S for v in rate]),
                           projection_over_hop=spread([m / h for m, h in zip(t["rest_ms"], t["hop_ms"])]))
                rows.append(row)
                print(json.dumps(row), flush=True)
        rec.close()
    return rows


def alloy_route(args):
    """Unfolded bands of the alloy: kk chains and a host mean against one chain per k-point."""
    from bloch_reference import commensurate_k
    from helpers import objects_from
    from lattice_seed_reference import ALLOY_LLD, alloy_case
    from rslmtoasa_amd.recursion import Recursion
    dims, p, _, _, _, emin, emax, cr, cvec = alloy_case(False)
    kk = p["nn"].shape[0]
    rec = Recursion(*objects_from(p, [1], ALLOY_LLD, emin=emin, emax=emax))
    k = commensurate_k(dims, np.random.default_rng(2).integers(0, 8, (64, 3)))
    group = p["iz"].astype(np.int32)

    def today():
        return rec.chebyshev_bloch(np.arange(1, kk + 1), k, cr, cell=cvec, group=group).mean(axis=5).transpose(0, 1, 2, 4, 3)

    def lattice():
        return rec.bloch_average(k, cr, group=group)
    a, b = today(), lattice()
    wall = {"bloch_all_sources_and_mean": [], "bloch_average": []}
    for _ in range(args.rounds):
        for name, fn in (("bloch_all_sources_and_mean", today), ("bloch_average", lattice)):
            t0 = time.perf_counter()
            fn()
            wall[name].append(1e3 * (time.perf_counter() - t0))
    rec.close()
    return dict(route="alloy 4x4x8, 64 k-points, 2 groups", atoms=kk, lld=ALLOY_LLD, rounds=args.rounds,
                deviation=float(np.abs(a - b).max() / np.abs(a).max()), wall_ms={n: spread(v) for n, v in wall.items()})


def cell_dos_route(args, rng):
    """Cell DOS moments on random vectors: the Kubo call with identity operators against cell_moments."""
    from helpers import objects_from, supercell_problem
    from rslmtoasa_amd.recursion import Recursion
    dims, lld = (22, 22, 22), 50
    p = supercell_problem(dims)
    kk = p["nn"].shape[0]
    rec = Recursion(*objects_from(p, [1], lld, emin=-3.0, emax=1.8))
    r = rng.random((kk, 3))
    ident = np.zeros(p["ee"].shape, np.complex128, order="F")
    ident[:, :, 0, :] = np.eye(18)[:, :, None]
    coefs = np.ascontiguousarray((np.exp(2j * np.pi * r) / float(np.sqrt(np.float32(kk)))).T)
    seeds = np.tile(np.arange(1, kk + 1, dtype=np.int32), (3, 1))

    def today():
        return rec.compute_moments_stochastic(ident, ident, 2 * lld + 2, seeds=seeds, coefs=coefs, diag=True)[:, :, 0, :], rec.timing()["total_ms"]

    def lattice():
        return rec.cell_moments(r), rec.timing()["total_ms"]
    (a, _), (b, _) = today(), lattice()
    dev = float(np.abs(np.einsum("llnv->lnv", b[:, :, :, 0, :]) - a).max() / np.abs(a).max())
    wall = {"kubo_diag_identity": [], "cell_moments": []}
    device = {"kubo_diag_identity": [], "cell_moments": []}
    for _ in range(args.rounds):
        for name, fn in (("kubo_diag_identity", today), ("cell_moments", lattice)):
            t0 = time.perf_counter()
            _, ms = fn()
            wall[name].append(1e3 * (time.perf_counter() - t0))
            device[name].append(ms)
    rec.close()
    return dict(route="cell DOS 22x22x22, 3 random vectors, 102 moments", atoms=kk, rounds=args.rounds, deviation=dev,
                wall_ms={n: spread(v) for n, v in wall.items()}, device_ms={n: spread(v) for n, v in device.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lld", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", nargs="*", default=["22x22x22", "46x46x46"])
    ap.add_argument("--nk", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--ngroup", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_v1.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    rows = grid_rows(args, rng)
    for row in (alloy_route(args), cell_dos_route(args, rng)):
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/time_lattice.py", adot_tb_per_s=ADOT_TB_S, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
