"""Device time of rsrec_chebyshev_evolve (kernels_evolve.hpp), one cell per process.

    python tools/time_evolve.py --cell 22 [--vectors 1 4] [--atau 10 25] [--orders 1 4 16] [--mom 50 500] [--rounds 3]
                                [--host-route] [--out profiles/evolve_v1.json] [--append]

Cell: the periodic bcc Fe supercell n^3 (22: 10 648 atoms, 46: 97 336) with the blocks of tests/golden/bccFe_nsp2_block.npz, D from
``position_commutator`` along x, random-phase vectors over all atoms, w = ``evolution_weights`` at korder = a tau + 40.
Step rows, per (vectors, a tau, evolve_orders), mom = 0, one record after two steps, after one warm-up call --rounds calls: device ms per
step (rsrec_get_timing out[0] / steps), ms per step in the H and D launches (out[1]) and in the step passes (out[23]), the passes' share
of the step, and the TB/s of the bytes the passes move: per step and vector, in block streams of kk * 5 184 B,
    fused (1):    6 + 8 (korder - 1)                      (order 0: x, y in and out of both chains; then p: x, y, y; g: x, x, dp, y, y)
    batched (P):  3 (korder - 1) + 2 (korder + 2 passes)  (source: x, x, dp of g; accumulation: every order once, y in and out per pass)
each as min and max over the rounds.  Beside them, in the same process, k_shot_accum of rsrec_kubo_single_shot (ne = 2, shot_orders = 16,
cond_ll = korder, v_out = v_b = D): ms per chain and order and TB/s of its (cond_ll + 4 passes) streams per chain.
Record rows, per (vectors, mom): one record after one step with only m_diag asked for: ms in the record stage (out[24]: one seed
projection, mom - 1 H launches, the Grams).
--host-route (the small cell): one step of one vector without the call -- rsrec_apply_operator per product through host arrays
(``ham_vec_matmul``, ``velo_vec_matmul``) and the sums in numpy -- as wall-clock ms per step.
Every row is printed as it is measured and the file is rewritten after every row.  No pass/fail ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def span(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=22)
    ap.add_argument("--vectors", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--atau", type=float, nargs="+", default=[10.0, 25.0])
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--mom", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-route", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds (one process per cell)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    from helpers import load_golden
    from rslmtoasa_amd.lattice import bcc_supercell
    from rslmtoasa_amd.recursion import (Control, Energy, Hamiltonian, Lattice, Recursion, chebyshev_scaling, evolution_weights,
                                         position_commutator, _ptr)
    z = load_golden("bccFe_nsp2_block")
    n = args.cell
    nn = bcc_supercell((n, n, n), z["slot_vec"])
    kk = nn.shape[0]
    en = Energy(float(z["emin"]), float(z["emax"]))
    rec = Recursion(Hamiltonian(ee=z["ee"], lsham=z["lsham"], hoh=False), Lattice(nn=nn, iz=np.ones(kk, np.int32), irec=np.array([1], np.int32), nmax=0, ntype=1),
                    Control(lld=21, nsp=2), en, device=0)
    a, b = chebyshev_scaling(en.energy_min, en.energy_max)
    d_op = position_commutator(z["ee"], z["slot_vec"], (1.0, 0.0, 0.0))
    result = dict(tool="tools/time_evolve.py", device=torch.cuda.get_device_name(0), rounds=args.rounds, steps=[], records=[], host_route=[])
    if args.append and args.out and os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
        for k in ("steps", "records", "host_route"):
            result[k] = old[k]

    def write():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

    rng = np.random.default_rng(7)
    stream = kk * 5184.0
    for nvec in args.vectors:
        seeds = np.tile(np.arange(1, kk + 1, dtype=np.int32), (nvec, 1))
        coefs = np.exp(2j * np.pi * rng.random((nvec, kk))) / np.sqrt(kk)
        for atau in args.atau:
            korder = int(round(atau)) + 40
            w = evolution_weights(atau / a, korder, a, b)
            shot_w = np.asfortranarray(np.repeat(w[:, None], 2, axis=1))
            ts = []
            for r in range(args.rounds + 1):
                rec.kubo_single_shot(d_op, d_op, shot_w, shot_w, seeds=seeds, coefs=coefs)
                if r:
                    ts.append(rec.timing()["shot_accum_ms"])
            shot_streams = 2 * nvec * (korder + 4.0 * -(-korder // 16))
            shot = dict(ms_per_chain_order=span([x / (2 * nvec * korder) for x in ts]), tb_per_s=span([shot_streams * stream * 1e-12 / (x * 1e-3) for x in ts]))
            for P in args.orders:
                rec.set_option("evolve_orders", P)
                t = {k: [] for k in ("total_ms", "hop_ms", "evolve_pass_ms")}
                steps = 2
                for r in range(args.rounds + 1):
                    rec.evolve(d_op, w, 1, stride=steps, mom=0, seeds=seeds, coefs=coefs)
                    tm = rec.timing()
                    if r:                              # (round 0: warm-up -- buffers, code objects)
                        for k in t:
                            t[k].append(tm[k] / steps)
                rec.set_option("evolve_orders", 0)
                streams = nvec * (6.0 + 8.0 * (korder - 1) if P == 1 else 3.0 * (korder - 1) + 2.0 * (korder + 2.0 * -(-korder // P)))
                row = dict(cell=n, atoms=kk, vectors=nvec, a_tau=atau, korder=korder, evolve_orders=P, form="fused" if P == 1 else "batched",
                           hop_launches_per_step=int(tm["hop_launches"]) // steps, ms_per_step=span(t["total_ms"]), spmm_ms_per_step=span(t["hop_ms"]),
                           pass_ms_per_step=span(t["evolve_pass_ms"]), pass_share=span([p / q for p, q in zip(t["evolve_pass_ms"], t["total_ms"])]),
                           pass_gb_per_step=round(streams * stream * 1e-9, 3),
                           pass_tb_per_s=span([streams * stream * 1e-12 / (x * 1e-3) for x in t["evolve_pass_ms"]]),
                           pass_ms_per_chain_order=span([x / (2 * nvec * korder) for x in t["evolve_pass_ms"]]), k_shot_accum=shot)
                print(json.dumps(row), flush=True)
                result["steps"].append(row)
                write()
        korder = int(round(args.atau[0])) + 40
        w = evolution_weights(args.atau[0] / a, korder, a, b)
        for mom in args.mom:
            t = []
            for r in range(args.rounds + 1):
                d_op_f = np.asfortranarray(d_op)
                out = np.zeros((18, mom, 1, nvec), np.complex128, order="F")
                rec._check(rec._L.rsrec_chebyshev_evolve(rec._h, nvec, kk, _ptr(seeds), _ptr(coefs), a, b, _ptr(d_op_f), None, korder, _ptr(w), 1, 1, mom,
                                                         None, None, None, None, _ptr(out)))
                tm = rec.timing()
                if r:
                    t.append(tm["evolve_record_ms"])
            row = dict(cell=n, atoms=kk, vectors=nvec, mom=mom, korder=korder, ms_per_record=span(t), ms_per_record_and_order=span([x / mom for x in t]))
            print(json.dumps(row), flush=True)
            result["records"].append(row)
            write()
    if args.host_route:
        korder = int(round(args.atau[0])) + 40
        w = evolution_weights(args.atau[0] / a, korder, a, b)
        psi = np.zeros((18, 18, kk), np.complex128, order="F")
        psi[np.arange(18), np.arange(18), :] = (np.exp(2j * np.pi * rng.random(kk)) / np.sqrt(kk))[None, :]
        t = []
        for r in range(args.rounds):
            t0 = time.perf_counter()
            p0, g0 = psi, np.zeros_like(psi)
            p1, g1 = rec.ham_vec_matmul(p0, a, b), rec.ham_vec_matmul(g0, a, b) + rec.velo_vec_matmul(d_op, p0) / a
            ps, cs = w[0] * p0 + w[1] * p1, w[0] * g0 + w[1] * g1
            for k in range(2, korder):
                p2 = 2.0 * rec.ham_vec_matmul(p1, a, b) - p0
                g2 = 2.0 * rec.ham_vec_matmul(g1, a, b) - g0 + (2.0 / a) * rec.velo_vec_matmul(d_op, p1)
                ps += w[k] * p2
                cs += w[k] * g2
                p0, p1, g0, g1 = p1, p2, g1, g2
            t.append((time.perf_counter() - t0) * 1e3)
        row = dict(cell=n, atoms=kk, vectors=1, korder=korder, route="rsrec_apply_operator per product through host arrays, sums in numpy", wall_ms_per_step=span(t))
        print(json.dumps(row), flush=True)
        result["host_route"].append(row)
        write()
    rec.close()


if __name__ == "__main__":
    main()
