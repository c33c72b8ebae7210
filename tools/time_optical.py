"""Device time of rsrec_kubo_optical (sigma(omega) from the orbital-diagonal Kubo moments, kernels_optical.hpp) on the reference's mesh,
and, in the same process on the same GPU, the route without the call: torch.matmul on complex128 for D mu D^T per orbital plus the
weighted diagonal sums.

    python tools/time_optical.py [--L 50 500] [--nset 1 8] [--nfermi 1 4] [--rounds 3] [--out profiles/optical_v1.json]

Per (L, nset, nfermi) at nen = 2510, nw = 2509, T = 0, moments resident in GPU memory for both routes, --rounds runs after one warm-up:
  device_ms      device ms of the call (rsrec_get_timing out[0]), min and max
  kernels_ms     ms in its kernels (out[5])
  tf_nominal     18 nset (4 nen L^2 + 4 L sum_{k<=nw} (nen - k)) flop -- every pair i < j <= i + nw -- per kernel second, as TF and as a
                 fraction of the 78.6 TF FP64 matrix peak.  At T = 0 the tiles without a non-zero weight are skipped, so
  tf_executed    counts stage 1 and the 64 x 32 tiles that were really formed (live_tiles of tiles_in_band) instead
  torch_ms       the torch route, by torch.cuda events around all sets: per (set, orbital) J = (D mu) D^T, per Fermi level the weights
                 times J and the sums along its diagonals (one strided view of a zero-padded copy, summed over rows)
  max_rel_diff   largest |call - torch| per orbital relative to the orbital's largest magnitude (the two routes on the same numbers)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_TF = 78.6


class BareHandle:
    """A handle with no lattice and no Hamiltonian: the call needs neither."""

    def __init__(self, en):
        from rslmtoasa_amd import _lib
        from rslmtoasa_amd.recursion import Recursion
        self.en, self._L, self._h = en, _lib.lib(), C.c_void_p()
        self._check, self.timing = Recursion._check.__get__(self), Recursion.timing.__get__(self)
        self._check(self._L.rsrec_create(C.byref(self._h), 0))

    def close(self):
        self._L.rsrec_destroy(self._h)


def torch_route(mu, D, F, nw, a):
    """opt (nset, nf, nw, 18) complex on the GPU from mu (nset, L, L, 18) [the Fortran (18, L, L, nset)], D (nen, L), F (nf, nen)."""
    import torch
    nset, nen, nf = mu.shape[0], D.shape[0], F.shape[0]
    Dc = D.to(torch.complex128)
    out = torch.empty((nset, nf, nw, 18), dtype=torch.complex128, device=mu.device)
    Z = torch.zeros((nen, 2 * nen), dtype=torch.complex128, device=mu.device)
    diag = Z.as_strided((nen, nen), (2 * nen + 1, 1))                # diag[i, k] = Z[i, i + k]: J(i, i + k), zero past the mesh
    scale = (np.pi / a ** 2) / torch.arange(1, nw + 1, device=mu.device, dtype=torch.float64)
    W = [(F[f][:, None] - F[f][None, :]).to(torch.complex128) for f in range(nf)]
    for s in range(nset):
        for l in range(18):
            M = mu[s, :, :, l].transpose(0, 1)                       # M(n, m)
            J = torch.matmul(torch.matmul(Dc, M), Dc.transpose(0, 1))
            for f in range(nf):
                torch.mul(W[f], J, out=Z[:, :nen])
                out[s, f, :, l] = diag.sum(dim=0)[1:nw + 1] * scale
    return out


def measure(cond, L, nset, nf, rounds):
    import torch
    import optical_reference as O
    from cond_reference import energy_mesh
    en = cond.en
    ene = energy_mesh(en.energy_min, en.energy_max, 2500)
    nen, nw = ene.size, ene.size - 1
    fermi = np.array([0.5 * (ene[1250] + ene[1251]), ene[900], 0.5 * (ene[1700] + ene[1701]), ene[400]])[:nf]
    g = torch.Generator(device="cuda").manual_seed(100 * L + nset)
    n = torch.arange(L, device="cuda", dtype=torch.float64)
    decay = 1.0 / (1.0 + 0.05 * (n[:, None] + n[None, :]))
    mu = torch.randn((nset, L, L, 18), dtype=torch.complex128, device="cuda", generator=g) * decay[None, :, :, None]
    a = O.scaled_axis(ene, en.energy_min, en.energy_max)[1]
    D = torch.from_numpy(O.basis_table(ene, en.energy_min, en.energy_max, L)).cuda()
    Fh = O.fermi_table(ene, en.energy_min, en.energy_max, fermi)
    F = torch.from_numpy(Fh).cuda()
    in_band = [(i0, j0) for i0 in range(0, nen, O.TILE_I) for j0 in range(0, nen, O.TILE_J)
               if min(j0 + O.TILE_J, nen) - 1 > i0 and j0 - min(i0 + O.TILE_I - 1, nen - 1) <= nw]
    live = sum(O.tile_is_live(i0, j0, nen, nw, Fh) for i0, j0 in in_band)
    nominal = 18.0 * nset * (4.0 * nen * L * L + 4.0 * L * sum(nen - k for k in range(1, nw + 1)))
    executed = 18.0 * nset * (4.0 * nen * L * L + 4.0 * L * live * O.TILE_I * O.TILE_J)
    dev, ker, tms = [], [], []
    got = ref = None
    for r in range(rounds + 1):                                        # round 0: warm-up (buffers, code objects, rocBLAS kernels)
        got = cond.optical(mu, ene, fermi)
        t = cond.timing()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ref = torch_route(mu, D, F, nw, a)
        e1.record()
        torch.cuda.synchronize()
        if r:
            dev.append(t[0]); ker.append(t[1]); tms.append(e0.elapsed_time(e1))
    ref = ref.cpu().numpy().transpose(3, 2, 1, 0)                      # (18, nw, nf, nset)
    diff = max(np.abs(got[l] - ref[l]).max() / np.abs(ref[l]).max() for l in range(18))
    tf = lambda flop, ms: flop / (ms * 1e-3) / 1e12   # noqa: E731
    row = dict(L=L, nen=nen, nw=nw, nset=nset, nfermi=nf, rounds=rounds,
               device_ms_min=round(min(dev), 3), device_ms_max=round(max(dev), 3), kernels_ms_min=round(min(ker), 3), kernels_ms_max=round(max(ker), 3),
               tiles_in_band=len(in_band), live_tiles=int(live),
               tf_nominal_min=round(tf(nominal, max(ker)), 2), tf_nominal_max=round(tf(nominal, min(ker)), 2),
               tf_nominal_of_peak_min=round(tf(nominal, max(ker)) / PEAK_TF, 3), tf_nominal_of_peak_max=round(tf(nominal, min(ker)) / PEAK_TF, 3),
               tf_executed_min=round(tf(executed, max(ker)), 2), tf_executed_max=round(tf(executed, min(ker)), 2),
               tf_executed_of_peak_min=round(tf(executed, max(ker)) / PEAK_TF, 3), tf_executed_of_peak_max=round(tf(executed, min(ker)) / PEAK_TF, 3),
               torch_ms_min=round(min(tms), 3), torch_ms_max=round(max(tms), 3),
               torch_over_call_min=round(min(tms) / max(dev), 2), torch_over_call_max=round(max(tms) / min(dev), 2),
               max_rel_diff=float("%.2e" % diff))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--nset", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--nfermi", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    from rslmtoasa_amd.conductivity import Conductivity
    from rslmtoasa_amd.recursion import Energy
    rec = BareHandle(Energy(-0.8, 0.6))
    cond = Conductivity(rec)
    result = dict(tool="tools/time_optical.py", device=torch.cuda.get_device_name(0), peak_tf=PEAK_TF, rows=[])
    for L in args.L:
        for nset in args.nset:
            for nf in args.nfermi:
                result["rows"].append(measure(cond, L, nset, nf, args.rounds))
                if args.out:
                    with open(args.out, "w") as f:
                        json.dump(result, f, indent=1)
                        f.write("\n")
    rec.close()


if __name__ == "__main__":
    main()
