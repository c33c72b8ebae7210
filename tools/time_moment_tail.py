"""Device time of rsrec_spectra_integrals (the integrals behind the SCF spectra: k_moment_series, k_moment_prefix, k_moment_cum,
k_moment_fermi of kernels_moments.hpp) on the reference's mesh, nen = 2510, nv1 = 2501, and -- with --dropin -- the two regions of the
tail in the timer reports of the Fortran SCF driver.

    python tools/time_moment_tail.py [--sites 1 64] [--reps 5] [--dropin] [--out profiles/moment_tail.json]

Per (sites, nop, nser, nen): device ms of the call (rsrec_get_timing out[0]: its kernels, without the transfers) over --reps runs after one
warm-up, as median, min and max, and the wall ms of the whole call from and to host arrays (the image goes up, mom and cum come back).
Rows: the call of the SCF moment stage (the 15 rows as they are), the quadrupoles' call (6 rows), a 12-series table over the 15 rows, and
the 15-row call on half and on twice the mesh -- the cumulative integrals are O(nen) per series, so the device time should follow nen.
--dropin: runs oracle/_ref/rslmto_gpu.x on the case Example_bulk_bccFe_nsp4_block (one site, channels_ldos = 2500, one SCF step) with
RSREC_DEFER_G0=1, three times per route, alternating: the device tail (region moment-integrals-gpu) and RSREC_HOST_MOMENT_TAIL=1 (region
moment-integrals-host: the reference's simpson_m / simpson_f loops, restated in fortran/bands_gpu.f90)."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASE = "Example_bulk_bccFe_nsp4_block"


class BareHandle:
    """A handle with no lattice and no Hamiltonian: the call needs neither when the image is passed in."""

    def __init__(self):
        from rslmtoasa_amd import _lib
        from rslmtoasa_amd.recursion import Recursion
        self._L, self._h = _lib.lib(), C.c_void_p()
        self._check, self.timing = Recursion._check.__get__(self), Recursion.timing.__get__(self)
        self._check(self._L.rsrec_create(C.byref(self._h), 0))

    def close(self):
        self._L.rsrec_destroy(self._h)


def device_times(sites, reps):
    from rslmtoasa_amd import bands
    from rslmtoasa_amd.green import Green
    rec = BareHandle()
    rng = np.random.default_rng(1)
    rows = []
    for ns in sites:
        for what, nop, tab, nen in (("scf rows", 15, False, 2510), ("quadrupole rows", 6, False, 2510), ("series table", 15, True, 2510),
                                    ("scf rows, nen / 2", 15, False, 1255), ("scf rows, 2 nen", 15, False, 5020)):
            ene = -1.2 + (2.0 / nen) * np.arange(nen)
            nv1, npts = nen - 9, (2 * nen) // 3 | 1
            spec = np.asfortranarray(rng.standard_normal((nop, nen, ns)))
            comb = None
            if tab:
                mom = rng.standard_normal((3, ns))
                comb = bands.series_table(mom / np.linalg.norm(mom, axis=0))[0]
            gr = Green(rec, ene)
            args = (nv1, npts, ene[1] - ene[0], ene[npts - 1], ene[npts - 1] + 0.3 * (ene[1] - ene[0]))
            gr.spectra_integrals(*args, spec=spec, comb=comb)           # warm-up: buffers, code objects
            dev, wall = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                mom_, cum_ = gr.spectra_integrals(*args, spec=spec, comb=comb)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(rec.timing()["total_ms"])
            row = dict(call=what, sites=ns, nop=nop, nser=int(cum_.shape[0]), nen=nen, nv1=nv1, reps=reps,
                       device_ms_median=round(float(np.median(dev)), 4), device_ms_min=round(min(dev), 4), device_ms_max=round(max(dev), 4),
                       wall_ms_median=round(float(np.median(wall)), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                       checksum=float(np.abs(cum_).sum() + np.abs(mom_).sum()))
            print(json.dumps(row), flush=True)
            rows.append(row)
    rec.close()
    return rows


def dropin_regions(runs, keep_logs=None):
    from oracle.make_fixtures import patch_namelist
    from rslmtoasa_amd._proc import run_with_unlimited_stack
    from test_fortran_dropin import EXE, MANIFEST, SCF
    from time_cond_tensor import region_seconds
    case = MANIFEST[CASE]
    out = {"case": CASE, "program": os.path.relpath(EXE, ROOT), "moment-integrals-gpu_s": [], "moment-integrals-host_s": [], "spectra-gpu_s": []}
    for k in range(2 * runs):                              # alternating: device tail, host tail, device tail, ...
        host = k % 2 == 1
        with tempfile.TemporaryDirectory() as d:
            work = os.path.join(d, "run")
            shutil.copytree(os.path.join(SCF, case["inputs"]), work)
            inp = os.path.join(work, "input.nml")
            with open(inp) as f:
                text = f.read()
            with open(inp, "w") as f:
                f.write(patch_namelist(text, case["patch"]))
            env = {"OMP_NUM_THREADS": "8", "RSREC_DEFER_G0": "1"}
            if host:
                env["RSREC_HOST_MOMENT_TAIL"] = "1"
            r = run_with_unlimited_stack([EXE], cwd=work, env=env, timeout=900, scrub=False)
            log = r.stdout + r.stderr
            assert r.returncode == 0, log[-3000:]
            if keep_logs:
                os.makedirs(keep_logs, exist_ok=True)
                with open(os.path.join(keep_logs, "scf_%s_%d.log" % ("host_tail" if host else "gpu_tail", k // 2)), "w") as f:
                    f.write(log)
            label = "moment-integrals-host" if host else "moment-integrals-gpu"
            out[label + "_s"].append(region_seconds(log, label))
            if not host:
                out["spectra-gpu_s"].append(region_seconds(log, "spectra-gpu"))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dropin", action="store_true")
    ap.add_argument("--runs", type=int, default=3, help="drop-in runs per route")
    ap.add_argument("--keep-logs", default=None, help="directory for the drop-in logs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    result = dict(tool="tools/time_moment_tail.py", device=device_times(args.sites, args.reps))

    def write():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    write()                                            # (the device times stay if a drop-in run fails)
    if args.dropin:
        result["dropin"] = dropin_regions(args.runs, args.keep_logs)
        write()


if __name__ == "__main__":
    main()
