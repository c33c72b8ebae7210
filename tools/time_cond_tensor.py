"""Device time of rsrec_kubo_conductivity (the conductivity tail: k_cond_series + k_cond_tensor, kernels_cond.hpp) on the reference's
mesh, nen = 2510, nv1 = 2501, and -- with --dropin -- the tail's two regions of the zero-edit drop-in's timer report.

    python tools/time_cond_tensor.py [--nvec 1 3 8] [--reps 5] [--dropin] [--out profiles/cond_tensor_v1.json]

Per (nvec, per_vector): device ms of the call (rsrec_get_timing out[0]; the call's device work is its two kernels) over --reps runs after
one warm-up, as median, min and max, and the wall ms of the whole call from host arrays (transfers included).
--dropin: runs oracle/_ref/rslmto_dropin.x on the case Generated_conductivity_fccPt_spin twice, without and with RSREC_HOST_COND_TAIL=1,
and reads the seconds of the regions conductivity-tensor-gpu and conductivity-tensor-host from each run's timer report (the host
region is the parent commit's tail: simpson_f of math_mod, 38 x nen x (1 + ntype) calls)."""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASE = "Generated_conductivity_fccPt_spin"


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


def device_times(nvecs, reps):
    import torch
    torch.cuda.init()                                  # torch's HIP runtime before librsrec's
    torch.cuda.set_device(0)
    from cond_reference import energy_mesh
    from rslmtoasa_amd.conductivity import Conductivity
    from rslmtoasa_amd.recursion import Energy
    en = Energy(-0.8, 0.6)
    rec = BareHandle(en)
    cond = Conductivity(rec)
    ene = energy_mesh(en.energy_min, en.energy_max, 2500)
    rng = np.random.default_rng(1)
    rows = []
    for nvec in nvecs:
        z = np.asfortranarray(rng.standard_normal((18, ene.size, nvec)) + 1j * rng.standard_normal((18, ene.size, nvec)))
        for pv in (False, True):
            cond.tensor(z, ene, nv1=2501, per_vector=pv, series=True)      # warm-up: buffers, code objects
            dev, wall = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                cond.tensor(z, ene, nv1=2501, per_vector=pv, series=True)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(cond.timing()[0])
            row = dict(nen=int(ene.size), nv1=2501, nvec=nvec, per_vector=int(pv), columns=38 * (1 + (nvec if pv else 0)), reps=reps,
                       device_ms_median=round(float(np.median(dev)), 4), device_ms_min=round(min(dev), 4), device_ms_max=round(max(dev), 4),
                       wall_ms_median=round(float(np.median(wall)), 3), wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
    rec.close()
    return rows


def region_seconds(log, label):
    """Seconds of one region from g_timer's report.  A row of the report is the label (behind the tree's branch marks) and seven
    columns -- MEAN, MAX, MIN, TOTAL, TOTAL (%), NCALLS, TOTAL NCALLS -- with '-' where a column does not apply: TOTAL is the fourth."""
    head = re.search(r"(?m)^\s*CATEGORY\s+MEAN\s+MAX\s+MIN\s+TOTAL\s+TOTAL \(%\)\s+NCALLS\s+TOTAL NCALLS\s*$", log)
    if not head:
        raise RuntimeError("no TIMER REPORT with the expected columns in the log")
    for line in log[head.end():].splitlines():
        m = re.match(r"^\W*%s\*?\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$" % re.escape(label), line)
        if m:
            return float(m.group(4))
    raise RuntimeError("region %s is not in the timer report" % label)


def dropin_regions(keep_logs=None):
    from oracle.make_fixtures import patch_namelist
    from rslmtoasa_amd._proc import run_with_unlimited_stack
    from test_fortran_dropin import DROPIN, MANIFEST, SCF
    case = MANIFEST[CASE]
    out = {}
    for switch in (False, True):
        with tempfile.TemporaryDirectory() as d:
            work = os.path.join(d, "run")
            shutil.copytree(os.path.join(SCF, case["inputs"]), work)
            inp = os.path.join(work, "input.nml")
            with open(inp) as f:
                text = f.read()
            with open(inp, "w") as f:
                f.write(patch_namelist(text, case["patch"]))
            env = {"OMP_NUM_THREADS": "8"}
            if switch:
                env["RSREC_HOST_COND_TAIL"] = "1"
            r = run_with_unlimited_stack([DROPIN], cwd=work, env=env, timeout=1500, scrub=False)
            log = r.stdout + r.stderr
            assert r.returncode == 0, log[-3000:]
            if keep_logs:
                os.makedirs(keep_logs, exist_ok=True)
                with open(os.path.join(keep_logs, "dropin_%s.log" % ("host_tail" if switch else "gpu_tail")), "w") as f:
                    f.write(log)
            label = "conductivity-tensor-host" if switch else "conductivity-tensor-gpu"
            out[label + "_s"] = region_seconds(log, label)
            out["conductivity-integrand-gpu_s" + ("_host_tail_run" if switch else "")] = region_seconds(log, "conductivity-integrand-gpu")
    out["case"] = CASE
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nvec", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dropin", action="store_true")
    ap.add_argument("--keep-logs", default=None, help="directory for the two drop-in logs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = dict(tool="tools/time_cond_tensor.py", device=device_times(args.nvec, args.reps))

    def write():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    write()                                            # (the device times stay if a drop-in run fails)
    if args.dropin:
        result["dropin"] = dropin_regions(args.keep_logs)
        write()


if __name__ == "__main__":
    main()
