"""Writes tests/golden/cond_integrand_L<L>.npz from the compiled reference's calculate_gamma_nm + calculate_conductivity_tensor
(tools/cond_fixture/cond_driver.f90; build it with tools/cond_fixture/build.sh after __graft_entry__.build()).

Synthetic inputs: an energy mesh built as energy%ene is (channels_ldos = 290: 300 points), moments with random orbital diagonals
(the only entries the reference reads) and zero elsewhere, two vectors, both cond_calctype values.  Stored: the inputs, gamma_nm at
full precision (every energy for small L, every 10th energy row otherwise, to stay well under 1 MB), and fort.123 of both runs.

    python tools/cond_fixture/make_fixture.py [--time L]     (--time: one run at channels_ldos = 2500, timed, no fixture)
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cond_reference import energy_mesh  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "cond_driver.x")
EMIN, EMAX, FERMI = -0.9, 0.7, 0.1


def synthetic_mu(L, nvec, seed):
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    decay = 1.0 / (1.0 + 0.3 * (n[:, None] + n[None, :]))
    mu = np.zeros((18, 18, L, L, nvec), np.complex128, order="F")
    for l in range(18):
        mu[l, l] = (rng.standard_normal((L, L, nvec)) + 1j * rng.standard_normal((L, L, nvec))) * decay[:, :, None]
    return mu


def run(L, nvec, nch, calctype, mu, ene, workdir):
    with open(os.path.join(workdir, "cond_in.bin"), "wb") as f:
        np.array([L, nvec, nch, calctype], np.int32).tofile(f)
        np.array([EMIN, EMAX, FERMI], np.float64).tofile(f)
        ene.astype(np.float64).tofile(f)
        np.asfortranarray(mu).ravel(order="F").tofile(f)
    t0 = time.perf_counter()
    subprocess.run([DRIVER], cwd=workdir, check=True, stdout=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    G = np.fromfile(os.path.join(workdir, "cond_gamma.bin"), np.complex128).reshape((nch + 10, L, L), order="F")
    f123 = np.loadtxt(os.path.join(workdir, "fort.123"))
    return G, f123, dt


def make(L, nvec=2, nch=290):
    ene = energy_mesh(EMIN, EMAX, nch)
    mu = synthetic_mu(L, nvec, 1000 + L)
    out = dict(cond_ll=L, nvec=nvec, channels_ldos=nch, energy_min=EMIN, energy_max=EMAX, fermi=FERMI, ene=ene,
               mu_diag=mu[np.arange(18), np.arange(18)])
    for calctype, name in ((1, "per_type"), (2, "random_vec")):
        with tempfile.TemporaryDirectory() as d:
            G, f123, _ = run(L, nvec, nch, calctype, mu, ene, d)
        out["fort123_" + name] = f123
    rows = np.arange(nch + 10) if L <= 8 else np.arange(0, nch + 10, 10)
    out["gamma_rows"] = rows
    out["gamma_nm"] = G[rows]
    path = os.path.join(ROOT, "tests", "golden", "cond_integrand_L%d.npz" % L)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def time_host(L, nvec, nch=2500):
    """Wall time of the reference's calculate_gamma_nm + calculate_conductivity_tensor (the driver's whole run, file writing and the
    Simpson integrations included) at channels_ldos = nch."""
    ene = energy_mesh(EMIN, EMAX, nch)
    mu = synthetic_mu(L, nvec, 7)
    with tempfile.TemporaryDirectory() as d:
        _, _, dt = run(L, nvec, nch, 2, mu, ene, d)
    print("host reference L=%d nvec=%d nE=%d: %.2f s on %d cores (OMP_NUM_THREADS=%s)" % (L, nvec, nch + 10, dt, os.cpu_count(),
                                                                                       os.environ.get("OMP_NUM_THREADS", "unset")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=0)
    ap.add_argument("--nvec", type=int, default=1)
    args = ap.parse_args()
    if args.time:
        time_host(args.time, args.nvec)
    else:
        for L in (7, 24):
            make(L)
