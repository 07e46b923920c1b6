#!/usr/bin/env python
"""Times supervised descent training on the device on seeded synthetic images.

  python tools/sdm_train_probe.py [--images 811] [--samples 11] [--landmarks 20] [--cells 3 --cell-size 12 --bins 4]
                                  [--reps 5] [--warmup 1] [--numpy] [--out sdm_train_probe.json]

One cascade step per call of fd_sdm_train (the step is what repeats; S steps cost S times as much), kernel timing on: the phases
{descriptors, gram, norm, cholesky, substitution, update} come from HIP events on the context's stream
(fd_sdm_train_last_phase_ms), the wall time from the host clock around the call (uploads, the one wait and the read-backs
included).  Medians, minima and maxima over --reps after --warmup calls.  --numpy: the same regression in numpy / LAPACK float64
on this machine's CPU (A^T A, Cholesky, two triangular solves), with the thread count the BLAS reports.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=811)
    ap.add_argument("--samples", type=int, default=11)
    ap.add_argument("--landmarks", type=int, default=20)
    ap.add_argument("--cells", type=int, default=3)
    ap.add_argument("--cell-size", type=int, default=12)
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from featuredetection_amd import capi
    ctx = capi.Context(0)
    ctx.set_kernel_timing(True)
    rng = np.random.default_rng(1)
    L, K, n, W = a.landmarks, a.samples, a.images, a.size
    half = a.cells * (a.cell_size // 2)
    # seeded images: block noise; landmarks anywhere the window fits; start shapes a few pixels off
    imgs = np.clip(128 + 40 * np.kron(rng.standard_normal((n, W // 4, W // 4)), np.ones((4, 4))), 0, 255).astype(np.uint8)
    gt = rng.uniform(half + 16, W - half - 17, (n, 2 * L)).astype(np.float32)
    gt_rows = np.repeat(gt, K, axis=0)
    x0 = (gt_rows + np.clip(rng.normal(0, 3.0, gt_rows.shape), -12, 12)).astype(np.float32)   # every window stays inside its image
    dp = [(a.cells, a.cell_size, a.bins)]
    nbytes, dim = capi.sdm_train_limits(L, dp, n * K)
    rec = dict(images=n, samples=K, rows=n * K, landmarks=L, dim=dim, device_bytes=nbytes, reps=a.reps, warmup=a.warmup)
    print("M = %d rows, D = %d, %.2f GB resident" % (n * K, dim, nbytes / 1e9), flush=True)
    walls, phases = [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        out = capi.sdm_train(ctx, [imgs], K, x0, gt_rows, dp, 1, capi.SDM_REG_AUTOMATIC, 0.5, False)
        t1 = time.perf_counter()
        ph = capi.sdm_train_last_phase_ms(ctx)
        print("call %d: wall %.1f ms, phases %s" % (r, 1e3 * (t1 - t0), {k: round(v, 3) for k, v in ph.items()}), flush=True)
        if r >= a.warmup:
            walls.append(1e3 * (t1 - t0))
            phases.append(ph)
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    rec["wall_ms"] = stat(walls)
    rec["phase_ms"] = {k: stat([p[k] for p in phases]) for k in phases[0]}
    rec["lambda"] = out["info"][1]["lam"]
    rec["err_l1"] = [i["err_l1"] for i in out["info"]]
    if a.numpy:
        # a system of the same size on the CPU (seeded normal A: its values do not change the operation count), LAPACK float64
        try:
            from threadpoolctl import threadpool_info
            rec["numpy_threads"] = [(p.get("internal_api"), p.get("num_threads")) for p in threadpool_info()]
        except Exception:
            rec["numpy_threads"] = "threadpoolctl not installed; OMP_NUM_THREADS=%s" % os.environ.get("OMP_NUM_THREADS")
        A = rng.standard_normal((n * K, dim)).astype(np.float32)
        b = (gt_rows - x0).astype(np.float32)
        ts = []
        for r in range(2):
            t0 = time.perf_counter()
            A64 = A.astype(np.float64)
            AtA, Atb = A64.T @ A64, A64.T @ b.astype(np.float64)
            lam = 0.5 * np.linalg.norm(AtA) / A.shape[0]
            AtA[np.diag_indices(dim)] += lam
            Lc = np.linalg.cholesky(AtA)
            R = np.linalg.solve(Lc.T, np.linalg.solve(Lc, Atb))
            ts.append(1e3 * (time.perf_counter() - t0))
            print("numpy float64 regression: %.1f ms" % ts[-1], flush=True)
        rec["numpy_regression_ms"] = ts
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
