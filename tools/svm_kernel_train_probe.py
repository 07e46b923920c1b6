"""Kernel SVM training on the device (fd_kernel_svm_gram, fd_kernel_svm_train, fd_kernel_svm_train_model): ms per call and
microseconds per SMO iteration for the RBF, polynomial and histogram-intersection kernels, next to libsvm's svm_train on this
machine's CPU for the same problems.

  python tools/svm_kernel_train_probe.py
  python tools/svm_kernel_train_probe.py --reps 30

Shapes: 20 + 100 x 455 (the tracker's default stores, 13 channels; Q in LDS) and 20 + 300 x 1085 (31 channels; Q in memory).  Every
call ends in a synchronise of its own and is timed with the host clock around it, after warm-up calls; medians with p10 / p90 are
reported.  The time per iteration is the slope between a run stopped at half the iterations (max_iterations) and the full run, so
that the Gram, the copies and the launches cancel.  libsvm (the compiled reference unit, oracle/_ref) is timed around svm_train
alone, single runs repeated, where that unit is present; it is the baseline -- the parent commit trains no kernel SVM.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # noqa: F401  before libfd_hip.so: the wheel brings its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((20, 100, 455), (20, 300, 1085))


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_p10=float(np.percentile(ms, 10)), ms_p90=float(np.percentile(ms, 90)))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()   # ends in a device synchronise
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import svm_kernel_train_model as K
    import svm_train_model as M
    from featuredetection_amd import capi
    from oracle import pyoracle as O
    ctx = capi.Context(0)
    ref = O.ref()
    results = []
    for n_pos, n_neg, d in SHAPES:
        x = M.ehog_like(n_pos, n_neg, d, seed=100 + n_neg)
        for kernel in (K.KERNELS[0], K.KERNELS[2], K.KERNELS[4]):
            sv_index, coef, sv, bias, alpha, info = capi.kernel_svm_train(ctx, x, n_pos, kernel)
            half = max(1, info["iterations"] // 2)
            full = timed(lambda: capi.kernel_svm_train(ctx, x, n_pos, kernel), a.reps)
            part = timed(lambda: capi.kernel_svm_train(ctx, x, n_pos, kernel, max_iterations=half), a.reps)
            gram = timed(lambda: capi.kernel_svm_gram(ctx, x, n_pos, kernel), a.reps)
            model = timed(lambda: capi.kernel_svm_train_model(ctx, x, n_pos, kernel)[0].close(), a.reps)
            q_in_lds, large, _ = capi.kernel_svm_train_limits(n_pos, n_neg, d)
            r = dict(kernel=K.kernel_id(kernel), n_pos=n_pos, n_neg=n_neg, d=d, q_in_lds=q_in_lds, large=large, info=info, train=full,
                     train_half_iterations=part, gram_call=gram, train_model=model,
                     us_per_iteration=(full["ms_median"] - part["ms_median"]) * 1e3 / max(1, info["iterations"] - half))
            if ref is not None:
                ms = []
                for _ in range(max(3, a.reps // 4)):
                    la, lrho = K.libsvm_train(ref, x, n_pos, kernel)[:2]
                    ms.append(K.last_train_seconds * 1e3)
                r["libsvm_cpu"] = stats(ms)
                r["libsvm_max_alpha_diff"] = float(np.abs(la - alpha).max())
                r["libsvm_rho_diff"] = float(abs(lrho - info["rho"]))
            else:
                r["libsvm_cpu"] = "not measured (oracle/_ref absent)"
            results.append(r)
    ctx.close()
    print(json.dumps(dict(probe="svm_kernel_train", reps=a.reps, results=results)))


if __name__ == "__main__":
    main()
