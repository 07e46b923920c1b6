"""Linear SVM training on the device (fd_linear_svm_train, fd_linear_svm_train_batch, fd_ehog_tracker_train_svm): ms per call and
microseconds per SMO iteration, next to libsvm's svm_train on this machine's CPU for the same problems.

  python tools/svm_train_probe.py                 all shapes
  python tools/svm_train_probe.py --reps 30

Shapes: 20 + 100 x 455 (the tracker's default stores, 13 channels; Q in LDS), 20 + 300 x 1085 (static negatives, 31 channels; Q in
memory), and 20 + 172 / 20 + 173 x 455, the last size with Q in LDS and the first without, for the cost of reading Q rows from
memory.  Every call ends in a synchronise of its own and is timed with the host clock around it, after warm-up calls; medians with
p10 / p90 are reported.  The time per iteration is the slope between a run stopped at half the iterations (max_iterations) and the
full run, so that the Gram, the copies and the launches cancel.  The batch figures are one call over 64 copies of the problem.
libsvm (the compiled reference unit, oracle/_ref) is timed around svm_train alone, single runs repeated `reps` times, where that
unit is present; it is the baseline -- the parent commit has no training path.  Prints one JSON line."""
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
SHAPES = ((20, 100, 455), (20, 172, 455), (20, 173, 455), (20, 300, 1085))


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
    import svm_train_model as M
    from featuredetection_amd import capi
    from oracle import pyoracle as O
    ctx = capi.Context(0)
    ref = O.ref()
    results = []
    for n_pos, n_neg, d in SHAPES:
        x = M.ehog_like(n_pos, n_neg, d, seed=100 + n_neg)
        w, bias, alpha, info = capi.linear_svm_train(ctx, x, n_pos)
        half = max(1, info["iterations"] // 2)
        full = timed(lambda: capi.linear_svm_train(ctx, x, n_pos), a.reps)
        part = timed(lambda: capi.linear_svm_train(ctx, x, n_pos, max_iterations=half), a.reps)
        gram = timed(lambda: capi.linear_svm_gram(ctx, x, n_pos), a.reps)
        batch = timed(lambda: capi.linear_svm_train_batch(ctx, [(x, n_pos)] * 64), max(3, a.reps // 4))
        r = dict(n_pos=n_pos, n_neg=n_neg, d=d, q_in_lds=capi.linear_svm_train_limits(n_pos, n_neg, d)[0], info=info, train=full,
                 train_half_iterations=part, gram_call=gram, batch64=batch,
                 us_per_iteration=(full["ms_median"] - part["ms_median"]) * 1e3 / max(1, info["iterations"] - half))
        if ref is not None:
            ms = []
            for _ in range(max(3, a.reps // 4)):
                la, lrho, lnsv = M.libsvm_train(ref, x, n_pos)
                ms.append(M.last_train_seconds * 1e3)
            r["libsvm_cpu"] = stats(ms)
            r["libsvm_max_alpha_diff"] = float(np.abs(la - alpha).max())
            r["libsvm_rho_diff"] = float(abs(lrho - info["rho"]))
        else:
            r["libsvm_cpu"] = "not measured (oracle/_ref absent)"
        results.append(r)
    # the tracker: 5 x 7 cells, 13 and 31 channels, on a 640 x 480 frame
    from featuredetection_amd import synth
    frame = synth.make_frame(640, 480, seed=3)
    for both, n_neg in ((False, 100), (True, 300)):
        fp = capi.cehog_params(cell_size=5, bin_count=18 if both else 9, signed_gradients=both, unsigned_gradients=True, interpolate_bins=False,
                               interpolate_cells=True, alpha=0.48)
        t = capi.EhogTracker(ctx, capi.ehog_tracker_params(fp, 5, 7, 5, 25, 480 * 5 // 7))
        t.update(frame)
        dd = 35 * t.channels
        x = M.ehog_like(20, n_neg, dd, seed=7)
        results.append(dict(tracker_train_svm=timed(lambda: t.train_svm(x, 20), a.reps), n_pos=20, n_neg=n_neg, d=dd,
                            set_svm=timed(lambda: t.set_svm(np.zeros((7, 5, t.channels), np.float32), 0.0), a.reps)))
        t.close()
    ctx.close()
    print(json.dumps(dict(probe="svm_train", reps=a.reps, results=results)))


if __name__ == "__main__":
    main()
