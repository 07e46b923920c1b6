"""liblinear's L2-loss SVC on the device (fd_liblinear_train): ms per call, ms per (pass, step) pair and the pass's share of the HBM
bandwidth, next to the dual trainers (fd_linear_svm_train / _train_large) on the sizes they take.

  python tools/liblinear_probe.py                 all sizes
  python tools/liblinear_probe.py --reps 10 --skip-largest

Sizes: 100 + 900 x 1116 (a tracker's stores with 31 channels), 4096 + 12288 x 1116 (the dual trainers' limit) and 65536 + 196608 x
1116.  x lives on the device; every call ends in a synchronise of its own and is timed with the host clock around it, after
warm-up calls; medians with p10 / p90.  The time per pair is the slope between a run stopped by max_cg_steps at about half the CG
steps and the full run, over the difference of their pair counts (a pair per fun, grad and Hv evaluation), so that the copies and
the set-up cancel.  The pass's bandwidth is the bytes of x one Hv pass has to read (the active rows at the returned w) over the
time of a whole pair, against 8 TB/s: a lower bound of the kernel's own share, the step and the two kernel boundaries included.
`forms` times the two kernel forms on sizes around the selection rule: a batch of one problem always takes the single-workgroup
form, FD_LIBLINEAR_SMALL_ROWS=0 the multi-workgroup one.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # before libfd_hip.so: the wheel brings its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = ((100, 900, 1116), (4096, 12288, 1116), (65536, 196608, 1116))
FORM_SIZES = ((40, 90, 39), (100, 157, 129), (100, 400, 129), (257, 1023, 129), (300, 700, 324), (100, 900, 1116))
HBM_PEAK = 8.0e12


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_p10=float(np.percentile(ms, 10)), ms_p90=float(np.percentile(ms, 90)))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()   # ends in a device synchronise
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def make_x(seed, n_pos, n_neg, d):
    """liblinear_cases.make_x in float32 and in blocks, for the sizes that would not fit in float64"""
    rng = np.random.default_rng(seed)
    direction = (rng.normal(size=d) / np.sqrt(d)).astype(np.float32)
    out = np.empty((n_pos + n_neg, d), np.float32)
    for r0 in range(0, n_pos + n_neg, 16384):
        r1 = min(r0 + 16384, n_pos + n_neg)
        y = np.where(np.arange(r0, r1) < n_pos, 1.0, -1.0).astype(np.float32)
        out[r0:r1] = np.abs(rng.standard_normal((r1 - r0, d), np.float32)) * 0.5 + 0.6 * y[:, None] * direction[None, :] + 0.25
    return out


def pairs(info):
    """(pass, step) pairs of a run: fun and grad at the start, an Hv per CG step, a fun per outer iteration, a grad per accepted one"""
    return 2 + info["cg_steps"] + info["trace_len"] + info["iterations"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-largest", action="store_true")
    a = ap.parse_args()
    from featuredetection_amd import capi
    ctx = capi.Context(0)
    os.environ.pop("FD_LIBLINEAR_SMALL_ROWS", None)
    results = []
    for n_pos, n_neg, d in SIZES[:2] if a.skip_largest else SIZES:
        n = n_pos + n_neg
        x = torch.from_numpy(make_x(n, n_pos, n_neg, d)).cuda()
        w, b, wd, trace, info = capi.liblinear_train(ctx, x, n_pos)
        half = max(1, info["cg_steps"] // 2)
        _, _, _, _, info_half = capi.liblinear_train(ctx, x, n_pos, max_cg_steps=half)
        full = timed(lambda: capi.liblinear_train(ctx, x, n_pos), a.reps)
        part = timed(lambda: capi.liblinear_train(ctx, x, n_pos, max_cg_steps=half), a.reps)
        ms_pair = (full["ms_median"] - part["ms_median"]) / max(1, pairs(info) - pairs(info_half))
        single, slab_rows, scratch, lds = capi.liblinear_train_limits(n_pos, n_neg, d)
        r = dict(n_pos=n_pos, n_neg=n_neg, d=d, single_workgroup=single, slab_rows=slab_rows, scratch_bytes=scratch, lds_bytes=lds, info=info,
                 pairs=pairs(info), train=full, train_half_cg=part, ms_per_pair=ms_pair)
        hv_bytes = 4.0 * info["n_active"] * d
        r["hv_pass_bytes"] = hv_bytes
        r["hv_pass_fraction_of_hbm_peak"] = hv_bytes / (ms_pair * 1e-3) / HBM_PEAK
        if n <= 1024:
            xh = x.cpu().numpy()
            r["linear_svm_train"] = timed(lambda: capi.linear_svm_train(ctx, xh, n_pos), a.reps)
            r["linear_svm_train_info"] = capi.linear_svm_train(ctx, xh, n_pos)[3]
        elif n <= capi.SVM_LARGE_MAX_N:
            xh = x.cpu().numpy()
            r["linear_svm_train_large"] = timed(lambda: capi.linear_svm_train_large(ctx, xh, n_pos), max(2, a.reps // 4), warmup=1)
            r["linear_svm_train_large_info"] = capi.linear_svm_train_large(ctx, xh, n_pos)[3]
            r["liblinear_train_host_x"] = timed(lambda: capi.liblinear_train(ctx, xh, n_pos), max(2, a.reps // 4), warmup=1)
        results.append(r)
        del x
    forms = []
    for n_pos, n_neg, d in FORM_SIZES:
        x = make_x(n_pos + n_neg + d, n_pos, n_neg, d)
        os.environ["FD_LIBLINEAR_SMALL_ROWS"] = "0"
        multi = timed(lambda: capi.liblinear_train(ctx, x, n_pos), a.reps)
        info = capi.liblinear_train(ctx, x, n_pos)[4]
        os.environ.pop("FD_LIBLINEAR_SMALL_ROWS")
        single = timed(lambda: capi.liblinear_train_batch(ctx, [(x, n_pos)]), a.reps)
        forms.append(dict(n_pos=n_pos, n_neg=n_neg, d=d, elements=(n_pos + n_neg) * d, pairs=pairs(info), multi_workgroup=multi,
                          single_workgroup=single, rule_picks_single=capi.liblinear_train_limits(n_pos, n_neg, d)[0]))
    ctx.close()
    print(json.dumps(dict(probe="liblinear", reps=a.reps, results=results, forms=forms)))


if __name__ == "__main__":
    main()
