"""Detector training on the device: the large linear C-SVC trainer (fd_linear_svm_train_large) and one image of a
hard-negative bootstrapping round (fd_aggregated_set_svm / _detect / _extract), next to libsvm's svm_train on this machine's CPU.

  python tools/detector_training_probe.py                        n = 2048, 8192, 16384 examples of 496 floats (4 x 4 cells x 31)
  python tools/detector_training_probe.py --sizes 2048 --reps 5
  python tools/detector_training_probe.py --libsvm-max-n 16384   libsvm on the largest problem too (minutes of CPU time)

The context runs on a stream of torch's, and every ABI call is bracketed by two device events on that stream (the calls end in a
synchronise of their own; the events give the time on the stream's clock), after warm-up calls; medians with p10 / p90.
  start_ms          a training stopped after one iteration: the upload of X, the Gram kernel (n^2 d), one solver launch, the finish
  us_per_iteration  the slope between two runs stopped at different iteration counts, so that the start cancels
  train_ms          the whole training, with its iteration count
libsvm (the compiled reference unit, oracle/_ref) is timed around svm_train alone on the same X where that unit is present and n
is at most --libsvm-max-n; otherwise the figure says "not measured".  The bootstrapping figures are for one 640 x 480 gray image:
update, detect with a freshly installed model (candidates before suppression), and the re-extraction of 100 of its candidates
one box per call (as DetectorTrainer does) and in one call.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch   # before libfd_hip.so: the wheel brings its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_p10=float(np.percentile(ms, 10)), ms_p90=float(np.percentile(ms, 90)))


def timed(stream, fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()   # ends in a synchronise of the context's stream
        t1.record(stream)
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 8192, 16384])
    ap.add_argument("--d", type=int, default=496)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--libsvm-max-n", type=int, default=8192)
    a = ap.parse_args()
    import svm_train_model as M
    from featuredetection_amd import capi, synth
    from oracle import pyoracle as O
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    ref = O.ref()
    results = []
    for n in a.sizes:
        n_pos = max(1, n // 16)
        x = M.ehog_like(n_pos, n - n_pos, a.d, seed=300 + n)
        w, bias, alpha, info = capi.linear_svm_train_large(ctx, x, n_pos)
        k1 = max(1, min(info["iterations"] // 3, 4000))
        k2 = max(k1 + 1, min(info["iterations"], 3 * k1))
        r = dict(n_pos=n_pos, n_neg=n - n_pos, d=a.d, info=info, lds_bytes=capi.linear_svm_train_large_limits(n_pos, n - n_pos, a.d)[0],
                 train=timed(stream, lambda: capi.linear_svm_train_large(ctx, x, n_pos), a.reps),
                 start=timed(stream, lambda: capi.linear_svm_train_large(ctx, x, n_pos, max_iterations=1), a.reps))
        t1 = timed(stream, lambda: capi.linear_svm_train_large(ctx, x, n_pos, max_iterations=k1), a.reps)
        t2 = timed(stream, lambda: capi.linear_svm_train_large(ctx, x, n_pos, max_iterations=k2), a.reps)
        r["us_per_iteration"] = (t2["ms_median"] - t1["ms_median"]) * 1e3 / (k2 - k1)
        r["slope_iterations"] = [k1, k2]
        if ref is not None and n <= a.libsvm_max_n:
            la, lrho, lnsv = M.libsvm_train(ref, x, n_pos)
            r["libsvm_cpu_ms"] = M.last_train_seconds * 1e3   # one run
            r["libsvm_max_alpha_diff"] = float(np.abs(la - alpha).max())
            r["libsvm_rho_diff"] = float(abs(lrho - info["rho"]))
        else:
            r["libsvm_cpu_ms"] = "not measured"
        results.append(r)
    # one image of a bootstrapping round
    gray = O.bgr2gray(synth.make_frame(640, 480, seed=3))
    rng = np.random.default_rng(4)
    weights = rng.normal(0, 0.05, (4, 4, 31)).astype(np.float32)
    det = capi.Aggregated(ctx, np.zeros((4, 4, 31), np.float32), 0.0, 0.0, cell_size=8, octave_layers=5, nms_overlap=1.0)

    def detect():
        det.set_svm(weights, 0.0, 0.0)
        return det.detect(gray)[1]

    cand = detect()
    boxes = [(int(c["x"]), int(c["y"]), int(c["w"]), int(c["h"])) for c in cand[:100]]
    boot = dict(candidates=len(cand), boxes=len(boxes), update=timed(stream, lambda: det.update(gray), a.reps),
                set_svm_and_detect=timed(stream, detect, a.reps),
                extract_one_by_one=timed(stream, lambda: [det.extract([b]) for b in boxes], a.reps),
                extract_one_call=timed(stream, lambda: det.extract(boxes), a.reps))
    det.close()
    ctx.close()
    print(json.dumps(dict(probe="detector_training", reps=a.reps, results=results, bootstrapping_image=boot)))


if __name__ == "__main__":
    main()
