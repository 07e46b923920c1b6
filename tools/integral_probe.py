"""Integral-image features on sampled windows (capi.Integral): update, Haar and SURF extraction, the measurement model, on frames in HBM.

  python tools/integral_probe.py                      640x480 and 1920x1080
  python tools/integral_probe.py --size 640x480       one size only
  python tools/integral_probe.py --profile DIR        also one `rocprofv3 --kernel-trace --stats` run per size (a fresh child process;
                                                      CSVs under DIR) and the mean microseconds per launch of every kernel
  python tools/integral_probe.py --hog                the integral HOG family instead: 1000 samples of a 640x480 frame with the reference's
                                                      default `feature ihog` configuration (gradientCount 30, 9 bins interpolated, spatial
                                                      histogram of 6-pixel cells, l2norm), three routes to the same n x 225 floats on the host
                                                      -- per sample (the three stand-alone calls on one sample at a time, what the host
                                                      layer's per-Mat loop issues), composed (the three stand-alone calls on all samples,
                                                      two host round trips between them) and fused (fd_integral_extract_hog) -- and
                                                      svm_evaluate_samples(hog=...) with a 256-SV RBF SVM
  python tools/integral_probe.py --hog --root DIR     ... of the tree under DIR (a checkout of another commit with its library built); a
                                                      tree without the fused call reports the first two routes

Frames are gray and device-resident (fd_integral_update with is_device = 1): `update` is the three launches and nothing else, and
its achieved fraction of HBM is (W H + 4 (W + 1)(H + 1)) bytes -- what it must read and write -- over the measured time, against the
8 TB/s DESIGN.md section 6 uses.  Samples are of mixed sizes (12 to 160 pixels, width != height) inside the frame; the extraction
calls leave their rows on the device (no download), but the n x 16 bytes of samples are uploaded inside the timed call, as they are
for a tracker.  svm_evaluate_samples is the whole call: upload, features, a 256-SV RBF SVM, distances back, logistic on the host.
Every call is bracketed by events on the context's stream; medians of `--calls` timed calls after `--warmup` calls.  One JSON line."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch   # before libfd_hip.so: the wheel brings its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((640, 480), (1920, 1080))
COUNTS = (4096, 262144)
HBM_BYTES_PER_S = 8e12
KERNEL = re.compile(r"\bk_\w+")


def make_samples(w, h, n, seed):
    rng = np.random.default_rng(seed)
    sw = rng.integers(12, 161, n)
    sh = np.minimum(sw + rng.integers(1, 40, n), h)
    x0 = (rng.random(n) * (w + 1 - sw + 1)).astype(np.int64)
    y0 = (rng.random(n) * (h + 1 - sh + 1)).astype(np.int64)
    return np.stack([x0 + sw // 2, y0 + sh // 2, sw, sh], 1).astype(np.int32)


def timed(stream, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))


def run(size, calls, warmup):
    from featuredetection_amd import capi, synth
    w, h = size
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    g = capi.Integral(ctx)
    frames = [torch.from_numpy(synth.bgr2gray_np(synth.make_frame(w, h, seed=200 + i))).cuda() for i in range(4)]
    torch.cuda.synchronize()
    out = dict(size="%dx%d" % size, calls=calls)
    turn = [0]

    def update():
        turn[0] += 1
        g.update_device(frames[turn[0] % len(frames)].data_ptr(), w, h, 1)
    with torch.cuda.stream(stream):
        med, p10, p90 = timed(stream, update, calls, warmup)
        moved = w * h + 4 * (w + 1) * (h + 1)
        out["update"] = dict(us_median=med * 1e3, us_p10=p10 * 1e3, us_p90=p90 * 1e3, bytes=moved,
                             hbm_fraction=moved / (med * 1e-3) / HBM_BYTES_PER_S)
        hp = capi.haar_params()
        for n in COUNTS:
            s = make_samples(w, h, n, seed=n)
            few = max(5, calls // 4) if n > 100000 else calls
            med, p10, p90 = timed(stream, lambda: g.extract_haar(hp, s, download=False), few, max(2, warmup // 4))
            out["extract_haar_%d" % n] = dict(ms_median=med, ms_p10=p10, ms_p90=p90, samples_per_s=n / (med * 1e-3))
            med, p10, p90 = timed(stream, lambda: g.extract_surf(12, 4, s, download=False), few, max(2, warmup // 4))
            out["extract_surf_%d" % n] = dict(ms_median=med, ms_p10=p10, ms_p90=p90, samples_per_s=n / (med * 1e-3))
        s = make_samples(w, h, COUNTS[0], seed=1)
        feats, valid = g.extract_haar(hp, s)
        assert valid.all()
        svm = capi.Svm(ctx, synth.make_svm_f32(9, feats, nsv=256, gamma=0.5, positive_fraction=0.1))
        med, p10, p90 = timed(stream, lambda: g.svm_evaluate_samples(svm, s, haar=hp), calls, warmup)
        out["svm_evaluate_haar_%d_256sv" % COUNTS[0]] = dict(ms_median=med, ms_p10=p10, ms_p90=p90, samples_per_s=COUNTS[0] / (med * 1e-3))
        svm.close()
    g.close()
    ctx.close()
    return out


HOG_SAMPLES = 1000


def run_hog(calls, warmup):
    from featuredetection_amd import capi, synth
    w, h = SIZES[0]
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    g = capi.Integral(ctx)
    frame = torch.from_numpy(synth.bgr2gray_np(synth.make_frame(w, h, seed=200))).cuda()
    torch.cuda.synchronize()
    G, BINS = 30, 9
    hist = capi.hist_params(kind=capi.HIST_SPATIAL, pw=G, ph=G, sx=1, sy=1, bins=BINS, cell=6, block=1, normalization=1)
    s = make_samples(w, h, HOG_SAMPLES, seed=3)
    out = dict(size="%dx%d" % (w, h), samples=HOG_SAMPLES, calls=calls)

    def composed(samples):
        grad, valid = g.gradient_patches(G, G, samples)
        bins = capi.gradient_binning_image(ctx, grad.reshape(len(samples) * G, G, 2), BINS, signed_gradients=False, interpolate=True)
        return capi.hist_patch_batch(ctx, bins.reshape(len(samples), G, G, 4), hist), valid

    def per_sample():
        return np.concatenate([composed(s[i:i + 1])[0] for i in range(len(s))])

    def entry(t):
        return dict(ms_median=t[0], ms_p10=t[1], ms_p90=t[2], samples_per_s=HOG_SAMPLES / (t[0] * 1e-3))
    with torch.cuda.stream(stream):
        g.update_device(frame.data_ptr(), w, h, 1)
        want, valid = composed(s)
        assert valid.all()
        out["composed"] = entry(timed(stream, lambda: composed(s), calls, warmup))
        assert np.array_equal(per_sample(), want)
        out["per_sample"] = entry(timed(stream, per_sample, max(3, calls // 8), 1))
        svm = capi.Svm(ctx, synth.make_svm_f32(9, want, nsv=256, gamma=0.5, positive_fraction=0.1))
        # SingleClassifierModel's per-sample loop: extract one patch, classify it
        out["per_sample_svm_256sv"] = entry(timed(stream, lambda: [svm.distance(composed(s[i:i + 1])[0]) for i in range(len(s))], max(3, calls // 8), 1))
        if hasattr(capi, "integral_hog_params"):
            hp = capi.integral_hog_params(G, G, bins=BINS, interpolate_bins=True, hist=hist)
            got, gvalid = g.extract_hog(hp, s)
            assert gvalid.all() and np.array_equal(got, want)
            out["fused"] = entry(timed(stream, lambda: g.extract_hog(hp, s), calls, warmup))
            out["fused_rows_on_device"] = entry(timed(stream, lambda: g.extract_hog(hp, s, download=False), calls, warmup))
            out["svm_evaluate_hog_256sv"] = entry(timed(stream, lambda: g.svm_evaluate_samples(svm, s, hog=hp), calls, warmup))
        svm.close()
    g.close()
    ctx.close()
    return out


def kernel_split(outdir):
    """calls and mean microseconds per launch of every kernel in the child's kernel_stats CSV"""
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    per = {}
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            m = KERNEL.search(r["Name"])
            name = m.group(0) if m else r["Name"]
            e = per.setdefault(name, dict(calls=0, total_us=0.0))
            e["calls"] += int(r["Calls"])
            e["total_us"] += float(r["TotalDurationNs"]) / 1e3
    for e in per.values():
        e["us_per_launch"] = e["total_us"] / max(e["calls"], 1)
    return dict(kernels=per, csv=files[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default=None)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 runs")
    ap.add_argument("--hog", action="store_true", help="the integral HOG routes on 640x480 instead")
    ap.add_argument("--root", default=None, help="measure the featuredetection_amd package of this tree")
    a = ap.parse_args()
    if a.root:
        sys.path.insert(0, os.path.abspath(a.root))
    if a.hog:
        print(json.dumps(dict(probe="integral_hog", results=[run_hog(a.calls, a.warmup)])))
        return
    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else list(SIZES)
    results, kernels = [], {}
    for size in sizes:
        results.append(run(size, a.calls, a.warmup))
        if a.profile:   # a process of its own: kernel times only, its call times are not reported
            d = os.path.join(a.profile, "%dx%d" % size)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--size", "%dx%d" % size, "--calls", str(a.calls), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit("rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
            kernels["%dx%d" % size] = kernel_split(d)
    print(json.dumps(dict(probe="integral", results=results, kernels=kernels)))


if __name__ == "__main__":
    main()
