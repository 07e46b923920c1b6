"""Extended-HOG tracker (fd_ehog_tracker): ms per frame of update (gray pyramid + feature layers + heat layers) on frames in HBM, next
to an FHOG fd_aggregated handle of the same cell size for context, ms per call of evaluate_samples / extract_cells /
extract_patches at n = 4,096 samples, and ms per call of heat_peak / heat_maxima.

  python tools/ehog_probe.py                      640x480 and 1920x1080
  python tools/ehog_probe.py --size 640x480       one size only
  python tools/ehog_probe.py --profile DIR        also one `rocprofv3 --kernel-trace --stats` run per size (a fresh child process;
                                                  CSVs under DIR) and the per-kernel microseconds per frame

Tracker defaults of ExtendedHogBasedMeasurementModel: cell 5, 35 cells as 5 x 7, 9 unsigned bins at alpha 0.48, cell interpolation, 5 layers
per octave; min width 5 * 5, max width the image height * 5 / 7.  The frames are BGR and device-resident (is_device = 1): no upload in the
timed window.  Each call is bracketed by events on the context's stream (the call itself ends in a synchronise; the host clock around it
is reported too), after warm-up calls; medians are reported.  The FHOG figure (window 5 x 7 cells of 5 px, 5 layers per octave, no
candidates) is context, not a target: it holds the same kind of work (pyramid, features, scores) plus the download of its score maps.
Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch   # before libfd_hip.so: the wheel brings its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((640, 480), (1920, 1080))
KERNEL = re.compile(r"\bk_\w+")
CELL, COLS, ROWS, OLC, NSAMPLES = 5, 5, 7, 5, 4096


def timed(stream, fn, reps):
    dev, host = [], []
    with torch.cuda.stream(stream):
        for i in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            fn(i)
            e1.record(stream)
            e1.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    return dict(ms_median=float(np.median(dev)), ms_p10=float(np.percentile(dev, 10)), ms_p90=float(np.percentile(dev, 90)),
                host_ms_median=float(np.median(host)))


def run(size, frames, warmup):
    from featuredetection_amd import capi, synth
    w, h = size
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    rng = np.random.default_rng(5)
    fp = capi.cehog_params(cell_size=CELL, bin_count=9, signed_gradients=False, unsigned_gradients=True, interpolate_bins=False,
                           interpolate_cells=True, alpha=0.48)
    tracker = capi.EhogTracker(ctx, capi.ehog_tracker_params(fp, COLS, ROWS, OLC, CELL * COLS, h * COLS // ROWS))
    tracker.set_svm(rng.normal(0, 0.05, (ROWS, COLS, tracker.channels)).astype(np.float32), 0.1)
    fhog = capi.Aggregated(ctx, rng.normal(0, 0.05, (ROWS, COLS, 31)).astype(np.float32), 0.1, 1e30, cell_size=CELL, octave_layers=OLC)
    imgs = [torch.from_numpy(synth.make_frame(w, h, seed=100 + i)).cuda() for i in range(4)]
    torch.cuda.synchronize()
    update = lambda i: tracker.update_device(imgs[i % len(imgs)].data_ptr(), w, h, 3)
    detect = lambda i: fhog.detect_device(imgs[i % len(imgs)].data_ptr(), w, h, 3, candidates=False)
    for i in range(warmup):
        update(i)
        detect(i)
    out = dict(size="%dx%d" % size, frames=frames, layers=int(len(tracker.layers())), cells=int(sum(int(l["rows"]) * int(l["cols"]) for l in tracker.layers())),
               update=timed(stream, update, frames), fhog_aggregated_detect=timed(stream, detect, frames))
    # samples around the frame, widths over the pyramid's range
    width = rng.integers(CELL * COLS, h * COLS // ROWS, NSAMPLES)
    samples = np.stack([rng.integers(0, w, NSAMPLES), rng.integers(0, h, NSAMPLES), width, width * ROWS // COLS], 1).astype(np.int32)
    for name, fn in (("evaluate_samples", lambda i: tracker.evaluate_samples(samples)), ("extract_cells", lambda i: tracker.extract_cells(samples)),
                     ("extract_patches", lambda i: tracker.extract_patches(samples, want_score=True))):
        for i in range(3):
            fn(i)
        out[name] = timed(stream, fn, max(5, frames // 4))
        out[name]["n"] = NSAMPLES
        out[name]["valid"] = int(fn(0)[0].sum())
    # the per-frame searches over the heat maps: k_ehog_peak is one workgroup over every offered position
    out["heat_peak"] = timed(stream, lambda i: tracker.heat_peak(), max(5, frames // 4))
    out["heat_maxima"] = timed(stream, lambda i: tracker.heat_maxima(-1.0, cap=1 << 20), max(5, frames // 4))
    out["heat_maxima"]["count"] = int(len(tracker.heat_maxima(-1.0, cap=1 << 20)))
    tracker.close()
    fhog.close()
    ctx.close()
    return out


def kernel_split(outdir, frames_total):
    """microseconds per frame of every kernel in the child's kernel_stats CSV (update and the FHOG detector run once per frame; the sample
    calls a few times per run)"""
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    per = {}
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            m = KERNEL.search(r["Name"])
            name = m.group(0) if m else r["Name"]
            per[name] = per.get(name, 0.0) + float(r["TotalDurationNs"]) / 1e3 / frames_total
    return dict(us_per_frame=per, csv=files[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default=None)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 runs")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else list(SIZES)
    results, kernels = [], {}
    for size in sizes:
        results.append(run(size, a.frames, a.warmup))
        if a.profile:   # a process of its own: kernel times only, its frame times are not reported
            d = os.path.join(a.profile, "%dx%d" % size)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--size", "%dx%d" % size, "--frames", str(a.frames), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit("rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
            kernels["%dx%d" % size] = kernel_split(d, a.frames + a.warmup)
    print(json.dumps(dict(probe="ehog", results=results, kernels=kernels)))


if __name__ == "__main__":
    main()
