"""Aggregated-features detector: FPDW channel features next to FHOG, exact and approximated feature pyramid, on frames in HBM.

  python tools/fpdw_probe.py                      ms per frame of the four detectors on 640x480 and 1920x1080
  python tools/fpdw_probe.py --size 640x480       one size only
  python tools/fpdw_probe.py --profile DIR        also one `rocprofv3 --kernel-trace --stats` run per size (a fresh child process;
                                                  CSVs under DIR) and the per-kernel microseconds per frame

Detectors: fhog / fpdw x exact / approx (explicit lambdas).  n = 8 layers per octave, window 8 x 8 cells of 8 px; fpdw as
DetectorTrainingApp builds it: fast gradient, no bin interpolation, normalisation radius = cell size, constant 0.01.  The frames are
BGR and device-resident (fd_aggregated_detect with is_device = 1): no upload in the timed window.  Each call is bracketed by events
on the context's stream (the call itself ends in a synchronise; the host clock around it is reported too), after warm-up calls of
every detector; the detectors take turns frame by frame.  The score threshold lets no candidate through, so that the four figures
hold the same work: pyramid, features, scores and their download.  The fhog figures are context, not a target.  Prints one JSON line."""
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
THRESHOLD = 1e30   # no candidates: random weights score the two feature types differently, and candidates are host work that depends on the frame


def detectors(capi, ctx):
    rng = np.random.default_rng(5)
    out = {}
    for features, d in (("fhog", 31), ("fpdw", 10)):
        weights = rng.normal(0, 0.05, (8, 8, d)).astype(np.float32)
        for approximate in (False, True):
            lambdas = np.linspace(0.05, 0.25, d) if approximate else None
            out["%s_%s" % (features, "approx" if approximate else "exact")] = capi.Aggregated(
                ctx, weights, 0.1, THRESHOLD, cell_size=8, octave_layers=8, approximate=approximate, lambdas=lambdas, features=features)
    return out


def run(size, frames, warmup):
    from featuredetection_amd import capi, synth
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    dets = detectors(capi, ctx)
    names = list(dets)
    imgs = [torch.from_numpy(synth.make_frame(size[0], size[1], seed=100 + i)).cuda() for i in range(4)]
    torch.cuda.synchronize()
    call = lambda name, i: dets[name].detect_device(imgs[i % len(imgs)].data_ptr(), size[0], size[1], 3, candidates=False)
    for i in range(warmup):
        for name in names:
            call(name, i)
    dev_ms, host_ms, ndet = ({n: [] for n in names} for _ in range(3))
    with torch.cuda.stream(stream):
        for i in range(frames):
            for k in range(len(names)):
                name = names[(i + k) % len(names)]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                fin, _ = call(name, i)
                e1.record(stream)
                e1.synchronize()
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                dev_ms[name].append(e0.elapsed_time(e1))
                ndet[name].append(len(fin))
    out = []
    for name in names:
        layers = dets[name].layers()
        t, h = np.array(dev_ms[name]), np.array(host_ms[name])
        out.append(dict(detector=name, size="%dx%d" % size, frames=frames, ms_per_frame_median=float(np.median(t)),
                        ms_per_frame_p10=float(np.percentile(t, 10)), ms_per_frame_p90=float(np.percentile(t, 90)),
                        host_ms_per_frame_median=float(np.median(h)), layers=int(len(layers)),
                        approximated_layers=int(layers["approximated"].sum()), detections_per_frame=float(np.mean(ndet[name]))))
        dets[name].close()
    ctx.close()
    return out


def kernel_split(outdir, frames_total):
    """microseconds per frame and detector round (all four detectors run once per frame) of every kernel in the child's kernel_stats CSV"""
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
        results += run(size, a.frames, a.warmup)
        if a.profile:   # a process of its own: kernel times only, its frame times are not reported
            d = os.path.join(a.profile, "%dx%d" % size)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--size", "%dx%d" % size, "--frames", str(a.frames), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit("rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
            kernels["%dx%d" % size] = kernel_split(d, a.frames + a.warmup)
    print(json.dumps(dict(probe="fpdw", results=results, kernels=kernels)))


if __name__ == "__main__":
    main()
