"""Aggregated-features detector: exact feature pyramid against the approximated one, on the same frames.

  python tools/aggregated_probe.py                       ms per frame of the three modes on 1920x1080 and 640x480
  python tools/aggregated_probe.py --profile DIR         the same, plus one `rocprofv3 --kernel-trace --stats` run per mode and size
                                                         (a fresh child process each; CSVs under DIR) and the per-kernel split
  python tools/aggregated_probe.py --mode M --size WxH   one mode only (what the profiled child runs)
  ... --profile DIR --csv FILE                           also writes the per-kernel table (mode, size, kernel, calls, us per frame)

Modes: exact (FHOG on every layer), approx (explicit lambdas), approx_est (lambdas estimated per frame: one more host wait).
n = 8 layers per octave, window 10 x 10 cells of 8 px, 31 channels.  Frames are uploaded by every call (host images), as the
detector's applications do.  The modes take turns frame by frame inside one process.  The exact mode runs the device code every earlier commit ran, so it stands in for them.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("exact", "approx", "approx_est")
SIZES = ((1920, 1080), (640, 480))
KERNEL = re.compile(r"\bk_\w+")


def run_modes(modes, size, frames, warmup):
    """ms per frame of every mode on the same frames, the modes taking turns frame by frame (and the order rotating), so that
    clock and thermal drift during the run falls on all of them alike"""
    from featuredetection_amd import capi, synth
    ctx = capi.Context(0)
    weights = np.random.default_rng(5).normal(0, 0.05, (10, 10, 31)).astype(np.float32)
    dets = {}
    for mode in modes:
        lambdas = np.linspace(0.05, 0.25, 31) if mode == "approx" else None
        dets[mode] = capi.Aggregated(ctx, weights, 0.1, 1.5, cell_size=8, octave_layers=8, approximate=mode != "exact", lambdas=lambdas)
    imgs = [synth.make_frame(size[0], size[1], seed=100 + i) for i in range(4)]
    for i in range(warmup):
        for mode in modes:
            dets[mode].detect(imgs[i % len(imgs)], candidates=False)
    times = {mode: [] for mode in modes}
    ndet = {mode: 0 for mode in modes}
    for i in range(frames):
        for k in range(len(modes)):
            mode = modes[(i + k) % len(modes)]
            t0 = time.perf_counter()
            fin, _ = dets[mode].detect(imgs[i % len(imgs)], candidates=False)
            times[mode].append((time.perf_counter() - t0) * 1e3)
            ndet[mode] += len(fin)
    out = []
    for mode in modes:
        layers = dets[mode].layers()
        t = np.array(times[mode])
        out.append(dict(mode=mode, size="%dx%d" % size, frames=frames, ms_per_frame_median=float(np.median(t)), ms_per_frame_mean=float(t.mean()),
                        ms_per_frame_p10=float(np.percentile(t, 10)), ms_per_frame_p90=float(np.percentile(t, 90)), layers=int(len(layers)),
                        approximated_layers=int(layers["approximated"].sum()), detections_per_frame=ndet[mode] / frames))
        dets[mode].close()
    ctx.close()
    return out


def kernel_rows(csv_path):
    """(kernel, calls, total ns) per row of a rocprofv3 kernel_stats CSV; the kernel is the first k_* identifier of the demangled
    name (parameter types such as `(anonymous namespace)::DownJobs` follow it), the whole name for the runtime's own kernels"""
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            m = KERNEL.search(r["Name"])
            rows.append((m.group(0) if m else r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])))
    return rows


def kernel_split(outdir, frames_total):
    """per-frame microseconds per kernel from the child's kernel_stats CSV; pre-score = every k_* kernel but the score kernels
    (gray conversion, pyramid, FHOG, and the two kernels of the approximated form), the runtime's copies and fills apart"""
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    per, calls = {}, {}
    for name, n, ns in kernel_rows(files[0]):
        per[name] = per.get(name, 0.0) + ns / 1e3 / frames_total
        calls[name] = calls.get(name, 0) + n
    ours = {k: v for k, v in per.items() if k.startswith("k_")}
    score = sum(v for k, v in ours.items() if k.startswith("k_fhog_score"))
    return dict(us_per_frame=per, calls=calls, pre_score_us_per_frame=sum(ours.values()) - score, score_us_per_frame=score,
                runtime_copy_fill_us_per_frame=sum(v for k, v in per.items() if not k.startswith("k_")), csv=files[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=MODES)
    ap.add_argument("--size", default=None)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 runs")
    ap.add_argument("--csv", default=None, help="with --profile: write the per-kernel table of all modes and sizes here")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else list(SIZES)
    modes = [a.mode] if a.mode else list(MODES)
    out = []
    table = []
    for size in sizes:
        results = run_modes(modes, size, a.frames, a.warmup)
        for r in results:
            if a.profile:   # the profiled run is a process of its own: kernel times only, its wall times are not reported
                d = os.path.join(a.profile, "%s_%dx%d" % (r["mode"], size[0], size[1]))
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                       "--mode", r["mode"], "--size", "%dx%d" % size, "--frames", str(a.frames), "--warmup", str(a.warmup)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=200)
                if p.returncode != 0:
                    raise SystemExit("rocprofv3 run failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
                r["kernels"] = kernel_split(d, a.frames + a.warmup)
                if r["kernels"] is None:
                    raise SystemExit("no kernel_stats CSV under %s" % d)
                for name, us in sorted(r["kernels"]["us_per_frame"].items(), key=lambda kv: -kv[1]):
                    table.append((r["mode"], r["size"], name, r["kernels"]["calls"][name], a.frames + a.warmup, "%.3f" % us))
            out.append(r)
    if a.csv and table:
        with open(a.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["mode", "size", "kernel", "calls", "frames", "us_per_frame"])
            w.writerows(table)
    print(json.dumps(dict(probe="aggregated", results=out)))


if __name__ == "__main__":
    main()
