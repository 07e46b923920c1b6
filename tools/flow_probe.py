#!/usr/bin/env python3
"""Time of the optical-flow transition model's device work (fd_flow) per frame, for gray frames that already lie on the
device, at 640 x 480 and 1920 x 1080 and at 76 and 1024 points:
  update    fd_flow_update alone (the padded levels and Scharr derivatives of one frame), then a synchronise
  track_fb  fd_flow_track_fb alone (forward, backward, one read-back)
  predict   what OpticalFlowTransitionModel::predict does with a frame: update, track_fb, fd_flow_median, and the motion applied to
            800 samples (numpy here, a loop over Sample objects in the host class)
Host clock around calls that end in a synchronise.  Frames are blurred seeded noise, each the previous one moved by (3, -2), so the
tracker iterates as it does on a real sequence.  Reports the median with p10 and p90 over --frames timed frames after --warmup frames.
Usage: python tools/flow_probe.py [--frames 200] [--warmup 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch   # before the library: whichever HIP runtime is loaded first serves the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from featuredetection_amd import capi   # noqa: E402


def textured(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((h, w))
    k = np.exp(-0.5 * (np.arange(-6, 7) / 2.0) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        a = sum(wt * np.roll(a, t - 6, axis=axis) for t, wt in enumerate(k))
    a = (a - a.min()) / (a.max() - a.min())
    return np.rint(a * 255).astype(np.uint8)


def points(w, h, n):
    """n points on a square grid over the central half of the frame"""
    side = int(np.ceil(np.sqrt(n)))
    xs, ys = np.meshgrid(np.linspace(w * 0.25, w * 0.75, side), np.linspace(h * 0.25, h * 0.75, side))
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)[:n]


def stats(samples):
    s = np.sort(np.asarray(samples)) * 1e3
    return "median %.3f ms (p10 %.3f, p90 %.3f)" % (np.median(s), s[int(0.1 * len(s))], s[int(0.9 * len(s))])


def run(ctx, w, h, n, frames, warmup):
    base = textured(w, h, 5)
    images = [torch.from_numpy(np.roll(base, (-2 * k, 3 * k), axis=(0, 1)).copy()).to("cuda:0") for k in range(4)]
    torch.cuda.synchronize()
    flow = capi.Flow(ctx, w, h)
    pts = points(w, h, n)
    rng = np.random.default_rng(1)
    sx, sy, ssize = rng.integers(0, w, 800), rng.integers(0, h, 800), rng.integers(40, 200, 800)
    z = rng.standard_normal((800, 3))
    flow.update(images[0])
    flow.update(images[1])
    ctx.synchronize()
    t_update, t_track, t_predict = [], [], []
    ok = 0
    for k in range(frames + warmup):
        image = images[(k + 2) % 4]
        t0 = time.perf_counter()
        flow.update(image)
        ctx.synchronize()
        t1 = time.perf_counter()
        flow.track_fb(pts)
        t2 = time.perf_counter()
        flow.update(image)
        fwd, bwd, fst, bst = flow.track_fb(pts)
        m = capi.flow_median(pts, fwd, bwd, fst, bst)
        if m["ok"]:
            vx = np.rint(float(m["median_x"]) + 10.0 * z[:, 0]).astype(np.int32)
            vy = np.rint(float(m["median_y"]) + 10.0 * z[:, 1]).astype(np.int32)
            vs = (float(m["median_ratio"]) * np.exp2(0.08 * z[:, 2])).astype(np.float32)
            _ = sx + vx, sy + vy, np.rint(ssize.astype(np.float32) * vs).astype(np.int32)
        t3 = time.perf_counter()
        if k >= warmup:
            t_update.append(t1 - t0)
            t_track.append(t2 - t1)
            t_predict.append(t3 - t2)
            ok += int(m["ok"])
    levels = flow.levels
    flow.close()
    print("%4d x %-4d %4d points, %d levels: update   %s" % (w, h, n, levels, stats(t_update)))
    print("%4d x %-4d %4d points            track_fb %s" % (w, h, n, stats(t_track)))
    print("%4d x %-4d %4d points            predict  %s   (median flow usable on %d of %d frames)" % (w, h, n, stats(t_predict), ok, frames))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    ctx = capi.Context(0)
    for w, h in ((640, 480), (1920, 1080)):
        for n in (76, 1024):
            run(ctx, w, h, n, args.frames, args.warmup)
    ctx.close()


if __name__ == "__main__":
    main()
