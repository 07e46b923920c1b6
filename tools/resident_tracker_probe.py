"""One frame of the reference's default tracker configuration -- transition opticalFlow (10 x 10 circular grid, fallback simple),
measurement on `ihog` (gradientCount 30, 9 bins interpolated, spatial histogram of 6-pixel cells, l2norm; scale 1.1) with a linear
SVM -- on 640 x 480 frames in HBM, at 100, 1000 and 8192 particles, as the library calls of two routes:

  generic    what the host layer's generic route asks of the library per frame: fd_flow_update, fd_integral_update, fd_flow_track_fb
             (waits, four arrays back), fd_flow_median on the host, fd_sample_maps_apply on the sample list, and
             fd_integral_svm_evaluate_samples (uploads the list, waits, distances back, the logistic on the host).  The host
             arithmetic between them (the Sample objects, resampling, moving the samples, the weighted mean) is NOT in the timing:
             the figure is a lower bound of that route.
  resident   fd_flow_update, fd_integral_update, fd_flow_track_fb_resident, fd_particles_sample_flow, _evaluate_integral,
             _weigh_classifier, _state_flow: the whole frame, draws uploaded, one read-back.

  python tools/resident_tracker_probe.py [--frames 60] [--warmup 10] [--rounds 5]
  python tools/resident_tracker_probe.py --host [--frames 40] [--rounds 3]
                 the same configuration through the host classes: tracker_app (AdaptiveCondensationTracker, `measurement
                 positionDependent`, adaptation included) on 640 x 480 PGM frames, once with FD_COND_DEVICE=0 and once with =1 per round
                 in turns; the app's own per-frame clock around tracker.process, the first 5 frames of a run left out

Both routes run in one process on the same build, alternating round by round.  A frame is timed by the host clock from its first
call to the return of its last, which waits for the stream on both routes.  Reported per route and particle count: the median
frame time over all rounds, the 10th and 90th percentile, and the spread of the per-round medians (the run-to-run noise a
difference has to exceed).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # before libfd_hip.so: the wheel brings its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 640, 480
COUNTS = (100, 1000, 8192)
G, BINS = 30, 9
TARGET = (320, 240, 120)   # x, y, size
SHIFT = (2, 1)
POSITION_DEVIATION, SIZE_DEVIATION, RANDOM_RATE = 10.0, 0.1, 0.35


def textured(seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((H, W))
    k = np.exp(-0.5 * (np.arange(-6, 7) / 2.0) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        a = sum(w * np.roll(a, t - 6, axis=axis) for t, w in enumerate(k))
    a = (a - a.min()) / (a.max() - a.min())
    return np.rint(a * 255).astype(np.uint8)


def run(frames_per_round, warmup, rounds):
    from featuredetection_amd import capi
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    base = textured(5)
    cycle = 8   # the texture moves by SHIFT per frame and jumps back every `cycle` frames (one frame without a usable flow)
    frames = [torch.from_numpy(np.roll(base, (SHIFT[1] * k, SHIFT[0] * k), axis=(0, 1)).copy()).cuda() for k in range(cycle)]
    torch.cuda.synchronize()
    hist = capi.hist_params(kind=capi.HIST_SPATIAL, pw=G, ph=G, sx=1, sy=1, bins=BINS, cell=6, block=1, normalization=1)
    hp = capi.integral_hog_params(G, G, bins=BINS, interpolate_bins=True, hist=hist)
    maps = [("resize", float(np.float32(1.1))), ("integral",)]
    x, y, size = TARGET
    pts_of = lambda k: (capi.flow_grid(10, 10, True) * np.float32(size) + np.array([x + SHIFT[0] * k, y + SHIFT[1] * k], np.float32)).astype(np.float32)
    out = dict(size="%dx%d" % (W, H), frames_per_round=frames_per_round, rounds=rounds, grid_points=int(len(pts_of(0))), routes={})
    with torch.cuda.stream(stream):
        flow, integral = capi.Flow(ctx, W, H), capi.Integral(ctx)
        integral.update_device(frames[0].data_ptr(), W, H, 1)
        box = capi.sample_maps_apply(maps, [(x, y, size, size)])
        feat, valid = integral.extract_hog(hp, box)
        assert valid[0]
        w = feat[0] - feat[0].mean()
        svm = capi.Svm(ctx, dict(kernel=0, dtype=1, sv=w[None, :].astype(np.float32), coeff=np.ones(1, np.float32), bias=np.float32(0)))
        own = float(svm.distance(feat)[0])
        threshold, logistic_a, logistic_b = 0.5 * own, 2.0, -4.0 / own
        for n in COUNTS:
            rng = np.random.default_rng(n)
            n_resampled = int((1 - RANDOM_RATE) * n)

            def draws():
                z = rng.standard_normal((n_resampled, 3))
                return np.stack([POSITION_DEVIATION * z[:, 0], POSITION_DEVIATION * z[:, 1], np.exp2(SIZE_DEVIATION * z[:, 2])], 1)

            def fresh_samples():
                s = rng.integers(40, 201, n - n_resampled)
                return np.stack([rng.integers(0, W - s + 1) + s // 2, rng.integers(0, H - s + 1) + s // 2, s], 1).astype(np.int32)

            particles = capi.Particles.unbound(ctx, n)
            turn = {"generic": 0, "resident": 0}
            next_id = [2]
            used = {"generic": 0, "resident": 0}

            def restart(route):
                turn[route] = 0
                flow.update(frames[0])
                if route == "resident":
                    particles.set(x=np.full(n, x), y=np.full(n, y), size=np.full(n, size), cluster_id=np.full(n, 1))

            def generic_frame():
                k = turn["generic"] = turn["generic"] + 1
                # the host's draws and sample list are made outside the clock: the generic route's host arithmetic is not measured
                z = draws()
                cx, cy = x + SHIFT[0] * (k % cycle), y + SHIFT[1] * (k % cycle)
                sizes = np.rint(size * z[:, 2]).astype(np.int32)
                xywh = np.concatenate([np.stack([np.rint(cx + z[:, 0]), np.rint(cy + z[:, 1]), sizes, sizes], 1).astype(np.int32),
                                       fresh_samples()[:, [0, 1, 2, 2]]])
                pts = pts_of((k - 1) % cycle)
                t0 = time.perf_counter()
                flow.update(frames[k % cycle])
                integral.update_device(frames[k % cycle].data_ptr(), W, H, 1)
                fwd, bwd, fst, bst = flow.track_fb(pts)
                motion = capi.flow_median(pts, fwd, bwd, fst, bst)
                mapped = capi.sample_maps_apply(maps, xywh)
                integral.svm_evaluate_samples(svm, mapped, hog=hp)
                t1 = time.perf_counter()
                used["generic"] += bool(motion["ok"])
                return t1 - t0

            def resident_frame():
                k = turn["resident"] = turn["resident"] + 1
                d0, d1, fresh, u = draws(), draws(), fresh_samples(), rng.random()
                pts = pts_of((k - 1) % cycle)
                t0 = time.perf_counter()
                flow.update(frames[k % cycle])
                integral.update_device(frames[k % cycle].data_ptr(), W, H, 1)
                flow.track_fb_resident(pts)
                particles.sample_flow(flow, n, n_resampled, u, d0, d1, fresh, next_id[0])
                particles.evaluate_integral(integral, svm, 1.0, maps, hog=hp)
                particles.weigh_classifier(logistic_a, logistic_b, threshold)
                info, motion = particles.state_flow(flow)
                t1 = time.perf_counter()
                next_id[0] += n - n_resampled
                used["resident"] += bool(motion["ok"])
                return t1 - t0

            step = {"generic": generic_frame, "resident": resident_frame}
            times = {"generic": [], "resident": []}
            for r in range(rounds):
                for route in (("generic", "resident") if r % 2 == 0 else ("resident", "generic")):
                    restart(route)
                    for _ in range(warmup):
                        step[route]()
                    times[route].append([step[route]() * 1e3 for _ in range(frames_per_round)])
            for route, per_round in times.items():
                flat = np.concatenate(per_round)
                medians = [float(np.median(r)) for r in per_round]
                out["routes"].setdefault(route, {})[str(n)] = dict(ms_median=float(np.median(flat)), ms_p10=float(np.percentile(flat, 10)),
                                                                   ms_p90=float(np.percentile(flat, 90)), round_medians_min=min(medians),
                                                                   round_medians_max=max(medians),
                                                                   flow_used_fraction=used[route] / float(rounds * (warmup + frames_per_round)))
            particles.close()
        flow.close()
        integral.close()
    ctx.close()
    return out


HOST_CONFIG = """tracking {
  seed 7
  transition opticalFlow { positionDeviation 10 sizeDeviation 0.08 fallback simple { positionDeviation 12.8 sizeDeviation 0.1 } }
  adaptive { resampling { particleCount %(n)d randomRate 0.35 minSize 40 maxSize 200 } }
  initialCount %(n)d
  measurement positionDependent {
    feature ihog { scale 1.1  signed false  interpolate true  bins 9  gradientCount 30
                   histogram spatial { cellSize 6  blockSize 1  interpolate false  normalization l2norm } }
    filter none  startFrameCount 1  stopFrameCount 0  targetThreshold 0.1  confidenceThreshold 0.95
    positiveOffsetFactor 0.05  negativeOffsetFactor 0.5  sampleNegativesAroundTarget 2  sampleAdditionalNegatives 10  sampleTestNegatives 10
    exploitSymmetry 0
    classifier { training { type libSvm c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.00556 logisticB -2.95 threshold 0 }
  }
}
"""


def run_host(frames, rounds):
    import subprocess
    import tempfile
    app = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
    out = dict(size="%dx%d" % (W, H), frames=frames, rounds=rounds, routes={"generic": {}, "device": {}})
    with tempfile.TemporaryDirectory() as tmp:
        base = textured(5)
        paths = []
        for k in range(frames + 1):
            path = os.path.join(tmp, "frame%d.pgm" % k)
            with open(path, "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (W, H))
                f.write(np.roll(base, (SHIFT[1] * (k % 8), SHIFT[0] * (k % 8)), axis=(0, 1)).tobytes())
            paths.append(path)
        x, y, size = TARGET
        for n in COUNTS:
            cfg = os.path.join(tmp, "tracking%d.cfg" % n)
            with open(cfg, "w") as f:
                f.write(HOST_CONFIG % dict(n=n))
            times = {"generic": [], "device": []}
            for r in range(rounds):
                for route in (("generic", "device") if r % 2 == 0 else ("device", "generic")):
                    env = dict(os.environ, FD_COND_DEVICE="1" if route == "device" else "0")
                    run = subprocess.run([app, cfg, str(x - size // 2), str(y - size // 2), str(size), str(size)] + paths, capture_output=True, text=True,
                                         env=env, timeout=300)
                    if run.returncode != 0:
                        sys.exit("tracker_app failed: " + run.stderr[-500:])
                    lines = [l.split() for l in run.stdout.splitlines() if l.startswith("frame ")]
                    if any(t[11] != route for t in lines):
                        sys.exit("tracker_app took another route than %s" % route)
                    times[route].append([float(t[13]) for t in lines[5:]])
            for route, per_round in times.items():
                flat = np.concatenate(per_round)
                medians = [float(np.median(r)) for r in per_round]
                out["routes"][route][str(n)] = dict(ms_median=float(np.median(flat)), ms_p10=float(np.percentile(flat, 10)), ms_p90=float(np.percentile(flat, 90)),
                                                    round_medians_min=min(medians), round_medians_max=max(medians))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resident_tracker_probe: no GPU; a frame time cannot be measured without one")
    print(json.dumps(run_host(a.frames, a.rounds) if a.host else run(a.frames, a.warmup, a.rounds)))
