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

  python tools/resident_tracker_probe.py [--frames 60] [--warmup 10] [--rounds 5] [--counts 100,1000,8192]
  python tools/resident_tracker_probe.py --pyramid hog|ehog|glbp|whi
                 the same two routes with the measurement on a pyramid feature type (20 x 20 patches of a pyramid with five layers per
                 octave between the scales 0.1 and 0.5; a linear SVM): the pyramid's update in place of fd_integral_update on both
                 routes, fd_hist_svm_evaluate_samples / fd_patch_svm_evaluate_samples on the generic one (resolves the windows on the
                 host, uploads the compacted list, waits), fd_particles_evaluate_pyramid on the resident one.  With --host:
                 tracker_app on `feature hog|ehog|glbp|whi` with `transition simple` (the host trackers take the device route on
                 these feature types with that transition model only)
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


PATCH = 20
PYRAMID = dict(octave_layers=5, min_scale=0.1, max_scale=0.5)


class IntegralMeasurement:
    """the default: `ihog` behind scale 1.1 on an integral image"""

    def __init__(self, capi, ctx):
        self.capi, self.integral = capi, capi.Integral(ctx)
        hist = capi.hist_params(kind=capi.HIST_SPATIAL, pw=G, ph=G, sx=1, sy=1, bins=BINS, cell=6, block=1, normalization=1)
        self.hp = capi.integral_hog_params(G, G, bins=BINS, interpolate_bins=True, hist=hist)
        self.maps = [("resize", float(np.float32(1.1))), ("integral",)]

    def update(self, frame):
        self.integral.update_device(frame.data_ptr(), W, H, 1)

    def features(self, xywh):
        return self.integral.extract_hog(self.hp, self.capi.sample_maps_apply(self.maps, xywh))

    def evaluate_host(self, svm, xywh):
        self.integral.svm_evaluate_samples(svm, self.capi.sample_maps_apply(self.maps, xywh), hog=self.hp)

    def evaluate_resident(self, particles, svm):
        particles.evaluate_integral(self.integral, svm, 1.0, self.maps, hog=self.hp)

    def close(self):
        self.integral.close()


class PyramidMeasurement:
    """--pyramid: a DirectPyramidFeatureExtractor's chain, not wrapped"""

    def __init__(self, capi, ctx, kind):
        self.capi, self.ctx, self.pyr = capi, ctx, capi.Pyramid(ctx, **PYRAMID)
        self.kw = None
        if kind in ("hog", "ehog"):
            self.pyr.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=BINS)
        elif kind == "glbp":
            self.pyr.set_layer_filter(capi.FD_LAYER_GRADMAG_LBP, lbp_type=1, grad_kernel=3, blur_kernel=3)
        if kind == "hog":
            self.kw = dict(hist=capi.hist_params(kind=capi.HIST_SPATIAL, pw=PATCH, ph=PATCH, sx=1, sy=1, bins=BINS, cell=5, block=1, normalization=2))
        elif kind == "glbp":
            self.kw = dict(hist=capi.hist_params(kind=capi.HIST_SPATIAL, pw=PATCH, ph=PATCH, sx=1, sy=1, bins=59, cell=5, block=1, normalization=2))
        elif kind == "ehog":
            self.kw = dict(ehog=capi.ehog_patch_params(PATCH, PATCH, bins=BINS, cell_w=5))
        else:
            self.kw = dict(patch=capi.patch_samples_params(PATCH, PATCH, capi.FD_FEATURE_WHI))
        self.prm = list(self.kw.values())[0]

    def update(self, frame):
        self.pyr.update_device(frame.data_ptr(), W, H, 1)

    def features(self, xywh):
        if "patch" in self.kw:
            return self.capi.patch_extract_samples(self.ctx, self.pyr, self.prm, xywh)
        extract = self.capi.ehog_extract_samples if "ehog" in self.kw else self.capi.hist_extract_samples
        return extract(self.ctx, self.pyr, self.prm, xywh)

    def evaluate_host(self, svm, xywh):
        if "patch" in self.kw:
            self.capi.patch_svm_evaluate_samples(self.ctx, self.pyr, self.prm, svm, xywh)
        else:
            self.capi.hist_svm_evaluate_samples(self.ctx, self.pyr, self.prm, svm, xywh)

    def evaluate_resident(self, particles, svm):
        particles.evaluate_pyramid(self.pyr, svm, 1.0, (), **self.kw)

    def close(self):
        self.pyr.close()


def run(frames_per_round, warmup, rounds, counts=COUNTS, pyramid=None):
    from featuredetection_amd import capi
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    base = textured(5)
    cycle = 8   # the texture moves by SHIFT per frame and jumps back every `cycle` frames (one frame without a usable flow)
    frames = [torch.from_numpy(np.roll(base, (SHIFT[1] * k, SHIFT[0] * k), axis=(0, 1)).copy()).cuda() for k in range(cycle)]
    torch.cuda.synchronize()
    x, y, size = TARGET
    pts_of = lambda k: (capi.flow_grid(10, 10, True) * np.float32(size) + np.array([x + SHIFT[0] * k, y + SHIFT[1] * k], np.float32)).astype(np.float32)
    out = dict(size="%dx%d" % (W, H), feature=pyramid or "ihog", frames_per_round=frames_per_round, rounds=rounds, grid_points=int(len(pts_of(0))),
               routes={})
    with torch.cuda.stream(stream):
        flow = capi.Flow(ctx, W, H)
        measurement = PyramidMeasurement(capi, ctx, pyramid) if pyramid else IntegralMeasurement(capi, ctx)
        measurement.update(frames[0])
        feat, valid = measurement.features(np.array([(x, y, size, size)], np.int32))
        assert valid[0]
        w = feat[0] - feat[0].mean()
        svm = capi.Svm(ctx, dict(kernel=0, dtype=1, sv=w[None, :].astype(np.float32), coeff=np.ones(1, np.float32), bias=np.float32(0)))
        own = float(svm.distance(feat)[0])
        threshold, logistic_a, logistic_b = 0.5 * own, 2.0, -4.0 / own
        for n in counts:
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
                measurement.update(frames[k % cycle])
                fwd, bwd, fst, bst = flow.track_fb(pts)
                motion = capi.flow_median(pts, fwd, bwd, fst, bst)
                measurement.evaluate_host(svm, xywh)
                t1 = time.perf_counter()
                used["generic"] += bool(motion["ok"])
                return t1 - t0

            def resident_frame():
                k = turn["resident"] = turn["resident"] + 1
                d0, d1, fresh, u = draws(), draws(), fresh_samples(), rng.random()
                pts = pts_of((k - 1) % cycle)
                t0 = time.perf_counter()
                flow.update(frames[k % cycle])
                measurement.update(frames[k % cycle])
                flow.track_fb_resident(pts)
                particles.sample_flow(flow, n, n_resampled, u, d0, d1, fresh, next_id[0])
                measurement.evaluate_resident(particles, svm)
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
        measurement.close()
        torch.cuda.synchronize()
    ctx.close()
    return out


HOST_CONFIG = """tracking {
  seed 7
  transition %(transition)s
  adaptive { resampling { particleCount %(n)d randomRate 0.35 minSize 40 maxSize 200 } }
  initialCount %(n)d
  measurement positionDependent {
    %(feature)s
    filter none  startFrameCount 1  stopFrameCount 0  targetThreshold 0.1  confidenceThreshold 0.95
    positiveOffsetFactor 0.05  negativeOffsetFactor 0.5  sampleNegativesAroundTarget 2  sampleAdditionalNegatives 10  sampleTestNegatives 10
    exploitSymmetry 0
    classifier { training { type libSvm c 1 compensateImbalance 0 negativeCapacity 100 } logisticA 0.00556 logisticB -2.95 threshold 0 }
  }
}
"""


# the host trackers take the device route on a pyramid feature type with `transition simple` only
HOST_TRANSITIONS = {False: "opticalFlow { positionDeviation 10 sizeDeviation 0.08 fallback simple { positionDeviation 12.8 sizeDeviation 0.1 } }",
                    True: "simple { positionDeviation 12.8 sizeDeviation 0.1 }"}
HOST_PYRAMID = "pyramid direct { patch { width 20 height 20 minWidth 40 maxWidth 200 } interval 5 }"
HOST_FEATURES = {
    None: """feature ihog { scale 1.1  signed false  interpolate true  bins 9  gradientCount 30
                   histogram spatial { cellSize 6  blockSize 1  interpolate false  normalization l2norm } }""",
    "hog": "feature hog { %s gradientKernel 3 blurKernel 0 bins 9 signed 0 interpolate 0 histogram spatial { cellSize 5 blockSize 2 interpolate 0 "
           "signedAndUnsigned 0 concatenate 0 normalization l2hys } }" % HOST_PYRAMID,
    "ehog": "feature ehog { %s gradientKernel 3 blurKernel 0 bins 9 signed 0 interpolate 0 histogram { cellSize 5 interpolate 0 signedAndUnsigned 0 "
            "alpha 0.2 } }" % HOST_PYRAMID,
    "glbp": "feature glbp { %s gradientKernel 3 blurKernel 3 type lbp8uniform histogram spatial { cellSize 5 blockSize 1 interpolate 0 concatenate 0 "
            "normalization l2hys } }" % HOST_PYRAMID,
    "whi": "feature whi { %s }" % HOST_PYRAMID,
}


def run_host(frames, rounds, counts=COUNTS, pyramid=None):
    import subprocess
    import tempfile
    app = os.path.join(ROOT, "featuredetection_amd", "tracker_app")
    out = dict(size="%dx%d" % (W, H), feature=pyramid or "ihog", frames=frames, rounds=rounds, routes={"generic": {}, "device": {}})
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
        for n in counts:
            cfg = os.path.join(tmp, "tracking%d.cfg" % n)
            with open(cfg, "w") as f:
                f.write(HOST_CONFIG % dict(n=n, feature=HOST_FEATURES[pyramid], transition=HOST_TRANSITIONS[pyramid is not None]))
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
    ap.add_argument("--pyramid", choices=("hog", "ehog", "glbp", "whi"), default=None)
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS), help="particle counts, comma separated")
    a = ap.parse_args()
    counts = tuple(int(c) for c in a.counts.split(","))
    if not torch.cuda.is_available():
        sys.exit("resident_tracker_probe: no GPU; a frame time cannot be measured without one")
    print(json.dumps(run_host(a.frames, a.rounds, counts, a.pyramid) if a.host else run(a.frames, a.warmup, a.rounds, counts, a.pyramid)))
    torch.cuda.synchronize()
