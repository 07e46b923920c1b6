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
                 in turns; the app's own per-frame clock around tracker.process, the first 5 frames of a run left out.  --app PATH
                 runs another build's tracker_app (beside its own libraries) in place of this tree's, to compare two builds in one
                 session

  python tools/resident_tracker_probe.py --wvm-svm [--counts 800] [--routes generic,resident]
                 the reference's face tracker (FaceTracking.cpp:73-129): condensation::WvmSvmModel on 20 x 20 HistEq64 patches of a
                 pyramid with five layers per octave for widths 80 .. 480, ResamplingSampler(800, 0.35, LowVarianceSampling,
                 SimpleTransitionModel(10, 0.1)), FilteringStateExtractor(WeightedMeanStateExtractor); a synthetic 280-filter WVM and a
                 1024-vector RBF SVM calibrated on the frames.  generic: the pyramid's update, the sampler on the host,
                 fd_wvm_svm_evaluate_samples (three blocking round trips), the state extraction on the host -- sampler and extraction as
                 vectorised numpy restatements, inside the clock and also reported on their own (host_ms_*: they cost far more than the
                 C++ classes' loops, so the generic figure is a Python baseline, not the host layer's).  resident: the pyramid's
                 update, fd_particles_sample, _evaluate_wvm_svm, _weigh_wvm_svm, fd_particles_state.  --routes generic runs on a library
                 without the resident calls.  With --host: tracker_app on `measurement wvmSvm` with the same models, once per route and
                 round in turns -- the C++ sampler and state extractor on the generic route

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


WVM_SVM_PATCH, WVM_SVM_MIN, WVM_SVM_MAX, WVM_SVM_LAYERS = 20, 80, 480, 5   # DirectPyramidFeatureExtractor(20, 20, 80, 480, 5)


def host_sample(gen, n, n_resampled, u, diffusion, fresh, first_id):
    """ResamplingSampler::sample with LowVarianceSampling and SimpleTransitionModel on arrays (numpy; the draws are given)"""
    cum = np.cumsum(gen["weight"])
    step = cum[-1] / n_resampled
    if step > 0:
        k = np.minimum(np.searchsorted(cum, step * u + np.arange(n_resampled) * step, "left"), len(cum) - 1)
    else:
        k = np.arange(n_resampled) % len(cum)
    vx = np.rint(gen["vx"][k] + diffusion[:, 0]).astype(np.int32)
    vy = np.rint(gen["vy"][k] + diffusion[:, 1]).astype(np.int32)
    vs = (gen["vsize"][k] * diffusion[:, 2]).astype(np.float32)
    size = np.rint(gen["size"][k].astype(np.float32) * vs).astype(np.int32)
    zeros = np.zeros(len(fresh), np.int32)
    return dict(x=np.concatenate([gen["x"][k] + vx, fresh[:, 0]]), y=np.concatenate([gen["y"][k] + vy, fresh[:, 1]]), size=np.concatenate([size, fresh[:, 2]]),
                vx=np.concatenate([vx, zeros]), vy=np.concatenate([vy, zeros]), vsize=np.concatenate([vs, np.ones(len(fresh), np.float32)]),
                cluster=np.concatenate([gen["cluster"][k], first_id + np.arange(len(fresh), dtype=np.int32)]))


def host_state(gen, target, weight):
    """FilteringStateExtractor(WeightedMeanStateExtractor) on arrays (numpy): the weighted mean over the largest cluster of targets"""
    if not target.any():
        return None
    ids, counts = np.unique(gen["cluster"][target], return_counts=True)
    member = target & (gen["cluster"] == ids[np.argmax(counts)])
    w = weight[member]
    total = w.sum()
    if total == 0:
        return None
    return tuple(int(np.dot(w, gen[k][member]) / total + 0.5) for k in ("x", "y", "size", "vx", "vy", "vsize"))


def wvm_svm_pyramid(capi, ctx):
    inc = 0.5 ** (1.0 / WVM_SVM_LAYERS)
    scale_of = lambda width: inc ** round(np.log(WVM_SVM_PATCH / width) / np.log(inc))
    return capi.Pyramid(ctx, octave_layers=WVM_SVM_LAYERS, min_scale=scale_of(WVM_SVM_MAX), max_scale=scale_of(WVM_SVM_MIN))


def wvm_svm_models(synth, layer):
    """the models see what the tracker's windows look like: patches of the pyramid's own first layer"""
    rng = np.random.default_rng(1)
    calib = synth.random_patches(layer, WVM_SVM_PATCH, WVM_SVM_PATCH, 2000, rng)
    wvm = synth.make_wvm(3, calib_patches=calib, min_survivors=200)
    eq = synth.histeq64_np(synth.random_patches(layer, WVM_SVM_PATCH, WVM_SVM_PATCH, 1400, rng))
    return wvm, synth.make_svm_u8(4, eq, nsv=1024, calib=eq[1024:], positive_fraction=0.5)


def run_wvm_svm(frames_per_round, warmup, rounds, counts, routes):
    from featuredetection_amd import capi, synth
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    base = textured(5)
    cycle = 8
    frames = [torch.from_numpy(np.roll(base, (SHIFT[1] * k, SHIFT[0] * k), axis=(0, 1)).copy()).cuda() for k in range(cycle)]
    torch.cuda.synchronize()
    x, y, size = TARGET
    out = dict(size="%dx%d" % (W, H), feature="wvmSvm", frames_per_round=frames_per_round, rounds=rounds, routes={})
    with torch.cuda.stream(stream):
        pyr = wvm_svm_pyramid(capi, ctx)
        pyr.update_device(frames[0].data_ptr(), W, H, 1)
        wvm, svm = wvm_svm_models(synth, pyr.layer(0))
        wg, sg = capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)
        out["wvm_filters"], out["svm_vectors"] = int(wvm["num_filters"]), 1024
        for n in counts:
            rng = np.random.default_rng(n)
            n_resampled = int((1 - RANDOM_RATE) * n)

            def draws():
                z = rng.standard_normal((n_resampled, 3))
                return np.stack([POSITION_DEVIATION * z[:, 0], POSITION_DEVIATION * z[:, 1], np.exp2(SIZE_DEVIATION * z[:, 2])], 1)

            def fresh_samples():
                s = rng.integers(WVM_SVM_MIN, WVM_SVM_MAX + 1, n - n_resampled)
                return np.stack([rng.integers(0, W - s + 1) + s // 2, rng.integers(0, H - s + 1) + s // 2, s], 1).astype(np.int32)

            particles = capi.Particles.unbound(ctx, n) if "resident" in routes else None
            state = dict(turn=0, next_id=2, gen=None, weight=None, positives=0, found=0)
            host_ms = []

            def restart(route):
                state.update(turn=0, next_id=2)
                if route == "resident":
                    particles.set(x=np.full(n, x), y=np.full(n, y), size=np.full(n, size), cluster_id=np.full(n, 1))
                else:
                    state["gen"] = dict(x=np.full(n, x, np.int32), y=np.full(n, y, np.int32), size=np.full(n, size, np.int32), vx=np.zeros(n, np.int32),
                                        vy=np.zeros(n, np.int32), vsize=np.ones(n, np.float32), cluster=np.ones(n, np.int32), weight=np.ones(n))

            def generic_frame():
                k = state["turn"] = state["turn"] + 1
                d, fresh, u = draws(), fresh_samples(), rng.random()
                t0 = time.perf_counter()
                pyr.update_device(frames[k % cycle].data_ptr(), W, H, 1)
                ta = time.perf_counter()
                gen = host_sample(state["gen"], n, n_resampled, u, d, fresh, state["next_id"])
                tb = time.perf_counter()
                target, weight = capi.wvm_svm_evaluate(ctx, pyr, wg, sg, np.stack([gen["x"], gen["y"], gen["size"], gen["size"]], 1))
                tc = time.perf_counter()
                found = host_state(gen, target.astype(bool), weight)
                t1 = time.perf_counter()
                host_ms.append(((tb - ta) + (t1 - tc)) * 1e3)   # the two numpy parts of this frame
                gen["weight"] = weight
                state["gen"] = gen
                state["next_id"] += n - n_resampled
                state["found"] += found is not None
                return t1 - t0

            def resident_frame():
                k = state["turn"] = state["turn"] + 1
                d, fresh, u = draws(), fresh_samples(), rng.random()
                t0 = time.perf_counter()
                pyr.update_device(frames[k % cycle].data_ptr(), W, H, 1)
                particles.sample(n, n_resampled, u, d, fresh, state["next_id"])
                particles.evaluate_wvm_svm(pyr, wg, sg, 1.0)
                particles.weigh_wvm_svm(wg, sg)
                info = particles.state()
                t1 = time.perf_counter()
                state["next_id"] += n - n_resampled
                state["found"] += info["found"]
                return t1 - t0

            step = {"generic": generic_frame, "resident": resident_frame}
            times = {route: [] for route in routes}
            found = {route: 0 for route in routes}
            for r in range(rounds):
                for route in (routes if r % 2 == 0 else routes[::-1]):
                    restart(route)
                    state["found"] = 0
                    for _ in range(warmup):
                        step[route]()
                    times[route].append([step[route]() * 1e3 for _ in range(frames_per_round)])
                    found[route] += state["found"]
            for route, per_round in times.items():
                flat = np.concatenate(per_round)
                medians = [float(np.median(r)) for r in per_round]
                out["routes"].setdefault(route, {})[str(n)] = dict(ms_median=float(np.median(flat)), ms_p10=float(np.percentile(flat, 10)),
                                                                   ms_p90=float(np.percentile(flat, 90)), round_medians_min=min(medians),
                                                                   round_medians_max=max(medians),
                                                                   found_fraction=found[route] / float(rounds * (warmup + frames_per_round)))
            if host_ms:
                out["routes"]["generic"][str(n)].update(host_ms_median=float(np.median(host_ms)), host_ms_p10=float(np.percentile(host_ms, 10)),
                                                        host_ms_p90=float(np.percentile(host_ms, 90)))
            if particles:
                particles.close()
        for h in (wg, sg, pyr):
            h.close()
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


WVM_SVM_HOST_CONFIG = """tracking {
  seed 7
  transition simple { positionDeviation 10 sizeDeviation 0.1 }
  adaptive { resampling { particleCount %(n)d randomRate 0.35 } }
  measurement wvmSvm {
    firstClassifier pwvm { classifierFile %(wvm)s }
    secondClassifier psvm { classifierFile %(svm)s threshold %(threshold)s }
  }
}
"""


# --self-learning: the reference's partiallyAdaptiveTrackingApp graph (its thresholds and its 10 examples per side) on the face tracker's
# models, the self-learning model on hog features of the probe's pyramid
SELF_LEARNING_HOST_CONFIG = """tracking {
  seed 7
  tracker partiallyAdaptive
  transition simple { positionDeviation 10 sizeDeviation 0.1 }
  measurement wvmSvm {
    firstClassifier pwvm { classifierFile %(wvm)s }
    secondClassifier psvm { classifierFile %(svm)s threshold %(threshold)s }
  }
  adaptive selfLearning {
    resampling { particleCount %(n)d randomRate 0.35 }
    positiveThreshold 0.85  negativeThreshold 0.05
    %(feature)s
    classifier { kernel rbf { gamma 0.5 } training { c 1 examples fixedsize positiveExamples 10 negativeExamples 50 minPositiveExamples 3 }
                 probabilistic fixed { logisticA 0.00556 logisticB -2.95 } }
  }
}
"""


def run_host(frames, rounds, counts=COUNTS, pyramid=None, wvm_svm=False, app=None, self_learning=False):
    import subprocess
    import tempfile
    app = app or os.path.join(ROOT, "featuredetection_amd", "tracker_app")
    out = dict(app=os.path.relpath(app, ROOT), size="%dx%d" % (W, H), feature="selfLearning" if self_learning else "wvmSvm" if wvm_svm else pyramid or "ihog", frames=frames, rounds=rounds, routes={"generic": {}, "device": {}})
    with tempfile.TemporaryDirectory() as tmp:
        base = textured(5)
        if wvm_svm:   # the models of run_wvm_svm, in the files the app loads
            from featuredetection_amd import capi, synth
            ctx = capi.Context(0)
            pyr = wvm_svm_pyramid(capi, ctx)
            pyr.update(base)
            wvm, svm = wvm_svm_models(synth, pyr.layer(0))
            pyr.close()
            ctx.close()
            models = dict(wvm=os.path.join(tmp, "face.fdwvm"), svm=os.path.join(tmp, "face.svm.txt"), threshold=repr(float(svm["threshold"])))
            synth.save_wvm(models["wvm"], wvm)
            synth.save_svm_text(models["svm"], svm, rows=WVM_SVM_PATCH, cols=WVM_SVM_PATCH)
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
                if self_learning:
                    f.write(SELF_LEARNING_HOST_CONFIG % dict(models, n=n, feature=HOST_FEATURES["hog"]))
                elif wvm_svm:
                    f.write(WVM_SVM_HOST_CONFIG % dict(models, n=n))
                else:
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
                    if any(t[11] != route for t in lines[5:] if self_learning) or any(t[11] != route for t in lines if not self_learning):
                        sys.exit("tracker_app took another route than %s" % route)   # the self-learning tracker's first frame is generic
                    times[route].append([float(t[-1]) for t in lines[5:]])
                    if self_learning:
                        out.setdefault("adaptive_frames", {})[route] = sum(1 for t in lines[5:] if t[13] == "adaptive")
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
    ap.add_argument("--wvm-svm", action="store_true", help="the face tracker's frame (WvmSvmModel); counts default to 800")
    ap.add_argument("--self-learning", action="store_true", help="through tracker_app: `tracker partiallyAdaptive` (WvmSvmModel + SelfLearningMeasurementModel "
                    "on hog), both routes; counts default to 800, the reference's particle count")
    ap.add_argument("--routes", default="generic,resident", help="with --wvm-svm: the routes to run, comma separated")
    ap.add_argument("--counts", default=None, help="particle counts, comma separated")
    ap.add_argument("--app", default=None, help="with --host: the tracker_app to run (default: this tree's)")
    a = ap.parse_args()
    counts = tuple(int(c) for c in a.counts.split(",")) if a.counts else ((800,) if a.wvm_svm or a.self_learning else COUNTS)
    if not torch.cuda.is_available():
        sys.exit("resident_tracker_probe: no GPU; a frame time cannot be measured without one")
    if a.self_learning:
        print(json.dumps(run_host(a.frames, a.rounds, counts, wvm_svm=True, app=a.app, self_learning=True)))
        sys.exit(0)
    if a.wvm_svm and a.host:
        print(json.dumps(run_host(a.frames, a.rounds, counts, wvm_svm=True, app=a.app)))
        sys.exit(0)
    if a.wvm_svm:
        print(json.dumps(run_wvm_svm(a.frames, a.warmup, a.rounds, counts, tuple(a.routes.split(",")))))
        torch.cuda.synchronize()
        sys.exit(0)
    print(json.dumps(run_host(a.frames, a.rounds, counts, a.pyramid, app=a.app) if a.host else run(a.frames, a.warmup, a.rounds, counts, a.pyramid)))
    torch.cuda.synchronize()
