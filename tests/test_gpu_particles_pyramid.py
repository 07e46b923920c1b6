"""SingleClassifierModel on the pyramid families for a resident particle set (fd_particles_evaluate_pyramid) on a 96 x 72
seeded gray image.  k_particles_windows resolves every particle to its window on the device; the trace is compared element for element
with the host's fd_pyramid_sample_windows on the mapped list, the scores bit for bit with the host-compacted calls
(fd_hist_svm_evaluate_samples, fd_patch_svm_evaluate_samples: the same kernels on the same rows at another list position), the weights
with tests/resident_model.py in units in the last place (WEIGHT_ULP_BOUND of tests/test_gpu_condensation.py: the device's exp against
libm's), and whole frames with the model chain of tests/condensation_model.py / resident_model.py."""
import math

import numpy as np
import pytest

import condensation_model as cm
import optflow_model as fm
import pyramid_samples_model as psm
import resident_model as model
from test_gpu_condensation import WEIGHT_ULP_BOUND, _same_generation

pytestmark = pytest.mark.gpu

W, H, ASPECT = 96, 72, 1.25
PW, PH = 12, 20                                             # the smaller patch of tests/test_gpu_pyramid_samples.py
PYR = dict(octave_layers=3, min_scale=0.3, max_scale=1.0)   # six kept layers, 96 x 72 down to 30 x 23; index 3 has scale 0.5 exactly
SCALE = float(np.float32(1.1))                              # the apps read the scale as a float
MAPS = {"none": [], "resize": [("resize", SCALE, 0.1, -0.05)]}
LOGISTIC_A, LOGISTIC_B = 0.3, -1.7
INT32_MAX = 2 ** 31 - 1
N = 257


def _height(size):
    return model.cv_round(ASPECT * int(size))


def particle_rows(layers, inc, n=N):
    """{x, y, size}: make_samples' list for the layer and border edges (its samples are squares: y is moved so that y - height / 2 stays
    what it was), then empty, negative and huge sizes, windows one pixel outside a layer next to their neighbours inside, products that
    land on .5, and seeded ones that hang over every border"""
    rows = []
    for x, y, width, _ in psm.make_samples(layers, inc, PW, PH).tolist():
        rows.append((x, y - psm.c_div2(width) + psm.c_div2(_height(width)), width))
    rows += [(40, 40, 0), (40, 40, -9), (40, 40, 4000), (40, 40, INT32_MAX), (-3, 30, 24), (30, -70, 24)]
    L = layers[2]
    width = int(round(PW / L["scale"]))
    for bx in (-1, 0, L["w"] - PW, L["w"] - PW + 1):    # bx = -1 | 0 and bx + patch_w = lw | lw + 1
        x, y, _, _ = psm.window_sample(L, PW, bx, 3)
        rows.append((x, y - psm.c_div2(width) + psm.c_div2(_height(width)), width))
    for offset in (5, 7, 1):                            # layers[3] has scale 0.5: an odd x - width / 2 lands on .5; 2.5 -> 2, 3.5 -> 4, 0.5 -> 0
        rows.append((offset + 24 // 2, 8 + _height(24) // 2, 24))
    rng = np.random.default_rng(11)
    rest = np.stack([rng.integers(-5, W + 5, n), rng.integers(-5, H + 5, n), rng.integers(10, 44, n)], 1).tolist()
    return np.array((rows + rest)[:n], np.int64)


def check_rows(layers, inc, rows):
    """the conditions of the fixture that do not need the device, on the rule's restatement"""
    xywh = np.array([(x, y, s, _height(s)) for x, y, s in rows.tolist()], np.int64)
    want = psm.sample_windows(layers, inc, PW, PH, xywh)
    ok = want[:, 3] == 1
    assert ok.sum() >= 20 and (~ok).sum() >= 7 and set(want[ok, 0].tolist()) == set(range(len(layers)))
    assert (xywh[:, 2] != xywh[:, 3]).any()
    L = layers[2]
    edge = [i for i, (x, y, s, h) in enumerate(xywh.tolist()) if s == int(round(PW / L["scale"]))]
    bxs = {psm.cv_round((xywh[i, 0] - psm.c_div2(int(xywh[i, 2]))) * L["scale"]): bool(ok[i]) for i in edge}
    assert bxs[-1] is False and bxs[0] is True and bxs[L["w"] - PW] is True and bxs[L["w"] - PW + 1] is False
    assert layers[3]["scale"] == 0.5
    halves = [(xywh[i, 0] - 12) * 0.5 for i in range(len(xywh)) if xywh[i, 2] == 24 and ok[i] and (xywh[i, 0] - 12) % 2 == 1]
    assert {2.5, 3.5, 0.5} <= set(halves)
    for i in range(len(xywh)):
        if xywh[i, 2] == 24 and ok[i] and (xywh[i, 0] - 12) * 0.5 in (2.5, 3.5, 0.5):
            assert want[i, 1] == {2.5: 2, 3.5: 4, 0.5: 0}[(xywh[i, 0] - 12) * 0.5]
    return want, ok


def make_image(seed=20261021):
    rng = np.random.default_rng(seed)
    return np.clip(np.kron(rng.integers(40, 216, (H // 4, W // 4)), np.ones((4, 4))) + rng.integers(-30, 30, (H, W)), 0, 255).astype(np.uint8)


def _pyramid(capi, ctx, image, kind=None, **kw):
    p = capi.Pyramid(ctx, **PYR)
    if kind is not None:
        p.set_layer_filter(kind, **kw)
    p.update(image)
    return p


@pytest.fixture(scope="module")
def scene(capi, ctx, synth):
    """the image's pyramids, and per feature kind its pyramid, its parameters (as keyword of evaluate_pyramid), the host-compacted call
    and a linear SVM on the rows of the default mapped list"""
    image = make_image()
    gray = _pyramid(capi, ctx, image)
    gradbin = _pyramid(capi, ctx, image, capi.FD_LAYER_GRADBIN, bins=9, interpolate=False)
    lbp = _pyramid(capi, ctx, image, capi.FD_LAYER_LBP, lbp_type=2)
    layers = gray.layers()
    assert 4 <= len(layers) <= 6 and [(l["w"], l["h"]) for l in layers] == [(l["w"], l["h"]) for l in gradbin.layers()]
    rows = particle_rows(layers, gray.inc)
    assert len(rows) == N
    check_rows(layers, gray.inc, rows)
    gen = cm.generation(N, x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    xywh = model.sample_xywh(gen, ASPECT)
    hist = lambda prm: (lambda p, svm, s: capi.hist_svm_evaluate_samples(ctx, p, prm, svm, s, want_distance=True))
    patch = lambda prm: (lambda p, svm, s: capi.patch_svm_evaluate_samples(ctx, p, prm, svm, s, want_distance=True))
    hog = capi.hist_params(0, PW, PH, 1, 1, bins=9, cell=6, block=2, cell_h=5)
    codes = capi.hist_params(1, PW, PH, 1, 1, bins=16, cell=6, block=1, normalization=2, cell_h=5)
    ehog = capi.ehog_patch_params(PW, PH, bins=9, cell_w=6, cell_h=5)
    spaces = {name: capi.patch_samples_params(PW, PH, getattr(capi, "FD_FEATURE_" + name), 1.0 / 127.5, -1.0) for name in ("GRAY", "HISTEQ", "WHI")}
    kinds = {
        "hist-hog": dict(pyr=gradbin, kw=dict(hist=hog), host=hist(hog), extract=lambda s: capi.hist_extract_samples(ctx, gradbin, hog, s)),
        "hist-lbp": dict(pyr=lbp, kw=dict(hist=codes), host=hist(codes), extract=lambda s: capi.hist_extract_samples(ctx, lbp, codes, s)),
        "ehog": dict(pyr=gradbin, kw=dict(ehog=ehog), host=hist(ehog), extract=lambda s: capi.ehog_extract_samples(ctx, gradbin, ehog, s)),
    }
    for name, pp in spaces.items():
        kinds["patch-" + name] = dict(pyr=gray, kw=dict(patch=pp), host=patch(pp), extract=lambda s, pp=pp: capi.patch_extract_samples(ctx, gray, pp, s))
    out = dict(image=image, gray=gray, gradbin=gradbin, lbp=lbp, rows=rows, gen=gen, xywh=xywh, kinds=kinds)
    for name, k in kinds.items():
        mapped = capi.sample_maps_apply(MAPS["resize"], xywh)
        host = k["pyr"].sample_windows(PW, PH, mapped)
        assert 20 <= host[:, 3].sum() <= N - 7, (name, host[:, 3].sum())     # the condition of the fixture, on the host's own rule
        feats, valid = k["extract"](mapped)
        assert np.array_equal(valid, host[:, 3] == 1)
        m = synth.make_svm_f32(5, feats[valid], nsv=12, positive_fraction=0.4, kernel=0)
        m["logistic_a"], m["logistic_b"] = LOGISTIC_A, LOGISTIC_B
        k["model"], k["svm"] = m, capi.Svm(ctx, m)
    yield out
    for p in (gray, gradbin, lbp):
        p.close()


# ---- 1. windows
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("maps", sorted(MAPS))
def test_windows_equal_the_host_rule(capi, ctx, scene, maps, n):
    k = scene["kinds"]["patch-GRAY"]
    rows = scene["rows"][:n]
    if n == 1:
        rows = scene["rows"][3:4]
    gen = cm.generation(n, x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    particles = capi.Particles.unbound(ctx, n)
    particles.set(**gen)
    particles.evaluate_pyramid(k["pyr"], k["svm"], ASPECT, MAPS[maps], **k["kw"])
    _, windows, valid = particles.trace()
    mapped = capi.sample_maps_apply(MAPS[maps], model.sample_xywh(gen, ASPECT))
    assert np.array_equal(mapped, model.apply_maps(MAPS[maps], model.sample_xywh(gen, ASPECT)))
    want = k["pyr"].sample_windows(PW, PH, mapped)
    assert np.array_equal(windows, want), np.flatnonzero((windows != want).any(1))[:5]
    assert np.array_equal(valid, want[:, 3].astype(np.uint8))
    if n == 257:
        assert want[:, 3].sum() >= 20 and (want[:, 3] == 0).sum() >= 7 and (want[want[:, 3] == 0] == (-1, 0, 0, 0)).all()
        if maps == "none":
            assert np.array_equal(want, check_rows(k["pyr"].layers(), k["pyr"].inc, scene["rows"])[0])
    particles.close()


# ---- 2. scores and weights
@pytest.mark.parametrize("kind", ["hist-hog", "hist-lbp", "ehog", "patch-GRAY", "patch-HISTEQ", "patch-WHI"])
def test_evaluate_and_weigh(capi, ctx, scene, kind):
    k = scene["kinds"][kind]
    pyr, svm, m = k["pyr"], k["svm"], k["model"]
    rng = np.random.default_rng(4)
    gen = {f: v.copy() for f, v in scene["gen"].items()}
    gen["weight"] = rng.random(N) * 3          # weights other than 1: the classifier sets the weight, it does not multiply
    gen["cluster_id"] = rng.integers(0, 4, N).astype(np.int32)
    mapped = capi.sample_maps_apply(MAPS["resize"], scene["xywh"])
    particles = capi.Particles.unbound(ctx, N)
    particles.set(**gen)
    particles.evaluate_pyramid(pyr, svm, ASPECT, MAPS["resize"], **k["kw"])
    _, windows, valid = particles.trace()
    got = particles.get()
    want = pyr.sample_windows(PW, PH, mapped)
    assert np.array_equal(windows, want) and np.array_equal(valid, want[:, 3].astype(np.uint8))
    ok = valid.astype(bool)
    host_target, host_weight, host_distance = k["host"](pyr, svm, mapped)
    assert got["score"][ok].tobytes() == host_distance[ok].tobytes()                      # the same kernel on the same rows
    assert np.unique(host_distance[ok]).size > ok.sum() // 2
    _same_generation(got, gen, [f for f in cm.FIELDS if f != "score"])                    # evaluate changes the scores only
    scores = np.where(ok, got["score"], 0.0)
    threshold = float(scores[np.flatnonzero(ok)[5]])                                      # a score exactly on the threshold
    for thr in (float(np.float32(m["threshold"])), threshold):
        particles.set(**gen)
        particles.evaluate_pyramid(pyr, svm, ASPECT, MAPS["resize"], **k["kw"])
        particles.weigh_classifier(LOGISTIC_A, LOGISTIC_B, thr)
        device = particles.get()
        wanted, best = model.weigh_classifier(gen, valid, scores, LOGISTIC_A, LOGISTIC_B, thr)
        _same_generation(device, wanted, [f for f in cm.FIELDS if f != "weight"])
        ulps = cm.ulp_distance(device["weight"], wanted["weight"])
        print("%s, threshold %r: max %d ulp over %d weights" % (kind, thr, max(ulps), N))
        assert max(ulps) <= WEIGHT_ULP_BOUND
        assert not device["weight"][~ok].any() and not device["score"][~ok].any()
        if thr == threshold:
            assert device["target"][np.flatnonzero(ok)[5]] == 1 and scores[np.flatnonzero(ok)[5]] == thr
        info = particles.state()
        assert info["best_score"] == best and info["n_valid"] == int(ok.sum()) and info["n_target"] == int(device["target"].sum())
        assert 0 < info["n_target"] <= info["n_valid"]
        if thr != threshold:   # the host's SingleClassifierModel on the same list
            assert np.array_equal(device["target"].astype(bool), host_target)
            assert max(cm.ulp_distance(device["weight"], host_weight)) <= WEIGHT_ULP_BOUND
    particles.close()


# ---- 3. no window anywhere
def test_no_window_anywhere(capi, ctx, scene):
    k = scene["kinds"]["patch-GRAY"]
    small = capi.Pyramid(ctx, octave_layers=3, min_scale=0.1, max_scale=0.2)   # every layer lower than the patch
    small.update(scene["image"])
    assert small.layers() and all(l["h"] < PH for l in small.layers())
    invalid = scene["rows"][~(scene["kinds"]["patch-GRAY"]["pyr"].sample_windows(PW, PH, scene["xywh"])[:, 3] == 1)]
    assert len(invalid) >= 7
    for pyr, rows in ((small, scene["rows"]), (k["pyr"], invalid)):
        n = len(rows)
        particles = capi.Particles.unbound(ctx, n)
        particles.set(x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
        particles.evaluate_pyramid(pyr, k["svm"], ASPECT, [], **k["kw"])
        _, windows, valid = particles.trace()
        assert not valid.any() and (windows == (-1, 0, 0, 0)).all()
        particles.weigh_classifier(LOGISTIC_A, LOGISTIC_B, -1e300)
        device = particles.get()
        assert not device["weight"].any() and not device["target"].any() and not device["score"].any()
        info = particles.state()
        assert info["found"] == 0 and info["n_valid"] == 0 and info["count"] == n
        particles.close()
    small.close()


# ---- 4. frames
def _target_svm(capi, ctx, k, box):
    """a linear model that answers to the target: its own features, centred; the threshold at half its own score"""
    feat, valid = k["extract"](box)
    assert valid[0]
    w = feat[0] - feat[0].mean()
    svm = capi.Svm(ctx, dict(kernel=0, dtype=1, sv=w[None, :].astype(np.float32), coeff=np.ones(1, np.float32), bias=np.float32(0)))
    own = float(svm.distance(feat)[0])
    assert own > 0
    return svm, 0.5 * own, 2.0, -4.0 / own


def _draws(rng, n, n_resampled, deviation=2.0, size_deviation=0.04):
    z = rng.standard_normal((n_resampled, 3))
    diffusion = np.stack([deviation * z[:, 0], deviation * z[:, 1], [math.pow(2, size_deviation * v) for v in z[:, 2]]], 1)
    fresh = np.array([cm.fresh_sample(rng.random(), 0, 0, 14, 44, W, H) for _ in range(n - n_resampled)])
    fresh[:, 0] += rng.integers(0, W - fresh[:, 2] + 1)
    fresh[:, 1] += rng.integers(0, H - fresh[:, 2] + 1)
    return diffusion, fresh, rng.random()


def _check_frame(capi, k, pyr, svm, want, windows, valid, scores, device, info, logistic, threshold):
    """the evaluated, weighed generation and its state against the model chain, fed with the host call's distances"""
    mapped = capi.sample_maps_apply(MAPS["resize"], model.sample_xywh(want, ASPECT))
    host = pyr.sample_windows(PW, PH, mapped)
    assert np.array_equal(windows, host) and np.array_equal(valid, host[:, 3].astype(np.uint8))
    ok = valid.astype(bool)
    _, _, distance = k["host"](pyr, svm, mapped)
    assert scores[ok].tobytes() == distance[ok].tobytes() and not distance[~ok].any()
    weighed, best = model.weigh_classifier(want, valid, distance, logistic[0], logistic[1], threshold)
    _same_generation(device, weighed, [f for f in cm.FIELDS if f != "weight"])
    worst = max(cm.ulp_distance(device["weight"], weighed["weight"]))
    assert worst <= WEIGHT_ULP_BOUND
    state = cm.filtered_state(device)
    assert info["best_score"] == best and info["weight_sum"] == cm.weight_sum(device["weight"]) and info["n_valid"] == int(ok.sum())
    assert (info["found"] == 1) == (state is not None)
    if state is not None:
        assert (info["x"], info["y"], info["size"], info["vx"], info["vy"]) == state[:5] and np.float32(info["vsize"]) == state[5]
    return state, int(ok.sum())


def test_two_frames(capi, ctx, scene):
    k = scene["kinds"]["hist-hog"]
    pyr = k["pyr"]
    x, y, size = 48, 36, 30
    svm, threshold, a, b = _target_svm(capi, ctx, k, capi.sample_maps_apply(MAPS["resize"], [(x, y, size, _height(size))]))
    particles = capi.Particles.unbound(ctx, N)
    particles.set(x=np.full(N, x), y=np.full(N, y), size=np.full(N, size), cluster_id=np.full(N, 1))
    rng = np.random.default_rng(N)
    n_resampled = cm.resampled_count(N, 0.2)
    next_id, found = 2, 0
    for frame in range(2):
        old = particles.get()
        diffusion, fresh, u = _draws(rng, N, n_resampled)
        particles.sample(N, n_resampled, u, diffusion, fresh, next_id)
        sampled = particles.get()
        particles.evaluate_pyramid(pyr, svm, ASPECT, MAPS["resize"], **k["kw"])
        _, windows, valid = particles.trace()
        scores = particles.get()["score"]
        particles.weigh_classifier(a, b, threshold)
        device = particles.get()
        info = particles.state()
        want, _ = cm.sample(old, N, n_resampled, u, diffusion, fresh, next_id)
        next_id += N - n_resampled
        _same_generation(sampled, want)
        state, n_valid = _check_frame(capi, k, pyr, svm, want, windows, valid, scores, device, info, (a, b), threshold)
        assert 20 <= n_valid < N
        found += state is not None
    assert found >= 1
    particles.close()


def test_a_flow_frame(capi, ctx):
    """track_fb_resident -> sample_flow -> evaluate_pyramid -> weigh_classifier -> state_flow on a texture moved by (2, 1)"""
    base = fm.textured(W, H, seed=31)
    frames = [base, np.roll(base, (1, 2), axis=(0, 1))]
    pp = capi.patch_samples_params(PW, PH, capi.FD_FEATURE_HISTEQ, 1.0 / 127.5, -1.0)
    pyr = capi.Pyramid(ctx, **PYR)
    k = dict(kw=dict(patch=pp), host=lambda p, svm, s: capi.patch_svm_evaluate_samples(ctx, p, pp, svm, s, want_distance=True),
             extract=lambda s: capi.patch_extract_samples(ctx, pyr, pp, s))
    flow = capi.Flow(ctx, W, H)
    x, y, size = 48, 36, 30
    pyr.update(frames[0])
    flow.update(frames[0])
    svm, threshold, a, b = _target_svm(capi, ctx, k, capi.sample_maps_apply(MAPS["resize"], [(x, y, size, _height(size))]))
    particles = capi.Particles.unbound(ctx, N)
    particles.set(x=np.full(N, x), y=np.full(N, y), size=np.full(N, size), cluster_id=np.full(N, 1))
    rng = np.random.default_rng(5)
    n_resampled = cm.resampled_count(N, 0.2)
    pyr.update(frames[1])
    flow.update(frames[1])
    old = particles.get()
    flow_d, fresh, u = _draws(rng, N, n_resampled)
    fall_d, _, _ = _draws(rng, N, n_resampled, 3.0, 0.05)
    flow.track_fb_resident(model.chain_points(x, y, size, ASPECT))
    particles.sample_flow(flow, N, n_resampled, u, flow_d, fall_d, fresh, 2)
    sampled = particles.get()
    particles.evaluate_pyramid(pyr, svm, ASPECT, MAPS["resize"], **k["kw"])
    _, windows, valid = particles.trace()
    scores = particles.get()["score"]
    particles.weigh_classifier(a, b, threshold)
    device = particles.get()
    info, motion = particles.state_flow(flow)   # the frame's one read-back
    assert motion["ok"]
    want, _ = model.sample_flow(old, motion, N, n_resampled, u, flow_d, fall_d, fresh, 2)
    _same_generation(sampled, want)
    _, n_valid = _check_frame(capi, k, pyr, svm, want, windows, valid, scores, device, info, (a, b), threshold)
    assert 20 <= n_valid < N
    particles.close()
    flow.close()
    pyr.close()


# ---- 5. arguments
def test_arguments(capi, ctx, synth, scene):
    k = scene["kinds"]["hist-hog"]
    pyr, svm, kw = k["pyr"], k["svm"], k["kw"]
    rows = scene["rows"][:8]
    particles = capi.Particles.unbound(ctx, 8)
    particles.set(x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    before = particles.get()

    def refused(call, code, match=""):
        with pytest.raises(capi.FdError) as e:
            call()
        assert e.value.code == code and match in str(e.value), e.value
        with pytest.raises(capi.FdError) as e:   # refused calls evaluate nothing
            particles.weigh_classifier(0.0, -1.0, 0.0)
        assert e.value.code == capi.FD_ERR_RUNTIME and "not been evaluated" in str(e.value)
        _same_generation(particles.get(), before)

    bad = capi.FD_ERR_INVALID_ARGUMENT
    refused(lambda: particles.evaluate_pyramid(pyr, svm, ASPECT, [("integral",)], **kw), bad, "FD_SAMPLE_MAP_RESIZE")
    refused(lambda: particles.evaluate_pyramid(pyr, svm, ASPECT, [("resize", 1.1)] * 5, **kw), bad, "sample maps")
    length = k["model"]["sv"].shape[1]
    u8 = np.random.default_rng(1).integers(0, 256, (16, length)).astype(np.uint8)
    refused(lambda: particles.evaluate_pyramid(pyr, capi.Svm(ctx, synth.make_svm_u8(3, u8, nsv=8, calib=u8, positive_fraction=0.5)), ASPECT, [], **kw), bad, "f32")
    refused(lambda: particles.evaluate_pyramid(pyr, scene["kinds"]["ehog"]["svm"], ASPECT, [], **kw), bad, "f32 vectors of length %d" % length)
    refused(lambda: particles.evaluate_pyramid(scene["lbp"], svm, ASPECT, [], **kw), bad, "gradient bin image")       # HOG on codes
    refused(lambda: particles.evaluate_pyramid(pyr, scene["kinds"]["patch-GRAY"]["svm"], ASPECT, [], **scene["kinds"]["patch-GRAY"]["kw"]), bad,
            "gray pyramid")                                                                                        # gray patches on bin images
    multi = capi.Pyramid(ctx, **PYR)
    multi.set_frames(2)
    multi.update_frames(images=[scene["image"], scene["image"]])
    refused(lambda: particles.evaluate_pyramid(multi, scene["kinds"]["patch-GRAY"]["svm"], ASPECT, [], **scene["kinds"]["patch-GRAY"]["kw"]), bad, "frames")
    other = capi.Context(0)
    foreign = capi.Pyramid(other, **PYR)
    foreign.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9, interpolate=False)
    foreign.update(scene["image"])
    refused(lambda: particles.evaluate_pyramid(foreign, svm, ASPECT, [], **kw), bad, "different contexts")
    fresh = capi.Pyramid(ctx, **PYR)   # never updated
    fresh.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9, interpolate=False)
    refused(lambda: particles.evaluate_pyramid(fresh, svm, ASPECT, [], **kw), capi.FD_ERR_RUNTIME, "not been updated with an image")
    with pytest.raises(ValueError):
        particles.evaluate_pyramid(pyr, svm, ASPECT, [])
    # an empty generation goes through the whole chain
    particles.sample(0, 0, 0.5, np.zeros((0, 3)), np.zeros((0, 3), np.int32), 0)
    particles.evaluate_pyramid(pyr, svm, ASPECT, MAPS["resize"], **kw)
    particles.weigh_classifier(0.0, -1.0, 0.0)
    info = particles.state()
    assert info["count"] == 0 and info["found"] == 0 and info["n_valid"] == 0
    # the evaluated call itself, last: the set works after every refusal
    particles.set(x=rows[:, 0], y=rows[:, 1], size=rows[:, 2])
    particles.evaluate_pyramid(pyr, svm, ASPECT, [], **kw)
    particles.weigh_classifier(LOGISTIC_A, LOGISTIC_B, 0.0)
    assert particles.state()["n_valid"] == int(pyr.sample_windows(PW, PH, model.sample_xywh(before, ASPECT))[:, 3].sum())
    for p in (multi, foreign, fresh):
        p.close()
    particles.close()
