"""fd_particles (the resident particle set of the Condensation tracker) against tests/condensation_model.py.  The integer outputs --
selected indices, sample fields, windows, target flags, the extracted state -- are compared bit for bit; weights, which go through
the device's exp, in units in the last place.  176 x 144 frames, cell 4, a window of 3 x 4 cells, two layers per octave."""
import math

import numpy as np
import pytest

import condensation_model as model
import ehog_model

pytestmark = pytest.mark.gpu

W, H, CELL, OLC, COLS, ROWS, MAXW = 176, 144, 4, 2, 3, 4, 100
ASPECT = ROWS / COLS
LOGISTIC_A, LOGISTIC_B, SVM_THRESHOLD, REJECTION = 0.25, -1.5, 0.0, -0.125
# The device's exp is not libm's.  Measured on an MI355X over every weight these tests and tests/test_gpu_condensation_host_app.py
# compare (test_weigh: 2 ulp over 237 weights in each mode; the chains of 65 and 300: 2 ulp; the two routes of tracker_app: 1, 2 and 2 ulp):
# at most 2 ulp between the device and libm.  Asserted: that maximum plus one.
WEIGHT_ULP_BOUND = 3


def _blob_frame(k):
    """noise with a textured 30 x 40 blob that moves 3 px right and 2 px down per frame"""
    rng = np.random.default_rng(99)
    frame = rng.integers(90, 130, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:40, 0:30]
    blob = (128 + 100 * np.sin(xx / 2.5) * np.cos(yy / 3.5)).astype(np.uint8)
    x0, y0 = 60 + 3 * k, 40 + 2 * k
    frame[y0:y0 + 40, x0:x0 + 30] = blob[:, :, None]
    return frame


class Scene:
    def __init__(self, capi, ctx):
        fp = capi.cehog_params(cell_size=CELL, bin_count=18, signed_gradients=True, unsigned_gradients=True, interpolate_bins=False,
                               interpolate_cells=True, alpha=0.2)
        self.prm = capi.ehog_tracker_params(fp, COLS, ROWS, OLC, COLS * CELL, MAXW)
        self.tracker = capi.EhogTracker(ctx, self.prm)
        self.frames = [_blob_frame(k) for k in range(6)]
        self.tracker.update(self.frames[0])
        # a linear model that answers to the blob: its own features, centred
        self.box = (60 + 15, 40 + 20, 30, 40)
        valid, feat = self.tracker.extract_patches([self.box])
        assert valid[0]
        w = feat[0] - feat[0].mean()
        self.weights = (w / np.abs(w).sum() * 8).astype(np.float32)
        self.bias = float(0.5 * (self.weights * feat[0]).sum())
        self.tracker.set_svm(self.weights, self.bias)
        self.layers = ehog_model.plan_layers(W, H, COLS, CELL, COLS * CELL, MAXW, OLC)

    def xywh(self, gen):
        size = gen["size"].astype(np.int64)
        return np.stack([gen["x"], gen["y"], gen["size"], [model.cv_round(ASPECT * int(s)) for s in size]], 1).astype(np.int32)


@pytest.fixture(scope="module")
def scene(capi, ctx):
    return Scene(capi, ctx)


def _same_generation(got, want, fields=model.FIELDS):
    for k in fields:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g != w)
            raise AssertionError("%s: %d of %d differ, first at %d: %r != %r" % (k, len(bad), g.size, bad[0], g[bad[0]], w[bad[0]]))


def _old_generation(n, seed):
    rng = np.random.default_rng(seed)
    return model.generation(x=rng.integers(0, W, n), y=rng.integers(0, H, n), size=rng.integers(8, 90, n), vx=rng.integers(-4, 5, n),
                            vy=rng.integers(-4, 5, n), vsize=rng.choice(np.array([1.0, 0.9, 1.1, 0.97, 1.3, 0.7], np.float32), n),
                            weight=rng.random(n), score=rng.standard_normal(n), target=rng.integers(0, 2, n), cluster_id=rng.integers(0, 5, n))


def _draws(count, n_resampled, seed):
    rng = np.random.default_rng(seed)
    diffusion = np.stack([3.0 * rng.standard_normal(n_resampled), 3.0 * rng.standard_normal(n_resampled),
                          [math.pow(2, 0.1 * z) for z in rng.standard_normal(n_resampled)]], 1).reshape(n_resampled, 3)
    if n_resampled > 3:   # exact halves: std::round goes away from zero
        diffusion[0, :2] = (0.5, -0.5)
        diffusion[1, :2] = (1.5, -2.5)
        diffusion[2] = (0.0, 0.0, 1.0)
    fresh = np.stack([rng.integers(0, W, count - n_resampled), rng.integers(0, H, count - n_resampled), rng.integers(8, 90, count - n_resampled)], 1)
    return diffusion, fresh.astype(np.int32).reshape(-1, 3)


def _weight_vectors(n, seed):
    rng = np.random.default_rng(seed)
    out = {"seeded": rng.random(n), "equal": np.ones(n), "all-zero": np.zeros(n)}
    dominant = np.full(n, 1e-3)
    dominant[n // 2] = 100.0
    out["dominant"] = dominant
    ends = rng.random(n)
    ends[:max(1, n // 8)] = 0
    ends[n - max(1, n // 8):] = 0
    out["zero-ends"] = ends
    return out


@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("n_old,count", [(1, 1), (2, 5), (64, 64), (65, 33), (257, 300), (1000, 1000), (8192, 8192)])
def test_sample_equals_the_model(capi, ctx, scene, n_old, count, rate):
    particles = capi.Particles(ctx, scene.tracker, max(n_old, count))
    n_resampled = model.resampled_count(count, rate)
    old = _old_generation(n_old, n_old * 7 + count)
    diffusion, fresh = _draws(count, n_resampled, count + 1)
    for name, weights in _weight_vectors(n_old, n_old).items():
        old["weight"] = weights.astype(np.float64)
        u = 0.0 if name == "equal" else 0.37
        particles.set(**old)
        particles.sample(count, n_resampled, u, diffusion, fresh, 1000)
        want, source = model.sample(old, count, n_resampled, u, diffusion, fresh, 1000)
        got = particles.get()
        copies = n_resampled if n_resampled and model.weight_sum(weights) / n_resampled > 0 else 0
        assert len(particles) == len(want["x"]) == copies + count - n_resampled, name
        assert copies == n_resampled or name in ("all-zero", "zero-ends")
        _same_generation(got, want)
        assert np.array_equal(particles.trace(windows=False)[0], source), name
        if name == "equal" and n_resampled == n_old >= 3:   # pointers land on the sums: strict > takes sample 0 twice, the last never
            assert source[:3].tolist() == [0, 0, 1] and source.max() == n_old - 2, (source[:4], source.max())
        if name == "dominant" and n_resampled > 2:
            assert (source[:n_resampled] == n_old // 2).sum() > n_resampled // 2
    particles.close()


def test_sample_arguments(capi, ctx, scene):
    for capacity in (0, -1, capi.FD_PARTICLES_MAX + 1):
        with pytest.raises(capi.FdError) as e:
            capi.Particles(ctx, scene.tracker, capacity)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    particles = capi.Particles(ctx, scene.tracker, 16)
    assert particles.capacity == 16 and len(particles) == 0
    old = _old_generation(16, 3)
    particles.set(**old)
    for count, n_resampled in ((17, 4), (8, 9), (8, -1)):
        with pytest.raises(capi.FdError) as e:
            particles.sample(count, n_resampled, 0.5, np.ones((16, 3)), np.ones((17, 3), np.int32), 0)
        assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError):
        particles.set(**_old_generation(17, 3))
    _same_generation(particles.get(), old)   # refused calls change nothing
    particles.sample(0, 0, 0.5, np.zeros((0, 3)), np.zeros((0, 3), np.int32), 0)
    assert len(particles) == 0
    info = particles.state()
    assert info["found"] == 0 and info["count"] == 0 and info["n_target"] == 0 and info["weight_sum"] == 0.0
    particles.sample(5, 4, 0.5, np.ones((4, 3)), np.full((5, 3), 20, np.int32), 7)   # no old sample: no copies, one fresh sample
    got = particles.get()
    assert len(got["x"]) == 1 and got["cluster_id"][0] == 7 and got["size"][0] == 20
    particles.close()


def _evaluation_samples(scene, patches):
    """seeded samples, off-image and zero-sized ones, and both sides of every width at which the layer changes"""
    rng = np.random.default_rng(17 + patches)
    n = 200
    rows = np.stack([rng.integers(-10, W + 10, n), rng.integers(-10, H + 10, n), rng.integers(4, 120, n)], 1).tolist()
    rows += [(-40, 20, 30), (W + 40, 20, 30), (80, -60, 30), (80, H + 60, 30), (80, 70, 0), (80, 70, -3), (80, 70, 1), (80, 70, 4000), (80, 70, 2 ** 30)]
    last = None
    for size in range(1, 260):
        win = model.window(88, 72, size, ASPECT, scene.layers, COLS, ROWS, CELL, OLC, patches)
        layer = None if win is None else win[0]
        if layer != last:
            rows += [(88, 72, size - 1), (88, 72, size), (70, 60, size - 1), (70, 60, size)]
        last = layer
    return np.array(rows, np.int64)


@pytest.mark.parametrize("patches", [0, 1], ids=["heat", "patches"])
def test_evaluate_equals_the_host_entry_points(capi, ctx, scene, patches):
    scene.tracker.update(scene.frames[0])
    s = _evaluation_samples(scene, patches)
    particles = capi.Particles(ctx, scene.tracker, len(s))
    gen = model.generation(len(s), x=s[:, 0], y=s[:, 1], size=s[:, 2])
    particles.set(**gen)
    particles.evaluate(patches, ASPECT)
    _, windows, valid = particles.trace()
    got = particles.get()
    xywh = scene.xywh(gen)
    if patches:
        host_valid, _, host_score = scene.tracker.extract_patches(xywh, want_score=True)
    else:
        host_valid, host_score = scene.tracker.evaluate_samples(xywh)
        host_score = host_score.astype(np.float64)
    assert np.array_equal(valid, host_valid)
    assert got["score"].tobytes() == host_score.tobytes()
    assert 0 < valid.sum() < len(s)
    layers_seen = set()
    for i, (x, y, size) in enumerate(s):
        win = model.window(x, y, size, ASPECT, scene.layers, COLS, ROWS, CELL, OLC, patches)
        assert windows[i].tolist() == ([0, 0, 0, 0] if win is None else [win[0], win[1], win[2], 1]), (i, x, y, size)
        if win is not None:
            layers_seen.add(win[0])
    assert len(layers_seen) >= 2
    _same_generation(got, gen, [k for k in model.FIELDS if k != "score"])   # evaluate changes the scores only
    particles.close()


@pytest.mark.parametrize("mode", [model.TARGET_LOST, model.SLIDING_WINDOW, model.ALL_TARGETS], ids=["lost", "sliding", "all"])
def test_weigh(capi, ctx, scene, mode):
    scene.tracker.update(scene.frames[0])
    s = _evaluation_samples(scene, 0)
    particles = capi.Particles(ctx, scene.tracker, len(s))
    gen = model.generation(len(s), x=s[:, 0], y=s[:, 1], size=s[:, 2], weight=np.random.default_rng(5).random(len(s)) * 2)
    particles.set(**gen)
    particles.evaluate(0, ASPECT)
    valid = particles.trace(windows=False)[2]
    scores = particles.get()["score"]
    particles.weigh(LOGISTIC_A, LOGISTIC_B, SVM_THRESHOLD, mode, REJECTION)
    got = particles.get()
    want, best = model.weigh(gen, valid, scores, LOGISTIC_A, LOGISTIC_B, SVM_THRESHOLD, mode, REJECTION)
    _same_generation(got, want, [k for k in model.FIELDS if k != "weight"])
    assert not got["weight"][valid == 0].any() and not got["target"][valid == 0].any()
    ulps = model.ulp_distance(got["weight"], want["weight"])
    print("k_particles_weigh against math.exp: max %d ulp over %d weights" % (max(ulps), len(ulps)))
    assert max(ulps) <= WEIGHT_ULP_BOUND
    info = particles.state()
    assert info["best_score"] == best and info["n_valid"] == int(valid.sum()) and info["n_target"] == int(got["target"].sum())
    assert info["n_target"] <= info["n_valid"] and info["n_valid"] > 0
    particles.close()


def _check_state(particles, gen):
    particles.set(**gen)
    info = particles.state()
    device = particles.get()
    want = model.filtered_state(device)
    assert info["count"] == len(gen["x"]) and info["n_target"] == int(np.asarray(gen["target"]).astype(bool).sum())
    assert info["weight_sum"] == model.weight_sum(device["weight"])
    if want is None:
        assert info["found"] == 0
    else:
        assert info["found"] == 1
        assert (info["x"], info["y"], info["size"], info["vx"], info["vy"]) == want[:5] and np.float32(info["vsize"]) == want[5]
    return info, want


@pytest.mark.parametrize("n", [1, 2, 65, 257, 1000, 8192])
def test_state_equals_the_model(capi, ctx, scene, n):
    particles = capi.Particles(ctx, scene.tracker, n)
    gen = _old_generation(n, 100 + n)
    info, want = _check_state(particles, gen)
    if n >= 65:
        assert want is not None
    gen["cluster_id"] = np.random.default_rng(n).integers(-2 ** 31 + 1, 2 ** 31 - 1, n).astype(np.int32)   # every sample its own cluster, any id
    _check_state(particles, gen)
    gen["target"][:] = 0
    info, want = _check_state(particles, gen)
    assert want is None and info["n_target"] == 0
    particles.close()


def test_state_special_cases(capi, ctx, scene):
    particles = capi.Particles(ctx, scene.tracker, 512)
    # zero weight sum in the winning cluster
    gen = model.generation(6, x=[10, 20, 30, 40, 50, 60], y=[5] * 6, size=[20] * 6, weight=[0, 0, 0, 1, 1, 0], target=[1] * 6, cluster_id=[4, 4, 4, 9, 9, 4])
    info, want = _check_state(particles, gen)
    assert want is None and info["cluster_id"] == 4
    # a tie: the cluster whose first member comes first
    gen = model.generation(4, x=[10, 20, 30, 40], y=[1, 2, 3, 4], size=[20] * 4, weight=[1, 1, 1, 3], target=[1] * 4, cluster_id=[7, 3, 3, 7])
    info, want = _check_state(particles, gen)
    assert info["cluster_id"] == 7 and want[:2] == (33, 3)   # (10 + 3 * 40) / 4 + 0.5, (1 + 3 * 4) / 4 + 0.5
    # the samples without the target flag do not count: cluster 3 has three members, two of them targets
    gen = model.generation(5, x=[10, 20, 30, 40, 50], y=[0] * 5, size=[20] * 5, target=[1, 1, 1, 1, 0], cluster_id=[3, 7, 7, 3, 3])
    info, want = _check_state(particles, gen)
    assert info["cluster_id"] == 3 and want[0] == 25
    # 300 clusters of one and one of two, hidden in the middle
    ids = np.arange(302, dtype=np.int32) * 37 - 5000
    ids[200] = ids[100]
    rng = np.random.default_rng(8)
    gen = model.generation(302, x=rng.integers(0, W, 302), y=rng.integers(0, H, 302), size=rng.integers(8, 90, 302), weight=rng.random(302),
                           target=np.ones(302), cluster_id=ids, vsize=np.full(302, 0.4, np.float32))
    info, want = _check_state(particles, gen)
    assert info["cluster_id"] == ids[100] and want[5] == 0   # a mean size factor of 0.4 is truncated to 0
    particles.close()


@pytest.mark.parametrize("bad", [-1e-300, float("nan"), float("inf")], ids=["negative", "nan", "inf"])
def test_bad_weights_raise_the_flag(capi, ctx, scene, bad):
    scene.tracker.update(scene.frames[0])
    particles = capi.Particles(ctx, scene.tracker, 300)
    gen = _old_generation(300, 12)
    gen["weight"][137] = bad
    gen["x"][137], gen["y"][137], gen["size"][137] = scene.box[:3]   # a sample with a window: its product is bad as well
    particles.set(**gen)
    with pytest.raises(capi.FdError) as e:
        particles.state()
    assert e.value.code == capi.FD_ERR_RUNTIME and e.value.info["bad_weight"] == 1 and e.value.info["found"] == 0
    with pytest.raises(capi.FdError) as e:   # refused on the host: no kernel walks these weights
        particles.sample(300, 300, 0.5, np.ones((300, 3)), np.zeros((0, 3), np.int32), 0)
    assert e.value.code == capi.FD_ERR_RUNTIME
    particles.evaluate(0, ASPECT)
    particles.weigh(LOGISTIC_A, LOGISTIC_B, SVM_THRESHOLD, model.SLIDING_WINDOW, REJECTION)
    got = particles.get()
    assert particles.trace(windows=False)[2][137]
    assert got["weight"].tobytes() == gen["weight"].tobytes()   # the generation is left unweighted
    with pytest.raises(capi.FdError) as e:
        particles.state()
    assert e.value.info["bad_weight"] == 1
    with pytest.raises(capi.FdError):
        particles.sample(300, 300, 0.5, np.ones((300, 3)), np.zeros((0, 3), np.int32), 0)
    particles.set(**_old_generation(300, 12))   # a good generation clears the flag
    assert particles.state()["bad_weight"] == 0
    particles.close()


@pytest.mark.parametrize("n,patches", [(65, 0), (300, 1)], ids=["65-heat", "300-patches"])
def test_six_frame_chain(capi, ctx, scene, n, patches):
    """sample -> evaluate -> weigh -> state over six frames of the moving blob: every frame equals the model stepping on the device's weights"""
    particles = capi.Particles(ctx, scene.tracker, n)
    x, y, size, _ = scene.box
    particles.set(x=np.full(n, x), y=np.full(n, y), size=np.full(n, size), cluster_id=np.full(n, 1))
    rng = np.random.default_rng(n)
    mode = model.ALL_TARGETS if patches else model.SLIDING_WINDOW
    next_id, found, worst = 2, 0, 0
    for k, frame in enumerate(scene.frames):
        scene.tracker.update(frame)
        old = particles.get()
        n_resampled = model.resampled_count(n, 0.2)
        z = rng.standard_normal((n_resampled, 3))
        diffusion = np.stack([4.0 * z[:, 0], 4.0 * z[:, 1], [math.pow(2, 0.05 * v) for v in z[:, 2]]], 1)
        fresh = np.array([model.fresh_sample(rng.random(), 0, 0, 12, MAXW, W, H) for _ in range(n - n_resampled)])
        fresh[:, 0] += rng.integers(0, W - fresh[:, 2] + 1)
        fresh[:, 1] += rng.integers(0, H - fresh[:, 2] + 1)
        u = rng.random()
        particles.sample(n, n_resampled, u, diffusion, fresh, next_id)
        want, source = model.sample(old, n, n_resampled, u, diffusion, fresh, next_id)
        next_id += n - n_resampled
        _same_generation(particles.get(), want)
        assert np.array_equal(particles.trace(windows=False)[0], source)
        particles.evaluate(patches, ASPECT)
        valid = particles.trace(windows=False)[2]
        scores = particles.get()["score"]
        particles.weigh(LOGISTIC_A, LOGISTIC_B, SVM_THRESHOLD, mode, REJECTION)
        device = particles.get()
        weighed, best = model.weigh(want, valid, scores, LOGISTIC_A, LOGISTIC_B, SVM_THRESHOLD, mode, REJECTION)
        _same_generation(device, weighed, [f for f in model.FIELDS if f != "weight"])
        worst = max(worst, max(model.ulp_distance(device["weight"], weighed["weight"])))
        info = particles.state()
        state = model.filtered_state(device)
        assert info["best_score"] == best and info["weight_sum"] == model.weight_sum(device["weight"])
        assert (info["found"] == 1) == (state is not None)
        if state is not None:
            found += 1
            assert (info["x"], info["y"], info["size"], info["vx"], info["vy"]) == state[:5] and np.float32(info["vsize"]) == state[5]
            print("frame %d: state (%d, %d, %d), blob at (%d, %d)" % (k, info["x"], info["y"], info["size"], x + 3 * k, y + 2 * k))
    print("chain of %d: max %d ulp between the device's weights and the model's" % (n, worst))
    assert worst <= WEIGHT_ULP_BOUND and found >= 1
    particles.close()
