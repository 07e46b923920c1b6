"""The arithmetic the resident particle set adds for the integral-feature models and the optical-flow transition, on
top of tests/condensation_model.py and tests/optflow_model.py: the wrapper chain of a feature extractor as maps of a sample
(PatchResizingFeatureExtractor.hpp:41-52, IntegralFeatureExtractor.hpp:36-47), SingleClassifierModel's weighing (.cpp:32-42), the
median flow stated without a sort (what k_flow_motion computes: the correct set by its predicate, every median an order statistic of
a multiset) and OpticalFlowTransitionModel::predict inside ResamplingSampler::sample.  Python floats are IEEE doubles, np.float32
scalars floats, one operation at a time.  Also the frames the chain tests share.  It never calls the library under test."""
import numpy as np

import condensation_model as cm
import optflow_model as fm

F = np.float32
RESIZE, INTEGRAL = "resize", "integral"
MAX_MAPS = 4
MAX_POINTS = 1024


# ---------------------------------------------------------------- the wrapper chain

def cv_round(v):
    """cvRound of a double: to the nearest, halves to even; outside the int range it saturates, a NaN gives 0 (fd_sample_maps_apply)"""
    v = np.float64(v)
    if v != v:
        return 0
    return int(np.clip(np.rint(v), -2 ** 31, 2 ** 31 - 1))


def map_resize(sample, factor, x_offset=0.0, y_offset=0.0):
    """PatchResizingFeatureExtractor: cvRound of double sums and products, in this order"""
    x, y, w, h = (int(v) for v in sample)
    return (cv_round(x + float(x_offset) * w), cv_round(y + float(y_offset) * h), cv_round(float(factor) * w), cv_round(float(factor) * h))


def map_integral(sample):
    """IntegralFeatureExtractor: one pixel wider and higher, moved by one where the size is odd"""
    x, y, w, h = (int(v) for v in sample)
    return (x + (0 if w % 2 == 0 else 1), y + (0 if h % 2 == 0 else 1), w + 1, h + 1)


def apply_maps(maps, samples):
    """maps: ("resize", factor[, x_offset[, y_offset]]) and ("integral",) from the outermost wrapper in; samples (n, 4) -> int32 (n, 4)"""
    out = []
    for s in np.asarray(samples, np.int64).reshape(-1, 4):
        s = tuple(int(v) for v in s)
        for m in maps:
            s = map_resize(s, *m[1:]) if m[0] == RESIZE else map_integral(s)
        out.append(s)
    return np.array(out, np.int32).reshape(-1, 4)


def sample_xywh(gen, aspect):
    """the samples of a generation as the measurement model sees them: height = cvRound(aspect * size) (Sample.hpp:127-129)"""
    return np.array([(int(x), int(y), int(s), cv_round(aspect * int(s))) for x, y, s in zip(gen["x"], gen["y"], gen["size"])], np.int32).reshape(-1, 4)


# ---------------------------------------------------------------- SingleClassifierModel

def weigh_classifier(gen, valid, scores, a, b, threshold):
    """SingleClassifierModel::evaluate on every sample: the weight is the probability, not a product.  (generation, best score)"""
    out = {k: v.copy() for k, v in gen.items()}
    best = cm.LOWEST
    for i in range(len(valid)):
        if not valid[i]:
            out["weight"][i], out["score"][i], out["target"][i] = 0.0, 0.0, 0
        else:
            s = float(scores[i])
            out["weight"][i] = cm.probability(s, a, b)
            out["score"][i] = s
            out["target"][i] = s >= threshold
        best = max(best, float(out["score"][i]))
    return out, best


# ---------------------------------------------------------------- the median flow, without a sort

def motion(points, fwd, bwd, fstatus, bstatus):
    """fd_flow_median's values as k_flow_motion forms them: dict(ok, n_valid, n_correct, median_x, median_y, median_ratio)"""
    points, fwd, bwd = (np.asarray(a, np.float32).reshape(-1, 2) for a in (points, fwd, bwd))
    n = len(points)
    out = dict(ok=False, n_valid=0, n_correct=0, median_x=F(0), median_y=F(0), median_ratio=F(1))
    with np.errstate(all="ignore"):
        status = np.asarray(fstatus).astype(bool) & np.asarray(bstatus).astype(bool)
        dx, dy = bwd[:, 0] - points[:, 0], bwd[:, 1] - points[:, 1]
        d = dx * dx + dy * dy
        valid = status & (d == d)
        correct = valid & ~(d > F(0.5))
        out["n_valid"] = int(valid.sum())
        if out["n_valid"] < n // 2:
            return out
        m = int(correct.sum())
        out["n_correct"] = m
        if m < n // 2 or m < 2:
            return out
        p, f = points[correct], fwd[correct]
        out["median_x"] = np.sort(f[:, 0] - p[:, 0])[m // 2]          # np.sort puts NaN last, as the host's comparison does
        out["median_y"] = np.sort(f[:, 1] - p[:, 1])[m // 2]
        a, b = np.triu_indices(m, 1)
        before, after = p[a] - p[b], f[a] - f[b]
        ratios = (after[:, 0] * after[:, 0] + after[:, 1] * after[:, 1]) / (before[:, 0] * before[:, 0] + before[:, 1] * before[:, 1])
        out["median_ratio"] = np.sqrt(np.sort(ratios)[len(ratios) // 2])
        out["ok"] = True
    return out


def same_float(a, b):
    """bit-identical floats; any two NaN count as the same (the device reports the default NaN)"""
    a, b = F(a), F(b)
    return bool((a != a and b != b) or a.tobytes() == b.tobytes())


def same_motion(got, want):
    return (bool(got["ok"]) == bool(want["ok"]) and got["n_valid"] == want["n_valid"] and got["n_correct"] == want["n_correct"]
            and all(same_float(got[k], want[k]) for k in ("median_x", "median_y", "median_ratio")))


# ---------------------------------------------------------------- the flow prediction inside the sampler

def predict_flow(x, y, size, median_x, median_y, median_ratio, dx, dy, factor):
    """OpticalFlowTransitionModel::apply (.cpp:173-190); dx = positionDeviation * z, factor = pow(2, sizeDeviation * z)"""
    nvx = cm.std_round(float(F(median_x)) + dx)
    nvy = cm.std_round(float(F(median_y)) + dy)
    nvs = F(float(F(median_ratio)) * factor)
    nsize = cm.std_round(float(F(F(int(size)) * nvs)))
    return int(x) + nvx, int(y) + nvy, nsize, nvx, nvy, nvs


def sample_flow(old, mot, count, n_resampled, u, flow_diffusion, fallback_diffusion, fresh, first_fresh_cluster_id):
    """ResamplingSampler::sample whose transition model is OpticalFlowTransitionModel with a SimpleTransitionModel fallback, given the
    motion and both blocks of draws: (new generation, source index per sample)"""
    if not mot["ok"]:
        return cm.sample(old, count, n_resampled, u, fallback_diffusion, fresh, first_fresh_cluster_id)
    picks = cm.low_variance_indices(old["weight"], n_resampled, u)
    rows, source = [], []
    for i, k in enumerate(picks):
        x, y, size, vx, vy, vs = predict_flow(old["x"][k], old["y"][k], old["size"][k], mot["median_x"], mot["median_y"], mot["median_ratio"],
                                              *flow_diffusion[i])
        rows.append((x, y, size, vx, vy, vs, 1.0, 0.0, 0, int(old["cluster_id"][k])))
        source.append(k)
    for j in range(count - n_resampled):
        rows.append((int(fresh[j][0]), int(fresh[j][1]), int(fresh[j][2]), 0, 0, F(1), 1.0, 0.0, 0, first_fresh_cluster_id + j))
        source.append(-1)
    new = {k: np.array([r[c] for r in rows], cm.DTYPES[k]) for c, k in enumerate(cm.FIELDS)}
    return new, np.array(source, np.int32)


# ---------------------------------------------------------------- crafted tracks for the motion tests

def crafted_tracks(n, seed, n_valid=None, n_correct=None, shift=(1.5, -0.75), zoom=1.03):
    """n points of a 200 x 200 area whose forward positions are a zoom about the centre plus a shift plus noise; the first n_correct
    (default all) come back within 0.1 px, the next up to n_valid (default all) come back 2 px off, the rest have a status byte
    cleared.  The points are shuffled.  (points, fwd, bwd float32 (n, 2), fstatus, bstatus uint8 (n,))"""
    rng = np.random.default_rng(seed)
    n_valid = n if n_valid is None else n_valid
    n_correct = n_valid if n_correct is None else n_correct
    pts = rng.uniform(0, 200, (n, 2)).astype(np.float32)
    fwd = ((pts - F(100)) * F(zoom) + F(100) + np.array(shift, np.float32) + rng.normal(0, 0.2, (n, 2)).astype(np.float32)).astype(np.float32)
    bwd = (pts + rng.uniform(-0.07, 0.07, (n, 2)).astype(np.float32)).astype(np.float32)
    bwd[n_correct:] += F(2)
    fst, bst = np.ones(n, np.uint8), np.ones(n, np.uint8)
    off = np.arange(n_valid, n)
    fst[off[::2]] = 0
    bst[off[1::2]] = 0
    order = rng.permutation(n)
    return pts[order], fwd[order], bwd[order], fst[order], bst[order]


# ---------------------------------------------------------------- the frames of the chain tests

CHAIN_W, CHAIN_H, CHAIN_SHIFT, CHAIN_UNRELATED = 96, 80, (2, 1), 3
CHAIN_TARGET = (48, 40, 40)   # x, y, size of the tracked square in frame 0


def chain_frames(count=6):
    """gray 96 x 80 frames: a seeded texture moved by (2, 1) per frame (a circular roll, so an exact shift), frame 3 an unrelated
    texture"""
    base = fm.textured(CHAIN_W, CHAIN_H, seed=31)
    other = fm.textured(CHAIN_W, CHAIN_H, seed=77)
    return [other if k == CHAIN_UNRELATED else np.roll(base, (CHAIN_SHIFT[1] * k, CHAIN_SHIFT[0] * k), axis=(0, 1)) for k in range(count)]


def chain_points(x, y, size, aspect=1.0):
    """the 10 x 10 circle grid on a target"""
    return fm.target_points(fm.grid(10, 10, True), x, y, size, cv_round(aspect * size))
