"""The arithmetic of the Condensation tracker's frame loop in Python floats (IEEE double) and numpy float32, operation for operation
as libCondensation has it: LowVarianceSampling::resample (.cpp:20-46), SimpleTransitionModel::predict (.cpp:25-44),
ResamplingSampler::sample (.cpp:50-59), GridSampler::sample (.cpp:37-53), FilteringStateExtractor + WeightedMeanStateExtractor
(.cpp:23-62), MaxWeightStateExtractor, ExtendedHogBasedMeasurementModel's weighting (.cpp:173-205) and the sample -> window rules (through
ehog_model).  Every random number is an input.  A generation of samples is a dict of equally long lists / arrays keyed like FIELDS.

Deviations from the reference that the library makes and this model states: the resampling walk stops at the last sample where
rounding leaves a pointer above the total weight; of equally large clusters the one whose first member has the lowest index wins."""
import math

import numpy as np

import ehog_model

F32 = np.float32
FIELDS = ("x", "y", "size", "vx", "vy", "vsize", "weight", "score", "target", "cluster_id")
DTYPES = dict(x=np.int32, y=np.int32, size=np.int32, vx=np.int32, vy=np.int32, vsize=np.float32, weight=np.float64, score=np.float64,
              target=np.uint8, cluster_id=np.int32)
TARGET_LOST, SLIDING_WINDOW, ALL_TARGETS = 0, 1, 2
LOWEST = -1.7976931348623157e308

std_round = ehog_model.std_round
cv_round = ehog_model.cv_round


def generation(n=0, **fields):
    """a generation of n samples: velocity 0, size factor 1, weight 1, score 0, no target flag, cluster 0 unless given"""
    default = dict(x=0, y=0, size=0, vx=0, vy=0, vsize=1, weight=1, score=0, target=0, cluster_id=0)
    return {k: np.array(fields[k], DTYPES[k]) if k in fields else np.full(n, default[k], DTYPES[k]) for k in FIELDS}


def weight_sum(weights):
    """computeWeightSum: added up in index order"""
    s = 0.0
    for w in weights:
        s = s + float(w)
    return s


def low_variance_indices(weights, count, u):
    """the index in `weights` of each of the `count` copies (none without samples or with a step that is not positive)"""
    if len(weights) == 0 or count <= 0:
        return []
    step = weight_sum(weights) / count
    if not step > 0:
        return []
    start = step * u
    out, k, running = [], 0, float(weights[0])
    for i in range(count):
        pointer = start + i * step
        while pointer > running and k + 1 < len(weights):   # the reference has no second condition: it walks off the end
            k += 1
            running = running + float(weights[k])
        out.append(k)
    return out


def predict(x, y, size, vx, vy, vsize, dx, dy, factor):
    """one sample through SimpleTransitionModel::predict; dx = positionDeviation * z, factor = pow(2, sizeDeviation * z)"""
    nvx = std_round(float(vx) + dx)
    nvy = std_round(float(vy) + dy)
    nvs = F32(float(F32(vsize)) * factor)
    nsize = std_round(float(F32(F32(int(size)) * nvs)))   # int * float: a float product, rounded as a float
    return int(x) + nvx, int(y) + nvy, nsize, nvx, nvy, nvs


def resampled_count(count, random_rate):
    return int((1 - random_rate) * count)


def sample(old, count, n_resampled, u, diffusion, fresh, first_fresh_cluster_id):
    """ResamplingSampler::sample given its draws: (new generation, source index per sample, -1 for a fresh one).  When no copy can be
    made the new generation holds the count - n_resampled fresh samples only (the caller who wants `count` of them asks for that)."""
    picks = low_variance_indices(old["weight"], n_resampled, u)
    rows, source = [], []
    for i, k in enumerate(picks):
        x, y, size, vx, vy, vs = predict(old["x"][k], old["y"][k], old["size"][k], old["vx"][k], old["vy"][k], old["vsize"][k], *diffusion[i])
        rows.append((x, y, size, vx, vy, vs, 1.0, 0.0, 0, int(old["cluster_id"][k])))
        source.append(k)
    for j in range(count - n_resampled):
        rows.append((int(fresh[j][0]), int(fresh[j][1]), int(fresh[j][2]), 0, 0, F32(1), 1.0, 0.0, 0, first_fresh_cluster_id + j))
        source.append(-1)
    new = {k: np.array([r[c] for r in rows], DTYPES[k]) for c, k in enumerate(FIELDS)}
    return new, np.array(source, np.int32)


def fresh_sample(size_draw, x_draw, y_draw, min_size, max_size, width, height):
    """ResamplingSampler::sampleValues (.cpp:61-71) from a uniform real in [0, 1) and the two uniform ints it asks for: (x, y, size)"""
    size = cv_round((size_draw * (float(max_size) / float(min_size) - 1.0) + 1.0) * min_size)
    return x_draw + ehog_model.int_div(size, 2), y_draw + ehog_model.int_div(size, 2), size


def grid_samples(width, height, min_size, max_size, size_scale, step_size):
    """GridSampler::sample: [(x, y, size)]; `size *= sizeScale` is an int times a float, truncated"""
    out = []
    size = min_size
    while size <= max_size:
        half = size // 2
        step = int(F32(F32(step_size) * F32(size)) + F32(0.5))
        for x in range(half, width - size + half, step):
            for y in range(half, height - size + half, step):
                out.append((x, y, size))
        size = int(F32(size) * F32(size_scale))
    return out


def probability(score, a, b):
    """ProbabilisticSvmClassifier::getProbability (.cpp:54-58)"""
    f = a + b * score
    return math.exp(-f) / (1.0 + math.exp(-f)) if f >= 0 else 1.0 / (1.0 + math.exp(f))


def weigh(gen, valid, scores, a, b, svm_threshold, mode, rejection_threshold):
    """ExtendedHogBasedMeasurementModel::scored on every sample: (generation, best score as evaluate(image, samples) keeps it)"""
    out = {k: v.copy() for k, v in gen.items()}
    best = LOWEST
    for i in range(len(valid)):
        if not valid[i]:
            out["weight"][i], out["score"][i], out["target"][i] = 0.0, 0.0, 0
        else:
            s = float(scores[i])
            out["weight"][i] = float(gen["weight"][i]) * probability(s, a, b)
            out["score"][i] = s
            out["target"][i] = s >= svm_threshold if mode == TARGET_LOST else (s > rejection_threshold if mode == SLIDING_WINDOW else True)
        best = max(best, float(out["score"][i]))
    return out, best


def largest_cluster(cluster_ids, members):
    """of the samples `members` (indices, ascending): the id of the largest cluster; of equally large ones the cluster met first"""
    counts, order = {}, []
    for i in members:
        c = int(cluster_ids[i])
        if c not in counts:
            counts[c] = 0
            order.append(c)
        counts[c] += 1
    best = None
    for c in order:
        if best is None or counts[c] > counts[best]:
            best = c
    return best


def weighted_mean_state(gen, members=None):
    """WeightedMeanStateExtractor::extract on the samples `members` (all by default): (x, y, size, vx, vy, vsize) or None"""
    members = list(range(len(gen["x"]))) if members is None else list(members)
    winner = largest_cluster(gen["cluster_id"], members)
    if winner is None:
        return None
    sx = sy = ss = svx = svy = svs = sw = 0.0
    for i in members:
        if int(gen["cluster_id"][i]) != winner:
            continue
        w = float(gen["weight"][i])
        sx = sx + w * int(gen["x"][i])
        sy = sy + w * int(gen["y"][i])
        ss = ss + w * int(gen["size"][i])
        svx = svx + w * int(gen["vx"][i])
        svy = svy + w * int(gen["vy"][i])
        svs = svs + w * float(F32(gen["vsize"][i]))
        sw = sw + w
    if sw == 0:
        return None
    return (int(sx / sw + 0.5), int(sy / sw + 0.5), int(ss / sw + 0.5), int(svx / sw + 0.5), int(svy / sw + 0.5), F32(int(svs / sw + 0.5)))


def filtered_state(gen):
    """FilteringStateExtractor(WeightedMeanStateExtractor)"""
    return weighted_mean_state(gen, [i for i in range(len(gen["x"])) if gen["target"][i]])


def max_weight_state(gen):
    """MaxWeightStateExtractor (.cpp:18-30): the first sample of the largest positive weight if it has the target flag, (x, y, size,
    vx, vy, vsize) or None"""
    best, max_weight = None, 0.0
    for i in range(len(gen["x"])):
        if float(gen["weight"][i]) > max_weight:
            max_weight, best = float(gen["weight"][i]), i
    if best is None or not gen["target"][best]:
        return None
    return tuple(gen[k][best] for k in ("x", "y", "size", "vx", "vy", "vsize"))


def window(x, y, size, aspect, layers, cell_cols, cell_rows, cell_size, octave_layers, patches):
    """the sample -> window rule of the measurement model: (layer, bx, by) or None; the height is cvRound(aspect * size)"""
    rule = ehog_model.patch_window if patches else ehog_model.sample_window
    return rule(int(x), int(y), int(size), cv_round(aspect * int(size)), layers, cell_cols, cell_rows, cell_size, octave_layers)


def ulp_distance(a, b):
    """distance of two float64 arrays in units in the last place (same sign or zero assumed where they differ little)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ia, ib = a.view(np.int64).astype(object), b.view(np.int64).astype(object)
    return np.array([abs(int(p) - int(q)) for p, q in zip(ia.ravel(), ib.ravel())], dtype=object).reshape(a.shape)


def nudge(weights, ulps):
    """every weight moved by `ulps` units in the last place (zero and negative results stay at zero)"""
    w = np.asarray(weights, np.float64).copy()
    for _ in range(abs(ulps)):
        w = np.nextafter(w, np.inf if ulps > 0 else 0.0)
    return w
