"""Restatements (numpy, no device) behind the sampled pyramid features and condensation::PositionDependentMeasurementModel:
the sample -> window rule of DirectPyramidFeatureExtractor::extract(x, y, width, height), imageprocessing::GradientMagnitudeFilter
on CV_8UC2 gradients, the glbp layer chain, MT19937 with the model's draw rule, and adapt's sample selection."""
import math

import numpy as np


# ---- the sample -> window rule (DirectPyramidFeatureExtractor.cpp:67-73,134-153, ImagePyramid.hpp:307-310)
def lround(v):
    """std::lround: half away from zero"""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def cv_round(v):
    """cvRound: half to even"""
    f = math.floor(v)
    d = v - f
    if d > 0.5 or (d == 0.5 and f % 2 != 0):
        return int(f) + 1
    return int(f)


def c_div2(v):
    """C's v / 2 for ints: truncation toward zero"""
    return int(v / 2) if v >= 0 else -((-v) // 2)


def sample_windows(layers, inc, pw, ph, xywh):
    """layers: dicts with index, scale, w, h (consecutive indices); xywh (n, 4) -> (n, 4) int32 {layer position, bx, by, valid}"""
    out = np.zeros((len(xywh), 4), np.int32)
    out[:, 0] = -1
    for i, (x, y, width, height) in enumerate(np.asarray(xywh).tolist()):
        if width <= 0 or not layers:
            continue
        index = lround(math.log(float(pw) / float(width)) / math.log(inc))
        real = index - layers[0]["index"]
        if real < 0 or real >= len(layers):
            continue
        L = layers[real]
        bx = cv_round((x - c_div2(width)) * L["scale"])
        by = cv_round((y - c_div2(height)) * L["scale"])
        if bx < 0 or by < 0 or bx + pw > L["w"] or by + ph > L["h"]:
            continue
        out[i] = (real, bx, by, 1)
    return out


def layer_table(width, height, count, inc, first_index=0):
    """`count` consecutive layers of a width x height image: scale inc^k, size cvRound(size * scale) (ImagePyramid.cpp:170-198)"""
    out = []
    for k in range(first_index, first_index + count):
        s = inc ** k
        out.append(dict(index=k, scale=s, w=cv_round(width * s), h=cv_round(height * s)))
    return out


def window_sample(layer, pw, bx, by, odd=0):
    """a sample {x, y, width, height} that the rule maps to the window (bx, by) of `layer` (None when rounding does not allow it);
    width = height = the patch width over the layer's scale (+ odd)"""
    width = int(round(pw / layer["scale"])) + odd
    for x in range(int(bx / layer["scale"]) + c_div2(width) - 2, int(bx / layer["scale"]) + c_div2(width) + 4):
        if cv_round((x - c_div2(width)) * layer["scale"]) == bx:
            for y in range(int(by / layer["scale"]) + c_div2(width) - 2, int(by / layer["scale"]) + c_div2(width) + 4):
                if cv_round((y - c_div2(width)) * layer["scale"]) == by:
                    return (x, y, width, width)
    return None


def make_samples(layers, inc, pw, ph):
    """about 60 samples that hit every category the tests name; the tests assert the categories on the result"""
    s = []
    for L in layers:
        W, H = L["w"] - pw, L["h"] - ph
        if W < 0 or H < 0:
            continue
        for bx, by in ((0, 0), (W, 0), (0, H), (W, H), (W // 2, H // 3), (W // 3, H // 2)):
            for odd in (0, 1):
                v = window_sample(L, pw, bx, by, odd)
                if v is not None and sample_windows(layers, inc, pw, ph, [v])[0, 0] == layers.index(L):
                    s.append(v)
                    break
        # one pixel past each border
        for bx, by in ((-1, H // 2), (W // 2, -1), (W + 1, H // 2), (W // 2, H + 1)):
            v = window_sample(L, pw, bx, by)
            if v is not None:
                s.append(v)
    first, last = layers[0], layers[-1]
    s.append((40, 40, 0, 10))                                           # width <= 0
    s.append((40, 40, -7, -7))
    s.append((60, 48, int(pw / first["scale"] * inc * inc), 10))        # maps before the first kept layer
    s.append((60, 48, int(pw / last["scale"] / inc / inc) + 1, 10))     # ... behind the last
    s.append((3, 2, int(round(pw / layers[1]["scale"])), 9))            # negative x - width / 2
    s.append((-5, -5, int(round(pw / layers[1]["scale"])) + 1, 11))
    s.append(s[0])                                                      # two identical samples
    s.append(s[5])
    return np.array(s, np.int32)


# ---- imageprocessing::GradientMagnitudeFilter, CV_8U branch (GradientMagnitudeFilter.hpp:39-50)
def magnitude_table():
    """s = x^2 + y^2 -> the r with r^2 - r < s <= r^2 + r (the rounded square root; no s is a half-integer square)"""
    s = np.arange(2 * 128 * 128 + 1, dtype=np.int64)
    r = np.zeros_like(s)
    for b in (128, 64, 32, 16, 8, 4, 2, 1):
        t = r + b
        r = np.where(t * t - t < s, t, r)
    return r


_MAG = magnitude_table()


def gradient_magnitude(grad2ch):
    g = np.asarray(grad2ch, np.uint8).astype(np.int64) - 127
    return np.minimum(_MAG[g[..., 0] ** 2 + g[..., 1] ** 2], 255).astype(np.uint8)


def glbp_layer(gray, ksize, blur, lbp_type):
    """GradientFilter(ksize, blur) -> GradientMagnitudeFilter -> LbpFilter(lbp_type)"""
    from oracle import pyoracle
    return pyoracle.lbp(gradient_magnitude(pyoracle.gradient_filter(gray, ksize, blur)), lbp_type)


# ---- MT19937 (init_genrand / genrand_int32) and the model's draw
class MT19937:
    def __init__(self, seed=5489):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xffffffff
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xffffffff
        self.i = 624

    def next(self):
        if self.i >= 624:
            mt = self.mt
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7fffffff)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
            self.i = 0
        y = self.mt[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        y ^= y >> 18
        return y & 0xffffffff

    def below(self, n):
        """distribution(generator, n) of the model: one 32-bit draw, (draw * n) >> 32, in [0, n)"""
        if n <= 0:
            raise ValueError("n must be positive")
        return (self.next() * n) >> 32


# ---- PositionDependentMeasurementModel::adapt's sample selection (PositionDependentMeasurementModel.cpp:94-231)
class Selection:
    """state: usable, frameCount; has_window(x, y, w, h) and probability(x, y, w, h) are the caller's view of the feature extractor and
    the classifier.  adapt() returns None where the model returns false, else (positives, negatives, test negatives) as (x, y, size)"""

    def __init__(self, seed=5489, start_frame_count=3, stop_frame_count=0, target_threshold=0.7, confidence_threshold=0.95,
                 positive_offset_factor=0.05, negative_offset_factor=0.5, negatives_around_target=0, additional_negatives=10, test_negatives=10,
                 aspect_ratio=1.0):
        self.rng = MT19937(seed)
        self.usable = False
        self.frame_count = 0
        self.start_frame_count, self.stop_frame_count = start_frame_count, stop_frame_count
        self.target_threshold, self.confidence_threshold = float(np.float32(target_threshold)), float(np.float32(confidence_threshold))
        self.pof, self.nof = np.float32(positive_offset_factor), np.float32(negative_offset_factor)
        self.around, self.additional, self.test = negatives_around_target, additional_negatives, test_negatives
        self.aspect = aspect_ratio

    def height(self, size):
        return cv_round(self.aspect * size)

    def random_sample(self, cols, rows):
        lo, hi = int(0.1 * min(cols, rows)), int(0.9 * min(cols, rows))
        size = self.rng.below(hi - lo) + lo
        half = c_div2(size)
        x = self.rng.below(cols - size) + half
        y = self.rng.below(rows - size) + half
        return (x, y, size)

    def adapt(self, cols, rows, particles, target, has_window, probability):
        """particles: (x, y, size, weight) in the tracker's order; target (x, y, size)"""
        if not self.usable:
            self.frame_count += 1
            if self.frame_count < self.start_frame_count:
                return None
        else:
            self.frame_count = 0
        tx, ty, ts = target
        if not has_window(tx, ty, ts, self.height(ts)):
            return None
        if self.usable and probability(tx, ty, ts, self.height(ts)) < self.target_threshold:
            return None
        pos = [target]
        if self.pof != 0:
            off = max(1, int(self.pof * np.float32(ts)))
            pos += [(tx - off, ty, ts), (tx + off, ty, ts), (tx, ty - off, ts), (tx, ty + off, ts)]
        bound = int(self.nof * np.float32(ts))   # the factors are floats: float * int in float
        xl, xh, yl, yh = tx - bound, tx + bound, ty - bound, ty + bound
        down = np.float32(1) - self.nof
        up = np.float32(1) / down
        sl, sh = int(down * np.float32(ts)), int(up * np.float32(ts))
        neg = []
        if self.around > 0:
            neg += [(xl, ty, ts), (xh, ty, ts), (tx, yl, ts), (tx, yh, ts), (tx, ty, sl), (tx, ty, sh)]
            if self.around > 1:
                neg += [(xl, yl, ts), (xl, yh, ts), (xh, yl, ts), (xh, yh, ts)]
                neg += [(xl, ty, sl), (xl, ty, sh), (xh, ty, sl), (xh, ty, sh)]
                neg += [(tx, yl, sl), (tx, yl, sh), (tx, yh, sl), (tx, yh, sh)]
                if self.around > 2:
                    neg += [(a, b, c) for a in (xl, xh) for b in (yl, yh) for c in (sl, sh)]

        def outside(s):
            return s[0] <= xl or s[0] >= xh or s[1] <= yl or s[1] >= yh or s[2] <= sl or s[2] >= sh

        if self.additional > 0:
            add = []   # (x, y, size, weight), ascending weight
            for p in particles:
                if not outside(p):
                    continue
                if len(add) < self.additional:
                    k = 0
                    while k < len(add) and add[k][3] < p[3]:   # lower_bound by weight
                        k += 1
                    add.insert(k, tuple(p))
                elif add[0][3] < p[3]:
                    add[0] = tuple(p)
                    i = 1
                    while i < len(add) and add[i - 1][3] > add[i][3]:
                        add[i - 1], add[i] = add[i], add[i - 1]
                        i += 1
            add = [a[:3] for a in add]
            while len(add) < self.additional:
                s = self.random_sample(cols, rows)
                if outside(s) and has_window(s[0], s[1], s[2], s[2]):
                    add.append(s)
            neg += add
        test = []
        while len(test) < self.test:
            s = self.random_sample(cols, rows)
            if outside(s) and has_window(s[0], s[1], s[2], s[2]):
                test.append(s)
        return pos, neg, test

    def training_vectors(self, pos, neg, has_window, probability, exploit_symmetry):
        """the number of vectors retrain receives: (positives, negatives), with the confidence predicates when the model is usable"""
        filtered = self.usable and self.confidence_threshold > 0
        counts = []
        for group, keep in ((pos, lambda p: p < self.confidence_threshold), (neg, lambda p: p > 1 - self.confidence_threshold)):
            n = 0
            for (x, y, s) in group:
                if has_window(x, y, s, self.height(s)) and (not filtered or keep(probability(x, y, s, self.height(s)))):
                    n += 2 if exploit_symmetry else 1
            counts.append(n)
        return tuple(counts)
