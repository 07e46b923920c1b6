"""numpy model of DESIGN.md 4.14: the flow pyramid (buildOpticalFlowPyramid with derivatives, replicated borders), pyramidal
Lucas-Kanade for one point (calcOpticalFlowPyrLK, default criteria) and OpticalFlowTransitionModel's host arithmetic (template grid,
median flow, the motion of a sample).  Integers where the specification has integers (Python ints / int64: nothing can wrap),
np.float32 scalars, one operation at a time, elsewhere.  Also the frames, point sets and cases the flow tests share."""
import functools

import numpy as np

F = np.float32
MAX_LEVELS = 8
EXIT_NONE, EXIT_SKIP_RANGE, EXIT_SKIP_EIGEN, EXIT_EPS, EXIT_OSCILLATION, EXIT_COUNT, EXIT_LEFT_RANGE = range(7)
EXIT_NAMES = ("none", "skip-range", "skip-eigen", "eps", "oscillation", "count", "left-range")
FLT_EPSILON = F(np.finfo(np.float32).eps)
FLT_SCALE = F(1.0) / F(1 << 20)
KERNEL = np.array([1, 4, 6, 4, 1], np.int64)


# ---------------------------------------------------------------- pyramid

def bgr2gray(img):
    img = np.asarray(img)
    if img.ndim == 2:
        return img.astype(np.uint8)
    b, g, r = (img[..., c].astype(np.int64) for c in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def reflect101(p, n):
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    for _ in range(4):
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return np.clip(p, 0, n - 1)


def pyr_down(img):
    h, w = img.shape
    dw, dh = (w + 1) // 2, (h + 1) // 2
    xs = reflect101(2 * np.arange(dw)[:, None] - 2 + np.arange(5)[None, :], w)   # (dw, 5)
    ys = reflect101(2 * np.arange(dh)[:, None] - 2 + np.arange(5)[None, :], h)
    src = img.astype(np.int64)
    vertical = (src[ys] * KERNEL[None, :, None]).sum(axis=1)                      # (dh, w)
    both = (vertical[:, xs] * KERNEL[None, None, :]).sum(axis=2)                  # (dh, dw)
    return ((both + 128) >> 8).astype(np.uint8)


def scharr(img):
    h, w = img.shape
    r = img.astype(np.int64)
    up, down = r[reflect101(np.arange(h) - 1, h)], r[reflect101(np.arange(h) + 1, h)]
    t0 = 3 * (up + down) + 10 * r
    t1 = down - up
    xl, xr = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    dx = t0[:, xr] - t0[:, xl]
    dy = 3 * (t1[:, xl] + t1[:, xr]) + 10 * t1
    assert np.abs(dx).max() <= 4080 and np.abs(dy).max() <= 4080
    return np.stack([dx, dy], axis=2).astype(np.int16)


def pad(a, win_w, win_h):
    return np.pad(a, ((win_h, win_h), (win_w, win_w)) + ((0, 0),) * (a.ndim - 2), mode="edge")


def build_pyramid(image, win_w, win_h, max_level):
    """levels from 0 up: dict(w, h, img uint8 (h + 2 win_h, w + 2 win_w), der int16 (.., .., 2)), borders included"""
    level = bgr2gray(image)
    out = []
    for l in range(max_level + 1):
        h, w = level.shape
        if l > 0 and (w <= win_w or h <= win_h):
            break
        out.append(dict(w=w, h=h, img=pad(level, win_w, win_h), der=pad(scharr(level), win_w, win_h)))
        level = pyr_down(level)
    return out


# ---------------------------------------------------------------- tracking

def _weights(a, b):
    one, s = F(1), F(16384)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _inside(fx, fy, win_w, win_h, w, h):
    return bool(fx >= F(-win_w) and fx < F(w) and fy >= F(-win_h) and fy < F(h))


def _taps(a, ix, iy, win_w, win_h, wts, shift):
    """DESCALE(sum of the four taps * weights, shift) over the window whose corner is (ix, iy) in the stored (bordered) array"""
    p = a[iy:iy + win_h + 1, ix:ix + win_w + 1].astype(np.int64)
    v = p[:-1, :-1] * wts[0] + p[:-1, 1:] * wts[1] + p[1:, :-1] * wts[2] + p[1:, 1:] * wts[3]
    return (v + (1 << (shift - 1))) >> shift


def track_point(from_pyr, to_pyr, pt, win_w, win_h, max_count, eps2, min_eig):
    nlev = len(from_pyr)
    trace = np.zeros((MAX_LEVELS, 2), np.uint8)
    half_x, half_y = F(win_w - 1) * F(0.5), F(win_h - 1) * F(0.5)
    den = F(2 * win_w * win_h)
    ptx, pty = F(pt[0]), F(pt[1])
    res_x = res_y = F(0)
    status = 1
    for level in range(nlev - 1, -1, -1):
        L, T = from_pyr[level], to_pyr[level]
        scale = F(1.0 / (1 << level))
        prev_x, prev_y = ptx * scale, pty * scale
        if level == nlev - 1:
            res_x, res_y = prev_x, prev_y
        else:
            res_x, res_y = F(2) * res_x, F(2) * res_y
        steps, reason = 0, EXIT_COUNT
        prev_x, prev_y = prev_x - half_x, prev_y - half_y
        fx, fy = np.floor(prev_x), np.floor(prev_y)
        if not _inside(fx, fy, win_w, win_h, L["w"], L["h"]):
            reason = EXIT_SKIP_RANGE
            if level == 0:
                status = 0
        else:
            ix, iy = int(fx) + win_w, int(fy) + win_h
            wts = _weights(prev_x - fx, prev_y - fy)
            I = _taps(L["img"], ix, iy, win_w, win_h, wts, 9)
            Ix = _taps(L["der"][..., 0], ix, iy, win_w, win_h, wts, 14)
            Iy = _taps(L["der"][..., 1], ix, iy, win_w, win_h, wts, 14)
            A11 = F(int((Ix * Ix).sum())) * FLT_SCALE
            A12 = F(int((Ix * Iy).sum())) * FLT_SCALE
            A22 = F(int((Iy * Iy).sum())) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            d = A11 - A22
            min_eig_value = ((A22 + A11) - np.sqrt(d * d + (F(4) * A12) * A12)) / den
            if min_eig_value < min_eig or D < FLT_EPSILON:
                reason = EXIT_SKIP_EIGEN
                if level == 0:
                    status = 0
            else:
                D = F(1) / D
                nx, ny = res_x - half_x, res_y - half_y
                pdx = pdy = F(0)
                for j in range(max_count):
                    fnx, fny = np.floor(nx), np.floor(ny)
                    if not _inside(fnx, fny, win_w, win_h, L["w"], L["h"]):
                        reason = EXIT_LEFT_RANGE
                        if level == 0:
                            status = 0
                        break
                    jx, jy = int(fnx) + win_w, int(fny) + win_h
                    diff = _taps(T["img"], jx, jy, win_w, win_h, _weights(nx - fnx, ny - fny), 9) - I
                    b1 = F(int((diff * Ix).sum())) * FLT_SCALE
                    b2 = F(int((diff * Iy).sum())) * FLT_SCALE
                    dx = (A12 * b2 - A22 * b1) * D
                    dy = (A12 * b1 - A11 * b2) * D
                    nx, ny = nx + dx, ny + dy
                    res_x, res_y = nx + half_x, ny + half_y
                    steps += 1
                    if dx * dx + dy * dy <= eps2:
                        reason = EXIT_EPS
                        break
                    if j > 0 and abs(dx + pdx) < F(0.01) and abs(dy + pdy) < F(0.01):
                        res_x, res_y = res_x - dx * F(0.5), res_y - dy * F(0.5)
                        reason = EXIT_OSCILLATION
                        break
                    pdx, pdy = dx, dy
        trace[level] = (steps, reason)
    return res_x, res_y, status, trace


def track(from_pyr, to_pyr, points, win_w, win_h, max_count=30, epsilon=0.01, min_eig_threshold=1e-4):
    """(out float32 (n, 2), status uint8 (n,), trace uint8 (n, MAX_LEVELS, 2) {steps, exit reason})"""
    points = np.asarray(points, np.float32).reshape(-1, 2)
    max_count = min(max(int(max_count), 0), 100)
    epsilon = min(max(float(epsilon), 0.0), 10.0)
    eps2, thr = F(epsilon * epsilon), F(min_eig_threshold)
    out = np.zeros((len(points), 2), np.float32)
    status = np.zeros(len(points), np.uint8)
    trace = np.zeros((len(points), MAX_LEVELS, 2), np.uint8)
    with np.errstate(all="ignore"):
        for i, pt in enumerate(points):
            x, y, status[i], trace[i] = track_point(from_pyr, to_pyr, pt, win_w, win_h, max_count, eps2, thr)
            out[i] = (x, y)
    return out, status, trace


# ---------------------------------------------------------------- OpticalFlowTransitionModel's host arithmetic

def grid(grid_w, grid_h, circle=True):
    """OpticalFlowTransitionModel.cpp:63-75"""
    gy = F(1) / F(grid_h + 2)
    gx = F(1) / F(grid_w + 2)
    r = F(0.5) - F(0.5) * (gx + gy)
    px = F(-0.5 + 0.5 * float(gx) + float(gx))   # a double expression stored as float
    py = F(-0.5 + 0.5 * float(gy) + float(gy))
    out = []
    for _ in range(grid_h):
        for _ in range(grid_w):
            if not circle or px * px + py * py < r * r:
                out.append((px, py))
            px = px + gx
        px = F(-0.5) + gx / F(2) + gx
        py = py + gy
    return np.array(out, np.float32).reshape(-1, 2)


def target_points(template, x, y, width, height):
    """.cpp:107-108: int * float + int, in float"""
    template = np.asarray(template, np.float32)
    return np.stack([F(width) * template[:, 0] + F(x), F(height) * template[:, 1] + F(y)], axis=1).astype(np.float32)


def median(points, fwd, bwd, fstatus, bstatus):
    """.cpp:114-170 with ties by index; dict(ok, n_valid, n_correct, median_x, median_y, median_ratio, order)"""
    points, fwd, bwd = (np.asarray(a, np.float32).reshape(-1, 2) for a in (points, fwd, bwd))
    n = len(points)
    out = dict(ok=False, n_valid=0, n_correct=0, median_x=F(0), median_y=F(0), median_ratio=F(1), order=np.zeros(0, np.int32))
    with np.errstate(all="ignore"):
        pairs = []
        for i in range(n):
            if fstatus[i] and bstatus[i]:
                dx, dy = bwd[i, 0] - points[i, 0], bwd[i, 1] - points[i, 1]
                d = dx * dx + dy * dy
                if d == d:
                    pairs.append((d, i))
        pairs.sort()
        out["n_valid"] = len(pairs)
        out["order"] = np.array([i for _, i in pairs], np.int32)
        if len(pairs) < n // 2:
            return out
        correct = 0
        while correct < len(pairs) and not pairs[correct][0] > F(0.5):
            correct += 1
        out["n_correct"] = correct
        if correct < n // 2 or correct < 2:
            return out
        idx = out["order"][:correct]
        out["median_x"] = np.sort(fwd[idx, 0] - points[idx, 0])[correct // 2]
        out["median_y"] = np.sort(fwd[idx, 1] - points[idx, 1])[correct // 2]
        a, b = np.triu_indices(correct, 1)
        before, after = points[idx[a]] - points[idx[b]], fwd[idx[a]] - fwd[idx[b]]
        ratios = (after[:, 0] * after[:, 0] + after[:, 1] * after[:, 1]) / (before[:, 0] * before[:, 0] + before[:, 1] * before[:, 1])
        out["median_ratio"] = np.sqrt(np.sort(ratios)[len(ratios) // 2])   # np.sort puts NaN last
        out["ok"] = True
    return out


def round_half_away(v):
    """std::round of a double"""
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def apply_motion(sample, motion, position_deviation, size_deviation, z):
    """.cpp:173-190 for one sample (x, y, size) with its three normal draws z = (zx, zy, zsize): (x, y, size, vx, vy, vsize)"""
    vx = float(motion["median_x"]) + position_deviation * z[0]
    vy = float(motion["median_y"]) + position_deviation * z[1]
    vs = float(motion["median_ratio"]) * pow(2.0, size_deviation * z[2])
    nvx, nvy, nvs = round_half_away(vx), round_half_away(vy), F(vs)
    size = round_half_away(float(F(sample[2]) * nvs))   # int * float: a float product
    return sample[0] + nvx, sample[1] + nvy, size, nvx, nvy, nvs


# ---------------------------------------------------------------- frames, points and cases of the tests

WIDTH, HEIGHT = 160, 128
FLAT = (96, 20, 40, 36)   # x, y, w, h of the patch painted flat


def textured(width=WIDTH, height=HEIGHT, seed=7, sigma=2.0):
    """seeded noise, blurred with a Gaussian (sigma 2, circular, so that a roll of the result is an exact shift), stretched to 0..255"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((height, width))
    radius = int(3 * sigma)
    k = np.exp(-0.5 * (np.arange(-radius, radius + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        a = sum(w * np.roll(a, t - radius, axis=axis) for t, w in enumerate(k))
    a = (a - a.min()) / (a.max() - a.min())
    return np.rint(a * 255).astype(np.uint8)


def zoomed(img, factor):
    """img magnified by `factor` about its centre (bilinear)"""
    h, w = img.shape
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    xs = np.clip((np.arange(w) - cx) / factor + cx, 0, w - 1)
    ys = np.clip((np.arange(h) - cy) / factor + cy, 0, h - 1)
    x0, y0 = np.minimum(np.floor(xs).astype(int), w - 2), np.minimum(np.floor(ys).astype(int), h - 2)
    fx, fy = (xs - x0)[None, :], (ys - y0)[:, None]
    a = img.astype(np.float64)
    top = a[y0][:, x0] * (1 - fx) + a[y0][:, x0 + 1] * fx
    bottom = a[y0 + 1][:, x0] * (1 - fx) + a[y0 + 1][:, x0 + 1] * fx
    return np.rint(top * (1 - fy) + bottom * fy).astype(np.uint8)


def _paint_flat(img):
    x, y, w, h = FLAT
    img = img.copy()
    img[y:y + h, x:x + w] = 128
    return img


@functools.lru_cache(maxsize=None)
def frame_pair(kind):
    """(previous, current) gray frames: 'roll' moves the content by (3, -2), 'zoom' magnifies it 1.08 x about the centre,
    'jump' moves it by (13, 9); each with a flat patch painted into both frames"""
    base = textured()
    if kind == "roll":
        nxt = np.roll(base, (-2, 3), axis=(0, 1))
    elif kind == "zoom":
        nxt = zoomed(base, 1.08)
    elif kind == "jump":
        nxt = np.roll(base, (9, 13), axis=(0, 1))
    else:
        raise ValueError(kind)
    return _paint_flat(base), _paint_flat(nxt)


def grid_points():
    """the 10 x 10 circle grid on a 64 x 64 target at the centre of the frame"""
    return target_points(grid(10, 10, True), WIDTH // 2, HEIGHT // 2, 64, 64)


def random_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, WIDTH - 1, n), rng.uniform(0, HEIGHT - 1, n)], axis=1).astype(np.float32)


# windows that hang into the border on each side and at the corners
EDGE_POINTS = np.array([[1.3, 60.7], [158.6, 64.2], [80.5, 0.8], [77.1, 126.9], [0.0, 0.0], [159.0, 127.0], [0.4, 127.0], [159.0, 0.6],
                        [-3.5, 40.25], [162.75, 90.5], [70.5, -2.5], [30.0, 130.25]], np.float32)
# no window inside the frame at level 0 (status 0); the last ones are far outside the int range as well
OUTSIDE_POINTS = np.array([[-40.5, 50.0], [230.0, 64.0], [80.0, -47.0], [80.0, 300.0], [1.0e6, 5.0], [3.0e9, -3.0e9], [-1.0e12, 64.0]], np.float32)
FLAT_POINTS = np.array([[FLAT[0] + 20.0, FLAT[1] + 18.0], [FLAT[0] + 17.5, FLAT[1] + 16.25], [FLAT[0] + 22.0, FLAT[1] + 19.5]], np.float32)


def _mixed():
    return np.concatenate([grid_points(), EDGE_POINTS, OUTSIDE_POINTS, FLAT_POINTS])


# name: (frame pair, win_w, win_h, max_level, max_count, backward, points)
CASES = {
    "roll-15x15-mixed": ("roll", 15, 15, 2, 30, False, _mixed()),
    "zoom-15x15-mixed": ("zoom", 15, 15, 2, 30, False, _mixed()),
    "roll-15x15-one": ("roll", 15, 15, 2, 30, False, random_points(1, 11)),
    "roll-3x3-n65": ("roll", 3, 3, 2, 30, False, np.concatenate([random_points(65 - len(EDGE_POINTS), 12), EDGE_POINTS])),
    "roll-5x7-n63": ("roll", 5, 7, 2, 30, False, np.concatenate([random_points(63 - len(EDGE_POINTS), 13), EDGE_POINTS])),
    "zoom-21x21-n64": ("zoom", 21, 21, 2, 30, False, np.concatenate([random_points(64 - len(EDGE_POINTS), 14), EDGE_POINTS])),
    "zoom-31x31-n65": ("zoom", 31, 31, 2, 30, False, np.concatenate([random_points(65 - len(EDGE_POINTS), 15), EDGE_POINTS])),
    "roll-15x15-level0-n257": ("roll", 15, 15, 0, 30, False, random_points(257, 16)),
    "zoom-15x15-level0-mixed": ("zoom", 15, 15, 0, 30, False, _mixed()),
    "zoom-15x15-count2-n64": ("zoom", 15, 15, 2, 2, False, random_points(64, 17)),
    "zoom-15x15-backward-n65": ("zoom", 15, 15, 2, 30, True, np.concatenate([random_points(65 - len(EDGE_POINTS), 18), EDGE_POINTS])),
    "jump-5x7-n64": ("jump", 5, 7, 2, 30, False, np.concatenate([random_points(64 - len(EDGE_POINTS), 19), EDGE_POINTS])),
}


@functools.lru_cache(maxsize=None)
def pyramids(kind, win_w, win_h, max_level):
    prev, cur = frame_pair(kind)
    return build_pyramid(prev, win_w, win_h, max_level), build_pyramid(cur, win_w, win_h, max_level)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the model's (out, status, trace) of a case; computed once per process, not to be modified"""
    kind, win_w, win_h, max_level, max_count, backward, points = CASES[name]
    prev, cur = pyramids(kind, win_w, win_h, max_level)
    result = track(cur, prev, points, win_w, win_h, max_count) if backward else track(prev, cur, points, win_w, win_h, max_count)
    for a in result:
        a.setflags(write=False)
    return result
