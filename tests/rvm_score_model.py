"""numpy restatement of the cascaded reduced-vector machine (RvmClassifier.cpp:75-126 through its cached evaluation path, with RbfKernel,
HistogramIntersectionKernel, LinearKernel and PolynomialKernel on f32 vectors), the error bound csrc/rvm.hip is held to, a calibration
that makes a window leave at EVERY level, and the ONE seeded case builder of tests/test_rvm_score_model.py (no GPU) and
tests/test_gpu_rvm_score.py (the kernels).  It shares no code with oracle/orc_classify.cpp or the library.

The cascade.  K_k = K(x, rsv_k); d_0 = -bias + c_00 K_0, d_k = d_{k-1} + c_kk K_k in fp64 (bias and c read as float32, widened); a window
leaves at the first level k with !(d_k >= thr_k && k + 1 < num_used), and (level, distance) = (k, d_k).  A NaN distance therefore leaves
at level 0.  The kernel values are the reference's f32 paths, operation by operation:
  RBF   sum = sum + (x_i - s_i)^2 in fp32, element order;  K = exp(-gamma * double(sum))
  HIK   sum = sum + (s_i < x_i ? s_i : x_i) in fp32, element order (std::min(x, s): x when x is NaN);  K = double(sum)
  linear / polynomial   dot = dot + double(x_i) * double(s_i) in fp64, element order;  K = dot or powi(p0 * dot + p1, degree), powi
        the square-and-multiply loop of PolynomialKernel.hpp:73-81
No operation of HIK, linear and polynomial is a libm call: every one is a correctly rounded IEEE operation in a fixed order, and the
library is built without contraction, so for these kernels the device must give this model's BITS (bound 0).

The RBF bound.  exp is the only operation that may differ.  Its argument is the same double on both sides (identical fp32 sum, one
rounded product).  Write u = 2^-53.  Both exps lie within 1 ulp of the true value, i.e. within a relative 2u of it, so
|K_dev - K_np| <= 4u K.  The term t_j = fl(c_jj K_j) is rounded once on each side: |t_dev - t_np| <= |c_jj| (4u K_j) + 2u |c_jj| K_j
= 6u |c_jj| K_j.  Each addition d_k = fl(d_{k-1} + t_k) (k = 0: fl(-bias + t_0)) rounds once on each side, and two roundings of values
that differ by e differ by at most e + 2u max|d_k|, with |d_k| <= A_k := |bias| + sum_{j<=k} |c_jj| K_j.  Summing over the k + 1
additions and the k + 1 terms, to first order in u,
        |d_k(dev) - d_k(np)| <= (6 + 2 (k + 1)) u A_k = (k + 4) 2^-52 A_k.
Every second-order product is below (k + 4)^2 2^-104 A_k, less than one further unit of 2^-52 A_k for any k < 2^50, so
        bound_k = (k + 5) 2^-52 A_k
(a first estimate was (2^-51 + (k + 1) 2^-53) sum |c_jj| K_j; the derivation gives twice the per-addition unit, because the two sides round
independently, 6u instead of 4u for the term, and the bias belongs to the magnitude the additions round at).

A row is SURE when |d_k - thr_k| > bound_k at every level k it visits, the exit level and the cascade's last level included (there
the comparison decides "positive").  On sure rows the device must give the model's level.  margin is the smallest |d_k - thr_k| over the
visited levels except level num_used - 1, where leaving does not depend on the threshold.

The fp64 check of the specification (spec_gap): with S the exact squared distance, the fp32 chain computes every term as
fl(fl(x - s)^2) (relative error (1 + e)^3) and adds dim terms in sequence (dim - 1 roundings), so |S32 - S| <= g S with
g = gamma_(dim+2) = (dim + 2) 2^-24 / (1 - (dim + 2) 2^-24); the fp64 sum S64 of the same terms is within (dim + 2) 2^-53 S of S.
exp maps an absolute error a of the argument into a relative error expm1(a) of the value, so |K32_j - K64_j| <= K64_j expm1(gamma (g +
(dim + 2) 2^-53) S64_j (1 + 2^-50)) + the 1-ulp errors of the two exps, and
        |d_k(model) - d_k(fp64)| <= sum_{j<=k} |c_jj| K64_j expm1(...)_j + bound_k."""
import functools
import types
import zlib

import numpy as np

LINEAR, POLY, RBF, HIK = 0, 1, 2, 3
KERNELS = {"rbf": RBF, "hik": HIK, "linear": LINEAR, "poly": POLY}
U52 = 2.0 ** -52
F32, F64 = np.float32, np.float64

# ---- restated from csrc/rvm.hip --------------------------------------------------------------------------------------------------------
PASS_CUTS = (2, 6, 16)   # pass_bounds: k_rvm_pass runs the levels [0, 2), [2, 6), [6, 16)
DEEP_FROM = 16           # RVM_DEEP_FROM: k_rvm_deep takes the levels from here on, 64 per block: [16, 80), [80, 144), [144, ...)
MAX_PATCH = 32           # RVM_MAX_DIM: the deep kernel's LDS slab holds MAX_PATCH^2 floats


def pass_rows_to_wrap(num_cus):
    return num_cus * 2048   # k_rvm_pass: num_cus * 8 workgroups of 256 windows; more rows than this wrap the grid-stride loop


def deep_rows_to_wrap(num_cus):
    return num_cus * 32     # k_rvm_deep: num_cus * 8 workgroups of 4 windows


def u8_load_path(dim):
    """which loop of rvm_kernel_value<true> reads a u8 patch of dim bytes for RBF: 16-byte chunks, dwords, or bytes"""
    return "chunk16" if dim % 16 == 0 else "dword" if dim % 4 == 0 else "scalar"


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def num_used(m):
    F = len(m["sv"])
    nu = int(m.get("num_used", 0))
    return F if nu <= 0 or nu > F else nu      # setNumFiltersToUse, RvmClassifier.cpp:119-126


def diag(m):
    c = np.asarray(m["coeff"], F32)
    k = np.arange(len(m["sv"]))
    return c[k * (k + 1) // 2 + k].astype(F64)


def _powi(base, exponent):   # PolynomialKernel.hpp:73-81
    tmp, ret = base.copy(), np.ones_like(base)
    t = int(exponent)
    while t > 0:
        if t % 2 == 1:
            ret = ret * tmp
        tmp = tmp * tmp
        t //= 2
    return ret


def kernel_values(m, feats, levels=None):
    """K [n, levels] float64: the reference's kernel value of every row against the first `levels` reduced set vectors"""
    sv = np.ascontiguousarray(m["sv"], F32)
    L = len(sv) if levels is None else levels
    sv = sv[:L]
    x = np.ascontiguousarray(feats, F32).reshape(-1, sv.shape[1])
    dim = sv.shape[1]
    kernel = int(m["kernel"])
    out = np.empty((len(x), L), F64)
    step = max(1, (1 << 22) // max(L, 1))
    with np.errstate(all="ignore"):
        for r0 in range(0, len(x), step):
            xc = x[r0:r0 + step]
            if kernel in (RBF, HIK):
                acc = np.zeros((len(xc), L), F32)
                for i in range(dim):
                    xi, si = xc[:, i, None], sv[None, :, i]
                    if kernel == RBF:
                        diff = xi - si
                        acc = acc + diff * diff
                    else:
                        acc = acc + np.where(si < xi, si, xi)
                assert acc.dtype == F32
                out[r0:r0 + step] = np.exp(-F64(m["p0"]) * acc.astype(F64)) if kernel == RBF else acc.astype(F64)
            else:
                dot = np.zeros((len(xc), L), F64)
                x64, s64 = xc.astype(F64), sv.astype(F64)
                for i in range(dim):
                    dot = dot + x64[:, i, None] * s64[None, :, i]
                out[r0:r0 + step] = dot if kernel == LINEAR else _powi(F64(m["p0"]) * dot + F64(m["p1"]), int(m["p2"]))
    return out


def distances(m, K):
    """D [n, levels]: the running distance after every level, whether or not the window is still in the cascade"""
    c = diag(m)
    D = np.empty_like(K)
    with np.errstate(all="ignore"):
        d = -F64(F32(m["bias"])) + c[0] * K[:, 0]
        D[:, 0] = d
        for k in range(1, K.shape[1]):
            d = d + c[k] * K[:, k]
            D[:, k] = d
    return D


def bounds(m, K):
    """B [n, levels]: the derived bound on |d_k(device) - d_k(model)|; zero for the kernels that take no libm function"""
    if int(m["kernel"]) != RBF:
        return np.zeros_like(K)
    A = abs(F64(F32(m["bias"]))) + np.cumsum(np.abs(diag(m))[None, :K.shape[1]] * K, axis=1)
    return (np.arange(K.shape[1]) + 5)[None, :] * U52 * A


def run(m, D, B):
    """the exits of the cascade of m (thresholds, num_used) on the distances D: per row level, dist, bound (at the exit level), margin, sure,
    positive"""
    nu = num_used(m)
    thr = np.asarray(m["thresholds"], F32).astype(F64)
    n = len(D)
    level = np.full(n, -1, np.int32)
    alive = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for k in range(nu):
            leaves = alive & ~((D[:, k] >= thr[k]) & (k + 1 < nu))
            level[leaves] = k
            alive &= ~leaves
        assert not alive.any() and level.min() >= 0
        rows = np.arange(n)
        dist = D[rows, level]
        visited = np.arange(nu)[None, :] <= level[:, None]
        gap = np.abs(D[:, :nu] - thr[None, :nu])
        sure = np.all(~visited | (gap > B[:, :nu]), axis=1)
        inner = visited.copy()
        inner[:, nu - 1] = False
        margin = np.where(inner, gap, np.inf).min(axis=1)
        positive = (level == nu - 1) & (dist >= thr[nu - 1])
    return types.SimpleNamespace(level=level, dist=dist, bound=B[rows, level], margin=margin, sure=sure, positive=positive,
                                 reached=np.array([(level >= k).sum() for k in range(nu)]))


def evaluate(m, feats):
    """the whole model on f32 rows"""
    K = kernel_values(m, feats, num_used(m))
    return run(m, distances(m, K), bounds(m, K))


def calibrate(m, feats, pass_rate, D=None):
    """float32 thresholds for the levels 0 .. num_used - 1 from the model's own distances: level by level, the midpoint of the gap at the
    quantile 1 - pass_rate of the rows still alive (at least one row leaves, at least one stays; where distances tie at the quantile,
    the nearest gap), the last level included; the levels that are not used keep -1e30"""
    nu = num_used(m)
    if D is None:
        D = distances(m, kernel_values(m, feats, nu))
    thr = np.full(len(m["sv"]), -1e30, F32)
    alive = np.ones(len(D), bool)
    for k in range(nu):
        v = np.sort(D[alive, k])
        assert len(v) >= 2 and np.all(np.isfinite(v)), (k, len(v))
        j = min(max(int(round((1.0 - pass_rate) * len(v))), 1), len(v) - 1)
        gaps = np.nonzero(v[1:] > v[:-1])[0] + 1       # tied distances (HIK rows that lie above a whole reduced set vector) have no gap:
        j = int(gaps[np.argmin(np.abs(gaps - j))])     # the nearest one
        thr[k] = F32(0.5 * (v[j - 1] + v[j]))
        alive &= D[:, k] >= F64(thr[k])
    return thr


def probability(m, d):
    return 1.0 / (1.0 + np.exp(F64(m["logistic_a"]) + F64(m["logistic_b"]) * d))   # ProbabilisticRvmClassifier.cpp:62


def spec_gap(m, feats):
    """(|D - D64|, its bound) [n, levels] for an RBF model: D64 is the cascade with the squared distance summed in fp64"""
    assert int(m["kernel"]) == RBF
    sv = np.ascontiguousarray(m["sv"], F32).astype(F64)
    x = np.ascontiguousarray(feats, F32).astype(F64)
    dim = sv.shape[1]
    S = np.zeros((len(x), len(sv)), F64)
    for i in range(dim):
        diff = x[:, i, None] - sv[None, :, i]
        S = S + diff * diff
    gamma = F64(m["p0"])
    K64 = np.exp(-gamma * S)
    K = kernel_values(m, feats)
    g = (dim + 2) * 2.0 ** -24 / (1 - (dim + 2) * 2.0 ** -24)
    rel = np.expm1(gamma * (g + (dim + 2) * 2.0 ** -53) * S * (1 + 2.0 ** -50))
    c = np.abs(diag(m))
    allowed = np.cumsum(c[None, :] * K64 * rel, axis=1) + bounds(m, K)
    return np.abs(distances(m, K) - distances(m, K64)), allowed


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
LEVELS_NUM_USED = (1, 2, 3, 6, 7, 16, 17, 79, 80, 81, 144, 145)
LEVELS_DIM, LEVELS_FILTERS, LEVELS_ROWS, LEVELS_PASS = 36, 145, 6000, 0.975
WRAP_DIM, WRAP_FILTERS, WRAP_PASS = 4, 20, 0.85
U8_PATCHES = ((2, 2), (4, 4), (8, 4), (12, 12), (6, 6), (5, 5), (7, 5), (32, 32))
U8_FILTERS, U8_PASS = 90, 0.955
U8_CONV = {"rbf": (1.0 / 255.0, 0.0), "hik": (0.5, -3.0), "linear": (1.0, 0.0), "poly": (1.0, 0.0)}
BENCH_PATCH, BENCH_FILTERS, BENCH_PASS = (20, 20), 100, 0.96
IMAGE_W, IMAGE_H = 96, 64
NONFINITE_NUM_USED, NONFINITE_ROWS = 20, 64
LIMIT_W, LIMIT_H, LIMIT_FILTERS, LIMIT_ROWS, LIMIT_PASS = 33, 32, 17, 300, 0.8
FEATURE_GRAY, FEATURE_HQ64 = 0, 1


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def image():
    """96x64 gray: fine noise on a diagonal ramp"""
    rng = _rng("image")
    yy, xx = np.mgrid[0:IMAGE_H, 0:IMAGE_W]
    ramp = 150.0 * (0.6 * xx / (IMAGE_W - 1) + 0.4 * yy / (IMAGE_H - 1))
    return np.clip(np.rint(ramp + rng.integers(0, 106, ramp.shape)), 0, 255).astype(np.uint8)


def window_origins(pw, ph):
    """(lx, ly) of every window of the one-layer pyramid at scale 1 and step 1, in scan order (rows of windows, left to right).  The
    reference's sliding window stops at x + pw < width, y + ph < height (strict): the last column and row of positions are not visited"""
    ys, xs = np.mgrid[0:IMAGE_H - ph, 0:IMAGE_W - pw]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def window_patches(img, pw, ph):
    """[windows, ph * pw] u8, in the order of window_origins"""
    v = np.lib.stride_tricks.sliding_window_view(img, (ph, pw))[:IMAGE_H - ph, :IMAGE_W - pw]
    return np.ascontiguousarray(v.reshape(-1, ph * pw))


def convert(patches, scale, shift):
    """ConversionFilter(CV_32F, scale, shift) as cv::Mat::convertTo does it in float: one product, one sum"""
    return patches.astype(F32) * F32(scale) + F32(shift)


def make_model(name, kernel, feats, fw, fh, filters):
    """reduced set vectors, coefficients, bias and gamma the way synth.make_rvm builds them; no thresholds yet (calibrate)"""
    rng = _rng(name + "/model")
    feats = np.ascontiguousarray(feats, F32)
    dim = fw * fh
    idx = rng.choice(len(feats), filters, replace=len(feats) < filters)
    sv = (0.85 * feats[idx] + 0.15 * feats.mean(0, keepdims=True)).astype(F32)
    coeff = np.zeros(filters * (filters + 1) // 2, F32)
    for k in range(filters):
        coeff[k * (k + 1) // 2: k * (k + 1) // 2 + k + 1] = rng.normal(0, 1, k + 1).astype(F32)
    sub = feats[:200].astype(F64)
    p0 = p1 = p2 = 0.0
    if kernel == RBF:
        d2 = ((sub[:, None, :] - sv[None, :8].astype(F64)) ** 2).sum(-1)
        p0 = float(F32(1.0 / np.median(d2)))
    elif kernel == POLY:   # rows in 0 .. 255: the base stays within 0.5 .. 1.5; degree 3 = 0b11 takes both branches of square-and-multiply twice
        p0, p1, p2 = 1.0 / (dim * 255.0 * 255.0), 0.5, 3.0
    elif kernel == HIK:
        coeff /= F32(np.abs(np.minimum(sub[:, None, :], sv[None, :8].astype(F64)).sum(-1)).mean())
    else:
        coeff /= F32(np.abs(sub @ sv[:8].astype(F64).T).mean())
    return dict(kernel=kernel, p0=p0, p1=p1, p2=p2, filter_w=fw, filter_h=fh, sv=sv, coeff=coeff, bias=F32(0.1), num_used=0,
                thresholds=np.full(filters, -1e30, F32), logistic_a=0.2, logistic_b=-1.5)


def _case(name, base, rows, pass_rate, num_useds, **kw):
    return types.SimpleNamespace(name=name, base=base, rows=rows, pass_rate=pass_rate, num_useds=tuple(num_useds), kernel=int(base["kernel"]),
                                 **kw)


def _f32_rows(name, kname, n, dim):
    rng = _rng(name + "/rows")
    if kname == "poly":
        return rng.integers(0, 256, (n, dim)).astype(F32)
    return rng.random((n, dim), dtype=F32)


def _levels(name, kname):
    rows = _f32_rows(name, kname, LEVELS_ROWS, LEVELS_DIM)
    return _case(name, make_model(name, KERNELS[kname], rows, 6, 6, LEVELS_FILTERS), rows, LEVELS_PASS, LEVELS_NUM_USED)


def _wrap(name, kname, num_cus):
    rows = _f32_rows(name, kname, pass_rows_to_wrap(num_cus) + 77, WRAP_DIM)
    return _case(name, make_model(name, KERNELS[kname], rows, 2, 2, WRAP_FILTERS), rows, WRAP_PASS, (WRAP_FILTERS,), num_cus=num_cus)


def _u8(name, pw, ph, kname):
    patches = window_patches(image(), pw, ph)
    scale, shift = U8_CONV[kname]
    rows = convert(patches, scale, shift)
    return _case(name, make_model(name, KERNELS[kname], rows, pw, ph, U8_FILTERS), rows, U8_PASS, (U8_FILTERS,), patches=patches, pw=pw, ph=ph,
                 space=FEATURE_GRAY, conv=(scale, shift), origins=window_origins(pw, ph))


def _bench_shape(name):
    from oracle import pyoracle   # the hq64 feature space is the oracle's HistEq64Filter, as in the existing detector tests
    pw, ph = BENCH_PATCH
    gray = window_patches(image(), pw, ph)
    patches = np.stack([pyoracle.histeq64(np.ascontiguousarray(p.reshape(ph, pw))).reshape(-1) for p in gray])
    scale, shift = 1.0 / 255.0, 0.0
    rows = convert(patches, scale, shift)
    return _case(name, make_model(name, RBF, rows, pw, ph, BENCH_FILTERS), rows, BENCH_PASS, (BENCH_FILTERS,), patches=patches, gray=gray, pw=pw,
                 ph=ph, space=FEATURE_HQ64, conv=(scale, shift), origins=window_origins(pw, ph))


NONFINITE_VALUES = (np.nan, np.inf, -np.inf)


def _nonfinite(name, kname):
    src = case("levels-" + kname)
    rows = src.rows[:NONFINITE_ROWS].copy()
    positions = (0, LEVELS_DIM // 2, LEVELS_DIM - 1)
    for r in range(len(rows)):
        rows[r, positions[(r // 3) % 3]] = NONFINITE_VALUES[r % 3]
    c = _case(name, src.base, rows, LEVELS_PASS, (NONFINITE_NUM_USED,))
    c.thresholds_from = "levels-" + kname
    return c


def _limit(name):
    rng = _rng(name + "/rows")
    rows = rng.random((LIMIT_ROWS, LIMIT_W * LIMIT_H), dtype=F32)
    return _case(name, make_model(name, RBF, rows, LIMIT_W, LIMIT_H, LIMIT_FILTERS), rows, LIMIT_PASS, (16, 17))


_BUILDERS = {}
for _kn in KERNELS:
    _BUILDERS["levels-" + _kn] = lambda name, cus, kn=_kn: _levels(name, kn)
    _BUILDERS["wrap-" + _kn] = lambda name, cus, kn=_kn: _wrap(name, kn, cus)
    _BUILDERS["nonfinite-" + _kn] = lambda name, cus, kn=_kn: _nonfinite(name, kn)
    for _pw, _ph in U8_PATCHES:
        _BUILDERS["u8-%dx%d-%s" % (_pw, _ph, _kn)] = lambda name, cus, pw=_pw, ph=_ph, kn=_kn: _u8(name, pw, ph, kn)
_BUILDERS["bench-shape"] = lambda name, cus: _bench_shape(name)
_BUILDERS["limit-rbf"] = lambda name, cus: _limit(name)
NAMES = list(_BUILDERS)


def names(prefix):
    return [n for n in NAMES if n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def case(name, num_cus=256):
    """the case of that name, built once per process; treat it as read-only.  num_cus matters to the wrap cases only"""
    c = _BUILDERS[name](name, num_cus)
    for a in (c.rows, c.base["sv"], c.base["coeff"], c.base["thresholds"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _tables(name, num_cus=256):
    """(K, D, B) of the case's rows over all its filters: computed once, whatever num_used a test takes"""
    c = case(name, num_cus)
    K = kernel_values(c.base, c.rows, max(c.num_useds))
    D, B = distances(c.base, K), bounds(c.base, K)
    for a in (K, D, B):
        a.setflags(write=False)
    return K, D, B


@functools.lru_cache(maxsize=None)
def model(name, nu=None, num_cus=256):
    """the case's model with num_used = nu (default: the case's largest) and the thresholds calibrated for it"""
    c = case(name, num_cus)
    nu = max(c.num_useds) if nu is None else nu
    assert nu in c.num_useds
    m = dict(c.base, num_used=nu)
    if getattr(c, "thresholds_from", None):   # the non-finite rows run under the thresholds of the finite rows they were made from
        src = case(c.thresholds_from)
        thr = calibrate(dict(src.base, num_used=nu), src.rows, src.pass_rate, D=_tables(c.thresholds_from)[1])
    else:
        thr = calibrate(m, c.rows, c.pass_rate, D=_tables(name, num_cus)[1])
    thr.setflags(write=False)
    m["thresholds"] = thr
    return m


@functools.lru_cache(maxsize=None)
def reference(name, nu=None, num_cus=256):
    """run() of model(name, nu) on the case's rows, computed once"""
    _, D, B = _tables(name, num_cus)
    return run(model(name, nu, num_cus), D, B)


def with_thresholds(name, value, nu=None, num_cus=256):
    """(model, reference) of the case with every threshold set to value"""
    m = dict(model(name, nu, num_cus))
    m["thresholds"] = np.full(len(m["sv"]), value, F32)
    _, D, B = _tables(name, num_cus)
    return m, run(m, D, B)
