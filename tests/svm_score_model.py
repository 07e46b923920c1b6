"""numpy restatement of kernel SVM scoring (SvmClassifier.cpp:55-60 with LinearKernel, PolynomialKernel, RbfKernel and
HistogramIntersectionKernel) for u8 and f32 rows, the error bounds the kernels of csrc/svm.hip are held to, and the ONE seeded case
builder of tests/test_svm_score_model.py (no GPU) and tests/test_gpu_svm_score.py (the kernels).

distance(m, x) = -bias + sum_i c_i K(x, s_i).  Integer kernel arguments (u8 rows) are exact: every partial sum of the float64 matrix
product is an integer below 2^53.  The f32 arguments, the kernel values and the sum over the support vectors are taken in long double
(64-bit mantissa) wherever the case is small enough for numpy's unaccelerated long double product, so the model's own error is far below
the 2^-53 unit of the bounds; the two large f32 cases (both judged at 1e-5) use float64 for the product.  The bias is read as float32,
the coefficients as float32 widened, as the library does.

scale(m, x) = sum_i |c_i| K(|x|, |s_i|) + |bias| (polynomial: |p0|, |p1|) is what the derived bounds are relative to."""
import functools
import math
import types
import zlib

import numpy as np

LINEAR, POLY, RBF, HIK = 0, 1, 2, 3
U8, F32 = 0, 1
U53, U24 = 2.0 ** -53, 2.0 ** -24
LD = np.longdouble
MUTANTS = ("drop_last_byte", "pad_as_zero", "shift_coefficients", "skip_last_sv")
GAMMA_U8 = float(np.float32(0.04 / 65025.0))   # SvmClassifier.cpp:264 with r = 0.04
P0_U8_POLY, P1_POLY = 1.0 / 65025.0, 0.7
DCOUNTS = (0, 1, 33, 65, 70)                   # at n = 65: nothing, one, a workgroup and a row, n, n + 5
_LD_LIMIT = 3e7                                 # multiply-adds up to which the f32 products run in long double


def degree(m):
    return int(m.get("p2", 0)) if m["kernel"] == POLY else 0


def _np_dtype(m):
    return np.uint8 if m["dtype"] == U8 else np.float32


def _args(kernel, x, s, exact_ld):
    """the kernel's argument for every (row, support vector): dot product, sum of minima, or sum of squared differences.
    x [n, d], s [nsv, d], float64 holding u8 or f32 values; returns long double [n, nsv]"""
    if kernel == HIK:
        out = np.empty((len(x), len(s)), LD)
        for j in range(len(s)):
            # bytes: exact integers; f32 values: float64 sum, 2^-29 of the float kernel's unit
            out[:, j] = np.minimum(x, s[j]).sum(1, dtype=np.int64 if x.dtype == np.uint8 else np.float64)
        return out
    if exact_ld:
        xl, sl = x.astype(LD), s.astype(LD)
        dot = xl @ sl.T if x.shape[1] else np.zeros((len(x), len(s)), LD)
        if kernel != RBF:
            return dot
        return np.maximum(((xl * xl).sum(1)[:, None] + (sl * sl).sum(1)[None, :]) - 2 * dot, 0)
    dot = (x @ s.T).astype(LD)
    if kernel != RBF:
        return dot
    return np.maximum(((x * x).sum(1)[:, None].astype(LD) + (s * s).sum(1)[None, :].astype(LD)) - 2 * dot, 0)


def _kernel_values(m, arg, absolute):
    k = m["kernel"]
    p0, p1 = float(m.get("p0", 0)), float(m.get("p1", 0))
    if k == RBF:
        return np.exp(-LD(p0) * arg)
    if k == POLY:
        if absolute:
            p0, p1 = abs(p0), abs(p1)
        return (LD(p0) * arg + LD(p1)) ** degree(m)
    return arg


def _sum(m, x, bias, absolute=False, mutant=None):
    dt = _np_dtype(m)
    sv = np.ascontiguousarray(m["sv"], dt)
    nsv, dim = sv.shape
    x = np.ascontiguousarray(x, dt).reshape(-1, dim)
    c = np.asarray(m["coeff"], np.float32).astype(LD)
    k = m["kernel"]
    if mutant is not None:
        assert m["dtype"] == U8 and mutant in MUTANTS and not absolute
    if mutant == "shift_coefficients":      # coefficient i + 1 for support vector i; the last one reads the zero padding
        c = np.concatenate([c[1:], np.zeros(1, LD)])
    if mutant == "skip_last_sv":
        c = c.copy()
        c[-1] = 0
    as_bytes = m["dtype"] == U8 and k == HIK       # minima of bytes need no widening (and u8 values are their own magnitudes)
    s64 = sv if as_bytes else sv.astype(np.float64)
    if absolute:
        c = np.abs(c)
        s64 = s64 if as_bytes else np.abs(s64)
    exact_ld = m["dtype"] == F32 and float(len(x)) * nsv * dim <= _LD_LIMIT
    out = np.empty(len(x), np.float64)
    step = max(1, (1 << 23) // dim)
    for r0 in range(0, len(x), step):
        xc = x[r0:r0 + step] if as_bytes else x[r0:r0 + step].astype(np.float64)
        if absolute and not as_bytes:
            xc = np.abs(xc)
        arg = _args(k, xc, s64, exact_ld)
        if mutant == "drop_last_byte":      # the support vector with the largest |coefficient| loses its last element
            j = int(np.argmax(np.abs(np.asarray(m["coeff"], np.float32))))
            arg[:, j] = _args(k, xc[:, :-1], s64[j:j + 1, :-1], False)[:, 0]
        if mutant == "pad_as_zero" and k == RBF:
            # the i8 kernel works on x - 128 and s - 128 with ABSENT elements as 0 in both; a pad byte of the row staged as the value 0
            # is -128 there against the table's 0: 128^2 more per pad element of the 32-wide k-step
            arg = arg + 16384 * ((-dim) % 32)
        out[r0:r0 + step] = ((_kernel_values(m, arg, absolute) * c[None, :]).sum(1) + bias).astype(np.float64)   # rounded once
    return out


def distance(m, x, mutant=None):
    """-bias + sum_i c_i K(x, s_i) per row, float64"""
    return _sum(m, x, -LD(np.float32(m["bias"])), mutant=mutant)


def scale(m, x):
    """sum_i |c_i| K(|x|, |s_i|) + |bias| per row"""
    return _sum(m, x, abs(LD(np.float32(m["bias"]))), absolute=True)


def coeff_sum(m):
    return float(np.abs(np.asarray(m["coeff"], np.float32).astype(np.float64)).sum())


# ---- bounds on |d_kernel - distance(m, x)| per row -------------------------------------------------------------------------------------
def _outer_units(m):   # fp64 sum of nsv terms in any order, an fp64 exp within 2 ulp, powi's multiplies and one contracted multiply-add
    return len(m["sv"]) + 8 + 2 * degree(m)


def bound(m, x, path):
    """path: 'u8' (every u8 kernel body), 'generic' (k_svm_generic on f32 rows), 'mfma' (f32 RBF on the matrix pipe)"""
    dim = np.asarray(m["sv"]).shape[1]
    lanes = math.ceil(dim / 64)
    if path == "u8":
        assert m["dtype"] == U8
        return _outer_units(m) * U53 * scale(m, x)
    assert m["dtype"] == F32
    if path == "mfma":   # the project's contract for this path (xx + ss - 2 x.s cancels in fp32, fast __expf): not derived
        assert m["kernel"] == RBF
        return np.full(len(x), 1e-5 * coeff_sum(m))
    assert path == "generic"
    if m["kernel"] in (LINEAR, POLY):   # fp64 products and sums: ceil(dim / 64) per lane + 6 shuffle levels (inside the 8), then the outer sum
        return (lanes + 8 + 2 * degree(m)) * U53 * scale(m, x) + _outer_units(m) * U53 * scale(m, x)
    if m["kernel"] == HIK:              # float sum of ceil(dim / 64) terms per lane + 6 shuffle levels
        return (lanes + 9) * U24 * scale(m, x)
    return np.full(len(x), (lanes + 9) * U24 * coeff_sum(m))   # RBF: relative error E of the SSD, |dK| <= gamma ssd K E <= E / e


def oracle_bound(m, x, path):
    """the same for the CPU oracle (oracle/orc_classify.cpp), whose kernel argument is ONE sequential sum of dim terms: float for RBF and
    HIK, double for the dot product.  dim takes the place of the kernel's ceil(dim / 64) + shuffle levels; for the polynomial kernel the
    error of the dot product reaches the kernel value multiplied by the degree (d base^g = g base^(g-1) p0 d dot, |p0 dot| <= |base| on
    the magnitudes scale() uses).  Measured on f32-poly3-d4099-s3: the oracle's 4099-term double sum is 126 units of 2^-53 scale() off,
    more than the 96 the kernel is allowed there."""
    dim = np.asarray(m["sv"]).shape[1]
    if path == "generic" and m["kernel"] in (LINEAR, POLY):
        return (max(degree(m), 1) * dim + 8 + 2 * degree(m) + _outer_units(m)) * U53 * scale(m, x)
    if path == "generic" and m["kernel"] == HIK:
        return np.asarray(m["sv"]).shape[1] * U24 * scale(m, x)
    if path == "generic" and m["kernel"] == RBF:
        return np.full(len(x), np.asarray(m["sv"]).shape[1] * U24 * coeff_sum(m))
    return bound(m, x, path)


# ---- the launchers' limits, restated from csrc/svm.hip -----------------------------------------------------------------------------------
LDS_LIMIT = 64 * 1024            # SVM_LDS_LIMIT: the dynamic LDS of a launch; the kernels' small static arrays do not count against it
F32_GENERIC_MAX_DIM = LDS_LIMIT // 4   # k_svm_generic stages one row: dim * 4 <= 64 KiB


def u8_lanes_fits(dim, pb):
    return pb * ((dim + 15) & ~15) <= LDS_LIMIT   # k_svm_u8_lanes stages pb rows padded to 16 bytes


U8_LANES_MAX_DIM = max(d for d in range(32000, 33000) if u8_lanes_fits(d, 2))


def u8_lanes_production_pb(dim, n):
    pb = 8 if n >= 16384 else 4 if n >= 8192 else 2
    while pb > 2 and not u8_lanes_fits(dim, pb):
        pb //= 2
    return pb


def u8_mfma_lds_bytes(dim, nsv):
    ks, nsv32 = (dim + 31) // 32, (nsv + 31) & ~31
    return 32 * (ks * 32 + 16) + 384 + 8 * (nsv32 // 32) * 32


def u8_mfma_available(m):
    nsv, dim = np.asarray(m["sv"]).shape
    return m["dtype"] == U8 and m["kernel"] == RBF and dim <= 1536 and u8_mfma_lds_bytes(dim, nsv) <= LDS_LIMIT


def u8_mfma_max_nsv(dim):
    """the largest support-vector count fd_svm_u8_mfma_available accepts at this length"""
    nsv = 32
    while u8_mfma_lds_bytes(dim, nsv + 32) <= LDS_LIMIT:
        nsv += 32
    return nsv


def rbf_mfma_lds_bytes(dim):
    kp = (dim + 7) & ~7
    return 2 * (kp // 8) * 256 * 4 + 64 * 4 + 8 * 64 * 8      # fd_svm_rbf_lds_bytes; the budget is 160 KiB


def svs_persistent_n(num_cus):
    return 64 * (num_cus // 2) * 2 + 70


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _model(kernel, dtype, sv, rng, p0=0.0, p1=0.0, p2=0):
    return dict(kernel=kernel, p0=p0, p1=p1, p2=p2, dtype=dtype, sv=sv, coeff=rng.normal(0, 1, len(sv)).astype(np.float32), bias=np.float32(0.25),
                threshold=0.0)


def _case(name, m, store, path, idx=None, **kw):
    """store: the rows as they lie in memory, [n, width >= dim]; only the first dim elements of a row belong to the vector"""
    dim = np.asarray(m["sv"]).shape[1]
    c = types.SimpleNamespace(name=name, m=m, store=store, dim=dim, path=path, idx=None if idx is None else np.asarray(idx, np.uint32), **kw)
    c.rows = np.ascontiguousarray(store[:, :dim] if idx is None else store[:, :dim][c.idx])   # what the launch scores, in output order
    return c


def _saturate(a):
    """rows 0..2: all 0, all 255, 0 / 255 alternating (the -128 shift and the zero padding at saturation)"""
    if len(a) >= 3:
        a[0], a[1] = 0, 255
        a[2] = np.where(np.arange(a.shape[1]) % 2 == 0, 0, 255)


def _u8(name, kernel, dim, nsv, n, width=None, p0=0.0, p1=0.0, p2=0, saturate=True):
    rng = _rng(name)
    sv = rng.integers(0, 256, (nsv, dim), dtype=np.uint8)
    store = rng.integers(0, 256, (n, width or dim), dtype=np.uint8)
    if saturate:
        _saturate(sv)
        _saturate(store[:, :dim])
    m = _model(kernel, U8, sv, rng, p0, p1, p2)
    # the mutants of test_svm_score_model.py must show: the last row and the support vector they edit differ in their last element
    store[-1, dim - 1], sv[int(np.argmax(np.abs(m["coeff"]))), dim - 1] = 201, 90
    return m, store


U8_MFMA_SHAPES = [(1, 1, 1), (3, 31, 31), (31, 33, 32), (33, 96, 33), (397, 31, 65), (400, 96, 65), (1535, 40, 33), (1536, 40, 65)]
U8_LANES_SHAPES = [(1, 1), (15, 63), (16, 64), (17, 65), (400, 130), (1600, 64)]
U8_LANES_N = 37
U8_THRESHOLD_N = (8191, 8193, 16383, 16387)
U8_LONG = (8200, 3, 16384)
F32_SHAPES = [(1, 1), (63, 3), (64, 4), (65, 5), (400, 200), (4099, 3)]
F32_KINDS = {   # kind: (kernel, degree, signed rows)
    "linear": (LINEAR, 0, False), "linear-signed": (LINEAR, 0, True), "poly1": (POLY, 1, False), "poly1-signed": (POLY, 1, True),
    "poly2": (POLY, 2, False), "poly3": (POLY, 3, False), "poly3-signed": (POLY, 3, True), "rbf": (RBF, 0, False), "hik": (HIK, 0, False)}
RBF_MFMA_SHAPES = [(1, 1, 1), (8, 255, 63), (9, 256, 64), (24, 257, 65), (32, 1, 130), (33, 255, 130), (41, 256, 65), (49, 257, 63), (324, 257, 130),
                   (600, 256, 65)]
RBF_MFMA_REFUSED_DIM = 640
RBF_SVS_SHAPES = [(321, 1, 1), (324, 257, 33), (328, 257, 65), (329, 257, 1), (329, 1, 33), (336, 257, 65)]

_BUILDERS = {}


def _register(name, fn):
    assert name not in _BUILDERS
    _BUILDERS[name] = fn
    return name


def _names(prefix):
    return [n for n in _BUILDERS if n.startswith(prefix)]


for _d, _s, _n in U8_MFMA_SHAPES:
    _register("u8mfma-d%d-s%d-n%d" % (_d, _s, _n),
              lambda name, d=_d, s=_s, n=_n: _case(name, *_u8(name, RBF, d, s, n, p0=GAMMA_U8), path="u8"))


def _u8_idx(name, width):
    m, store = _u8(name, RBF, 400, 96, 65, width=width, p0=GAMMA_U8)
    idx = _rng(name + "/idx").integers(0, 65, 70)
    idx[:4] = (64, 0, 64, 2)   # repeated slots, the last row, saturated rows
    return _case(name, m, store, "u8", idx=idx)


_register("u8mfma-idx-bytes", lambda name: _u8_idx(name, 403))   # a stride that is no multiple of 4 forces byte staging at dim = 400
_register("u8mfma-idx-words", lambda name: _u8_idx(name, 400))
_register("u8mfma-count", lambda name: _case(name, *_u8(name, RBF, 400, 96, 65, p0=GAMMA_U8), path="u8"))
_register("u8bound-accepted", lambda name: _case(name, *_u8(name, RBF, 1536, u8_mfma_max_nsv(1536), 33, p0=GAMMA_U8), path="u8"))
_register("u8bound-refused", lambda name: _case(name, *_u8(name, RBF, 1536, u8_mfma_max_nsv(1536) + 1, 33, p0=GAMMA_U8), path="u8"))

for _d, _s in U8_LANES_SHAPES:
    _register("u8lanes-hik-d%d-s%d" % (_d, _s), lambda name, d=_d, s=_s: _case(name, *_u8(name, HIK, d, s, U8_LANES_N), path="u8"))
    _register("u8lanes-linear-d%d-s%d" % (_d, _s), lambda name, d=_d, s=_s: _case(name, *_u8(name, LINEAR, d, s, U8_LANES_N), path="u8"))
for _g, _d, _s in [(1, 15, 63), (2, 17, 65), (3, 400, 130), (3, 1, 1)]:
    _register("u8lanes-poly%d-d%d-s%d" % (_g, _d, _s),
              lambda name, g=_g, d=_d, s=_s: _case(name, *_u8(name, POLY, d, s, U8_LANES_N, p0=P0_U8_POLY, p1=P1_POLY, p2=g), path="u8"))
for _s in (1, 130):   # dim > 1536: no MFMA tables, RBF runs in k_svm_u8_lanes
    _register("u8lanes-rbf-d1600-s%d" % _s, lambda name, s=_s: _case(name, *_u8(name, RBF, 1600, s, U8_LANES_N, p0=GAMMA_U8), path="u8"))
for _k, _kn in ((HIK, "hik"), (LINEAR, "linear")):
    _register("u8thresholds-" + _kn, lambda name, k=_k: _case(name, *_u8(name, k, 48, 70, max(U8_THRESHOLD_N)), path="u8"))
_register("u8long-hik", lambda name: _case(name, *_u8(name, HIK, *U8_LONG, saturate=False), path="u8"))


def _f32(name, kernel, deg, signed, dim, nsv, n):
    rng = _rng(name)
    draw = (lambda shape: ((rng.random(shape) - 0.5) * 0.4).astype(np.float32)) if signed else (lambda shape: (rng.random(shape) * 0.2).astype(np.float32))
    sv, store = draw((nsv, dim)), draw((n, dim))
    p0 = {POLY: 0.3, RBF: 0.5}.get(kernel, 0.0)
    return _case(name, _model(kernel, F32, sv, rng, p0, P1_POLY if kernel == POLY else 0.0, deg), store, "generic")


for _kind, (_k, _g, _sg) in F32_KINDS.items():
    for _d, _s in F32_SHAPES:
        _register("f32-%s-d%d-s%d" % (_kind, _d, _s), lambda name, k=_k, g=_g, sg=_sg, d=_d, s=_s: _f32(name, k, g, sg, d, s, 7))
for _kind in ("linear", "rbf"):
    _register("f32count-" + _kind, lambda name, k=F32_KINDS[_kind][0]: _f32(name, k, 0, False, 63, 5, 65))
for _kind, (_k, _g, _sg) in F32_KINDS.items():
    if not _sg and _g in (0, 3):   # the longest vector the launcher accepts
        _register("f32longest-" + _kind, lambda name, k=_k, g=_g: _f32(name, k, g, False, F32_GENERIC_MAX_DIM, 2, 2))
_register("u8longest-hik", lambda name: _case(name, *_u8(name, HIK, U8_LANES_MAX_DIM, 2, 2, saturate=False), path="u8"))


def _hog_like(rng, n, dim):
    """non-negative rows with 0.5 <= |x|^2 <= 4"""
    v = rng.random((n, dim)) + 0.05
    v *= np.sqrt(rng.uniform(0.55, 3.9, n) / (v * v).sum(1))[:, None]
    v = v.astype(np.float32)
    assert np.all((v.astype(np.float64) ** 2).sum(1) >= 0.5) and np.all((v.astype(np.float64) ** 2).sum(1) <= 4.0)
    return v


def _mfma(name, dim, nsv, n):
    rng = _rng(name)
    sv = _hog_like(rng, nsv, dim)
    return _case(name, _model(RBF, F32, sv, rng, p0=0.5), _hog_like(rng, n, dim), "mfma")


for _d, _s, _n in RBF_MFMA_SHAPES:
    _register("rbfmfma-d%d-s%d-n%d" % (_d, _s, _n), lambda name, d=_d, s=_s, n=_n: _mfma(name, d, s, n))
_register("rbfmfma-refused-d%d" % RBF_MFMA_REFUSED_DIM, lambda name: _mfma(name, RBF_MFMA_REFUSED_DIM, 3, 2))
for _d, _s, _n in RBF_SVS_SHAPES:
    _register("rbfsvs-d%d-s%d-n%d" % (_d, _s, _n), lambda name, d=_d, s=_s, n=_n: _mfma(name, d, s, n))
SVS_PERSISTENT = "rbfsvs-persistent"   # built for a CU count: case(SVS_PERSISTENT, num_cus)

NAMES = list(_BUILDERS)
U8_NAMES = [n for n in NAMES if n.startswith("u8")]


def names(prefix):
    return _names(prefix)


@functools.lru_cache(maxsize=None)
def case(name, num_cus=256):
    """the case of that name, built once per process; treat it as read-only"""
    if name == SVS_PERSISTENT:
        c = _mfma(name, 324, 257, svs_persistent_n(num_cus))
    else:
        c = _BUILDERS[name](name)
    for a in (c.store, c.rows, c.m["sv"], c.m["coeff"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, num_cus=256):
    """(distance, bound) of the case's rows, computed once"""
    c = case(name, num_cus)
    d, b = distance(c.m, c.rows), bound(c.m, c.rows, c.path)
    d.setflags(write=False)
    b.setflags(write=False)
    return d, b
