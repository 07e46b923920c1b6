"""numpy restatement of the four histogram patch filters (HistogramFilter.cpp:23-251, HogFilter.cpp:58-122, SpatialHistogramFilter.cpp:56-94,
PyramidHogFilter.cpp:33-113, SpatialPyramidHistogramFilter.cpp:37-81), the error bound k_hist_features and k_hog_tile (csrc/hog.hip) are
held to, the fragment-major layout of the f32 MFMA operand, and the ONE seeded case builder of tests/test_hist_model.py (no GPU) and
tests/test_gpu_hist_features.py (the kernels).  Written from the reference's source, neither from oracle/ nor from the kernels.

features(case, patches) walks the reference's loops (pixels row-major, the four cell neighbours of a pixel in the reference's order, cells,
blocks and pyramid levels in its order) with all patches of the batch side by side, in float64.  The constants the reference holds as
floats enter as those float32 values, widened: 1.f / 255.f, eps = 1e-4f, the clip 0.2 and the cache weights (weight2 = float(realIndex -
index1), weight1 = 1.f - weight2, a float subtraction).  So the model differs from the reference by accumulation rounding only.
features32 is the same walk in float32 (with the reference's double sums inside normalize): the reference's own arithmetic, bit for bit.
Cell counts are cvRound's (half to even).  A bin value >= binCount contributes nothing: that is the library's defined behaviour; the
reference indexes its histogram with the raw byte and reads and writes past it there.

bound(case, patches): every quantity on the way to an output element is a sum or a product of non-negative numbers (or a quotient or a
square root of such), so the float32 result of a quantity q is q (1 + theta) with |theta| <= gamma_k = k u / (1 - k u), u = 2^-24, where
k counts the float32 roundings on the longest path to it; + and * count one rounding, / and sqrt two.  The counts, with
(1 + theta_a) / (1 + theta_b) = 1 + theta_(a + 2 b):
  cell histogram entry    kc = P * ops: P the most pixel contributions one cell receives (row entries x column entries of the busiest
                          cell, twice that for two bins per pixel), ops the operations per contribution: 1 (count), 2 (factor * weight,
                          add), 2 (row weight * column weight, add) or 4 (factor * weight * row weight * column weight, add)
  unsigned bin            ku = kc + 1
  energy of nb bins       ke = 2 kh + 1 + nb (a square doubles the count of its argument), block energy kE = ke + cells per block
  HOG normaliser          kn = kE + 1 (+ eps) + 2 (sqrt) + 2 (1 / .); an output element kh + 1 + 2 kn
  pyramid level           four adds per level above the finest
  block sum               + cells per block (concatenated: + 1)
  normalize, L2           the double sum of squares of a vector whose entries have at most kmax: 2 kmax + 1 (all float64 roundings of
                          the sum, the square root and the division together are below one float32 unit: fewer than 2^28 of them);
                          kd = 2 kmax + 1 + 2 (sqrt, rounded to float) + 1 (+ eps) + 2 (1 / ., rounded to float); an element k + 1 + 2 kd.
                          The wave-reduced form of the 1x1-block SpatialHistogramFilter sums the same float64 terms in another order:
                          the same count.
  L1                      kd = kmax + 1 + 1 + 1 + 2; an element k + 1 + 2 kd;  L1SQRT: + 2
  L2HYS                   min(., 0.2) is 1-Lipschitz: an entry v with |error| <= gamma_k v becomes c = min(v, 0.2) with the same absolute
                          error, gamma_k (v / c) c <= gamma_(k v / c) c: the count is multiplied by max(1, v / 0.2), then L2 again.
An element whose model value is exactly 0 has the bound 0: sums of non-negative terms are 0 only when every term is."""
import functools
import types
import zlib

import numpy as np

HOG, SPATIAL, PYRAMID_HOG, SPATIAL_PYRAMID = 0, 1, 2, 3
NONE, L2NORM, L2HYS, L1NORM, L1SQRT = 0, 1, 2, 3, 4
U24 = 2.0 ** -24
F32 = np.float32
FACTOR, EPS, CLIP = F32(1) / F32(255), F32(1e-4), F32(0.2)
LDS_BUDGET = 160 * 1024
MUTANTS = ("cell_end_rounds_up", "cells_past_64_dropped", "blocks_past_64_dropped", "block_walk_uses_rows_for_cols", "eps_outside_sqrt",
           "unsigned_half_from_signed_energy", "out_of_range_bin_clamped", "interp_same_cell_added_once", "stale_vector_from_previous_window")
FRAG_MUTANTS = ("pad_elements_not_zero", "xx_without_last_block", "rows_past_N_not_zero")


def cv_round(v):
    return int(np.rint(v))   # half to even, like cvRound


def geometry(c):
    g = types.SimpleNamespace(hb=c.bins // 2)
    if c.kind in (HOG, SPATIAL):
        g.rows, g.cols = cv_round(c.ph / (c.cell_h or c.cell)), cv_round(c.pw / c.cell)
        g.bw, g.bh = c.block, c.block_h or c.block
        g.brows, g.bcols = g.rows - g.bh + 1, g.cols - g.bw + 1
        g.real = c.bins + g.hb if c.kind == HOG and c.sau else c.bins
        if c.kind == HOG:
            g.F = g.brows * g.bcols * g.bw * g.bh * g.real
        elif g.bw == 1 and g.bh == 1:
            g.F = g.rows * g.cols * c.bins
        else:
            g.F = g.brows * g.bcols * (g.bw * g.bh * c.bins if c.concatenate else c.bins)
    else:
        g.max_level = c.levels - 1
        g.rows = g.cols = 1 << g.max_level
        g.hist_count = sum(1 << (2 * l) for l in range(c.levels))
        g.real = c.bins + g.hb if c.kind == PYRAMID_HOG and c.sau else c.bins
        g.F = g.hist_count * g.real
    return g


def _axis(size, count, interpolate, mutant=None):
    """per pixel index of one axis: the (cell, weight) entries it feeds, in the reference's order"""
    ent = [[] for _ in range(size)]
    if not interpolate:   # HistogramFilter.cpp:144-147
        for i in range(count):
            end = ((i + 1) * size) // count
            if mutant == "cell_end_rounds_up":
                end = min(size, -((-(i + 1) * size) // count))
            for m in range((i * size) // count, end):
                ent[m].append((i, 1.0))
        return ent
    for m in range(size):   # createCache, HistogramFilter.cpp:199-220
        real = float(count) * (float(m) + 0.5) / float(size) - 0.5
        i1 = int(np.floor(real))
        i2 = i1 + 1
        w2 = F32(real - i1)
        w1 = F32(1) - w2
        if i1 < 0:
            i1, w1 = i2, F32(0)
        elif i2 >= count:
            i2, w2 = i1, F32(0)
        ent[m] = [(i1, float(w1)), (i2, float(w2))]
        if mutant == "interp_same_cell_added_once" and i1 == i2:
            ent[m] = ent[m][:1]
    return ent


def _seq(a):
    """sum over the last axis, one addend after the other"""
    return np.add.accumulate(a, axis=-1)[..., -1]


def _cells(c, g, patches, dt, mutant):
    n, B = len(patches), c.bins
    P = np.ascontiguousarray(patches, np.uint8).reshape(n, c.ph, c.pw, c.ch)
    H = np.zeros((n, g.rows, g.cols, B), dt)
    ar = np.arange(n)
    rent, cent = _axis(c.ph, g.rows, c.interpolate, mutant), _axis(c.pw, g.cols, c.interpolate, mutant)
    planes = []
    for k in range(max(1, c.ch // 2)):
        b = P[..., 2 * k].astype(np.intp)
        if mutant == "out_of_range_bin_clamped":
            b = np.minimum(b, B - 1)
        planes.append((b, None if c.ch == 1 else dt(FACTOR) * P[..., 2 * k + 1].astype(dt), bool((b >= B).any())))
    for y in range(c.ph):
        for x in range(c.pw):
            for r, wr in rent[y]:
                for cc, wc in cent[x]:
                    for b, w, oob in planes:
                        bb = b[:, y, x]
                        if c.interpolate:
                            val = dt(wr) * dt(wc) if w is None else (w[:, y, x] * dt(wr)) * dt(wc)
                        else:
                            val = dt(1) if w is None else w[:, y, x]
                        if oob:
                            ok = bb < B
                            H[ar[ok], r, cc, bb[ok]] += val if w is None else val[ok]
                        else:
                            H[ar, r, cc, bb] += val
    if mutant == "cells_past_64_dropped":
        H.reshape(n, -1, B)[:, 64:] = 0
    if mutant == "stale_vector_from_previous_window" and getattr(c, "grid", 0) and n > c.grid:
        H[c.grid:] += H[:n - c.grid].copy()
    return H


def _normalize(v, k, mode, dt, aux):
    """HistogramFilter::normalize on the last axis of v; k: the rounding counts of its entries"""
    k = np.broadcast_to(np.asarray(k, np.float64), v.shape)

    def scaled(v, k, s, kd):
        norm = s.astype(dt)
        inv = (1.0 / (norm + dt(EPS)).astype(np.float64)).astype(dt)
        return v * inv[..., None], k + 1 + 2 * kd[..., None]

    def l2(v, k):
        d = v.astype(np.float64)
        return scaled(v, k, np.sqrt(_seq(d * d)), 2 * k.max(-1) + 6)

    def l1(v, k):
        return scaled(v, k, _seq(np.abs(v.astype(np.float64))), k.max(-1) + 5)

    if mode == L2NORM:
        return l2(v, k)
    if mode == L2HYS:
        v, k = l2(v, k)
        aux["clipped"] = aux.get("clipped", 0) + int((v > dt(CLIP)).sum())
        k = k * np.maximum(1.0, v.astype(np.float64) / float(CLIP))
        return l2(np.minimum(v, dt(CLIP)), k)
    if mode == L1NORM:
        return l1(v, k)
    if mode == L1SQRT:
        v, k = l1(v, k)
        return np.sqrt(v), k + 2
    return v, k


def _pixel_contributions(c, g, positive=False):
    """entries per cell row and per cell column (positive: only those with a weight above 0)"""
    rent, cent = _axis(c.ph, g.rows, c.interpolate), _axis(c.pw, g.cols, c.interpolate)
    per_row, per_col = np.zeros(g.rows, int), np.zeros(g.cols, int)
    for e in rent:
        for i, w in e:
            per_row[i] += w > 0 or not positive
    for e in cent:
        for i, w in e:
            per_col[i] += w > 0 or not positive
    return per_row, per_col


def _evaluate(c, patches, dt=np.float64, mutant=None, aux=None):
    """(features [n, F], rounding counts broadcastable to them)"""
    aux = {} if aux is None else aux
    g = geometry(c)
    n, B, hb = len(patches), c.bins, c.bins // 2
    H = _cells(c, g, patches, dt, mutant)
    per_row, per_col = _pixel_contributions(c, g)
    ops = (2 if c.ch == 1 else 4) if c.interpolate else (1 if c.ch == 1 else 2)
    kc = float(max(1, per_row.max() * per_col.max()) * (2 if c.ch == 4 else 1) * ops)
    eps_out = mutant == "eps_outside_sqrt"

    def normaliser(en):   # 1.f / sqrt(energy + eps)
        return dt(1) / (np.sqrt(en) + dt(EPS)) if eps_out else dt(1) / np.sqrt(en + dt(EPS))

    if c.kind == HOG:
        hv = H.reshape(n, g.rows * g.cols, B)
        U = hv[..., :hb] + hv[..., hb:2 * hb] if c.sau else None
        E = _seq(U * U) if c.sau and mutant != "unsigned_half_from_signed_energy" else _seq(hv * hv)   # HogFilter.cpp:102-122
        ku = kc + 1 if c.sau else kc
        kn = (2 * ku + 1 + (hb if c.sau else B)) + g.bw * g.bh + 5
        stride = g.rows if mutant == "block_walk_uses_rows_for_cols" else g.cols
        out = []
        for bl in range(g.brows * g.bcols):   # HogFilter.cpp:69-100
            br, bc = divmod(bl, g.bcols)
            cells = [((br + dr) * stride + bc + dc) % (g.rows * g.cols) for dr in range(g.bh) for dc in range(g.bw)]
            en = np.zeros(n, dt)
            for ci in cells:
                en = en + E[:, ci]
            nrm = normaliser(en)[:, None]
            for ci in cells:
                out.append(nrm * hv[:, ci])
                if c.sau:
                    out.append(nrm * U[:, ci])
            if mutant == "blocks_past_64_dropped" and bl >= 64:
                for o in out[-(len(cells) * (2 if c.sau else 1)):]:
                    o[...] = 0
        return np.concatenate(out, axis=1), ku + 1 + 2 * kn
    if c.kind == SPATIAL:
        if g.bw == 1 and g.bh == 1:   # SpatialHistogramFilter.cpp:59-61
            return _normalize(H.reshape(n, -1), kc, c.normalization, dt, aux)
        stride = g.rows if mutant == "block_walk_uses_rows_for_cols" else g.cols
        hv = H.reshape(n, g.rows * g.cols, B)
        out, ks = [], []
        for bl in range(g.brows * g.bcols):   # :70-94
            br, bc = divmod(bl, g.bcols)
            cells = [((br + dr) * stride + bc + dc) % (g.rows * g.cols) for dr in range(g.bh) for dc in range(g.bw)]
            if c.concatenate:
                v, k = np.concatenate([hv[:, ci] for ci in cells], axis=1), kc + 1
            else:
                v = np.zeros((n, B), dt)
                for ci in cells:
                    v = v + hv[:, ci]
                k = kc + len(cells)
            v, k = _normalize(v, k, c.normalization, dt, aux)
            if mutant == "blocks_past_64_dropped" and bl >= 64:
                v = np.zeros_like(v)
            out.append(v)
            ks.append(np.broadcast_to(k, v.shape))
        return np.concatenate(out, axis=1), np.concatenate(ks, axis=1)
    # the pyramid kinds: PyramidHogFilter.cpp:33-113, SpatialPyramidHistogramFilter.cpp:37-81
    G = g.rows
    level = H
    if c.kind == PYRAMID_HOG and c.sau:   # copyCellHistograms
        level = np.concatenate([H, H[..., :hb] + H[..., hb:2 * hb]], axis=-1)
    kh = kc + 1 if c.kind == PYRAMID_HOG and c.sau else kc
    levels, counts = [level.reshape(n, G * G, g.real)], [kh]
    for lv in range(g.max_level - 1, -1, -1):   # combineHistograms: the four children in row-major order, added to zero
        level = ((level[:, 0::2, 0::2] + level[:, 0::2, 1::2]) + level[:, 1::2, 0::2]) + level[:, 1::2, 1::2]
        kh = kh + 4
        levels.insert(0, level.reshape(n, -1, g.real))
        counts.insert(0, kh)
    out, ks = [], []
    for hv, kh in zip(levels, counts):
        if c.kind == PYRAMID_HOG:   # normalizeHistograms
            part = hv[..., B:] if c.sau and mutant != "unsigned_half_from_signed_energy" else hv[..., :B]
            kn = 2 * kh + 1 + part.shape[-1] + 5
            v, k = normaliser(_seq(part * part))[..., None] * hv, kh + 1 + 2 * kn
        else:
            v, k = _normalize(hv, kh, c.normalization, dt, aux)
        out.append(v.reshape(n, -1))
        ks.append(np.broadcast_to(k, v.shape).reshape(n, -1))
    return np.concatenate(out, axis=1), np.concatenate(ks, axis=1)


def features(c, patches, mutant=None, aux=None):
    """float64 [n, F]"""
    return _evaluate(c, patches, np.float64, mutant, aux)[0]


def features32(c, patches):
    """float32 [n, F]: the reference's own arithmetic in the reference's order"""
    out = _evaluate(c, patches, np.float32)[0]
    assert out.dtype == np.float32
    return out


def bound(c, patches):
    """float64 [n, F]: gamma_k |feature|"""
    v, k = _evaluate(c, patches, np.float64)
    k = np.broadcast_to(np.asarray(k, np.float64), v.shape)
    assert np.all(k * U24 < 0.5)
    return k * U24 / (1 - k * U24) * v


def oracle_features(oracle, c, patches):
    """the CPU oracle's filter of the case on every patch, float32 [n, F]"""
    kw = dict(interpolate=c.interpolate)
    if c.kind == HOG:
        fn = lambda p: oracle.hog_filter(p, c.bins, c.cell, c.block, signed_and_unsigned=c.sau, cell_h=c.cell_h, block_h=c.block_h, **kw)
    elif c.kind == SPATIAL:
        fn = lambda p: oracle.spatial_histogram(p, c.bins, c.cell, c.block, concatenate=c.concatenate, normalization=c.normalization,
                                                cell_h=c.cell_h, block_h=c.block_h, **kw)
    elif c.kind == PYRAMID_HOG:
        fn = lambda p: oracle.pyramid_hog(p, c.bins, c.levels, signed_and_unsigned=c.sau, **kw)
    else:
        fn = lambda p: oracle.spatial_pyramid_histogram(p, c.bins, c.levels, normalization=c.normalization, **kw)
    return np.stack([np.asarray(fn(np.ascontiguousarray(p)), np.float32).ravel() for p in patches])


def worst(err, b):
    """(largest error / bound, flat index); an error where the bound is 0 counts as infinite"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i


def exact(c):
    """kinds the kernel computes in the reference's order (tests/test_gpu_parity.py::test_histogram_filters_match_oracle): everything but
    the whole-vector normalisation of the 1x1-block SpatialHistogramFilter"""
    return not (c.kind == SPATIAL and c.block == 1 and (c.block_h or 1) == 1 and c.normalization != NONE)


def lds_bytes(c):
    """hist_lds_bytes of csrc/hog.hip: the patch, the four tables, the output vector with the raw cells and scratch behind it"""
    g = geometry(c)
    ncell = g.rows * g.cols
    if c.kind == HOG:
        floats = ((g.F + 3) & ~3) + ncell * c.bins + ncell + g.brows * g.bcols
    elif c.kind == PYRAMID_HOG or (c.kind == SPATIAL and not (g.bw == 1 and g.bh == 1)):
        floats = ((g.F + 3) & ~3) + ncell * c.bins
    else:
        floats = g.F
    return ((c.pw * c.ph * c.ch + 15) & ~15) + 16 * (c.pw + c.ph) + 4 * (g.rows + g.cols) + 16 + 4 * floats


# ---- the fragment-major operand of the f32 MFMA SVM (csrc/rbf_mfma.hpp) ------------------------------------------------------------
def frag_layout(rows, KP):
    """index [rows, KP] into the fragment-major buffer: tiles of 32 vectors of KP = 8 Q floats; a tile is Q groups of 256 floats, in a
    group the float4 of lane (h, r) holds elements 8 q + 4 h .. + 3 of vector r"""
    row, k = np.arange(rows, dtype=np.int64)[:, None], np.arange(KP, dtype=np.int64)[None, :]
    return (row >> 5) * 32 * KP + (k >> 3) * 256 + (((k >> 2) & 1) * 32 + (row & 31)) * 4 + (k & 3)


def frag_buffers(feat, per_block, mutant=None):
    """what k_hog_tile<true> leaves for the SVM: (fragment-major buffer of Npad rows, |x|^2 per row, KP); Npad = N rounded up to 64"""
    feat = np.asarray(feat, np.float64)
    N, F = feat.shape
    KP, npad = (F + 7) & ~7, (N + 63) & ~63
    lay = frag_layout(npad, KP)
    buf, xx = np.zeros(npad * KP), np.zeros(npad)
    buf[lay[:N, :F]] = feat
    xx[:N] = (feat * feat).sum(1)
    if mutant == "pad_elements_not_zero":   # the padding repeats the last element (and is summed into |x|^2 like every stored element)
        buf[lay[:N, F:]] = feat[:, F - 1:F]
        xx[:N] += (KP - F) * feat[:, F - 1] ** 2
    elif mutant == "xx_without_last_block":
        xx[:N] -= (feat[:, F - per_block:] ** 2).sum(1)
    elif mutant == "rows_past_N_not_zero":   # the rest of the last 32-row tile repeats the last window
        last = ((N + 31) & ~31)
        buf[lay[N:last]] = buf[lay[N - 1]]
        xx[N:last] = xx[N - 1]
    else:
        assert mutant is None
    return buf, xx, KP


def frag_distance(m, buf, xx, KP):
    """-bias + sum c exp(-gamma (|x|^2 + |s|^2 - 2 x.s)) for EVERY row of the buffer, the way the matrix-pipe kernel forms it"""
    sv = np.asarray(m["sv"], np.float32).astype(np.float64)
    svp = np.zeros((len(sv), KP))
    svp[:, :sv.shape[1]] = sv
    rows = buf[frag_layout(len(xx), KP)]
    ssd = np.maximum(xx[:, None] + (svp * svp).sum(1)[None, :] - 2 * rows @ svp.T, 0)
    return (np.exp(-float(m["p0"]) * ssd) * np.asarray(m["coeff"], np.float32).astype(np.float64)[None, :]).sum(1) - float(np.float32(m["bias"]))


def rbf_mfma_fits(F):
    kp = (F + 7) & ~7
    return 2 * (kp // 8) * 256 * 4 + 64 * 4 + 8 * 64 * 8 <= LDS_BUDGET   # fd_svm_rbf_lds_bytes


def svm_for(name, feats, nsv=24):
    """the seeded f32 RBF model of a k_hog_tile case: support vectors drawn from the features, gamma = 1 / median squared distance"""
    rng = _rng(name + "/svm")
    feats = np.ascontiguousarray(feats, np.float32)
    sv = feats[rng.choice(len(feats), min(nsv, len(feats)), replace=False)].copy()
    f64, s64 = feats.astype(np.float64), sv.astype(np.float64)
    ssd = np.maximum((f64 * f64).sum(1)[:, None] + (s64 * s64).sum(1)[None, :] - 2 * f64 @ s64.T, 0)
    gamma = 1.0 / float(np.median(ssd))
    m = dict(kernel=2, p0=gamma, p1=0.0, p2=0, dtype=1, sv=sv, coeff=rng.normal(0, 1, len(sv)).astype(np.float32), bias=np.float32(0.25),
             threshold=0.0)
    return m, np.exp(-gamma * ssd)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


CASES = {}      # fd_hist_patch_batch: name -> dict(params, n, content, tags)
DEFAULTS = dict(kind=HOG, pw=20, ph=20, ch=2, bins=9, cell=5, cell_h=0, block=1, block_h=0, levels=2, interpolate=False, sau=False,
                concatenate=False, normalization=L2NORM)
ZERO_CONTENT = ("zero-weights", "oob-bins", "oob-255")              # every output element is exactly 0
# the only cases that may leave more than a quarter of their output at exactly 0, by name, each sparse by construction
SPARSE_BY_CONSTRUCTION = {
    "hog-3x20-c1": "one pixel per cell: one of 9 bins", "hog-3x20-c1-interp": "cell size 1: the second cache weight is 0, one pixel per cell",
    "pyrhog-3x20-l5-interp": "16 x 16 cells on 3 x 20 pixels: the empty ranges of the table builder",
    "hog-one-bin-255": "one bin", "spatial-hys-one-bin-255": "one bin", "hog-corner-pixel": "one pixel", "spatial-hys-corner-pixel": "one pixel",
    "spatial-64x64-c5-bins233": "the LDS limit: 25 pixels on 233 bins", "spatial-64x64-c5-bins234": "the LDS limit: 25 pixels on 234 bins",
}


def _add(name, n=5, content="random", tags=(), **kw):
    assert name not in CASES and set(kw) <= set(DEFAULTS), name
    CASES[name] = dict(params=dict(DEFAULTS, **kw), n=n, content=content, tags=tuple(tags))


# geometry of k_hist_features
for _ip in (False, True):
    _s = "-interp" if _ip else ""
    _add("hog-27x27-c3-b1" + _s, pw=27, ph=27, bins=2, cell=3, block=1, interpolate=_ip, tags=("cells>64", "blocks>64", "F>>64"))
    _add("hog-23x17-c5-b2" + _s, pw=23, ph=17, cell=5, block=2, interpolate=_ip, tags=("cells do not divide",))
    _add("hog-10x10-c4" + _s, pw=10, ph=10, cell=4, interpolate=_ip, tags=("quotient 2.5",))
    _add("hog-14x14-c4" + _s, pw=14, ph=14, cell=4, interpolate=_ip, tags=("quotient 3.5",))
    _add("hog-8x8-c8-1cell" + _s, pw=8, ph=8, cell=8, interpolate=_ip, tags=("1x1 grid",))
    _add("hog-20x5-c5-1row" + _s, pw=20, ph=5, cell=5, interpolate=_ip, tags=("1xN grid",))
    _add("hog-5x20-c5-1col" + _s, pw=5, ph=20, cell=5, interpolate=_ip, tags=("Nx1 grid",))
    _add("spatial-8x8-c8-1cell" + _s, kind=SPATIAL, ch=1, bins=4, pw=8, ph=8, cell=8, interpolate=_ip, tags=("1x1 grid",))
    _add("spatial-20x5-c5-b2x1-1row" + _s, kind=SPATIAL, ch=1, bins=4, pw=20, ph=5, cell=5, block=2, block_h=1, interpolate=_ip, tags=("1xN grid",))
    _add("hog-3x20-c1" + _s, pw=3, ph=20, cell=1, interpolate=_ip, tags=("3x20 cell 1",))
    _add("pyrhog-3x20-l3" + _s, kind=PYRAMID_HOG, pw=3, ph=20, bins=2, levels=3, interpolate=_ip, tags=("more cells than pixels",))
_add("pyrhog-3x20-l5-interp", kind=PYRAMID_HOG, pw=3, ph=20, levels=5, interpolate=True, n=3, tags=("more cells than pixels", "empty range"))
_add("spatial-27x27-c3-b1", kind=SPATIAL, ch=1, bins=2, pw=27, ph=27, cell=3, tags=("cells>64",))
_add("hog-27x27-c3-b2", pw=27, ph=27, bins=2, cell=3, block=2, sau=True, tags=("blocks=64",))
_add("spatial-27x27-c3-b2-concat", kind=SPATIAL, ch=1, bins=3, pw=27, ph=27, cell=3, block=2, concatenate=True, normalization=L2HYS, tags=("blocks=64",))
_add("spatial-30x27-c3-b2", kind=SPATIAL, ch=1, bins=3, pw=30, ph=27, cell=3, block=2, normalization=L1NORM, tags=("blocks>64", "non-square grid"))
_add("hog-64x64-c8-b2-ch4-interp", pw=64, ph=64, ch=4, cell=8, block=2, interpolate=True, n=3, tags=("64x64",))
_add("hog-64x64-c8-b2", pw=64, ph=64, cell=8, block=2, n=3, tags=("64x64",))
_add("hog-64x5-c5", pw=64, ph=5, cell=5, tags=("64x5",))
_add("spatial-1x64-c1x8-interp", kind=SPATIAL, ch=1, bins=4, pw=1, ph=64, cell=1, cell_h=8, interpolate=True, tags=("1x64", "Nx1 grid"))
_add("spatial-1x64-c1x8", kind=SPATIAL, ch=1, bins=4, pw=1, ph=64, cell=1, cell_h=8, tags=("1x64", "Nx1 grid"))
for _b in (1, 59, 256):
    # 64 x 64 patches, 2 x 2 cells of 1024 pixels: every bin of 256 is met
    _add("spatial-bins%d-b1" % _b, kind=SPATIAL, ch=1, bins=_b, pw=64, ph=64, cell=32, n=4, tags=("bins %d" % _b,))
    _add("spatial-bins%d-b2-interp" % _b, kind=SPATIAL, ch=1, bins=_b, pw=64, ph=64, cell=32, block=2, interpolate=True, normalization=L2HYS, n=4,
         tags=("bins %d" % _b,))
_add("hog-bins64-ch2", bins=64, pw=64, ph=64, cell=32, block=2, n=4, tags=("bins 64 ch2",))
_add("hog-bins64-ch4-interp", bins=64, ch=4, block=2, interpolate=True, sau=True, tags=("bins 64 ch4",))
_add("spatial-bins64-ch4", kind=SPATIAL, bins=64, ch=4, block=2, normalization=L1SQRT, tags=("bins 64 ch4",))
_add("pyrhog-l1", kind=PYRAMID_HOG, levels=1, tags=("levels 1",))
_add("pyrhog-l2-sau", kind=PYRAMID_HOG, bins=8, levels=2, sau=True, tags=("levels 2", "sau level 2"))
_add("pyrhog-l3-sau-ch4-interp", kind=PYRAMID_HOG, ch=4, bins=8, levels=3, sau=True, interpolate=True, tags=("sau level 3",))
_add("pyrhog-32x32-l5", kind=PYRAMID_HOG, pw=32, ph=32, bins=2, levels=5, n=3, tags=("levels 5",))
_add("spyr-l1", kind=SPATIAL_PYRAMID, ch=1, bins=4, levels=1, normalization=L2NORM, tags=("levels 1",))
_add("spyr-l2-interp", kind=SPATIAL_PYRAMID, ch=1, bins=4, levels=2, interpolate=True, normalization=L2HYS, tags=("levels 2",))
_add("spyr-32x32-l5", kind=SPATIAL_PYRAMID, ch=1, bins=2, pw=32, ph=32, levels=5, normalization=L1SQRT, n=3, tags=("levels 5",))
_add("hog-28x20-c5x4-b2x3", pw=28, ph=20, cell=5, cell_h=4, block=2, block_h=3, sau=True, bins=8, tags=("non-square",))
_add("spatial-20x20-c4x10-b3x1-concat-interp", kind=SPATIAL, ch=1, bins=4, cell=4, cell_h=10, block=3, block_h=1, concatenate=True,
     interpolate=True, tags=("non-square",))
for _nz in range(5):
    _add("spatial-b2-norm%d" % _nz, kind=SPATIAL, bins=9, block=2, normalization=_nz, concatenate=False, tags=("block norm %d" % _nz,))
    _add("spatial-b2-concat-norm%d" % _nz, kind=SPATIAL, ch=1, bins=4, block=2, normalization=_nz, concatenate=True, tags=("block norm %d" % _nz, "concat"))
    _add("spatial-b1-norm%d" % _nz, kind=SPATIAL, ch=1, bins=16, normalization=_nz, tags=("wave norm %d" % _nz,))
# launch of k_hist_features
_add("launch-n1", n=1, block=2, tags=("n=1",))
_add("launch-second-window", kind=SPATIAL, ch=1, bins=4, pw=8, ph=8, cell=4, normalization=NONE, n=-1, tags=("second window",))   # n = num_cus * 32 + 3
# content, set by bytes
for _ct in ("zero-weights", "one-bin-255", "oob-bins", "oob-255", "oob-half", "corner-pixel", "alternate-0-255"):
    _add("hog-" + _ct, block=2, content=_ct, tags=(_ct,))
    _add("spatial-hys-" + _ct, kind=SPATIAL, block=2, normalization=L2HYS, interpolate=True, content=_ct, tags=(_ct,))
_add("spatial-l1sqrt-zero-weights", kind=SPATIAL, normalization=L1SQRT, content="zero-weights", tags=("l1sqrt of zeros",))
_add("spatial-ch1-oob-half", kind=SPATIAL, ch=1, bins=4, content="oob-half", tags=("oob-half", "lbp codes on fewer bins"))
_add("spatial-ch1-oob-255", kind=SPATIAL, ch=1, bins=59, content="oob-255", tags=("oob-255",))
_add("hog-ch4-both-bins-equal", ch=4, block=2, interpolate=True, content="both-equal", tags=("both-equal",))
_add("pyrhog-ch4-both-bins-equal", kind=PYRAMID_HOG, ch=4, levels=2, content="both-equal", tags=("both-equal",))
_add("spatial-hys-dominant-bin", kind=SPATIAL, bins=9, block=2, normalization=L2HYS, content="dominant", tags=("hys clips",))
# the LDS limit of fd_hist_patch_batch: 64 x 64 patches, 13 x 13 cells, one vector of 169 * bins floats
LDS_ACCEPTED, LDS_REFUSED = "spatial-64x64-c5-bins233", "spatial-64x64-c5-bins234"
_add(LDS_ACCEPTED, kind=SPATIAL, ch=1, bins=233, pw=64, ph=64, cell=5, n=3, tags=("lds accepted",))
_add(LDS_REFUSED, kind=SPATIAL, ch=1, bins=234, pw=64, ph=64, cell=5, n=3, tags=("lds refused",))
NAMES = list(CASES)


def _content(rng, content, n, c):
    B = c.bins
    bins = rng.integers(0, B, (n, c.ph, c.pw, max(1, c.ch // 2)))
    wts = rng.integers(0, 256, bins.shape)
    yy, xx = np.mgrid[:c.ph, :c.pw]
    checker = ((yy + xx) % 2 == 0)[None, :, :, None]
    oob = min(B, 255)   # the first value outside the histogram that a byte holds
    if content == "zero-weights":
        wts[:] = 0
    elif content == "one-bin-255":
        bins[:], wts[:] = B - 1, 255
    elif content == "oob-bins":
        bins[:] = oob
    elif content == "oob-255":
        bins[:] = 255
    elif content == "oob-half":
        bins = np.where(checker, bins, np.where(rng.random(bins.shape) < 0.5, oob, 255))
    elif content == "corner-pixel":
        wts[:] = 0
        wts[:, 0, 0], wts[-1, -1, -1] = 255, 255
    elif content == "alternate-0-255":
        wts = np.where(checker, 0, 255) + 0 * wts
    elif content == "both-equal":
        bins[..., 1] = bins[..., 0]
    elif content == "dominant":
        bins = np.where(rng.random(bins.shape) < 0.7, 0, bins)
    else:
        assert content == "random", content
    if c.ch == 1:
        return bins[..., 0].astype(np.uint8)
    return np.stack([bins, wts], axis=-1).reshape(n, c.ph, c.pw, c.ch).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name, num_cus=256):
    """the fd_hist_patch_batch case of that name, built once per process; treat it as read-only"""
    spec = CASES[name]
    c = types.SimpleNamespace(name=name, content=spec["content"], tags=spec["tags"], **spec["params"])
    n = spec["n"]
    if n < 0:
        c.grid = num_cus * 32   # the grid of k_hist_features: window i and window i + grid share a workgroup
        n = c.grid + 3
    c.patches = _content(_rng(name), c.content, n, c)
    # what the oracle can be given: it indexes its histogram with the raw byte, so an out-of-range bin becomes bin 0 with weight 0
    # (+ 0.f changes no accumulator); a one-channel image has no weight to clear
    c.oracle_patches = c.patches
    if (c.patches.reshape(n, c.ph, c.pw, c.ch)[..., 0::2] >= c.bins).any():
        c.oracle_patches = None
        if c.ch > 1:
            p = c.patches.reshape(n, c.ph, c.pw, c.ch // 2, 2).copy()
            p[p[..., 0] >= c.bins] = 0
            c.oracle_patches = p.reshape(c.patches.shape)
            c.oracle_patches.setflags(write=False)
    c.patches.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, num_cus=256):
    """(features, bound) of the case, float64, computed once"""
    c = case(name, num_cus)
    f, b = features(c, c.patches), bound(c, c.patches)
    f.setflags(write=False)
    b.setflags(write=False)
    return f, b


def patch_case(kind=HOG, **kw):
    """a parameter set outside the table (patches cut from pyramid layers)"""
    return types.SimpleNamespace(**dict(DEFAULTS, kind=kind, **kw))


# ---- the pyramid routes: gray images, k_hog_tile geometries ------------------------------------------------------------------------------------
REGION = 56   # side of the content regions: a 32 x 32 window with its gradient border fits them on the 0.7 layer too (39 pixels)


def gray_image(name, w, h):
    """full-range noise; an image of 100 pixels or more holds three regions larger than every patch on both layers: flat, a 0 / 255
    checkerboard, and vertical step edges two pixels apart.  On the gradient layers the first two are all weights 0 (the central
    difference of a period-2 pattern is 0) and the third is the largest horizontal response, 127, in one bin at every pixel"""
    rng = _rng("image/" + name)
    img = rng.integers(0, 256, (h, w)).astype(np.uint8)
    if min(w, h) >= 100:
        r = REGION
        yy, xx = np.mgrid[:r, :r]
        img[2:2 + r, 2:2 + r] = 77
        img[2:2 + r, w - r - 2:w - 2] = np.where((yy + xx) % 2 == 0, 0, 255)
        img[h - r - 2:h - 2, 2:2 + r] = np.where((xx // 2) % 2 == 0, 0, 255)
    return img


STEP_RESPONSE = 127   # the weight of a 0 / 255 step on a FD_LAYER_GRADBIN layer


# name -> (patch w, patch h, cell, block, bins, signed + unsigned, why)
TILE_GEOMETRIES = {
    "20x20-c3-b2-9": (20, 20, 3, 2, 9, False, "C=49: one window per pass (WPW == 1)"),
    "32x32-c4-b1-9": (32, 32, 4, 1, 9, False, "C=64 and 64 blocks: HOG_MAX_CELLS / HOG_MAX_BLOCKS"),
    "20x20-c6-b2-9": (20, 20, 6, 2, 9, False, "C=9: 5 passes of 7, the last one past row 31"),
    "10x10-c10-b1-9": (10, 10, 10, 1, 9, False, "C=1: WPW == 64, F=9 padded to 16"),
    "20x20-c4-b1-9": (20, 20, 4, 1, 9, False, "F=225 padded to 232"),
    "23x17-c5-b2-8-sau": (23, 17, 5, 2, 8, True, "C=15, signed + unsigned"),
    "32x12-c4-b3-9": (32, 12, 4, 3, 9, False, "one block row"),
    "20x20-c5-b2-64": (20, 20, 5, 2, 64, False, "cells * bins == 1024: HOG_MAX_HIST"),
    "20x20-c3-b7-9": (20, 20, 3, 7, 9, False, "C=49 with one block: F = 441, the WPW == 1 shape the MFMA SVM's tile takes"),
}
# name -> (image w, image h, pyramid arguments, step x, step y, why)
TILE_LAUNCHES = {
    "few": (37, 35, dict(octave_layers=1, min_scale=1.0, max_scale=1.0), 4, 4, "fewer than 32 windows"),
    "two-layers": (121, 119, dict(octave_layers=2, min_scale=0.7, max_scale=1.0), 2, 3, "N % 64 != 0 over two layers, step (2, 3)"),
}
TILE_PERSISTENT_FRAG = "20x20-c3-b7-9"   # the same launch through k_hog_tile<true>
TILE_PERSISTENT = ("20x20-c3-b2-9", 150, 150, dict(octave_layers=1, min_scale=1.0, max_scale=1.0), 1, 1)   # more than num_cus * 64 items


def tile_case(geo):
    pw, ph, cell, block, bins, sau, _ = TILE_GEOMETRIES[geo]
    return patch_case(HOG, pw=pw, ph=ph, cell=cell, block=block, bins=bins, sau=sau)


EXTRACT_HIST_IMAGE = ("extract-hist", 121, 119)
EXTRACT_HIST = [   # fd_extract_hist: (layer filter, parameter set); the channels are the layer's; 20 x 20 windows at step (2, 3), two layers
    (dict(kind=1, bins=9), dict(kind=HOG, block=2, interpolate=True)),
    (dict(kind=1, bins=9), dict(kind=PYRAMID_HOG, levels=2)),
    (dict(kind=1, bins=8, signed_gradients=True, interpolate=True), dict(kind=HOG, bins=8, block=2, sau=True)),
    (dict(kind=2, lbp_type=1), dict(kind=SPATIAL, bins=59, normalization=L2HYS)),
    (dict(kind=2, lbp_type=1), dict(kind=SPATIAL, bins=16, block=2, normalization=L1SQRT)),   # uniform codes 16 .. 58: dropped
    (dict(kind=3, lbp_type=1), dict(kind=SPATIAL_PYRAMID, bins=59, levels=2, normalization=L1NORM)),
    (dict(kind=3, lbp_type=0), dict(kind=SPATIAL, bins=64, block=2, concatenate=True, interpolate=True)),   # codes 64 .. 255: dropped
]


def content_windows(f, patches, bins):
    """(windows whose model vector is exactly 0, windows of a gradient layer with the step response at every pixel: one bin, or the two
    opposite ones of signed gradients)"""
    p = patches.reshape(len(patches), -1, patches.shape[-1])
    saturated = (p[..., 1] == STEP_RESPONSE).all(1) & (np.abs(p[..., 0].astype(int) - p[:, :1, 0]) % max(1, bins // 2) == 0).all(1)
    return np.nonzero(~f.any(1))[0], np.nonzero(saturated)[0]


def cut_windows(layers, windows, pw, ph):
    """the windows ({layer position, x, y, ...} rows) out of the layer images"""
    return np.stack([layers[w[0]][w[2]:w[2] + ph, w[1]:w[1] + pw] for w in windows])
