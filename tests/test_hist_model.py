"""The float64 model of the histogram patch filters (tests/hist_model.py) on every case tests/test_gpu_hist_features.py runs, without a GPU:
the CPU oracle stays inside the bound the kernels are held to and, where the library promises the reference's bits, equals the model's
float32 walk bit for bit; the case table holds every edge the kernels branch on; and subtly wrong kernels, built into the model, leave
the bound by a factor of ten on a named case."""
import numpy as np
import pytest

import hist_model as M
import svm_score_model as S


@pytest.mark.parametrize("name", M.NAMES)
def test_oracle_is_inside_the_bound_of_the_gpu_test(oracle, name):
    """a one-channel image with out-of-range bins is the one input the oracle cannot be given (it indexes with the raw byte, as the
    reference does); with weights, the out-of-range pixels reach it as weight 0"""
    c = M.case(name)
    f, b = M.reference(name)
    assert f.shape == (len(c.patches), M.geometry(c).F) and np.all(np.isfinite(f)) and np.all(f >= 0) and np.all(b[f > 0] > 0) and np.all(b[f == 0] == 0)
    if c.oracle_patches is None:
        assert c.ch == 1
        return
    fo = M.oracle_features(oracle, c, c.oracle_patches)
    assert fo.shape == f.shape
    ratio, i = M.worst(np.abs(fo - f), b)
    print("%s: max |oracle - model| / bound = %.3g (element %d of %d)" % (name, ratio, i, f.size))
    assert ratio <= 1, (name, i)
    if M.exact(c):
        f32 = M.features32(c, c.patches)
        assert f32.tobytes() == fo.tobytes(), (name, np.abs(f32 - fo).max())


def test_cases_hold_what_the_issue_lists():
    cs = {n: M.case(n) for n in M.NAMES}
    gs = {n: M.geometry(c) for n, c in cs.items()}
    cells = {n: g.rows * g.cols for n, g in gs.items()}
    blocks = {n: g.brows * g.bcols for n, g in gs.items() if hasattr(g, "brows")}
    assert cells["hog-27x27-c3-b1"] == 81 and blocks["hog-27x27-c3-b1"] == 81 and blocks["hog-27x27-c3-b2"] == 64
    assert (gs["hog-23x17-c5-b2"].cols, gs["hog-23x17-c5-b2"].rows) == (5, 3)
    assert gs["hog-10x10-c4"].rows == 2 and gs["hog-14x14-c4"].rows == 4                      # 2.5 and 3.5: half to even
    shapes = {(g.rows, g.cols, c.interpolate) for c, g in zip(cs.values(), gs.values())}
    for ip in (False, True):
        assert (1, 1, ip) in shapes and any(r == 1 and k > 1 and i == ip for r, k, i in shapes) and any(k == 1 and r > 1 and i == ip for r, k, i in shapes)
    assert any(g.cols > c.pw for c, g in zip(cs.values(), gs.values()))                        # more cells than pixels along one side
    assert (3, 20, 1) in {(c.pw, c.ph, c.cell) for c in cs.values()}
    # the host table builder's empty range: an interpolating grid with a cell no pixel names
    c = cs["pyrhog-3x20-l5-interp"]
    assert set(range(16)) - {i for e in M._axis(c.pw, 16, True) for i, _ in e}
    assert {(64, 64), (64, 5), (1, 64)} <= {(c.pw, c.ph) for c in cs.values()}
    assert {1, 59, 256} <= {c.bins for c in cs.values() if c.ch == 1}
    assert {2, 4} <= {c.ch for c in cs.values() if c.bins == 64}
    for kind in (M.PYRAMID_HOG, M.SPATIAL_PYRAMID):
        assert {1, 2, 5} <= {c.levels for c in cs.values() if c.kind == kind}
    g = gs["pyrhog-32x32-l5"]
    assert g.rows * g.cols == 256 and g.hist_count == 341
    assert {2, 3} <= {c.levels for c in cs.values() if c.kind == M.PYRAMID_HOG and c.sau}
    assert {M.HOG, M.SPATIAL} <= {c.kind for c in cs.values() if c.cell_h and c.block_h}                # non-square cells and blocks
    block_form = [c for c in cs.values() if c.kind == M.SPATIAL and (c.block > 1 or c.block_h > 1)]
    wave_form = [c for c in cs.values() if c.kind == M.SPATIAL and c.block == 1 and c.block_h in (0, 1)]
    assert {c.normalization for c in block_form if c.concatenate} == set(range(5)) == {c.normalization for c in block_form if not c.concatenate}
    assert {c.normalization for c in wave_form} == set(range(5))
    assert max(g.F for g in gs.values()) > 64 * 64
    second = cs["launch-second-window"]
    assert len(cs["launch-n1"].patches) == 1 and len(second.patches) == second.grid + 3
    assert all(3 <= len(c.patches) <= 70 for n, c in cs.items() if n not in ("launch-n1", "launch-second-window"))
    c = M.case("launch-second-window", 304)
    assert len(c.patches) == 304 * 32 + 3 and (c.pw, c.ph, c.ch) == (8, 8, 1)
    assert {"zero-weights", "one-bin-255", "oob-bins", "oob-255", "oob-half", "corner-pixel", "alternate-0-255", "both-equal"} <= {c.content for c in cs.values()}
    for c in cs.values():
        px = c.patches.reshape(len(c.patches), c.ph, c.pw, c.ch)
        if c.content == "oob-bins":
            assert (px[..., 0] == c.bins).all()
        if c.content == "oob-255":
            assert (px[..., 0] == 255).all() and c.bins < 255
        if c.content == "oob-half":
            assert 0.4 < (px[..., 0] >= c.bins).mean() < 0.6
        if c.content == "both-equal":
            assert c.ch == 4 and (px[..., 0] == px[..., 2]).all()
        if c.content == "corner-pixel":
            assert (px[..., 1] > 0).sum() == len(px) + 1
    # L2HYS clips, and not everything
    aux = {}
    c = cs["spatial-hys-dominant-bin"]
    f = M.features(c, c.patches, aux=aux)
    assert 0 < aux["clipped"] < f.size // 2
    # the LDS limit, from hist_lds_bytes
    assert M.lds_bytes(cs[M.LDS_ACCEPTED]) <= M.LDS_BUDGET < M.lds_bytes(cs[M.LDS_REFUSED]) and cs[M.LDS_REFUSED].bins == cs[M.LDS_ACCEPTED].bins + 1
    assert all(M.lds_bytes(c) <= M.LDS_BUDGET for n, c in cs.items() if n != M.LDS_REFUSED)
    # k_hog_tile: the lane layouts of the issue
    tg = {n: M.geometry(M.tile_case(n)) for n in M.TILE_GEOMETRIES}
    assert [tg[n].rows * tg[n].cols for n in M.TILE_GEOMETRIES] == [49, 64, 9, 1, 25, 15, 24, 16, 49]
    assert tg["32x32-c4-b1-9"].brows * tg["32x32-c4-b1-9"].bcols == 64 and tg["32x12-c4-b3-9"].brows == 1
    assert (tg["10x10-c10-b1-9"].F, tg["20x20-c4-b1-9"].F) == (9, 225) and 16 * 64 == 1024 == 16 * M.tile_case("20x20-c5-b2-64").bins
    assert -(-32 // (64 // 9)) * (64 // 9) > 32                                                 # C = 9: the fifth pass of 7 runs past row 31


@pytest.mark.parametrize("name", [n for n in M.NAMES if M.CASES[n]["content"] not in M.ZERO_CONTENT])
def test_cases_are_not_mostly_zero(name):
    """No case leaves more than a quarter of its output at exactly 0.  The all-zero contents are exempt (their assertion is exact
    equality), and so are, by name and with the reason, the cases that are sparse by construction: there the opposite is asserted, so
    that the list holds nothing it need not."""
    f, _ = M.reference(name)
    nonzero = float((f > 0).mean())
    if name in M.SPARSE_BY_CONSTRUCTION:
        assert nonzero < 0.75, (name, nonzero)
    else:
        assert nonzero >= 0.75, (name, nonzero)


def test_zero_contents_are_exactly_zero():
    for name in M.NAMES:
        if M.CASES[name]["content"] in M.ZERO_CONTENT:
            assert not M.reference(name)[0].any(), name
    assert set(M.SPARSE_BY_CONSTRUCTION) <= set(M.NAMES)


# the cases every mutant has to show on (each is checked; one that no case catches means a case is missing)
MUTANT_CASES = {
    "cell_end_rounds_up": ["hog-23x17-c5-b2", "hog-14x14-c4", "pyrhog-3x20-l3"],
    "cells_past_64_dropped": ["hog-27x27-c3-b1", "spatial-27x27-c3-b1", "pyrhog-32x32-l5", "spatial-64x64-c5-bins233"],
    "blocks_past_64_dropped": ["hog-27x27-c3-b1", "spatial-30x27-c3-b2"],
    "block_walk_uses_rows_for_cols": ["hog-23x17-c5-b2", "hog-28x20-c5x4-b2x3", "spatial-30x27-c3-b2"],
    "eps_outside_sqrt": ["hog-3x20-c1", "pyrhog-3x20-l3"],
    "unsigned_half_from_signed_energy": ["hog-28x20-c5x4-b2x3", "pyrhog-l2-sau", "pyrhog-l3-sau-ch4-interp"],
    "out_of_range_bin_clamped": ["hog-oob-bins", "hog-oob-255", "spatial-hys-oob-half", "spatial-ch1-oob-half", "spatial-ch1-oob-255"],
    "interp_same_cell_added_once": ["hog-8x8-c8-1cell-interp", "hog-20x5-c5-1row-interp", "hog-5x20-c5-1col-interp", "spatial-1x64-c1x8-interp"],
    "stale_vector_from_previous_window": ["launch-second-window"],
}


@pytest.mark.parametrize("mutant,name", [(m, n) for m in M.MUTANTS for n in MUTANT_CASES[m]])
def test_bound_rejects_a_subtly_wrong_kernel(mutant, name):
    c = M.case(name)
    f, b = M.reference(name)
    fm = M.features(c, c.patches, mutant=mutant)
    ratio, i = M.worst(np.abs(fm - f), b)
    print("%s on %s: %.3g bounds at element %d" % (mutant, name, ratio, i))
    assert ratio >= 10, (mutant, name, ratio)


def test_every_mutant_is_the_identity_where_it_should_be():
    """the mutants are one-line changes: on a case without the edge they change nothing"""
    c = M.case("spatial-b2-norm1")
    f, _ = M.reference("spatial-b2-norm1")
    for mutant in M.MUTANTS:
        assert np.array_equal(M.features(c, c.patches, mutant=mutant), f), mutant
    assert set(MUTANT_CASES) == set(M.MUTANTS)


# ---- k_hog_tile: the cut patches of the oracle's pyramid, the fragment layout ---------------------------------------------------------------------
def tile_inputs(pyramid_cls, geo, launch):
    """(windows, patches) of a k_hog_tile case from a pyramid class with the library's interface (the oracle's here, the library's on
    the GPU)"""
    pw, ph, _, _, bins, sau, _ = M.TILE_GEOMETRIES[geo]
    w, h, kw, sx, sy, _ = M.TILE_LAUNCHES[launch]
    p = pyramid_cls(**kw)
    p.set_layer_filter(1, bins=bins, signed_gradients=sau)
    p.update(M.gray_image(launch, w, h))
    wins = p.windows(pw, ph, sx, sy)
    patches = M.cut_windows([p.layer(i) for i in range(len(p.layers()))], wins, pw, ph)
    p.close()
    return wins, patches


def test_tile_launches_are_the_issue_s(oracle):
    wins, _ = tile_inputs(oracle.Pyramid, "20x20-c6-b2-9", "few")
    assert 0 < len(wins) < 32
    wins, _ = tile_inputs(oracle.Pyramid, "20x20-c6-b2-9", "two-layers")
    assert len(wins) % 64 != 0 and len(set(wins[:, 0])) == 2
    first = int(np.argmax(wins[:, 0] != wins[0, 0]))          # the layer boundary lies inside a pass of 7 windows and inside a 32-row tile
    assert first % 7 != 0 and first % 32 != 0
    geo, w, h, _, sx, sy = M.TILE_PERSISTENT
    assert (w - 19) * (h - 19) > 256 * 16 * 4 and M.geometry(M.tile_case(geo)).rows == 7
    gf = M.geometry(M.tile_case(M.TILE_PERSISTENT_FRAG))
    assert gf.rows * gf.cols == 49 and gf.F == 441 and M.rbf_mfma_fits(gf.F)


@pytest.mark.parametrize("geo", list(M.TILE_GEOMETRIES))
def test_tile_cases_against_the_oracle_and_the_fragment_mutants(oracle, geo):
    c = M.tile_case(geo)
    g = M.geometry(c)
    _, patches = tile_inputs(oracle.Pyramid, geo, "two-layers")
    f, b = M.features(c, patches), M.bound(c, patches)
    fo = M.oracle_features(oracle, c, patches)
    ratio, _ = M.worst(np.abs(fo - f), b)
    assert ratio <= 1 and M.features32(c, patches).tobytes() == fo.tobytes()
    # the image's regions reach the layers: windows that are all weights 0 (flat, checkerboard) and windows at the step response
    zero, saturated = M.content_windows(f, patches, c.bins)
    assert len(zero) >= 2 and len(saturated) >= 1 and not fo[zero].any() and len(zero) + len(saturated) < len(f) // 2, (geo, len(zero), len(saturated))
    if not M.rbf_mfma_fits(g.F):
        assert geo in ("20x20-c3-b2-9", "20x20-c5-b2-64")
        return
    # the seeded RBF model of the GPU test, here on the oracle's features
    m, kv = M.svm_for(geo, fo)
    assert ((kv >= 0.05) & (kv <= 0.95)).mean() >= 0.5, geo
    N = len(fo)
    d = S.distance(m, fo)
    sb = S.bound(m, fo, "mfma")
    buf, xx, KP = M.frag_buffers(fo, g.bw * g.bh * g.real)
    base = M.frag_distance(m, buf, xx, KP)
    assert np.all(np.abs(base[:N] - d) <= 1e-3 * sb)          # the layout, read back, is the plain vector
    zero_row = S.distance(m, np.zeros((1, g.F), np.float32))[0]
    assert np.all(np.abs(base[N:] - zero_row) <= 1e-3 * sb[0])
    for mutant in M.FRAG_MUTANTS:
        if mutant == "pad_elements_not_zero" and g.F % 8 == 0:
            continue
        dm = M.frag_distance(m, *M.frag_buffers(fo, g.bw * g.bh * g.real, mutant))
        # rows past N: no returned distance depends on them; the row that moves is one of the last tile's own
        rows = slice(N, None) if mutant == "rows_past_N_not_zero" else slice(0, N)
        assert N % 32 != 0 and np.max(np.abs(dm - base)[rows]) > sb[0], (geo, mutant)
    assert any(M.geometry(M.tile_case(n)).F % 8 for n in M.TILE_GEOMETRIES)


@pytest.mark.parametrize("case", [i for i, (lf, _) in enumerate(M.EXTRACT_HIST) if lf["kind"] != 3])
def test_extract_hist_image_reaches_the_layers(oracle, case):
    """(the oracle's pyramid has no FD_LAYER_GRADMAG_LBP filter: those layers exist on the device only)
    the windows fd_extract_hist sees: some lie wholly in the flat, the checkerboard and the step-edge region on either layer"""
    lf, kw = M.EXTRACT_HIST[case]
    name, w, h = M.EXTRACT_HIST_IMAGE
    p = oracle.Pyramid(octave_layers=2, min_scale=0.7, max_scale=1.0)
    p.set_layer_filter(**lf)
    p.update(M.gray_image(name, w, h))
    wins = p.windows(20, 20, 2, 3)
    patches = M.cut_windows([p.layer(i) for i in range(len(p.layers()))], wins, 20, 20)
    p.close()
    assert len(set(wins[:, 0])) == 2
    c = M.patch_case(ch=patches.shape[3] if patches.ndim == 4 else 1, **kw)
    f = M.features(c, patches)
    flat = patches.reshape(len(patches), 400, -1)
    if lf["kind"] == 1:
        zero, saturated = M.content_windows(f, flat[..., :2], c.bins)
        assert len(zero) >= 2 and len(saturated) >= 1 and {0, 1} <= set(wins[zero, 0]), (len(zero), len(saturated))
    else:   # LBP codes: a window of one code throughout (all of it in one bin, or all of it dropped)
        one_code = (flat[..., 0] == flat[:, :1, 0]).all(1)
        assert one_code.any() and not one_code.all()
    if not (flat[..., 0::2] >= c.bins).any():
        ratio, _ = M.worst(np.abs(M.oracle_features(oracle, c, patches) - f), M.bound(c, patches))
        assert ratio <= 1
