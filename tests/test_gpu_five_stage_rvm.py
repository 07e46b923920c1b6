"""fd_detect_five_stage_rvm: FiveStageSlidingWindowDetector with a ProbabilisticRvmClassifier first stage ("firstClassifier prvm") and an
f32 SVM or a second RVM behind it.  Every expected value is composed here from the oracle's own pieces (windows, patch filters, Rvm.eval,
overlap_elimination, Svm.distance, block_nms); each case first asserts, on oracle values alone, that the comparison is well posed: no two
first-stage probabilities closer than 1e-9 (the overlap elimination's order is fixed), no survivor within the f32 tolerance of the second
threshold, and every stage strictly thinner than the one before."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(octave_layers=2, min_scale=0.2, max_scale=0.4)
STEP = 2
OE = (5.0, 0.0)
# name -> (full frame?, pw, ph, feature space, conv_scale, conv_shift): the feature spaces of test_rvm_sliding_window_detector
ROWS = {
    "hq64_20x20": (False, 20, 20, 1, 1.0, 0.0),
    "gray_24x24": (False, 24, 24, 0, 1.0 / 255.0, 0.0),
    "histeq_16x24": (False, 16, 24, 2, 0.5, -3.0),
    "full_hq64_20x20": (True, 20, 20, 1, 1.0, 0.0),
}
# (row, SVM kernel) -> seed of make_svm_f32.  9 wherever its model meets the three conditions above; chosen on the CPU otherwise.
SVM_SEEDS = {("gray_24x24", 2): 13, ("gray_24x24", 0): 20, ("gray_24x24", 1): 18, ("gray_24x24", 3): 10, ("histeq_16x24", 2): 10,
             ("histeq_16x24", 0): 10, ("histeq_16x24", 1): 10, ("histeq_16x24", 3): 10, ("full_hq64_20x20", 2): 10}
# row -> pass_rate of the second RVM make_rvm(21, feats[2::3], ..., n_filters=12), tuned on the CPU until 0 < positives < survivors
RVM2_PASS = {"histeq_16x24": 0.85, "full_hq64_20x20": 0.9}
SVM_CASES = [(r, k) for r in ROWS for k in (2, 0, 1, 3)]

_scenes = {}


def image_of(frame640, full):
    return frame640 if full else np.ascontiguousarray(frame640[:240, :320])


def window_features(oracle, po, pw, ph, space, scale, shift, roi=None):
    """(windows, f32 feature rows) of the oracle pyramid: patch -> feature space -> ConversionFilter(CV_32F, scale, shift)"""
    layers = [po.layer(i) for i in range(len(po.layers()))]
    wins = po.windows(pw, ph, STEP, STEP, roi)
    pat = np.stack([np.ascontiguousarray(layers[lp][ly:ly + ph, lx:lx + pw]) for lp, lx, ly, *_ in wins])
    if space == 1:
        pat = np.stack([oracle.histeq64(p_) for p_ in pat])
    elif space == 2:
        pat = np.stack([oracle.equalize_hist(p_) for p_ in pat])
    feats = pat.reshape(len(pat), -1).astype(np.float32) * np.float32(scale) + np.float32(shift)
    return wins, feats


def scene(oracle, synth, frame640, row):
    """the oracle's first stage on one row of ROWS (cached: the SVM / RVM cases of a row share it)"""
    if row not in _scenes:
        full, pw, ph, space, scale, shift = ROWS[row]
        po = oracle.Pyramid(**KW)
        po.update(image_of(frame640, full))
        wins, feats = window_features(oracle, po, pw, ph, space, scale, shift)
        rvm = synth.make_rvm(3, feats[::3], pw, ph, n_filters=30, kernel=2)
        _scenes[row] = dict(po=po, wins=wins, feats=feats, rvm=rvm)
    return _scenes[row]


def svm_tolerance(m, d):
    """what test_svm_distance_batch grants the f32 distances d of model m"""
    csum = float(np.abs(m["coeff"]).sum())
    scale = csum * (np.abs(d).max() / max(csum, 1e-30) if m["kernel"] in (0, 1, 3) else 1.0)
    return 1e-4 * np.abs(d) + 1e-5 * max(scale, 1.0)


def first_stage(oracle, rvm, wins, feats):
    """positives of the RVM cascade in window order: (window indices, oracle detections with the classifier's probability)"""
    ro = oracle.Rvm(rvm)
    lv, d = ro.eval(feats)
    last = (rvm.get("num_used", 0) or len(rvm["thresholds"])) - 1
    pos = np.nonzero((lv == last) & (d >= rvm["thresholds"][last]))[0]
    dets = np.zeros(len(pos), oracle.DET_DTYPE)
    for q, i in zip(dets, pos):
        q["layer"], q["lx"], q["ly"], q["cx"], q["cy"], q["w"], q["h"] = (int(v) for v in wins[i])
        q["level"], q["positive"], q["fout"], q["prob"] = last, 1, np.float32(d[i]), ro.probability(d[i])
    ro.close()
    return pos, dets, d


def second_stage(oracle, second, rows):
    """(passes, distance, tolerance of the distance against the device, threshold) of the second classifier on f32 rows"""
    if "thresholds" in second:   # an RVM
        r2 = oracle.Rvm(second)
        lv, d = r2.eval(rows)
        r2.close()
        last = (second.get("num_used", 0) or len(second["thresholds"])) - 1
        thr = float(second["thresholds"][last])
        return (lv == last) & (d >= thr), d, 1e-12 * np.abs(d), thr, lv == last
    d = oracle.Svm(second).distance(rows)
    thr = float(second.get("threshold", 0.0))
    return d >= thr, d, svm_tolerance(second, d), thr, np.ones(len(d), bool)


def final_stage(oracle, pos2, img_w, img_h, roi):
    """stages 4-5 on the second stage's positives (all of probability 0.5): the centres that remain, or None where every positive does"""
    if roi is not None or len(pos2) == 0:
        return None
    pmap = np.zeros((img_h, img_w), np.float32)
    for q in pos2:
        if 0 <= q["cx"] < img_w and 0 <= q["cy"] < img_h:
            pmap[q["cy"], q["cx"]] = max(pmap[q["cy"], q["cx"]], np.float32(0.5))
    ys, xs = np.nonzero(oracle.block_nms(pmap, 35, ((pmap > np.float32(0.3)) * 255).astype(np.uint8)))
    if len(xs) == 0:
        ys, xs = np.nonzero(oracle.block_nms(pmap, 35, None))   # FiveStageSlidingWindowDetector.cpp:289-293
    if len(xs) == 0:
        return None                                             # "return svmPatchesPositive": all of them
    return sorted(zip(xs.tolist(), ys.tolist()))


def expected(oracle, rvm, second, wins, feats, img_w, img_h, roi=None):
    pos, dets, d1 = first_stage(oracle, rvm, wins, feats)
    prob = np.sort(dets["prob"])
    assert len(prob) < 2 or np.diff(prob).min() > 1e-9, "two first-stage probabilities within 1e-9: choose another seed"
    keep = oracle.overlap_elimination(dets, *OE)
    passes, d2, tol, thr, reached = second_stage(oracle, second, feats[pos[keep]])
    assert np.all(~reached | (np.abs(d2 - thr) > tol)), "a survivor lies within the tolerance of the second threshold: choose another seed"
    pos2 = dets[keep][passes]
    maxima = final_stage(oracle, pos2, img_w, img_h, roi)
    nfinal = len(pos2) if maxima is None else len(maxima)
    stages = [len(pos), len(keep), int(passes.sum()), nfinal]
    assert len(wins) > stages[0] > stages[1] > stages[2] > 0 and stages[3] > 0, stages
    if roi is None:
        assert stages[2] > stages[3], stages
    return dict(stages=stages, pos2=pos2, dist2=d2[passes], tol2=tol[passes], maxima=maxima, first=dets)


def geometry(q):
    return tuple(int(q[f]) for f in ("layer", "lx", "ly", "cx", "cy", "w", "h"))


def check(dets, stages, exp, roi=None):
    assert stages.tolist() == exp["stages"], (stages.tolist(), exp["stages"])
    want = {geometry(q): (dv, t) for q, dv, t in zip(exp["pos2"], exp["dist2"], exp["tol2"])}
    assert len(want) == len(exp["pos2"])
    assert len(dets) == exp["stages"][3]
    for q in dets:
        assert geometry(q) in want, geometry(q)
        dv, t = want[geometry(q)]
        assert abs(float(q["score"]) - float(np.float32(dv))) <= t + abs(dv) * 2.0 ** -23, (q["score"], dv, t)   # score = (float)distance
        assert q["probability"] == 0.5 and q["positive"] == 1
    got = sorted((int(q["cx"]), int(q["cy"])) for q in dets)
    if exp["maxima"] is not None:
        assert got == exp["maxima"]          # exactly the maxima, each an expected positive with that centre
    else:
        assert sorted(geometry(q) for q in dets) == sorted(want)   # roi (or no maximum at all): every second-stage positive


def make_second_svm(oracle, synth, sc, row, kernel):
    calib = sc["feats"][1::3]
    m = synth.make_svm_f32(SVM_SEEDS.get((row, kernel), 9), calib, nsv=256, gamma=sc["rvm"]["p0"], positive_fraction=0.3, kernel=kernel)
    if kernel == 1:
        # make_svm_f32 leaves the degree at 0, where every kernel value is 1 and all survivors share one distance: a polynomial of degree 2,
        # (gamma x.s + 1)^2, with the bias that makes 30 % of the calibration vectors positive (the rule of make_svm_f32, by the oracle)
        m = dict(m, p1=1.0, p2=2.0, bias=np.float32(0.0))
        m["bias"] = np.float32(np.quantile(oracle.Svm(m).distance(calib), 0.7))
    return m


def make_second_rvm(synth, sc, row):
    _, pw, ph = ROWS[row][:3]
    return synth.make_rvm(21, sc["feats"][2::3], pw, ph, n_filters=12, pass_rate=RVM2_PASS.get(row, 0.8))


def gpu_pyramid(capi, ctx, frame640, row):
    pg = capi.Pyramid(ctx, **KW)
    pg.update(image_of(frame640, ROWS[row][0]))
    return pg


def run(capi, ctx, pg, rg, second, row, **kw):
    _, _, _, space, scale, shift = ROWS[row]
    return capi.detect_five_stage_rvm(ctx, pg, rg, second, feature_space=space, conv_scale=scale, conv_shift=shift, oe_dist=OE[0], oe_ratio=OE[1],
                                      sx=STEP, sy=STEP, **kw)


@pytest.mark.parametrize("row,kernel", SVM_CASES)
def test_svm_second_stage_matches_oracle_composition(oracle, capi, ctx, synth, frame640, row, kernel):
    sc = scene(oracle, synth, frame640, row)
    svm = make_second_svm(oracle, synth, sc, row, kernel)
    exp = expected(oracle, sc["rvm"], svm, sc["wins"], sc["feats"], sc["po"].img_w, sc["po"].img_h)
    pg, rg, sg = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, sc["rvm"]), capi.Svm(ctx, svm)
    dets, stages = run(capi, ctx, pg, rg, sg, row)
    check(dets, stages, exp)
    sg.close(); rg.close(); pg.close()


@pytest.mark.parametrize("row", list(ROWS))
def test_rvm_second_stage_matches_oracle_composition(oracle, capi, ctx, synth, frame640, row):
    sc = scene(oracle, synth, frame640, row)
    r2 = make_second_rvm(synth, sc, row)
    exp = expected(oracle, sc["rvm"], r2, sc["wins"], sc["feats"], sc["po"].img_w, sc["po"].img_h)
    pg, rg, r2g = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, sc["rvm"]), capi.Rvm(ctx, r2)
    dets, stages = run(capi, ctx, pg, rg, r2g, row)
    check(dets, stages, exp)
    r2g.close(); rg.close(); pg.close()


ROI = (60, 40, 200, 150)


@pytest.mark.parametrize("which", ["svm", "rvm"])
def test_roi_variant(oracle, capi, ctx, synth, frame640, which):
    """detect(image, roi) (:331-380): no block NMS, the whole output is the set of second-stage positives"""
    row = "hq64_20x20"
    sc = scene(oracle, synth, frame640, row)
    _, pw, ph, space, scale, shift = ROWS[row]
    wins, feats = window_features(oracle, sc["po"], pw, ph, space, scale, shift, ROI)
    assert 0 < len(wins) < len(sc["wins"])
    second = make_second_svm(oracle, synth, sc, row, 2) if which == "svm" else make_second_rvm(synth, sc, row)
    exp = expected(oracle, sc["rvm"], second, wins, feats, sc["po"].img_w, sc["po"].img_h, roi=ROI)
    assert exp["maxima"] is None and exp["stages"][3] == exp["stages"][2]
    pg, rg = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, sc["rvm"])
    sg = capi.Svm(ctx, second) if which == "svm" else capi.Rvm(ctx, second)
    dets, stages = run(capi, ctx, pg, rg, sg, row, roi=ROI)
    check(dets, stages, exp, roi=ROI)
    assert np.all(np.diff(dets["probability"]) <= 0)
    sg.close(); rg.close(); pg.close()


def test_first_stage_is_detect_rvm(oracle, capi, ctx, synth, frame640):
    """Stage 1 of the new call is fd_detect_rvm on the same pyramid: with a second stage that passes everything and an overlap elimination
    that removes nothing (dist 0: |dx| < 0 never holds), the roi variant returns the first stage's records, every field but score and
    probability equal to fd_detect_rvm's.  Those two are overwritten by stage 3 (the second distance, 0.5); the first stage's probability is
    checked through what it decides: the overlap elimination of the call keeps as many as fd_overlap_elimination keeps of fd_detect_rvm's
    records."""
    row = "hq64_20x20"
    sc = scene(oracle, synth, frame640, row)
    _, pw, ph, space, scale, shift = ROWS[row]
    svm = dict(make_second_svm(oracle, synth, sc, row, 2), threshold=-1e30)
    pg, rg, sg = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, sc["rvm"]), capi.Svm(ctx, svm)
    whole = (0, 0, sc["po"].img_w, sc["po"].img_h)
    ref, _, _ = capi.detect_rvm(ctx, pg, rg, feature_space=space, conv_scale=scale, conv_shift=shift, sx=STEP, sy=STEP, roi=whole, want_all=False)
    ref = ref.copy()
    dets, stages = capi.detect_five_stage_rvm(ctx, pg, rg, sg, feature_space=space, conv_scale=scale, conv_shift=shift, oe_dist=0.0, oe_ratio=0.0, sx=STEP,
                                              sy=STEP, roi=whole)
    assert stages[0] == len(ref) > 50
    assert stages[1] == stages[2] == stages[3] == len(ref) == len(dets)   # nothing eliminated, nothing refused: the records themselves
    key = lambda a: np.lexsort((a["ly"], a["lx"], a["layer"]))
    a, b = ref[key(ref)], dets[key(dets)].copy()
    for f in ("cx", "cy", "w", "h", "layer", "lx", "ly", "level", "positive"):
        assert np.array_equal(a[f], b[f]), f
    # and the count of the first stage under the call's own parameters
    ref2, _, _ = capi.detect_rvm(ctx, pg, rg, feature_space=space, conv_scale=scale, conv_shift=shift, sx=STEP, sy=STEP, want_all=False)
    _, st2 = run(capi, ctx, pg, rg, sg, row)
    assert st2[0] == len(ref2)
    # stage 2 on fd_detect_rvm's records is what the call keeps
    keep = capi.overlap_elimination(ref2, *OE)
    assert st2[1] == len(keep)
    sg.close(); rg.close(); pg.close()


def test_both_orders_return_the_same_bytes(oracle, capi, ctx, synth, frame640, monkeypatch):
    """FD_FS_SPEC=0 (two waits: the SVM on the survivors) against the default (one wait: the SVM on every positive, queued behind the cascade)"""
    for row, kernel in (("hq64_20x20", 2), ("histeq_16x24", 1), ("full_hq64_20x20", 3)):
        sc = scene(oracle, synth, frame640, row)
        svm = make_second_svm(oracle, synth, sc, row, kernel)
        pg, rg, sg = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, sc["rvm"]), capi.Svm(ctx, svm)
        monkeypatch.delenv("FD_FS_SPEC", raising=False)
        d1, s1 = run(capi, ctx, pg, rg, sg, row)
        d1, s1 = d1.copy(), s1.copy()
        monkeypatch.setenv("FD_FS_SPEC", "0")
        d0, s0 = run(capi, ctx, pg, rg, sg, row)
        monkeypatch.delenv("FD_FS_SPEC", raising=False)
        assert s1[2] > 0 and np.array_equal(s0, s1) and d0.tobytes() == d1.tobytes(), row
        sg.close(); rg.close(); pg.close()


def test_image_entry_point_equals_update_and_detect(oracle, capi, ctx, synth, frame640):
    import torch
    row = "hq64_20x20"
    sc = scene(oracle, synth, frame640, row)
    _, pw, ph, space, scale, shift = ROWS[row]
    img = image_of(frame640, False)
    for second_m, mk in ((make_second_svm(oracle, synth, sc, row, 2), capi.Svm), (make_second_rvm(synth, sc, row), capi.Rvm)):
        pg, rg, sg = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, sc["rvm"]), mk(ctx, second_m)
        want, wst = run(capi, ctx, pg, rg, sg, row)
        want, wst = want.copy(), wst.copy()
        assert wst[2] > 0
        p2 = capi.Pyramid(ctx, **KW)
        fi = capi.FiveStageRvmImage(ctx, p2, rg, sg, feature_space=space, conv_scale=scale, conv_shift=shift, oe_dist=OE[0], oe_ratio=OE[1], sx=STEP, sy=STEP)
        got, gst = fi.detect(img)
        assert np.array_equal(gst, wst) and got.tobytes() == want.tobytes()
        p2.update(np.ascontiguousarray(img[::-1]))   # other content in between
        dev = torch.from_numpy(img.copy()).cuda()
        torch.cuda.synchronize()
        got, gst = fi.detect_device(dev.data_ptr(), img.shape[1], img.shape[0], 3)
        assert np.array_equal(gst, wst) and got.tobytes() == want.tobytes()
        p2.close(); sg.close(); rg.close(); pg.close()


def test_greyworld_image_filter(oracle, capi, ctx, synth, frame640):
    """fd_pyramid_set_image_filter holds for the _image entry point: expected values from oracle.Pyramid.update(oracle.greyworld(frame))"""
    row = "hq64_20x20"
    _, pw, ph, space, scale, shift = ROWS[row]
    img = np.clip(np.rint(image_of(frame640, False).astype(np.float64) * np.array((0.55, 0.8, 1.0))), 0, 255).astype(np.uint8)
    po = oracle.Pyramid(**KW)
    po.update(oracle.greyworld(img))
    plain = oracle.Pyramid(**KW)
    plain.update(img)
    assert any(not np.array_equal(po.layer(i), plain.layer(i)) for i in range(len(po.layers())))
    wins, feats = window_features(oracle, po, pw, ph, space, scale, shift)
    rvm = synth.make_rvm(3, feats[::3], pw, ph, n_filters=30, kernel=2)
    svm = synth.make_svm_f32(GREYWORLD_SVM_SEED, feats[1::3], nsv=256, gamma=rvm["p0"], positive_fraction=0.3, kernel=2)
    exp = expected(oracle, rvm, svm, wins, feats, po.img_w, po.img_h)
    pg, rg, sg = capi.Pyramid(ctx, **KW), capi.Rvm(ctx, rvm), capi.Svm(ctx, svm)
    pg.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
    fi = capi.FiveStageRvmImage(ctx, pg, rg, sg, feature_space=space, conv_scale=scale, conv_shift=shift, oe_dist=OE[0], oe_ratio=OE[1], sx=STEP, sy=STEP)
    dets, stages = fi.detect(img)
    check(dets, stages, exp)
    sg.close(); rg.close(); pg.close(); po.close(); plain.close()


GREYWORLD_SVM_SEED = 9


def test_more_positives_than_the_speculative_capacity(oracle, capi, ctx, synth, frame640, monkeypatch):
    """An RVM cut to its first level passes most windows: more positives than the one-wait order's launches cover, so the call takes the
    two-wait order on its own, and the result is the oracle composition's."""
    row = "full_hq64_20x20"
    sc = scene(oracle, synth, frame640, row)
    # seeds chosen on the CPU: with seed 3 two of the 6706 positives of the first level share one probability, and the overlap
    # elimination's order would be the sort's; seed 9 leaves 4.9e-9 between the closest two, SVM seed 30 a margin of 1.5 tolerances
    rvm = dict(synth.make_rvm(9, sc["feats"][::3], 20, 20, n_filters=30, kernel=2), num_used=1)
    svm = synth.make_svm_f32(30, sc["feats"][1::3], nsv=256, gamma=rvm["p0"], positive_fraction=0.3, kernel=2)
    exp = expected(oracle, rvm, svm, sc["wins"], sc["feats"], sc["po"].img_w, sc["po"].img_h)
    assert exp["stages"][0] > 4096
    pg, rg, sg = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, rvm), capi.Svm(ctx, svm)
    monkeypatch.delenv("FD_FS_SPEC", raising=False)
    dets, stages = run(capi, ctx, pg, rg, sg, row)
    dets, stages = dets.copy(), stages.copy()
    check(dets, stages, exp)
    monkeypatch.setenv("FD_FS_SPEC", "0")
    d0, s0 = run(capi, ctx, pg, rg, sg, row)
    assert np.array_equal(s0, stages) and d0.tobytes() == dets.tobytes()
    sg.close(); rg.close(); pg.close()


def test_refusals_leave_the_handles_usable(oracle, capi, ctx, synth, frame640):
    import ctypes as C
    row = "hq64_20x20"
    sc = scene(oracle, synth, frame640, row)
    _, pw, ph, space, scale, shift = ROWS[row]
    svm = make_second_svm(oracle, synth, sc, row, 2)
    exp = expected(oracle, sc["rvm"], svm, sc["wins"], sc["feats"], sc["po"].img_w, sc["po"].img_h)
    pg, rg, sg = gpu_pyramid(capi, ctx, frame640, row), capi.Rvm(ctx, sc["rvm"]), capi.Svm(ctx, svm)
    r2 = capi.Rvm(ctx, make_second_rvm(synth, sc, row))
    rng = np.random.default_rng(2)
    u8 = capi.Svm(ctx, synth.make_svm_u8(4, rng.integers(0, 256, (80, pw * ph), dtype=np.uint8), nsv=64))
    other_dim = capi.Svm(ctx, synth.make_svm_f32(5, rng.random((300, 24 * 24)).astype(np.float32), nsv=32, positive_fraction=0.3))
    other_size = capi.Rvm(ctx, synth.make_rvm(6, rng.random((300, 24 * 24)).astype(np.float32), 24, 24, n_filters=4))
    multi = capi.Pyramid(ctx, **KW)
    multi.set_frames(2)
    img = image_of(frame640, False)
    multi.update_frames(images=[img, img])
    filtered = capi.Pyramid(ctx, **KW)
    filtered.set_layer_filter(capi.FD_LAYER_GRADBIN, bins=9)
    filtered.update(img)
    dp = capi.fd_rvm_detect_params(space, scale, shift, STEP, STEP)
    out = np.zeros(4096, capi.DET_DTYPE)
    cnt, st = C.c_int(), np.zeros(4, np.int32)

    def raw(p, first, s, r):
        return capi.lib().fd_detect_five_stage_rvm(ctx.h, p.h, first.h, C.byref(dp), s.h if s else None, r.h if r else None, OE[0], OE[1], None,
                                                   out.ctypes.data_as(C.c_void_p), len(out), C.byref(cnt), st.ctypes.data_as(C.c_void_p))

    refused = [("both second classifiers", (pg, rg, sg, r2)), ("no second classifier", (pg, rg, None, None)), ("u8 SVM", (pg, rg, u8, None)),
               ("SVM of another dimension", (pg, rg, other_dim, None)), ("RVM of another filter size", (pg, rg, None, other_size)),
               ("the first handle as second", (pg, rg, None, rg)), ("multi-frame pyramid", (multi, rg, sg, None)),
               ("layer-filtered pyramid", (filtered, rg, sg, None))]
    for what, args in refused:
        assert raw(*args) == capi.FD_ERR_INVALID_ARGUMENT == 1, what
        dets, stages = run(capi, ctx, pg, rg, sg, row)   # the next valid call gives the expected result
        check(dets, stages, exp)
    # the _image entry point refuses before it touches the pyramid
    before = [pg.layer(i) for i in range(len(pg.layers()))]
    other = np.ascontiguousarray(img[::-1])
    rc = capi.lib().fd_detect_five_stage_rvm_image(ctx.h, pg.h, rg.h, C.byref(dp), u8.h, None, other.ctypes.data_as(C.c_void_p), other.shape[1], other.shape[0], 3, 0,
                                                   OE[0], OE[1], None, out.ctypes.data_as(C.c_void_p), len(out), C.byref(cnt), st.ctypes.data_as(C.c_void_p))
    assert rc == capi.FD_ERR_INVALID_ARGUMENT
    assert all(np.array_equal(a, pg.layer(i)) for i, a in enumerate(before))
    with pytest.raises(TypeError):
        capi.detect_five_stage_rvm(ctx, pg, rg, object())
    for h in (u8, other_dim, other_size, r2, sg, rg, multi, filtered, pg):
        h.close()
