"""k_wvm_prefilter on the packed plan (a wavefront's 64 tasks span layers; balanced row groups; layer fields per lane) against the
CPU oracle and against the per-layer plan (FD_WVD_PACK=0, read per call): fd_detect_wvm positives -- window, level, fp32 output --
and five-stage results bit for bit, the same number of windows queued for stage B either way.  Shapes: layers with fewer than 64
tasks (one wavefront over three and more layers), layers of one row / one column of windows, fewer rows than K, window steps 2 and
12 (K = 1), a roi, a call just above the dense path's 512 windows, 1 / 7 / 8 / 9 frames, a 24x24 model, K pinned to 1 and to 16."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = lambda v: float(np.float32(v))  # noqa: E731
FF = dict(inc=F32(0.92), min_scale=F32(0.05), max_scale=F32(0.16))   # FaceFrontal.cfg: the bench's pyramid
WIDE = dict(inc=F32(0.9), min_scale=0.16, max_scale=0.5)
# name: (W, H, pyramid, sx, sy, roi).  Windows per layer (nx, ny), from the oracle's enumeration:
CASES = {
    "small_layers": (400, 300, FF, 1, 1, None),              # (39, 25) ... (15, 7), (12, 4), (10, 2): the last three share a wavefront
    "one_row": (430, 125, WIDE, 1, 1, None),                 # twelve layers down to (60, 3), (52, 1)
    "one_column": (125, 430, WIDE, 1, 1, None),              # ... (3, 60), (1, 52)
    "step2": (400, 300, FF, 2, 2, None),                     # (20, 13) ... (6, 2), (5, 1)
    "step12_rows": (430, 125, WIDE, 1, 12, None),            # 2 sy > ph: K = 1; (195, 4) ... (52, 1)
    "roi": (400, 300, FF, 1, 1, (20, 10, 360, 280)),
    "just_dense": (276, 207, FF, 1, 1, None),                # 525 windows (the dense path starts at 512): (21, 11) ... (9, 2)
}
FIELDS = (("layer", "layer"), ("lx", "lx"), ("ly", "ly"), ("level", "level"), ("positive", "positive"))


def _both_plans(monkeypatch, run):
    monkeypatch.delenv("FD_WVD_PACK", raising=False)
    a = run()
    monkeypatch.setenv("FD_WVD_PACK", "0")
    b = run()
    monkeypatch.delenv("FD_WVD_PACK")
    return a, b


def _check_wvm(oracle, capi, ctx, monkeypatch, frame, kw, model, sx, sy, roi):
    pg = capi.Pyramid(ctx, **kw)
    pg.update(frame)
    wg = capi.Wvm(ctx, model)
    n = pg.window_count(model["filter_w"], model["filter_h"], sx, sy, roi)
    assert n >= 512, "the call must take the dense path"

    def run():
        det, _, _ = capi.detect_wvm(ctx, pg, wg, sx, sy, roi=roi, want_all=False, cap=1 << 16)
        return det.copy(), wg.last_queue_length()
    (dp, qp), (dl, ql) = _both_plans(monkeypatch, run)
    assert dp.tobytes() == dl.tobytes()
    assert qp == ql and qp >= 0
    po = oracle.Pyramid(**kw)
    po.update(frame)
    do, _, _ = oracle.sliding_wvm(po, oracle.Wvm(model), sx, sy, roi, want_all=False)
    assert len(dp) == len(do)
    for fg, fo in FIELDS:
        assert np.array_equal(dp[fg], do[fo]), fg
    assert np.array_equal(dp["score"].view(np.uint32), do["fout"].view(np.uint32))
    po.close(); wg.close(); pg.close()
    return n, len(dp), qp


@pytest.mark.parametrize("name", list(CASES))
def test_positives_bit_exact_on_either_plan(oracle, capi, ctx, synth, small_models, monkeypatch, name):
    W, H, kw, sx, sy, roi = CASES[name]
    n, npos, q = _check_wvm(oracle, capi, ctx, monkeypatch, synth.make_frame(W, H, seed=4100 + W), kw, small_models[0], sx, sy, roi)
    print("%s: %d windows, %d queued for stage B, %d positives" % (name, n, q, npos))
    if name == "just_dense":
        assert n < 640
    if name in ("small_layers", "one_row", "one_column"):
        assert npos > 0 and q > 0


def test_patch_24x24(oracle, capi, ctx, synth, frame640, monkeypatch):
    gray = oracle.bgr2gray(frame640)
    calib = synth.random_patches(gray[::4, ::4].copy(), 24, 24, 3000, np.random.default_rng(5))
    model = synth.make_wvm(17, fw=24, fh=24, n_per=5, n_levels=4, calib_patches=calib, min_survivors=48)
    n, npos, q = _check_wvm(oracle, capi, ctx, monkeypatch, synth.make_frame(400, 300, seed=4243), FF, model, 1, 1, None)
    assert npos > 0 and q > 0


_oracle_frames = {}


@pytest.mark.parametrize("nframes", [1, 7, 8, 9])
def test_five_stage_frames_on_either_plan(oracle, capi, ctx, synth, small_models, monkeypatch, nframes):
    """1 frame: fd_detect_five_stage; 7: one round-robin launch; 8: one frame per XCD; 9: the XCD split and its remainder"""
    wvm, svm = small_models
    W, H = 400, 300
    frames = [synth.make_frame(W, H, seed=4300 + f % 3) for f in range(nframes)]
    pg = capi.Pyramid(ctx, **FF)
    if nframes > 1:
        pg.set_frames(nframes)
        pg.update_frames(images=frames)
    else:
        pg.update(frames[0])
    wg, sg = capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)

    def run():
        res = capi.detect_five_stage_frames(ctx, pg, wg, sg, nframes) if nframes > 1 else [capi.detect_five_stage(ctx, pg, wg, sg)]
        return [(d.copy(), s.copy()) for d, s in res], wg.last_queue_length()
    (rp, qp), (rl, ql) = _both_plans(monkeypatch, run)
    assert qp == ql and qp > 0
    wo, so = oracle.Wvm(wvm), oracle.Svm(svm)
    total = 0
    for f in range(nframes):
        assert rp[f][0].tobytes() == rl[f][0].tobytes() and np.array_equal(rp[f][1], rl[f][1]), f
        if f % 3 not in _oracle_frames:
            po = oracle.Pyramid(**FF)
            po.update(frames[f])
            _oracle_frames[f % 3] = oracle.five_stage(po, wo, so)
            po.close()
        do, sto = _oracle_frames[f % 3]
        dg, stg = rp[f]
        assert np.array_equal(stg, sto), (f, stg, sto)
        for fld in ("cx", "cy", "w", "h", "layer", "lx", "ly"):   # the windows; a detection's score is the SVM's distance (tolerance, not bits)
            assert np.array_equal(dg[fld], do[fld]), (f, fld)
        total += int(stg[0])
    assert total > 0
    wg.close(); sg.close(); pg.close()


def test_model_chosen_walk_of_several_windows(oracle, capi, ctx, synth, small_models, monkeypatch):
    """32 frames of 640x480 are 8096 wavefronts at K = 1 for the 3072 wavefront slots of an MI355X (256 CUs x 3 workgroups x 4), so
    the cost model itself picks K = 3 (88 wavefronts per frame): balanced row groups, the histogram slide and lanes of several steps
    on the packed plan without FD_WVD_K, against the oracle and the per-layer plan."""
    wvm, svm = small_models
    NF = 32
    frames = [synth.make_frame(640, 480, seed=4400 + f % 3) for f in range(NF)]
    po = oracle.Pyramid(**FF)
    po.update(frames[0])
    w = po.windows(20, 20, 1, 1)
    nx = [len(np.unique(w[w[:, 0] == l, 1])) for l in np.unique(w[:, 0])]
    ny = [len(np.unique(w[w[:, 0] == l, 2])) for l in np.unique(w[:, 0])]
    if "FD_WVD_K" not in os.environ:
        assert capi.wvd_packed_plan(nx, ny, NF, 1, 20, 3072, tasks=[])[0] > 1
    pg = capi.Pyramid(ctx, **FF)
    pg.set_frames(NF)
    pg.update_frames(images=frames)
    wg, sg = capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)

    def run():
        return [(d.copy(), st.copy()) for d, st in capi.detect_five_stage_frames(ctx, pg, wg, sg, NF)], wg.last_queue_length()
    (rp, qp), (rl, ql) = _both_plans(monkeypatch, run)
    assert qp == ql and qp > 0
    wo, so = oracle.Wvm(wvm), oracle.Svm(svm)
    want = []
    for i in range(3):
        po.update(frames[i])
        want.append(oracle.five_stage(po, wo, so))
    po.close()
    for f in range(NF):
        assert rp[f][0].tobytes() == rl[f][0].tobytes() and np.array_equal(rp[f][1], rl[f][1]), f
        do, sto = want[f % 3]
        dg, stg = rp[f]
        assert np.array_equal(stg, sto), (f, stg, sto)
        for fld in ("cx", "cy", "w", "h", "layer", "lx", "ly"):
            assert np.array_equal(dg[fld], do[fld]), (f, fld)
    assert sum(int(st[0]) for _, st in want) > 0
    wg.close(); sg.close(); pg.close()


@pytest.mark.parametrize("k", [1, 16])
def test_pinned_k(k):
    """FD_WVD_K is read once per process: the tests above in a child process with K pinned -- 16 makes every small layer a single
    row group (ny < K) and cuts the layers of 17 .. 31 rows into two balanced ones"""
    env = dict(os.environ, FD_WVD_K=str(k))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_gpu_prefilter_packed.py", "-k", "not pinned"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
