"""fd_flow on the device against the numpy model (tests/optflow_model.py): the stored levels and derivatives, the
tracked points, status flags and traces, bit for bit -- the build keeps division and square root correctly rounded and contraction
off, and the window sums are integers."""
import numpy as np
import pytest

import optflow_model as M

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_levels(flow, pyramid, previous=False):
    assert flow.levels == len(pyramid)
    for l, want in enumerate(pyramid):
        img, der = flow.level(l, previous=previous)
        assert img.shape == want["img"].shape and np.array_equal(img, want["img"]), "level %d" % l
        assert np.array_equal(der, want["der"]), "derivatives of level %d" % l


@pytest.mark.parametrize("width,height,win_w,win_h,max_level,levels", [(33, 17, 5, 7, 2, 2), (64, 48, 15, 15, 2, 2), (64, 48, 15, 15, 0, 1),
                                                                        (160, 128, 31, 31, 4, 3), (9, 7, 3, 3, 3, 2), (7, 5, 3, 3, 3, 1)])
def test_pyramid_equals_the_model(capi, ctx, width, height, win_w, win_h, max_level, levels):
    img = M.textured(width, height, seed=width)
    flow = capi.Flow(ctx, width, height, win_w=win_w, win_h=win_h, max_level=max_level)
    assert flow.levels == levels
    flow.update(img)
    _check_levels(flow, M.build_pyramid(img, win_w, win_h, max_level))
    flow.close()


def test_bgr_on_the_host_and_gray_on_the_device(capi, ctx, synth):
    import torch
    bgr = synth.make_frame(160, 128, seed=3)
    gray = M.bgr2gray(bgr)
    want = M.build_pyramid(gray, 15, 15, 2)
    a = capi.Flow(ctx, 160, 128)
    a.update(bgr)
    _check_levels(a, want)
    b = capi.Flow(ctx, 160, 128)
    dev = torch.from_numpy(gray).to("cuda:0")
    torch.cuda.synchronize()
    b.update(dev)
    _check_levels(b, want)
    wide = torch.zeros((128, 200), dtype=torch.uint8, device="cuda:0")   # rows 200 bytes apart
    wide[:, :160] = dev
    torch.cuda.synchronize()
    b.update(wide[:, :160])
    _check_levels(b, want)
    devbgr = torch.from_numpy(bgr).to("cuda:0")
    torch.cuda.synchronize()
    b.update(devbgr)
    _check_levels(b, want)
    a.close()
    b.close()


def test_the_current_frame_becomes_the_previous_one(capi, ctx):
    prev, cur = M.frame_pair("zoom")
    flow = capi.Flow(ctx, M.WIDTH, M.HEIGHT)
    flow.update(prev)
    flow.update(cur)
    _check_levels(flow, M.build_pyramid(cur, 15, 15, 2))
    _check_levels(flow, M.build_pyramid(prev, 15, 15, 2), previous=True)
    third = M.textured(seed=99)
    flow.update(third)
    _check_levels(flow, M.build_pyramid(third, 15, 15, 2))
    _check_levels(flow, M.build_pyramid(cur, 15, 15, 2), previous=True)
    flow.close()


@pytest.fixture(scope="module")
def flows(capi, ctx):
    """one fd_flow per (frame pair, window, max_level) of the cases, both frames given"""
    made = {}

    def get(kind, win_w, win_h, max_level, max_count):
        key = (kind, win_w, win_h, max_level, max_count)
        if key not in made:
            prev, cur = M.frame_pair(kind)
            f = capi.Flow(ctx, M.WIDTH, M.HEIGHT, win_w=win_w, win_h=win_h, max_level=max_level, max_count=max_count)
            f.update(prev)
            f.update(cur)
            made[key] = f
        return made[key]
    yield get
    for f in made.values():
        f.close()


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_tracking_equals_the_model(flows, name):
    kind, win_w, win_h, max_level, max_count, backward, points = M.CASES[name]
    want_out, want_status, want_trace = M.reference(name)
    flow = flows(kind, win_w, win_h, max_level, max_count)
    out, status, trace = flow.track(points, backward=backward, trace=True)
    differing = np.flatnonzero((out.view(np.uint32) != want_out.view(np.uint32)).any(axis=1) | (status != want_status))
    assert np.array_equal(trace, want_trace), "traces differ at points %s" % np.flatnonzero((trace != want_trace).any(axis=(1, 2)))[:10]
    assert len(differing) == 0, "points %s: got %s want %s" % (differing[:10], out[differing[:10]], want_out[differing[:10]])
    assert _same_bits(out, want_out) and np.array_equal(status, want_status)
    out2, status2 = flow.track(points, backward=backward)   # without the trace
    assert _same_bits(out2, out) and np.array_equal(status2, status)


def test_cases_hold_what_the_issue_lists():
    sizes = {len(c[6]) for c in M.CASES.values()}
    assert {1, 63, 64, 65, 257} <= sizes
    assert {(c[1], c[2]) for c in M.CASES.values()} >= {(3, 3), (5, 7), (15, 15), (21, 21), (31, 31)}
    assert {c[3] for c in M.CASES.values()} >= {0, 2} and any(c[4] == 2 for c in M.CASES.values()) and any(c[5] for c in M.CASES.values())
    assert {c[0] for c in M.CASES.values()} >= {"roll", "zoom"}
    # windows that hang into the border on each of the four sides, points outside, points on the flat patch: in both pairs
    e = M.EDGE_POINTS
    assert (e[:, 0] < 7).any() and (e[:, 0] > M.WIDTH - 8).any() and (e[:, 1] < 7).any() and (e[:, 1] > M.HEIGHT - 8).any()
    for name in ("roll-15x15-mixed", "zoom-15x15-mixed"):
        pts = M.CASES[name][6]
        _, status, trace = M.reference(name)
        n_out, n_flat = len(M.OUTSIDE_POINTS), len(M.FLAT_POINTS)
        outside = slice(len(pts) - n_flat - n_out, len(pts) - n_flat)
        assert np.array_equal(pts[outside], M.OUTSIDE_POINTS) and not status[outside].any() and (trace[outside, 0, 1] == M.EXIT_SKIP_RANGE).all()
        assert not status[-n_flat:].any() and (trace[-n_flat:, 0, 1] == M.EXIT_SKIP_EIGEN).all()


@pytest.mark.parametrize("name", ["roll-15x15-mixed", "zoom-21x21-n64", "jump-5x7-n64"])
def test_track_fb_is_forward_then_backward(flows, name):
    kind, win_w, win_h, max_level, max_count, _, points = M.CASES[name]
    flow = flows(kind, win_w, win_h, max_level, max_count)
    fwd, fst = flow.track(points)
    bwd, bst = flow.track(fwd, backward=True)
    f2, b2, fs2, bs2 = flow.track_fb(points)
    assert _same_bits(f2, fwd) and _same_bits(b2, bwd) and np.array_equal(fs2, fst) and np.array_equal(bs2, bst)
    if name == "roll-15x15-mixed":   # and the model end to end: the median flow of the grid
        prev, cur = M.pyramids(kind, win_w, win_h, max_level)
        want_fwd, want_fst, _ = M.reference(name)
        want_bwd, want_bst, _ = M.track(cur, prev, want_fwd, win_w, win_h, max_count)
        assert _same_bits(b2, want_bwd) and np.array_equal(bs2, want_bst)


def test_many_points(capi, flows):
    """more points than one round of workgroups: 4096 points, each equal to the same point tracked on its own"""
    flow = flows("zoom", 15, 15, 2, 30)
    base = M.CASES["zoom-15x15-backward-n65"][6][:64]
    points = np.tile(base, (64, 1))
    out, status = flow.track(points)
    one, one_status = flow.track(base)
    assert _same_bits(out, np.tile(one, (64, 1))) and np.array_equal(status, np.tile(one_status, 64))


def test_clean_failures(capi, ctx):
    flow = capi.Flow(ctx, 64, 48)
    pts = np.array([[10.0, 10.0]], np.float32)
    with pytest.raises(capi.FdError) as e:
        flow.track(pts)
    assert e.value.code == 2 and "two frames" in str(e.value)          # FD_ERR_RUNTIME
    flow.update(M.textured(64, 48, seed=1))
    with pytest.raises(capi.FdError):
        flow.track(pts)                                                # one frame is not enough either
    with pytest.raises(capi.FdError):
        flow.track_fb(pts)
    with pytest.raises(capi.FdError):
        flow.level(0, previous=True)
    flow.update(M.textured(64, 48, seed=2))
    out, status = flow.track(pts)
    assert status.shape == (1,)
    with pytest.raises(capi.FdError) as e:
        flow.track(np.zeros((capi.FD_FLOW_MAX_POINTS + 1, 2), np.float32))
    assert e.value.code == 1                                           # FD_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.FdError):
        flow.level(2)                                                  # 16 x 12 was not built
    with pytest.raises(ValueError):
        flow.update(M.textured(65, 48, seed=1))
    out, status = flow.track(np.zeros((0, 2), np.float32))
    assert out.shape == (0, 2)
    flow.close()
    for bad in (dict(win_w=2), dict(win_h=32), dict(win_w=33, win_h=33), dict(max_level=8), dict(max_level=-1)):
        with pytest.raises(capi.FdError) as e:
            capi.Flow(ctx, 64, 48, **bad)
        assert e.value.code == 1, bad
    with pytest.raises(capi.FdError):
        capi.Flow(ctx, 0, 48)
    clamped = capi.Flow(ctx, 64, 48, max_count=1000, epsilon=-1.0)     # clamped as OpenCV clamps them, not refused
    clamped.close()
    ctx.synchronize()
