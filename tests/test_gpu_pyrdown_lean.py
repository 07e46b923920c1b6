"""k_pyrdown_tiled with host-built tile entries, scalar row offsets and one load + byte permute per staged dword: every kept layer
byte for byte against the CPU oracle.  The pyramids of the first two tests keep every generation of the scale-1 chain, which is
the gray image itself and goes through k_pyrdown_tiled only: widths on either side of one and two 62-column tiles and of every
residue mod 4 (where a row's last dword ends), layers narrower than 8 pixels (the byte gather), heights on either side of one and
two 16-row tiles; then several frames on either launch (a frame's tiles on its XCD, or the (tiles, 1, frames) grid), and two
pyramids whose first pyrDown runs inside k_resize_down with the same column arithmetic."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = lambda v: float(np.float32(v))  # noqa: E731
CHAIN = dict(octave_layers=1, min_scale=1 / 64, max_scale=1.0)             # 1, 1/2, ..., 1/64: pyrDown after pyrDown of the gray image
BENCH = dict(inc=F32(0.92), min_scale=F32(0.05), max_scale=F32(0.16))      # FaceFrontal.cfg: the bench's pyramid
FIRST_DOWN = dict(inc=F32(0.92), min_scale=0.2, max_scale=0.5)             # keeps the generation k_resize_down makes
WIDTHS = [8, 9, 10, 11, 123, 124, 125, 126, 127, 247, 248, 249, 250, 251]
HEIGHTS = [3, 4, 5, 31, 32, 33, 34, 63, 65]
DISTINCT = 3   # the frames of a call cycle through this many images: the oracle builds each pyramid once
_oracle_layers = {}


def _gray(W, H, i):
    return np.random.default_rng(1000 * W + 10 * H + i).integers(0, 256, (H, W), dtype=np.uint8)


def _want(oracle, kw, image, key):
    if key not in _oracle_layers:
        po = oracle.Pyramid(**kw)
        try:
            po.update(image)
            _oracle_layers[key] = (po.layers(), [po.layer(k) for k in range(len(po.layers()))])
        finally:
            po.close()
    return _oracle_layers[key]


def _layers_of(capi, ctx, kw, frames):
    n = len(frames)
    pg = capi.Pyramid(ctx, **kw)
    try:
        if n > 1:
            pg.set_frames(n)
            pg.update_frames(images=frames)
        else:
            pg.update(frames[0])
        info = pg.layers()
        return info, [[pg.frame_layer(f, k) if n > 1 else pg.layer(k) for k in range(len(info))] for f in range(n)]
    finally:
        pg.close()


def _assert_chain(oracle, capi, ctx, W, H):
    image = _gray(W, H, 0)
    lo, want = _want(oracle, CHAIN, image, ("chain", W, H, 0))
    info, got = _layers_of(capi, ctx, CHAIN, [image])
    assert info == lo and len(info) >= 2, (W, H, info)   # the gray image and at least one pyrDown of it
    for k in range(len(info)):
        assert np.array_equal(got[0][k], want[k]), ("%dx%d" % (W, H), info[k])


@pytest.mark.parametrize("W", WIDTHS)
def test_chain_widths(oracle, capi, ctx, W):
    _assert_chain(oracle, capi, ctx, W, 35)


@pytest.mark.parametrize("H", HEIGHTS)
def test_chain_heights(oracle, capi, ctx, H):
    _assert_chain(oracle, capi, ctx, 125, H)


@pytest.mark.parametrize("nframes", [8, 16, 9])
@pytest.mark.parametrize("size", [(125, 35), (250, 65)], ids=lambda s: "%dx%d" % s)
def test_chain_frames_on_either_launch(oracle, capi, ctx, monkeypatch, size, nframes):
    W, H = size
    frames = [_gray(W, H, f % DISTINCT) for f in range(nframes)]
    monkeypatch.delenv("FD_PYR_XCD", raising=False)
    info, got = _layers_of(capi, ctx, CHAIN, frames)
    monkeypatch.setenv("FD_PYR_XCD", "0")
    info0, got0 = _layers_of(capi, ctx, CHAIN, frames)
    assert info == info0 and len(info) >= 2
    for f in range(nframes):
        lo, want = _want(oracle, CHAIN, frames[f], ("chain", W, H, f % DISTINCT))
        assert lo == info
        for k in range(len(info)):
            assert np.array_equal(got[f][k], want[k]), (size, "frame %d of %d, layer %s" % (f, nframes, info[k]))
            assert np.array_equal(got0[f][k], want[k]), (size, "FD_PYR_XCD=0: frame %d of %d, layer %s" % (f, nframes, info[k]))
            assert np.array_equal(got[f][k], got0[f][k])


@pytest.mark.parametrize("name,kw,size", [("bench", BENCH, (640, 480)), ("first_down", FIRST_DOWN, (333, 250))])
def test_eight_frames_behind_the_fused_resize(oracle, capi, ctx, synth, name, kw, size):
    W, H = size
    frames = [synth.make_frame(W, H, seed=500 + W + f % DISTINCT) for f in range(8)]
    info, got = _layers_of(capi, ctx, kw, frames)
    assert len(info) > 0
    for f in range(8):
        lo, want = _want(oracle, kw, frames[f], (name, W, H, f % DISTINCT))
        assert lo == info
        for k in range(len(info)):
            assert np.array_equal(got[f][k], want[k]), (name, "frame %d, layer %s" % (f, info[k]))
