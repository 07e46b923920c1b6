"""k_pyrdown_tiled with a frame's tiles on the frame's XCD (multi-frame pyramids whose frame count is a multiple of 8: a 1-D grid,
workgroup b takes tiles of the frames (b & 7) + 8 i) against the (tiles, 1, frames) launch every other frame count keeps and
FD_PYR_XCD=0 selects: every kept layer byte for byte against the CPU oracle and identical both ways.  Frame sizes whose deepest
generation is one tile and whose layer widths fall on either side of a multiple of the 62-column tile; pyramids that keep the
pyrDown generations themselves, and one whose scale-1 layer is the gray image (its chain is not fused into the resize)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = lambda v: float(np.float32(v))  # noqa: E731
PYRAMIDS = {
    "bench": dict(inc=F32(0.92), min_scale=F32(0.05), max_scale=F32(0.16)),   # FaceFrontal.cfg: the bench's pyramid
    "first_down": dict(inc=F32(0.92), min_scale=0.2, max_scale=0.5),          # the first pyrDown generation is kept
    "scale1": dict(inc=F32(0.92), min_scale=0.2, max_scale=1.0),              # the scale-1 chain: pyrDown of the gray image itself
}
SIZES = [(640, 480), (641, 481), (333, 250), (127, 35)]
DISTINCT = 3   # the frames of a call cycle through this many images: the oracle builds each pyramid once
_oracle_layers = {}


def _want(oracle, synth, W, H, name, i):
    key = (W, H, name, i)
    if key not in _oracle_layers:
        po = oracle.Pyramid(**PYRAMIDS[name])
        po.update(synth.make_frame(W, H, seed=300 + W + i))
        _oracle_layers[key] = (po.layers(), [po.layer(k) for k in range(len(po.layers()))])
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


@pytest.mark.parametrize("nframes", [8, 16, 1, 7, 9])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(PYRAMIDS))
def test_pyrdown_layers_bit_exact_on_either_launch(oracle, capi, ctx, synth, monkeypatch, name, size, nframes):
    W, H = size
    frames = [synth.make_frame(W, H, seed=300 + W + f % DISTINCT) for f in range(nframes)]
    monkeypatch.delenv("FD_PYR_XCD", raising=False)
    info, got = _layers_of(capi, ctx, PYRAMIDS[name], frames)
    monkeypatch.setenv("FD_PYR_XCD", "0")
    info0, got0 = _layers_of(capi, ctx, PYRAMIDS[name], frames)
    assert info == info0 and len(info) > 0
    for f in range(nframes):
        lo, want = _want(oracle, synth, W, H, name, f % DISTINCT)
        assert lo == info
        for k in range(len(info)):
            assert np.array_equal(got[f][k], want[k]), (name, size, "frame %d of %d, layer %s" % (f, nframes, info[k]))
            assert np.array_equal(got0[f][k], want[k]), (name, size, "FD_PYR_XCD=0: frame %d of %d, layer %s" % (f, nframes, info[k]))
