"""The host side of a pyramid update, byte for byte against the CPU oracle, where it can go wrong without any kernel being wrong:
launches that split because a stage has more than 16 jobs (18 layers per octave: 17 resize + pyrDown chains, 17 plain resizes,
18 pyrDowns per generation, 60 filtered layers), and one handle whose settings change between updates of the same frame size, so
that everything derived from the layout has to be derived again.  127x35 is the smallest frame that still has fused chains, reflects
at both tile edges and ends inside a dword."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H = 127, 35
CHAINS = dict(octave_layers=18, min_scale=0.1, max_scale=0.5)   # first-octave layers not kept: 17 chains through k_resize_down
KEPT = dict(octave_layers=18, min_scale=0.1, max_scale=1.0)     # first-octave layers kept: 17 through k_resize_tiled
GRADBIN = dict(kind=1, bins=9)


def _oracle_pyramid(oracle, kw, layer_filter):
    po = oracle.Pyramid(**kw)
    if layer_filter:
        po.set_layer_filter(**layer_filter)
    return po


def _assert_frames(oracle, pg, kw, frames, what, layer_filter=None, nlayers=None):
    """every layer of every frame held by pg against a fresh oracle pyramid with the same settings"""
    po = _oracle_pyramid(oracle, kw, layer_filter)
    try:
        for f, frame in enumerate(frames):
            po.update(frame)
            lo, lg = po.layers(), pg.layers()
            assert lo == lg and len(lo) > 0, what
            assert nlayers is None or len(lo) == nlayers, (what, len(lo))
            for k in range(len(lo)):
                got = pg.frame_layer(f, k) if len(frames) > 1 else pg.layer(k)
                assert np.array_equal(got, po.layer(k)), (what, "frame %d of %d, layer %s" % (f, len(frames), lo[k]))
    finally:
        po.close()


@pytest.mark.parametrize("nframes", [1, 8])
def test_seventeen_fused_chains_two_launches(oracle, capi, ctx, synth, nframes):
    """17 chains of k_resize_down (two launches, two tile lists) and 18 layers in pyrDown generation 2 (two launches)"""
    frames = [synth.make_frame(W, H, seed=300 + i) for i in range(nframes)]
    pg = capi.Pyramid(ctx, **CHAINS)
    try:
        if nframes > 1:
            pg.set_frames(nframes)
            pg.update_frames(images=frames)
        else:
            pg.update(frames[0])
        _assert_frames(oracle, pg, CHAINS, frames, "%d frames" % nframes, nlayers=42)
    finally:
        pg.close()


@pytest.mark.parametrize("layer_filter", [None, dict(GRADBIN, blur_kernel=3)], ids=["plain", "gradbin_blur"])
def test_seventeen_kept_resizes_sixty_layers(oracle, capi, ctx, synth, layer_filter):
    """17 kept first-octave layers (two k_resize_tiled launches) and 60 kept layers (four blur and four gradbin launches)"""
    frame = synth.make_frame(W, H, seed=320)
    pg = capi.Pyramid(ctx, **KEPT)
    try:
        if layer_filter:
            pg.set_layer_filter(**layer_filter)
        pg.update(frame)
        _assert_frames(oracle, pg, KEPT, [frame], "kept", layer_filter=layer_filter, nlayers=60)
    finally:
        pg.close()


def test_one_handle_reconfigured_between_updates(oracle, capi, ctx, synth):
    """the frame size never changes: only the setters can tell the pyramid that its layout and launches are out of date"""
    frames = [synth.make_frame(W, H, seed=340 + i) for i in range(16)]   # other content at every step: nothing stale can pass
    pg = capi.Pyramid(ctx, **CHAINS)
    try:
        pg.update(frames[0])
        _assert_frames(oracle, pg, CHAINS, frames[:1], "BGR update")
        pg.set_frames(8)
        pg.update_frames(images=frames[1:9])
        _assert_frames(oracle, pg, CHAINS, frames[1:9], "8 frames")
        pg.set_frames(1)
        gray = oracle.bgr2gray(frames[9])
        pg.update(gray)
        _assert_frames(oracle, pg, CHAINS, [gray], "1-channel image")
        steps = [("gradbin", GRADBIN), ("gradbin + blur", dict(GRADBIN, blur_kernel=3)), ("lbp", dict(kind=2)), ("no filter", dict(kind=0))]
        for i, (what, lf) in enumerate(steps):
            pg.set_layer_filter(**lf)
            pg.update(frames[10 + i])
            _assert_frames(oracle, pg, CHAINS, [frames[10 + i]], what, layer_filter=lf)
        # grey-world in front of the gray conversion (the oracle's chain: its grey-world output fed to its pyramid), and back
        bgr = frames[14]
        assert all(bgr[..., c].any() for c in range(3))   # the reference arithmetic is defined
        pg.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
        pg.update(bgr)
        _assert_frames(oracle, pg, CHAINS, [oracle.greyworld(bgr)], "grey-world")
        pg.set_image_filter(capi.IMAGE_GRAY)
        pg.update(frames[15])
        _assert_frames(oracle, pg, CHAINS, [frames[15]], "back to gray")
    finally:
        pg.close()
