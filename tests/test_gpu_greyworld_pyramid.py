"""The grey-world image filter inside the pyramid (fd_pyramid_set_image_filter, FD_IMAGE_GREYWORLD_GRAY): the reference chain
GreyWorldNormalizationFilter -> GrayscaleFilter is oracle.Pyramid.update(oracle.greyworld(frame)).  Every comparison is bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FF = dict(inc=float(np.float32(0.92)), min_scale=float(np.float32(0.05)), max_scale=float(np.float32(0.16)))  # FaceFrontal.cfg
KINDS = ("plain", "cast", "sat")
# the six pairs of test_pyramid_layers_bit_exact and two tiny frames; 1283x721 and 97x131 have w*h % 4 == 3 (the tail)
CASES = [((640, 480), FF), ((640, 480), dict(octave_layers=5, min_scale=1 / 16, max_scale=1.0)),
         ((321, 243), dict(octave_layers=3, min_scale=0.1, max_scale=0.8)),
         ((1283, 721), dict(octave_layers=4, min_scale=0.05, max_scale=0.6)),
         ((97, 131), dict(octave_layers=6, min_scale=0.2, max_scale=1.0)),
         ((1920, 1080), dict(inc=float(np.float32(0.9)), min_scale=float(np.float32(0.09)), max_scale=float(np.float32(0.25)))),
         ((13, 9), dict(octave_layers=3, min_scale=0.06, max_scale=1.0)),
         ((2, 2), dict(octave_layers=1, min_scale=0.03, max_scale=1.0))]


def variant(frame, kind):
    """plain: as is; cast: channel gains 0.55, 0.8, 1.0 on B, G, R; sat: red gain 1.9, clipped to 255 (a saturated channel)"""
    if kind == "plain":
        return frame
    gains = {"cast": (0.55, 0.8, 1.0), "sat": (1.0, 1.0, 1.9)}[kind]
    return np.clip(np.rint(frame.astype(np.float64) * np.array(gains)), 0, 255).astype(np.uint8)


def oracle_chain(oracle, frame, layer_filter=None, **kw):
    po = oracle.Pyramid(**kw)
    if layer_filter:
        po.set_layer_filter(**layer_filter)
    po.update(oracle.greyworld(frame))
    return po


def assert_same_layers(pg, po, what):
    lo, lg = po.layers(), pg.layers()
    assert lo == lg and len(lo) > 0, what
    for i in range(len(lo)):
        assert np.array_equal(pg.layer(i), po.layer(i)), (what, "layer %d" % i)


def differs(pa, pb):
    return any(not np.array_equal(pa.layer(i), pb.layer(i)) for i in range(len(pa.layers())))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size,kw", CASES)
def test_greyworld_pyramid_layers_bit_exact(oracle, capi, ctx, synth, size, kw, kind):
    import torch
    frame = variant(synth.make_frame(size[0], size[1], seed=size[0]), kind)
    assert all(frame[..., c].any() for c in range(3))   # the reference arithmetic is defined
    po = oracle_chain(oracle, frame, **kw)
    plain = oracle.Pyramid(**kw)
    plain.update(frame)
    assert differs(po, plain), "the filter changes nothing here: the comparison would not see a build that ignores it"
    pg = capi.Pyramid(ctx, **kw)
    assert pg.image_filter == capi.IMAGE_GRAY
    pg.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
    assert pg.image_filter == capi.IMAGE_GREYWORLD_GRAY
    pg.update(frame)
    assert_same_layers(pg, po, "host image")
    # the same frame at a device address that is not 4-byte aligned, behind an update with other content
    pg.update(np.ascontiguousarray(frame[::-1]))
    n = frame.size
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    buf[1:1 + n].copy_(torch.from_numpy(frame.reshape(-1)))
    torch.cuda.synchronize()
    assert (buf.data_ptr() + 1) % 4 != 0
    pg.update_device(buf.data_ptr() + 1, size[0], size[1], 3)
    assert_same_layers(pg, po, "unaligned device image")
    pg.close(); po.close(); plain.close()


def test_greyworld_under_a_layer_filter(oracle, capi, ctx, frame640):
    kw = dict(octave_layers=3, min_scale=0.2, max_scale=1.0)
    po = oracle_chain(oracle, frame640, layer_filter=dict(kind=1, bins=9), **kw)
    plain = oracle.Pyramid(**kw)
    plain.set_layer_filter(kind=1, bins=9)
    plain.update(frame640)
    assert differs(po, plain)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_layer_filter(kind=1, bins=9)
    pg.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
    pg.update(frame640)
    assert_same_layers(pg, po, "bin images")
    pg.close(); po.close(); plain.close()


def test_greyworld_set_and_reset(oracle, capi, ctx, synth, frame640):
    a, b = variant(synth.make_frame(640, 480, seed=77), "sat"), variant(frame640, "cast")
    pg = capi.Pyramid(ctx, **FF)
    pg.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
    pg.update(a)
    pg.update(b)   # the statistics of a are gone
    po = oracle_chain(oracle, b, **FF)
    assert_same_layers(pg, po, "second update")
    # an image of one channel and an unknown kind are refused, and the pyramid goes on working
    with pytest.raises(capi.FdError) as e:
        pg.update(oracle.bgr2gray(b))
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT == 1
    with pytest.raises(capi.FdError) as e:
        pg.set_image_filter(7)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    assert pg.image_filter == capi.IMAGE_GREYWORLD_GRAY
    assert_same_layers(pg, po, "after the refused calls")
    pg.update(b)
    assert_same_layers(pg, po, "update after the refused calls")
    # back to the plain chain
    pg.set_image_filter(capi.IMAGE_GRAY)
    assert pg.image_filter == capi.IMAGE_GRAY
    pg.update(b)
    plain = oracle.Pyramid(**FF)
    plain.update(b)
    assert differs(plain, po)
    assert_same_layers(pg, plain, "filter off")
    pg.update(oracle.bgr2gray(b))   # gray input is accepted again
    assert_same_layers(pg, plain, "gray input, filter off")
    pg.close(); po.close(); plain.close()


@pytest.mark.parametrize("n", [3, 64])
def test_greyworld_multi_frame_own_statistics(oracle, capi, ctx, synth, n):
    """every frame of a multi-frame pyramid is normalised with its own sums and maxima: different content and different casts"""
    import torch
    base = [synth.make_frame(640, 480, seed=500 + k) for k in range(5)]
    frames = [variant(base[f % 5], KINDS[f % 3]) for f in range(n)]   # 15 different frames, neighbours never alike
    pm = capi.Pyramid(ctx, **FF)
    pm.set_frames(n)
    pm.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
    pm.update_frames(images=frames)
    want = {}
    for f in range(n):
        key = (f % 5, f % 3)
        if key not in want:
            po = oracle_chain(oracle, frames[f], **FF)
            want[key] = [po.layer(i) for i in range(len(po.layers()))]
            assert po.layers() == pm.layers()
            po.close()
    for f in range(n):
        for i, lay in enumerate(want[(f % 5, f % 3)]):
            assert np.array_equal(pm.frame_layer(f, i), lay), (f, i)
    # device-resident frames, in another order
    order = list(range(n))[::-1]
    dev = [torch.from_numpy(frames[f]).cuda() for f in order]
    pm.update_frames(device_ptrs=[t.data_ptr() for t in dev], w=640, h=480, ch=3)
    for slot, f in enumerate(order):
        for i, lay in enumerate(want[(f % 5, f % 3)]):
            assert np.array_equal(pm.frame_layer(slot, i), lay), (slot, f, i)
    with pytest.raises(capi.FdError) as e:   # one channel is refused here too
        pm.update_frames(images=[oracle.bgr2gray(fr) for fr in frames])
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT
    pm.close()


def _same_detections(dg, stg, do, sto, what):
    assert np.array_equal(stg, sto), (what, stg, sto)
    for f in ("cx", "cy", "w", "h", "layer", "lx", "ly", "level"):
        assert np.array_equal(dg[f], do[f]), (what, f)
    print(what, "max |score - fout| =", float(np.abs(dg["score"] - do["fout"]).max()) if len(do) else 0.0)
    assert np.array_equal(dg["probability"], do["prob"]), what
    assert np.array_equal(dg["score"], do["fout"]), what


def test_greyworld_detection_every_entry_point(oracle, capi, ctx, synth, frame640, small_models):
    import torch
    wvm, svm = small_models
    wo, so = oracle.Wvm(wvm), oracle.Svm(svm)
    frames = [frame640, variant(frame640, "sat"), variant(synth.make_frame(640, 480, seed=31), "cast")]
    exp = []
    for fr in frames:
        po = oracle_chain(oracle, fr, **FF)
        exp.append(oracle.five_stage(po, wo, so, 5.0, 0.0, 1, 1, None))
        po.close()
    plain = oracle.Pyramid(**FF)
    plain.update(frame640)
    _, st_plain = oracle.five_stage(plain, wo, so, 5.0, 0.0, 1, 1, None)
    plain.close()
    assert not np.array_equal(st_plain, exp[0][1]), "grey-world does not change this frame's stage counts"
    assert all(len(d) > 0 for d, _ in exp) and st_plain[3] > 0

    def pyramid():
        p = capi.Pyramid(ctx, **FF)
        p.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
        return p

    sets = [(pyramid(), capi.Wvm(ctx, wvm), capi.Svm(ctx, svm)) for _ in frames]
    pg, wg, sg = sets[0]
    # fd_pyramid_update + fd_detect_five_stage
    pg.update(frames[0])
    _same_detections(*capi.detect_five_stage(ctx, pg, wg, sg), *exp[0], "detect_five_stage")
    # fd_detect_five_stage_image, host and device image
    one = capi.FiveStageImage(ctx, pg, wg, sg)
    dev = [torch.from_numpy(fr).cuda() for fr in frames]
    for k, fr in enumerate(frames):
        _same_detections(*one.detect(fr), *exp[k], "FiveStageImage.detect %d" % k)
    _same_detections(*one.detect_device(dev[1].data_ptr(), 640, 480, 3), *exp[1], "FiveStageImage.detect_device")
    # the multi-frame call, in one piece and in two halves
    pm = pyramid()
    pm.set_frames(len(frames))
    pm.update_frames(images=frames)
    for k, (d, st) in enumerate(capi.detect_five_stage_frames(ctx, pm, wg, sg, len(frames), cap=4096)):
        _same_detections(d, st, *exp[k], "detect_five_stage_frames %d" % k)
    pm.update_frames(device_ptrs=[t.data_ptr() for t in dev[::-1]], w=640, h=480, ch=3)
    for k, (d, st) in enumerate(capi.FiveStageFrames(ctx, pm, wg, sg, len(frames), cap=4096).end()):
        _same_detections(d, st, *exp[len(frames) - 1 - k], "FiveStageFrames %d" % k)
    pm.close()
    # batch jobs that update their own pyramids: host frames, device frames, in one piece and in two halves
    dfr = [(t.data_ptr(), 640, 480, 3) for t in dev]
    for what, res in (("batch, host frames", capi.detect_five_stage_batch(ctx, sets, host_frames=frames)),
                      ("batch, device frames", capi.detect_five_stage_batch(ctx, sets, device_frames=dfr)),
                      ("FiveStageBatch, host frames", capi.FiveStageBatch(ctx, sets, host_frames=frames[::-1]).end()[::-1]),
                      ("FiveStageBatch, device frames", capi.FiveStageBatch(ctx, sets, device_frames=dfr).end())):
        for k, (d, st) in enumerate(res):
            _same_detections(d, st, *exp[k], "%s %d" % (what, k))
    for p_, w_, s_ in sets:
        w_.close(); s_.close(); p_.close()


def test_greyworld_channel_that_is_zero_everywhere(capi, ctx, synth):
    """The reference divides by a zero mean and rounds a NaN here, which is undefined: the condition is that the update succeeds and
    gives what a plain pyramid gives for the stand-alone filter's output (fd_greyworld)."""
    frame = synth.make_frame(97, 131, seed=3).copy()
    frame[..., 1] = 0
    kw = dict(octave_layers=3, min_scale=0.2, max_scale=1.0)
    pg = capi.Pyramid(ctx, **kw)
    pg.set_image_filter(capi.IMAGE_GREYWORLD_GRAY)
    pg.update(frame)
    plain = capi.Pyramid(ctx, **kw)
    plain.update(ctx.greyworld(frame))
    assert pg.layers() == plain.layers() and len(pg.layers()) > 0
    for i in range(len(pg.layers())):
        assert np.array_equal(pg.layer(i), plain.layer(i)), i
    pg.close(); plain.close()
