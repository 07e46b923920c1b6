"""fd_particles_state_examples_pyramid: the selection of tests/test_gpu_particles_examples.py with the chosen samples
resolved to windows of a pyramid on the device (k_particles_examples_windows) and their rows made by the list kernels of the pyramid
families, one configuration per family at the 12 x 20 patch of tests/test_gpu_particles_pyramid.py (two cells by two of 6 x 5 under
2 x 2 blocks: the smallest patch with more than one block position in either direction; the gray-patch kinds also at their smallest
legal patches, 1 x 1 and 2 x 2): cell histograms on a gradient bin image, extended HOG, gray patches and the whi chain.  Every record, valid flag and row is compared
bit for bit with tests/self_learning_model.py and the family's *_extract_samples call on the chosen samples.  The generation is
evaluated and weighed on the device first; the thresholds are weights it made.  In the second form the rows are extracted behind another
chain than the one the generation was evaluated with, and a chosen sample has no window there."""
import numpy as np
import pytest

import condensation_model as cm
from test_gpu_particles_examples import COUNTS, check
from test_gpu_particles_pyramid import ASPECT, LOGISTIC_A, LOGISTIC_B, MAPS, N, scene   # noqa: F401  (scene: the fixture)

pytestmark = pytest.mark.gpu

KINDS = ["hist-hog", "ehog", "patch-GRAY", "patch-WHI"]   # hog, ehog, grayscale, whi


def _weighed(capi, ctx, scene, kind, maps):
    k = scene["kinds"][kind]
    gen = {f: v.copy() for f, v in scene["gen"].items()}
    gen["cluster_id"][:] = 3
    particles = capi.Particles.unbound(ctx, N)
    particles.set(**gen)
    particles.evaluate_pyramid(k["pyr"], k["svm"], ASPECT, maps, **k["kw"])
    particles.weigh_classifier(LOGISTIC_A, LOGISTIC_B, float(np.float32(k["model"]["threshold"])))
    device, valid = particles.get(), particles.trace()[2]
    seen = np.sort(device["weight"][valid == 1])
    unique = np.unique(seen)
    assert 0 < valid.sum() < N and len(unique) >= 3
    high = float(max([u for u in unique[:-1] if (seen > u).sum() >= 12] or [unique[-2]]))
    low = float(min([u for u in unique[1:] if (seen < u).sum() >= 12] or [unique[1]]))
    return k, particles, device, valid, seen, high, low


@pytest.mark.parametrize("kind", KINDS)
def test_rows_of_every_family(capi, ctx, scene, kind):
    k, particles, device, valid, seen, high, low = _weighed(capi, ctx, scene, kind, MAPS["resize"])
    n_high, n_low, n_invalid = int((seen > high).sum()), int((seen < low).sum()), int((valid == 0).sum())
    print("%s: %d valid of %d, %d above %r, %d below %r" % (kind, valid.sum(), N, n_high, high, n_low, low))
    assert n_high > 0 and n_low > 0
    plain = particles.state()
    fake = dict(kinds={kind: k["kw"]})
    for max_count in COUNTS:
        for require_window in (0, 1):
            params = capi.examples_params(high, low, max_count, require_window)
            info, pos, neg, rows = check(capi, particles, fake, device, params, kind, maps=MAPS["resize"], valid=valid, plain=plain, integral=k["pyr"],
                                         extract=k["extract"])
            assert len(pos["index"]) == min(n_high, max_count) and pos["valid"].all() and rows.shape[1] > 0 and rows[:len(pos["index"])].any()
            if require_window:
                assert neg["valid"].all() and len(neg["index"]) == min(n_low, max_count)
            else:
                assert len(neg["index"]) == min(n_invalid + n_low, max_count)
    assert {f: v.tobytes() for f, v in particles.get().items()} == {f: device[f].tobytes() for f in cm.FIELDS}   # the generation is untouched
    particles.close()


@pytest.mark.parametrize("kind", ["hist-hog", "patch-WHI"])
def test_rows_behind_another_chain(capi, ctx, scene, kind):
    """evaluated without a map, extracted behind one that enlarges and moves the samples: windows of other layers, and some have none"""
    k, particles, device, valid, seen, high, low = _weighed(capi, ctx, scene, kind, MAPS["none"])
    chain = [("resize", 1.5, 0.2, 0.2)]
    fake = dict(kinds={kind: k["kw"]})
    flags = []
    for max_count in COUNTS:
        params = capi.examples_params(high, low, max_count, 0)
        info, pos, neg, rows = check(capi, particles, fake, device, params, kind, maps=chain, integral=k["pyr"], extract=k["extract"])
        flags += pos["valid"].tolist() + neg["valid"].tolist()
    print("%s: %d of %d chosen samples have a window behind the other chain" % (kind, sum(flags), len(flags)))
    assert 0 in flags and 1 in flags
    particles.close()


def test_another_patch_size_and_arguments(capi, ctx, scene):
    k, particles, device, valid, seen, high, low = _weighed(capi, ctx, scene, "patch-GRAY", MAPS["resize"])
    params = capi.examples_params(high, low, 10, 0)
    huge = capi.patch_samples_params(32, 32, capi.FD_FEATURE_GRAY, 1.0, 0.0)   # larger than the smallest kept layers, not than the largest
    check(capi, particles, dict(kinds={"p": dict(patch=huge)}), device, params, "p", maps=MAPS["resize"], integral=k["pyr"],
          extract=lambda s: capi.patch_extract_samples(ctx, k["pyr"], huge, s))
    # the smallest patches the gray-patch family takes: 1 x 1 (grayscale), 2 x 2 (the whi chain's frequency grid divides by side - 1)
    for pw, space in ((1, capi.FD_FEATURE_GRAY), (2, capi.FD_FEATURE_WHI)):
        tiny = capi.patch_samples_params(pw, pw, space, 1.0 / 127.5, -1.0)
        _, pos, neg, rows = check(capi, particles, dict(kinds={"p": dict(patch=tiny)}), device, params, "p", maps=MAPS["resize"], integral=k["pyr"],
                                  extract=lambda s, tiny=tiny: capi.patch_extract_samples(ctx, k["pyr"], tiny, s))
        assert rows.shape[1] == pw * pw and len(pos["index"]) + len(neg["index"]) > 0
    length, capacity = capi.particles_examples_bounds(10, **k["kw"])
    assert (length, capacity) == (12 * 20, 20 * 12 * 20)

    def refused(match, code=None, **kw):
        with pytest.raises(capi.FdError) as e:
            particles.state_examples(kw.pop("params", params), kw.pop("pyr", k["pyr"]), ASPECT, kw.pop("maps", MAPS["resize"]), **kw)
        assert e.value.code == (code or capi.FD_ERR_INVALID_ARGUMENT) and match in str(e.value), e.value

    refused("max_count 0", params=capi.examples_params(high, low, 0), **k["kw"])
    refused("max_count 33", params=capi.examples_params(high, low, 33), **k["kw"])
    refused("inf", params=capi.examples_params(float("inf"), low), **k["kw"])
    refused("row_capacity %d" % (capacity - 1), row_capacity=capacity - 1, **k["kw"])
    refused("FD_SAMPLE_MAP_RESIZE", maps=[("integral",)], **k["kw"])
    refused("gray pyramid", pyr=scene["gradbin"], **k["kw"])
    refused("FD_LAYER_GRADBIN", **scene["kinds"]["ehog"]["kw"])   # an extended-HOG extractor on the gray pyramid
    particles.close()
