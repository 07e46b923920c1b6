"""k_resize_down (cv::resize of the frame + the first cv::pyrDown of the result in one kernel) byte for byte against the CPU oracle:
multi-frame calls (one workgroup per XCD and frame from eight frames on), the bench's pyramid, pyramids whose first pyrDown layers
are kept (so they are compared directly), FD_PYR_FUSED=2 (every first-octave layer fused AND written), and frame sizes whose
resized widths end inside a dword and whose tiles reflect at the layer's edges."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = lambda v: float(np.float32(v))  # noqa: E731
BENCH = dict(inc=F32(0.92), min_scale=F32(0.05), max_scale=F32(0.16))   # FaceFrontal.cfg: the bench's pyramid
FIRST_DOWN = dict(inc=F32(0.92), min_scale=0.2, max_scale=0.5)          # first-octave layers not kept, their pyrDowns kept
ODD_SIZES = [(641, 481), (333, 250), (127, 35)]


def _compare(oracle, capi, ctx, synth, W, H, kw, nframes, seed):
    frames = [synth.make_frame(W, H, seed=seed + i) for i in range(nframes)]
    pg = capi.Pyramid(ctx, **kw)
    try:
        if nframes > 1:
            pg.set_frames(nframes)
            pg.update_frames(images=frames)
        else:
            pg.update(frames[0])
        po = oracle.Pyramid(**kw)
        for f, frame in enumerate(frames):
            po.update(frame)
            lo, lg = po.layers(), pg.layers()
            assert lo == lg
            for k in range(len(lo)):
                got = pg.frame_layer(f, k) if nframes > 1 else pg.layer(k)
                assert np.array_equal(got, po.layer(k)), (W, H, kw, "frame %d of %d, layer %s" % (f, nframes, lo[k]))
        po.close()
    finally:
        pg.close()


@pytest.mark.parametrize("nframes", [1, 7, 8, 64])
@pytest.mark.parametrize("kw", [BENCH, FIRST_DOWN], ids=["bench", "first_down"])
def test_multi_frame_calls_bit_exact(oracle, capi, ctx, synth, kw, nframes):
    _compare(oracle, capi, ctx, synth, 640, 480, kw, nframes, seed=900)


@pytest.mark.parametrize("size", ODD_SIZES)
@pytest.mark.parametrize("nframes", [1, 8])
@pytest.mark.parametrize("kw", [BENCH, FIRST_DOWN], ids=["bench", "first_down"])
def test_odd_frame_sizes_bit_exact(oracle, capi, ctx, synth, kw, nframes, size):
    _compare(oracle, capi, ctx, synth, size[0], size[1], kw, nframes, seed=40 + size[0])


FUSED2 = r"""
import sys
sys.path.insert(0, %(root)r)
import torch  # noqa: F401  (before libfd_hip.so, as in conftest.py)
import numpy as np
from featuredetection_amd import capi, synth
from oracle import pyoracle as O
O.lib()
ctx = capi.Context(0)
kw = dict(inc=float(np.float32(0.92)), min_scale=0.2, max_scale=1.0)   # every first-octave layer is a kept layer
bad = []
for (W, H) in [(640, 480), (641, 481), (333, 250), (127, 35)]:
    for n in (1, 8):
        frames = [synth.make_frame(W, H, seed=70 + W + i) for i in range(n)]
        pg = capi.Pyramid(ctx, **kw)
        if n > 1:
            pg.set_frames(n)
            pg.update_frames(images=frames)
        else:
            pg.update(frames[0])
        po = O.Pyramid(**kw)
        for f in range(n):
            po.update(frames[f])
            lo = po.layers()
            if lo != pg.layers():
                bad.append((W, H, n, "layer tables"))
                continue
            for k in range(len(lo)):
                got = pg.frame_layer(f, k) if n > 1 else pg.layer(k)
                if not np.array_equal(got, po.layer(k)):
                    bad.append((W, H, n, f, lo[k]))
        po.close()
        pg.close()
ctx.close()
print("BAD", bad)
print("OK" if not bad else "FAIL")
"""


def test_fused_mode_2_writes_first_octave_layers_bit_exact():
    """FD_PYR_FUSED=2 (read once per process, hence a child process): the kept first-octave layers are resized by k_resize_down too and
    written from its LDS tile, so every resized pixel of the kernel is compared, not only what its pyrDown keeps of it."""
    env = dict(os.environ, FD_PYR_FUSED="2")
    r = subprocess.run([sys.executable, "-c", FUSED2 % dict(root=ROOT)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
