"""k_resize_down with pair slots (the two source rows of a resized row interleaved byte-wise in LDS, read as two 16-bit words) byte for
byte against the CPU oracle, on the frame sizes where the new addressing can go wrong: source widths of every residue mod 4 around one
and two tile columns (a source dword hanging over a slot, tiles whose first source column is not 0), heights where the row below
the last clamps to it and the row above the first clamps to 0, both grid forms (fewer than eight frames / one workgroup set per XCD),
pyramids with scales near 1 and near 0.5, and FD_PYR_FUSED=2, where every resized pixel of the kernel is written and compared."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_resize_down import _compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = lambda v: float(np.float32(v))  # noqa: E731
SIZES = [(w, h) for w in (129, 130, 131, 257) for h in (35, 36, 37, 70)]
PYRAMIDS = {
    "inc095": dict(inc=F32(0.95), min_scale=0.2, max_scale=0.5),      # 13 first-octave layers, scales 0.95 .. 0.525; their pyrDowns kept
    "inc071": dict(inc=F32(0.71), min_scale=0.2, max_scale=0.5),      # one first-octave layer at 0.707
    "bench": dict(inc=F32(0.92), min_scale=F32(0.05), max_scale=F32(0.16)),
    "first_down": dict(inc=F32(0.92), min_scale=0.2, max_scale=0.5),  # the kernel's pyrDown layers are kept layers: compared directly
}


@pytest.mark.parametrize("nframes", [1, 7, 8, 9])
@pytest.mark.parametrize("name", list(PYRAMIDS))
def test_pair_slots_bit_exact(oracle, capi, ctx, synth, name, nframes):
    for (W, H) in SIZES:
        _compare(oracle, capi, ctx, synth, W, H, PYRAMIDS[name], nframes, seed=3000 + 7 * W + H)


FUSED2 = r"""
import sys
sys.path.insert(0, %(root)r)
import torch  # noqa: F401  (before libfd_hip.so, as in conftest.py)
import numpy as np
from featuredetection_amd import capi, synth
from oracle import pyoracle as O
O.lib()
ctx = capi.Context(0)
bad = []
for inc in (0.92, 0.95):
    kw = dict(inc=float(np.float32(inc)), min_scale=0.2, max_scale=1.0)   # every first-octave layer is a kept layer
    for (W, H) in [(131, 37), (257, 70)]:
        for n in (1, 8):
            frames = [synth.make_frame(W, H, seed=170 + W + i) for i in range(n)]
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
                    bad.append((inc, W, H, n, "layer tables"))
                    continue
                for k in range(len(lo)):
                    got = pg.frame_layer(f, k) if n > 1 else pg.layer(k)
                    if not np.array_equal(got, po.layer(k)):
                        bad.append((inc, W, H, n, f, lo[k]))
            po.close()
            pg.close()
ctx.close()
print("BAD", bad)
print("OK" if not bad else "FAIL")
"""


def test_fused_mode_2_every_resized_pixel():
    """FD_PYR_FUSED=2 (read once per process, hence a child process): the kept first-octave layers come out of k_resize_down's LDS
    tile, so every resized pixel is compared, not only what its pyrDown keeps of it."""
    env = dict(os.environ, FD_PYR_FUSED="2")
    r = subprocess.run([sys.executable, "-c", FUSED2 % dict(root=ROOT)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
