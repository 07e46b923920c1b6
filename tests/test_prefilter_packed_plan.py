"""The packed plan of k_wvm_prefilter (csrc/wvm.hip: wvd_plan_packed; csrc/wvm_dense.hpp: wvd_packed_task) through its host hook,
fd_debug_wvd_packed_plan: no GPU.  The hook decodes tasks with the function the kernel decodes its lanes with."""
import numpy as np
import pytest

# the kept layers of a 640x480 frame with the FaceFrontal pyramid (inc 0.92, scales 0.05-0.16), as the CPU oracle builds them
FF_LAYERS = [(96, 72), (88, 66), (80, 60), (74, 55), (68, 51), (62, 47), (57, 43), (52, 39), (48, 36), (44, 33), (40, 30), (37, 28), (34, 26)]


@pytest.fixture(scope="module")
def capi():
    from featuredetection_amd import capi as c
    c.lib()
    return c


def _check_cover(nx, ny, k, tiles, ntask, dec):
    """every window of every layer exactly once, rows per task <= K, tiles = ceil(tasks / 64); returns the lane-step utilisation"""
    assert tiles == -(-ntask // 64)
    assert len(dec) == ntask
    li, ix, iy0, rows = dec.T.astype(np.int64)
    assert rows.min() >= 1 and rows.max() <= k
    assert np.all(np.diff(li) >= 0) and li.min() >= 0 and li.max() < len(nx)   # layer-major
    for i in range(len(nx)):
        m = li == i
        g = -(-int(ny[i]) // k)
        assert int(m.sum()) == int(nx[i]) * g, (i, k)
        assert np.all((ix[m] >= 0) & (ix[m] < nx[i]) & (iy0[m] >= 0) & (iy0[m] + rows[m] <= ny[i]))
        assert np.array_equal(ix[m], np.tile(np.arange(int(nx[i])), g))          # group-major, column-minor
        assert rows[m].max() - rows[m].min() <= 1                                 # balanced row groups
        seen = np.zeros((int(ny[i]), int(nx[i])), np.int32)
        for s in range(k):
            ok = m & (s < rows)
            np.add.at(seen, (iy0[ok] + s, ix[ok]), 1)
        assert np.all(seen == 1), i
    steps = np.zeros(tiles * 64, np.int64)
    steps[:ntask] = rows
    return rows.sum() / (64.0 * steps.reshape(tiles, 64).max(axis=1).sum())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_packed_plan_covers_every_window_once(capi, seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        n = int(rng.integers(1, 15))
        nx = rng.integers(1, 401, n).astype(np.int32)
        ny = rng.integers(1, 301, n).astype(np.int32)
        frames = int(rng.choice([1, 1, 8, 64]))
        sy = int(rng.choice([1, 1, 2, 3, 12]))
        ph = int(rng.choice([16, 20, 24]))
        slots = int(rng.choice([256, 3072]))
        k, tiles, ntask, dec = capi.wvd_packed_plan(nx, ny, frames, sy, ph, slots)
        assert 1 <= k <= 16
        if 2 * sy > ph:
            assert k == 1
        _check_cover(nx, ny, k, tiles, ntask, dec)


def test_packed_plan_small_and_degenerate_layers(capi):
    """layers of one column, one row, fewer rows than K, fewer than 64 tasks: a tile spans several layers"""
    nx = np.array([1, 7, 3, 1, 64, 2], np.int32)
    ny = np.array([1, 1, 2, 40, 1, 5], np.int32)
    for frames, slots in ((64, 8), (1, 3072), (64, 1)):
        k, tiles, ntask, dec = capi.wvd_packed_plan(nx, ny, frames, 1, 20, slots)
        _check_cover(nx, ny, k, tiles, ntask, dec)
    k, tiles, ntask, dec = capi.wvd_packed_plan(nx, ny, 1, 1, 20, 3072)
    assert k == 1   # fewer tiles than slots: nothing is walked
    _check_cover(nx, ny, k, tiles, ntask, dec)
    assert len(set(dec[:64, 0].tolist())) >= 3


def _ff_windows():
    """(nx, ny) of every layer from fd_pyramid_windows, or None without a device"""
    try:
        import torch
    except ImportError:
        return None
    if not torch.cuda.is_available():
        return None
    from featuredetection_amd import capi as c
    F = np.float32
    ctx = c.Context(0)
    p = c.Pyramid(ctx, inc=float(F(0.92)), min_scale=float(F(0.05)), max_scale=float(F(0.16)))
    try:
        p.update(np.zeros((480, 640, 3), np.uint8))
        w = p.windows(20, 20, 1, 1)   # rows {layerPos, lx, ly, ...}
        return [(len(np.unique(w[w[:, 0] == l, 1])), len(np.unique(w[w[:, 0] == l, 2]))) for l in np.unique(w[:, 0])]
    finally:
        p.close()
        ctx.close()


def test_packed_plan_facefrontal(capi):
    """The headline: 64 frames of 640x480, 3072 wavefront slots.  Lane-step utilisation (windows / 64 x steps of every tile) of the
    packed plan, worked out on the CPU for these layers: >= 0.946 for every K <= 10 (per-layer plan: 0.92 at K = 3, 0.83 at K = 6)."""
    nxy = _ff_windows()
    if nxy is None:   # no device: the 13 layer sizes
        nxy = [(w - 19, h - 19) for w, h in FF_LAYERS]
    assert len(nxy) == len(FF_LAYERS)
    nx, ny = np.array([a for a, _ in nxy], np.int32), np.array([b for _, b in nxy], np.int32)
    k, tiles, ntask, dec = capi.wvd_packed_plan(nx, ny, 64, 1, 20, 3072)
    util = _check_cover(nx, ny, k, tiles, ntask, dec)
    print("K", k, "tiles per frame", tiles, "utilisation", util)
    assert util >= 0.93
    assert k >= 4
