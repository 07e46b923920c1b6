"""What k_pyrdown_tiled puts into LDS, without a GPU: fd_debug_pyrdown_stage stages a tile with the kernel's own tile-entry builder
and per-lane staging function (one clamped dword load and one byte permute per row; reflected bytes below 8 columns).  Every staged
byte that a stored output of the tile reads must be the BORDER_REFLECT_101 source pixel, on every tile of every layer width from 1
to 260 and the layer heights on either side of one and two tile rows.  Also the tiles per launch of the headline pyramid, against
the layer sizes of the CPU oracle."""
import numpy as np
import pytest

PD_W, PD_H = 62, 16
WIDTHS = list(range(1, 261))       # 1..7: the byte gather; 8..260: the dword path, up to five tile columns
HEIGHTS = [1, 2, 3, 4, 5, 31, 32, 33, 34, 35, 36]


def reflect101(p, n):
    """BORDER_REFLECT_101 from its definition: gfedcb|abcdefgh|gfedcba"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _check_layer(capi, src):
    sh, sw = src.shape
    dw, dh = (sw + 1) // 2, (sh + 1) // 2
    tiles_x, tiles_y = -(-dw // PD_W), -(-dh // PD_H)
    assert capi.pyrdown_stage(src, None) == tiles_x * tiles_y
    for t in range(tiles_x * tiles_y):
        nt, staged, e = capi.pyrdown_stage(src, t)
        dx0, dy0 = (t % tiles_x) * PD_W, (t // tiles_x) * PD_H
        nx, ny = min(PD_W, dw - dx0), min(PD_H, dh - dy0)
        assert nt == tiles_x * tiles_y
        assert e == dict(src_off=0, dst_off=dy0 * dw + dx0, sw=sw, sh=sh, dx0=dx0, dy0=dy0, nx=nx, ny=ny), (sw, sh, t)
        # a stored output (x, y) of the tile reads staged rows 2 y .. 2 y + 4 and columns 2 x .. 2 x + 4
        rows = [reflect101(2 * dy0 - 2 + r, sh) for r in range(2 * (ny - 1) + 5)]
        cols = [reflect101(2 * dx0 - 2 + c, sw) for c in range(2 * (nx - 1) + 5)]
        want = src[np.ix_(rows, cols)]
        got = staged[:len(rows), :len(cols)]
        if not np.array_equal(got, want):
            r, c = np.argwhere(got != want)[0]
            raise AssertionError("%dx%d tile %d: staged[%d][%d] = %d, source (%d, %d) = %d" % (sw, sh, t, r, c, got[r, c], rows[r], cols[c], want[r, c]))


@pytest.mark.parametrize("sh", HEIGHTS)
def test_staged_tile_is_the_reflected_source(capi, sh):
    rng = np.random.default_rng(7000 + sh)
    for sw in WIDTHS:
        _check_layer(capi, rng.integers(0, 256, (sh, sw), dtype=np.uint8))


def test_hook_rejects_what_is_not_a_tile(capi):
    src = np.zeros((5, 9), np.uint8)
    assert capi.pyrdown_stage(src, None) == 1
    with pytest.raises(capi.FdError):
        capi.pyrdown_stage(src, 1)
    with pytest.raises(capi.FdError):
        capi.pyrdown_stage(src, -1)


def test_headline_tiles_per_launch(oracle, capi):
    """640x480, inc 0.92, scales 0.05 .. 0.16: generation 1 of every chain but the scale-1 chain (the gray image itself) comes out of
    k_resize_down, so the k_pyrdown_tiled launches are {generation 1 of chain 0}, then generation 2, 3, 4 of all chains.  The layer
    sizes are the oracle's, from a pyramid that keeps every layer down to the same smallest scale."""
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    po = oracle.Pyramid(inc=f32(0.92), min_scale=f32(0.05), max_scale=1.0)
    try:
        po.update(np.zeros((480, 640), np.uint8))
        octl = po.octave_layers
        size = {L["index"]: (L["w"], L["h"]) for L in po.layers()}
    finally:
        po.close()
    assert size[0] == (640, 480)
    depth = max(size) // octl
    launches = [[0]] + [[c + (d - 1) * octl for c in range(octl) if c + d * octl in size] for d in range(2, depth + 1)]
    per_launch = []
    for sources in launches:
        n = 0
        for s in sources:
            sw, sh = size[s]
            dw, dh = size[s + octl]                     # the oracle's size of the layer this pyrDown makes
            assert (dw, dh) == ((sw + 1) // 2, (sh + 1) // 2)
            want = -(-dw // PD_W) * -(-dh // PD_H)
            assert capi.pyrdown_stage(np.zeros((sh, sw), np.uint8), None) == want
            n += want
        per_launch.append(n)
    assert len(per_launch) == 4 and all(n > 0 for n in per_launch), per_launch
    print("tiles per launch:", per_launch)
