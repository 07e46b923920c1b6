"""What k_resize_down puts into LDS and where its threads read it, without a GPU: fd_debug_resize_stage stages a tile with the launch
plan's own column table and tile columns and the kernel's own row, fetch, interleave and addressing functions.  The stage is 36 pair
slots of 512 bytes, one per resized row of the tile: the row's two source rows, interleaved byte-wise.  For every resized pixel
that a stored pyrDown output of the tile reads, the four bytes its thread reads (two 16-bit words at an even offset) must be the
source pixels (y0, x), (y1, x), (y0, x + 1), (y1, x + 1) that k_resize_tiled's coordinates name -- on every tile of every fused
first-octave layer, for source widths 64 .. 700 of every residue mod 4 and eleven heights.  The right neighbour of the image's last
column is exempt (its weight is 0; the dword that holds it hangs over the row).  Also the headline's tiles per frame."""
import numpy as np
import pytest

FT_W, FT_H = 62, 16            # pyrDown tile
G0_W, G0_H = 127, 35           # resized pixels under it
SLOT, SLOTS = 512, 36
OCTL = 8                       # layers per octave at inc = 0.92: round(log 0.5 / log 0.92)
WIDTHS = list(range(64, 701, 13))          # 13 = 1 mod 4: every residue, 49 widths
HEIGHTS = [6, 9, 35, 36, 37, 64, 65, 66, 70, 97, 130]


def reflect101(p, n):
    """BORDER_REFLECT_101 from its definition, on an array of coordinates"""
    p = np.asarray(p).copy()
    assert n > 1
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def src_coord(d, scale, n, clamp_like_columns):
    """k_resize_tiled's srcX / srcY: the left / upper source coordinate of destination coordinates d, and the one behind it"""
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)     # double arithmetic, rounded to float
    s = np.floor(f).astype(np.int64)
    if clamp_like_columns:
        s = np.where(s < 0, 0, np.where(s >= n - 1, n - 1, s))
        return s, s + 1                                   # s + 1 == n: the exempt neighbour of the last column
    return np.clip(s, 0, n - 1), np.clip(s + 1, 0, n - 1)


def fused_layers(sw, sh):
    """the first-octave layers below scale 1 of a sw x sh frame (ImagePyramid: cvRound(size * 0.5 ** (i / OCTL)))"""
    out = []
    for i in range(1, OCTL):
        s = 0.5 ** (i / OCTL)
        out.append((int(np.rint(sw * s)), int(np.rint(sh * s))))
    return out


def _check_layer(capi, src, dw0, dh0):
    sh, sw = src.shape
    dw1, dh1 = (dw0 + 1) // 2, (dh0 + 1) // 2
    tiles_x, tiles_y = -(-dw1 // FT_W), -(-dh1 // FT_H)
    assert capi.resize_stage(src, dw0, dh0, None) == tiles_x * tiles_y
    scale_x, scale_y = 1. / (dw0 / sw), 1. / (dh0 / sh)
    for t in range(tiles_x * tiles_y):
        nt, staged, off, e = capi.resize_stage(src, dw0, dh0, t)
        tx, ty = t % tiles_x, t // tiles_x
        assert nt == tiles_x * tiles_y
        assert (e["tx"], e["ty"], e["gx0"], e["gy0"], e["dw1"], e["dh1"]) == (tx, ty, 2 * tx * FT_W - 2, 2 * ty * FT_H - 2, dw1, dh1)
        assert 0 <= e["X0"] and e["X0"] + e["ncol"] <= sw and e["ncol"] <= 256, e
        # a stored output (x, y) of the tile reads resized rows 2 y .. 2 y + 4 and columns 2 x .. 2 x + 4 of the tile
        nx, ny = min(FT_W, dw1 - tx * FT_W), min(FT_H, dh1 - ty * FT_H)
        rows, cols = 2 * (ny - 1) + 5, 2 * (nx - 1) + 5
        assert rows <= G0_H and cols <= G0_W
        gy = reflect101(e["gy0"] + np.arange(rows), dh0)
        gx = reflect101(e["gx0"] + np.arange(cols), dw0)
        y0, y1 = src_coord(gy, scale_y, sh, False)
        x0, x1 = src_coord(gx, scale_x, sw, True)
        o = off[:rows, :cols].astype(np.int64)
        where = "%dx%d -> %dx%d tile %d" % (sw, sh, dw0, dh0, t)
        assert (o % 2 == 0).all() and (o >= 0).all() and (o + 3 < SLOT * SLOTS).all(), where
        assert (o // SLOT == np.arange(rows)[:, None]).all(), where        # the left pair lies in the row's own slot
        flat = staged.reshape(-1)
        last = np.broadcast_to(x1[None, :] >= sw, o.shape)
        x1c = np.minimum(x1, sw - 1)
        for k, (yy, xx, exempt) in enumerate(((y0, x0, None), (y1, x0, None), (y0, x1c, last), (y1, x1c, last))):
            got, want = flat[o + k], src[np.ix_(yy, xx)]
            bad = got != want
            if exempt is not None:
                bad &= ~exempt
            if bad.any():
                r, c = np.argwhere(bad)[0]
                raise AssertionError("%s: tile entry (%d, %d) byte %d at stage offset %d = %d, source (%d, %d) = %d" % (
                    where, r, c, k, o[r, c] + k, got[r, c], yy[r], xx[c], want[r, c]))


@pytest.mark.parametrize("sh", HEIGHTS)
def test_threads_read_the_four_source_pixels(capi, sh):
    rng = np.random.default_rng(8100 + sh)
    assert {w % 4 for w in WIDTHS} == {0, 1, 2, 3}
    for sw in WIDTHS:
        src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        for dw0, dh0 in fused_layers(sw, sh):
            _check_layer(capi, src, dw0, dh0)


def test_hook_rejects_what_is_not_a_tile(capi):
    src = np.zeros((40, 90), np.uint8)
    assert capi.resize_stage(src, 70, 30, None) == 1
    with pytest.raises(capi.FdError):
        capi.resize_stage(src, 70, 30, 1)
    with pytest.raises(capi.FdError):
        capi.resize_stage(src, 70, 30, -1)
    with pytest.raises(capi.FdError):
        capi.resize_stage(src, 40, 30, None)      # scale 2.25: not a first-octave layer
    with pytest.raises(capi.FdError):
        capi.resize_stage(src, 91, 30, None)      # an enlargement


def test_headline_tiles_per_frame(oracle, capi):
    """640x480, inc 0.92: the first-octave layers below scale 1 (sizes from the oracle's pyramid) are the fused layers of the headline
    call -- seven: the scale-1 layer is the gray image itself and its pyrDown stays with k_pyrdown_tiled --, and their 62 x 16 pyrDown
    tiles are the work list of one frame: 70 + 65 + 48 + 44 + 40 + 36 + 27 = 330.  (The kernel's measured LDS instructions per launch,
    11.98 M at 142 per wavefront and tile, are 330 tiles x 64 frames x 4 wavefronts.)"""
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    po = oracle.Pyramid(inc=f32(0.92), min_scale=f32(0.05), max_scale=1.0)
    try:
        po.update(np.zeros((480, 640), np.uint8))
        octl = po.octave_layers
        size = {L["index"]: (L["w"], L["h"]) for L in po.layers()}
    finally:
        po.close()
    assert size[0] == (640, 480) and octl == OCTL
    src = np.zeros((480, 640), np.uint8)
    per_layer = [capi.resize_stage(src, size[i][0], size[i][1], None) for i in range(1, octl)]
    print("tiles per fused layer:", per_layer)
    want = [-(-size[i + octl][0] // FT_W) * -(-size[i + octl][1] // FT_H) for i in range(1, octl)]   # from the oracle's pyrDown layers
    assert per_layer == want
    assert [size[i] for i in range(1, octl)] == fused_layers(640, 480)
    assert sum(per_layer) == 330, per_layer
