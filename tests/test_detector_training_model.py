"""tests/detector_training_model.py on hand-computed cases: the box -> layer / cell / bounds rule of
AggregatedFeaturesExtractor::extract(Rect), Annotations, adjustSize, mirroring, the overlap test and the order in which hard
negatives are accepted."""
import math

import numpy as np

import detector_training_model as T

# a 160 x 120 image, cell 8, window 4 x 4 cells (32 pixels), two layers per octave: layer 0 is the image (20 x 15 cells), layer 1
# is 113 x 85 pixels (cvRound(160 / sqrt 2), cvRound(120 / sqrt 2)), 14 x 10 cells
LAYERS = [dict(index=0, rows=15, cols=20, scale_x=1.0, scale_y=1.0),
          dict(index=1, rows=10, cols=14, scale_x=113.0 / 160.0, scale_y=85.0 / 120.0)]
W = dict(window_w=4, window_h=4, cell=8, octave_layers=2)


def _resolve(box):
    return T.resolve(box, LAYERS, **W)


def test_round_is_half_away_from_zero():
    assert [T.cround(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 0.49999, -0.49999, 45.31)] == [1, 2, 3, -1, -2, 0, 0, 45]


def test_layer_of_a_box_width():
    # the window's own width is layer 0; 45 pixels: log(32 / 45) / log(2^-1/2) = 0.98 -> 1
    assert T.layer_index(32, 4, 8, 2) == 0 and T.layer_index(45, 4, 8, 2) == 1 and T.layer_index(64, 4, 8, 2) == 2
    # between layers 0 and 1 the power is 1/2 at the width 32 * 2^(1/4) = 38.05...: 38 is below (0.4959 -> 0), 39 above (0.5708 -> 1).
    # (A power of exactly k + 1/2 would need 32 / width = 2^(-(2k+1)/4), which no integer width gives; the tie rule itself is
    # test_round_is_half_away_from_zero's.)
    assert abs(math.log(32 / 38) / math.log(2 ** -0.5) - 0.4959) < 1e-4 and T.layer_index(38, 4, 8, 2) == 0
    assert abs(math.log(32 / 39) / math.log(2 ** -0.5) - 0.5708) < 1e-4 and T.layer_index(39, 4, 8, 2) == 1
    # below layer 0 the index is negative: 16 pixels -> -2; 27 -> log(32/27)/log(inc) = -0.49 -> 0; 26 -> -0.599 -> -1
    assert T.layer_index(16, 4, 8, 2) == -2 and T.layer_index(27, 4, 8, 2) == 0 and T.layer_index(26, 4, 8, 2) == -1


def test_box_that_is_exactly_a_window():
    assert _resolve((16, 8, 32, 32)) == (0, 2, 1)   # centre (32, 24) -> cell (4, 3) -> first cell (2, 1)
    assert T.bounds_in_image(2, 1, LAYERS[0], 4, 4, 8) == (16, 8, 32, 32)
    # layer 1: centre (32.5, 32.5) -> (32.5 * 0.70625 / 8, 32.5 * 0.70833 / 8) = (2.87, 2.88) -> cell (2, 2) -> first cell (0, 0);
    # bounds: 32 / 0.70625 = 45.31 -> 45, 32 / 0.70833 = 45.18 -> 45
    assert _resolve((10, 10, 45, 45)) == (1, 0, 0)
    assert T.bounds_in_image(0, 0, LAYERS[1], 4, 4, 8) == (0, 0, 45, 45)
    assert T.bounds_in_image(3, 2, LAYERS[1], 4, 4, 8) == (34, 23, 45, 45)   # 24 / 0.70625 = 33.98, 16 / 0.70833 = 22.59


def test_centre_on_a_cell_edge_truncates():
    assert _resolve((16, 8, 32, 32))[1] == 2          # centre x = 32.0 = 4 * 8: cell 4
    assert _resolve((15, 8, 33, 32))[1] == 1          # centre x = 31.5: cell 3
    assert _resolve((16, 7, 32, 33))[2] == 0          # centre y = 23.5: cell 2
    assert _resolve((16, 8, 32, 31))[2] == 0          # the centre is x + 0.5 w in double: 8 + 15.5 = 23.5


def test_window_leaving_the_layer_by_one_cell():
    assert _resolve((0, 0, 32, 32)) == (0, 0, 0)       # centre (16, 16): the first position
    assert _resolve((-4, 0, 32, 32)) is None           # centre x = 12: cell 1, first cell -1
    assert _resolve((0, -4, 32, 32)) is None
    assert _resolve((132, 92, 32, 32)) == (0, 16, 11)  # the last column and row position: 16 + 4 = 20 cols, 11 + 4 = 15 rows
    assert _resolve((140, 92, 32, 32)) is None         # centre x = 156: cell 19, 17 + 4 = 21 > 20
    assert _resolve((132, 100, 32, 32)) is None        # centre y = 116: cell 14, 12 + 4 = 16 > 15


def test_layers_outside_the_pyramid_and_degenerate_widths():
    assert _resolve((60, 40, 16, 16)) is None and _resolve((0, 0, 64, 64)) is None   # indices -2 and 2
    assert _resolve((10, 10, 0, 5)) is None and _resolve((10, 10, -3, 5)) is None


def test_extract_copies_the_window():
    feats = [np.arange(15 * 20 * 3, dtype=np.float32).reshape(15, 20, 3), np.zeros((10, 14, 3), np.float32)]
    data, bounds = T.extract((16, 8, 32, 32), LAYERS, feats, **W)
    assert np.array_equal(data, feats[0][1:5, 2:6]) and bounds == (16, 8, 32, 32)
    data[:] = -1
    assert feats[0].min() == 0    # a copy
    assert T.extract((140, 92, 32, 32), LAYERS, feats, **W) is None


def test_annotations():
    lms = [T.landmark("face", 50, 40, 20, 30), T.landmark("ignore-blur", 100.5, 60.5, 11, 10), T.landmark_from_rect("ignored", 3, 4, 5, 6),
           T.landmark("tiny", 10, 10, 4, 4), T.landmark("wide", 30, 30, 40, 4)]
    a = T.annotations(lms, min_size=(8, 8))
    # corners rounded half away from zero: 50 -+ 10 and 40 -+ 15; 100.5 - 5.5 = 95, 60.5 - 5 = 55.5 -> 56, 106, 65.5 -> 66
    assert a["non_negatives"] == [(40, 25, 20, 30), (95, 56, 11, 10), (3, 4, 5, 6), (8, 8, 4, 4), (10, 28, 40, 4)]
    assert a["positives"] == [(40, 25, 20, 30), (10, 28, 40, 4)]          # too small means both sides below the minimum
    assert a["fuzzies"] == [(95, 56, 11, 10), (3, 4, 5, 6), (8, 8, 4, 4)]
    assert T.annotations(lms)["fuzzies"] == [(95, 56, 11, 10), (3, 4, 5, 6)]
    assert T.landmark_bounds(T.landmark("a", 2.5, -2.5, 0, 0)) == (3, -3, 0, 0)


def test_adjust_size_grows_the_short_side():
    lm = T.landmark("a", 50, 40, 20, 30)
    assert T.adjust_size(lm, 1.0, 1.0, 1.0) == ("a", 50, 40, 30, 30)            # width < aspect * height
    assert T.adjust_size(lm, 1.0, 1.0, 0.5) == ("a", 50, 40, 20, 40)            # width > 0.5 * 30: height = width / aspect
    assert T.adjust_size(lm, 1.5, 1.0, 1.0) == ("a", 50, 40, 30, 30)            # equal: unchanged
    out = T.adjust_size(lm, 1.2, 1.1, 4.0 / 3.0)
    assert out[3].dtype == np.float32 and out[4].dtype == np.float32
    # float products: 1.2f * 20 = 24.000002, 1.1f * 30 = 33.000004; 24 < 4/3 * 33.000004 = 44.000005 -> width = float(44.000005)
    assert out[4] == np.float32(1.1) * np.float32(30) and out[3] == np.float32((4.0 / 3.0) * float(np.float32(1.1) * np.float32(30)))


def test_mirroring():
    assert T.flip_landmark(T.landmark("a", 0, 7, 3, 4), 128) == ("a", 127, 7, 3, 4)
    assert T.flip_landmark(T.landmark("a", 127, 7, 3, 4), 128) == ("a", 0, 7, 3, 4)
    assert T.flip_landmark(T.landmark("a", 40.25, 7, 3, 4), 128)[1] == np.float32(86.75)
    img = np.arange(12, dtype=np.uint8).reshape(2, 6)
    assert T.flip_image(img).tolist() == [[5, 4, 3, 2, 1, 0], [11, 10, 9, 8, 7, 6]] and T.flip_image(img).flags.c_contiguous
    bgr = np.arange(12, dtype=np.uint8).reshape(1, 4, 3)
    assert T.flip_image(bgr)[0].tolist() == [[9, 10, 11], [6, 7, 8], [3, 4, 5], [0, 1, 2]]


def test_overlap_at_the_threshold():
    a, b = (0, 0, 10, 10), (5, 0, 10, 10)
    assert T.overlap(a, b) == 50.0 / 150.0 and T.overlap(a, (10, 0, 10, 10)) == 0.0 and T.overlap(a, a) == 1.0
    assert T.overlap((0, 0, 4, 4), (0, 0, 4, 16)) == 0.25             # exactly representable
    assert not T.is_overlapping((0, 0, 4, 4), [(0, 0, 4, 16)], 0.25)  # == keeps
    assert T.is_overlapping((0, 0, 4, 4), [(0, 0, 4, 16)], 0.2499999)  # > rejects
    assert T.is_overlapping((0, 0, 4, 4), [(100, 100, 5, 5), (0, 0, 4, 15)], 0.25)
    assert not T.is_overlapping((0, 0, 4, 4), [], 0.0)


def test_hard_negatives_come_in_candidate_order_not_by_score():
    non_neg = [(0, 0, 10, 10)]
    dets = [(50, 50, 10, 10), (1, 1, 10, 10), (70, 70, 10, 10), (-5, 0, 10, 10), (20, 20, 10, 10), (90, 90, 10, 10)]

    def extract_fn(box):   # the re-extracted bounds move by one pixel; a box that starts left of the image has no patch
        return None if box[0] < 0 else ("f%d" % box[0], (box[0] + 1, box[1], box[2], box[3]))

    got = T.select_hard_negatives(dets, non_neg, 0.3, 3, extract_fn)
    assert [g[0] for g in got] == [(50, 50, 10, 10), (70, 70, 10, 10), (20, 20, 10, 10)]   # the overlapping and the null one skipped
    assert [g[1] for g in got] == ["f50", "f70", "f20"] and got[0][2] == (51, 50, 10, 10)
    assert len(T.select_hard_negatives(dets, non_neg, 0.3, 100, extract_fn)) == 4
    assert T.select_hard_negatives(dets, non_neg, 0.3, 0, extract_fn) == []
    # the overlap test sees the re-extracted bounds, not the detection
    assert T.select_hard_negatives([(10, 0, 10, 10)], non_neg, 0.0, 5, lambda b: ("f", (9, 0, 10, 10))) == []
    assert len(T.select_hard_negatives([(9, 0, 10, 10)], non_neg, 0.0, 5, lambda b: ("f", (10, 0, 10, 10)))) == 1


def test_random_bounds_limits():
    assert T.random_bounds_limits(128, 96, 4, 4, 8) == (32, 96, 1.0)
    assert T.random_bounds_limits(128, 96, 3, 5, 8)[:2] == (24, 57)      # int(96 * 0.6) = 57
    assert T.is_random_bounds((0, 0, 32, 32), 128, 96, 4, 4, 8) and T.is_random_bounds((32, 0, 96, 96), 128, 96, 4, 4, 8)
    assert not T.is_random_bounds((33, 0, 96, 96), 128, 96, 4, 4, 8) and not T.is_random_bounds((0, 0, 31, 31), 128, 96, 4, 4, 8)
    assert T.is_random_bounds((0, 0, 30, 50), 128, 96, 3, 5, 8) and not T.is_random_bounds((0, 0, 30, 49), 128, 96, 3, 5, 8)
