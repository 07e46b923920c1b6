"""fd_sample_layer_table (host only): the width -> layer table the device reads in place of the log in the sample -> window rule
(k_particles_windows).  Every entry is compared with the layer fd_sample_windows and its restatement
(tests/pyramid_samples_model.py) give a centred sample of that width on layers large enough to hold it: the table is the rule's own
index expression, so every width on either side of every layer change must agree, and the table must end exactly behind the largest
width that has a layer."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pyramid_samples_model as model

INT32_MAX = 2 ** 31 - 1
SIDE = 1 << 20   # layer size: holds the window of every centred sample below
GRID = list(itertools.product((0.5, 0.8, float(np.float32(0.9)), 0.95), (-2, 0, 3), (1, 4, 64), (1, 16, 31)))


def _layers(inc, first, count):
    return [dict(index=k, scale=inc ** k, w=SIDE, h=SIDE) for k in range(first, first + count)]


def _layer_of(capi, inc, first, count, pw, widths):
    """the layer position fd_sample_windows gives a centred sample of each width, -1 for none"""
    w = np.asarray(widths, np.int64)
    c = np.maximum(w, 0) // 2 + 3
    out = capi.sample_windows(_layers(inc, first, count), inc, pw, pw, np.stack([c, c, w, w], 1).astype(np.int32))
    assert np.array_equal(out[:, 3] == 1, out[:, 0] >= 0)
    return out[:, 0]


def _raw(capi, n_layers, first, inc, pw, cap, table, with_length=True):
    length = C.c_int(-7)
    rc = capi.lib().fd_sample_layer_table(n_layers, first, inc, pw, cap, table.ctypes.data_as(C.c_void_p) if table is not None else None,
                                          C.byref(length) if with_length else None)
    return rc, length.value


@pytest.mark.parametrize("inc,first,count,pw", GRID)
def test_table_is_the_rule(capi, inc, first, count, pw):
    rc, length = _raw(capi, count, first, inc, pw, 0, None)
    assert rc in (capi.FD_OK, capi.FD_ERR_CAPACITY) and 0 <= length <= INT32_MAX
    assert (rc == capi.FD_OK) == (length == 0)
    # length is exact: the width in front of it has a layer, the widths from it on have none
    edge = [w for w in range(max(length - 2, -1), length + 3) if w <= INT32_MAX]
    got = _layer_of(capi, inc, first, count, pw, edge)
    if length == 0:
        assert (got == -1).all()
    elif length == INT32_MAX:
        assert got[edge.index(INT32_MAX)] >= 0
    else:
        assert got[edge.index(length - 1)] >= 0 and (got[edge.index(length):] == -1).all(), (length, got)
    if length > capi.FD_SAMPLE_TABLE_MAX:
        with pytest.raises(capi.FdError) as e:
            capi.sample_layer_table(count, first, inc, pw)
        assert e.value.code == capi.FD_ERR_CAPACITY and e.value.length == length
        return
    table = capi.sample_layer_table(count, first, inc, pw)
    assert table.dtype == np.int16 and len(table) == length
    widths = np.arange(-1, length + 3)
    want = _layer_of(capi, inc, first, count, pw, widths)
    # the restatement, width by width (sample_windows of the model is the rule in Python: libm's log, lround)
    c = np.maximum(widths, 0) // 2 + 3
    restated = model.sample_windows(_layers(inc, first, count), inc, pw, pw, np.stack([c, c, widths, widths], 1))[:, 0]
    assert np.array_equal(want, restated)
    padded = np.full(len(widths), -1, np.int64)   # entries are -1 outside the table
    padded[1:1 + length] = table
    assert np.array_equal(padded, want), np.flatnonzero(padded != want)[:5] - 1
    if length:   # no layer below some width, then layers that do not decrease; both sides of every change were compared above
        kept = table[table >= 0].astype(np.int64)
        assert table[0] == -1 and table[-1] >= 0 and (table[:length - len(kept)] == -1).all() and (np.diff(kept) >= 0).all()


def test_known_table(capi):
    """0.8, four layers from index 0, patch width 16: lround(log(16 / w) / log(0.8)) changes between 17|18, 22|23, 27|28 and ends behind 34"""
    table = capi.sample_layer_table(4, 0, 0.8, 16)
    assert table.tolist() == [-1] * 15 + [0] * 3 + [1] * 5 + [2] * 5 + [3] * 7
    assert len(capi.sample_layer_table(0, 0, 0.8, 16)) == 0          # no layers: no table
    assert len(capi.sample_layer_table(1, -2, 0.5, 1)) == 0          # index -2 of patch width 1: widths below 1
    assert capi.sample_layer_table(64, -70, 0.95, 31).max() == 63 and capi.sample_layer_table(64, -70, 0.95, 31)[1] >= 0


def test_capacity_and_arguments(capi):
    rc, length = _raw(capi, 4, 0, 0.8, 16, 0, None)
    assert (rc, length) == (capi.FD_ERR_CAPACITY, 35)
    small = np.full(40, 99, np.int16)
    assert _raw(capi, 4, 0, 0.8, 16, 34, small) == (capi.FD_ERR_CAPACITY, 35) and (small == 99).all()   # nothing written
    assert _raw(capi, 4, 0, 0.8, 16, 35, small) == (capi.FD_OK, 35) and (small[35:] == 99).all() and small[34] == 3
    bad = capi.FD_ERR_INVALID_ARGUMENT
    table = np.zeros(64, np.int16)
    assert _raw(capi, -1, 0, 0.8, 16, 64, table)[0] == bad
    assert _raw(capi, 40000, 0, 0.8, 16, 64, table)[0] == bad          # positions are int16
    assert _raw(capi, 4, 0, 0.8, 0, 64, table)[0] == bad
    for inc in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert _raw(capi, 4, 0, inc, 16, 64, table)[0] == bad, inc
    assert _raw(capi, 4, 0, 0.8, 16, -1, table)[0] == bad
    assert _raw(capi, 4, 0, 0.8, 16, 64, None)[0] == bad
    assert _raw(capi, 4, 0, 0.8, 16, 64, table, with_length=False)[0] == bad


def test_a_table_longer_than_the_device_takes(capi):
    inc, first, count, pw = 0.8, 0, 64, 16
    estimate = pw / inc ** (first + count - 1 + 0.5)   # the width at which the index rounds past the last layer
    assert capi.FD_SAMPLE_TABLE_MAX + 2 < estimate < INT32_MAX - 2   # the condition of this test
    with pytest.raises(capi.FdError) as e:
        capi.sample_layer_table(count, first, inc, pw)
    assert e.value.code == capi.FD_ERR_CAPACITY
    length = e.value.length
    assert length > capi.FD_SAMPLE_TABLE_MAX and abs(length - estimate) <= 2
    assert _layer_of(capi, inc, first, count, pw, [length - 1, length, length + 1]).tolist() == [count - 1, -1, -1]
    table = capi.sample_layer_table(count, first, inc, pw, cap=length)   # the host function itself builds it, at any length
    assert len(table) == length and table[-1] == count - 1
    probe = np.unique(np.concatenate([np.flatnonzero(np.diff(table.astype(np.int64))) + d for d in (0, 1)]))   # both sides of every change
    assert len(probe) == 2 * count and np.array_equal(table[probe], _layer_of(capi, inc, first, count, pw, probe))
