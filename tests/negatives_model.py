"""The additional negatives of condensation::PositionDependentMeasurementModel::adapt (PositionDependentMeasurementModel.cpp:155-192) in
numpy: the box around the target in the host's float and int arithmetic, the `outside` predicate, and the choice -- once as the closed
form fd_particles_state_negatives documents (choose) and once as a literal restatement of the reference's loop (reference_loop).  A
generation is a dict of arrays keyed like condensation_model.FIELDS; a choice is the array of sample indices in the list's order."""
import numpy as np

NEGATIVES_MAX = 64
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def scales(offset_factor):
    """(negativeOffsetFactor, downScaleBound, upScaleBound) as the floats adapt forms"""
    with np.errstate(divide="ignore"):
        f = np.float32(offset_factor)
        down = np.float32(1) - f
        return f, down, np.float32(1) / down


def _to_int(v):
    """(int) of a float: truncated; saturated outside the int range, 0 for a NaN"""
    v = np.float32(v)
    if np.isnan(v):
        return 0
    if v >= np.float32(2147483648.0):
        return INT32_MAX
    if v <= np.float32(-2147483648.0):
        return INT32_MIN
    return int(np.trunc(v))


def _wrap(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def bounds(offset_factor, x, y, size, down_scale=None, up_scale=None):
    """[xLow, xHigh, yLow, yHigh, sizeLow, sizeHigh] of the target {x, y, size}: float * int is a float product, the int sums wrap"""
    f, down, up = scales(offset_factor)
    down = down if down_scale is None else np.float32(down_scale)
    up = up if up_scale is None else np.float32(up_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.float32(size)   # int -> float: to the nearest, ties to even
        offset = _to_int(f * s)
        return [_wrap(x - offset), _wrap(x + offset), _wrap(y - offset), _wrap(y + offset), _to_int(down * s), _to_int(up * s)]


def outside(b, x, y, size):
    x, y, size = (np.asarray(v, np.int64) for v in (x, y, size))
    return (x <= b[0]) | (x >= b[1]) | (y <= b[2]) | (y >= b[3]) | (size <= b[4]) | (size >= b[5])


def choose(gen, max_count, offset_factor, target):
    """the closed form: of the samples outside the box the max_count largest under (weight descending, index ascending), listed by
    (weight ascending, index descending)"""
    weight = np.asarray(gen["weight"], np.float64) + 0.0
    candidates = np.flatnonzero(outside(bounds(offset_factor, *target), gen["x"], gen["y"], gen["size"]))
    best = candidates[np.lexsort((candidates, -weight[candidates]))][:max_count]
    return best[np.lexsort((-best, weight[best]))].astype(np.int32)


def reference_loop(gen, max_count, offset_factor, target):
    """:172-192 line by line: a list ascending by weight, lower_bound insertion while it is not full, afterwards the front is replaced
    when front.weight < sample.weight and bubbled up while prev > next"""
    b = bounds(offset_factor, *target)
    weight = [float(w) for w in gen["weight"]]
    chosen = []
    for i in range(len(weight)):
        if not outside(b, gen["x"][i], gen["y"][i], gen["size"][i]):
            continue
        if len(chosen) < max_count:
            low = 0
            while low < len(chosen) and weight[chosen[low]] < weight[i]:   # std::lower_bound on a sorted list
                low += 1
            chosen.insert(low, i)
        elif weight[chosen[0]] < weight[i]:
            chosen[0] = i
            k = 1
            while k < len(chosen) and weight[chosen[k - 1]] > weight[chosen[k]]:
                chosen[k - 1], chosen[k] = chosen[k], chosen[k - 1]
                k += 1
    return np.array(chosen, np.int32)


def records(gen, order):
    """what the device reports for a choice: dict of index, x, y, size (int32) and weight (float64, the stored bits)"""
    order = np.asarray(order, np.int32)
    out = {k: np.asarray(gen[k], np.int32)[order] for k in ("x", "y", "size")}
    out["index"] = order
    out["weight"] = np.asarray(gen["weight"], np.float64)[order]
    return out
