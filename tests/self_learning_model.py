"""The examples of condensation::SelfLearningMeasurementModel::adapt (SelfLearningMeasurementModel.cpp:89-125) in numpy / plain
Python, both branches, for the tests of fd_particles_examples_select and fd_particles_state_examples_* (DESIGN.md 4.7).

The reference walks the samples in index order and collects the candidates of either side; a side with more than `max_count`
candidates is sorted (positives by weight descending, negatives ascending) and cut to its first `max_count`, a side with fewer is
left as collected.  Its std::sort is unstable; the sorts here are stable, which is the project's tie rule: equal weights keep the
lower index first.

 - bootstrap branch (the model is not usable, :103-121): every sample of the generation is walked, with or without a patch; whether
   a chosen sample has one is found out by the extraction afterwards.
 - usable branch (:91-101, fed by evaluate, :53-74): only samples with a patch ever enter the lists; one without has weight 0 but is
   no example.

The walk tests the negative threshold only where the positive one was not passed (`else if`), and so does select() here.  The library
tests the two independently and refuses negative_threshold > positive_threshold: for every pair it accepts no weight passes both
tests, and the two forms are the same."""
import numpy as np


def weight_ok(w):
    return bool(w >= 0.0 and w <= np.finfo(np.float64).max)


def select(weight, valid, positive_threshold, negative_threshold, max_count, require_window):
    """(positive indices, negative indices) in list order; ValueError for a weight that is negative or not finite"""
    weight = np.asarray(weight, np.float64)
    if not all(weight_ok(w) for w in weight):
        raise ValueError("a weight is negative or not finite")
    good, bad = [], []
    for i, w in enumerate(weight):
        if require_window and not valid[i]:
            continue
        if w > positive_threshold:
            good.append(i)
        elif w < negative_threshold:
            bad.append(i)
    if len(good) > max_count:
        good = sorted(good, key=lambda i: -weight[i])[:max_count]   # stable: equal weights stay in index order
    if len(bad) > max_count:
        bad = sorted(bad, key=lambda i: weight[i])[:max_count]
    return np.array(good, np.int32), np.array(bad, np.int32)


def records(gen, index, valid=None):
    """the records fd_particles_state_examples_* reports for these samples of a generation (dict of arrays)"""
    index = np.asarray(index, np.int64)
    out = {"index": index.astype(np.int32), "x": gen["x"][index].astype(np.int32), "y": gen["y"][index].astype(np.int32),
           "size": gen["size"][index].astype(np.int32), "weight": gen["weight"][index].astype(np.float64)}
    if valid is not None:
        out["valid"] = np.asarray(valid, np.int32)
    return out
