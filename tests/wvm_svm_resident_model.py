"""condensation::WvmSvmModel for a resident particle set (fd_particles_evaluate_wvm_svm / _weigh_wvm_svm) restated on
per-sample (valid, level, fout) and the SVM distances of the selected samples: the key t, the selection of the up to 8 most probable WVM
positives with its tie rule, targets, weights with libm's exp, best_score and n_valid.  Python floats are IEEE doubles, one operation at
a time; math.exp is libm's.  It never calls the library under test."""
import math

import numpy as np

RESCORED = 8                      # WvmSvmModel.cpp:98-99: resize(8)
LOWEST = -1.7976931348623157e308  # numeric_limits<double>::lowest(): the best score of a generation without samples


def key(logistic_a, logistic_b, fout):
    """t = logisticA + logisticB * (double)fout: one product, one sum (ProbabilisticWvmClassifier.cpp:52)"""
    return float(logistic_a) + float(logistic_b) * float(np.float32(fout))


def exp(t):
    try:
        return math.exp(t)
    except OverflowError:
        return math.inf


def p_wvm(t):
    """1.0f / (1.0f + exp(t)) in double"""
    return 1.0 / (1.0 + exp(t))


def p_svm(logistic_a, logistic_b, distance):
    """ProbabilisticSvmClassifier.cpp:54-58"""
    f = float(logistic_a) + float(logistic_b) * float(distance)
    return exp(-f) / (1.0 + exp(-f)) if f >= 0 else 1.0 / (1.0 + exp(f))


def positives(wvm, level, fout):
    """WvmClassifier::classify: the last filter is reached and passed"""
    level, fout = np.asarray(level), np.asarray(fout, np.float32)
    return (level + 1 == int(wvm["num_filters"])) & (fout >= np.float32(wvm["thresholds"][int(wvm["num_filters"]) - 1]))


def order(t, i):
    """the sort key of a candidate: ascending t (descending probability), a NaN behind every number, equal t by particle index"""
    return (1, 0.0, i) if t != t else (0, t + 0.0, i)


def select(wvm, valid, level, fout):
    """the particles the SVM re-scores, most probable first: of the WVM positives whose particle is valid the up to 8 with the smallest
    (t, index)"""
    pos = positives(wvm, level, fout)
    cand = [order(key(wvm["logistic_a"], wvm["logistic_b"], fout[i]), i) for i in range(len(valid)) if valid[i] and pos[i]]
    return [c[2] for c in sorted(cand)[:RESCORED]]


def tie_free(wvm, valid, level, fout):
    """the precondition under which the reference's unstable sort + resize(8) selects what select() does: with more than 8 candidates the
    8th and 9th most probable differ in probability (probabilities are what the reference compares)"""
    pos = positives(wvm, level, fout)
    probs = sorted((p_wvm(key(wvm["logistic_a"], wvm["logistic_b"], fout[i])) for i in range(len(valid)) if valid[i] and pos[i]), reverse=True)
    return len(probs) <= RESCORED or probs[RESCORED - 1] != probs[RESCORED], len(probs)


def weigh(wvm, svm, valid, level, fout, selected, distances):
    """(target uint8, weight float64, score float64, best_score, n_valid) given the SVM distances of select()'s particles, in its order"""
    n = len(valid)
    target, weight, score = np.zeros(n, np.uint8), np.zeros(n, np.float64), np.zeros(n, np.float64)
    where = {i: k for k, i in enumerate(selected)}
    threshold = float(np.float32(svm.get("threshold", 0.0)))
    best = LOWEST
    for i in range(n):
        if valid[i]:
            score[i] = float(np.float32(fout[i]))
            w = 0.5 * p_wvm(key(wvm["logistic_a"], wvm["logistic_b"], fout[i]))
            if i in where:
                d = float(distances[where[i]])
                target[i] = d >= threshold
                w = 2 * w * p_svm(svm.get("logistic_a", 0.00556), svm.get("logistic_b", -2.95), d)
            weight[i] = w
        best = max(best, float(score[i]))
    return target, weight, score, best, int(np.count_nonzero(valid))
