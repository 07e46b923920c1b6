"""The problems the liblinear tests share: the six recorded ones of tests/golden/liblinear_tron.npz (inputs and the w that the
reference's linear.cpp + tron.cpp gave at eps = 0.01) and two generated larger ones.  A case is (x float32 (n, d), n_pos, n_neg,
C, bias); models and references are computed once per process."""
import os

import numpy as np

import liblinear_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "liblinear_tron.npz")
EXTRA = {"n1280": (7, 257, 1023, 129, 1.0, 1), "n1000": (8, 300, 700, 324, 1.0, 0)}   # seed, n_pos, n_neg, d, C, bias
_cache = {}


def make_x(seed, n_pos, n_neg, d, sep=0.6):
    """two overlapping classes on a 1/1024 grid (exact in float32)"""
    rng = np.random.default_rng(seed)
    y = np.concatenate([np.ones(n_pos), -np.ones(n_neg)])
    direction = rng.normal(size=d) / np.sqrt(d)
    x = np.abs(rng.normal(size=(n_pos + n_neg, d))) * 0.5 + sep * y[:, None] * direction[None, :] + 0.25
    return (np.round(x * 1024) / 1024).astype(np.float32)


def golden():
    if "golden" not in _cache:
        _cache["golden"] = np.load(GOLDEN)
    return _cache["golden"]


def golden_names():
    return [str(n) for n in golden()["names"]]


def all_names():
    return golden_names() + sorted(EXTRA)


def case(name):
    if ("case", name) not in _cache:
        if name in EXTRA:
            seed, n_pos, n_neg, d, c, bias = EXTRA[name]
            v = (make_x(seed, n_pos, n_neg, d), n_pos, n_neg, c, bool(bias))
        else:
            g = golden()
            n_pos, n_neg, d, bias = (int(t) for t in g[name + "_meta"])
            v = (np.ascontiguousarray(g[name + "_x"], np.float32), n_pos, n_neg, float(g[name + "_C"]), bool(bias))
        v[0].setflags(write=False)
        _cache[("case", name)] = v
    return _cache[("case", name)]


def model(name, solver_tol=0.0):
    """the float64 model's run on the case, at the reference's eps or at a solver tolerance"""
    key = ("model", name, solver_tol)
    if key not in _cache:
        x, n_pos, n_neg, c, bias = case(name)
        _cache[key] = M.tron(x, n_pos, n_neg, C=c, bias=bias, eps=0.01, solver_tol=solver_tol)
    return _cache[key]
