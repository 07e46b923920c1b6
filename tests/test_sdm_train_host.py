"""sdm_train_app --prepare-only (no device call) against the model of the reference's data preparation in tests/sdm_train_model.py
(LandmarkBasedSupervisedDescentTraining.cpp:34-193,211-291,383-414): mean, normalised mean, both alignment statistics, rescaled mean
and start shapes are equal float for float when the model replays the traced draws."""
import json
import os
import subprocess

import numpy as np
import pytest

import sdm_train_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "sdm_train_app")


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sdm_prepare"))
    ts = T.make_set(20261019, 12, 3)
    lst, cfg = T.write_app_inputs(d, ts, samples_k=3)
    trace = os.path.join(d, "trace.json")
    r = subprocess.run([APP, lst, cfg, os.path.join(d, "unused.txt"), "--seed", "11", "--trace", trace, "--prepare-only"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(os.path.join(d, "unused.txt"))
    return ts, json.load(open(trace))


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def test_preparation_equals_the_model(prepared):
    ts, tr = prepared
    gt = ts["gt"][::ts["samples"]]
    assert (tr["images"], tr["samples"], tr["landmarks"]) == (12, 4, T.L)
    m = T.prepare(gt, ts["boxes"], f32(tr["draws"]), tr["samples"])
    assert np.array_equal(f32(tr["mean"]), m["mean"])
    assert np.array_equal(f32(tr["normalised_mean"]), m["normalised_mean"])
    assert np.array_equal(f32(tr["alignment_statistics_1"]), m["stats1"])
    assert np.array_equal(f32(tr["rescaled_mean"]), m["rescaled_mean"])
    assert np.array_equal(f32(tr["alignment_statistics_2"]), m["stats2"])
    assert np.array_equal(f32(tr["start_shapes"]).reshape(-1, 2 * T.L), m["start_shapes"])


def test_preparation_properties(prepared):
    ts, tr = prepared
    nm = f32(tr["normalised_mean"]).astype(np.float64)
    assert abs((nm * nm).sum() - 1.0) < 1e-5 and abs(nm[:T.L].sum()) < 1e-5 and abs(nm[T.L:].sum()) < 1e-5
    st2 = f32(tr["alignment_statistics_2"])
    assert abs(st2[4] - 1.0) < 0.05 and abs(st2[6] - 1.0) < 0.05   # the rescaled mean has the data's scale
    draws = f32(tr["draws"]).reshape(-1, 3)
    assert draws.shape == (12 * 3, 3) and len(np.unique(draws[:, 0])) == len(draws)   # one engine: no draw repeats
    x0 = f32(tr["start_shapes"]).reshape(12, 4, -1)
    gt = ts["gt"][::ts["samples"]]
    assert np.abs(x0[:, 0] - gt).mean() < 4.0   # the aligned rescaled mean lies on the faces
    assert tr["steps"] == [] and tr["R"] == []


def test_seed_decides_the_draws(prepared, tmp_path):
    ts, tr = prepared
    lst, cfg = T.write_app_inputs(str(tmp_path), ts, samples_k=3)
    out = []
    for seed in ("11", "12"):
        trace = str(tmp_path / ("t%s.json" % seed))
        subprocess.run([APP, lst, cfg, "x", "--seed", seed, "--trace", trace, "--prepare-only"], check=True)
        out.append(json.load(open(trace))["draws"])
    assert out[0] == tr["draws"] and out[1] != out[0]
