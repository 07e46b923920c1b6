"""sdm_train_app on the 24 synthetic faces written as PGM: the --trace replayed by the model and by capi.sdm_train, the saved model
through sdm_fit_app --non-adaptive, and two interleaved image sizes coming back in the caller's order."""
import json
import os
import subprocess

import numpy as np
import pytest

import sdm_train_model as T
from test_gpu_sdm_train import check_training

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_APP = os.path.join(ROOT, "featuredetection_amd", "sdm_train_app")
FIT_APP = os.path.join(ROOT, "featuredetection_amd", "sdm_fit_app")


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def run_app(d, ts):
    lst, cfg = T.write_app_inputs(d, ts)
    trace, model = os.path.join(d, "trace.json"), os.path.join(d, "model.txt")
    r = subprocess.run([TRAIN_APP, lst, cfg, model, "--seed", "7", "--trace", trace], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tr = json.load(open(trace))
    dims = [s["dim"] for s in tr["steps"][1:]]
    R = [f32(r_).reshape(dm, 2 * T.L) for r_, dm in zip(tr["R"], dims)]
    return tr, R, model


@pytest.fixture(scope="module")
def app_run(tmp_path_factory):
    ts = T.make_set(20261019, T.N_TRAIN, T.K_SAMPLES)
    return (ts,) + run_app(str(tmp_path_factory.mktemp("sdm_train_app")), ts)


def test_trace_replayed_by_the_model(capi, ctx, app_run):
    ts, tr, R, _ = app_run
    k = ts["samples"]
    gt_img = ts["gt"][::k]
    prep = T.prepare(gt_img, ts["boxes"], f32(tr["draws"]), k)
    x0 = f32(tr["start_shapes"]).reshape(-1, 2 * T.L)
    assert np.array_equal(x0, prep["start_shapes"])
    assert np.array_equal(f32(tr["rescaled_mean"]), prep["rescaled_mean"])
    # the cfg says regularisationFactor 0.5, regulariseAffineComponent 0: the same call through the C ABI
    out = capi.sdm_train(ctx, [np.stack(ts["images"])], k, x0, ts["gt"], T.DESC_PARAMS, T.VARIANT, capi.SDM_REG_AUTOMATIC, 0.5, False)
    images = [ts["images"][i] for i in range(T.N_TRAIN) for _ in range(k)]
    check_training(capi, ctx, out, x0, ts["gt"], images)   # every step's R within bound 2 of the model, lambda within its bound
    assert all(np.array_equal(a, b) for a, b in zip(R, out["R"]))
    assert np.array_equal(f32(tr["final_shapes"]).reshape(-1, 2 * T.L), out["shapes_steps"][-1])
    for s, i in zip(tr["steps"], out["info"]):
        assert s["lambda"] == i["lam"] and s["err_l1"] == i["err_l1"] and s["err_fro"] == i["err_fro"]


def test_saved_model_through_sdm_fit_app(capi, ctx, app_run, tmp_path):
    ts, tr, R, model_path = app_run
    hs = T.make_set(77, 1, 0)
    img, box, gt = hs["images"][0], hs["boxes"][0], hs["gt"][0]
    pgm = str(tmp_path / "held_out.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([FIT_APP, "--non-adaptive", model_path, pgm] + [str(v) for v in box], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    app_shape = f32([float(v) for v in r.stdout.split()])
    mean = f32(tr["rescaled_mean"])
    sdm = capi.Sdm(ctx, dict(L=T.L, S=len(R), mean=mean, R=R, variant=T.VARIANT, desc_params=np.asarray(T.DESC_PARAMS, np.int32).reshape(-1)))
    fitted, st = sdm.fit(img[None], np.asarray([box], np.int32))
    assert not st.any() and np.array_equal(app_shape, fitted[0])
    aligned, _ = capi.Sdm(ctx, dict(L=T.L, S=1, mean=mean, R=[np.zeros_like(R[0])], variant=T.VARIANT,
                                    desc_params=np.asarray(T.DESC_PARAMS[0], np.int32))).fit(img[None], np.asarray([box], np.int32))
    before, after = T.errors(gt, aligned[0])[0], T.errors(gt, app_shape)[0]
    print("held-out face through the apps: L1 %.3f -> %.3f" % (before, after))
    assert after < before


def test_interleaved_sizes_come_back_in_the_callers_order(capi, ctx, tmp_path):
    sizes = [(128, 128) if i % 2 == 0 else (144, 112) for i in range(T.N_TRAIN)]
    ts = T.make_set(5, T.N_TRAIN, T.K_SAMPLES, sizes=sizes)
    tr, R, _ = run_app(str(tmp_path), ts)
    k = ts["samples"]
    x0 = f32(tr["start_shapes"]).reshape(-1, 2 * T.L)
    # the host class sorts by (width, height): the 128-wide faces (even) first, then the 144-wide
    order = list(range(0, T.N_TRAIN, 2)) + list(range(1, T.N_TRAIN, 2))
    rows = np.concatenate([np.arange(i * k, (i + 1) * k) for i in order])
    groups = [np.stack([ts["images"][i] for i in order[:12]]), np.stack([ts["images"][i] for i in order[12:]])]
    out = capi.sdm_train(ctx, groups, k, x0[rows], ts["gt"][rows], T.DESC_PARAMS, T.VARIANT, capi.SDM_REG_AUTOMATIC, 0.5, False)
    final = np.empty_like(x0)
    final[rows] = out["shapes_steps"][-1]
    assert np.array_equal(f32(tr["final_shapes"]).reshape(-1, 2 * T.L), final)
    assert all(np.array_equal(a, b) for a, b in zip(R, out["R"]))
