"""Supervised descent training on the device (csrc/sdm_train.hpp) against the float64 model in
tests/sdm_train_model.py: the Gram kernel, the Cholesky solve, the error return for a matrix that is not positive definite, the
cascade trainer, its bit-equality with fd_sdm_optimize_batch, size groups and the invalid-row error."""
import numpy as np
import pytest

import sdm_train_model as T

pytestmark = pytest.mark.gpu

# one tile; exact tile multiples; D and N no multiples of 16, M no multiple of 4; more than two Cholesky panels with a short last one
SHAPES = [(5, 17, 2), (33, 64, 16), (70, 130, 6), (144, 321, 10)]
EPS = 2.0 ** -53


def lr_case(M, D, N):
    rng = np.random.default_rng(1000 * M + D)
    return rng.standard_normal((M, D)).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)


@pytest.mark.parametrize("M,D,N", SHAPES)
def test_gram(capi, ctx, M, D, N):
    A, b = lr_case(M, D, N)
    x, lam, ata, atb = capi.sdm_linear_regression(ctx, A, b, capi.SDM_REG_AUTOMATIC, 0.5, True, want_normal_equations=True)
    m = T.linear_regression(A, b, T.AUTOMATIC, 0.5, True)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    ea = np.abs(ata - m["AtA"]) / (M * EPS * (np.abs(A64).T @ np.abs(A64)))
    eb = np.abs(atb - m["Atb"]) / (M * EPS * (np.abs(A64).T @ np.abs(b64)))
    print("gram %s: max error / bound AtA %.3f Atb %.3f, lambda rel %.2e" % ((M, D, N), ea.max(), eb.max(), abs(lam - m["lam"]) / m["lam"]))
    assert ea.max() <= 1.0 and eb.max() <= 1.0
    assert np.array_equal(ata, ata.T)
    assert abs(lam - m["lam"]) <= D * D * EPS * m["lam"]
    x2, lam2, ata2, atb2 = capi.sdm_linear_regression(ctx, A, b, capi.SDM_REG_AUTOMATIC, 0.5, True, want_normal_equations=True)
    assert np.array_equal(ata, ata2) and np.array_equal(atb, atb2) and np.array_equal(x, x2) and lam == lam2


def check_solve(R, m, tag, R64_dev=None):
    """bound 2 of DESIGN.md 4.9.  Backward error: ||Mreg R - Atb||_F <= 8 D 2^-53 (||Mreg||_F ||R||_F + ||Atb||_F) holds for the
    double solution a Cholesky solve returns (R64_dev, where the entry point exposes it).  The float R is that solution rounded once,
    |R - R64| <= 2^-24 |R64|, which moves the residual by at most 2^-24 ||Mreg||_F ||R||_F: the float R is held to the sum of the two.
    Forward error of the float R: |R - R_model| <= 2^-24 |R_model| + 8 D 2^-53 cond2(Mreg) max|R_model|."""
    R64 = R.astype(np.float64)
    nM = np.linalg.norm(m["Mreg"])
    if R64_dev is not None:
        back64, bb64 = np.linalg.norm(m["Mreg"] @ R64_dev - m["Atb"]), T.backward_bound(m["Mreg"], R64_dev, m["Atb"])
        print("solve %s: double solution backward %.3e (bound %.3e)" % (tag, back64, bb64))
        assert back64 <= bb64
        assert np.array_equal(R, R64_dev.astype(np.float32))
    back = np.linalg.norm(m["Mreg"] @ R64 - m["Atb"])
    bb = T.backward_bound(m["Mreg"], R64, m["Atb"]) + 2.0 ** -24 * nM * np.linalg.norm(R64)
    fwd = np.abs(R64 - m["R64"]) / T.forward_bound(m["Mreg"], m["R64"])
    print("solve %s: backward %.3e (bound %.3e), forward error / bound %.3f, cond %.3e" % (tag, back, bb, fwd.max(), np.linalg.cond(m["Mreg"])))
    assert np.isfinite(R).all()
    assert back <= bb
    assert fwd.max() <= 1.0


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("reg,lam", [(T.AUTOMATIC, 0.5), (T.MANUAL, 1.0)])
@pytest.mark.parametrize("M,D,N", SHAPES)
def test_solve(capi, ctx, M, D, N, reg, lam, affine):
    A, b = lr_case(M, D, N)
    if not affine:
        A[:, -1] = 1.0   # the column regularise_affine == 0 leaves alone is the bias column
    R, lam_dev = capi.sdm_linear_regression(ctx, A, b, reg, lam, affine)
    m = T.linear_regression(A, b, reg, lam, affine)
    assert abs(lam_dev - m["lam"]) <= D * D * EPS * m["lam"]
    check_solve(R, m, (M, D, N, reg, affine), capi.sdm_linear_regression_solution(ctx, D, N))


def test_not_positive_definite(capi, ctx):
    A, b = lr_case(5, 17, 2)
    with pytest.raises(capi.FdError) as e:
        capi.sdm_linear_regression(ctx, A, b, capi.SDM_REG_MANUAL, 0.0, True)
    assert e.value.code == capi.FD_ERR_RUNTIME and "lambda" in str(e.value)
    R, _ = capi.sdm_linear_regression(ctx, A, b, capi.SDM_REG_MANUAL, 1.0, True)   # the context is fine
    check_solve(R, T.linear_regression(A, b, T.MANUAL, 1.0, True), "after the error")


def test_eigenvalue_threshold_is_not_built(capi, ctx):
    A, b = lr_case(5, 17, 2)
    with pytest.raises(capi.FdError) as e:
        capi.sdm_linear_regression(ctx, A, b, capi.SDM_REG_EIGENVALUE_THRESHOLD, 0.5, True)
    assert e.value.code == capi.FD_ERR_INVALID_ARGUMENT and "EigenvalueThreshold" in str(e.value)


def device_desc(capi, ctx):
    return lambda gray, px, py, nc, cs, nb, variant: capi.sdm_descriptors(ctx, gray, px, py, 0, variant, nc, cs, nb)


def run_training(capi, ctx, ts, groups, order):
    """groups: list of [count,H,W] arrays; order: the set's image index of every image in group order"""
    k = ts["samples"]
    rows = np.concatenate([np.arange(i * k, (i + 1) * k) for i in order])
    x0, gt = ts["x0"][rows], ts["gt"][rows]
    out = capi.sdm_train(ctx, groups, k, x0, gt, T.DESC_PARAMS, T.VARIANT, capi.SDM_REG_AUTOMATIC, 0.5, False)
    images = [ts["images"][i] for i in order for _ in range(k)]
    return out, x0, gt, images


def check_training(capi, ctx, out, x0, gt, images):
    S = len(T.DESC_PARAMS)
    steps, info = out["shapes_steps"], out["info"]
    assert np.array_equal(steps[0], x0) and not out["row_status"].any()
    slack = np.sqrt(x0.size) * 2.0 ** -23 * np.abs(steps).max()
    for s in range(S + 1):
        l1, fro = T.errors(gt, steps[s])
        assert abs(info[s]["err_l1"] - l1) <= 1e-12 * l1 and abs(info[s]["err_fro"] - fro) <= 1e-12 * fro
        assert info[s]["rows"] == len(x0) and info[s]["pivot_flag"] == 0
        if s:
            assert info[s]["err_fro"] <= info[s - 1]["err_fro"] + slack
    print("train L1", [round(i["err_l1"], 3) for i in info])
    for s in range(S):
        # A rebuilt from the device's descriptors at the shapes the step started from; the model solves the same system
        A = T.feature_matrix(device_desc(capi, ctx), images, steps[s], T.DESC_PARAMS[s], T.VARIANT)
        m = T.linear_regression(A, gt - steps[s], T.AUTOMATIC, 0.5, False)
        D = A.shape[1]
        assert info[s + 1]["dim"] == D and out["R"][s].shape == (D, x0.shape[1])
        assert abs(info[s + 1]["lam"] - m["lam"]) <= D * D * EPS * m["lam"]
        check_solve(out["R"][s], m, "training step %d" % s)


@pytest.fixture(scope="module")
def trainset():
    return T.make_set(20261019, T.N_TRAIN, T.K_SAMPLES)


@pytest.fixture(scope="module")
def trained(capi, ctx, trainset):
    return run_training(capi, ctx, trainset, [np.stack(trainset["images"])], list(range(T.N_TRAIN)))


def test_training(capi, ctx, trainset, trained):
    out, x0, gt, images = trained
    check_training(capi, ctx, out, x0, gt, images)
    again = run_training(capi, ctx, trainset, [np.stack(trainset["images"])], list(range(T.N_TRAIN)))[0]
    assert np.array_equal(again["shapes_steps"], out["shapes_steps"])
    assert all(np.array_equal(a, b) for a, b in zip(again["R"], out["R"]))
    assert [i["lam"] for i in again["info"]] == [i["lam"] for i in out["info"]]


def sdm_model(R, s):
    return dict(L=T.L, S=s, mean=T.MEAN, R=R[:s], variant=T.VARIANT, desc_params=np.asarray(T.DESC_PARAMS, np.int32)[:s].reshape(-1))


def test_held_out_faces_improve(capi, ctx, trained):
    out = trained[0]
    hs = T.make_set(77, T.N_HELDOUT, 0)
    fitted, st = capi.Sdm(ctx, sdm_model(out["R"], len(out["R"]))).optimize(np.stack(hs["images"]), hs["x0"])
    before, after = T.errors(hs["gt"], hs["x0"])[0], T.errors(hs["gt"], fitted)[0]
    print("held-out L1 %.3f -> %.3f" % (before, after))
    assert not st.any() and after < before


def test_trajectory_equals_optimize(capi, ctx, trained):
    """the trainer's shapes after step s are bit for bit fd_sdm_optimize_batch's on the model of the first s regressors"""
    out, x0, gt, images = trained
    imgs = np.stack(images)
    for s in range(1, len(out["R"]) + 1):
        fitted, st = capi.Sdm(ctx, sdm_model(out["R"], s)).optimize(imgs, x0)
        assert not st.any()
        assert np.array_equal(fitted, out["shapes_steps"][s]), "step %d" % s


def test_two_size_groups(capi, ctx):
    """12 faces of 128x128 and 12 of 144x112, interleaved in the set; the groups hold them sorted by size"""
    sizes = [(128, 128) if i % 2 == 0 else (144, 112) for i in range(T.N_TRAIN)]
    ts = T.make_set(5, T.N_TRAIN, T.K_SAMPLES, sizes=sizes)
    even, odd = list(range(0, T.N_TRAIN, 2)), list(range(1, T.N_TRAIN, 2))
    groups = [np.stack([ts["images"][i] for i in even]), np.stack([ts["images"][i] for i in odd])]
    assert groups[0].shape[1:] == (128, 128) and groups[1].shape[1:] == (112, 144)
    out, x0, gt, images = run_training(capi, ctx, ts, groups, even + odd)
    check_training(capi, ctx, out, x0, gt, images)
    # every size group on its own reaches the same shapes through the fit (rows are in group order: the even faces first)
    k, half = ts["samples"], len(even) * ts["samples"]
    for grp, rows in ((groups[0], np.arange(0, half)), (groups[1], np.arange(half, 2 * half))):
        fitted, st = capi.Sdm(ctx, sdm_model(out["R"], len(out["R"]))).optimize(np.repeat(grp, k, axis=0), x0[rows])
        assert not st.any() and np.array_equal(fitted, out["shapes_steps"][-1][rows])


def test_row_whose_window_leaves_the_image(capi, ctx, trainset):
    k = trainset["samples"]
    x0 = trainset["x0"].copy()
    bad = 7 * k + 3
    x0[bad, 0] = 400.0   # far right of the 128-pixel image: the window fails the reference's roi assertion
    with pytest.raises(capi.FdError) as e:
        capi.sdm_train(ctx, [np.stack(trainset["images"])], k, x0, trainset["gt"], T.DESC_PARAMS, T.VARIANT, capi.SDM_REG_AUTOMATIC, 0.5, False)
    assert e.value.code == capi.FD_ERR_RUNTIME
    assert np.flatnonzero(e.value.row_status).tolist() == [bad]
    assert all(not r.any() for r in e.value.R)   # R_out untouched


def test_groups_resident_on_the_device(capi, ctx, trainset, trained):
    """on_device = 1: the images of a group are read where they lie in HBM; same bits as the uploaded group"""
    import torch
    out = trained[0]
    imgs = torch.from_numpy(np.stack(trainset["images"])).cuda()
    torch.cuda.synchronize()
    k = trainset["samples"]
    dev = capi.sdm_train(ctx, [(imgs.data_ptr(), imgs.shape[0], imgs.shape[1], imgs.shape[2])], k, trainset["x0"], trainset["gt"], T.DESC_PARAMS,
                         T.VARIANT, capi.SDM_REG_AUTOMATIC, 0.5, False)
    assert np.array_equal(dev["shapes_steps"], out["shapes_steps"]) and all(np.array_equal(a, b) for a, b in zip(dev["R"], out["R"]))


def test_rows_the_kernels_cannot_index_are_refused(capi, ctx):
    """rows x 2L >= 2^31 is an argument error before anything is allocated (the shape arrays are never read)"""
    import ctypes as C
    L = 68
    p, _keep = capi._sdm_train_params(L, ((3, 12, 4),), 1, capi.SDM_REG_AUTOMATIC, 0.5, True)
    g = (capi.fd_sdm_train_group * 1)()
    img = np.zeros((1, 64, 64), np.uint8)
    g[0].images, g[0].width, g[0].height, g[0].count, g[0].on_device = img.ctypes.data, 64, 64, 1 << 24, 0
    one = np.zeros(2 * L, np.float32)
    ptrs = (C.c_void_p * 1)(one.ctypes.data)
    rc = capi.lib().fd_sdm_train(ctx.h, C.byref(p), g, 1, 1, one.ctypes.data, one.ctypes.data, ptrs, None, None, None)
    assert rc == capi.FD_ERR_INVALID_ARGUMENT and b"2^31" in capi.lib().fd_last_error(ctx.h)
