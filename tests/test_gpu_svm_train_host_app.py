"""svm_train_app: libsvm::LibSvmClassifier::createOneClassKernelSvm and createBinaryKernelSvm(.., probabilistic) from a feature matrix
and a config with headTrackingApp's keys, against capi.one_class_svm_train / kernel_svm_cv_sigmoid / kernel_svm_train with the
permutation libc draws after srand(seed) (tests/svm_cv_sigmoid_model.libc_perm)."""
import os
import subprocess

import numpy as np
import pytest

import svm_cv_sigmoid_model as CV
import svm_kernel_train_model as K
import svm_one_class_model as OC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "featuredetection_amd", "svm_train_app")
KERNEL_CFG = {K.HIK: "kernel hik\n", K.LINEAR: "kernel linear\n", K.RBF: "kernel rbf\n{\n\tgamma %r\n}\n",
              K.POLY: "kernel poly ; the reference's keys\n{\n\talpha %r\n\tconstant %r\n\tdegree %d\n}\n"}


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _run(tmp_path, x, n_pos, kernel, training, seed=None):
    feats, cfg, out = tmp_path / "features.txt", tmp_path / "classifier.cfg", tmp_path / "svm.txt"
    with open(feats, "w") as f:
        f.write("%d %d %d\n" % (n_pos, len(x) - n_pos, x.shape[1]))
        for row in x:
            f.write(" ".join("%.9g" % v for v in row) + "\n")
    kind, p0, p1, p2 = kernel
    kcfg = KERNEL_CFG[kind]
    kcfg = kcfg % p0 if kind == K.RBF else (kcfg % (p0, p1, int(p2)) if kind == K.POLY else kcfg)
    cfg.write_text(kcfg + training)
    run = subprocess.run([APP, str(feats), str(cfg), str(out)] + (["--seed", str(seed)] if seed is not None else []), capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    printed = dict(line.split() for line in run.stdout.strip().splitlines())
    return printed, out


def _read_svm(path, kernel, d):
    """the text format of SvmClassifier::store (nine significant digits: exact for float32) as a capi.Svm model dict, and the
    Logistic line's two numbers or None"""
    tokens = open(path).read().split()
    names = {K.HIK: ["HIK"], K.LINEAR: ["Linear"], K.RBF: ["RBF", None], K.POLY: ["Polynomial", None, None, None]}[kernel[0]]
    assert tokens[0] == "Kernel" and tokens[1] == names[0]
    at = 1 + len(names)
    assert tokens[at] == "Bias" and tokens[at + 2] == "Coefficients"
    bias, n = np.float32(tokens[at + 1]), int(tokens[at + 3])
    coeff = np.array(tokens[at + 4:at + 4 + n], np.float32)
    at += 4 + n
    assert tokens[at:at + 6] == ["SupportVectors", str(n), "1", str(d), "1", "5"]
    sv = np.array(tokens[at + 6:at + 6 + n * d], np.float32).reshape(n, d)
    rest = tokens[at + 6 + n * d:]
    logistic = None
    if rest:
        assert rest[0] == "Logistic" and len(rest) == 3
        logistic = (float(rest[1]), float(rest[2]))
    return dict(kernel=kernel[0], p0=kernel[1], p1=kernel[2], p2=kernel[3], dtype=1, sv=sv, coeff=coeff, bias=bias), logistic


def test_one_class(capi, ctx, tmp_path):
    x, kernel, nu = OC.case_x("int40"), OC.HIK_KERNEL, 0.26
    printed, out = _run(tmp_path, x, len(x), kernel, "training one-class\n{\n\tC 1\n\tnu %r\n}\n" % nu)
    sv_index, coef, sv, bias, alpha, info = capi.one_class_svm_train(ctx, x, kernel, nu=nu, eps=1e-4)
    assert float(printed["rho"]) == info["rho"] and int(printed["n_sv"]) == info["n_sv"] and int(printed["iterations"]) == info["iterations"]
    assert "probA" not in printed
    model, logistic = _read_svm(out, kernel, x.shape[1])
    assert logistic is None
    assert _bits(model["coeff"]) == _bits(coef) and _bits(model["sv"]) == _bits(sv) and _bits(model["bias"]) == _bits(np.float32(bias))
    assert capi.FD_DTYPE_F32 == model["dtype"]
    trained, _ = capi.one_class_svm_train_model(ctx, x, kernel, nu=nu, eps=1e-4)
    assert _bits(capi.Svm(ctx, model).distance(x)) == _bits(trained.distance(x))


def test_one_class_ignores_the_negatives_and_reports_infinite_rho(capi, ctx, tmp_path):
    """the reference's default nu = 1; the negatives of the matrix are not read"""
    x, n_pos, kernels, perm, c, wp, wn = CV.case("int65")
    printed, out = _run(tmp_path, x, n_pos, kernels[0], "training one-class\n{\n\tnu 1\n}\n")
    assert printed["rho"] == "inf" and int(printed["n_sv"]) == n_pos


@pytest.mark.parametrize("compensate", [False, True], ids=["plain", "compensateImbalance"])
def test_probabilistic_binary(capi, ctx, tmp_path, compensate):
    x, n_pos, kernels, _, c, _, _ = CV.case("int65")
    kernel, seed = kernels[0], 7
    wp, wn = ((len(x) - n_pos) / n_pos, n_pos / (len(x) - n_pos)) if compensate else (1.0, 1.0)
    printed, out = _run(tmp_path, x, n_pos, kernel, "training binary\n{\n\tC %r\n\tnu 0.5\n\tcompensateImbalance %s\n\tprobabilistic true\n}\n" %
                        (c, "true" if compensate else "false"), seed)
    a, b, dec, cv = capi.kernel_svm_cv_sigmoid(ctx, x, n_pos, kernel, CV.libc_perm(seed, len(x)), C=c, weight_pos=wp, weight_neg=wn, eps=1e-4)
    sv_index, coef, sv, bias, alpha, info = capi.kernel_svm_train(ctx, x, n_pos, kernel, C=c, weight_pos=wp, weight_neg=wn, eps=1e-4)
    assert (float(printed["probA"]), float(printed["probB"])) == (a, b)
    assert float(printed["rho"]) == info["rho"] and int(printed["n_sv"]) == info["n_sv"]
    model, logistic = _read_svm(out, kernel, x.shape[1])
    assert logistic == (b, a)   # ProbabilisticSvmClassifier's A and B are libsvm's B and A
    assert _bits(model["coeff"]) == _bits(coef) and _bits(model["sv"]) == _bits(sv) and _bits(model["bias"]) == _bits(np.float32(bias))
    trained, _ = capi.kernel_svm_train_model(ctx, x, n_pos, kernel, C=c, weight_pos=wp, weight_neg=wn, eps=1e-4)
    assert _bits(capi.Svm(ctx, model).distance(x)) == _bits(trained.distance(x))
    if not compensate:   # another seed, another shuffle
        other, _ = _run(tmp_path, x, n_pos, kernel, "training binary\n{\n\tC %r\n\tprobabilistic true\n}\n" % c, seed + 1)
        assert float(other["probA"]) != a and float(other["rho"]) == info["rho"]


def test_binary_without_the_fit_writes_no_logistic_line(capi, ctx, tmp_path):
    x, n_pos, kernels, _, c, wp, wn = CV.case("float55")
    printed, out = _run(tmp_path, x, n_pos, kernels[1], "training binary\n{\n\tC %r\n}\n" % c, 9)
    info = capi.kernel_svm_train(ctx, x, n_pos, kernels[1], C=c, eps=1e-4)[5]
    assert "probA" not in printed and float(printed["rho"]) == info["rho"]
    assert _read_svm(out, kernels[1], x.shape[1])[1] is None


def test_bad_config_is_an_error(tmp_path):
    x = OC.case_x("int40")
    feats, cfg = tmp_path / "f.txt", tmp_path / "c.cfg"
    feats.write_text("40 0 10\n" + "\n".join(" ".join("%g" % v for v in row) for row in x) + "\n")
    for text in ("kernel sigmoid\ntraining binary\n", "kernel hik\ntraining ternary\n", "kernel hik\ntraining one-class\n{\n\tnu 1.5\n}\n"):
        cfg.write_text(text)
        run = subprocess.run([APP, str(feats), str(cfg), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=120)
        assert run.returncode == 1 and run.stderr.startswith("error:"), (text, run.stderr)
