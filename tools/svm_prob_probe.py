"""libsvm's sigmoid fit and one-class training on the device (fd_kernel_svm_cv_sigmoid, fd_one_class_svm_train): ms per call for
the RBF and histogram-intersection kernels, next to libsvm's svm_train with probability = 1 / svm_type ONE_CLASS on this machine's
CPU for the same problems.

  python tools/svm_prob_probe.py
  python tools/svm_prob_probe.py --reps 30

Shapes: 20 + 100 x 455 and 20 + 300 x 1085 ehog-like rows, as tools/svm_kernel_train_probe.py; the one-class problems are the same
rows without their labels, nu = 0.5.  Every call ends in a synchronise of its own and is timed with the host clock around it, after
warm-up calls; medians with p10 / p90 are reported.  fd_kernel_svm_train on the whole problem is timed next to the fit, since
libsvm's svm_train with probability = 1 includes the final training and the device call does not.  libsvm (the compiled reference
unit, oracle/_ref) is timed around svm_train alone, where that unit is present; it is the baseline -- the parent commit has neither
mode, so there is no parent time and no ratio to pass.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # noqa: F401  before libfd_hip.so: the wheel brings its own HIP runtime (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((20, 100, 455), (20, 300, 1085))
SEED, NU = 7, 0.5


def stats(ms):
    return dict(ms_median=float(np.median(ms)), ms_p10=float(np.percentile(ms, 10)), ms_p90=float(np.percentile(ms, 90)))


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()   # ends in a device synchronise
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import svm_cv_sigmoid_model as CV
    import svm_kernel_train_model as K
    import svm_one_class_model as OC
    import svm_train_model as M
    from featuredetection_amd import capi
    from oracle import pyoracle as O
    ctx = capi.Context(0)
    ref = O.ref()
    cpu_reps = max(3, a.reps // 4)
    results = []
    for n_pos, n_neg, d in SHAPES:
        x = M.ehog_like(n_pos, n_neg, d, seed=100 + n_neg)
        perm = CV.libc_perm(SEED, n_pos + n_neg)
        for kernel in (K.KERNELS[0], K.KERNELS[4]):
            pa, pb, dec, cv = capi.kernel_svm_cv_sigmoid(ctx, x, n_pos, kernel, perm)
            r = dict(kernel=K.kernel_id(kernel), n_pos=n_pos, n_neg=n_neg, d=d, prob_a=pa, prob_b=pb, newton_iterations=cv["newton_iterations"],
                     fold_iterations=[f["iterations"] for f in cv["folds"]], fold_launches=cv["folds"][0]["launches"],
                     cv_sigmoid=timed(lambda: capi.kernel_svm_cv_sigmoid(ctx, x, n_pos, kernel, perm), a.reps),
                     final_train=timed(lambda: capi.kernel_svm_train(ctx, x, n_pos, kernel), a.reps))
            sv_index, coef, sv, bias, alpha, info = capi.one_class_svm_train(ctx, x, kernel, nu=NU)
            r["one_class"] = dict(info=info, train=timed(lambda: capi.one_class_svm_train(ctx, x, kernel, nu=NU), a.reps))
            if ref is not None:
                ms = []
                for _ in range(cpu_reps):
                    la, lb = CV.libsvm_prob(ref, x, n_pos, kernel, SEED)
                    ms.append(CV.last_train_seconds * 1e3)
                r["libsvm_cpu_probability"] = stats(ms)
                r["libsvm_prob_a_diff"], r["libsvm_prob_b_diff"] = abs(la - pa), abs(lb - pb)
                ms = []
                for _ in range(cpu_reps):
                    oa, orho, _ = OC.libsvm_train(ref, x, kernel, NU)
                    ms.append(OC.last_train_seconds * 1e3)
                r["one_class"]["libsvm_cpu"] = stats(ms)
                r["one_class"]["libsvm_max_alpha_diff"] = float(np.abs(oa - alpha).max())
                r["one_class"]["libsvm_rho_diff"] = float(abs(orho - info["rho"]))
            else:
                r["libsvm_cpu_probability"] = r["one_class"]["libsvm_cpu"] = "not measured (oracle/_ref absent)"
            results.append(r)
    ctx.close()
    print(json.dumps(dict(probe="svm_prob", reps=a.reps, results=results)))


if __name__ == "__main__":
    main()
