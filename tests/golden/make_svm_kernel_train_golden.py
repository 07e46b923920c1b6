"""Writes tests/golden/svm_kernel_train_{a,b,c}.npz: what the compiled reference's svm_train (oracle/_ref/libfdref.so, built where
the reference tree is present) returns on the small training problems of tests/svm_train_model.py for every kernel of
tests/svm_kernel_train_model.py and every parameter set of the case: alpha, rho, the support-vector count, and the model's own
sv_indices / sv_coef (padded to n with -1 / 0) and labels.  X is the seeded generator's (pinned by svm_train_{a,b,c}.npz).

    python tests/golden/make_svm_kernel_train_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import svm_train_model as M   # noqa: E402
import svm_kernel_train_model as K   # noqa: E402
from oracle import pyoracle as O   # noqa: E402


def main():
    ref = O.ref()
    if ref is None:
        raise SystemExit("oracle/_ref/libfdref.so is not built")
    for name in "abc":
        x, n_pos, n_neg = M.case_x(name)
        n = n_pos + n_neg
        params = np.array(M.params_of(name), np.float64)   # rows (C, weight_pos, weight_neg)
        alpha = np.zeros((len(K.KERNELS), len(params), n))
        rho = np.zeros((len(K.KERNELS), len(params)))
        n_sv = np.zeros((len(K.KERNELS), len(params)), np.int32)
        sv_index = -np.ones((len(K.KERNELS), len(params), n), np.int32)
        sv_coef = np.zeros((len(K.KERNELS), len(params), n))
        label = np.zeros((len(K.KERNELS), len(params), 2), np.int32)
        for ki, kernel in enumerate(K.KERNELS):
            for pi, (c, wp, wn) in enumerate(params):
                a, r, si, sc, lb = K.libsvm_train(ref, x, n_pos, kernel, c, wp, wn, 1e-4)
                alpha[ki, pi], rho[ki, pi], n_sv[ki, pi], label[ki, pi] = a, r, len(si), lb
                sv_index[ki, pi, :len(si)] = si
                sv_coef[ki, pi, :len(si)] = sc
        np.savez_compressed(os.path.join(HERE, "svm_kernel_train_%s.npz" % name), kernels=np.array(K.KERNELS, np.float64), params=params,
                            eps=np.float64(1e-4), xsum=np.float64(x.astype(np.float64).sum()), alpha=alpha, rho=rho, n_sv=n_sv,
                            sv_index=sv_index, sv_coef=sv_coef, label=label)


if __name__ == "__main__":
    main()
