"""Writes tests/golden/svm_train_{a,b,c}.npz and svm_train_def.npz: the small training problems of tests/svm_train_model.py (n <= 24) with what the
compiled reference's svm_train (oracle/_ref/libfdref.so, built where the reference tree is present) returns for every
parameter set of the case: alpha (from sv_coef / sv_indices), rho and the support-vector count.

    python tests/golden/make_svm_train_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import svm_train_model as M   # noqa: E402
from oracle import pyoracle as O   # noqa: E402


def main():
    ref = O.ref()
    if ref is None:
        raise SystemExit("oracle/_ref/libfdref.so is not built")
    for name in "abc":
        x, n_pos, n_neg = M.case_x(name)
        params = np.array(M.params_of(name), np.float64)   # rows (C, weight_pos, weight_neg)
        res = [M.libsvm_train(ref, x, n_pos, c, wp, wn, 1e-4) for c, wp, wn in params]
        np.savez_compressed(os.path.join(HERE, "svm_train_%s.npz" % name), x=x, n_pos=np.int32(n_pos), n_neg=np.int32(n_neg),
                            params=params, eps=np.float64(1e-4), alpha=np.array([r[0] for r in res]),
                            rho=np.array([r[1] for r in res]), n_sv=np.array([r[2] for r in res], np.int32))
    # the larger cases d, e, f: libsvm's alpha and rho only (X comes from the seeded generator; a checksum pins it)
    big = {}
    for name in "def":
        x, n_pos, n_neg = M.case_x(name)
        alpha, rho, n_sv = M.libsvm_train(ref, x, n_pos, 1.0, 1.0, 1.0, 1e-4)
        big["alpha_" + name], big["rho_" + name], big["xsum_" + name] = alpha, np.float64(rho), np.float64(x.astype(np.float64).sum())
    np.savez_compressed(os.path.join(HERE, "svm_train_def.npz"), **big)


if __name__ == "__main__":
    main()
