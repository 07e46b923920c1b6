"""Writes tests/golden/svm_train_large.npz: what the compiled reference's svm_train (oracle/_ref/libfdref.so, built where the
reference tree is present) returns for case g of tests/svm_train_large_cases.py, a problem with more than 1024 examples:
alpha (from sv_coef / sv_indices), rho and the support-vector count.  The reference's libsvm is compiled with its info() output
off, so its iteration count cannot be read; `iterations` is the count of tests/svm_train_model.py on the same problem, recorded
once the model's alpha and rho agree with libsvm's.  X comes from the seeded generator; its sum pins it.

    python tests/golden/make_svm_train_large_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import svm_train_model as M   # noqa: E402
import svm_train_large_cases as L   # noqa: E402
from oracle import pyoracle as O   # noqa: E402


def main():
    ref = O.ref()
    if ref is None:
        raise SystemExit("oracle/_ref/libfdref.so is not built")
    x, n_pos, n_neg = L.case_x("g")
    alpha, rho, n_sv = M.libsvm_train(ref, x, n_pos, 1.0, 1.0, 1.0, 1e-4)
    r = M.train(x, n_pos, 1.0, 1.0, 1.0, 1e-4)
    if np.abs(r["alpha"] - alpha).max() > 1e-12 or abs(r["rho"] - rho) > 1e-12 or r["n_sv"] != n_sv or not r["converged"]:
        raise SystemExit("the model and libsvm disagree on case g")
    iterations = r["iterations"]
    np.savez_compressed(os.path.join(HERE, "svm_train_large.npz"), alpha=alpha, rho=np.float64(rho), n_sv=np.int32(n_sv),
                        iterations=np.int32(iterations), xsum=np.float64(x.astype(np.float64).sum()))
    print("n = %d, %d support vectors, %d iterations, rho = %r" % (len(x), n_sv, iterations, rho))


if __name__ == "__main__":
    main()
