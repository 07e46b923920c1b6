"""Records tests/golden/svm_one_class_*.npz and svm_cv_sigmoid_*.npz from the compiled reference's libsvm (oracle/_ref): the
one-class models of svm_one_class_model.case_x("int40") for every kernel and nu, and per case of svm_cv_sigmoid_model.CASES the
permutation, the cross-validation decision values (svm_train and svm_predict_values fold by fold) and probA, probB of svm_train
with probability = 1.  Run from the repository root: python tests/golden/make_svm_prob_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import svm_cv_sigmoid_model as CV   # noqa: E402
import svm_kernel_train_model as K   # noqa: E402
import svm_one_class_model as OC   # noqa: E402
from oracle import pyoracle   # noqa: E402

ref = pyoracle.ref()
assert ref is not None, "oracle/_ref is absent"
x = OC.case_x("int40")
kernels = K.KERNELS + [OC.LINEAR_KERNEL]
alpha = np.zeros((len(kernels), len(OC.NUS), len(x)))
rho = np.zeros((len(kernels), len(OC.NUS)))
for ki, kernel in enumerate(kernels):
    for ni, nu in enumerate(OC.NUS):
        alpha[ki, ni], rho[ki, ni], _ = OC.libsvm_train(ref, x, kernel, nu)
np.savez_compressed(os.path.join(HERE, "svm_one_class_int40.npz"), xsum=float(x.astype(np.float64).sum()), kernels=np.array(kernels),
                    nus=np.array(OC.NUS), alpha=alpha, rho=rho, eps=1e-4)
for name in CV.CASES:
    x, n_pos, ks, perm, c, wp, wn = CV.case(name)
    seed = CV.CASES[name][6]
    dec = np.array([CV.libsvm_cv_dec(ref, x, n_pos, k, perm, c, wp, wn) for k in ks])
    ab = np.array([CV.libsvm_prob(ref, x, n_pos, k, seed, c, wp, wn) for k in ks])
    np.savez_compressed(os.path.join(HERE, "svm_cv_sigmoid_%s.npz" % name), xsum=float(x.astype(np.float64).sum()), kernels=np.array(ks),
                        perm=perm, dec=dec, prob_a=ab[:, 0], prob_b=ab[:, 1], eps=1e-4)
    print(name, ab.tolist())
