"""The problems of the large linear C-SVC trainer's tests (fd_linear_svm_train_large): the smallest shapes beyond the 1024 examples
of the small trainer at which its kernel can still go wrong.  Generated from seeds by svm_train_model.ehog_like.

  p  1 + 1024 x 5      the first size the small trainer refuses: not a tile multiple, one thread owns two elements
  q  150 + 1935 x 7    n = 2 * 1024 + 37: three elements per thread, a partial last step of the unrolled loops
  r  40 + 1100 x 5     rows of both classes duplicated (quad_coef = 0 -> TAU)
  g  60 + 1140 x 9     the problem whose libsvm solution is recorded (tests/golden/svm_train_large.npz)

Every model run (svm_train_model.train, pure Python) converges, in 5 to 315 iterations and well under a second each on a CPU, with
the parameters below; the TAU branch is taken five times in either run of r.
"""
import svm_train_model as M


def case_x(name):
    if name == "p":
        return M.ehog_like(1, 1024, 5, 21), 1, 1024
    if name == "q":
        return M.ehog_like(150, 1935, 7, 22), 150, 1935
    if name == "r":
        x = M.ehog_like(40, 1100, 5, 23)
        x[3] = x[1]          # positive copy of a positive
        x[700] = x[1]        # negative copies of it
        x[1139] = x[1]
        x[900] = x[800]      # negative copy of a negative
        return x, 40, 1100
    if name == "g":
        return M.ehog_like(60, 1140, 9, 24), 60, 1140
    raise KeyError(name)


# (case, (C, weight_pos, weight_neg))
CASES = [("p", (1.0, 1.0, 1.0)), ("p", (0.5, 8.0, 0.25)), ("q", (1.0, 1.0, 1.0)), ("r", (1.0, 1.0, 1.0)), ("r", (2.0, 3.0, 0.5)),
         ("g", (1.0, 1.0, 1.0))]
