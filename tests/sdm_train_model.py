"""Float64 model of supervised descent training: one cascade step of
LandmarkBasedSupervisedDescentTraining::train (.cpp:297-365) with linearRegression (.cpp:439-518), and the synthetic
faces the tests train on.  numpy only; the descriptors come from a callback (the CPU oracle or the device)."""
import numpy as np

MANUAL, AUTOMATIC = 0, 1

# box-relative landmark positions of the synthetic face, centred ([-0.5, 0.5]^2 is the face box): also the model mean
MEAN_XY = np.array([(-.25, -.2), (.25, -.2), (0, .05), (-.18, .28), (.18, .28)], np.float64)
L = len(MEAN_XY)
MEAN = np.concatenate([MEAN_XY[:, 0], MEAN_XY[:, 1]]).astype(np.float32)


def normal_equations(A, b):
    A64, b64 = np.asarray(A, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    return A64.T @ A64, A64.T @ b64


def regularised(AtA, M, reg, lam, regularise_affine):
    """(lambda, Mreg): Manual: lambda as given; Automatic: lambda * ||AtA||_F / M; the last diagonal element is the bias"""
    D = AtA.shape[0]
    lam = float(lam) * np.sqrt(np.sum(AtA * AtA)) / M if reg == AUTOMATIC else float(lam)
    d = np.full(D, lam)
    if not regularise_affine:
        d[-1] = 0.0
    return lam, AtA + np.diag(d)


def linear_regression(A, b, reg=AUTOMATIC, lam=0.5, regularise_affine=True):
    """returns dict(R float32 [D,N], R64, lam, AtA, Atb, Mreg): Cholesky factorisation and two triangular solves in double, one
    rounding to float"""
    AtA, Atb = normal_equations(A, b)
    lam, Mreg = regularised(AtA, A.shape[0], reg, lam, regularise_affine)
    Lc = np.linalg.cholesky(Mreg)
    R64 = np.linalg.solve(Lc.T, np.linalg.solve(Lc, Atb))
    return dict(R=R64.astype(np.float32), R64=R64, lam=lam, AtA=AtA, Atb=Atb, Mreg=Mreg)


def feature_matrix(desc, images, shapes, dp, variant=1):
    """A: row r = the L descriptors of shapes[r] on images[r] (landmark-major), then a 1.  desc(gray, px, py, num_cells, cell_size,
    num_bins, variant) -> [L, len] float32 or None when a window leaves the image"""
    rows = []
    for img, s in zip(images, shapes):
        n = len(s) // 2
        d = desc(img, s[:n], s[n:], int(dp[0]), int(dp[1]), int(dp[2]), variant)
        if d is None:
            raise RuntimeError("a patch window leaves the image")
        rows.append(np.concatenate([np.asarray(d, np.float32).reshape(-1), np.ones(1, np.float32)]))
    return np.stack(rows)


def errors(gt, x):
    d = (np.asarray(gt, np.float32) - np.asarray(x, np.float32)).astype(np.float64)
    return np.abs(d).sum() / d.size, np.sqrt((d * d).sum())


def train(desc, images, shapes0, gt, desc_params, variant=1, reg=AUTOMATIC, lam=0.5, regularise_affine=True):
    """images: one per row.  Returns dict(R: list of float32 [D_s, 2L], shapes: list of S+1 [M, 2L] float32, info: list of S+1 dicts).
    The update is x += (float)(A R) with the float R, accumulated in double and rounded once, as the fit does."""
    dp = np.asarray(desc_params, np.int64).reshape(-1, 3)
    x = np.asarray(shapes0, np.float32).copy()
    gt = np.asarray(gt, np.float32)
    e = errors(gt, x)
    out = dict(R=[], shapes=[x.copy()], info=[dict(lam=0.0, err_l1=e[0], err_fro=e[1])], steps=[])
    for s in range(len(dp)):
        A = feature_matrix(desc, images, x, dp[s], variant)
        b = gt - x
        lr = linear_regression(A, b, reg, lam, regularise_affine)
        x = x + (A.astype(np.float64) @ lr["R"].astype(np.float64)).astype(np.float32)
        e = errors(gt, x)
        out["R"].append(lr["R"])
        out["steps"].append(lr)
        out["shapes"].append(x.copy())
        out["info"].append(dict(lam=lr["lam"], err_l1=e[0], err_fro=e[1]))
    return out


def fit(desc, image, shape0, Rs, desc_params, variant=1):
    dp = np.asarray(desc_params, np.int64).reshape(-1, 3)
    x = np.asarray(shape0, np.float32).copy()
    for s, R in enumerate(Rs):
        A = feature_matrix(desc, [image], [x], dp[s], variant)
        x = x + (A.astype(np.float64) @ R.astype(np.float64)).astype(np.float32)[0]
    return x


# ---- bounds of the tests: a backward-stable Cholesky solve in double plus one rounding to float
def backward_bound(Mreg, R, Atb):
    D = Mreg.shape[0]
    return 8.0 * D * 2.0 ** -53 * (np.linalg.norm(Mreg) * np.linalg.norm(R) + np.linalg.norm(Atb))


def forward_bound(Mreg, R_model):
    D = Mreg.shape[0]
    return 2.0 ** -24 * np.abs(R_model) + 8.0 * D * 2.0 ** -53 * np.linalg.cond(Mreg) * np.abs(R_model).max()


# ---- synthetic faces
def align_mean(mean, box, sx=1.0, sy=1.0, tx=0.0, ty=0.0):
    """alignMean (.cpp:383-394) in float, evaluated as the cv::MatExpr is: ((m * s) + (0.5f + t)) * w + x"""
    f = np.float32
    m = np.asarray(mean, np.float32)
    n = len(m) // 2
    x, y, w, h = (int(v) for v in box)
    ax = (m[:n] * f(sx) + f(f(0.5) + f(tx))) * f(w) + f(x)
    ay = (m[n:] * f(sy) + f(f(0.5) + f(ty))) * f(h) + f(y)
    return np.concatenate([ax, ay]).astype(np.float32)


def make_face(rng, width=128, height=128):
    """one synthetic training face: (gray [height,width] u8, box (x, y, side, side), landmarks [2L] float32)"""
    bg = rng.standard_normal((height // 4, width // 4))
    img = 128.0 + 25.0 * np.kron(bg, np.ones((4, 4)))
    x0, y0 = int(rng.integers(24, 40)), int(rng.integers(24, 40))
    side = int(rng.integers(56, 72))
    pts = np.empty((L, 2))
    pts[:, 0] = x0 + (MEAN_XY[:, 0] + 0.5) * side
    pts[:, 1] = y0 + (MEAN_XY[:, 1] + 0.5) * side
    pts += rng.normal(0.0, 1.5, pts.shape)
    yy, xx = np.mgrid[0:height, 0:width]
    for i in range(L):
        r2 = (xx - pts[i, 0]) ** 2 + (yy - pts[i, 1]) ** 2
        img[r2 <= 64.0] = 250 - 20 * i
        img[r2 <= 36.0] = 30 + 40 * i
    gray = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return gray, (x0, y0, side, side), np.concatenate([pts[:, 0], pts[:, 1]]).astype(np.float32)


def make_set(seed, n, k, width=128, height=128, sizes=None):
    """n faces with k perturbed start shapes each plus the aligned mean (k + 1 samples per image, the mean first): dict(images
    [list of n], boxes, gt [n*(k+1), 2L], x0 [n*(k+1), 2L], draws [n*k, 3]).  sizes: optional per-face (width, height)"""
    rng = np.random.default_rng(seed)
    images, boxes, gts, x0s, draws = [], [], [], [], []
    for i in range(n):
        w, h = sizes[i] if sizes is not None else (width, height)
        g, box, lm = make_face(rng, w, h)
        images.append(g)
        boxes.append(box)
        x0s.append(align_mean(MEAN, box))
        gts.append(lm)
        for _ in range(k):
            s, tx, ty = rng.normal(1.0, 0.06), rng.normal(0.0, 0.04), rng.normal(0.0, 0.04)   # draw order: scale, tx, ty
            draws.append((s, tx, ty))
            x0s.append(align_mean(MEAN, box, s, s, tx, ty))
            gts.append(lm)
    return dict(images=images, boxes=boxes, gt=np.stack(gts), x0=np.stack(x0s), draws=np.array(draws).reshape(-1, 3), samples=k + 1)


# the configuration of the CPU and GPU training tests
N_TRAIN, K_SAMPLES, DESC_PARAMS, VARIANT = 24, 5, ((2, 8, 4), (2, 8, 4), (1, 8, 4)), 1
N_HELDOUT = 8


# ---- the data preparation of LandmarkBasedSupervisedDescentTraining::train (.cpp:34-193,211-291,383-414), float for float as the host
# class evaluates it (superviseddescent/LandmarkBasedSupervisedDescentTraining.hpp lists how the cv::MatExpr lines fold)
_f = np.float32


def _dsum(v):
    s = 0.0
    for x in v:
        s += float(x)
    return s


def align_mean_ref(mean, box, sx=1.0, sy=1.0, tx=0.0, ty=0.0):
    """alignMean: x * (float)(s * w) + (float)((0.5 + t) * w + box.x), s and t floats"""
    m = np.asarray(mean, np.float32)
    n = len(m) // 2
    x, y, w, h = (int(v) for v in box)
    ax, bx = _f(float(_f(sx)) * w), _f((0.5 + float(_f(tx))) * w + x)
    ay, by = _f(float(_f(sy)) * h), _f((0.5 + float(_f(ty))) * h + y)
    return np.concatenate([m[:n] * ax + bx, m[n:] * ay + by]).astype(np.float32)


def calculate_mean(gt):
    gt = np.asarray(gt, np.float32)
    s = np.zeros(gt.shape[1], np.float32)
    for r in gt:
        s = s + r
    return s * _f(1.0 / gt.shape[0])


def normalise_unit_sum_squared_norms(mean):
    m = np.asarray(mean, np.float32).copy()
    n = len(m) // 2
    m[:n] = m[:n] + _f(-(_dsum(m[:n]) / n))
    m[n:] = m[n:] + _f(-(_dsum(m[n:]) / n))
    total = _f(0.0)
    for p in range(n):
        total = _f(total + _f(_f(m[p] * m[p]) + _f(m[p + n] * m[p + n])))
    return m * _f(1.0 / float(np.sqrt(total)))


def alignment_statistics(boxes, gt, x0):
    """[tx.mu, tx.sigma, ty.mu, ty.sigma, sx.mu, sx.sigma, sy.mu, sy.sigma] as floats"""
    n = gt.shape[1] // 2
    d = [[], [], [], []]
    for box, g, e in zip(boxes, gt, x0):
        for k, (a, b, size) in enumerate(((g[:n], e[:n], box[2]), (g[n:], e[n:], box[3]))):
            d[k].append(_f(_f(_dsum(b) / n - _dsum(a) / n) / _f(size)))
            d[2 + k].append(_f((float(b.max()) - float(b.min())) / (float(a.max()) - float(a.min()))))
    out = []
    for v in d:
        s = sq = 0.0
        for x in v:
            s += float(x)
            sq += float(x) * float(x)
        mean = s / len(v)
        out += [_f(mean), _f(np.sqrt(max(sq / len(v) - mean * mean, 0.0)))]
    return np.array(out, np.float32)


def rescale_model(mean, st):
    m = np.asarray(mean, np.float32)
    n = len(m) // 2
    ax, bx = _f(1.0 / float(st[4])), _f(-float(st[0]) / float(st[4]))
    ay, by = _f(1.0 / float(st[6])), _f(-float(st[2]) / float(st[6]))
    return np.concatenate([m[:n] * ax + bx, m[n:] * ay + by]).astype(np.float32)


def prepare(gt, boxes, draws, samples):
    """gt [n, 2L] float32, boxes [n] (x, y, w, h), draws [n * (samples - 1), 3] (scale, tx, ty) as traced.  Returns dict(mean,
    normalised_mean, stats1, rescaled_mean, stats2, start_shapes [n * samples, 2L])"""
    gt = np.asarray(gt, np.float32)
    mean = calculate_mean(gt)
    nm = normalise_unit_sum_squared_norms(mean)
    st1 = alignment_statistics(boxes, gt, np.stack([align_mean_ref(nm, b) for b in boxes]))
    rm = rescale_model(nm, st1)
    st2 = alignment_statistics(boxes, gt, np.stack([align_mean_ref(rm, b) for b in boxes]))
    draws = np.asarray(draws, np.float32).reshape(-1, 3)
    shapes, k = [], 0
    for b in boxes:
        shapes.append(align_mean_ref(rm, b))
        for _ in range(samples - 1):
            s, tx, ty = draws[k]
            k += 1
            shapes.append(align_mean_ref(rm, b, s, s, tx, ty))
    return dict(mean=mean, normalised_mean=nm, stats1=st1, rescaled_mean=rm, stats2=st2, start_shapes=np.stack(shapes))


def write_app_inputs(dirname, ts, desc_params=DESC_PARAMS, samples_k=K_SAMPLES, factor=0.5, affine=0):
    """images.lst, training.cfg, the PGMs and landmark files of a set for sdm_train_app; returns (lst path, cfg path)"""
    import os
    names = ["lm%d" % i for i in range(L)]
    with open(os.path.join(dirname, "images.lst"), "w") as lst:
        for i, (img, box, lm) in enumerate(zip(ts["images"], ts["boxes"], ts["gt"][::ts["samples"]])):
            pgm, lmf = os.path.join(dirname, "face%02d.pgm" % i), os.path.join(dirname, "face%02d.txt" % i)
            with open(pgm, "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
            with open(lmf, "w") as f:
                for j, nme in enumerate(names):
                    f.write("%s %.9g %.9g\n" % (nme, lm[j], lm[j + L]))
            lst.write("%s %d %d %d %d %s\n" % (pgm, box[0], box[1], box[2], box[3], lmf))
    with open(os.path.join(dirname, "training.cfg"), "w") as f:
        f.write("parameters\n{\n\tnumSamplesPerImage %d\n\tnumCascadeSteps %d\n\tregularisationFactor %g\n\tregulariseAffineComponent %d\n"
                "\tregulariseWithEigenvalueThreshold 0\n\tfeatureDescriptors\n\t{\n" % (samples_k, len(desc_params), factor, affine))
        for s, (nc, cs, nb) in enumerate(desc_params):
            f.write('\t\t%d\n\t\t{\n\t\t\tdescriptorType vlhog-uoctti\n\t\t\tdescriptorParameters "numCells %d cellSize %d numBins %d"\n\t\t}\n' % (s, nc, cs, nb))
        f.write("\t}\n}\nmodelLandmarks\n{\n\tlandmarkType synthetic\n\tlandmarks\n\t{\n" + "".join("\t\t%s\n" % nme for nme in names) + "\t}\n}\n")
    return os.path.join(dirname, "images.lst"), os.path.join(dirname, "training.cfg")
