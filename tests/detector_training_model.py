"""numpy / Python restatement of the host rules of detector training, operation for operation:

  AggregatedFeaturesExtractor::extract(Rect)   box -> layer, cell, bounds (AggregatedFeaturesExtractor.cpp:83-128,
                                               ImagePyramid::getLayer(double) ImagePyramid.cpp:307-310, Patch::computeBounds)
  Annotations                                  Annotations.hpp:20-100
  DetectorTrainer                              adjustSize, mirroring, the overlap test, the selection of hard negatives
                                               (DetectorTrainer.cpp:147-255)

The layer rules themselves (which layers a pyramid has, their scales) are aggregated_approx_model's; here a layer is anything with
the fields index, rows, cols, scale_x, scale_y (a dict, or a record of capi.Aggregated.layers()).  Landmarks are tuples
(name, x, y, width, height) with the centre (x, y) and float32 members like imageio::RectLandmark's; boxes are (x, y, w, h) ints.
"""
import math

import numpy as np

F = np.float32


def cround(v):
    """std::round: half away from zero"""
    v = float(v)
    return int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))


def trunc(v):
    """static_cast<int>"""
    return int(v)


# ---------------- extract(Rect) ----------------
def layer_index(box_width, window_w, cell, octave_layers):
    """ImagePyramid::getLayer(patchWidthPx / width): round(log(scale) / log(inc)), inc = pow(0.5, 1 / octave_layers)"""
    inc = math.pow(0.5, 1.0 / octave_layers)
    scale = float(window_w * cell) / float(box_width)
    return cround(math.log(scale) / math.log(inc))


def resolve(box, layers, window_w, window_h, cell, octave_layers):
    """(position of the layer in `layers`, first cell x, first cell y) of a box, or None where extract returns a null patch"""
    x, y, w, h = (int(v) for v in box)
    if w < 1:
        return None
    index = layer_index(w, window_w, cell, octave_layers)
    pos = [i for i, L in enumerate(layers) if int(L["index"]) == index]
    if not pos:
        return None
    L = layers[pos[-1]]
    cx, cy = x + 0.5 * w, y + 0.5 * h   # Point_<double>
    cell_x = trunc((cx * float(L["scale_x"])) / cell)
    cell_y = trunc((cy * float(L["scale_y"])) / cell)
    x0, y0 = cell_x - window_w // 2, cell_y - window_h // 2   # Patch::computeBounds: positive sizes, so // is C's /
    if x0 < 0 or y0 < 0 or x0 + window_w > int(L["cols"]) or y0 + window_h > int(L["rows"]):
        return None
    return pos[-1], x0, y0


def bounds_in_image(x0, y0, layer, window_w, window_h, cell):
    """computeBoundsInImagePixels: std::round of the cell bounds through the layer's actual scales"""
    sx, sy = float(layer["scale_x"]), float(layer["scale_y"])
    return (cround((x0 * cell) / sx), cround((y0 * cell) / sy), cround((window_w * cell) / sx), cround((window_h * cell) / sy))


def extract(box, layers, feature_layers, window_w, window_h, cell, octave_layers):
    """(features (window_h, window_w, D), bounds) or None; feature_layers[i]: the (rows, cols, D) array of layers[i]"""
    r = resolve(box, layers, window_w, window_h, cell, octave_layers)
    if r is None:
        return None
    i, x0, y0 = r
    return feature_layers[i][y0:y0 + window_h, x0:x0 + window_w].copy(), bounds_in_image(x0, y0, layers[i], window_w, window_h, cell)


# ---------------- landmarks, Annotations ----------------
def landmark(name, x, y, w, h):
    return (name, F(x), F(y), F(w), F(h))


def landmark_from_rect(name, x, y, w, h):
    """RectLandmark(name, Rect): the centre in float"""
    return (name, F(x) + F(0.5) * F(w), F(y) + F(0.5) * F(h), F(w), F(h))


def landmark_bounds(lm):
    """Annotations::getBounds: Landmark::getRect in float, its corners rounded half away from zero"""
    _, x, y, w, h = lm
    tlx, tly = F(x - F(0.5) * w), F(y - F(0.5) * h)
    brx, bry = F(tlx + w), F(tly + h)
    bx, by = cround(tlx), cround(tly)
    return (bx, by, cround(brx) - bx, cround(bry) - by)


def annotations(landmarks, min_size=(0, 0)):
    """dict(non_negatives, positives, fuzzies): a landmark is fuzzy when its name starts with "ignore" or both its sides are below
    min_size"""
    out = dict(non_negatives=[], positives=[], fuzzies=[])
    for lm in landmarks:
        b = landmark_bounds(lm)
        out["non_negatives"].append(b)
        fuzzy = lm[0][:6] == "ignore" or (b[2] < min_size[0] and b[3] < min_size[1])
        out["fuzzies" if fuzzy else "positives"].append(b)
    return out


def adjust_size(lm, width_scale, height_scale, aspect):
    """DetectorTrainer::adjustSize: float sizes, the aspect ratio (window width / height) in double"""
    name, x, y, w, h = lm
    aspect = float(aspect)
    aspect_inv = 1.0 / aspect
    width, height = F(F(width_scale) * w), F(F(height_scale) * h)
    if float(width) < aspect * float(height):
        width = F(aspect * float(height))
    elif float(width) > aspect * float(height):
        height = F(float(width) * aspect_inv)
    return (name, x, y, width, height)


def flip_landmark(lm, image_width):
    """flipHorizontally: float mirroredX = imageWidth - x - 1"""
    name, x, y, w, h = lm
    return (name, F(F(F(image_width) - x) - F(1)), y, w, h)


def flip_image(image):
    return np.ascontiguousarray(image[:, ::-1])


# ---------------- overlap, hard negatives ----------------
def intersection(a, b):
    """cv::Rect operator&"""
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    w, h = min(a[0] + a[2], b[0] + b[2]) - x1, min(a[1] + a[3], b[1] + b[3]) - y1
    return (x1, y1, w, h) if w > 0 and h > 0 else (0, 0, 0, 0)


def overlap(a, b):
    """computeOverlap: intersection over union in double"""
    i = intersection(a, b)
    inter = float(i[2] * i[3])
    union = a[2] * a[3] + b[2] * b[3] - inter
    return inter / union


def is_overlapping(box, others, threshold):
    return any(overlap(box, o) > threshold for o in others)


def select_hard_negatives(detections, non_negatives, threshold, max_count, extract_fn):
    """addHardNegativeExamples: the detections in the detector's candidate order (NonMaximumSuppression(1.0) returns its input
    as it is), each re-extracted (extract_fn(box) -> (features, bounds) or None); accepted when the re-extracted patch exists and
    its bounds do not overlap a non-negative box; until max_count are accepted.  Returns [(detection, features, bounds)]."""
    out = []
    for det in detections:
        if len(out) >= max_count:
            break
        r = extract_fn(det)
        if r is None or is_overlapping(r[1], non_negatives, threshold):
            continue
        out.append((tuple(int(v) for v in det), r[0], r[1]))
    return out


def random_bounds_limits(image_w, image_h, window_w, window_h, cell):
    """createRandomBounds draws width in [window width in pixels, min(image width, int(image height * aspect))], height =
    round(width / aspect), x in [0, image width - width], y in [0, image height - height]"""
    aspect = float(window_w) / float(window_h)
    return window_w * cell, min(image_w, int(image_h * aspect)), aspect


def is_random_bounds(box, image_w, image_h, window_w, window_h, cell):
    lo, hi, aspect = random_bounds_limits(image_w, image_h, window_w, window_h, cell)
    x, y, w, h = box
    return lo <= w <= hi and h == cround(w * (1.0 / aspect)) and 0 <= x <= image_w - w and 0 <= y <= image_h - h


# ---------------- the training loop (DetectorTrainer::train), replayed ----------------
def textured_square(size, rng):
    """a square with a bright frame, a dark inside and a bright diagonal cross, on which some noise"""
    s = np.full((size, size), 40.0)
    b = max(2, size // 8)
    s[:b] = s[-b:] = 230
    s[:, :b] = s[:, -b:] = 230
    for k in range(size):
        lo, hi = max(0, k - 1), min(size, k + 2)
        s[k, lo:hi] = 230
        s[k, size - hi:size - lo] = 230
    return np.clip(s + rng.normal(0, 6, s.shape), 0, 255).astype(np.uint8)


def make_training_set(seed, count=6, width=128, height=96, held_out=True):
    """count gray images of noise with one textured square each (sizes 34 .. 46 pixels), as [(image, [(name, x, y, w, h) boxes with
    their top-left corner])]; image 2 also has an `ignore` region; the last entry is the held-out image when asked for"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count + (1 if held_out else 0)):
        img = rng.integers(96, 160, (height, width)).astype(np.uint8)
        size = int(rng.integers(34, 47))
        x, y = int(rng.integers(4, width - size - 4)), int(rng.integers(4, height - size - 4))
        img[y:y + size, x:x + size] = textured_square(size, rng)
        boxes = [("square", x, y, size, size)]
        if k == 2:
            ix = 4 if x > width // 2 else width - 40
            boxes.append(("ignore-region", ix, 8, 36, 36))
        out.append((img, boxes))
    return out


class ModelBackend:
    """feature layers and window scores from the CPU oracle: Pyramid, fhog, and aggregated_approx_model's score map and candidates"""

    def __init__(self, oracle, cfg):
        import aggregated_approx_model as A
        self.O, self.A, self.cfg = oracle, A, cfg

    def update(self, image):
        c = self.cfg
        h, w = image.shape[:2]
        lo, hi = self.A.limits(c["window_w"], c["window_h"], c["cell"], c["n"], 0, w, h)
        pyr = self.O.Pyramid(octave_layers=c["n"], min_scale=lo, max_scale=hi)
        pyr.update(image)
        self.layers, self.feats = [], []
        for k, L in enumerate(pyr.layers()):
            self.layers.append(dict(index=L["index"], rows=L["h"] // c["cell"], cols=L["w"] // c["cell"], scale=L["scale"], scale_x=L["w"] / w,
                                    scale_y=L["h"] / h))
            self.feats.append(self.O.fhog(pyr.layer(k), cell_size=c["cell"], unsigned_bins=9))

    def extract(self, box):
        c = self.cfg
        r = extract(box, self.layers, self.feats, c["window_w"], c["window_h"], c["cell"], c["n"])
        return None if r is None else (r[0].reshape(-1), r[1])

    def detect(self, weights, bias, threshold):
        scores = self.A.all_scores(self.layers, self.feats, weights, bias)
        _, boxes, _ = self.A.candidates(self.layers, scores, threshold, self.cfg)
        return [tuple(int(v) for v in b) for b in boxes]


class NegativeStore:
    """the negatives of the classifier: unlimited, or HardNegativeExampleManagement(capacity) -- ConfidenceBasedExampleManagement
    for negatives with nothing kept unconditionally: the confidence of a negative x is -(w . x - bias); free space is filled
    least confident first, then the least confident new example replaces the most confident stored one while it is the less
    confident of the two.  An untrained classifier takes the examples in their order."""

    def __init__(self, capacity):
        self.capacity, self.rows = capacity, []

    def add(self, new, svm):
        if not self.capacity:
            self.rows += list(new)
            return
        if svm is None:
            self.rows += list(new)[:max(0, self.capacity - len(self.rows))]
            return
        w, bias = svm

        def conf(x):
            return -(float(w.reshape(-1).astype(np.float64) @ x.astype(np.float64)) - float(bias))

        existing = sorted(range(len(self.rows)), key=lambda p: -conf(self.rows[p]))
        incoming = sorted(new, key=conf)
        while len(self.rows) < self.capacity and incoming:
            self.rows.append(incoming.pop(0))
        for p in existing:
            if not incoming or not conf(incoming[0]) < conf(self.rows[p]):
                break
            self.rows[p] = incoming.pop(0)


def replay_training(images, cfg, params, backend, train_fn, draws=None, seed=0):
    """DetectorTrainer::train on [(image, boxes)] (boxes with their top-left corner).  cfg: window_w, window_h, cell, n; params:
    mirror, random_per_image, max_hard_per_image, rounds, negative_threshold, overlap, max_negatives, C.
    train_fn(x float32 (n, d), n_pos, C) -> (weights float32 (d,), rho, iterations).  draws: the random boxes of every image block
    in draw order (a list per (image, mirrored) block, as a trace records them); None: drawn here from numpy's generator.
    Returns the list of records ("image", index, mirrored, round), ("positive" | "random" | "hard", box, accepted, bounds | None),
    ("training", initial, n_pos, n_neg, new_pos, new_neg, iterations, rho, weights)."""
    ww, wh, cell = cfg["window_w"], cfg["window_h"], cfg["cell"]
    aspect = float(ww) / float(wh)
    rng = np.random.default_rng(seed)
    rec, positives, new_pos, new_neg = [], [], [], []
    store = NegativeStore(params["max_negatives"])
    svm = None
    block = [0]

    def random_box(w, h):
        lo, hi, _ = random_bounds_limits(w, h, ww, wh, cell)
        bw = int(rng.integers(lo, hi + 1))
        bh = cround(bw * (1.0 / aspect))
        return (int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1)), bw, bh)

    def add_negative(kind, box, non_negatives):
        r = backend.extract(box)
        ok = r is not None and not is_overlapping(r[1], non_negatives, params["overlap"])
        rec.append((kind, tuple(int(v) for v in box), ok, None if r is None else r[1]))
        if ok:
            new_neg.append(r[0])
        return ok

    def one_image(image, landmarks, initial):
        ann = annotations(landmarks)
        backend.update(image)
        if initial:
            for box in ann["positives"]:
                r = backend.extract(box)
                rec.append(("positive", box, r is not None, None if r is None else r[1]))
                if r is not None:
                    new_pos.append(r[0])
            mine = None if draws is None else list(draws[block[0]])
            added = 0
            while added < params["random_per_image"]:
                box = random_box(image.shape[1], image.shape[0]) if mine is None else mine.pop(0)
                added += 1 if add_negative("random", box, ann["non_negatives"]) else 0
            assert not mine, "the trace holds draws the replay does not need"
            block[0] += 1
        else:
            added = 0
            for det in backend.detect(svm[0], svm[1], params["negative_threshold"]):
                if added >= params["max_hard_per_image"]:
                    break
                added += 1 if add_negative("hard", det, ann["non_negatives"]) else 0

    def collect(initial, rnd):
        for k, (image, boxes) in enumerate(images):
            lms = [adjust_size(landmark_from_rect(*b), 1.0, 1.0, aspect) for b in boxes]
            rec.append(("image", k, 0, rnd))
            one_image(image, lms, initial)
            if params["mirror"]:
                rec.append(("image", k, 1, rnd))
                one_image(flip_image(image), [flip_landmark(lm, image.shape[1]) for lm in lms], initial)

    def train(initial):
        nonlocal svm
        if not new_pos and not new_neg:
            return
        positives.extend(new_pos)
        store.add(new_neg, svm)
        x = np.stack(positives + store.rows).astype(np.float32)
        w, rho, iterations = train_fn(x, len(positives), params["C"])
        w = w.reshape(wh, ww, -1)
        rec.append(("training", initial, len(positives), len(store.rows), len(new_pos), len(new_neg), iterations, rho, w))
        svm = (w, np.float32(rho))
        del new_pos[:], new_neg[:]

    collect(True, -1)
    train(True)
    for rnd in range(params["rounds"]):
        collect(False, rnd)
        train(False)
    return rec


def parse_trace(text):
    """the records of DetectorTrainer::setTrace in replay_training's form, and the random draws of every image block"""
    rec, draws = [], []
    lines = text.splitlines()
    for k, line in enumerate(lines):
        t = line.split()
        if t[0] == "image":
            rec.append(("image", int(t[1]), int(t[2]), int(t[3])))
            if int(t[3]) == -1:
                draws.append([])
        elif t[0] in ("positive", "random", "hard"):
            box = tuple(int(v) for v in t[1:5])
            rest = t[5:]
            accepted = None
            if t[0] != "positive":
                accepted, rest = bool(int(rest[0])), rest[1:]
            bounds = tuple(int(v) for v in rest[1:5]) if rest[0] == "1" else None
            rec.append((t[0], box, bounds is not None if accepted is None else accepted, bounds))
            if t[0] == "random":
                draws[-1].append(box)
        elif t[0] == "training":
            w = lines[k + 1].split()
            assert w[0] == "weights"
            rec.append(("training", bool(int(t[1])), int(t[2]), int(t[3]), int(t[4]), int(t[5]), int(t[6]), float.fromhex(t[7]),
                        np.array([float.fromhex(v) for v in w[2:]], np.float32), np.float32(float.fromhex(w[1]))))
    return rec, draws
