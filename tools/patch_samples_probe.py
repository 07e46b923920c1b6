"""The RVM cascade on sampled gray patches: the fused kernel, the composed route and the per-sample loop.

  python tools/patch_samples_probe.py [--reps 200] [--warmup 20] [--loop-reps 3] [--loop-max 4000] [--sizes 27,100,..]

640 x 480 frame, gray pyramid of 3 layers per octave over scales 0.125 .. 1 (10 kept layers), 20 x 20 HistEq64 patches converted with
(1 / 255, 0), the 100-filter RBF model of rvm_score_model's bench-shape (make_model on the extracted vectors) with thresholds that let
about 60 % of the survivors pass each level for as long as 32 of the 4000 calibration rows remain (the rest of the levels pass everything,
so a few windows in a thousand run all 100 levels).  For n = 27 (a 3 x 3 x 3 validator grid) / 100 / 1000 / 4000 / 65536 samples drawn over all
layers, one fd_patch_rvm_evaluate_samples call per route:
  fused     FD_PATCH_FUSED=1: window list upload, k_rvm_samples, one read-back
  composed  FD_PATCH_FUSED=0: window list upload, k_window_patches in list mode, the cascade's passes and its deep kernel, one read-back
  loop      what the host layer does without the sampled call, sample by sample on the same inputs: the patch cut from the downloaded
            layer (downloaded once per frame, not timed), histeq64 on that one patch, the conversion on the host, Rvm.eval on its one
            vector.  Up to --loop-max samples; above, the loop is not run.
The routes take turns call by call inside one process (the loop fewer times: it is slow); every shape is warmed up first; every timing
is the host clock around a call that ends in the stream's synchronise.  Prints one JSON line with medians, 10th and 90th percentiles
(milliseconds) and, per n, whether the fused median lies below the composed route's 10th percentile (the dispatch rule's condition)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PW = PH = 20
SIZES = (27, 100, 1000, 4000, 65536)


def stats(t):
    t = np.array(t) * 1e3
    return dict(median=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), n=int(len(t)))


def draw_samples(pyr, layers, n, rng):
    """n samples with a window each, spread over all layers: candidates around every layer's windows, kept where the rule finds one"""
    out = np.zeros((0, 4), np.int32)
    while len(out) < n:
        cand = []
        for _ in range(2 * n):
            L = layers[int(rng.integers(len(layers)))]
            width = int(round(PW / L["scale"]))
            cand.append((int(rng.integers(0, int(L["w"] / L["scale"]) + 1)), int(rng.integers(0, int(L["h"] / L["scale"]) + 1)), width, width))
        cand = np.array(cand, np.int32)
        out = np.concatenate([out, cand[pyr.sample_windows(PW, PH, cand)[:, 3] == 1]])
    return np.ascontiguousarray(out[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--loop-max", type=int, default=4000)
    ap.add_argument("--sizes", type=str, default=",".join(str(n) for n in SIZES), help="sample counts, comma-separated")
    args = ap.parse_args()
    import torch  # noqa: F401  (the HIP runtime of the wheel first, as bench.py loads it)
    import rvm_score_model as M
    from featuredetection_amd import capi, synth
    ctx = capi.Context(0)
    frame = synth.make_frame(640, 480, seed=11)
    rng = np.random.default_rng(3)
    pyr = capi.Pyramid(ctx, octave_layers=3, min_scale=0.125, max_scale=1.0)
    pyr.update(frame)
    layers = pyr.layers()
    assert len(layers) == 10, len(layers)
    scale, shift = 1.0 / 255.0, 0.0
    pp = capi.patch_samples_params(PW, PH, capi.FD_FEATURE_HQ64, scale, shift)
    sizes = [int(v) for v in args.sizes.split(",")]
    base = draw_samples(pyr, layers, max(max(sizes), 4000), rng)
    feats, valid = capi.patch_extract_samples(ctx, pyr, pp, base[:4000])
    assert valid.all()
    m = dict(M.make_model("bench-shape", M.RBF, feats, PW, PH, M.BENCH_FILTERS), num_used=0)
    D = M.distances(m, M.kernel_values(m, feats))
    thr, alive = np.full(M.BENCH_FILTERS, -1e30, np.float32), np.ones(len(D), bool)
    for k in range(M.BENCH_FILTERS):
        if alive.sum() < 32:
            break
        thr[k] = np.float32(np.quantile(D[alive, k], 0.4))
        alive &= D[:, k] >= np.float64(thr[k])
    m["thresholds"] = thr
    rvm = capi.Rvm(ctx, m)
    limg = [pyr.layer(i) for i in range(len(layers))]   # the host layer's cached download
    result = dict(image="640x480", layers=len(layers), patch="%dx%d hq64" % (PW, PH), filters=M.BENCH_FILTERS, samples={})

    def call(route, s):
        os.environ["FD_PATCH_FUSED"] = route
        return capi.patch_rvm_evaluate_samples(ctx, pyr, pp, rvm, s)

    for n in sizes:
        s = base[:n]
        wins = pyr.sample_windows(PW, PH, s)

        def loop():
            lv, d = np.empty(n, np.int32), np.empty(n)
            for i, (l, bx, by, _) in enumerate(wins.tolist()):
                patch = limg[l][by:by + PH, bx:bx + PW][None]
                x = ctx.histeq64(patch).reshape(1, -1).astype(np.float32) * np.float32(scale) + np.float32(shift)
                a, b = rvm.eval(x)
                lv[i], d[i] = a[0], b[0]
            return lv, d
        for _ in range(args.warmup):
            call("1", s)
            call("0", s)
        _, lf, df, _ = call("1", s)
        _, lc, dc, _ = call("0", s)
        assert np.array_equal(lf, lc) and df.tobytes() == dc.tobytes()
        with_loop = n <= args.loop_max
        if with_loop:
            ll, dl = loop()
            assert np.array_equal(lf, ll) and df.tobytes() == dl.tobytes()
        tf, tc, tl = [], [], []
        for r in range(args.reps):
            for route, t in (("1", tf), ("0", tc)) if r % 2 == 0 else (("0", tc), ("1", tf)):
                t0 = time.perf_counter()
                call(route, s)
                t.append(time.perf_counter() - t0)
            if with_loop and r % max(1, args.reps // args.loop_reps) == 0 and len(tl) < args.loop_reps:
                t0 = time.perf_counter()
                loop()
                tl.append(time.perf_counter() - t0)
        row = dict(fused_ms=stats(tf), composed_ms=stats(tc), mean_exit_level=float(lf.mean()))
        row["fused_median_below_composed_p10"] = bool(row["fused_ms"]["median"] < row["composed_ms"]["p10"])
        if with_loop:
            row["loop_ms"] = stats(tl)
        result["samples"][str(n)] = row
    os.environ.pop("FD_PATCH_FUSED", None)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
