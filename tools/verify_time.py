#!/usr/bin/env python3
"""Times RANSAC homography verification on the bench's 4K image
(blob_image(3840, 2160, seed=42), 4 octaves x 5 scales) against a copy of it
shifted by a whole number of octave-top pixels (default 16 right, 8 down; the
uncovered border is mid-gray): both are detected, oriented, described and
matched both ways once, the pairs that pass ratio 0.8 and the mutual check are
selected, and every step then verifies them on the device
(sift_verify_features, K = 4096 hypotheses).

In the same process and alternating with it, every step also times a plain
torch statement of the scoring on the same points and the same K matrices: an
fp64 batched product of the matrices with the homogeneous points, then the same
comparison, chunked over the hypotheses.

Prints one JSON line and writes it to --out: medians over --steps after
--warmup of the three stage times (events around each stage's launches), the
score kernel's achieved fp64 rate -- 21 operations per pair and hypothesis,
none of them fused: the definition forbids contraction -- as a fraction of the
78.6 TFLOP/s vector fp64 peak of the MI355X spec sheet (which counts a fused
multiply-add as two, so half of it is this kernel's ceiling), and how far the
torch arm's counts are from the kernel's (its product may round differently).
One run on a shared machine: compare the two arms with each other, not with
another day's figures."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sift-scale-space-extrema-detection_amd"))

FP64_VECTOR_PEAK = 78.6e12   # AMD Instinct MI355X spec sheet, vector fp64, FMA = 2
FLOP_PER_EVAL = 21           # 12 for (u, v, w), 4 for (du, dv), 3 for the squared residual, 2 for t2 * (w * w)


def torch_score(torch, Hm, hom, X, Y, t2, chunk):
    """int64 [K]: inlier counts of Hm [K, 3, 3] over hom [3, M] -> (X, Y) [M]."""
    out = []
    for a in range(0, Hm.shape[0], chunk):
        uvw = Hm[a:a + chunk] @ hom                        # [c, 3, M]
        w = uvw[:, 2]
        du, dv = uvw[:, 0] - X * w, uvw[:, 1] - Y * w
        out.append(((w > 0) & ((du * du + dv * dv) < t2 * (w * w))).sum(dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--shift", type=int, nargs=2, default=(16, 8), help="x y, multiples of 2^(octaves-1)")
    ap.add_argument("--hypotheses", type=int, default=4096)
    ap.add_argument("--ransac-seed", type=int, default=1)
    ap.add_argument("--thresh", type=float, default=3.0)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk-mib", type=int, default=1024, help="torch arm: size of one [c, 3, M] product")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_time_4k_o4_s5.json"))
    args = ap.parse_args()
    dx, dy = args.shift
    top = 1 << (args.octaves - 1)
    if dx % top or dy % top or dx < 0 or dy < 0:
        ap.error("--shift must be non-negative multiples of %d" % top)

    import torch
    torch.cuda.init()  # before the library's own runtime, as bench.py does
    import sift_amd
    from sift_amd.synth import blob_image

    p = sift_amd.make_params(args.octaves, args.scales)
    img = blob_image(args.width, args.height, seed=args.seed)
    moved = np.full_like(img, 0.5)
    moved[:args.height - dy, :args.width - dx] = img[dy:, dx:]   # a point (x, y) of img is (x - dx, y - dy) here
    K = args.hypotheses
    rows = []
    with sift_amd.Context(0) as a, sift_amd.Context(0) as b:
        for ctx, im in ((a, img), (b, moved)):
            ctx.detect(im, p)
            ctx.orient()
            ctx.describe()
        fwd, rev = a.match_features(b), b.match_features(a)
        pairs = a.select_matches(fwd, rev, args.ratio)
        M = len(pairs)
        pts = a.pair_points(b, pairs)

        dev = torch.device("cuda")
        xy = torch.from_numpy(pts.view(np.float64).reshape(-1, 4).copy()).to(dev)
        hom = torch.stack([xy[:, 0], xy[:, 1], torch.ones_like(xy[:, 0])])       # [3, M]
        X, Y = xy[:, 2], xy[:, 3]
        chunk = max(1, (args.chunk_mib << 20) // (8 * 3 * max(M, 1)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t2 = args.thresh * args.thresh

        diff = None
        for it in range(args.warmup + args.steps):
            H, best, inl = a.verify_features(b, pairs, K, args.ransac_seed, args.thresh)
            t = a.verify_timings()
            if it == 0:
                Hs, counts = a.homography_hypotheses()
                Hm = torch.from_numpy(Hs.copy()).to(dev)
            e0.record()
            tc = torch_score(torch, Hm, hom, X, Y, t2, chunk)
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                rows.append(dict(t, torch_score_ms=e0.elapsed_time(e1)))
            if diff is None:
                d = np.abs(tc.cpu().numpy() - np.maximum(counts, 0))[counts >= 0]
                diff = dict(torch_counts_equal=int((d == 0).sum()), torch_counts_max_abs_diff=int(d.max(initial=0)))

    out = {k: round(statistics.median(r[k] for r in rows), 4) for k in rows[0]}
    flop = float(FLOP_PER_EVAL) * K * M
    rate = flop / (out["score_ms"] * 1e-3) if out["score_ms"] > 0 else 0.0
    err = float(np.abs(H - np.array([[1.0, 0, -dx], [0, 1.0, -dy], [0, 0, 1.0]])).max()) if best >= 0 else None
    out.update(image="%dx%d" % (args.width, args.height), octaves=args.octaves, scales=args.scales, seed=args.seed,
               shift=[dx, dy], steps=args.steps, warmup=args.warmup, ratio=args.ratio, pairs=M, hypotheses=K,
               valid_hypotheses=int((counts >= 0).sum()), ransac_seed=args.ransac_seed, thresh=args.thresh,
               best_hypothesis=best, inliers=len(inl), model_max_abs_error=err,
               evaluations=K * M, fp64_flop_per_s=round(rate, 1),
               fp64_vector_peak_fraction=round(rate / FP64_VECTOR_PEAK, 4), fp64_peak_source="spec sheet",
               torch_over_score=round(out["torch_score_ms"] / out["score_ms"], 3) if out["score_ms"] > 0 else None,
               torch_chunk_hypotheses=chunk, **diff)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
