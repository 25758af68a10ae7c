#!/usr/bin/env python3
"""Times guided descriptor matching against the brute-force match on the bench's
4K image (blob_image(3840, 2160, seed=42), 4 octaves x 5 scales) and a copy of
it shifted by a whole number of octave-top pixels (default 16 right, 8 down; the
uncovered border is mid-gray), the case of tools/verify_time.py.

Both images are detected, oriented and described once.  One brute-force match
each way, the mutual pairs that pass ratio 0.8, the RANSAC and its refit
(sift_verify_features_refit) give the model.  Every step then runs, in one
process and alternating: sift_match_features (every train row for every query
row), and sift_match_features_guided with the refitted model at each --radii
(default 4 and 16 pixels).

Prints one JSON line and writes it to --out: medians over --steps after
--warmup of the brute-force match_ms and of each radius's grid_ms and match_ms
(events around the launches), the grid and the three sums of each radius, the
pairs sift_match_select accepts from each arm at the same ratio without a mutual
check, the fraction of the brute-force arm's accepted pairs that the guided arm
accepts with the same train row, an estimate of the bytes the guided kernels
move (from the sums: 16 per visited row, 136 per candidate, 161 per query row,
and for the filing 177 read and 152 written per train row plus 12 per cell),
and brute / guided.  One run on a shared machine: compare the arms with each
other, not with another day's figures."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sift-scale-space-extrema-detection_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--shift", type=int, nargs=2, default=(16, 8), help="x y, multiples of 2^(octaves-1)")
    ap.add_argument("--radii", type=float, nargs="+", default=(4.0, 16.0))
    ap.add_argument("--hypotheses", type=int, default=4096)
    ap.add_argument("--ransac-seed", type=int, default=1)
    ap.add_argument("--thresh", type=float, default=3.0)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_time_4k_o4_s5.json"))
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
    brute_rows, guided_rows = [], {r: [] for r in args.radii}
    with sift_amd.Context(0) as a, sift_amd.Context(0) as b:
        described = []
        for ctx, im in ((a, img), (b, moved)):
            ctx.detect(im, p)
            ctx.orient()
            described.append(int(ctx.describe()[1].sum()))
        fwd, rev = a.match_features(b), b.match_features(a)
        mutual = a.select_matches(fwd, rev, args.ratio)
        H, best, rounds, inl = a.verify_features_refit(b, mutual, args.hypotheses, args.ransac_seed, args.thresh)
        if best < 0:
            raise RuntimeError("the RANSAC found no model")
        nq, nt = len(fwd), len(rev)
        for it in range(args.warmup + args.steps):
            fwd = a.match_features(b)
            if it >= args.warmup:
                brute_rows.append(a.match_timings()["match_ms"])
            for r in args.radii:
                rec = a.match_features_guided(b, H, r)
                if it >= args.warmup:
                    guided_rows[r].append(a.guided_timings())
        brute_pairs = a.select_matches(fwd, None, args.ratio)
        brute_ms = statistics.median(brute_rows)
        radii = []
        for r in args.radii:
            rec = a.match_features_guided(b, H, r)
            info = a.guided_info()
            pairs = a.select_matches(rec, None, args.ratio)
            same = np.isin(brute_pairs["query"], pairs["query"])
            same[same] = rec["best"][brute_pairs["query"][same]] == brute_pairs["train"][same]
            grid_ms = statistics.median(t["grid_ms"] for t in guided_rows[r])
            match_ms = statistics.median(t["match_ms"] for t in guided_rows[r])
            cells = info["ncx"] * info["ncy"]
            moved_bytes = (16 * info["n_visited"] + 136 * info["n_candidates"] + 161 * nq + (177 + 152) * nt +
                           12 * cells)
            radii.append(dict(info, radius=r, grid_ms=round(grid_ms, 4), match_ms=round(match_ms, 4),
                              guided_ms=round(grid_ms + match_ms, 4), pairs=len(pairs),
                              brute_pairs_kept=round(float(same.mean()), 4) if len(same) else None,
                              visited_per_query=round(info["n_visited"] / max(info["n_projected"], 1), 2),
                              candidates_per_query=round(info["n_candidates"] / max(info["n_projected"], 1), 2),
                              bytes_moved_estimate=int(moved_bytes),
                              brute_over_guided=round(brute_ms / (grid_ms + match_ms), 2)))

    err = float(np.abs(H - np.array([[1.0, 0, -dx], [0, 1.0, -dy], [0, 0, 1.0]])).max())
    out = dict(image="%dx%d" % (args.width, args.height), octaves=args.octaves, scales=args.scales, seed=args.seed,
               shift=[dx, dy], steps=args.steps, warmup=args.warmup, ratio=args.ratio, n_query=nq, n_train=nt,
               described=described, model_pairs=len(mutual), model_inliers=len(inl), model_rounds=rounds,
               model_max_abs_error=err, brute_match_ms=round(brute_ms, 4), brute_pairs=len(brute_pairs),
               brute_descriptor_pairs=nq * nt, radii=radii)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
