#!/usr/bin/env python3
"""Times descriptor matching on the bench's 4K image (blob_image(3840, 2160,
seed=42), 4 octaves x 5 scales) against the same generator's image with
another seed: both are detected, oriented and described once, then every step
matches the first image's descriptors against the second's on the device
(sift_match_features), matches the other way, and selects the mutual pairs
that pass the ratio test.

In the same process and alternating with it, every step also times a plain
torch statement of the same match on the same descriptors: chunked fp32 matmul
of the shifted rows (exact: every value stays below 2^24), the two norms, and
topk(2, largest=False) per chunk.

Prints one JSON line: medians over --steps after --warmup of the device times
(events around each side's launches), the achieved int8 rate 2 * 128 * n_q *
n_t / match_ms as a fraction of the ~5 POPS dense int8 peak, and whether the
two arms agree on every distance.  One run on a shared machine: compare the
two arms with each other, not with another day's figures."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sift-scale-space-extrema-detection_amd"))

INT8_PEAK_OPS = 5.0e15


def torch_match(torch, q, qn, t, tn, t_ok, chunk):
    """(d2 [n_q, 2] float32, index [n_q, 2]) of the two nearest unmasked train rows."""
    d2, idx = [], []
    pen = torch.where(t_ok, tn, torch.full_like(tn, float("inf")))
    for a in range(0, q.shape[0], chunk):
        d = (qn[a:a + chunk, None] + pen[None, :]) - 2.0 * (q[a:a + chunk] @ t.T)
        v, i = torch.topk(d, 2, dim=1, largest=False)
        d2.append(v)
        idx.append(i)
    return torch.cat(d2), torch.cat(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs=2, default=(42, 43))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--chunk-mib", type=int, default=2048, help="torch arm: distance chunk size")
    args = ap.parse_args()

    import torch
    torch.cuda.init()  # before the library's own runtime, as bench.py does
    import sift_amd
    from sift_amd.synth import blob_image

    p = sift_amd.make_params(args.octaves, args.scales)
    rows = []
    with sift_amd.Context(0) as a, sift_amd.Context(0) as b:
        feats = []
        for ctx, seed in ((a, args.seeds[0]), (b, args.seeds[1])):
            ctx.detect(blob_image(args.width, args.height, seed=seed), p)
            ctx.orient()
            feats.append(ctx.describe())
        (da, oka), (db, okb) = feats
        nq, nt = len(da), len(db)

        dev = torch.device("cuda")
        q = (torch.from_numpy(da.astype(np.int16)).to(dev) - 128).float()
        t = (torch.from_numpy(db.astype(np.int16)).to(dev) - 128).float()
        qn, tn = (q * q).sum(1), (t * t).sum(1)
        t_ok = torch.from_numpy(okb).to(dev)
        chunk = max(1, (args.chunk_mib << 20) // (4 * max(nt, 1)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        same = None
        for it in range(args.warmup + args.steps):
            fwd = a.match_features(b)
            match_ms = a.match_timings()["match_ms"]
            rev = b.match_features(a)
            pairs = a.select_matches(fwd, rev, args.ratio)
            select_ms = a.match_timings()["select_ms"]
            e0.record()
            d2, _ = torch_match(torch, q, qn, t, tn, t_ok, chunk)
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                rows.append(dict(match_ms=match_ms, rev_match_ms=b.match_timings()["match_ms"], select_ms=select_ms,
                                 torch_ms=e0.elapsed_time(e1)))
            if same is None:  # the arms agree on every distance of the described queries
                got = np.stack([fwd["d2_best"], fwd["d2_second"]], 1)[oka]
                same = bool((d2.cpu().numpy()[oka].astype(np.int64) == got).all())

    out = {k: round(statistics.median(r[k] for r in rows), 4) for k in rows[0]}
    ops = 2.0 * 128 * nq * nt
    out.update(image="%dx%d" % (args.width, args.height), octaves=args.octaves, scales=args.scales,
               seeds=list(args.seeds), steps=args.steps, warmup=args.warmup, n_query=nq, n_train=nt,
               described=[int(oka.sum()), int(okb.sum())], pairs=len(pairs), ratio=args.ratio,
               int8_ops_per_s=round(ops / (out["match_ms"] * 1e-3), 1),
               int8_peak_fraction=round(ops / (out["match_ms"] * 1e-3) / INT8_PEAK_OPS, 4),
               torch_over_match=round(out["torch_ms"] / out["match_ms"], 3), torch_d2_equal=same,
               torch_chunk_rows=chunk)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
