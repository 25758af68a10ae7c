#!/usr/bin/env python3
"""Times the keypoint budget on the bench's 4K image (blob_image(3840, 2160,
seed=42), 4 octaves x 5 scales), on the detection's own device list.  Three
arms alternate in one process, every step:

  a  sift_keypoint_select_device, max_total = 8192               (select_timing)
  b  the same entry point, 64 px cells, 4 per cell               (select_timing)
  c  torch on the same device and the same records: abs of interp_value,
     topk(8192), then a sort of the indices                      (events)

Arm c is timing only; its index set is compared with arm a's when the 8192nd
and the 8193rd strongest keys differ (with a tie there topk may pick another
member of the tie than the definition does).

For context the same run times orient + describe + match_features (device
times) of this image against the generator's image with another seed, on the
full lists and on the lists limited to 8192 keypoints.

Prints one JSON line: medians over --steps after --warmup.  One run on a shared
machine: compare the arms with each other, not with another day's figures."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sift-scale-space-extrema-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def feature_pass(a, b):
    """Device ms of orient + describe on both contexts and of the match a -> b; the lists lose their features first."""
    out = {}
    for name, ctx in (("query", a), ("train", b)):
        ctx.limit_keypoints()  # no limit: the same list, its orientations and descriptors dropped
        ctx.orient()
        ctx.describe()
        t = ctx.feature_timings()
        out[name + "_orient_ms"], out[name + "_describe_ms"] = t["orient_ms"], t["describe_ms"]
    rows = len(a.match_features(b))
    out["match_ms"] = a.match_timings()["match_ms"]
    out["total_ms"] = sum(out.values())
    return out, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs=2, default=(42, 43))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-total", type=int, default=8192)
    ap.add_argument("--cell-px", type=int, default=64)
    ap.add_argument("--max-per-cell", type=int, default=4)
    ap.add_argument("--context-steps", type=int, default=3, help="feature passes timed on the full lists")
    args = ap.parse_args()

    import torch
    torch.cuda.init()  # before the library's own runtime, as bench.py does
    import budget_ref as br
    import sift_amd
    from sift_amd.synth import blob_image

    L = sift_amd.lib()
    p = sift_amd.make_params(args.octaves, args.scales)
    W, H, K = args.width, args.height, args.max_total
    rows = []
    with sift_amd.Context(0) as a, sift_amd.Context(0) as b:
        kp = a.detect(blob_image(W, H, seed=args.seeds[0]), p)
        b.detect(blob_image(W, H, seed=args.seeds[1]), p)
        d_kp, n = a.device_keypoints()
        d_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_copy = torch.zeros(n * 6, dtype=torch.float64, device="cuda")  # 48-byte records: six 8-byte words
        a.copy_keypoints_device(d_copy.data_ptr(), n)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def select(bud):
            m = ctypes.c_size_t()
            rc = L.sift_keypoint_select_device(a._h, d_kp, n, W, H, ctypes.byref(bud), d_idx.data_ptr(), n,
                                               ctypes.byref(m))
            assert rc == 0, L.sift_last_error(a._h)
            return a.select_timing(), d_idx[:m.value].cpu().numpy()

        for it in range(args.warmup + args.steps):
            total_ms, idx_a = select(sift_amd.make_budget(K))
            grid_ms, idx_b = select(sift_amd.make_budget(None, args.cell_px, args.max_per_cell))
            e0.record()
            v = d_copy.view(n, 6)[:, 5].abs()
            _, top = torch.topk(v, min(K, n))
            idx_c, _ = torch.sort(top)
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                rows.append(dict(select_total_ms=total_ms, select_grid_ms=grid_ms, torch_topk_sort_ms=e0.elapsed_time(e1)))

        keys = np.sort(br.keys(kp))[::-1]
        distinct = bool(n > K and keys[K - 1] != keys[K])
        same = bool((idx_c.cpu().numpy() == idx_a).all()) if distinct or n <= K else None
        ref_ok = bool((idx_a == br.select(kp, W, H, br.budget(K))).all() and
                      (idx_b == br.select(kp, W, H, br.budget(None, args.cell_px, args.max_per_cell))).all())

        full = [feature_pass(a, b) for _ in range(1 + args.context_steps)][1:]
        full_rows = full[0][1]
        a.limit_keypoints(max_total=K)
        b.limit_keypoints(max_total=K)
        lim = [feature_pass(a, b) for _ in range(1 + args.context_steps)][1:]
        lim_rows = lim[0][1]

    out = {k: round(statistics.median(r[k] for r in rows), 4) for k in rows[0]}
    med = lambda runs: {k: round(statistics.median(r[0][k] for r in runs), 3) for k in runs[0][0]}
    out.update(image="%dx%d" % (W, H), octaves=args.octaves, scales=args.scales, seeds=list(args.seeds),
               steps=args.steps, warmup=args.warmup, n_keypoints=int(n), max_total=K, kept_total=len(idx_a),
               cell_px=args.cell_px, max_per_cell=args.max_per_cell, cells=int(np.prod(br.grid(W, H, args.cell_px))),
               kept_grid=len(idx_b), torch_over_select_total=round(out["torch_topk_sort_ms"] / out["select_total_ms"], 3),
               keys_at_quota_differ=distinct, torch_index_set_equal=same, restatement_equal=ref_ok,
               features_full=dict(med(full), query_rows=full_rows), features_limited=dict(med(lim), query_rows=lim_rows))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
