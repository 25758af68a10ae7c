#!/usr/bin/env python3
"""Times the orientation and descriptor stages on the bench's 4K image
(blob_image(3840, 2160, seed=42), 4 octaves x 5 scales): detection, then
sift_orient and sift_describe with their results kept on the device.  Prints
one JSON line; the stage times are device times (events around each stage's
launches), medians over --steps detections after --warmup."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sift-scale-space-extrema-detection_amd"))

import sift_amd  # noqa: E402
from sift_amd.synth import blob_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    img = blob_image(args.width, args.height, seed=42)
    p = sift_amd.make_params(args.octaves, args.scales)
    rows = []
    with sift_amd.Context(0) as ctx:
        L, h = ctx._L, ctx._h
        n, nd = ctypes.c_size_t(), ctypes.c_size_t()
        for it in range(args.warmup + args.steps):
            n_kp = len(ctx.detect(img, p))
            t = ctx.timings()
            t0 = time.perf_counter()
            ctx._check(L.sift_orient(h, None, 0, ctypes.byref(n)), "sift_orient")
            t1 = time.perf_counter()
            ctx._check(L.sift_describe(h, None, None, 0, ctypes.byref(n), ctypes.byref(nd)), "sift_describe")
            t2 = time.perf_counter()
            f = ctx.feature_timings()
            if it >= args.warmup:
                rows.append(dict(detect_device_ms=t["gauss_dog_ms"] + t["extrema_ms"] + t["refine_ms"],
                                 orient_ms=f["orient_ms"], describe_ms=f["describe_ms"],
                                 orient_wall_ms=1e3 * (t1 - t0), describe_wall_ms=1e3 * (t2 - t1)))
    out = {k: round(statistics.median(r[k] for r in rows), 4) for k in rows[0]}
    out.update(image="%dx%d" % (args.width, args.height), octaves=args.octaves, scales=args.scales, steps=args.steps,
               keypoints=n_kp, records=n.value, described=nd.value)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
