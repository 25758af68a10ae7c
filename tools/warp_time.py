#!/usr/bin/env python3
"""Times the homography warp (sift_warp_gray_device, sift_warp_rgba_device,
bilinear) on the bench's 4K image (blob_image(3840, 2160, seed=42)), destination
and source both 3840 x 2160, through three maps:
  identity   every pixel valid, gx = gy = 1;
  shift      the inverse of the (16, 8) shift of tools/verify_time.py;
  rot5       a 5-degree rotation about the centre with a mild perspective row.
The RGBA source is the gray image's display bytes in R, G, B with A = 255.

Beside each arm, in the same process and alternating with it, two yardsticks:
  copy   a device-to-device copy of one image (torch's Tensor.copy_ of a
         contiguous tensor, a hipMemcpyAsync): it reads the source's bytes and
         writes the destination's, the byte floor on that machine that day;
  torch  torch.nn.functional.grid_sample (fp32, bilinear, align_corners=True,
         zeros padding) over a grid built beforehand from the same map, on the
         fp32 image (RGBA: four fp32 channels; the conversion from bytes and
         the grid's construction are not timed).  What a caller would otherwise
         use; its result differs in the last bits and is reported, not compared.

The warp is timed four times per step: the full product (mask and count), with
the count alone, bare (neither), and bare in nearest mode: one load and no
interpolation on the same coordinates, which separates the coordinate
arithmetic from the rest.  Times are device times: the library's events around
its kernels, torch events around the yardsticks.  Prints one JSON line and writes it to --out: medians over
--steps after --warmup and the ratios.  One run on a shared machine: compare
the arms with each other, not with another day's figures."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sift-scale-space-extrema-detection_amd"))


def maps(w, h, inverse):
    t = np.deg2rad(5.0)
    c, s = np.cos(t), np.sin(t)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    rot = np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [2e-5, -1e-5, 1.0]])
    return {"identity": np.eye(3), "shift": inverse([[1, 0, -16], [0, 1, -8], [0, 0, 1]]), "rot5": rot}


def sampling_grid(torch, m, w, h, dev):
    """grid_sample's normalised grid [1, h, w, 2] of the map m (fp64 on the host, then fp32)."""
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        ww = m[2, 0] * X + m[2, 1] * Y + m[2, 2]
        sx = (m[0, 0] * X + m[0, 1] * Y + m[0, 2]) / ww
        sy = (m[1, 0] * X + m[1, 1] * Y + m[1, 2]) / ww
    g = np.stack([2 * sx / (w - 1) - 1, 2 * sy / (h - 1) - 1], axis=-1).astype(np.float32)
    return torch.from_numpy(g[None]).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_time_4k.json"))
    args = ap.parse_args()
    W, H = args.width, args.height

    import torch
    import torch.nn.functional as F
    torch.cuda.init()  # before the library's own runtime, as bench.py does
    import sift_amd
    from sift_amd.synth import blob_image

    dev = torch.device("cuda")
    L = sift_amd.lib()
    img = blob_image(W, H, seed=args.seed)
    byte = np.clip(np.floor(img.astype(np.float64) * 255 + 0.5), 0, 255).astype(np.uint8)
    rgba = np.stack([byte, byte, byte, np.full_like(byte, 255)], axis=-1)
    src = {"gray": torch.from_numpy(img).to(dev), "rgba": torch.from_numpy(rgba).to(dev)}
    dst = {k: torch.zeros_like(v) for k, v in src.items()}
    tin = {"gray": src["gray"][None, None].contiguous(),
           "rgba": src["rgba"].permute(2, 0, 1)[None].float().contiguous()}
    d_mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    fill4 = np.zeros(4, dtype=np.uint8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dp = ctypes.POINTER(ctypes.c_double)
    arms = maps(W, H, sift_amd.homography_inverse)
    grids = {name: sampling_grid(torch, m, W, H, dev) for name, m in arms.items()}
    torch.cuda.synchronize()

    def warp(ctx, kind, m, full, mode=sift_amd.WARP_BILINEAR, count=None):
        count = full if count is None else count
        n = ctypes.c_size_t()
        mm = np.ascontiguousarray(m, dtype=np.float64).reshape(9)
        common = (W, H, W * (4 if kind == "rgba" else 1))
        fill = fill4.ctypes.data_as(ctypes.c_void_p) if kind == "rgba" else ctypes.c_float(0.0)
        fn = L.sift_warp_rgba_device if kind == "rgba" else L.sift_warp_gray_device
        rc = fn(ctx._h, src[kind].data_ptr(), *common, mm.ctypes.data_as(dp), mode, fill,
                dst[kind].data_ptr(), *common, d_mask.data_ptr() if full else None, ctypes.byref(n) if count else None)
        if rc:
            raise RuntimeError("%s: %d" % (fn.__name__, rc))
        return ctx.warp_timing(), n.value

    def timed(f):
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    rows, info = {}, {}
    with sift_amd.Context(0) as ctx:
        for it in range(args.warmup + args.steps):
            for name, m in arms.items():
                for kind in ("gray", "rgba"):
                    full_ms, n_valid = warp(ctx, kind, m, True)
                    near_ms, _ = warp(ctx, kind, m, False, sift_amd.WARP_NEAREST)
                    count_ms, _ = warp(ctx, kind, m, False, count=True)
                    bare_ms, _ = warp(ctx, kind, m, False)
                    ours = dst[kind].clone() if it == 0 else None
                    copy_ms, _ = timed(lambda: dst[kind].copy_(src[kind]))
                    torch_ms, ref = timed(lambda: F.grid_sample(tin[kind], grids[name], mode="bilinear",
                                                                padding_mode="zeros", align_corners=True))
                    if it == 0:
                        if kind == "gray":
                            d = (ours - ref[0, 0]).abs()
                        else:
                            d = (ours.float() - ref[0].permute(1, 2, 0)).abs()
                        inner = d[8:-8, 8:-8]   # away from the border, where the two differ by the padding rule
                        info[(name, kind)] = dict(n_valid=int(n_valid), valid_fraction=round(n_valid / (W * H), 4),
                                                  torch_median_abs_diff=float(inner.median()))
                    del ref
                    if it >= args.warmup:
                        rows.setdefault((name, kind), []).append(
                            dict(warp_ms=full_ms, warp_count_only_ms=count_ms, warp_bare_ms=bare_ms,
                                 nearest_bare_ms=near_ms, copy_ms=copy_ms, torch_ms=torch_ms))

    out = dict(image="%dx%d" % (W, H), seed=args.seed, steps=args.steps, warmup=args.warmup, mode="bilinear",
               bytes_per_image={"gray": W * H * 4, "rgba": W * H * 4}, arms={})
    for (name, kind), rs in rows.items():
        a = {k: round(statistics.median(r[k] for r in rs), 4) for k in rs[0]}
        a["warp_over_copy"] = round(a["warp_ms"] / a["copy_ms"], 3) if a["copy_ms"] > 0 else None
        a["bare_over_copy"] = round(a["warp_bare_ms"] / a["copy_ms"], 3) if a["copy_ms"] > 0 else None
        a["torch_over_warp"] = round(a["torch_ms"] / a["warp_ms"], 3) if a["warp_ms"] > 0 else None
        a["bytes_per_s"] = round(2 * W * H * 4 / (a["warp_bare_ms"] * 1e-3), 1) if a["warp_bare_ms"] > 0 else None
        a.update(info[(name, kind)])
        out["arms"]["%s_%s" % (name, kind)] = a
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
