#!/usr/bin/env python3
"""The validation metrics measured on one GPU, one process: hipEvent medians of --repeats calls after --warmup untimed ones, the
minimum and maximum beside each median.

  op      the device path of metrics.image_metrics as a user calls it (dsd_op_image_metrics: scratch allocation, the launch
          sequence, the release, then the one read-back; all of it inside the events, and once more on the host clock) at
          16x1x256x256 with scales 1 and 5 and at 155x1x240x240 (one BraTS volume's axial slices) with scales 5.
  torch   calibration, on no product path: the same SSIM written in torch-eager fp32 ops on the same GPU the way MONAI writes
          it (a grouped conv2d with the 11 x 11 outer-product kernel; the pyramid by F.avg_pool2d).  It is fp32: it misses the
          1e-10 the device kernel is held to by four to six decades.
  host    calibration: the float64 scipy path (host_io.ssim_scale_table) on ONE slice, times the slice count.
  bytes   the bytes the algorithm needs (both images read once as fp32) over the op's median, beside the HBM rate.
  step    one denoising step of a batch of 16 at 256 x 256 from the committed bench figure (profiles/r03_bench_1gpu.json,
          ms_per_step), so that the cost of a validation pass can be read beside even a 2-step sample.

    python tools/bench_image_metrics.py --json profiles/image_metrics_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--hbm-bytes-per-s", type=float, default=8.0e12, help="the HBM3E peak of an MI355X")
ap.add_argument("--json")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffusion_models_dsdiff_amd import _lib, host_io  # noqa: E402
from diffusion_models_dsdiff_amd.metrics import MS_SSIM_BETAS, _device  # noqa: E402

SHAPES = [((16, 1, 256, 256), 1), ((16, 1, 256, 256), 5), ((155, 1, 240, 240), 5)]


def stats(v, unit="ms"):
    return {f"median_{unit}": round(statistics.median(v), 4), f"min_{unit}": round(min(v), 4), f"max_{unit}": round(max(v), 4), "runs": len(v)}


def events(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def torch_form(p, t, scales, data_range):
    """MONAI's formulation in torch-eager fp32, five scales the torchmetrics way; returns ssim [B] (scales 1) or ms_ssim [B]."""
    C = p.shape[1]
    d = torch.arange(11, dtype=torch.float32, device=p.device) - 5
    g = torch.exp(-(d / 1.5) ** 2 / 2)
    g = g / g.sum()
    k = torch.outer(g, g)[None, None].expand(C, 1, 11, 11).contiguous()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vals = []
    for s in range(scales):
        blur = lambda a: F.conv2d(a, k, groups=C)
        mx, my = blur(p), blur(t)
        sx, sy, sxy = blur(p * p) - mx * mx, blur(t * t) - my * my, blur(p * t) - mx * my
        cs = (2 * sxy + c2) / (sx + sy + c2)
        full = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
        vals.append((full.flatten(1).mean(1), cs.flatten(1).mean(1)))
        if s < scales - 1:
            p, t = F.avg_pool2d(p, 2), F.avg_pool2d(t, 2)
    if scales == 1:
        return vals[0][0]
    b = torch.tensor(MS_SSIM_BETAS, device=p.device)
    return torch.prod(torch.stack([v[1] for v in vals[:-1]] + [vals[-1][0]], 1).clamp_min(0) ** b, 1)


def main():
    name, ncu, _ = _lib.require_gpu(0)
    step = json.load(open(os.path.join(ROOT, "profiles", "r03_bench_1gpu.json")))["ms_per_step"]
    res = {"gpu": name, "repeats": args.repeats, "warmup": args.warmup, "hbm_bytes_per_s": args.hbm_bytes_per_s,
           "denoising_step_ms_batch16_256": step, "denoising_step_source": "profiles/r03_bench_1gpu.json ms_per_step", "cases": {}}
    g = torch.Generator(device="cuda").manual_seed(3)
    for shape, scales in SHAPES:
        t = torch.rand(shape, device="cuda", generator=g) * 2 - 1
        p = (t + 0.1 * torch.randn(shape, device="cuda", generator=g)).clamp_(-1, 1)
        r = {"op": events(lambda: _device(p, t, scales, 2.0, None), args.warmup, args.repeats),
             "torch_eager_fp32": events(lambda: torch_form(p, t, scales, 2.0), args.warmup, args.repeats)}
        wall = []
        for _ in range(args.repeats):                                  # the whole call as a user sees it, read-back included
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scale, _elem = _device(p, t, scales, 2.0, None)
            wall.append((time.perf_counter() - t0) * 1e3)
        r["op_with_read_back_host_clock"] = stats(wall)
        p0, t0_ = p[0].cpu().numpy(), t[0].cpu().numpy()
        host = []
        for _ in range(4):                                             # the first run (scipy's import, cold pages) is not kept
            t0 = time.perf_counter()
            one = host_io.ssim_scale_table(p0, t0_, scales, 2.0)
            host.append((time.perf_counter() - t0) * 1e3)
        host_ms = statistics.median(host[1:])
        r["host_scipy_float64"] = {"one_slice_ms": round(host_ms, 3), "min_ms": round(min(host[1:]), 3), "max_ms": round(max(host[1:]), 3),
                                   "runs": 3, "slices": shape[0], "all_slices_ms": round(host_ms * shape[0], 2)}
        key = "ssim" if scales == 1 else "ms_ssim"
        ours = scale[:, 0, 0] if scales == 1 else np.prod(np.maximum(np.concatenate([scale[:, :-1, 1], scale[:, -1:, 0]], 1), 0) ** np.asarray(MS_SSIM_BETAS), 1)
        r["value_check"] = {"what": key, "op_vs_host_slice0": float(abs(scale[0] - one).max()),
                            "torch_fp32_vs_op_max": float(np.abs(torch_form(p, t, scales, 2.0).double().cpu().numpy() - ours).max())}
        nbytes = 2 * 4 * int(np.prod(shape))
        r["algorithmic_bytes"] = nbytes
        r["achieved_bytes_per_s"] = round(nbytes / (r["op"]["median_ms"] * 1e-3), 1)
        r["share_of_hbm_rate"] = round(r["achieved_bytes_per_s"] / args.hbm_bytes_per_s, 5)
        r["op_over_one_denoising_step"] = round(r["op"]["median_ms"] / step, 6)
        res["cases"]["x".join(map(str, shape)) + f"_scales{scales}"] = r
        print(json.dumps({"case": "x".join(map(str, shape)), "scales": scales, **{k: v for k, v in r.items()}}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
