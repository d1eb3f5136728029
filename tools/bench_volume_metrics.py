#!/usr/bin/env python3
"""The volume metric table measured on one GPU, one process: hipEvent medians of --repeats calls after --warmup untimed ones, the
minimum and maximum beside each median.

  op      the device path of metrics.volume_metrics as a user calls it (dsd_op_volume_metrics: scratch allocation, three passes
          with their folds, the selection, the release, then the one read-back; all of it inside the events) at 155 x 240 x 240
          with an ellipsoid mask (one BraTS volume) and at 24 x 100 x 90, with win = 0 (what the metric table asks for) and with
          win = 9 (the reference's stand-alone ssim on top), fp32 voxels.
  host    calibration, on the same box: the same columns through the float64 numpy functions of host_io (nrmse, mape, smape, logac,
          medsymac, psnr; and ssim for win = 9), each volume --host-runs times on the host clock.
  bytes   the bytes the table's passes read and write (three reads of both volumes and the mask, the l array written once and read by
          the twelve histogram passes) over the op's median, beside the HBM rate.

    python tools/bench_volume_metrics.py --json profiles/volume_metrics_bench.json
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
ap.add_argument("--host-runs", type=int, default=3)
ap.add_argument("--hbm-bytes-per-s", type=float, default=8.0e12, help="the HBM3E peak of an MI355X")
ap.add_argument("--json")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffusion_models_dsdiff_amd import _lib, host_io  # noqa: E402
from diffusion_models_dsdiff_amd.metrics import _volume_device  # noqa: E402

SHAPES = [(155, 240, 240), (24, 100, 90)]
COLUMNS = ("nrmse", "mape", "smape", "logac", "medsymac", "psnr")


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


def volume(shape, seed):
    """A smooth volume plus noise under an ellipsoid mask, zero outside a slightly larger one; fp32 values."""
    D, H, W = shape
    r = np.random.RandomState(seed)
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float32)
    q = ((z - D / 2 + 0.3) / (0.42 * D)) ** 2 + ((y - H / 2 + 0.2) / (0.40 * H)) ** 2 + ((x - W / 2 + 0.1) / (0.38 * W)) ** 2
    t = (600. + 400. * np.cos(z / 9.) * np.sin(y / 17.) * np.cos(x / 23.)).astype(np.float32)
    p = (t + 25. * r.randn(D, H, W)).astype(np.float32)
    outer = q <= 1.25
    return np.where(outer, t, 0).astype(np.float64), np.where(outer, p, 0).astype(np.float64), q <= 1.0


def main():
    name, ncu, _ = _lib.require_gpu(0)
    res = {"gpu": name, "repeats": args.repeats, "warmup": args.warmup, "hbm_bytes_per_s": args.hbm_bytes_per_s, "cases": {}}
    S = _lib.VOLUME_SLOTS.index
    for shape in SHAPES:
        t, p, mask = volume(shape, 5)
        td, pd, md = (torch.from_numpy(a).cuda() for a in (t.astype(np.float32), p.astype(np.float32), mask))
        n = int(np.prod(shape))
        r = {"voxels": n, "n_M": int(mask.sum())}
        for win in (0, 9):
            r[f"op_win{win}"] = events(lambda: _volume_device(td, pd, md, win), args.warmup, args.repeats)
        host, host_ssim, vals = [], [], {}
        for _ in range(args.host_runs):
            t0 = time.perf_counter()
            vals = {k: getattr(host_io, k)(t, p, mask) for k in COLUMNS}
            host.append((time.perf_counter() - t0) * 1e3)
        for _ in range(max(1, args.host_runs - 1)):
            t0 = time.perf_counter()
            vals["ssim3d"] = host_io.ssim(t, p, mask)
            host_ssim.append((time.perf_counter() - t0) * 1e3)
        r["host_numpy_float64_six_columns"] = stats(host)
        r["host_scipy_float64_ssim_win9"] = stats(host_ssim)
        raw = _volume_device(td, pd, md, 9)
        r["value_check"] = {k: float(abs(raw[S(k)] / vals[k] - 1)) for k in COLUMNS}
        r["value_check"]["ssim3d_abs"] = float(abs(raw[S("ssim3d")] - vals["ssim3d"]))
        nbytes = 3 * (2 * 4 + 1) * n + 8 * n + 12 * 8 * n
        r["table_bytes_read_and_written"] = nbytes
        r["achieved_bytes_per_s"] = round(nbytes / (r["op_win0"]["median_ms"] * 1e-3), 1)
        r["share_of_hbm_rate"] = round(r["achieved_bytes_per_s"] / args.hbm_bytes_per_s, 5)
        r["host_over_op_win0"] = round(r["host_numpy_float64_six_columns"]["median_ms"] / r["op_win0"]["median_ms"], 2)
        res["cases"]["x".join(map(str, shape))] = r
        print(json.dumps({"case": "x".join(map(str, shape)), **r}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
