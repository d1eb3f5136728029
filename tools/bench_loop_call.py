#!/usr/bin/env python3
"""Host cost of one device-loop call: wall time of a 1-step dsd_sample call (checks, binding, one forward of the tiny DSUnetModel
of tests/golden/model.npz on 2 x 1 x 32 x 32, one update, finish, synchronise) through the Python API.  The network is a few
hundred microseconds of device work, so what the host does per call shows.  Prints one JSON line: the median of every repeat
(--repeats of --calls calls each) in microseconds, their median and their spread.  Compare two checkouts run alternately."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()

import torch
from diffusion_models_dsdiff_amd import _lib
from diffusion_models_dsdiff_amd._sched import run_device_loop
from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
from diffusion_models_dsdiff_amd.UNet_DS_Diff.model import DSUnetModel
from util import golden, fixture_params, randn, cond_image

_lib.require_gpu(0)
gm = golden("model")
unet = DSUnetModel(**json.loads(str(gm["tiny_cfg"])))
unet.load_state_dict(fixture_params(gm, "tiny"), strict=True)
unet.cuda()
shape = (2, 1, 32, 32)
xT, c = randn(shape, 12).cuda(), cond_image(shape, 11).cuda()
sched = create_gaussian_diffusion(steps=1000, timestep_respacing="8")._schedule(True, 0.5, True)


def call():
    t0 = time.perf_counter()
    run_device_loop(unet, sched, xT, c, seed=5, n_steps=1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


for _ in range(50):
    call()
medians = [statistics.median(call() for _ in range(args.calls)) for _ in range(args.repeats)]
print(json.dumps({"label": args.label, "calls": args.calls, "us_per_call_repeats": [round(m, 2) for m in medians],
                  "us_per_call": round(statistics.median(medians), 2), "spread_us": round(max(medians) - min(medians), 2)}))
