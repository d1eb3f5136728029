#!/usr/bin/env python3
"""Cross-attention / vector conditioning in the latent device loops, measured on one GPU with synthetic weights.

The bench-size latent UNetModel of tools/workloads.py (320 channels, 64x64x6 input = 3 state + 3 'concat' channels, attention at
ds 1/2/4), built without and with spatial transformers (context 77 x 768, 'hybrid'), batch 16, bf16x6:
  - ms per network evaluation of both builds (UNetModel.forward);
  - the 20-step DDIM (eta 0) device loop against the per-step loop (network call + dsd_op_sampler_update), both builds;
  - with --baseline FILE (repeatable): the 'concat'-only device loop of this build over the same loop of another build's
    library, whose lines were written by `DSD_LIBRARY=<that build's libdsdiff.so> python tools/bench_cond_keys.py --concat-only
    --json FILE` on the same machine, run in turn with this one.  The ratio is recorded, not asserted.  (A library from before
    the loops took one entry point each no longer matches the binding's loop signatures: run that build from its own checkout.)
Every timed run follows one untimed run of the same loop; the loops alternate; hipEvents; medians of --repeats runs.

    python tools/bench_cond_keys.py [--batch 16] [--steps 20] [--repeats 3] [--concat-only] [--baseline other.json ...] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNET = dict(image_size=64, in_channels=6, out_channels=3, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2,
            channel_mult=[1, 2, 4, 4], num_head_channels=64, use_new_attention_order=True)
TOKENS, CTX = 77, 768


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def alternate(fns, repeats):
    """{name: [ms]}: one untimed run of each, then ``repeats`` rounds over all of them in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[1])
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--concat-only", action="store_true")
    ap.add_argument("--baseline", action="append", default=[])
    ap.add_argument("--json")
    args = ap.parse_args()
    from workloads import fill_
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd._sched import Conditioning, run_device_loop, sampler_update
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DDPM
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    B = args.batch
    g = torch.Generator().manual_seed(2030)
    xT = torch.randn(B, 3, 64, 64, generator=g).cuda()
    cc = torch.randn(B, 3, 64, 64, generator=g).cuda()
    ctx = torch.randn(B, TOKENS, CTX, generator=g).cuda()
    sm = DDIMSampler(DDPM(timesteps=1000, parameterization="eps"))
    sm.make_schedule(args.steps, ddim_eta=0.0, verbose=False)
    sched = sm._schedule(False, True)
    res = {"workload": f"latent UNetModel 320 ch, 64x64x6, batch {B}, bf16x6; {args.steps}-step DDIM eta 0; context {TOKENS}x{CTX}",
           "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH)}
    builds = {"concat": dict(UNET)}
    if not args.concat_only:
        builds["hybrid"] = dict(UNET, use_spatial_transformer=True, transformer_depth=1, context_dim=CTX)
    for name, params in builds.items():
        unet = fill_(UNetModel(**params), 2031)
        context = ctx if name == "hybrid" else None
        cond = Conditioning(cc, ctx, None) if name == "hybrid" else cc
        t = torch.full((B,), 500.0).cuda()
        x_in = torch.cat([xT, cc], 1).contiguous()

        def host():
            x = xT.clone()
            for k in range(sched.steps):
                out = unet(torch.cat([x, cc], 1), torch.full((B,), float(sched.t_model[k]), device="cuda"), context=context)
                sampler_update(sched, k, out, x, None, seed=1)
            return x

        fns = {"device_loop_ms": lambda: run_device_loop(unet, sched, xT, cond, seed=1)}
        if not args.concat_only:
            fns.update({"evaluation_ms": lambda: unet(x_in, t, context=context), "per_step_loop_ms": host})
        ms = alternate(fns, args.repeats)
        y = fns["device_loop_ms"]()
        out = {k: stats(v) for k, v in ms.items()}
        out["finite"] = bool(torch.isfinite(y).all())
        if not args.concat_only:
            out["loops_bit_identical"] = bool(torch.equal(y, host()))
            out["device_over_per_step"] = round(out["device_loop_ms"]["median"] / out["per_step_loop_ms"]["median"], 4)
            out["plan"] = unet.plan_info()
        res[name] = out
        del unet
        torch.cuda.empty_cache()
    if args.baseline:
        theirs = []
        for path in args.baseline:
            with open(path) as f:
                theirs.append(json.loads(f.read().strip().splitlines()[-1])["concat"]["device_loop_ms"]["median"])
        res["baseline_concat_device_loop_ms"] = theirs
        res["concat_loop_over_baseline"] = round(res["concat"]["device_loop_ms"]["median"] / statistics.mean(theirs), 4)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
