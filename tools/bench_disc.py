#!/usr/bin/env python3
"""UNet_disc_Model (the four-stream DisC-Diff denoiser) measured on one GPU with synthetic weights, one process.

At the sizes of the reference's two yamls — configs/disc-diff.yaml (160 channels, channel_mult 1-2-4-4) and
configs/disc-diff-origin.yaml (96 channels, channel_mult 1-1-2-2-3-3), 320x320 inputs, bf16x6:
  - ms per network evaluation (UNet_disc_Model._run without feature export, what the loops run), launches and executed
    TFLOP/s of the plan; beside it the same forward written in torch ops on the same GPU (tests/disc_ref.py), as bench.py
    reports torch_eager_same_gpu for the flagship;
  - the bottleneck head fused (csrc/disc.hip) against unfused (DSD_DISC_UNFUSED: avg_into / se_scale / concat copies) inside
    the network, from the per-op hipEvent profile (dsd_profile_*): the ops between conv_distinct and dim_reduction_non_zeros,
    with their algorithmic bytes against the 8 TB/s HBM rate tools/workloads.py uses for memory-bound kernels; the two plans
    alternate, every profiled forward after an untimed one of the same plan;
  - the --steps-step DDIM (eta 0) device loop against the per-step loop (forward + dsd_op_sampler_update) on the same handle.
Medians of --repeats alternated runs, each after an untimed run; hipEvents.  A batch that does not fit is halved until it does
and the line says so.  Nothing here imports the reference.

    python tools/bench_disc.py [--batch 16] [--size 320] [--steps 20] [--repeats 3] [--only disc-diff,disc-diff-origin]
                               [--no-eager] [--json out.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

YAMLS = {
    "disc-diff": dict(image_size=32, in_channels=1, out_channels=1, model_channels=160, attention_resolutions=[16], num_res_blocks=2,
                      channel_mult=[1, 2, 4, 4], num_head_channels=32, use_new_attention_order=True),
    "disc-diff-origin": dict(image_size=32, in_channels=1, out_channels=1, model_channels=96, attention_resolutions=[32, 16, 8],
                             num_res_blocks=2, channel_mult=[1, 1, 2, 2, 3, 3], num_head_channels=48, use_new_attention_order=True),
}
PEAK_HBM_GBS = 8000.0


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
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[1])
    return ms


def head_ops(unet):
    """(ms, bytes, launches-as-ops) of the bottleneck head in the last profiled forward: the memory-bound ops the plan names
    after conv_distinct's or an SE_Attention parameter (everything between the eight convolutions and the Conv1x1)."""
    ms = by = n = 0
    for kind, op_ms, _, op_bytes, layer in unet.profile_ops():
        if kind.startswith("conv_"):
            continue
        if layer.startswith("SE_Attention_") or layer.startswith("conv_distinct.0"):
            ms, by, n = ms + op_ms, by + op_bytes, n + 1
    return ms, by, n


def head_ab(unet, x_in, t, repeats):
    """Fused and unfused head alternated in one process: the plan is rebuilt at every switch (the switch is read when a plan
    is built), an untimed forward follows, then the profiled one."""
    out = {"fused": [], "unfused": []}
    info = {}
    for _ in range(repeats):
        for route in ("fused", "unfused"):
            if route == "unfused":
                os.environ["DSD_DISC_UNFUSED"] = "1"
            try:
                unet._run(x_in, t, want_feats=False)
                torch.cuda.synchronize()
                unet.profile(True)
                unet._run(x_in, t, want_feats=False)
                ms, by, n = head_ops(unet)
                unet.profile(False)
                info[route] = dict(ops=n, launches=unet.plan_info()["launches"])
            finally:
                os.environ.pop("DSD_DISC_UNFUSED", None)
            out[route].append((ms, by))
    unet._run(x_in, t, want_feats=False)                          # back on the fused plan
    res = {}
    for route, v in out.items():
        m = statistics.median(a for a, _ in v)
        res[route] = dict(ms=stats([a for a, _ in v]), ops=info[route]["ops"], plan_launches=info[route]["launches"])
        if route == "fused":
            res[route]["bytes"] = v[0][1]
            res[route]["hbm_gbs"] = round(v[0][1] / m / 1e6, 1)
            res[route]["hbm_fraction_of_peak"] = round(v[0][1] / m / 1e6 / PEAK_HBM_GBS, 4)
    res["fused_over_unfused"] = round(res["fused"]["ms"]["median"] / res["unfused"]["ms"]["median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=",".join(YAMLS))
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    from workloads import fill_
    import disc_ref
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd._sched import run_device_loop, sampler_update
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import UNet_disc_Model
    S = args.size
    sched = create_gaussian_diffusion(steps=1000, timestep_respacing=str(args.steps), rescale_timesteps=True)._schedule(True, 0.0, True)
    res = {"workload": f"UNet_disc_Model, {S}x{S}x4 input, bf16x6; {args.steps}-step DDIM eta 0",
           "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH)}
    for name in args.only.split(","):
        params = YAMLS[name]
        unet = fill_(UNet_disc_Model(**params), 2041)
        B, out = args.batch, {}
        while True:
            g = torch.Generator().manual_seed(2040)
            xT, cc = torch.randn(B, 1, S, S, generator=g).cuda(), torch.randn(B, 3, S, S, generator=g).cuda()
            x_in, t = torch.cat([xT, cc], 1).contiguous(), torch.full((B,), 500.0).cuda()
            try:
                unet._run(x_in, t, want_feats=False)
                torch.cuda.synchronize()
                break
            except (_lib.DsdError, RuntimeError) as e:
                if B == 1 or "memory" not in str(e).lower():
                    raise
                out["batch_note"] = f"batch {B} did not fit ({str(e)[:80]}); halved"
                B //= 2
                torch.cuda.empty_cache()
        out["batch"] = B
        ms = alternate({"evaluation_ms": lambda: unet._run(x_in, t, want_feats=False)}, args.repeats)
        out["evaluation_ms"] = stats(ms["evaluation_ms"])
        out["plan"] = unet.plan_info()
        out["executed_tflops"] = round(out["plan"]["flops"] / out["evaluation_ms"]["median"] / 1e9, 1)
        print(f"[{name}] evaluation {out['evaluation_ms']['median']} ms at batch {B}", file=sys.stderr, flush=True)
        out["head"] = head_ab(unet, x_in, t, args.repeats)
        print(f"[{name}] head {out['head']}", file=sys.stderr, flush=True)
        if not args.no_eager:
            sd = {k: v.detach().cuda() for k, v in unet.state_dict().items()}
            eb = B
            while True:
                try:
                    eager = lambda: disc_ref._DiscNet(disc_ref.unet_config(params), sd).forward(x_in[:eb], t[:eb])[8]
                    with torch.no_grad():
                        ms = alternate({"torch_eager_ms": eager}, args.repeats)
                        ref = eager()
                    break
                except RuntimeError as e:
                    if eb == 1 or "memory" not in str(e).lower():
                        raise
                    eb //= 2
                    torch.cuda.empty_cache()
            out["torch_eager_same_gpu"] = dict(batch=eb, ms=stats(ms["torch_eager_ms"]))
            out["torch_eager_ms_per_sample_over_native"] = round(
                (out["torch_eager_same_gpu"]["ms"]["median"] / eb) / (out["evaluation_ms"]["median"] / B), 3)
            got = unet._run(x_in[:eb].contiguous(), t[:eb].contiguous(), want_feats=False)[0]
            out["native_vs_torch_rel_l2"] = float((got.double() - ref.double()).norm() / ref.double().norm())
            del sd, ref, got
            torch.cuda.empty_cache()
            unet._run(x_in, t, want_feats=False)
            print(f"[{name}] torch eager {out['torch_eager_same_gpu']}", file=sys.stderr, flush=True)

        def host():
            x = xT.clone()
            for k in range(sched.steps):
                o = unet._run(torch.cat([x, cc], 1), torch.full((B,), float(sched.t_model[k]), device="cuda"), want_feats=False)[0]
                sampler_update(sched, k, o, x, None, seed=1)
            return x

        fns = {"device_loop_ms": lambda: run_device_loop(unet, sched, xT, cc, seed=1), "per_step_loop_ms": host}
        ms = alternate(fns, args.repeats)
        y = fns["device_loop_ms"]()
        out.update({k: stats(v) for k, v in ms.items()})
        out["finite"] = bool(torch.isfinite(y).all())
        out["loops_bit_identical"] = bool(torch.equal(y, host()))
        out["device_over_per_step"] = round(out["device_loop_ms"]["median"] / out["per_step_loop_ms"]["median"], 4)
        res[name] = out
        del unet
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
