#!/usr/bin/env python3
"""BASELINE configs[4] on one GPU: DiT-B/8 on 512x512 (4096 tokens, 12 heads of 64, depth 12), one evaluation of a slice batch,
per arithmetic mode, with the per-kernel split from dsd_profile_* (hipEvents on the launch stream).  Synthetic weights.

    python tools/bench_dit.py [--batch 16] [--modes f16,bf16,bf16x6] [--iters 5] [--json out.json]

With --loop the DiT is timed as a denoiser of the device sampling loops instead: the 20-step DPM-Solver++ loop (order 2, logSNR
spacing, dynamic thresholding: GaussianDiffusion.dpm_solver_sample_loop) on DiT-B/8 at 512x512, batch 16, fp16, against the same
20 steps through the per-step path on the same handle (one torch.cat, one DiT.forward and one dsd_op_dpm_step per step); and the
same pair on a launch-bound shape, DiT-S/2 on 32x32 at batch 1, with and without graph replay.  One process, the loops
alternated, medians of --repeats runs, each timed run preceded by an untimed two-step run of its own (the second-order solver
takes no fewer).  Reports loop_over_python per
shape.  With --baseline FILE (repeatable) the lines another build wrote with --json on the same machine — the parent commit's
library, run in turn with this one — are recorded beside the per-evaluation time measured here, with their ratio.

    python tools/bench_dit.py --loop [--steps 20] [--repeats 3] [--baseline other.json ...] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def synth_dit(**kw):
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import DiT
    dit = DiT(num_classes=0, **kw)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in dit.parameters():
            p.normal_(0.0, 0.02, generator=g)
    return dit


def loop_shape(dit, B, steps, repeats, prec, graph_too):
    """The DPM-Solver++ device loop against the per-step path on one handle: {loop, loop_graph, python}_ms and their ratios."""
    import ctypes as C
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    L = _lib.lib()
    S = dit.input_size
    dit.set_precision(prec)
    d = create_gaussian_diffusion(steps=1000, learn_sigma=True, timestep_respacing=str(steps), rescale_timesteps=True)
    g = torch.Generator().manual_seed(5)
    xT = torch.randn(B, 1, S, S, generator=g).cuda()
    cond = torch.randn(B, dit.in_channels - 1, S, S, generator=g).clamp(-1, 1).cuda()
    ns = dsa.NoiseScheduleVP(schedule="discrete", betas=torch.from_numpy(d.betas).float())
    sol = dsa.DPM_Solver(dsa.model_wrapper(dit, ns, model_type="noise", model_kwargs=dict(c_concat=[cond])), ns,
                         algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")
    # both sides run prebuilt schedules: the host-side table building of DPM_Solver.sample is in neither timed region
    scs = {n: sol.build_schedule(n, None, None, 2, "logSNR", False, False, "dpmsolver") for n in (2, steps)}

    def device(graph, n=steps):
        _lib.check(L.dsd_set_graph(dit._h, int(graph)))
        try:
            return dsa.run_dpm_loop(sol.model_fn_, scs[n], xT)
        finally:
            _lib.check(L.dsd_set_graph(dit._h, 0))

    def host(n=steps):
        sc = scs[n]
        x = xT.clone()
        m_cur, m_prev = torch.empty_like(x), torch.empty_like(x)
        for k in range(n):
            out = dit(torch.cat([x, cond], 1), torch.full((B,), float(sc.t_input[k]), device="cuda"))
            _lib.check(L.dsd_op_dpm_step(C.byref(sc.c), k, _lib.dptr(out), out.shape[1], _lib.dptr(x), _lib.dptr(m_cur),
                                         _lib.dptr(m_prev), B, S, S, _lib.stream_ptr()))
            m_cur, m_prev = m_prev, m_cur
        return x

    def forward():
        return dit(torch.cat([xT, cond], 1), torch.full((B,), 500.0, device="cuda"))
    kinds = [("loop", lambda n=steps: device(False, n))] + ([("loop_graph", lambda n=steps: device(True, n))] if graph_too else [])
    kinds.append(("python", host))
    for _, fn in kinds:                                            # warm-up: plans, code objects, the captured graph
        fn(2)
    t = {k + "_ms": [] for k, _ in kinds}
    t["forward_ms"] = []
    outs = {}
    for _ in range(repeats):
        for k, fn in kinds:
            fn(2)                                                  # untimed: settles this path's plan and buffers (order 2 needs 2 steps)
            torch.cuda.synchronize()
            outs[k], ms = timed(fn)
            t[k + "_ms"].append(ms)
        forward()
        torch.cuda.synchronize()
        _, ms = timed(lambda: [forward() for _ in range(5)])
        t["forward_ms"].append(ms / 5)
    res = {k: stats(v) for k, v in t.items()}
    res.update(batch=B, steps=steps, precision=prec, input=S, patch=dit.patch_size, launches_per_forward=dit.plan_info().get("launches"))
    res["loop_over_python"] = res["loop_ms"]["median"] / res["python_ms"]["median"]
    res["loop_ms_per_step"] = res["loop_ms"]["median"] / steps
    res["python_ms_per_step"] = res["python_ms"]["median"] / steps
    res["python_loop_bit_identical"] = bool(torch.equal(outs["loop"], outs["python"]))
    if graph_too:
        res["loop_graph_over_python"] = res["loop_graph_ms"]["median"] / res["python_ms"]["median"]
        res["loop_graph_over_loop"] = res["loop_graph_ms"]["median"] / res["loop_ms"]["median"]
        res["graph_bit_identical"] = bool(torch.equal(outs["loop"], outs["loop_graph"]))
    return res


def loop_bench(args):
    from diffusion_models_dsdiff_amd import _lib
    name, _, _ = _lib.require_gpu(0)
    out = {"bench": "dit_device_loop", "gpu": name, "sampler": f"DPM-Solver++ order 2, logSNR, dynamic thresholding, {args.steps} steps",
           "repeats": args.repeats, "shapes": {}}
    big = synth_dit(input_size=args.size, patch_size=args.patch, in_channels=4, hidden_size=args.hidden, depth=args.depth,
                    num_heads=args.heads)
    out["shapes"]["dit_b8_512"] = loop_shape(big, args.batch, args.steps, args.repeats, "f16", False)
    del big
    small = synth_dit(input_size=32, patch_size=2, in_channels=4, hidden_size=384, depth=12, num_heads=6)
    out["shapes"]["dit_s2_32_b1"] = loop_shape(small, 1, args.steps, args.repeats, "f16", True)
    if args.baseline:
        theirs = []
        for path in args.baseline:
            with open(path) as f:
                theirs.append(json.load(f)["f16"]["ms_per_forward_median"])
        mine = out["shapes"]["dit_b8_512"]["forward_ms"]["median"]
        out["baseline_forward_ms"] = theirs
        out["forward_over_baseline"] = mine / statistics.mean(theirs)
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--modes", default="f16,bf16,bf16x6")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--patch", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--json", default=None)
    ap.add_argument("--loop", action="store_true", help="time the DPM-Solver++ device loop against the per-step path (see above)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="append", default=[],
                    help="--json file of another build's plain run on the same machine (repeatable), for --loop")
    args = ap.parse_args()
    if args.loop:
        return loop_bench(args)
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import DiT
    B = args.batch
    dit = DiT(input_size=args.size, patch_size=args.patch, in_channels=4, hidden_size=args.hidden, depth=args.depth,
              num_heads=args.heads, num_classes=0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in dit.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.02, generator=g)
            else:
                p.normal_(0.0, 0.02, generator=g)
    x = torch.randn(B, 4, args.size, args.size).cuda()
    t = torch.full((B,), 500.0).cuda()
    res = {"batch": B, "gpu": torch.cuda.get_device_name(0), "tokens": (args.size // args.patch) ** 2, "hidden": args.hidden,
           "depth": args.depth, "heads": args.heads}
    for prec in args.modes.split(","):
        dit.set_precision(prec)
        for _ in range(2):
            out = dit(x, t)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(3):
            e0.record()
            for _ in range(args.iters):
                out = dit(x, t)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.iters)
        info = dit.plan_info()
        dit.profile(True)
        for _ in range(2):
            dit(x, t)
        rep, runs = dit.profile_report()
        dit.profile(False)
        kinds = {}
        for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"]):
            per = v["ms"] / runs
            kinds[k] = {"ms": round(per, 3), "calls": v["calls"] // runs,
                        "tflops": round(v["flops"] / runs / per / 1e9, 1) if v["flops"] else None,
                        "gbps": round(v["bytes"] / runs / per / 1e6, 1) if v["bytes"] else None}
        res[prec] = {"ms_per_forward_median": round(sorted(ms)[1], 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                     "plan_tflop": round(info["flops"] / 1e12, 3), "tflops": round(info["flops"] / sorted(ms)[1] / 1e9, 1),
                     "finite": bool(torch.isfinite(out).all()), "kernels": kinds}
        print(prec, json.dumps(res[prec]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
