#!/usr/bin/env python3
"""The latent trainer's inference (trainers/trainer_latent_diffusion.py:153-189,492-544) on one GPU with synthetic weights:
batch 16 of 256^2 one-channel slices, the SD-v1 f = 8 first stage (32x32x4 latents), K condition keys encoded in one pass,
50-step DDIM (eta 0) on a UNetModel with the unet_config of the reference's v2-1-cddpm-disc yaml (in_channels 4*(K+1)), decode.
Three loops for the same steps, alternated in one process: the device loop (dsd_sample) with graph replay off, with
replay on, and the per-step Python loop (network call + dsd_op_sampler_update, the closure path).  hipEvents, median / min / max
of --repeats runs.  Prints one JSON line.
With --guidance-scale S (S != 1) three more loops join the alternation: the guided device loop at the batch
(dsd_sample with a dsd_guidance: 2B network rows per step, u = zeros), the unguided loop at the batch, and the unguided loop at twice
the batch — the same network work as the guided one, so guided(B) against unguided(2B) is what the combine and the doubled
state cost.  Each of the three is preceded by one untimed step of its own, so that no timed run pays for the plan of another
batch size.
With --mask the masked device loop (dsd_sample with a dsd_inpaint: centre half of the latent sampled, Philox blend noise) is timed
against the unmasked loop, and with --encode the DDIM inversion loop (dsd_invert, all steps) against plain sampling — the
same network work per step, so each ratio is what the blend kernel / the inversion step costs.  Same alternation and untimed
first step as the guided loops.
With --plms the PLMS device loop (dsd_sample_plms: one network evaluation per step plus one more at the first step, so
steps + 1 in all) is timed against the DDIM loop of the same steps: plms_over_ddim is expected near (steps + 1) / steps and is
measured here, not assumed.  The network of this bench is a v-model, which PLMS does not take; the PLMS schedule is packed as for
a noise-predicting one — the same kernels and the same work.
With --dpm-family LIST (of ss3, ms3, ms2) the DPM-Solver++ loops of 21 network evaluations are timed in the same alternation:
singlestep order 3 and multistep order 3 (dsd_sample_dpm_program) and multistep order 2 (dsd_sample_dpm, the loop
that existed before them).  The host tables are built once outside the timed region, every timed run follows an untimed run of
the same loop, and the result holds the ms per network evaluation of each and the ratios to ms2.  For a build from before the
program entry, copy this script into a checkout of that commit (this tree's binding does not load such a library) and run
`--dpm-family ms2` there; --baseline with those lines then also records this build's ms2 loop over that build's.
With --bpd the variational-bound loop (dsd_calc_bpd: q_sample, one network evaluation and the terms / finalize launches per
step, Philox noise) is timed against the mode-A DDPM sampling loop of the same handle, schedule and step count (dsd_sample):
bpd_over_ddpm is what the three small launches cost beside a network evaluation.  Same alternation and untimed first step.
With --adaptive the adaptive step-size solver (DPM_Solver.dpm_solver_adaptive, order 2, --adaptive-tol atol,rtol: one
dsd_sample_dpm_adaptive_trial and one read-back of B floats per trial) is run once untimed for its count of network evaluations
and then timed against a singlestep_fixed program of exactly that many (dsd_sample_dpm_program) in the same alternation:
adaptive_over_fixed_same_nfe is what the error kernel, the read-back, the per-trial binding and the host's coefficient rows
(adaptive_host_rows_ms_per_trial) cost beside the network.
With --baseline FILE (repeatable) the bench lines that another build wrote with --json on the same machine — the parent commit's,
run in turn with this one — are recorded beside the result: their device_loop_ms medians per K, and the ratio of this
build's plain loop (the median of its device, unmasked and sample loops, which are the same call) to their mean.

    python tools/bench_latent.py [--batch 16] [--steps 50] [--keys 1,3] [--repeats 3] [--guidance-scale 3] [--mask] [--encode]
                                 [--plms] [--bpd] [--dpm-family ss3,ms3,ms2] [--adaptive] [--baseline other.json ...] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SD_VAE = dict(double_z=True, z_channels=4, resolution=256, in_channels=1, out_ch=1, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)
UNET = dict(image_size=32, model_channels=96, out_channels=4, num_res_blocks=2, attention_resolutions=[32, 16, 8],
            channel_mult=[1, 1, 2, 2, 3, 3], num_head_channels=48, use_new_attention_order=True, legacy=False)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_k(K, args):
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd._sched import (Guidance, Inpaint, invert_coefficients, run_device_loop, run_bpd_loop,
                                                    run_invert_loop, run_plms_loop, sampler_update)
    from diffusion_models_dsdiff_amd.ldm.models.autoencoder import AutoencoderKL
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    from oracle.synth import synth_params, randn
    dd = dict(SD_VAE)
    up = dict(UNET, in_channels=4 * (K + 1))
    ld = LatentDiffusion(first_stage_config=AutoencoderKL(dd, None, 4), conditioning_key="concat", scale_factor=0.18215,
                         timesteps=1000, parameterization="v",
                         unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": up})
    ld.load_state_dict(synth_params([(k, tuple(v.shape)) for k, v in ld.state_dict().items() if "." in k], 700 + K), strict=False)
    ld = ld.cuda()
    unet = ld.model.diffusion_model
    B, h = args.batch, args.size // 8
    cond = randn((B, K, args.size, args.size), 710).cuda()
    xT = randn((B, 4, h, h), 711).cuda()
    smp = DDIMSampler(ld)
    smp.make_schedule(args.steps, ddim_eta=0.0, verbose=False)
    sched = smp._schedule(False, True)
    pl = PLMSSampler(ld)
    pl.make_schedule(args.steps, verbose=False)
    plms_sched = pl._schedule().with_pred(_lib.PRED_EPS)
    L = _lib.lib()

    def device(graph):
        _lib.check(L.dsd_set_graph(unet._h, int(graph)))
        try:
            return run_device_loop(unet, sched, xT, c, seed=1)
        finally:
            _lib.check(L.dsd_set_graph(unet._h, 0))

    def host():
        x = xT.clone()
        cc = c.contiguous()
        for k in range(sched.steps):
            out = unet(torch.cat([x, cc], 1), torch.full((B,), float(sched.t_model[k]), device="cuda"))
            sampler_update(sched, k, out, x, None, seed=1)
        return x

    def cfg_loop(kind, n_steps=0):
        if kind == "guided":
            return run_device_loop(unet, sched, xT, c, seed=1, n_steps=n_steps,
                                   guidance=Guidance(torch.zeros_like(c), args.guidance_scale, sched.steps))
        if kind == "unguided":
            return run_device_loop(unet, sched, xT, c, seed=1, n_steps=n_steps)
        return run_device_loop(unet, sched, torch.cat([xT, xT]), torch.cat([c, c]), seed=1, n_steps=n_steps)   # "unguided_2x"

    x0 = randn((B, 4, h, h), 712).cuda()
    mask = torch.ones(B, 1, h, h, device="cuda")
    mask[:, :, h // 4:h - h // 4, h // 4:h - h // 4] = 0.
    inv_coef = invert_coefficients(torch.from_numpy(smp.ddim_alphas.astype("float32")), torch.tensor(smp.ddim_alphas_prev))

    if args.bpd:
        import numpy as np
        from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
        gd_a = create_gaussian_diffusion(steps=1000, timestep_respacing=str(args.steps), parameterization="v")
        sched_a, plv = gd_a._schedule(False, 0.0, True), gd_a._post_log_var()
        prior_lv = float(np.float32(gd_a.log_one_minus_alphas_cumprod[-1]))
        x_start = x0.clamp(-1, 1)

    def i2i_loop(kind, n_steps=0):
        if kind == "bpd":
            return run_bpd_loop(unet, sched_a, plv, prior_lv, x_start, c, seed=1, n_steps=n_steps)["vb"]
        if kind == "ddpm_a":
            return run_device_loop(unet, sched_a, xT, c, seed=1, n_steps=n_steps)
        if kind == "masked":
            return run_device_loop(unet, sched, xT, c, seed=1, n_steps=n_steps, inpaint=Inpaint(x0, mask))
        if kind == "invert":
            return run_invert_loop(unet, inv_coef, x0, c, n_steps=n_steps)
        if kind == "plms":
            return run_plms_loop(unet, plms_sched, xT, c, n_steps=n_steps)
        return run_device_loop(unet, sched, xT, c, seed=1, n_steps=n_steps)       # "unmasked" / "sample" / "ddim": the plain loop

    DPM_EVALS = 21
    dpm_kinds = tuple(k for k in args.dpm_family.split(",") if k)
    assert set(dpm_kinds) <= {"ss3", "ms3", "ms2"}, dpm_kinds
    dpm_runs = {}

    def dpm_prepare():
        from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
        ns = dsa.NoiseScheduleVP("discrete", alphas_cumprod=ld.alphas_cumprod.detach().float().cpu())
        fn = dsa.model_wrapper(unet, ns, model_type="v", model_kwargs=dict(c_concat=[c]))
        sol = dsa.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")
        for kind in dpm_kinds:
            if kind == "ms2":
                sched = sol.build_schedule(DPM_EVALS, order=2, skip_type="time_uniform")
                assert sched.steps == DPM_EVALS
                dpm_runs[kind] = lambda sched=sched: dsa.run_dpm_loop(fn, sched, xT)
            else:
                prog = sol.build_program(DPM_EVALS, order=3, skip_type="time_uniform",
                                         method="singlestep" if kind == "ss3" else "multistep")
                assert prog.steps == DPM_EVALS
                dpm_runs[kind] = lambda prog=prog: dsa.run_dpm_program(fn, prog, xT)[0]

    ad = {}

    def adaptive_prepare():
        """The adaptive loop (order 2, --adaptive-tol) once, untimed, for its count of evaluations; then a singlestep_fixed program
        of exactly that many — the same network work without the error kernel, the read-back and the per-trial binding."""
        import time
        from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
        ns = dsa.NoiseScheduleVP("discrete", alphas_cumprod=ld.alphas_cumprod.detach().float().cpu())
        fn = dsa.model_wrapper(unet, ns, model_type="v", model_kwargs=dict(c_concat=[c]))
        sol = dsa.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")
        atol, rtol = (float(v) for v in args.adaptive_tol.split(","))
        rows, host_ms = sol.adaptive_trial_program, [0.]

        def timed_rows(*a):                                        # host time of the coefficient rows of a trial
            t0 = time.perf_counter()
            out = rows(*a)
            host_ms[0] += (time.perf_counter() - t0) * 1e3
            return out
        sol.adaptive_trial_program = timed_rows
        run = lambda: sol.dpm_solver_adaptive(xT, 2, 1., 1. / ns.total_N, atol=atol, rtol=rtol, max_nfe=400, return_trace=True)
        _, trace = run()
        nfe = 2 * len(trace)
        prog = sol.build_program(nfe, order=2, skip_type="logSNR", method="singlestep_fixed")
        assert prog.steps == nfe
        ad.update(nfe=nfe, trials=len(trace), rejected=sum(not t[4] for t in trace), atol=atol, rtol=rtol, host_ms=host_ms)
        dpm_runs["adaptive"] = lambda: run()[0]
        dpm_runs["fixed_same_nfe"] = lambda: dsa.run_dpm_program(fn, prog, xT)[0]

    i2i_kinds = ((("masked", "unmasked") if args.mask else ()) + (("invert", "sample") if args.encode else ()) +
                 (("plms", "ddim") if args.plms else ()) + (("bpd", "ddpm_a") if args.bpd else ()))
    cfg_kinds = ("guided", "unguided", "unguided_2x") if args.guidance_scale != 1. else ()
    c = ld.encode_conditions(cond, seed=3)["c_concat"][0]          # warm-up: plans, code objects
    for kind in cfg_kinds:
        cfg_loop(kind)
    for kind in i2i_kinds:
        i2i_loop(kind)
    if dpm_kinds:
        dpm_prepare()
    if args.adaptive:
        adaptive_prepare()
        dpm_kinds = dpm_kinds + ("adaptive", "fixed_same_nfe")
    for kind in dpm_kinds:
        dpm_runs[kind]()
    y = device(False)
    device(True)
    device(True)
    host()
    ld.decode_first_stage(y)
    torch.cuda.synchronize()
    t = {"encode_ms": [], "device_loop_ms": [], "device_loop_graph_ms": [], "python_loop_ms": [], "decode_ms": []}
    t.update({kind + "_loop_ms": [] for kind in cfg_kinds + i2i_kinds + dpm_kinds})
    outs = {}
    for _ in range(args.repeats):
        c, ms = timed(lambda: ld.encode_conditions(cond, seed=3)["c_concat"][0])
        t["encode_ms"].append(ms)
        outs["dev"], ms = timed(lambda: device(False))
        t["device_loop_ms"].append(ms)
        outs["graph"], ms = timed(lambda: device(True))
        t["device_loop_graph_ms"].append(ms)
        outs["host"], ms = timed(host)
        t["python_loop_ms"].append(ms)
        _, ms = timed(lambda: ld.decode_first_stage(outs["dev"]))
        t["decode_ms"].append(ms)
        for kind in cfg_kinds:
            cfg_loop(kind, n_steps=1)                              # untimed: settles the plan of this batch size
            torch.cuda.synchronize()
            _, ms = timed(lambda: cfg_loop(kind))
            t[kind + "_loop_ms"].append(ms)
        for kind in i2i_kinds:
            i2i_loop(kind, n_steps=1)                              # untimed, as above
            torch.cuda.synchronize()
            _, ms = timed(lambda: i2i_loop(kind))
            t[kind + "_loop_ms"].append(ms)
        for kind in dpm_kinds:
            dpm_runs[kind]()                                       # untimed run of the same loop
            torch.cuda.synchronize()
            if kind == "adaptive":
                ad["host_ms"][0] = 0.
            _, ms = timed(dpm_runs[kind])
            t[kind + "_loop_ms"].append(ms)
            if kind == "adaptive":
                t.setdefault("adaptive_host_rows_ms", []).append(ad["host_ms"][0])
    res = {k: stats(v) for k, v in t.items()}
    for k in ("device_loop", "device_loop_graph", "python_loop") + tuple(kind + "_loop" for kind in cfg_kinds + i2i_kinds):
        res[k + "_ms_per_step"] = res[k + "_ms"]["median"] / sched.steps
    if cfg_kinds:
        res["guidance_scale"] = args.guidance_scale
        res["guided_over_unguided_2x"] = res["guided_loop_ms"]["median"] / res["unguided_2x_loop_ms"]["median"]
        res["guided_over_unguided"] = res["guided_loop_ms"]["median"] / res["unguided_loop_ms"]["median"]
    if args.mask:
        res["masked_over_unmasked"] = res["masked_loop_ms"]["median"] / res["unmasked_loop_ms"]["median"]
    if args.encode:
        res["invert_over_sample"] = res["invert_loop_ms"]["median"] / res["sample_loop_ms"]["median"]
    if args.plms:
        res["plms_over_ddim"] = res["plms_loop_ms"]["median"] / res["ddim_loop_ms"]["median"]
        res["plms_network_evaluations"] = sched.steps + 1
    if args.bpd:
        res["bpd_over_ddpm"] = res["bpd_loop_ms"]["median"] / res["ddpm_a_loop_ms"]["median"]
    if args.adaptive:
        nfe = ad["nfe"]
        res.update(adaptive_network_evaluations=nfe, adaptive_trials=ad["trials"], adaptive_rejected=ad["rejected"],
                   adaptive_atol=ad["atol"], adaptive_rtol=ad["rtol"],
                   adaptive_ms_per_evaluation=res["adaptive_loop_ms"]["median"] / nfe,
                   fixed_same_nfe_ms_per_evaluation=res["fixed_same_nfe_loop_ms"]["median"] / nfe,
                   adaptive_over_fixed_same_nfe=res["adaptive_loop_ms"]["median"] / res["fixed_same_nfe_loop_ms"]["median"],
                   adaptive_host_rows_ms_per_trial=res["adaptive_host_rows_ms"]["median"] / ad["trials"])
        dpm_kinds = tuple(k for k in dpm_kinds if k not in ("adaptive", "fixed_same_nfe"))
    if dpm_kinds:
        res["dpm_network_evaluations"] = DPM_EVALS
        for kind in dpm_kinds:
            res[kind + "_ms_per_evaluation"] = res[kind + "_loop_ms"]["median"] / DPM_EVALS
            if "ms2" in dpm_kinds and kind != "ms2":
                res[kind + "_over_ms2"] = res[kind + "_loop_ms"]["median"] / res["ms2_loop_ms"]["median"]
    e2e = res["encode_ms"]["median"] + res["device_loop_ms"]["median"] + res["decode_ms"]["median"]
    res["end_to_end_ms"] = e2e
    res["slices_per_s"] = B / (e2e / 1000.)
    res["graph_bit_identical"] = bool(torch.equal(outs["dev"], outs["graph"]))
    res["python_loop_bit_identical"] = bool(torch.equal(outs["dev"], outs["host"]))
    res["unet_config"] = up
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--keys", default="1,3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--guidance-scale", type=float, default=1.0,
                    help="!= 1: also time the guided loop against the unguided loop at the batch and at twice the batch")
    ap.add_argument("--mask", action="store_true", help="also time the masked loop against the unmasked loop")
    ap.add_argument("--encode", action="store_true", help="also time the DDIM inversion loop against plain sampling")
    ap.add_argument("--plms", action="store_true", help="also time the PLMS loop against the DDIM loop of the same steps")
    ap.add_argument("--bpd", action="store_true", help="also time the variational-bound loop against the mode-A DDPM sampling loop")
    ap.add_argument("--dpm-family", default="", help="comma list of ss3, ms3, ms2: also time those DPM-Solver++ loops of 21 evaluations")
    ap.add_argument("--adaptive", action="store_true",
                    help="also time DPM_Solver.dpm_solver_adaptive (order 2) against a singlestep_fixed program of the same evaluations")
    ap.add_argument("--adaptive-tol", default="0.0078,0.05", help="atol,rtol of --adaptive")
    ap.add_argument("--baseline", action="append", default=[],
                    help="bench line of another build on the same machine (repeatable): record its plain loop beside this one's")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from diffusion_models_dsdiff_amd import _lib
    name, ncu, _ = _lib.require_gpu(0)
    out = {"bench": "latent_inference", "gpu": name, "batch": args.batch, "size": args.size, "latent": [4, args.size // 8, args.size // 8],
           "first_stage": dict(SD_VAE, embed_dim=4), "scale_factor": 0.18215, "sampler": f"DDIM eta 0, {args.steps} steps",
           "repeats": args.repeats, "keys": {}}
    for K in [int(v) for v in args.keys.split(",")]:
        out["keys"][str(K)] = run_k(K, args)
    if args.baseline:
        base = []
        for path in args.baseline:
            with open(path) as f:
                base.append(json.loads(f.readline()))
        for K, res in out["keys"].items():
            theirs = [b["keys"][K]["device_loop_ms"]["median"] for b in base if K in b["keys"]]
            if not theirs:
                continue
            plain = [res[k]["median"] for k in ("device_loop_ms", "unmasked_loop_ms", "sample_loop_ms", "ddim_loop_ms") if k in res]
            res["baseline_device_loop_ms"] = theirs
            res["plain_loop_ms"] = statistics.median(plain)
            res["plain_over_baseline"] = res["plain_loop_ms"] / statistics.mean(theirs)
            ms2 = [b["keys"][K]["ms2_loop_ms"]["median"] for b in base if "ms2_loop_ms" in b["keys"].get(K, {})]
            if ms2 and "ms2_loop_ms" in res:
                res["baseline_ms2_loop_ms"] = ms2
                res["ms2_over_baseline"] = res["ms2_loop_ms"]["median"] / statistics.mean(ms2)
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
