#!/usr/bin/env python3
"""Generate tests/golden/bpd.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_bpd.py

The reference's own GaussianDiffusion._vb_terms_bpd / _prior_bpd / p_mean_variance / ddim_reverse_sample / calc_bpd_loop
(Disc_diff/guided_diffusion/gaussian_diffusion.py) on the case grid of tests/bpd_cases.py.

  op cases    a "model" that returns a stored tensor; every case twice: as the reference computes it (fp32) and from the same
              reference functions called on float64 tensors.  Stored: vb / xstart_mse / mse per sample for every case, the
              mean / log_variance / pred_xstart / ddim_reverse_sample planes for the plane cases, the prior of every size.
  loop cases  calc_bpd_loop with fed noise (torch.randn_like replaced by a feeder) on the tiny DSUnetModels, the latent
              UNetModel and the restated DiT of tests/dit_loops_util.py, each also with 3e-6 relative noise on every network
              output: the movement of each scalar is recorded.

Stored: results, the reference's float64 tables, measured bars.  Inputs regenerate from seeds (tests/bpd_cases.py), weights from
synth_params.  Asserted here: every op case lies further than 100 op bars from its twins (wrong t; other variance type where the
two differ, 0 < t < T-1; clip off where the clip acts), and the op bar stays <= 1e-3.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ["DSD_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import bpd_cases as BC  # noqa: E402
from gen_cfg import _params  # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(8)
PERTURB, PERTURB_SEED = 3e-6, 761
BAR_MAX, TWIN_FACTOR = 1e-3, 100.


def ref_diffusion(pred, var, respacing, rescale=False):
    import Disc_diff.guided_diffusion.gaussian_diffusion as gd
    from Disc_diff.guided_diffusion.respace import space_timesteps, SpacedDiffusion
    vt = {"small": gd.ModelVarType.FIXED_SMALL, "large": gd.ModelVarType.FIXED_LARGE, "range": gd.ModelVarType.LEARNED_RANGE}[var]
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, respacing), betas=gd.get_named_beta_schedule("linear", 1000),
                           model_mean_type=gd.ModelMeanType.START_X if pred == "x0" else gd.ModelMeanType.EPSILON,
                           model_var_type=vt, loss_type=gd.LossType.MSE, rescale_timesteps=rescale,
                           parameterization="v" if pred == "v" else "eps")


def tables_of(d):
    return {k: np.asarray(getattr(d, k), dtype=np.float64) for k in BC.TABLES}


def ref_terms(d, c, inp, dtype, t=None, clip=None):
    """The reference's functions on one op case; ``t`` / ``clip`` override the case's (the twins)."""
    from Disc_diff.guided_diffusion.nn import mean_flat
    x_start, noise, x_t, out = (inp[k].to(dtype) for k in ("x_start", "noise", "x_t", "out"))
    B = x_start.shape[0]
    tt = torch.tensor([inp["t"] if t is None else t] * B)
    clip = bool(c["clip"]) if clip is None else clip
    model = lambda x, ts, **kw: out
    r = d._vb_terms_bpd(model, x_start=x_start, x_t=x_t, t=tt, clip_denoised=clip)
    eps = d._predict_eps_from_xstart(x_t, tt, r["pred_xstart"])
    res = dict(vb=r["output"], xstart_mse=mean_flat((r["pred_xstart"] - x_start) ** 2), mse=mean_flat((eps - noise) ** 2))
    if BC.is_plane_case(c) and t is None and clip == bool(c["clip"]):
        p = d.p_mean_variance(model, x_t, tt, clip_denoised=clip)
        res.update(mean=p["mean"], log_variance=p["log_variance"], pred_xstart=p["pred_xstart"],
                   reverse=d.ddim_reverse_sample(model, x_t, tt, clip_denoised=clip)["sample"])
    return {k: v.numpy() for k, v in res.items()}


def gen_ops(out):
    cases = BC.op_cases()
    diffs = {(p, v): ref_diffusion(p, v, BC.RESPACING) for p in BC.PREDS for v in BC.VARS}
    tab = tables_of(diffs[("eps", "small")])
    T = len(tab["betas"])
    for k, v in tab.items():
        out["tab_" + k] = v
    out["tab_timestep_map"] = np.asarray(diffs[("eps", "small")].timestep_map, dtype=np.int64)
    n = len(cases)
    r32 = {q: np.zeros((n, BC.OP_B), np.float32) for q in BC.QUANTITIES}
    r64 = {q: np.zeros((n, BC.OP_B), np.float64) for q in BC.QUANTITIES}
    res32 = []
    for c in cases:
        d = diffs[(c["pred"], c["var"])]
        inp = BC.op_inputs(c, tab)
        a, b = ref_terms(d, c, inp, torch.float32), ref_terms(d, c, inp, torch.float64)
        assert a["vb"].dtype == np.float32 and b["vb"].dtype == np.float64
        res32.append(a)
        for q in BC.QUANTITIES:
            r32[q][c["i"]], r64[q][c["i"]] = a[q], b[q]
        if BC.is_plane_case(c):
            for pl in ("mean", "log_variance", "pred_xstart", "reverse"):
                out[f"plane_{c['i']}_{pl}"] = a[pl].astype(np.float32)
                out[f"plane64_{c['i']}_{pl}_rel"] = np.float64(np.linalg.norm(a[pl] - b[pl]) / np.linalg.norm(b[pl]))
    bars = {q: BC.rel(r32[q], r64[q]) for q in BC.QUANTITIES}
    for q in BC.QUANTITIES:
        out["op32_" + q], out["op64_" + q], out["bar_" + q] = r32[q], r64[q], np.float64(bars[q])
        worst = int(np.argmax(np.max(np.abs(r32[q] - r64[q]) / np.abs(r64[q]), axis=1)))
        print(f"op bar {q}: {bars[q]:.3e} (case {worst}: { {k: v for k, v in cases[worst].items()} })")
    # the prior of every input size (x_start of the first case of each (size, Cz))
    pr32, pr64, seen = [], [], []
    d = diffs[("eps", "small")]
    for c in cases:
        key = (tuple(c["size"]), c["cz"])
        if key in seen:
            continue
        seen.append(key)
        xs = BC.op_inputs(c, tab)["x_start"]
        pr32.append(d._prior_bpd(xs).numpy())
        pr64.append(d._prior_bpd(xs.double()).numpy())
    out["prior_case"] = np.asarray([next(c["i"] for c in cases if (tuple(c["size"]), c["cz"]) == k) for k in seen], dtype=np.int64)
    out["prior32"], out["prior64"] = np.stack(pr32), np.stack(pr64)
    bars["prior"] = BC.rel(out["prior32"], out["prior64"])
    out["bar_prior"] = np.float64(bars["prior"])
    print(f"op bar prior: {bars['prior']:.3e}")
    assert max(bars.values()) <= BAR_MAX, bars
    # twins: a loop or op that took the wrong step, the other fixed variance or dropped the clip cannot pass
    far = lambda a, b: max(BC.rel(a[q], b[q]) / bars[q] for q in BC.QUANTITIES)
    counts = {"t": 0, "var": 0, "clip": 0}
    other_var = {"small": "large", "large": "small", "range": "small"}
    for c in cases:
        d, inp, a = diffs[(c["pred"], c["var"])], BC.op_inputs(c, tab), res32[c["i"]]
        wrong_t = (inp["t"] + 1) % T if inp["t"] != 0 else 2
        assert far(ref_terms(d, c, inp, torch.float32, t=wrong_t), a) > TWIN_FACTOR, ("t", c)
        counts["t"] += 1
        if c["tn"] in ("t1", "mid") and c["var"] != "range":   # FIXED_SMALL and FIXED_LARGE share their t = 0 entry and nearly meet at T-1
            assert far(ref_terms(diffs[(c["pred"], other_var[c["var"]])], c, inp, torch.float32), a) > TWIN_FACTOR, ("var", c)
            counts["var"] += 1
        if c["clip"] and c["dist"] == 0.5 and c["tn"] == "last":   # the prediction leaves [-1, 1] by far
            assert far(ref_terms(d, c, inp, torch.float32, clip=False), a) > TWIN_FACTOR, ("clip", c)
            counts["clip"] += 1
    print("twins further than", TWIN_FACTOR, "bars:", counts)
    assert min(counts.values()) > 0
    out["op_cases"] = np.asarray(n)


class _Feed:
    def __init__(self, z):
        self.z, self.k = z, 0

    def __call__(self, *a, **kw):
        z = self.z[self.k]
        self.k += 1
        return z


def loop_net(name):
    """model(x, t, **model_kwargs) -> output tensor of a loop case's network, and its conditioning."""
    lc = BC.LOOP_CASES[name]
    if lc["net"] in ("tiny", "tinyfilm"):
        from UNet_DS_Diff.model import DSUnetModel
        gm = np.load(os.path.join(HERE, "model.npz"), allow_pickle=False)
        m = DSUnetModel(**json.loads(str(gm[lc["net"] + "_cfg"])))
        m.load_state_dict(_params(gm, lc["net"]), strict=True)
        m.eval()
        return lambda x, t, c: m(torch.cat([x, c], 1), t)[0]
    if lc["net"] == "lat":
        from ldm.modules.diffusionmodules.openaimodel import UNetModel
        gl = np.load(os.path.join(HERE, "latent_ldm.npz"), allow_pickle=False)
        m = UNetModel(**json.loads(str(gl["unet_cfg"])))
        m.load_state_dict(_params(gl, "unet"), strict=True)
        m.eval()
        return lambda x, t, c: m(torch.cat([x, c], 1), t)
    import dit_loops_util as DU
    return lambda x, t, c: DU.oracle_net(lc["net"], c)(x, t)


def gen_loops(out):
    for name, lc in BC.LOOP_CASES.items():
        d = ref_diffusion(lc["pred"], lc["var"], lc["respacing"], lc["rescale"])
        x_start, cond, z = BC.loop_inputs(name)
        net = loop_net(name)

        def run(perturb):
            gen = torch.Generator().manual_seed(PERTURB_SEED)

            def model(x, t, **kw):
                o = net(x, t, cond)
                if perturb:
                    o = o + PERTURB * o.pow(2).mean().sqrt() * torch.randn(o.shape, generator=gen)
                return o
            feed, orig = _Feed(z), torch.randn_like
            torch.randn_like = feed
            try:
                r = d.calc_bpd_loop(model, x_start, clip_denoised=bool(lc["clip"]))
            finally:
                torch.randn_like = orig
            assert feed.k == d.num_timesteps
            return {k: v.numpy() for k, v in r.items()}
        a, b = run(False), run(True)
        for k in ("vb", "xstart_mse", "mse", "prior_bpd", "total_bpd"):
            assert np.isfinite(a[k]).all(), (name, k)
            out[f"loop_{name}_{k}"] = a[k]
            out[f"loop_{name}_{k}_moved"] = np.abs(b[k].astype(np.float64) - a[k]) / np.abs(a[k])
            print(f"loop {name} {k}: shape {a[k].shape}, moved at most {out[f'loop_{name}_{k}_moved'].max():.2e} by {PERTURB:g} noise")
    out["loop_cases"] = json.dumps(BC.LOOP_CASES)


def main():
    out = {}
    gen_ops(out)
    gen_loops(out)
    path = os.path.join(HERE, "bpd.npz")
    np.savez_compressed(path, **out)
    print("wrote bpd.npz:", len(out), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
