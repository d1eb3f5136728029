#!/usr/bin/env python3
"""Generate tests/golden/plms.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_plms.py

The reference's own PLMSSampler.sample (ldm/models/diffusion/plms.py) with parameterization "eps", tensor conditioning, u = zeros,
eta = 0, driven through the DDPM stand-in of gen_cfg.py plus the q_sample of gen_img2img.py (draws from a _NoiseFeed).

  latent cases  the UNetModel of latent_ldm.npz: B = 2, 4x8x8 state, 8 'concat' channels; c = randn(seed)
  pixel cases   the `tiny` DSUnetModel of model.npz: B = 2, 1x32x32, cond / x_T seeds of loops.npz
  mask          [B,1,h,w], the centre half zero; x0 = randn(seed); every masked case beside its unmasked twin
  threshold     dynamic_threshold (norm_thresholding) beside the unthresholded twin

Two checks run here so the fixture can be neither vacuous nor ill-conditioned: the threshold engages (rms > v) in some but not
all of the S + 1 update calls of every thresholded case and moves the result by more than 1e-2; and every stored case, re-run
with Gaussian noise of 3e-6 relative RMS on every network output (the size of the GPU-against-oracle forward error), moves by
less than 2e-5 — a fifth of the 1e-4 chain bar the GPU tests hold it to.

Stored: outputs, seeds, tables and the configs' json only.  Weights regenerate from synth_params; inputs and noise from seeds.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ["DSD_REFERENCE"])
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

from oracle.synth import randn, cond_image  # noqa: E402
from gen_cfg import _NoiseFeed, _params, shim  # noqa: E402
from gen_img2img import center_mask, with_q_sample  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_grad_enabled(False)
torch.set_num_threads(8)

SCALE = 3.0
SEEDS = dict(x0=740, blend=741, blend_cfg=742, blend_thr=743, perturb=744)
PERTURB = 3e-6            # relative RMS of the perturbation of every network output
MOVE_MAX = 2e-5
LAT_THR, PIX_THR = 2.0, 2.0
# name -> (steps, guidance scale, blend-noise seed name or None, thresholded, twin)
LAT_CASES = {
    "plms20": (20, 1., None, False, None),
    "plms_s1": (1, 1., None, False, None), "plms_s2": (2, 1., None, False, None),
    "plms_s4": (4, 1., None, False, None), "plms_s5": (5, 1., None, False, None),
    "plms_cfg": (20, SCALE, None, False, None),
    "plms_mask": (20, 1., "blend", False, "plms20"),
    "plms_mask_cfg": (20, SCALE, "blend_cfg", False, "plms_cfg"),
    "plms_s10": (10, 1., None, False, None),
    "plms_thr": (10, 1., None, True, "plms_s10"),
    "plms_mask_cfg_s10": (10, SCALE, "blend_thr", False, None),
    "plms_mask_cfg_thr": (10, SCALE, "blend_thr", True, "plms_mask_cfg_s10"),
}
PIX_CASES = {
    "plms20": (20, 1., None, False, None),
    "plms_cfg": (20, SCALE, None, False, None),
    "plms_mask": (20, 1., "blend", False, "plms20"),
    "plms_s10": (10, 1., None, False, None),
    "plms_thr": (10, 1., None, True, "plms_s10"),
}

rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))


def plms(s, x_T, c, u, steps, scale, blend_seed, x0, mask, thr, perturb=False, trace=None):
    """One run of the reference's sampler.  ``perturb``: Gaussian noise of PERTURB relative RMS on every network output;
    ``trace``: a list that receives (per-sample rms of pred_x0, v) of every norm_thresholding call."""
    import ldm.models.diffusion.plms as plms_mod
    blend = _NoiseFeed(x_T.shape, blend_seed or 0, steps)
    with_q_sample(s, blend)
    apply, count = s.apply_model, [0]
    gen = torch.Generator().manual_seed(SEEDS["perturb"])

    def apply_model(x, t, cc):
        count[0] += 1
        out = apply(x, t, cc)
        if perturb:
            out = out + PERTURB * out.pow(2).mean().sqrt() * torch.randn(out.shape, generator=gen)
        return out
    norm = plms_mod.norm_thresholding

    def norm_thresholding(p0, value):
        if trace is not None:
            trace.append((p0.pow(2).flatten(1).mean(1).sqrt().numpy().copy(), value))
        return norm(p0, value)
    s.apply_model, plms_mod.norm_thresholding = apply_model, norm_thresholding
    try:
        y, _ = plms_mod.PLMSSampler(s, device=torch.device("cpu")).sample(
            steps, x_T.shape[0], tuple(x_T.shape[1:]), c, eta=0., verbose=False, x_T=x_T.clone(), mask=mask, x0=x0,
            unconditional_guidance_scale=scale, unconditional_conditioning=u, dynamic_threshold=thr)
    finally:
        s.apply_model, plms_mod.norm_thresholding = apply, norm
    assert count[0] == steps + 1, (count[0], steps)                           # the first step evaluates twice
    assert blend.k == (steps if mask is not None else 0)
    return y.numpy()


def space(out, sp, s, x_T, c, cases, v):
    u = torch.zeros_like(c)
    x0, mask = randn(tuple(x_T.shape), SEEDS["x0"]), center_mask(x_T.shape)
    s.parameterization = "eps"
    for name, (steps, scale, bs, thresholded, twin) in cases.items():
        kw = dict(steps=steps, scale=scale, blend_seed=SEEDS[bs] if bs else None, x0=x0 if bs else None, mask=mask if bs else None,
                  thr=v if thresholded else None)
        trace = []
        y = out[f"{sp}_{name}_y"] = plms(s, x_T, c, u, trace=trace, **kw)
        move = rel(plms(s, x_T, c, u, perturb=True, **kw), y)
        print(f"{sp}_{name}: max |y| {np.abs(y).max():.3f}, moved {move:.2e} by {PERTURB:g} noise on the network output")
        assert move < MOVE_MAX, (sp, name, move)
        if thresholded:
            assert len(trace) == steps + 1
            engaged = [bool((r > val).any()) for r, val in trace]
            print(f"{sp}_{name}: threshold {v} engaged in {sum(engaged)} of {len(trace)} update calls; rms per call:",
                  [np.round(r, 3).tolist() for r, _ in trace])
            assert 0 < sum(engaged) < len(trace), (sp, name)
        if twin:
            d = rel(y, out[f"{sp}_{twin}_y"])
            print(f"{sp}_{name}: rel-L2 to its twin {twin} {d:.3f}")
            assert d > 1e-2, (sp, name, d)


def main():
    import ldm.models.diffusion.plms as plms_mod
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from UNet_DS_Diff.model import DSUnetModel
    out = {"scale": np.float64(SCALE), "lat_thr": np.float64(LAT_THR), "pix_thr": np.float64(PIX_THR),
           "lat_cases": json.dumps(LAT_CASES), "pix_cases": json.dumps(PIX_CASES)}
    out.update({k + "_seed": np.asarray(v) for k, v in SEEDS.items()})

    gl = np.load(os.path.join(OUT, "latent_ldm.npz"), allow_pickle=False)
    ucfg = json.loads(str(gl["unet_cfg"]))
    m = UNetModel(**ucfg)
    m.load_state_dict(_params(gl, "unet"), strict=True)
    m.eval()
    c = randn((2, 8, 8, 8), 700)
    out.update({"lat_unet_cfg": json.dumps(ucfg), "lat_xT_seed": int(gl["xT_seed"]), "lat_c_seed": 700})
    s = shim(lambda x, t: m(x, t))
    space(out, "lat", s, randn((2, 4, 8, 8), int(gl["xT_seed"])), c, LAT_CASES, LAT_THR)

    # the reference's tables for 20 steps (make_schedule :47-53): what PLMSSampler._schedule must pack
    smp = plms_mod.PLMSSampler(s, device=torch.device("cpu"))
    smp.make_schedule(20, verbose=False)
    out.update({"ddim_timesteps": np.asarray(smp.ddim_timesteps), "ddim_alphas": np.asarray(smp.ddim_alphas),
                "ddim_alphas_prev": np.asarray(smp.ddim_alphas_prev),
                "ddim_sqrt_one_minus_alphas": np.asarray(smp.ddim_sqrt_one_minus_alphas), "ddim_sigmas": np.asarray(smp.ddim_sigmas)})

    gm = np.load(os.path.join(OUT, "model.npz"), allow_pickle=False)
    go = np.load(os.path.join(OUT, "loops.npz"), allow_pickle=False)
    t = DSUnetModel(**json.loads(str(gm["tiny_cfg"])))
    t.load_state_dict(_params(gm, "tiny"), strict=True)
    t.eval()
    shape = (2, 1, 32, 32)
    c = cond_image(shape, int(go["cond_seed"]))
    out.update({"pix_cond_seed": int(go["cond_seed"]), "pix_xT_seed": int(go["xT_seed"])})
    space(out, "pix", shim(lambda x, tt: t(x, tt)[0]), randn(shape, int(go["xT_seed"])), c, PIX_CASES, PIX_THR)

    np.savez_compressed(os.path.join(OUT, "plms.npz"), **out)
    print("wrote plms", {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
