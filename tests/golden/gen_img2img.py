#!/usr/bin/env python3
"""Generate tests/golden/img2img.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_img2img.py

Everything of the reference's DDIMSampler that starts from an image (ldm/models/diffusion/ddim.py): masked sampling
(sample(mask=, x0=), ddim_sampling :160-163), encode (:263-308), stochastic_encode (:310-324) and decode (:326-346), driven through
the DDPM stand-in of gen_cfg.py plus a q_sample (ddpm.py:356-359) whose draws come from a _NoiseFeed.

  latent cases  the UNetModel of latent_ldm.npz: B = 2, 4x8x8 state, 8 'concat' channels, 20 steps; c = randn(seed), u = zeros
  pixel cases   the `tiny` DSUnetModel of model.npz: B = 2, 1x32x32, cond / x_T seeds of loops.npz, u = zeros
  mask          [B,1,h,w], the centre half zero (the log_images form); x0 = randn(seed)
  masked runs   v-prediction (as cfg.npz), eta 0 / eta 1 / eta 0 at guidance scale 3, each beside the unmasked run with the same noise
  encode        parameterization "eps": 20 and 12 steps, unguided and at scale 3; the 12-step unguided run with
                return_intermediates = 3; decode of that latent from t_start = 12; stochastic_encode at indices (3, 17)

Stored: outputs, seeds and the configs' json only.  Weights regenerate from synth_params; inputs and noise from seeds.
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
from gen_cfg import _NoiseFeed, _params, shim, STEPS, SCALE  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_grad_enabled(False)
torch.set_num_threads(8)

T_ENC = 12
SENC_T = (3, 17)
SEEDS = dict(x0=720, step_eta0=721, step_eta1=722, blend_eta0=723, blend_eta1=724, blend_cfg=725, senc=726)


def center_mask(shape):
    b, _, h, w = shape
    m = torch.ones(b, 1, h, w)
    m[:, :, h // 4:h - h // 4, w // 4:w - w // 4] = 0.
    return m


def with_q_sample(s, feed):
    ext = lambda a, t, shp: a.gather(-1, t).reshape(t.shape[0], *((1,) * (len(shp) - 1)))
    s.q_sample = lambda x0, t: ext(s.sqrt_alphas_cumprod, t, x0.shape) * x0 + ext(s.sqrt_one_minus_alphas_cumprod, t,
                                                                                 x0.shape) * feed()
    return s


def ddim(s, x_T, c, u, eta, step_seed, blend_seed=None, x0=None, mask=None, scale=1.):
    import ldm.models.diffusion.ddim as ddim_mod
    feed, blend = _NoiseFeed(x_T.shape, step_seed, STEPS), _NoiseFeed(x_T.shape, blend_seed or 0, STEPS)
    with_q_sample(s, blend)
    orig = ddim_mod.noise_like
    ddim_mod.noise_like = lambda shp, dev, rep=False: feed()
    try:
        y, _ = ddim_mod.DDIMSampler(s, device=torch.device("cpu")).sample(
            STEPS, x_T.shape[0], tuple(x_T.shape[1:]), dict(c_concat=[c]), eta=eta, verbose=False, x_T=x_T.clone(), mask=mask,
            x0=x0, unconditional_guidance_scale=scale, unconditional_conditioning=dict(c_concat=[u]))
    finally:
        ddim_mod.noise_like = orig
    assert feed.k == STEPS and blend.k == (STEPS if mask is not None else 0)
    return y.numpy()


def space(out, sp, s, x_T, c, u):
    import ldm.models.diffusion.ddim as ddim_mod
    x0 = randn(tuple(x_T.shape), SEEDS["x0"])
    mask = center_mask(x_T.shape)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    s.parameterization = "v"
    for key, eta, ss, bs, sc in (("mask_eta0", 0., "step_eta0", "blend_eta0", 1.), ("mask_eta1", 1., "step_eta1", "blend_eta1", 1.),
                                 ("mask_cfg", 0., "step_eta0", "blend_cfg", SCALE)):
        out[f"{sp}_{key}_y"] = ddim(s, x_T, c, u, eta, SEEDS[ss], SEEDS[bs], x0, mask, sc)
        out[f"{sp}_{key}_nomask_y"] = ddim(s, x_T, c, u, eta, SEEDS[ss], scale=sc)
        print(sp, key, "rel-L2 masked against unmasked, same noise:", rel(out[f"{sp}_{key}_y"], out[f"{sp}_{key}_nomask_y"]))
        assert rel(out[f"{sp}_{key}_y"], out[f"{sp}_{key}_nomask_y"]) > 1e-2
    s.parameterization = "eps"
    smp = ddim_mod.DDIMSampler(s, device=torch.device("cpu"))
    smp.make_schedule(STEPS, ddim_eta=0., verbose=False)
    for key, n, sc in (("enc20", STEPS, 1.), ("enc12", T_ENC, 1.), ("enc20_cfg", STEPS, SCALE), ("enc12_cfg", T_ENC, SCALE)):
        y, o = smp.encode(x0.clone(), c, n, unconditional_guidance_scale=sc, unconditional_conditioning=u,
                          return_intermediates=3 if key == "enc12" else None)
        out[f"{sp}_{key}_y"] = y.numpy()
        if key == "enc12":
            out[f"{sp}_enc12_inter_steps"] = np.asarray(o["intermediate_steps"])
            out[f"{sp}_enc12_inter"] = torch.stack(o["intermediates"]).numpy()
    out[f"{sp}_dec12_y"] = smp.decode(torch.from_numpy(out[f"{sp}_enc12_y"]), c, T_ENC).numpy()
    print(sp, "decode(encode(x0)) over 12 steps, rel-L2 to x0:", rel(out[f"{sp}_dec12_y"], x0.numpy()))
    out[f"{sp}_senc_y"] = smp.stochastic_encode(x0, torch.tensor(SENC_T), noise=randn(tuple(x0.shape), SEEDS["senc"])).numpy()


def main():
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from UNet_DS_Diff.model import DSUnetModel
    out = {"steps": np.asarray(STEPS), "scale": np.float64(SCALE), "t_enc": np.asarray(T_ENC), "senc_t": np.asarray(SENC_T)}
    out.update({k + "_seed": np.asarray(v) for k, v in SEEDS.items()})

    gl = np.load(os.path.join(OUT, "latent_ldm.npz"), allow_pickle=False)
    ucfg = json.loads(str(gl["unet_cfg"]))
    m = UNetModel(**ucfg)
    m.load_state_dict(_params(gl, "unet"), strict=True)
    m.eval()
    c = randn((2, 8, 8, 8), 700)
    out.update({"lat_unet_cfg": json.dumps(ucfg), "lat_xT_seed": int(gl["xT_seed"]), "lat_c_seed": 700})
    space(out, "lat", shim(lambda x, t: m(x, t)), randn((2, 4, 8, 8), int(gl["xT_seed"])), c, torch.zeros_like(c))

    gm = np.load(os.path.join(OUT, "model.npz"), allow_pickle=False)
    go = np.load(os.path.join(OUT, "loops.npz"), allow_pickle=False)
    t = DSUnetModel(**json.loads(str(gm["tiny_cfg"])))
    t.load_state_dict(_params(gm, "tiny"), strict=True)
    t.eval()
    shape = (2, 1, 32, 32)
    c = cond_image(shape, int(go["cond_seed"]))
    out.update({"pix_cond_seed": int(go["cond_seed"]), "pix_xT_seed": int(go["xT_seed"])})
    space(out, "pix", shim(lambda x, tt: t(x, tt)[0]), randn(shape, int(go["xT_seed"])), c, torch.zeros_like(c))

    np.savez_compressed(os.path.join(OUT, "img2img.npz"), **out)
    print("wrote img2img", {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
