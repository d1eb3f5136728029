#!/usr/bin/env python3
"""Generate tests/golden/disc.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_disc.py

The reference's own Disc_diff.guided_diffusion.unet.SuperResModelNew (UNet_disc_Model, use_checkpoint=False, .eval()) run
unchanged — the four-stream DisC-Diff denoiser of configs/disc-diff.yaml / disc-diff-origin.yaml.  Stored:

  forwards   all nine outputs (com_h1..4, dist_h1..4, out) at integer t = [3, 700, 41][:B] and at t = [499.5, 20.0, 0.25][:B]
             tiny   model_channels 32, channel_mult (1,2), 1 res block, attention at ds 2, 16-channel heads, new attention order,
                    x_batch [2,4,16,24]
             film   channel_mult (1,1,3), attention at ds 1 and 2, 2 heads, use_scale_shift_norm, resblock_updown, out_channels 2,
                    x_batch [2,4,16,24]
             odd    channel_mult (1,2,3), 2 res blocks, attention at ds 4, 32-channel heads, x_batch [3,4,12,20]: a 3x5 bottleneck
                    (15 pixels), 48-channel halves, Cr = 6
  chains     the reference's own SpacedDiffusion (1000 steps respaced to 10, eps prediction) over SuperResModelNew with
             model_kwargs = dict(t1, t2, dwi), x_T and the per-step normals fed (torch.randn_like replaced by a feeder):
             tiny_ddim  ddim_sample_loop eta 0     tiny_ddpm  p_sample_loop, FIXED_LARGE
             film_ddpm  p_sample_loop, learn_sigma (LEARNED_RANGE; the model's two output channels)
Weights are not stored: (names, shapes, seed) only, rebuilt through oracle.synth.synth_params (every zero_module of the
reference is re-randomised); inputs and noise come from oracle.synth.randn seeds.

Asserted here, values as printed by this script (8 threads):
  a stream mix-up cannot pass: swapping T1 and T2 / replacing DWI moves `out` by (relative L2)
      tiny 1.125 / 0.990    film 1.038 / 0.813    odd 1.193 / 0.904                                    (bar: > 0.1)
  3e-6 relative noise on every network output moves the chains by
      tiny_ddim 1.93e-06    tiny_ddpm 1.04e-06    film_ddpm 2.40e-06                                      (bar: < 2e-5)
Recorded (``<key>_ref_f32_vs_f64``): the reference's float32 against float64, `out` / worst of the eight features
      tiny 1.45e-06 / 4.5e-07    film 1.29e-06 / 6.0e-07    odd 1.03e-06 / 6.8e-07
  The reference cannot itself run in float64 (its GroupNorm32 hands float32 inputs to the module's parameters), so the float64
  side is tests/disc_ref.py, which this script first holds against the reference in float32: every one of the nine outputs of
  every forward, and all three chains, came out bit-equal (rel-L2 0.0) on this build of torch.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))          # tests/: disc_ref
sys.path.insert(0, os.environ.get("DSD_REFERENCE", "/root/reference"))
sys.dont_write_bytecode = True

from oracle import samplers as OS  # noqa: E402
from oracle.synth import synth_params, randn  # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(int(os.environ.get("DSD_GEN_THREADS", "8")))

# key -> (constructor keywords, x_batch shape, weight seed, input seed)
CFG = {
    "tiny": (dict(image_size=16, in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
                  channel_mult=[1, 2], num_head_channels=16, use_new_attention_order=True), (2, 4, 16, 24), 610, 611),
    "film": (dict(image_size=16, in_channels=1, model_channels=32, out_channels=2, num_res_blocks=1, attention_resolutions=[1, 2],
                  channel_mult=[1, 1, 3], num_heads=2, use_scale_shift_norm=True, resblock_updown=True), (2, 4, 16, 24), 620, 621),
    "odd": (dict(image_size=16, in_channels=1, model_channels=32, out_channels=1, num_res_blocks=2, attention_resolutions=[4],
                 channel_mult=[1, 2, 3], num_head_channels=32), (3, 4, 12, 20), 630, 631),
}
T_INT, T_FLOAT = [3, 700, 41], [499.5, 20.0, 0.25]
# name -> (model, ddim, eta, learn_sigma, x_T seed, plane seeds, noise seed)
CHAINS = {
    "tiny_ddim": ("tiny", True, 0.0, False, 640, (641, 642, 643), 644),
    "tiny_ddpm": ("tiny", False, 0.0, False, 650, (651, 652, 653), 654),
    "film_ddpm": ("film", False, 0.0, True, 660, (661, 662, 663), 664),
}
STEPS, SHAPE = 10, (2, 1, 16, 24)


class _Feed:
    def __init__(self, z):
        self.z, self.k = z, 0

    def __call__(self, *a, **kw):
        z = self.z[self.k]
        self.k += 1
        return z


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    import contextlib
    import io
    import Disc_diff.guided_diffusion.gaussian_diffusion as gd
    from Disc_diff.guided_diffusion.respace import SpacedDiffusion, space_timesteps
    from Disc_diff.guided_diffusion.unet import SuperResModelNew
    import disc_ref as R
    out, nets = {}, {}
    for key, (kw, shp, wseed, xseed) in CFG.items():
        with contextlib.redirect_stdout(io.StringIO()):                       # (the constructor prints image_size)
            m = SuperResModelNew(**kw, use_checkpoint=False).eval()
        ns = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        sd = synth_params(ns, wseed)
        m.load_state_dict(sd, strict=True)
        nets[key] = (m, kw, sd)
        x = randn(shp, xseed)
        B = shp[0]
        out.update({key + "_cfg": json.dumps(kw), key + "_params": json.dumps([[n, list(s)] for n, s in ns]), key + "_seed": wseed,
                    key + "_xshape": np.asarray(shp), key + "_xseed": xseed})
        for tag, t in (("int", torch.tensor(T_INT[:B])), ("float", torch.tensor(T_FLOAT[:B]))):
            got = m(x, t)
            assert len(got) == 9
            out[f"{key}_t_{tag}"] = t.numpy()
            for i, v in enumerate(got):
                out[f"{key}_{tag}_{i}"] = v.numpy()
            ref = R.disc_forward(kw, sd, x, t)
            print(f"{key} t {tag}: disc_ref vs reference, worst of nine rel-L2 {max(rel(a, b) for a, b in zip(ref, got)):.3e}")
        t = torch.tensor(T_INT[:B])
        base = m(x, t)
        swap = m(x[:, [0, 2, 1, 3]], t)[8]
        dwi = m(torch.cat([x[:, :3], randn((B, 1) + shp[2:], xseed + 5)], 1), t)[8]
        e_swap, e_dwi = rel(swap, base[8]), rel(dwi, base[8])
        print(f"{key}: swapping T1/T2 moves out by {e_swap:.3f}, replacing DWI by {e_dwi:.3f}")
        assert e_swap > 0.1 and e_dwi > 0.1
        # the reference itself cannot run in float64 (its GroupNorm32 forces float32 inputs onto the module's parameters), so the
        # float64 yardstick is tests/disc_ref.py, pinned to the reference's float32 by the comparison above
        full = R.disc_forward(kw, sd, x, t, dtype=torch.float64)
        f_out, f_feat = rel(base[8], full[8]), max(rel(a, b) for a, b in zip(base[:8], full[:8]))
        out[key + "_ref_f32_vs_f64"] = np.asarray([f_out, f_feat])
        print(f"{key}: reference float32 vs disc_ref in float64: out {f_out:.3e}, worst feature {f_feat:.3e}")

    for name, (key, ddim, eta, learn_sigma, xseed, pseeds, nseed) in CHAINS.items():
        m, kw, sd = nets[key]
        diff = SpacedDiffusion(use_timesteps=space_timesteps(1000, str(STEPS)), betas=gd.get_named_beta_schedule("linear", 1000),
                               model_mean_type=gd.ModelMeanType.EPSILON,
                               model_var_type=gd.ModelVarType.LEARNED_RANGE if learn_sigma else gd.ModelVarType.FIXED_LARGE,
                               loss_type=gd.LossType.MSE, rescale_timesteps=False, parameterization="eps")
        x_T = randn(SHAPE, xseed)
        planes = [randn(SHAPE, s) for s in pseeds]
        z = randn((STEPS,) + SHAPE, nseed)

        def run(model):
            feed, orig = _Feed(z), torch.randn_like
            torch.randn_like = feed
            try:
                fn = diff.ddim_sample_loop if ddim else diff.p_sample_loop
                y = fn(model, SHAPE, noise=x_T.clone(), clip_denoised=True, model_kwargs=dict(t1=planes[0], t2=planes[1], dwi=planes[2]),
                       device="cpu", **(dict(eta=eta) if ddim else {}))
            finally:
                torch.randn_like = orig
            assert feed.k == STEPS
            return y
        y = run(m)

        class Noisy(torch.nn.Module):                                        # 3e-6 relative noise on every network output
            def __init__(self):
                super().__init__()
                self.k = 0

            def forward(self, x, t, **kwargs):
                o = m(x, t, **kwargs)
                self.k += 1
                return o[:8] + (o[8] * (1 + 3e-6 * randn(tuple(o[8].shape), 7000 + self.k)),)
        e_noise = rel(run(Noisy()), y)
        ora = OS.DiffusionA(steps=1000, timestep_respacing=str(STEPS), learn_sigma=learn_sigma, parameterization="eps")
        net = lambda x_in, t: R.disc_forward(kw, sd, x_in, t)[8]
        want = (ora.ddim_sample_loop(net, x_T, z, cond=planes, eta=eta) if ddim else ora.p_sample_loop(net, x_T, z, cond=planes))
        print(f"{name}: 3e-6 output noise moves the chain by {e_noise:.3e}; disc_ref chain vs reference {rel(want, y):.3e}; "
              f"max |y| {float(y.abs().max()):.3f}")
        assert e_noise < 2e-5
        out.update({name + "_model": key, name + "_ddim": int(ddim), name + "_eta": np.float64(eta), name + "_learn_sigma": int(learn_sigma),
                    name + "_steps": STEPS, name + "_shape": np.asarray(SHAPE), name + "_xT_seed": xseed,
                    name + "_plane_seeds": np.asarray(pseeds), name + "_noise_seed": nseed, name + "_y": y.numpy()})
    if os.environ.get("DSD_GEN_DRY"):
        return
    np.savez_compressed(os.path.join(HERE, "disc.npz"), **out)
    print("wrote disc.npz", os.path.getsize(os.path.join(HERE, "disc.npz")), "bytes")


if __name__ == "__main__":
    main()
