#!/usr/bin/env python3
"""Generate tests/golden/trace.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_trace.py

The intermediates and per-step callbacks of the reference's own samplers: DDIMSampler.sample (ldm/models/diffusion/ddim.py:
149,178-183), PLMSSampler.sample (plms.py:139,169-174) through the DDPM stand-in of gen_cfg.py with the q_sample of
gen_img2img.py, and LatentDiffusion.p_sample_loop / progressive_denoising (ddpm.py:991-1093) run as they stand on a subclass that
skips the constructor (no first stage, no Lightning) and keeps register_schedule, p_sample, p_mean_variance and q_posterior.
ddpm.py imports packages this container lacks (Lightning, torchvision, diffusers, ...): a finder answers those imports with empty
modules; none of their code is reached by the loops.

  lat  the UNetModel of latent_ldm.npz: B = 2, 4x8x8 state, 8 'concat' channels; c = randn(seed), u = zeros
  pix  the `tiny` DSUnetModel of model.npz: B = 2, 1x32x32, cond / x_T seeds of loops.npz

Every case runs with callback and img_callback installed.  Stored per case: every kept x_inter / pred_x0 entry, the loop
iterations they belong to (found by object identity: the samplers append the very tensors they hand to img_callback or get back
from the step), the argument sequence each callback saw, the tensors img_callback received at two steps (ICB_AT), the sample.
Seeds and configs as json; no weights.

As gen_plms.py does, every case is re-run with Gaussian noise of 3e-6 relative RMS on every network output, and EVERY stored
entry, taken separately, must move by less than 2e-5 relative L2 (the stack would hide an early pred_x0, which divides by
sqrt(alpha_t), behind x_T's norm).  Changed for that bar: the guided case runs S = 4 with log_every_t 2 instead of S = 7 with
3 — guidance at scale 3 multiplies the perturbation of an eps prediction (|1 - s| + |s| = 5), and with S = 7 the reference alone
moved its later entries by up to 6e-5 (lat) / 1.2e-4 (pix); with S = 4 every entry stays below 1.6e-5.  The pixel ddim_log3
runs S = 5 (5 executed steps): at S = 7 its third pred_x0 entry moved by 2.01e-5.
"""
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

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
THR = 2.0
SEEDS = dict(x0=760, step=761, blend=762, perturb=763)
PERTURB = 3e-6
MOVE_MAX = 2e-5
DDPM_T = 12
# name -> sampler, steps, log_every_t, and what differs from (eps, eta 0, unguided, unmasked, no threshold)
CASES = {
    "ddim_log3": dict(kind="ddim", steps=7, log=3),
    "ddim_log1": dict(kind="ddim", steps=7, log=1),
    "ddim_log100": dict(kind="ddim", steps=7, log=100),
    "ddim_eta1": dict(kind="ddim", steps=7, log=3, eta=1.),
    "ddim_cfg": dict(kind="ddim", steps=4, log=2, scale=SCALE),           # S = 4: see the docstring
    "ddim_mask": dict(kind="ddim", steps=7, log=3, mask=True),
    "ddim_v": dict(kind="ddim", steps=7, log=3, param="v"),
    "plms_log2": dict(kind="plms", steps=6, log=2),
    "plms_log2_thr": dict(kind="plms", steps=6, log=2, thr=THR),
    "ddpm_log5": dict(kind="ddpm", steps=DDPM_T, log=5),
    "ddpm_log5_mask": dict(kind="ddpm", steps=DDPM_T, log=5, mask=True),
    "prog_log5": dict(kind="prog", steps=DDPM_T, log=5),
}
# the four-stream model (a dense state) runs a subset; its ddim_log3 runs S = 5 (docstring)
PIX_CASES = {k: CASES[k] for k in ("ddim_log3", "ddim_cfg", "plms_log2_thr", "ddpm_log5_mask", "prog_log5")}
PIX_CASES["ddim_log3"] = dict(kind="ddim", steps=5, log=3)
ICB_AT = lambda steps: (1, steps - 1)        # the iterations whose img_callback tensor is stored

rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))


def executed(case):
    """The iterations a case executes: the 'uniform' discretisation of S on 1000 steps is range(0, 1000, 1000 // S), so S = 7
    executes 8 and S = 6 executes 7 (ddim.py make_schedule -> make_ddim_timesteps); the DDPM loops execute ``steps``."""
    if case["kind"] in ("ddim", "plms"):
        from ldm.modules.diffusionmodules.util import make_ddim_timesteps
        return int(make_ddim_timesteps("uniform", case["steps"], 1000, verbose=False).shape[0])
    return case["steps"]


ABSENT = ("pytorch_lightning", "lightning", "torchvision", "omegaconf", "diffusers", "taming", "monai", "SimpleITK", "sklearn", "cv2",
          "h5py", "training_project", "nibabel", "skimage")


class _Empty(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name == "rank_zero_only":
            return lambda f: f
        return type(name, (nn.Module,), {})


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in ABSENT:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _Empty(spec.name)

    def exec_module(self, module):
        pass


def reference_ddpm():
    sys.meta_path.insert(0, _Finder())
    import ldm.models.diffusion.ddpm as ddpm_mod
    return ddpm_mod


def stand_in(ddpm_mod, net, clip_denoised):
    """LatentDiffusion without its constructor: the schedule of register_schedule (defaults: linear, 1000 steps), apply_model =
    DiffusionWrapper 'concat' on ``net``; p_sample records what it returns, so entries can be matched to iterations."""
    class Stand(ddpm_mod.LatentDiffusion):
        device = torch.device("cpu")

        def __init__(self):
            nn.Module.__init__(self)
            self.parameterization, self.v_posterior = "eps", 0.
            self.clip_denoised, self.log_every_t, self.num_timesteps_cond = clip_denoised, 100, 1
            self.register_schedule()                                     # LatentDiffusion's: DDPM's + shorten_cond_schedule = False
            assert not self.shorten_cond_schedule
            self.returned = []

        def apply_model(self, x, t, c, return_ids=False):
            return net[0](torch.cat([x, c], 1), t)

        def p_sample(self, *a, **kw):
            out = ddpm_mod.LatentDiffusion.p_sample(self, *a, **kw)
            self.returned.append(out)
            return out
    return Stand()


def _perturbed(apply, on, gen):
    def apply_model(x, t, cc, *a, **kw):
        out = apply(x, t, cc, *a, **kw)
        if on:
            out = out + PERTURB * out.pow(2).mean().sqrt() * torch.randn(out.shape, generator=gen)
        return out
    return apply_model


def run(env, case, perturb=False):
    """One run of the reference -> dict(y, x=[...], p0=[...], keep=[...], cb=[...], icb=[...], icb_t={k: tensor})."""
    kind, S, steps, log = case["kind"], case["steps"], executed(case), case["log"]
    x_T, c, u = env["xT"], env["c"], env["u"]
    masked = bool(case.get("mask"))
    x0, mask = (env["x0"], env["mask"]) if masked else (None, None)
    gen = torch.Generator().manual_seed(SEEDS["perturb"])
    feed, blend = _NoiseFeed(x_T.shape, SEEDS["step"], steps), _NoiseFeed(x_T.shape, SEEDS["blend"], steps)
    cb, icb, seen = [], [], []
    callback = lambda i: cb.append(int(i))

    def img_callback(t, i):
        icb.append(int(i))
        seen.append(t)
    res = {}
    if kind in ("ddim", "plms"):
        import ldm.models.diffusion.ddim as ddim_mod
        import ldm.models.diffusion.plms as plms_mod
        s = env["shim"]
        s.parameterization = case.get("param", "eps")
        with_q_sample(s, blend)
        apply = s.apply_model
        s.apply_model = _perturbed(apply, perturb, gen)
        orig = ddim_mod.noise_like
        ddim_mod.noise_like = lambda shp, dev, rep=False: feed()
        try:
            kw = dict(callback=callback, img_callback=img_callback, eta=case.get("eta", 0.), verbose=False, x_T=x_T, mask=mask, x0=x0,
                      log_every_t=log, unconditional_guidance_scale=case.get("scale", 1.))
            if kind == "ddim":
                y, inter = ddim_mod.DDIMSampler(s, device=torch.device("cpu")).sample(
                    S, x_T.shape[0], tuple(x_T.shape[1:]), dict(c_concat=[c]), unconditional_conditioning=dict(c_concat=[u]), **kw)
            else:
                y, inter = plms_mod.PLMSSampler(s, device=torch.device("cpu")).sample(
                    S, x_T.shape[0], tuple(x_T.shape[1:]), c, unconditional_conditioning=u, dynamic_threshold=case.get("thr"), **kw)
        finally:
            s.apply_model, ddim_mod.noise_like = apply, orig
        assert inter["x_inter"][0] is x_T and inter["pred_x0"][0] is x_T and inter["x_inter"][-1] is y
        # img_callback got the very pred_x0 objects the sampler appends
        keep = [next(k for k, t in enumerate(seen) if t is p) for p in inter["pred_x0"][1:]]
        res.update(x=inter["x_inter"][1:], p0=inter["pred_x0"][1:])
        assert feed.k == (steps if kind == "ddim" else 0)
    else:
        ddpm_mod = env["ddpm_mod"]
        st = env["stand"]
        st.returned = []
        with_q_sample(st, blend)
        apply = st.apply_model
        st.apply_model = _perturbed(apply, perturb, gen)
        orig = ddpm_mod.noise_like
        ddpm_mod.noise_like = lambda shp, dev, rep=False: feed()
        try:
            if kind == "ddpm":
                y, inter = st.p_sample_loop(c, tuple(x_T.shape), return_intermediates=True, x_T=x_T, verbose=False, callback=callback,
                                            timesteps=steps, mask=mask, x0=x0, img_callback=img_callback, log_every_t=log)
                assert inter[0] is x_T and inter[-1] is y
                keep = [next(k for k, t in enumerate(seen) if t is p) for p in inter[1:]]    # img_callback got the appended img
                res.update(x=inter[1:], p0=[])
            else:
                y, inter = st.progressive_denoising(c, tuple(x_T.shape), verbose=False, callback=callback, img_callback=img_callback,
                                                    mask=mask, x0=x0, x_T=x_T, start_T=steps, log_every_t=log)
                keep = [next(k for k, r in enumerate(st.returned) if r[1] is p) for p in inter]  # x0_partial of p_sample's return
                res.update(x=[], p0=inter)
        finally:
            del st.apply_model
            ddpm_mod.noise_like = orig
        assert feed.k == steps
    assert blend.k == (steps if masked else 0)
    assert len(cb) == len(icb) == len(seen) == steps
    res.update(y=y, keep=keep, cb=cb, icb=icb, icb_t={k: seen[k] for k in ICB_AT(steps)})
    return {k: ([t.numpy().copy() for t in v] if k in ("x", "p0") else v) for k, v in res.items()}


def space(out, sp, env):
    for name, case in (PIX_CASES if sp == "pix" else CASES).items():
        if case["kind"] in ("ddpm", "prog"):
            env["stand"] = env["stand_clip"] if sp == "pix" else env["stand_noclip"]
        r = run(env, case)
        p = run(env, case, perturb=True)
        assert p["keep"] == r["keep"] and p["cb"] == r["cb"] and p["icb"] == r["icb"]
        key = f"{sp}_{name}"
        moves = {}
        for part in ("x", "p0"):
            for j, (a, b) in enumerate(zip(p[part], r[part])):
                moves[f"{part}{j}"] = rel(a, b)
                out[f"{key}_{part}{j}"] = b
        for k, t in r["icb_t"].items():
            moves[f"icb{k}"] = rel(p["icb_t"][k].numpy(), t.numpy())
            out[f"{key}_icb{k}"] = t.numpy().copy()
        if not r["x"]:                                                        # elsewhere the sample is the last x entry
            out[f"{key}_y"] = r["y"].numpy().copy()
        out[f"{key}_keep"] = np.asarray(r["keep"], dtype=np.int32)
        out[f"{key}_cb"] = np.asarray(r["cb"], dtype=np.int32)
        out[f"{key}_icb"] = np.asarray(r["icb"], dtype=np.int32)
        worst = max(moves, key=moves.get)
        print(f"{key}: keep {r['keep']} cb {r['cb'][:3]}.. entries moved at most {moves[worst]:.2e} ({worst}) by {PERTURB:g} noise on "
              f"the network output; max |pred_x0| {max([np.abs(a).max() for a in r['p0']] or [0]):.2f}")
        bad = {k: v for k, v in moves.items() if not v < MOVE_MAX}
        assert not bad, (key, bad)


def main():
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from UNet_DS_Diff.model import DSUnetModel
    ddpm_mod = reference_ddpm()
    out = {"scale": np.float64(SCALE), "thr": np.float64(THR), "lat_cases": json.dumps(CASES), "pix_cases": json.dumps(PIX_CASES),
           "lat_executed": json.dumps({k: executed(v) for k, v in CASES.items()}),
           "pix_executed": json.dumps({k: executed(v) for k, v in PIX_CASES.items()})}
    out.update({k + "_seed": np.asarray(v) for k, v in SEEDS.items()})

    gl = np.load(os.path.join(OUT, "latent_ldm.npz"), allow_pickle=False)
    ucfg = json.loads(str(gl["unet_cfg"]))
    m = UNetModel(**ucfg)
    m.load_state_dict(_params(gl, "unet"), strict=True)
    m.eval()
    shape = (2, 4, 8, 8)
    c = randn((2, 8, 8, 8), 700)
    out.update({"lat_unet_cfg": json.dumps(ucfg), "lat_xT_seed": int(gl["xT_seed"]), "lat_c_seed": 700})
    net = [lambda x, t: m(x, t)]
    space(out, "lat", dict(shim=shim(net[0]), ddpm_mod=ddpm_mod, stand_noclip=stand_in(ddpm_mod, net, False), xT=randn(shape, int(gl["xT_seed"])),
                           c=c, u=torch.zeros_like(c), x0=randn(shape, SEEDS["x0"]), mask=center_mask(shape)))

    gm = np.load(os.path.join(OUT, "model.npz"), allow_pickle=False)
    go = np.load(os.path.join(OUT, "loops.npz"), allow_pickle=False)
    t = DSUnetModel(**json.loads(str(gm["tiny_cfg"])))
    t.load_state_dict(_params(gm, "tiny"), strict=True)
    t.eval()
    shape = (2, 1, 32, 32)
    c = cond_image(shape, int(go["cond_seed"]))
    out.update({"pix_cond_seed": int(go["cond_seed"]), "pix_xT_seed": int(go["xT_seed"])})
    net = [lambda x, tt: t(x, tt)[0]]
    space(out, "pix", dict(shim=shim(net[0]), ddpm_mod=ddpm_mod, stand_clip=stand_in(ddpm_mod, net, True), xT=randn(shape, int(go["xT_seed"])),
                           c=c, u=torch.zeros_like(c), x0=randn(shape, SEEDS["x0"]), mask=center_mask(shape)))

    np.savez_compressed(os.path.join(OUT, "trace.npz"), **out)
    print("wrote trace", len(out), "arrays,", os.path.getsize(os.path.join(OUT, "trace.npz")), "bytes")


if __name__ == "__main__":
    main()
