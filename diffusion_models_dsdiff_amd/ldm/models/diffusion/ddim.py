"""DDIMSampler — drop-in for ldm/models/diffusion/ddim.py (make_schedule :25-55, sample :57-126,
ddim_sampling :128-185, p_sample_ddim :187-261), executed by dsd_sample (mode B_DDIM); with
``unconditional_guidance_scale`` / ``unconditional_conditioning`` / ``ucg_schedule`` by dsd_sample with a dsd_guidance; with ``mask`` / ``x0``
by dsd_sample with a dsd_inpaint.  encode :263-308 runs dsd_invert, stochastic_encode :310-324 dsd_op_q_sample, decode :326-346 the tail of
the sampling loop."""
from __future__ import annotations

import numpy as np
import torch

from .... import _lib
from ...._sched import (Guidance, Inpaint, Schedule, StepCallbacks, Trace, cat_conditioning, cat_unconditional, find_unet,
                         guidance_active, wrapper_key, invert_coefficients, kept_iterations, philox_seed, q_sample_rows,
                         run_device_loop, run_invert_loop)


class MaskWithoutX0(AssertionError, NotImplementedError):
    """``mask`` without ``x0``: the reference asserts (ddim.py:161); this sampler used to answer every mask with
    NotImplementedError.  Callers written against either keep working."""


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=True):
    """ldm/modules/diffusionmodules/util.py:53-67 (+1 offset kept)."""
    if ddim_discr_method == "uniform":
        stride = num_ddpm_timesteps // num_ddim_timesteps
        steps = np.asarray(list(range(0, num_ddpm_timesteps, stride)))
    elif ddim_discr_method == "quad":
        steps = ((np.linspace(0, np.sqrt(num_ddpm_timesteps * .8), num_ddim_timesteps)) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    steps_out = steps + 1
    if verbose:
        print(f"Selected timesteps for ddim sampler: {steps_out}")
    return steps_out


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=True):
    """util.py:70-81; ``alphacums`` = the model's fp32 alphas_cumprod buffer as a numpy array."""
    a_t = alphacums[ddim_timesteps]
    a_prev = np.asarray([alphacums[0]] + alphacums[ddim_timesteps[:-1]].tolist())
    sigmas = eta * np.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))
    return sigmas, a_t, a_prev


def pack_schedule(sampler, mode: int, use_original_steps: bool, clip_denoised: bool) -> Schedule:
    """The coefficient rows of a sampler that has run make_schedule (DDIMSampler, PLMSSampler: the two share the tables,
    ddim.py:25-55 / plms.py:26-57), row k = the k-th executed iteration, for the device loop of ``mode``."""
    m = sampler.model
    buf = lambda name: getattr(m, name).detach().float().cpu().numpy()
    if use_original_steps:
        ts = np.arange(sampler.ddpm_num_timesteps)
        alphas, alphas_prev = buf("alphas_cumprod"), buf("alphas_cumprod_prev")
        s1m, sig = buf("sqrt_one_minus_alphas_cumprod"), sampler.ddim_sigmas_for_original_num_steps
    else:
        ts = sampler.ddim_timesteps
        alphas, alphas_prev = sampler.ddim_alphas, sampler.ddim_alphas_prev
        s1m, sig = sampler.ddim_sqrt_one_minus_alphas, sampler.ddim_sigmas
    n = len(ts)
    order = np.arange(n - 1, -1, -1)              # index = total_steps - i - 1  (:163)
    steps = np.asarray(ts)[order]                 # np.flip(timesteps)
    coef = np.zeros((n, _lib.DSD_NCOEF), dtype=np.float32)
    coef[:, 0] = buf("sqrt_alphas_cumprod")[steps]               # predict_*_from_z_and_v gather by t
    coef[:, 1] = buf("sqrt_one_minus_alphas_cumprod")[steps]
    coef[:, 4] = np.asarray(alphas)[order].astype(np.float32)    # torch.full(..., alphas[index]) -> fp32
    coef[:, 5] = np.asarray(alphas_prev)[order].astype(np.float32)
    coef[:, 6] = np.asarray(sig)[order].astype(np.float32)
    coef[:, 7] = np.asarray(s1m)[order].astype(np.float32)
    pred = {"eps": _lib.PRED_EPS, "v": _lib.PRED_V}[m.parameterization]
    return Schedule(mode, pred, coef, steps.astype(np.float32), np.ones(n, dtype=np.int32), clip_denoised=clip_denoised)


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", device=torch.device("cuda"), **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.device = device

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps, verbose)
        acp = self.model.alphas_cumprod.detach().float().cpu().numpy()
        assert acp.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        sig, a_t, a_prev = make_ddim_sampling_parameters(acp, self.ddim_timesteps, ddim_eta, verbose)
        self.ddim_sigmas = np.asarray(sig, dtype=np.float64)
        self.ddim_alphas = np.asarray(a_t)
        self.ddim_alphas_prev = np.asarray(a_prev)
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - self.ddim_alphas)          # fp32, like np.sqrt(1 - fp32 tensor)
        acp_prev = self.model.alphas_cumprod_prev.detach().float().cpu()
        acp_t = self.model.alphas_cumprod.detach().float().cpu()
        self.ddim_sigmas_for_original_num_steps = (ddim_eta * torch.sqrt(
            (1 - acp_prev) / (1 - acp_t) * (1 - acp_t / acp_prev))).numpy()

    def _schedule(self, use_original_steps: bool, clip_denoised: bool) -> Schedule:
        return pack_schedule(self, _lib.MODE_B_DDIM, use_original_steps, clip_denoised)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               clip_denoised=True, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, dynamic_threshold=None,
               ucg_schedule=None, step_noise=None, seed=None, mask_noise=None, **kwargs):
        """:57-126 -> (samples, intermediates).  Unsupported reference options raise instead of being ignored.
        Classifier-free guidance (:194-219) runs in the device loop: ``unconditional_conditioning`` comes in the form of
        ``conditioning`` (dict with c_concat lists, list, or tensor); ``ucg_schedule`` holds one scale per executed step.
        ``mask`` / ``x0`` (:160-163) run in the device loop too, guided or not: in front of every network evaluation the state
        becomes q_sample(x0, t)*mask + (1 - mask)*state.  ``mask_noise`` ([steps,B,C,H,W]) feeds q_sample's draws (an extension
        like ``step_noise``); without it they are Philox normals of ``seed``.
        Intermediates (:149,178-183): {"x_inter": [x_T, ...], "pred_x0": [x_T, ...]}, the state and pred_x0 after every step
        whose index is a multiple of ``log_every_t`` and after the first; ``callback(i)`` then ``img_callback(pred_x0, i)`` run
        after every step, which cuts the device loop into single-step calls (same bits)."""
        if quantize_x0 or score_corrector is not None or dynamic_threshold is not None or temperature != 1. or noise_dropout != 0.:
            raise NotImplementedError("quantisation / score corrector / dynamic threshold / temperature / noise dropout are not "
                                      "on the medical hot path")
        if mask is not None and x0 is None:
            raise MaskWithoutX0("a mask needs x0, the image it keeps (ddim.py:161)")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose,
                           ddim_discretize=kwargs.get("ddim_discretize", "uniform"))
        C_, H, W = shape
        size = (batch_size, C_, H, W)
        use_orig = kwargs.get("ddim_use_original_steps", False)
        sched = self._schedule(use_orig, clip_denoised)
        device = self.model.betas.device
        guidance = None
        if ucg_schedule is not None:
            assert len(ucg_schedule) == sched.steps                                   # :166
        if guidance_active(unconditional_guidance_scale, unconditional_conditioning, ucg_schedule):
            u = cat_unconditional(conditioning, unconditional_conditioning, device, wrapper_key(self.model))
            guidance = Guidance(u, ucg_schedule if ucg_schedule is not None else unconditional_guidance_scale, sched.steps)
        img = x_T if x_T is not None else torch.randn(size, device=device)
        inpaint = None
        if mask is not None:                                                          # x0 alone changes nothing (:160)
            inpaint = Inpaint(x0.to(device), mask.to(device), mask_noise.to(device) if mask_noise is not None else None)
        # :149,178-183: the state and pred_x0 of every log_every_t-th step, callback(i) then img_callback(pred_x0, i) after each
        trace = Trace(kept_iterations(sched.steps, log_every_t))
        out = run_device_loop(self._unet(), sched, img.to(device), cat_conditioning(conditioning, device, wrapper_key(self.model)), step_noise=step_noise,
                              seed=seed, guidance=guidance, inpaint=inpaint, trace=trace,
                              callbacks=StepCallbacks(callback, img_callback, image="pred_x0"))
        return out, {"x_inter": [img] + trace.states, "pred_x0": [img] + trace.pred_x0s}

    def _unet(self):
        return find_unet(self.model.model if hasattr(self.model, "model") else self.model)

    def _guidance(self, cond, scale, uncond, steps, device):
        if not guidance_active(scale, uncond):
            return None
        return Guidance(cat_unconditional(cond, uncond, device, wrapper_key(self.model)), scale, steps)

    @torch.no_grad()
    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, callback=None):
        """:263-308, deterministic DDIM inversion on the device -> (x_next, out).  The reference hands the loop index i to the
        network as its time (:282) and feeds the output to the update as a noise prediction whatever the parameterization; the
        first is kept, a v-model raises.  Intermediates are read between first_step / n_steps segments of the loop."""
        if callback is not None:
            raise NotImplementedError("per-step callbacks are not on the device loop")
        if self.model.parameterization == "v":
            raise NotImplementedError("DDIMSampler.encode takes the network output as a noise prediction (ddim.py:284-295); for a "
                                      "v-model the reference's inversion is not one, so it is not reproduced")
        num_reference_steps = self.ddpm_num_timesteps if use_original_steps else self.ddim_timesteps.shape[0]
        assert t_enc <= num_reference_steps                                           # :268
        n = int(t_enc)
        if use_original_steps:
            buf = lambda name: getattr(self.model, name).detach().float().cpu()
            alphas_next, alphas = buf("alphas_cumprod")[:n], buf("alphas_cumprod_prev")[:n]
        else:
            alphas_next = torch.from_numpy(np.asarray(self.ddim_alphas[:n], dtype=np.float32))
            alphas = torch.tensor(np.asarray(self.ddim_alphas_prev[:n], dtype=np.float64))                  # :276
        coef = invert_coefficients(alphas_next, alphas)
        device = self.model.betas.device
        if unconditional_guidance_scale != 1.:
            assert unconditional_conditioning is not None                             # :286
        cond = cat_conditioning(c, device, wrapper_key(self.model))
        guidance = self._guidance(c, unconditional_guidance_scale, unconditional_conditioning, n, device)
        marks = []                                                                    # :296-302
        for i in range(n):
            if return_intermediates and (i % (n // return_intermediates) == 0 and i < n - 1 or i >= n - 2):
                marks.append(i)
        x_next, unet, done = x0.to(device), self._unet(), 0
        intermediates = []
        for i in marks + ([n - 1] if n and (not marks or marks[-1] != n - 1) else []):
            x_next = run_invert_loop(unet, coef, x_next, cond, guidance, first_step=done, n_steps=i + 1 - done)
            done = i + 1
            if i in marks:
                intermediates.append(x_next)
        out = {"x_encoded": x_next, "intermediate_steps": marks}
        if return_intermediates:
            out.update({"intermediates": intermediates})
        return x_next, out

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None, seed=None):
        """:310-324: sqrt(alphas)[t] * x0 + sqrt(1 - alphas)[t] * noise, ``t`` a [B] index tensor into the current schedule.
        ``seed`` (extension): Philox normals when no ``noise`` is given."""
        if use_original_steps:
            sa = self.model.sqrt_alphas_cumprod.detach().float().cpu()
            s1 = self.model.sqrt_one_minus_alphas_cumprod.detach().float().cpu()
        else:
            sa = torch.sqrt(torch.from_numpy(np.asarray(self.ddim_alphas, dtype=np.float32)))
            s1 = torch.from_numpy(np.asarray(self.ddim_sqrt_one_minus_alphas, dtype=np.float32))
        if not x0.is_cuda:
            raise RuntimeError("stochastic_encode runs on the MI355X only (no CPU fallback): x0 is on the CPU")
        idx = t.detach().long().cpu()
        return q_sample_rows(sa[idx].to(x0.device), s1[idx].to(x0.device), x0, noise.to(x0.device) if noise is not None else None,
                             seed=philox_seed(seed) if noise is None else 0)

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None, step_noise=None, seed=None):
        """:326-346: the last ``t_start`` iterations of the current schedule (timesteps[:t_start], flipped), i.e. the sampling
        loop from first_step = steps - t_start, with the eta of the last make_schedule and p_sample_ddim's default clipping.
        ``step_noise`` ([t_start,B,C,H,W]) / ``seed`` are extensions."""
        if callback is not None:
            raise NotImplementedError("per-step callbacks are not on the device loop")
        sched = self._schedule(use_original_steps, True)
        t_start = min(int(t_start), sched.steps)
        first = sched.steps - t_start
        if t_start <= 0:
            return x_latent
        device = self.model.betas.device
        guidance = self._guidance(cond, unconditional_guidance_scale, unconditional_conditioning, sched.steps, device)
        if step_noise is not None:                                                    # rows of the executed iterations
            full = torch.zeros((sched.steps,) + tuple(step_noise.shape[1:]), device=device, dtype=torch.float32)
            full[first:] = step_noise.to(device)
            step_noise = full
        return run_device_loop(self._unet(), sched, x_latent.to(device), cat_conditioning(cond, device, wrapper_key(self.model)), step_noise=step_noise,
                               seed=seed, first_step=first, guidance=guidance)

