"""PLMSSampler — drop-in for ldm/models/diffusion/plms.py (make_schedule :26-57, sample :59-116, plms_sampling :118-176,
p_sample_plms :178-245 with sampling_util.norm_thresholding), executed by dsd_sample_plms: the history of
noise predictions, the first step's predictor / corrector pair, classifier-free guidance, the mask blend and the norm threshold all
run in the device loop."""
from __future__ import annotations

import torch

from .... import _lib
from ...._sched import (Guidance, Inpaint, Schedule, StepCallbacks, Trace, cat_conditioning, cat_unconditional, find_unet,
                         guidance_active, kept_iterations, wrapper_key, run_plms_loop)
from .ddim import DDIMSampler, MaskWithoutX0, pack_schedule


class PLMSSampler(object):
    def __init__(self, model, schedule="linear", device=torch.device("cuda"), **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.device = device

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        """:26-57: the tables of DDIMSampler.make_schedule (same attributes), eta 0 only.  A step count whose timesteps leave
        the table (S = 3 on 1000 steps reaches index 1000) raises IndexError, as in the reference."""
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        DDIMSampler.make_schedule(self, ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=ddim_eta, verbose=verbose)

    def _schedule(self, use_original_steps: bool = False) -> Schedule:
        return pack_schedule(self, _lib.MODE_B_PLMS, use_original_steps, clip_denoised=False)   # PLMS has no clip_denoised

    def _unet(self):
        return find_unet(self.model.model if hasattr(self.model, "model") else self.model)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, dynamic_threshold=None, seed=None, mask_noise=None, **kwargs):
        """:59-176 -> (samples, intermediates); S steps make S + 1 network evaluations (the first step evaluates twice).
        ``temperature`` and ``noise_dropout`` are accepted and have no effect, as in the reference: PLMS takes eta = 0 only, so
        sigma_t is 0 and they act on ``sigma_t * noise`` — a zero tensor (:221-223); the loop draws no update noise.
        ``dynamic_threshold`` = v rescales every pred_x0 by v / max(rms(pred_x0), v) per sample (norm_thresholding), the
        first step's predictor included.  ``mask`` / ``x0`` blend q_sample(x0, t) into the state in front of every step (:152-155);
        ``mask_noise`` ([S,B,C,H,W]) feeds q_sample's draws, else they are Philox normals of ``seed`` (both extensions, as in
        DDIMSampler.sample).  The conditioning comes as a tensor, a list or dict(c_concat=[...]), the unconditional one alike.
        Intermediates and ``callback`` / ``img_callback`` as in DDIMSampler.sample (:139,169-174); pred_x0 is the one of the step's
        final get_x_prev_and_pred_x0.  Unsupported reference options raise instead of being ignored."""
        if quantize_x0:
            raise NotImplementedError("quantize_x0 needs a VQ first stage; not on the device loop")
        if score_corrector is not None:
            raise NotImplementedError("score correctors are not on the device loop")
        if (callback is not None or img_callback is not None) and not self.model.betas.is_cuda:
            raise NotImplementedError("per-step callbacks (callback / img_callback) run between single-step calls of the device loop: "
                                      "they need the model on the GPU (no CPU fallback)")
        if self.model.parameterization == "v":
            raise NotImplementedError("PLMSSampler takes the network output as a noise prediction (plms.py:227-243); for a "
                                      "v-model the reference's update is not one, so it is not reproduced")
        if mask is not None and x0 is None:
            raise MaskWithoutX0("a mask needs x0, the image it keeps (plms.py:153)")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C_, H, W = shape
        size = (batch_size, C_, H, W)
        sched = self._schedule()
        device = self.model.betas.device
        guidance = None
        if guidance_active(unconditional_guidance_scale, unconditional_conditioning):
            u = cat_unconditional(conditioning, unconditional_conditioning, device, wrapper_key(self.model))
            guidance = Guidance(u, unconditional_guidance_scale, sched.steps)
        img = x_T if x_T is not None else torch.randn(size, device=device)
        inpaint = None
        if mask is not None:
            inpaint = Inpaint(x0.to(device), mask.to(device), mask_noise.to(device) if mask_noise is not None else None)
        # :139,169-174: the state and the step's final pred_x0 of every log_every_t-th step; callback(i), img_callback(pred_x0, i)
        trace = Trace(kept_iterations(sched.steps, log_every_t))
        out = run_plms_loop(self._unet(), sched, img.to(device), cat_conditioning(conditioning, device, wrapper_key(self.model)),
                            threshold=dynamic_threshold, guidance=guidance, inpaint=inpaint, seed=seed, trace=trace,
                            callbacks=StepCallbacks(callback, img_callback, image="pred_x0"))
        return out, {"x_inter": [img] + trace.states, "pred_x0": [img] + trace.pred_x0s}
