"""DPMSolverSampler — drop-in for ldm/models/diffusion/dpm_solver_new/sampler.py:20-103: DPM-Solver++ multistep order 2,
uniform time spacing, over the LDM model's fp32 ``betas`` buffer; the loop runs in dsd_sample_dpm."""
from __future__ import annotations

import torch

from .dpm_solver_pytorch import NoiseScheduleVP, model_wrapper, DPM_Solver

MODEL_TYPES = {"eps": "noise", "v": "v"}


class _ApplyModel:
    """``lambda x, t, c: model.apply_model(x, t, c)`` of the reference (:90), kept as an object so the solver can find
    the native network behind it."""

    def __init__(self, ldm_model):
        self.ldm_model = ldm_model
        self.diffusion_model = getattr(getattr(ldm_model, "model", None), "diffusion_model", None)
        self.conditioning_key = getattr(getattr(ldm_model, "model", None), "conditioning_key", None)

    def __call__(self, x, t, c):
        return self.ldm_model.apply_model(x, t, c)


class DPMSolverSampler(object):
    def __init__(self, model, device=torch.device("cuda"), **kwargs):
        self.model = model
        self.device = device
        self.alphas_cumprod = model.alphas_cumprod.clone().detach().to(torch.float32)
        self.betas = model.betas.clone().detach().to(torch.float32)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        """:35-103 -> (samples, None).  ``unconditional_guidance_scale`` / ``unconditional_conditioning`` run classifier-free
        guidance in the device loop.  The reference supports the tensor form of the two conditionings there (its
        ``torch.cat([unconditional_condition, condition])`` raises TypeError on a dict); the dict (``c_concat`` lists) and list
        forms, in which the unconditional conditioning mirrors the conditioning, are accepted as an extension."""
        if mask is not None or quantize_x0 or score_corrector is not None:
            raise NotImplementedError("inpainting mask / quantisation / score corrector options are not on the medical hot path")
        C_, H, W = shape
        size = (batch_size, C_, H, W)
        device = self.model.betas.device
        img = torch.randn(size, device=device) if x_T is None else x_T
        ns = NoiseScheduleVP("discrete", betas=self.betas)
        slot = "c_concat" if getattr(getattr(self.model, "model", None), "conditioning_key", None) in (None, "concat") \
            else "c_crossattn"                                # apply_model's filing of a tensor or list (ddpm.py:862-866)
        if not isinstance(conditioning, dict):
            if unconditional_conditioning is not None:        # the same wrapping keeps the two in one form
                assert not isinstance(unconditional_conditioning, dict) and \
                    isinstance(unconditional_conditioning, list) == isinstance(conditioning, list), \
                    "unconditional_conditioning must come in the form of the conditioning"
                unconditional_conditioning = {slot: unconditional_conditioning if isinstance(
                    unconditional_conditioning, list) else [unconditional_conditioning]}
            conditioning = {slot: conditioning if isinstance(conditioning, list) else [conditioning]}
        model_fn = model_wrapper(_ApplyModel(self.model), ns, model_type=MODEL_TYPES[self.model.parameterization],
                                 guidance_type="classifier-free", condition=conditioning,
                                 unconditional_condition=unconditional_conditioning,
                                 guidance_scale=unconditional_guidance_scale)
        dpm_solver = DPM_Solver(model_fn, ns, algorithm_type="dpmsolver++")
        x = dpm_solver.sample(img.to(device), steps=S, skip_type="time_uniform", method="multistep", order=2)
        return x.to(device), None
