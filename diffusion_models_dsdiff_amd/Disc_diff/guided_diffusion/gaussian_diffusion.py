"""GaussianDiffusion — drop-in for Disc_diff/guided_diffusion/gaussian_diffusion.py (sampling and evaluation side).

Same constructor, enums and sampling entry points as the reference (``p_sample_loop`` :524-567,
``ddim_sample_loop`` :705-737, ``p_sample`` :422-465, ``ddim_sample`` :618-665 and their
``*_progressive`` generators).  The float64 schedule tables are built on the host exactly as
:141-178 does; the loop itself (network + fused update) runs on the MI355X through dsd_sample.  The evaluation half — ``calc_bpd_loop``
:938-991 with ``_vb_terms_bpd`` / ``_prior_bpd``, ``p_mean_variance`` as a method, ``ddim_reverse_sample`` and the q_* helpers —
runs through dsd_calc_bpd and the dsd_op_vlb_terms / dsd_op_prior_bpd / dsd_op_ddim_reverse_step kernels.
``training_losses`` :821-920 (and its training_project/utils twin :824-) is here as an EVALUATION — the validation loss of a
checkpoint, forward only, one timestep per sample — through dsd_eval_loss, with the contrastive ``disentangle=`` terms over the
content / style / anatomy / lesion heads (:907-975, ``get_disentangle_loss`` :1056-1094) through dsd_set_disentangle /
dsd_op_contrast_rows; anything with a gradient stays out.
"""
from __future__ import annotations

import enum
import math

import numpy as np
import torch as th

from ... import _lib
from ... import _sched
from ..._sched import (Schedule, ddim_reverse_step, disc_planes, is_disc, is_dit, kwargs_conditioning, loop_denoiser, loss_rows,
                       model_output_of, pair_mse_rows, philox_seed, prior_bpd, q_sample_rows, run_bpd_loop, run_device_loop,
                       run_eval_loss, sampler_update, vlb_terms, vlb_terms_rows, _seed_from_torch)


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    """gaussian_diffusion.py:31-54."""
    if schedule_name == "linear":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps,
                                   lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    """gaussian_diffusion.py:57-73."""
    n = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)])


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self == LossType.KL or self == LossType.RESCALED_KL


class GaussianDiffusion:
    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type, rescale_timesteps=False,
                 parameterization="eps"):
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        self.rescale_timesteps = rescale_timesteps
        self.parameterization = parameterization
        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert len(betas.shape) == 1, "betas must be 1-D"
        assert (betas > 0).all() and (betas <= 1).all()
        self.num_timesteps = int(betas.shape[0])
        one_minus = 1.0 - betas
        self.alphas_cumprod = np.cumprod(one_minus, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(one_minus) / (1.0 - self.alphas_cumprod)

    # ------------------------------------------------------------------ host -> device schedule
    def _model_timestep_values(self) -> np.ndarray:
        """Value handed to the network for loop index i (``_scale_timesteps`` :381-384; overridden by SpacedDiffusion)."""
        t = np.arange(self.num_timesteps, dtype=np.float32)
        if self.rescale_timesteps:
            t = t * np.float32(1000.0 / self.num_timesteps)
        return t

    def _pred_code(self) -> int:
        if self.parameterization == "v":
            return _lib.PRED_V
        if self.model_mean_type == ModelMeanType.EPSILON:
            return _lib.PRED_EPS
        if self.model_mean_type == ModelMeanType.START_X:
            return _lib.PRED_X0
        raise NotImplementedError("ModelMeanType.PREVIOUS_X is not used by any shipped config")

    def _schedule(self, ddim: bool, eta: float, clip_denoised: bool) -> Schedule:
        T = self.num_timesteps
        idx = np.arange(T - 1, -1, -1)                          # loop order: i = T-1 .. 0  (:595,:764)
        f32 = lambda a: np.asarray(a, dtype=np.float64)[idx].astype(np.float32)   # arr[t].float()  (:1003)
        coef = np.zeros((T, _lib.DSD_NCOEF), dtype=np.float32)
        coef[:, 0] = f32(self.sqrt_alphas_cumprod)
        coef[:, 1] = f32(self.sqrt_one_minus_alphas_cumprod)
        coef[:, 2] = f32(self.sqrt_recip_alphas_cumprod)
        coef[:, 3] = f32(self.sqrt_recipm1_alphas_cumprod)
        learned = self.model_var_type == ModelVarType.LEARNED_RANGE
        if self.model_var_type == ModelVarType.LEARNED:
            raise NotImplementedError("ModelVarType.LEARNED is not used by any shipped config")
        if ddim:
            coef[:, 4] = f32(self.alphas_cumprod)
            coef[:, 5] = f32(self.alphas_cumprod_prev)
        else:
            coef[:, 4] = f32(self.posterior_mean_coef1)
            coef[:, 5] = f32(self.posterior_mean_coef2)
            if learned:                                          # :287-290
                coef[:, 6] = f32(self.posterior_log_variance_clipped)
                coef[:, 7] = f32(np.log(self.betas))
            elif self.model_var_type == ModelVarType.FIXED_LARGE:   # :299-302
                coef[:, 6] = f32(np.log(np.append(self.posterior_variance[1], self.betas[1:])))
            else:                                                # FIXED_SMALL :303-306
                coef[:, 6] = f32(self.posterior_log_variance_clipped)
        t_model = self._model_timestep_values()[idx]
        nonzero = (idx != 0).astype(np.int32)                    # :457-459
        mode = _lib.MODE_A_DDIM if ddim else _lib.MODE_A_DDPM
        return Schedule(mode, self._pred_code(), coef, t_model, nonzero, learned_range=learned,
                        clip_denoised=clip_denoised, eta=eta)

    # ------------------------------------------------------------------ loops
    def _loop(self, ddim, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress,
              eta=0.0, step_noise=None, seed=None):
        assert isinstance(shape, (tuple, list))
        model_kwargs = model_kwargs or {}
        sched = self._schedule(ddim, eta, clip_denoised)
        hooks = denoised_fn is not None or cond_fn is not None
        self._check_hooks(ddim, denoised_fn, cond_fn)
        unet = loop_denoiser(model, model_kwargs)        # None for a DiT that is to receive labels / its own cond=
        if hooks and unet is not None:
            # a Python hook sits between network and update: per-step host loop; a bare native U-Net does not concatenate
            # c_concat itself (DiffusionWrapper.forward does, ddpm.py:1328-1333)
            if unet is model and is_disc(unet):
                if "c_concat" in model_kwargs:               # (t1 / t2 / dwi are concatenated by the loop below, as :271-275)
                    model = lambda x, t, _u=unet, **kw: _u(th.cat([x] + [c.to(x.device) for c in kw["c_concat"]], 1), t)
            elif unet is model:
                model = lambda x, t, _u=unet, **kw: _u(th.cat([x] + [c.to(x.device) for c in kw.get("c_concat", [])], 1), t,
                                                       context=kw.get("context"), y=kw.get("y"))
            unet = None
        if device is None:
            device = next(model.parameters()).device if hasattr(model, "parameters") else th.device("cuda")
            if th.device(device).type != "cuda":
                device = th.device("cuda")
        img = noise if noise is not None else th.randn(*shape, device=device)      # :591-594
        img = img.to(device)
        planes = disc_planes(model_kwargs, device)               # t1 / t2 / dwi: concatenated behind x (:271-275)
        if unet is not None and is_disc(unet) and planes is not None:
            return run_device_loop(unet, sched, img, th.cat(planes, 1), step_noise=step_noise, seed=seed)
        bundle = kwargs_conditioning(unet, model, model_kwargs, device) if unet is not None and not is_dit(unet) else None
        if bundle is not None:                                # context= / y= (or c_crossattn / c_adm) for a UNetModel
            return run_device_loop(unet, sched, img, bundle, step_noise=step_noise, seed=seed)
        c_concat = model_kwargs.get("c_concat")
        if unet is not None and c_concat is None and is_dit(unet):
            c_concat = [img.new_zeros((img.shape[0], 0) + tuple(img.shape[2:]))]      # an unconditional DiT: all input is state
        if unet is not None and c_concat is not None:
            cond = th.cat([c.to(device) for c in c_concat], 1)
            return run_device_loop(unet, sched, img, cond, step_noise=step_noise, seed=seed)
        # generic callable (closure / foreign module): python loop, fused HIP update per step
        seed = _seed_from_torch() if seed is None else seed
        x = img.float().contiguous().clone()
        B = x.shape[0]
        tvals = th.from_numpy(sched.t_model)
        for k in range(sched.steps):
            tv = tvals[k]
            is_int = (not self.rescale_timesteps) and float(tv) == int(tv)
            t = th.full((B,), int(tv) if is_int else float(tv), device=device,
                        dtype=th.long if is_int else th.float32)
            out = model_output_of(model(x if planes is None else th.cat([x] + planes, 1), t, **model_kwargs))
            self._hooked_update(sched, k, out, x, t, None if step_noise is None else step_noise[k].to(device), seed,
                                denoised_fn, cond_fn, model_kwargs)
        return x

    # ---- denoised_fn / cond_fn (:312-313, :386-398, :460-463)
    def _check_hooks(self, ddim, denoised_fn, cond_fn):
        if cond_fn is None:
            return
        if ddim:
            raise NotImplementedError(
                "cond_fn with DDIM (condition_score, gaussian_diffusion.py:400-420) is not built: it re-derives pred_xstart from a "
                "shifted eps WITHOUT clipping it again, which the fused update cannot express.  Use p_sample_loop(..., cond_fn=...) "
                "(classifier guidance on the DDPM mean, supported for the fixed variance types), or write the step loop over "
                "model(x, t) and _sched.sampler_update() yourself")
        if self.model_var_type == ModelVarType.LEARNED_RANGE:
            raise NotImplementedError(
                "cond_fn needs the per-pixel variance of the step; with learn_sigma it lives inside the fused update.  Use a "
                "fixed-variance diffusion (learn_sigma=False) with p_sample_loop(..., cond_fn=...)")

    def _hooked_update(self, sched, k, out, x, t, noise, seed, denoised_fn, cond_fn, model_kwargs, want_x0=False):
        """One update with the reference's hooks, still on the fused HIP kernel.
        denoised_fn acts on the predicted x_start BEFORE the clip (process_xstart :311-316): x_start is formed here from the
        network output with the reference's fp32 expressions, handed to denoised_fn, and the kernel is then run in its
        x_start-prediction mode (it clips and does the rest).  cond_fn shifts the mean by variance * gradient (:386-398);
        the sample is linear in the mean, so the shift is added to the kernel's result."""
        if denoised_fn is None and cond_fn is None:
            return sampler_update(sched, k, out, x, noise, seed, want_x0=want_x0)
        grad = None
        if cond_fn is not None:
            grad = cond_fn(x, t, **model_kwargs).float()              # x is still x_t here; t as the network received it
        out, run = self._apply_denoised_fn(sched, k, out, x, denoised_fn)
        x0_out = sampler_update(run, k, out, x, noise, seed, want_x0=want_x0)
        if grad is not None:
            # p_mean_var["variance"] of this step (:296-309): the variance TABLE (FIXED_SMALL pairs the raw posterior variance,
            # 0 at t = 0, with the clipped log), gathered in float64 and rounded to fp32 as _extract_into_tensor does
            i = self.num_timesteps - 1 - k
            var = (np.append(self.posterior_variance[1], self.betas[1:]) if self.model_var_type == ModelVarType.FIXED_LARGE
                   else self.posterior_variance)
            x.add_(float(np.float32(var[i])) * grad)
        return x0_out

    @staticmethod
    def _apply_denoised_fn(sched, k, out, x, denoised_fn):
        """process_xstart's hook (:311-313): (network output, schedule) for the kernels.  With a denoised_fn the x_start is
        formed here with the reference's fp32 expressions, post-processed, and handed on as an x_start prediction."""
        if denoised_fn is None:
            return out, sched
        c = th.from_numpy(sched.coef[k]).to(x.device)
        C = x.shape[1]
        eps_or_v, rest = (out[:, :C], out[:, C:]) if sched.c.learned_range else (out, None)
        if sched.c.pred == _lib.PRED_V:                            # predict_start_from_z_and_v :236-242
            x0 = c[0] * x - c[1] * eps_or_v
        elif sched.c.pred == _lib.PRED_EPS:                        # _predict_xstart_from_eps :352-357
            x0 = c[2] * x - c[3] * eps_or_v
        else:
            x0 = eps_or_v
        x0 = denoised_fn(x0).float()
        return (x0 if rest is None else th.cat([x0, rest], 1)), sched.with_pred(_lib.PRED_X0)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False, step_noise=None, seed=None):
        """:524-567.  ``step_noise`` ([T,B,1,H,W]) / ``seed`` are extensions: injected normals (parity runs) or
        the Philox seed; by default the per-step noise is on-device Philox seeded from torch's generator."""
        return self._loop(False, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                          progress, 0.0, step_noise, seed)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, step_noise=None, seed=None):
        """:705-737."""
        return self._loop(True, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                          progress, eta, step_noise, seed)

    def dpm_solver_sample_loop(self, model, shape, clip_denoised=None, model_kwargs=None, noise=None, device=None):
        """:467-522 — DPM-Solver++ multistep order 2 over this (possibly respaced) schedule: ``num_timesteps`` network
        evaluations, logSNR spacing, dynamic thresholding, no lower-order final step.  As in the reference the network
        receives the solver's continuous model time (no timestep_map / rescale) and ``clip_denoised`` is unused.
        ``noise`` (x_T) is an extension for reproducible runs; the reference draws it itself (:470)."""
        from .sampler import NoiseScheduleVP, model_wrapper, DPM_Solver
        if device is None:
            device = next(model.parameters()).device if hasattr(model, "parameters") else th.device("cuda")
            if th.device(device).type != "cuda":
                device = th.device("cuda")
        x = (noise if noise is not None else th.randn(*shape, device=device)).to(device)
        thresholding, denoise = True, False
        noise_schedule = NoiseScheduleVP(schedule="discrete", betas=th.from_numpy(self.betas).float())
        model_fn_continuous = model_wrapper(model, noise_schedule, model_type="noise", model_kwargs=model_kwargs or {})
        dpm_solver = DPM_Solver(model_fn_continuous, noise_schedule, algorithm_type="dpmsolver++",
                                correcting_x0_fn="dynamic_thresholding" if thresholding else None)
        return dpm_solver.sample(x, steps=(self.num_timesteps - 1 if denoise else self.num_timesteps), order=2,
                                 skip_type="logSNR", method="multistep", lower_order_final=False,
                                 denoise_to_zero=denoise, solver_type="dpmsolver")

    def _progressive(self, ddim, model, shape, noise, clip_denoised, model_kwargs, device, eta, denoised_fn=None, cond_fn=None):
        model_kwargs = model_kwargs or {}
        sched = self._schedule(ddim, eta, clip_denoised)
        self._check_hooks(ddim, denoised_fn, cond_fn)
        if device is None:
            device = th.device("cuda")
        img = (noise if noise is not None else th.randn(*shape, device=device)).to(device).float().contiguous().clone()
        seed = _seed_from_torch()
        B = img.shape[0]
        for k in range(sched.steps):
            i = self.num_timesteps - 1 - k
            t = th.tensor([i] * B, device=device)
            out = self._call_model(model, img, t, model_kwargs)
            x0 = self._hooked_update(sched, k, out, img, self._model_t(t), None, seed, denoised_fn, cond_fn, model_kwargs, want_x0=True)
            yield {"sample": img.clone(), "pred_xstart": x0}

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False):
        """:569-616 (yields {"sample","pred_xstart"} per step)."""
        yield from self._progressive(False, model, shape, noise, clip_denoised, model_kwargs, device, 0.0, denoised_fn, cond_fn)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                     cond_fn=None, model_kwargs=None, device=None, progress=False, eta=0.0):
        """:739-786."""
        yield from self._progressive(True, model, shape, noise, clip_denoised, model_kwargs, device, eta, denoised_fn, cond_fn)

    # ------------------------------------------------------------------ single steps
    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    def _model_t(self, t):
        """loop index -> the timestep the network (and cond_fn) receives (respace.py:123-128)."""
        tv = th.from_numpy(self._model_timestep_values()).to(t.device)[t]
        return tv if self.rescale_timesteps else tv.long()

    def _call_model(self, model, x, t, model_kwargs):
        """p_mean_variance's network call (:266-278): loop index -> network timestep, tuple -> tensor."""
        tv = th.from_numpy(self._model_timestep_values()).to(x.device)[t]
        if not self.rescale_timesteps:
            tv = tv.long()
        planes = disc_planes(model_kwargs, x.device)             # :271-275
        return model_output_of(model(x if planes is None else th.cat([x] + planes, 1), tv, **model_kwargs))

    def _single(self, ddim, model, x, t, clip_denoised, model_kwargs, eta, denoised_fn=None, cond_fn=None):
        model_kwargs = model_kwargs or {}
        i = int(t[0])
        assert bool((t == i).all()), "all samples of a batch share the timestep in every reference loop"
        sched = self._schedule(ddim, eta, clip_denoised)
        self._check_hooks(ddim, denoised_fn, cond_fn)
        out = self._call_model(model, x, t, model_kwargs)
        xn = x.float().contiguous().clone()
        x0 = self._hooked_update(sched, self.num_timesteps - 1 - i, out, xn, self._model_t(t.to(x.device)), None, _seed_from_torch(),
                                 denoised_fn, cond_fn, model_kwargs, want_x0=True)
        return {"sample": xn, "pred_xstart": x0}

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None):
        """:422-465."""
        return self._single(False, model, x, t, clip_denoised, model_kwargs, 0.0, denoised_fn, cond_fn)

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        """:618-665."""
        return self._single(True, model, x, t, clip_denoised, model_kwargs, eta, denoised_fn, cond_fn)

    # ------------------------------------------------------------------ the forward process and its posterior
    def q_mean_variance(self, x_start, t):
        """:180-194."""
        mean = _extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        variance = _extract_into_tensor(1.0 - self.alphas_cumprod, t, x_start.shape)
        log_variance = _extract_into_tensor(self.log_one_minus_alphas_cumprod, t, x_start.shape)
        return mean, variance, log_variance

    def q_sample(self, x_start, t, noise=None):
        """:196-212, on the q_sample kernel (dsd_op_q_sample, per-row coefficients)."""
        if noise is None:
            noise = th.randn_like(x_start)
        assert noise.shape == x_start.shape
        t = t.to(x_start.device)
        a = _extract_into_tensor(self.sqrt_alphas_cumprod, t, t.shape)
        s = _extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, t.shape)
        return q_sample_rows(a, s, x_start, noise)

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """:214-234."""
        assert x_start.shape == x_t.shape
        posterior_mean = (_extract_into_tensor(self.posterior_mean_coef1, t, x_t.shape) * x_start
                          + _extract_into_tensor(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        posterior_variance = _extract_into_tensor(self.posterior_variance, t, x_t.shape)
        posterior_log_variance_clipped = _extract_into_tensor(self.posterior_log_variance_clipped, t, x_t.shape)
        return posterior_mean, posterior_variance, posterior_log_variance_clipped

    def _predict_xstart_from_eps(self, x_t, t, eps):
        """:352-357."""
        assert x_t.shape == eps.shape
        return (_extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
                - _extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * eps)

    def _predict_eps_from_xstart(self, x_t, t, pred_xstart):
        """:369-373."""
        return ((_extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - pred_xstart)
                / _extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape))

    # ------------------------------------------------------------------ variational bound
    def _post_log_var(self) -> np.ndarray:
        """posterior_log_variance_clipped in loop order, fp32 of the float64 table (:225-227, :1003)."""
        return self.posterior_log_variance_clipped[::-1].astype(np.float32)

    def _step_of(self, t) -> int:
        i = int(t[0])
        assert bool((t == i).all()), "all samples of a batch share the timestep in every reference loop"
        return i

    def _evaluate(self, model, x, t, clip_denoised, denoised_fn, model_kwargs):
        """The network evaluation in front of p_mean_variance's arithmetic: (loop index i, iteration k, output, schedule)."""
        i = self._step_of(t)
        sched = self._schedule(False, 0.0, clip_denoised)
        out = self._call_model(model, x, t.to(x.device), model_kwargs or {})
        out, run = self._apply_denoised_fn(sched, self.num_timesteps - 1 - i, out.float(), x.float(), denoised_fn)
        return i, self.num_timesteps - 1 - i, out, run

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """:244-350 as a method: {"mean", "variance", "log_variance", "pred_xstart"}, the planes of the terms kernel
        (dsd_op_vlb_terms).  ``denoised_fn`` goes through the x_start-mode hook path of the sampling loops: x_start is formed
        from the network output, post-processed, and the kernel runs as for an x_start prediction."""
        i, k, out, run = self._evaluate(model, x, t, clip_denoised, denoised_fn, model_kwargs)
        xc = x.float().contiguous()
        mean, log_variance, pred_xstart = vlb_terms(run, k, float(self._post_log_var()[k]), out, xc, xc, xc, want_planes=True)
        if self.model_var_type == ModelVarType.LEARNED_RANGE:
            variance = th.exp(log_variance)                                        # :294
        else:
            table = (np.append(self.posterior_variance[1], self.betas[1:]) if self.model_var_type == ModelVarType.FIXED_LARGE
                     else self.posterior_variance)                                 # :296-308
            variance = _extract_into_tensor(table, t.to(x.device), x.shape)
        return {"mean": mean, "variance": variance, "log_variance": log_variance, "pred_xstart": pred_xstart}

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0):
        """:667-703 on dsd_op_ddim_reverse_step."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        i, k, out, run = self._evaluate(model, x, t, clip_denoised, denoised_fn, model_kwargs)
        xn = x.float().contiguous().clone()
        x0 = ddim_reverse_step(run, k, float(np.float32(self.alphas_cumprod_next[i])), out, xn, want_x0=True)
        return {"sample": xn, "pred_xstart": x0}

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """:788-819: {"output": [N] bits per dimension (the decoder NLL at t == 0, else the KL), "pred_xstart"}."""
        i, k, out, run = self._evaluate(model, x_t, t, clip_denoised, None, model_kwargs)
        output = th.empty((x_start.shape[0],), device=x_t.device, dtype=th.float32)
        xt = x_t.float().contiguous()
        _, _, pred_xstart = vlb_terms(run, k, float(self._post_log_var()[k]), out, xt, x_start.to(x_t.device), xt, vb=output,
                                      want_planes=True)
        return {"output": output, "pred_xstart": pred_xstart}

    def _prior_bpd(self, x_start):
        """:922-936 on dsd_op_prior_bpd."""
        T = self.num_timesteps
        return prior_bpd(np.float32(self.sqrt_alphas_cumprod[T - 1]), np.float32(self.log_one_minus_alphas_cumprod[T - 1]), x_start)

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, step_noise=None, seed=None):
        """:938-991: {"total_bpd", "prior_bpd" [N]; "vb", "xstart_mse", "mse" [N,T], column k at t = T-1-k}.  ``step_noise``
        ([T,N,C,H,W]) / ``seed`` are extensions as on the sampling loops: the normals q_sample draws at every timestep, fed for
        parity runs, else on-device Philox seeded from torch's generator.  A native denoiser with at most ``c_concat`` runs the
        device loop (dsd_calc_bpd); a generic callable, or a DiT that is to receive labels, is evaluated
        step by step around the same kernels."""
        model_kwargs = model_kwargs or {}
        sched = self._schedule(False, 0.0, clip_denoised)
        T = self.num_timesteps
        plv = self._post_log_var()
        prior_lv = float(np.float32(self.log_one_minus_alphas_cumprod[T - 1]))
        if not x_start.is_cuda:
            x_start = x_start.to(th.device("cuda"))
        device = x_start.device
        xs = x_start.float().contiguous()
        unet = loop_denoiser(model, model_kwargs)
        bundle = kwargs_conditioning(unet, model, model_kwargs, device) if unet is not None and not is_dit(unet) else None
        c_concat = model_kwargs.get("c_concat")
        planes = disc_planes(model_kwargs, device)               # t1 / t2 / dwi: the three condition planes of UNet_disc_Model
        if unet is not None and is_disc(unet) and planes is not None:
            c_concat = planes
        if unet is not None and c_concat is None and is_dit(unet):
            c_concat = [xs.new_zeros((xs.shape[0], 0) + tuple(xs.shape[2:]))]
        if unet is not None and (c_concat is not None or bundle is not None):
            cond = bundle if bundle is not None else th.cat([c.to(device) for c in c_concat], 1)
            res = run_bpd_loop(unet, sched, plv, prior_lv, xs, cond, step_noise=step_noise, seed=seed)
        else:
            seed = philox_seed(seed)
            B = xs.shape[0]
            res = {key: th.zeros((B, T), device=device, dtype=th.float32) for key in ("vb", "xstart_mse", "mse")}
            res["prior_bpd"] = self._prior_bpd(xs)
            tvals = th.from_numpy(sched.t_model)
            for k in range(T):
                a = th.full((B,), float(sched.coef[k, 0]), device=device)
                s = th.full((B,), float(sched.coef[k, 1]), device=device)
                z = None if step_noise is None else step_noise[k].to(device)
                x_t = q_sample_rows(a, s, xs, z, seed, k)              # the loop's Philox stream (seed, k + 2^32) when not fed
                tv = tvals[k]
                is_int = (not self.rescale_timesteps) and float(tv) == int(tv)
                t = th.full((B,), int(tv) if is_int else float(tv), device=device, dtype=th.long if is_int else th.float32)
                out = model_output_of(model(x_t if planes is None else th.cat([x_t] + planes, 1), t, **model_kwargs))
                vlb_terms(sched, k, float(plv[k]), out, x_t, xs, z, seed, vb=res["vb"][:, k], xstart_mse=res["xstart_mse"][:, k],
                          mse=res["mse"][:, k])
        res["total_bpd"] = res["vb"].sum(dim=1) + res["prior_bpd"]             # :984
        return res

    # ------------------------------------------------------------------ the denoising loss (evaluation)
    def get_v(self, x, noise, t):
        """:375-379."""
        return (_extract_into_tensor(self.sqrt_alphas_cumprod, t, x.shape) * noise
                - _extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x.shape) * x)

    def _loss_rows(self, t):
        """The per-sample values of a batch of timesteps ``t`` [B]: (network timestep, a = sqrt_alphas_cumprod[t], s =
        sqrt_one_minus_alphas_cumprod[t], (vlb coefficient rows, posterior_log_variance_clipped[t], t == 0)), each the fp32 of the
        float64 table as _extract_into_tensor rounds it."""
        idx = t.detach().cpu().numpy().astype(np.int64)
        if idx.ndim != 1:
            raise ValueError(f"t must be a [B] tensor of timestep indices, got shape {tuple(t.shape)}")
        T = self.num_timesteps
        if idx.size and (idx.min() < 0 or idx.max() >= T):
            raise ValueError(f"t must lie in [0, {T - 1}], got [{idx.min()}, {idx.max()}]")
        f32 = lambda a: np.asarray(a, dtype=np.float64)[idx].astype(np.float32)
        sched = self._schedule(False, 0.0, False)                       # clip_denoised=False (:847, :872)
        vlb = (sched.coef[T - 1 - idx], f32(self.posterior_log_variance_clipped), (idx == 0).astype(np.int32))
        return self._model_timestep_values()[idx], f32(self.sqrt_alphas_cumprod), f32(self.sqrt_one_minus_alphas_cumprod), vlb

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, disentangle=None, disen_lambda=0.1, seed=None):
        """The reference's training_losses, forward only: a dict of [N] tensors.  ``t`` [N] (long) may hold a different timestep
        for every sample.  The denoiser picks the form: a UNet_disc_Model takes Disc_diff/guided_diffusion/gaussian_diffusion.py:
        821-920 (``t1`` / ``t2`` / ``dwi`` of ``model_kwargs`` behind x_t; terms "mse", "com", "dist", "disent" = com / dist, "vb"
        with a learned sigma, "loss"); any other takes training_project/utils/gaussian_diffusion.py:824- (the condition from
        ``c_concat``, or from ``F_Data1``, ``F_Data2``, ``S_Data1`` [, ``edge``] as there; terms "mse", "vb", "loss").  "mse" is the
        Charbonnier loss both copies compute under that name (smooth_L1).  A native denoiser runs dsd_eval_loss (q_sample, one
        forward with per-sample t, the loss kernels); a foreign callable is called as ``model(x_t, t)`` around the same
        kernels.  ``noise`` None: on-device Philox normals keyed by ``seed`` (an extension, as on the loops), else by torch's
        generator.

        ``disentangle`` 'contrast' | 'eu' | 'eu&contrast' (training_project form only, :907-975) adds "disen_c_s_loss" and
        "disen_s_a_l_loss" (0-dim fp32: get_disentangle_loss over content + style at temperature 0.05 and over style + anatomy +
        lesion at 0.1, labels as :932-951) and "contrast_map" with the four raw [R,R] fp32 matrices (the two logits and the two
        perfect_logit = 2*mask - 1) under the reference's keys.  The reference passes each through get_heatmap to a viridis RGB
        image; colouring is presentation and stays with the caller.  A native DSUnetModel computes them inside the same
        dsd_eval_loss call from the head tensors in its workspace; a foreign callable must return ``(out, dict)`` with the
        'content' / 'style' / 'anatomy' / 'lesion' lists.  ``disen_lambda`` is unread, as in the reference.  The KL loss types
        ignore ``disentangle``, as the reference's branch does."""
        if disentangle is not None and not (isinstance(disentangle, str) and disentangle in _sched.DISENTANGLE_MODES):
            raise NotImplementedError(f"disentangle={disentangle!r} is not supported: get_disentangle_loss "
                                      f"(training_project/utils/gaussian_diffusion.py:1056-1094) knows {_sched.DISENTANGLE_MODES}")
        if not isinstance(self.loss_type, LossType):
            raise NotImplementedError(self.loss_type)
        if not x_start.is_cuda:
            raise RuntimeError("training_losses runs on the MI355X only (no CPU fallback): x_start is on the CPU")
        model_kwargs = model_kwargs or {}
        device = x_start.device
        xs = x_start.detach().float().contiguous()
        if noise is not None:
            assert noise.shape == x_start.shape
            noise = noise.to(device)
        seed = philox_seed(seed) if noise is None else 0
        t_model, a, s, vlb = self._loss_rows(t)
        unet = loop_denoiser(model, {k: v for k, v in model_kwargs.items() if k in ("t1", "t2", "dwi", "c_concat", "context", "y",
                                                                                   "c_crossattn", "c_adm")})
        disc = is_disc(unet) if unet is not None else "t1" in model_kwargs      # a foreign callable: the form its kwargs spell
        if disc:
            planes = [model_kwargs[k].to(device) for k in ("t1", "t2", "dwi")]          # KeyError as the reference's (:840)
        else:
            planes = model_kwargs.get("c_concat")
            if planes is None and "F_Data1" in model_kwargs:                            # training_project :881-884
                planes = [model_kwargs["F_Data1"], model_kwargs["F_Data2"], model_kwargs["S_Data1"]]
                if "edge" in model_kwargs:
                    planes.append(model_kwargs["edge"])
            planes = [planes] if th.is_tensor(planes) else planes
            planes = None if planes is None else [c.to(device) for c in planes]
        learned = self.model_var_type == ModelVarType.LEARNED_RANGE
        kl = self.loss_type.is_vb()
        want_vb = kl or learned
        pred = self._pred_code()                                        # p_mean_variance's reading of the output (vb)
        if self.parameterization not in ("eps", "x0", "v"):             # :878-885: the target follows `parameterization` alone
            raise NotImplementedError(f"Parameterization {self.parameterization} not yet supported")
        target = {"eps": _lib.PRED_EPS, "x0": _lib.PRED_X0, "v": _lib.PRED_V}[self.parameterization]
        if kl:
            disentangle = None
        if disentangle is not None and (disc or (unet is not None and _sched.is_latent_denoiser(unet))):
            raise ValueError(f"disentangle= needs the content / style / anatomy / lesion heads of a DSUnetModel; "
                             f"{type(unet).__name__ if unet is not None else 'the DisC-Diff form (t1 / t2 / dwi)'} has none")
        rider = None
        if unet is not None:
            bundle = kwargs_conditioning(unet, model, model_kwargs, device) if not is_dit(unet) and not disc else None
            if bundle is None:
                if planes is None and is_dit(unet):
                    planes = [xs.new_zeros((xs.shape[0], 0) + tuple(xs.shape[2:]))]
                if planes is None:
                    raise KeyError("training_losses needs the condition: 'c_concat', or 'F_Data1' / 'F_Data2' / 'S_Data1' [/ 'edge']")
                bundle = th.cat(planes, 1)
            if disentangle is not None:
                rider = _sched.Disentangle(disentangle, xs.shape[0], device)
            got = run_eval_loss(unet, pred, _lib.LOSS_CHARBONNIER, xs, bundle, t_model, a, s, noise=noise, seed=seed,
                                vlb=vlb if want_vb else None, learned_range=learned, target=target, disentangle=rider)
        else:
            rows = [th.from_numpy(np.ascontiguousarray(r)).to(device) for r in (a, s)]
            x_t = q_sample_rows(rows[0], rows[1], xs, noise, seed, 0)
            tv = th.from_numpy(np.ascontiguousarray(t_model)).to(device)
            x_in = x_t if planes is None or not disc else th.cat([x_t] + planes, 1)
            kw = {} if disc or planes is None else {"c_concat": planes}
            if kl:              # the KL types call the network inside p_mean_variance (:271-276): model(x_input, t, **model_kwargs)
                x_in, kw = (th.cat([x_t] + planes, 1) if model_kwargs.get("t1") is not None else x_t), dict(model_kwargs)
            full = model(x_in, tv if self.rescale_timesteps else tv.long(), **kw)
            out = model_output_of(full).float()
            got = {"mse": loss_rows(target, _lib.LOSS_CHARBONNIER, out, xs, noise, rows[0], rows[1], seed, 0)}
            if want_vb:
                got["vb"] = vlb_terms_rows(pred, learned, False, th.from_numpy(vlb[0]), th.from_numpy(vlb[1]), th.from_numpy(vlb[2]),
                                           out, x_t, xs, noise, seed, 0)[0]
            if disc and not kl:
                com = [f for f in full[0:4] if f is not None]
                dist = [f for f in full[4:8] if f is not None]
                got["com"], got["dist"] = pair_mse_rows(com), pair_mse_rows(dist)
            if disentangle is not None:
                if not (isinstance(full, tuple) and len(full) >= 2 and isinstance(full[1], dict)):
                    raise ValueError("disentangle= reads the feature dict a DSUnetModel returns beside its output: the model must "
                                     f"return (out, dict), got {type(full).__name__}")
                c_s, s_a_l = _sched.head_views(full[1])
                labels = [_sched.label_rows(l) for l in _sched.disentangle_labels(xs.shape[0], len(full[1]["content"]),
                                                                                 len(full[1]["style"]), len(full[1]["anatomy"]),
                                                                                 len(full[1]["lesion"]))]
                mode = {"contrast": "cl", "eu": "eu", "eu&contrast": "eu&cl"}[disentangle]
                l_cs, m_cs = _sched.contrast_rows(c_s, labels[0], mode, 0.05)           # :960-961
                l_sal, m_sal = _sched.contrast_rows(s_a_l, labels[1], mode, 0.1)        # :965-966 (the default temperature)
                got["disen"] = {"disen_c_s_loss": l_cs, "disen_s_a_l_loss": l_sal,
                                "contrast_map": {"c_s_heatmap": m_cs, "perfect_c_s_heatmap": _sched.perfect_logit(labels[0].to(device)),
                                                 "s_a_l_heatmap": m_sal, "perfect_s_a_l_heatmap": _sched.perfect_logit(labels[1].to(device))}}
        if rider is not None:
            got["disen"] = rider.terms()
        terms = {}
        if kl:                                                          # :841-851
            terms["loss"] = got["vb"] * self.num_timesteps if self.loss_type == LossType.RESCALED_KL else got["vb"]
            return terms
        if learned:                                                     # :857-877
            terms["vb"] = got["vb"]
            if self.loss_type == LossType.RESCALED_MSE:
                terms["vb"] = terms["vb"] * (self.num_timesteps / 1000.0)
        terms["mse"] = got["mse"]
        if disc:                                                        # :898-916
            terms["com"], terms["dist"] = got["com"], got["dist"]
            terms["disent"] = terms["com"] / terms["dist"]
            terms["loss"] = terms["mse"] + terms["disent"] + terms["vb"] if "vb" in terms else terms["mse"] + terms["disent"]
        else:                                                           # training_project :977-980
            terms.update(got.get("disen", {}))                          # :969-975 (the disentangle terms stay out of "loss")
            terms["loss"] = terms["mse"] + terms["vb"] if "vb" in terms else terms["mse"]
        return terms

    def get_disentangle_loss(self, feature, label, contrast='eu', temperature=0.1):
        """:1056-1094 on the device (dsd_op_contrast_rows): (loss, logits, perfect_logit) of ``feature`` [B, n_views, ...] (a CUDA
        tensor, read in place) and ``label`` [B, n_views].  'contrast': the supervised-contrastive loss on cosine / temperature;
        'eu': the same-label over different-label ratio of the Euclidean distances / n, returned matrix logits * 2 - 1;
        'eu&contrast': eu + 0.05 contrast with the cosine logits."""
        assert feature.shape[0] == label.shape[0]
        if contrast not in _sched.DISENTANGLE_MODES:
            raise NotImplementedError(f"contrast {contrast} not supported")
        if not feature.is_cuda:
            raise RuntimeError("get_disentangle_loss runs on the MI355X only (no CPU fallback): feature is on the CPU")
        rows = _sched.label_rows(label)
        loss, logits = _sched.contrast_rows(th.unbind(feature, dim=1), rows, contrast, temperature)
        return loss, logits, _sched.perfect_logit(rows.to(feature.device))


def _extract_into_tensor(arr, timesteps, broadcast_shape):
    """:994-1006."""
    res = th.from_numpy(arr).to(device=timesteps.device)[timesteps].float()
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res.expand(broadcast_shape)
