"""DPM-Solver / DPM-Solver++ sampler — native counterpart of the reference's
Disc_diff/guided_diffusion/sampler.py (NoiseScheduleVP :7-149, model_wrapper :151-302, DPM_Solver :305-1222) and of
its twin ldm/models/diffusion/dpm_solver_new/dpm_solver_pytorch.py.

The noise-schedule scalars are host-side fp32 torch expressions in the reference's operation order; the sampling loop
(network evaluation, data/noise prediction, dynamic thresholding, update) runs on the MI355X.  Built: ``method='multistep'``
with ``order`` 1..3, ``method='singlestep'`` ("DPM-Solver-fast", orders and times from
``get_orders_and_timesteps_for_singlestep_solver``) and ``method='singlestep_fixed'``, both ``algorithm_type``s, both
``solver_type``s, all three ``skip_type``s, ``lower_order_final``, ``denoise_to_zero``, ``return_intermediate``,
``DPM_Solver.inverse``, dynamic thresholding, classifier-free guidance (both halves in one 2B-row network pass).  Multistep of
order 1 or 2 without intermediates runs through ``dsd_sample_dpm`` (include/dsdiff.h); everything else is packed by
``build_program`` into a ``dsd_dpm_program`` — one row per network evaluation — for ``dsd_sample_dpm_program``.
``DPM_Solver.dpm_solver_adaptive`` is the adaptive step-size solver (:921-980): every trial — one singlestep step of ``order``
evaluations, the lower-order result from the same model values and the per-sample error norm between the two — is one call of
``dsd_sample_dpm_adaptive_trial``, and the host keeps what the reference keeps on (1,)-tensors: the step size, accept or
reject, the end test.  ``sample(method='adaptive')`` still raises and names that method; ``correcting_xt_fn``, classifier
guidance and score-type networks raise ``NotImplementedError`` — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ..._lib import (DPM_MS0, DPM_MS1, DPM_MS2, DPM_MS3, DPM_SS_S1, DPM_SS_S2, DPM_SS_T2, DPM_SS_T3, DPM_SS_T3_TAYLOR, DSD_DPM_NCOEF,
                      DSD_NCOEF, DsdDpmProgram, DsdDpmSchedule, check, dptr, lib, stream_ptr)
from ..._sched import (Conditioning, Guidance, cat_conditioning, cat_unconditional, check_latent_io, concat_of, conditioning_set,
                       is_dit, is_latent_denoiser, kwargs_conditioning, loop_denoiser, model_output_of, wrapper_key)

_PRED = {"noise": 0, "x_start": 1, "v": 2}


def interpolate_fn(x: torch.Tensor, xp: torch.Tensor, yp: torch.Tensor) -> torch.Tensor:
    """y(x) on the polyline (xp, yp); x [N,1], xp/yp [1,K]; outside the knots the end segments continue (:1224-1262).
    The knot interval is the slot x takes when sorted in with the knots (ties as torch.sort leaves them)."""
    K = xp.shape[1]
    merged = torch.cat([x, xp.expand(x.shape[0], K)], dim=1)
    slot = torch.argmin(torch.sort(merged, dim=1)[1], dim=1)             # knots sorted ahead of x
    j = (slot - 1).clamp(0, K - 2)
    x0, x1 = xp[0][j], xp[0][j + 1]
    y0, y1 = yp[0][j], yp[0][j + 1]
    return (y0 + (x[:, 0] - x0) * (y1 - y0) / (x1 - x0)).reshape(-1, 1)


class NoiseScheduleVP:
    """Forward VP-SDE wrapper (:7-149): log alpha_t, sigma_t, lambda_t = log alpha_t - log sigma_t and its inverse."""

    def __init__(self, schedule="discrete", betas=None, alphas_cumprod=None, continuous_beta_0=0.1,
                 continuous_beta_1=20., dtype=torch.float32):
        if schedule not in ["discrete", "linear"]:
            raise ValueError(
                "Unsupported noise schedule {}. The schedule needs to be 'discrete' or 'linear'".format(schedule))
        self.schedule = schedule
        self.T = 1.
        if schedule == "discrete":
            if betas is not None:
                log_alphas = 0.5 * torch.log(1 - betas.detach().cpu()).cumsum(dim=0)
            else:
                assert alphas_cumprod is not None
                log_alphas = 0.5 * torch.log(alphas_cumprod.detach().cpu())
            self.log_alpha_array = self.numerical_clip_alpha(log_alphas).reshape((1, -1,)).to(dtype=dtype)
            self.total_N = self.log_alpha_array.shape[1]
            self.t_array = torch.linspace(0., 1., self.total_N + 1)[1:].reshape((1, -1)).to(dtype=dtype)
        else:
            self.total_N = 1000
            self.beta_0 = continuous_beta_0
            self.beta_1 = continuous_beta_1

    def numerical_clip_alpha(self, log_alphas, clipped_lambda=-5.1):
        """:93-104 — cut the tail of the schedule whose half-logSNR is below ``clipped_lambda``."""
        lambs = log_alphas - 0.5 * torch.log(1. - torch.exp(2. * log_alphas))
        idx = int(torch.searchsorted(torch.flip(lambs, [0]), torch.tensor(clipped_lambda, dtype=lambs.dtype)))
        return log_alphas[:-idx] if idx > 0 else log_alphas

    def marginal_log_mean_coeff(self, t):
        t = torch.as_tensor(t, dtype=torch.float32).cpu()
        if self.schedule == "discrete":
            return interpolate_fn(t.reshape((-1, 1)), self.t_array, self.log_alpha_array).reshape((-1))
        return -0.25 * t ** 2 * (self.beta_1 - self.beta_0) - 0.5 * t * self.beta_0

    def marginal_alpha(self, t):
        return torch.exp(self.marginal_log_mean_coeff(t))

    def marginal_std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.marginal_log_mean_coeff(t)))

    def marginal_lambda(self, t):
        log_mean_coeff = self.marginal_log_mean_coeff(t)
        return log_mean_coeff - 0.5 * torch.log(1. - torch.exp(2. * log_mean_coeff))

    def inverse_lambda(self, lamb):
        lamb = torch.as_tensor(lamb, dtype=torch.float32).cpu()
        if self.schedule == "linear":
            tmp = 2. * (self.beta_1 - self.beta_0) * torch.logaddexp(-2. * lamb, torch.zeros((1,)))
            Delta = self.beta_0 ** 2 + tmp
            return tmp / (torch.sqrt(Delta) + self.beta_0) / (self.beta_1 - self.beta_0)
        log_alpha = -0.5 * torch.logaddexp(torch.zeros((1,)), -2. * lamb)
        return interpolate_fn(log_alpha.reshape((-1, 1)), torch.flip(self.log_alpha_array, [1]),
                              torch.flip(self.t_array, [1])).reshape((-1,))


class _ModelFn:
    """What ``model_wrapper`` returns: the network, its output type and its conditioning, kept apart so the solver can
    hand them to the device loop.  Calling it evaluates the noise prediction at continuous time (:247-279)."""

    def __init__(self, model, noise_schedule, model_type, model_kwargs, condition, unconditional_condition=None,
                 guidance_scale=1.):
        self.model, self.noise_schedule, self.model_type = model, noise_schedule, model_type
        self.model_kwargs, self.condition = dict(model_kwargs or {}), condition
        # classifier-free guidance (:324-332); None = off (guidance_scale 1.0 or no unconditional condition)
        self.unconditional_condition, self.guidance_scale = unconditional_condition, float(guidance_scale)

    def input_time(self, t_continuous):
        """get_model_input_time :236-245."""
        if self.noise_schedule.schedule == "discrete":
            return (t_continuous - 1. / self.noise_schedule.total_N) * 1000.
        return t_continuous

    def network(self, x, t_input):
        if self.condition is None:
            out = self.model(x, t_input, **self.model_kwargs)
        else:
            out = self.model(x, t_input, self.condition, **self.model_kwargs)
        return model_output_of(out)

    def bundle(self, unet, device):
        """The Conditioning of a UNetModel denoiser where the condition (or model_kwargs) carries more than ``c_concat``: the
        wrapper's c_crossattn / c_adm under its key, or the bare network's context= / y=.  None: the 'concat' path."""
        if unet is None or is_dit(unet) or not is_latent_denoiser(unet):
            return None
        if self.condition is None:
            return kwargs_conditioning(unet, self.model, self.model_kwargs, device)
        key = wrapper_key(self.model)
        if key in (None, "concat") and not (isinstance(self.condition, dict) and
                                            ("c_crossattn" in self.condition or "c_adm" in self.condition)):
            return None
        return cat_conditioning(self.condition, device, key)

    def c_concat(self) -> Optional[list]:
        src = self.condition if self.condition is not None else self.model_kwargs
        if isinstance(src, dict):
            src = src.get("c_concat")
        if isinstance(src, torch.Tensor):
            src = [src]
        return src

    def __call__(self, x, t_continuous):
        if self.unconditional_condition is not None:
            raise NotImplementedError("a guided model function is evaluated inside the device loop (DPM_Solver.sample) only")
        ns = self.noise_schedule
        t = torch.as_tensor(t_continuous, dtype=torch.float32).reshape(-1).expand(x.shape[0])
        out = self.network(x, self.input_time(t).to(x.device))
        if out.shape[1] == 2 * x.shape[1]:
            out = out[:, :x.shape[1]]
        if self.model_type == "noise":
            return out
        a = ns.marginal_alpha(t).to(x.device)[:, None, None, None]
        s = ns.marginal_std(t).to(x.device)[:, None, None, None]
        if self.model_type == "x_start":
            return (x - a * out) / s
        if self.model_type == "v":
            return a * out + s * x
        return -s * out                                                    # "score"


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond", condition=None,
                  unconditional_condition=None, guidance_scale=1., classifier_fn=None, classifier_kwargs={}):
    """:151-302 / dpm_solver_pytorch.py:188-336.  ``model`` is the denoiser as the reference passes it (the native
    DSUnetModel / UNetModel, a DiffusionWrapper around it, or any callable ``model(x, t_input, [cond], **model_kwargs)``).
    ``guidance_type="classifier-free"`` with an ``unconditional_condition`` and ``guidance_scale != 1`` (:324-332) runs the
    guided device loop; the unconditional condition comes in the form of ``condition``.  The reference takes tensors there (its
    ``torch.cat([unconditional_condition, condition])`` raises on anything else); the dict (``c_concat`` lists) and list forms
    are accepted as an extension."""
    assert model_type in ["noise", "x_start", "v", "score"]
    assert guidance_type in ["uncond", "classifier", "classifier-free"]
    if guidance_type == "classifier":
        raise NotImplementedError("classifier guidance (guidance_type='classifier': a classifier gradient per step) cannot run "
                                  "inside the device loop; classifier-free guidance can")
    if guidance_type == "classifier-free" and guidance_scale != 1. and unconditional_condition is not None:
        if model_type == "score":
            raise NotImplementedError("score-type networks are not part of the conditional-DDPM path")
        if condition is None:
            raise ValueError("classifier-free guidance needs the condition the unconditional one replaces")
        return _ModelFn(model, noise_schedule, model_type, model_kwargs, condition, unconditional_condition, guidance_scale)
    return _ModelFn(model, noise_schedule, model_type, model_kwargs, condition if guidance_type != "uncond" else None)


class DpmSchedule:
    """Owns the host arrays a dsd_dpm_schedule points to."""

    def __init__(self, pred, data_pred, thresholding, ratio, max_val, coef, t_input, order):
        steps = len(order)
        self.coef = np.ascontiguousarray(coef, dtype=np.float32).reshape(steps, DSD_NCOEF)
        self.t_input = np.ascontiguousarray(t_input, dtype=np.float32).reshape(steps)
        self.order = np.ascontiguousarray(order, dtype=np.int32).reshape(steps)
        self.c = DsdDpmSchedule()
        self.c.steps, self.c.pred, self.c.data_pred = steps, int(pred), int(data_pred)
        self.c.thresholding, self.c.threshold_ratio, self.c.threshold_max = int(thresholding), float(ratio), float(max_val)
        self.c.coef = self.coef.ctypes.data_as(C.POINTER(C.c_float))
        self.c.t_input = self.t_input.ctypes.data_as(C.POINTER(C.c_float))
        self.c.order = self.order.ctypes.data_as(C.POINTER(C.c_int32))

    @property
    def steps(self) -> int:
        return int(self.c.steps)


class DpmProgram:
    """Owns the host arrays a dsd_dpm_program points to: one row per network evaluation.  ``evals`` is a list of dicts with
    kind, t (continuous time, for the tests), t_input, alpha, sigma, coef (up to DSD_DPM_NCOEF scalars), slot (write, ma, mb,
    mc) and keep; ``lead_intermediate``: sample() puts x_T in front of the kept states (the multistep loop appends it :1147)."""

    def __init__(self, pred, data_pred, thresholding, ratio, max_val, evals, lead_intermediate=False):
        n = len(evals)
        self.evals, self.lead_intermediate = evals, bool(lead_intermediate)
        self.kind = np.asarray([e["kind"] for e in evals], dtype=np.int32).reshape(n)
        self.t_input = np.asarray([e["t_input"] for e in evals], dtype=np.float32).reshape(n)
        self.alpha = np.asarray([e["alpha"] for e in evals], dtype=np.float32).reshape(n)
        self.sigma = np.asarray([e["sigma"] for e in evals], dtype=np.float32).reshape(n)
        self.coef = np.zeros((n, DSD_DPM_NCOEF), dtype=np.float32)
        for k, e in enumerate(evals):
            self.coef[k, :len(e["coef"])] = np.asarray(e["coef"], dtype=np.float32)
        self.slot = np.ascontiguousarray([list(e["slot"]) for e in evals], dtype=np.int32).reshape(n, 4)
        self.keep = np.asarray([1 if e.get("keep") else 0 for e in evals], dtype=np.int32).reshape(n)
        self.c = DsdDpmProgram()
        self.c.n_eval, self.c.pred, self.c.data_pred = n, int(pred), int(data_pred)
        self.c.thresholding, self.c.threshold_ratio, self.c.threshold_max = int(thresholding), float(ratio), float(max_val)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        self.c.kind, self.c.t_input = self.kind.ctypes.data_as(i32p), self.t_input.ctypes.data_as(f32p)
        self.c.alpha, self.c.sigma = self.alpha.ctypes.data_as(f32p), self.sigma.ctypes.data_as(f32p)
        self.c.coef, self.c.slot = self.coef.ctypes.data_as(f32p), self.slot.ctypes.data_as(i32p)
        self.c.keep = self.keep.ctypes.data_as(i32p)

    @property
    def steps(self) -> int:
        return int(self.c.n_eval)

    @property
    def n_kept(self) -> int:
        return int(self.keep.sum())


class DPM_Solver:
    def __init__(self, model_fn, noise_schedule, algorithm_type="dpmsolver++", correcting_x0_fn=None,
                 correcting_xt_fn=None, thresholding_max_val=1., dynamic_thresholding_ratio=0.995):
        """:306-377."""
        assert algorithm_type in ["dpmsolver", "dpmsolver++"]
        if not isinstance(model_fn, _ModelFn):
            raise TypeError("model_fn must come from this module's model_wrapper(...) so the solver can reach the network")
        if model_fn.model_type == "score":
            raise NotImplementedError("score-type networks are not part of the conditional-DDPM path")
        if correcting_xt_fn is not None or not (correcting_x0_fn is None or correcting_x0_fn == "dynamic_thresholding"):
            raise NotImplementedError("python corrector callbacks (correcting_xt_fn, a callable correcting_x0_fn) cannot run inside the "
                                      "device loop")
        self.model_fn_ = model_fn
        self.noise_schedule = noise_schedule
        self.algorithm_type = algorithm_type
        self.correcting_x0_fn = correcting_x0_fn
        self.correcting_xt_fn = None
        self.dynamic_thresholding_ratio = dynamic_thresholding_ratio
        self.thresholding_max_val = thresholding_max_val

    # ------------------------------------------------------------------ host tables
    def get_time_steps(self, skip_type, t_T, t_0, N, device=None):
        """:416-443 (N+1 times from t_T down to t_0)."""
        ns = self.noise_schedule
        if skip_type == "logSNR":
            lambda_T = ns.marginal_lambda(torch.tensor(t_T))
            lambda_0 = ns.marginal_lambda(torch.tensor(t_0))
            return ns.inverse_lambda(torch.linspace(lambda_T.item(), lambda_0.item(), N + 1))
        elif skip_type == "time_uniform":
            return torch.linspace(t_T, t_0, N + 1)
        elif skip_type == "time_quadratic":
            return torch.linspace(t_T ** 0.5, t_0 ** 0.5, N + 1).pow(2)
        raise ValueError(
            "Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'".format(skip_type))

    def _time_range(self, t_start, t_end):
        """(t_T, t_0) of sample() :1113-1115."""
        ns = self.noise_schedule
        t_0 = 1. / ns.total_N if t_end is None else t_end
        t_T = ns.T if t_start is None else t_start
        assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
        return t_T, t_0

    def _multistep_evals(self, steps, t_T, t_0, order, skip_type, lower_order_final, solver_type, ev):
        """The evaluations of the multistep loop (:1130-1176), one ev(time, kind, coef, slot, keep) per step: the step's order,
        then cx, lead * phi_1 and, for order 2 (:784-815), cd and 1 / r0, for order 3 (:840-867) its six further terms — every
        scalar in the reference's fp32 expressions.  History planes k % 3, (k-1) % 3, (k-2) % 3.  The one place these are formed:
        build_schedule packs the rows of order <= 2 for dsd_sample_dpm, build_program all of them."""
        ns, pp = self.noise_schedule, self.algorithm_type == "dpmsolver++"
        assert steps >= order
        ts = self.get_time_steps(skip_type, t_T, t_0, steps)
        assert ts.shape[0] - 1 == steps
        lam = [ns.marginal_lambda(t) for t in ts]
        for k in range(steps):
            s, t, step = ts[k], ts[k + 1], k + 1
            if step < order:
                so = step
            elif lower_order_final and steps < 10:
                so = min(order, steps + 1 - step)
            else:
                so = order
            h = lam[k + 1] - lam[k]
            la_s, la_t = ns.marginal_log_mean_coeff(s), ns.marginal_log_mean_coeff(t)
            sig_s, sig_t = ns.marginal_std(s), ns.marginal_std(t)
            alpha_t = torch.exp(la_t)
            if pp:
                phi_1 = torch.expm1(-h)
                cx, lead = sig_t / sig_s, alpha_t
            else:
                phi_1 = torch.expm1(h)
                cx, lead = torch.exp(la_t - la_s), sig_t
            coef = [cx, lead * phi_1]
            if so == 2:
                h_0 = lam[k] - lam[k - 1]
                r0 = h_0 / h
                if solver_type == "dpmsolver":
                    cd = 0.5 * (lead * phi_1)
                elif pp:
                    cd = -(lead * (phi_1 / h + 1.))
                else:
                    cd = lead * (phi_1 / h - 1.)
                coef += [cd, 1. / r0]
            elif so == 3:
                h_1, h_0 = lam[k - 1] - lam[k - 2], lam[k] - lam[k - 1]
                r0, r1 = h_0 / h, h_1 / h
                phi_2 = phi_1 / h + 1. if pp else phi_1 / h - 1.
                phi_3 = phi_2 / h - 0.5
                c2 = lead * phi_2
                coef += [c2 if pp else -c2, lead * phi_3, 1. / r0, 1. / r1, r0 / (r0 + r1), 1. / (r0 + r1)]
            ev(s, (DPM_MS0, DPM_MS1, DPM_MS2, DPM_MS3)[so], coef, (k % 3, k % 3, (k - 1) % 3, (k - 2) % 3), True)

    def build_schedule(self, steps, t_start=None, t_end=None, order=2, skip_type="time_uniform",
                       lower_order_final=True, denoise_to_zero=False, solver_type="dpmsolver") -> DpmSchedule:
        """Per-evaluation coefficient rows of the multistep loop (:1130-1176) for dsd_sample_dpm: alpha, sigma, cx, lead * phi_1,
        cd, 1 / r0 of every step (the kind DPM_MS<o> of a row is its order o)."""
        if solver_type not in ["dpmsolver", "taylor"]:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        if order not in (1, 2):
            raise NotImplementedError("a dsd_dpm_schedule holds multistep order 1 and 2 (got {}); build_program packs order 3 and "
                                      "the singlestep solvers".format(order))
        t_T, t_0 = self._time_range(t_start, t_end)
        evals = []
        ev = lambda *row: evals.append(self._eval_row(*row))
        self._multistep_evals(steps, t_T, t_0, order, skip_type, lower_order_final, solver_type, ev)
        if denoise_to_zero:
            ev(torch.ones((1,)) * t_0, DPM_MS0, [], (0, 0, 0, 0), True)
        rows = [[e["alpha"], e["sigma"]] + (e["coef"] + [0.] * 4)[:4] + [0.] * (DSD_NCOEF - 6) for e in evals]
        thr = self.correcting_x0_fn == "dynamic_thresholding"
        return DpmSchedule(_PRED[self.model_fn_.model_type], self.algorithm_type == "dpmsolver++", thr, self.dynamic_thresholding_ratio,
                           self.thresholding_max_val, rows, [e["t_input"] for e in evals], [e["kind"] - DPM_MS0 for e in evals])

    def get_orders_and_timesteps_for_singlestep_solver(self, steps, order, skip_type, t_T, t_0, device=None):
        """The singlestep schedule of :445-501 ("DPM-Solver-fast"): ``steps`` evaluations spent on as many steps of ``order`` as
        fit, the rest on lower orders — order 3 ends on [1], [2] or, where ``steps`` divides by 3, on [2, 1] in place of a last
        third-order step; order 2 ends on [1] for an odd count.  Outer times: with 'logSNR' one spacing of K intervals (K =
        steps // 3 + 1 for order 3, the number of steps for order 2, and 1 for order 1, where the reference's loop then runs
        out of times after its first step); otherwise the grid of ``steps`` intervals read at the cumulated orders."""
        if order not in (1, 2, 3):
            raise ValueError("'order' must be '1' or '2' or '3'.")
        if order == 1:
            orders, K = [1] * steps, 1
        elif order == 2:
            orders = [2] * (steps // 2) + [1] * (steps % 2)
            K = len(orders)
        else:
            tail = {0: [2, 1], 1: [1], 2: [2]}[steps % 3]
            orders = [3] * ((steps - sum(tail)) // 3) + tail
            K = steps // 3 + 1
        if skip_type == "logSNR":
            return self.get_time_steps(skip_type, t_T, t_0, K), orders
        starts = np.concatenate([[0], np.cumsum(orders)])
        return self.get_time_steps(skip_type, t_T, t_0, steps)[torch.from_numpy(starts).long()], orders

    def _singlestep_evals(self, s, t, order, r1, r2, solver_type, ev):
        """The evaluations of one singlestep step from s to t (:509-553, :555-635, :637-758): every scalar the reference forms
        on its (1,)-tensors, in its expressions; where it writes '+ c * D' the row carries -c (the kernel subtracts)."""
        ns, pp = self.noise_schedule, self.algorithm_type == "dpmsolver++"
        lam_s, lam_t = ns.marginal_lambda(s), ns.marginal_lambda(t)
        h = lam_t - lam_s
        la_s, la_t = ns.marginal_log_mean_coeff(s), ns.marginal_log_mean_coeff(t)
        sig_s, sig_t = ns.marginal_std(s), ns.marginal_std(t)
        alpha_t = torch.exp(la_t)
        cx_to = lambda la_u, sig_u: sig_u / sig_s if pp else torch.exp(la_u - la_s)
        phi_1 = torch.expm1(-h) if pp else torch.expm1(h)
        lead_t = alpha_t if pp else sig_t
        if order == 1:
            ev(s, DPM_MS1, [cx_to(la_t, sig_t), lead_t * phi_1], (0, 0, 0, 0), True)
            return
        if r1 is None:
            r1 = 0.5 if order == 2 else 1. / 3.
        s1 = ns.inverse_lambda(lam_s + r1 * h)
        la_s1, sig_s1 = ns.marginal_log_mean_coeff(s1), ns.marginal_std(s1)
        phi_11 = torch.expm1(-r1 * h) if pp else torch.expm1(r1 * h)
        lead_s1 = torch.exp(la_s1) if pp else sig_s1
        ev(s, DPM_SS_S1, [cx_to(la_s1, sig_s1), lead_s1 * phi_11], (0, 0, 0, 0), False)
        if order == 2:
            if solver_type == "dpmsolver":
                cd = (0.5 / r1) * (lead_t * phi_1)
            elif pp:
                cd = -((1. / r1) * (alpha_t * (phi_1 / h + 1.)))
            else:
                cd = (1. / r1) * (sig_t * (phi_1 / h - 1.))
            ev(s1, DPM_SS_T2, [cx_to(la_t, sig_t), lead_t * phi_1, cd], (1, 0, 1, 0), True)
            return
        if r2 is None:
            r2 = 2. / 3.
        s2 = ns.inverse_lambda(lam_s + r2 * h)
        la_s2, sig_s2 = ns.marginal_log_mean_coeff(s2), ns.marginal_std(s2)
        lead_s2 = torch.exp(la_s2) if pp else sig_s2
        if pp:
            phi_12 = torch.expm1(-r2 * h)
            phi_22 = torch.expm1(-r2 * h) / (r2 * h) + 1.
            phi_2 = phi_1 / h + 1.
        else:
            phi_12 = torch.expm1(r2 * h)
            phi_22 = torch.expm1(r2 * h) / (r2 * h) - 1.
            phi_2 = phi_1 / h - 1.
        phi_3 = phi_2 / h - 0.5
        c_s2 = r2 / r1 * (lead_s2 * phi_22)
        ev(s1, DPM_SS_S2, [cx_to(la_s2, sig_s2), lead_s2 * phi_12, -c_s2 if pp else c_s2], (1, 0, 1, 0), False)
        if solver_type == "dpmsolver":
            c_t = (1. / r2) * (lead_t * phi_2)
            ev(s2, DPM_SS_T3, [cx_to(la_t, sig_t), lead_t * phi_1, -c_t if pp else c_t], (2, 0, 2, 0), True)
        else:
            c2 = lead_t * phi_2
            ev(s2, DPM_SS_T3_TAYLOR, [cx_to(la_t, sig_t), lead_t * phi_1, c2 if pp else -c2, lead_t * phi_3, 1. / r1, 1. / r2, r1, r2,
                                      r2 - r1], (2, 0, 1, 2), True)

    def _eval_row(self, t_eval, kind, coef, slot, keep):
        """One DpmProgram row: the evaluation's time, model time, alpha / sigma there and its coefficients as fp32 values."""
        ns = self.noise_schedule
        f = lambda v: float(torch.as_tensor(v, dtype=torch.float32).reshape(-1)[0])
        t_eval = torch.as_tensor(t_eval, dtype=torch.float32).reshape(-1)
        return dict(kind=kind, t=f(t_eval), t_input=f(self.model_fn_.input_time(t_eval)), alpha=f(ns.marginal_alpha(t_eval)),
                    sigma=f(ns.marginal_std(t_eval)), coef=[f(v) for v in coef], slot=slot, keep=bool(keep))

    def build_program(self, steps, t_start=None, t_end=None, order=2, skip_type="time_uniform", method="multistep",
                      lower_order_final=True, denoise_to_zero=False, solver_type="dpmsolver",
                      return_intermediate=False) -> DpmProgram:
        """One row per network evaluation of sample() (:1121-1213) for dsd_sample_dpm_program: the multistep loop of order 1..3
        (history planes k % 3, (k-1) % 3, (k-2) % 3) or the singlestep / singlestep_fixed loop (model_s, model_s1, model_s2 in
        planes 0, 1, 2; r1 / r2 from lambda_inner :1192-1200)."""
        if solver_type not in ["dpmsolver", "taylor"]:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        if method == "adaptive":
            raise NotImplementedError("method='adaptive' is not a program of evaluations: its step count follows a per-step error norm, "
                                      "read back every trial.  Call DPM_Solver.dpm_solver_adaptive(x, order, t_T, t_0, atol=, rtol=) "
                                      "— sample() passes it exactly these")
        if method not in ("multistep", "singlestep", "singlestep_fixed"):
            raise ValueError("Got wrong method {}".format(method))
        if order not in (1, 2, 3):
            raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))
        ns, pp = self.noise_schedule, self.algorithm_type == "dpmsolver++"
        t_T, t_0 = self._time_range(t_start, t_end)
        evals = []

        def ev(t_eval, kind, coef, slot, keep):
            evals.append(self._eval_row(t_eval, kind, coef, slot, keep and return_intermediate))

        if method == "multistep":
            self._multistep_evals(steps, t_T, t_0, order, skip_type, lower_order_final, solver_type, ev)
        else:
            if method == "singlestep":
                outer, orders = self.get_orders_and_timesteps_for_singlestep_solver(steps, order, skip_type, t_T, t_0)
            else:
                K = steps // order
                orders = [order, ] * K
                outer = self.get_time_steps(skip_type, t_T, t_0, K)
            for step, so in enumerate(orders):
                s, t = outer[step], outer[step + 1]
                lam_in = ns.marginal_lambda(self.get_time_steps(skip_type, s.item(), t.item(), so))
                h_in = lam_in[-1] - lam_in[0]
                r1 = None if so <= 1 else (lam_in[1] - lam_in[0]) / h_in
                r2 = None if so <= 2 else (lam_in[2] - lam_in[0]) / h_in
                self._singlestep_evals(s, t, so, r1, r2, solver_type, ev)
        if denoise_to_zero:
            w = len(evals) % 3
            ev(torch.ones((1,)) * t_0, DPM_MS0, [], (w, w, w, w), True)
        thr = self.correcting_x0_fn == "dynamic_thresholding"
        return DpmProgram(_PRED[self.model_fn_.model_type], pp, thr, self.dynamic_thresholding_ratio, self.thresholding_max_val,
                          evals, lead_intermediate=return_intermediate and method == "multistep")

    # ------------------------------------------------------------------ device loop
    @torch.no_grad()
    def sample(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type="time_uniform", method="multistep",
               lower_order_final=True, denoise_to_zero=False, solver_type="dpmsolver", atol=0.0078, rtol=0.05,
               return_intermediate=False):
        """:1017-1217.  x: the state at t_start on the GPU ([B,1,H,W], or [B,Cz,h,w] latents); returns the sample at t_end, with
        ``return_intermediate`` the pair (sample, list of the states the reference appends)."""
        if method == "multistep" and order in (1, 2) and not return_intermediate:
            sched = self.build_schedule(steps, t_start, t_end, order, skip_type, lower_order_final, denoise_to_zero,
                                        solver_type)
            return run_dpm_loop(self.model_fn_, sched, x)
        prog = self.build_program(steps, t_start, t_end, order, skip_type, method, lower_order_final, denoise_to_zero,
                                  solver_type, return_intermediate)
        y, kept = run_dpm_program(self.model_fn_, prog, x)
        if not return_intermediate:
            return y
        lead = [x.detach().float().clone()] if prog.lead_intermediate else []
        return y, lead + list(kept.unbind(0))

    # ------------------------------------------------------------------ adaptive step size
    def adaptive_trial_program(self, s, t, order, solver_type="dpmsolver"):
        """One trial of dpm_solver_adaptive from s to t (:949-968): (the DpmProgram of the higher-order singlestep step — r1 = 0.5,
        or r1 = 1/3 and r2 = 2/3, as Python floats like the reference's — and the three coefficients of the update of order - 1
        from the same model values).  Order 2: dpm_solver_first_update, the first parenthesis of the SS_T2 row; order 3: the
        second-order singlestep update with r1 = 1/3, whose model_s1 is the one the third-order step evaluates."""
        if order not in (2, 3):
            raise ValueError("For adaptive step size solver, order must be 2 or 3, got {}".format(order))
        if solver_type not in ["dpmsolver", "taylor"]:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        evals, low = [], []
        r1, r2 = (0.5, None) if order == 2 else (1. / 3., 2. / 3.)
        self._singlestep_evals(s, t, order, r1, r2, solver_type, lambda *row: evals.append(self._eval_row(*row[:4], False)))
        if order == 2:
            lower = evals[-1]["coef"][:2] + [0.]
        else:
            self._singlestep_evals(s, t, 2, r1, None, solver_type, lambda *row: low.append(self._eval_row(*row[:4], False)))
            lower = low[-1]["coef"][:3]
        thr = self.correcting_x0_fn == "dynamic_thresholding"
        prog = DpmProgram(_PRED[self.model_fn_.model_type], self.algorithm_type == "dpmsolver++", thr,
                          self.dynamic_thresholding_ratio, self.thresholding_max_val, evals)
        return prog, np.asarray(lower, dtype=np.float32)

    @torch.no_grad()
    def dpm_solver_adaptive(self, x, order, t_T, t_0, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5,
                            solver_type='dpmsolver', max_nfe=None, return_trace=False):
        """:921-980 — the adaptive step-size solver on singlestep DPM-Solver of ``order`` 2 or 3: the reference's signature and
        return value.  The host side is the reference's own fp32 expressions on (1,)-tensors; a trial (``order`` network
        evaluations, x_lower, the error norm) is one device call whose B error norms are read back.  Extensions: ``max_nfe`` —
        the reference has no guard; with it a loop that would pass that many evaluations raises RuntimeError with the count;
        ``return_trace`` — returns (x_0, [(s, t, h, E, accepted) per trial])."""
        if order not in (2, 3):
            raise ValueError("For adaptive step size solver, order must be 2 or 3, got {}".format(order))
        if solver_type not in ["dpmsolver", "taylor"]:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        if not (t_T > t_0 > 0):
            raise ValueError(f"dpm_solver_adaptive integrates down from t_T to t_0 > 0 (got t_T {t_T}, t_0 {t_0}); the adaptive "
                             "inverse is not built")
        if not (atol > 0 and rtol >= 0 and theta > 0 and h_init > 0):
            raise ValueError(f"dpm_solver_adaptive needs atol > 0, rtol >= 0, theta > 0 and h_init > 0 (got atol {atol}, rtol {rtol}, "
                             f"theta {theta}, h_init {h_init})")
        if not x.is_cuda:
            raise NotImplementedError("the adaptive solver runs on the MI355X only (there is no CPU implementation and no CPU "
                                      "fallback): x is on the CPU")
        ns = self.noise_schedule
        s = t_T * torch.ones((1,))
        lambda_s = ns.marginal_lambda(s)
        lambda_0 = ns.marginal_lambda(t_0 * torch.ones_like(s))
        h = h_init * torch.ones_like(s)
        x = x.detach().float().contiguous()
        x_prev = x
        nfe, trace = 0, []
        with AdaptiveTrial(self.model_fn_, x, order) as trial:
            while torch.abs((s - t_0)).mean() > t_err:
                if max_nfe is not None and nfe + order > max_nfe:
                    raise RuntimeError(f"dpm_solver_adaptive did not reach t_0 = {t_0} within max_nfe = {max_nfe} network evaluations: "
                                       f"{nfe} spent in {len(trace)} trials, now at s = {float(s):.6g} with h = {float(h):.3g}")
                t = ns.inverse_lambda(lambda_s + h)
                prog, lower = self.adaptive_trial_program(s, t, order, solver_type)
                x_higher, x_lower, E_b = trial.run(prog, lower, atol, rtol, x, x_prev)
                E = E_b.max()
                accepted = bool(torch.all(E <= 1.))
                trace.append((float(s), float(t), float(h), float(E), accepted))
                if accepted:
                    x = x_higher
                    s = t
                    x_prev = x_lower
                    lambda_s = ns.marginal_lambda(s)
                h = torch.min(theta * h * torch.float_power(E, -1. / order).float(), lambda_0 - lambda_s)
                nfe += order
        return (x, trace) if return_trace else x

    def inverse(self, x, steps=20, t_start=None, t_end=None, **sample_kwargs):
        """DPM_Solver.inverse (:1001-1015): sample() run upwards in time, from ``t_start`` (default: the schedule's first time,
        1/N) to ``t_end`` (default T); every other argument is sample()'s."""
        ns = self.noise_schedule
        lo = 1. / ns.total_N if t_start is None else t_start
        hi = ns.T if t_end is None else t_end
        assert lo > 0 and hi > 0, f"inverse needs positive times, got t_start {lo} and t_end {hi}"
        return self.sample(x, steps, lo, hi, **sample_kwargs)


def _loop_denoiser_and_guidance(fn: "_ModelFn", steps: int, x_T: torch.Tensor, guidance: Optional[Guidance]):
    """What both DPM routes settle before they touch the device: the native denoiser behind ``fn`` (None: the per-step path), the
    'concat' condition, and the guidance — the caller's, or what ``fn`` carries from model_wrapper — checked against them."""
    unet, cc = loop_denoiser(fn.model, fn.model_kwargs), fn.c_concat()   # None for a DiT that is to receive labels / cond=
    bundle = fn.bundle(unet, x_T.device)
    if bundle is not None:
        cc = [concat_of(bundle, x_T)]
    if guidance is None and fn.unconditional_condition is not None:
        u = cat_unconditional(fn.condition, fn.unconditional_condition, x_T.device, wrapper_key(fn.model) if bundle is not None else None)
        guidance = Guidance(u if isinstance(u, Conditioning) else u.detach().float(), fn.guidance_scale, steps)
    if guidance is not None:
        if cc is None:
            raise ValueError("classifier-free guidance needs the 'concat' condition the unconditional one replaces")
        guidance.check(bundle if bundle is not None else torch.cat([c.to(x_T.device) for c in cc], 1).detach().float(), steps)
        if unet is None:
            raise NotImplementedError("classifier-free guidance runs in the device loop only: it needs a native DSUnetModel / "
                                      "UNetModel / DiT behind the model")
    return unet, cc, guidance, bundle


def _native_loop_inputs(unet, cc, bundle, guidance: Optional[Guidance], x: torch.Tensor):
    """What a device DPM loop hands the library for a native denoiser: (the 'concat' tensor, the bound guidance or None, the context
    manager that holds the rest of the conditioning on the handle); None for the per-step path."""
    if unet is not None and cc is None and is_dit(unet):
        cc = [x.new_zeros((x.shape[0], 0) + tuple(x.shape[2:]))]    # an unconditional DiT: all input is state
    if unet is None or cc is None:
        return None
    unet.sync_params()
    cond = torch.cat([c.to(x.device) for c in cc], 1).detach().float().contiguous()
    if is_latent_denoiser(unet):
        check_latent_io(unet, x, bundle if bundle is not None else cond)
    else:
        assert x.shape[1] == 1, "the denoised image has one channel"
        assert cond.shape[0] == x.shape[0] and cond.shape[2:] == x.shape[2:]
    g = C.byref(guidance.bind()) if guidance is not None else None
    return cond, g, conditioning_set(unet, bundle, guidance.uncond if guidance is not None else None)


@torch.no_grad()
def run_dpm_loop(fn: _ModelFn, sched: DpmSchedule, x_T: torch.Tensor, guidance: Optional[Guidance] = None) -> torch.Tensor:
    """The multistep loop on the device (dsd_sample_dpm).  ``guidance`` (default: what ``fn`` carries from model_wrapper):
    classifier-free guidance; its unconditional conditioning must have the shape, dtype and device of the concatenated condition."""
    unet, cc, guidance, bundle = _loop_denoiser_and_guidance(fn, sched.steps, x_T, guidance)
    if not x_T.is_cuda:
        raise RuntimeError("sampling runs on the MI355X only (no CPU fallback): x is on the CPU")
    x = x_T.detach().float().contiguous().clone()
    B, Cx, H, W = x.shape
    ready = _native_loop_inputs(unet, cc, bundle, guidance, x)
    if ready is not None:
        cond, g, held = ready
        with held:
            check(lib().dsd_sample_dpm(unet._h, C.byref(sched.c), g, dptr(cond), cond.shape[1], dptr(x), Cx, B, H, W, stream_ptr()))
        return x
    assert Cx == 1, "the denoised image has one channel"
    # any other callable: python loop over the network, fused HIP post-network step per evaluation
    m_cur, m_prev = torch.empty_like(x), torch.empty_like(x)
    for k in range(sched.steps):
        t_in = torch.full((B,), float(sched.t_input[k]), device=x.device, dtype=torch.float32)
        out = fn.network(x, t_in).float().contiguous()
        check(lib().dsd_op_dpm_step(C.byref(sched.c), k, dptr(out), out.shape[1], dptr(x), dptr(m_cur), dptr(m_prev), B, H, W,
                                    stream_ptr()))
        m_cur, m_prev = m_prev, m_cur
    return x


def _run_program_per_evaluation(fn: _ModelFn, prog: DpmProgram, x: torch.Tensor, kept: Optional[torch.Tensor] = None):
    """A DpmProgram on ``x`` (in place) for any callable that is no native denoiser: a python loop over the network with the
    fused HIP evaluation step (dsd_op_dpm_eval) after each call; the states the program keeps go to ``kept``.  Returns the
    history planes and the base plane the program left."""
    B, Cx, H, W = x.shape
    hist, base = x.new_empty((3, B, Cx, H, W)), torch.empty_like(x)
    j = 0
    for k in range(prog.steps):
        t_in = torch.full((B,), float(prog.t_input[k]), device=x.device, dtype=torch.float32)
        out = fn.network(x, t_in).float().contiguous()
        if out.shape[1] not in (Cx, 2 * Cx):
            raise ValueError(f"the network returned {out.shape[1]} channels for a state of {Cx}")
        check(lib().dsd_op_dpm_eval(C.byref(prog.c), k, None, dptr(out), out.shape[1] // Cx, 1., dptr(x), 0, dptr(hist), dptr(base),
                                    B, Cx, H, W, stream_ptr()))
        if prog.keep[k]:
            kept[j].copy_(x)
            j += 1
    return hist, base


@torch.no_grad()
def run_dpm_program(fn: _ModelFn, prog: DpmProgram, x_T: torch.Tensor, guidance: Optional[Guidance] = None):
    """A DpmProgram on the device: dsd_sample_dpm_program for the native denoisers, guided or not, and for any other
    callable the python loop over the network with dsd_op_dpm_eval per evaluation.  Returns (sample, kept states
    [n_kept,B,C,H,W])."""
    unet, cc, guidance, bundle = _loop_denoiser_and_guidance(fn, prog.steps, x_T, guidance)
    if not x_T.is_cuda:
        raise NotImplementedError("the singlestep, third-order and intermediate-keeping solvers run on the MI355X only (there is "
                                  "no CPU implementation and no CPU fallback): x is on the CPU")
    x = x_T.detach().float().contiguous().clone()
    B, Cx, H, W = x.shape
    kept = x.new_empty((prog.n_kept, B, Cx, H, W))
    ready = _native_loop_inputs(unet, cc, bundle, guidance, x)
    if ready is not None:
        cond, g, held = ready
        with held:
            check(lib().dsd_sample_dpm_program(unet._h, C.byref(prog.c), g, dptr(cond), cond.shape[1], dptr(x), Cx, B, H, W,
                                               dptr(kept), stream_ptr()))
        return x, kept
    _run_program_per_evaluation(fn, prog, x, kept)
    return x, kept


class AdaptiveTrial:
    """The device side of dpm_solver_adaptive's trials for one start state: settles once what every trial shares — the native
    denoiser behind ``fn`` (or the per-evaluation path of any other callable), the 'concat' condition, the guidance with one scale
    per evaluation, the rest of the conditioning held on the handle — and ``run`` executes one trial."""

    def __init__(self, fn: _ModelFn, x: torch.Tensor, order: int, guidance: Optional[Guidance] = None):
        self.fn, self.order = fn, int(order)
        self.unet, cc, self.guidance, bundle = _loop_denoiser_and_guidance(fn, self.order, x, guidance)
        if not x.is_cuda:
            raise NotImplementedError("the adaptive solver runs on the MI355X only (there is no CPU implementation and no CPU "
                                      "fallback): x is on the CPU")
        self.ready = _native_loop_inputs(self.unet, cc, bundle, self.guidance, x.detach().float().contiguous())
        self.err = np.zeros(x.shape[0], dtype=np.float32)

    def __enter__(self):
        if self.ready is not None:
            self.ready[2].__enter__()
        return self

    def __exit__(self, *exc):
        if self.ready is not None:
            return self.ready[2].__exit__(*exc)
        return False

    @torch.no_grad()
    def run(self, prog: DpmProgram, lower, atol, rtol, x: torch.Tensor, x_prev: torch.Tensor):
        """One trial from the state ``x`` (left as it is): returns (x_higher, x_lower, E [B] on the CPU)."""
        if prog.steps != self.order:
            raise ValueError(f"a trial of order {self.order} has {self.order} evaluations; the program has {prog.steps}")
        if x_prev.shape != x.shape or x_prev.device != x.device or x_prev.dtype != torch.float32 or x.dtype != torch.float32:
            raise ValueError(f"x_prev must have the shape, dtype and device of x: {tuple(x_prev.shape)} {x_prev.dtype} {x_prev.device} "
                             f"against {tuple(x.shape)} {x.dtype} {x.device}")
        lower = np.ascontiguousarray(lower, dtype=np.float32).reshape(3)
        lp = lower.ctypes.data_as(C.POINTER(C.c_float))
        xh, x_prev = x.contiguous().clone(), x_prev.contiguous()
        x_lower = torch.empty_like(xh)
        B, Cx, H, W = xh.shape
        if self.ready is not None:
            cond, g, _ = self.ready
            check(lib().dsd_sample_dpm_adaptive_trial(self.unet._h, C.byref(prog.c), g, dptr(cond), cond.shape[1], lp, float(atol),
                                                      float(rtol), dptr(xh), dptr(x_prev), dptr(x_lower), Cx, B, H, W,
                                                      self.err.ctypes.data_as(C.POINTER(C.c_float)), stream_ptr()))
            return xh, x_lower, torch.from_numpy(self.err.copy())
        hist, base = _run_program_per_evaluation(self.fn, prog, xh)               # any other callable; then the error kernel
        err = torch.empty(B, device=xh.device, dtype=torch.float32)
        ma, mb = hist[int(prog.slot[0, 0])], hist[int(prog.slot[1, 0])]
        check(lib().dsd_op_dpm_adaptive_error(self.order - 1, lp, float(atol), float(rtol), dptr(base), dptr(ma), dptr(mb), dptr(xh), 0,
                                              dptr(x_prev), dptr(x_lower), dptr(err), B, Cx, H, W, stream_ptr()))
        return xh, x_lower, err.cpu()


@torch.no_grad()
def dynamic_thresholding(x0: torch.Tensor, ratio: float = 0.995, max_val: float = 1.):
    """DPM_Solver.dynamic_thresholding_fn :379-388 on the device.  Returns (thresholded x0, s [B])."""
    x0 = x0.detach().float().contiguous()
    B = x0.shape[0]
    y, s = torch.empty_like(x0), torch.empty(B, device=x0.device, dtype=torch.float32)
    check(lib().dsd_op_dpm_threshold(dptr(x0), B, x0[0].numel(), float(ratio), float(max_val), dptr(y), dptr(s), stream_ptr()))
    return y, s


def expand_dims(v, dims):
    """:1265-1274."""
    return v[(...,) + (None,) * (dims - 1)]
