"""Host side of dsd_sample: packs per-iteration fp32 coefficient rows and drives the device loop."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import DSD_NCOEF, DsdGuidance, DsdSchedule, check, dptr, lib, stream_ptr


class Schedule:
    """Owns the host arrays a dsd_schedule points to.  Row k = k-th executed iteration (largest t first)."""

    def __init__(self, mode: int, pred: int, coef: np.ndarray, t_model: np.ndarray, nonzero: np.ndarray,
                 learned_range: bool = False, clip_denoised: bool = True, eta: float = 0.0):
        steps = int(coef.shape[0])
        assert coef.shape == (steps, DSD_NCOEF) and t_model.shape == (steps,) and nonzero.shape == (steps,)
        self.coef = np.ascontiguousarray(coef, dtype=np.float32)
        self.t_model = np.ascontiguousarray(t_model, dtype=np.float32)
        self.nonzero = np.ascontiguousarray(nonzero, dtype=np.int32)
        self.c = DsdSchedule()
        self.c.steps, self.c.mode, self.c.pred = steps, int(mode), int(pred)
        self.c.learned_range, self.c.clip_denoised, self.c.eta = int(learned_range), int(clip_denoised), float(eta)
        self.c.coef = self.coef.ctypes.data_as(C.POINTER(C.c_float))
        self.c.t_model = self.t_model.ctypes.data_as(C.POINTER(C.c_float))
        self.c.nonzero = self.nonzero.ctypes.data_as(C.POINTER(C.c_int32))

    @property
    def steps(self) -> int:
        return int(self.c.steps)

    def with_pred(self, pred: int) -> "Schedule":
        """The same schedule for a network output of another kind (DSD_PRED_*): the denoised_fn hook hands the update kernel
        an x_start it has already formed and post-processed."""
        return Schedule(int(self.c.mode), int(pred), self.coef, self.t_model, self.nonzero, bool(self.c.learned_range),
                        bool(self.c.clip_denoised), float(self.c.eta))


class Guidance:
    """Classifier-free guidance of a device loop (dsd_guidance): the unconditional conditioning ``uncond``, laid out like the
    conditioning it replaces, and one fp32 scale per executed step — a constant ``unconditional_guidance_scale`` is the array
    filled with it, ``ucg_schedule`` is the array itself (ddim.py:165-167)."""

    def __init__(self, uncond: torch.Tensor, scale, steps: int):
        if uncond is None:
            raise ValueError("guidance needs the unconditional conditioning")
        if np.ndim(scale) == 0:
            scale = np.full(int(steps), float(scale))
        self.scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        if self.scale.shape[0] != int(steps):
            raise ValueError(f"guidance carries {self.scale.shape[0]} scales but the loop executes {int(steps)} steps "
                             "(ucg_schedule needs one scale per step)")
        self.uncond = uncond

    def check(self, cond: torch.Tensor, steps: int) -> None:
        u = self.uncond
        if self.scale.shape[0] != int(steps):
            raise ValueError(f"guidance carries {self.scale.shape[0]} scales but the schedule executes {int(steps)} steps")
        if not torch.is_tensor(u) or tuple(u.shape) != tuple(cond.shape) or u.dtype != cond.dtype or u.device != cond.device:
            raise ValueError("the unconditional conditioning must have the shape, dtype and device of the conditioning: "
                             f"{tuple(getattr(u, 'shape', ()))} {getattr(u, 'dtype', None)} {getattr(u, 'device', None)} against "
                             f"{tuple(cond.shape)} {cond.dtype} {cond.device}")

    def bind(self) -> DsdGuidance:
        """The C struct (the arrays it points to stay alive on self)."""
        self._u = self.uncond.detach().float().contiguous()
        g = DsdGuidance()
        g.uncond = self._u.data_ptr()
        g.scale = self.scale.ctypes.data_as(C.POINTER(C.c_float))
        g.n_scale = int(self.scale.shape[0])
        return g


def guidance_active(scale, uncond, ucg_schedule=None) -> bool:
    """ddim.py:194 / dpm_solver_pytorch.py:325: guidance is off without an unconditional conditioning or at scale 1.0."""
    if uncond is None:
        return False
    return ucg_schedule is not None or scale != 1.


def cat_conditioning(c, device):
    """The 'concat' conditioning in the three forms the reference takes (dict with c_concat lists, list, tensor) -> one
    [B,Cc,H,W] tensor on ``device``."""
    if isinstance(c, dict):
        c = c["c_concat"]
    parts = list(c) if isinstance(c, (list, tuple)) else [c]
    return torch.cat([t.to(device) for t in parts], 1)


def cat_unconditional(c, u, device):
    """The unconditional conditioning must come in the form of the conditioning, as p_sample_ddim asserts (ddim.py:199-217)."""
    if isinstance(c, dict):
        assert isinstance(u, dict), "unconditional_conditioning must be a dict like the conditioning"
        for k in c:
            assert k in u, f"unconditional_conditioning lacks the key {k!r}"
            if isinstance(c[k], list):
                assert isinstance(u[k], list) and len(u[k]) == len(c[k]), \
                    f"unconditional_conditioning[{k!r}] must be a list of {len(c[k])} tensors like the conditioning"
    elif isinstance(c, list):
        assert isinstance(u, list) and len(u) == len(c), "unconditional_conditioning must be a list like the conditioning"
    else:
        assert torch.is_tensor(u), "unconditional_conditioning must be a tensor like the conditioning"
    return cat_conditioning(u, device)


def find_unet(model):
    """Locate the native denoiser behind the object the reference passes as ``model``
    (DiffusionWrapper.diffusion_model, ddpm.py:1323; or the network itself): the four-stream DSUnetModel, or the plain
    UNetModel that denoises VAE latents (run by the latent loops, dsd_sample_latent / dsd_sample_dpm_latent)."""
    from .UNet_DS_Diff.model import DSUnetModel
    from .ldm.modules.diffusionmodules.openaimodel import UNetModel
    kinds = (DSUnetModel, UNetModel)
    if isinstance(model, kinds):
        return model
    inner = getattr(model, "diffusion_model", None)
    if isinstance(inner, kinds):
        return inner
    inner = getattr(getattr(model, "model", None), "diffusion_model", None)
    if isinstance(inner, kinds):
        return inner
    return None


def is_latent_denoiser(unet) -> bool:
    """True for the plain UNetModel (multi-channel latent state, DSD_BLOCK_UNET handle)."""
    from .ldm.modules.diffusionmodules.openaimodel import UNetModel
    return isinstance(unet, UNetModel)


def check_latent_io(unet, x: torch.Tensor, cond: torch.Tensor) -> None:
    """Shape checks of the latent loops that the C entry points cannot see (they take one H, W)."""
    if unet.use_spatial_transformer:
        raise ValueError("the latent loops take 'concat' conditioning only; this UNetModel has a spatial transformer")
    if cond.dim() != 4 or cond.shape[0] != x.shape[0] or tuple(cond.shape[2:]) != tuple(x.shape[2:]):
        raise ValueError(f"conditioning {tuple(cond.shape)} does not match the latent state {tuple(x.shape)} "
                         "(same batch and spatial size needed for the 'concat' conditioning)")


def _seed_from_torch() -> int:
    """Philox seed drawn from torch's CPU generator so torch.manual_seed() makes sampling reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


@torch.no_grad()
def run_device_loop(unet, sched: Schedule, x_T: torch.Tensor, cond: torch.Tensor,
                    step_noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                    first_step: int = 0, n_steps: int = 0, guidance: Optional[Guidance] = None) -> torch.Tensor:
    """x_T [B,1,H,W], cond [B,Cc,H,W] (CUDA fp32).  Returns x after the selected iterations.
    With the plain UNetModel the state is a latent x_T [B,Cz,H,W] (dsd_sample_latent; step_noise [steps,B,Cz,H,W]).
    ``guidance``: classifier-free guidance (dsd_sample_guided / dsd_sample_latent_guided, mode B_DDIM); its unconditional
    conditioning must have the shape, dtype and device of ``cond``."""
    if guidance is not None:
        guidance.check(cond, sched.steps)
    if unet is None:
        raise RuntimeError("no native denoiser (DSUnetModel / UNetModel) behind the model handed to the sampler")
    if not x_T.is_cuda:
        raise RuntimeError("sampling runs on the MI355X only (no CPU fallback): x_T is on the CPU")
    unet.sync_params()
    x = x_T.detach().float().contiguous().clone()
    cond = cond.detach().float().contiguous()
    g = guidance.bind() if guidance is not None else None
    if is_latent_denoiser(unet):
        check_latent_io(unet, x, cond)
        B, Cz, H, W = x.shape
        if step_noise is not None:
            step_noise = step_noise.detach().float().contiguous()
            if tuple(step_noise.shape) != (sched.steps, B, Cz, H, W):
                raise ValueError(f"step_noise must be [steps,B,Cz,H,W] = {(sched.steps, B, Cz, H, W)}, got {tuple(step_noise.shape)}")
        if seed is None:
            seed = _seed_from_torch()
        if g is not None:
            check(lib().dsd_sample_latent_guided(unet._h, C.byref(sched.c), C.byref(g), dptr(cond), cond.shape[1], dptr(x), Cz,
                                                 dptr(step_noise), C.c_uint64(seed), B, H, W, first_step, n_steps, stream_ptr()))
            return x
        check(lib().dsd_sample_latent(unet._h, C.byref(sched.c), dptr(cond), cond.shape[1], dptr(x), Cz, dptr(step_noise),
                                      C.c_uint64(seed), B, H, W, first_step, n_steps, stream_ptr()))
        return x
    B, Cx, H, W = x.shape
    assert Cx == 1 and cond.shape[0] == B and cond.shape[2:] == x.shape[2:]
    if step_noise is not None:
        step_noise = step_noise.detach().float().contiguous()
        assert step_noise.shape == (sched.steps, B, 1, H, W), "step_noise must be [steps,B,1,H,W]"
    if seed is None:
        seed = _seed_from_torch()
    if g is not None:
        check(lib().dsd_sample_guided(unet._h, C.byref(sched.c), C.byref(g), dptr(cond), cond.shape[1], dptr(x), dptr(step_noise),
                                      C.c_uint64(seed), B, H, W, first_step, n_steps, stream_ptr()))
        return x
    check(lib().dsd_sample(unet._h, C.byref(sched.c), dptr(cond), cond.shape[1], dptr(x), dptr(step_noise),
                           C.c_uint64(seed), B, H, W, first_step, n_steps, stream_ptr()))
    return x


@torch.no_grad()
def sampler_update(sched: Schedule, k: int, model_out: torch.Tensor, x: torch.Tensor,
                   noise: Optional[torch.Tensor], seed: int = 0, want_x0: bool = False):
    """One fused update (dsd_op_sampler_update); x is updated in place."""
    B, Cx, H, W = x.shape
    if Cx > 1:
        # multi-channel states (latents): the update is elementwise, so [B,C,H,W] is B*C one-channel images — except for
        # the learned-range variance, whose model output interleaves mean and variance channels per sample
        if sched.c.learned_range:
            raise NotImplementedError("learned-range variance on multi-channel states is not on the sampling hot path")
        B = B * Cx
    x0 = torch.empty_like(x) if want_x0 else None
    check(lib().dsd_op_sampler_update(C.byref(sched.c), k, dptr(model_out.float().contiguous()), dptr(x),
                                      dptr(noise.float().contiguous()) if noise is not None else None,
                                      C.c_uint64(seed), B, H, W, dptr(x0), stream_ptr()))
    return x0


@torch.no_grad()
def sampler_update_guided(sched: Schedule, k: int, out_uncond: torch.Tensor, out_cond: torch.Tensor, scale: float,
                          x2: torch.Tensor, noise: Optional[torch.Tensor], seed: int = 0, want_x0: bool = False,
                          state_channels: Optional[int] = None):
    """One guided DDIM update (dsd_op_sampler_update_guided).  ``x2`` holds the 2B state rows (uncond half first), updated in
    place: a contiguous [2B,Cz,H,W] tensor, or — with ``state_channels`` = Cz — a [2B,Cz+Cc,H,W] denoiser input whose first Cz
    channels are the state.  out_uncond / out_cond / noise are [B,Cz,H,W]."""
    B, Cz, H, W = out_cond.shape
    assert x2.shape[0] == 2 * B and x2.is_contiguous() and tuple(x2.shape[2:]) == (H, W)
    assert (state_channels or x2.shape[1]) == Cz
    x0 = torch.empty_like(out_cond, dtype=torch.float32) if want_x0 else None
    check(lib().dsd_op_sampler_update_guided(C.byref(sched.c), k, dptr(out_uncond.float().contiguous()),
                                             dptr(out_cond.float().contiguous()), float(scale), dptr(x2),
                                             x2.shape[1] * H * W, dptr(noise.float().contiguous()) if noise is not None else None,
                                             C.c_uint64(seed), B, Cz, H, W, dptr(x0), stream_ptr()))
    return x0
