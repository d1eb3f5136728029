"""Host side of dsd_sample: packs per-iteration fp32 coefficient rows and drives the device loop."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import (DSD_NCOEF, DsdBpd, DsdConditioning, DsdGuidance, DsdInpaint, DsdInvertSchedule, DsdSchedule, DsdTrace, check, dptr,
                   lib, stream_ptr)


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

    def check(self, cond, steps: int) -> None:
        u = self.uncond
        if self.scale.shape[0] != int(steps):
            raise ValueError(f"guidance carries {self.scale.shape[0]} scales but the schedule executes {int(steps)} steps")
        if isinstance(cond, Conditioning) or isinstance(u, Conditioning):
            # part by part, as p_sample_ddim pairs the two dicts key by key (ddim.py:199-217)
            if not (isinstance(cond, Conditioning) and isinstance(u, Conditioning)):
                raise ValueError("the unconditional conditioning must come in the form of the conditioning (a dict with its keys)")
            for name, key in (("concat", "c_concat"), ("context", "c_crossattn"), ("y", "c_adm")):
                a, b = getattr(cond, name), getattr(u, name)
                if (a is None) != (b is None):
                    raise ValueError(f"unconditional_conditioning and conditioning differ in {key!r}: guidance needs the "
                                     f"unconditional twin of every part ({name})")
                if a is not None and (tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype or a.device != b.device):
                    raise ValueError(f"the unconditional {key!r} must have the shape, dtype and device of the conditional one: "
                                     f"{tuple(b.shape)} {b.dtype} {b.device} against {tuple(a.shape)} {a.dtype} {a.device}")
            return
        if not torch.is_tensor(u) or tuple(u.shape) != tuple(cond.shape) or u.dtype != cond.dtype or u.device != cond.device:
            raise ValueError("the unconditional conditioning must have the shape, dtype and device of the conditioning: "
                             f"{tuple(getattr(u, 'shape', ()))} {getattr(u, 'dtype', None)} {getattr(u, 'device', None)} against "
                             f"{tuple(cond.shape)} {cond.dtype} {cond.device}")

    def bind(self) -> DsdGuidance:
        """The C struct (the arrays it points to stay alive on self)."""
        u = self.uncond.concat if isinstance(self.uncond, Conditioning) else self.uncond
        self._u = u.detach().float().contiguous() if u is not None and u.shape[1] else None
        g = DsdGuidance()
        g.uncond = self._u.data_ptr() if self._u is not None else None
        g.scale = self.scale.ctypes.data_as(C.POINTER(C.c_float))
        g.n_scale = int(self.scale.shape[0])
        return g


class Inpaint:
    """Masked sampling of a device loop (dsd_inpaint; ddim.py:160-163, ddpm.py:1085-1087): ``x0`` is the image the mask keeps,
    laid out like the state; ``mask`` is [B,1,H,W] (broadcast over the channels, the form log_images builds) or [B,C,H,W], 1 where
    x0 is kept and 0 where the loop samples; ``noise`` ([steps,B,C,H,W], optional) feeds q_sample's draws, else Philox."""

    def __init__(self, x0: torch.Tensor, mask: torch.Tensor, noise: Optional[torch.Tensor] = None):
        if mask is None:
            raise ValueError("masked sampling needs a mask")
        if x0 is None:
            raise ValueError("a mask needs the image it keeps (x0)")
        self.x0, self.mask, self.noise = x0, mask, noise

    def check(self, x: torch.Tensor, steps: int) -> None:
        """Against the state ``x`` [B,C,H,W] of a loop that executes ``steps`` iterations."""
        B, Cz, H, W = x.shape
        like = lambda t: torch.is_tensor(t) and t.dtype == x.dtype and t.device == x.device
        desc = lambda t: f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', None)} {getattr(t, 'device', None)}"
        if not like(self.x0) or tuple(self.x0.shape) != tuple(x.shape):
            raise ValueError(f"x0 must have the shape, dtype and device of the state: {desc(self.x0)} against {desc(x)}")
        if not like(self.mask) or self.mask.dim() != 4 or tuple(self.mask.shape) not in ((B, 1, H, W), (B, Cz, H, W)):
            raise ValueError(f"the mask must be [B,1,H,W] or [B,C,H,W] with the dtype and device of the state: {desc(self.mask)} "
                             f"against {desc(x)}")
        if self.noise is not None and (not like(self.noise) or tuple(self.noise.shape) != (int(steps), B, Cz, H, W)):
            raise ValueError(f"mask_noise must be [steps,B,C,H,W] = {(int(steps), B, Cz, H, W)} with the dtype and device of the "
                             f"state: {desc(self.noise)}")

    def bind(self) -> DsdInpaint:
        """The C struct (the tensors it points to stay alive on self)."""
        self._x0, self._mask = self.x0.detach().float().contiguous(), self.mask.detach().float().contiguous()
        self._noise = self.noise.detach().float().contiguous() if self.noise is not None else None
        p = DsdInpaint()
        p.x0, p.mask, p.mask_channels = self._x0.data_ptr(), self._mask.data_ptr(), int(self._mask.shape[1])
        p.noise = self._noise.data_ptr() if self._noise is not None else None
        return p


def guidance_active(scale, uncond, ucg_schedule=None) -> bool:
    """ddim.py:194 / dpm_solver_pytorch.py:325: guidance is off without an unconditional conditioning or at scale 1.0."""
    if uncond is None:
        return False
    return ucg_schedule is not None or scale != 1.


CONCAT_KEYS = ("concat", "hybrid", "hybrid-adm")
CONTEXT_KEYS = ("crossattn", "hybrid", "hybrid-adm", "crossattn-adm")
ADM_KEYS = ("hybrid-adm", "crossattn-adm")


class Conditioning:
    """The conditioning bundle of a latent device loop beside plain 'concat': ``concat`` [B,Cc,H,W] (appended to the state),
    ``context`` [B,tokens,context_dim] (cross-attention) and ``y`` (the label_emb input: int labels [B] or vectors [B,width]),
    each a tensor or None — what DiffusionWrapper.forward (ddpm.py:1328-1365) makes of the reference's conditioning dict."""

    def __init__(self, concat=None, context=None, y=None):
        self.concat, self.context, self.y = concat, context, y

    def __eq__(self, other):
        if not isinstance(other, Conditioning):
            return NotImplemented
        same = lambda a, b: (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))
        return same(self.concat, other.concat) and same(self.context, other.context) and same(self.y, other.y)

    __hash__ = None

    def __repr__(self):
        d = lambda t: None if t is None else tuple(t.shape)
        return f"Conditioning(concat={d(self.concat)}, context={d(self.context)}, y={d(self.y)})"


def conditioning_key_of(c) -> Optional[str]:
    """The conditioning key a dict spells out by the entries it carries (None where it cannot: 'adm' reads its vector from
    ``c_crossattn[0]`` and is told apart by the wrapper's key only)."""
    if not isinstance(c, dict):
        return "concat"
    has = tuple(k in c and c[k] is not None for k in ("c_concat", "c_crossattn", "c_adm"))
    return {(True, False, False): "concat", (False, True, False): "crossattn", (True, True, False): "hybrid",
            (True, True, True): "hybrid-adm", (False, True, True): "crossattn-adm"}.get(has)


def _parts(c, name, key, device):
    if not isinstance(c, dict) or name not in c or c[name] is None:
        raise ValueError(f"the conditioning lacks {name!r}, which conditioning_key={key!r} reads")
    v = c[name]
    parts = list(v) if isinstance(v, (list, tuple)) else [v]
    if not parts or not all(torch.is_tensor(t) for t in parts):
        raise ValueError(f"conditioning[{name!r}] must be a tensor or a non-empty list of tensors")
    return [t.to(device) for t in parts]


def cat_conditioning(c, device, key: Optional[str] = None):
    """What the denoiser receives of a conditioning in the forms the reference takes, on ``device``.  ``key``: the wrapper's
    conditioning_key (default: read off the dict's entries).  Under 'concat' — a dict with c_concat lists, a list, a tensor — one
    [B,Cc,H,W] tensor; under every other key a Conditioning: c_concat joined along the channels where the key has it,
    c_crossattn along the tokens, ``y`` = c_adm, or c_crossattn[0] under 'adm' (ddpm.py:1328-1365).  A list or tensor under a
    key other than 'concat' is c_crossattn, as apply_model files it (:862-866)."""
    if key is None:
        key = conditioning_key_of(c)
        if key is None:
            raise ValueError(f"cannot tell the conditioning key from the entries {sorted(c)}: c_concat, c_crossattn (+ c_adm) "
                             "combine to 'concat', 'crossattn', 'hybrid', 'hybrid-adm', 'crossattn-adm'")
    if key == "concat":
        if isinstance(c, dict):
            c = c["c_concat"]
        parts = list(c) if isinstance(c, (list, tuple)) else [c]
        return torch.cat([t.to(device) for t in parts], 1)
    if not isinstance(c, dict):
        c = {"c_crossattn": list(c) if isinstance(c, (list, tuple)) else [c]}
    out = Conditioning()
    if key in CONCAT_KEYS:
        out.concat = torch.cat(_parts(c, "c_concat", key, device), 1)
    if key in CONTEXT_KEYS:
        out.context = torch.cat(_parts(c, "c_crossattn", key, device), 1)
        if out.context.dim() != 3:
            raise ValueError(f"conditioning['c_crossattn'] must hold [B, tokens, context_dim] tensors, got {tuple(out.context.shape)}")
    if key in ADM_KEYS:
        adm = _parts(c, "c_adm", key, device)
        if len(adm) != 1:
            raise ValueError("conditioning['c_adm'] must be one tensor")
        out.y = adm[0]
    elif key == "adm":
        out.y = _parts(c, "c_crossattn", key, device)[0]
    elif key not in CONTEXT_KEYS:
        raise ValueError(f"conditioning_key={key!r} is not one the reference's DiffusionWrapper dispatches")
    return out


def cat_unconditional(c, u, device, key: Optional[str] = None):
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
    if key is None and isinstance(c, dict):
        key = conditioning_key_of(c)
    return cat_conditioning(u, device, key)


def wrapper_key(model) -> Optional[str]:
    """The conditioning_key of the DiffusionWrapper behind what a sampler was handed (None: no wrapper, or an unconditional
    one — the conditioning's own entries then say what it is)."""
    for m in (model, getattr(model, "model", None)):
        k = getattr(m, "conditioning_key", None)
        if isinstance(k, str):
            return k
    return None


def kwargs_conditioning(unet, model, model_kwargs, device):
    """The Conditioning a ``model_kwargs`` dict spells for a UNetModel denoiser, or None where it holds at most ``c_concat`` (the
    callers' own path).  Two spellings: UNetModel.forward's keywords ``context=`` / ``y=`` (beside ``c_concat``), for the bare
    network, and the wrapper's ``c_crossattn`` / ``c_adm`` under its conditioning_key."""
    kw = dict(model_kwargs or {})
    if "context" in kw or "y" in kw:
        extra = set(kw) - {"c_concat", "context", "y"}
        if extra:
            raise ValueError(f"model_kwargs {sorted(extra)} beside context= / y= cannot reach the UNetModel")
        cc = kw.get("c_concat")
        cc = [cc] if torch.is_tensor(cc) else cc
        mv = lambda t: None if t is None else t.to(device)
        return Conditioning(torch.cat([t.to(device) for t in cc], 1) if cc else None, mv(kw.get("context")), mv(kw.get("y")))
    if "c_crossattn" in kw or "c_adm" in kw:
        return cat_conditioning(kw, device, wrapper_key(model))
    return None


def concat_of(cond, x: torch.Tensor) -> torch.Tensor:
    """The 'concat' tensor of a loop's conditioning (a tensor, or a Conditioning whose concat part may be absent: [B,0,H,W])."""
    if isinstance(cond, Conditioning):
        return cond.concat if cond.concat is not None else x.new_zeros((x.shape[0], 0) + tuple(x.shape[2:]))
    return cond


@contextlib.contextmanager
def conditioning_set(unet, cond, uncond=None):
    """dsd_set_conditioning around a latent device loop: installs the context / y of ``cond`` (and their unconditional twins of
    ``uncond``) on the denoiser's handle and clears them afterwards, whatever the loop did.  A tensor ``cond`` installs nothing."""
    if not isinstance(cond, Conditioning) or (cond.context is None and cond.y is None):
        yield
        return
    from .ldm.modules.diffusionmodules.openaimodel import UNetModel
    if not isinstance(unet, UNetModel):
        raise ValueError("'c_crossattn' / 'c_adm' conditioning needs a UNetModel denoiser: the DiT and the four-stream model take "
                         "'concat' conditioning only")
    u = uncond if isinstance(uncond, Conditioning) else Conditioning()
    keep = []

    def ctx(t):
        if t is None:
            return None
        t = t.detach().float().contiguous()
        keep.append(t)
        return t.data_ptr()

    def lab(t):
        if t is None:
            return None
        t = unet.label_input(t.detach(), cond.y.device)
        keep.append(t)
        return t.data_ptr()

    c = DsdConditioning()
    if cond.context is not None:
        c.context, c.context_uncond, c.tokens = ctx(cond.context), ctx(u.context), int(cond.context.shape[1])
        c.B = int(cond.context.shape[0])
    if cond.y is not None:
        c.y, c.y_uncond = lab(cond.y), lab(u.y)
        c.y_width = 0 if unet.label_kind == 1 else int(unet.label_width)
        c.B = int(cond.y.shape[0])
    check(lib().dsd_set_conditioning(unet._h, C.byref(c)))
    try:
        yield
    finally:
        check(lib().dsd_set_conditioning(unet._h, None))


def find_unet(model):
    """Locate the native denoiser behind the object the reference passes as ``model``
    (DiffusionWrapper.diffusion_model, ddpm.py:1323; or the network itself): the four-stream DSUnetModel, or one of the two
    that read the state from their own input — the plain UNetModel that denoises VAE latents and the DiT the reference's
    trainer swaps in for the U-Net (the device loops read the kind off the handle)."""
    from .UNet_DS_Diff.DiT_models import DiT
    from .UNet_DS_Diff.model import DSUnetModel
    from .ldm.modules.diffusionmodules.openaimodel import UNetModel
    from .Disc_diff.guided_diffusion.unet import UNet_disc_Model
    kinds = (DSUnetModel, UNetModel, DiT, UNet_disc_Model)
    if isinstance(model, kinds):
        return model
    inner = getattr(model, "diffusion_model", None)
    if isinstance(inner, kinds):
        return inner
    inner = getattr(getattr(model, "model", None), "diffusion_model", None)
    if isinstance(inner, kinds):
        return inner
    return None


def loop_denoiser(model, model_kwargs=None):
    """find_unet for a sampler call that carries ``model_kwargs``: the denoiser the device loop may run, or None for the per-step
    path.  The device loops hand a DiT its input and t and nothing else, so a call whose ``model_kwargs`` hold anything beside
    ``c_concat`` — labels ``y``, DiT.forward's own ``cond`` — keeps the per-step path, where the network receives them as
    ``model(x, t, **model_kwargs)``."""
    unet = find_unet(model)
    if unet is not None and is_dit(unet) and set(model_kwargs or {}) - {"c_concat"}:
        return None
    if unet is not None and is_disc(unet) and disc_planes(model_kwargs) is not None:
        from .Disc_diff.guided_diffusion.unet import SuperResModelNew
        if unet is model and not isinstance(unet, SuperResModelNew):
            # the reference calls model(x_input, t, **model_kwargs): UNet_disc_Model.forward takes no keywords (unet.py:985)
            raise TypeError("UNet_disc_Model.forward() got an unexpected keyword argument 't1' (only SuperResModelNew takes and "
                            "ignores the t1 / t2 / dwi of model_kwargs)")
    return unet


def is_disc(unet) -> bool:
    """The four-stream DisC-Diff denoiser (UNet_disc_Model / SuperResModelNew): a one-channel state beside t1, t2, dwi."""
    from .Disc_diff.guided_diffusion.unet import UNet_disc_Model
    return isinstance(unet, UNet_disc_Model)


DISC_KEYS = ("t1", "t2", "dwi")


def disc_planes(model_kwargs, device=None):
    """[t1, t2, dwi] of a ``model_kwargs`` dict in the order p_mean_variance concatenates them behind x
    (Disc_diff/guided_diffusion/gaussian_diffusion.py:271-275), or None where ``t1`` is absent."""
    kw = model_kwargs or {}
    if kw.get("t1") is None:
        return None
    return [kw[k] if device is None else kw[k].to(device) for k in DISC_KEYS]


def model_output_of(out):
    """The tensor a sampler reads of what a network returned: the ninth element of UNet_disc_Model's 9-tuple
    (gaussian_diffusion.py:277-278), the first of any other tuple (DSUnetModel's (out, dict))."""
    if isinstance(out, tuple):
        return out[8] if len(out) == 9 else out[0]
    return out


def is_dit(unet) -> bool:
    from .UNet_DS_Diff.DiT_models import DiT
    return isinstance(unet, DiT)


def is_latent_denoiser(unet) -> bool:
    """True for the denoisers whose state is the first channels of their own input (multi-channel latent state): the plain
    UNetModel (DSD_BLOCK_UNET handle) and the DiT (DSD_BLOCK_DIT)."""
    from .ldm.modules.diffusionmodules.openaimodel import UNetModel
    return isinstance(unet, UNetModel) or is_dit(unet)


def dit_state_channels(in_channels: int, learn_sigma: bool, cond_channels: int):
    """(Cz, out_ch) of a DiT under a sampler: the state is what the 'concat' conditioning leaves of the input, Cz = in_channels -
    Cc, and the output has in_channels // 3 * 2 channels with learn_sigma (DiT_models.py:163, sic), else in_channels.  The
    samplers read the prediction from the first Cz of them and a learned variance from the next Cz, so out_ch must be Cz or
    2*Cz: 4 input channels with 3 of conditioning (the shipped yaml) give (1, 2), 6 with 4 give (2, 4), 5 with 4 give (1, 2),
    3 unconditional without learn_sigma give (3, 3)."""
    in_channels, cond_channels = int(in_channels), int(cond_channels)
    out_ch = in_channels // 3 * 2 if learn_sigma else in_channels
    cz = in_channels - cond_channels
    if cond_channels < 0 or cz < 1:
        raise ValueError(f"a DiT of {in_channels} input channels leaves no state beside {cond_channels} conditioning channels")
    if out_ch not in (cz, 2 * cz):
        raise ValueError(f"a DiT of {in_channels} input channels (learn_sigma={bool(learn_sigma)}) has {out_ch} output channels; "
                         f"with {cond_channels} conditioning channels the state has {cz}, which needs {cz} or {2 * cz}")
    return cz, out_ch


def check_latent_io(unet, x: torch.Tensor, cond) -> None:
    """Shape checks of the latent loops that the C entry points cannot see (they take one H, W), and the parts of a Conditioning
    against what the network can take, each named by its key, before any device work."""
    bundle = cond if isinstance(cond, Conditioning) else Conditioning()
    cond = concat_of(cond, x)
    if is_dit(unet):
        if bundle.context is not None or bundle.y is not None:
            raise ValueError("the DiT takes 'concat' conditioning only in the device loops: 'c_crossattn' / 'c_adm' cannot reach it")
        if cond.dim() != 4 or cond.shape[0] != x.shape[0] or tuple(cond.shape[2:]) != tuple(x.shape[2:]):
            raise ValueError(f"conditioning {tuple(cond.shape)} does not match the state {tuple(x.shape)} "
                             "(same batch and spatial size needed for the 'concat' conditioning)")
        if tuple(x.shape[2:]) != (unet.input_size, unet.input_size):
            raise ValueError(f"the DiT takes {unet.input_size}x{unet.input_size} inputs (input_size) but the state is "
                             f"{tuple(x.shape)}")
        cz, _ = dit_state_channels(unet.in_channels, unet.learn_sigma, cond.shape[1])
        if cz != x.shape[1]:
            raise ValueError(f"the DiT takes {unet.in_channels} input channels but state + conditioning have {x.shape[1]} + "
                             f"{cond.shape[1]}")
        return
    B = x.shape[0]
    if unet.use_spatial_transformer:
        ctx = bundle.context
        if ctx is None:
            raise ValueError("this UNetModel has a spatial transformer: the conditioning needs 'c_crossattn' (a context)")
        if ctx.dim() != 3 or ctx.shape[0] != B or ctx.shape[2] != unet.context_dim:
            raise ValueError(f"'c_crossattn' must be [B, tokens, context_dim] = [{B}, tokens, {unet.context_dim}], got {tuple(ctx.shape)}")
    elif bundle.context is not None:
        raise ValueError("'c_crossattn' given but this UNetModel has no spatial transformer (use_spatial_transformer=False)")
    if unet.num_classes is not None:
        if bundle.y is None:
            raise ValueError(f"this UNetModel has a label_emb (num_classes={unet.num_classes!r}): the conditioning needs 'c_adm' "
                             "('c_crossattn' under the key 'adm')")
        if bundle.y.shape[0] != B:
            raise ValueError(f"'c_adm' has {bundle.y.shape[0]} rows but the state has {B}")
        unet.label_input(bundle.y, bundle.y.device)
    elif bundle.y is not None:
        raise ValueError("'c_adm' given but this UNetModel has no label_emb (num_classes is None)")
    if cond.dim() != 4 or cond.shape[0] != x.shape[0] or tuple(cond.shape[2:]) != tuple(x.shape[2:]):
        raise ValueError(f"conditioning {tuple(cond.shape)} does not match the latent state {tuple(x.shape)} "
                         "(same batch and spatial size needed for the 'concat' conditioning)")


def _seed_from_torch() -> int:
    """Philox seed drawn from torch's CPU generator so torch.manual_seed() makes sampling reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def philox_seed(seed: Optional[int] = None) -> int:
    """``seed`` itself, or one drawn from torch's generator when none is given."""
    return int(seed) if seed is not None else _seed_from_torch()


def _ref(struct):
    """byref of a bound guidance / inpaint struct, or None (NULL: unguided / unmasked)."""
    return C.byref(struct) if struct is not None else None


def _check_four_stream_io(unet, x: torch.Tensor, cond: torch.Tensor) -> None:
    """The four-stream model denoises a one-channel image beside 'concat' planes of its size (the library checks the latent
    denoisers' shapes against their handles)."""
    if not is_latent_denoiser(unet):
        assert x.shape[1] == 1 and cond.shape[0] == x.shape[0] and cond.shape[2:] == x.shape[2:]


def _loop_inputs(unet, x_T: torch.Tensor, cond: torch.Tensor, steps: int, guidance: Optional[Guidance],
                 inpaint: Optional[Inpaint], cpu_message: str):
    """The prologue every device loop shares: the guidance / inpaint checks, the denoiser and device tests, parameters synced,
    the state cloned.  ``cond``: the 'concat' tensor or a Conditioning.  Returns (x, the 'concat' tensor, bound guidance or None,
    bound inpaint or None, the context manager that holds the rest of the conditioning on the handle)."""
    if guidance is not None:
        guidance.check(cond, steps)
    if inpaint is not None:
        inpaint.check(x_T, steps)
    if unet is None:
        raise RuntimeError("no native denoiser (DSUnetModel / UNetModel / DiT) behind the model handed to the sampler")
    if not x_T.is_cuda:
        raise RuntimeError(cpu_message)
    unet.sync_params()
    x = x_T.detach().float().contiguous().clone()
    if is_latent_denoiser(unet):
        check_latent_io(unet, x, cond)
    elif isinstance(cond, Conditioning):
        raise ValueError("the four-stream model takes 'concat' conditioning only: 'c_crossattn' / 'c_adm' cannot reach it")
    held = conditioning_set(unet, cond, guidance.uncond if guidance is not None else None)
    cond = concat_of(cond, x).detach().float().contiguous()
    g = guidance.bind() if guidance is not None else None
    inp = inpaint.bind() if inpaint is not None else None
    return x, cond, g, inp, held


def kept_iterations(total_steps: int, log_every_t: int) -> list:
    """The loop iterations k (0 = the first executed, largest t) whose result the reference's samplers append to their
    intermediates: ``index % log_every_t == 0 or index == total_steps - 1`` with index = total_steps - 1 - k (ddim.py:157,181;
    plms.py likewise; ddpm.py:1041,1089 and trainer_ddpm.py:455 with index = the timestep i)."""
    total_steps, log_every_t = int(total_steps), int(log_every_t)
    return [k for k in range(total_steps) if (total_steps - 1 - k) % log_every_t == 0 or k == 0]


class Trace:
    """The intermediates of a device loop (dsd_set_trace): ``keep`` = ascending loop iterations, ``x`` / ``pred_x0`` = which of the
    two buffers are wanted.  After the loop ``states`` / ``pred_x0s`` are lists of per-entry [B,Cz,H,W] tensors, one per kept
    iteration the call's window covered (views of one [n_keep,B,Cz,H,W] buffer each)."""

    def __init__(self, keep: Sequence[int], x: bool = True, pred_x0: bool = True):
        self.keep = [int(k) for k in keep]
        self.want_x, self.want_x0 = bool(x), bool(pred_x0)
        self.x = self.pred_x0 = None
        self.states, self.pred_x0s = [], []

    def alloc(self, like: torch.Tensor) -> None:
        """The two buffers for a state like ``like``; kept when they are there already, so the calls of a split run fill one pair."""
        shape = (max(len(self.keep), 1),) + tuple(like.shape)
        have = self.x if self.x is not None else self.pred_x0
        if have is not None and tuple(have.shape) == shape and have.device == like.device:
            return
        new = lambda want: torch.zeros(shape, device=like.device, dtype=torch.float32) if want else None
        self.x, self.pred_x0 = new(self.want_x), new(self.want_x0)

    def collect(self, k0: int, k1: int) -> None:
        js = [j for j, k in enumerate(self.keep) if k0 <= k < k1]
        self.states = [self.x[j] for j in js] if self.x is not None else []
        self.pred_x0s = [self.pred_x0[j] for j in js] if self.pred_x0 is not None else []


@contextlib.contextmanager
def trace_set(unet, keep: Sequence[int], x: Optional[torch.Tensor], pred_x0: Optional[torch.Tensor]):
    """dsd_set_trace around one or more loop calls on the denoiser's handle: installs (keep, x, pred_x0) — the two tensors are
    [len(keep),B,Cz,H,W] device buffers or None — and always clears it afterwards, whatever the loop did."""
    keep_arr = np.ascontiguousarray(keep, dtype=np.int32).reshape(-1)
    t = DsdTrace()
    t.keep = keep_arr.ctypes.data_as(C.POINTER(C.c_int32))
    t.n_keep = int(keep_arr.shape[0])
    t.x = x.data_ptr() if x is not None else None
    t.pred_x0 = pred_x0.data_ptr() if pred_x0 is not None else None
    check(lib().dsd_set_trace(unet._h, C.byref(t)))
    try:
        yield
    finally:
        check(lib().dsd_set_trace(unet._h, None))


class StepCallbacks:
    """The reference's per-step ``callback(i)`` and ``img_callback(image, i)``, called in that order after every iteration.
    ``index``: iteration k -> the ``i`` the reference passes (DDIM / PLMS: k itself, ddim.py:178-179; the DDPM loops: the timestep
    steps - 1 - k, ddpm.py:1091-1092).  ``image``: "pred_x0" (DDIM, PLMS) or "x" (the DDPM loops: the state, after the blend)."""

    def __init__(self, callback=None, img_callback=None, index=None, image: str = "pred_x0"):
        assert image in ("pred_x0", "x")
        self.callback, self.img_callback, self.index, self.image = callback, img_callback, index or (lambda k: k), image

    def __bool__(self):
        return self.callback is not None or self.img_callback is not None

    @property
    def needs_x0(self) -> bool:
        return self.img_callback is not None and self.image == "pred_x0"

    def after(self, k: int, x: torch.Tensor, pred_x0: Optional[torch.Tensor]) -> None:
        i = self.index(k)
        if self.callback:
            self.callback(i)
        if self.img_callback:
            self.img_callback((pred_x0 if self.image == "pred_x0" else x).clone(), i)


def _run_traced(unet, call, x: torch.Tensor, steps: int, first_step: int, n_steps: int, trace: Optional[Trace],
                callbacks: Optional[StepCallbacks]) -> None:
    """``call(first_step, n_steps)`` runs iterations of a device loop in place on ``x``.  Plain: one call.  With ``trace``: the
    same call with the trace installed.  With ``callbacks``: single-step segments (n_steps = 1; the loops' state between them is
    ``x``, PLMS's history stays on the handle), each with a one-entry trace pointing at the slots of ``trace`` where the iteration
    is kept, and the callbacks after each.  Every route returns the same bits."""
    k0 = max(int(first_step), 0)
    k1 = steps if n_steps <= 0 else min(steps, k0 + int(n_steps))
    if trace is not None:
        trace.alloc(x)
    if not callbacks:
        if trace is None or not trace.keep:
            call(first_step, n_steps)
        else:
            with trace_set(unet, trace.keep, trace.x, trace.pred_x0):
                call(first_step, n_steps)
    else:
        slot = {k: j for j, k in enumerate(trace.keep)} if trace is not None else {}
        scratch = torch.empty_like(x) if callbacks.needs_x0 else None
        for k in range(k0, k1):
            j = slot.get(k)
            tx = trace.x[j] if j is not None and trace.x is not None else None
            t0 = trace.pred_x0[j] if j is not None and trace.pred_x0 is not None else scratch
            if tx is None and t0 is None:
                call(k, 1)
            else:
                with trace_set(unet, [k], tx, t0):
                    call(k, 1)
            callbacks.after(k, x, t0)
    if trace is not None:
        trace.collect(k0, k1)


@torch.no_grad()
def run_device_loop(unet, sched: Schedule, x_T: torch.Tensor, cond: torch.Tensor,
                    step_noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                    first_step: int = 0, n_steps: int = 0, guidance: Optional[Guidance] = None,
                    inpaint: Optional[Inpaint] = None, trace: Optional[Trace] = None,
                    callbacks: Optional[StepCallbacks] = None) -> torch.Tensor:
    """dsd_sample.  x_T [B,1,H,W], cond [B,Cc,H,W] (CUDA fp32).  Returns x after the selected iterations.
    With the plain UNetModel or the DiT the state is a latent x_T [B,Cz,H,W]; step_noise is [steps,B,Cz,H,W].
    ``guidance``: classifier-free guidance (mode B_DDIM); its unconditional conditioning must have the shape, dtype and device
    of ``cond``.  ``inpaint``: masked sampling (modes B_DDIM and B_DDPM), guided or not.  ``trace``: the intermediates
    (dsd_set_trace), filled in place; ``callbacks``: the reference's per-step callbacks, which cut the run into single-step
    calls.  Neither changes a bit of the returned sample."""
    x, cond, g, inp, held = _loop_inputs(unet, x_T, cond, sched.steps, guidance, inpaint,
                                         "sampling runs on the MI355X only (no CPU fallback): x_T is on the CPU")
    B, Cz, H, W = x.shape
    _check_four_stream_io(unet, x, cond)
    if step_noise is not None:
        step_noise = step_noise.detach().float().contiguous()
        if tuple(step_noise.shape) != (sched.steps, B, Cz, H, W):
            raise ValueError(f"step_noise must be [steps,B,Cz,H,W] = {(sched.steps, B, Cz, H, W)}, got {tuple(step_noise.shape)}")
    seed = C.c_uint64(philox_seed(seed))

    def call(first, n):
        check(lib().dsd_sample(unet._h, C.byref(sched.c), _ref(g), _ref(inp), dptr(cond), cond.shape[1], dptr(x), Cz,
                               dptr(step_noise), seed, B, H, W, first, n, stream_ptr()))

    with held:
        _run_traced(unet, call, x, sched.steps, first_step, n_steps, trace, callbacks)
    return x


@torch.no_grad()
def run_plms_loop(unet, sched: Schedule, x_T: torch.Tensor, cond: torch.Tensor, threshold: Optional[float] = None,
                  guidance: Optional[Guidance] = None, inpaint: Optional[Inpaint] = None, seed: Optional[int] = None,
                  first_step: int = 0, n_steps: int = 0, trace: Optional[Trace] = None,
                  callbacks: Optional[StepCallbacks] = None) -> torch.Tensor:
    """The PLMS device loop (dsd_sample_plms) on a DSD_MODE_B_PLMS schedule: x_T [B,1,H,W] with the four-stream model,
    [B,Cz,H,W] with the plain UNetModel.  ``threshold``: dynamic_threshold of norm_thresholding (None / <= 0:
    off).  The history of noise predictions stays on the denoiser's handle: ``first_step`` = k > 0 continues the run whose
    iterations 0 .. k-1 ran last on it (x_T = the state they returned) and fails otherwise.  ``seed`` keys the blend noise of
    ``inpaint`` when it carries none; PLMS itself draws no noise.  ``trace`` / ``callbacks``: as in run_device_loop."""
    x, cond, g, inp, held = _loop_inputs(unet, x_T, cond, sched.steps, guidance, inpaint,
                                         "sampling runs on the MI355X only (no CPU fallback): x_T is on the CPU")
    thr = C.c_float(float(threshold) if threshold is not None else 0.0)
    seed = C.c_uint64(philox_seed(seed) if inp is not None and inp.noise is None else 0)
    B, Cz, H, W = x.shape
    _check_four_stream_io(unet, x, cond)

    def call(first, n):
        check(lib().dsd_sample_plms(unet._h, C.byref(sched.c), _ref(g), _ref(inp), thr, dptr(cond), cond.shape[1], dptr(x), Cz, seed,
                                    B, H, W, first, n, stream_ptr()))

    with held:
        _run_traced(unet, call, x, sched.steps, first_step, n_steps, trace, callbacks)
    return x


@torch.no_grad()
def plms_step(order: int, a_t: float, a_prev: float, sqrt_1m_at: float, out_cond: torch.Tensor, h_new: torch.Tensor,
              x: torch.Tensor, o1: Optional[torch.Tensor] = None, o2: Optional[torch.Tensor] = None,
              x_saved: Optional[torch.Tensor] = None, out_uncond: Optional[torch.Tensor] = None, scale: float = 1.0,
              threshold: Optional[float] = None, state_channels: Optional[int] = None) -> None:
    """One PLMS update (dsd_op_plms_step; _lib.PLMS_PREDICT / PLMS_CORRECT / PLMS_AB2..4), x and the history updated in place.
    ``h_new`` / ``o1`` / ``o2`` / ``x_saved`` are contiguous [B,Cz,H,W] planes; ``x`` is [B,Cz,H,W] (2B rows with ``out_uncond``),
    or a [rows,Cz+Cc,H,W] denoiser input with ``state_channels`` = Cz."""
    B, Cz, H, W = out_cond.shape
    cz, stride = _rows(x, state_channels)
    assert cz == Cz and x.shape[0] == (2 * B if out_uncond is not None else B) and tuple(x.shape[2:]) == (H, W)
    for t in (h_new, o1, o2, x_saved):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (B, Cz, H, W))
    ou, oc = _f32c(out_uncond), _f32c(out_cond)
    check(lib().dsd_op_plms_step(int(order), float(a_t), float(a_prev), float(sqrt_1m_at), dptr(ou),
                                 dptr(oc), float(scale), dptr(h_new), dptr(o1), dptr(o2), dptr(x_saved),
                                 dptr(x), stride, float(threshold) if threshold is not None else 0.0, B, Cz, H, W, stream_ptr()))


@torch.no_grad()
def sampler_update(sched: Schedule, k: int, model_out: torch.Tensor, x: torch.Tensor,
                   noise: Optional[torch.Tensor], seed: int = 0, want_x0: bool = False):
    """One fused update (dsd_op_sampler_update); x is updated in place."""
    B, Cx, H, W = x.shape
    if not sched.c.learned_range and model_out.shape[1] == 2 * Cx:
        model_out = model_out[:, :Cx]          # a variance half the schedule does not use (gaussian_diffusion.py:484-485)
    if Cx > 1:
        # multi-channel states (latents): the update is elementwise, so [B,C,H,W] is B*C one-channel images.  With a
        # learned-range variance a sample's output is [mean(Cx), variance(Cx)] planes, which is the one-channel layout of a
        # (Cx*H) x W image: element (b, c, p) keeps its variance partner and its Philox counter b*Cx*H*W + c*H*W + p
        if sched.c.learned_range:
            H = Cx * H
        else:
            B = B * Cx
    x0 = torch.empty_like(x) if want_x0 else None
    mo, z = _f32c(model_out), _f32c(noise)
    check(lib().dsd_op_sampler_update(C.byref(sched.c), k, dptr(mo), dptr(x), dptr(z), C.c_uint64(seed), B, H, W, dptr(x0),
                                      stream_ptr()))
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
    ou, oc, z = _f32c(out_uncond), _f32c(out_cond), _f32c(noise)
    check(lib().dsd_op_sampler_update_guided(C.byref(sched.c), k, dptr(ou), dptr(oc), float(scale), dptr(x2), x2.shape[1] * H * W,
                                             dptr(z), C.c_uint64(seed), B, Cz, H, W, dptr(x0), stream_ptr()))
    return x0


def invert_coefficients(alphas_next: torch.Tensor, alphas: torch.Tensor) -> np.ndarray:
    """[steps,2] fp32 (cx, ce) of DDIMSampler.encode's update (ddim.py:292-295), formed with the reference's own torch
    expressions on 0-d tensors of the reference's dtypes and rounded to fp32 once — where a 0-d tensor meets the fp32 state.
    ``alphas_next`` is fp32; ``alphas`` is float64 for the DDIM sub-schedule (torch.tensor of a numpy float64 array, :276), so
    there the scalar arithmetic is float64; with use_original_steps both are fp32 buffers."""
    n = int(alphas_next.shape[0])
    coef = np.zeros((n, 2), dtype=np.float32)
    for i in range(n):
        cx = (alphas_next[i] / alphas[i]).sqrt()
        ce = alphas_next[i].sqrt() * ((1 / alphas_next[i] - 1).sqrt() - (1 / alphas[i] - 1).sqrt())
        coef[i, 0], coef[i, 1] = float(cx.to(torch.float32)), float(ce.to(torch.float32))
    return coef


@torch.no_grad()
def run_invert_loop(unet, coef: np.ndarray, x0: torch.Tensor, cond: torch.Tensor, guidance: Optional[Guidance] = None,
                    first_step: int = 0, n_steps: int = 0) -> torch.Tensor:
    """DDIM inversion on the device (dsd_invert): ``coef`` [steps,2] from invert_coefficients.  The model time of iteration i
    is the loop index i itself — DDIMSampler.encode passes ``i``, not a timestep of the schedule
    (ddim.py:282); a quirk of the reference, kept for parity."""
    coef = np.ascontiguousarray(coef, dtype=np.float32)
    steps = int(coef.shape[0])
    assert coef.shape == (steps, 2)
    x, cond, g, _, held = _loop_inputs(unet, x0, cond, steps, guidance, None,
                                       "DDIM inversion runs on the MI355X only (no CPU fallback): x0 is on the CPU")
    t_model = np.arange(steps, dtype=np.float32)
    sc = DsdInvertSchedule()
    sc.steps = steps
    sc.coef = coef.ctypes.data_as(C.POINTER(C.c_float))
    sc.t_model = t_model.ctypes.data_as(C.POINTER(C.c_float))
    B, Cz, H, W = x.shape
    _check_four_stream_io(unet, x, cond)
    with held:
        check(lib().dsd_invert(unet._h, C.byref(sc), _ref(g), dptr(cond), cond.shape[1], dptr(x), Cz, B, H, W, first_step, n_steps,
                               stream_ptr()))
    return x


@torch.no_grad()
def run_bpd_loop(unet, sched: Schedule, post_log_var: np.ndarray, prior_log_var: float, x_start: torch.Tensor, cond: torch.Tensor,
                 step_noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, first_step: int = 0, n_steps: int = 0,
                 out: Optional[dict] = None) -> dict:
    """The variational-bound device loop (dsd_calc_bpd) on a DSD_MODE_A_DDPM schedule: x_start [B,1,H,W] with the
    four-stream model, [B,Cz,H,W] with the UNetModel or the DiT; read only.  ``post_log_var`` [steps]: the fp32
    posterior_log_variance_clipped in iteration order; ``prior_log_var``: log(1 - alphas_cumprod[T-1]).  ``step_noise``
    [steps,B,Cz,H,W] feeds q_sample's normals, else Philox stream (seed, k + 2^32).  Returns {"vb", "xstart_mse", "mse"} [B,steps]
    (column k = iteration k) and {"prior_bpd"} [B]; ``out`` (a dict this function returned) is written in place, so a split run
    fills its columns call by call."""
    if unet is None:
        raise RuntimeError("no native denoiser (DSUnetModel / UNetModel / DiT) behind the model handed to the bound")
    if not x_start.is_cuda:
        raise RuntimeError("the variational bound runs on the MI355X only (no CPU fallback): x_start is on the CPU")
    unet.sync_params()
    xs = x_start.detach().float().contiguous()
    bundle = cond
    if is_latent_denoiser(unet):
        check_latent_io(unet, xs, bundle)
    elif isinstance(bundle, Conditioning):
        raise ValueError("the four-stream model takes 'concat' conditioning only: 'c_crossattn' / 'c_adm' cannot reach it")
    cond = concat_of(bundle, xs).detach().float().contiguous()
    post_log_var = np.ascontiguousarray(post_log_var, dtype=np.float32)
    assert post_log_var.shape == (sched.steps,)
    B, Cz, H, W = xs.shape
    if step_noise is not None:
        step_noise = step_noise.detach().float().contiguous()
        if tuple(step_noise.shape) != (sched.steps, B, Cz, H, W):
            raise ValueError(f"step_noise must be [steps,B,C,H,W] = {(sched.steps, B, Cz, H, W)}, got {tuple(step_noise.shape)}")
    seed = philox_seed(seed)
    if out is None:
        out = {k: torch.zeros((B, sched.steps), device=xs.device, dtype=torch.float32) for k in ("vb", "xstart_mse", "mse")}
        out["prior_bpd"] = torch.zeros((B,), device=xs.device, dtype=torch.float32)
    bpd = DsdBpd()
    bpd.post_log_var = post_log_var.ctypes.data_as(C.POINTER(C.c_float))
    bpd.vb, bpd.xstart_mse, bpd.mse = out["vb"].data_ptr(), out["xstart_mse"].data_ptr(), out["mse"].data_ptr()
    bpd.prior, bpd.prior_log_var = out["prior_bpd"].data_ptr(), float(prior_log_var)
    _check_four_stream_io(unet, xs, cond)
    with conditioning_set(unet, bundle):
        check(lib().dsd_calc_bpd(unet._h, C.byref(sched.c), C.byref(bpd), dptr(cond), cond.shape[1], dptr(xs), Cz, dptr(step_noise),
                                 C.c_uint64(seed), B, H, W, first_step, n_steps, stream_ptr()))
    return out


@torch.no_grad()
def vlb_terms(sched: Schedule, k: int, post_log_var: float, model_out: torch.Tensor, x_t: torch.Tensor, x_start: torch.Tensor,
              noise: Optional[torch.Tensor], seed: int = 0, vb: Optional[torch.Tensor] = None,
              xstart_mse: Optional[torch.Tensor] = None, mse: Optional[torch.Tensor] = None, want_planes: bool = False,
              state_channels: Optional[int] = None):
    """The bound's terms of iteration k (dsd_op_vlb_terms).  ``vb`` / ``xstart_mse`` / ``mse``: fp32 views of B elements with one
    stride — a column of the [B,steps] results — written in place (None: not wanted).  ``x_t`` is [B,Cz,H,W], or a [B,Cz+Cc,H,W]
    denoiser input with ``state_channels`` = Cz; ``model_out`` [B,Cz,H,W], or [B,2Cz,H,W] where it carries a variance half.
    ``want_planes``: returns p_mean_variance's (mean, log_variance, pred_xstart)."""
    B, Cz, H, W = x_start.shape
    cz, x_stride = _rows(x_t, state_channels)
    assert cz == Cz and x_t.shape[0] == B and tuple(x_t.shape[2:]) == (H, W)
    mo, xs, z = _f32c(model_out), _f32c(x_start), _f32c(noise)
    assert mo.shape[0] == B and mo.shape[1] in (Cz, 2 * Cz) and tuple(mo.shape[2:]) == (H, W)
    if sched.c.learned_range and mo.shape[1] != 2 * Cz:
        raise ValueError(f"a learned-range variance needs {2 * Cz} output channels; the model output has {mo.shape[1]}")
    terms = [t for t in (vb, xstart_mse, mse) if t is not None]
    stride = 0
    for t in terms:
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 and t.shape[0] == B
        assert stride in (0, t.stride(0) or 1) or B == 1, "vb / xstart_mse / mse must share their stride"
        stride = t.stride(0) or 1
    planes = [torch.empty((B, Cz, H, W), device=xs.device, dtype=torch.float32) for _ in range(3)] if want_planes else [None] * 3
    tp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    check(lib().dsd_op_vlb_terms(C.byref(sched.c), int(k), float(post_log_var), dptr(mo), mo.shape[1] * H * W, dptr(x_t), x_stride,
                                 dptr(xs), dptr(z), C.c_uint64(seed), tp(vb), tp(xstart_mse), tp(mse), stride, dptr(planes[0]),
                                 dptr(planes[1]), dptr(planes[2]), B, Cz, H, W, stream_ptr()))
    return tuple(planes) if want_planes else None


@torch.no_grad()
def prior_bpd(sqrt_acp: float, log_1m_acp: float, x_start: torch.Tensor) -> torch.Tensor:
    """_prior_bpd (dsd_op_prior_bpd): [B] bits per dimension."""
    B, Cz, H, W = x_start.shape
    xs = _f32c(x_start)
    out = torch.empty((B,), device=xs.device, dtype=torch.float32)
    check(lib().dsd_op_prior_bpd(float(sqrt_acp), float(log_1m_acp), dptr(xs), dptr(out), B, Cz, H, W, stream_ptr()))
    return out


@torch.no_grad()
def ddim_reverse_step(sched: Schedule, k: int, alpha_bar_next: float, model_out: torch.Tensor, x: torch.Tensor,
                      want_x0: bool = False, state_channels: Optional[int] = None):
    """One step of the DDIM reverse ODE (dsd_op_ddim_reverse_step), x updated in place to x_{t+1}."""
    B, _, H, W = x.shape
    Cz, stride = _rows(x, state_channels)
    mo = _f32c(model_out)
    assert mo.shape[0] == B and mo.shape[1] >= Cz and tuple(mo.shape[2:]) == (H, W)
    x0 = torch.empty((B, Cz, H, W), device=x.device, dtype=torch.float32) if want_x0 else None
    check(lib().dsd_op_ddim_reverse_step(C.byref(sched.c), int(k), float(alpha_bar_next), dptr(mo), mo.shape[1] * H * W, dptr(x),
                                         stride, dptr(x0), B, Cz, H, W, stream_ptr()))
    return x0


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """``t`` as a contiguous fp32 tensor (None stays None).  The caller keeps the result in a local until its launch is queued:
    the copy a channel slice needs would otherwise be freed as soon as its pointer is taken, and the next copy could be handed
    the same memory — two arguments of one launch aliasing each other."""
    return None if t is None else t.float().contiguous()


def _rows(x: torch.Tensor, state_channels: Optional[int]):
    """(Cz, row stride) of a contiguous [rows,C,H,W] tensor whose first ``state_channels`` (default: all) channels are the state."""
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
    return int(state_channels or x.shape[1]), int(x.shape[1] * x.shape[2] * x.shape[3])


@torch.no_grad()
def mask_blend(a: float, s: float, x0: torch.Tensor, mask: torch.Tensor, x: torch.Tensor, noise: Optional[torch.Tensor],
               seed: int = 0, step: int = 0, guided: bool = False, state_channels: Optional[int] = None) -> None:
    """One blend (dsd_op_mask_blend), x updated in place: x = (a*x0 + s*z)*mask + (1 - mask)*x.  ``x`` is [B,Cz,H,W], or a
    [B,Cz+Cc,H,W] denoiser input with ``state_channels`` = Cz; ``guided``: 2B rows, row b read, rows b and B+b written."""
    B, Cz, H, W = x0.shape
    cz, stride = _rows(x, state_channels)
    assert cz == Cz and x.shape[0] == (2 * B if guided else B) and tuple(x.shape[2:]) == (H, W)
    x0c, mc, z = _f32c(x0), _f32c(mask), _f32c(noise)
    check(lib().dsd_op_mask_blend(float(a), float(s), dptr(x0c), dptr(mc), int(mask.shape[1]), dptr(x), stride, int(guided), dptr(z),
                                  C.c_uint64(seed), C.c_uint64(step), B, Cz, H, W, stream_ptr()))


@torch.no_grad()
def q_sample_rows(a: torch.Tensor, s: torch.Tensor, x0: torch.Tensor, noise: Optional[torch.Tensor], seed: int = 0,
                  step: int = 0) -> torch.Tensor:
    """a[b]*x0_b + s[b]*z_b (dsd_op_q_sample): a, s device fp32 [B] (coefficient tables gathered by t); z fed or Philox."""
    B, Cz, H, W = x0.shape
    out = torch.empty((B, Cz, H, W), device=x0.device, dtype=torch.float32)
    ac, sc, x0c, z = _f32c(a), _f32c(s), _f32c(x0), _f32c(noise)
    check(lib().dsd_op_q_sample(dptr(ac), dptr(sc), dptr(x0c), dptr(z), C.c_uint64(seed), C.c_uint64(step), dptr(out), 0, B, Cz, H,
                                W, stream_ptr()))
    return out


@torch.no_grad()
def ddim_invert_step(cx: float, ce: float, out_cond: torch.Tensor, x: torch.Tensor, out_uncond: Optional[torch.Tensor] = None,
                     scale: float = 1.0, state_channels: Optional[int] = None) -> None:
    """One inversion step (dsd_op_ddim_invert_step), x updated in place; with ``out_uncond`` the guided step on 2B rows."""
    B, Cz, H, W = out_cond.shape
    cz, stride = _rows(x, state_channels)
    assert cz == Cz and x.shape[0] == (2 * B if out_uncond is not None else B) and tuple(x.shape[2:]) == (H, W)
    ou, oc = _f32c(out_uncond), _f32c(out_cond)
    check(lib().dsd_op_ddim_invert_step(float(cx), float(ce), dptr(ou), dptr(oc), float(scale), dptr(x), stride, B, Cz, H, W,
                                        stream_ptr()))


# ------------------------------------------------------------------------------------------------ the denoising loss (loss.hip)
LOSS_KINDS = {"l2": 0, "l1": 1, "charbonnie": 2}     # DSD_LOSS_*; 'charbonnie' is the reference's spelling (ddpm.py:377)
LOSS_TERMS = ("mse", "vb", "com", "dist")            # the columns of dsd_eval_loss's [B, DSD_LOSS_NTERMS] result


def _loss_on_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"the denoising loss runs on the MI355X only (no CPU fallback): {what} is on the CPU")


def _row(t, device) -> torch.Tensor:
    """A per-sample row [B] as contiguous device fp32."""
    return torch.as_tensor(t).detach().to(device=device, dtype=torch.float32).contiguous()


@torch.no_grad()
def loss_rows(pred: int, kind: int, model_out: torch.Tensor, x_start: Optional[torch.Tensor], noise: Optional[torch.Tensor],
              a: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0) -> torch.Tensor:
    """[B] mean over C*H*W of kind(target - prediction) (dsd_op_loss_rows).  ``pred`` (PRED_*) names the target: the noise,
    x_start, or get_v's a[b]*noise - s[b]*x_start; ``kind``: LOSS_L2 / LOSS_L1 / LOSS_CHARBONNIER.  ``model_out`` is [B,C,H,W] or,
    with a variance half, [B,2C,H,W] (its first C channels are read in place).  ``noise`` None: the Philox normals q_sample_rows
    draws for the same (seed, step)."""
    ref = x_start if x_start is not None else noise
    _loss_on_gpu(model_out, "model_out")
    B, Cz, H, W = ref.shape
    mo, xs, z = _f32c(model_out), _f32c(x_start), _f32c(noise)
    assert mo.shape[0] == B and mo.shape[1] in (Cz, 2 * Cz) and tuple(mo.shape[2:]) == (H, W)
    ar, sr = (None, None) if a is None else (_row(a, mo.device), _row(s, mo.device))
    out = torch.empty((B,), device=mo.device, dtype=torch.float32)
    check(lib().dsd_op_loss_rows(int(pred), int(kind), dptr(mo), mo.shape[1] * H * W, dptr(xs), dptr(z), C.c_uint64(seed),
                                 C.c_uint64(step), dptr(ar), dptr(sr), dptr(out), 1, B, Cz, H, W, stream_ptr()))
    return out


@torch.no_grad()
def pair_mse_rows(feats: Sequence[torch.Tensor]) -> torch.Tensor:
    """[B]: the sum over the pairs of 2, 3 or 4 feature tensors [B,...] of mean_flat((f_i - f_j)^2), in the order of
    training_losses' com / dist terms (dsd_op_pair_mse_rows)."""
    fs = [_f32c(f) for f in feats]
    _loss_on_gpu(fs[0], "the features")
    B = fs[0].shape[0]
    n = fs[0].numel() // B
    assert all(f.shape == fs[0].shape for f in fs)
    ptrs = (C.c_void_p * len(fs))(*[f.data_ptr() for f in fs])
    out = torch.empty((B,), device=fs[0].device, dtype=torch.float32)
    check(lib().dsd_op_pair_mse_rows(ptrs, len(fs), B, n, dptr(out), stream_ptr()))
    return out


@torch.no_grad()
def vlb_terms_rows(pred: int, learned_range: bool, clip_denoised: bool, coef: torch.Tensor, post_log_var: torch.Tensor,
                   decoder: torch.Tensor, model_out: torch.Tensor, x_t: torch.Tensor, x_start: torch.Tensor,
                   noise: Optional[torch.Tensor], seed: int = 0, step: int = 0):
    """The bound's terms with a timestep per sample (dsd_op_vlb_terms_rows): ``coef`` [B,DSD_NCOEF] (the MODE_A_DDPM rows),
    ``post_log_var`` [B], ``decoder`` [B] (t == 0).  Returns (vb, xstart_mse, mse), [B] each."""
    _loss_on_gpu(model_out, "model_out")
    B, Cz, H, W = x_start.shape
    mo, xt, xs, z = _f32c(model_out), _f32c(x_t), _f32c(x_start), _f32c(noise)
    dev = mo.device
    cf, plv = _row(coef, dev), _row(post_log_var, dev)
    dec = torch.as_tensor(decoder).to(device=dev, dtype=torch.int32).contiguous()
    assert tuple(cf.shape) == (B, DSD_NCOEF) and tuple(plv.shape) == (B,) and tuple(dec.shape) == (B,)
    if learned_range and mo.shape[1] != 2 * Cz:
        raise ValueError(f"a learned-range variance needs {2 * Cz} output channels; the model output has {mo.shape[1]}")
    outs = torch.empty((3, B), device=dev, dtype=torch.float32)
    check(lib().dsd_op_vlb_terms_rows(int(pred), int(bool(learned_range)), int(bool(clip_denoised)), dptr(cf), dptr(plv), dptr(dec),
                                      dptr(mo), mo.shape[1] * H * W, dptr(xt), 0, dptr(xs), dptr(z), C.c_uint64(seed),
                                      C.c_uint64(step), dptr(outs[0]), dptr(outs[1]), dptr(outs[2]), 1, B, Cz, H, W, stream_ptr()))
    return outs[0], outs[1], outs[2]


@torch.no_grad()
def run_eval_loss(unet, pred: int, kind: int, x_start: torch.Tensor, cond, t_model, a, s, noise: Optional[torch.Tensor] = None,
                  seed: int = 0, step: int = 0, vlb=None, learned_range: bool = False, target: Optional[int] = None,
                  disentangle: Optional["Disentangle"] = None) -> dict:
    """dsd_eval_loss: q_sample with the rows ``a`` / ``s``, one evaluation of the native denoiser with ``t_model`` [B] as its
    timesteps, and the loss kernels.  ``pred``: what the network predicts; ``target`` (default: the same) the target of the mse
    term where the reference reads the two off different attributes.  ``cond``: the 'concat' tensor or a Conditioning, as in the loops.  ``vlb``: None, or
    (coef [B,DSD_NCOEF], post_log_var [B], decoder [B]) for the vb term.  Returns {"mse": [B]} plus "vb" (with ``vlb``) and
    "com" / "dist" (UNet_disc_Model), read back from one [B, LOSS_NTERMS] buffer.  ``disentangle``: a Disentangle installed as the
    call's rider (dsd_set_disentangle; DSUnetModel only), whose loss / logits buffers the same call fills."""
    from ._lib import DsdLoss, LOSS_NTERMS
    if unet is None:
        raise RuntimeError("no native denoiser (DSUnetModel / UNet_disc_Model / UNetModel / DiT) behind the model handed to the loss")
    _loss_on_gpu(x_start, "x_start")
    unet.sync_params()
    xs = x_start.detach().float().contiguous()
    dev = xs.device
    bundle = cond
    if is_latent_denoiser(unet):
        check_latent_io(unet, xs, bundle)
    elif isinstance(bundle, Conditioning):
        raise ValueError("the four-stream model takes 'concat' conditioning only: 'c_crossattn' / 'c_adm' cannot reach it")
    cond = concat_of(bundle, xs).detach().float().contiguous()
    B, Cz, H, W = xs.shape
    z = _f32c(noise)
    if z is not None and tuple(z.shape) != (B, Cz, H, W):
        raise ValueError(f"noise must have the shape of x_start {(B, Cz, H, W)}, got {tuple(z.shape)}")
    rows = [_row(r, dev) for r in (t_model, a, s)]
    for r in rows:
        if tuple(r.shape) != (B,):
            raise ValueError(f"t / a / s must be [B] = [{B}], got {tuple(r.shape)}")
    terms = torch.zeros((B, LOSS_NTERMS), device=dev, dtype=torch.float32)
    spec = DsdLoss()
    spec.target, spec.pred = int(pred if target is None else target), int(pred)
    spec.kind, spec.learned_range = int(kind), int(bool(learned_range))
    spec.t_model, spec.a, spec.s = (r.data_ptr() for r in rows)
    held = []
    if vlb is not None:
        cf, plv = _row(vlb[0], dev), _row(vlb[1], dev)
        dec = torch.as_tensor(vlb[2]).to(device=dev, dtype=torch.int32).contiguous()
        assert tuple(cf.shape) == (B, DSD_NCOEF) and tuple(plv.shape) == (B,) and tuple(dec.shape) == (B,)
        held = [cf, plv, dec]
        spec.vlb_coef, spec.post_log_var, spec.decoder = cf.data_ptr(), plv.data_ptr(), dec.data_ptr()
    spec.terms = terms.data_ptr()
    _check_four_stream_io(unet, xs, cond)
    with conditioning_set(unet, bundle), disentangle_set(unet, disentangle):
        check(lib().dsd_eval_loss(unet._h, C.byref(spec), dptr(cond), cond.shape[1], dptr(xs), Cz, dptr(z), C.c_uint64(seed),
                                  C.c_uint64(step), B, H, W, stream_ptr()))
    del held
    out = {"mse": terms[:, 0]}
    if vlb is not None:
        out["vb"] = terms[:, 1]
    if is_disc(unet):
        out["com"], out["dist"] = terms[:, 2], terms[:, 3]
    return out


# ------------------------------------------------------------------------------------- the disentanglement losses (contrast.hip)
# get_disentangle_loss's spellings (training_project/utils/gaussian_diffusion.py:1056-1094) and the op's own
CONTRAST_MODES = {"contrast": _lib.CONTRAST_CL, "cl": _lib.CONTRAST_CL, "eu": _lib.CONTRAST_EU, "eu&contrast": _lib.CONTRAST_EU_CL,
                  "eu&cl": _lib.CONTRAST_EU_CL, "l1": _lib.CONTRAST_L1}
DISENTANGLE_MODES = ("contrast", "eu", "eu&contrast")     # what training_losses(disentangle=) takes
HEAD_VIEWS = dict(content=3, style=3, anatomy=2, lesion=2)  # DSUnetModel's head tensors (model.py:695-725)


def disentangle_labels(B: int, n_content: int = 3, n_style: int = 3, n_anatomy: int = 2, n_lesion: int = 2):
    """The two label tensors of training_losses(disentangle=) (:932-951), int64 on the CPU: c_s [B, n_content + n_style] with
    row b = [b]*n_content + [-1, -2, ...], s_a_l [B, n_style + n_anatomy + n_lesion] with row b = [-1, -2, ...] +
    [2b]*n_anatomy + [2b+1]*n_lesion."""
    style = [-1 - j for j in range(n_style)]
    c_s = torch.tensor([[b] * n_content + style for b in range(B)], dtype=torch.int64).reshape(B, n_content + n_style)
    s_a_l = torch.tensor([style + [2 * b] * n_anatomy + [2 * b + 1] * n_lesion for b in range(B)],
                         dtype=torch.int64).reshape(B, n_style + n_anatomy + n_lesion)
    return c_s, s_a_l


def label_rows(label: torch.Tensor) -> torch.Tensor:
    """[B, n_views] labels in the row order of the features, torch.cat(torch.unbind(label, 1), 0): row view*B + b."""
    return torch.cat(torch.unbind(label, dim=1), dim=0).contiguous().view(-1)


def perfect_logit(rows: torch.Tensor) -> torch.Tensor:
    """2*mask - 1 of a [R] label row (:1068-1070; contrastive_loss.py:81 writes the same matrix with torch.where)."""
    r = rows.view(-1, 1)
    return 2 * torch.eq(r, r.T).float() - 1


@torch.no_grad()
def contrast_rows(views: Sequence[torch.Tensor], labels: torch.Tensor, metric: str = "eu", temperature: float = 0.1):
    """(loss, logits [R,R]) of dsd_op_contrast_rows over ``views``, n_views CUDA tensors [B, ...] of one shape whose samples are
    the R = n_views*B rows view*B + b, and ``labels`` [R] in that order.  ``metric``: "cl" / "contrast" (supervised contrastive
    on cosine / temperature), "eu" (distance ratio on the fp64 Euclidean distance / n), "eu&cl" / "eu&contrast" (eu + 0.05 cl,
    the cosine logits returned) or "l1" (the eu ratio on the L1 distance / n: the ``contrast=False`` variant of
    trainers/trainer_ds_diff.py:341-354).  Views that share one row stride (slices of a stacked [B, n_views, ...] tensor) are
    read in place."""
    if metric not in CONTRAST_MODES:
        raise NotImplementedError(f"contrast {metric} not supported")
    if len(views) < 1 or len(views) > _lib.CONTRAST_MAX_VIEWS:
        raise ValueError(f"1 to {_lib.CONTRAST_MAX_VIEWS} views are taken, got {len(views)}")
    _loss_on_gpu(views[0], "the features")
    B = int(views[0].shape[0])
    if any(v.shape != views[0].shape for v in views):
        raise ValueError("the views differ in shape: " + ", ".join(str(tuple(v.shape)) for v in views))
    vs = [v.detach().reshape(B, -1) for v in views]
    n = int(vs[0].shape[1])
    inplace = all(v.dtype == torch.float32 and (n == 1 or v.stride(1) == 1) and v.stride(0) == vs[0].stride(0) and v.stride(0) >= n
                  for v in vs)
    if not inplace:
        vs = [v.float().contiguous() for v in vs]
    R = B * len(vs)
    if R < 2 or R > _lib.CONTRAST_MAX_ROWS:
        raise ValueError(f"{len(vs)} views of {B} samples are {R} rows; 2 to {_lib.CONTRAST_MAX_ROWS} are taken")
    lab = torch.as_tensor(labels).detach().reshape(-1).to(device=vs[0].device, dtype=torch.int32).contiguous()
    if lab.numel() != R:
        raise ValueError(f"{lab.numel()} labels for {R} rows")
    loss = torch.zeros((1,), device=vs[0].device, dtype=torch.float32)
    logits = torch.empty((R, R), device=vs[0].device, dtype=torch.float32)
    ptrs = (C.c_void_p * len(vs))(*[v.data_ptr() for v in vs])
    check(lib().dsd_op_contrast_rows(ptrs, len(vs), B, n, int(vs[0].stride(0)) if inplace else n, C.c_void_p(lab.data_ptr()),
                                     CONTRAST_MODES[metric], C.c_float(float(temperature)), dptr(loss), dptr(logits), stream_ptr()))
    return loss[0], logits


class Disentangle:
    """The rider of one dsd_eval_loss call on a DSUnetModel (dsd_set_disentangle): ``mode`` as training_losses(disentangle=)
    spells it, the label rows of a batch of ``B`` (disentangle_labels) and the buffers the call fills: ``loss`` [2] (c_s, s_a_l),
    ``logits_cs`` [6B,6B], ``logits_sal`` [7B,7B]."""

    def __init__(self, mode: str, B: int, device, temperature_cs: float = 0.05, temperature_sal: float = 0.1):
        if mode not in DISENTANGLE_MODES:
            raise NotImplementedError(f"disentangle {mode!r} not supported: one of {DISENTANGLE_MODES}")
        self.mode, self.B = mode, int(B)
        self.temperature_cs, self.temperature_sal = float(temperature_cs), float(temperature_sal)
        self.labels_cs, self.labels_sal = (label_rows(l).to(device=device, dtype=torch.int32) for l in disentangle_labels(self.B))
        new = lambda *shape: torch.zeros(shape, device=device, dtype=torch.float32)
        self.loss, self.logits_cs, self.logits_sal = new(2), new(6 * self.B, 6 * self.B), new(7 * self.B, 7 * self.B)

    def terms(self) -> dict:
        """What training_losses adds (:960-975): the two 0-dim losses and the four raw matrices of ``contrast_map``."""
        return {"disen_c_s_loss": self.loss[0], "disen_s_a_l_loss": self.loss[1],
                "contrast_map": {"c_s_heatmap": self.logits_cs, "perfect_c_s_heatmap": perfect_logit(self.labels_cs),
                                 "s_a_l_heatmap": self.logits_sal, "perfect_s_a_l_heatmap": perfect_logit(self.labels_sal)}}


@contextlib.contextmanager
def disentangle_set(unet, d: Optional[Disentangle]):
    """dsd_set_disentangle around a dsd_eval_loss call on the denoiser's handle; always cleared afterwards.  None: nothing."""
    if d is None:
        yield
        return
    spec = _lib.DsdDisentangle()
    spec.mode = CONTRAST_MODES[d.mode]
    spec.temperature_cs, spec.temperature_sal = d.temperature_cs, d.temperature_sal
    spec.labels_cs, spec.n_labels_cs = d.labels_cs.data_ptr(), int(d.labels_cs.numel())
    spec.labels_sal, spec.n_labels_sal = d.labels_sal.data_ptr(), int(d.labels_sal.numel())
    spec.loss, spec.logits_cs, spec.logits_sal = d.loss.data_ptr(), d.logits_cs.data_ptr(), d.logits_sal.data_ptr()
    check(lib().dsd_set_disentangle(unet._h, C.byref(spec)))
    try:
        yield
    finally:
        check(lib().dsd_set_disentangle(unet._h, None))


def head_views(feats: dict):
    """(content + style, style + anatomy + lesion) view lists of DSUnetModel's feature dict, in the order training_losses
    concatenates them (:909-918, :940); ValueError naming the keys a dict lacks."""
    missing = [k for k in HEAD_VIEWS if k not in feats]
    if missing:
        raise ValueError(f"disentangle= reads the 'content' / 'style' / 'anatomy' / 'lesion' lists of the model's dict; it lacks {missing}")
    f = {k: list(feats[k]) for k in HEAD_VIEWS}
    return f["content"] + f["style"], f["style"] + f["anatomy"] + f["lesion"]
