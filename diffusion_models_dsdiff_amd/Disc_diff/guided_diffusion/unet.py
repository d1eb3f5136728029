"""UNet_disc_Model / SuperResModelNew — drop-in for the reference's Disc_diff/guided_diffusion/unet.py:726-1044,1063-1076,
executed by libdsdiff.so (dsd_create_disc).

The four-stream DisC-Diff denoiser that ``configs/disc-diff.yaml`` and ``configs/disc-diff-origin.yaml`` name as
``unet_config.target`` and that ``sr_create_model`` (script_util.py) builds: four single-channel encoders with their own weights
(``input_blocks``, ``input_blocks_T1``, ``input_blocks_T2``, ``input_blocks_DWI``), every skip the four-stream mean, a bottleneck
head of two shared convolutions, five SE gates and a Conv1x1, one decoder.  Same constructor signature, same ``state_dict``
names, shapes and order, ``forward`` returns the reference's 9-tuple ``(com_h1..4, dist_h1..4, out)``.  The nn.Module only holds
the parameters; every FLOP runs in the hand-written gfx950 kernels behind the C ABI (include/dsdiff.h).  No CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from ... import _lib as _L
from ..._lib import DsdConfig, check, dptr, lib, stream_ptr
from ...UNet_DS_Diff.model import NativeModule
from ...blocks import SE_Attention                            # noqa: F401  (unet.py:82-109 lives with the single blocks)

__all__ = ["UNet_disc_Model", "SuperResModelNew", "SE_Attention"]


class UNet_disc_Model(NativeModule):
    """unet.py:726-1044.  ``device_index`` (an extension): the GPU to run on; a negative one builds the parameter table only
    (names, shapes, ``state_dict``), without a device."""

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, use_checkpoint=False, use_fp16=False, num_heads=1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, device_index: int = 0):
        super().__init__()
        if dims != 2 or not conv_resample or dropout != 0 or use_fp16:
            raise NotImplementedError("hot path is dims=2, conv_resample=True, dropout=0, fp32 (SURVEY.md 8)")
        if in_channels != 1:
            raise ValueError(f"in_channels must be 1: every stream of UNet_disc_Model.forward receives one plane of x_batch "
                             f"(unet.py:997-1000), got {in_channels}")
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads                                       # :777-778
        channel_mult = [int(m) for m in channel_mult]
        self.image_size = image_size
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = attention_resolutions
        self.dropout = dropout
        self.channel_mult = tuple(channel_mult)
        self.conv_resample = conv_resample
        self.use_checkpoint = use_checkpoint
        self.dtype = torch.float32
        self.num_heads = num_heads
        self.num_head_channels = num_head_channels
        self.num_heads_upsample = num_heads_upsample
        self.num_classes = None
        self._device_index = device_index

        if device_index >= 0:
            _L.require_gpu(device_index)
        cfg = DsdConfig()
        cfg.in_channels, cfg.model_channels, cfg.out_channels = in_channels, model_channels, out_channels
        cfg.n_levels = len(channel_mult)
        for i, m in enumerate(channel_mult):
            cfg.channel_mult[i], cfg.num_res_blocks[i] = m, int(num_res_blocks)
        ar = [int(a) for a in attention_resolutions]
        cfg.n_attention_resolutions = len(ar)
        for i, a in enumerate(ar):
            cfg.attention_resolutions[i] = a
        cfg.num_heads, cfg.num_head_channels, cfg.num_heads_upsample = num_heads, num_head_channels, num_heads_upsample
        cfg.use_scale_shift_norm = int(bool(use_scale_shift_norm))
        cfg.resblock_updown = int(bool(resblock_updown))
        cfg.use_new_attention_order = int(bool(use_new_attention_order))
        self._cfg = cfg
        check(lib().dsd_create_disc(C.byref(cfg), device_index, C.byref(self._h)))
        self._build_params()
        conv_ch = int(channel_mult[0] * model_channels) * channel_mult[-1]
        self._half = int(conv_ch / 2)
        if device_index >= 0:
            if os.environ.get("DSD_PRECISION"):
                self.set_precision(os.environ["DSD_PRECISION"])
            half = model_channels // 2
            freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half).contiguous()
            check(lib().dsd_set_timestep_freqs(self._h, C.c_void_p(freqs.data_ptr()), half))

    # ---- reference API ---------------------------------------------------------------------------
    def forward(self, x_batch, timesteps):
        """:985-1044.  x_batch: [B,4,H,W] fp32 CUDA (x, T1, T2, DWI); timesteps: [B] int64 or float.  Returns
        (com_h1, com_h2, com_h3, com_h4, dist_h1, dist_h2, dist_h3, dist_h4, out)."""
        out, feats = self._run(x_batch, timesteps, want_feats=True)
        return tuple(feats) + (out,)

    @torch.no_grad()
    def _run(self, x, timesteps, want_feats: bool):
        if self._device_index < 0:
            raise _L.DsdError("this UNet_disc_Model was built without a device (parameter table only)")
        if not x.is_cuda:
            raise _L.DsdError("UNet_disc_Model runs on the MI355X only: input tensor is on the CPU (no CPU fallback)")
        self.sync_params()
        x = x.float().contiguous()
        B, Cc, H, W = x.shape
        t = timesteps.to(x.device)
        t_is_float = t.dtype.is_floating_point
        t = (t.float() if t_is_float else t.long()).contiguous()
        assert t.shape == (B,)
        out = torch.empty((B, self.out_channels, H, W), device=x.device, dtype=torch.float32)
        feats, fptr = [], None
        if want_feats:
            ds = 2 ** (len(self.channel_mult) - 1)
            feats = [torch.empty((B, self._half, H // ds, W // ds), device=x.device, dtype=torch.float32) for _ in range(8)]
            fptr = (C.c_void_p * 8)(*[f.data_ptr() for f in feats])
        check(lib().dsd_forward(self._h, dptr(x), C.c_void_p(t.data_ptr()), int(t_is_float), B, Cc, H, W, dptr(out), fptr,
                                stream_ptr()))
        return out, feats

    def convert_to_fp16(self):
        raise NotImplementedError("the hot path is fp32 end-to-end (SURVEY.md 9, quirk 8)")

    def convert_to_fp32(self):
        return None


class SuperResModelNew(UNet_disc_Model):
    """unet.py:1063-1076: takes ``**kwargs`` (t1 / t2 / dwi, already concatenated behind x by the sampler) and ignores them."""

    def __init__(self, image_size, in_channels, *args, **kwargs):
        super().__init__(image_size, in_channels, *args, **kwargs)

    def forward(self, x, timesteps, **kwargs):
        return super().forward(x, timesteps)
