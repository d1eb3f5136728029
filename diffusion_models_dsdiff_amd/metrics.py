"""Validation metrics of a batch of samples: MAE, Gaussian SSIM and MS-SSIM, evaluated on the device.

What every trainer of the reference does at the end of ``validation_step`` — ``MAEMetric`` and ``SSIMMetric(spatial_dims=2[,
data_range=2.0])`` of monai.metrics on the samples (trainers/trainer_ddpm.py:79-80,529-532, 540-565;
trainers/trainer_use_gaussian_diff.py:99-102,519-584) — and the per-slice MS-SSIM behind the "ssim" column of the inference metric
table (inference/test_metrics.py:249-274).  Device tensors go through ``dsd_op_image_metrics`` (csrc/metrics.hip: fp64 from the
load onward, one launch sequence, one read-back); CPU tensors take the float64 host functions of ``host_io``, so the module works
without a GPU.  There is no other path: a device tensor without the library is an error.

PARITY UNPINNED: MONAI and torchmetrics are not installable here and the reference holds no value of either.  The formulas are the
published definitions (``host_io.ssim_gaussian``, ``host_io.multiscale_structural_similarity``); tests/test_image_metrics_cpu.py
cross-checks them against MONAI's own formulation (a grouped conv2d with the 11 x 11 outer-product kernel) and
tests/test_image_metrics_gpu.py holds the device to 1e-10 of them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, host_io

MS_SSIM_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _check(shape, scales, data_range, pre):
    """The refusals of dsd_op_image_metrics, for the host path (the device path gets them from the library)."""
    B, Cn, H, W = shape
    if not 1 <= scales <= _lib.METRICS_MAX_SCALES:
        raise ValueError(f"image_metrics: scales is {scales}; 1 to {_lib.METRICS_MAX_SCALES} are taken")
    if min(H, W) >> (scales - 1) < 11:
        raise ValueError(f"image_metrics: scale {scales} of a {H} x {W} image has a side of {min(H, W) >> (scales - 1)}; "
                         "the 11-tap window needs 11")
    if not (np.isfinite(data_range) and data_range >= 0):
        raise ValueError(f"image_metrics: data_range is {data_range}; a positive value, or 0 for each sample's own range")
    if pre is not None:
        if len(pre) != 7:
            raise ValueError("image_metrics: pre is (mean_pred, div_pred, mean_target, div_target, add, lo, hi)")
        if pre[1] == 0 or pre[3] == 0:
            raise ValueError(f"image_metrics: pre divides by div = 0 ({pre[1]}, {pre[3]})")
        if pre[5] > pre[6]:
            raise ValueError(f"image_metrics: pre clips to lo = {pre[5]} above hi = {pre[6]}")


def _host(pred, target, scales, data_range, pre):
    """scale [B,S,2] and elem [B,6] as the device writes them, from the float64 host functions."""
    p, t = pred.detach().double().numpy(), target.detach().double().numpy()
    if pre is not None:
        mp, dp, mt, dt, add, lo, hi = (float(v) for v in pre)
        p, t = np.clip((p - mp) / dp + add, lo, hi), np.clip((t - mt) / dt + add, lo, hi)
    scale = np.stack([host_io.ssim_scale_table(p[b], t[b], scales, data_range if data_range > 0 else None) for b in range(p.shape[0])])
    d = (p - t).reshape(p.shape[0], -1)
    flat = lambda a: a.reshape(a.shape[0], -1)
    elem = np.stack([np.abs(d).sum(1), (d * d).sum(1), flat(t).min(1), flat(t).max(1), flat(p).min(1), flat(p).max(1)], axis=1)
    return scale, elem


def _device(pred, target, scales, data_range, pre):
    p, t = pred.detach().float().contiguous(), target.detach().float().contiguous()
    B, Cn, H, W = p.shape
    out = torch.empty(B * (2 * scales + 6), dtype=torch.float64, device=p.device)
    spec = _lib.DsdImageMetrics()
    spec.pred, spec.target = p.data_ptr(), t.data_ptr()
    spec.B, spec.C, spec.H, spec.W, spec.scales = B, Cn, H, W, scales
    spec.data_range = float(data_range)
    spec.pre = (C.c_double * 7)(*[float(v) for v in pre]) if pre is not None else None
    spec.scale_out = out.data_ptr()
    spec.elem_out = out.data_ptr() + B * scales * 2 * 8
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().dsd_op_image_metrics(C.byref(spec), _lib.stream_ptr()))
    host = out.cpu().numpy()                                       # the one read-back
    return host[:B * scales * 2].reshape(B, scales, 2), host[B * scales * 2:].reshape(B, 6)


def image_metrics(pred, target, scales=1, data_range=1.0, pre=None):
    """pred / target: tensors [B,C,H,W] on one device.  Returns float64 CPU tensors per sample:

      mae, mse [B]   the mean of |p - t| and of (p - t)^2 over C*H*W
      ssim [B]       the Gaussian SSIM of scale 0 (``host_io.ssim_gaussian``: MONAI's SSIMMetric value), not clamped
      cs [B,S]       the mean contrast-structure map of every scale, not clamped
      ms_ssim [B]    with scales == 5: prod_{s<4} max(cs_s, 0)^beta_s * max(ssim_4, 0)^beta_4, betas (0.0448, 0.2856, 0.3001,
                     0.2363, 0.1333), as ``host_io.multiscale_structural_similarity``
      scale [B,S,2]  (ssim mean, cs mean) of every scale and  elem [B,6]  sum |d|, sum d^2, min t, max t, min p, max p: the raw
                     outputs of dsd_op_image_metrics

    data_range: a positive value, or 0 for each sample's own max(range(pred), range(target)).  pre: None or the seven floats
    (mean_pred, div_pred, mean_target, div_target, add, lo, hi) of  x <- clip((x - mean) / div + add, lo, hi)  applied in float64
    at the load; ``host_io.scale12bit`` is (mean, std / 400, 2048, 1e-10, 4095).  Device tensors are evaluated by the library
    (fp32 values, fp64 arithmetic); CPU tensors by the float64 host functions."""
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError(f"image_metrics: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be one shape [B,C,H,W]")
    if pred.device != target.device:
        raise ValueError("image_metrics: pred and target are on different devices")
    scales, data_range = int(scales), float(data_range)
    if pred.is_cuda:
        scale, elem = _device(pred, target, scales, data_range, pre)
    else:
        _check(tuple(pred.shape), scales, data_range, pre)
        scale, elem = _host(pred, target, scales, data_range, pre)
    n = float(pred[0].numel())
    out = {"mae": elem[:, 0] / n, "mse": elem[:, 1] / n, "ssim": scale[:, 0, 0].copy(), "cs": scale[:, :, 1].copy(), "scale": scale,
           "elem": elem}
    if scales == len(MS_SSIM_BETAS):
        vals = np.maximum(np.concatenate([scale[:, :-1, 1], scale[:, -1:, 0]], axis=1), 0.0)
        out["ms_ssim"] = np.prod(vals ** np.asarray(MS_SSIM_BETAS, dtype=np.float64), axis=1)
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)) for k, v in out.items()}


def _batch(v):
    """A [B,C,H,W] tensor, or the list of [C,H,W] tensors monai.data.decollate_batch yields."""
    return torch.stack(list(v)) if isinstance(v, (list, tuple)) else v


class _Cumulative:
    """The part of monai.metrics.CumulativeIterationMetric the trainers use: ``__call__(y_pred=, y=)`` returns the per-sample
    values [B,1] (float64, CPU) and keeps them; ``aggregate()`` is the mean over everything seen since the last ``reset()``."""

    def __init__(self):
        self._seen = []

    def _values(self, y_pred, y):
        raise NotImplementedError

    def __call__(self, y_pred, y):
        v = self._values(_batch(y_pred), _batch(y)).reshape(-1, 1)
        self._seen.append(v)
        return v

    def aggregate(self):
        if not self._seen:
            raise ValueError("aggregate() before any call: there is nothing to average")
        return torch.cat(self._seen).mean()

    def reset(self):
        self._seen = []


class MAEMetric(_Cumulative):
    """monai.metrics.MAEMetric(reduction="mean"): per sample the mean of |y_pred - y| over every element.  It rides on
    ``image_metrics``, so the images must take the 11-tap window (both sides >= 11), as in every validation_step."""

    def __init__(self, reduction="mean", get_not_nans=False):
        super().__init__()
        if reduction != "mean" or get_not_nans:
            raise ValueError(f"MAEMetric: reduction {reduction!r}, get_not_nans {get_not_nans!r}; only reduction='mean' without "
                             "the not-nan count is supported")

    def _values(self, y_pred, y):
        return image_metrics(y_pred, y)["mae"]


class SSIMMetric(_Cumulative):
    """monai.metrics.SSIMMetric(spatial_dims=2, data_range=1.0, kernel_type="gaussian", win_size=11, kernel_sigma=1.5) with
    k1 = 0.01, k2 = 0.03: per sample ``host_io.ssim_gaussian``."""

    def __init__(self, spatial_dims=2, data_range=1.0, kernel_type="gaussian", win_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03,
                 reduction="mean", get_not_nans=False):
        super().__init__()
        one = lambda v: v[0] if isinstance(v, (list, tuple)) and len(set(v)) == 1 else v
        got = dict(spatial_dims=spatial_dims, kernel_type=str(kernel_type).lower(), win_size=one(win_size), kernel_sigma=one(kernel_sigma),
                   k1=k1, k2=k2, reduction=reduction, get_not_nans=bool(get_not_nans))
        want = dict(spatial_dims=2, kernel_type="gaussian", win_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, reduction="mean",
                    get_not_nans=False)
        bad = {k: v for k, v in got.items() if v != want[k]}
        if bad:
            raise ValueError(f"SSIMMetric: {bad} not supported; the device kernel is built for {want}")
        if not data_range > 0:
            raise ValueError(f"SSIMMetric: data_range is {data_range}; a positive value is needed")
        self.data_range = float(data_range)

    def _values(self, y_pred, y):
        return image_metrics(y_pred, y, data_range=self.data_range)["ssim"]
