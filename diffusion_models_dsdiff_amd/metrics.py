"""Validation metrics of a batch of samples: MAE, Gaussian SSIM and MS-SSIM, and the metric table of a volume, evaluated on the device.

What every trainer of the reference does at the end of ``validation_step`` — ``MAEMetric`` and ``SSIMMetric(spatial_dims=2[,
data_range=2.0])`` of monai.metrics on the samples (trainers/trainer_ddpm.py:79-80,529-532, 540-565;
trainers/trainer_use_gaussian_diff.py:99-102,519-584) — and the per-slice MS-SSIM behind the "ssim" column of the inference metric
table (inference/test_metrics.py:249-274).  Device tensors go through ``dsd_op_image_metrics`` (csrc/metrics.hip: fp64 from the
load onward, one launch sequence, one read-back); CPU tensors take the float64 host functions of ``host_io``, so the module works
without a GPU.  There is no other path: a device tensor without the library is an error.

``volume_metrics`` is the per-id row of the inference metric table (inference/get_metric_BraTs.py:78-104 over the array functions of
inference/test_metrics.py:149-246,378-400): NRMSE, MAPE, sMAPE, logac, medsymac, PSNR and the box-window SSIM of one [D,H,W] pair.
Device tensors go through ``dsd_op_volume_metrics`` (csrc/volume_metrics.hip); CPU tensors and arrays through ``host_io.nrmse`` ...
``host_io.ssim``, which are also what tests/test_volume_metrics_gpu.py holds the device to.

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


# ------------------------------------------------------------------------------------------------ the metric table of a volume
VOLUME_STATUS = (
    (_lib.VOLUME_EMPTY_MASK, "volume_metrics: the mask is empty"),
    (_lib.VOLUME_EMPTY_CROP, "volume_metrics: the mask's bounding box [lo, hi) has a side of 0 (the upper bound is exclusive)"),
    (_lib.VOLUME_ZERO_STD, "volume_metrics: target or pred has a standard deviation of 0 in a domain the 12-bit rescale is taken over"),
    (_lib.VOLUME_ZERO_RANGE, "volume_metrics: the target's range is 0 under nrmse or psnr"),
    (_lib.VOLUME_SMALL_R, "win_size must be odd and not exceed any image side"),       # host_io.structural_similarity's own words
)


def _volume_check(shape_t, shape_p, shape_m, win):
    """The refusals of dsd_op_volume_metrics that need no device, in its words."""
    if len(shape_t) != 3 or tuple(shape_t) != tuple(shape_p):
        raise ValueError(f"volume_metrics: target {tuple(shape_t)} and pred {tuple(shape_p)} must be one shape [D,H,W]")
    if shape_m is not None and tuple(shape_m) != tuple(shape_t):
        raise ValueError(f"volume_metrics: mask {tuple(shape_m)} does not have the volumes' shape {tuple(shape_t)}")
    D, H, W = (int(v) for v in shape_t)
    if min(D, H, W) < 1:
        raise ValueError(f"volume_metrics: bad shape: D {D} H {H} W {W}")
    if D * H * W > 1 << _lib.VOLUME_MAX_LOG2:
        raise ValueError(f"volume_metrics: D*H*W = {D * H * W} voxels; up to 2^{_lib.VOLUME_MAX_LOG2} are taken")
    if not (win == 0 or (3 <= win <= 11 and win % 2 == 1)):
        raise ValueError(f"volume_metrics: win is {win}; 0 (no ssim3d) or an odd value from 3 to 11")


def _volume_device(target, pred, mask, win):
    """out [DSD_VOLUME_NOUT] of dsd_op_volume_metrics as a float64 array (``_lib.VOLUME_SLOTS`` names the slots): fp64 tensors go
    as they are, everything else as fp32; the mask as uint8."""
    dt = torch.float64 if target.dtype == torch.float64 or pred.dtype == torch.float64 else torch.float32
    t, p = target.detach().to(dt).contiguous(), pred.detach().to(dt).contiguous()
    m = None if mask is None else (mask.detach() != 0).to(torch.uint8).contiguous()
    out = torch.empty(_lib.VOLUME_NOUT, dtype=torch.float64, device=t.device)
    spec = _lib.DsdVolumeMetrics()
    spec.target, spec.pred = t.data_ptr(), p.data_ptr()
    spec.elem_is_double = int(dt == torch.float64)
    spec.mask = m.data_ptr() if m is not None else None
    spec.D, spec.H, spec.W = (int(v) for v in t.shape)
    spec.win = int(win)
    spec.out = out.data_ptr()
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().dsd_op_volume_metrics(C.byref(spec), _lib.stream_ptr()))
    return out.cpu().numpy()                                       # the one read-back


def _volume_host(t, p, mask, win):
    """The same slots from the float64 host functions (and numpy for the auxiliary values)."""
    t, p = np.asarray(t, dtype=np.float64), np.asarray(p, dtype=np.float64)
    mask = None if mask is None else np.asarray(mask) != 0
    m = host_io._mask(t, mask)
    nz = np.nonzero(m)
    if nz[0].size == 0:
        raise ValueError(VOLUME_STATUS[0][1])
    lo, hi = [int(a.min()) for a in nz], [int(a.max()) for a in nz]
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    out = dict(nrmse=host_io.nrmse(t, p, mask), mape=host_io.mape(t, p, mask), smape=host_io.smape(t, p, mask),
               logac=host_io.logac(t, p, mask), medsymac=host_io.medsymac(t, p, mask), psnr=host_io.psnr(t, p, mask), ssim3d=float("nan"),
               status=0.0, n_M=float(nz[0].size))
    if win == 9:
        out["ssim3d"] = host_io.ssim(t, p, mask)
    elif win:                                                      # host_io.ssim's statements with another window
        tr, pr = (t[sl], p[sl]) if mask is not None else (t, p)
        tr, pr = host_io.scale12bit(tr), host_io.scale12bit(pr)
        out["ssim3d"] = host_io.structural_similarity(tr, pr, win_size=win, data_range=tr.max() - tr.min())
    for a, name in enumerate("dhw"):
        out["lo_" + name], out["hi_" + name] = float(lo[a]), float(hi[a])
    doms = {"M": (t[m], p[m]), "Z": (np.where(m, t, 0)[sl], np.where(m, p, 0)[sl]), "R": (t[sl], p[sl]) if mask is not None else (t, p)}
    for d, (a, b) in doms.items():
        empty = a.size == 0
        out["mean_t_" + d], out["std_t_" + d] = (float("nan"),) * 2 if empty else (float(np.mean(a)), float(np.std(a)))
        out["mean_p_" + d], out["std_p_" + d] = (float("nan"),) * 2 if empty else (float(np.mean(b)), float(np.std(b)))
    return np.asarray([out[k] for k in _lib.VOLUME_SLOTS], dtype=np.float64)


def volume_metrics(target, pred, mask=None, win=0):
    """target / pred: tensors or arrays [D,H,W]; mask: the same shape (non-zero = inside) or None; win: the window of the 3-D SSIM,
    0 (skipped: ``ssim3d`` is NaN) or odd 3..11, the reference uses 9.  Returns a dict of Python floats

      nrmse, mape, smape, logac, medsymac   over M, the voxels inside the mask (``host_io.nrmse`` ... ``host_io.medsymac``)
      psnr                                   over Z: zero outside the mask, cropped to the mask's box [lo, hi) (``host_io.psnr``)
      ssim3d                                 over R: the raw crop, or the whole volume without a mask (``host_io.ssim``)

    plus the auxiliary values ``n_M`` (int), ``lo`` / ``hi`` (per axis the smallest / largest index holding a mask voxel; the crop
    drops plane ``hi``) and ``mean_t_M`` ... ``std_p_R``, the mean and population std of target and pred in each domain.  CUDA tensors
    are evaluated by the library (fp64 tensors as fp64, others as fp32 values, fp64 arithmetic); anything on the CPU by the float64
    host functions, bit for bit.  An empty mask, a box with a side of 0, a zero std or range, or (win > 0) a side of R below win raise
    ValueError on the device path; the host functions answer those with numpy's own errors or non-finite values."""
    win = int(win)
    on_device = isinstance(target, torch.Tensor) and target.is_cuda
    _volume_check(target.shape, pred.shape, None if mask is None else mask.shape, win)
    if on_device:
        if not (isinstance(pred, torch.Tensor) and pred.device == target.device) or \
                (mask is not None and not (isinstance(mask, torch.Tensor) and mask.device == target.device)):
            raise ValueError("volume_metrics: target, pred and mask are on different devices")
        raw = _volume_device(target, pred, mask, win)
    else:
        cpu = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        raw = _volume_host(cpu(target), cpu(pred), None if mask is None else cpu(mask), win)
    status = int(raw[_lib.VOLUME_SLOTS.index("status")])
    for bit, text in VOLUME_STATUS:
        if status & bit:
            raise ValueError(text)
    out = {k: float(v) for k, v in zip(_lib.VOLUME_SLOTS, raw)}
    del out["status"]
    out["n_M"] = int(out["n_M"])
    out["lo"] = tuple(int(out.pop("lo_" + a)) for a in "dhw")
    out["hi"] = tuple(int(out.pop("hi_" + a)) for a in "dhw")
    return out
