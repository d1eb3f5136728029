"""Shared cases and float64 references of the image-metric tests (test_image_metrics_cpu.py, test_image_metrics_gpu.py).

Images are Gaussian blobs plus noise drawn from a seed, held as fp32 values so that host and device start from the same
numbers.  Every reference is a float64 host function of host_io (scipy) or plain numpy, computed once per case and cached; none
goes through diffusion_models_dsdiff_amd.metrics."""
import functools

import numpy as np

from diffusion_models_dsdiff_amd import host_io

TILE_W, TILE_H = 32, 16          # window positions one map workgroup owns (DSD_METRICS_TILE_W / _H, asserted in the GPU file)
HALO = 10
BAR = 1e-10                      # absolute, on every ssim / cs / ms_ssim value: > 3 decades above float64 reordering (2.2e-14),
BAR_REL = 1e-12                  # 2 decades below the best fp32 window (1.5e-8); relative, on mae / mse / the elem sums
SIZES = [(11, 11), (12, 13), (11, 37), (65, 33), (176, 176), (177, 183)]


def blob_image(C, H, W, seed):
    """[C,H,W] float64 in [-1,1]: per channel three Gaussian blobs of its own plus noise."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((C, H, W))
    for c in range(C):
        img = -0.6 * np.ones((H, W))
        for _ in range(3):
            cy, cx, s, a = r.uniform(0, H), r.uniform(0, W), r.uniform(0.08, 0.3) * max(H, W), r.uniform(0.5, 1.4)
            img += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        out[c] = img + 0.05 * r.randn(H, W)
    return np.clip(out, -1.0, 1.0)


def pair(B, C, H, W, seed, kind="noisy"):
    """(pred, target) fp32 [B,C,H,W].  noisy: pred = target + noise;  same: pred = target;  negative: pred = -target + noise;
    offset: the 12-bit form, mean 2048 and std 400;  amp: [-1,1] data whose amplitude differs per sample (for a per-sample range)."""
    r = np.random.RandomState(seed + 1000)
    t = np.stack([blob_image(C, H, W, seed + 17 * b) for b in range(B)])
    if kind == "amp":
        t = t * np.asarray([1.0, 0.6, 0.3, 0.8][:B]).reshape(B, 1, 1, 1)
    noise = 0.1 * r.randn(*t.shape)
    p = {"noisy": t + noise, "amp": t + noise, "same": t.copy(), "negative": -t + noise, "offset": t + noise}[kind]
    if kind == "offset":
        m, s = t.mean(), t.std()
        t, p = (t - m) / s * 400. + 2048., (p - m) / s * 400. + 2048.
    else:
        p = np.clip(p, -1.0, 1.0)
    return p.astype(np.float32), t.astype(np.float32)


def pre12(p, t):
    """The seven numbers of host_io.scale12bit for a batch: mean and std over the whole array, in float64."""
    p, t = p.astype(np.float64), t.astype(np.float64)
    return (float(np.mean(p)), float(np.std(p) / 400.), float(np.mean(t)), float(np.std(t) / 400.), 2048., 1e-10, 4095.)


# name: (B, C, H, W, seed, kind, scales, data_range, 12-bit pre)
CASES = {
    # window edges: one output, the first size with more than one, a single output row
    "win_11x11": (1, 1, 11, 11, 1, "noisy", 1, 2.0, False),
    "win_12x13": (3, 2, 12, 13, 2, "noisy", 1, 2.0, False),
    "win_11x37": (1, 2, 11, 37, 3, "noisy", 1, 2.0, False),
    # tile edges: exactly one tile of outputs, one more in both directions, two tiles less one
    "tile_exact": (1, 1, TILE_H + HALO, TILE_W + HALO, 4, "noisy", 1, 2.0, False),
    "tile_plus1": (3, 2, TILE_H + 1 + HALO, TILE_W + 1 + HALO, 5, "noisy", 1, 2.0, False),
    "tile_2minus1": (1, 2, 2 * TILE_H - 1 + HALO, 2 * TILE_W - 1 + HALO, 6, "noisy", 1, 2.0, False),
    "mid_65x33": (3, 1, 65, 33, 7, "noisy", 2, 1.0, False),
    # five scales: the smallest admissible size, and 177 x 183 (H halves odd, odd, even, even: two odd-row drops)
    "ms_176": (1, 1, 176, 176, 8, "noisy", 5, 2.0, False),
    "ms_177x183": (3, 2, 177, 183, 9, "noisy", 5, 2.0, False),
    "ms_177x183_12bit": (3, 1, 177, 183, 10, "amp", 5, 0.0, True),
    "ms_176_12bit_c2": (1, 2, 176, 176, 11, "amp", 5, 0.0, True),
    # where an fp32 E[x^2] - m^2 loses its digits
    "offset_2048": (3, 1, 65, 33, 12, "offset", 1, 0.0, False),
    "same": (1, 2, 27, 43, 13, "same", 1, 2.0, False),
    "negative": (1, 1, 176, 176, 14, "negative", 5, 2.0, False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(pred, target fp32 [B,C,H,W], scales, data_range, pre, and the float64 references scale [B,S,2], elem [B,6], mae,
    mse, ssim [B], ms_ssim [B] or None).  Cached: shared between the tests, never written to."""
    B, C, H, W, seed, kind, scales, data_range, pre_on = CASES[name]
    p, t = pair(B, C, H, W, seed, kind)
    pre = pre12(p, t) if pre_on else None
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    if pre is not None:                                   # host_io.scale12bit's expression, with the batch's mean and std
        p64 = np.clip(((p64 - pre[0]) / pre[1]) + pre[4], pre[5], pre[6])
        t64 = np.clip(((t64 - pre[2]) / pre[3]) + pre[4], pre[5], pre[6])
    rng = None if data_range == 0 else data_range
    scale = np.stack([host_io.ssim_scale_table(p64[b], t64[b], scales, rng) for b in range(B)])
    ssim = np.asarray([host_io.ssim_gaussian(p64[b], t64[b], rng) for b in range(B)])
    d = (p64 - t64).reshape(B, -1)
    fl = lambda a: a.reshape(B, -1)
    elem = np.stack([np.abs(d).sum(1), (d * d).sum(1), fl(t64).min(1), fl(t64).max(1), fl(p64).min(1), fl(p64).max(1)], axis=1)
    ms = None
    if scales == 5:
        betas = np.asarray((0.0448, 0.2856, 0.3001, 0.2363, 0.1333))
        ms = np.prod(np.maximum(np.concatenate([scale[:, :4, 1], scale[:, 4:, 0]], axis=1), 0.0) ** betas, axis=1)
        if C == 1:                                        # the existing host function, where it applies (one 2-D pair)
            direct = np.asarray([host_io.multiscale_structural_similarity(p64[b, 0], t64[b, 0], rng) for b in range(B)])
            assert np.abs(direct - ms).max() < 1e-13, (name, direct, ms)
    out = dict(pred=p, target=t, scales=scales, data_range=data_range, pre=pre, scale=scale, ssim=ssim, elem=elem,
               mae=np.asarray([host_io.mae(p64[b], t64[b]) for b in range(B)]), mse=(d * d).mean(1), ms_ssim=ms)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def tensors(c, device="cpu"):
    """(pred, target) of a case as fresh torch tensors (the cached arrays are read-only)."""
    import torch
    return torch.from_numpy(c["pred"].copy()).to(device), torch.from_numpy(c["target"].copy()).to(device)


def ssim_conv2d(pred, target, data_range):
    """MONAI's own formulation, independent of host_io's: torch float64 F.conv2d with the 11 x 11 outer-product kernel,
    groups = C, no padding; the map averaged over channels and positions.  pred / target [C,H,W]."""
    import torch
    import torch.nn.functional as F
    x, y = torch.as_tensor(np.asarray(pred), dtype=torch.float64)[None], torch.as_tensor(np.asarray(target), dtype=torch.float64)[None]
    C = x.shape[1]
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(d / 1.5) ** 2 / 2)
    g = g / g.sum()
    k = torch.outer(g, g)[None, None].expand(C, 1, 11, 11).contiguous()
    R = float(max(x.max() - x.min(), y.max() - y.min())) if data_range is None else float(data_range)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    blur = lambda a: F.conv2d(a, k, groups=C)
    mx, my = blur(x), blur(y)
    sx, sy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    cs = (2 * sxy + c2) / (sx + sy + c2)
    return float((((2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1)) * cs).mean())


def volume(seed=21, D=6, H=190, W=200):
    """A synthetic [D,H,W] pair of fp32-valued float64 volumes and a box mask, for the metric table."""
    r = np.random.RandomState(seed)
    t = np.stack([blob_image(1, H, W, seed + i)[0] for i in range(D)]) * 500. + 600.
    p = t + 25. * r.randn(D, H, W)
    mask = np.zeros((D, H, W), dtype=bool)
    mask[:, 4:186, 6:196] = True
    return t.astype(np.float32).astype(np.float64), p.astype(np.float32).astype(np.float64), mask
