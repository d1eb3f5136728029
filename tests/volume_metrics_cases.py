"""Shared cases and float64 references of the volume-metric tests (test_volume_metrics_cpu.py, test_volume_metrics_gpu.py,
test_volume_ssim3d_gpu.py).

Volumes are built the way image_metrics_cases.volume() builds its pair: per slice ``blob_image * 500 + 600``, the prediction the
reference plus 25 * randn, both rounded through fp32 so that host and device start from the same numbers.  Every reference is a
float64 host function of host_io or plain numpy, computed once per case and cached; none goes through
diffusion_models_dsdiff_amd.metrics."""
import functools

import numpy as np

from diffusion_models_dsdiff_amd import host_io
from image_metrics_cases import BAR, BAR_REL, blob_image  # noqa: F401  (the project's bars: 1e-10 absolute, 1e-12 relative)

TILE_W, TILE_H = 32, 16          # window positions one ssim3d row workgroup owns (DSD_VOLUME_TILE_W / _H, asserted in the GPU files)
WIN = 9                          # the reference's window
COLUMNS = ("nrmse", "mape", "smape", "logac", "medsymac", "psnr")
DOMAINS = ("M", "Z", "R")


def pair(D, H, W, seed):
    r = np.random.RandomState(seed)
    t = np.stack([blob_image(1, H, W, seed * 100 + i)[0] for i in range(D)]) * 500. + 600.
    p = t + 25. * r.randn(D, H, W)
    return t.astype(np.float32).astype(np.float64), p.astype(np.float32).astype(np.float64)


def ellipsoid(D, H, W, grow=1.0):
    """Off the centre by (0.3, 0.2, 0.1) voxels: a centred one is symmetric and holds an even number of voxels at every size."""
    z, y, x = np.mgrid[0:D, 0:H, 0:W].astype(np.float64)
    q = (((z - (D - 1) / 2 - 0.3) / (0.42 * D * grow)) ** 2 + ((y - (H - 1) / 2 - 0.2) / (0.40 * H * grow)) ** 2 +
         ((x - (W - 1) / 2 - 0.1) / (0.38 * W * grow)) ** 2)
    return q <= 1.0


def box(shape, sl):
    m = np.zeros(shape, dtype=bool)
    m[sl] = True
    return m


def _ell(D, H, W, seed):
    t, p = pair(D, H, W, seed)
    outer = ellipsoid(D, H, W, 1.12)                     # outside the slightly larger ellipsoid both volumes are 0, as a skull-stripped scan
    return np.where(outer, t, 0.0), np.where(outer, p, 0.0), ellipsoid(D, H, W)


def _build(name):
    if name == "min":                                    # the crop is 9 x 9 x 10: one and two interior positions of the 9^3 window
        t, p = pair(12, 15, 16, 1)
        return t, p, box(t.shape, (slice(1, -1), slice(2, -3), slice(3, -2)))
    if name == "ell":
        return _ell(14, 37, 45, 2)
    if name == "nomask":                                 # R is the whole volume, Z is [0, n - 1)
        t, p = pair(9, 9, 40, 3)
        return t, p, None
    if name == "big":
        return _ell(24, 100, 90, 4)
    if name == "clip":                                   # 24 masked voxels at +-9000, alternately in target and pred
        t, p, m = _ell(14, 37, 45, 2)
        t, p = t.copy(), p.copy()
        at = np.argwhere(m)
        at = at[np.linspace(0, len(at) - 1, 24).astype(int)]
        for i, (z, y, x) in enumerate(at):
            (t if i % 2 == 0 else p)[z, y, x] = 9000. if (i // 2) % 2 == 0 else -9000.
        return t, p, m
    if name == "f64":                                    # no value is an fp32 value: it goes up as fp64
        t, p, m = _ell(14, 37, 45, 2)
        return t * 0.1, p * 0.1, m
    # ssim3d tile edges at win 9: exactly one tile of window positions, one more in every direction (behind a mask, whose crop
    # drops the last plane), two tiles less one
    if name == "tile_exact":
        t, p = pair(WIN, TILE_H + WIN - 1, TILE_W + WIN - 1, 5)
        return t, p, None
    if name == "tile_plus1":
        t, p = pair(WIN + 3, TILE_H + WIN + 2, TILE_W + WIN + 2, 6)
        return t, p, box(t.shape, (slice(1, None), slice(1, None), slice(1, None)))
    if name == "tile_2minus1":
        t, p = pair(WIN, 2 * TILE_H - 1 + WIN - 1, 2 * TILE_W - 1 + WIN - 1, 7)
        return t, p, None
    if name == "lastplane":                              # the voxels of M that the exclusive bound drops differ most
        t, p = pair(10, 20, 22, 8)
        m = box(t.shape, (slice(2, 8), slice(3, 15), slice(4, 18)))
        last = np.zeros_like(m)
        last[7], last[:, 14], last[:, :, 17] = True, True, True
        p = np.where(m & last, t + 300., p).astype(np.float32).astype(np.float64)
        return t, p, m
    raise KeyError(name)


NAMES = ("min", "ell", "nomask", "big", "clip", "f64", "tile_exact", "tile_plus1", "tile_2minus1", "lastplane")
FP32_VALUED = tuple(n for n in NAMES if n != "f64")


def crop_slices(t, mask):
    nz = np.nonzero(host_io._mask(t, mask))
    return tuple(slice(int(a.min()), int(a.max())) for a in nz)


def ssim_ref(t, p, mask, win):
    """host_io.ssim's statements with a window of ``win`` (host_io.ssim itself at 9)."""
    if win == 9:
        return host_io.ssim(t, p, mask)
    if mask is not None:
        sl = crop_slices(t, mask)
        t, p = t[sl], p[sl]
    t, p = host_io.scale12bit(t), host_io.scale12bit(p)
    return host_io.structural_similarity(t, p, win_size=win, data_range=t.max() - t.min())


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(target, pred float64 [D,H,W], mask bool or None, and the references: the six columns, ssim3d at win 9 (None where R
    does not take the window), n_M, lo, hi and mean / std per domain).  Cached: shared between the tests, never written to."""
    t, p, mask = _build(name)
    m = host_io._mask(t, mask)
    sl = crop_slices(t, mask)
    out = dict(target=t, pred=p, mask=mask)
    for k in COLUMNS:
        out[k] = getattr(host_io, k)(t, p, mask)
    r_shape = tuple(s.stop - s.start for s in sl) if mask is not None else t.shape
    out["ssim3d"] = host_io.ssim(t, p, mask) if min(r_shape) >= WIN else None
    out["n_M"] = int(m.sum())
    out["lo"], out["hi"] = tuple(s.start for s in sl), tuple(s.stop for s in sl)
    doms = {"M": (t[m], p[m]), "Z": (np.where(m, t, 0)[sl], np.where(m, p, 0)[sl]), "R": (t[sl], p[sl]) if mask is not None else (t, p)}
    for d, (a, b) in doms.items():
        out["mean_t_" + d], out["std_t_" + d], out["mean_p_" + d], out["std_p_" + d] = (float(np.mean(a)), float(np.std(a)), float(np.mean(b)),
                                                                                    float(np.std(b)))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_cases():
    """What the cases are chosen for, asserted on the CPU."""
    c = case("clip")
    m = c["mask"]
    for a in (c["target"][m], c["pred"][m]):
        s = host_io.scale12bit(a)
        assert (s == 1e-10).any() and (s == 4095).any(), "clip: both ends of the 12-bit rescale are reached"
    n = {k: case(k)["n_M"] for k in ("min", "ell", "nomask", "big")}
    assert n["min"] == 10 * 10 * 11 and n["nomask"] == 9 * 9 * 40
    assert any(v % 2 for v in n.values()) and any(v % 2 == 0 for v in n.values()), n      # both forms of the median
    assert (case("min")["hi"][0] - case("min")["lo"][0], ) + tuple(h - l for h, l in zip(case("min")["hi"][1:], case("min")["lo"][1:])) == (9, 9, 10)
    f = case("f64")
    assert not np.array_equal(f["target"].astype(np.float32).astype(np.float64), f["target"])
    for k in FP32_VALUED:
        for v in ("target", "pred"):
            assert np.array_equal(case(k)[v].astype(np.float32).astype(np.float64), case(k)[v]), (k, v)
    # lastplane: an inclusive upper bound moves psnr by far more than the bar
    c = case("lastplane")
    t, p, m = c["target"], c["pred"], c["mask"]
    nz = np.nonzero(m)
    inc = tuple(slice(int(a.min()), int(a.max()) + 1) for a in nz)
    tz, pz = np.where(m, t, 0)[inc], np.where(m, p, 0)[inc]
    assert abs(host_io.peak_signal_noise_ratio(tz, pz, tz.max() - tz.min()) - c["psnr"]) > 1.0
    return n
