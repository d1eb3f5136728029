"""Sub-pixel form of the upsample convolution (host side, no GPU): the phase weights of dsd_subpixel_weights_host turn
conv3x3(nearest_x2(x)) into four 2x2 convolutions on the low-resolution map, exactly (float64)."""
import ctypes as C

import numpy as np

from diffusion_models_dsdiff_amd import _lib


def _conv3x3_up_ref(x, w):
    """float64 conv3x3(nearest_x2(x)), padding 1; x [C, H, W], w [Co, C, 3, 3]."""
    u = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    up = np.pad(u, ((0, 0), (1, 1), (1, 1)))
    H2, W2 = u.shape[1:]
    y = np.zeros((w.shape[0], H2, W2))
    for kh in range(3):
        for kw in range(3):
            y += np.einsum("oc,chw->ohw", w[:, :, kh, kw], up[:, kh:kh + H2, kw:kw + W2])
    return y


def _phase_weights(w):
    Co, Ci = w.shape[:2]
    out = np.zeros((4, Co, 2, 2, Ci), dtype=np.float64)
    wc = np.ascontiguousarray(w, dtype=np.float32)
    _lib.check(_lib.lib().dsd_subpixel_weights_host(wc.ctypes.data_as(C.c_void_p), Co, Ci, out.ctypes.data_as(C.c_void_p)))
    return out


def test_subpixel_phase_weights_reproduce_upsample_conv():
    rng = np.random.default_rng(11)
    Ci, Co, H, W = 3, 5, 4, 6
    x = rng.standard_normal((Ci, H, W))
    w = rng.standard_normal((Co, Ci, 3, 3)).astype(np.float32)
    wp = _phase_weights(w)
    ref = _conv3x3_up_ref(x, w.astype(np.float64))
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))     # low-resolution row / column -1 and H / W are zeros
    y = np.zeros_like(ref)
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        acc = np.zeros((Co, H, W))
        for a in range(2):
            for b in range(2):
                # input row i + py - 1 + a, column j + px - 1 + b (+1 for the padding)
                acc += np.einsum("oc,chw->ohw", wp[ph, :, a, b, :], xp[:, py + a:py + a + H, px + b:px + b + W])
        y[:, py::2, px::2] = acc
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


def test_subpixel_phase_tap_table():
    """Each phase tap is the sum of 1, 2 or 4 original taps: rows p = 0 {0}, {1, 2}; p = 1 {0, 1}, {2} (same for columns)."""
    w = np.zeros((1, 1, 3, 3), dtype=np.float32)
    rows = {0: ({0}, {1, 2}), 1: ({0, 1}, {2})}
    for kh in range(3):
        for kw in range(3):
            w[...] = 0
            w[0, 0, kh, kw] = 1
            wp = _phase_weights(w)
            for ph in range(4):
                py, px = ph >> 1, ph & 1
                for a in range(2):
                    for b in range(2):
                        want = 1.0 if (kh in rows[py][a] and kw in rows[px][b]) else 0.0
                        assert wp[ph, 0, a, b, 0] == want, (kh, kw, ph, a, b)
