"""Upsample convolutions in the sub-pixel form (bf16x6): conv3x3(nearest_x2(x)) run as four 2x2 convolutions on the
low-resolution map (conv2d_subpixel_ok, conv_split.hip), against float64 at the bf16x6 bar of tests/test_ops_gpu.py
(2e-6 rel-L2), border rows and columns checked on their own.  Shapes the tap-reuse kernel does not take (16 x 16 and 8 x 8
inputs) keep the folded gather and are covered here as well."""
import pytest
import torch
import torch.nn.functional as F

from util import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-6


@pytest.fixture(scope="module")
def ops():
    from diffusion_models_dsdiff_amd import ops as m, _lib
    _lib.require_gpu(0)
    return m


def cu(t):
    return t.cuda().contiguous()


CASES = [
    # N, H, W, Cin, Cout, emb / residual
    (1, 128, 128, 320, 320, False),    # -> 256 x 256, the first decoder level's Upsample
    (1, 64, 64, 640, 640, True),       # -> 128 x 128
    (2, 32, 32, 640, 640, True),       # -> 64 x 64, two samples
    (2, 16, 16, 640, 1280, False),     # -> 32 x 32 (folded: width 16)
    (1, 8, 8, 1280, 1280, True),       # -> 16 x 16 (folded)
    (2, 16, 64, 64, 160, True),        # non-square, 32 x 128 output, one column tile per phase
]


@pytest.mark.parametrize("case", CASES)
def test_subpixel_upsample_conv(ops, case):
    N, H, W, Cin, Cout, fuse = case
    g = torch.Generator().manual_seed(sum(case[:5]) + 17)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    emb = torch.randn(N, Cout, generator=g) if fuse else None
    res = torch.randn(N, Cout, 2 * H, 2 * W, generator=g) if fuse else None
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
    if fuse:
        ref = ref + emb.double()[:, :, None, None] + res.double()
    y = ops.conv2d(cu(ops.to_nhwc(x)), cu(w), cu(b), upsample=True, emb=cu(emb) if fuse else None,
                   res=cu(ops.to_nhwc(res)) if fuse else None, precision="bf16x6")
    yy = ops.to_nchw(y).double().cpu()
    assert rel_l2(yy, ref) < TOL, case
    OH, OW = 2 * H, 2 * W
    for sl in ((..., 0, slice(None)), (..., OH - 1, slice(None)), (..., slice(None), 0), (..., slice(None), OW - 1),
               (..., slice(0, None, 2), slice(1, None, 2)), (..., slice(1, None, 2), slice(0, None, 2))):
        assert rel_l2(yy[sl], ref[sl]) < TOL, (case, sl)


def test_subpixel_matches_folded_f32(ops):
    """GPU against GPU: the sub-pixel bf16x6 launch against the exact fp32 folded-gather kernel on the same input."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 320, 64, 64, generator=g)
    w = torch.randn(320, 320, 3, 3, generator=g) / (320 * 9) ** 0.5
    b = torch.randn(320, generator=g)
    xs, ws, bs = cu(ops.to_nhwc(x)), cu(w), cu(b)
    y6 = ops.conv2d(xs, ws, bs, upsample=True, precision="bf16x6")
    y32 = ops.conv2d(xs, ws, bs, upsample=True, precision="f32")
    assert rel_l2(y6, y32) < 1e-6
