"""Every device-resident form the plan builder derives from a weight (net.h DerivedWeight: the bf16 and fp16 pieces of the
split modes, the sub-pixel phase weights of an upsample layer, the packed Winograd weights, the 16-bit copies of the
half-precision DiT modes) must be rebuilt when its source parameter is uploaded again.  A form that is not runs the OLD
weights silently, so each case edits one weight of a handle that has already run, and compares with a FRESH handle holding
the edited weights: the same kernels on the same bits, hence ``torch.equal``.  The op kinds of the plan prove that the case
reached the kernel path whose weights it means to test; shapes are the smallest that do."""
import pytest
import torch

from oracle.synth import synth_params
from util import randn

pytestmark = pytest.mark.gpu


def _res(ch, wino=False):
    def make():
        from diffusion_models_dsdiff_amd import blocks
        m = blocks.ResBlock(ch, 128, 0, out_channels=ch)
        return m.winograd(True) if wino else m
    return make


def _up():
    from diffusion_models_dsdiff_amd import blocks
    return blocks.Upsample(160, True)


def _dit():
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import DiT
    return DiT(input_size=16, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=4, num_classes=10)


def _emb_args(shape, seed):
    return lambda: (randn(shape, seed).cuda(), randn((shape[0], 128), seed + 1).cuda())


def _dit_args():
    return randn((2, 4, 16, 16), 5).cuda(), torch.tensor([17.0, 999.0]).cuda(), torch.tensor([1, 4]).cuda()


# id -> (constructor, precision, inputs, edited weight, the op kind that proves the path)
CASES = {
    # three bf16 pieces under the layer's own name: ResBlock(64 -> 64) on 8x8
    "bf16_pieces": (_res(64), "bf16x6", _emb_args((1, 64, 8, 8), 11), "in_layers.2.weight", lambda k: k.startswith("conv_bf16x6<")),
    # "#f16": the same block in f16x3
    "f16_pieces": (_res(64), "f16x3", _emb_args((1, 64, 8, 8), 11), "in_layers.2.weight", lambda k: k.startswith("conv_f16x3<")),
    # "#sub": the smallest shape conv2d_subpixel_shape_ok admits (width 32, H * W = 256, Cout a multiple of 160)
    "subpixel": (_up, "bf16x6", lambda: (randn((1, 160, 8, 32), 13).cuda(),), "conv.weight", lambda k: k.endswith("+subpixel")),
    # "#wino": conv2d_wino_shape_ok wants Cout = 0 or 64 (mod 128), so 160 channels are out; 64 is the smallest count it takes
    # (one column tile), and 512 x 256 pixels / 256 per workgroup = 512 workgroups, the threshold of conv2d_wino_worthwhile
    "winograd": (_res(64, wino=True), "bf16x6", _emb_args((1, 64, 512, 256), 15), "in_layers.2.weight", lambda k: k == "conv_wino_bf16x6"),
    # "#h16" / "#b16": the tiny DiT of test_dit_gpu.py in the half-precision modes
    "f16_copy": (_dit, "f16", _dit_args, "blocks.0.mlp.fc1.weight", lambda k: k == "gemm16_gelu"),
    "bf16_copy": (_dit, "bf16", _dit_args, "blocks.0.mlp.fc1.weight", lambda k: k == "gemm16_gelu"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_edit_invalidates_derived_weight(case):
    make, prec, inputs, wname, is_path = CASES[case]
    m = make().set_precision(prec)
    sd = synth_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 501)   # (no zero-initialised site left)
    m.load_state_dict(sd, strict=True)
    args = inputs()
    m.profile(True)
    y0 = m(*args).clone()
    kinds = [op[0] for op in m.profile_ops()]
    m.profile(False)
    assert any(is_path(k) for k in kinds), (case, sorted(set(kinds)))
    # overwrite the source weight through .data (bumps neither version nor pointer) and announce it
    p = dict(m.named_parameters())[wname]
    new = torch.randn(p.shape, generator=torch.Generator().manual_seed(3)) * float(p.std())
    with torch.no_grad():
        p.data.copy_(new)
    m.mark_dirty([wname])
    y1 = m(*args).clone()
    fresh = make().set_precision(prec)
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    y2 = fresh(*args)
    assert not torch.equal(y1, y0) and float((y1 - y0).abs().max()) > 1e-4 * float(y0.abs().max()), case
    assert torch.equal(y1, y2), (case, float((y1 - y2).abs().max()))
