"""The KL-VAE's one-head AttnBlock (512 channels at the yaml's size) on both of its routes (GPU): materialised scores, the
default, and one fused attention launch on the wide-head kernels (dsd_set_vae_fused_attention, csrc/attention_wide.hip).

Fixture: the reference's own AttnBlock(512) (tests/golden/wide_heads.npz, gen_wide_heads.py); tolerance 1e-5, the bar of
test_vae_gpu.py.  (The U-Net / DiT fixtures of that file wait for attention() itself to dispatch to the wide kernels; the
oracle is pinned against them in test_wide_heads_cpu.py.)"""
import pytest
import torch

from oracle import vae as V
from oracle.synth import synth_params
from util import golden, fixture_params, rel_l2, randn

pytestmark = pytest.mark.gpu
TOL_VAE = 1e-5


def inputs(g, key):
    x = randn(tuple(int(v) for v in g[key + "_xshape"]), int(g[key + "_xseed"]))
    ctx = randn(tuple(int(v) for v in g[key + "_cshape"]), int(g[key + "_cseed"])) if key + "_cshape" in g.files else None
    return x.cuda(), None if ctx is None else ctx.cuda()


def test_vae_attn_block_golden_both_routes():
    """ldm/modules/diffusionmodules/model.py AttnBlock(512) alone: materialised scores (default) and the fused route."""
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.model import AttnBlock
    g = golden("wide_heads")
    key = "vae_attn_c512"
    m = AttnBlock(512)
    m.load_state_dict(fixture_params(g, key), strict=True)
    x, _ = inputs(g, key)
    out = {}
    for fused in (False, True):
        m.set_fused_attention(fused)
        for prec in ("bf16x6", "f32"):
            m.set_precision(prec)
            y = m(x)
            err = rel_l2(y, g[key + "_y"])
            print(f"AttnBlock(512) fused={fused} {prec}: rel-L2 vs the reference block {err:.3e}")
            assert y.shape == g[key + "_y"].shape and err < TOL_VAE, (fused, prec, err)
            out[fused, prec] = y
    assert not torch.equal(out[True, "f32"], out[False, "f32"])        # two routes, not one (they agree to rounding only)


def test_vae_fused_attention_drops_the_score_buffer():
    """At a 32 x 32 mid map (T = 1024, C = 512) the materialised route's plan holds the T x T scores (4 T^2 bytes), the V
    transpose and, in bf16x6, the split planes; the fused route's holds none of them.  Derived from the allocation."""
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.model import AttnBlock
    T = 32 * 32
    x = randn((1, 512, 32, 32), 770).cuda()
    ws = {}
    for fused in (False, True):
        m = AttnBlock(512)
        m.set_fused_attention(fused)
        y = m(x)
        assert bool(torch.isfinite(y).all())
        ws[fused] = int(_lib.lib().dsd_workspace_bytes(m._h))
    print(f"AttnBlock(512) at 32x32: workspace {ws[False]} B materialised, {ws[True]} B fused")
    assert ws[True] > 0 and ws[False] - ws[True] >= 4 * T * T, ws


VAE_DD = dict(double_z=True, z_channels=4, resolution=32, in_channels=1, out_ch=1, ch=32, ch_mult=[1, 2, 4], num_res_blocks=1,
              attn_resolutions=[8], dropout=0.0)


def test_autoencoder_kl_encode_decode_both_routes_vs_oracle():
    """Two small AutoencoderKLs, encode -> decode against oracle/vae.py on the default route and on the fused route: AttnBlocks
    (level 2 and mid, 8 x 8) of 128 channels — one head at the narrow kernels' limit — and of 256 channels, the wide kernels."""
    from diffusion_models_dsdiff_amd.ldm.models.autoencoder import AutoencoderKL
    for dd, embed in ((VAE_DD, 4), (dict(VAE_DD, ch=64, ch_mult=[1, 2, 4]), 4)):      # AttnBlocks of 128 / 256 channels
        m = AutoencoderKL(dd, None, embed)
        sd = synth_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 780)
        m.load_state_dict(sd, strict=True)
        vc = V.VaeConfig(**dd, embed_dim=embed)
        x = randn((2, 1, 32, 32), 781)
        mo = V.encode(vc, sd, x)
        z = mo[:, :embed]                                                           # the posterior's mode
        yo = V.decode(vc, sd, z)
        for fused in (False, True):
            m.set_fused_attention(fused)
            for prec in ("bf16x6", "f32"):
                m.set_precision(prec)
                post = m.encode(x.cuda())
                e1 = rel_l2(post.parameters, mo)
                e2 = rel_l2(m.decode(z.cuda()), yo)
                print(f"AutoencoderKL ch={dd['ch']} fused={fused} {prec}: encode rel-L2 {e1:.3e}, decode rel-L2 {e2:.3e}")
                assert e1 < TOL_VAE and e2 < TOL_VAE, (dd["ch"], fused, prec, e1, e2)
