"""UNet_disc_Model / SuperResModelNew (the four-stream DisC-Diff denoiser) without a GPU: the parameter table of the native
handle against the reference's state_dict (tests/golden/disc.npz, gen_disc.py), the torch restatement tests/disc_ref.py against
the reference's recorded forwards and chains, the builders, the constructor's refusals and the sampler-side rule for what a
network returned.  No test here reads the reference."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import disc_ref as R
from oracle import samplers as OS
from util import rel_l2

TOL_NET = 2e-6      # the oracle-vs-reference bar of tests/golden/gen_unet_xattn.py / test_pinned_cpu.py
TOL_LOOP = 1e-5

YAML_PARAMS = {     # unet_config.params of the reference's configs/disc-diff.yaml and configs/disc-diff-origin.yaml
    "disc-diff": dict(use_checkpoint=True, image_size=32, in_channels=1, out_channels=1, model_channels=160,
                      attention_resolutions=[16], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_head_channels=32,
                      use_new_attention_order=True),
    "disc-diff-origin": dict(use_checkpoint=True, image_size=32, in_channels=1, out_channels=1, model_channels=96,
                             attention_resolutions=[32, 16, 8], num_res_blocks=2, channel_mult=[1, 1, 2, 2, 3, 3],
                             num_head_channels=48, use_new_attention_order=True),
}


def _table(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def _raw_table(kw):
    """The table of a dsd_create_disc handle made with device = -1, without the Python module."""
    from diffusion_models_dsdiff_amd import _lib
    L = _lib.lib()
    cfg = _lib.DsdConfig()
    cfg.in_channels, cfg.model_channels, cfg.out_channels = kw["in_channels"], kw["model_channels"], kw["out_channels"]
    cfg.n_levels = len(kw["channel_mult"])
    for i, m in enumerate(kw["channel_mult"]):
        cfg.channel_mult[i], cfg.num_res_blocks[i] = m, kw["num_res_blocks"]
    cfg.n_attention_resolutions = len(kw["attention_resolutions"])
    for i, a in enumerate(kw["attention_resolutions"]):
        cfg.attention_resolutions[i] = a
    cfg.num_heads, cfg.num_head_channels, cfg.num_heads_upsample = kw.get("num_heads", 1), kw.get("num_head_channels", -1), -1
    cfg.use_scale_shift_norm, cfg.resblock_updown = int(kw.get("use_scale_shift_norm", False)), int(kw.get("resblock_updown", False))
    cfg.use_new_attention_order = int(kw.get("use_new_attention_order", False))
    h = C.c_void_p()
    _lib.check(L.dsd_create_disc(C.byref(cfg), -1, C.byref(h)))
    got = []
    name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
    for i in range(L.dsd_param_count(h)):
        _lib.check(L.dsd_param_info(h, i, C.byref(name), shape, C.byref(ndim)))
        got.append((name.value.decode(), tuple(shape[k] for k in range(ndim.value))))
    L.dsd_destroy(h)
    return got


@pytest.mark.parametrize("key", R.CONFIGS)
def test_parameter_table_matches_the_reference(key):
    """Names, shapes and ORDER of the reference's state_dict, from the bare handle and from the module built over it."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import SuperResModelNew, UNet_disc_Model
    kw, ref = R.case(key)[0], R.names_shapes(key)
    assert _raw_table(kw) == ref
    m = SuperResModelNew(**kw, device_index=-1)
    assert isinstance(m, UNet_disc_Model) and _table(m) == ref
    with pytest.raises(Exception, match="without a device"):
        m(torch.zeros(1, 4, 8, 8), torch.zeros(1))


@pytest.mark.parametrize("name", sorted(YAML_PARAMS))
def test_yaml_targets_instantiate_and_are_self_consistent(name):
    """Both shipped yamls name Disc_diff.guided_diffusion.unet.UNet_disc_Model; instantiate_from_config resolves it (table only:
    no device) and the table has the structure of unet.py:795-967."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import UNet_disc_Model
    from diffusion_models_dsdiff_amd.ldm.util import instantiate_from_config
    p = YAML_PARAMS[name]
    m = instantiate_from_config({"target": "Disc_diff.guided_diffusion.unet.UNet_disc_Model", "params": dict(p, device_index=-1)})
    assert type(m) is UNet_disc_Model
    sd = dict(_table(m))
    mc, conv_ch = p["model_channels"], p["model_channels"] * p["channel_mult"][-1]
    half = conv_ch // 2
    enc = {k: v for k, v in sd.items() if k.startswith("input_blocks.")}
    assert enc["input_blocks.0.0.weight"] == (mc, 1, 3, 3)
    for sfx in ("_T1", "_T2", "_DWI"):                       # deep copies: the same shapes under their own prefixes
        assert {k.replace("input_blocks" + sfx, "input_blocks"): v for k, v in sd.items() if k.startswith("input_blocks" + sfx + ".")} == enc
    for se in R.SE_NAMES:
        assert sd[se + ".se.0.weight"] == (half // 8, half) and sd[se + ".se.2.weight"] == (half, half // 8)
        assert se + ".se.0.bias" not in sd
    assert sd["dim_reduction_non_zeros.0.weight"] == (conv_ch, int(2.5 * conv_ch), 1, 1)
    assert sd["conv_common.0.weight"] == sd["conv_distinct.0.weight"] == (half, conv_ch, 3, 3)
    assert sd["out.2.weight"] == (1, mc, 3, 3) and sd["time_embed.2.weight"] == (4 * mc, 4 * mc)
    known = ("time_embed.", "input_blocks", "middle_block.", "output_blocks.", "SE_Attention_", "dim_reduction_non_zeros.0.",
             "conv_common.0.", "conv_distinct.0.", "out.")
    assert all(k.startswith(known) for k in sd)
    n_blocks = 1 + sum(p["num_res_blocks"] + (i != len(p["channel_mult"]) - 1) for i in range(len(p["channel_mult"])))
    assert len({k.split(".")[1] for k in enc}) == n_blocks
    heads_dim = p["num_head_channels"]
    assert half % 16 == 0 and conv_ch % heads_dim == 0


@pytest.mark.parametrize("key", R.CONFIGS)
def test_disc_ref_forward_vs_reference(key):
    kw, sd, x, runs = R.case(key)
    for tag, t, want in runs:
        got = R.disc_forward(kw, sd, x, t)
        assert len(got) == 9
        for i, (a, b) in enumerate(zip(got, want)):
            err = rel_l2(a, b)
            print(f"{key} t {tag} output {i}: disc_ref vs reference rel-L2 {err:.3e}")
            assert tuple(a.shape) == b.shape and float(np.abs(b).max()) > 1e-3 and err <= TOL_NET, (key, tag, i, err)
    f64 = R.disc_forward(kw, sd, x, runs[0][1], dtype=torch.float64)
    rec = R.fixture()[key + "_ref_f32_vs_f64"]
    assert f64[8].dtype == torch.float64 and abs(rel_l2(runs[0][2][8], f64[8]) - float(rec[0])) < 2e-7


@pytest.mark.parametrize("name", R.CHAINS)
def test_disc_ref_chain_vs_reference(name):
    key, kw, sd, o, x_T, planes, z, want = R.chain_case(name)
    ora = OS.DiffusionA(steps=1000, timestep_respacing=str(o["steps"]), learn_sigma=o["learn_sigma"], parameterization="eps")
    net = lambda x_in, t: R.disc_forward(kw, sd, x_in, t)[8]
    got = ora.ddim_sample_loop(net, x_T, z, cond=planes, eta=o["eta"]) if o["ddim"] else ora.p_sample_loop(net, x_T, z, cond=planes)
    err = rel_l2(got, want)
    print(f"{name}: disc_ref chain vs reference rel-L2 {err:.3e}")
    assert tuple(got.shape) == want.shape and err <= TOL_LOOP


def test_chains_differ_and_streams_matter():
    g = R.fixture()
    assert rel_l2(g["tiny_ddpm_y"], g["tiny_ddim_y"]) > 1e-2
    kw, sd, x, runs = R.case("tiny")
    swapped = R.disc_forward(kw, sd, x[:, [0, 2, 1, 3]], runs[0][1])[8]
    assert rel_l2(swapped, runs[0][2][8]) > 0.1                 # T1 / T2 are not interchangeable


@pytest.mark.parametrize("learn_sigma", [False, True])
def test_sr_create_model_layout(learn_sigma):
    """script_util.py:90-126: channel_mult (1,1,2,2,3,3), attention at 8 / 16 / 32 whatever the argument says, out_channels
    doubled under learn_sigma."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import script_util as SU
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.respace import SpacedDiffusion
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import SuperResModelNew
    m = SU.sr_create_model(64, 1, 32, 1, learn_sigma=learn_sigma, use_checkpoint=False, attention_resolutions="4", num_heads=2,
                           num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=True, dropout=0, resblock_updown=False,
                           use_fp16=False, device_index=-1)
    assert type(m) is SuperResModelNew and m.channel_mult == (1, 1, 2, 2, 3, 3) and tuple(m.attention_resolutions) == (8, 16, 32)
    sd = dict(_table(m))
    assert m.out_channels == (2 if learn_sigma else 1) and sd["out.2.weight"] == (m.out_channels, 32, 3, 3)
    # one res block per level + a downsample between levels: blocks 1..11; ds 8 / 16 / 32 are levels 3, 4, 5 = blocks 7, 9, 11
    attn = sorted(int(k.split(".")[1]) for k in sd if k.startswith("input_blocks.") and k.endswith(".1.qkv.weight"))
    assert attn == [7, 9, 11]
    assert sd["input_blocks.11.0.emb_layers.1.weight"] == (2 * 96, 128)          # FiLM: scale and shift
    assert sd["conv_common.0.weight"] == (48, 96, 3, 3)
    args = argparse.Namespace(image_size=64, in_channel=1, num_channels=32, num_res_blocks=1, learn_sigma=learn_sigma, use_checkpoint=False,
                              attention_resolutions="4", num_heads=2, num_head_channels=-1, num_heads_upsample=-1,
                              use_scale_shift_norm=True, dropout=0.1, resblock_updown=False, use_fp16=False, diffusion_steps=100,
                              noise_schedule="linear", use_kl=False, predict_xstart=False, rescale_timesteps=False,
                              rescale_learned_sigmas=False, timestep_respacing="10", parameterization="eps")
    with pytest.raises(NotImplementedError):                    # dropout reaches the constructor as in the reference
        SU.sr_create_model_and_diffusion(args)
    args.dropout = 0
    orig = SU.sr_create_model
    SU.sr_create_model = lambda *a, **k: orig(*a, **k, device_index=-1)
    try:
        m2, d = SU.sr_create_model_and_diffusion(args)
    finally:
        SU.sr_create_model = orig
    assert _table(m2) == _table(m) and isinstance(d, SpacedDiffusion) and d.num_timesteps == 10


@pytest.mark.parametrize("bad", [dict(use_fp16=True), dict(dims=3), dict(dropout=0.1), dict(conv_resample=False)])
def test_constructor_rejections(bad):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import UNet_disc_Model
    kw = dict(R.case("tiny")[0], device_index=-1)
    with pytest.raises(NotImplementedError, match="hot path is dims=2, conv_resample=True, dropout=0, fp32"):
        UNet_disc_Model(**dict(kw, **bad))


def test_library_rejections_without_a_device():
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import UNet_disc_Model
    kw = dict(R.case("tiny")[0], device_index=-1)
    with pytest.raises(ValueError, match="in_channels must be 1"):
        UNet_disc_Model(**dict(kw, in_channels=2))
    with pytest.raises(_lib.DsdError, match=r"channel_mult\[0\] = 2"):
        UNet_disc_Model(**dict(kw, channel_mult=[2, 2]))
    m = UNet_disc_Model(**kw)
    with pytest.raises(_lib.DsdError, match="all four encoder streams"):
        m.share_zero_streams(True)
    m.share_zero_streams(False)


def test_se_attention_is_reexported():
    from diffusion_models_dsdiff_amd import blocks
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import unet
    assert unet.SE_Attention is blocks.SE_Attention


def test_nine_tuple_takes_the_last_and_two_tuple_the_first():
    """gaussian_diffusion.py:271-278 of the reference: t1 / t2 / dwi are concatenated behind x and model_output is the NINTH element
    of the network's tuple; DSUnetModel's (out, dict) keeps [0]."""
    from diffusion_models_dsdiff_amd import _sched
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import gaussian_diffusion as gd
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    t9 = tuple(torch.full((1,), float(i)) for i in range(9))
    assert _sched.model_output_of(t9) is t9[8] and _sched.model_output_of((t9[0], {})) is t9[0] and _sched.model_output_of(t9[3]) is t9[3]
    d = create_gaussian_diffusion(steps=100, timestep_respacing="10")
    x, planes = torch.zeros(2, 1, 4, 4), [torch.full((2, 1, 4, 4), float(i + 1)) for i in range(3)]
    seen = {}

    def nine(x_in, t, **kw):
        seen["x"], seen["kw"] = x_in, sorted(kw)
        return tuple(x_in[:, :1] + i for i in range(9))

    out = d._call_model(nine, x, torch.tensor([3, 3]), dict(t1=planes[0], t2=planes[1], dwi=planes[2]))
    assert seen["x"].shape == (2, 4, 4, 4) and [float(seen["x"][0, c, 0, 0]) for c in range(4)] == [0.0, 1.0, 2.0, 3.0]
    assert seen["kw"] == ["dwi", "t1", "t2"] and float(out[0, 0, 0, 0]) == 8.0
    two = lambda x_in, t, **kw: (x_in + 5.0, {"style": []})
    assert float(d._call_model(two, x, torch.tensor([3, 3]), {})[0, 0, 0, 0]) == 5.0
    assert gd.model_output_of is _sched.model_output_of
