"""What the reference's own DiT and UNetModel(use_spatial_transformer=True) computed, held against the oracle without a GPU
(tests/golden/dit.npz, tests/golden/unet_xattn.npz: gen_dit.py, gen_unet_xattn.py), and the witness of the import stand-ins those
generators ran the reference through (tests/golden/ref_standins.py).

The reference imports timm (PatchEmbed, Attention, Mlp) for its DiT and omegaconf (one ``type(x) == ListConfig`` test) for its
transformer U-Net; the build image has neither, so the generators install stand-ins.  The fixtures are the reference's code
from end to end EXCEPT those three small modules, so the modules are checked here against code that is not the project's:
nn.MultiheadAttention, F.unfold and F.gelu, in float64, to 1e-12 absolute (float64 arithmetic on O(1) values).  No test here
reads the reference."""
import ctypes as C
import hashlib
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cond_keys_util as U
import pinned_util as P
from oracle import dit as OD, samplers as OS, unet as O
from util import GOLDEN, fixture_params, randn, rel_l2

TOL_NET = 2e-6      # the oracle-vs-reference bars of test_oracle_golden.py
TOL_LOOP = 1e-5
WITNESS = 1e-12


def standins():
    spec = importlib.util.spec_from_file_location("ref_standins", os.path.join(GOLDEN, "ref_standins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------- 1. the stand-ins' witness
@pytest.mark.parametrize("dim,heads,tokens", [(64, 4, 64), (72, 3, 27), (144, 2, 50), (96, 3, 9)])
def test_standin_attention_is_multihead_attention(dim, heads, tokens):
    """27, 50 and 9 tokens are no multiple of 4; head dims 16, 24, 72, 32."""
    R = standins()
    torch.manual_seed(dim + tokens)
    a = R.Attention(dim, num_heads=heads, qkv_bias=True).double()
    for p in a.parameters():
        torch.nn.init.normal_(p, std=dim ** -0.5 if p.dim() == 2 else 0.1)
    mha = torch.nn.MultiheadAttention(dim, heads, bias=True, batch_first=True).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(a.qkv.weight)
        mha.in_proj_bias.copy_(a.qkv.bias)
        mha.out_proj.weight.copy_(a.proj.weight)
        mha.out_proj.bias.copy_(a.proj.bias)
        x = torch.randn(3, tokens, dim, dtype=torch.float64)
        got, want = a(x), mha(x, x, x, need_weights=False)[0]
    err = float((got - want).abs().max())
    print(f"Attention({dim}, {heads}) on {tokens} tokens vs nn.MultiheadAttention: max abs {err:.2e}")
    assert float(want.abs().max()) > 0.1 and err < WITNESS
    assert [n for n, _ in a.named_parameters()] == ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias"]


@pytest.mark.parametrize("size,patch,cin,dim", [(16, 2, 4, 64), (6, 2, 4, 72), (32, 8, 3, 96)])
def test_standin_patch_embed_is_unfold_and_matmul(size, patch, cin, dim):
    R = standins()
    torch.manual_seed(size)
    pe = R.PatchEmbed(size, patch, cin, dim, bias=True).double()
    with torch.no_grad():
        x = torch.randn(2, cin, size, size, dtype=torch.float64)
        want = F.unfold(x, patch, stride=patch).transpose(1, 2) @ pe.proj.weight.reshape(dim, -1).T + pe.proj.bias
        got = pe(x)
    err = float((got - want).abs().max())
    print(f"PatchEmbed({size}, {patch}, {cin}, {dim}) vs unfold @ W^T + b: max abs {err:.2e}")
    assert got.shape == (2, (size // patch) ** 2, dim) and float(want.abs().max()) > 0.1 and err < WITNESS
    assert pe.patch_size == (patch, patch) and pe.grid_size == (size // patch,) * 2 and pe.num_patches == (size // patch) ** 2
    assert isinstance(pe.norm, torch.nn.Identity) and [n for n, _ in pe.named_parameters()] == ["proj.weight", "proj.bias"]


def test_standin_mlp_is_fc2_gelu_tanh_fc1():
    R = standins()
    torch.manual_seed(3)
    mlp = R.Mlp(in_features=72, hidden_features=288, act_layer=lambda: torch.nn.GELU(approximate="tanh"), drop=0).double()
    with torch.no_grad():
        x = torch.randn(5, 27, 72, dtype=torch.float64)
        h = x @ mlp.fc1.weight.T + mlp.fc1.bias
        want = (0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))) @ mlp.fc2.weight.T + mlp.fc2.bias
        got = mlp(x)
    err = float((got - want).abs().max())
    print(f"Mlp(72, 288) vs fc2(gelu_tanh(fc1(x))) written out: max abs {err:.2e}")
    assert float(want.abs().max()) > 0.1 and err < WITNESS
    assert [n for n, _ in mlp.named_parameters()] == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


def test_standin_listconfig_and_install():
    import sys
    R = standins()
    assert issubclass(R.ListConfig, list) and list(R.ListConfig([24])) == [24] and type(R.ListConfig([24])) is not list
    keep = {k: sys.modules.get(k) for k in ("omegaconf", "omegaconf.listconfig", "timm", "timm.models", "timm.models.vision_transformer")}
    try:
        R.install()
        from omegaconf.listconfig import ListConfig
        from timm.models.vision_transformer import PatchEmbed, Attention, Mlp
        assert (ListConfig, PatchEmbed, Attention, Mlp) == (R.ListConfig, R.PatchEmbed, R.Attention, R.Mlp)
    finally:
        for k, v in keep.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


# ---------------------------------------------------------------------------------------- 2. the DiT
@pytest.mark.parametrize("key", P.DIT_FORWARDS)
def test_oracle_dit_forward_vs_reference(key):
    kw, sd, x, cond, y, runs = P.dit_case(key)
    x_in = x if cond is None else torch.cat([x, cond], 1)
    for tag, t, want in runs:
        got = OD.dit_forward(sd, x_in, t, y, **P.dit_oracle_kw(kw))
        err = rel_l2(got, want)
        print(f"{key} t {tag}: oracle vs reference DiT rel-L2 {err:.3e}")
        assert got.shape == want.shape and float(np.abs(want).max()) > 1e-3 and err < TOL_NET, (key, tag, err)


def test_oracle_forward_with_cfg_vs_reference():
    g = P.fixture("dit")
    kw, sd = P.cfg_of(g, "cfg"), fixture_params(g, "cfg")
    x, t, y, s = randn((4, 6, 16, 16), int(g["cfg_xseed"])), torch.from_numpy(g["cfg_t"]), torch.from_numpy(g["cfg_y"]), float(g["cfg_scale"])
    assert int(y.max()) == kw["num_classes"] and s == 2.5                  # the null label rides in the second half
    full = OD.dit_forward(sd, torch.cat([x[:2], x[:2]]), t, y, **P.dit_oracle_kw(kw))
    eps = full[2:, :3] + s * (full[:2, :3] - full[2:, :3])
    got = torch.cat([torch.cat([eps, eps]), full[:, 3:]], 1)
    err = rel_l2(got, g["cfg_out"])
    print(f"forward_with_cfg: oracle composition vs reference rel-L2 {err:.3e}")
    assert got.shape == g["cfg_out"].shape and err < TOL_NET


def test_sincos_tables_are_the_references():
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import get_2d_sincos_pos_embed
    g = P.fixture("dit")
    digests = json.loads(str(g["pe_sha256"]))
    assert set(digests) == {"64_8", "96_8", "72_3", "144_16", "768_4", "1152_16"}
    stored = 0
    for k, digest in digests.items():
        D, grid = (int(v) for v in k.split("_"))
        tab = get_2d_sincos_pos_embed(D, grid)
        assert tab.dtype == np.float64 and tab.shape == (grid * grid, D)
        assert hashlib.sha256(np.ascontiguousarray(tab).tobytes()).hexdigest() == digest, k
        if "pe_" + k in g.files:
            stored += 1
            assert np.array_equal(tab, g["pe_" + k]), k
    assert stored >= 4
    assert np.array_equal(g["fresh_pos_embed"][0], get_2d_sincos_pos_embed(64, 8).astype(np.float32))


def _table(kind, ia):
    from diffusion_models_dsdiff_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.dsd_block_create(kind, (C.c_int32 * len(ia))(*[int(v) for v in ia]), len(ia), -1, C.byref(h)))
    got = []
    name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
    for i in range(L.dsd_param_count(h)):
        _lib.check(L.dsd_param_info(h, i, C.byref(name), shape, C.byref(ndim)))
        got.append((name.value.decode(), tuple(shape[k] for k in range(ndim.value))))
    L.dsd_destroy(h)
    return got


def test_dit_parameter_table_matches_the_reference():
    """A table-only DSD_BLOCK_DIT handle (device = -1) of d64 carries exactly the names and shapes of the reference DiT's
    state_dict, the label table with its classifier-free row among them.  (The order differs in one place, which no
    load_state_dict reads: the reference lists pos_embed, the DiT module's own parameter, first.)"""
    from diffusion_models_dsdiff_amd import _lib
    g = P.fixture("dit")
    kw = P.cfg_of(g, "d64")
    ia = [kw["input_size"], kw["patch_size"], kw["in_channels"], kw["hidden_size"], kw["depth"], kw["num_heads"],
          int(kw["hidden_size"] * 4.0), kw["num_classes"], 1, 1]
    got, ref = _table(_lib.BLOCK_DIT, ia), P.names_shapes(g, "d64")
    assert dict(got) == dict(ref) and len(got) == len(ref) and dict(got)["y_embedder.embedding_table.weight"] == (11, 64)
    assert [n for n, _ in got if n != "pos_embed"] == [n for n, _ in ref if n != "pos_embed"]


@pytest.mark.parametrize("key", list(P.ST_KEYS) + sorted(U.MODELS))
def test_transformer_unet_parameter_table_matches_the_reference(key):
    """Table-only DSD_BLOCK_UNET handles: the reference's names and shapes in the reference's order, so weights drawn from one
    seed over either list are the same tensors (the GPU tests of the six conditioning-key models rely on it)."""
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import unet_iargs
    g = P.fixture("unet_xattn")
    got, ref = _table(_lib.BLOCK_UNET, unet_iargs(**P.cfg_of(g, key))), P.names_shapes(g, key)
    assert dict(got) == dict(ref) and [n for n, _ in got] == [n for n, _ in ref]


def test_oracle_dit_chain_vs_reference():
    """The reference's DDIMSampler over its DiT (dit_loops_util's M3 layout), 4 steps, eta 0 and eta 0.5 with fed noise."""
    import dit_loops_util as D
    g = P.fixture("dit")
    kw, sd = P.cfg_of(g, "chain"), fixture_params(g, "chain")
    assert kw == D.MODELS["M3"][0]                                         # the fixture's live twin
    steps = int(g["chain_steps"])
    x_T = randn((2, 3, 16, 16), int(g["chain_xT_seed"]))
    net = lambda x, t: OD.dit_forward(sd, x, t.float(), None, **P.dit_oracle_kw(kw))
    for key in ("chain_eta0", "chain_eta05"):
        z = randn((steps,) + tuple(x_T.shape), int(g[key + "_noise_seed"]))
        got = OS.DiffusionB(parameterization="eps").ddim_sample(net, steps, x_T, z, None, eta=float(g[key + "_eta"]))
        err = rel_l2(got, g[key + "_y"])
        print(f"DiT {key}: oracle chain vs reference rel-L2 {err:.3e}")
        assert got.shape == g[key + "_y"].shape and err < TOL_LOOP
    assert rel_l2(g["chain_eta05_y"], g["chain_eta0_y"]) > 1e-2            # the fed noise arrived


# ---------------------------------------------------------------------------------------- 3. the transformer U-Net
@pytest.mark.parametrize("key", P.ST_KEYS)
def test_oracle_transformer_unet_vs_reference(key):
    params, sd, x, ctx, runs = P.st_case(key)
    cfg = O.UNetConfig.from_params(params)
    for tag, t, want in runs:
        got = O.plain_unet_forward(cfg, sd, x, t, context=ctx)
        err = rel_l2(got, want)
        print(f"{key} t {tag}: oracle vs reference UNetModel rel-L2 {err:.3e}")
        assert got.shape == want.shape and err < TOL_NET, (key, tag, err)


def test_fixture_configurations_are_the_live_tests():
    """st1 / st2 are tests/test_latent_gpu.py::ST_CFGS with its inputs, the six models are cond_keys_util's: each fixture has a
    live twin running against the oracle."""
    from test_latent_gpu import ST_CFGS
    g = P.fixture("unet_xattn")
    for key in ("st1", "st2"):
        params, shp, ntok = ST_CFGS[key]
        assert P.cfg_of(g, key) == params and tuple(g[key + "_xshape"]) == shp and int(g[key + "_cshape"][1]) == ntok
        assert (int(g[key + "_seed"]), int(g[key + "_xseed"]), int(g[key + "_cseed"])) == (410, 411, 412)
    for name in U.MODELS:
        assert P.cfg_of(g, name) == U.unet_params(name) and int(g[name + "_seed"]) == U.WEIGHT_SEED
    assert tuple(g["crossattn5_hw"]) == (5, 5)
    for key, d in (("w160", 160), ("w320", 320)):                          # one head as wide as the attention level
        shapes = dict(P.names_shapes(g, key))
        assert shapes["middle_block.1.transformer_blocks.0.attn1.to_q.weight"] == (d, d) and P.cfg_of(g, key)["num_heads"] == 1


@pytest.mark.parametrize("name", sorted(U.MODELS))
def test_oracle_conditioning_key_models_vs_reference(name):
    params, sd, x, c, runs = P.cond_case(name)
    net = P.oracle_wrapped(name, params, sd)
    for tag, t, want in runs:
        got = net(x, t, **c)
        err = rel_l2(got, want)
        print(f"{name} t {tag}: oracle vs reference UNetModel rel-L2 {err:.3e}")
        assert got.shape == want.shape and err < TOL_NET, (name, tag, err)


@pytest.mark.parametrize("name", ["crossattn", "hybrid"])
def test_oracle_unet_chains_vs_reference(name):
    """The reference's DDIMSampler, 4 steps, eta 0.5, fed noise; unguided and at scale 3.0 against another conditioning."""
    g = P.fixture("unet_xattn")
    params, sd = P.cfg_of(g, name), fixture_params(g, name)
    x_T, c, u, z, steps, eta, scale = P.chain_inputs(name)
    ora = P.oracle_wrapped(name, params, sd)
    plain = lambda x, t: ora(x, t, **c)
    guided = lambda x, t: ora(x, t, **u) + scale * (ora(x, t, **c) - ora(x, t, **u))      # ddim.py:194-219
    for tag, net in (("plain", plain), ("guided", guided)):
        got = OS.DiffusionB(parameterization="eps").ddim_sample(net, steps, x_T, z, None, eta=eta)
        want = g[f"{name}_chain_{tag}_y"]
        err = rel_l2(got, want)
        print(f"{name} chain {tag}: oracle vs reference rel-L2 {err:.3e}")
        assert got.shape == want.shape and err < TOL_LOOP, (name, tag, err)
    assert rel_l2(g[name + "_chain_guided_y"], g[name + "_chain_plain_y"]) > 1e-2          # the scale is not ignored
