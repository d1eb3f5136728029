"""Cross-attention and vector conditioning, host side (no GPU): the label_emb parameter tables against the reference's, the
oracle helper of the GPU tests against the reference fixture, DiffusionWrapper's dispatch of the seven conditioning keys, and
the Conditioning / Guidance objects the device loops are driven with (tests/golden/cond_keys.npz: gen_cond_keys.py)."""
import ctypes as C
import json

import pytest
import torch

import cond_keys_util as U
from util import fixture_params, golden, randn, rel_l2


def _table(params):
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import unet_iargs
    L = _lib.lib()
    ia = [int(v) for v in unet_iargs(**params)]
    h = C.c_void_p()
    _lib.check(L.dsd_block_create(_lib.BLOCK_UNET, (C.c_int32 * len(ia))(*ia), len(ia), -1, C.byref(h)))
    got = []
    name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
    for i in range(L.dsd_param_count(h)):
        _lib.check(L.dsd_param_info(h, i, C.byref(name), shape, C.byref(ndim)))
        got.append((name.value.decode(), tuple(shape[k] for k in range(ndim.value))))
    L.dsd_destroy(h)
    return got


@pytest.mark.parametrize("key", ["cls", "cont", "seq", "adm"])
def test_label_emb_parameter_tables_match_the_reference(key):
    """Table-only DSD_BLOCK_UNET handles: names and shapes of the reference UNetModel's state_dict for the three label_emb
    forms, label_emb.* right behind time_embed.* as the reference declares them."""
    g = golden("cond_keys")
    ref = [(n, tuple(s)) for n, s in json.loads(str(g[key + "_params"]))]
    got = _table(json.loads(str(g[key + "_cfg"])))
    assert dict(got) == dict(ref)
    assert [n for n, _ in got] == [n for n, _ in ref]
    labels = [n for n, _ in got if n.startswith("label_emb.")]
    assert labels == {"cls": ["label_emb.weight"], "adm": ["label_emb.weight"], "cont": ["label_emb.weight", "label_emb.bias"],
                      "seq": ["label_emb.0.0.weight", "label_emb.0.0.bias", "label_emb.0.2.weight", "label_emb.0.2.bias"]}[key]


def test_argument_lists_of_today_are_unchanged():
    """No label and no spatial transformer: the handle's integers end with the attention resolutions, as before; a label
    without a transformer spells the transformer's four integers as off."""
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import unet_iargs
    g = golden("cond_keys")
    p = json.loads(str(g["cls_cfg"]))
    plain = {k: v for k, v in p.items() if k != "num_classes"}
    base = unet_iargs(**plain)
    assert base[-2:] == [1, 2] and len(base) == 11 + 2 + 2 + 1 + 1
    assert unet_iargs(**p) == base + [0, 1, 0, 0, 1, 7]
    assert unet_iargs(**dict(plain, num_classes="continuous")) == base + [0, 1, 0, 0, 2, 1]
    assert unet_iargs(**dict(plain, num_classes="sequential", adm_in_channels=12)) == base + [0, 1, 0, 0, 3, 12]
    st = dict(plain, use_spatial_transformer=True, context_dim=24)
    assert unet_iargs(**dict(st, num_classes=7)) == unet_iargs(**st) + [1, 7]
    no_label = dict(_table(plain))
    assert not any(n.startswith("label_emb") for n in no_label)
    assert {n: s for n, s in _table(p) if not n.startswith("label_emb")} == no_label


@pytest.mark.parametrize("key", ["cls", "cont", "seq"])
def test_oracle_helper_equals_the_reference_forward(key):
    """The helper the GPU tests compare 'hybrid-adm' against restates UNetModel.forward with emb + label_emb(y): on the
    fixture's networks it gives the reference's own outputs (fp32 on both sides: 1e-5 covers the conv re-association)."""
    g = golden("cond_keys")
    params = json.loads(str(g[key + "_cfg"]))
    sd = fixture_params(g, key)
    x = randn(tuple(int(v) for v in g[key + "_xshape"]), int(g[key + "_seed"]) + 1)
    y = torch.from_numpy(g[key + "_y"])
    for t, want in ((torch.tensor([999, 17]), g[key + "_out_int"]), (torch.tensor([499.5, 20.0]), g[key + "_out_float"])):
        assert rel_l2(U.oracle_forward(params, sd, x, t, y=y), want) < 1e-5


def _wrapper(key):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    return DiffusionWrapper({"target": "cond_keys_util.Recorder", "params": {}}, key)


def test_diffusion_wrapper_dispatches_all_seven_keys():
    """ddpm.py:1328-1365 onto a recording stand-in."""
    x, t = randn((2, 4, 8, 8), 1), torch.tensor([5, 6])
    cc, ca, cb, adm = randn((2, 2, 8, 8), 2), randn((2, 5, 24), 3), randn((2, 3, 24), 4), randn((2, 12), 5)
    seen = lambda w: w.diffusion_model.calls[-1]
    w = _wrapper(None)
    w(x, t)
    assert torch.equal(seen(w)["x"], x) and seen(w)["context"] is None and seen(w)["y"] is None
    w = _wrapper("concat")
    w(x, t, c_concat=[cc, cc])
    assert torch.equal(seen(w)["x"], torch.cat([x, cc, cc], 1)) and seen(w)["context"] is None and seen(w)["y"] is None
    w = _wrapper("crossattn")
    w(x, t, c_crossattn=[ca, cb])
    assert torch.equal(seen(w)["x"], x) and torch.equal(seen(w)["context"], torch.cat([ca, cb], 1)) and seen(w)["y"] is None
    assert seen(w)["context"].shape == (2, 8, 24)                                      # lists join along the tokens
    w = _wrapper("hybrid")
    w(x, t, c_concat=[cc], c_crossattn=[ca])
    assert torch.equal(seen(w)["x"], torch.cat([x, cc], 1)) and torch.equal(seen(w)["context"], ca) and seen(w)["y"] is None
    w = _wrapper("hybrid-adm")
    w(x, t, c_concat=[cc], c_crossattn=[ca], c_adm=adm)
    assert torch.equal(seen(w)["x"], torch.cat([x, cc], 1)) and torch.equal(seen(w)["context"], ca) and torch.equal(seen(w)["y"], adm)
    with pytest.raises(AssertionError):
        w(x, t, c_concat=[cc], c_crossattn=[ca])
    w = _wrapper("crossattn-adm")
    w(x, t, c_crossattn=[ca], c_adm=adm)
    assert torch.equal(seen(w)["x"], x) and torch.equal(seen(w)["context"], ca) and torch.equal(seen(w)["y"], adm)
    w = _wrapper("adm")
    w(x, t, c_crossattn=[adm])
    assert torch.equal(seen(w)["x"], x) and seen(w)["context"] is None and torch.equal(seen(w)["y"], adm)
    with pytest.raises(AssertionError):
        _wrapper("film")
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    with pytest.raises(NotImplementedError, match="transformer_depth > 1"):
        DiffusionWrapper({"target": "cond_keys_util.Recorder", "params": {}, "sequential_crossattn": True}, "crossattn")


def test_concat_only_inputs_give_what_they_gave():
    """Tensors, lists and c_concat-only dicts: one [B,Cc,H,W] tensor, with or without the key spelled out."""
    from diffusion_models_dsdiff_amd import _sched as S
    a, b = randn((2, 2, 8, 8), 1), randn((2, 1, 8, 8), 2)
    for c, want in ((a, a), ([a, b], torch.cat([a, b], 1)), ({"c_concat": [a, b]}, torch.cat([a, b], 1)), ({"c_concat": a}, a)):
        for key in (None, "concat"):
            got = S.cat_conditioning(c, "cpu", key)
            assert torch.is_tensor(got) and torch.equal(got, want)
    u = S.cat_unconditional({"c_concat": [a, b]}, {"c_concat": [a * 0 + 1, b]}, "cpu")
    assert torch.is_tensor(u) and u.shape == (2, 3, 8, 8)
    g = S.Guidance(u, 3.0, 4)
    g.check(torch.cat([a, b], 1), 4)
    assert list(g.scale) == [3.0] * 4
    with pytest.raises(AssertionError, match="lacks the key 'c_concat'"):
        S.cat_unconditional({"c_concat": [a]}, {}, "cpu")


def test_conditioning_from_dicts_lists_and_tensors():
    from diffusion_models_dsdiff_amd import _sched as S
    cc, ca, cb, adm = randn((2, 2, 8, 8), 2), randn((2, 5, 24), 3), randn((2, 3, 24), 4), randn((2, 12), 5)
    full = {"c_concat": [cc], "c_crossattn": [ca, cb], "c_adm": adm}
    ctx = torch.cat([ca, cb], 1)
    # the key read off the dict's entries, and spelled out
    assert S.cat_conditioning(full, "cpu") == S.Conditioning(cc, ctx, adm) == S.cat_conditioning(full, "cpu", "hybrid-adm")
    # c_concat only where the key has it (the trainer's dict carries all three whatever the key)
    assert S.cat_conditioning(full, "cpu", "crossattn-adm") == S.Conditioning(None, ctx, adm)
    assert S.cat_conditioning(full, "cpu", "crossattn") == S.Conditioning(None, ctx, None)
    assert S.cat_conditioning(full, "cpu", "hybrid") == S.Conditioning(cc, ctx, None)
    assert torch.equal(S.cat_conditioning(full, "cpu", "concat"), cc)
    assert S.cat_conditioning({"c_crossattn": [adm]}, "cpu", "adm") == S.Conditioning(None, None, adm)
    # a tensor or a list under another key than 'concat' is c_crossattn (apply_model)
    assert S.cat_conditioning(ca, "cpu", "crossattn") == S.Conditioning(None, ca, None)
    assert S.cat_conditioning([ca, cb], "cpu", "crossattn") == S.Conditioning(None, ctx, None)
    assert S.cat_conditioning(adm, "cpu", "adm") == S.Conditioning(None, None, adm)
    assert S.Conditioning(cc, ctx, adm) != S.Conditioning(cc, ctx, adm + 1)
    # model_kwargs of the bare network
    kw = S.kwargs_conditioning(None, None, dict(c_concat=[cc], context=ctx, y=adm), "cpu")
    assert kw == S.Conditioning(cc, ctx, adm)
    assert S.kwargs_conditioning(None, None, dict(c_concat=[cc]), "cpu") is None


def test_malformed_conditionings_name_the_key():
    from diffusion_models_dsdiff_amd import _sched as S
    cc, ca, adm = randn((2, 2, 8, 8), 2), randn((2, 5, 24), 3), randn((2, 12), 5)
    with pytest.raises(ValueError, match="lacks 'c_crossattn'.*'hybrid'"):
        S.cat_conditioning({"c_concat": [cc]}, "cpu", "hybrid")
    with pytest.raises(ValueError, match="lacks 'c_concat'.*'hybrid'"):
        S.cat_conditioning({"c_crossattn": [ca]}, "cpu", "hybrid")
    with pytest.raises(ValueError, match="lacks 'c_adm'.*'crossattn-adm'"):
        S.cat_conditioning({"c_crossattn": [ca]}, "cpu", "crossattn-adm")
    with pytest.raises(ValueError, match="lacks 'c_crossattn'.*'adm'"):
        S.cat_conditioning({"c_adm": adm}, "cpu", "adm")
    with pytest.raises(ValueError, match=r"'c_crossattn'.*\[B, tokens, context_dim\]"):
        S.cat_conditioning({"c_crossattn": [adm]}, "cpu", "crossattn")
    with pytest.raises(ValueError, match="'c_adm'.*one tensor"):
        S.cat_conditioning({"c_crossattn": [ca], "c_adm": [adm, adm]}, "cpu", "crossattn-adm")
    with pytest.raises(ValueError, match="cannot tell the conditioning key"):
        S.cat_conditioning({"c_adm": adm}, "cpu")
    with pytest.raises(ValueError, match="'film'"):
        S.cat_conditioning({"c_crossattn": [ca]}, "cpu", "film")
    with pytest.raises(ValueError, match="model_kwargs \\['labels'\\]"):
        S.kwargs_conditioning(None, None, dict(context=ca, labels=adm), "cpu")


def test_guidance_pairs_the_parts_key_by_key():
    """ddim.py:199-217: the unconditional dict mirrors the conditioning key by key and list element by list element; a twin
    equal to the conditional part is legal (the reference's c_adm)."""
    from diffusion_models_dsdiff_amd import _sched as S
    cc, ca, cb, adm = randn((2, 2, 8, 8), 2), randn((2, 5, 24), 3), randn((2, 3, 24), 4), randn((2, 12), 5)
    c = {"c_concat": [cc], "c_crossattn": [ca, cb], "c_adm": adm}
    u = {"c_concat": [cc], "c_crossattn": [ca * 0, cb * 0], "c_adm": adm}
    cond, unc = S.cat_conditioning(c, "cpu", "hybrid-adm"), S.cat_unconditional(c, u, "cpu", "hybrid-adm")
    assert unc == S.Conditioning(cc, torch.zeros(2, 8, 24), adm)
    g = S.Guidance(unc, [1.0, 2.0, 3.0], 3)
    g.check(cond, 3)
    assert list(g.scale) == [1.0, 2.0, 3.0]
    with pytest.raises(AssertionError, match="lacks the key 'c_adm'"):
        S.cat_unconditional(c, {k: v for k, v in u.items() if k != "c_adm"}, "cpu", "hybrid-adm")
    with pytest.raises(AssertionError, match=r"\['c_crossattn'\] must be a list of 2"):
        S.cat_unconditional(c, dict(u, c_crossattn=[ca]), "cpu", "hybrid-adm")
    with pytest.raises(AssertionError, match="must be a dict"):
        S.cat_unconditional(c, ca, "cpu", "hybrid-adm")
    with pytest.raises(ValueError, match="'c_adm'.*twin"):
        S.Guidance(S.Conditioning(cc, unc.context, None), 2.0, 3).check(cond, 3)
    with pytest.raises(ValueError, match="unconditional 'c_crossattn' must have the shape"):
        S.Guidance(S.Conditioning(cc, unc.context[:, :5], adm), 2.0, 3).check(cond, 3)
    with pytest.raises(ValueError, match="form of the conditioning"):
        S.Guidance(cc, 2.0, 3).check(cond, 3)
    with pytest.raises(ValueError, match="3 scales .* 4 steps"):
        g.check(cond, 4)
    # Cc = 0: nothing to point the C struct's uncond at
    g0 = S.Guidance(S.Conditioning(None, unc.context, None), 2.0, 3)
    assert g0.bind().uncond is None


def test_latent_diffusion_accepts_the_keys_and_unet_keeps_raising_for_n_embed():
    from diffusion_models_dsdiff_amd.ldm.models.diffusion import ddpm
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel, label_emb_kind
    assert ddpm.CONDITIONING_KEYS == (None, "concat", "crossattn", "hybrid", "adm", "hybrid-adm", "crossattn-adm")
    assert label_emb_kind(None) == (0, 0) and label_emb_kind(7) == (1, 7) and label_emb_kind("continuous") == (2, 1)
    assert label_emb_kind("sequential", 12) == (3, 12)
    with pytest.raises(AssertionError):
        label_emb_kind("sequential")
    with pytest.raises(ValueError):
        label_emb_kind("film")
    with pytest.raises(NotImplementedError, match="n_embed"):
        UNetModel(8, 4, 32, 4, 1, [2], channel_mult=[1, 2], num_head_channels=16, n_embed=16)
