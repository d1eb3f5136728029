"""Shared by the tests that read tests/golden/dit.npz and tests/golden/unet_xattn.npz — fixtures taken from the reference's own
DiT and UNetModel(use_spatial_transformer=True) (gen_dit.py, gen_unet_xattn.py; the reference's two missing imports are served
by tests/golden/ref_standins.py, witnessed in tests/test_pinned_cpu.py): the stored configurations, their regenerated weights
and inputs, and the stored outputs."""
import functools
import json

import torch

import cond_keys_util as U
from util import fixture_params, golden, randn

DIT_FORWARDS = ("d64", "d96", "d72", "d144", "d768")
ST_KEYS = ("st1", "st2", "w160", "w320")     # w160 / w320: heads of 160 / 320 channels, held against the oracle only


@functools.lru_cache(maxsize=None)
def fixture(name):
    return golden(name)


def cfg_of(g, key):
    return json.loads(str(g[key + "_cfg"]))


def names_shapes(g, key):
    return [(n, tuple(s)) for n, s in json.loads(str(g[key + "_params"]))]


def dit_out_channels(kw):
    return kw["in_channels"] // 3 * 2 if kw.get("learn_sigma", True) else kw["in_channels"]


def dit_oracle_kw(kw):
    return dict(patch_size=kw["patch_size"], num_heads=kw["num_heads"], out_channels=dit_out_channels(kw))


def dit_case(key):
    """(constructor keywords, weights, x, cond or None, labels or None, [(tag, t, reference output)])."""
    g = fixture("dit")
    kw = cfg_of(g, key)
    x = randn(tuple(int(v) for v in g[key + "_xshape"]), int(g[key + "_xseed"]))
    cond = randn(tuple(int(v) for v in g[key + "_cshape"]), int(g[key + "_cseed"])) if key + "_cshape" in g.files else None
    y = torch.from_numpy(g[key + "_y"]) if key + "_y" in g.files else None
    runs = [(tag, torch.from_numpy(g[f"{key}_t_{tag}"]), g[f"{key}_out_{tag}"]) for tag in ("int", "float")]
    return kw, fixture_params(g, key), x, cond, y, runs


def st_case(key):
    """(UNetModel keywords, weights, x, context, [(tag, t, reference output)]) of st1 / st2 / w160 / w320."""
    g = fixture("unet_xattn")
    x = randn(tuple(int(v) for v in g[key + "_xshape"]), int(g[key + "_xseed"]))
    ctx = randn(tuple(int(v) for v in g[key + "_cshape"]), int(g[key + "_cseed"]))
    runs = [("int", torch.tensor([999, 17]), g[key + "_out_int"]), ("float", torch.tensor([499.5, 20.0]), g[key + "_out_float"])]
    return cfg_of(g, key), fixture_params(g, key), x, ctx, runs


def cond_case(name):
    """(UNetModel keywords, weights, state x, conditioning dict, [(tag, t, reference output)]) of a cond_keys_util model."""
    g = fixture("unet_xattn")
    hw = tuple(int(v) for v in g[name + "_hw"])
    x = randn((2, U.MODELS[name][1]) + hw, int(g[name + "_xseed"]))
    runs = [("int", torch.tensor([999, 17]), g[name + "_out_int"]), ("float", torch.tensor([499.5, 20.0]), g[name + "_out_float"])]
    return cfg_of(g, name), fixture_params(g, name), x, U.conditioning(name, 2, hw), runs


def wrapped(net, key):
    """DiffusionWrapper.forward's dispatch (ddpm.py:1328-1365) over a callable ``net(x, t, context=None, y=None)``."""
    def forward(x, t, c_concat=None, c_crossattn=None, c_adm=None):
        x_in = torch.cat([x] + c_concat, 1) if key.startswith("hybrid") else x
        if key == "adm":
            return net(x_in, t, y=c_crossattn[0])
        return net(x_in, t, context=torch.cat(c_crossattn, 1), y=c_adm)
    return forward


def oracle_wrapped(name, params, sd):
    return wrapped(lambda x_in, t, context=None, y=None: U.oracle_forward(params, sd, x_in, t, context=context, y=y), U.MODELS[name][0])


def chain_inputs(name):
    """(x_T, conditioning, unconditional conditioning, fed noise [steps, B, ...], steps, eta, scale) of the U-Net chains."""
    g = fixture("unet_xattn")
    steps = int(g["chain_steps"])
    x_T = randn((2, U.MODELS[name][1], 8, 8), int(g["chain_xT_seed"]))
    z = randn((steps,) + tuple(x_T.shape), int(g["chain_noise_seed"]))
    c, u = U.conditioning(name, 2, (8, 8)), U.conditioning(name, 2, (8, 8), seed=int(g["chain_uncond_seed"]))
    return x_T, c, u, z, steps, float(g["chain_eta"]), float(g["chain_scale"])
