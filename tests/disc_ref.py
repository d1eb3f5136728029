"""UNet_disc_Model.forward (Disc_diff/guided_diffusion/unet.py:985-1044 of the reference) restated in torch from oracle.unet's
building blocks, state-dict driven, in float32 or float64, on any device; tests/golden/disc.npz (gen_disc.py) pins it to the
reference's own code.  Also the bottleneck head alone (:1015-1033) on pre-activation convolution outputs, the float64 yardstick
of the dsd_op_disc_bottleneck tests, and the fixture's cases."""
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet as O
from oracle.synth import randn
from util import fixture_params, golden

STREAMS = ("", "_T1", "_T2", "_DWI")
SE_NAMES = ("SE_Attention_com", "SE_Attention_dist_1", "SE_Attention_dist_2", "SE_Attention_dist_3", "SE_Attention_dist_4")
CONFIGS = ("tiny", "film", "odd")
CHAINS = ("tiny_ddim", "tiny_ddpm", "film_ddpm")


def unet_config(kw):
    """oracle.unet.UNetConfig of UNet_disc_Model's keywords: the AttentionBlock(num_heads, num_head_channels) head rule is what
    the oracle's spec builder applies under ``legacy``."""
    keys = O.UNetConfig.__dataclass_fields__.keys()
    d = {k: v for k, v in kw.items() if k in keys}
    d.setdefault("num_heads", 1)                      # UNet_disc_Model's default (unet.py:768)
    return O.UNetConfig(**d, legacy=True)


def se_gate(x, w1, w2):
    """SE_Attention.forward (unet.py:105-109)."""
    y = torch.sigmoid(F.linear(F.relu(F.linear(x.mean(dim=(2, 3)), w1)), w2))
    return x * y[:, :, None, None]


def bottleneck(com_pre, dist_pre, w1, w2):
    """com_pre / dist_pre: four NCHW pre-activation outputs each; w1 / w2: five SE weight pairs (com, dist_1..4).
    Returns (cat [B,5*half,h,w], [com_h1..4, dist_h1..4])."""
    com = [F.silu(c) for c in com_pre]
    dist = [se_gate(F.silu(d), w1[1 + i], w2[1 + i]) for i, d in enumerate(dist_pre)]
    com_h = se_gate(torch.mean(torch.stack(com), dim=0), w1[0], w2[0])
    return torch.cat([com_h] + dist, dim=1), com + dist


class _DiscNet(O._Net):
    """oracle.unet._Net in the dtype of the state dict (the oracle's GroupNorm and softmax force float32)."""

    def gn(self, name, x):
        return F.group_norm(x, 32, self.p(name + ".weight"), self.p(name + ".bias"), 1e-5)

    def attn(self, prefix, L, x):
        b, c, hh, ww = x.shape
        xf = x.reshape(b, c, -1)
        qkv = F.conv1d(self.gn(prefix + ".norm", xf), self.p(prefix + ".qkv.weight"), self.p(prefix + ".qkv.bias"))
        n_heads, new_order = L["heads"], self.cfg.use_new_attention_order
        bs, width, length = qkv.shape
        ch = width // (3 * n_heads)
        scale = 1 / math.sqrt(math.sqrt(ch))
        if new_order:                                                            # QKVAttention :537-555
            q, k, v = qkv.chunk(3, dim=1)
            q, k, v = (q * scale).reshape(bs * n_heads, ch, length), (k * scale).reshape(bs * n_heads, ch, length), v.reshape(bs * n_heads, ch, length)
        else:                                                                    # QKVAttentionLegacy :505-521
            q, k, v = qkv.reshape(bs * n_heads, ch * 3, length).split(ch, dim=1)
            q, k = q * scale, k * scale
        w = torch.softmax(torch.einsum("bct,bcs->bts", q, k), dim=-1)
        a = torch.einsum("bts,bcs->bct", w, v).reshape(bs, -1, length)
        a = F.conv1d(a, self.p(prefix + ".proj_out.weight"), self.p(prefix + ".proj_out.bias"))
        return (xf + a).reshape(b, c, hh, ww)

    def forward(self, x_batch, timesteps):
        dt = self.p("time_embed.0.weight").dtype
        t_emb = O.timestep_embedding(timesteps, self.cfg.model_channels).to(dt)
        emb = F.linear(t_emb, self.p("time_embed.0.weight"), self.p("time_embed.0.bias"))
        emb = F.linear(F.silu(emb), self.p("time_embed.2.weight"), self.p("time_embed.2.bias"))
        h = [x_batch[:, i:i + 1].to(dt) for i in range(4)]
        hs = []
        for bi, layers in enumerate(self.spec["input_blocks"]):
            h = [self.block(f"input_blocks{s}.{bi}", layers, hi, emb) for s, hi in zip(STREAMS, h)]
            hs.append(torch.mean(torch.stack(h), dim=0))
        com_pre = [self.conv("conv_common.0", hi) for hi in h]
        dist_pre = [self.conv("conv_distinct.0", hi) for hi in h]
        cat, feats = bottleneck(com_pre, dist_pre, [self.p(n + ".se.0.weight") for n in SE_NAMES],
                                [self.p(n + ".se.2.weight") for n in SE_NAMES])
        hh = F.silu(self.conv("dim_reduction_non_zeros.0", cat, pad=0))
        hh = self.block("middle_block", self.spec["middle"], hh, emb)
        for bi, layers in enumerate(self.spec["output_blocks"]):
            hh = self.block(f"output_blocks.{bi}", layers, torch.cat([hh, hs.pop()], dim=1), emb)
        return tuple(feats) + (self.conv("out.2", F.silu(self.gn("out.0", hh))),)


@torch.no_grad()
def disc_forward(kw, sd, x_batch, timesteps, dtype=torch.float32):
    """The 9-tuple (com_h1..4, dist_h1..4, out) for UNet_disc_Model(**kw) with state dict ``sd``."""
    sd = {k: v.to(dtype).to(x_batch.device) for k, v in sd.items()}
    return _DiscNet(unet_config(kw), sd).forward(x_batch.to(dtype), timesteps)


# ---------------------------------------------------------------------------------------- the fixture
_G = {}


def fixture():
    if "g" not in _G:
        _G["g"] = golden("disc")
    return _G["g"]


def case(key):
    """(constructor keywords, state dict, x_batch [B,4,H,W], [(tag, t, nine reference outputs)])."""
    g = fixture()
    kw = json.loads(str(g[key + "_cfg"]))
    x = randn(tuple(int(v) for v in g[key + "_xshape"]), int(g[key + "_xseed"]))
    runs = [(tag, torch.from_numpy(g[f"{key}_t_{tag}"]), [g[f"{key}_{tag}_{i}"] for i in range(9)]) for tag in ("int", "float")]
    return kw, fixture_params(g, key), x, runs


def names_shapes(key):
    return [(n, tuple(s)) for n, s in json.loads(str(fixture()[key + "_params"]))]


def chain_case(name):
    """(model key, constructor keywords, state dict, dict(ddim, eta, learn_sigma, steps), x_T, [t1, t2, dwi], noise [steps,...],
    the reference's sample)."""
    g = fixture()
    key = str(g[name + "_model"])
    kw = json.loads(str(g[key + "_cfg"]))
    shape = tuple(int(v) for v in g[name + "_shape"])
    opts = dict(ddim=bool(g[name + "_ddim"]), eta=float(g[name + "_eta"]), learn_sigma=bool(g[name + "_learn_sigma"]),
                steps=int(g[name + "_steps"]))
    x_T = randn(shape, int(g[name + "_xT_seed"]))
    planes = [randn(shape, int(s)) for s in g[name + "_plane_seeds"]]
    z = randn((opts["steps"],) + shape, int(g[name + "_noise_seed"]))
    return key, kw, fixture_params(g, key), opts, x_T, planes, z, g[name + "_y"]
