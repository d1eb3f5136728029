"""Import stand-ins for the two packages the reference needs and the build image lacks — FIXTURE GENERATORS ONLY.

``install()`` puts into ``sys.modules``

  omegaconf / omegaconf.listconfig        ``class ListConfig(list)``: the reference's UNetModel constructor imports it for one
                                          ``type(context_dim) == ListConfig`` test (openaimodel.py:640)
  timm / timm.models / timm.models.vision_transformer
                                          ``PatchEmbed``, ``Attention``, ``Mlp``: the three modules UNet_DS_Diff/DiT_models.py
                                          builds its DiT from

so that the reference's own DiT and UNetModel(use_spatial_transformer=True) run unchanged on the CPU and fixtures can be taken
from them (gen_dit.py, gen_unet_xattn.py).  The three modules are written here from their published definition (timm 0.9,
models/vision_transformer.py, layers/patch_embed.py, layers/mlp.py: norm_layer=None, no qk-norm, no dropout); the attention is
the unfused form (scale q, softmax(q k^T), @ v), not scaled_dot_product_attention, so the fp32 summation order is the plain one.
Parameter names come out as the reference's module tree produces them: x_embedder.proj.*, blocks.i.attn.qkv.*, attn.proj.*,
mlp.fc1.*, mlp.fc2.*.

Every fixture taken through these lines is only as good as they are: tests/test_pinned_cpu.py witnesses them in float64 against
code that is not ours (nn.MultiheadAttention, F.unfold, F.gelu).  Nothing in the package imports this file.
"""
import sys
import types

import torch.nn as nn


class ListConfig(list):
    pass


class PatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, bias=True):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.grid_size = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size, bias=bias)
        self.norm = nn.Identity()

    def forward(self, x):
        return self.norm(self.proj(x).flatten(2).transpose(1, 2))


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        attn = ((q * self.scale) @ k.transpose(-2, -1)).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, N, C))


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        assert drop == 0
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


def install():
    """Register the stand-ins, in front of an installed omegaconf or timm too (a newer timm runs a fused attention, whose
    fp32 summation order is not the one the fixtures are meant to hold)."""
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    oc = module("omegaconf")
    oc.listconfig = module("omegaconf.listconfig", ListConfig=ListConfig)
    tm = module("timm")
    tm.models = module("timm.models")
    tm.models.vision_transformer = module("timm.models.vision_transformer", PatchEmbed=PatchEmbed, Attention=Attention, Mlp=Mlp)
