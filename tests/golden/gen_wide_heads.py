#!/usr/bin/env python3
"""Generate tests/golden/wide_heads.npz by importing the REFERENCE on CPU (build container only).

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_wide_heads.py

Attention with head dims beyond 128 on the reference's own blocks — the widths of the SD-v1 U-Net (configs/v1-inference.yaml:
model_channels 320, channel_mult [1,2,4,4], num_heads 8 -> heads of 40, 80 and 160), of AttentionBlock's num_heads=1 default
and of the KL-VAE's one-head AttnBlock:

    attn_c256_h1      AttentionBlock(256, num_heads=1, use_new_attention_order=False)      x [2,256,5,7]    d = 256, legacy order
    attn_c320_h2      AttentionBlock(320, num_heads=2, use_new_attention_order=True)       x [1,320,6,6]    d = 160, new order
    xattn_d160        CrossAttention(160, context_dim=24, heads=1, dim_head=160)           x [2,33,160], context [2,9,24]
    spatial_tf_d160   SpatialTransformer(320, 2, 160, depth=1, context_dim=24)             x [1,320,6,6], context [1,9,24]
    vae_attn_c512     ldm.modules.diffusionmodules.model.AttnBlock(512)                    x [1,512,6,7]

Weights are not stored: (names, shapes, seed) only; inputs come from seeds (stored alongside the shapes).
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
REF = os.environ.get("DSD_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from oracle.synth import synth_params, randn  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_grad_enabled(False)
torch.set_num_threads(8)

# key -> (weight seed, x shape, x seed, context shape or None, context seed)
CASES = {
    "attn_c256_h1": (700, (2, 256, 5, 7), 701, None, 0),
    "attn_c320_h2": (710, (1, 320, 6, 6), 711, None, 0),
    "xattn_d160": (720, (2, 33, 160), 721, (2, 9, 24), 722),
    "spatial_tf_d160": (730, (1, 320, 6, 6), 731, (1, 9, 24), 732),
    "vae_attn_c512": (740, (1, 512, 6, 7), 741, None, 0),
}


def main():
    from ldm.modules.attention import CrossAttention, SpatialTransformer
    from ldm.modules.diffusionmodules.model import AttnBlock
    from ldm.modules.diffusionmodules.openaimodel import AttentionBlock
    mods = {
        "attn_c256_h1": AttentionBlock(256, num_heads=1, use_new_attention_order=False),
        "attn_c320_h2": AttentionBlock(320, num_heads=2, use_new_attention_order=True),
        "xattn_d160": CrossAttention(160, context_dim=24, heads=1, dim_head=160),
        "spatial_tf_d160": SpatialTransformer(320, 2, 160, depth=1, context_dim=24),
        "vae_attn_c512": AttnBlock(512),
    }
    out = {}
    for key, (seed, xshape, xseed, cshape, cseed) in CASES.items():
        m = mods[key]
        ns = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        m.load_state_dict(synth_params(ns, seed), strict=True)
        m.eval()
        x = randn(xshape, xseed)
        y = m(x) if cshape is None else m(x, context=randn(cshape, cseed))
        out.update({key + "_params": json.dumps([[n, list(s)] for n, s in ns]), key + "_seed": seed,
                    key + "_xshape": np.asarray(xshape), key + "_xseed": xseed, key + "_y": y.numpy()})
        if cshape is not None:
            out.update({key + "_cshape": np.asarray(cshape), key + "_cseed": cseed})
    np.savez_compressed(os.path.join(OUT, "wide_heads.npz"), **out)
    print("wrote wide_heads", {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
