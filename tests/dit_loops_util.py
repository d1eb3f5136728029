"""Shared by tests/test_dit_loops_cpu.py and tests/test_dit_loops_gpu.py: the small DiT models, their inputs and the oracle
chains of the DiT-under-the-device-loops tests.

PINNED BY THE REFERENCE: the network of every oracle chain here is oracle/dit.py, which reproduces the reference's own DiT to
the last bit on the fixtures of tests/golden/dit.npz (tests/test_pinned_cpu.py; M3 is the layout of that file's DDIM chain).
Those fixtures are the reference's code plus tests/golden/ref_standins.py, three timm modules (timm is absent from the image)
witnessed against nn.MultiheadAttention and F.unfold.  The samplers around the network are the oracle's restatements of the
reference loops (oracle/samplers.py, oracle/dpm.py).  Still unpinned: the half-precision modes' rounding places and
host_io.py's metrics."""
import functools

import numpy as np
import torch

from oracle import dit as OD
from oracle import dpm as ODPM
from oracle import samplers as OS
from oracle import schedules as S
from oracle.synth import synth_params, randn

DIT_TARGET = "diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models.DiT"
_BASE = dict(input_size=16, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=4, num_classes=0)
# name -> (constructor keywords, Cz, Cc)
MODELS = {
    "M1": (dict(_BASE), 1, 3),                                              # the yaml's layout: 1 state + 3 condition channels
    "M2": (dict(_BASE, in_channels=6), 2, 4),                               # multi-channel learned range
    "M3": (dict(_BASE, in_channels=3, learn_sigma=False), 3, 0),            # unconditional
    "M4": (dict(_BASE, input_size=32, hidden_size=128, num_heads=2), 1, 3),  # head dim 64: the LDS-DMA attention kernel
}
WEIGHT_SEED = 901
CHAIN_STEPS = 10                 # respaced steps of the oracle chains
CHAIN_BATCH = {"M1": 2, "M2": 3}
PERTURB, MOVE_MAX = 3e-6, 2e-5   # the conditioning guard of the oracle chains (as tests/golden/gen_plms.py)


def names_shapes(kw):
    """(name, shape) of DiT(**kw)'s state_dict in declaration order, without building a handle (the CPU tests have no GPU)."""
    D, p, cin, depth = kw["hidden_size"], kw["patch_size"], kw["in_channels"], kw["depth"]
    cout = cin // 3 * 2 if kw.get("learn_sigma", True) else cin
    T, mlp = (kw["input_size"] // p) ** 2, int(D * 4.0)
    lin = lambda n, i, o: [(n + ".weight", (o, i)), (n + ".bias", (o,))]
    out = [("x_embedder.proj.weight", (D, cin, p, p)), ("x_embedder.proj.bias", (D,))]
    out += lin("t_embedder.mlp.0", 256, D) + lin("t_embedder.mlp.2", D, D)
    assert kw.get("num_classes", 1000) == 0
    out += [("pos_embed", (1, T, D))]
    for i in range(depth):
        b = f"blocks.{i}"
        out += lin(b + ".attn.qkv", D, 3 * D) + lin(b + ".attn.proj", D, D) + lin(b + ".mlp.fc1", D, mlp) + lin(b + ".mlp.fc2", mlp, D)
        out += lin(b + ".adaLN_modulation.1", D, 6 * D)
    out += lin("final_layer.linear", D, p * p * cout) + lin("final_layer.adaLN_modulation.1", D, 2 * D)
    return out


@functools.lru_cache(maxsize=None)
def weights(name):
    """Randomised as tests/test_dit_gpu.py does it: the default initialisation zeroes the adaLN and output layers, so every
    output would be 0 and every loop would pass trivially."""
    return synth_params(names_shapes(MODELS[name][0]), WEIGHT_SEED)


def inputs(name, B, seed=0):
    """(x_T [B,Cz,S,S], cond [B,Cc,S,S]) on the CPU."""
    kw, Cz, Cc = MODELS[name]
    S_ = kw["input_size"]
    return randn((B, Cz, S_, S_), 1300 + seed), randn((B, Cc, S_, S_), 1400 + seed)


def oracle_net(name, cond, perturb_gen=None):
    """model(x_in, t) of the oracle samplers: oracle/dit.py on the concatenated input (the samplers concatenate ``cond``
    themselves when handed it; here the closure does, so one callable serves DiffusionA and dpm_multistep)."""
    kw, Cz, Cc = MODELS[name]
    sd = weights(name)
    out_ch = kw["in_channels"] // 3 * 2 if kw.get("learn_sigma", True) else kw["in_channels"]

    def net(x, t):
        out = OD.dit_forward(sd, torch.cat([x, cond], 1), t.float(), None, patch_size=kw["patch_size"], num_heads=kw["num_heads"],
                             out_channels=out_ch)
        if perturb_gen is not None:
            out = out + PERTURB * out.pow(2).mean().sqrt() * torch.randn(out.shape, generator=perturb_gen)
        return out
    return net


def spaced_betas():
    betas, _ = S.spaced(S.named_beta_schedule("linear", 1000), S.space_timesteps(1000, str(CHAIN_STEPS)))
    return torch.from_numpy(np.asarray(betas)).float()


def chain_noise(name):
    kw, Cz, _ = MODELS[name]
    return randn((CHAIN_STEPS, CHAIN_BATCH[name], Cz, kw["input_size"], kw["input_size"]), 1500)


DIFFUSION_KW = dict(steps=1000, timestep_respacing=str(CHAIN_STEPS), learn_sigma=True, rescale_timesteps=True)
CHAINS = ("ddpm", "ddim", "dpm")
DDIM_ETA = 0.5


def oracle_chain(name, kind, perturb=False):
    """One oracle chain of the DiT ``name`` (learn_sigma models): 'ddpm' = DiffusionA.p_sample_loop with the learned-range
    variance, 'ddim' = ddim_sample_loop (eta 0.5), 'dpm' = dpm_multistep (++, order 2, logSNR, thresholding: what
    GaussianDiffusion.dpm_solver_sample_loop runs), which reads the first Cz output channels."""
    Cz = MODELS[name][1]
    x_T, cond = inputs(name, CHAIN_BATCH[name])
    gen = torch.Generator().manual_seed(1600) if perturb else None
    net = oracle_net(name, cond, gen)
    if kind == "dpm":
        return ODPM.dpm_multistep(lambda x, t: net(x, t)[:, :Cz], ODPM.NoiseSchedule(betas=spaced_betas()), x_T.clone(),
                                  steps=CHAIN_STEPS, order=2, skip_type="logSNR", thresholding=True, lower_order_final=False)
    d = OS.DiffusionA(**DIFFUSION_KW)
    if kind == "ddpm":
        return d.p_sample_loop(net, x_T, chain_noise(name))
    return d.ddim_sample_loop(net, x_T, chain_noise(name), eta=DDIM_ETA)


@functools.lru_cache(maxsize=None)
def oracle_chain_cached(name, kind):
    return oracle_chain(name, kind)
