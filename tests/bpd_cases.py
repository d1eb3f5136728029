"""Shared by tests/golden/gen_bpd.py, tests/test_bpd_cpu.py and tests/test_bpd_gpu.py: the case grid of the variational-bound
fixture (tests/golden/bpd.npz), its inputs (regenerated from seeds: the fixture stores results only) and a torch restatement of
gaussian_diffusion.py:788-819, 922-991 and losses.py that runs in fp32 or float64."""
import itertools

import numpy as np
import torch

from oracle.synth import randn

SIZES = ((5, 7), (15, 15), (24, 40))
CZS = (1, 2, 3)
PREDS = ("eps", "x0", "v")
VARS = ("small", "large", "range")
CLIPS = (1, 0)
T_NAMES = ("t0", "t1", "mid", "last")
DISTS = (0.02, 0.5)
OP_B = 3
RESPACING = "10"
BIG = dict(size=(128, 128), cz=1, pred="eps", var="range", clip=1, tn="mid", dist=0.5)   # several blocks in the reduction
SPECIALS = (-1.0, 1.0, 0.9995, -0.9995, 0.0)      # all three branches of the discretised likelihood select
# the plane cases (mean / log_variance / pred_xstart / ddim_reverse_sample stored in full): the 5x7, Cz = 2 slice of the grid
PLANE_SIZE, PLANE_CZ, PLANE_DIST, PLANE_T = (5, 7), 2, 0.5, ("t0", "mid")
TABLES = ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
          "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1",
          "posterior_mean_coef2", "betas", "alphas_cumprod_next")
QUANTITIES = ("vb", "xstart_mse", "mse")


def t_of(tn, T):
    return {"t0": 0, "t1": 1, "mid": T // 2, "last": T - 1}[tn]


def op_cases():
    """The grid in a fixed order; case i is row i of the fixture's op arrays.  The last case is BIG."""
    out = []
    for size, cz, pred, var, clip, tn, dist in itertools.product(SIZES, CZS, PREDS, VARS, CLIPS, T_NAMES, DISTS):
        out.append(dict(size=size, cz=cz, pred=pred, var=var, clip=clip, tn=tn, dist=dist))
    out.append(dict(BIG))
    for i, c in enumerate(out):
        c["i"] = i
    return out


def is_plane_case(c):
    return tuple(c["size"]) == PLANE_SIZE and c["cz"] == PLANE_CZ and c["dist"] == PLANE_DIST and c["tn"] in PLANE_T


def op_inputs(c, tab):
    """fp32 CPU tensors of one op case: x_start (with SPECIALS planted at the head of every sample), noise, x_t = q_sample and
    the stored "network output" (with a variance half of 0.6 * N' for 'range').
    ``tab``: the float64 tables (fixture entries tab_*, or a diffusion object's attributes)."""
    H, W = c["size"]
    shape = (OP_B, c["cz"], H, W)
    seed = 5000 + 7 * c["i"]
    t = t_of(c["tn"], len(tab["betas"]))
    x_start = (0.5 * randn(shape, seed)).clamp(-1, 1)
    flat = x_start.view(OP_B, -1)
    flat[:, :len(SPECIALS)] = torch.tensor(SPECIALS)
    noise = randn(shape, seed + 1)
    c0 = torch.tensor(np.float32(tab["sqrt_alphas_cumprod"][t]))
    c1 = torch.tensor(np.float32(tab["sqrt_one_minus_alphas_cumprod"][t]))
    x_t = c0 * x_start + c1 * noise
    # noise + dist * N: near the truth as an eps prediction, far from it as x0 / v.  One exception, the x0 prediction at t = 0:
    # the reference's own fp32 decoder likelihood of a prediction many standard deviations off is 1.6e-2 from exact arithmetic
    # (both CDFs saturate), which would make the bar of every case useless; there the output is x_start + c1 * dist * N, as far
    # from x_start in units of the step's noise level
    n2 = randn(shape, seed + 2)
    out = x_start + c1 * (np.float32(c["dist"]) * n2) if (c["pred"] == "x0" and t == 0) else noise + np.float32(c["dist"]) * n2
    if c["var"] == "range":
        out = torch.cat([out, 0.6 * randn(shape, seed + 3)], 1)
    return dict(x_start=x_start, noise=noise, x_t=x_t, out=out.contiguous(), t=t)


# ---------------------------------------------------------------------------------------------- restatement
def _cdf(x):
    return 0.5 * (1.0 + torch.tanh(torch.tensor(np.sqrt(2.0 / np.pi)) * (x + 0.044715 * torch.pow(x, 3))))


def _normal_kl(m1, lv1, m2, lv2):
    return 0.5 * (-1.0 + lv2 - lv1 + torch.exp(lv1 - lv2) + ((m1 - m2) ** 2) * torch.exp(-lv2))


def _discretized_ll(x, means, log_scales):
    centered = x - means
    inv = torch.exp(-log_scales)
    cdf_plus = _cdf(inv * (centered + 1.0 / 255.0))
    cdf_min = _cdf(inv * (centered - 1.0 / 255.0))
    return torch.where(x < -0.999, torch.log(cdf_plus.clamp(min=1e-12)),
                       torch.where(x > 0.999, torch.log((1.0 - cdf_min).clamp(min=1e-12)),
                                   torch.log((cdf_plus - cdf_min).clamp(min=1e-12))))


def _mean_flat(x):
    return x.mean(dim=list(range(1, x.dim())))


def restate(c, inp, tab, dtype):
    """{"vb", "xstart_mse", "mse" [B]; "mean", "log_variance", "pred_xstart", "reverse"} of one op case in ``dtype``: the fp32
    tables (arr[t].float(), :1003) meet tensors of ``dtype``, every operation in the reference's order."""
    t = inp["t"]
    f = lambda name, arr=None: torch.tensor(np.float32((tab[name] if arr is None else arr)[t]))
    x_start, noise, x_t, out = (inp[k].to(dtype) for k in ("x_start", "noise", "x_t", "out"))
    C = x_start.shape[1]
    post_lv = f("posterior_log_variance_clipped")
    if c["var"] == "range":
        out, var = out[:, :C], out[:, C:]
        frac = (var + 1) / 2
        log_variance = frac * f("", np.log(tab["betas"])) + (1 - frac) * post_lv
    elif c["var"] == "large":
        log_variance = f("", np.log(np.append(tab["posterior_variance"][1], tab["betas"][1:]))).expand(x_t.shape)
    else:
        log_variance = post_lv.expand(x_t.shape)            # fp32 whatever ``dtype``: _extract_into_tensor(...).float()
    if c["pred"] == "v":
        x0 = f("sqrt_alphas_cumprod") * x_t - f("sqrt_one_minus_alphas_cumprod") * out
    elif c["pred"] == "eps":
        x0 = f("sqrt_recip_alphas_cumprod") * x_t - f("sqrt_recipm1_alphas_cumprod") * out
    else:
        x0 = out
    if c["clip"]:
        x0 = x0.clamp(-1, 1)
    mean = f("posterior_mean_coef1") * x0 + f("posterior_mean_coef2") * x_t
    true_mean = f("posterior_mean_coef1") * x_start + f("posterior_mean_coef2") * x_t
    kl = _mean_flat(_normal_kl(true_mean, post_lv.expand(x_t.shape), mean, log_variance)) / np.log(2.0)
    nll = _mean_flat(-_discretized_ll(x_start, mean, 0.5 * log_variance)) / np.log(2.0)
    eps = (f("sqrt_recip_alphas_cumprod") * x_t - x0) / f("sqrt_recipm1_alphas_cumprod")
    abar_next = f("alphas_cumprod_next")
    reverse = x0 * torch.sqrt(abar_next) + torch.sqrt(1 - abar_next) * eps
    return dict(vb=nll if t == 0 else kl, xstart_mse=_mean_flat((x0 - x_start) ** 2), mse=_mean_flat((eps - noise) ** 2),
                mean=mean, log_variance=log_variance, pred_xstart=x0, reverse=reverse)


def restate_prior(x_start, tab, dtype):
    T = len(tab["betas"])
    m = torch.tensor(np.float32(tab["sqrt_alphas_cumprod"][T - 1])) * x_start.to(dtype)
    lv = torch.tensor(np.float32(tab["log_one_minus_alphas_cumprod"][T - 1])).expand(m.shape)
    return _mean_flat(_normal_kl(m, lv, 0.0, torch.tensor(0.0).to(m))) / np.log(2.0)


def rel(a, b):
    """Largest relative distance of the entries of ``a`` from ``b`` (float64)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---------------------------------------------------------------------------------------------- loop cases
# name -> dict(net, pred (parameterization), var, respacing, rescale, clip, B, shape of one x_start, seeds)
LOOP_CASES = {
    "tiny_v_large_10": dict(net="tiny", pred="v", var="large", respacing="10", rescale=True, clip=1, B=2, shape=(1, 32, 32), cc=1),
    "film_eps_range_6": dict(net="tinyfilm", pred="eps", var="range", respacing="6", rescale=True, clip=1, B=2, shape=(1, 32, 32), cc=3),
    "lat_v_small_6": dict(net="lat", pred="v", var="small", respacing="6", rescale=False, clip=0, B=2, shape=(4, 8, 8), cc=8),
    "dit_eps_range_6": dict(net="M2", pred="eps", var="range", respacing="6", rescale=True, clip=1, B=2, shape=(2, 16, 16), cc=4),
}
LOOP_SEED = 6100


def loop_inputs(name):
    """(x_start [B,Cz,H,W] in [-1, 1], cond [B,Cc,H,W], step noise [steps,B,Cz,H,W]) on the CPU."""
    from oracle.synth import cond_image
    lc = LOOP_CASES[name]
    k = LOOP_SEED + 10 * list(LOOP_CASES).index(name)
    B, (Cz, H, W) = lc["B"], lc["shape"]
    x_start = (0.5 * randn((B, Cz, H, W), k)).clamp(-1, 1)
    cond = cond_image((B, lc["cc"], H, W), k + 1) if lc["net"] in ("tiny", "tinyfilm") else randn((B, lc["cc"], H, W), k + 1)
    return x_start, cond, randn((int(lc["respacing"]), B, Cz, H, W), k + 2)


def diffusion_kwargs(lc):
    """Keywords of the product's create_gaussian_diffusion for a loop case."""
    return dict(steps=1000, timestep_respacing=lc["respacing"], rescale_timesteps=lc["rescale"],
                learn_sigma=lc["var"] == "range", sigma_small=lc["var"] == "small", parameterization=lc["pred"])
