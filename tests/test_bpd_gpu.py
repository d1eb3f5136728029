"""Variational bound on the MI355X: the terms / prior / ddim-reverse kernels against the fixture the reference generated
(tests/golden/bpd.npz, tests/golden/gen_bpd.py), and the device loop dsd_calc_bpd against the per-step path, the
reference's recorded loops and its own invariants.

Bars.  Scalars (vb, xstart_mse, mse, prior): the reference's fp32 result is only so close to exact arithmetic (the KL's
-1 + lv2 - lv1 + exp(..) cancels when it is small, cdf_plus - cdf_min near saturation), so the yardstick per quantity is the
largest relative distance between the reference's fp32 and float64 results over the fixture, stored by the generator; the GPU is
held to 4x that against the float64 value: 2x because two independent fp32 evaluations lie either side of it, 2x because the
device expf / logf / tanhf and the fp64 summation are other implementations than torch's CPU ones.  Planes and
ddim_reverse_sample are elementwise: 3e-6 relative L2, the kernel bar of the project.  Loop scalars: 5x the larger of the op bar
and the recorded movement of that scalar under 3e-6 noise on the network output (the chain margin of the other loop tests).
Measured values: DESIGN.md section 7."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import bpd_cases as BC
import dit_loops_util as U
from util import golden, fixture_params

pytestmark = pytest.mark.gpu


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def diffusion(pred="eps", var="large", respacing=BC.RESPACING, rescale=False):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, timestep_respacing=respacing, rescale_timesteps=rescale,
                                     learn_sigma=var == "range", sigma_small=var == "small", predict_xstart=pred == "x0",
                                     parameterization="v" if pred == "v" else "eps")


@functools.lru_cache(maxsize=None)
def sched_of(pred, var, clip):
    return diffusion(pred, var)._schedule(False, 0.0, bool(clip))


@pytest.fixture(scope="module")
def fx():
    _lib().require_gpu(0)
    g = golden("bpd")
    d = diffusion()
    tab = {k: np.asarray(getattr(d, k), dtype=np.float64) for k in BC.TABLES}
    return g, tab, {q: float(g["bar_" + q]) for q in BC.QUANTITIES + ("prior",)}


def run_op(c, inp, noise="fed", planes=False, seed=0, shift=False):
    """dsd_op_vlb_terms on one op case -> ({quantity: [B] tensor}, planes or None).  shift: every tensor starts 4 bytes past a
    16-byte boundary, so the launcher takes V = 1 on the same data."""
    from diffusion_models_dsdiff_amd._sched import vlb_terms
    d, s = diffusion(c["pred"], c["var"]), sched_of(c["pred"], c["var"], c["clip"])
    k = d.num_timesteps - 1 - inp["t"]

    def dev(t):
        t = t.cuda().contiguous()
        if not shift:
            return t
        buf = torch.empty(t.numel() + 1, device="cuda", dtype=torch.float32)
        buf[1:].copy_(t.reshape(-1))
        v = buf[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4
        return v
    res = {q: torch.full((BC.OP_B,), float("nan"), device="cuda") for q in BC.QUANTITIES}
    z = dev(inp["noise"]) if noise == "fed" else None
    p = vlb_terms(s, k, float(d._post_log_var()[k]), dev(inp["out"]), dev(inp["x_t"]), dev(inp["x_start"]), z, seed, vb=res["vb"],
                  xstart_mse=res["xstart_mse"], mse=res["mse"], want_planes=planes)
    return res, p


@pytest.mark.parametrize("size", BC.SIZES + (BC.BIG["size"],))
def test_op_cases_against_the_reference(fx, size):
    """Every op case of one sample size: the three scalars within 4 stored bars of the reference's float64 value; for the plane
    cases p_mean_variance's planes and ddim_reverse_sample within 3e-6 relative L2 of the reference's fp32 ones."""
    from diffusion_models_dsdiff_amd._sched import ddim_reverse_step
    g, tab, bars = fx
    worst = {q: 0.0 for q in BC.QUANTITIES}
    worst_plane, n = 0.0, 0
    for c in BC.op_cases():
        if tuple(c["size"]) != tuple(size):
            continue
        n += 1
        inp = BC.op_inputs(c, tab)
        plane = BC.is_plane_case(c)
        res, p = run_op(c, inp, planes=plane)
        for q in BC.QUANTITIES:
            worst[q] = max(worst[q], BC.rel(res[q].cpu().numpy(), g["op64_" + q][c["i"]]))
        if plane:
            d, s = diffusion(c["pred"], c["var"]), sched_of(c["pred"], c["var"], c["clip"])
            x = inp["x_t"].cuda().clone()
            x0 = ddim_reverse_step(s, d.num_timesteps - 1 - inp["t"], float(np.float32(d.alphas_cumprod_next[inp["t"]])),
                                   inp["out"].cuda(), x, want_x0=True)
            for name, got in zip(("mean", "log_variance", "pred_xstart", "pred_xstart", "reverse"), p + (x0, x)):
                ref = g[f"plane_{c['i']}_{name}"]
                worst_plane = max(worst_plane, float(np.linalg.norm(got.cpu().numpy() - ref) / np.linalg.norm(ref)))
    print(f"{size}: {n} cases, worst relative distance from the float64 reference {worst} (bars x4: "
          f"{ {q: 4 * bars[q] for q in BC.QUANTITIES} }), planes rel-L2 {worst_plane:.2e}")
    assert n == (1 if tuple(size) == BC.BIG["size"] else 3 * 3 * 3 * 2 * 4 * 2)
    for q in BC.QUANTITIES:
        assert worst[q] <= 4 * bars[q], (q, worst[q], bars[q])
    assert worst_plane <= 3e-6


def test_prior_against_the_reference(fx):
    g, tab, bars = fx
    d = diffusion()
    cases = BC.op_cases()
    worst = 0.0
    for row, i in enumerate(g["prior_case"]):
        xs = BC.op_inputs(cases[int(i)], tab)["x_start"].cuda()
        worst = max(worst, BC.rel(d._prior_bpd(xs).cpu().numpy(), g["prior64"][row]))
    print(f"prior: worst relative distance from the float64 reference {worst:.3e} (bar x4: {4 * bars['prior']:.3e})")
    assert worst <= 4 * bars["prior"]


def _case(fx, **want):
    c = next(c for c in BC.op_cases() if all(c[k] == v for k, v in want.items()))
    return c, BC.op_inputs(c, fx[1])


@pytest.mark.parametrize("tn", ("t0", "mid"))
@pytest.mark.parametrize("noise", ("fed", "philox"))
def test_scalar_and_vector_paths_and_two_runs_are_bit_identical(fx, tn, noise):
    """24x40 with two channels (a multiple of four, several blocks): the same data 4 bytes past a 16-byte boundary forces V = 1;
    scalars and planes must carry the same bits, with fed and with regenerated noise, in the decoder and the KL form; so must a
    second run."""
    c, inp = _case(fx, size=(24, 40), cz=2, pred="eps", var="range", clip=1, tn=tn, dist=0.5)
    a, pa = run_op(c, inp, noise, planes=True, seed=77)
    b, pb = run_op(c, inp, noise, planes=True, seed=77, shift=True)
    a2, _ = run_op(c, inp, noise, planes=True, seed=77)
    for q in BC.QUANTITIES:
        assert bool(torch.isfinite(a[q]).all()) and torch.equal(a[q], b[q]) and torch.equal(a[q], a2[q]), q
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    if noise == "philox":                                   # another seed draws other normals: only mse reads them
        o, _ = run_op(c, inp, noise, seed=78)
        assert torch.equal(o["vb"], a["vb"]) and not torch.equal(o["mse"], a["mse"])


def test_planes_and_scalars_agree(fx):
    """The scalars are the means of what the planes hold: (pred_xstart - x_start)^2 and the KL of the stored mean / log-variance
    against the true posterior, recomputed in float64 on the host."""
    g, tab, bars = fx
    c, inp = _case(fx, size=(24, 40), cz=3, pred="v", var="range", clip=1, tn="mid", dist=0.5)
    res, (mean, lv, x0) = run_op(c, inp, planes=True)
    d = diffusion(c["pred"], c["var"])
    t = inp["t"]
    xs, xt = inp["x_start"].double(), inp["x_t"].double()
    mse = ((x0.cpu().double() - xs) ** 2).flatten(1).mean(1)
    assert BC.rel(res["xstart_mse"].cpu().numpy(), mse.numpy()) <= 1e-6
    tm = float(np.float32(d.posterior_mean_coef1[t])) * xs + float(np.float32(d.posterior_mean_coef2[t])) * xt
    kl = BC._normal_kl(tm, torch.tensor(float(np.float32(d.posterior_log_variance_clipped[t])), dtype=torch.float64),
                       mean.cpu().double(), lv.cpu().double()).flatten(1).mean(1) / np.log(2.0)
    assert BC.rel(res["vb"].cpu().numpy(), kl.numpy()) <= 4 * bars["vb"]


# ---------------------------------------------------------------------------------------------- loops
@functools.lru_cache(maxsize=None)
def loop_env(name):
    """(object handed to calc_bpd_loop, the native denoiser, x_start, cond, noise) of a loop case, on the GPU."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.model import DSUnetModel
    _lib().require_gpu(0)
    lc = BC.LOOP_CASES[name]
    if lc["net"] == "tiny":
        gm = golden("model")
        model = DiffusionWrapper({"target": "UNet_DS_Diff.model.DSUnetModel", "params": json.loads(str(gm["tiny_cfg"]))}, "concat")
        unet = model.diffusion_model
        unet.load_state_dict(fixture_params(gm, "tiny"), strict=True)
    elif lc["net"] == "tinyfilm":
        gm = golden("model")
        model = unet = DSUnetModel(**json.loads(str(gm["tinyfilm_cfg"])))
        unet.load_state_dict(fixture_params(gm, "tinyfilm"), strict=True)
    elif lc["net"] == "lat":
        gl = golden("latent_ldm")
        model = unet = UNetModel(**json.loads(str(gl["unet_cfg"])))
        unet.load_state_dict(fixture_params(gl, "unet"), strict=True)
    else:
        model = DiffusionWrapper({"target": U.DIT_TARGET, "params": U.MODELS[lc["net"]][0]}, "concat")
        unet = model.diffusion_model
        unet.load_state_dict(U.weights(lc["net"]), strict=True)
    x_start, cond, z = (t.cuda() for t in BC.loop_inputs(name))
    return model, unet, x_start, cond, z


def loop_diffusion(name):
    lc = BC.LOOP_CASES[name]
    return diffusion(lc["pred"], lc["var"], lc["respacing"], lc["rescale"])


def per_step(name, **kw):
    """calc_bpd_loop's per-step path: a closure hides the native denoiser, so every step is dsd_op_q_sample, one dsd_forward /
    dsd_block_forward and dsd_op_vlb_terms."""
    _, unet, x_start, cond, _ = loop_env(name)

    def closure(x, t, **_):
        out = unet(torch.cat([x, cond], 1), t)
        return out[0] if isinstance(out, tuple) else out
    return loop_diffusion(name).calc_bpd_loop(closure, x_start, clip_denoised=bool(BC.LOOP_CASES[name]["clip"]), **kw)


def device(name, **kw):
    model, _, x_start, cond, _ = loop_env(name)
    return loop_diffusion(name).calc_bpd_loop(model, x_start, clip_denoised=bool(BC.LOOP_CASES[name]["clip"]),
                                              model_kwargs=dict(c_concat=[cond]), **kw)


KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


@pytest.mark.parametrize("name", list(BC.LOOP_CASES))
def test_device_loop_against_the_reference_and_the_per_step_path(fx, name):
    """The device loop returns the reference's keys and shapes, equals the per-step path bit for bit with fed and with Philox
    noise, leaves x_start untouched, and lies within 5x max(op bar, recorded 3e-6-noise movement) of every scalar the reference
    recorded (the DiT's network is the restated one, oracle/dit.py, pinned on the reference's own DiT by tests/golden/dit.npz)."""
    g, tab, bars = fx
    _, _, x_start, _, z = loop_env(name)
    keep = x_start.clone()
    T, B = int(BC.LOOP_CASES[name]["respacing"]), BC.LOOP_CASES[name]["B"]
    dev = device(name, step_noise=z)
    assert torch.equal(x_start, keep)
    assert set(dev) == set(KEYS)
    assert all(dev[k].shape == ((B, T) if k in ("vb", "xstart_mse", "mse") else (B,)) and dev[k].dtype == torch.float32 for k in KEYS)
    assert torch.equal(dev["total_bpd"], dev["vb"].sum(dim=1) + dev["prior_bpd"])
    ps = per_step(name, step_noise=z)
    for k in KEYS:
        assert bool(torch.isfinite(dev[k]).all()) and torch.equal(dev[k], ps[k]), k
    a, b = device(name, seed=4242), per_step(name, seed=4242)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["mse"], dev["mse"]) and torch.equal(a["prior_bpd"], dev["prior_bpd"])
    assert torch.equal(x_start, keep)
    op_bar = {"vb": bars["vb"], "xstart_mse": bars["xstart_mse"], "mse": bars["mse"], "prior_bpd": bars["prior"], "total_bpd": bars["vb"]}
    for k in KEYS:
        ref, moved = g[f"loop_{name}_{k}"].astype(np.float64), g[f"loop_{name}_{k}_moved"]
        err = np.abs(dev[k].cpu().numpy().astype(np.float64) - ref) / np.abs(ref)
        bar = 5 * np.maximum(op_bar[k], moved)
        print(f"{name} {k}: worst relative distance from the reference {err.max():.3e} (smallest bar {bar.min():.3e})")
        assert bool((err <= bar).all()), (name, k, err.max())


@pytest.mark.parametrize("name", ["tiny_v_large_10", "dit_eps_range_6"])
def test_split_runs_graph_replay_and_slice_ids(name):
    """first_step / n_steps as (0,1), (1,2), (3,rest) fill the same columns with the same bits; so does the loop under
    dsd_set_graph (and the replay counter moves); with slice ids and Philox noise a batch of four gives what two batches of two give."""
    from diffusion_models_dsdiff_amd._sched import run_bpd_loop
    L = _lib()
    _, unet, x_start, cond, z = loop_env(name)
    d = loop_diffusion(name)
    sched = d._schedule(False, 0.0, bool(BC.LOOP_CASES[name]["clip"]))
    plv, prior_lv = d._post_log_var(), float(np.float32(d.log_one_minus_alphas_cumprod[-1]))
    run = lambda xs, c, **kw: run_bpd_loop(unet, sched, plv, prior_lv, xs, c, **kw)
    whole = run(x_start, cond, step_noise=z)
    out = None
    for first, n in ((0, 1), (1, 2), (3, 0)):
        out = run(x_start, cond, step_noise=z, first_step=first, n_steps=n, out=out)
    for k in whole:
        assert torch.equal(out[k], whole[k]), k
    caps, launches = C.c_int(), C.c_int()
    L.check(L.lib().dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
    before = launches.value
    L.check(L.lib().dsd_set_graph(unet._h, 1))
    try:
        rep = [run(x_start, cond, step_noise=z) for _ in range(2)]
        L.check(L.lib().dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
    finally:
        L.check(L.lib().dsd_set_graph(unet._h, 0))
    assert launches.value > before
    for k in whole:
        assert torch.equal(rep[0][k], whole[k]) and torch.equal(rep[1][k], whole[k]), k
    x4, c4 = torch.cat([x_start, x_start.flip(-1)]).contiguous(), torch.cat([cond, cond.flip(-1)]).contiguous()
    ids = [7, 3, 9, 5]

    def with_ids(v, xs, c):
        arr = (C.c_int64 * max(1, len(v)))(*v)
        L.check(L.lib().dsd_set_slice_ids(unet._h, arr, len(v)))
        return run(xs, c, seed=99)
    try:
        four = with_ids(ids, x4, c4)
        halves = [with_ids(ids[:2], x4[:2].contiguous(), c4[:2].contiguous()), with_ids(ids[2:], x4[2:].contiguous(), c4[2:].contiguous())]
    finally:
        L.check(L.lib().dsd_set_slice_ids(unet._h, None, 0))
    plain = run(x4, c4, seed=99)
    for k in four:                                             # the network at another batch size: rounding, as in the PLMS test
        assert BC.rel(four[k].cpu().numpy(), torch.cat([halves[0][k], halves[1][k]]).cpu().numpy()) <= 1e-5, k
    assert BC.rel(plain["mse"].cpu().numpy(), four["mse"].cpu().numpy()) > 1e-3      # the ids do key the noise
    before = L.lib().dsd_device_bytes(unet._h)
    run(x_start, cond, step_noise=z)
    assert L.lib().dsd_device_bytes(unet._h) == before > 0


def test_python_surface_matches_the_reference(fx):
    """Keys, shapes and values of the single-step methods on the tiny model: _vb_terms_bpd and p_mean_variance agree with the
    loop's column; q_sample / q_mean_variance / q_posterior_mean_variance / _predict_* are the reference's expressions;
    ddim_reverse_sample asserts eta == 0; ModelVarType.LEARNED keeps raising."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import gaussian_diffusion as gd
    name = "tiny_v_large_10"
    model, unet, x_start, cond, z = loop_env(name)
    d = loop_diffusion(name)
    kw = dict(model_kwargs=dict(c_concat=[cond]))
    dev = device(name, step_noise=z)
    T, B = d.num_timesteps, x_start.shape[0]
    for i in (0, 4, T - 1):
        k = T - 1 - i
        t = torch.tensor([i] * B, device="cuda")
        x_t = d.q_sample(x_start, t, noise=z[k])
        a = float(np.float32(d.sqrt_alphas_cumprod[i])) * x_start + float(np.float32(d.sqrt_one_minus_alphas_cumprod[i])) * z[k]
        assert torch.equal(x_t, a)
        r = d._vb_terms_bpd(model, x_start, x_t, t, clip_denoised=True, **kw)
        assert set(r) == {"output", "pred_xstart"} and r["output"].shape == (B,) and r["pred_xstart"].shape == x_start.shape
        assert torch.equal(r["output"], dev["vb"][:, k])
        p = d.p_mean_variance(model, x_t, t, clip_denoised=True, **kw)
        assert set(p) == {"mean", "variance", "log_variance", "pred_xstart"} and all(v.shape == x_start.shape for v in p.values())
        assert torch.equal(p["pred_xstart"], r["pred_xstart"])
        large = np.append(d.posterior_variance[1], d.betas[1:])
        assert torch.equal(p["variance"], torch.full_like(x_t, float(np.float32(large[i]))))
        assert torch.equal(p["log_variance"], torch.full_like(x_t, float(np.float32(np.log(large[i])))))
        mean, _, lvc = d.q_posterior_mean_variance(p["pred_xstart"], x_t, t)
        assert torch.equal(mean, p["mean"]) and lvc.shape == x_t.shape
        eps = d._predict_eps_from_xstart(x_t, t, p["pred_xstart"])
        assert BC.rel(((eps.double() - z[k].double()) ** 2).flatten(1).mean(1).cpu().numpy(), dev["mse"][:, k].cpu().numpy()) <= 1e-6
        assert d._predict_xstart_from_eps(x_t, t, eps).shape == x_t.shape
        rv = d.ddim_reverse_sample(model, x_t, t, clip_denoised=True, **kw)
        assert set(rv) == {"sample", "pred_xstart"} and torch.equal(rv["pred_xstart"], p["pred_xstart"])
        den = d.p_mean_variance(model, x_t, t, clip_denoised=True, denoised_fn=lambda x: 0.5 * x, **kw)
        raw = d.p_mean_variance(model, x_t, t, clip_denoised=False, **kw)["pred_xstart"]      # denoised_fn acts before the clip
        assert torch.equal(den["pred_xstart"], (0.5 * raw).clamp(-1, 1)) and not torch.equal(den["pred_xstart"], p["pred_xstart"])
    m, v, lv = d.q_mean_variance(x_start, torch.tensor([T - 1] * B, device="cuda"))
    assert m.shape == v.shape == lv.shape == x_start.shape
    assert torch.equal(d._prior_bpd(x_start), dev["prior_bpd"])
    with pytest.raises(AssertionError, match="deterministic"):
        d.ddim_reverse_sample(model, x_start, torch.tensor([1] * B, device="cuda"), eta=0.5, **kw)
    bad = gd.GaussianDiffusion(betas=d.betas, model_mean_type=gd.ModelMeanType.EPSILON, model_var_type=gd.ModelVarType.LEARNED,
                               loss_type=gd.LossType.MSE)
    with pytest.raises(NotImplementedError, match="LEARNED"):
        bad.calc_bpd_loop(model, x_start, **kw)


def test_rejections_leave_outputs_and_x_start_untouched():
    """Every rejection happens on the host, before any launch: a sampler mode other than DSD_MODE_A_DDPM, null outputs, a null
    post_log_var, a learned-range schedule on a model without a variance half, channel, shape and slice-id misfits."""
    from diffusion_models_dsdiff_amd import _sched
    from diffusion_models_dsdiff_amd._lib import DsdBpd
    L = _lib()
    name = "tiny_v_large_10"
    _, unet, x_start, cond, z = loop_env(name)
    d = loop_diffusion(name)
    sched = d._schedule(False, 0.0, True)
    plv, prior_lv = d._post_log_var(), 0.0
    B, T = x_start.shape[0], sched.steps
    keep = x_start.clone()
    out = {k: torch.full((B, T), 7.0, device="cuda") for k in ("vb", "xstart_mse", "mse")}
    out["prior_bpd"] = torch.full((B,), 7.0, device="cuda")
    run = lambda s, xs=x_start, c=cond, **kw: _sched.run_bpd_loop(unet, s, plv, prior_lv, xs, c, out=out, **kw)
    with pytest.raises(L.DsdError, match=r"DSD_MODE_A_DDPM.*mode 1"):
        run(d._schedule(True, 0.0, True))
    with pytest.raises(L.DsdError, match=r"model has 1 output channels but the schedule expects 2 \(learned_range needs a variance half\)"):
        run(diffusion("eps", "range")._schedule(False, 0.0, True))
    with pytest.raises(L.DsdError, match="cond must have 1 or 3 channels, got 2"):
        run(sched, c=torch.cat([cond, cond], 1).contiguous())
    arr = (C.c_int64 * 3)(1, 2, 3)
    L.check(L.lib().dsd_set_slice_ids(unet._h, arr, 3))
    try:
        with pytest.raises(L.DsdError, match="dsd_set_slice_ids gave 3 ids but the batch has 2 slices"):
            run(sched)
    finally:
        L.check(L.lib().dsd_set_slice_ids(unet._h, None, 0))

    def raw(**null):
        bpd = DsdBpd()
        bpd.post_log_var = plv.ctypes.data_as(C.POINTER(C.c_float))
        bpd.vb, bpd.xstart_mse, bpd.mse, bpd.prior = (out[k].data_ptr() for k in ("vb", "xstart_mse", "mse", "prior_bpd"))
        for k in null:
            setattr(bpd, k, None)
        return L.lib().dsd_calc_bpd(unet._h, C.byref(sched.c), C.byref(bpd), L.dptr(cond), cond.shape[1], L.dptr(x_start), 1, None,
                                    C.c_uint64(1), B, x_start.shape[2], x_start.shape[3], 0, 0, L.stream_ptr())
    for field, msg in (("vb", b"null output"), ("mse", b"null output"), ("post_log_var", b"post_log_var is null; 10 steps")):
        assert raw(**{field: True}) != 0 and msg in L.lib().dsd_last_error(), field
    _, lat, xl, cl, _ = loop_env("lat_v_small_6")
    dl = loop_diffusion("lat_v_small_6")
    with pytest.raises(L.DsdError, match=r"the UNetModel takes 12 input channels but state \+ conditioning have 3 \+ 8"):
        _sched.run_bpd_loop(lat, dl._schedule(False, 0.0, True), dl._post_log_var(), 0.0, xl[:, :3].contiguous(), cl, out=None)
    torch.cuda.synchronize()
    assert torch.equal(x_start, keep) and all(bool((v == 7.0).all()) for v in out.values())
