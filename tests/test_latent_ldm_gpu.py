"""Latent diffusion sampling as the latent trainer runs it (trainers/trainer_latent_diffusion.py:153-189,492-544): the f = 8
KL first stage with scale_factor, K condition keys encoded in one pass, and the three sample_log branches (DDIMSampler,
DPMSolverSampler, LatentDiffusion.sample) on a native UNetModel with 4-channel latents, all in the device-resident latent
loops (dsd_sample / dsd_sample_dpm on a DSD_BLOCK_UNET handle).  Fixtures: the reference's own samplers (tests/golden/latent_ldm.npz,
tests/golden/gen_latent_ldm.py)."""
import ctypes as C
import json

import pytest
import torch

from oracle import dpm as ODPM, samplers as OS, unet as O, vae as V
from util import golden, fixture_params, rel_l2, randn

pytestmark = pytest.mark.gpu

STEPS = 20


def _g():
    return golden("latent_ldm")


def make_ldm(parameterization="v", scale_by_std=False, timesteps=1000, load=True):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import LatentDiffusion, latent_diffusion_param_table
    g = _g()
    dd = json.loads(str(g["vae_cfg"]))
    embed = dd.pop("embed_dim")
    up = json.loads(str(g["unet_cfg"]))
    ld = LatentDiffusion(first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                                             "params": {"ddconfig": dd, "embed_dim": embed}},
                         cond_stage_config="__is_first_stage__", conditioning_key="concat", scale_factor=float(g["scale_factor"]),
                         scale_by_std=scale_by_std, timesteps=timesteps, parameterization=parameterization, image_size=8, channels=4,
                         unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": up})
    sd = fixture_params(g, "vae", "first_stage_model.")
    sd.update(fixture_params(g, "unet", "model.diffusion_model."))
    if not load:
        return g, ld.cuda(), dd, embed, up, sd
    missing, unexpected = ld.load_state_dict(sd, strict=False)
    assert not unexpected
    table = dict(latent_diffusion_param_table({"params": up}, dd, embed, scale_by_std))
    own = {k: tuple(v.shape) for k, v in ld.state_dict().items()}
    assert all(own.get(k) == s for k, s in table.items()), [k for k, s in table.items() if own.get(k) != s][:5]
    # only the schedule buffers (and the scale_factor buffer the constructor sets) are not in the weights
    assert set(missing) - {"scale_factor"} <= {k for k in own if k not in table}
    return g, ld.cuda(), dd, embed, up, sd


@pytest.fixture(scope="module")
def ldm():
    return make_ldm()


def test_first_stage_f8_encode_scaled_sample_decode(ldm):
    g, ld, dd, embed, up, sd = ldm
    x = randn((2, 1, 64, 64), int(g["x_seed"])).cuda()
    post = ld.encode_first_stage(x)
    assert rel_l2(post.parameters, g["moments"]) < 1e-5
    z = ld.get_first_stage_encoding(post, noise=torch.from_numpy(g["post_noise"]))
    assert z.shape == (2, 4, 8, 8) and rel_l2(z, g["z_scaled"]) < 1e-5
    zin = randn((2, 4, 8, 8), int(g["zin_seed"])).cuda()
    rec = ld.decode_first_stage(zin)
    assert rec.shape == (2, 1, 64, 64) and rel_l2(rec, g["zin_decoded"]) < 1e-4
    # the 1/scale_factor rounding: float64 inverse for a Python float, fp32 reciprocal for a 0-d buffer
    import numpy as np
    assert ld.inverse_scale() == float(np.float32(1. / float(g["scale_factor"])))
    ld2 = make_ldm(scale_by_std=True)[1]
    assert "scale_factor" in ld2.state_dict()
    assert ld2.inverse_scale() == float(1. / torch.tensor(float(g["scale_factor"])))
    with pytest.raises(NotImplementedError):
        ld2.on_train_batch_start(None, 0)


def test_condition_keys_encoded_in_one_pass(ldm):
    g, ld, *_ = ldm
    cond = randn((2, 2, 64, 64), int(g["cond_seed"])).cuda()
    c = ld.encode_conditions([cond[:, :1], cond[:, 1:]], noise=torch.from_numpy(g["cond_noise"]))
    assert list(c) == ["c_concat"] and c["c_concat"][0].shape == (2, 8, 8, 8)
    assert rel_l2(c["c_concat"][0], g["c_concat"]) < 1e-5


def _cc(g):
    return {"c_concat": [torch.from_numpy(g["c_concat"]).cuda()]}


@pytest.mark.parametrize("key,eta", [("ddim_eta0", 0.0), ("ddim_eta1", 1.0)])
def test_ddim_sampler_on_latents_vs_reference(ldm, key, eta):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    g, ld, *_ = ldm
    xT = randn((2, 4, 8, 8), int(g["xT_seed"])).cuda()
    z = randn((STEPS, 2, 4, 8, 8), int(g[key + "_noise_seed"])).cuda()
    y, _ = DDIMSampler(ld).sample(STEPS, 2, (4, 8, 8), _cc(g), eta=eta, verbose=False, x_T=xT, step_noise=z)
    assert y.shape == (2, 4, 8, 8) and rel_l2(y, g[key + "_y"]) < 1e-4
    assert rel_l2(ld.decode_first_stage(y), g[key + "_decoded"]) < 1e-4


def test_dpm_solver_sampler_on_latents_vs_reference(ldm):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.dpm_solver_new.sampler import DPMSolverSampler
    g, ld, *_ = ldm
    xT = randn((2, 4, 8, 8), int(g["xT_seed"])).cuda()
    y, _ = DPMSolverSampler(ld).sample(STEPS, 2, (4, 8, 8), _cc(g), verbose=False, x_T=xT)
    assert rel_l2(y, g["dpm_y"]) < 1e-4
    assert rel_l2(ld.decode_first_stage(y), g["dpm_decoded"]) < 1e-4


def test_latent_diffusion_ddpm_sample_vs_oracle(ldm):
    """LatentDiffusion.sample (ddpm.py:1048-1115, mode B_DDPM, clip_denoised False) against oracle.samplers.DiffusionB on a
    50-step eps-model, same fed noise."""
    g, ld2, dd, embed, up, sd = make_ldm(parameterization="eps", timesteps=50)
    ucfg = O.UNetConfig.from_params(up)
    usd = {k[len("model.diffusion_model."):]: v for k, v in sd.items() if k.startswith("model.diffusion_model.")}
    cc = torch.from_numpy(g["c_concat"])
    xT, z = randn((2, 4, 8, 8), 601), randn((50, 2, 4, 8, 8), 602)
    y = ld2.sample(dict(c_concat=[cc.cuda()]), batch_size=2, shape=(2, 4, 8, 8), x_T=xT.cuda(), step_noise=z.cuda())
    od = OS.DiffusionB(timesteps=50, parameterization="eps")
    yo = od.p_sample_loop(lambda xx, tt: O.plain_unet_forward(ucfg, usd, xx, tt), xT, z, [cc], clip_denoised=False)
    assert rel_l2(y, yo) < 1e-4
    with pytest.raises(NotImplementedError):
        ldm[1].sample(dict(c_concat=[cc.cuda()]), batch_size=2, shape=(2, 4, 8, 8))   # v: the reference raises too (:941-946)


def _ddim_sched(ld, eta=1.0):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(ld)
    s.make_schedule(STEPS, ddim_eta=eta, verbose=False)
    return s._schedule(False, True)


def test_device_loop_matches_host_loop_and_graph_replay(ldm):
    """dsd_sample against the per-step host loop (network call + dsd_op_sampler_update over B*Cz planes) with the same
    pre-drawn noise; graph replay on / off bit-identical."""
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd._sched import run_device_loop, sampler_update
    g, ld, *_ = ldm
    unet = ld.model.diffusion_model
    sched = _ddim_sched(ld)
    cc = torch.from_numpy(g["c_concat"]).cuda()
    xT = randn((2, 4, 8, 8), 611).cuda()
    z = randn((STEPS, 2, 4, 8, 8), 612).cuda()
    dev = run_device_loop(unet, sched, xT, cc, step_noise=z)
    x = xT.clone()
    for k in range(sched.steps):
        out = unet(torch.cat([x, cc], 1), torch.full((2,), float(sched.t_model[k]), device="cuda"))
        sampler_update(sched, k, out, x, z[k])
    assert torch.equal(dev, x)
    _lib.check(_lib.lib().dsd_set_graph(unet._h, 1))
    try:
        rep = run_device_loop(unet, sched, xT, cc, step_noise=z)
        rep2 = run_device_loop(unet, sched, xT, cc, step_noise=z)
        caps, launches = C.c_int(), C.c_int()
        _lib.check(_lib.lib().dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
    finally:
        _lib.check(_lib.lib().dsd_set_graph(unet._h, 0))
    assert launches.value > 0 and torch.equal(rep, dev) and torch.equal(rep2, dev)
    # first_step / n_steps: two halves chain to the whole
    half = run_device_loop(unet, sched, xT, cc, step_noise=z, n_steps=STEPS // 2)
    assert torch.equal(run_device_loop(unet, sched, half, cc, step_noise=z, first_step=STEPS // 2), dev)


def test_philox_latent_noise_seeds_and_slice_ids(ldm):
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    g, ld, *_ = ldm
    unet = ld.model.diffusion_model
    sched = _ddim_sched(ld)
    cc2 = torch.from_numpy(g["c_concat"]).cuda()
    cc = torch.cat([cc2, cc2.flip(0)], 0)
    xT = randn((4, 4, 8, 8), 621).cuda()
    a = run_device_loop(unet, sched, xT, cc, seed=1234)
    assert torch.isfinite(a).all()
    assert torch.equal(a, run_device_loop(unet, sched, xT, cc, seed=1234))
    assert not torch.equal(a, run_device_loop(unet, sched, xT, cc, seed=1235))
    L = _lib.lib()

    def ids(v):
        arr = (C.c_int64 * len(v))(*v)
        _lib.check(L.dsd_set_slice_ids(unet._h, arr, len(v)))
    try:
        ids([10, 11, 12, 13])
        full = run_device_loop(unet, sched, xT, cc, seed=77)
        ids([10, 11])
        lo = run_device_loop(unet, sched, xT[:2], cc[:2], seed=77)
        ids([12, 13])
        hi = run_device_loop(unet, sched, xT[2:], cc[2:], seed=77)
    finally:
        _lib.check(L.dsd_set_slice_ids(unet._h, None, 0))
    assert torch.equal(full, torch.cat([lo, hi], 0))
    assert not torch.equal(full[:, 0], full[:, 1])


def test_latent_loops_reject_bad_input(ldm):
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd._sched import run_device_loop, Schedule
    from diffusion_models_dsdiff_amd._lib import dptr, stream_ptr
    g, ld, *_ = ldm
    unet = ld.model.diffusion_model
    sched = _ddim_sched(ld)
    cc = torch.from_numpy(g["c_concat"]).cuda()
    with pytest.raises(ValueError, match="spatial|does not match"):
        run_device_loop(unet, sched, randn((2, 4, 8, 8), 1).cuda(), cc[:, :, :4, :4].contiguous())
    lr = Schedule(_lib.MODE_A_DDPM, _lib.PRED_EPS, sched.coef, sched.t_model, sched.nonzero, learned_range=True)
    with pytest.raises(_lib.DsdError, match="learned-range"):
        run_device_loop(unet, lr, randn((2, 4, 8, 8), 1).cuda(), cc)
    # a block that is not a UNetModel (the first stage's decoder handle)
    x = randn((2, 4, 8, 8), 1).cuda()
    rc = _lib.lib().dsd_sample(ld.first_stage_model._dec._h, C.byref(sched.c), None, None, dptr(cc), 8, dptr(x), 4, None,
                               C.c_uint64(1), 2, 8, 8, 0, 0, stream_ptr())
    assert rc != 0 and "DSD_BLOCK_UNET" in _lib.lib().dsd_last_error().decode()
    with pytest.raises(_lib.DsdError, match="input channels"):
        run_device_loop(unet, sched, randn((2, 3, 8, 8), 1).cuda(), cc)


def test_trainer_shape_smoke():
    """256^2 one-channel slices through the f = 8 first stage (32x32x4 latents), then 2 DDIM steps of a UNetModel with the
    v2-1-cddpm-disc unet_config at batch 2: finite, deterministic, row 0 against the oracle."""
    from diffusion_models_dsdiff_amd.ldm.models.autoencoder import AutoencoderKL
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from oracle.synth import synth_params
    g = _g()
    dd = json.loads(str(g["vae_cfg"]))
    embed = dd.pop("embed_dim")
    up = dict(image_size=32, in_channels=8, model_channels=96, out_channels=4, num_res_blocks=2, attention_resolutions=[32, 16, 8],
              channel_mult=[1, 1, 2, 2, 3, 3], num_head_channels=48, use_new_attention_order=True, legacy=False)
    ld = LatentDiffusion(first_stage_config=AutoencoderKL(dd, None, embed), conditioning_key="concat", scale_factor=0.18215,
                         timesteps=1000, parameterization="v", unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                                                                             "params": up})
    ld.load_state_dict(fixture_params(g, "vae", "first_stage_model."), strict=False)
    usd = synth_params([(k, tuple(v.shape)) for k, v in ld.model.diffusion_model.state_dict().items()], 630)
    ld.model.diffusion_model.load_state_dict(usd, strict=True)
    ld = ld.cuda()
    img = randn((2, 1, 256, 256), 631).cuda()
    c = ld.encode_conditions(img, noise=randn((2, 4, 32, 32), 632))
    xT = randn((2, 4, 32, 32), 633).cuda()
    y, _ = DDIMSampler(ld).sample(2, 2, (4, 32, 32), c, eta=0.0, verbose=False, x_T=xT)
    y2, _ = DDIMSampler(ld).sample(2, 2, (4, 32, 32), c, eta=0.0, verbose=False, x_T=xT)
    assert torch.isfinite(y).all() and torch.equal(y, y2)
    rec = ld.decode_first_stage(y)
    assert rec.shape == (2, 1, 256, 256) and torch.isfinite(rec).all()
    ucfg = O.UNetConfig.from_params(up)
    yo = OS.DiffusionB(timesteps=1000, parameterization="v").ddim_sample(
        lambda xx, tt: O.plain_unet_forward(ucfg, usd, xx, tt), 2, xT[:1].cpu(), torch.zeros((2, 1, 4, 32, 32)),
        cond=[c["c_concat"][0][:1].cpu()], eta=0.0)
    assert rel_l2(y[:1], yo) < 1e-4


def test_dpm_latent_dynamic_thresholding_per_sample_over_all_channels(ldm):
    """dsd_sample_dpm with dynamic thresholding on a Cz = 4 state: the quantile is taken per sample over all C*h*w
    elements (dynamic_thresholding_fn, dpm_solver_pytorch.py:418), against oracle.dpm on the same network; a low threshold
    makes the clamp bite on every step."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    from util import dpm_case_betas
    g, ld, dd, embed, up, sd = ldm
    unet = ld.model.diffusion_model
    ucfg = O.UNetConfig.from_params(up)
    usd = {k[len("model.diffusion_model."):]: v for k, v in sd.items() if k.startswith("model.diffusion_model.")}
    cc = torch.from_numpy(g["c_concat"])
    xT = randn((2, 4, 8, 8), 641)
    betas = dpm_case_betas(("B", "betas"))
    ns = dsa.NoiseScheduleVP("discrete", **betas)
    kw = dict(steps=10, order=2, skip_type="time_uniform", lower_order_final=True)
    fn = lambda: dsa.model_wrapper(unet, ns, model_type="v", model_kwargs=dict(c_concat=[cc.cuda()]))
    y = dsa.DPM_Solver(fn(), ns, correcting_x0_fn="dynamic_thresholding", thresholding_max_val=0.05,
                       dynamic_thresholding_ratio=0.6).sample(xT.cuda(), **kw)
    net = lambda x, t: O.plain_unet_forward(ucfg, usd, torch.cat([x, cc], 1), t)
    want = ODPM.dpm_multistep(net, ODPM.NoiseSchedule(**betas), xT.clone(), model_type="v", thresholding=True, ratio=0.6,
                              max_val=0.05, **kw)
    assert rel_l2(y, want) < 1e-4
    plain = dsa.DPM_Solver(fn(), ns).sample(xT.cuda(), **kw)
    assert rel_l2(y, plain) > 1e-2                                     # the thresholding is active


def test_guided_diffusion_loop_routes_unet_model_to_latent_loop(ldm):
    """The guided-diffusion ddim_sample_loop / p_sample_loop handed a bare UNetModel with c_concat (no hooks) run
    dsd_sample, against oracle.samplers.DiffusionA with the same fed noise."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    from diffusion_models_dsdiff_amd import _lib
    g, ld, dd, embed, up, sd = ldm
    unet = ld.model.diffusion_model
    ucfg = O.UNetConfig.from_params(up)
    usd = {k[len("model.diffusion_model."):]: v for k, v in sd.items() if k.startswith("model.diffusion_model.")}
    cc = torch.from_numpy(g["c_concat"])
    zT, z = randn((2, 4, 8, 8), 651), randn((10, 2, 4, 8, 8), 652)
    d = create_gaussian_diffusion(steps=1000, timestep_respacing="10", rescale_timesteps=True, parameterization="v")
    od = OS.DiffusionA(steps=1000, timestep_respacing="10", rescale_timesteps=True, parameterization="v")
    net = lambda xx, tt: O.plain_unet_forward(ucfg, usd, xx, tt)
    L = _lib.lib()

    def graph_launches():
        caps, launches = C.c_int(), C.c_int()
        _lib.check(L.dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
        return launches.value
    before = graph_launches()
    _lib.check(L.dsd_set_graph(unet._h, 1))       # replayed graphs exist only in the device loop: the counter shows it ran
    try:
        y = d.ddim_sample_loop(unet, (2, 4, 8, 8), noise=zT.cuda(), clip_denoised=False, model_kwargs=dict(c_concat=[cc.cuda()]),
                               eta=1.0, step_noise=z.cuda())
        y2 = d.p_sample_loop(unet, (2, 4, 8, 8), noise=zT.cuda(), clip_denoised=False, model_kwargs=dict(c_concat=[cc.cuda()]),
                             step_noise=z.cuda())
        after = graph_launches()
    finally:
        _lib.check(L.dsd_set_graph(unet._h, 0))
    assert after > before
    assert rel_l2(y, od.ddim_sample_loop(net, zT, z, [cc], clip_denoised=False, eta=1.0)) < 1e-4
    assert rel_l2(y2, od.p_sample_loop(net, zT, z, [cc], clip_denoised=False)) < 1e-4


def test_init_from_ckpt_round_trip(ldm, tmp_path):
    """A reference-named checkpoint (with training-only extras) loads into a fresh LatentDiffusion by name; one that lacks the
    first stage's weights raises instead of leaving them at their initial values."""
    g, ld, dd, embed, up, sd = ldm
    ck = {k: v.detach().cpu() for k, v in ld.state_dict().items()}
    ck.update({"model_ema.decay": torch.tensor(0.999), "logvar": torch.zeros(1000)})
    path = tmp_path / "last.ckpt"
    torch.save({"state_dict": ck}, str(path))
    fresh = make_ldm(load=False)[1]
    missing, unexpected = fresh.init_from_ckpt(str(path))
    assert not missing and sorted(unexpected) == ["logvar", "model_ema.decay"]
    for k, v in fresh.state_dict().items():
        assert torch.equal(v.detach().cpu(), ck[k]), k
    x = randn((1, 1, 64, 64), 661).cuda()
    assert torch.equal(fresh.encode_first_stage(x).parameters, ld.encode_first_stage(x).parameters)
    bad = {("first_stage_model.vae." + k[len("first_stage_model."):] if k.startswith("first_stage_model.") else k): v
           for k, v in ck.items()}
    torch.save({"state_dict": bad}, str(path))
    with pytest.raises(KeyError, match="network weight"):
        fresh.init_from_ckpt(str(path))
