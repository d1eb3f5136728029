"""The DiT backbone (DSD_BLOCK_DIT) as a denoiser of the device sampling loops (GPU): the loops run it without a Python step,
bit for bit what a per-step loop over dsd_block_forward and the per-step ops computes; the chains against the oracle; graph
replay, first_step / n_steps segments, slice-keyed Philox noise; guidance, masks, PLMS and DDIM encode / decode through the
reference's sampler classes; the rejections.

PINNED BY THE REFERENCE: the network of every oracle chain is oracle/dit.py, which equals the reference's own DiT to the last
bit on the fixtures of tests/golden/dit.npz (tests/test_pinned_cpu.py), and one chain of that file — the reference's DDIMSampler
over the reference DiT of M3 — is run here on the device loop.  The fixtures rest on the reference's code and on
tests/golden/ref_standins.py: three timm modules (PatchEmbed, Attention, Mlp; timm is absent from the image), witnessed against
nn.MultiheadAttention and F.unfold.  The sampler arithmetic is the oracle's restatement of the reference loops
(oracle/samplers.py, oracle/dpm.py), held to the project's 1e-4 chain bar; the chains' conditioning is guarded in
tests/test_dit_loops_cpu.py.  Still unpinned: the rounding places of the half-precision modes and host_io.py's metrics."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import dit_loops_util as U
from util import rel_l2, randn

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's chain bar (BASELINE north star; every loop test)
STEPS = 4           # per-step comparisons: the first-order start, the second-order / history ramp and the steady state
_ENV = {}


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


def env(name):
    """DiffusionWrapper(DiT) inside an eps DDPMModel, weights of dit_loops_util; built once per model."""
    if name not in _ENV:
        from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
        _lib().require_gpu(0)
        kw, Cz, Cc = U.MODELS[name]
        m = DDPMModel(unet_config={"target": U.DIT_TARGET, "params": kw}, conditioning_key="concat", timesteps=1000,
                      parameterization="eps").cuda()
        unet = m.model.diffusion_model
        unet.load_state_dict(U.weights(name), strict=True)
        _ENV[name] = dict(name=name, m=m, wrap=m.model, unet=unet, Cz=Cz, Cc=Cc, S=kw["input_size"],
                          B={"M1": 2, "M2": 3, "M3": 2, "M4": 2}[name])
    return _ENV[name]


def data(e, B=None, seed=0):
    x, c = U.inputs(e["name"], B or e["B"], seed)
    return x.cuda(), c.cuda()


def noise(e, steps, B=None, seed=1700):
    return randn((steps, B or e["B"], e["Cz"], e["S"], e["S"]), seed).cuda()


def fwd(e, x_in, t):
    """One evaluation the way today's per-step path makes it: DiT.forward = dsd_block_forward on the concatenated input."""
    return e["unet"](x_in, torch.full((x_in.shape[0],), float(t), device="cuda"))


def diffusion(**kw):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, timestep_respacing=str(kw.pop("n", STEPS)), rescale_timesteps=True, **kw)


def ddim_sampler(e, steps=STEPS, eta=0.0):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(e["m"])
    s.make_schedule(steps, ddim_eta=eta, verbose=False)
    return s


def plms_sched(e, steps=STEPS):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    s = PLMSSampler(e["m"])
    s.make_schedule(steps, verbose=False)
    return s._schedule()


def dpm_solver(e, cond, uncond=None, scale=1.0):
    """DPM-Solver++ with dynamic thresholding over the respaced betas, as GaussianDiffusion.dpm_solver_sample_loop sets it up."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    ns = dsa.NoiseScheduleVP(schedule="discrete", betas=U.spaced_betas())
    kw = dict(model_kwargs=dict(c_concat=[cond])) if uncond is None else dict(
        guidance_type="classifier-free", condition=cond, unconditional_condition=uncond, guidance_scale=scale)
    return dsa.DPM_Solver(dsa.model_wrapper(e["wrap"], ns, model_type="noise", **kw), ns, algorithm_type="dpmsolver++",
                          correcting_x0_fn="dynamic_thresholding")


DPM_KW = dict(order=2, skip_type="logSNR", method="multistep", lower_order_final=False, denoise_to_zero=False, solver_type="dpmsolver")


def dpm_schedule(sol, steps=STEPS):
    return sol.build_schedule(steps, None, None, 2, "logSNR", False, False, "dpmsolver")


# ---------------------------------------------------------------------------------------- 1. the device loop is what runs
def test_reference_loops_run_on_the_device(monkeypatch):
    """p_sample_loop / ddim_sample_loop / dpm_solver_sample_loop on DiffusionWrapper(M1), the reference's call: no Python step
    calls DiT.forward (before the binding: one call per step through the generic-callable loop)."""
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import DiT
    e = env("M1")
    xT, c = data(e)
    calls = [0]
    forward = DiT.forward

    def counting(self, *a, **kw):
        calls[0] += 1
        return forward(self, *a, **kw)
    monkeypatch.setattr(DiT, "forward", counting)
    d = diffusion(learn_sigma=True)
    shape, kw = tuple(xT.shape), dict(model_kwargs=dict(c_concat=[c]), noise=xT)
    for y in (d.p_sample_loop(e["wrap"], shape, seed=5, **kw), d.ddim_sample_loop(e["wrap"], shape, **kw),
              d.dpm_solver_sample_loop(e["wrap"], shape, **kw)):
        assert y.shape == xT.shape and bool(torch.isfinite(y).all()) and not torch.equal(y, xT)
    assert calls[0] == 0


# ---------------------------------------------------------------------------------------- 2. bit identity with the per-step path
def _update_loop(e, sched, xT, c, z):
    from diffusion_models_dsdiff_amd._sched import sampler_update
    x = xT.clone()
    for k in range(sched.steps):
        sampler_update(sched, k, fwd(e, torch.cat([x, c], 1), sched.t_model[k]), x, z[k])
    return x


@pytest.mark.parametrize("body", ["ddpm_fixed", "ddpm_learned", "ddim_eta0", "ddim_eta05"])
@pytest.mark.parametrize("name", ["M1", "M2", "M3"])
def test_update_loops_equal_the_per_step_path(name, body):
    """DDPM (fixed and learned-range variance) and DDIM (eta 0, 0.5) of the guided-diffusion family with fed noise.  M2: two
    state channels inside a six-channel input, a four-channel output; M3: no conditioning, no variance half."""
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    e = env(name)
    xT, c = data(e)
    learned = body == "ddpm_learned"
    sched = diffusion(learn_sigma=learned)._schedule(body.startswith("ddim"), 0.5 if body == "ddim_eta05" else 0.0, True)
    z = noise(e, sched.steps)
    if learned and name == "M3":                        # no variance half to read: rejected, by message, the state untouched
        with pytest.raises(_lib().DsdError, match="learned-range variance needs 6 output channels .* the DiT has 3"):
            run_device_loop(e["unet"], sched, xT, c, step_noise=z)
        return
    dev = run_device_loop(e["unet"], sched, xT, c, step_noise=z)
    assert bool(torch.isfinite(dev).all()) and not torch.equal(dev, xT)
    assert torch.equal(dev, _update_loop(e, sched, xT, c, z))


def _dpm_loop(e, sc, xT, c, u=None, scale=1.0):
    """The per-step DPM loop: one sample is all Cz*H*W elements (the thresholding quantile), the output rows hold Cm of them."""
    L = _lib()
    B, Cz, H, W = xT.shape
    guided = u is not None
    x = (torch.cat([xT, xT]) if guided else xT.clone()).contiguous()
    cin = torch.cat([u, c]) if guided else c
    m_cur, m_prev = torch.empty_like(xT), torch.empty_like(xT)
    for k in range(sc.steps):
        out = fwd(e, torch.cat([x, cin], 1), sc.t_input[k]).contiguous()
        Cm = out.shape[1] // Cz
        if guided:
            L.check(L.lib().dsd_op_dpm_step_guided(C.byref(sc.c), k, L.dptr(out[:B]), L.dptr(out[B:]), Cm, float(scale), L.dptr(x), 0,
                                                   L.dptr(m_cur), L.dptr(m_prev), B, Cz, H, W, L.stream_ptr()))
        else:
            L.check(L.lib().dsd_op_dpm_step(C.byref(sc.c), k, L.dptr(out), Cm, L.dptr(x), L.dptr(m_cur), L.dptr(m_prev), B, Cz * H, W,
                                            L.stream_ptr()))
        m_cur, m_prev = m_prev, m_cur
    return x[:B]


@pytest.mark.parametrize("name", ["M1", "M2", "M3"])
def test_dpm_loop_equals_the_per_step_path(name):
    e = env(name)
    xT, c = data(e)
    sol = dpm_solver(e, c)
    dev = sol.sample(xT, steps=STEPS, **DPM_KW)
    assert bool(torch.isfinite(dev).all()) and torch.equal(dev, _dpm_loop(e, dpm_schedule(sol), xT, c))


def _plms_loop(e, sched, xT, c, u=None, scale=1.0):
    from diffusion_models_dsdiff_amd._sched import plms_step
    L = _lib()
    B, Cz = xT.shape[:2]
    guided = u is not None
    x = (torch.cat([xT, xT]) if guided else xT.clone()).contiguous()
    cin = torch.cat([u, c]) if guided else c
    hist = [torch.zeros_like(xT) for _ in range(3)]
    halves = lambda o: dict(out_uncond=o[:B, :Cz], out_cond=o[B:, :Cz], scale=scale) if guided else dict(out_cond=o[:, :Cz])
    for k in range(sched.steps):
        co = (sched.coef[k, 4], sched.coef[k, 5], sched.coef[k, 7])
        out = fwd(e, torch.cat([x, cin], 1), sched.t_model[k])
        if k == 0:
            plms_step(L.PLMS_PREDICT, *co, h_new=hist[0], x=x, x_saved=hist[1], **halves(out))
            out = fwd(e, torch.cat([x, cin], 1), sched.t_model[min(1, sched.steps - 1)])
            plms_step(L.PLMS_CORRECT, *co, h_new=hist[0], x=x, x_saved=hist[1], **halves(out))
        else:
            plms_step(min(k, 3) + 1, *co, h_new=hist[k % 3], x=x, o1=hist[(k + 2) % 3], o2=hist[(k + 1) % 3], **halves(out))
    return x[:B]


@pytest.mark.parametrize("name", ["M1", "M2", "M3"])
def test_plms_and_inversion_equal_the_per_step_path(name):
    """PLMS with S = 4 (predict / correct, then Adams-Bashforth 2, 3 and 4: the whole history ramp) and DDIM inversion."""
    from diffusion_models_dsdiff_amd._sched import ddim_invert_step, invert_coefficients, run_invert_loop, run_plms_loop
    e = env(name)
    xT, c = data(e)
    sched = plms_sched(e)
    dev = run_plms_loop(e["unet"], sched, xT, c)
    assert bool(torch.isfinite(dev).all()) and torch.equal(dev, _plms_loop(e, sched, xT, c))
    s = ddim_sampler(e, 5)
    coef = invert_coefficients(torch.from_numpy(np.asarray(s.ddim_alphas[:STEPS], dtype=np.float32)),
                               torch.tensor(np.asarray(s.ddim_alphas_prev[:STEPS], dtype=np.float64)))
    inv = run_invert_loop(e["unet"], coef, xT, c)
    x = xT.clone()
    for i in range(STEPS):                              # the model time of iteration i is i itself (ddim.py:282)
        ddim_invert_step(coef[i, 0], coef[i, 1], fwd(e, torch.cat([x, c], 1), i)[:, :e["Cz"]], x)
    assert bool(torch.isfinite(inv).all()) and not torch.equal(inv, xT) and torch.equal(inv, x)


@pytest.mark.parametrize("name", ["M1", "M2"])
def test_guided_and_masked_loops_equal_the_per_step_path(name):
    """Guided DDIM (eta 0.5, fed noise), guided DPM-Solver++ and guided PLMS evaluate 2B rows, uncond half first; the masked
    DDIM loop blends in front of every evaluation.  Both output halves are read through the 2*Cz-channel row stride."""
    from diffusion_models_dsdiff_amd._sched import (Guidance, Inpaint, mask_blend, run_device_loop, run_plms_loop, sampler_update,
                                                    sampler_update_guided)
    e = env(name)
    xT, c = data(e)
    B, Cz = xT.shape[:2]
    u = randn(tuple(c.shape), 1801).cuda()
    scale = 3.0
    sched = ddim_sampler(e, eta=0.5)._schedule(False, True)
    z = noise(e, sched.steps)
    dev = run_device_loop(e["unet"], sched, xT, c, step_noise=z, guidance=Guidance(u, scale, sched.steps))
    x2, cin = torch.cat([xT, xT]).contiguous(), torch.cat([u, c])
    for k in range(sched.steps):
        out = fwd(e, torch.cat([x2, cin], 1), sched.t_model[k])
        sampler_update_guided(sched, k, out[:B, :Cz], out[B:, :Cz], scale, x2, z[k])
    assert bool(torch.isfinite(dev).all()) and torch.equal(dev, x2[:B]) and torch.equal(x2[:B], x2[B:])
    plain = run_device_loop(e["unet"], sched, xT, c, step_noise=z)
    assert rel_l2(dev, plain) > 1e-3                                                   # the scale is not ignored
    # masked, unguided
    x0, mask, zb = randn(tuple(xT.shape), 1802).cuda(), (randn((B, 1) + tuple(xT.shape[2:]), 1803) > 0).float().cuda(), noise(e, sched.steps, seed=1804)
    dev = run_device_loop(e["unet"], sched, xT, c, step_noise=z, inpaint=Inpaint(x0, mask, zb))
    x = xT.clone()
    for k in range(sched.steps):
        mask_blend(sched.coef[k, 0], sched.coef[k, 1], x0, mask, x, zb[k])
        sampler_update(sched, k, fwd(e, torch.cat([x, c], 1), sched.t_model[k]), x, z[k])
    assert torch.equal(dev, x) and not torch.equal(dev, plain)
    # guided DPM-Solver++
    sol = dpm_solver(e, c, u, scale)
    dev = sol.sample(xT, steps=STEPS, **DPM_KW)
    sc = dpm_schedule(sol)
    assert bool(torch.isfinite(dev).all()) and torch.equal(dev, _dpm_loop(e, sc, xT, c, u, scale))
    # guided PLMS
    ps = plms_sched(e)
    dev = run_plms_loop(e["unet"], ps, xT, c, guidance=Guidance(u, scale, ps.steps))
    assert torch.equal(dev, _plms_loop(e, ps, xT, c, u, scale))


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_half_precision_loops_equal_the_per_step_path(prec):
    """M4 (heads of 64: the LDS-DMA attention kernel) in the single-product modes: the state, the updates and the model output
    stay fp32, so the bar is still equality, plus a finite result (the modes' accuracy: tests/test_half_gpu.py)."""
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    e = env("M4")
    xT, c = data(e)
    e["unet"].set_precision(prec)
    try:
        sol = dpm_solver(e, c)
        dev = sol.sample(xT, steps=STEPS, **DPM_KW)
        assert bool(torch.isfinite(dev).all()) and torch.equal(dev, _dpm_loop(e, dpm_schedule(sol), xT, c))
        sched = diffusion(learn_sigma=True)._schedule(False, 0.0, True)
        z = noise(e, sched.steps)
        dev = run_device_loop(e["unet"], sched, xT, c, step_noise=z)
        assert bool(torch.isfinite(dev).all()) and torch.equal(dev, _update_loop(e, sched, xT, c, z))
    finally:
        e["unet"].set_precision("bf16x6")


# ---------------------------------------------------------------------------------------- 3. against the oracle
@pytest.mark.parametrize("kind", U.CHAINS)
@pytest.mark.parametrize("name", ["M1", "M2"])
def test_chains_against_the_oracle(name, kind):
    """10 respaced steps, bf16x6, through the reference's entry points against oracle.samplers.DiffusionA / oracle.dpm with
    oracle.dit as the network.  M2's DDPM chain pins the multi-channel learned-range arithmetic."""
    e = env(name)
    B = U.CHAIN_BATCH[name]
    xT, c = data(e, B)
    d = diffusion(n=U.CHAIN_STEPS, learn_sigma=True)
    kw = dict(model_kwargs=dict(c_concat=[c]), noise=xT)
    if kind == "ddpm":
        got = d.p_sample_loop(e["wrap"], tuple(xT.shape), step_noise=U.chain_noise(name).cuda(), **kw)
    elif kind == "ddim":
        got = d.ddim_sample_loop(e["wrap"], tuple(xT.shape), eta=U.DDIM_ETA, step_noise=U.chain_noise(name).cuda(), **kw)
    else:
        got = d.dpm_solver_sample_loop(e["wrap"], tuple(xT.shape), **kw)
    err = rel_l2(got, U.oracle_chain_cached(name, kind))
    print(f"{name} {kind}: {U.CHAIN_STEPS}-step chain rel-L2 vs oracle {err:.3e}")
    assert err <= TOL


def test_ddim_chain_against_the_reference():
    """tests/golden/dit.npz: the reference's own DDIMSampler (ldm/models/diffusion/ddim.py) over the reference's own DiT in the
    layout of M3, 4 steps, eta 0 and eta 0.5 with fed noise, at the bar tests/test_latent_ldm_gpu.py holds its chains to.  The
    weights are the fixture's; M3's own come back afterwards."""
    import pinned_util as P
    from util import fixture_params
    g = P.fixture("dit")
    kw = P.cfg_of(g, "chain")
    assert kw == U.MODELS["M3"][0]
    e = env("M3")
    steps = int(g["chain_steps"])
    xT = randn((2, 3, 16, 16), int(g["chain_xT_seed"])).cuda()
    none = torch.zeros((2, 0, 16, 16), device="cuda")                  # M3 takes no conditioning
    e["unet"].load_state_dict(fixture_params(g, "chain"), strict=True)
    try:
        out = {}
        for key in ("chain_eta0", "chain_eta05"):
            eta = float(g[key + "_eta"])
            z = randn((steps,) + tuple(xT.shape), int(g[key + "_noise_seed"])).cuda()
            y, _ = ddim_sampler(e, steps, eta).sample(steps, 2, tuple(xT.shape[1:]), [none], eta=eta, verbose=False, x_T=xT,
                                                      step_noise=z)
            err = rel_l2(y, g[key + "_y"])
            print(f"M3 {key}: {steps}-step DDIM chain rel-L2 vs reference {err:.3e}")
            assert y.shape == g[key + "_y"].shape and err <= TOL, (key, err)
            out[key] = y
        assert rel_l2(out["chain_eta05"], out["chain_eta0"]) > 1e-2
    finally:
        e["unet"].load_state_dict(U.weights("M3"), strict=True)


# ---------------------------------------------------------------------------------------- 4. loop properties
def _slice_ids(unet, ids):
    L = _lib()
    arr = (C.c_int64 * max(1, len(ids)))(*ids)
    L.check(L.lib().dsd_set_slice_ids(unet._h, arr, len(ids)))


def test_segments_graph_replay_slice_ids_and_neutral_guidance():
    from diffusion_models_dsdiff_amd._sched import Guidance, run_device_loop, run_plms_loop
    L = _lib()
    e = env("M2")
    unet = e["unet"]
    xT, c = data(e)
    steps = 5                                           # uniform timesteps 1, 201 .. 801; iterations 3 and 4 are past the PLMS ramp
    sched = ddim_sampler(e, steps, eta=0.5)._schedule(False, True)
    ps = plms_sched(e, steps)
    assert sched.steps == steps and ps.steps == steps
    z = noise(e, steps)
    ddim = run_device_loop(unet, sched, xT, c, step_noise=z)
    plms = run_plms_loop(unet, ps, xT, c)
    # first_step / n_steps: after iteration 0, inside the PLMS history ramp, the rest
    x, y = xT, xT
    for first, n in ((0, 1), (1, 2), (3, 0)):
        x = run_device_loop(unet, sched, x, c, step_noise=z, first_step=first, n_steps=n)
        y = run_plms_loop(unet, ps, y, c, first_step=first, n_steps=n)
    assert torch.equal(x, ddim) and torch.equal(y, plms)
    # graph replay
    caps, launches = C.c_int(), C.c_int()
    L.check(L.lib().dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
    before = launches.value
    L.check(L.lib().dsd_set_graph(unet._h, 1))
    try:
        rep = [run_device_loop(unet, sched, xT, c, step_noise=z) for _ in range(2)]
        rep_plms = run_plms_loop(unet, ps, xT, c)
        L.check(L.lib().dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
    finally:
        L.check(L.lib().dsd_set_graph(unet._h, 0))
    assert launches.value > before and torch.equal(rep[0], ddim) and torch.equal(rep[1], ddim) and torch.equal(rep_plms, plms)
    # device-drawn noise keyed by slice id: a batch of 4 = two batches of 2
    x4, c4 = data(e, 4, seed=1)
    try:
        _slice_ids(unet, [0, 1, 2, 3])
        full = run_device_loop(unet, sched, x4, c4, seed=77)
        _slice_ids(unet, [0, 1])
        lo = run_device_loop(unet, sched, x4[:2], c4[:2], seed=77)
        _slice_ids(unet, [2, 3])
        hi = run_device_loop(unet, sched, x4[2:], c4[2:], seed=77)
    finally:
        _slice_ids(unet, [])
    assert torch.equal(full, torch.cat([lo, hi])) and not torch.equal(full[:, 0], full[:, 1])
    assert not torch.equal(full, run_device_loop(unet, sched, x4, c4, seed=78))
    # guidance with u == c is the unguided run
    assert torch.equal(run_device_loop(unet, sched, xT, c, step_noise=z, guidance=Guidance(c.clone(), 3.0, steps)), ddim)
    assert L.lib().dsd_device_bytes(unet._h) > 0


# ---------------------------------------------------------------------------------------- 5. today's refusals now run
def test_sampler_classes_run_a_dit():
    """DDIMSampler.sample guided and masked, PLMSSampler.sample, DDIMSampler.encode / decode on DiffusionWrapper(M1) inside the
    DDPMModel: each ran into 'no native denoiser' / 'device loop only' before.  Each differs from its plain twin by far more
    than any rounding, so an ignored scale or mask cannot pass."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    e = env("M1")
    m = e["m"]
    xT, c = data(e)
    B, shape = xT.shape[0], tuple(xT.shape[1:])
    S = 8
    plain, _ = DDIMSampler(m).sample(S, B, shape, [c], verbose=False, x_T=xT)
    guided, _ = DDIMSampler(m).sample(S, B, shape, [c], verbose=False, x_T=xT, unconditional_guidance_scale=3.,
                                      unconditional_conditioning=[torch.zeros_like(c)])
    x0 = randn(tuple(xT.shape), 1901).cuda()
    mask = torch.zeros((B, 1) + shape[1:], device="cuda")
    mask[:, :, :, : shape[2] // 2] = 1.
    masked, _ = DDIMSampler(m).sample(S, B, shape, [c], verbose=False, x_T=xT, mask=mask, x0=x0, seed=3)
    plms, _ = PLMSSampler(m).sample(S, B, shape, [c], verbose=False, x_T=xT)
    s = DDIMSampler(m)
    s.make_schedule(S, verbose=False)
    enc, _ = s.encode(plain, [c], S)
    dec = s.decode(enc, [c], S)
    for nm, y, twin in (("guided", guided, plain), ("masked", masked, plain), ("plms", plms, plain), ("encode", enc, plain),
                        ("decode", dec, enc)):
        d = rel_l2(y, twin)
        print(f"{nm}: rel-L2 to its twin {d:.3f}")
        assert y.shape == xT.shape and bool(torch.isfinite(y).all()) and d > 0.1, nm


# ---------------------------------------------------------------------------------------- 6. rejections
def test_rejections_by_message_leave_the_state_alone():
    from diffusion_models_dsdiff_amd import _sched
    L = _lib()
    e1, e2, e3 = env("M1"), env("M2"), env("M3")
    sched = diffusion()._schedule(True, 0.0, True)
    learned = diffusion(learn_sigma=True)._schedule(False, 0.0, True)

    def raw(e, sc, x, c, Cz):
        """dsd_sample itself, past the Python-side checks."""
        B, _, H, W = x.shape
        keep = x.clone()
        rc = L.lib().dsd_sample(e["unet"]._h, C.byref(sc.c), None, None, L.dptr(c), c.shape[1], L.dptr(x), Cz, None, C.c_uint64(1), B, H,
                                W, 0, 0, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and torch.equal(x, keep)
        return L.lib().dsd_last_error().decode()

    x, c = data(e1)
    big = randn((2, 1, 32, 32), 1).cuda()
    assert "the DiT takes 16x16 inputs (input_size) but the state is 32x32" in raw(e1, sched, big, randn((2, 3, 32, 32), 2).cuda(), 1)
    assert "the DiT takes 4 input channels but state + conditioning have 1 + 2" in raw(e1, sched, x, c[:, :2].contiguous(), 1)
    x2 = randn((2, 3, 16, 16), 3).cuda()                 # M2 as 3 state + 3 condition channels: 4 output channels fit neither
    assert "the DiT has 4 output channels but a state of 3 channels needs 3, or 6" in raw(e2, sched, x2, randn((2, 3, 16, 16), 4).cuda(), 3)
    x3, c3 = data(e3)
    assert "a learned-range variance needs 6 output channels (2 per state channel) but the DiT has 3" in raw(e3, learned, x3, c3, 3)
    # the Python-visible twins, raised before the library is entered
    keep = x.clone()
    with pytest.raises(ValueError, match="16x16 inputs"):
        _sched.run_device_loop(e1["unet"], sched, big, randn((2, 3, 32, 32), 2).cuda())
    with pytest.raises(ValueError, match="does not match the state"):
        _sched.run_device_loop(e1["unet"], sched, x, randn((2, 3, 8, 8), 2).cuda())
    with pytest.raises(ValueError, match="2 output channels; with 1 conditioning channels the state has 3, which needs 3 or 6"):
        _sched.run_device_loop(e1["unet"], sched, torch.cat([x, x, x], 1), c[:, :1].contiguous())
    with pytest.raises(ValueError, match="4 input channels but state \\+ conditioning have 2 \\+ 3"):
        _sched.run_device_loop(e1["unet"], sched, torch.cat([x, x], 1), c)
    assert torch.equal(x, keep)
    # a block that is neither denoiser keeps the UNetModel's message
    from diffusion_models_dsdiff_amd.blocks import AttentionBlock
    blk = AttentionBlock(32, num_heads=1)
    rc = L.lib().dsd_sample(blk._h, C.byref(sched.c), None, None, L.dptr(c), 3, L.dptr(x), 1, None, C.c_uint64(1), 2, 16, 16, 0, 0,
                            L.stream_ptr())
    assert rc != 0 and "the latent loops take a DSD_BLOCK_UNET handle (the plain UNetModel)" in L.lib().dsd_last_error().decode()
    assert torch.equal(x, keep)


def test_unet_rejections_keep_their_text():
    """A DSD_BLOCK_UNET call that was rejected before the DiT binding is rejected with the same text."""
    from diffusion_models_dsdiff_amd import _sched
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from util import golden
    L = _lib()
    L.require_gpu(0)
    unet = UNetModel(**json.loads(str(golden("plms")["lat_unet_cfg"])))        # 4 latent + 8 condition channels in, 4 out
    x, c = randn((2, 4, 8, 8), 1).cuda(), randn((2, 8, 8, 8), 2).cuda()
    sched = diffusion()._schedule(True, 0.0, True)
    learned = diffusion(learn_sigma=True)._schedule(False, 0.0, True)
    keep = x.clone()
    with pytest.raises(L.DsdError, match=r"learned-range variance needs one state channel \(the model output interleaves mean and "
                                         r"variance per sample\); Cz = 4"):
        _sched.run_device_loop(unet, learned, x, c)
    with pytest.raises(L.DsdError, match=r"the UNetModel takes 12 input channels but state \+ conditioning have 3 \+ 8"):
        _sched.run_device_loop(unet, sched, x[:, :3].contiguous(), c)
    with pytest.raises(L.DsdError, match="the UNetModel has 4 output channels but the sampler expects 2"):
        _sched.run_device_loop(unet, sched, x[:, :2].contiguous(), torch.cat([c, c[:, :2]], 1).contiguous())
    assert torch.equal(x, keep)


# ---------------------------------------------------------------------------------------- 7. the scalar path
def test_scalar_path_on_an_odd_sample_size():
    """15x15 with patch 3: a sample of 225 elements is no multiple of 4, so every update kernel takes V = 1 and the state rows
    inside the four-channel input are not 16-byte aligned.  The DiT handle takes the size (input_size % patch_size == 0 is all
    it asks), so the bits must equal the per-step path as above."""
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    _lib().require_gpu(0)
    kw = dict(U.MODELS["M1"][0], input_size=15, patch_size=3)
    wrap = DiffusionWrapper({"target": U.DIT_TARGET, "params": kw}, "concat")
    unet = wrap.diffusion_model
    unet.load_state_dict(U.synth_params(U.names_shapes(kw), U.WEIGHT_SEED), strict=True)
    e = dict(unet=unet, wrap=wrap, Cz=1, Cc=3, S=15, B=3, name="odd")
    xT, c = randn((3, 1, 15, 15), 2001).cuda(), randn((3, 3, 15, 15), 2002).cuda()
    sched = diffusion(learn_sigma=True)._schedule(False, 0.0, True)
    z = noise(e, sched.steps)
    dev = run_device_loop(unet, sched, xT, c, step_noise=z)
    assert bool(torch.isfinite(dev).all()) and torch.equal(dev, _update_loop(e, sched, xT, c, z))
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    ns = dsa.NoiseScheduleVP(schedule="discrete", betas=U.spaced_betas())
    sol = dsa.DPM_Solver(dsa.model_wrapper(wrap, ns, model_type="noise", model_kwargs=dict(c_concat=[c])), ns,
                         algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")
    assert torch.equal(sol.sample(xT, steps=STEPS, **DPM_KW), _dpm_loop(e, dpm_schedule(sol), xT, c))


# ---------------------------------------------------------------------------------------- 8. what the loops do not carry
def test_labels_and_cond_kwargs_keep_the_per_step_path(monkeypatch):
    """A class-conditional DiT sampled with model_kwargs=dict(y=labels), or with DiT.forward's own cond=, is not a case of the
    device loops (they pass the network its input and t only): the per-step path runs it, one forward per step, and the labels
    reach the network."""
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import DiT
    _lib().require_gpu(0)
    kw = dict(U.MODELS["M1"][0], num_classes=3)
    m = DiT(**kw)
    m.load_state_dict(U.synth_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], U.WEIGHT_SEED), strict=True)
    calls = [0]
    forward = DiT.forward

    def counting(self, *a, **k):
        calls[0] += 1
        return forward(self, *a, **k)
    monkeypatch.setattr(DiT, "forward", counting)
    d = diffusion(learn_sigma=True)
    xT, c = randn((2, 1, 16, 16), 2101).cuda(), randn((2, 3, 16, 16), 2102).cuda()
    z = randn((STEPS, 2, 1, 16, 16), 2103).cuda()
    run = lambda **mk: d.p_sample_loop(m, (2, 1, 16, 16), noise=xT, step_noise=z, model_kwargs=mk)
    a = run(cond=c, y=torch.tensor([0, 1]).cuda())
    assert calls[0] == STEPS
    b = run(cond=c, y=torch.tensor([2, 1]).cuda())
    assert not torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])              # the labels reached the network
    calls[0] = 0
    plain = run(cond=c)                                                         # forward's own concat argument: per step
    assert calls[0] == STEPS
    assert torch.equal(plain, run(c_concat=[c])) and calls[0] == STEPS          # the same chain in the device loop: no forward
