"""CPU side of classifier-free guidance (tests/golden/cfg.npz, tests/golden/gen_cfg.py): the reference's guided DDIM /
DPM-Solver++ chains reproduced by the oracle networks plus a guided step restated here in fp32 torch — which pins the fixture to
the reference and the combine orders the device kernels follow — and the argument-form checks of the three Python surfaces,
which raise before any GPU call."""
import json

import numpy as np
import pytest
import torch

from oracle import dpm as ODPM, samplers as OS, schedules as S, unet as O
from util import golden, fixture_params, rel_l2, randn, cond_image

STEPS = 20
TOL = 1e-5        # the bar of test_latent_ldm_cpu.py for its chains


# ---------------------------------------------------------------------------------------- the guided step, restated
def guided_ddim_net(net, c, u, scales):
    """ddim.py:194-219: one 2B pass on x_in = cat([x]*2), c_in = cat([u, c]); out = out_u + s * (out_c - out_u) on the raw
    outputs.  A step whose scale is exactly 1.0 takes the unguided branch (:194)."""
    k = [0]

    def f(x, t):
        s = float(scales[k[0]])
        k[0] += 1
        if s == 1.:
            return net(torch.cat([x, c], 1), t)
        out_u, out_c = net(torch.cat([torch.cat([x] * 2), torch.cat([u, c])], 1), torch.cat([t] * 2)).chunk(2)
        return out_u + s * (out_c - out_u)
    return f


def guided_dpm_net(net, ns, c, u, scale, steps, model_type="v"):
    """dpm_solver_pytorch.py:283-299,324-332: each half becomes a noise prediction from its own output and the shared x_t, then
    noise = noise_u + s * (noise_c - noise_u).  Evaluation k happens at time ts[k] of the time_uniform grid."""
    ts = ODPM.time_steps(ns, "time_uniform", ns.T, 1. / ns.total_N, steps)
    k = [0]

    def f(x, t_input):
        tc = ts[k[0]].expand(2 * x.shape[0])
        k[0] += 1
        x_in = torch.cat([x] * 2)
        out = net(torch.cat([x_in, torch.cat([u, c])], 1), torch.cat([t_input] * 2))
        a, sg = ns.alpha(tc)[:, None, None, None], ns.std(tc)[:, None, None, None]
        if model_type == "v":
            out = a * out + sg * x_in
        elif model_type == "x_start":
            out = (x_in - a * out) / sg
        nu, nc = out.chunk(2)
        return nu + scale * (nc - nu)
    return f


def _latent():
    g, gl = golden("cfg"), golden("latent_ldm")
    up = json.loads(str(g["lat_unet_cfg"]))
    assert up == json.loads(str(gl["unet_cfg"]))
    ucfg, usd = O.UNetConfig.from_params(up), fixture_params(gl, "unet")
    net = lambda xx, tt: O.plain_unet_forward(ucfg, usd, xx, tt)
    c = randn((2, 8, 8, 8), int(g["lat_c_seed"]))
    return g, net, c, torch.zeros_like(c), randn((2, 4, 8, 8), int(g["lat_xT_seed"]))


def _pixel():
    g, gm = golden("cfg"), golden("model")
    cfg, sd = O.UNetConfig.from_params(json.loads(str(gm["tiny_cfg"]))), fixture_params(gm, "tiny")
    net = lambda xx, tt: O.unet_forward(cfg, sd, xx, tt)[0]
    c = cond_image((2, 1, 32, 32), int(g["pix_cond_seed"]))
    return g, net, c, torch.zeros_like(c), randn((2, 1, 32, 32), int(g["pix_xT_seed"]))


def _ns():
    return ODPM.NoiseSchedule(betas=torch.tensor(S.make_beta_schedule("linear", 1000, 1e-4, 2e-2), dtype=torch.float32))


@pytest.mark.parametrize("space", ["lat", "pix"])
def test_oracle_reproduces_guided_ddim(space):
    g, net, c, u, xT = _latent() if space == "lat" else _pixel()
    od = OS.DiffusionB(timesteps=1000, parameterization="v")
    scale = float(g["scale"])
    for key, eta in (("ddim_eta0", 0.0), ("ddim_eta1", 1.0)):
        z = randn((STEPS,) + tuple(xT.shape), int(g[f"{space}_{key}_noise_seed"]))
        for suffix, sc in (("_y", scale), ("_s1_y", 1.0)):
            y = od.ddim_sample(guided_ddim_net(net, c, u, [sc] * STEPS), STEPS, xT.clone(), z, eta=eta)
            assert rel_l2(y, g[f"{space}_{key}{suffix}"]) < TOL, (space, key, suffix)
        assert rel_l2(g[f"{space}_{key}_y"], g[f"{space}_{key}_s1_y"]) > 1e-2        # the fixture is guided
    if space == "lat":
        z = randn((STEPS,) + tuple(xT.shape), int(g["lat_ddim_eta0_noise_seed"]))
        ucg = g["ucg_schedule"]
        assert ucg.shape == (STEPS,) and ucg[0] == 1.0 and ucg[-1] == 4.0
        y = od.ddim_sample(guided_ddim_net(net, c, u, ucg), STEPS, xT.clone(), z, eta=0.0)
        assert rel_l2(y, g["lat_ddim_ucg_y"]) < TOL


@pytest.mark.parametrize("space", ["lat", "pix"])
def test_oracle_reproduces_guided_dpm_solver(space):
    g, net, c, u, xT = _latent() if space == "lat" else _pixel()
    ns = _ns()
    kw = dict(steps=STEPS, order=2, skip_type="time_uniform")
    y = ODPM.dpm_multistep(guided_dpm_net(net, ns, c, u, float(g["scale"]), STEPS), ns, xT.clone(), model_type="noise", **kw)
    assert rel_l2(y, g[space + "_dpm_y"]) < TOL
    y1 = ODPM.dpm_multistep(lambda xx, tt: net(torch.cat([xx, c], 1), tt), ns, xT.clone(), model_type="v", **kw)
    assert rel_l2(y1, g[space + "_dpm_s1_y"]) < TOL
    assert rel_l2(g[space + "_dpm_y"], g[space + "_dpm_s1_y"]) > 1e-2


# ---------------------------------------------------------------------------------------- argument forms (no GPU call)
def _ddpm():
    from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
    return DDPMModel(timesteps=1000, parameterization="v")


def test_ddim_sampler_argument_forms():
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    sm = DDIMSampler(_ddpm())
    c, xT = torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8)
    run = lambda cond, u, **kw: sm.sample(4, 2, (1, 8, 8), cond, verbose=False, x_T=xT, unconditional_conditioning=u, **kw)
    # the unconditional conditioning comes in the form of the conditioning (ddim.py:199-217)
    with pytest.raises(AssertionError, match="dict"):
        run(dict(c_concat=[c]), c, unconditional_guidance_scale=3.)
    with pytest.raises(AssertionError, match="list"):
        run(dict(c_concat=[c]), dict(c_concat=c), unconditional_guidance_scale=3.)
    with pytest.raises(AssertionError, match="list"):
        run([c], c, unconditional_guidance_scale=3.)
    with pytest.raises(AssertionError, match="tensor"):
        run(c, [c], unconditional_guidance_scale=3.)
    with pytest.raises(AssertionError):
        run(c, c, ucg_schedule=[1., 2., 3.])                              # one scale per executed step (:166)
    for cond, u in ((dict(c_concat=[c]), dict(c_concat=[c[:, :, :4]])), ([c], [c[:1]]), (c, c.double())):
        with pytest.raises(ValueError, match="shape, dtype and device"):
            run(cond, u, unconditional_guidance_scale=3.)
    # guidance is off without an unconditional conditioning or at scale 1.0 (:194): the unguided path, which finds no network here
    for kw in (dict(u=None, unconditional_guidance_scale=3.), dict(u=c[:1], unconditional_guidance_scale=1.)):
        with pytest.raises(RuntimeError, match="no native denoiser"):
            run(c, **kw)
    with pytest.raises(RuntimeError, match="no native denoiser"):
        run(c, c, unconditional_guidance_scale=3.)                        # well-formed: reaches the loop
    for bad in (dict(mask=c), dict(quantize_x0=True), dict(score_corrector=object()), dict(dynamic_threshold=0.9),
                dict(temperature=0.5), dict(noise_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            run(c, c, unconditional_guidance_scale=3., **bad)


def test_dpm_solver_sampler_and_model_wrapper_argument_forms():
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.dpm_solver_new.sampler import DPMSolverSampler
    c, xT = torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8)
    sm = DPMSolverSampler(_ddpm())
    with pytest.raises(AssertionError, match="form of the conditioning"):
        sm.sample(4, 2, (1, 8, 8), c, x_T=xT, unconditional_guidance_scale=3., unconditional_conditioning=[c])
    with pytest.raises(AssertionError, match="dict"):
        sm.sample(4, 2, (1, 8, 8), dict(c_concat=[c]), x_T=xT, unconditional_guidance_scale=3., unconditional_conditioning=c)
    with pytest.raises(NotImplementedError, match="device loop only"):        # no native network behind this model
        sm.sample(4, 2, (1, 8, 8), c, x_T=xT, unconditional_guidance_scale=3., unconditional_conditioning=c)
    ns = dsa.NoiseScheduleVP("discrete", betas=torch.tensor(S.make_beta_schedule("linear", 1000), dtype=torch.float32))
    with pytest.raises(NotImplementedError, match="classifier guidance"):
        dsa.model_wrapper(lambda x, t: x, ns, guidance_type="classifier", classifier_fn=lambda *a: None)
    with pytest.raises(ValueError, match="needs the condition"):
        dsa.model_wrapper(lambda x, t: x, ns, guidance_type="classifier-free", unconditional_condition=c, guidance_scale=3.)
    # off at scale 1.0 or without the unconditional condition (dpm_solver_pytorch.py:325)
    assert dsa.model_wrapper(lambda x, t, cc: x, ns, guidance_type="classifier-free", condition=c, unconditional_condition=c,
                             guidance_scale=1.).unconditional_condition is None
    assert dsa.model_wrapper(lambda x, t, cc: x, ns, guidance_type="classifier-free", condition=c,
                             guidance_scale=3.).unconditional_condition is None
    net = lambda x, t, cc: x
    fn = dsa.model_wrapper(net, ns, model_type="v", guidance_type="classifier-free", condition=dict(c_concat=[c]),
                           unconditional_condition=dict(c_concat=[c[:, :, :4]]), guidance_scale=3.)
    assert fn.unconditional_condition is not None and fn.guidance_scale == 3.
    with pytest.raises(ValueError, match="shape, dtype and device"):
        dsa.DPM_Solver(fn, ns).sample(xT, steps=4)
    fn = dsa.model_wrapper(net, ns, model_type="v", guidance_type="classifier-free", condition=c, unconditional_condition=c,
                           guidance_scale=3.)
    with pytest.raises(NotImplementedError, match="device loop only"):        # well-formed, but no native network to run it
        dsa.DPM_Solver(fn, ns).sample(xT, steps=4)
    with pytest.raises(NotImplementedError, match="device loop"):
        fn(xT, torch.ones(2))


def test_run_device_loop_guidance_checks():
    from diffusion_models_dsdiff_amd._sched import Guidance, guidance_active
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    sm = DDIMSampler(_ddpm())
    sm.make_schedule(4, verbose=False)
    sched = sm._schedule(False, True)
    c, xT = torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8)
    g = Guidance(c, 3., 4)
    assert g.scale.dtype == np.float32 and g.scale.tolist() == [3.] * 4
    assert Guidance(c, np.linspace(1., 4., 4), 4).scale.tolist() == [1., 2., 3., 4.]
    with pytest.raises(ValueError, match="scales"):
        Guidance(c, [1., 2.], 4)
    with pytest.raises(ValueError, match="scales"):
        run_device_loop(None, sched, xT, c, guidance=Guidance(c, 3., 5))
    for u in (c[:, :, :4], c.double(), None):
        with pytest.raises(ValueError):
            run_device_loop(None, sched, xT, c, guidance=Guidance(u, 3., 4))
    assert guidance_active(3., c) and guidance_active(1., c, [1.] * 4)
    assert not guidance_active(3., None) and not guidance_active(1., c) and not guidance_active(1., None, [2.] * 4)


def test_guidance_struct_and_header_agree():
    import ctypes as C
    import os
    import re
    from diffusion_models_dsdiff_amd import _lib
    assert C.sizeof(_lib.DsdGuidance) == 24 and _lib.DsdGuidance.scale.offset == 8 and _lib.DsdGuidance.n_scale.offset == 16
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsdiff.h")).read()
    for sym in ("dsd_sample", "dsd_sample_dpm", "dsd_op_sampler_update_guided", "dsd_op_dpm_step_guided"):
        assert sym in _lib.EXPORTS and re.search(r"\bint %s\(" % sym, hdr), sym
