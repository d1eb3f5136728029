"""The samplers' intermediates and per-step callbacks on the device (GPU): every entry of tests/golden/trace.npz (the reference's
own DDIMSampler / PLMSSampler / p_sample_loop / progressive_denoising, tests/golden/gen_trace.py) through the public methods, the
callbacks' arguments, then dsd_set_trace itself: traced, segmented and graph-replayed runs against the plain run bit for bit,
x[j] against a run stopped after keep[j] + 1 steps, split runs, pred_x0 against the update op on the module's own forward (the
four-stream model, the UNetModel, a learned-range DiT, the DisC-Diff network), the sentinel, the rejections, log_images."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from util import golden, fixture_params, rel_l2, randn, cond_image
from test_img2img_cpu import center_mask
from test_trace_cpu import cases, entries

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's chain bar (test_plms_gpu.py, test_img2img_gpu.py), here per entry
TOL_OP = 1e-6       # same arithmetic, other tiling (test_plms_gpu.py, test_img2img_gpu.py)
G = golden("trace")
ALL = [(sp, n) for sp in ("lat", "pix") for n in cases(sp)]


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------- models
@pytest.fixture(scope="module")
def pix():
    """The `tiny` DSUnetModel of model.npz behind a DiffusionWrapper inside an eps DDPMModel; cond / x_T of loops.npz, u = zeros."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
    _lib().require_gpu(0)
    gm = golden("model")
    wrap = DiffusionWrapper({"target": "UNet_DS_Diff.model.DSUnetModel", "params": json.loads(str(gm["tiny_cfg"]))}, "concat")
    wrap.diffusion_model.load_state_dict(fixture_params(gm, "tiny"), strict=True)
    m = DDPMModel(timesteps=1000, parameterization="eps").cuda()
    m.model = wrap
    shape = (2, 1, 32, 32)
    c = cond_image(shape, int(G["pix_cond_seed"])).cuda()
    return dict(m=m, wrap=wrap, unet=wrap.diffusion_model, c=c, u=torch.zeros_like(c), xT=randn(shape, int(G["pix_xT_seed"])).cuda(),
                x0=randn(shape, int(G["x0_seed"])).cuda(), mask=center_mask(shape).cuda(), key="pix")


@pytest.fixture(scope="module")
def lat():
    """The latent UNetModel of latent_ldm.npz inside an eps LatentDiffusion with the fixture's first stage; c = randn, u = zeros."""
    from diffusion_models_dsdiff_amd.ldm.models.autoencoder import AutoencoderKL
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    _lib().require_gpu(0)
    gl = golden("latent_ldm")
    dd = json.loads(str(gl["vae_cfg"]))
    embed = dd.pop("embed_dim")
    ld = LatentDiffusion(first_stage_config=AutoencoderKL(dd, None, embed), conditioning_key="concat", scale_factor=0.18215,
                         timesteps=1000, parameterization="eps", image_size=8, channels=4,
                         unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                                      "params": json.loads(str(G["lat_unet_cfg"]))})
    ld.load_state_dict(fixture_params(gl, "vae", "first_stage_model."), strict=False)
    ld.model.diffusion_model.load_state_dict(fixture_params(gl, "unet"), strict=True)
    ld = ld.cuda()
    shape = (2, 4, 8, 8)
    c = randn((2, 8, 8, 8), int(G["lat_c_seed"])).cuda()
    return dict(m=ld, wrap=ld.model, unet=ld.model.diffusion_model, c=c, u=torch.zeros_like(c),
                xT=randn(shape, int(G["lat_xT_seed"])).cuda(), x0=randn(shape, int(G["x0_seed"])).cuda(),
                mask=center_mask(shape).cuda(), key="lat")


def _noise(e, seed, steps):
    return randn((steps,) + tuple(e["xT"].shape), int(seed)).cuda()


def _ddpm_sched(e, T):
    """B_DDPM over t = T-1 .. 0 of the 1000-step tables, clipped for the pixel model (DDPM's default) and not for the latent one."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion._schedule(e["m"], T)


# ---------------------------------------------------------------------------------------- 1. the fixture, through the public methods
def run_case(e, case, callbacks=True):
    """A fixture case through the drop-in -> dict(y, x, p0, cb, icb, seen); ``x`` / ``p0`` without the leading x_T."""
    from diffusion_models_dsdiff_amd._sched import StepCallbacks, Trace, kept_iterations, run_device_loop
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    kind, steps, log = case["kind"], case["executed"], case["log"]
    cb, icb, seen = [], [], []
    kw = {}
    if callbacks:
        kw = dict(callback=lambda i: cb.append(int(i)), img_callback=lambda t, i: (icb.append(int(i)), seen.append(t)))
    masked = bool(case.get("mask"))
    mk = dict(mask=e["mask"], x0=e["x0"], mask_noise=_noise(e, G["blend_seed"], steps)) if masked else {}
    shape = tuple(e["xT"].shape)
    if kind in ("ddim", "plms"):
        e["m"].parameterization = case.get("param", "eps")
        try:
            common = dict(verbose=False, x_T=e["xT"], log_every_t=log, unconditional_guidance_scale=case.get("scale", 1.), **mk, **kw)
            if kind == "ddim":
                y, inter = DDIMSampler(e["m"]).sample(case["steps"], 2, shape[1:], dict(c_concat=[e["c"]]), eta=case.get("eta", 0.),
                                                      unconditional_conditioning=dict(c_concat=[e["u"]]),
                                                      step_noise=_noise(e, G["step_seed"], steps), **common)
            else:
                y, inter = PLMSSampler(e["m"]).sample(case["steps"], 2, shape[1:], e["c"], unconditional_conditioning=e["u"],
                                                      dynamic_threshold=case.get("thr"), **common)
        finally:
            e["m"].parameterization = "eps"
        assert inter["x_inter"][0] is e["xT"] and inter["pred_x0"][0] is e["xT"]
        x, p0 = inter["x_inter"][1:], inter["pred_x0"][1:]
    elif e["key"] == "lat":
        args = dict(x_T=e["xT"], verbose=False, log_every_t=log, step_noise=_noise(e, G["step_seed"], steps), **mk, **kw)
        if kind == "ddpm":
            y, inter = e["m"].p_sample_loop(e["c"], shape, return_intermediates=True, timesteps=steps, **args)
            assert inter[0] is e["xT"]
            x, p0 = inter[1:], []
        else:
            y, p0 = e["m"].progressive_denoising(e["c"], shape, start_T=steps, **args)
            x = []
    else:   # the pixel model sits in the trainer's DDPMModel, whose loop always runs all 1000 steps: the driver, on 12
        sched = _ddpm_sched(e, steps)
        from diffusion_models_dsdiff_amd._sched import Inpaint
        tr = Trace(kept_iterations(steps, log), x=kind == "ddpm", pred_x0=kind == "prog")
        cbs = StepCallbacks(kw.get("callback"), kw.get("img_callback"), index=lambda k: steps - 1 - k, image="x")
        y = run_device_loop(e["unet"], sched, e["xT"], e["c"], step_noise=_noise(e, G["step_seed"], steps), trace=tr, callbacks=cbs,
                            inpaint=Inpaint(mk["x0"], mk["mask"], mk["mask_noise"]) if masked else None)
        x, p0 = tr.states, tr.pred_x0s
    return dict(y=y, x=x, p0=p0, cb=cb, icb=icb, seen=seen)


@pytest.mark.parametrize("space,name", ALL, ids=[f"{s}_{n}" for s, n in ALL])
def test_entries_and_callbacks_vs_reference(space, name, request):
    e = request.getfixturevalue(space)
    case = cases(space)[name]
    r = run_case(e, case)
    for part in ("x", "p0"):
        want = entries(space, name, part)
        assert len(r[part]) == len(want), (part, len(r[part]), len(want))
        for j, (a, b) in enumerate(zip(r[part], want)):
            err = rel_l2(a, b)
            print(f"{space}_{name} {part}{j}: rel-L2 to the reference {err:.3e}")
            assert tuple(a.shape) == tuple(b.shape) and err < TOL, (part, j, err)
    if r["x"]:
        assert torch.equal(r["x"][-1], r["y"])                                # the last kept state is the sample
    else:
        assert rel_l2(r["y"], G[f"{space}_{name}_y"]) < TOL
    # the callbacks: the reference's argument sequences, callback before img_callback, the tensors at two steps
    assert r["cb"] == G[f"{space}_{name}_cb"].tolist() and r["icb"] == G[f"{space}_{name}_icb"].tolist()
    for k in (1, case["executed"] - 1):
        err = rel_l2(r["seen"][k], G[f"{space}_{name}_icb{k}"])
        print(f"{space}_{name} img_callback tensor of iteration {k}: rel-L2 to the reference {err:.3e}")
        assert err < TOL
    # without callbacks the loop runs in one call with the trace installed: the same bits, entry by entry
    q = run_case(e, case, callbacks=False)
    assert torch.equal(q["y"], r["y"])
    for part in ("x", "p0"):
        assert len(q[part]) == len(r[part]) and all(torch.equal(a, b) for a, b in zip(q[part], r[part])), part


def test_progressive_denoising_rejects_by_name(lat):
    e = lat
    for bad, word in ((dict(temperature=0.5), "temperature"), (dict(noise_dropout=0.1), "noise_dropout")):
        with pytest.raises(NotImplementedError, match=word):
            e["m"].progressive_denoising(e["c"], tuple(e["xT"].shape), x_T=e["xT"], start_T=2, **bad)


# ---------------------------------------------------------------------------------------- 2. dsd_set_trace under the driver
def _mode(e, mode):
    """(run(**kw) -> sample, steps) of a driver-level loop: guided DDIM with eta 1 and fed noise, masked thresholded PLMS, masked
    DDPM.  Five or six iterations: PLMS's predictor / corrector start, its history ramp and the steady state."""
    from diffusion_models_dsdiff_amd._sched import Guidance, Inpaint, run_device_loop, run_plms_loop
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    if mode == "ddim_cfg":
        s = DDIMSampler(e["m"])
        s.make_schedule(5, ddim_eta=1.0, verbose=False)
        sched = s._schedule(False, True)
        z = _noise(e, 811, sched.steps)
        return (lambda **kw: run_device_loop(e["unet"], sched, e["xT"], e["c"], step_noise=z, guidance=Guidance(e["u"], 3.0, sched.steps),
                                             **kw)), sched.steps
    if mode == "plms_thr_mask":
        s = PLMSSampler(e["m"])
        s.make_schedule(5, verbose=False)
        sched = s._schedule()
        zb = _noise(e, 812, sched.steps)
        return (lambda **kw: run_plms_loop(e["unet"], sched, e["xT"], e["c"], threshold=2.0, inpaint=Inpaint(e["x0"], e["mask"], zb),
                                           **kw)), sched.steps
    sched = _ddpm_sched(e, 6)
    z, zb = _noise(e, 813, 6), _noise(e, 814, 6)
    return (lambda **kw: run_device_loop(e["unet"], sched, e["xT"], e["c"], step_noise=z, inpaint=Inpaint(e["x0"], e["mask"], zb), **kw)), 6


@pytest.mark.parametrize("mode", ["ddim_cfg", "plms_thr_mask", "ddpm_mask"])
@pytest.mark.parametrize("space", ["lat", "pix"])
def test_traced_segmented_replayed_and_split_runs(space, mode, request):
    """lat: the state lives strided inside the denoiser's input (2B rows under guidance); pix: dense planes (cfg_io when guided)."""
    from diffusion_models_dsdiff_amd._sched import StepCallbacks, Trace
    e = request.getfixturevalue(space)
    run, steps = _mode(e, mode)
    plain = run()
    assert bool(torch.isfinite(plain).all()) and not torch.equal(plain, e["xT"])
    full = Trace(range(steps))                                                # n_keep = steps
    assert torch.equal(run(trace=full), plain)
    assert len(full.states) == len(full.pred_x0s) == steps and torch.equal(full.states[-1], plain)
    assert all(tuple(t.shape) == tuple(e["xT"].shape) for t in full.states + full.pred_x0s)
    one = Trace([2])                                                          # n_keep = 1
    assert torch.equal(run(trace=one), plain)
    assert torch.equal(one.states[0], full.states[2]) and torch.equal(one.pred_x0s[0], full.pred_x0s[2])
    # snapshot self-consistency: x[j] is the state of a run stopped after keep[j] + 1 steps (guided: its conditional half)
    for k in range(steps):
        assert torch.equal(run(n_steps=k + 1), full.states[k]), k
    # segmented by callbacks
    seen = []
    seg = Trace([0, steps - 1])
    y = run(trace=seg, callbacks=StepCallbacks(lambda i: seen.append(i), lambda t, i: seen.append(t), image="pred_x0"))
    assert torch.equal(y, plain) and seen[0::2] == list(range(steps))
    assert all(torch.equal(t, full.pred_x0s[k]) for k, t in enumerate(seen[1::2]))
    assert torch.equal(seg.states[0], full.states[0]) and torch.equal(seg.pred_x0s[1], full.pred_x0s[-1])
    # graph replay: the snapshots lie outside the cached network graph
    L = _lib()
    L.check(L.lib().dsd_set_graph(e["unet"]._h, 1))
    try:
        rep = Trace(range(steps))
        for _ in range(2):                                                    # capture, then replay
            assert torch.equal(run(trace=rep), plain)
            assert torch.equal(rep.x, full.x) and torch.equal(rep.pred_x0, full.pred_x0)
    finally:
        L.check(L.lib().dsd_set_graph(e["unet"]._h, 0))
    # a run split in two windows fills the same buffers; the first window holds no kept iteration
    sp = Trace([3, steps - 1])
    sp.alloc(e["xT"])
    sp.x.fill_(7.), sp.pred_x0.fill_(7.)
    mid = run(trace=sp, first_step=0, n_steps=3)
    assert bool((sp.x == 7.).all()) and bool((sp.pred_x0 == 7.).all()) and sp.states == []
    mid_run, _ = _mode(dict(e, xT=mid), mode)
    assert torch.equal(mid_run(trace=sp, first_step=3), plain)
    assert torch.equal(sp.x[0], full.states[3]) and torch.equal(sp.x[1], plain)
    assert torch.equal(sp.pred_x0[0], full.pred_x0s[3]) and torch.equal(sp.pred_x0[1], full.pred_x0s[-1])


def test_no_trace_leaves_a_sentinel_untouched(lat):
    from diffusion_models_dsdiff_amd._sched import trace_set
    e = lat
    run, steps = _mode(e, "ddim_cfg")
    buf = torch.full((2, steps) + tuple(e["xT"].shape), 7., device="cuda")
    plain = run()                                                             # never set
    with trace_set(e["unet"], list(range(steps)), buf[0], buf[1]):
        pass                                                                  # set and cleared
    assert torch.equal(run(), plain)
    torch.cuda.synchronize()
    assert bool((buf == 7.).all())
    with trace_set(e["unet"], [1], buf[0], None):                             # x alone: one slot written, pred_x0 stays
        assert torch.equal(run(), plain)
    assert not bool((buf[0, 0] == 7.).any()) and bool((buf[0, 1:] == 7.).all()) and bool((buf[1] == 7.).all())


# ---------------------------------------------------------------------------------------- 3. pred_x0 against the update op
def _host_loop(fwd, sched, xT, c, z):
    """The per-step path: the module's own forward, then the fused update with its pred_xstart output."""
    from diffusion_models_dsdiff_amd._sched import sampler_update
    x, xs, p0s = xT.clone(), [], []
    for k in range(sched.steps):
        out = fwd(torch.cat([x, c], 1), sched.t_model[k])
        p0s.append(sampler_update(sched, k, out, x, z[k], want_x0=True))
        xs.append(x.clone())
    return xs, p0s


def _against_host(unet, fwd, sched, xT, c, z, tag):
    from diffusion_models_dsdiff_amd._sched import Trace, run_device_loop
    tr = Trace(range(sched.steps))
    y = run_device_loop(unet, sched, xT, c, step_noise=z, trace=tr)
    assert torch.equal(y, run_device_loop(unet, sched, xT, c, step_noise=z))
    xs, p0s = _host_loop(fwd, sched, xT, c, z)
    for k in range(sched.steps):
        ex, e0 = rel_l2(tr.states[k], xs[k]), rel_l2(tr.pred_x0s[k], p0s[k])
        print(f"{tag} iteration {k}: x {ex:.3e} pred_x0 {e0:.3e} against the host loop")
        assert tuple(tr.pred_x0s[k].shape) == tuple(xT.shape) and ex < TOL_OP and e0 < TOL_OP, (tag, k, ex, e0)
    assert float(tr.pred_x0s[0].abs().max()) > 0.


@pytest.mark.parametrize("body", ["ddim_v", "ddpm"])
@pytest.mark.parametrize("space", ["lat", "pix"])
def test_pred_x0_equals_the_update_op_family_b(space, body, request):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    e = request.getfixturevalue(space)
    if body == "ddim_v":                                                      # predict_start_from_z_and_v, eta 1
        e["m"].parameterization = "v"
        try:
            s = DDIMSampler(e["m"])
            s.make_schedule(4, ddim_eta=1.0, verbose=False)
            sched = s._schedule(False, True)
        finally:
            e["m"].parameterization = "eps"
    else:
        sched = _ddpm_sched(e, 4)                                             # the clipped x_recon (pix clips, lat does not)
    fwd = lambda x_in, t: (lambda o: o[0] if isinstance(o, tuple) else o)(
        e["unet"](x_in, torch.full((x_in.shape[0],), float(t), device="cuda"))).float().contiguous()
    _against_host(e["unet"], fwd, sched, e["xT"], e["c"], _noise(e, 821, sched.steps), f"{space} {body}")


def test_pred_x0_on_a_learned_range_dit_and_the_disc_network():
    """Family A: the clipped pred_xstart; under a learned-range variance the Cz state channels only (M2: Cz = 2 of a 4-channel
    output).  PLMS on both handles: the traced run is the plain run, x[j] the stopped run."""
    import test_dit_loops_gpu as TDIT
    import test_disc_gpu as TDISC
    from diffusion_models_dsdiff_amd._sched import Trace, run_plms_loop
    e = TDIT.env("M2")
    xT, c = TDIT.data(e)
    sched = TDIT.diffusion(learn_sigma=True)._schedule(False, 0.0, True)
    assert sched.c.learned_range
    _against_host(e["unet"], lambda x_in, t: TDIT.fwd(e, x_in, t), sched, xT, c, TDIT.noise(e, sched.steps), "DiT M2 learned range")
    d = TDISC.model("tiny")
    xd, cd = TDISC.data("tiny")
    sd = TDISC.diffusion()._schedule(True, 0.5, True)
    _against_host(d["unet"], lambda x_in, t: TDISC.fwd(d, x_in, t), sd, xd, cd, randn((sd.steps,) + tuple(xd.shape), 3200).cuda(),
                  "DisC tiny A_DDIM")
    for env_, x_, c_, tag in ((TDIT.env("M1"), *TDIT.data(TDIT.env("M1")), "DiT M1"), (d, xd, cd, "DisC tiny")):
        ps = TDIT.plms_sched(env_)
        plain = run_plms_loop(env_["unet"], ps, x_, c_)
        tr = Trace(range(ps.steps))
        assert torch.equal(run_plms_loop(env_["unet"], ps, x_, c_, trace=tr), plain), tag
        for k in range(ps.steps):
            assert torch.equal(run_plms_loop(env_["unet"], ps, x_, c_, n_steps=k + 1), tr.states[k]), (tag, k)


# ---------------------------------------------------------------------------------------- 4. rejections
def test_trace_rejections_name_the_fault(lat):
    from diffusion_models_dsdiff_amd import _sched
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.dpm_solver_new import DPMSolverSampler
    L, e = _lib(), lat
    h = e["unet"]._h
    run, steps = _mode(e, "ddim_cfg")
    plain = run()
    buf = torch.full((2, 3) + tuple(e["xT"].shape), 7., device="cuda")

    def set_trace(keep, x, p0, n=None):
        t = L.DsdTrace()
        arr = (C.c_int32 * max(len(keep), 1))(*keep)
        t.keep, t.n_keep = arr, len(keep) if n is None else n
        t.x, t.pred_x0 = (x.data_ptr() if x is not None else None), (p0.data_ptr() if p0 is not None else None)
        L.check(L.lib().dsd_set_trace(h, C.byref(t)))
    try:
        with pytest.raises(L.DsdError, match="not strictly ascending"):
            set_trace([2, 1], buf[0], buf[1])
        with pytest.raises(L.DsdError, match="not strictly ascending"):
            set_trace([1, 1], buf[0], buf[1])
        with pytest.raises(L.DsdError, match="both buffers are NULL"):
            set_trace([0, 1], None, None)
        with pytest.raises(L.DsdError, match="n_keep is 0"):
            set_trace([], buf[0], buf[1])
        with pytest.raises(L.DsdError, match=r"keep\[0\] = -1 is out of range"):
            set_trace([-1, 1], buf[0], buf[1])
        assert torch.equal(run(), plain)                                      # none of them was installed
        set_trace([0, steps], buf[0], buf[1])                                 # the loop knows the schedule: rejected there
        with pytest.raises(L.DsdError, match=rf"keep\[1\] = {steps} is out of range"):
            run()
        torch.cuda.synchronize()
        assert bool((buf == 7.).all())                                        # before any device work
        # the loops that do not honour a trace say so
        set_trace([0], buf[0], buf[1])
        s = DDIMSampler(e["m"])
        s.make_schedule(4, verbose=False)
        with pytest.raises(L.DsdError, match="dsd_invert does not honour a trace"):
            s.encode(e["xT"], e["c"], 2)
        with pytest.raises(L.DsdError, match="dsd_sample_dpm.* does not honour a trace"):
            DPMSolverSampler(e["m"]).sample(4, 2, tuple(e["xT"].shape[1:]), e["c"], x_T=e["xT"])
        from diffusion_models_dsdiff_amd import _lib as LL
        sched = _ddpm_sched(e, 3)
        a = _sched.Schedule(LL.MODE_A_DDPM, sched.c.pred, sched.coef, sched.t_model, sched.nonzero, clip_denoised=False)
        with pytest.raises(L.DsdError, match="dsd_calc_bpd does not honour a trace"):
            _sched.run_bpd_loop(e["unet"], a, np.zeros(3, dtype=np.float32), 0.0, e["x0"], e["c"])
    finally:
        L.check(L.lib().dsd_set_trace(h, None))
    assert torch.equal(run(), plain)
    torch.cuda.synchronize()
    assert bool((buf == 7.).all())


# ---------------------------------------------------------------------------------------- 5. log_images, the decoded row
def test_log_images_denoise_row(pix):
    from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
    e = pix
    B, H, W = 4, 32, 32
    batch = {"t1ce": torch.zeros(B, 1, H, W), "image": cond_image((B, 1, H, W), 41)}
    torch.manual_seed(5)
    log = e["m"].log_images(batch, N=B, sampler="ddim", ddim_steps=4)         # 4 steps, log_every_t 100: x_T, the first, the last
    assert tuple(log["samples"].shape) == (B, 1, H, W)
    assert tuple(log["denoise_row"].shape) == (3, 1 * (H + 2) + 2, 3 * (W + 2) + 2)   # a quarter of the batch, three entries
    assert torch.equal(log["denoise_row"][0, 2:2 + H, 2 * (W + 2) + 2:2 * (W + 2) + 2 + W], log["samples"][0, 0])
    assert "denoise_row" not in e["m"].log_images(batch, N=B, sampler="ddim", ddim_steps=4, pred_mode=True)
    assert "denoise_row" not in e["m"].log_images(batch, N=B, sampler="dpm", ddim_steps=4)
    short = DDPMModel(timesteps=6, parameterization="eps", log_every_t=2).cuda()      # the ancestral branch: t = 5, 4, 2, 0 kept
    short.model = e["wrap"]
    log = short.log_images(batch, N=B, sampler="ddpm", ddim_steps=4)
    assert tuple(log["denoise_row"].shape) == (3, B * (H + 2) + 2, 5 * (W + 2) + 2)   # the whole batch, x_T + four entries
    for b in range(B):
        assert torch.equal(log["denoise_row"][0, b * (H + 2) + 2:b * (H + 2) + 2 + H, 4 * (W + 2) + 2:4 * (W + 2) + 2 + W],
                           log["samples"][b, 0])


def test_latent_denoise_row_decodes_every_entry(lat):
    e = lat
    y, inter = e["m"].p_sample_loop(e["c"], tuple(e["xT"].shape), return_intermediates=True, x_T=e["xT"], timesteps=3, log_every_t=2,
                                    verbose=False, seed=3)
    assert len(inter) == 3 and inter[0] is e["xT"] and torch.equal(inter[-1], y)      # x_T, t = 2 (first, and 2 % 2 == 0), t = 0
    row = e["m"]._get_denoise_row_from_list(inter)
    img = e["m"].decode_first_stage(y)
    h, w = img.shape[2:]
    assert tuple(row.shape) == (3, 2 * (h + 2) + 2, 3 * (w + 2) + 2)
    assert torch.equal(row[0, 2:2 + h, 2 * (w + 2) + 2:2 * (w + 2) + 2 + w], img[0, 0])
