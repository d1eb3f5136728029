"""UNet_disc_Model / SuperResModelNew on the GPU: the bottleneck-head kernels (dsd_op_disc_bottleneck, csrc/disc.hip) against
float64, the nine outputs of the forward and three sampling chains against what the reference's own code computed
(tests/golden/disc.npz, gen_disc.py), every device loop bit for bit against its per-step form, and the rejections."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import disc_ref as R
from util import rel_l2, randn

pytestmark = pytest.mark.gpu

TOL_OP = 3e-6        # fp32 kernels against float64 (the bar of tests/test_attention_wide_gpu.py)
TOL_ROUTES = 1e-6    # two fp32 evaluation orders of the same head
TOL_NET = {"bf16x6": 5e-6, "f32": 5e-6, "bf16x3": 1e-4}     # the bars tests/test_cond_keys_gpu.py holds latent_unet.npz to
TOL_CHAIN = 1e-4     # the project's chain bar
STEPS = 4
_ENV = {}


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


def model(key):
    """SuperResModelNew of a fixture configuration with the fixture's weights, inside a DiffusionWrapper / DDPMModel; once."""
    if key not in _ENV:
        from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
        _lib().require_gpu(0)
        kw, sd, x, runs = R.case(key)
        m = DDPMModel(unet_config={"target": "Disc_diff.guided_diffusion.unet.SuperResModelNew", "params": kw},
                      conditioning_key="concat", timesteps=1000, parameterization="eps").cuda()
        unet = m.model.diffusion_model
        unet.load_state_dict(sd, strict=True)
        _ENV[key] = dict(m=m, wrap=m.model, unet=unet, kw=kw)
    return _ENV[key]


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _op(com, dist, w1, w2, Cr, feats=True, unfused=0):
    """dsd_op_disc_bottleneck on NHWC device tensors; returns (cat, [eight features] or None)."""
    L = _lib()
    B, HW, half = com[0].shape
    cat = torch.full((B, HW, 5 * half), float("nan"), device="cuda")
    f = [torch.full((B, HW, half), float("nan"), device="cuda") for _ in range(8)] if feats else None
    L.check(L.lib().dsd_op_disc_bottleneck(_ptrs(com), _ptrs(dist), _ptrs(w1), _ptrs(w2), B, HW, half, Cr, L.dptr(cat),
                                           _ptrs(f) if feats else None, unfused, L.stream_ptr()))
    return cat, f


# ---------------------------------------------------------------------------------------- 1. the head kernels
@pytest.mark.parametrize("half", [32, 48, 144, 320])
@pytest.mark.parametrize("hw", [(3, 5), (8, 12), (40, 40)])
@pytest.mark.parametrize("B", [2, 3])
def test_op_bottleneck(B, hw, half):
    """15 pixels (less than one chunk, no multiple of anything), 96 (two chunks, the second shorter), 1600 (25 chunks); halves of
    8, 12, 36 and 80 float4 columns (3, 21, 7 pixel rows per workgroup and 16 idle threads at 80).  Against the float64
    restatement at 3e-6 on the concat and on each feature; a second run bit-identical; the composition of older ops at 1e-6,
    by its flag and by DSD_DISC_UNFUSED; without the feature outputs the same concat."""
    h, w = hw
    HW, Cr = h * w, half // 8
    seed = 9000 + 100 * B + HW + half
    pre = [(1.5 * randn((B, half, h, w), seed + i)).cuda() for i in range(8)]             # NCHW, as the convolutions leave them
    w1 = [(randn((Cr, half), seed + 20 + i) / half ** 0.5).cuda() for i in range(5)]
    w2 = [(randn((half, Cr), seed + 30 + i) / Cr ** 0.5 * 2).cuda() for i in range(5)]
    want_cat, want_f = R.bottleneck([p.double() for p in pre[:4]], [p.double() for p in pre[4:]], [v.double() for v in w1],
                                    [v.double() for v in w2])
    nhwc = [p.permute(0, 2, 3, 1).reshape(B, HW, half).contiguous() for p in pre]
    back = lambda t: t.reshape(B, h, w, -1).permute(0, 3, 1, 2)
    cat, f = _op(nhwc[:4], nhwc[4:], w1, w2, Cr)
    err = rel_l2(back(cat), want_cat)
    errs = [rel_l2(back(a), b) for a, b in zip(f, want_f)]
    print(f"B {B} HW {HW} half {half}: concat rel-L2 vs float64 {err:.3e}, worst feature {max(errs):.3e}")
    assert bool(torch.isfinite(cat).all()) and err <= TOL_OP and max(errs) <= TOL_OP
    ungated = torch.cat([torch.mean(torch.stack(want_f[:4]), 0)] + [torch.nn.functional.silu(p.double()) for p in pre[4:]], 1)
    assert rel_l2(ungated, want_cat) > 0.1                                      # a head without its gates cannot pass
    cat2, f2 = _op(nhwc[:4], nhwc[4:], w1, w2, Cr)
    assert torch.equal(cat, cat2) and all(torch.equal(a, b) for a, b in zip(f, f2))
    cat3, none = _op(nhwc[:4], nhwc[4:], w1, w2, Cr, feats=False)
    assert none is None and torch.equal(cat, cat3)
    ucat, uf = _op(nhwc[:4], nhwc[4:], w1, w2, Cr, unfused=1)
    e_u = max([rel_l2(ucat, cat)] + [rel_l2(a, b) for a, b in zip(uf, f)])
    print(f"   fused vs unfused rel-L2 {e_u:.3e}")
    assert e_u <= TOL_ROUTES and rel_l2(back(ucat), want_cat) <= TOL_OP
    os.environ["DSD_DISC_UNFUSED"] = "1"
    try:
        ecat, _ = _op(nhwc[:4], nhwc[4:], w1, w2, Cr, feats=False, unfused=-1)
    finally:
        del os.environ["DSD_DISC_UNFUSED"]
    dcat, _ = _op(nhwc[:4], nhwc[4:], w1, w2, Cr, feats=False, unfused=-1)
    assert torch.equal(ecat, ucat) and torch.equal(dcat, cat)


def test_op_refuses_halves_that_are_no_multiple_of_four():
    L = _lib()
    t = [torch.zeros(1, 4, 6, device="cuda") for _ in range(4)]
    w = [torch.zeros(1, 6, device="cuda") for _ in range(5)]
    cat = torch.zeros(1, 4, 30, device="cuda")
    rc = L.lib().dsd_op_disc_bottleneck(_ptrs(t), _ptrs(t), _ptrs(w), _ptrs(w), 1, 4, 6, 1, L.dptr(cat), None, 0, L.stream_ptr())
    assert rc != 0 and "half = 6 is not a multiple of 4" in L.lib().dsd_last_error().decode()


# ---------------------------------------------------------------------------------------- 2. the forward
@pytest.mark.parametrize("prec", ["bf16x6", "f32", "bf16x3"])
@pytest.mark.parametrize("key", R.CONFIGS)
def test_forward_vs_reference(key, prec):
    """All nine outputs at integer and fractional t; tiny / film run B = 2, odd B = 3 on a 3x5 bottleneck."""
    e = model(key)
    kw, sd, x, runs = R.case(key)
    e["unet"].set_precision(prec)
    try:
        for tag, t, want in runs:
            got = e["unet"](x.cuda(), t.cuda())
            assert isinstance(got, tuple) and len(got) == 9
            errs = [rel_l2(a, b) for a, b in zip(got, want)]
            print(f"{key} {prec} t {tag}: out {errs[8]:.3e}, worst feature {max(errs[:8]):.3e}")
            assert all(tuple(a.shape) == b.shape for a, b in zip(got, want)) and max(errs) <= TOL_NET[prec], (key, prec, tag, errs)
    finally:
        e["unet"].set_precision("bf16x6")


def test_forward_routes_agree_and_sampling_output_is_the_ninth():
    """The unfused head (DSD_DISC_UNFUSED, read when the plan is built) gives the fused head's network output to fp32 rounding
    and still meets the reference; the loops' evaluation (no feature export) is bit-equal to the ninth output of forward."""
    e = model("odd")
    kw, sd, x, runs = R.case("odd")
    tag, t, want = runs[0]
    fused = e["unet"](x.cuda(), t.cuda())
    os.environ["DSD_DISC_UNFUSED"] = "1"
    try:
        unf = e["unet"](x.cuda(), t.cuda())
    finally:
        del os.environ["DSD_DISC_UNFUSED"]
    errs = [rel_l2(a, b) for a, b in zip(unf, fused)]
    print(f"odd: unfused vs fused head, nine outputs, worst rel-L2 {max(errs):.3e}")
    assert max(errs) <= 2e-6 and max(rel_l2(a, b) for a, b in zip(unf, want)) <= TOL_NET["bf16x6"]
    out, _ = e["unet"]._run(x.cuda(), t.cuda(), want_feats=False)
    assert torch.equal(out, e["unet"](x.cuda(), t.cuda())[8])


# ---------------------------------------------------------------------------------------- 3. the chains
def diffusion(n=STEPS, **kw):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, timestep_respacing=str(n), **kw)


@pytest.mark.parametrize("name", R.CHAINS)
def test_chain_vs_reference(name, monkeypatch):
    """The reference's SpacedDiffusion over its SuperResModelNew with model_kwargs = dict(t1, t2, dwi), here on the device loop:
    no Python step evaluates the network."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import UNet_disc_Model
    key, kw, sd, o, x_T, planes, z, want = R.chain_case(name)
    e = model(key)
    calls = [0]
    run = UNet_disc_Model._run

    def counting(self, *a, **k):
        calls[0] += 1
        return run(self, *a, **k)
    monkeypatch.setattr(UNet_disc_Model, "_run", counting)
    d = diffusion(o["steps"], learn_sigma=o["learn_sigma"])
    mk = dict(t1=planes[0].cuda(), t2=planes[1].cuda(), dwi=planes[2].cuda())
    args = dict(noise=x_T.cuda(), model_kwargs=mk, step_noise=z.cuda())
    got = (d.ddim_sample_loop(e["unet"], tuple(x_T.shape), eta=o["eta"], **args) if o["ddim"]
           else d.p_sample_loop(e["unet"], tuple(x_T.shape), **args))
    err = rel_l2(got, want)
    print(f"{name}: {o['steps']}-step chain rel-L2 vs reference {err:.3e}")
    assert calls[0] == 0 and tuple(got.shape) == want.shape and err <= TOL_CHAIN
    # the same planes as a three-channel c_concat behind the DiffusionWrapper: the same loop, the same bits
    args["model_kwargs"] = dict(c_concat=[torch.cat([p.cuda() for p in planes], 1)])
    via = (d.ddim_sample_loop(e["wrap"], tuple(x_T.shape), eta=o["eta"], **args) if o["ddim"]
           else d.p_sample_loop(e["wrap"], tuple(x_T.shape), **args))
    assert calls[0] == 0 and torch.equal(via, got)


# ---------------------------------------------------------------------------------------- 4. device loops = per-step loops
def data(key, seed=0):
    x = R.case(key)[2]
    B, _, H, W = x.shape
    return randn((B, 1, H, W), 3000 + seed).cuda(), randn((B, 3, H, W), 3100 + seed).cuda()


def fwd(e, x_in, t):
    return e["unet"](x_in, torch.full((x_in.shape[0],), float(t), device="cuda"))[8]


def _update_loop(e, sched, xT, c, z, first=0, last=None):
    from diffusion_models_dsdiff_amd._sched import sampler_update
    x = xT.clone()
    for k in range(first, sched.steps if last is None else last):
        sampler_update(sched, k, fwd(e, torch.cat([x, c], 1), sched.t_model[k]), x, z[k])
    return x


@pytest.mark.parametrize("key,body", [("tiny", "ddim_eta0"), ("tiny", "ddpm_fixed"), ("film", "ddpm_learned"), ("odd", "ddim_eta05")])
def test_update_loops_equal_the_per_step_path(key, body):
    """With graph replay off and on, and split as (0, 1), (1, rest)."""
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    e = model(key)
    xT, c = data(key)
    sched = diffusion(learn_sigma=body == "ddpm_learned")._schedule(body.startswith("ddim"), 0.5 if body == "ddim_eta05" else 0.0, True)
    z = randn((sched.steps,) + tuple(xT.shape), 3200).cuda()
    want = _update_loop(e, sched, xT, c, z)
    dev = run_device_loop(e["unet"], sched, xT, c, step_noise=z)
    assert bool(torch.isfinite(dev).all()) and not torch.equal(dev, xT) and torch.equal(dev, want)
    part = run_device_loop(e["unet"], sched, xT, c, step_noise=z, first_step=0, n_steps=1)
    assert torch.equal(part, _update_loop(e, sched, xT, c, z, 0, 1))
    assert torch.equal(run_device_loop(e["unet"], sched, part, c, step_noise=z, first_step=1, n_steps=0), want)
    before = e["unet"].graph_stats()["launches"]
    e["unet"].use_graph(True)
    try:
        rep = [run_device_loop(e["unet"], sched, xT, c, step_noise=z) for _ in range(2)]
        part = run_device_loop(e["unet"], sched, xT, c, step_noise=z, first_step=0, n_steps=1)
        rest = run_device_loop(e["unet"], sched, part, c, step_noise=z, first_step=1, n_steps=0)
        after = e["unet"].graph_stats()["launches"]
    finally:
        e["unet"].use_graph(False)
    assert after > before and all(torch.equal(r, want) for r in rep) and torch.equal(rest, want)


def _sampler_schedules(e, eta=0.5):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    s = DDIMSampler(e["m"])
    s.make_schedule(STEPS, ddim_eta=eta, verbose=False)
    p = PLMSSampler(e["m"])
    p.make_schedule(STEPS, verbose=False)
    return s._schedule(False, True), p._schedule()


def test_guided_and_masked_ddim_equal_the_per_step_path():
    """Guidance against zero planes (2B rows, uncond half first) and the masked loop's blend in front of every evaluation."""
    from diffusion_models_dsdiff_amd._sched import Guidance, Inpaint, mask_blend, run_device_loop, sampler_update, sampler_update_guided
    e = model("tiny")
    xT, c = data("tiny", 1)
    B = xT.shape[0]
    sched, _ = _sampler_schedules(e)
    z = randn((sched.steps,) + tuple(xT.shape), 3300).cuda()
    u, scale = torch.zeros_like(c), 3.0
    dev = run_device_loop(e["unet"], sched, xT, c, step_noise=z, guidance=Guidance(u, scale, sched.steps))
    x2, cin = torch.cat([xT, xT]).contiguous(), torch.cat([u, c])
    for k in range(sched.steps):
        out = fwd(e, torch.cat([x2, cin], 1), sched.t_model[k])
        sampler_update_guided(sched, k, out[:B], out[B:], scale, x2, z[k])
    plain = run_device_loop(e["unet"], sched, xT, c, step_noise=z)
    assert bool(torch.isfinite(dev).all()) and torch.equal(dev, x2[:B]) and torch.equal(x2[:B], x2[B:]) and rel_l2(dev, plain) > 1e-3
    x0, mask = randn(tuple(xT.shape), 3301).cuda(), (randn(tuple(xT.shape), 3302) > 0).float().cuda()
    zb = randn((sched.steps,) + tuple(xT.shape), 3303).cuda()
    dev = run_device_loop(e["unet"], sched, xT, c, step_noise=z, inpaint=Inpaint(x0, mask, zb))
    x = xT.clone()
    for k in range(sched.steps):
        mask_blend(sched.coef[k, 0], sched.coef[k, 1], x0, mask, x, zb[k])
        sampler_update(sched, k, fwd(e, torch.cat([x, c], 1), sched.t_model[k]), x, z[k])
    assert torch.equal(dev, x) and not torch.equal(dev, plain)


def _solver(e, c):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    ns = dsa.NoiseScheduleVP(schedule="discrete", betas=torch.from_numpy(diffusion(10).betas).float())
    return dsa.DPM_Solver(dsa.model_wrapper(e["wrap"], ns, model_type="noise", model_kwargs=dict(c_concat=[c])), ns,
                          algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")


def test_dpm_solver_loops_equal_the_per_step_path():
    """DPM-Solver++ multistep order 2 (the step body) and a singlestep order-3 program, dynamic thresholding on."""
    L = _lib()
    e = model("film")                                   # two output channels: the solver reads the first
    xT, c = data("film", 2)
    B, Cz, H, W = xT.shape
    sol = _solver(e, c)
    kw = dict(order=2, skip_type="logSNR", method="multistep", lower_order_final=False, denoise_to_zero=False, solver_type="dpmsolver")
    dev = sol.sample(xT, steps=STEPS, **kw)
    sc = sol.build_schedule(STEPS, None, None, 2, "logSNR", False, False, "dpmsolver")
    x, m_cur, m_prev = xT.clone(), torch.empty_like(xT), torch.empty_like(xT)
    for k in range(sc.steps):
        out = fwd_all(e, torch.cat([x, c], 1), sc.t_input[k])
        L.check(L.lib().dsd_op_dpm_step(C.byref(sc.c), k, L.dptr(out), out.shape[1] // Cz, L.dptr(x), L.dptr(m_cur), L.dptr(m_prev), B,
                                        Cz * H, W, L.stream_ptr()))
        m_cur, m_prev = m_prev, m_cur
    assert bool(torch.isfinite(dev).all()) and not torch.equal(dev, xT) and torch.equal(dev, x)
    kw = dict(steps=6, order=3, method="singlestep", skip_type="logSNR")
    dev = sol.sample(xT, **kw)
    prog = sol.build_program(**kw)
    x = xT.clone()
    hist, base = x.new_empty((3, B, Cz, H, W)), torch.empty_like(x)
    for k in range(prog.steps):
        out = fwd_all(e, torch.cat([x, c], 1), prog.t_input[k])
        L.check(L.lib().dsd_op_dpm_eval(C.byref(prog.c), k, None, L.dptr(out), out.shape[1] // Cz, 1., L.dptr(x), 0, L.dptr(hist),
                                        L.dptr(base), B, Cz, H, W, L.stream_ptr()))
    assert bool(torch.isfinite(dev).all()) and torch.equal(dev, x)


def fwd_all(e, x_in, t):
    return e["unet"](x_in, torch.full((x_in.shape[0],), float(t), device="cuda"))[8].contiguous()


def test_plms_equals_the_per_step_path():
    from diffusion_models_dsdiff_amd._sched import plms_step, run_plms_loop
    L = _lib()
    e = model("odd")
    xT, c = data("odd", 3)
    _, sched = _sampler_schedules(e)
    dev = run_plms_loop(e["unet"], sched, xT, c)
    x = xT.clone()
    hist = [torch.zeros_like(xT) for _ in range(3)]
    for k in range(sched.steps):
        co = (sched.coef[k, 4], sched.coef[k, 5], sched.coef[k, 7])
        out = fwd(e, torch.cat([x, c], 1), sched.t_model[k])
        if k == 0:
            plms_step(L.PLMS_PREDICT, *co, h_new=hist[0], x=x, x_saved=hist[1], out_cond=out)
            out = fwd(e, torch.cat([x, c], 1), sched.t_model[min(1, sched.steps - 1)])
            plms_step(L.PLMS_CORRECT, *co, h_new=hist[0], x=x, x_saved=hist[1], out_cond=out)
        else:
            plms_step(min(k, 3) + 1, *co, h_new=hist[k % 3], x=x, o1=hist[(k + 2) % 3], o2=hist[(k + 1) % 3], out_cond=out)
    assert bool(torch.isfinite(dev).all()) and not torch.equal(dev, xT) and torch.equal(dev, x)


def test_calc_bpd_loop_equals_the_per_step_path():
    """The variational bound: the device loop (model_kwargs t1 / t2 / dwi on the native model) against the per-step path a foreign
    callable takes, which concatenates the planes as gaussian_diffusion.py:271-275 and reads the ninth output."""
    e = model("film")
    xT, c = data("film", 4)
    d = diffusion(learn_sigma=True)
    mk = dict(t1=c[:, 0:1].contiguous(), t2=c[:, 1:2].contiguous(), dwi=c[:, 2:3].contiguous())
    x_start = xT.clamp(-1, 1)
    z = randn((d.num_timesteps,) + tuple(xT.shape), 3400).cuda()
    dev = d.calc_bpd_loop(e["unet"], x_start, model_kwargs=mk, step_noise=z)
    seen = []

    def foreign(x_in, t, **kw):
        seen.append((tuple(x_in.shape), sorted(kw)))
        return e["unet"](x_in, t)
    host = d.calc_bpd_loop(foreign, x_start, model_kwargs=mk, step_noise=z)
    assert seen and all(s == ((xT.shape[0], 4) + tuple(xT.shape[2:]), ["dwi", "t1", "t2"]) for s in seen)
    for k in ("vb", "xstart_mse", "mse", "prior_bpd", "total_bpd"):
        assert bool(torch.isfinite(dev[k]).all()) and torch.equal(dev[k], host[k]), k
    assert float(dev["vb"].abs().sum()) > 0


def test_per_step_sampling_path_takes_the_ninth_output():
    """A foreign callable around the native model: the generic loop concatenates t1 / t2 / dwi itself and reads element 8 — the
    device loop's numbers, since both run the same kernels."""
    e = model("tiny")
    xT, c = data("tiny", 5)
    d = diffusion()
    mk = dict(t1=c[:, 0:1].contiguous(), t2=c[:, 1:2].contiguous(), dwi=c[:, 2:3].contiguous())
    z = randn((d.num_timesteps,) + tuple(xT.shape), 3500).cuda()
    dev = d.p_sample_loop(e["unet"], tuple(xT.shape), noise=xT, model_kwargs=mk, step_noise=z)
    host = d.p_sample_loop(lambda x_in, t, **kw: e["unet"](x_in, t, **kw), tuple(xT.shape), noise=xT, model_kwargs=mk, step_noise=z)
    assert torch.equal(dev, host) and not torch.equal(dev, xT)


def test_slice_ids_key_the_device_noise():
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    e = model("tiny")
    sched = diffusion()._schedule(False, 0.0, True)
    x4, c4 = randn((4, 1, 16, 24), 3600).cuda(), randn((4, 3, 16, 24), 3601).cuda()
    unet = e["unet"]
    try:
        unet.set_slice_ids([0, 1, 2, 3])
        full = run_device_loop(unet, sched, x4, c4, seed=77)
        unet.set_slice_ids([0, 1])
        lo = run_device_loop(unet, sched, x4[:2], c4[:2], seed=77)
        unet.set_slice_ids([2, 3])
        hi = run_device_loop(unet, sched, x4[2:], c4[2:], seed=77)
    finally:
        unet.set_slice_ids(None)
    assert torch.equal(full, torch.cat([lo, hi])) and not torch.equal(full, run_device_loop(unet, sched, x4, c4, seed=78))


# ---------------------------------------------------------------------------------------- 5. rejections
@pytest.mark.parametrize("Cc", [1, 2, 4])
def test_loops_refuse_other_condition_counts(Cc):
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    e = model("tiny")
    sched = diffusion()._schedule(True, 0.0, True)
    xT = randn((2, 1, 16, 24), 3700).cuda()
    keep = xT.clone()
    with pytest.raises(_lib().DsdError, match=rf"3 condition planes \(t1, t2, dwi\) behind the state, got Cc = {Cc} \({Cc + 1} input channels, 4 needed\)"):
        run_device_loop(e["unet"], sched, xT, randn((2, Cc, 16, 24), 3701).cuda())
    assert torch.equal(xT, keep)


def test_other_rejections():
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.unet import UNet_disc_Model
    L = _lib()
    e = model("tiny")
    with pytest.raises(L.DsdError, match="all four encoder streams"):
        e["unet"].share_zero_streams(True)
    with pytest.raises(L.DsdError, match=r"takes 4 channels \(x, T1, T2, DWI\), got 2"):
        e["unet"](torch.zeros(2, 2, 16, 24, device="cuda"), torch.zeros(2, device="cuda"))
    assert L.lib().dsd_plan(e["unet"]._h, 2, 2, 16, 24) != 0 and "got 2" in L.lib().dsd_last_error().decode()
    # the bare UNet_disc_Model takes no keywords (unet.py:985): t1 in model_kwargs is a TypeError there, as in the reference
    bare = UNet_disc_Model(**e["kw"])
    bare.load_state_dict(R.case("tiny")[1], strict=True)
    xT, c = data("tiny", 6)
    mk = dict(t1=c[:, 0:1].contiguous(), t2=c[:, 1:2].contiguous(), dwi=c[:, 2:3].contiguous())
    with pytest.raises(TypeError, match="t1"):
        diffusion().ddim_sample_loop(bare, tuple(xT.shape), noise=xT, model_kwargs=mk)
    with pytest.raises(TypeError):
        bare(torch.cat([xT, c], 1), torch.zeros(2, device="cuda"), t1=mk["t1"])
    got = diffusion().ddim_sample_loop(bare, tuple(xT.shape), noise=xT, model_kwargs=dict(c_concat=[c]))
    assert torch.equal(got, diffusion().ddim_sample_loop(e["unet"], tuple(xT.shape), noise=xT, model_kwargs=mk))
