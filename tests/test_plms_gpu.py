"""The PLMS sampler on the device (GPU): the update / norm kernels against the fp32 restatement of test_plms_cpu.py on fed
tensors, every chain of tests/golden/plms.npz (the reference's own PLMSSampler, tests/golden/gen_plms.py) through
PLMSSampler.sample, the device loop against a host loop, graph replay, first_step splits and the resident history, guidance with
u == c, masks against the restatement, blend noise keyed by slice id, and the rejections."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import samplers as OS
from util import golden, fixture_params, rel_l2, randn, cond_image
from test_img2img_cpu import blend, center_mask, guided
from test_plms_cpu import cases, latent_env, pixel_env, plms_chain, plms_combine, plms_update

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's chain bar (test_cfg_gpu.py, test_img2img_gpu.py)
TOL_OP = 1e-6       # same arithmetic, other tiling (test_img2img_gpu.py)
G = golden("plms")
CASES = [(sp, name) for sp in ("lat", "pix") for name in cases(G, sp)]


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------- models
def _pixel_wrap():
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    gm = golden("model")
    wrap = DiffusionWrapper({"target": "UNet_DS_Diff.model.DSUnetModel", "params": json.loads(str(gm["tiny_cfg"]))}, "concat")
    wrap.diffusion_model.load_state_dict(fixture_params(gm, "tiny"), strict=True)
    return wrap


@pytest.fixture(scope="module")
def pix():
    """The `tiny` DSUnetModel of model.npz behind a DiffusionWrapper inside an eps DDPMModel; cond / x_T of loops.npz, u = zeros."""
    from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
    _lib().require_gpu(0)
    wrap = _pixel_wrap()
    m = DDPMModel(timesteps=1000, parameterization="eps").cuda()
    m.model = wrap
    shape = (2, 1, 32, 32)
    c = cond_image(shape, int(G["pix_cond_seed"])).cuda()
    return dict(m=m, wrap=wrap, unet=wrap.diffusion_model, c=c, u=torch.zeros_like(c), xT=randn(shape, int(G["pix_xT_seed"])).cuda(),
                x0=randn(shape, int(G["x0_seed"])).cuda(), mask=center_mask(shape).cuda(), key="pix", thr=float(G["pix_thr"]))


@pytest.fixture(scope="module")
def lat():
    """The latent UNetModel of latent_ldm.npz inside an eps LatentDiffusion (first stage built, never run); c = randn, u = zeros."""
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
    ld.model.diffusion_model.load_state_dict(fixture_params(gl, "unet"), strict=True)
    ld = ld.cuda()
    shape = (2, 4, 8, 8)
    c = randn((2, 8, 8, 8), int(G["lat_c_seed"])).cuda()
    return dict(m=ld, wrap=ld.model, unet=ld.model.diffusion_model, c=c, u=torch.zeros_like(c),
                xT=randn(shape, int(G["lat_xT_seed"])).cuda(), x0=randn(shape, int(G["x0_seed"])).cuda(),
                mask=center_mask(shape).cuda(), key="lat", thr=float(G["lat_thr"]))


@pytest.fixture(params=["pix", "lat"])
def env(request):
    return request.getfixturevalue(request.param)


def _sched(m, steps):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    s = PLMSSampler(m)
    s.make_schedule(steps, verbose=False)
    return s._schedule()


def _slice_ids(unet, ids):
    L = _lib()
    arr = (C.c_int64 * max(1, len(ids)))(*ids)
    L.check(L.lib().dsd_set_slice_ids(unet._h, arr, len(ids)))


def _net(e, x, t, cond):
    out = e["wrap"](x, t, c_concat=[cond])
    return (out[0] if isinstance(out, tuple) else out).float().contiguous()


def _noise(e, seed, steps):
    return randn((steps,) + tuple(e["xT"].shape), int(seed)).cuda()


def _oracle(e):
    """(oracle network on the 'concat' input, DiffusionB tables) of the environment, on the CPU."""
    _, net, _, _, _ = latent_env() if e["key"] == "lat" else pixel_env()
    return net, OS.DiffusionB(timesteps=1000, parameterization="eps")


# ---------------------------------------------------------------------------------------- the update op
# B=3 Cz=1 5x7: 35 elements — the scalar path, a reduction smaller than a wave.  B=2 Cz=4 8x8 inside a [.,12,8,8] buffer: the
# vector path at the row stride of the latent denoiser's input.  B=2 Cz=4 64x64: 16384 elements, the reduction spans 16 blocks.
OP_SHAPES = [(3, 1, 5, 7, 0), (2, 4, 8, 8, 8), (2, 4, 64, 64, 0)]


@pytest.mark.parametrize("thr_on", [False, True], ids=["nothr", "thr"])
@pytest.mark.parametrize("is_guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=["3x1x5x7", "2x4x8x8_strided", "2x4x64x64"])
def test_plms_step_op_matches_torch(shape, is_guided, thr_on):
    from diffusion_models_dsdiff_amd._sched import plms_step
    L = _lib()
    L.require_gpu(0)
    B, Cz, H, W, Cc = shape
    scale = 3.0
    gen = torch.Generator().manual_seed(1000 * B + 10 * H + Cz + 2 * is_guided + thr_on)
    r = lambda *s: torch.randn(*s, generator=gen)
    a_t, a_prev = np.float32(0.35), np.float32(0.47)
    s1m = np.sqrt(np.float32(1.) - a_t)
    ou, oc, x, xs, e0 = r(B, Cz, H, W), r(B, Cz, H, W), r(B, Cz, H, W) * 1.5, r(B, Cz, H, W) * 1.5, r(B, Cz, H, W)
    o1, o2, o3, junk, cc = r(B, Cz, H, W), r(B, Cz, H, W), r(B, Cz, H, W), r(B, Cz, H, W), r(2 * B, max(Cc, 1), H, W)
    x[0] *= 40.                                                               # sample 0 far above the other samples' rms,
    xs[0] *= 40.                                                              # whatever the combination of the predictions adds
    e_m = ou + scale * (oc - ou) if is_guided else oc                         # plms.py:193
    rows = 2 * B if is_guided else B
    # order -> (e_t, history oldest first, e_next, the x the update applies to)
    setups = {L.PLMS_PREDICT: (e_m, [], None, x), L.PLMS_CORRECT: (e0, [], e_m, xs), L.PLMS_AB2: (e_m, [o1], None, x),
              L.PLMS_AB3: (e_m, [o2, o1], None, x), L.PLMS_AB4: (e_m, [o3, o2, o1], None, x)}
    for order, (e_t, old, e_next, xin) in setups.items():
        ep = e_t if order == L.PLMS_PREDICT else plms_combine(e_t, old, e_next)
        p0 = (xin - torch.full((B, 1, 1, 1), float(s1m)) * ep) / torch.full((B, 1, 1, 1), float(a_t)).sqrt()
        rms = p0.pow(2).flatten(1).mean(1).sqrt()
        v = float((rms.min() * rms.max()).sqrt()) if thr_on else None         # one sample above the threshold, one below
        if thr_on:
            assert rms.max() > 1.5 * v and rms.min() < v / 1.5
        want = plms_update(xin, ep, a_t, a_prev, s1m, v)
        tag = f"order {order} guided {is_guided} thr {v}"

        def run():
            h_new = {L.PLMS_CORRECT: e0, L.PLMS_AB4: o3}.get(order, junk).clone().cuda()
            d = dict(o1=o1.clone().cuda(), o2=o2.clone().cuda(), x_saved=(xs if order == L.PLMS_CORRECT else junk).clone().cuda())
            state = torch.cat([x, r(B, Cz, H, W)]) if is_guided else x.clone()          # the second half: overwritten
            buf = (torch.cat([state, cc[:rows]], 1) if Cc else state).cuda().contiguous()
            plms_step(order, a_t, a_prev, s1m, oc.cuda(), h_new, buf, o1=d["o1"] if order >= L.PLMS_AB2 else None,
                      o2=d["o2"] if order >= L.PLMS_AB3 else None, x_saved=d["x_saved"] if order <= L.PLMS_CORRECT else None,
                      out_uncond=ou.cuda() if is_guided else None, scale=scale, threshold=v, state_channels=Cz)
            return buf, h_new, d
        buf, h_new, d = run()
        got = buf[:, :Cz]
        err = rel_l2(got[:B], want)
        print(f"{shape} {tag}: rel-L2 to torch {err:.3e}")
        assert err < TOL_OP, tag
        if is_guided:
            assert torch.equal(got[:B], got[B:]), tag                         # rows b and B+b
        if Cc:
            assert torch.equal(buf[:, Cz:].cpu(), cc[:rows]), tag             # the conditioning channels stay
        # the retired plane holds e_t afterwards (the corrector leaves it), the other planes are untouched
        assert rel_l2(h_new, e_t) < TOL_OP and (is_guided and order != L.PLMS_CORRECT or torch.equal(h_new.cpu(), e_t)), tag
        assert torch.equal(d["o1"].cpu(), o1) and torch.equal(d["o2"].cpu(), o2), tag
        assert torch.equal(d["x_saved"].cpu(), {L.PLMS_PREDICT: x, L.PLMS_CORRECT: xs}.get(order, junk)), tag
        buf2, h2, _ = run()                                                   # deterministic: no atomics in the reduction
        assert torch.equal(buf2[:, :Cz], got) and torch.equal(h2, h_new), tag


# ---------------------------------------------------------------------------------------- fixture chains, public method
@pytest.mark.parametrize("space,name", CASES, ids=[f"{s}_{n}" for s, n in CASES])
def test_plms_sampler_vs_reference(space, name, request):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.plms import PLMSSampler
    e = request.getfixturevalue(space)
    steps, scale, bs, thresholded, twin = cases(G, space)[name]
    kw = dict(verbose=False, x_T=e["xT"], unconditional_guidance_scale=scale, unconditional_conditioning=e["u"])
    if bs:
        kw.update(mask=e["mask"], x0=e["x0"], mask_noise=_noise(e, G[bs + "_seed"], steps))
    if thresholded:
        kw.update(dynamic_threshold=e["thr"])
    shape = tuple(e["xT"].shape[1:])
    y, inter = PLMSSampler(e["m"]).sample(steps, 2, shape, e["c"], **kw)
    ref = G[f"{space}_{name}_y"]
    print(f"{space}_{name}: rel-L2 to the reference {rel_l2(y, ref):.3e}")
    assert tuple(y.shape) == ref.shape and rel_l2(y, ref) < TOL
    assert inter["x_inter"][0] is e["xT"] and torch.equal(inter["x_inter"][-1], y)
    if twin:                                                                  # the mask / the threshold is live
        assert rel_l2(y, G[f"{space}_{twin}_y"]) > 1e-2
    if name == "plms20":                                                      # the other forms of the conditioning; zero-tensor options
        y2, _ = PLMSSampler(e["m"]).sample(steps, 2, shape, dict(c_concat=[e["c"]]), verbose=False, x_T=e["xT"], temperature=0.5,
                                           noise_dropout=0.2, x0=e["x0"])
        assert torch.equal(y2, y)
    if name == "plms_cfg":
        y2, _ = PLMSSampler(e["m"]).sample(steps, 2, shape, [e["c"]], verbose=False, x_T=e["xT"], unconditional_guidance_scale=scale,
                                           unconditional_conditioning=[e["u"]])
        assert torch.equal(y2, y)


# ---------------------------------------------------------------------------------------- loop-level checks
def _host_loop(e, sched, scale, inp, thr):
    """The loop written here: forward through the module, the blend op and dsd_op_plms_step per iteration, with a history of
    its own in the ring order the library documents (iteration k retires plane k % 3)."""
    from diffusion_models_dsdiff_amd._sched import mask_blend, plms_step
    L = _lib()
    B, steps = e["xT"].shape[0], sched.steps
    is_guided = scale is not None
    x = (torch.cat([e["xT"], e["xT"]]) if is_guided else e["xT"].clone()).contiguous()
    cin = torch.cat([e["u"], e["c"]]) if is_guided else e["c"]
    hist = [torch.zeros_like(e["xT"]) for _ in range(3)]
    t = lambda k: torch.full((x.shape[0],), float(sched.t_model[k]), device="cuda")
    for k in range(steps):
        if inp is not None:
            mask_blend(sched.coef[k, 0], sched.coef[k, 1], inp[0], inp[1], x, inp[2][k], guided=is_guided)
        co = (sched.coef[k, 4], sched.coef[k, 5], sched.coef[k, 7])
        kw = dict(scale=scale or 1., threshold=thr)
        halves = lambda out: dict(out_uncond=out[:B], out_cond=out[B:]) if is_guided else dict(out_cond=out)
        out = _net(e, x, t(k), cin)
        if k == 0:
            plms_step(L.PLMS_PREDICT, *co, h_new=hist[0], x=x, x_saved=hist[1], **halves(out), **kw)
            out = _net(e, x, t(min(1, steps - 1)), cin)
            plms_step(L.PLMS_CORRECT, *co, h_new=hist[0], x=x, x_saved=hist[1], **halves(out), **kw)
        else:
            plms_step(min(k, 3) + 1, *co, h_new=hist[k % 3], x=x, o1=hist[(k + 2) % 3], o2=hist[(k + 1) % 3], **halves(out), **kw)
    return x[:B]


@pytest.mark.parametrize("mode", ["plain", "guided_masked_thr"])
def test_device_loop_matches_host_loop_graph_replay_and_split(env, mode):
    from diffusion_models_dsdiff_amd._sched import Guidance, Inpaint, run_plms_loop
    L = _lib()
    e, steps = env, 10
    unet, c, xT = e["unet"], e["c"], e["xT"]
    full = mode != "plain"
    sched = _sched(e["m"], steps)
    zb = _noise(e, 911, steps)
    kw = lambda: dict(threshold=e["thr"] if full else None, guidance=Guidance(e["u"], 3.0, steps) if full else None,
                      inpaint=Inpaint(e["x0"], e["mask"], zb) if full else None)
    dev = run_plms_loop(unet, sched, xT, c, **kw())
    host = _host_loop(e, sched, 3.0 if full else None, (e["x0"], e["mask"], zb) if full else None, e["thr"] if full else None)
    print(f"{e['key']} {mode}: device loop against the host loop {rel_l2(dev, host):.3e}")
    assert rel_l2(dev, host) < TOL_OP
    assert torch.equal(run_plms_loop(unet, sched, xT, c, **kw()), dev)        # two runs, bit for bit
    caps, launches = C.c_int(), C.c_int()
    L.check(L.lib().dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
    before = launches.value
    L.check(L.lib().dsd_set_graph(unet._h, 1))
    try:
        rep = run_plms_loop(unet, sched, xT, c, **kw())
        rep2 = run_plms_loop(unet, sched, xT, c, **kw())
        L.check(L.lib().dsd_graph_stats(unet._h, C.byref(caps), C.byref(launches)))
    finally:
        L.check(L.lib().dsd_set_graph(unet._h, 0))
    assert launches.value > before and torch.equal(rep, dev) and torch.equal(rep2, dev)
    # split after iteration 0 (both first-step evaluations in one segment), inside the ramp, and after it
    x = xT
    for first, n in ((0, 1), (1, 2), (3, 0)):
        x = run_plms_loop(unet, sched, x, c, first_step=first, n_steps=n, **kw())
    assert torch.equal(x, dev)


def test_history_must_be_resident():
    """first_step = 5 on a handle that has run nothing fails with the history message and leaves the state alone; after the
    iterations before it have run it continues them; another schedule length or batch is not that history."""
    from diffusion_models_dsdiff_amd._sched import run_plms_loop
    from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
    L = _lib()
    L.require_gpu(0)
    wrap = _pixel_wrap().cuda()
    m = DDPMModel(timesteps=1000, parameterization="eps").cuda()
    m.model = wrap
    unet = wrap.diffusion_model
    shape = (2, 1, 32, 32)
    c, xT = cond_image(shape, int(G["pix_cond_seed"])).cuda(), randn(shape, int(G["pix_xT_seed"])).cuda()
    s10, s20 = _sched(m, 10), _sched(m, 20)
    with pytest.raises(L.DsdError, match="PLMS history for iteration 5 is not resident"):
        run_plms_loop(unet, s10, xT, c, first_step=5)
    whole = run_plms_loop(unet, s10, xT, c)
    with pytest.raises(L.DsdError, match="PLMS history for iteration 5 is not resident"):        # it holds iteration 10's
        run_plms_loop(unet, s10, xT, c, first_step=5)
    head = run_plms_loop(unet, s10, xT, c, n_steps=5)
    with pytest.raises(L.DsdError, match="PLMS history for iteration 5 is not resident"):
        run_plms_loop(unet, s20, head, c, first_step=5)
    with pytest.raises(L.DsdError, match="PLMS history for iteration 5 is not resident"):
        run_plms_loop(unet, s10, head[:1], c[:1], first_step=5)
    with pytest.raises(L.DsdError, match="PLMS history for iteration 4 is not resident"):
        run_plms_loop(unet, s10, head, c, first_step=4)
    assert torch.equal(run_plms_loop(unet, s10, head, c, first_step=5), whole)  # the rejected calls left the history alone
    # the planes are sized once: a second run of the same shape allocates nothing
    before = L.lib().dsd_device_bytes(unet._h)
    run_plms_loop(unet, s10, xT, c, threshold=2.0)
    assert L.lib().dsd_device_bytes(unet._h) == before and before > 3 * xT.numel() * 4


def test_guided_with_uncond_equal_cond_and_masks_against_the_restatement(env):
    """u == c at scale 3.0 reproduces the unguided run (bar: test_masked_guided_with_uncond_equal_cond...); an all-ones mask makes
    every iteration start from q_sample(x0, t), so the result is the last blend followed by one update on the run's history; a
    [B,Cz,h,w] mask blends per channel.  The masked runs are checked against the restated chain on the oracle network."""
    from diffusion_models_dsdiff_amd._sched import Guidance, Inpaint, run_plms_loop
    e, steps = env, 5
    sched = _sched(e["m"], steps)
    run = lambda **kw: run_plms_loop(e["unet"], sched, e["xT"], e["c"], **kw)
    plain = run(threshold=e["thr"])
    same = run(threshold=e["thr"], guidance=Guidance(e["c"].clone(), 3.0, steps))
    print(f"{e['key']}: u == c against the unguided run {rel_l2(same, plain):.3e}")
    assert rel_l2(same, plain) < 1e-5 and rel_l2(run(), plain) > 1e-2
    net, od = _oracle(e)
    zb = _noise(e, 921, steps)
    x0, c, u, xT = e["x0"].cpu(), e["c"].cpu(), e["u"].cpu(), e["xT"].cpu()
    ones = torch.ones_like(e["mask"])
    per_channel = (torch.rand(tuple(e["xT"].shape), generator=torch.Generator().manual_seed(5)) > 0.5).float().cuda()
    for mask in (ones, per_channel):
        pre = lambda i, t, img: blend(od, x0, mask.cpu(), t, zb[i].cpu(), img)
        want = plms_chain(od, guided(net, c, u, 1.), xT.clone(), steps, pre=pre)
        got = run(inpaint=Inpaint(e["x0"], mask, zb))
        print(f"{e['key']}: mask {tuple(mask.shape)} against the restatement {rel_l2(got, want):.3e}")
        assert rel_l2(got, want) < TOL and rel_l2(got, run()) > 1e-2
    # all ones: nothing of x_T survives the first blend
    assert torch.equal(run_plms_loop(e["unet"], sched, torch.zeros_like(e["xT"]), e["c"], inpaint=Inpaint(e["x0"], ones, zb)),
                       run(inpaint=Inpaint(e["x0"], ones, zb)))


def test_slice_ids_key_the_blend_noise(env):
    """With dsd_set_slice_ids the Philox blend noise of a slice does not depend on how slices are grouped into batches: a mask
    that keeps everything, one iteration — the result is the first step's update pair on q_sample(x0, t) of the blend's draws."""
    from diffusion_models_dsdiff_amd._sched import Inpaint, run_plms_loop
    e = env
    sched = _sched(e["m"], 10)
    ones = torch.ones_like(e["mask"])

    def run(rows, ids):
        _slice_ids(e["unet"], ids)
        try:
            return run_plms_loop(e["unet"], sched, e["xT"][rows], e["c"][rows], seed=77, n_steps=1,
                                 inpaint=Inpaint(e["x0"][rows], ones[rows]))
        finally:
            _slice_ids(e["unet"], [])
    both = run(slice(0, 2), [11, 5])
    assert rel_l2(run(slice(0, 1), [11]), both[:1]) < 1e-5 and rel_l2(run(slice(1, 2), [5]), both[1:]) < 1e-5
    assert rel_l2(run(slice(1, 2), [6]), both[1:]) > 1e-2                     # another slice, other normals
    assert rel_l2(run(slice(1, 2), []), both[1:]) > 1e-2                      # without ids: keyed by the batch position


# ---------------------------------------------------------------------------------------- rejections
def test_modes_are_rejected_with_a_reason(env):
    from diffusion_models_dsdiff_amd._sched import (Guidance, Inpaint, Schedule, run_device_loop, run_plms_loop, sampler_update,
                                                    sampler_update_guided)
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    L = _lib()
    e, steps = env, 10
    unet, c, u, xT = e["unet"], e["c"], e["u"], e["xT"]
    sched = _sched(e["m"], steps)
    inp, guid = lambda: Inpaint(e["x0"], e["mask"]), lambda: Guidance(u, 3.0, steps)
    # every existing sampling entry point refuses the PLMS mode
    for kw in (dict(), dict(guidance=guid()), dict(inpaint=inp()), dict(inpaint=inp(), guidance=guid())):
        with pytest.raises(L.DsdError, match="DSD_MODE_B_PLMS.*dsd_sample_plms"):
            run_device_loop(unet, sched, xT, c, **kw)
    out = torch.zeros_like(xT)
    with pytest.raises(L.DsdError, match="DSD_MODE_B_PLMS.*dsd_sample_plms"):
        sampler_update(sched, 0, out, xT.clone(), out)
    with pytest.raises(L.DsdError, match="DSD_MODE_B_PLMS.*dsd_sample_plms"):
        sampler_update_guided(sched, 0, out, out, 3.0, torch.cat([xT, xT]), out)
    # and the PLMS loop refuses every other mode, sigma != 0, learned range, a prediction that is no noise prediction
    dd = DDIMSampler(e["m"])
    dd.make_schedule(steps, ddim_eta=1.0, verbose=False)
    eta1 = dd._schedule(False, False)
    for mode in (L.MODE_A_DDPM, L.MODE_A_DDIM, L.MODE_B_DDPM, L.MODE_B_DDIM):
        with pytest.raises(L.DsdError, match="take a DSD_MODE_B_PLMS schedule"):
            run_plms_loop(unet, Schedule(mode, L.PRED_EPS, sched.coef, sched.t_model, sched.nonzero), xT, c)
    with pytest.raises(L.DsdError, match="eta = 0 only"):
        run_plms_loop(unet, Schedule(L.MODE_B_PLMS, L.PRED_EPS, eta1.coef, eta1.t_model, eta1.nonzero), xT, c)
    with pytest.raises(L.DsdError, match="learned-range"):
        run_plms_loop(unet, Schedule(L.MODE_B_PLMS, L.PRED_EPS, sched.coef, sched.t_model, sched.nonzero, learned_range=True), xT, c)
    with pytest.raises(L.DsdError, match="noise prediction"):
        run_plms_loop(unet, sched.with_pred(L.PRED_V), xT, c)
    with pytest.raises(ValueError, match="mask must be"):
        run_plms_loop(unet, sched, xT, c, inpaint=Inpaint(e["x0"], e["mask"][:, :, :4].contiguous()))
    # the C entry points themselves
    x = xT.clone()
    Cz, H, W = x.shape[1:]
    scales = np.full(steps, 3.0, np.float32)
    sp = scales.ctypes.data_as(C.POINTER(C.c_float))

    def call(p=None, g=None):
        gp, ip = C.byref(g) if g is not None else None, C.byref(p) if p is not None else None
        return L.lib().dsd_sample_plms(unet._h, C.byref(sched.c), gp, ip, 0.0, L.dptr(c), c.shape[1], L.dptr(x), Cz, C.c_uint64(1), 2,
                                       H, W, 0, 0, L.stream_ptr())
    err = lambda: L.lib().dsd_last_error().decode()
    x0p, mp = e["x0"].data_ptr(), e["mask"].data_ptr()
    assert call(L.DsdInpaint(None, mp, 1, None)) != 0 and "x0 is null" in err()
    assert call(L.DsdInpaint(x0p, None, 1, None)) != 0 and "mask is null" in err()
    for ch in (0, 2, Cz + 1):
        assert call(L.DsdInpaint(x0p, mp, ch, None)) != 0 and f"the mask has {ch} channels" in err()
    assert call(None, L.DsdGuidance(None, sp, steps)) != 0 and "uncond is null" in err()
    assert call(None, L.DsdGuidance(u.data_ptr(), sp, steps - 1)) != 0 and "scales" in err()
    try:
        _slice_ids(unet, [0, 1, 2, 3])
        assert call() != 0 and "4 ids but the batch has 2" in err()
    finally:
        _slice_ids(unet, [])
    hp = L.dptr(torch.zeros_like(x))
    assert L.lib().dsd_op_plms_step(5, 0.5, 0.6, 0.7, None, hp, 1.0, hp, None, None, None, L.dptr(x), 0, 0.0, 2, Cz, H, W,
                                    L.stream_ptr()) != 0 and "unknown PLMS order 5" in err()
    assert L.lib().dsd_op_plms_step(L.PLMS_AB3, 0.5, 0.6, 0.7, None, hp, 1.0, hp, hp, None, None, L.dptr(x), 0, 0.0, 2, Cz, H, W,
                                    L.stream_ptr()) != 0 and "needs o2" in err()
    torch.cuda.synchronize()
    assert torch.equal(x, xT)                                                 # nothing ran
