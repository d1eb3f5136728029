"""The paths through the sampler kernels (GPU, op level, no network): one kernel per update serves guided and unguided calls and
16-byte and scalar accesses, so equal output halves must give the unguided op's bits, the two access widths must agree bit for
bit, and every mode of the update must match the same fp32 expressions in torch."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_cfg_gpu import TOL_OP          # the bar these ops already meet: same arithmetic, other tiling
from util import rel_l2

pytestmark = pytest.mark.gpu

B = 3
CONTIGUOUS = [(1, 8, 8), (1, 5, 7)]                  # n = 64: 16-byte accesses; n = 35: scalar
STRIDED = [(2, 1, 6, 6), (3, 1, 5, 5)]               # (Cz, Cc, H, W): n = 72 in rows of 108 (16-byte); n = 75 in rows of 100 (scalar)


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    L.require_gpu(0)
    return L


def _gen(seed):
    gen = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=gen)


def _ddim(L, pred="eps", clip=True, sigma=0.37):
    from diffusion_models_dsdiff_amd._sched import Schedule
    coef = np.zeros((2, L.DSD_NCOEF), np.float32)
    coef[1] = [0.83, 0.5577, 0, 0, 0.6889, 0.78, sigma, 0.5577]
    return Schedule(L.MODE_B_DDIM, {"eps": L.PRED_EPS, "v": L.PRED_V}[pred], coef, np.asarray([9., 4.], np.float32),
                    np.ones(2, np.int32), clip_denoised=clip)


def _dpm(L, pred=2, data_pred=1, thr=1, order=2):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.sampler import DpmSchedule
    coef = np.zeros((2, L.DSD_NCOEF), np.float32)
    coef[:, :6] = np.asarray([0.31, 0.95, 0.87, -0.42, -0.21, 1.37], np.float32)
    return DpmSchedule(pred, data_pred, thr, 0.9, 0.5, coef, [10.0, 5.0], [1, order])


# ---------------------------------------------------------------------------------------- equal halves = the unguided op
@pytest.mark.parametrize("shape", CONTIGUOUS)
def test_update_with_equal_halves_is_the_unguided_update(shape):
    """out_u + s*(out_c - out_u) with out_u == out_c is out_u + s*0 = out_u exactly, so the guided op must give the unguided
    op's bits on rows [:B] and the same in rows [B:]; fed noise and Philox noise, pred_xstart too."""
    from diffusion_models_dsdiff_amd._sched import sampler_update, sampler_update_guided
    L = _lib()
    r = _gen(11 + shape[1])
    for pred in ("eps", "v"):
        for clip in (False, True):
            sc = _ddim(L, pred, clip)
            out, x, z = r(B, *shape).cuda(), (r(B, *shape) * 1.5).cuda(), r(B, *shape).cuda()
            for noise, seed in ((z, 0), (None, 4321)):
                xu, x2 = x.clone(), torch.cat([x, x])
                x0u = sampler_update(sc, 1, out, xu, noise, seed=seed, want_x0=True)
                x0g = sampler_update_guided(sc, 1, out, out.clone(), 3.0, x2, noise, seed=seed, want_x0=True)
                tag = f"pred={pred} clip={clip} philox={noise is None}"
                assert not torch.equal(xu, x), tag
                assert torch.equal(x2[:B], xu) and torch.equal(x2[B:], x2[:B]) and torch.equal(x0g, x0u), tag


@pytest.mark.parametrize("shape", CONTIGUOUS)
def test_dpm_step_with_equal_halves_is_the_unguided_step(shape):
    """noise_u + s*(noise_c - noise_u) with equal halves is noise_u exactly: x and m_cur of the guided step are the unguided
    step's bits.  Orders 0 / 1 / 2, the three prediction types, noise and data prediction, thresholding, a learned-sigma output."""
    L = _lib()
    Cz, H, W = shape
    r = _gen(23 + H)
    for pred in (0, 1, 2):                                                    # eps, x_start, v
        for order in (0, 1, 2):
            for data_pred, thr in ((0, 0), (1, 0), (1, 1)):
                for Cm in (1, 2):
                    sc = _dpm(L, pred, data_pred, thr, order)
                    out, x, m1 = r(B, Cm, H, W).cuda(), (r(B, Cz, H, W) * 2).cuda(), r(B, Cz, H, W).cuda()
                    xu, mu = x.clone(), torch.empty_like(x)
                    L.check(L.lib().dsd_op_dpm_step(C.byref(sc.c), 1, L.dptr(out), Cm, L.dptr(xu), L.dptr(mu), L.dptr(m1), B, H, W,
                                                    L.stream_ptr()))
                    x2, mg, out2 = torch.cat([x, x]), torch.empty_like(x), out.clone()
                    L.check(L.lib().dsd_op_dpm_step_guided(C.byref(sc.c), 1, L.dptr(out), L.dptr(out2), Cm, 3.0, L.dptr(x2), 0,
                                                           L.dptr(mg), L.dptr(m1), B, Cz, H, W, L.stream_ptr()))
                    tag = f"pred={pred} order={order} data_pred={data_pred} thr={thr} Cm={Cm}"
                    assert not torch.equal(xu, x), tag
                    assert torch.equal(x2[:B], xu) and torch.equal(x2[B:], x2[:B]) and torch.equal(mg, mu), tag


# ---------------------------------------------------------------------------------------- 16-byte and scalar accesses agree
def _place(t, off):
    """A contiguous copy of ``t`` on the device, ``off`` floats into its allocation: off = 1 leaves no pointer 16-byte aligned."""
    buf = torch.empty(t.numel() + 4, device="cuda", dtype=torch.float32)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


def _widths_agree(fn, **tensors):
    """fn(**tensors) once on 16-byte-aligned copies and once on copies one float into their allocations (the launcher then
    takes the scalar instantiation): every tensor, updated in place or not, must come out the same."""
    a = {k: _place(v, 0) for k, v in tensors.items()}
    b = {k: _place(v, 1) for k, v in tensors.items()}
    fn(**a)
    fn(**b)
    for k in tensors:
        assert torch.equal(a[k], b[k]), k
    return a


def _states(r, guided):
    """(Cz, H, W, state_channels, x) for every shape: a state of its own, and one inside a [rows,Cz+Cc,H,W] denoiser input."""
    rep = 2 if guided else 1
    for Cz, H, W in CONTIGUOUS:
        yield Cz, H, W, None, torch.cat([r(B, Cz, H, W) * 1.5] * rep)
    for Cz, Cc, H, W in STRIDED:
        yield Cz, H, W, Cz, torch.cat([torch.cat([r(B, Cz, H, W) * 1.5] * rep), r(rep * B, Cc, H, W)], 1).contiguous()


def _check_guided_state(got, x, Cz):
    """Both halves of the 2B-row state carry the same new state; the channels behind it (the conditioning's) are untouched."""
    st = got[:, :Cz]
    assert torch.equal(st[:B], st[B:]) and not torch.equal(st.cpu(), x[:, :Cz]) and torch.equal(got[:, Cz:].cpu(), x[:, Cz:])


def test_update_access_widths_agree():
    from diffusion_models_dsdiff_amd._sched import sampler_update_guided
    L = _lib()
    r = _gen(31)
    sc = _ddim(L, "v", True)
    for Cz, H, W in CONTIGUOUS:                                               # the unguided op takes no row stride
        for philox in (False, True):
            def fn(out, x, z, x0):
                L.check(L.lib().dsd_op_sampler_update(C.byref(sc.c), 1, L.dptr(out), L.dptr(x), None if philox else L.dptr(z),
                                                      C.c_uint64(99), B, H, W, L.dptr(x0), L.stream_ptr()))
            x = r(B, Cz, H, W) * 1.5
            got = _widths_agree(fn, out=r(B, Cz, H, W), x=x, z=r(B, Cz, H, W), x0=torch.zeros(B, Cz, H, W))
            assert not torch.equal(got["x"].cpu(), x)
    for Cz, H, W, sch, x in _states(r, True):
        for philox in (False, True):
            def fn(ou, oc, x, z):
                sampler_update_guided(sc, 1, ou, oc, 3.0, x, None if philox else z, seed=99, state_channels=sch)
            got = _widths_agree(fn, ou=r(B, Cz, H, W), oc=r(B, Cz, H, W), x=x, z=r(B, Cz, H, W))
            _check_guided_state(got["x"], x, Cz)


def test_dpm_step_access_widths_agree():
    L = _lib()
    r = _gen(37)
    sc = _dpm(L, pred=2, data_pred=1, thr=1, order=2)
    for Cz, H, W in CONTIGUOUS:
        def fn(out, x, m, m1):
            L.check(L.lib().dsd_op_dpm_step(C.byref(sc.c), 1, L.dptr(out), 1, L.dptr(x), L.dptr(m), L.dptr(m1), B, H, W,
                                            L.stream_ptr()))
        _widths_agree(fn, out=r(B, Cz, H, W), x=r(B, Cz, H, W) * 2, m=torch.zeros(B, Cz, H, W), m1=r(B, Cz, H, W))
    for Cz, H, W, sch, x in _states(r, True):
        def fn(ou, oc, x, m, m1):
            L.check(L.lib().dsd_op_dpm_step_guided(C.byref(sc.c), 1, L.dptr(ou), L.dptr(oc), 1, 3.0, L.dptr(x),
                                                   x.shape[1] * H * W, L.dptr(m), L.dptr(m1), B, Cz, H, W, L.stream_ptr()))
        got = _widths_agree(fn, ou=r(B, Cz, H, W), oc=r(B, Cz, H, W), x=x, m=torch.zeros(B, Cz, H, W), m1=r(B, Cz, H, W))
        _check_guided_state(got["x"], x, Cz)


def test_blend_invert_and_plms_access_widths_agree():
    from diffusion_models_dsdiff_amd._sched import ddim_invert_step, mask_blend, plms_step
    L = _lib()
    r = _gen(41)
    for guided in (False, True):
        for Cz, H, W, sch, x in _states(r, guided):
            s = lambda: r(B, Cz, H, W)
            for philox in (False, True):
                for mc in (1, Cz):
                    def blend(x0, mask, x, z):
                        mask_blend(0.8, 0.6, x0, mask, x, None if philox else z, seed=7, step=3, guided=guided, state_channels=sch)
                    got = _widths_agree(blend, x0=s(), mask=(r(B, mc, H, W) > 0).float(), x=x, z=s())
                    assert not torch.equal(got["x"].cpu(), x)

            def invert(ou, oc, x):
                ddim_invert_step(1.02, -0.05, oc, x, out_uncond=ou if guided else None, scale=3.0, state_channels=sch)
            got = _widths_agree(invert, ou=s(), oc=s(), x=x)
            assert not torch.equal(got["x"].cpu(), x)

            def plms(ou, oc, h_new, o1, o2, x):                               # AB4: h_new holds the oldest prediction on entry
                plms_step(L.PLMS_AB4, 0.6889, 0.78, 0.5577, oc, h_new, x, o1=o1, o2=o2, out_uncond=ou if guided else None,
                          scale=3.0, threshold=0.5, state_channels=sch)
            h0 = s()
            got = _widths_agree(plms, ou=s(), oc=s(), h_new=h0, o1=s(), o2=s(), x=x)
            assert not torch.equal(got["x"].cpu(), x) and not torch.equal(got["h_new"].cpu(), h0)


# ---------------------------------------------------------------------------------------- every mode of the update
def _update_ref(mode, coef, eta, out, x, z):
    """sampler.hip's expressions for the guided-diffusion modes and the LDM DDPM step in fp32 torch, its order (pred eps, clip on,
    nonzero)."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    c = [f(v) for v in coef]
    x0 = (c[2] * x - c[3] * out[:, :1]).clamp(-1., 1.)
    if mode == "A_DDIM":
        eps = (c[2] * x - x0) / c[3]
        ab, abp = c[4], c[5]
        sigma = f(eta) * ((1. - abp) / (1. - ab)).sqrt() * (1. - ab / abp).sqrt()
        return x0 * abp.sqrt() + (1. - abp - sigma * sigma).sqrt() * eps + sigma * z, x0
    mean = c[4] * x0 + c[5] * x
    logvar = c[6]
    if out.shape[1] == 2:                                                     # learned range
        frac = (out[:, 1:] + 1.) / 2.
        logvar = frac * c[7] + (1. - frac) * c[6]
    return mean + (0.5 * logvar).exp() * z, x0


@pytest.mark.parametrize("shape", CONTIGUOUS)
@pytest.mark.parametrize("mode", ["A_DDPM_learned_range", "A_DDIM", "B_DDPM"])
def test_update_modes_match_torch(mode, shape):
    from diffusion_models_dsdiff_amd._sched import Schedule, sampler_update
    L = _lib()
    Cz, H, W = shape
    r = _gen(53 + H)
    lr = mode == "A_DDPM_learned_range"
    coef = np.zeros((2, L.DSD_NCOEF), np.float32)
    if mode == "A_DDIM":
        coef[1] = [0, 0, 1.2048, 0.6720, 0.6889, 0.78, 0, 0]                  # alpha_bar, alpha_bar_prev in c4, c5
    else:
        coef[1] = [0, 0, 1.2048, 0.6720, 0.31, 0.68, -3.2, -1.9]              # posterior mean coefficients, min / max log variance
    sc = Schedule(getattr(L, "MODE_" + mode[:6]), L.PRED_EPS, coef, np.asarray([9., 4.], np.float32), np.ones(2, np.int32),
                  learned_range=lr, clip_denoised=True, eta=0.5)
    out, x, z = r(B, 2 if lr else 1, H, W), r(B, Cz, H, W) * 1.5, r(B, Cz, H, W)
    want, want_x0 = _update_ref(mode[:6], coef[1], 0.5, out, x, z)
    xd = x.cuda()
    x0 = sampler_update(sc, 1, out.cuda(), xd, z.cuda(), want_x0=True)
    print(f"{mode} {shape}: x {rel_l2(xd, want):.3e}, pred_xstart {rel_l2(x0, want_x0):.3e}")
    assert rel_l2(xd, want) < TOL_OP and rel_l2(x0, want_x0) < TOL_OP


# ---------------------------------------------------------------------------------------- one entry point per loop
from test_cfg_gpu import pix, lat          # noqa: E402,F401  the tiny DSUnetModel of model.npz, the UNetModel of latent_ldm.npz; B = 2


def _ddim4(m):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(m)
    s.make_schedule(4, ddim_eta=0.5, verbose=False)                           # eta > 0: the Philox seed reaches the result
    return s._schedule(False, True)


def test_four_stream_handle_takes_one_state_channel(pix):
    """dsd_sample on a four-stream handle with Cz = 2: rejected before device work, both numbers named, x untouched."""
    L = _lib()
    sched, c = _ddim4(pix["m"]), pix["c"]
    x = torch.cat([pix["xT"], pix["xT"]], 1).contiguous()
    keep = x.clone()
    rc = L.lib().dsd_sample(pix["unet"]._h, C.byref(sched.c), None, None, L.dptr(c), c.shape[1], L.dptr(x), 2, None, C.c_uint64(1), 2,
                            32, 32, 0, 0, L.stream_ptr())
    msg = L.lib().dsd_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "state of 1 channel" in msg and "Cz = 2" in msg and "the denoised image has one channel" in msg, msg
    assert torch.equal(x, keep)


def test_null_guidance_and_mask_are_the_plain_loops(pix, lat):
    """dsd_sample(g = NULL, inp = NULL) and dsd_sample_dpm(g = NULL) with Cz = 1 on the four-stream handle and Cz = 4 on the
    UNetModel handle: the bits of run_device_loop / run_dpm_loop on the same inputs and seed."""
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    L = _lib()
    for e in (pix, lat):
        c, (B, Cz, H, W) = e["c"], e["xT"].shape
        assert Cz == (1 if e["key"] == "pix" else 4)
        sched = _ddim4(e["m"])
        want = run_device_loop(e["unet"], sched, e["xT"], c, seed=77)
        x = e["xT"].clone()
        L.check(L.lib().dsd_sample(e["unet"]._h, C.byref(sched.c), None, None, L.dptr(c), c.shape[1], L.dptr(x), Cz, None,
                                   C.c_uint64(77), B, H, W, 0, 0, L.stream_ptr()))
        assert torch.equal(x, want) and not torch.equal(x, e["xT"]), e["key"]
        ns = dsa.NoiseScheduleVP("discrete", betas=e["m"].betas.detach().float().cpu())
        fn = dsa.model_wrapper(e["wrap"], ns, model_type="v", model_kwargs=dict(c_concat=[c]))
        dpm = dsa.DPM_Solver(fn, ns, algorithm_type="dpmsolver++").build_schedule(steps=4, order=2, skip_type="time_uniform",
                                                                                 lower_order_final=True)
        want = dsa.run_dpm_loop(fn, dpm, e["xT"])
        x = e["xT"].clone()
        L.check(L.lib().dsd_sample_dpm(e["unet"]._h, C.byref(dpm.c), None, L.dptr(c), c.shape[1], L.dptr(x), Cz, B, H, W,
                                       L.stream_ptr()))
        assert torch.equal(x, want) and not torch.equal(x, e["xT"]), e["key"]
