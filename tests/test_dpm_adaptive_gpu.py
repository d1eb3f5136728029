"""The adaptive step-size DPM-Solver on the device (GPU): dsd_op_dpm_adaptive_error against the same fp32 torch operations
(x_lower bit for bit, the error norm against float64), the one-trial entry against the per-evaluation path, every case of
tests/golden/dpm_adaptive.npz (the reference's own runs, tests/golden/gen_dpm_adaptive.py) through
DPM_Solver.dpm_solver_adaptive on the native models — the same accept / reject sequence and nfe, E within the fixture's margin,
the sample at the project's chain bar — guidance with u == c, graph replay, the DiT against a per-step host loop, max_nfe and
the library's rejections."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import dpm as ODPM
from util import golden, fixture_params, rel_l2, randn, cond_image
import dpm_adaptive_ref as A
import dit_loops_util as U
from test_dpm_adaptive_cpu import LATENT, PIXEL, cases, solver
from test_dpm_family_cpu import betas

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's chain bar
SHAPE = (2, 1, 32, 32)
# The error norm against float64 on the same inputs: the largest relative error over the cases of test_error_op_* was measured
# ("adaptive error estimate") and ten times that is asserted.  Per element the kernel rounds the difference,
# delta and the quotient to fp32 (three roundings of 2^-24 each, squared: up to ~3.6e-7 on one element, averaging out over the
# sum, which is in fp64); the result is rounded to fp32 once more.
E_MEASURED = 4.411e-8   # n = 16384, lower order 2 (35: 3.251e-8, 1024: 4.393e-8)
E_RTOL = 10 * E_MEASURED


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


def _sampler():
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    return dsa


# ---------------------------------------------------------------------------------------- models
@pytest.fixture(scope="module")
def pix():
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    _lib().require_gpu(0)
    gm, g = golden("model"), golden("dpm_adaptive")
    wrap = DiffusionWrapper({"target": "UNet_DS_Diff.model.DSUnetModel", "params": json.loads(str(gm["tiny_cfg"]))}, "concat")
    wrap.diffusion_model.load_state_dict(fixture_params(gm, "tiny"), strict=True)
    c = cond_image(SHAPE, int(g["pix_cond_seed"])).cuda()
    return dict(g=g, wrap=wrap, unet=wrap.diffusion_model, c=c, xT=randn(SHAPE, int(g["pix_xT_seed"])).cuda(), key="pix")


@pytest.fixture(scope="module")
def lat():
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    _lib().require_gpu(0)
    g, gl = golden("dpm_adaptive"), golden("latent_ldm")
    unet = UNetModel(**json.loads(str(g["lat_unet_cfg"])))
    unet.load_state_dict(fixture_params(gl, "unet"), strict=True)
    c = randn((2, 8, 8, 8), int(g["lat_c_seed"])).cuda()
    return dict(g=g, wrap=unet, unet=unet, c=c, xT=randn((2, 4, 8, 8), int(g["lat_xT_seed"])).cuda(), key="lat")


def _solve(e, name, model=None, uncond=None):
    case = cases(e["g"], e["key"])[name]
    model = e["wrap"] if model is None else model
    if uncond is None and case.get("scale", 1.) != 1.:
        uncond = torch.zeros_like(e["c"])
    if uncond is not None:
        sol, kw = solver(dict(case, scale=case.get("scale", 3.)), model, cond=e["c"], uncond=uncond)
    else:
        sol, kw = solver(case, model, model_kwargs=dict(c_concat=[e["c"]]))
    return sol, dict(kw, t_T=float(e["g"]["t_T"]), t_0=float(e["g"]["t_0"]))


def _run(e, name, **more):
    sol, kw = _solve(e, name)
    return sol.dpm_solver_adaptive(e["xT"], return_trace=True, **dict(kw, **more))


# ---------------------------------------------------------------------------------------- 1. the error kernel
ATOL, RTOL = 0.0078, 0.05


def _planes(B, n, gen):
    """base, ma, mb, x_prev [B,n] and the lower-order row: small enough that delta takes atol on some elements, rtol*|x_lower|
    on others and rtol*|x_prev| on the rest."""
    base, ma, mb, xp = (torch.randn(B, n, generator=gen) * 0.3 for _ in range(4))
    lower = np.asarray([0.83, -0.41, 0.27], np.float32)
    return base, ma, mb, xp, lower


def _err_op(order, lower, base, ma, mb, xh, xp, stride=0, rows=None, shift=0):
    """dsd_op_dpm_adaptive_error on copies of the CPU tensors [B,n]; x_higher sits in `rows` rows of `stride` floats; shift: every
    buffer starts `shift` floats behind a 16-byte boundary.  Returns (x_lower, E) on the CPU."""
    L = _lib()
    B, n = base.shape
    rows, bs = rows or B, stride or n

    def dev(t, numel=None):
        buf = torch.full(((numel or t.numel()) + 4,), 7.0, device="cuda")
        v = buf[shift:shift + (numel or t.numel())]
        return buf, v
    keep = []
    ptrs = []
    for t in (base, ma, mb, xp):
        buf, v = dev(t)
        v.copy_(t.reshape(-1))
        keep.append(buf)
        ptrs.append(C.c_void_p(v.data_ptr()))
    hbuf, hv = dev(None, rows * bs)
    hv.view(rows, bs)[:B, :n] = xh.cuda()
    lbuf, lv = dev(base)
    err = torch.empty(B, device="cuda")
    low = np.ascontiguousarray(lower if order == 3 else [lower[0], lower[1], 0.], dtype=np.float32)
    L.check(L.lib().dsd_op_dpm_adaptive_error(order - 1, low.ctypes.data_as(C.POINTER(C.c_float)), ATOL, RTOL, ptrs[0], ptrs[1],
                                              ptrs[2] if order == 3 else None, C.c_void_p(hv.data_ptr()), stride, ptrs[3],
                                              C.c_void_p(lv.data_ptr()), L.dptr(err), B, 1, 1, n, L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((lbuf[:shift] == 7.0).all()) and bool((lbuf[shift + B * n:] == 7.0).all())      # nothing beside x_lower
    return lv.view(B, n).cpu(), err.cpu()


@pytest.mark.parametrize("n", [35, 1024, 16384])
def test_error_op_against_torch(n):
    """B = 3; 35 elements: the scalar path inside one block, 1024: the 16-byte path, one block, 16384: 16 blocks per sample.  Both
    lower orders; x_higher contiguous and in the first B rows of a 2B-row state with a wider row stride.  x_lower equals the same
    fp32 torch operations bit for bit, E the float64 norm within E_RTOL; delta takes each of its three forms; two runs and the
    unaligned twin (scalar path) give the same bits."""
    _lib().require_gpu(0)
    gen = torch.Generator().manual_seed(31 + n)
    B = 3
    worst = 0.
    for order in (2, 3):
        base, ma, mb, xp, lower = _planes(B, n, gen)
        low = lower if order == 3 else np.asarray([lower[0], lower[1], 0.], np.float32)
        want_l = A.lower_cpu(low, order, base, ma, mb)
        xh = want_l + 0.004 * torch.randn(B, n, generator=gen)
        lim = RTOL * torch.max(want_l.abs(), xp.abs())
        assert bool((lim < ATOL).any()) and bool(((lim >= ATOL) & (want_l.abs() > xp.abs())).any()) \
            and bool(((lim >= ATOL) & (want_l.abs() < xp.abs())).any())
        want_e = A.error_f64(xh, want_l, xp, ATOL, RTOL)
        for stride, rows in ((0, None), (2 * n + 4 if n % 4 == 0 else 2 * n + 1, 2 * B)):
            got_l, got_e = _err_op(order, lower, base, ma, mb, xh, xp, stride, rows)
            tag = f"n={n} order={order} stride={stride}"
            np.testing.assert_array_equal(got_l.numpy(), want_l.numpy(), err_msg=tag)
            rel = float(((got_e.double() - want_e).abs() / want_e).max())
            worst = max(worst, rel)
            print(f"{tag}: E {got_e.tolist()}, largest relative error to float64 {rel:.3e}")
            assert rel <= E_RTOL, (tag, rel)
            assert rel_l2(got_e, A.error_cpu(xh, want_l, xp, ATOL, RTOL)) < 1e-5, tag         # and the reference's fp32 expression
            again_l, again_e = _err_op(order, lower, base, ma, mb, xh, xp, stride, rows)
            assert torch.equal(again_l, got_l) and torch.equal(again_e, got_e), tag
            off_l, off_e = _err_op(order, lower, base, ma, mb, xh, xp, stride, rows, shift=1)
            assert torch.equal(off_l, got_l) and torch.equal(off_e, got_e), tag + " unaligned twin"
    print(f"n={n}: largest relative error of E over the cases {worst:.3e}")


# ---------------------------------------------------------------------------------------- 2. one trial
def _per_step_trial(unet, c, order, atol, rtol):
    """trial(prog, lower, x, x_prev) on the per-evaluation path of a state-in-input denoiser: its forward on the concatenated
    input, dsd_op_dpm_eval after each, then dsd_op_dpm_adaptive_error on the planes."""
    L = _lib()

    def trial(prog, lower, x, x_prev):
        B, Cz, H, W = x.shape
        xh, xl = x.clone(), torch.empty_like(x)
        hist, base = x.new_empty((3, B, Cz, H, W)), torch.empty_like(x)
        for k in range(prog.steps):
            out = unet(torch.cat([xh, c], 1), torch.full((B,), float(prog.t_input[k]), device="cuda")).contiguous()
            L.check(L.lib().dsd_op_dpm_eval(C.byref(prog.c), k, None, L.dptr(out), out.shape[1] // Cz, 1., L.dptr(xh), 0, L.dptr(hist),
                                            L.dptr(base), B, Cz, H, W, L.stream_ptr()))
        err = torch.empty(B, device="cuda")
        L.check(L.lib().dsd_op_dpm_adaptive_error(order - 1, lower.ctypes.data_as(C.POINTER(C.c_float)), atol, rtol, L.dptr(base),
                                                  L.dptr(hist[int(prog.slot[0, 0])]), L.dptr(hist[int(prog.slot[1, 0])]), L.dptr(xh), 0,
                                                  L.dptr(x_prev.contiguous()), L.dptr(xl), L.dptr(err), B, Cz, H, W, L.stream_ptr()))
        return xh, xl, err.cpu()
    return trial


@pytest.mark.parametrize("order,stype", [(2, "dpmsolver"), (3, "dpmsolver"), (3, "taylor")])
def test_one_trial_entry(lat, order, stype):
    """A trial that is rejected (a step of 3 in logSNR under atol 1e-4, rtol 1e-3) and one that is accepted (a step of 0.05 under
    the default tolerances): the caller's x and x_prev are untouched, a repeated trial gives the same bits, and x_higher, x_lower
    and E equal the per-evaluation path bit for bit."""
    dsa = _sampler()
    ns = dsa.NoiseScheduleVP("discrete", betas=betas())
    sol = dsa.DPM_Solver(dsa.model_wrapper(lat["wrap"], ns, model_type="v", model_kwargs=dict(c_concat=[lat["c"]])), ns,
                         correcting_x0_fn="dynamic_thresholding" if order == 2 else None)
    x, x_prev = lat["xT"].clone(), (lat["xT"] * 0.9).contiguous()
    s = torch.ones(1)
    seen = []
    with dsa.AdaptiveTrial(sol.model_fn_, x, order) as trial:
        for h, atol, rtol in ((3.0, 1e-4, 1e-3), (0.05, ATOL, RTOL)):
            prog, lower = sol.adaptive_trial_program(s, ns.inverse_lambda(ns.marginal_lambda(s) + h), order, stype)
            xh, xl, E = trial.run(prog, lower, atol, rtol, x, x_prev)
            assert torch.equal(x, lat["xT"]) and torch.equal(x_prev, lat["xT"] * 0.9)
            xh2, xl2, E2 = trial.run(prog, lower, atol, rtol, x, x_prev)
            assert torch.equal(xh, xh2) and torch.equal(xl, xl2) and torch.equal(E, E2)
            wh, wl, wE = _per_step_trial(lat["unet"], lat["c"], order, atol, rtol)(prog, lower, x, x_prev)
            print(f"order {order} {stype} h {h}: E {E.tolist()}")
            assert torch.equal(xh, wh) and torch.equal(xl, wl) and torch.equal(E, wE), (order, stype, h)
            assert not torch.equal(xh, x) and bool(torch.isfinite(xh).all())
            seen.append(bool(E.max() <= 1.))
    assert seen == [False, True]


# ---------------------------------------------------------------------------------------- 3. the fixture through the public method
def _check_case(e, name):
    g, tag = e["g"], f"{e['key']}_{name}"
    y, trace = _run(e, name)
    E, acc = np.asarray([t[3] for t in trace]), [t[4] for t in trace]
    want_E, e_tol = g[tag + "_E"], float(g[tag + "_e_tol"])
    err = rel_l2(y, g[tag + "_y"])
    dE = float(np.abs(E[:len(want_E)] - want_E[:len(E)]).max())
    print(f"{tag}: {len(trace)} trials, rel-L2 to the reference {err:.3e}, largest |E - E_ref| {dE:.3e} (e_tol {e_tol:.3e})")
    assert acc == g[tag + "_accepted"].tolist(), tag
    assert len(trace) * cases(g, e["key"])[name]["order"] == int(g[tag + "_nfe"]), tag
    assert dE <= e_tol, (tag, dE, e_tol)
    assert err < TOL, (tag, err)
    return y, trace


@pytest.mark.parametrize("name", sorted(PIXEL))
def test_fixture_cases_pixel(pix, name):
    y, trace = _check_case(pix, name)
    if name == "ad2_v_pp":
        y2, trace2 = _run(pix, name)
        assert torch.equal(y, y2) and trace == trace2                          # a second call: the same bits


@pytest.mark.parametrize("name", sorted(LATENT))
def test_fixture_cases_latent(lat, name):
    _check_case(lat, name)


def test_guided_with_uncond_equal_cond_is_the_unguided_run(pix, lat):
    """e_u + s*(e_c - e_u) with e_u == e_c is e_c: u == c at scale 3 on 2B rows takes the unguided run's decisions.  The two runs
    differ by the rounding of a 2B-row against a B-row network pass, i.e. by a forward error; the generator measured what an error
    of that size does to these cases (3e-6 noise moves ad3_v_plain_loose by 1.2e-5) and keeps only cases it moves by less than
    2e-5, so the bar between two such runs is the chain bar both are held to against the reference, and every E within the
    fixture's e_tol."""
    for e, name in ((pix, "ad3_v_plain_loose"), (lat, "ad2_v_pp")):
        plain, trace = _run(e, name)
        sol, kw = _solve(e, name, uncond=e["c"].clone())
        guided, gtrace = sol.dpm_solver_adaptive(e["xT"], return_trace=True, **kw)
        print(f"{e['key']}_{name}: u == c against the unguided run {rel_l2(guided, plain):.3e}")
        assert [t[4] for t in gtrace] == [t[4] for t in trace], name
        assert max(abs(a[3] - b[3]) for a, b in zip(gtrace, trace)) <= float(e["g"][f"{e['key']}_{name}_e_tol"]), name
        assert rel_l2(guided, plain) < TOL, name


def test_graph_replay_is_bit_identical(pix, lat):
    L = _lib()
    for e, name in ((pix, "ad3_v_pp_cfg"), (lat, "ad2_v_pp")):
        dev, trace = _run(e, name)
        caps, launches = C.c_int(), C.c_int()
        L.check(L.lib().dsd_graph_stats(e["unet"]._h, C.byref(caps), C.byref(launches)))
        before = launches.value
        L.check(L.lib().dsd_set_graph(e["unet"]._h, 1))
        try:
            rep, rtrace = _run(e, name)
            L.check(L.lib().dsd_graph_stats(e["unet"]._h, C.byref(caps), C.byref(launches)))
        finally:
            L.check(L.lib().dsd_set_graph(e["unet"]._h, 0))
        assert launches.value > before and torch.equal(rep, dev) and rtrace == trace, name


def test_max_nfe_raises(pix):
    with pytest.raises(RuntimeError, match=r"max_nfe = 7 network evaluations: 6 spent in 3 trials"):
        _run(pix, "ad2_v_pp", max_nfe=7)
    y, trace = _run(pix, "ad2_eps_pp", max_nfe=22)                               # exactly what the run needs
    assert len(trace) == 11


# ---------------------------------------------------------------------------------------- 4. the DiT
def test_dit_against_a_per_step_host_loop():
    """15x15 (225 elements: the scalar path, state rows inside the 4-channel input unaligned), thresholding on: the public method
    on the device loop equals the host loop of dpm_adaptive_ref with a per-evaluation trial — sample and trace, bit for bit."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    dsa = _sampler()
    _lib().require_gpu(0)
    kw = dict(U.MODELS["M1"][0], input_size=15, patch_size=3, hidden_size=384, num_heads=6, depth=2)
    wrap = DiffusionWrapper({"target": U.DIT_TARGET, "params": kw}, "concat")
    wrap.diffusion_model.load_state_dict(U.synth_params(U.names_shapes(kw), U.WEIGHT_SEED), strict=True)
    unet = wrap.diffusion_model
    xT, c = randn((3, 1, 15, 15), 2201).cuda(), randn((3, 3, 15, 15), 2202).cuda()
    b = U.spaced_betas()
    ns = dsa.NoiseScheduleVP("discrete", betas=b)
    sol = dsa.DPM_Solver(dsa.model_wrapper(wrap, ns, model_type="noise", model_kwargs=dict(c_concat=[c])), ns,
                         algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")
    for order in (2, 3):
        args = dict(order=order, t_T=1., t_0=1. / ns.total_N, atol=ATOL, rtol=RTOL)
        y, trace = sol.dpm_solver_adaptive(xT, return_trace=True, max_nfe=150, **args)
        want, wtrace, nfe = A.run_adaptive_cpu(sol, ODPM.NoiseSchedule(betas=b), None, xT, trial=_per_step_trial(unet, c, order, ATOL, RTOL),
                                               **args)
        print(f"DiT order {order}: {len(trace)} trials, {sum(not t[4] for t in trace)} rejected")
        assert bool(torch.isfinite(y).all()) and nfe == order * len(trace)
        assert trace == wtrace and torch.equal(y, want), order


# ---------------------------------------------------------------------------------------- 5. rejections
def test_rejections_leave_the_state_untouched(pix, lat):
    dsa, L = _sampler(), _lib()
    ns = dsa.NoiseScheduleVP("discrete", betas=betas())
    s, t = torch.ones(1), torch.ones(1) * 0.9
    for e in (pix, lat):
        sol = dsa.DPM_Solver(dsa.model_wrapper(e["wrap"], ns, model_type="v", model_kwargs=dict(c_concat=[e["c"]])), ns)
        x = e["xT"].clone()
        x_prev, x_lower = x.clone(), torch.full_like(x, 5.0)
        B, Cz, H, W = x.shape
        err = np.full(B, -1.0, np.float32)
        scales = np.full(3, 3.0, np.float32)
        u = torch.zeros_like(e["c"])
        f32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))

        def call(p, low, atol=ATOL, rtol=RTOL, guid=None, xx=x, xp=x_prev, xl=x_lower, out=err, cond=e["c"]):
            gp = C.byref(guid) if guid is not None else None
            return L.lib().dsd_sample_dpm_adaptive_trial(e["unet"]._h, C.byref(p.c), gp, L.dptr(cond), e["c"].shape[1], f32(low), atol, rtol,
                                                         L.dptr(xx), L.dptr(xp), L.dptr(xl), Cz, B, H, W, f32(out), L.stream_ptr())

        def rejected(rc, text):
            msg = L.lib().dsd_last_error().decode()
            assert rc != 0 and text in msg, (text, msg)
        p2, l2 = sol.adaptive_trial_program(s, t, 2)
        p3, l3 = sol.adaptive_trial_program(s, t, 3)
        two = sol.build_program(steps=4, order=2, method="singlestep_fixed")
        rejected(call(two, l2), "the program has 4 evaluation(s) (first kind 4, last kind 6); a trial is exactly one singlestep step")
        rejected(call(sol.build_program(steps=3, order=3, method="multistep", lower_order_final=False), l3), "the program has 3 evaluation(s) (first kind 1, last kind 3)")
        rejected(call(sol.build_program(steps=1, order=1, method="singlestep"), l2), "the program has 1 evaluation(s) (first kind 1, last kind 1)")
        bad = l2.copy()
        bad[0] += 0.125
        rejected(call(p2, bad), "does not belong to the step")
        bad = l3.copy()
        bad[2] = np.inf
        rejected(call(p3, bad), "c2 of the lower-order row is inf")
        bad = l2.copy()
        bad[2] = 0.5
        rejected(call(p2, bad), "c2 of the lower-order row is 0.5")
        rejected(call(p2, None), "the lower-order coefficients are null")
        rejected(call(p2, l2, atol=0.), "atol 0; it must be positive")
        rejected(call(p2, l2, atol=-1.), "atol -1; it must be positive")
        rejected(call(p2, l2, rtol=-0.5), "rtol -0.5; it must not be negative")
        rejected(call(p2, l2, xp=None), "null array")
        rejected(call(p2, l2, xl=None), "null array")
        rejected(call(p2, l2, out=None), "null array")
        rejected(call(p2, l2, xx=None), "null argument")
        rejected(call(p2, l2, guid=L.DsdGuidance(u.data_ptr(), f32(scales), 3)), "guidance carries 3 scales but the schedule executes 2 steps")
        rejected(call(p3, l3, guid=L.DsdGuidance(None, f32(scales), 3)), "uncond is null")
        p = sol.adaptive_trial_program(s, t, 2)[0]
        p.keep[1] = 1
        rejected(call(p, l2), "keeps 1 intermediate states but the output for them is null")
        p = sol.adaptive_trial_program(s, t, 3)[0]
        p.c.threshold_ratio, p.c.thresholding = 1.5, 1
        rejected(call(p, l3), "threshold_ratio 1.5 outside [0,1]")
        # the kernel alone
        op = lambda order, low, *a: L.lib().dsd_op_dpm_adaptive_error(order, f32(low), *a, B, Cz, H, W, L.stream_ptr())
        d = L.dptr
        rejected(op(3, l3, ATOL, RTOL, d(x), d(x), d(x), d(x), 0, d(x_prev), d(x_lower), d(x_lower)), "lower order 3; it is 1 or 2")
        rejected(op(2, l3, ATOL, RTOL, d(x), d(x), None, d(x), 0, d(x_prev), d(x_lower), d(x_lower)), "null array")
        rejected(op(1, l2, 0., RTOL, d(x), d(x), None, d(x), 0, d(x_prev), d(x_lower), d(x_lower)), "atol 0; it must be positive")
        rejected(op(1, l2, ATOL, RTOL, d(x), d(x), None, d(x), 3, d(x_prev), d(x_lower), d(x_lower)), "x_row_stride 3 is smaller than one sample")
        torch.cuda.synchronize()
        assert torch.equal(x, e["xT"]) and torch.equal(x_prev, e["xT"]) and bool((x_lower == 5.0).all()) and bool((err == -1.0).all())
        # the Python surface of a trial
        with dsa.AdaptiveTrial(sol.model_fn_, x, 2) as trial:
            with pytest.raises(ValueError, match="a trial of order 2 has 2 evaluations; the program has 3"):
                trial.run(p3, l3, ATOL, RTOL, x, x_prev)
            with pytest.raises(ValueError, match="x_prev must have the shape, dtype and device of x"):
                trial.run(p2, l2, ATOL, RTOL, x, x_prev[:1])
            with pytest.raises(ValueError, match="x_prev must have the shape, dtype and device of x"):
                trial.run(p2, l2, ATOL, RTOL, x, x_prev.cpu())
    with pytest.raises(NotImplementedError, match="error norm"):
        sol.sample(pix["xT"], method="adaptive")
