"""The DPM-Solver family on the device (GPU): dsd_op_dpm_eval against the same fp32 torch operations bit for bit, every case of
tests/golden/dpm_family.npz (the reference's own runs, tests/golden/gen_dpm_family.py) through DPM_Solver.sample / .inverse at
the project's chain bar, the existing multistep loop restated as a program, the generic-callable path, the latent UNetModel, the
DiT against a per-step loop, graph replay, return_intermediate and the rejections."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from util import golden, fixture_params, rel_l2, randn, cond_image
import dpm_family_ref as R
import dit_loops_util as U
from test_dpm_family_cpu import PIXEL, betas, cases, solver

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's chain bar
SHAPE = (2, 1, 32, 32)


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
    gm, g = golden("model"), golden("dpm_family")
    wrap = DiffusionWrapper({"target": "UNet_DS_Diff.model.DSUnetModel", "params": json.loads(str(gm["tiny_cfg"]))}, "concat")
    wrap.diffusion_model.load_state_dict(fixture_params(gm, "tiny"), strict=True)
    c = cond_image(SHAPE, int(g["pix_cond_seed"])).cuda()
    return dict(g=g, wrap=wrap, unet=wrap.diffusion_model, c=c, xT=randn(SHAPE, int(g["pix_xT_seed"])).cuda(), key="pix")


@pytest.fixture(scope="module")
def lat():
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    _lib().require_gpu(0)
    g, gl = golden("dpm_family"), golden("latent_ldm")
    unet = UNetModel(**json.loads(str(g["lat_unet_cfg"])))
    unet.load_state_dict(fixture_params(gl, "unet"), strict=True)
    c = randn((2, 8, 8, 8), int(g["lat_c_seed"])).cuda()
    return dict(g=g, wrap=unet, unet=unet, c=c, xT=randn((2, 4, 8, 8), int(g["lat_xT_seed"])).cuda(), key="lat")


def _solve(e, name, model=None):
    """(solver, sample keyword arguments, start state) of a fixture case on the environment's model."""
    case = cases(e["g"], e["key"])[name]
    model = e["wrap"] if model is None else model
    if case.get("scale", 1.) != 1.:
        sol, kw = solver(case, model, cond=e["c"], uncond=torch.zeros_like(e["c"]))
    else:
        sol, kw = solver(case, model, model_kwargs=dict(c_concat=[e["c"]]))
    x = torch.from_numpy(e["g"][f"{e['key']}_{name}_x"]).cuda() if case.get("inverse") else e["xT"]
    return sol, kw, x, (sol.inverse if case.get("inverse") else sol.sample)


# ---------------------------------------------------------------------------------------- 1. the per-evaluation op, bit for bit
def _program(kinds, pred, data_pred, thr, gen):
    """A program of the given kinds with random coefficients of both signs; slots as the builder lays them out."""
    dsa = _sampler()
    slots = {0: (0, 0, 0, 0), 1: (0, 0, 0, 0), 2: (1, 1, 0, 0), 3: (2, 2, 1, 0), 4: (0, 0, 0, 0), 5: (1, 0, 1, 0), 6: (1, 0, 1, 0),
             7: (2, 0, 2, 0), 8: (2, 0, 1, 2)}
    evals = []
    for kind in kinds:
        coef = (torch.rand(9, generator=gen) * 1.5 + 0.25) * torch.where(torch.rand(9, generator=gen) < 0.4, -1., 1.)
        coef[8] = coef[7] - coef[6] if coef[7] != coef[6] else 0.5
        a, s = float(torch.rand(1, generator=gen)) * 0.6 + 0.3, float(torch.rand(1, generator=gen)) * 0.6 + 0.3
        evals.append(dict(kind=kind, t=0.5, t_input=10.0, alpha=a, sigma=s, coef=coef.tolist(), slot=slots[kind], keep=False))
    return dsa.DpmProgram(pred, data_pred, thr, 0.995, 1.0, evals)


PROGRAMS = ([1, 2, 3, 0], [4, 5, 8], [4, 6], [4, 5, 7])      # every kind, each where its history / base exists


def _op(prog, k, out, x, hist, base, out_u=None, scale=1., stride=0):
    """dsd_op_dpm_eval on copies of the CPU tensors; returns (state rows [rows,C,H,W], hist, base) back on the CPU."""
    L = _lib()
    B, Cz, H, W = x.shape
    n = Cz * H * W
    rows = 2 * B if out_u is not None else B
    bs = stride or n
    xd = torch.full((rows, bs), 7.0, device="cuda")
    xd[:, :n] = torch.cat([x] * (rows // B)).reshape(rows, n).cuda()
    hd, bd = torch.stack(hist).cuda().contiguous(), base.cuda().contiguous()
    od, ud = out.cuda().contiguous(), out_u.cuda().contiguous() if out_u is not None else None
    L.check(L.lib().dsd_op_dpm_eval(C.byref(prog.c), k, L.dptr(ud), L.dptr(od), out.shape[1] // Cz, float(scale), L.dptr(xd), stride,
                                    L.dptr(hd), L.dptr(bd), B, Cz, H, W, L.stream_ptr()))
    assert bool((xd[:, n:] == 7.0).all())                                     # nothing beside the state inside a wider row
    return xd[:, :n].reshape(rows, Cz, H, W).cpu(), hd.cpu(), bd.cpu()


def _check_op(prog, k, B, Cz, H, W, Cm, gen, guided=False, stride=0, tag=""):
    out = torch.randn(B, Cm * Cz, H, W, generator=gen)
    out_u = torch.randn(B, Cm * Cz, H, W, generator=gen) if guided else None
    x = torch.randn(B, Cz, H, W, generator=gen) * 2
    hist = [torch.randn(B, Cz, H, W, generator=gen) for _ in range(3)]
    base = torch.randn(B, Cz, H, W, generator=gen)
    got_x, got_h, got_b = _op(prog, k, out, x, hist, base, out_u, 2.5, stride)
    h2, b2 = list(hist), [base]
    want = R.eval_cpu(prog, k, out, x, h2, b2, out_u, 2.5)
    tag = f"{tag} kinds={prog.kind.tolist()} k={k} pred={prog.c.pred} data={prog.c.data_pred} thr={prog.c.thresholding} {B}x{Cz}x{H}x{W}"
    np.testing.assert_array_equal(got_x[:B].numpy(), want.numpy(), err_msg=tag)
    if guided:
        np.testing.assert_array_equal(got_x[B:].numpy(), want.numpy(), err_msg=tag + " row B+b")
    np.testing.assert_array_equal(got_h.numpy(), torch.stack(h2).numpy(), err_msg=tag + " history")
    np.testing.assert_array_equal(got_b.numpy(), b2[0].numpy(), err_msg=tag + " base")


@pytest.mark.parametrize("shape", [(3, 1, 24, 40), (3, 1, 5, 7), (2, 1, 15, 15)])
def test_eval_op_bit_exact(shape):
    """Model value, thresholding and the update of every kind x prediction type x algorithm, with and without thresholding,
    against the same fp32 torch operations on the CPU: 24x40 takes the 16-byte path, 5x7 = 35 and 15x15 = 225 elements the
    scalar one.  History planes and the base plane are compared too (the written plane thresholded, the others untouched)."""
    _lib().require_gpu(0)
    gen = torch.Generator().manual_seed(21)
    B, Cz, H, W = shape
    for kinds in PROGRAMS:
        for pred in (0, 1, 2):
            for data_pred in (1, 0):
                for thr in (1, 0):
                    prog = _program(kinds, pred, data_pred, thr, gen)
                    for k in range(len(kinds)):
                        _check_op(prog, k, B, Cz, H, W, 1, gen)


def test_eval_op_learned_sigma_and_guided_rows():
    """A learned-sigma output (twice the state's channels) contributes its first half, on one channel and on four; guided, the state sits inside a wider input row (row
    stride larger than the sample, 16-byte and scalar), both rows of a sample are written and nothing beside them."""
    _lib().require_gpu(0)
    gen = torch.Generator().manual_seed(22)
    for kinds in PROGRAMS:
        prog = _program(kinds, 2, 1, 1, gen)
        for k in range(len(kinds)):
            _check_op(prog, k, 3, 1, 24, 40, 2, gen, tag="Cm=2")
            _check_op(prog, k, 2, 1, 5, 7, 2, gen, tag="Cm=2")
            _check_op(prog, k, 2, 4, 8, 8, 1, gen, guided=True, stride=12 * 64, tag="guided")
            _check_op(prog, k, 2, 1, 15, 15, 1, gen, guided=True, stride=4 * 225, tag="guided")
            _check_op(prog, k, 2, 1, 24, 40, 2, gen, guided=True, tag="guided Cm=2")
            _check_op(prog, k, 2, 4, 8, 8, 2, gen, tag="Cm=2 Cz=4")               # a learned sigma on a latent state


# ---------------------------------------------------------------------------------------- 2. the fixture through the public solver
@pytest.mark.parametrize("name", sorted(PIXEL))
def test_fixture_cases_pixel(pix, name):
    sol, kw, x, run = _solve(pix, name)
    y = run(x, **kw)
    err = rel_l2(y, pix["g"][f"pix_{name}_y"])
    print(f"pix_{name}: rel-L2 to the reference {err:.3e}")
    assert err < TOL, (name, err)
    assert torch.equal(y, run(x, **kw)), name                                 # a second call: the same bits


@pytest.mark.parametrize("name", ["ms3_v_10", "ss3_v_cfg_9"])
def test_fixture_cases_latent(lat, name):
    sol, kw, x, run = _solve(lat, name)
    y = run(x, **kw)
    err = rel_l2(y, lat["g"][f"lat_{name}_y"])
    print(f"lat_{name}: rel-L2 to the reference {err:.3e}")
    assert err < TOL, (name, err)
    assert torch.equal(y, run(x, **kw)), name


# ---------------------------------------------------------------------------------------- 3. the existing loop as a program
def test_multistep_program_equals_the_existing_loop(pix, lat):
    """Order <= 2 through dsd_sample_dpm_program equals dsd_sample_dpm (guided or not) on the same schedule bit for bit, pixel and
    latent, unguided and guided, with thresholding and denoise_to_zero."""
    from diffusion_models_dsdiff_amd._sched import Guidance
    dsa = _sampler()
    for e in (pix, lat):
        ns = dsa.NoiseScheduleVP("discrete", betas=betas())
        for alg, stype, thr in (("dpmsolver++", "dpmsolver", True), ("dpmsolver", "taylor", False), ("dpmsolver++", "taylor", False)):
            fn = dsa.model_wrapper(e["wrap"], ns, model_type="v", model_kwargs=dict(c_concat=[e["c"]]))
            sol = dsa.DPM_Solver(fn, ns, algorithm_type=alg, correcting_x0_fn="dynamic_thresholding" if thr else None)
            args = dict(steps=7, order=2, skip_type="logSNR", lower_order_final=True, denoise_to_zero=True, solver_type=stype)
            sched, prog = sol.build_schedule(**args), sol.build_program(method="multistep", **args)
            assert prog.kind.tolist() == sched.order.tolist()
            for guided in (False, True):
                g = (lambda n: Guidance(torch.zeros_like(e["c"]), 3.0, n)) if guided else (lambda n: None)
                old = dsa.run_dpm_loop(fn, sched, e["xT"], g(sched.steps))
                new, _ = dsa.run_dpm_program(fn, prog, e["xT"], g(prog.steps))
                assert torch.equal(old, new), (e["key"], alg, stype, guided)


# ---------------------------------------------------------------------------------------- 4. the generic-callable path
@pytest.mark.parametrize("name", ["ms3_eps_logsnr_7_lof_thr", "ss3_v_taylor_9", "ssf3_v_9_dz"])
def test_generic_callable_path(pix, name):
    """A foreign callable goes through the python loop with dsd_op_dpm_eval per evaluation: the device loop's numbers."""
    closure = lambda x, t, **kw: pix["wrap"](x, t, c_concat=[pix["c"]])
    case = cases(pix["g"], "pix")[name]
    sol, kw = solver(case, closure)
    y, kept = sol.sample(pix["xT"], return_intermediate=True, **kw)
    assert rel_l2(y, pix["g"][f"pix_{name}_y"]) < TOL, name
    dev, dkept = _solve(pix, name)[0].sample(pix["xT"], return_intermediate=True, **kw)
    assert rel_l2(y, dev) < 1e-5 and len(kept) == len(dkept) and torch.equal(kept[-1], y), name


# ---------------------------------------------------------------------------------------- 5. the DiT
def _dit(size, patch):
    """DiT-S/2-sized blocks (hidden 384, 6 heads) at depth 2: 1 state + 3 condition channels, learned sigma."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    kw = dict(U.MODELS["M1"][0], input_size=size, patch_size=patch, hidden_size=384, num_heads=6, depth=2)
    wrap = DiffusionWrapper({"target": U.DIT_TARGET, "params": kw}, "concat")
    wrap.diffusion_model.load_state_dict(U.synth_params(U.names_shapes(kw), U.WEIGHT_SEED), strict=True)
    return wrap


def _per_step(unet, prog, xT, c):
    """The per-step loop: DiT.forward (dsd_block_forward) on the concatenated input, then dsd_op_dpm_eval."""
    L = _lib()
    B, Cz, H, W = xT.shape
    x = xT.clone()
    hist, base = x.new_empty((3, B, Cz, H, W)), torch.empty_like(x)
    for k in range(prog.steps):
        out = unet(torch.cat([x, c], 1), torch.full((B,), float(prog.t_input[k]), device="cuda")).contiguous()
        L.check(L.lib().dsd_op_dpm_eval(C.byref(prog.c), k, None, L.dptr(out), out.shape[1] // Cz, 1., L.dptr(x), 0, L.dptr(hist),
                                        L.dptr(base), B, Cz, H, W, L.stream_ptr()))
    return x


@pytest.mark.parametrize("size,patch", [(8, 2), (15, 3)])
def test_dit_loop_equals_the_per_step_path(size, patch):
    """8x8 (16-byte path) and 15x15 (225 elements: scalar path, state rows inside the 4-channel input unaligned): the device loop
    equals the per-step loop bit for bit, singlestep order 3 and multistep order 3 with thresholding, bf16x6 and f16."""
    dsa = _sampler()
    _lib().require_gpu(0)
    wrap = _dit(size, patch)
    unet = wrap.diffusion_model
    xT, c = randn((3, 1, size, size), 2201).cuda(), randn((3, 3, size, size), 2202).cuda()
    ns = dsa.NoiseScheduleVP("discrete", betas=U.spaced_betas())
    sol = dsa.DPM_Solver(dsa.model_wrapper(wrap, ns, model_type="noise", model_kwargs=dict(c_concat=[c])), ns,
                         algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding")
    try:
        for prec in ("bf16x6", "f16"):
            unet.set_precision(prec)
            for kw in (dict(steps=6, order=3, method="singlestep", skip_type="logSNR"),
                       dict(steps=5, order=3, method="multistep", skip_type="time_uniform", solver_type="taylor")):
                y = sol.sample(xT, **kw)
                assert bool(torch.isfinite(y).all())
                assert torch.equal(y, _per_step(unet, sol.build_program(**kw), xT, c)), (size, prec, kw)
    finally:
        unet.set_precision("bf16x6")


# ---------------------------------------------------------------------------------------- 6. graph replay, intermediates
def test_graph_replay_is_bit_identical(pix, lat):
    L = _lib()
    for e, name in ((pix, "ss3_eps_logsnr_10_thr"), (lat, "ss3_v_cfg_9")):
        sol, kw, x, run = _solve(e, name)
        dev = run(x, **kw)
        caps, launches = C.c_int(), C.c_int()
        L.check(L.lib().dsd_graph_stats(e["unet"]._h, C.byref(caps), C.byref(launches)))
        before = launches.value
        L.check(L.lib().dsd_set_graph(e["unet"]._h, 1))
        try:
            rep, rep2 = run(x, **kw), run(x, **kw)
            L.check(L.lib().dsd_graph_stats(e["unet"]._h, C.byref(caps), C.byref(launches)))
        finally:
            L.check(L.lib().dsd_set_graph(e["unet"]._h, 0))
        assert launches.value > before and torch.equal(rep, dev) and torch.equal(rep2, dev), name


def test_return_intermediate(pix):
    """The reference's count of entries (one per outer step for singlestep; x_T and one per update for multistep; one more with
    denoise_to_zero), the last entry is the final state, the final state is the run's without intermediates, and every entry of
    the recorded case is within the chain bar of the fixture's."""
    g = pix["g"]
    sol, kw, x, run = _solve(pix, "ss3_v_uniform_9")
    y, kept = run(x, return_intermediate=True, **kw)
    want = g["pix_ss3_v_uniform_9_inter"]
    assert len(kept) == want.shape[0] == 4
    assert torch.equal(kept[-1], y) and torch.equal(y, run(x, **kw))
    for i, (a, b) in enumerate(zip(kept, want)):
        assert rel_l2(a, b) < TOL, i
    sol, kw, x, run = _solve(pix, "ms3_eps_logsnr_7_lof_thr")
    y, kept = run(x, return_intermediate=True, **kw)
    assert len(kept) == 8 and torch.equal(kept[0], x) and torch.equal(kept[-1], y) and torch.equal(y, run(x, **kw))
    sol, kw, x, run = _solve(pix, "ssf3_v_9_dz")
    y, kept = run(x, return_intermediate=True, **kw)
    assert len(kept) == 4 and torch.equal(kept[-1], y) and torch.equal(y, run(x, **kw))
    y2, kept2 = sol.sample(x, steps=6, order=2, return_intermediate=True)       # order 2 with intermediates: the program's route
    assert len(kept2) == 7 and torch.equal(y2, sol.sample(x, steps=6, order=2))


# ---------------------------------------------------------------------------------------- 7. rejections
def test_rejections_leave_the_state_untouched(pix, lat):
    dsa, L = _sampler(), _lib()
    gen = torch.Generator().manual_seed(23)
    good = lambda: _program([4, 5, 8, 1, 2, 3, 0], 2, 1, 1, gen)         # a singlestep step, then the multistep ramp
    for e in (pix, lat):
        x = e["xT"].clone()
        B, Cz, H, W = x.shape
        scales = np.full(7, 3.0, np.float32)
        u = torch.zeros_like(e["c"])

        def call(p, guid=None, inter=None, cond=e["c"], xx=x):
            gp = C.byref(guid) if guid is not None else None
            return L.lib().dsd_sample_dpm_program(e["unet"]._h, C.byref(p.c), gp, L.dptr(cond), e["c"].shape[1], L.dptr(xx), Cz, B, H,
                                                  W, inter, L.stream_ptr())

        def rejected(rc, text):
            msg = L.lib().dsd_last_error().decode()
            assert rc != 0 and text in msg, (text, msg)
        p = good()
        p.kind[2] = 9
        rejected(call(p), "evaluation 2 has kind 9; the table ends at 8")
        p = good()
        p.kind[0] = -1
        rejected(call(p), "evaluation 0 has kind -1")
        rejected(call(_program([2], 2, 1, 1, gen)), "evaluation 0 (kind 2) reads history plane 0 as model value 2, which no evaluation")
        rejected(call(_program([1, 3], 2, 1, 1, gen)), "evaluation 1 (kind 3) reads history plane 1 as model value 2")
        rejected(call(_program([5, 8], 2, 1, 1, gen)), "evaluation 0 (kind 5) comes after 0 stage(s) of a singlestep step; it needs 1")
        rejected(call(_program([4, 8], 2, 1, 1, gen)), "evaluation 1 (kind 8) comes after 1 stage(s) of a singlestep step; it needs 2")
        rejected(call(_program([4, 1], 2, 1, 1, gen)), "evaluation 1 (kind 1) comes after 1 stage(s) of a singlestep step; it needs 0")
        rejected(call(_program([4, 5], 2, 1, 1, gen)), "it ends after 2 stage(s) of a singlestep step")
        p = good()
        p.slot[1, 2] = 3
        rejected(call(p), "evaluation 1 names history plane 3 (slot[2]); there are planes 0..2")
        p = good()
        p.c.threshold_ratio = 1.5
        rejected(call(p), "threshold_ratio 1.5 outside [0,1]")
        p = good()
        p.c.coef = None
        rejected(call(p), "null array")
        p = good()
        rejected(call(p, cond=None), "null argument")
        rejected(call(p, L.DsdGuidance(u.data_ptr(), scales.ctypes.data_as(C.POINTER(C.c_float)), 6)),
                 "guidance carries 6 scales but the schedule executes 7 steps")
        rejected(call(p, L.DsdGuidance(None, scales.ctypes.data_as(C.POINTER(C.c_float)), 7)), "uncond is null")
        p.keep[2] = 1
        rejected(call(p), "keeps 1 intermediate states but the output for them is null")
        # the per-evaluation op
        p = good()
        out, hist = torch.zeros_like(x), x.new_zeros((3,) + tuple(x.shape))
        rc = L.lib().dsd_op_dpm_eval(C.byref(p.c), 1, None, L.dptr(out), 1, 1., L.dptr(x), 0, L.dptr(hist), None, B, Cz, H, W,
                                     L.stream_ptr())
        rejected(rc, "evaluation 1 (kind 5) is a singlestep stage: it needs the base plane")
        rc = L.lib().dsd_op_dpm_eval(C.byref(p.c), 7, None, L.dptr(out), 1, 1., L.dptr(x), 0, L.dptr(hist), None, B, Cz, H, W,
                                     L.stream_ptr())
        rejected(rc, "evaluation 7 of a program of 7")
        rc = L.lib().dsd_op_dpm_eval(C.byref(p.c), 0, None, L.dptr(out), 1, 1., L.dptr(x), 3, L.dptr(hist), L.dptr(out), B, Cz, H, W,
                                     L.stream_ptr())
        rejected(rc, "x_row_stride 3 is smaller than one sample")
        assert torch.equal(x, e["xT"])                                        # nothing ran
    # the Python surface
    ns = dsa.NoiseScheduleVP("discrete", betas=betas())
    sol = dsa.DPM_Solver(dsa.model_wrapper(pix["wrap"], ns, model_kwargs=dict(c_concat=[pix["c"]])), ns)
    with pytest.raises(NotImplementedError, match="error norm"):
        sol.sample(pix["xT"], method="adaptive")
    foreign = dsa.model_wrapper(lambda xx, t, cc: xx, ns, guidance_type="classifier-free", condition=pix["c"],
                                unconditional_condition=torch.zeros_like(pix["c"]), guidance_scale=3.)
    with pytest.raises(NotImplementedError, match="device loop only"):
        dsa.DPM_Solver(foreign, ns).sample(pix["xT"], steps=9, order=3, method="singlestep")
