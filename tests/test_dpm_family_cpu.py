"""CPU side of the DPM-Solver family (tests/golden/dpm_family.npz, tests/golden/gen_dpm_family.py): the host program builder
against the reference's recorded order lists, outer timesteps, evaluation times and r1 / r2; the restatement of
tests/dpm_family_ref.py driven by the oracle networks against every fixture case — which pins the fixture to the reference and
the operation order the device kernels follow; the product program interpreted on the CPU against that restatement, bit for
bit; and the options that still raise."""
import json

import numpy as np
import pytest
import torch

from oracle import dpm as ODPM, schedules as S, unet as O
from util import golden, fixture_params, rel_l2, randn, cond_image
import dpm_family_ref as R

TOL = 1e-5        # the bar of test_plms_cpu.py / test_cfg_cpu.py for their chains
SKIPS = ("logSNR", "time_uniform", "time_quadratic")


def betas():
    return torch.tensor(S.make_beta_schedule("linear", 1000, 1e-4, 2e-2), dtype=torch.float32)


def cases(g, space):
    return json.loads(str(g[space + "_cases"]))


def ref_kwargs(case, **over):
    """The fixture's case -> keyword arguments of dpm_family_ref.ref_sample."""
    kw = dict(case["smp"])
    kw.update(model_type=case["mtype"], algorithm=case["sol"]["algorithm_type"],
              thresholding=case["sol"].get("correcting_x0_fn") == "dynamic_thresholding", inverse=bool(case.get("inverse")))
    kw.update(over)
    return kw


def solver(case, model, cond=None, uncond=None, model_kwargs=None):
    """The product's DPM_Solver for a fixture case and its sample() keyword arguments."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    ns = dsa.NoiseScheduleVP("discrete", betas=betas())
    if uncond is not None:
        fn = dsa.model_wrapper(model, ns, model_type=case["mtype"], guidance_type="classifier-free", condition=cond,
                               unconditional_condition=uncond, guidance_scale=case.get("scale", 1.))
    else:
        fn = dsa.model_wrapper(model, ns, model_type=case["mtype"], model_kwargs=model_kwargs or {})
    sol = dsa.DPM_Solver(fn, ns, **case["sol"])
    return sol, dict(case["smp"])


def pixel_env():
    g, gm = golden("dpm_family"), golden("model")
    cfg, sd = O.UNetConfig.from_params(json.loads(str(gm["tiny_cfg"]))), fixture_params(gm, "tiny")
    net = lambda xx, tt: O.unet_forward(cfg, sd, xx, tt)[0]
    c = cond_image((2, 1, 32, 32), int(g["pix_cond_seed"]))
    return g, net, c, randn((2, 1, 32, 32), int(g["pix_xT_seed"]))


def latent_env():
    g, gl = golden("dpm_family"), golden("latent_ldm")
    up = json.loads(str(g["lat_unet_cfg"]))
    assert up == json.loads(str(gl["unet_cfg"]))
    ucfg, usd = O.UNetConfig.from_params(up), fixture_params(gl, "unet")
    net = lambda xx, tt: O.plain_unet_forward(ucfg, usd, xx, tt)
    return g, net, randn((2, 8, 8, 8), int(g["lat_c_seed"])), randn((2, 4, 8, 8), int(g["lat_xT_seed"]))


PIXEL = {"ms3_v_uniform_10", "ms3_eps_logsnr_7_lof_thr", "ms3_eps_plain_9", "ss3_v_uniform_9", "ss3_eps_logsnr_10_thr",
         "ss3_eps_plain_quad_11", "ss3_v_taylor_9", "ss3_eps_plain_taylor_logsnr_9", "ss2_x0_uniform_7", "ss2_eps_plain_taylor_8",
         "ss1_eps_5", "ssf3_v_9_dz", "inverse_ms2_v_10", "ss3_v_cfg_9"}


def test_fixture_holds_every_case():
    g = golden("dpm_family")
    assert set(cases(g, "pix")) == PIXEL and set(cases(g, "lat")) == {"ms3_v_10", "ss3_v_cfg_9"}


# ---------------------------------------------------------------------------------------- host tables
def test_builder_reproduces_recorded_orders_and_outer_timesteps():
    """get_orders_and_timesteps_for_singlestep_solver for steps 5..12 x order 1..3 x the three skip types, bit for bit — both ways
    of placing the outer times (K points for logSNR, the `steps` grid indexed otherwise)."""
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    g = golden("dpm_family")
    ns = dsa.NoiseScheduleVP("discrete", betas=betas())
    sol = dsa.DPM_Solver(dsa.model_wrapper(lambda x, t: x, ns), ns)
    ons = ODPM.NoiseSchedule(betas=betas())
    n = 0
    for skip in SKIPS:
        for order in (1, 2, 3):
            for steps in range(5, 13):
                outer, orders = sol.get_orders_and_timesteps_for_singlestep_solver(steps, order, skip, ns.T, 1. / ns.total_N)
                tag = f"tab_{skip}_{order}_{steps}"
                assert list(orders) == g[tag + "_orders"].tolist(), tag
                np.testing.assert_array_equal(outer.numpy(), g[tag + "_outer"], err_msg=tag)
                o2, ord2 = R.singlestep_orders(ons, steps, order, skip, ons.T, 1. / ons.total_N)   # the restatement's too
                assert ord2 == list(orders) and torch.equal(o2, outer), tag
                n += 1
    assert n == 72


@pytest.mark.parametrize("name", ["ss3_v_uniform_9", "ss3_eps_logsnr_10_thr"])
def test_program_matches_recorded_evaluations(name):
    """Evaluation times, alpha / sigma there and r1 / r2 of every singlestep step, as the reference's run recorded them: fp32
    equality.  r1 / r2 are read back from the program's taylor rows (coef 6, 7), which carry them as they are."""
    g, _, c, xT = pixel_env()
    case = cases(g, "pix")[name]
    sol, kw = solver(case, lambda x, t, **k: x)
    prog = sol.build_program(**kw)
    assert prog.steps == kw["steps"]
    np.testing.assert_array_equal(np.asarray([e["t"] for e in prog.evals], np.float32), g[f"pix_{name}_rec_t"])
    np.testing.assert_array_equal(prog.alpha, g[f"pix_{name}_rec_alpha"])
    np.testing.assert_array_equal(prog.sigma, g[f"pix_{name}_rec_sigma"])
    taylor = sol.build_program(**dict(kw, solver_type="taylor"))
    r = np.asarray([taylor.coef[k, 6:8] for k in range(taylor.steps) if taylor.kind[k] == 8], np.float32)
    rec = g[f"pix_{name}_rec_r"]
    np.testing.assert_array_equal(r, rec[rec[:, 1] != 0])
    rec_ref = {}
    R.ref_sample(lambda x, t: x, ODPM.NoiseSchedule(betas=betas()), xT.clone(), record=rec_ref, **ref_kwargs(case))
    np.testing.assert_array_equal(np.asarray(rec_ref["r"], np.float32), rec)
    np.testing.assert_array_equal(np.asarray(rec_ref["t"], np.float32), g[f"pix_{name}_rec_t"])


def test_program_shapes():
    """Kinds, slots and kept states of the programs the builder packs: the ramp 1,2,3,...,2,1 of lower_order_final, the ring of
    three planes, one kept state per reference append."""
    g = golden("dpm_family")
    table = cases(g, "pix")
    sol, kw = solver(table["ms3_eps_logsnr_7_lof_thr"], lambda x, t, **k: x)
    p = sol.build_program(return_intermediate=True, **kw)
    assert p.kind.tolist() == [1, 2, 3, 3, 3, 2, 1] and p.c.thresholding == 1 and p.lead_intermediate and p.n_kept == 7
    assert p.slot[:, 0].tolist() == [0, 1, 2, 0, 1, 2, 0] and p.slot[4].tolist() == [1, 1, 0, 2]
    sol, kw = solver(table["ms3_eps_plain_9"], lambda x, t, **k: x)
    assert sol.build_program(**kw).kind.tolist() == [1, 2, 3, 3, 3, 3, 3, 3, 3]
    sol, kw = solver(table["ss3_v_uniform_9"], lambda x, t, **k: x)
    p = sol.build_program(return_intermediate=True, **kw)
    assert p.kind.tolist() == [4, 5, 7, 4, 5, 7, 4, 6, 1] and p.keep.tolist() == [0, 0, 1, 0, 0, 1, 0, 1, 1] and not p.lead_intermediate
    sol, kw = solver(table["ssf3_v_9_dz"], lambda x, t, **k: x)
    assert sol.build_program(**kw).kind.tolist() == [4, 5, 7] * 3 + [0]
    sol, kw = solver(table["ss3_v_taylor_9"], lambda x, t, **k: x)
    assert sol.build_program(**kw).kind.tolist() == [4, 5, 8, 4, 5, 8, 4, 6, 1]


# ---------------------------------------------------------------------------------------- fixture chains
def _run_ref(net, c, x, case, u=None, **over):
    kw = ref_kwargs(case, **over)
    f = lambda xx, tt: net(torch.cat([xx, c], 1), tt)
    fu = (lambda xx, tt: net(torch.cat([xx, u], 1), tt)) if u is not None else None
    return R.ref_sample(f, ODPM.NoiseSchedule(betas=betas()), x.clone(), net_uncond=fu, scale=case.get("scale", 1.), **kw)


@pytest.mark.parametrize("name", sorted(PIXEL))
def test_restatement_reproduces_the_reference_pixel(name):
    g, net, c, xT = pixel_env()
    case = cases(g, "pix")[name]
    x = torch.from_numpy(g[f"pix_{name}_x"]) if case.get("inverse") else xT
    u = torch.zeros_like(c) if case.get("scale", 1.) != 1. else None
    if case.get("intermediates"):
        y, kept = _run_ref(net, c, x, case, u, return_intermediate=True)
        want = g[f"pix_{name}_inter"]
        assert len(kept) == want.shape[0]
        for a, b in zip(kept, want):
            assert rel_l2(a, b) < TOL, name
    else:
        y = _run_ref(net, c, x, case, u)
    assert rel_l2(y, g[f"pix_{name}_y"]) < TOL, (name, rel_l2(y, g[f"pix_{name}_y"]))


@pytest.mark.parametrize("name", ["ms3_v_10", "ss3_v_cfg_9"])
def test_restatement_reproduces_the_reference_latent(name):
    g, net, c, xT = latent_env()
    case = cases(g, "lat")[name]
    u = torch.zeros_like(c) if case.get("scale", 1.) != 1. else None
    y = _run_ref(net, c, xT, case, u)
    assert rel_l2(y, g[f"lat_{name}_y"]) < TOL, (name, rel_l2(y, g[f"lat_{name}_y"]))


@pytest.mark.parametrize("name", ["ms3_eps_logsnr_7_lof_thr", "ms3_eps_plain_9", "ss3_v_taylor_9", "ss3_eps_plain_taylor_logsnr_9",
                                  "ss3_eps_plain_quad_11", "ss2_x0_uniform_7", "ss2_eps_plain_taylor_8", "ssf3_v_9_dz",
                                  "inverse_ms2_v_10", "ss3_v_cfg_9"])
def test_program_interpreted_on_cpu_equals_the_restatement(name):
    """The product's program, run row by row with the kernels' torch operations, equals the reference's expressions bit for bit on
    the same network: the host scalars, the folded signs and the slot scheme are the reference's arithmetic."""
    g, net, c, xT = pixel_env()
    case = cases(g, "pix")[name]
    x = torch.from_numpy(g[f"pix_{name}_x"]) if case.get("inverse") else xT
    guided = case.get("scale", 1.) != 1.
    u = torch.zeros_like(c) if guided else None
    sol, kw = solver(case, lambda xx, tt, **k: xx)
    prog = (sol.build_program(**kw) if not case.get("inverse") else
            sol.build_program(kw.pop("steps"), t_start=1. / sol.noise_schedule.total_N, t_end=sol.noise_schedule.T, **kw))
    f = lambda xx, tt: net(torch.cat([xx, c], 1), tt)
    fu = (lambda xx, tt: net(torch.cat([xx, u], 1), tt)) if guided else None
    y, _ = R.run_program_cpu(prog, f, x.clone(), fu, case.get("scale", 1.))
    np.testing.assert_array_equal(y.numpy(), _run_ref(net, c, x, case, u).numpy(), err_msg=name)


# ---------------------------------------------------------------------------------------- what still raises
def test_unbuilt_options_raise_with_a_reason():
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import sampler as dsa
    ns = dsa.NoiseScheduleVP("discrete", betas=betas())
    sol = dsa.DPM_Solver(dsa.model_wrapper(lambda x, t, **k: x, ns), ns)
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="error norm"):
        sol.sample(x, method="adaptive")
    with pytest.raises(NotImplementedError, match="correcting_xt_fn"):
        dsa.DPM_Solver(dsa.model_wrapper(lambda x, t: x, ns), ns, correcting_xt_fn=lambda x, t, s: x)
    with pytest.raises(NotImplementedError, match="classifier guidance"):
        dsa.model_wrapper(lambda x, t: x, ns, guidance_type="classifier")
    with pytest.raises(NotImplementedError, match="score-type"):
        dsa.DPM_Solver(dsa.model_wrapper(lambda x, t: x, ns, model_type="score"), ns)
    with pytest.raises(ValueError, match="wrong method"):
        sol.sample(x, method="euler")
    with pytest.raises(ValueError, match="order must be"):
        sol.sample(x, order=4)
    with pytest.raises(ValueError, match="solver_type"):
        sol.sample(x, order=3, solver_type="heun")
    with pytest.raises(NotImplementedError, match="no CPU"):                  # CPU tensors never fall back to a CPU loop
        sol.sample(x, steps=9, order=3, method="singlestep")
    assert callable(sol.inverse)


def test_ctypes_mirror_of_the_program_struct():
    """The struct's size, the coefficient width and the kind values of the binding against the header's, parsed from it."""
    import ctypes as C
    import os
    import re
    from diffusion_models_dsdiff_amd import _lib
    assert C.sizeof(_lib.DsdDpmProgram) == 24 + 7 * C.sizeof(C.c_void_p)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsdiff.h")) as f:
        h = f.read()
    assert int(re.search(r"#define\s+DSD_DPM_NCOEF\s+(\d+)", h).group(1)) == _lib.DSD_DPM_NCOEF == 9
    kinds = {k: int(v) for k, v in re.findall(r"DSD_DPM_((?:MS|SS)\w+)\s*=\s*(\d+)", h)}
    assert kinds == {"MS0": _lib.DPM_MS0, "MS1": _lib.DPM_MS1, "MS2": _lib.DPM_MS2, "MS3": _lib.DPM_MS3, "SS_S1": _lib.DPM_SS_S1,
                     "SS_S2": _lib.DPM_SS_S2, "SS_T2": _lib.DPM_SS_T2, "SS_T3": _lib.DPM_SS_T3,
                     "SS_T3_TAYLOR": _lib.DPM_SS_T3_TAYLOR}
    assert sorted(kinds.values()) == list(range(9))
