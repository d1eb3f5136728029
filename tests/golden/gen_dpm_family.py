#!/usr/bin/env python3
"""Generate tests/golden/dpm_family.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dpm_family.py

The reference's own DPM_Solver.sample / .inverse for what dpm.npz does not hold: multistep order 3, the singlestep solvers
("DPM-Solver-fast", singlestep_fixed) of order 1..3, both algorithm types and solver types, return_intermediate, inverse, one
guided case per space.  Disc_diff/guided_diffusion/sampler.py runs every unguided case but the x_start one (its noise_pred_fn
does not broadcast alpha_t over images for model_type="x_start", :256-257) and has its guidance commented out (:281-298), so
the x_start case and the guided cases come from the twin ldm/models/diffusion/dpm_solver_new/dpm_solver_pytorch.py.

  pixel cases   the `tiny` DSUnetModel of model.npz: B = 2, 1x32x32, cond seed 80, x_T seed 81 (those of dpm.npz), linear betas
  latent cases  the UNetModel of latent_ldm.npz: B = 2, 4x8x8 state, 8 'concat' channels, c = randn(700), v-prediction

Three checks run here and a case that fails one is not stored: the network is evaluated `steps` times (+1 with denoise_to_zero);
the case, re-run with Gaussian noise of 3e-6 relative RMS on every network output (the size of the GPU-against-oracle forward
error), moves by less than 2e-5 — a fifth of the 1e-4 chain bar; and it lies more than 1e-3 rel-L2 (ten chain bars) from its
named twin (lower order, other method, other solver type or unguided), so a loop that falls back cannot pass.

Stored: outputs, recorded tables, seeds and the cases' json only.  Weights regenerate from synth_params; inputs from seeds.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ["DSD_REFERENCE"])
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

from oracle.synth import randn, cond_image  # noqa: E402
from gen_cfg import _params  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_grad_enabled(False)
torch.set_num_threads(8)

SCALE = 3.0
PERTURB, MOVE_MAX, TWIN_MIN = 3e-6, 2e-5, 1e-3
PERTURB_SEED = 760
THR = dict(correcting_x0_fn="dynamic_thresholding")
PP, PLAIN = dict(algorithm_type="dpmsolver++"), dict(algorithm_type="dpmsolver")

# name -> dict(mod "A" (Disc_diff copy) | "B" (LDM twin), model_type, solver kwargs, sample kwargs, scale, twin = the sample /
# solver kwargs that differ in the twin run, inverse, intermediates)
PIX_CASES = {
    "ms3_v_uniform_10": dict(mod="A", mtype="v", sol=PP, smp=dict(steps=10, order=3, skip_type="time_uniform", method="multistep"),
                             twin=dict(order=2)),
    "ms3_eps_logsnr_7_lof_thr": dict(mod="A", mtype="noise", sol=dict(PP, **THR),
                                     smp=dict(steps=7, order=3, skip_type="logSNR", method="multistep"), twin=dict(order=2)),
    "ms3_eps_plain_9": dict(mod="A", mtype="noise", sol=PLAIN,
                            smp=dict(steps=9, order=3, skip_type="time_uniform", method="multistep", lower_order_final=False),
                            twin=dict(order=2)),
    "ss3_v_uniform_9": dict(mod="A", mtype="v", sol=PP, smp=dict(steps=9, order=3, skip_type="time_uniform", method="singlestep"),
                            twin=dict(order=2), intermediates=True, record=True),
    "ss3_eps_logsnr_10_thr": dict(mod="A", mtype="noise", sol=dict(PP, **THR),
                                  smp=dict(steps=10, order=3, skip_type="logSNR", method="singlestep"), twin=dict(order=2), record=True),
    "ss3_eps_plain_quad_11": dict(mod="A", mtype="noise", sol=PLAIN,
                                  smp=dict(steps=11, order=3, skip_type="time_quadratic", method="singlestep"), twin=dict(order=2)),
    "ss3_v_taylor_9": dict(mod="A", mtype="v", sol=PP,
                           smp=dict(steps=9, order=3, skip_type="time_uniform", method="singlestep", solver_type="taylor"),
                           twin=dict(solver_type="dpmsolver")),
    "ss3_eps_plain_taylor_logsnr_9": dict(mod="A", mtype="noise", sol=PLAIN,
                                          smp=dict(steps=9, order=3, skip_type="logSNR", method="singlestep", solver_type="taylor"),
                                          twin=dict(solver_type="dpmsolver")),
    "ss2_x0_uniform_7": dict(mod="B", mtype="x_start", sol=PP, smp=dict(steps=7, order=2, skip_type="time_uniform", method="singlestep"),
                             twin=dict(order=1)),
    "ss2_eps_plain_taylor_8": dict(mod="A", mtype="noise", sol=PLAIN,
                                   smp=dict(steps=8, order=2, skip_type="time_uniform", method="singlestep", solver_type="taylor"),
                                   twin=dict(solver_type="dpmsolver")),
    "ss1_eps_5": dict(mod="A", mtype="noise", sol=PP, smp=dict(steps=5, order=1, skip_type="time_uniform", method="singlestep"),
                      twin=dict(steps=4)),
    "ssf3_v_9_dz": dict(mod="A", mtype="v", sol=dict(PP, **THR),
                        smp=dict(steps=9, order=3, skip_type="time_uniform", method="singlestep_fixed", denoise_to_zero=True),
                        twin=dict(method="singlestep")),
    # inverse of the order-2 twin's output of ms3_v_uniform_10 (x = that output), back up to T
    "inverse_ms2_v_10": dict(mod="A", mtype="v", sol=PP, smp=dict(steps=10, order=2, skip_type="time_uniform", method="multistep"),
                             twin=dict(order=1), inverse=True),
    "ss3_v_cfg_9": dict(mod="B", mtype="v", sol=PP, smp=dict(steps=9, order=3, skip_type="time_uniform", method="singlestep"),
                        scale=SCALE, twin=dict(scale=1.)),
}
LAT_CASES = {
    "ms3_v_10": dict(mod="B", mtype="v", sol=PP, smp=dict(steps=10, order=3, skip_type="time_uniform", method="multistep"),
                     twin=dict(order=2)),
    "ss3_v_cfg_9": dict(mod="B", mtype="v", sol=PP, smp=dict(steps=9, order=3, skip_type="time_uniform", method="singlestep"),
                        scale=SCALE, twin=dict(scale=1.)),
}

rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))


def modules():
    import Disc_diff.guided_diffusion.sampler as sa
    import ldm.models.diffusion.dpm_solver_new.dpm_solver_pytorch as sb
    return {"A": sa, "B": sb}


def betas_b():
    from ldm.modules.diffusionmodules.util import make_beta_schedule
    return torch.tensor(make_beta_schedule("linear", 1000, 1e-4, 2e-2), dtype=torch.float32)


def run(net, case, x, c, perturb=False, rec=None, **over):
    """One run of the reference's solver.  net(x_in [rows,C+Cc,..], t) -> out; ``over``: the twin's differing arguments;
    ``rec``: a dict that receives the evaluation times, alpha / sigma there and the (r1, r2) of every singlestep step."""
    mod = modules()[case["mod"]]
    smp, sol_kw, scale = dict(case["smp"]), dict(case["sol"]), case.get("scale", 1.)
    for k, v in over.items():
        if k == "scale":
            scale = v
        else:
            smp[k] = v
    ns = mod.NoiseScheduleVP("discrete", betas=betas_b())
    gen = torch.Generator().manual_seed(PERTURB_SEED)
    count = [0]

    def model(x_in, t, cc=None, c_concat=None):
        count[0] += 1
        out = net(torch.cat([x_in] + (c_concat if c_concat is not None else [cc]), 1), t)
        if perturb:
            out = out + PERTURB * out.pow(2).mean().sqrt() * torch.randn(out.shape, generator=gen)
        return out
    if case["mod"] == "A":                                  # no guidance in this copy: the condition rides in model_kwargs
        fn = mod.model_wrapper(model, ns, model_type=case["mtype"], model_kwargs=dict(c_concat=[c]))
    else:
        fn = mod.model_wrapper(model, ns, model_type=case["mtype"], guidance_type="classifier-free", condition=c,
                               unconditional_condition=torch.zeros_like(c) if scale != 1. else None, guidance_scale=scale)
    sol = mod.DPM_Solver(fn, ns, **sol_kw)
    if rec is not None:
        mf, upd = sol.model_fn, sol.singlestep_dpm_solver_update
        rec.update(t=[], alpha=[], sigma=[], r=[])

        def model_fn(xx, t):
            rec["t"].append(float(t.reshape(-1)[0]))
            rec["alpha"].append(float(ns.marginal_alpha(t).reshape(-1)[0]))
            rec["sigma"].append(float(ns.marginal_std(t).reshape(-1)[0]))
            return mf(xx, t)

        def update(xx, s, t, order, **kw):
            rec["r"].append([float(kw["r1"]) if kw.get("r1") is not None else 0., float(kw["r2"]) if kw.get("r2") is not None else 0.])
            return upd(xx, s, t, order, **kw)
        sol.model_fn, sol.singlestep_dpm_solver_update = model_fn, update
    inter = bool(case.get("intermediates"))
    y = (sol.inverse if case.get("inverse") else sol.sample)(x.clone(), return_intermediate=inter, **smp)
    y, kept = y if inter else (y, None)
    want = smp["steps"] // smp["order"] * smp["order"] if smp["method"] == "singlestep_fixed" else smp["steps"]
    assert count[0] == want + (1 if smp.get("denoise_to_zero") else 0), (count[0], smp)
    return y.numpy(), (torch.stack(kept).numpy() if inter else None)


def space(out, sp, net, x_T, c, cases):
    kept_cases = {}
    for name, case in cases.items():
        x = x_T
        if case.get("inverse"):                             # starts from the sample of the order-2 multistep run
            x = torch.from_numpy(run(net, dict(cases["ms3_v_uniform_10"]), x_T, c, order=2)[0])
        rec = {} if case.get("record") else None
        y, kept = run(net, case, x, c, rec=rec)
        ok = bool(np.isfinite(y).all())
        move = rel(run(net, case, x, c, perturb=True)[0], y)
        d = rel(run(net, case, x, c, **case["twin"])[0], y)
        print(f"{sp}_{name}: max |y| {np.abs(y).max():.3f}, moved {move:.2e} by {PERTURB:g} noise on the network output, "
              f"rel-L2 to its twin {case['twin']} {d:.2e}")
        if not (ok and move < MOVE_MAX and d > TWIN_MIN):
            print(f"{sp}_{name}: DROPPED (finite {ok}, move {move:.2e} < {MOVE_MAX:g}, twin {d:.2e} > {TWIN_MIN:g})")
            continue
        kept_cases[name] = case
        out[f"{sp}_{name}_y"] = y
        if kept is not None:
            out[f"{sp}_{name}_inter"] = kept
        if case.get("inverse"):
            out[f"{sp}_{name}_x"] = x.numpy()
        if rec is not None:
            for k in ("t", "alpha", "sigma", "r"):
                out[f"{sp}_{name}_rec_{k}"] = np.asarray(rec[k], dtype=np.float32)
    out[f"{sp}_cases"] = json.dumps(kept_cases)


def tables(out):
    """get_orders_and_timesteps_for_singlestep_solver :445-501 for steps 5..12 x order 1..3 x the three skip types."""
    sa = modules()["A"]
    ns = sa.NoiseScheduleVP("discrete", betas=betas_b())
    sol = sa.DPM_Solver(lambda x, t: x, ns)
    for skip in ("logSNR", "time_uniform", "time_quadratic"):
        for order in (1, 2, 3):
            for steps in range(5, 13):
                outer, orders = sol.get_orders_and_timesteps_for_singlestep_solver(steps, order, skip, ns.T, 1. / ns.total_N, "cpu")
                out[f"tab_{skip}_{order}_{steps}_orders"] = np.asarray(orders, dtype=np.int32)
                out[f"tab_{skip}_{order}_{steps}_outer"] = outer.numpy()


def main():
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from UNet_DS_Diff.model import DSUnetModel
    out = {"scale": np.float64(SCALE)}
    tables(out)

    gm = np.load(os.path.join(OUT, "model.npz"), allow_pickle=False)
    t = DSUnetModel(**json.loads(str(gm["tiny_cfg"])))
    t.load_state_dict(_params(gm, "tiny"), strict=True)
    t.eval()
    shape = (2, 1, 32, 32)
    out.update({"pix_cond_seed": np.asarray(80), "pix_xT_seed": np.asarray(81)})
    space(out, "pix", lambda x, tt: t(x, tt)[0], randn(shape, 81), cond_image(shape, 80), PIX_CASES)

    gl = np.load(os.path.join(OUT, "latent_ldm.npz"), allow_pickle=False)
    ucfg = json.loads(str(gl["unet_cfg"]))
    m = UNetModel(**ucfg)
    m.load_state_dict(_params(gl, "unet"), strict=True)
    m.eval()
    out.update({"lat_unet_cfg": json.dumps(ucfg), "lat_xT_seed": np.asarray(int(gl["xT_seed"])), "lat_c_seed": np.asarray(700)})
    space(out, "lat", lambda x, tt: m(x, tt), randn((2, 4, 8, 8), int(gl["xT_seed"])), randn((2, 8, 8, 8), 700), LAT_CASES)

    np.savez_compressed(os.path.join(OUT, "dpm_family.npz"), **out)
    print("wrote dpm_family", len(out), "entries,", os.path.getsize(os.path.join(OUT, "dpm_family.npz")), "bytes")


if __name__ == "__main__":
    main()
