#!/usr/bin/env python3
"""Generate tests/golden/dpm_adaptive.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dpm_adaptive.py

The reference's own DPM_Solver.dpm_solver_adaptive (Disc_diff/guided_diffusion/sampler.py:921-980; the guided case and the
latent case from the twin ldm/models/diffusion/dpm_solver_new/dpm_solver_pytorch.py:958-1012, whose model_wrapper has the
guidance), on the models, seeds and perturbation of gen_dpm_family.py:

  pixel cases   the `tiny` DSUnetModel of model.npz: B = 2, 1x32x32, cond seed 80, x_T seed 81, linear betas, t_T = 1, t_0 = 1e-3
  latent case   the UNetModel of latent_ldm.npz: B = 2, 4x8x8 state, 8 'concat' channels, c = randn(700), v-prediction

Per case the run records, trial by trial, (s, t), the error norm E and whether the trial was accepted.  A case is stored only
if: the network was evaluated order x trials times; the run repeated with Gaussian noise of 3e-6 relative RMS on every network
output takes the same accept / reject sequence and moves the sample by less than gen_dpm_family.py's MOVE_MAX; and the closest
any E comes to the decision threshold, min |E - 1|, is at least ten times the largest |dE| that noise produced in any trial.
e_tol = min |E - 1| / 10 is stored: an E within e_tol of the recorded one cannot flip a decision, and a forward error of the
size of the perturbation stays within it.  The kept set must hold an order-2 and an order-3 case with two or more rejections
each and one case without any.

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
from gen_dpm_family import MOVE_MAX, PERTURB, PERTURB_SEED, PLAIN, PP, SCALE, THR, betas_b, modules, rel  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_grad_enabled(False)
torch.set_num_threads(8)

T_T, T_0 = 1.0, 1e-3
E_MARGIN = 10.0
TOL, LOOSE = dict(atol=0.0078, rtol=0.05), dict(atol=0.05, rtol=0.2)

# name -> dict(mod "A" (Disc_diff copy) | "B" (LDM twin), model_type, solver kwargs, order, adaptive kwargs, scale)
PIX_CASES = {
    "ad2_v_pp": dict(mod="A", mtype="v", sol=PP, order=2, ad=dict(TOL)),
    "ad2_v_plain": dict(mod="A", mtype="v", sol=PLAIN, order=2, ad=dict(TOL)),
    "ad3_v_pp": dict(mod="A", mtype="v", sol=PP, order=3, ad=dict(TOL)),
    "ad3_v_plain_loose": dict(mod="A", mtype="v", sol=PLAIN, order=3, ad=dict(LOOSE)),
    "ad2_eps_pp": dict(mod="A", mtype="noise", sol=PP, order=2, ad=dict(TOL)),
    "ad3_v_pp_taylor": dict(mod="A", mtype="v", sol=PP, order=3, ad=dict(TOL, solver_type="taylor")),
    "ad3_v_plain_taylor_loose": dict(mod="A", mtype="v", sol=PLAIN, order=3, ad=dict(LOOSE, solver_type="taylor")),
    "ad2_v_pp_thr": dict(mod="A", mtype="v", sol=dict(PP, **THR), order=2, ad=dict(TOL)),
    "ad3_eps_pp_thr": dict(mod="A", mtype="noise", sol=dict(PP, **THR), order=3, ad=dict(TOL)),
    "ad3_v_pp_cfg": dict(mod="B", mtype="v", sol=PP, order=3, ad=dict(TOL), scale=SCALE),
    "ad2_v_pp_cfg": dict(mod="B", mtype="v", sol=PP, order=2, ad=dict(TOL), scale=SCALE),
}
LAT_CASES = {
    "ad2_v_pp": dict(mod="B", mtype="v", sol=PP, order=2, ad=dict(TOL)),
    "ad3_v_pp": dict(mod="B", mtype="v", sol=PP, order=3, ad=dict(TOL)),
}


def run(net, case, x, c, perturb=False):
    """One run of the reference's adaptive solver; returns (sample, E per trial, (s, t) per trial, network evaluations)."""
    mod = modules()[case["mod"]]
    scale = case.get("scale", 1.)
    ns = mod.NoiseScheduleVP("discrete", betas=betas_b())
    gen = torch.Generator().manual_seed(PERTURB_SEED)
    count = [0]

    def model(x_in, t, cc=None, c_concat=None):
        count[0] += 1
        out = net(torch.cat([x_in] + (c_concat if c_concat is not None else [cc]), 1), t)
        if perturb:
            out = out + PERTURB * out.pow(2).mean().sqrt() * torch.randn(out.shape, generator=gen)
        return out
    if case["mod"] == "A":
        fn = mod.model_wrapper(model, ns, model_type=case["mtype"], model_kwargs=dict(c_concat=[c]))
    else:
        fn = mod.model_wrapper(model, ns, model_type=case["mtype"], guidance_type="classifier-free", condition=c,
                               unconditional_condition=torch.zeros_like(c) if scale != 1. else None, guidance_scale=scale)
    sol = mod.DPM_Solver(fn, ns, **case["sol"])
    E, st = [], []
    first, second, power = sol.dpm_solver_first_update, sol.singlestep_dpm_solver_second_update, torch.float_power

    def lower_of(update):                                   # the lower-order update is the call that returns its intermediates
        def f(xx, s, t, *a, **kw):
            if kw.get("return_intermediate"):
                st.append([float(s.reshape(-1)[0]), float(t.reshape(-1)[0])])
            return update(xx, s, t, *a, **kw)
        return f

    def float_power(e, p):                                  # :977 — the one place E is used after the accept / reject decision
        E.append(float(e))
        return power(e, p)
    sol.dpm_solver_first_update, sol.singlestep_dpm_solver_second_update = lower_of(first), lower_of(second)
    torch.float_power = float_power
    try:
        y = sol.dpm_solver_adaptive(x.clone(), case["order"], T_T, T_0, **case["ad"])
    finally:
        torch.float_power = power
    assert len(E) == len(st), (len(E), len(st))
    return y.numpy(), np.asarray(E, np.float32), np.asarray(st, np.float32), count[0]


def space(out, sp, net, x_T, c, cases):
    kept = {}
    for name, case in cases.items():
        y, E, st, n_eval = run(net, case, x_T, c)
        acc = E <= 1.
        yp, Ep, _, n_eval_p = run(net, case, x_T, c, perturb=True)
        same = len(Ep) == len(E) and bool(((Ep <= 1.) == acc).all())
        move = rel(yp, y)
        gap = float(np.abs(E - 1.).min())
        dE = float(np.abs(Ep - E).max()) if same else float("inf")
        print(f"{sp}_{name}: {len(E)} trials, {int((~acc).sum())} rejected, nfe {n_eval}, min |E-1| {gap:.3g}, perturbed: same sequence "
              f"{same}, moved {move:.2e}, max |dE| {dE:.2e} (margin {gap / dE if dE else float('inf'):.0f}x)")
        ok = (bool(np.isfinite(y).all()) and n_eval == case["order"] * len(E) and n_eval_p == n_eval and same and move < MOVE_MAX
              and gap >= E_MARGIN * dE)
        if not ok:
            print(f"{sp}_{name}: DROPPED")
            continue
        kept[name] = case
        out[f"{sp}_{name}_y"] = y
        out[f"{sp}_{name}_nfe"] = np.asarray(n_eval)
        out[f"{sp}_{name}_E"] = E
        out[f"{sp}_{name}_accepted"] = acc
        out[f"{sp}_{name}_st"] = st
        out[f"{sp}_{name}_e_tol"] = np.float64(gap / E_MARGIN)
    out[f"{sp}_cases"] = json.dumps(kept)
    return {n: int((~(out[f"{sp}_{n}_accepted"])).sum()) for n in kept}, kept


def main():
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from UNet_DS_Diff.model import DSUnetModel
    out = {"scale": np.float64(SCALE), "t_T": np.float64(T_T), "t_0": np.float64(T_0)}

    gm = np.load(os.path.join(OUT, "model.npz"), allow_pickle=False)
    t = DSUnetModel(**json.loads(str(gm["tiny_cfg"])))
    t.load_state_dict(_params(gm, "tiny"), strict=True)
    t.eval()
    shape = (2, 1, 32, 32)
    out.update({"pix_cond_seed": np.asarray(80), "pix_xT_seed": np.asarray(81)})
    rej, cases = space(out, "pix", lambda x, tt: t(x, tt)[0], randn(shape, 81), cond_image(shape, 80), PIX_CASES)

    gl = np.load(os.path.join(OUT, "latent_ldm.npz"), allow_pickle=False)
    ucfg = json.loads(str(gl["unet_cfg"]))
    m = UNetModel(**ucfg)
    m.load_state_dict(_params(gl, "unet"), strict=True)
    m.eval()
    out.update({"lat_unet_cfg": json.dumps(ucfg), "lat_xT_seed": np.asarray(int(gl["xT_seed"])), "lat_c_seed": np.asarray(700)})
    space(out, "lat", lambda x, tt: m(x, tt), randn((2, 4, 8, 8), int(gl["xT_seed"])), randn((2, 8, 8, 8), 700), LAT_CASES)

    for order in (2, 3):
        assert any(cases[n]["order"] == order and r >= 2 for n, r in rej.items()), f"no order-{order} case with two rejections"
    assert any(r == 0 for r in rej.values()), "no accept-only case"
    np.savez_compressed(os.path.join(OUT, "dpm_adaptive.npz"), **out)
    print("wrote dpm_adaptive", len(out), "entries,", os.path.getsize(os.path.join(OUT, "dpm_adaptive.npz")), "bytes")


if __name__ == "__main__":
    main()
