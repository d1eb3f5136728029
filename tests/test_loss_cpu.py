"""The denoising loss without a GPU: the torch restatement of tests/loss_cases.py against what the reference's own
training_losses recorded (tests/golden/loss.npz, tests/golden/gen_loss.py), and the host side of the product's methods — argument
validation, LossType scaling, the two raises, key names, shapes, the ldm loss weights.

DDPM.p_losses / get_loss / get_v and LatentDiffusion.p_losses: the fixture holds the reference's own (gen_loss.py imports its
ddpm.py through the stand-in finder of gen_trace.py); the restatement (loss_cases.restate_p_losses) is held to it here."""
import json

import numpy as np
import pytest
import torch

import bpd_cases as BC
import loss_cases as LC
from util import golden


def product_diffusion(rc):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import gaussian_diffusion as gd, respace as rs
    return LC.make_diffusion(gd, rs, rc)


def restate_vb(d, rc, inp, x_t, dtype):
    """_vb_terms_bpd(clip_denoised=False) per sample through the bound's restatement (tests/bpd_cases.py), one t per row."""
    tab = {k: np.asarray(getattr(d, k), dtype=np.float64) for k in BC.TABLES}
    c = dict(pred=rc["pred"], var=rc["var"], clip=0)
    out = []
    for b, t in enumerate(inp["t"]):
        one = dict(x_start=inp["x_start"][b:b + 1], noise=inp["noise"][b:b + 1], x_t=x_t[b:b + 1], out=inp["out"][b:b + 1], t=int(t))
        out.append(BC.restate(c, one, tab, dtype)["vb"])
    return torch.cat(out)


def restate_case(name, dtype):
    """training_losses of one reference-level case from the restated pieces, in ``dtype``."""
    rc = LC.REF_OP_CASES[name]
    inp = LC.ref_inputs(name)
    d = product_diffusion(rc)
    a, s = LC.rows(dict(sqrt_alphas_cumprod=d.sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod=d.sqrt_one_minus_alphas_cumprod), inp["t"])
    x_start, noise, out = (inp[k].to(dtype) for k in ("x_start", "noise", "out"))
    x_t = LC._b(a, x_start) * x_start + LC._b(s, x_start) * noise
    mse = LC.mean_flat(LC.elementwise("charbonnie", LC.target_of(rc["pred"], x_start, noise, a, s), out[:, :rc["cz"]]))
    vb = restate_vb(d, rc, inp, x_t, dtype) if rc["var"] == "range" or "KL" in rc["loss"] else None
    com = dist = None
    if rc["form"] == "disc":
        fs = [f.to(dtype) for f in inp["feats"]]
        com, dist = LC.restate_pairs(fs[:4]), LC.restate_pairs(fs[4:])
    return LC.combine(rc["loss"], d.num_timesteps, mse, vb, com, dist)


@pytest.mark.parametrize("name", list(LC.REF_OP_CASES))
def test_restatement_against_the_reference(name):
    """Float64 restatement against the reference's float64 run: the same formula (1e-9); fp32 against its fp32 run: within four of
    the gaps the generator measured between the reference's two runs, not below the op bar."""
    g = golden("loss")
    r64, r32 = restate_case(name, torch.float64), restate_case(name, torch.float32)
    assert sorted(r64) == json.loads(str(g[f"ref_{name}_keys"]))
    for k in r64:
        assert tuple(r64[k].shape) == (LC.OP_B,)
        assert LC.rel(r64[k].numpy(), g[f"ref64_{name}_{k}"]) <= 1e-9, (name, k)
        assert LC.rel(r32[k].numpy(), g[f"ref64_{name}_{k}"]) <= max(4 * float(g["gap_" + k]), LC.TOL_OP), (name, k)


def test_fixture_matches_the_case_tables():
    g = golden("loss")
    assert json.loads(str(g["ref_cases"])) == json.loads(json.dumps(LC.REF_OP_CASES))
    assert json.loads(str(g["net_cases"])) == json.loads(json.dumps(LC.NET_CASES))
    for name, nc in LC.NET_CASES.items():
        assert np.array_equal(g[f"net_{name}_t"], LC.net_t(nc)) and len(set(LC.net_t(nc).tolist())) > 1      # mixed t
        want = {"mse", "loss"} | ({"vb"} if nc["var"] == "range" else set()) | ({"com", "dist", "disent"} if nc["form"] == "disc" else set())
        assert set(json.loads(str(g[f"net_{name}_keys"]))) == want


def test_exports_and_struct():
    from diffusion_models_dsdiff_amd import _lib as L
    for name in ("dsd_eval_loss", "dsd_op_loss_rows", "dsd_op_pair_mse_rows", "dsd_op_vlb_terms_rows"):
        assert name in L.EXPORTS
    assert [f[0] for f in L.DsdLoss._fields_] == ["target", "pred", "kind", "learned_range", "t_model", "a", "s", "vlb_coef",
                                                  "post_log_var", "decoder", "terms"]
    assert (L.LOSS_L2, L.LOSS_L1, L.LOSS_CHARBONNIER, L.LOSS_NTERMS) == (0, 1, 2, 4)


def test_training_losses_rejections():
    d = product_diffusion(LC.REF_OP_CASES["disc_eps_fixed_mse"])
    x = torch.zeros(2, 1, 8, 8)
    t = torch.tensor([0, 3])
    model = lambda x, t, **kw: x
    with pytest.raises(NotImplementedError, match="disentangle"):
        d.training_losses(model, x, t, disentangle=object())
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        d.training_losses(model, x, t)
    with pytest.raises(ValueError, match=r"\[B\]"):
        d._loss_rows(torch.zeros(2, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="must lie in"):
        d._loss_rows(torch.tensor([0, d.num_timesteps]))


def test_loss_rows_follow_the_timestep_map():
    """SpacedDiffusion: the network receives timestep_map[t] (rescaled where asked), per sample; a / s / the vb rows come from
    the respaced tables."""
    rc = dict(LC.REF_OP_CASES["disc_x0_range_mse_spaced"], rescale=True)
    d = product_diffusion(rc)
    t = torch.tensor([0, 5, 9])
    tm, a, s, (coef, plv, dec) = d._loss_rows(t)
    want = np.asarray(d.timestep_map, dtype=np.float32)[t.numpy()] * np.float32(1000.0 / d.original_num_steps)
    assert np.array_equal(tm, want) and tm.dtype == np.float32
    assert np.array_equal(a, d.sqrt_alphas_cumprod[t.numpy()].astype(np.float32)) and dec.tolist() == [1, 0, 0]
    assert coef.shape == (3, 8) and np.array_equal(coef[:, 0], a) and np.array_equal(coef[:, 1], s)
    assert np.array_equal(plv, d.posterior_log_variance_clipped[t.numpy()].astype(np.float32))
    assert np.array_equal(coef[:, 7], np.log(d.betas)[t.numpy()].astype(np.float32))          # the learned range's upper end


@pytest.mark.parametrize("par", LC.PREDS)
def test_ldm_loss_weights_and_raises(par):
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DDPM
    m = DDPM(parameterization=par, loss_type="l1", l_simple_weight=0.5, original_elbo_weight=0.25, logvar_init=0.1)
    tab = LC.ldm_tables(par)
    assert torch.equal(m.lvlb_weights, tab["lvlb_weights"]) and bool(torch.isfinite(m.lvlb_weights).all())
    assert "lvlb_weights" not in m.state_dict() and tuple(m.logvar.shape) == (LC.T,) and float(m.logvar[3]) == pytest.approx(0.1)
    assert (m.loss_type, m.l_simple_weight, m.original_elbo_weight, m.learn_logvar) == ("l1", 0.5, 0.25, False)
    x, t = torch.zeros(2, 1, 4, 4), torch.tensor([0, 5])
    v = m.get_v(x + 1, x + 2, t)
    a, s = LC.rows(tab, t.numpy())
    assert torch.equal(v, LC.target_of("v", x + 1, x + 2, a, s))
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        m.get_loss(x, x)
    m.loss_type = "huber"
    with pytest.raises(NotImplementedError, match="unknown loss type"):
        m.get_loss(x, x)


def test_latent_p_losses_refuses_a_learned_logvar():
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    m = LatentDiffusion.__new__(LatentDiffusion)
    m.learn_logvar = True
    with pytest.raises(NotImplementedError, match="learn_logvar"):
        LatentDiffusion.p_losses(m, torch.zeros(1, 1, 4, 4), None, torch.tensor([0]))


@pytest.mark.parametrize("name", list(LC.P_STUB))
def test_restated_p_losses_against_the_reference(name):
    """The float64 restatement of p_losses / get_loss / get_v against the reference's own float64 run (1e-9), and the product's
    lvlb_weights / get_v (host arithmetic) against the reference's fp32 run."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DDPM
    g = golden("loss")
    par, kind = LC.P_STUB[name]
    c, inp = LC.p_stub_inputs(name)
    tab = LC.ldm_tables(par)
    ls = LC.restate_loss(c, inp, torch.float64)
    w = LC.P_WEIGHTS
    _, d = LC.restate_p_losses(ls, inp["t"], tab["lvlb_weights"], w["l_simple_weight"], w["original_elbo_weight"])
    _, d2 = LC.restate_p_losses(ls, inp["t"], tab["lvlb_weights"], w["l_simple_weight"], w["original_elbo_weight"],
                                logvar=torch.full((LC.T,), w["logvar_init"]))
    for k in d:
        assert LC.rel(d[k].numpy(), g[f"p64_{name}_ddpm/{k}"]) <= 1e-9 and LC.rel(d2[k].numpy(), g[f"p64_{name}_ldm/{k}"]) <= 1e-9, k
    assert LC.rel(ls.numpy(), g[f"p64_{name}_get_loss_rows"]) <= 1e-9
    m = DDPM(parameterization=par, loss_type=kind, **w)
    v = m.get_v(inp["x_start"], inp["noise"], torch.from_numpy(inp["t"]))
    assert np.array_equal(v.numpy(), g[f"p_{name}_get_v"])
