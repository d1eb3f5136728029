"""The denoising loss on the MI355X: the kernels of loss.hip against the float64 restatement of tests/loss_cases.py, dsd_eval_loss
against the composition of the exported pieces, and training_losses / p_losses against what the reference recorded
(tests/golden/loss.npz, tests/golden/gen_loss.py).

Bars.  loss_rows and pair_mse_rows are sums of well-conditioned fp32 terms: TOL_OP = 3e-6 against float64, the kernel bar of
tests/test_disc_gpu.py.  vlb_terms_rows: the bar tests/test_bpd_gpu.py holds vlb_terms to, 4x the gap the bound's generator
measured between the reference's fp32 and float64 runs (bpd.npz bar_vb), against float64.  Reference-level and network-level
terms: per term, 4x the largest gap gen_loss.py measured between the reference's own fp32 and float64 runs over the stored
cases, and not below TOL_OP (stub model) / TOL_NET = 5e-6 (networks, the bar of tests/test_disc_gpu.py).  Measured floors:
mse 1.3e-7, com 5.1e-8, dist 9.4e-8, disent 1.5e-7, loss 1.1e-6, vb 4.2e-4 (stub); mse 8.4e-8 ... vb 1.9e-4 (DisC networks) — so
the bars are 3e-6 / 5e-6 for every term but loss (4.6e-6 with the stub) and vb (1.7e-3 stub, 7.6e-4 networks).
DDPM.p_losses / get_loss / get_v and LatentDiffusion.p_losses are held to the reference's own (imported through the stand-in
finder of tests/golden/gen_trace.py): measured floor 1.0e-7 around a stub, so TOL_OP there and TOL_NET on the networks."""
import functools
import json

import numpy as np
import pytest
import torch

import bpd_cases as BC
import loss_cases as LC
from util import fixture_params, golden

pytestmark = pytest.mark.gpu
TOL_NET = 5e-6
PRED = {"eps": 0, "x0": 1, "v": 2}
KIND = {"l2": 0, "l1": 1, "charbonnie": 2}


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def g():
    _lib().require_gpu(0)
    return golden("loss")


def product_diffusion(rc):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import gaussian_diffusion as gd, respace as rs
    return LC.make_diffusion(gd, rs, rc)


def run_loss(c, inp, noise="fed", seed=0, step=0, rows=slice(None)):
    from diffusion_models_dsdiff_amd._sched import loss_rows
    z = inp["noise"][rows].cuda() if noise == "fed" else None
    return loss_rows(PRED[c["pred"]], KIND[c["kind"]], inp["out"][rows].cuda(), inp["x_start"][rows].cuda(), z, inp["a"][rows].cuda(),
                     inp["s"][rows].cuda(), seed, step)


# ---------------------------------------------------------------------------------------------- op grid
@pytest.mark.parametrize("size", LC.SIZES + (LC.BIG["size"],))
def test_loss_rows_against_float64(g, size):
    """Every op case of one sample size (3 channel counts x 3 targets x 3 loss kinds, B = 3 with t = (0, T/2, T-1) in one batch;
    every other case reads the prediction half of an output with a variance half in place): within TOL_OP of float64."""
    worst, n = 0.0, 0
    for c in LC.op_cases():
        if tuple(c["size"]) != tuple(size):
            continue
        n += 1
        inp = LC.op_inputs(c)
        got = run_loss(c, inp)
        assert bool(torch.isfinite(got).all())
        worst = max(worst, LC.rel(got.cpu().numpy(), LC.restate_loss(c, inp, torch.float64).numpy()))
    print(f"{size}: {n} cases, worst relative distance from float64 {worst:.3e} (bar {LC.TOL_OP:g})")
    assert n == (1 if tuple(size) == LC.BIG["size"] else 27) and worst <= LC.TOL_OP


@pytest.mark.parametrize("nf", (2, 3, 4))
def test_pair_mse_rows_against_float64(g, nf):
    from diffusion_models_dsdiff_amd._sched import pair_mse_rows
    fs = LC.pair_inputs(nf)
    got = pair_mse_rows([f.cuda() for f in fs])
    err = LC.rel(got.cpu().numpy(), LC.restate_pairs([f.double() for f in fs]).numpy())
    print(f"pair_mse_rows, {nf} tensors: {err:.3e}")
    assert tuple(got.shape) == (LC.PAIR_SHAPE[0],) and err <= LC.TOL_OP
    assert torch.equal(got, pair_mse_rows([f.cuda() for f in fs]))


def _vlb_case(var, pred, size=(15, 15), cz=2):
    c = next(c for c in BC.op_cases() if tuple(c["size"]) == size and c["cz"] == cz and c["pred"] == pred and c["var"] == var
             and c["clip"] == 0 and c["tn"] == "mid" and c["dist"] == 0.5)
    return c


def _vlb_rows(d, sched, t):
    T = d.num_timesteps
    return sched.coef[T - 1 - t], d.posterior_log_variance_clipped[t].astype(np.float32), (t == 0).astype(np.int32)


@pytest.mark.parametrize("var,pred", [("range", "eps"), ("small", "v"), ("large", "x0")])
def test_vlb_terms_rows_mixed_t_and_shared_t(g, var, pred):
    """Mixed t = (0, mid, last) in one batch: every row within 4 bound bars of the float64 restatement at ITS t.  One shared t:
    the bits of dsd_op_vlb_terms, in the decoder and the KL form."""
    import test_bpd_gpu as TB
    from diffusion_models_dsdiff_amd._sched import vlb_terms, vlb_terms_rows
    gb = golden("bpd")
    bars = {q: float(gb["bar_" + q]) for q in BC.QUANTITIES}
    c = _vlb_case(var, pred)
    d, sched = TB.diffusion(pred, var), TB.sched_of(pred, var, 0)
    tab = {k: np.asarray(getattr(d, k), dtype=np.float64) for k in BC.TABLES}
    T = d.num_timesteps
    t = np.array([0, T // 2, T - 1])
    inp = BC.op_inputs(c, tab)
    a, s = LC.rows(tab, t)
    if pred == "x0":       # row 0 sits at t = 0: the recipe's x_start prediction there (tests/bpd_cases.py op_inputs), same deviation
        inp["out"][0] = inp["x_start"][0] + s[0] * (inp["out"][0] - inp["noise"][0])
    x_t = LC._b(a, inp["x_start"]) * inp["x_start"] + LC._b(s, inp["x_start"]) * inp["noise"]
    coef, plv, dec = _vlb_rows(d, sched, t)
    got = vlb_terms_rows(PRED[pred], var == "range", False, torch.from_numpy(coef.copy()), torch.from_numpy(plv), torch.from_numpy(dec),
                         inp["out"].cuda(), x_t.cuda(), inp["x_start"].cuda(), inp["noise"].cuda())
    for b in range(3):
        one = dict(x_start=inp["x_start"][b:b + 1], noise=inp["noise"][b:b + 1], x_t=x_t[b:b + 1], out=inp["out"][b:b + 1], t=int(t[b]))
        want = BC.restate(c, one, tab, torch.float64)
        for q, v in zip(BC.QUANTITIES, got):
            err = LC.rel(v[b:b + 1].cpu().numpy(), want[q].numpy())
            assert err <= 4 * bars[q], (var, pred, b, q, err)
    for ts in (0, T // 2):
        tt = np.array([ts] * 3)
        a, s = LC.rows(tab, tt)
        xt = (LC._b(a, inp["x_start"]) * inp["x_start"] + LC._b(s, inp["x_start"]) * inp["noise"]).cuda()
        coef, plv, dec = _vlb_rows(d, sched, tt)
        rows = vlb_terms_rows(PRED[pred], var == "range", False, torch.from_numpy(coef.copy()), torch.from_numpy(plv),
                              torch.from_numpy(dec), inp["out"].cuda(), xt, inp["x_start"].cuda(), inp["noise"].cuda())
        res = [torch.empty(3, device="cuda") for _ in range(3)]
        vlb_terms(sched, T - 1 - ts, float(plv[0]), inp["out"].cuda(), xt, inp["x_start"].cuda(), inp["noise"].cuda(), vb=res[0],
                  xstart_mse=res[1], mse=res[2])
        for x, y in zip(rows, res):
            assert torch.equal(x, y), (var, pred, ts)


def test_mixed_t_equals_one_sample_calls(g):
    """A batch with mixed t against three one-sample calls, each at its own t (the v target reads a[b], s[b]): a kernel that read
    row 0's coefficients for every sample would be far off."""
    c = next(c for c in LC.op_cases() if tuple(c["size"]) == (15, 15) and c["cz"] == 2 and c["pred"] == "v" and c["kind"] == "l2")
    inp = LC.op_inputs(c)
    whole = run_loss(c, inp)
    singles = torch.cat([run_loss(c, inp, rows=slice(b, b + 1)) for b in range(LC.OP_B)])
    assert LC.rel(whole.cpu().numpy(), singles.cpu().numpy()) <= LC.TOL_OP
    wrong = dict(inp, a=inp["a"][:1].repeat(3), s=inp["s"][:1].repeat(3))
    assert LC.rel(run_loss(c, wrong).cpu().numpy(), whole.cpu().numpy()) > 1e-2


@pytest.mark.parametrize("pred", LC.PREDS)
def test_two_runs_and_philox_noise(g, pred):
    """Two identical calls agree bit for bit; with no noise fed the target's noise is the one q_sample_rows draws for the same
    seed and step, and another seed moves the eps / v losses only."""
    from diffusion_models_dsdiff_amd._sched import q_sample_rows
    c = next(c for c in LC.op_cases() if tuple(c["size"]) == (24, 40) and c["cz"] == 3 and c["pred"] == pred and c["kind"] == "charbonnie")
    inp = LC.op_inputs(c)
    assert torch.equal(run_loss(c, inp), run_loss(c, inp))
    zero, one = torch.zeros(LC.OP_B, device="cuda"), torch.ones(LC.OP_B, device="cuda")
    z = q_sample_rows(zero, one, torch.zeros_like(inp["x_start"]).cuda(), None, seed=31, step=5)      # 0*0 + 1*z = z
    assert float(z.std()) > 0.9
    fed = run_loss(c, dict(inp, noise=z.cpu()))
    drawn = run_loss(c, inp, noise="philox", seed=31, step=5)
    assert torch.equal(fed, drawn)
    other = run_loss(c, inp, noise="philox", seed=32, step=5)
    assert torch.equal(other, drawn) == (pred == "x0")


# ---------------------------------------------------------------------------------------------- reference level (stub model)
def _check_terms(got, g, prefix, name, floor, gap_prefix=""):
    worst = {}
    for k in json.loads(str(g[f"{prefix}_{name}_keys"])):
        ref = g[f"{prefix}64_{name}_{k}"] if f"{prefix}64_{name}_{k}" in g.files else g[f"{prefix}_{name}_{k}"]
        bar = max(4 * float(g["gap_" + gap_prefix + k]), floor)
        worst[k] = (LC.rel(got[k].cpu().numpy(), ref), bar)
    print(f"{name}: " + ", ".join(f"{k} {e:.2e} (bar {b:.1e})" for k, (e, b) in worst.items()))
    return worst


@pytest.mark.parametrize("name", list(LC.REF_OP_CASES))
def test_training_losses_of_a_foreign_callable_against_the_reference(g, name):
    """Both forms around a stub that returns stored tensors — the path a foreign callable takes: model(x_t, t) itself, then the
    op-level kernels.  Keys, shapes and every term against the reference's float64 run."""
    rc = LC.REF_OP_CASES[name]
    inp = LC.ref_inputs(name)
    d = product_diffusion(rc)
    out, fs = inp["out"].cuda(), [f.cuda() for f in inp["feats"]]
    seen = {}

    def stub(x, t, **kw):
        seen.update(x=tuple(x.shape), t=t.clone(), kw=sorted(kw))
        return tuple(fs) + (out,) if rc["form"] == "disc" else out
    planes = [p.cuda() for p in inp["planes"]]
    kw = dict(t1=planes[0], t2=planes[1], dwi=planes[2]) if rc["form"] == "disc" else dict(F_Data1=planes[0], F_Data2=planes[1], S_Data1=planes[2])
    got = d.training_losses(stub, inp["x_start"].cuda(), torch.from_numpy(inp["t"]).cuda(), model_kwargs=kw, noise=inp["noise"].cuda())
    assert sorted(got) == json.loads(str(g[f"ref_{name}_keys"]))
    assert all(tuple(v.shape) == (LC.OP_B,) and v.dtype == torch.float32 for v in got.values())
    want_t = torch.as_tensor(np.asarray(d.timestep_map)[inp["t"]])
    kl = "KL" in rc["loss"]                               # the KL types call model(x, t, **model_kwargs) as p_mean_variance does
    assert torch.equal(seen["t"].cpu().long(), want_t) and seen["kw"] == (sorted(kw) if kl else [] if rc["form"] == "disc" else ["c_concat"])
    assert seen["x"][1] == (rc["cz"] + 3 if rc["form"] == "disc" else rc["cz"])
    for k, (err, bar) in _check_terms(got, g, "ref", name, LC.TOL_OP).items():
        assert err <= bar, (name, k, err, bar)


# ---------------------------------------------------------------------------------------------- network level
def _native(src, key):
    """(object handed to the diffusion, the native denoiser) of a fixture network: weights of disc.npz / model.npz /
    latent_ldm.npz, of tests/cond_keys_util.py ('cond') or of tests/dit_loops_util.py ('dit')."""
    import cond_keys_util as CU
    import dit_loops_util as DU
    from oracle.synth import synth_params
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DiffusionWrapper
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from diffusion_models_dsdiff_amd.UNet_DS_Diff.model import DSUnetModel
    if src == "dit":
        model = DiffusionWrapper({"target": DU.DIT_TARGET, "params": DU.MODELS[key][0]}, "concat")
        unet = model.diffusion_model
        unet.load_state_dict(DU.weights(key), strict=True)
    elif src == "cond":
        model = unet = UNetModel(**CU.unet_params(key))
        unet.load_state_dict(synth_params([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], CU.WEIGHT_SEED), strict=True)
    else:
        gm = golden(src)
        if src == "disc":
            model = DiffusionWrapper({"target": "Disc_diff.guided_diffusion.unet.SuperResModelNew",
                                      "params": json.loads(str(gm[key + "_cfg"]))}, "concat")
            unet = model.diffusion_model
        elif src == "model":
            model = unet = DSUnetModel(**json.loads(str(gm[key + "_cfg"])))
        else:
            model = unet = UNetModel(**json.loads(str(gm["unet_cfg"])))
        unet.load_state_dict(fixture_params(gm, key), strict=True)
    unet.cuda()
    return model, unet


@functools.lru_cache(maxsize=None)
def net_env(name):
    """(object handed to training_losses, the native denoiser, x_start, planes, noise, t, context or None) of a network case."""
    nc = LC.NET_CASES[name]
    model, unet = _native(nc["src"], nc["key"])
    x_start, planes, z, t = LC.net_inputs(name)
    ctx = LC.net_context(name)
    return model, unet, x_start.cuda(), [p.cuda() for p in planes], z.cuda(), torch.from_numpy(t).cuda(), None if ctx is None else ctx.cuda()


def net_kwargs(nc, planes, ctx=None):
    if nc["form"] == "disc":
        return dict(t1=planes[0], t2=planes[1], dwi=planes[2])
    return dict(c_concat=planes) if ctx is None else dict(c_concat=planes, context=ctx)


@pytest.mark.parametrize("name", list(LC.NET_CASES))
def test_training_losses_on_the_native_networks(g, name):
    """dsd_eval_loss behind training_losses on the DisC net, the four-stream net, the latent UNetModel without and with a
    context (the dsd_set_conditioning route) and the small DiT, mixed t: every term against what the reference's training_losses
    recorded around its own networks; x_start untouched; a second call gives the same bits and allocates nothing."""
    L = _lib()
    nc = LC.NET_CASES[name]
    model, unet, x_start, planes, z, t, ctx = net_env(name)
    d = product_diffusion(nc)
    keep = x_start.clone()
    got = d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes, ctx), noise=z)
    assert torch.equal(x_start, keep)
    assert sorted(got) == json.loads(str(g[f"net_{name}_keys"]))
    assert all(tuple(v.shape) == (nc["B"],) and bool(torch.isfinite(v).all()) for v in got.values())
    before = L.lib().dsd_device_bytes(unet._h)
    again = d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes, ctx), noise=z)
    assert L.lib().dsd_device_bytes(unet._h) == before > 0
    for k in got:
        assert torch.equal(got[k], again[k]), k
    for k, (err, bar) in _check_terms(got, g, "net", name, TOL_NET, "net_").items():
        assert err <= bar, (name, k, err, bar)


@pytest.mark.parametrize("name", list(LC.NET_CASES))
@pytest.mark.parametrize("noise", ("fed", "philox"))
def test_eval_loss_equals_the_composition(g, name, noise):
    """dsd_eval_loss against q_sample_rows + one forward of the same network + dsd_op_loss_rows / dsd_op_vlb_terms_rows /
    dsd_op_pair_mse_rows (a closure hides the native denoiser, so training_losses takes the foreign-callable path): same bits in
    every term, with fed and with Philox noise.  The forward hands UNet_disc_Model's bottleneck tensors out as NCHW; the closure
    lays them out as the workspace holds them (NHWC), so the per-block partial sums cover the same elements and the com / dist
    terms check the workspace offsets the device call reads."""
    nc = LC.NET_CASES[name]
    model, unet, x_start, planes, z, t, ctx = net_env(name)
    d = product_diffusion(nc)
    kw = dict(noise=z) if noise == "fed" else dict(seed=77)

    def closure(x, ts, c_concat=None, **_):
        out = unet(torch.cat([x] + list(c_concat), 1) if c_concat is not None else x, ts, **({} if ctx is None else {"context": ctx}))
        if isinstance(out, tuple) and len(out) == 9:
            out = tuple(f.permute(0, 2, 3, 1).contiguous() for f in out[:8]) + (out[8],)
        return out
    dev = d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes, ctx), **kw)
    comp = d.training_losses(closure, x_start, t, model_kwargs=net_kwargs(nc, planes), **kw)
    assert sorted(dev) == sorted(comp)
    for k in dev:
        assert bool(torch.isfinite(dev[k]).all()) and torch.equal(dev[k], comp[k]), (name, k)


def test_profile_records_of_the_loss_kernels(g):
    """While the handle profiles, dsd_eval_loss adds records of the kinds loss_rows, vlb_terms_rows and pair_mse_rows behind the
    plan's kinds (one call each per evaluation; com and dist are two pair_mse_rows calls); the device bytes count the call's scratch."""
    L = _lib()
    nc = LC.NET_CASES["disc_film"]
    model, unet, x_start, planes, z, t, _ = net_env("disc_film")
    d = product_diffusion(nc)
    plain = d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes), noise=z)
    unet.profile(True)
    try:
        prof = d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes), noise=z)
        rep, runs = unet.profile_report()
    finally:
        unet.profile(False)
    for k in plain:
        assert torch.equal(plain[k], prof[k]), k
    n = x_start.numel() * 4
    assert runs == 1 and rep["loss_rows"]["calls"] == 1 and rep["vlb_terms_rows"]["calls"] == 1 and rep["pair_mse_rows"]["calls"] == 2
    assert rep["loss_rows"]["bytes"] == 3 * n and rep["vlb_terms_rows"]["bytes"] == 5 * n            # v target; learned range
    assert all(rep[k]["ms"] > 0 for k in ("loss_rows", "vlb_terms_rows", "pair_mse_rows")) and "conv" in " ".join(rep)
    assert L.lib().dsd_device_bytes(unet._h) > L.lib().dsd_workspace_bytes(unet._h)


# ---------------------------------------------------------------------------------------------- ldm: p_losses / get_loss / get_v
@pytest.mark.parametrize("name", list(LC.P_STUB))
def test_ddpm_p_losses_of_a_foreign_callable_against_the_reference(g, name):
    """DDPM.p_losses / get_loss / get_v and LatentDiffusion.p_losses around a stub network, mixed t, against the reference's own
    (float64 run): keys under 'val/', every value within max(4 x the reference's fp32-vs-float64 gap, TOL_OP)."""
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import DDPM, LatentDiffusion
    par, kind = LC.P_STUB[name]
    m = DDPM(parameterization=par, loss_type=kind, **LC.P_WEIGHTS)
    c, inp = LC.p_stub_inputs(name)
    t = torch.from_numpy(inp["t"])
    out = inp["out"].cuda()
    m.model = lambda x, ts, **kw: out
    m.model.conditioning_key = None
    bar = max(4 * float(g["gap_p"]), LC.TOL_OP)
    ref = lambda k: g[f"p64_{name}_{k}"]
    loss, d = m.p_losses(inp["x_start"].cuda(), t.cuda(), noise=inp["noise"].cuda())
    assert set(d) == {"val/loss_simple", "val/loss_vlb", "val/loss"} and loss is d["val/loss"] and loss.dim() == 0
    for k in d:
        assert LC.rel(d[k].cpu().numpy(), ref("ddpm/" + k)) <= bar, k
    target = LC.target_of(par, inp["x_start"], inp["noise"], inp["a"], inp["s"])
    assert LC.rel(m.get_loss(out, target.cuda(), mean=True).cpu().numpy(), ref("get_loss_mean")) <= bar
    el = m.get_loss(out, target.cuda(), mean=False)
    assert el.shape == out.shape and LC.rel(el.mean(dim=[1, 2, 3]).cpu().numpy(), ref("get_loss_rows")) <= bar
    v = m.get_v(inp["x_start"].cuda(), inp["noise"].cuda(), t.cuda())
    assert float(np.linalg.norm(v.cpu().numpy() - ref("get_v")) / np.linalg.norm(ref("get_v"))) <= LC.TOL_OP
    lat = LatentDiffusion.__new__(LatentDiffusion)
    lat.__dict__.update(m.__dict__)
    lat.apply_model = lambda x, ts, cond: out
    loss2, d2 = LatentDiffusion.p_losses(lat, inp["x_start"].cuda(), {"c_concat": [out]}, t.cuda(), noise=inp["noise"].cuda())
    for k in d2:
        assert LC.rel(d2[k].cpu().numpy(), ref("ldm/" + k)) <= bar, k


@pytest.mark.parametrize("name", list(LC.P_NET))
def test_latent_p_losses_on_the_native_networks(g, name):
    """LatentDiffusion.p_losses through dsd_eval_loss on the native four-stream, DisC and latent denoisers under every
    conditioning key the loops take ('concat', 'crossattn', 'hybrid', 'adm', 'hybrid-adm', 'crossattn-adm'), mixed t, against
    what the reference's own p_losses recorded around its own networks and DiffusionWrapper.  The module is the project's
    DDPMModel (a DDPM around a DiffusionWrapper: LatentDiffusion without a first stage); the network is reached through
    dsd_eval_loss and never called from Python; Philox noise gives the same bits as the same noise fed."""
    from diffusion_models_dsdiff_amd._sched import q_sample_rows
    from diffusion_models_dsdiff_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from diffusion_models_dsdiff_amd.trainers.trainer_ddpm import DDPMModel
    import cond_keys_util as CU
    pc = LC.P_NET[name]
    _, unet = _native(pc["src"], pc["key"])
    m = DDPMModel(conditioning_key=pc["ckey"], timesteps=1000, parameterization=pc["par"], loss_type=pc["kind"], **LC.P_WEIGHTS)
    wrap = torch.nn.Module()
    wrap.diffusion_model, wrap.conditioning_key = unet, pc["ckey"]
    wrap.forward = None                                   # a call from Python would fail: the native path must not make one
    m.model = wrap
    x_start, cond, z, t = LC.p_net_inputs(name)
    cond = CU.to_cuda(cond)
    loss, d = LatentDiffusion.p_losses(m, x_start.cuda(), cond, t.cuda(), noise=z.cuda())
    assert sorted(d) == json.loads(str(g[f"pnet_{name}_keys"])) and loss is d["val/loss"]
    worst = {k: LC.rel(d[k].cpu().numpy(), g[f"pnet_{name}_{k}"]) for k in d}
    print(f"{name} ({pc['ckey']}): " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f" (bar {TOL_NET:g})")
    assert max(worst.values()) <= TOL_NET, (name, worst)
    drawn = q_sample_rows(torch.zeros(LC.P_B, device="cuda"), torch.ones(LC.P_B, device="cuda"), torch.zeros_like(x_start).cuda(), None,
                          seed=41, step=0)
    a = LatentDiffusion.p_losses(m, x_start.cuda(), cond, t.cuda(), noise=drawn)[1]
    b = LatentDiffusion.p_losses(m, x_start.cuda(), cond, t.cuda(), seed=41)[1]
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_rejections(g):
    from diffusion_models_dsdiff_amd._sched import loss_rows, pair_mse_rows
    L = _lib()
    x = torch.zeros(2, 1, 8, 8, device="cuda")
    with pytest.raises(L.DsdError, match="unknown loss kind"):
        loss_rows(0, 7, x, x, x)
    with pytest.raises(L.DsdError, match="unknown prediction type"):
        loss_rows(5, 0, x, x, x)
    with pytest.raises(L.DsdError, match="rows a and s"):
        loss_rows(2, 0, x, x, x)
    with pytest.raises(L.DsdError, match="2, 3 or 4"):
        pair_mse_rows([x])
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        loss_rows(0, 0, x.cpu(), x.cpu(), x.cpu())
