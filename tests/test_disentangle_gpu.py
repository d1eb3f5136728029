"""The disentanglement losses on the MI355X: the kernels of contrast.hip against the float64 restatement of
tests/disentangle_cases.py, the dsd_set_disentangle rider of dsd_eval_loss against the composition of the exported pieces, and
training_losses(disentangle=) against what the reference recorded (tests/golden/disentangle.npz, tests/golden/gen_disentangle.py).

Bars.  The op forms every dot product and distance in fp64 and follows the reference where it is fp32 (the logits, the mask
denominator, the final divisions): TOL_OP = 3e-6 against float64 — relative on the loss, rel-L2 on the returned matrix — the
kernel bar of tests/test_loss_gpu.py.  Stub level: per entry max(4 x the gap gen_disentangle.py measured between the reference's
fp32 and float64 runs, TOL_OP); the gaps are 0 ... 7.4e-8, so every bar is TOL_OP.  Native network: per entry max(4 x the
change the reference's own result shows when its head tensors move by 5e-6 relative (sens_*, 0 ... 6.0e-7), TOL_NET = 5e-6),
so every bar is TOL_NET.  Near pairs: 1e-5 elementwise; fp64 sums give about 1e-9 there and an fp32 Gram matrix about 1e-1."""
import json

import numpy as np
import pytest
import torch

import disentangle_cases as DC
import loss_cases as LC
from test_loss_gpu import net_env, net_kwargs, product_diffusion
from util import golden

pytestmark = pytest.mark.gpu


def _lib():
    from diffusion_models_dsdiff_amd import _lib as L
    return L


def _sched():
    from diffusion_models_dsdiff_amd import _sched as S
    return S


@pytest.fixture(scope="module")
def g():
    _lib().require_gpu(0)
    return golden("disentangle")


def temperature_of(views):
    return DC.T_CS if views == 6 else DC.T_SAL


def device_views(views, stride=0):
    """Separately allocated device tensors; stride > n: rows of a wider allocation whose padding is NaN."""
    out = []
    for v in views:
        if stride:
            wide = torch.full((v.shape[0], stride), float("nan"), device="cuda")
            wide[:, :v.shape[1]] = v.cuda()
            out.append(wide[:, :v.shape[1]])
        else:
            out.append(v.cuda())
    return out


# ---------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("views,B,n", DC.OP_SHAPES)
def test_contrast_rows_against_float64(g, views, B, n):
    """Every mode and the L1 metric against the float64 restatement (distances formed directly, no Gram matrix).  B = 1: no style
    row has a positive, the 1e-6 of the denominator keeps the loss finite and equal to the restatement's."""
    S = _sched()
    cpu = DC.op_views(views, B, n)
    rows = DC.op_labels(views, B)
    dev = device_views(cpu, n + 3 if (views, B, n) == DC.STRIDED else 0)
    assert len({v.data_ptr() for v in dev}) == views
    for metric in DC.METRICS:
        loss, logits = S.contrast_rows(dev, torch.from_numpy(rows), metric, temperature_of(views))
        want_loss, want_logits = DC.restate(cpu, rows, metric, temperature_of(views), torch.float64)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and tuple(logits.shape) == (views * B, views * B)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(logits).all())
        e_loss, e_map = DC.dist(loss.item(), want_loss.item()), DC.dist(logits.cpu().numpy(), want_logits.numpy())
        print(f"({views}, {B}, {n}) {metric}: loss {loss.item():.6f} err {e_loss:.2e}, matrix rel-L2 {e_map:.2e} (bar {DC.TOL_OP:g})")
        assert e_loss <= DC.TOL_OP and e_map <= DC.TOL_OP, (metric, e_loss, e_map)


def test_near_pairs_keep_their_distance(g):
    """View 1 = view 0 * (1 + 1e-3 N(0, 1)): the squared distance of such a pair is 1e-6 of the squared norms it is the difference
    of in the Gram form.  Values are scaled so the returned 2 d / n - 1 sits near 2 and its relative error is the distance's."""
    S = _sched()
    views, B, n = 6, 3, 256
    cpu = DC.op_views(views, B, n, seed=12900)
    scale = 1.5 * n / 1e-3 / float(cpu[0].norm(dim=1).mean())           # d = 1e-3 |x|, so d / n is about 1.5
    cpu = [v * scale for v in cpu]
    cpu[1] = cpu[0] * (1 + 1e-3 * LC.randn((B, n), 12901))
    _, logits = S.contrast_rows(device_views(cpu), torch.from_numpy(DC.op_labels(views, B)), "eu", 0.1)
    logits = logits.cpu().double()
    worst = 0.0
    for b in range(B):
        d = (cpu[0][b].double() - cpu[1][b].double()).norm()
        want = 2 * (d.float() / n).double() - 1
        assert 0.5 < float(want) < 4, float(want)
        for i, j in ((b, B + b), (B + b, b)):
            worst = max(worst, abs(float(logits[i, j]) - float(want)) / float(want))
    print(f"near pairs: worst relative error of the eu entries {worst:.2e} (bar 1e-5)")
    assert worst <= 1e-5


def test_zero_row_has_cosine_zero(g):
    S = _sched()
    views, B, n = 7, 3, 333
    cpu = DC.op_views(views, B, n)
    cpu[2] = torch.zeros_like(cpu[2])
    rows = DC.op_labels(views, B)
    for metric in ("cl", "eu&cl"):
        loss, logits = S.contrast_rows(device_views(cpu), torch.from_numpy(rows), metric, 0.1)
        zero = logits[2 * B:3 * B]
        assert bool((zero == 0).all()) and bool((logits[:, 2 * B:3 * B] == 0).all()) and bool(torch.isfinite(loss))
        want = DC.restate(cpu, rows, metric, 0.1, torch.float64)[0]
        assert DC.dist(loss.item(), want.item()) <= DC.TOL_OP


def test_two_runs_agree_bit_for_bit(g):
    S = _sched()
    views, B, n = 7, 16, 4099
    dev = device_views(DC.op_views(views, B, n))
    rows = torch.from_numpy(DC.op_labels(views, B))
    for metric in DC.METRICS:
        a, b = S.contrast_rows(dev, rows, metric, 0.1), S.contrast_rows(dev, rows, metric, 0.1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), metric


def test_module_and_method_forms(g):
    """get_disentangle_loss and ContrastiveLoss on a stacked [B, n_views, ...] tensor (views read in place at a row stride of
    n_views * n) against the restatement; the label-free form with its eye mask."""
    from diffusion_models_dsdiff_amd.loss_function.contrastive_loss import ContrastiveLoss
    views, B, n = 6, 3, 256
    cpu = DC.op_views(views, B, n)
    feature = torch.stack(cpu, 1).reshape(B, views, 4, 8, 8).cuda()
    label = torch.from_numpy(DC.cs_labels(B))
    d = product_diffusion(LC.REF_OP_CASES[DC.STUB_CASE])
    for mode in DC.MODES:
        loss, logits, perfect = d.get_disentangle_loss(feature, label, mode, temperature=0.05)
        want = DC.restate(cpu, DC.rows_of(label.numpy()), DC.METRIC_OF[mode], 0.05, torch.float64)
        assert DC.dist(loss.item(), want[0].item()) <= DC.TOL_OP and DC.dist(logits.cpu().numpy(), want[1].numpy()) <= DC.TOL_OP
        assert torch.equal(perfect.cpu(), DC.perfect(DC.rows_of(label.numpy())))
    crit = ContrastiveLoss(contrast_mode="all", contrastive_method="cl")
    loss, logits, perfect = crit(feature, label, temperature=0.05)
    ref = d.get_disentangle_loss(feature, label, "contrast", temperature=0.05)
    assert torch.equal(loss, ref[0]) and torch.equal(logits, ref[1]) and torch.equal(perfect, ref[2])
    one = feature[:, :1]
    loss, logits, perfect = crit(one)                                       # eye mask: no positives, loss -0 / 1e-6 = 0
    want = DC.restate([cpu[0]], np.arange(B), "cl", 0.1, torch.float64)
    assert float(loss) == 0.0 == float(want[0]) and DC.dist(logits.cpu().numpy(), want[1].numpy()) <= DC.TOL_OP
    assert torch.equal(perfect.cpu(), 2 * torch.eye(B) - 1)


# ---------------------------------------------------------------------------------------------- stub level
@pytest.mark.parametrize("mode", DC.MODES)
def test_training_losses_of_a_foreign_callable_against_the_reference(g, mode):
    rc = LC.REF_OP_CASES[DC.STUB_CASE]
    inp = LC.ref_inputs(DC.STUB_CASE)
    d = product_diffusion(rc)
    out = inp["out"].cuda()
    feats = {k: [f.cuda() for f in v] for k, v in DC.stub_feats().items()}
    kw = dict(F_Data1=inp["planes"][0].cuda(), F_Data2=inp["planes"][1].cuda(), S_Data1=inp["planes"][2].cuda())
    got = d.training_losses(lambda x, t, **_: (out, feats), inp["x_start"].cuda(), torch.from_numpy(inp["t"]).cuda(), model_kwargs=kw,
                            noise=inp["noise"].cuda(), disentangle=mode)
    assert got["disen_c_s_loss"].dim() == 0 and got["disen_s_a_l_loss"].dtype == torch.float32 and set(got["contrast_map"]) == set(DC.MAPS)
    flat = DC.flat_terms(got)
    assert sorted(flat) == sorted(str(k) for k in json.loads(str(g[f"stub_{mode}_keys"])))
    for k, v in flat.items():
        err, bar = DC.dist(v, g[f"stub64_{mode}_{k}"]), max(4 * float(g["gap_" + k]), DC.TOL_OP)
        print(f"stub {mode} {k}: {err:.2e} (bar {bar:.1e})")
        assert err <= bar, (mode, k, err, bar)
    plain = d.training_losses(lambda x, t, **_: out, inp["x_start"].cuda(), torch.from_numpy(inp["t"]).cuda(), model_kwargs=kw,
                              noise=inp["noise"].cuda())
    assert sorted(plain) == ["loss", "mse"] and all(torch.equal(plain[k], got[k]) for k in plain)


# ---------------------------------------------------------------------------------------------- native network
def _closure(unet):
    return lambda x, ts, c_concat=None, **_: unet(torch.cat([x] + list(c_concat), 1), ts)


@pytest.mark.parametrize("mode", DC.MODES)
@pytest.mark.parametrize("name", DC.NET_NAMES)
def test_rider_on_the_native_network(g, name, mode):
    """One dsd_eval_loss call with the rider: (a) equal to dsd_op_contrast_rows on the features the same network's forward hands
    out (the workspace holds them NHWC, the forward exports NCHW: another order of the same fp64 sums); (b) against the
    reference's own network and training_losses; (c) mse / vb / loss bit-equal to the call without disentangle; same bits twice."""
    nc = LC.NET_CASES[name]
    model, unet, x_start, planes, z, t, _ = net_env(name)
    d = product_diffusion(nc)
    kw = net_kwargs(nc, planes)
    plain = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z)
    got = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z, disentangle=mode)
    again = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z, disentangle=mode)
    comp = d.training_losses(_closure(unet), x_start, t, model_kwargs=kw, noise=z, disentangle=mode)
    assert set(got) == set(plain) | set(DC.LOSSES) | {"contrast_map"} == set(comp)
    for k in plain:                                                                                              # (c)
        assert torch.equal(plain[k], got[k]), (name, mode, k)
    f_got, f_again, f_comp = DC.flat_terms(got), DC.flat_terms(again), DC.flat_terms(comp)
    for k in DC.LOSSES + DC.MAPS:
        assert np.isfinite(f_got[k]).all() and np.array_equal(f_got[k], f_again[k]), k
        e_comp = DC.dist(f_got[k], f_comp[k])                                                                     # (a)
        e_ref, bar = DC.dist(f_got[k], g[f"net_{name}_{mode}_{k}"]), max(4 * float(g[f"sens_{name}_{mode}_{k}"]), DC.TOL_NET)   # (b)
        print(f"{name} {mode} {k}: rider vs op composition {e_comp:.2e} (bar {DC.TOL_OP:g}), vs reference {e_ref:.2e} (bar {bar:.1e})")
        assert e_comp <= DC.TOL_OP and e_ref <= bar, (name, mode, k, e_comp, e_ref, bar)
    later = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z)         # the rider is gone with its call
    assert set(later) == set(plain) and all(torch.equal(plain[k], later[k]) for k in plain)


@pytest.mark.parametrize("mode", DC.MODES)
def test_rider_on_a_two_channel_input(g, mode):
    """(d) One condition plane (zero al / l planes, the 2-channel branch), with zero-stream sharing asked for: the rider's plan
    switches it off; results equal the op composition on the forward's features, the other terms keep their bits."""
    nc = LC.NET_CASES["ds_tiny"]
    model, unet, x_start, planes, z, t, _ = net_env("ds_tiny")
    d = product_diffusion(nc)
    kw = dict(c_concat=planes[:1])
    unet.share_zero_streams(True)
    try:
        got = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z, disentangle=mode)
    finally:
        unet.share_zero_streams(False)
    plain = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z)
    comp = d.training_losses(_closure(unet), x_start, t, model_kwargs=kw, noise=z, disentangle=mode)
    f_got, f_comp = DC.flat_terms(got), DC.flat_terms(comp)
    for k in plain:
        assert torch.equal(plain[k], got[k]), k
    for k in DC.LOSSES + DC.MAPS:
        err = DC.dist(f_got[k], f_comp[k])
        print(f"2-channel {mode} {k}: {err:.2e} (bar {DC.TOL_OP:g})")
        assert np.isfinite(f_got[k]).all() and err <= DC.TOL_OP, (mode, k, err)


def test_profile_records_carry_the_kernels_name(g):
    nc = LC.NET_CASES["ds_tiny"]
    model, unet, x_start, planes, z, t, _ = net_env("ds_tiny")
    d = product_diffusion(nc)
    plain = d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes), noise=z, disentangle="eu&contrast")
    unet.profile(True)
    try:
        prof = d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes), noise=z, disentangle="eu&contrast")
        rep, runs = unet.profile_report()
    finally:
        unet.profile(False)
    assert all(np.array_equal(a, b) for a, b in zip(DC.flat_terms(plain).values(), DC.flat_terms(prof).values()))
    B, feat = nc["B"], unet(torch.cat([x_start] + planes, 1), t)[1]["style"][0]
    assert runs == 1 and rep["contrast_rows"]["calls"] == 2 and rep["contrast_rows"]["ms"] > 0 and rep["loss_rows"]["calls"] == 1
    assert rep["contrast_rows"]["bytes"] == (6 + 7) * B * (feat.numel() // B) * 4


# ---------------------------------------------------------------------------------------------- rejections
@pytest.mark.parametrize("name", ("disc_tiny", "lat", "dit"))
def test_other_denoisers_are_refused(g, name):
    """UNet_disc_Model, UNetModel and DiT have no such heads: ValueError from training_losses; with a rider installed on their
    handle dsd_eval_loss itself fails, before any device work, and works again once the rider is cleared."""
    L, S = _lib(), _sched()
    nc = LC.NET_CASES[name]
    model, unet, x_start, planes, z, t, ctx = net_env(name)
    d = product_diffusion(nc)
    kw = net_kwargs(nc, planes, ctx)
    with pytest.raises(ValueError, match="heads"):
        d.training_losses(model, x_start, t, model_kwargs=kw, noise=z, disentangle="eu")
    plain = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z)
    with S.disentangle_set(unet, S.Disentangle("eu", nc["B"], x_start.device)):
        with pytest.raises(L.DsdError, match="DSUnetModel"):
            d.training_losses(model, x_start, t, model_kwargs=kw, noise=z)
    later = d.training_losses(model, x_start, t, model_kwargs=kw, noise=z)
    assert all(torch.equal(plain[k], later[k]) for k in plain)


def test_label_rows_must_match_the_batch(g):
    L, S = _lib(), _sched()
    nc = LC.NET_CASES["ds_tiny"]
    model, unet, x_start, planes, z, t, _ = net_env("ds_tiny")
    d = product_diffusion(nc)
    with S.disentangle_set(unet, S.Disentangle("eu", nc["B"] + 1, x_start.device)):
        with pytest.raises(L.DsdError, match="labels"):
            d.training_losses(model, x_start, t, model_kwargs=net_kwargs(nc, planes), noise=z)


def test_bad_arguments(g):
    from diffusion_models_dsdiff_amd.loss_function.contrastive_loss import ContrastiveLoss
    L, S = _lib(), _sched()
    v = [torch.zeros(37, 8, device="cuda") for _ in range(7)]
    with pytest.raises(ValueError, match="259 rows"):
        S.contrast_rows(v, torch.zeros(259), "eu")
    with pytest.raises(ValueError, match="labels"):
        S.contrast_rows(v[:6], torch.zeros(5), "eu")
    with pytest.raises(L.DsdError, match="temperature"):
        S.contrast_rows([x[:2] for x in v[:6]], torch.zeros(12), "cl", temperature=0.0)
    f, lab = torch.zeros(2, 6, 4, device="cuda"), torch.zeros(2, 6, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="infoNCE"):
        ContrastiveLoss(contrastive_method="infoNCE")(f, lab)
    with pytest.raises(NotImplementedError, match="'one'"):
        ContrastiveLoss(contrast_mode="one", contrastive_method="cl")(f, lab)
    d = product_diffusion(LC.REF_OP_CASES[DC.STUB_CASE])
    x, t = torch.zeros(2, 1, 8, 8, device="cuda"), torch.tensor([0, 3], device="cuda")
    with pytest.raises(ValueError, match=r"\(out, dict\)"):
        d.training_losses(lambda x, t, **_: x, x, t, disentangle="eu")
    with pytest.raises(ValueError, match="lacks"):
        d.training_losses(lambda x, t, **_: (x, {"style": []}), x, t, disentangle="eu")
