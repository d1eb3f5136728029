"""The disentanglement losses without a GPU: the torch restatement of tests/disentangle_cases.py against what the reference's own
training_losses(disentangle=) recorded (tests/golden/disentangle.npz, tests/golden/gen_disentangle.py), the label builders, the
exports and every rejection that happens before device work."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import disentangle_cases as DC
import loss_cases as LC
from util import golden


def product_diffusion(rc):
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion import gaussian_diffusion as gd, respace as rs
    return LC.make_diffusion(gd, rs, rc)


@pytest.mark.parametrize("mode", DC.MODES)
def test_restatement_against_the_reference(mode):
    """Float64 restatement against the reference's run on float64 tensors: the same formula (1e-9).  fp32 restatement against the
    same: within four of the gaps the generator measured between the reference's two runs, not below the op bar."""
    g = golden("disentangle")
    r64 = DC.flat_terms(DC.restate_terms(DC.stub_feats(torch.float64), mode, torch.float64))
    r32 = DC.flat_terms(DC.restate_terms(DC.stub_feats(torch.float32), mode, torch.float32))
    assert set(r64) | {"mse", "loss"} == set(json.loads(str(g[f"stub_{mode}_keys"])))
    for k in r64:
        want = g[f"stub64_{mode}_{k}"]
        e64, e32, bar = DC.dist(r64[k], want), DC.dist(r32[k], want), max(4 * float(g["gap_" + k]), DC.TOL_OP)
        print(f"{mode} {k}: float64 {e64:.2e} (bar 1e-9), fp32 {e32:.2e} (bar {bar:.1e})")
        assert e64 <= 1e-9 and e32 <= bar, (mode, k, e64, e32, bar)


def test_label_builders_equal_the_reference():
    from diffusion_models_dsdiff_amd import _sched as S
    g = golden("disentangle")
    cs, sal = S.disentangle_labels(LC.OP_B)
    assert np.array_equal(cs.numpy(), g["stub_labels_cs"]) and np.array_equal(sal.numpy(), g["stub_labels_sal"])
    assert np.array_equal(DC.cs_labels(LC.OP_B), g["stub_labels_cs"]) and np.array_equal(DC.sal_labels(LC.OP_B), g["stub_labels_sal"])
    assert cs.dtype == torch.int64 and tuple(cs.shape) == (LC.OP_B, 6) and tuple(sal.shape) == (LC.OP_B, 7)
    assert np.array_equal(S.label_rows(cs).numpy(), DC.rows_of(g["stub_labels_cs"]))
    assert S.label_rows(cs).tolist()[:4] == [0, 1, 2, 0] and S.label_rows(sal).tolist()[-3:] == [1, 3, 5]
    for rows in (S.label_rows(cs), S.label_rows(sal)):
        assert torch.equal(S.perfect_logit(rows), DC.perfect(rows.numpy()))
    for mode in DC.MODES:      # the stored perfect_logit matrices are those of the stored labels
        assert np.array_equal(g[f"stub32_{mode}_perfect_c_s_heatmap"], DC.perfect(DC.rows_of(g["stub_labels_cs"])).numpy())
        assert np.array_equal(g[f"stub32_{mode}_perfect_s_a_l_heatmap"], DC.perfect(DC.rows_of(g["stub_labels_sal"])).numpy())
    one = S.disentangle_labels(1)
    assert one[0].tolist() == [[0, 0, 0, -1, -2, -3]] and one[1].tolist() == [[-1, -2, -3, 0, 0, 1, 1]]


def test_fixture_matches_the_case_tables():
    g = golden("disentangle")
    assert tuple(json.loads(str(g["modes"]))) == DC.MODES and tuple(json.loads(str(g["net_names"]))) == DC.NET_NAMES
    for name in DC.NET_NAMES:
        B = LC.NET_CASES[name]["B"]
        for mode in DC.MODES:
            assert tuple(g[f"net_{name}_{mode}_c_s_heatmap"].shape) == (6 * B, 6 * B)
            assert tuple(g[f"net_{name}_{mode}_s_a_l_heatmap"].shape) == (7 * B, 7 * B)
            for k in DC.LOSSES + DC.MAPS:
                assert float(g[f"sens_{name}_{mode}_{k}"]) < 1e-4      # a bar of 4 * sens stays a check


def test_exports_and_struct():
    from diffusion_models_dsdiff_amd import _lib as L
    for name in ("dsd_set_disentangle", "dsd_op_contrast_rows"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert [f[0] for f in L.DsdDisentangle._fields_] == ["mode", "temperature_cs", "temperature_sal", "labels_cs", "n_labels_cs",
                                                         "labels_sal", "n_labels_sal", "loss", "logits_cs", "logits_sal"]
    assert (L.CONTRAST_CL, L.CONTRAST_EU, L.CONTRAST_EU_CL, L.CONTRAST_L1) == (0, 1, 2, 3)
    assert L.CONTRAST_MAX_ROWS >= 7 * 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsdiff.h")).read()
    assert f"DSD_CONTRAST_MAX_ROWS = {L.CONTRAST_MAX_ROWS}" in header and f"DSD_CONTRAST_MAX_VIEWS = {L.CONTRAST_MAX_VIEWS}" in header


def _op(views, n_views, B, n, stride, labels, mode, temperature, loss, logits):
    from diffusion_models_dsdiff_amd import _lib as L
    arr = (C.c_void_p * max(n_views, 1))(*([views] * max(n_views, 1))) if views is not None else None
    return L.lib().dsd_op_contrast_rows(arr, n_views, B, n, stride, labels, mode, C.c_float(temperature), loss, logits, None)


def test_op_rejections_before_device_work():
    """Every argument dsd_op_contrast_rows refuses is refused before anything touches a device: the pointers here point nowhere."""
    from diffusion_models_dsdiff_amd import _lib as L
    p = C.c_void_p(0x1000)
    err = lambda: L.lib().dsd_last_error().decode()
    assert _op(None, 6, 2, 16, 0, p, 0, 0.1, p, p) != 0 and "null" in err()
    assert _op(0x1000, 6, 2, 16, 0, None, 0, 0.1, p, p) != 0 and "null" in err()
    assert _op(0x1000, 6, 2, 16, 0, p, 0, 0.1, None, p) != 0 and "null" in err()
    assert _op(0x1000, 6, 2, 16, 0, p, 0, 0.1, p, None) != 0 and "null" in err()
    assert _op(None, 6, 2, 16, 0, p, 0, 0.1, p, p) != 0
    assert _op(0x1000, 6, 2, 16, 0, p, 4, 0.1, p, p) != 0 and "mode" in err()
    assert _op(0x1000, 6, 2, 16, 0, p, -1, 0.1, p, p) != 0 and "mode" in err()
    for mode in (L.CONTRAST_CL, L.CONTRAST_EU_CL):
        assert _op(0x1000, 6, 2, 16, 0, p, mode, 0.0, p, p) != 0 and "temperature" in err()
        assert _op(0x1000, 6, 2, 16, 0, p, mode, -0.1, p, p) != 0 and "temperature" in err()
    assert _op(0x1000, 7, 37, 16, 0, p, 1, 0.1, p, p) != 0 and "rows" in err()          # 259 rows
    assert _op(0x1000, 8, L.CONTRAST_MAX_ROWS // 8 + 1, 16, 0, p, 1, 0.1, p, p) != 0 and "rows" in err()
    assert _op(0x1000, 9, 2, 16, 0, p, 1, 0.1, p, p) != 0 and "views" in err()
    assert _op(0x1000, 6, 2, 16, 15, p, 1, 0.1, p, p) != 0 and "row_stride" in err()
    assert _op(0x1000, 6, 2, 0, 0, p, 1, 0.1, p, p) != 0
    assert _op(0x1000, 1, 1, 16, 0, p, 1, 0.1, p, p) != 0 and "rows" in err()           # a single row has no pair


def test_python_rejections():
    from diffusion_models_dsdiff_amd import _sched as S
    from diffusion_models_dsdiff_amd.loss_function.contrastive_loss import ContrastiveLoss
    d = product_diffusion(LC.REF_OP_CASES[DC.STUB_CASE])
    x, t = torch.zeros(2, 1, 8, 8), torch.tensor([0, 3])
    model = lambda x, t, **kw: x
    for bad in (object(), "l1", "cosine", True):
        with pytest.raises(NotImplementedError, match="disentangle"):
            d.training_losses(model, x, t, disentangle=bad)
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):       # a known mode passes that check and reaches the next
        d.training_losses(model, x, t, disentangle="eu")
    with pytest.raises(NotImplementedError, match="not supported"):
        d.get_disentangle_loss(torch.zeros(2, 6, 4), torch.zeros(2, 6, dtype=torch.long), contrast="cosine")
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        d.get_disentangle_loss(torch.zeros(2, 6, 4), torch.zeros(2, 6, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="not supported"):
        S.contrast_rows([torch.zeros(2, 4)] * 6, torch.zeros(12), metric="l2")
    with pytest.raises(ValueError, match="lacks"):
        S.head_views({"style": [], "content": []})
    f, lab = torch.zeros(2, 6, 4), torch.zeros(2, 6, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="infoNCE"):
        ContrastiveLoss(contrastive_method="infoNCE")(f, lab)
    with pytest.raises(NotImplementedError, match="'one'"):
        ContrastiveLoss(contrast_mode="one", contrastive_method="cl")(f, lab)
    with pytest.raises(NotImplementedError, match="mask"):
        ContrastiveLoss(contrastive_method="cl")(f, mask=torch.eye(2))
    with pytest.raises(ValueError, match="Cannot define both"):
        ContrastiveLoss(contrastive_method="cl")(f, lab, torch.eye(2))
    with pytest.raises(ValueError, match="Unknown contrastive method"):      # the reference's own end of forward with 'simclr'
        ContrastiveLoss()(f[:, :1])
    with pytest.raises(ValueError, match="Unknown mode"):
        ContrastiveLoss(contrast_mode="some", contrastive_method="cl")(f, lab)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        ContrastiveLoss(contrastive_method="cl")(torch.zeros(2, 6), lab)
    with pytest.raises(ValueError, match="Num of labels"):
        ContrastiveLoss(contrastive_method="cl")(f, lab[:1])
    with pytest.raises(RuntimeError, match="runs on the MI355X only"):
        ContrastiveLoss(contrastive_method="cl")(f, lab)
    with pytest.raises(NotImplementedError, match="disentangle"):
        S.Disentangle("l1", 2, "cpu")
