"""MAE, Gaussian SSIM and MS-SSIM, host side (no GPU): the float64 restatement against MONAI's own formulation and against the
existing MS-SSIM, the accumulators on CPU tensors, every refusal of dsd_op_image_metrics, and the unchanged host metric table.

PARITY UNPINNED: MONAI and torchmetrics are absent; host_io.ssim_gaussian is pinned to the published definition by two
independent formulations (a separable scipy correlation, a grouped torch conv2d with the outer-product kernel)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import image_metrics_cases as IC
from diffusion_models_dsdiff_amd import _lib, host_io
from diffusion_models_dsdiff_amd.metrics import MAEMetric, SSIMMetric, image_metrics


# ---------------------------------------------------------------------------------------- 1. two formulations of one definition
@pytest.mark.parametrize("C_", (1, 2))
@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ssim_gaussian_against_the_conv2d_formulation(size, C_):
    p, t = IC.pair(1, C_, size[0], size[1], seed=31 + size[0] + size[1], kind="noisy")
    p, t = p[0].astype(np.float64), t[0].astype(np.float64)
    a, b = host_io.ssim_gaussian(p, t, data_range=2.0), IC.ssim_conv2d(p, t, 2.0)
    print(f"[-1,1] {size} C={C_}: {a!r} {b!r} diff {abs(a - b):.3e}")
    assert abs(a - b) <= 1e-12
    p12, t12 = host_io.scale12bit(p), host_io.scale12bit(t)                 # the 12-bit form, the sample's own range
    a, b = host_io.ssim_gaussian(p12, t12, data_range=None), IC.ssim_conv2d(p12, t12, None)
    print(f"12-bit {size} C={C_}: {a!r} {b!r} diff {abs(a - b):.3e}")
    assert abs(a - b) <= 1e-12
    assert 0.0 < a < 1.0


@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scale_0_of_the_existing_ms_ssim_is_ssim_gaussian(size):
    """With one beta of 1 multiscale_structural_similarity returns max(mean(full[inner]), 0) of scale 0."""
    p, t = IC.pair(1, 1, size[0], size[1], seed=77 + size[0], kind="noisy")
    p, t = p[0, 0].astype(np.float64), t[0, 0].astype(np.float64)
    for rng, a, b in ((2.0, p, t), (None, host_io.scale12bit(p), host_io.scale12bit(t))):
        old = host_io.multiscale_structural_similarity(a, b, data_range=rng, betas=(1.0,))
        assert old > 0
        assert abs(old - host_io.ssim_gaussian(a, b, data_range=rng)) <= 1e-12
        assert abs(old - host_io.ssim_scale_table(a, b, 1, rng)[0, 0]) <= 1e-12


def test_scale_table_rebuilds_the_existing_ms_ssim():
    for name in ("ms_176", "ms_177x183_12bit", "negative"):
        c = IC.case(name)                                                       # (the case asserts table -> product == the old function)
        assert c["ms_ssim"] is not None and c["scale"].shape == (c["pred"].shape[0], 5, 2)
    neg = IC.case("negative")
    assert neg["scale"][0, 0, 1] < 0 and neg["ms_ssim"][0] == 0.0               # the table is not clamped, the product is


def test_mae():
    p, t = IC.pair(1, 2, 12, 13, seed=5)
    assert host_io.mae(p[0], t[0]) == float(np.mean(np.abs(p[0].astype(np.float64) - t[0].astype(np.float64))))


# ---------------------------------------------------------------------------------------- 2. the module on CPU tensors
def test_image_metrics_host_path_equals_the_references():
    for name in ("win_12x13", "ms_177x183_12bit", "offset_2048"):
        c = IC.case(name)
        out = image_metrics(*IC.tensors(c), scales=c["scales"], data_range=c["data_range"], pre=c["pre"])
        assert out["ssim"].dtype == torch.float64 and tuple(out["cs"].shape) == (c["pred"].shape[0], c["scales"])
        assert np.abs(out["scale"].numpy() - c["scale"]).max() <= 1e-12
        assert np.abs(out["ssim"].numpy() - c["ssim"]).max() <= 1e-12
        assert np.allclose(out["mae"].numpy(), c["mae"], rtol=1e-12, atol=0) and np.allclose(out["mse"].numpy(), c["mse"], rtol=1e-12, atol=0)
        assert np.array_equal(out["elem"].numpy()[:, 2:], c["elem"][:, 2:])
        if c["scales"] == 5:
            assert np.abs(out["ms_ssim"].numpy() - c["ms_ssim"]).max() <= 1e-12
        else:
            assert "ms_ssim" not in out


def test_accumulators_on_cpu_tensors():
    c1, c2 = IC.case("tile_plus1"), IC.case("win_11x37")                        # two unequal batches: 3 and 1 samples
    mae, ssim = MAEMetric(reduction="mean"), SSIMMetric(spatial_dims=2, data_range=2.0)
    (p1, t1), (p2, t2) = IC.tensors(c1), IC.tensors(c2)
    v_tensor = ssim(y_pred=p1, y=t1)
    ssim.reset()
    v_list, m_list = ssim(y_pred=list(p1), y=list(t1)), mae(y_pred=list(p1), y=list(t1))
    assert tuple(v_list.shape) == (3, 1) and torch.equal(v_list, v_tensor)
    assert np.abs(v_list.numpy()[:, 0] - c1["ssim"]).max() <= 1e-12
    assert np.allclose(m_list.numpy()[:, 0], c1["mae"], rtol=1e-12, atol=0)
    ssim(y_pred=p2, y=t2)
    mae(y_pred=p2, y=t2)
    assert ssim.aggregate().dim() == 0
    assert abs(ssim.aggregate().item() - np.concatenate([c1["ssim"], c2["ssim"]]).mean()) <= 1e-12
    assert abs(mae.aggregate().item() - np.concatenate([c1["mae"], c2["mae"]]).mean()) <= 1e-14
    ssim.reset()
    mae.reset()
    with pytest.raises(ValueError, match="nothing to average"):
        ssim.aggregate()
    ssim(y_pred=p2, y=t2)
    assert abs(ssim.aggregate().item() - c2["ssim"].mean()) <= 1e-12              # nothing of the first epoch is left


@pytest.mark.parametrize("kw, text", [
    (dict(spatial_dims=3), "spatial_dims"), (dict(win_size=7), "win_size"), (dict(kernel_sigma=1.0), "kernel_sigma"),
    (dict(kernel_type="uniform"), "kernel_type"), (dict(reduction="sum"), "reduction"), (dict(k1=0.02), "k1")])
def test_ssim_metric_names_what_it_does_not_support(kw, text):
    with pytest.raises(ValueError, match=text) as e:
        SSIMMetric(**kw)
    assert "'win_size': 11" in str(e.value) and "'spatial_dims': 2" in str(e.value)


def test_mae_metric_names_what_it_does_not_support():
    with pytest.raises(ValueError, match="reduction='mean'"):
        MAEMetric(reduction="sum")
    with pytest.raises(ValueError, match="data_range"):
        SSIMMetric(data_range=0.0)


# ---------------------------------------------------------------------------------------- 3. the C ABI's refusals
def _spec(**kw):
    s = _lib.DsdImageMetrics()
    s.pred, s.target, s.scale_out, s.elem_out = 4096, 4096, 4096, 4096          # never dereferenced: every case is refused first
    s.B, s.C, s.H, s.W, s.scales, s.data_range = 2, 1, 32, 32, 1, 1.0
    keep = []
    for k, v in kw.items():
        if k == "pre":
            v = (C.c_double * 7)(*v)
            keep.append(v)
        setattr(s, k, v)
    return s, keep


REFUSALS = [
    (dict(pred=None), "pred is null"), (dict(target=None), "target is null"), (dict(scale_out=None), "scale_out is null"),
    (dict(elem_out=None), "elem_out is null"),
    (dict(scales=0), "scales is 0; 1 to 5"), (dict(scales=6, H=512, W=512), "scales is 6; 1 to 5"),
    (dict(scales=5, H=175, W=300), "scale 5 of a 175 x 300 image has a side of 10; the 11-tap window needs 11"),
    (dict(H=10, W=64), "scale 1 of a 10 x 64 image has a side of 10"),
    (dict(B=65536), "B is 65536; up to 65535"),
    (dict(C=1025, H=1024, W=1024), "C*H*W = 1074790400 elements; up to 2^30"),
    (dict(data_range=-1.0), "data_range is -1;"), (dict(data_range=float("nan")), "data_range is nan;"),
    (dict(data_range=float("inf")), "data_range is inf;"),
    (dict(pre=(0., 0., 0., 1., 0., 0., 1.)), "divides the prediction by div = 0"),
    (dict(pre=(0., 1., 0., 0., 0., 0., 1.)), "divides the target by div = 0"),
    (dict(pre=(0., 1., 0., 1., 0., 2., 1.)), "lo = 2 above hi = 1"),
]


@pytest.mark.parametrize("kw, text", REFUSALS, ids=[t[:24] for _, t in REFUSALS])
def test_c_abi_refusals_name_the_value(kw, text):
    L = _lib.lib()
    spec, _keep = _spec(**kw)
    assert L.dsd_op_image_metrics(C.byref(spec), None) != 0
    msg = L.dsd_last_error().decode()
    assert msg.startswith("image_metrics: ") and text in msg, msg


def test_c_abi_refuses_a_null_spec_and_the_binding_matches_the_header():
    L = _lib.lib()
    assert L.dsd_op_image_metrics(None, None) != 0 and "spec is null" in L.dsd_last_error().decode()
    assert C.sizeof(_lib.DsdImageMetrics) == 72 and _lib.DsdImageMetrics.data_range.offset == 40
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsdiff.h")).read()
    assert f"DSD_METRICS_TILE_W = {_lib.METRICS_TILE_W}, DSD_METRICS_TILE_H = {_lib.METRICS_TILE_H}" in hdr
    assert (IC.TILE_W, IC.TILE_H) == (_lib.METRICS_TILE_W, _lib.METRICS_TILE_H)


def test_host_path_refuses_what_the_library_refuses():
    x = torch.zeros(1, 1, 32, 32)
    for kw, text in ((dict(scales=6), "scales is 6"), (dict(scales=3), "has a side of 8"), (dict(data_range=-2.0), "data_range is -2"),
                     (dict(pre=(0, 0, 0, 1, 0, 0, 1)), "div = 0"), (dict(pre=(0, 1, 0, 1, 0, 2, 1)), "lo = 2")):
        with pytest.raises(ValueError, match=text):
            image_metrics(x, x, **kw)
    with pytest.raises(ValueError, match="one shape"):
        image_metrics(x, x[0])


# ---------------------------------------------------------------------------------------- 4. the keyword unset
def test_metric_table_without_a_device_is_the_untouched_formula(tmp_path):
    t, p, mask = IC.volume(D=3)
    m = mask.astype(bool)
    tt, pp = np.where(m, t, 0), np.where(m, p, 0)
    nz = np.nonzero(m)
    sl = tuple(slice(int(a.min()), int(a.max())) for a in nz)
    tt, pp = host_io.scale12bit(tt[sl]), host_io.scale12bit(pp[sl])
    direct = float(np.mean([host_io.multiscale_structural_similarity(pp[i], tt[i]) for i in range(tt.shape[0])]))
    assert host_io.ssim_torch(t, p, mask) == direct
    assert host_io.ssim_torch(t, p, mask, device=None) == direct
    col = host_io.METRIC_COLUMNS.index("ssim")
    assert host_io.metric_row(t, p, mask)[col] == direct
    os.makedirs(tmp_path / "gt" / "a1")
    host_io.write_nifti(str(tmp_path / "gt" / "a1" / "ce.nii.gz"), t.astype(np.float32))
    host_io.write_nifti(str(tmp_path / "gt" / "a1" / "mask.nii.gz"), mask.astype(np.uint8))
    host_io.write_nifti(str(tmp_path / "a1_x_pred.nii.gz"), p.astype(np.float32))
    table = host_io.metric_table([str(tmp_path / "a1_x_pred.nii.gz")], str(tmp_path / "gt"), mask_name="mask.nii.gz")
    assert table[1][0] == "a1" and table[1][1 + col] == direct
    again = host_io.metric_table([str(tmp_path / "a1_x_pred.nii.gz")], str(tmp_path / "gt"), mask_name="mask.nii.gz", device=None)
    assert np.array_equal(np.asarray(table[1][1:]), np.asarray(again[1][1:]), equal_nan=True)
