"""dsd_op_volume_metrics and dsd_op_kth_double on the device (GPU): every value against the float64 host functions of host_io and
plain numpy (volume_metrics_cases.py; never the code under test).  Bars, the project's own: 1e-12 relative on nrmse, mape, smape,
logac, medsymac, psnr and the auxiliary means and stds, 1e-10 absolute on the ``ssim`` column; n_M and the box exact; the selection
exact (==).  Reordered float64 arithmetic stays within 8.5e-15 relative on such volumes, so the bars leave two decades and still
separate an fp64 kernel from fp32 partial sums; each test prints its measured maximum before it asserts."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import image_metrics_cases as IC
import volume_metrics_cases as VC

pytestmark = pytest.mark.gpu

AUX = tuple(k + d for d in VC.DOMAINS for k in ("mean_t_", "std_t_", "mean_p_", "std_p_"))


def _up(c, dtype):
    t, p = (torch.from_numpy(c[k].copy()).to("cuda", dtype) for k in ("target", "pred"))
    m = None if c["mask"] is None else torch.from_numpy(c["mask"].copy()).cuda()
    return t, p, m


def _rel(got, want):
    return abs(got / want - 1.0) if want != 0 else abs(got)


def _compare(name, dtype, win=0):
    from diffusion_models_dsdiff_amd.metrics import volume_metrics
    c = VC.case(name)
    got = volume_metrics(*_up(c, dtype), win=win)
    err = {k: _rel(got[k], c[k]) for k in VC.COLUMNS + AUX}
    print(f"{name} {dtype}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert got["n_M"] == c["n_M"] and got["lo"] == c["lo"] and got["hi"] == c["hi"], (got["n_M"], got["lo"], got["hi"])
    assert max(err.values()) <= VC.BAR_REL, err
    return c, got


def test_the_cases_are_derived_from_the_kernels_tile():
    from diffusion_models_dsdiff_amd import _lib
    assert (VC.TILE_W, VC.TILE_H) == (_lib.VOLUME_TILE_W, _lib.VOLUME_TILE_H)


@pytest.mark.parametrize("name", VC.NAMES)
def test_every_case_as_fp64(name):
    _compare(name, torch.float64)


@pytest.mark.parametrize("name", VC.FP32_VALUED)
def test_every_fp32_valued_case_as_fp32(name):
    _compare(name, torch.float32)


def test_both_forms_of_the_median_and_the_clipped_rescale():
    """n_M odd (ell) and even (big): the middle element, and half the sum of the two middle ones; clip reaches both ends of s12."""
    assert VC.case("ell")["n_M"] % 2 == 1 and VC.case("big")["n_M"] % 2 == 0
    for name in ("ell", "big", "clip"):
        c, got = _compare(name, torch.float32)
        m = VC.host_io._mask(c["target"], c["mask"])
        ts, ps = VC.host_io.scale12bit(c["target"][m]), VC.host_io.scale12bit(c["pred"][m])
        l = np.sort(np.fabs(np.log(ps / ts)))
        upper = float(np.exp(l[len(l) // 2]) - 1)
        if len(l) % 2 == 0:
            assert _rel(upper, c["medsymac"]) > 1e-9                 # the upper middle element alone is another number
        assert _rel(got["medsymac"], c["medsymac"]) <= VC.BAR_REL


def test_the_exclusive_crop_bound():
    c, got = _compare("lastplane", torch.float32)
    assert got["hi"] == (7, 14, 17)                                    # the largest index with a mask voxel; the crop stops before it


def test_two_calls_agree_bit_for_bit():
    from diffusion_models_dsdiff_amd.metrics import _volume_device
    for name, dtype, win in (("ell", torch.float32, 9), ("f64", torch.float64, 0), ("nomask", torch.float32, 9)):
        t, p, m = _up(VC.case(name), dtype)
        a, b = _volume_device(t, p, m, win), _volume_device(t, p, m, win)
        assert a.tobytes() == b.tobytes(), name


def test_status_words():
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd.metrics import _volume_device, volume_metrics
    S = _lib.VOLUME_SLOTS.index
    c = VC.case("min")
    t, p, m = _up(c, torch.float32)
    # an empty mask: everything but n_M is NaN
    raw = _volume_device(t, p, torch.zeros_like(m), 0)
    assert int(raw[S("status")]) == _lib.VOLUME_EMPTY_MASK and raw[S("n_M")] == 0
    assert all(math.isnan(raw[S(k)]) for k in VC.COLUMNS + AUX)
    with pytest.raises(ValueError, match="the mask is empty"):
        volume_metrics(t, p, torch.zeros_like(m))
    # a mask in one plane: the exclusive bound leaves a crop with a side of 0; the columns over M stand
    one = torch.zeros_like(m)
    one[5, 2:9, 3:11] = True
    raw = _volume_device(t, p, one, 9)
    assert int(raw[S("status")]) == _lib.VOLUME_EMPTY_CROP
    assert math.isnan(raw[S("psnr")]) and math.isnan(raw[S("ssim3d")]) and math.isnan(raw[S("mean_t_Z")])
    want = VC.host_io.nrmse(c["target"], c["pred"], one.cpu().numpy())
    assert _rel(raw[S("nrmse")], want) <= VC.BAR_REL
    assert _rel(raw[S("medsymac")], VC.host_io.medsymac(c["target"], c["pred"], one.cpu().numpy())) <= VC.BAR_REL
    with pytest.raises(ValueError, match="side of 0"):
        volume_metrics(t, p, one)
    # a constant volume: no std, no range
    k = torch.full_like(t, 3.0)
    raw = _volume_device(k, k, m, 0)
    assert int(raw[S("status")]) == _lib.VOLUME_ZERO_STD | _lib.VOLUME_ZERO_RANGE
    assert all(math.isnan(raw[S(x)]) for x in VC.COLUMNS)
    # a constant target under a varying prediction: the range under nrmse is 0 (and with it the target's std)
    raw = _volume_device(k, p, m, 0)
    assert int(raw[S("status")]) & _lib.VOLUME_ZERO_RANGE and math.isnan(raw[S("nrmse")])
    with pytest.raises(ValueError, match="standard deviation of 0|range is 0"):
        volume_metrics(k, p, m)
    # a constant prediction: its std alone is 0; nrmse and psnr stand
    raw = _volume_device(t, k, m, 0)
    assert int(raw[S("status")]) == _lib.VOLUME_ZERO_STD
    assert _rel(raw[S("nrmse")], VC.host_io.nrmse(c["target"], np.full_like(c["pred"], 3.0), c["mask"])) <= VC.BAR_REL
    assert _rel(raw[S("psnr")], VC.host_io.psnr(c["target"], np.full_like(c["pred"], 3.0), c["mask"])) <= VC.BAR_REL


def test_device_refusals_come_from_the_library():
    from diffusion_models_dsdiff_amd import _lib
    x = torch.zeros(4, 5, 6, device="cuda")
    out = torch.zeros(_lib.VOLUME_NOUT, dtype=torch.float64, device="cuda")

    def call(**kw):
        spec = _lib.DsdVolumeMetrics()
        spec.target, spec.pred, spec.out = x.data_ptr(), x.data_ptr(), out.data_ptr()
        spec.D, spec.H, spec.W = 4, 5, 6
        for k, v in kw.items():
            setattr(spec, k, v)
        return _lib.lib().dsd_op_volume_metrics(C.byref(spec), _lib.stream_ptr())

    for kw, text in ((dict(target=None), "target is null"), (dict(pred=None), "pred is null"), (dict(out=None), "out is null"),
                     (dict(D=0), "bad shape"), (dict(D=1 << 14, H=1 << 7, W=(1 << 6) + 1), "up to 2\\^27"), (dict(win=4), "win is 4"),
                     (dict(win=13), "win is 13"), (dict(win=1), "win is 1"), (dict(elem_is_double=2), "elem_is_double is 2")):
        with pytest.raises(_lib.DsdError, match=text):
            _lib.check(call(**kw))
    _lib.check(call())                                                   # and the plain call goes through
    d = torch.zeros(8, dtype=torch.float64, device="cuda")
    for n, k, text in ((0, 0, "n is 0"), (8, 8, "k is 8"), (8, -1, "k is -1")):
        with pytest.raises(_lib.DsdError, match=text):
            _lib.check(_lib.lib().dsd_op_kth_double(d.data_ptr(), n, k, d.data_ptr(), _lib.stream_ptr()))


# ---------------------------------------------------------------------------------------------------------------- metric table
def _row_err(dev, host):
    cols = VC.host_io.METRIC_COLUMNS
    err = {}
    for name, a, b in zip(cols, dev, host):
        if name in ("cc", "lpips", "fid"):
            assert a == 0.0 and b == 0.0 and isinstance(a, float)
        elif name == "mi":
            assert math.isnan(a) and math.isnan(b)
        elif name == "ssim":
            err[name] = abs(a - b)
        else:
            err[name] = _rel(a, b)
    return err


_ROWS = {}


def _table_volume(kind):
    """IC.volume()'s 6 x 190 x 200 pair under its box mask, or a 6 x 240 x 250 one under an ellipsoid whose box is 220 x 218: the
    slices of either crop take the five scales of the MS-SSIM column (a side of 176).  The host row is computed once."""
    if kind not in _ROWS:
        t, p, mask = IC.volume() if kind == "box" else IC.volume(seed=23, H=240, W=250)
        if kind == "ellipsoid":
            mask = VC.ellipsoid(*t.shape, grow=1.15)
            sides = [int(a.max()) - int(a.min()) for a in np.nonzero(mask)]
            assert min(sides[1:]) >= 176 and mask.sum() < 0.8 * mask.size, sides
        _ROWS[kind] = (t, p, mask, VC.host_io.metric_row(t, p, mask))
    return _ROWS[kind]


@pytest.mark.parametrize("kind", ["box", "ellipsoid"])
def test_metric_row_on_the_device(kind):
    t, p, mask, host = _table_volume(kind)
    dev = VC.host_io.metric_row(t, p, mask, device=torch.device("cuda"), table_on_device=True)
    err = _row_err(dev, host)
    print(f"metric_row {kind}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert all(isinstance(v, float) for v in dev) and len(dev) == len(VC.host_io.METRIC_COLUMNS)
    assert err.pop("ssim") <= VC.BAR and max(err.values()) <= VC.BAR_REL
    # device= alone is what it was: the ssim column from the device, the rest the host's bits
    only = VC.host_io.metric_row(t, p, mask, device=torch.device("cuda"))
    col = VC.host_io.METRIC_COLUMNS.index("ssim")
    assert only[col] == VC.host_io.ssim_torch(t, p, mask, device=torch.device("cuda"))
    assert [v for i, v in enumerate(only) if i not in (col, 5)] == [v for i, v in enumerate(host) if i not in (col, 5)]


def test_metric_row_goes_up_as_fp64_when_the_values_are_not_fp32_values():
    """The five volume columns at their bars on a volume no fp32 array holds.  The ssim column is formed from an fp32 cast of Z, as
    host_io.ssim_torch(device=) forms it; on the host that cast alone moves the column of this volume by 1.6e-10 (float64 against
    the fp32-rounded voxels through the same host loop), past the 1e-10 bar, so the column is held to the existing device column,
    which makes the same cast, and its distance from the host loop is printed."""
    t, p, mask, _ = _table_volume("box")
    t, p = t * 0.1, p * 0.1
    assert not VC.host_io._fp32_valued(t)
    host = VC.host_io.metric_row(t, p, mask)
    dev = VC.host_io.metric_row(t, p, mask, device=torch.device("cuda"), table_on_device=True)
    err = _row_err(dev, host)
    print("metric_row fp64 upload: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    ssim_err = err.pop("ssim")
    assert max(err.values()) <= VC.BAR_REL
    same_path = VC.host_io.ssim_torch(t, p, mask, device=torch.device("cuda"))      # the existing device column: the same fp32 cast
    print(f"ssim column: {ssim_err:.2e} from the host loop, {abs(dev[6] - same_path):.2e} from ssim_torch(device=)")
    assert abs(dev[6] - same_path) <= VC.BAR


def test_metric_table_round_trip_through_nifti(tmp_path):
    t, p, mask, _ = _table_volume("box")
    for id_, s in (("a1", 1.0), ("b2", 1.5)):
        os.makedirs(tmp_path / "gt" / id_)
        VC.host_io.write_nifti(str(tmp_path / "gt" / id_ / "ce.nii.gz"), (t * s).astype(np.float32))
        VC.host_io.write_nifti(str(tmp_path / "gt" / id_ / "mask.nii.gz"), mask.astype(np.uint8))
        VC.host_io.write_nifti(str(tmp_path / f"{id_}_x_pred.nii.gz"), (p * s + 3.0).astype(np.float32))
    files = sorted(str(f) for f in tmp_path.glob("*_pred.nii.gz"))
    host = VC.host_io.metric_table(files, str(tmp_path / "gt"), mask_name="mask.nii.gz")
    dev = VC.host_io.metric_table(files, str(tmp_path / "gt"), mask_name="mask.nii.gz", device=torch.device("cuda"), table_on_device=True)
    assert [r[0] for r in dev] == [r[0] for r in host] == [0, "a1", "b2"]
    for h, d in zip(host[1:], dev[1:]):
        err = _row_err(d[1:], h[1:])
        print(f"metric_table {h[0]}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert err.pop("ssim") <= VC.BAR and max(err.values()) <= VC.BAR_REL
    mean = np.mean(np.asarray([r[1:] for r in dev[1:]], dtype=np.float32), axis=0)          # the float32 mean row, as before
    assert all((math.isnan(a) and math.isnan(b)) or a == float(b) for a, b in zip(dev[0][1:], mean))
    VC.host_io.write_metric_csv(str(tmp_path / "m.csv"), dev)
    assert open(tmp_path / "m.csv").readline().strip() == "ids," + ",".join(VC.host_io.METRIC_COLUMNS)


# ------------------------------------------------------------------------------------------------------------------- selection
def _kth(x, k):
    from diffusion_models_dsdiff_amd import _lib
    out = torch.empty(1, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().dsd_op_kth_double(x.data_ptr(), x.numel(), int(k), out.data_ptr(), _lib.stream_ptr()))
    return out.item()


def _kth_inputs(n, seed):
    r = np.random.RandomState(seed)
    top48 = (np.float64(1.2345).view(np.uint64) & ~np.uint64(0xFFFF)) | r.randint(0, 1 << 16, n).astype(np.uint64)
    tail = np.abs(r.randn(n))
    tail[n - n // 3:] = np.inf                                            # as the l array: +inf past the values
    return {"random": r.randn(n) * 10.0 ** r.randint(-8, 8, n), "equal": np.full(n, -2.5), "two": r.choice([-1.0, 3.0], n),
            "top48": top48.view(np.float64), "negatives": -np.abs(r.randn(n)) - 1e-3, "inf_tail": tail}


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65537, 1000003])
def test_kth_double_is_np_sort(n):
    for kind, x in _kth_inputs(n, n % 1000).items():
        want = np.sort(x)
        ks = sorted({0, (n - 1) // 2, n // 2, n - 1})
        if kind == "inf_tail":
            nv = n - n // 3
            ks = sorted({0, (nv - 1) // 2, nv // 2, nv - 1})
        d = torch.from_numpy(x.copy()).cuda()
        for k in ks:
            got = _kth(d, k)
            assert got == want[k], (kind, n, k, got, want[k])
        assert torch.equal(d.cpu(), torch.from_numpy(x))                   # the input is left as it was
