"""metrics.volume_metrics without a GPU: the host path is the seven host_io functions bit for bit, the refusals and the status
words map to ValueError, the ctypes structure follows include/dsdiff.h, and ``table_on_device=False`` changes nothing."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import image_metrics_cases as IC
import volume_metrics_cases as VC
from diffusion_models_dsdiff_amd import _lib, host_io, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsdiff.h")).read(), flags=re.S)


def test_the_cases_hold_what_they_are_chosen_for():
    n = VC.check_cases()
    print("n_M:", n)


@pytest.mark.parametrize("name", ["min", "ell", "nomask", "clip", "f64", "lastplane"])
def test_host_path_equals_the_host_functions_exactly(name):
    c = VC.case(name)
    got = metrics.volume_metrics(c["target"], c["pred"], c["mask"], win=9 if c["ssim3d"] is not None else 0)
    for k in VC.COLUMNS:
        assert got[k] == c[k], (k, got[k], c[k])
    if c["ssim3d"] is not None:
        assert got["ssim3d"] == host_io.ssim(c["target"], c["pred"], c["mask"])
    else:
        assert math.isnan(got["ssim3d"])
    assert got["n_M"] == c["n_M"] and isinstance(got["n_M"], int)
    assert got["lo"] == c["lo"] and got["hi"] == c["hi"]
    for d in VC.DOMAINS:
        for k in ("mean_t_", "std_t_", "mean_p_", "std_p_"):
            assert got[k + d] == c[k + d], k + d
    assert all(isinstance(v, float) for k, v in got.items() if k not in ("n_M", "lo", "hi"))


def test_cpu_tensors_take_the_host_path_and_other_windows_follow_host_io_ssim():
    c = VC.case("ell")
    t, p, m = torch.from_numpy(c["target"].copy()), torch.from_numpy(c["pred"].copy()), torch.from_numpy(c["mask"].copy())
    got = metrics.volume_metrics(t, p, m, win=3)
    assert got["nrmse"] == c["nrmse"] and got["medsymac"] == c["medsymac"] and got["psnr"] == c["psnr"]
    assert got["ssim3d"] == VC.ssim_ref(c["target"], c["pred"], c["mask"], 3)
    assert abs(got["ssim3d"] - c["ssim3d"]) > 1e-3                      # another window is another number
    assert math.isnan(metrics.volume_metrics(t, p, m)["ssim3d"])          # win = 0: skipped


def test_python_side_refusals():
    t = np.zeros((4, 5, 6))
    for bad in (2, 4, 13, 1, -3):
        with pytest.raises(ValueError, match=f"win is {bad}"):
            metrics.volume_metrics(t, t, None, win=bad)
    with pytest.raises(ValueError, match="must be one shape"):
        metrics.volume_metrics(t, np.zeros((4, 5, 7)))
    with pytest.raises(ValueError, match="must be one shape"):
        metrics.volume_metrics(np.zeros((5, 6)), np.zeros((5, 6)))
    with pytest.raises(ValueError, match="mask"):
        metrics.volume_metrics(t, t, np.zeros((4, 5, 5), dtype=bool))
    with pytest.raises(ValueError, match="bad shape"):
        metrics.volume_metrics(np.zeros((0, 5, 6)), np.zeros((0, 5, 6)))
    with pytest.raises(ValueError, match="the mask is empty"):
        metrics.volume_metrics(t, t, np.zeros(t.shape, dtype=bool))
    c = VC.case("min")                                                    # the host's own window check, in its words
    with pytest.raises(ValueError, match="win_size must be odd and not exceed any image side"):
        metrics.volume_metrics(c["target"], c["pred"], c["mask"], win=11)


def test_status_words_become_value_errors(monkeypatch):
    c = VC.case("min")
    want = {_lib.VOLUME_EMPTY_MASK: "mask is empty", _lib.VOLUME_EMPTY_CROP: "side of 0", _lib.VOLUME_ZERO_STD: "standard deviation of 0",
            _lib.VOLUME_ZERO_RANGE: "range is 0", _lib.VOLUME_SMALL_R: "win_size must be odd and not exceed any image side"}
    assert sorted(want) == sorted(b for b, _ in metrics.VOLUME_STATUS) == [1, 2, 4, 8, 16]
    real = metrics._volume_host
    for bit, text in want.items():
        def fake(*a, _bit=bit):
            raw = real(*a)
            raw[_lib.VOLUME_SLOTS.index("status")] = float(_bit)
            return raw
        monkeypatch.setattr(metrics, "_volume_host", fake)
        with pytest.raises(ValueError, match=text):
            metrics.volume_metrics(c["target"], c["pred"], c["mask"])
    monkeypatch.setattr(metrics, "_volume_host", real)
    assert metrics.volume_metrics(c["target"], c["pred"], c["mask"])["nrmse"] == c["nrmse"]


def test_structure_slots_and_status_bits_follow_the_header():
    code = _header()
    body = re.search(r"typedef struct dsd_volume_metrics \{(.*?)\} dsd_volume_metrics;", code, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"(.*?[\s\*])([A-Za-z_][\w, ]*)$", decl).groups()
        for n in names.split(","):
            fields.append((n.strip(), "*" in typ, typ.strip()))
    got = [(n, t) for n, t in _lib.DsdVolumeMetrics._fields_]
    assert [n for n, _ in got] == [n for n, _, _ in fields]
    for (n, ct), (_, ptr, typ) in zip(got, fields):
        if ptr:
            assert C.sizeof(ct) == C.sizeof(C.c_void_p), n
        else:
            assert typ == "int32_t" and ct is C.c_int32, (n, typ)
    assert C.sizeof(_lib.DsdVolumeMetrics) == 7 * 8                       # ptr ptr (int pad) ptr (int int) (int int) ptr
    assert _lib.DsdVolumeMetrics.mask.offset == 24 and _lib.DsdVolumeMetrics.out.offset == 48
    slots = re.search(r"enum \{\s*DSD_VOLUME_NRMSE = 0,(.*?)DSD_VOLUME_NOUT\s*\}", code, flags=re.S).group(1)
    names = ["nrmse"] + [s.strip()[len("DSD_VOLUME_"):].lower() for s in slots.split(",") if s.strip()]
    assert names == [s.lower() for s in _lib.VOLUME_SLOTS] and _lib.VOLUME_NOUT == len(names)
    for name, val in (("EMPTY_MASK", _lib.VOLUME_EMPTY_MASK), ("EMPTY_CROP", _lib.VOLUME_EMPTY_CROP), ("ZERO_STD", _lib.VOLUME_ZERO_STD),
                      ("ZERO_RANGE", _lib.VOLUME_ZERO_RANGE), ("SMALL_R", _lib.VOLUME_SMALL_R), ("TILE_W", _lib.VOLUME_TILE_W),
                      ("TILE_H", _lib.VOLUME_TILE_H), ("MAX_LOG2", _lib.VOLUME_MAX_LOG2)):
        assert int(re.search(r"DSD_VOLUME_%s = (\d+)" % name, code).group(1)) == val, name
    assert (VC.TILE_W, VC.TILE_H) == (_lib.VOLUME_TILE_W, _lib.VOLUME_TILE_H)
    L = _lib.lib()
    assert len(L.dsd_op_volume_metrics.argtypes) == 2 and len(L.dsd_op_kth_double.argtypes) == 5


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, float) and math.isnan(x):
            assert isinstance(y, float) and math.isnan(y)
        else:
            assert x == y and type(x) is type(y), (x, y)


def test_table_on_device_off_is_the_call_without_the_keyword(tmp_path):
    t, p, mask = IC.volume(D=2)
    base = host_io.metric_row(t, p, mask)
    _same(host_io.metric_row(t, p, mask, table_on_device=False), base)
    _same(host_io.metric_row(t, p, mask, device=None, table_on_device=True), base)      # no device: nothing to move
    for id_ in ("a1", "b2"):
        os.makedirs(tmp_path / "gt" / id_)
        s = 1.0 if id_ == "a1" else 1.5
        host_io.write_nifti(str(tmp_path / "gt" / id_ / "ce.nii.gz"), (t * s).astype(np.float32))
        host_io.write_nifti(str(tmp_path / "gt" / id_ / "mask.nii.gz"), mask.astype(np.uint8))
        host_io.write_nifti(str(tmp_path / f"{id_}_x_pred.nii.gz"), (p * s).astype(np.float32))
    files = sorted(str(f) for f in tmp_path.glob("*_pred.nii.gz"))
    base = host_io.metric_table(files, str(tmp_path / "gt"), mask_name="mask.nii.gz")
    again = host_io.metric_table(files, str(tmp_path / "gt"), mask_name="mask.nii.gz", table_on_device=False)
    assert len(base) == 3
    for a, b in zip(base, again):
        _same(a, b)


def test_infer_2d_has_the_switch_and_it_needs_gt_dir():
    from diffusion_models_dsdiff_amd import infer_2d
    with pytest.raises(SystemExit):
        infer_2d.main(["--model-yaml", "m", "--infer-yaml", "i", "--input", "x", "--output", "o", "--metric-table-on-device"])
