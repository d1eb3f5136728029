"""infer_2d --metric-table-on-device (GPU): the CSV the entry point writes with every number column evaluated on the device equals,
within the bars of the volume-metric tests, the table the float64 host functions give for the volumes it wrote."""
import csv
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import volume_metrics_cases as VC
from util import golden, fixture_params, cond_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_infer_2d_metric_table_on_device(tmp_path):
    """One id, three 192 x 192 slices (the MS-SSIM column needs a side of 176), a mask file; 2 DDIM steps of the tiny network."""
    from diffusion_models_dsdiff_amd import host_io
    gm = golden("model")
    params = json.loads(str(gm["tiny_cfg"]))
    model_yaml = {"model": {"params": {"parameterization": "v", "diffusion_steps": 1000, "noise_schedule": "linear",
                                       "unet_config": {"target": "UNet_DS_Diff.model.DSUnetModel", "params": params}}}}
    infer_yaml = {"cuda_idx": 0, "test_batch_size": 3, "seed": 11, "sampler_setting": {"sampler": "ddim", "sample_steps": 2, "ddim_eta": 0}}
    (tmp_path / "m.yaml").write_text(yaml.safe_dump(model_yaml))
    (tmp_path / "i.yaml").write_text(yaml.safe_dump(infer_yaml))
    torch.save(fixture_params(gm, "tiny"), tmp_path / "ckpt.pt")
    S, D = 192, 3
    cond = cond_image((D, 1, S, S), 78).numpy()
    os.makedirs(tmp_path / "h5" / "p01")
    os.makedirs(tmp_path / "gt" / "p01")
    for z in range(D):
        host_io.write_h5(str(tmp_path / "h5" / "p01" / f"t1_{z}.h5"), {"F_Data1": cond[z, 0]})
    gt = np.random.default_rng(5).uniform(-1, 1, (D, S, S)).astype(np.float32)
    mask = np.zeros((D, S, S), dtype=np.uint8)
    mask[:, 3:190, 5:188] = 1
    host_io.write_nifti(str(tmp_path / "gt" / "p01" / "ce.nii.gz"), gt)
    host_io.write_nifti(str(tmp_path / "gt" / "p01" / "mask.nii.gz"), mask)
    r = subprocess.run([sys.executable, "-m", "diffusion_models_dsdiff_amd.infer_2d", "--model-yaml", str(tmp_path / "m.yaml"),
                        "--infer-yaml", str(tmp_path / "i.yaml"), "--ckpt", str(tmp_path / "ckpt.pt"), "--input", str(tmp_path / "h5"),
                        "--input-keys", "F_Data1", "--output", str(tmp_path / "pred"), "--gt-dir", str(tmp_path / "gt"),
                        "--mask-name", "mask.nii.gz", "--metric-table-on-device"],
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = list(csv.reader(open(str(tmp_path / "pred") + "_metric.csv")))
    assert rows[0] == ["ids"] + host_io.METRIC_COLUMNS and [x[0] for x in rows[1:]] == ["0", "p01"]
    host = host_io.metric_table({"p01": str(tmp_path / "pred" / "p01" / "pred.nii.gz")}, str(tmp_path / "gt"), mask_name="mask.nii.gz")
    worst = {}
    for got, want in zip(rows[1:], host):
        for name, a, b in zip(host_io.METRIC_COLUMNS, got[1:], want[1:]):
            a = float(a)
            if name == "mi":
                assert math.isnan(a) and math.isnan(b)
            elif name in ("cc", "lpips", "fid"):
                assert a == 0.0 and b == 0.0
            elif got[0] == "0":                                            # the mean row is a float32 mean: one float32 ulp
                assert abs(a / b - 1) <= 2.0 ** -23, (name, a, b)
            elif name == "ssim":
                worst[name] = max(worst.get(name, 0.0), abs(a - b))
            else:
                worst[name] = max(worst.get(name, 0.0), abs(a / b - 1))
    print("infer_2d --metric-table-on-device against the host table: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst.pop("ssim") <= VC.BAR and max(worst.values()) <= VC.BAR_REL
