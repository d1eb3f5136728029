#!/usr/bin/env python3
"""Generate tests/golden/disentangle.npz by importing the REFERENCE on CPU (build container only).

    DSD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_disentangle.py

The reference's own GaussianDiffusion.training_losses(disentangle=m) (training_project/utils/gaussian_diffusion.py:907-975 with
get_disentangle_loss :1056-1094 and loss_function/contrastive_loss.py) for m in 'contrast', 'eu', 'eu&contrast', imported the
way gen_loss.py imports it.  get_heatmap (training_project/utils/util.py:144-155: min-max normalisation, viridis, uint8) is
replaced by the identity, so the four matrices are stored raw.

  stub    a stub model that returns stored tensors (the output of the loss case STUB_CASE and the head lists of
          tests/disentangle_cases.py stub_feats), once as fp32 and once called on float64 tensors; the labels the reference handed
          to get_disentangle_loss; the gap between the two runs per entry (gap_*).
  net     the reference's own DSUnetModel with the `tiny` / `tinyfilm` weights of model.npz (the ds_tiny / ds_tinyfilm cases of
          tests/loss_cases.py), fp32, every mode; and per entry the change of the result when the network's own head tensors
          are perturbed by Gaussian noise of relative size NET_NOISE (sens_*): 1 / temperature amplifies feature error.

Stored: results only.  Inputs regenerate from seeds (tests/disentangle_cases.py, tests/loss_cases.py).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ["DSD_REFERENCE"])
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import disentangle_cases as DC  # noqa: E402
import loss_cases as LC  # noqa: E402
from gen_cfg import _params  # noqa: E402
import gen_trace as GT  # noqa: E402

GT.ABSENT = tuple(m for m in GT.ABSENT if m != "training_project")
sys.meta_path.insert(0, GT._Finder())

torch.set_grad_enabled(False)
torch.set_num_threads(8)

import training_project.utils.gaussian_diffusion as gd  # noqa: E402
import training_project.utils.respace as rs  # noqa: E402

gd.get_heatmap = lambda m: m


def run_ref(rc, model, x_start, noise, t, planes, mode, dtype, labels=None):
    d = LC.make_diffusion(gd, rs, rc)
    if labels is not None:
        inner = d.get_disentangle_loss

        def spy(feature, label, *a, **kw):
            labels.append(label.numpy().copy())
            return inner(feature, label, *a, **kw)
        d.get_disentangle_loss = spy
    kw = dict(F_Data1=planes[0].to(dtype), F_Data2=planes[1].to(dtype), S_Data1=planes[2].to(dtype))
    terms = d.training_losses(model, x_start.to(dtype), torch.from_numpy(t), model_kwargs=kw, noise=noise.to(dtype), disentangle=mode)
    return DC.flat_terms(terms)


def gen_stub(out):
    rc = LC.REF_OP_CASES[DC.STUB_CASE]
    inp = LC.ref_inputs(DC.STUB_CASE)
    gaps = {}
    for mode in DC.MODES:
        res, labels = {}, []
        for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
            o, feats = inp["out"].to(dtype), DC.stub_feats(dtype)
            res[tag] = run_ref(rc, lambda x, ts, **kw: (o, feats), inp["x_start"], inp["noise"], inp["t"], inp["planes"], mode, dtype,
                               labels if tag == "32" else None)
        for k in res["32"]:
            out[f"stub32_{mode}_{k}"] = res["32"][k].astype(np.float32)
            out[f"stub64_{mode}_{k}"] = res["64"][k]
            gaps.setdefault(k, []).append(DC.dist(res["32"][k], res["64"][k]))
        out[f"stub_{mode}_keys"] = json.dumps(sorted(res["32"]))
        out["stub_labels_cs"], out["stub_labels_sal"] = labels
        print(f"stub {mode}: " + ", ".join(f"{k} {DC.dist(res['32'][k], res['64'][k]):.1e}" for k in sorted(res["32"])))
    for k, v in gaps.items():
        out["gap_" + k] = np.float64(max(v))
        print(f"largest fp32-vs-float64 gap of the reference, {k}: {max(v):.3e}")


def gen_net(out):
    from UNet_DS_Diff.model import DSUnetModel
    g = np.load(os.path.join(HERE, "model.npz"), allow_pickle=False)
    for name in DC.NET_NAMES:
        nc = LC.NET_CASES[name]
        m = DSUnetModel(**json.loads(str(g[nc["key"] + "_cfg"])))
        m.load_state_dict(_params(g, nc["key"]), strict=True)
        m.eval()
        x_start, planes, noise, t = LC.net_inputs(name)
        seen = []

        def net(x, ts, c_concat=None, **kw):
            seen.append(m(torch.cat([x] + list(c_concat), 1), ts))
            return seen[-1]
        for mode in DC.MODES:
            del seen[:]
            r = run_ref(nc, net, x_start, noise, t, planes, mode, torch.float32)
            o, feats = seen[0]
            again = run_ref(nc, lambda x, ts, **kw: (o, feats), x_start, noise, t, planes, mode, torch.float32)
            assert all(np.array_equal(r[k], again[k]) for k in r), name
            gen = torch.Generator().manual_seed(13000 + DC.MODES.index(mode))
            noisy = {k: [f + DC.NET_NOISE * f.norm() / f.numel() ** 0.5 * torch.randn(f.shape, generator=gen) for f in feats[k]]
                     for k, _ in DC.HEADS}
            p = run_ref(nc, lambda x, ts, **kw: (o, noisy), x_start, noise, t, planes, mode, torch.float32)
            for k, v in r.items():
                assert np.isfinite(v).all(), (name, mode, k)
                out[f"net_{name}_{mode}_{k}"] = v.astype(np.float32)
                out[f"sens_{name}_{mode}_{k}"] = np.float64(DC.dist(p[k], v))
            out[f"net_{name}_{mode}_keys"] = json.dumps(sorted(r))
            print(f"net {name} {mode}: " + ", ".join(f"{k} {float(r[k]):.5f} (sens {DC.dist(p[k], r[k]):.1e})" for k in DC.LOSSES)
                  + "; maps " + ", ".join(f"{DC.dist(p[k], r[k]):.1e}" for k in DC.MAPS))


def main():
    out = {}
    gen_stub(out)
    gen_net(out)
    out["modes"], out["net_names"] = json.dumps(DC.MODES), json.dumps(DC.NET_NAMES)
    path = os.path.join(HERE, "disentangle.npz")
    np.savez_compressed(path, **out)
    print("wrote disentangle.npz:", len(out), "entries,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
