#!/usr/bin/env python3
"""The disentanglement losses measured on one GPU, one process, hipEvent medians of --repeats runs after an untimed one.

  op      per mode ('contrast', 'eu', 'eu&contrast') and for the L1 metric, at batch --batch with head tensors of the size
          configs/v2-1-cddpm-ds-disc.yaml gives at 256x256 (480 x 8 x 8): dsd_op_contrast_rows on content + style (R = 6B) and
          on style + anatomy + lesion (R = 7B), beside the same formulas written in torch ops on the same GPU the way the
          reference writes them (the R x R x D broadcast of CosineSimilarity, cdist in float64): the calibration.
  net     training_losses on the full-size network (synthetic weights) at batch --batch with and without disentangle=, the two
          alternated; a batch that does not fit is halved until it does and the line says so.  Then one profiled call per mode:
          the time dsd_profile records for the contrast_rows calls behind the forward (three kernels each, no allocation).
  plain   dsd_eval_loss without a rider through training_losses on the ds_tiny fixture network (tests/loss_cases.py) and, with
          --full, on the full-size network.  Run once per library (DSD_LIBRARY=<the parent's build>, then the in-tree one): the
          two JSONs are compared by hand or with --compare.

    python tools/bench_disentangle.py --only op,net --json profiles/disentangle_bench.json
    DSD_LIBRARY=<parent build> python tools/bench_disentangle.py --only plain --json parent.json
    python tools/bench_disentangle.py --only plain --json this.json
    python tools/bench_disentangle.py --merge profiles/disentangle_bench.json parent.json this.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only", default="op,net,plain")
ap.add_argument("--full", action="store_true", help="plain: the full-size network too")
ap.add_argument("--json")
ap.add_argument("--merge", nargs=3, metavar=("OUT", "PARENT", "THIS"))
args = ap.parse_args()

if args.merge:
    out, parent, this = (json.load(open(p)) if os.path.exists(p) else {} for p in args.merge)
    out["plain_eval_loss"] = {"parent": parent.get("plain"), "this": this.get("plain"), "parent_library": parent.get("library"),
                              "library": this.get("library")}
    json.dump(out, open(args.merge[0], "w"), indent=1)
    print(json.dumps(out["plain_eval_loss"], indent=1))
    sys.exit(0)

import torch  # noqa: E402
import yaml  # noqa: E402

from diffusion_models_dsdiff_amd import _lib, _sched as S  # noqa: E402
from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion  # noqa: E402

HEAD = (480, 8, 8)
MODES = ("contrast", "eu", "eu&contrast")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "runs": len(v)}


def alternate(fns, repeats):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[1])
    return {k: stats(v) for k, v in ms.items()}


def torch_form(X, rows, mode, temperature):
    """get_disentangle_loss / ContrastiveLoss in torch ops, as the reference writes them (:1056-1094, contrastive_loss.py)."""
    R, n = X.shape
    lab = rows.view(-1, 1)
    mask = torch.eq(lab, lab.T)
    eye = torch.eye(R, dtype=torch.bool, device=X.device)

    def cl():
        logits = torch.nn.functional.cosine_similarity(X.unsqueeze(1), X.unsqueeze(0), dim=-1) / temperature
        lm = (~eye).float()
        m = mask.float() * lm
        log_prob = logits - torch.log((torch.exp(logits) * lm).sum(1, keepdim=True))
        return -((m * log_prob).sum(1) / (m.sum(1) + 1e-6)).mean()

    def ratio(logits):
        return torch.div((logits * ~eye * mask).sum(), (logits * ~mask).sum())
    if mode == "contrast":
        return cl()
    if mode == "eu":
        return ratio(torch.cdist(X.double(), X.double(), p=2).float() / n)
    if mode == "l1":
        return ratio(torch.cdist(X, X, p=1) / n)
    return ratio(torch.cdist(X, X, p=2) / n) + 0.05 * cl()


def bench_op(B, repeats):
    out = {}
    g = torch.Generator(device="cuda").manual_seed(7)
    n = HEAD[0] * HEAD[1] * HEAD[2]
    for views, temperature in ((6, 0.05), (7, 0.1)):
        vs = [torch.randn(B, n, device="cuda", generator=g) + 0.5 for _ in range(views)]
        lab = S.disentangle_labels(B)[0 if views == 6 else 1]
        rows = S.label_rows(lab).cuda()
        X = torch.cat(vs, 0)
        for mode in MODES + ("l1",):
            fns = {"op": lambda: S.contrast_rows(vs, rows, mode, temperature)[0]}
            try:
                torch_form(X, rows, mode, temperature)
                fns["torch"] = lambda: torch_form(X, rows, mode, temperature)
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
            r = alternate(fns, repeats)
            r["rows"], r["n"], r["feature_bytes"] = views * B, n, views * B * n * 4
            if "torch" in r:
                r["loss_op"], r["loss_torch"] = float(fns["op"]()), float(fns["torch"]())
            out[f"{views}views_{mode}"] = r
            print(f"op {views} views {mode}: " + ", ".join(f"{k} {v['median_ms']} ms" for k, v in r.items() if isinstance(v, dict)), flush=True)
    return out


def full_network():
    from bench import synth_weights_
    from diffusion_models_dsdiff_amd.ldm.util import instantiate_from_config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "v2-1-cddpm-ds-disc.yaml")))
    uc = dict(cfg["model"]["params"]["unet_config"])
    torch.manual_seed(2024)
    model = instantiate_from_config(uc)
    synth_weights_(model, 2024)
    model.sync_params(force=True)
    return model


def loss_inputs(B, size):
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(B, 1, size, size, device="cuda", generator=g).clamp_(-1, 1)
    cond = [torch.randn(B, 1, size, size, device="cuda", generator=g).clamp_(-1, 1) for _ in range(3)]
    z = torch.randn(B, 1, size, size, device="cuda", generator=g)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=g)
    return x, cond, z, t


def bench_net(model, B, size, repeats, modes):
    d = create_gaussian_diffusion(steps=1000)
    while True:
        try:
            x, cond, z, t = loss_inputs(B, size)
            fns = {"plain": lambda: d.training_losses(model, x, t, model_kwargs=dict(c_concat=cond), noise=z)["loss"]}
            for m in modes:
                fns[m] = (lambda m: lambda: d.training_losses(model, x, t, model_kwargs=dict(c_concat=cond), noise=z, disentangle=m)["loss"])(m)
            r = alternate(fns, repeats)
            break
        except (torch.cuda.OutOfMemoryError, _lib.DsdError) as e:
            if B == 1 or "memory" not in str(e).lower():
                raise
            B //= 2
            torch.cuda.empty_cache()
    r["batch"], r["size"] = B, size
    for m in modes:
        r[m]["extra_ms"] = round(r[m]["median_ms"] - r["plain"]["median_ms"], 4)
        r[m]["extra_percent"] = round(100 * (r[m]["median_ms"] / r["plain"]["median_ms"] - 1), 4)
    if modes:   # the kernels' own time: the records dsd_profile keeps of the two contrast_rows calls behind the forward
        model.profile(True)
        try:
            for m in modes:
                fns[m]()
            rep, runs = model.profile_report()
        finally:
            model.profile(False)
        c = rep["contrast_rows"]
        r["contrast_rows_profile"] = {"ms_per_call": round(c["ms"] / c["calls"], 4), "calls": c["calls"], "feature_bytes_per_call": c["bytes"] / c["calls"],
                                      "forwards": runs}
    print("net: " + ", ".join(f"{k} {v.get('median_ms', v.get('ms_per_call'))} ms" for k, v in r.items() if isinstance(v, dict)), flush=True)
    return r


def bench_plain(repeats, full, B, size):
    import loss_cases as LC
    import test_loss_gpu as TL
    out = {}
    nc = LC.NET_CASES["ds_tiny"]
    model, unet, x_start, planes, z, t, _ = TL.net_env("ds_tiny")
    d = TL.product_diffusion(nc)
    out["ds_tiny"] = alternate({"eval_loss": lambda: d.training_losses(model, x_start, t, model_kwargs=dict(c_concat=planes), noise=z)["loss"]},
                               4 * repeats)["eval_loss"]
    out["ds_tiny"]["launches"] = unet.plan_info()["launches"]
    if full:
        net = full_network()
        out["full"] = bench_net(net, B, size, repeats, ())
        out["full"]["launches"] = net.plan_info()["launches"]
    print("plain:", json.dumps(out), flush=True)
    return out


def main():
    name, ncu, _ = _lib.require_gpu(0)
    res = {"gpu": name, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "batch": args.batch, "repeats": args.repeats}
    only = set(args.only.split(","))
    if "op" in only:
        res["op"] = bench_op(args.batch, args.repeats)
    if "net" in only:
        res["net"] = bench_net(full_network(), args.batch, args.size, args.repeats, MODES)
    if "plain" in only:
        res["plain"] = bench_plain(args.repeats, args.full, args.batch, args.size)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))


if __name__ == "__main__":
    main()
