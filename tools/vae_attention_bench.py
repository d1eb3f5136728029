#!/usr/bin/env python3
"""KL-VAE AttnBlock: the materialised route (default) against the fused route (dsd_set_vae_fused_attention), on the two first
stages the project ships numbers for, at 256 x 256:

    kl64   configs/autoencoder_kl_64x64x3.yaml   ch 128, ch_mult [1,2,4]     mid map 64 x 64 (T = 4096), C = 512
    sdv1   the SD-v1 first stage                 ch 128, ch_mult [1,2,4,4]   mid map 32 x 32 (T = 1024), C = 512

Per first stage, route and repeat: encode and decode wall time (device events around `--iters` calls after a warm-up, profiler
off), then the `vae_attention` op time of one encode from the per-op events (dsd_profile_op_get; a run of its own).  The routes
alternate inside a repeat, so drift of the box hits both alike; the spread over the repeats is printed with the medians.

    python tools/vae_attention_bench.py [--batch 16] [--repeats 3] [--iters 3] [--routes off,on] [--json out.json]

--routes off runs on a library without the setter too (the parent of the change that added it)."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffusion_models_dsdiff_amd.ldm.models.autoencoder import AutoencoderKL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--routes", default="off,on")
ap.add_argument("--precision", default="bf16x6")
ap.add_argument("--json", default=None)
args = ap.parse_args()
routes = args.routes.split(",")

STAGES = {
    "kl64": (dict(double_z=True, z_channels=3, resolution=256, in_channels=1, out_ch=1, ch=128, ch_mult=[1, 2, 4], num_res_blocks=2,
                  attn_resolutions=[], dropout=0.0), 3, 1),
    "sdv1": (dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                  num_res_blocks=2, attn_resolutions=[], dropout=0.0), 4, 3),
}


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def attn_op_ms(half, x):
    half.profile(True)
    half(x)
    ms = sum(o[1] for o in half.profile_ops() if o[0] == "vae_attention")
    half.profile(False)
    return ms


rows = []
for name, (dd, embed, cin) in STAGES.items():
    torch.manual_seed(7)
    m = AutoencoderKL(dd, None, embed, train_from_hgf=(cin != 1))
    m.set_precision(args.precision)
    g = torch.Generator().manual_seed(8)
    f = 2 ** (len(dd["ch_mult"]) - 1)
    x = torch.randn(args.batch, cin, 256, 256, generator=g).cuda()
    z = torch.randn(args.batch, embed, 256 // f, 256 // f, generator=g).cuda()
    ref = {}
    for rep in range(args.repeats):
        for route in routes:
            if route == "on" or hasattr(m, "set_fused_attention"):
                m.set_fused_attention(route == "on")
            enc = timed(lambda: m.encode(x), args.iters)
            dec = timed(lambda: m.decode(z), args.iters)
            a_enc, a_dec = attn_op_ms(m._enc, x), attn_op_ms(m._dec, z)
            mo = m.encode(x).parameters
            ref.setdefault(route, mo)
            rows.append(dict(stage=name, route=route, repeat=rep, batch=args.batch, precision=args.precision, encode_ms=enc,
                             decode_ms=dec, vae_attention_encode_ms=a_enc, vae_attention_decode_ms=a_dec))
            print(json.dumps(rows[-1]), flush=True)
    if len(ref) == 2:
        d = float((ref["on"].double() - ref["off"].double()).norm() / ref["off"].double().norm())
        print(f"{name}: moments of the two routes differ by rel-L2 {d:.3e}", flush=True)
    del m
    torch.cuda.empty_cache()

print(f"\nbatch {args.batch}, {args.precision}, 256 x 256, median of {args.repeats} (min .. max)")
summary = []
for name in STAGES:
    for route in routes:
        sel = [r for r in rows if r["stage"] == name and r["route"] == route]
        line = dict(stage=name, route=route)
        txt = f"{name:5s} {route:3s}"
        for k in ("vae_attention_encode_ms", "vae_attention_decode_ms", "encode_ms", "decode_ms"):
            v = [r[k] for r in sel]
            line[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
            txt += f"  {k[:-3]} {statistics.median(v):8.2f} ({min(v):.2f} .. {max(v):.2f})"
        summary.append(line)
        print(txt)
if args.json:
    with open(args.json, "w") as fjs:
        json.dump(dict(rows=rows, summary=summary), fjs, indent=1)
