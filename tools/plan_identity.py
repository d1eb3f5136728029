#!/usr/bin/env python3
"""Before / after identity of the plan builder (csrc/net.cpp): what one library plans and computes for every kind of
network the builder assembles, as a JSON that two builds can be compared on field by field.

    DSD_LIBRARY=<a build> python tools/plan_identity.py --out a.json        # one fresh process per library
    python tools/plan_identity.py --out b.json                              # (the in-tree build)
    python tools/plan_identity.py --compare a.json b.json [--json verdict.json]
A library from before the device loops took one entry point each no longer matches the binding's loop signatures (the
zero-stream case runs a loop): run such a build from its own checkout, not through DSD_LIBRARY.

Per case: plan_info() (workspace_bytes, launches, flops, device_bytes), every op of profile_ops() as (kind, flops, bytes,
layer name) in launch order (the times are dropped), and the SHA-256 of the output of one forward on seeded inputs.
Cases: the tiny fixture DSUnetModels (2 / 4 input channels, with and without feature outputs), every arithmetic mode and
planner switch on one of them, zero-stream sharing in a device loop, the 981.5 M headline network at 256x256 (batch 1 with
a forward, batch 16 as a plan; defaults and Winograd), the latent UNetModel (plain and with spatial transformers), the tiny
DiT in bf16x6 / f16 / bf16, the KL-VAE at fixture size and at the size of configs/autoencoder_kl_64x64x3.yaml, one handle of
every other block kind, and a precision round trip (bf16x6 -> f16x3 -> bf16x6) with device_bytes after each forward.
--skip-full leaves the headline network out (it needs ~10 GB of device memory and most of the run time)."""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def compare(pa, pb, out):
    a, b = json.load(open(pa)), json.load(open(pb))
    cases = {}
    for k in sorted(set(a["cases"]) | set(b["cases"])):
        ca, cb = a["cases"].get(k), b["cases"].get(k)
        fields = sorted(set(ca or {}) | set(cb or {}))
        cases[k] = {f: ca is not None and cb is not None and ca.get(f) == cb.get(f) for f in fields}
    verdict = {"a": a["library"], "b": b["library"], "n_cases": len(cases), "n_ops": sum(len(c.get("ops", [])) for c in a["cases"].values()),
               "cases": cases, "all_equal": bool(cases) and all(all(c.values()) and c for c in cases.values())}
    for k, c in cases.items():
        if not all(c.values()):
            print("DIFFERENT", k, [f for f, ok in c.items() if not ok])
    print(f"{len(cases)} cases, all_equal = {verdict['all_equal']}")
    if out:
        json.dump(verdict, open(out, "w"), indent=1)
    return 0 if verdict["all_equal"] else 1


ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2)
ap.add_argument("--json")
ap.add_argument("--skip-full", action="store_true")
args = ap.parse_args()
if args.compare:
    sys.exit(compare(args.compare[0], args.compare[1], args.json))

import torch, yaml
from diffusion_models_dsdiff_amd import _lib, blocks
from diffusion_models_dsdiff_amd.UNet_DS_Diff.model import DSUnetModel
from diffusion_models_dsdiff_amd.UNet_DS_Diff.DiT_models import DiT
from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.model import Encoder, Decoder
from diffusion_models_dsdiff_amd.ldm.models.autoencoder import AutoencoderKL
from oracle.synth import synth_params, randn, cond_image
from util import golden, fixture_params

_lib.require_gpu(0)
CASES = {}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def record(name, m, run, hash_output=True):
    """run() -> tensor or list of tensors.  One profiled forward for the op list, one plain forward for the hash."""
    m.profile(True)
    run()
    ops = [[k, fl, by, nm] for k, _ms, fl, by, nm in m.profile_ops()]
    m.profile(False)
    c = {"ops": ops}
    if hash_output:
        out = run()
        c["sha256"] = sha(*(out if isinstance(out, (list, tuple)) else [out]))
    c["plan"] = m.plan_info()
    CASES[name] = c
    print(f"{name}: {len(ops)} ops, {c['plan']}", flush=True)
    return c


def synth(m, seed):
    m.load_state_dict(synth_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed), strict=True)
    return m


def unet_run(m, x, t, feats):
    def run():
        y, f = m._run(x, t, want_feats=feats)
        return [y] + [v for k in sorted(f) for v in f[k]]
    return run


# ---- the tiny fixture DSUnetModels
g = golden("model")
for key in ("tiny", "tinyfilm"):
    m = DSUnetModel(**json.loads(str(g[key + "_cfg"])))
    m.load_state_dict(fixture_params(g, key), strict=True)
    t = torch.tensor([999, 17]).cuda()
    for C in (2, 4):
        x = randn((2, C, 32, 32), 70 + C).cuda()
        for feats in (True, False):
            record(f"{key}_c{C}_feats{int(feats)}", m, unet_run(m, x, t, feats))
    if key != "tiny":
        continue
    # ---- every arithmetic mode and planner switch, on this one
    x = randn((2, 4, 32, 32), 71).cuda()
    for prec in ("f32", "bf16x6", "bf16x3", "f16x3"):
        m.set_precision(prec)
        record(f"tiny_{prec}", m, unet_run(m, x, t, False))
    m.set_precision("bf16x6")
    for nm, on, off in (("lanes_off", lambda: m.stream_lanes(False), lambda: m.stream_lanes(True)),
                        ("gn_stats_off", lambda: m.fuse_gn_stats(False), lambda: m.fuse_gn_stats(True)),
                        ("gn_apply_off", lambda: m.fuse_gn_apply(False), lambda: m.fuse_gn_apply(True)),
                        ("winograd_on", lambda: m.winograd(True), lambda: m.winograd(False))):
        on()
        record("tiny_" + nm, m, unet_run(m, x, t, False))
        off()
    # ---- zero-stream sharing: planned by the device loops only
    from diffusion_models_dsdiff_amd.Disc_diff.guided_diffusion.script_util import create_gaussian_diffusion
    from diffusion_models_dsdiff_amd._sched import run_device_loop
    sched = create_gaussian_diffusion(steps=1000, parameterization="v")._schedule(False, 0.0, True)
    shape = (2, 1, 32, 32)
    cond, xT = cond_image(shape, 21).cuda(), randn(shape, 22).cuda()
    m.share_zero_streams(True)
    record("tiny_share_zero_streams", m, lambda: run_device_loop(m, sched, xT, cond, seed=5, first_step=0, n_steps=2))
    m.share_zero_streams(False)
    # ---- precision round trip: which derived weights are resident after each forward
    trip = []
    for prec in ("bf16x6", "f16x3", "bf16x6"):
        m.set_precision(prec)
        y = m._run(x, t, want_feats=False)[0]
        trip.append({"precision": prec, "sha256": sha(y), "plan": m.plan_info()})
    CASES["tiny_precision_round_trip"] = {"steps": trip}
    print("tiny_precision_round_trip:", [s["plan"]["device_bytes"] for s in trip], flush=True)
    del m

# ---- latent UNetModel: the fixture, and with spatial transformers (tests/test_latent_gpu.py)
g = golden("latent_ldm")
m = UNetModel(**json.loads(str(g["unet_cfg"])))
m.load_state_dict(fixture_params(g, "unet"), strict=True)
x, t = randn((2, m.in_channels, 8, 8), 31).cuda(), torch.tensor([999., 17.]).cuda()
record("latent_unet", m, lambda: m(x, t))
ST = dict(image_size=16, in_channels=6, model_channels=64, out_channels=3, num_res_blocks=1, attention_resolutions=[2],
          channel_mult=[1, 2], num_head_channels=16, use_spatial_transformer=True, transformer_depth=1, context_dim=40,
          use_linear_in_transformer=True, legacy=True, resblock_updown=True, use_scale_shift_norm=True)
mst = synth(UNetModel(**ST), 410)
xs, cs = randn((2, 6, 16, 8), 411).cuda(), randn((2, 7, 40), 412).cuda()
record("latent_unet_spatial_transformer", mst, lambda: mst(xs, t, context=cs))
del m, mst

# ---- tiny DiT (tests/test_dit_gpu.py) in the fp32-grade mode and both half-precision modes
dit = synth(DiT(input_size=16, patch_size=2, in_channels=4, hidden_size=64, depth=2, num_heads=4, num_classes=10), 901)
xd, cd, yd = randn((2, 3, 16, 16), 5).cuda(), randn((2, 1, 16, 16), 6).cuda(), torch.tensor([1, 4]).cuda()
for prec in ("bf16x6", "f16", "bf16"):
    dit.set_precision(prec)
    record(f"dit_{prec}", dit, lambda: dit(xd, torch.tensor([17.0, 999.0]).cuda(), yd, cond=cd))
del dit

# ---- KL-VAE: fixture size and the yaml's size
gv = golden("vae")
dd = json.loads(str(gv["small_cfg"]))
dd.pop("embed_dim")
sdv = fixture_params(gv, "small")
xshape = tuple(int(v) for v in gv["small_xshape"])
f = 2 ** (len(dd["ch_mult"]) - 1)
enc, dec = Encoder(**dd), Decoder(**dd)
enc.load_state_dict({k[len("encoder."):]: v for k, v in sdv.items() if k.startswith("encoder.")}, strict=True)
dec.load_state_dict({k[len("decoder."):]: v for k, v in sdv.items() if k.startswith("decoder.")}, strict=True)
xe = randn(xshape, 50).cuda()
ze = randn((xshape[0], dd["z_channels"], xshape[2] // f, xshape[3] // f), 51).cuda()
record("vae_encoder_fixture", enc, lambda: enc(xe))
record("vae_decoder_fixture", dec, lambda: dec(ze))
del enc, dec
cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "autoencoder_kl_64x64x3.yaml")))["model"]["params"]
vae = synth(AutoencoderKL(dict(cfg["ddconfig"]), cfg.get("lossconfig"), cfg["embed_dim"]), 77)
xv, zv = randn((1, 1, 256, 256), 78).cuda(), randn((1, cfg["embed_dim"], 64, 64), 79).cuda()
record("vae_encoder_yaml", vae._enc, lambda: vae._enc(xv))
record("vae_decoder_yaml", vae._dec, lambda: vae._dec(zv))
del vae

# ---- one handle of every other block kind
emb = randn((2, 128), 20).cuda()
x64 = randn((2, 64, 16, 16), 21).cuda()
tok, ctx = randn((2, 16, 64), 60).cuda(), randn((2, 9, 32), 61).cuda()
for name, mod, run in [
        ("block_res", blocks.ResBlock(64, 128, 0, out_channels=32), lambda b: b(x64, emb)),
        ("block_res_film_up", blocks.ResBlock(64, 128, 0, use_scale_shift_norm=True, up=True), lambda b: b(x64, emb)),
        ("block_res_down", blocks.ResBlock(64, 128, 0, down=True), lambda b: b(x64, emb)),
        ("block_attn", blocks.AttentionBlock(64, num_head_channels=16, use_new_attention_order=True), lambda b: b(x64)),
        ("block_upsample", blocks.Upsample(64, True), lambda b: b(x64)),
        ("block_downsample", blocks.Downsample(64, True), lambda b: b(x64)),
        ("block_disentangle", blocks.FeatureDisentangle(64, 32), lambda b: b(x64)),
        ("block_se", blocks.SE_Attention(64, 8), lambda b: b(x64)),
        ("block_crossattn", blocks.CrossAttention(64, context_dim=32, heads=4, dim_head=16), lambda b: b(tok, ctx)),
        ("block_ff_geglu", blocks.FeedForward(64, mult=4, glu=True), lambda b: b(tok)),
        ("block_basic_transformer", blocks.BasicTransformerBlock(64, 4, 16, context_dim=32), lambda b: b(tok, ctx)),
        ("block_spatial_transformer", blocks.SpatialTransformer(64, 4, 16, depth=1, context_dim=[32], use_linear=True), lambda b: b(x64, [ctx]))]:
    synth(mod, 300)
    record(name, mod, lambda mod=mod, run=run: run(mod))
    del mod

# ---- the headline network, as tests/test_model_gpu.py's full_model fixture builds it
if not args.skip_full:
    FULL = dict(image_size=32, in_channels=1, out_channels=1, model_channels=320, attention_resolutions=[32, 16, 8],
                num_res_blocks=2, channel_mult=[1, 1, 2, 2, 3, 3], num_head_channels=32, use_new_attention_order=True,
                use_spatial_transformer=False, legacy=False, use_checkpoint=True, adm_in_channels=2048, num_classes=None,
                use_linear_in_transformer=True, transformer_depth=1, context_dim=None)
    full = synth(DSUnetModel(**FULL), 2024)
    x1, t1 = randn((1, 2, 256, 256), 5).cuda(), torch.tensor([731]).cuda()
    x16, t16 = randn((16, 2, 256, 256), 6).cuda(), (torch.arange(16) * 61 + 3).cuda()
    for nm, wino in (("full", False), ("full_winograd", True)):
        full.winograd(wino)
        record(nm + "_b1", full, unet_run(full, x1, t1, False))
        record(nm + "_b16_plan", full, unet_run(full, x16, t16, False), hash_output=False)

json.dump({"library": os.path.relpath(_lib.LIB_PATH, ROOT), "cases": CASES}, open(args.out, "w"))
print(f"wrote {len(CASES)} cases to {args.out}")
