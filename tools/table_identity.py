#!/usr/bin/env python3
"""Before / after identity of what a handle IS: the parameter table (dsd_param_info: index, name, shape) of every kind of
network on table-only handles (device -1), and dsd_last_error() of dsd_create / dsd_block_create for one malformed
configuration per validity rule.  No GPU needed.

    DSD_LIBRARY=<a build> python tools/table_identity.py --out a.json       # one process per library
    python tools/table_identity.py --out b.json                             # (the in-tree build)
    python tools/table_identity.py --compare a.json b.json [--json verdict.json]

Tables: the fixture DSUnetModels (the one table serves 2 and 4 input channels: the handle is the same, dsd_forward picks the
branch), the fixture UNet_disc_Model, the latent UNetModel plain / with spatial transformers / with each label_emb kind, the tiny
DiT with and without classes and learn_sigma, the KL-VAE encoder and decoder at fixture size, one handle of every other kind."""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def compare(pa, pb, out):
    a, b = json.load(open(pa)), json.load(open(pb))
    verdict = {"a": a["library"], "b": b["library"]}
    for part in ("tables", "errors"):
        names = sorted(set(a[part]) | set(b[part]))
        verdict[part] = {k: k in a[part] and k in b[part] and a[part][k] == b[part][k] for k in names}
        for k, ok in verdict[part].items():
            if not ok:
                print("DIFFERENT", part, k, a[part].get(k) if part == "errors" else "", b[part].get(k) if part == "errors" else "")
    verdict["n_tables"], verdict["n_errors"] = len(verdict["tables"]), len(verdict["errors"])
    verdict["n_params"] = sum(len(t) for t in a["tables"].values())
    verdict["all_equal"] = all(bool(verdict[p]) and all(verdict[p].values()) for p in ("tables", "errors"))
    print(f"{verdict['n_tables']} tables ({verdict['n_params']} parameters), {verdict['n_errors']} errors, all_equal = {verdict['all_equal']}")
    if out:
        json.dump(verdict, open(out, "w"), indent=1)
    return 0 if verdict["all_equal"] else 1


def collect(verbose=False):
    """(tables, errors, library path) of the library _lib loads."""
    from diffusion_models_dsdiff_amd import _lib
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.openaimodel import unet_iargs
    from diffusion_models_dsdiff_amd.ldm.modules.diffusionmodules.model import _iargs as vae_iargs
    import disc_ref as R
    from util import golden

    L = _lib.lib()
    TABLES, ERRORS = {}, {}


    def config(kw, disc=False):
        cfg = _lib.DsdConfig()
        cfg.in_channels, cfg.model_channels, cfg.out_channels = kw["in_channels"], kw["model_channels"], kw["out_channels"]
        nrb = kw["num_res_blocks"]
        cfg.n_levels = len(kw["channel_mult"])
        for i, m in enumerate(kw["channel_mult"][:_lib.DSD_MAX_LEVELS]):
            cfg.channel_mult[i], cfg.num_res_blocks[i] = m, nrb if isinstance(nrb, int) else nrb[i]
        cfg.n_attention_resolutions = len(kw["attention_resolutions"])
        for i, a in enumerate(kw["attention_resolutions"]):
            cfg.attention_resolutions[i] = a
        cfg.num_heads, cfg.num_head_channels, cfg.num_heads_upsample = kw.get("num_heads", 1 if disc else -1), kw.get("num_head_channels", -1), -1
        cfg.use_scale_shift_norm, cfg.resblock_updown = int(kw.get("use_scale_shift_norm", False)), int(kw.get("resblock_updown", False))
        cfg.use_new_attention_order, cfg.legacy = int(kw.get("use_new_attention_order", False)), int(kw.get("legacy", True))
        return cfg


    def create(what, arg):
        """(rc, handle) of dsd_create ("model"), dsd_create_disc ("disc") or dsd_block_create (a kind) on no device."""
        h = C.c_void_p()
        if what in ("model", "disc"):
            rc = (L.dsd_create_disc if what == "disc" else L.dsd_create)(C.byref(config(arg, what == "disc")), -1, C.byref(h))
        else:
            ia = [int(v) for v in arg]
            rc = L.dsd_block_create(what, (C.c_int32 * len(ia))(*ia), len(ia), -1, C.byref(h))
        return rc, h


    def table(name, what, arg):
        rc, h = create(what, arg)
        _lib.check(rc)
        rows = []
        cname, shape, ndim = C.c_char_p(), (C.c_int64 * 8)(), C.c_int()
        for i in range(L.dsd_param_count(h)):
            _lib.check(L.dsd_param_info(h, i, C.byref(cname), shape, C.byref(ndim)))
            rows.append([i, cname.value.decode(), [int(shape[k]) for k in range(ndim.value)]])
        L.dsd_destroy(h)
        TABLES[name] = rows
        if verbose:
            print(f"{name}: {len(rows)} parameters", flush=True)


    def error(name, what, arg):
        rc, h = create(what, arg)
        ERRORS[name] = L.dsd_last_error().decode() if rc else "(created)"
        if not rc:
            L.dsd_destroy(h)


    g = golden("model")
    tiny = json.loads(str(g["tiny_cfg"]))
    table("tiny", "model", tiny)
    table("tinyfilm", "model", json.loads(str(g["tinyfilm_cfg"])))
    table("disc_tiny", "disc", R.case("tiny")[0])
    lat = json.loads(str(golden("latent_ldm")["unet_cfg"]))
    table("latent_unet", _lib.BLOCK_UNET, unet_iargs(**lat))
    ST = dict(in_channels=6, model_channels=64, out_channels=3, num_res_blocks=1, attention_resolutions=[2], channel_mult=[1, 2],
              num_head_channels=16, use_spatial_transformer=True, transformer_depth=1, context_dim=40, use_linear_in_transformer=True,
              legacy=True, resblock_updown=True, use_scale_shift_norm=True)
    table("latent_unet_spatial_transformer", _lib.BLOCK_UNET, unet_iargs(**ST))
    table("latent_unet_spatial_transformer_conv_classes", _lib.BLOCK_UNET, unet_iargs(**dict(ST, use_linear_in_transformer=False, num_classes=7)))
    for nm, kw in (("classes", dict(num_classes=7)), ("continuous", dict(num_classes="continuous")),
                   ("sequential", dict(num_classes="sequential", adm_in_channels=12))):
        table("latent_unet_label_" + nm, _lib.BLOCK_UNET, unet_iargs(**dict(lat, **kw)))
    DIT = [16, 2, 4, 64, 2, 4, 256, 0, 0, 0]    # input, patch, in_channels, hidden, depth, heads, mlp_hidden, classes, learn_sigma, cfg_emb
    table("dit", _lib.BLOCK_DIT, DIT)
    table("dit_classes", _lib.BLOCK_DIT, DIT[:7] + [10, 0, 1])
    table("dit_classes_nocfg", _lib.BLOCK_DIT, DIT[:7] + [10, 0, 0])
    table("dit_learn_sigma", _lib.BLOCK_DIT, DIT[:2] + [6] + DIT[3:8] + [1, 0])
    dd = json.loads(str(golden("vae")["small_cfg"]))
    VAE = vae_iargs(dd["ch"], dd["out_ch"], dd["ch_mult"], dd["num_res_blocks"], dd["attn_resolutions"], dd["in_channels"], dd["resolution"],
                    dd["z_channels"], dd.get("double_z", True), dd.get("embed_dim") or dd["z_channels"], 1)
    table("vae_encoder", _lib.BLOCK_VAE_ENCODER, VAE)
    table("vae_decoder", _lib.BLOCK_VAE_DECODER, VAE)
    table("vae_encoder_noquant", _lib.BLOCK_VAE_ENCODER, VAE[:8] + [0] + VAE[9:])
    table("vae_decoder_noquant", _lib.BLOCK_VAE_DECODER, VAE[:8] + [0] + VAE[9:])
    SMALL = {"res": (_lib.BLOCK_RES, [64, 32, 128, 0, 0, 0]), "res_film_up": (_lib.BLOCK_RES, [64, 64, 128, 1, 1, 0]),
             "attn": (_lib.BLOCK_ATTN, [64, 4, 1]), "upsample": (_lib.BLOCK_UPSAMPLE, [64]), "downsample": (_lib.BLOCK_DOWNSAMPLE, [64]),
             "disentangle": (_lib.BLOCK_DISENTANGLE, [64, 32]), "se": (_lib.BLOCK_SE, [64, 8]), "crossattn": (_lib.BLOCK_CROSSATTN, [64, 32, 4, 16]),
             "ff_geglu": (_lib.BLOCK_FF_GEGLU, [64, 4]), "basic_transformer": (_lib.BLOCK_BASIC_TRANSFORMER, [64, 4, 16, 32]),
             "spatial_transformer": (_lib.BLOCK_SPATIAL_TRANSFORMER, [64, 4, 16, 2, 32, 1]),
             "spatial_transformer_conv": (_lib.BLOCK_SPATIAL_TRANSFORMER, [64, 4, 16, 1, 32, 0]), "vae_attn": (_lib.BLOCK_VAE_ATTN, [64])}
    for nm, (kind, ia) in SMALL.items():
        table("block_" + nm, kind, ia)

    # ---- one malformed configuration per rule
    for nm, (kind, ia) in SMALL.items():
        error(f"short_{nm}", kind, ia[:-1])
        error(f"none_{nm}", kind, [])
    error("unknown_kind", 15, [1, 2, 3])
    error("unknown_kind_negative", -1, [1, 2, 3])
    U = unet_iargs(**lat)
    nl = U[10]
    error("dit_short", _lib.BLOCK_DIT, DIT[:9])
    error("dit_patch", _lib.BLOCK_DIT, [16, 3] + DIT[2:])
    error("dit_patch_zero", _lib.BLOCK_DIT, [16, 0] + DIT[2:])
    error("dit_heads", _lib.BLOCK_DIT, DIT[:5] + [5] + DIT[6:])
    error("dit_head_dim", _lib.BLOCK_DIT, DIT[:3] + [24, 2, 4] + DIT[6:])
    error("dit_head_dim_wide", _lib.BLOCK_DIT, DIT[:3] + [512, 2, 2] + DIT[6:])
    error("dit_depth", _lib.BLOCK_DIT, DIT[:4] + [0] + DIT[5:])
    error("dit_mlp", _lib.BLOCK_DIT, DIT[:6] + [254] + DIT[7:])
    error("dit_learn_sigma_cout", _lib.BLOCK_DIT, DIT[:2] + [2] + DIT[3:8] + [1, 0])
    error("vae_short", _lib.BLOCK_VAE_ENCODER, VAE[:10])
    error("vae_dec_short", _lib.BLOCK_VAE_DECODER, VAE[:10])
    error("vae_mult", _lib.BLOCK_VAE_ENCODER, VAE[:9] + [9] + VAE[10:])
    error("vae_mult_zero", _lib.BLOCK_VAE_ENCODER, VAE[:9] + [0] + VAE[10:])
    error("vae_mult_truncated", _lib.BLOCK_VAE_ENCODER, VAE[:11])
    error("vae_attn_res", _lib.BLOCK_VAE_DECODER, VAE[:10 + VAE[9]] + [-1])
    error("vae_attn_res_truncated", _lib.BLOCK_VAE_DECODER, VAE[:10 + VAE[9]] + [3, 16])
    error("vae_ch", _lib.BLOCK_VAE_ENCODER, [48] + VAE[1:])
    error("vae_ch_small", _lib.BLOCK_VAE_DECODER, [0] + VAE[1:])
    error("vae_nrb", _lib.BLOCK_VAE_ENCODER, VAE[:7] + [0] + VAE[8:])
    error("vae_z", _lib.BLOCK_VAE_DECODER, VAE[:4] + [0] + VAE[5:])
    error("unet_short", _lib.BLOCK_UNET, U[:11])
    error("unet_levels", _lib.BLOCK_UNET, U[:10] + [9] + U[11:])
    error("unet_levels_zero", _lib.BLOCK_UNET, U[:10] + [0] + U[11:])
    error("unet_mult_truncated", _lib.BLOCK_UNET, U[:12 + nl])
    error("unet_attention_resolutions", _lib.BLOCK_UNET, U[:11 + 2 * nl] + [9])
    error("unet_attention_resolutions_negative", _lib.BLOCK_UNET, U[:11 + 2 * nl] + [-1])
    error("unet_attention_resolutions_truncated", _lib.BLOCK_UNET, U[:11 + 2 * nl] + [2, 1])
    error("unet_st_depth", _lib.BLOCK_UNET, U + [1, 2, 24, 0])
    error("unet_st_ctx_dim", _lib.BLOCK_UNET, U + [1, 1, 0, 0])
    error("unet_st_truncated_is_ignored", _lib.BLOCK_UNET, U + [1, 2, 24])
    error("unet_label_kind", _lib.BLOCK_UNET, U + [0, 1, 0, 0, 4, 7])
    error("unet_label_kind_negative", _lib.BLOCK_UNET, U + [0, 1, 0, 0, -1, 7])
    error("unet_label_width_classes", _lib.BLOCK_UNET, U + [0, 1, 0, 0, 1, 0])
    error("unet_label_width_sequential", _lib.BLOCK_UNET, U + [0, 1, 0, 0, 3, 0])
    error("unet_label_continuous_width_is_ignored", _lib.BLOCK_UNET, U + [0, 1, 0, 0, 2, 0])
    # the order of the rules of one handle: trunk (build_spec) between the transformer rule and the label rule
    error("unet_st_depth_before_trunk", _lib.BLOCK_UNET, U[:1] + [48] + U[2:] + [1, 2, 24, 0])
    error("unet_trunk_before_label", _lib.BLOCK_UNET, U[:1] + [48] + U[2:] + [0, 1, 0, 0, 4, 7])
    error("unet_model_channels", _lib.BLOCK_UNET, U[:1] + [48] + U[2:])
    error("unet_heads", _lib.BLOCK_UNET, U[:3] + [-1, -1] + U[5:])
    # the two models
    error("model_in_channels", "model", dict(tiny, in_channels=2))
    error("model_levels", "model", dict(tiny, channel_mult=[1] * 9, num_res_blocks=1))
    error("model_channels", "model", dict(tiny, model_channels=48))
    error("model_heads", "model", dict(tiny, num_heads=-1, num_head_channels=-1))
    error("model_final_ch", "model", dict(tiny, channel_mult=[2] + list(tiny["channel_mult"])[1:]))
    dcfg = R.case("tiny")[0]
    error("disc_levels", "disc", dict(dcfg, channel_mult=[1] * 9, num_res_blocks=1))
    error("disc_mult0", "disc", dict(dcfg, channel_mult=[2] + list(dcfg["channel_mult"])[1:]))
    error("disc_mult0_before_trunk", "disc", dict(dcfg, model_channels=48, channel_mult=[2] + list(dcfg["channel_mult"])[1:]))
    error("disc_channels", "disc", dict(dcfg, model_channels=48))
    return TABLES, ERRORS, os.path.relpath(_lib.LIB_PATH, ROOT)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.json))
    tables, errors, library = collect(verbose=True)
    json.dump({"library": library, "tables": tables, "errors": errors}, open(args.out, "w"))
    print(f"wrote {len(tables)} tables and {len(errors)} errors to {args.out}")
