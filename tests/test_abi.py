"""The C-ABI library loads and exports every symbol include/dsdiff.h declares (no compute calls, no GPU)."""
import ctypes as C
import os
import re

from diffusion_models_dsdiff_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "dsdiff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dsd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    L = _lib.lib()
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/dsdiff.h but not exported by libdsdiff.so"
    assert sorted(_lib.EXPORTS) == names, "python binding list out of sync with the header"


# one entry point per device loop (the handle picks the denoiser, g / inp are nullable), and the per-variant twins each once had
VARIANTS = {"dsd_sample": ("_latent", "_guided", "_latent_guided", "_masked", "_latent_masked"),
            "dsd_sample_dpm": ("_latent", "_guided", "_latent_guided"), "dsd_sample_dpm_program": ("_latent",),
            "dsd_sample_plms": ("_latent",), "dsd_invert": ("_latent",), "dsd_calc_bpd": ("_latent",)}
LOOPS = tuple(VARIANTS)
REMOVED = [loop + v for loop, vs in VARIANTS.items() for v in vs]


def test_one_entry_point_per_device_loop():
    names = header_functions()
    assert len(REMOVED) == 12
    for n in LOOPS:
        assert n in names and n in _lib.EXPORTS, n
    for n in REMOVED:
        assert n not in names, f"{n} is declared in include/dsdiff.h again"
        assert n not in _lib.EXPORTS, n


def test_loop_signatures_match_header():
    """Parameter count, scalar types and pointer sizes of the ctypes argtypes against the declaration, for every device loop and
    dsd_op_plms_step."""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsdiff.h")).read(), flags=re.S)
    L = _lib.lib()
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}
    for sym in LOOPS + ("dsd_op_plms_step",):
        assert sym in _lib.EXPORTS
        decl = re.search(r"\bint %s\((.*?)\);" % sym, code, flags=re.S)
        assert decl, sym
        params = [p.strip() for p in decl.group(1).split(",")]
        argtypes = getattr(L, sym).argtypes
        assert argtypes is not None and len(argtypes) == len(params), (sym, argtypes and len(argtypes), len(params))
        for p, a in zip(params, argtypes):                                    # scalars by type; every pointer is pointer-sized
            if "*" in p:
                assert C.sizeof(a) == C.sizeof(C.c_void_p), (sym, p)
            else:
                assert a is ctype[p.split()[0]], (sym, p, a)


def test_struct_layouts_match_header():
    # dsd_config: 3 + 1 + 8 + 8 + 1 + 8 + 7 int32 ; dsd_schedule: 5 int32 + float + 3 pointers
    assert C.sizeof(_lib.DsdConfig) == 4 * (3 + 1 + 8 + 8 + 1 + 8 + 7)
    assert C.sizeof(_lib.DsdSchedule) == 24 + 3 * C.sizeof(C.c_void_p)


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        return
    try:
        _lib.require_gpu(0)
    except _lib.DsdError as e:
        assert "device" in str(e).lower() or "hip" in str(e).lower()
    else:
        raise AssertionError("require_gpu must raise without a GPU")


def test_parameter_table_matches_reference_names():
    """Table-only handle (device = -1): names/shapes equal the reference state_dict stored in the golden fixture."""
    import json
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "model.npz"))
    for key in ("tiny", "tinyfilm"):
        params = json.loads(str(g[key + "_cfg"]))
        cfg = _lib.DsdConfig()
        cfg.in_channels, cfg.model_channels, cfg.out_channels = params["in_channels"], params["model_channels"], params["out_channels"]
        cm = params["channel_mult"]
        nrb = params["num_res_blocks"]
        nrb = [nrb] * len(cm) if isinstance(nrb, int) else nrb
        cfg.n_levels = len(cm)
        for i in range(len(cm)):
            cfg.channel_mult[i], cfg.num_res_blocks[i] = cm[i], nrb[i]
        ar = params["attention_resolutions"]
        cfg.n_attention_resolutions = len(ar)
        for i, a in enumerate(ar):
            cfg.attention_resolutions[i] = a
        cfg.num_heads = params.get("num_heads", -1)
        cfg.num_head_channels = params.get("num_head_channels", -1)
        cfg.num_heads_upsample = -1
        cfg.use_scale_shift_norm = int(params.get("use_scale_shift_norm", False))
        cfg.resblock_updown = int(params.get("resblock_updown", False))
        cfg.use_new_attention_order = int(params.get("use_new_attention_order", False))
        cfg.legacy = int(params.get("legacy", True))
        h = C.c_void_p()
        L = _lib.lib()
        _lib.check(L.dsd_create(C.byref(cfg), -1, C.byref(h)))
        got = {}
        name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        for i in range(L.dsd_param_count(h)):
            _lib.check(L.dsd_param_info(h, i, C.byref(name), shape, C.byref(ndim)))
            got[name.value.decode()] = tuple(shape[k] for k in range(ndim.value))
        L.dsd_destroy(h)
        ref = {n: tuple(s) for n, s in json.loads(str(g[key + "_params"]))}
        assert got == ref


def test_bad_config_is_rejected():
    cfg = _lib.DsdConfig()
    cfg.in_channels, cfg.model_channels, cfg.out_channels, cfg.n_levels = 3, 32, 1, 1
    cfg.channel_mult[0], cfg.num_res_blocks[0] = 1, 1
    cfg.num_heads, cfg.num_head_channels, cfg.num_heads_upsample = -1, 16, -1
    h = C.c_void_p()
    assert _lib.lib().dsd_create(C.byref(cfg), -1, C.byref(h)) != 0
    assert b"in_channels" in _lib.lib().dsd_last_error()


def test_vae_parameter_tables_match_reference_names():
    """Table-only VAE handles (device = -1): encoder + quant_conv and post_quant_conv + decoder carry exactly the
    parameter names / shapes of the reference's Encoder / Decoder / AutoencoderKL (tests/golden/vae.npz)."""
    import json
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "vae.npz"))
    L = _lib.lib()
    for key in ("small", "rgb"):
        dd = json.loads(str(g[key + "_cfg"]))
        ia = [dd["ch"], dd["out_ch"], dd["in_channels"], dd["resolution"], dd["z_channels"], 1, dd["embed_dim"], dd["num_res_blocks"], 1,
              len(dd["ch_mult"])] + dd["ch_mult"] + [len(dd["attn_resolutions"])] + dd["attn_resolutions"]
        got = {}
        for kind in (_lib.BLOCK_VAE_ENCODER, _lib.BLOCK_VAE_DECODER):
            h = C.c_void_p()
            arr = (C.c_int32 * len(ia))(*ia)
            _lib.check(L.dsd_block_create(kind, arr, len(ia), -1, C.byref(h)))
            name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
            for i in range(L.dsd_param_count(h)):
                _lib.check(L.dsd_param_info(h, i, C.byref(name), shape, C.byref(ndim)))
                got[name.value.decode()] = tuple(shape[k] for k in range(ndim.value))
            L.dsd_destroy(h)
        ref = {n: tuple(s) for n, s in json.loads(str(g[key + "_params"]))}
        assert got == ref


def test_plain_unet_parameter_table_matches_reference_names():
    """Table-only DSD_BLOCK_UNET handles carry exactly the reference UNetModel's state_dict (tests/golden/latent_unet.npz)."""
    import json
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "latent_unet.npz"))
    L = _lib.lib()
    for key in ("lu", "lu2"):
        p = json.loads(str(g[key + "_cfg"]))
        cm = p["channel_mult"]
        nrb = p["num_res_blocks"]
        nrb = [nrb] * len(cm) if isinstance(nrb, int) else nrb
        ar = p["attention_resolutions"]
        ia = [p["in_channels"], p["model_channels"], p["out_channels"], p.get("num_heads", -1), p.get("num_head_channels", -1), -1,
              int(p.get("use_scale_shift_norm", False)), int(p.get("resblock_updown", False)),
              int(p.get("use_new_attention_order", False)), int(p.get("legacy", True)), len(cm)] + cm + nrb + [len(ar)] + ar
        h = C.c_void_p()
        _lib.check(L.dsd_block_create(_lib.BLOCK_UNET, (C.c_int32 * len(ia))(*ia), len(ia), -1, C.byref(h)))
        got = {}
        name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        for i in range(L.dsd_param_count(h)):
            _lib.check(L.dsd_param_info(h, i, C.byref(name), shape, C.byref(ndim)))
            got[name.value.decode()] = tuple(shape[k] for k in range(ndim.value))
        L.dsd_destroy(h)
        assert got == {n: tuple(s) for n, s in json.loads(str(g[key + "_params"]))}


def test_no_product_kernel_spills_or_uses_scratch():
    """Every gfx950 kernel embedded in the shipped library is read back (AMDGPU metadata note of each code object,
    tools/kernel_resources.py): no kernel on a product path may spill registers or use scratch memory.  Besides the cost, two
    kernels keep registers that an inline-asm load is still filling live across compiler-scheduled code: a spill
    of such a register is silent corruption (seen once, round 3: attention16_dma_kernel under its 128-register cap).
    Exempt: the diagnostic what-if instantiations of the half-precision GEMM that keep every fragment in registers on purpose
    (timing only, never on a product path) and the scalar-register spills of the opt-in Winograd kernel."""
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels()
    assert len(ks) > 150                                   # the parser sees the library's kernels at all
    names = " ".join(k["name"] for k in ks)
    for must in ("conv_split_ad_kernel", "attention16_dma_kernel", "gemm16_kernel", "conv_out1_kernel", "sampler_update_kernel"):
        assert must in names, must
    bad = []
    for k in ks:
        diag_gemm = re.search(r"gemm16_kernelIDF16_Li0ELi(2|3|7|15|34)E", k["name"]) is not None
        if diag_gemm:
            continue
        if k["scratch"] or k["vgpr_spills"] or (k["sgpr_spills"] and "conv_wino_kernel" not in k["name"]):
            bad.append(k)
    assert not bad, bad
    # the 8-wave attention kernel must fit two workgroups per CU
    a8 = [k for k in ks if "attention16_dma_kernel" in k["name"] and "Li0ELi8ELi1E" in k["name"]]
    assert a8 and all(k["vgpr"] <= 128 for k in a8), a8


def test_unet_spatial_transformer_parameter_table_matches_the_reference_block():
    """UNetModel(use_spatial_transformer=True): the reference's constructor cannot run here on that branch (it imports omegaconf),
    so the parameter table of a table-only DSD_BLOCK_UNET handle is pinned part by part: every attention slot must carry exactly
    the names and shapes of the reference's own SpatialTransformer(64, 4, 16, depth=1, context_dim=[32], use_linear=True)
    (tests/golden/xattn.npz `spatial_tf_lin_params`, generated from the imported reference), under the slot's prefix; everything
    else must equal the table of the same network without the transformer, minus its AttentionBlock entries."""
    import json
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "xattn.npz"))
    ref = {n: tuple(s) for n, s in json.loads(str(g["spatial_tf_lin_params"]))}
    L = _lib.lib()

    def table(extra):
        ia = [4, 64, 4, 4, -1, -1, 0, 0, 0, 0, 2, 1, 2, 1, 1, 1, 1] + extra     # model_channels 64, mult (1, 2), attention at ds 1
        h = C.c_void_p()
        _lib.check(L.dsd_block_create(_lib.BLOCK_UNET, (C.c_int32 * len(ia))(*ia), len(ia), -1, C.byref(h)))
        got = {}
        name, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        for i in range(L.dsd_param_count(h)):
            _lib.check(L.dsd_param_info(h, i, C.byref(name), shape, C.byref(ndim)))
            got[name.value.decode()] = tuple(shape[k] for k in range(ndim.value))
        L.dsd_destroy(h)
        return got

    plain, st = table([]), table([1, 1, 32, 1])
    slots = sorted({n.rsplit(".qkv.weight", 1)[0] for n in plain if n.endswith(".qkv.weight")})
    assert "input_blocks.1.1" in slots and "middle_block.1" in slots
    slots64 = [s for s in slots if plain[s + ".norm.weight"] == (64,)]          # 64-channel slots: heads 4 x dim_head 16 = the fixture
    assert slots64
    for s in slots64:
        mine = {n[len(s) + 1:]: shp for n, shp in st.items() if n.startswith(s + ".")}
        assert mine == ref, s
    rest_plain = {n: shp for n, shp in plain.items() if not any(n.startswith(s + ".") for s in slots)}
    rest_st = {n: shp for n, shp in st.items() if not any(n.startswith(s + ".") for s in slots)}
    assert rest_plain == rest_st
    for s in slots:                                                              # 128-channel slots: the same sub-names, wider
        assert f"{s}.transformer_blocks.0.attn2.to_k.weight" in st and st[f"{s}.transformer_blocks.0.attn2.to_k.weight"][1] == 32
        assert f"{s}.qkv.weight" not in st


def test_conv_planner_lane_hint():
    """dsd_conv_plan (host-side, no GPU): a 320 -> 320 3x3 layer on a 128 x 128 map at batch 1 alone takes 96-column tiles (256
    workgroups fill the chip once); planned for a stream-lane region — three siblings beside it — it takes the 256-row tile
    with 160 columns, the shape the tap-reuse kernel with the fused GroupNorm runs on.  Layers that fill
    the chip on their own are planned the same either way."""
    L = _lib.lib()

    def plan(shape, lanes):
        st, nt, ks = C.c_int(), C.c_int(), C.c_int()
        sb = C.c_uint64()
        _lib.check(L.dsd_conv_plan(*shape, 3, 1, 2 | (256 if lanes else 0), C.byref(st), C.byref(nt), C.byref(ks), C.byref(sb)))
        return st.value, nt.value, ks.value

    alone, in_lane = plan((1, 128, 128, 320, 320), False), plan((1, 128, 128, 320, 320), True)
    assert alone[1] < 5 and alone[2] == 1
    assert in_lane == (2, 5, 1)
    for shape in ((16, 256, 256, 320, 320), (16, 128, 128, 320, 320), (1, 256, 256, 320, 320)):
        assert plan(shape, False) == plan(shape, True) == (2, 5, 1), shape
