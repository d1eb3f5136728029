"""The references of test_tail_kernels_gpu.py without a GPU: every case builder runs, the float64 and float32 evaluations of
each listed case exist and agree to float32 accuracy, and the properties the GPU tests lean on hold for the chosen inputs."""
import os
import re

import pytest
import torch

import tail_cases as TC
from tail_cases import maxabs, three

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_kinds_match_header():
    from diffusion_models_dsdiff_amd import _lib
    src = open(os.path.join(ROOT, "include", "dsdiff.h")).read()
    body = re.search(r"enum \{ (DSD_TAIL_SE_SCALE.*?) \};", src, flags=re.S).group(1)
    names = [n.strip().split(" ")[0] for n in body.split(",")]
    assert names[-1] == "DSD_TAIL_NKINDS"
    assert [n[len("DSD_TAIL_"):].lower() for n in names[:-1]] == list(_lib.TAIL_KINDS)


def test_wrap_counts():
    def fact(n):
        return [d for d in range(2, int(n ** 0.5) + 1) if n % d == 0]
    assert fact(TC.WRAP) == []                      # a prime: no shaped kernel can have exactly this count
    N, C, HW = TC.TRANSPOSE_WRAP
    assert TC.CAP < N * C * HW < TC.CAP + 65536 and (N * C * HW) % 256
    N, C, H, W, p = TC.PATCH_WRAP
    assert TC.CAP < N * C * H * W < TC.CAP + 65536 and H % p == 0 and W % p == 0
    r, i = TC.GEGLU_WRAP
    assert TC.CAP < r * i < TC.CAP + 65536
    for N, H, W, C in (TC.UPSAMPLE_WRAP,):
        assert TC.CAP < N * 4 * H * W * (C // 4) < TC.CAP + 65536
    N, H, W, C = TC.AVGPOOL_WRAP
    assert TC.CAP < N * (H // 2) * (W // 2) * (C // 4) < TC.CAP + 65536 and H % 2 == 0 and W % 2 == 0
    N, T, C = TC.GATED_WRAP
    assert TC.CAP < N * T * C // 4 < TC.CAP + 65536
    assert TC.AVG_WRAP4 % (11 * 13) == 0


def test_data_movement_references():
    x = TC.randn((2, 3, 8, 12), 1)
    t = TC.patchify_ref(x, 2)                                    # (c, ph, pw) inside a token, tokens row-major over (th, tw)
    assert t.shape == (2, 24, 12) and float(t[1, 1 * 6 + 2, 2 * 4 + 1 * 2 + 0]) == float(x[1, 2, 1 * 2 + 1, 2 * 2 + 0])
    tok = TC.randn((2, 4 * 6, 2 * 2 * 3), 2)
    img = TC.unpatchify_ref(tok, 3, 4, 6, 2)                     # (ph, pw, c) inside a token
    assert img.shape == (2, 3, 8, 12) and float(img[1, 2, 3 * 2 + 1, 5 * 2 + 0]) == float(tok[1, 3 * 6 + 5, (1 * 2 + 0) * 3 + 2])
    u = TC.upsample2_ref(TC.randn((1, 2, 3, 4), 3))
    assert u.shape == (1, 4, 6, 4) and torch.equal(u[:, 1::2, 0::2], u[:, 0::2, 1::2])


@pytest.mark.parametrize("bf16", [False, True])
def test_cast_vector_covers_the_edges(bf16):
    dt = torch.bfloat16 if bf16 else torch.float16
    v = TC.cast_vector(bf16)
    r = v.to(dt)
    one_ulp = 2.0 ** -(7 if bf16 else 10)
    assert float(r[0]) == 1.0 and float(r[1]) == 1.0 + 2 * one_ulp          # ties go to the even neighbour, down and up
    assert bool(torch.isinf(r).any()) and bool(torch.isnan(r).any()) and bool((r == 0).any())
    assert float(r[8]) == float(v[8]) and bool(torch.isinf(r[9])) and not bool(torch.isinf(v[9]))   # largest finite; first to inf
    if not bf16:
        sub = (r != 0) & (r.float().abs() < 2.0 ** -14)
        assert bool(sub.any()) and bool(((v != 0) & (r == 0)).any())        # subnormal results and flushed-by-rounding ones
    assert TC.same_bits(r, v.to(dt)) and not TC.same_bits(r, (-v).to(dt))


def test_every_reference_evaluates_in_both_precisions():
    n = 0
    pool = TC.act_pool()
    for fn, args in ([(TC.gelu_tanh_ref, (pool,))] + [(TC.geglu_ref, (TC.geglu_input(r, i),)) for r, i in TC.GEGLU_SHAPES]
                     + [(lambda t, s=s: TC.softmax_ref(t, s), (TC.softmax_input(r, c, s),)) for r, c in TC.SOFTMAX_SHAPES for s in TC.SOFTMAX_SCALES]
                     + [(lambda a, g, b, e=e: TC.layer_norm_ref(a, g, b, e), TC.layer_norm_input(r, c, k)) for r, c in TC.LAYER_NORM_SHAPES for e, k in TC.LAYER_NORM_KINDS]
                     + [(lambda a, m, c=c: TC.ln_mod_ref(a, m, c, False, 1e-6), TC.ln_mod_input(n_, t, c, False)) for n_, t, c in TC.LN_MOD_SHAPES]
                     + [(TC.se_ref, TC.se_input(*s)) for s in TC.SE_SHAPES]
                     + [(lambda *s, d=d: TC.avg_ref(list(s), d, True), TC.avg_sources(k, c, b, 5)) for k, d, c, _, b in TC.AVG_SILU_CASES]):
        ref64, cpu32 = three(fn, *args)
        assert ref64.dtype == torch.float64 and cpu32.dtype == torch.float32 and ref64.shape == cpu32.shape
        assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(cpu32).all())
        assert maxabs(cpu32.double() - ref64) <= 1e-3 * max(1.0, maxabs(ref64))
        n += 1
    assert n == 1 + 3 + 18 + 24 + 4 + 4 + 4


def test_layer_norm_offset_rows_are_what_they_claim():
    x, _, _ = TC.layer_norm_input(3, 320, "offset")
    assert maxabs(x.double().mean(1) - 1000.0) < 0.3 and maxabs(x.double().std(1) - 1.0) < 0.2


@pytest.mark.parametrize("bf16", [False, True])
def test_ln_modulate16_cap_holds_for_the_reference(bf16):
    """at most 1 element in 1000 of the float32 evaluation, rounded once, is more than one 16-bit ulp from the rounded float64
    result: the cap test_ln_modulate16 puts on the kernel is one the reference's own arithmetic meets"""
    dt = torch.bfloat16 if bf16 else torch.float16
    for i, C in enumerate(TC.LN16_WIDTHS):
        N, T = (5, 1) if i % 2 == 0 else (1, 5)
        x, mod = TC.ln_mod_input(N, T, C, aligned=True)
        stride, sh, sc = TC.ln_mod_layout(C, True)
        assert stride % 4 == 0 and sh % 4 == 0 and sc % 4 == 0 and sh != sc and max(sh, sc) + C <= stride
        ref64, cpu32 = three(lambda a, m: TC.ln_mod_ref(a, m, C, True, 1e-6), x, mod)
        assert TC.frac_beyond_one_ulp(cpu32.to(dt), ref64.to(dt), bf16) <= 1e-3
    one = torch.tensor([1.0, 1.0, 0.0, 3.0], dtype=torch.float64)
    assert TC.ulp16(one, bf16).tolist() == [2.0 ** -(7 if bf16 else 10)] * 2 + [2.0 ** ((-126 - 7) if bf16 else -24), 2.0 ** -(6 if bf16 else 9)]
    a = torch.tensor([1.0, 1.0 + 2.0 ** -6, 2.0], dtype=dt)
    b = torch.tensor([1.0, 1.0, 2.0], dtype=dt)
    assert abs(TC.frac_beyond_one_ulp(a, b, bf16) - 1 / 3) < 1e-12


def test_one_rounding_inputs_are_exact_in_float32():
    x = TC.int_blocks(1000003, 3, 512)
    assert x.numel() == 1000003 and bool((x == x.round()).all()) and maxabs(x) <= 512 + 45
    assert not torch.equal(x[:62501], x[62501:125002])            # the sixteen copies differ
