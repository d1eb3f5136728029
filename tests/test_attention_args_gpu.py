"""The attention launch arguments that only the networks set (GPU), through dsd_op_attention: Tq != Tk with separate q / k / v
buffers and scale_s (CrossAttention), scale_q alone (the DiT), the fused [N,T,3C] buffer in both head orders, and an output row
stride wider than heads * d — for both fp32-grade kernels (split 0: fp32 MFMA, 1: bf16x6) against float64,
softmax((q scale_q)(k scale_k)^T scale_s) v per head, at the project's attention bar of 3e-6 rel-L2
(test_ops_gpu.py::test_qkv_attention_vs_oracle).  Layouts move addresses, not arithmetic: the fused runs must be bit-identical
to the separate-buffer run with the same scales, and whatever lies outside the written columns keeps its sentinel."""
import pytest
import torch

from util import rel_l2

pytestmark = pytest.mark.gpu

TOL = 3e-6
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    from diffusion_models_dsdiff_amd import ops as m, _lib
    _lib.require_gpu(0)
    return m


def make(case, seed=0):
    N, Tq, Tk, heads, d = case
    g = torch.Generator().manual_seed(sum(case) + seed)
    return (torch.randn(N, Tq, heads, d, generator=g), torch.randn(N, Tk, heads, d, generator=g),
            torch.randn(N, Tk, heads, d, generator=g))


def ref64(q, k, v, sq, sk, ss):
    """[N, Tq, heads, d] float64"""
    s = torch.einsum("nqhd,nkhd->nhqk", q.double() * sq, k.double() * sk) * ss
    return torch.einsum("nhqk,nkhd->nqhd", torch.softmax(s, dim=-1), v.double())


def sentinel(n):
    return (torch.arange(n, dtype=torch.float32, device="cuda") % 1021) * 0.25 + 1000.0


def run(ops, case, q, k, v, scales, split, form="separate", ldo_extra=0):
    """form: separate (contiguous q / k / v, ld = heads * d, hs = d) | fused_new ([N,T,3C] as q | k | v, hs = d) | fused_legacy
    ([N,T,3C] as heads x (q, k, v), hs = 3d).  -> ([N, Tq, heads, d] result, everything outside it intact)"""
    N, Tq, Tk, heads, d = case
    C = heads * d
    ldo = C + ldo_extra
    buf0 = sentinel(GUARD + N * Tq * ldo + GUARD)
    buf = buf0.clone()
    out = buf[GUARD:GUARD + N * Tq * ldo].view(N, Tq, ldo)
    if form == "separate":
        qb, kb, vb = (t.reshape(t.shape[0], t.shape[1], C).contiguous().cuda() for t in (q, k, v))
        ld, hs = (C, C, C), (d, d, d)
    else:
        assert Tq == Tk
        if form == "fused_new":
            f = torch.cat([t.reshape(N, Tq, C) for t in (q, k, v)], dim=2)
            off, h = (0, C, 2 * C), d
        else:
            f = torch.stack([q, k, v], dim=3).reshape(N, Tq, 3 * C)      # [N, T, heads, 3, d]
            off, h = (0, d, 2 * d), 3 * d
        f = f.contiguous().cuda().view(-1)
        qb, kb, vb = f[off[0]:], f[off[1]:], f[off[2]:]
        ld, hs = (3 * C,) * 3, (h,) * 3
    ops.attention(qb, kb, vb, out, N, Tq, Tk, heads, d, ld[0], ld[1], ld[2], ldo, hs[0], hs[1], hs[2], scale_q=scales[0],
                  scale_k=scales[1], scale_s=scales[2], split=split)
    torch.cuda.synchronize()
    res = out[..., :C].reshape(N, Tq, heads, d).clone()
    chk = buf.clone()
    chk[GUARD:GUARD + N * Tq * ldo].view(N, Tq, ldo)[..., :C] = buf0[GUARD:GUARD + N * Tq * ldo].view(N, Tq, ldo)[..., :C]
    return res, torch.equal(chk, buf0)


def forms(d):
    """the networks' scalings: CrossAttention (scale_s), the DiT (scale_q), QKVAttention (scale_q = scale_k)"""
    return {"cross": (1.0, 1.0, d ** -0.5), "dit": (d ** -0.5, 1.0, 1.0), "qkv": (d ** -0.25, d ** -0.25, 1.0)}


CASES = [
    (2, 16, 9, 4, 16), (2, 16, 5, 4, 16),           # the cross-attention fixture's family
    (1, 4096, 77, 8, 40),                           # the latent U-Net's cross-attention: zero-padded head dim, ragged key tile
    (2, 130, 1, 2, 64),                             # a single key
    (1, 33, 31, 1, 4),                              # smallest head dim, fewer keys than one sub-tile
    (1, 70, 32, 2, 32), (1, 70, 33, 2, 32), (1, 70, 64, 2, 32), (1, 70, 65, 2, 96),   # sub-tile and stage boundaries
    (1, 129, 65, 3, 88), (1, 64, 96, 2, 112),       # attention_split_kernel<6> / <7>, attention_kernel<3> / <4>
    (1, 200, 200, 1, 100),
    (2, 70, 70, 2, 32),                             # Tq == Tk with two heads: the two fused head orders differ
]


@pytest.mark.parametrize("case", CASES)
def test_attention_forms_vs_fp64(ops, case):
    N, Tq, Tk, heads, d = case
    q, k, v = make(case)
    for fname, sc in forms(d).items():
        ref = ref64(q, k, v, *sc)
        for split in (0, 1):
            a, intact = run(ops, case, q, k, v, sc, split)
            err = rel_l2(a, ref)
            print(f"attention {case} {fname} split={split}: rel-L2 vs fp64 {err:.3e}")
            assert err < TOL, (case, fname, split, err)
            assert intact, (case, fname, split)
            if Tq == Tk:     # the same data as one fused buffer, both head orders: addresses only
                for form in ("fused_new", "fused_legacy"):
                    f, intact = run(ops, case, q, k, v, sc, split, form=form)
                    assert torch.equal(f, a), (case, fname, split, form, int((f != a).sum()))
                    assert intact, (case, fname, split, form)


@pytest.mark.parametrize("case", [(2, 16, 9, 4, 16), (1, 129, 65, 3, 88), (2, 70, 70, 2, 32)])
def test_attention_wide_output_rows(ops, case):
    """ldo = heads * d + 32: the columns beyond heads * d keep their sentinel, the result is the ldo = heads * d run's."""
    N, Tq, Tk, heads, d = case
    q, k, v = make(case, seed=1)
    sc = forms(d)["cross"]
    ref = ref64(q, k, v, *sc)
    for split in (0, 1):
        a, intact = run(ops, case, q, k, v, sc, split, ldo_extra=32)
        err = rel_l2(a, ref)
        print(f"attention {case} ldo+32 split={split}: rel-L2 vs fp64 {err:.3e}")
        assert err < TOL, (case, split, err)
        assert intact, (case, split)
        assert torch.equal(a, run(ops, case, q, k, v, sc, split)[0])
        if Tq == Tk:
            assert torch.equal(a, run(ops, case, q, k, v, sc, split, form="fused_legacy", ldo_extra=32)[0])


@pytest.mark.parametrize("case,spike", [((1, 130, 100, 1, 32), 97), ((1, 130, 70, 2, 96), 68), ((1, 40, 77, 2, 40), 76)])
def test_attention_running_max_last_partial_tile(ops, case, spike):
    """Tq != Tk and one key far above the rest in the last, partial key tile: the running maximum moves there and everything
    accumulated before is rescaled (KEYS is 64 for d <= 64 and 32 above)."""
    N, Tq, Tk, heads, d = case
    q, k, v = make(case, seed=2)
    k[:, spike] *= 30.0
    for fname, sc in forms(d).items():
        ref = ref64(q, k, v, *sc)
        for split in (0, 1):
            a, intact = run(ops, case, q, k, v, sc, split)
            err = rel_l2(a, ref)
            print(f"attention {case} spike at key {spike} {fname} split={split}: rel-L2 vs fp64 {err:.3e}")
            assert err < TOL, (case, fname, split, err)
            assert intact
