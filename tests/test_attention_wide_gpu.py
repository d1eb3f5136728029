"""The wide-head attention kernels (csrc/attention_wide.hip: 128 < d <= 512, the head dim sliced across the four waves of a
workgroup) through dsd_op_attention, with the harness of test_attention_args_gpu.py: sentinel guard around the output, the
networks' three scale forms, both fp32-grade arithmetics (split 0: fp32 MFMA, 1: bf16x6), float64 reference, the project's
attention bar of 3e-6 rel-L2.  (Plain fp32 attention on these inputs is 3.6e-7 .. 8.5e-7 from float64 over d = 132 .. 512, so the
bar holds for the arithmetic itself with more than 3x margin: an excess is a kernel defect.)

What can go wrong only here: a slice boundary inside a head (d = 132 and 160 do not fill four equal slices; one or two waves
hold nothing but padding), the four waves of a workgroup disagreeing on the running maximum (their output slices would be
scaled differently), and the clamped K / V addresses of the padded part."""
import pytest
import torch

from test_attention_args_gpu import TOL, forms, make, ref64, run
from util import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from diffusion_models_dsdiff_amd import ops as m, _lib
    _lib.require_gpu(0)
    return m


CASES = [
    (1, 33, 31, 1, 132),            # the smallest wide head; fewer keys than a sub-tile; wave 3 all padding, wave 2 four columns
    (1, 70, 65, 2, 160),            # the SD-v1 head
    (1, 64, 96, 2, 200),
    (2, 130, 1, 1, 256),            # a single key
    (1, 129, 33, 1, 388),           # 96-wide slices (three d tiles per wave), ragged
    (1, 70, 32, 1, 512), (1, 70, 64, 1, 512),
    (1, 256, 77, 8, 160),           # the U-Net's real cross-attention at its 1280-channel levels
    (1, 1024, 1024, 1, 512),        # the sdv1 VAE's AttnBlock at 256 x 256
    (2, 70, 70, 2, 160), (1, 200, 200, 1, 512),     # Tq == Tk: the two fused head orders
]


@pytest.mark.parametrize("case", CASES)
def test_wide_attention_forms_vs_fp64(ops, case):
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


@pytest.mark.parametrize("case", [(2, 70, 70, 2, 160)])
def test_wide_attention_wide_output_rows(ops, case):
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
        assert torch.equal(a, run(ops, case, q, k, v, sc, split, form="fused_legacy", ldo_extra=32)[0])


@pytest.mark.parametrize("case,spike", [((1, 130, 100, 1, 160), 97), ((1, 40, 77, 1, 512), 76)])
def test_wide_attention_running_max_last_partial_tile(ops, case, spike):
    """One key far above the rest in the last, partial key tile: the running maximum moves there and everything accumulated
    before is rescaled — by the same factor in all four waves, or the slices of an output row disagree."""
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


@pytest.mark.parametrize("d", [516, 130])
def test_head_dim_limit_is_named(ops, d):
    """An argument check: nothing is launched.  Above 512, or where d % 4 != 0, the error names the limit."""
    from diffusion_models_dsdiff_amd._lib import DsdError
    ld = (d + 3) // 4 * 4      # rows stay 16-byte aligned: only the head dim is at fault
    qb, kb, vb = (torch.zeros(8, ld, device="cuda") for _ in range(3))
    out = torch.zeros(8, ld, device="cuda")
    for split in (0, 1):
        with pytest.raises(DsdError) as e:
            ops.attention(qb, kb, vb, out, 1, 8, 8, 1, d, ld, ld, ld, ld, d // 4 * 4, d // 4 * 4, d // 4 * 4, split=split)
        assert "512" in str(e.value) and "head dim" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0
