"""Kernel-level tests (GPU) of the small kernels around the convolutions and the transformer blocks: all of csrc/misc.hip except
linear and timestep_embedding, layer_norm (csrc/norm.hip), cast16 / uncast16 / ln_modulate16 (csrc/gemm16.hip).  Each kernel is
launched alone through dsd_op_tail, exactly as the networks launch it, and compared with plain torch on the CPU (tail_cases.py).

Every output lies between two 256-byte guard bands of a sentinel pattern that must survive; an output that is not written in
place starts as NaN; the read-only operands of the in-place kernels must come back unchanged.

Three kinds of comparison:
  * data movement (transposes, upsample2, patchify, unpatchify, embed_add without `a`), the one-add kernels (add2,
    add_rows_broadcast, embed_add) and the casts: bit-exact.  Channel order of a token: patchify (c, ph, pw) — Conv2d weight
    order, F.unfold's own; unpatchify (ph, pw, c) — DiT.unpatchify.
  * one-rounding arithmetic (gated_residual, avgpool2, avg_into without activation): an element-wise bound from 2^-24 per fp32
    operation against float64, stated at each test.
  * transcendental and reduction kernels: maxabs(got - ref64) <= 4 maxabs(cpu32 - ref64) + 4 * 2^-24 maxabs(ref64), cpu32 the
    same torch expression in float32 on the CPU (ln_modulate16: rounded once to the 16-bit type, floor 2^-11 / 2^-8, and at
    most 1 element in 1000 more than one 16-bit ulp from cpu32).  Each case prints err_kernel / err_cpu32.

Grid-stride wrap: one case per kernel with a capped grid, the cap (65535 blocks of 256; 256*32 blocks in avg_into) plus a ragged
tail, so that some threads take a second iteration.  65535*256 + 1027 is a prime: the flat kernels (gelu_tanh, add2, cast16,
uncast16) run exactly that count, the kernels whose count is a product of dimensions the nearest convenient count above it
(tail_cases.py: *_WRAP).  The big one-rounding wrap cases use small integers as inputs: the float32 evaluation of the reference
is then exact, i.e. it is the float64 value, and no gigabyte-sized float64 tensor has to be formed.

ln_modulate's listed shape (2, 6, 1152) has N*T = 12, a multiple of 4; the other three leave the last block partly empty.

Measured err_kernel / err_cpu32 on an MI355X, the maximum over a kernel's cases (1.00: the kernel's worst element is as far
from float64 as the CPU's own float32 evaluation, usually bit-identical):
    avg_into + SiLU   1.00
    gelu_tanh         1.00 (the 16.8 M-element wrap case too)
    geglu             1.00 (likewise)
    softmax_rows      2.07
    layer_norm        2.51 (rows of mean 1000; 2.05 on ordinary rows)
    ln_modulate       1.02
    ln_modulate16     1.00 (fp16 and bf16, every width)
    se_scale          3.31 at (2, 9, 260, 16), 2.21 at (3, 35, 320, 20), 1.00 at the other two shapes
se_scale comes closest to the 4: its two small matrix products are summed by one thread per output in index order, torch's in
blocks, and w2 is large on purpose (saturated gates), which multiplies whatever the hidden layer's sums differ by.  layer_norm's
2.5 is on rows of mean 1000, where the result inherits the rounding of the mean (2^-24 * 1000 against a deviation of 1) and the
kernel and torch add the row in different orders.
"""
import pytest
import torch

import tail_cases as TC
from tail_cases import U24, maxabs, three

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from diffusion_models_dsdiff_amd import ops as m, _lib
    _lib.require_gpu(0)
    return m


def cu(t):
    return t.cuda().contiguous()


class Band:
    """n elements of `dtype` on the device between two guard bands of 256 bytes (64 floats) holding a sentinel pattern.
    fill: the initial contents (in-place kernels, partly written outputs); None: NaN."""

    def __init__(self, n, dtype=torch.float32, fill=None):
        g = 256 // torch.empty((), dtype=dtype).element_size()
        self.n, self.g = n, g
        self.pat = ((torch.arange(g, dtype=torch.float32, device="cuda") % 1021) * 0.25 + 1000.0).to(dtype)
        self.buf = torch.empty(n + 2 * g, dtype=dtype, device="cuda")
        self.buf[:g] = self.pat
        self.buf[g + n:] = self.pat.flip(0)
        self.mid = self.buf[g:g + n]
        if fill is None:
            self.mid.fill_(NAN)
        else:
            self.mid.copy_(fill.reshape(-1))

    def intact(self):
        torch.cuda.synchronize()
        return torch.equal(self.buf[:self.g], self.pat) and torch.equal(self.buf[self.g + self.n:], self.pat.flip(0))

    def cpu(self, shape=None):
        t = self.mid.cpu()
        return t if shape is None else t.reshape(shape)


def check3(name, got, ref64, cpu32, floor=U24):
    """the transcendental / reduction tolerance of the module docstring; prints the measured ratio"""
    ek, e32 = maxabs(got.double() - ref64), maxabs(cpu32.double() - ref64)
    tol = 4 * e32 + 4 * floor * maxabs(ref64)
    ratio = ek / e32 if e32 > 0 else (0.0 if ek == 0 else float("inf"))
    print(f"RATIO {name}: err_kernel {ek:.3e} err_cpu32 {e32:.3e} ratio {ratio:.2f} tol {tol:.3e}")
    assert ek <= tol, (name, ek, e32, tol)


def raises(ops, text, *call):
    from diffusion_models_dsdiff_amd._lib import DsdError
    with pytest.raises(DsdError) as e:
        ops.tail(*call)
    assert text in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ pure data movement
def run_transposes(ops, N, C, HW, seed):
    x = TC.randn((N, C, HW), seed)
    want = TC.nchw_to_nhwc_ref(x)
    dx = cu(x)
    y = Band(x.numel())
    ops.tail("nchw_to_nhwc", [dx, y.mid], [N, C, HW])
    assert y.intact() and torch.equal(y.cpu(want.shape), want)
    assert torch.equal(dx.cpu(), x)
    back = Band(x.numel())
    ops.tail("nhwc_to_nchw", [y.mid, back.mid], [N, C, HW])
    assert back.intact() and y.intact() and torch.equal(back.cpu(x.shape), x)      # the round trip is the identity
    # nhwc_to_nchw on an input of its own
    z = TC.randn((N, HW, C), seed + 1)
    out = Band(z.numel())
    ops.tail("nhwc_to_nchw", [cu(z), out.mid], [N, C, HW])
    assert out.intact() and torch.equal(out.cpu((N, C, HW)), z.permute(0, 2, 1).contiguous())


@pytest.mark.parametrize("shape", TC.TRANSPOSE_SHAPES)
def test_transposes(ops, shape):
    run_transposes(ops, *shape, seed=100)


def test_transposes_wrap(ops):
    N, C, HW = TC.TRANSPOSE_WRAP
    assert N * C * HW > TC.CAP and (N * C * HW) % 256
    run_transposes(ops, N, C, HW, seed=101)


def run_upsample2(ops, N, H, W, C, seed):
    x = TC.randn((N, H, W, C), seed)
    want = TC.upsample2_ref(x)
    y = Band(want.numel())
    ops.tail("upsample2", [cu(x), y.mid], [N, H, W, C])
    assert y.intact() and torch.equal(y.cpu(want.shape), want)


@pytest.mark.parametrize("shape", TC.UPSAMPLE_SHAPES)
def test_upsample2(ops, shape):
    run_upsample2(ops, *shape, seed=110)


def test_upsample2_wrap(ops):
    N, H, W, C = TC.UPSAMPLE_WRAP
    assert C == 4 and N * 4 * H * W > TC.CAP and (N * 4 * H * W) % 256
    run_upsample2(ops, N, H, W, C, seed=111)


def run_patch(ops, N, C, H, W, p, seed):
    h, w = H // p, W // p
    x = TC.randn((N, C, H, W), seed)
    want = TC.patchify_ref(x, p)                       # [N, h w, C p p], channels (c, ph, pw)
    y = Band(x.numel())
    ops.tail("patchify", [cu(x), y.mid], [N, C, H, W, p])
    assert y.intact() and torch.equal(y.cpu(want.shape), want)
    t = TC.randn((N, h * w, p * p * C), seed + 1)      # channels (ph, pw, c)
    want = TC.unpatchify_ref(t, C, h, w, p)
    img = Band(t.numel())
    ops.tail("unpatchify", [cu(t), img.mid], [N, C, h, w, p])
    assert img.intact() and torch.equal(img.cpu(want.shape), want)


@pytest.mark.parametrize("shape", TC.PATCH_SHAPES)
def test_patchify_unpatchify(ops, shape):
    run_patch(ops, *shape, seed=120)


def test_patchify_unpatchify_wrap(ops):
    N, C, H, W, p = TC.PATCH_WRAP
    assert N * C * H * W > TC.CAP and (N * C * H * W) % 256 and H // p != W // p
    run_patch(ops, N, C, H, W, p, seed=121)


@pytest.mark.parametrize("N,C,K", [(1, 1, 1), (3, 5, 7), (5, 257, 10), (2, 768, 4)])
def test_embed_add(ops, N, C, K):
    table, a = TC.randn((K, C), 130), TC.randn((N, C), 131)
    idx = torch.randint(0, K, (N,), generator=TC.gen(132))
    idx[0] = K - 1
    dt, di = cu(table), cu(idx)
    y = Band(N * C)
    ops.tail("embed_add", [None, dt, di, y.mid], [N, C])                            # a == nullptr: a lookup, bit-exact
    assert y.intact() and torch.equal(y.cpu((N, C)), table[idx])
    y = Band(N * C)
    ops.tail("embed_add", [cu(a), dt, di, y.mid], [N, C])                           # one add
    assert y.intact() and torch.equal(y.cpu((N, C)), a + table[idx])
    y = Band(N * C, fill=a)
    ops.tail("embed_add", [y.mid, dt, di, y.mid], [N, C])                           # in place on a, as the networks call it
    assert y.intact() and torch.equal(y.cpu((N, C)), a + table[idx])
    assert torch.equal(dt.cpu(), table) and torch.equal(di.cpu(), idx)


# ------------------------------------------------------------------------------------------------ one add: bit-exact
def run_add2(ops, n, seed):
    a, b = TC.randn((n,), seed), TC.randn((n,), seed + 1, 3.0)
    da, db = cu(a), cu(b)
    y = Band(n)
    ops.tail("add2", [da, db, y.mid], [n])
    assert y.intact() and torch.equal(y.cpu(), a + b)
    y = Band(n, fill=a)
    ops.tail("add2", [y.mid, db, y.mid], [n])                                       # in place on a, as the networks call it
    assert y.intact() and torch.equal(y.cpu(), a + b) and torch.equal(db.cpu(), b) and torch.equal(da.cpu(), a)


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_add2(ops, n):
    run_add2(ops, n, 140)


def test_add2_wrap(ops):
    run_add2(ops, TC.WRAP, 141)


def run_add_rows(ops, N, TCn, seed):
    x, pos = TC.randn((N, TCn), seed), TC.randn((TCn,), seed + 1)
    dp = cu(pos)
    y = Band(N * TCn, fill=x)
    ops.tail("add_rows_broadcast", [y.mid, dp], [N, TCn])
    assert y.intact() and torch.equal(y.cpu((N, TCn)), x + pos[None]) and torch.equal(dp.cpu(), pos)


@pytest.mark.parametrize("N,TCn", [(1, 1), (3, 35), (2, 771), (5, 256)])
def test_add_rows_broadcast(ops, N, TCn):
    run_add_rows(ops, N, TCn, 150)


def test_add_rows_broadcast_wrap(ops):
    N, TCn = 3, 5592663                                                             # 16777989 = CAP + 1029
    assert N * TCn > TC.CAP and (N * TCn) % 256
    run_add_rows(ops, N, TCn, 151)


# ------------------------------------------------------------------------------------------------ casts: bit-exact
def run_casts(ops, n, bf16):
    dt = torch.bfloat16 if bf16 else torch.float16
    x = TC.tiled(TC.cast_vector(bf16), n)
    want = x.to(dt)
    dx = cu(x)
    y = Band(n, dtype=dt, fill=torch.zeros(n, dtype=dt))
    ops.tail("cast16", [dx, y.mid], [n, int(bf16)])
    assert y.intact() and TC.same_bits(y.cpu(), want) and TC.same_bits(dx.cpu(), x)
    back = Band(n)
    ops.tail("uncast16", [cu(want), back.mid], [n, int(bf16)])
    assert back.intact() and TC.same_bits(back.cpu(), want.float())


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n", TC.CAST_SIZES)
def test_cast16_uncast16(ops, n, bf16):
    run_casts(ops, n, bf16)


@pytest.mark.parametrize("bf16", [False, True])
def test_cast16_uncast16_wrap(ops, bf16):
    run_casts(ops, TC.WRAP, bf16)


# ------------------------------------------------------------------------------------------------ one-rounding arithmetic
def run_gated(ops, N, T, C, integers, seed):
    """x += gate * y is ONE fmaf: |got - ref64| <= 2^-23 (|x| + |g y|) (2^-24 for the single rounding, the factor 2 is margin)"""
    stride, off = 6 * C + 8, 2 * C + 4
    if integers:       # exact in float32: the float32 evaluation IS the float64 value
        x, y = TC.int_blocks(N * T * C, seed, 64).reshape(N, T, C), TC.int_blocks(N * T * C, seed + 1, 64).reshape(N, T, C)
        mod = TC.int_blocks(N * stride, seed + 2, 64).reshape(N, stride)
        g = mod[:, None, off:off + C]
        ref, bound = x + g * y, (x.abs() + (g * y).abs()) * 2.0 ** -23
    else:
        x, y, mod = TC.randn((N, T, C), seed), TC.randn((N, T, C), seed + 1), TC.randn((N, stride), seed + 2)
        g = mod.double()[:, None, off:off + C]
        ref, bound = x.double() + g * y.double(), (x.double().abs() + (g * y.double()).abs()) * 2.0 ** -23
    dy = cu(y)
    room = torch.full((mod.numel() + min(T * C, 1 << 16),), NAN, device="cuda")   # NaN behind mod: an index that runs past a
    dm = room[:mod.numel()].view(N, stride)                                        # row's gate reads NaN, not foreign memory
    dm.copy_(mod)
    out = Band(x.numel(), fill=x)
    ops.tail("gated_residual", [out.mid, dy, dm], [N, T, C, stride, off])
    got = out.cpu(x.shape)
    assert out.intact() and torch.equal(dy.cpu(), y) and torch.equal(dm.cpu(), mod)
    assert bool(((got.to(ref.dtype) - ref).abs() <= bound).all())


@pytest.mark.parametrize("shape", TC.GATED_SHAPES)
def test_gated_residual(ops, shape):
    run_gated(ops, *shape, integers=False, seed=160)


def test_gated_residual_wrap(ops):
    N, T, C = TC.GATED_WRAP
    assert C == 4 and N * T > TC.CAP and (N * T) % 256
    run_gated(ops, N, T, C, integers=True, seed=161)


def run_avgpool2(ops, N, H, W, C, integers, seed):
    """three adds and one multiply: |got - ref64| <= 4 * 2^-24 (|v0| + |v1| + |v2| + |v3|) * 0.25"""
    if integers:       # exact in float32, see run_gated
        x = TC.int_blocks(N * H * W * C, seed, 512).reshape(N, H, W, C)
        xr = x
    else:
        x = TC.randn((N, H, W, C), seed)
        xr = x.double()
    v = TC.avgpool_parts(xr)
    ref = (v[0] + v[1] + v[2] + v[3]) * 0.25
    bound = (v[0].abs() + v[1].abs() + v[2].abs() + v[3].abs()) * (0.25 * 4 * U24)
    y = Band(ref.numel())
    ops.tail("avgpool2", [cu(x), y.mid], [N, H, W, C])
    got = y.cpu(ref.shape)
    assert y.intact() and bool(((got.to(ref.dtype) - ref).abs() <= bound).all())


@pytest.mark.parametrize("shape", TC.AVGPOOL_SHAPES)
def test_avgpool2(ops, shape):
    run_avgpool2(ops, *shape, integers=False, seed=170)


def test_avgpool2_wrap(ops):
    N, H, W, C = TC.AVGPOOL_WRAP
    total4 = N * (H // 2) * (W // 2)
    assert C == 4 and total4 > TC.CAP and total4 % 256
    run_avgpool2(ops, N, H, W, C, integers=True, seed=171)


def avg_launch(ops, srcs, bmask, div, N, HW, C, dstC, coff, act, per_sample=None):
    """-> (dst [N HW, dstC], its initial contents, guards intact, sources unchanged).  A broadcast source is ONE sample at the
    front of a buffer of the full size whose remainder is NaN: a kernel that ignores its bmask bit reads NaN, not foreign memory."""
    dev = []
    for k, s in enumerate(srcs):
        d = cu(s)
        if bmask >> k & 1:
            d[1:] = NAN
        dev.append(d)
    before = [d.clone() for d in dev]
    init = (torch.arange(N * HW * dstC, dtype=torch.float32) % 509) * 0.5 - 2000.0
    dst = Band(N * HW * dstC, fill=init)
    ops.tail("avg_into", dev + [None] * (4 - len(dev)) + [dst.mid], [N * HW, C, dstC, coff, act, HW if per_sample is None else per_sample, bmask], [div])
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dev, before))
    return dst.cpu((N * HW, dstC)), init.reshape(N * HW, dstC), dst.intact(), same


def outside_kept(got, init, coff, C):
    keep = torch.ones(got.shape[1], dtype=torch.bool)
    keep[coff:coff + C] = False
    return torch.equal(got[:, keep], init[:, keep])


@pytest.mark.parametrize("nsrc,div,C,coff,bmask", TC.AVG_CASES)
def test_avg_into(ops, nsrc, div, C, coff, bmask):
    """k adds (k - 1 between the sources, one division): |got - ref64| <= (k + 1) 2^-24 sum_k |src_k| / div"""
    N, HW, dstC = TC.AVG_N, TC.AVG_H * TC.AVG_W, C + 36
    srcs = TC.avg_sources(nsrc, C, bmask, 180 + nsrc)
    got, init, intact, same = avg_launch(ops, srcs, bmask, div, N, HW, C, dstC, coff, 0)
    ref = TC.avg_ref([s.double() for s in srcs], div).reshape(N * HW, C)
    bound = sum(s.double().abs() for s in srcs).reshape(N * HW, C) * ((nsrc + 1) * U24 / div)
    assert intact and same and outside_kept(got, init, coff, C)
    assert bool(((got[:, coff:coff + C].double() - ref).abs() <= bound).all())


def test_avg_into_wrap(ops):
    """256*32*256 + 515 float4 with bmask = 1; small integers and div = 2: exact in float32 (see run_gated)"""
    cols, N = 11, 13
    HW = TC.AVG_WRAP4 // (cols * N)
    C, dstC, coff = 4 * cols, 4 * cols + 36, 32
    assert N * HW * cols == TC.AVG_WRAP4
    mk = lambda s: torch.randint(-512, 513, (N, HW, C), generator=TC.gen(s), dtype=torch.int16).float()
    a, b = mk(190)[:1].expand(N, HW, C).contiguous(), mk(191)
    got, init, intact, same = avg_launch(ops, [a, b], 1, 2.0, N, HW, C, dstC, coff, 0)
    ref, bound = ((a + b) / 2.0).reshape(N * HW, C), (a.abs() + b.abs()).reshape(N * HW, C) * (3 * U24 / 2.0)
    assert intact and same and outside_kept(got, init, coff, C)
    assert bool(((got[:, coff:coff + C] - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ transcendental / reductions
@pytest.mark.parametrize("nsrc,div,C,coff,bmask", TC.AVG_SILU_CASES)
def test_avg_into_silu(ops, nsrc, div, C, coff, bmask):
    N, HW, dstC = TC.AVG_N, TC.AVG_H * TC.AVG_W, C + 36
    srcs = TC.avg_sources(nsrc, C, bmask, 200 + nsrc)
    got, init, intact, same = avg_launch(ops, srcs, bmask, div, N, HW, C, dstC, coff, 1)
    ref64, cpu32 = three(lambda *s: TC.avg_ref(list(s), div, silu=True), *srcs)
    assert intact and same and outside_kept(got, init, coff, C)
    check3(f"avg_into_silu[{nsrc},{div},{C},{coff},{bmask}]", got[:, coff:coff + C].reshape(ref64.shape), ref64, cpu32)


def run_gelu_tanh(ops, n):
    x = TC.tiled(TC.act_pool(), n)
    ref64, cpu32 = three(TC.gelu_tanh_ref, x)
    y = Band(n, fill=x)
    ops.tail("gelu_tanh", [y.mid], [n])
    assert y.intact()
    check3(f"gelu_tanh[{n}]", y.cpu(), ref64, cpu32)


@pytest.mark.parametrize("n", [1, 3000])
def test_gelu_tanh(ops, n):
    run_gelu_tanh(ops, n)


def test_gelu_tanh_wrap(ops):
    run_gelu_tanh(ops, TC.WRAP)


def run_geglu(ops, rows, inner):
    x = TC.geglu_input(rows, inner)
    ref64, cpu32 = three(TC.geglu_ref, x)
    dx = cu(x)
    y = Band(rows * inner)
    ops.tail("geglu", [dx, y.mid], [rows, inner])
    assert y.intact() and torch.equal(dx.cpu(), x)
    check3(f"geglu[{rows},{inner}]", y.cpu((rows, inner)), ref64, cpu32)


@pytest.mark.parametrize("rows,inner", TC.GEGLU_SHAPES)
def test_geglu(ops, rows, inner):
    run_geglu(ops, rows, inner)


def test_geglu_wrap(ops):
    rows, inner = TC.GEGLU_WRAP
    assert rows * inner > TC.CAP and (rows * inner) % 256
    run_geglu(ops, rows, inner)


@pytest.mark.parametrize("scale", TC.SOFTMAX_SCALES)
@pytest.mark.parametrize("rows,cols", TC.SOFTMAX_SHAPES)
def test_softmax_rows(ops, rows, cols, scale):
    x = TC.softmax_input(rows, cols, scale)
    ref64, cpu32 = three(lambda t: TC.softmax_ref(t, scale), x)
    y = Band(rows * cols, fill=x)
    ops.tail("softmax_rows", [y.mid], [rows, cols], [scale])
    got = y.cpu((rows, cols))
    assert y.intact()
    check3(f"softmax_rows[{rows},{cols},{scale}]", got, ref64, cpu32)
    assert maxabs(got.double().sum(dim=1) - 1.0) <= cols * U24
    spike, equal = TC.softmax_rows_special(rows, cols)
    if spike is not None:
        rest = torch.ones(cols, dtype=torch.bool)
        rest[cols // 3] = False
        assert maxabs(got[spike, rest]) <= 1e-40 and abs(float(got[spike, cols // 3]) - 1.0) <= U24   # the others underflowed
    if equal is not None:
        assert bool((got[equal] == got[equal, 0]).all())                                            # equal logits, equal weights


@pytest.mark.parametrize("eps,kind", TC.LAYER_NORM_KINDS)
@pytest.mark.parametrize("rows,C", TC.LAYER_NORM_SHAPES)
def test_layer_norm(ops, rows, C, eps, kind):
    x, gamma, beta = TC.layer_norm_input(rows, C, kind)
    ref64, cpu32 = three(lambda a, g, b: TC.layer_norm_ref(a, g, b, eps), x, gamma, beta)
    dx = cu(x)
    y = Band(rows * C)
    ops.tail("layer_norm", [dx, cu(gamma), cu(beta), y.mid], [rows, C], [eps])
    assert y.intact() and torch.equal(dx.cpu(), x)
    check3(f"layer_norm[{rows},{C},{eps},{kind}]", y.cpu((rows, C)), ref64, cpu32)


@pytest.mark.parametrize("N,T,C", TC.LN_MOD_SHAPES)
def test_ln_modulate(ops, N, T, C):
    eps = 1e-6
    stride, sh, sc = TC.ln_mod_layout(C, aligned=False)
    assert sh % C and sc % C and sh != sc
    x, mod = TC.ln_mod_input(N, T, C, aligned=False)
    ref64, cpu32 = three(lambda a, m: TC.ln_mod_ref(a, m, C, False, eps), x, mod)
    dx, dm = cu(x), cu(mod)
    y = Band(N * T * C)
    ops.tail("ln_modulate", [dx, dm, y.mid], [N, T, C, stride, sh, sc], [eps])
    assert y.intact() and torch.equal(dx.cpu(), x) and torch.equal(dm.cpu(), mod)
    check3(f"ln_modulate[{N},{T},{C}]", y.cpu((N, T, C)), ref64, cpu32)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("C", TC.LN16_WIDTHS)
def test_ln_modulate16(ops, C, bf16):
    """every instantiation (NV 1, 2, 3, 4, 5, 8) at its full width and with a partial last vector; N*T = 5"""
    eps = 1e-6
    dt = torch.bfloat16 if bf16 else torch.float16
    N, T = (5, 1) if TC.LN16_WIDTHS.index(C) % 2 == 0 else (1, 5)
    stride, sh, sc = TC.ln_mod_layout(C, aligned=True)
    x, mod = TC.ln_mod_input(N, T, C, aligned=True)
    ref64, cpu32 = three(lambda a, m: TC.ln_mod_ref(a, m, C, True, eps), x, mod)
    cpu16 = cpu32.to(dt)
    assert TC.frac_beyond_one_ulp(cpu16, ref64.to(dt), bf16) <= 1e-3          # the cap holds for the reference's own arithmetic
    dx, dm = cu(x), cu(mod)
    y = Band(N * T * C, dtype=dt)
    ops.tail("ln_modulate16", [dx, dm, y.mid], [N, T, C, stride, sh, sc, int(bf16)], [eps])
    got = y.cpu((N, T, C))
    assert y.intact() and torch.equal(dx.cpu(), x) and torch.equal(dm.cpu(), mod)
    check3(f"ln_modulate16[{C},{'bf16' if bf16 else 'f16'}]", got, ref64, cpu16, floor=2.0 ** -8 if bf16 else 2.0 ** -11)
    assert not bool(torch.isnan(got).any()) and TC.frac_beyond_one_ulp(got, cpu16, bf16) <= 1e-3


@pytest.mark.parametrize("N,HW,C,Cr", TC.SE_SHAPES)
def test_se_scale(ops, N, HW, C, Cr):
    x, w1, w2 = TC.se_input(N, HW, C, Cr)
    ref64, cpu32 = three(TC.se_ref, x, w1, w2)
    dx = cu(x)
    y = Band(x.numel())
    ops.tail("se_scale", [dx, cu(w1), cu(w2), y.mid], [N, HW, C, Cr])
    assert y.intact() and torch.equal(dx.cpu(), x)
    check3(f"se_scale[{N},{HW},{C},{Cr}]", y.cpu(x.shape), ref64, cpu32)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    buf = torch.zeros(8192, device="cuda")
    raises(ops, "avgpool2: bad shape", "avgpool2", [buf, buf], [1, 3, 4, 4])                      # odd H
    raises(ops, "avgpool2: bad shape", "avgpool2", [buf, buf], [1, 4, 3, 4])                      # odd W
    raises(ops, "avgpool2: bad shape", "avgpool2", [buf, buf], [1, 4, 4, 6])                      # C % 4
    raises(ops, "upsample2: bad shape", "upsample2", [buf, buf], [1, 2, 2, 6])
    raises(ops, "gated_residual: widths must be multiples of 4", "gated_residual", [buf, buf, buf], [1, 2, 8, 56, 18])
    raises(ops, "avg_into: channel counts must be multiples of 4", "avg_into", [buf, None, None, None, buf], [4, 4, 40, 2, 0, 0, 0], [1.0])
    raises(ops, "C=2052", "ln_modulate16", [buf, buf, buf], [1, 1, 2052, 6 * 2052, 0, 2052, 0], [1e-6])
    raises(ops, "C=66", "ln_modulate16", [buf, buf, buf], [1, 1, 66, 400, 0, 68, 0], [1e-6])
    raises(ops, "shift_off=6", "ln_modulate16", [buf, buf, buf], [1, 1, 64, 400, 6, 128, 0], [1e-6])


def test_avg_into_broadcast_needs_per_sample_pixels(ops):
    """bmask != 0 indexes a source with i % (per_sample_pixels * C / 4) on the device: 0 (the launcher's default) and a count
    that does not divide the pixels are refused before any launch"""
    buf = torch.zeros(4096, device="cuda")
    for per_sample in (0, -15, 7):
        raises(ops, "per_sample_pixels", "avg_into", [buf, buf, None, None, buf], [45, 4, 40, 0, 0, per_sample, 1], [2.0])
    dst = Band(45 * 40, fill=torch.zeros(45 * 40))
    ops.tail("avg_into", [buf, buf, None, None, dst.mid], [45, 4, 40, 0, 0, 0, 0], [2.0])         # no broadcast: 0 is fine
    assert dst.intact()
