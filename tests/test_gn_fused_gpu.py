"""The fused GroupNorm routes the networks run by default, kernel by kernel against float64 (GPU): the statistics epilogues of the
convolutions, GroupNorm + SiLU applied while the tap-reuse kernel stages its rows, gn_finalize beyond the one-source case,
avg_into_stats and gn_small — through dsd_op_conv2d_gn / dsd_op_gn_finalize / dsd_op_avg_into_stats / dsd_op_gn_small, which
launch nothing but conv2d(), gn_finalize(), avg_into_stats() and gn_small() as net.cpp does.

The bound on the emitted statistics (a).  A chunk is a run of R = OH*OW / chunks consecutive output pixels of one sample (sub-pixel
form: chunk (2 py + px) * (H*W / 256) + t holds the phase-(py, px) outputs of low-resolution pixels [256 t, 256 t + 256):
conv_split_kernels.inc, `q.stats = p.stats + sph * (ohw / 256) * sub_cout * 2` with sph = n0 / sub_cout, py = sph >> 1, px = sph & 1).
With u = 2^-24, rho = max - min and a = max |v| of a column inside the chunk, the emitted (sum, sumsq) must satisfy, against fp64
sums of the tensor that was WRITTEN (y read back and widened: what the standalone pass would see),
    |d sum| <= 2^-18 R rho        |d var| <= 2^-17 rho^2 + 2^-50 a^2,   var = sumsq / R - (sum / R)^2 in fp64.
Derivation, checked against each kernel:
  * split_epilogue / subpixel_epilogue (StatAcc; staged, 128-row, 256-row, tap-reuse and sub-pixel kernels): a lane adds its 16
    (128-row tile) or 32 (256-row tile: two row blocks, the shift taken in the first) values of a column as d = v - r, r its first
    value, S += d, Q = fma(d, d, Q) in fp32.  d carries one rounding (|d| <= rho), the n <= 32 additions at most n more:
    |dS| <= 33 u sum|d| <= 33 u n rho and |dQ| <= 34 u sum d^2.  flush() rebuilds sum = S + n r and sumsq = Q + 2 r S + n r^2 in fp64,
    and everything above a lane (stats_reduce: shuffle, LDS, four waves) is fp64 in a fixed order.  Summed over the R / n lanes of
    a column |d sum| <= 33 u R rho = 1.03 * 2^-19 R rho.  In the variance r cancels: per lane the contribution to R var is
    Q + 2 (r - m) S + n (r - m)^2 (m the chunk mean), so |d(R var)| <= 34 u sum d^2 + 2 |r - m| 33 u sum|d| <= (34 + 66) u n rho^2 and,
    with the error of (sum/R)^2 around m, 2 |m'| |d sum| / R with |m'| <= rho in the shifted frame (~ 3 u rho^2 more),
    |d var| <= 103 u rho^2 = 0.80 * 2^-17 rho^2.  The fp64 operations (about eight roundings on terms <= a^2) are the 2^-50 a^2.
  * conv_tr16.hip (16x16x32 MFMA shape) keeps its own copy with 16 values per lane and bias + emb added as one term: the same
    bound with n = 16.  conv_wino.hip keeps another: 16 tiles x 2 pixels = 32 values per lane, the pair's d0 + d1 formed first
    (one rounding for two values: no more than the chain's), Q by two fmas: the same bound.
  * conv_direct_cols_kernel<9, true> sums in fp64 throughout: its statistics must hold 1e-12 relative (of sum|v| and sum v^2),
    asserted on top of the bound above.
Unshifted fp32 partials would miss the variance bound by orders of magnitude once mean >> sigma, so every case runs with bias ~ N(0, 1)
and with bias + 100.

Tolerances elsewhere: PREC_TOL of tests/test_ops_gpu.py for convolution outputs (the GN + SiLU instantiation holds the bf16x6 bar, as
test_gn_silu_conv_out1_vs_fp64 does with the same hardware exp2 / rcp), 2e-6 rel-L2 for normalised tensors (the project's GroupNorm
bar), and for gn_finalize's scale an elementwise bound from its fp32 roundings: scale = fl(fl(rstd) gamma) is two roundings,
FiLM's fl(1 + f) and the product two more, so |scale - ref| <= (k + 1) u |ref| with k = 2 or 4 (one u for the fp64 parts and the
reference's own rounding).  avg_into_stats without activation: three fp32 additions and one division, each <= u sum|src| / div
before / after the division: |dst - ref| <= 4 u sum|src| / div; its fp64 partials hold 1e-12 relative.
"""
import re

import pytest
import torch
import torch.nn.functional as F

from util import rel_l2
from test_ops_gpu import PREC_TOL
from test_conv_args_gpu import Problem, sentinel, y_layout, GUARD

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SG = 64          # doubles in front of and behind a statistics buffer


@pytest.fixture(scope="module")
def ops():
    from diffusion_models_dsdiff_amd import ops as m, _lib
    _lib.require_gpu(0)
    return m


_problems = {}


def problem(*key, **kw):
    """One problem (operands + its float64 convolution) at a time, shared by consecutive tests on the same shape."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _problems:
        _problems.clear()
        _problems[k] = Problem(*key, **kw)
    return _problems[k]


def bare(key, seed, stride=1):
    """Operands of a 3x3 problem (x, w, b, emb, res) without the float64 convolution, for the tests that need none or their own."""
    N, H, W, Cin, Cout = key
    P = Problem.__new__(Problem)
    P.key, P.N, P.H, P.W, P.Cin, P.Cout, P.ks, P.stride, P.ups, P.pad = key, N, H, W, Cin, Cout, 3, stride, False, (-1, -1)
    P.OH, P.OW = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    g = torch.Generator().manual_seed(sum(key) + seed)
    P.x = torch.randn(N, Cin, H, W, generator=g)
    P.w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    P.b = torch.randn(Cout, generator=g)
    P.emb = torch.randn(N, Cout, generator=g)
    P.res = torch.randn(N, Cout, P.OH, P.OW, generator=g)
    P.gen = g
    return P


def nan_stats(n):
    return torch.full((SG + n + SG,), float("nan"), dtype=torch.float64, device=DEV)


def launch(ops, P, bias, y="plain", emb=None, res=False, prec="bf16x6", structure="auto", no_scratch=False, want_stats=True, gn=None):
    """One dsd_op_conv2d_gn launch into sentinel-filled buffers.  y: plain | ld_off | nchw; emb: None | plain | strided; gn: None or
    (scale, shift) [N, Cin] device tensors.
    -> dict(out: logical NHWC result, name, ksplit, chunks, stats [N, chunks, Cout, 2] or None, intact, guards)"""
    N, H, W, Cin, Cout = P.N, P.H, P.W, P.Cin, P.Cout
    xb = P.x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = P.w.to(DEV)
    ld, off = y_layout(P, y)
    rows = N * P.OH * P.OW
    buf0 = sentinel(GUARD + rows * ld + GUARD)
    buf = buf0.clone()

    def view(b):
        body = b[GUARD:GUARD + rows * ld]
        return body.view(N, Cout, P.OH, P.OW) if y == "nchw" else body.view(N, P.OH, P.OW, ld)[..., off:off + Cout]

    e, es = None, 0
    if emb == "plain":
        e = P.emb.to(DEV)
    elif emb == "strided":
        es = (Cout + 40 + 3) // 4 * 4
        eb = torch.full((N, es), float("nan"))
        eb[:, 8:8 + Cout] = P.emb
        e = eb.to(DEV)[:, 8:8 + Cout]
    r = P.res.permute(0, 2, 3, 1).contiguous().to(DEV) if res else None
    kw = dict(stride=P.stride, upsample=P.ups, emb=e, res=r, precision=prec, structure=structure, y_ld=ld if y == "ld_off" else 0,
              out_nchw=y == "nchw", emb_stride=es, no_scratch=no_scratch, pad_lo=P.pad[0], pad_total=P.pad[1],
              gn_scale=None if gn is None else gn[0], gn_shift=None if gn is None else gn[1])
    args = (xb, (N, H, W, Cin), wd, bias.to(DEV), view(buf))
    qname, qks, chunks = ops.conv2d_gn(*args, query=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(buf, buf0), "a query wrote to y"
    sbuf = stats = None
    if want_stats:
        n = N * max(chunks, 1) * Cout * 2
        sbuf = nan_stats(n)
        stats = sbuf[SG:SG + n]
    name, ksplit, chunks2 = ops.conv2d_gn(*args, stats=stats, **kw)
    assert (name, ksplit, chunks2) == (qname, qks, chunks), "the query and the launch disagree"
    out = (view(buf).permute(0, 2, 3, 1) if y == "nchw" else view(buf)).contiguous()
    chk = buf.clone()
    view(chk).copy_(view(buf0))
    guards = want_stats and bool(torch.isnan(sbuf[:SG]).all() and torch.isnan(sbuf[SG + n:]).all())
    return dict(out=out, name=name, ksplit=ksplit, chunks=chunks, stats=stats.view(N, chunks, Cout, 2) if want_stats else None,
                intact=torch.equal(chk, buf0), guards=guards)


def chunked(out, chunks, sub):
    """logical NHWC output -> float64 [N, chunks, R, C] in the kernels' chunk order"""
    N, OH, OW, C = out.shape
    if sub:
        H, W = OH // 2, OW // 2
        v = out.view(N, H, 2, W, 2, C).permute(0, 2, 4, 1, 3, 5)      # [N, py, px, H, W, C]
        return v.reshape(N, chunks, 4 * H * W // chunks, C).double()
    return out.reshape(N, chunks, OH * OW // chunks, C).double()


def check_stats(tag, out, stats, sub=False, fp64=False):
    """the finiteness and the bound of the module docstring (all on the device, float64)"""
    assert bool(torch.isfinite(stats).all()), f"{tag}: statistics left unwritten / not finite"
    N, chunks, C, _ = stats.shape
    v = chunked(out, chunks, sub)
    R = v.shape[2]
    if sub:
        assert R == 256
    s_ref = v.sum(2)
    m = s_ref / R
    var_ref = ((v - m[:, :, None]) ** 2).mean(2)
    rho = v.amax(2) - v.amin(2)
    a = v.abs().amax(2)
    ds = (stats[..., 0] - s_ref).abs()
    dv = (stats[..., 1] / R - (stats[..., 0] / R) ** 2 - var_ref).abs()
    bs, bv = 2.0 ** -18 * R * rho, 2.0 ** -17 * rho ** 2 + 2.0 ** -50 * a ** 2
    print(f"{tag}: R={R} chunks={chunks} worst |d sum| / bound {float((ds / bs).max()):.3e}  |d var| / bound {float((dv / bv).max()):.3e}")
    assert bool((ds <= bs).all()), f"{tag}: sum off by up to {float((ds / bs).max()):.3e} of the bound"
    assert bool((dv <= bv).all()), f"{tag}: variance off by up to {float((dv / bv).max()):.3e} of the bound"
    if fp64:
        q_ref = (v * v).sum(2)
        assert bool((ds <= 1e-12 * v.abs().sum(2)).all()), f"{tag}: fp64 sums beyond 1e-12"
        assert bool(((stats[..., 1] - q_ref).abs() <= 1e-12 * q_ref).all()), f"{tag}: fp64 sums of squares beyond 1e-12"


def tile_cols(name):
    """column-tile width from the kernel name (32 per unit of the template argument; the F(2,3) kernel: 128)"""
    m = re.search(r"<(\d)>", name)
    return 32 * int(m.group(1)) if m else 128


def stats_case(ops, P, expect, prec="bf16x6", structure="auto", sub=False, fp64=False, ragged=None):
    """(a) for one kernel: bias ~ N(0, 1) and bias + 100, each run twice; without scratch; and the slice / emb / res variant."""
    nchunks = None
    for shift in (0.0, 100.0):
        bias = (P.b + shift).float()
        ref = P.base + (bias.double() - P.b.double())[None, :, None, None]
        r1 = launch(ops, P, bias, prec=prec, structure=structure)
        tag = f"stats {P.key} {prec} bias+{shift:g} {r1['name']}"
        assert re.fullmatch(expect, r1["name"]), f"{tag}: expected {expect}"
        assert r1["chunks"] > 0 and r1["ksplit"] == 1, tag
        if ragged is not None:
            assert (P.Cout % tile_cols(r1["name"]) != 0) == ragged, f"{tag}: column tiles of {tile_cols(r1['name'])} on {P.Cout} columns"
        assert r1["intact"] and r1["guards"], f"{tag}: wrote outside y or the statistics"
        err = rel_l2(r1["out"].permute(0, 3, 1, 2), ref)
        print(f"{tag}: rel-L2 vs fp64 {err:.3e}")
        assert err < PREC_TOL[prec], (tag, err)
        check_stats(tag, r1["out"], r1["stats"], sub, fp64)
        r2 = launch(ops, P, bias, prec=prec, structure=structure)
        assert torch.equal(r1["out"], r2["out"]) and torch.equal(r1["stats"], r2["stats"]), f"{tag}: a second run differs"
        nchunks = r1["chunks"]
    # wherever the query says the kernel emits statistics, the launch without scratch does too
    r3 = launch(ops, P, P.b, prec=prec, structure=structure, no_scratch=True)
    assert re.fullmatch(expect, r3["name"]) and r3["chunks"] == nchunks and r3["intact"] and r3["guards"]
    check_stats(f"stats {P.key} {prec} no scratch", r3["out"], r3["stats"], sub, fp64)
    # a channel slice of a wider tensor, a column range of a wider embedding, a residual: the statistics of the slice as written
    r4 = launch(ops, P, P.b, y="ld_off", emb="strided", res=True, prec=prec, structure=structure)
    tag = f"stats {P.key} {prec} slice+emb+res {r4['name']}"
    assert re.fullmatch(expect, r4["name"]) and r4["chunks"] == nchunks, tag
    assert r4["intact"] and r4["guards"], f"{tag}: the slice's neighbours or the statistics' guards lost their sentinels"
    err = rel_l2(r4["out"].permute(0, 3, 1, 2), P.ref(False, True, True))
    print(f"{tag}: rel-L2 vs fp64 {err:.3e}")
    assert err < PREC_TOL[prec], (tag, err)
    check_stats(tag, r4["out"], r4["stats"], sub, fp64)
    r5 = launch(ops, P, P.b, y="ld_off", emb="strided", res=True, prec=prec, structure=structure)
    assert torch.equal(r4["out"], r5["out"]) and torch.equal(r4["stats"], r5["stats"]), f"{tag}: a second run differs"
    return nchunks


# ---------------------------------------------------------------------------------------------- (a) statistics epilogues
@pytest.mark.parametrize("prec", ["bf16x6", "f16x3", "bf16x3"])
def test_stats_staged(ops, prec):
    P = problem(2, 16, 16, 64, 64)
    assert stats_case(ops, P, r"conv_%s<\d>/staged" % prec, prec=prec, structure="staged") == 2          # 256 pixels / 128 rows


@pytest.mark.parametrize("cout", [96, 100])
def test_stats_r128(ops, cout):
    """100 columns: the last 32-column block of the tile holds 4 (the ragged path of split_epilogue: st.rows, st.first)."""
    P = problem(2, 64, 64, 64, cout)
    assert stats_case(ops, P, r"conv_bf16x6<[1-3]>/r128", structure="adirect", ragged=cout == 100) == 32


def test_stats_256_rows_wide_ragged_tiles(ops):
    P = problem(2, 128, 96, 64, 300)           # a width that is no power of two keeps the launch off the tap-reuse kernel
    assert stats_case(ops, P, r"conv_bf16x6<5>", structure="adirect256", ragged=True) == 48


TR_STATS = [((9, 64, 64, 32, 160), r"conv_bf16x6<5>/tr", False, 16), ((2, 128, 128, 64, 300), r"conv_bf16x6<5>/tr", True, 64),
            ((1, 256, 256, 64, 128), r"conv_bf16x6<4>/tr", False, 256)]


@pytest.mark.parametrize("key,name,ragged,chunks", TR_STATS)
def test_stats_tap_reuse(ops, key, name, ragged, chunks):
    P = problem(*key)
    for mfma16 in (0, 1):
        prev = ops.conv_mfma16(mfma16)
        try:
            assert stats_case(ops, P, name, ragged=ragged) == chunks
        finally:
            ops.conv_mfma16(prev)


def test_stats_subpixel(ops):
    P = problem(2, 16, 64, 64, 160, ups=True)
    assert stats_case(ops, P, r"conv_bf16x6<5>/tr\+subpixel", sub=True) == 16       # 4 phases x 1024 / 256


def test_stats_winograd(ops):
    P = problem(1, 64, 64, 64, 128)
    assert stats_case(ops, P, r"conv_wino_bf16x6", structure="winograd", ragged=False) == 16


def test_stats_direct_cols(ops):
    P = problem(2, 32, 32, 1, 32)
    assert stats_case(ops, P, r"conv_direct_cols", prec="f32", fp64=True) == 8


# ---------------------------------------------------------------------------------------------- (b) exact constant channels
@pytest.mark.parametrize("key,name,ragged", [((9, 64, 64, 32, 160), r"conv_bf16x6<5>/tr", False),
                                             ((2, 128, 128, 64, 224), r"conv_bf16x6<4>/tr", True)])
def test_constant_channels_are_exact(ops, key, name, ragged):
    """Every fourth GroupNorm group gets all-zero weights and one fp32 bias (and embedding) value for the whole group: those
    columns hold one value v per sample, the shifted partials are exactly zero and (sum, sumsq) = (R v, R v v) exactly (R = 256,
    v v has 48 bits).  The group's variance is then zero up to fp64 rounding of the cross-chunk sums (<< eps) and gn_finalize gives
    rstd = 1 / sqrt(eps) to fp32 rounding — unshifted partials gave 9e-5 here once (conv_split_kernels.inc).  224 columns on
    128-column tiles put constant groups into the ragged tile too.  No float64 convolution is needed for this."""
    N, H, W, Cin, Cout = key
    cpg = Cout // 32
    P = bare(key, 0)
    const = (torch.arange(Cout) // cpg) % 4 == 3
    P.w[const] = 0.0
    bias = torch.randn(32, generator=P.gen).repeat_interleave(cpg) * 3 + 0.7
    P.emb = torch.randn(N, 32, generator=P.gen).repeat_interleave(cpg, dim=1)
    for mfma16 in (0, 1):
        prev = ops.conv_mfma16(mfma16)
        try:
            for emb in (None, "plain"):
                r = launch(ops, P, bias, emb=emb)
                tag = f"constant {key} mfma16={mfma16} emb={emb} {r['name']}"
                assert re.fullmatch(name, r["name"]) and r["chunks"] == H * W // 256 and r["intact"] and r["guards"], tag
                assert (Cout % tile_cols(r["name"]) != 0) == ragged, tag
                v = (bias[None, :] + P.emb if emb else bias[None, :].expand(N, -1)).to(DEV)[:, const]        # fp32, as the epilogue adds
                yc = r["out"][..., const.to(DEV)]
                assert torch.equal(yc, v[:, None, None, :].expand_as(yc)), f"{tag}: a zero-weight column is not bias (+ emb)"
                st = r["stats"][:, :, const.to(DEV)]
                v64 = v.double()[:, None, :].expand(N, r["chunks"], -1)
                assert torch.equal(st[..., 0], 256.0 * v64), f"{tag}: sum of a constant column is not exactly R v"
                assert torch.equal(st[..., 1], 256.0 * v64 * v64), f"{tag}: sum of squares of a constant column is not exactly R v v"
                check_stats(tag, r["out"], r["stats"])
                eps = 1e-5
                scale, _ = ops.gn_finalize([r["stats"].contiguous()], N, H * W, Cout, torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV), eps)
                want = float(torch.tensor(1.0, dtype=torch.float64) / torch.tensor(eps, dtype=torch.float32).double().sqrt())
                got = scale[:, const.to(DEV)].double()
                assert bool(((got - want).abs() <= 2 * U * want).all()), f"{tag}: rstd of a zero-variance group {float(got.min())} .. {float(got.max())}, not {want}"
        finally:
            ops.conv_mfma16(prev)


# ---------------------------------------------------------------------------------------------- (c) refusals
def refused(ops, P, match, **kw):
    """the call must raise and name the reason, and neither the sentinel-filled output nor the NaN-filled statistics buffer may change"""
    from diffusion_models_dsdiff_amd import _lib
    N, Cout = P.N, P.Cout
    ld, off = y_layout(P, kw.get("y", "plain"))
    rows = N * P.OH * P.OW
    buf0 = sentinel(GUARD + rows * ld + GUARD)
    buf = buf0.clone()
    body = buf[GUARD:GUARD + rows * ld]
    yv = body.view(N, Cout, P.OH, P.OW) if kw.get("y") == "nchw" else body.view(N, P.OH, P.OW, ld)[..., off:off + Cout]
    n = N * 4 * Cout * 2
    sbuf = nan_stats(n)
    gn = kw.get("gn", (None, None))
    args = dict(stride=P.stride, upsample=P.ups, precision=kw.get("prec", "bf16x6"), structure=kw.get("structure", "auto"),
                out_nchw=kw.get("y") == "nchw", no_scratch=kw.get("no_scratch", False), gn_scale=gn[0], gn_shift=gn[1],
                stats=sbuf[SG:SG + n] if kw.get("stats", True) else None)
    with pytest.raises(_lib.DsdError, match=match):
        ops.conv2d_gn(P.x.permute(0, 2, 3, 1).contiguous().to(DEV), (N, P.H, P.W, P.Cin), P.w.to(DEV), P.b.to(DEV), yv, **args)
    torch.cuda.synchronize()
    assert torch.equal(buf, buf0), f"{P.key} {kw}: a refused launch wrote to y"
    assert bool(torch.isnan(sbuf).all()), f"{P.key} {kw}: a refused launch wrote statistics"


def operands(*key):
    return bare(key, 1)


def test_refusals_launch_nothing(ops):
    cannot = "cannot emit"
    refused(ops, operands(2, 16, 16, 64, 64), cannot, prec="f32")                                   # fp32 MFMA kernel
    for no_scratch in (False, True):
        refused(ops, operands(1, 8, 8, 960, 960), cannot, no_scratch=no_scratch)                    # split-K: the reduction writes y
    refused(ops, operands(2, 128, 128, 64, 320), cannot, y="nchw")
    refused(ops, operands(3, 40, 24, 64, 320), cannot, structure="adirect256")                     # 960 pixels per sample, 256-row tiles
    refused(ops, operands(3, 44, 32, 64, 192), cannot, structure="winograd")                       # 1408 pixels per sample, 256 per block
    refused(ops, operands(2, 16, 16, 6, 320), cannot, prec="f32")                                   # conv_direct_lds
    refused(ops, operands(2, 16, 16, 6, 320), cannot, prec="bf16x6")
    one = lambda P: torch.ones(P.N, P.Cin, device=DEV)
    P = operands(2, 64, 64, 64, 96)                                                                 # 96-column tiles: not the tap-reuse kernel
    refused(ops, P, "does not apply", stats=False, gn=(one(P), one(P)))
    P = operands(2, 16, 16, 64, 64)
    refused(ops, P, "does not apply", stats=False, prec="f32", gn=(one(P), one(P)))
    P = operands(9, 64, 64, 32, 160)                                                                # the tap-reuse kernel, half the coefficients
    refused(ops, P, "come together", stats=False, gn=(one(P), None))
    refused(ops, P, "come together", stats=False, gn=(None, one(P)))
    # a statistics buffer smaller than the chunks need
    from diffusion_models_dsdiff_amd import _lib
    y0 = sentinel(9 * 64 * 64 * 160)
    y = y0.clone()
    small = nan_stats(9 * 15 * 160 * 2)
    with pytest.raises(_lib.DsdError, match="statistics buffer"):
        ops.conv2d_gn(P.x.permute(0, 2, 3, 1).contiguous().to(DEV), (9, 64, 64, 32), P.w.to(DEV), P.b.to(DEV), y.view(9, 64, 64, 160),
                      precision="bf16x6", stats=small[SG:SG + 9 * 15 * 160 * 2])
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and bool(torch.isnan(small).all())


# ---------------------------------------------------------------------------------------------- (d) GN + SiLU inside the convolution
GN_SHAPES = [((9, 64, 64, 32, 160), r"conv_bf16x6<5>/tr\+gn"), ((2, 128, 128, 64, 300), r"conv_bf16x6<5>/tr\+gn"),
             ((2, 128, 256, 64, 128), r"conv_bf16x6<4>/tr\+gn")]     # (the 128-column tile with two samples: 1 x 256 x 256 has one)


@pytest.mark.parametrize("key,name", GN_SHAPES)
def test_gn_silu_inside_conv(ops, key, name):
    """conv(silu(x scale + shift)) + bias (+ emb + res) with coefficients drawn per (sample, channel): shift ~ N(1.5, 1) makes
    silu(shift) != 0, so a kernel that pads before the activation is wrong on the border ring, and one that reads another
    sample's coefficients is wrong everywhere."""
    N, H, W, Cin, Cout = key
    P = bare(key, 31)
    x, w, b = P.x, P.w, P.b
    scale = 1.0 + 0.3 * torch.randn(N, Cin, generator=P.gen)
    shift = 1.5 + torch.randn(N, Cin, generator=P.gen)
    act = F.silu(x.double() * scale.double()[:, :, None, None] + shift.double()[:, :, None, None])
    P.base = F.conv2d(act, w.double(), b.double(), padding=1)
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    gn = (scale.to(DEV), shift.to(DEV))
    for mfma16 in (0, 1):
        prev = ops.conv_mfma16(mfma16)
        try:
            for kw in (dict(want_stats=False), dict(want_stats=True, y="ld_off", emb="strided", res=True)):
                full = kw["want_stats"]
                r = launch(ops, P, b, gn=gn, **kw)
                tag = f"gn+silu conv {key} mfma16={mfma16} stats={full} {r['name']}"
                assert re.fullmatch(name, r["name"]) and r["name"].endswith("+gn") and r["intact"], tag
                ref = P.ref(False, full, full)
                out = r["out"].permute(0, 3, 1, 2).double().cpu()
                err, err_ring = rel_l2(out, ref), rel_l2(out[:, :, ring], ref[:, :, ring])
                print(f"{tag}: rel-L2 vs fp64 {err:.3e}, border ring {err_ring:.3e}")
                assert err < PREC_TOL["bf16x6"], (tag, err)
                assert err_ring < PREC_TOL["bf16x6"], (tag, err_ring)
                for n in range(N):      # and every sample's ring on its own
                    assert rel_l2(out[n][:, ring], ref[n][:, ring]) < PREC_TOL["bf16x6"], (tag, n)
                if full:
                    assert r["chunks"] == H * W // 256 and r["guards"], tag
                    check_stats(tag, r["out"], r["stats"])
        finally:
            ops.conv_mfma16(prev)


# ---------------------------------------------------------------------------------------------- (e) gn_finalize
def partials(x, c0, c1, chunks):
    """float64 (sum, sumsq) of channels [c0, c1) of x [N, C, HW] over `chunks` uneven runs of pixels -> [N, chunks, c, 2]"""
    N, _, HW = x.shape
    cuts = [0] + sorted({max(1, (HW * (i + 1)) // chunks - (i % 2)) for i in range(chunks - 1)}) + [HW]
    assert len(cuts) == chunks + 1
    xs = x[:, c0:c1].double()
    return torch.stack([torch.stack([xs[:, :, a:b].sum(2), (xs[:, :, a:b] ** 2).sum(2)], -1) for a, b in zip(cuts[:-1], cuts[1:])], 1)


@pytest.mark.parametrize("C,split,chunks,film", [(96, (40, 56), (2, 5), False), (320, (192, 128), (3, 1), True), (64, (64,), (1,), False),
                                                 (96, (40, 56), (5, 2), True)])
def test_gn_finalize_sources_and_film(ops, C, split, chunks, film):
    """40 + 56 of 96 channels: the boundary cuts the group of channels 39 .. 41, and the two sources come in different chunk counts."""
    N, HW, eps = 3, 120, 1e-5
    g = torch.Generator().manual_seed(C + len(split))
    x = torch.randn(N, C, HW, generator=g) * 3 + 1.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    srcs, c0 = [], 0
    for c, ch in zip(split, chunks):
        srcs.append(partials(x, c0, c0 + c, ch).contiguous().to(DEV))
        c0 += c
    fs = 2 * C + 8
    fb = torch.full((N, fs), float("nan"))
    fb[:, :2 * C] = torch.randn(N, 2 * C, generator=g) * 0.5
    scale, shift = ops.gn_finalize(srcs, N, HW, C, gamma.to(DEV), beta.to(DEV), eps, film=fb.to(DEV) if film else None, film_stride=fs if film else 0)
    xg = x.double().view(N, 32, -1)
    mean, var = xg.mean(2), xg.var(2, unbiased=False)
    rstd = (1.0 / (var + float(torch.tensor(eps, dtype=torch.float32).double())).sqrt()).repeat_interleave(C // 32, 1)
    mean = mean.repeat_interleave(C // 32, 1)
    sc_ref = rstd * gamma.double()
    sh_ref = beta.double() - mean * sc_ref
    if film:
        f = 1.0 + fb[:, :C].double()
        sc_ref, sh_ref = sc_ref * f, sh_ref * f + fb[:, C:2 * C].double()
    ref = x.double() * sc_ref[:, :, None] + sh_ref[:, :, None]
    got = x.double() * scale.double().cpu()[:, :, None] + shift.double().cpu()[:, :, None]
    err = rel_l2(got, ref)
    k = 4 if film else 2
    worst = float(((scale.double().cpu() - sc_ref).abs() / sc_ref.abs()).max() / U)
    print(f"gn_finalize C={C} sources {split} chunks {chunks} film={film}: x scale + shift rel-L2 {err:.3e}, scale off by {worst:.2f} u (bound {k + 1})")
    assert err < 2e-6
    assert bool(((scale.double().cpu() - sc_ref).abs() <= (k + 1) * U * sc_ref.abs()).all()), worst


def test_gn_finalize_refuses_sources_that_do_not_cover(ops):
    from diffusion_models_dsdiff_amd import _lib
    N, HW, C = 3, 120, 96
    a = torch.zeros(N, 2, 40, 2, dtype=torch.float64, device=DEV)
    b = torch.zeros(N, 2, 48, 2, dtype=torch.float64, device=DEV)
    ones = torch.ones(C, device=DEV)
    for srcs in ([a, b], [a]):
        with pytest.raises(_lib.DsdError, match="do not cover"):
            ops.gn_finalize(srcs, N, HW, C, ones, ones)


def test_conv_stats_into_gn_finalize(ops):
    """The pipeline the networks run: tap-reuse convolution with statistics -> gn_finalize -> y scale + shift against the float64
    GroupNorm of the y that was written."""
    P = bare((9, 64, 64, 32, 160), 7)
    for mfma16 in (0, 1):
        prev = ops.conv_mfma16(mfma16)
        try:
            r = launch(ops, P, (P.b + 100.0).float(), emb="plain")
        finally:
            ops.conv_mfma16(prev)
        assert re.fullmatch(r"conv_bf16x6<5>/tr", r["name"]) and r["chunks"] == 16
        g = torch.Generator().manual_seed(5)
        gamma, beta = torch.randn(160, generator=g), torch.randn(160, generator=g)
        scale, shift = ops.gn_finalize([r["stats"].contiguous()], P.N, 4096, 160, gamma.to(DEV), beta.to(DEV), 1e-5)
        y = r["out"].double().view(P.N, 4096, 160)
        ref = F.group_norm(y.permute(0, 2, 1).cpu(), 32, gamma.double(), beta.double(), 1e-5)
        got = (y * scale.double()[:, None, :] + shift.double()[:, None, :]).permute(0, 2, 1)
        err = rel_l2(got, ref)
        print(f"conv stats -> gn_finalize mfma16={mfma16}: rel-L2 vs fp64 GroupNorm of the written y {err:.3e}")
        assert err < 2e-6


# ---------------------------------------------------------------------------------------------- (f) avg_into_stats
def gn_geom(HW, C):
    """gn_geom of norm.hip: (float4 columns per thread K, pixels per chunk, chunks)"""
    cols = C // 4
    if cols <= 256:
        k, rpi = 1, 256 // cols
    else:
        k = 2
        while cols % k or cols // k > 256:
            k += 1
        rpi = 1
    ppc = max(-(-HW // 256), 32)
    ppc = -(-ppc // rpi) * rpi
    return k, ppc, -(-HW // ppc)


AVG_K = {32: 1, 96: 1, 1280: 2, 2304: 3, 2560: 4}
AVG_ALL = [(ns, bm, div, act) for ns in (1, 2, 4) for bm in (0, 0b0101) for div in (1.0, 4.0) for act in (0, 1)]
AVG_SOME = [(1, 0, 4.0, 1), (2, 0b0101, 1.0, 0), (4, 0b0101, 4.0, 0), (4, 0, 1.0, 1), (2, 0, 4.0, 0), (4, 0b0101, 1.0, 1)]


@pytest.mark.parametrize("HW", [35, 4096])
@pytest.mark.parametrize("C", sorted(AVG_K))
def test_avg_into_stats(ops, C, HW):
    """Every argument combination on the 35-pixel map, a covering half dozen on the 4096-pixel one (K = 1 .. 4 float4 columns per
    thread, ragged last chunk wherever the pixels per chunk do not divide HW)."""
    N, dstC, coff = 2, C + 64, 32
    K, ppc, nchunk = gn_geom(HW, C)
    assert K == AVG_K[C]
    g = torch.Generator(device=DEV).manual_seed(C + HW)
    full = [torch.randn(N, HW, C, generator=g, device=DEV) * 2 + 0.5 for _ in range(4)]
    cols = torch.arange(dstC, device=DEV)
    inside = (cols >= coff) & (cols < coff + C)
    pad = nchunk * ppc - HW
    for ns, bmask, div, act in (AVG_ALL if HW == 35 else AVG_SOME):
        srcs = [full[k][0].contiguous() if (bmask >> k) & 1 else full[k] for k in range(ns)]
        buf0 = sentinel(GUARD + N * HW * dstC + GUARD)
        buf = buf0.clone()
        dst = buf[GUARD:GUARD + N * HW * dstC].view(N, HW, dstC)
        n = N * nchunk * C * 2
        sbuf = nan_stats(n)
        got_chunks = ops.avg_into_stats(srcs, div, N, HW, C, dst, dstC, coff, act, bmask, sbuf[SG:SG + n])
        tag = f"avg_into_stats C={C} HW={HW} sources={ns} bmask={bmask:#x} div={div} act={act}"
        assert got_chunks == nchunk, tag
        part = sbuf[SG:SG + n].view(N, nchunk, C, 2)
        assert bool(torch.isfinite(part).all()) and bool(torch.isnan(sbuf[:SG]).all() and torch.isnan(sbuf[SG + n:]).all()), tag
        chk = buf.clone()
        chk[GUARD:GUARD + N * HW * dstC].view(N, HW, dstC)[..., coff:coff + C] = buf0[GUARD:GUARD + N * HW * dstC].view(N, HW, dstC)[..., coff:coff + C]
        assert torch.equal(chk, buf0), f"{tag}: wrote outside the channel slice"
        assert inside.sum() == C
        s64 = [(t[None].expand(N, -1, -1) if t.dim() == 2 else t).double() for t in srcs]
        ref = sum(s64) / div
        out = dst[..., coff:coff + C]
        if act:
            err = rel_l2(out, F.silu(ref))
            assert err < 2e-6, (tag, err)
        else:
            bound = 4 * U * sum(t.abs() for t in s64) / div
            assert bool(((out.double() - ref).abs() <= bound).all()), tag
        w = F.pad(out.double(), (0, 0, 0, pad)).view(N, nchunk, ppc, C)        # zero rows behind the last chunk add nothing
        s_ref, q_ref, a_ref = w.sum(2), (w * w).sum(2), w.abs().sum(2)
        assert bool(((part[..., 0] - s_ref).abs() <= 1e-12 * a_ref).all()), f"{tag}: sums"
        assert bool(((part[..., 1] - q_ref).abs() <= 1e-12 * q_ref).all()), f"{tag}: sums of squares"


# ---------------------------------------------------------------------------------------------- (g) gn_small
@pytest.mark.parametrize("N,HW,C", [(2, 35, 96), (3, 64, 320), (1, 1024, 1024)])     # 3 channels per group (V = 1), 10 (V = 2), the reach
def test_gn_small(ops, N, HW, C):
    g = torch.Generator().manual_seed(HW + C)
    x = torch.randn(N, C, HW, generator=g) * 3 + 1.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    fs = 2 * C + 8
    fb = torch.full((N, fs), float("nan"))
    fb[:, :2 * C] = torch.randn(N, 2 * C, generator=g) * 0.5
    base = F.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5)
    xd = x.permute(0, 2, 1).contiguous().to(DEV)
    for film in (False, True):
        for silu in (False, True):
            ref = base * (1.0 + fb[:, :C].double()[:, :, None]) + fb[:, C:2 * C].double()[:, :, None] if film else base
            ref = F.silu(ref) if silu else ref
            y = ops.gn_small(xd, gamma.to(DEV), beta.to(DEV), 1e-5, film=fb.to(DEV) if film else None, film_stride=fs if film else 0, silu=silu)
            err = rel_l2(y.permute(0, 2, 1), ref)
            print(f"gn_small N={N} HW={HW} C={C} film={film} silu={silu}: rel-L2 vs fp64 {err:.3e}")
            assert err < 2e-6, (film, silu, err)


def test_gn_small_refuses_beyond_its_reach(ops):
    from diffusion_models_dsdiff_amd import _lib
    for shape, match in (((1, 64, 80), "C % 32"), ((1, 2048, 1024), "reach")):
        x = torch.zeros(*shape, device=DEV)
        ones = torch.ones(shape[2], device=DEV)
        with pytest.raises(_lib.DsdError, match=match):
            ops.gn_small(x, ones, ones)
