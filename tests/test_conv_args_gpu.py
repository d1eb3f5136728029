"""The convolution launch arguments that only the networks set (GPU): batch stride of the input planes (x_bs), asymmetric
padding, row stride of the output (y_ld: a channel slice of the concat tensor), NCHW output, embedding row stride + column
offset, and launches without split-K scratch — on every kernel structure, through dsd_op_conv2d_ex.

Every case asserts: (a) the kernel name the library reports is the structure the case is meant to hit; (b) rel-L2 against
float64 (F.conv2d on the explicitly padded / upsampled input + emb + res) within PREC_TOL of tests/test_ops_gpu.py; (c) the
run is BIT-identical to the plain run of the same data through the same binding (contiguous batch, NHWC, y_ld = Cout,
contiguous emb) whenever both report the same kernel name and split-K factor — these arguments move addresses, not
arithmetic; (d) everything in the output buffer outside the written slice (guard bands in front of and behind it included)
still holds its sentinel.

Shapes start from the smallest cases of test_ops_gpu.py / test_subpixel_gpu.py that reach each kernel.  Where the issue's
shape reports another kernel the shape was changed, not the assertion: (2,64,64,128,96) with the r128 bit runs split-K, so
the r128 row uses Cin = 64; (2,128,128,64,320) with the 256-row bit runs the tap-reuse kernel, so the plain 256-row row uses a
width that is no power of two; (8,64,64,32,160) gets 96-column tiles and no tap reuse, nine samples get the 160-column tile.
y_ld is Cout + 32 (offset 0) and Cout + 64 (offset 32), rounded up to a multiple of 4 where Cout is none (the slice rule).
Those small shapes all get 32-column tiles, so one 24000 x 300 problem adds the wide tiles of every structure, and one stride of
2 GiB + 256 B between the samples adds byte offsets past 2^31 (past 2^32 with three samples: the launch leaves the buffer kernels).
"""
import re

import pytest
import torch
import torch.nn.functional as F

from util import rel_l2
from test_ops_gpu import PREC_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from diffusion_models_dsdiff_amd import ops as m, _lib
    _lib.require_gpu(0)
    return m


class Problem:
    """One convolution problem: fp32 operands and its float64 result (conv + bias), computed once."""

    def __init__(self, N, H, W, Cin, Cout, ks=3, stride=1, ups=False, pad=(-1, -1)):
        self.key = (N, H, W, Cin, Cout, ks, stride, ups, pad)
        self.N, self.H, self.W, self.Cin, self.Cout, self.ks, self.stride, self.ups, self.pad = self.key
        g = torch.Generator().manual_seed(sum(self.key[:7]) + 23)
        self.x = torch.randn(N, Cin, H, W, generator=g)
        self.w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
        self.b = torch.randn(Cout, generator=g)
        xin = F.interpolate(self.x.double(), scale_factor=2, mode="nearest") if ups else self.x.double()
        lo, total = pad if pad[0] >= 0 else (ks // 2, 2 * (ks // 2))
        xin = F.pad(xin, (lo, total - lo, lo, total - lo))
        self.base = F.conv2d(xin, self.w.double(), self.b.double(), stride=stride)      # [N, Cout, OH, OW] float64
        self.OH, self.OW = self.base.shape[2:]
        self.emb = torch.randn(N, Cout, generator=g)
        self.res = torch.randn(N, Cout, self.OH, self.OW, generator=g)

    def ref(self, shared, emb, res):
        r = self.base[:1].expand(self.N, -1, -1, -1) if shared else self.base
        if emb:
            r = r + self.emb.double()[:, :, None, None]
        if res:
            r = r + self.res.double()
        return r


_cache = {"key": None, "prob": None, "plain": {}}


def problem(*key, **kw):
    """The problem and the plain runs made on it are kept while consecutive cases use it (one at a time: memory)."""
    p = Problem(*key, **kw) if _cache["key"] != (key, tuple(sorted(kw.items()))) else _cache["prob"]
    if p is not _cache["prob"]:
        _cache.update(key=(key, tuple(sorted(kw.items()))), prob=p, plain={})
    return p


def sentinel(n):
    return (torch.arange(n, dtype=torch.float32, device=DEV) % 1021) * 0.25 + 1000.0


FAR = 2 ** 29 + 64   # a batch stride whose byte offset (2 GiB + 256) no longer fits a signed 32-bit integer
GUARD = 64   # floats in front of and behind the output buffer (keeps it 16-byte aligned)


def y_layout(P, y):
    """row stride and channel offset of the output slice"""
    if y == "ld":
        return (P.Cout + 32 + 3) // 4 * 4, 0
    if y == "ld_off":
        return (P.Cout + 64 + 3) // 4 * 4, 32
    return P.Cout, 0


def launch(ops, P, x="contig", y="plain", emb=None, res=False, prec="f32", structure="auto", no_scratch=False):
    """x: contig | repeat (sample 0 repeated, contiguous) | shared (x_bs = 0) | strided (x_bs = 2 planes, NaN between them) |
    far (x_bs = FAR, NaN between the planes; built on the device)
    y: plain | ld | ld_off | nchw        emb: None | plain | strided (wider rows, column offset 8, NaN around the columns)
    -> (logical NHWC result, kernel name, split-K factor, sentinels intact)"""
    N, H, W, Cin, Cout = P.N, P.H, P.W, P.Cin, P.Cout
    xl = P.x[:1].expand(N, -1, -1, -1) if x in ("repeat", "shared") else P.x
    xn = xl.permute(0, 2, 3, 1).contiguous()
    plane = H * W * Cin
    if x == "shared":
        xb, x_bs = xn[:1].contiguous().to(DEV), 0
    elif x == "strided":
        x_bs = 2 * plane
        xb = torch.full((N, x_bs), float("nan"))
        xb[:, :plane] = xn.reshape(N, plane)
        xb = xb.to(DEV)
    elif x == "far":
        x_bs = FAR
        xb = torch.full(((N - 1) * x_bs + plane,), float("nan"), device=DEV)
        for n in range(N):
            xb[n * x_bs:n * x_bs + plane] = xn[n].reshape(-1).to(DEV)
    else:
        xb, x_bs = xn.to(DEV), -1
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
    name, ksplit = ops.conv2d_ex(xb, (N, H, W, Cin), P.w.to(DEV), P.b.to(DEV), view(buf), stride=P.stride, upsample=P.ups, emb=e,
                                 res=r, precision=prec, structure=structure, x_batch_stride=x_bs, pad_lo=P.pad[0],
                                 pad_total=P.pad[1], y_ld=ld if y in ("ld", "ld_off") else 0, out_nchw=y == "nchw", emb_stride=es,
                                 no_scratch=no_scratch)
    out = (view(buf).permute(0, 2, 3, 1) if y == "nchw" else view(buf)).contiguous()
    chk = buf.clone()
    view(chk).copy_(view(buf0))
    return out, name, ksplit, torch.equal(chk, buf0)


def check(ops, P, expect, same_kernel=True, bitwise=True, **kw):
    """(a) - (d) for one launch; same_kernel = False: the arguments are meant to divert the launch to another kernel than the
    plain run's, (c) is then asserted only if it did not; bitwise = False: no (c) at all (two kernels under one name)."""
    prec = kw.get("prec", "f32")
    out, name, ksplit, intact = launch(ops, P, **kw)
    assert re.fullmatch(expect, name), f"{P.key} {kw}: ran {name}, expected {expect}"                       # (a)
    err = rel_l2(out.permute(0, 3, 1, 2), P.ref(kw.get("x") in ("repeat", "shared"), kw.get("emb") is not None, kw.get("res", False)))
    print(f"conv_ex {P.key} {kw}: {name} split-K x{ksplit} rel-L2 vs fp64 {err:.3e}")
    assert err < PREC_TOL[prec], (P.key, kw, name, err)                                                     # (b)
    pkw = dict(kw, x="repeat" if kw.get("x") in ("repeat", "shared") else "contig", y="plain", emb="plain" if kw.get("emb") else None)
    pk = tuple(sorted(pkw.items())) + (ops.conv_mfma16(),)
    if pk not in _cache["plain"]:
        _cache["plain"][pk] = launch(ops, P, **pkw)[:3]
    pout, pname, pks = _cache["plain"][pk]
    if same_kernel:
        assert (pname, pks) == (name, ksplit), f"{P.key} {kw}: {name} x{ksplit}, the plain run {pname} x{pks}"
    if bitwise and (pname, pks) == (name, ksplit):
        assert torch.equal(out, pout), f"{P.key} {kw}: {name} differs from its plain run in {int((out != pout).sum())} elements"   # (c)
    assert intact, f"{P.key} {kw}: {name} wrote outside its slice"                                          # (d)
    return name, ksplit


# argument sets
X_BOTH = [dict(x="shared"), dict(x="strided")]
Y_LD = [dict(y="ld"), dict(y="ld_off")]
EPI = [dict(emb="strided"), dict(res=True), dict(y="ld", emb="strided", res=True), dict(y="ld_off", emb="strided", res=True)]
FULL = dict(y="ld", emb="strided", res=True)


def test_direct_cols(ops):
    P = problem(2, 32, 32, 1, 32)
    for kw in [dict()] + X_BOTH + Y_LD + [dict(x="shared", y="ld"), dict(x="strided", y="ld"), dict(x="strided", y="ld_off")] + EPI:
        check(ops, P, r"conv_direct_cols", **kw)
    # NCHW is not this kernel's: the launch goes to the LDS kernel
    check(ops, P, r"conv_direct_lds", same_kernel=False, y="nchw")


def test_direct_lds(ops):
    P = problem(2, 16, 16, 6, 320)     # the latent U-Net's first layer (69 KB of filter in LDS)
    for kw in [dict()] + X_BOTH + Y_LD + [dict(y="nchw"), dict(x="strided", y="ld"), dict(x="shared", y="nchw")] + EPI:
        check(ops, P, r"conv_direct_lds", **kw)


@pytest.mark.parametrize("key,pad", [((1, 4, 4, 6, 5), (-1, -1)), ((2, 4, 4, 6, 5), (0, 1)), ((2, 5, 5, 6, 5), (0, 1)),
                                     ((2, 5, 4, 6, 5), (0, 1)), ((2, 4, 5, 6, 5), (-1, -1))])
def test_scalar(ops, key, pad):
    P = problem(*key, ks=3, stride=2, pad=pad)
    for kw in [dict(), dict(y="nchw")] + Y_LD + X_BOTH + [dict(y="nchw", emb="strided", res=True)] + EPI:
        check(ops, P, r"conv_scalar", **kw)


MFMA_ARGS = [dict()] + Y_LD + X_BOTH + EPI + [dict(x="strided", y="ld"), dict(x="shared", y="ld_off"), dict(y="nchw"),
                                              dict(y="nchw", emb="strided", res=True)]


@pytest.mark.parametrize("key,ks", [((3, 12, 20, 64, 160), 3), ((3, 12, 20, 64, 100), 3), ((2, 8, 8, 96, 32), 1)])
def test_mfma_buffer_loads(ops, key, ks):
    """fp32 MFMA kernel, hardware-range-checked buffer loads (Cin % 32 == 0): ragged M tile (720 rows), ragged N tile (100)."""
    P = problem(*key, ks=ks)
    for kw in MFMA_ARGS:
        check(ops, P, r"conv_mfma<\d>", **kw)


def test_mfma_pointer_loads(ops):
    P = problem(3, 5, 7, 36, 20)       # Cin % 32 != 0: masked K chunk, pointer loads
    for kw in MFMA_ARGS:
        check(ops, P, r"conv_mfma<\d>", **kw)


@pytest.mark.parametrize("cout", [2, 3, 4, 8])
def test_mfma_masked_n_tile_nchw(ops, cout):
    """The last layer with out_channels > 1: one masked N tile, every tile on the edge path."""
    P = problem(3, 16, 16, 320, cout)
    for kw in [dict(), dict(y="nchw"), dict(y="nchw", x="strided"), dict(y="nchw", res=True)]:
        check(ops, P, r"conv_mfma<1>", **kw)


# structure bit -> name suffix (conv2d_route_name): the 256-row A-direct kernel keeps the plain name
SUFFIX = {"staged": "/staged", "adirect": "/r128", "adirect256": ""}
SPLIT_SHAPES = {"staged": ((2, 16, 16, 64, 64), 2), "adirect": ((2, 64, 64, 64, 96), 1), "adirect256": ((3, 40, 24, 64, 320), 1)}


@pytest.mark.parametrize("structure", ["staged", "adirect", "adirect256"])
def test_split_structures(ops, structure):
    key, stride = SPLIT_SHAPES[structure]
    P = problem(*key, stride=stride)
    name = r"conv_bf16x6<\d>" + SUFFIX[structure]
    for kw in [dict()] + Y_LD + [dict(x="strided"), dict(x="shared")] + EPI + [dict(x="strided", **FULL)]:
        check(ops, P, name, prec="bf16x6", structure=structure, **kw)
    for prec in ("f16x3", "bf16x3"):
        check(ops, P, r"conv_%s<\d>" % prec + SUFFIX[structure], prec=prec, structure=structure, **FULL)


@pytest.mark.parametrize("prec,structure,name", [("f32", "auto", r"conv_mfma<[2-5]>"), ("bf16x6", "staged", r"conv_bf16x6<5>/staged"),
                                                 ("bf16x6", "adirect", r"conv_bf16x6<5>/r128"), ("bf16x6", "adirect256", r"conv_bf16x6<5>")])
def test_wide_column_tiles(ops, prec, structure, name):
    """The small shapes above all get 32-column tiles (the planner narrows tiles until the grid fills the chip).  A grid of more
    than 512 tiles keeps the wide ones: 24000 rows (ragged last row tile for both tile heights), 300 columns (ragged last
    column tile), a width that keeps the 256-row launch off the tap-reuse kernel."""
    P = problem(2, 125, 96, 64, 300)
    for kw in [dict(), FULL, dict(y="ld_off", emb="strided", res=True), dict(x="strided"), dict(y="nchw", emb="strided", res=True)]:
        check(ops, P, name, prec=prec, structure=structure, **kw)


@pytest.mark.parametrize("cout", [4, 8, 100])
@pytest.mark.parametrize("structure", ["staged", "adirect", "adirect256"])
def test_split_structures_nchw(ops, structure, cout):
    key, stride = SPLIT_SHAPES[structure]
    P = problem(*key[:4], cout, stride=stride)
    for kw in [dict(), dict(y="nchw"), dict(y="nchw", emb="strided", res=True), dict(y="nchw", x="strided")]:
        check(ops, P, r"conv_bf16x6<\d>" + SUFFIX[structure], prec="bf16x6", structure=structure, **kw)


@pytest.mark.parametrize("hw", [(16, 16), (15, 17)])
@pytest.mark.parametrize("structure", ["staged", "adirect", "adirect256"])
def test_split_structures_asym_pad_stride2(ops, structure, hw):
    """The VAE's Downsample: no padding in front, one zero row / column behind, stride 2."""
    P = problem(2, hw[0], hw[1], 64, 64, stride=2, pad=(0, 1))
    for kw in [dict(), dict(y="ld"), dict(x="strided", y="ld_off"), dict(y="nchw")]:
        check(ops, P, r"conv_bf16x6<\d>" + SUFFIX[structure], prec="bf16x6", structure=structure, **kw)


@pytest.mark.parametrize("key", [(2, 8, 8, 320, 100), (1, 8, 8, 960, 960)])
def test_split_k(ops, key):
    """Split-K: the reduction kernel has an epilogue of its own (y_ld, NCHW, emb, res)."""
    P = problem(*key)
    for kw in [dict()] + Y_LD + [dict(y="nchw"), dict(y="nchw", emb="strided", res=True), dict(x="strided", **FULL)] + EPI:
        name, ks = check(ops, P, r"conv_bf16x6<\d>/r128\+splitk", prec="bf16x6", **kw)
        assert ks > 1, (key, kw, ks)
    _, ks = check(ops, P, r"conv_bf16x3<\d>/r128\+splitk", prec="bf16x3", **FULL)
    assert ks > 1
    _, ks = check(ops, P, r"conv_f16x3<\d>/r128\+splitk", prec="f16x3", structure="adirect", **FULL)
    assert ks > 1
    # without scratch the launch is unsplit and named so, and still within the bar
    for kw in [dict(), FULL, dict(y="nchw")]:
        _, ks = check(ops, P, r"conv_bf16x6<\d>/r128", prec="bf16x6", no_scratch=True, **kw)
        assert ks == 1, (key, kw, ks)


TR_SHAPES = [
    # N, H, W, Cin, Cout, ups, the name with the 32x32x16 MFMA shape, the name with 16x16x32
    (9, 64, 64, 32, 160, False, "/tr", "/tr"),
    (2, 128, 128, 64, 320, False, "/tr", "/tr"),
    (2, 128, 128, 64, 300, False, "/tr", "/tr"),            # a ragged second column tile (300 = 160 + 140)
    (1, 256, 256, 64, 128, False, "/tr", "/tr"),            # the 128-column tile (the 16x16x32 build has none: same kernel)
    (2, 64, 64, 32, 320, True, "/tr\\+subpixel", "/tr"),    # folded nearest x2: tap reuse only where the sub-pixel form is off
]


@pytest.mark.parametrize("case", TR_SHAPES)
def test_tap_reuse(ops, case):
    N, H, W, Cin, Cout, ups, n32, n16 = case
    P = problem(N, H, W, Cin, Cout, ups=ups)
    for mfma16 in (0, 1):
        prev = ops.conv_mfma16(mfma16)
        try:
            name = r"conv_bf16x6<\d>" + (n16 if mfma16 else n32)
            for kw in [dict(), FULL, dict(y="ld_off", emb="strided", res=True), dict(x="strided"), dict(x="shared", y="ld")]:
                check(ops, P, name, prec="bf16x6", **kw)
            # NCHW output is not the tap-reuse kernel's: the launch diverts to the plain 256-row kernel and stays correct
            check(ops, P, r"conv_bf16x6<\d>", same_kernel=False, prec="bf16x6", y="nchw", emb="strided", res=True)
        finally:
            ops.conv_mfma16(prev)


def test_tap_reuse_asym_pad_diverts(ops):
    P = problem(2, 128, 128, 64, 320, pad=(0, 1))
    for mfma16 in (0, 1):
        prev = ops.conv_mfma16(mfma16)
        try:
            for kw in [dict(), FULL]:
                check(ops, P, r"conv_bf16x6<\d>", prec="bf16x6", **kw)
        finally:
            ops.conv_mfma16(prev)


def test_subpixel(ops):
    P = problem(2, 16, 64, 64, 160, ups=True)
    for kw in [dict(), FULL, dict(y="ld_off", emb="strided", res=True), dict(x="strided"), dict(x="shared"), dict(x="strided", **FULL)]:
        check(ops, P, r"conv_bf16x6<5>/tr\+subpixel", prec="bf16x6", **kw)
    # NCHW output: the folded gather instead
    check(ops, P, r"conv_bf16x6<\d>", same_kernel=False, prec="bf16x6", y="nchw")


@pytest.mark.parametrize("key", [(1, 64, 64, 64, 128), (3, 44, 32, 64, 192)])
def test_winograd(ops, key):
    P = problem(*key)
    for kw in [dict(), FULL, dict(y="ld_off", emb="strided", res=True), dict(x="strided"), dict(x="shared", y="ld")]:
        check(ops, P, r"conv_wino_bf16x6", prec="bf16x6", structure="winograd", **kw)
    # the weights are packed before the output layout is known (as in the planner): an NCHW launch takes the direct kernel
    check(ops, P, r"conv_bf16x6<\d>", same_kernel=False, prec="bf16x6", structure="winograd", y="nchw")


FAR_CASES = [
    # problem, its keywords, precision, structure, kernel
    ((2, 8, 8, 96, 32), dict(ks=1), "f32", "auto", r"conv_mfma<1>"),
    ((2, 5, 7, 36, 20), dict(), "f32", "auto", r"conv_mfma<1>"),
    ((2, 16, 16, 6, 320), dict(), "f32", "auto", r"conv_direct_lds"),
    ((2, 32, 32, 1, 32), dict(), "f32", "auto", r"conv_direct_cols"),
    ((2, 16, 16, 64, 64), dict(stride=2), "bf16x6", "staged", r"conv_bf16x6<1>/staged"),
    ((2, 16, 16, 64, 64), dict(stride=2), "bf16x6", "adirect", r"conv_bf16x6<1>/r128"),
    ((2, 16, 16, 64, 64), dict(stride=2), "bf16x6", "adirect256", r"conv_bf16x6<1>"),
    ((2, 128, 128, 64, 320), dict(), "bf16x6", "auto", r"conv_bf16x6<5>/tr"),
    ((2, 16, 64, 64, 160), dict(ups=True), "bf16x6", "auto", r"conv_bf16x6<5>/tr\+subpixel"),
    ((2, 32, 64, 32, 320), dict(), "bf16x6", "winograd", r"conv_wino_bf16x6"),
]


@pytest.mark.parametrize("key,pkw,prec,structure,name", FAR_CASES)
def test_batch_stride_past_2_gib(ops, key, pkw, prec, structure, name):
    """The second sample 2 GiB + 256 B behind the first: the buffer-load kernels address it with unsigned 32-bit byte offsets
    (conv2d_split_eligible keeps the whole extent below 4 GiB), the others with 64-bit pointers."""
    P = problem(*key, **pkw)
    for kw in [dict(x="far"), dict(x="far", **FULL)]:
        check(ops, P, name, prec=prec, structure=structure, **kw)


def test_batch_extent_past_4_gib_leaves_the_buffer_kernels(ops):
    """Three samples at that stride are more than a buffer descriptor spans: the launch goes to the fp32 kernel with pointer loads,
    whatever mode was asked for.  (The name is also that of the buffer-load kernel the plain fp32 run takes: no bit comparison.)"""
    P = problem(3, 16, 16, 64, 64, stride=2)
    for prec in ("f32", "bf16x6"):
        check(ops, P, r"conv_mfma<1>", same_kernel=False, bitwise=False, prec=prec, x="far", **FULL)


@pytest.mark.parametrize("prec", ["f32", "bf16x6"])
@pytest.mark.parametrize("T,Cin,Cout", [(96, 64, 96), (100, 64, 100), (96, 96, 64)])
def test_tall_1x1_as_gemm(ops, T, Cin, Cout, prec):
    """The VAE attention's A @ B^T: a 1x1 convolution on a T x 1 map, no bias, no scratch."""
    g = torch.Generator().manual_seed(T + Cin + Cout)
    A, B = torch.randn(T, Cin, generator=g), torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    ref = A.double() @ B.double().T
    buf0 = sentinel(GUARD + T * Cout + GUARD)
    buf = buf0.clone()
    Y = buf[GUARD:GUARD + T * Cout].view(T, Cout)
    name, ks = ops.conv2d_ex(A.to(DEV), (1, T, 1, Cin), B.view(Cout, Cin, 1, 1).to(DEV), None, Y, precision=prec, no_scratch=True)
    assert re.fullmatch(r"conv_mfma<\d>" if prec == "f32" else r"conv_bf16x6<\d>/r128", name), name
    assert ks == 1
    err = rel_l2(Y, ref)
    print(f"gemm_nt T={T} K={Cin} N={Cout} {prec}: {name} rel-L2 vs fp64 {err:.3e}")
    assert err < PREC_TOL[prec]
    chk = buf.clone()
    chk[GUARD:GUARD + T * Cout] = buf0[GUARD:GUARD + T * Cout]
    assert torch.equal(chk, buf0)


def test_argument_checks_launch_nothing(ops):
    from diffusion_models_dsdiff_amd import _lib
    N, H, W, Cin, Cout = 1, 8, 8, 32, 32
    x = torch.randn(N, H, W, Cin).to(DEV)
    w, b = torch.randn(Cout, Cin, 3, 3).to(DEV), torch.zeros(Cout).to(DEV)
    buf0 = sentinel(N * H * W * 72 + 8)
    buf = buf0.clone()
    body = buf[:N * H * W * 72].view(N, H, W, 72)
    emb = torch.zeros(N, 72).to(DEV)
    bad = [
        dict(y=body[..., :Cout], y_ld=16),                                  # y_ld < Cout
        dict(y=body[..., :Cout], y_ld=70),                                  # a slice's row stride must be a multiple of 4
        dict(y=body[..., 2:2 + Cout], y_ld=72),                             # slice pointer not 16-byte aligned
        dict(y=buf[1:1 + N * H * W * Cout]),                                # plain output, misaligned
        dict(y=body[..., :Cout], y_ld=72, out_nchw=True),                   # NCHW has no row stride
        dict(y=body[..., :Cout], y_ld=72, emb=emb, emb_stride=16),          # emb_stride < Cout
        dict(y=body[..., :Cout], y_ld=72, emb=emb[:, 2:], emb_stride=72),   # emb column offset not 16-byte aligned
        dict(y=body[..., :Cout], y_ld=72, x_batch_stride=H * W * Cin - 4),  # between 0 and one plane
        dict(y=body[..., :Cout], y_ld=72, pad_lo=0, pad_total=-1),          # half a padding
    ]
    for prec in ("f32", "bf16x6"):
        for kw in bad:
            kw = dict(kw)
            y = kw.pop("y")
            with pytest.raises(_lib.DsdError):
                ops.conv2d_ex(x, (N, H, W, Cin), w, b, y, precision=prec, **kw)
            torch.cuda.synchronize()
            assert torch.equal(buf, buf0), kw
    # and the same buffer with good arguments is written
    name, _ = ops.conv2d_ex(x, (N, H, W, Cin), w, b, body[..., 32:64], y_ld=72, emb=emb[:, 8:], emb_stride=72)
    assert not torch.equal(buf, buf0)
    assert torch.equal(body[..., :32], buf0[:N * H * W * 72].view(N, H, W, 72)[..., :32])
