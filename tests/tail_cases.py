"""Inputs and references of test_tail_kernels_gpu.py (plain torch on the CPU: importing and calling these needs no GPU).

Every builder draws from seeded CPU generators.  A reference is ONE torch expression `fn`, evaluated twice on the same inputs:
in float64 (`ref64`) and in float32 (`cpu32`, the reference's own arithmetic) — see `three`.
"""
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24                       # one fp32 rounding, relative
CAP = 65535 * 256                      # elements one pass of a grid capped at 65535 blocks covers
WRAP = CAP + 1027                      # cap plus a ragged tail (a prime: only the flat kernels can have exactly this count)
AVG_WRAP4 = 256 * 32 * 256 + 515       # avg_into's own cap (256*32 blocks), in float4


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=gen(seed)) * scale + shift


def three(fn, *tensors):
    """(ref64, cpu32) of one torch expression; integer tensors pass through unchanged"""
    def conv(dt):
        return [t.to(dt) if torch.is_tensor(t) and t.is_floating_point() else t for t in tensors]
    return fn(*conv(torch.float64)), fn(*conv(torch.float32))


# ------------------------------------------------------------------------------------------------ pure data movement
TRANSPOSE_SHAPES = [(3, 5, 7), (2, 320, 35), (1, 4, 1)]                      # (N, C, HW)
TRANSPOSE_WRAP = (3, 7, 798953)                                              # 16778013 = CAP + 1053
UPSAMPLE_SHAPES = [(2, 3, 5, 4), (1, 1, 1, 8), (3, 6, 2, 36)]                # (N, H, W, C)
UPSAMPLE_WRAP = (1, 2050, 2047, 4)                                           # 4 H W = 16785400 float4 out = CAP + 8440
PATCH_SHAPES = [(2, 3, 8, 12, 2), (1, 4, 6, 6, 1), (2, 1, 16, 8, 8), (1, 5, 9, 6, 3)]   # (N, C, H, W, p); h != w in three of them
PATCH_WRAP = (1, 3, 2366, 2364, 2)                                           # 16779672 = CAP + 2712


def nchw_to_nhwc_ref(x):               # [N, C, HW] -> [N, HW, C]
    return x.permute(0, 2, 1).contiguous()


def upsample2_ref(x):                  # NHWC, nearest x2
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()


def patchify_ref(x, p):
    """[N, C, H, W] -> [N, (H/p)(W/p), C p p], token channels in Conv2d weight order (c, ph, pw): F.unfold's own order"""
    return F.unfold(x, kernel_size=p, stride=p).transpose(1, 2).contiguous()


def unpatchify_ref(t, c, h, w, p):
    """DiT.unpatchify: tokens [N, h w, p p c] (order ph, pw, c) -> [N, c, h p, w p]"""
    x = t.reshape(t.shape[0], h, w, p, p, c)
    return torch.einsum("nhwpqc->nchpwq", x).reshape(t.shape[0], c, h * p, w * p).contiguous()


# ------------------------------------------------------------------------------------------------ casts
def cast_vector(bf16, seed=11):
    """fp32 values for cast16, the special ones first: exact ties in both directions, the largest finite value and the first
    that rounds to inf, the fp16 subnormal range down to below half its smallest subnormal, +-0, +-inf, NaN; then normals."""
    mant = 7 if bf16 else 10
    h = 2.0 ** -(mant + 1)                                     # half an ulp of 1.0 in the 16-bit type
    if bf16:
        top = (2.0 - 2.0 ** -7) * 2.0 ** 127                   # largest finite bf16
        over = (2.0 - 2.0 ** -8) * 2.0 ** 127                  # the tie between it and 2^128: rounds (to even) to inf
    else:
        top, over = 65504.0, 65520.0
    sp = [1.0 + h, 1.0 + 3 * h, 1.0 + 5 * h, 1.0 + 7 * h,      # ties: down to even, up to even, down, up
          1.0 + h * (1 + 2.0 ** -12), 1.0 + h * (1 - 2.0 ** -12),   # just above / below a tie
          1.0 + 3 * h * (1 + 2.0 ** -13), 1.0 + 3 * h * (1 - 2.0 ** -13),
          top, over, top * (1 + 2.0 ** -12), 1e5, 3e38,
          2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -24, 2.0 ** -24, 1e-6, 6e-8,     # fp16: smallest normal, subnormals
          2.0 ** -15 + 2.0 ** -25, 2.0 ** -15 + 3 * 2.0 ** -25,               # ties inside the subnormal range
          2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -25 * (1 - 2.0 ** -20), 2.0 ** -26, 1e-9, 1e-30]
    sp = sp + [-v for v in sp] + [0.0, -0.0, float("inf"), -float("inf"), float("nan")]
    v = torch.cat([torch.tensor(sp, dtype=torch.float64).float(), randn(1200, seed), randn(300, seed + 1, 300.0), randn(300, seed + 2, 1e-4)])
    over32 = torch.tensor(over, dtype=torch.float64).float()
    assert float(over32) == over and torch.isinf(over32.to(torch.bfloat16 if bf16 else torch.float16))
    assert len(sp) < 255
    return v


def int_blocks(n, seed, amp):
    """n small integers as float32, cheap at 10^8: sixteen copies of one random block in [-amp, amp], copy k shifted by 3 k"""
    m = (n + 15) // 16
    base = torch.randint(-amp, amp + 1, (m,), generator=gen(seed), dtype=torch.int16).float()
    return (base[None, :] + torch.arange(16, dtype=torch.float32)[:, None] * 3).reshape(-1)[:n].contiguous()


def tiled(v, n):
    return v.repeat((n + v.numel() - 1) // v.numel())[:n].contiguous()


def same_bits(a, b):
    """bit equality of two tensors of one dtype, NaNs compared by NaN-ness only"""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.view(it)[~na], b.view(it)[~nb])


CAST_SIZES = [1, 255, 257]


# ------------------------------------------------------------------------------------------------ one-rounding arithmetic
AVGPOOL_SHAPES = [(2, 2, 2, 4), (1, 6, 10, 36), (3, 4, 2, 8)]               # (N, H, W, C)
AVGPOOL_WRAP = (1, 4098, 16378, 4)                                           # 2049 * 8189 = 16779261 float4 out = CAP + 2301
GATED_SHAPES = [(2, 5, 8), (3, 7, 36), (1, 1, 4)]                            # (N, T, C)
GATED_WRAP = (3, 5592663, 4)                                                 # N T = 16777989 float4 = CAP + 1029
# (nsrc, div, C, coff, bmask): 1..4 sources, div in {1, 2, 4, 3}, C in {4, 36}, coff in {0, 32}, bmask in {0, 1, 2, 5, 15}
AVG_CASES = [(1, 1.0, 4, 0, 0), (1, 1.0, 36, 32, 1), (2, 2.0, 36, 0, 2), (2, 2.0, 4, 32, 1), (2, 3.0, 36, 32, 0),
             (3, 3.0, 36, 32, 5), (3, 3.0, 4, 0, 0), (3, 4.0, 4, 32, 2), (4, 4.0, 36, 0, 15), (4, 4.0, 4, 32, 5),
             (4, 4.0, 36, 32, 0), (4, 3.0, 36, 0, 2), (4, 1.0, 4, 0, 1)]
AVG_SILU_CASES = [(1, 1.0, 4, 0, 0), (2, 2.0, 36, 32, 1), (4, 4.0, 36, 32, 5), (4, 3.0, 4, 0, 15)]
AVG_N, AVG_H, AVG_W = 3, 3, 5


def avgpool_parts(x):
    """the four taps of AvgPool2d(2, 2) on NHWC, in the kernel's order"""
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def avg_sources(nsrc, C, bmask, seed, N=AVG_N, HW=AVG_H * AVG_W):
    """full [N, HW, C] sources; a source whose bmask bit is set is the same sample for the whole batch"""
    out = []
    for k in range(nsrc):
        s = randn((N, HW, C), seed + k, 1.0 + k)
        if bmask >> k & 1:
            s = s[:1].expand(N, HW, C).contiguous()
        out.append(s)
    return out


def avg_ref(srcs, div, silu=False):
    v = srcs[0]
    for s in srcs[1:]:
        v = v + s
    v = v / div
    return F.silu(v) if silu else v


# ------------------------------------------------------------------------------------------------ transcendental / reductions
def act_pool(seed=21):
    """a grid over [-12, 12], +-0, +-1e-30, +-88 and random normals; the special values first"""
    sp = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0])
    grid = torch.linspace(-12.0, 12.0, 1921)
    grid = grid[torch.randperm(grid.numel(), generator=gen(seed))]
    return torch.cat([sp, grid, randn(1073, seed + 1)])          # 3000 values


GEGLU_SHAPES = [(3, 5), (2, 1280), (1, 1)]                                   # (rows, inner)
GEGLU_WRAP = (13, 1290615)                                                   # 16777995 = CAP + 1035


def gelu_tanh_ref(x):
    return F.gelu(x, approximate="tanh")


def geglu_ref(x):                                                            # rows of [a | gate]
    a, g = x.chunk(2, dim=-1)
    return a * F.gelu(g)


def geglu_input(rows, inner, seed=31):
    n = rows * inner
    gate = tiled(act_pool(seed), n).reshape(rows, inner)
    return torch.cat([randn((rows, inner), seed + 5), gate], dim=1).contiguous()


SOFTMAX_SHAPES = [(3, 1), (2, 63), (5, 256), (3, 257), (2, 1000), (1, 4096)]  # (rows, cols)
SOFTMAX_SCALES = [1.0, 0.0625, -1.5]


def softmax_rows_special(rows, cols):
    """(spike row, all-equal row) of a case, None where the case has no such row; row 0 is always an ordinary random row"""
    return (rows - 1 if rows >= 2 and cols > 1 else None), (1 if rows >= 3 else None)


def softmax_input(rows, cols, scale, seed=41):
    """spike row: the scaled logit at column cols // 3 exceeds every other by 100 (the others' exponentials underflow);
    all-equal row: one value throughout"""
    x = randn((rows, cols), seed + cols, 3.0)
    spike, equal = softmax_rows_special(rows, cols)
    if spike is not None:
        j = cols // 3
        others = torch.cat([x[spike, :j], x[spike, j + 1:]]) * scale
        x[spike, j] = (float(others.max()) + 100.0) / scale
    if equal is not None:
        x[equal] = x[equal, 0]
    return x


def softmax_ref(x, scale):
    return torch.softmax(x * scale, dim=-1)


LAYER_NORM_SHAPES = [(1, 4), (5, 63), (4, 64), (7, 65), (3, 320), (2, 1280)]  # (rows, C)
LAYER_NORM_KINDS = [(1e-5, "unit"), (1e-6, "offset"), (1e-6, "unit"), (1e-5, "offset")]


def layer_norm_input(rows, C, kind, seed=51):
    """offset: every row has mean 1000 and standard deviation 1 (what the two-pass variance is for)"""
    x = randn((rows, C), seed + C) + 1000.0 if kind == "offset" else randn((rows, C), seed + C, 2.0, 0.5)
    return x, randn((C,), seed + 1, 1.0, 1.0), randn((C,), seed + 2)


def layer_norm_ref(x, gamma, beta, eps):
    return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


LN_MOD_SHAPES = [(2, 3, 64), (1, 5, 100), (3, 1, 768), (2, 6, 1152)]          # (N, T, C)
LN16_WIDTHS = [4, 64, 256, 260, 512, 768, 1024, 1152, 1280, 1284, 1792, 2048]


def ln_mod_layout(C, aligned):
    """(mod_stride, shift_off, scale_off): a padded row and two distinct offsets that are not multiples of C (the 16-bit kernel
    reads them as float4, so there they are multiples of 4)"""
    return (6 * C + 8, C + 4, 3 * C + 8) if aligned else (6 * C + 4, 2 * C + 3, 4 * C + 1)


def ln_mod_input(N, T, C, aligned, seed=61):
    stride, sh, sc = ln_mod_layout(C, aligned)
    return randn((N, T, C), seed + C, 1.5, 0.7), randn((N, stride), seed + 1, 0.5)


def ln_mod_ref(x, mod, C, aligned, eps):
    _, sh, sc = ln_mod_layout(C, aligned)
    return F.layer_norm(x, (C,), eps=eps) * (1 + mod[:, None, sc:sc + C]) + mod[:, None, sh:sh + C]


def ulp16(v, bf16):
    """spacing of the 16-bit type at v (float64 tensor)"""
    mant, emin = (7, -126) if bf16 else (10, -14)
    e = torch.frexp(v.abs())[1].double() - 1
    e = torch.where(v == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.exp2(e - mant)


def frac_beyond_one_ulp(a16, b16, bf16):
    """share of the elements of a16 that are more than one 16-bit ulp (of b16) away from b16"""
    a, b = a16.double(), b16.double()
    return float(((a - b).abs() > ulp16(b, bf16)).double().mean())


SE_SHAPES = [(2, 1, 32, 2), (3, 35, 320, 20), (1, 4096, 64, 4), (2, 9, 260, 16)]   # (N, HW, C, Cr)


def se_input(N, HW, C, Cr, seed=71):
    """per-channel offsets keep the pooled means away from 0; w1 of both signs drives some hidden units negative (ReLU clamps
    them) and the large w2 saturates some gates (the builder asserts both)"""
    x = randn((N, HW, C), seed + C) + randn((1, 1, C), seed + 1, 2.0)
    w1 = randn((Cr, C), seed + 2, C ** -0.5)
    w2 = randn((C, Cr), seed + 3, 12.0)
    pre = x.double().mean(1) @ w1.double().t()
    gate = torch.sigmoid(torch.relu(pre) @ w2.double().t())
    assert bool((pre < 0).any()) and bool((pre > 0).any()) and bool((gate > 0.999).any()) and bool((gate < 0.001).any())
    return x, w1, w2


def se_ref(x, w1, w2):
    hid = torch.relu(x.mean(dim=1) @ w1.t())
    return x * torch.sigmoid(hid @ w2.t())[:, None, :]


def maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0
