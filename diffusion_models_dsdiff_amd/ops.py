"""Kernel-level entry points (dsd_op_*) on torch CUDA tensors — used by tests and micro-benchmarks.

Activations cross this boundary as NHWC; helpers convert from the reference's NCHW.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import lib, check, dptr, stream_ptr, DsdConvEx, DsdConvGn


def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16x6": 2, "f16x3": 3}   # the convolution modes (f16 / bf16 are DiT-handle modes)


STRUCTURES = {"auto": 0, "adirect": 16, "staged": 32, "adirect256": 64, "winograd": 128}


def conv2d(x_nhwc, w_oihw, bias, stride=1, upsample=False, emb=None, res=None, precision="f32", structure="auto"):
    N, H, W, Cin = x_nhwc.shape
    Cout, _, ks, _ = w_oihw.shape
    IH, IW = (H * 2, W * 2) if upsample else (H, W)
    pad = ks // 2
    OH, OW = (IH + 2 * pad - ks) // stride + 1, (IW + 2 * pad - ks) // stride + 1
    y = torch.empty((N, OH, OW, Cout), device=x_nhwc.device, dtype=torch.float32)
    check(lib().dsd_op_conv2d_prec(dptr(x_nhwc), N, H, W, Cin, dptr(w_oihw.contiguous()), dptr(bias), Cout, ks, stride,
                                   int(upsample), dptr(emb), dptr(res), PRECISIONS[precision] | STRUCTURES[structure],
                                   dptr(y), stream_ptr()))
    return y


def conv_out_hw(H, W, ks, stride=1, upsample=False, pad_total=-1):
    IH, IW = (H * 2, W * 2) if upsample else (H, W)
    pt = pad_total if pad_total >= 0 else 2 * (ks // 2)
    return (IH + pt - ks) // stride + 1, (IW + pt - ks) // stride + 1


def conv2d_ex(x, shape, w_oihw, bias, y, stride=1, upsample=False, emb=None, res=None, precision="f32", structure="auto",
              x_batch_stride=-1, pad_lo=-1, pad_total=-1, y_ld=0, out_nchw=False, emb_stride=0, no_scratch=False):
    """The convolution with the launch arguments only the networks set (dsd_op_conv2d_ex).  x: any contiguous fp32 CUDA tensor
    holding the planes (`shape` = (N, H, W, Cin) says how it is read, x_batch_stride how far the samples lie apart); y: the
    caller's output buffer, written in place — a channel slice of a wider NHWC tensor is passed as the (non-contiguous) view
    buf[..., c0:c0 + Cout] with y_ld = buf.shape[-1], emb likewise as a column view with emb_stride.  Returns (kernel name,
    split-K factor) of the launch."""
    N, H, W, Cin = shape
    Cout, _, ks, _ = w_oihw.shape
    ex = DsdConvEx(x_batch_stride=int(x_batch_stride), pad_lo=pad_lo, pad_total=pad_total, y_ld=int(y_ld), out_nchw=int(out_nchw),
                   emb_stride=int(emb_stride), no_scratch=int(no_scratch), ksplit=0)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # views: the pointer of the first element
    assert x.is_cuda and x.is_contiguous() and y.is_cuda and (res is None or res.is_contiguous())
    check(lib().dsd_op_conv2d_ex(ptr(x), N, H, W, Cin, dptr(w_oihw.contiguous()), dptr(bias), Cout, ks, stride, int(upsample),
                                 ptr(emb), dptr(res), PRECISIONS[precision] | STRUCTURES[structure], C.byref(ex), ptr(y),
                                 stream_ptr()))
    return ex.kernel.decode(), ex.ksplit


def conv2d_gn(x, shape, w_oihw, bias, y, gn_scale=None, gn_shift=None, stats=None, query=False, stride=1, upsample=False, emb=None,
              res=None, precision="f32", structure="auto", x_batch_stride=-1, pad_lo=-1, pad_total=-1, y_ld=0, out_nchw=False,
              emb_stride=0, no_scratch=False):
    """conv2d_ex with the GroupNorm arguments (dsd_op_conv2d_gn): gn_scale / gn_shift [N, Cin] fp32 — the kernel then computes
    conv(silu(x * scale + shift)) —, stats: a float64 CUDA tensor (or view) that receives [N, chunks, Cout, 2] (sum, sum of
    squares) of the output; query=True launches nothing.  Returns (kernel name, split-K factor, chunks per sample the kernel
    of these arguments emits: size stats from a query)."""
    N, H, W, Cin = shape
    Cout, _, ks, _ = w_oihw.shape
    ex = DsdConvEx(x_batch_stride=int(x_batch_stride), pad_lo=pad_lo, pad_total=pad_total, y_ld=int(y_ld), out_nchw=int(out_nchw),
                   emb_stride=int(emb_stride), no_scratch=int(no_scratch), ksplit=0)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    assert x.is_cuda and x.is_contiguous() and y.is_cuda and (res is None or res.is_contiguous())
    assert stats is None or (stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous())
    for t in (gn_scale, gn_shift):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (N, Cin))
    gn = DsdConvGn(gn_scale=None if gn_scale is None else gn_scale.data_ptr(), gn_shift=None if gn_shift is None else gn_shift.data_ptr(),
                   stats=None if stats is None else stats.data_ptr(), stats_doubles=0 if stats is None else stats.numel(),
                   stats_chunks=0, query=int(query))
    check(lib().dsd_op_conv2d_gn(ptr(x), N, H, W, Cin, dptr(w_oihw.contiguous()), dptr(bias), Cout, ks, stride, int(upsample),
                                 ptr(emb), dptr(res), PRECISIONS[precision] | STRUCTURES[structure], C.byref(ex), C.byref(gn), ptr(y),
                                 stream_ptr()))
    return ex.kernel.decode(), ex.ksplit, gn.stats_chunks


def gn_finalize(srcs, N, HW, C_, gamma, beta, eps=1e-5, film=None, film_stride=0):
    """gn_finalize on caller-supplied statistics (dsd_op_gn_finalize).  srcs: one or two float64 CUDA tensors [N, chunks, c, 2]
    (sum, sum of squares per chunk and column), the second covering the channels behind the first; film: [N, film_stride] fp32
    (scale in columns [0, C), shift in [C, 2C)).  Returns (scale, shift), [N, C] each."""
    assert 1 <= len(srcs) <= 2
    for t in srcs:
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 4 and t.shape[0] == N and t.shape[3] == 2
    p1 = srcs[1] if len(srcs) == 2 else None
    scale = torch.empty((N, C_), device=srcs[0].device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    check(lib().dsd_op_gn_finalize(C.c_void_p(srcs[0].data_ptr()), srcs[0].shape[1], srcs[0].shape[2],
                                   None if p1 is None else C.c_void_p(p1.data_ptr()), 0 if p1 is None else p1.shape[1],
                                   0 if p1 is None else p1.shape[2], N, HW, C_, dptr(gamma), dptr(beta), eps, dptr(film),
                                   int(film_stride), dptr(scale), dptr(shift), stream_ptr()))
    return scale, shift


def avg_into_stats(srcs, div, N, HW, C_, dst, dstC, coff, act, bmask, partial):
    """dst[..., coff:coff + C] = act(sum(srcs) / div) and the statistics of what was written (dsd_op_avg_into_stats).  srcs: 1 to
    4 contiguous fp32 CUDA tensors [N, HW, C] ([HW, C] where bit k of bmask is set); dst: the tensor (or view) whose first element
    is row 0, column 0 of the [N * HW, dstC] destination; partial: a float64 CUDA tensor (or view) with room for
    [N, chunks, C, 2].  Returns the chunk count the statistics were written with."""
    assert 1 <= len(srcs) <= 4 and dst.is_cuda and partial.is_cuda and partial.dtype == torch.float64 and partial.is_contiguous()
    p = [dptr(t) for t in srcs] + [None] * (4 - len(srcs))
    n = C.c_int(0)
    check(lib().dsd_op_avg_into_stats(p[0], p[1], p[2], p[3], float(div), N, HW, C_, C.c_void_p(dst.data_ptr()), dstC, coff,
                                      int(act), int(bmask), C.c_void_p(partial.data_ptr()), partial.numel(), C.byref(n),
                                      stream_ptr()))
    return n.value


def gn_small(x_nhwc, gamma, beta, eps=1e-5, film=None, film_stride=0, silu=False):
    """GroupNorm32 (+ FiLM, + SiLU) of a small map in one launch (dsd_op_gn_small), x [N, H, W, C] or [N, HW, C]."""
    N, Cc = x_nhwc.shape[0], x_nhwc.shape[-1]
    HW = x_nhwc.numel() // (N * Cc)
    y = torch.empty_like(x_nhwc)
    check(lib().dsd_op_gn_small(dptr(x_nhwc), N, HW, Cc, dptr(gamma), dptr(beta), eps, dptr(film), int(film_stride), int(silu),
                                dptr(y), stream_ptr()))
    return y


def conv_mfma16(on=None):
    """MFMA shape of the tap-reuse convolution kernel (dsd_set_conv_mfma16: 0 = 32x32x16, 1 = 16x16x32), process-wide.  Sets it
    and returns the previous setting; on=None only reads it."""
    L = lib()
    prev = L.dsd_set_conv_mfma16(int(bool(on)))
    if on is None:
        L.dsd_set_conv_mfma16(prev)
    return prev


def group_norm(x_nhwc, gamma, beta, eps=1e-5, silu=False):
    N, H, W, Cc = x_nhwc.shape
    y = torch.empty_like(x_nhwc)
    check(lib().dsd_op_group_norm(dptr(x_nhwc), N, H * W, Cc, dptr(gamma), dptr(beta), eps, int(silu), dptr(y),
                                  stream_ptr()))
    return y


def gn_silu_conv_out1(x_nhwc, gamma, beta, w_oihw, bias, eps=1e-5):
    """The U-Net's `out` layer in one pass: Conv3x3(SiLU(GroupNorm32(x))) -> [N, H, W] (one output channel)."""
    N, H, W, Cc = x_nhwc.shape
    y = torch.empty((N, H, W), device=x_nhwc.device, dtype=torch.float32)
    check(lib().dsd_op_gn_silu_conv_out1(dptr(x_nhwc), N, H, W, Cc, dptr(gamma), dptr(beta), eps, dptr(w_oihw.contiguous()),
                                         dptr(bias), dptr(y), stream_ptr()))
    return y


def qkv_attention(qkv_ntc, heads, new_order=True, split=False):
    """split: bf16x6 arithmetic (operands as 3 bf16 pieces, 6 products) instead of the fp32 matrix cores."""
    N, T, C3 = qkv_ntc.shape
    a = torch.empty((N, T, C3 // 3), device=qkv_ntc.device, dtype=torch.float32)
    check(lib().dsd_op_qkv_attention(dptr(qkv_ntc), N, T, C3 // 3, heads, int(new_order), int(split), dptr(a), stream_ptr()))
    return a


def attention(q, k, v, out, N, Tq, Tk, heads, d, ldq, ldk, ldv, ldo, q_hs, k_hs, v_hs, scale_q=1.0, scale_k=1.0, scale_s=1.0,
              split=False):
    """softmax((q scale_q)(k scale_k)^T scale_s) v per head with every launch argument of the kernel (dsd_op_attention).
    q / k / v / out: fp32 CUDA tensors or views; only their first element's address and the strides given here are used."""
    check(lib().dsd_op_attention(C.c_void_p(q.data_ptr()), C.c_void_p(k.data_ptr()), C.c_void_p(v.data_ptr()), N, Tq, Tk, heads, d,
                                 ldq, ldk, ldv, ldo, q_hs, k_hs, v_hs, float(scale_q), float(scale_k), float(scale_s), int(split),
                                 C.c_void_p(out.data_ptr()), stream_ptr()))
    return out


def gemm_half(x, w, bias=None, dtype="f16", epi="store", gate=None, T=1, y=None):
    """nn.Linear on 16-bit operands (one MFMA per product, fp32 accumulation): y = x w^T + bias.  epi "store" | "gelu" |
    "gated" (y fp32 in/out: y += gate[m // T] * round16(x w^T + bias))."""
    M, K = x.shape
    N = w.shape[0]
    e = {"store": 0, "gelu": 1, "gated": 2}[epi]
    if e == 2:
        assert y is not None and gate is not None
    else:
        y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    check(lib().dsd_op_gemm_half(dptr(x), dptr(w.contiguous()), dptr(bias), M, N, K, int(dtype == "bf16"), e, dptr(gate), int(T),
                                 dptr(y), stream_ptr()))
    return y


def attention_half(qkv_ntc, heads, dtype="f16", thr=-1.0):
    """timm Attention core on qkv[N,T,3C] (q | k | v): softmax(q k^T d^-1/2) v with 16-bit operands, fp32 statistics."""
    N, T, C3 = qkv_ntc.shape
    a = torch.empty((N, T, C3 // 3), device=qkv_ntc.device, dtype=torch.float32)
    check(lib().dsd_op_attention_half(dptr(qkv_ntc), N, T, C3 // 3, heads, int(dtype == "bf16"), float(thr), dptr(a), stream_ptr()))
    return a


def timestep_embedding(t, dim, freqs=None):
    """freqs: optional [dim//2] fp32 CUDA tensor, the caller's own exp(-ln(1e4) k / half) table (the shim path)."""
    is_float = t.dtype.is_floating_point
    t = t.float().contiguous() if is_float else t.long().contiguous()
    y = torch.empty((t.shape[0], dim), device=t.device, dtype=torch.float32)
    check(lib().dsd_op_timestep_embedding(C.c_void_p(t.data_ptr()), int(is_float), t.shape[0], dim, dptr(freqs), dptr(y),
                                          stream_ptr()))
    return y


def linear(x, w, bias=None, act_in=0):
    N, K = x.shape
    y = torch.empty((N, w.shape[0]), device=x.device, dtype=torch.float32)
    check(lib().dsd_op_linear(dptr(x), N, K, dptr(w.contiguous()), dptr(bias), w.shape[0], act_in, dptr(y), stream_ptr()))
    return y


def tail(kind, ptrs, ints, floats=()):
    """One of the small element-wise / layout / LayerNorm kernels alone (dsd_op_tail; argument order per kind in
    include/dsdiff.h).  kind: a name of _lib.TAIL_KINDS; ptrs: CUDA tensors or views (only the first element's address is
    used) or None; ints / floats: the launcher's scalars."""
    from ._lib import TAIL_KINDS
    p = (C.c_void_p * max(len(ptrs), 1))(*[None if t is None else t.data_ptr() for t in ptrs])
    i = (C.c_int64 * max(len(ints), 1))(*[int(v) for v in ints])
    f = (C.c_float * max(len(floats), 1))(*[float(v) for v in floats])
    check(lib().dsd_op_tail(TAIL_KINDS.index(kind), p, i, f, stream_ptr()))


def philox_normal(n, seed, step, device="cuda"):
    y = torch.empty((n,), device=device, dtype=torch.float32)
    check(lib().dsd_op_philox_normal(dptr(y), n, seed, step, stream_ptr()))
    return y
