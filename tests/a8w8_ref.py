"""numpy restatement of the reference's GemmA8W8 context-phase arithmetic -- the yardstick of tests/test_gpu_a8w8*.py.

NOT a pinned oracle: the reference's CUDA kernels cannot be built for this backend, so this file restates them, one numpy
float32 operation per line where the reference has one f32 operation (its library is built with -ffp-contract=off and IEEE
division), from
  * GemmA8W8GPU::DispatchKernel            csrc/core/operator/general/gemm_lowp/gemm_a8w8_gpu.cpp:119-210
  * per_channel_symm_dynamic_quantization   csrc/core/kernel/cuda/gemm_lowp/gemm_a8w8_perc_kernel.cu:28-133
  * A_perc_symm_B_perc_asymm_dequantization csrc/core/kernel/cuda/gemm_lowp/gemm_a8w8_perc_kernel.cu:400-469
  * the export side                         python/pyhie/allspark/model/quantization_utils.py:65-66 (op type GemmA8W8)
Weights [Wq int8 [K, N], scales FT [1, N], zeros FT [1, N], (bias FT [N])], per-channel only; x FT [M, K].
A row of zeros is DEFINED as q = 0, a_scale = 0 (the reference's q for such a row is an artefact of fminf on a NaN and is
multiplied by a zero scale: the same output).  alpha is not applied (the reference's A8W8 path ignores it).  NaN / Inf inputs
are unspecified.  The integer product is taken in float64 (exact below 2^53, and BLAS-fast)."""
import numpy as np

from oracle.numerics import bf16_round, f16_round

MAX_K = 131072   # 127 * 128 * K < 2^31


def ft_round(a, ft):
    return (bf16_round if ft == "bf16" else f16_round)(np.asarray(a, np.float32))


def quantize_rows(x):
    """x: float32 [M, K] holding FT values -> (q int8 [M, K], a_scale f32 [M], rsum i32 [M])."""
    x = np.asarray(x, np.float32)
    amax = np.abs(x).max(axis=1).astype(np.float32)                       # exact
    a_scale = (amax / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore"):
        rec = (np.float32(127) / amax).astype(np.float32)
    rec = np.where(amax > 0, rec, np.float32(0)).astype(np.float32)       # the all-zero row: q = 0
    p = (x * rec[:, None]).astype(np.float32)
    q = np.rint(np.minimum(np.float32(127), np.maximum(np.float32(-128), p))).astype(np.int8)   # round half to even
    rsum = q.astype(np.int32).sum(axis=1, dtype=np.int32)
    return q, a_scale, rsum


def int_product(q, wq):
    """sum_k q[m, k] * wq[k, n], exact, as int64."""
    assert q.shape[1] <= MAX_K
    return np.rint(q.astype(np.float64) @ wq.astype(np.float64)).astype(np.int64)


def dequant(acc, a_scale, rsum, scales, zeros, bias=None):
    """The unrounded f32 result f[m, n]; scales / zeros / bias: float32 arrays holding FT values ([1, N] or [N])."""
    s = np.asarray(scales, np.float32).reshape(1, -1)
    z = np.asarray(zeros, np.float32).reshape(1, -1)
    zr = (z * rsum.astype(np.float32)[:, None]).astype(np.float32)
    f = (acc.astype(np.float32) - zr).astype(np.float32)
    sc = (np.asarray(a_scale, np.float32)[:, None] * s).astype(np.float32)
    f = (f * sc).astype(np.float32)
    if bias is not None:
        f = (f + np.asarray(bias, np.float32).reshape(1, -1)).astype(np.float32)
    return f


def unary(v, act):
    v = np.asarray(v, np.float64)
    if act in (None, "none"):
        return v
    if act == "silu":
        return v / (1.0 + np.exp(-v))
    if act == "gelu_erf":
        from math import erf
        return 0.5 * v * (1.0 + np.vectorize(erf)(v * 0.70710678))
    if act == "gelu_tanh":
        return 0.5 * v * (1.0 + np.tanh(0.7978845608 * (v + 0.044715 * v ** 3)))
    if act == "relu":
        return np.maximum(v, 0.0)
    raise ValueError(act)


def gemm_a8w8(x, wq, scales, zeros, ft, bias=None, act=None, residual=None, parts=False):
    """y FT (as float32) [M, N].  parts=True: also the unrounded f and the FT value the activation was applied to."""
    q, a_scale, rsum = quantize_rows(x)
    f = dequant(int_product(q, wq), a_scale, rsum, scales, zeros, bias)
    y = ft_round(f, ft)
    pre = y
    if act not in (None, "none"):
        y = ft_round(unary(y, act).astype(np.float32), ft)
    if residual is not None:
        y = ft_round((y + np.asarray(residual, np.float32)).astype(np.float32), ft)
    return (y, f, pre) if parts else y


def swiglu_a8w8(x, gq, gs, gz, uq, us, uz, ft, parts=False):
    """FT(FT(SiLU(FT(gate))) * FT(up)): GemmA8W8(SILU), GemmA8W8, Binary MUL on one quantised A."""
    q, a_scale, rsum = quantize_rows(x)
    g = ft_round(dequant(int_product(q, gq), a_scale, rsum, gs, gz), ft)
    u = ft_round(dequant(int_product(q, uq), a_scale, rsum, us, uz), ft)
    sg = ft_round(unary(g, "silu").astype(np.float32), ft)
    y = ft_round((sg * u).astype(np.float32), ft)
    return (y, sg, u) if parts else y


def dequantized_product(x, wq, scales, zeros):
    """float64 x . ((Wq - zero) * scale): what the operator approximates (no activation quantisation)."""
    w = (wq.astype(np.float64) - np.asarray(zeros, np.float64).reshape(1, -1)) * np.asarray(scales, np.float64).reshape(1, -1)
    return np.asarray(x, np.float64) @ w
