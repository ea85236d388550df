"""GPU tests of the int8-activation GEMM (op GemmA8W8, context phase): quantiser, GEMM, epilogues, layout, operator.

Yardstick: tests/a8w8_ref.py, the numpy restatement of the reference's arithmetic (no pinned oracle exists: see its docstring).
Quantiser and GEMM are compared for EQUALITY: every step is an exact integer operation or a single IEEE f32 operation in a fixed
order, so a difference means an operation out of order or fused.  Only results that pass through libm (SiLU, GELU) use the
project's one-ulp criterion (tests/test_gpu_gemm.py::assert_close)."""
import numpy as np
import pytest
import torch

from oracle import quant
from oracle.numerics import bf16_round, f16_round
from tests import a8w8_ref
from tests.test_gpu_gemm import FT, SMALL, assert_close, make_case, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(pkg):
    from dash_infer_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def rnd(ft):
    return bf16_round if ft == "bf16" else f16_round


def host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def same_values(got, ref, what):
    """Equality by value: +0 and -0 alike, every element finite."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, what
    bad = ~(got == ref)
    assert not bad.any(), (f"{what}: {bad.sum()} / {bad.size} elements differ; first at {tuple(np.argwhere(bad)[0])}: "
                           f"got {got[bad][0]!r}, expected {ref[bad][0]!r}; max |diff| {np.nanmax(np.abs(got - ref)):.3e}")


def quant_inputs(rng, M, K, ft):
    x = rng.normal(0, 1, (M, K)).astype(np.float32)
    if M >= 3:
        x[1] = 0                                             # an all-zero row
        x[2, K // 3] = 6.0e4 if ft == "f16" else 3.0e38      # a row holding a single huge value
    return rnd(ft)(x)


def check_quantized(qa, x, K, what):
    q, a_scale, rsum = a8w8_ref.quantize_rows(x)
    torch.cuda.synchronize()
    got_q = qa.q.cpu().numpy()
    Kp = (K + 63) // 64 * 64
    assert got_q.shape == (x.shape[0], Kp)
    np.testing.assert_array_equal(got_q[:, :K], q, err_msg=what + ": q")
    assert not got_q[:, K:].any(), what + ": the padding of the k-tile must be zero"
    np.testing.assert_array_equal(qa.a_scale.cpu().numpy().view(np.uint32), a_scale.view(np.uint32), err_msg=what + ": a_scale bits")
    np.testing.assert_array_equal(qa.rsum.cpu().numpy(), rsum, err_msg=what + ": rsum")


# ------------------------------------------------------------------ 2. quantiser, exact -------
@pytest.mark.parametrize("ft", ["bf16", "f16"])
@pytest.mark.parametrize("K", [96, 519, 3584, 18944])
@pytest.mark.parametrize("M", [1, 5, 130])
def test_quantizer_exact(ops, M, K, ft):
    rng = np.random.default_rng(M * 100003 + K)
    x = quant_inputs(rng, M, K, ft)
    check_quantized(ops.act_quant_i8(to_dev(x, ft)), x, K, f"M={M} K={K} {ft}")


def test_quantizer_wide_and_strided_rows(ops):
    rng = np.random.default_rng(5)
    K = 131072 - 64                                           # beyond the register-resident widths: the row is read twice
    x = quant_inputs(rng, 3, K, "bf16")
    check_quantized(ops.act_quant_i8(to_dev(x, "bf16")), x, K, "wide")
    big = quant_inputs(rng, 7, 1000, "bf16")                  # rows of a wider matrix: ldx 1000, K 520, from column 8
    check_quantized(ops.act_quant_i8(to_dev(big, "bf16")[:, 8:528]), big[:, 8:528], 520, "strided")


@pytest.mark.parametrize("ft", ["bf16", "f16"])
@pytest.mark.parametrize("K", [96, 520, 3584, 8192, 9000])    # one-launch widths (<= 4096, <= 8192) and the two-launch form
@pytest.mark.parametrize("M", [1, 5, 130])
def test_norm_quantizer_exact(ops, M, K, ft):
    """Only the quantiser is under test: the FT-rounded norm is the product's own dihip_rmsnorm_rows output."""
    rng = np.random.default_rng(M * 7919 + K)
    h = rng.normal(0, 2, (M, K)).astype(np.float32)
    if M >= 3:
        h[1] = 0
        h[2, K // 3] = 1.0e6
    gamma = rnd(ft)(rng.uniform(0.5, 1.5, K).astype(np.float32))
    hd, gd = to_dev(h), to_dev(gamma, ft)
    xn = host(ops.rmsnorm_rows(hd, gd, 1e-6))
    check_quantized(ops.norm_act_quant_i8(hd, gd, 1e-6), xn, K, f"norm M={M} K={K} {ft}")


# ------------------------------------------------------------------ 3. GEMM, exact ------------
def a8_case(rng, M, N, K, ft, style):
    x, q, s, z = make_case(rng, M, N, K, -1, 8, ft, style=style)
    x = rnd(ft)(rng.normal(0, 1, (M, K)).astype(np.float32))
    if M >= 3:
        x[1] = 0
    bias = rnd(ft)(rng.normal(0, 0.2, N).astype(np.float32))
    return x, q, s, z, bias


SHAPES = sorted({(M, N, K) for M, N, K, _ in SMALL}) + [(2048, 4608, 3584), (300, 3584, 18944), (64, 512, 131072 - 64)]


@pytest.mark.parametrize("ft", ["bf16", "f16"])
@pytest.mark.parametrize("style", ["iq", "synthetic"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_exact(ops, M, N, K, style, ft):
    rng = np.random.default_rng(M + 31 * N + 977 * K)
    x, q, s, z, bias = a8_case(rng, M, N, K, ft, style)
    pw = ops.pack_lowp(to_dev(q), to_dev(s, ft), to_dev(z, ft), -1, 8)
    xd, bd = to_dev(x, ft), to_dev(bias, ft)
    for b, bdev in ((None, None), (bias, bd)):
        ref = a8w8_ref.gemm_a8w8(x, q, s, z, ft, bias=b)
        assert np.isfinite(ref).all()
        same_values(host(ops.gemm_a8w8(xd, pw, bias=bdev)), ref, f"M={M} N={N} K={K} {style} {ft} bias={b is not None}")


def test_k_beyond_the_accumulator_range_is_a_parameter_error(ops, pkg):
    from dash_infer_amd import capi
    K = 131072 + 64
    x = torch.zeros(1, K, dtype=torch.bfloat16, device="cuda")
    pw = ops.PackedWeight(8, 16, K, -1, torch.bfloat16, torch.zeros(16, dtype=torch.uint8, device="cuda"),
                          torch.zeros(16, dtype=torch.int32, device="cuda"))
    with pytest.raises(capi.DihipError) as e:
        ops.gemm_a8w8(x, pw, ws=torch.empty(1 << 20, dtype=torch.uint8, device="cuda"))
    assert e.value.code == capi.PARAM_ERROR


# ------------------------------------------------------------------ 4. epilogues --------------
@pytest.mark.parametrize("ft", ["bf16", "f16"])
@pytest.mark.parametrize("act", ["silu", "gelu_erf", "gelu_tanh"])
@pytest.mark.parametrize("M,N,K", [(17, 261, 519), (130, 512, 1024)])
def test_activation_epilogue(ops, M, N, K, act, ft):
    rng = np.random.default_rng(M + N + K)
    x, q, s, z, bias = a8_case(rng, M, N, K, ft, "iq")
    pw = ops.pack_lowp(to_dev(q), to_dev(s, ft), to_dev(z, ft), -1, 8)
    ref, _, pre = a8w8_ref.gemm_a8w8(x, q, s, z, ft, bias=bias, act=act, parts=True)
    got = host(ops.gemm_a8w8(to_dev(x, ft), pw, bias=to_dev(bias, ft), act=act))
    assert_close(got, ref, ft, what=f"{act} {ft}", pre=None)
    # without libm the activation epilogue is exact as well
    same_values(host(ops.gemm_a8w8(to_dev(x, ft), pw, bias=to_dev(bias, ft), act="relu")),
                a8w8_ref.gemm_a8w8(x, q, s, z, ft, bias=bias, act="relu"), f"relu {ft}")


@pytest.mark.parametrize("ft", ["bf16", "f16"])
def test_residual_epilogue_exact(ops, ft):
    rng = np.random.default_rng(77)
    M, N, K = 33, 80, 256
    x, q, s, z, bias = a8_case(rng, M, N, K, ft, "iq")
    res = rnd(ft)(rng.normal(0, 1, (M, N)).astype(np.float32))
    pw = ops.pack_lowp(to_dev(q), to_dev(s, ft), to_dev(z, ft), -1, 8)
    got = host(ops.gemm_a8w8(to_dev(x, ft), pw, bias=to_dev(bias, ft), residual=to_dev(res, ft)))
    same_values(got, a8w8_ref.gemm_a8w8(x, q, s, z, ft, bias=bias, residual=res), f"residual {ft}")


@pytest.mark.parametrize("ft", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", [(17, 261, 519), (300, 1000, 1536)])
def test_swiglu_epilogue(ops, M, N, K, ft):
    rng = np.random.default_rng(M * N)
    x, gq, gs, gz, _ = a8_case(rng, M, N, K, ft, "iq")
    _, uq, us, uz = make_case(rng, 1, N, K, -1, 8, ft, style="iq")
    pg = ops.pack_lowp(to_dev(gq), to_dev(gs, ft), to_dev(gz, ft), -1, 8)
    pu = ops.pack_lowp(to_dev(uq), to_dev(us, ft), to_dev(uz, ft), -1, 8)
    ref, sg, u = a8w8_ref.swiglu_a8w8(x, gq, gs, gz, uq, us, uz, ft, parts=True)
    qa = ops.act_quant_i8(to_dev(x, ft))
    got = host(ops.gemm_a8w8_swiglu_q(qa, pg, pu))
    # FT(SiLU(.)) may flip by one ulp (libm's last bit): its effect on the product is one ulp of sg times |u|
    assert_close(got, ref, ft, what=f"swiglu {ft}", pre=np.abs(sg) * np.abs(u))
    # the norm form: quantised FT(RMSNorm(h) * gamma), same pair
    h = rng.normal(0, 2, (M, K)).astype(np.float32)
    gamma = rnd(ft)(rng.uniform(0.5, 1.5, K).astype(np.float32))
    hd, gd = to_dev(h), to_dev(gamma, ft)
    if K % 4 == 0:
        xn = host(ops.rmsnorm_rows(hd, gd, 1e-6))
        ref2, sg2, u2 = a8w8_ref.swiglu_a8w8(xn, gq, gs, gz, uq, us, uz, ft, parts=True)
        assert_close(host(ops.a8w8_norm_swiglu(hd, gd, 1e-6, pg, pu)), ref2, ft, what=f"norm swiglu {ft}", pre=np.abs(sg2) * np.abs(u2))


@pytest.mark.parametrize("ft", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", [(17, 261, 519), (300, 512, 1536)])
def test_addto_epilogue_exact(ops, M, N, K, ft):
    rng = np.random.default_rng(M + N)
    x, q, s, z, _ = a8_case(rng, M, N, K, ft, "synthetic")
    h_res = rng.normal(0, 1, (M, N)).astype(np.float32)
    pw = ops.pack_lowp(to_dev(q), to_dev(s, ft), to_dev(z, ft), -1, 8)
    _, f, _ = a8w8_ref.gemm_a8w8(x, q, s, z, ft, parts=True)
    ref = (h_res + f).astype(np.float32)                      # one IEEE add on the unrounded f
    same_values(host(ops.a8w8_gemm_addto(to_dev(x, ft), pw, to_dev(h_res))), ref, f"addto {ft}")
    same_values(host(ops.a8w8_gemm_addto(to_dev(x, ft), pw, None)), f, f"addto without residual {ft}")
    # the norm form of the STD epilogue, exact: the quantiser's input is the product's own norm
    if K % 4 == 0:
        hh = rng.normal(0, 2, (M, K)).astype(np.float32)
        gamma = rnd(ft)(rng.uniform(0.5, 1.5, K).astype(np.float32))
        hd, gd = to_dev(hh), to_dev(gamma, ft)
        xn = host(ops.rmsnorm_rows(hd, gd, 1e-6))
        same_values(host(ops.a8w8_norm_gemm(hd, gd, 1e-6, pw)), a8w8_ref.gemm_a8w8(xn, q, s, z, ft), f"norm gemm {ft}")


# ------------------------------------------------------------------ 5. layout map -------------
@pytest.mark.parametrize("ft", ["bf16", "f16"])
def test_layout_map_identity_a_asymmetric_b(ops, ft):
    """A = identity rows (hand-made xq, a_scale 1, zero points 0, scales 1): y == xq . Wq exactly -- row m of the result is row
    k = m of an ASYMMETRIC B, so any k the A fragment pairs with the wrong byte of the B chunk shows up as a wrong row."""
    K, N = 192, 80
    M = K
    rng = np.random.default_rng(3)
    wq = (np.arange(K)[:, None] * 7 + np.arange(N)[None, :] * 3) % 200 - 100        # every (k, n) distinct along both axes, |.| <= 100
    wq = wq.astype(np.int8)
    pw = ops.pack_lowp(to_dev(wq), to_dev(np.ones((1, N), np.float32), ft), to_dev(np.zeros((1, N), np.float32), ft), -1, 8)
    xq = np.eye(M, K, dtype=np.int8)
    qa = ops.QuantizedAct(to_dev(xq), to_dev(np.ones(M, np.float32)), to_dev(xq.sum(axis=1).astype(np.int32)), K)
    same_values(host(ops.gemm_a8w8_q(qa, pw)), wq.astype(np.float32), f"identity {ft}")
    # small random integers on both sides, sums exactly representable in FT (|sum| <= 256 for bf16)
    xq = np.zeros((40, K), np.int8)
    for m in range(40):
        xq[m, rng.choice(K, 2, replace=False)] = rng.choice([-1, 1], 2)
    ref = xq.astype(np.int64) @ wq.astype(np.int64)
    assert np.abs(ref).max() <= 256
    qa = ops.QuantizedAct(to_dev(xq), to_dev(np.ones(40, np.float32)), to_dev(xq.sum(axis=1).astype(np.int32)), K)
    same_values(host(ops.gemm_a8w8_q(qa, pw)), ref.astype(np.float32), f"two-hot {ft}")


# ------------------------------------------------------------------ 6. determinism / invariance
def test_deterministic_and_batch_invariant(ops):
    rng = np.random.default_rng(11)
    M, N, K = 2048, 1000, 1536
    x, q, s, z, bias = a8_case(rng, M, N, K, "bf16", "iq")
    pw = ops.pack_lowp(to_dev(q), to_dev(s, "bf16"), to_dev(z, "bf16"), -1, 8)
    xd, bd = to_dev(x, "bf16"), to_dev(bias, "bf16")
    y1 = ops.gemm_a8w8(xd, pw, bias=bd, act="silu")
    y2 = ops.gemm_a8w8(xd, pw, bias=bd, act="silu")
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
    for r0 in (0, 640, 1920):                                 # per-row quantisation: a row does not depend on its batch
        part = ops.gemm_a8w8(xd[r0:r0 + 128].contiguous(), pw, bias=bd, act="silu")
        torch.cuda.synchronize()
        assert torch.equal(part.view(torch.int16), y1[r0:r0 + 128].view(torch.int16))
    one = ops.gemm_a8w8(xd[77:78].contiguous(), pw, bias=bd, act="silu")
    torch.cuda.synchronize()
    assert torch.equal(one.view(torch.int16), y1[77:78].view(torch.int16))


# ------------------------------------------------------------------ 7. operator ---------------
def view_of(ptr, shape, dtype):
    import ctypes as C
    n = int(np.prod(shape))
    t = torch.empty(n, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), n * t.element_size(), 3) == 0
    return t.view(*shape)


@pytest.mark.parametrize("ft,act", [("bf16", None), ("f16", None), ("bf16", "relu")])
def test_gemm_a8w8_operator_both_phases(ops, pkg, ft, act):
    from dash_infer_amd import hostapi
    rng = np.random.default_rng(21)
    K, N = 512, 384
    W = rnd(ft)(rng.normal(0, 0.05, (K, N)).astype(np.float32))
    q, s, z = quant.iq_quantize_a16w8(W, -1, ft)
    bias = rnd(ft)(rng.normal(0, 0.2, N).astype(np.float32))
    m = hostapi.Model(ops.cur_stream(), 4, 2, 128, 16)
    for name in ("a8", "a16"):      # each operator packs (and may release) its own copy
        m.set_weight(name + ".w", to_dev(q), "i8")
        m.set_weight(name + ".s", to_dev(s, ft), ft)
        m.set_weight(name + ".z", to_dev(z, ft), ft)
        m.set_weight(name + ".b", to_dev(bias, ft), ft)
    attrs = "alpha=f:1.0" + (f";activation=i:{ {'relu': 4}[act] }" if act else "")
    op8 = op16 = None
    for M in (1, 5, 40):            # batch changes -> Reshape again, same op instances
        x = rnd(ft)(rng.normal(0, 1, (M, 1, K)).astype(np.float32))
        x_dev = to_dev(x, ft)
        m.set_tensor("x", x_dev, ft)
        if op8 is None:
            op8 = m.create_op("GemmA8W8", "a8", ["x"], ["y8"], ["a8.w", "a8.s", "a8.z", "a8.b"], attrs)
            op16 = m.create_op("GemmA16W8", "a16", ["x"], ["y16"], ["a16.w", "a16.s", "a16.z", "a16.b"], attrs)
        m.set_phase(1)
        m.reshape(op8)
        m.alloc(op8)
        m.forward(op8)
        dt, shape, ptr = m.get_tensor("y8")
        assert dt == hostapi.DT[ft] and shape == [M, 1, N]
        y = view_of(ptr, shape, FT[ft]).float().cpu().numpy().reshape(M, N)
        same_values(y, a8w8_ref.gemm_a8w8(x.reshape(M, K), q, s, z, ft, bias=bias, act=act), f"context phase M={M} {ft}")
        m.set_phase(0)
        for op in (op8, op16):
            m.reshape(op)
            m.alloc(op)
            m.forward(op)
        y8 = view_of(m.get_tensor("y8")[2], [M, N], FT[ft])
        y16 = view_of(m.get_tensor("y16")[2], [M, N], FT[ft])
        assert torch.equal(y8.view(torch.int16), y16.view(torch.int16)), f"decoder phase M={M}: not the GemmA16W8 result"
    m.close()


def test_gemm_a8w8_operator_rejects_bad_attributes(ops, pkg):
    from dash_infer_amd import hostapi
    m = hostapi.Model(ops.cur_stream(), 4, 2, 128, 16)
    m.set_weight("w", torch.zeros(64, 32, dtype=torch.int8, device="cuda"), "i8")
    m.set_weight("s", torch.zeros(1, 32, dtype=torch.bfloat16, device="cuda"), "bf16")
    m.set_weight("z", torch.zeros(1, 32, dtype=torch.bfloat16, device="cuda"), "bf16")
    m.set_tensor("x", torch.zeros(1, 1, 64, dtype=torch.bfloat16, device="cuda"), "bf16")
    m.set_tensor("r", torch.zeros(1, 1, 32, dtype=torch.bfloat16, device="cuda"), "bf16")
    for bad in ("GroupSize=i:128", "GroupSize=i:64", "transB=b:1", "is_pooler=b:1"):
        with pytest.raises(hostapi.HostError) as e:
            m.create_op("GemmA8W8", "g", ["x"], ["y"], ["w", "s", "z"], bad)
        assert e.value.code == 2
    with pytest.raises(hostapi.HostError) as e:               # exactly one input: no fused residual
        m.create_op("GemmA8W8", "g", ["x", "r"], ["y"], ["w", "s", "z"], "")
    assert e.value.code == 2
    m.create_op("GemmA8W8", "g", ["x"], ["y"], ["w", "s", "z"], "GroupSize=i:-1")
    m.close()
