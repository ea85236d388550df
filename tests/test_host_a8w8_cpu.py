"""GemmA8W8 (QuantMode.A8W8: int8 per-channel weights, activations quantised per row in the context phase) without a GPU:
registration of the operator, the fusion pass on a GemmA8W8 graph, workspace sizing, and a self-check of the numpy restatement the
GPU tests compare against (tests/a8w8_ref.py)."""
import numpy as np
import pytest

from oracle.numerics import bf16_round
from tests import a8w8_ref, ref_graph


@pytest.fixture()
def hostapi(pkg):
    from dash_infer_amd import hostapi as h
    return h


def test_gemm_a8w8_is_registered_and_the_probe_list_is_unchanged(hostapi):
    lib = hostapi.lib()
    assert lib.dihost_op_registered(b"GemmA8W8") == 1
    assert lib.dihost_op_registered(b"GemmA16W8") == 1
    assert lib.dihost_op_registered(b"GemmA8W8Sparse.made.up") == 0
    assert lib.dihost_op_registered(b"") == 0
    assert lib.dihost_op_registered(None) == 0
    assert "GemmA8W8" not in lib.dihost_registered_ops().decode().split(",")   # (tests/test_host_ops_cpu.py pins that list)


def fuse(hostapi, graph):
    m = hostapi.Model(None, 4, 2, 128, 16)
    try:
        ref_graph.add_graph(m, graph)
        return m.graph_fuse_dry()
    finally:
        m.close()


def test_a8w8_graph_fuses_to_the_same_operator_types(hostapi):
    from dash_infer_amd import ref_graph as product_graph
    g16 = product_graph.qwen2_graph(2, 8, -1, 1e-6, 4, 2, 1e6)
    g8 = product_graph.qwen2_graph(2, 8, -1, 1e-6, 4, 2, 1e6, act_quant=True)
    assert g16 == ref_graph.qwen2_graph(2, 8, -1, 1e-6, 4, 2, 1e6)             # the default output is unchanged
    assert [o[0] for o in g8].count("GemmA8W8") == 10 and not any(o[0] == "GemmA16W8" for o in g8)
    assert all("GroupSize" not in o[5] for o in g8)
    assert [(o[1:5]) for o in g8] == [(o[1:5]) for o in g16]                  # names, tensors and weights as in the A16W8 list
    r16, r8 = fuse(hostapi, g16), fuse(hostapi, g8)
    assert r8["fused"] and r8["device_resident"] and r8["layers"] == 2, r8["why"]
    assert r8["types"] == r16["types"]
    assert r8["wiring"] == r16["wiring"]
    with pytest.raises(ValueError):
        product_graph.qwen2_graph(1, 4, 128, 1e-6, 4, 2, 1e6, act_quant=True)
    with pytest.raises(ValueError):
        product_graph.qwen2_graph(1, 8, 128, 1e-6, 4, 2, 1e6, act_quant=True)


@pytest.mark.parametrize("which", [2, 5, 8, 9, 11])    # qkv, o, gate, up, down of layer 0
def test_a_graph_mixing_a8w8_and_a16w8_is_left_unfused(hostapi, which):
    from dash_infer_amd import ref_graph as product_graph
    g = product_graph.qwen2_graph(2, 8, -1, 1e-6, 4, 2, 1e6, act_quant=True)
    assert g[which][0] == "GemmA8W8"
    g[which] = ("GemmA16W8",) + g[which][1:]
    r = fuse(hostapi, g)
    assert not r["fused"]
    assert r["types"] == [o[0] for o in g]
    assert "GemmA8W8" in r["why"] and "mixed" in r["why"], r["why"]


def test_sub_channel_a8w8_is_left_unfused(hostapi):
    from dash_infer_amd import ref_graph as product_graph
    g = product_graph.qwen2_graph(1, 8, -1, 1e-6, 4, 2, 1e6, act_quant=True)
    g[2] = g[2][:5] + (g[2][5] + ";GroupSize=i:128",)
    r = fuse(hostapi, g)
    assert not r["fused"] and "per-channel" in r["why"], r["why"]


def test_workspace_bytes(pkg):
    from dash_infer_amd import capi
    l = capi.lib()
    for M, N, K in [(1, 48, 96), (5, 48, 96), (130, 261, 519), (2048, 4608, 3584), (300, 3584, 18944), (64, 512, 131072)]:
        assert l.dihip_gemm_a8w8_workspace_bytes(M, N, K) >= M * ((K + 63) // 64 * 64) + 8 * M
    for M, N, K in [(0, 48, 96), (4, 0, 96), (4, 48, 0), (-1, 48, 96), (4, 48, 131072 + 1)]:
        assert l.dihip_gemm_a8w8_workspace_bytes(M, N, K) == 0


@pytest.mark.parametrize("M,N,K", [(5, 48, 96), (130, 261, 519), (64, 512, 18944)])
def test_the_restatement_against_the_dequantised_product(M, N, K):
    """Self-check of tests/a8w8_ref.py (not of the product): per row the only approximation is the activation rounding,
    |x - a_scale q| <= a_scale / 2, so |y - x.W| <= a_scale / 2 * sum_k |W[k, n]| + the f32 / FT roundings."""
    rng = np.random.default_rng(M + N + K)
    x = bf16_round(rng.normal(0, 1, (M, K)).astype(np.float32))
    x[M // 2] = 0
    wq = rng.integers(-128, 128, (K, N)).astype(np.int8)
    s = bf16_round(rng.uniform(0.9 * 2 / 256, 1.1 * 2 / 256, (1, N)).astype(np.float32))
    z = bf16_round(rng.uniform(-10, 10, (1, N)).astype(np.float32))
    q, a_scale, rsum = a8w8_ref.quantize_rows(x)
    assert q.dtype == np.int8 and q.min() >= -127 and q.max() <= 127
    assert (np.abs(q).max(axis=1)[a_scale > 0] == 127).all() and (q[M // 2] == 0).all() and a_scale[M // 2] == 0
    np.testing.assert_array_equal(rsum, q.astype(np.int64).sum(axis=1))
    assert np.abs(x - a_scale[:, None].astype(np.float64) * q).max() <= 0.5 * a_scale.max() * (1 + 1e-6)
    acc = a8w8_ref.int_product(q, wq)
    np.testing.assert_array_equal(acc[:3], q[:3].astype(np.int64) @ wq.astype(np.int64))
    assert np.abs(acc).max() < 2 ** 31
    y, f, _ = a8w8_ref.gemm_a8w8(x, wq, s, z, "bf16", parts=True)
    assert np.isfinite(y).all() and (y[M // 2] == 0).all()
    ref = a8w8_ref.dequantized_product(x, wq, s, z)
    w_abs = np.abs((wq.astype(np.float64) - z.astype(np.float64)) * s.astype(np.float64)).sum(axis=0)
    bound = 0.5 * a_scale.astype(np.float64)[:, None] * w_abs[None, :]
    f32_terms = 2.0 ** -21 * (np.abs(acc) + np.abs(z.astype(np.float64) * rsum[:, None])) * (a_scale[:, None].astype(np.float64) * s)
    assert (np.abs(f - ref) <= bound + f32_terms + 1e-6).all()
    assert (np.abs(y - f) <= 2.0 ** -8 * np.abs(f) + 1e-30).all()
