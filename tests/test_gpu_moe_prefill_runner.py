"""The mixture-of-experts CONTEXT phase through the operator layer and the two runners: above 2 048 (token, expert) slots the
MOEA16W8 operator, DihipMoeBlock and decoder.DecodeSession all take the grouped expert GEMM (dihip_moe_experts_gemm), at or
below they keep the decode path.  Model: the small synthetic MoE model of tests/test_gpu_host_runner.py."""
import numpy as np
import pytest
import torch

from oracle import quant
from oracle.numerics import bf16_round
from tests.test_gpu_host_ops import dev, view_of
from tests.test_gpu_host_runner import MOE_SMALL, Host

pytestmark = pytest.mark.gpu


def test_moe_operator_takes_the_grouped_gemm_above_2048_slots(pkg):
    """MOEA16W8 over 300 rows at top-8 (2 400 slots) is dihip_moe_experts_gemm on the same tensors, bit for bit; over 256 rows
    (2 048 slots) it is still dihip_moe_experts."""
    from dash_infer_amd import hostapi, ops
    rng = np.random.default_rng(18)
    E, k, hidden, proj, G = 16, 8, 256, 384, -1

    def experts(K, N):
        qs, ss, zs = [], [], []
        for _ in range(E):
            q, s, z = quant.iq_quantize_a16w8(bf16_round(rng.normal(0, 0.05, (K, N)).astype(np.float32)), G, "bf16")
            qs.append(q); ss.append(s); zs.append(z)
        return np.stack(qs), np.stack(ss), np.stack(zs)

    gq, gs, gz = experts(hidden, proj)
    uq, us, uz = experts(hidden, proj)
    dq, ds, dz = experts(proj, hidden)
    packed = [ops.pack_experts([torch.from_numpy(q).cuda() for q in qs], [dev(s) for s in ss], [dev(z) for z in zs], G, 8)
              for qs, ss, zs in ((gq, gs, gz), (uq, us, uz), (dq, ds, dz))]
    m = hostapi.Model(ops.cur_stream(), 4, 2, 128, 16)
    m.set_weight("gu", torch.from_numpy(np.concatenate([gq, uq], axis=2)).cuda(), "i8")       # [E, hidden, 2*proj]
    m.set_weight("gu.scales", dev(np.concatenate([gs, us], axis=2)), "bf16")
    m.set_weight("gu.zeros", dev(np.concatenate([gz, uz], axis=2)), "bf16")
    m.set_weight("dn", torch.from_numpy(dq).cuda(), "i8")
    m.set_weight("dn.scales", dev(ds), "bf16")
    m.set_weight("dn.zeros", dev(dz), "bf16")
    op = None
    for T, want in ((300, ops.moe_experts_gemm), (256, ops.moe_experts), (300, ops.moe_experts_gemm)):
        xd = dev(rng.normal(0, 1, (T, 1, hidden)).astype(np.float32))
        ld = dev(rng.normal(0, 1.5, (T, 1, E)).astype(np.float32))
        m.set_tensor("x", xd, "bf16")
        m.set_tensor("router", ld, "bf16")
        if op is None:
            op = m.create_op("MOEA16W8", "decoder.layer.0.mlp.moe", ["x", "router"], ["y"],
                             ["gu", "gu.scales", "gu.zeros", "dn", "dn.scales", "dn.zeros"], f"num_experts=i:{E};num_experts_per_tok=i:{k}")
        m.reshape(op)
        m.alloc(op)
        m.forward(op)
        _, shape, ptr = m.get_tensor("y")
        y = view_of(ptr, shape, torch.bfloat16).reshape(T, hidden)
        scores, idx = ops.moe_route(ld.reshape(T, E), k)
        ref = want(xd.reshape(T, hidden), idx, scores, *packed)
        torch.cuda.synchronize()
        assert torch.equal(y, ref), f"T = {T}: the operator is not {want.__name__}: max diff {(y.float() - ref.float()).abs().max()}"
    m.close()


def test_long_moe_prompt_runner_is_bit_identical_to_decode_session(pkg):
    """A 264-token prompt at top-8 (2 112 slots): the C++ runner's context-phase logits equal DecodeSession's bit for bit, the first
    token is the oracle's, and five decode steps replayed as a hipGraph give what the eager steps give."""
    from dash_infer_amd import decoder
    from tests.test_gpu_decoder import oracle_of
    cfg = decoder.ModelConfig("moe-prefill-runner-test", **MOE_SMALL, moe=decoder.MoEConfig(16, 8, 256))
    model = decoder.build_random_model(cfg, decoder.QuantSpec(8, -1), seed=2468, keep_fp=True)
    span, max_len, steps, L = 16, 288, 5, 264
    prompt = [int(t) for t in np.random.default_rng(4).integers(0, cfg.vocab, L)]
    assert L * cfg.moe.top_k > 2048
    sess = decoder.DecodeSession(model, 1, max_len=max_len, span_len=span, kv_mode="none")
    lo0 = sess.prefill([prompt]).clone()
    first = sess.ids.cpu().tolist()[0]
    want = []
    for _ in range(steps):
        sess.step()
        torch.cuda.synchronize()
        want.append((sess.logits.clone(), sess.ids.cpu().tolist()))
    lo_ref = oracle_of(model, "none").prefill([prompt])
    tol = 1e-2 * max(1.0, float(np.abs(lo_ref).max()))
    err = float(np.abs(lo0[0].cpu().numpy() - lo_ref[0]).max())
    print(f"MoE prefill (grouped GEMM) vs oracle: max |diff| {err:.3e} (bound {tol:.3e})")
    assert err <= tol and first == int(np.argmax(lo_ref[0]))
    for graph in (True, False):
        h = Host(model, 1, max_len, span, "none")
        assert h.report["fused"] and h.report["types"].count("DihipMoeBlock") == len(model.layers), h.report["why"]
        k, v = h.spans()
        assert h.start(prompt, k, v) == first
        assert torch.equal(h.logits()[0], lo0[0]), "context-phase logits are not bit-identical to DecodeSession"
        for t in range(steps):
            ids = h.steps(1, graph=graph)          # graph: step 0 captures, the others replay
            assert ids == want[t][1], f"step {t} (graph={graph}): ids differ"
            assert torch.equal(h.logits(), want[t][0]), f"step {t} (graph={graph}): logits are not bit-identical to DecodeSession"
        h.close()
