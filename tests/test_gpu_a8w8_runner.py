"""A GemmA8W8 model (QuantMode.A8W8) through the C++ model runner: the fused list (context phase on the int8 x int8 GEMMs, decoder
phase on the A16W8 kernels) against the UNFUSED list of stand-alone GemmA8W8 operators, and the decode steps after an A8W8 prefill.

Measured figures (MI355X, printed by the test; not asserted where the issue says so) are recorded in DESIGN.md."""
import numpy as np
import pytest
import torch

from tests import ref_graph
from tests.test_gpu_host_runner import KV, SMALL, WIDE, Host

pytestmark = pytest.mark.gpu

PROMPT_LENGTHS = (3, 9, 17, 33, 47, 64, 70, 300)


class A8Host(Host):
    """tests/test_gpu_host_runner.py::Host with the projections of the list as GemmA8W8 (act_quant) or GemmA16W8."""

    def __init__(self, model, batch, max_len, span, kv_mode, fuse=True, act_quant=True):
        from dash_infer_amd import hostapi, ops
        cfg = model.cfg
        self.cfg, self.nl, self.spr = cfg, len(model.layers), (max_len + span - 1) // span
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        self.pool = ops.SpanPool(2 * batch * self.nl * self.spr + 4, cfg.n_kv, span, cfg.head_dim, kv_mode, torch.bfloat16)
        with torch.cuda.stream(self.stream):
            self.m = hostapi.Model(ops.cur_stream(), cfg.n_heads, cfg.n_kv, cfg.head_dim, span, KV[kv_mode], max_batch=batch, max_len=max_len)
            ref_graph.register_weights(self.m, model, "bf16")
            self.graph = ref_graph.qwen2_graph(self.nl, 8, -1, cfg.eps, cfg.n_heads, cfg.n_kv, cfg.rope_theta, act_quant=act_quant)
            ref_graph.add_graph(self.m, self.graph)
            self.report = self.m.graph_build(fuse=fuse)
        self.stream.synchronize()


def prefill_logits(model, prompts, max_len, span, fuse, act_quant):
    """Context-phase logits (f32 copy) and first id of every prompt, one request at a time."""
    out = []
    for pr in prompts:
        h = A8Host(model, 1, max_len, span, "none", fuse=fuse, act_quant=act_quant)
        assert h.report["fused"] == fuse, h.report["why"]
        k, v = h.spans()
        first = h.start(pr, k, v)
        out.append((h.logits().float().clone()[-1], first))
        h.close()
    return out


@pytest.mark.parametrize("shape,seed", [(SMALL, 41), (WIDE, 42)])
def test_a8w8_model_context_phase_fused_vs_unfused(pkg, shape, seed):
    from dash_infer_amd import decoder
    cfg = decoder.ModelConfig("a8w8-runner-test", **shape)
    model = decoder.build_random_model(cfg, decoder.QuantSpec(8, -1), seed=seed, keep_fp=True, decisive=1.5)
    rng = np.random.default_rng(seed)
    prompts = [[int(t) for t in rng.integers(0, cfg.vocab, n)] for n in PROMPT_LENGTHS]
    span, max_len = 16, 320
    fused8 = prefill_logits(model, prompts, max_len, span, True, True)
    unfused8 = prefill_logits(model, prompts, max_len, span, False, True)
    fused16 = prefill_logits(model, prompts, max_len, span, True, False)
    unfused16 = prefill_logits(model, prompts, max_len, span, False, False)
    skipped, worst8, worst16, worst_x = 0, 0.0, 0.0, 0.0
    for n, (lf, idf), (lu, idu), (lf16, _), (lu16, _) in zip(PROMPT_LENGTHS, fused8, unfused8, fused16, unfused16):
        scale = max(1.0, float(lu.abs().max()))
        d8 = float((lf - lu).abs().max())
        d16 = float((lf16 - lu16).abs().max())
        dx = float((lf - lf16).abs().max())
        top2 = torch.topk(lu, 2).values
        margin = float(top2[0] - top2[1])
        print(f"{cfg.hidden}-wide, {n:3d} tokens: fused vs unfused  A8W8 {d8 / scale:.3e}  A16W8 {d16 / scale:.3e} (of max |logit| {scale:.2f}); "
              f"A8W8 vs A16W8 (fused) {dx / scale:.3e}; unfused top-2 margin {margin:.3f}")
        worst8, worst16, worst_x = max(worst8, d8 / scale), max(worst16, d16 / scale), max(worst_x, dx / scale)
        # (a) the bound tests/test_gpu_host_runner.py uses for fused vs unfused
        assert d8 <= 3e-2 * scale, f"{n} tokens: fused A8W8 list differs from the unfused one by {d8 / scale:.3e} of max |logit|"
        # (b) the first id wherever the unfused list's own top-2 margin exceeds twice that distance
        if margin > 2 * d8:
            assert idf == idu, f"{n} tokens: first id {idf} != {idu} at margin {margin:.3f}, distance {d8:.3e}"
        else:
            skipped += 1
    print(f"{cfg.hidden}-wide: worst fused-vs-unfused A8W8 {worst8:.3e}, A16W8 {worst16:.3e}; A8W8 vs A16W8 {worst_x:.3e} (not asserted); "
          f"{skipped}/{len(PROMPT_LENGTHS)} prompts without a decisive margin")
    assert 4 * skipped <= len(PROMPT_LENGTHS), f"{skipped} of {len(PROMPT_LENGTHS)} prompts skipped the id check (top-2 margin <= 2 x distance)"


def test_decode_after_an_a8w8_prefill_replays_bit_identically(pkg):
    """(c) six decode steps after the A8W8 prefill: graph replay == eager, the operator types of the A16W8 graph, and -- the decoder
    phase being GemmA16W8 on the same weights -- a cache written by the A8W8 prefill is the only difference to the A16W8 graph."""
    from dash_infer_amd import decoder
    cfg = decoder.ModelConfig("a8w8-runner-test", **SMALL)
    model = decoder.build_random_model(cfg, decoder.QuantSpec(8, -1), seed=43, keep_fp=True, decisive=1.5)
    rng = np.random.default_rng(43)
    prompts = [[int(t) for t in rng.integers(0, cfg.vocab, n)] for n in (19, 70)]
    span, max_len, steps = 16, 96, 6
    runs, types = {}, {}
    for tag, graph, act_quant in (("graph", True, True), ("eager", False, True), ("a16w8", True, False)):
        h = A8Host(model, 2, max_len, span, "none", fuse=True, act_quant=act_quant)
        assert h.report["fused"], h.report["why"]
        types[tag] = h.report["types"]
        firsts = []
        for pr in prompts:
            k, v = h.spans()
            firsts.append(h.start(pr, k, v))
        out = []
        for _ in range(steps):
            ids = h.steps(1, graph=graph)
            out.append((h.logits().float().clone(), ids))
        runs[tag] = (firsts, out)
        h.close()
    assert types["graph"] == types["a16w8"]
    assert runs["graph"][0] == runs["eager"][0]
    for t, ((la, ia), (lb, ib)) in enumerate(zip(runs["graph"][1], runs["eager"][1])):
        assert ia == ib and torch.equal(la, lb), f"step {t}"
    assert all(torch.isfinite(l).all() for l, _ in runs["graph"][1])
