#!/usr/bin/env python3
"""bench.py -- decode tokens/s (+ achieved HBM GB/s) of the quantized decode hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload int4_b1|int8_b1|int4_b32_u4kv] [--full] [--dump-outputs DIR]

A "step" is one decode step of Qwen2-7B (synthetic InstantQuant weights, synthetic KV history of
2048 tokens) over one batch; at N > 1 the model is tensor-parallel over N ranks (one process per
GPU, RCCL all-reduce over xGMI) -- total work is fixed, so scaling is "strong".  W warm-up graph
replays, then exactly K replays are timed between barrier + synchronize on both sides; the maximum
over ranks is used; rank 0 prints ONE JSON line.

A plain run does only that, on the path `value` comes from (its warm-up ends with one untimed pass of
min(K, 256) steps, so that its one timed block is not a cold first one).  --full adds everything else the record
holds: the other runner's figures, per-kernel breakdown and roofline, CPU baselines, the secondary
workloads, and the median of 5 such K-step blocks.  --dump-outputs DIR writes what the timed path
computed in its last step (logits, next token ids) as DIR/<name>.npy; the inputs are seeded, so two
builds can be compared output for output.

Default workload: the configuration BASELINE.json's metric and target are quoted on -- Qwen2-7B int4
(group 128) weight-only, bf16 KV, batch 1, seq 2048 (first row).
`--workload int8_b1` is BASELINE.json configs[1]; `int4_b32_u4kv` is configs[2].
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    #                 wbits group kv     batch gptq
    "int4_b1":       (4, 128, "none", 1, True),
    "int8_b1":       (8, -1, "none", 1, False),
    "int4_b32_u4kv": (4, 128, "u4", 32, True),
    # BASELINE configs[3]: ONE RANK'S SHARE of Qwen2-72B int4 g128 at TP = 8 (per-rank shapes of SURVEY 8(a3): 8 query / 1 KV
    # head, qkv 8192 -> 1280, o 1024 -> 8192, gate/up 8192 -> 3712, down 3712 -> 8192, vocabulary slice 19008; 80 layers),
    # batch 16, 4096 cached tokens.  The all-reduces are NOT in it (one GPU): it is the rank-local part of the TP = 8 step.
    "cfg3_rank":     (4, 128, "none", 16, True),
    # The headline model's TP = 8 target on ONE GPU: rank 0's share of Qwen2-7B int4 g128 at TP = 8 (tp.py: 4 of the 28 query heads +
    # their replicated KV head, qkv 3584 -> 768, o 512 -> 3584, gate/up 3584 -> 2432 (19 of the 148 groups), down 2432 -> 3584,
    # vocabulary slice 19008; 28 layers, ~15.4 MB of weights per layer), batch 1, 2048 cached tokens.  All-reduces NOT in it: the
    # rank-local part of the TP = 8 step, i.e. the ceiling of the >= 3.5x target (per-layer fixed cost does not shard).
    "tp8_rank_7b":   (4, 128, "none", 1, True),
    # BASELINE configs[4] (decode part): the MoE feed-forward block of Qwen2-57B-A14B -- router, top-8 of 64 int8 experts
    # (3584 -> 2560 -> 3584), combine -- 16 tokens, 28 layers' expert stacks; attention / shared expert are the dense path
    "moe_layer":     (8, -1, "none", 16, False),
    # BASELINE configs[4] as a whole decode step on ONE GPU: Qwen2-57B-A14B int8 per-channel (attention, router, 64 routed experts
    # top-8, shared expert behind its sigmoid gate; 28 layers, ~57 GB of int8 weights), batch 16, 1024 cached tokens ("prefix")
    "cfg5_moe":      (8, -1, "none", 16, False),
    # the CONTEXT phase of the headline model (north star: "MFMA utilisation for prefill shown against gfx950 peaks"): one
    # "step" = the product's DecodeSession.prefill of ONE 2048-token prompt through all 28 layers (qkv GEMM, Rotary, ContextSpanCopy,
    # MFMA prefill attention, o / gate-up / down GEMMs, lm_head on the last row); value = prompt tokens / s; roofline = the
    # prefill attention kernel against the dense bf16 MFMA peak
    "prefill_2048":  (4, 128, "none", 1, True),
}
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 / f16 MFMA
SEQ_LEN = 2048
SEQ_LEN_OF = {"cfg3_rank": 4096, "cfg5_moe": 1024}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s


def load_pkg():
    from __graft_entry__ import _load_pkg
    return _load_pkg()


def cpu_baseline(wbits, group, cores_hint=None):
    """The oracle ("port": plain-C restatement of the reference's CPU_SubC_Ref loop, OpenMP over the
    host cores) timed on a bounded sample: the five linear layers of ONE Qwen2-7B decoder layer at
    batch 1; decode tokens/s is extrapolated over 28 layers (attention and lm_head excluded: the
    sample bounds the CPU path from above)."""
    import numpy as np
    from oracle import cbind
    rng = np.random.default_rng(0)
    shapes = [(3584, 4608), (3584, 3584), (3584, 18944), (3584, 18944), (18944, 3584)]
    cores = os.cpu_count() or 1
    cases = []
    for K, N in shapes:
        G = (K + group - 1) // group if group > 0 else 1
        x = rng.uniform(-1, 1, (1, K)).astype(np.float32)
        s = rng.uniform(0.001, 0.002, (G, N)).astype(np.float32)
        z = rng.uniform(0, 15, (G, N)).astype(np.float32)
        q = rng.integers(0, 256, (K, (N + 1) // 2 if wbits == 4 else N), dtype=np.uint8)
        if wbits == 8:
            q = q.view(np.int8)
        cases.append((x, q, s, z))
        cbind.gemm_a16wx(x, q, s, z, group, wbits, ft="bf16")  # warm (thread pool, page faults)
    def one_pass():
        t0 = time.perf_counter()
        for x, q, s, z in cases:
            cbind.gemm_a16wx(x, q, s, z, group, wbits, ft="bf16")
        return time.perf_counter() - t0

    # thread count: all logical CPUs is not always the fastest (SMT siblings, cgroup quotas, other tenants: 7 ... 200 ms
    # observed for the same pass with 256 threads); calibrate over a few counts, then measure with the best one
    try:
        import ctypes, ctypes.util
        gomp = ctypes.CDLL(ctypes.util.find_library("gomp") or "libgomp.so.1")
        best = (None, None)
        for n in sorted({cores, max(1, cores // 2), max(1, cores // 4), min(cores, 64), min(cores, 32)}, reverse=True):
            gomp.omp_set_num_threads(n)
            one_pass()
            t = sorted(one_pass() for _ in range(5))[2]
            if best[0] is None or t < best[0]:
                best = (t, n)
        cores = best[1]
        gomp.omp_set_num_threads(cores)
    except Exception:  # noqa: BLE001 -- no libgomp handle: OpenMP's own default
        pass
    # repeat the one-layer sample for about budget_s seconds of CPU work (a single pass is tens of ms); median pass
    budget_s, passes, t_start = 6.0, [], time.perf_counter()
    while len(passes) < 3 or (time.perf_counter() - t_start < budget_s and len(passes) < 400):
        passes.append(one_pass())
    passes.sort()
    t_layer = passes[len(passes) // 2]
    return {"value": round(1.0 / (28 * t_layer), 3), "unit": "tokens/s", "cores": cores, "kind": "port",
            "sample": "plain-C oracle (CPU_SubC_Ref loop, OpenMP) on the 5 linear layers of 1 of 28 Qwen2-7B decoder "
                      f"layers at batch 1, extrapolated x28; median of {len(passes)} passes in "
                      f"{time.perf_counter() - t_start:.1f} s: {t_layer * 1e3:.1f} ms/layer (min {passes[0] * 1e3:.1f}, "
                      f"max {passes[-1] * 1e3:.1f})"}


def cpu_baseline_torch(wbits, group, seq_len=SEQ_LEN, budget_s=15.0, weights="bf16"):
    """the reference's x86 path cannot be built here (oneDNN / MKL / intel_gemm are LFS stubs), so the
    SAME decode graph is timed through PyTorch-CPU (oneDNN + MKL, the libraries the reference's x86 operators call:
    csrc/core/operator/general/gemm/gemm_op_cpu.cpp:75-126, generate_opt/batch_mqa/batch_mqa_op.cpp:140-179) on this box's
    host cores: f32 activations, linear layers as bf16(x) . bf16(W_dequantised) -> f32, attention as alpha Q K^T -> f32 softmax
    -> P V over a contiguous f32 cache of `seq_len` tokens, RMSNorm / RoPE / SwiGLU / residual in f32, bf16 lm_head.  Whole
    Qwen2-7B step = 28 decoder layers + final norm + lm_head at batch 1; the timed sample runs the layer graph over 4 distinct
    layers' weights in rotation (1.9 GB: larger than the last-level caches) and the lm_head once per 28 layer passes."""
    import platform
    import torch
    torch.manual_seed(0)
    hid, n, g, H, inter, vocab, L = 3584, 28, 4, 128, 18944, 152064, 28
    cores = os.cpu_count() or 1

    wdt = torch.bfloat16 if weights == "bf16" else torch.float32

    def mk(K, N):  # a dequantised weight as the x86 path would hold it: bf16 (medium_bf16) or f32 [K, N]
        return (torch.randn(K, N, dtype=torch.float32) * 0.02).to(wdt)

    nrot = 4
    layers = [dict(qkv=mk(hid, (n + 2 * g) * H), qkv_b=torch.zeros((n + 2 * g) * H), o=mk(n * H, hid), gate=mk(hid, inter),
                   up=mk(hid, inter), down=mk(inter, hid), ln1=torch.ones(hid), ln2=torch.ones(hid),
                   k=torch.randn(g, seq_len + 1, H), v=torch.randn(g, seq_len + 1, H)) for _ in range(nrot)]
    lm_head, fnorm = mk(hid, vocab), torch.ones(hid)
    inv = 1.0 / (1e6 ** (torch.arange(0, H, 2, dtype=torch.float32) / H))
    ang = seq_len * inv
    cos, sin = torch.cos(ang), torch.sin(ang)

    def lin(x, w):
        return torch.mm(x.to(wdt), w).float()

    def rms(x, gam):
        return (gam * x) * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6)

    def rope(t):  # [heads, H]
        a, b = t[:, : H // 2], t[:, H // 2:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

    def layer(h, w):
        qkv = lin(rms(h, w["ln1"]), w["qkv"]) + w["qkv_b"]
        q = rope(qkv[0, : n * H].view(n, H)).view(g, n // g, H)
        w["k"][:, seq_len] = rope(qkv[0, n * H:(n + g) * H].view(g, H))
        w["v"][:, seq_len] = qkv[0, (n + g) * H:].view(g, H)
        p = torch.softmax(torch.bmm(q, w["k"].transpose(1, 2)) * (H ** -0.5), -1)   # [g, n/g, L+1]
        att = torch.bmm(p, w["v"]).reshape(1, n * H)
        h = h + lin(att, w["o"])
        x2 = rms(h, w["ln2"])
        act = torch.nn.functional.silu(lin(x2, w["gate"])) * lin(x2, w["up"])
        return h + lin(act, w["down"])

    def one_step_sample():  # 28 layer passes + lm_head = one token
        h = torch.randn(1, hid)
        t0 = time.perf_counter()
        for i in range(L):
            h = layer(h, layers[i % nrot])
        logits = lin(rms(h, fnorm), lm_head)
        int(torch.argmax(logits))
        return time.perf_counter() - t0

    with torch.no_grad():
        best = (None, None)
        for nthr in sorted({cores, max(1, cores // 2), max(1, cores // 4), min(cores, 64), min(cores, 32)}, reverse=True):
            torch.set_num_threads(nthr)
            one_step_sample()
            t = min(one_step_sample() for _ in range(2))
            if best[0] is None or t < best[0]:
                best = (t, nthr)
        torch.set_num_threads(best[1])
        ts, t_start = [], time.perf_counter()
        while len(ts) < 3 or (time.perf_counter() - t_start < budget_s and len(ts) < 200):
            ts.append(one_step_sample())
    ts.sort()
    med = ts[len(ts) // 2]
    cpu_model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        cpu_model = platform.processor()
    return {"value": round(1.0 / med, 3), "unit": "tokens/s", "cores": best[1], "kind": "port", "port_of": "the reference's x86 decode graph on the libraries its CPU operators call (oneDNN / MKL via PyTorch-CPU): a stand-in, the reference's own x86 build needs LFS-stubbed libraries", "weights": weights,
            "library": f"PyTorch-CPU {torch.__version__} (oneDNN / MKL), torch.set_num_threads({best[1]}) of {cores} logical CPUs; {cpu_model}",
            "sample": f"whole Qwen2-7B decode step at batch 1, seq {seq_len}: 28 x [RMSNorm, qkv bf16 GEMV + bias, RoPE, GQA attention over "
                      f"{seq_len + 1} cached tokens (f32), o GEMV + residual, RMSNorm, gate/up GEMV + SwiGLU, down GEMV + residual] over "
                      f"{nrot} distinct layers' {weights} weights in rotation + final norm + {weights} lm_head + argmax; median of {len(ts)} steps in "
                      f"{time.perf_counter() - t_start:.1f} s ({med * 1e3:.1f} ms/token; min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f}); "
                      f"weights dequantised to {weights} as the x86 path holds them (int{wbits} g{group} on the GPU)"}


def timed_blocks(run_n, steps, blocks, world=1, device=None, sync=None, before_block=None):
    """`blocks` timed blocks of EXACTLY `steps` steps each.  A block is bracketed by barrier + synchronize on both sides; its time
    is the MAXIMUM over the ranks (all-reduce MAX on `device`: the GPU under RCCL, the CPU under gloo in the tests).  before_block runs
    untimed in front of each block (rewinding the sequences: every block then decodes the same positions).  The reported
    time is the MEDIAN block (one clock ramp or a noisy neighbour cannot move the headline); min / max ride
    along.  -> (median_s, [block seconds, max over ranks])"""
    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
    if sync is None:
        sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)

    def barrier():
        sync()
        if dist is not None:
            dist.barrier()
        sync()

    times = []
    for _ in range(max(1, blocks)):
        if before_block is not None:   # untimed: e.g. rewind the sequences so that every block decodes the same positions
            before_block()
        barrier()
        t0 = time.perf_counter()
        run_n(steps)
        barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=device if device is not None else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        times.append(el)
    srt = sorted(times)
    return srt[len(srt) // 2], times


def settle_steps(args):
    """Warm-up steps a plain run adds after --warmup, rewound like a block and untimed: its ONE timed block is then not the slow
    first block that --full's median of 5 leaves out.  A fixed count: the dumped outputs stay the same from run to run."""
    return 0 if args.full else min(args.steps, 256)


def blocks_summary(times, steps):
    srt = sorted(times)
    return {"count": len(times), "steps_each": steps, "ms_per_step_median": round(srt[len(srt) // 2] / steps * 1e3, 4),
            "ms_per_step_min": round(srt[0] / steps * 1e3, 4), "ms_per_step_max": round(srt[-1] / steps * 1e3, 4),
            "spread": round((srt[-1] - srt[0]) / srt[len(srt) // 2], 4)}


def host_runner_bench(args, torch, decoder, ops, model, sess, batch, max_len, kv_mode, fuse, graph, steps, blocks, outputs=None):
    """The SAME decode step through the C++ operator layer (dash-infer_amd/host): the reference's Qwen2 operator list
    (dash-infer_amd/ref_graph.py: qwen_v15.py:187-388; the MoE layers of qwen_v20_moe.py:318-391 for cfg5_moe) -> fusion pass (host/fusion_pass.cpp; fuse=False: the list as it is, fourteen launches
    per layer) -> OpFactory -> HipModelRunner (host/model_runner.cpp: Alloc -> Forward per operator per step, model.cpp:1248-1325),
    the fused step captured once as a hipGraph and replayed.  The requests adopt the Python session's cache spans (same random
    history); the weights are the same quantised tensors, re-laid-out by the operators' own InitV2."""
    from dash_infer_amd import hostapi
    from dash_infer_amd import ref_graph
    cfg = model.cfg
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    kvc = {"none": 0, "i8": 1, "u4": 2}[kv_mode]
    with torch.cuda.stream(stream):
        m = hostapi.Model(ops.cur_stream(), cfg.n_heads, cfg.n_kv, cfg.head_dim, sess.pool.S, kvc, max_batch=batch, max_len=max_len)
        try:
            ref_graph.register_weights(m, model)
            g = ref_graph.qwen2_graph(len(model.layers), model.quant.wbits, model.quant.group, cfg.eps, cfg.n_heads, cfg.n_kv, cfg.rope_theta,
                                      moe=(cfg.moe.num_experts, cfg.moe.top_k) if cfg.moe is not None else None)
            # the list travels as a SERIALIZED allspark TransformerProto (csrc/proto/allspark.proto) and enters the C++ layer through its
            # wire-format reader (host/graph_wire.h) -- the ingest AsModel does from a converter export (model.cpp:265-287)
            m.graph_add_serialized(ref_graph.to_transformer_proto(g))
            rep = m.graph_build(fuse=fuse)
            gen = torch.Generator().manual_seed(7)
            ids = torch.randint(0, cfg.vocab, (batch,), generator=gen).tolist()
            for b in range(batch):
                ks = [[int(p) for p in sess.kv[li].k_host[b].tolist()] for li in range(len(model.layers))]
                vs = [[int(p) for p in sess.kv[li].v_host[b].tolist()] for li in range(len(model.layers))]
                m.request_adopt(SEQ_LEN, ids[b], ks, vs)
            m.decode_steps(max(2, args.warmup), graph=graph)
            if settle_steps(args):
                m.requests_rewind(SEQ_LEN)
                m.decode_steps(settle_steps(args), graph=graph)
            m.sync_ids()

            def run_n(n):
                m.decode_steps(n, graph=graph)

            med, times = timed_blocks(run_n, steps, blocks, sync=stream.synchronize, before_block=lambda: m.requests_rewind(SEQ_LEN))
            last = m.sync_ids()
            if outputs is not None:   # --dump-outputs: the last timed step's logits and next ids, copied before the model is closed
                outputs.update(logits=model_tensor(m, "logits"), next_ids=last)
        finally:
            m.close()
    return {"tokens_per_s": round(batch * steps / med, 2), "ms_per_step": round(med / steps * 1e3, 4), "blocks": blocks_summary(times, steps),
            "fused": rep["fused"], "operators": f"{rep['ops']} ({len(rep['types'])} operators run per step)", "hipGraph": bool(graph),
            "why_unfused": rep["why"] if not rep["fused"] else None, "last_ids": last[:4]}


def host_runner_bench_tp(args, torch, decoder, ops, cfg, spec, sess, comm, batch, max_len, kv_mode, rank, world, local_rank, steps, blocks,
                         outputs=None):
    """N > 1: the decode step through the C++ operator layer on every rank -- one HipModelRunner per rank PROCESS over
    its tp.py weight slices (the reference-shaped K-split lm_head: Gemm(splitk) + AllReduce, model_base.py:690-703), the reference's
    operator list with its AllReduce operators -> fusion pass -> OpFactory(HIP), HIPContext carrying the rank's RCCL communicator (and
    the one-shot P2P communicator when it passed its probe: AllReduceOpHIP takes it for decode rows), the step captured and replayed as
    a hipGraph.  Set-up is VOTED: a rank that cannot build its model makes every rank skip the leg (nobody is left alone in a
    collective).  -> the host_runner record, or {"skipped": why}."""
    import torch.distributed as dist
    from dash_infer_amd import hostapi, ref_graph
    dev = torch.device("cuda", local_rank)
    m, err, stream = None, None, torch.cuda.Stream()
    rccl = comm.rccl if isinstance(comm, decoder.P2PComm) else comm
    try:
        if not isinstance(rccl, decoder.RcclComm):
            raise RuntimeError(f"the C++ layer needs the C-ABI RCCL communicator (got {type(rccl).__name__})")
        model_k = decoder.build_random_model(cfg, spec, seed=1234, rank=rank, nranks=world, layers=args.layers, keep_fp=True, lm_head_split="k")
        kvc = {"none": 0, "i8": 1, "u4": 2}[kv_mode]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            m = hostapi.Model(ops.cur_stream(), cfg.n_heads, cfg.n_kv, cfg.head_dim, sess.pool.S, kvc, max_batch=batch, max_len=max_len,
                              rank=rank, nranks=world, comm=rccl.handle)
            if isinstance(comm, decoder.P2PComm):
                m.set_p2p_comm(comm.handle)
            ref_graph.register_weights(m, model_k)
            g = ref_graph.qwen2_graph(len(model_k.layers), model_k.quant.wbits, model_k.quant.group, cfg.eps, cfg.n_heads, cfg.n_kv, cfg.rope_theta,
                                      tp_allreduce=True, tp_lm_head=True)
            m.graph_add_serialized(ref_graph.to_transformer_proto(g))
            rep = m.graph_build(fuse=True)
            if not (rep["fused"] and rep["device_resident"]):
                raise RuntimeError("the tensor-parallel list did not fuse: " + rep["why"])
            gen = torch.Generator().manual_seed(7)
            ids = torch.randint(0, cfg.vocab, (batch,), generator=gen).tolist()
            for b in range(batch):
                ks = [[int(p) for p in sess.kv[li].k_host[b].tolist()] for li in range(len(model_k.layers))]
                vs = [[int(p) for p in sess.kv[li].v_host[b].tolist()] for li in range(len(model_k.layers))]
                m.request_adopt(SEQ_LEN, ids[b], ks, vs)
        stream.synchronize()
    except Exception as e:  # noqa: BLE001
        err = f"{type(e).__name__}: {e}"[:300]
    ok = torch.tensor([0 if err else 1], dtype=torch.int32, device=dev)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 0:
        if m is not None:
            m.close()
        return {"skipped": err or "another rank could not set the C++ runner up"}
    try:
        with torch.cuda.stream(stream):
            m.decode_steps(max(2, args.warmup), graph=True)
            if settle_steps(args):
                m.requests_rewind(SEQ_LEN)
                m.decode_steps(settle_steps(args), graph=True)
            m.sync_ids()

            def run_n(n):
                m.decode_steps(n, graph=True)

            med, times = timed_blocks(run_n, steps, blocks, world, dev, sync=stream.synchronize, before_block=lambda: m.requests_rewind(SEQ_LEN))
            last = m.sync_ids()
            if outputs is not None:
                outputs.update(logits=model_tensor(m, "logits"), next_ids=last)
    finally:
        m.close()
    return {"fused_graph": {"tokens_per_s": round(batch * steps / med, 2), "ms_per_step": round(med / steps * 1e3, 4), "blocks": blocks_summary(times, steps),
                            "fused": True, "operators": f"{rep['ops']} ({len(rep['types'])} operators run per step)", "hipGraph": True,
                            "allreduce": "AllReduceOpHIP: " + ("one-shot P2P for decode rows, RCCL beyond" if isinstance(comm, decoder.P2PComm) else "RCCL"),
                            "lm_head": "K-split Gemm + AllReduce (the reference's TP tail)", "last_ids": last[:4]}}


def prefill_bench(args, torch, decoder, ops, outputs):
    """--workload prefill_2048 (see WORKLOADS).  Timed with HIP events on the launch stream around whole prefill calls (eager
    launches: the context phase is not graph-captured); with --full, the attention kernel alone is timed the same way over all
    layers' calls, and every GEMM of a layer alone."""
    wbits, group, kv_mode, batch, gptq = WORKLOADS["prefill_2048"]
    cfg = decoder.QWEN2_7B
    L = 2048
    t0 = time.time()
    host_leg = args.runner in ("auto", "host")
    model = decoder.build_random_model(cfg, decoder.QuantSpec(wbits, group, gptq_like_zeros=gptq), seed=1234, layers=args.layers, keep_fp=host_leg)
    sess = decoder.DecodeSession(model, 1, max_len=L + 16, span_len=128, kv_mode=kv_mode)
    gen = torch.Generator().manual_seed(11)
    prompt = [int(t) for t in torch.randint(0, cfg.vocab, (L,), generator=gen)]
    t_build = time.time() - t0
    nl = len(model.layers)
    steps = max(1, args.steps)
    python_outputs = {}

    def time_python_runner():
        for _ in range(max(1, args.warmup)):
            sess.prefill([prompt])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t_wall = time.perf_counter()
        e0.record()
        for _ in range(steps):
            lo = sess.prefill([prompt])
        e1.record()
        torch.cuda.synchronize()
        t_wall = (time.perf_counter() - t_wall) / steps
        if args.dump_outputs:
            python_outputs.update(logits=lo.float().cpu().numpy(), next_ids=sess.ids.cpu().numpy())
        return e0.elapsed_time(e1) / steps, t_wall

    # a plain run times the path `value` comes from: the C++ operator layer, or the Python session where that does not run
    ms = t_wall = None
    if args.full or not host_leg:
        ms, t_wall = time_python_runner()
    # the same context phase through the C++ operator layer: serialized reference graph -> fusion pass -> OpFactory(HIP) -> model runner
    # (request_start = AsModel's context phase of one request: PreProcessId, embedding, the fused layers at M = 2048, GetLastLine, lm_head,
    # GenerateOp), over the Python session's span pool
    host = None
    host_outputs = {}
    if host_leg:
        try:
            host = prefill_host_bench(args, torch, ops, model, sess, prompt, steps, outputs=host_outputs if args.dump_outputs else None)
        except Exception as e:  # the line must still be printed: the Python session's figure stands
            host = {"error": f"{type(e).__name__}: {e}"[:300]}
    value_from_host = bool(host and "ms_per_prompt" in host and host.get("fused"))
    if not value_from_host and ms is None:
        ms, t_wall = time_python_runner()
    outputs.update(host_outputs if value_from_host else python_outputs)
    out_d = {
        "metric": "prefill (context phase) tokens/sec, Qwen2-7B weight-only quantized, one 2048-token prompt",
        "value": None, "unit": "tokens/s", "n_gpus": 1, "steps": steps, "warmup": args.warmup,
        "ms_per_step": None, "higher_is_better": True, "runner": "python: decoder.DecodeSession.prefill (ctypes over the C-ABI)",
        "python_runner": {"tokens_per_s": round(L / (ms * 1e-3), 1), "ms_per_prompt": round(ms, 3)} if ms is not None else None,
        "host_runner": host, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic (random-init InstantQuant weights of the Qwen2-7B shapes, random prompt)",
        "config": {"workload": f"Qwen2-7B prefill_2048: int{wbits} weight-only group {group}, 16-bit KV spans, batch 1, prompt {L} tokens, "
                               f"{nl} layers, eager launches (DecodeSession.prefill)", "global_batch": 1, "seq_len": L, "parallelism": "tp1",
                   "layers": nl},
        "build_s": round(t_build, 1),
    }
    if ms is not None:
        out_d["value"], out_d["ms_per_step"] = round(L / (ms * 1e-3), 1), round(ms, 3)
    if args.full:
        out_d.update(prefill_kernels(torch, ops, model, sess, cfg, wbits, group, L, ms, t_wall))
    if value_from_host:  # as for the decode workloads: `value` is the C++ operator layer's figure
        out_d["value"], out_d["ms_per_step"] = host["tokens_per_s"], host["ms_per_prompt"]
        out_d["runner"] = "host: C++ operator layer -- serialized reference graph -> fusion pass -> OpFactory(HIP) -> model runner (context phase, eager)"
    if args.layers is not None:
        out_d["invalid"] = "debug run with a truncated layer stack"
    return out_d


def prefill_kernels(torch, ops, model, sess, cfg, wbits, group, L, ms, t_wall):
    """--full, prefill_2048: the attention kernel and every GEMM of a layer alone, each timed with HIP events -> roofline, attention,
    gemms and context_phase of the record (`ms`, `t_wall`: the Python session's whole prefill)."""
    nl = len(model.layers)
    # the attention kernel alone: all layers' calls on resident fused qkv rows
    n, g, H = cfg.n_heads, cfg.n_kv, cfg.head_dim
    qkv = (torch.randn(L, (n + 2 * g) * H, device="cuda") * 0.5).to(torch.bfloat16)
    out = torch.empty(L, n * H, dtype=torch.bfloat16, device="cuda")
    def attn_all():
        for _ in range(nl):
            ops.prefill_attn(qkv[:, : n * H], qkv[:, n * H:(n + g) * H], qkv[:, (n + g) * H:], n, g, H, sess.scale, out=out)
    attn_all()
    torch.cuda.synchronize()
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record()
    for _ in range(5):
        attn_all()
    a1.record()
    torch.cuda.synchronize()
    attn_us = a0.elapsed_time(a1) / (5 * nl) * 1e3
    flops = 4.0 * n * H * L * L / 2.0   # causal: QK^T and PV, half the square
    tflops = flops / (attn_us * 1e-6) / 1e12
    # every GEMM of a layer alone, the same way: layer 0's weights on resident activations, the product's own calls
    lw = model.layers[0]
    sc = ops.Scratch(max(ops.lowp_workspace_bytes(wbits, L, p.N, p.K, group) for p in (lw.qkv, lw.o, lw.gate, lw.down)), "cuda")
    h = torch.randn(L, cfg.hidden, device="cuda") * 0.5
    attn_in = (torch.randn(L, n * H, device="cuda") * 0.5).to(torch.bfloat16)
    act_in = (torch.randn(L, lw.down.K, device="cuda") * 0.5).to(torch.bfloat16)
    calls = {
        "qkv_norm_gemm": (lambda: ops.fused_norm_gemm(h, lw.ln1, cfg.eps, lw.qkv, lw.qkv_bias, sc), lw.qkv.N * lw.qkv.K),
        "o_gemm_addto": (lambda: ops.fused_gemm_addto(attn_in, lw.o, h, sc, M=L), lw.o.N * lw.o.K),
        "gate_up_swiglu_gemm": (lambda: ops.fused_norm_swiglu(h, lw.ln2, cfg.eps, lw.gate, lw.up, sc), 2 * lw.gate.N * lw.gate.K),
        "down_gemm_addto": (lambda: ops.fused_gemm_addto(act_in, lw.down, h, sc, M=L), lw.down.N * lw.down.K),
    }
    gemms = {}
    for name, (fn, nk) in calls.items():
        fn()
        torch.cuda.synchronize()
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g0.record()
        for _ in range(20):
            fn()
        g1.record()
        torch.cuda.synchronize()
        us = g0.elapsed_time(g1) / 20 * 1e3
        gemms[name] = {"avg_us": round(us, 2), "tflops": round(2.0 * L * nk / (us * 1e-6) / 1e12, 1),
                       "share_of_step": round(us * nl / (ms * 1e3), 4)}
    # GEMM flops of the step (2 M N K per projection) for the record
    gemm_flops = 2.0 * L * sum(p.N * p.K for lw_ in model.layers for p in (lw_.qkv, lw_.o, lw_.gate, lw_.up, lw_.down))
    dom = gemms["gate_up_swiglu_gemm"]
    dom_flops = 2.0 * L * 2 * lw.gate.N * lw.gate.K
    return {
        # the kernel the context phase spends most of its time in (the launch includes the RMSNorm kernel in front of it)
        "roofline": {"bound": "mfma", "kernel": "dihip::gemm_prefill_kernel<4, bf16, SwiGLU> (RMSNorm + gate/up weight-only GEMM + SwiGLU, M = 2048)",
                     "achieved": dom["tflops"], "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(dom["tflops"] / MFMA_BF16_PEAK_TFLOPS, 4),
                     "traffic": None, "avg_launch_us": dom["avg_us"], "algorithmic_flops_per_launch": dom_flops},
        "attention": {"kernel": "dihip::prefill_attn_kernel (causal flash attention, 28 query / 4 KV heads, head 128)", "tflops": round(tflops, 1),
                      "frac_of_mfma_peak": round(tflops / MFMA_BF16_PEAK_TFLOPS, 4), "avg_launch_us": round(attn_us, 2),
                      "algorithmic_flops_per_launch": flops},
        "gemms": gemms,
        "context_phase": {"attention_share": round(attn_us * nl / (ms * 1e3), 4), "gemm_tflops_if_rest_were_gemm": round(
            gemm_flops / max(1e-9, (ms * 1e-3 - attn_us * nl * 1e-6)) / 1e12, 1), "host_wall_ms": round(t_wall * 1e3, 3)},
    }


def prefill_host_bench(args, torch, ops, model, sess, prompt, steps, outputs=None):
    from dash_infer_amd import hostapi
    from dash_infer_amd import ref_graph
    cfg = model.cfg
    L = len(prompt)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        m = hostapi.Model(ops.cur_stream(), cfg.n_heads, cfg.n_kv, cfg.head_dim, sess.pool.S, 0, max_batch=1, max_len=sess.max_len)
        try:
            ref_graph.register_weights(m, model)
            g = ref_graph.qwen2_graph(len(model.layers), model.quant.wbits, model.quant.group, cfg.eps, cfg.n_heads, cfg.n_kv, cfg.rope_theta)
            m.graph_add_serialized(ref_graph.to_transformer_proto(g))
            rep = m.graph_build(fuse=True)
            ks = [[int(p) for p in sess.kv[li].k_host[0].tolist()] for li in range(len(model.layers))]
            vs = [[int(p) for p in sess.kv[li].v_host[0].tolist()] for li in range(len(model.layers))]

            def once():
                first = m.request_start(prompt, ks, vs)
                m.request_stop(0)
                return first

            for _ in range(max(1, args.warmup)):
                once()
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t_wall = time.perf_counter()
            e0.record(stream)
            for _ in range(steps):
                first = once()
            e1.record(stream)
            stream.synchronize()
            t_wall = (time.perf_counter() - t_wall) / steps
            ms = e0.elapsed_time(e1) / steps
            if outputs is not None:   # --dump-outputs: the last prompt's logits (the lm_head row) and first generated id
                outputs.update(logits=model_tensor(m, "logits"), next_ids=[first])
        finally:
            m.close()
    return {"tokens_per_s": round(L / (ms * 1e-3), 1), "ms_per_prompt": round(ms, 3), "host_wall_ms": round(t_wall * 1e3, 3), "fused": rep["fused"],
            "operators": rep["ops"], "first_token": int(first) if first is not None else None}


def moe_layer_bench(args, torch, ops, outputs):
    """--workload moe_layer: one "step" = the mixture-of-experts block of all 28 layers for a batch of 16 tokens (each layer
    its own 64-expert stack: 49 GB, nothing cache-resident).  Algorithmic bytes per layer: every (token, expert) slot streams
    3 * hidden * width int8 weights + scales unless another slot of the step picked the same expert; counted per distinct
    expert actually selected by the synthetic router logits."""
    E, k, hidden, proj, wbits, L, T = 64, 8, 3584, 2560, 8, 28, 16
    dt = torch.bfloat16

    def experts(N, K):
        q = torch.randint(-128, 128, (K, N), dtype=torch.int8, device="cuda")
        s = (torch.rand(1, N, device="cuda") * 0.002 + 0.007).to(dt)
        z = (torch.rand(1, N, device="cuda") * 4 - 2).to(dt)
        return ops.pack_experts([q] * E, [s] * E, [z] * E, -1, wbits)

    t0 = time.time()
    stacks = [(experts(proj, hidden), experts(proj, hidden), experts(hidden, proj)) for _ in range(L)]
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(T, hidden, device="cuda", generator=gen).to(dt)
    logits = [torch.randn(T, E, device="cuda", generator=gen).to(dt) for _ in range(L)]
    ws = torch.empty(int(ops.lib().dihip_moe_workspace_bytes(T, k, hidden, proj)), dtype=torch.uint8, device="cuda")
    out = torch.empty(T, hidden, dtype=dt, device="cuda")
    distinct = 0
    for li in range(L):
        _, ex = ops.moe_route(logits[li], k)
        distinct += int(torch.unique(ex).numel())
    t_build = time.time() - t0

    def step():
        for li, (g, u, d) in enumerate(stacks):
            sc, ex = ops.moe_route(logits[li], k)
            ops.moe_experts(x, ex, sc, g, u, d, ws=ws, out=out)

    step()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    for _ in range(args.warmup):
        gr.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gr.replay()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        outputs["out"] = out.float().cpu().numpy()
    ms = elapsed / args.steps * 1e3
    bytes_step = distinct * (3 * hidden * proj + 2 * (2 * proj + hidden) * 2)  # int8 weights + bf16 (scale, zero) per column
    gbs = bytes_step / (ms * 1e-3) / 1e9
    return {
        "metric": "MoE feed-forward block: tokens/sec through 28 layers (+ achieved HBM GB/s), Qwen2-57B-A14B int8 experts",
        "value": round(T * args.steps / elapsed, 2), "unit": "tokens/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic (random int8 expert weights, random router logits)",
        "config": {"workload": f"Qwen2-57B-A14B moe_layer: router softmax/top-{k} + {E} int8 per-channel experts ({hidden}->{proj}->{hidden}) + "
                               f"combine, {T} tokens, {L} layers' expert stacks (attention, shared expert and the TP all-reduce are "
                               "not in this workload), hipGraph=on", "global_batch": T, "parallelism": "tp1", "layers": L},
        "step_hbm": {"algorithmic_bytes_per_rank": int(bytes_step), "achieved_GBps_per_gpu": round(gbs, 1),
                     "frac_of_peak": round(gbs / HBM_PEAK_GBS, 4), "distinct_experts_per_step": distinct},
        "roofline": {"bound": "hbm", "kernel": "dihip::gemv_stream_kernel<8, 2, 4, 0, *, 0, true> (expert GEMVs over GROUPS of up to 4 (token, expert) slots that picked "
                               "the same expert; DIHIP_MOE_GROUP=0: <8, 2, 1, ...>, one slot per launch row)",
                     "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                     "traffic": None, "note": "whole-block figure: route + gate/up + down + combine launches"},
        "build_s": round(t_build, 1),
    }


def kernel_breakdown(sess, torch, ops, iters=5):
    """Average launch duration of every hot-path kernel: the launches of all layers (each layer its
    own weights: 1.9+ GB per sweep, far beyond the 256 MB Infinity Cache) are captured into one
    hipGraph per kernel kind and replayed; HIP events on the launch stream bracket the replays.  The
    figure includes the ~1.6 us dependent-launch boundary of a graph node chain."""
    m, cfg, sc = sess.model, sess.model.cfg, sess.scratch
    B = sess.B
    res = {}

    def timed(name, nbytes, fn, layers=None):
        layers = m.layers if layers is None else layers
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for li, lw in enumerate(layers):
                fn(li, lw)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for li, lw in enumerate(layers):
                fn(li, lw)
        for _ in range(3):  # warm replays: clocks / caches settle before the timed ones
            g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / len(layers))
        avg = sum(ts) / len(ts)
        res[name] = {"avg_us": round(avg * 1e3, 2), "min_us": round(min(ts) * 1e3, 2), "bytes": int(nbytes),
                     "GBps": round(nbytes / (avg * 1e-3) / 1e9, 1)}

    l0 = m.layers[0]
    act_b = lambda p: B * p.K * 2 + B * p.N * 2
    timed("qkv_norm_gemv", l0.qkv.nbytes + act_b(l0.qkv),
          lambda li, lw: ops.fused_norm_gemm(sess.h, lw.ln1, cfg.eps, lw.qkv, lw.qkv_bias, sc, out=sess.qkv))
    kvb = {"none": sess.H * 2, "i8": sess.H + 8, "u4": sess.H // 2 + 8}[sess.kv_mode]
    if sess.fused_attention:
        timed("rope_append_span_attention", B * 2 * sess.g_loc * SEQ_LEN * kvb,
              lambda li, lw: ops.span_attn_decode_fused(sess.qkv, sess.kv[li], sess.old_lens, sess.rope_tab, sess.n_loc, sess.g_loc,
                                                        sess.H, sess.max_len, sess.scale, sess.attn_ws, out=sess.attn,
                                                        sync=sess.attn_sync if sess.attn_merge_in_launch else None))
    elif getattr(sess, "step_attention", False):   # uint4 cache, bf16 rows: one launch (dihip_span_attn_decode_step)
        timed("rope_append_span_attention", B * 2 * sess.g_loc * SEQ_LEN * kvb,
              lambda li, lw: ops.span_attn_decode_step(sess.qkv, sess.kv[li], sess.old_lens, sess.rope_tab, sess.n_loc, sess.g_loc, sess.H,
                                                       sess.max_len, sess.scale, sess.attn_ws,
                                                       sess.attn_sync if sess.attn_merge_in_launch else None, out=sess.attn,
                                                       out_layout=ops.ACT_FRAG32 if sess.attn_frag else ops.ACT_ROWMAJOR))
    else:
        def sep(li, lw):
            ops.rope_kv_append(sess.kv[li], sess.q, sess.qkv, sess.old_lens, sess.inv_freq, sess.n_loc, sess.g_loc, sess.H)
            ops.span_attn_decode(sess.q, sess.kv[li], sess.new_lens, sess.n_loc, sess.g_loc, sess.H, sess.max_len, sess.scale,
                                 sess.attn_ws, sess.attn_sync, out=sess.attn,
                                 out_layout=ops.ACT_FRAG32 if sess.attn_frag else ops.ACT_ROWMAJOR)
        timed("rope_append_span_attention", B * 2 * sess.g_loc * SEQ_LEN * kvb, sep)
    if getattr(sess, "attn_block", False):
        # what the step actually runs at batch 1 (round 5): the three operators above + the o-projection below as ONE launch
        timed("attn_block_qkv_attention_o", l0.qkv.nbytes + act_b(l0.qkv) + B * 2 * sess.g_loc * SEQ_LEN * kvb + l0.o.nbytes + act_b(l0.o),
              lambda li, lw: ops.decode_attn_block(sess.h, sess.h, lw.ln1, cfg.eps, lw.qkv, lw.qkv_bias, lw.o, sess.kv[li], sess.old_lens, sess.rope_tab,
                                                   sess.n_loc, sess.g_loc, sess.H, sess.max_len, sess.scale, sess.attn_ws, sess.block_sync, out=sess.partial))
    timed("o_gemv_addto", l0.o.nbytes + act_b(l0.o),
          lambda li, lw: ops.fused_gemm_addto(sess.attn, lw.o, sess.h, sc, out=sess.partial, M=B,
                                              x_layout=ops.ACT_FRAG32 if sess.attn_frag else ops.ACT_ROWMAJOR))
    timed("gate_up_swiglu", l0.gate.nbytes + l0.up.nbytes + B * l0.gate.K * 4 + B * l0.gate.N * 2,
          lambda li, lw: ops.fused_norm_swiglu(sess.h, lw.ln2, cfg.eps, lw.gate, lw.up, sc, out=sess.act,
                                               y_layout=ops.ACT_FRAG32 if sess.act_frag else ops.ACT_ROWMAJOR))
    timed("down_gemv_addto", l0.down.nbytes + act_b(l0.down),
          lambda li, lw: ops.fused_gemm_addto(sess.act, lw.down, sess.h, sc, out=sess.partial, M=B,
                                              x_layout=ops.ACT_FRAG32 if sess.act_frag else ops.ACT_ROWMAJOR))
    timed("lm_head", m.lm_head.nbytes,
          lambda li, lw: ops.lm_head(sess.h, m.final_norm, cfg.eps, m.lm_head, sc, out=sess.logits), layers=[None] * 4)
    return res


def allreduce_alone(torch, comm, sess, n_layers, graph_on, step_ms, world):
    """Time of the step's hidden-row all-reduces alone (2 per layer), back to back, max over ranks."""
    import torch.distributed as dist

    def barrier():
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
    try:
        n_ar = 2 * n_layers
        buf = torch.zeros_like(sess.h)

        def ar_only():
            for _ in range(n_ar):
                comm.allreduce_(buf)
        s_ar = torch.cuda.Stream()
        s_ar.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_ar):
            ar_only()
        torch.cuda.current_stream().wait_stream(s_ar)
        barrier()
        if graph_on:
            g_ar = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_ar):
                ar_only()
            run_ar = g_ar.replay
        else:
            run_ar = ar_only
        run_ar()
        barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            run_ar()
        e1.record()
        barrier()
        ar_ms = e0.elapsed_time(e1) / 5
        t_ar = torch.tensor([ar_ms], dtype=torch.float64, device="cuda")
        dist.all_reduce(t_ar, op=dist.ReduceOp.MAX)
        ar_ms = float(t_ar.item())
        return {"count_per_step": n_ar, "bytes_each": int(buf.numel() * buf.element_size()),
                "us_per_step": round(ar_ms * 1e3, 1), "us_each": round(ar_ms * 1e3 / n_ar, 2),
                "share_of_step": round(ar_ms / step_ms, 4),
                "note": "the step's hidden-row all-reduces alone, back to back (max over ranks); inside the step they also wait for the slowest rank's GEMV"}
    except Exception as e:  # noqa: BLE001 -- never lose the headline number to a diagnostic
        return {"error": repr(e)}


def tp_ab_runs(args, torch, decoder, model, comm, batch, max_len, kv_mode, ids, rank, world, local_rank, blocks=3):
    """TP > 1: the decode step under {rccl, p2p-oneshot} x {all-reduce on the compute stream, on a side stream beside the next
    GEMV's weight prefetch}, each its own DecodeSession + hipGraph over the SAME sharded model, `blocks` blocks of --steps steps
    (median, max over ranks).  Every rank walks the same list in the same order (collectives inside)."""
    dev = torch.device("cuda", local_rank)
    comms = []
    rccl = comm.rccl if isinstance(comm, decoder.P2PComm) else comm
    comms.append(("rccl", rccl))
    if isinstance(comm, decoder.P2PComm):
        comms.append(("p2p-oneshot", comm))
    else:
        comms.append(("p2p-oneshot", None))   # unavailable / failed verification on this node: recorded as such
    res = []
    for name, c in comms:
        for overlap in (False, True):
            row = {"allreduce": name, "overlap": overlap}
            if c is None:
                row["skipped"] = f"not available here: {getattr(comm, 'backend', None)}"
                res.append(row)
                continue
            try:
                sv = decoder.DecodeSession(model, batch, max_len, span_len=128, kv_mode=kv_mode, comm=c, ar_overlap=overlap)
                sv.fill_cache_random(SEQ_LEN)
                sv.set_state(ids, [SEQ_LEN] * batch)
                try:
                    sv.capture(warmup=1)
                    run_n, graph_on = sv.replay_steps, True
                except Exception as e:  # noqa: BLE001
                    row["capture_error"] = repr(e)[:200]
                    torch.cuda.synchronize()
                    sv.set_state(ids, [SEQ_LEN] * batch)
                    graph_on = False

                    def run_n(n, sv=sv):
                        for _ in range(n):
                            sv.step()
                run_n(max(2, args.warmup))
                med, times = timed_blocks(run_n, args.steps, blocks, world, dev,
                                          before_block=lambda sv=sv: sv.set_state(ids, [SEQ_LEN + args.warmup] * batch))
                row.update(tokens_per_s=round(batch * args.steps / med, 2), ms_per_step=round(med / args.steps * 1e3, 4), hipGraph=graph_on,
                           blocks=blocks_summary(times, args.steps), backend_label=c.backend)
                if not overlap:
                    a = allreduce_alone(torch, c, sv, len(model.layers), graph_on, med / args.steps * 1e3, world)
                    row["allreduce_alone"] = {k: a.get(k) for k in ("us_each", "us_per_step", "share_of_step", "error") if k in a}
                del sv
            except Exception as e:  # noqa: BLE001
                row["error"] = repr(e)[:300]
            res.append(row)
    return res


def secondary_workloads(names=("int4_b32_u4kv", "int8_b1", "prefill_2048", "cfg3_rank", "tp8_rank_7b", "cfg5_moe"), steps=10, warmup=3, timeout=150,
                        deadline=None):
    """Each secondary workload in its own process (own model, own allocator).  -> full records (for the detail file).  A child that
    fails, times out, or would start after `deadline` (time.time() value: the run's wall budget) costs only its own entry."""
    import subprocess
    res = []
    for w in names:
        left = None if deadline is None else deadline - time.time()
        if left is not None and left < 25:
            res.append({"workload": w, "skipped": "wall budget of this run spent (DIHIP_BENCH_BUDGET_S)"})
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", w, "--steps", str(steps if w != "prefill_2048" else 3),
               "--warmup", str(warmup if w != "prefill_2048" else 1), "--blocks", "3", "--no-cpu-baseline", "--no-extra", "--full"]
        t0 = time.time()
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout if left is None else max(20, min(timeout, left)), cwd=ROOT)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not line:
                res.append({"workload": w, "error": f"rc {p.returncode}: {(p.stderr or p.stdout)[-400:]}"})
                continue
            d = json.loads(line[-1])
            d["workload"] = w
            d["wall_s"] = round(time.time() - t0, 1)
            res.append(d)
        except Exception as e:  # noqa: BLE001
            res.append({"workload": w, "error": repr(e)[:300]})
    return res


def compact_extra(d):
    """One secondary workload as it rides in the headline line: the numbers, not the tables (those are in the detail file)."""
    if "error" in d or "skipped" in d:
        return {k: d[k] for k in ("workload", "error", "skipped") if k in d}
    c = {"workload": d.get("workload"), "value": d.get("value"), "unit": d.get("unit"), "ms_per_step": d.get("ms_per_step"),
         "step_frac": (d.get("step_hbm") or {}).get("frac_of_peak"), "roofline_frac": (d.get("roofline") or {}).get("frac"),
         "bound": (d.get("roofline") or {}).get("bound")}
    if "attention" in d:
        c["attention_tflops"] = d["attention"].get("tflops")
    return c


def rocprof_kernel_stats(workload, steps=16, warmup=4, timeout=300):
    """`rocprofv3 --kernel-trace --stats` of a short run of THIS bench (same workload, Python runner, nothing extra), collected INSIDE
    the run when rocprofv3 is on PATH, so that roofline.frac comes from the same clock as the summaries under profiles/ (kernel begin
    .. end, no graph-node boundary).  Returns ({kernel name: {"calls", "avg_us"}}, note)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if os.environ.get("DIHIP_BENCH_ROCPROF", "1") == "0":
        return None, "DIHIP_BENCH_ROCPROF=0"
    if not exe:
        return None, "rocprofv3 not on PATH"
    d = tempfile.mkdtemp(prefix="dihip_prof_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "b", "--", sys.executable, os.path.abspath(__file__),
           "--workload", workload, "--steps", str(steps), "--warmup", str(warmup), "--blocks", "2", "--no-cpu-baseline", "--no-extra",
           "--runner", "python", "--full"]
    try:
        env = dict(os.environ, TMPDIR="/tmp", DIHIP_BENCH_ROCPROF="0")
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd="/tmp", env=env)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return None, f"rocprofv3 rc {p.returncode}: {(p.stderr or p.stdout)[-300:]}"
        stats = {}
        for r in csv.DictReader(open(files[0])):
            stats[r["Name"]] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3), "pct": float(r["Percentage"])}
        return stats, "rocprofv3 --kernel-trace --stats of `bench.py --workload %s --steps %d --runner python`, collected inside this run" % (workload, steps)
    except Exception as e:  # noqa: BLE001 -- a profiler hiccup never costs the bench line
        return None, repr(e)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def csrc_tree_hash():
    """sha256 over the kernel sources (dash-infer_amd/csrc/*.hip, *.hpp, *.h, Makefile) in name order: stamps a PMC summary with
    the code it was collected on (tools/gpu_pmc.sh writes it, pmc_traffic() compares)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "dash-infer_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.hpp")) + glob.glob(os.path.join(d, "*.h")) + [os.path.join(d, "Makefile")]):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(kernel_substr, workload="int4_b1"):
    """HBM bytes per launch of a kernel from the newest committed rocprofv3 PMC summary of this workload
    (profiles/*_pmc_hbm_traffic[_<workload>].csv, written by tools/gpu_pmc.sh: FETCH_SIZE doubled per the gfx950 correction + WRITE_SIZE)."""
    import csv
    import glob
    suffix = "" if workload == "int4_b1" else "_" + workload
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_hbm_traffic%s.csv" % suffix)))
    if not files:
        return None, None
    key = kernel_substr.rstrip(">")  # template argument lists may have grown a defaulted tail
    tot = 0
    stamp = None
    for r in csv.DictReader(open(files[-1])):
        stamp = r.get("csrc_hash") or stamp
        if key in r["kernel"]:
            tot += int(r["avg_bytes_corrected"])
    # a summary collected on other kernel sources says nothing about this build: refuse it (VERDICT r2 housekeeping)
    if stamp != csrc_tree_hash():
        return None, "STALE: profiles/%s was collected on kernel sources %s, this tree is %s -- re-run tools/gpu_pmc.sh" % (
            os.path.basename(files[-1]), stamp or "(unstamped)", csrc_tree_hash())
    # not measured by THIS run: counters need their own rocprofv3 passes (tools/gpu_pmc.sh); the summary read here is named
    return (tot or None), "committed PMC summary profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this bench, " \
                          "gfx950 FETCH_SIZE x2 correction); not collected by this run" % os.path.basename(files[-1])


def pmc_traffic_live(workload, timeout=150):
    """HBM bytes per launch of every dihip kernel, collected INSIDE this run when the committed PMC summary is stale or missing:
    two separate rocprofv3 passes (--pmc FETCH_SIZE, --pmc WRITE_SIZE, each with --kernel-trace only -- MI355X_MICROARCH.md, HBM) over a
    short eager run of THIS bench on a truncated layer stack (per-launch traffic does not depend on the layer count; 6 layers + lm_head
    = 1.9 GB, far beyond the 256 MB Infinity Cache); FETCH_SIZE doubled per the guide's gfx950 correction.
    -> ({kernel name: bytes per launch}, note) or (None, why)."""
    import collections
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if os.environ.get("DIHIP_BENCH_PMC", "1") == "0" or os.environ.get("DIHIP_BENCH_ROCPROF", "1") == "0":
        return None, "DIHIP_BENCH_PMC=0"
    if not exe:
        return None, "rocprofv3 not on PATH"
    acc = collections.defaultdict(float)
    d = tempfile.mkdtemp(prefix="dihip_pmc_", dir="/tmp")
    try:
        for ctr, mult in (("FETCH_SIZE", 2), ("WRITE_SIZE", 1)):
            cmd = [exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", os.path.join(d, ctr), "-o", "pmc", "--", sys.executable,
                   os.path.abspath(__file__), "--workload", workload, "--steps", "3", "--warmup", "1", "--blocks", "1", "--layers", "6",
                   "--no-cpu-baseline", "--no-graph", "--runner", "python", "--no-extra", "--full"]
            env = dict(os.environ, TMPDIR="/tmp", DIHIP_BENCH_ROCPROF="0", DIHIP_BENCH_PMC="0")
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd="/tmp", env=env)
            files = glob.glob(os.path.join(d, ctr, "**", "*counter_collection*.csv"), recursive=True)
            if p.returncode != 0 or not files:
                return None, f"rocprofv3 --pmc {ctr} rc {p.returncode}: {(p.stderr or p.stdout)[-200:]}"
            n, v = collections.defaultdict(int), collections.defaultdict(float)
            for r in csv.DictReader(open(files[0])):
                k = r["Kernel_Name"]
                if "dihip" in k and "pack" not in k:
                    n[k] += 1
                    v[k] += float(r["Counter_Value"])
            for k in n:
                acc[k] += v[k] / n[k] * 1024 * mult   # rocprofv3 reports FETCH_SIZE / WRITE_SIZE in KB
        return {k: int(b) for k, b in acc.items()}, ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes collected inside this run "
                                                     "(6-layer stack, eager; FETCH_SIZE x2 gfx950 correction)")
    except Exception as e:  # noqa: BLE001 -- a profiler hiccup never costs the bench line
        return None, repr(e)[:200]
    finally:
        shutil.rmtree(d, ignore_errors=True)


def write_detail(out):
    """The full record (kernel tables, every runner's figures, the secondary workloads' own lines) -> gpurun_out/bench_detail.json
    (gpurun_out/ travels back from a gpurun call); the path, or None when the directory cannot be written."""
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        key = out.get("workload_key") or "other"
        p = os.path.join(d, "bench_detail.json" if key == "int4_b1" and out.get("n_gpus") == 1 else "bench_detail_%s_n%s.json" % (key, out.get("n_gpus")))
        json.dump(out, open(p, "w"), indent=1)
        return os.path.relpath(p, ROOT)
    except OSError:
        return None


def model_tensor(m, name):
    """Host copy of a tensor the C++ operator layer's model owns (hostapi.Model.get_tensor: dtype code, shape, device pointer),
    as float32 rows [-1, last dim]; the copy is exactly the tensor's own size."""
    import ctypes as C
    import numpy as np
    import torch
    dt, shp, p = m.get_tensor(name)
    raw = {1: np.float32, 2: np.float16, 9: np.uint16}[dt]   # f32, f16, bf16 (hostapi.DT)
    a = np.empty(int(np.prod(shp)), dtype=raw)
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    if a.nbytes and hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(p), a.nbytes, 2) != 0:   # 2: hipMemcpyDeviceToHost
        raise RuntimeError(f"hipMemcpy of model tensor {name} failed")
    if dt == 9:
        a = (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32).reshape(-1, shp[-1] if shp else 1)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """--dump-outputs: {name: array} -> d/<name>.npy, float32 (token ids float64, exact).  An array beyond its share of the 64 MB
    budget is written as a fixed, seeded sample of its elements: d/<name>_sample.npy beside d/<name>_sample_index.npy."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(1, len(arrays))
    for name, a in sorted(arrays.items()):
        a = np.asarray(a)
        a = a.astype(np.float64 if a.dtype.kind in "iub" else np.float32)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, (share - 4096) // (a.itemsize + 8), replace=False))   # 4 KB: the .npy headers
            np.save(os.path.join(d, name + "_sample_index.npy"), idx.astype(np.float64))
            a, name = a.reshape(-1)[idx], name + "_sample"
        np.save(os.path.join(d, name + ".npy"), a)


def _short(sv, n):
    sv = str(sv)
    return sv if len(sv) <= n else sv[: n - 3] + "..."


def headline_line(out, detail=None, limit=4096):
    """The line the driver parses: the contract's fields + step_hbm + roofline (the time-dominant kernel) + its runner-up (roofline_gemv or
    roofline_attn_block) + cpu_baseline,
    every string bounded, the secondary workloads as numbers only.  Guaranteed < `limit` bytes: optional parts are dropped, in order,
    until it fits (tests/test_bench_line_contract.py)."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype")
    line = {k: out.get(k) for k in keep}
    line["data"] = _short(out.get("data", "synthetic"), 120)
    cfgd = dict(out.get("config", {}))
    cfgd["workload"] = _short(cfgd.get("workload", ""), 200)
    line["config"] = cfgd
    line["step_hbm"] = out.get("step_hbm")

    def rl(r):
        if not r:
            return None
        c = {k: r.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "avg_kernel_us_rocprof",
                                   "algorithmic_bytes_per_launch", "algorithmic_flops_per_launch", "share_of_step", "frac_graph_events") if k in r}
        c["kernel"] = _short(r.get("kernel", ""), 150)
        c["clock"] = "rocprofv3 kernel-trace avg, collected in this run" if "avg_kernel_us_rocprof" in r else "HIP events around graph-chained launches"
        if r.get("traffic_source"):
            c["traffic_source"] = _short(r["traffic_source"].replace("committed PMC summary ", ""), 60)
        return c

    line["roofline"] = rl(out.get("roofline"))
    # the runner-up of the two kernels a layer's time is spent in, under the name of what it is: `roofline_gemv` (RMSNorm + gate/up + SwiGLU)
    # or `roofline_attn_block` (the fused attention block) -- whichever is NOT the time-dominant one above
    other = out.get("roofline_other") or []
    dom = (out.get("roofline") or {}).get("kernel", "")
    second_key = "roofline_attn_block" if "gate/up" in dom else "roofline_gemv"
    pick = [r for r in other if ("decode_attn_block" in r.get("kernel", "")) == (second_key == "roofline_attn_block") and
            ("gate/up" in r.get("kernel", "") or "decode_attn_block" in r.get("kernel", ""))] or other
    if pick:
        line[second_key] = rl(pick[0])
    cb = out.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                                "sample": _short(cb.get("sample", ""), 260), "library": _short(cb.get("library", ""), 90)}
    for k in ("cpu_baseline_error", "roofline_error", "invalid", "comm_backend", "ar_overlap", "lm_head_split"):
        if out.get(k) not in (None, False):
            line[k] = _short(out[k], 160) if isinstance(out[k], str) else out[k]
    line["runner"] = _short(out.get("runner", ""), 90)
    if isinstance(out.get("host_runner"), dict) and out["host_runner"].get("skipped"):
        line["host_runner_skipped"] = _short(out["host_runner"]["skipped"], 160)
    if out.get("python_runner"):
        line["python_runner_tokens_per_s"] = out["python_runner"].get("tokens_per_s")
    if out.get("blocks"):
        line["blocks"] = {k: out["blocks"].get(k) for k in ("count", "ms_per_step_min", "ms_per_step_max")}
    if out.get("allreduce"):
        line["allreduce"] = {k: out["allreduce"].get(k) for k in ("us_each", "us_per_step", "share_of_step", "error") if k in out["allreduce"]}
    if out.get("tp_ab"):
        line["tp_ab"] = [{k: (_short(r[k], 80) if isinstance(r[k], str) else r[k]) for k in ("allreduce", "overlap", "tokens_per_s", "skipped", "error") if k in r}
                         for r in out["tp_ab"]]
    if out.get("kernels"):
        line["kernels_us"] = {k: v.get("avg_us") for k, v in out["kernels"].items()}
    if out.get("extra"):
        line["extra"] = [compact_extra(w) for w in out["extra"].get("workloads", [])]
        for w in line["extra"]:
            if "error" in w:
                w["error"] = _short(w["error"], 120)
    line["detail"] = detail
    line["wall_s"] = out.get("wall_s")
    for drop in ("kernels_us", "tp_ab", "blocks", "roofline_gemv", "roofline_attn_block", "extra", "python_runner_tokens_per_s", "runner", "allreduce"):
        if len(json.dumps(line)) < limit:
            break
        line.pop(drop, None)
    return line


def fail_line(msg, args, rank=0, rc=2):
    """A run that cannot start says so in ONE JSON line on stdout (rank 0) and a non-zero return code -- never a traceback."""
    if rank == 0:
        print(json.dumps({"error": msg, "metric": None, "value": None, "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup}), flush=True)
    raise SystemExit(rc)


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n, argv, visible, backend_env=None):
    """bench.py --gpus N without a launcher: spawn the N ranks under torch.distributed.run (the driver's own command line:
    --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...) and return its code.  Fewer GPUs than ranks:
    one JSON error line, rc 2 (DIHIP_BENCH_BACKEND=gloo, the CPU test's path, skips the device check)."""
    import subprocess
    if os.environ.get("DIHIP_BENCH_BACKEND", "nccl") != "gloo" and visible < n:
        print(json.dumps({"error": f"needs {n} GPUs, {visible} visible", "metric": None, "value": None, "n_gpus": n}), flush=True)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env, cwd=ROOT).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload", default="int4_b1", choices=list(WORKLOADS) + ["launch_selftest"])  # int4_b1 = the headline configuration
    ap.add_argument("--layers", type=int, default=None, help="debug: fewer decoder layers (result marked invalid)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="debug: eager launches instead of hipGraph replay")
    ap.add_argument("--steps-per-graph", type=int, default=1,
                    help="consecutive decode steps captured per hipGraph (measured: 1 is fastest, back-to-back replays already pipeline)")
    ap.add_argument("--blocks", type=int, default=None,
                    help="timed blocks of --steps steps each; the median block is reported (default: 1 block, 5 with --full)")
    ap.add_argument("--runner", default="auto", choices=["auto", "python", "host"],
                    help="whose step `value` is: the C++ operator layer (host: reference operator list -> fusion pass -> OpFactory -> "
                         "model runner, hipGraph replay) or decoder.DecodeSession (python: the same C-ABI calls from Python).  auto = host "
                         "where it applies (one GPU, dense model), python otherwise; --full puts both figures in the line")
    ap.add_argument("--no-extra", action="store_true", help="with --full: no unfused host-runner figures, no secondary workloads, no TP A/B")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: both runners' figures, the unfused list, per-kernel breakdown and roofline (rocprofv3, "
                         "PMC), CPU baselines, secondary workloads, TP all-reduce share and A/B, the detail file.  Without it a run sets up, "
                         "warms up, times --steps steps of the path `value` comes from and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step (logits, next token ids, ...) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.blocks is None:
        args.blocks = 5 if args.full else 1

    t_main = time.time()
    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` the way the driver runs --gpus 1: this process becomes the launcher of N rank processes
        # (torch.distributed.run, one per GPU, rendezvous on 127.0.0.1) and passes their line and return code through
        raise SystemExit(self_launch(args.gpus, sys.argv[1:], torch.cuda.device_count() if torch.cuda.is_available() else 0))
    if world != args.gpus:
        fail_line(f"WORLD_SIZE {world} != --gpus {args.gpus}", args, rank)
    if args.workload == "launch_selftest":
        # the launch / rendezvous / barrier / max-over-ranks / one-line plumbing alone, on CPU over gloo (tests/test_bench_self_launch.py)
        dist = None
        if world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo", rank=rank, world_size=world)
        med, times = timed_blocks(lambda n: time.sleep(0.002 * n * (1 + rank)), args.steps, 2, world, torch.device("cpu"), sync=lambda: None)
        if rank == 0:
            print(json.dumps({"metric": "launch selftest (no GPU work)", "value": round(args.steps / med, 2), "unit": "steps/s", "n_gpus": world,
                              "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(med / args.steps * 1e3, 4), "comm_backend": "gloo"}), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    if not torch.cuda.is_available() or torch.cuda.device_count() <= local_rank:
        fail_line(f"needs {max(args.gpus, local_rank + 1)} GPUs, {torch.cuda.device_count() if torch.cuda.is_available() else 0} visible", args, rank)
    load_pkg()
    from dash_infer_amd import decoder, ops
    torch.cuda.set_device(local_rank)
    comm = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        # "auto": the one-shot peer-to-peer all-reduce if its guarded set-up + probe pass on every rank, RCCL otherwise (labelled)
        comm = decoder.make_comm(rank, world, torch.device("cuda", local_rank), backend=os.environ.get("DIHIP_TP_ALLREDUCE", "auto"),
                                 allow_labelled_fallback=True)

    wbits, group, kv_mode, batch, gptq = WORKLOADS[args.workload]
    outputs = {}   # --dump-outputs: what the timed path computed in its last step
    if args.workload == "prefill_2048":
        assert world == 1, "prefill_2048 is a one-GPU workload"
        out = prefill_bench(args, torch, decoder, ops, outputs)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, outputs)
        print(json.dumps(out), flush=True)
        return
    if args.workload == "moe_layer":
        assert world == 1, "moe_layer is a one-GPU workload"
        out = moe_layer_bench(args, torch, ops, outputs)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, outputs)
        print(json.dumps(out), flush=True)
        return
    global SEQ_LEN
    SEQ_LEN = SEQ_LEN_OF.get(args.workload, SEQ_LEN)
    cfg = decoder.QWEN2_7B
    model_name = "Qwen2-7B"
    if args.workload == "cfg3_rank":
        assert world == 1, "cfg3_rank times ONE rank's share of the TP = 8 step on one GPU (use --gpus 1)"
        cfg = decoder.ModelConfig("Qwen2-72B/TP8-rank", hidden=8192, layers=80, n_heads=8, n_kv=1, head_dim=128, inter=3712, vocab=19008)
        model_name = "Qwen2-72B (rank-local share of TP=8: all-reduce excluded)"
    if args.workload == "tp8_rank_7b":
        assert world == 1, "tp8_rank_7b times ONE rank's share of the TP = 8 step on one GPU (use --gpus 1)"
        cfg = decoder.ModelConfig("Qwen2-7B/TP8-rank", hidden=3584, layers=28, n_heads=4, n_kv=1, head_dim=128, inter=2432, vocab=19008)
        model_name = "Qwen2-7B (rank-0 share of TP=8: all-reduce excluded)"
    if args.workload == "cfg5_moe":
        cfg, model_name = decoder.QWEN2_57B_A14B, "Qwen2-57B-A14B"
    spec = decoder.QuantSpec(wbits, group, gptq_like_zeros=gptq)
    t_build = time.time()
    # the C++ operator layer is measured beside the Python runner on the one-GPU workloads, the mixture-of-experts one included
    # (its operators re-lay-out the unpacked quantised tensors themselves: keep them)
    host_leg = world == 1 and args.runner != "python"
    if args.runner == "host" and not host_leg:
        raise SystemExit("--runner host: the operator-layer runner covers the one-GPU workloads")
    model = decoder.build_random_model(cfg, spec, seed=1234, rank=rank, nranks=world, layers=args.layers, keep_fp=host_leg)
    blocks = max(1, args.blocks)
    # (kept tight: the decode attention's split width is fixed from max_len; the blocks rewind to SEQ_LEN instead of growing it)
    max_len = SEQ_LEN + args.steps + args.warmup + 16
    sess = decoder.DecodeSession(model, batch, max_len, span_len=128, kv_mode=kv_mode, comm=comm)
    sess.fill_cache_random(SEQ_LEN)
    gen = torch.Generator().manual_seed(7)
    ids = torch.randint(0, cfg.vocab, (batch,), generator=gen)
    sess.set_state(ids, [SEQ_LEN] * batch)
    distinct_experts = sess.count_distinct_experts() if cfg.moe is not None else None
    t_build = time.time() - t_build

    # The one-shot peer-to-peer all-reduce has never run across xGMI on the box it was developed on: before it is timed,
    # two whole decode steps run eagerly with EVERY peer-to-peer sum checked against RCCL's on a copy (same addends, real
    # load, all message sizes of the step).  Any rank seeing a difference beyond summation-order ulps sends ALL ranks to
    # RCCL, and the JSON line says so -- a wrong sum can cost a run its fast path, never its correctness.
    if world > 1 and isinstance(comm, decoder.P2PComm):
        comm.start_verification()
        for _ in range(2):
            sess.step()
        torch.cuda.synchronize()
        ok, summary = comm.finish_verification(torch.device("cuda", local_rank))
        if ok:
            comm.backend = f"{comm.backend} (verified against rccl: {summary})"
        else:
            base = comm.rccl
            base.backend = f"{base.backend} (p2p-oneshot FAILED verification against rccl: {summary})"
            print(f"[rank {rank}] {base.backend}", file=sys.stderr)
            sess.comm = comm = base
        sess.set_state(ids, [SEQ_LEN] * batch)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def run_eager(n):
        for _ in range(n):
            sess.step()

    graph_on = not args.no_graph
    python_outputs = {}

    def time_python_runner():
        """decoder.DecodeSession's step: capture (unless --no-graph), warm-up, timed blocks -> (median block s, block times)"""
        nonlocal graph_on
        run_n = run_eager
        if graph_on:
            try:
                sess.capture(warmup=1, steps_per_graph=max(1, args.steps_per_graph))
                run_n = sess.replay_steps
            except Exception as e:  # noqa: BLE001 -- e.g. a collective that refuses stream capture: measure eager launches
                print(f"[rank {rank}] hipGraph capture failed ({type(e).__name__}: {e}); timing eager launches", file=sys.stderr)
                graph_on = False
                torch.cuda.synchronize()
                sess.set_state(ids, [SEQ_LEN] * batch)
        run_n(args.warmup)
        if settle_steps(args):
            sess.set_state(ids, [SEQ_LEN + args.warmup] * batch)
            run_n(settle_steps(args))
        # exactly K decode steps per block (graphs of --steps-per-graph consecutive steps + single-step graphs), barrier + synchronize
        # on both sides, max over ranks; the median of --blocks blocks is the reported time
        med, times = timed_blocks(run_n, args.steps, blocks, world, torch.device("cuda", local_rank),
                                  before_block=lambda: sess.set_state(ids, [SEQ_LEN + args.warmup] * batch))
        if args.dump_outputs:
            python_outputs.update(logits=sess.logits.float().cpu().numpy(), next_ids=sess.ids.cpu().numpy())
        return med, times

    # A plain run times the path `value` comes from and nothing else: the C++ operator layer where it runs (one GPU; every rank's
    # runner at TP > 1), the Python runner where it does not or fails.  --full times the Python runner first, as the record always had it.
    host_tp_leg = world > 1 and args.runner != "python" and os.environ.get("DIHIP_BENCH_HOST_TP", "1") != "0" and cfg.moe is None
    elapsed = block_times = last_ids = python_runner = None
    if args.full or not (host_leg or host_tp_leg):
        elapsed, block_times = time_python_runner()
        last_ids = sess.ids.tolist()
        python_runner = {"tokens_per_s": round(batch * args.steps / elapsed, 2), "ms_per_step": round(elapsed / args.steps * 1e3, 4)}
    host_runner = None
    host_outputs = {}
    if host_leg:
        try:
            host_runner = {"fused_graph": host_runner_bench(args, torch, decoder, ops, model, sess, batch, max_len, kv_mode, True, True,
                                                            args.steps, blocks, outputs=host_outputs if args.dump_outputs else None)}
            if args.full and not args.no_extra:   # the reference's own operator list, one launch per operator, eager: what fusion + capture buy
                host_runner["unfused_eager"] = host_runner_bench(args, torch, decoder, ops, model, sess, batch, max_len, kv_mode, False,
                                                                 False, max(4, args.steps // 4), min(blocks, 3))
            if python_runner:
                host_runner["fused_graph_vs_python_runner"] = round(host_runner["fused_graph"]["tokens_per_s"] / python_runner["tokens_per_s"], 4)
        except Exception as e:  # noqa: BLE001 -- never lose the headline number to the second runner
            if args.runner == "host":
                raise
            host_runner = {"error": repr(e)}
    if world == 1 and os.environ.get("DIHIP_BENCH_HOST_TP") == "force" and cfg.moe is None:
        # plumbing check on a one-GPU box: the N > 1 leg with a ONE-rank process group and RCCL communicator (the list keeps its AllReduce
        # operators and the K-split tail; nothing is exchanged).  Not a measurement: reported under host_runner_tp_selftest only.
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", local_rank))
        c1 = decoder.RcclComm(0, 1, torch.device("cuda", local_rank))
        selftest = host_runner_bench_tp(args, torch, decoder, ops, cfg, spec, sess, c1, batch, max_len, kv_mode, 0, 1, local_rank, max(4, args.steps // 4), 1)
        dist.destroy_process_group()
        if isinstance(host_runner, dict):
            host_runner["tp_leg_selftest_one_rank"] = selftest
    if host_tp_leg:
        host_runner = host_runner_bench_tp(args, torch, decoder, ops, cfg, spec, sess, comm, batch, max_len, kv_mode, rank, world, local_rank,
                                           args.steps, blocks, outputs=host_outputs if args.dump_outputs else None)
        if "fused_graph" in host_runner and python_runner:
            host_runner["fused_graph_vs_python_runner"] = round(host_runner["fused_graph"]["tokens_per_s"] / python_runner["tokens_per_s"], 4)
    value_from_host = isinstance(host_runner, dict) and "fused_graph" in host_runner and host_runner["fused_graph"].get("fused")
    if value_from_host:
        elapsed = host_runner["fused_graph"]["ms_per_step"] * 1e-3 * args.steps
        block_times = None
        outputs = host_outputs
        last_ids = last_ids or host_runner["fused_graph"].get("last_ids")
    else:
        if python_runner is None:   # plain run, the operator layer gave no figure: the Python runner's is `value`, as in a full run
            elapsed, block_times = time_python_runner()
            last_ids = sess.ids.tolist()
            python_runner = {"tokens_per_s": round(batch * args.steps / elapsed, 2), "ms_per_step": round(elapsed / args.steps * 1e3, 4)}
        outputs = python_outputs

    # share of the step spent in the tensor-parallel all-reduces: the step's collectives alone (2 per layer on the hidden rows,
    # same backend, same message), captured into a graph and replayed between events -- every rank takes part
    ar_info = allreduce_alone(torch, comm, sess, len(model.layers), graph_on, elapsed / args.steps * 1e3, world) if world > 1 and args.full else None
    # one SCALE invocation answers DESIGN section 4's open questions: RCCL vs the one-shot peer-to-peer all-reduce, each with the
    # all-reduce on the compute stream and overlapped on a side stream beside a weight prefetch -- the SAME model, same process
    tp_ab = None
    if world > 1 and args.full and not args.no_extra:
        tp_ab = tp_ab_runs(args, torch, decoder, model, comm, batch, max_len, kv_mode, ids, rank, world, local_rank)

    ms_per_step = elapsed / args.steps * 1e3
    tokens_per_s = batch * args.steps / elapsed
    # whole-step algorithmic bytes: this rank's packed weights + scales/zeros + lm_head + KV read
    step_bytes = sess.algorithmic_bytes_per_step(SEQ_LEN + args.warmup + args.steps // 2)
    step_gbs = step_bytes / (ms_per_step * 1e-3) / 1e9

    out = {
        "metric": f"decode tokens/sec (whole job) + achieved HBM GB/s, {model_name} weight-only quantized decode",
        "value": round(tokens_per_s, 2),
        "unit": "tokens/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": f"synthetic (random-init InstantQuant weights of the {cfg.name} shapes, random {SEQ_LEN}-token KV history)",
        "config": {"workload": f"{model_name} {args.workload}: int{wbits} weight-only group {group}, KV {kv_mode}, batch {batch}, "
                               f"seq {SEQ_LEN}, TP={world}, greedy, hipGraph={'on' if graph_on else 'off'}, "
                               f"{max(1, args.steps_per_graph)} steps per graph",
                   "global_batch": batch, "seq_len": SEQ_LEN, "parallelism": f"tp{world}",
                   "layers": len(model.layers)},
        "step_hbm": {"algorithmic_bytes_per_rank": int(step_bytes), "achieved_GBps_per_gpu": round(step_gbs, 1),
                     "frac_of_peak": round(step_gbs / HBM_PEAK_GBS, 4)},
        "runner": (("host: C++ operator layer -- reference operator list -> fusion pass -> OpFactory(HIP) -> model runner, hipGraph replay"
                    + (f", one runner per rank process (TP={world})" if world > 1 else ""))
                   if value_from_host else "python: decoder.DecodeSession over the C-ABI (hipGraph replay)"),
        "blocks": blocks_summary(block_times, args.steps) if block_times else (host_runner or {}).get("fused_graph", {}).get("blocks"),
        "python_runner": python_runner,
        "host_runner": host_runner,   # host_runner.fused_graph.tokens_per_s = the operator-API figure; .unfused_eager = op by op
        "comm_backend": (comm.backend if comm is not None else None),  # which all-reduce ran: never a silent substitute
        "ar_overlap": bool(getattr(sess, "ar_overlap", False)),        # all-reduce on a side stream + weight prefetch beside it
        "allreduce": ar_info,                                          # TP > 1: time of the step's all-reduces alone and their share
        "tp_ab": tp_ab,                                                # TP > 1: rccl / p2p-oneshot x overlap off / on, same run
        "lm_head_split": getattr(model, "lm_split", "vocab") if world > 1 else None,
        "build_s": round(t_build, 1),
        "workload_key": args.workload,
        "last_ids": (last_ids or [])[:4],
        **({"distinct_routed_experts_per_layer": distinct_experts} if distinct_experts is not None else {}),
    }
    if args.layers is not None:
        out["invalid"] = "debug run with a truncated layer stack"

    if rank == 0 and cfg.moe is not None:
        out["roofline"] = {"bound": "hbm", "kernel": "whole decode step (the routed experts' grouped slot GEMVs dominate: dihip::gemv_stream_kernel<8, 2, 4, 0, *, 0, true>; "
                                                       "their block alone is --workload moe_layer)",
                           "achieved": round(step_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(step_gbs / HBM_PEAK_GBS, 4),
                           "traffic": None, "traffic_source": None,
                           "note": "algorithmic bytes count every DISTINCT routed expert of a layer once per step; the slot kernels stream an "
                                   "expert once per GROUP of up to 4 slots that picked it (once per slot with DIHIP_MOE_GROUP=0)"}
    if rank == 0:
        budget = float(os.environ.get("DIHIP_BENCH_BUDGET_S", "420"))   # wall budget of the whole run; the headline prints regardless
        deadline = t_main + budget
        full = args.full and args.workload == "int4_b1" and world == 1 and not args.no_extra and args.layers is None
        try:
            if cfg.moe is not None or not args.full:
                raise StopIteration  # the per-kernel breakdown below is the dense layer's, and a run of its own (--full)
            kb = kernel_breakdown(sess, torch, ops)
            gpt = 1 if (group > 0 and group == (128 if wbits == 4 else 64)) else 0
            if batch <= 4:
                kname = "gemv_stream_kernel<%d, 2, %d, 1, 1, %d>" % (wbits, 1 if batch == 1 else 4, gpt)
                kdesc = " (RMSNorm + gate/up GEMV + SwiGLU)"
            else:
                # the 7B gate/up pair (>= 24 MB) runs on the K-slice kernel unless DIHIP_GEMM_KSLICE=0 selects the panel kernel
                fam = "gemm_panel_kernel" if os.environ.get("DIHIP_GEMM_KSLICE", "1") == "0" else "gemm_kslice_kernel"
                kname = "%s<%d, 2, %d, 1, %d>" % (fam, wbits, 2 if batch > 16 else 1, gpt)
                kdesc = " (gate/up small-batch GEMM + SwiGLU; the timed launch pair includes the RMSNorm kernel)"
            # the kernels a layer of the step launches, each with its breakdown entry: (profiler name fragment, description, entry)
            cands = [(kname, kdesc, "gate_up_swiglu")]
            if getattr(sess, "attn_block", False) and "attn_block_qkv_attention_o" in kb:
                cands.append(("decode_attn_block_kernel", " (RMSNorm + qkv GEMV + RoPE + KV append + span attention + o GEMV + residual, one launch)",
                              "attn_block_qkv_attention_o"))
            if batch <= 4:
                cands.append(("gemv_stream_kernel<%d, 2, %d, 0, 2, %d>" % (wbits, 1 if batch == 1 else 4, gpt), " (down GEMV + residual)", "down_gemv_addto"))
            stats, note = (rocprof_kernel_stats(args.workload, timeout=max(30, min(240, deadline - time.time() - 60))) if full else (None, None))

            live = [None, None]   # PMC passes inside this run, once, only when the committed summary cannot be used

            def traffic_of(frag):
                if world != 1:
                    return None, None   # PMC passes: TP = 1 shapes
                t, src = pmc_traffic(frag, args.workload)
                if t is None and full and time.time() < deadline - 150:
                    if live[1] is None:
                        live[0], live[1] = pmc_traffic_live(args.workload, timeout=max(30, min(150, (deadline - time.time() - 60) / 2)))
                    hit = [b for k, b in (live[0] or {}).items() if frag.rstrip(">") in k]
                    return (sum(hit) if hit else None), live[1]
                return t, src

            def roof(frag, desc, entry):
                e = kb[entry]
                traffic, traffic_source = traffic_of(frag)
                r = {"bound": "hbm", "kernel": "dihip::" + frag + desc, "achieved": e["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(e["GBps"] / HBM_PEAK_GBS, 4),
                     "clock": "HIP events on the launch stream around hipGraph-chained launches of this kernel over all layers "
                              "(includes the ~1.6 us dependent-launch boundary)",
                     "traffic": traffic, "traffic_source": traffic_source, "avg_launch_us": e["avg_us"], "algorithmic_bytes_per_launch": e["bytes"],
                     "share_of_step": round(e["avg_us"] * len(model.layers) / (ms_per_step * 1e3), 4)}
                hit = [(n, v) for n, v in (stats or {}).items() if frag.rstrip(">") in n]
                if hit:
                    # the same kernel on the profiler's clock (kernel begin .. end), collected inside this run: `achieved` / `frac`
                    # follow from THAT average -- the figure the summaries under profiles/ give; the event-timed one stays beside it
                    calls = sum(v["calls"] for _, v in hit)
                    avg = sum(v["avg_us"] * v["calls"] for _, v in hit) / calls
                    r.update({"achieved_graph_events": r["achieved"], "frac_graph_events": r["frac"], "avg_kernel_us_rocprof": round(avg, 3),
                              "rocprof_calls": calls, "achieved": round(e["bytes"] / (avg * 1e-6) / 1e9, 1),
                              "frac": round(e["bytes"] / (avg * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                              "share_of_step": round(avg * len(model.layers) / (ms_per_step * 1e3), 4),
                              "clock": "rocprofv3 --kernel-trace --stats average of this kernel, collected inside this run (kernel begin .. "
                                       "end); *_graph_events: HIP events around graph-chained launches (includes the ~1.6 us boundary)"})
                return r

            roofs = [roof(*c) for c in cands]
            # `roofline` = the kernel the step spends most of its time in; the others ride along under roofline_other
            roofs.sort(key=lambda r: -(r.get("avg_kernel_us_rocprof") or r["avg_launch_us"]))
            out["roofline"] = roofs[0]
            out["roofline_other"] = roofs[1:]
            if note:
                out["roofline"]["rocprof_note"] = note
            out["kernels"] = kb
            if stats:
                out["rocprof_top_kernels"] = [{"kernel": n[:120], **v} for n, v in sorted(stats.items(), key=lambda kv: -kv[1]["pct"])[:12]]
        except StopIteration:
            pass
        except Exception as e:  # never lose the headline number to the breakdown
            out["roofline_error"] = repr(e)[:300]
        if args.full and world == 1 and not args.no_cpu_baseline and args.workload in ("int4_b1", "int8_b1", "int4_b32_u4kv"):  # the CPU graph below is Qwen2-7B's
            try:
                out["cpu_baseline"] = cpu_baseline_torch(wbits, group, budget_s=12.0)
            except Exception as e:
                out["cpu_baseline_error"] = repr(e)[:300]
            if time.time() < deadline - 90:
                try:  # the same graph with f32 weights (the x86 path's default matmul precision): MKL sgemv, bandwidth bound
                    out["cpu_baseline_f32"] = cpu_baseline_torch(wbits, group, budget_s=8.0, weights="f32")
                except Exception as e:
                    out["cpu_baseline_f32_error"] = repr(e)[:300]
            if time.time() < deadline - 60:
                try:  # second figure: the plain-C oracle loop (the restated CPU_SubC_Ref), linear layers only
                    out["cpu_baseline_port"] = cpu_baseline(wbits, group)
                except Exception as e:
                    out["cpu_baseline_port_error"] = repr(e)[:300]
        # the secondary workloads of the north star (batch 32 + uint4 KV, int8, the context phase, the TP rank shapes, the MoE step):
        # each in its own process; their full records go to the detail file, their numbers ride in the headline line
        if full:
            out["extra"] = {"workloads": secondary_workloads(deadline=deadline)}
        out["wall_s"] = round(time.time() - t_main, 1)
        detail = write_detail(out) if args.full else None
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, outputs)
        print(json.dumps(headline_line(out, detail)), flush=True)   # ONE line, small, LAST: what the driver parses
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
