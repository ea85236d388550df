#!/usr/bin/env python3
"""Mixture-of-experts decode step (route + expert GEMVs + combine) at the Qwen2-57B-A14B shape of BASELINE configs[4]:
64 experts, top-8, hidden 3584, expert width 2560, int8 per-channel weight-only.  Reports us per layer and the
weight bytes streamed per second (each (token, expert) slot reads 3 * hidden * proj bytes + scales).

    python tools/moe_bench.py --prefill [T ...]        (default 128 256 512 2048)

The CONTEXT phase at the same expert shape, int8 per-channel and int4 g128: dihip_moe_experts_gemm (slot sort + grouped MFMA
GEMMs + finalize) against dihip_moe_experts (grouped GEMVs up to 2 048 slots, one GEMV per slot above) on the same inputs, and
for scale the dense SwiGLU + down GEMMs of ONE expert over as many rows as there are slots (the same arithmetic with one weight
set).  Event-timed medians, A/B alternated in one process; TFLOP/s = 6 * slots * hidden * proj / t."""
import statistics
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from __graft_entry__ import _load_pkg
_load_pkg()
from dash_infer_amd import ops


def prefill_bench(Ts):
    E, k, hidden, proj = 64, 8, 3584, 2560
    dt = torch.bfloat16
    REPS, WARM = 9, 2          # the per-slot path takes tens of milliseconds per call at 2 048 tokens

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3   # us

    def one(N, K, wbits, G, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        ng = 1 if G <= 0 else K // G
        if wbits == 8:
            q = torch.randint(-128, 128, (K, N), dtype=torch.int8, device="cuda", generator=g)
        else:
            q = torch.randint(0, 256, (K, N // 2), dtype=torch.uint8, device="cuda", generator=g)
        s = (torch.rand(ng, N, device="cuda", generator=g) * (0.002 if wbits == 8 else 0.03) + 0.007).to(dt)
        z = (torch.rand(ng, N, device="cuda", generator=g) * 4 - 2 + (8 if wbits == 4 else 0)).to(dt)
        return q, s, z

    print(f"{'weights':<10}{'T':>6}{'slots':>7}{'gemm us':>10}{'TFLOP/s':>9}{'gemv us':>11}{'TFLOP/s':>9}{'speed-up':>10}{'dense us':>10}{'TFLOP/s':>9}")
    for wbits, G in ((8, -1), (4, 128)):
        trip = [one(proj, hidden, wbits, G, 1), one(proj, hidden, wbits, G, 2), one(hidden, proj, wbits, G, 3)]
        stacks = [ops.pack_experts([q] * E, [s] * E, [z] * E, G, wbits) for q, s, z in trip]
        dense = [ops.pack_lowp(q, s, z, G, wbits) for q, s, z in trip]
        for T in Ts:
            slots = T * k
            gx = torch.Generator(device="cuda").manual_seed(T)
            x = torch.randn(T, hidden, device="cuda", generator=gx).to(dt)
            logits = torch.randn(T, E, device="cuda", generator=gx).to(dt)
            sc, ex = ops.moe_route(logits, k)
            ws = torch.empty(ops.moe_gemm_workspace_bytes(T, k, E, hidden, proj), dtype=torch.uint8, device="cuda")
            out_a, out_b = torch.empty(T, hidden, dtype=dt, device="cuda"), torch.empty(T, hidden, dtype=dt, device="cuda")
            fa = lambda: ops.moe_experts_gemm(x, ex, sc, *stacks, ws=ws, out=out_a)
            fb = lambda: ops.moe_experts(x, ex, sc, *stacks, ws=ws, out=out_b)
            xs = torch.randn(slots, hidden, device="cuda", generator=gx).to(dt)
            scr = ops.Scratch(max(ops.lowp_workspace_bytes(wbits, slots, proj, hidden, G), ops.lowp_workspace_bytes(wbits, slots, hidden, proj, G)))
            act, yd = torch.empty(slots, proj, dtype=dt, device="cuda"), torch.empty(slots, hidden, dtype=dt, device="cuda")

            def fd():
                ops.prenorm_swiglu(xs, dense[0], dense[1], scr, slots, out=act)
                ops.gemm_lowp(act, dense[2], scratch=scr, out=yd)

            for _ in range(WARM):
                fa(); fb(); fd()
            torch.cuda.synchronize()
            diff = (out_a.float() - out_b.float()).abs().max().item() / max(out_b.float().abs().max().item(), 1e-9)
            ta, tb, td = [], [], []
            for _ in range(REPS):   # alternated: both see the same clocks and the same cache history
                ta.append(timed(fa)); tb.append(timed(fb)); td.append(timed(fd))
            ta, tb, td = statistics.median(ta), statistics.median(tb), statistics.median(td)
            flop = 6.0 * slots * hidden * proj
            name = f"int{wbits} " + ("pc" if G <= 0 else f"g{G}")
            print(f"{name:<10}{T:>6}{slots:>7}{ta:>10.1f}{flop / ta / 1e6:>9.1f}{tb:>11.1f}{flop / tb / 1e6:>9.1f}{tb / ta:>10.2f}{td:>10.1f}"
                  f"{flop / td / 1e6:>9.1f}   (gemm vs gemv outputs: max rel diff {diff:.1e})", flush=True)
        del stacks, dense
        torch.cuda.empty_cache()


if "--prefill" in sys.argv:
    prefill_bench([int(a) for a in sys.argv[1:] if a.isdigit()] or [128, 256, 512, 2048])
    sys.exit(0)

E, k, hidden, proj, wbits = 64, 8, 3584, 2560, 8
layers = 4
dt = torch.bfloat16
def experts(N, K):
    q = torch.randint(-128, 128, (K, N), dtype=torch.int8, device="cuda")
    s = (torch.rand(1, N, device="cuda") * 0.002 + 0.007).to(dt)
    z = (torch.rand(1, N, device="cuda") * 4 - 2).to(dt)
    return ops.pack_experts([q] * E, [s] * E, [z] * E, -1, wbits)
stacks = [(experts(proj, hidden), experts(proj, hidden), experts(hidden, proj)) for _ in range(layers)]
for T in (1, 4, 16, 32):
    x = torch.randn(T, hidden, device="cuda").to(dt)
    logits = torch.randn(T, E, device="cuda").to(dt)
    ws = torch.empty(int(ops.lib().dihip_moe_workspace_bytes(T, k, hidden, proj)), dtype=torch.uint8, device="cuda")
    out = torch.empty(T, hidden, dtype=dt, device="cuda")
    def sweep():
        for g, u, d in stacks:
            sc, ex = ops.moe_route(logits, k)
            ops.moe_experts(x, ex, sc, g, u, d, ws=ws, out=out)
    sweep(); torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        sweep()
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        gr.replay()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (10 * layers)
    byts = T * k * 3 * hidden * proj          # upper bound: every slot a different expert
    print(f"T={T}: {us:.1f} us/layer; {T*k} slots, {byts/1e6:.0f} MB of expert weights -> {byts/us/1e3:.0f} GB/s")
