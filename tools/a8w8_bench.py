#!/usr/bin/env python3
"""Context-phase GEMMs of Qwen2-7B, int8 per-channel weights: A16W8 (gemm_prefill_kernel) against A8W8 (activation quantiser +
gemm_a8w8_kernel, both launches timed), same packed weights, A/B alternated in one process.

    python tools/a8w8_bench.py [M ...]        (default 2048 512)

Per shape: event-timed after warm-up, REPS repetitions each, median; TOP/s = 2 M N K / t (the SwiGLU pair counts both
matrices); ratio = t_A16W8 / t_A8W8 (> 1: A8W8 faster)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from __graft_entry__ import _load_pkg
_load_pkg()
from dash_infer_amd import ops

REPS, WARM = 30, 5
HID, INTER, QKV = 3584, 18944, 4608


def packed(N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    wq = torch.randint(-128, 128, (K, N), dtype=torch.int8, device="cuda", generator=g)
    s = (torch.rand(1, N, device="cuda", generator=g) * 0.002 + 0.007).to(torch.bfloat16)
    z = (torch.rand(1, N, device="cuda", generator=g) * 20 - 10).to(torch.bfloat16)
    return ops.pack_lowp(wq, s, z, -1, 8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3   # us


def ab(fa, fb):
    for _ in range(WARM):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):   # alternated: both see the same clocks and the same cache history
        ta.append(timed(fa))
        tb.append(timed(fb))
    return statistics.median(ta), statistics.median(tb)


def main():
    Ms = [int(a) for a in sys.argv[1:]] or [2048, 512]
    w_qkv, w_o, w_gate, w_up, w_down = packed(QKV, HID, 1), packed(HID, HID, 2), packed(INTER, HID, 3), packed(INTER, HID, 4), packed(HID, INTER, 5)
    print(f"{'shape':<34}{'M':>6}{'A16W8 us':>11}{'TOP/s':>8}{'A8W8 us':>10}{'TOP/s':>8}{'ratio':>7}")
    for M in Ms:
        x = torch.randn(M, HID, device="cuda").to(torch.bfloat16)
        xi = torch.randn(M, INTER, device="cuda").to(torch.bfloat16)
        h = torch.randn(M, HID, device="cuda")
        bias = torch.randn(QKV, device="cuda").to(torch.bfloat16)
        gamma = torch.ones(HID, device="cuda").to(torch.bfloat16)
        sc = ops.Scratch(max(ops.lowp_workspace_bytes(8, M, INTER, HID, -1), ops.lowp_workspace_bytes(8, M, HID, INTER, -1)))
        ws = torch.empty(max(ops.a8w8_workspace_bytes(M, INTER, HID), ops.a8w8_workspace_bytes(M, HID, INTER)), dtype=torch.uint8, device="cuda")
        y_qkv = torch.empty(M, QKV, dtype=torch.bfloat16, device="cuda")
        y_act = torch.empty(M, INTER, dtype=torch.bfloat16, device="cuda")
        h_out = torch.empty(M, HID, device="cuda")
        cases = [
            (f"qkv  N {QKV} K {HID} bias", 2.0 * M * QKV * HID,
             lambda: ops.gemm_lowp(x, w_qkv, bias=bias, scratch=sc, out=y_qkv),
             lambda: ops.gemm_a8w8(x, w_qkv, bias=bias, ws=ws, out=y_qkv)),
            (f"o    N {HID} K {HID} addto", 2.0 * M * HID * HID,
             lambda: ops.fused_gemm_addto(x, w_o, h, sc, out=h_out),
             lambda: ops.a8w8_gemm_addto(x, w_o, h, ws=ws, out=h_out)),
            (f"gate/up N {INTER} x2 K {HID} norm+swiglu", 4.0 * M * INTER * HID,
             lambda: ops.fused_norm_swiglu(h, gamma, 1e-6, w_gate, w_up, sc, out=y_act),
             lambda: ops.a8w8_norm_swiglu(h, gamma, 1e-6, w_gate, w_up, ws=ws, out=y_act)),
            (f"down N {HID} K {INTER} addto", 2.0 * M * HID * INTER,
             lambda: ops.fused_gemm_addto(xi, w_down, h, sc, out=h_out),
             lambda: ops.a8w8_gemm_addto(xi, w_down, h, ws=ws, out=h_out)),
        ]
        for name, flop, fa, fb in cases:
            ta, tb = ab(fa, fb)
            print(f"{name:<34}{M:>6}{ta:>11.1f}{flop / ta / 1e6:>8.0f}{tb:>10.1f}{flop / tb / 1e6:>8.0f}{ta / tb:>7.2f}", flush=True)


if __name__ == "__main__":
    main()
