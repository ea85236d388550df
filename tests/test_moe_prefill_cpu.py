"""The context-phase MoE entry points without a GPU: the workspace sizer's contract and the Python wrappers' signatures."""
import inspect
import itertools


def test_gemm_workspace_sizer(pkg):
    from dash_infer_amd import capi
    lib = capi.lib()
    new, old = lib.dihip_moe_gemm_workspace_bytes, lib.dihip_moe_workspace_bytes
    tokens, experts = (1, 2, 127, 128, 129, 300, 2048, 8200, 32768), (1, 7, 8, 64, 256)
    for k, (hidden, proj) in itertools.product((1, 2, 8), ((128, 128), (256, 384), (3584, 2560))):
        for E in experts:
            prev = 0
            for T in tokens:
                n = int(new(T, k, E, hidden, proj))
                assert n >= int(old(T, k, hidden, proj)) > 0
                assert n >= prev, "monotone in the tokens"
                prev = n
        for T in tokens:
            sizes = [int(new(T, k, E, hidden, proj)) for E in experts]
            assert sizes == sorted(sizes), "monotone in the experts"
    # the tables are small next to the rows: linear in the slot count (sorted_slot + a tile entry per 128 + a counter row per 1024)
    assert int(new(32768, 8, 64, 3584, 2560)) - int(old(32768, 8, 3584, 2560)) < 32768 * 8 * 8
    for bad in ((0, 8, 64, 128, 128), (-1, 8, 64, 128, 128), (4, 0, 64, 128, 128), (4, 8, 0, 128, 128), (4, 8, 64, 0, 128), (4, 8, 64, 128, -5)):
        assert int(new(*bad)) == 0


def test_python_wrappers(pkg):
    from dash_infer_amd import capi, ops
    assert list(inspect.signature(ops.moe_experts_gemm).parameters) == ["x", "experts", "scores", "gate", "up", "down", "ws", "out", "flags"]
    assert list(inspect.signature(ops.moe_experts_gemm).parameters) == list(inspect.signature(ops.moe_experts).parameters)
    assert list(inspect.signature(ops.moe_sort_slots).parameters) == ["experts", "num_experts", "hidden", "proj", "ws"]
    assert ops.MOE_GEMM_MAX_SLOTS >= 32768 * 8
    for name in ("dihip_moe_gemm_workspace_bytes", "dihip_moe_sort_slots", "dihip_moe_experts_gemm"):
        assert name in capi._SIGS and name in capi.header_symbols() and hasattr(capi.lib(), name)
    assert ops.moe_gemm_workspace_bytes(300, 8, 16, 256, 384) == int(capi.lib().dihip_moe_gemm_workspace_bytes(300, 8, 16, 256, 384))
