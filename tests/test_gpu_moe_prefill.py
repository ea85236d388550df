"""GPU tests of the mixture-of-experts CONTEXT phase: the slot sort (dihip_moe_sort_slots) and the grouped expert GEMM
(dihip_moe_experts_gemm) against oracle/moe.py, plus the properties the design promises: tables equal to a stable argsort, a
slot's result independent of the other tokens of the call (bit for bit), slot counts beyond the per-slot path's 65 535, the
DIHIP_MOE_NO_FINALIZE hand-off to dihip_moe_combine, and the refusals.

Shapes: hidden / proj must be multiples of the packed k-tile (int8: 64, int4: 128) as for dihip_moe_experts, so the ragged
case uses hidden 320 / proj 448 (int8): neither a multiple of the 256 / 128 output columns of a workgroup, K = 5 and 7 k-tiles.
"""
import numpy as np
import pytest
import torch

from oracle import moe
from oracle.numerics import bf16_round
from tests.test_gpu_moe import dev, make_experts, pack

pytestmark = pytest.mark.gpu

FORMS = [(8, -1), (8, 128), (4, 128)]


@pytest.fixture(scope="module")
def ops(pkg):
    from dash_infer_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def build_case(ops, wbits, G, T, E, k, hidden, proj, seed, everyone=0, nobody=None):
    rng = np.random.default_rng(seed)
    x = bf16_round(rng.normal(0, 1, (T, hidden)).astype(np.float32))
    gate, up, down = (make_experts(rng, E, proj, hidden, G, wbits), make_experts(rng, E, proj, hidden, G, wbits),
                      make_experts(rng, E, hidden, proj, G, wbits))
    logits = bf16_round(rng.normal(0, 1.5, (T, E)).astype(np.float32))
    if nobody is not None:
        logits[:, nobody] = -30.0
    if everyone is not None:
        logits[:, everyone] = 4.0
    c = dict(wbits=wbits, G=G, T=T, E=E, k=k, hidden=hidden, proj=proj, x=x, gate=gate, up=up, down=down)
    c["pg"], c["pu"], c["pd"] = pack(ops, *gate, G, wbits), pack(ops, *up, G, wbits), pack(ops, *down, G, wbits)
    c["xd"] = dev(x, torch.bfloat16)
    c["scores"], c["experts"] = ops.moe_route(dev(logits, torch.bfloat16), k)
    # the routing is test_gpu_moe.py's subject: the oracle's expert FFN gets the routing the kernels got
    c["s_ref"], c["e_ref"] = c["scores"].cpu().numpy(), c["experts"].cpu().numpy()
    if T <= 300:
        np.testing.assert_array_equal(c["e_ref"], moe.route(logits, k)[1])
    return c


def oracle(c, experts, rows=None):
    rows = slice(None) if rows is None else rows
    return moe.experts_ffn(c["x"][rows], experts[rows], c["s_ref"][rows], list(zip(*c["gate"])), list(zip(*c["up"])),
                           list(zip(*c["down"])), c["G"], c["wbits"])


_cases = {}


@pytest.fixture(params=FORMS, ids=lambda f: f"w{f[0]}g{f[1]}")
def case150(request, ops):
    """T = 150, E = 6, top-3, 256 -> 384 -> 256: expert 0 is picked by every token (150 rows = one full tile + 22), expert 5
    by nobody.  Built once per weight form, with the whole-call output and the oracle's."""
    key = request.param
    if key not in _cases:
        wbits, G = key
        c = build_case(ops, wbits, G, 150, 6, 3, 256, 384, wbits * 10 + (G > 0), everyone=0, nobody=5)
        c["out"] = ops.moe_experts_gemm(c["xd"], c["experts"], c["scores"], c["pg"], c["pu"], c["pd"])
        torch.cuda.synchronize()
        c["ref"] = oracle(c, c["e_ref"])
        _cases[key] = c
    return _cases[key]


def test_sort_tables(ops):
    T, E, k, hidden, proj = 300, 7, 3, 64, 64
    rng = np.random.default_rng(3)
    picks = [0] * 128 + [1] * 129 + [2] * 1            # expert 3: none
    picks += list(rng.integers(4, 7, 2 * T - len(picks)))
    picks = np.array(picks, np.int32)
    rng.shuffle(picks)
    ex = np.full((T, k), -1, np.int32)                  # column 1 is held by another rank throughout
    ex[:, 0], ex[:, 2] = picks[:T], picks[T:]
    flat = ex.reshape(-1)
    valid = np.nonzero(flat >= 0)[0]
    order = valid[np.argsort(flat[valid], kind="stable")]
    offs = np.concatenate([[0], np.cumsum(np.bincount(flat[valid], minlength=E))])
    assert list(np.diff(offs)[:4]) == [128, 129, 1, 0]

    nbytes = ops.moe_gemm_workspace_bytes(T, k, E, hidden, proj)
    base = int(ops.lib().dihip_moe_workspace_bytes(T, k, hidden, proj))
    runs = []
    for _ in range(2):
        ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
        off, srt, tiles, nt = ops.moe_sort_slots(dev(ex), E, hidden, proj, ws=ws)
        torch.cuda.synchronize()
        runs.append(ws.cpu().numpy().copy())
    assert np.array_equal(runs[0], runs[1])                                  # equal bytes, scratch included
    assert np.all(runs[0][:base] == 0xAB)                                    # act / ys / group tables untouched
    off, srt, tiles, nt = off.cpu().numpy(), srt.cpu().numpy(), tiles.cpu().numpy(), int(nt.item())
    np.testing.assert_array_equal(off, offs)
    np.testing.assert_array_equal(srt[:len(order)], order)
    # the tile table: each expert's range cut into tiles of <= 128 rows, in order, nothing shared between experts
    want = [(e, p, min(128, offs[e + 1] - p), 0) for e in range(E) for p in range(offs[e], offs[e + 1], 128)]
    assert nt == len(want) == 1 + 2 + 1 + 0 + sum(-(-int(n) // 128) for n in np.diff(offs)[4:])
    np.testing.assert_array_equal(tiles[:nt], np.array(want, np.int32))
    assert tiles.shape[0] == -(-T * k // 128) + E                            # the host's bound on the grid


def test_matches_oracle(ops, case150):
    c = case150
    ref = c["ref"]
    np.testing.assert_allclose(c["out"].float().cpu().numpy(), ref, rtol=2e-2, atol=2e-2 * np.abs(ref).max())
    assert int((c["e_ref"] == 0).sum()) == 150 and int((c["e_ref"] == 5).sum()) == 0
    # expert parallelism: slots whose expert lives on another rank (-1) contribute nothing
    ex2 = c["experts"].clone()
    ex2[:, 1] = -1
    out2 = ops.moe_experts_gemm(c["xd"], ex2, c["scores"], c["pg"], c["pu"], c["pd"])
    e2 = c["e_ref"].copy()
    e2[:, 1] = -1
    ref2 = oracle(c, e2)
    np.testing.assert_allclose(out2.float().cpu().numpy(), ref2, rtol=2e-2, atol=2e-2 * np.abs(ref2).max())


def test_rows_do_not_depend_on_the_other_tokens(ops, case150):
    """Every token picks expert 0 (once), and expert 0 sorts first, so sorted position p is token p's slot: tokens 127 / 128 end
    the full tile and start the 22-row one, 149 ends it."""
    c = case150
    assert np.all((c["e_ref"] == 0).sum(axis=1) == 1)
    for t in (0, 64, 127, 128, 140, 149):
        one = ops.moe_experts_gemm(c["xd"][t:t + 1].contiguous(), c["experts"][t:t + 1].contiguous(), c["scores"][t:t + 1].contiguous(),
                                   c["pg"], c["pu"], c["pd"])
        assert torch.equal(one[0], c["out"][t]), f"token {t}: max diff {(one[0].float() - c['out'][t].float()).abs().max()}"
    perm = torch.from_numpy(np.random.default_rng(1).permutation(c["T"])).cuda()
    outp = ops.moe_experts_gemm(c["xd"][perm].contiguous(), c["experts"][perm].contiguous(), c["scores"][perm].contiguous(),
                                c["pg"], c["pu"], c["pd"])
    assert torch.equal(outp, c["out"][perm])
    assert torch.equal(c["out"], ops.moe_experts_gemm(c["xd"], c["experts"], c["scores"], c["pg"], c["pu"], c["pd"]))


def test_no_finalize_then_combine_is_bit_identical(ops, case150):
    c = case150
    T, hidden, proj, k, E = c["T"], c["hidden"], c["proj"], c["k"], c["E"]
    rng = np.random.default_rng(5)
    shared = dev(bf16_round(rng.normal(0, 1, (T, hidden)).astype(np.float32)), torch.bfloat16)
    sig = dev(bf16_round(rng.uniform(0, 1, (T, 1)).astype(np.float32)), torch.bfloat16)
    h = dev(rng.normal(0, 1, (T, hidden)).astype(np.float32), torch.float32)
    for with_res in (True, False):
        ref = torch.empty_like(h)
        ops.moe_shared_combine(ref, h if with_res else None, c["out"], shared, sig)
        ws = torch.full((ops.moe_gemm_workspace_bytes(T, k, E, hidden, proj),), 0xAB, dtype=torch.uint8, device="cuda")
        assert ops.moe_experts_gemm(c["xd"], c["experts"], c["scores"], c["pg"], c["pu"], c["pd"], ws=ws, flags=ops.MOE_NO_FINALIZE) is None
        got = torch.empty_like(h)
        ops.moe_combine(got, h if with_res else None, ws, c["scores"], c["experts"], shared, sig, proj)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), f"residual={with_res}: max diff {(got - ref).abs().max()}"


def test_ragged_n_and_k(ops):
    c = build_case(ops, 8, -1, 140, 5, 2, 320, 448, 11, everyone=1)
    out = ops.moe_experts_gemm(c["xd"], c["experts"], c["scores"], c["pg"], c["pu"], c["pd"])
    ref = oracle(c, c["e_ref"])
    np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=2e-2, atol=2e-2 * np.abs(ref).max())


def test_beyond_the_per_slot_limit(ops):
    """65 600 slots: dihip_moe_experts refuses (the slot is gridDim.y); the grouped GEMM serves them, deterministically, and --
    rows being independent -- equals the same call on the two halves of the tokens."""
    T, E, k, hidden, proj = 8200, 8, 8, 128, 128
    c = build_case(ops, 8, -1, T, E, k, hidden, proj, 21, everyone=None)
    with pytest.raises(Exception):
        ops.moe_experts(c["xd"], c["experts"], c["scores"], c["pg"], c["pu"], c["pd"])
    run = lambda lo, hi: ops.moe_experts_gemm(c["xd"][lo:hi].contiguous(), c["experts"][lo:hi].contiguous(), c["scores"][lo:hi].contiguous(),
                                              c["pg"], c["pu"], c["pd"])
    out = run(0, T)
    assert torch.equal(out, run(0, T))
    assert torch.equal(out, torch.cat([run(0, T // 2), run(T // 2, T)]))
    rows = np.sort(np.random.default_rng(2).choice(T, 16, replace=False))
    ref = oracle(c, c["e_ref"], rows)
    np.testing.assert_allclose(out[torch.from_numpy(rows).cuda()].float().cpu().numpy(), ref, rtol=2e-2, atol=2e-2 * np.abs(ref).max())


def test_refusals_launch_nothing(ops):
    from dash_infer_amd import capi
    T, E, k, hidden, proj = 4, 4, 2, 128, 128
    c = build_case(ops, 8, -1, T, E, k, hidden, proj, 31, everyone=None)
    need = ops.moe_gemm_workspace_bytes(T, k, E, hidden, proj)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full((T, hidden), 7.0, dtype=torch.bfloat16, device="cuda")
    p, s = ops.ptr, ops.cur_stream()

    def call(wbits=8, x=c["xd"], tokens=T, ws_bytes=need, experts=c["experts"]):
        return ops.lib().dihip_moe_experts_gemm(s, wbits, p(x), p(experts), p(c["scores"]), p(c["pg"].w), p(c["pg"].sz), p(c["pu"].w),
                                                p(c["pu"].sz), p(c["pd"].w), p(c["pd"].sz), tokens, k, E, hidden, proj, -1, p(out), p(ws),
                                                ws_bytes, ops.dt_code(c["xd"]), 0)

    assert call(wbits=3) == capi.PARAM_ERROR
    assert call(x=None) == capi.PARAM_ERROR
    assert call(ws_bytes=need - 1) == capi.MEMORY_ERROR
    assert call(tokens=ops.MOE_GEMM_MAX_SLOTS // k + 1) == capi.EXCEED_LIMIT_ERROR
    sort = lambda tokens, ws_bytes, ex=c["experts"]: ops.lib().dihip_moe_sort_slots(s, p(ex), tokens, k, E, hidden, proj, p(ws), ws_bytes)
    assert sort(T, need - 1) == capi.MEMORY_ERROR
    assert sort(T, need, None) == capi.PARAM_ERROR
    assert sort(ops.MOE_GEMM_MAX_SLOTS // k + 1, need) == capi.EXCEED_LIMIT_ERROR
    torch.cuda.synchronize()
    assert bool((ws == 0xAB).all()) and bool((out == 7.0).all())
    assert call() == capi.SUCCESS
    torch.cuda.synchronize()
    assert not bool((out == 7.0).all())
