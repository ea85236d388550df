"""Generator of tests/golden/lowp_plans.json: the host-side plans of the weight-only GEMM on a 256-CU device, as the library
answers them WITHOUT a GPU (tests/test_lowp_plans_cpu.py asserts them row for row).

  queries  inputs -> outputs of the shape-only exports (workspace sizes, dihip_gemm_lowp_prefers_frag,
           dihip_prenorm_rowsq_supported, dihip_gemm_prefill_tail_parts, dihip_debug_gemv_plan, packed sizes).  These were
           generated with the library of the commit BEFORE the route refactor and are kept as they are:
               python tests/golden/make_lowp_plan_golden.py --queries-only      (DIHIP_LIB_DIR = that build)
  routes   call description -> dihip_debug_gemm_route.  `form` names the entry point and layouts the row stands for;
           tools/gemm_route_sweep.py issues exactly these calls on the GPU.  Regenerate (queries are kept) with
               python tests/golden/make_lowp_plan_golden.py

The rows: every form and every batch of {1, 4, 5, 16, 17, 32, 33, 64, 2048} -- both sides of each band edge -- on the
Qwen2-7B int4 g128 bf16 layers; one batch per band on the other shapes / quantisations / dtypes; then, greedily, whatever
reaches a launch-thunk specialisation of the dispatcher (dispatcher_specs() mirrors its tables) that no earlier row reached.
The specialisations left are listed in two sections: `unreachable` -- no call of the generator's pool is routed there (a
finding: an instantiation nobody launches), with the reason -- and `over_budget` -- reachable, with a call that reaches it, but
left out by the 400-row budget.  The greedy pass alternates bf16 and f16 so that the budget is spent on both."""
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "lowp_plans.json")
SWITCHES = ("DIHIP_GEMV_STREAM", "DIHIP_GEMM_KSLICE", "DIHIP_GEMM_PANEL", "DIHIP_GEMM_PREFILL", "DIHIP_PREFILL_TAIL_SPLIT",
            "DIHIP_DEFER_RMSNORM")
F16, BF16 = 1, 2
PLAIN, RMSNORM = 0, 1
STD, SWIGLU, ADDTO = 0, 1, 2
ROW, FRAG = 0, 1
ROWSQ, NORM, PRENORM, NO_WS, NO_SYNC, UNALIGNED = 1, 2, 4, 8, 16, 32
ROUTE_FIELDS = 16
FAMILIES = ("none", "gemv_stream", "gemm_kslice", "gemm_panel", "gemv_batch", "gemm_prefill", "gemm_lowp")
BATCHES = (1, 4, 5, 16, 17, 32, 33, 64, 2048)
BANDS = (1, 16, 33, 2048)                 # one batch per band: decode GEMV, small batch, general, context phase
QUANTS = ((4, 128), (4, 256), (4, -1), (8, -1), (8, 64), (8, 128))

# (name, N, K, role): role picks the forms a layer is called with
Q7B = (("qkv", 4608, 3584, "gemm"), ("o", 3584, 3584, "addto"), ("gate_up", 18944, 3584, "swiglu"), ("down", 3584, 18944, "addto"))
OTHER = (("72b_qkv", 1280, 8192, "gemm"), ("72b_o", 8192, 1024, "addto"), ("72b_gate_up", 3712, 8192, "swiglu"),
         ("72b_down", 8192, 3712, "addto"), ("7b8_qkv", 768, 3584, "gemm"), ("7b8_o", 3584, 512, "addto"),
         ("7b8_gate_up", 2432, 3584, "swiglu"), ("7b8_down", 3584, 2432, "addto"))
DENSE = (("lm_head", 152064, 3584), ("72b_lm_head", 19008, 8192), ("router", 64, 3584))
UNALIGNED_SHAPES = ((4, 50, 200, 64), (8, 50, 200, 64), (4, 33, 130, 32), (8, 33, 130, 32))   # test_pack_kernels_byte_exact
TAIL_SHAPES = ((4, 2048, 4608, 3584, 128, 0), (4, 2048, 18944, 3584, 128, 1), (4, 2048, 3584, 3584, 128, 0),
               (4, 2048, 3584, 18944, 128, 0), (4, 2048, 4096, 3584, 128, 0), (4, 2048, 6400, 3584, 128, 0),
               (4, 512, 4608, 3584, 128, 0), (4, 32, 4608, 3584, 128, 0), (4, 2048, 4608, 1024, 256, 0),
               (8, 2048, 4608, 512, -1, 0))                                                   # test_small_batch_plans_cpu.py


def load_lib():
    path = os.path.join(os.environ.get("DIHIP_LIB_DIR") or os.path.join(ROOT, "dash-infer_amd", "lib"), "libdashinfer_hip.so")
    try:
        import torch  # noqa: F401  its HIP runtime must be the process's (dash-infer_amd/capi.py)
    except ImportError:
        pass
    l = C.CDLL(path)
    i, z = C.c_int, C.c_size_t
    for name, res, args in (("dihip_gemm_lowp_workspace_bytes", z, [i] * 5), ("dihip_dense_workspace_bytes", z, [i] * 3),
                            ("dihip_gemm_lowp_prefers_frag", i, [i] * 6), ("dihip_prenorm_rowsq_supported", i, [i] * 8),
                            ("dihip_gemm_prefill_tail_parts", i, [i] * 6),
                            ("dihip_debug_gemv_plan", i, [i] * 6 + [C.POINTER(i)] * 4 + [C.POINTER(z)]),
                            ("dihip_gemm_lowp_packed_weight_bytes", z, [i] * 3), ("dihip_gemm_lowp_packed_sz_bytes", z, [i] * 3),
                            ("dihip_dense_packed_weight_bytes", z, [i] * 2),
                            ("dihip_debug_gemm_route", i, [i] * 11 + [C.POINTER(C.c_longlong)])):
        if hasattr(l, name):
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
    return l


def gemv_plan(lib, wbits, M, N, K, g, dual):
    b, u, wk, wn, lds = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    st = lib.dihip_debug_gemv_plan(wbits, M, N, K, g, dual, C.byref(b), C.byref(u), C.byref(wk), C.byref(wn), C.byref(lds))
    return [st] if st else [st, b.value, u.value, wk.value, wn.value, lds.value]


def query(lib, wbits, M, N, K, g):
    """Everything the shape-only exports say about one (wbits, M, N, K, group)."""
    if wbits == 16:
        return {"in": [wbits, M, N, K, g], "workspace": lib.dihip_dense_workspace_bytes(M, N, K),
                "lowp_workspace": lib.dihip_gemm_lowp_workspace_bytes(16, M, N, K, g),
                "prefers_frag": [lib.dihip_gemm_lowp_prefers_frag(16, M, N, K, g, 0)],
                "gemv_plan": [gemv_plan(lib, 16, M, N, K, g, 0)], "packed": [lib.dihip_dense_packed_weight_bytes(N, K)]}
    return {"in": [wbits, M, N, K, g], "workspace": lib.dihip_gemm_lowp_workspace_bytes(wbits, M, N, K, g),
            "prefers_frag": [lib.dihip_gemm_lowp_prefers_frag(wbits, M, N, K, g, d) for d in (0, 1)],
            # (dual, dtype, x_layout) in itertools.product order
            "rowsq": [lib.dihip_prenorm_rowsq_supported(wbits, M, N, K, g, d, dt, lay)
                      for d, dt, lay in itertools.product((0, 1), (BF16, F16), (ROW, FRAG))],
            "tail_parts": [lib.dihip_gemm_prefill_tail_parts(wbits, M, N, K, g, d) for d in (0, 1)],
            "gemv_plan": [gemv_plan(lib, wbits, M, N, K, g, d) for d in (0, 1)],
            "packed": [lib.dihip_gemm_lowp_packed_weight_bytes(wbits, N, K), lib.dihip_gemm_lowp_packed_sz_bytes(N, K, g)]}


def query_inputs():
    rows = [(4, M, N, K, 128) for _, N, K, _ in Q7B for M in BATCHES]
    rows += [(w, M, N, K, g) for (w, g) in QUANTS[1:] for _, N, K, _ in (Q7B[0], Q7B[3]) for M in (5, 2048)]
    rows += [(4, M, N, K, 128) for _, N, K, _ in OTHER for M in (5, 2048)]
    rows += [(16, M, N, K, -1) for _, N, K in DENSE for M in (1, 32)]
    rows += [(w, 16, N, K, g) for (w, N, K, g) in UNALIGNED_SHAPES]
    rows += [(w, M, N, K, g) for (w, M, N, K, g, _) in TAIL_SHAPES]
    return list(dict.fromkeys(rows))


# ---- routes ---------------------------------------------------------------------------------------------------------------
def route(lib, wbits, dtype, pro, epi, M, N, K, g, xl, yl, flags):
    out = (C.c_longlong * ROUTE_FIELDS)()
    st = lib.dihip_debug_gemm_route(wbits, dtype, pro, epi, M, N, K, g, xl, yl, flags, out)
    assert st == 0, (st, wbits, dtype, pro, epi, M, N, K, g, xl, yl, flags)
    return list(out)


def form_desc(lib, form, wbits, M, N, K, g):
    """(pro, epi, x_layout, y_layout, flags) of the GemmCall an entry point builds, or None when the form does not apply."""
    small = 4 < M <= 32
    dual = form.startswith(("norm_swiglu", "prenorm_swiglu"))
    pf = FRAG if lib.dihip_gemm_lowp_prefers_frag(wbits, M, N, K, g, 1 if dual else 0) else ROW   # layout of the call's own norm rows
    lay = {"row": ROW, "frag": FRAG}
    name, _, tail = form.partition(":")
    opts = tail.split(",") if tail else []
    if any(o == "frag" for o in opts) and not small:
        return None
    if wbits == 16:
        if name == "a16w16":
            return PLAIN, STD, ROW, ROW, 0
        if name == "lm_head":
            return (RMSNORM, ADDTO, ROW, ROW, 0) if M <= 4 else (PLAIN, ADDTO, pf, ROW, 0)
        return None
    if name == "std":
        return PLAIN, STD, ROW, ROW, (NO_SYNC if "nosync" in opts else 0)
    if name == "norm_gemm":
        return (RMSNORM, STD, ROW, ROW, 0) if M <= 4 else (PLAIN, STD, pf, ROW, 0)
    if name == "norm_swiglu":       # opts: y layout
        yl = lay[opts[0]]
        return (RMSNORM, SWIGLU, ROW, ROW, 0) if M <= 4 else (PLAIN, SWIGLU, FRAG if yl == FRAG else pf, yl, 0)
    if name in ("addto", "addto_norm", "addto_prenorm"):   # opts: x layout
        return PLAIN, ADDTO, lay[opts[0]], ROW, {"addto": 0, "addto_norm": NORM, "addto_prenorm": PRENORM}[name]
    if name in ("prenorm_gemm", "prenorm_gemm_rowsq"):     # opts: x layout
        return PLAIN, STD, lay[opts[0]], ROW, (ROWSQ if name.endswith("rowsq") else 0)
    if name in ("prenorm_swiglu", "prenorm_swiglu_rowsq"):  # opts: x layout, y layout
        return PLAIN, SWIGLU, lay[opts[0]], lay[opts[1]], (ROWSQ if name.endswith("rowsq") else 0)
    return None


FORMS = {
    "gemm": ("std", "norm_gemm", "prenorm_gemm:row", "prenorm_gemm:frag", "prenorm_gemm_rowsq:row", "prenorm_gemm_rowsq:frag"),
    "swiglu": ("std", "norm_swiglu:row", "norm_swiglu:frag", "prenorm_swiglu:row,row", "prenorm_swiglu:frag,row",
               "prenorm_swiglu:frag,frag", "prenorm_swiglu_rowsq:frag,row", "prenorm_swiglu_rowsq:frag,frag"),
    "addto": ("std", "addto:row", "addto:frag", "addto_norm:row", "addto_norm:frag", "addto_prenorm:row", "addto_prenorm:frag"),
    "dense": ("a16w16", "lm_head"),
}
ALL_FORMS = tuple(dict.fromkeys(f for fs in FORMS.values() for f in fs))


def make_row(lib, form, wbits, dtype, M, N, K, g):
    d = form_desc(lib, form, wbits, M, N, K, g)
    if d is None:
        return None
    pro, epi, xl, yl, flags = d
    r = route(lib, wbits, dtype, pro, epi, M, N, K, g, xl, yl, flags)
    if r[15] != 0:       # the entry point refuses the call (deferred norms on a kernel that has none, ...): not a launch
        return None
    return [form, wbits, dtype, M, N, K, g, pro, epi, xl, yl, flags, r]


def spec_of(row):
    """The launch-thunk specialisation a row reaches: (family, wbits, dtype, MT|MR, NT, PRO, EPI, GPT, RS)."""
    wbits, dtype, r = row[1], row[2], row[12]
    fam = FAMILIES[r[0]]
    mt, nt, pro, epi, gpt, rs = r[1:7]
    if fam == "gemv_stream":
        return fam, wbits, dtype, mt, 0, pro, epi, gpt, 0
    if fam == "gemm_kslice":
        return fam, wbits, dtype, mt, 0, 0, epi, gpt, rs
    if fam == "gemm_panel":
        return fam, wbits, dtype, mt, 0, 0, epi, gpt, 0
    if fam == "gemv_batch":
        return fam, wbits, dtype, mt, nt, 0, epi, gpt, 0
    if fam == "gemm_prefill":
        return fam, wbits, dtype, 0, 0, 0, epi, gpt, 0
    return fam, wbits, dtype, mt, nt, pro, epi, 0, 0


def dispatcher_specs():
    """Every specialisation the thunk tables of csrc/gemm_lowp.hip name."""
    s = set()
    fts = (BF16, F16)
    for ft in fts:
        for w, gp in ((4, 0), (4, 1), (8, 0), (8, 1), (16, 0)):
            for mr in (1, 4):
                for pro, epi in ((PLAIN, STD), (RMSNORM, STD), (RMSNORM, SWIGLU), (PLAIN, SWIGLU), (PLAIN, ADDTO), (RMSNORM, ADDTO)):
                    s.add(("gemv_stream", w, ft, mr, 0, pro, epi, gp, 0))
        for w, gp in ((4, 0), (4, 1), (8, 0)):
            for mt in (1, 2):
                for epi in (STD, SWIGLU, ADDTO):
                    s.add(("gemm_kslice", w, ft, mt, 0, 0, epi, gp, 0))
        for w, gp in ((4, 0), (4, 1), (8, 0), (8, 1)):
            for mt in (1, 2):
                for epi in (STD, SWIGLU, ADDTO):
                    s.add(("gemm_panel", w, ft, mt, 0, 0, epi, gp, 0))
                    for nt in (1, 2):
                        s.add(("gemv_batch", w, ft, mt, nt, 0, epi, gp, 0))
        for w in (4, 8):
            for epi in (STD, SWIGLU, ADDTO):
                for gp in (0, 1):
                    s.add(("gemm_prefill", w, ft, 0, 0, 0, epi, gp, 0))
            for mt, nt, pro, epi in ((1, 2, PLAIN, STD), (1, 4, PLAIN, STD), (2, 2, PLAIN, STD), (2, 4, PLAIN, STD),
                                     (1, 2, RMSNORM, STD), (1, 4, RMSNORM, STD), (1, 4, RMSNORM, SWIGLU), (1, 4, PLAIN, SWIGLU),
                                     (2, 4, PLAIN, SWIGLU), (1, 2, PLAIN, ADDTO), (1, 4, PLAIN, ADDTO), (2, 2, PLAIN, ADDTO),
                                     (2, 4, PLAIN, ADDTO)):
                s.add(("gemm_lowp", w, ft, mt, nt, pro, epi, 0, 0))
        for mt, pro, epi in ((1, RMSNORM, ADDTO), (1, PLAIN, ADDTO), (2, PLAIN, ADDTO), (1, PLAIN, STD), (2, PLAIN, STD)):
            s.add(("gemm_lowp", 16, ft, mt, 4, pro, epi, 0, 0))
    for w, gp in ((4, 0), (4, 1), (8, 0)):     # the deferred-row-norm consumer of the K-slice kernel: bf16
        for mt in (1, 2):
            for epi in (STD, SWIGLU):
                s.add(("gemm_kslice", w, BF16, mt, 0, 0, epi, gp, 1))
    return s


def route_rows(lib, budget):
    rows, seen = [], set()

    def add(row):
        if row is not None and tuple(row[:12]) not in seen:
            seen.add(tuple(row[:12]))
            rows.append(row)

    # 1. every batch and every form on the Qwen2-7B int4 g128 bf16 layers
    for _, N, K, role in Q7B:
        for M in BATCHES:
            for form in FORMS[role]:
                add(make_row(lib, form, 4, BF16, M, N, K, 128))
    # 2. one batch per band: the other quantisations and f16 on the 7B layers, the TP ranks, the unquantised matrices, the
    #    shapes that fit no tile, the tail-split shapes
    natural = {"gemm": "norm_gemm", "swiglu": "norm_swiglu:row", "addto": "addto:row"}
    for (w, g), dt in itertools.product(QUANTS, (BF16, F16)):
        if (w, g, dt) != (4, 128, BF16):
            for (_, N, K, role), M in zip(itertools.cycle(Q7B), BANDS):
                add(make_row(lib, natural[role], w, dt, M, N, K, g))
    for (_, N, K, role), M in zip(OTHER, itertools.cycle(BANDS)):
        add(make_row(lib, natural[role], 4, BF16, M, N, K, 128))
    for name, N, K in DENSE:
        for M in (1, 4, 16, 33):
            add(make_row(lib, "a16w16" if name == "router" else "lm_head", 16, BF16, M, N, K, -1))
    for w, N, K, g in UNALIGNED_SHAPES:
        for M in (1, 64) if w == 4 else (16,):
            add(make_row(lib, "std", w, BF16, M, N, K, g))
    for w, M, N, K, g, dual in TAIL_SHAPES:
        add(make_row(lib, "prenorm_swiglu:row,row" if dual else "std", w, BF16, M, N, K, g))
    add(make_row(lib, "std:nosync", 4, BF16, 33, 4608, 3584, 128))   # sync == NULL: the counters follow the slab
    # 3. greedily: candidates that reach a specialisation nobody reached yet
    want = dispatcher_specs()
    covered = {spec_of(r) for r in rows}
    shapes = [(N, K) for _, N, K, _ in Q7B + OTHER] + [(4608, 1024), (4608, 512)]
    unal = [(N, K) for _, N, K, _ in UNALIGNED_SHAPES]
    cands = itertools.chain(
        ((f, w, dt, M, N, K, g) for (w, g) in QUANTS + ((4, 64), (8, 32)) for M in BATCHES for (N, K) in shapes + unal
         for f in ALL_FORMS if f not in FORMS["dense"] for dt in (BF16, F16)),
        ((f, 16, dt, M, N, K, -1) for M in BATCHES for _, N, K in DENSE for f in FORMS["dense"] for dt in (BF16, F16)))
    for f, w, dt, M, N, K, g in cands:
        if len(rows) >= budget or want <= covered:
            break
        row = make_row(lib, f, w, dt, M, N, K, g)
        if row is not None and spec_of(row) in want and spec_of(row) not in covered:
            covered.add(spec_of(row))
            add(row)
    stray = sorted({spec_of(r) for r in rows} - want)
    assert not stray, f"rows reach specialisations the dispatcher tables do not name: {stray}"
    return rows, sorted(want - covered)


def why_unreachable(spec):
    fam, w, ft, mt, nt, pro, epi, gpt, rs = spec
    if fam == "gemv_stream" and w != 16 and (pro, epi) == (RMSNORM, ADDTO):
        return "no entry point: a quantised GEMM with the RMSNorm prologue and the f32 add-to epilogue is not exposed"
    if fam == "gemv_stream" and w == 16:
        return "no entry point: unquantised weights are called as dihip_gemm_a16w16 (plain, std) and dihip_lm_head (RMSNorm, add-to) only"
    if fam == "gemm_lowp" and w == 16 and pro == RMSNORM:
        return "dihip_lm_head uses the RMSNorm prologue for M <= 4 only, and those calls are the decode GEMV's unless DIHIP_GEMV_STREAM=0"
    return "no candidate of the generator's pool is routed here"


def dump(doc):
    with open(OUT, "w") as f:
        f.write("{\n")
        f.write(f' "num_cus": {doc["num_cus"]},\n')
        for key in ("queries", "routes", "unreachable", "over_budget"):
            f.write(f' "{key}": [\n')
            f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in doc[key]))
            f.write("\n ]" + ("\n" if key == "over_budget" else ",\n"))
        f.write("}\n")


def main():
    set_ = [s for s in SWITCHES if s in os.environ]
    assert not set_, f"unset {set_}: the fixture records the default routes"
    lib = load_lib()
    old = json.load(open(OUT)) if os.path.exists(OUT) else {"num_cus": 256, "queries": []}
    if "--queries-only" in sys.argv:
        old["queries"] = [query(lib, *q) for q in query_inputs()]
        dump(old)
        print(len(old["queries"]), "query rows")
        return
    budget = 400
    rows, uncovered = route_rows(lib, budget)
    reachable = {spec_of(r): r for r in route_rows(lib, 1 << 30)[0]}
    assert rows[0][12][13] == 256, "generate on a machine without a GPU (256 CUs assumed) or on an MI355X"
    old["routes"] = rows
    old["unreachable"] = [list(s) + [why_unreachable(s)] for s in uncovered if s not in reachable]
    old["over_budget"] = [list(s) + [reachable[s][:7]] for s in uncovered if s in reachable]
    dump(old)
    print(len(old["queries"]), "query rows,", len(rows), "route rows,", len(old["unreachable"]), "specialisations unreachable,",
          len(old["over_budget"]), "over the budget,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
