"""Issues every `routes` row of tests/golden/lowp_plans.json through the public entry points of the weight-only GEMM, so that
a kernel trace shows which kernels the library REALLY launches for them, and compares such traces.

  run      rocprofv3 --kernel-trace --output-format csv -d DIR -o sweep -- python tools/gemm_route_sweep.py run
           Zero-filled buffers of the packed sizes (contents do not affect routing).  A one-workgroup marker kernel
           (dihip_increment_u32) separates the rows in the trace.  DIHIP_LIB_DIR selects another build of the library; only
           entry points that every build has are used.
  check    python tools/gemm_route_sweep.py check NEW_kernel_trace.csv [--against OLD_kernel_trace.csv] [--out FILE]
           The trace must agree with the fixture's routes (kernel family, template arguments, grid, workgroup size), and
           row for row with the other build's trace (kernel name, grid, workgroup size, LDS size).  The trace's LDS column is
           a kernel's STATIC allocation (0 for a gemm_prefill launch with 66560 dynamic bytes, measured), the route's LDS
           field the DYNAMIC bytes of the launch (gemv_stream, gemm_prefill, gemm_lowp; 0 for the families whose kernels
           declare their LDS): a launch has at most one of the two, which is what is checked against the routes, so the
           dynamic size is pinned by the CPU test alone.  Writes the summary; exit status 1 on any difference.
"""
import argparse
import collections
import csv
import ctypes as C
import importlib.util
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lowp_plans.json")
MARKER = "increment_u32_kernel"
ROW, FRAG = 0, 1


def load_module(name, path, **kw):
    spec = importlib.util.spec_from_file_location(name, path, **kw)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# ---- run ------------------------------------------------------------------------------------------------------------------
def run(rows):
    import torch
    pkg_dir = os.path.join(ROOT, "dash-infer_amd")
    pkg = load_module("dash_infer_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    from dash_infer_amd import capi
    lib = C.CDLL(pkg.LIB_PATH)
    for name, (res, args) in capi._SIGS.items():    # the bindings of this tree, for whatever the loaded build exports
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    print("library:", pkg.LIB_PATH, lib.dihip_version().decode(), flush=True)

    bufs = {}

    def zeros(key, nbytes):
        if key not in bufs or bufs[key].numel() < nbytes:
            bufs[key] = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        return C.c_void_p(bufs[key].data_ptr())

    weights = collections.OrderedDict()

    def packed(wbits, N, K, g, which):
        key = (wbits, N, K, g)
        if key not in weights:
            while len(weights) >= 6:                    # a handful of matrices stay resident
                weights.popitem(last=False)
            wb = lib.dihip_dense_packed_weight_bytes(N, K) if wbits == 16 else lib.dihip_gemm_lowp_packed_weight_bytes(wbits, N, K)
            sb = 256 if wbits == 16 else lib.dihip_gemm_lowp_packed_sz_bytes(N, K, g)
            weights[key] = [torch.zeros(int(b), dtype=torch.uint8, device="cuda") for b in (wb, sb, wb, sb)]
        return C.c_void_p(weights[key][which].data_ptr())

    sync = zeros("sync", lib.dihip_gemm_lowp_sync_bytes())
    marker = zeros("marker", 256)
    parts = C.c_int(0)
    issued = 0
    for i, row in enumerate(rows):
        form, wbits, dtype, M, N, K, g, pro, epi, xl, yl, flags, _ = row
        name = form.partition(":")[0]
        ws_bytes = lib.dihip_dense_workspace_bytes(M, N, K) if wbits == 16 else lib.dihip_gemm_lowp_workspace_bytes(wbits, M, N, K, g)
        ws = zeros("ws", ws_bytes)
        x = zeros("x", max(M, 32) * K * 4)              # FT rows, FRAG32 tiles or the f32 hidden stream
        y = zeros("y", max(M, 32) * N * 4)
        xnorm = zeros("xnorm", max(M, 32) * N * 2)
        gamma = zeros("gamma", max(N, K) * 2)
        rowsq = zeros("rowsq", lib.dihip_rowsq_bytes())
        w0, s0, w1, s1 = (packed(wbits, N, K, g, j) for j in range(4))
        dims = (M, N, K, g)
        if name == "std":
            fn = lib.dihip_gemm_a16w4 if wbits == 4 else lib.dihip_gemm_a16w8
            st = fn(None, x, w0, s0, None, None, y, *dims, 0, 1.0, ws, ws_bytes, None if "nosync" in form else sync, dtype)
        elif name == "a16w16":
            st = lib.dihip_gemm_a16w16(None, x, w0, None, None, y, M, N, K, 0, 1.0, ws, ws_bytes, sync, dtype)
        elif name == "lm_head":
            st = lib.dihip_lm_head(None, y, x, gamma, 1e-6, w0, M, N, K, ws, ws_bytes, sync, dtype)
        elif name == "norm_gemm":
            st = lib.dihip_fused_norm_gemm(None, wbits, x, gamma, 1e-6, w0, s0, None, y, *dims, 0, ws, ws_bytes, sync, dtype)
        elif name == "norm_swiglu":
            st = lib.dihip_fused_norm_swiglu_ex(None, wbits, x, gamma, 1e-6, w0, s0, w1, s1, y, *dims, ws, ws_bytes, sync, dtype, yl)
        elif name == "addto":
            st = lib.dihip_fused_gemm_addto_ex(None, wbits, x, w0, s0, None, y, *dims, ws, ws_bytes, sync, dtype, xl)
        elif name == "addto_norm":
            st = lib.dihip_fused_gemm_addto_norm(None, wbits, x, w0, s0, None, y, *dims, ws, ws_bytes, sync, dtype, xl, gamma, 1e-6, xnorm, ROW)
        elif name == "addto_prenorm":
            st = lib.dihip_fused_gemm_addto_prenorm(None, wbits, x, w0, s0, None, y, *dims, ws, ws_bytes, sync, dtype, xl, gamma, 1e-6,
                                                    xnorm, ROW, rowsq, lib.dihip_rowsq_bytes(), C.cast(C.pointer(parts), C.c_void_p))
        elif name in ("prenorm_gemm", "prenorm_gemm_rowsq"):
            rs = (rowsq, 1) if name.endswith("rowsq") else (None, 0)
            st = lib.dihip_prenorm_gemm_rowsq(None, wbits, x, xl, w0, s0, None, y, *dims, 0, ws, ws_bytes, sync, dtype, *rs, 1e-6)
        elif name in ("prenorm_swiglu", "prenorm_swiglu_rowsq"):
            rs = (rowsq, 1) if name.endswith("rowsq") else (None, 0)
            st = lib.dihip_prenorm_swiglu_rowsq(None, wbits, x, xl, w0, s0, w1, s1, y, *dims, ws, ws_bytes, sync, dtype, yl, *rs, 1e-6)
        else:
            raise SystemExit(f"row {i}: unknown form {form}")
        if st != 0:
            raise SystemExit(f"row {i} {row[:12]}: status {st}: {lib.dihip_last_error().decode()}")
        if lib.dihip_increment_u32(None, marker, 1) != 0:
            raise SystemExit("marker launch failed")
        issued += 1
        if i % 50 == 49:
            torch.cuda.synchronize()        # a fault surfaces near the row that caused it
            print(f"{i + 1} rows issued", flush=True)
    torch.cuda.synchronize()
    print(f"issued {issued} rows; marker count {int(bufs['marker'][:4].view(torch.int32)[0])}", flush=True)


# ---- check ----------------------------------------------------------------------------------------------------------------
Launch = collections.namedtuple("Launch", "name grid wg lds")


def read_trace(path):
    """Launches of the trace in dispatch order, split into rows at the marker kernel."""
    with open(path, newline="") as f:
        recs = list(csv.DictReader(f))
    col = lambda *names: next(n for n in names if n in recs[0])
    lds_col = col("LDS_Block_Size", "Group_Segment_Size", "LDS_Block_Size_v")
    order = col("Dispatch_Id", "Start_Timestamp")
    recs.sort(key=lambda r: int(r[order]))
    rows, cur = [], []
    for r in recs:
        wg = tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")
        grid = tuple(int(r[f"Grid_Size_{a}"]) // max(w, 1) for a, w in zip("XYZ", wg))   # the trace counts work-items
        if MARKER in r["Kernel_Name"]:
            rows.append(cur)
            cur = []
        else:
            cur.append(Launch(r["Kernel_Name"], grid, wg, int(r[lds_col])))
    return rows


KERNEL_RE = re.compile(r"(gemv_stream|gemm_kslice|gemm_panel|gemv_batch|gemm_prefill|gemm_lowp)_kernel<([^>]*)>")


def expected_args(row):
    """Template arguments of the family's kernel as the route records them."""
    wbits, dtype, r = row[1], row[2], row[12]
    fam, mt, nt, pro, epi, gpt, rs = r[0], *r[1:7]
    return {1: ("gemv_stream", [wbits, dtype, mt, pro, epi, gpt]), 2: ("gemm_kslice", [wbits, dtype, mt, epi, gpt] + ([1] if rs else [])),
            3: ("gemm_panel", [wbits, dtype, mt, epi, gpt]), 4: ("gemv_batch", [wbits, dtype, mt, nt, epi, gpt]),
            5: ("gemm_prefill", [wbits, dtype, epi, gpt]), 6: ("gemm_lowp", [wbits, dtype, mt, nt, pro, epi])}[fam]


def check_against_routes(rows, trace):
    diffs, static_lds, seen = [], collections.defaultdict(collections.Counter), collections.defaultdict(set)
    if len(rows) != len(trace):
        return [f"the fixture has {len(rows)} rows, the trace {len(trace)}"], static_lds, seen
    for i, (row, launches) in enumerate(zip(rows, trace)):
        r = row[12]
        fam, args = expected_args(row)
        mine = [(l, KERNEL_RE.search(l.name)) for l in launches]
        mine = [(l, m) for l, m in mine if m]
        for l in launches:
            if "dihip::" in l.name:
                seen[fam].add(re.sub(r"\(.*", "", l.name))
        if len(mine) != 1:
            diffs.append(f"row {i} {row[:7]}: {len(mine)} GEMM kernels in the trace, expected one {fam}")
            continue
        l, m = mine[0]
        got = [int(re.sub(r"\(.*\)", "", a).strip().replace("false", "0").replace("true", "1")) for a in m.group(2).split(",")]
        if m.group(1) != fam or got[:len(args)] != args or any(got[len(args):]):
            diffs.append(f"row {i} {row[:7]}: route {fam}<{args}>, trace {m.group(1)}<{got}>")
        if list(l.grid) != r[7:10] or l.wg[0] != r[10]:
            diffs.append(f"row {i} {row[:7]}: route grid {r[7:10]} x {r[10]} threads, trace {list(l.grid)} x {l.wg[0]}")
        if l.lds and r[11]:
            diffs.append(f"row {i} {row[:7]}: {l.lds} bytes of static LDS in the trace and {r[11]} dynamic bytes in the route")
        static_lds[fam][l.lds] += 1
    return diffs, static_lds, seen


def check(args):
    rows = json.load(open(args.fixture))["routes"]
    new = read_trace(args.trace)
    out = [f"fixture rows: {len(rows)}; rows in {args.trace}: {len(new)}; launches: {sum(map(len, new))}"]
    diffs, static_lds, seen = check_against_routes(rows, new)
    out.append(f"trace vs routes (family, template arguments, grid, workgroup size; static or dynamic LDS): {len(diffs)} differences")
    out += ["  " + d for d in diffs]
    out.append("static LDS in the trace, rows per family and size: "
               + "; ".join(f"{f} " + ", ".join(f"{b} B x {n}" for b, n in sorted(d.items())) for f, d in sorted(static_lds.items())))
    ndiff = len(diffs)
    if args.against:
        old = read_trace(args.against)
        d2 = [] if len(old) == len(new) else [f"{len(new)} rows against {len(old)}"]
        for i, (a, b) in enumerate(zip(new, old)):
            if a != b:
                d2.append(f"row {i} {rows[i][:7] if i < len(rows) else ''}: {a} != {b}")
        out.append(f"trace vs {args.against} (kernel name, grid, workgroup size, LDS size; row for row, "
                   f"{sum(map(len, old))} launches): {len(d2)} differences")
        out += ["  " + d for d in d2]
        ndiff += len(d2)
    out.append("kernels seen per family:")
    for fam in sorted(seen):
        out.append(f"  {fam}: {len(seen[fam])}")
        out += ["    " + k for k in sorted(seen[fam])]
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    sys.stdout.write(text if len(text) < 20000 else text[:20000] + "...\n")
    return 1 if ndiff else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("run", "check"))
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--fixture", default=FIXTURE)
    ap.add_argument("--against")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.mode == "run":
        run(json.load(open(args.fixture))["routes"])
        return 0
    return check(args)


if __name__ == "__main__":
    sys.exit(main())
