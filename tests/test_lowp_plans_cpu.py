"""The host-side plans of the weight-only GEMM, pinned row for row (tests/golden/lowp_plans.json; generator and the choice of
rows: tests/golden/make_lowp_plan_golden.py).  The library answers all of it from shapes alone; without a device it plans
for 256 CUs, the MI355X's.

  queries  the shape-only exports.  Recorded with the library as it was BEFORE the route decision was unified
           (csrc/gemm_lowp_plan.hpp): workspace sizes, layout preferences and plans must not move.
  routes   dihip_debug_gemm_route: family, template specialisation, grid, threads, LDS and slab bytes of every call the
           fixture lists.  A routing change shows up here as the rows it moved.
"""
import ctypes as C
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope="module")
def gen(golden_dir):
    spec = importlib.util.spec_from_file_location("make_lowp_plan_golden", os.path.join(golden_dir, "make_lowp_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "lowp_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib(pkg, gen, golden):
    from dash_infer_amd import capi
    set_ = [s for s in gen.SWITCHES if s in os.environ]
    if set_:
        pytest.fail(f"{set_} set in the environment: the fixture pins the default routes")
    lib = capi.lib()
    cus = C.c_int(0)
    if lib.dihip_device_info(C.byref(cus), None, None, 0) != 0:
        cus.value = 256      # no device: the plans assume the MI355X's count
    if cus.value != golden["num_cus"]:
        pytest.skip(f"the fixture is for {golden['num_cus']} CUs, this device has {cus.value}")
    return lib


def test_fixture_shape(golden, gen):
    assert 0 < len(golden["routes"]) <= 400 and len(golden["queries"]) > 0
    # every specialisation the dispatcher names is reached by a row or listed as left out, in exactly one place
    reached = {gen.spec_of(r) for r in golden["routes"]}
    unreachable = {tuple(u[:9]) for u in golden["unreachable"]}
    over_budget = {tuple(u[:9]) for u in golden["over_budget"]}
    assert reached | unreachable | over_budget == gen.dispatcher_specs()
    assert not (reached & unreachable) and not (reached & over_budget) and not (unreachable & over_budget)
    assert all(isinstance(u[9], str) and u[9] for u in golden["unreachable"])      # the reason


def test_over_budget_rows_reach_their_specialisation(lib, golden, gen):
    for u in golden["over_budget"]:
        row = gen.make_row(lib, *u[9])
        assert row is not None and gen.spec_of(row) == tuple(u[:9]), u


def test_shape_queries_unchanged(lib, golden, gen):
    bad = []
    for q in golden["queries"]:
        got = gen.query(lib, *q["in"])
        if got != q:
            bad.append((q["in"], {k: (q[k], got[k]) for k in q if got[k] != q[k]}))
    assert not bad, f"{len(bad)} of {len(golden['queries'])} query rows differ (recorded, got): {bad[:5]}"


def test_routes(lib, golden, gen):
    bad = []
    for row in golden["routes"]:
        form, wbits, dtype, M, N, K, g, pro, epi, xl, yl, flags, want = row
        # the call an entry point builds for this form is part of what is pinned
        assert gen.form_desc(lib, form, wbits, M, N, K, g) == (pro, epi, xl, yl, flags), row[:12]
        got = gen.route(lib, wbits, dtype, pro, epi, M, N, K, g, xl, yl, flags)
        if got != want:
            bad.append((row[:12], want, got))
    assert not bad, f"{len(bad)} of {len(golden['routes'])} routes differ (call, recorded, got): {bad[:5]}"
