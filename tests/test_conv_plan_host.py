"""The launch plans of the convolution GEMMs (csrc/conv_plan.h) against the table the previous launchers produced.

tests/golden/conv_plans.json holds, for every distinct GEMM of the single-GPU bench steps and of the parametrisations in
tests/test_gpu_kernels.py, under the default and the ordered (I2V_TUNE_SPLIT_ATOMICS = 0) context, what run_conv /
launch_wgrad decided before the planner was split from them (written by an instrumented build of that code, never by the
planner).  A change that picks another tile, split, finish or kernel form for one of these shapes fails here, without a GPU;
the value tests cannot see it.  A row: the export's arguments (``args``), the tuning keys that differ from the defaults and
the forced tile it was planned under, the plan, and ``src`` -- which run launched the shape (sgg / 801: the relation step at
2 x 600x1000 / 600x801; isd / isd128: the detector step at 32 / 128 ROIs; kernels: tests/test_gpu_kernels.py; example: shapes
named in the planner's comments).  Field order: include/i2vsgg_hip.h, i2v_conv_fwd_plan / i2v_conv_wgrad_plan."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plans.json")
FWD_FORMS = {"IGEMM": 0, "GEMM": 1, "GEMM_DMA32": 2, "GEMM_DMA16": 3, "GEMM_KGROUPS2": 4, "GEMM_KGROUPS4": 5}
FWD_FINISHES = {"NONE": 0, "IN_KERNEL": 1, "ATOMICS": 2}
WGRAD_FINISHES = {"DIRECT": 0, "ATOMICS": 1, "ORDERED_TILES": 2, "ORDERED_PARTS": 3, "EXTERNAL_PARTS": 4}
F_STATUS, F_FORM, F_FINISH, F_WS_WANTED = 0, 5, 7, 8
W_STATUS, W_FINISH = 0, 7


@pytest.fixture(scope="module")
def lib():
    from i2vsgg_amd import build
    build.build()
    from i2vsgg_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


class tuned:
    """The row's tuning and forced tile for the block; the process's own values afterwards."""

    def __init__(self, lib, row):
        self.lib, self.row = lib, row

    def __enter__(self):
        self.old = {int(k): self.lib.i2v_get_tuning(int(k)) for k in self.row["tuning"]}
        for k, v in self.row["tuning"].items():
            assert self.lib.i2v_set_tuning(int(k), v) == 0
        assert self.lib.i2v_conv_set_tile(self.row["tile"]) == 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.i2v_set_tuning(k, v)
        self.lib.i2v_conv_set_tile(-1)
        return False


def plan_of(lib, row):
    n = 13 if row["kind"] == "fwd" else 17
    out = (ctypes.c_int32 * n)()
    fn = lib.i2v_conv_fwd_plan if row["kind"] == "fwd" else lib.i2v_conv_wgrad_plan
    assert fn(*row["args"], out, n) == 0
    return list(out)


def test_the_table_covers_every_form_and_finish(table):
    rows = table["rows"]
    assert 200 <= len(rows) and os.path.getsize(TABLE) < (1 << 20)
    fwd = [r["plan"] for r in rows if r["kind"] == "fwd" and r["plan"][F_STATUS] == 0]
    wg = [r["plan"] for r in rows if r["kind"] == "wgrad" and r["plan"][W_STATUS] == 0]
    assert {p[F_FORM] for p in fwd} == set(FWD_FORMS.values())
    assert {p[F_FINISH] for p in fwd} == set(FWD_FINISHES.values())
    assert {p[W_FINISH] for p in wg} == set(WGRAD_FINISHES.values())
    # both contexts
    assert any(r["tuning"].get("4") == 0 for r in rows) and any("4" not in r["tuning"] for r in rows)


def test_the_defaults_are_the_tables(lib, table):
    assert [lib.i2v_get_tuning(k) for k in range(len(table["defaults"]))] == table["defaults"]


def test_every_plan_equals_the_table(lib, table):
    bad = []
    for i, row in enumerate(table["rows"]):
        with tuned(lib, row):
            got = plan_of(lib, row)
        if got != row["plan"]:
            bad.append((i, row, got))
    assert not bad, "%d plans moved; the first: row %d %r -> %r" % (len(bad), bad[0][0], bad[0][1], bad[0][2])


def test_the_split_queries_agree_with_the_plan(lib, table):
    """i2v_conv_fwd_splits / i2v_conv_split_workspace_bytes are views of the same plan (they take no flags and no batch)."""
    n = 0
    for row in table["rows"]:
        if row["kind"] != "fwd" or row["args"][9] > 1:
            continue
        shape, ws = row["args"][:9], row["args"][11]
        with tuned(lib, row):
            splits, want = lib.i2v_conv_fwd_splits(*shape, ws), lib.i2v_conv_split_workspace_bytes(*shape)
        plan = row["plan"]
        if plan[F_STATUS] != 0:
            assert splits < 0 and want == 0, row
            continue
        assert splits == (1 if plan[F_FINISH] == FWD_FINISHES["ATOMICS"] else 0), row
        assert want == plan[F_WS_WANTED], row
        n += 1
    assert n >= 100


def test_planning_counts_no_ordered_fallback(lib, table):
    """Only a launch counts a refused ordered sum; asking for the plan does not."""
    lib.i2v_ordered_fallbacks(1)
    rows = [r for r in table["rows"] if r["plan"][-1] == 1]
    assert rows
    for row in rows[:8]:
        with tuned(lib, row):
            assert plan_of(lib, row)[-1] == 1
    assert lib.i2v_ordered_fallbacks(0) == 0


def test_plan_exports_check_their_arguments(lib):
    out = (ctypes.c_int32 * 17)()
    assert lib.i2v_conv_fwd_plan(1, 8, 8, 4, 8, 1, 1, 1, 0, 0, 0, 0, out, 12) == -1           # too few slots
    assert lib.i2v_conv_wgrad_plan(1, 8, 8, 4, 8, 1, 1, 1, 0, 0, 0, 0, 0, -1, 0, out, 16) == -1
    assert lib.i2v_conv_fwd_plan(1, 8, 8, 3, 8, 1, 1, 1, 0, 0, 0, 0, out, 13) == -1 and b"multiple of 4" in lib.i2v_last_error()
    # a shape the kernels do not take is a plan with a status, not an error: a 7x7 filter of 256 channels overflows the tap table
    assert lib.i2v_conv_fwd_plan(1, 32, 32, 256, 64, 7, 7, 1, 3, 0, 0, 0, out, 13) == 0 and out[0] == 1
    assert lib.i2v_conv_fwd_splits(1, 32, 32, 256, 64, 7, 7, 1, 3, 0) < 0
