"""The launch plans of RoIAlign and NMS (csrc/roi_plan.h) against the table of what the launchers decided before the
planner was split from them.

tests/golden/roi_plans.json restates, row by row, the conditions and the grid / LDS expressions of the launchers in
csrc/roi_ops.hip and csrc/rpn.hip (and of the route formula ops._RoIAlignFn.backward held) as they stood in the commit before
the planner; ``src`` names the lines.  A change that sends one of these shapes to another kernel form, grid or LDS size fails
here, without a GPU.  Field order: include/i2vsgg_hip.h, i2v_roi_align_fwd_plan / i2v_roi_align_bwd_plan / i2v_nms_plan."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "roi_plans.json")
N_FIELDS = {"align_fwd": 6, "align_bwd": 9, "nms": 11}
FORM_AT = {"align_fwd": 1, "align_bwd": 2, "nms": 6}
FORMS = {"align_fwd": ("ROI128", "ROI64", "COLS", "ROWS", "GENERIC"), "align_bwd": ("SCATTER", "GATHER_ROW", "GATHER_ROW2"),
         "nms": ("SUPER", "PIPELINED", "GENERIC")}
B_STATUS, B_ROUTE, B_FORM, B_GROUPS, B_AVG, B_P7, B_GRID, B_THREADS, B_LDS = range(9)
NHWC, NCHW = 0, 1


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
    """The given tuning keys for the block; the process's own values afterwards."""

    def __init__(self, lib, tuning):
        self.lib, self.tuning = lib, {int(k): v for k, v in tuning.items()}

    def __enter__(self):
        self.old = {k: self.lib.i2v_get_tuning(k) for k in self.tuning}
        for k, v in self.tuning.items():
            assert self.lib.i2v_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.i2v_set_tuning(k, v)
        return False


def plan_of(lib, kind, args, rc=0):
    n = N_FIELDS[kind]
    out = (ctypes.c_int32 * n)()
    fn = {"align_fwd": lib.i2v_roi_align_fwd_plan, "align_bwd": lib.i2v_roi_align_bwd_plan, "nms": lib.i2v_nms_plan}[kind]
    assert fn(*args, out, n) == rc, lib.i2v_last_error()
    return list(out)


def test_the_defaults_are_the_tables(lib, table):
    assert {k: lib.i2v_get_tuning(int(k)) for k in table["defaults"]} == table["defaults"]


def test_the_table_covers_every_form_and_the_named_cases(table):
    rows = table["rows"]
    assert os.path.getsize(TABLE) < (1 << 20)
    for kind, names in FORMS.items():
        ok = [r for r in rows if r["kind"] == kind and r["plan"][0] == 0]
        assert {r["form"] for r in ok} == set(names), kind
        for r in ok:
            assert r["plan"][FORM_AT[kind]] == names.index(r["form"]) and len(r["plan"]) == N_FIELDS[kind] and r["src"], r
    by = {(r["kind"], r["case"]): r for r in rows}
    assert len(by) == len(rows)

    def row(kind, case):
        return by[kind, case]

    # the cases the table must hold, with the figures they were asked to show
    assert (row("align_fwd", "R = 128 (4 x 32, the benchmark's)")["form"], row("align_fwd", "R = 128 (4 x 32, the benchmark's)")["plan"][3]) == ("ROI128", 1024)
    assert [(row("align_fwd", "R = %d" % r)["form"], row("align_fwd", "R = %d" % r)["plan"][3]) for r in (32, 63, 64)] == \
        [("ROI64", 512), ("ROI64", 1008), ("ROI128", 512)]
    assert [row("align_fwd", c)["form"] for c in ("8 x 8, avg = 1", "8 x 8, avg = 0", "8 x 9, avg = 0", "out NCHW", "C = 192", "C = 6",
                                                  "feat NCHW", "ROIALIGN_COLS = 1", "ROIALIGN_COLS = 0")] == \
        ["COLS", "ROI128", "COLS", "COLS", "COLS", "GENERIC", "GENERIC", "COLS", "ROWS"]
    assert row("align_fwd", "ROIALIGN_COLS = 0")["plan"][3] == 128 * 7
    assert row("align_fwd", "B = 8, H = W = 256, C = 1024 (exactly 2^31 bytes)")["form"] == "COLS"
    assert row("align_fwd", "B = 7, H = W = 256, C = 1024")["form"] == "ROI128"
    p = row("align_bwd", "B = 4, C = 1024, 38 x 63, R = 128 (the benchmark's 4 x 32)")["plan"]
    assert p == [0, 1, 2, 1, 1, 1, 1216, 256, 35328]
    p = row("align_bwd", "B = 1, same map, R = 32 (the benchmark's 1 x 32)")["plan"]
    assert (p[B_GROUPS], p[B_GRID]) == (2, 608)
    assert [row("align_bwd", "C = 128, B = 1, H = %d" % h)["plan"][B_GROUPS] for h in (512, 513)] == [2, 1]
    assert row("align_bwd", "W = 78")["plan"][B_ROUTE] == 1 and row("align_bwd", "W = 78")["plan"][B_LDS] == 43008
    for c in ("W = 79", "PW = 8, avg = 1", "C = 192", "NCHW in", "NCHW out", "R = 0"):
        assert row("align_bwd", c)["plan"][B_ROUTE] == 0 and row("align_bwd", c)["form"] == "SCATTER", c
    assert row("align_bwd", "PW = 8, avg = 0")["plan"][B_ROUTE:B_P7 + 1] == [1, 2, 1, 0, 0]
    assert row("align_bwd", "7 x 6, avg = 1")["plan"][B_AVG:B_P7 + 1] == [1, 0]
    assert (row("align_bwd", "ROIALIGN_BWD = 0 at W = 63")["form"], row("align_bwd", "ROIALIGN_BWD = 0 at W = 63")["plan"][B_LDS]) == ("GATHER_ROW", 51712)
    assert (row("align_bwd", "ROIALIGN_BWD = 0 at W = 78")["form"], row("align_bwd", "ROIALIGN_BWD = 0 at W = 78")["plan"][B_LDS]) == ("GATHER_ROW", 59392)
    assert row("align_bwd", "scatter, avg = 1")["plan"][B_GRID] == 100 * 8 and row("align_bwd", "scatter, avg = 0")["plan"][B_GRID] == 100 * 7
    for n in (1, 64, 65, 12000, 12352):
        p = row("nms", "n = %d" % n)["plan"]
        assert (p[6], p[7], p[10]) == (0, 48, 131072), n
    assert row("nms", "n = 12353")["form"] == "GENERIC"
    assert [(row("nms", "NMS_SCAN = %d" % k)["form"], row("nms", "NMS_SCAN = %d" % k)["plan"][7]) for k in (0, 1, 3)] == \
        [("PIPELINED", 0), ("SUPER", 0), ("SUPER", 3)]
    assert all(row("nms", "NMS_SCAN = %d at n = 12353" % k)["form"] == "GENERIC" for k in (0, 1, 3))
    assert row("nms", "mask launch, n = 12000, n_img = 3")["plan"][2:5] == [188, 188, 3]


def test_every_plan_equals_the_table(lib, table):
    bad = []
    for i, row in enumerate(table["rows"]):
        with tuned(lib, row["tuning"]):
            got = plan_of(lib, row["kind"], row["args"])
        if got != row["plan"]:
            bad.append((i, row, got))
    assert not bad, "%d plans moved; the first: row %d %r -> %r" % (len(bad), bad[0][0], bad[0][1], bad[0][2])


def test_the_gather_route_is_the_old_formula(lib):
    """route == GATHER exactly where ops._RoIAlignFn.backward's formula held, swept over the formula's own variables."""
    n = 0
    for fl in (NHWC, NCHW):
        for ol in (NHWC, NCHW):
            for C in (64, 128, 192, 1024):
                for W in (2, 63, 77, 78, 79, 82, 83, 114, 115, 200):
                    for pw, avg in ((7, 1), (7, 0), (8, 0), (8, 1), (9, 0)):
                        for R in (0, 1, 128):
                            old = fl == NHWC and ol == NHWC and C % 128 == 0 and W * 512 + 21504 <= 60 * 1024 and pw + avg <= 8 and R > 0
                            p = plan_of(lib, "align_bwd", [ol, R, 7, pw, avg, fl, 2, C, 20, W])
                            assert p[B_ROUTE] == int(old) and p[B_STATUS] == 0, (fl, ol, C, W, pw, avg, R, p)
                            n += old
    assert n >= 40


def test_the_kernel_names_the_profilers_count_are_the_planned_ones(lib):
    """ops.ROIALIGN_BWD_KERNELS / ops.NMS_KERNELS (what bench.py and the PMC tools count per op) at the benchmark's headline shapes
    under the default tuning: 4 x 32 and 1 x 32 RoIAlign backward, NMS at 12000 and 6000."""
    from i2vsgg_amd import ops
    bwd_kernel = {0: "roi_align_bwd_kernel", 1: "roi_align_bwd_row_kernel", 2: "roi_align_bwd_row2_kernel"}
    scan_kernel = {0: "nms_scan_super_kernel", 1: "nms_scan_pipelined_kernel", 2: "nms_scan_kernel"}
    for B in (4, 1):
        p = ops.roi_align_bwd_plan(False, B * 32, 7, 7, 1, True, B, 1024, 38, 63)
        assert p["status"] == 0 and p["route"] == ops.ROUTE_GATHER and ops.ROIALIGN_BWD_GATHER
        assert ops.ROIALIGN_BWD_KERNELS == {bwd_kernel[p["form"]]: 1}
    for n in (12000, 6000):
        p = plan_of(lib, "nms", [1, n])
        assert ops.NMS_KERNELS == {"nms_mask_kernel": 1, scan_kernel[p[6]]: 1}


def test_plan_exports_check_their_arguments_and_report_refusals(lib):
    out = (ctypes.c_int32 * 16)()
    # too few slots
    assert lib.i2v_roi_align_fwd_plan(NHWC, 1, 128, 8, 8, 4, 7, 7, 1, NHWC, out, 5) == -1 and b"I2V_ROI_ALIGN_FWD_PLAN_FIELDS" in lib.i2v_last_error()
    assert lib.i2v_roi_align_bwd_plan(NHWC, 4, 7, 7, 1, NHWC, 1, 128, 8, 8, out, 8) == -1
    assert lib.i2v_nms_plan(1, 100, out, 10) == -1
    assert lib.i2v_nms_plan(1, 100, None, 11) == -1
    # bad shapes are errors, as at the entry points
    assert lib.i2v_roi_align_bwd_plan(NHWC, 4, 7, 7, 2, NHWC, 1, 128, 8, 8, out, 9) == -1 and b"avg must be 0/1" in lib.i2v_last_error()
    assert lib.i2v_nms_plan(1, 65537, out, 11) == -1
    # a shape an entry point refuses is a plan with a status.  The gather route's further bounds:
    p = plan_of(lib, "align_bwd", [NHWC, 1 << 26, 7, 7, 1, NHWC, 1, 128, 8, 8])              # R * (PH + avg) = 2^29
    assert (p[B_STATUS], p[B_ROUTE]) == (4, 1)
    p = plan_of(lib, "align_bwd", [NHWC, (1 << 26) - 1, 7, 7, 1, NHWC, 1, 128, 8, 8])        # pairs fit; grad_out of 128 * 49 * 4 B per ROI does not
    assert (p[B_STATUS], p[B_ROUTE]) == (6, 1)
    p = plan_of(lib, "align_bwd", [NHWC, 85598, 7, 7, 1, NHWC, 1, 128, 8, 8])                # 85598 * 25088 B < 2^31 <= 85599 * 25088 B
    assert p[B_STATUS] == 0
    assert plan_of(lib, "align_bwd", [NHWC, 85599, 7, 7, 1, NHWC, 1, 128, 8, 8])[B_STATUS] == 6
    p = plan_of(lib, "align_bwd", [NHWC, 4, 7, 7, 1, NHWC, 1 << 14, 128, 1 << 17, 8])        # B * H * (C / 128) = 2^31
    assert (p[B_STATUS], p[B_ROUTE]) == (5, 1)
    # the entry points turn a status into I2V_ERR_ARG before anything touches the device (the pointers are never read)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.i2v_roi_align_bwd_gather(p, p, 1 << 26, 7, 7, 1.0, 1, p, 1, 128, 8, 8, None, 0, None) == -1
    assert lib.i2v_last_error() == b"roi_align_bwd_gather: map too wide for the LDS row buffer"
    assert lib.i2v_roi_align_bwd_gather(p, p, 4, 7, 7, 1.0, 1, p, 1, 192, 8, 8, None, 0, None) == -1
    assert lib.i2v_last_error() == b"roi_align_bwd_gather: C must be a multiple of 128 (NHWC in and out)"
