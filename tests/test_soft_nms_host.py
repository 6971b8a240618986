"""Soft-NMS, host side (no GPU): the host form of i2vsgg_amd/soft_nms.py -- the specification the kernel is held to in
tests/test_gpu_soft_nms.py -- on hand-worked cases, against the pinned greedy NMS, on the properties the rules promise, and the
margins that make the gaussian order comparison on the GPU meaningful; then the launch plans of csrc/roi_plan.h."""
import ctypes
import functools
import math

import numpy as np
import pytest

import nms_cases as nc
import soft_nms_cases as sc
from i2vsgg_amd import soft_nms as sn

F32 = np.float32


def f32(x):
    return F32(x)


# Three 10 x 10 boxes (+1 extents: area 100) on one row: B is A moved 2 px right, C is A moved 6 px right.
#   IoU(A, B) = 80 / (100 + 100 - 80) = 80 / 120        IoU(A, C) = 40 / 160 = 0.25        IoU(B, C) = 60 / 140
HAND = np.array([[0, 0, 9, 9, 0.9], [2, 0, 11, 9, 0.8], [6, 0, 15, 9, 0.7]], F32)
I_AB, I_AC, I_BC = f32(80) / f32(120), f32(40) / f32(160), f32(60) / f32(140)


def _run(rows, method, nt=0.3, sigma=0.5, min_score=0.001, stats=None):
    out, src, num = sn.soft_nms_host(rows, None, method, nt, sigma, min_score, stats)
    return out[0, :num[0]], src[0, :num[0]]


def test_hand_worked_hard():
    # A is picked; B (0.667 > 0.3) is dropped, C (0.25) stays untouched; C is picked
    out, src = _run(HAND, "hard")
    assert src.tolist() == [0, 2]
    assert np.array_equal(out, HAND[[0, 2]])


def test_hand_worked_linear():
    # A is picked: B <- 0.8 * (1 - 80/120), C untouched (0.25 is not > 0.3).  C (0.7) now leads B (0.2667) and is picked:
    # B <- B * (1 - 60/140) = 0.152..., then B is picked last
    b1 = f32(0.8) * (f32(1) - I_AB)
    b2 = b1 * (f32(1) - I_BC)
    out, src = _run(HAND, "linear")
    assert src.tolist() == [0, 2, 1]
    assert out[:, 4].view(np.int32).tolist() == np.array([f32(0.9), f32(0.7), b2], F32).view(np.int32).tolist()
    assert np.array_equal(out[:, :4], HAND[[0, 2, 1], :4])
    # with min_score between b2 and b1 the second decay drops B; with min_score above b1 the first one does
    assert _run(HAND, "linear", min_score=0.2)[1].tolist() == [0, 2]
    assert b2 < f32(0.2) < b1
    assert _run(HAND, "linear", min_score=0.3)[1].tolist() == [0, 2]


def test_hand_worked_gaussian():
    # every other live row is decayed at every pick, the weight in float64, one rounding to float32:
    # A picked: B <- 0.8 exp(-(80/120)^2 / 0.5) = 0.3289, C <- 0.7 exp(-0.25^2 / 0.5) = 0.6177; C picked: B <- B exp(-(60/140)^2 / 0.5)
    def g(s, iou):
        return F32(np.float64(s) * math.exp(-(float(iou) * float(iou)) / 0.5))

    b1, c1 = g(f32(0.8), I_AB), g(f32(0.7), I_AC)
    b2 = g(b1, I_BC)
    assert c1 > b1
    stats = {}
    out, src = _run(HAND, "gaussian", stats=stats)
    assert src.tolist() == [0, 2, 1]
    want = np.array([f32(0.9), c1, b2], F32)
    assert np.abs(out[:, 4].view(np.int32) - want.view(np.int32)).max() <= 1          # math.exp against numpy's: a last bit
    assert stats["decays"][0].tolist() == [0, 1, 2]
    assert abs(stats["pick_gap"] - (float(c1) - float(b1)) / float(c1)) < 1e-6


@functools.lru_cache(maxsize=None)
def _pinned_sets():
    """Sets of tests/nms_cases.py whose IoUs hold no NaN (a NaN suppresses in the reference's ``!(ovr <= thresh)`` and applies no
    decay under the strict ``>`` of the rules here, so the degenerate cases are not comparable)."""
    ladders = {c.name: c for c in nc.ladder_cases()}
    return [nc.threshold_case(0.3), nc.threshold_case(0.7), ladders["cap48_L48"], ladders["cap5_L5"], ladders["end_n1025"]]


@pytest.mark.parametrize("k", range(5))
def test_hard_emits_the_pinned_greedy_keep_list(k):
    case = _pinned_sets()[k]
    S, _, _, ovr = nc.suppression_matrix(case.dets, case.thresh)
    assert not np.isnan(ovr).any()
    keep = nc.greedy_keep(S)
    out, src = _run(case.dets, "hard", nt=case.thresh)
    assert np.array_equal(src, keep), case.name
    assert np.array_equal(out, case.dets[keep])
    assert 0 < len(keep) < len(case.dets)


def test_a_nan_iou_is_where_hard_leaves_the_reference_and_decays_nothing():
    """Two equal zero-area boxes: inter = 0, d = 0 + 0 - 0, IoU = 0 / 0.  The reference's ``!(ovr <= thresh)`` lets a NaN suppress
    (``greedy_keep`` drops the second box); under the strict ``iou > Nt`` of the rules here no method applies a decay to it."""
    rows = np.array([[100, 100, 99, 150, 0.9], [100, 100, 99, 150, 0.8], [300, 200, 360, 260, 0.7]], F32)
    S, _, _, ovr = nc.suppression_matrix(rows, 0.3)
    assert np.isnan(ovr[0, 1]) and S[0, 1] and nc.greedy_keep(S).tolist() == [0, 2]
    area = (rows[:, 2] - rows[:, 0] + F32(1)) * (rows[:, 3] - rows[:, 1] + F32(1))
    assert area.tolist() == [0, 0, 61 * 61] and np.isnan(sn.iou_row(rows[:, :4], area, 0)[1])
    for method in sn.METHODS:
        stats = {}
        out, src = _run(rows, method, stats=stats)
        assert src.tolist() == [0, 1, 2] and np.array_equal(out, rows), method          # kept, scores untouched (gaussian too)
        assert stats["decays"][0].tolist() == [0, 0, 0], method
    # the same pair among ordinary boxes, as nms_cases' degenerate set holds it: hard keeps one row more than the pinned greedy rule
    case = nc.degenerate_cases()[0]
    b = case.dets[:, :4]
    with np.errstate(all="ignore"):
        ok = np.isfinite(b).all(1) & (b[:, 2] - b[:, 0] + F32(1) >= 0) & (b[:, 3] - b[:, 1] + F32(1) >= 0)
    dets = nc.with_scores(b[ok])
    S, _, _, ovr = nc.suppression_matrix(dets, case.thresh)
    assert np.isnan(ovr[np.triu_indices(len(dets), 1)]).any()
    keep = nc.greedy_keep(S)
    src = _run(dets, "hard", nt=case.thresh)[1]
    with np.errstate(all="ignore"):
        strict = nc.greedy_keep((ovr > F32(case.thresh)) & np.triu(np.ones(S.shape, bool), 1))
    assert np.array_equal(src, strict) and set(keep.tolist()) < set(src.tolist())


def test_the_banded_gaussian_case_at_the_capacity_keeps_the_margin():
    c = sc.banded_gaussian_case()
    assert len(c.rows) == 4096 and sc.fit(c.stats, 4096) and min(c.stats["pick_gap"], c.stats["min_score_gap"]) > 2.0 ** -10
    assert (np.diff(c.rows[:, 4]) <= 0).all() and c.num > 4000
    active = np.nonzero(c.rows[:, 1] < nc.FILLER_Y)[0]
    assert len(active) == 24 and active.min() < 64 and active.max() >= 4032          # first and last lanes' rows among them ...
    assert ((active > 1024) & (active < 3072)).any()                                 # ... and rows of the middle registers
    assert (c.decays > 0).sum() >= 8 and c.decays.max() >= 3 and (np.diff(c.src) < 0).any()


def test_threshold_pairs_sit_on_the_threshold_and_one_ulp_to_either_side():
    t = F32(sc.NT)
    seen = set()
    for wa, wb, which in sc.threshold_pairs()[:30]:
        rows = np.array([[0, 0, wa - 1, 0, 0.9], [0, 0, wb - 1, 0, 0.8]], F32)
        area = (rows[:, 2] - rows[:, 0] + F32(1)) * (rows[:, 3] - rows[:, 1] + F32(1))
        iou = sn.iou_row(rows[:, :4], area, 0)[1]
        assert int(iou.view(np.int32)) - int(t.view(np.int32)) == which
        seen.add(which)
        for method in ("hard", "linear"):
            out, src = _run(rows, method, nt=sc.NT)
            if which <= 0:                                   # == Nt and below: strict >, nothing happens
                assert np.array_equal(out, rows)
            elif method == "hard":
                assert src.tolist() == [0]
            else:
                assert src.tolist() == [0, 1] and out[1, 4] == F32(0.8) * (F32(1) - iou)
    assert seen == {-1, 0, 1}


@pytest.mark.parametrize("method", sn.METHODS)
@pytest.mark.parametrize("n", (65, 300))
def test_properties_of_every_family(n, method):
    for batch in sc.batches(n, method):
        for c in batch:
            what = (c.family, n, len(c.rows), method)
            s = c.out[:, 4]
            assert (np.diff(s) <= 0).all(), what                                     # emission order is non-increasing
            assert len(set(c.src.tolist())) == c.num and (c.src >= 0).all() and (c.src < len(c.rows)).all(), what
            assert np.array_equal(c.out[:, :4], c.rows[c.src, :4]), what
            untouched = c.decays == 0
            assert np.array_equal(s[untouched], c.rows[c.src[untouched], 4]), what
            assert (s <= c.rows[c.src, 4]).all(), what                               # scores only fall
            if c.num < len(c.rows):                                                  # only a decayed row is ever dropped
                gone = np.setdiff1d(np.arange(len(c.rows)), c.src)
                boxes = c.rows[:, :4]
                area = (boxes[:, 2] - boxes[:, 0] + F32(1)) * (boxes[:, 3] - boxes[:, 1] + F32(1))
                for g in gone[:50]:
                    iou = sn.iou_row(boxes, area, int(g))[c.src]
                    assert (iou > (0 if method == "gaussian" else F32(sc.NT))).any(), what
            if c.family == "ladder" and method != "hard" and len(c.rows) >= 8:
                assert (np.diff(c.src) < 0).any(), what                              # a decay changed the next pick
            if c.family == "stack" and len(c.rows) > 1:
                assert c.num < len(c.rows) and (c.decays[1:] == np.arange(1, c.num)).all(), what


def test_a_row_no_decay_was_applied_to_is_never_dropped():
    # disjoint boxes with scores below min_score, zero and negative: all are emitted, in score order, untouched
    rows = np.concatenate([nc.filler(6), np.array([0.5, 0.0005, 0.0, -0.0, -1.0, -2.0], F32)[:, None]], 1).astype(F32)
    rows[3, 4] = F32(0.0)
    for method in ("hard", "linear"):
        out, src = _run(rows, method)
        assert src.tolist() == list(range(6)) and np.array_equal(out, rows), method
    # gaussian applies a decay of weight exactly 1 to a disjoint row (IoU 0): the score keeps its bits, the drop rule acts
    out, src = _run(rows, "gaussian")
    assert src.tolist() == [0] and np.array_equal(out, rows[:1])
    out, src = _run(rows, "gaussian", min_score=-10.0)
    assert src.tolist() == list(range(6)) and np.array_equal(out, rows)


def test_count_zero_and_count_one():
    dets = np.zeros((3, 4, 5), F32)
    dets[:, :, :] = [0, 0, 10, 10, 0.5]
    for method in sn.METHODS:
        out, src, num = sn.soft_nms_host(dets, [0, 1, 4], method, 0.3)
        # four identical boxes: hard drops three, linear scales them to 0 < min_score; gaussian keeps them at 0.5 e^-2, e^-4, e^-6
        assert num.tolist() == [0, 1, 4 if method == "gaussian" else 1]
        assert (src[0] == -1).all() and src[1].tolist() == [0, -1, -1, -1] and np.array_equal(out[1, 0], dets[1, 0])
    out, src, num = sn.soft_nms_host(np.zeros((1, 0, 5), F32), None, "linear", 0.3)
    assert out.shape == (1, 0, 5) and num.tolist() == [0]


def test_equal_scores_resolve_to_the_lowest_row():
    rows = np.concatenate([nc.filler(5), np.full((5, 1), 0.25, F32)], 1).astype(F32)
    for method in ("hard", "linear"):
        assert _run(rows, method)[1].tolist() == [0, 1, 2, 3, 4]
    # two tied boxes that overlap: the lower row is picked and decays the other, which then comes last
    rows[3, :4] = rows[1, :4] + F32(5)
    assert _run(rows, "linear")[1].tolist() == [0, 1, 2, 4, 3]
    assert _run(rows, "hard")[1].tolist() == [0, 1, 2, 4]
    # -0 and +0 are equal scores
    z = np.concatenate([nc.filler(2), np.array([[-0.0], [0.0]], F32)], 1).astype(F32)
    out, src = _run(z, "linear")
    assert src.tolist() == [0, 1] and not np.signbit(out[:, 4]).any()
    for c in sc.batches(64, "linear")[0]:
        if c.family == "equal":
            assert (np.diff(c.rows[:, 4]) == 0).sum() >= len(c.rows) // 2


@pytest.mark.parametrize("n", sc.SIZES)
def test_every_gaussian_case_keeps_the_margin(n):
    """Both recorded gaps above n * 2^-22 (soft_nms.py, Exactness): the device's order can then be held to the host's."""
    for batch in sc.batches(n, "gaussian"):
        assert len({len(c.rows) for c in batch}) == (3 if n >= 3 else len({n, (2 * n) // 3, n // 3}))
        for c in batch:
            assert sc.fit(c.stats, n), (c.family, n, len(c.rows), c.stats)
            assert c.stats.get("pick_gap", np.inf) > sn.margin(n) and c.stats.get("min_score_gap", np.inf) > sn.margin(n)
            stats = {}
            out, src, num = sn.soft_nms_host(c.rows, None, "gaussian", sc.NT, sc.SIGMA, sc.MIN_SCORE, stats)
            assert np.array_equal(src[0, :num[0]], c.src) and stats["decays"][0].tolist() == c.decays.tolist()


def test_postprocess_host_cuts_on_the_decayed_scores():
    # class 1: A, B, C of the hand-worked case (linear leaves 0.9, 0.7, 0.152); class 2: one box of 0.2 far away
    dets = np.zeros((3, 4, 5), F32)
    dets[1, :3] = HAND
    dets[2, 0] = [500, 500, 520, 520, 0.2]
    counts = np.array([0, 3, 1], np.int32)
    out, num = sn.postprocess_host(dets, counts, "linear", 0.3, max_per_image=0)
    assert num.tolist() == [0, 3, 1]
    out, num = sn.postprocess_host(dets, counts, "linear", 0.3, max_per_image=4)
    assert num.tolist() == [0, 3, 1]
    # the third largest of {0.9, 0.7, 0.152, 0.2} is 0.2: B, 0.8 before its decays, goes
    out, num = sn.postprocess_host(dets, counts, "linear", 0.3, max_per_image=3)
    assert num.tolist() == [0, 2, 1] and out[1, :2, 4].tolist() == [F32(0.9), F32(0.7)] and (out[1, 2:] == 0).all()


def test_options():
    assert sn.options(None) is None and sn.options("off") is None
    assert sn.options("linear") == sn.SoftNMS("linear", 0.5, 0.001)
    assert sn.options(("gaussian", 0.25, 0.01)) == sn.SoftNMS("gaussian", 0.25, 0.01)
    assert sn.options(sn.SoftNMS("hard")) == sn.SoftNMS("hard", 0.5, 0.001)
    with pytest.raises(ValueError):
        sn.options("quadratic")
    with pytest.raises(ValueError):
        sn.options(("gaussian", 0.0, 0.001))


# ---------------------------------------------------------------------------------------------- the planner (csrc/roi_plan.h)
@pytest.fixture(scope="module")
def lib():
    from i2vsgg_amd import build
    build.build()
    from i2vsgg_amd import _lib
    return _lib.lib


def _plan(lib, n_set, n, rc=0):
    out = (ctypes.c_int32 * 7)()
    assert lib.i2v_soft_nms_plan(n_set, n, out, 7) == rc, lib.i2v_last_error()
    return list(out)


def test_soft_nms_plans(lib):
    # status, form (0 WAVE, 1 BLOCK), waves, rows per lane, grid, threads, dynamic LDS
    assert _plan(lib, 1, 1) == [0, 0, 1, 1, 1, 64, 16]
    assert _plan(lib, 3, 64) == [0, 0, 1, 1, 3, 64, 1024]
    assert _plan(lib, 3, 65) == [0, 0, 1, 2, 3, 64, 1040]
    assert _plan(lib, 1, 128)[3] == 2 and _plan(lib, 1, 129)[3] == 4 and _plan(lib, 1, 256)[3] == 4
    assert _plan(lib, 35, 300) == [0, 0, 1, 5, 35, 64, 4800]                  # the test loop: 300 rois, 36 classes
    assert _plan(lib, 1, 320)[3] == 5 and _plan(lib, 1, 321)[3] == 8
    assert _plan(lib, 1, 512) == [0, 0, 1, 8, 1, 64, 8192]
    assert _plan(lib, 1, 513) == [0, 1, 16, 1, 1, 1024, 513 * 16 + 256]
    assert _plan(lib, 2, 1024)[1:4] == [1, 16, 1] and _plan(lib, 2, 1025)[1:4] == [1, 16, 2]
    assert _plan(lib, 1, 2048)[3] == 2 and _plan(lib, 1, 2049)[3] == 4
    assert _plan(lib, 1, 4096) == [0, 1, 16, 4, 1, 1024, 65536 + 256]
    assert _plan(lib, 1, 4097)[0] == 1                                       # a status, as the entry point's refusal
    for n in range(1, 4097, 7):                                              # every row has a register
        p = _plan(lib, 1, n)
        assert p[0] == 0 and p[3] * p[5] >= n and p[3] in (1, 2, 4, 5, 8) and p[5] == 64 * p[2] and p[6] >= 16 * n
    out = (ctypes.c_int32 * 7)()
    assert lib.i2v_soft_nms_plan(1, 100, out, 6) == -1 and b"I2V_SOFT_NMS_PLAN_FIELDS" in lib.i2v_last_error()
    assert lib.i2v_soft_nms_plan(0, 100, out, 7) == -1


def test_the_entry_point_refuses_what_the_plan_refuses(lib):
    """Argument checks only: nothing is launched, the pointers are never read."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.i2v_soft_nms(p, None, 1, 4097, 1, 0.3, 0.5, 0.001, p, p, p, None, 0, None) == -1
    assert lib.i2v_last_error() == b"soft_nms: at most 4096 rows per set"
    assert lib.i2v_soft_nms_workspace_bytes(35, 300) == 0
    # the post-processing entries refuse the same before their first launch
    soft = lambda R, method, sigma: lib.i2v_det_postprocess_soft(p, p, p, 0, None, None, 600.0, 1000.0, 1.0, R, 5, 0.0, 0.3, 100, method,
                                                                 sigma, 0.001, p, p, None, 0, None)
    assert soft(4097, 1, 0.5) == -1 and lib.i2v_last_error() == b"soft_nms: at most 4096 rows per set"
    assert soft(300, 3, 0.5) == -1 and b"method" in lib.i2v_last_error()
    assert soft(300, 2, 0.0) == -1 and b"sigma" in lib.i2v_last_error()
    assert soft(300, 1, 0.5) == -3 and b"workspace" in lib.i2v_last_error()          # accepted as far as the workspace check
    assert lib.i2v_det_postprocess_soft_info(p, p, p, 0, None, None, p, 4097, 5, 0.0, 0.3, 100, 1, 0.5, 0.001, p, p, None, 0, None) == -1
    assert lib.i2v_version() >= 111
