"""Greedy NMS on the device (i2v_nms_sorted: nms_mask_kernel and the scan kernels of csrc/nms.hip) on the built edge cases of
tests/nms_cases.py, against the oracle's nms_sorted, bit for bit: deep suppress-release chains around the sweep cap of the
fixed-point resolve, across the 1024-row super-block edge and at the hand-over to the generic scan; pairs whose IoU is the
threshold, one ulp to either side, and around the mask kernel's band; degenerate boxes.  Which regime each case lands in is
asserted on the CPU (tests/test_nms_cases_host.py).  Needs a real MI355X: `pytest -m gpu`."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import nms_cases as nc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# I2V_NMS_SCAN: 2 = the default (super-blocks, 48 fixed-point sweeps), 5 / 3 = that many sweeps (any value >= 3 is the cap:
# launch_nms), 1 = super-blocks resolved serially, 0 = the pipelined 64-row scan.  n = 12353 takes the generic scan in every form.
ALL_FORMS = (2, 5, 3, 1, 0)
TWO_FORMS = (2, 0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import ops as o
    return o


@pytest.fixture(scope="module")
def oracle():
    from oracle import cops, rpn
    return cops, rpn


@contextlib.contextmanager
def scan_form(mode):
    from i2vsgg_amd._lib import TUNE, lib
    assert lib.i2v_get_tuning(TUNE["I2V_NMS_SCAN"]) == 2
    try:
        assert lib.i2v_set_tuning(TUNE["I2V_NMS_SCAN"], mode) == 0
        yield
    finally:
        lib.i2v_set_tuning(TUNE["I2V_NMS_SCAN"], 2)
    assert lib.i2v_get_tuning(TUNE["I2V_NMS_SCAN"]) == 2


@functools.lru_cache(maxsize=None)
def _ladders():
    return {c.name: c for c in nc.ladder_cases()}


@functools.lru_cache(maxsize=None)
def _reference(kind, key):
    """The case and the oracle's keep list, computed once and shared by the scan forms."""
    from oracle import cops
    case = {"ladder": lambda: _ladders()[key], "batched": lambda: nc.batched_case()[key], "thresh": lambda: nc.threshold_case(key),
            "degenerate": lambda: nc.degenerate_cases()[key]}[kind]()
    ref = cops.nms_sorted(case.dets, case.thresh)
    ref.setflags(write=False)
    case.dets.setflags(write=False)
    return case, ref


def _check(ops, dets, thresh, refs, cap, what):
    """One launch over dets (n, 5) or (n_img, n, 5): num and keep[:num] against the oracle's lists cut at the cap."""
    keep, num = ops.nms_sorted(torch.from_numpy(np.array(dets, np.float32)).to(DEV), thresh, max_keep=cap)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    assert num.shape == (len(refs),)
    for i, ref in enumerate(refs):
        want = ref[:cap] if cap > 0 else ref
        assert int(num[i]) == want.size, (what, i, int(num[i]), want.size)
        assert np.array_equal(keep[i, :want.size], want), (what, i)


LADDER_NAMES = ["cap48_L47", "cap48_L48", "cap48_L49", "cap5_L4", "cap5_L5", "cap5_L6", "whole_super_block", "straddle",
                "three_regimes"] + ["end_n%d" % n for n in nc.END_N]


@pytest.mark.parametrize("mode", ALL_FORMS)
@pytest.mark.parametrize("name", LADDER_NAMES)
def test_ladders_and_caps(ops, name, mode):
    """Chains as deep as the sweep cap, one less and one more; a whole super-block of chain; chains over the super-block edge and up
    to the last row on both sides of every scan boundary -- uncapped and with max_keep around the first super-block's count, at 1
    and in mid-ladder."""
    assert sorted(LADDER_NAMES) == sorted(_ladders())
    case, ref = _reference("ladder", name)
    with scan_form(mode):
        for cap in nc.caps_for(case, ref):
            _check(ops, case.dets, case.thresh, [ref], cap, (name, mode, cap))


@pytest.mark.parametrize("mode", ALL_FORMS)
def test_batched_regimes(ops, mode):
    """n_img = 3 in one launch: a super-block that settles, one that falls back, filler alone."""
    cases, refs = zip(*(_reference("batched", k) for k in range(3)))
    dets = np.stack([c.dets for c in cases])
    caps = sorted({0, 1} | {c for case, ref in zip(cases, refs) for c in nc.caps_for(case, ref)})
    with scan_form(mode):
        for cap in caps:
            _check(ops, dets, nc.LADDER_THRESH, refs, cap, ("batched", mode, cap))


@pytest.mark.parametrize("mode", TWO_FORMS)
@pytest.mark.parametrize("thresh", nc.THRESHOLDS)
def test_threshold_pairs(ops, thresh, mode):
    """728 independent pairs per threshold: IoU equal to the threshold, one ulp off, inside the band of thresh (1 +- 2^-21) and just
    outside it on either side; every decision shows in the keep list on its own."""
    case, ref = _reference("thresh", thresh)
    with scan_form(mode):
        _check(ops, case.dets, thresh, [ref], 0, (thresh, mode))


@pytest.mark.parametrize("mode", TWO_FORMS)
@pytest.mark.parametrize("k", range(3))
def test_degenerate_boxes(ops, k, mode):
    """Zero-area, negative-extent, infinite and NaN boxes among ordinary ones: the oracle's answer, whatever it is."""
    case, ref = _reference("degenerate", k)
    with scan_form(mode):
        _check(ops, case.dets, case.thresh, [ref], 0, (case.name, mode))


def test_detection_postprocess_ladder(ops, oracle):
    """The product caller that batches NMS per class: 128 rois whose decode is a 60-row ladder plus filler, for three classes
    in one n_img = C - 1 launch; in the default form every image's super-block falls back to the serial resolve."""
    cops, orpn = oracle
    from i2vsgg_amd._lib import TUNE, lib
    assert lib.i2v_get_tuning(TUNE["I2V_NMS_SCAN"]) == 2
    rois, prob, pred, want_boxes, (im_h, im_w) = nc.detection_ladder()
    R, C = prob.shape
    assert np.array_equal(cops.decode_clip(rois[:, 1:], pred[:, :4], im_h, im_w), want_boxes)
    want = orpn.detection_postprocess(rois, prob, pred, im_h, im_w, 1.0, False, None, None, 0.0, nc.LADDER_THRESH, 0)
    dets, counts = ops.detection_postprocess(*(torch.from_numpy(a).to(DEV) for a in (rois, prob, pred)), im_h, im_w, 1.0,
                                             False, None, None, 0.0, nc.LADDER_THRESH, 0)
    counts, dets = counts.cpu().numpy(), dets.cpu().numpy()
    assert counts[0] == 0
    for j in range(1, C):
        assert len(want[j]) == R - 30                        # every other ladder row is gone
        assert counts[j] == len(want[j]), (j, counts[j], len(want[j]))
        assert np.array_equal(dets[j, :counts[j]], want[j]), j
    assert lib.i2v_get_tuning(TUNE["I2V_NMS_SCAN"]) == 2
