"""Track stitching on the MI355X: csrc/track_stitch.hip (ops.track_stitch) against the host form of i2vsgg_amd.seqnms, bit for
bit in every output -- both evaluate the same float64 expressions in the same order on exactly widened float32 inputs, so
there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqnms_cases as cases  # noqa: E402
import stitch_cases as sc  # noqa: E402

DEV = "cuda:0"


def _device(pk, tid, **kw):
    from i2vsgg_amd import ops
    return [t.cpu().numpy() for t in ops.track_stitch(pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score, tid, device=DEV, **kw)]


@pytest.fixture(scope="module")
def batch():
    """The launch of 35 groups, packed once, with Seq-NMS's ids from the host form; nobody writes to either."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from i2vsgg_amd import seqnms
    all_boxes, frame_index = cases.device_batch()
    pk = seqnms.pack(all_boxes, frame_index)
    return all_boxes, frame_index, pk, seqnms.seq_nms_arrays_host(pk)[0]


def test_device_equals_host_form_on_the_batch(batch):
    from i2vsgg_amd import seqnms
    all_boxes, frame_index, pk, tid = batch
    assert len(pk.group_off) - 1 == 35 and len(pk.score) == 3834 and {0, 1, 63, 64} <= set(np.diff(pk.box_off).tolist())
    stats = {}
    want = seqnms.stitch_arrays_host(pk, tid, 3, 0.3, stats=stats)
    sc.same_bits(_device(pk, tid, max_gap=3, stitch_iou=0.3), want)
    assert stats["links"] >= 300 and stats["chains_of_three"] >= 20 and stats["claimed_met"] >= 20
    assert stats["links_over_absent_numbers"] >= 30 and len(want[4]) > 300
    stats = {}
    want = seqnms.stitch_arrays_host(pk, tid, 7, 0.1, stats=stats)
    sc.same_bits(_device(pk, tid, max_gap=7, stitch_iou=0.1), want)
    assert stats["multi"] >= 20


def test_other_gaps_and_max_equal_the_host_form(batch):
    from i2vsgg_amd import seqnms
    all_boxes, frame_index, pk, tid = batch
    sc.same_bits(_device(pk, tid, max_gap=1, stitch_iou=0.3), seqnms.stitch_arrays_host(pk, tid, 1, 0.3))
    tid_max = seqnms.seq_nms_arrays_host(pk, rescore="max")[0]
    want = seqnms.stitch_arrays_host(pk, tid_max, 3, 0.3, "max")
    sc.same_bits(_device(pk, tid_max, max_gap=3, stitch_iou=0.3, rescore="max"), want)
    assert not np.array_equal(want[1], seqnms.stitch_arrays_host(pk, tid_max, 3, 0.3)[1])
    none = _device(pk, tid, max_gap=7, stitch_iou=2.0)           # nothing qualifies: Seq-NMS's own answer
    seq = seqnms.seq_nms_arrays_host(pk)
    assert np.array_equal(none[0], seq[0]) and np.array_equal(none[1].view(np.uint32), seq[1].view(np.uint32))
    assert np.array_equal(none[2], seq[2]) and not none[3].any() and all(len(x) == 0 for x in none[4:])


def test_two_runs_give_the_same_bits(batch):
    all_boxes, frame_index, pk, tid = batch
    sc.same_bits(_device(pk, tid, max_gap=7, stitch_iou=0.1), _device(pk, tid, max_gap=7, stitch_iou=0.1))


def test_hand_worked_cases_on_the_device():
    from i2vsgg_amd import seqnms
    for name in sorted(sc.HAND):
        case = sc.HAND[name]
        pk = seqnms.pack(*sc.hand_nested(name))
        tid = seqnms.seq_nms_arrays(pk, device=DEV, **case.get("nms", {}))[0]
        sc.check_hand(name, tid, _device(pk, tid, **case.get("stitch", {})), pk)


def test_the_tiny_groups_in_one_launch():
    """600 groups, half of them empty (the background class of every video)."""
    from i2vsgg_amd import seqnms
    pk = seqnms.pack(*cases.tiny_nested(cases.tiny_groups(300)))
    assert len(pk.group_off) - 1 == 600
    tid = seqnms.seq_nms_arrays_host(pk)[0]
    want = seqnms.stitch_arrays_host(pk, tid)
    sc.same_bits(_device(pk, tid), want)
    assert len(want[4]) > 100


def test_public_layout_device_equals_host(batch):
    from i2vsgg_amd import seqnms
    all_boxes, frame_index, pk, tid = batch
    host = seqnms.seq_nms_stitched(all_boxes, frame_index, device=None, max_gap=3, stitch_iou=0.3)
    dev = seqnms.seq_nms_stitched(all_boxes, frame_index, device=DEV, max_gap=3, stitch_iou=0.3)
    for a, b in zip(host, dev):
        for row_a, row_b in zip(a, b):
            for x, y in zip(row_a, row_b):
                x, y = np.asarray(x), np.asarray(y)
                assert x.shape == y.shape and x.dtype == y.dtype
                assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert sum(int(m.sum()) for row in dev[2] for m in row) > 300


def test_the_wrapper_refuses_what_it_cannot_run():
    from i2vsgg_amd import ops, seqnms
    from i2vsgg_amd._lib import I2VError
    pk = seqnms.pack(*sc.hand_nested("chain3"))
    tid = seqnms.seq_nms_arrays_host(pk)[0]
    t = lambda **k: (k.get("group_off", pk.group_off), pk.frame_no, k.get("box_off", pk.box_off), pk.box, pk.score, k.get("tid", tid))
    with pytest.raises(I2VError, match="GPU only"):
        ops.track_stitch(*t(), device="cpu")
    with pytest.raises(ValueError, match="sizes"):
        ops.track_stitch(*t(box_off=pk.box_off[:-1]), device=DEV)
    with pytest.raises(ValueError, match="sizes"):
        ops.track_stitch(*t(tid=tid[:-1]), device=DEV)
    with pytest.raises(I2VError, match="max_gap lies in"):
        ops.track_stitch(*t(), max_gap=8, device=DEV)
    res = ops.track_stitch(pk.group_off[:1], pk.frame_no[:0], pk.box_off[:1], pk.box[:0], pk.score[:0], tid[:0], device=DEV)
    assert [x.numel() for x in res] == [0, 0, 0, 1, 0, 0, 0, 0] and int(res[3][0]) == 0      # no groups: nothing is launched
    twice = tid.copy()
    twice[0] = twice[1]                                          # slot 0 of group 1 holds two boxes
    with pytest.raises(I2VError, match="track_stitch: .* group 1"):
        ops.track_stitch(*t(tid=twice), device=DEV)
    sc.same_bits([x.cpu().numpy() for x in ops.track_stitch(*t(), device=DEV)], seqnms.stitch_arrays_host(pk, tid))   # and runs after it
