"""Trajectory mAP of object tracks, host side (no GPU): the hand-worked answers, the conversions from Seq-NMS's result and from
per-frame annotations, the packer's limits, the metric, the command line, and the reference's own eval_detection_scores / viou
on gap-free trajectories (tests/golden/track_eval.npz, tools/gen_golden.py gen_track_eval)."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqnms_cases  # noqa: E402
import track_eval_cases as cases  # noqa: E402
from conftest import golden, record_margin  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_OV_REL = 1e-12        # the reference adds in list order, the host form in lane order: a few ulps of a sum of <= 100 terms


@pytest.fixture(scope="module")
def batch():
    """The generated batch with the host form's answer; nobody writes to either."""
    from i2vsgg_amd import track_eval
    prediction, groundtruth = cases.batch()
    return (prediction, groundtruth) + track_eval.match(prediction, groundtruth, cases.THRESHOLDS)


# ---------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_worked_cases(name):
    from i2vsgg_amd import track_eval
    pk, vol, ov, hit, hit_ov = track_eval.match(*cases.hand(name), thresholds=cases.THRESHOLDS)
    cases.check_hand(name, pk, ov, hit)
    assert np.array_equal(hit_ov >= 0, hit >= 0)
    areas = [100.0 if tr["boxes"][0] != cases.HALF else 50.0 for tr in cases.HAND[name]["pred"]]
    want = sorted(a * len(tr["frames"]) for a, tr in zip(areas, cases.HAND[name]["pred"]))
    assert sorted(vol[:pk.n_pred].tolist()) == want


def test_lane_sum_is_the_stated_order():
    """Lane l adds x[l], x[l + 64], ...; then the partials in lane order -- written out again in Python floats."""
    from i2vsgg_amd import track_eval
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 65, 129, 300):
        x = rng.uniform(0, 1e4, n)
        part = [0.0] * 64
        for i in range(n):
            part[i % 64] += float(x[i])
        total = 0.0
        for v in part:
            total += v
        assert track_eval._lane_sum(x) == total
    x = rng.uniform(0, 1e4, 300)
    assert track_eval._lane_sum(x) != float(np.sum(x)) or track_eval._lane_sum(x[::-1]) != track_eval._lane_sum(x)  # an order, not a set


def test_batch_holds_every_edge_and_the_matching_is_greedy(batch):
    prediction, groundtruth, pk, vol, ov, hit, hit_ov = batch
    cases.check_batch_facts(pk, hit)
    n_gt = np.diff(pk.cell_gt_off)
    for c in range(len(pk.cells)):                               # the rules again, cell by cell, in plain Python
        p0, p1 = int(pk.cell_pred_off[c]), int(pk.cell_pred_off[c + 1])
        assert (ov[p0:p1, :n_gt[c]] >= 0).all() and (ov[p0:p1, :n_gt[c]] <= 1).all() and (ov[p0:p1, n_gt[c]:] == -1).all()
        order = sorted(range(p0, p1), key=lambda p: -pk.pred_score[p])
        for k, thr in enumerate(cases.THRESHOLDS):
            taken = set()
            for p in order:
                best, arg = -1.0, -1
                for g in range(n_gt[c]):
                    if g not in taken and ov[p, g] >= thr and ov[p, g] > best:
                        best, arg = ov[p, g], g
                assert hit[k, p] == arg and hit_ov[k, p] == best
                taken.add(arg)


def test_gap_free_overlap_is_the_relation_metrics_viou(batch):
    """For gap-free trajectories the rule is the reference's viou: video._viou computes it from durations (numpy's own
    summation order: equal to a few ulps)."""
    from i2vsgg_amd import video
    prediction, groundtruth, pk, vol, ov, hit, hit_ov = batch
    checked = 0
    for c in range(len(pk.cells)):
        for p in range(int(pk.cell_pred_off[c]), int(pk.cell_pred_off[c + 1])):
            for g in range(int(pk.cell_gt_off[c]), int(pk.cell_gt_off[c + 1])):
                a0, a1, b0, b1 = (int(x) for x in (pk.traj_off[p], pk.traj_off[p + 1], pk.traj_off[pk.n_pred + g], pk.traj_off[pk.n_pred + g + 1]))
                fa, fb = pk.frame[a0:a1], pk.frame[b0:b1]
                if (np.diff(fa) != 1).any() or (np.diff(fb) != 1).any():
                    continue
                pr = [0, 0, 0, 0, fa[0], fa[-1] + 1, a0, a1 - a0, a0, a1 - a0]
                gr = [0, 0, 0, 0, fb[0], fb[-1] + 1, b0, b1 - b0, b0, b1 - b0]
                want = video._viou(pr, gr, 6, pk.box, vol[p], vol[pk.n_pred + g])
                assert abs(ov[p, g - int(pk.cell_gt_off[c])] - want) <= 1e-13 * max(want, 1e-300)
                checked += 1
    assert checked > 300


def test_stats_report_the_margins():
    from i2vsgg_amd import track_eval
    st = {}
    track_eval.match(*cases.hand("three_quarters"), thresholds=cases.THRESHOLDS, stats=st)
    assert st["ov"] == pytest.approx(0.05 / 0.7) and "ov_gap" not in st
    pred = {"v": [cases._t(1, [0, 1, 2, 3], score=0.5)]}
    gt = {"v": [cases._t(1, [0, 1, 2]), cases._t(1, [0, 1, 2, 3])]}                 # 0.75 and 1.0 to choose from at 0.5 and 0.7
    st = {}
    pk, vol, ov, hit, hit_ov = track_eval.match(pred, gt, cases.THRESHOLDS, stats=st)
    assert st["ov_gap"] == 0.25 and hit[:, 0].tolist() == [1, 1, 1]


# ---------------------------------------------------------------------------------------------------------------------
# conversions
# ---------------------------------------------------------------------------------------------------------------------
def test_from_seq_nms_round_trip():
    """Every surviving box of Seq-NMS's result is in exactly one trajectory, at its frame number, with its score."""
    from i2vsgg_amd import seqnms, track_eval
    all_boxes, frame_index = seqnms_cases.device_batch()
    out, tracks = seqnms.seq_nms(all_boxes, frame_index, device=None)
    trajs = track_eval.from_seq_nms(out, tracks, frame_index)
    assert set(trajs) == set(v for v, _ in frame_index)
    seen = {}
    for vid, lst in trajs.items():
        assert [(t["category"], t["tid"]) for t in lst] == sorted((t["category"], t["tid"]) for t in lst)
        for t in lst:
            assert t["frames"] == sorted(set(t["frames"])) and len(t["boxes"]) == len(t["frames"])
            for f, b in zip(t["frames"], t["boxes"]):
                seen[(vid, f, t["category"], t["tid"])] = (b, t["score"])
    n = 0
    for j in range(len(out)):
        for i, (vid, fno) in enumerate(frame_index):
            c = np.asarray(out[j][i], np.float32).reshape(-1, 5)
            for r in range(len(c)):
                b, s = seen[(vid, fno, j, int(tracks[j][i][r]))]
                assert b == [float(x) for x in c[r, :4]] and np.float32(s) == c[r, 4]
                n += 1
    assert n == len(seen) > 1000
    lens = [len(t["frames"]) for lst in trajs.values() for t in lst]
    long = track_eval.from_seq_nms(out, tracks, frame_index, min_len=5)
    assert sum(len(lst) for lst in long.values()) == sum(1 for x in lens if x >= 5) > 0 and min(lens) < 5
    track_eval.pack(trajs, trajs)                                # what it returns is what pack takes
    bad = [[np.array(c, np.float32).reshape(-1, 5) for c in row] for row in out]
    vid, t = next((vid, t) for vid, lst in trajs.items() for t in lst if len(t["frames"]) > 1)
    i = frame_index.index((vid, t["frames"][0]))                 # one member of a longer track gets another score
    bad[t["category"]][i][list(tracks[t["category"]][i]).index(t["tid"]), 4] += 0.125
    with pytest.raises(AssertionError, match="do not share one score"):
        track_eval.from_seq_nms(bad, tracks, frame_index)


def test_from_frame_annotations_round_trip():
    """tracked_boxes.pkl of a one-class video and back: the tracks Seq-NMS made, box for box."""
    from i2vsgg_amd import seqnms, track_eval
    frame_no = list(range(3, 40))
    all_boxes, frame_index = seqnms_cases.nested([("a", frame_no, {1: seqnms_cases.gen_cells(np.random.default_rng(8), 37, n_obj=4, clutter=3)})], 2)
    out, tracks = seqnms.seq_nms(all_boxes, frame_index, device=None)
    names = ["%06d.jpg" % f for f in frame_no]
    anno = seqnms.to_annotations(out, tracks, names, min_score=0.0, max_per_class=64)
    index = dict(zip(names, frame_index))
    got = track_eval.from_frame_annotations(anno, index)
    assert track_eval.from_frame_annotations(anno, index.__getitem__) == got
    want = track_eval.from_seq_nms(out, tracks, frame_index)
    key = lambda t: t["tid"]
    assert len(got["a"]) == len(want["a"]) > 4
    for g, w in zip(sorted(got["a"], key=key), sorted(want["a"], key=key)):
        assert g["category"] == w["category"] == 1 and g["frames"] == w["frames"] and g["boxes"] == w["boxes"]
    res = track_eval.evaluate(want, got)
    assert res["mAP_at"] == {"0.5": 1.0, "0.7": 1.0, "0.9": 1.0}
    # a tid that changes its class, and a tid twice in one frame, name the frame
    broken = dict((k, dict(v)) for k, v in anno.items())
    last = [n for n in names if 0 in anno[n]["tids"]][-1]
    broken[last]["box_classes"] = [7 if t == 0 else c for c, t in zip(anno[last]["box_classes"], anno[last]["tids"])]
    with pytest.raises(ValueError, match="tid 0 of video 'a' changes its class from 1 to 7 in frame %r" % last):
        track_eval.from_frame_annotations(broken, index)
    twice = dict((k, dict(v)) for k, v in anno.items())
    twice[last] = {"boxes": [[0, 0, 5, 5], [1, 1, 6, 6]], "box_classes": [1, 1], "tids": [0, 0]}
    with pytest.raises(ValueError, match="two boxes in frame %r" % last):
        track_eval.from_frame_annotations(twice, index)


def test_frame_index_of_paths_is_the_tools_rule():
    from i2vsgg_amd import seqnms
    paths = ["d/b.jpg", "d/a.jpg", "d/c.jpg", "d/e.jpg", "d/d.jpg"]
    assert seqnms.frame_index_of_paths(paths, 2) == {"d/a.jpg": ("0", 0), "d/b.jpg": ("0", 1), "d/c.jpg": ("1", 0), "d/d.jpg": ("1", 1),
                                                     "d/e.jpg": ("2", 0)}
    assert seqnms.frame_index_of_paths(paths)["d/e.jpg"] == ("0", 4) and seqnms.frame_index_of_paths([]) == {}


# ---------------------------------------------------------------------------------------------------------------------
# limits and malformed input
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_refuses_what_the_kernels_cannot_take():
    from i2vsgg_amd import track_eval
    t = cases._t
    one = {"v": [t(1, [0, 1])]}
    with pytest.raises(ValueError, match=r"cell \('v', 1\) has 4097 ground-truth trajectories, at most 4096"):
        track_eval.pack({}, {"v": [t(1, [0])] * 4097})
    track_eval.pack({}, {"v": [t(1, [0])] * 4096})
    long = {"category": 1, "frames": np.arange(2 ** 20 + 1), "boxes": np.zeros((2 ** 20 + 1, 4), np.float32)}
    with pytest.raises(ValueError, match=r"ground truth 0 of cell \('v', 1\) has 1048577 frames, at most 1048576"):
        track_eval.pack({}, {"v": [long]})
    with pytest.raises(ValueError, match=r"the frames of prediction 0 of cell \('v', 1\) are not strictly ascending"):
        track_eval.pack({"v": [t(1, [0, 2, 2], score=0.5)]}, one)
    with pytest.raises(ValueError, match=r"prediction 0 of cell \('v', 1\) has 2 frames and 1 boxes"):
        track_eval.pack({"v": [dict(t(1, [0, 1], score=0.5), boxes=[cases.B])]}, one)
    with pytest.raises(ValueError, match=r"ground truth 0 of cell \('v', 1\) has 0 frames"):
        track_eval.pack({}, {"v": [t(1, [])]})
    with pytest.raises(ValueError, match=r"prediction 0 of cell \('v', 1\) holds a box that is not finite or has x2 < x1"):
        track_eval.pack({"v": [t(1, [0], [0, 0, np.nan, 5], score=0.5)]}, one)
    with pytest.raises(ValueError, match="x2 < x1"):
        track_eval.pack({"v": [t(1, [0], [5, 0, 4, 5], score=0.5)]}, one)
    with pytest.raises(ValueError, match=r"prediction 0 of cell \('v', 1\) has a score that is not finite"):
        track_eval.pack({"v": [t(1, [0], score=float("nan"))]}, one)


def test_pack_layout_and_float32_widens_exactly():
    from i2vsgg_amd import track_eval
    b32 = np.array([[0.1, 0.2, 10.3, 10.4]], np.float32)
    pred = {"v": [{"category": 2, "score": 0.5, "frames": [4], "boxes": b32}, {"category": 1, "score": 0.25, "frames": [4], "boxes": b32.tolist()}],
            "w": [cases._t(1, [0], score=0.5)], "x": [cases._t(1, [0], score=0.5)]}
    gt = {"w": [], "v": [cases._t(1, [3, 4, 9])]}                # w has no ground truth, x is not annotated: neither takes part
    pk = track_eval.pack(pred, gt)
    assert pk.cells == [("v", 1), ("v", 2)] and (pk.n_pred, pk.n_gt) == (2, 1)
    assert pk.cell_pred_off.tolist() == [0, 1, 2] and pk.cell_gt_off.tolist() == [0, 1, 1] and pk.traj_off.tolist() == [0, 1, 2, 5]
    assert pk.frame.tolist() == [4, 4, 3, 4, 9] and pk.pred_src.tolist() == [1, 0] and pk.pred_score.tolist() == [0.25, 0.5]
    assert pk.box.dtype == np.float64 and np.array_equal(pk.box[1], b32[0].astype(np.float64)) and np.array_equal(pk.box[0], pk.box[1])
    assert pk.traj_off.dtype == pk.frame.dtype == pk.cell_pred_off.dtype == pk.cell_gt_off.dtype == np.int32
    empty = track_eval.pack({}, {})
    assert empty.cells == [] and track_eval.match_arrays_host(empty)[1].shape == (0, 0)


def test_a_device_is_refused_not_served_by_the_host_form():
    """The library has no kernel for these tables: asking for a device is an error, never a quiet host run."""
    from i2vsgg_amd import track_eval
    pred, gt = cases.hand("identical")
    for call in (lambda: track_eval.match(pred, gt, device="cuda:0"), lambda: track_eval.evaluate(pred, gt, device="cuda:0"),
                 lambda: track_eval.match_arrays(track_eval.pack(pred, gt), device="cpu")):
        with pytest.raises(NotImplementedError, match="no device form"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------------------------------
def test_metric_sanity_pair(batch):
    """Ground truth fed back as predictions: mAP 1 at every threshold; every box shifted off its object: 0."""
    from i2vsgg_amd import track_eval
    groundtruth = batch[1]
    rng = np.random.default_rng(0)
    as_pred = lambda shift: dict((vid, [dict(t, score=float(rng.random()), boxes=np.asarray(t["boxes"], np.float64) + shift) for t in lst])
                                 for vid, lst in groundtruth.items())
    res = track_eval.evaluate(as_pred(0.0), groundtruth)
    assert res["mAP"] == 1.0 and set(res["mAP_at"].values()) == {1.0} and set(res["recall_at"].values()) == {1.0}
    assert all(v is None or v == [1.0, 1.0, 1.0] for v in res["ap"].values())
    for b in res["recall_by_length"].values():
        assert b["n_gt"] > 0 and set(b["recall_at"].values()) == {1.0}
    res = track_eval.evaluate(as_pred(1000.0), groundtruth)
    assert res["mAP"] == 0.0 and set(res["mAP_at"].values()) == {0.0} and set(res["recall_at"].values()) == {0.0}
    json.dumps(res)


def test_seq_nms_tracks_beat_the_same_boxes_as_one_frame_tracks():
    """seqnms_cases.device_batch through Seq-NMS (host form), from_seq_nms, evaluate, against the objects the generator
    planted: better at 0.5 than the same boxes as one-frame tracks -- the point of the stage, and what frame-level mAP cannot see."""
    from i2vsgg_amd import seqnms, track_eval
    all_boxes, frame_index, groundtruth = cases.seqnms_batch_with_groundtruth()
    again, index_again = seqnms_cases.device_batch()
    assert frame_index == index_again
    for j in range(len(all_boxes)):                              # the replay is the generator's batch, box for box
        for i in range(len(frame_index)):
            assert np.array_equal(np.asarray(all_boxes[j][i]), np.asarray(again[j][i]))
    out, tracks = seqnms.seq_nms(all_boxes, frame_index, device=None)
    trajs = track_eval.from_seq_nms(out, tracks, frame_index)
    res = track_eval.evaluate(trajs, groundtruth)
    single = track_eval.from_seq_nms(out, cases.one_frame_tracks(out, frame_index), frame_index)
    base = track_eval.evaluate(single, groundtruth)
    assert base["n_pred_total"] == sum(len(t["frames"]) for lst in trajs.values() for t in lst) > res["n_pred_total"] > 300
    assert res["n_gt_total"] == base["n_gt_total"] > 40 and res["n_videos"] == 7
    assert res["mAP_at"]["0.5"] > base["mAP_at"]["0.5"] and res["recall_at"]["0.5"] > base["recall_at"]["0.5"]


def test_evaluate_on_a_hand_worked_set():
    """Class 1: two ground truths (2 and 40 frames), predictions scored 0.9 (exact), 0.8 (a false positive), 0.7 (0.75 of the
    long one); class 2 has predictions only and stays out of the mean; class 3 has a ground truth and no prediction."""
    from i2vsgg_amd import track_eval
    t = cases._t
    gt = {"v": [t(1, [0, 1]), t(1, range(40)), t(3, range(200))], "u": []}
    pred = {"v": [t(1, range(30), score=0.7), t(1, [0, 1], cases.FAR, score=0.8), t(1, [0, 1], score=0.9), t(2, [0], score=0.99)],
            "u": [t(1, [0], score=1.0)]}
    res = track_eval.evaluate(pred, gt, thresholds=(0.5, 0.7, 0.9), length_buckets=(32, 128))
    # at 0.5 and 0.7: tp fp tp -> precision 1, 1/2, 2/3 at recall 1/2, 1/2, 1: AP = 1/2 * 1 + 1/2 * 2/3; at 0.9: tp fp fp: 1/2
    assert res["ap"]["1"] == pytest.approx([0.5 + 1.0 / 3.0, 0.5 + 1.0 / 3.0, 0.5], abs=1e-7)
    assert res["ap"]["2"] is None and res["ap"]["3"] == [0.0, 0.0, 0.0] and res["classes"] == ["1", "3", "2"]
    assert res["n_gt"] == {"1": 2, "3": 1, "2": 0} and res["n_pred"] == {"1": 3, "3": 0, "2": 1} and res["n_videos"] == 1
    assert res["mAP_at"]["0.5"] == pytest.approx((0.5 + 1.0 / 3.0) / 2, abs=1e-7) and res["mAP_at"]["0.9"] == pytest.approx(0.25)
    assert res["mAP"] == pytest.approx(np.mean(list(res["mAP_at"].values())))
    assert res["recall_at"] == {"0.5": 2.0 / 3.0, "0.7": 2.0 / 3.0, "0.9": 1.0 / 3.0}
    by = res["recall_by_length"]
    assert list(by) == ["<32", "32..127", ">=128"] and [b["n_gt"] for b in by.values()] == [1, 1, 1]
    assert by["<32"]["recall_at"] == {"0.5": 1.0, "0.7": 1.0, "0.9": 1.0} and by["32..127"]["recall_at"] == {"0.5": 1.0, "0.7": 1.0, "0.9": 0.0}
    assert by[">=128"]["recall_at"] == {"0.5": 0.0, "0.7": 0.0, "0.9": 0.0}
    other = track_eval.evaluate(pred, gt, thresholds=(0.75, 0.76), length_buckets=(2, 3, 41))
    assert other["ap"]["1"][0] > other["ap"]["1"][1] and list(other["recall_by_length"]) == ["<2", "2..2", "3..40", ">=41"]
    assert [b["n_gt"] for b in other["recall_by_length"].values()] == [0, 1, 1, 1]
    assert other["recall_by_length"]["<2"]["recall_at"] == {"0.75": None, "0.76": None}


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own functions
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_reference_matching():
    """The reference's eval_detection_scores with viou on single trajectories: the same predictions hit, with the same ov to
    1e-12 (the reference adds in list order; the integer cases are exact and agree in every bit)."""
    from i2vsgg_amd import track_eval
    g = golden("track_eval")
    assert len(g["seeds"]) == cases.GOLDEN_CASES and tuple(g["thresholds"]) == cases.THRESHOLDS
    worst, m_ov, m_gap = 0.0, np.inf, np.inf
    for k, seed in enumerate(g["seeds"]):
        integer = k % 2 == 0
        st = {}
        pk, vol, ov, hit, hit_ov = track_eval.match(*cases.golden_case(int(seed), integer), thresholds=cases.THRESHOLDS, stats=st)
        p0, p1 = int(g["pred_off"][k]), int(g["pred_off"][k + 1])
        want_hit, want_ov = g["hit"][:, p0:p1], g["hit_ov"][:, p0:p1]
        assert pk.n_pred == p1 - p0 and np.array_equal(hit >= 0, want_hit), k
        assert np.array_equal(np.isnan(want_ov), ~want_hit)
        rel = np.abs(hit_ov[want_hit] - want_ov[want_hit]) / want_ov[want_hit]
        if integer:
            assert (rel == 0).all(), k
        else:
            assert st.get("ov", np.inf) == g["margin_ov"][k] and st.get("ov_gap", np.inf) == g["margin_ov_gap"][k]
            assert min(g["margin_ov"][k], g["margin_ov_gap"][k]) >= g["margin_bound"] == 1e-9
            m_ov, m_gap = min(m_ov, g["margin_ov"][k]), min(m_gap, g["margin_ov_gap"][k])
        worst = max(worst, rel.max() if len(rel) else 0.0)
    record_margin("test_golden_reference_matching", "hit ov vs the reference, largest rel. difference", worst, GOLDEN_OV_REL)
    record_margin("test_golden_reference_matching", "float32 cases: smallest rel. margin of an ov to a threshold (at least)", m_ov, 1e-9)
    record_margin("test_golden_reference_matching", "float32 cases: smallest rel. gap of two rival ov (at least)", m_gap, 1e-9)
    assert worst <= GOLDEN_OV_REL
    assert g["hit"][0].sum() > g["hit"][1].sum() > g["hit"][2].sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# scripts
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_tracks_script_on_the_host(tmp_path, capsys):
    """tracks.json + a per-frame pickle with tids (and a trajectory .json) -> the table, the summary line and track_eval.json."""
    sys.path.insert(0, ROOT)
    import eval_tracks
    from i2vsgg_amd import track_eval
    names = ["%04d.jpg" % k for k in range(12)]                  # 2 videos of 6 frames
    anno = dict((n, {"boxes": [], "box_classes": [], "tids": [], "rels": []}) for n in names)
    for k, n in enumerate(names):
        x = 3.0 * (k % 6)
        anno[n]["boxes"].append([x, 0.0, x + 19.0, 19.0]), anno[n]["box_classes"].append(1), anno[n]["tids"].append(0)
        if k % 6 != 2:                                           # tid 1 leaves for one frame
            anno[n]["boxes"].append([100.0, x, 129.0, x + 29.0]), anno[n]["box_classes"].append(2), anno[n]["tids"].append(1)
    tracks = {"0": [{"category": 1, "score": 0.9, "frames": list(range(6)), "boxes": [[3.0 * f, 0.0, 3.0 * f + 19.0, 19.0] for f in range(6)]},
                    {"category": 2, "score": 0.8, "frames": [0, 1], "boxes": [[100.0, 0.0, 129.0, 29.0], [100.0, 3.0, 129.0, 32.0]]}],
              "1": [{"category": 1, "score": 0.7, "frames": [0, 1, 2], "boxes": [[3.0 * f, 0.0, 3.0 * f + 19.0, 19.0] for f in range(3)]}]}
    with open(tmp_path / "annotations.pkl", "wb") as f:
        pickle.dump(anno, f)
    with open(tmp_path / "tracks.json", "w") as f:
        json.dump(tracks, f)
    res = eval_tracks.main(["--tracks", str(tmp_path / "tracks.json"), "--groundtruth", str(tmp_path / "annotations.pkl"),
                            "--frames_per_video", "6", "--cpu", "--out", str(tmp_path / "out" / "track_eval.json")])
    out = capsys.readouterr().out
    assert "AP@0.5" in out and "trajectory mAP" in out and "2 videos, 3 predictions, 4 ground truths" in out
    # class 1: exact (ov 1) and half (ov 0.5): AP 1 at 0.5, 1/2 above; class 2: 2 of 5 frames (0.4) and nothing: 0
    assert res["ap"] == {"1": [1.0, 0.5, 0.5], "2": [0.0, 0.0, 0.0]} and res["mAP_at"] == {"0.5": 0.5, "0.7": 0.25, "0.9": 0.25}
    with open(tmp_path / "out" / "track_eval.json") as f:
        assert json.load(f) == res
    gts = eval_tracks.load_groundtruth(str(tmp_path / "annotations.pkl"), frames_per_video=6)
    assert [t["frames"] for t in gts["0"]] == [[0, 1, 2, 3, 4, 5], [0, 1, 3, 4, 5]]
    with open(tmp_path / "gt.json", "w") as f:
        json.dump(gts, f)
    again = eval_tracks.main(["--tracks", str(tmp_path / "tracks.json"), "--groundtruth", str(tmp_path / "gt.json"), "--cpu",
                              "--thresholds", "0.4", "0.5"])
    assert again["ap"] == {"1": [1.0, 1.0], "2": [0.5, 0.0]} and track_eval.evaluate(tracks, gts, (0.4, 0.5)) == again


def test_track_detections_writes_and_scores_tracks(tmp_path, capsys):
    """--save_tracks writes tracks.json beside the pickles; --groundtruth prints the table right after linking.  Tracks scored
    against the annotations made from themselves: mAP 1."""
    sys.path.insert(0, ROOT)
    import eval_tracks
    import track_detections
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    imdb = get_imdb("synthetic_16_v")
    n = len(imdb.roidb)
    rng = np.random.default_rng(0)
    all_boxes = [[[] for _ in range(n)] for _ in range(imdb.num_classes)]
    e0 = imdb.roidb[0]
    j = int(e0["gt_classes"][0])                                 # one class, so that a tid names one object of a video
    for i in range(n):
        rows = [list(e0["boxes"][0].astype(np.float32) + rng.uniform(-2, 2, 4)) + [rng.uniform(0.72, 1.0)]]
        all_boxes[j][i] = np.asarray(rows, np.float32).reshape(-1, 5)
    det = tmp_path / "detections.pkl"
    with open(det, "wb") as f:
        pickle.dump(all_boxes, f)
    args = ["--detections", str(det), "--imdbval_name", "synthetic_16_v", "--frames_per_video", "8", "--cpu", "--min_score", "0.0"]
    plain = track_detections.main(args)
    assert "trajectory mAP" not in capsys.readouterr().out and not (tmp_path / "tracks.json").exists()
    saved = track_detections.main(args + ["--save_tracks"])
    assert "wrote %s" % (tmp_path / "tracks.json") in capsys.readouterr().out
    with open(tmp_path / "tracks.json") as f:
        tracks = json.load(f)
    assert sorted(tracks) == ["0", "1"] and all(t["category"] == j for lst in tracks.values() for t in lst)
    assert sum(len(t["frames"]) for lst in tracks.values() for t in lst) == n
    scored = track_detections.main(args + ["--groundtruth", str(tmp_path / "tracked_boxes.pkl"), "--thresholds", "0.5", "0.9"])
    out = capsys.readouterr().out
    assert "trajectory mAP 1.0000 (@0.5 1.0000  @0.9 1.0000)" in out
    for a, b in ((plain, saved), (plain, scored)):               # the return value is the same with and without the options
        assert pickle.dumps(a[2]) == pickle.dumps(b[2]) and all(np.array_equal(x, y) for r, s in zip(a[1], b[1]) for x, y in zip(r, s))
    res = eval_tracks.main(["--tracks", str(tmp_path / "tracks.json"), "--groundtruth", str(tmp_path / "tracked_boxes.pkl"),
                            "--imdbval_name", "synthetic_16_v", "--frames_per_video", "8", "--cpu"])
    assert res["mAP"] == 1.0 and res["n_videos"] == 2
