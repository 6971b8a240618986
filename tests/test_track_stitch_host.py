"""Track stitching without a GPU: the host form (seqnms.stitch_arrays_host) against hand-worked cases and a naive second
statement of the rules, the identity when nothing is stitched, the nested layout, the end-to-end effect on trajectory recall,
the script, and the argument checks of the C entry point (no launch happens).  No tolerance anywhere: float32 as bits."""
import ctypes
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqnms_cases as cases  # noqa: E402
import stitch_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batch():
    """``seqnms_cases.device_batch()`` packed, with Seq-NMS's answer; nobody writes to either."""
    from i2vsgg_amd import seqnms
    pk = seqnms.pack(*cases.device_batch())
    return pk, seqnms.seq_nms_arrays_host(pk)


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.HAND))
def test_hand_worked_cases(name):
    from i2vsgg_amd import seqnms
    case = sc.HAND[name]
    pk = seqnms.pack(*sc.hand_nested(name))
    tid = seqnms.seq_nms_arrays_host(pk, **case.get("nms", {}))[0]
    stats = {}
    res = seqnms.stitch_arrays_host(pk, tid, stats=stats, **case.get("stitch", {}))
    sc.check_hand(name, tid, res, pk)
    if "stats" in case:
        assert stats == case["stats"]
    assert res[0].dtype == res[2].dtype == res[3].dtype == res[4].dtype == res[5].dtype == np.int32
    assert res[1].dtype == res[6].dtype == res[7].dtype == np.float32 and res[6].shape == (len(case["fills"]), 4)


def test_nested_layout_merges_the_new_rows():
    from i2vsgg_amd import seqnms, track_eval
    ab, fi = sc.hand_nested("bridge")                            # a slot that exists but is empty gets its row
    stats = {}
    out, tracks, interp = seqnms.seq_nms_stitched(ab, fi, device=None, stats=stats)
    assert stats == {"links": 1, "added": 1}
    assert np.array_equal(out[1][1], np.array([[4, 0, 24, 20, 0.625]], np.float32)) and out[1][1].dtype == np.float32
    assert tracks[1][1].tolist() == [0] and tracks[1][1].dtype == np.int32 and interp[1][1].tolist() == [True]
    assert out[1][0][:, 4].tolist() == [0.625] and interp[1][0].tolist() == [False] and interp[1][2].tolist() == [False]
    assert out[0][1] == [] and len(tracks[0][1]) == 0 and len(interp[0][1]) == 0        # the background comes back as it came
    ab, fi = sc.hand_nested("chain3")                            # descending score: Y's real row, then X's new one
    out, tracks, interp = seqnms.seq_nms_stitched(ab, fi, device=None)
    assert np.array_equal(out[1][1], np.array([[0, 100, 20, 120, 0.875], [4, 0, 24, 20, 0.5]], np.float32))
    assert tracks[1][1].tolist() == [0, 1] and interp[1][1].tolist() == [False, True]
    assert tracks[1][0].tolist() == [0, 1] and out[1][0][:, 4].tolist() == [0.875, 0.5] and interp[1][0].tolist() == [False, False]
    # a stitched track's rows share one score: track_eval.from_seq_nms takes the result unchanged
    trajs = track_eval.from_seq_nms(out, tracks, fi)["v"]
    assert [(t["tid"], t["frames"], t["score"]) for t in trajs] == [(0, [0, 1, 2, 3, 4], 0.875), (1, [0, 1, 2, 3, 4], 0.5)]
    assert trajs[1]["boxes"] == [[0, 0, 20, 20], [4, 0, 24, 20], [8, 0, 28, 20], [12, 0, 32, 20], [16, 0, 36, 20]]
    names = ["f%d.jpg" % i for i in range(5)]
    anno = seqnms.to_annotations(out, tracks, names, min_score=0.0, interp=interp)
    assert anno["f1.jpg"] == {"boxes": [[0.0, 100.0, 20.0, 120.0], [4.0, 0.0, 24.0, 20.0]], "box_classes": [1, 1], "scores": [0.875, 0.5],
                              "tids": [0, 1], "rels": [], "interp": [False, True]}
    assert "interp" not in seqnms.to_annotations(out, tracks, names, min_score=0.0)["f1.jpg"]


def test_arguments_and_malformed_tables():
    from i2vsgg_amd import seqnms
    pk = seqnms.pack(*sc.hand_nested("chain3"))
    tid = seqnms.seq_nms_arrays_host(pk)[0]
    for bad in (0, 8, 1.5, True):
        with pytest.raises(ValueError, match="max_gap"):
            seqnms.stitch_arrays_host(pk, tid, max_gap=bad)
    with pytest.raises(ValueError, match="rescore"):
        seqnms.stitch_arrays_host(pk, tid, rescore="median")
    with pytest.raises(ValueError, match="track ids"):
        seqnms.stitch_arrays_host(pk, tid[:-1])
    twice = tid.copy()
    twice[0] = twice[1]                                          # slot 0 of group 1 holds two boxes
    with pytest.raises(ValueError, match="group 1 .*twice in slot 0"):
        seqnms.stitch_arrays_host(pk, twice)
    runs = tid.copy()
    runs[np.nonzero(tid == 3)[0]] = 2                            # X of frame 4 under the id of X of frame 0
    with pytest.raises(ValueError, match="group 1 .*not one run"):
        seqnms.stitch_arrays_host(pk, runs)
    far = tid.copy()
    far[0] = len(tid)
    with pytest.raises(ValueError, match="group 1 .*outside"):
        seqnms.stitch_arrays_host(pk, far)


# ---------------------------------------------------------------------------------------------------------------------
# identity
# ---------------------------------------------------------------------------------------------------------------------
def test_nothing_qualifies_gives_seq_nms_bit_for_bit(batch):
    from i2vsgg_amd import seqnms
    pk, (tid, new, n_tracks) = batch
    for rescore in ("avg", "max"):
        want = seqnms.seq_nms_arrays_host(pk, rescore=rescore)
        stats = {}
        res = seqnms.stitch_arrays_host(pk, want[0], max_gap=7, stitch_iou=2.0, rescore=rescore, stats=stats)
        assert np.array_equal(res[0], want[0]) and np.array_equal(res[1].view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(res[2], want[2]) and stats["links"] == 0
        assert not res[3].any() and len(res[3]) == len(pk.group_off) and all(len(x) == 0 for x in res[4:])
    ab, fi = cases.device_batch()
    plain = seqnms.seq_nms(ab, fi, device=None)
    off = seqnms.seq_nms_stitched(ab, fi, device=None, max_gap=0)
    none = seqnms.seq_nms_stitched(ab, fi, device=None, max_gap=3, stitch_iou=2.0)
    for got in (off, none):
        assert pickle.dumps(got[:2]) == pickle.dumps(plain)
        assert all(len(m) == len(t) and not m.any() for row_m, row_t in zip(got[2], got[1]) for m, t in zip(row_m, row_t))


# ---------------------------------------------------------------------------------------------------------------------
# a naive second form
# ---------------------------------------------------------------------------------------------------------------------
def test_naive_form_agrees_on_the_tiny_groups():
    from i2vsgg_amd import seqnms
    pk = seqnms.pack(*cases.tiny_nested(cases.tiny_groups(300)))
    tid = seqnms.seq_nms_arrays_host(pk)[0]
    stats = {}
    res = seqnms.stitch_arrays_host(pk, tid, stats=stats)
    assert sc.check_against_naive(pk, tid, res) > 100 and stats["links"] > 100 and stats["multi"] > 10
    kw = dict(max_gap=2, stitch_iou=0.05, rescore="max")
    sc.check_against_naive(pk, tid, seqnms.stitch_arrays_host(pk, tid, **kw), **kw)


@pytest.mark.parametrize("kw", [dict(max_gap=3, stitch_iou=0.3), dict(max_gap=7, stitch_iou=0.1), dict(max_gap=1, stitch_iou=0.3),
                                dict(max_gap=3, stitch_iou=0.3, rescore="max")], ids=["3-0.3", "7-0.1", "1-0.3", "max"])
def test_naive_form_agrees_on_the_device_batch(batch, kw):
    from i2vsgg_amd import seqnms
    pk, (tid, _, n_tracks) = batch
    res = seqnms.stitch_arrays_host(pk, tid, **kw)
    assert sc.check_against_naive(pk, tid, res, **kw) > 200
    assert int(res[2].sum()) < int(n_tracks.sum())


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_stitching_restores_trajectory_recall(seed):
    """Four objects over 48 frames, each missed for runs of 1-3 frames every 5-8 frames: no fragment reaches a vIoU of 0.5
    with its annotated trajectory, every stitched track does."""
    from i2vsgg_amd import seqnms, track_eval
    ab, fi, gts = sc.scenario(seed)
    recall = lambda out, tracks: track_eval.evaluate(track_eval.from_seq_nms(out, tracks, fi), gts, [0.5])["recall_at"]["0.5"]
    out, tracks, interp = seqnms.seq_nms_stitched(ab, fi, device=None, max_gap=3, stitch_iou=0.3)
    with_, without = recall(out, tracks), recall(*seqnms.seq_nms(ab, fi, device=None))
    print("seed %d: trajectory recall@0.5 %.3f without stitching, %.3f with" % (seed, without, with_))
    assert with_ == 1.0
    assert without < with_
    assert sum(int(m.sum()) for m in interp[1]) == sum(len(c) for c in out[1]) - sum(len(c) for c in seqnms.seq_nms(ab, fi, device=None)[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# script
# ---------------------------------------------------------------------------------------------------------------------
def _detections(tmp_path, missed=()):
    """The set-up of test_seqnms_host.test_track_detections_script; ``missed``: frame positions within a video without rows."""
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    imdb = get_imdb("synthetic_16_v")
    n = len(imdb.roidb)
    rng = np.random.default_rng(0)
    all_boxes = [[[] for _ in range(n)] for _ in range(imdb.num_classes)]
    for j in range(1, imdb.num_classes):
        for i in range(n):
            e = imdb.roidb[i]
            gt = e["boxes"][e["gt_classes"] == j].astype(np.float32)
            rows = [list(b + rng.uniform(-2, 2, 4)) + [rng.uniform(0.72, 1.0)] for b in gt]
            rows += [list(b + rng.uniform(-3, 3, 4)) + [rng.uniform(0.1, 0.6)] for b in gt[:1]]        # a weaker duplicate
            all_boxes[j][i] = np.asarray(rows if i % 8 not in missed else [], np.float32).reshape(-1, 5)
    det = tmp_path / "detections.pkl"
    with open(det, "wb") as f:
        pickle.dump(all_boxes, f)
    return imdb, all_boxes, ["--detections", str(det), "--imdbval_name", "synthetic_16_v", "--frames_per_video", "8", "--cpu"]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_script_without_the_switch_writes_what_it_wrote(tmp_path, capsys):
    """No --stitch_gap (and --stitch_gap 0): the two pickles are, byte for byte, the pickles of ``seq_nms`` and
    ``to_annotations`` as the script called them before the switch existed, and no line is added."""
    sys.path.insert(0, ROOT)
    import track_detections
    from i2vsgg_amd import seqnms
    imdb, all_boxes, args = _detections(tmp_path, missed=(3,))
    track_detections.main(args)
    printed = capsys.readouterr().out
    assert "stitch" not in printed and printed.count("\n") == 3
    with open(tmp_path / "detections.pkl", "rb") as f:
        all_boxes = pickle.load(f)                               # as the script reads them
    paths = [imdb.image_path_at(i) for i in range(len(all_boxes[0]))]
    index = seqnms.frame_index_of_paths(paths, 8)
    frame_index = [index[p] for p in paths]
    out, tracks = seqnms.seq_nms(all_boxes, frame_index, 0.5, 0.3, "avg", 0.0, device=None)
    anno = seqnms.to_annotations(out, tracks, [p.split("/")[-1] for p in paths], 0.7, 10, 1, frame_index)
    want = [pickle.dumps(obj, pickle.HIGHEST_PROTOCOL) for obj in (out, anno)]
    got = [_read(tmp_path / name) for name in ("detections_seqnms.pkl", "tracked_boxes.pkl")]
    assert got == want and all("interp" not in e for e in anno.values())
    track_detections.main(args + ["--stitch_gap", "0", "--stitch_iou", "0.1"])
    assert [_read(tmp_path / name) for name in ("detections_seqnms.pkl", "tracked_boxes.pkl")] == want
    assert "stitch" not in capsys.readouterr().out


def test_script_with_the_switch(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import track_detections
    imdb, all_boxes, args = _detections(tmp_path, missed=(3, 4))
    plain_out, plain_tracks, plain_anno = track_detections.main(args + ["--save_tracks"])
    with open(tmp_path / "tracks.json") as f:
        plain_trajs = json.load(f)
    capsys.readouterr()
    out, tracks, anno = track_detections.main(args + ["--stitch_gap", "3", "--stitch_iou", "0.3", "--save_tracks"])
    printed = capsys.readouterr().out
    count = lambda ab: sum(len(np.asarray(c).reshape(-1, 5)) for row in ab[1:] for c in row)
    line = [ln for ln in printed.split("\n") if ln.startswith("stitch:")]
    assert len(line) == 1
    links, added = [int(x) for x in re.match(r"stitch: (\d+) links .* (\d+) boxes added$", line[0]).groups()]
    assert links > 0 and added == count(out) - count(plain_out) == 2 * links     # two missed frames per bridged gap
    with open(tmp_path / "detections_seqnms.pkl", "rb") as f:
        assert count(pickle.load(f)) == count(out)
    with open(tmp_path / "tracked_boxes.pkl", "rb") as f:
        saved = pickle.load(f)
    assert pickle.dumps(saved) == pickle.dumps(anno)
    assert all(len(e["interp"]) == len(e["boxes"]) == len(e["tids"]) for e in saved.values())
    names = [imdb.image_path_at(i).split("/")[-1] for i in range(len(all_boxes[0]))]
    for i, name in enumerate(names):                             # the relation loop gets boxes in the missed frames, marked
        if i % 8 in (3, 4):
            assert plain_anno[name]["boxes"] == [] and all(saved[name]["interp"])
        else:
            assert not any(saved[name]["interp"]) and len(saved[name]["boxes"]) == len(plain_anno[name]["boxes"])
    assert sum(sum(e["interp"]) for e in saved.values()) == added
    with open(tmp_path / "tracks.json") as f:
        trajs = json.load(f)                                     # tracks.json holds the stitched tracks
    n_tr = lambda d: sum(len(v) for v in d.values())
    n_fr = lambda d: sum(len(t["frames"]) for v in d.values() for t in v)
    assert n_tr(trajs) == n_tr(plain_trajs) - links and n_fr(trajs) == n_fr(plain_trajs) + added
    assert any(3 in t["frames"] and 4 in t["frames"] for v in trajs.values() for t in v)
    assert not any(3 in t["frames"] or 4 in t["frames"] for v in plain_trajs.values() for t in v)


# ---------------------------------------------------------------------------------------------------------------------
# C entry point
# ---------------------------------------------------------------------------------------------------------------------
def test_track_stitch_entry_point_validates_its_arguments():
    from i2vsgg_amd import _lib
    L, p = _lib.lib, ctypes.c_void_p(16)
    err = lambda: L.i2v_last_error()
    assert L.i2v_version() >= 109
    need = L.i2v_track_stitch_workspace_bytes(24, 300, 5000, 3)
    assert need >= 256 + 28 * 5000 + 4 * 24 + 28 * 3 * 5000
    assert L.i2v_track_stitch_workspace_bytes(24, 300, 5000, 7) > need and L.i2v_track_stitch_workspace_bytes(24, 300, 10000, 3) > need
    names = ("group_off", "frame_no", "box_off", "box", "score", "tid")
    outs = ("tid2", "score2", "n_tracks2", "fill_off", "fill_slot", "fill_tid", "fill_box", "fill_score")
    args = lambda **k: ([k.get(n, p) for n in names] + [k.get("ng", 24), k.get("nf", 300), k.get("nb", 5000), k.get("max_gap", 3),
                        k.get("iou", 0.3), k.get("rescore", 0)] + [k.get(n, p) for n in outs] + [k.get("ws", p), k.get("wsb", need), None])
    for name in names + outs:
        assert L.i2v_track_stitch(*args(**{name: None})) == -1 and b"null" in err(), name
    assert L.i2v_track_stitch(*args(ws=None)) == -1 and b"workspace" in err()
    for gap in (0, 8, -1):
        assert L.i2v_track_stitch(*args(max_gap=gap)) == -1 and b"max_gap lies in [1, 7]" in err(), gap
    for name in ("ng", "nf", "nb"):
        assert L.i2v_track_stitch(*args(**{name: -1})) == -1 and b"negative" in err(), name
    assert L.i2v_track_stitch(*args(rescore=2)) == -1 and b"rescore" in err()
    assert L.i2v_track_stitch(*args(iou=float("nan"))) == -1 and b"not a number" in err()
    assert L.i2v_track_stitch(*args(wsb=need - 1)) == -1 and b"workspace too small" in err()
    assert L.i2v_track_stitch(*args(nb=2 ** 30, max_gap=7)) == -1 and b"int32" in err()
    assert L.i2v_track_stitch(*args(ng=0, nf=0, nb=0)) == 0                              # no groups: nothing is launched
