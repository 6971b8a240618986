"""Seq-NMS without a GPU: the host form of i2vsgg_amd.seqnms against hand-worked cases, a brute-force enumeration of all link
paths, a plain full-recomputation restatement of the rules and the properties a track set must have; the nested layout, the
script, and the argument checks of the C entry point (no launch happens)."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqnms_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat(frame_no, cells):
    from i2vsgg_amd import seqnms
    return seqnms.pack(*cases.nested([("v", frame_no, {1: cells})], 2))


def _one_class_group(pk):
    """Flat range of the single real group (video 0, class 1) of a two-class pack."""
    f0, f1 = int(pk.group_off[1]), int(pk.group_off[2])
    return f0, f1, int(pk.box_off[f0]), int(pk.box_off[f1])


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_worked(name):
    from i2vsgg_amd import seqnms
    pk = seqnms.pack(*cases.hand_nested(name))
    assert len(pk.group_off) == 3 and pk.box_off[pk.group_off[1]] == 0      # class 0 (background) owns slots without boxes
    tid, new, n_tracks = seqnms.seq_nms_arrays_host(pk, **cases.HAND[name].get("kwargs", {}))
    assert n_tracks[0] == 0
    f0 = int(pk.group_off[1])
    cases.check_hand(name, tid, new, n_tracks[1], pk.box_off[f0:] - pk.box_off[f0])


def test_hand_case_arithmetic():
    """The overlaps the hand-worked cases are built on, from the restated formula."""
    b = lambda x, y: [x, y, x + 20, y + 20]
    assert cases.overlap(b(0, 0), b(5, 0)) == 336.0 / 546.0 >= 0.5
    assert cases.overlap(b(0, 0), b(2, 0)) == 399.0 / 483.0 > 0.3
    assert cases.overlap(b(0, 0), b(0, 12)) == 189.0 / 693.0 <= 0.3
    assert cases.overlap(b(0, 0), b(5, 12)) == 144.0 / 738.0 < 0.5
    assert cases.overlap(b(0, 0), b(0, 0)) == 1.0 and cases.overlap(b(0, 0), b(21, 0)) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# brute force and the plain restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_first_track_is_the_brute_force_maximum():
    from i2vsgg_amd import seqnms
    groups = cases.tiny_groups(300)
    assert sum(1 for fn, _ in groups if any(b - a != 1 for a, b in zip(fn, fn[1:]))) >= 50
    checked = 0
    for frame_no, cells in groups:
        pk = _flat(frame_no, cells)
        tid, new, n_tracks = seqnms.seq_nms_arrays_host(pk)
        if len(pk.score) == 0:
            assert n_tracks[1] == 0
            continue
        want = cases.brute_force_best_sum(frame_no, cells)
        got = 0.0
        for s in pk.score[tid == 0]:                   # flat order is frame order
            got += float(s)
        assert abs(got - want) <= 1e-12 * abs(want), (frame_no, got, want)
        checked += 1
    assert checked >= 250


def test_host_form_equals_the_plain_restatement():
    """Full recomputation in every pass, scalar Python floats: the early end of a pass's recomputation changes nothing."""
    from i2vsgg_amd import seqnms
    rng = np.random.default_rng(5)
    groups = cases.tiny_groups(60, seed=99)
    groups += [(cases.frame_numbers(rng, nf, gaps), cases.gen_cells(rng, nf, n_obj=3, clutter=2))
               for nf, gaps in ((12, 0), (20, 2), (33, 1))]
    for rescore in ("avg", "max"):
        for frame_no, cells in groups:
            pk = _flat(frame_no, cells)
            tid, new, n_tracks = seqnms.seq_nms_arrays_host(pk, rescore=rescore)
            wt, ws, wk = cases.naive_seq_nms(frame_no, cells, rescore=rescore)
            assert n_tracks[1] == wk
            assert list(tid) == [x for row in wt for x in row]
            assert [np.float32(x) for x in new] == [x for row in ws for x in row]


# ---------------------------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nf,gaps", [(1, 40, 0), (2, 40, 3), (3, 90, 2)])
def test_track_properties(seed, nf, gaps):
    from i2vsgg_amd import seqnms
    rng = np.random.default_rng(seed)
    frame_no, cells = cases.frame_numbers(rng, nf, gaps), cases.gen_cells(rng, nf, n_obj=4, clutter=3)
    pk = _flat(frame_no, cells)
    link_iou, nms_iou = 0.5, 0.3
    tid, new, n_tracks = seqnms.seq_nms_arrays_host(pk, link_iou, nms_iou)
    f0, f1, p0, p1 = _one_class_group(pk)
    assert p0 == 0 and p1 == len(pk.score)
    K = int(n_tracks[1])
    assert K > 0 and tid.min() >= -1 and tid.max() == K - 1
    slot = np.repeat(np.arange(f1 - f0), np.diff(pk.box_off[f0:f1 + 1]))          # frame position of every flat box
    sums = []
    for k in range(K):
        mem = np.nonzero(tid == k)[0]
        assert len(mem) >= 1 and len(set(slot[mem])) == len(mem)                   # one box per frame
        for a, b in zip(mem, mem[1:]):
            assert slot[b] == slot[a] + 1 and frame_no[slot[b]] == frame_no[slot[a]] + 1
            assert cases.overlap(pk.box[a], pk.box[b]) >= link_iou
        s = 0.0
        for m in mem:
            s += float(pk.score[m])
        sums.append(s)
        assert (new[mem] == np.float32(s / len(mem))).all()
    for a, b in zip(sums, sums[1:]):                    # extraction order: non-increasing sums, up to n * 2^-53 rounding
        assert b <= a * (1 + 1e-12)
    assert (new[tid < 0] == pk.score[tid < 0]).all()    # a suppressed box keeps its score
    for t in range(f1 - f0):                            # survivors of a frame overlap pairwise <= nms_iou
        sv = [n for n in range(int(pk.box_off[f0 + t]), int(pk.box_off[f0 + t + 1])) if tid[n] >= 0]
        for x in range(len(sv)):
            for y in range(x + 1, len(sv)):
                assert cases.overlap(pk.box[sv[x]], pk.box[sv[y]]) <= nms_iou
    # every suppressed box overlaps, by more than nms_iou, a survivor of its frame that was taken by an earlier pass
    assert (tid < 0).any()
    for n in np.nonzero(tid < 0)[0]:
        t = slot[n]
        sv = [m for m in range(int(pk.box_off[f0 + t]), int(pk.box_off[f0 + t + 1])) if tid[m] >= 0]
        assert any(cases.overlap(pk.box[n], pk.box[m]) > nms_iou for m in sv)


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_and_public_layout_round_trip():
    from i2vsgg_amd import seqnms
    all_boxes, frame_index = cases.device_batch()
    pk = seqnms.pack(all_boxes, frame_index)
    C, n_img = len(all_boxes), len(frame_index)
    assert pk.n_classes == C == 5 and len(pk.vids) == 7 and len(pk.group_off) == 7 * C + 1
    assert len(pk.frame_no) == C * n_img and pk.box_off[-1] == len(pk.score) == len(pk.box) == len(pk.row)
    assert pk.box.dtype == np.float32 and pk.score.dtype == np.float32 and pk.box_off.dtype == np.int32
    assert np.diff(pk.box_off).max() == 64 and (np.diff(pk.box_off) >= 0).all()
    for g in range(len(pk.group_off) - 1):              # a group's frames ascend; its slots are its video's images
        f0, f1 = pk.group_off[g], pk.group_off[g + 1]
        assert (np.diff(pk.frame_no[f0:f1]) > 0).all()
        assert [frame_index[i] for i in pk.slot_image[f0:f1]] == [(pk.vids[g // C], int(n)) for n in pk.frame_no[f0:f1]]
    tid, new, n_tracks = seqnms.seq_nms_arrays_host(pk)
    out, tracks = seqnms.seq_nms(all_boxes, frame_index, device=None)
    assert len(out) == C and all(len(out[j]) == n_img for j in range(C)) and all(out[0][i] == [] for i in range(n_img))
    cells = seqnms.scatter(pk, tid, new)
    total = 0
    for j in range(1, C):
        for i in range(n_img):
            src = np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)
            if len(src) == 0:
                assert len(np.asarray(out[j][i]).reshape(-1, 5)) == 0 and len(tracks[j][i]) == 0
                continue
            t, s = cells[(j, i)]
            keep = np.nonzero(t >= 0)[0]
            keep = keep[np.argsort(-s[keep], kind="stable")]
            assert out[j][i].dtype == np.float32 and out[j][i].shape == (len(keep), 5) and tracks[j][i].dtype == np.int32
            assert (out[j][i][:, :4] == src[keep, :4]).all() and (out[j][i][:, 4] == s[keep]).all()
            assert (tracks[j][i] == t[keep]).all()
            assert (np.diff(out[j][i][:, 4]) <= 0).all()                           # descending new score
            total += len(keep)
    assert total == int((tid >= 0).sum()) > 0


def test_row_order_on_equal_scores_is_the_original_one():
    from i2vsgg_amd import seqnms
    rows = [[100, 0, 120, 20, 0.5], [0, 0, 20, 20, 0.5], [200, 0, 220, 20, 0.75], [300, 0, 320, 20, 0.5]]
    out, tracks = seqnms.seq_nms(*cases.nested([("v", [0], {1: [rows]})], 2), device=None)
    assert out[1][0][:, 0].tolist() == [200.0, 100.0, 0.0, 300.0] and tracks[1][0].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_cap_of_64_boxes_per_frame_and_class(n):
    from i2vsgg_amd import seqnms
    assert seqnms.CAP == 64
    rows = [[30.0 * k, 0, 30.0 * k + 20, 20, 0.25 + k / 256.0] for k in range(n)]        # far apart: nothing suppresses
    rows[3][4] = 0.125                                                                   # the weakest, in the middle
    ab, fi = cases.nested([("v", [0], {1: [rows]})], 2)
    pk = seqnms.pack(ab, fi)
    assert len(pk.score) == min(n, 64) and (np.diff(pk.row) > 0).all()                   # packed in row order
    tid, new, _ = seqnms.seq_nms_arrays_host(pk)
    t, s = seqnms.scatter(pk, tid, new)[(1, 0)]
    assert len(t) == n
    if n <= 64:
        assert (t >= 0).all() and sorted(t.tolist()) == list(range(n))
    else:
        assert t[3] == -1 and (np.delete(t, 3) >= 0).all()                               # the 65th by score is suppressed
    out, tracks = seqnms.seq_nms(ab, fi, device=None)
    assert len(out[1][0]) == min(n, 64) and (n <= 64 or 0.125 not in out[1][0][:, 4])


def test_score_thresh_filters_before_packing():
    from i2vsgg_amd import seqnms
    # the strong box would be suppressed by nothing; the weak twin below the threshold takes no part at all
    rows = [[0, 0, 20, 20, 0.25], [2, 0, 22, 20, 0.125], [100, 0, 120, 20, 0.0625]]
    ab, fi = cases.nested([("v", [0, 1], {1: [rows, rows]})], 2)
    pk = seqnms.pack(ab, fi, score_thresh=0.1)
    assert len(pk.score) == 4 and pk.row.tolist() == [0, 1, 0, 1] and (pk.score >= 0.1).all()
    assert len(seqnms.pack(ab, fi).score) == 6
    out, tracks = seqnms.seq_nms(ab, fi, score_thresh=0.1, device=None)
    assert [len(c) for c in out[1]] == [1, 1] and out[1][0][0, 4] == 0.25
    out, tracks = seqnms.seq_nms(ab, fi, device=None)
    assert [len(c) for c in out[1]] == [2, 2] and out[1][0][:, 4].tolist() == [0.25, 0.0625]


def test_pack_refuses_what_the_rules_cannot_order():
    from i2vsgg_amd import seqnms
    ab, fi = cases.nested([("v", [0, 1], {1: [[[0, 0, 9, 9, 0.5]], [[0, 0, 9, 9, 0.5]]]})], 2)
    with pytest.raises(ValueError):
        seqnms.pack(ab, [("v", 3), ("v", 3)])
    with pytest.raises(ValueError):
        seqnms.pack(ab, fi[:1])
    ab[1][0][0, 4] = np.nan
    with pytest.raises(ValueError):
        seqnms.pack(ab, fi)
    with pytest.raises(ValueError):
        seqnms.seq_nms_arrays_host(seqnms.pack(*cases.hand_nested("avg")), rescore="median")


def test_to_annotations_cut():
    from i2vsgg_amd import seqnms
    obj = lambda s: [[0, 0, 20, 20, s]]
    two = lambda s: [[0, 0, 20, 20, s], [100, 0, 120, 20, 0.5]]
    ab, fi = cases.nested([("a", [0, 1, 2], {1: [obj(0.875)] * 3, 2: [two(0.75), obj(0.75), obj(0.75)]}),
                           ("b", [0], {1: [obj(0.9375)]})], 3)
    out, tracks = seqnms.seq_nms(ab, fi, device=None)
    names = ["f%d.jpg" % i for i in range(4)]
    anno = seqnms.to_annotations(out, tracks, names)
    assert sorted(anno) == sorted(names)
    assert anno["f0.jpg"] == {"boxes": [[0.0, 0.0, 20.0, 20.0]] * 2, "box_classes": [1, 2], "scores": [0.875, 0.75], "tids": [0, 0],
                              "rels": []}                                       # 0.5 is not > 0.7
    assert anno["f3.jpg"]["scores"] == [0.9375]
    assert seqnms.to_annotations(out, tracks, names, min_score=0.0)["f0.jpg"]["tids"] == [0, 0, 1]
    assert seqnms.to_annotations(out, tracks, names, min_score=0.0, max_per_class=1)["f0.jpg"]["tids"] == [0, 0]
    long = seqnms.to_annotations(out, tracks, names, min_score=0.0, min_len=2, frame_index=fi)
    assert long["f0.jpg"]["tids"] == [0, 0] and long["f3.jpg"]["boxes"] == []     # video b's track 0 of class 1 has one member


# ---------------------------------------------------------------------------------------------------------------------
# script
# ---------------------------------------------------------------------------------------------------------------------
def test_track_detections_script(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import eval_detections
    import track_detections
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
            all_boxes[j][i] = np.asarray(rows, np.float32).reshape(-1, 5)
    det = tmp_path / "detections.pkl"
    with open(det, "wb") as f:
        pickle.dump(all_boxes, f)
    out, tracks, anno = track_detections.main(["--detections", str(det), "--imdbval_name", "synthetic_16_v", "--frames_per_video", "8",
                                               "--cpu"])
    assert "seq-nms: 2 videos, 15 classes" in capsys.readouterr().out
    assert (tmp_path / "detections_seqnms.pkl").exists() and (tmp_path / "tracked_boxes.pkl").exists()
    res = eval_detections.main(["--detections", str(tmp_path / "detections_seqnms.pkl"), "--imdbval_name", "synthetic_16_v", "--cpu"])
    assert res is not None
    with open(tmp_path / "tracked_boxes.pkl", "rb") as f:
        anno = pickle.load(f)
    assert sorted(anno) == sorted(imdb.image_path_at(i).split("/")[-1] for i in range(n))
    kept = 0
    for a in anno.values():                             # what RelationStep._stage_pairs and forward_relation_eval read
        nb = len(a["boxes"])
        assert np.array(a["boxes"], np.float64).reshape(-1, 4).shape == (nb, 4)
        assert len(a["box_classes"]) == nb and np.asarray(a["scores"], np.float32).reshape(nb).shape == (nb,) and len(a["tids"]) == nb
        assert a["rels"] == [] and all(1 <= c < imdb.num_classes for c in a["box_classes"]) and all(s > 0.7 for s in a["scores"])
        kept += nb
    assert 0 < kept <= sum(len(c) for row in out[1:] for c in row)


# ---------------------------------------------------------------------------------------------------------------------
# C entry point
# ---------------------------------------------------------------------------------------------------------------------
def test_seqnms_entry_point_validates_its_arguments():
    from i2vsgg_amd import _lib
    L, p = _lib.lib, ctypes.c_void_p(16)
    err = lambda: L.i2v_last_error()
    assert L.i2v_version() >= 104
    need = L.i2v_seqnms_workspace_bytes(24, 300, 5000)
    assert need == L.i2v_seqnms_workspace_bytes(24, 300, 5000) >= 256 + 20 * 5000 + 20 * 300
    assert L.i2v_seqnms_workspace_bytes(24, 300, 10000) > need and L.i2v_seqnms_workspace_bytes(24, 600, 5000) > need
    args = lambda **k: [k.get("group_off", p), k.get("frame_no", p), k.get("box_off", p), k.get("box", p), p, k.get("ng", 24),
                        k.get("nf", 300), k.get("nb", 5000), 0.5, 0.3, k.get("rescore", 0), k.get("tid", p), p, k.get("nt", p),
                        k.get("ws", p), k.get("wsb", need), None]
    for name in ("group_off", "frame_no", "box_off", "box", "tid", "nt"):
        assert L.i2v_seqnms(*args(**{name: None})) == -1 and b"null" in err(), name
    for name in ("ng", "nf", "nb"):
        assert L.i2v_seqnms(*args(**{name: -1})) == -1 and b"negative" in err(), name
    assert L.i2v_seqnms(*args(rescore=2)) == -1 and b"rescore" in err()
    assert L.i2v_seqnms(*args(wsb=need - 1)) == -1 and b"workspace" in err()
    assert L.i2v_seqnms(*args(ws=None)) == -1 and b"workspace" in err()
    assert L.i2v_seqnms(*args(ng=0)) == 0                                   # nothing to do: no launch either
