"""Video relations without a GPU: the host implementation of i2vsgg_amd.video against the reference's association() and
evaluate() (tests/golden/video_association.npz, video_eval.npz, video_eval_edges.npz; tools/gen_golden.py --only video), the
host pre-pass, the argument validation of the new C entry points."""
import copy
import ctypes

import numpy as np
import pytest

from conftest import golden, record_margin
import video_golden as vg


@pytest.fixture(scope="module")
def inputs():
    return vg.cases()


@pytest.fixture(scope="module")
def reference(inputs):
    return vg.reference_relations(golden("video_association"), inputs)


def test_host_association_matches_the_reference(inputs, reference):
    from i2vsgg_amd import video
    got = video.associate(copy.deepcopy(inputs), device=None)
    assert sum(len(r) for r in reference.values()) > 1500
    vg.assert_same_relations(got, reference, "test_host_association_matches_the_reference", record_margin)


def test_association_returns_names_when_given():
    from i2vsgg_amd import video
    frames = {"a": [[t, [[0.5, [1.0, 2.0, 3.0], [[0.0, 0.0, 10.0, 10.0], [5.0, 5.0, 20.0, 20.0]], 7]]] for t in range(12)]}
    rel = video.associate(frames, names=(["bg", "cat", "dog", "sofa"], ["p0", "p1", "on"]))["a"]
    assert len(rel) == 1 and rel[0]["triplet"] == ["cat", "on", "sofa"] and rel[0]["duration"] == [0, 12]
    assert rel[0]["score"] == 0.5 and rel[0]["rel_idex"] == [7] * 12 and len(rel[0]["sub_traj"]) == 12


def test_fill_empty_frames_matches_the_reference(inputs):
    from i2vsgg_amd import video
    g = golden("video_association")
    stays_empty = filled = 0
    for v, vid in enumerate(g["vids"].tolist()):
        frames = sorted(inputs[vid], key=lambda f: int(f[0]))
        out = video.fill_empty_frames(inputs[vid])
        src = g["filled_src"][g["frame_off"][v]:g["frame_off"][v + 1]]
        assert len(out) == len(src)
        for i, (fno, preds) in enumerate(out):
            assert fno == frames[i][0]
            if src[i] < 0:
                assert preds == []
                stays_empty += 1
            else:
                assert preds is frames[int(src[i])][1], (vid, i)
                filled += int(src[i]) != i
    assert stays_empty >= 3 and filled >= 10


def test_host_evaluation_matches_the_reference(reference):
    from i2vsgg_amd import video
    g = golden("video_eval")
    gts = vg.groundtruth(g, reference)
    thr = float(g["viou_threshold"])
    pe, ov, hit, _ = video.match(reference, gts, thr, device=None)
    assert pe.vids == g["vids"].tolist() and (pe.pred_off == g["pred_off"]).all()
    assert (hit == g["hit"]).all()
    seen = ~np.isnan(g["ov"])
    rel = np.abs(ov[seen] - g["ov"][seen]) / np.maximum(g["ov"][seen], 1e-300)
    rel[g["ov"][seen] == ov[seen]] = 0
    record_margin("test_host_evaluation_matches_the_reference", "relative ov difference", rel.max(), 1e-12)
    assert rel.max() <= 1e-12
    mean_ap, rec, mprec = video.evaluate(reference, gts, thr, device=None)
    got = np.array([mean_ap, rec[50], rec[100], mprec[1], mprec[5], mprec[10]], np.float64)
    record_margin("test_host_evaluation_matches_the_reference", "largest metric difference", np.abs(got - g["metrics"]).max(), 1e-6)
    assert np.abs(got - g["metrics"]).max() <= 1e-6
    assert 0 < g["metrics"][0] < 1


@pytest.fixture(scope="module")
def edge_set():
    return vg.eval_edge_set(vg.EDGE_SEED, grid=True, clamped=False)


def test_host_evaluation_matches_the_reference_on_the_edges(edge_set):
    """tests/golden/video_eval_edges.npz (tools/gen_golden.py --only video_edges): the reference on a set with 150 ground
    truths in one video, duplicate annotations, tied scores and overlaps exactly on the threshold, at thresholds 0.5 and 0."""
    from i2vsgg_amd import video
    name = "test_host_evaluation_matches_the_reference_on_the_edges"
    g = golden("video_eval_edges")
    assert int(g["seed"]) == vg.EDGE_SEED
    pred, gts = edge_set
    for tag, thr in (("50", 0.5), ("00", 0.0)):
        pe, ov, hit, hit_ov = video.match(pred, gts, thr, device=None)
        vg.assert_edge_golden(g, tag, pe, ov, hit, video.evaluate(pred, gts, thr, device=None), name, record_margin)
    # worked by hand: 100 / (100 + 200 - 100), 300 / (300 + 400 - 300), touching durations
    pe, ov, hit, hit_ov = video.match(pred, gts, 0.5, device=None)
    p0 = vg.edge_rows(pe, "exact")
    assert ov[p0, 0] == 0.5 and hit[p0] == 0 and hit_ov[p0] == 0.5
    assert ov[p0 + 1, 1] == 0.75 and hit[p0 + 1] == 1
    assert ov[p0 + 2, 2] == 0.0 and hit[p0 + 2] == -1 and hit_ov[p0 + 2] == -1.0
    pe, ov, hit, hit_ov = video.match(pred, gts, 0.0, device=None)
    assert hit[p0 + 2] == 2 and hit_ov[p0 + 2] == 0.0
    pe, ov, hit, hit_ov = video.match(pred, gts, 0.75, device=None)
    assert hit[p0] == -1 and hit[p0 + 1] == 1 and hit_ov[p0 + 1] == 0.75


def test_voc_ap_both_forms():
    from i2vsgg_amd import video
    rec, prec = np.array([0.25, 0.25, 0.5, 0.75]), np.array([1.0, 0.5, 2 / 3.0, 0.75])
    assert abs(video.voc_ap(rec, prec) - (0.25 * 1.0 + 0.25 * 0.75 + 0.25 * 0.75)) < 1e-12
    # 11 points: t = 0 .. 0.2 -> 1.0; 0.3 .. 0.7 -> 0.75; 0.8 .. 1.0 -> 0
    assert abs(video.voc_ap(rec, prec, use_07_metric=True) - (3 * 1.0 + 5 * 0.75) / 11.0) < 1e-12


def test_from_frame_results():
    from i2vsgg_amd import video
    lab = np.zeros((100, 3))
    lab[:2] = [[3, 7, 5], [5, 1, 3]]
    sub, obj = np.zeros((100, 4)), np.zeros((100, 4))
    sub[:2] = [[1, 2, 30, 40], [5, 6, 70, 80]]
    obj[:2] = [[5, 6, 70, 80], [1, 2, 30, 40]]
    results = {"vid_a/000007.jpg": (lab, np.array([0.75, 0.5]), sub, obj, np.array([4, 9])),
               "vid_a/000008.jpg": (None, None, None, None, None)}
    fr = video.from_frame_results(results, lambda p: (p.split("/")[0], int(p.split("/")[1][:-4])))
    assert fr == {"vid_a": [[7, [[0.75, [3.0, 7.0, 5.0], [[1.0, 2.0, 30.0, 40.0], [5.0, 6.0, 70.0, 80.0]], 4],
                                 [0.5, [5.0, 1.0, 3.0], [[5.0, 6.0, 70.0, 80.0], [1.0, 2.0, 30.0, 40.0]], 9]]],
                            [8, []]]}
    assert video.from_frame_results(results, {"vid_a/000007.jpg": ("x", 0), "vid_a/000008.jpg": ("y", 0)}).keys() == {"x", "y"}
    assert [f[0] for f in video.from_frame_results(results)["0"]] == [0, 1]


def test_video_entry_points_validate_their_arguments():
    from i2vsgg_amd import _lib
    L, p = _lib.lib, ctypes.c_void_p(16)
    err = lambda: L.i2v_last_error()
    assert L.i2v_version() >= 101
    need = L.i2v_video_associate_workspace_bytes(3, 40, 4000)
    assert need == L.i2v_video_associate_workspace_bytes(3, 40, 4000) and need >= 4
    args = lambda **k: [k.get("frame_off", p), p, p, k.get("score", p), p, p, k.get("nv", 3), 40, k.get("np", 4000), k.get("mx", 100),
                        p, p, p, p, p, k.get("ws", p), k.get("wsb", need), None]
    assert L.i2v_video_associate(*args(frame_off=None)) == -1 and b"null" in err()
    assert L.i2v_video_associate(*args(score=None)) == -1 and b"null" in err()
    assert L.i2v_video_associate(*args(mx=101)) == -1 and b"100" in err()
    assert L.i2v_video_associate(*args(nv=-1)) == -1 and b"negative" in err()
    assert L.i2v_video_associate(*args(np=-5)) == -1 and b"negative" in err()
    assert L.i2v_video_associate(*args(wsb=need - 1)) == -1 and b"workspace" in err()
    assert L.i2v_video_associate(*args(ws=None)) == -1 and b"workspace" in err()
    need = L.i2v_video_viou_match_workspace_bytes(400, 60)
    assert need == L.i2v_video_viou_match_workspace_bytes(400, 60) >= 2 * 460 * 8
    assert L.i2v_video_viou_match_workspace_bytes(800, 60) > need
    args = lambda **k: [k.get("pred_off", p), p, p, p, p, k.get("boxes", p), 2, k.get("np", 400), 60, 9000, k.get("mp", 200),
                        k.get("mg", 30), 0.5, p, p, p, p, k.get("wsb", need), None]
    assert L.i2v_video_viou_match(*args(pred_off=None)) == -1 and b"null" in err()
    assert L.i2v_video_viou_match(*args(boxes=None)) == -1 and b"null" in err()
    assert L.i2v_video_viou_match(*args(mp=201)) == -1 and b"200" in err()
    assert L.i2v_video_viou_match(*args(mg=5000)) == -1 and b"4096" in err()
    assert L.i2v_video_viou_match(*args(np=-1)) == -1 and b"negative" in err()
    assert L.i2v_video_viou_match(*args(wsb=need - 1)) == -1 and b"workspace" in err()
