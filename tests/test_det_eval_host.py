"""Detection evaluation without a GPU: the host form of i2vsgg_amd.detection_eval against the reference's own voc_eval
(tests/golden/det_eval.npz; tools/gen_golden.py --only det_eval), the results-file quantisation against literal strings, the
offset tables, the imdb hook and the script, and the argument validation of the new C entry points."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

import det_eval_golden as dg


@pytest.fixture(scope="module")
def gold_inputs():
    return dg.golden_inputs()


def test_host_form_matches_the_reference(gold_inputs):
    from i2vsgg_amd import detection_eval as de
    g, all_boxes, roidb, classes = gold_inputs
    pk = de.pack(all_boxes, roidb, len(classes))
    assert len(pk.det_key) == len(g["det"]) and np.array_equal(pk.npos, g["npos"])
    for t, thr in enumerate(g["thresholds"]):
        flag, ovmax, jmax = de.match_arrays_host(pk, float(thr))
        cur = de.curve_arrays_host(pk, flag)
        dg.check_against_reference(g, pk, t, cur)
        if thr == 0.5:                                   # an overlap of exactly the threshold is a false positive
            assert (ovmax == 0.5).any() and (flag[ovmax == 0.5] == de.FP).all()
            assert (jmax > 63).any() and (flag == de.IGNORED).any()


def test_evaluate_returns_the_reference_numbers(gold_inputs):
    from i2vsgg_amd import detection_eval as de
    g, all_boxes, roidb, classes = gold_inputs
    res = de.evaluate(all_boxes, roidb, classes, 0.5, use_07_metric=False)
    res07 = de.evaluate(all_boxes, roidb, classes, 0.5, use_07_metric=True)
    assert np.array_equal(res07["aps"], g["ap_11pt_0"])                      # 11 sequential additions: the same bits
    for k, name in enumerate(classes[1:]):               # the bound of check_against_reference, not a second standard
        want = g["ap_area_0"][k]
        assert (np.isnan(want) and np.isnan(res["aps"][k])) or abs(res["aps"][k] - want) <= dg.ap_bound(res["rec"][name]), name
    assert np.isnan(res["mean_ap"]) and np.isnan(res["aps"][-1])              # detections of a class without ground truth
    assert res["mean_ap_present"] == np.mean(res["aps"][:-1])
    assert res07["mean_ap"] == np.mean(g["ap_11pt_0"])                        # the 11-point form of that class is 0, not nan
    empty = classes[-2]
    assert len(res["rec"][empty]) == 0 and len(res["prec"][empty]) == 0 and res["ap"][empty] == 0.0
    assert set(res["ap"]) == set(classes[1:]) and res["rec"][classes[1]].dtype == np.float64


def test_quantisation_is_the_results_files():
    from i2vsgg_amd import detection_eval as de
    rng = np.random.default_rng(3)
    s = np.concatenate([rng.random(500), [0.0005, 0.0015, 0.0025, 0.1235, 0.9995, 1.0, 0.0, 0.9994999, 0.0625, 0.3125]]).astype(np.float32)
    key = de.quantise_scores(s)
    assert key.dtype == np.int32
    for v, k in zip(s, key):
        text = "{:.3f}".format(v)                        # what the writer formats: the float32 value itself
        assert float(text) == k / 1000.0 and int(round(float(text) * 1000)) == k, (v, text, k)
    assert de.quantise_scores(np.float32([0.0625]))[0] == 62 and de.quantise_scores(np.float32([0.3125]))[0] == 312   # halves: to even
    assert de.quantise_scores(np.float64([0.0005]))[0] in (0, 1) and de.quantise_scores([-0.1234])[0] == -123
    x = np.concatenate([rng.uniform(0, 1000, 500), [0.25, 0.75, 10.05, 99.95, 3.5, 0.125, 7.375, 0.0]]).astype(np.float32)
    q = de.quantise_coords(x)
    assert q.dtype == np.float64
    for v, got in zip(x, q):
        assert got == float("{:.1f}".format(np.float64(v) + 1.0)), (v, got)
    assert de.quantise_coords(np.float32([0.25, 0.75, 0.125, 7.375])).tolist() == [1.2, 1.8, 1.1, 8.4]     # exact halves go to even digits
    assert de.quantise_coords(np.float32([0.05]))[0] == 1.1 and np.round(np.float64(np.float32(0.05)) + 1.0, 1) == 1.1
    assert de.quantise_coords(np.zeros((0, 4), np.float32)).shape == (0, 4)
    with pytest.raises(ValueError):
        de.quantise_scores([np.nan])


def test_pack_offset_tables():
    from i2vsgg_amd import detection_eval as de
    f = lambda rows: np.asarray(rows, np.float32)
    all_boxes = [[[], [], []],
                 [f([[0, 0, 9, 9, 0.9], [1, 1, 5, 5, 0.8]]), np.zeros((0, 5), np.float32), f([[2, 2, 8, 8, 0.7]])],
                 [[], [], []],
                 [[], f([[3, 3, 7, 7, 0.6004], [0, 0, 4.26, 4.24, 0.5996], [1, 1, 2, 2, 0.5]]), []]]
    roidb = [{"boxes": np.array([[0, 0, 9, 4], [5, 5, 9, 9]], np.uint16), "gt_classes": np.array([1, 3]), "gt_ishard": np.array([0, 1])},
             {"boxes": np.zeros((0, 4), np.uint16), "gt_classes": np.zeros(0, np.int32)},
             {"boxes": np.array([[1, 1, 2, 2], [2, 2, 3, 3], [4, 4, 6, 6]], np.uint16), "gt_classes": np.array([1, 2, 1]),
              "gt_ishard": np.array([0, 0, 0])}]
    pk = de.pack(all_boxes, roidb, 4)
    assert (pk.n_classes, pk.n_images) == (3, 3)
    assert pk.det_key.tolist() == [900, 800, 700, 600, 600, 500]
    assert pk.cls_off.tolist() == [0, 3, 3, 6] and pk.det_img.tolist() == [0, 0, 2, 1, 1, 1]
    assert pk.seg_det_off.tolist() == [0, 2, 3, 6] and pk.seg_cls.tolist() == [0, 0, 2] and pk.seg_img.tolist() == [0, 2, 1]
    assert pk.seg_gt.tolist() == [0, 2, 7]
    assert pk.gt_off.tolist() == [0, 1, 1, 3, 3, 3, 4, 5, 5, 5]
    assert pk.gt_box.tolist() == [[1, 1, 10, 5], [2, 2, 3, 3], [5, 5, 7, 7], [3, 3, 4, 4], [6, 6, 10, 10]]
    assert pk.gt_hard.tolist() == [0, 0, 0, 0, 1] and pk.gt_row.tolist() == [0, 0, 2, 1, 1] and pk.npos.tolist() == [3, 1, 0]
    assert pk.det_box[0].tolist() == [1, 1, 10, 10] and pk.det_box[4].tolist() == [1, 1, 5.3, 5.2]
    flag, ovmax, jmax = de.match_arrays_host(pk, 0.5)
    assert ovmax[0] == 0.5 and flag[0] == de.FP and jmax[0] == 0          # 50 / 100: not above the threshold
    assert flag[3] == de.FP and ovmax[3] == -np.inf and jmax[3] == -1      # no ground truth of the class in the image
    # equal keys keep the results-file order
    cur = de.curve_arrays_host(pk, flag)
    assert cur["perm"].tolist() == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        de.pack(all_boxes, roidb[:2], 4)
    many = [{"boxes": np.zeros((de.MAX_GT + 1, 4), np.uint16), "gt_classes": np.ones(de.MAX_GT + 1, np.int32)}]
    with pytest.raises(ValueError):                       # the kernel's limit is the host form's too
        de.pack([[[]], [[]]], many, 2)


def test_empty_and_degenerate_inputs():
    from i2vsgg_amd import detection_eval as de
    classes = ("__background__", "a", "b")
    roidb = [{"boxes": np.array([[0, 0, 9, 9]], np.uint16), "gt_classes": np.array([1]), "gt_ishard": np.array([0])}]
    none = [[[]], [np.zeros((0, 5), np.float32)], [[]]]
    res = de.evaluate(none, roidb, classes)
    assert res["aps"].tolist() == [0.0, 0.0] and res["mean_ap"] == 0.0 and len(res["rec"]["a"]) == 0
    some = [[[]], [np.float32([[0, 0, 9, 9, 0.5]])], [np.float32([[0, 0, 9, 9, 0.5]])]]
    res = de.evaluate(some, roidb, classes)
    assert res["ap"]["a"] == 1.0 and np.isnan(res["ap"]["b"]) and np.isnan(res["mean_ap"]) and res["mean_ap_present"] == 1.0
    eleven = 0.
    for _ in range(11):
        eleven = eleven + 1.0 / 11.                      # the reference's own accumulation: 1.0000000000000002
    assert de.evaluate(some, roidb, classes, use_07_metric=True)["aps"].tolist() == [eleven, 0.0]


def test_synthetic_imdb_hook_writes_files_and_lines(tmp_path, capsys):
    from i2vsgg_amd import detection_eval as de
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    imdb = get_imdb("synthetic_12_v")
    assert hasattr(imdb, "evaluate_detections")
    rng = np.random.default_rng(5)
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(12)] for _ in range(imdb.num_classes)]
    for i, e in enumerate(imdb.roidb):
        for b, c in zip(e["boxes"], e["gt_classes"]):
            if rng.random() < 0.8:
                d = np.concatenate([b + rng.uniform(-2, 2, 4), [rng.random()]]).astype(np.float32)[None]
                all_boxes[c][i] = np.concatenate([all_boxes[c][i], d])
    res = imdb.evaluate_detections(all_boxes, str(tmp_path / "out"), device=None)
    out = capsys.readouterr().out
    for name in imdb.classes[1:]:
        assert ("AP for %s = " % name) in out
        with open(tmp_path / "out" / (name + "_pr.pkl"), "rb") as f:
            pr = pickle.load(f)
        assert set(pr) == {"rec", "prec", "ap"} and np.array_equal(pr["rec"], res["rec"][name])
    line = [l for l in out.splitlines() if l.startswith("Mean AP = ")]
    assert len(line) == 1 and line[0] == "Mean AP = {:.4f}".format(res["mean_ap"])
    with open(tmp_path / "out" / "detection_eval.json") as f:
        js = json.load(f)
    assert set(js["ap"]) == set(imdb.classes[1:]) and "mean_ap" in js and "mean_ap_present" in js
    assert res["mean_ap_present"] > 0.5                  # most boxes were detected within 2 px
    # nothing detected at all, as a detector with random weights may do
    nothing = [[np.zeros((0, 5), np.float32) for _ in range(12)] for _ in range(imdb.num_classes)]
    res0 = imdb.evaluate_detections(nothing, str(tmp_path / "out0"), device=None)
    assert np.nan_to_num(res0["aps"]).sum() == 0.0


def test_eval_detections_script_on_the_host(tmp_path, capsys):
    import eval_detections
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    imdb = get_imdb("synthetic_6")
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(6)] for _ in range(imdb.num_classes)]
    for i, e in enumerate(imdb.roidb):
        for b, c in zip(e["boxes"], e["gt_classes"]):
            all_boxes[c][i] = np.concatenate([all_boxes[c][i], np.float32([list(b) + [0.5 + 0.01 * i]])])
    with open(tmp_path / "detections.pkl", "wb") as f:
        pickle.dump(all_boxes, f)
    res = eval_detections.main(["--detections", str(tmp_path / "detections.pkl"), "--imdbval_name", "synthetic_6", "--cpu",
                                "--output_dir", str(tmp_path / "o")])
    out = capsys.readouterr().out
    assert "Mean AP = " in out and "AP for class1 = " in out and os.path.exists(tmp_path / "o" / "detection_eval.json")
    seen = set(int(c) for e in imdb.roidb for c in e["gt_classes"])
    # every annotated box detected exactly and nothing else: 1 for a class that occurs, 0 (no detections) for one that does not
    assert res["aps"].tolist() == [1.0 if c in seen else 0.0 for c in range(1, imdb.num_classes)] and len(seen) > 3
    res07 = eval_detections.main(["--detections", str(tmp_path / "detections.pkl"), "--imdbval_name", "synthetic_6", "--cpu",
                                  "--voc07", "--ovthresh", "0.7"])
    assert "VOC07 metric? Yes" in capsys.readouterr().out and np.nanmax(res07["aps"]) <= 1.0 + 1e-12


def test_det_eval_entry_points_validate_their_arguments():
    from i2vsgg_amd import _lib
    L, p = _lib.lib, ctypes.c_void_p(16)
    err = lambda: L.i2v_last_error()
    assert L.i2v_version() >= 102
    need = L.i2v_det_eval_match_workspace_bytes(5000)
    assert need == L.i2v_det_eval_match_workspace_bytes(5000) >= 256 + 4 * 5000
    args = lambda **k: [k.get("seg", p), p, k.get("gt_off", p), k.get("key", p), p, k.get("gt_box", p), p, k.get("ns", 40),
                        k.get("nd", 5000), 300, 90, k.get("mg", 80), 0.5, p, p, p, k.get("ws", p), k.get("wsb", need), None]
    assert L.i2v_det_eval_match(*args(seg=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_match(*args(gt_off=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_match(*args(key=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_match(*args(gt_box=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_match(*args(mg=4097)) == -1 and b"4096" in err()
    assert L.i2v_det_eval_match(*args(ns=-1)) == -1 and b"negative" in err()
    assert L.i2v_det_eval_match(*args(nd=-3)) == -1 and b"negative" in err()
    assert L.i2v_det_eval_match(*args(wsb=need - 1)) == -1 and b"workspace" in err()
    assert L.i2v_det_eval_match(*args(ws=None)) == -1 and b"workspace" in err()
    need = L.i2v_det_eval_curve_workspace_bytes(5000)
    assert need == L.i2v_det_eval_curve_workspace_bytes(5000) >= 256 + 8 * 5000 + 8 * 5000
    assert L.i2v_det_eval_curve_workspace_bytes(300000) > need
    args = lambda **k: [k.get("key", p), k.get("cls_off", p), p, k.get("npos", p), k.get("nc", 15), k.get("nd", 5000), p, p, p, p,
                        k.get("prec", p), p, p, k.get("ws", p), k.get("wsb", need), None]
    assert L.i2v_det_eval_curve(*args(cls_off=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_curve(*args(key=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_curve(*args(npos=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_curve(*args(prec=None)) == -1 and b"null" in err()
    assert L.i2v_det_eval_curve(*args(nc=256)) == -1 and b"255" in err()
    assert L.i2v_det_eval_curve(*args(nc=-1)) == -1 and b"negative" in err()
    assert L.i2v_det_eval_curve(*args(nc=0)) == -1 and b"without a class" in err()
    assert L.i2v_det_eval_curve(*args(wsb=need - 1)) == -1 and b"workspace" in err()
    assert L.i2v_det_eval_curve(*args(ws=None)) == -1 and b"workspace" in err()
