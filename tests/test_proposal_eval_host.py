"""Proposal / detection recall on the host (i2vsgg_amd/proposal_eval.py): hand-worked covers, the host form against the plain
step loop of tests/proposal_eval_cases.py bit for bit, the metric against numbers computed by hand, ``pack``'s refusals and
eval_proposals.py --cpu on both file layouts."""
import json
import pickle

import numpy as np
import pytest

import proposal_eval_cases as pc
from i2vsgg_amd import proposal_eval as pe


def _cover(cand, roidb_entry, limits=(None,), areas=("all",)):
    pk = pe.pack([cand], [roidb_entry], limits, areas)
    return pk, pe.cover_arrays_host(pk)


@pytest.mark.parametrize("name", sorted(pc.hand_cases()))
def test_hand_worked_cover(name):
    cand, gt, want_ov, want_cand, want_step = pc.hand_cases()[name]
    for got in (_cover(cand, pc.entry(gt))[1], [x[None, None] for x in pc.cover_plain(cand, gt)]):
        ov, pick, step = got
        assert ov.shape == (1, 1, len(gt)) and ov.dtype == np.float64 and pick.dtype == np.int32 and step.dtype == np.int32
        assert np.array_equal(ov[0, 0], np.float64(want_ov)), (name, ov)
        assert pick[0, 0].tolist() == want_cand and step[0, 0].tolist() == want_step, (name, pick, step)


def test_no_ground_truth_gives_nan_recalls():
    res = pe.evaluate([np.float64([[0, 0, 9, 9]])], [pc.entry(np.zeros((0, 4)))], limits=(None,), areas=("all",))
    r = res[(None, "all")]
    assert r["num_pos"] == 0 and len(r["gt_overlaps"]) == 0 and np.isnan(r["recalls"]).all() and np.isnan(r["ar"])
    # a row of class 0 and a row whose gt_overlaps maximum is below 1 are no ground truths either
    e = pc.entry([[0, 0, 9, 9], [20, 0, 29, 9], [40, 0, 49, 9]], classes=[0, 2, 3], crowd=(1,))
    pk = pe.pack([np.zeros((0, 4))], [e], (None,), ("all",))
    assert pk.gt_row.tolist() == [2] and pk.gt_cls.tolist() == [3]


def test_a_box_on_a_boundary_counts_in_both_ranges():
    # 32 x 32 pixels = 32^2 exactly: small AND medium; 33 x 32 is medium only; the area is computed from the box without seg_areas
    gt = np.float64([[0, 0, 31, 31], [100, 0, 132, 31]])
    cand = gt.copy()
    pk, (ov, pick, step) = _cover(cand, pc.entry(gt), areas=("small", "medium", "large"))
    assert pk.gt_area.tolist() == [1024.0, 1056.0]
    assert ov[0, 0].tolist() == [1.0, -1.0] and pick[0, 0].tolist() == [0, -1] and step[0, 0].tolist() == [0, -1]
    assert ov[0, 1].tolist() == [1.0, 1.0] and pick[0, 1].tolist() == [0, 1] and step[0, 1].tolist() == [0, 1]
    assert ov[0, 2].tolist() == [-1.0, -1.0]
    # seg_areas, where the entry has them, decide instead of the box
    pk, (ov, _, _) = _cover(cand, pc.entry(gt, areas=[9216.0, 5.0]), areas=("small", "medium", "large"))
    assert pk.gt_area.tolist() == [9216.0, 5.0]
    assert ov[0, 0].tolist() == [-1.0, 1.0] and ov[0, 1].tolist() == [1.0, -1.0] and ov[0, 2].tolist() == [1.0, -1.0]


def test_a_limit_cuts_the_best_candidate_off():
    gt = np.float64([[0, 0, 9, 9]])
    cand = np.float64([[5, 0, 14, 9], [3, 0, 12, 9], [0, 0, 9, 9, ], [1, 0, 10, 9]])        # 1/3, 7/13, 1, 9/11
    pk, (ov, pick, step) = _cover(cand, pc.entry(gt), limits=(1, 2, 3, 1000, None))
    assert pk.limits.tolist() == [1, 2, 3, 1000, 2 ** 31 - 1]
    assert np.array_equal(ov[:, 0, 0], np.float64([1.0 / 3.0, 7.0 / 13.0, 1.0, 1.0, 1.0]))
    assert pick[:, 0, 0].tolist() == [0, 1, 2, 2, 2] and step[:, 0, 0].tolist() == [0] * 5
    # columns past the fourth are not read: a score column changes nothing
    pk5 = pe.pack([np.concatenate([cand, np.full((4, 2), 7.0)], 1).astype(np.float32)], [pc.entry(gt)], (1, 2, 3, 1000, None), ("all",))
    assert np.array_equal(pk5.cand_box, pk.cand_box) and pk5.cand_box.dtype == np.float64


def _counts():
    rng = np.random.default_rng(11)
    counts = [(int(n), int(m)) for n, m in zip(rng.integers(0, 81, 220), rng.integers(0, 13, 220))]
    return counts + [(0, 5), (3, 12), (80, 0), (1, 1), (80, 12)]


def test_host_form_equals_the_plain_loop_on_seeded_images():
    counts = _counts()
    assert len(counts) >= 200 and any(n < m for n, m in counts) and any(n == 0 < m for n, m in counts)
    cands, roidb = pc.random_batch(5, counts, size=1200)
    pk = pe.pack(cands, roidb, (1, 5, None), pc.ALL_AREAS)
    got, want = pe.cover_arrays_host(pk), pc.cover_cells_plain(pk)
    for g, w, name in zip(got, want, ("ov", "cand", "step")):
        assert g.shape == (3, 8, len(pk.gt_area)) and g.dtype == w.dtype
        assert np.array_equal(g, w), name
    ov, pick, step = got
    inside = ov[2, 0] >= 0
    assert inside.all() and (pick[2, 0] == -1).any() and (ov > 0.999).any() and ((ov > 0) & (ov < 0.3)).any()
    frac = pk.cand_box[(pk.cand_box != np.round(pk.cand_box)).any(1)]
    assert len(frac) > 100                                            # integer and fractional coordinates both occur
    for a in range(1, 8):                                             # every range holds something, and not everything
        assert 0 < (ov[2, a] >= 0).sum() < len(pk.gt_area), pc.ALL_AREAS[a]
    # the steps of a cell are 0 .. m-1, each once
    g0, g1 = pk.gt_off[-2], pk.gt_off[-1]
    assert sorted(step[2, 0, g0:g1].tolist()) == list(range(g1 - g0))


def test_evaluate_against_recalls_computed_by_hand():
    cands = [np.float64([[0, 0, 9, 9]]), np.float32([[5, 0, 14, 9], [51, 0, 60, 9]]), np.uint16([[3, 0, 12, 9]])]
    roidb = [pc.entry([[0, 0, 9, 9]], [1]), pc.entry([[0, 0, 9, 9], [50, 0, 59, 9]], [2, 3]), pc.entry([[0, 0, 9, 9]], [1])]
    res = pe.evaluate(cands, roidb, limits=(1, None), areas=("all", "small", "large"))
    assert set(res) == {(1, "all"), (1, "small"), (1, "large"), (None, "all"), (None, "small"), (None, "large"), "per_class"}
    thr = np.arange(0.5, 0.95 + 1e-5, 0.05)
    # all candidates: the overlaps are 1, {1/3, 9/11}, 7/13
    r = res[(None, "all")]
    assert np.array_equal(r["gt_overlaps"], np.float64([1.0 / 3.0, 7.0 / 13.0, 9.0 / 11.0, 1.0])) and r["num_pos"] == 4
    want = np.float64([0.75, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25])
    assert np.array_equal(r["thresholds"], thr) and np.array_equal(r["recalls"], want) and r["ar"] == want.mean() == 0.45
    # one candidate per image: image 1 keeps (5, 0, 14, 9) only; its second ground truth is a miss
    r = res[(1, "all")]
    assert np.array_equal(r["gt_overlaps"], np.float64([0.0, 1.0 / 3.0, 7.0 / 13.0, 1.0]))
    want = np.float64([0.5] + [0.25] * 9)
    assert np.array_equal(r["recalls"], want) and r["ar"] == want.mean()
    assert np.array_equal(res[(None, "small")]["recalls"], res[(None, "all")]["recalls"])            # 10 x 10 boxes: all small
    assert res[(None, "large")]["num_pos"] == 0 and np.isnan(res[(None, "large")]["ar"])
    pcl = res["per_class"]
    assert set(pcl) == {1, None}
    assert pcl[None]["hits"].tolist() == [0, 2, 0, 1] and pcl[None]["counts"].tolist() == [0, 2, 1, 1]
    assert pcl[1]["hits"].tolist() == [0, 2, 0, 0] and pcl[1]["counts"].dtype == np.int64
    # given thresholds; no "all" range, no per-class table
    r = pe.evaluate(cands, roidb, limits=(None,), areas=("small",), thresholds=[0.3, 0.9])
    assert r[(None, "small")]["recalls"].tolist() == [1.0, 0.25] and r["per_class"] == {}


def test_pack_refuses_what_breaks_a_cap():
    e = pc.entry([[0, 0, 9, 9]])
    one = np.float64([[0, 0, 9, 9]])
    with pytest.raises(ValueError, match="65535 candidates"):
        pe.pack([np.zeros((pe.MAX_CAND + 1, 4), np.float32)], [e])
    pe.pack([np.zeros((pe.MAX_CAND, 4), np.float32)], [e])
    with pytest.raises(ValueError, match="4096 ground truths"):
        pe.pack([one], [pc.entry(np.tile(one, (pe.MAX_GT + 1, 1)))])
    with pytest.raises(ValueError):
        pe.pack([[[0, 0, 9, 9], [0, 0, 9]]], [e])                     # ragged rows
    with pytest.raises(ValueError, match="x1 y1 x2 y2"):
        pe.pack([np.zeros((3, 3))], [e])
    with pytest.raises(ValueError, match="candidate arrays"):
        pe.pack([one, one], [e])
    with pytest.raises(ValueError, match="1 to 8 limits"):
        pe.pack([one], [e], limits=range(1, 10))
    with pytest.raises(ValueError, match="1 to 8 limits"):
        pe.pack([one], [e], limits=())
    with pytest.raises(ValueError, match="positive int or None"):
        pe.pack([one], [e], limits=(0,))
    with pytest.raises(ValueError, match="1 to 8 area"):
        pe.pack([one], [e], areas=list(pc.ALL_AREAS) + ["all"])
    with pytest.raises(ValueError, match="unknown area"):
        pe.pack([one], [e], areas=("tiny",))
    with pytest.raises(ValueError, match="not finite"):
        pe.pack([np.float64([[0, 0, np.inf, 9]])], [e])


def test_eval_proposals_script_on_the_host(tmp_path, capsys):
    import eval_proposals
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    imdb = get_imdb("synthetic_6")
    rng = np.random.default_rng(2)
    # proposals.pkl: every annotated box moved by up to two pixels, behind one box that touches nothing useful
    props, all_boxes = [], [[np.zeros((0, 5), np.float32) for _ in range(6)] for _ in range(imdb.num_classes)]
    for i, e in enumerate(imdb.roidb):
        b = np.asarray(e["boxes"], np.float32)
        props.append(np.concatenate([np.float32([[0, 0, 3, 3]]), b + rng.integers(-2, 3, size=b.shape).astype(np.float32)]))
        for j, (box, c) in enumerate(zip(b, e["gt_classes"])):
            all_boxes[c][i] = np.concatenate([all_boxes[c][i], np.float32([list(box) + [0.9 - 0.1 * j]])])
    with open(tmp_path / "proposals.pkl", "wb") as f:
        pickle.dump(props, f)
    with open(tmp_path / "detections.pkl", "wb") as f:
        pickle.dump(all_boxes, f)
    res = eval_proposals.main(["--candidates", str(tmp_path / "proposals.pkl"), "--imdbval_name", "synthetic_6", "--cpu", "--limits", "1",
                               "100", "all", "--out", str(tmp_path / "o" / "proposal_recall.json")])
    out = capsys.readouterr().out
    want = pe.evaluate(props, imdb.roidb, (1, 100, None), pe.DEFAULT_AREAS, num_classes=imdb.num_classes)
    assert set(res) == set(want) and (None, "all") in res and (1, "small") in res
    for key in want:
        if key != "per_class":
            assert np.array_equal(res[key]["recalls"], want[key]["recalls"], equal_nan=True) and res[key]["num_pos"] == want[key]["num_pos"]
    n_gt = sum(len(e["boxes"]) for e in imdb.roidb)
    assert res[(None, "all")]["num_pos"] == n_gt and res[(None, "all")]["recalls"][0] == 1.0 and res[(1, "all")]["recalls"][0] < 0.5
    assert res["per_class"][None]["counts"].sum() == n_gt and len(res["per_class"][None]["counts"]) == imdb.num_classes
    line = [x for x in out.splitlines() if x.startswith("AR@all") and " all " in x]
    assert len(line) == 1 and ("= %.4f" % res[(None, "all")]["ar"]) in line[0] and "recall@0.50 = 1.0000" in line[0]
    with open(tmp_path / "o" / "proposal_recall.json") as f:
        js = json.load(f)
    assert len(js["cells"]) == 12 and set(js["per_class"]) == {"1", "100", "all"}
    # detections.pkl: the annotated boxes themselves under their classes -> every ground truth covered exactly, at any size
    res = eval_proposals.main(["--candidates", str(tmp_path / "detections.pkl"), "--imdbval_name", "synthetic_6", "--cpu", "--areas", "all"])
    assert set(res) == {(k, "all") for k in pe.DEFAULT_LIMITS} | {"per_class"}
    r = res[(None, "all")]
    assert r["ar"] == 1.0 and (r["gt_overlaps"] == 1.0).all() and r["num_pos"] == n_gt
    cands = pe.candidates_from_detections(all_boxes)
    assert len(cands) == 6 and all((np.diff(c[:, 4]) <= 0).all() for c in cands)
    # equal scores keep the class order: a stable sort
    tie = [[], [np.float32([[0, 0, 9, 9, 0.5]])], [np.float32([[1, 1, 8, 8, 0.5], [2, 2, 7, 7, 0.7]])]]
    assert pe.candidates_from_detections(tie)[0][:, 0].tolist() == [2.0, 0.0, 1.0]


def test_proposal_cover_entry_point_validates_its_arguments():
    """No compute without a GPU: only the argument validation in front of the launch is exercised."""
    import ctypes
    from i2vsgg_amd import _lib
    L, p = _lib.lib, ctypes.c_void_p(16)
    err = lambda: _lib.lib.i2v_last_error()
    need = L.i2v_proposal_cover_workspace_bytes(2000)
    assert need == L.i2v_proposal_cover_workspace_bytes(0) >= 4

    def args(cand_off=p, limits=p, ov=p, ni=3, nc=10, ng=5, nl=5, na=4, mg=5, mc=10, ws=p, wsb=need):
        return (cand_off, p, p, p, p, limits, p, ni, nc, ng, nl, na, mg, mc, ov, p, p, ws, wsb, None)
    assert L.i2v_proposal_cover(*args(cand_off=None)) == -1 and b"null" in err()
    assert L.i2v_proposal_cover(*args(limits=None)) == -1 and b"null" in err()
    assert L.i2v_proposal_cover(*args(ov=None)) == -1 and b"null" in err()
    assert L.i2v_proposal_cover(*args(ni=-1)) == -1 and b"negative" in err()
    assert L.i2v_proposal_cover(*args(nl=9)) == -1 and b"1 to 8 limits" in err()
    assert L.i2v_proposal_cover(*args(na=0)) == -1 and b"1 to 8 area" in err()
    assert L.i2v_proposal_cover(*args(mg=pe.MAX_GT + 1)) == -1 and b"4096" in err()
    assert L.i2v_proposal_cover(*args(mc=pe.MAX_CAND + 1)) == -1 and b"65535" in err()
    assert L.i2v_proposal_cover(*args(wsb=need - 1)) == -1 and b"workspace" in err()
    assert L.i2v_proposal_cover(*args(ws=None)) == -1 and b"workspace" in err()


def test_the_file_layout_is_told_by_depth_and_a_partial_file_is_refused(tmp_path):
    import eval_proposals
    rows = [[0, 0, 9, 9], [1, 1, 8, 8]]
    files = {"lists": [rows, [], rows[:1]],                                       # images stored as plain lists of rows
             "arrays": [np.float32(rows), np.zeros((0, 4), np.float32), np.float32(rows[:1])],
             "boxes": [[[], [], []], [np.float32([r + [0.5] for r in rows]), np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32)],
                       [[], [], np.float32([rows[0] + [0.9]])]]}
    got = {}
    for name, obj in files.items():
        with open(tmp_path / (name + ".pkl"), "wb") as f:
            pickle.dump(obj, f)
        got[name] = pe.load_candidates(str(tmp_path / (name + ".pkl")))
        assert [c.shape[0] for c in got[name]] == [2, 0, 1] and all(c.ndim == 2 for c in got[name]), name
    assert all(np.array_equal(a, b) for a, b in zip(got["lists"], got["arrays"])) and got["boxes"][0].shape == (2, 5)
    with open(tmp_path / "bad.pkl", "wb") as f:
        pickle.dump([np.zeros((2, 3))], f)
    with pytest.raises(ValueError, match="neither"):
        pe.load_candidates(str(tmp_path / "bad.pkl"))
    # three images against an imdb of six: refused, not scored as a subset
    with pytest.raises(SystemExit, match="holds 3 images"):
        eval_proposals.main(["--candidates", str(tmp_path / "arrays.pkl"), "--imdbval_name", "synthetic_6", "--cpu"])
