"""Image relation recall@K on the host (i2vsgg_amd.image_relations, ``device=None``): the numpy host form against the scalar
restatement of the rules in tests/image_relation_cases.py -- every output equal, floats by their bits --, the hand-worked cases,
the fractions of ``evaluate``, the packing errors and the script.  No GPU."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_relation_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRETURNS = (50, 100)
N_REL = 12
_GEN = {}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _generated():
    """200 generated images, their scalar reference and the host form's outputs, computed once; nobody writes to them."""
    if not _GEN:
        from i2vsgg_amd import image_relations as ir
        relations, annotations = cases.generated_set(5, 200, n_rel=N_REL)
        seen = ir.seen_triplets_of(dict((k, annotations[k]) for k in sorted(annotations)[:60]))
        ref = cases.reference(relations, annotations, N_REL, NRETURNS, 0.5, None, seen)
        pk = ir.pack(relations, annotations, N_REL, NRETURNS, None, seen)
        _GEN.update(relations=relations, annotations=annotations, seen=seen, ref=ref, pk=pk, out=ir.evaluate_packed(pk, NRETURNS, 0.5))
    return _GEN


def _assert_equals_reference(pk, out, ref):
    hit, hit_ov, gt_rank, totals, zs_totals, per_predicate = out
    assert pk.keys == ref["keys"]
    assert pk.pred_off.tolist() == ref["pred_off"] and pk.gt_off.tolist() == ref["gt_off"]
    assert pk.pred_row.tolist() == ref["pred_row"]
    assert pk.gt_zs.tolist() == ref["gt_zs"] and pk.gt_trip[:, 1].tolist() == ref["gt_pred"]
    assert hit.dtype == np.int32 and gt_rank.dtype == np.int32 and hit_ov.dtype == np.float64 and totals.dtype == np.int64
    assert hit.tolist() == ref["hit"]
    assert gt_rank.tolist() == ref["gt_rank"]
    assert np.array_equal(_bits(hit_ov), _bits(ref["hit_ov"]))
    assert totals.tolist() == ref["totals"] and zs_totals.tolist() == ref["zs_totals"]
    assert per_predicate.tolist() == ref["per_predicate"]


def test_host_form_equals_the_scalar_restatement_on_generated_images():
    g = _generated()
    _assert_equals_reference(g["pk"], g["out"], g["ref"])


def test_generated_images_exercise_what_they_are_meant_to():
    """What the comparison above relies on: hits and misses in each mode, a prediction that took a ground truth other than its
    best, an overlap exactly at the threshold, an image over the cut, hits that K separates, ties and a zero-shot split."""
    g = _generated()
    ref, pk = g["ref"], g["pk"]
    for m in range(2):
        hits, n = ref["totals"][m][1]
        assert 0 < hits < n and n == len(pk.gt_trip) > 3000
        assert 0 < ref["totals"][m][0][0] < hits                   # K = 50 and K = 100 differ
        assert ref["n_second"][m] > 0 and ref["n_exact"][m] > 0
        assert 0 < ref["zs_totals"][m][1][0] < ref["zs_totals"][m][1][1] < n
        assert sum(1 for h in ref["hit"][m] if h < 0) > 0
    assert ref["hit"][0] != ref["hit"][1]                        # the modes are not one computation done twice
    assert ref["n_over_cut"] > 0 and (pk.n_before_cut > 100).sum() == ref["n_over_cut"]
    assert (np.diff(pk.pred_off) == 0).any() and np.diff(pk.pred_off).max() == 100
    ties = sum(1 for i in range(len(pk.keys)) for a, b in zip(pk.pred_conf[pk.pred_off[i]:pk.pred_off[i + 1] - 1],
                                                                pk.pred_conf[pk.pred_off[i] + 1:pk.pred_off[i + 1]]) if a == b)
    assert ties > 100


def test_evaluate_equals_the_scalar_restatement_and_thresholds_and_cap_matter():
    from i2vsgg_amd import image_relations as ir
    g = _generated()
    res = ir.evaluate(g["relations"], g["annotations"], N_REL, NRETURNS, seen_triplets=g["seen"])
    ref = g["ref"]
    for m, mode in enumerate(ir.MODES):
        for j, k in enumerate(NRETURNS):
            for name in ("recall", "zero_shot_recall", "mean_recall"):
                assert np.array_equal(_bits(res[mode][name][k]), _bits(ref[name][m][j])), (mode, name, k)
            assert list(res[mode]["totals"][k]) == ref["totals"][m][j]
    assert res["n_images"] == 200 and res["n_gt"] == len(ref["gt_pred"]) and res["n_gt_zero_shot"] == sum(ref["gt_zs"]) and res["n_ignored"] == 0
    sub = dict((k, g["relations"][k]) for k in sorted(g["relations"])[:40])
    sub_anno = dict((k, g["annotations"][k]) for k in sorted(g["annotations"])[:40])
    for kw in ({"iou_threshold": 0.3}, {"iou_threshold": 0.7}, {"k_per_pair": 1}, {"nreturns": (1, 5, 20, 70)}):
        full = dict(nreturns=NRETURNS, iou_threshold=0.5, k_per_pair=None, seen_triplets=g["seen"])
        full.update(kw)
        want = cases.reference(sub, sub_anno, N_REL, **full)
        pk = ir.pack(sub, sub_anno, N_REL, full["nreturns"], full["k_per_pair"], full["seen_triplets"])
        _assert_equals_reference(pk, ir.evaluate_packed(pk, full["nreturns"], full["iou_threshold"]), want)
        base = cases.reference(sub, sub_anno, N_REL, NRETURNS, 0.5, None, g["seen"])
        assert want["hit"] != base["hit"] or want["totals"] != base["totals"], kw


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_worked_case(name):
    from i2vsgg_amd import image_relations as ir
    c = cases.hand_cases()[name]
    kw = dict(c["kwargs"])
    nreturns = c.get("nreturns", (50,))
    thr = kw.pop("iou_threshold", 0.5)
    pk = ir.pack(c["relations"], c["annotations"], c["n_rel"], nreturns, kw.get("k_per_pair"), kw.get("seen_triplets"))
    hit, hit_ov, gt_rank, totals, zs_totals, _ = ir.evaluate_packed(pk, nreturns, thr)
    assert pk.pred_row.tolist() == c["pred_row"]
    assert hit.tolist() == c["hit"] and gt_rank.tolist() == c["gt_rank"]
    assert np.array_equal(_bits(hit_ov), _bits(c["hit_ov"]))
    res = ir.evaluate(c["relations"], c["annotations"], c["n_rel"], nreturns, thr, **kw)
    for k, per_mode in c["totals"].items():
        for m, mode in enumerate(ir.MODES):
            assert res[mode]["totals"][k] == per_mode[m]
            assert res[mode]["recall"][k] == np.float64(per_mode[m][0]) / np.float64(per_mode[m][1])
    for k, per_mode in c.get("zs_totals", {}).items():
        for m, mode in enumerate(ir.MODES):
            assert res[mode]["zs_totals"][k] == per_mode[m]
            assert res[mode]["zero_shot_recall"][k] == np.float64(per_mode[m][0]) / np.float64(per_mode[m][1])
    if "zs_totals" not in c:
        assert all(np.isnan(res[mode]["zero_shot_recall"][k]) for mode in ir.MODES for k in nreturns)
    for key, value in c.get("counts", {}).items():
        assert res[key] == value, key
    if "train" in c:
        assert ir.seen_triplets_of(c["train"]) == kw["seen_triplets"]
    # ... and the scalar restatement agrees with the hand
    _assert_equals_reference(pk, ir.evaluate_packed(pk, nreturns, thr),
                             cases.reference(c["relations"], c["annotations"], c["n_rel"], nreturns, thr, kw.get("k_per_pair"), kw.get("seen_triplets")))


def test_evaluate_fractions_worked_by_hand():
    from i2vsgg_amd import image_relations as ir
    rel, anno, n_rel = cases.fractions_case()
    res = ir.evaluate(rel, anno, n_rel, nreturns=(50, 1))
    r, p = res["relation"], res["phrase"]
    assert r["totals"][50] == (3, 7) and r["recall"][50] == np.float64(3.0) / np.float64(7.0)
    assert r["totals"][1] == (1, 7) and r["recall"][1] == np.float64(1.0) / np.float64(7.0)
    assert r["per_predicate"][50].tolist() == [[1, 2], [1, 1], [1, 1], [0, 1], [0, 1], [0, 1], [0, 0]]
    assert r["mean_recall"][50] == (np.float64(0.5) + 1.0 + 1.0) / np.float64(6.0)
    assert r["mean_recall"][1] == np.float64(0.5) / np.float64(6.0)
    assert p["totals"][50] == (4, 7) and p["mean_recall"][50] == (np.float64(0.5) + 1.0 + 1.0 + 1.0) / np.float64(6.0)   # the swapped pair
    assert np.isnan(r["zero_shot_recall"][50]) and r["zs_totals"][50] == (0, 0)
    assert res["n_images"] == 1 and res["n_gt"] == 7 and res["n_gt_zero_shot"] == 0
    lines = []
    ir.report(res, lines.append)
    assert any("relation detection R@50: 0.4286 (3 of 7)" in s for s in lines)
    assert json.loads(json.dumps(ir.to_json(res)))["relation"]["zero_shot_recall"]["50"] is None


def test_packing_errors():
    from i2vsgg_amd import image_relations as ir
    two = {"boxes": [[5, 5, 50, 60], [40, 10, 90, 80]], "box_classes": [2, 4]}
    good = cases.record([((2, 2, 4), 0.9, [5, 5, 50, 60], [40, 10, 90, 80], 0)])
    ok = {"x": dict(two, rels=[[0, 1, 2]])}
    assert ir.evaluate({"x": good}, ok, 5)["relation"]["recall"][50] == 1.0
    for rels in ([[0, 2, 1]], [[-1, 1, 1]], [[0, 1, 5]], [[0, 1, -1]]):
        with pytest.raises(ValueError):
            ir.pack({"x": good}, {"x": dict(two, rels=rels)}, 5)
    for field, value in ((1, np.inf), (1, np.nan), (2, np.nan), (3, -np.inf)):
        bad = [np.array(x) for x in good]
        bad[field][0] = value
        with pytest.raises(ValueError, match="not finite"):
            ir.pack({"x": tuple(bad)}, ok, 5)
    with pytest.raises(ValueError, match="not finite"):
        ir.pack({}, {"x": {"boxes": [[0, 0, np.nan, 5], [1, 1, 2, 2]], "box_classes": [1, 2], "rels": [[0, 1, 0]]}}, 5)
    with pytest.raises(ValueError, match="at most %d" % ir.MAX_GT):
        ir.pack({}, {"x": dict(two, rels=[[0, 1, 2]] * (ir.MAX_GT + 1))}, 5)
    assert len(ir.pack({}, {"x": dict(two, rels=[[0, 1, 2]] * ir.MAX_GT)}, 5).gt_trip) == ir.MAX_GT
    for nreturns in ((), (0,), (50, 50), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="nreturns"):
            ir.pack({"x": good}, ok, 5, nreturns)
    with pytest.raises(ValueError, match="k_per_pair"):
        ir.pack({"x": good}, ok, 5, k_per_pair=0)
    with pytest.raises(ValueError, match="iou_threshold"):
        ir.evaluate({"x": good}, ok, 5, iou_threshold=0.0)
    with pytest.raises(ValueError, match="record"):
        ir.pack({"x": (good[0], good[1], good[2], good[3], good[4][:0])}, ok, 5)
    from i2vsgg_amd import _lib, ops
    assert _lib.lib.i2v_version() >= 107
    with pytest.raises(_lib.I2VError, match="match_host"):       # no quiet fall-back: the ops are the GPU's, the host form has its own name
        ops.image_relation_match([0], [0], np.zeros((0, 3)), np.zeros((0, 8)), np.zeros((0, 3)), np.zeros((0, 8)), device="cpu")
    assert _lib.lib.i2v_image_relation_match(None, None, None, None, None, None, 1, 0, 0, 0, 0.5, None, None, None, None, 0, None) == -1
    assert _lib.lib.i2v_image_relation_count(None, None, None, None, 0, 5, 9, None, None, None, None, 0, None) == -1
    assert b"values of K" in _lib.lib.i2v_last_error()
    empty = ir.evaluate({}, {}, 5)                               # nothing to evaluate: nan, not an error
    assert empty["n_images"] == 0 and np.isnan(empty["relation"]["recall"][50]) and np.isnan(empty["phrase"]["mean_recall"][100])


def test_script_round_trip_on_the_host(tmp_path, capsys):
    """eval_image_relations.py --cpu on pickled files prints and writes what ``evaluate`` returns."""
    sys.path.insert(0, ROOT)
    import eval_image_relations
    from i2vsgg_amd import image_relations as ir
    g = _generated()
    keys = sorted(g["annotations"])
    test = dict((k, g["annotations"][k]) for k in keys[60:100])
    train = dict((k, g["annotations"][k]) for k in keys[:60])
    pred = dict((k, g["relations"][k]) for k in keys[55:100])    # five images the ground truth does not hold
    paths = [str(tmp_path / n) for n in ("relations.pkl", "annotations.pkl", "train.pkl", "out.json")]
    for path, obj in zip(paths, (pred, test, train)):
        with open(path, "wb") as f:
            pickle.dump(obj, f)
    res = eval_image_relations.main(["--prediction", paths[0], "--groundtruth", paths[1], "--num_relations", str(N_REL), "--train_annotations",
                                     paths[2], "--k_per_pair", "2", "--nreturns", "20", "50", "--iou", "0.4", "--cpu", "--out", paths[3]])
    want = ir.evaluate(pred, test, N_REL, (20, 50), 0.4, 2, ir.seen_triplets_of(train))
    with open(paths[3]) as f:
        written = json.load(f)
    assert written == json.loads(json.dumps(ir.to_json(want))) == json.loads(json.dumps(ir.to_json(res)))
    assert res["n_ignored"] == 5 and res["n_images"] == 40 and 0 < res["n_gt_zero_shot"] < res["n_gt"]
    ref = cases.reference(pred, test, N_REL, (20, 50), 0.4, 2, ir.seen_triplets_of(train))
    assert written["relation"]["totals"]["50"] == ref["totals"][0][1] and written["phrase"]["zs_totals"]["20"] == ref["zs_totals"][1][0]
    out = capsys.readouterr().out
    assert "relation detection R@50: %.4f" % want["relation"]["recall"][50] in out and "phrase detection R@20" in out
