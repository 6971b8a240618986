"""Predicate recognition on the host: the rules of i2vsgg_amd.recognition on a hand-worked case, its numpy form against the
reference's own recognition_output / evaluate_recognition (tests/golden/recognition.npz, tools/gen_golden.py
``gen_recognition``), the mean against numpy's, the packing errors, the C-ABI argument errors and the scoring script."""
import ctypes
import json
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recognition_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def gold_set():
    """The golden case set, packed once, with the host form's answer; nobody writes to either."""
    from i2vsgg_amd import recognition
    cs = cases.golden_set()
    pk = recognition.pack(cs["frame_recognitions"], cs["groundtruth"], cs["classes"], cs["predicates"])
    return cs, pk, recognition.align_arrays_host(pk)


def test_hand_worked_case():
    """C = 3 (bg, cat, dog), R = 6.  Video "a": the pair (1, 2) over [0, 4) with two predicates -- frame 1 lacks the pair and
    frame 3 is empty, so frames 0 and "2" give its two rows -- and the pair (2, 1) over [0, 3) with three rows.  Video "b": the
    annotated pair (8, 7) occurs only as (7, 8): a segment without rows.  Video "c" has no predictions."""
    from i2vsgg_amd import recognition
    fr, gt, classes, predicates = cases.hand_case()
    pk = recognition.pack(fr, gt, classes, predicates)
    assert pk.segments == [("a", 1, 2, 0, 4), ("a", 2, 1, 0, 3), ("b", 8, 7, 0, 1)] and pk.n_videos_missing == 1
    assert pk.seg_off.tolist() == [0, 2, 5, 5] and pk.inst.tolist() == [[0, 1, 0, 2], [0, 1, 3, 2], [1, 1, 5, 1], [2, 1, 0, 2]]
    assert pk.rows.shape == (5, 12)
    assert pk.rows[pk.seg_row[0]].tolist() == [0, 0.75, 0.25, 0, 0.25, 0.75, -1, -2, -3, -4, -5, -6]
    assert pk.rows[pk.seg_row[1]].tolist() == [0, 0.25, 0.75, 0, 0.25, 0.5, -3, -2, -5, -2, -5, -6]      # pair 1 of frame "2"
    mean, count, top, hit, totals, per_class = recognition.align_arrays_host(pk)
    assert count.tolist() == [2, 3, 0]
    assert mean[0].tolist() == [0, 0.5, 0.5, 0, 0.25, 0.625, -2, -2, -4, -3, -5, -6]
    assert mean[1].tolist() == [0, 1.0 / 3, 1.75 / 3, 0, 1.125 / 3, 1.375 / 3, -17.0 / 3, -14.0 / 3, -11.0 / 3, -8.0 / 3, -5.0 / 3, -5.0 / 3]
    assert not mean[2].any()
    pad = [-1] * 10
    # segment 0: cat and dog tie as subject (cat, the lower index, first); predicates 0 and 1 tie at the top
    assert top[0].tolist() == [[1, 2, 0] + pad[3:], [2, 1, 0] + pad[3:], [0, 1, 3, 2, 4, 5] + pad[6:]]
    # segment 1: predicates 4 and 5 tie at the top: 4 takes the first place, so the annotated 5 is no hit@1
    assert top[1].tolist() == [[2, 1, 0] + pad[3:], [2, 1, 0] + pad[3:], [4, 5, 3, 2, 1, 0] + pad[6:]]
    assert top[2].tolist() == [pad, pad, pad]
    #                        sub@1 sub@5 obj@1 obj@5 pre@1 pre@5 rel@1
    assert hit.tolist() == [[1, 1, 1, 1, 1, 1, 1],        # cat p0 dog
                            [1, 1, 1, 1, 0, 1, 0],        # cat p3 dog: p3 is third
                            [0, 1, 0, 1, 0, 1, 0],        # cat p5 cat: dog ranks first twice, p5 loses the tie
                            [0, 0, 0, 0, 0, 0, 0]]        # no rows
    assert totals.tolist() == [2, 3, 2, 3, 1, 3, 1, 3]
    assert per_class.tolist() == [[[0, 0], [0, 0]], [[2, 4], [4, 4]], [[2, 2], [2, 2]]]
    res = recognition.evaluate(fr, gt, classes, predicates)
    assert res["sub"] == {1: 2 / 3, 5: 1.0} and res["obj"] == {1: 2 / 3, 5: 1.0} and res["pre"] == {1: 1 / 3, 5: 1.0}
    assert res["rel"] == {1: 1 / 3} and res["objects"] == {1: {1: 0.5, 2: 1.0}, 5: {1: 1.0, 2: 1.0}}
    assert (res["n_aligned"], res["n_unaligned"], res["n_videos_missing"]) == (3, 1, 1)
    recs = recognition.video_recognitions(pk, mean)
    assert list(recs) == ["a"] and [r["triplet"] for r in recs["a"]] == [[1, 0, 2], [1, 3, 2], [1, 5, 1]]
    assert recs["a"][2]["pre_score"].tolist() == mean[1, 6:].tolist() and recs["a"][1]["obj_score"].tolist() == [0, 0.25, 0.625]
    lines = []
    recognition.report(res, classes, out=lines.append)
    assert lines[0] == "object #1 acc@1 : 0.5" and lines[-1] == "relationship recognition accurancy@1: {}".format(1 / 3)
    assert len(lines) == 4 + 7 and lines[4] == "subject recognition accurancy@1: {}".format(2 / 3)


def test_a_class_without_an_instance_is_nan_without_a_warning():
    import warnings
    from i2vsgg_amd import recognition
    fr, gt, classes, predicates = cases.hand_case()
    wide = dict((v, dict((f, dict(r, **dict((k, np.hstack([r[k], np.zeros((len(r[k]), 1), np.float32)])) for k in ("sub_scores", "obj_scores")))
                          if r else {}) for f, r in frames.items())) for v, frames in fr.items())      # a fourth class that never scores
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = recognition.evaluate(wide, gt, classes + ["emu"], predicates)
        empty = recognition.evaluate({}, gt, classes, predicates)
    assert np.isnan(res["objects"][1][3]) and np.isnan(res["objects"][5][3]) and res["objects"][1][2] == 1.0
    assert np.isnan(empty["sub"][1]) and np.isnan(empty["rel"][1]) and empty["n_videos_missing"] == 3 and empty["n_aligned"] == 0


def test_host_form_equals_the_reference_metrics_bit_for_bit(gold_set):
    """evaluate_recognition, compiled from its own lines, on video_recognitions of the golden case set: both sides are hits /
    total in float64."""
    from i2vsgg_amd import recognition
    cs, pk, out = gold_set
    g = golden("recognition")
    assert len(pk.segments) == int(g["n_segments"]) and len(pk.inst) == int(g["n_instances"]) and 200 <= len(pk.segments) <= 600
    res = recognition.result_of(pk, out[4], out[5])
    seven = [res["sub"][1], res["sub"][5], res["obj"][1], res["obj"][5], res["pre"][1], res["pre"][5], res["rel"][1]]
    assert np.array_equal(_bits(seven), _bits(g["metrics"]))
    assert 0.05 < res["rel"][1] < 0.95 and res["n_unaligned"] > 0                      # a set that can tell right from wrong
    for k, nre in enumerate((1, 5)):
        got = [res["objects"][nre][c] for c in range(1, 16)]
        assert not np.isnan(got).any()
        assert np.array_equal(_bits(got), _bits(g["per_class"][k, 1:]))
    assert recognition.evaluate(cs["frame_recognitions"], cs["groundtruth"], cs["classes"], cs["predicates"])["pre"] == res["pre"]


def test_recognition_output_equals_the_reference(gold_set):
    """The numpy tail on the golden's seeded frame record: the reference's four outputs exactly; the arithmetic is
    float32(float64(rel) + log(0.5 * (prior + 1/15))), which is also what the kernel's host form computes from the table."""
    from i2vsgg_amd import eval as ev
    g = golden("recognition")
    rec = cases.frame_record()
    keep = dict((k, np.array(v)) for k, v in rec.items() if k != "tids")
    sub, obj, pre, tids = ev.recognition_output(rec)
    for got, name in ((sub, "sub_scores"), (obj, "obj_scores"), (pre, "pre_scores")):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), g[name].view(np.uint32)), name
    assert np.array_equal(np.asarray(tids), g["tids"])
    assert not sub[:, 0].any() and not obj[:, 0].any()
    for k, v in keep.items():                                                        # the record is left as it was
        assert np.array_equal(np.asarray(rec[k]), v), k
    want = (rec["rel_scores"].astype(np.float64) + np.log(0.5 * (rec["rel_so_prior"] + 1.0 / 15))).astype(np.float32)
    assert np.array_equal(pre.view(np.uint32), want.view(np.uint32))
    assert ev.SO_PRIOR_SMOOTHING == 1.0 / 15
    assert ev.recognition_output({"boxes": [], "classes": [], "confs": []}) == (None,) * 4
    assert ev.recognition_output(dict(rec, boxes=rec["boxes"][:1])) == (None,) * 4
    assert ev.recognition_output({"boxes": rec["boxes"], "classes": [1] * 6, "confs": [1.0] * 6}) == (None,) * 4


def test_rows_host_form_uses_the_table_like_the_gathered_prior():
    """recognition_rows_host (the form the kernel is compared with) reads log(0.5 * (prior + 1/15)) from a table computed once;
    recognition_output takes the log of the gathered rows.  The same values either way, also with class 0 wrapping to the last
    row, and log(1/30) without a prior."""
    from i2vsgg_amd import eval as ev
    rng = np.random.default_rng(11)
    B, P, C, R = 5, 7, 16, 62
    prob = rng.dirichlet(np.ones(C), B).astype(np.float32)
    prob[2, 1:] = 0.0                                                                # every class at zero: arg-max 0
    prob[3, [4, 9]] = prob[3].max() + np.float32(0.125)                              # two equal largest: the lower wins
    rel = rng.dirichlet(np.ones(R), P).astype(np.float32)
    ixs, ixo = rng.integers(0, B, P), rng.integers(0, B, P)
    ixs[0], ixo[0], ixs[1] = 2, 3, 3
    prior = rng.uniform(0, 1, (C - 1, C - 1, R))
    sub, obj, pre, cls = ev.recognition_rows_host(prob, rel, ixs, ixo, ev.prior_log_table(prior, C, R))
    assert cls[2] == 0 and cls[3] == 4 and cls.dtype == np.int32
    rec = {"boxes": [[0, 0, 1, 1]] * B, "sub_scores": prob[ixs], "obj_scores": prob[ixo], "rel_scores": rel, "tids": [[0, 1]] * P,
           "rel_so_prior": prior[cls[ixs] - 1, cls[ixo] - 1]}
    want = ev.recognition_output(rec)
    for a, b in zip((sub, obj, pre), want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    none = ev.recognition_rows_host(prob, rel, ixs, ixo, ev.prior_log_table(None, C, R))[2]
    assert np.array_equal(none, (rel.astype(np.float64) + np.log(1.0 / 30)).astype(np.float32))


def test_the_generator_redraws_no_segment():
    """Ties are a condition, not a measurement: a segment in which two of the 11 largest means of a group are equal would be
    drawn again, and at most 5 % of the draws may be.  Observed on the CPU: 0 re-draws in 316 draws of the golden set, 0 in
    the 271 draws (4 of them planted ties, which are exempt) of each of the four device sets."""
    cs = cases.golden_set()
    assert cs["draws"] == 316 and cs["redraws"] <= 0.05 * cs["draws"]
    for C, R in ((16, 62), (35, 132), (2, 1), (81, 512)):
        ds = cases.device_set(C, R)
        assert ds["draws"] == 271 and ds["redraws"] <= 0.05 * ds["draws"]
    # the condition itself: it sees a tie among the 11 largest and not one below them
    m = np.arange(40, dtype=np.float64)
    assert not cases.has_tie(m, 10, 20)
    tied = m.copy()
    tied[25] = tied[30]
    assert cases.has_tie(tied, 10, 20)
    low = m.copy()
    low[21] = low[22]                                                                # ranks 17 and 18 of the third group
    assert not cases.has_tie(low, 10, 20)


def test_mean_equals_numpy_mean_bit_for_bit(gold_set):
    """align_arrays_host's mean (one add per row, one division) is np.vstack(rows).mean(axis=0), on the golden set and on the
    edge set with segments of 1 to 300 rows."""
    from i2vsgg_amd import recognition
    sets = [(gold_set[1], gold_set[2][0])]
    ds = cases.device_set(16, 62)
    pk = recognition.pack(ds["frame_recognitions"], ds["groundtruth"], ds["classes"], ds["predicates"])
    sets.append((pk, recognition.align_arrays_host(pk)[0]))
    seen = set()
    for pk, mean in sets:
        for s in range(len(pk.seg_off) - 1):
            idx = pk.seg_row[pk.seg_off[s]:pk.seg_off[s + 1]]
            seen.add(len(idx))
            if len(idx):
                want = np.vstack([pk.rows[r] for r in idx]).mean(axis=0)
                assert np.array_equal(_bits(mean[s]), _bits(want)), s
    assert {0, 1, 2, 63, 64, 65, 300} <= seen


def test_device_case_set_has_the_cases_it_promises():
    from i2vsgg_amd import recognition
    ds = cases.device_set(16, 62)
    pk = recognition.pack(ds["frame_recognitions"], ds["groundtruth"], ds["classes"], ds["predicates"])
    counts = np.diff(pk.seg_off)
    assert len(counts) > 256 and {0, 1, 2, 63, 64, 65, 300} <= set(counts.tolist())
    assert sorted(ds["row_counts"].values()) == sorted(counts.tolist())              # skipped, dropped and missing frames as planned
    doubled = sum(1 for v in ds["frame_recognitions"].values() for r in v.values() if r and len(set(map(tuple, r["tids"]))) < len(r["tids"]))
    assert doubled >= 5
    assert any(isinstance(k, str) for v in ds["frame_recognitions"].values() for k in v)
    mean, count, top, hit, totals, per_class = recognition.align_arrays_host(pk)
    s0 = pk.segments.index(("edges", 0, 1, 0, 1))
    assert mean[s0, 1] == mean[s0, 15] == 0.9375 and top[s0, 0, :2].tolist() == [1, 15]      # two equal maxima
    assert top[s0, 2, :2].tolist() == [1, 61] and mean[s0, 33] == mean[s0, 93] == 0.5
    assert len(pk.inst) > len(pk.segments) and 0 < totals[6] < totals[7] < len(pk.inst)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_refuses_malformed_tids():
    from i2vsgg_amd import recognition
    fr, gt, classes, predicates = cases.hand_case()
    fr["a"][0]["tids"] = [[1, 2], 3]
    with pytest.raises(ValueError, match="frame 0 of video a"):
        recognition.pack(fr, gt, classes, predicates)
    fr["a"][0]["tids"] = [[1, 2]]                                                    # one pair, two rows of scores
    with pytest.raises(ValueError, match="frame 0 of video a"):
        recognition.pack(fr, gt, classes, predicates)


def test_pack_refuses_a_non_finite_score():
    from i2vsgg_amd import recognition
    for bad in (np.nan, np.inf):
        fr, gt, classes, predicates = cases.hand_case()
        fr["a"]["2"]["pre_scores"][1, 3] = bad
        with pytest.raises(ValueError, match="frame 2 of video a.*non-finite"):
            recognition.pack(fr, gt, classes, predicates)


def test_pack_refuses_unknown_names():
    from i2vsgg_amd import recognition
    fr, gt, classes, predicates = cases.hand_case()
    gt["a"][0]["triplet"] = ["emu", "p0", "dog"]
    with pytest.raises(ValueError, match="unknown class name 'emu'"):
        recognition.pack(fr, gt, classes, predicates)
    gt["a"][0]["triplet"] = ["cat", "p9", "dog"]
    with pytest.raises(ValueError, match="unknown predicate name 'p9'"):
        recognition.pack(fr, gt, classes, predicates)
    gt["a"][0]["triplet"] = [1, 6, 2]
    with pytest.raises(ValueError, match="predicate label 6"):
        recognition.pack(fr, gt, classes, predicates)


def test_annotation_tids_layouts():
    """forward_predicate_eval's reading of an annotation's tids: per relation, or per box; anything else names the frame."""
    from i2vsgg_amd.model.faster_rcnn.faster_rcnn_SGG_emb import pair_track_ids
    anno = {"boxes": [[0, 0, 9, 9]] * 4, "rels": [[0, 1, 5], [2, 3, 1], [0, 1, 7], [3, 2, 0]]}
    per_rel = dict(anno, tids=[[10, 11], [12, 13], [99, 98], [13, 12]])
    assert pair_track_ids(per_rel) == [[10, 11], [12, 13], [13, 12]]                 # unique pairs, the first relation's tids
    per_box = dict(anno, tids=[10, 11, 12, np.int64(13)])
    assert pair_track_ids(per_box) == [[10, 11], [12, 13], [13, 12]]
    for bad in ([[10, 11]] * 3, [10, 11, 12], [[10, 11, 12]] * 4, ["a", "b", "c", "d"], [], None):
        with pytest.raises(ValueError, match="frame7"):
            pair_track_ids(dict(anno, tids=bad), "frame7")


def test_cabi_null_pointers_are_status_codes():
    from i2vsgg_amd import _lib
    L = _lib.lib
    p = ctypes.c_void_p(256)
    assert L.i2v_version() >= 105
    assert L.i2v_recognition_rows_workspace_bytes(7) >= 4 and L.i2v_recognition_align_workspace_bytes(3, 4) >= 8
    assert L.i2v_recognition_rows(None, p, p, p, p, 5, 7, 16, 62, p, p, p, p, p, 256, None) == -1
    assert b"recognition_rows: null" in L.i2v_last_error()
    assert L.i2v_recognition_rows(p, p, p, p, p, 5, 7, 16, 62, p, p, None, p, p, 256, None) == -1
    assert L.i2v_recognition_rows(p, p, p, p, p, 5, 7, 16, 62, p, p, p, p, None, 256, None) == -1
    assert b"workspace" in L.i2v_last_error()
    assert L.i2v_recognition_rows(p, p, p, p, p, 5, 7, 1, 62, p, p, p, p, p, 256, None) == -1
    assert L.i2v_recognition_rows(p, p, p, p, p, -1, 7, 16, 62, p, p, p, p, p, 256, None) == -1
    assert L.i2v_recognition_align(None, p, p, p, 9, 9, 3, 4, 16, 62, p, p, p, p, p, p, p, 256, None) == -1
    assert b"recognition_align: null" in L.i2v_last_error()
    assert L.i2v_recognition_align(p, p, p, p, 9, 9, 3, 4, 16, 62, p, p, p, None, p, p, p, 256, None) == -1
    assert L.i2v_recognition_align(p, p, p, p, 9, 9, 3, 4, 16, 62, p, p, p, p, None, p, p, 256, None) == -1
    assert L.i2v_recognition_align(p, p, p, p, 9, 9, 3, 4, 16, 62, p, p, p, p, p, p, p, 4, None) == -1
    assert b"workspace" in L.i2v_last_error()


def test_cabi_width_over_the_limit_is_a_status_code():
    """The means of one segment are ranked in LDS: 2 * C + R is at most I2V_RECOGNITION_MAX_WIDTH (2048, in the header);
    81 / 512 (VidOR's classes and well over its predicates) is far inside."""
    from i2vsgg_amd import _lib
    L = _lib.lib
    p = ctypes.c_void_p(256)
    text = open(os.path.join(ROOT, "include", "i2vsgg_hip.h")).read()
    assert "#define I2V_RECOGNITION_MAX_WIDTH 2048" in text
    assert 2 * 81 + 512 <= 2048
    assert L.i2v_recognition_align(p, p, p, p, 9, 9, 3, 4, 81, 2048 - 2 * 81 + 1, p, p, p, p, p, p, p, 256, None) == -1
    assert b"over the limit of 2048" in L.i2v_last_error()
    assert L.i2v_recognition_align(p, p, p, p, 9, 9, 3, 4, 1, 10, p, p, p, p, p, p, p, 256, None) == -1
    assert b"at least 2 classes" in L.i2v_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the scoring script
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_script_on_the_host(tmp_path, capsys, gold_set):
    """eval_recognition.py --cpu on written files returns the numbers of recognition.evaluate(device=None); string frame
    numbers, as a JSON round trip makes them, change nothing."""
    from i2vsgg_amd import recognition
    import eval_recognition
    cs, pk, out = gold_set
    pred, gt, cl, pr = tmp_path / "frame_recognitions.pkl", tmp_path / "gt.json", tmp_path / "classes.json", tmp_path / "predicates.json"
    with open(pred, "wb") as f:
        pickle.dump(cs["frame_recognitions"], f)
    for path, obj in ((gt, cs["groundtruth"]), (cl, cs["classes"]), (pr, dict((n, i) for i, n in enumerate(cs["predicates"])))):
        with open(path, "w") as f:
            json.dump(obj, f)
    res = eval_recognition.main(["--prediction", str(pred), "--groundtruth", str(gt), "--classes", str(cl), "--predicates", str(pr),
                                 "--cpu"])
    want = recognition.result_of(pk, out[4], out[5])
    assert json.dumps(recognition.to_json(res), sort_keys=True) == json.dumps(recognition.to_json(want), sort_keys=True)
    text = capsys.readouterr().out
    assert "predicate recognition accurancy@5: {}".format(want["pre"][5]) in text and "object #15 acc@5 : " in text
    assert "Number of videos in ground truth: 30" in text
