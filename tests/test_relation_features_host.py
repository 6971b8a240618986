"""Video relation features on the host: the numpy form of the pooling against the reference's own function (golden), against
numpy's mean and against the spelled-out rule; packing, files and edges.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import relation_feature_cases as cases  # noqa: E402
from relation_feature_cases import GOLDEN, bits, load_golden  # noqa: E402
from i2vsgg_amd import relation_features as rf  # noqa: E402
from i2vsgg_amd import video  # noqa: E402

CASES = cases.kernel_cases()


def test_golden_from_the_reference_function_bit_for_bit():
    assert os.path.getsize(GOLDEN) < 200 * 1024
    dims, skipped, shuffled = set(), 0, False
    for store, relations, want in load_golden():
        dims.add(store.dim)
        pooled = rf.pool(relations, store)
        mem_off, mem_slot, _, ids = rf.pack(relations, store)
        skipped += int((mem_slot < 0).sum())
        keys = list(store.table)
        shuffled |= keys != sorted(keys)
        assert len(ids) == len(want) > 0
        for vid, rels in relations.items():
            assert len(rels) <= 40
            for pno in range(len(rels)):
                got, count = pooled[vid][pno]
                assert count >= 1
                assert np.array_equal(bits(got), bits(want[(vid, pno)])), (vid, pno)
    assert dims == {8, 300} and skipped > 0 and shuffled


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_form_is_the_rule_and_numpy_mean(name):
    case = CASES[name]
    pooled, count, status = rf.pool_arrays_host(case["feat"], case["slot_off"], case["mem_off"], case["mem_slot"], case["mem_idx"])
    want, want_count = cases.expected(case)
    assert status == 0 and np.array_equal(count, want_count)
    assert np.array_equal(bits(pooled), bits(want))
    if case["dim"] >= 2:      # a single column is a contiguous vector to numpy: summed pairwise, not in member order
        for r in range(len(count)):
            rows = cases.rows_of(case, r)
            if len(rows):
                ref = np.array([case["feat"][i] for i in rows]).mean(axis=0)                 # lib/utils.py:126
                assert ref.dtype == np.float32 and np.array_equal(bits(pooled[r]), bits(ref)), r


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_depend_on_the_member_order(name):
    seen, differ = cases.assert_order_sensitive(CASES[name])
    if name in ("dim300", "dim8", "dim6", "some_skipped", "first_skipped", "thousand_relations"):
        assert seen >= 5 and differ >= 1


def test_first_valid_row_starts_the_sum():
    case = CASES["first_skipped"]
    assert (case["mem_slot"][case["mem_off"][:-1][np.diff(case["mem_off"]) > 0]] == -1).all()
    pooled, count, _ = rf.pool_arrays_host(case["feat"], case["slot_off"], case["mem_off"], case["mem_slot"], case["mem_idx"])
    assert np.array_equal(count, np.maximum(np.diff(case["mem_off"]) - 2, 0))


def _store(rows_by_key, dim):
    store = rf.HostStore(dim)
    for key, rows in rows_by_key.items():
        store.append(key, rows)
    return store


def test_edges(tmp_path):
    rng = np.random.default_rng(3)
    a, b = cases.values(rng, (3, 5)), cases.values(rng, (2, 5))
    neg = np.full((1, 5), -0.0, np.float32)
    store = _store({("v", 0): a, ("v", 1): b, ("v", 3): neg}, 5)
    rels = {"v": [{"triplet": [1, 7, 2], "duration": [0, 2], "rel_idex": [2, 1]},          # two relations share row a[2]
                  {"triplet": [1, "ride", 2], "duration": [0, 3], "rel_idex": [2, 0, 5]},  # frame 2 has no slot: skipped
                  {"triplet": [1, 7, 2], "duration": [2, 3], "rel_idex": [0]},             # no frame of its own: count 0
                  {"triplet": [1, 7, 2], "duration": [3, 4], "rel_idex": [0]}],            # a single -0.0 member
            "w": []}
    pooled = rf.pool(rels, store)
    assert [c for _, c in pooled["v"]] == [2, 2, 0, 1] and pooled["w"] == []
    assert np.array_equal(bits(pooled["v"][0][0]), bits((a[2] + b[1]) / np.float32(2)))
    assert np.array_equal(bits(pooled["v"][1][0]), bits((a[2] + b[0]) / np.float32(2)))
    assert np.array_equal(bits(pooled["v"][2][0]), bits(np.zeros(5)))
    assert np.signbit(pooled["v"][3][0]).all() and (pooled["v"][3][0] == 0).all()
    written, skipped = rf.write(pooled, rels, str(tmp_path), names=dict((k, "pred%d" % k) for k in range(9)))
    assert (written, skipped) == (3, 1)
    assert sorted(os.path.relpath(os.path.join(d, f), str(tmp_path)) for d, _, fs in os.walk(str(tmp_path)) for f in fs) == [
        "pred7/v_0.npy", "pred7/v_3.npy", "ride/v_1.npy"]
    assert np.array_equal(bits(np.load(str(tmp_path / "ride" / "v_1.npy"))), bits(pooled["v"][1][0]))
    # a rel_idex of the wrong length raises at packing
    with pytest.raises(ValueError, match="rel_idex has 1 entries"):
        rf.pack({"v": [{"triplet": [1, 7, 2], "duration": [0, 2], "rel_idex": [0]}]}, store)
    # an empty relation list
    mem_off, mem_slot, mem_idx, ids = rf.pack({}, store)
    p, c, st = rf.pool_arrays_host(store.feat, store.slot_off, mem_off, mem_slot, mem_idx)
    assert mem_off.tolist() == [0] and ids == [] and p.shape == (0, 5) and c.shape == (0,) and st == 0 and rf.pool({}, store) == {}


def test_out_of_range_entries_give_the_status_and_leave_the_neighbours():
    case = cases.make_case(31, 8, [4, 6, 5, 3, 7])
    clean = rf.pool_arrays_host(case["feat"], case["slot_off"], case["mem_off"], case["mem_slot"], case["mem_idx"])
    n_slots = len(case["slot_off"]) - 1

    def run(**changes):
        arrays = dict((k, case[k].copy()) for k in ("slot_off", "mem_off", "mem_slot", "mem_idx"))
        for k, (i, v) in changes.items():
            arrays[k][i] = v
        return rf.pool_arrays_host(case["feat"], **arrays)

    m = int(case["mem_off"][1]) + 2                                                          # a member of relation 1
    past = int(np.diff(case["slot_off"])[case["mem_slot"][m]])
    # (change, the relation it breaks, the relations it leaves as they were); a decreasing mem_off breaks relation 2 (its end
    # lies before its start) and gives relation 3 other members
    for changes, bad, same in (({"mem_idx": (m, past)}, 1, (0, 2, 3, 4)), ({"mem_idx": (m, -1)}, 1, (0, 2, 3, 4)),
                               ({"mem_slot": (m, n_slots)}, 1, (0, 2, 3, 4)), ({"mem_slot": (m, -2)}, 1, (0, 2, 3, 4)),
                               ({"mem_off": (3, int(case["mem_off"][2]) - 1)}, 2, (0, 1, 4))):
        pooled, count, status = run(**changes)
        assert status == bad + 1, (changes, status)
        assert count[bad] == 0 and not pooled[bad].any()
        for r in same:
            assert count[r] == clean[1][r] and np.array_equal(bits(pooled[r]), bits(clean[0][r]))
    # through pool(): the relation is named
    store = _store({("v", 0): cases.values(np.random.default_rng(1), (2, 4))}, 4)
    with pytest.raises(ValueError, match="outside its frame's pairs"):
        rf.pool({"v": [{"triplet": [0, 0, 0], "duration": [0, 1], "rel_idex": [2]}]}, store)


def test_script_from_files_equals_pool_on_the_arrays(tmp_path):
    import pool_relation_features as script
    store, relations, _ = load_golden()[0]
    feats, out = str(tmp_path / "feats"), str(tmp_path / "video")
    assert rf.save_frame_feats(store, feats) == len(store.table)
    again = rf.from_files(feats)
    assert sorted(again.table) == list(again.table) == sorted(store.table)                   # a different slot order, the same rows
    with open(str(tmp_path / "video_relations.json"), "w") as f:
        json.dump(relations, f)
    script.main(["--relations", str(tmp_path / "video_relations.json"), "--frame_feats", feats, "--save_videofeat_path", out, "--cpu"])
    pooled = rf.pool(relations, store)
    n = 0
    for vid, rels in relations.items():
        for pno, rel in enumerate(rels):
            got = np.load(os.path.join(out, rel["triplet"][1], "%s_%d.npy" % (vid, pno)))
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(pooled[vid][pno][0]))
            n += 1
    assert n == sum(len(r) for r in relations.values()) > 0


def test_filled_frames_have_no_slot():
    """from_frame_results -> associate -> pack: a frame that fill_empty_frames filled from its neighbour takes part in the
    relation (duration, rel_idex) but has no features of its own: its member is -1."""
    box_s, box_o = [10.0, 10.0, 50.0, 60.0], [30.0, 20.0, 90.0, 80.0]

    def frame(conf):
        labels = np.zeros((100, 3)); labels[0] = [2, 5, 3]
        sub, obj = np.zeros((100, 4)), np.zeros((100, 4))
        sub[0], obj[0] = box_s, box_o
        return labels, np.array([conf], np.float32), sub, obj, np.array([1], np.int64)

    results, index = {}, {}
    for k in range(12):
        path = "frame%02d.jpg" % k
        results[path] = (None,) * 5 if k == 5 else frame(0.5 + k / 64.0)
        index[path] = ("0", k)
    relations = video.associate(video.from_frame_results(results, index))
    assert len(relations["0"]) == 1 and relations["0"][0]["duration"] == [0, 12] and len(relations["0"][0]["rel_idex"]) == 12
    store = rf.HostStore(4)
    rng = np.random.default_rng(5)
    for path, res in results.items():
        if res[1] is not None:                                                               # the frame's result is not the five Nones
            store.append(path, cases.values(rng, (2, 4)))
    store.rekey(index)
    mem_off, mem_slot, mem_idx, ids = rf.pack(relations, store)
    assert ids == [("0", 0)] and mem_off.tolist() == [0, 12]
    assert (mem_slot >= 0).tolist() == [k != 5 for k in range(12)] and mem_slot[5] == -1 and (mem_idx == 1).all()
    pooled = rf.pool(relations, store)
    rows = np.array([store.rows_of(("0", k))[1] for k in range(12) if k != 5])
    assert pooled["0"][0][1] == 11 and np.array_equal(bits(pooled["0"][0][0]), bits(cases.sequential_mean(rows)))


def test_arena_rows_counts_ordered_pairs():
    gt = {"a": {"boxes": [[0, 0, 1, 1]] * 3}, "b": {"boxes": [[0, 0, 1, 1]]}, "c": {"boxes": []}, "d": {"boxes": [[0, 0, 1, 1]] * 2}}
    assert rf.arena_rows(gt, ["a", "b", "c", "d"]) == 6 + 2
    with pytest.raises(SystemExit, match="feat_arena_mb"):
        rf.arena_for(gt, ["a", "d"], 300, "cpu", limit_mb=0.001)


def test_feature_block_sets_and_clears_the_sink():
    from i2vsgg_amd import eval as ev
    sink = rf.ArenaSink("cpu")
    assert ev._FEATURE_SINK[0] is None
    with pytest.raises(ZeroDivisionError):
        with ev.keeping_relation_features(sink) as s:
            assert s is sink and ev._FEATURE_SINK[0] is sink and sink.arena is None
            with pytest.raises(RuntimeError, match="active already"):
                with ev.keeping_relation_features(rf.ArenaSink("cpu")):
                    pass
            1 / 0
    assert ev._FEATURE_SINK[0] is None                   # cleared on the way out of a failed loop too


def test_binding_refuses_bad_arguments_without_a_gpu():
    """Only the argument validation in front of the launch runs."""
    import ctypes
    from i2vsgg_amd import _lib
    L, p = _lib.lib, ctypes.c_void_p(256)
    assert L.i2v_version() >= 108 and L.i2v_relation_feature_pool_workspace_bytes(10) >= 4
    assert L.i2v_relation_feature_pool(p, None, p, p, p, 4, 1, 1, 1, 8, p, p, p, 256, None) == -1 and b"null" in L.i2v_last_error()
    assert L.i2v_relation_feature_pool(p, p, p, p, p, 4, 1, 1, 1, 0, p, p, p, 256, None) == -1 and b"dim" in L.i2v_last_error()
    assert L.i2v_relation_feature_pool(p, p, p, p, p, 4, 1, 1, 1, 8, p, p, p, 3, None) == -1 and b"workspace" in L.i2v_last_error()
