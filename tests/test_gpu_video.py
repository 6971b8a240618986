"""Video relations on the MI355X: csrc/video.hip (ops.video_associate, ops.video_viou_match) against the reference's results
(tests/golden/video_*.npz), against the host implementation on fresh videos and on evaluation sets with the matcher's edges
built in (video_golden.eval_edge_set), run to run, and through video_sgg_emb.py."""
import copy
import json
import os
import pickle

import numpy as np
import pytest

from conftest import golden, record_margin
import video_golden as vg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    return vg.cases()


@pytest.fixture(scope="module")
def reference(inputs):
    return vg.reference_relations(golden("video_association"), inputs)


def test_device_association_matches_the_reference(inputs, reference):
    """Every golden video in one launch."""
    from i2vsgg_amd import video
    got = video.associate(copy.deepcopy(inputs), device="cuda:0")
    vg.assert_same_relations(got, reference, "test_device_association_matches_the_reference", record_margin)


def test_device_association_matches_the_host_form_on_fresh_videos():
    """64 seeded videos of 30-600 frames, about 10 000 frames, generic float boxes, one launch; the kernel's per-prediction
    relation ids, and per relation start, length and score, equal the host implementation's bit for bit.  The videos come
    through vg.fresh_videos, which re-draws a video whose host decisions come within 1e-9 (relative) of a threshold and
    asserts that at most 5 % of the draws are rejected.  Rate seen on the CPU with the host form: 1 of 65 draws rejected
    (10 032 frames; smallest margin kept 8.1e-9), drawing and host association together about 42 s."""
    import torch
    from i2vsgg_amd import ops, video
    frames, host, info = vg.fresh_videos(20260, 64)
    record_margin("test_device_association_matches_the_host_form_on_fresh_videos", "draws rejected", info["rejected"],
                  0.05 * info["draws"])
    assert sum(len(f) for f in frames.values()) > 8000
    pk = video.pack_frames(copy.deepcopy(frames))
    want = video.associate_arrays_host(pk)
    got = [t.cpu().numpy() for t in ops.video_associate(pk.frame_off, pk.frame_no, pk.pred_off, pk.score, pk.triplet, pk.boxes,
                                                        device="cuda:0")]
    assert (got[4] == want[4]).all() and (got[0] == want[0]).all()
    for v in range(len(pk.vids)):
        base, n = int(pk.pred_off[pk.frame_off[v]]), int(want[4][v])
        for k in (1, 2, 3):
            assert (got[k][base:base + n] == want[k][base:base + n]).all(), (pk.vids[v], k)
    dev = video.associate(copy.deepcopy(frames), device="cuda:0")
    assert dev == host
    torch.cuda.synchronize()


def test_device_viou_match_matches_the_reference(reference):
    from i2vsgg_amd import video
    g = golden("video_eval")
    gts = vg.groundtruth(g, reference)
    thr = float(g["viou_threshold"])
    pe, ov, hit, hit_ov = video.match(reference, gts, thr, device="cuda:0")
    assert pe.vids == g["vids"].tolist()
    seen = ~np.isnan(g["ov"])
    assert (ov[seen] >= 0).all()
    rel = np.abs(ov[seen] - g["ov"][seen]) / np.maximum(g["ov"][seen], 1e-300)
    rel[g["ov"][seen] == ov[seen]] = 0
    record_margin("test_device_viou_match_matches_the_reference", "relative ov difference", rel.max(), 1e-12)
    assert rel.max() <= 1e-12
    assert (hit == g["hit"]).all()
    rows = np.nonzero(hit >= 0)[0]
    assert len(rows) > 50 and (hit_ov[rows] == ov[rows, hit[rows]]).all() and (hit_ov[hit < 0] == -1).all()
    mean_ap, rec, mprec = video.evaluate(reference, gts, thr, device="cuda:0")
    got = np.array([mean_ap, rec[50], rec[100], mprec[1], mprec[5], mprec[10]], np.float64)
    record_margin("test_device_viou_match_matches_the_reference", "largest metric difference", np.abs(got - g["metrics"]).max(), 1e-6)
    assert np.abs(got - g["metrics"]).max() <= 1e-6


@pytest.fixture(scope="module")
def grid_set():
    """The edge set on the quarter-pixel grid (every sum exact), packed once; the host form's result per threshold."""
    from i2vsgg_amd import video
    pred, gts = vg.eval_edge_set(vg.EDGE_SEED, grid=True)
    pe = video.pack_eval(pred, gts)
    return pred, gts, pe, dict((thr, video.match_arrays_host(pe, thr)) for thr in (0.0, 0.5, 0.75))


def _device_match(pe, thr):
    from i2vsgg_amd import ops
    return [t.cpu().numpy() for t in ops.video_viou_match(pe.pred_off, pe.pred_rel, pe.pred_score, pe.gt_off, pe.gt_rel, pe.boxes,
                                                          thr, device="cuda:0")]


@pytest.mark.parametrize("thr", [0.0, 0.5, 0.75])
def test_device_matcher_on_the_edge_set(grid_set, thr):
    """vg.eval_edge_set on the grid: 200 predictions against 150 ground truths (detected bits 1 and 2 of a lane), duplicate
    annotations in neighbouring lanes and in one lane, tied scores, overlaps of exactly 0.5, 0.75 and 0, trajectories of 1,
    63, 64, 65, 128 and 600 boxes and trajectories shorter than their durations.  ov, hit and hit_ov equal the host form's
    bit for bit; the coverage is asserted on what the device returned."""
    from i2vsgg_amd import video
    name = "test_device_matcher_on_the_edge_set"
    pred, gts, pe, host = grid_set
    ov, hit, hit_ov = _device_match(pe, thr)
    want = host[thr]
    assert ov.shape == want[0].shape and (ov.view(np.int64) == want[0].view(np.int64)).all()
    assert (hit == want[1]).all()
    assert (hit_ov.view(np.int64) == want[2].view(np.int64)).all()
    # coverage, on the device's own output
    w = hit[:200]
    assert vg.edge_rows(pe, "wide") == 0 and (w > 63).any() and (w > 127).any() and (w < 0).any()
    if thr == 0.5:                                       # the best candidate is taken: the second best, or nothing
        for j, a in enumerate(vg.EDGE_FALLBACK):
            assert w[a] == a and int(ov[150 + j].argmax()) == a and ov[150 + j, a + 3] >= thr
            assert (w[150 + j], w[a + 3]) == ((a + 3, -1) if j % 2 == 0 else (-1, a + 3))
    p0 = vg.edge_rows(pe, "twins")
    assert hit[p0:p0 + 4].tolist() == [5, 6, 67, 3]      # the generator asserts ov >= 0.75 on these four rows
    assert (hit_ov[p0:p0 + 2] == ov[p0:p0 + 2, 5]).all() and (hit_ov[p0 + 2:p0 + 4] == ov[p0 + 2:p0 + 4, 3]).all()
    left = ov[p0 + 4].copy()                             # the third prediction over the first pair: both twins are taken
    left[[5, 6]] = -1
    assert left.max() >= 0 and (left < 0.5).all()
    assert hit[p0 + 4] == (int(left.argmax()) if thr == 0.0 else -1)     # the first of the best that are left, ov 0 included
    p0 = vg.edge_rows(pe, "tied")
    for k in range(3):                                   # a group's first member in list order that reaches the threshold
        reach = [i for i in (k, k + 3, k + 6) if ov[p0 + i, k] >= thr]
        assert thr > 0.5 or reach[0] == k                # the generator asserts ov >= 0.5 of every member
        assert [hit[p0 + i] for i in (k, k + 3, k + 6)] == [k if reach and i == reach[0] else -1 for i in (k, k + 3, k + 6)]
    p0 = vg.edge_rows(pe, "exact")
    assert ov[p0:p0 + 3, :3].diagonal().tolist() == [0.5, 0.75, 0.0]
    assert hit[p0:p0 + 5].tolist() == {0.0: [0, 1, 2, 3, 4], 0.5: [0, 1, -1, -1, -1], 0.75: [-1, 1, -1, -1, -1]}[thr]
    assert hit_ov[p0 + 1] == 0.75 and hit_ov[p0 + 2] == (0.0 if thr == 0.0 else -1.0)
    p0 = vg.edge_rows(pe, "nomatch")
    assert (ov[p0:p0 + 4] == -1).all() and (hit[p0:p0 + 4] == -1).all()
    p0 = vg.edge_rows(pe, "clamped")
    assert ov[p0 + 2, 2] == 0.0 and (ov[p0:p0 + 4, :4].diagonal()[[0, 1, 3]] > 0).all()
    # the metrics: the device path returns exactly what the host path returns
    dev, cpu = video.evaluate(pred, gts, thr, device="cuda:0"), video.evaluate(pred, gts, thr, device=None)
    assert dev[0] == cpu[0] and dev[1] == cpu[1] and dev[2] == cpu[2]
    if thr in (0.0, 0.5):                                # the reference ran these two, without `clamped`
        tag = "%02d" % int(100 * thr)
        without = dict((k, v) for k, v in pred.items() if k != "clamped"), dict((k, v) for k, v in gts.items() if k != "clamped")
        vg.assert_edge_golden(golden("video_eval_edges"), tag, pe, ov, hit, video.evaluate(*without, viou_threshold=thr, device="cuda:0"),
                              name, record_margin)


def test_device_matcher_on_generic_boxes():
    """Three edge sets with generic double boxes (no `exact` video, `clamped` included) at threshold 0.5: equal hits, ov within
    4 L 2**-53 relative of the host form's, L the longest trajectory of the set: the two volumes and the intersection are
    sums of at most L positive terms, each within (L - 1) 2**-53 of exact in any order, and v1 + v2 - inter >= inter, so
    the quotient amplifies the three by at most 3; one more rounding for the division.  A set whose host decisions come
    within 1e-9 (relative) of the threshold or of each other is drawn again (vg.fresh_edge_sets) and at most 5 % of the draws
    may be rejected.  Seen on the CPU with the host form alone: 0 of 3 draws rejected from this seed, smallest margin kept
    0.174; 0 of 40 from seed 9000, smallest margin 0.156 -- the sets are built, not sampled, and their overlaps lie well
    away from 0.5.  With three draws the 5 % cap means no rejection at all; the 40 draws are the evidence for the rate."""
    name = "test_device_matcher_on_generic_boxes"
    sets, info = vg.fresh_edge_sets(7200, 3)
    record_margin(name, "draws rejected", info["rejected"], 0.05 * info["draws"])
    worst = 0.0
    for pe, (h_ov, h_hit, h_hit_ov) in sets:
        L = int(max(pe.pred_rel[:, [7, 9]].max(), pe.gt_rel[:, [7, 9]].max()))
        assert L >= 600
        bound = 4 * L * 2.0 ** -53
        ov, hit, hit_ov = _device_match(pe, 0.5)
        assert (hit == h_hit).all() and (hit > 127).any()
        assert ((ov < 0) == (h_ov < 0)).all() and (ov[h_ov < 0] == -1).all()
        assert ((ov == 0) == (h_ov == 0)).all()
        pos = h_ov > 0
        ratio = (np.abs(ov[pos] - h_ov[pos]) / h_ov[pos]).max() / bound
        worst = max(worst, ratio)
        rows = hit >= 0
        assert (hit_ov[rows] == ov[rows, hit[rows]]).all() and (hit_ov[~rows] == -1).all()
    record_margin(name, "ov difference / (4 L 2^-53)", worst, 1.0)
    assert worst <= 1.0


def test_two_runs_give_the_same_bits(inputs, reference, grid_set):
    from i2vsgg_amd import ops, video
    pk = video.pack_frames(copy.deepcopy(inputs))
    run = lambda: [t.cpu().numpy() for t in ops.video_associate(pk.frame_off, pk.frame_no, pk.pred_off, pk.score, pk.triplet,
                                                               pk.boxes, device="cuda:0")]
    a, b = run(), run()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    g = golden("video_eval")
    pe = video.pack_eval(reference, vg.groundtruth(g, reference))
    run = lambda: [t.cpu().numpy() for t in ops.video_viou_match(pe.pred_off, pe.pred_rel, pe.pred_score, pe.gt_off, pe.gt_rel,
                                                                 pe.boxes, 0.5, device="cuda:0")]
    a, b = run(), run()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    a, b = _device_match(grid_set[2], 0.5), _device_match(grid_set[2], 0.5)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_malformed_tables_are_reported_not_followed():
    from i2vsgg_amd import _lib, ops
    frame_off, frame_no = np.array([0, 2], np.int32), np.array([0, 1], np.int32)
    pred_off = np.array([0, 1, 2], np.int32)
    score, trip, boxes = np.array([0.5, 0.5]), np.ones((2, 3), np.int32), np.tile([0.0, 0.0, 9.0, 9.0], (2, 2))
    rel_id, _, rel_len, _, n_rel = ops.video_associate(frame_off, frame_no, pred_off, score, trip, boxes, device="cuda:0")
    assert n_rel.tolist() == [1] and rel_id.tolist() == [0, 0] and rel_len.tolist()[0] == 2
    with pytest.raises(_lib.I2VError):
        ops.video_associate(np.array([0, 5], np.int32), frame_no, pred_off, score, trip, boxes, device="cuda:0")


def test_malformed_matcher_tables_are_reported_not_followed():
    """video_match_kernel refuses an offset table that leaves its arrays (the status word, raised as I2VError);
    video_viou_kernel gives a prediction of a video that does not exist a row of -1; vm_span counts a trajectory that leaves
    the box array as empty."""
    from i2vsgg_amd import _lib, ops
    box = np.array([[0.0, 0.0, 9.0, 9.0], [0.0, 0.0, 9.0, 19.0], [50.0, 50.0, 59.0, 59.0]])
    row = lambda v, t, sub, obj: [v, t, t, t, 0, 1, sub, 1, obj, 1]
    pred_rel = np.array([row(0, 1, 0, 0), row(0, 2, 2, 2), row(1, 1, 0, 0)], np.int32)
    gt_rel = np.array([row(0, 1, 0, 0), row(0, 2, 0, 0), row(1, 1, 1, 0)], np.int32)
    pred_off, gt_off, score = np.array([0, 2, 3], np.int32), np.array([0, 2, 3], np.int32), np.array([0.5, 0.25, 0.75])
    call = lambda **k: [t.cpu().numpy() for t in ops.video_viou_match(k.get("pred_off", pred_off), k.get("pred_rel", pred_rel), score,
                                                                      k.get("gt_off", gt_off), k.get("gt_rel", gt_rel), box, 0.5,
                                                                      device="cuda:0")]
    ov, hit, hit_ov = call()
    assert ov.tolist() == [[1.0, -1.0], [-1.0, 0.0], [0.5, -1.0]] and hit.tolist() == [0, -1, 0] and hit_ov.tolist() == [1.0, -1.0, 0.5]
    with pytest.raises(_lib.I2VError):                   # the second video's predictions run past the three there are
        call(pred_off=np.array([0, 2, 5], np.int32))
    with pytest.raises(_lib.I2VError):                   # a decreasing ground-truth table
        call(gt_off=np.array([0, 2, 1], np.int32))
    for v in (2, -1, 1 << 30):                           # a video that does not exist: no overlap is computed, nothing is hit
        bad = pred_rel.copy()
        bad[0, 0] = v
        ov, hit, hit_ov = call(pred_rel=bad)
        assert (ov[0] == -1).all() and hit[0] == -1 and hit_ov[0] == -1 and hit[2] == 0
    for off, n in ((2, 2), (3, 1), (-1, 1), (0, -1), (0x7fffffff, 0x7fffffff)):      # (offset, length) leaves the three boxes
        bad = pred_rel.copy()
        bad[0, 6:8] = off, n
        ov, hit, hit_ov = call(pred_rel=bad)
        assert ov[0].tolist() == [0.0, -1.0] and hit[0] == -1                         # an empty subject: ov 0 / 100
        assert ov[2].tolist() == [0.5, -1.0] and hit.tolist()[1:] == [-1, 0]
        bad = gt_rel.copy()
        bad[0, 8:10] = off, n
        ov, hit, hit_ov = call(gt_rel=bad)
        assert ov[0].tolist() == [0.0, -1.0] and hit.tolist() == [-1, -1, 0]


def test_script_writes_video_relations(tmp_path):
    """video_sgg_emb.py --frames_per_video 8 (test_sgg_emb.py's frame loop, then the association on the GPU) writes a
    video_relations.json that the host form reproduces from the same run's relations.pkl; a run of test_sgg_emb.py alone writes
    no such file and a relations.pkl with the same arrays, bit for bit.  With 8 frames each video is short of the 10
    members a relation needs; the whole imdb as one video (10 frames) is run too, from the pickle."""
    from i2vsgg_amd import video
    import test_sgg_emb as tr
    import video_sgg_emb as tv
    from i2vsgg_amd._lib import TUNE, lib
    outs = []
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)        # no split-K atomics: two forwards of a frame are bit-equal
        for name, run, extra in (("with", tv.main, ["--frames_per_video", "8"]), ("without", tr.main, [])):
            out = str(tmp_path / name)
            run(["--imdbval_name", "synthetic_10_v", "--scale", "192", "--frames", "3", "--output_dir", out] + extra)
            outs.append(os.path.join(out, "res101", "synthetic"))
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
    with open(os.path.join(outs[0], "relations.pkl"), "rb") as f:
        first = pickle.load(f)
    with open(os.path.join(outs[1], "relations.pkl"), "rb") as f:
        second = pickle.load(f)
    assert not os.path.exists(os.path.join(outs[1], "video_relations.json"))
    assert set(first) == set(second) and len(first) == 10      # the loader's order is not part of the file's meaning
    for k in first:
        for a, b in zip(first[k], second[k]):
            assert (a is None and b is None) or np.asarray(a).tobytes() == np.asarray(b).tobytes()
    with open(os.path.join(outs[0], "video_relations.json")) as f:
        written = json.load(f)
    paths = sorted(first)
    again = video.associate(video.from_frame_results(first, lambda p: (str(paths.index(p) // 8), paths.index(p) % 8)), device=None)
    assert written == json.loads(json.dumps(again))
    assert len(written) == (len(paths) + 7) // 8
    # the whole imdb as one video, from the pickle: device and host form write the same file
    one = tv.main(["--relations", os.path.join(outs[0], "relations.pkl")])
    with open(os.path.join(outs[0], "video_relations.json")) as f:
        assert json.load(f) == json.loads(json.dumps(one))
    by_path = dict((p, first[p]) for p in paths)
    assert one == video.associate(video.from_frame_results(by_path), device=None) and list(one) == ["0"]
