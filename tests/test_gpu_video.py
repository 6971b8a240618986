"""Video relations on the MI355X: csrc/video.hip (ops.video_associate, ops.video_viou_match) against the reference's results
(tests/golden/video_*.npz), against the host implementation on fresh videos, run to run, and through video_sgg_emb.py."""
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


def test_two_runs_give_the_same_bits(inputs, reference):
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


def test_malformed_tables_are_reported_not_followed():
    from i2vsgg_amd import _lib, ops
    frame_off, frame_no = np.array([0, 2], np.int32), np.array([0, 1], np.int32)
    pred_off = np.array([0, 1, 2], np.int32)
    score, trip, boxes = np.array([0.5, 0.5]), np.ones((2, 3), np.int32), np.tile([0.0, 0.0, 9.0, 9.0], (2, 2))
    rel_id, _, rel_len, _, n_rel = ops.video_associate(frame_off, frame_no, pred_off, score, trip, boxes, device="cuda:0")
    assert n_rel.tolist() == [1] and rel_id.tolist() == [0, 0] and rel_len.tolist()[0] == 2
    with pytest.raises(_lib.I2VError):
        ops.video_associate(np.array([0, 5], np.int32), frame_no, pred_off, score, trip, boxes, device="cuda:0")


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
