"""The track mode of the video association on the MI355X: video_associate_tracks_kernel (csrc/video.hip) against the host form
on a mixed batch, with its open table at the bound, run to run, on malformed tables, and through video_sgg_emb.py.  Equality is
equality of bits: the kernel's only floating-point work is one lane's sequence of adds per relation."""
import copy
import json
import os
import pickle

import numpy as np
import pytest

import track_association_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAPS = [0, 1, 3, 7]


@pytest.fixture(scope="module")
def batch():
    from i2vsgg_amd import video
    rel, tracks = tc.mixed_batch()
    return rel, tracks, video.pack_track_frames(rel, tracks)


def _device(t, G, **kw):
    from i2vsgg_amd import ops
    args = t.args() if hasattr(t, "args") else (t.frame_off, t.frame_no, t.pred_off, t.score, t.key, t.since)
    return [x.cpu().numpy() for x in ops.video_associate_tracks(*args, max_gap=G, device=DEV, **kw)]


def _same(got, want, t):
    """rel_id and n_rel everywhere; start, end, length and score (by its bits) over each video's n_rel entries."""
    assert (got[5] == want[5]).all() and (got[0] == want[0]).all()
    for v in range(len(t.frame_off) - 1):
        base, n = int(t.pred_off[t.frame_off[v]]), int(want[5][v])
        for k in (1, 2, 3):
            assert (got[k][base:base + n] == want[k][base:base + n]).all(), (v, k)
        assert (got[4][base:base + n].view(np.int64) == want[4][base:base + n].view(np.int64)).all(), v


@pytest.mark.parametrize("G", GAPS)
def test_device_form_matches_the_host_form(batch, G):
    """24 seeded videos in ONE launch (track_association_cases.mixed_batch: 2752 frames, 242 573 predictions; videos of 30-300
    frames, one without a frame, one of one frame, one whose frames are all empty; frames of 0, 1, 99 and 100 predictions;
    frame-number gaps; tracks that leave for 1-9 frames; scores on a grid of 1/64 in every second video; the same keys in
    every video).  Measured on the CPU, one run: drawing 0.8 s, packing 0.5 s, the host form 0.3 s per gap (one pass of
    array operations per frame), the gather 0.5-0.9 s."""
    from i2vsgg_amd import video
    rel, tracks, pk = batch
    want = video.associate_tracks_arrays_host(pk, G)
    got = _device(pk, G)
    _same(got, want, pk)
    assert int(want[5].sum()) > 10000 and (want[2][:10] - want[1][:10] >= want[3][:10]).all()
    assert video.associate_tracks(copy.deepcopy(rel), tracks, G, DEV) == video.associate_tracks(copy.deepcopy(rel), tracks, G, None)


@pytest.mark.parametrize("G", [7, 3])
def test_the_open_table_at_its_bound(G):
    """One video whose frames cycle through G + 1 disjoint sets of 100 keys for 26 frames: at max_gap = G every key's relation
    spans the video, so 100 * (G + 1) entries (800 at G = 7, the table's size) are open at once; asserted on the device's own
    output.  At max_gap = G - 1 the same video gives 1-member relations only.  A second video of the launch: a key that
    returns after exactly G + 1 frames (extends) and then after G + 2 (a new id), and four keys equal in two of their three
    fields that never merge."""
    period, n_frames = G + 1, 26
    near = [(1, 2, 3), (1, 2, 4), (1, 5, 3), (6, 2, 3)]
    second = [(t, [(k, 0, 0.5) for k in near] + ([((9, 9, 9), 0, 0.25)] if t in (0, G + 1, 2 * G + 3) else []))
              for t in range(2 * G + 4)]
    t = tc.Tables([tc.bound_video(n_frames, period), second])
    rel_id, start, end, length, score, n_rel = _device(t, G)
    assert n_rel.tolist() == [100 * period, 6]
    for f in range(n_frames):
        c = f % period
        ids = rel_id[100 * f:100 * f + 100]
        assert (ids == 100 * c + 99 - np.arange(100)).all(), f         # the frame's ranks: score ascends with k
        frames = np.arange(c, n_frames, period)
        assert (start[ids] == c).all() and (end[ids] == frames[-1] + 1).all() and (length[ids] == len(frames)).all()
        assert len(frames) in (n_frames // period, -(-n_frames // period))
        assert (score[ids].view(np.int64) == ((np.arange(100) + 1) / 128.0).view(np.int64)).all()
    base = 100 * n_frames
    per = [rel_id[t.pred_off[n_frames + f]:t.pred_off[n_frames + f + 1]].tolist() for f in range(2 * G + 4)]
    assert all(p[:4] == [0, 1, 2, 3] for p in per)                      # never merged, never split
    assert (length[base:base + 4] == 2 * G + 4).all() and (start[base:base + 4] == 0).all() and (end[base:base + 4] == 2 * G + 4).all()
    assert per[0][4] == 4 and per[G + 1][4] == 4 and per[2 * G + 3][4] == 5
    assert (start[base + 4], end[base + 4], length[base + 4]) == (0, G + 2, 2) and (start[base + 5], length[base + 5]) == (2 * G + 3, 1)
    from i2vsgg_amd import video
    _same([rel_id, start, end, length, score, n_rel], video.associate_tracks_arrays_host(t, G), t)
    # one frame less of reach: no relation gets a second member
    got = _device(t, G - 1)
    assert got[5][0] == 100 * n_frames and (got[3][:100 * n_frames] == 1).all()
    assert (got[0][:100 * n_frames].reshape(n_frames, 100) == 100 * np.arange(n_frames)[:, None] + 99 - np.arange(100)).all()
    _same(got, video.associate_tracks_arrays_host(t, G - 1), t)


def test_two_runs_give_the_same_bytes(batch):
    pk = batch[2]
    a, b = _device(pk, 3), _device(pk, 3)
    assert len(a) == 6
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_malformed_tables_are_reported_not_followed():
    from i2vsgg_amd import _lib, ops, video
    row = lambda k, s: ((k, 1, 0), 0, s)
    good = [(0, [row(0, 0.5), row(1, 0.25)]), (1, [row(1, 0.75), row(0, 0.5)]), (2, [row(0, 0.5)])]
    other = [(5, [row(3, 0.125)]), (6, [row(3, 0.25), row(4, 0.5)])]
    t = tc.Tables([good, other])
    clean = _device(t, 0)
    assert clean[5].tolist() == [2, 2] and clean[0].tolist() == [0, 1, 1, 0, 0, 0, 0, 1]
    with pytest.raises(_lib.I2VError):                   # the second video's frames run past the five there are
        ops.video_associate_tracks(np.array([0, 3, 9], np.int32), *t.args()[1:], max_gap=0, device=DEV)
    many = tc.Tables([good[:1] + [(1, [row(k, 0.5) for k in range(101)])] + good[2:], other])
    with pytest.raises(_lib.I2VError, match="frame 1"):
        _device(many, 0)
    # a repeated key in one frame: the frame is skipped, the launch raises, and the other video comes out as without it
    twice = tc.Tables([[good[0], (1, [row(1, 0.75), row(1, 0.5)]), good[2]], other])
    with pytest.raises(_lib.I2VError, match="frame 1"):
        _device(twice, 1)
    got, alone = _device(twice, 1, read_status=False), _device(tc.Tables([other]), 1)
    assert got[5].tolist() == [2, 2] and got[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 1]     # key 0 bridges the skipped frame
    assert got[3][:2].tolist() == [2, 1] and (got[1][0], got[2][0]) == (0, 3)
    for k in range(5):
        assert got[k][5:].tobytes() == alone[k].tobytes(), k
    with pytest.raises(ValueError, match="repeats a key"):
        video.associate_tracks_arrays_host(twice, 1)
    with pytest.raises(ValueError, match="max_gap"):
        ops.video_associate_tracks(*t.args(), max_gap=1.5, device=DEV)
    with pytest.raises(_lib.I2VError, match="max_gap"):
        ops.video_associate_tracks(*t.args(), max_gap=8, device=DEV)


def test_script_associates_along_tracks(tmp_path, capsys):
    """video_sgg_emb.py --associate tracks --max_gap 7 on the synthetic imdb (10 frames, small), its annotated boxes pickled with
    tids 0 .. n-1 per frame and passed as --target_gt_rels_path, writes a video_relations.json that the host form reproduces
    from the same run's relations.pkl; --relations ... --tracks ... --cpu writes the same file again; --max_gap without
    --associate tracks exits with a message.  At 10 frames few keys reach 10 members: the content of the result is the other
    tests' matter, here the files are compared and nothing else."""
    import video_sgg_emb as tv
    from i2vsgg_amd import video
    from i2vsgg_amd.model.utils import config as c
    from i2vsgg_amd.roi_data_layer.roidb import combined_roidb
    saved = copy.deepcopy(dict(c.cfg))                   # the script sets the scales in the global cfg: put it back afterwards
    out = str(tmp_path / "out")
    boxes = str(tmp_path / "tracked_boxes.pkl")
    try:
        c.cfg_from_file(c.default_cfg_file("res101"))
        annos = combined_roidb("synthetic_10_v", False)[0].gt_rels(62)
        for a in annos.values():
            a["tids"] = list(range(len(a["boxes"])))
        with open(boxes, "wb") as f:
            pickle.dump(annos, f)
        run = ["--imdbval_name", "synthetic_10_v", "--scale", "192", "--frames", "3", "--output_dir", out, "--target_gt_rels_path", boxes]
        # --frames_per_video is given: the script's first parser would otherwise read "--frames 3" as its abbreviation
        tv.main(run + ["--frames_per_video", "10", "--associate", "tracks", "--max_gap", "7"])
    finally:
        c._merge_a_into_b(c.AttrDict(saved), c.cfg)
    assert "along tracks (max_gap 7, " in capsys.readouterr().out
    where = os.path.join(out, "res101", "synthetic")
    with open(os.path.join(where, "relations.pkl"), "rb") as f:
        results = pickle.load(f)
    with open(os.path.join(where, "video_relations.json")) as f:
        written = json.load(f)
    paths = sorted(results)
    index = dict((p, ("0", k)) for k, p in enumerate(paths))
    again = video.associate_tracks(video.from_frame_results(results, index, annos), annos, 7, None, frame_to_video=index)
    assert written == json.loads(json.dumps(again)) and list(written) == ["0"]
    os.remove(os.path.join(where, "video_relations.json"))
    tv.main(["--relations", os.path.join(where, "relations.pkl"), "--tracks", boxes, "--associate", "tracks", "--max_gap", "7", "--cpu"])
    with open(os.path.join(where, "video_relations.json")) as f:
        assert json.load(f) == written
    with pytest.raises(SystemExit, match="--associate tracks"):
        tv.main(["--relations", os.path.join(where, "relations.pkl"), "--max_gap", "1"])
    with pytest.raises(SystemExit, match="--tracks"):
        tv.main(["--relations", os.path.join(where, "relations.pkl"), "--associate", "tracks"])
