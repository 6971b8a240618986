"""Video relation NMS, host side (no GPU): the host form of i2vsgg_amd.video.suppress against decisions taken from the
reference's viou (tests/golden/video_nms.npz), against a literal restatement of the rules and against answers worked by hand; the
packer's refusals; the new ``max_per_video`` keyword; the end-to-end case; the scripts with ``--cpu``."""
import copy
import json
import os
import pickle

import numpy as np
import pytest

from conftest import golden, record_margin
import video_nms_cases as nc

FRACTIONAL_RTOL = 1e-12      # the reference adds in the same order; what is left is nothing but the bound the issue sets
MARGIN = 1e-9                # no decisive ov of a fractional golden case lies closer to its threshold (relative)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _golden_pk(g, k):
    from i2vsgg_amd import video
    cell_off, rel = g["c%d_cell_off" % k], g["c%d_rel" % k]
    return video.PackedNMS([], None, cell_off, rel, g["c%d_score" % k], g["c%d_boxes" % k], None, None, None)


def test_host_form_equals_the_reference_decisions():
    """keep / by from the reference's viou table are the host form's; by_ov in every bit on the integer cases, within 1e-12 on
    the two fractional ones, whose decisive overlaps keep 1e-9 from the threshold."""
    from i2vsgg_amd import video
    g = golden("video_nms")
    n = int(g["n_cases"])
    assert n == nc.GOLDEN_CASES and float(g["margin_bound"]) == MARGIN
    worst, smallest = 0.0, np.inf
    for k in range(n):
        case = nc.golden_case(k, int(g["c%d_seed" % k]))
        pk = video.pack_nms(case.prediction, case.pool)                      # the built inputs are the recorded ones
        for name in ("cell_off", "rel", "boxes", "score"):
            assert getattr(pk, name).tobytes() == g["c%d_%s" % (k, name)].tobytes(), (k, name)
        T = float(g["c%d_T" % k])
        assert T == case.T
        st = {}
        keep, by, by_ov, _ = video.suppress_arrays_host(_golden_pk(g, k), T, st)
        assert (keep == g["c%d_keep" % k]).all() and (by == g["c%d_by" % k]).all(), k
        ref = g["c%d_by_ov" % k]
        if k < n - 2:
            assert (_bits(by_ov) == _bits(ref)).all(), k
        else:
            hit = by >= 0
            assert hit.any() and (by_ov[~hit] == -1.0).all()
            err = np.abs(by_ov[hit] - ref[hit]) / ref[hit]
            worst = max(worst, float(err.max()))
            smallest = min(smallest, st["ov"])
            assert err.max() <= FRACTIONAL_RTOL, (k, err.max())
            assert st["ov"] >= MARGIN and float(g["margin"][k]) >= MARGIN
    record_margin("test_host_form_equals_the_reference_decisions", "fractional cases: by_ov vs the reference, largest rel. difference", worst,
                  FRACTIONAL_RTOL)
    record_margin("test_host_form_equals_the_reference_decisions", "fractional cases: smallest rel. margin of a decisive ov (at least)",
                  smallest, MARGIN)
    kept = sum(int(g["c%d_keep" % k].sum()) for k in range(n))
    total = sum(len(g["c%d_keep" % k]) for k in range(n))
    assert 0 < kept < total                                                  # the golden suppresses, and not everything


# ---- the rules once more, literally: python floats, one pair at a time ---------------------------------------------------------
def _literal(rels, T, planted=None):
    """``rels``: one video's relations.  -> indices kept, {suppressed index: (by index, ov)}, ranked over ALL of them (no pool)."""
    def vol(t):
        v = 0.0
        for b in t:
            v += ((b[2] - b[0]) + 1) * ((b[3] - b[1]) + 1)
        return v

    def viou(ta, da, tb, db):
        inter = 0.0
        for f in range(max(da[0], db[0]), min(da[1], db[1])):
            a, b = ta[f - da[0]], tb[f - db[0]]
            inter += max(0, (min(a[2], b[2]) - max(a[0], b[0])) + 1) * max(0, (min(a[3], b[3]) - max(a[1], b[1])) + 1)
        return inter / ((vol(ta) + vol(tb)) - inter) if min(da[1], db[1]) > max(da[0], db[0]) else 0.0
    rank = sorted(range(len(rels)), key=lambda i: (-rels[i]["score"], -i if planted == "rank" else i))
    kept, by = [], {}
    for j in rank:
        for i in kept:
            a, b = rels[i], rels[j]
            if a["triplet"] == b["triplet"] and j not in by:
                ov = min(viou(a["sub_traj"], a["duration"], b["sub_traj"], b["duration"]),
                         viou(a["obj_traj"], a["duration"], b["obj_traj"], b["duration"]))
                if ov >= T if planted == "ge" else ov > T:
                    by[j] = (i, ov)
        if j not in by:
            kept.append(j)
    return kept, by


def _host(case):
    """The host form's answer in the literal form's terms, per video."""
    from i2vsgg_amd import video
    pk = video.pack_nms(case.prediction, case.pool)
    keep, by, by_ov, vol = video.suppress_arrays_host(pk, case.T)
    out = {}
    for v, vid in enumerate(pk.vids):
        p0, p1 = int(pk.video_off[v]), int(pk.video_off[v + 1])
        order = p0 + np.argsort(pk.rank[p0:p1], kind="stable")
        kept = [int(pk.src[p]) for p in order if keep[p]]
        sup = dict((int(pk.src[p]), (int(pk.src[by[p]]), float(by_ov[p]))) for p in order if not keep[p])
        out[vid] = (kept, sup)
    return out, pk, vol


CASES = dict((c.name, c) for c in nc.built_cases())
NO_POOL = [n for n, c in CASES.items() if all(len(r) <= c.pool for r in c.prediction.values())]


@pytest.mark.parametrize("name", NO_POOL)
def test_host_form_equals_the_literal_rules(name):
    case = CASES[name]
    got, pk, vol = _host(case)
    for vid, rels in case.prediction.items():
        kept, by = _literal(rels, case.T)
        assert got[vid][0] == kept, vid
        assert set(got[vid][1]) == set(by), vid
        for j, (i, ov) in by.items():
            assert got[vid][1][j][0] == i and _bits(got[vid][1][j][1]) == _bits(ov), (vid, j)
    # the volumes: one python sum per trajectory
    for p in range(0, len(pk.rel), max(1, len(pk.rel) // 50)):
        for which in (0, 1):
            off, n = int(pk.rel[p, 6 + 2 * which]), int(pk.rel[p, 7 + 2 * which])
            v = 0.0
            for b in pk.boxes[off:off + n].tolist():
                v += ((b[2] - b[0]) + 1) * ((b[3] - b[1]) + 1)
            assert _bits(vol[p, which]) == _bits(v)


def test_a_planted_error_is_caught():
    """The comparison above is not blind: suppression with >= differs on the case with ov exactly at T, a non-strict rank on the
    case with equal scores."""
    at, tie = CASES["at_T"], CASES["tie"]
    assert _literal(at.prediction["v"], at.T)[0] == _host(at)[0]["v"][0] == [0, 1]
    assert _literal(at.prediction["v"], at.T, planted="ge")[0] == [0]
    assert _literal(tie.prediction["v"], tie.T)[0] == _host(tie)[0]["v"][0] == [2, 0]
    assert _literal(tie.prediction["v"], tie.T, planted="rank")[0] == [2, 1]
    sizes = CASES["sizes"]                               # and on built data: the coarse score grid has ties inside the cells
    differs = [vid for vid, rels in sizes.prediction.items() if _literal(rels, sizes.T, planted="rank")[0] != _literal(rels, sizes.T)[0]]
    assert differs


@pytest.mark.parametrize("k", range(len(nc.hand_cases())))
def test_hand_cases(k):
    from i2vsgg_amd import video
    case, want = nc.hand_cases()[k]
    out, info = video.suppress(case.prediction, case.T, case.cap, case.pool)
    for vid, idx in want.items():
        assert len(out[vid]) == len(idx) and all(a is case.prediction[vid][i] for a, i in zip(out[vid], idx)), (case.name, vid)
        assert info[vid]["kept"] == len(idx) and info[vid]["candidates"] == min(case.pool, len(case.prediction[vid]))


def test_the_chain():
    """Boxes 20 wide at x = 0, 4, 8 over 3 frames: ov AB = BC = 2/3, AC = 3/7.  At T = 0.5 A suppresses B; C stays, because B is
    not kept; by[B] = A with ov 2/3."""
    from i2vsgg_amd import video
    case = CASES["chain"]
    pk = video.pack_nms(case.prediction, case.pool)
    keep, by, by_ov, vol = video.suppress_arrays_host(pk, 0.5)
    assert keep.tolist() == [1, 0, 1] and by.tolist() == [-1, 0, -1]
    assert by_ov.tolist() == [-1.0, 480.0 / 720.0, -1.0] and (vol == 600.0).all()
    keep, by, by_ov, _ = video.suppress_arrays_host(pk, 0.4)                   # AC = 3/7 > 0.4: A takes both
    assert keep.tolist() == [1, 0, 0] and by.tolist() == [-1, 0, 0] and by_ov[2] == 360.0 / 840.0


def test_cells_and_ranks_of_the_packer():
    from i2vsgg_amd import video
    case = CASES["multi"]
    pk = video.pack_nms(case.prediction, case.pool)
    assert pk.vids == ["a", "empty", "b", "one"] and pk.video_off.tolist() == [0, 48, 48, 118, 119]
    assert np.diff(pk.cell_off).tolist().count(1) == 2 and len(pk.cell_off) - 1 == 5        # the triplet with one member, the video of one
    first = []
    for c in range(len(pk.cell_off) - 1):
        r0, r1 = int(pk.cell_off[c]), int(pk.cell_off[c + 1])
        assert len(set(map(tuple, pk.rel[r0:r1, :4].tolist()))) == 1                       # one video, one triplet
        assert (np.diff(pk.rank[r0:r1]) > 0).all()                                         # rank order within the cell
        first.append((int(pk.rel[r0, 0]), int(pk.rank[r0])))
    assert first == sorted(first)                                                          # cells by their first member's rank
    for v in range(len(pk.vids)):
        p0, p1 = int(pk.video_off[v]), int(pk.video_off[v + 1])
        order = np.argsort(pk.rank[p0:p1])
        s, i = pk.score[p0:p1][order], pk.src[p0:p1][order]
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))).all()
    cut = video.pack_nms(CASES["pool"].prediction, 3)
    assert cut.src.tolist() == [1, 2, 3] and cut.n_input.tolist() == [6]


def test_pack_nms_refusals():
    from i2vsgg_amd import video
    good = CASES["chain"].prediction

    def broken(k, **change):
        p = copy.deepcopy(good)
        p["v"][k].update(change)
        return p
    box = good["v"][1]["sub_traj"][0]
    for change, what in ((dict(sub_traj=[box] * 2), "sub_traj holds 2 boxes"), (dict(duration=[0, 4]), "holds 3 boxes for the duration"),
                         (dict(obj_traj=[[0.0, 0.0, float("inf"), 5.0]] * 3), "not finite"), (dict(obj_traj=[[0.0, 0.0, float("nan"), 5.0]] * 3), "not finite"),
                         (dict(sub_traj=[[5.0, 0.0, 4.0, 9.0]] * 3), "x2 < x1"), (dict(sub_traj=[[0.0, 9.0, 4.0, 8.0]] * 3), "y2 < y1"),
                         (dict(score=float("nan")), "score is not finite"), (dict(sub_traj=[[0.0, 1.0, 2.0]] * 3), "not a list of boxes")):
        with pytest.raises(ValueError, match="video 'v' relation 1: .*" + what):
            video.pack_nms(broken(1, **change))
    for pool in (4097, 0, -1, 2.5, True):
        with pytest.raises(ValueError, match="pool is an int in \\[1, 4096\\]"):
            video.pack_nms(good, pool)
    assert len(video.pack_nms(good, 4096).rel) == 3
    for T in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold lies in \\[0, 1\\]"):
            video.suppress(good, T)
    with pytest.raises(Exception, match="GPU only"):
        video.suppress(good, 0.5, device="cpu")
    # a table the kernel would report raises in the host form, naming the cell
    pk = video.pack_nms(CASES["multi"].prediction)
    for name, change in (("rel", (3, 7, 5)), ("rel", (60, 8, 10 ** 6)), ("cell_off", (2, None, 10 ** 6))):
        arr = getattr(pk, name).copy()
        bad = copy.copy(pk)
        if name == "rel":
            arr[change[0], change[1]] = change[2]
        else:
            arr[change[0]] = change[2]
        setattr(bad, name, arr)
        with pytest.raises(ValueError, match="cell \\d+ is malformed"):
            video.suppress_arrays_host(bad, 0.5)


def test_extra_keys_pass_through_and_the_dicts_are_the_same_objects():
    from i2vsgg_amd import video
    case = CASES["multi"]
    pred = dict((vid, [dict(r, rel_idex=[k] * 3, sub_tid=k, note={"k": k}) for k, r in enumerate(rels)]) for vid, rels in case.prediction.items())
    before = copy.deepcopy(pred)
    out, info = video.suppress(pred, case.T)
    assert pred == before and list(out) == list(pred) and out["empty"] == []
    for vid, rels in out.items():
        ids = [id(r) for r in pred[vid]]
        assert all(id(r) in ids for r in rels)
        assert all(r["note"] == {"k": r["sub_tid"]} and pred[vid][r["sub_tid"]] is r for r in rels)
        s = [r["score"] for r in rels]
        assert s == sorted(s, reverse=True)
        assert info[vid] == {"candidates": len(pred[vid]), "suppressed": len(pred[vid]) - len(rels), "kept": len(rels)}
    assert info["empty"] == {"candidates": 0, "suppressed": 0, "kept": 0}


def _frames():
    from i2vsgg_amd import synthetic as syn
    return {"a": syn.video_frames(310, 30, integer=True, quant=64), "b": syn.video_frames(311, 24, n_objects=5)}


def test_max_per_video_defaults_to_the_output_of_before():
    from i2vsgg_amd import video
    fr = _frames()
    usual = video.associate(fr)
    assert usual == video.associate(fr, max_per_video=video.MAX_PER_VIDEO) and max(len(r) for r in usual.values()) > 7
    for cap in (0, 7, 4096):
        got = video.associate(fr, max_per_video=cap)
        assert all(got[v] == usual[v][:cap] for v in usual) or cap > video.MAX_PER_VIDEO
    wide = video.associate(fr, max_per_video=4096)
    assert all(wide[v][:video.MAX_PER_VIDEO] == usual[v] for v in usual)
    pk = video.pack_frames(fr)
    res = video.associate_arrays_host(pk)
    assert video.gather_relations(pk, *res) == usual and video.gather_relations(pk, *res, max_per_video=3) == dict((v, r[:3]) for v, r in usual.items())
    with pytest.raises(ValueError, match="max_per_video"):
        video.associate(fr, max_per_video=-1)


def test_track_mode_max_per_video_defaults_to_the_output_of_before():
    import track_association_cases as tc
    from i2vsgg_amd import video
    fr, tracks = tc.unambiguous_videos(n_videos=2)
    usual = video.associate_tracks(fr, tracks, 2)
    assert usual == video.associate_tracks(fr, tracks, 2, max_per_video=200) and sum(len(r) for r in usual.values()) > 2
    assert video.associate_tracks(fr, tracks, 2, max_per_video=2) == dict((v, r[:2]) for v, r in usual.items())


def test_duplicates_fill_the_cap_and_suppression_frees_it():
    """Six videos, four annotated relations each, every one predicted 60 times with 0-2 px of jitter: today's top 200 against
    suppression at vIoU 0.7 before the cap."""
    from i2vsgg_amd import video
    pred, gt = nc.duplicates_case()
    top = dict((vid, sorted(rels, key=lambda r: r["score"], reverse=True)[:video.MAX_PER_VIDEO]) for vid, rels in pred.items())
    ap0, rec0, _ = video.evaluate(top, gt)
    out, info = video.suppress(pred, 0.7)
    ap1, rec1, _ = video.evaluate(out, gt)
    assert ap0 < 0.5 and rec0[50] <= 0.75 and ap1 == 1.0 and rec1[50] == 1.0 and rec1[100] == 1.0
    assert ap1 > ap0 and rec1[50] > rec0[50]
    for vid in pred:
        assert len(out[vid]) == len(gt[vid]) == 4 and sorted(tuple(r["triplet"]) for r in out[vid]) == sorted(tuple(r["triplet"]) for r in gt[vid])
        assert info[vid] == {"candidates": 240, "suppressed": 236, "kept": 4}


# ---- the scripts ---------------------------------------------------------------------------------------------------------------
def test_scripts_with_cpu(tmp_path, capsys):
    """video_sgg_emb.py --relations ... --cpu: without --rel_nms the file holds the bytes of json.dump(video.associate(...)), as
    before; with it, what associate(max_per_video=pool) + suppress give.  nms_video_relations.py and eval_video_relations.py
    --rel_nms on the written files."""
    from i2vsgg_amd import synthetic as syn, video
    import eval_video_relations as ev
    import nms_video_relations as nv
    import video_sgg_emb as tv
    frames = syn.video_frames(312, 40, integer=True, quant=64)
    results = nc.frame_results(frames)
    pkl = str(tmp_path / "relations.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(results, f)
    out = str(tmp_path / "video_relations.json")
    fr = video.from_frame_results(results, dict((p, ("0", k)) for k, p in enumerate(sorted(results))))
    tv.main(["--relations", pkl, "--cpu"])
    usual = video.associate(fr)
    with open(out, "rb") as f:
        plain = f.read()
    assert plain == json.dumps(usual).encode() and len(usual["0"]) > 20
    capsys.readouterr()
    tv.main(["--relations", pkl, "--cpu", "--rel_nms", "0.7", "--rel_nms_pool", "500"])
    said = capsys.readouterr().out
    want, info = video.suppress(video.associate(fr, max_per_video=500), 0.7, pool=500)
    with open(out, "rb") as f:
        assert f.read() == json.dumps(want).encode()
    assert video.nms_totals(info) in said and 0 < len(want["0"]) < len(usual["0"])          # the twin objects' relations went
    with open(out, "wb") as f:
        f.write(plain)
    for bad in (["--rel_nms_pool", "100"], ["--rel_nms", "1.5"], ["--rel_nms", "0.5", "--rel_nms_pool", "5000"]):
        with pytest.raises(SystemExit):
            tv.main(["--relations", pkl, "--cpu"] + bad)
    # the stand-alone step on the file of the plain run
    nms = str(tmp_path / "nms.json")
    rels, info2 = nv.main(["--prediction", out, "--out", nms, "--viou", "0.7", "--cpu"])
    with open(nms) as f:
        assert json.load(f) == json.loads(json.dumps(rels)) == json.loads(json.dumps(video.suppress(json.loads(plain.decode()), 0.7)[0]))
    assert "relation NMS: 1 videos, %d candidates" % len(usual["0"]) in capsys.readouterr().out
    capped, _ = nv.main(["--prediction", out, "--out", nms, "--viou", "0.7", "--max_per_video", "3", "--pool", "50", "--cpu"])
    assert len(capped["0"]) == 3 and capped["0"] == video.suppress(json.loads(plain.decode()), 0.7, 3, 50)[0]["0"]
    with pytest.raises(SystemExit, match="pool is an int"):
        nv.main(["--prediction", out, "--out", nms, "--viou", "0.7", "--pool", "5000", "--cpu"])
    # scoring: without the flag as before, with it the suppressed prediction's score
    gt = str(tmp_path / "gt.json")
    with open(gt, "w") as f:
        json.dump({"0": syn.video_groundtruth(usual["0"], 5)}, f)
    groundtruth = json.load(open(gt))
    plain_pred = json.loads(plain.decode())
    capsys.readouterr()
    res = ev.main(["--prediction", out, "--groundtruth", gt, "--cpu"])
    assert "relation NMS" not in capsys.readouterr().out
    ref = video.evaluate(plain_pred, groundtruth)
    assert res[0] == ref[0] and res[1] == ref[1] and res[2] == ref[2]
    res = ev.main(["--prediction", out, "--groundtruth", gt, "--cpu", "--rel_nms", "0.7"])
    assert "relation NMS" in capsys.readouterr().out
    ref = video.evaluate(video.suppress(plain_pred, 0.7)[0], groundtruth)
    assert res[0] == ref[0] and res[1] == ref[1] and res[2] == ref[2]


def test_entry_point_validates_its_arguments():
    """Without a GPU only the argument checks in front of the launch run."""
    import ctypes
    from i2vsgg_amd import _lib
    L = _lib.lib
    err = lambda: L.i2v_last_error()
    assert L.i2v_version() >= 110
    need = L.i2v_video_relation_nms_workspace_bytes(10, 1000)
    assert need >= 4
    p = ctypes.c_void_p(16)

    def args(cell_off=p, rel=p, boxes=p, nc_=2, nr=5, nb=40, T=0.5, keep=p, by=p, by_ov=p, vol=p, ws=p, wsb=need):
        return (cell_off, rel, boxes, nc_, nr, nb, T, keep, by, by_ov, vol, ws, wsb, None)
    for name in ("cell_off", "rel", "boxes", "keep", "by", "by_ov", "vol"):
        assert L.i2v_video_relation_nms(*args(**{name: None})) == -1 and b"null" in err(), name
    assert L.i2v_video_relation_nms(*args(ws=None)) == -1 and b"workspace" in err()
    assert L.i2v_video_relation_nms(*args(wsb=need - 1)) == -1 and b"workspace too small" in err()
    for name in ("nc_", "nr", "nb"):
        assert L.i2v_video_relation_nms(*args(**{name: -1})) == -1 and b"negative" in err(), name
    for T in (-0.25, 1.25, float("nan")):
        assert L.i2v_video_relation_nms(*args(T=T)) == -1 and b"threshold lies in [0, 1]" in err(), T
    assert L.i2v_video_relation_nms(*args(nc_=0, nr=0, nb=0)) == 0                       # empty input: nothing is launched
    assert L.i2v_video_relation_nms(*args(nc_=3, nr=0, nb=0, rel=None, keep=None, by=None, by_ov=None, vol=None, boxes=None)) == 0
