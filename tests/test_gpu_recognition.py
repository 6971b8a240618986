"""Predicate recognition on the MI355X: csrc/recognition.hip (ops.recognition_rows, ops.recognition_align) against the numpy
forms of i2vsgg_amd.eval / i2vsgg_amd.recognition, bit for bit -- both sides evaluate the same expressions in the same order,
so no margin is needed and the recorded figure is the number of differing elements, bound 0 --, the reference's metrics
(tests/golden/recognition.npz), the per-frame branch ``forward_predicate_eval`` / ``recognition_frame`` and the script."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden, record_margin

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recognition_cases as cases  # noqa: E402

DEV = "cuda:0"
NAMES = ("mean", "count", "top", "hit", "totals", "per_class")
_SETS = {}


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _differing(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((_raw(got) != _raw(want)).sum())


def _set(C, R):
    """A device case set, packed once, with the host form's answer; nobody writes to either."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    if (C, R) not in _SETS:
        from i2vsgg_amd import recognition
        ds = cases.device_set(C, R)
        pk = recognition.pack(ds["frame_recognitions"], ds["groundtruth"], ds["classes"], ds["predicates"])
        _SETS[(C, R)] = (pk, recognition.align_arrays_host(pk))
    return _SETS[(C, R)]


# ---------------------------------------------------------------------------------------------------------------------
# the per-frame tail
# ---------------------------------------------------------------------------------------------------------------------
def _tail_inputs(R, seed=3):
    rng = np.random.default_rng(seed + R)
    B, P, C = 5, 7, 16
    prob = rng.dirichlet(np.ones(C), B).astype(np.float32)
    prob[3, [4, 9]] = prob[3].max() + np.float32(0.125)          # two equal largest probabilities: class 4 must win
    prob[1, 0] = 0.9375                                          # the background column is read as zero
    rel = rng.dirichlet(np.ones(R), P).astype(np.float32)
    ixs, ixo = rng.integers(0, B, P), rng.integers(0, B, P)
    ixs[0], ixo[0], ixs[1], ixo[2] = 3, 1, 1, 3
    return prob, rel, ixs, ixo, rng.uniform(0, 1, (C - 1, C - 1, R)) * (rng.random((C - 1, C - 1, R)) < 0.5)


@pytest.mark.parametrize("R", [10, 62, 132])                    # one, one and three column passes of a wave
def test_rows_equal_the_numpy_tail_bit_for_bit(R):
    from i2vsgg_amd import eval as ev, ops
    prob, rel, ixs, ixo, prior = _tail_inputs(R)
    for so_prior in (prior, None):
        L = ev.prior_log_table(so_prior, 16, R)
        want = ev.recognition_rows_host(prob, rel, ixs, ixo, L)
        got = [t.cpu().numpy() for t in ops.recognition_rows(prob, rel, ixs, ixo, L, device=DEV)]
        assert want[3][3] == 4 and want[3][1] != 0 and got[3].dtype == np.int32
        bad = sum(_differing(g, w) for g, w in zip(got, want))
        record_margin("test_rows_equal_the_numpy_tail_bit_for_bit[%d]" % R,
                      "differing elements, %s prior" % ("with" if so_prior is not None else "without"), bad, 0)
        assert bad == 0
        # ... and the tail as the reference states it: the log of the gathered prior rows, added in place
        rec = {"boxes": [[0, 0, 1, 1]] * 5, "sub_scores": prob[ixs], "obj_scores": prob[ixo], "rel_scores": rel, "tids": [[0, 1]] * 7,
               "rel_so_prior": (prior if so_prior is not None else np.zeros_like(prior))[want[3][ixs] - 1, want[3][ixo] - 1]}
        for g, w in zip(got[:3], ev.recognition_output(rec)[:3]):
            assert _differing(g, w) == 0
    assert not np.array_equal(got[2], rel)


def test_rows_index_out_of_range_raises_and_writes_nothing():
    from i2vsgg_amd import eval as ev, ops
    from i2vsgg_amd._lib import I2VError, lib, ptr
    prob, rel, ixs, ixo, prior = _tail_inputs(62)
    L = ev.prior_log_table(prior, 16, 62)
    for bad_value in (5, -1):
        bad = ixs.copy()
        bad[4] = bad_value
        with pytest.raises(I2VError, match="pair 4"):
            ops.recognition_rows(prob, rel, bad, ixo, L, device=DEV)
        t = [torch.as_tensor(x).to(DEV).contiguous() for x in (prob, rel, bad.astype(np.int64), ixo.astype(np.int64), L)]
        outs = [torch.full(s, -7.0, device=DEV) for s in ((7, 16), (7, 16), (7, 62))] + [torch.full((5,), -7, device=DEV, dtype=torch.int32)]
        ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
        rc = lib.i2v_recognition_rows(*[ptr(x) for x in t], 5, 7, 16, 62, *[ptr(x) for x in outs], ptr(ws), 256,
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        sub, obj, pre, cls = [x.cpu().numpy() for x in outs]
        assert int(ws[:4].view(torch.int32).item()) == 5                             # 1 + the pair's index
        assert (sub[4] == -7).all() and (obj[4] == -7).all() and (pre[4] == -7).all()
        keep = np.arange(7) != 4
        want = ev.recognition_rows_host(prob, rel, np.where(keep, bad, 0), ixo, L)
        assert np.array_equal(sub[keep], want[0][keep]) and np.array_equal(pre[keep], want[2][keep]) and np.array_equal(cls, want[3])
    with pytest.raises(I2VError):
        ops.recognition_rows(prob, rel, ixs, ixo, L, device="cpu")
    with pytest.raises(ValueError):
        ops.recognition_rows(prob, rel, ixs[:-1], ixo, L, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# the video level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,R", [(16, 62), (35, 132), (2, 1), (81, 512)])
def test_align_equals_the_host_form_bit_for_bit(C, R):
    """Segments of 0, 1, 2, 63, 64, 65 and 300 rows, skipped / empty / missing frames, doubled pairs, planted equal means (two
    equal maxima; ties inside the top 10), more than 256 segments; a group narrower than 10 at (2, 1), eleven columns per lane at
    (81, 512)."""
    from i2vsgg_amd import recognition
    pk, want = _set(C, R)
    counts = np.diff(pk.seg_off)
    assert len(counts) > 256 and {0, 1, 2, 63, 64, 65, 300} <= set(counts.tolist())
    assert len(pk.inst) > len(counts) or R == 1                  # second predicates on a pair, where there are two
    got = recognition.align_arrays(pk, DEV)
    for name, g, w in zip(NAMES, got, want):
        bad = _differing(g, w)
        record_margin("test_align_equals_the_host_form_bit_for_bit[%d-%d]" % (C, R), "differing elements of " + name, bad, 0)
        assert bad == 0, name
    s0 = pk.segments.index(("edges", 0, 1, 0, 1))
    assert got[0][s0, 1] == got[0][s0, C - 1] and got[2][s0, 0, 0] == 1                 # two equal maxima: the lower index first
    assert (got[2][counts == 0] == -1).all() and not got[0][counts == 0].any()
    if C == 2:
        assert (got[2][counts > 0][:, :2, :2] == [1, 0]).all() and (got[2][counts > 0][:, :2, 2:] == -1).all()
        assert (got[2][counts > 0][:, 2, 0] == 0).all() and (got[2][:, 2, 1:] == -1).all()
    assert 0 < got[4][7] < len(pk.inst)


def test_align_two_runs_give_the_same_bits():
    from i2vsgg_amd import recognition
    pk, want = _set(16, 62)
    a, b = recognition.align_arrays(pk, DEV), recognition.align_arrays(pk, DEV)
    for x, y in zip(a, b):
        assert _differing(x, y) == 0


def test_align_malformed_tables_raise():
    from i2vsgg_amd import ops
    from i2vsgg_amd._lib import I2VError
    pk, want = _set(16, 62)
    call = lambda **kw: ops.recognition_align(kw.get("rows", pk.rows), kw.get("seg_off", pk.seg_off), kw.get("seg_row", pk.seg_row),
                                              kw.get("inst", pk.inst), 16, 62, device=DEV)
    s = int(np.nonzero(np.diff(pk.seg_off) > 2)[0][0])
    for value in (len(pk.rows), -1):
        seg_row = pk.seg_row.copy()
        seg_row[pk.seg_off[s] + 1] = value
        with pytest.raises(I2VError, match="segment %d" % s):
            call(seg_row=seg_row)
    seg_off = pk.seg_off.copy()
    seg_off[-1] = len(pk.seg_row) + 1
    with pytest.raises(I2VError, match="segment %d" % (len(seg_off) - 2)):
        call(seg_off=seg_off)
    for col, value in ((1, 16), (2, 62), (3, -1), (0, len(pk.seg_off) - 1), (2, 100000)):
        inst = pk.inst.copy()
        inst[9, col] = value
        with pytest.raises(I2VError, match="instance 9"):
            call(inst=inst)
    with pytest.raises(I2VError):
        ops.recognition_align(pk.rows, pk.seg_off, pk.seg_row, pk.inst, 16, 62, device="cpu")
    with pytest.raises(I2VError, match="over the limit"):
        ops.recognition_align(np.zeros((1, 2 * 16 + 2100)), [0, 1], [0], [[0, 1, 0, 1]], 16, 2100, device=DEV)
    out = ops.recognition_align(np.zeros((0, 94)), [0], [], np.zeros((0, 4)), 16, 62, device=DEV)    # nothing to do
    assert out[0].shape == (0, 94) and out[4].tolist() == [0] * 8
    for got, w in zip(call(), want):                                                 # the launch after the refused ones is clean
        assert _differing(got.cpu().numpy(), w) == 0


def test_device_form_reproduces_the_reference_metrics():
    from i2vsgg_amd import recognition
    g = golden("recognition")
    cs = cases.golden_set()
    res = recognition.evaluate(cs["frame_recognitions"], cs["groundtruth"], cs["classes"], cs["predicates"], device=DEV)
    seven = [res["sub"][1], res["sub"][5], res["obj"][1], res["obj"][5], res["pre"][1], res["pre"][5], res["rel"][1]]
    assert np.array_equal(_raw(np.asarray(seven, np.float64)), _raw(g["metrics"]))
    for k, nre in enumerate((1, 5)):
        got = np.asarray([res["objects"][nre][c] for c in range(1, 16)], np.float64)
        assert np.array_equal(_raw(got), _raw(g["per_class"][k, 1:]))
    host = recognition.evaluate(cs["frame_recognitions"], cs["groundtruth"], cs["classes"], cs["predicates"])
    assert json.dumps(recognition.to_json(host), sort_keys=True) == json.dumps(recognition.to_json(res), sort_keys=True)


# ---------------------------------------------------------------------------------------------------------------------
# the per-frame branch
# ---------------------------------------------------------------------------------------------------------------------
H, W = 320, 480


@pytest.fixture(scope="module")
def frame_net():
    """res50, random-init vrd from syn.vrd_params; a 320 x 480 frame with 6 boxes and 5 relations of which two share a pair;
    split-K atomics off, so that two forwards of the frame are bit-equal."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from i2vsgg_amd import synthetic as syn
    from i2vsgg_amd._lib import TUNE, lib
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.faster_rcnn.resnet_SGG_emb import resnet
    from i2vsgg_amd.model.utils import config as c
    c.cfg_from_file(c.default_cfg_file("res101"))
    n_rel, n_cls = 62, 16
    torch.manual_seed(0)
    args = argparse.Namespace(num_relations=n_rel, num_classes=n_cls, emb_dim=300, use_obj_visual=True, spatial_type=2, vrd_task="pre_det")
    net = resnet(tuple(range(n_cls)), args, 50, obj_vecs=syn.word_vectors(22, n_cls), prd_vecs=syn.word_vectors(21, n_rel))
    net.create_architecture()
    sd = {k[len("vrd."):]: v for k, v in syn.vrd_params(13).items() if k.startswith("vrd.")}
    assert not load_reference_state(net.vrd, sd, strict=False).unexpected_keys
    net.to(DEV).eval()
    net.vrd._so_prior = np.random.default_rng(5).uniform(0, 1, (n_cls - 1, n_cls - 1, n_rel))
    boxes = np.floor(syn.boxes(61, 6, H, W, 48, 200)).astype(np.float64).tolist()
    rels = [[0, 1, 3], [2, 4, 10], [0, 1, 7], [5, 3, 1], [3, 0, 20]]
    per_rel = [[10, 11], [12, 14], [10, 11], [15, 13], [13, 10]]
    net.vrd.target_gt_rels = {
        "full": {"boxes": boxes, "rels": rels, "tids": per_rel},
        "per_box": {"boxes": boxes, "rels": rels, "tids": [10, 11, 12, 13, 14, 15]},
        "none": {"boxes": [], "rels": [], "tids": []},
        "one": {"boxes": boxes[:1], "rels": [], "tids": []},
        "no_rels": {"boxes": boxes, "rels": [], "tids": []},
        "bad": {"boxes": boxes, "rels": rels, "tids": per_rel[:3]}}
    im = torch.from_numpy(syn.frames(50, 1, H, W)[0]).to(DEV)
    info = torch.from_numpy(np.array([[H, W, 1.0]], np.float32)).to(DEV)
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)
    try:
        yield net, im, info
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)


def test_recognition_frame_equals_the_host_tail_of_its_record(frame_net):
    from i2vsgg_amd import eval as ev
    from i2vsgg_amd.model.faster_rcnn.faster_rcnn_SGG_emb import build_pair_tables, rasterize_masks
    net, im, info = frame_net
    with torch.no_grad():
        fmap = net.RCNN_base(im)
        rec = net.forward_predicate_eval(fmap, info, "full")
    assert sorted(rec) == sorted(["ixs", "ixo", "boxes", "classes", "confs", "rel_so_prior", "rel_scores", "sub_scores", "obj_scores",
                                  "pre_feat", "tids"])
    assert rec["ixs"].tolist() == [0, 2, 5, 3] and rec["ixo"].tolist() == [1, 4, 3, 0]          # unique pairs, first-seen order
    assert rec["tids"] == [[10, 11], [12, 14], [15, 13], [13, 10]]
    assert all(rec[k].is_cuda for k in ("rel_scores", "sub_scores", "obj_scores", "pre_feat")) and rec["rel_scores"].shape == (4, 62)
    got = ev.recognition_frame(net, im, info, "full")
    want = ev.recognition_output(rec)                                                # downloads the record's tensors
    for name, g, w in zip(("sub", "obj", "pre"), got, want):
        bad = _differing(g, w)
        record_margin("test_recognition_frame_equals_the_host_tail_of_its_record", "differing elements of " + name, bad, 0)
        assert bad == 0, name
    assert got[3] == want[3] == rec["tids"]
    assert not got[0][:, 0].any() and not got[1][:, 0].any()
    # classes / confs are classify_boxes's
    anno = net.vrd.target_gt_rels["full"]
    cls, conf = net.classify_boxes(fmap, np.array(anno["boxes"]) * 1.0)
    assert np.array_equal(rec["classes"], cls) and np.array_equal(np.asarray(rec["confs"]).view(np.uint32), conf.view(np.uint32))
    assert (rec["classes"] >= 1).all() and rec["rel_so_prior"].shape == (4, 62)
    assert np.array_equal(rec["rel_so_prior"], net.vrd._so_prior[cls[rec["ixs"]] - 1, cls[rec["ixo"]] - 1])
    # rel_scores are the relation head's in eval mode on the same tables
    gt, union, bnd, _, ixs, ixo = build_pair_tables(anno, 1.0, float(H), float(W), 62)
    b5 = np.zeros((6, 5), np.float32)
    b5[:, 1:] = gt
    r5 = np.zeros((4, 5), np.float32)
    r5[:, 1:] = union
    assert not net.vrd.training
    with torch.no_grad():
        score, feat = net.vrd.forward_device(fmap[:1], torch.from_numpy(b5).to(DEV), torch.from_numpy(r5).to(DEV), rasterize_masks(bnd, DEV),
                                             torch.from_numpy(ixs).to(DEV), torch.from_numpy(ixo).to(DEV))
    assert torch.equal(score, rec["rel_scores"]) and torch.equal(feat, rec["pre_feat"])
    assert np.allclose(score.sum(1).cpu().numpy(), 1.0, atol=1e-4)                   # softmax over predicates
    # without a prior: log(1/30) everywhere
    prior = net.vrd._so_prior
    try:
        net.vrd._so_prior = None
        plain = ev.recognition_frame(net, im, info, "full")
    finally:
        net.vrd._so_prior = prior
    assert np.array_equal(plain[2], (score.cpu().numpy().astype(np.float64) + np.log(1.0 / 30)).astype(np.float32))
    assert _differing(plain[0], got[0]) == 0 and not np.array_equal(plain[2], got[2])


def test_degenerate_frames_and_tids_layouts(frame_net):
    from i2vsgg_amd import eval as ev
    net, im, info = frame_net
    with torch.no_grad():
        fmap = net.RCNN_base(im)
        assert net.forward_predicate_eval(fmap, info, "none") == {"boxes": [], "classes": [], "confs": []}
        for key, n in (("one", 1), ("no_rels", 6)):
            rec = net.forward_predicate_eval(fmap, info, key)
            assert sorted(rec) == ["boxes", "classes", "confs"] and len(rec["classes"]) == len(rec["confs"]) == n
        with pytest.raises(ValueError, match="bad"):
            net.forward_predicate_eval(fmap, info, "bad")
    for key in ("none", "one", "no_rels"):
        assert ev.recognition_frame(net, im, info, key) == (None,) * 4
    a, b = ev.recognition_frame(net, im, info, "full"), ev.recognition_frame(net, im, info, "per_box")
    for x, y in zip(a[:3], b[:3]):
        assert _differing(x, y) == 0
    assert a[3] == b[3] == [[10, 11], [12, 14], [15, 13], [13, 10]]


def test_script_writes_recognitions_and_metrics(tmp_path):
    """recognize_sgg_emb.py on the synthetic recognition set (2 videos x 12 frames, res50, small frames) writes
    frame_recognitions.pkl and recognition.json; eval_recognition.py --cpu on the written files gives the same metrics."""
    import pickle
    import eval_recognition
    import recognize_sgg_emb
    from i2vsgg_amd.model.utils import config as c
    out = str(tmp_path / "out")
    saved = copy.deepcopy(dict(c.cfg))                   # the script loads res50.yml into the global cfg: put it back afterwards
    try:
        fr, res = recognize_sgg_emb.main(["--imdbval_name", "synthetic_24_v", "--net", "res50", "--scale", "192", "--frames_per_video", "12",
                                          "--output_dir", out])
    finally:
        c._merge_a_into_b(c.AttrDict(saved), c.cfg)
    d = os.path.join(out, "res50", "synthetic")
    with open(os.path.join(d, "frame_recognitions.pkl"), "rb") as f:
        written = pickle.load(f)
    with open(os.path.join(d, "recognition.json")) as f:
        metrics = json.load(f)
    assert sorted(written) == ["0", "1"] and all(sorted(v) == list(range(12)) for v in written.values())
    assert sum(1 for v in written.values() for r in v.values() if not r) >= 2        # the single-box frames
    assert sum(1 for v in written.values() for r in v.values() if r) >= 12
    for r in (r for v in written.values() for r in v.values() if r):
        assert r["sub_scores"].shape == (len(r["tids"]), 16) and r["pre_scores"].shape == (len(r["tids"]), 62)
        assert r["pre_scores"].dtype == np.float32 and not r["sub_scores"][:, 0].any()
    assert res["n_aligned"] == sum(len(v) for v in metrics["groundtruth"].values()) >= 8 and res["n_videos_missing"] == 0
    again = eval_recognition.main(["--prediction", os.path.join(d, "frame_recognitions.pkl"), "--groundtruth",
                                   os.path.join(d, "recognition.json"), "--cpu"])
    from i2vsgg_amd import recognition
    assert json.dumps(recognition.to_json(again), sort_keys=True) == json.dumps(metrics["metrics"], sort_keys=True)
    assert json.dumps(recognition.to_json(res), sort_keys=True) == json.dumps(metrics["metrics"], sort_keys=True)
