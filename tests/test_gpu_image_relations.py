"""Image relation recall@K on the MI355X: csrc/image_relations.hip (ops.image_relation_match, ops.image_relation_count) against
the numpy host form of i2vsgg_amd.image_relations, bit for bit -- both sides evaluate the same expressions in the same order, so
no margin is needed and the bound on differing elements is 0.  The host form itself is held to the scalar restatement of the rules
in tests/test_image_relations_host.py; nothing here compares the code under test with itself."""
import argparse
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_relation_cases as cases  # noqa: E402

DEV = "cuda:0"
NAMES = ("hit", "hit_ov", "gt_rank", "totals", "zs_totals", "per_predicate")
NRETURNS = (50, 100)
N_REL = 12
_BATCH = {}


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _differing(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((_raw(got) != _raw(want)).sum())


def _batch():
    """The device batch, packed once, with the host form's answer; nobody writes to either."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    if not _BATCH:
        from i2vsgg_amd import image_relations as ir
        relations, annotations = cases.device_set()
        seen = ir.seen_triplets_of(dict((k, annotations[k]) for k in sorted(annotations)[:10]))
        pk = ir.pack(relations, annotations, N_REL, NRETURNS, None, seen)
        _BATCH.update(pk=pk, want=ir.evaluate_packed(pk, NRETURNS, 0.5))
    return _BATCH["pk"], _BATCH["want"]


def test_device_equals_the_host_form_bit_for_bit():
    """40 images in one launch of each kernel: 1, 63, 64, 65 and 130 ground truths (one pass of the wave, the pass boundary, three
    passes), 0, 1, 99 and 100 predictions, images without a record and with a record of Nones, a zero-shot split."""
    from i2vsgg_amd import image_relations as ir
    pk, want = _batch()
    n_gt, n_pred = np.diff(pk.gt_off), np.diff(pk.pred_off)
    assert len(pk.keys) == 40 and pk.n_ignored == 1
    assert {1, 63, 64, 65, 130} <= set(n_gt.tolist()) and {0, 1, 99, 100} <= set(n_pred.tolist())
    assert 0 < (pk.gt_zs != 0).sum() < len(pk.gt_zs)
    for m in range(2):                                           # the host answer is not trivial: hits, misses, K matters
        assert 0 < want[3][m, 0, 0] < want[3][m, 1, 0] < want[3][m, 1, 1]
        assert 0 < want[4][m, 1, 0] < want[4][m, 1, 1]
    assert not np.array_equal(want[0][0], want[0][1])
    got = ir.evaluate_packed(pk, NRETURNS, 0.5, device=DEV)
    for name, g, w in zip(NAMES, got, want):
        assert _differing(g, w) == 0, name


def test_two_runs_give_the_same_bits():
    from i2vsgg_amd import image_relations as ir
    pk, _ = _batch()
    a, b = ir.evaluate_packed(pk, NRETURNS, 0.5, device=DEV), ir.evaluate_packed(pk, NRETURNS, 0.5, device=DEV)
    for x, y in zip(a, b):
        assert _differing(x, y) == 0


@pytest.mark.parametrize("thr", [0.3, 0.7])
def test_other_thresholds_equal_the_host_form(thr):
    from i2vsgg_amd import image_relations as ir
    pk, at_half = _batch()
    want = ir.evaluate_packed(pk, (1, 10, 100), thr)
    assert not np.array_equal(want[0], at_half[0])               # the threshold decides something
    got = ir.evaluate_packed(pk, (1, 10, 100), thr, device=DEV)
    for name, g, w in zip(NAMES, got, want):
        assert _differing(g, w) == 0, name


def test_hand_worked_cases_on_the_device():
    from i2vsgg_amd import image_relations as ir
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    for name, c in sorted(cases.hand_cases().items()):
        kw = dict(c["kwargs"])
        nreturns = c.get("nreturns", (50,))
        thr = kw.pop("iou_threshold", 0.5)
        pk = ir.pack(c["relations"], c["annotations"], c["n_rel"], nreturns, kw.get("k_per_pair"), kw.get("seen_triplets"))
        hit, hit_ov, gt_rank, totals, zs_totals, _ = ir.evaluate_packed(pk, nreturns, thr, device=DEV)
        assert hit.tolist() == c["hit"] and gt_rank.tolist() == c["gt_rank"], name
        assert _differing(hit_ov, np.asarray(c["hit_ov"], np.float64)) == 0, name
        for j, k in enumerate(nreturns):
            if k in c["totals"]:
                assert [tuple(t) for t in totals[:, j].tolist()] == c["totals"][k], name
            if k in c.get("zs_totals", {}):
                assert [tuple(t) for t in zs_totals[:, j].tolist()] == c["zs_totals"][k], name
        res = ir.evaluate(c["relations"], c["annotations"], c["n_rel"], nreturns, thr, device=DEV, **kw)
        for key, value in c.get("counts", {}).items():
            assert res[key] == value, (name, key)


def _direct(pk, pred_off, gt_off, max_gt):
    """i2v_image_relation_match on the batch with the given tables, outputs pre-filled with -7: (status, hit, hit_ov, gt_rank)."""
    from i2vsgg_amd._lib import lib, ptr
    t = [torch.as_tensor(np.ascontiguousarray(x)).to(DEV) for x in (pred_off, gt_off, pk.pred_trip, pk.pred_box, pk.gt_trip, pk.gt_box)]
    n_pred, n_gt = len(pk.pred_trip), len(pk.gt_trip)
    hit = torch.full((2, n_pred), -7, device=DEV, dtype=torch.int32)
    hit_ov = torch.full((2, n_pred), -7.0, device=DEV, dtype=torch.float64)
    gt_rank = torch.full((2, n_gt), -7, device=DEV, dtype=torch.int32)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    rc = lib.i2v_image_relation_match(*[ptr(x) for x in t], len(pred_off) - 1, n_pred, n_gt, max_gt, 0.5, ptr(hit), ptr(hit_ov), ptr(gt_rank),
                                      ptr(ws), 256, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return int(ws[:4].view(torch.int32).item()), hit.cpu().numpy(), hit_ov.cpu().numpy(), gt_rank.cpu().numpy()


def test_malformed_images_raise_the_status_word_and_leave_the_others_intact():
    """The tables are checked before anything is read through them.  An offset is shared by two images, so the single-image cases
    sit at the end of the table: a prediction offset that steps back, a ground-truth offset past the array.  Four images in the
    middle of the batch are refused by a ``max_gt`` below their 130 ground truths."""
    from i2vsgg_amd import ops
    from i2vsgg_amd._lib import I2VError
    pk, want = _batch()
    I = len(pk.keys)
    last_p, last_g = slice(int(pk.pred_off[I - 1]), int(pk.pred_off[I])), slice(int(pk.gt_off[I - 1]), int(pk.gt_off[I]))
    assert last_p.stop - last_p.start > 1 and last_g.stop - last_g.start > 1
    keep_p, keep_g = np.arange(len(pk.pred_trip)) < last_p.start, np.arange(len(pk.gt_trip)) < last_g.start

    def others_intact(hit, hit_ov, gt_rank, keep_p, keep_g):
        assert np.array_equal(hit[:, keep_p], want[0][:, keep_p]) and np.array_equal(gt_rank[:, keep_g], want[2][:, keep_g])
        assert _differing(hit_ov[:, keep_p], want[1][:, keep_p]) == 0

    # 1. non-monotone: the last image's predictions end before they begin -- its ground truths come out as -1, no prediction of
    #    its own range exists to be written
    pred_off = pk.pred_off.copy()
    pred_off[I] = pred_off[I - 1] - 1
    status, hit, hit_ov, gt_rank = _direct(pk, pred_off, pk.gt_off, 4096)
    assert status == I
    others_intact(hit, hit_ov, gt_rank, keep_p, keep_g)
    assert (gt_rank[:, last_g] == -1).all() and (hit[:, last_p] == -7).all() and (hit_ov[:, last_p] == -7).all()
    with pytest.raises(I2VError, match="image %d" % (I - 1)):
        ops.image_relation_match(pred_off, pk.gt_off, pk.pred_trip, pk.pred_box, pk.gt_trip, pk.gt_box, device=DEV)
    # 2. the last image's ground truths end past the array -- its predictions come out as -1, nothing is read or written there
    gt_off = pk.gt_off.copy()
    gt_off[I] = len(pk.gt_trip) + 5
    status, hit, hit_ov, gt_rank = _direct(pk, pk.pred_off, gt_off, 4096)
    assert status == I
    others_intact(hit, hit_ov, gt_rank, keep_p, keep_g)
    assert (hit[:, last_p] == -1).all() and (hit_ov[:, last_p] == -1.0).all() and (gt_rank[:, last_g] == -7).all()
    # 3. more ground truths than the caller's max_gt: images 4, 14, 24, 34 (130 each) are refused, their neighbours are not
    big = np.nonzero(np.diff(pk.gt_off) > 129)[0]
    assert big.tolist() == [4, 14, 24, 34]
    status, hit, hit_ov, gt_rank = _direct(pk, pk.pred_off, pk.gt_off, 129)
    assert status == 35
    img_p, img_g = np.repeat(np.arange(I), np.diff(pk.pred_off)), np.repeat(np.arange(I), np.diff(pk.gt_off))
    bad_p, bad_g = np.isin(img_p, big), np.isin(img_g, big)
    others_intact(hit, hit_ov, gt_rank, ~bad_p, ~bad_g)
    assert bad_p.any() and (hit[:, bad_p] == -1).all() and (hit_ov[:, bad_p] == -1.0).all() and (gt_rank[:, bad_g] == -1).all()
    # a predicate outside the table is refused by the count, a device that is no GPU by both
    trip = pk.gt_trip.copy()
    trip[9, 1] = N_REL
    with pytest.raises(I2VError, match="ground truth 9"):
        ops.image_relation_count(want[2], trip, pk.gt_zs, NRETURNS, N_REL, device=DEV)
    with pytest.raises(I2VError):
        ops.image_relation_match(pk.pred_off, pk.gt_off, pk.pred_trip, pk.pred_box, pk.gt_trip, pk.gt_box, device="cpu")
    with pytest.raises(ValueError):
        ops.image_relation_count(want[2], pk.gt_trip, pk.gt_zs, (), N_REL, device=DEV)
    # the launch after the refused ones is clean
    status, hit, hit_ov, gt_rank = _direct(pk, pk.pred_off, pk.gt_off, 4096)
    assert status == 0
    others_intact(hit, hit_ov, gt_rank, np.ones(len(pk.pred_trip), bool), np.ones(len(pk.gt_trip), bool))


def test_relation_loop_scores_its_triplets_with_the_flag(tmp_path, capsys):
    """image_sgg_emb.py (test_sgg_emb.py's loop, then the evaluation) on the synthetic imdb (10 frames, small): after relations.pkl
    it prints the recalls and writes image_relations.json, which the host form reproduces from the returned results."""
    import json
    import pickle
    import eval_image_relations
    import image_sgg_emb as tr
    from i2vsgg_amd import image_relations as ir
    from i2vsgg_amd.model.utils import config as c
    from i2vsgg_amd.roi_data_layer.roidb import combined_roidb
    saved = copy.deepcopy(dict(c.cfg))                   # the script sets the scales in the global cfg: put it back afterwards
    try:
        c.cfg_from_file(c.default_cfg_file("res101"))
        gt = combined_roidb("synthetic_10_v", False)[0].gt_rels(62)
        path = str(tmp_path / "annotations.pkl")
        with open(path, "wb") as f:
            pickle.dump(gt, f)
        out = str(tmp_path / "out")
        results, metrics = tr.main(["--imdbval_name", "synthetic_10_v", "--scale", "192", "--frames", "3", "--output_dir", out,
                                    "--image_groundtruth", path, "--train_annotations", path])
    finally:
        c._merge_a_into_b(c.AttrDict(saved), c.cfg)
    with open(os.path.join(out, "res101", "synthetic", "image_relations.json")) as f:
        written = json.load(f)
    want = ir.evaluate(eval_image_relations.by_annotation_key(results, gt), gt, 62, seen_triplets=ir.seen_triplets_of(gt))
    assert written == json.loads(json.dumps(ir.to_json(want))) == json.loads(json.dumps(ir.to_json(metrics)))
    with open(os.path.join(out, "res101", "synthetic", "relations.pkl"), "rb") as f:
        assert sorted(pickle.load(f)) == sorted(results)         # the loop's own file, as test_sgg_emb.py alone writes it
    assert written["n_images"] == 10 and written["n_ignored"] == 0 and written["n_gt_zero_shot"] == 0
    assert written["n_gt"] == sum(len(a["rels"]) for a in gt.values()) == written["relation"]["totals"]["100"][1]
    # the loop ran on the annotated boxes: a written row of an annotated pair under its annotated predicate overlaps it fully, so
    # that relation is recalled (by that row, or by a better-ranked one that took it first)
    assert written["relation"]["totals"]["100"][0] >= sum(
        1 for k, r in eval_image_relations.by_annotation_key(results, gt).items() if r[1] is not None
        for s, o, p in set(map(tuple, gt[k]["rels"]))
        if any((r[2][i] == gt[k]["boxes"][s]).all() and (r[3][i] == gt[k]["boxes"][o]).all() and r[0][i][1] == p for i in range(len(r[1]))))
    assert "relation detection R@100: %.4f" % want["relation"]["recall"][100] in capsys.readouterr().out


def test_every_cell_of_a_frame_recalls_every_annotated_relation():
    """End to end on one frame (res50, 320 x 480, 6 pairwise-distinct annotated boxes, 5 relations of which two share a pair):
    ``relation_frame`` with k = pairs x predicates returns every cell, so each annotated cell is present with overlap 1 and both
    recalls at K = k are exactly 1; at K = 1 they are the host form's on the same record."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from i2vsgg_amd import eval as ev, image_relations as ir, synthetic as syn
    from i2vsgg_amd._lib import TUNE, lib
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.faster_rcnn.resnet_SGG_emb import resnet
    from i2vsgg_amd.model.utils import config as c
    H, W = 320, 480
    c.cfg_from_file(c.default_cfg_file("res101"))
    n_rel, n_cls = 62, 16
    torch.manual_seed(0)
    args = argparse.Namespace(num_relations=n_rel, num_classes=n_cls, emb_dim=300, use_obj_visual=True, spatial_type=2, vrd_task="pre_det")
    net = resnet(tuple(range(n_cls)), args, 50, obj_vecs=syn.word_vectors(22, n_cls), prd_vecs=syn.word_vectors(21, n_rel))
    net.create_architecture()
    sd = {k[len("vrd."):]: v for k, v in syn.vrd_params(13).items() if k.startswith("vrd.")}
    assert not load_reference_state(net.vrd, sd, strict=False).unexpected_keys
    net.to(DEV).eval()
    boxes = np.floor(syn.boxes(61, 6, H, W, 48, 200)).astype(np.float64).tolist()
    assert len(set(tuple(b) for b in boxes)) == 6
    anno = {"boxes": boxes, "box_classes": [3, 7, 3, 1, 12, 7], "rels": [[0, 1, 3], [2, 4, 10], [0, 1, 7], [5, 3, 1], [3, 0, 20]]}
    net.vrd.target_gt_rels = {"full": anno}
    im = torch.from_numpy(syn.frames(50, 1, H, W)[0]).to(DEV)
    info = torch.from_numpy(np.array([[H, W, 1.0]], np.float32)).to(DEV)
    k = 6 * 5 * n_rel
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)
    try:
        rec = ev.relation_frame(net, im, info, "full", k=k)[1]
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
    assert len(rec[1]) == k and rec[0].shape == (k, 3)
    got = ir.evaluate({"full": rec}, {"full": anno}, n_rel, nreturns=(1, k), device=DEV)
    host = ir.evaluate({"full": rec}, {"full": anno}, n_rel, nreturns=(1, k))
    for mode in ir.MODES:
        assert got[mode]["totals"][k] == (5, 5) and got[mode]["recall"][k] == 1.0
        assert got[mode]["totals"][1] == host[mode]["totals"][1] and got[mode]["totals"][1][0] in (0, 1)
        assert _differing(np.float64(got[mode]["recall"][1]).reshape(1), np.float64(host[mode]["recall"][1]).reshape(1)) == 0
        assert got[mode]["mean_recall"][k] == 1.0 and np.array_equal(got[mode]["per_predicate"][k], host[mode]["per_predicate"][k])
