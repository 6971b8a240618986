"""Seq-NMS on the MI355X: csrc/seqnms.hip (ops.seq_nms) against the host form of i2vsgg_amd.seqnms, bit for bit -- both
evaluate the same float64 expressions in the same order on exactly widened float32 inputs, so no draw is rejected and no
margin is needed -- and the tracked boxes' scores in the relation loop."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqnms_cases as cases  # noqa: E402

DEV = "cuda:0"


def _device(pk, **kw):
    from i2vsgg_amd import ops
    return [t.cpu().numpy() for t in ops.seq_nms(pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score, device=DEV, **kw)]


def _same(got, want):
    assert np.array_equal(got[0], want[0])                                          # tid
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))          # the bits of new_score
    assert np.array_equal(got[2], want[2])                                          # n_tracks


@pytest.fixture(scope="module")
def batch():
    """The launch of about 24 groups, packed once, with the host form's answer; nobody writes to either."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from i2vsgg_amd import seqnms
    all_boxes, frame_index = cases.device_batch()
    pk = seqnms.pack(all_boxes, frame_index)
    return all_boxes, frame_index, pk, seqnms.seq_nms_arrays_host(pk)


def test_device_equals_host_form_bit_for_bit(batch):
    all_boxes, frame_index, pk, want = batch
    counts = np.diff(pk.box_off)
    lengths = sorted(set(np.diff(pk.group_off).tolist()))
    assert lengths == [1, 2, 3, 37, 64, 65, 130] and len(pk.group_off) - 1 == 35     # 7 videos x (background + 4 classes)
    assert {0, 1, 63, 64} <= set(counts.tolist()) and 2000 <= len(pk.score) <= 8000
    per_group = [int(pk.box_off[pk.group_off[g + 1]] - pk.box_off[pk.group_off[g]]) for g in range(len(pk.group_off) - 1)]
    assert sum(1 for g, n in enumerate(per_group) if n == 0 and g % 5) >= 1           # a real class without a box
    got = _device(pk)
    _same(got, want)
    assert want[2].sum() > 300 and (want[0] < 0).any() and want[2].max() >= 64


def test_two_runs_give_the_same_bits_and_max_equals_host(batch):
    from i2vsgg_amd import seqnms
    all_boxes, frame_index, pk, want = batch
    _same(_device(pk), _device(pk))
    sub = seqnms.pack(*cases.nested([("a", list(range(3, 40)), {1: cases.gen_cells(np.random.default_rng(8), 37, n_obj=4, clutter=3)})], 2))
    got, host = _device(sub, rescore="max"), seqnms.seq_nms_arrays_host(sub, rescore="max")
    _same(got, host)
    assert not np.array_equal(host[1], seqnms.seq_nms_arrays_host(sub)[1])
    for kw in (dict(link_iou=0.3, nms_iou=0.5), dict(link_iou=0.7, nms_iou=0.1)):    # other thresholds, other tracks
        _same(_device(sub, **kw), seqnms.seq_nms_arrays_host(sub, **kw))


def test_hand_worked_cases_on_the_device():
    from i2vsgg_amd import seqnms
    for name in sorted(cases.HAND):
        pk = seqnms.pack(*cases.hand_nested(name))
        tid, new, n_tracks = _device(pk, **cases.HAND[name].get("kwargs", {}))
        f0 = int(pk.group_off[1])
        assert n_tracks[0] == 0
        cases.check_hand(name, tid, new, n_tracks[1], pk.box_off[f0:] - pk.box_off[f0])


def test_first_track_is_the_brute_force_maximum_on_the_device():
    """All 300 tiny groups in one launch."""
    from i2vsgg_amd import seqnms
    groups = cases.tiny_groups(300)
    pk = seqnms.pack(*cases.tiny_nested(groups))
    assert len(pk.group_off) - 1 == 600
    tid, new, n_tracks = _device(pk)
    checked = 0
    for g, (frame_no, cells) in enumerate(groups):
        f0, f1 = int(pk.group_off[2 * g + 1]), int(pk.group_off[2 * g + 2])
        p, q = int(pk.box_off[f0]), int(pk.box_off[f1])
        if p == q:
            assert n_tracks[2 * g + 1] == 0
            continue
        want = cases.brute_force_best_sum(frame_no, cells)
        got = 0.0
        for s in pk.score[p:q][tid[p:q] == 0]:
            got += float(s)
        assert abs(got - want) <= 1e-12 * abs(want), (g, got, want)
        checked += 1
    assert checked >= 250


def test_public_layout_device_equals_host(batch):
    from i2vsgg_amd import seqnms
    all_boxes, frame_index, pk, want = batch
    dev_out, dev_tr = seqnms.seq_nms(all_boxes, frame_index, device=DEV)
    tid, new = want[0], want[1]
    cells = seqnms.scatter(pk, tid, new)                                            # the host form's answer, laid out by hand
    for j in range(len(all_boxes)):
        for i in range(len(frame_index)):
            if (j, i) not in cells:
                assert len(np.asarray(dev_out[j][i]).reshape(-1, 5)) == 0 and len(dev_tr[j][i]) == 0
                continue
            t, s = cells[(j, i)]
            keep = np.nonzero(t >= 0)[0]
            keep = keep[np.argsort(-s[keep], kind="stable")]
            assert np.array_equal(dev_tr[j][i], t[keep]) and np.array_equal(dev_out[j][i][:, 4], s[keep])
            assert np.array_equal(dev_out[j][i][:, :4], np.asarray(all_boxes[j][i], np.float32)[keep, :4])


def test_seq_nms_runs_on_the_gpu_only():
    from i2vsgg_amd import ops, seqnms
    from i2vsgg_amd._lib import I2VError
    pk = seqnms.pack(*cases.hand_nested("avg"))
    with pytest.raises(I2VError):
        ops.seq_nms(pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score, device="cpu")
    with pytest.raises(ValueError):
        ops.seq_nms(pk.group_off, pk.frame_no, pk.box_off[:-1], pk.box, pk.score, device=DEV)
    tid, new, n_tracks = ops.seq_nms(pk.group_off[:1], pk.frame_no[:0], pk.box_off[:1], pk.box[:0], pk.score[:0], device=DEV)
    assert tid.numel() == 0 and n_tracks.numel() == 0                               # no groups: nothing is launched


# ---------------------------------------------------------------------------------------------------------------------
# the relation loop reads the tracked boxes' scores
# ---------------------------------------------------------------------------------------------------------------------
def test_relation_loop_uses_the_scores_of_an_annotation():
    """An annotation entry with a "scores" key enters with those confidences (lib/utils.py:611), in the frame-by-frame form
    and in the replayed step alike; an entry without the key enters with confidence 1, as before."""
    from i2vsgg_amd import eval as ev, synthetic as syn
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
    H, W = 320, 480
    im = torch.from_numpy(syn.frames(50, 1, H, W)[0]).to(DEV)
    info = np.array([[H, W, 1.0]], np.float32)
    plain = syn.relation_annotation(60, 5, 5, n_rel, n_cls, im_h=H, im_w=W)
    assert "scores" not in plain
    scores = [0.9375, 0.5, 0.75, 0.8125, 0.625]
    net.vrd.target_gt_rels = {"plain": plain, "scored": dict(plain, scores=scores), "ones": dict(plain, scores=[1.0] * 5),
                              "tids": dict(plain, scores=np.asarray(scores, np.float32), tids=[0, 1, 2, 0, 1])}
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)
        it = torch.from_numpy(info).to(DEV)
        data, want = {}, {}
        for key in ("plain", "scored", "ones", "tids"):
            data[key], want[key] = ev.relation_frame(net, im, it, key)
        step = ev.RelationStep(net, frames=2, device=DEV, cap_boxes=6)
        got = step(torch.cat([im, im]), np.concatenate([info, info]), ["scored", "plain"])
        got += step(torch.cat([im, im]), np.concatenate([info, info]), ["ones", "tids"])
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
    assert data["plain"]["scores"] == [1] * 5 and data["scored"]["scores"] == scores
    for res, key in zip(got, ("scored", "plain", "ones", "tids")):                  # the step and the frame form: the same five values
        for a, b in zip(res, want[key]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), key
    for a, b in zip(want["ones"], want["plain"]):                                   # no key == confidence 1 (x * 1.0f is exact)
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(want["tids"], want["scored"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert len(want["scored"][1]) == 100 and not np.array_equal(want["scored"][1], want["plain"][1])
    assert want["scored"][1].max() < want["plain"][1].max()                         # every product has two factors below 1
    # the confidences are rel_score * conf[s] * conf[o] (two fp32 roundings) of the cells the frame form names
    rel = data["scored"]["rel_score"].cpu().numpy()
    pair, pred = want["scored"][4], want["scored"][0][:, 1].astype(np.int64)
    cf = np.asarray(scores, np.float32)
    expect = (rel[pair, pred] * cf[data["scored"]["ixs"][pair]]) * cf[data["scored"]["ixo"][pair]]
    assert np.array_equal(want["scored"][1], expect.astype(np.float32))
