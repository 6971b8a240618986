"""Video relation features on the device: the pooling kernel against its numpy form bit for bit, malformed tables, the relation
step that keeps the head's features, the classifier on pooled features and the scripts end to end."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import relation_feature_cases as cases  # noqa: E402
from relation_feature_cases import bits, load_golden  # noqa: E402
from i2vsgg_amd import relation_features as rf  # noqa: E402
from i2vsgg_amd import synthetic as syn  # noqa: E402

DEV = "cuda:0"
CASES = cases.kernel_cases()
TABLES = ("slot_off", "mem_off", "mem_slot", "mem_idx")


def device_pool(case, feat=None):
    from i2vsgg_amd import ops
    pooled, count = ops.relation_feature_pool(case["feat"] if feat is None else feat, *(case[k] for k in TABLES), device=DEV)
    return pooled.cpu().numpy(), count.cpu().numpy()


def host_pool(case):
    pooled, count, status = rf.pool_arrays_host(case["feat"], *(case[k] for k in TABLES))
    assert status == 0
    return pooled, count


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_host_form_bit_for_bit(name):
    case = CASES[name]
    cases.assert_order_sensitive(case)
    want, want_count = host_pool(case)
    got, count = device_pool(case)
    assert np.array_equal(count, want_count)
    assert np.array_equal(bits(got), bits(want))
    if name == "all_skipped":
        assert not count.any() and not got.any()
    if name == "shared_rows":
        assert len(np.unique(np.concatenate([cases.rows_of(case, r) for r in range(3)]))) <= 6


def test_rows_off_16_bytes_take_the_4_byte_path():
    """dim 300 with the first row 4 bytes past a 16-byte boundary: no 16-byte load may be issued, the bits are the same."""
    case = CASES["dim300"]
    n = case["feat"].size
    buf = torch.zeros(n + 4, device=DEV)
    feat = buf[1:1 + n].view(case["feat"].shape)
    feat.copy_(torch.from_numpy(case["feat"]))
    assert feat.data_ptr() % 16 == 4 and feat.is_contiguous()
    want, want_count = host_pool(case)
    got, count = device_pool(case, feat)
    assert np.array_equal(count, want_count) and np.array_equal(bits(got), bits(want))


def test_golden_on_the_device():
    for store, relations, want in load_golden():
        pooled = rf.pool(relations, store, device=DEV)
        for (vid, pno), row in want.items():
            assert pooled[vid][pno][1] >= 1 and np.array_equal(bits(pooled[vid][pno][0]), bits(row)), (vid, pno)


def test_two_runs_give_the_same_bits():
    case = CASES["some_skipped"]
    a, b = device_pool(case), device_pool(case)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_malformed_tables_give_the_status_and_an_empty_relation():
    """Every table entry is checked against the array sizes before anything is read through it: no fault is provoked."""
    from i2vsgg_amd import _lib, ops
    L = _lib.lib
    case = cases.make_case(31, 8, [4, 6, 5, 3, 7])
    clean = host_pool(case)
    n_slots = len(case["slot_off"]) - 1
    m = int(case["mem_off"][1]) + 2                                                          # a member of relation 1
    past = int(np.diff(case["slot_off"])[case["mem_slot"][m]])
    feat = torch.from_numpy(case["feat"]).to(DEV)
    for table, i, v, bad, same in (("mem_idx", m, past, 1, (0, 2, 3, 4)), ("mem_idx", m, -1, 1, (0, 2, 3, 4)),
                                   ("mem_slot", m, n_slots, 1, (0, 2, 3, 4)), ("mem_slot", m, -2, 1, (0, 2, 3, 4)),
                                   ("mem_off", 3, int(case["mem_off"][2]) - 1, 2, (0, 1, 4))):
        arrays = dict((k, torch.from_numpy(case[k].copy()).to(DEV)) for k in TABLES)
        arrays[table][i] = v
        host = rf.pool_arrays_host(case["feat"], *(arrays[k].cpu().numpy() for k in TABLES))
        pooled = torch.full((5, 8), 7.0, device=DEV)
        count = torch.full((5,), 7, device=DEV, dtype=torch.int32)
        ws = torch.zeros(256, device=DEV, dtype=torch.uint8)
        rc = L.i2v_relation_feature_pool(feat.data_ptr(), *(arrays[k].data_ptr() for k in TABLES), feat.shape[0], n_slots, 5,
                                         arrays["mem_slot"].numel(), 8, pooled.data_ptr(), count.data_ptr(), ws.data_ptr(), 256,
                                         _lib.stream())
        assert rc == 0
        status = int(ws[:4].view(torch.int32).item())
        assert status == bad + 1 == host[2], (table, v, status)
        pooled, count = pooled.cpu().numpy(), count.cpu().numpy()
        assert count[bad] == 0 and not pooled[bad].any()
        assert np.array_equal(bits(pooled), bits(host[0])) and np.array_equal(count, host[1])
        for r in same:
            assert count[r] == clean[1][r] and np.array_equal(bits(pooled[r]), bits(clean[0][r]))
        with pytest.raises(_lib.I2VError, match="relation %d" % bad):
            ops.relation_feature_pool(feat, *(arrays[k] for k in TABLES))
    # argument errors are status codes with text
    t = dict((k, torch.from_numpy(case[k]).to(DEV)) for k in TABLES)
    out, cnt, ws = torch.zeros((5, 8), device=DEV), torch.zeros(5, device=DEV, dtype=torch.int32), torch.zeros(256, device=DEV, dtype=torch.uint8)

    def call(feat_p=feat.data_ptr(), dim=8, ws_bytes=256, slot_p=t["slot_off"].data_ptr()):
        return L.i2v_relation_feature_pool(feat_p, slot_p, t["mem_off"].data_ptr(), t["mem_slot"].data_ptr(), t["mem_idx"].data_ptr(),
                                           feat.shape[0], n_slots, 5, t["mem_slot"].numel(), dim, out.data_ptr(), cnt.data_ptr(),
                                           ws.data_ptr(), ws_bytes, _lib.stream())
    assert call(slot_p=None) == -1 and b"null" in L.i2v_last_error()
    assert call(feat_p=None) == -1 and b"null" in L.i2v_last_error()
    assert call(dim=0) == -1 and b"dim" in L.i2v_last_error()
    assert call(ws_bytes=3) == -1 and b"workspace" in L.i2v_last_error()
    assert call() == 0


def _vrd_args(n_rel=62, n_cls=16):
    return argparse.Namespace(num_relations=n_rel, num_classes=n_cls, emb_dim=300, use_obj_visual=True, spatial_type=2,
                              vrd_task="pre_det")


@pytest.fixture(scope="module")
def frames_run():
    """The shapes of test_relation_step_equals_frame_by_frame_eval (frames=2, cap_boxes=6; 5, 3, 1 and 9 boxes: a frame
    without a slot and a batch that grows the capacity), run once: frame by frame, the step with and without its features."""
    from i2vsgg_amd import eval as ev
    from i2vsgg_amd._lib import TUNE, lib
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.faster_rcnn.resnet_SGG_emb import resnet
    from i2vsgg_amd.model.utils import config as c
    saved = copy.deepcopy(dict(c.cfg))                        # put back below: other modules rely on the cfg they find
    c.cfg_from_file(c.default_cfg_file("res101"))
    c.cfg_from_list(["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30"])
    n_rel, n_cls = 62, 16
    torch.manual_seed(0)
    net = resnet(tuple(range(n_cls)), _vrd_args(), 50, obj_vecs=syn.word_vectors(22, n_cls), prd_vecs=syn.word_vectors(21, n_rel))
    net.create_architecture()
    sd = {k[len("vrd."):]: v for k, v in syn.vrd_params(13).items() if k.startswith("vrd.")}
    load_reference_state(net.vrd, sd, strict=False)
    net.to(DEV).eval()
    H, W = 320, 480
    ims = [torch.from_numpy(syn.frames(50 + i, 1, H, W)[0]).to(DEV) for i in range(4)]
    infos = np.array([[H, W, 1.0], [H, W, 1.25], [H, W, 0.8], [H, W, 1.0]], np.float32)
    nbox = [5, 3, 1, 9]
    keys = ["f%d" % i for i in range(4)]
    net.vrd.target_gt_rels = {keys[i]: syn.relation_annotation(60 + i, nbox[i], min(nbox[i], nbox[i] * (nbox[i] - 1)), n_rel, n_cls,
                                                               im_h=int(H / infos[i, 2]), im_w=int(W / infos[i, 2])) for i in range(4)}
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)         # no split-K atomics: two forwards of a frame are bit-equal
        # the --frames 1 path, inside the block a wrapper of the loop opens: relation_frame appends pre_feat itself
        with ev.keeping_relation_features(rf.ArenaSink(DEV)) as sink:
            single = [ev.relation_frame(net, ims[i], torch.from_numpy(infos[i:i + 1]).to(DEV), keys[i]) for i in range(4)]
            inside = ev.RelationStep(net, frames=2, device=DEV, cap_boxes=6)
            assert inside.keep_features and inside.arena is sink.arena and inside.feat is not None and sink.net is net
        del inside
        feats = [s[0]["pre_feat"].cpu().numpy() if s[1][1] is not None else None for s in single]
        scores = [s[0]["rel_score"].cpu().numpy() if s[1][1] is not None else None for s in single]
        plain = ev.RelationStep(net, frames=2, device=DEV, cap_boxes=6)
        without = plain(torch.cat(ims[:2]), infos[:2], keys[:2]) + plain(torch.cat(ims[2:]), infos[2:], keys[2:])
        assert plain.feat is None and not plain.keep_features and plain.arena is None
        step = ev.RelationStep(net, frames=2, device=DEV, cap_boxes=6, keep_features=True)
        step.arena = rf.arena_for(net.vrd.target_gt_rels, keys, 300, DEV)
        got = step(torch.cat(ims[:2]), infos[:2], keys[:2])
        graphed = step.graph_error is None and bool(step.shapes[step._staged].graph) and step.cap_boxes == 6
        got += step(torch.cat(ims[2:]), infos[2:], keys[2:])    # 9 boxes: the capacity grows, feat is allocated again
        graphed = graphed and step.cap_boxes == 10 and bool(step.shapes[step._staged].graph)
        torch.cuda.synchronize()
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
        c._merge_a_into_b(c.AttrDict(saved), c.cfg)
    return {"net": net, "keys": keys, "nbox": nbox, "single": [s[1] for s in single], "feats": feats, "scores": scores,
            "without": without, "with": got, "arena": step.arena, "graphed": graphed, "frame_arena": sink.arena}


def test_relation_step_keeps_the_features_of_frame_by_frame(frames_run):
    r = frames_run
    arena = r["arena"]
    assert r["graphed"]
    assert arena.n_rows == arena.total_rows == sum(n * (n - 1) for n in r["nbox"] if n >= 2)
    assert list(arena.table) == ["f0", "f1", "f3"]                                          # one box: no slot
    for i, key in enumerate(r["keys"]):
        if r["feats"][i] is None:
            assert key not in arena.table and r["with"][i] == (None,) * 5
            continue
        assert arena.table[key][1] == r["nbox"][i] * (r["nbox"][i] - 1)
        assert np.array_equal(bits(arena.rows_of(key)), bits(r["feats"][i])), key
        assert np.array_equal(bits(r["frame_arena"].rows_of(key)), bits(r["feats"][i])), key
    assert list(r["frame_arena"].table) == ["f0", "f1", "f3"] and r["frame_arena"].n_rows == arena.n_rows
    for f in range(4):                                                                      # the triplets do not change
        for a, b, c in zip(r["with"][f], r["without"][f], r["single"][f]):
            assert (a is None and b is None and c is None) or (
                np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(a), np.asarray(c))), f


def test_classify_of_a_single_member_is_the_frames_score_row(frames_run):
    """A relation with exactly one valid member pools to that pair's feature, and the head's last step on it is the frame's own
    ``rel_score`` row: within 1e-5 absolute, the head tests' ``logits peak`` bound (softmax does not amplify a logit error)."""
    r = frames_run
    arena = r["arena"]
    index = {"f0": ("0", 0), "f1": ("0", 1), "f3": ("0", 3)}
    table = dict((index[k], v) for k, v in arena.table.items())
    rels = {"0": [{"triplet": [1, 2, 3], "duration": [0, 1], "rel_idex": [7]},               # frame 0, pair 7
                  {"triplet": [1, 2, 3], "duration": [1, 4], "rel_idex": [4, 0, 0]},         # frame 1 pair 4; 2 has no slot; 3 pair 0
                  {"triplet": [1, 2, 3], "duration": [2, 4], "rel_idex": [0, 71]}]}          # frame 2 has no slot; frame 3, pair 71
    mem_off, mem_slot, mem_idx, _ = rf.pack(rels, table)
    from i2vsgg_amd import ops
    pooled, count = ops.relation_feature_pool(arena.feat, arena.slot_off, mem_off, mem_slot, mem_idx)
    assert count.tolist() == [1, 2, 1]
    assert np.array_equal(bits(pooled[0].cpu().numpy()), bits(r["feats"][0][7]))
    assert np.array_equal(bits(pooled[2].cpu().numpy()), bits(r["feats"][3][71]))
    prob = rf.classify(r["net"].vrd, pooled).cpu().numpy()
    assert prob.shape == (3, 62) and abs(prob.sum(1) - 1).max() < 1e-5
    err = max(np.abs(prob[0] - r["scores"][0][7]).max(), np.abs(prob[2] - r["scores"][3][71]).max())
    record_margin("test_classify_of_a_single_member_is_the_frames_score_row", "classify vs rel_score row, abs", err, 1e-5)
    assert err <= 1e-5


def test_scripts_end_to_end(tmp_path):
    """video_sgg_emb.py with the three feature flags writes the same relations.pkl and video_relations.json as without them, the
    predicate embeddings, the frame features and one file per relation that pool_relation_features.py --cpu reproduces from
    the files."""
    import pool_relation_features as pf
    import video_sgg_emb as tv
    from i2vsgg_amd._lib import TUNE, lib
    from i2vsgg_amd.model.utils import config as c
    A, B, C = str(tmp_path / "A"), str(tmp_path / "B"), str(tmp_path / "C")
    base = ["--net", "res50", "--imdbval_name", "synthetic_10_v", "--scale", "192", "--frames", "3"]
    hold = {}
    old = lib.i2v_get_tuning(TUNE["I2V_SPLIT_BELOW"])
    saved = copy.deepcopy(dict(c.cfg))                        # the script loads res50.yml and the scales into the global cfg: put it back afterwards
    try:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], 0)         # no split-K atomics: two forwards of a frame are bit-equal
        relations = tv.main(base + ["--output_dir", str(tmp_path / "with"), "--save_feat_path", A, "--save_frame_feats",
                                    "--save_videofeat_path", B], hold=hold)
        sem = rf.semantic_embedding(hold["net"].vrd)           # under the same tuning as the run (the split decides the order)
        tv.main(base + ["--output_dir", str(tmp_path / "without")])
    finally:
        lib.i2v_set_tuning(TUNE["I2V_SPLIT_BELOW"], old)
        c._merge_a_into_b(c.AttrDict(saved), c.cfg)
    for name in ("relations.pkl", "video_relations.json"):
        with open(os.path.join(str(tmp_path / "with"), "res50", "synthetic", name), "rb") as f, \
                open(os.path.join(str(tmp_path / "without"), "res50", "synthetic", name), "rb") as g:
            assert f.read() == g.read(), name
    arena = hold["arena"]
    assert sem.shape == (62, 300) and np.array_equal(bits(np.load(os.path.join(A, "semantic_embedding.npy"))), bits(sem))
    store = rf.from_files(A)
    assert sorted(store.table) == sorted(arena.table) and len(store.table) > 0
    for key in store.table:
        assert np.array_equal(bits(store.rows_of(key)), bits(arena.rows_of(key)))
    n_rel = sum(len(r) for r in relations.values())
    if n_rel == 0:
        # the association left no relation on this set: hand-made ones over the run's frames, one per pair index 0 and 1, the
        # whole video long; through the arena on the device and through the files on the host
        vid = sorted(set(k[0] for k in arena.table))[0]
        fnos = sorted(k[1] for k in arena.table if k[0] == vid)
        lo, hi = 0, fnos[-1] + 1
        relations = {vid: [{"triplet": [1, p, 2], "duration": [lo, hi], "rel_idex": [p] * (hi - lo)} for p in (0, 1)]}
        with open(str(tmp_path / "video_relations.json"), "w") as f:
            json.dump(relations, f)
        rel_file = str(tmp_path / "video_relations.json")
        written, _ = rf.write(rf.pool(relations, arena, device=DEV), relations, B)
        assert written == 2
    else:
        rel_file = os.path.join(str(tmp_path / "with"), "res50", "synthetic", "video_relations.json")
    pf.main(["--relations", rel_file, "--frame_feats", A, "--save_videofeat_path", C, "--cpu"])
    files = sorted(os.path.relpath(os.path.join(d, f), B) for d, _, fs in os.walk(B) for f in fs)
    assert files == sorted(os.path.relpath(os.path.join(d, f), C) for d, _, fs in os.walk(C) for f in fs) and len(files) > 0
    for name in files:
        assert np.array_equal(bits(np.load(os.path.join(B, name))), bits(np.load(os.path.join(C, name)))), name
