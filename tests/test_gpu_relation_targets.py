"""The rel_det targets on the MI355X: csrc/relation_targets.hip (ops.relation_targets) against the host form of
i2vsgg_amd.relation_targets, bit for bit -- both evaluate the same float64 expressions in the same order and every decision of a
draw is integer arithmetic, so no margin is needed -- and the rel_det training forward against the annotated-box task.  The two
loose comparisons (1e-3 relative, the project's tolerance) write what they saw to parity_margins.txt
(profiles/r14_relation_target_margins.txt is a copy of one run)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relation_target_cases as cases  # noqa: E402
from conftest import record_margin  # noqa: E402

DEV = "cuda:0"
REL = 1e-3
N_REL, N_CLS = 62, 16


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from i2vsgg_amd import relation_targets
    return relation_targets


def _device(rt, t, n_rel=cases.N_REL):
    from i2vsgg_amd import ops
    res = ops.relation_targets(*t, n_rel=n_rel, device=DEV, read_status=False)
    return {k: (int(v.item()) if k == "status" else v.cpu().numpy()) for k, v in res.items()}


def test_device_equals_host_form_bit_for_bit(rt):
    n = 0
    for name, t, n_rel in cases.all_cases():
        want = rt.relation_targets_host(*t, n_rel=n_rel)
        cases.same(_device(rt, t, n_rel), want, name)
        n += int(want["n_pairs"].sum())
    dets, annos, info, u = cases.capped_case()
    pk = rt.pack(dets, annos, info, cases.N_REL, u=u)
    cases.same(rt.relation_targets(pk, cases.N_REL, device=DEV), rt.relation_targets(pk, cases.N_REL), "capped")
    assert n > 500


def test_two_runs_give_the_same_bits(rt):
    for name, t, n_rel in cases.all_cases():
        if name in ("three_unequal_frames", "more_than_64_pairs", "candidates_1_9_10_11_4032_u_rng"):
            cases.same(_device(rt, t, n_rel), _device(rt, t, n_rel), name)


def test_malformed_tables_raise_the_status_word_and_spare_the_other_frames(rt):
    from i2vsgg_amd import _lib, ops
    for name, t, bad in cases.malformed_cases():
        cases.check_malformed(_device(rt, t), t, bad)
    name, t, bad = cases.malformed_cases()[0]
    with pytest.raises(_lib.I2VError, match="frame %d" % max(bad)):
        ops.relation_targets(*t, n_rel=cases.N_REL, device=DEV)


def test_empty_minibatch_and_argument_errors(rt):
    from i2vsgg_amd import ops
    z = np.zeros
    res = ops.relation_targets(z(1, np.int32), z((0, 4)), z(0, np.int32), z(1, np.int32), z((0, 4)), z(0, np.int32), z(1, np.int32),
                               z((0, 3), np.int32), z((0, 10), np.uint32), z(0), z(0), n_rel=5, device=DEV)
    assert res["rel5"].shape == (0, 5) and res["samp"].shape == (0, 10, 2)
    with pytest.raises(ValueError, match="sizes"):
        ops.relation_targets(z(3, np.int32), z((0, 4)), z(0, np.int32), z(2, np.int32), z((0, 4)), z(0, np.int32), z(2, np.int32),
                             z((0, 3), np.int32), z((0, 10), np.uint32), z(1), z(1), n_rel=5, device=DEV)


# ---- the training forward ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(rt):
    """ResNet-50 net in training mode without dropout, two frames of 200 x 320 with their annotations; nobody changes its
    weights for good (the optimizer-step test puts them back)."""
    from i2vsgg_amd import synthetic as syn
    from i2vsgg_amd.model.faster_rcnn.resnet_SGG_emb import resnet
    from i2vsgg_amd.model.utils import config as c
    c.cfg_from_file(c.default_cfg_file("res101"))
    c.cfg_from_list(["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30"])
    torch.manual_seed(0)
    args = argparse.Namespace(num_relations=N_REL, num_classes=N_CLS, emb_dim=300, use_obj_visual=True, spatial_type=2, vrd_task="pre_det")
    net = resnet(tuple(range(N_CLS)), args, 50, obj_vecs=syn.word_vectors(22, N_CLS), prd_vecs=syn.word_vectors(21, N_REL))
    net.create_architecture()
    net.vrd.dropout = False
    annos = {"f%d" % i: syn.relation_annotation(40 + i, 6, 5, N_REL, N_CLS, 200, 320) for i in range(2)}
    net.vrd.source_gt_rels = annos
    net.to(DEV).train()
    im, info = syn.frames(9, 2, 200, 320)
    z = torch.zeros(2, 1, 5, device=DEV)
    return net, torch.from_numpy(im).to(DEV), torch.from_numpy(info).to(DEV), z, annos


def _loss_and_grads(net, fn):
    for p in net.parameters():
        p.grad = None
    loss = fn()
    loss.backward()
    return float(loss.item()), {n: p.grad.detach().double().cpu().numpy() for n, p in net.named_parameters() if n.startswith("vrd.")}


def _compare(test, got, want):
    (lg, gg), (lw, gw) = got, want
    worst = abs(lg - lw) / abs(lw)
    record_margin(test, "loss", worst, REL)
    assert worst < REL and lw > 0.1
    assert set(gg) == set(gw) and len(gg) >= 20
    for n in sorted(gw):
        e = np.abs(gg[n] - gw[n]).max() / max(np.abs(gw[n]).max(), 1e-30)
        record_margin(test, "grad " + n, e, REL)
        assert np.abs(gw[n]).max() > 0 and e < REL, (n, e)


# A ReLU unit whose pre-activation lies within the float32 error of its GEMM of zero may fall on either side when the same rows
# go through a GEMM of another height (64 + 64 rows per frame against a handful: other tiles, another split of K), and its
# gradient then appears or vanishes whole: the comparison of two such forwards is only posed away from the kinks.  So, as
# tests/relation_head_ref.py does for the head-only step, the biases are nudged first until no float64 pre-activation of the
# compared rows lies within tau of its layer's largest, tau = 2^-24 (float32) x sqrt(K) (the layer's sum of K products, rounding
# errors adding as a random walk; fc6: K = 50176, tau = 1.1e-4) x 8.  Only the float64 pre-activations decide; no result of the
# forwards under comparison is looked at.  Measured before this was in place, padded against unpadded rows after the tests
# above had run: 3 of fc7's 598 016 outputs on one side of zero in one forward and on the other in the other (the largest of
# them 2.2e-4, where the layer's largest is 870), the fc7 bias gradient of one of those units off by 9.6e-3 of the tensor's
# largest entry, every other unit within 2.4e-7; the same two forwards run alone had no such output and agreed to 3e-7.
TAU = lambda k: 2.0 ** -24 * float(k) ** 0.5 * 8.0
RELU_LAYERS = ("fc6", "fc7", "fc8", "fc_so", "conv_lo.0", "conv_lo.1", "conv_lo.2", "fc_lov", "fc_fusion")      # forward order


def _pre_activation(layer, x):
    """(rows, units) float64, on the device."""
    if hasattr(layer, "fc"):
        return x.double() @ layer.fc.weight.double().t() + layer.fc.bias.double()
    c = layer.conv
    cols = torch.nn.functional.unfold(x[:, :c.cin].double(), c.k, padding=c.pad, stride=c.stride)
    zz = c.weight.double().reshape(c.cout, -1) @ cols + c.bias.double()[None, :, None]
    return zz.permute(0, 2, 1).reshape(-1, c.cout)


def _condition(net, forward):
    """Nudge the ReLU layers' biases, in forward order, until every pre-activation of ``forward``'s rows is at least TAU of the
    layer's largest away from zero (twice that once a bias has to move).  -> {layer: biases moved}; the caller puts the biases
    back (``_biases`` / ``_restore``)."""
    moved = {}
    steps = torch.arange(1, 33, device=DEV, dtype=torch.float64)
    steps = torch.stack((steps, -steps), 1).reshape(-1)                        # +1, -1, +2, -2, ...
    for name in RELU_LAYERS:
        layer = net.vrd.get_submodule(name)
        bias = layer.fc.bias if hasattr(layer, "fc") else layer.conv.bias
        seen = {}
        hook = layer.register_forward_pre_hook(lambda m, a: seen.__setitem__("x", a[0].detach()))
        try:
            for _ in range(6):
                with torch.no_grad():
                    forward()
                    zz = _pre_activation(layer, seen["x"])
                    tau = TAU(seen["x"].shape[1] if hasattr(layer, "fc") else layer.conv.cin * layer.conv.k ** 2) * float(zz.abs().max())
                    units = torch.nonzero((zz.abs() < tau).any(0)).view(-1)
                    if not len(units):
                        break
                    v = zz[:, units]                                           # the smallest shift, a multiple of 2 tau, that clears every row
                    ok = ((v[:, :, None] + 2.0 * tau * steps[None, None, :]).abs() >= 2.0 * tau).all(0)
                    assert bool(ok.any(1).all()), name
                    bias[units] = (bias[units].double() + 2.0 * tau * steps[ok.int().argmax(1)]).float()
                    moved[name] = moved.get(name, 0) + len(units)
            else:
                raise AssertionError("%s: pre-activations near zero after 6 rounds" % name)
        finally:
            hook.remove()
    from i2vsgg_amd import ops
    ops.PARAM_EPOCH += 1                                                       # parameters changed under the caches keyed on them
    return moved


def _biases(net):
    return {n: p.detach().clone() for n, p in net.vrd.named_parameters() if n.endswith("bias")}


def _restore(net, saved):
    from i2vsgg_amd import ops
    with torch.no_grad():
        for n, p in net.vrd.named_parameters():
            if n in saved:
                p.copy_(saved[n])
    ops.PARAM_EPOCH += 1


def test_rel_det_on_the_annotated_boxes_equals_pre_det(rt, model):
    """Detections that are the annotated boxes: every annotated relation has its one candidate, so the rel_det forward sees the
    pre_det forward's pairs (in 64 + 64 padded rows per frame instead of 6 + 5): same loss, same ``vrd.*`` gradients."""
    from i2vsgg_amd import synthetic as syn
    net, im, info, z, annos = model
    net.vrd.source_det_boxes = {k: syn.detections_for(0, a, exact=True) for k, a in annos.items()}
    paths = ["f0", "f1"]
    saved = _biases(net)
    try:
        net.args.vrd_task = "pre_det"
        print("biases nudged:", _condition(net, lambda: net(im, info, z, z, paths)))
        want = _loss_and_grads(net, lambda: net(im, info, z, z, paths))
        net.args.vrd_task = "rel_det"
        got = _loss_and_grads(net, lambda: net(im, info, z, z, paths))
    finally:
        net.args.vrd_task = "pre_det"
        _restore(net, saved)
    assert net.rel_det_n_pairs.tolist() == [5, 5] and net.rel_det_n_dropped.tolist() == [0, 0] and int(net.rel_det_status) == 0
    _compare("test_rel_det_on_the_annotated_boxes_equals_pre_det", got, want)


def test_padded_rows_equal_unpadded_rows(rt, model):
    """Jittered detections, wrong-class copies and distractors: the padded forward against ``vrd.forward_device`` + ``bce_rows``
    on the host form's rows without the padding.  The padding rows add nothing."""
    from i2vsgg_amd import ops, synthetic as syn
    from i2vsgg_amd.model.faster_rcnn.faster_rcnn_SGG_emb import rasterize_masks
    net, im, info, z, annos = model
    paths = ["f0", "f1"]
    dets = {k: syn.detections_for(3 + i, a, jitter=0.12, copies=3, im_h=200, im_w=320) for i, (k, a) in enumerate(annos.items())}
    net.vrd.source_det_boxes = dets
    np.random.seed(11)
    pk = rt.pack([dets[q] for q in paths], [annos[q] for q in paths], info.cpu().numpy(), N_REL)
    host = rt.relation_targets(pk, N_REL)
    n = host["n_pairs"]
    assert n.min() > 5 and n.sum() >= 30                                       # more pairs than the 5 + 5 annotated ones
    rows = np.concatenate([np.arange(f * rt.P, f * rt.P + n[f]) for f in range(2)])
    counts = np.diff(pk.det_off)
    box_rows = np.concatenate([np.arange(f * rt.B, f * rt.B + counts[f]) for f in range(2)])
    remap = np.full(2 * rt.B, -1, np.int64)
    remap[box_rows] = np.arange(len(box_rows))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

    def unpadded():
        with torch.no_grad():
            fmap = net.RCNN_base(im)
        score, _ = net.vrd.forward_device(fmap, t(pk.boxes5[box_rows]), t(host["rel5"][rows]), rasterize_masks(host["bounds"][rows], DEV),
                                          t(remap[host["ixs"][rows]]), t(remap[host["ixo"][rows]]))
        return ops.bce_rows(score, t(host["labels"][rows]), t(host["w"][rows]))

    saved = _biases(net)
    try:
        print("biases nudged:", _condition(net, unpadded))
        want = _loss_and_grads(net, unpadded)
        net.args.vrd_task = "rel_det"
        np.random.seed(11)
        got = _loss_and_grads(net, lambda: net(im, info, z, z, paths))
    finally:
        net.args.vrd_task = "pre_det"
        _restore(net, saved)
    assert net.rel_det_n_pairs.tolist() == n.tolist()
    _compare("test_padded_rows_equal_unpadded_rows", got, want)


def test_one_eager_step_changes_the_relation_head_only(rt, model):
    from i2vsgg_amd import synthetic as syn, train
    net, im, info, z, annos = model
    net.vrd.source_det_boxes = {k: syn.detections_for(3 + i, a, im_h=200, im_w=320) for i, (k, a) in enumerate(annos.items())}
    before = {n: p.detach().clone() for n, p in list(net.named_parameters()) + list(net.named_buffers())}
    opt = train.make_optimizer("sgd", [(n, p) for n, p in net.named_parameters() if n.startswith("vrd.")], 1e-2)
    try:
        net.args.vrd_task = "rel_det"
        opt.zero_grad()
        loss = net(im, info, z, z, ["f0", "f1"])
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        after = dict(list(net.named_parameters()) + list(net.named_buffers()))
        changed = [n for n in before if not torch.equal(before[n], after[n].detach())]
        assert changed and all(n.startswith("vrd.") for n in changed), [n for n in changed if not n.startswith("vrd.")]
        assert {"vrd.fc6.fc.weight", "vrd.fc_rel.fc.weight", "vrd.fc_so.fc.weight", "vrd.conv_lo.0.conv.weight"} <= set(changed)
        assert int(net.rel_det_n_pairs.sum()) > 0
    finally:
        net.args.vrd_task = "pre_det"
        opt.unfuse()
        with torch.no_grad():
            for n, p in list(net.named_parameters()) + list(net.named_buffers()):
                p.copy_(before[n])                        # the fixture's weights, for the tests after this one
        opt.bump()


def test_a_minibatch_without_a_match_has_zero_loss_and_no_pair(rt, model):
    net, im, info, z, annos = model
    far = {"boxes": [[300.0, 180.0, 319.0, 199.0]], "box_classes": [1], "scores": [0.9]}
    wrong = {k: {"boxes": a["boxes"], "box_classes": [c % (N_CLS - 1) + 1 for c in a["box_classes"]], "scores": [1.0] * len(a["boxes"])}
             for k, a in annos.items()}
    try:
        net.args.vrd_task = "rel_det"
        for dets in ({"f0": far, "f1": {"boxes": [], "box_classes": [], "scores": []}}, wrong):
            net.vrd.source_det_boxes = dets
            for p in net.parameters():
                p.grad = None
            loss = net(im, info, z, z, ["f0", "f1"])
            assert float(loss.item()) == 0.0 and int(net.rel_det_n_pairs.sum()) == 0 and int(net.rel_det_status) == 0
            loss.backward()                               # a zero loss still has a (zero) gradient: the loop's exchange needs one
            assert float(net.vrd.fc_rel.fc.weight.grad.abs().max()) == 0.0
    finally:
        net.args.vrd_task = "pre_det"
    with pytest.raises(KeyError, match="source_det_boxes"):
        net.args.vrd_task = "rel_det"
        try:
            net.vrd.source_det_boxes = {}
            net(im, info, z, z, ["f0", "f1"])
        finally:
            net.args.vrd_task = "pre_det"


def test_training_script_runs_rel_det_from_a_detector_checkpoint(rt, tmp_path, capsys):
    """``trainval_sgg_emb.py --vrd_task rel_det`` on the synthetic set at a 192-px shorter side (so ``im_scale`` is not 1 and some
    synthetic detections lie outside the frame), with the reference's ``--r``: every key without 'vrd' comes from the detector
    file.  The global cfg singleton is put back afterwards."""
    import copy
    import trainval_sgg_emb as ts
    from i2vsgg_amd import train
    from i2vsgg_amd.model.utils import config as c
    saved = copy.deepcopy(dict(c.cfg))
    try:
        twin = train.build_sgg_net(50, seed=5, device=DEV)
        det = {k: v.detach().cpu().clone() for k, v in twin.state_dict().items() if "vrd" not in k}
        del twin
        torch.save({"model": det, "pooling_mode": "align", "epoch": 7, "session": 9}, tmp_path / "detector.pth")
        common = ["--net", "res50", "--bs", "2", "--imdb_name", "synthetic_12_v", "--scale", "192", "--iters_per_epoch", "3", "--disp_interval",
                  "3", "--save_dir", str(tmp_path), "--vrd_task", "rel_det"]
        ts.main(common + ["--source_det_boxes_path", "synthetic", "--r", "--load_name", str(tmp_path / "detector.pth")])
        out = capsys.readouterr().out
        assert "(eager, rel_det)" in out and "loss:" in out and "loaded checkpoint" in out
        ck = torch.load(tmp_path / "res50" / "synthetic" / "SGG_emb_p_prior_adap_synthetic_rel_det_session_1_epoch_1_step_2_un.pth",
                        map_location="cpu")
        assert torch.equal(ck["model"]["RCNN_base.6.5.conv3.weight"], det["RCNN_base.6.5.conv3.weight"])
        assert all(torch.isfinite(v).all() for v in ck["model"].values() if v.is_floating_point())
        with pytest.raises(SystemExit) as e:
            ts.main(common)
        assert "--source_det_boxes_path" in str(e.value)
        with pytest.raises(SystemExit):
            ts.main(common + ["--source_det_boxes_path", "synthetic", "--resume_train"])
    finally:
        c._merge_a_into_b(c.AttrDict(saved), c.cfg)
