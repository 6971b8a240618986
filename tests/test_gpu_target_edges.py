"""The target-assignment path on the device -- ops.bbox_overlaps (bbox_overlaps_kernel, csrc/rpn.hip), ops.bbox_transform
(bbox_transform_kernel, csrc/heads.hip), _AnchorTargetLayer and _ProposalTargetLayer -- on the built cases of tests/target_cases.py:
IoUs exactly on 0.7 / 0.3 / 0.5 / 0.1 / 0.0 and one pixel row to either side, unit boxes on both sides, tied and duplicate
ground truth, frames without ground truth, zero-padded rois, one-class images, both BG_THRESH_LO.  Everything is compared with
the oracle (oracle/rpn.py), which tests/test_target_cases_host.py holds to the exact rules, to the reference's own outputs on
these cases, and shows to differ from every wrong variant (``>`` for ``>=``, last-index argmax, swapped fills, a fused union).

IoUs, labels, weights, sampled rois, dx and dy are compared bit for bit (single-rounded fp32 operations; the library is built with
-ffp-contract=off).  dw and dh go through logf: they are held to the float64 log of the fp32 quotient within LOG_ULP = numpy's
own worst error on the transform cases (tc.numpy_log_ulp, measured in the host test) + 2 ulp for the device's logf; a normalised
target (t - mean) / std to tc.normalised_bound of that.  The observed worst cases are written through
conftest.record_margin (profiles/target_edges_margins.txt is a copy of one run).  Needs a real MI355X: `pytest -m gpu`."""
import copy
import functools

import numpy as np
import pytest
import torch

import target_cases as tc
from conftest import record_margin

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
SET = ["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30"]
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import ops as o
    return o


@pytest.fixture()
def cfg(ops):
    """cfgs/res101.yml; the global cfg singleton is put back afterwards (a test here changes BG_THRESH_LO and BATCH_SIZE)."""
    from i2vsgg_amd.model.utils import config as c
    saved = copy.deepcopy(dict(c.cfg))
    c.cfg_from_file(c.default_cfg_file("res101"))
    c.cfg_from_list(SET)
    assert c.cfg.TRAIN.BG_THRESH_LO == 0.0 and c.cfg.TRAIN.RPN_BATCHSIZE == 256 and tuple(c.cfg.TRAIN.BBOX_NORMALIZE_STDS) == STDS
    assert c.cfg.TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED and tuple(c.cfg.TRAIN.BBOX_NORMALIZE_MEANS) == MEANS
    yield c.cfg
    c._merge_a_into_b(c.AttrDict(saved), c.cfg)


@functools.lru_cache(maxsize=None)
def log_ulp():
    """numpy's own worst log error on the transform cases + 2 ulp for the device's logf."""
    return tc.numpy_log_ulp() + 2.0


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the shared cases are read-only


# ----------------------------------------------------------------------------------------------------------- bbox_overlaps
@functools.lru_cache(maxsize=None)
def _overlap_reference(kind, key):
    """The case and the oracle's (ov, max, argmax) per image, computed once, read-only."""
    from oracle import rpn
    case = {c.name: c for c in tc.edge_overlap_cases()}[key] if kind == "edge" else tc.shape_case(*key)
    ovs = [rpn.iou_matrix(bx, gt) for bx, gt in tc.case_images(case)]
    ref = (np.stack(ovs), np.stack([o.max(1) for o in ovs]), np.stack([o.argmax(1) for o in ovs]).astype(np.int32))
    for a in ref + (case.boxes, case.gt):
        a.setflags(write=False)
    return case, ref


def _check_overlaps(ops, case, ref, what):
    boxes, gt = dev(case.boxes), dev(case.gt)
    ov, mx, am = ops.bbox_overlaps(boxes, gt, want_matrix=True)
    none, mx2, am2 = ops.bbox_overlaps(boxes, gt, want_matrix=False)
    assert none is None and am.dtype == torch.int32
    ov, mx, am, mx2, am2 = (t.cpu().numpy() for t in (ov, mx, am, mx2, am2))
    assert np.array_equal(ov, ref[0]), what
    assert np.array_equal(mx, ref[1]) and np.array_equal(am, ref[2]), what
    assert np.array_equal(mx2, ref[1]) and np.array_equal(am2, ref[2]), what          # the same without the matrix


@pytest.mark.parametrize("name", ["thresholds", "zero_area", "ties", "fractional"])
def test_overlaps_edge_cases(ops, name):
    """IoUs on every constant and a pixel row beside it; unit boxes on both sides (0 column, -1 row, -1 where they meet, argmax 0
    on a row of -1); duplicate and equally overlapped ground truth (first index); fractional boxes (one rounding per operation)."""
    case, ref = _overlap_reference("edge", name)
    _check_overlaps(ops, case, ref, name)
    if name == "thresholds":
        d = np.diagonal(ref[0][0])
        for i, key, side, fam in case.prop["pairs"]:
            if side == "at":
                assert d[i] == F32(float(tc.CONSTANTS[key]))


@pytest.mark.parametrize("B", tc.SHAPE_B)
@pytest.mark.parametrize("form", tc.SHAPE_FORMS)
def test_overlaps_shapes(ops, form, B):
    """K in {1, 20, 30, 64, 1024} x N in {1, 255, 256, 257, 513} for shared (N,4), batched (B,N,4) and (B,N,5) boxes: both
    box_stride / box_off forms, block tails on either side of 256 threads, the documented cap on K."""
    for N in tc.SHAPE_N:
        for K in tc.SHAPE_K:
            case, ref = _overlap_reference("shape", (B, N, K, form))
            assert ref[0].shape == (B, N, K)
            _check_overlaps(ops, case, ref, case.name)


def test_overlaps_rejects_more_than_1024_boxes(ops):
    from i2vsgg_amd._lib import I2VError
    case = tc.shape_case(1, 257, tc.K_OVER_CAP, "shared")
    with pytest.raises(I2VError, match="bbox_overlaps: bad shape"):
        ops.bbox_overlaps(dev(case.boxes), dev(case.gt), want_matrix=True)
    case, ref = _overlap_reference("shape", (1, 257, 1024, "shared"))                  # and the cap itself still runs
    _check_overlaps(ops, case, ref, case.name)


# ----------------------------------------------------------------------------------------------------------- bbox_transform
def _check_targets(got, ex, gt, what, test, normalised=False):
    """got (B,N,4) against the oracle: dx, dy bit for bit; dw, dh within the log bound of the float64 log of the fp32 quotient."""
    from oracle import rpn
    ex = np.broadcast_to(ex if ex.ndim == 3 else ex[None], gt.shape[:2] + (4,))
    want = np.stack([rpn.box_targets(ex[b], gt[b, :, :4]) for b in range(gt.shape[0])])
    if normalised:
        want = ((want - np.asarray(MEANS, F32)) / np.asarray(STDS, F32)).astype(F32)
    assert np.array_equal(got[..., :2], want[..., :2]), what
    bound = tc.normalised_bound(log_ulp()) if normalised else log_ulp()
    seen = tc.log_ulp_of(got, ex, gt, MEANS if normalised else None, STDS if normalised else None)
    record_margin(test, "%s: dw, dh vs float64 log (ulp)" % what, seen, bound)
    assert seen <= bound, (what, seen, bound)
    return seen


@pytest.mark.parametrize("name", ["mixed", "shared"])
def test_bbox_transform_edges(ops, name):
    """ex batched with gt of row stride 5, ex shared with stride 4: ground truth equal to the roi (every component exactly 0),
    unit and one-pixel-wide boxes on either side, rois on the clip border, integer and fractional boxes; plain and normalised."""
    case = {c.name: c for c in tc.transform_cases()}[name]
    ex, gt = dev(case.ex), dev(case.gt)
    plain = ops.bbox_transform(ex, gt).cpu().numpy()
    norm = ops.bbox_transform(ex, gt, MEANS, STDS).cpu().numpy()
    assert plain.shape == case.gt.shape[:2] + (4,) and np.isfinite(plain).all() and np.isfinite(norm).all()
    _check_targets(plain, case.ex, case.gt, name, "test_bbox_transform_edges")
    _check_targets(norm, case.ex, case.gt, name + " normalised", "test_bbox_transform_edges", normalised=True)
    for r in case.prop["zero_rows"]:
        assert (plain[:, r] == 0).all() and (norm[:, r] == 0).all(), r


# ----------------------------------------------------------------------------------------------------------- anchor targets
def _ascene(name):
    return {s.name: s for s in tc.anchor_scenes()}[name]


def _inside_order(x, scene, inside):
    H, W = scene.feat
    B = x.shape[0]
    if x.shape[1] == 1:
        return x.reshape(B, 9, H, W).transpose(0, 2, 3, 1).reshape(B, -1)[:, inside]
    return x.reshape(B, 9, 4, H, W).transpose(0, 3, 4, 1, 2).reshape(B, -1, 4)[:, inside]


def _anchor_layer(cfg):
    from i2vsgg_amd.model.rpn.anchor_target_layer import _AnchorTargetLayer
    return _AnchorTargetLayer(16, cfg.ANCHOR_SCALES, cfg.ANCHOR_RATIOS)


def _anchor_inputs(scene):
    B, (H, W) = scene.gt.shape[0], scene.feat
    nb = (scene.gt[:, :, 2] > 0).sum(1).astype(np.int64)
    return torch.zeros(B, 18, H, W, device=DEV), dev(scene.gt), dev(scene.im_info), dev(nb)


ANCHOR_SCENES = [s.name for s in tc.anchor_scenes()]


@pytest.mark.parametrize("name", ANCHOR_SCENES)
def test_anchor_target_layer_host_sampling(cfg, name):
    """Labels, inside and outside weights bit-equal to the oracle under the reference's seed -- frames without ground truth in
    either order (the weight is the LAST image's), ground truth equal to an anchor and its duplicate, a tiny box whose best
    anchors tie, a box only outside anchors touch, anchors exactly on 0.7 and 0.3, more than 128 foreground anchors, a map whose
    anchors are mostly outside; the targets of every anchor at the bbox_transform bound."""
    from oracle import rpn
    scene = _ascene(name)
    anc, inside, total = tc.scene_anchors(scene)
    want = rpn.anchor_target_layer(*scene.feat, scene.gt, scene.im_info, np.random.RandomState(3))
    np.random.seed(3)
    got = [t.cpu().numpy() for t in _anchor_layer(cfg)(_anchor_inputs(scene))]
    for nm, g, w in zip(("labels", "targets", "inw", "outw"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, nm
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    outside = np.ones(total, bool)
    outside[inside] = False
    H, W = scene.feat
    assert (got[1].reshape(-1, 9, 4, H, W).transpose(0, 3, 4, 1, 2).reshape(-1, total, 4)[:, outside] == 0).all()
    am = np.stack([rpn.iou_matrix(anc, scene.gt[b]).argmax(1) for b in range(scene.gt.shape[0])])
    gt_sel = np.stack([scene.gt[b, am[b]] for b in range(scene.gt.shape[0])])
    _check_targets(_inside_order(got[1], scene, inside), anc, gt_sel, name, "test_anchor_target_layer_host_sampling")


@pytest.mark.parametrize("name", ANCHOR_SCENES)
def test_anchor_target_layer_device_sampling(cfg, name):
    """device_sampling = True draws from torch's generator: what it keeps must be a legal draw of the labels the rules give before
    any subsampling (tc.exact_anchor_labels, which the host test shows to be the oracle's): foreground kept only from foreground,
    min(#fg, 128) of it; background only from background, min(#bg, 256 - kept fg) of it; nothing else labelled; the weight from
    the last image's count.  sample_record holds the labels that went out."""
    scene = _ascene(name)
    anc, inside, total = tc.scene_anchors(scene)
    B = scene.gt.shape[0]
    layer = _anchor_layer(cfg)
    layer.device_sampling, layer.sample_record = True, {}
    torch.manual_seed(5)
    _, gt, info, _ = _anchor_inputs(scene)
    L, T, IW, OW = (t.cpu().numpy() for t in layer.targets_yxa(*scene.feat, gt, info))
    assert np.array_equal(layer.sample_record["labels"].cpu().numpy(), L[:, inside])
    outside = np.ones(total, bool)
    outside[inside] = False
    assert (L[:, outside] == -1).all() and (OW[:, outside] == 0).all() and (IW[:, outside] == 0).all()
    for b in range(B):
        pre, _ = tc.exact_anchor_labels(anc, scene.gt[b])
        lab = L[b, inside]
        assert set(np.unique(lab)) <= {-1.0, 0.0, 1.0}
        assert ((lab == 1) <= (pre == 1)).all() and ((lab == 0) <= (pre == 0)).all(), (name, b)
        n_fg = min(int((pre == 1).sum()), 128)
        assert int((lab == 1).sum()) == n_fg and int((lab == 0).sum()) == min(int((pre == 0).sum()), 256 - n_fg), (name, b)
        assert np.array_equal(IW[b, inside], (lab == 1).astype(F32))
    # the weight is 1 / count by torch's own fp32 division on the device, whose rounding is not this project's to set: one ulp
    w = F32(1.0 / int((L[B - 1, inside] >= 0).sum()))
    assert np.array_equal(OW[:, inside] != 0, L[:, inside] >= 0)
    seen = np.unique(OW[:, inside][L[:, inside] >= 0])
    assert seen.size == 1 and abs(float(seen[0]) - float(w)) <= float(np.spacing(w)), (seen, w)


# ----------------------------------------------------------------------------------------------------------- proposal targets
def _pscene(name):
    return {s.name: s for s in tc.proposal_scenes()}[name]


def _proposal_layer(cfg, lo, R):
    from i2vsgg_amd.model.rpn.proposal_target_layer_cascade import _ProposalTargetLayer
    cfg.TRAIN.BG_THRESH_LO, cfg.TRAIN.BATCH_SIZE = lo, R                              # the cfg fixture puts both back
    return _ProposalTargetLayer(16)


def _proposal_inputs(scene):
    nb = (scene.gt[:, :, 2] > 0).sum(1).astype(np.int64)
    return dev(scene.rois), dev(scene.gt), dev(nb)


PROPOSAL_SCENES = [s.name for s in tc.proposal_scenes()]


@pytest.mark.parametrize("R", tc.PROPOSAL_R)
@pytest.mark.parametrize("lo", tc.BG_LO)
@pytest.mark.parametrize("name", PROPOSAL_SCENES)
def test_proposal_target_layer_host_sampling(cfg, name, lo, R):
    """All five outputs against the oracle under the reference's seed, BG_THRESH_LO = 0.0 (res101.yml) and 0.1 (the default),
    R = 32 and 128: rois, labels and both weights bit-equal, dx and dy bit-equal, dw and dh at the normalised bbox_transform
    bound, every component exactly 0 on background rows.  A scene with an image of neither class (no ground truth and no
    proposals; no ground truth under BG_THRESH_LO = 0.1) raises ValueError, as the reference does."""
    from oracle import rpn
    scene = _pscene(name)
    layer = _proposal_layer(cfg, lo, R)
    np.random.seed(3)
    if tc.raises(scene, lo):
        with pytest.raises(ValueError):
            layer(*_proposal_inputs(scene))
        return
    got = [t.cpu().numpy() for t in layer(*_proposal_inputs(scene))]
    want = rpn.proposal_target_layer(scene.rois, scene.gt, np.random.RandomState(3), batch_size=R, bg_lo=lo)
    for nm, g, w in zip(("rois", "labels", "targets", "inw", "outw"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, nm
        if nm != "targets":
            assert np.array_equal(g, w), nm
    _check_emitted_targets(scene, got, "%s lo %.1f R %d" % (name, lo, R), "test_proposal_target_layer_host_sampling")


def _check_emitted_targets(scene, out, what, test):
    """The targets of emitted (rois, labels, targets): exactly 0 where the label is 0, the normalised transform of the roi
    towards the FIRST best ground-truth box elsewhere."""
    from oracle import rpn
    rois, labels, targets = out[:3]
    assert (targets[labels == 0] == 0).all() and np.isfinite(targets).all(), what
    B = rois.shape[0]
    am = [rpn.iou_matrix(rois[b, :, 1:], scene.gt[b]).argmax(1) for b in range(B)]
    gt_sel = np.stack([scene.gt[b, am[b]] for b in range(B)])
    live = labels > 0
    if live.any():                                                                    # the live rows of all images as one batch
        _check_targets(targets[live][None], rois[live][None, :, 1:], gt_sel[live][None], what, test, normalised=True)


@pytest.mark.parametrize("R", tc.PROPOSAL_R)
@pytest.mark.parametrize("lo", tc.BG_LO)
@pytest.mark.parametrize("name", PROPOSAL_SCENES)
def test_proposal_target_layer_device_sampling(cfg, name, lo, R):
    """device_sampling = True, through sample_record: every slot below nfg holds a roi the oracle calls foreground and every
    other slot one it calls background; nfg is what the rules give; no padding row (zero roi, appended zero ground truth) is
    kept; labels, targets and weights are what the oracle emits for the recorded keep.  An image with neither class (the host
    path raises on it): nfg = 0, all labels 0, finite (zero) targets."""
    from oracle import rpn
    scene = _pscene(name)
    layer = _proposal_layer(cfg, lo, R)
    layer.device_sampling, layer.sample_record = True, {}
    torch.manual_seed(5)
    out = [t.cpu().numpy() for t in layer(*_proposal_inputs(scene))]
    rois, labels, targets, inw, outw = out
    keep, nfg = layer.sample_record["keep"].cpu().numpy(), layer.sample_record["nfg"].cpu().numpy().reshape(-1)
    cand = tc.proposal_candidates(scene)
    B, P = scene.rois.shape[:2]
    assert keep.shape == (B, R) and (keep >= 0).all() and (keep < cand.shape[1]).all()
    fg_per = int(round(0.25 * R))
    for b in range(B):
        ov = rpn.iou_matrix(cand[b, :, 1:], scene.gt[b])
        mx, am = ov.max(1), ov.argmax(1)
        assert np.array_equal(layer.sample_record["max_ov"][b].cpu().numpy(), mx)
        fg, bg = mx >= 0.5, (mx < 0.5) & (mx >= lo)
        regime = scene.prop["regime"][lo][b]
        assert nfg[b] == {"both": min(fg_per, int(fg.sum())), "fg": R, "bg": 0, "none": 0}[regime], (name, b, regime)
        want_rois = cand[b, keep[b]].copy()
        want_rois[:, 0] = b
        assert np.array_equal(rois[b], want_rois)
        if regime == "none":
            assert (labels[b] == 0).all() and (targets[b] == 0).all() and (inw[b] == 0).all() and (outw[b] == 0).all()
            continue
        assert fg[keep[b, :nfg[b]]].all() and bg[keep[b, nfg[b]:]].all(), (name, b)
        if regime == "both":
            assert len(set(keep[b, :nfg[b]].tolist())) == nfg[b]                     # foreground without replacement
        n_real, n_gt = scene.prop["n_real"][b], int((scene.gt[b, :, 2] > 0).sum())
        pad = np.r_[np.arange(n_real, P), np.arange(P + n_gt, cand.shape[1])]
        assert not np.isin(keep[b], pad).any(), (name, b)
        want_lab = scene.gt[b, am[keep[b]], 4].copy()
        want_lab[nfg[b]:] = 0
        assert np.array_equal(labels[b], want_lab)
        if "bg_row" in scene.prop["marks"][b]:
            assert (keep[b, nfg[b]:] == scene.prop["marks"][b]["bg_row"]).all()
    live = np.repeat((labels > 0)[:, :, None], 4, 2).astype(F32)
    assert np.array_equal(inw, live) and np.array_equal(outw, live)
    _check_emitted_targets(scene, out, "%s lo %.1f R %d device" % (name, lo, R), "test_proposal_target_layer_device_sampling")
