#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING THE REFERENCE's own Python in this container.

Build-container only: needs /root/reference (read-only) and never ships to the GPU box;
only the .npz outputs do.  Inputs are regenerated from seeds by i2vsgg_amd.synthetic, so
the fixtures hold reference OUTPUTS (plus the few inputs that are cheaper to store than to
regenerate).

Two tiers, recorded per file in the ``tier`` field:
  "direct"       the reference module imports as shipped (sys.path only):
                 rpn/generate_anchors.py, rpn/bbox_transform.py, nms/nms_cpu.py, datasets/voc_eval.py (by path)
  "extracted"    roi_align/src/roi_align.c:80-136 ``ROIAlignForwardCpu``: the file as a whole needs <TH/TH.h> (its
                 THFloatTensor wrappers), the function itself only <math.h>; oracle/build_ref.py pipes the function's
                 own text to gcc unmodified (no stand-in header, nothing of it written to disk but the .so)
                 lib/utils.py:584-628 ``detection_output``: the module cannot be imported (a module-level json.load of an
                 absolute path), so the function's own lines are compiled from the file and run unmodified, with the
                 ``np.float`` alias numpy 1.24 removed restored for the call; the same for its video functions (_iou,
                 VideoRelation, greedy_relational_association, association, viou, eval_*_scores, voc_ap, evaluate)
  "placeholders" the module imports after registering in-process placeholders for
                 three third-party packages absent from this image and for the
                 reference's un-buildable compiled extensions:
                   easydict.EasyDict  -> attribute-access dict (what the package is)
                   torchvision, cv2   -> empty modules (imported, unused on this path)
                   model.<ext>._ext   -> empty modules (torch.utils.ffi builds, gone in torch>=1.0)
                   model._C           -> roi_pool_forward backed by oracle.cops (vrd only;
                                         the real source is absent from the reference tree)
                 The reference's own code runs unmodified.
"""
import argparse
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "lib"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from i2vsgg_amd import synthetic as syn  # noqa: E402
from oracle import cops  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def save(name, tier, **arrays):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, tier=np.array(tier), **arrays)
    print("  wrote %-38s %8.1f KB  [%s]" % (name + ".npz", os.path.getsize(path) / 1024.0, tier))


# ----------------------------------------------------------------------------- tier "direct"
def gen_direct():
    from model.rpn.generate_anchors import generate_anchors
    from model.rpn import bbox_transform as bt
    from model.nms.nms_cpu import nms_cpu

    base = generate_anchors(scales=np.array([8, 16, 32]), ratios=np.array([0.5, 1, 2]))
    # the shift-grid recipe of proposal_layer.py:81-95, executed with the reference's base anchors
    H, W, stride = 38, 63, 16
    sx, sy = np.meshgrid(np.arange(0, W) * stride, np.arange(0, H) * stride)
    shifts = torch.from_numpy(np.vstack((sx.ravel(), sy.ravel(), sx.ravel(), sy.ravel())).transpose()).contiguous().float()
    anc = (torch.from_numpy(base).float().view(1, 9, 4) + shifts.view(-1, 1, 4)).view(-1, 4)
    save("anchors", "direct", base=base, grid_38x63=anc.numpy())

    # decode + clip on seeded deltas (B=2 so that per-image clip limits differ)
    rng = np.random.default_rng(101)
    deltas = (rng.standard_normal((2, anc.shape[0], 4)) * np.array([0.3, 0.3, 0.5, 0.5])).astype(np.float32)
    im_info = np.array([[600, 1000, 1.0], [576, 992, 1.2]], np.float32)
    boxes = anc.view(1, -1, 4).expand(2, -1, 4)
    prop = bt.bbox_transform_inv(boxes, torch.from_numpy(deltas), 2)
    prop = bt.clip_boxes(prop, torch.from_numpy(im_info), 2)
    save("decode_clip", "direct", im_info=im_info, proposals=prop.numpy())

    # IoU and regression targets
    gt, _ = syn.gt_boxes(5, 2, 8)
    rois = np.stack([syn.boxes(50 + b, 300) for b in range(2)])
    rois[0, 5] = [10, 10, 10, 10]                      # zero-area roi -> -1 row
    ov3 = bt.bbox_overlaps_batch(torch.from_numpy(rois), torch.from_numpy(gt))
    ov2 = bt.bbox_overlaps_batch(anc[::7].contiguous(), torch.from_numpy(gt))
    ex = torch.from_numpy(rois)
    gts = torch.from_numpy(np.stack([syn.boxes(70 + b, 300) for b in range(2)]))
    tg = bt.bbox_transform_batch(ex, gts)
    save("box_math", "direct", rois=rois, gt=gt, overlaps_rois=ov3.numpy(), overlaps_anchors=ov2.numpy(),
         tgt_gt=gts.numpy(), targets=tg.numpy())

    # NMS keep lists on tie-free, pre-sorted dets
    out = {}
    for n in (1, 2, 63, 64, 65, 300, 1000, 6000, 12000):
        for clustered in (False, True):
            dets = syn.tie_free_dets(1000 + n, n, clustered=clustered)
            for th in (0.7, 0.3):
                keep = nms_cpu(torch.from_numpy(dets), th).numpy().astype(np.int32)
                out["n%d_%s_t%02d" % (n, "c" if clustered else "u", int(th * 10))] = keep
    save("nms_keep", "direct", **out)


# ----------------------------------------------------------------------------- RoIAlign: the reference's own C (tier "extracted")
def gen_roi_align():
    """``ROIAlignForwardCpu`` (roi_align/src/roi_align.c:80-136) -- the function's own text compiled
    where it lies by oracle/build_ref.py (self-contained: <math.h> only; the THFloatTensor wrappers at :16-78 are not
    built) -- on 8x8 grids, and ``RoIAlignAvg``'s ``avg_pool2d(x, kernel_size=2, stride=1)`` of it
    (roi_align/modules/roi_align.py:27-29) -> 7x7, for C in {4, 64, 1024} over ROIs of every class (seeded, full-image,
    sub-pixel, malformed, partly outside, beyond the far edge, single point).  Full tensors up to C = 64; the C = 1024 case
    (7.9 MB) as sha256 of the bytes + sums + a strided sample."""
    import hashlib
    from oracle import build_ref
    build_ref.build()
    out = {}
    for C, H, W, B in syn.ROI_ALIGN_GOLDEN_CASES:
        feat, rois = syn.roi_align_golden_inputs(C, H, W, B)
        a8 = build_ref.roi_align_fwd(feat, rois, 8, 8, 1.0 / 16.0)
        a7 = torch.nn.functional.avg_pool2d(torch.from_numpy(a8), kernel_size=2, stride=1).numpy()
        p7 = build_ref.roi_align_fwd(feat, rois, 7, 7, 1.0 / 16.0)           # RoIAlign(7,7): the un-averaged module
        tag = "c%d" % C
        out[tag + "_rois"] = rois
        for key, v in (("a8", a8), ("avg7", a7), ("p7", p7)):
            out["%s_%s_shape" % (tag, key)] = np.array(v.shape)
            out["%s_%s_sha256" % (tag, key)] = np.array(hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
            out["%s_%s_sum" % (tag, key)] = np.array(v.astype(np.float64).sum())
            out["%s_%s_abs" % (tag, key)] = np.array(np.abs(v.astype(np.float64)).sum())
            if C <= 64:
                out["%s_%s" % (tag, key)] = v
            else:
                out["%s_%s_sample" % (tag, key)] = v.reshape(-1)[::211].copy()
        same = np.array_equal(a8, cops.roi_align_fwd(feat, rois, 8, 8, 1.0 / 16.0))
        print("   C=%4d: 8x8 %s |sum| %.4e   oracle restatement bit-equal: %s" % (C, a8.shape, np.abs(a8).sum(), same))
    save("roi_align_fwd", "extracted", **out)


def gen_roi_align_fresh():
    """``ROIAlignForwardCpu`` (oracle/build_ref.py, as gen_roi_align) on the shapes of tests/roi_align_pin.py FRESH_SHAPES --
    non-square grids and another scale, which roi_align_fwd.npz does not hold: the ROIs and the full outputs (~95k floats)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import build_ref
    from roi_align_pin import fresh_roi_align_inputs
    build_ref.build()
    out = {}
    for i, (feat, rois, ah, aw, scale) in enumerate(fresh_roi_align_inputs()):
        ref = build_ref.roi_align_fwd(feat, rois, ah, aw, scale)
        out["s%d_rois" % i] = rois
        out["s%d_feat_sum" % i] = np.array(feat.astype(np.float64).sum())
        out["s%d_out" % i] = ref
        same = np.array_equal(ref, cops.roi_align_fwd(feat, rois, ah, aw, scale))
        print("   %s %dx%d scale %g: oracle restatement bit-equal: %s" % (feat.shape, ah, aw, scale, same))
    save("roi_align_fwd_fresh", "extracted", **out)


# ----------------------------------------------------------------------------- the two eval tails
def gen_eval_tails():
    """f1: the per-image detection loop of test_net_instance_styleD_bilinear.py:151-221 driven with the reference's own
    importable pieces (bbox_transform_inv, clip_boxes, nms_cpu -- what model.nms.nms_wrapper.nms always calls) in the loop's
    order.  The loop itself lives in a script that needs a dataset and a checkpoint, so its control flow is restated here, line
    by line; every arithmetic step is the reference's function.  Tier "direct".
    f3: lib/utils.py:584-628 ``detection_output``.  lib/utils.py cannot be imported (a module-level json.load of an absolute
    path, :34-35), so the function's own source lines are compiled from the file (ast) and run unmodified; it spells the
    float64 dtype ``np.float``, an alias numpy removed in 1.24 -- restored for the call.  Tier "extracted"."""
    import ast
    from model.rpn import bbox_transform as bt
    from model.nms.nms_cpu import nms_cpu

    def nms(dets, thresh):                                  # nms_wrapper.py:13-20
        if dets.shape[0] == 0:
            return []
        return nms_cpu(dets.cpu(), thresh)

    out = {}
    for tag, (C, R, thresh, scale, agnostic) in {"c16": (16, 300, 0.0, 1.6, False), "c8_t05": (8, 120, 0.05, 1.0, False),
                                                 "c16_cag": (16, 300, 0.0, 1.25, True)}.items():
        rng = np.random.default_rng(900 + C + R)
        im_h, im_w = 600.0, 1000.0
        xy = rng.uniform(0, 1, (R, 2)) * [im_w - 120, im_h - 120]
        wh = rng.uniform(16, 300, (R, 2))
        rois = np.concatenate([np.zeros((R, 1)), xy, np.minimum(xy + wh, [im_w - 1, im_h - 1])], 1).astype(np.float32)
        logits = (rng.standard_normal((R, C)) * 2).astype(np.float32)
        prob = torch.softmax(torch.from_numpy(logits), 1).numpy()
        assert len(np.unique(prob)) == prob.size                         # tie-free scores
        pred = (rng.standard_normal((R, 4 if agnostic else 4 * C)) * 0.5).astype(np.float32)
        stds, means = (0.1, 0.1, 0.2, 0.2), (0.0, 0.0, 0.0, 0.0)         # cfg.TRAIN.BBOX_NORMALIZE_STDS / _MEANS
        # ---- :151-171
        scores = torch.from_numpy(prob).view(1, R, C)
        boxes = torch.from_numpy(rois).view(1, R, 5)[:, :, 1:5]
        im_info = torch.tensor([[im_h, im_w, scale]])
        box_deltas = torch.from_numpy(pred).view(1, R, -1)
        box_deltas = box_deltas.view(-1, 4) * torch.FloatTensor(stds) + torch.FloatTensor(means)
        box_deltas = box_deltas.view(1, -1, 4) if agnostic else box_deltas.view(1, -1, 4 * C)
        pred_boxes = bt.bbox_transform_inv(boxes, box_deltas, 1)
        pred_boxes = bt.clip_boxes(pred_boxes, im_info, 1)
        pred_boxes /= im_info[0][2].item()
        scores = scores.squeeze()
        pred_boxes = pred_boxes.squeeze()
        # ---- :181-207
        all_boxes = [np.zeros((0, 5), np.float32)]
        for j in range(1, C):
            inds = torch.nonzero(scores[:, j] > thresh).view(-1)
            if inds.numel() > 0:
                cls_scores = scores[:, j][inds]
                _, order = torch.sort(cls_scores, 0, True)
                cls_boxes = pred_boxes[inds, :] if agnostic else pred_boxes[inds][:, j * 4:(j + 1) * 4]
                cls_dets = torch.cat((cls_boxes, cls_scores.unsqueeze(1)), 1)
                cls_dets = cls_dets[order]
                keep = nms(cls_dets, 0.3)                   # cfg.TEST.NMS
                cls_dets = cls_dets[keep.view(-1).long()]
                all_boxes.append(cls_dets.cpu().numpy())
            else:
                all_boxes.append(np.zeros((0, 5), np.float32))
        # ---- :214-221
        max_per_image = 100
        image_scores = np.hstack([all_boxes[j][:, -1] for j in range(1, C)])
        before = len(image_scores)
        if len(image_scores) > max_per_image:
            image_thresh = np.sort(image_scores)[-max_per_image]
            for j in range(1, C):
                keepj = np.where(all_boxes[j][:, -1] >= image_thresh)[0]
                all_boxes[j] = all_boxes[j][keepj, :]
        out[tag + "_rois"], out[tag + "_prob"], out[tag + "_pred"] = rois, prob, pred
        out[tag + "_args"] = np.array([im_h, im_w, scale, float(agnostic), thresh, 0.3, max_per_image], np.float64)
        out[tag + "_count"] = np.array([a.shape[0] for a in all_boxes], np.int32)
        out[tag + "_dets"] = np.concatenate(all_boxes, 0).astype(np.float32)
        print("    detection loop %-8s %3d rois x %2d classes: %4d detections after NMS, %3d kept" % (
            tag, R, C, before, out[tag + "_dets"].shape[0]))
    save("det_postprocess", "direct", **out)

    # ---- f3: detection_output, compiled from its own lines of lib/utils.py
    path = os.path.join(REF, "lib", "utils.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "detection_output")
    assert (fn.lineno, fn.end_lineno) == (584, 627), (fn.lineno, fn.end_lineno)      # :628 is the blank line after the return
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    detection_output = ns["detection_output"]
    had = hasattr(np, "float")
    if not had:
        np.float = float                                    # the alias numpy 1.24 removed (the function's dtype spelling)
    try:
        out = {}
        for tag, (nb, nrel) in {"b9": (9, 26), "b5": (5, 26), "b16": (16, 62), "b1": (1, 26)}.items():
            rng = np.random.default_rng(77 + nb)
            xy = rng.uniform(0, 400, (nb, 2))
            bboxes = np.concatenate([xy, xy + rng.uniform(20, 200, (nb, 2))], 1)
            classes = rng.integers(1, 16, nb)
            confs = rng.uniform(0.05, 1.0, nb).astype(np.float32)
            pairs = [(i, j) for i in range(nb) for j in range(nb) if i != j]        # faster_rcnn_SGG_emb.py:597-606
            ixs, ixo = np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)
            rel = torch.softmax(torch.from_numpy(rng.standard_normal((max(len(pairs), 1), nrel)).astype(np.float32) * 2), 1)
            vrd_data = {"bboxes": bboxes, "classes": classes, "scores": confs, "ixs": ixs, "ixo": ixo, "rel_score": rel.clone(),
                        "rel_so_prior": None}
            res = detection_output(vrd_data)
            out[tag + "_bboxes"], out[tag + "_classes"], out[tag + "_scores"] = bboxes, classes, confs
            out[tag + "_ixs"], out[tag + "_ixo"], out[tag + "_rel_score"] = ixs, ixo, rel.numpy()
            if res[0] is None:
                out[tag + "_none"] = np.array(1)
                continue
            rlp, conf, sub, obj, idx = res
            assert len(np.unique(conf)) == conf.size        # tie-free ranking
            out[tag + "_rlp"], out[tag + "_conf"], out[tag + "_sub"], out[tag + "_obj"], out[tag + "_idx"] = rlp, conf, sub, obj, idx
            print("    detection_output %-4s %2d boxes, %3d pairs x %2d predicates -> %3d triplets, best %.4f" % (
                tag, nb, len(pairs), nrel, conf.size, conf[0]))
    finally:
        if not had:
            del np.float
    save("detection_output", "extracted", **out)


# ----------------------------------------------------------------------------- placeholders
class _AttrDict(dict):
    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = v

    def __setitem__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, _AttrDict):
            v = _AttrDict(v)
        super().__setitem__(k, v)

    __setattr__ = __setitem__

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def install_placeholders():
    ed = types.ModuleType("easydict")
    ed.EasyDict = _AttrDict
    sys.modules["easydict"] = ed
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    sys.modules["cv2"] = types.ModuleType("cv2")
    for ext in ("roi_align", "roi_pooling", "roi_crop", "nms"):
        m = types.ModuleType("model.%s._ext" % ext)
        setattr(m, ext, types.ModuleType(ext))
        sys.modules["model.%s._ext" % ext] = m
        sys.modules["model.%s._ext.%s" % (ext, ext)] = getattr(m, ext)

    import yaml
    from model.utils import config
    with open(os.path.join(REF, "cfgs", "res101.yml")) as f:
        config._merge_a_into_b(_AttrDict(yaml.safe_load(f)), config.cfg)
    config.cfg_from_list(["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]",
                          "MAX_NUM_GT_BOXES", "30"])          # parser_func.py:198-199
    return config.cfg


def _rpn_inputs(seed, B, H=38, W=63):
    """Synthetic rpn_cls_prob / rpn_bbox_pred maps with tie-free fg scores."""
    rng = np.random.default_rng(seed)
    n = B * 9 * H * W
    fg = (rng.permutation(n).astype(np.float32) + 1.0) / np.float32(n + 2)     # distinct, in (0,1)
    fg = fg.reshape(B, 9, H, W)
    prob = np.concatenate([1.0 - fg, fg], 1).astype(np.float32)
    deltas = (rng.standard_normal((B, 36, H, W)) * 0.25).astype(np.float32)
    return prob, deltas


def gen_rpn_layers(cfg):
    from model.rpn.proposal_layer import _ProposalLayer
    from model.rpn.anchor_target_layer import _AnchorTargetLayer
    from model.rpn.proposal_target_layer_cascade import _ProposalTargetLayer

    layer = _ProposalLayer(16, cfg.ANCHOR_SCALES, cfg.ANCHOR_RATIOS)
    out = {}
    for B in (1, 2):
        prob, deltas = _rpn_inputs(200 + B, B)
        info = np.array([[600, 1000, 1.0], [600, 1000, 1.0]], np.float32)[:B]
        for mode, key, target, post in (("train", "TRAIN", False, None), ("test", "TEST", False, None),
                                        ("target", "TRAIN", True, 32), ("target128", "TRAIN", True, 128)):
            if post is not None:
                cfg.TRAIN.RPN_POST_NMS_TOP_N_TARGET = post
            rois = layer((torch.from_numpy(prob), torch.from_numpy(deltas), torch.from_numpy(info), key),
                         target=target)
            out["rois_B%d_%s" % (B, mode)] = rois.numpy()
    cfg.TRAIN.RPN_POST_NMS_TOP_N_TARGET = 128
    save("proposal_layer", "placeholders", **out)

    # anchor targets: np.random call order is part of the contract (seed = cfg.RNG_SEED = 3)
    atl = _AnchorTargetLayer(16, cfg.ANCHOR_SCALES, cfg.ANCHOR_RATIOS)
    out = {}
    for B in (1, 2):
        gt, nb = syn.gt_boxes(300 + B, B, 8)
        info = torch.tensor([[600, 1000, 1.0]] * B)
        np.random.seed(3)
        res = atl((torch.zeros(B, 18, 38, 63), torch.from_numpy(gt), info, torch.from_numpy(nb)))
        for name, t in zip(("labels", "targets", "inw", "outw"), res):
            out["B%d_%s" % (B, name)] = t.numpy()
    save("anchor_target", "placeholders", **out)

    ptl = _ProposalTargetLayer(16)
    out = {}
    for B, R in ((1, 128), (2, 32), (4, 128)):         # (4, 128): one branch of the yml's own step (TRAIN.BATCH_SIZE: 128)
        cfg.TRAIN.BATCH_SIZE = R
        gt, nb = syn.gt_boxes(400 + B, B, 8)
        rois = np.zeros((B, 2000, 5), np.float32)
        for b in range(B):
            rois[b, :, 0] = b
            rois[b, :, 1:] = syn.boxes(410 + b, 2000, min_side=24, max_side=380)
            # make some proposals near gt so that fg exists
            jit = np.random.default_rng(420 + b).normal(0, 8, (64, 4)).astype(np.float32)
            rois[b, :64, 1:] = np.clip(gt[b, np.arange(64) % 8, :4] + jit, 0, [999, 599, 999, 599])
        np.random.seed(3)
        res = ptl(torch.from_numpy(rois), torch.from_numpy(gt), torch.from_numpy(nb))
        for name, t in zip(("rois", "labels", "targets", "inw", "outw"), res):
            out["B%d_R%d_%s" % (B, R, name)] = t.numpy()
    cfg.TRAIN.BATCH_SIZE = 128
    save("proposal_target", "placeholders", **out)


def gen_target_edges(cfg):
    """tests/golden/target_edges.npz: the reference's own bbox_overlaps_batch, bbox_transform_batch, _AnchorTargetLayer and
    _ProposalTargetLayer on the built cases of tests/target_cases.py.  Outputs only -- the inputs are rebuilt from the builders.
    Kept small: overlap matrices for the edge cases, max / argmax alone for the shape grid (shared boxes, one image); anchor
    targets only where the outside weight is non-zero (the labelled anchors: what the loss reads); labels as int8.  A scene the
    reference raises on is kept out and the exception's text recorded under ``<key>_error``."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import target_cases as tc
    from model.rpn import bbox_transform as bt
    from model.rpn.anchor_target_layer import _AnchorTargetLayer
    from model.rpn.proposal_target_layer_cascade import _ProposalTargetLayer
    t = torch.from_numpy
    out = {}

    def overlaps(case):
        return bt.bbox_overlaps_batch(t(case.boxes), t(case.gt)).numpy()
    for case in tc.edge_overlap_cases():
        ov = overlaps(case)
        mx, am = torch.max(t(ov), 2)
        out.update({"ov_%s_ov" % case.name: ov, "ov_%s_max" % case.name: mx.numpy(), "ov_%s_argmax" % case.name: am.numpy().astype(np.int16)})
    for N in tc.SHAPE_N:
        for K in tc.SHAPE_K:
            case = tc.shape_case(1, N, K, "shared")
            mx, am = torch.max(t(overlaps(case)), 2)
            out.update({"sh_%s_max" % case.name: mx.numpy(), "sh_%s_argmax" % case.name: am.numpy().astype(np.int16)})
    for case in tc.transform_cases():
        out["tf_%s_targets" % case.name] = bt.bbox_transform_batch(t(case.ex), t(case.gt)).numpy()

    atl = _AnchorTargetLayer(16, cfg.ANCHOR_SCALES, cfg.ANCHOR_RATIOS)
    for sc in tc.anchor_scenes():
        B, (H, W) = sc.gt.shape[0], sc.feat
        nb = (sc.gt[:, :, 2] > 0).sum(1).astype(np.int64)
        np.random.seed(3)
        try:
            L, T, IW, OW = (x.numpy() for x in atl((torch.zeros(B, 18, H, W), t(sc.gt), t(sc.im_info), t(nb))))
        except Exception as e:                                            # noqa: BLE001 -- whatever the reference raises
            out["at_%s_error" % sc.name] = np.array("%s: %s" % (type(e).__name__, e))
            print("    anchor scene %s: the reference raises %s: %s" % (sc.name, type(e).__name__, e))
            continue
        assert np.array_equal(L, L.astype(np.int8)) and np.array_equal(IW, (IW > 0).astype(np.float32))
        out.update({"at_%s_labels" % sc.name: L.astype(np.int8), "at_%s_inw" % sc.name: (IW > 0), "at_%s_outw" % sc.name: OW,
                    "at_%s_targets_labelled" % sc.name: T[OW > 0]})

    ptl = _ProposalTargetLayer(16)
    saved = (cfg.TRAIN.BG_THRESH_LO, cfg.TRAIN.BATCH_SIZE)
    for sc in tc.proposal_scenes():
        nb = (sc.gt[:, :, 2] > 0).sum(1).astype(np.int64)
        for lo in tc.BG_LO:
            for R in tc.PROPOSAL_R:
                cfg.TRAIN.BG_THRESH_LO, cfg.TRAIN.BATCH_SIZE = lo, R
                key = "pt_%s_lo%02d_R%d" % (sc.name, int(lo * 10), R)
                np.random.seed(3)
                try:
                    res = ptl(t(sc.rois), t(sc.gt), t(nb))
                except Exception as e:                                    # noqa: BLE001
                    out[key + "_error"] = np.array("%s: %s" % (type(e).__name__, e))
                    print("    proposal scene %s: the reference raises %s: %s" % (key, type(e).__name__, e))
                    continue
                for name, x in zip(("rois", "labels", "targets", "inw", "outw"), res):
                    out["%s_%s" % (key, name)] = x.numpy()
    cfg.TRAIN.BG_THRESH_LO, cfg.TRAIN.BATCH_SIZE = saved
    save("target_edges", "placeholders", **out)


def _load(module, params, prefix):
    sd = {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}
    missing = module.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys, missing.unexpected_keys
    left = [k for k in missing.missing_keys if "num_batches_tracked" not in k]
    assert not left, left
    return module


def gen_nets(cfg):
    import model.faster_rcnn.resnet_instance_styleD_bilinear as R
    from model.rpn.rpn import _RPN
    from model.utils.net_utils import _smooth_l1_loss

    # --- discriminators: outputs + grads through the GRL
    p = syn.netd_params(12)
    dp = _load(R.netD_pixel(context=True), p, "netD_pixel.")
    ds = _load(R.netD_style(context=True), p, "netD_style.")
    rng = np.random.default_rng(500)
    x = torch.from_numpy(rng.standard_normal((6, 1024, 7, 7), dtype=np.float32)).requires_grad_()
    d, feat = dp(x, 0.1)
    loss = 0.5 * torch.mean(d ** 2) + feat.sum() * 1e-3
    loss.backward()
    out = dict(pix_d=d.detach().numpy(), pix_feat=feat.detach().numpy(), pix_gx=x.grad.numpy()[:, ::16].copy(),
               pix_gw1=dp.conv1.weight.grad.numpy()[:8], pix_gw3=dp.conv3.weight.grad.numpy())
    y = torch.from_numpy(rng.standard_normal((2, 512, 19, 32), dtype=np.float32)).requires_grad_()
    d, feat = ds(y, 0.01)
    loss = 0.5 * torch.mean((1 - d) ** 2)
    loss.backward()
    out.update(sty_d=d.detach().numpy(), sty_feat=feat.detach().numpy(), sty_gx=y.grad.numpy()[:, ::16].copy(),
               sty_gw1=ds.fc_1.weight.grad.numpy()[:16], sty_gb2=ds.fc_2.bias.grad.numpy(),
               sty_gfc1=ds.fc1.weight.grad.numpy())
    save("discriminators", "placeholders", **out)

    # --- backbone pieces on reduced spatial size (ResNet-101 blocks, frozen BN, eval)
    bp = syn.backbone_params(0, 101)
    net = R.resnet101()
    sd = {}
    names = {"RCNN_base.0": "conv1", "RCNN_base.1": "bn1", "RCNN_base.4": "layer1", "RCNN_base.5": "layer2",
             "RCNN_base.6": "layer3", "RCNN_top.0": "layer4"}
    for k, v in bp.items():
        for a, b in names.items():
            if k.startswith(a + "."):
                sd[b + k[len(a):]] = v
    miss = net.load_state_dict(sd, strict=False)
    assert not miss.unexpected_keys
    assert all(("fc." in k) or ("num_batches" in k) for k in miss.missing_keys), miss.missing_keys
    net.eval()
    base = torch.nn.Sequential(net.conv1, net.bn1, net.relu, net.maxpool, net.layer1, net.layer2, net.layer3)
    im, _ = syn.frames(600, 2, 97, 131)
    with torch.no_grad():
        x = torch.from_numpy(im)
        taps = {}
        for i, m in enumerate(base):
            x = m(x)
            if i in (3, 4, 5, 6):
                taps["after_%d" % i] = x.numpy()
        rng = np.random.default_rng(601)
        pool5 = torch.from_numpy(rng.standard_normal((3, 1024, 7, 7), dtype=np.float32))
        taps["head_to_tail"] = net.layer4(pool5).mean(3).mean(2).numpy()
    # keep the fixture small: layer taps as (sum, abs-sum, strided sample) + the final map in full
    out = {}
    for k, v in taps.items():
        out[k + "_shape"] = np.array(v.shape)
        out[k + "_sum"] = np.array(v.astype(np.float64).sum())
        out[k + "_abs"] = np.array(np.abs(v.astype(np.float64)).sum())
        out[k + "_sample"] = v.reshape(-1)[::53].copy()
    out["after_6_full"] = taps["after_6"]
    out["head_to_tail_full"] = taps["head_to_tail"]
    save("backbone_small", "placeholders", **out)

    # --- RPN head + train-mode losses (B=2)
    rp = syn.rpn_params(10)
    rpn = _load(_RPN(1024), rp, "RCNN_rpn.")
    rpn.train()
    rng = np.random.default_rng(700)
    feat = torch.from_numpy(np.abs(rng.standard_normal((2, 1024, 38, 63), dtype=np.float32)))
    gt, nb = syn.gt_boxes(701, 2, 8)
    info = torch.tensor([[600, 1000, 1.0]] * 2)
    cfg.TRAIN.RPN_POST_NMS_TOP_N = 2000
    np.random.seed(3)
    rois, lc, lb = rpn(feat, info, torch.from_numpy(gt), torch.from_numpy(nb))
    save("rpn_train", "placeholders", rois=rois.numpy(), loss_cls=lc.detach().numpy(),
         loss_box=lb.detach().numpy())

    # --- smooth L1
    rng = np.random.default_rng(710)
    a, b = (torch.from_numpy(rng.standard_normal((64, 4), dtype=np.float32)) for _ in range(2))
    iw = torch.from_numpy((rng.random((64, 4)) > 0.5).astype(np.float32))
    save("smooth_l1", "placeholders",
         s1=_smooth_l1_loss(a, b, iw, iw).numpy(),
         s3=_smooth_l1_loss(a.view(2, 8, 4, 4), b.view(2, 8, 4, 4), iw.view(2, 8, 4, 4), iw.view(2, 8, 4, 4) * 0.01,
                            sigma=3, dim=[1, 2, 3]).numpy())


def gen_full_frame(cfg):
    """the reference ResNet on FULL 600x1000 frames, pinned by shape + sums + a strided sample
    (the real 150x250 / 75x125 / 38x63 tile-padding paths of the implicit-GEMM and Winograd kernels).
    res101 on the two bench frames (configs[1]); res50 on one frame (configs[0], cfgs/res50.yml plumbing)."""
    import model.faster_rcnn.resnet_instance_styleD_bilinear as R
    names = {"RCNN_base.0": "conv1", "RCNN_base.1": "bn1", "RCNN_base.4": "layer1", "RCNN_base.5": "layer2",
             "RCNN_base.6": "layer3", "RCNN_top.0": "layer4"}
    out = {}
    for layers, ctor, nfr, seed in ((101, R.resnet101, 2, 1), (50, R.resnet50, 1, 0)):
        bp = syn.backbone_params(0, layers)
        net = ctor()
        sd = {}
        for k, v in bp.items():
            for a, b in names.items():
                if k.startswith(a + "."):
                    sd[b + k[len(a):]] = v
        miss = net.load_state_dict(sd, strict=False)
        assert not miss.unexpected_keys
        assert all(("fc." in k) or ("num_batches" in k) for k in miss.missing_keys), miss.missing_keys
        net.eval()
        im, _ = syn.frames(seed, nfr, 600, 1000)
        with torch.no_grad():
            x = net.maxpool(net.relu(net.bn1(net.conv1(torch.from_numpy(im)))))
            f1 = net.layer2(net.layer1(x))          # base_feat1: the style tap (resnet_instance...:412-420)
            f = net.layer3(f1)                      # base_feat
        for key, v in (("feat1", f1.numpy()), ("feat", f.numpy())):
            tag = "r%d_%s" % (layers, key)
            out[tag + "_shape"] = np.array(v.shape)
            out[tag + "_sum"] = np.array(v.astype(np.float64).sum())
            out[tag + "_abs"] = np.array(np.abs(v.astype(np.float64)).sum())
            out[tag + "_sample"] = v.reshape(-1)[::251].copy()
        print("   res%d: feat %s |sum| %.4e" % (layers, tuple(f.shape), float(out["r%d_feat_abs" % layers])))
    save("backbone_full_frame", "placeholders", **out)


def gen_context(cfg):
    """the reference ``_fasterRCNN`` (instance_styleD) with ic = gc = True run as shipped --
    context vectors of both discriminators concatenated in front of the layer4 feature
    (faster_rcnn_instance_styleD_bilinear.py:62-67,122-148) -- with the two pieces the reference cannot run here
    supplied by the harness: the RPN (fixed proposals, so that no near-tied score decides the sample) and RoIAlignAvg
    (legacy autograd.Function over an unbuildable extension -> the reference's compiled ROIAlignForwardCpu, oracle/build_ref.py).  Forward only, training mode."""
    import model.faster_rcnn.resnet_instance_styleD_bilinear as R
    n_cls = 16
    cfg.TRAIN.BATCH_SIZE = 32
    try:
        net = R.resnet(tuple(range(n_cls)), 50, pretrained=False, class_agnostic=False, ic=True, gc=True)
        net.create_architecture()
        p = {}
        p.update(syn.backbone_params(0, 50, top=True))
        p.update(syn.det_head_params(11, n_cls, feat_d=2048 + 512 + 128))
        p.update(syn.netd_params(12))
        miss = net.load_state_dict(p, strict=False)
        assert not miss.unexpected_keys, miss.unexpected_keys
        assert all(k.startswith("RCNN_rpn.") or "num_batches" in k for k in miss.missing_keys), miss.missing_keys
        im, info, gt, nb, rois = syn.context_inputs()

        class FixedRPN(torch.nn.Module):
            def forward(self, base_feat, im_info, gt_boxes, num_boxes, target=False):
                return torch.from_numpy(rois), torch.zeros(1), torch.zeros(1)

        class HarnessAlign(torch.nn.Module):
            def forward(self, feat, r):
                from oracle import build_ref          # the reference's own compiled forward (bit-equal to oracle.cops)
                x = torch.from_numpy(build_ref.roi_align_fwd(feat.detach().numpy(), r.detach().numpy(), 8, 8, 1.0 / 16.0))
                return torch.nn.functional.avg_pool2d(x, kernel_size=2, stride=1)

        net.RCNN_rpn = FixedRPN()
        net.RCNN_roi_align = HarnessAlign()
        net.train()
        np.random.seed(3)
        with torch.no_grad():
            out = net(torch.from_numpy(im), torch.from_numpy(info), torch.from_numpy(gt), torch.from_numpy(nb),
                      target=False, eta=0.1, eta_style=0.001)
        r, cls_prob, bbox_pred, _, _, l_cls, l_box, label, d_inst, d_sty = out
        save("context_ic_gc", "placeholders", rois=r.numpy(), labels=label.numpy(), cls_prob=cls_prob.numpy(),
             bbox_pred=bbox_pred.numpy(), loss_cls=l_cls.numpy(), loss_box=l_box.numpy(), d_instance=d_inst.numpy(),
             d_style=d_sty.numpy())
    finally:
        cfg.TRAIN.BATCH_SIZE = 128


def gen_step(cfg):
    """the reference ``_fasterRCNN`` (instance_styleD, ic = gc = False) run as shipped for ONE D+G step's
    forward passes -- source (faster_rcnn_instance_styleD_bilinear.py:47-182, target=False) then target (target=True) -- and
    the eight scalars the loop assembles from them (trainval_net_instance_styleD_bilinear.py:276-296).  Its own backbone, own
    ``_RPN`` (proposal layer with ``nms_cpu``, anchor targets), own ``_ProposalTargetLayer`` under ``np.random.seed(3)``, own
    discriminators and heads.  The one piece it cannot run here is ``RoIAlignFunction`` (a torch-0.4 legacy Function over an
    extension that needs TH); the harness's ``RCNN_roi_align`` does what ``RoIAlignAvg.forward`` does
    (roi_align/modules/roi_align.py:26-29) with the reference's own compiled ``ROIAlignForwardCpu`` (oracle/build_ref.py)
    in the Function's place: align to 8x8, ``avg_pool2d(x, kernel_size=2, stride=1)``.  Forward only, training mode.
    Two cases: res101 on 2+2 frames of 320x480, and res101 on 1+1 full 600x1000 frames; 32 ROIs per frame (configs[2])."""
    import model.faster_rcnn.resnet_instance_styleD_bilinear as R
    from oracle import build_ref
    build_ref.build()
    n_cls = 16

    class RefAlignAvg(torch.nn.Module):
        def forward(self, features, rois):
            x = torch.from_numpy(build_ref.roi_align_fwd(features.detach().numpy(), rois.detach().numpy(), 7 + 1, 7 + 1, 1.0 / 16.0))
            return torch.nn.functional.avg_pool2d(x, kernel_size=2, stride=1)

    cfg.TRAIN.BATCH_SIZE = 32
    cfg.TRAIN.RPN_POST_NMS_TOP_N_TARGET = 32
    cfg.TRAIN.RPN_POST_NMS_TOP_N = 2000
    out = {}
    try:
        for tag, B, H, W in (("small", 2, 320, 480), ("full", 1, 600, 1000)):
            net = R.resnet(tuple(range(n_cls)), 101, pretrained=False, class_agnostic=False)
            net.create_architecture()
            p = syn.instance_styled_step_params()
            miss = net.load_state_dict(p, strict=False)
            assert not miss.unexpected_keys, miss.unexpected_keys
            assert all("num_batches" in k for k in miss.missing_keys), miss.missing_keys
            net.RCNN_roi_align = RefAlignAvg()
            net.train()
            im, info, gt, nb, im_t, info_t = syn.instance_styled_step_inputs(B, H, W, n_cls)
            stash = []
            net.RCNN_rpn.register_forward_hook(lambda m, i, o: stash.append(o[0].detach().numpy().copy()))
            np.random.seed(3)
            with torch.no_grad():
                (rois, cls_prob, bbox_pred, rpn_loss_cls, rpn_loss_box, RCNN_loss_cls, RCNN_loss_bbox, rois_label, d_inst,
                 d_sty) = net(torch.from_numpy(im), torch.from_numpy(info), torch.from_numpy(gt), torch.from_numpy(nb),
                              target=False, eta=0.1, eta_style=0.001)
                d_inst_t, d_sty_t = net(torch.from_numpy(im_t), torch.from_numpy(info_t), torch.zeros(B, 1, 5), torch.zeros(B),
                                        target=True, eta=0.1, eta_style=0.001)
            losses = np.array([rpn_loss_cls.mean(), rpn_loss_box.mean(), RCNN_loss_cls.mean(), RCNN_loss_bbox.mean(),
                               0.5 * torch.mean(d_inst ** 2), 0.5 * torch.mean(d_sty ** 2),
                               0.5 * torch.mean((1 - d_inst_t) ** 2), 0.5 * torch.mean((1 - d_sty_t) ** 2)], np.float64)
            print("   %s: " % tag + " ".join("%.6f" % v for v in losses))
            out.update({tag + "_losses": losses, tag + "_rpn_rois_src": stash[0], tag + "_rpn_rois_tgt": stash[1],
                        tag + "_rois": rois.numpy(), tag + "_labels": rois_label.numpy(), tag + "_cls_prob": cls_prob.numpy(),
                        tag + "_bbox_pred": bbox_pred.numpy(), tag + "_d_instance": d_inst.numpy(), tag + "_d_style": d_sty.numpy(),
                        tag + "_d_instance_t": d_inst_t.numpy(), tag + "_d_style_t": d_sty_t.numpy()})
        out["loss_names"] = np.array(["rpn_loss_cls", "rpn_loss_box", "RCNN_loss_cls", "RCNN_loss_bbox", "dloss_s_p",
                                      "dloss_s_style", "dloss_t_p", "dloss_t_style"])
        save("instance_styled_step", "placeholders+extracted", **out)
    finally:
        cfg.TRAIN.BATCH_SIZE = 128
        cfg.TRAIN.RPN_POST_NMS_TOP_N_TARGET = 128


def gen_vrd(cfg):
    """vrd.forward logits / BCE loss / grads with eval-mode dropout."""
    import pickle
    import tempfile
    C = types.ModuleType("model._C")

    def roi_pool_forward(inp, rois, scale, ph, pw):
        out, arg = cops.roi_pool_fwd(inp.detach().numpy(), rois.detach().numpy(), ph, pw, scale)
        return torch.from_numpy(out), torch.from_numpy(arg)
    C.roi_pool_forward = roi_pool_forward
    C.nms = None            # bound at import by roi_layers/nms.py:5, never called on this path
    import model
    model._C = C
    sys.modules["model._C"] = C
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    # faster_rcnn_SGG_emb.py imports at module level things this path never calls
    import model.faster_rcnn.resnet_SGG_emb as S
    import torch.nn.functional as F

    n_rel, n_cls = 62, 16
    tmp = tempfile.mkdtemp()
    paths = {}
    for k in ("so_prior", "gt_s", "gt_t"):
        paths[k] = os.path.join(tmp, k + ".pkl")
        with open(paths[k], "wb") as f:
            pickle.dump({} if k != "so_prior" else [[0.0]], f)
    args = argparse.Namespace(num_relations=n_rel, num_classes=n_cls, emb_dim=300, use_obj_visual=True,
                              spatial_type=2, source_so_prior_path=paths["so_prior"],
                              source_gt_rels_path=paths["gt_s"], target_gt_rels_path=paths["gt_t"])
    prd = syn.word_vectors(21, n_rel)
    obj = syn.word_vectors(22, n_cls)
    head = S.vrd(args, obj, prd)
    p = syn.vrd_params(13)
    _load(head, p, "vrd.")
    head.eval()            # dropout off; eval also applies the softmax -> undo by calling in train w/o dropout
    head.training = True
    F_dropout = F.dropout
    S.F.dropout = lambda x, training=True: x
    try:
        from oracle import nets
        anno = syn.relation_annotation(31, 8, 8, n_rel, n_cls)
        ih, iw = 600.0, 1000.0
        boxes, rel_boxes, spatial, labels, ixs, ixo = nets.build_pairs(anno["boxes"], anno["rels"], 1.0, ih, iw, n_rel)
        rng = np.random.default_rng(32)
        fmap = np.abs(rng.standard_normal((1, 1024, 38, 63), dtype=np.float32))
        # pair builder pinned against the reference's own helper methods
        ub = np.array([head._getUnionBBox(np.array(anno["boxes"][s]), np.array(anno["boxes"][o]), ih, iw)
                       for s, o in zip(ixs, ixo)])
        dm = np.array([head._getDualMask(ih, iw, np.array(anno["boxes"][s])) for s in ixs])
        classes = np.array(anno["box_classes"]).astype(np.float32)
        score, feat = head(fmap, boxes, rel_boxes, spatial, classes, ixs, ixo)
        loss = head.criterion(score, torch.from_numpy(labels).float())
        loss.backward()
        save("vrd_head", "placeholders", union_boxes=ub, dual_masks=dm, scores=score.detach().numpy(),
             rel_feat=feat, loss=loss.detach().numpy(),
             g_fc6_w=head.fc6.fc.weight.grad.numpy()[:4, ::97].copy(),
             g_fc6_b=head.fc6.fc.bias.grad.numpy(), g_fc7_b=head.fc7.fc.bias.grad.numpy(),
             g_fc_rel_w=head.fc_rel.fc.weight.grad.numpy(),
             g_conv0_w=head.conv_lo[0].conv.weight.grad.numpy(),
             g_sem0_b=head.prd_sem_embeddings[0].bias.grad.numpy(),
             g_fc6_w_sum=np.array(head.fc6.fc.weight.grad.numpy().astype(np.float64).sum()),
             g_fc6_w_abs=np.array(np.abs(head.fc6.fc.weight.grad.numpy().astype(np.float64)).sum()))
        # the variants of resnet_SGG_emb.py:94-123 / :166-180 (the reference's scripts only ever run the defaults: its
        # type=bool flags parse every CLI value to True -- but the class implements them, so they are pinned too)
        out = {}
        for tag, (ov, st) in {"nov_s1": (False, 1), "ov_s1": (True, 1), "nov_s2": (False, 2), "ov_s0": (True, 0)}.items():
            a2 = argparse.Namespace(**dict(vars(args), use_obj_visual=ov, spatial_type=st))
            h2 = S.vrd(a2, obj, prd)
            _load(h2, syn.vrd_params(13, use_obj_visual=ov, spatial_type=st), "vrd.")
            h2.eval()
            h2.training = True
            if st == 1:
                sp = np.array([h2._getRelativeLoc(np.array(anno["boxes"][s_]), np.array(anno["boxes"][o_])) for s_, o_ in zip(ixs, ixo)])
                out[tag + "_spatial"] = sp
            else:
                sp = spatial
            sc2, ft2 = h2(fmap, boxes, rel_boxes, sp, classes, ixs, ixo)
            l2 = h2.criterion(sc2, torch.from_numpy(labels).float())
            l2.backward()
            out[tag + "_scores"], out[tag + "_rel_feat"], out[tag + "_loss"] = sc2.detach().numpy(), ft2, l2.detach().numpy()
            out[tag + "_g_fusion_w"] = h2.fc_fusion.fc.weight.grad.numpy()[::16].copy()
            out[tag + "_g_fc7_b"] = h2.fc7.fc.bias.grad.numpy()
            if st in (1, 2):
                out[tag + "_g_lov_w"] = h2.fc_lov.fc.weight.grad.numpy()[::4].copy()
            print("    vrd variant %-7s use_obj_visual=%s spatial_type=%d: loss %.6f, fc_fusion %s" % (
                tag, ov, st, float(l2), tuple(h2.fc_fusion.fc.weight.shape)))
        save("vrd_head_variants", "placeholders", **out)
    finally:
        S.F.dropout = F_dropout


# ----------------------------------------------------------------------------- video association / evaluation
def _utils_functions(names):
    """Functions (and the VideoRelation class) of lib/utils.py compiled from their own lines: the module cannot be imported
    (a module-level json.load of an absolute path).  ``objects_list`` / ``predicates_list`` are plain id lists, so that
    serialize() keeps ids; ``print`` is silenced."""
    import ast
    import collections
    path = os.path.join(REF, "lib", "utils.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names)
    ns = {"np": np, "json": __import__("json"), "defaultdict": collections.defaultdict, "print": lambda *a, **k: None,
          "objects_list": list(range(64)), "predicates_list": list(range(200))}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def gen_video():
    """tests/golden/video_association.npz and video_eval.npz: the reference's association() and evaluate() on the videos of
    i2vsgg_amd.synthetic.video_fixture_cases().  The inputs are regenerated from seeds; the files hold the reference's
    results (relations as triplet, score, duration and, per member, which input prediction its boxes are), the frames
    after its fill of empty ones, and the smallest margin of the decisions that rest on computed doubles."""
    import copy
    import json
    import tempfile
    import time
    from i2vsgg_amd import video
    MARGIN = 1e-9
    ns = _utils_functions(["_iou", "VideoRelation", "greedy_relational_association", "voc_ap", "viou", "eval_detection_scores",
                           "eval_tagging_scores", "evaluate", "association"])
    cases = syn.video_fixture_cases()
    iou_margin = [np.inf]
    ref_iou = ns["_iou"]

    def iou_logged(a, b):                                # every IoU the reference computes, against its threshold
        v = ref_iou(a, b)
        iou_margin[0] = min(iou_margin[0], abs(v - 0.5) / 0.5)
        return v
    ns["_iou"] = iou_logged
    out = {"vids": np.array(list(cases))}
    frame_off, filled_src, rel_off, trip, score, dur, mem_off, mem_frame, mem_pred = [0], [], [0], [], [], [], [0], [], []
    margins = {"iou": np.inf, "mean": np.inf, "score": np.inf}
    facts = {"kept_max": 0, "len9": 0, "len10": 0, "contested": 0, "multi_candidate": 0, "ties_mean": 0, "score_ties_in_frame": 0,
             "over_100": 0, "stays_empty": 0, "filled": 0, "gap": 0}
    predictions = {}
    for vid, frames in cases.items():
        # the package's host form on the same input: the margins of the mean / score comparisons (its sums run in member
        # order, the reference's np.mean pairwise: decisions closer than MARGIN could differ and may not enter the file)
        st = {"exact_sums": all(p[0] * 64 == int(p[0] * 64) for f in frames for p in f[1])}
        pk = video.pack_frames(copy.deepcopy({vid: frames}))
        res = video.associate_arrays_host(pk, st)
        for k in margins:
            margins[k] = min(margins[k], st.get(k, np.inf))
        lens = res[2][:int(res[4][0])]
        facts["kept_max"] = max(facts["kept_max"], int((lens >= 10).sum()))
        facts["len9"] += int((lens == 9).sum())
        facts["len10"] += int((lens == 10).sum())
        for k in ("contested", "multi_candidate", "ties_mean"):
            facts[k] += st.get(k, 0)
        facts["over_100"] += sum(len(f[1]) > 100 for f in frames)
        facts["score_ties_in_frame"] += sum(len(set(p[0] for p in f[1])) < len(f[1]) for f in frames)
        nos = sorted(int(f[0]) for f in frames)
        facts["gap"] += sum(b - a > 1 for a, b in zip(nos, nos[1:]))
        # the reference, on lists of its own
        mine = copy.deepcopy(frames)
        mine.sort(key=lambda x: int(x[0]))
        where, lists = {}, {}
        for i, f in enumerate(mine):
            lists[id(f[1])] = i
            for j, p in enumerate(f[1]):
                where[id(p[2][0])] = (i, j, 0)
                where[id(p[2][1])] = (i, j, 1)
        was_empty = [len(f[1]) == 0 for f in mine]
        t0 = time.time()
        rels = ns["association"]({vid: mine})[vid]
        print("    association %-6s %3d frames -> %3d relations (%.1f s)" % (vid, len(mine), len(rels), time.time() - t0))
        for i, f in enumerate(mine):                     # association() fills its argument in place
            src = lists[id(f[1])]
            filled_src.append(src if len(f[1]) else -1)
            facts["stays_empty"] += len(f[1]) == 0
            facts["filled"] += was_empty[i] and len(f[1]) > 0
        frame_off.append(len(filled_src))
        for r in rels:
            trip.append(r["triplet"])
            score.append(r["score"])
            dur.append(r["duration"])
            for s, o in zip(r["sub_traj"], r["obj_traj"]):
                ws, wo = where[id(s)], where[id(o)]
                assert ws[:2] == wo[:2] and ws[2] == 0 and wo[2] == 1
                mem_frame.append(ws[0])
                mem_pred.append(ws[1])
            mem_off.append(len(mem_frame))
        rel_off.append(len(trip))
        predictions[vid] = rels
    margins["iou"] = min(margins["iou"], iou_margin[0])
    print("    margins", margins, "facts", facts)
    assert min(margins.values()) >= MARGIN, "a decision within %g of its threshold: choose another seed" % MARGIN
    assert facts["kept_max"] > 200 and facts["len9"] and facts["len10"] and facts["contested"] and facts["multi_candidate"]
    assert facts["ties_mean"] and facts["score_ties_in_frame"] and facts["over_100"] and facts["stays_empty"] and facts["filled"]
    assert facts["gap"]
    moved = [r for r in predictions["moved"] if r["triplet"] == [3, 60, 4]]
    assert sorted(r["duration"] for r in moved) == [[0, 25], [25, 60]]       # the object moved away, the subject stayed
    save("video_association", "extracted", frame_off=np.asarray(frame_off, np.int32), filled_src=np.asarray(filled_src, np.int32),
         rel_off=np.asarray(rel_off, np.int32), triplet=np.asarray(trip, np.int32), score=np.asarray(score, np.float64),
         duration=np.asarray(dur, np.int32), mem_off=np.asarray(mem_off, np.int32), mem_frame=np.asarray(mem_frame, np.int16),
         mem_pred=np.asarray(mem_pred, np.int16), margin_iou=np.float64(margins["iou"]), margin_mean=np.float64(margins["mean"]),
         margin_score=np.float64(margins["score"]), **out)

    # ---- evaluation: the reference's predictions against ground truth made from them; one video has none
    gts = dict((vid, syn.video_groundtruth(predictions[vid], 300 + k)) for k, vid in enumerate(predictions))
    gts["v07"] = []
    thr = 0.5
    st = {}
    pe, ov_h, hit_h, _ = video.match(predictions, gts, thr, stats=st)
    assert min(st.get("ov", 1), st.get("ov_gap", 1)) >= MARGIN, st
    ov_ref = np.full(ov_h.shape, np.nan)
    tp_ref = np.zeros(len(hit_h), bool)
    ref_viou = ns["viou"]
    calls = []
    ns["viou"] = lambda t1, d1, t2, d2: calls.append((id(t1), id(t2), ref_viou(t1, d1, t2, d2))) or calls[-1][2]
    lens = []
    for v, vid in enumerate(pe.vids):
        preds, g = predictions[vid], gts[vid]
        pid = dict((id(r[key]), (k, c)) for k, r in enumerate(preds) for c, key in enumerate(("sub_traj", "obj_traj")))
        gid = dict((id(r[key]), (k, c)) for k, r in enumerate(g) for c, key in enumerate(("sub_traj", "obj_traj")))
        del calls[:]
        _, _, hit_scores = ns["eval_detection_scores"](g, preds, thr)
        order = np.argsort(-np.array([r["score"] for r in preds]), kind="stable")
        p0 = int(pe.pred_off[v])
        tp_ref[p0 + order] = np.isfinite(hit_scores)
        for (a, b, val), (a2, b2, val2) in zip(calls[0::2], calls[1::2]):
            assert pid[a][0] == pid[a2][0] and gid[b][0] == gid[b2][0] and pid[a][1] == 0 and pid[a2][1] == 1
            ov_ref[p0 + pid[a][0], gid[b][0]] = min(val, val2)
        lens += [len(r["sub_traj"]) for r in preds]
    # the reference computes an overlap exactly for the ground truths of equal triplet that are not yet detected; with the
    # package's hit list the same cells must be the computed ones, and the same predictions the true positives
    assert ((hit_h >= 0) == tp_ref).all()
    seen = ~np.isnan(ov_ref)
    assert np.allclose(ov_ref[seen], ov_h[seen], rtol=1e-12, atol=0)
    for v in range(len(pe.vids)):
        p0, p1 = int(pe.pred_off[v]), int(pe.pred_off[v + 1])
        taken = set()
        for p in p0 + np.argsort(-pe.pred_score[p0:p1], kind="stable"):
            want = set(g for g in np.nonzero(ov_h[p] >= 0)[0] if g not in taken)
            assert want == set(np.nonzero(seen[p])[0]), (v, p)
            if hit_h[p] >= 0:
                taken.add(int(hit_h[p]))
    n_over = np.array([(ov_h[:, g] >= thr).sum() for g in range(ov_h.shape[1])])
    assert (hit_h < 0).any() and (ov_h.max(1) < 0).any() and min(lens) == 10 and max(lens) >= 500
    both = [(ov_h[int(pe.pred_off[v]):int(pe.pred_off[v + 1])] >= thr).sum(0).max() for v in range(len(pe.vids))]
    assert max(both) >= 2                                # two predictions over one ground truth
    assert ((ov_h > 0) & (ov_h < thr)).any()             # a partial overlap
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(gts, f)
    try:
        mean_ap, rec, mprec = ns["evaluate"](predictions, f.name, thr)
    finally:
        os.unlink(f.name)
    print("    evaluate: mAP %.6f  R@50 %.6f  R@100 %.6f  P@1 %.6f  P@5 %.6f  P@10 %.6f" % (
        mean_ap, rec[50], rec[100], mprec[1], mprec[5], mprec[10]))
    save("video_eval", "extracted", vids=np.array(pe.vids), pred_off=pe.pred_off, hit=hit_h.astype(np.int32), ov=ov_ref,
         metrics=np.array([mean_ap, rec[50], rec[100], mprec[1], mprec[5], mprec[10]], np.float64), viou_threshold=np.float64(thr),
         gt_seed_base=np.int32(300), no_gt=np.array(["v07"]), margin_ov=np.float64(st.get("ov", np.inf)),
         margin_ov_gap=np.float64(st.get("ov_gap", np.inf)))


def gen_video_edges():
    """tests/golden/video_eval_edges.npz: the reference's eval_detection_scores / viou / evaluate on
    tests/video_golden.py eval_edge_set(EDGE_SEED, grid=True, clamped=False) -- more than 64 and 128 ground truths, duplicate
    annotations, tied scores, overlaps exactly on the threshold -- at thresholds 0.5 and 0.0.  Per threshold: which
    predictions (packed order) are true positives, the overlaps the reference computed (flat cell index into the
    (n_pred, max_gt) table, value) and the six metrics.  The reference raises on a trajectory shorter than its duration,
    so the ``clamped`` video stays out."""
    import json
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import video_golden as vg
    from i2vsgg_amd import video
    ns = _utils_functions(["voc_ap", "viou", "eval_detection_scores", "eval_tagging_scores", "evaluate"])
    predictions, gts = vg.eval_edge_set(vg.EDGE_SEED, grid=True, clamped=False)
    ref_viou = ns["viou"]
    calls = []
    ns["viou"] = lambda t1, d1, t2, d2: calls.append((id(t1), id(t2), ref_viou(t1, d1, t2, d2))) or calls[-1][2]
    out = {}
    for tag, thr in (("50", 0.5), ("00", 0.0)):
        pe, ov_h, hit_h, _ = video.match(predictions, gts, thr)
        tp_ref = np.zeros(len(hit_h), bool)
        cell, val = [], []
        for v, vid in enumerate(pe.vids):
            preds, g = predictions.get(vid, []), gts[vid]
            pid = dict((id(r[key]), (k, c)) for k, r in enumerate(preds) for c, key in enumerate(("sub_traj", "obj_traj")))
            gid = dict((id(r[key]), (k, c)) for k, r in enumerate(g) for c, key in enumerate(("sub_traj", "obj_traj")))
            del calls[:]
            _, _, hit_scores = ns["eval_detection_scores"](g, preds, thr)
            order = np.argsort(-np.array([r["score"] for r in preds]), kind="stable")
            p0 = int(pe.pred_off[v])
            tp_ref[p0 + order] = np.isfinite(hit_scores)
            for (a, b, x), (a2, b2, x2) in zip(calls[0::2], calls[1::2]):
                assert pid[a][0] == pid[a2][0] and gid[b][0] == gid[b2][0] and pid[a][1] == 0 and pid[a2][1] == 1
                cell.append((p0 + pid[a][0]) * ov_h.shape[1] + gid[b][0])
                val.append(min(x, x2))
        cell, val = np.asarray(cell, np.int32), np.asarray(val, np.float64)
        # the package's host form must already agree: equal true positives, and on this grid equal bits
        assert ((hit_h >= 0) == tp_ref).all()
        assert (ov_h.reshape(-1)[cell] == val).all()
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump(gts, f)
        try:
            mean_ap, rec, mprec = ns["evaluate"](predictions, f.name, thr)
        finally:
            os.unlink(f.name)
        print("    threshold %.1f: %d of %d true positives, %d overlaps; mAP %.6f  R@50 %.6f  R@100 %.6f  P@1 %.6f  P@5 %.6f  P@10 %.6f"
              % (thr, tp_ref.sum(), len(tp_ref), len(cell), mean_ap, rec[50], rec[100], mprec[1], mprec[5], mprec[10]))
        out["tp_" + tag], out["ov_cell_" + tag], out["ov_" + tag] = tp_ref, cell, val
        out["metrics_" + tag] = np.array([mean_ap, rec[50], rec[100], mprec[1], mprec[5], mprec[10]], np.float64)
    assert out["tp_00"].sum() > out["tp_50"].sum() and (out["ov_00"] == 0.0).any() and (out["ov_50"] == 0.5).any()
    save("video_eval_edges", "extracted", seed=np.int32(vg.EDGE_SEED), vids=np.array(pe.vids), pred_off=pe.pred_off,
         max_gt=np.int32(ov_h.shape[1]), thresholds=np.array([0.5, 0.0]), **out)


# ----------------------------------------------------------------------------- detection evaluation (VOC AP)
def det_eval_fixture_inputs(seed=4100, n_images=240, n_classes=9):
    """The seeded detections and annotations of tests/golden/det_eval.npz: (all_boxes, roidb, classes).  Ground-truth boxes
    are integers (the XML holds integers); detection coordinates lie on a quarter-pixel grid (halves of the '%.1f' included)
    and the quantised scores of a class are pairwise distinct.  Class ``n_classes - 2`` has no detections, class
    ``n_classes - 1`` detections but no ground truth."""
    rng = np.random.default_rng(seed)
    classes = tuple(["__background__"] + ["kind%d" % c for c in range(1, n_classes)])
    no_det, no_gt = n_classes - 2, n_classes - 1
    gts = [[] for _ in range(n_images)]                  # rows x1 y1 x2 y2 cls hard
    dets = [[[] for _ in range(n_images)] for _ in range(n_classes)]      # rows x1 y1 x2 y2 (score comes later)

    def rand_box(lo=24, hi=200):
        w, h = rng.integers(lo, hi, 2)
        x, y = rng.integers(0, 700 - w), rng.integers(300, 900 - h)
        return [int(x), int(y), int(x + w), int(y + h)]

    for i in range(8, n_images):                         # the generic part (images 0-7 hold the constructions)
        for _ in range(int(rng.integers(0, 9))):
            c = int(rng.integers(1, no_gt))              # classes 1 .. no_det have ground truth
            b = rand_box()
            gts[i].append(b + [c, int(rng.random() < 0.15)])
            if c == no_det:
                continue
            for _ in range(int(rng.choice([0, 1, 1, 1, 2, 3]))):          # detections near it; several: duplicates
                jit = rng.integers(-40, 41, 4) / 4.0 * (1.0 if rng.random() < 0.7 else 4.0)
                d = np.asarray(b, np.float64) + jit
                dets[c][i].append([min(d[0], d[2]), min(d[1], d[3]), max(d[0], d[2]), max(d[1], d[3])])
        for _ in range(int(rng.integers(0, 4))):         # detections of anything anywhere
            c = int(rng.choice([k for k in range(1, n_classes) if k != no_det]))
            b = np.asarray(rand_box(), np.float64) + rng.integers(0, 4, 4) / 4.0
            dets[c][i].append(b.tolist())
    # image 0, class 1: a duplicate of a claimed ground truth; best claimed while the second best is free
    gts[0] += [[10, 10, 60, 60, 1, 0], [14, 10, 64, 60, 1, 0]]
    dets[1][0] += [[10, 10, 60, 60], [11, 10, 61, 60], [10.25, 10.5, 60, 59.75]]
    # image 0, class 2: two identical ground truths (the first wins), then a second detection that finds the first claimed
    gts[0] += [[100, 100, 150, 150, 2, 0], [100, 100, 150, 150, 2, 0]]
    dets[2][0] += [[100, 100, 150, 150], [100.5, 100, 150, 150.5]]
    # image 1, class 3: the best match is hard, and it is the best-scored detection of the class
    gts[1] += [[200, 200, 260, 260, 3, 1], [300, 200, 360, 260, 3, 0]]
    dets[3][1] += [[200, 200, 260, 260], [300.5, 200.5, 360, 260]]
    # image 2, class 4: an overlap of exactly 0.5 -- [1,1,10,10] against [1,1,10,5] in the file's coordinates
    gts[2] += [[0, 0, 9, 4, 4, 0]]
    dets[4][2] += [[0, 0, 9, 9]]
    # image 3, class 5: 80 ground truths in one image, detections on most of them
    for r in range(8):
        for q in range(10):
            b = [20 + 60 * q, 20 + 60 * r, 60 + 60 * q, 60 + 60 * r]
            gts[3].append(b + [5, int((r * 10 + q) % 17 == 5)])
            if (r * 10 + q) % 5 != 2:
                dets[5][3].append((np.asarray(b, np.float64) + rng.integers(-12, 13, 4) / 4.0).tolist())
    dets[5][3].append([20 + 60 * 7, 20 + 60 * 6, 60 + 60 * 7, 60 + 60 * 6])       # index 67 > 63, exact
    # image 4: detections of class 1 in an image that has none of its ground truth
    gts[4] += [[50, 50, 120, 120, 2, 0]]
    dets[1][4] += [[50, 50, 120, 120], [300.75, 310.25, 400.5, 420]]
    # scores: distinct thousandths within a class, off the grid by less than half a step; the constructions' first
    # detections get the class's best scores in the order listed
    special = {1: [(0, 0), (0, 1), (0, 2)], 2: [(0, 0), (0, 1)], 3: [(1, 0), (1, 1)]}
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in range(n_classes)]
    for c in range(1, n_classes):
        where = [(i, k) for i in range(n_images) for k in range(len(dets[c][i]))]
        assert len(where) < 990, (c, len(where))
        first = [w for w in special.get(c, []) if w in where]
        rest = [w for w in where if w not in first]
        rest = [rest[j] for j in rng.permutation(len(rest))]
        keys = np.sort(rng.permutation(np.arange(1, 1000))[:len(where)])[::-1]
        score = {}
        for key, w in zip(keys, first + rest):
            score[w] = np.float32((key + rng.uniform(-0.4, 0.4)) / 1000.0)
        for i in range(n_images):
            if dets[c][i]:
                rows = [list(dets[c][i][k]) + [score[(i, k)]] for k in range(len(dets[c][i]))]
                all_boxes[c][i] = np.asarray(rows, np.float64).astype(np.float32)
    roidb = []
    for i in range(n_images):
        g = np.asarray(gts[i], np.int64).reshape(-1, 6)
        roidb.append({"boxes": g[:, :4].astype(np.uint16), "gt_classes": g[:, 4].astype(np.int32),
                      "gt_ishard": g[:, 5].astype(np.int32)})
    return all_boxes, roidb, classes


def _write_voc_files(tmp, all_boxes, roidb, classes):
    """What the reference's evaluation reads: the image-set file, one minimal XML per image (boxes + 1, difficult,
    truncated) and one results file per class in the writer's own line format (_write_voc_results_file).  Returns the
    image-set file; the results of class ``name`` are ``tmp/det_<name>.txt``, the annotations ``tmp/Annotations/<id>.xml``."""
    os.makedirs(os.path.join(tmp, "Annotations"))
    names = ["%06d" % i for i in range(len(roidb))]
    setfile = os.path.join(tmp, "test.txt")
    with open(setfile, "w") as f:
        f.write("".join(n + "\n" for n in names))
    for i, e in enumerate(roidb):
        objs = "".join("<object><name>%s</name><truncated>0</truncated><difficult>%d</difficult><bndbox><xmin>%d</xmin>"
                       "<ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                       % ((classes[cl], hard) + tuple(int(v) + 1 for v in bx))
                       for bx, cl, hard in zip(e["boxes"], e["gt_classes"], e["gt_ishard"]))
        with open(os.path.join(tmp, "Annotations", names[i] + ".xml"), "w") as f:
            f.write("<annotation>%s</annotation>" % objs)
    for c in range(1, len(classes)):
        with open(os.path.join(tmp, "det_%s.txt" % classes[c]), "wt") as f:
            for i in range(len(roidb)):
                d = all_boxes[c][i]
                for k in range(d.shape[0]):
                    f.write('{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}\n'.format(names[i], d[k, -1], d[k, 0] + 1, d[k, 1] + 1,
                                                                              d[k, 2] + 1, d[k, 3] + 1))
    return setfile


def _load_voc_eval():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_voc_eval", os.path.join(REF, "lib", "datasets", "voc_eval.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def time_det_eval(n_images=2400):
    """Orientation for profiles/r10_det_eval.txt: the reference's voc_eval on this machine's CPU on the seeded set of
    tests/det_eval_golden.py fresh_set (files written first, annotations parsed and cached before the clock starts)."""
    import contextlib
    import io
    import tempfile
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import det_eval_golden as dg
    ref = _load_voc_eval()
    all_boxes, roidb, classes = dg.fresh_set(n_images=n_images)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        setfile = _write_voc_files(tmp, all_boxes, roidb, classes)
        print("  reference writer format, %d images: files written in %.1f s" % (n_images, time.perf_counter() - t0))
        total, n_det = 0.0, 0
        for c in range(1, len(classes)):
            args = (os.path.join(tmp, "det_%s.txt" % classes[c]), os.path.join(tmp, "Annotations", "{:s}.xml"), setfile, classes[c],
                    os.path.join(tmp, "cache"))
            if c == 1:
                with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                    t0 = time.perf_counter()
                    ref.voc_eval(*args)                  # parses the XML and writes the cache
                    print_later = time.perf_counter() - t0
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                t0 = time.perf_counter()
                rec, prec, ap = ref.voc_eval(*args)
                dt = time.perf_counter() - t0
            total += dt
            n_det += len(rec)
            print("  voc_eval %-8s %7d detections %8.2f s   ap %.4f" % (classes[c], len(rec), dt, ap))
        print("  first call with the XML parse: %.1f s; voc_eval over all classes, annotations cached: %.1f s for %d detections "
              "(%.1f us per detection)" % (print_later, total, n_det, 1e6 * total / max(n_det, 1)))


def gen_det_eval():
    """tests/golden/det_eval.npz: the reference's own ``voc_eval`` (lib/datasets/voc_eval.py, loaded by path, unmodified) on
    seeded detections written in its results-file format and annotations written as minimal VOC XML, per class, both AP
    forms, at two overlap thresholds.  The file holds the inputs and rec / prec / ap."""
    import contextlib
    import io
    import tempfile
    from i2vsgg_amd import detection_eval as de
    ref = _load_voc_eval()
    all_boxes, roidb, classes = det_eval_fixture_inputs()
    C, I = len(classes) - 1, len(roidb)
    thresholds = (0.5, 0.7)
    # --- the conditions the fixture must meet
    pk = de.pack(all_boxes, roidb, len(classes))
    for k in range(C):
        keys = pk.det_key[pk.cls_off[k]:pk.cls_off[k + 1]]
        assert len(np.unique(keys)) == len(keys), "quantised scores of class %d tie" % (k + 1)
    for c in range(1, C + 1):
        for d in all_boxes[c]:
            if len(d):
                xy = d[:, :4].astype(np.float64)
                assert (xy * 4 == np.round(xy * 4)).all() and (np.abs(xy) < 2 ** 20).all()
                assert ((d[:, :4] + np.float32(1)).astype(np.float64) == xy + 1.0).all()
    flag, ovmax, jmax = de.match_arrays_host(pk, 0.5)
    n_per = np.diff(pk.cls_off)
    assert (n_per == 0).any() and ((n_per > 0) & (pk.npos == 0)).any()                   # no detections; detections, npos 0
    seg_ng = np.diff(pk.gt_off)[pk.seg_gt]
    assert (seg_ng == 0).any() and (seg_ng > 64).any()
    big = np.nonzero(seg_ng > 64)[0][0]
    assert (jmax[pk.seg_det_off[big]:pk.seg_det_off[big + 1]] > 63).any()
    assert (ovmax == 0.5).any() and (flag[ovmax == 0.5] == de.FP).all()
    have = dict(dup=False, second_free=False, twin=False, hard_first=False)
    for s in range(len(pk.seg_gt)):
        d0, d1 = pk.seg_det_off[s], pk.seg_det_off[s + 1]
        g0, g1 = pk.gt_off[pk.seg_gt[s]], pk.gt_off[pk.seg_gt[s] + 1]
        if g1 == g0:
            continue
        ov = de._overlaps(pk.det_box[d0:d1], pk.gt_box[g0:g1])
        claimed = set(jmax[d0:d1][flag[d0:d1] == de.TP].tolist())
        for q in range(d1 - d0):
            j = jmax[d0 + q]
            if flag[d0 + q] == de.FP and ovmax[d0 + q] > 0.5 and not pk.gt_hard[g0 + j]:
                have["dup"] = True
                free = [g for g in range(g1 - g0) if g != j and ov[q, g] > 0.5 and g not in claimed and not pk.gt_hard[g0 + g]]
                have["second_free"] |= bool(free)
            if (ov[q] == ov[q, j]).sum() > 1 and (pk.gt_box[g0:g1][ov[q] == ov[q, j]] == pk.gt_box[g0 + j]).all() and flag[d0 + q] == de.TP:
                have["twin"] = True
    for k in range(C):
        a, b = pk.cls_off[k], pk.cls_off[k + 1]
        if b > a and flag[a + np.argmax(pk.det_key[a:b])] == de.IGNORED:
            have["hard_first"] = True
    assert all(have.values()), have
    assert (flag == de.IGNORED).sum() > 1
    # --- the reference's files and its own evaluation
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        setfile = _write_voc_files(tmp, all_boxes, roidb, classes)
        for ti, thr in enumerate(thresholds):
            recs, precs = [], []
            ap = np.zeros((2, C), np.float64)
            for c in range(1, C + 1):
                for m, use07 in enumerate((False, True)):
                    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                        rec, prec, a = ref.voc_eval(os.path.join(tmp, "det_%s.txt" % classes[c]),
                                                    os.path.join(tmp, "Annotations", "{:s}.xml"), setfile, classes[c],
                                                    os.path.join(tmp, "cache"), ovthresh=thr, use_07_metric=use07)
                    ap[m, c - 1] = a
                recs.append(np.asarray(rec, np.float64))
                precs.append(np.asarray(prec, np.float64))
                assert len(rec) == n_per[c - 1]
            out["rec_%d" % ti], out["prec_%d" % ti] = np.concatenate(recs), np.concatenate(precs)
            out["ap_area_%d" % ti], out["ap_11pt_%d" % ti] = ap[0], ap[1]
            print("    ovthresh %.1f  ap %s" % (thr, np.array2string(ap[0], precision=4)))
    det = np.concatenate([d for c in range(1, C + 1) for d in all_boxes[c] if len(d)]).astype(np.float32)
    det_cls = np.concatenate([np.full(len(d), c, np.int32) for c in range(1, C + 1) for d in all_boxes[c] if len(d)])
    det_img = np.concatenate([np.full(len(d), i, np.int32) for c in range(1, C + 1) for i, d in enumerate(all_boxes[c]) if len(d)])
    gt_img = np.concatenate([np.full(len(e["boxes"]), i, np.int32) for i, e in enumerate(roidb)])
    save("det_eval", "direct", thresholds=np.asarray(thresholds, np.float64), classes=np.array(classes), n_images=np.int32(I),
         det=det, det_cls=det_cls, det_img=det_img, gt_img=gt_img,
         gt_box=np.concatenate([e["boxes"] for e in roidb]).astype(np.int32),
         gt_cls=np.concatenate([e["gt_classes"] for e in roidb]).astype(np.int32),
         gt_hard=np.concatenate([e["gt_ishard"] for e in roidb]).astype(np.int32), npos=pk.npos, **out)


# ----------------------------------------------------------------------------- predicate recognition
def gen_recognition():
    """tests/golden/recognition.npz: the reference's recognition_output (lib/utils.py:570-582) on one seeded frame record and
    its evaluate_recognition (:335-372) on ``recognition.video_recognitions`` of the seeded case set of
    tests/recognition_cases.py (the reference's alignment, which was to produce those records, is commented out).  The file
    holds data only: the four outputs, the seven returned numbers and the per-class values parsed from the printed lines."""
    import copy
    import re
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import recognition_cases as cases
    from i2vsgg_amd import recognition
    ns = _utils_functions(["recognition_output", "evaluate_recognition"])
    rec = cases.frame_record()
    data = copy.deepcopy(rec)
    data["rel_scores"] = torch.from_numpy(data["rel_scores"])
    sub, obj, pre, tids = ns["recognition_output"](data)
    cs = cases.golden_set()
    assert cs["redraws"] == 0, cs["redraws"]
    pk = recognition.pack(cs["frame_recognitions"], cs["groundtruth"], cs["classes"], cs["predicates"])
    mean = recognition.align_arrays_host(pk)[0]
    lines = []
    ns["print"] = lambda *a, **k: lines.append(" ".join(str(x) for x in a))
    acc = ns["evaluate_recognition"](recognition.video_recognitions(pk, mean))
    per_class = np.full((2, 16), np.nan)
    for line in lines:
        m = re.match(r"object #(\d+) acc@(\d+) : (.*)$", line)
        if m:
            per_class[(1, 5).index(int(m.group(2))), int(m.group(1))] = float(m.group(3))
    seven = np.array([acc["sub"][1], acc["sub"][5], acc["obj"][1], acc["obj"][5], acc["pre"][1], acc["pre"][5], acc["rel"][1]],
                     np.float64)
    print("  recognition: %d segments, %d instances, %d aligned; sub@1 %.4f obj@1 %.4f pre@1 %.4f pre@5 %.4f rel@1 %.4f" % (
        len(pk.segments), len(pk.inst), sum(len(v) for v in recognition.video_recognitions(pk, mean).values()), *seven[[0, 2, 4, 5, 6]]))
    save("recognition", "extracted", sub_scores=sub, obj_scores=obj, pre_scores=pre, tids=np.asarray(tids, np.int64), metrics=seven,
         per_class=per_class, n_segments=np.array(len(pk.segments)), n_instances=np.array(len(pk.inst)))


# ----------------------------------------------------------------------------- video relation features
def gen_video_relation_feat():
    """tests/golden/video_relation_feat.npz: the reference's generate_static_relation_feat (lib/utils.py:100-132) run in a temp
    dir on the seeded inputs of tests/relation_feature_cases.golden_inputs().  The file holds data only, per case ``c<i>_``: the
    frame features in loader order with their slot table (video index, frame number, row offsets), the relations (video index,
    pno, duration, predicate name, rel_idex) and the contents of the .npy files the reference wrote."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import relation_feature_cases as cases
    ns = _utils_functions(["generate_static_relation_feat"])
    ns["os"] = os
    out = {}
    for c, case in enumerate(cases.golden_inputs()):
        vids = list(case["relations"])
        with tempfile.TemporaryDirectory() as tmp:
            feat_dir, save_dir = os.path.join(tmp, "feat"), os.path.join(tmp, "video")
            for vid, fno, rows in case["slots"]:
                os.makedirs(os.path.join(feat_dir, vid), exist_ok=True)
                np.savez(os.path.join(feat_dir, vid, str(fno)), pre_feat=rows)
            ns["generate_static_relation_feat"](case["relations"], save_dir, feat_dir)
            rel_vid, rel_pno, rel_dur, rel_pred, idex_off, idex, want = [], [], [], [], [0], [], []
            for vid, rels in case["relations"].items():
                for pno, rel in enumerate(rels):
                    got = np.load(os.path.join(save_dir, rel["triplet"][1], "%s_%d.npy" % (vid, pno)))
                    assert got.dtype == np.float32 and got.shape == (case["dim"],) and np.isfinite(got).all()
                    rel_vid.append(vids.index(vid))
                    rel_pno.append(pno)
                    rel_dur.append(rel["duration"])
                    rel_pred.append(rel["triplet"][1])
                    idex.extend(rel["rel_idex"])
                    idex_off.append(len(idex))
                    want.append(got)
        slot_off = np.zeros(len(case["slots"]) + 1, np.int32)
        np.cumsum([len(s[2]) for s in case["slots"]], out=slot_off[1:])
        p = "c%d_" % c
        out.update({p + "vids": np.array(vids), p + "feat": np.concatenate([s[2] for s in case["slots"]]),
                    p + "slot_vid": np.array([vids.index(s[0]) for s in case["slots"]], np.int32),
                    p + "slot_fno": np.array([s[1] for s in case["slots"]], np.int32), p + "slot_off": slot_off,
                    p + "rel_vid": np.array(rel_vid, np.int32), p + "rel_pno": np.array(rel_pno, np.int32),
                    p + "rel_dur": np.array(rel_dur, np.int32).reshape(-1, 2), p + "rel_pred": np.array(rel_pred),
                    p + "idex_off": np.array(idex_off, np.int32), p + "idex": np.array(idex, np.int32),
                    p + "pooled": np.stack(want)})
        print("  case %d: dim %d, %d frame files, %d relations" % (c, case["dim"], len(case["slots"]), len(want)))
    save("video_relation_feat", "extracted", n_cases=np.array(len(cases.golden_inputs())), **out)


# ----------------------------------------------------------------------------- trajectory mAP of object tracks
def gen_track_eval():
    """tests/golden/track_eval.npz: the reference's eval_detection_scores / viou on the gap-free cases of
    tests/track_eval_cases.py golden_case.  Every trajectory enters as a relation with ``triplet = (class,)`` and ``sub_traj =
    obj_traj =`` the trajectory, so ``min(s_iou, o_iou)`` is the single vIoU and the reference's greedy loop is the matching of
    i2vsgg_amd.track_eval.  Per case: the seed it ended on, per threshold which predictions (packed order) hit and with what
    ov, and the smallest margins.  The reference adds in list order, the package in its lane order: a float32 case with a
    decision closer than 1e-9 (relative) to a threshold or a rival ov is redrawn from the next seed -- never dropped; the
    integer cases are exact in any order and keep their ties."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_eval_cases as tc
    from i2vsgg_amd import track_eval
    MARGIN = 1e-9
    ns = _utils_functions(["viou", "eval_detection_scores"])
    ref_viou = ns["viou"]
    calls = []
    ns["viou"] = lambda t1, d1, t2, d2: calls.append((id(t1), ref_viou(t1, d1, t2, d2))) or calls[-1][1]
    thr = list(tc.THRESHOLDS)
    seeds, off, hits, ovs, m_ov, m_gap, redraws = [], [0], [], [], [], [], 0
    for k in range(tc.GOLDEN_CASES):
        integer = k % 2 == 0
        seed = tc.GOLDEN_SEED + 100 * k
        while True:
            prediction, groundtruth = tc.golden_case(seed, integer)
            st = {}
            pk, _, ov_h, hit_h, hit_ov_h = track_eval.match(prediction, groundtruth, thr, stats=st)
            if integer or min(st.get("ov", np.inf), st.get("ov_gap", np.inf)) >= MARGIN:
                break
            seed, redraws = seed + 1, redraws + 1
        rel = lambda tr, score=None: dict(
            triplet=(tr["category"],), duration=[tr["frames"][0], tr["frames"][-1] + 1], score=score,
            sub_traj=np.asarray(tr["boxes"], np.float64).tolist(), obj_traj=np.asarray(tr["boxes"], np.float64).tolist())
        preds = [rel(tr, tr["score"]) for tr in prediction["g"]]
        for r in preds:
            r["obj_traj"] = r["sub_traj"]
        gts = [rel(tr) for tr in groundtruth["g"]]
        for r in gts:
            r["obj_traj"] = r["sub_traj"]
        order = np.argsort(-np.array([r["score"] for r in preds]), kind="stable")
        pid = dict((id(r["sub_traj"]), i) for i, r in enumerate(preds))
        hit_ref, ov_ref = np.zeros((len(thr), pk.n_pred), bool), np.full((len(thr), pk.n_pred), np.nan)
        for t, th in enumerate(thr):
            del calls[:]
            _, _, hit_scores = ns["eval_detection_scores"](gts, preds, th)
            tp = np.zeros(len(preds), bool)
            tp[order] = np.isfinite(hit_scores)
            best = np.full(len(preds), -np.inf)
            for i, val in calls:                                 # a prediction's hit is its largest computed ov >= threshold
                if val >= th:
                    best[pid[i]] = max(best[pid[i]], val)
            assert (np.isfinite(best) == tp).all()
            hit_ref[t] = tp[pk.pred_src]
            ov_ref[t] = np.where(tp, best, np.nan)[pk.pred_src]
        # the package's host form must already agree
        assert ((hit_h >= 0) == hit_ref).all(), k
        assert np.allclose(hit_ov_h[hit_ref], ov_ref[hit_ref], rtol=1e-12, atol=0), k
        if integer:
            assert (hit_ov_h[hit_ref] == ov_ref[hit_ref]).all(), k
        print("    case %2d seed %d (%s): %3d predictions, %3d ground truths, hits %s, margins ov %.3g gap %.3g" % (
            k, seed, "integer" if integer else "float32", pk.n_pred, pk.n_gt, hit_ref.sum(1).tolist(), st.get("ov", np.inf),
            st.get("ov_gap", np.inf)))
        seeds.append(seed)
        off.append(off[-1] + pk.n_pred)
        hits.append(hit_ref)
        ovs.append(ov_ref)
        m_ov.append(st.get("ov", np.inf))
        m_gap.append(st.get("ov_gap", np.inf))
    hits, ovs = np.concatenate(hits, 1), np.concatenate(ovs, 1)
    assert len(seeds) == tc.GOLDEN_CASES and hits[0].sum() > hits[1].sum() > hits[2].sum() > 0 and (~hits[0]).any()
    assert np.isfinite(m_gap[1::2]).any() and np.isfinite(m_gap[0::2]).any()       # rival ground truths, float32 and integer
    print("    %d redraws" % redraws)
    save("track_eval", "extracted", seeds=np.asarray(seeds, np.int32), pred_off=np.asarray(off, np.int32), thresholds=np.asarray(thr),
         hit=hits, hit_ov=ovs, margin_ov=np.asarray(m_ov), margin_ov_gap=np.asarray(m_gap), margin_bound=np.float64(MARGIN))


# ----------------------------------------------------------------------------- video relation NMS
def gen_video_nms():
    """tests/golden/video_nms.npz: greedy suppression decided from the reference's own ``viou`` on the cases of
    tests/video_nms_cases.py golden_case.  Per case the table of min(viou(subjects), viou(objects)) of EVERY same-triplet pair
    comes from the reference's function; the greedy decisions (rank order, strict ``>``) are taken from that table by the loop
    below.  The file holds data only, per case ``c<k>_``: the packed inputs (cell_off, rel, boxes, score), the threshold, the
    seed the case ended on and keep / by / by_ov.  Integer boxes make every sum exact in any order, so the package's host form
    must equal those cases in every bit; a fractional case with a decisive ov closer than 1e-9 (relative) to its threshold is
    redrawn from the next seed -- never dropped."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import video_nms_cases as nc
    from i2vsgg_amd import video
    MARGIN = 1e-9
    ref_viou = _utils_functions(["viou"])["viou"]
    out, margins, redraws = {}, [], 0
    for k in range(nc.GOLDEN_CASES):
        integer = k < nc.GOLDEN_CASES - 2
        seed = nc.GOLDEN_SEED + 100 * k
        while True:
            case = nc.golden_case(k, seed)
            T = case.T
            pk = video.pack_nms(case.prediction, case.pool)
            rels = [case.prediction[vid][int(pk.src[p])] for v, vid in enumerate(pk.vids)
                    for p in range(int(pk.video_off[v]), int(pk.video_off[v + 1]))]
            R = len(rels)
            keep, by, by_ov, margin, pairs = np.zeros(R, np.int32), np.full(R, -1, np.int32), np.full(R, -1.0), np.inf, 0
            for c in range(len(pk.cell_off) - 1):
                r0, r1 = int(pk.cell_off[c]), int(pk.cell_off[c + 1])
                assert len(set(tuple(rels[i]["triplet"]) for i in range(r0, r1))) == 1
                table = {}
                for i in range(r0, r1):
                    for j in range(i + 1, r1):
                        a, b = rels[i], rels[j]
                        table[i, j] = min(ref_viou(a["sub_traj"], a["duration"], b["sub_traj"], b["duration"]),
                                          ref_viou(a["obj_traj"], a["duration"], b["obj_traj"], b["duration"]))
                pairs += len(table)
                gone = set()
                for i in range(r0, r1):
                    if i in gone:
                        continue
                    keep[i] = 1
                    for j in range(i + 1, r1):
                        if j not in gone:
                            margin = min(margin, abs(table[i, j] - T) / max(T, 1e-300))
                            if table[i, j] > T:
                                gone.add(j)
                                by[j], by_ov[j] = i, table[i, j]
            if integer or margin >= MARGIN:
                break
            seed, redraws = seed + 1, redraws + 1
        keep_h, by_h, by_ov_h, _ = video.suppress_arrays_host(pk, T)           # the package's host form must already agree
        assert (keep_h == keep).all() and (by_h == by).all(), k
        assert np.allclose(by_ov_h, by_ov, rtol=1e-12, atol=0), k
        if integer:
            assert (by_ov_h.view(np.int64) == by_ov.view(np.int64)).all(), k
        print("    case %2d seed %d (%s): T %.3g, %3d relations in %d cells, %5d pairs, %3d kept, margin %.3g" % (
            k, seed, "integer" if integer else "fractional", T, R, len(pk.cell_off) - 1, pairs, int(keep.sum()), margin))
        margins.append(margin)
        out.update({"c%d_cell_off" % k: pk.cell_off, "c%d_rel" % k: pk.rel, "c%d_boxes" % k: pk.boxes, "c%d_score" % k: pk.score,
                    "c%d_T" % k: np.float64(T), "c%d_seed" % k: np.int64(seed), "c%d_keep" % k: keep, "c%d_by" % k: by,
                    "c%d_by_ov" % k: by_ov})
    assert min(margins[-2:]) >= MARGIN
    print("    %d redraws; smallest margin of a fractional case %.3g" % (redraws, min(margins[-2:])))
    save("video_nms", "extracted", n_cases=np.array(nc.GOLDEN_CASES), margin=np.asarray(margins), margin_bound=np.float64(MARGIN), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    todo = a.only.split(",") if a.only else ["direct", "roialign", "roialign_fresh", "tails", "rpn", "nets", "full", "ctx", "step",
                                             "vrd", "video", "det_eval", "recognition", "video_relation_feat", "track_eval",
                                             "video_nms", "target_edges"]
    if "direct" in todo:
        print("[direct imports]")
        gen_direct()
    if "roialign" in todo:
        print("[RoIAlign forward: the reference's C function compiled from its own lines]")
        gen_roi_align()
    if "roialign_fresh" in todo:
        print("[RoIAlign forward on further shapes: the same compiled function]")
        gen_roi_align_fresh()
    if "tails" in todo:
        print("[eval tails: direct imports + detection_output compiled from its own lines]")
        gen_eval_tails()
    if "det_eval" in todo:
        print("[detection evaluation: lib/datasets/voc_eval.py imported as shipped]")
        gen_det_eval()
    if "det_eval_time" in todo:
        print("[the reference's voc_eval, timed on this CPU]")
        time_det_eval()
    if "video" in todo:
        print("[video association / evaluation: lib/utils.py functions compiled from their own lines]")
        gen_video()
    if "video" in todo or "video_edges" in todo:
        print("[video evaluation on the edge set: the same lib/utils.py functions]")
        gen_video_edges()
    if "recognition" in todo:
        print("[predicate recognition: recognition_output / evaluate_recognition of lib/utils.py compiled from their own lines]")
        gen_recognition()
    if "video_relation_feat" in todo:
        print("[video relation features: generate_static_relation_feat of lib/utils.py compiled from its own lines]")
        gen_video_relation_feat()
    if "track_eval" in todo:
        print("[trajectory mAP of object tracks: viou / eval_detection_scores of lib/utils.py compiled from their own lines]")
        gen_track_eval()
    if "video_nms" in todo:
        print("[video relation NMS: viou of lib/utils.py compiled from its own lines, the greedy loop taken from its table]")
        gen_video_nms()
    if any(t in todo for t in ("rpn", "nets", "full", "vrd", "ctx", "step", "target_edges")):
        print("[imports with placeholders]")
        cfg = install_placeholders()
        if "rpn" in todo:
            gen_rpn_layers(cfg)
        if "target_edges" in todo:
            gen_target_edges(cfg)
        if "nets" in todo:
            gen_nets(cfg)
        if "full" in todo:
            gen_full_frame(cfg)
        if "ctx" in todo:
            gen_context(cfg)
        if "step" in todo:
            gen_step(cfg)
        if "vrd" in todo:
            gen_vrd(cfg)


if __name__ == "__main__":
    main()
