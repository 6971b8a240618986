"""Seeded synthetic weights, frames, boxes and relation annotations.

No dataset or checkpoint is reachable (no network), so every parity fixture, the smoke
test and the benchmark are driven by the generators below.  Inputs are regenerated from a
seed with numpy's PCG64 ``default_rng`` (platform-stable), so golden files only need to
hold outputs.  Parameter names are the reference's state_dict keys
(``RCNN_base.6.3.conv2.weight``, ``vrd.fc6.fc.weight`` ...) so reference checkpoints
and these synthetic ones load through the same path.
"""
import math

import numpy as np
import torch

RESNET_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}


def _normal(rng, shape, std, device=None, gen=None):
    if rng is not None:
        return torch.from_numpy((rng.standard_normal(shape, dtype=np.float32) * np.float32(std)))
    return torch.randn(shape, device=device, generator=gen, dtype=torch.float32) * std


def _conv_w(rng, cout, cin, k, device, gen):
    # He-normal over fan-out as ResNet.__init__ does (resnet_instance_styleD_bilinear.py:238-241)
    return _normal(rng, (cout, cin, k, k), math.sqrt(2.0 / (k * k * cout)), device, gen)


def _bn(rng, c, device, gen, prefix, out, gamma=(0.5, 1.0)):
    if rng is not None:
        g = rng.uniform(gamma[0], gamma[1], c).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, c).astype(np.float32)
        m = rng.uniform(-0.1, 0.1, c).astype(np.float32)
        v = rng.uniform(0.5, 1.5, c).astype(np.float32)
        g, b, m, v = (torch.from_numpy(t) for t in (g, b, m, v))
    else:
        u = lambda lo, hi: torch.rand(c, device=device, generator=gen) * (hi - lo) + lo
        g, b, m, v = u(*gamma), u(-0.1, 0.1), u(-0.1, 0.1), u(0.5, 1.5)
    out[prefix + ".weight"], out[prefix + ".bias"] = g, b
    out[prefix + ".running_mean"], out[prefix + ".running_var"] = m, v


def _layer(rng, out, key, inplanes, planes, nblocks, stride, device, gen):
    for i in range(nblocks):
        k = "%s.%d" % (key, i)
        cin = inplanes if i == 0 else planes * 4
        out[k + ".conv1.weight"] = _conv_w(rng, planes, cin, 1, device, gen)
        _bn(rng, planes, device, gen, k + ".bn1", out)
        out[k + ".conv2.weight"] = _conv_w(rng, planes, planes, 3, device, gen)
        _bn(rng, planes, device, gen, k + ".bn2", out)
        out[k + ".conv3.weight"] = _conv_w(rng, planes * 4, planes, 1, device, gen)
        _bn(rng, planes * 4, device, gen, k + ".bn3", out, gamma=(0.2, 0.5))
        if i == 0 and (stride != 1 or inplanes != planes * 4):
            out[k + ".downsample.0.weight"] = _conv_w(rng, planes * 4, cin, 1, device, gen)
            _bn(rng, planes * 4, device, gen, k + ".downsample.1", out)
    return planes * 4


def backbone_params(seed=0, layers=101, top=True, device=None, numpy_rng=True):
    """conv1..layer3 as ``RCNN_base.N`` (+ layer4 as ``RCNN_top.0`` when ``top``)."""
    rng = np.random.default_rng(seed) if numpy_rng else None
    gen = None if numpy_rng else torch.Generator(device=device).manual_seed(seed)
    blocks = RESNET_BLOCKS[layers]
    p = {"RCNN_base.0.weight": _conv_w(rng, 64, 3, 7, device, gen)}
    _bn(rng, 64, device, gen, "RCNN_base.1", p)
    c = _layer(rng, p, "RCNN_base.4", 64, 64, blocks[0], 1, device, gen)
    c = _layer(rng, p, "RCNN_base.5", c, 128, blocks[1], 2, device, gen)
    c = _layer(rng, p, "RCNN_base.6", c, 256, blocks[2], 2, device, gen)
    if top:
        _layer(rng, p, "RCNN_top.0", c, 512, blocks[3], 2, device, gen)
    return _to(p, device)


def _to(p, device):
    if device is None:
        return p
    return {k: v.to(device) for k, v in p.items()}


def rpn_params(seed=10, din=1024, n_anchor=9, device=None, std=0.01):
    """rpn/rpn.py:27-36; normal(0, 0.01) like _init_weights (faster_rcnn_instance...:205-207)
    but with non-zero biases so the bias path is exercised."""
    rng = np.random.default_rng(seed)
    p = {
        "RCNN_rpn.RPN_Conv.weight": _normal(rng, (512, din, 3, 3), std),
        "RCNN_rpn.RPN_Conv.bias": _normal(rng, (512,), 0.01),
        "RCNN_rpn.RPN_cls_score.weight": _normal(rng, (2 * n_anchor, 512, 1, 1), std),
        "RCNN_rpn.RPN_cls_score.bias": _normal(rng, (2 * n_anchor,), 0.01),
        "RCNN_rpn.RPN_bbox_pred.weight": _normal(rng, (4 * n_anchor, 512, 1, 1), std),
        "RCNN_rpn.RPN_bbox_pred.bias": _normal(rng, (4 * n_anchor,), 0.01),
    }
    return _to(p, device)


def det_head_params(seed=11, n_classes=16, feat_d=2048, device=None):
    rng = np.random.default_rng(seed)
    p = {
        "RCNN_cls_score.weight": _normal(rng, (n_classes, feat_d), 0.01),
        "RCNN_cls_score.bias": _normal(rng, (n_classes,), 0.01),
        "RCNN_bbox_pred.weight": _normal(rng, (4 * n_classes, feat_d), 0.001),
        "RCNN_bbox_pred.bias": _normal(rng, (4 * n_classes,), 0.01),
    }
    return _to(p, device)


def netd_params(seed=12, dim=512, rank=5, device=None):
    """netD_pixel (1x1 convs, no bias) + netD_style (two 512->dim*rank FCs + 512->1)."""
    rng = np.random.default_rng(seed)
    p = {
        "netD_pixel.conv1.weight": _normal(rng, (512, 1024, 1, 1), 0.01),
        "netD_pixel.conv2.weight": _normal(rng, (128, 512, 1, 1), 0.01),
        "netD_pixel.conv3.weight": _normal(rng, (1, 128, 1, 1), 0.01),
        # kaiming_normal_(fan_out, relu): std = sqrt(2 / out_features)
        "netD_style.fc_1.weight": _normal(rng, (dim * rank, 512), math.sqrt(2.0 / (dim * rank))),
        "netD_style.fc_1.bias": _normal(rng, (dim * rank,), 0.02),
        "netD_style.fc_2.weight": _normal(rng, (dim * rank, 512), math.sqrt(2.0 / (dim * rank))),
        "netD_style.fc_2.bias": _normal(rng, (dim * rank,), 0.02),
        "netD_style.fc1.weight": _normal(rng, (1, dim), math.sqrt(2.0)),
        "netD_style.fc1.bias": _normal(rng, (1,), 0.02),
    }
    return _to(p, device)


VRD_SHAPES = (
    # key, out, in  (resnet_SGG_emb.py:83-127)
    ("vrd.fc6.fc", 4096, 1024 * 7 * 7),
    ("vrd.fc7.fc", 4096, 4096),
    ("vrd.so_vis_embeddings.fc", None, 4096),     # out = emb_dim
    ("vrd.fc8.fc", 256, 4096),
    ("vrd.fc_so.fc", 256, 600),
    ("vrd.fc_lov.fc", 256, 64),
    ("vrd.fc_fusion.fc", 256, 768),
    ("vrd.fc_rel.fc", None, 256),                 # out = emb_dim
    ("vrd.prd_sem_embeddings.0", 1024, 300),
    ("vrd.prd_sem_embeddings.2", None, 1024),     # out = emb_dim
)
VRD_CONVS = (("vrd.conv_lo.0.conv", 96, 2, 5), ("vrd.conv_lo.1.conv", 128, 96, 5),
             ("vrd.conv_lo.2.conv", 64, 128, 8))


def vrd_params(seed=13, emb_dim=300, device=None, numpy_rng=True, fc6_in=1024 * 7 * 7, use_obj_visual=True, spatial_type=2):
    """All ``vrd.*`` tensors: 226 480 996 parameters at emb_dim=300 (906 MB fp32).  ``use_obj_visual`` / ``spatial_type``: the
    variants of resnet_SGG_emb.py:94-123 (no ``fc_so``; ``fc_lov`` on 8 inputs / no spatial branch; ``fc_fusion`` narrower);
    the tensors every variant has are the same numbers as the default's (drawn in the same order, the others skipped)."""
    rng = np.random.default_rng(seed) if numpy_rng else None
    gen = None if numpy_rng else torch.Generator(device=device).manual_seed(seed)
    p = {}
    n_fusion = 256 * (1 + int(bool(use_obj_visual)) + int(spatial_type in (1, 2)))
    for key, cout, cin in VRD_SHAPES:
        cout = emb_dim if cout is None else cout
        cin = fc6_in if key == "vrd.fc6.fc" else cin
        full = (cout, cin)
        if key == "vrd.fc_lov.fc" and spatial_type == 1:
            cin = 8
        if key == "vrd.fc_fusion.fc":
            cin = n_fusion
        if (cout, cin) != full or (key == "vrd.fc_so.fc" and not use_obj_visual) or (key == "vrd.fc_lov.fc" and spatial_type not in (1, 2)):
            # keep the default's random stream for every other tensor: draw the default-shaped tensor, then a narrower one
            _normal(rng, full, 1.0 / math.sqrt(full[1]), device, gen)
            _normal(rng, (full[0],), 1.0 / math.sqrt(full[1]), device, gen)
            if (key == "vrd.fc_so.fc" and not use_obj_visual) or (key == "vrd.fc_lov.fc" and spatial_type not in (1, 2)):
                continue
            r2 = np.random.default_rng(seed + 1000 + cin) if numpy_rng else None
            bound = 1.0 / math.sqrt(cin)
            p[key + ".weight"] = _normal(r2, (cout, cin), bound, device, gen)
            p[key + ".bias"] = _normal(r2, (cout,), bound, device, gen)
            continue
        bound = 1.0 / math.sqrt(cin)                 # nn.Linear default scale
        p[key + ".weight"] = _normal(rng, (cout, cin), bound, device, gen)
        p[key + ".bias"] = _normal(rng, (cout,), bound, device, gen)
    for key, cout, cin, k in VRD_CONVS:
        bound = 1.0 / math.sqrt(cin * k * k)
        w, b = _normal(rng, (cout, cin, k, k), bound, device, gen), _normal(rng, (cout,), bound, device, gen)
        if spatial_type == 2:
            p[key + ".weight"], p[key + ".bias"] = w, b
    return _to(p, device)


# ------------------------------------------------------------------------ inputs
def frames(seed, batch, h=600, w=1000):
    """Mean-subtracted BGR-scale frames (B,3,h,w) fp32 and im_info (B,3)=[h,w,1]."""
    rng = np.random.default_rng(seed)
    im = (rng.standard_normal((batch, 3, h, w), dtype=np.float32) * np.float32(50.0))
    info = np.tile(np.array([[h, w, 1.0]], np.float32), (batch, 1))
    return im, info


def boxes(seed, n, im_h=600, im_w=1000, min_side=32, max_side=400):
    """n boxes: x1,y1 uniform, w,h in [min_side,max_side] px, clipped (fp32, (n,4))."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(0, im_w - min_side - 1, n)
    y1 = rng.uniform(0, im_h - min_side - 1, n)
    bw = rng.uniform(min_side, max_side, n)
    bh = rng.uniform(min_side, max_side, n)
    x2 = np.minimum(x1 + bw, im_w - 1)
    y2 = np.minimum(y1 + bh, im_h - 1)
    return np.stack([x1, y1, x2, y2], 1).astype(np.float32)


def gt_boxes(seed, batch, n_gt, n_classes=16, max_gt=30, im_h=600, im_w=1000):
    """(B,max_gt,5) zero-padded [x1,y1,x2,y2,cls] with integer pixel corners, num_boxes (B,)."""
    out = np.zeros((batch, max_gt, 5), np.float32)
    rng = np.random.default_rng(seed + 7919)
    for b in range(batch):
        bx = np.floor(boxes(seed * 131 + b, n_gt, im_h, im_w, 48, 360))
        out[b, :n_gt, :4] = bx
        out[b, :n_gt, 4] = rng.integers(1, n_classes, n_gt)
    return out, np.full((batch,), n_gt, np.int64)


def relation_annotation(seed, n_boxes=32, n_pairs=32, n_rel=62, n_classes=16, im_h=600, im_w=1000):
    """One frame's VidVRD-style annotation dict like ``vrd.source_gt_rels[im_path]``
    (faster_rcnn_SGG_emb.py:169-172): boxes (python lists, unscaled pixels), box_classes,
    rels = [s, o, predicate] with 1-3 predicates on each of n_pairs distinct ordered pairs."""
    rng = np.random.default_rng(seed)
    bx = np.floor(boxes(seed + 1, n_boxes, im_h, im_w)).astype(np.float64)
    pairs = set()
    while len(pairs) < n_pairs:
        s, o = (int(v) for v in rng.integers(0, n_boxes, 2))
        if s != o:
            pairs.add((s, o))
    rels = []
    for s, o in sorted(pairs, key=lambda _: rng.random()):
        for r in rng.choice(n_rel, size=int(rng.integers(1, 4)), replace=False):
            rels.append([s, o, int(r)])
    order = rng.permutation(len(rels))
    return {"boxes": bx.tolist(), "box_classes": rng.integers(1, n_classes, n_boxes).tolist(),
            "rels": [rels[i] for i in order]}


def detections_for(seed, anno, exact=False, jitter=0.08, copies=1, n_wrong=2, n_distractors=4, n_classes=16, im_h=600, im_w=1000):
    """Detections for one annotated frame, in the layout ``seqnms.to_annotations`` writes and ``vrd.source_det_boxes`` holds:
    {"boxes" (unscaled pixels), "box_classes", "scores"}.  ``exact``: the annotated boxes themselves, in their order, score 1.
    Otherwise ``copies`` times every annotated box with each corner coordinate moved by at most ``jitter`` of that side (so its overlap with
    the annotated box is at least ((1 - 2 jitter) / (1 + 2 jitter))^2: 0.52 at the default, a match; above 0.17 some fall
    below 0.5), ``n_wrong`` copies of annotated boxes under another class and ``n_distractors`` boxes anywhere, all clipped
    to the image, in a seeded order, scores in (0.7, 1)."""
    gt = np.asarray(anno["boxes"], np.float64).reshape(-1, 4)
    cls = [int(c) for c in anno["box_classes"]]
    if exact:
        return {"boxes": gt.tolist(), "box_classes": cls, "scores": [1.0] * len(cls)}
    rng = np.random.default_rng(seed + 4241)
    side = np.stack([gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]] * 2, 1)
    out = [gt + rng.uniform(-jitter, jitter, gt.shape) * side for _ in range(copies)]
    out_cls = list(cls) * copies
    if len(gt) and n_wrong:
        pick = rng.integers(0, len(gt), n_wrong)
        out.append(gt[pick] + rng.uniform(-jitter, jitter, (n_wrong, 4)) * side[pick])
        out_cls += [cls[i] % (n_classes - 1) + 1 for i in pick]
    if n_distractors:
        out.append(boxes(seed + 4242, n_distractors, im_h, im_w).astype(np.float64))
        out_cls += [int(c) for c in rng.integers(1, n_classes, n_distractors)]
    b = np.clip(np.concatenate(out), 0, [im_w - 1, im_h - 1, im_w - 1, im_h - 1])
    order = rng.permutation(len(b))
    scores = rng.uniform(0.7, 1.0, len(b))
    return {"boxes": b[order].tolist(), "box_classes": [out_cls[i] for i in order], "scores": scores.tolist()}


def word_vectors(seed, n, dim=300):
    """Stand-in for the GloVe rows (``all_obj_vecs`` / ``all_prd_vecs``): (n,dim) fp32."""
    return np.random.default_rng(seed).standard_normal((n, dim), dtype=np.float32)


def tie_free_dets(seed, n, im_h=600, im_w=1000, clustered=False):
    """(n,5) [x1,y1,x2,y2,score] sorted by strictly decreasing score (tie-free)."""
    rng = np.random.default_rng(seed)
    if clustered:
        k = max(1, n // 40)
        centres = boxes(seed + 3, k, im_h, im_w, 48, 300)
        b = centres[rng.integers(0, k, n)] + rng.normal(0, 6.0, (n, 4)).astype(np.float32)
        b = np.stack([np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3]),
                      np.maximum(b[:, 0], b[:, 2]), np.maximum(b[:, 1], b[:, 3])], 1)
        b[:, 0::2] = np.clip(b[:, 0::2], 0, im_w - 1)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, im_h - 1)
    else:
        b = boxes(seed + 3, n, im_h, im_w, 16, 400)
    s = np.sort(rng.permutation(4 * n + 16)[:n].astype(np.float32))[::-1] / np.float32(4 * n + 16)
    return np.concatenate([b.astype(np.float32), s[:, None].astype(np.float32)], 1)


def roi_cases(seed, B, H, W, scale=16.0, n=24):
    """(n+6,5) ROIs [b,x1,y1,x2,y2] for a (B,C,H,W) map: n seeded boxes plus a full-image, a sub-pixel, a malformed
    (x2<x1, y2<y1), a partly outside (negative), a beyond-the-far-edge and a single-point box -- the classes
    tests/golden/roi_align_fwd.npz (tools/gen_golden.py gen_roi_align) and the ROI kernel tests cover."""
    rng = np.random.default_rng(seed)
    bx = boxes(int(rng.integers(1 << 30)), n, H * scale, W * scale, 16, min(H, W) * scale * 0.9)
    r = np.zeros((n + 6, 5), np.float32)
    r[:n, 1:] = bx
    r[:n, 0] = rng.integers(0, B, n)
    r[n + 0] = [0, 0, 0, W * scale - 1, H * scale - 1]            # full image
    r[n + 1] = [B - 1, 40.5, 33.25, 41.0, 33.5]                   # sub-pixel
    r[n + 2] = [0, 120, 90, 60, 30]                               # malformed: x2<x1, y2<y1
    r[n + 3] = [B - 1, -50, -40, 80, 70]                          # partly outside (negative)
    r[n + 4] = [0, W * scale - 30, H * scale - 30, W * scale + 90, H * scale + 60]   # beyond the far edge
    r[n + 5] = [B - 1, 10, 10, 10, 10]                            # single point
    return r


def sampled_rois(seed, B, H, W, R, n_gt=8, scale=16.0, with_gt=False):
    """(B*R,5) ROIs [b,x1,y1,x2,y2] shaped like the proposal target layer's output for a (B,C,H,W) map: per frame at most
    round(0.25 R) foreground ROIs, each a jittered copy (every corner moved by at most 6 % of the box's side: IoU >= 0.6) of
    one of n_gt <= 8 gt boxes, so that they pile up in clusters as the sampler's do; the rest background boxes drawn over the
    whole frame.  ``with_gt``: also the (B,n_gt,4) gt boxes the foreground was drawn around."""
    rng = np.random.default_rng(seed)
    im_h, im_w = H * scale, W * scale
    n_fg = min(int(round(0.25 * R)), R)
    out = np.zeros((B * R, 5), np.float32)
    gts = np.zeros((B, min(n_gt, 8), 4), np.float32)
    for b in range(B):
        gts[b] = gt = boxes(int(rng.integers(1 << 30)), min(n_gt, 8), im_h, im_w, 48, min(im_h, im_w) * 0.6).astype(np.float64)
        src = gt[rng.integers(0, gt.shape[0], n_fg)]
        side = np.concatenate([src[:, 2:] - src[:, :2]] * 2, 1)
        fg = np.clip(src + rng.uniform(-0.06, 0.06, src.shape) * side, 0, [im_w - 1, im_h - 1, im_w - 1, im_h - 1])
        bg = boxes(int(rng.integers(1 << 30)), R - n_fg, im_h, im_w, 16, min(im_h, im_w) * 0.8)
        r = out[b * R:(b + 1) * R]
        r[:, 0] = b
        r[:n_fg, 1:] = fg
        r[n_fg:, 1:] = bg
    return (out, gts) if with_gt else out


ROI_ALIGN_GOLDEN_CASES = ((4, 9, 11, 2), (64, 19, 32, 2), (1024, 38, 63, 1))          # (C, H, W, B)


def roi_align_golden_inputs(C, H, W, B):
    """The seeded map (B,C,H,W) and rois of one tests/golden/roi_align_fwd.npz case."""
    feat = np.random.default_rng(9000 + C + H).standard_normal((B, C, H, W), dtype=np.float32)
    return feat, roi_cases(9100 + C, B, H, W)


def instance_styled_step_params(layers=101, n_cls=16):
    """Seeded weights of the tests/golden/instance_styled_step.npz model (reference state_dict keys)."""
    p = {}
    p.update(backbone_params(0, layers, top=True))
    p.update(rpn_params(10, std=0.01))      # 0.02 saturates the scores: hundreds of exact ties among the top proposals
    p.update(det_head_params(11, n_cls))
    p.update(netd_params(12))
    return p


def instance_styled_step_inputs(B, H, W, n_cls=16):
    """Source frames + gt, target frames of one instance_styleD step of the golden: (im, info, gt, nb, im_t, info_t)."""
    im, info = frames(5, B, H, W)
    gt, nb = gt_boxes(6, B, 6, n_cls, im_h=H, im_w=W)
    im_t, info_t = frames(8, B, H, W)
    return im, info, gt, nb, im_t, info_t


def context_inputs(B=2, H=320, W=480):
    """Inputs of the ic/gc fixture (tools/gen_golden.py gen_context and tests/test_gpu_models.py): frames, gt, fixed proposals."""
    im, info = frames(5, B, H, W)
    gt, nb = gt_boxes(6, B, 6, 16, im_h=H, im_w=W)
    rois = np.zeros((B, 600, 5), np.float32)
    for b in range(B):
        rois[b, :, 0] = b
        rois[b, :, 1:] = boxes(430 + b, 600, im_h=H, im_w=W, min_side=16, max_side=220)
        jit = np.random.default_rng(440 + b).normal(0, 6, (48, 4)).astype(np.float32)
        rois[b, :48, 1:] = np.clip(gt[b, np.arange(48) % 6, :4] + jit, 0, [W - 1, H - 1, W - 1, H - 1])
    return im, info, gt, nb, rois


# ----------------------------------------------------------------------------------------------------------------
# videos for the association / evaluation of i2vsgg_amd.video (tests/golden/video_*.npz hold the reference's results)
# ----------------------------------------------------------------------------------------------------------------
def video_frames(seed, n_frames, n_objects=7, n_pred=100, integer=False, quant=0, p_break=0.02, first_frame=0, n_cand=120):
    """One video's per-frame relation predictions, [[fno, [[conf, [s, p, o], [sub_box, obj_box], rel_idex], ...]], ...], as
    the relation test loop would hand them over: a few persistent objects whose boxes drift slowly (object 1 is a twin of
    object 0: same class, nearly the same box, the same scores -- true ties, and two predictions that want one relation),
    ``n_cand`` (subject, predicate, object) candidates whose scores move slowly (triangle waves plus a little noise), the best ``n_pred`` of
    them per frame, listed in a shuffled order.  With probability ``p_break`` per frame an object jumps, which ends its
    relations.  Only uniform draws and + - * are used, so every machine regenerates the same bits.  ``integer``: boxes
    with integer coordinates; ``quant``: scores rounded to multiples of 1/quant (exact sums, many ties)."""
    rng = np.random.RandomState(seed)
    cls = rng.randint(1, 16, n_objects)
    cls[1] = cls[0]

    def draw_box():
        w, h = rng.randint(60, 200), rng.randint(60, 200)
        x, y = rng.randint(0, 640 - w), rng.randint(0, 360 - h)
        b = np.array([x, y, x + w, y + h], np.float64)
        return b if integer else b + rng.random_sample(4)

    box = np.stack([draw_box() for _ in range(n_objects)])
    pairs = [(i, j) for i in range(n_objects) for j in range(n_objects) if i != j and not (i < 2 and j < 2)]
    cand = []
    while len(cand) < n_cand:
        i, j = pairs[rng.randint(len(pairs))]
        if i == 1:
            continue                                     # the twin's candidates are copies of object 0's, below
        c = (i, j, int(rng.randint(1, 62)))
        if c not in cand:
            cand.append(c)
    wave = [(rng.random_sample() * 0.6 + 0.2, rng.random_sample() * 0.15, int(rng.randint(40, 200)), int(rng.randint(200)))
            for _ in cand]
    twin = [k for k, c in enumerate(cand) if c[0] == 0][:12]
    cand += [(1, cand[k][1], cand[k][2]) for k in twin]
    wave += [wave[k] for k in twin]
    frames = []
    for t in range(n_frames):
        if t:
            step = rng.randint(-2, 3, (n_objects, 4)).astype(np.float64) if integer else rng.random_sample((n_objects, 4)) * 3 - 1.5
            step[:, 2:] = step[:, :2] + (step[:, 2:] - step[:, :2]) * 0.25          # mostly a translation
            if integer:
                step = np.round(step)
            box = box + step
            for k in np.nonzero(rng.random_sample(n_objects) < p_break)[0]:
                if k > 1:
                    box[k] = draw_box()
            box[1] = box[0] + (2.0 if integer else 2.25)
        score = np.empty(len(cand))
        noise = rng.random_sample(len(cand)) * 0.02      # no two stretches of a wave repeat the same numbers
        noise[n_cand:] = noise[twin]
        for k, (b, a, period, phase) in enumerate(wave):
            u = ((t + phase) % period) / float(period)
            score[k] = b + a * (4 * abs(u - 0.5) - 1) + noise[k]
        if quant:
            score = np.round(score * quant) / quant
        best = np.argsort(-score, kind="stable")[:n_pred]
        best = best[rng.permutation(len(best))]
        frames.append([first_frame + t, [[float(score[k]), [float(cls[cand[k][0]]), float(cand[k][2]), float(cls[cand[k][1]])],
                                          [box[cand[k][0]].tolist(), box[cand[k][1]].tolist()], int(k)] for k in best]])
    return frames


def video_fixture_cases():
    """The videos of tests/golden/video_association.npz, {vid: frames}: a dozen of 30-150 frames, one long, and the edge
    cases by construction (tools/gen_golden.py asserts that each is present before it writes the file)."""
    out = {}
    for k, (n, integer, quant) in enumerate([(30, False, 0), (48, True, 0), (64, False, 0), (80, True, 64), (96, False, 0),
                                             (120, False, 64), (150, True, 0), (40, False, 0)]):
        out["v%02d" % k] = video_frames(100 + k, n, integer=integer, quant=quant, first_frame=7 * k)
    # empty frames: both ends, inside, a run of 11 (its middle stays empty), short runs near the ends, a gap in numbers
    fr = video_frames(120, 90)
    for i in [0, 1, 5, 6, 20, 30, 31, 32] + list(range(45, 56)) + [83, 84, 85, 88, 89]:
        fr[i][1] = []
    del fr[70:73]
    out["empty"] = fr
    # a frame with more than 100 predictions, in a video short enough that the window of an empty frame is clipped twice
    fr = video_frames(121, 34, n_pred=130, n_cand=140)
    fr[3][1] = []
    fr[31][1] = []
    out["wide"] = fr
    # the object of a relation moves away while its subject stays; relations of exactly 9 and exactly 10 members
    fr = video_frames(122, 60, p_break=0.0, integer=True)
    sub, obj, far = [10.0, 10.0, 110.0, 110.0], [200.0, 50.0, 300.0, 150.0], [400.0, 200.0, 500.0, 300.0]
    for t, f in enumerate(fr):
        f[1].append([0.96875 if t < 25 else 0.9609375, [3.0, 60.0, 4.0], [list(sub), list(obj if t < 25 else far)], 900])
        if 5 <= t < 14:
            f[1].append([0.953125, [3.0, 59.0, 4.0], [list(sub), list(obj)], 901])
        if 20 <= t < 30:
            f[1].append([0.9375, [3.0, 58.0, 4.0], [list(sub), list(obj)], 902])
    out["moved"] = fr
    # many short relations: more than 200 survive the 10-member rule
    out["many"] = video_frames(123, 260, p_break=0.03, n_objects=9)
    fr = video_frames(125, 600, p_break=0.004)
    for f in fr:                                         # one relation as long as the video
        f[1].append([0.97265625, [5.0, 60.0, 6.0], [[20.5, 30.25, 140.0, 200.5], [300.0, 40.5, 420.25, 210.0]], 900])
    out["long"] = fr
    return out


def video_groundtruth(relations, seed):
    """Ground truth for ``video.evaluate`` made from one video's predicted relations: some are annotated with jittered
    boxes (hits), some with a shifted duration (a partial overlap), some triplets are never predicted, and some
    predictions have no annotation of their triplet."""
    rng = np.random.RandomState(seed)
    gts, seen = [], set()
    for k, r in enumerate(relations):
        key = (tuple(r["triplet"]), tuple(r["duration"]))
        if k % 3 == 2 or key in seen:                    # not annotated; twins share one annotation
            continue
        seen.add(key)
        n = len(r["sub_traj"])
        shift = [0, 0, n // 3, (2 * n) // 3][k % 4]      # the annotation starts later: a partial overlap
        jit = lambda traj: [[c + float(rng.randint(-3, 4)) for c in b] for b in traj[shift:]]
        gts.append({"triplet": list(r["triplet"]), "duration": [r["duration"][0] + shift, r["duration"][1]],
                    "sub_traj": jit(r["sub_traj"]), "obj_traj": jit(r["obj_traj"])})
        if len(gts) >= 30:
            break
    for k in range(3):                                   # annotated, never predicted
        b = [[10.0 * k, 20.0, 90.0 + 10 * k, 120.0]] * 12
        gts.append({"triplet": [1, 61 - k, 2], "duration": [3, 15], "sub_traj": b, "obj_traj": b})
    return gts


def recognition_set(seed, keys, sizes, frames_per_video, n_rel=62, n_classes=16, classes=None, n_tracks=4, n_relations=5):
    """A small predicate-recognition set: every ``frames_per_video`` consecutive entries of ``keys`` (frame file names, in
    order; ``sizes``: their (h, w)) are a video "0", "1", ... whose objects carry track ids that persist over its frames.
    -> (target_gt_rels, groundtruth): per frame ``{"boxes", "box_classes", "rels": [[s, o, p]], "tids": [[subject_tid,
    object_tid]] per relation}`` (the layout ``forward_predicate`` reads in eval mode, faster_rcnn_SGG_emb.py:277-322), and the
    video-level ``{vid: [{"triplet": [s, p, o], "subject_tid", "object_tid", "duration": [start, end)}]}`` that matches them:
    a relation is annotated in every frame of its duration in which both of its tracks are visible.  Subjects and objects are
    named from ``classes`` when given (labels otherwise); predicates are labels."""
    rng = np.random.default_rng(seed)
    per = int(frames_per_video) if frames_per_video > 0 else max(len(keys), 1)
    annos, gt = {}, {}
    for v in range((len(keys) + per - 1) // per):
        frames_v = list(range(v * per, min((v + 1) * per, len(keys))))
        nf = len(frames_v)
        cls = rng.integers(1, n_classes, n_tracks)
        pos = rng.uniform(0.05, 0.55, (n_tracks, 2))                  # top-left corner and size as fractions of the frame
        ext = rng.uniform(0.25, 0.4, (n_tracks, 2))
        vel = rng.uniform(-0.01, 0.01, (n_tracks, 2))
        visible = rng.random((nf, n_tracks)) < 0.85
        visible[:, :2] = True                                         # two tracks in every frame
        if nf > 2:
            visible[nf // 2, 1:] = False                              # ... but for one frame with a single box
        pairs = [(s, o) for s in range(n_tracks) for o in range(n_tracks) if s != o]
        rels = []
        for i in rng.permutation(len(pairs))[:n_relations]:
            a = int(rng.integers(0, max(nf - 1, 1)))
            rels.append((pairs[i][0], pairs[i][1], int(rng.integers(0, n_rel)), a, int(rng.integers(a + 1, nf + 1))))
        rels.append(rels[0][:2] + ((rels[0][2] + 1) % n_rel,) + rels[0][3:])     # a second predicate on the first pair
        seen = {}
        for t, k in enumerate(frames_v):
            h, w = sizes[k]
            tracks = [j for j in rng.permutation(n_tracks) if visible[t, j]]
            x1, y1 = (pos[tracks] + vel[tracks] * t).T
            bx = np.floor(np.stack([x1 * w, y1 * h, np.minimum((x1 + ext[tracks, 0]) * w, w - 1),
                                    np.minimum((y1 + ext[tracks, 1]) * h, h - 1)], 1))
            slot = dict((j, i) for i, j in enumerate(tracks))
            fr, ft = [], []
            for r, (s, o, p, a, b) in enumerate(rels):
                if a <= t < b and s in slot and o in slot:
                    fr.append([slot[s], slot[o], p])
                    ft.append([int(s), int(o)])
                    seen.setdefault(r, []).append(t)
            annos[keys[k]] = {"boxes": bx.tolist(), "box_classes": [int(cls[j]) for j in tracks], "rels": fr, "tids": ft}
        name = (lambda c: classes[c]) if classes is not None else int
        gt[str(v)] = [{"triplet": [name(int(cls[s])), p, name(int(cls[o]))], "subject_tid": int(s), "object_tid": int(o),
                       "duration": [min(seen[r]), max(seen[r]) + 1]} for r, (s, o, p, a, b) in enumerate(rels) if r in seen]
    return annos, gt
