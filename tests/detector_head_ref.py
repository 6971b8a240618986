"""A float64 reference of the detector head of the instance_styleD step (no tests here): everything of ``_fasterRCNN.forward_features``
behind ``extract_feature`` plus the loss of ``train.InstanceStyleDStep._body``, on the CPU, in plain torch.  Nothing here imports a
kernel, ``i2vsgg_amd.ops``, ``i2vsgg_amd.optim`` or a product module: the formulas are the reference's (``oracle/nets.py``: rpn_head,
netd_pixel, netd_style, head_to_tail, _GRL; rpn/rpn.py:76-108; faster_rcnn_instance_styleD_bilinear.py:62-182; trainval_net_instance_
styleD_bilinear.py:271-296), written out again.

The reference samples nothing.  It is GIVEN what the sampling layers produced -- the anchor target layer's (labels, targets, inside,
outside weights) in (y, x, a) order, the proposal target layer's (rois, labels, targets, inside, outside weights), or for a target-domain
call the proposal layer's rois -- and from there on it is differentiable float64:

  source  rpn_cls + rpn_box + rcnn_cls + rcnn_box + 0.5 mean(d_inst^2) + style_lambda 0.5 mean(d_style^2)
  target  0.5 mean((1 - d_inst)^2) + style_lambda 0.5 mean((1 - d_style)^2)

RoIAlignAvg is a matrix product with the coefficient matrix ``tests/roi_align_pin.roi_align_matrix`` extracts from the pinned forward.
Every ReLU takes an optional mask (RPN_Conv, netD_pixel's two, layer4's nine through ``bottleneck_ref.chain_forward``); without one the
reference chooses ``pre > 0`` itself.  The sign of ``signed_sqrt`` and the smooth-L1 switch at |d| = 1 / sigma^2 are float64's own (the
``choices`` of a run; a float32 evaluation is handed them so that both compute the same polynomial).

``plant`` puts ONE deliberate backward-or-wiring error into the reference (PLANTS), for the host test that shows the bounds of
tests/test_gpu_detector_head.py would catch it."""
import numpy as np
import torch
import torch.nn.functional as F

import bottleneck_ref as BR
from i2vsgg_amd import synthetic as syn
from i2vsgg_amd.model.utils.config import cfg
from oracle import cops, nets, rpn as orpn
from roi_align_pin import roi_align_matrix

B, N_CLS, ROIS = 2, 16, 8
IM_H, IM_W = 160, 224
FEAT, FEAT1 = (B, 1024, 10, 14), (B, 512, 20, 28)
ETA, ETA_STYLE, STYLE_LAMBDA = 0.5, 0.3, 0.7            # distinct and not 1: a swapped or dropped factor shows
ANCHOR_SCALES, ANCHOR_RATIOS = (2, 4, 6), (0.5, 1, 2)   # 32 / 64 / 96 px anchors: all three sizes fit into 160 x 224
N_GT = (3, 1)
Z_MARGIN, SL1_MARGIN = 1e-3, 1e-4
CFG_LIST = ["TRAIN.BATCH_SIZE", str(ROIS), "TRAIN.RPN_POST_NMS_TOP_N_TARGET", str(ROIS), "ANCHOR_SCALES", str(list(ANCHOR_SCALES)),
            "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30", "POOLING_MODE", "align"]

# id -> ic, gc, class_agnostic, target
CASES = {
    "plain": dict(ic=False, gc=False, agnostic=False, target=False),
    "context": dict(ic=True, gc=True, agnostic=False, target=False),
    "agnostic_ic": dict(ic=True, gc=False, agnostic=True, target=False),
    "target_plain": dict(ic=False, gc=False, agnostic=False, target=True),
    "target_context": dict(ic=True, gc=True, agnostic=False, target=True),
}

PLANTS = ("grl_pixel_sign_flipped",            # netD_pixel's reversal layer returns +eta g
          "grl_style_factor_dropped",          # netD_style's reversal layer returns -g
          "eta_swapped",                       # eta at netD_style, eta_style at netD_pixel
          "ic_context_not_detached",           # feat_instance computed from pooled_feat, not pooled_feat.detach()
          "gc_context_not_detached",           # feat_image computed from base_feat1, not base_feat1.detach()
          "context_filter_gradient_dropped",   # the context vectors carry no gradient into the discriminators' filters
          "rpn_cls_over_all_anchors",          # RPN cross entropy divided by the number of anchors, not of labelled anchors
          "rpn_box_sigma_1",                   # sigma 1 at the RPN smooth-L1 site
          "rpn_box_not_averaged",              # RPN box loss summed over the frames
          "bbox_gather_class_0",               # bbox_pred gathered at class 0 instead of the row's label
          "roi_align_gradient_missing",        # base_feat.grad without the RoIAlign contribution
          "rpn_gradient_missing",              # base_feat.grad without the RPN contribution
          "style_lambda_ignored",              # style terms weighted by 1
          "bias_lr_not_doubled",               # (optimiser) a bias steps with the plain rate
          "bias_decayed")                      # (optimiser) a bias decays like a filter
OPTIMISER_PLANTS = PLANTS[-2:]


def plant_applies(plant, case):
    """Whether the term ``plant`` breaks exists in ``case``."""
    c = CASES[case]
    if plant in ("ic_context_not_detached",):
        return c["ic"] and not c["target"]
    if plant in ("gc_context_not_detached",):
        return c["gc"] and not c["target"]
    if plant == "context_filter_gradient_dropped":
        return (c["ic"] or c["gc"]) and not c["target"]
    if plant in ("rpn_cls_over_all_anchors", "rpn_box_sigma_1", "rpn_box_not_averaged", "rpn_gradient_missing"):
        return not c["target"]
    if plant == "bbox_gather_class_0":
        return not c["target"] and not c["agnostic"]
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def feat_d(case):
    c = CASES[case]
    return 2048 + (512 if c["gc"] else 0) + (128 if c["ic"] else 0)


def make_params(case):
    """The float32 parameters of a case by the reference's state_dict keys: layer4 of a ResNet-50 (filters + raw BatchNorm buffers),
    the RPN, both discriminators, the two heads.  The discriminators' and the heads' filters are scaled up from their init so that
    every loss term, and the adversarial share of every gradient, is O(1) of its tensor."""
    c = CASES[case]
    p = {k: v for k, v in syn.backbone_params(1, 50, top=True).items() if k.startswith("RCNN_top.")}
    p.update(syn.rpn_params(10, std=0.02))
    p.update(syn.det_head_params(11, N_CLS, feat_d(case)))
    if c["agnostic"]:
        p["RCNN_bbox_pred.weight"], p["RCNN_bbox_pred.bias"] = p["RCNN_bbox_pred.weight"][:4].clone(), p["RCNN_bbox_pred.bias"][:4].clone()
    p.update(syn.netd_params(12))
    for k, s in (("netD_pixel.conv1.weight", 4.0), ("netD_pixel.conv2.weight", 4.0), ("netD_pixel.conv3.weight", 8.0),
                 ("RCNN_cls_score.weight", 4.0), ("RCNN_bbox_pred.weight", 10.0)):
        p[k] = p[k] * s
    return p


def make_inputs(seed=0):
    """Two post-ReLU maps (non-negative, half zeros, unit scale) and the ground truth of two frames: 3 and 1 boxes, zero padded.
    One 96 x 96 box per frame sits midway between four 96 px anchors (IoU 0.7245 with each: four foreground anchors at least);
    the two smaller boxes of frame 0 move with the seed."""
    g = torch.Generator().manual_seed(7000 + seed)
    feat = torch.relu(torch.randn(*FEAT, generator=g))
    feat1 = torch.relu(torch.randn(*FEAT1, generator=g))
    j = torch.randint(-3, 4, (4,), generator=g).tolist()
    mg = int(cfg.MAX_NUM_GT_BOXES)
    gt = np.zeros((B, mg, 5), np.float32)
    gt[0, 0] = (32, 16, 127, 111, 3)
    gt[0, 1] = (140 + j[0], 40 + j[1], 203 + j[0], 103 + j[1], 7)
    gt[0, 2] = (20 + j[2], 110 + j[3], 83 + j[2], 150 + j[3], 11)
    gt[1, 0] = (64, 32, 159, 127, 5)
    info = np.array([[IM_H, IM_W, 1.0]] * B, np.float32)
    return dict(feat=feat, feat1=feat1, gt=gt, num_boxes=np.array(N_GT, np.float32), info=info)


def roi_matrices(rois):
    """rois (B, R, 5) or (B*R, 5), frame-major -> per frame the float64 (R*49, H*W) matrix of the pinned RoIAlignAvg forward."""
    r = np.asarray(rois, np.float32).reshape(-1, 5)
    assert all((r[i * (len(r) // B):(i + 1) * (len(r) // B), 0] == i).all() for i in range(B)), "rois are frame-major"
    mats = roi_align_matrix(r, B, FEAT[2], FEAT[3], 7, 7, 1.0 / 16.0, cops.roi_align_avg_fwd)
    return [torch.from_numpy(m) for m in mats]


def host_samples(case, inputs, params, seed=0):
    """What the sampling layers give on the host: ``oracle.rpn``'s proposal layer on the float32 RPN head, then its anchor target and
    proposal target layers on a seeded ``RandomState`` (source), or the proposal layer's top ROIS boxes (target)."""
    T = cfg.TRAIN
    with torch.no_grad():
        cls, prob, box = nets.rpn_head(inputs["feat"], params)
    A = len(ANCHOR_SCALES) * len(ANCHOR_RATIOS)
    kw = dict(ratios=ANCHOR_RATIOS, scales=ANCHOR_SCALES)
    if CASES[case]["target"]:
        rois, _ = orpn.proposal_layer(prob[:, A:].numpy(), box.numpy(), inputs["info"], T.RPN_PRE_NMS_TOP_N, T.RPN_POST_NMS_TOP_N_TARGET,
                                      T.RPN_NMS_THRESH, **kw)
        return dict(rois=rois)
    rng = np.random.RandomState(100 + seed)
    H, W = FEAT[2:]
    L, Tg, IW, OW = orpn.anchor_target_layer(H, W, inputs["gt"], inputs["info"], rng, rpn_batch=T.RPN_BATCHSIZE, fg_frac=T.RPN_FG_FRACTION,
                                             pos_ov=T.RPN_POSITIVE_OVERLAP, neg_ov=T.RPN_NEGATIVE_OVERLAP, **kw)
    yxa = lambda t, k: t.transpose(0, 2, 3, 1).reshape(B, H * W * A, k)
    at = (L.reshape(B, A, H, W).transpose(0, 2, 3, 1).reshape(B, -1), yxa(Tg, 4), yxa(IW, 4)[..., 0], yxa(OW, 4)[..., 0])
    props, _ = orpn.proposal_layer(prob[:, A:].numpy(), box.numpy(), inputs["info"], T.RPN_PRE_NMS_TOP_N, T.RPN_POST_NMS_TOP_N, T.RPN_NMS_THRESH, **kw)
    norm = bool(T.BBOX_NORMALIZE_TARGETS_PRECOMPUTED)
    pt = orpn.proposal_target_layer(props, inputs["gt"], rng, batch_size=T.BATCH_SIZE, fg_fraction=T.FG_FRACTION, fg_thresh=T.FG_THRESH,
                                    bg_hi=T.BG_THRESH_HI, bg_lo=T.BG_THRESH_LO, means=T.BBOX_NORMALIZE_MEANS if norm else (0.0,) * 4,
                                    stds=T.BBOX_NORMALIZE_STDS if norm else (1.0,) * 4)
    return dict(anchor=at, proposal=pt, rois=pt[0])


def check_anchor_labels(labels):
    """Every frame holds labelled foreground (>= 4), labelled background and, inside the image, ignored anchors."""
    lab = np.asarray(labels).reshape(B, -1)
    inside = _inside_anchors()
    for b in range(B):
        assert (lab[b] == 1).sum() >= 4 and (lab[b] == 0).sum() >= 1, ((lab[b] == 1).sum(), (lab[b] == 0).sum())
        assert (lab[b][~inside] == -1).all()
    assert (lab[:, inside] == -1).sum() >= 1


def _inside_anchors():
    a = orpn.anchor_grid(FEAT[2], FEAT[3], 16, ANCHOR_RATIOS, ANCHOR_SCALES)
    return (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < IM_W) & (a[:, 3] < IM_H)


def top_blocks(p, dtype=torch.float32):
    """layer4 as ``bottleneck_ref`` block dicts, the BatchNorms folded in ``dtype`` (float32: FrozenBN.folded()'s own arithmetic)."""
    blocks = []
    for i in range(3):
        k = "RCNN_top.0.%d" % i
        b = dict(stride=2 if i == 0 else 1, w1=p[k + ".conv1.weight"], w2=p[k + ".conv2.weight"], w3=p[k + ".conv3.weight"],
                 wd=p.get(k + ".downsample.0.weight"), sd=None, bd=None)
        for n, bn in (("1", k + ".bn1"), ("2", k + ".bn2"), ("3", k + ".bn3")) + ((("d", k + ".downsample.1"),) if b["wd"] is not None else ()):
            raw = {q: p[bn + "." + q].to(dtype) for q in ("weight", "bias", "running_mean", "running_var")}
            b["s" + n], b["b" + n] = BR.fold(raw)
        blocks.append(b)
    return blocks


TOP_NAMES = {"w1": "conv1.weight", "w2": "conv2.weight", "w3": "conv3.weight", "wd": "downsample.0.weight"}


def build_case(case, max_seeds=16):
    """Inputs, parameters and host samples of ``case`` at the first seed at which the two conditions of ``run`` hold in float64 (the
    conditions involve no device result).  -> dict(inputs, params, blocks, samples, seed)."""
    params = make_params(case)
    blocks = top_blocks(params)
    for seed in range(max_seeds):
        inputs = make_inputs(seed)
        samples = host_samples(case, inputs, params, seed)
        if "anchor" in samples:
            check_anchor_labels(samples["anchor"][0])
        with torch.no_grad():
            out = run(case, inputs, params, blocks, samples, want_grad=False)
        if conditions_hold(out):
            return dict(inputs=inputs, params=params, blocks=blocks, samples=samples, seed=seed)
    raise AssertionError("case %r: the conditions hold at none of %d seeds: the case is wrong" % (case, max_seeds))


def conditions_hold(out):
    return out["margins"]["style_z"] >= Z_MARGIN and out["margins"]["smooth_l1"] >= SL1_MARGIN


# ---------------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------------
class _GRL(torch.autograd.Function):
    """utils/net_utils.py:52-61: identity forward, -lam g backward."""

    @staticmethod
    def forward(ctx, x, lam):
        ctx.lam = lam
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * -ctx.lam, None


def _relu(pre, mask):
    m = (pre.detach() > 0) if mask is None else mask
    return pre * m.to(pre.dtype), m


def _style(x, p, lam, sign, dim=512, rank=5):
    """netD_style.forward (:122-146) -> d (b, 1), the normalised z (b, dim), the pooled z before the root, its sign."""
    x = _GRL.apply(x, lam)
    b, c, h, w = x.shape
    x = x.reshape(b, c, -1).permute(0, 2, 1)
    x1 = F.linear(x, p["netD_style.fc_1.weight"], p["netD_style.fc_1.bias"])
    x2 = F.linear(x, p["netD_style.fc_2.weight"], p["netD_style.fc_2.bias"])
    z = (x1 * x2).reshape(b, h * w, dim, rank).sum(-1).sum(1)
    sign = (z.detach() > 0) if sign is None else sign
    s = sign.to(z.dtype) * 2 - 1
    root = s * torch.sqrt(z * s)                                        # sqrt(relu(z)) - sqrt(relu(-z)) with the side given
    zn = root / torch.linalg.vector_norm(root, dim=1, keepdim=True).clamp_min(1e-12)
    d = torch.sigmoid(F.linear(zn, p["netD_style.fc1.weight"], p["netD_style.fc1.bias"]))
    return d, zn, z.detach(), sign


def _pixel(x, p, lam, m1, m2):
    """netD_pixel.forward (:66-83) -> d (R, 1, 7, 7), the context mean (R, 128), the two pre-activations, the two masks."""
    x = _GRL.apply(x, lam)
    p1 = F.conv2d(x, p["netD_pixel.conv1.weight"])
    h1, m1 = _relu(p1, m1)
    p2 = F.conv2d(h1, p["netD_pixel.conv2.weight"])
    h2, m2 = _relu(p2, m2)
    d = torch.sigmoid(F.conv2d(h2, p["netD_pixel.conv3.weight"]))
    return d, h2.mean((2, 3)), (p1.detach(), p2.detach()), (m1, m2)


def _smooth_l1(pred, target, in_w, out_w, sigma, near):
    """utils/net_utils.py:122-136 before its sums -> (the weighted element losses, the side of the switch, the smallest relative
    distance of an argument from the switch)."""
    s2 = sigma ** 2
    d = in_w * (pred - target)
    ad = d.abs()
    if near is None:
        near = ad.detach() < 1.0 / s2
    n = near.to(d.dtype)
    loss = out_w * (d * d * (s2 / 2.0) * n + (ad - 0.5 / s2) * (1.0 - n))
    margin = float((ad.detach().double() - 1.0 / s2).abs().min() * s2)
    return loss, near, margin


def run(case, inputs, params, blocks, samples, masks=None, choices=None, dtype=torch.float64, plant=None, want_grad=True,
        reuse=None, dirty=(), context=None):
    """One evaluation in ``dtype``.
    inputs   dict(feat, feat1)                      the two maps
    params   {state_dict key: tensor}               RPN, discriminators, heads (layer4's filters are read from ``blocks``)
    blocks   bottleneck_ref block dicts of layer4   filters + folded (scale, shift)
    samples  dict(anchor=(labels, targets, inw, outw) in (y, x, a) order, proposal=(rois, labels, targets, inw, outw)) for a source
             case, dict(rois=...) for a target case
    masks    dict(rpn=, h1=, h2=, top=[(m1, m2, mo)] * 3) of booleans, any key missing or None: the reference's own ``pre > 0``
    choices  dict(style_sign=, near_rpn=, near_rcnn=) of an earlier run (a float32 run takes the float64 run's)
    reuse / dirty: stage outputs of an earlier run of the same case and the stages to compute again (central differences)
    context  dict(feat_instance=, feat_image=) held constant in place of the run's own context vectors (central differences along a
             map: what ``.detach()`` means to a derivative)
    -> dict(values, grads {name: tensor or None; 'base_feat', 'base_feat1' the two maps}, pre, masks, choices, margins, stages)."""
    if plant is not None and plant not in PLANTS:
        raise ValueError("unknown plant %r" % (plant,))
    c = CASES[case]
    masks, choices = dict(masks or {}), dict(choices or {})
    to = lambda t: torch.as_tensor(t).detach().to(dtype)
    feat, feat1 = to(inputs["feat"]), to(inputs["feat1"])
    p = {k: to(v) for k, v in params.items() if not k.startswith("RCNN_top.")}
    blk = [{k: (to(v) if torch.is_tensor(v) else v) for k, v in b.items()} for b in blocks]
    leaves = {"base_feat": feat, "base_feat1": feat1}
    leaves.update(p)
    for i, b in enumerate(blk):
        leaves.update({"RCNN_top.0.%d.%s" % (i, TOP_NAMES[n]): b[n] for n in BR.NAMES if b[n] is not None})
    if want_grad:
        for t in leaves.values():
            t.requires_grad_(True)
    stages = {}

    def stage(name, fn):
        if reuse is not None and name not in dirty:
            stages[name] = reuse[name]
        else:
            stages[name] = fn()
        return stages[name]

    eta, eta_style, lam = ETA, ETA_STYLE, STYLE_LAMBDA
    if plant == "eta_swapped":
        eta, eta_style = eta_style, eta
    if plant == "style_lambda_ignored":
        lam = 1.0
    grl_pixel = -eta if plant == "grl_pixel_sign_flipped" else eta
    grl_style = 1.0 if plant == "grl_style_factor_dropped" else eta_style
    values, pre, used, margins = {}, {}, {}, {}
    need_ctx = not c["target"]

    # ---- netD_style on the layer2 tap (faster_rcnn_instance_styleD_bilinear.py:66-71)
    def style():
        d, zn, z, sign = _style(feat1, p, grl_style, choices.get("style_sign"))
        ctx = None
        if c["gc"] and need_ctx:
            if plant == "gc_context_not_detached":
                ctx = zn
            elif torch.is_grad_enabled():
                ctx = _style(feat1.detach(), p, grl_style, sign)[1]
            else:
                ctx = zn
            if plant == "context_filter_gradient_dropped":
                ctx = ctx.detach()
        return d, ctx, z, sign
    d_style, feat_image, z, sign = stage("style", style)
    if context is not None and feat_image is not None:
        feat_image = context["feat_image"]
    choices["style_sign"] = sign
    rms = z.double().pow(2).mean(1, keepdim=True).sqrt()
    margins["style_z"] = float((z.double().abs() / rms).min())
    values["d_style"] = d_style

    # ---- the RPN head and its two losses (rpn/rpn.py:63-108)
    if not c["target"]:
        def rpn():
            x = feat.detach() if plant == "rpn_gradient_missing" else feat
            z1 = F.conv2d(x, p["RCNN_rpn.RPN_Conv.weight"], p["RCNN_rpn.RPN_Conv.bias"], padding=1)
            h, m = _relu(z1, masks.get("rpn"))
            cls = F.conv2d(h, p["RCNN_rpn.RPN_cls_score.weight"], p["RCNN_rpn.RPN_cls_score.bias"])
            box = F.conv2d(h, p["RCNN_rpn.RPN_bbox_pred.weight"], p["RCNN_rpn.RPN_bbox_pred.bias"])
            return cls, box, z1.detach(), m
        cls, box, pre["rpn"], used["rpn"] = stage("rpn", rpn)
        labels, tg, inw, outw = (torch.as_tensor(np.asarray(t)) for t in samples["anchor"])
        A = cls.shape[1] // 2
        cl = cls.permute(0, 2, 3, 1)
        pair = torch.stack((cl[..., :A], cl[..., A:]), -1).reshape(-1, 2)              # (bg, fg) per anchor, (y, x, a) order
        lab = labels.reshape(-1).long()
        keep = lab >= 0
        ce = F.cross_entropy(pair[keep], lab[keep], reduction="sum")
        values["rpn_cls"] = ce / (lab.numel() if plant == "rpn_cls_over_all_anchors" else int(keep.sum()))
        pred = box.permute(0, 2, 3, 1).reshape(B, -1, 4)
        el, choices["near_rpn"], m_rpn = _smooth_l1(pred, tg.to(dtype), inw.to(dtype).unsqueeze(2), outw.to(dtype).unsqueeze(2),
                                                    1.0 if plant == "rpn_box_sigma_1" else 3.0, choices.get("near_rpn"))
        per_frame = el.sum((1, 2))
        values["rpn_box"] = per_frame.sum() if plant == "rpn_box_not_averaged" else per_frame.mean()
    else:
        m_rpn = float("inf")

    # ---- RoIAlignAvg as a matrix product, netD_pixel on the pooled rows
    rois = np.asarray(samples["rois"], np.float32).reshape(-1, 5)
    mats = samples.get("_mats")
    if mats is None:
        mats = samples["_mats"] = roi_matrices(rois)

    def pool():
        x = feat.detach() if plant == "roi_align_gradient_missing" else feat
        rows = [m.to(dtype) @ x[b].reshape(FEAT[1], -1).t() for b, m in enumerate(mats)]             # (R*49, C) per frame
        return torch.cat(rows, 0).reshape(-1, 7, 7, FEAT[1]).permute(0, 3, 1, 2)
    pooled = stage("pool", pool)

    def pixel():
        d, ctx, pr, mk = _pixel(pooled, p, grl_pixel, masks.get("h1"), masks.get("h2"))
        if not (c["ic"] and need_ctx):
            ctx = None
        else:
            if plant != "ic_context_not_detached" and torch.is_grad_enabled():
                ctx = _pixel(pooled.detach(), p, grl_pixel, mk[0], mk[1])[1]
            if plant == "context_filter_gradient_dropped":
                ctx = ctx.detach()
        return d, ctx, pr, mk
    d_inst, feat_instance, (pre["h1"], pre["h2"]), (used["h1"], used["h2"]) = stage("pixel", pixel)
    values["d_instance"] = d_inst
    if context is not None and feat_instance is not None:
        feat_instance = context["feat_instance"]

    if c["target"]:
        values["dloss_t"] = 0.5 * ((1 - d_inst) ** 2).mean()
        values["dloss_t_style"] = 0.5 * ((1 - d_style) ** 2).mean()
        values["total"] = values["dloss_t"] + lam * values["dloss_t_style"]
        margins["smooth_l1"] = float("inf")
    else:
        # ---- layer4 + mean (_head_to_tail), the context columns, the two heads and their losses (:149-176)
        h, pre["top"], used["top"] = pooled, [], []
        for i in range(3):
            def top(i=i, h=h):
                o, pr, mk = BR.chain_forward(h, blk[i:i + 1], None if masks.get("top") is None else masks["top"][i:i + 1])
                return o, pr[0], mk[0]
            h, pr, mk = stage("top%d" % i, top)
            pre["top"].append(pr)
            used["top"].append(mk)
        _, plabels, ptg, pinw, poutw = (torch.as_tensor(np.asarray(t)) for t in samples["proposal"])
        plabels = plabels.reshape(-1).long()

        def head():
            x = h.mean(3).mean(2)
            if c["gc"]:
                x = torch.cat((feat_image.unsqueeze(1).repeat(1, x.shape[0] // B, 1).view(-1, feat_image.shape[1]), x), 1)
            if c["ic"]:
                x = torch.cat((feat_instance, x), 1)
            bp = F.linear(x, p["RCNN_bbox_pred.weight"], p["RCNN_bbox_pred.bias"])
            if not c["agnostic"]:
                idx = torch.zeros_like(plabels) if plant == "bbox_gather_class_0" else plabels
                bp = torch.gather(bp.view(bp.shape[0], -1, 4), 1, idx.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
            return bp, F.linear(x, p["RCNN_cls_score.weight"], p["RCNN_cls_score.bias"])
        bbox_pred, cls_score = stage("head", head)
        values["cls_prob"] = F.softmax(cls_score, 1).view(B, -1, cls_score.shape[1])
        values["bbox_pred"] = bbox_pred.view(B, -1, 4)
        values["rcnn_cls"] = F.cross_entropy(cls_score, plabels)
        el, choices["near_rcnn"], m_rcnn = _smooth_l1(bbox_pred, ptg.reshape(-1, 4).to(dtype), pinw.reshape(-1, 4).to(dtype),
                                                      poutw.reshape(-1, 4).to(dtype), 1.0, choices.get("near_rcnn"))
        values["rcnn_box"] = el.sum(1).mean()
        values["dloss_s"] = 0.5 * (d_inst ** 2).mean()
        values["dloss_s_style"] = 0.5 * (d_style ** 2).mean()
        values["total"] = (values["rpn_cls"] + values["rpn_box"] + values["rcnn_cls"] + values["rcnn_box"] + values["dloss_s"] +
                           lam * values["dloss_s_style"])
        margins["smooth_l1"] = min(m_rpn, m_rcnn)

    grads = None
    if want_grad:
        names = list(leaves)
        got = torch.autograd.grad(values["total"], [leaves[n] for n in names], allow_unused=True)
        grads = dict(zip(names, got))
    ctx = dict(feat_instance=None if feat_instance is None else feat_instance.detach(),
               feat_image=None if feat_image is None else feat_image.detach())
    return dict(values={k: v.detach() for k, v in values.items()}, grads=grads, pre=pre, masks=used, choices=choices, margins=margins,
                stages=stages, context=ctx)


# the stages a tensor's value reaches (central differences recompute only these)
def dirty_stages(name):
    if name == "base_feat":
        return ("rpn", "pool", "pixel", "top0", "top1", "top2", "head")
    if name == "base_feat1" or name.startswith("netD_style."):
        return ("style", "head")
    if name.startswith("RCNN_rpn."):
        return ("rpn",)
    if name.startswith("netD_pixel."):
        return ("pixel", "head")
    if name.startswith("RCNN_top.0."):
        return tuple("top%d" % i for i in range(int(name.split(".")[2]), 3)) + ("head",)
    return ("head",)


# ---------------------------------------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------------------------------------
def group_of(name, lr, plant=None):
    """(lr, weight decay) of the reference's param groups (trainval_net_instance_styleD_bilinear.py:134-148)."""
    T = cfg.TRAIN
    if "bias" in name:
        return (lr * ((T.DOUBLE_BIAS + 1) if plant != "bias_lr_not_doubled" else 1),
                T.WEIGHT_DECAY if (T.BIAS_DECAY or plant == "bias_decayed") else 0.0)
    return lr, T.WEIGHT_DECAY


def sgd(p0, g, m0, lr, plant=None):
    """torch.optim.SGD's rule in float64: m1 = mu m0 + g + wd p0, p1 = p0 - lr m1, for every name of ``g`` that has a gradient."""
    mu = cfg.TRAIN.MOMENTUM
    m1, p1 = {}, {}
    for k, gk in g.items():
        if gk is None or k not in p0:
            continue
        lr_k, wd_k = group_of(k, lr, plant)
        p = p0[k].detach().double()
        m1[k] = mu * m0[k].detach().double() + gk.double() + wd_k * p
        p1[k] = p - lr_k * m1[k]
    return m1, p1


def momentum_like(g, seed=5):
    """float32 momentum buffers at the scale of the gradients: N(0, 1) x max|g_k|."""
    gen = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=gen, dtype=torch.float32) * float(v.abs().max()) for k, v in g.items() if v is not None}


# ---------------------------------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------------------------------
def rel_max(got, want):
    """max |got - want| over max |want|, in float64."""
    want = torch.as_tensor(want).detach().double().cpu()
    got = torch.as_tensor(got).detach().double().cpu().reshape(want.shape)
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def gpu_bound(e32):
    """The bound a device tensor is held to, from the float32 CPU reference's own error ``e32`` under the same masks."""
    return min(1e-4, max(16.0 * e32, 1e-6))


def e32_table(case, inputs, params, blocks, samples, ref64):
    """The reference in float32 under the float64 run's masks and choices -> {tensor name: its error relative to the float64
    tensor's largest element}, values and gradients alike."""
    r32 = run(case, inputs, params, blocks, samples, masks=ref64["masks"], choices=ref64["choices"], dtype=torch.float32)
    out = {k: rel_max(r32["values"][k], v) for k, v in ref64["values"].items()}
    out.update({k: rel_max(r32["grads"][k], v) for k, v in ref64["grads"].items() if v is not None})
    return out
