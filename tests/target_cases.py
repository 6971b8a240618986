"""Built cases for the target-assignment path -- i2v_bbox_overlaps (csrc/rpn.hip), i2v_bbox_transform (csrc/heads.hip) and the two
layers on top of them, _AnchorTargetLayer and _ProposalTargetLayer -- shared by the host test, the GPU test and the golden
generator, plus a plain statement of the rules the cases are designed with.  Every decision of this path compares an fp32 IoU
with a constant or with another IoU; the cases put IoUs ON those constants, one pixel row to either side, and on each other.
Which side a pair falls on and which regime a scene lands in is decided here and asserted on the CPU
(tests/test_target_cases_host.py); the GPU test only compares with the oracle.  Seeded numpy only; nothing here imports the
package, torch or the oracle.

Boxes of the decision cases have integer pixel corners and areas below 2^24: every difference, product and sum of the IoU is
exact in fp32 and the quotient's rounding is the only one.  Two statements of the rules live here:

  exact_*   integer cross-multiplication (I * q against p * U) and fractions.Fraction: no rounding at all
  plain_*   float64 arithmetic with one fp32 rounding after every operation (for + - * / a float64 result rounded to fp32 IS
            the correctly rounded fp32 result: 53 >= 2 * 24 + 2), first-index argmax, the reference's fill order; ``variant``
            selects one deliberately wrong form, which the host test must be able to tell from the right one
"""
import collections
import fractions

import numpy as np

F32 = np.float32
Fr = fractions.Fraction

# every constant either layer compares an IoU with: RPN_POSITIVE_OVERLAP, RPN_NEGATIVE_OVERLAP, FG_THRESH = BG_THRESH_HI, the
# default BG_THRESH_LO, the yml's BG_THRESH_LO
CONSTANTS = collections.OrderedDict([("0.7", Fr(7, 10)), ("0.3", Fr(3, 10)), ("0.5", Fr(1, 2)), ("0.1", Fr(1, 10)), ("0.0", Fr(0))])
VARIANTS = ("strict_ge", "last_argmax", "fill_swapped", "fused")
IM_H, IM_W, FEAT_H, FEAT_W = 600, 1000, 38, 63

OvCase = collections.namedtuple("OvCase", "name boxes gt prop")          # boxes (N,4) | (B,N,4) | (B,N,5); gt (B,K,5)
TfCase = collections.namedtuple("TfCase", "name ex gt prop")             # ex (N,4) | (B,N,4); gt (B,N,4|5)
AnchorScene = collections.namedtuple("AnchorScene", "name gt im_info feat prop")
ProposalScene = collections.namedtuple("ProposalScene", "name rois gt prop")


# ----------------------------------------------------------------------------------------------------------- anchors
def base_anchors():
    """The nine base anchors of ratios (0.5, 1, 2) x scales (8, 16, 32) on a 16-pixel cell, ratio-major: sides 23x12, 16x16,
    11x22 times the scale, centred on 7.5."""
    rows = []
    for w, h in ((23, 12), (16, 16), (11, 22)):
        for s in (8, 16, 32):
            hw, hh = (w * s - 1) / 2.0, (h * s - 1) / 2.0
            rows.append([7.5 - hw, 7.5 - hh, 7.5 + hw, 7.5 + hh])
    return np.array(rows, F32)


def anchor_grid(feat_h=FEAT_H, feat_w=FEAT_W, stride=16):
    """(feat_h * feat_w * 9, 4) in (y, x, a) order."""
    ys, xs = np.meshgrid(np.arange(feat_h) * stride, np.arange(feat_w) * stride, indexing="ij")
    shift = np.stack([xs, ys, xs, ys], -1).reshape(-1, 1, 4).astype(F32)
    return (shift + base_anchors()[None]).reshape(-1, 4)


def anchor_index(cy, cx, a, feat_w=FEAT_W):
    return (cy * feat_w + cx) * 9 + a


def inside_mask(anchors, im_h, im_w):
    return (anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < im_w) & (anchors[:, 3] < im_h)


# ----------------------------------------------------------------------------------------------------------- exact rules
def iou_fraction(box, gt):
    """The IoU of one pair as a Fraction under the reference's rules: +1 extents, a unit (1x1) gt -> 0, a unit box -> -1 (last)."""
    b = [Fr(float(v)) for v in box[:4]]
    g = [Fr(float(v)) for v in gt[:4]]
    bw, bh, gw, gh = b[2] - b[0] + 1, b[3] - b[1] + 1, g[2] - g[0] + 1, g[3] - g[1] + 1
    if bw == 1 and bh == 1:
        return Fr(-1)
    if gw == 1 and gh == 1:
        return Fr(0)
    iw = max(Fr(0), min(b[2], g[2]) - max(b[0], g[0]) + 1)
    ih = max(Fr(0), min(b[3], g[3]) - max(b[1], g[1]) + 1)
    return iw * ih / (bw * bh + gw * gh - iw * ih)


def exact_iu(boxes, gt):
    """Integer boxes (N,4) against (K,>=4): intersection and union as int64 (N,K) and the two unit-box masks."""
    b = np.asarray(boxes, np.float64)[:, :4]
    g = np.asarray(gt, np.float64)[:, :4]
    assert np.array_equal(b, np.round(b)) and np.array_equal(g, np.round(g)), "exact_iu: integer corners only"
    b, g = b.astype(np.int64), g.astype(np.int64)
    bw, bh = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    gw, gh = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
    assert (bw > 0).all() and (bh > 0).all() and (gw > 0).all() and (gh > 0).all()
    assert (bw * bh).max(initial=0) < 2 ** 24 and (gw * gh).max(initial=0) < 2 ** 24, "areas must be exact in fp32"
    iw = np.maximum(0, np.minimum(b[:, None, 2], g[None, :, 2]) - np.maximum(b[:, None, 0], g[None, :, 0]) + 1)
    ih = np.maximum(0, np.minimum(b[:, None, 3], g[None, :, 3]) - np.maximum(b[:, None, 1], g[None, :, 1]) + 1)
    inter = iw * ih
    union = (bw * bh)[:, None] + (gw * gh)[None, :] - inter
    return inter, union, (bw == 1) & (bh == 1), (gw == 1) & (gh == 1)


def exact_sign(iu, c):
    """sign(IoU - c) for every pair, c a Fraction >= 0, without a division: I q - p U, with the fills 0 and -1 applied in the
    reference's order."""
    inter, union, bzero, gzero = iu
    p, q = c.numerator, c.denominator
    num = inter * q - p * union
    num = np.where(gzero[None, :], -p, num)
    num = np.where(bzero[:, None], -q - p, num)
    return np.sign(num)


def exact_values(iu):
    """The IoUs as float64 with the fills applied.  I and U are below 2^25, so two different rationals differ by more than
    2^-50 and stay different in float64, and equal rationals give equal float64s: order and ties are those of the rationals."""
    inter, union, bzero, gzero = iu
    v = inter.astype(np.float64) / union.astype(np.float64)
    v = np.where(gzero[None, :], 0.0, v)
    return np.where(bzero[:, None], -1.0, v)


def exact_anchor_labels(anchors, gt, pos=Fr(7, 10), neg=Fr(3, 10)):
    """Labels of the inside anchors of one image before any subsampling (anchor_target_layer.py:100-113): background below
    ``neg``, then foreground for every anchor that ties for a gt box's best IoU (a best of 0 counts as 1e-5: nobody), then
    foreground at or above ``pos``.  Returns (labels int8, first argmax)."""
    iu = exact_iu(anchors, gt)
    v = exact_values(iu)
    lab = np.full(v.shape[0], -1, np.int8)
    lab[(exact_sign(iu, neg) < 0).all(1)] = 0
    gmax = v.max(0)
    gmax = np.where(gmax == 0, 1e-5, gmax)
    lab[(v == gmax[None, :]).any(1)] = 1
    lab[(exact_sign(iu, pos) >= 0).any(1)] = 1
    return lab, v.argmax(1)


def exact_proposal_classes(rois, gt, lo, fg=Fr(1, 2), hi=Fr(1, 2)):
    """(foreground mask, background mask, first argmax) of one image's candidate rois (proposal_target_layer_cascade.py:142-147):
    fg at or above ``fg``; bg below ``hi`` and at or above ``lo``."""
    iu = exact_iu(rois, gt)
    is_fg = (exact_sign(iu, fg) >= 0).any(1)
    is_bg = (exact_sign(iu, hi) < 0).all(1) & (exact_sign(iu, lo) >= 0).any(1)
    return is_fg, is_bg, exact_values(iu).argmax(1)


# ----------------------------------------------------------------------------------------------------------- plain rules
def _r(x):
    """One fp32 rounding of a float64 result."""
    return np.asarray(x, np.float64).astype(F32).astype(np.float64)


def plain_overlaps(boxes, gt, variant=None):
    """bbox_overlaps_batch for one image (bbox_transform.py:168-213): boxes (N,4), gt (K,>=4) -> (ov (N,K), max (N,), argmax (N,))
    in fp32.  variant "fused": the union takes iw * ih unrounded, as a contracted multiply-subtract would; "fill_swapped": the
    -1 fill before the 0 fill; "last_argmax": the last of tied maxima."""
    b = np.asarray(boxes, F32).astype(np.float64)[:, :4]
    g = np.asarray(gt, F32).astype(np.float64)[:, :4]
    bw, bh = _r(_r(b[:, 2] - b[:, 0]) + 1), _r(_r(b[:, 3] - b[:, 1]) + 1)
    gw, gh = _r(_r(g[:, 2] - g[:, 0]) + 1), _r(_r(g[:, 3] - g[:, 1]) + 1)
    barea, garea = _r(bw * bh)[:, None], _r(gw * gh)[None, :]
    iw = _r(_r(np.minimum(b[:, None, 2], g[None, :, 2]) - np.maximum(b[:, None, 0], g[None, :, 0])) + 1)
    ih = _r(_r(np.minimum(b[:, None, 3], g[None, :, 3]) - np.maximum(b[:, None, 1], g[None, :, 1])) + 1)
    iw, ih = np.where(iw < 0, 0.0, iw), np.where(ih < 0, 0.0, ih)
    inter = _r(iw * ih)
    ua = _r(_r(barea + garea) - (iw * ih if variant == "fused" else inter))
    with np.errstate(all="ignore"):
        ov = _r(inter / ua)
    bzero, gzero = ((bw == 1) & (bh == 1))[:, None], ((gw == 1) & (gh == 1))[None, :]
    if variant == "fill_swapped":
        ov = np.where(gzero, 0.0, np.where(bzero, -1.0, ov))
    else:
        ov = np.where(bzero, -1.0, np.where(gzero, 0.0, ov))
    ov = ov.astype(F32)
    mx = ov.max(1)
    if variant == "last_argmax":
        am = ov.shape[1] - 1 - ov[:, ::-1].argmax(1)
    else:
        am = ov.argmax(1)
    return ov, mx, am.astype(np.int32)


def _ge(a, c, variant):
    return a > c if variant == "strict_ge" else a >= c


def plain_anchor_labels(anchors, gt, variant=None, pos=0.7, neg=0.3):
    """exact_anchor_labels in the reference's arithmetic: fp32 IoUs compared with the python constants."""
    ov, mx, am = plain_overlaps(anchors, gt, variant)
    lab = np.full(ov.shape[0], -1, np.int8)
    lab[mx < neg] = 0
    gmax = ov.max(0)
    gmax = np.where(gmax == 0, F32(1e-5), gmax)
    lab[(ov == gmax[None, :]).any(1)] = 1
    lab[_ge(mx, pos, variant)] = 1
    return lab, am


def plain_proposal_classes(rois, gt, lo, variant=None, fg=0.5, hi=0.5):
    ov, mx, am = plain_overlaps(rois, gt, variant)
    return _ge(mx, fg, variant), (mx < hi) & _ge(mx, lo, variant), am


def plain_box_targets(ex, gt):
    """bbox_transform_batch (bbox_transform.py:36-75) evaluated in float64 on the fp32 inputs: (N,4) float64."""
    e = np.asarray(ex, F32).astype(np.float64)
    g = np.asarray(gt, F32).astype(np.float64)[..., :4]
    ew, eh = e[..., 2] - e[..., 0] + 1, e[..., 3] - e[..., 1] + 1
    gw, gh = g[..., 2] - g[..., 0] + 1, g[..., 3] - g[..., 1] + 1
    ecx, ecy, gcx, gcy = e[..., 0] + 0.5 * ew, e[..., 1] + 0.5 * eh, g[..., 0] + 0.5 * gw, g[..., 1] + 0.5 * gh
    return np.stack([(gcx - ecx) / ew, (gcy - ecy) / eh, np.log(gw / ew), np.log(gh / eh)], -1)


def plain_log_targets(ex, gt):
    """What dw and dh are held to: the float64 log of the fp32 quotient (extents and quotient rounded to fp32 once per
    operation, as any fp32 implementation has them): (..., 2) float64."""
    e = np.asarray(ex, F32).astype(np.float64)
    g = np.asarray(gt, F32).astype(np.float64)[..., :4]
    ew, eh = _r(_r(e[..., 2] - e[..., 0]) + 1), _r(_r(e[..., 3] - e[..., 1]) + 1)
    gw, gh = _r(_r(g[..., 2] - g[..., 0]) + 1), _r(_r(g[..., 3] - g[..., 1]) + 1)
    return np.stack([np.log(_r(gw / ew)), np.log(_r(gh / eh))], -1)


def ulp_error(got, want64):
    """|got - want| in units of the fp32 spacing at want (the spacing of the smallest normal number where want is 0)."""
    want64 = np.asarray(want64, np.float64)
    sp = np.spacing(np.maximum(np.abs(want64), np.finfo(F32).tiny).astype(F32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / sp


def numpy_log_ulp(cases=None):
    """The worst error, in ulp, of numpy's fp32 log of the fp32 quotient against plain_log_targets over the transform cases:
    the reference's own error on them (torch-CPU and numpy both call an fp32 log)."""
    worst = 0.0
    for c in cases or transform_cases():
        ex = np.broadcast_to(c.ex if c.ex.ndim == 3 else c.ex[None], c.gt.shape[:2] + (4,))
        e, g = np.asarray(ex, F32), np.asarray(c.gt, F32)
        ew, eh = e[..., 2] - e[..., 0] + F32(1), e[..., 3] - e[..., 1] + F32(1)
        gw, gh = g[..., 2] - g[..., 0] + F32(1), g[..., 3] - g[..., 1] + F32(1)
        got = np.stack([np.log(gw / ew), np.log(gh / eh)], -1)
        assert got.dtype == F32
        worst = max(worst, float(ulp_error(got, plain_log_targets(ex, c.gt)).max()))
    return worst


def dxdy_bound(ex, gt):
    """Absolute bound (..., 2) on an fp32 evaluation of dx and dy, one rounding per operation, against plain_box_targets.  With
    u = 2^-24: each extent carries 2u (a difference and a +1), each centre u of itself plus that of half its extent, the
    difference of the centres u of itself, and the quotient the extent's 2u and its own u -- so the error is within
    u ((ew + gw + |ecx| + |gcx|) / ew + 4 |dx|); the bound is twice that."""
    e = np.asarray(ex, F32).astype(np.float64)
    g = np.asarray(gt, F32).astype(np.float64)[..., :4]
    t = plain_box_targets(ex, gt)
    out = []
    for a, k in ((0, 0), (1, 1)):
        ew, gw = e[..., a + 2] - e[..., a] + 1, g[..., a + 2] - g[..., a] + 1
        ecx, gcx = e[..., a] + 0.5 * ew, g[..., a] + 0.5 * gw
        out.append(2.0 ** -23 * ((ew + gw + np.abs(ecx) + np.abs(gcx)) / ew + 4 * np.abs(t[..., k])))
    return np.stack(out, -1)


def log_ulp_of(got, ex, gt, means=None, stds=None):
    """The worst error, in ulp, of got[..., 2:4] against plain_log_targets -- normalised in float64 with the fp32 means / stds
    when they are given."""
    want = plain_log_targets(ex, gt)
    if means is not None:
        want = (want - np.asarray(means, F32).astype(np.float64)[2:]) / np.asarray(stds, F32).astype(np.float64)[2:]
    return float(ulp_error(np.asarray(got)[..., 2:4], want).max())


def normalised_bound(log_ulp):
    """The bound, in ulp, on a normalised dw / dh, (t - mean) / std, given ``log_ulp`` on t: the subtraction and the division
    round once each (half an ulp each) and the quotient may land in a binade whose ulp is relatively half as large."""
    return 2.0 * log_ulp + 1.0


def plain_proposal_target(rois, gt, rng, R, lo, fg_fraction=0.25, means=(0.0, 0.0, 0.0, 0.0), stds=(0.1, 0.1, 0.2, 0.2)):
    """_ProposalTargetLayer.forward (proposal_target_layer_cascade.py:33-56, 116-212) from plain_overlaps and
    plain_box_targets, with numpy's legacy generator in the reference's call order.  rois (B,P,5), gt (B,G,5) -> rois (B,R,5),
    labels (B,R), targets float64 (B,R,4), inside-w, outside-w (B,R,4) and the kept indices into the P + G candidates and n_fg
    per image.  Raises ValueError on an image that has neither class."""
    rois, gt = np.asarray(rois, F32), np.asarray(gt, F32)
    B, G = gt.shape[:2]
    app = np.zeros_like(gt)
    app[:, :, 1:5] = gt[:, :, :4]
    cand = np.concatenate([rois, app], 1)
    fg_per = int(np.round(fg_fraction * R)) or 1
    out_rois, out_lab, out_tg = np.zeros((B, R, 5), F32), np.zeros((B, R), F32), np.zeros((B, R, 4), np.float64)
    keeps, nfgs = [], []
    for b in range(B):
        fg, bg, assign = plain_proposal_classes(cand[b, :, 1:5], gt[b], lo)
        fg, bg = np.nonzero(fg)[0], np.nonzero(bg)[0]
        if fg.size and bg.size:
            nfg = min(fg_per, fg.size)
            fg = fg[rng.permutation(fg.size)[:nfg]]
            bg = bg[np.floor(rng.rand(R - nfg) * bg.size).astype(np.int64)]
        elif fg.size:
            fg, bg, nfg = fg[np.floor(rng.rand(R) * fg.size).astype(np.int64)], bg[:0], R
        elif bg.size:
            bg, fg, nfg = bg[np.floor(rng.rand(R) * bg.size).astype(np.int64)], fg[:0], 0
        else:
            raise ValueError("image %d has neither foreground nor background rois" % b)
        keep = np.concatenate([fg, bg])
        keeps.append(keep)
        nfgs.append(nfg)
        out_rois[b] = cand[b, keep]
        out_rois[b, :, 0] = b
        out_lab[b] = gt[b, assign[keep], 4]
        out_lab[b, nfg:] = 0
        tg = plain_box_targets(cand[b, keep, 1:5], gt[b, assign[keep], :4])
        tg = (tg - np.asarray(means, F32).astype(np.float64)) / np.asarray(stds, F32).astype(np.float64)
        out_tg[b] = np.where(out_lab[b, :, None] > 0, tg, 0.0)
    inw = np.repeat((out_lab > 0)[:, :, None], 4, 2).astype(F32)
    return out_rois, out_lab, out_tg, inw, inw.copy(), np.stack(keeps), np.asarray(nfgs)


# ----------------------------------------------------------------------------------------------------------- overlap cases
def partial_gt_for(box, c):
    """Integer search: a gt box as wide as ``box`` that shares its lowest ih rows and reaches below it (it overlaps the box only
    partly), with IoU = ih / (ah + gh - ih) equal to the Fraction ``c``; the smallest ih.  Returns (gt, ih, gh)."""
    x1, y1, x2, y2 = (int(v) for v in box)
    ah = y2 - y1 + 1
    for ih in range(1, ah):
        for gh in range(ih + 1, 4 * ah):
            if Fr(ih, ah + gh - ih) == c:
                return [x1, y2 - ih + 1, x2, y2 - ih + gh], ih, gh
    raise AssertionError("no partial gt for %r at %s" % (box, c))


THRESHOLD_ANCHORS = ((18, 30, 3), (18, 30, 0))      # (cy, cx, a): a 128x128 and a 184x96 anchor in the middle of the 38x63 grid


def threshold_pairs():
    """[(constant key, side, family, box, gt)]: for every constant a pair whose rational IoU equals it ("at"), one pixel row to
    the low side and one to the high side.  Family "nested": [100,100,199,y] inside [100,100,199,199]; family "anchor<a>": a
    real inside anchor of the 38x63 grid against the gt partial_gt_for finds (the anchor's sides are multiples of 8 with no
    factor 5, so no box nested in it has a tenth of its area ratio).  For 0.0 the pairs touch: the gt starts on the row below
    the box ("at", IoU exactly 0), overlaps its last row ("high") or leaves a row free ("low": still 0 -- only a unit box goes
    lower, see zero_area_case)."""
    grid = anchor_grid()
    anchors = [("anchor%d" % a, [int(v) for v in grid[anchor_index(cy, cx, a)]]) for cy, cx, a in THRESHOLD_ANCHORS]
    out = []
    for key, c in CONSTANTS.items():
        if c == 0:
            for fam, box in [("nested", [100, 100, 199, 199])] + anchors:
                h = box[3] - box[1] + 1
                for side, d in (("at", 1), ("low", 2), ("high", 0)):
                    out.append((key, side, fam, box, [box[0], box[3] + d, box[2], box[3] + d + h - 1]))
            continue
        rows = int(100 * c)
        assert Fr(rows, 100) == c
        for side, d in (("at", 0), ("low", -1), ("high", 1)):
            out.append((key, side, "nested", [100, 100, 199, 100 + rows + d - 1], [100, 100, 199, 199]))
        for fam, box in anchors:
            gt, _, _ = partial_gt_for(box, c)
            for side, d in (("at", 0), ("low", 1), ("high", -1)):
                out.append((key, side, fam, box, [gt[0], gt[1] + d, gt[2], gt[3] + d]))
    return out


def threshold_case():
    """All threshold pairs in one call: row i against column i is pair i (the other entries are whatever they are)."""
    pairs = threshold_pairs()
    boxes = np.array([p[3] for p in pairs], F32)
    gt = np.zeros((1, len(pairs), 5), F32)
    gt[0, :, :4] = [p[4] for p in pairs]
    gt[0, :, 4] = 1 + np.arange(len(pairs)) % 15
    return OvCase("thresholds", boxes, gt, {"pairs": [(i, p[0], p[1], p[2]) for i, p in enumerate(pairs)]})


def zero_area_case():
    """Unit boxes on both sides.  gt: a normal box, a zero padding row, a real unit box [120,130,120,130], a normal box.
    rois: normal, unit, unit ON the unit gt, a normal roi that covers the unit gt, a zero padding roi, a roi disjoint from all."""
    gt = np.zeros((1, 4, 5), F32)
    gt[0] = [[100, 100, 199, 199, 3], [0, 0, 0, 0, 0], [120, 130, 120, 130, 5], [300, 120, 420, 260, 7]]
    boxes = np.array([[110, 90, 210, 180], [50, 50, 50, 50], [120, 130, 120, 130], [90, 100, 150, 160], [0, 0, 0, 0],
                      [600, 400, 700, 500]], F32)
    prop = {"zero_cols": [1, 2], "minus_rows": [1, 2, 4], "all_zero_rows": [5]}
    return OvCase("zero_area", boxes, gt, prop)


def tie_case():
    """gt: G, G again with another class, H1, H2 (same size, 100 apart).  rois: G itself (ties columns 0 and 1 at IoU 1), a roi
    disjoint from every box (all 0), a roi that overlaps H1 and H2 by the same 50 columns (ties columns 2 and 3 at 1/5)."""
    gt = np.zeros((1, 4, 5), F32)
    gt[0] = [[40, 300, 139, 449, 2], [40, 300, 139, 449, 9], [300, 100, 399, 199, 4], [500, 100, 599, 199, 6]]
    boxes = np.array([[40, 300, 139, 449], [700, 400, 800, 550], [350, 100, 549, 199]], F32)
    return OvCase("ties", boxes, gt, {"argmax": [0, 0, 2], "tied": [(0, 1), (0, 1, 2, 3), (2, 3)], "value": [Fr(1), Fr(0), Fr(1, 5)]})


def fractional_case(seed=11):
    """257 rois against 20 boxes with fractional fp32 corners: iw * ih and the areas are NOT exact here, so an implementation
    that contracts the union's multiply-subtract differs in the last bit of some IoUs."""
    rng = np.random.default_rng(seed)

    def boxes(n):
        x1, y1 = rng.uniform(0, 700, n), rng.uniform(0, 400, n)
        return np.stack([x1, y1, x1 + rng.uniform(20, 300, n), y1 + rng.uniform(20, 200, n)], 1).astype(F32)
    gt = np.zeros((1, 20, 5), F32)
    gt[0, :, :4] = boxes(20)
    gt[0, :, 4] = 1 + np.arange(20) % 15
    return OvCase("fractional", boxes(257), gt, {})


SHAPE_K = (1, 20, 30, 64, 1024)        # 1024: the documented cap of i2v_bbox_overlaps
SHAPE_N = (1, 255, 256, 257, 513)      # around the 256-thread block
SHAPE_B = (1, 3)
SHAPE_FORMS = ("shared", "b4", "b5")   # (N,4) for every image; (B,N,4); (B,N,5) with the image index in column 0
K_OVER_CAP = 1025


def shape_case(B, N, K, form, seed=0):
    """Random integer boxes, with the things a real call has planted in: the last quarter of the gt rows zero padding (when
    K >= 4), gt row 1 a duplicate of row 0, roi 0 equal to gt 0 of image 0, the last roi a unit box."""
    rng = np.random.default_rng([seed, B, N, K, SHAPE_FORMS.index(form)])

    def boxes(shape):
        x1, y1 = rng.integers(0, 800, shape), rng.integers(0, 450, shape)
        return np.stack([x1, y1, x1 + rng.integers(8, 200, shape), y1 + rng.integers(8, 150, shape)], -1).astype(F32)
    gt = np.zeros((B, K, 5), F32)
    gt[:, :, :4] = boxes((B, K))
    gt[:, :, 4] = 1 + rng.integers(0, 15, (B, K))
    if K >= 2:
        gt[:, 1, :4] = gt[:, 0, :4]
    if K >= 4:
        gt[:, K - K // 4:] = 0
    bx = boxes((N,) if form == "shared" else (B, N))
    bx[..., 0, :] = gt[0, 0, :4]
    if N > 1:
        bx[..., N - 1, :] = [33, 44, 33, 44]
    if form == "b5":
        bx = np.concatenate([np.broadcast_to(np.arange(B, dtype=F32)[:, None, None], (B, N, 1)), bx], 2)
    return OvCase("B%d_N%d_K%d_%s" % (B, N, K, form), np.ascontiguousarray(bx, F32), gt, {})


def case_images(case):
    """[(boxes (N,4), gt (K,5))] per image of an overlap case, whatever form its boxes have."""
    out = []
    for b in range(case.gt.shape[0]):
        bx = case.boxes if case.boxes.ndim == 2 else case.boxes[b]
        out.append((bx[:, -4:], case.gt[b]))
    return out


def edge_overlap_cases():
    return [threshold_case(), zero_area_case(), tie_case(), fractional_case()]


# ----------------------------------------------------------------------------------------------------------- transform cases
def transform_cases(seed=21):
    """ex / gt pairs for bbox_transform.  "mixed": B = 2, N = 300, ex batched (B,N,4), gt with row stride 5; random integer and
    fractional rois, and planted at the head of every image: gt == roi (target exactly 0), a unit gt, a gt one pixel wide, a
    unit roi, a roi one pixel wide, rois on the clip border of a 600x1000 image.  "shared": the same gt rows with stride 4
    against ONE (N,4) set of rois."""
    rng = np.random.default_rng(seed)
    B, N = 2, 300

    def boxes(n, frac):
        x1, y1 = rng.uniform(0, 800, n), rng.uniform(0, 450, n)
        b = np.stack([x1, y1, x1 + rng.uniform(4, 199, n), y1 + rng.uniform(4, 149, n)], 1)
        return (b if frac else np.round(b)).astype(F32)
    ex = np.stack([np.concatenate([boxes(N // 2, False), boxes(N - N // 2, True)]) for _ in range(B)])
    gt = np.zeros((B, N, 5), F32)
    for b in range(B):
        gt[b, :, :4] = np.concatenate([boxes(N // 2, False), boxes(N - N // 2, True)])
        gt[b, :, 4] = 1 + np.arange(N) % 15
    planted = [([100, 100, 199, 199], [100, 100, 199, 199]),            # 0 gt == roi
               ([100.25, 50.5, 180.75, 90.125], [100.25, 50.5, 180.75, 90.125]),
               ([100, 100, 199, 199], [150, 150, 150, 150]),            # 2 unit gt
               ([0, 0, 0, 0], [0, 0, 0, 0]),                            # 3 padding on padding: also exactly 0
               ([100, 100, 199, 199], [140, 80, 140, 260]),             # 4 gt one pixel wide
               ([60, 70, 60, 70], [40, 50, 90, 120]),                   # 5 unit roi
               ([60, 70, 60, 170], [40, 50, 90, 120]),                  # 6 roi one pixel wide
               ([0, 0, 120, 80], [10, 5, 100, 90]),                     # 7.. rois on the clip border
               ([900, 500, 999, 599], [880, 480, 990, 590]),
               ([0, 0, 999, 599], [300, 200, 420, 330])]
    for b in range(B):
        for i, (e, g) in enumerate(planted):
            ex[b, i], gt[b, i, :4] = e, g
    prop = {"zero_rows": [0, 1, 3], "planted": len(planted)}
    return [TfCase("mixed", ex, gt, prop),
            TfCase("shared", np.ascontiguousarray(ex[0]), np.ascontiguousarray(gt[:, :, :4]), {"zero_rows": [], "planted": len(planted)})]


# ----------------------------------------------------------------------------------------------------------- anchor scenes
def _gt_rows(rows, G):
    out = np.zeros((G, 5), F32)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def _anchor_box(cy, cx, a, grid=None, feat_w=FEAT_W):
    grid = anchor_grid() if grid is None else grid
    return [int(v) for v in grid[anchor_index(cy, cx, a, feat_w)]]


NORMAL_GT = [[120, 80, 330, 300, 3], [400, 250, 640, 520, 8], [700, 60, 930, 210, 12], [50, 380, 260, 560, 1]]
TINY_GT = [497, 301, 504, 308, 4]        # 8x8: no anchor reaches 0.3 on it; the 88x176 anchors that contain it tie for its best
OUTSIDE_GT = [0, 0, 7, 7, 6]             # the corner: inside anchors that start at x < 8 start at y >= 8 and the other way round


def threshold_gts():
    """The anchor-family threshold pairs as ground truth, each in a corner of the image of its own so that no pair sees another:
    (constant, side, (cy, cx, a), gt row).  The anchor at (cy, cx, a) then has exactly that IoU as its best."""
    out = []
    for (key, side), (cy, cx) in zip((("0.7", "at"), ("0.3", "at"), ("0.7", "low"), ("0.3", "low")), ((8, 12), (8, 45), (26, 12), (26, 45))):
        box = _anchor_box(cy, cx, 3)
        gt, _, _ = partial_gt_for(box, CONSTANTS[key])
        d = 1 if side == "low" else 0
        out.append((key, side, (cy, cx, 3), [gt[0], gt[1] + d, gt[2], gt[3] + d, 2 + len(out)]))
    return out


def anchor_scenes():
    """Scenes for _AnchorTargetLayer: gt (B,G,5), im_info (B,3), feature size.  ``prop`` names what each image is built to be."""
    info = np.array([[IM_H, IM_W, 1.0]] * 2, F32)
    feat = (FEAT_H, FEAT_W)
    G = 30
    normal, empty = _gt_rows(NORMAL_GT, G), np.zeros((G, 5), F32)
    eq = _anchor_box(20, 20, 3)
    many = _gt_rows([_anchor_box(cy, cx, 3) + [1 + (cy + cx) % 15] for cy in (5, 12, 19, 26, 33) for cx in range(5, 55, 7)], 40)
    scenes = [
        AnchorScene("empty_first", np.stack([empty, normal]), info, feat, {"empty": [0]}),
        AnchorScene("empty_last", np.stack([normal, empty]), info, feat, {"empty": [1]}),
        AnchorScene("anchor_equal_dup", np.stack([_gt_rows([eq + [5], eq + [9]] + NORMAL_GT[:2], G), normal]), info, feat,
                    {"equal": (0, (20, 20, 3))}),
        AnchorScene("tiny_tie_outside", np.stack([_gt_rows([TINY_GT] + NORMAL_GT[:1], G), _gt_rows([OUTSIDE_GT], G)]), info, feat,
                    {"tiny": (0, 0), "outside": (1, 0)}),
        AnchorScene("thresholds", np.stack([_gt_rows([t[3] for t in threshold_gts()], G), normal]), info, feat,
                    {"pairs": [(0,) + t[:3] for t in threshold_gts()]}),
        AnchorScene("many_fg", np.stack([many, _gt_rows(NORMAL_GT, 40)]), info, feat, {"many": [0]}),
    ]
    # a 20x20 map of a 320x320 image: only 128x128, 256x256, 184x96 and 88x176 anchors fit, most anchors are outside
    sinfo = np.array([[320, 320, 1.0]] * 2, F32)
    grid = anchor_grid(20, 20)
    sbox = [int(v) for v in grid[anchor_index(9, 9, 3, 20)]]
    sgt, _, _ = partial_gt_for(sbox, CONSTANTS["0.7"])
    small = [_gt_rows([sgt + [3], [200, 30, 290, 110, 7]], G), _gt_rows([[int(v) for v in grid[anchor_index(10, 10, 4, 20)]] + [2]], G)]
    scenes.append(AnchorScene("small_map", np.stack(small), sinfo, (20, 20), {"pairs": [(0, "0.7", "at", (9, 9, 3))]}))
    return scenes


def scene_anchors(scene):
    """(inside anchors (n,4), their indices into the whole grid, the grid's size); the inside test uses image 0 (a reference quirk)."""
    grid = anchor_grid(*scene.feat)
    inside = np.nonzero(inside_mask(grid, int(scene.im_info[0, 0]), int(scene.im_info[0, 1])))[0]
    return grid[inside], inside, grid.shape[0]


# ----------------------------------------------------------------------------------------------------------- proposal scenes
G1, G2 = [100, 100, 199, 199], [500, 300, 599, 399]
PROPOSAL_G = 8
PROPOSAL_R = (32, 128)
BG_LO = (0.0, 0.1)                         # cfgs/res101.yml, the default


def _shifted(box, d):
    return [box[0] + d, box[1], box[2] + d, box[3]]


def _image_thresholds():
    """Both classes, more foreground than round(0.25 * 128): G1 shifted right by 1..33 columns ((100 - d) / (100 + d) >= 1/2) and
    G2 by 1..10; rois exactly on 1/2, one row below it, exactly on 1/10, one row below it, and touching G1 (exactly 0); bulk
    background.  ``marks`` name the rows of the decision rois."""
    rois = [[100, 100, 199, 149], [100, 100, 199, 148], [100, 100, 199, 109], [100, 100, 199, 108], [100, 200, 199, 249]]
    marks = {"at_0.5": 0, "below_0.5": 1, "at_0.1": 2, "below_0.1": 3, "at_0.0": 4}
    rois += [_shifted(G1, d) for d in range(1, 34)] + [_shifted(G2, d) for d in range(1, 11)]
    rois += [[100, 100, 199 - d, 199 - 2 * d] for d in range(1, 11)]             # foreground of another size: dw, dh != 0
    rois += [[100 + 3 * i, 120 + i, 260 + 3 * i, 260 + 2 * i] for i in range(30)]                   # partial overlaps with G1
    rois += [[650 + 5 * i, 20 + 7 * i, 760 + 5 * i, 110 + 7 * i] for i in range(20)]                # disjoint from both
    return rois, [G1 + [3], G2 + [5]], marks


def _image_few_fg():
    """Two foreground rois (plus the appended gt: three), fewer than round(0.25 * 32) = 8; background rois around."""
    rois = [_shifted(G1, 5), [100, 100, 189, 179]] + [[60 + 4 * i, 150 + 2 * i, 170 + 4 * i, 290 + 2 * i] for i in range(40)]
    return rois, [G1 + [11]], {}


def _image_dup_gt():
    """G1 twice with classes 2 and 7: every label comes from the first."""
    rois = [_shifted(G1, d) for d in range(0, 30, 3)] + [[100, 100, 199, 120 + i] for i in range(25)]    # (21 + i) / 100
    rois += [[100 + d, 100, 199, 199 - d] for d in range(1, 11)]
    return rois, [G1 + [2], G1 + [7], G2 + [4]], {}


def _image_only_fg():
    """Every roi at or above 1/2 on G1 or G2, every other row padding: no background under either BG_THRESH_LO."""
    return [_shifted(G1, d) for d in range(0, 30)] + [_shifted(G2, d) for d in range(0, 20)], [G1 + [3], G2 + [5]], {}


def _image_single_bg():
    """Foreground rois and ONE background candidate (IoU 0.3 with G1): sampling with replacement repeats it."""
    return [_shifted(G1, d) for d in range(0, 12)] + [[100, 100, 199, 129]], [G1 + [6]], {"bg_row": 12}


def _image_no_gt():
    """No ground truth: every real roi has max overlap 0 -- background under BG_THRESH_LO = 0.0, nothing under 0.1."""
    return [[20 * i, 10 * i, 20 * i + 150, 10 * i + 120] for i in range(40)], [], {}


def _image_neither():
    """No ground truth and no proposals: every candidate is a unit box (-1)."""
    return [], [], {}


def _proposal_scene(name, images, P, prop):
    B = len(images)
    rois, gt = np.zeros((B, P, 5), F32), np.zeros((B, PROPOSAL_G, 5), F32)
    marks = []
    for b, (r, g, m) in enumerate(images):
        assert len(r) <= P and len(g) <= PROPOSAL_G
        rois[b, :, 0] = b
        if r:
            rois[b, :len(r), 1:] = r                       # the rest of the rows stay zero: a short proposal list
        if g:
            gt[b, :len(g)] = g
        marks.append(m)
    return ProposalScene(name, rois, gt, dict(prop, marks=marks, n_real=[len(i[0]) for i in images]))


def proposal_scenes():
    """Scenes for _ProposalTargetLayer: rois (B,P,5), gt (B,8,5).  prop["regime"][lo] lists per image which sampling branch the
    reference takes under that BG_THRESH_LO: "both", "fg", "bg" or "none" (the reference raises on "none")."""
    return [
        _proposal_scene("thresholds_mix", [_image_thresholds(), _image_few_fg(), _image_dup_gt()], 128,
                        {"regime": {0.0: ["both", "both", "both"], 0.1: ["both", "both", "both"]}}),
        _proposal_scene("one_class", [_image_only_fg(), _image_single_bg()], 64,
                        {"regime": {0.0: ["fg", "both"], 0.1: ["fg", "both"]}}),
        _proposal_scene("no_gt", [_image_no_gt(), _image_thresholds()], 300,
                        {"regime": {0.0: ["bg", "both"], 0.1: ["none", "both"]}}),
        _proposal_scene("neither", [_image_thresholds(), _image_neither()], 128,
                        {"regime": {0.0: ["both", "none"], 0.1: ["both", "none"]}}),
    ]


def proposal_candidates(scene):
    """(B, P + G, 5): the rois with the ground truth appended, as the layer forms them."""
    app = np.zeros_like(scene.gt)
    app[:, :, 1:5] = scene.gt[:, :, :4]
    return np.concatenate([scene.rois, app], 1)


def raises(scene, lo):
    return "none" in scene.prop["regime"][lo]
