"""Detection mAP of the detector test loop: the PASCAL VOC evaluation behind ``imdb.evaluate_detections``
(lib/datasets/voc_eval.py ``voc_eval`` / ``voc_ap`` and the results-file writer of the reference's dataset classes).

``evaluate`` takes what ``test_instance_styled.py`` collects -- ``all_boxes[class][image]``, (n, 5) rows of x1 y1 x2 y2
score -- and the roidb the loop already holds (``boxes``, ``gt_classes``, ``gt_ishard`` per image; no XML is read) and
returns per class recall, precision and AP, and the mean AP.

The rules, which the host form and the kernels (csrc/det_eval.hip) share:

* The reference writes its detections to a text file and reads them back, so a score enters as what ``'%.3f'`` of it reads
  back as and a coordinate as what ``'%.1f'`` of ``coordinate + 1`` reads back as.  That rounding is part of the metric and
  is done here with real string formatting.  ``coordinate + 1`` is ``float64(value) + 1.0``.  The quantised score is a
  whole number of thousandths and is carried as an int32 key.  The annotations are the roidb boxes + 1 (the +1 IoU is
  translation invariant, so both sides carry the + 1).
* Within a class the detections are taken in descending score, EQUAL SCORES IN RESULTS-FILE ORDER (image index, then row
  in ``all_boxes[c][i]``): a stable sort.  The reference sorts with an unstable ``np.argsort``, which leaves the order of
  equal scores unspecified; this is the documented choice here.
* A detection is compared with the ground truths of its class in its image: float64 IoU with the +1 convention in the
  reference's operation order, the first maximum wins.  No ground truth there: a false positive.  ``ovmax > ovthresh``
  (strict) and the best ground truth neither hard nor claimed: a true positive, which claims it.  Claimed: a false
  positive (no second best).  Hard: neither.  Images are independent, so the match runs per (class, image) segment.
* Per class: integer prefix sums of tp and fp, ``rec = tp / npos`` (npos = the class's ground truths that are not hard),
  ``prec = tp / max(tp + fp, eps)``, and ``voc_ap`` in the area form (terms added in index order) or the 11-point form.
  No detections: empty curves, ap 0.  ``npos == 0`` with detections: nan recall and a nan area ap, as the reference's
  division gives; ``mean_ap`` is the plain mean (nan then, as the reference prints), ``mean_ap_present`` the nan-mean.

``device=None`` runs everything in numpy on the host; with a device the match and the curves are HIP kernels.  Both start
from the same packed arrays and agree bit for bit.
"""
import numpy as np

from .packing import cat, offsets

MAX_GT = 4096                # ground truths of one class in one image (csrc/det_eval.hip DE_MAXG)
MAX_CLASSES = 255            # foreground classes
MAX_PER_CLASS = 1 << 24      # detections of one class
TP, FP, IGNORED = 1, 2, 0


# ------------------------------------------------------------------------------------------------------------------
# results-file quantisation
# ------------------------------------------------------------------------------------------------------------------
def quantise_scores(scores):
    """int32 thousandths of what ``'%.3f' % score`` reads back as."""
    s = np.asarray(scores).astype(np.float64).reshape(-1)
    if not np.isfinite(s).all():
        raise ValueError("detection_eval: a detection score is not finite")
    if s.size == 0:
        return np.zeros(0, np.int32)
    text = np.char.mod("%.3f", s)
    key = np.char.replace(text, ".", "").astype(np.int64)        # "-0.124" -> -124: the digits ARE the thousandths
    if np.abs(key).max() >= 2 ** 31:
        raise ValueError("detection_eval: a detection score is out of the int32 range of thousandths")
    return key.astype(np.int32)


def quantise_coords(coords):
    """What ``'%.1f' % (coordinate + 1)`` reads back as, float64; the sum is ``float64(coordinate) + 1.0``."""
    x = np.asarray(coords)
    shape = x.shape
    x = x.astype(np.float64).reshape(-1) + 1.0
    if not np.isfinite(x).all():
        raise ValueError("detection_eval: a detection coordinate is not finite")
    if x.size == 0:
        return np.zeros(shape, np.float64)
    return np.char.mod("%.1f", x).astype(np.float64).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------
# packing
# ------------------------------------------------------------------------------------------------------------------
class Packed(object):
    """Flat arrays of one evaluation (the layout of ``ops.det_eval_match`` / ``ops.det_eval_curve``).  Foreground class
    ``c`` of ``all_boxes`` is class ``k = c - 1`` here.

    det_key (D) int32, det_box (D, 4) float64: the detections in results-file order (class, image, row);
    det_img (D) int32: their image;
    cls_off (C + 1): class k owns detections [cls_off[k], cls_off[k + 1]);
    seg_det_off (S + 1), seg_cls (S), seg_img (S), seg_gt (S): segment s, a (class, image) pair that has detections, owns
        detections [seg_det_off[s], seg_det_off[s + 1]) and ground-truth slot seg_gt[s] = seg_cls[s] * I + seg_img[s];
    gt_off (C * I + 1): slot k * I + i owns ground truths [gt_off[slot], gt_off[slot + 1]), in roidb row order;
    gt_box (G, 4) float64 (annotation + 1), gt_hard (G) int32, gt_row (G) int32: the row in the image's roidb entry;
    npos (C) int32: ground truths of the class that are not hard."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def pack(all_boxes, roidb, num_classes):
    C, I = int(num_classes) - 1, len(roidb)
    if C > MAX_CLASSES:
        raise ValueError("detection_eval: at most %d foreground classes (got %d)" % (MAX_CLASSES, C))
    if len(all_boxes) < num_classes or any(len(all_boxes[c]) != I for c in range(1, num_classes)):
        raise ValueError("detection_eval: all_boxes must be [num_classes][%d images]" % I)
    parts, seg_cls, seg_img, seg_n = [], [], [], []
    for c in range(1, num_classes):
        row = all_boxes[c]
        for i in range(I):
            d = row[i]
            if len(d) == 0:                              # [] or a (0, 5) array: the writer skips it
                continue
            d = np.asarray(d)
            if d.ndim != 2 or d.shape[1] < 5:
                raise ValueError("detection_eval: all_boxes[%d][%d] must be (n, 5) rows of x1 y1 x2 y2 score" % (c, i))
            parts.append(d)
            seg_cls.append(c - 1)
            seg_img.append(i)
            seg_n.append(d.shape[0])
    if parts:
        flat = np.concatenate([p.astype(np.float64) for p in parts])         # float32 -> float64 is exact
        det_key, det_box = quantise_scores(flat[:, -1]), quantise_coords(flat[:, :4])
    else:
        det_key, det_box = np.zeros(0, np.int32), np.zeros((0, 4), np.float64)
    seg_cls, seg_img, seg_n = np.asarray(seg_cls, np.int32), np.asarray(seg_img, np.int32), np.asarray(seg_n, np.int64)
    if seg_n.sum() >= 2 ** 30:
        raise ValueError("detection_eval: too many detections")
    seg_det_off = offsets(seg_n, "detection_eval: too many detections")
    per_class = np.bincount(seg_cls, weights=seg_n, minlength=C).astype(np.int64) if C else np.zeros(0, np.int64)
    if len(per_class) and per_class.max() >= MAX_PER_CLASS:
        raise ValueError("detection_eval: at most %d detections of one class" % (MAX_PER_CLASS - 1))
    cls_off = offsets(per_class, "detection_eval: too many detections")
    det_img = np.repeat(seg_img, seg_n).astype(np.int32)

    g_box, g_cls, g_img, g_hard, g_row = [], [], [], [], []
    for i, e in enumerate(roidb):
        b = np.asarray(e["boxes"]).astype(np.float64).reshape(-1, 4)
        cl = np.asarray(e["gt_classes"]).astype(np.int64).reshape(-1)
        hard = np.asarray(e["gt_ishard"]).astype(np.int32).reshape(-1) if "gt_ishard" in e else np.zeros(len(cl), np.int32)
        if not (len(b) == len(cl) == len(hard)):
            raise ValueError("detection_eval: roidb[%d] boxes / gt_classes / gt_ishard differ in length" % i)
        g_box.append(b + 1.0)
        g_cls.append(cl)
        g_img.append(np.full(len(cl), i, np.int64))
        g_hard.append((hard != 0).astype(np.int32))
        g_row.append(np.arange(len(cl), dtype=np.int32))
    g_box, g_cls, g_img = cat(g_box, (4,), np.float64), cat(g_cls, (), np.int64), cat(g_img, (), np.int64)
    g_hard, g_row = cat(g_hard, (), np.int32), cat(g_row, (), np.int32)
    fg = (g_cls >= 1) & (g_cls < num_classes)
    g_box, g_cls, g_img, g_hard, g_row = g_box[fg], g_cls[fg], g_img[fg], g_hard[fg], g_row[fg]
    slot = (g_cls - 1) * I + g_img
    by_slot = np.argsort(slot, kind="stable")
    counts = np.bincount(slot, minlength=C * I) if C * I else np.zeros(0, np.int64)
    if len(counts) and counts.max() > MAX_GT:
        raise ValueError("detection_eval: at most %d ground truths of one class in one image (got %d)" % (MAX_GT, counts.max()))
    gt_off = offsets(counts, "detection_eval: too many ground truths")
    npos = np.bincount(g_cls[g_hard == 0] - 1, minlength=C).astype(np.int32) if C else np.zeros(0, np.int32)
    return Packed(n_classes=C, n_images=I, det_key=det_key, det_box=det_box, det_img=det_img, cls_off=cls_off,
                  seg_det_off=seg_det_off, seg_cls=seg_cls, seg_img=seg_img, seg_gt=(seg_cls.astype(np.int64) * I + seg_img).astype(np.int32),
                  gt_off=gt_off, gt_box=np.ascontiguousarray(g_box[by_slot]), gt_hard=np.ascontiguousarray(g_hard[by_slot]),
                  gt_row=np.ascontiguousarray(g_row[by_slot]), npos=npos)


# ------------------------------------------------------------------------------------------------------------------
# host form
# ------------------------------------------------------------------------------------------------------------------
def _overlaps(bb, gt):
    """(n_det, n_gt) IoU, +1 convention, float64, voc_eval's operation order."""
    ixmin = np.maximum(gt[None, :, 0], bb[:, None, 0])
    iymin = np.maximum(gt[None, :, 1], bb[:, None, 1])
    ixmax = np.minimum(gt[None, :, 2], bb[:, None, 2])
    iymax = np.minimum(gt[None, :, 3], bb[:, None, 3])
    iw = np.maximum(ixmax - ixmin + 1., 0.)
    ih = np.maximum(iymax - iymin + 1., 0.)
    inters = iw * ih
    uni = (((bb[:, 2] - bb[:, 0] + 1.) * (bb[:, 3] - bb[:, 1] + 1.))[:, None] +
           ((gt[:, 2] - gt[:, 0] + 1.) * (gt[:, 3] - gt[:, 1] + 1.))[None, :] - inters)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inters / uni


def match_arrays_host(pk, ovthresh=0.5):
    """The rules of ``ops.det_eval_match`` in numpy, on the same arrays: (flag (D) int32, ovmax (D) float64, jmax (D)
    int32), each at the detection's results-file position.  jmax is -1 and ovmax -inf without a ground truth."""
    D = len(pk.det_key)
    flag = np.zeros(D, np.int32)
    ovmax = np.full(D, -np.inf, np.float64)
    jmax = np.full(D, -1, np.int32)
    for s in range(len(pk.seg_gt)):
        d0, d1 = int(pk.seg_det_off[s]), int(pk.seg_det_off[s + 1])
        g0, g1 = int(pk.gt_off[pk.seg_gt[s]]), int(pk.gt_off[pk.seg_gt[s] + 1])
        if g1 == g0:
            flag[d0:d1] = FP
            continue
        ov = _overlaps(pk.det_box[d0:d1], pk.gt_box[g0:g1])
        jm = np.argmax(ov, axis=1)                       # the first maximum (the first nan, if any)
        om = np.max(ov, axis=1)
        ovmax[d0:d1], jmax[d0:d1] = om, jm
        hard = pk.gt_hard[g0:g1]
        claimed = np.zeros(g1 - g0, bool)
        f = np.full(d1 - d0, FP, np.int32)
        for q in np.argsort(-pk.det_key[d0:d1].astype(np.int64), kind="stable"):
            if om[q] > ovthresh:
                j = jm[q]
                if hard[j]:
                    f[q] = IGNORED
                elif not claimed[j]:
                    f[q] = TP
                    claimed[j] = True
        flag[d0:d1] = f
    return flag, ovmax, jmax


def ap_area(rec, prec):
    """``voc_ap`` area form; the terms are added in index order (np.cumsum), which the kernel does too."""
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    with np.errstate(invalid="ignore"):
        terms = (mrec[i + 1] - mrec[i]) * mpre[i + 1]
        return np.float64(np.cumsum(terms)[-1]) if len(terms) else np.float64(0.0)


def ap_11pt(rec, prec):
    """``voc_ap`` 11-point form of the 2007 devkit."""
    ap = 0.
    for t in np.arange(0., 1.1, 0.1):
        with np.errstate(invalid="ignore"):
            above = rec >= t
        p = np.max(prec[above]) if above.any() else 0
        ap = ap + p / 11.
    return np.float64(ap)


def curve_arrays_host(pk, flag):
    """The rules of ``ops.det_eval_curve`` in numpy: dict of perm, cum_tp, cum_fp (D) int32, rec, prec (D) float64 -- all
    in class order at the class's own offsets -- and ap_area, ap_11pt (C) float64."""
    D, C = len(pk.det_key), pk.n_classes
    out = {"perm": np.zeros(D, np.int32), "cum_tp": np.zeros(D, np.int32), "cum_fp": np.zeros(D, np.int32),
           "rec": np.zeros(D, np.float64), "prec": np.zeros(D, np.float64),
           "ap_area": np.zeros(C, np.float64), "ap_11pt": np.zeros(C, np.float64)}
    eps = np.finfo(np.float64).eps
    for k in range(C):
        a, b = int(pk.cls_off[k]), int(pk.cls_off[k + 1])
        perm = a + np.argsort(-pk.det_key[a:b].astype(np.int64), kind="stable")
        f = flag[perm]
        tp, fp = np.cumsum(f == TP), np.cumsum(f == FP)
        with np.errstate(divide="ignore", invalid="ignore"):
            rec = tp / float(pk.npos[k])
        prec = tp / np.maximum(tp + fp, eps)
        out["perm"][a:b], out["cum_tp"][a:b], out["cum_fp"][a:b] = perm, tp, fp
        out["rec"][a:b], out["prec"][a:b] = rec, prec
        out["ap_area"][k], out["ap_11pt"][k] = ap_area(rec, prec), ap_11pt(rec, prec)
    return out


# ------------------------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------------------------
def evaluate_packed(pk, ovthresh=0.5, device=None):
    """(flag, ovmax, jmax, curves) of packed arrays, on the host (``device=None``) or by the kernels."""
    if device is None:
        flag, ovmax, jmax = match_arrays_host(pk, ovthresh)
        return flag, ovmax, jmax, curve_arrays_host(pk, flag)
    from . import ops
    flag, ovmax, jmax = ops.det_eval_match(pk.seg_det_off, pk.seg_gt, pk.gt_off, pk.det_key, pk.det_box, pk.gt_box, pk.gt_hard,
                                           ovthresh, device=device)
    names = ("perm", "cum_tp", "cum_fp", "rec", "prec", "ap_area", "ap_11pt")
    cur = ops.det_eval_curve(pk.det_key, pk.cls_off, flag, pk.npos, device=device)
    return flag.cpu().numpy(), ovmax.cpu().numpy(), jmax.cpu().numpy(), dict((n, t.cpu().numpy()) for n, t in zip(names, cur))


def evaluate(all_boxes, roidb, classes, ovthresh=0.5, use_07_metric=False, device=None):
    """``all_boxes[c][i]``: (n, 5) detections of class c (an index into ``classes``, 0 the background) in image i;
    ``roidb[i]``: boxes, gt_classes, gt_ishard.  Returns {"rec", "prec", "ap": {class name: ...}, "aps": (C,) array in
    class order, "mean_ap": np.mean(aps), "mean_ap_present": the mean over the classes whose ap is a number}."""
    pk = pack(all_boxes, roidb, len(classes))
    _, _, _, cur = evaluate_packed(pk, ovthresh, device)
    aps = np.asarray(cur["ap_11pt" if use_07_metric else "ap_area"], np.float64)
    rec, prec, ap = {}, {}, {}
    for k in range(pk.n_classes):
        a, b = int(pk.cls_off[k]), int(pk.cls_off[k + 1])
        name = classes[k + 1]
        rec[name], prec[name], ap[name] = cur["rec"][a:b].copy(), cur["prec"][a:b].copy(), aps[k]
    present = aps[~np.isnan(aps)]
    return {"rec": rec, "prec": prec, "ap": ap, "aps": aps,
            "mean_ap": np.float64(np.mean(aps)) if len(aps) else np.float64(np.nan),
            "mean_ap_present": np.float64(np.mean(present)) if len(present) else np.float64(np.nan)}


def report(result, classes, output_dir=None, out=print):
    """The reference's lines (``AP for <cls> = %.4f``, ``Mean AP = %.4f``) and, with ``output_dir``, its ``<cls>_pr.pkl``
    files ({'rec', 'prec', 'ap'}) plus ``detection_eval.json`` (a nan is written as null)."""
    import json
    import os
    import pickle
    num = lambda x: None if np.isnan(x) else float(x)
    for name in classes[1:]:
        out("AP for {} = {:.4f}".format(name, result["ap"][name]))
        if output_dir is not None:
            with open(os.path.join(output_dir, name + "_pr.pkl"), "wb") as f:
                pickle.dump({"rec": result["rec"][name], "prec": result["prec"][name], "ap": result["ap"][name]}, f)
    out("Mean AP = {:.4f}".format(result["mean_ap"]))
    if output_dir is not None:
        with open(os.path.join(output_dir, "detection_eval.json"), "w") as f:
            json.dump({"ap": dict((name, num(result["ap"][name])) for name in classes[1:]), "mean_ap": num(result["mean_ap"]),
                       "mean_ap_present": num(result["mean_ap_present"]),
                       "n_detections": dict((name, int(len(result["rec"][name]))) for name in classes[1:])}, f, indent=1)
