"""Image relation recall@K: relation detection, phrase detection and predicate detection recall@50/100 of image relation
work (Lu et al., ECCV 2016), with zero-shot recall and per-predicate ("mean") recall, over what the relation test loop writes.

The reference has no image-level relation metric (``lib/utils.py`` evaluates videos only), so the rules below are this
project's own, as Seq-NMS's and rel_det's are.  They are stated once here for the host form (``match_host`` / ``count_host``)
and the kernels (csrc/image_relations.hip, ``ops.image_relation_match`` / ``ops.image_relation_count``), which agree bit for
bit in every output.

Inputs.
  ``relations`` is what ``test_sgg_emb.py`` pickles: it maps a frame key to the five values of ``eval.detection_output``
  -- ``(rlp_labels (k,3) [subject class, predicate, object class], tuple_confs (n,), sub_bboxes (k,4), obj_bboxes (k,4),
  rel_idex (n,))`` -- or to five Nones.  ``annotations`` maps a frame key to ``{"boxes", "box_classes", "rels": [[s, o,
  predicate], ...]}``, the layout of ``vrd.target_gt_rels`` and of ``synthetic.relation_annotation``.  Both use unscaled image
  pixels.

Images.
  The images evaluated are the keys of ``annotations`` that have at least one entry in ``rels``, in sorted key order.  A key
  missing from ``relations``, or mapped to Nones, has no predictions; its ground truths still count in every denominator
  (what ``evaluate`` in lib/utils.py:395 does for a video without predictions).  Keys of ``relations`` that are not in
  ``annotations`` are ignored, and are counted in ``n_ignored``.

Ground truths.
  A ground truth is one row of ``rels``, kept in annotation order, duplicates included.  It has the triplet
  ``(box_classes[s], predicate, box_classes[o])`` and the two boxes ``boxes[s]``, ``boxes[o]``.  A row whose ``s`` or ``o``
  lies outside ``boxes``, or whose predicate lies outside ``[0, n_rel)``, is a ``ValueError`` at packing.

Predictions.
  An image's predictions are its first ``len(tuple_confs)`` rows.  They are ranked in descending float32 confidence, equal
  confidences in file order: a stable sort, done at packing.  If ``k_per_pair`` is given, the ranked list is walked and a row
  is dropped when ``k_per_pair`` better-ranked rows with its ``rel_idex`` were already kept.  This is a cap applied to the
  written top-k list; it is not a ranking rule of the loop (``relation_topk`` ranks all cells of all pairs together, so a
  pair's later predicates may never have been written).  Then the list is cut to ``max(nreturns)``.  A non-finite confidence
  or coordinate is a ``ValueError``.

Overlap.
  Float64, +1 pixel convention, in the operation order of ``packing.overlap_plus1`` (lib/model/nms/nms_cpu.py:14,26-31):
  ``iw = (min(ax2, bx2) - max(ax1, bx1)) + 1``, ``ih`` likewise, ``inter = iw * ih``, ``area = ((x2 - x1) + 1) * ((y2 - y1) +
  1)``, ``overlap = inter / ((area_a + area_b) - inter)``.  A non-positive ``iw`` or ``ih`` gives 0.

Candidate score.
  Relation mode: ``ov(pred, gt) = min(overlap(sub, gt_sub), overlap(obj, gt_obj))``.  Phrase mode: ``ov(pred, gt)`` is the
  overlap of the two union boxes; a union box is the elementwise min of x1 and y1 and the elementwise max of x2 and y2 of
  the subject and the object box, which is exact.  Where the triplets differ, ``ov`` is -1.

Matching.
  Per image and per mode; the modes do not interact.  Predictions are taken in rank order.  Each prediction takes the
  not-yet-taken ground truth with the largest ``ov >= iou_threshold`` (default 0.5; it must be positive); on equal ``ov`` the
  lower index wins.  A prediction whose best ground truth is already taken takes the next best.  Outputs, all at the image's
  own offsets: ``hit (n_pred)`` the ground-truth index within the image or -1; ``hit_ov`` the overlap of the hit or -1;
  ``gt_rank (n_gt)`` the 0-based rank of the prediction that took the ground truth, or -1.

Counters (integers, so they do not depend on summation order).
  For each mode and each ``K`` in ``nreturns`` (at most 8 values) ground truth g is hit at K when ``0 <= gt_rank[g] < K``.
  ``totals[mode][K] = (hits, n_gt)``; ``zs_totals[mode][K]`` the same over ground truths flagged zero-shot;
  ``per_predicate[mode][K][p] = (hits, n_gt)`` per predicate ``p``.  A ground truth is zero-shot when its triplet is not in
  ``seen_triplets``, a set of ``(s_cls, predicate, o_cls)`` (``seen_triplets_of(annotations)`` builds one from training
  annotations).  Without ``seen_triplets`` nothing is zero-shot.

Results (``evaluate``).
  Per mode (``"relation"``, ``"phrase"``): ``recall[K] = hits / n_gt``; ``zero_shot_recall[K]`` (nan without a zero-shot
  ground truth); ``mean_recall[K]``, the mean over the predicates that have ground truths of ``hits_p / n_p``, added in
  predicate order; and the raw integer tables.  Also ``n_images``, ``n_gt``, ``n_gt_zero_shot``, ``n_ignored``.  All divisions
  are float64, done on the host from the integer counters.

Predicate detection.
  On annotated boxes (the relation loop's default input) every prediction's boxes are annotated boxes, so relation-mode recall
  IS predicate-detection recall.  On detections (``--target_gt_rels_path tracked_boxes.pkl``) it is relation detection, and
  phrase mode phrase detection.  There is no third mode.

Limits: ``MAX_GT = 4096`` ground truths in one image (one taken-bit each in the kernel's LDS); any number of predictions, the
kernel being sized for the loop's 100.  Exceeding a limit is a ``ValueError``.
"""
import numpy as np

from .packing import cat, offsets, overlap_plus1

MAX_GT = 4096                # ground truths of one image (csrc/image_relations.hip IR_MAXG)
MAX_K = 8                    # values of K in one evaluation
MODES = ("relation", "phrase")


class Packed(object):
    """Flat arrays of one evaluation (the layout of ``ops.image_relation_match`` / ``ops.image_relation_count``).

    keys: the images evaluated, in order; n_ignored: predicted images without annotation; n_rel; max_pred: the cut;
    pred_off, gt_off (I + 1) int32: image i owns predictions [pred_off[i], pred_off[i + 1]) and ground truths [gt_off[i],
        gt_off[i + 1]);
    pred_trip (n_pred, 3) int32 [subject class, predicate, object class], pred_box (n_pred, 8) float64 [subject box, object
        box], pred_conf (n_pred) float32, pred_row (n_pred) int32 the row in the image's record: all in rank order;
    n_before_cut (I) int32: the predictions an image had after the per-pair cap, before the cut to max_pred;
    gt_trip (n_gt, 3) int32, gt_box (n_gt, 8) float64, gt_zs (n_gt) int32: the ground truths in annotation order."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _nreturns(nreturns):
    ks = [int(k) for k in nreturns]
    if not 1 <= len(ks) <= MAX_K or any(k < 1 for k in ks) or len(set(ks)) != len(ks):
        raise ValueError("image_relations: nreturns holds 1 to %d distinct positive values of K (got %r)" % (MAX_K, list(nreturns)))
    return ks


def seen_triplets_of(annotations):
    """The set of (subject class, predicate, object class) of every relation of ``annotations`` (the training set's, for the
    zero-shot split)."""
    seen = set()
    for anno in annotations.values():
        cls = anno["box_classes"]
        for s, o, p in anno["rels"]:
            seen.add((int(cls[int(s)]), int(p), int(cls[int(o)])))
    return seen


def _image_predictions(key, rec, max_pred, k_per_pair):
    """One image's record -> (trip (n,3) int32, box (n,8) float64, conf (n) float32, row (n) int32, n before the cut)."""
    if rec is None or len(rec) != 5 or rec[1] is None:
        return None
    rlp, conf, sub, obj, idx = rec
    conf = np.asarray(conf, np.float32).reshape(-1)
    n = len(conf)
    rlp, sub, obj = np.asarray(rlp, np.float64), np.asarray(sub, np.float64), np.asarray(obj, np.float64)
    idx = np.asarray(idx).reshape(-1)
    if rlp.ndim != 2 or rlp.shape[1] != 3 or sub.ndim != 2 or sub.shape[1] != 4 or obj.shape != sub.shape or min(len(rlp), len(sub)) < n \
            or len(idx) != n:
        raise ValueError("image_relations.pack: image %r: the record is (rlp_labels (k,3), tuple_confs (n,), sub_bboxes (k,4), "
                         "obj_bboxes (k,4), rel_idex (n,)) with n <= k" % (key,))
    rlp, sub, obj = rlp[:n], sub[:n], obj[:n]
    if not (np.isfinite(conf).all() and np.isfinite(sub).all() and np.isfinite(obj).all() and np.isfinite(rlp).all()):
        raise ValueError("image_relations.pack: image %r: a confidence, label or coordinate is not finite" % (key,))
    if n and np.abs(rlp).max() >= 2 ** 31:
        raise ValueError("image_relations.pack: image %r: a label is out of the int32 range" % (key,))
    order = np.argsort(-conf, kind="stable")                     # descending, equal confidences in file order
    if k_per_pair is not None:
        kept, seen = [], {}
        for r in order.tolist():
            pair = int(idx[r])
            if seen.get(pair, 0) < k_per_pair:
                seen[pair] = seen.get(pair, 0) + 1
                kept.append(r)
        order = np.asarray(kept, np.int64)
    before = len(order)
    order = order[:max_pred]
    return rlp[order].astype(np.int32), np.hstack([sub[order], obj[order]]), conf[order], order.astype(np.int32), before


def pack(relations, annotations, n_rel, nreturns=(50, 100), k_per_pair=None, seen_triplets=None):
    """-> ``Packed``: the evaluated images in sorted key order, their predictions ranked, capped and cut, their ground truths."""
    n_rel, max_pred = int(n_rel), max(_nreturns(nreturns))
    if n_rel < 1:
        raise ValueError("image_relations.pack: n_rel must be at least 1")
    if k_per_pair is not None:
        k_per_pair = int(k_per_pair)
        if k_per_pair < 1:
            raise ValueError("image_relations.pack: k_per_pair must be at least 1")
    seen = None if seen_triplets is None else set((int(s), int(p), int(o)) for s, p, o in seen_triplets)
    keys = sorted(k for k, a in annotations.items() if len(a["rels"]) > 0)
    n_ignored = sum(1 for k in relations if k not in annotations)
    p_trip, p_box, p_conf, p_row, p_n, before = [], [], [], [], [], []
    g_trip, g_box, g_zs, g_n = [], [], [], []
    for key in keys:
        anno = annotations[key]
        boxes = np.asarray(anno["boxes"], np.float64).reshape(-1, 4)
        cls = np.asarray(anno["box_classes"]).reshape(-1)
        rels = np.asarray(anno["rels"])
        if rels.ndim != 2 or rels.shape[1] != 3 or len(cls) != len(boxes):
            raise ValueError("image_relations.pack: image %r: rels are [s, o, predicate] rows and box_classes has one entry per box" % (key,))
        if len(rels) > MAX_GT:
            raise ValueError("image_relations.pack: image %r: at most %d ground truths in one image (got %d)" % (key, MAX_GT, len(rels)))
        rels = rels.astype(np.int64)
        s, o, p = rels[:, 0], rels[:, 1], rels[:, 2]
        if (s < 0).any() or (s >= len(boxes)).any() or (o < 0).any() or (o >= len(boxes)).any():
            raise ValueError("image_relations.pack: image %r: a relation names a box outside [0, %d)" % (key, len(boxes)))
        if (p < 0).any() or (p >= n_rel).any():
            raise ValueError("image_relations.pack: image %r: a predicate lies outside [0, %d)" % (key, n_rel))
        if not np.isfinite(boxes).all():
            raise ValueError("image_relations.pack: image %r: an annotated coordinate is not finite" % (key,))
        trip = np.stack([cls[s].astype(np.int64), p, cls[o].astype(np.int64)], 1)
        g_trip.append(trip.astype(np.int32))
        g_box.append(np.hstack([boxes[s], boxes[o]]))
        g_zs.append(np.zeros(len(trip), np.int32) if seen is None
                    else np.asarray([0 if tuple(t) in seen else 1 for t in trip.tolist()], np.int32))
        g_n.append(len(trip))
        got = _image_predictions(key, relations.get(key), max_pred, k_per_pair)
        if got is None:
            p_n.append(0)
            before.append(0)
            continue
        p_trip.append(got[0]), p_box.append(got[1]), p_conf.append(got[2]), p_row.append(got[3])
        p_n.append(len(got[0]))
        before.append(got[4])
    pred_off, gt_off = (offsets(n, "image_relations.pack: too many rows") for n in (p_n, g_n))
    return Packed(keys=keys, n_ignored=n_ignored, n_rel=n_rel, max_pred=max_pred, pred_off=pred_off, gt_off=gt_off,
                  pred_trip=cat(p_trip, (3,), np.int32), pred_box=cat(p_box, (8,), np.float64), pred_conf=cat(p_conf, (), np.float32),
                  pred_row=cat(p_row, (), np.int32), n_before_cut=np.asarray(before, np.int32),
                  gt_trip=cat(g_trip, (3,), np.int32), gt_box=cat(g_box, (8,), np.float64), gt_zs=cat(g_zs, (), np.int32))


# ------------------------------------------------------------------------------------------------------------------
# host form
# ------------------------------------------------------------------------------------------------------------------
def _union(box8):
    return np.stack([np.minimum(box8[:, 0], box8[:, 4]), np.minimum(box8[:, 1], box8[:, 5]),
                     np.maximum(box8[:, 2], box8[:, 6]), np.maximum(box8[:, 3], box8[:, 7])], 1)


def scores_host(pred_trip, pred_box, gt_trip, gt_box):
    """(2, n_pred, n_gt) float64: ``ov`` of one image in relation and in phrase mode, -1 where the triplets differ."""
    same = (pred_trip[:, None, :] == gt_trip[None, :, :]).all(2)
    rel = np.minimum(overlap_plus1(pred_box[:, :4], gt_box[:, :4]), overlap_plus1(pred_box[:, 4:], gt_box[:, 4:]))
    phr = overlap_plus1(_union(pred_box), _union(gt_box))
    return np.stack([np.where(same, rel, -1.0), np.where(same, phr, -1.0)])


def match_host(pk, iou_threshold=0.5):
    """The rules of ``ops.image_relation_match`` in numpy, on the same arrays: (hit (2, n_pred) int32, hit_ov (2, n_pred)
    float64, gt_rank (2, n_gt) int32), mode 0 relation and 1 phrase."""
    n_pred, n_gt = len(pk.pred_trip), len(pk.gt_trip)
    thr = np.float64(iou_threshold)
    hit = np.full((2, n_pred), -1, np.int32)
    hit_ov = np.full((2, n_pred), -1.0, np.float64)
    gt_rank = np.full((2, n_gt), -1, np.int32)
    for i in range(len(pk.pred_off) - 1):
        p0, p1, g0, g1 = int(pk.pred_off[i]), int(pk.pred_off[i + 1]), int(pk.gt_off[i]), int(pk.gt_off[i + 1])
        if p1 == p0 or g1 == g0:
            continue
        same = (pk.pred_trip[p0:p1, None, :] == pk.gt_trip[None, g0:g1, :]).all(2)
        if not same.any():
            continue
        ov2 = scores_host(pk.pred_trip[p0:p1], pk.pred_box[p0:p1], pk.gt_trip[g0:g1], pk.gt_box[g0:g1])
        for m in range(2):
            ov = ov2[m]
            cand = same & (ov >= thr)
            free = np.ones(g1 - g0, bool)
            for q in np.nonzero(cand.any(1))[0].tolist():
                row = np.where(cand[q] & free, ov[q], -1.0)
                g = int(np.argmax(row))                          # the first of equal maxima: the lower index
                if not (cand[q, g] and free[g]):
                    continue
                free[g] = False
                hit[m, p0 + q], hit_ov[m, p0 + q], gt_rank[m, g0 + g] = g, ov[q, g], q
    return hit, hit_ov, gt_rank


def count_host(pk, gt_rank, nreturns):
    """The rules of ``ops.image_relation_count`` in numpy: (totals (2, K, 2), zs_totals (2, K, 2), per_predicate (2, K, n_rel,
    2)) int64, hits and ground truths."""
    ks = _nreturns(nreturns)
    K, R = len(ks), pk.n_rel
    totals, zs_totals = np.zeros((2, K, 2), np.int64), np.zeros((2, K, 2), np.int64)
    per_predicate = np.zeros((2, K, R, 2), np.int64)
    pred = pk.gt_trip[:, 1].astype(np.int64)
    zs = pk.gt_zs != 0
    for m in range(2):
        for j, k in enumerate(ks):
            h = (gt_rank[m] >= 0) & (gt_rank[m] < k)
            totals[m, j] = h.sum(), len(h)
            zs_totals[m, j] = (h & zs).sum(), zs.sum()
            per_predicate[m, j, :, 0] = np.bincount(pred[h], minlength=R)
            per_predicate[m, j, :, 1] = np.bincount(pred, minlength=R)
    return totals, zs_totals, per_predicate


# ------------------------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------------------------
def evaluate_packed(pk, nreturns=(50, 100), iou_threshold=0.5, device=None):
    """(hit, hit_ov, gt_rank, totals, zs_totals, per_predicate) of packed arrays as numpy arrays, on the host
    (``device=None``) or by the kernels."""
    if not float(iou_threshold) > 0.0:
        raise ValueError("image_relations: iou_threshold must be positive (got %r)" % (iou_threshold,))
    if device is None:
        hit, hit_ov, gt_rank = match_host(pk, iou_threshold)
        return (hit, hit_ov, gt_rank) + count_host(pk, gt_rank, nreturns)
    from . import ops
    ks = _nreturns(nreturns)
    hit, hit_ov, gt_rank = ops.image_relation_match(pk.pred_off, pk.gt_off, pk.pred_trip, pk.pred_box, pk.gt_trip, pk.gt_box,
                                                    iou_threshold, device=device)
    counters = ops.image_relation_count(gt_rank, pk.gt_trip, pk.gt_zs, ks, pk.n_rel, device=device)
    return tuple(t.cpu().numpy() for t in (hit, hit_ov, gt_rank) + tuple(counters))


def _ratio(hits, total):
    return np.float64(hits) / np.float64(total) if total else np.float64("nan")


def result_of(pk, nreturns, totals, zs_totals, per_predicate):
    ks = _nreturns(nreturns)
    res = {}
    for m, mode in enumerate(MODES):
        r = {"recall": {}, "zero_shot_recall": {}, "mean_recall": {}, "totals": {}, "zs_totals": {}, "per_predicate": {}}
        for j, k in enumerate(ks):
            r["totals"][k] = (int(totals[m, j, 0]), int(totals[m, j, 1]))
            r["zs_totals"][k] = (int(zs_totals[m, j, 0]), int(zs_totals[m, j, 1]))
            r["per_predicate"][k] = np.array(per_predicate[m, j], np.int64)
            r["recall"][k] = _ratio(*r["totals"][k])
            r["zero_shot_recall"][k] = _ratio(*r["zs_totals"][k])
            acc, n = np.float64(0.0), 0
            for p in range(pk.n_rel):                            # added in predicate order
                if per_predicate[m, j, p, 1]:
                    acc = acc + np.float64(per_predicate[m, j, p, 0]) / np.float64(per_predicate[m, j, p, 1])
                    n += 1
            r["mean_recall"][k] = acc / np.float64(n) if n else np.float64("nan")
        res[mode] = r
    res.update(n_images=len(pk.keys), n_gt=int(len(pk.gt_trip)), n_gt_zero_shot=int((pk.gt_zs != 0).sum()), n_ignored=int(pk.n_ignored))
    return res


def evaluate(relations, annotations, n_rel, nreturns=(50, 100), iou_threshold=0.5, k_per_pair=None, seen_triplets=None, device=None):
    """Recall@K, zero-shot recall@K and mean (per-predicate) recall@K of ``relations`` against ``annotations`` in relation and
    in phrase mode (the module docstring has the rules and the layout of the result).  ``device=None``: everything on the host."""
    pk = pack(relations, annotations, n_rel, nreturns, k_per_pair, seen_triplets)
    out = evaluate_packed(pk, nreturns, iou_threshold, device)
    return result_of(pk, nreturns, *out[3:])


def report(result, out=print):
    for mode in MODES:
        r = result[mode]
        for k in sorted(r["recall"]):
            out("{} detection R@{}: {:.4f} ({} of {})   zero-shot R@{}: {:.4f} ({} of {})   mean R@{}: {:.4f}".format(
                mode, k, r["recall"][k], r["totals"][k][0], r["totals"][k][1], k, r["zero_shot_recall"][k], r["zs_totals"][k][0],
                r["zs_totals"][k][1], k, r["mean_recall"][k]))
    out("{} images, {} ground truths ({} zero-shot), {} predicted images without annotation ignored".format(
        result["n_images"], result["n_gt"], result["n_gt_zero_shot"], result["n_ignored"]))


def to_json(result):
    """The result with string keys and plain numbers (a nan is written as null)."""
    num = lambda x: None if np.isnan(x) else float(x)
    out = {}
    for mode in MODES:
        r = result[mode]
        out[mode] = {"recall": dict((str(k), num(v)) for k, v in r["recall"].items()),
                     "zero_shot_recall": dict((str(k), num(v)) for k, v in r["zero_shot_recall"].items()),
                     "mean_recall": dict((str(k), num(v)) for k, v in r["mean_recall"].items()),
                     "totals": dict((str(k), list(v)) for k, v in r["totals"].items()),
                     "zs_totals": dict((str(k), list(v)) for k, v in r["zs_totals"].items()),
                     "per_predicate": dict((str(k), np.asarray(v).tolist()) for k, v in r["per_predicate"].items())}
    out.update((k, int(result[k])) for k in ("n_images", "n_gt", "n_gt_zero_shot", "n_ignored"))
    return out
