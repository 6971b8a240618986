"""Trajectory-level average precision of object tracks (the VidOR / ImageNet-VID video object detection metric): the score
of the Seq-NMS stage (``seqnms.py``, ``track_detections.py``) against annotated object trajectories.

A predicted trajectory counts when its voluminal IoU (vIoU) with a not yet detected annotated trajectory of its class reaches
a threshold.  The reference has this rule for relation pairs only (lib/utils.py:221-295, ``viou`` / ``eval_detection_scores``;
``video.match`` here); single object tracks, and trajectories with gaps -- annotated objects leave the frame and come back --
are this module's.  The host form (``match_arrays_host``) follows the rules below and is their specification; the packed tables
and the fixed summation order are laid out so that a kernel can equal it bit for bit.  No such kernel is in the library yet:
a ``device`` other than None is refused, never served by the host form quietly.

The rules.

* Trajectory.  (video, class, score, frames, boxes): ``frames`` strictly ascending, gaps allowed, one box [x1, y1, x2, y2] per
  frame.  Boxes arrive as float32 or float64 and are widened to float64 exactly; everything that decides something is float64
  in the order written here.
* Volume.  The sum over a trajectory's frames of ``((x2 - x1) + 1) * ((y2 - y1) + 1)``, the +1 convention of the reference's
  ``viou`` (lib/utils.py:256-261).
* Intersection.  Over the frame numbers both trajectories hold, each such frame contributing ``max(0, (min(x2) - max(x1)) + 1)
  * max(0, (min(y2) - max(y1)) + 1)``.  ``ov = inter / ((vol_p + vol_g) - inter)``; 0 when the trajectories share no frame.
  For gap-free trajectories this is the reference's ``viou``.
* Summation order.  Both sums run over the elements of one trajectory in frame order -- the volume over its own frames, the
  intersection over the PREDICTION's frames, a frame the ground truth does not hold adding nothing.  Lane l of 64 adds the
  elements l, l + 64, l + 128, ... in that order, starting from 0.0; then the 64 partials are added in lane order 0, 1, ...,
  63, starting from 0.0 (``_lane_sum``: what a wave of 64 lanes computes without atomics).
* Cells and matching.  A cell is one (video, class).  Within a cell the predictions go in descending score, equal scores in
  packed order; each takes the not yet detected ground truth of largest ``ov >= threshold`` (the lowest index on equal ov),
  otherwise it is a false positive: ``eval_detection_scores`` with one trajectory instead of two.  Several thresholds are
  matched independently from one ``ov`` table.
* Metric.  Per class and threshold: all predictions of the class over all videos that have ground truth of any class, in
  descending score (stable in packed order), tp = hit or no hit, AP = ``video.voc_ap`` of ``video._prec_rec``.  ``mAP[thr]`` is
  the mean over the classes that have at least one ground-truth trajectory; ``mAP`` is its mean over the thresholds.  Trajectory
  recall per threshold is detected ground truths / ground truths, also by the ground truth's length in frames.
* Limits.  A cell has at most 4096 ground-truth trajectories (64 lanes x 64 bits, as ``VM_MAXG`` of csrc/video.hip), a
  trajectory at most 2^20 frames; ``pack`` raises ``ValueError`` naming the cell past either.  Boxes are finite with ``x2 >= x1``
  and ``y2 >= y1`` (so every volume is positive and no ov is nan), scores are finite.

What runs where.  Everything here is host code (numpy): packing, volumes, the ov table, the matching, the metric and the
conversions from the tree's file layouts.
"""
import numpy as np

from .packing import cat, offsets
from .video import _note, _prec_rec, voc_ap

MAX_GT = 4096                # ground-truth trajectories of one cell (64 lanes x 64 "detected" bits)
MAX_LEN = 1 << 20            # frames of one trajectory
DEFAULT_THRESHOLDS = (0.5, 0.7, 0.9)
DEFAULT_LENGTH_BUCKETS = (32, 128)


# ---------------------------------------------------------------------------------------------------------------------
# the tree's file layouts -> trajectories
# ---------------------------------------------------------------------------------------------------------------------
def from_seq_nms(all_boxes, tracks, frame_index, min_len=1):
    """``seqnms.seq_nms``'s result ``(all_boxes', tracks)`` with ``frame_index[i] = (vid, fno)`` as predicted trajectories
    {vid: [{"category": j, "score", "frames": [...], "boxes": [[x1, y1, x2, y2], ...], "tid"}, ...]}, per video in class order,
    then track id.  A track's score is the one its boxes share after ``avg`` / ``max`` rescoring: the first member's, and the
    others must equal it.  Tracks of fewer than ``min_len`` members are left out."""
    members = {}
    for j in range(len(all_boxes)):
        for i, (vid, fno) in enumerate(frame_index):
            c = np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)
            t = np.asarray(tracks[j][i]).reshape(-1)
            if len(c) != len(t):
                raise ValueError("track_eval.from_seq_nms: class %d, image %d has %d boxes and %d track ids" % (j, i, len(c), len(t)))
            for r in range(len(c)):
                members.setdefault(vid, {}).setdefault((j, int(t[r])), []).append((int(fno), c[r]))
    out = dict((vid, []) for vid, _ in frame_index)
    for vid, by_track in members.items():
        for (j, tid) in sorted(by_track):
            rows = sorted(by_track[(j, tid)], key=lambda m: m[0])
            if len(rows) < min_len:
                continue
            score = rows[0][1][4]
            assert all(m[1][4] == score for m in rows), "track (%r, %d, %d): its boxes do not share one score" % (vid, j, tid)
            out[vid].append({"category": j, "score": float(score), "frames": [m[0] for m in rows],
                             "boxes": [[float(x) for x in m[1][:4]] for m in rows], "tid": tid})
    return out


def from_frame_annotations(anno, frame_index_by_name):
    """The per-frame pickle layout of annotated and tracked boxes, {name: {"boxes", "box_classes", "tids", ...}}, as
    ground-truth trajectories {vid: [{"category", "frames", "boxes", "tid"}, ...]} grouped by (video, tid), per video in the
    order of each tid's first frame.  ``frame_index_by_name`` maps a name to (vid, fno): a dict or a callable.  A tid whose
    class changes inside a video, or that has two boxes in one frame, is a ``ValueError`` naming the frame."""
    look = frame_index_by_name if callable(frame_index_by_name) else frame_index_by_name.__getitem__
    frames = sorted(((look(name), name) for name in anno), key=lambda e: (str(e[0][0]), int(e[0][1])))
    out, by_tid = {}, {}
    for (vid, fno), name in frames:
        e = anno[name]
        boxes = np.asarray(e["boxes"], np.float64).reshape(-1, 4)
        classes, tids = list(e["box_classes"]), list(e["tids"])
        if not len(boxes) == len(classes) == len(tids):
            raise ValueError("track_eval.from_frame_annotations: frame %r has %d boxes, %d classes and %d tids"
                             % (name, len(boxes), len(classes), len(tids)))
        out.setdefault(vid, [])
        for b, c, t in zip(boxes.tolist(), classes, tids):
            c = c.item() if isinstance(c, np.generic) else c
            tr = by_tid.get((vid, int(t)))
            if tr is None:
                tr = by_tid[(vid, int(t))] = {"category": c, "frames": [], "boxes": [], "tid": int(t)}
                out[vid].append(tr)
            if tr["category"] != c:
                raise ValueError("track_eval.from_frame_annotations: tid %d of video %r changes its class from %r to %r in frame %r"
                                 % (int(t), vid, tr["category"], c, name))
            if tr["frames"] and tr["frames"][-1] == int(fno):
                raise ValueError("track_eval.from_frame_annotations: tid %d of video %r has two boxes in frame %r" % (int(t), vid, name))
            tr["frames"].append(int(fno))
            tr["boxes"].append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
class Packed(object):
    """Flat arrays of a batch of cells (offset tables, as the packed-table ops take them): trajectory t owns rows ``traj_off[t] ..
    traj_off[t + 1]`` of ``frame`` / ``box``, the ``n_pred`` predictions first, then the ``n_gt`` ground truths; cell c is
    ``cells[c] = (vid, category)`` and owns predictions ``cell_pred_off[c] ..`` and ground truths ``n_pred + cell_gt_off[c] ..``.
    ``pred_src[p]`` / ``gt_src[g]``: the trajectory's index in its video's list."""

    def __init__(self, cells, n_pred, n_gt, traj_off, frame, box, cell_pred_off, cell_gt_off, pred_score, pred_src, gt_src):
        self.cells, self.n_pred, self.n_gt, self.traj_off, self.frame, self.box = cells, n_pred, n_gt, traj_off, frame, box
        self.cell_pred_off, self.cell_gt_off, self.pred_score = cell_pred_off, cell_gt_off, pred_score
        self.pred_src, self.gt_src = pred_src, gt_src


def _trajectory(tr, cell, what):
    frames = np.asarray(tr["frames"], np.int64).reshape(-1)
    raw = np.asarray(tr["boxes"])
    if raw.dtype not in (np.float32, np.float64):
        raw = raw.astype(np.float64)
    boxes = raw.astype(np.float64).reshape(-1, 4)                # float32 widens exactly
    name = "%s of cell %r" % (what, cell)
    if len(frames) == 0 or len(frames) != len(boxes):
        raise ValueError("track_eval.pack: %s has %d frames and %d boxes (at least one, and as many)" % (name, len(frames), len(boxes)))
    if len(frames) > MAX_LEN:
        raise ValueError("track_eval.pack: %s has %d frames, at most %d" % (name, len(frames), MAX_LEN))
    if (np.diff(frames) <= 0).any() or frames[0] < -2 ** 31 or frames[-1] >= 2 ** 31:
        raise ValueError("track_eval.pack: the frames of %s are not strictly ascending int32" % name)
    if not np.isfinite(boxes).all() or (boxes[:, 2] < boxes[:, 0]).any() or (boxes[:, 3] < boxes[:, 1]).any():
        raise ValueError("track_eval.pack: %s holds a box that is not finite or has x2 < x1 or y2 < y1" % name)
    return frames.astype(np.int32), boxes


def pack(prediction, groundtruth):
    """``prediction`` {vid: [{"category", "score", "frames", "boxes"}, ...]} and ``groundtruth`` {vid: [{"category", "frames",
    "boxes"}, ...]} as ``Packed``.  Only the videos of ``groundtruth`` that have a trajectory take part, in its order; a video's
    cells are its classes in order of first appearance, ground truths first.  A cell may have no prediction or no ground truth."""
    cells, n_p, n_g = [], [], []
    pf, pb, gf, gb, score, pred_src, gt_src = [], [], [], [], [], [], []
    for vid, gts in groundtruth.items():
        if len(gts) == 0:
            continue
        preds = prediction.get(vid, [])
        by_class = {}
        for k, tr in enumerate(gts):
            by_class.setdefault(tr["category"], ([], []))[1].append(k)
        for k, tr in enumerate(preds):
            by_class.setdefault(tr["category"], ([], []))[0].append(k)
        for cat_, (pk_, gk_) in by_class.items():
            cell = (vid, cat_)
            if len(gk_) > MAX_GT:
                raise ValueError("track_eval.pack: cell %r has %d ground-truth trajectories, at most %d" % (cell, len(gk_), MAX_GT))
            cells.append(cell)
            n_p.append(len(pk_))
            n_g.append(len(gk_))
            for k in pk_:
                f, b = _trajectory(preds[k], cell, "prediction %d" % k)
                s = float(preds[k]["score"])
                if not np.isfinite(s):
                    raise ValueError("track_eval.pack: prediction %d of cell %r has a score that is not finite" % (k, cell))
                pf.append(f), pb.append(b), score.append(s), pred_src.append(k)
            for k in gk_:
                f, b = _trajectory(gts[k], cell, "ground truth %d" % k)
                gf.append(f), gb.append(b), gt_src.append(k)
    traj_off = offsets([len(f) for f in pf + gf], "track_eval.pack: more than 2^31 boxes")
    return Packed(cells, len(pf), len(gf), traj_off, cat(pf + gf, (), np.int32), cat(pb + gb, (4,), np.float64),
                  offsets(n_p, "track_eval.pack: more than 2^31 predictions"), offsets(n_g, "track_eval.pack: more than 2^31 ground truths"),
                  np.asarray(score, np.float64).reshape(-1), np.asarray(pred_src, np.int64), np.asarray(gt_src, np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the host form
# ---------------------------------------------------------------------------------------------------------------------
def _lane_sum(x):
    """The stated order: lane l of 64 adds x[l], x[l + 64], ... in order, then the 64 partials are added in lane order.  A lane
    whose turn has no element adds +0.0, which leaves a partial that started at +0.0 as it is."""
    n = len(x)
    rows = np.zeros(((n + 63) // 64, 64))
    rows.reshape(-1)[:n] = x
    part = np.zeros(64)
    for r in rows:                                               # an explicit loop: numpy's own reduction order is pairwise
        part = part + r
    total = 0.0
    for v in part.tolist():
        total += v
    return total


def _area_plus1(b):
    return ((b[:, 2] - b[:, 0]) + 1.0) * ((b[:, 3] - b[:, 1]) + 1.0)


def _inter(fp, bp, fg, bg):
    """(intersection, any common frame) of a prediction and a ground truth: a sparse join over the prediction's frames."""
    j = np.minimum(np.searchsorted(fg, fp), len(fg) - 1)
    found = fg[j] == fp
    if not found.any():
        return 0.0, False
    a, b = bp, bg[j]
    iw = (np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0])) + 1.0
    ih = (np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1])) + 1.0
    return _lane_sum(np.where(found, np.maximum(iw, 0.0) * np.maximum(ih, 0.0), 0.0)), True


def match_arrays_host(pk, thresholds=DEFAULT_THRESHOLDS, stats=None):
    """The rules of the module docstring in numpy, on the packed arrays: (vol (T), ov (n_pred, max_gt),
    hit (K, n_pred) int32, hit_ov (K, n_pred)).  ``stats`` (a dict) receives the smallest relative margin of an ov against any
    threshold (``ov``) and between two unequal qualifying ov that one prediction chooses from (``ov_gap``)."""
    thr = np.asarray(thresholds, np.float64).reshape(-1)
    counts = np.diff(pk.cell_gt_off)
    max_gt = int(counts.max()) if len(counts) else 0
    NP, T, K = pk.n_pred, len(pk.traj_off) - 1, len(thr)
    span = lambda t: slice(int(pk.traj_off[t]), int(pk.traj_off[t + 1]))
    area = _area_plus1(pk.box)
    vol = np.array([_lane_sum(area[span(t)]) for t in range(T)], np.float64).reshape(-1)
    ov = np.full((NP, max_gt), -1.0)
    hit, hit_ov = np.full((K, NP), -1, np.int32), np.full((K, NP), -1.0)
    for c in range(len(pk.cells)):
        p0, p1, g0, g1 = int(pk.cell_pred_off[c]), int(pk.cell_pred_off[c + 1]), int(pk.cell_gt_off[c]), int(pk.cell_gt_off[c + 1])
        for p in range(p0, p1):
            sp = span(p)
            for g in range(g0, g1):
                sg = span(NP + g)
                inter, shared = _inter(pk.frame[sp], pk.box[sp], pk.frame[sg], pk.box[sg])
                ov[p, g - g0] = inter / ((vol[p] + vol[NP + g]) - inter) if shared else 0.0
        order = p0 + np.argsort(-pk.pred_score[p0:p1], kind="stable")
        for k in range(K):
            taken = np.zeros(g1 - g0, bool)
            for p in order:
                row = ov[p, :g1 - g0]
                if stats is not None and len(row):
                    _note(stats, "ov", (np.abs(row - thr[k]) / max(abs(thr[k]), 1e-300)).min())
                    u = np.unique(row[(row >= thr[k]) & ~taken])
                    if len(u) > 1:
                        _note(stats, "ov_gap", (np.diff(u) / u[1:]).min())
                cand = (row >= 0) & (row >= thr[k]) & ~taken
                if cand.any():
                    g = int(np.where(cand, row, -1.0).argmax())      # the first maximum: the lowest index
                    taken[g] = True
                    hit[k, p], hit_ov[k, p] = g, row[g]
    return vol, ov, hit, hit_ov


def match_arrays(pk, thresholds=DEFAULT_THRESHOLDS, device=None, stats=None):
    """``match_arrays_host`` for ``device=None``.  The library has no kernel for these tables: any other device is an error."""
    if device is not None:
        raise NotImplementedError("track_eval: the matching has no device form in this library (got device %r); "
                                  "match_arrays_host is the host form: pass device=None" % (device,))
    return match_arrays_host(pk, thresholds, stats)


def match(prediction, groundtruth, thresholds=DEFAULT_THRESHOLDS, device=None, stats=None):
    """(Packed, vol, ov, hit, hit_ov): ``hit[k, p]`` is the index, within its cell, of the ground truth that prediction p
    detects at ``thresholds[k]``, or -1."""
    pk = pack(prediction, groundtruth)
    return (pk,) + tuple(match_arrays(pk, thresholds, device, stats))


# ---------------------------------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------------------------------
def _key(thr):
    return "%g" % thr


def _bucket_names(bounds):
    b = [int(x) for x in bounds]
    return ["<%d" % b[0]] + ["%d..%d" % (lo, hi - 1) for lo, hi in zip(b[:-1], b[1:])] + [">=%d" % b[-1]]


def evaluate(prediction, groundtruth, thresholds=DEFAULT_THRESHOLDS, length_buckets=DEFAULT_LENGTH_BUCKETS, device=None):
    """Trajectory mAP and recall as a plain dict (``json.dump`` takes it): ``thresholds``; ``classes`` (as strings, in order of
    first appearance) with ``n_gt`` / ``n_pred`` per class; ``ap`` {class: [AP per threshold], None for a class without ground
    truth}; ``mAP_at`` {threshold: mean over the classes with ground truth}; ``mAP`` (its mean over the thresholds); ``recall_at``
    {threshold: detected / ground truths}; ``recall_by_length`` {bucket: {"n_gt", "recall_at"}} with the buckets ``< b0``,
    ``b0 .. b1 - 1``, ..., ``>= b_last`` of the ground truth's length in frames."""
    thr = [float(t) for t in thresholds]
    bounds = sorted(int(b) for b in length_buckets)
    if not bounds:
        raise ValueError("track_eval.evaluate: at least one length bucket bound")
    pk, _, _, hit, _ = match(prediction, groundtruth, thr, device)
    K, NP = len(thr), pk.n_pred
    classes = []
    for _, c in pk.cells:
        if c not in classes:
            classes.append(c)
    cell_class = np.array([classes.index(c) for _, c in pk.cells], np.int64)
    pred_class = np.repeat(cell_class, np.diff(pk.cell_pred_off))
    gt_class = np.repeat(cell_class, np.diff(pk.cell_gt_off))
    gt_len = np.diff(pk.traj_off)[NP:]
    gt_bucket = np.searchsorted(np.asarray(bounds), gt_len, side="right")
    detected = np.zeros((K, pk.n_gt), bool)                      # per threshold: the ground truths some prediction took
    pred_cell = np.repeat(np.arange(len(pk.cells)), np.diff(pk.cell_pred_off))
    for k in range(K):
        p = np.nonzero(hit[k] >= 0)[0]
        detected[k, pk.cell_gt_off[pred_cell[p]] + hit[k, p]] = True
    ap, n_gt, n_pred = {}, {}, {}
    per_thr = [[] for _ in range(K)]
    for ci, c in enumerate(classes):
        mine = np.nonzero(pred_class == ci)[0]
        mine = mine[np.argsort(-pk.pred_score[mine], kind="stable")]
        ng = int((gt_class == ci).sum())
        n_gt[str(c)], n_pred[str(c)] = ng, int(len(mine))
        if ng == 0:
            ap[str(c)] = None                                    # without ground truth: not in the mean
            continue
        row = []
        for k in range(K):
            prec, rec = _prec_rec(hit[k, mine] >= 0, ng)
            row.append(float(voc_ap(rec, prec)))
            per_thr[k].append(row[-1])
        ap[str(c)] = row
    m_ap = [float(np.mean(x)) if x else 0.0 for x in per_thr]
    names = _bucket_names(bounds)
    by_len = {}
    for b, name in enumerate(names):
        sel = gt_bucket == b
        n = int(sel.sum())
        by_len[name] = {"n_gt": n, "recall_at": dict((_key(t), float(detected[k, sel].sum()) / n if n else None) for k, t in enumerate(thr))}
    return {"thresholds": thr, "classes": [str(c) for c in classes], "n_videos": len(set(v for v, _ in pk.cells)), "n_pred_total": NP,
            "n_gt_total": pk.n_gt, "n_gt": n_gt, "n_pred": n_pred, "ap": ap,
            "mAP_at": dict((_key(t), m_ap[k]) for k, t in enumerate(thr)), "mAP": float(np.mean(m_ap)) if m_ap else 0.0,
            "recall_at": dict((_key(t), float(detected[k].sum()) / pk.n_gt if pk.n_gt else 0.0) for k, t in enumerate(thr)),
            "recall_by_length": by_len}


def report(res, names=None):
    """Prints the per-class table and the summary line of ``evaluate``'s result.  ``names``: class id -> name."""
    thr = res["thresholds"]
    print("%-20s %6s %6s  %s" % ("class", "gt", "pred", "  ".join("AP@%-5s" % _key(t) for t in thr)))
    for c in res["classes"]:
        label = str(names[int(c)]) if names is not None else c
        row = res["ap"][c]
        cols = "  ".join("%8.4f" % x for x in row) if row is not None else "  ".join("%8s" % "-" for _ in thr)
        print("%-20s %6d %6d  %s" % (label[:20], res["n_gt"][c], res["n_pred"][c], cols))
    for name, b in res["recall_by_length"].items():
        print("recall, %-9s frames (%5d gt): %s" % (name, b["n_gt"], "  ".join(
            "@%s %s" % (k, "-" if v is None else "%.4f" % v) for k, v in b["recall_at"].items())))
    print("trajectory mAP %.4f (%s); recall %s; %d videos, %d predictions, %d ground truths" % (
        res["mAP"], "  ".join("@%s %.4f" % (k, v) for k, v in res["mAP_at"].items()),
        "  ".join("@%s %.4f" % (k, v) for k, v in res["recall_at"].items()), res["n_videos"], res["n_pred_total"], res["n_gt_total"]))
