"""Proposal and detection recall: is every annotated object covered by some candidate box, and how well?  Recall at IoU
0.5 ... 0.95, the average recall (AR), per candidate budget (AR@10 / 100 / 300 / 1000 / all) and per object size -- the
standard metric of the Faster R-CNN code line (the reference carries it as the disabled block of lib/datasets/imdb.py next to
``create_roidb_from_box_list``).  Candidates are the RPN's proposals (``proposals.pkl`` of
``proposals_instance_styled.py``) or a detector's boxes (``detections.pkl``).

The rules, which the host form and the kernel (csrc/proposal_eval.hip) share:

* Inputs.  ``candidates[i]``: the candidate boxes of roidb image ``i``, (n, 4) or (n, >= 5), in the coordinates of the roidb
  boxes; row order is rank order, best first; only columns 0..3 are read.  The roidb entries hold ``boxes``, ``gt_classes``,
  ``gt_overlaps`` (dense or sparse) and, optionally, ``seg_areas``.
* Ground truths of an image: the rows with ``gt_classes > 0`` whose row maximum of ``gt_overlaps`` equals 1.  The area of one
  is ``seg_areas[row]`` as float64; an entry without ``seg_areas`` gives ``((x2 - x1) + 1) * ((y2 - y1) + 1)`` in float64.
* Area ranges, inclusive on both ends, float64 (``AREAS``): all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large
  [96^2, 1e10], 96-128, 128-256, 256-512, 512-inf [512^2, 1e10].  A box on a boundary belongs to both neighbouring ranges,
  as in the standard method.  A call names 1 to 8 ranges.
* Limits: 1 to 8 candidate budgets, each a positive int or ``None`` (all candidates).  For limit L the candidates of an
  image are its first ``min(n, L)`` rows.
* Overlap: ``packing.overlap_plus1`` / ``i2v_overlap_plus1`` -- float64, the +1 convention, an empty intersection gives 0.
  This is ``bbox_overlaps`` of lib/model/utils/bbox.pyx:15-61 in its own operation order: ``iw = (min(x2) - max(x1)) + 1``,
  ``ih`` likewise, nothing unless both are positive, else ``iw * ih / ((area_a + area_b) - iw * ih)``.  Boxes enter as
  ``float64(value)``: float32 or uint16 inputs convert exactly.  Coordinates must be finite.
* Cover.  For one (image, limit, area) cell with the ground truths g_0 .. g_{m-1} (those in range, in roidb row order) and the
  candidates c_0 .. c_{k-1}, repeat m times: among the ground truths not yet retired find the largest overlap with any
  candidate not yet retired; ties go to the lowest ground-truth position, then to the lowest candidate position (numpy
  ``argmax``'s first occurrence on both axes); record that overlap for that ground truth with the candidate's index and the
  step number; retire both.  An overlap of exactly 0 is still a valid maximum: it retires the lowest free candidate, as the
  standard loop does.  When no candidate is left (k < m, or k == 0) every remaining ground truth records overlap 0,
  candidate -1 and the step number it would have had, taken in ascending position.  The standard code asserts at this
  point; recording a miss instead is this project's rule.
* Metric, per (limit, area) cell: ``gt_overlaps`` = all recorded overlaps, sorted; ``num_pos`` their count; ``thresholds``
  = ``np.arange(0.5, 0.95 + 1e-5, 0.05)`` unless given; ``recalls[t] = count(gt_overlaps >= t) / float(num_pos)``; ``ar =
  recalls.mean()``.  ``num_pos == 0`` gives nan recalls, as the division does.  When the ``all`` range was requested the
  result also carries, per limit, the recall at IoU 0.5 per ground-truth class as integers: hits and counts.
* Limits of the implementation: at most ``MAX_GT`` ground truths and ``MAX_CAND`` candidates per image, ``MAX_LIMITS``
  limits, ``MAX_AREAS`` ranges, totals below 2^31.  Breaking one is a ``ValueError`` from ``pack``.

``device=None`` runs numpy only (this module imports without the library); given a device the cover runs on the GPU
(``ops.proposal_cover``) and everything after it is the same host code.  Both forms give the same bits.
"""
import numpy as np

from .packing import cat, offsets, overlap_plus1

MAX_GT = 4096                # ground truths of one image (csrc/proposal_eval.hip PE_MAXG)
MAX_CAND = 65535             # candidates of one image (PE_MAXC)
MAX_LIMITS = 8
MAX_AREAS = 8
NO_LIMIT = 2 ** 31 - 1       # how ``None`` travels in the int32 limits table

AREAS = {"all": (0.0, 1e10), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e10),
         "96-128": (96.0 ** 2, 128.0 ** 2), "128-256": (128.0 ** 2, 256.0 ** 2), "256-512": (256.0 ** 2, 512.0 ** 2),
         "512-inf": (512.0 ** 2, 1e10)}
DEFAULT_LIMITS = (10, 100, 300, 1000, None)
DEFAULT_AREAS = ("all", "small", "medium", "large")


class Packed(object):
    """Flat arrays of one evaluation (the layout of ``ops.proposal_cover``): cand_off (I + 1) int32, cand_box (N, 4) float64,
    gt_off (I + 1) int32, gt_box (G, 4) float64, gt_area (G) float64, gt_cls (G) int32, gt_row (G) int32 (the row in the image's
    roidb entry), limits (L) int32 (``None`` as 2^31 - 1), ranges (A, 2) float64; ``limit_names`` / ``area_names``: the limits
    and ranges as the call named them."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _dense(x):
    return np.asarray(x.toarray() if hasattr(x, "toarray") else x)


def pack(candidates, roidb, limits=DEFAULT_LIMITS, areas=DEFAULT_AREAS):
    limits, areas = list(limits), list(areas)
    if not 1 <= len(limits) <= MAX_LIMITS:
        raise ValueError("proposal_eval: a call names 1 to %d limits (got %d)" % (MAX_LIMITS, len(limits)))
    if not 1 <= len(areas) <= MAX_AREAS:
        raise ValueError("proposal_eval: a call names 1 to %d area ranges (got %d)" % (MAX_AREAS, len(areas)))
    lim = []
    for v in limits:
        if v is None:
            lim.append(NO_LIMIT)
        elif isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 < int(v) <= NO_LIMIT:
            lim.append(int(v))
        else:
            raise ValueError("proposal_eval: a limit is a positive int or None (got %r)" % (v,))
    for name in areas:
        if name not in AREAS:
            raise ValueError("proposal_eval: unknown area range %r (one of %s)" % (name, ", ".join(AREAS)))
    if len(candidates) != len(roidb):
        raise ValueError("proposal_eval: %d candidate arrays for %d roidb images" % (len(candidates), len(roidb)))
    c_parts, c_n = [], []
    g_box, g_area, g_cls, g_row, g_n = [], [], [], [], []
    for i, (cand, e) in enumerate(zip(candidates, roidb)):
        try:
            cand = np.asarray(cand)
        except ValueError:                               # rows of different lengths
            raise ValueError("proposal_eval: candidates[%d] must be (n, 4) or (n, >= 5) rows of x1 y1 x2 y2" % i)
        if cand.size == 0:
            cand = np.zeros((0, 4), np.float64)
        if cand.ndim != 2 or cand.shape[1] < 4 or cand.dtype == object:
            raise ValueError("proposal_eval: candidates[%d] must be (n, 4) or (n, >= 5) rows of x1 y1 x2 y2" % i)
        if cand.shape[0] > MAX_CAND:
            raise ValueError("proposal_eval: at most %d candidates of one image (image %d has %d)" % (MAX_CAND, i, cand.shape[0]))
        c_parts.append(cand[:, :4].astype(np.float64))
        c_n.append(cand.shape[0])
        boxes = np.asarray(e["boxes"]).astype(np.float64).reshape(-1, 4)
        cls = np.asarray(e["gt_classes"]).astype(np.int64).reshape(-1)
        ov = _dense(e["gt_overlaps"]).astype(np.float64)
        if len(boxes) != len(cls) or ov.size % max(len(cls), 1) or (len(cls) == 0 and ov.size):
            raise ValueError("proposal_eval: roidb[%d] boxes / gt_classes / gt_overlaps differ in length" % i)
        row_max = ov.reshape(len(cls), -1).max(axis=1) if ov.size else np.zeros(len(cls))
        rows = np.flatnonzero((cls > 0) & (row_max == 1))
        if len(rows) > MAX_GT:
            raise ValueError("proposal_eval: at most %d ground truths of one image (image %d has %d)" % (MAX_GT, i, len(rows)))
        b = boxes[rows]
        if e.get("seg_areas") is not None:
            area = np.asarray(e["seg_areas"]).astype(np.float64).reshape(-1)[rows]
        else:
            area = ((b[:, 2] - b[:, 0]) + 1.0) * ((b[:, 3] - b[:, 1]) + 1.0)
        g_box.append(b)
        g_area.append(area)
        g_cls.append(cls[rows])
        g_row.append(rows)
        g_n.append(len(rows))
    cand_box, gt_box = cat(c_parts, (4,), np.float64), cat(g_box, (4,), np.float64)
    if not (np.isfinite(cand_box).all() and np.isfinite(gt_box).all()):
        raise ValueError("proposal_eval: a box coordinate is not finite")
    gt_cls = cat(g_cls, (), np.int64)
    if len(gt_cls) and gt_cls.max() >= 2 ** 31:
        raise ValueError("proposal_eval: a class index is out of the int32 range")
    return Packed(cand_off=offsets(c_n, "proposal_eval: too many candidates"), cand_box=cand_box,
                  gt_off=offsets(g_n, "proposal_eval: too many ground truths"), gt_box=gt_box, gt_area=cat(g_area, (), np.float64),
                  gt_cls=gt_cls.astype(np.int32), gt_row=cat(g_row, (), np.int32), limits=np.asarray(lim, np.int32),
                  ranges=np.ascontiguousarray(np.asarray([AREAS[n] for n in areas], np.float64).reshape(-1, 2)),
                  limit_names=limits, area_names=areas)


# ------------------------------------------------------------------------------------------------------------------
# host form
# ------------------------------------------------------------------------------------------------------------------
def _sweep(G, C, g_free, c_free, n_steps):
    """The cover as a sweep: the (ground truth, candidate) pairs of an image lie in ``G`` / ``C`` in the order (overlap
    descending, ground truth ascending, candidate ascending); the pair the rules pick at every step is the first one whose ground
    truth and candidate are both still free.  Walks the list once, a block at a time, and returns the positions of the
    ``n_steps`` picks; ``g_free`` / ``c_free`` are updated in place."""
    picks, p, P, block = [], 0, len(G), 256
    while len(picks) < n_steps:
        if p >= P:
            raise AssertionError("proposal_eval: the pair list ended before the cover did")
        q = min(p + block, P)
        hit = np.flatnonzero(g_free[G[p:q]] & c_free[C[p:q]])
        if len(hit) == 0:
            p, block = q, min(block * 2, 1 << 16)
            continue
        h = p + int(hit[0])
        g_free[G[h]] = False
        c_free[C[h]] = False
        picks.append(h)
        p, block = h + 1, 256
    return picks


def cover_arrays_host(pk):
    """The rules of ``ops.proposal_cover`` in numpy, on the same arrays: (ov (L, A, G) float64, cand (L, A, G) int32, step (L, A,
    G) int32).  A ground truth outside the range of a cell holds -1 in all three."""
    L, A, NG = len(pk.limits), len(pk.ranges), len(pk.gt_area)
    ov_out = np.full((L, A, NG), -1.0, np.float64)
    cand_out = np.full((L, A, NG), -1, np.int32)
    step_out = np.full((L, A, NG), -1, np.int32)
    for i in range(len(pk.cand_off) - 1):
        c0, c1 = int(pk.cand_off[i]), int(pk.cand_off[i + 1])
        g0, g1 = int(pk.gt_off[i]), int(pk.gt_off[i + 1])
        n, ng = c1 - c0, g1 - g0
        if ng == 0:
            continue
        # every pair of the image once, ground-truth major, then a stable sort on the overlap: ties keep (ground truth, candidate)
        ov = overlap_plus1(pk.gt_box[g0:g1], pk.cand_box[c0:c1]).reshape(-1)
        order = np.argsort(-ov, kind="stable")
        G, C, OV = (order // max(n, 1)).astype(np.int64), (order % max(n, 1)).astype(np.int64), ov[order]
        area = pk.gt_area[g0:g1]
        for l in range(L):
            k = min(n, int(pk.limits[l]))
            for a in range(A):
                g_free = (area >= pk.ranges[a, 0]) & (area <= pk.ranges[a, 1])
                m = int(g_free.sum())
                if m == 0:
                    continue
                c_free = np.arange(n) < k
                picks = _sweep(G, C, g_free, c_free, min(m, k))
                o, c, s = ov_out[l, a, g0:g1], cand_out[l, a, g0:g1], step_out[l, a, g0:g1]
                if picks:
                    o[G[picks]], c[G[picks]], s[G[picks]] = OV[picks], C[picks], np.arange(len(picks))
                left = np.flatnonzero(g_free)                    # no candidate left: misses, in ascending position
                o[left], c[left], s[left] = 0.0, -1, len(picks) + np.arange(len(left))
    return ov_out, cand_out, step_out


# ------------------------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------------------------
def cover_arrays(pk, device=None):
    """(ov, cand, step) of packed arrays as numpy arrays, on the host (``device=None``) or by the kernel."""
    if device is None:
        return cover_arrays_host(pk)
    from . import ops
    return tuple(t.cpu().numpy() for t in ops.proposal_cover(pk.cand_off, pk.cand_box, pk.gt_off, pk.gt_box, pk.gt_area, pk.limits,
                                                             pk.ranges, device=device))


def default_thresholds():
    return np.arange(0.5, 0.95 + 1e-5, 0.05)


def metrics(pk, ov, thresholds=None, num_classes=None):
    """The metric of every (limit, area) cell from the cover's overlaps: what ``evaluate`` returns."""
    thresholds = default_thresholds() if thresholds is None else np.asarray(thresholds, np.float64).reshape(-1)
    res = {}
    inside = [(pk.gt_area >= lo) & (pk.gt_area <= hi) for lo, hi in pk.ranges]
    for l, limit in enumerate(pk.limit_names):
        for a, name in enumerate(pk.area_names):
            got = np.sort(ov[l, a][inside[a]])
            num_pos = len(got)
            recalls = np.zeros_like(thresholds)
            with np.errstate(divide="ignore", invalid="ignore"):
                for t, thr in enumerate(thresholds):
                    recalls[t] = np.float64((got >= thr).sum()) / float(num_pos)
                ar = recalls.mean() if len(recalls) else np.float64(np.nan)
            res[(limit, name)] = {"ar": ar, "recalls": recalls, "thresholds": thresholds, "gt_overlaps": got, "num_pos": num_pos}
    per_class = {}
    if "all" in pk.area_names:
        a = pk.area_names.index("all")
        n_cls = int(num_classes) if num_classes is not None else (int(pk.gt_cls.max()) + 1 if len(pk.gt_cls) else 1)
        for l, limit in enumerate(pk.limit_names):
            counts = np.bincount(pk.gt_cls[inside[a]], minlength=n_cls).astype(np.int64)
            hits = np.bincount(pk.gt_cls[inside[a] & (ov[l, a] >= 0.5)], minlength=n_cls).astype(np.int64)
            per_class[limit] = {"hits": hits, "counts": counts}
    res["per_class"] = per_class
    return res


def evaluate(candidates, roidb, limits=DEFAULT_LIMITS, areas=DEFAULT_AREAS, thresholds=None, device=None, num_classes=None):
    """Returns a dict keyed by (limit, area name), each holding ``ar``, ``recalls``, ``thresholds``, ``gt_overlaps`` (sorted) and
    ``num_pos``, and under ``"per_class"``, when the ``all`` range was requested, {limit: {"hits", "counts"}}: int64 arrays over
    the class index (``num_classes`` entries; by default up to the largest annotated class) of the ground truths covered at IoU
    >= 0.5 and of all ground truths."""
    pk = pack(candidates, roidb, limits, areas)
    ov, _, _ = cover_arrays(pk, device)
    return metrics(pk, ov, thresholds, num_classes)


def candidates_from_detections(all_boxes):
    """``all_boxes[class][image]`` (n, 5) rows of x1 y1 x2 y2 score -> per image the detections of all foreground classes
    concatenated in class order and sorted by score descending (a stable sort)."""
    n_images = len(all_boxes[1]) if len(all_boxes) > 1 else 0
    out = []
    for i in range(n_images):
        rows = [np.asarray(all_boxes[c][i], np.float64).reshape(-1, 5) for c in range(1, len(all_boxes)) if len(all_boxes[c][i])]
        d = np.concatenate(rows) if rows else np.zeros((0, 5), np.float64)
        out.append(d[np.argsort(-d[:, 4], kind="stable")])
    return out


def _is_rows(x):
    """One image's candidates: (n, >= 4) numbers (an array or a list of rows), or nothing."""
    try:
        a = np.asarray(x, np.float64)
    except (ValueError, TypeError):                      # lists of arrays of different lengths: a class of all_boxes
        return False
    return (a.ndim == 2 and a.shape[1] >= 4) or (a.ndim == 1 and a.size == 0)


def load_candidates(path):
    """A ``proposals.pkl`` (one entry per image: (n, >= 4) rows, an array or a list of rows) or a ``detections.pkl``
    (``all_boxes[class][image]``, (n, 5) rows) -> the per-image candidate list.  The layout is told by depth: every entry of a
    proposals file is itself a table of rows, an entry of ``all_boxes`` is a list of such tables."""
    import pickle
    with open(path, "rb") as f:
        obj = pickle.load(f)
    if all(_is_rows(x) for x in obj):
        return [np.asarray(x, np.float64).reshape(len(x), -1) if len(x) else np.zeros((0, 4), np.float64) for x in obj]
    if all(isinstance(x, (list, tuple)) and all(_is_rows(d) for d in x) for x in obj):
        return candidates_from_detections(obj)
    raise ValueError("proposal_eval: %s holds neither a list of (n, >= 4) arrays nor all_boxes[class][image]" % path)


def _label(limit):
    return "all" if limit is None else str(limit)


def report(result, out=print):
    """One line per (limit, area): AR, the recall at the threshold nearest IoU 0.5 and the number of ground truths."""
    for key, r in result.items():
        if key == "per_class":
            continue
        thr = r["thresholds"]
        at = int(np.argmin(np.abs(thr - 0.5))) if len(thr) else None
        out("AR@%-5s %-8s = %.4f   recall@%.2f = %.4f   (%d ground truths)"
            % (_label(key[0]), key[1], r["ar"], thr[at] if at is not None else 0.5, r["recalls"][at] if at is not None else np.nan,
               r["num_pos"]))


def to_json(result):
    """The result as plain lists and numbers (a nan is written as null)."""
    num = lambda x: None if np.isnan(x) else float(x)
    cells = [{"limit": _label(k[0]), "area": k[1], "ar": num(r["ar"]), "recalls": [num(x) for x in r["recalls"]],
              "thresholds": [float(x) for x in r["thresholds"]], "num_pos": int(r["num_pos"])}
             for k, r in result.items() if k != "per_class"]
    per_class = dict((_label(k), {"hits": v["hits"].tolist(), "counts": v["counts"].tolist()}) for k, v in result["per_class"].items())
    return {"cells": cells, "per_class": per_class}
