"""Bounding-box voting (Gidaris & Komodakis, "Object detection via a multi-region & semantic segmentation-aware CNN model",
ICCV 2015; Detectron's ``TEST.BBOX_VOTE``) for the detection test loop: after NMS -- greedy or soft -- each kept box is replaced
by the score-weighted mean of all candidates of its class that overlap it, so the boxes the NMS used to suppress or decay lend
their coordinates instead of being thrown away.  The reference has none; like Soft-NMS (``soft_nms.py``) it is built to the rules
below, and the host form in this module (plain numpy) is the specification.  There is no device form in the library yet
(DESIGN.md 7n says why); ``box_vote_host`` refines a frame's ``all_boxes`` on the host, and a device kernel is to be tested
against it.

The rules
---------
Input, per set (one class of one frame).  *Kept* rows ``[x1, y1, x2, y2, score]`` in float32 with a count, and *candidate* rows
``[x1, y1, x2, y2, score]`` in float32 with a count, as ``det_gather_kernel`` leaves them: thresholded, in descending score
order.  Rows past a count are ignored.  Candidate scores are strictly positive (inside the post-processing: ``score_thresh >= 0``,
anything else is an argument error when voting is on).  Coordinates are finite with ``x2 >= x1 - 1`` and ``y2 >= y1 - 1``.

IoU.  ``soft_nms.iou_row``, imported, not restated: float32, one rounding per operation, ``+ 1`` extents,
``inter / ((area_k + area_c) - inter)``.

Vote.  Candidate ``c`` votes for kept row ``k`` iff ``iou(k, c) >= vote_thresh``; ``vote_thresh`` is a float32 value, 0.8 by
default (Detectron's ``VOTE_TH``).  The comparison is ``>=``, so a NaN IoU does not vote.

New box.  For each coordinate ``q``: ``(float)(sum_c (double)s_c * (double)q_c / sum_c (double)s_c)``, the sums over the voters
in float64.  The host form adds in ascending candidate row order; the device may add in any fixed order.

Score.  Unchanged (Detectron's scoring method ``ID``): the order of the rows, their count and the image-wide ``max_per_image`` cut
are untouched.  Other scoring methods are out of scope.

No voter.  The row keeps its bits.  That happens only to a zero-area kept box, whose IoU with itself is 0 / 0.

Capacity.  A device form takes at most 4096 candidates per set, as Soft-NMS does; more is an argument error, never another route.
The host form has no limit, but the exactness bound below is derived for that many.

Exactness.  Each product ``s_c * q_c`` of two float32 values is exact in float64.  A float64 sum of n <= 4096 non-negative terms
has relative error <= (n - 1) 2^-53 whatever the order -- so has a sum of terms of one sign, and for coordinates of mixed sign the
same bound holds relative to the sum of magnitudes -- hence the quotient of two such sums lies within a few times
4096 * 2^-53 ~ 2^-40 of the exact value, and rounding it to float32 once leaves device and host at most 1 float32 ulp apart
(and apart at all only where the exact value sits within 2^-40 of a rounding boundary).  Scores, counts and row order are
bit-equal, and two runs on the device give the same bits: the reduction order is fixed and there is no floating-point atomic.
A kept row whose only voter is itself keeps its bits too: ``s * q`` is exact, and the correctly rounded quotient of ``s q`` by
``s`` is ``q``."""
import numpy as np

from .soft_nms import iou_row

F32 = np.float32
VOTE_THRESH = 0.8
MAX_CANDIDATES = 4096


def options(spec):
    """None -> None (off); a number t with 0 < t <= 1 -> the float32 threshold as a Python float."""
    if spec is None:
        return None
    if isinstance(spec, (bool, str)) or not np.isscalar(spec):
        raise ValueError("bbox_vote: None or a threshold in (0, 1], not %r" % (spec,))
    t = float(F32(spec))
    if not 0.0 < t <= 1.0:
        raise ValueError("bbox_vote: the threshold must be in (0, 1], not %r" % (spec,))
    return t


def _areas(boxes):
    with np.errstate(all="ignore"):
        return (boxes[:, 2] - boxes[:, 0] + F32(1)) * (boxes[:, 3] - boxes[:, 1] + F32(1))


def _one_set(kept, cands, thresh, stats):
    """kept (k, 5), cands (c, 5) -> the voted rows (k, 5)."""
    out = kept.copy()
    k, c = len(kept), len(cands)
    if not k or not c:
        if stats is not None:
            stats["voters"].append(np.zeros(k, np.int64))
        return out
    # one table of boxes: the kept row behind the candidates, so that iou_row(table, area, c) is IoU(kept, every candidate)
    table = np.concatenate([cands[:, :4], kept[:1, :4]], 0)
    area = _areas(table)
    s64 = cands[:, 4].astype(np.float64)
    voters = np.zeros(k, np.int64)
    for r in range(k):
        table[c] = kept[r, :4]
        area[c] = _areas(table[c:])[0]
        with np.errstate(all="ignore"):
            votes = np.nonzero(iou_row(table, area, c)[:c] >= thresh)[0]
        voters[r] = len(votes)
        if not len(votes):
            continue
        den = np.float64(0)
        num = np.zeros(4, np.float64)
        for i in votes:                                 # ascending candidate row order
            den = den + s64[i]
            num = num + s64[i] * cands[i, :4].astype(np.float64)
        out[r, :4] = (num / den).astype(F32)
    if stats is not None:
        stats["voters"].append(voters)
    return out


def box_vote_host(kept, kept_counts, cands, cand_counts, vote_thresh=VOTE_THRESH, stats=None):
    """The specification.  kept (n_set, n_kept, 5) or (n_kept, 5) float32 with kept_counts (n_set,) or None (all rows), cands
    (n_set, n_cand, 5) or (n_cand, 5) with cand_counts likewise -> out (n_set, n_kept, 5): a copy of ``kept`` whose valid rows
    carry the voted coordinates.  ``stats``: a dict that receives ``voters``, a list over the sets of the voters each valid
    kept row had."""
    kept, cands = np.asarray(kept, F32), np.asarray(cands, F32)
    if kept.ndim == 2:
        kept = kept[None]
    if cands.ndim == 2:
        cands = cands[None]
    n_set, n_kept, n_cand = kept.shape[0], kept.shape[1], cands.shape[1]
    if cands.shape[0] != n_set:
        raise ValueError("box_vote_host: %d kept sets, %d candidate sets" % (n_set, cands.shape[0]))
    kc = np.full(n_set, n_kept, np.int64) if kept_counts is None else np.asarray(kept_counts).reshape(n_set)
    cc = np.full(n_set, n_cand, np.int64) if cand_counts is None else np.asarray(cand_counts).reshape(n_set)
    thresh = F32(vote_thresh)
    out = kept.copy()
    if stats is not None:
        stats["voters"] = []
    for i in range(n_set):
        k = int(min(max(int(kc[i]), 0), n_kept))
        c = int(min(max(int(cc[i]), 0), n_cand))
        out[i, :k] = _one_set(kept[i, :k], cands[i, :c], thresh, stats)
    return out
