"""Soft-NMS (Bodla et al., "Soft-NMS -- Improving Object Detection With One Line of Code", ICCV 2017) for the detection test
loop: overlapping detections of a class have their scores decayed instead of being deleted.  The reference has none; like
Seq-NMS (``seqnms.py``) it is built to the rules below, and the host form in this module (plain numpy) is the specification
the device kernel (``csrc/soft_nms.hip``, ``ops.soft_nms``, ``ops.detection_postprocess(soft_nms=...)``) is tested against.

The rules
---------
Input.  A *set* is up to ``n`` rows ``[x1, y1, x2, y2, score]`` in float32 with a valid count; rows past the count are
ignored.  Rows arrive as ``det_gather_kernel`` leaves them: descending score, equal scores in ascending roi index.  Boxes and
scores are finite and boxes have non-negative extents (``x2 >= x1 - 1``, ``y2 >= y1 - 1``: zero area is allowed).

IoU.  The arithmetic of the reference's ``nms_cpu.py:14-29``: float32, one rounding per operation, ``+ 1`` on widths and
heights, ``inter / ((area_m + area_i) - inter)``.  Two zero-area boxes give 0 / 0: that NaN compares false with ``> Nt`` and
applies no decay under any method.

Loop.  While live rows remain:

1. pick the live row ``m`` with the largest current score; on equal scores (``-0 == +0``) the lowest input row wins;
2. emit ``m`` with its current score (a zero is emitted as ``+0``) and retire it;
3. apply the method's decay to every other live row ``i``, with ``iou = IoU(m, i)``:
   ``hard``: if ``iou > Nt`` the row is dropped;
   ``linear``: if ``iou > Nt``, ``s_i = s_i * (1.0f - iou)`` in float32;
   ``gaussian``: always, ``s_i = (float)((double)s_i * exp(-((double)iou * (double)iou) / (double)sigma))`` -- the weight in
   float64, rounded once (``sigma`` itself is a float32 value, as the C-ABI carries it);
4. a row a decay has just been applied to is dropped if ``s_i < min_score``.  A row no decay was applied to is never dropped.

Defaults: ``Nt = cfg.TEST.NMS``, ``sigma = 0.5``, ``min_score = 0.001``.

Output.  Per set the emitted rows in emission order with their final scores, the input row each came from, their count.
Scores only fall, so the emitted scores are non-increasing: ``dets[j, :counts[j]]`` stays in descending score order.

Capacity.  ``n <= 4096`` rows per set on the device (300 at test time, the reference's large-scale 1000, the training 2000);
more is an argument error, never another route.

Exactness.  ``hard`` and ``linear`` hold no transcendental: device and host agree bit for bit.  ``gaussian`` takes a float64
``exp``; the device's and numpy's may differ in the last float64 bit, which moves the float32 product by at most one ulp per
decay, so the requirement is the same rows in the same order and ``|s_dev - s_host| <= d * 2^-23 * s_host`` for a row that
received ``d`` decays.  ``d`` counts the decays whose weight is not exactly 1 (``iou != 0``: ``exp(-0.0)`` is 1 on both
sides, and such a decay leaves the bits alone).  The order comparison means something only where no decision of the host
form sits within that error: ``stats`` records, as ``video._note`` does, the smallest relative gap between the picked score
and any other live score at a pick (``pick_gap``) and between a decayed score and ``min_score`` (``min_score_gap``); a pair
of rows that have both received no inexact decay is left out (their scores are the same bits on the device).  A test case
is fit for the order comparison when both gaps exceed ``n * 2^-22``."""
import collections

import numpy as np

F32 = np.float32
METHODS = ("hard", "linear", "gaussian")           # I2V_SOFT_NMS_HARD / _LINEAR / _GAUSSIAN
MAX_ROWS = 4096

SoftNMS = collections.namedtuple("SoftNMS", "method sigma min_score")
SoftNMS.__new__.__defaults__ = (0.5, 0.001)


def options(spec):
    """None / "off" -> None; a method name, a (method, sigma, min_score) triple or a ``SoftNMS`` -> ``SoftNMS``."""
    if spec is None or spec == "off":
        return None
    opt = SoftNMS(spec) if isinstance(spec, str) else SoftNMS(*spec)
    if opt.method not in METHODS:
        raise ValueError("soft_nms: method %r is none of %s" % (opt.method, ", ".join(METHODS)))
    if not float(opt.sigma) > 0.0:
        raise ValueError("soft_nms: sigma must be positive")
    return SoftNMS(opt.method, float(opt.sigma), float(opt.min_score))


def margin(n):
    """The relative gap a decision of the host form must keep for the device's gaussian order to be comparable."""
    return n * 2.0 ** -22


def _note(stats, key, value):
    if stats is not None and value < stats.get(key, np.inf):
        stats[key] = float(value)


def iou_row(boxes, area, m):
    """IoU of row m against every row: nms_cpu.py:20-29 in float32, one rounding per operation."""
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        w = np.fmax(zero, np.fmin(boxes[m, 2], boxes[:, 2]) - np.fmax(boxes[m, 0], boxes[:, 0]) + one)
        h = np.fmax(zero, np.fmin(boxes[m, 3], boxes[:, 3]) - np.fmax(boxes[m, 1], boxes[:, 1]) + one)
        inter = w * h
        iou = inter / ((area[m] + area) - inter)
    assert iou.dtype == F32
    return iou


def _one_set(rows, method, nt, sigma, min_score, stats):
    """(emitted rows (k, 5), their input rows (k,), the inexact decays each received (k,))."""
    n = rows.shape[0]
    boxes = np.ascontiguousarray(rows[:, :4])
    s = rows[:, 4].copy()
    with np.errstate(all="ignore"):
        area = (boxes[:, 2] - boxes[:, 0] + F32(1)) * (boxes[:, 3] - boxes[:, 1] + F32(1))
    live = np.ones(n, bool)
    decays = np.zeros(n, np.int64)
    out, src = [], []
    nt, min_score, sig = F32(nt), F32(min_score), np.float64(F32(sigma))
    for _ in range(n):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        m = int(idx[np.argmax(s[idx])])                     # argmax: the first of equal maxima, the lowest row
        if stats is not None and len(idx) > 1:
            rest = idx[idx != m]
            rest = rest[(decays[rest] > 0) | (decays[m] > 0)]
            if len(rest):
                ref = abs(float(s[m])) or 1.0
                _note(stats, "pick_gap", (float(s[m]) - float(s[rest].max())) / ref)
        out.append(np.concatenate([boxes[m], [s[m] + F32(0)]]).astype(F32))
        src.append(m)
        live[m] = False
        iou = iou_row(boxes, area, m)
        with np.errstate(all="ignore"):
            if method == "gaussian":
                applied = live & ~np.isnan(iou)
                inexact = applied & (iou != 0)
                i64 = iou[inexact].astype(np.float64)
                s[inexact] = (s[inexact].astype(np.float64) * np.exp(-(i64 * i64) / sig)).astype(F32)
            else:
                applied = live & (iou > nt)
                inexact = applied
                if method == "linear":
                    s[applied] = s[applied] * (F32(1) - iou[applied])
        decays[inexact] += 1
        if method == "hard":
            live &= ~applied
        else:
            if stats is not None and inexact.any():
                ref = abs(float(min_score)) or 1.0
                _note(stats, "min_score_gap", float(np.abs(s[inexact].astype(np.float64) - float(min_score)).min()) / ref)
            live &= ~(applied & (s < min_score))
    k = len(out)
    return (np.stack(out) if k else np.zeros((0, 5), F32)), np.asarray(src, np.int32), decays[np.asarray(src, np.int64)] if k else np.zeros(0, np.int64)


def soft_nms_host(dets, counts, method, nt, sigma=0.5, min_score=0.001, stats=None):
    """The specification.  dets (n_set, n, 5) or (n, 5) float32, counts (n_set,) or None (all n rows) ->
    (out_dets (n_set, n, 5), out_src (n_set, n) int32, out_num (n_set,) int32): rows past ``out_num`` are zero / -1.
    ``stats``: a dict that receives ``pick_gap`` and ``min_score_gap`` (the smallest seen; absent: no such decision was made)
    and ``decays``, a list over the sets of the inexact decays each emitted row received."""
    if method not in METHODS:
        raise ValueError("soft_nms_host: method %r is none of %s" % (method, ", ".join(METHODS)))
    dets = np.asarray(dets, F32)
    if dets.ndim == 2:
        dets = dets[None]
    n_set, n = dets.shape[0], dets.shape[1]
    counts = np.full(n_set, n, np.int64) if counts is None else np.asarray(counts).reshape(n_set)
    out_dets = np.zeros((n_set, n, 5), F32)
    out_src = np.full((n_set, n), -1, np.int32)
    out_num = np.zeros(n_set, np.int32)
    if stats is not None:
        stats["decays"] = []
    for i in range(n_set):
        c = int(min(max(int(counts[i]), 0), n))
        rows, src, d = _one_set(dets[i, :c], method, nt, sigma, min_score, stats)
        out_dets[i, :len(src)], out_src[i, :len(src)], out_num[i] = rows, src, len(src)
        if stats is not None:
            stats["decays"].append(d)
    return out_dets, out_src, out_num


def postprocess_host(sorted_dets, counts, method, nt, sigma=0.5, min_score=0.001, max_per_image=100, stats=None):
    """Per class ``soft_nms_host`` on the thresholded, sorted rows (sorted_dets (C, R, 5), counts (C,)), then the image-wide cut
    of test_net_instance_styleD_bilinear.py:214-221 on the DECAYED scores: when more than ``max_per_image`` rows survive over all
    classes, those with score >= the ``max_per_image``-th largest stay.  Returns (dets (C, R, 5), counts (C,) int32)."""
    out, _, num = soft_nms_host(sorted_dets, counts, method, nt, sigma, min_score, stats)
    if max_per_image > 0:
        scores = np.concatenate([out[j, :num[j], 4] for j in range(out.shape[0])])
        if len(scores) > max_per_image:
            image_thresh = np.sort(scores)[-max_per_image]
            for j in range(out.shape[0]):
                keep = int((out[j, :num[j], 4] >= image_thresh).sum())      # non-increasing scores: a prefix
                out[j, keep:] = 0
                num[j] = keep
    return out, num
