"""Predicate recognition at the video level: track alignment and accuracy@1/5 (the pre_det branch of the reference's test
loop, test_net_SGG_emb.py:213-228 and :318-324; ``alignment`` lib/utils.py:529-568, ``evaluate_recognition`` :335-372).

The reference's ``alignment`` is commented out and returns two empty dicts; its commented body is taken as the specification
and ``evaluate_recognition``, which is live, literally.  The rules, stated once for the host form (``align_arrays_host``) and
the kernel (csrc/recognition.hip, ``ops.recognition_align``), which agree bit for bit:

* A frame's record is what ``eval.recognition_output`` returns: ``{"sub_scores" (P,C), "obj_scores" (P,C), "pre_scores" (P,R),
  "tids": [[subject_tid, object_tid]] * P}``, or ``{}``.  A row is ``[sub | obj | pre]`` of one pair, widened to float64.
* A segment is a unique (video, subject_tid, object_tid, start, end) of the ground truth, in first-seen order.  Its rows come
  from the frames ``start <= fno < end`` in ascending frame number whose ``tids`` holds ``[subject_tid, object_tid]`` (the first
  occurrence, as ``.index`` finds it).  A missing frame, an empty frame and a frame without the pair are skipped (the
  reference's commented loop would raise there; this rule is this project's).
* mean = the float64 sum of the segment's rows in that order, one add per row and column, divided once by their number:
  ``np.vstack(rows).mean(axis=0)``.
* Within each of the three column groups the columns are ranked by descending mean, the lower index first on equal values, and
  the first ``min(10, width)`` are kept (``np.argsort(-x)[:10]`` wherever that is well defined; unused slots are -1).
* One instance per ground-truth relation, in order: hit@n = the label is among the first n of its group's ranking;
  rel@1 = sub@1 * obj@1 * pre@1.  Several relations on one track pair share a segment and count once each.
* A segment without rows has count 0, mean 0 and ranking -1; its instances have no hits and are left out of every total.
* objects[n][c] = subject hits of the instances whose subject is c plus object hits of those whose object is c.
"""
import collections

import numpy as np

TOP = 10
NRETURNS = (1, 5)

Packed = collections.namedtuple("Packed", "rows seg_off seg_row inst n_classes n_rel segments inst_video n_videos_missing")


def _label(value, names, what):
    if isinstance(value, (int, np.integer)):
        if not 0 <= int(value) < len(names):
            raise ValueError("recognition.pack: %s label %d is outside [0, %d)" % (what, int(value), len(names)))
        return int(value)
    try:
        return list(names).index(value)
    except ValueError:
        raise ValueError("recognition.pack: unknown %s name %r" % (what, value)) from None


def _frame_rows(vid, fno, rec, C, R):
    """A frame's record, checked once: -> (tids as lists of two ints, rows (P, 2C+R) float64)."""
    where = "frame %s of video %s" % (fno, vid)
    try:
        tids = [[int(t[0]), int(t[1])] if len(t) == 2 else None for t in rec["tids"]]
    except (TypeError, ValueError, IndexError):
        tids = [None]
    if any(t is None for t in tids):
        raise ValueError("recognition.pack: %s: tids are [subject_tid, object_tid] per pair" % where)
    parts = [np.asarray(rec[k], np.float64) for k in ("sub_scores", "obj_scores", "pre_scores")]
    for a, w, k in zip(parts, (C, C, R), ("sub_scores", "obj_scores", "pre_scores")):
        if a.ndim != 2 or a.shape != (len(tids), w):
            raise ValueError("recognition.pack: %s: %s has shape %s for %d tids and width %d" % (where, k, a.shape, len(tids), w))
        if not np.isfinite(a).all():
            raise ValueError("recognition.pack: %s: %s holds a non-finite score (ranking needs a total order)" % (where, k))
    return tids, np.hstack(parts)


def pack(frame_recognitions, groundtruth, classes, predicates):
    """``frame_recognitions``: {vid: {fno (int or str): record or {}}}; ``groundtruth``: VidVRD-style {vid: [{"triplet": [s, p, o]
    (names or labels), "subject_tid", "object_tid", "duration": [start, end]}]}; ``classes`` (0: background) and
    ``predicates``: the names behind the labels.  -> ``Packed`` (the arrays of ``ops.recognition_align`` and what
    ``video_recognitions`` needs to name them).  Videos absent from the predictions are skipped and counted."""
    C, R = len(classes), len(predicates)
    rows, row_of, checked = [], {}, {}
    seg_of, segments, seg_off, seg_row, inst, inst_video = {}, [], [0], [], [], []
    missing = 0
    for vid, relations in groundtruth.items():
        if vid not in frame_recognitions:
            missing += 1
            continue
        frames = dict((int(k), v) for k, v in frame_recognitions[vid].items())
        for rel in relations:
            stid, otid = int(rel["subject_tid"]), int(rel["object_tid"])
            start, end = int(rel["duration"][0]), int(rel["duration"][1])
            key = (vid, stid, otid, start, end)
            if key not in seg_of:
                seg_of[key] = len(segments)
                segments.append(key)
                for fno in sorted(f for f in frames if start <= f < end):
                    rec = frames[fno]
                    if not rec:
                        continue
                    if (vid, fno) not in checked:
                        checked[(vid, fno)] = _frame_rows(vid, fno, rec, C, R)
                    tids, frame_rows = checked[(vid, fno)]
                    if [stid, otid] not in tids:
                        continue
                    pair = tids.index([stid, otid])
                    if (vid, fno, pair) not in row_of:
                        row_of[(vid, fno, pair)] = len(rows)
                        rows.append(frame_rows[pair])
                    seg_row.append(row_of[(vid, fno, pair)])
                seg_off.append(len(seg_row))
            s, p, o = rel["triplet"]
            inst.append([seg_of[key], _label(s, classes, "class"), _label(p, predicates, "predicate"), _label(o, classes, "class")])
            inst_video.append(vid)
    return Packed(np.array(rows, np.float64).reshape(len(rows), 2 * C + R), np.asarray(seg_off, np.int32),
                  np.asarray(seg_row, np.int32), np.asarray(inst, np.int32).reshape(len(inst), 4), C, R, segments, inst_video,
                  missing)


def align_arrays_host(pk):
    """The numpy form of the kernel's rules: the same float64 operations in the same order.  -> (mean (S,W) float64, count (S)
    int32, top (S,3,10) int32, hit (T,7) int32, totals (8) int64, per_class (C,2,2) int64)."""
    C, R = pk.n_classes, pk.n_rel
    W, S, T = 2 * C + R, len(pk.seg_off) - 1, len(pk.inst)
    mean = np.zeros((S, W), np.float64)
    count = np.diff(pk.seg_off).astype(np.int32)
    top = np.full((S, 3, TOP), -1, np.int32)
    for s in range(S):
        idx = pk.seg_row[pk.seg_off[s]:pk.seg_off[s + 1]]
        if len(idx) == 0:
            continue
        acc = pk.rows[idx[0]].copy()
        for r in idx[1:]:
            acc = acc + pk.rows[r]
        mean[s] = acc / np.float64(len(idx))
        for g, (off, width) in enumerate(((0, C), (C, C), (2 * C, R))):
            order = np.argsort(-mean[s, off:off + width], kind="stable")[:TOP]     # descending, the lower index first on ties
            top[s, g, :len(order)] = order
    hit = np.zeros((T, 7), np.int32)
    totals = np.zeros(8, np.int64)
    per_class = np.zeros((C, 2, 2), np.int64)
    if T:
        seg, ls, lp, lo = pk.inst.T
        aligned = count[seg] > 0
        tp = top[seg]                                                # (T, 3, 10); -1 equals no label
        for col, (g, lab) in enumerate(((0, ls), (1, lo), (2, lp))):
            for k, n in enumerate(NRETURNS):
                hit[:, 2 * col + k] = (tp[:, g, :n] == lab[:, None]).any(1) & aligned
        hit[:, 6] = hit[:, 0] * hit[:, 2] * hit[:, 4]
        totals[:7] = hit[aligned].sum(0)
        totals[7] = aligned.sum()
        for k in range(2):
            np.add.at(per_class[:, k, 0], ls[aligned], hit[aligned, k])
            np.add.at(per_class[:, k, 1], ls[aligned], 1)
            np.add.at(per_class[:, k, 0], lo[aligned], hit[aligned, 2 + k])
            np.add.at(per_class[:, k, 1], lo[aligned], 1)
    return mean, count, top, hit, totals, per_class


def align_arrays(pk, device):
    """The device form (``ops.recognition_align``), as numpy arrays."""
    from . import ops
    return tuple(t.cpu().numpy() for t in ops.recognition_align(pk.rows, pk.seg_off, pk.seg_row, pk.inst, pk.n_classes, pk.n_rel,
                                                                 device=device))


def _ratio(hits, total):
    return np.float64(hits) / np.float64(total) if total else np.float64("nan")      # np.mean([]) without the warning


def result_of(pk, totals, per_class):
    n = int(totals[7])
    res = {"sub": {}, "obj": {}, "pre": {}, "rel": {1: _ratio(totals[6], n)}, "objects": {1: {}, 5: {}}}
    for k, nre in enumerate(NRETURNS):
        res["sub"][nre], res["obj"][nre], res["pre"][nre] = (_ratio(totals[2 * j + k], n) for j in range(3))
        for c in range(1, pk.n_classes):
            res["objects"][nre][c] = _ratio(per_class[c, k, 0], per_class[c, k, 1])
    res.update(n_aligned=n, n_unaligned=len(pk.inst) - n, n_videos_missing=pk.n_videos_missing)
    return res


def evaluate(frame_recognitions, groundtruth, classes, predicates, device=None):
    """Accuracy@1/5 of subject, object and predicate, relationship accuracy@1 and per-class object accuracy of per-frame
    recognitions against video-level annotations.  ``device=None``: everything on the host."""
    pk = pack(frame_recognitions, groundtruth, classes, predicates)
    out = align_arrays_host(pk) if device is None else align_arrays(pk, device)
    return result_of(pk, out[4], out[5])


def video_recognitions(pk, mean):
    """{vid: [{"sub_score", "obj_score", "pre_score", "triplet": [s, p, o] labels}]}: the per-instance records the reference's
    ``evaluate_recognition`` takes (what its ``alignment`` was to return), one per instance of a segment with rows."""
    C = pk.n_classes
    count = np.diff(pk.seg_off)
    out = {}
    for (seg, ls, lp, lo), vid in zip(pk.inst.tolist(), pk.inst_video):
        if count[seg] == 0:
            continue
        m = np.asarray(mean[seg])
        out.setdefault(vid, []).append({"sub_score": m[:C], "obj_score": m[C:2 * C], "pre_score": m[2 * C:], "triplet": [ls, lp, lo]})
    return out


def report(result, classes, out=print):
    """The lines ``evaluate_recognition`` prints (:357-371), its spelling included."""
    for nre in NRETURNS:
        for c in range(1, len(classes)):
            out("object #{} acc@{} : {}".format(c, nre, result["objects"][nre][c]))
    for key, name in (("sub", "subject"), ("obj", "object"), ("pre", "predicate")):
        for nre in NRETURNS:
            out("{} recognition accurancy@{}: {}".format(name, nre, result[key][nre]))
    out("relationship recognition accurancy@1: {}".format(result["rel"][1]))


def to_json(result):
    """The result with string keys and plain floats (nan stays nan: json writes NaN, and reads it back)."""
    plain = lambda d: dict((str(k), float(v)) for k, v in d.items())
    out = dict((k, plain(result[k])) for k in ("sub", "obj", "pre", "rel"))
    out["objects"] = dict((str(n), plain(result["objects"][n])) for n in result["objects"])
    out.update((k, int(result[k])) for k in ("n_aligned", "n_unaligned", "n_videos_missing"))
    return out


def predicate_names(path, n_rel):
    """The predicate names of a JSON file (a list, or the reference's {name: label} of ./data/predicates.json); without a
    file the labels stand for themselves ("0", "1", ...: ground truths then carry integer labels)."""
    if not path:
        return [str(r) for r in range(n_rel)]
    import json
    with open(path) as f:
        names = json.load(f)
    if isinstance(names, dict):
        out = [None] * (max(names.values()) + 1)
        for name, label in names.items():
            out[label] = name
        return out
    return list(names)


def widths(frame_recognitions):
    """(number of classes, number of predicates) from the first frame record that has scores."""
    for frames in frame_recognitions.values():
        for rec in frames.values():
            if rec:
                return np.shape(rec["sub_scores"])[1], np.shape(rec["pre_scores"])[1]
    raise ValueError("recognition.widths: no frame has scores")
