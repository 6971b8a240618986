"""Video level of the relation test loop: per-frame triplets -> video relation instances -> VidVRD metrics.

``associate`` links the top triplets of consecutive frames into relation instances (triplet, duration, subject and object
trajectory, score) and ``evaluate`` scores them against annotated relations: detection mAP, recall@50/100 and tagging
precision@1/5/10 (lib/utils.py ``association`` / ``evaluate`` of the reference).

What runs where.  Packing the nested lists into flat arrays, the fill of empty frames, the final "at least 10 members,
best 200" selection and the gather of trajectories are host code (list logic on small data).  The frame loop of the
association and the trajectory overlaps / matching of the detection metric are HIP kernels (csrc/video.hip) when a
``device`` is given.  With ``device=None`` the same rules run as plain numpy on the host: evaluation scripts work on a
machine without a GPU, and the kernels have something to be compared with.  Both paths share the packing, the selection
and the gather, and both do their arithmetic in float64 in the same operation order, so they agree bit for bit.

``associate_tracks`` is a second association mode for boxes that carry track ids (Seq-NMS's): relations are keyed by the tracks
of their subject and object instead of by box overlap and may bridge up to ``max_gap`` frames.  Its rules are this project's
own and stand in its docstring; it has its own packer, host form, kernel and gather and shares nothing with ``associate`` but
the constants.

``suppress`` is the step between either association and the per-video cap: duplicate relations of one triplet are suppressed
greedily by the overlap of their trajectories (csrc/video_nms.hip, or the same rules in numpy).  It is off unless a caller asks
for it; its rules stand in its docstring.
"""
import numpy as np

from .packing import cat, offsets

MAX_PER_FRAME = 100          # predictions of one frame that take part
MAX_PER_VIDEO = 200          # relations kept per video
MIN_MEMBERS = 10             # a relation seen on fewer frames is dropped
FILL_WINDOW = 4              # an empty frame is filled unless every frame within this many positions is empty too
REL_COLS = 10                # ops.video_viou_match relation row


# ------------------------------------------------------------------------------------------------------------------
# host pre-pass
# ------------------------------------------------------------------------------------------------------------------
def fill_empty_frames(frames):
    """``frames``: [[frame number, predictions], ...] of one video.  Returns a new list in ascending frame number (stable)
    where an empty frame has taken the predictions of its nearest non-empty neighbour (the left one on equal distance),
    unless every frame within 4 positions of it (itself included, the window clipped to the video) is empty too."""
    frames = sorted(frames, key=lambda fr: int(fr[0]))
    n = len(frames)
    empty = [len(fr[1]) == 0 for fr in frames]
    if all(empty):
        return [[fr[0], fr[1]] for fr in frames]
    left, right = [0] * n, [0] * n                   # distance to the nearest non-empty frame on either side, 0: none
    last = -1
    for i in range(n):
        if not empty[i]:
            last = i
        elif last >= 0:
            left[i] = i - last
    last = -1
    for i in range(n - 1, -1, -1):
        if not empty[i]:
            last = i
        elif last >= 0:
            right[i] = last - i
    out = []
    for i, fr in enumerate(frames):
        preds = fr[1]
        if empty[i]:
            lo = max(0, i - FILL_WINDOW) if i >= FILL_WINDOW else 0
            hi = min(n - 1, i + FILL_WINDOW)
            if not all(empty[lo:hi + 1]):
                src = i - left[i] if right[i] == 0 or (0 < left[i] <= right[i]) else i + right[i]
                preds = frames[src][1]
        out.append([fr[0], preds])
    return out


def from_frame_results(results, frame_to_video=None, tracks=None):
    """What ``test_sgg_emb.py`` pickles -- {frame path: (rlp_labels, tuple_confs, sub_bboxes, obj_bboxes, rel_idex)}, five
    Nones for a frame without pairs -- as ``frame_relations`` {vid: [[fno, [[conf, [s, p, o], [sub_box, obj_box],
    rel_idex], ...]], ...]}.  ``frame_to_video`` maps a path to (vid, fno): a dict or a callable; None: one video "0",
    frames numbered in the order of ``results``.  ``tracks``: the per-frame box pickle the loop ran on (keyed by frame path or
    file name, ``tids`` one int per box); every prediction then gets a fifth element [sub_tid, obj_tid], and what
    ``associate_tracks`` refuses is refused here."""
    out = {}
    for k, (path, res) in enumerate(results.items()):
        if frame_to_video is None:
            vid, fno = "0", k
        elif callable(frame_to_video):
            vid, fno = frame_to_video(path)
        else:
            vid, fno = frame_to_video[path]
        labels, confs, sub, obj, idx = res
        preds = []
        if isinstance(confs, np.ndarray):
            labels, sub, obj = np.asarray(labels).tolist(), np.asarray(sub).tolist(), np.asarray(obj).tolist()
            confs, idx = confs.tolist(), np.asarray(idx).tolist()
            preds = [[confs[j], labels[j], [sub[j], obj[j]], idx[j]] for j in range(len(confs))]
        if tracks is not None:
            where = "video %r frame %d" % (vid, int(fno))
            boxes, classes, tids = _frame_tracks(_key_of(tracks, path), where)
            _, _, _, bi, bj = _resolve(preds, boxes, classes, where)
            for j, p in enumerate(preds):
                p.append([int(tids[bi[j]]), int(tids[bj[j]])])
        out.setdefault(vid, []).append([fno, preds])
    return out


# ------------------------------------------------------------------------------------------------------------------
# association
# ------------------------------------------------------------------------------------------------------------------
class Packed(object):
    """Flat arrays of a batch of videos (the layout of ``ops.video_associate``)."""

    def __init__(self, vids, frame_off, frame_no, pred_off, score, triplet, boxes, rel_idex):
        self.vids, self.frame_off, self.frame_no, self.pred_off = vids, frame_off, frame_no, pred_off
        self.score, self.triplet, self.boxes, self.rel_idex = score, triplet, boxes, rel_idex


def pack_frames(frame_relations):
    """Sort the frames, fill the empty ones, order each frame's predictions by descending score (stable) and cut them to
    the first 100.  Videos without a single prediction are left out, as the reference leaves them out of its result."""
    vids, frame_off, frame_no, counts = [], [0], [], []
    score, trip, boxes, idex = [], [], [], []
    for vid, frames in frame_relations.items():
        frames = fill_empty_frames(frames)
        if not any(len(fr[1]) for fr in frames):
            continue
        vids.append(vid)
        for fno, preds in frames:
            if len(preds) > 1:
                preds = sorted(preds, key=lambda p: p[0], reverse=True)[:MAX_PER_FRAME]
            frame_no.append(int(fno))
            counts.append(len(preds))
            for p in preds:
                score.append(p[0])
                trip.append(p[1])
                boxes.append(list(p[2][0]) + list(p[2][1]))
                idex.append(p[3])
        frame_off.append(len(frame_no))
    pred_off = offsets(counts, "video.pack_frames: more than 2^31 predictions")
    rel_idex = np.empty(len(idex), object)
    rel_idex[:] = idex
    return Packed(vids, np.asarray(frame_off, np.int32), np.asarray(frame_no, np.int32), pred_off,
                  np.asarray(score, np.float64).reshape(-1), np.asarray(trip, np.float64).astype(np.int32).reshape(-1, 3),
                  np.asarray(boxes, np.float64).reshape(-1, 8), rel_idex)


def _iou(a, b):
    """IoU of box rows in the reference's operation order: no +1, 0 for an empty or touching intersection."""
    left, right = np.maximum(a[:, 0], b[:, 0]), np.minimum(a[:, 2], b[:, 2])
    up, down = np.maximum(a[:, 1], b[:, 1]), np.minimum(a[:, 3], b[:, 3])
    s1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    s2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    sc = (down - up) * (right - left)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = sc / (s1 + s2 - sc)
    return np.where((left >= right) | (down <= up), 0.0, iou)


def _check_cap(max_per_video):
    if isinstance(max_per_video, bool) or not isinstance(max_per_video, (int, np.integer)) or max_per_video < 0:
        raise ValueError("video: max_per_video is an int >= 0 (got %r)" % (max_per_video,))
    return int(max_per_video)


def _note(stats, key, value):
    if stats is not None and value < stats.get(key, np.inf):
        stats[key] = float(value)


def _gap_margin(stats, key, values, same):
    """Smallest relative gap between neighbouring unequal values of a descending order; equal values must be true ties
    (``same(i, j)``: built from the same numbers), else the margin is 0.  ``stats["exact_sums"]``: the caller knows that
    every sum is exact (scores on a coarse binary grid), so equal values are equal in any summation order."""
    if stats is None or len(values) < 2:
        return
    order = np.argsort(-values, kind="stable")
    v = values[order]
    gap = (v[:-1] - v[1:]) / np.maximum(np.maximum(np.abs(v[:-1]), np.abs(v[1:])), 1e-300)
    for k in np.nonzero(gap == 0)[0]:
        stats["ties_" + key] = stats.get("ties_" + key, 0) + 1
        if not stats.get("exact_sums") and not same(order[k], order[k + 1]):
            _note(stats, key, 0.0)
    if (gap > 0).any():
        _note(stats, key, gap[gap > 0].min())


def associate_arrays_host(pk, stats=None):
    """The rules of ``ops.video_associate`` in numpy, on the same arrays, with the same outputs.  ``stats`` (a dict)
    collects the smallest relative margin of the decisions that rest on computed doubles: ``iou`` (an IoU against 0.5),
    ``mean`` (two unequal means of open relations of one frame)."""
    P = len(pk.score)
    rel_id = np.zeros(P, np.int32)
    rel_start, rel_len, rel_score = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.float64)
    n_rel = np.zeros(len(pk.frame_off) - 1, np.int32)
    for v in range(len(pk.frame_off) - 1):
        f0, f1 = int(pk.frame_off[v]), int(pk.frame_off[v + 1])
        base = int(pk.pred_off[f0])
        span = int(pk.pred_off[f1]) - base
        r_start, r_len, r_sum = np.zeros(span, np.int32), np.zeros(span, np.int32), np.zeros(span, np.float64)
        nxt, prev_no = 0, None
        o_id = np.zeros(0, np.int64)                 # the open relations, in the order the last frame touched them
        o_trip, o_box = np.zeros((0, 3), np.int32), np.zeros((0, 8))
        for f in range(f0, f1):
            p0, p1 = int(pk.pred_off[f]), int(pk.pred_off[f + 1])
            fno = int(pk.frame_no[f])
            if prev_no is None or fno != prev_no + 1:
                o_id = o_id[:0]
            prev_no = fno
            order = np.argsort(-pk.score[p0:p1], kind="stable")[:MAX_PER_FRAME]
            S, T, B = pk.score[p0:p1][order], pk.triplet[p0:p1][order], pk.boxes[p0:p1][order]
            n, m = len(S), len(o_id)
            assign = np.full(n, -1, np.int64)
            if n and m:
                means = r_sum[o_id] / r_len[o_id]
                _gap_margin(stats, "mean", means,
                            lambda i, j: r_sum[o_id[i]] == r_sum[o_id[j]] and r_len[o_id[i]] == r_len[o_id[j]])
                cand = np.argsort(-means, kind="stable")
                pi, ci = np.nonzero((T[:, None, :] == o_trip[cand][None, :, :]).all(-1))
                if len(pi):
                    si, oi = _iou(o_box[cand[ci], :4], B[pi, :4]), _iou(o_box[cand[ci], 4:], B[pi, 4:])
                    if stats is not None:
                        _note(stats, "iou", min(np.abs(si - 0.5).min(), np.abs(oi - 0.5).min()) / 0.5)
                    ok = (si >= 0.5) & (oi >= 0.5)
                    compat = np.zeros((n, m), bool)
                    compat[pi[ok], ci[ok]] = True
                    if stats is not None:
                        stats["contested"] = stats.get("contested", 0) + int((compat.sum(0) > 1).sum())
                        stats["multi_candidate"] = stats.get("multi_candidate", 0) + int((compat.sum(1) > 1).sum())
                    avail = np.ones(m, bool)
                    for p in np.nonzero(compat.any(1))[0]:
                        c = compat[p] & avail
                        if c.any():
                            r = int(c.argmax())
                            avail[r] = False
                            assign[p] = cand[r]
            ids = np.empty(n, np.int64)
            new = assign < 0
            ids[~new] = o_id[assign[~new]]
            ids[new] = nxt + np.arange(int(new.sum()))
            nxt += int(new.sum())
            r_start[ids[new]] = fno
            r_sum[ids] = np.where(new, S, r_sum[ids] + S)        # ids of one frame are distinct
            r_len[ids] += 1
            rel_id[p0 + order] = ids
            o_id, o_trip, o_box = ids, T, B
        n_rel[v] = nxt
        rel_start[base:base + nxt], rel_len[base:base + nxt] = r_start[:nxt], r_len[:nxt]
        rel_score[base:base + nxt] = r_sum[:nxt] / np.maximum(r_len[:nxt], 1)
        if stats is not None:
            keep = np.nonzero(r_len[:nxt] >= MIN_MEMBERS)[0]
            _gap_margin(stats, "score", rel_score[base + keep],
                        lambda i, j: r_sum[keep[i]] == r_sum[keep[j]] and r_len[keep[i]] == r_len[keep[j]])
    return rel_id, rel_start, rel_len, rel_score, n_rel


def gather_relations(pk, rel_id, rel_start, rel_len, rel_score, n_rel, names=None, max_per_video=MAX_PER_VIDEO):
    """Per video: drop relations of fewer than 10 members, order the rest by score (descending, stable in creation order),
    keep ``max_per_video`` (200), and collect each one's trajectories and ``rel_idex`` from its members."""
    out = {}
    for v, vid in enumerate(pk.vids):
        f0, f1 = int(pk.frame_off[v]), int(pk.frame_off[v + 1])
        base, end = int(pk.pred_off[f0]), int(pk.pred_off[f1])
        nr = int(n_rel[v])
        keep = np.nonzero(rel_len[base:base + nr] >= MIN_MEMBERS)[0]
        keep = keep[np.argsort(-rel_score[base + keep], kind="stable")][:_check_cap(max_per_video)]
        ids = rel_id[base:end]
        by_rel = np.argsort(ids, kind="stable")                  # members of a relation, in frame order
        first = np.searchsorted(ids[by_rel], np.arange(nr + 1))
        rels = []
        for k in keep:
            mem = base + by_rel[first[k]:first[k + 1]]
            s, p, o = (int(x) for x in pk.triplet[mem[0]])
            start = int(rel_start[base + k])
            rels.append({
                "triplet": [names[0][s], names[1][p], names[0][o]] if names is not None else [s, p, o],
                "score": float(rel_score[base + k]),
                "duration": [start, start + int(rel_len[base + k])],
                "sub_traj": pk.boxes[mem, :4].tolist(),
                "obj_traj": pk.boxes[mem, 4:].tolist(),
                "rel_idex": list(pk.rel_idex[mem]),
            })
        out[vid] = rels
    return out


def associate(frame_relations, device=None, names=None, stats=None, max_per_video=MAX_PER_VIDEO):
    """``frame_relations``: {vid: [[fno, [[conf, [s, p, o], [sub_box, obj_box], rel_idex], ...]], ...]}.  Returns {vid:
    [{triplet, score, duration, sub_traj, obj_traj, rel_idex}, ...]}, at most 200 per video in descending score; triplets
    as ids, or as names with ``names=(objects, predicates)``.  ``device``: all videos in one kernel launch on that GPU;
    None: the host implementation.  ``max_per_video``: the cap, for a caller that wants the pool ``suppress`` reads instead of
    the final 200."""
    pk = pack_frames(frame_relations)
    if device is None:
        res = associate_arrays_host(pk, stats)
    else:
        from . import ops
        res = [t.cpu().numpy() for t in ops.video_associate(pk.frame_off, pk.frame_no, pk.pred_off, pk.score, pk.triplet,
                                                            pk.boxes, device=device)]
    return gather_relations(pk, *res, names=names, max_per_video=max_per_video)


# ------------------------------------------------------------------------------------------------------------------
# association along object tracks
# ------------------------------------------------------------------------------------------------------------------
MAX_GAP = 7                  # frames a relation may stay out of its frames' lists and still go on


def _key_of(tracks, path):
    """The annotation of a frame: by the key as given, then by its file name (the pickle's own key)."""
    if path in tracks:
        return tracks[path]
    name = path.split("/")[-1] if isinstance(path, str) else path
    return tracks.get(name)


def tracks_by_frame(tracks, paths, frame_to_video=None):
    """The per-frame box pickle {frame key: annotation} as {(vid, fno): annotation} for the frames ``paths``, numbered as
    ``from_frame_results`` numbers them.  A frame without an entry is left out (the packer names it)."""
    out = {}
    for k, path in enumerate(paths):
        if frame_to_video is None:
            vid, fno = "0", k
        elif callable(frame_to_video):
            vid, fno = frame_to_video(path)
        else:
            vid, fno = frame_to_video[path]
        anno = _key_of(tracks, path)
        if anno is not None:
            out[(vid, int(fno))] = anno
    return out


def _frame_tracks(anno, where):
    """One frame of the box pickle as (boxes (n,4) float64, classes (n,) int64, tids (n,) int64), or ``ValueError``."""
    if anno is None:
        raise ValueError("video tracks: %s has no entry in the box pickle" % where)
    boxes = np.asarray(anno["boxes"], np.float64).reshape(-1, 4)
    classes = np.asarray(anno["box_classes"], np.int64).reshape(-1)
    n = len(boxes)
    tids = anno.get("tids")
    if tids is None:
        raise ValueError("video tracks: %s has no tids: the pickle is not a tracked one (seqnms.to_annotations)" % where)
    flat = list(tids)
    if len(flat) != n or len(classes) != n or not all(isinstance(t, (int, np.integer)) and not isinstance(t, bool) for t in flat):
        raise ValueError("video tracks: %s: tids holds one int per box (%d boxes); [subject_tid, object_tid] per relation is the "
                         "recognition set's layout, not this one" % (where, n))
    tids = np.asarray(flat, np.int64).reshape(-1)
    if (tids < 0).any():
        raise ValueError("video tracks: %s has a negative tid" % where)
    if len(set(zip(classes.tolist(), tids.tolist()))) != n:
        raise ValueError("video tracks: %s has two boxes with the same (class, tid)" % where)
    return boxes, classes, tids


def _resolve(preds, boxes, classes, where):
    """The subject and object box index of a frame's predictions from their ``rel_idex`` (ordered pairs, i-major over i != j),
    checked against the prediction's own boxes and classes.  -> (score (k,), triplet (k,3) int64, idex (k,), i (k,), j (k,))."""
    n, k = len(boxes), len(preds)
    score = np.asarray([p[0] for p in preds], np.float64).reshape(k)
    trip = np.asarray([p[1] for p in preds], np.float64).reshape(k, 3).astype(np.int64)
    pbox = np.asarray([list(p[2][0]) + list(p[2][1]) for p in preds], np.float64).reshape(k, 8)
    idex = np.asarray([p[3] for p in preds], np.int64).reshape(k)
    if k == 0:
        return score, trip, idex, idex, idex
    if n < 2 or (idex < 0).any() or (idex >= n * (n - 1)).any():
        raise ValueError("video tracks: %s: a rel_idex lies outside the %d ordered pairs of %d boxes" % (where, n * max(n - 1, 0), n))
    i, j = idex // (n - 1), idex % (n - 1)
    j = j + (j >= i)
    if (pbox[:, :4].view(np.int64) != boxes[i].view(np.int64)).any() or (pbox[:, 4:].view(np.int64) != boxes[j].view(np.int64)).any():
        raise ValueError("video tracks: %s: a prediction's box is not the pickle's box its rel_idex names: the wrong pickle?" % where)
    if (trip[:, 0] != classes[i]).any() or (trip[:, 2] != classes[j]).any():
        raise ValueError("video tracks: %s: a triplet's classes disagree with the pickle's box classes" % where)
    return score, trip, idex, i, j


class PackedTracks(object):
    """Flat arrays of a batch of videos (the layout of ``ops.video_associate_tracks``) and, for the gather, per video the
    objects [(class, tid), ...] by object index and per frame number (object index (n,), boxes (n,4))."""

    def __init__(self, vids, frame_off, frame_no, pred_off, score, key, since, rel_idex, objects, frames):
        self.vids, self.frame_off, self.frame_no, self.pred_off = vids, frame_off, frame_no, pred_off
        self.score, self.key, self.since, self.rel_idex, self.objects, self.frames = score, key, since, rel_idex, objects, frames


def _check_gap(max_gap):
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError("video tracks: max_gap is an int in [0, %d] (got %r)" % (MAX_GAP, max_gap))
    return int(max_gap)


def pack_track_frames(frame_relations, tracks, frame_to_video=None):
    """The tables of the track mode (``associate_tracks`` states the rules).  ``tracks``: {(vid, fno): annotation}; with
    ``frame_to_video`` (a dict path -> (vid, fno)) the box pickle as it is, keyed by frame path or file name.  Every video of
    ``frame_relations`` takes part, in its order, also one without frames or predictions."""
    if frame_to_video is not None:
        tracks = tracks_by_frame(tracks, list(frame_to_video), frame_to_video)
    vids, frame_off, frame_no, counts = [], [0], [], []
    score, key, since, idex, objects, tables = [], [], [], [], [], []
    for vid, frames in frame_relations.items():
        frames = sorted(frames, key=lambda fr: int(fr[0]))
        vids.append(vid)
        index, run, objs, table = {}, {}, [], {}         # (class, tid) -> object index; object index -> [last frame, run start]
        for fno, preds in frames:
            fno = int(fno)
            where = "video %r frame %d" % (vid, fno)
            if fno in table:
                raise ValueError("video tracks: %s appears twice" % where)
            boxes, classes, tids = _frame_tracks(tracks.get((vid, fno)), where)
            oid = np.empty(len(boxes), np.int64)
            start = np.empty(len(boxes), np.int64)
            for b, ct in enumerate(zip(classes.tolist(), tids.tolist())):
                o = index.setdefault(ct, len(objs))
                if o == len(objs):
                    objs.append(ct)
                r = run.get(o)
                run[o] = r = [fno, r[1] if r is not None and r[0] == fno - 1 else fno]
                oid[b], start[b] = o, r[1]
            table[fno] = (oid, boxes)
            s, trip, ix, i, j = _resolve(preds, boxes, classes, where)
            for p, pred in enumerate(preds):
                if len(pred) > 4 and [int(x) for x in pred[4]] != [int(tids[i[p]]), int(tids[j[p]])]:
                    raise ValueError("video tracks: %s: a prediction's tids are not those of the boxes its rel_idex names" % where)
            order = np.argsort(-s, kind="stable")[:MAX_PER_FRAME]
            frame_no.append(fno)
            counts.append(len(order))
            if len(order):
                score.append(s[order])
                key.append(np.stack([oid[i[order]], trip[order, 1], oid[j[order]]], 1))
                since.append(np.maximum(start[i[order]], start[j[order]]))
                idex.append(ix[order])
        frame_off.append(len(frame_no))
        objects.append(objs)
        tables.append(table)
    pred_off = offsets(counts, "video.pack_track_frames: more than 2^31 predictions")
    return PackedTracks(vids, np.asarray(frame_off, np.int32), np.asarray(frame_no, np.int32), pred_off, cat(score, (), np.float64),
                        cat(key, (3,), np.int64).astype(np.int32), cat(since, (), np.int64).astype(np.int32),
                        cat(idex, (), np.int64), objects, tables)


def associate_tracks_arrays_host(pk, max_gap=0):
    """The rules of ``ops.video_associate_tracks`` in numpy, on the same arrays, with the same outputs (rel_id, rel_start,
    rel_end, rel_len, rel_score, n_rel); one pass of array operations per frame.  A table the kernel would report (a frame of
    more than 100 predictions, a frame number that does not ascend, a repeated key) raises ``ValueError``."""
    G = _check_gap(max_gap)
    P, V = len(pk.score), len(pk.frame_off) - 1
    rel_id = np.zeros(P, np.int32)
    rel_start, rel_end, rel_len = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    rel_score, n_rel = np.zeros(P, np.float64), np.zeros(V, np.int32)
    key = np.asarray(pk.key, np.int64).reshape(-1, 3)
    for v in range(V):
        f0, f1 = int(pk.frame_off[v]), int(pk.frame_off[v + 1])
        if f1 == f0:
            continue
        base, end = int(pk.pred_off[f0]), int(pk.pred_off[f1])
        _, kid = np.unique(key[base:end], axis=0, return_inverse=True)       # the video's keys, densely numbered
        kid = kid.reshape(-1)
        n_keys = int(kid.max()) + 1 if len(kid) else 0
        o_id, o_last = np.full(n_keys, -1, np.int64), np.zeros(n_keys, np.int64)   # the open relation of every key
        r_start, r_end, r_len = np.zeros(end - base, np.int32), np.zeros(end - base, np.int32), np.zeros(end - base, np.int32)
        r_sum = np.zeros(end - base, np.float64)
        nxt, prev_no = 0, None
        for f in range(f0, f1):
            p0, p1 = int(pk.pred_off[f]), int(pk.pred_off[f + 1])
            fno = int(pk.frame_no[f])
            if p1 - p0 > MAX_PER_FRAME or (prev_no is not None and fno <= prev_no):
                raise ValueError("video tracks: frame %d of the table holds more than %d predictions or a frame number that "
                                 "does not ascend" % (f, MAX_PER_FRAME))
            prev_no = fno
            if p1 == p0:
                continue
            order = np.argsort(-pk.score[p0:p1], kind="stable")
            S, K, since = pk.score[p0:p1][order], kid[p0 - base:p1 - base][order], pk.since[p0:p1][order].astype(np.int64)
            if len(np.unique(K)) != len(K):
                raise ValueError("video tracks: frame %d of the table repeats a key" % f)
            L = o_last[K]
            ext = (o_id[K] >= 0) & (fno - L >= 1) & (fno - L <= G + 1) & (since <= L)
            new = ~ext
            ids = np.where(ext, o_id[K], nxt + np.cumsum(new) - 1)
            nxt += int(new.sum())
            r_start[ids[new]] = fno
            r_end[ids] = fno + 1
            r_sum[ids] = np.where(new, S, r_sum[ids] + S)        # ids of one frame are distinct
            r_len[ids] = np.where(new, 1, r_len[ids] + 1)
            o_id[K], o_last[K] = ids, fno
            rel_id[p0 + order] = ids
        n_rel[v] = nxt
        rel_start[base:base + nxt], rel_end[base:base + nxt], rel_len[base:base + nxt] = r_start[:nxt], r_end[:nxt], r_len[:nxt]
        rel_score[base:base + nxt] = r_sum[:nxt] / np.maximum(r_len[:nxt], 1)
    return rel_id, rel_start, rel_end, rel_len, rel_score, n_rel


def gather_track_relations(pk, rel_id, rel_start, rel_end, rel_len, rel_score, n_rel, names=None, max_per_video=MAX_PER_VIDEO):
    """Per video: drop relations of fewer than 10 members, order the rest by score (descending, stable in creation order),
    keep ``max_per_video`` (200), and read each one's trajectories and pair indices from its two tracks' boxes, for every frame
    of the duration."""
    out = {}
    for v, vid in enumerate(pk.vids):
        f0, f1 = int(pk.frame_off[v]), int(pk.frame_off[v + 1])
        base, end = int(pk.pred_off[f0]), int(pk.pred_off[f1])
        nr = int(n_rel[v])
        keep = np.nonzero(rel_len[base:base + nr] >= MIN_MEMBERS)[0]
        keep = keep[np.argsort(-rel_score[base + keep], kind="stable")][:_check_cap(max_per_video)]
        ids = rel_id[base:end]
        by_rel = np.argsort(ids, kind="stable")                  # members of a relation, in frame order
        first = np.searchsorted(ids[by_rel], np.arange(nr + 1))
        member_frame = np.repeat(pk.frame_no[f0:f1], np.diff(pk.pred_off[f0:f1 + 1]))
        objs, table = pk.objects[v], pk.frames[v]
        rels = []
        for k in keep:
            mem = by_rel[first[k]:first[k + 1]]
            so, p, oo = (int(x) for x in pk.key[base + mem[0]])
            start, stop = int(rel_start[base + k]), int(rel_end[base + k])
            own = dict(zip(member_frame[mem].tolist(), pk.rel_idex[base + mem].tolist()))
            sub, obj, idex = [], [], []
            for fno in range(start, stop):
                oid, boxes = table[fno]                          # ``since``: both tracks have a box in every frame of the duration
                i, j = int(np.nonzero(oid == so)[0][0]), int(np.nonzero(oid == oo)[0][0])
                pair = i * (len(oid) - 1) + j - (j > i)
                assert own.get(fno, pair) == pair, (vid, fno, own[fno], pair)
                sub.append(boxes[i].tolist())
                obj.append(boxes[j].tolist())
                idex.append(pair)
            s, o = objs[so][0], objs[oo][0]
            rels.append({
                "triplet": [names[0][s], names[1][p], names[0][o]] if names is not None else [s, p, o],
                "score": float(rel_score[base + k]),
                "duration": [start, stop],
                "sub_traj": sub,
                "obj_traj": obj,
                "rel_idex": idex,
                "sub_tid": int(objs[so][1]),
                "obj_tid": int(objs[oo][1]),
                "members": int(rel_len[base + k]),
            })
        out[vid] = rels
    return out


def gap_frames(relations):
    """Frames of the relations' durations that are not members: what ``max_gap`` bridged."""
    return sum(r["duration"][1] - r["duration"][0] - r["members"] for rels in relations.values() for r in rels)


def associate_tracks(frame_relations, tracks, max_gap=0, device=None, names=None, frame_to_video=None, max_per_video=MAX_PER_VIDEO):
    """Association along the object tracks that Seq-NMS computed: a second mode beside ``associate`` for boxes that carry a
    track id.  ``associate`` rediscovers identity frame by frame from box overlaps; here identity is given, so two objects of
    one class that pass each other keep their relations, and a relation that leaves its frames' top 100 for a few frames
    goes on.  The rules are this project's own (the reference has no tracks); both forms follow them.

    Inputs.  ``frame_relations`` as ``from_frame_results`` returns it, and ``tracks``, the per-frame box pickle the frame loop
    ran on, in the layout of ``seqnms.to_annotations``: per frame ``boxes``, ``box_classes`` and ``tids`` with one int per box,
    track ids per (video, class).  ``tracks`` is keyed by (vid, fno); with ``frame_to_video`` (a dict path -> (vid, fno)) it is
    the pickle as it is.

    Identity.  A track is (video, class, tid).  Per video, tracks get a dense object index in order of first appearance
    (frames ascending, box order within a frame).  A prediction's ``rel_idex`` is its ordered-pair index (i-major over i != j):
    for n boxes i = p // (n-1), j' = p % (n-1), j = j' + (j' >= i) are its subject and object box, and so its two tracks.

    Refused (``ValueError`` naming the frame): a result frame missing from the pickle; no ``tids``, or ``tids`` not of one int
    per box (``synthetic.recognition_set`` uses the key for [subject_tid, object_tid] per relation); a negative tid; two
    boxes of one frame with the same (class, tid); a prediction whose subject or object box is not bit-equal to the pickle's
    box it resolves to (the wrong pickle); classes that disagree with the triplet; a frame number twice in a video.

    Per frame the predictions are ordered by descending score, stable, and cut to 100.  ``fill_empty_frames`` is not applied:
    the gap rule serves an empty frame.

    Key: (subject object index, predicate, object object index); distinct within a frame by what is refused.

    Presence.  Every prediction has ``since``, the larger of its two tracks' run starts: the first frame number of the maximal
    run of consecutive frame numbers of the video, ending at this frame, in which the track has a box in the pickle.  Top-100
    membership plays no part in it.

    Extension.  A video has at most one open relation per key.  The prediction at frame number f extends the open relation of
    its key, whose last member is at frame number L, iff 1 <= f - L <= max_gap + 1 and since <= L; otherwise it opens a
    relation, which takes the place of the open one of its key (that one can never be extended again: a later ``since`` is no
    smaller).  ``max_gap`` is an int in [0, 7]; with 0 a relation must appear in consecutive frames, as in the box mode, and the
    ``since`` condition cannot fail.  A missing frame number, or a frame where either track has no box, ends the relation
    whatever ``max_gap`` is: ``since`` then lies past L.

    Numbering: new relations get ids 0, 1, 2, ... per video, frames ascending, within a frame in ranked order.

    Score: the float64 sum of the members' scores in member order, from the first member's score, divided by the number of
    members.  Gap frames are not members: they enter neither the mean nor the 10-member rule.

    Selection as in ``gather_relations``: at least 10 members, descending score stable in creation order, the first 200
    (``max_per_video``).

    Output per relation: ``triplet``, ``score``, ``duration`` = [first member's frame, last member's frame + 1), ``sub_traj`` /
    ``obj_traj`` (the tracks' boxes from the pickle for EVERY frame of the duration), ``rel_idex`` (per frame of the duration the
    pair index of (subject box, object box) in that frame; on member frames it equals the prediction's own, which is
    asserted), ``sub_tid``, ``obj_tid`` and ``members``.  ``relation_features.pack`` / ``pool`` and ``pack_eval`` / ``evaluate``
    read it unchanged.

    ``device``: all videos in one kernel launch on that GPU (``ops.video_associate_tracks``); None: the host form."""
    max_gap = _check_gap(max_gap)
    pk = pack_track_frames(frame_relations, tracks, frame_to_video)
    if device is None:
        res = associate_tracks_arrays_host(pk, max_gap)
    else:
        from . import ops
        res = [t.cpu().numpy() for t in ops.video_associate_tracks(pk.frame_off, pk.frame_no, pk.pred_off, pk.score, pk.key, pk.since,
                                                                   max_gap, device=device)]
    return gather_track_relations(pk, *res, names=names, max_per_video=max_per_video)


# ------------------------------------------------------------------------------------------------------------------
# evaluation
# ------------------------------------------------------------------------------------------------------------------
class PackedEval(object):
    """Flat arrays of predictions and ground truths of the videos that have ground truth (``ops.video_viou_match``)."""

    def __init__(self, vids, pred_off, pred_rel, pred_score, gt_off, gt_rel, boxes):
        self.vids, self.pred_off, self.pred_rel, self.pred_score = vids, pred_off, pred_rel, pred_score
        self.gt_off, self.gt_rel, self.boxes = gt_off, gt_rel, boxes


def _rel_rows(v, rels, vocab, boxes, n_box):
    """The relation rows (REL_COLS int32 each) of the relations ``rels`` of video index ``v``; their trajectories are appended
    to the list ``boxes`` (``n_box[0]`` counts its rows) and the triplets' elements numbered through ``vocab``."""
    out = np.zeros((len(rels), REL_COLS), np.int32)
    for k, r in enumerate(rels):
        out[k, 0] = v
        out[k, 1:4] = [vocab.setdefault(x, len(vocab)) for x in r["triplet"]]
        out[k, 4:6] = r["duration"]
        for c, key in ((6, "sub_traj"), (8, "obj_traj")):
            out[k, c], out[k, c + 1] = n_box[0], len(r[key])
            if len(r[key]):
                boxes.append(np.asarray(r[key], np.float64).reshape(-1, 4))
                n_box[0] += len(r[key])
    return out


def pack_eval(prediction, groundtruth):
    vocab = {}
    boxes, n_box = [], [0]
    rows = lambda v, rels: _rel_rows(v, rels, vocab, boxes, n_box)
    vids, pred_off, gt_off, pred_rel, gt_rel, score = [], [0], [0], [], [], []
    for vid, gts in groundtruth.items():
        if len(gts) == 0:                                # the reference skips a video without ground truth
            continue
        preds = prediction.get(vid, [])
        v = len(vids)
        vids.append(vid)
        pred_rel.append(rows(v, preds))
        gt_rel.append(rows(v, gts))
        score.extend(float(r["score"]) for r in preds)
        pred_off.append(pred_off[-1] + len(preds))
        gt_off.append(gt_off[-1] + len(gts))
    return PackedEval(vids, np.asarray(pred_off, np.int32), cat(pred_rel, (REL_COLS,), np.int32), np.asarray(score, np.float64),
                      np.asarray(gt_off, np.int32), cat(gt_rel, (REL_COLS,), np.int32), cat(boxes, (4,), np.float64))


def _viou(pr, gr, c, boxes, vol_p, vol_g):
    """Voluminal IoU of one trajectory pair (+1 pixel convention): intersection over the common frames, volumes over the
    whole trajectories."""
    lo, hi = max(pr[4], gr[4]), min(pr[5], gr[5])
    if hi <= lo:
        return 0.0
    n = max(0, min(hi - lo, pr[c + 1] - (lo - pr[4]), gr[c + 1] - (lo - gr[4])))     # never past the end of a trajectory
    a = boxes[pr[c] + lo - pr[4]:pr[c] + lo - pr[4] + n]
    b = boxes[gr[c] + lo - gr[4]:gr[c] + lo - gr[4] + n]
    w = np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]) + 1.0
    h = np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]) + 1.0
    inter = float(np.sum(np.maximum(w, 0.0) * np.maximum(h, 0.0)))
    return inter / (vol_p + vol_g - inter)


def match_arrays_host(pe, viou_threshold=0.5, stats=None):
    """The rules of ``ops.video_viou_match`` in numpy.  Returns (ov (n_pred, max_gt), hit (n_pred), hit_ov (n_pred)).
    ``stats``: smallest relative margin of an ov against the threshold (``ov``) and between two unequal ov that one
    prediction chooses from (``ov_gap``)."""
    counts = np.diff(pe.gt_off)
    max_gt = int(counts.max()) if len(counts) else 0
    n_pred = len(pe.pred_rel)
    ov = np.full((n_pred, max_gt), -1.0)
    hit, hit_ov = np.full(n_pred, -1, np.int32), np.full(n_pred, -1.0)

    def volumes(rel):
        b = pe.boxes
        area = (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)
        return np.array([[area[r[c]:r[c] + r[c + 1]].sum() for c in (6, 8)] for r in rel]).reshape(-1, 2)

    vp, vg = volumes(pe.pred_rel), volumes(pe.gt_rel)
    for v in range(len(pe.vids)):
        p0, p1, g0, g1 = int(pe.pred_off[v]), int(pe.pred_off[v + 1]), int(pe.gt_off[v]), int(pe.gt_off[v + 1])
        for p in range(p0, p1):
            pr = pe.pred_rel[p]
            for g in np.nonzero((pe.gt_rel[g0:g1, 1:4] == pr[1:4]).all(1))[0]:
                gr = pe.gt_rel[g0 + g]
                s = _viou(pr, gr, 6, pe.boxes, vp[p, 0], vg[g0 + g, 0])
                o = _viou(pr, gr, 8, pe.boxes, vp[p, 1], vg[g0 + g, 1])
                ov[p, g] = min(s, o)
        taken = np.zeros(g1 - g0, bool)
        for p in p0 + np.argsort(-pe.pred_score[p0:p1], kind="stable"):
            row = ov[p, :g1 - g0]
            if stats is not None and (row >= 0).any():
                x = row[row >= 0]
                _note(stats, "ov", np.abs(x - viou_threshold).min() / max(viou_threshold, 1e-300))
                u = np.unique(x[x >= viou_threshold])
                if len(u) > 1:
                    _note(stats, "ov_gap", (np.diff(u) / u[1:]).min())
            cand = (row >= 0) & (row >= viou_threshold) & ~taken
            if cand.any():
                g = int(np.where(cand, row, -1.0).argmax())
                taken[g] = True
                hit[p], hit_ov[p] = g, row[g]
    return ov, hit, hit_ov


def match(prediction, groundtruth, viou_threshold=0.5, device=None, stats=None):
    """Detection matching of every video that has ground truth: (PackedEval, ov, hit, hit_ov) with ``hit[p]`` the index of
    the ground truth (within its video) that prediction p detects, or -1."""
    pe = pack_eval(prediction, groundtruth)
    if device is None:
        return (pe,) + match_arrays_host(pe, viou_threshold, stats)
    from . import ops
    ov, hit, hit_ov = ops.video_viou_match(pe.pred_off, pe.pred_rel, pe.pred_score, pe.gt_off, pe.gt_rel, pe.boxes,
                                           viou_threshold, device=device)
    return pe, ov.cpu().numpy(), hit.cpu().numpy(), hit_ov.cpu().numpy()


def voc_ap(rec, prec, use_07_metric=False):
    """VOC average precision: the area under the precision envelope, or the 11-point mean of the 2007 devkit."""
    rec, prec = np.asarray(rec), np.asarray(prec)
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            above = rec >= t
            ap = ap + (np.max(prec[above]) if above.any() else 0) / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def _prec_rec(tp, n_gt):
    eps = np.finfo(np.float32).eps
    cum_tp = np.cumsum(tp).astype(np.float32)
    cum_fp = np.cumsum(~tp).astype(np.float32)
    return cum_tp / np.maximum(cum_tp + cum_fp, eps), cum_tp / np.maximum(n_gt, eps)


def _tagging_precision(gts, preds):
    """Precision over the distinct predicted triplets in descending score; trajectories play no part."""
    want = set(tuple(r["triplet"]) for r in gts)
    seen, tp = set(), []
    for r in sorted(preds, key=lambda r: r["score"], reverse=True):
        t = tuple(r["triplet"])
        if t not in seen:
            seen.add(t)
            tp.append(t in want)
    return _prec_rec(np.asarray(tp, bool), len(want))[0]


def evaluate(prediction, groundtruth, viou_threshold=0.5, det_nreturns=(50, 100), tag_nreturns=(1, 5, 10), device=None):
    """(mean_ap, {n: detection recall@n}, {n: tagging precision@n}) over the videos of ``groundtruth`` that have relations."""
    pe, _, hit, _ = match(prediction, groundtruth, viou_threshold, device)
    video_ap, n_gt_total = [], 0
    tp_at = dict((n, 0) for n in det_nreturns)
    prec_at = dict((n, []) for n in tag_nreturns)
    for v, vid in enumerate(pe.vids):
        gts, preds = groundtruth[vid], prediction.get(vid, [])
        p0, p1 = int(pe.pred_off[v]), int(pe.pred_off[v + 1])
        n_gt_total += len(gts)
        tp = (hit[p0:p1] >= 0)[np.argsort(-pe.pred_score[p0:p1], kind="stable")]
        prec, rec = _prec_rec(tp, len(gts))
        video_ap.append(voc_ap(rec, prec))
        for n in det_nreturns:
            tp_at[n] += int(tp[:n].sum())
        tag = _tagging_precision(gts, preds)
        for n in tag_nreturns:
            cut = min(n, tag.size)
            prec_at[n].append(tag[cut - 1] if cut > 0 else 0.)
    mean_ap = np.mean(video_ap)
    # recall@n is the last element of a cumulative sum over all videos' first n predictions: their order plays no part
    rec_at_n = dict((n, np.float32(tp_at[n]) / np.maximum(n_gt_total, np.finfo(np.float32).eps)) for n in det_nreturns)
    mprec_at_n = dict((n, np.mean(prec_at[n])) for n in tag_nreturns)
    return mean_ap, rec_at_n, mprec_at_n


# ------------------------------------------------------------------------------------------------------------------
# relation NMS: duplicate relations suppressed by trajectory overlap, between the association and the per-video cap
# ------------------------------------------------------------------------------------------------------------------
NMS_POOL = 2048              # candidates of one video that take part by default
NMS_MAX_POOL = 4096          # the most they can be (csrc/video_nms.hip RN_MAXCELL: a cell is at most a video's candidates)
NMS_MAX_FRAMES = 1 << 20     # frames of one trajectory (RN_MAXLEN)


class PackedNMS(object):
    """Flat arrays of the candidates of a batch of videos (the layout of ``ops.video_relation_nms``): ``rel`` (R, 10) the
    matcher's relation row, ``boxes`` (n_boxes, 4) float64, ``cell_off`` (C+1) the cells' rows, ``score`` (R).  For the way
    back: ``video_off`` (V+1; a video's candidates are contiguous), ``src`` (R; the relation's index in its video's input
    list), ``rank`` (R; its rank among its video's candidates) and ``n_input`` (V; relations the video came with)."""

    def __init__(self, vids, video_off, cell_off, rel, score, boxes, src, rank, n_input):
        self.vids, self.video_off, self.cell_off, self.rel, self.score, self.boxes = vids, video_off, cell_off, rel, score, boxes
        self.src, self.rank, self.n_input = src, rank, n_input


def _check_threshold(viou_threshold):
    t = float(viou_threshold)
    if not 0.0 <= t <= 1.0:
        raise ValueError("video.suppress: the vIoU threshold lies in [0, 1] (got %r)" % (viou_threshold,))
    return t


def _check_relation(vid, k, r):
    """What ``suppress`` states about one relation, or ``ValueError`` naming the video and the relation's index."""
    def refuse(why):
        raise ValueError("video.pack_nms: video %r relation %d: %s" % (vid, k, why))
    try:
        fstart, fend = (int(x) for x in r["duration"])
        score = float(r["score"])
        trajs = [np.asarray(r[key], np.float64) for key in ("sub_traj", "obj_traj")]
    except (TypeError, ValueError, KeyError) as e:
        refuse("not a relation (%s)" % (e,))
    if not np.isfinite(score):
        refuse("its score is not finite")
    for name, b in zip(("sub_traj", "obj_traj"), trajs):
        if b.size % 4 or (b.ndim != 2 and b.size):
            refuse("%s is not a list of boxes [x1, y1, x2, y2]" % name)
        b = b.reshape(-1, 4)
        if len(b) != fend - fstart:
            refuse("%s holds %d boxes for the duration [%d, %d)" % (name, len(b), fstart, fend))
        if len(b) > NMS_MAX_FRAMES:
            refuse("%s holds more than 2^20 frames" % name)
        if not np.isfinite(b).all():
            refuse("%s holds a box that is not finite" % name)
        if (b[:, 2] < b[:, 0]).any() or (b[:, 3] < b[:, 1]).any():
            refuse("%s holds a box with x2 < x1 or y2 < y1" % name)


def pack_nms(prediction, pool=NMS_POOL):
    """The tables of ``suppress`` (which states the rules) for {vid: [relation, ...]}: every video of ``prediction`` takes part,
    in its order, also one without relations.  Every relation is checked, also one the pool drops."""
    if isinstance(pool, bool) or not isinstance(pool, (int, np.integer)) or not 1 <= pool <= NMS_MAX_POOL:
        raise ValueError("video.pack_nms: pool is an int in [1, %d] (got %r)" % (NMS_MAX_POOL, pool))
    vocab, boxes, n_box = {}, [], [0]
    vids, video_off, cells, rows, score, src, rank, n_input = [], [0], [], [], [], [], [], []
    for v, (vid, rels) in enumerate(prediction.items()):
        for k, r in enumerate(rels):
            _check_relation(vid, k, r)
        s = np.asarray([float(r["score"]) for r in rels], np.float64).reshape(-1)
        order = np.argsort(-s, kind="stable")[:int(pool)]          # (score descending, input index ascending)
        by_cell = {}                                             # insertion order: the rank of a cell's first member
        for q, k in enumerate(order.tolist()):
            by_cell.setdefault(tuple(rels[k]["triplet"]), []).append(q)
        packed = [q for members in by_cell.values() for q in members]
        vids.append(vid)
        n_input.append(len(rels))
        cells.extend(len(members) for members in by_cell.values())
        rows.append(_rel_rows(v, [rels[order[q]] for q in packed], vocab, boxes, n_box))
        score.append(s[order[packed]])
        src.append(order[packed])
        rank.append(np.asarray(packed, np.int64))
        video_off.append(video_off[-1] + len(packed))
    return PackedNMS(vids, np.asarray(video_off, np.int32), offsets(cells, "video.pack_nms: more than 2^31 relations"),
                     cat(rows, (REL_COLS,), np.int32), cat(score, (), np.float64), cat(boxes, (4,), np.float64),
                     cat(src, (), np.int64), cat(rank, (), np.int64), np.asarray(n_input, np.int64))


def _check_nms_cell(pk, c):
    """What the kernel reports through its status word raises here, naming the cell."""
    rel, R, NB = pk.rel, len(pk.rel), len(pk.boxes)
    r0, r1 = int(pk.cell_off[c]), int(pk.cell_off[c + 1])
    bad = r0 < 0 or r1 < r0 or r1 > R or r1 - r0 > NMS_MAX_POOL
    if not bad:
        m = rel[r0:r1].astype(np.int64)
        for c0 in (6, 8):
            off, ln = m[:, c0], m[:, c0 + 1]
            bad = bad or bool(((off < 0) | (ln < 0) | (off + ln > NB) | (ln != m[:, 5] - m[:, 4]) | (ln > NMS_MAX_FRAMES)).any())
    if bad:
        raise ValueError("video.suppress: cell %d is malformed: its offsets are out of range, it holds more than %d relations or a "
                         "trajectory disagrees with its duration" % (c, NMS_MAX_POOL))
    return r0, r1


def _volumes(rel, boxes):
    """vol (R, 2): per trajectory the sum of its boxes' +1 areas, the frames in order from 0.0, one accumulator each (a loop
    over frames, vectorised over trajectories)."""
    vol = np.zeros((len(rel), 2))
    for which in (0, 1):
        off, ln = rel[:, 6 + 2 * which].astype(np.int64), rel[:, 7 + 2 * which].astype(np.int64)
        acc = np.zeros(len(rel))
        for f in range(int(ln.max()) if len(ln) else 0):
            m = np.nonzero(ln > f)[0]
            b = boxes[off[m] + f]
            acc[m] = acc[m] + ((b[:, 2] - b[:, 0]) + 1.0) * ((b[:, 3] - b[:, 1]) + 1.0)
        vol[:, which] = acc
    return vol


def _viou_row(rel, boxes, vol, i, js, which):
    """vIoU of trajectory ``which`` of row i with each of the rows js: the intersection over the common frames, ascending from
    0.0, one accumulator per pair (a loop over frames, vectorised over pairs); 0 where the durations share no frame."""
    m = rel[js].astype(np.int64)
    a0, a1 = int(rel[i, 4]), int(rel[i, 5])
    lo, hi = np.maximum(a0, m[:, 4]), np.minimum(a1, m[:, 5])
    cnt = np.maximum(hi - lo, 0)
    xi, yj = int(rel[i, 6 + 2 * which]) + (lo - a0), m[:, 6 + 2 * which] + (lo - m[:, 4])
    acc = np.zeros(len(js))
    for f in range(int(cnt.max()) if len(cnt) else 0):
        k = np.nonzero(cnt > f)[0]
        x, y = boxes[xi[k] + f], boxes[yj[k] + f]
        w = (np.minimum(x[:, 2], y[:, 2]) - np.maximum(x[:, 0], y[:, 0])) + 1.0
        h = (np.minimum(x[:, 3], y[:, 3]) - np.maximum(x[:, 1], y[:, 1])) + 1.0
        acc[k] = acc[k] + np.maximum(w, 0.0) * np.maximum(h, 0.0)
    out = np.zeros(len(js))
    k = cnt > 0
    out[k] = acc[k] / ((vol[i, which] + vol[js[k], which]) - acc[k])
    return out


def suppress_arrays_host(pk, viou_threshold, stats=None):
    """The rules of ``ops.video_relation_nms`` in numpy, on the same arrays, with the same outputs: (keep (R) int32, by (R)
    int32, by_ov (R) float64, vol (R, 2) float64).  Like the kernel it compares only kept rows with the later rows that are
    still alive.  ``stats``: the smallest relative margin of an ov it evaluated against the threshold (``ov``)."""
    T = _check_threshold(viou_threshold)
    R = len(pk.rel)
    cells = [_check_nms_cell(pk, c) for c in range(len(pk.cell_off) - 1)]
    keep, by, by_ov = np.zeros(R, np.int32), np.full(R, -1, np.int32), np.full(R, -1.0)
    vol = np.zeros((R, 2))
    for r0, r1 in cells:
        vol[r0:r1] = _volumes(pk.rel[r0:r1], pk.boxes)
    for r0, r1 in cells:
        alive = np.ones(r1 - r0, bool)
        for i in range(r1 - r0):
            if not alive[i]:
                continue
            keep[r0 + i] = 1
            js = r0 + i + 1 + np.nonzero(alive[i + 1:])[0]
            if not len(js):
                continue
            ov = np.minimum(_viou_row(pk.rel, pk.boxes, vol, r0 + i, js, 0), _viou_row(pk.rel, pk.boxes, vol, r0 + i, js, 1))
            _note(stats, "ov", np.abs(ov - T).min() / max(T, 1e-300))
            hit = js[ov > T]                                     # strict: ov == T stays
            alive[hit - r0] = False
            by[hit], by_ov[hit] = r0 + i, ov[ov > T]
    return keep, by, by_ov, vol


def suppress(prediction, viou_threshold, max_per_video=MAX_PER_VIDEO, pool=NMS_POOL, device=None, stats=None):
    """Suppress duplicate video relations by trajectory overlap: the step of a VidVRD-style pipeline between the association
    and the per-video cap.  The association emits the same relation many times (every near-identical candidate of the
    per-frame top 100 grows a chain of its own); the matcher lets each ground truth be detected once, so the duplicates fill
    the cap and count as false positives.  ``prediction`` is {vid: [relation, ...]} as ``gather_relations`` /
    ``gather_track_relations`` write it -- with ``max_per_video=pool`` there, so that this step sees the candidates before the
    cap.  Returns (prediction', info): per video the SAME dict objects, filtered and ordered, and info[vid] = {"candidates",
    "suppressed", "kept"} (kept: what is returned, after the cap).  The host form is the specification; the kernel
    (csrc/video_nms.hip) follows it bit for bit.

    Relation.  A dict with ``triplet``, ``score``, ``duration`` = [fstart, fend), ``sub_traj``, ``obj_traj``; any further key
    (``rel_idex``, track ids, ...) passes through untouched.  ``len(sub_traj) == len(obj_traj) == fend - fstart``; boxes are
    finite with x2 >= x1 and y2 >= y1; scores are finite; a trajectory holds at most 2^20 frames.  ``pack_nms`` raises
    ``ValueError`` naming the video and the relation's index otherwise (the matcher clamps such rows; this op refuses them).
    Boxes widen to float64 exactly, and every decision is float64.

    Candidates.  Per video the ``pool`` best by (score descending, input index ascending); the rest are dropped.  ``pool``
    defaults to 2048 and is at most 4096.  A cell is one (video, triplet).  Cells are ordered by the rank of their first member
    and within a cell the packed order is the rank order: the kernel sorts nothing.

    Overlap.  vol(t) is the sum over the trajectory's frames, in frame order from 0.0 with one accumulator, of ((x2 - x1) + 1) *
    ((y2 - y1) + 1).  inter(a, b) is the sum over the common frames max(fstart) .. min(fend) - 1, ascending, from 0.0 with one
    accumulator, of max(0, (min(x2) - max(x1)) + 1) * max(0, (min(y2) - max(y1)) + 1).  viou = inter / ((vol_a + vol_b) - inter);
    ov = min(viou_subject, viou_object), and 0 where the durations share no frame.  This is the reference's ``viou``
    (lib/utils.py:221-262).  The sums are sequential on purpose: one lane owns one pair and needs no reduction.

    Suppression, greedy as in nms_cpu.py and Seq-NMS.  A cell is gone through in rank order; a relation that no kept relation
    suppresses is kept; a kept relation i suppresses every later j of its cell with ov(i, j) > T.  The comparison is strict:
    ov == T stays.  T lies in [0, 1].  Per relation the outputs are ``keep`` (0 / 1), ``by`` (the packed index of the first
    kept relation, in rank order, that suppresses it, or -1), ``by_ov`` (its ov with that relation, or -1.0) and ``vol`` (2
    per relation).

    Cap.  After suppression each video keeps its kept relations in descending score (stable) and takes the first
    ``max_per_video`` (200).

    ``device``: every cell of every video in one kernel launch on that GPU (``ops.video_relation_nms``); None: the host form
    (``suppress_arrays_host``, which also fills ``stats``)."""
    T = _check_threshold(viou_threshold)
    cap = _check_cap(max_per_video)
    pk = pack_nms(prediction, pool)
    if device is None:
        keep = suppress_arrays_host(pk, T, stats)[0]
    else:
        from . import ops
        keep = ops.video_relation_nms(pk.cell_off, pk.rel, pk.boxes, T, device=device)[0].cpu().numpy()
    out, info = {}, {}
    for v, vid in enumerate(pk.vids):
        p0, p1 = int(pk.video_off[v]), int(pk.video_off[v + 1])
        kept = p0 + np.nonzero(keep[p0:p1])[0]
        kept = kept[np.argsort(pk.rank[kept], kind="stable")]    # rank order: descending score, stable in input order
        rels = prediction[vid]
        out[vid] = [rels[int(pk.src[p])] for p in kept[:cap]]
        info[vid] = {"candidates": p1 - p0, "suppressed": p1 - p0 - len(kept), "kept": len(out[vid])}
    return out, info


def nms_totals(info):
    """The sums of ``suppress``'s info over the videos, as one line."""
    tot = dict((key, sum(i[key] for i in info.values())) for key in ("candidates", "suppressed", "kept"))
    return "relation NMS: %d videos, %d candidates, %d suppressed, %d kept" % (len(info), tot["candidates"], tot["suppressed"], tot["kept"])
