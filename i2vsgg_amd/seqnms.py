"""Seq-NMS (Han et al., 2016): link the per-frame, per-class detections of a video into object tracks.

The stage between the detector's ``all_boxes[class][image]`` (``test_instance_styled.py``) and the boxes the relation
loop reads (``--target_gt_rels_path``).  The reference ran it outside its tree: test_net_instance_styleD_bilinear.py:209-211
dumps its input, faster_rcnn_SGG_emb.py:460-474 reads its output back.  The tool was not published, so the rules below are
this project's own; the host form (``seq_nms_arrays_host``) and the kernel (csrc/seqnms.hip, ``ops.seq_nms``) both follow them.

The rules.  A *group* is one (video, class); its frames are the video's frames in ascending frame number (a frame without
boxes of the class is present with zero boxes).

* Cap.  A frame contributes at most ``CAP = 64`` boxes to a group: the packer keeps the 64 best by score (equal scores: the
  earlier row), in their original row order; the rows beyond come back as suppressed.
* Arithmetic.  Boxes and scores are float32 and are widened to float64 exactly; everything that decides something is float64
  in the order written here.
* Overlap (``packing.overlap_plus1``), the +1 convention of lib/model/nms/nms_cpu.py:14,26-27: ``iw = (min(x2) - max(x1)) + 1``, ``ih`` likewise; 0 if
  either is ``<= 0``, else ``iw*ih / ((area_a + area_b) - iw*ih)`` with ``area = ((x2 - x1) + 1) * ((y2 - y1) + 1)``.
* Links.  Box a of frame t links to box b of frame t+1 when ``frame_no[t+1] == frame_no[t] + 1`` (a gap in the numbers
  breaks every link) and ``overlap >= link_iou``.
* One pass, over the boxes still alive, from the last frame to the first: ``best[t][a] = score[a] + max(best[t+1][b] over
  alive linked b)``, or ``score[a]`` alone without such a b; ``ptr[t][a]`` is that b (the lowest on ties) or none.  The pass
  starts at the alive (t, a) of largest ``best`` (ties: the lowest t, then the lowest a) and the path follows ``ptr``.
* Rescore.  The path's boxes get one new score: ``avg``, the float64 sum of their original scores in frame order divided by
  their number, rounded to float32; or ``max``.
* Suppress.  In each frame of the path the path's box leaves the alive set, and with it every alive box of that frame and
  group whose overlap with it is ``> nms_iou`` (strict, nms_cpu.py:31).
* Ids.  The path's boxes get the track id k = 0, 1, 2, ... in extraction order per group; suppressed boxes get -1 and keep
  their score.  Passes repeat until no box is alive.

After a path that spans frames ts..te only frames <= te can change, and below ts a frame whose ``best`` and ``ptr`` come out
unchanged ends the recomputation (frame t reads only frame t+1): both forms use this, it changes no result.
"""
import numpy as np

from .packing import cat, offsets, overlap_plus1

CAP = 64                     # boxes of one frame that take part in a group (csrc/seqnms.hip SQ_CAP)
RESCORE = ("avg", "max")


class Packed(object):
    """Flat arrays of a batch of groups (the layout of ``ops.seq_nms``) and where every packed box came from: slot f is
    image ``slot_image[f]``, group g is (``vids[g // n_classes]``, class ``g % n_classes``), box n is row ``row[n]`` of its
    cell ``all_boxes[class][image]``."""

    def __init__(self, vids, n_classes, group_off, frame_no, box_off, box, score, slot_image, row, cell_rows):
        self.vids, self.n_classes, self.group_off, self.frame_no, self.box_off = vids, n_classes, group_off, frame_no, box_off
        self.box, self.score, self.slot_image, self.row, self.cell_rows = box, score, slot_image, row, cell_rows


def _cell(c):
    return np.asarray(c, np.float32).reshape(-1, 5)


def frame_index_of_paths(paths, frames_per_video=0):
    """{path: (vid, fno)} for an imdb without video ids, the one rule of the command-line tools: the frames in the order of
    their paths, every ``frames_per_video`` consecutive ones a video "0", "1", ... numbered from 0 (0 or less: one video)."""
    per = frames_per_video if frames_per_video > 0 else max(len(paths), 1)
    return dict((path, (str(k // per), k % per)) for k, path in enumerate(sorted(paths)))


def pack(all_boxes, frame_index, score_thresh=0.0):
    """``all_boxes[j][i]``: (n, 5) float32 rows [x1, y1, x2, y2, score] of class j in image i (the nested list that
    ``test_instance_styled.py`` pickles; an empty cell may be ``[]``).  ``frame_index[i] = (vid, fno)``.  Rows with
    ``score < score_thresh`` are left out, then a cell is cut to its ``CAP`` best rows.  Groups are ordered by video (in
    the order of first appearance), then class."""
    n_classes, n_img = len(all_boxes), len(frame_index)
    for j in range(n_classes):
        if len(all_boxes[j]) != n_img:
            raise ValueError("seqnms.pack: class %d has %d images, frame_index has %d" % (j, len(all_boxes[j]), n_img))
    videos = {}
    for i, (vid, fno) in enumerate(frame_index):
        videos.setdefault(vid, []).append((int(fno), i))
    group_off, frame_no, counts, slot_image, box, score, row = [0], [], [], [], [], [], []
    cell_rows = np.zeros((n_classes, n_img), np.int64)
    for vid, frames in videos.items():
        frames.sort()
        if any(frames[k][0] == frames[k + 1][0] for k in range(len(frames) - 1)):
            raise ValueError("seqnms.pack: video %r has two frames with one number" % (vid,))
        for j in range(n_classes):
            for fno, i in frames:
                c = _cell(all_boxes[j][i])
                cell_rows[j, i] = len(c)
                if not np.isfinite(c).all():
                    raise ValueError("seqnms.pack: class %d, image %d holds a value that is not finite" % (j, i))
                keep = np.nonzero(c[:, 4] >= score_thresh)[0]
                if len(keep) > CAP:
                    keep = np.sort(keep[np.argsort(-c[keep, 4], kind="stable")[:CAP]])
                frame_no.append(fno)
                slot_image.append(i)
                counts.append(len(keep))
                box.append(c[keep, :4])
                score.append(c[keep, 4])
                row.append(keep)
            group_off.append(len(frame_no))
    box_off = offsets(counts, "seqnms.pack: more than 2^31 boxes")
    return Packed(list(videos), n_classes, np.asarray(group_off, np.int32), np.asarray(frame_no, np.int32), box_off,
                  cat(box, (4,), np.float32), cat(score, (), np.float32), np.asarray(slot_image, np.int64),
                  cat(row, (), np.int64), cell_rows)


def _group_host(frame_no, B, S32, link_iou, nms_iou, rescore):
    """One group: per frame the float64 boxes ``B[t]`` and the float32 scores ``S32[t]``.  Returns per frame (tid, new
    score), and the number of tracks."""
    nf = len(B)
    S = [s.astype(np.float64) for s in S32]
    cnt = [len(s) for s in S]
    link = [None] * nf
    for t in range(nf - 1):
        if int(frame_no[t + 1]) == int(frame_no[t]) + 1 and cnt[t] and cnt[t + 1]:
            link[t] = overlap_plus1(B[t], B[t + 1]) >= link_iou
    alive = [np.ones(n, bool) for n in cnt]
    best = [np.zeros(n) for n in cnt]
    ptr = [np.full(n, -1, np.int64) for n in cnt]
    tid = [np.full(n, -1, np.int32) for n in cnt]
    new = [s.copy() for s in S32]
    fmax, farg = np.full(nf, -np.inf), np.full(nf, -1, np.int64)
    ts, te, k, total = nf, nf - 1, 0, sum(cnt)
    while k < total:
        for t in range(te, -1, -1):
            al = alive[t]
            b, pb = S[t], np.full(cnt[t], -1, np.int64)
            if link[t] is not None:
                mask = link[t] & alive[t + 1][None, :]
                has = mask.any(1)
                cand = np.where(mask, best[t + 1][None, :], -np.inf)
                pb = np.where(has, cand.argmax(1), -1)               # the first maximum: the lowest b
                b = np.where(has, S[t] + np.where(has, cand.max(1), 0.0), S[t])
            changed = bool((((b != best[t]) | (pb != ptr[t])) & al).any())
            best[t], ptr[t] = np.where(al, b, best[t]), np.where(al, pb, ptr[t])
            idx = np.nonzero(al)[0]
            if len(idx):
                farg[t] = idx[np.argmax(best[t][idx])]
                fmax[t] = best[t][farg[t]]
            else:
                farg[t], fmax[t] = -1, -np.inf
            if k > 0 and t < ts and not changed:
                break
        if not (farg >= 0).any():
            break
        ts = int(np.argmax(np.where(farg >= 0, fmax, -np.inf)))          # the first maximum: the lowest t
        t, a, path = ts, int(farg[ts]), []
        while True:
            path.append((t, a))
            al = alive[t]
            kill = al &(overlap_plus1(B[t][a:a + 1], B[t])[0] > nms_iou)
            kill[a] = True
            alive[t] = al & ~kill
            nx = int(ptr[t][a])
            if nx < 0 or t + 1 >= nf:
                break
            t, a = t + 1, nx
        te = t
        if rescore == "max":
            ns = max(S32[t][a] for t, a in path)
        else:
            s = 0.0
            for t, a in path:
                s += float(S32[t][a])
            ns = np.float32(s / float(len(path)))
        for t, a in path:
            tid[t][a], new[t][a] = k, ns
        k += 1
    return tid, new, k


def seq_nms_arrays_host(pk, link_iou=0.5, nms_iou=0.3, rescore="avg", stats=None):
    """The rules of ``ops.seq_nms`` in numpy (vectorised per frame), on the same arrays, with the same outputs: (tid (N)
    int32, new_score (N) float32, n_tracks (G) int32).  ``stats`` (a dict) receives ``passes``, the number of tracks."""
    if rescore not in RESCORE:
        raise ValueError("seq_nms: rescore is 'avg' or 'max' (got %r)" % (rescore,))
    N, G = len(pk.score), len(pk.group_off) - 1
    tid, new, n_tracks = np.full(N, -1, np.int32), pk.score.astype(np.float32).copy(), np.zeros(G, np.int32)
    box64 = pk.box.astype(np.float64)
    for g in range(G):
        f0, f1 = int(pk.group_off[g]), int(pk.group_off[g + 1])
        if pk.box_off[f1] == pk.box_off[f0]:
            continue
        span = [(int(pk.box_off[f]), int(pk.box_off[f + 1])) for f in range(f0, f1)]
        t_, n_, k = _group_host(pk.frame_no[f0:f1], [box64[p:q] for p, q in span], [pk.score[p:q] for p, q in span],
                                float(link_iou), float(nms_iou), rescore)
        for (p, q), tt, nn in zip(span, t_, n_):
            tid[p:q], new[p:q] = tt, nn
        n_tracks[g] = k
    if stats is not None:
        stats["passes"] = int(n_tracks.sum())
    return tid, new, n_tracks


def seq_nms_arrays(pk, link_iou=0.5, nms_iou=0.3, rescore="avg", device=None):
    """``seq_nms_arrays_host`` (``device=None``) or the kernel, as numpy arrays."""
    if device is None:
        return seq_nms_arrays_host(pk, link_iou, nms_iou, rescore)
    from . import ops
    return tuple(t.cpu().numpy() for t in ops.seq_nms(pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score, link_iou, nms_iou,
                                                      rescore, device=device))


def scatter(pk, tid, new_score):
    """Per cell ``(j, i)`` with rows: (tid, score) over the cell's ORIGINAL rows.  A row that was not packed (below the score
    threshold or beyond the cap) has id -1, as a suppressed one; its score entry is nan (the caller holds the original)."""
    out = {}
    for g in range(len(pk.group_off) - 1):
        j = g % pk.n_classes
        for f in range(int(pk.group_off[g]), int(pk.group_off[g + 1])):
            i = int(pk.slot_image[f])
            n = int(pk.cell_rows[j, i])
            if n == 0:
                continue
            p, q = int(pk.box_off[f]), int(pk.box_off[f + 1])
            t, s = np.full(n, -1, np.int32), np.full(n, np.nan, np.float32)
            t[pk.row[p:q]], s[pk.row[p:q]] = tid[p:q], new_score[p:q]
            out[(j, i)] = (t, s)
    return out


def seq_nms(all_boxes, frame_index, link_iou=0.5, nms_iou=0.3, rescore="avg", score_thresh=0.0, device="cuda:0"):
    """Returns ``(all_boxes', tracks)``.  ``all_boxes'`` has the nested layout of ``all_boxes``: per cell the surviving boxes
    (those on a track) with their new scores, rows in descending new score (equal scores: the original row order), so
    ``eval_detections.py`` / ``detection_eval`` read it unchanged.  ``tracks[j][i]``: the int32 track ids of those rows
    (numbered per (video, class)).  A cell without rows is handed back as it came.  ``device=None`` runs the host form."""
    pk = pack(all_boxes, frame_index, score_thresh)
    tid, new = seq_nms_arrays(pk, link_iou, nms_iou, rescore, device)[:2]
    cells = scatter(pk, tid, new)
    n_classes, n_img = pk.n_classes, len(frame_index)
    out = [[all_boxes[j][i] for i in range(n_img)] for j in range(n_classes)]
    tracks = [[np.zeros(0, np.int32) for _ in range(n_img)] for _ in range(n_classes)]
    for (j, i), (t, s) in cells.items():
        keep = np.nonzero(t >= 0)[0]
        keep = keep[np.argsort(-s[keep], kind="stable")]
        c = _cell(all_boxes[j][i])[keep].copy()
        c[:, 4] = s[keep]
        out[j][i], tracks[j][i] = c, t[keep]
    return out, tracks


def to_annotations(all_boxes, tracks, names, min_score=0.7, max_per_class=10, min_len=1, frame_index=None):
    """``seq_nms``'s result as the pickle ``--target_gt_rels_path`` reads: {frame file name ``names[i]``: {"boxes" (unscaled
    pixels), "box_classes", "scores", "tids", "rels": []}}.  Per frame and class the first ``max_per_class`` rows with score
    ``> min_score`` are kept (the reference's own cut, faster_rcnn_SGG_emb.py:446-449), and of those the ones whose track
    has at least ``min_len`` members.  Track ids are per (video, class): ``frame_index[i] = (vid, fno)`` tells the videos
    apart when ``min_len > 1`` (None: one video)."""
    n_classes, n_img = len(all_boxes), len(names)
    length = {}
    if min_len > 1:
        for j in range(n_classes):
            for i in range(n_img):
                vid = frame_index[i][0] if frame_index is not None else None
                for t in np.asarray(tracks[j][i]).tolist():
                    length[(vid, j, t)] = length.get((vid, j, t), 0) + 1
    out = {}
    for i in range(n_img):
        vid = frame_index[i][0] if frame_index is not None else None
        boxes, classes, scores, tids = [], [], [], []
        for j in range(1, n_classes):
            c, t = _cell(all_boxes[j][i]), np.asarray(tracks[j][i])
            for r in range(min(int(max_per_class), len(c))):
                if c[r, 4] > min_score and (min_len <= 1 or length[(vid, j, int(t[r]))] >= min_len):
                    boxes.append([float(x) for x in c[r, :4]])
                    classes.append(j)
                    scores.append(float(c[r, 4]))
                    tids.append(int(t[r]))
        out[names[i]] = {"boxes": boxes, "box_classes": classes, "scores": scores, "tids": tids, "rels": []}
    return out
