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

A gap in the numbers, or one missed detection, therefore ends a track.  The second step, off by default, joins such tracklets
and interpolates the missed boxes: ``stitch_arrays_host`` states its rules, ``seq_nms_stitched`` is ``seq_nms`` followed by it
(csrc/track_stitch.hip, ``ops.track_stitch``).  ``seq_nms`` itself does what it did.
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


# ---------------------------------------------------------------------------------------------------------------------
# track stitching: the second step, off by default
# ---------------------------------------------------------------------------------------------------------------------
MAX_STITCH_GAP = 7           # missing frame numbers a link may bridge (csrc/track_stitch.hip TS_MAXGAP)


def _stitch_args(pk, tid, max_gap, rescore):
    if rescore not in RESCORE:
        raise ValueError("track_stitch: rescore is 'avg' or 'max' (got %r)" % (rescore,))
    if isinstance(max_gap, bool) or int(max_gap) != max_gap or not 1 <= int(max_gap) <= MAX_STITCH_GAP:
        raise ValueError("track_stitch: max_gap is an int in [1, %d] (got %r)" % (MAX_STITCH_GAP, max_gap))
    tid = np.ascontiguousarray(np.asarray(tid, np.int32).reshape(-1))
    if len(tid) != len(pk.score):
        raise ValueError("track_stitch: %d track ids for %d boxes" % (len(tid), len(pk.score)))
    return tid, int(max_gap)


def _group_tracklets(g, frame_no, span, tid):
    """The tracklets of group g, in order of their start: lists [tid, start frame number, start box, end frame number, end
    box, end slot, start slot, members in frame order].  A table Seq-NMS cannot have written is a ``ValueError``."""
    bad = lambda why: ValueError("track_stitch: group %d is malformed: %s" % (g, why))
    n_box = span[-1][1] - span[0][0] if span else 0
    tr, open_, seen, prev_no = [], {}, set(), None
    for f, (p, q) in enumerate(span):
        fno = int(frame_no[f])
        if q < p or (prev_no is not None and fno <= prev_no):
            raise bad("the offsets or the frame numbers do not ascend at slot %d" % f)
        follows = prev_no is not None and fno == prev_no + 1
        now = {}
        for n in range(p, q):
            t = int(tid[n])
            if t == -1:
                continue
            if t < -1 or t >= n_box:
                raise bad("track id %d lies outside [-1, %d)" % (t, n_box))
            if t in now:
                raise bad("track id %d twice in slot %d" % (t, f))
            k = open_.get(t) if follows else None
            if k is None:
                if t in seen:
                    raise bad("track id %d is not one run of consecutive frame numbers" % t)
                seen.add(t)
                k = len(tr)
                tr.append([t, fno, n, fno, n, f, f, [n]])
            else:
                tr[k][3], tr[k][4], tr[k][5] = fno, n, f
                tr[k][7].append(n)
            now[t] = k
        open_, prev_no = now, fno
    return tr


def stitch_arrays_host(pk, tid, max_gap=3, stitch_iou=0.3, rescore="avg", stats=None):
    """Track stitching: Seq-NMS's tracklets joined across missed frames, the boxes of the missed frames interpolated.  The
    rules are this project's own; this host form and the kernel (csrc/track_stitch.hip, ``ops.track_stitch``) both follow
    them.  Everything that decides something is float64 on exactly widened float32 inputs, in the operation order written here.

    Inputs: Seq-NMS's tables (``pk``: ``group_off``, ``frame_no``, ``box_off``, ``box``, ``score`` -- the ORIGINAL scores),
    its ``tid`` output, ``max_gap`` in [1, 7], ``stitch_iou``, ``rescore``.

    * Tracklets.  A tracklet is a Seq-NMS track (group, tid): by construction one run of consecutive frame numbers with one
      box per frame.  Its start box is its box in a slot whose previous slot either does not carry the preceding frame
      number or has no box of that tid; its end box is the mirror image.  Boxes with tid -1 take no part and come back
      untouched.
    * Order.  A group's tracklets are visited as successors B in ascending (start frame number, tid).
    * Candidates of B.  A tracklet A of the same group is a candidate when A has no successor yet, ``1 <= s_B - e_A - 1 <=
      max_gap`` (missing frame NUMBERS; adjacent tracklets are never joined: Seq-NMS already decided about them) and
      ``packing.overlap_plus1(end box of A, start box of B) >= stitch_iou``.
    * Choice.  B takes the candidate of largest overlap; ties go to the smaller gap, then to the lower tid.  A then has its
      successor and B its predecessor: first come, first served in visiting order, no claim is revisited.
    * Ids.  A chain is a maximal run of linked tracklets, its root its first tracklet.  New ids are dense per group: the new
      id of a chain is the number of roots with a lower Seq-NMS tid.  Seq-NMS's ids are dense, so without a link the ids are
      Seq-NMS's.
    * Score.  All boxes of a chain share one score.  ``avg``: the float64 sum of the ORIGINAL scores of the chain's real
      members in frame order, from 0.0, divided by their number, rounded to float32; ``max``: their maximum.  For a chain of
      one tracklet this is bit for bit the score Seq-NMS gave.
    * Interpolation.  A link from A (end box a at frame number e) to B (start box b at frame number s) gives every slot of
      the group with a frame number f strictly between e and s one new row: ``w = double(f - e) / double(s - e)``, per
      coordinate ``c = a_c + (b_c - a_c) * w`` rounded to float32, with the chain's new id and the chain's score.  Frame
      numbers the video does not have get nothing, so a link may add fewer than ``s - e - 1`` rows, or none.  Rows are
      emitted per group in link order -- B's visiting order -- then ascending frame.
    * Malformed.  A group whose offsets or frame numbers do not ascend, that holds a tid twice in one slot, a tid outside
      [-1, boxes of the group) or a tid that is not one run of consecutive frame numbers is no table of Seq-NMS's:
      ``ValueError`` here, the status word on the device, both naming the group.

    Returns (``tid2`` (N) int32, ``score2`` (N) float32, ``n_tracks2`` (G) int32, ``fill_off`` (G+1) int32, ``fill_slot``
    (M) int32: the slot a new row belongs to, ``fill_tid`` (M) int32, ``fill_box`` (M,4) float32, ``fill_score`` (M) float32).
    ``stats`` (a dict) receives ``links``, ``chains_of_three`` (chains that reach a third tracklet), ``claimed_met``
    (candidates that qualified by gap and overlap but were already taken), ``multi`` (successors with more than one free
    candidate), ``links_over_absent_numbers`` (links that emit fewer rows than missing numbers) and ``ties`` (successors whose
    best overlap two free candidates share)."""
    tid, max_gap = _stitch_args(pk, tid, max_gap, rescore)
    stitch_iou = float(stitch_iou)
    N, G = len(pk.score), len(pk.group_off) - 1
    tid2, score2, n_tracks2 = tid.copy(), pk.score.astype(np.float32).copy(), np.zeros(G, np.int32)
    box64 = pk.box.astype(np.float64).reshape(-1, 4)
    counts, f_slot, f_tid, f_box, f_score = [], [], [], [], []
    st = dict.fromkeys(("links", "chains_of_three", "claimed_met", "multi", "links_over_absent_numbers", "ties"), 0)
    for g in range(G):
        f0, f1 = int(pk.group_off[g]), int(pk.group_off[g + 1])
        if not 0 <= f0 <= f1 <= len(pk.frame_no):
            raise ValueError("track_stitch: group %d is malformed: its slots lie outside the table" % g)
        span = [(int(pk.box_off[f]), int(pk.box_off[f + 1])) for f in range(f0, f1)]
        if span and not 0 <= span[0][0] <= span[-1][1] <= N:
            raise ValueError("track_stitch: group %d is malformed: its boxes lie outside the table" % g)
        tr = _group_tracklets(g, pk.frame_no[f0:f1], span, tid)
        T = len(tr)
        end_no, end_box = np.array([t[3] for t in tr], np.int64), np.array([t[4] for t in tr], np.int64)
        old = np.array([t[0] for t in tr], np.int64)
        succ, pred, links = np.full(T, -1, np.int64), np.full(T, -1, np.int64), []
        for b in sorted(range(T), key=lambda k: (tr[k][1], tr[k][0])):
            gap = tr[b][1] - end_no - 1
            cand = np.nonzero((gap >= 1) & (gap <= max_gap))[0]
            if not len(cand):
                continue
            ov = overlap_plus1(box64[end_box[cand]], box64[tr[b][2]:tr[b][2] + 1])[:, 0]
            st["claimed_met"] += int(((ov >= stitch_iou) & (succ[cand] >= 0)).sum())
            keep = (ov >= stitch_iou) & (succ[cand] < 0)
            cand, ov = cand[keep], ov[keep]
            if not len(cand):
                continue
            st["multi"] += len(cand) > 1
            st["ties"] += int((ov == ov.max()).sum()) > 1
            a = int(cand[min(range(len(cand)), key=lambda i: (-ov[i], gap[cand[i]], old[cand[i]]))])
            succ[a], pred[b] = b, a
            links.append((a, b))
        roots = [k for k in range(T) if pred[k] < 0]
        new_id = dict((k, i) for i, k in enumerate(sorted(roots, key=lambda k: tr[k][0])))
        chain_id, chain_score = {}, {}
        for r in roots:
            members, k, length = [], r, 0
            while k >= 0:
                members += tr[k][7]
                chain_id[k] = new_id[r]
                k, length = int(succ[k]), length + 1
            st["chains_of_three"] += length >= 3
            if rescore == "max":
                ns = max(np.float32(pk.score[n]) for n in members)
            else:
                s = 0.0
                for n in members:
                    s += float(pk.score[n])
                ns = np.float32(s / float(len(members)))
            chain_score[new_id[r]] = ns
            tid2[members], score2[members] = new_id[r], ns
        n_tracks2[g] = len(roots)
        rows = 0
        for a, b in links:
            e, s, pa, pb = tr[a][3], tr[b][1], box64[tr[a][4]], box64[tr[b][2]]
            added = 0
            for f in range(f0 + tr[a][5] + 1, f0 + tr[b][6]):
                w = float(int(pk.frame_no[f]) - e) / float(s - e)
                f_slot.append(f)
                f_tid.append(chain_id[b])
                f_box.append((pa + (pb - pa) * w).astype(np.float32))
                f_score.append(chain_score[chain_id[b]])
                added += 1
            st["links_over_absent_numbers"] += added < s - e - 1
            rows += added
        st["links"] += len(links)
        counts.append(rows)
    if stats is not None:
        stats.update((k, int(v)) for k, v in st.items())
    return (tid2, score2, n_tracks2, offsets(counts, "track_stitch: more than 2^31 new rows"), np.asarray(f_slot, np.int32).reshape(-1),
            np.asarray(f_tid, np.int32).reshape(-1), cat([x.reshape(1, 4) for x in f_box], (4,), np.float32),
            np.asarray(f_score, np.float32).reshape(-1))


def stitch_arrays(pk, tid, max_gap=3, stitch_iou=0.3, rescore="avg", device=None, stats=None):
    """``stitch_arrays_host`` (``device=None``) or the kernel (``ops.track_stitch``), as numpy arrays.  ``stats`` is the host
    form's alone."""
    if device is None:
        return stitch_arrays_host(pk, tid, max_gap, stitch_iou, rescore, stats)
    from . import ops
    tid, max_gap = _stitch_args(pk, tid, max_gap, rescore)
    return tuple(t.cpu().numpy() for t in ops.track_stitch(pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score, tid, max_gap,
                                                           stitch_iou, rescore, device=device))


def seq_nms_stitched(all_boxes, frame_index, link_iou=0.5, nms_iou=0.3, rescore="avg", score_thresh=0.0, max_gap=3, stitch_iou=0.3,
                     device="cuda:0", stats=None):
    """``seq_nms`` followed by the stitching step (``stitch_arrays_host`` has the rules).  Returns ``(all_boxes', tracks,
    interp)`` in ``seq_nms``'s nested layout: per cell the surviving boxes with their chain's score and, merged in, the
    interpolated rows of the cell's slot; ``tracks[j][i]`` the new ids, ``interp[j][i]`` one bool per row (True: interpolated).
    Rows are in descending score as ``seq_nms`` orders them, stable over the surviving rows in their original order followed
    by the interpolated ones in the order they were emitted.  A cell without rows is handed back as it came.  ``max_gap = 0``
    skips the step: ``seq_nms``'s own result with ``interp`` all False.  ``device=None`` runs both host forms.  ``stats`` (a
    dict) receives ``links`` and ``added``."""
    pk = pack(all_boxes, frame_index, score_thresh)
    tid, new, n_tracks = seq_nms_arrays(pk, link_iou, nms_iou, rescore, device)
    links, fill = 0, {}
    if max_gap:
        tid2, new, n_tracks2, fill_off, fill_slot, fill_tid, fill_box, fill_score = stitch_arrays(pk, tid, max_gap, stitch_iou, rescore,
                                                                                                 device)
        links, tid = int(n_tracks.sum()) - int(n_tracks2.sum()), tid2          # every link takes one root away
        for g in range(len(pk.group_off) - 1):
            for r in range(int(fill_off[g]), int(fill_off[g + 1])):
                fill.setdefault((g % pk.n_classes, int(pk.slot_image[fill_slot[r]])), []).append(r)
    if stats is not None:
        stats["links"], stats["added"] = links, sum(len(v) for v in fill.values())
    cells = scatter(pk, tid, new)
    n_classes, n_img = pk.n_classes, len(frame_index)
    out = [[all_boxes[j][i] for i in range(n_img)] for j in range(n_classes)]
    tracks = [[np.zeros(0, np.int32) for _ in range(n_img)] for _ in range(n_classes)]
    interp = [[np.zeros(0, bool) for _ in range(n_img)] for _ in range(n_classes)]
    for j, i in sorted(set(cells) | set(fill)):
        c, t = np.zeros((0, 5), np.float32), np.zeros(0, np.int32)
        if (j, i) in cells:
            t, s = cells[(j, i)]
            keep = np.nonzero(t >= 0)[0]
            c, t = _cell(all_boxes[j][i])[keep].copy(), t[keep]
            c[:, 4] = s[keep]
        rows = fill.get((j, i), [])
        mark = np.concatenate([np.zeros(len(c), bool), np.ones(len(rows), bool)])
        if rows:
            c = np.concatenate([c, np.concatenate([fill_box[rows], fill_score[rows][:, None]], 1)]).astype(np.float32)
            t = np.concatenate([t, fill_tid[rows]]).astype(np.int32)
        order = np.argsort(-c[:, 4], kind="stable")
        out[j][i], tracks[j][i], interp[j][i] = c[order], t[order], mark[order]
    return out, tracks, interp


def to_annotations(all_boxes, tracks, names, min_score=0.7, max_per_class=10, min_len=1, frame_index=None, interp=None):
    """``seq_nms``'s result as the pickle ``--target_gt_rels_path`` reads: {frame file name ``names[i]``: {"boxes" (unscaled
    pixels), "box_classes", "scores", "tids", "rels": []}}.  Per frame and class the first ``max_per_class`` rows with score
    ``> min_score`` are kept (the reference's own cut, faster_rcnn_SGG_emb.py:446-449), and of those the ones whose track
    has at least ``min_len`` members.  Track ids are per (video, class): ``frame_index[i] = (vid, fno)`` tells the videos
    apart when ``min_len > 1`` (None: one video).  ``interp`` (``seq_nms_stitched``'s third result): every entry also gets
    an ``"interp"`` list, one bool per box; None writes no such key."""
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
        boxes, classes, scores, tids, marks = [], [], [], [], []
        for j in range(1, n_classes):
            c, t = _cell(all_boxes[j][i]), np.asarray(tracks[j][i])
            for r in range(min(int(max_per_class), len(c))):
                if c[r, 4] > min_score and (min_len <= 1 or length[(vid, j, int(t[r]))] >= min_len):
                    boxes.append([float(x) for x in c[r, :4]])
                    classes.append(j)
                    scores.append(float(c[r, 4]))
                    tids.append(int(t[r]))
                    if interp is not None:
                        marks.append(bool(interp[j][i][r]))
        out[names[i]] = {"boxes": boxes, "box_classes": classes, "scores": scores, "tids": tids, "rels": []}
        if interp is not None:
            out[names[i]]["interp"] = marks
    return out
