"""torch-facing wrappers of the packed-table ops: the evaluation and target kernels that read flat arrays and offset tables
(csrc/seqnms.hip, track_stitch.hip, video.hip, video_nms.hip, det_eval.hip, recognition.hip, relation_features.hip, relation_targets.hip, image_relations.hip,
proposal_eval.hip;
csrc/table_common.h is what those share, ``packing.py`` what their host packers share).  ``ops`` re-exports the public names.

Every op takes arrays or tensors, stages them on the device, launches on torch's current stream and, unless it says
otherwise, reads its status word back: a malformed table raises ``I2VError`` naming the first bad entry.  The steps that are
the same in every op are the helpers below; the table names, the size checks and the ``lib.i2v_...`` call stay in the op.
"""
import numpy as np
import torch

from . import launch
from ._lib import I2VError, check, lib, need_cuda, ptr, stream


def _device(device, host_form, default="cuda"):
    """The GPU an op runs on: ``device``, or ``default`` when it is None.  Anything but a GPU is refused, naming the op's
    host form."""
    dev = torch.device(device if device is not None else default)
    if dev.type != "cuda":
        raise I2VError("i2vsgg_amd ops run on the GPU only (got device %s); %s is the host form" % (dev, host_form))
    return dev


def _to_dev(x, dtype, device):
    return torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()


def _stage(dev, dtype, *tables):
    """The tables as contiguous ``dtype`` tensors on the device."""
    return tuple(_to_dev(x, dtype, dev) for x in tables)


def _max_rows(off):
    """The largest row count of an offset table (0 for an empty one); taken on the host, before the table is staged."""
    counts = np.diff(np.asarray(torch.as_tensor(off).cpu()))
    return int(counts.max()) if len(counts) else 0


def _launch(dev, what, call, ws_bytes, tag):
    """Runs ``call(ws pointer, ws bytes, stream)``, the tail of every table entry point, with the device current and a
    workspace of ``ws_bytes``, and checks its return code.  The workspace is the launch context's buffer ``tag``; ``tag`` None:
    a zeroed buffer of the call's own.  Returns the workspace, whose header holds the status words."""
    with torch.cuda.device(dev):
        ws = launch.workspace(ws_bytes, dev, tag) if tag is not None else torch.zeros((ws_bytes,), device=dev, dtype=torch.uint8)
        check(call(ptr(ws), ws.numel(), stream()), what)
    return ws


def _status(ws, word, what, entry="entry", text="the offset tables are out of range at", tail=""):
    """Reads status word ``word`` of the workspace (the caller reads the results next anyway): 0, or 1 + the first malformed
    ``entry``, which raises."""
    bad = int(ws[4 * word:4 * word + 4].view(torch.int32).item())
    if bad:
        raise I2VError("%s: %s %s %d%s" % (what, text, entry, bad - 1, tail))


def relation_topk(rel_score, conf, ixs, ixo, k=100):
    """Top-k (pair, predicate) cells of ``rel_score * conf[ixs] * conf[ixo]`` (lib/utils.py:584-628), on the device.
    rel_score (n_pairs, n_rel) fp32, conf (n_boxes,) fp32, ixs / ixo (n_pairs,) int64.  Returns (pair, pred, conf):
    int32, int32, fp32 tensors of length min(k, n_pairs * n_rel), descending."""
    need_cuda(rel_score, conf, ixs, ixo)
    rel_score, conf = rel_score.float().contiguous(), conf.float().contiguous()
    ixs, ixo = ixs.long().contiguous(), ixo.long().contiguous()
    n_pairs, n_rel = rel_score.shape
    k = min(int(k), n_pairs * n_rel)
    dev = rel_score.device
    pair = torch.empty((k,), device=dev, dtype=torch.int32)
    pred = torch.empty((k,), device=dev, dtype=torch.int32)
    out = torch.empty((k,), device=dev, dtype=torch.float32)
    if n_pairs * n_rel == 0:                                     # no cell to rank: the entry point takes no empty table
        return pair, pred, out
    ws = launch.workspace(lib.i2v_relation_topk_workspace_bytes(n_pairs, n_rel), dev, "reltopk")
    check(lib.i2v_relation_topk(ptr(rel_score), ptr(conf), ptr(ixs), ptr(ixo), n_pairs, n_rel, k, ptr(pair), ptr(pred), ptr(out),
                                ptr(ws), ws.numel(), stream()), "relation_topk")
    return pair, pred, out


def video_associate(frame_off, frame_no, pred_off, score, triplet, boxes, device=None):
    """Frame-to-video association of a packed batch of videos in one launch (include/i2vsgg_hip.h, i2v_video_associate;
    ``video.pack_frames`` builds the arrays).  Arrays or tensors: frame_off (V+1), frame_no (F), pred_off (F+1) int32,
    score (P) fp64, triplet (P,3) int32, boxes (P,8) fp64.  Returns device tensors (rel_id (P) int32, rel_start (P) int32,
    rel_len (P) int32, rel_score (P) fp64, n_rel (V) int32)."""
    dev = _device(device, "video.associate(device=None)")
    max_per_frame = _max_rows(pred_off)
    frame_off, frame_no, pred_off, triplet = _stage(dev, torch.int32, frame_off, frame_no, pred_off, triplet)
    score, boxes = _stage(dev, torch.float64, score, boxes)
    V, F, P = frame_off.numel() - 1, frame_no.numel(), score.numel()
    if pred_off.numel() != F + 1 or triplet.numel() != 3 * P or boxes.numel() != 8 * P:
        raise ValueError("video_associate: array sizes do not agree")
    rel_id, rel_start, rel_len = (torch.zeros((P,), device=dev, dtype=torch.int32) for _ in range(3))
    rel_score = torch.zeros((P,), device=dev, dtype=torch.float64)
    n_rel = torch.zeros((max(V, 0),), device=dev, dtype=torch.int32)
    ws = _launch(dev, "video_associate", lambda *tail: lib.i2v_video_associate(
        ptr(frame_off), ptr(frame_no), ptr(pred_off), ptr(score), ptr(triplet), ptr(boxes), V, F, P, max_per_frame, ptr(rel_id),
        ptr(rel_start), ptr(rel_len), ptr(rel_score), ptr(n_rel), *tail), lib.i2v_video_associate_workspace_bytes(V, F, P), "video")
    if V > 0:
        _status(ws, 0, "video_associate")
    return rel_id, rel_start, rel_len, rel_score, n_rel


def video_associate_tracks(frame_off, frame_no, pred_off, score, key, since, max_gap=0, device=None, read_status=True):
    """Association along object tracks for a packed batch of videos in one launch (include/i2vsgg_hip.h,
    i2v_video_associate_tracks; ``video.pack_track_frames`` builds the arrays, ``video.associate_tracks_arrays_host`` is the
    numpy form).  Arrays or tensors: frame_off (V+1), frame_no (F), pred_off (F+1) int32, score (P) fp64, key (P,3) int32,
    since (P) int32; ``max_gap`` an int in [0, 7].  Returns device tensors (rel_id (P), rel_start (P), rel_end (P), rel_len (P)
    int32, rel_score (P) fp64, n_rel (V) int32).  ``read_status=False`` returns what the kernel wrote for the well-formed
    frames without raising for the malformed ones."""
    dev = _device(device, "video.associate_tracks(device=None)")
    if isinstance(max_gap, bool) or int(max_gap) != max_gap:
        raise ValueError("video_associate_tracks: max_gap is an int in [0, 7] (got %r)" % (max_gap,))
    frame_off, frame_no, pred_off, key, since = _stage(dev, torch.int32, frame_off, frame_no, pred_off, key, since)
    score, = _stage(dev, torch.float64, score)
    V, F, P = frame_off.numel() - 1, frame_no.numel(), score.numel()
    if V < 0 or pred_off.numel() != F + 1 or key.numel() != 3 * P or since.numel() != P:
        raise ValueError("video_associate_tracks: array sizes do not agree")
    rel_id, rel_start, rel_end, rel_len = (torch.zeros((P,), device=dev, dtype=torch.int32) for _ in range(4))
    rel_score = torch.zeros((P,), device=dev, dtype=torch.float64)
    n_rel = torch.zeros((V,), device=dev, dtype=torch.int32)
    ws = _launch(dev, "video_associate_tracks", lambda *tail: lib.i2v_video_associate_tracks(
        ptr(frame_off), ptr(frame_no), ptr(pred_off), ptr(score), ptr(key), ptr(since), V, F, P, int(max_gap), ptr(rel_id),
        ptr(rel_start), ptr(rel_end), ptr(rel_len), ptr(rel_score), ptr(n_rel), *tail),
        lib.i2v_video_associate_tracks_workspace_bytes(V, F, P), "video")
    if read_status and V > 0:
        _status(ws, 0, "video_associate_tracks", "frame", "the tables are out of range, or a frame holds more than 100 predictions, "
                "a frame number that does not ascend or a repeated key, at")
    return rel_id, rel_start, rel_end, rel_len, rel_score, n_rel


def video_viou_match(pred_off, pred_rel, pred_score, gt_off, gt_rel, boxes, viou_threshold=0.5, device=None):
    """Trajectory overlaps and the detection metric's greedy matching for a packed batch of videos
    (include/i2vsgg_hip.h, i2v_video_viou_match; ``video.pack_eval`` builds the arrays).  Returns device tensors (ov
    (n_pred, max_gt) fp64, hit (n_pred) int32, hit_ov (n_pred) fp64)."""
    dev = _device(device, "video.match(device=None)")
    max_pred, max_gt = _max_rows(pred_off), _max_rows(gt_off)
    pred_off, gt_off, pred_rel, gt_rel = _stage(dev, torch.int32, pred_off, gt_off, pred_rel, gt_rel)
    pred_score, boxes = _stage(dev, torch.float64, pred_score, boxes)
    V, NP, NG, NB = pred_off.numel() - 1, pred_score.numel(), gt_rel.numel() // 10, boxes.numel() // 4
    if gt_off.numel() != V + 1 or pred_rel.numel() != 10 * NP or gt_rel.numel() != 10 * NG or boxes.numel() != 4 * NB:
        raise ValueError("video_viou_match: array sizes do not agree")
    ov = torch.full((NP, max_gt), -1.0, device=dev, dtype=torch.float64)
    hit = torch.full((NP,), -1, device=dev, dtype=torch.int32)
    hit_ov = torch.full((NP,), -1.0, device=dev, dtype=torch.float64)
    ws = _launch(dev, "video_viou_match", lambda *tail: lib.i2v_video_viou_match(
        ptr(pred_off), ptr(pred_rel), ptr(pred_score), ptr(gt_off), ptr(gt_rel), ptr(boxes), V, NP, NG, NB, max_pred, max_gt,
        float(viou_threshold), ptr(ov), ptr(hit), ptr(hit_ov), *tail), lib.i2v_video_viou_match_workspace_bytes(NP, NG), "video")
    if V > 0 and NP > 0:
        _status(ws, 0, "video_viou_match")
    return ov, hit, hit_ov


def video_relation_nms(cell_off, rel, boxes, viou_threshold, device=None, read_status=True):
    """Greedy suppression of duplicate video relations by trajectory overlap, every (video, triplet) cell of a packed batch
    in one launch (include/i2vsgg_hip.h, i2v_video_relation_nms; ``video.pack_nms`` builds the arrays, ``video.suppress`` states
    the rules and ``video.suppress_arrays_host`` is the numpy form).  Arrays or tensors: cell_off (C+1) int32, rel (R,10) int32
    (the matcher's relation row, a cell's rows in rank order), boxes (n_boxes,4) fp64; ``viou_threshold`` in [0, 1].  Returns
    device tensors (keep (R) int32, by (R) int32, by_ov (R) fp64, vol (R,2) fp64).  A malformed cell raises ``I2VError`` naming
    it; ``read_status=False`` returns what the kernel wrote for the well-formed cells instead (a malformed cell's rows stay
    keep 0, by -1, by_ov -1.0, vol 0.0)."""
    dev = _device(device, "video.suppress(device=None)")
    cell_off, rel = _stage(dev, torch.int32, cell_off, rel)
    boxes, = _stage(dev, torch.float64, boxes)
    C, R, NB = cell_off.numel() - 1, rel.numel() // 10, boxes.numel() // 4
    if C < 0 or rel.numel() != 10 * R or boxes.numel() != 4 * NB:
        raise ValueError("video_relation_nms: array sizes do not agree")
    keep = torch.zeros((R,), device=dev, dtype=torch.int32)
    by = torch.full((R,), -1, device=dev, dtype=torch.int32)
    by_ov = torch.full((R,), -1.0, device=dev, dtype=torch.float64)
    vol = torch.zeros((R, 2), device=dev, dtype=torch.float64)
    ws = _launch(dev, "video_relation_nms", lambda *tail: lib.i2v_video_relation_nms(
        ptr(cell_off), ptr(rel), ptr(boxes), C, R, NB, float(viou_threshold), ptr(keep), ptr(by), ptr(by_ov), ptr(vol), *tail),
        lib.i2v_video_relation_nms_workspace_bytes(C, R), "video")
    if read_status and C > 0 and R > 0:
        _status(ws, 0, "video_relation_nms", "cell", "the tables are out of range, a cell holds more than 4096 relations or a "
                "trajectory disagrees with its duration, at")
    return keep, by, by_ov, vol


def seq_nms(group_off, frame_no, box_off, box, score, link_iou=0.5, nms_iou=0.3, rescore="avg", device=None):
    """Seq-NMS of a packed batch of (video, class) groups in one launch (include/i2vsgg_hip.h, i2v_seqnms; ``seqnms.pack``
    builds the arrays).  Arrays or tensors: group_off (G+1), frame_no (F), box_off (F+1) int32, box (N,4) fp32, score (N)
    fp32.  Returns device tensors (tid (N) int32, new_score (N) fp32, n_tracks (G) int32)."""
    dev = _device(device, "seqnms.seq_nms(device=None)")
    if rescore not in ("avg", "max"):
        raise ValueError("seq_nms: rescore is 'avg' or 'max' (got %r)" % (rescore,))
    group_off, frame_no, box_off = _stage(dev, torch.int32, group_off, frame_no, box_off)
    box, score = _stage(dev, torch.float32, box, score)
    G, F, N = group_off.numel() - 1, frame_no.numel(), score.numel()
    if G < 0 or box_off.numel() != F + 1 or box.numel() != 4 * N:
        raise ValueError("seq_nms: array sizes do not agree")
    tid = torch.full((N,), -1, device=dev, dtype=torch.int32)
    new_score = score.clone()
    n_tracks = torch.zeros((G,), device=dev, dtype=torch.int32)
    ws = _launch(dev, "seq_nms", lambda *tail: lib.i2v_seqnms(
        ptr(group_off), ptr(frame_no), ptr(box_off), ptr(box), ptr(score), G, F, N, float(link_iou), float(nms_iou),
        1 if rescore == "max" else 0, ptr(tid), ptr(new_score), ptr(n_tracks), *tail), lib.i2v_seqnms_workspace_bytes(G, F, N), "seqnms")
    if G > 0:
        _status(ws, 0, "seq_nms", "group")
    return tid, new_score, n_tracks


def track_stitch(group_off, frame_no, box_off, box, score, tid, max_gap=3, stitch_iou=0.3, rescore="avg", device=None):
    """The stitching step after Seq-NMS for a packed batch of groups (include/i2vsgg_hip.h, i2v_track_stitch;
    ``seqnms.stitch_arrays_host`` states the rules and is the numpy form).  Arrays or tensors: ``seq_nms``'s tables (score: the
    original scores) and its ``tid`` (N) int32; ``max_gap`` an int in [1, 7].  Returns device tensors (tid2 (N) int32, score2
    (N) fp32, n_tracks2 (G) int32, fill_off (G+1) int32, fill_slot (M) int32, fill_tid (M) int32, fill_box (M,4) fp32,
    fill_score (M) fp32), M = fill_off[G] new rows; a malformed group raises ``I2VError`` naming it."""
    dev = _device(device, "seqnms.stitch_arrays_host")
    if rescore not in ("avg", "max"):
        raise ValueError("track_stitch: rescore is 'avg' or 'max' (got %r)" % (rescore,))
    if isinstance(max_gap, bool) or int(max_gap) != max_gap:
        raise ValueError("track_stitch: max_gap is an int in [1, 7] (got %r)" % (max_gap,))
    group_off, frame_no, box_off, tid = (t.reshape(-1) for t in _stage(dev, torch.int32, group_off, frame_no, box_off, tid))
    box, score = _stage(dev, torch.float32, box, score)
    G, F, N, max_gap = group_off.numel() - 1, frame_no.numel(), score.numel(), int(max_gap)
    if G < 0 or box_off.numel() != F + 1 or box.numel() != 4 * N or tid.numel() != N:
        raise ValueError("track_stitch: array sizes do not agree")
    rows = max(max_gap, 0) * N                                   # the bound the entry point states; M of them are written
    tid2, score2 = tid.clone(), score.clone()                    # what a malformed group keeps
    n_tracks2 = torch.zeros((G,), device=dev, dtype=torch.int32)
    fill_off = torch.zeros((G + 1,), device=dev, dtype=torch.int32)
    fill_slot, fill_tid = (torch.zeros((rows,), device=dev, dtype=torch.int32) for _ in range(2))
    fill_box, fill_score = torch.zeros((rows, 4), device=dev), torch.zeros((rows,), device=dev)
    ws = _launch(dev, "track_stitch", lambda *tail: lib.i2v_track_stitch(
        ptr(group_off), ptr(frame_no), ptr(box_off), ptr(box), ptr(score), ptr(tid), G, F, N, max_gap, float(stitch_iou),
        1 if rescore == "max" else 0, ptr(tid2), ptr(score2), ptr(n_tracks2), ptr(fill_off), ptr(fill_slot), ptr(fill_tid),
        ptr(fill_box), ptr(fill_score), *tail), lib.i2v_track_stitch_workspace_bytes(G, F, N, max_gap), "track_stitch")
    if G == 0:
        return tid2, score2, n_tracks2, fill_off, fill_slot[:0], fill_tid[:0], fill_box[:0], fill_score[:0]
    _status(ws, 0, "track_stitch", "group", "the tables are out of range, the frame numbers do not ascend or a track id is repeated "
            "in a slot, out of range or not one run, at")
    M = int(fill_off[G].item())
    return tid2, score2, n_tracks2, fill_off, fill_slot[:M], fill_tid[:M], fill_box[:M], fill_score[:M]


def relation_targets(det_off, det_box, det_cls, gt_off, gt_box, gt_cls, rel_off, rel, u, ih, iw, n_rel, device=None, read_status=True):
    """The rel_det targets of a minibatch in two launches (include/i2vsgg_hip.h, i2v_relation_targets; the rules and the
    tables: ``i2vsgg_amd.relation_targets``, whose ``pack`` builds them).  Arrays or tensors; ``u`` (N_r, 10) uint32 (a tensor:
    its int32 view).  Returns a dict of device tensors: rel5 (F*64, 5) fp32, bounds (F*64, 2, 4) int32, labels (F*64, n_rel)
    fp32, ixs / ixo (F*64) int64, w (F*64) fp32, n_pairs / n_dropped (F) int32, samp (N_r, 10, 2) int32 and ``status`` (the
    int32 status word).  ``read_status=False`` leaves the status word on the device: nothing is read back, the call only enqueues."""
    dev = _device(device, "relation_targets.relation_targets_host")
    if isinstance(u, np.ndarray):
        u = np.ascontiguousarray(u, np.uint32).view(np.int32)
    elif torch.is_tensor(u) and u.dtype != torch.int32:
        u = u.view(torch.int32)
    det_off, gt_off, rel_off, det_cls, gt_cls, rel, u = _stage(dev, torch.int32, det_off, gt_off, rel_off, det_cls, gt_cls, rel, u)
    det_box, gt_box, ih, iw = _stage(dev, torch.float64, det_box, gt_box, ih, iw)
    F, ND, NG, NR, n_rel = ih.numel(), det_cls.numel(), gt_cls.numel(), rel.numel() // 3, int(n_rel)
    if (iw.numel() != F or det_off.numel() != F + 1 or gt_off.numel() != F + 1 or rel_off.numel() != F + 1 or det_box.numel() != 4 * ND
            or gt_box.numel() != 4 * NG or rel.numel() != 3 * NR or u.numel() != 10 * NR or n_rel < 0):
        raise ValueError("relation_targets: array sizes do not agree")
    rows = F * 64
    out = {"rel5": torch.empty((rows, 5), device=dev), "bounds": torch.empty((rows, 2, 4), device=dev, dtype=torch.int32),
           "labels": torch.empty((rows, n_rel), device=dev), "ixs": torch.empty((rows,), device=dev, dtype=torch.int64),
           "ixo": torch.empty((rows,), device=dev, dtype=torch.int64), "w": torch.empty((rows,), device=dev),
           "n_pairs": torch.empty((F,), device=dev, dtype=torch.int32), "n_dropped": torch.empty((F,), device=dev, dtype=torch.int32),
           "samp": torch.empty((NR, 10, 2), device=dev, dtype=torch.int32)}
    # the status word is part of the result: its own buffer (tag None), not the shared workspace the next op overwrites
    ws = _launch(dev, "relation_targets", lambda *tail: lib.i2v_relation_targets(
        ptr(det_off), ptr(det_box), ptr(det_cls), ptr(gt_off), ptr(gt_box), ptr(gt_cls), ptr(rel_off), ptr(rel), ptr(u), ptr(ih),
        ptr(iw), F, ND, NG, NR, n_rel, ptr(out["rel5"]), ptr(out["bounds"]), ptr(out["labels"]), ptr(out["ixs"]), ptr(out["ixo"]),
        ptr(out["w"]), ptr(out["n_pairs"]), ptr(out["n_dropped"]), ptr(out["samp"]), *tail),
        lib.i2v_relation_targets_workspace_bytes(F), None)
    if read_status and F > 0:
        _status(ws, 0, "relation_targets", "frame")
    out["status"] = ws[:4].view(torch.int32)[0]
    return out


def recognition_rows(cls_prob, rel_prob, ixs, ixo, L, device=None):
    """The per-frame tail of predicate recognition in one launch (include/i2vsgg_hip.h, i2v_recognition_rows;
    ``eval.recognition_rows_host`` is the numpy form).  cls_prob (B,C) fp32, rel_prob (P,R) fp32, ixs / ixo (P) int64, L
    (C-1,C-1,R) fp64.  Returns device tensors (sub (P,C), obj (P,C), pre (P,R) fp32, cls (B) int32)."""
    dev = _device(device, "eval.recognition_rows_host", cls_prob.device if torch.is_tensor(cls_prob) else "cuda")
    cls_prob, rel_prob = _stage(dev, torch.float32, cls_prob, rel_prob)
    ixs, ixo = _stage(dev, torch.int64, ixs, ixo)
    L = _to_dev(L, torch.float64, dev)
    if cls_prob.dim() != 2 or rel_prob.dim() != 2:
        raise ValueError("recognition_rows: cls_prob and rel_prob are matrices")
    (B, C), (P, R) = cls_prob.shape, rel_prob.shape
    if ixs.numel() != P or ixo.numel() != P or L.numel() != (C - 1) * (C - 1) * R:
        raise ValueError("recognition_rows: array sizes do not agree")
    sub = torch.zeros((P, C), device=dev)
    obj = torch.zeros((P, C), device=dev)
    pre = torch.zeros((P, R), device=dev)
    cls = torch.zeros((B,), device=dev, dtype=torch.int32)
    ws = _launch(dev, "recognition_rows", lambda *tail: lib.i2v_recognition_rows(
        ptr(cls_prob), ptr(rel_prob), ptr(ixs), ptr(ixo), ptr(L), B, P, C, R, ptr(sub), ptr(obj), ptr(pre), ptr(cls), *tail),
        lib.i2v_recognition_rows_workspace_bytes(P), "recognition_rows")
    if P > 0:
        _status(ws, 0, "recognition_rows", "pair")
    return sub, obj, pre, cls


def recognition_align(rows, seg_off, seg_row, inst, n_classes, n_rel, device=None):
    """Video-level alignment and accuracy@n of a packed batch of videos (include/i2vsgg_hip.h, i2v_recognition_align;
    ``recognition.pack`` builds the arrays).  rows (N, 2C+R) fp64, seg_off (S+1), seg_row (M), inst (T,4) int32.  Returns
    device tensors (mean (S,W) fp64, count (S) int32, top (S,3,10) int32, hit (T,7) int32, totals (8) int64, per_class
    (C,2,2) int64)."""
    dev = _device(device, "recognition.align_arrays_host")
    C, R = int(n_classes), int(n_rel)
    W = 2 * C + R
    rows = _to_dev(rows, torch.float64, dev)
    seg_off, seg_row, inst = _stage(dev, torch.int32, seg_off, seg_row, inst)
    S, M, T = seg_off.numel() - 1, seg_row.numel(), inst.numel() // 4
    if S < 0 or W <= 0 or rows.numel() % W or inst.numel() != 4 * T:
        raise ValueError("recognition_align: array sizes do not agree")
    N = rows.numel() // W
    mean = torch.zeros((S, W), device=dev, dtype=torch.float64)
    count = torch.zeros((S,), device=dev, dtype=torch.int32)
    top = torch.full((S, 3, 10), -1, device=dev, dtype=torch.int32)
    hit = torch.zeros((T, 7), device=dev, dtype=torch.int32)
    totals = torch.zeros((8,), device=dev, dtype=torch.int64)
    per_class = torch.zeros((max(C, 0), 2, 2), device=dev, dtype=torch.int64)
    ws = _launch(dev, "recognition_align", lambda *tail: lib.i2v_recognition_align(
        ptr(rows), ptr(seg_off), ptr(seg_row), ptr(inst), N, M, S, T, C, R, ptr(mean), ptr(count), ptr(top), ptr(hit), ptr(totals),
        ptr(per_class), *tail), lib.i2v_recognition_align_workspace_bytes(S, T), "recognition_align")
    _status(ws, 0, "recognition_align", "segment", "the row table is out of range at")
    _status(ws, 1, "recognition_align", "instance", "segment or labels out of range at")
    return mean, count, top, hit, totals, per_class


def image_relation_match(pred_off, gt_off, pred_trip, pred_box, gt_trip, gt_box, iou_threshold=0.5, device=None):
    """The greedy match of every image's ranked triplets against its annotated relations, one wave per (image, mode)
    (include/i2vsgg_hip.h, i2v_image_relation_match; ``image_relations.pack`` builds the arrays).  Arrays or tensors: pred_off,
    gt_off (I+1), pred_trip (n_pred,3), gt_trip (n_gt,3) int32; pred_box (n_pred,8), gt_box (n_gt,8) fp64.  Returns device
    tensors, mode 0 relation and 1 phrase: (hit (2,n_pred) int32, hit_ov (2,n_pred) fp64, gt_rank (2,n_gt) int32)."""
    dev = _device(device, "image_relations.match_host")
    max_gt = min(max(_max_rows(gt_off), 0), 4096)
    pred_off, gt_off, pred_trip, gt_trip = _stage(dev, torch.int32, pred_off, gt_off, pred_trip, gt_trip)
    pred_box, gt_box = _stage(dev, torch.float64, pred_box, gt_box)
    I, NP, NG = pred_off.numel() - 1, pred_trip.numel() // 3, gt_trip.numel() // 3
    if (I < 0 or gt_off.numel() != I + 1 or pred_trip.numel() != 3 * NP or gt_trip.numel() != 3 * NG or pred_box.numel() != 8 * NP
            or gt_box.numel() != 8 * NG):
        raise ValueError("image_relation_match: array sizes do not agree")
    hit = torch.full((2, NP), -1, device=dev, dtype=torch.int32)
    hit_ov = torch.full((2, NP), -1.0, device=dev, dtype=torch.float64)
    gt_rank = torch.full((2, NG), -1, device=dev, dtype=torch.int32)
    ws = _launch(dev, "image_relation_match", lambda *tail: lib.i2v_image_relation_match(
        ptr(pred_off), ptr(gt_off), ptr(pred_trip), ptr(pred_box), ptr(gt_trip), ptr(gt_box), I, NP, NG, max_gt, float(iou_threshold),
        ptr(hit), ptr(hit_ov), ptr(gt_rank), *tail), lib.i2v_image_relation_match_workspace_bytes(I), "image_relations")
    if I > 0:
        _status(ws, 0, "image_relation_match", "image")
    return hit, hit_ov, gt_rank


def image_relation_count(gt_rank, gt_trip, gt_zs, nreturns, n_rel, device=None):
    """The integer counters of recall@K from a match (include/i2vsgg_hip.h, i2v_image_relation_count).  gt_rank (2,n_gt),
    gt_trip (n_gt,3), gt_zs (n_gt) int32; ``nreturns``: 1 to 8 values of K.  Returns device tensors (totals (2,K,2),
    zs_totals (2,K,2), per_predicate (2,K,n_rel,2) int64): hits and ground truths per mode and K."""
    dev = _device(device, "image_relations.count_host")
    ks = np.ascontiguousarray(np.asarray(nreturns, np.int64).reshape(-1))
    n_rel = int(n_rel)
    if not 1 <= len(ks) <= 8 or (ks < 1).any() or (ks >= 2 ** 31).any():
        raise ValueError("image_relation_count: nreturns holds 1 to 8 positive values of K (got %r)" % (list(nreturns),))
    ks = ks.astype(np.int32)
    gt_rank, gt_trip, gt_zs = _stage(dev, torch.int32, gt_rank, gt_trip, gt_zs)
    NG, K = gt_zs.numel(), len(ks)
    if gt_rank.numel() != 2 * NG or gt_trip.numel() != 3 * NG or n_rel < 1:
        raise ValueError("image_relation_count: array sizes do not agree")
    totals = torch.zeros((2, K, 2), device=dev, dtype=torch.int64)
    zs_totals = torch.zeros((2, K, 2), device=dev, dtype=torch.int64)
    per_predicate = torch.zeros((2, K, n_rel, 2), device=dev, dtype=torch.int64)
    # the workspace it shares with the match: status word 1 is the count's
    ws = _launch(dev, "image_relation_count", lambda *tail: lib.i2v_image_relation_count(
        ptr(gt_rank), ptr(gt_trip), ptr(gt_zs), ks.ctypes.data, NG, n_rel, K, ptr(totals), ptr(zs_totals), ptr(per_predicate), *tail),
        lib.i2v_image_relation_match_workspace_bytes(0), "image_relations")
    _status(ws, 1, "image_relation_count", "ground truth", "the predicate of", " lies outside [0, %d)" % n_rel)
    return totals, zs_totals, per_predicate


def relation_feature_pool(feat, slot_off, mem_off, mem_slot, mem_idx, device=None):
    """The pooled feature of every video relation in one launch (include/i2vsgg_hip.h, i2v_relation_feature_pool;
    ``relation_features.pack`` builds the tables, ``relation_features.pool_arrays_host`` is the numpy form).  feat (n_rows, dim)
    fp32 (a device tensor is used where it lies), slot_off (S+1), mem_off (R+1), mem_slot (M), mem_idx (M) int32.  Returns
    device tensors (pooled (R, dim) fp32, count (R) int32); a non-zero status word raises."""
    dev = _device(device, "relation_features.pool_arrays_host", feat.device if torch.is_tensor(feat) and feat.is_cuda else "cuda")
    feat = _to_dev(feat, torch.float32, dev)
    if feat.dim() != 2 or feat.shape[1] < 1:
        raise ValueError("relation_feature_pool: feat is a matrix (n_rows, dim) with dim >= 1")
    slot_off, mem_off, mem_slot, mem_idx = (t.reshape(-1) for t in _stage(dev, torch.int32, slot_off, mem_off, mem_slot, mem_idx))
    N, D = feat.shape
    S, R, M = slot_off.numel() - 1, mem_off.numel() - 1, mem_slot.numel()
    if S < 0 or R < 0 or mem_idx.numel() != M:
        raise ValueError("relation_feature_pool: array sizes do not agree")
    pooled = torch.zeros((R, D), device=dev)
    count = torch.zeros((R,), device=dev, dtype=torch.int32)
    ws = _launch(dev, "relation_feature_pool", lambda *tail: lib.i2v_relation_feature_pool(
        ptr(feat), ptr(slot_off), ptr(mem_off), ptr(mem_slot), ptr(mem_idx), N, S, R, M, D, ptr(pooled), ptr(count), *tail),
        lib.i2v_relation_feature_pool_workspace_bytes(R), "relation_features")
    if R > 0:
        _status(ws, 0, "relation_feature_pool", "relation")
    return pooled, count


def det_eval_match(seg_det_off, seg_gt, gt_off, det_key, det_box, gt_box, gt_hard, ovthresh=0.5, device=None):
    """The VOC match of every detection against the ground truths of its class and image, one wave per (class, image)
    segment (include/i2vsgg_hip.h, i2v_det_eval_match; ``detection_eval.pack`` builds the arrays).  Arrays or tensors:
    seg_det_off (S+1), seg_gt (S), gt_off (slots+1), det_key (D), gt_hard (G) int32; det_box (D,4), gt_box (G,4) fp64.
    Returns device tensors at the detections' own positions: (flag (D) int32: 1 tp, 2 fp, 0 neither; ovmax (D) fp64;
    jmax (D) int32)."""
    dev = _device(device, "detection_eval.match_arrays_host")
    max_gt = _max_rows(gt_off)
    seg_det_off, seg_gt, gt_off, det_key, gt_hard = _stage(dev, torch.int32, seg_det_off, seg_gt, gt_off, det_key, gt_hard)
    det_box, gt_box = _stage(dev, torch.float64, det_box, gt_box)
    S, D, NS, G = seg_gt.numel(), det_key.numel(), gt_off.numel() - 1, gt_hard.numel()
    if seg_det_off.numel() != S + 1 or NS < 0 or det_box.numel() != 4 * D or gt_box.numel() != 4 * G:
        raise ValueError("det_eval_match: array sizes do not agree")
    flag = torch.full((D,), 2, device=dev, dtype=torch.int32)
    ovmax = torch.full((D,), float("-inf"), device=dev, dtype=torch.float64)
    jmax = torch.full((D,), -1, device=dev, dtype=torch.int32)
    ws = _launch(dev, "det_eval_match", lambda *tail: lib.i2v_det_eval_match(
        ptr(seg_det_off), ptr(seg_gt), ptr(gt_off), ptr(det_key), ptr(det_box), ptr(gt_box), ptr(gt_hard), S, D, NS, G, max_gt,
        float(ovthresh), ptr(flag), ptr(ovmax), ptr(jmax), *tail), lib.i2v_det_eval_match_workspace_bytes(D), "det_eval")
    if S > 0 and D > 0:
        _status(ws, 0, "det_eval_match", "segment")
    return flag, ovmax, jmax


def det_eval_curve(det_key, cls_off, flag, npos, device=None):
    """Per class: the stable score order, cumulative tp / fp, recall, precision and both VOC AP forms
    (include/i2vsgg_hip.h, i2v_det_eval_curve).  det_key (D), cls_off (C+1), flag (D), npos (C) int32.  Returns device
    tensors (perm, cum_tp, cum_fp (D) int32, rec, prec (D) fp64, ap_area, ap_11pt (C) fp64)."""
    dev = _device(device, "detection_eval.curve_arrays_host")
    det_key, cls_off, flag, npos = _stage(dev, torch.int32, det_key, cls_off, flag, npos)
    D, C = det_key.numel(), cls_off.numel() - 1
    if C < 0 or flag.numel() != D or npos.numel() != C:
        raise ValueError("det_eval_curve: array sizes do not agree")
    perm, cum_tp, cum_fp = (torch.zeros((D,), device=dev, dtype=torch.int32) for _ in range(3))
    rec, prec = (torch.zeros((D,), device=dev, dtype=torch.float64) for _ in range(2))
    ap_area, ap_11pt = (torch.zeros((C,), device=dev, dtype=torch.float64) for _ in range(2))
    ws = _launch(dev, "det_eval_curve", lambda *tail: lib.i2v_det_eval_curve(
        ptr(det_key), ptr(cls_off), ptr(flag), ptr(npos), C, D, ptr(perm), ptr(cum_tp), ptr(cum_fp), ptr(rec), ptr(prec), ptr(ap_area),
        ptr(ap_11pt), *tail), lib.i2v_det_eval_curve_workspace_bytes(D), "det_eval")
    if C > 0:
        _status(ws, 0, "det_eval_curve", "class")
    return perm, cum_tp, cum_fp, rec, prec, ap_area, ap_11pt


def proposal_cover(cand_off, cand_box, gt_off, gt_box, gt_area, limits, ranges, device=None, out=None):
    """The greedy cover of every (image, limit, area range) cell, one workgroup per cell (include/i2vsgg_hip.h,
    i2v_proposal_cover; ``proposal_eval.pack`` builds the arrays).  Arrays or tensors: cand_off, gt_off (I+1), limits (L) int32;
    cand_box (N,4), gt_box (G,4), gt_area (G), ranges (A,2) fp64.  Returns device tensors (ov (L,A,G) fp64, cand (L,A,G) int32,
    step (L,A,G) int32), -1 where a ground truth lies outside the range.  ``out``: three such tensors to write into instead
    (an image with malformed tables leaves its entries as they were)."""
    dev = _device(device, "proposal_eval.cover_arrays_host")
    if (np.asarray(torch.as_tensor(limits).cpu()).reshape(-1) < 1).any():
        raise ValueError("proposal_cover: every limit is >= 1 (2^31 - 1: no limit)")
    max_cand, max_gt = max(_max_rows(cand_off), 0), max(_max_rows(gt_off), 0)
    cand_off, gt_off, limits = (t.reshape(-1) for t in _stage(dev, torch.int32, cand_off, gt_off, limits))
    cand_box, gt_box, gt_area, ranges = _stage(dev, torch.float64, cand_box, gt_box, gt_area, ranges)
    I, N, G, L, A = cand_off.numel() - 1, cand_box.numel() // 4, gt_area.numel(), limits.numel(), ranges.numel() // 2
    if I < 0 or gt_off.numel() != I + 1 or cand_box.numel() != 4 * N or gt_box.numel() != 4 * G or ranges.numel() != 2 * A:
        raise ValueError("proposal_cover: array sizes do not agree")
    if not 1 <= L <= 8 or not 1 <= A <= 8:
        raise ValueError("proposal_cover: 1 to 8 limits and 1 to 8 area ranges (got %d and %d)" % (L, A))
    if out is None:
        ov = torch.full((L, A, G), -1.0, device=dev, dtype=torch.float64)
        cand = torch.full((L, A, G), -1, device=dev, dtype=torch.int32)
        step = torch.full((L, A, G), -1, device=dev, dtype=torch.int32)
    else:
        ov, cand, step = out
        for t, dt in ((ov, torch.float64), (cand, torch.int32), (step, torch.int32)):
            if t.device != dev or t.dtype != dt or tuple(t.shape) != (L, A, G) or not t.is_contiguous():
                raise ValueError("proposal_cover: out is (ov fp64, cand int32, step int32), each (%d, %d, %d) on %s" % (L, A, G, dev))
    # the caps are the kernel's to refuse, image by image (status word): what it sizes its LDS by stays inside them
    ws = _launch(dev, "proposal_cover", lambda *tail: lib.i2v_proposal_cover(
        ptr(cand_off), ptr(cand_box), ptr(gt_off), ptr(gt_box), ptr(gt_area), ptr(limits), ptr(ranges), I, N, G, L, A,
        min(max_gt, 4096), min(max_cand, 65535), ptr(ov), ptr(cand), ptr(step), *tail), lib.i2v_proposal_cover_workspace_bytes(I),
        "proposal_eval")
    if I > 0:
        _status(ws, 0, "proposal_cover", "image", "the offset tables are out of range or over a cap at")
    return ov, cand, step
