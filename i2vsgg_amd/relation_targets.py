"""Training targets of the relation head on DETECTED boxes: the ``rel_det`` task (faster_rcnn_SGG_emb.py:476-578).

The reference's branch does not run as shipped (it reads ``res['box']`` / ``res['cls']``, which are never set, calls ``vrd``
with the wrong arity and hands the loss an index list: SURVEY.md A9, A10), but what it means to compute is plain: match the
detections of a frame to its annotated boxes, let every annotated relation draw up to 10 (subject detection, object detection)
candidates without replacement with probability proportional to the product of the two overlaps, merge equal pairs into
multi-hot rows, build union boxes and dual masks.  The exact rules below are this project's own; the host form
(``relation_targets_host``) and the kernels (csrc/relation_targets.hip, ``ops.relation_targets``) both follow them.

Inputs, for a minibatch of F frames, as packed tables (``pack`` builds them): ``det_off`` (F+1), ``det_box`` (N_d, 4) float64
in network-input pixels, ``det_cls`` (N_d) int32; ``gt_off`` (F+1), ``gt_box`` (N_g, 4) float64 (the annotation times
``im_scale`` in float64), ``gt_cls`` (N_g) int32; ``rel_off`` (F+1), ``rel`` (N_r, 3) int32 -- subject box, object box (local
to the frame) and predicate; ``u`` (N_r, 10) uint32; ``ih``, ``iw`` (F) float64.

* Detections (``pack``, on the host).  The unscaled detections are filtered as :468-470 does: a box entirely outside the image
  (``x1 >= w or y1 >= h or x2 <= 0 or y2 <= 0``, with ``h = ih / scale``, ``w = iw / scale``) is dropped, the rest are clipped
  to ``[0, w] x [0, h]``; the kept boxes are multiplied by the scale.  A frame keeps at most ``CAP = 64`` detections: the 64
  best by score (equal scores: the lower row), left in row order -- lane a of the kernel is detection a, as in Seq-NMS.
* Match.  The overlap is float64 in the +1 convention of lib/model/nms/nms_cpu.py:14,26-31, in the operation order of
  ``packing.overlap_plus1``.  Detection a matches annotated box g when the classes are equal and ``overlap >= 0.5``.
* Candidates of the annotated relation (gs, go, r): every (a, b) with a matching gs, b matching go and a != b, a-major,
  ascending.  The integer weight of a candidate is ``floor((overlap(a, gs) * overlap(b, go)) * 65536.0)``: at least 16384,
  never 0, and within 2^-14 (relative) of the reference's weight.
* Draws.  ``K = min(10, number of candidates)``.  Draw k: ``total`` = the integer sum of the weights still alive;
  ``t = (uint64(u[rel, k]) * total) >> 32``; the first alive candidate, in candidate order, whose running integer sum exceeds
  t is drawn and leaves the alive set.  All integer (``total <= 64 * 63 * 65536 < 2^28``): any scan order gives the same pick,
  and no transcendental function or float sum takes part in a decision.  This is successive sampling, the distribution of the
  reference's ``np.random.choice(p=p, replace=False)`` up to the 2^-14 quantisation.  The uniforms are an input: the training
  loop draws one ``np.random.randint(0, 2**32, size=(N_r, 10), dtype=np.uint32)`` per minibatch from the global stream.
* Pairs.  The entries (relation in annotation order, draw in draw order) of a frame merge by (a, b) in first-seen order.  A
  pair's label row is the multi-hot of the predicates of all its entries (the target the pre_det branch builds at :234-235,
  not the index list of :544,:559).  Union box and 32 x 32 mask bounds are ``build_pair_tables``' float64 expressions on the
  two detection boxes.
* Capacity.  ``P = 64`` pair rows and ``B = 64`` box rows per frame, fixed shapes.  Unique pairs beyond P are dropped in
  first-seen order and counted in ``n_dropped``.  Padding rows: ``ixs = ixo = f * B``, a zero union box, zero bounds, zero
  labels, weight 0.
* Row weight.  ``w = float32(1.0 / (n_pairs[f] * F))``: ``ops.bce_rows(score, labels, w)`` is then the mean over the F frames
  of the per-frame BCE mean, a frame without a pair contributing the zero loss the reference returns for it (:489,:494,:516).
* Malformed tables.  Frame f is malformed when, in one of the three offset tables, ``0 <= off[f] <= off[f+1] <= size`` fails
  or an earlier entry lies above ``off[f]`` (so well-formed frames never share rows); when it has more than CAP detections;
  when ``ih`` / ``iw`` is not in (0, 1e9]; or when one of its relations names a box outside its annotated boxes or a predicate
  outside ``[0, n_rel)``.  Such a frame raises ``status`` to at least f + 1 and comes out as padding rows without draws.

Outputs: ``rel5`` (F*P, 5) float32 [frame, union box]; ``bounds`` (F*P, 2, 4) int32; ``labels`` (F*P, n_rel) float32;
``ixs`` / ``ixo`` (F*P) int64, rows of the padded (F*B, 5) box table; ``w`` (F*P) float32; ``n_pairs`` / ``n_dropped`` (F)
int32; ``samp`` (N_r, 10, 2) int32, -1 where there is no draw; ``status``.
"""
import numpy as np

from .packing import cat, overlap_plus1

CAP = 64                     # detections of one frame (csrc/relation_targets.hip RT_CAP)
P = 64                       # pair rows per frame
B = 64                       # box rows per frame
DRAWS = 10
MARGIN = 10
OUTPUTS = ("rel5", "bounds", "labels", "ixs", "ixo", "w", "n_pairs", "n_dropped", "samp")


class Packed(object):
    """The tables of one minibatch (module docstring), the padded box table ``boxes5`` (F*B, 5) float32 [frame, box] and, per
    frame, the rows of the frame's detections that were kept (``kept``)."""
    TABLES = ("det_off", "det_box", "det_cls", "gt_off", "gt_box", "gt_cls", "rel_off", "rel", "u", "ih", "iw")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_frames(self):
        return len(self.ih)

    def tables(self):
        return tuple(getattr(self, k) for k in self.TABLES)


def draw_uniforms(n_relations):
    """The minibatch's uniforms from numpy's global stream (the training script seeds it with cfg.RNG_SEED)."""
    return np.random.randint(0, 2 ** 32, size=(n_relations, DRAWS), dtype=np.uint32)


def pack(dets, annos, im_info, n_rel, u=None, names=None):
    """``dets[f]``: {"boxes" (unscaled pixels), "box_classes", "scores"} (what ``seqnms.to_annotations`` writes);
    ``annos[f]``: {"boxes", "box_classes", "rels"} (``source_gt_rels``); ``im_info`` (F, 3) = [ih, iw, scale].  ``u`` None:
    ``draw_uniforms``.  Malformed input is refused with a message that names the frame (``names[f]`` if given)."""
    info = np.asarray(im_info, np.float64).reshape(-1, 3)
    F = info.shape[0]
    if len(dets) != F or len(annos) != F:
        raise ValueError("relation_targets.pack: %d frames of detections, %d of annotations, %d rows of im_info" % (len(dets), len(annos), F))
    who = lambda f: "frame %d%s" % (f, " (%s)" % (names[f],) if names is not None else "")
    det_off, gt_off, rel_off = [0], [0], [0]
    det_box, det_cls, gt_box, gt_cls, rel, kept = [], [], [], [], [], []
    for f in range(F):
        ih, iw, sc = float(info[f, 0]), float(info[f, 1]), float(info[f, 2])
        if not (np.isfinite([ih, iw, sc]).all() and ih > 0 and iw > 0 and sc > 0):
            raise ValueError("relation_targets.pack: %s: im_info %r is not a positive finite size and scale" % (who(f), (ih, iw, sc)))
        d, an = dets[f], annos[f]
        try:
            db = np.asarray(d["boxes"], np.float64).reshape(-1, 4)
            gb = np.asarray(an["boxes"], np.float64).reshape(-1, 4)
            rl = np.asarray(an["rels"], np.int64).reshape(-1, 3)
        except (ValueError, TypeError) as e:
            raise ValueError("relation_targets.pack: %s: boxes are rows of 4, relations rows of 3 (%s)" % (who(f), e))
        dc, ds = np.asarray(d["box_classes"], np.int64).reshape(-1), np.asarray(d["scores"], np.float64).reshape(-1)
        gc = np.asarray(an["box_classes"], np.int64).reshape(-1)
        if len(dc) != len(db) or len(ds) != len(db):
            raise ValueError("relation_targets.pack: %s: %d detected boxes, %d classes, %d scores" % (who(f), len(db), len(dc), len(ds)))
        if len(gc) != len(gb):
            raise ValueError("relation_targets.pack: %s: %d annotated boxes, %d classes" % (who(f), len(gb), len(gc)))
        if not (np.isfinite(db).all() and np.isfinite(ds).all() and np.isfinite(gb).all()):
            raise ValueError("relation_targets.pack: %s holds a box or score that is not finite" % who(f))
        if len(rl) and (rl[:, :2].min() < 0 or rl[:, :2].max() >= len(gb)):
            raise ValueError("relation_targets.pack: %s: a relation names a box outside its %d annotated boxes" % (who(f), len(gb)))
        if len(rl) and (rl[:, 2].min() < 0 or rl[:, 2].max() >= n_rel):
            raise ValueError("relation_targets.pack: %s: a predicate outside [0, %d)" % (who(f), n_rel))
        h, w = ih / sc, iw / sc                                                    # :465
        keep = np.nonzero(~((db[:, 0] >= w) | (db[:, 1] >= h) | (db[:, 2] <= 0) | (db[:, 3] <= 0)))[0]      # :468
        if len(keep) > CAP:
            keep = np.sort(keep[np.argsort(-ds[keep], kind="stable")[:CAP]])
        k = db[keep]
        k = np.stack([np.maximum(0, k[:, 0]), np.maximum(0, k[:, 1]), np.minimum(w, k[:, 2]), np.minimum(h, k[:, 3])], 1) * sc
        det_box.append(k); det_cls.append(dc[keep]); kept.append(keep)
        gt_box.append(gb * sc); gt_cls.append(gc); rel.append(rl)
        det_off.append(det_off[-1] + len(keep)); gt_off.append(gt_off[-1] + len(gb)); rel_off.append(rel_off[-1] + len(rl))
    n_r = rel_off[-1]
    if u is None:
        u = draw_uniforms(n_r)
    u = np.ascontiguousarray(u, np.uint32)
    if u.shape != (n_r, DRAWS):
        raise ValueError("relation_targets.pack: u is %r, the minibatch has %d relations: (%d, %d) wanted" % (u.shape, n_r, n_r, DRAWS))
    pk = Packed(det_off=np.asarray(det_off, np.int32), det_box=cat(det_box, (4,), np.float64), det_cls=cat(det_cls, (), np.int32),
                gt_off=np.asarray(gt_off, np.int32), gt_box=cat(gt_box, (4,), np.float64), gt_cls=cat(gt_cls, (), np.int32),
                rel_off=np.asarray(rel_off, np.int32), rel=cat(rel, (3,), np.int32), u=u,
                ih=np.ascontiguousarray(info[:, 0]), iw=np.ascontiguousarray(info[:, 1]), kept=kept)
    pk.boxes5 = box_table(pk)
    return pk


def box_table(pk):
    """The padded (F*B, 5) float32 box table [frame, box]: row f*B + a is detection a of frame f, the rest zero boxes."""
    F = pk.n_frames
    out = np.zeros((F * B, 5), np.float32)
    out[:, 0] = np.repeat(np.arange(F), B)
    for f in range(F):
        d0, d1 = int(pk.det_off[f]), int(pk.det_off[f + 1])
        if 0 <= d0 <= d1 <= len(pk.det_box) and d1 - d0 <= B:
            out[f * B:f * B + d1 - d0, 1:] = pk.det_box[d0:d1]
    return out


def _frame_ok(f, det_off, n_d, gt_off, n_g, rel_off, n_r, rel, ih, iw, n_rel):
    for off, size in ((det_off, n_d), (gt_off, n_g), (rel_off, n_r)):
        a, b = int(off[f]), int(off[f + 1])
        if a < 0 or b < a or b > size or (f and int(np.max(off[:f])) > a):
            return False
    if int(det_off[f + 1]) - int(det_off[f]) > CAP:
        return False
    if not (0.0 < ih[f] <= 1.0e9 and 0.0 < iw[f] <= 1.0e9):
        return False
    r = rel[int(rel_off[f]):int(rel_off[f + 1])]
    n = int(gt_off[f + 1]) - int(gt_off[f])
    return not len(r) or bool(r[:, :2].min() >= 0 and r[:, :2].max() < n and r[:, 2].min() >= 0 and r[:, 2].max() < n_rel)


def _mask_bounds(bb, ih, iw):
    rh, rw = 32.0 / ih, 32.0 / iw                        # _getDualMask (resnet_SGG_emb.py:246-256), as build_pair_tables
    return np.stack([np.maximum(0, np.floor(bb[:, 0] * rw)), np.maximum(0, np.floor(bb[:, 1] * rh)),
                     np.minimum(32, np.ceil(bb[:, 2] * rw)), np.minimum(32, np.ceil(bb[:, 3] * rh))], 1)


def draw(weights, u_row, K):
    """The draws of one relation: ``weights`` (int64, in candidate order, 0 where there is no candidate), the relation's
    uniforms, K draws -> the drawn candidates in draw order."""
    wt, picks = np.array(weights, np.int64), []
    for k in range(K):
        cs = np.cumsum(wt)
        t = (int(u_row[k]) * int(cs[-1])) >> 32
        c = int(np.searchsorted(cs, t, side="right"))    # the first running sum above t: an alive candidate
        wt[c] = 0
        picks.append(c)
    return picks


def relation_targets_host(det_off, det_box, det_cls, gt_off, gt_box, gt_cls, rel_off, rel, u, ih, iw, n_rel):
    """The rules of the module docstring in numpy (vectorised per relation) on the packed tables -> a dict of the outputs
    (numpy arrays) plus ``status``."""
    det_off, gt_off, rel_off = (np.asarray(x, np.int64).reshape(-1) for x in (det_off, gt_off, rel_off))
    det_box, gt_box = np.asarray(det_box, np.float64).reshape(-1, 4), np.asarray(gt_box, np.float64).reshape(-1, 4)
    det_cls, gt_cls = np.asarray(det_cls, np.int64).reshape(-1), np.asarray(gt_cls, np.int64).reshape(-1)
    rel, u = np.asarray(rel, np.int64).reshape(-1, 3), np.asarray(u, np.uint32).reshape(-1, DRAWS)
    ih, iw = np.asarray(ih, np.float64).reshape(-1), np.asarray(iw, np.float64).reshape(-1)
    F, n_r = len(ih), len(rel)
    out = {"rel5": np.zeros((F * P, 5), np.float32), "bounds": np.zeros((F * P, 2, 4), np.int32),
           "labels": np.zeros((F * P, n_rel), np.float32), "ixs": np.repeat(np.arange(F, dtype=np.int64) * B, P),
           "w": np.zeros(F * P, np.float32), "n_pairs": np.zeros(F, np.int32), "n_dropped": np.zeros(F, np.int32),
           "samp": np.full((n_r, DRAWS, 2), -1, np.int32), "status": 0}
    out["ixo"] = out["ixs"].copy()
    out["rel5"][:, 0] = np.repeat(np.arange(F), P)
    for f in range(F):
        if not _frame_ok(f, det_off, len(det_box), gt_off, len(gt_box), rel_off, n_r, rel, ih, iw, n_rel):
            out["status"] = f + 1                        # the largest malformed frame + 1
            continue
        d0, d1, g0, g1 = int(det_off[f]), int(det_off[f + 1]), int(gt_off[f]), int(gt_off[f + 1])
        db = det_box[d0:d1]
        if d1 == d0 or g1 == g0:
            continue
        ov = overlap_plus1(db, gt_box[g0:g1])
        match = (det_cls[d0:d1, None] == gt_cls[None, g0:g1]) & (ov >= 0.5)
        index, labels = {}, []
        for r in range(int(rel_off[f]), int(rel_off[f + 1])):
            gs, go, pr = (int(v) for v in rel[r])
            A, Bc = np.nonzero(match[:, gs])[0], np.nonzero(match[:, go])[0]
            if not len(A) or not len(Bc):
                continue
            wt = np.floor((ov[A, gs][:, None] * ov[Bc, go][None, :]) * 65536.0).astype(np.int64)
            wt = np.where(A[:, None] != Bc[None, :], wt, 0).reshape(-1)          # a == b is no candidate
            for k, c in enumerate(draw(wt, u[r], min(DRAWS, int(np.count_nonzero(wt))))):
                a, b = int(A[c // len(Bc)]), int(Bc[c % len(Bc)])
                out["samp"][r, k] = (a, b)
                if (a, b) not in index:
                    index[(a, b)] = len(labels)
                    labels.append(np.zeros(n_rel, np.float32))
                labels[index[(a, b)]][pr] = 1
        n_unique = len(index)
        n = min(n_unique, P)
        out["n_pairs"][f], out["n_dropped"][f] = n, n_unique - n
        if n == 0:
            continue
        pairs = np.asarray(list(index)[:n], np.int64)
        sb, ob = db[pairs[:, 0]], db[pairs[:, 1]]
        union = np.stack([np.maximum(0, np.minimum(sb[:, 0], ob[:, 0]) - MARGIN), np.maximum(0, np.minimum(sb[:, 1], ob[:, 1]) - MARGIN),
                          np.minimum(iw[f], np.maximum(sb[:, 2], ob[:, 2]) + MARGIN),
                          np.minimum(ih[f], np.maximum(sb[:, 3], ob[:, 3]) + MARGIN)], 1)
        rows = slice(f * P, f * P + n)
        out["rel5"][rows, 1:] = union
        out["bounds"][rows] = np.stack([_mask_bounds(sb, ih[f], iw[f]), _mask_bounds(ob, ih[f], iw[f])], 1).astype(np.int32)
        out["labels"][rows] = np.stack(labels[:n])
        out["ixs"][rows], out["ixo"][rows] = f * B + pairs[:, 0], f * B + pairs[:, 1]
        out["w"][rows] = np.float32(1.0 / (n * F))
    return out


def relation_targets(pk, n_rel, device=None):
    """``relation_targets_host`` on a ``Packed`` (``device=None``) or the kernels, as a dict of numpy arrays plus ``status``."""
    if device is None:
        return relation_targets_host(*pk.tables(), n_rel=n_rel)
    from . import ops
    res = ops.relation_targets(*pk.tables(), n_rel=n_rel, device=device, read_status=False)
    return {k: (int(v.item()) if k == "status" else v.cpu().numpy()) for k, v in res.items()}
