"""Video relation features: the second product of the reference's relation test loop, the hand-off to the video-level stage
(``save_semantic_embedding`` test_net_SGG_emb.py:147-149, the ``pre_feat`` saving :171-182, ``generate_static_relation_feat``
lib/utils.py:100-132).  One feature vector per video relation: the mean over the relation's member frames of the row of the
frame's ``pre_feat`` (the relation head's ``emb_dim`` feature per ordered pair) that the member's ``rel_idex`` names.  The
reference keeps one ``.npz`` per frame on disk and loads one per (relation, frame); here the rows stay on the device
(``FeatureArena``) and the pooling is one gather kernel (csrc/relation_features.hip, ``ops.relation_feature_pool``).

The rules, stated once for the host form (``pool_arrays_host``) and the kernel, which agree bit for bit:

* A *slot* is one frame ``(vid, fno)`` that had features of its own: its result in the relation loop is not the five Nones.  A
  slot owns ``n_pairs`` rows of ``dim`` float32; row ``k`` is ordered pair ``k``, the index ``ops.relation_topk`` returns as
  ``pair``, which is the ``rel_idex`` of every relation member.  A frame has no slot if it has fewer than two boxes, if
  ``video.fill_empty_frames`` filled it from a neighbour, or if it is missing from the run ("if the frame is filled with
  neighbor frames, then the npz is not saved").
* A relation with ``duration = [fstart, fend)`` and ``rel_idex`` of length ``fend - fstart`` has member ``j`` on frame number
  ``fstart + j``; any other length is a ``ValueError`` at packing.  For each member, in member order: no slot for the frame --
  the member is skipped (no error; ``j`` still advances, as in the reference); otherwise its row is
  ``slot_off[slot] + rel_idex[j]``.
* The pooled feature is, per column, the float32 sum of the valid rows in member order -- the sum starts from the first valid
  row's value, not from ``+0.0`` (a ``-0.0`` survives, as it does in numpy), one add per row -- then one float32 division by
  the number of valid rows.  This is ``np.array(rows).mean(axis=0)`` of lib/utils.py:126 bit for bit: numpy reduces axis 0 of a
  float32 matrix row by row in float32 -- for ``dim >= 2``; a single column is a contiguous vector to numpy, which it sums
  pairwise, and there the rule above stands, not numpy's order (``emb_dim`` is 300).  (The kernel divides in float64 and
  rounds once to float32: the same value, since 53 >= 2 * 24 + 2.)
* ``count[r]`` is the number of valid rows.  With ``count[r] == 0`` the row is all zeros; the reference writes NaN there, and
  ``write`` writes no file for such a relation and counts it -- the one stated deviation.
* Status: 0, or 1 + the largest index of a relation with an out-of-range table entry (``mem_off`` not monotone or past the
  member arrays, ``mem_slot`` below -1 or past the slots, a slot range that leaves the rows, ``mem_idx`` outside its slot).
  Such a relation comes out as count 0 and zeros, and nothing is read through its entries; its neighbours are unaffected.

What runs where.  Packing, the slot table and the files are host code (list logic on small data); the rows and the pooling are
on the device when a ``device`` is given.  With ``device=None`` the same rules run as numpy: the reference's two-step flow
from files (``from_files`` + ``pool_relation_features.py``) works on a machine without a GPU.
"""
import os

import numpy as np


class _Store(object):
    """Rows of every slot, one after another, and the host's table ``key -> (slot, n_pairs)``.  ``key`` is ``(vid, fno)`` for
    ``pack`` (``rekey`` maps a loop's own keys, e.g. frame paths, to it)."""

    def __init__(self, dim):
        self.dim = int(dim)
        self.table = {}
        self._off = [0]

    @property
    def slot_off(self):
        return np.asarray(self._off, np.int32)

    @property
    def n_rows(self):
        return self._off[-1]

    def _claim(self, key, n_pairs, dim):
        if key in self.table:
            raise ValueError("relation_features: frame %r has a slot already" % (key,))
        if dim != self.dim or n_pairs < 0:
            raise ValueError("relation_features: frame %r: rows of width %d, the store holds width %d" % (key, dim, self.dim))
        r0 = self._off[-1]
        self.table[key] = (len(self._off) - 1, int(n_pairs))
        self._off.append(r0 + int(n_pairs))
        return r0

    def rekey(self, index):
        """Rename the slots' keys through ``index`` (a dict or a callable: key -> (vid, fno))."""
        fn = index if callable(index) else index.__getitem__
        table = {}
        for key, v in self.table.items():
            vid, fno = fn(key)
            table[(str(vid), int(fno))] = v
        if len(table) != len(self.table):
            raise ValueError("relation_features: two frames share one (vid, fno)")
        self.table = table
        return self

    def rows_of(self, key):
        """The slot's rows as a float32 numpy array (n_pairs, dim)."""
        slot, n = self.table[key]
        r0 = self._off[slot]
        f = self.feat[r0:r0 + n]
        return f.detach().cpu().numpy() if hasattr(f, "detach") else np.array(f)


class HostStore(_Store):
    """The store on the host: ``feat`` is a float32 numpy array (what ``from_files`` returns)."""

    def __init__(self, dim):
        _Store.__init__(self, dim)
        self._parts = []
        self._feat = None

    def append(self, key, rows):
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2:
            raise ValueError("relation_features: frame %r: rows are (n_pairs, dim)" % (key,))
        self._claim(key, rows.shape[0], rows.shape[1])
        self._parts.append(rows)
        self._feat = None

    @property
    def feat(self):
        if self._feat is None:
            self._feat = np.concatenate(self._parts) if self._parts else np.zeros((0, self.dim), np.float32)
        return self._feat


class FeatureArena(_Store):
    """Device store of one run: a ``(total_rows, dim)`` float32 tensor filled by appending.  ``total_rows`` is known before the
    loop (``arena_rows``)."""

    def __init__(self, total_rows, dim, device):
        import torch
        _Store.__init__(self, dim)
        self.total_rows = int(total_rows)
        self.device = torch.device(device)
        self.feat = torch.zeros((self.total_rows, self.dim), device=self.device)

    def append(self, key, rows):
        """``rows``: a device tensor (n_pairs, dim) float32; copied device-to-device on the current stream."""
        if rows.dim() != 2 or not rows.is_cuda:
            raise ValueError("relation_features: frame %r: rows are a device tensor (n_pairs, dim)" % (key,))
        n = int(rows.shape[0])
        if self.n_rows + n > self.total_rows:
            raise ValueError("relation_features: frame %r: %d rows do not fit the arena (%d of %d used)"
                             % (key, n, self.n_rows, self.total_rows))
        r0 = self._claim(key, n, int(rows.shape[1]))
        self.feat[r0:r0 + n].copy_(rows, non_blocking=True)


def arena_rows(target_gt_rels, keys):
    """Rows the run's frames need: the sum over ``keys`` (frames, as ``target_gt_rels`` names them) of nb * (nb - 1) for nb >= 2
    annotated boxes (every ordered pair of a frame has one row)."""
    total = 0
    for k in keys:
        nb = len(target_gt_rels[k]["boxes"])
        if nb >= 2:
            total += nb * (nb - 1)
    return total


def arena_for(target_gt_rels, keys, dim, device, limit_mb=4096):
    """The arena of a run, refused with a clear message above ``limit_mb`` MiB."""
    rows = arena_rows(target_gt_rels, keys)
    need = rows * int(dim) * 4
    if need > float(limit_mb) * (1 << 20):
        raise SystemExit("relation features: %d pair rows of %d floats need %.1f MiB on the device, over --feat_arena_mb %g; raise "
                         "it, or run fewer frames at a time" % (rows, dim, need / float(1 << 20), limit_mb))
    return FeatureArena(rows, dim, device)


class ArenaSink(object):
    """What ``eval.keeping_relation_features`` takes: the arena of one run, made when the loop's network first shows up
    (``attach``) and sized from ALL the frames its ``target_gt_rels`` annotates -- the loop's own frame list is not known here, and
    the annotations of a run name its frames.  ``arena`` and ``net`` are None until then."""

    def __init__(self, device, limit_mb=4096):
        self.device, self.limit_mb, self.arena, self.net = device, limit_mb, None, None

    def attach(self, net):
        if self.arena is None:
            gt = net.vrd.target_gt_rels
            self.arena, self.net = arena_for(gt, list(gt), net.vrd.emb_dim, self.device, self.limit_mb), net
        elif net is not self.net:
            raise ValueError("relation_features: the sink holds the features of another network")
        return self.arena


def from_files(feat_dir):
    """The same store from ``<feat_dir>/<vid>/<fno>.npz`` files with key ``pre_feat`` (the reference's layout), on the host."""
    found = []
    for vid in sorted(os.listdir(feat_dir)):
        d = os.path.join(feat_dir, vid)
        if not os.path.isdir(d):
            continue
        for name in os.listdir(d):
            stem, ext = os.path.splitext(name)
            if ext == ".npz" and stem.lstrip("-").isdigit():
                found.append((vid, int(stem), os.path.join(d, name)))
    found.sort(key=lambda t: (t[0], t[1]))
    store = None
    for vid, fno, path in found:
        with np.load(path) as z:
            rows = np.asarray(z["pre_feat"], np.float32)
        rows = rows.reshape(rows.shape[0], -1) if rows.ndim != 2 else rows
        if store is None:
            store = HostStore(rows.shape[1])
        store.append((vid, fno), rows)
    if store is None:
        raise ValueError("relation_features.from_files: no <vid>/<fno>.npz under %s" % feat_dir)
    return store


def save_frame_feats(store, feat_dir):
    """``<feat_dir>/<vid>/<fno>.npz`` (``pre_feat``) per slot: what ``from_files`` reads.  The store's keys are (vid, fno)."""
    for (vid, fno) in store.table:
        d = os.path.join(feat_dir, str(vid))
        os.makedirs(d, exist_ok=True)
        np.savez(os.path.join(d, "%d.npz" % int(fno)), pre_feat=store.rows_of((vid, fno)))
    return len(store.table)


def pack(video_relations, slots):
    """``video_relations``: {vid: [{"duration": [fstart, fend), "rel_idex": [...], ...}, ...]} (``video.associate``);
    ``slots``: a store, or its table {(vid, fno): (slot, n_pairs)}.  -> (mem_off (R+1), mem_slot (M), mem_idx (M) int32,
    [(vid, pno), ...]): ``pno`` is the index in the video's list, as in the reference's file name."""
    table = slots.table if hasattr(slots, "table") else slots
    mem_off, mem_slot, mem_idx, ids = [0], [], [], []
    for vid, rels in video_relations.items():
        for pno, rel in enumerate(rels):
            fstart, fend = (int(x) for x in rel["duration"])
            idex = rel["rel_idex"]
            if fend < fstart or len(idex) != fend - fstart:
                raise ValueError("relation_features.pack: video %r relation %d: rel_idex has %d entries for the duration [%d, %d)"
                                 % (vid, pno, len(idex), fstart, fend))
            for j, k in enumerate(idex):
                slot = table.get((str(vid), fstart + j))
                mem_slot.append(-1 if slot is None else slot[0])
                mem_idx.append(int(k))
            mem_off.append(len(mem_slot))
            ids.append((vid, pno))
    if len(mem_slot) >= 2 ** 31:
        raise ValueError("relation_features.pack: more than 2^31 members")
    return (np.asarray(mem_off, np.int32), np.asarray(mem_slot, np.int32).reshape(-1), np.asarray(mem_idx, np.int64).clip(
        -2 ** 31, 2 ** 31 - 1).astype(np.int32).reshape(-1), ids)


def pool_arrays_host(feat, slot_off, mem_off, mem_slot, mem_idx):
    """The rules of ``ops.relation_feature_pool`` in numpy, on the same arrays: (pooled (R, dim) float32, count (R) int32,
    status)."""
    feat = np.asarray(feat, np.float32)
    slot_off, mem_off, mem_slot, mem_idx = (np.asarray(x, np.int64).reshape(-1) for x in (slot_off, mem_off, mem_slot, mem_idx))
    n_rows, dim = feat.shape
    S, R, M = len(slot_off) - 1, len(mem_off) - 1, len(mem_slot)
    pooled, count, status = np.zeros((R, dim), np.float32), np.zeros(R, np.int32), 0
    for r in range(R):
        m0, m1 = int(mem_off[r]), int(mem_off[r + 1])
        bad = m0 < 0 or m1 < m0 or m1 > M
        rows = np.zeros(0, np.int64)
        if not bad:
            s, k = mem_slot[m0:m1], mem_idx[m0:m1]
            bad = bool(((s < -1) | (s >= S)).any())
            if not bad:
                s, k = s[s >= 0], k[s >= 0]
                b, e = slot_off[s], slot_off[s + 1]
                bad = bool(((b < 0) | (e < b) | (e > n_rows) | (k < 0) | (k >= e - b)).any())
                rows = b + k
        if bad:
            status = max(status, r + 1)
            continue
        count[r] = len(rows)
        if len(rows):
            # a running sum is sequential by definition and starts from the first row (a reduce over a single column is a
            # contiguous vector to numpy, which it adds pairwise)
            pooled[r] = np.add.accumulate(feat[rows], axis=0, dtype=np.float32)[-1] / np.float32(len(rows))
    return pooled, count, status


def pool(video_relations, store, device=None):
    """-> {vid: [(pooled (dim,) float32, count), ...]} aligned with ``video_relations[vid]``.  ``store``: a ``FeatureArena`` or a
    ``HostStore`` whose keys are (vid, fno).  ``device``: the kernel on that GPU; None: the host form."""
    mem_off, mem_slot, mem_idx, ids = pack(video_relations, store)
    if device is None:
        feat = store.feat.detach().cpu().numpy() if hasattr(store.feat, "detach") else store.feat
        pooled, count, status = pool_arrays_host(feat, store.slot_off, mem_off, mem_slot, mem_idx)
        if status:
            raise ValueError("relation_features.pool: relation %d (video %r, #%d) has a rel_idex outside its frame's pairs"
                             % ((status - 1,) + tuple(ids[status - 1])))
    else:
        from . import ops
        p, c = ops.relation_feature_pool(store.feat, store.slot_off, mem_off, mem_slot, mem_idx, device=device)
        pooled, count = p.cpu().numpy(), c.cpu().numpy()
    out = dict((vid, []) for vid in video_relations)
    for r, (vid, _) in enumerate(ids):
        out[vid].append((pooled[r], int(count[r])))
    return out


def write(pooled, video_relations, save_path, names=None):
    """``<save_path>/<predicate>/<vid>_<pno>.npy`` per relation, as lib/utils.py:127-132 writes them.  The directory is
    ``triplet[1]`` as it stands in the relation (a name, or an id; with ``names``, the predicates' names, an id is looked up).
    Relations with count 0 are skipped.  -> (files written, relations skipped)."""
    written = skipped = 0
    for vid, rels in video_relations.items():
        for pno, rel in enumerate(rels):
            feat, count = pooled[vid][pno]
            if count == 0:
                skipped += 1
                continue
            pre = rel["triplet"][1]
            if names is not None and not isinstance(pre, str):
                pre = names[int(pre)]
            d = os.path.join(save_path, str(pre))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "%s_%d.npy" % (vid, pno)), np.asarray(feat, np.float32))
            written += 1
    return written, skipped


def report(video_relations, pooled, seconds):
    """The line the scripts print: relations, members, skipped members, count-0 relations and milliseconds."""
    n_rel = sum(len(r) for r in video_relations.values())
    members = sum(len(rel["rel_idex"]) for rels in video_relations.values() for rel in rels)
    valid = sum(c for rows in pooled.values() for _, c in rows)
    empty = sum(1 for rows in pooled.values() for _, c in rows if c == 0)
    return "relation features: %d relations, %d members, %d skipped (no frame features), %d relations without a frame, %.1f ms" % (
        n_rel, members, members - valid, empty, 1e3 * seconds)


def _prd_vecs(vrd):
    import torch
    dev = vrd.fc_rel.fc.weight.device
    return torch.from_numpy(np.asarray(vrd.prd_vecs, np.float32)).to(dev)


def semantic_embedding(vrd):
    """``prd_sem_embeddings(prd_vecs)``, un-normalised, as float32 numpy (n_rel, emb_dim): the array ``save_semantic_embedding``
    writes (resnet_SGG_emb.py:224-228)."""
    import torch
    with torch.no_grad():
        return vrd.prd_sem_embeddings(_prd_vecs(vrd)).float().cpu().numpy()


def classify(vrd, pooled):
    """The head's own last step (resnet_SGG_emb.py:208-219) on pooled features: softmax over the predicates of the cosine of
    each pooled vector and each semantic embedding, with the three ops of ``vrd.forward_device``.  ``pooled``: (R, emb_dim), array
    or tensor.  -> device tensor (R, n_rel)."""
    import torch
    import torch.nn.functional as F
    from . import ops
    with torch.no_grad():
        prd = _prd_vecs(vrd)
        x = torch.as_tensor(pooled).to(device=prd.device, dtype=torch.float32).contiguous()
        sem = ops.l2norm_rows(vrd.prd_sem_embeddings(prd))
        return F.softmax(ops.linear(ops.l2norm_rows(x), sem), dim=1)
