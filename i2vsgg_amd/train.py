"""Training steps of the two reference loops, as reusable objects.

``SGGEmbStep``      one step of trainval_net_SGG_emb.py:189-255 (pre_det): backbone forward (no grad,
                    the reference detaches it), relation head forward + backward, SGD(momentum) update
                    of the ``vrd.*`` parameters with the reference's param groups (:129-150).
``InstanceStyleDStep`` one D+G adversarial step of trainval_net_instance_styleD_bilinear.py:262-341.

Both keep their inputs resident on the device, can be captured into a HIP graph (the step is launch
bound otherwise: ~300 small kernels), and all-reduce gradients over RCCL when world_size > 1.
The capture machinery they share is ``graphs.CapturedStep``; the optimizers (optim.py), the staging helpers (staging.py)
and ``replay_graph`` are imported here under the names callers have always used (``train.FusedSGD``, ...).
"""
import numpy as np
import torch

from . import _lib, launch, ops, parallel
from . import synthetic as syn
from .graphs import CapturedStep, replay_graph, _REPLAY_STREAMS                                   # noqa: F401
from .model.utils.config import cfg
from .optim import FusedSGD, FusedAdam, make_optimizer, _same_memory_order                       # noqa: F401
from .staging import (_Slot, _place_u8, parse_u8_meta, place_frames, step_uploader, synthetic_sgg_batch,      # noqa: F401
                      sgg_head_inputs, _rasterize_host)


class _FrameSet:
    """What the backbone half of the SGG_emb step owns for ONE minibatch size (n, H, W): the staged frames, one launch
    context per frame branch and the captured graph of the step whose backbone half has this size."""

    def __init__(self, key, device, n_ctx, arena):
        n, h, w = key
        self.key = key
        self.im = torch.zeros((n, 4, h, w), device=device).contiguous(memory_format=torch.channels_last)
        self.ctx = [launch.LaunchContext(device, arena=arena) for _ in range(n_ctx)]
        self.fh = self.fw = None      # extent of the C4 map, known after the first pass
        self.graph = None             # None: not captured yet; False: capture failed (eager launches for this size)
        self.fitted = False
        self.tick = 0
        # stage-split schedule (round 6): this size as the FRONT half's (stem .. layer3[:cut]) and as the BACK half's
        # (layer3[cut:]) input; a graph is captured per (front size, back size) pair -- the back half of a call works on the
        # previous minibatch, whose size may differ
        self.ctx_front = launch.LaunchContext(device, arena=arena)
        self.ctx_back = launch.LaunchContext(device, arena=arena)
        self.fitted_front = self.fitted_back = False
        self.graphs = {}              # back size key -> graph (or False)

    def drop_graphs(self):
        self.graph = None
        self.graphs.clear()


class _StagePipeline:
    """Host-side twin of the three head-input slots of the stage-split schedule (in -> mid -> cur): which minibatch each holds and
    which one the head trained last.  No device state: ``tests/test_host_logic.py`` drives it on the CPU.

    A minibatch reaches the head two calls after it was staged.  ``prime()`` fills every slot with the minibatch staged first, so a
    resident minibatch is trained by every call; once a NEWER minibatch waits behind one the head has already trained, the next
    call runs no head (``bubble``) -- in a loop that stages before every call that is exactly its second call."""

    def __init__(self):
        self.inp = self.mid = self.cur = 0
        self.last_trained = -1

    def staged(self):
        self.inp += 1

    def prime(self):
        self.mid = self.cur = self.inp
        self.last_trained = -1

    @property
    def bubble(self):
        return self.cur <= self.last_trained and max(self.mid, self.inp) > self.cur

    def call(self):
        """One call of the step: -> the minibatch its head trains, or None for a bubble; the slots advance."""
        head = None if self.bubble else self.cur
        if head is not None:
            self.last_trained = head
        self.cur, self.mid = self.mid, self.inp
        return head


class SGGEmbStep(CapturedStep):
    """One step of trainval_net_SGG_emb.py:189-255 (pre_det) as a replayable object.

    A step = one backbone pass (no grad: the reference detaches the feature map, faster_rcnn_SGG_emb.py:148), one
    relation-head forward + backward, one gradient exchange (world > 1), one SGD(momentum) update of ``vrd.*``.

    Schedule (``overlap``, the default with HIP graphs): the backbone is frozen in this loop, so the backbone pass of
    the NEXT minibatch does not depend on this step's update.  The whole step is ONE captured graph with branches
    between a fork and a join: [head fwd + bwd (+ exchange) + SGD of batch k] beside [backbone of batch k+1, one branch per
    frame].  The branches own disjoint device state (``launch.LaunchContext``: zero arena, split-K workspace, scratch) and
    meet only at graph edges: the feature-map hand-off (one copy before the fork) and the join.  There is one graph launch
    per step on the caller's stream, no side stream, no event and no priority for a caller to get wrong.

    Round 6 (``bb_split="stage"``, the default): the backbone half is cut by STAGE, not by frame -- [head of batch k-2] beside
    [stem .. layer3[:cut] of batch k, all frames] beside [layer3[cut:] of batch k-1, all frames]; a minibatch reaches the head two
    calls after its ``stage()`` (``lag`` 2, three slots in -> mid -> cur; ``bubble`` / ``run_staged`` for loops).  The paragraphs
    below describe the one-call pipeline of ``bb_split="frame"`` / ``"none"``; the stage form differs only in the extra slot.

    Minibatches move through a two-slot pipeline so that ``stage()`` may be called at any time between steps:
    ``stage(b)`` writes the frames of b (read by the NEXT call's backbone branches) and its head inputs into the ``in``
    slot; a call runs head(``cur``) beside backbone(frames) and ends with cur <- in (one small copy inside the graph, behind
    the head).  A batch staged before call k is therefore consumed by the backbone in call k and by the head in call k+1 --
    features and boxes / labels of one batch always meet.  ``overlap=False`` (and eager mode): backbone and head of the
    staged batch in the same call.

    Minibatches of a data loader differ in size (the loader pads every batch to its own aspect ratio,
    roibatchLoader.py:162-190) and in the number of boxes and pairs per frame.  The captured step takes them all:
      * the head half is size-free: boxes / pairs are zero-padded to a CAPACITY (``n_boxes`` / ``n_pairs`` per frame; pad
        rows carry loss weight 0, so their gradient is exactly zero), the feature maps sit packed at the start of a
        capacity buffer and the ROI op reads their extent from device memory (``ops.PackedMaps``; the extent travels
        through the slots with the batch);
      * the backbone half is captured once per frame size: ``shapes[(n, H, W)]`` holds the staged frames, the per-frame
        launch contexts (arenas sized for that size) and the graph [rotate, hand-off, fork, head | backbone(n, H, W), join];
        a call replays the graph of the size staged last.  At most ``max_graphs`` graphs are kept (least recently used
        goes first); they share one memory pool, since no two of them ever run at the same time.
    """

    def __init__(self, net, n_frames, vrd_lr=1e-4, seed=1, device="cuda:0", h=600, w=1000, n_boxes=32, n_pairs=32,
                 use_graph=True, fuse_sgd=True, zero_arena=True, overlap=None, max_graphs=16, trace_rows=0, stage_synthetic=True,
                 optimizer="sgd", bb_split=None):
        import os
        self.net, self.dev, self.n_frames = net, torch.device(device), n_frames
        if not (net.vrd.use_obj_visual and net.vrd.spatial_type == 2):
            raise ValueError("SGGEmbStep packs the inputs of the reference's default relation head (use_obj_visual=True, "
                             "spatial_type=2: what every reference script runs); the other vrd variants run through "
                             "vrd.forward / forward_device")
        self.world = parallel.world_size()
        self.geom = (h, w, n_boxes, n_pairs)
        # data parallelism for everything except vrd.fc6, which is cut by output columns (parallel.py): its 822 MB
        # gradient -- 91 % of the exchange -- stays local and its SGD update stays fused into the wgrad epilogue
        self.tp = parallel.exchange_enabled() and os.environ.get("I2V_TP_FC6", "1") != "0" and \
            net.vrd.fc6.fc.weight.shape[0] % max(self.world, 1) == 0
        if self.tp and net.vrd.tp is None:
            net.vrd.enable_fc6_tp(parallel.rank(), self.world)
        self.opt = make_optimizer(optimizer, [(n, p) for n, p in net.named_parameters() if n.startswith("vrd.")], vrd_lr)
        self.fused = self.opt.fuse_wgrad() if fuse_sgd else []
        self.loss = torch.zeros((), device=self.dev)
        self._seed = torch.full((), 1.0 / max(self.world, 1), device=self.dev)
        self.graph_error = None
        self.use_graph = use_graph
        if overlap is None:
            overlap = os.environ.get("I2V_OVERLAP", "1") != "0"
        self.overlap = bool(overlap) and use_graph       # the schedule asked for; in force once capture() has succeeded
        self._pipelined = False                          # (until then a call is the sequential eager step)
        self._graphs_on = False
        self.zero_arena = zero_arena
        # How the backbone half is cut into graph branches beside the head (I2V_BB_SPLIT / ``bb_split``):
        #   "stage" (default, round 6): by STAGE -- [stem .. layer3[:cut] of batch k+2] and [layer3[cut:] of batch k+1], every
        #           kernel over ALL frames of its minibatch; a batch reaches the head two calls after it was staged (``lag`` 2);
        #   "frame" (rounds 2-5): one branch per frame of batch k+1 (``lag`` 1);
        #   "none": one branch for the whole backbone of batch k+1.
        mode = bb_split if bb_split is not None else os.environ.get("I2V_BB_SPLIT", "stage")
        mode = {"1": "frame", "0": "none", "2": "stage"}.get(str(mode), str(mode))
        if mode not in ("stage", "frame", "none"):
            raise ValueError("SGGEmbStep: bb_split must be 'stage', 'frame' or 'none', got %r" % (mode,))
        self.stage_split = mode == "stage" and use_graph
        self.bb_split = mode == "frame" and use_graph and n_frames > 1
        # blocks of layer3 in the front half: 6-7 of ResNet-101's 23 balance the chains (tools/stage_split_probe.py); never more
        # than a third of the stage (ResNet-50 has 6)
        n3 = len(net.RCNN_base[6])
        self.cut = max(1, min(int(os.environ.get("I2V_STAGE_CUT", "6")), max(n3 // 3, 1), n3 - 1))
        self._frame_streams = [launch.role_stream(self.dev, ("frame", f)) for f in range(max(n_frames, 2))] \
            if (self.bb_split or self.stage_split) else []
        # host-side twins of the three head-input slots (which minibatch each holds) and of what the head has trained: with
        # the backbone cut by stage a batch reaches the head two calls after its stage(); in a loop that stages a new batch
        # before every call the second call would find the FIRST batch in ``cur`` again -- that call runs no head (``bubble``)
        self._pipe, self.n_bubbles = _StagePipeline(), 0
        self._mid_key = None          # key of the frame set whose front-half output ``mid_next`` holds
        self.mid_next_flat = self.mid_cur_flat = None
        self.mid_slot = None
        self._side = None
        self.ctx_head = launch.LaunchContext(self.dev, arena=zero_arena, ordered=True)      # head branch: bit-reproducible sums
        self.ctx_bb = launch.LaunchContext(self.dev, arena=zero_arena)        # eager backbone passes (any size)
        self.shapes, self.max_graphs, self._tick, self._pool = {}, int(max_graphs), 0, None
        self.cap_boxes, self.cap_pairs = n_frames * n_boxes, n_frames * n_pairs      # rows of the padded head inputs
        self.cap_cells = 0
        self.fmap_flat = self.fmap_head_flat = None
        self.cur = self.inp = None    # head inputs: ``inp`` is written by stage(), ``cur`` read by the head
        self._staged = None           # key of the frame set staged last
        self._fmap_key = None         # key of the frame set whose features ``fmap_flat`` holds
        self.primed = False
        self.trace = torch.zeros((trace_rows, len(self.TRACE_COLS)), device=self.dev, dtype=torch.float64) if trace_rows else None
        self._trace_i = torch.zeros((1,), device=self.dev, dtype=torch.long)
        if stage_synthetic:           # a loop fed by a data loader stages its own first minibatch (``stage_batch``)
            self.reseed(seed)

    @property
    def lag(self):
        """How many calls after its ``stage()`` a minibatch reaches the head: 0 sequential, 1 overlapped with the backbone cut by
        frame (or not at all), 2 with the backbone cut by stage.  After ``capture()`` the first ``lag - 1`` calls run no head
        (``bubble``: the pipeline fills); a loop ends with ``lag`` calls without a new ``stage()`` (``flush``)."""
        return (2 if self.stage_split else 1) if self._pipelined else 0

    @property
    def bubble(self):
        """True when the NEXT call will run no head (backbone cut by stage): the head's slot holds a minibatch it has already
        trained while a newer one waits behind it in the pipeline -- the call advances the backbone halves only and its return
        value is stale (``n_bubbles`` counts them).  In a loop that stages before every call that is the second call; a resident
        minibatch (nothing newer staged) is trained by every call."""
        return bool(self._pipelined and self.stage_split and self._pipe.bubble)

    # ------------------------------------------------------------------ compatibility views
    @property
    def graph(self):
        """The captured graph of the frame size staged last (None when that size runs on eager launches)."""
        fs = self.shapes.get(self._staged)
        return (fs.graph or None) if fs is not None else None

    @property
    def im(self):
        return self.shapes[self._staged].im

    @property
    def fmap(self):
        """Feature maps of the last backbone pass as a (n,1024,h,w) channels_last view."""
        fs = self.shapes[self._fmap_key]
        n, c = fs.key[0], self._channels
        return self.fmap_flat[:n * fs.fh * fs.fw * c].view(n, fs.fh, fs.fw, c).permute(0, 3, 1, 2)

    # ------------------------------------------------------------------ data side
    def _layout(self, nb, npair):
        f32, i64 = torch.float32, torch.long
        # boxes and union boxes in ONE roi table (the head pools them in one pass), subject and object indices in one index
        # vector: what the head would otherwise concatenate every step
        return {"rois": ((nb + npair, 5), f32), "labels": ((npair, self.net.vrd.n_rel), f32), "ix12": ((2 * npair,), i64),
                "masks": ((npair, 4, 32, 32), f32), "wrow": ((npair,), f32), "extent": ((2,), torch.int32)}

    def _synthetic(self, seed):
        """frames in the layout the device front-end emits (ops.image_prep: NHWC with the stem's
        zero fourth channel) + the host-side head inputs of faster_rcnn_SGG_emb.py:170-245."""
        h, w, n_boxes, n_pairs = self.geom
        head = self.net.vrd
        im, info, annos = synthetic_sgg_batch(seed, self.n_frames, n_boxes, n_pairs, head.n_rel, head.n_obj, h, w)
        head.source_gt_rels = annos
        self.paths = sorted(annos, key=lambda s: int(s[1:]))
        fields = sgg_head_inputs([annos[p] for p in self.paths], info, head.n_rel)
        im4 = torch.zeros((im.shape[0], 4) + tuple(im.shape[2:]), device=self.dev).contiguous(memory_format=torch.channels_last)
        im4[:, :3] = torch.from_numpy(im).to(self.dev)
        return im4, info, fields

    def _frames(self, key):
        fs = self.shapes.get(key)
        if fs is None:
            fs = self.shapes[key] = _FrameSet(key, self.dev, key[0] if self.bb_split else 1, self.zero_arena)
        self._tick += 1
        fs.tick = self._tick
        return fs

    def _geom_dev(self, fs):
        if getattr(fs, "_geom", None) is None:
            fs._geom = torch.tensor([fs.fh, fs.fw], dtype=torch.int32, device=self.dev)
        return fs._geom

    def _grow(self, nb, npair):
        """Padded head inputs too small for this batch: new capacity (multiples of 16 rows), every graph is stale."""
        if self.tp:
            raise ValueError("SGGEmbStep: %d boxes / %d pairs exceed the capacity %d / %d; with fc6 cut across the ranks every "
                             "rank must hold the same number of rows -- construct the step with larger n_boxes / n_pairs"
                             % (nb, npair, self.cap_boxes, self.cap_pairs))
        up = lambda n, cap: max(cap, (n + 15) // 16 * 16)
        self.cap_boxes, self.cap_pairs = up(nb, self.cap_boxes), up(npair, self.cap_pairs)
        self.invalidate_graphs()

    def stage(self, frames, info, fields, size=None):
        """Hand the NEXT minibatch to the step.  ``frames``: (n,4,H,W) channels_last device tensor (the device front-end's
        blob), or (n,3,H,W) float frames on the device or the host (a roibatchLoader batch; pinned host memory crosses
        asynchronously), or -- with ``size`` = (n, H, W) -- a callable that writes the frames into the frame set it is given
        (``stage_batch_u8``).  ``info``: (n,3) im_info rows.  ``fields``: ``sgg_head_inputs`` of the batch.  Ordered on the
        caller's stream like everything else: it may be called right after ``__call__`` returns, the copies queue behind
        the step that is still running."""
        if fields is None:
            raise ValueError("SGGEmbStep.stage: a minibatch without an annotated relation (the reference loop skips it, "
                             "faster_rcnn_SGG_emb.py:177-183)")
        placer = None
        if callable(frames):
            if size is None:
                raise ValueError("SGGEmbStep.stage: a frame-writing callable needs size=(n, H, W)")
            placer = frames
            n, H, W = size
        else:
            n, _, H, W = frames.shape
        if int(n) != self.n_frames:
            raise ValueError("SGGEmbStep.stage: %d frames, the step was built for %d" % (n, self.n_frames))
        key = (int(n), int(H), int(W))
        fs = self._frames(key)
        if placer is not None:
            placer(fs)
        else:
            place_frames(fs.im, frames, self)
        self.info = np.asarray(info, np.float32).reshape(-1, 3) if not torch.is_tensor(info) else info.detach().cpu().numpy().reshape(-1, 3)
        nb, npair = fields["boxes"].shape[0], fields["relb"].shape[0]
        self.n_rows = nb + npair
        host_masks = _rasterize_host(fields["bounds"])
        if not self.use_graph:
            # eager launches: exact sizes, nothing is padded
            lay = self._layout(nb, npair)
            if self.inp is None or not self.inp.same_layout(lay):
                self.cur = _Slot(lay, self.dev)
                self.mid_slot = _Slot(lay, self.dev)
                self.inp = _Slot(lay, self.dev, host=True)
                self._bind(nb, npair)
            if self.tp:
                parallel.assert_same_rows(self.n_rows, "boxes + pairs")
        else:
            if nb > self.cap_boxes or npair > self.cap_pairs:
                self._grow(nb, npair)
            lay = self._layout(self.cap_boxes, self.cap_pairs)
            if self.inp is None or not self.inp.same_layout(lay):
                old, old_caps = (self.cur if self.inp is not None else None), getattr(self, "_caps", None)
                old_mid = self.mid_slot if self.inp is not None else None
                self.cur = _Slot(lay, self.dev)
                self.mid_slot = _Slot(lay, self.dev)             # stage-split schedule: the batch between ``in`` and ``cur``
                self.inp = _Slot(lay, self.dev, host=True)
                self._bind(self.cap_boxes, self.cap_pairs)
                if old is not None and self._pipelined:          # the batches in flight move to the larger slots
                    ob, op = old_caps
                    for src, dst in ((old, self.cur), (old_mid, self.mid_slot)):
                        if src is None:
                            continue
                        o, n = src.views, dst.views
                        n["rois"][:ob].copy_(o["rois"][:ob]); n["rois"][self.cap_boxes:self.cap_boxes + op].copy_(o["rois"][ob:])
                        n["ix12"][:op].copy_(o["ix12"][:op]); n["ix12"][self.cap_pairs:self.cap_pairs + op].copy_(o["ix12"][op:])
                        for name in ("labels", "masks", "wrow"):
                            n[name][:op].copy_(o[name])
                        n["extent"].copy_(o["extent"])
        cb, cp = (nb, npair) if not self.use_graph else (self.cap_boxes, self.cap_pairs)
        rois = np.zeros((cb + cp, 5), np.float32)
        rois[:nb], rois[cb:cb + npair] = fields["boxes"], fields["relb"]
        ix12 = np.zeros((2 * cp,), np.int64)
        ix12[:npair], ix12[cp:cp + npair] = fields["ixs"], fields["ixo"]
        host = {"rois": rois, "labels": fields["labels"], "ix12": ix12, "masks": host_masks, "wrow": fields["wrow"],
                "extent": np.zeros((2,), np.int32)}                  # (h, w) of the C4 maps; filled by _measure() for a new size
        if fs.fh is not None:
            host["extent"][:] = (fs.fh, fs.fw)
        self.inp.write_host(host)
        self._pipe.staged()
        self._staged = key
        first = not self.primed and self.cur is not None and not self._pipelined
        if first and not getattr(self, "_filled", False):
            # the very first batch: the head's slot starts out holding it
            self.cur.buf.copy_(self.inp.buf)
            self._filled = True

    def _bind(self, nb, npair):
        """The head reads the ``cur`` slot: its fields, and the box / pair halves of the packed ones, as attributes."""
        v = self.cur.views
        self.rois, self.ix12, self.labels, self.masks, self.wrow = v["rois"], v["ix12"], v["labels"], v["masks"], v["wrow"]
        self.boxes, self.relb = v["rois"][:nb], v["rois"][nb:]
        self.ixs, self.ixo = v["ix12"][:npair], v["ix12"][npair:]
        self._caps = (nb, npair)
        self._filled = False

    def stage_batch(self, data):
        """One roibatchLoader(path_return=True) minibatch as the DataLoader collates it -- (im_data (n,3,H,W), im_info (n,3),
        gt_boxes, num_boxes, paths) -- looked up in ``vrd.source_gt_rels`` by the last path component as the reference loop
        does (trainval_net_SGG_emb.py:211-217).  Returns False for the batches the reference skips (a frame outside the
        aspect-ratio range, :209-210; no annotated relation in any frame, faster_rcnn_SGG_emb.py:177-183)."""
        if not isinstance(data, (list, tuple)) or len(data) <= 2:
            return False
        info = data[1].detach().cpu().numpy().reshape(-1, 3)
        rels = self.net.vrd.source_gt_rels
        fields = sgg_head_inputs([rels.get(str(p).split("/")[-1]) for p in data[4]], info, self.net.vrd.n_rel)
        if fields is None:
            return False
        self.stage(data[0], info, fields)
        return True

    def stage_batch_u8(self, data):
        """One ``roibatchLoader(device_prep=True, path_return=True)`` minibatch (``collate_device_prep``): uint8 frames as
        decoded + meta; the image work runs on the device (``_place_u8``), a quarter of the float blob's bytes cross PCIe.
        Same contract as ``stage_batch`` otherwise; a minibatch the device front-end does not take (the square trim) -> False."""
        if not isinstance(data, (list, tuple)) or len(data) <= 2:
            return False
        frames = data[0]
        rows, size, info = parse_u8_meta(data[1])
        if size is None:
            return False
        rels = self.net.vrd.source_gt_rels
        fields = sgg_head_inputs([rels.get(str(p).split("/")[-1]) for p in data[4]], info, self.net.vrd.n_rel)
        if fields is None:
            return False
        self.stage(lambda fs: _place_u8(step_uploader(self), frames, rows, fs.im), info, fields, size=(len(frames),) + size)
        return True

    def reseed(self, seed):
        """Stage the synthetic minibatch of ``seed`` (the data layer's job; resident before the timed region)."""
        self.stage(*self._synthetic(seed))

    # ------------------------------------------------------------------ feature-map buffers
    _channels = 1024

    def _reserve_cells(self, cells):
        if cells <= self.cap_cells:
            return
        n = self.n_frames * self._channels * cells
        new, new_h = torch.zeros(n, device=self.dev), torch.zeros(n, device=self.dev)
        if self.fmap_flat is not None:
            new[:self.fmap_flat.numel()].copy_(self.fmap_flat)
            new_h[:self.fmap_head_flat.numel()].copy_(self.fmap_head_flat)
        if self.stage_split:          # the front half's output (layer3[cut - 1]: the C4 map's shape) of this call and of the last
            m_next, m_cur = torch.zeros(n, device=self.dev), torch.zeros(n, device=self.dev)
            if self.mid_next_flat is not None:
                m_next[:self.mid_next_flat.numel()].copy_(self.mid_next_flat)
                m_cur[:self.mid_cur_flat.numel()].copy_(self.mid_cur_flat)
            self.mid_next_flat, self.mid_cur_flat = m_next, m_cur
        self.fmap_flat, self.fmap_head_flat, self.cap_cells = new, new_h, cells
        self.invalidate_graphs()                                 # they hold the old buffers' addresses

    def reserve(self, h, w):
        """Size the feature-map buffers for frames of up to (h, w) pixels (a loop that knows its largest minibatch avoids
        re-capturing when it arrives)."""
        self._reserve_cells(((h + 15) // 16 + 1) * ((w + 15) // 16 + 1))

    def _fmap_dst(self, fs, f=None):
        """Where the feature maps of frame set ``fs`` (all frames, or frame f) live in the packed buffer: the backbone's last
        layer writes there (``RCNN_base(..., out=)``: no copy afterwards)."""
        n, c = fs.key[0], self._channels
        dst = self.fmap_flat[:n * fs.fh * fs.fw * c].view(n, fs.fh, fs.fw, c).permute(0, 3, 1, 2)
        return dst if f is None else dst[f:f + 1]

    def _measure(self, fs):
        """First sight of a frame size: one eager pass tells the extent of its C4 map (and sizes the eager arena)."""
        if fs.fh is None:
            with self.ctx_bb, torch.no_grad():
                fm = self.net.RCNN_base(fs.im[:1])
            self._channels = int(fm.shape[1])
            fs.fh, fs.fw = int(fm.shape[2]), int(fm.shape[3])
            self._reserve_cells(fs.fh * fs.fw)
            if self._staged == fs.key and self.inp is not None:      # the batch staged for this size carries its extent
                g = self._geom_dev(fs)
                self.inp.views["extent"].copy_(g)
                if not self._pipelined:
                    self.cur.views["extent"].copy_(g)

    # ------------------------------------------------------------------ the two halves of a step
    def _rotate(self):
        """Sequential schedule: the head of this call works on the batch staged last."""
        if not self._pipelined:
            self.cur.buf.copy_(self.inp.buf)

    def _rotate_after_head(self):
        """Overlapped schedule: the head of call k reads ``cur`` = batch k-1 while the backbone branches work on the frames of
        batch k; once the head is done, batch k's head inputs (still in ``inp``: the next stage() is ordered behind this call)
        move to ``cur`` for call k+1.  ONE small copy per step."""
        if self._pipelined and self.stage_split:     # three slots: in (batch k) -> mid (k-1) -> cur (k-2, the head's)
            self.cur.buf.copy_(self.mid_slot.buf)
            self.mid_slot.buf.copy_(self.inp.buf)
        elif self._pipelined:
            self.cur.buf.copy_(self.inp.buf)

    def _mid_view(self, flat, fs):
        n, c = fs.key[0], self._channels
        return flat[:n * fs.fh * fs.fw * c].view(n, fs.fh, fs.fw, c).permute(0, 3, 1, 2)

    def _front(self, fs, ctx):
        """stem .. layer3[:cut] of the frames staged last, all frames in one pass -> ``mid_next``."""
        with ctx:
            with torch.no_grad():
                self.net.RCNN_base.forward_front(fs.im, self.cut, out=self._mid_view(self.mid_next_flat, fs))

    def _back(self, fs, ctx):
        """layer3[cut:] of the previous call's front output (``mid_cur``, a minibatch of size ``fs``) -> the packed feature maps."""
        with ctx:
            with torch.no_grad():
                self.net.RCNN_base.forward_back(self._mid_view(self.mid_cur_flat, fs), self.cut, out=self._fmap_dst(fs))

    def _backbone(self, fs):
        with self.ctx_bb:
            with torch.no_grad():
                self.net.RCNN_base(fs.im, out=self._fmap_dst(fs))          # static address across replays
        self._fmap_key = fs.key

    def _backbone_per_frame(self, fs, join=True):
        """Captured form with ``bb_split``: the frames of the minibatch are independent chains of ~100 short kernels each
        (a layer3 GEMM of one frame runs ~15 us, a quarter of it set-up, first-load latency and the store tail with the
        matrix pipe idle).  One graph branch per frame: the kernels of the two chains are co-resident on every CU, the
        fixed phases of one lie under the K loops of the other."""
        main = torch.cuda.current_stream(self.dev)
        n = fs.key[0]
        for f in range(n):
            st = self._frame_streams[f]
            with launch.branch(st, main):
                with fs.ctx[f]:
                    with torch.no_grad():
                        self.net.RCNN_base(fs.im[f:f + 1], out=self._fmap_dst(fs, f))
        if join:
            launch.join(main, *self._frame_streams[:n])
        self._fmap_key = fs.key

    TRACE_COLS = ("loss", "features", "scores", "embedding", "rng_canary", "fc7_weight", "fc6_weight_head", "boxes", "labels")

    def _head(self, fs=None):
        with self.ctx_head:
            if self.use_graph:        # packed maps, extent from the batch's slot: the launches are the same for every size
                src = self.fmap_head_flat if self._pipelined else self.fmap_flat
                fmap = ops.PackedMaps(src, self.n_frames, self._channels, self.cur.views["extent"])
            else:
                fmap = self.fmap
            score, x = self.net.vrd.forward_device(fmap, self.boxes, self.relb, self.masks, self.ixs, self.ixo,
                                                   rois=self.rois, ix12=self.ix12)
            loss = ops.bce_rows(score, self.labels, self.wrow)     # sum_r wrow[r] * mean_c BCE: one kernel each way
            if self.trace is not None:
                self._record(loss, fmap, score, x)
            self.opt.zero_grad()
            loss.backward(self._seed)                              # d(loss / world): a resident scalar, no division node
            self.loss.copy_(loss.detach())
            parallel.all_reduce_grads(self.opt.params())           # world > 1: RCCL, captured with the rest of the branch
            self.opt.step()
        self._rotate_after_head()

    @torch.no_grad()
    def _record(self, loss, fmap, score, x):
        """Diagnostic rows (``trace_rows``): per step, checksums of everything the head forward read and produced, written by
        the step itself (inside the graph) so that two trajectories can be compared step by step and tensor by tensor
        without putting anything but the graph launch on the caller's stream."""
        v = self.net.vrd
        d = lambda t: torch.linalg.vector_norm(t.detach().reshape(-1).float(), 2, dtype=torch.float64)    # accumulated in double
        feats = fmap.buf if isinstance(fmap, ops.PackedMaps) else fmap
        row = torch.stack([loss.detach().double(), d(feats), d(score), d(x), torch.rand((), device=self.dev).double(),
                           d(v.fc7.fc.weight), d(v.fc6.fc.weight.view(-1)[:1 << 22]), d(self.boxes), d(self.labels)])
        i = self._trace_i.clamp(max=self.trace.shape[0] - 1)
        self.trace.index_copy_(0, i, row.view(1, -1))
        self._trace_i.add_(1)

    def _body(self):
        """Sequential form (eager, and what the sequential graph captures): backbone, then head, of the staged batch."""
        fs = self.shapes[self._staged]
        self._measure(fs)
        self._rotate()
        self._backbone(fs)
        self._head()

    def _body_overlapped(self, fs):
        """What the overlapped graph of frame set ``fs`` captures.  Fork / join through the capturing stream: everything a
        side stream does lies between ``side.wait_stream(main)`` and ``main.wait_stream(side)``, i.e. inside the graph."""
        main = torch.cuda.current_stream(self.dev)
        self._rotate()
        self.fmap_head_flat.copy_(self.fmap_flat)   # hand-off: features of the batch now in ``cur`` (computed by the previous call)
        if self.stage_split:
            # Round 6.  [head of batch k-2] | [front half of batch k: stem .. layer3[:cut]] | [back half of batch k-1].  Three
            # chains as with one branch per frame, but every backbone kernel runs over BOTH frames: fuller launches, half as
            # many of them, the Winograd-domain filters read once per pair of frames.  The step is bound by the sum of its
            # kernels' alone-times with all chains ending together, and 2-frame kernels have less of it:
            # 4.40 -> 4.08-4.12 ms per step (tools/stage_split_probe.py).  The price is one more call of latency (``lag`` 2).
            fb = self.shapes[self._mid_key]         # the minibatch whose front half ran in the previous call
            self.mid_cur_flat.copy_(self.mid_next_flat)
            sa, sb = self._frame_streams[0], self._frame_streams[1]
            with launch.branch(sa, main):
                self._front(fs, fs.ctx_front)
            with launch.branch(sb, main):
                self._back(fb, fb.ctx_back)
            self._head()
            launch.join(main, sa, sb)
            return
        if self.bb_split:                   # one branch per frame, forked from the capturing stream itself (a fork inside a
            self._backbone_per_frame(fs, join=False)      # forked branch crashes hipStreamEndCapture on ROCm 7.2)
            self._head()
            launch.join(main, *self._frame_streams[:fs.key[0]])
            return
        with launch.branch(self._side, main):
            self._backbone(fs)              # batch k+1
        self._head()                        # batch k
        launch.join(main, self._side)

    def prime(self):
        """Overlapped schedule only: backbone pass of the batch staged first, so that the first call's head finds its
        features (``cur`` <- ``in`` as the end of a call would have done)."""
        if self.overlap and not self.primed:
            fs = self.shapes[self._staged]
            self._measure(fs)
            if self.stage_split:
                # the batch staged first fills EVERY stage of the pipeline: both backbone halves run here, all three slots hold
                # it.  A resident minibatch is then trained by every call from the first; a staging loop trains it in its first
                # call, runs no head in the second (``bubble``: the slot still holds the first batch) and is in step from the third
                self.cur.buf.copy_(self.inp.buf)
                self.mid_slot.buf.copy_(self.inp.buf)
                self._front(fs, self.ctx_bb)
                self.mid_cur_flat.copy_(self.mid_next_flat)
                self._back(fs, self.ctx_bb)
                self._mid_key = self._fmap_key = fs.key
                self._pipe.prime()
            else:
                self.cur.buf.copy_(self.inp.buf)
                self._backbone(fs)
        self.primed = True

    def _fill_call(self, fs):
        """A call while the stage pipeline fills: the graph's two backbone chains on eager launches, the slots advance, no head."""
        fb = self.shapes[self._mid_key]
        self.mid_cur_flat.copy_(self.mid_next_flat)
        self._back(fb, self.ctx_bb)
        self._front(fs, self.ctx_bb)
        self.cur.buf.copy_(self.mid_slot.buf)
        self.mid_slot.buf.copy_(self.inp.buf)
        self._fmap_key, self._mid_key = fb.key, fs.key

    # ------------------------------------------------------------------ capture
    def _graph_holders(self):
        return self.shapes.values()

    def capture(self, warmup=2, restore=False):
        """Warm up eagerly (sizes the arenas, fills the allocator), then capture the step for the staged frame size into ONE
        HIP graph (other sizes are captured when they are first staged).  Returns False (and keeps the eager form,
        ``graph_error`` says why) when graphs are off or capture fails.  ``restore``: the warm-up steps are real training
        steps on the staged batch; put parameters, momentum and the RNG state back afterwards (a training loop that must
        not see them).  ``warmup=0`` re-captures (after a learning-rate change: rates live in the captured kernel
        arguments)."""
        saved = self._snapshot() if (restore and warmup) else None
        try:
            return self._capture(warmup)
        finally:
            if saved is not None:
                self._restore(saved)      # AFTER the recording: it changes no training state here (_capture_frames)

    def _capture(self, warmup):
        if self.tp:
            parallel.assert_same_rows(self.cap_boxes + self.cap_pairs if self.use_graph else self.n_rows, "boxes + pairs")
        if warmup == 0:
            self.invalidate_graphs()
        fs = self.shapes[self._staged]
        self._measure(fs)
        pipelined, self._pipelined = self._pipelined, False     # the warm-up steps are sequential eager steps
        self._warm_up(warmup, self._body, lambda: (self.ctx_bb.fit(), self.ctx_head.fit()))
        self._pipelined = pipelined
        if not self.use_graph:
            return False
        if self.overlap and not self._pipelined:
            self._pipelined = True
            self.prime()
            torch.cuda.synchronize(self.dev)
        ok = self._capture_frames(fs)
        if ok:
            self._graphs_on = True
        elif not self._graphs_on:
            self._pipelined = False      # nothing was ever captured: plain sequential eager steps (the documented fall-back)
            self.overlap = False
        return ok

    def _capture_frames(self, fs):
        """Capture the step whose backbone half works on frame set ``fs``.  Nothing here changes the training state: the
        per-frame arenas are sized by eager backbone passes into scratch outputs (the backbone is frozen), the head half is
        recorded, not run."""
        self._measure(fs)
        staged = self._pipelined and self.stage_split
        fb = self.shapes[self._mid_key] if staged else None       # the minibatch the back half of this graph works on
        if self._pipelined and self.bb_split and not fs.fitted:
            for _rep in range(2):
                for f, ctx in enumerate(fs.ctx):
                    with ctx:
                        with torch.no_grad():
                            self.net.RCNN_base(fs.im[f:f + 1])
                    ctx.fit()
            torch.cuda.synchronize(self.dev)
        if staged and not (fs.fitted_front and fb.fitted_back):
            # arenas of the two half contexts, sized by eager passes into SCRATCH outputs (mid_next / the feature maps hold live
            # pipeline state: the fitting passes must not write them; what they read may be stale)
            for _rep in range(2):
                if not fs.fitted_front:
                    with fs.ctx_front:
                        with torch.no_grad():
                            self.net.RCNN_base.forward_front(fs.im, self.cut)
                    fs.ctx_front.fit()
                if not fb.fitted_back:
                    with fb.ctx_back:
                        with torch.no_grad():
                            self.net.RCNN_base.forward_back(self._mid_view(self.mid_cur_flat, fb), self.cut)
                    fb.ctx_back.fit()
            fs.fitted_front = fb.fitted_back = True
            torch.cuda.synchronize(self.dev)
        fs.fitted = True
        if staged:                    # a graph per (front size, back size) pair
            old = self._evict_lru([(f, k) for f in self.shapes.values() for k, g in f.graphs.items() if g])
            if old is not None and old.graph is not None and not any(old.graphs.values()):
                old.graph = None      # its last pair graph went
        else:
            self._evict_lru([(f, None) for f in self.shapes.values() if f.graph])
        if self._pipelined and self._side is None:
            self._side = launch.role_stream(self.dev, "side")
        fmap_key = self._fmap_key
        try:                          # (the recording starts with a device synchronisation: the fitting passes above are finished)
            g = self._record_graph((lambda: self._body_overlapped(fs)) if self._pipelined else self._body)      # fs is the staged set
        finally:
            self._fmap_key = fmap_key        # recording is not running: the buffer still holds what it held
        fs.graph = g                  # False: eager launches for this size
        if staged:
            fs.graphs[fb.key] = g
        return bool(g)

    def _step(self):
        """A call of the step.  Returns the device scalar holding the loss of the batch the head just processed.
        Before a successful ``capture()`` a call is the sequential eager step."""
        fs = self.shapes[self._staged]
        if self._graphs_on and self._pipelined and self.stage_split:
            self._measure(fs)
            if self._pipe.call() is None:
                self._fill_call(fs)              # the pipeline fills: both backbone halves, no head
                self.n_bubbles += 1
            else:
                fb_key = self._mid_key
                if fs.graphs.get(fb_key) is None:
                    self._capture_frames(fs)     # first sight of this (front size, back size) pair
                g = fs.graphs.get(fb_key)
                self._tick += 1
                fs.tick = self._tick
                fs.graph = g if g else fs.graph
                if g:
                    replay_graph(g, self.dev)
                else:
                    self._body_overlapped(fs)    # this pair could not be captured: the same schedule on eager launches
                self._fmap_key, self._mid_key = fb_key, fs.key
        elif self._graphs_on:
            if fs.graph is None:
                self._capture_frames(fs)         # first sight of this frame size (or the graphs were invalidated)
            self._tick += 1
            fs.tick = self._tick
            if fs.graph:
                replay_graph(fs.graph, self.dev)
                self._fmap_key = fs.key
            elif self._pipelined:
                self._body_overlapped(fs)        # this size could not be captured: the same schedule on eager launches
            else:
                self._body()
        else:
            self._body()
        self.opt.bump()
        return self.loss

    def flush(self):
        """Overlapped schedule: one more call without a new ``stage()`` -- the batches already in the pipeline advance one stage
        (``lag`` such calls end a loop: the last one runs the head of the batch staged last)."""
        return self()


def run_staged(step, stagers, keep):
    """Drive ``step`` (any schedule) over ``1 + len(stagers)`` minibatches: the first one is staged (and the step captured)
    already, ``stagers[k]()`` stages the next.  One minibatch is staged before every call while there are any; calls go on until
    the head has trained every minibatch; ``keep[j]`` (a device vector) receives the loss of minibatch j right behind its call
    (no host synchronisation).  Calls that run no head (``SGGEmbStep.bubble``) are not counted."""
    trained, nxt, total = 0, 0, len(stagers) + 1
    while trained < total:
        if nxt < len(stagers):
            stagers[nxt]()
            nxt += 1
        bubble = getattr(step, "bubble", False)
        loss = step()
        if not bubble:
            keep[trained].copy_(loss)
            trained += 1
    return keep


class _SplitBatch(torch.autograd.Function):
    """(x[:n], x[n:]) along the batch axis as views; the backward writes the two gradients into ONE buffer (autograd's own
    slice backward zero-fills a full-size tensor per slice and adds them)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.shape = n, tuple(x.shape)
        ctx.fmt = torch.channels_last if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) else torch.contiguous_format
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        ref = ga if ga is not None else gb
        out = torch.empty(ctx.shape, device=ref.device, dtype=ref.dtype, memory_format=ctx.fmt)
        for dst, g in ((out[:ctx.n], ga), (out[ctx.n:], gb)):
            if g is None:
                dst.zero_()
            else:
                dst.copy_(g)
        return out, None


class _DomainSet:
    """What the instance_styleD step owns for ONE pair of minibatch sizes (source (n,Hs,Ws), target (n,Ht,Wt)) and one
    ``im_info[0]`` (the anchor-target layer's inside test follows it, anchor_target_layer.py:85-86): the staged frames,
    the launch contexts and the captured graph."""

    def __init__(self, key, device, batched, branches):
        n, hs, ws, ht, wt = key[:5]
        # frames live in the layout the stem consumes (NHWC, zero fourth channel: ops.image_prep's blob): stage() does the
        # NCHW3 -> NHWC4 placement once, outside the step, instead of a fill + a copy per branch inside it
        z = lambda b, h, w: torch.zeros((b, 4, h, w), device=device).contiguous(memory_format=torch.channels_last)
        self.key = key
        self.im_s, self.im_t = z(n, hs, ws), z(n, ht, wt)
        self.im_st = z(2 * n, hs, ws) if (batched and (hs, ws) == (ht, wt)) else None
        # ordered=True (round 6): every split reduction of the detector step in a fixed order -- bit-reproducible steps at
        # +0.3 % (round 5: +4 %, most of it ONE unsplit 18-row filter gradient)
        self.ctx = launch.LaunchContext(device, ordered=True)
        self.ctx_src = launch.LaunchContext(device, ordered=True) if branches else None
        self.ctx_tgt = launch.LaunchContext(device, ordered=True) if branches else None
        self.graph = None             # None: not captured yet; False: capture failed (eager launches for this key)
        self.fitted = False
        self.tick = 0

    def drop_graphs(self):
        self.graph = None


class InstanceStyleDStep(CapturedStep):
    """One D+G adversarial step (trainval_net_instance_styleD_bilinear.py:262-341): source forward with
    detection + RPN losses and 0.5*mean(d^2) for both discriminators, target forward with
    0.5*mean((1-d)^2), style terms weighted by style_lambda, ONE backward through the gradient-reversal
    layers, one SGD step over every trainable parameter.

    Eager by default with the target layers sampling on the host from the reference's np.random stream (bit parity with
    the reference's RNG contract; two small D2H copies per step).  ``capture()`` switches the target layers to
    device-side sampling (same subsample sizes, torch's generator) and records the whole step -- both forwards, the
    backward, the gradient exchange and the update -- into ONE HIP graph.

    The two data loaders of the loop pad every minibatch to its own aspect ratio (roibatchLoader.py:162-190), so source
    and target frames come in several sizes.  ``stage()`` takes any; a graph is captured the first time a (source size,
    target size) pair is met -- after one eager step at that size that sizes the arenas and fills the host-built caches
    (anchor grids), whose effect on parameters, momentum and the RNG stream is undone -- and replayed from then on; at most
    ``max_graphs`` are kept, in one shared memory pool (no two of them ever run at the same time)."""

    def __init__(self, net, n_frames, lr=5e-4, eta=0.1, eta_style=0.001, style_lambda=1.0, seed=3, device="cuda:0",
                 h=600, w=1000, n_gt=8, cr=False, max_graphs=32, stage_synthetic=True, optimizer="sgd"):
        self.net, self.dev = net, torch.device(device)
        self.cr = cr                  # --cr: consistency regularisation between instance- and image-level D (:299-312)
        self.world = parallel.world_size()
        self.eta, self.eta_style, self.style_lambda = eta, eta_style, style_lambda
        self.geom = (h, w)
        self.n_frames, self.n_gt = n_frames, n_gt
        import os
        self.batched = True
        # filter gradients of the bottleneck nodes on a side branch of the step (launch.SideBranch)
        # (only with the one-pass backbone: a filter met twice in one backward would have its two gradients added on the main
        # stream while the side branch may still be writing the first)
        self.wgrad_branch = False      # filter gradients on a side branch: -1 % of the step for +2.4 GB; a test sets it
        self._wgrad_stream = launch.role_stream(self.dev, "wgrad") if self.wgrad_branch else None
        # the captured step: source and target as two branches of the graph (_body_branches)
        self.branches = os.environ.get("I2V_ISD_BRANCHES", "1") != "0" and self.dev.type == "cuda" and not self.wgrad_branch
        self._branch_streams = [launch.role_stream(self.dev, ("domain", i)) for i in range(2)] if self.branches else []
        self.sets, self.max_graphs, self._tick, self._pool = {}, int(max_graphs), 0, None
        self._cur = None              # the _DomainSet staged last
        self._graphs_on = False
        mg = int(cfg.MAX_NUM_GT_BOXES)
        self.info = torch.zeros((n_frames, 3), device=self.dev)        # shared by every size: a captured step reads them
        self.info_t = torch.zeros((n_frames, 3), device=self.dev)
        self.gt = torch.zeros((n_frames, mg, 5), device=self.dev)
        self.nb = torch.zeros((n_frames,), device=self.dev)
        self.gt_t = torch.zeros((n_frames, 1, 5), device=self.dev)
        self.nb_t = torch.zeros((n_frames,), device=self.dev)
        if stage_synthetic:           # a loop fed by data loaders stages its own first minibatch (``stage_batch``)
            self.reseed(seed)
        self.opt = make_optimizer(optimizer, list(net.named_parameters()), lr)
        # the gradient exchange in buckets (parallel.exchange_in_buckets; only when an exchange exists): bucket of every
        # parameter, and a hook per parameter that marks, on the stream its gradient was produced on, where its bucket stands
        ids, _ = parallel.detector_buckets([it["name"] for it in self.opt.items])
        used = sorted(set(ids))
        self._buckets = [[i for i, b in enumerate(ids) if b == k] for k in used]
        self._marks = None            # the parallel.BucketMarks of the branch whose backward is being queued
        for i, p in enumerate(self.opt.params()):
            p.register_hook(lambda g, k=used.index(ids[i]): self._bucket_hit(k))
        # total, det = the four detection losses summed, the four discriminator terms (trainval_net_instance...:276-296), then the
        # four detection losses one by one (rpn_loss_cls, rpn_loss_box, RCNN_loss_cls, RCNN_loss_bbox: :276-279)
        self.names = ["total", "det", "dloss_s", "dloss_t", "dloss_s_style", "dloss_t_style"] + \
            (["source_adv_cst", "target_adv_cst"] if cr else []) + ["rpn_cls", "rpn_box", "rcnn_cls", "rcnn_box"]
        self._loss_buf = torch.zeros((len(self.names),), device=self.dev)           # static addresses: a captured step writes here
        self.losses = {k: self._loss_buf[i] for i, k in enumerate(self.names)}      # (views: one stack + one copy per step)
        self.graph_error = None

    # ------------------------------------------------------------------ compatibility views
    @property
    def graph(self):
        return (self._cur.graph or None) if self._cur is not None else None

    im_s = property(lambda self: self._cur.im_s)
    im_t = property(lambda self: self._cur.im_t)
    im_st = property(lambda self: self._cur.im_st)
    ctx = property(lambda self: self._cur.ctx)
    ctx_src = property(lambda self: self._cur.ctx_src)
    ctx_tgt = property(lambda self: self._cur.ctx_tgt)

    # ------------------------------------------------------------------ data side
    def stage(self, im_s, info, gt, nb, im_t, info_t=None, placers=None):
        """Hand the next minibatch to the step: source frames (N,3,H,W) with ``im_info`` (N,3), ``gt_boxes``
        (N,MAX_NUM_GT_BOXES,5) and ``num_boxes`` (N,) -- one roi_data_layer batch -- and N target frames with their
        ``im_info`` (default: the source's).  Host tensors cross PCIe here (pinned ones asynchronously); everything is
        copied into static device tensors on the caller's stream (a captured step is bound to their addresses)."""
        n, _, hs, ws = im_s.shape
        ht, wt = int(im_t.shape[2]), int(im_t.shape[3])
        if int(n) != self.n_frames or int(im_t.shape[0]) != self.n_frames:
            raise ValueError("InstanceStyleDStep.stage: %d source / %d target frames, the step was built for %d"
                             % (n, im_t.shape[0], self.n_frames))
        if tuple(gt.shape[1:]) != tuple(self.gt.shape[1:]):
            raise ValueError("InstanceStyleDStep.stage: gt_boxes must be (N, MAX_NUM_GT_BOXES = %d, 5)" % self.gt.shape[1])
        info_t = info if info_t is None else info_t
        info0 = info[0].tolist()                    # a loader's im_info is a host tensor: no synchronisation
        key = (int(n), int(hs), int(ws), ht, wt, int(info0[0]), int(info0[1]))
        ds = self.sets.get(key)
        if ds is None:
            ds = self.sets[key] = _DomainSet(key, self.dev, self.batched, self.branches)
        self._tick += 1
        ds.tick = self._tick
        self._cur = ds
        self.info0 = (int(info0[0]), int(info0[1]))
        cp = lambda dst, src: dst.copy_(src, non_blocking=True)
        for k, (dst, src) in enumerate(((ds.im_s, im_s), (ds.im_t, im_t))):
            if placers is not None:                              # the device front-end writes the frames itself (_place_u8)
                placers[k](dst)
            else:
                place_frames(dst, src, self)
        cp(self.info, info); cp(self.info_t, info_t); cp(self.gt, gt); cp(self.nb, nb)
        if ds.im_st is not None:
            ds.im_st[:n].copy_(ds.im_s); ds.im_st[n:].copy_(ds.im_t)

    def stage_batch_u8(self, data_s, data_t):
        """The same with ``roibatchLoader(device_prep=True)`` minibatches (``collate_device_prep``): uint8 frames, the image work
        on the device.  False when either minibatch cannot go that way (the square trim) or would be skipped."""
        if not all(isinstance(d, (list, tuple)) and len(d) >= 4 for d in (data_s, data_t)):
            return False
        (ms, size_s, info), (mt, size_t, info_t) = parse_u8_meta(data_s[1]), parse_u8_meta(data_t[1])
        if size_s is None or size_t is None:
            return False
        n, up = len(data_s[0]), step_uploader(self)
        self.stage(torch.empty((n, 0) + size_s), torch.from_numpy(info), data_s[2], data_s[3], torch.empty((n, 0) + size_t),
                   torch.from_numpy(info_t), placers=(lambda dst: _place_u8(up, data_s[0], ms, dst),
                                                      lambda dst: _place_u8(up, data_t[0], mt, dst)))
        return True

    def stage_batch(self, data_s, data_t):
        """One minibatch of each of the loop's two ``roibatchLoader`` iterators as the DataLoader collates them
        (trainval_net_instance_styleD_bilinear.py:236-291): source (im_data, im_info, gt_boxes, num_boxes), target
        (im_data, im_info, ...) whose boxes are not used.  Returns False for the batches the reference skips (:241-252)."""
        if not isinstance(data_s, (list, tuple)) or not isinstance(data_t, (list, tuple)) or len(data_s) < 4 or len(data_t) < 2:
            return False
        self.stage(data_s[0], data_s[1], data_s[2], data_s[3], data_t[0], data_t[1])
        return True

    def reseed(self, seed):
        """Stage the synthetic minibatch of ``seed`` (frames, 8 GT boxes per source frame)."""
        h, w = self.geom
        ims, info = syn.frames(seed, self.n_frames, h, w)
        imt, _ = syn.frames(seed + 100, self.n_frames, h, w)
        gt, nb = syn.gt_boxes(seed, self.n_frames, self.n_gt, self.net.n_classes, cfg.MAX_NUM_GT_BOXES, h, w)
        f = torch.from_numpy
        self.stage(f(ims), f(info), f(gt), f(nb), f(imt))

    def _body(self):
        net = self.net
        with self.ctx:
            batched = self.batched and self.im_st is not None      # one pass needs source and target frames of one size
            if batched:
                # ONE backbone pass over the source and the target frames (the reference makes two, :271 and :293; with
                # frozen BN they are the same arithmetic): half the launches of the trunk's forward, data-gradient and
                # filter-gradient kernels, each over twice the pixels, and no accumulation adds between two backward
                # passes through the same filters
                feat, feat1 = net.extract_feature(self.im_st)
                n = self.im_s.shape[0]
                (fs, ft), (f1s, f1t) = _SplitBatch.apply(feat, n), _SplitBatch.apply(feat1, n)
                out = net.forward_features(fs, f1s, self.info, self.gt, self.nb, False, self.eta, self.eta_style)
            else:
                out = net(self.im_s, self.info, self.gt, self.nb, target=False, eta=self.eta, eta_style=self.eta_style)
            _, _, _, l_rpn_cls, l_rpn_box, l_cls, l_box, _, d_inst, d_style = out
            parts = dict(rpn_cls=_mean1(l_rpn_cls), rpn_box=_mean1(l_rpn_box), rcnn_cls=_mean1(l_cls), rcnn_box=_mean1(l_box))
            loss = parts["rpn_cls"] + parts["rpn_box"] + parts["rcnn_cls"] + parts["rcnn_box"]
            dloss_s = ops.half_mse(d_inst)                  # 0.5 * mean(d^2) (:276-277), one kernel each way
            dloss_s_style = ops.half_mse(d_style)
            if batched:
                d_inst_t, d_style_t = net.forward_features(ft, f1t, self.info_t, self.gt_t, self.nb_t, True, self.eta,
                                                           self.eta_style)
            else:
                d_inst_t, d_style_t = net(self.im_t, self.info_t, self.gt_t, self.nb_t, target=True, eta=self.eta,
                                          eta_style=self.eta_style)
            dloss_t = ops.half_mse(d_inst_t, 1.0)           # 0.5 * mean((1 - d)^2) (:294-295)
            dloss_t_style = ops.half_mse(d_style_t, 1.0)
            total = loss + dloss_s + dloss_t + self.style_lambda * (dloss_s_style + dloss_t_style)
            vals = dict(det=loss, dloss_s=dloss_s, dloss_t=dloss_t, dloss_s_style=dloss_s_style, dloss_t_style=dloss_t_style, **parts)
            if self.cr:
                cst = consistency_terms(d_inst, d_style, d_inst_t, d_style_t)
                total = total + cst["source_adv_cst"] + cst["target_adv_cst"]
                vals.update(cst)
            vals["total"] = total
            self.opt.zero_grad()
            side = launch.WGRAD_BRANCH = launch.SideBranch(self._wgrad_stream) if self.wgrad_branch else None
            try:
                (total / self.world).backward()
                if side is not None:
                    side.join()
            finally:
                launch.WGRAD_BRANCH = None
            parallel.all_reduce_grads(self.opt.params())
            self.opt.step()
            self._loss_buf.copy_(torch.stack([vals[k].detach().reshape(()) for k in self.names]))

    eager_step = _body

    def _body_branches(self):
        """The captured form by default (``I2V_ISD_BRANCHES=0``: the one-pass form above): the source and the target forward /
        backward as TWO BRANCHES of the step graph -- they are independent until their gradients meet (the reference runs
        them one after the other, :271-296).  An 8-frame layer3 GEMM runs at 102 TF alone; two 4-frame chains side by side
        reach 114 TF (tools/corun_probe.py): one chain's set-up / store phases lie under the other's K loops, with no edge
        between the branches until the join.  Each branch owns a LaunchContext (arena, split-K workspace, scratch) and
        returns its gradients through ``torch.autograd.grad`` (no AccumulateGrad on a shared ``.grad`` from two streams);
        the capturing stream adds them after the join."""
        net, main = self.net, torch.cuda.current_stream(self.dev)
        params = self.opt.params()
        self.opt.zero_grad()
        s_src, s_tgt = self._branch_streams
        vals, grads = {}, {}
        # Each branch's autograd graph is gone before the other branch's forward starts (only detached values leave the
        # block): a parameter's AccumulateGrad node lives as long as a graph references it and remembers the stream it was
        # made on -- shared between the two branches the engine would synchronise their streams with each other.
        def source():
            out = net(self.im_s, self.info, self.gt, self.nb, target=False, eta=self.eta, eta_style=self.eta_style)
            _, _, _, l_rpn_cls, l_rpn_box, l_cls, l_box, _, d_inst, d_style = out
            v = dict(rpn_cls=_mean1(l_rpn_cls), rpn_box=_mean1(l_rpn_box), rcnn_cls=_mean1(l_cls), rcnn_box=_mean1(l_box))
            v.update({"det": v["rpn_cls"] + v["rpn_box"] + v["rcnn_cls"] + v["rcnn_box"],
                      "dloss_s": ops.half_mse(d_inst), "dloss_s_style": ops.half_mse(d_style)})
            part = v["det"] + v["dloss_s"] + self.style_lambda * v["dloss_s_style"]
            if self.cr:
                v["source_adv_cst"] = _consistency_term(d_inst, d_style)
                part = part + v["source_adv_cst"]
            g = torch.autograd.grad(part / self.world, params, allow_unused=True)
            v["_src"] = part
            net.RCNN_rpn.rpn_loss_cls = net.RCNN_rpn.rpn_loss_box = 0      # the module keeps its last losses (rpn.py:89-108): they hold the graph
            return {k: t.detach() for k, t in v.items()}, g

        def target():
            d_inst_t, d_style_t = net(self.im_t, self.info_t, self.gt_t, self.nb_t, target=True, eta=self.eta,
                                      eta_style=self.eta_style)
            v = {"dloss_t": ops.half_mse(d_inst_t, 1.0), "dloss_t_style": ops.half_mse(d_style_t, 1.0)}
            part = v["dloss_t"] + self.style_lambda * v["dloss_t_style"]
            if self.cr:
                v["target_adv_cst"] = _consistency_term(d_inst_t, d_style_t)
                part = part + v["target_adv_cst"]
            g = torch.autograd.grad(part / self.world, params, allow_unused=True)
            v["_tgt"] = part
            return {k: t.detach() for k, t in v.items()}, g

        exchange = parallel.exchange_enabled()
        marks = {}
        try:
            with launch.branch(s_src, main), self.ctx_src:
                self._marks = marks["s"] = parallel.BucketMarks(True) if exchange else None
                v, grads["s"] = source()
                vals.update(v)
            with launch.branch(s_tgt, main), self.ctx_tgt:
                self._marks = marks["t"] = parallel.BucketMarks(True) if exchange else None
                v, grads["t"] = target()
                vals.update(v)
        finally:
            self._marks = None
        if exchange:
            # Round 6: the exchange runs on the CAPTURING stream, which has nothing else to do between the fork of the two domain
            # branches and their join.  Bucket k (backward order: heads + layer4 + RPN, layer3 in three slices, the early layers)
            # is summed over the two domains and all-reduced as soon as BOTH branches have queued its last gradient -- an event
            # edge from each -- so the 80 MB of bucket 0 cross xGMI beside the backward of layer3, each layer3 slice beside the
            # next, and only the last bucket (layer2 / layer1 / netD_style, ~10 MB) is exposed.  Rounds 1-5: one all-reduce of
            # all 202 MB after the join.  (Not a third forked branch: RCCL runs a collective on a stream of its own forked from
            # the issuing one, and a fork inside a forked branch ends hipStreamEndCapture in a host segfault -- DESIGN.md 5.1;
            # the first form of this schedule died exactly so.)
            tokens = parallel.exchange_in_buckets(params, self._buckets, [grads["s"], grads["t"]], (marks["s"], marks["t"]), main)
            parallel.finish_buckets(tokens)
            launch.join(main, s_src, s_tgt)
        else:
            launch.join(main, s_src, s_tgt)
            both = [(a, b) for a, b in zip(grads["s"], grads["t"]) if a is not None and b is not None]
            if both:
                torch._foreach_add_([a for a, _ in both], [b for _, b in both])
            for p, a, b in zip(params, grads["s"], grads["t"]):
                p.grad = a if a is not None else b
        vals["total"] = vals.pop("_src") + vals.pop("_tgt")
        self.opt.step()
        self._loss_buf.copy_(torch.stack([vals[k].detach().reshape(()) for k in self.names]))

    def _bucket_hit(self, k):
        m = self._marks
        if m is not None:
            m.hit(k)

    def _device_sampling(self, on):
        atl = self.net.RCNN_rpn.RPN_anchor_target
        atl.device_sampling = on
        # the inside-anchor test follows im_info[0] (anchor_target_layer.py:85-86); its value is known on the host from the
        # staged batch, so the layer needs no device read -- and a captured step is keyed by it (``_DomainSet``)
        atl.image_size = self.info0 if on else None
        self.net.RCNN_proposal_target.device_sampling = on

    def _graph_holders(self):
        return self.sets.values()

    def capture(self, warmup=2, restore=False):
        """Device-side target sampling, eager warm-up, then the whole step for the staged sizes as ONE HIP graph (other
        sizes are captured when they are first staged).  False (eager form kept, host-side sampling restored, ``graph_error``
        says why) when capture fails.  ``restore``: the warm-up steps are real training steps on the staged batch; put
        parameters, momentum and the RNG state back afterwards.  ``warmup=0`` re-captures (after a learning-rate change:
        the rates live in the captured kernel arguments)."""
        if warmup == 0:
            self.invalidate_graphs()
        ok = self._capture_set(self._cur, warmup, restore)
        if ok:
            self._graphs_on = True
        elif not self._graphs_on:
            self._device_sampling(False)         # the eager form keeps the np.random contract it documents
        return ok

    def _capture_set(self, ds, warmup, restore):
        saved = self._snapshot() if (restore and warmup) else None
        body = self._body_branches if self.branches else self._body

        def fit():
            if not ds.fitted:
                for ctx in (ds.ctx, ds.ctx_src, ds.ctx_tgt):
                    if ctx is not None:
                        ctx.fit()
                ds.fitted = True
        try:
            self._device_sampling(True)
            self._warm_up(warmup, body, fit)
        finally:
            if saved is not None:
                self._restore(saved)      # BEFORE the recording: it registers torch's generator (device-side sampling), so the RNG state in force may matter
        self._evict_lru([(d, None) for d in self.sets.values() if d.graph])
        ds.graph = self._record_graph(body)      # (synchronises the device first, on the warmup=0 path too); False: eager launches for this key
        return bool(ds.graph)

    def _step(self):
        ds = self._cur
        if self._graphs_on:
            if ds.graph is None:
                # first sight of this pair of sizes (or the graphs were invalidated): one eager step sizes its arenas and
                # fills the host-built caches, its effect on the training state is undone, then the step is recorded
                self._capture_set(ds, 0 if ds.fitted else 1, True)
            if ds.graph:
                replay_graph(ds.graph, self.dev)
            else:
                self._device_sampling(True)
                (self._body_branches if self.branches else self._body)()
            self.opt.bump()
        else:
            self._body()
            if not ds.fitted:           # eager use: size the arena of atomically accumulated outputs after the first step
                ds.ctx.fit()
                ds.fitted = True
        return self.losses["total"]


def _mean1(t):
    """``t.mean()`` of the loop (trainval_net_instance_styleD_bilinear.py:276-279) without a reduction kernel when t holds one
    element (the detector returns its four losses as 1-element tensors)."""
    return t.reshape(()) if t.numel() == 1 else t.mean()


def _consistency_term(di, ds):
    """One domain's term of ``consistency_terms`` below."""
    per_roi = di.mean(3).mean(2)
    rois_per_frame = per_roi.shape[0] // ds.shape[0]
    prob = ds.reshape(ds.shape[0], -1)[:, :1].repeat(1, rois_per_frame).view(-1, 1)
    return torch.nn.functional.mse_loss(per_roi, prob.detach())


def consistency_terms(d_inst, d_style, d_inst_t, d_style_t):
    """trainval_net_instance_styleD_bilinear.py:299-311 (``--cr``): MSE between the per-ROI mean of the instance
    discriminator map and the (detached) image-level discriminator output repeated once per ROI.  The reference
    hard-codes 128 ROIs per image (``repeat(1,128)``); here the repeat count is the actual
    number of ROIs per frame, which is the same thing at TRAIN.BATCH_SIZE = 128."""
    out = {}
    for name, di, ds in (("source_adv_cst", d_inst, d_style), ("target_adv_cst", d_inst_t, d_style_t)):
        per_roi = di.mean(3).mean(2)                                  # (B*R, 1)
        rois_per_frame = per_roi.shape[0] // ds.shape[0]
        prob = ds.reshape(ds.shape[0], -1)[:, :1].repeat(1, rois_per_frame).view(-1, 1)
        out[name] = torch.nn.functional.mse_loss(per_roi, prob.detach())
    return out


def build_instance_styled_net(layers=101, n_cls=16, seed=0, device="cuda:0", ic=False, gc=False, class_agnostic=False):
    from .model.faster_rcnn.resnet_instance_styleD_bilinear import resnet
    torch.manual_seed(seed)
    net = resnet(tuple(range(n_cls)), layers, class_agnostic=class_agnostic, ic=ic, gc=gc)
    net.create_architecture()
    _randomise_bn(net, seed + 1)
    return net.to(device).train()


def _randomise_bn(net, seed):
    """Frozen-BN statistics as a trained checkpoint would have them (gamma < 1 on the block outputs keeps
    activations O(1) through 33 residual blocks)."""
    g = torch.Generator().manual_seed(seed)
    for name, m in net.named_modules():
        if m.__class__.__name__ == "FrozenBN":
            c = m.weight.numel()
            hi = 0.5 if name.endswith("bn3") else 1.0
            m.weight.data.copy_(torch.rand(c, generator=g) * (hi - 0.2) + 0.2)
            m.bias.data.copy_(torch.rand(c, generator=g) * 0.2 - 0.1)
            m.running_mean.copy_(torch.rand(c, generator=g) * 0.2 - 0.1)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            m.invalidate()


def build_sgg_net(layers=101, n_rel=62, n_cls=16, seed=0, device="cuda:0", emb_dim=300, use_obj_visual=True, spatial_type=2,
                  vrd_task="pre_det"):
    """Random-init SGG_emb model of the reference architecture (no checkpoint is reachable).  ``emb_dim``,
    ``use_obj_visual``, ``spatial_type``, ``vrd_task``: the reference's flags (parser_func.py:155-163,182)."""
    import argparse
    from .model.faster_rcnn.resnet_SGG_emb import resnet
    torch.manual_seed(seed)
    args = argparse.Namespace(num_relations=n_rel, num_classes=n_cls, emb_dim=int(emb_dim), use_obj_visual=bool(use_obj_visual),
                              spatial_type=int(spatial_type), vrd_task=vrd_task)
    net = resnet(tuple(range(n_cls)), args, layers, obj_vecs=syn.word_vectors(22, n_cls),
                 prd_vecs=syn.word_vectors(21, n_rel))
    net.create_architecture()
    _randomise_bn(net, seed + 1)
    return net.to(device).train()


# FLOPs of the implicit-GEMM launches of one SGGEmbStep (algorithmic: 2*M*N*K per launch) -------------
def conv_flops_backbone(n_frames, h=600, w=1000, blocks=(3, 4, 23)):
    """2*MAC of conv1..layer3 for n_frames frames (166.1 GFLOP/frame at 600x1000).
    Returns (flops, launches)."""
    def out(n, k, s, p):
        return (n + 2 * p - k) // s + 1
    fl, n = 0, 0
    H, W = out(h, 7, 2, 3), out(w, 7, 2, 3)
    fl += 2 * H * W * 64 * 49 * 3; n += 1
    H, W = -(-(H - 3) // 2) + 1, -(-(W - 3) // 2) + 1
    cin = 64
    for planes, nb, stride in ((64, blocks[0], 1), (128, blocks[1], 2), (256, blocks[2], 2)):
        for i in range(nb):
            s = stride if i == 0 else 1
            Ho, Wo = out(H, 1, s, 0), out(W, 1, s, 0)
            fl += 2 * Ho * Wo * planes * cin                       # conv1 1x1 (strided)
            fl += 2 * Ho * Wo * planes * planes * 9                # conv2 3x3
            fl += 2 * Ho * Wo * planes * 4 * planes                # conv3 1x1
            n += 3
            if i == 0:
                fl += 2 * Ho * Wo * planes * 4 * cin               # downsample
                n += 1
            H, W, cin = Ho, Wo, planes * 4
    return fl * n_frames, n
