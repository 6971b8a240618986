"""Host side of a minibatch and its way onto the device: synthetic batches, the relation head's input tables, packed
slots that cross PCIe as one copy, and the copy-stream uploader."""
import numpy as np
import torch

from . import launch, ops
from . import synthetic as syn
from .model.utils.config import cfg


def synthetic_sgg_batch(seed, n_frames, n_boxes=32, n_pairs=32, n_rel=62, n_cls=16, h=600, w=1000):
    """frames + per-frame annotation dicts (keys ``f0..``) + im_info."""
    im, info = syn.frames(seed, n_frames, h, w)
    annos = {"f%d" % i: syn.relation_annotation(seed * 1000 + i, n_boxes, n_pairs, n_rel, n_cls, h, w)
             for i in range(n_frames)}
    return im, info, annos


def sgg_head_inputs(annos, info, n_rel):
    """Head inputs of one minibatch on the host, exact sizes (faster_rcnn_SGG_emb.py:170-245 for every frame of the batch;
    frames without an annotated relation contribute nothing, :177-183): ``annos`` one annotation dict per frame (unscaled
    pixel boxes, as in the ``source_gt_rels`` pickle), ``info`` (n_frames,3) im_info rows [h, w, scale].
    -> dict of numpy arrays: boxes (nb,5), relb (np,5) [frame index in column 0], labels (np,n_rel), ixs / ixo (np,) rows of
    ``boxes``, bounds (np,2,4) integer bounds of the 32x32 dual masks, wrow (np,) = 1 / (pairs of the frame * frames with
    pairs): sum_r wrow[r] * mean_c BCE is the mean over frames of the per-frame BCE mean."""
    from .model.faster_rcnn.faster_rcnn_SGG_emb import build_pair_tables
    boxes, relb, bounds, labels, ixs, ixo, counts, off = [], [], [], [], [], [], [], 0
    for f, anno in enumerate(annos):
        if anno is None or len(anno["rels"]) < 1:
            continue
        gt, union, bnd, lab, s, o = build_pair_tables(anno, float(info[f][2]), float(info[f][0]), float(info[f][1]), n_rel)
        b5 = np.zeros((gt.shape[0], 5), np.float32); b5[:, 0] = f; b5[:, 1:] = gt
        r5 = np.zeros((union.shape[0], 5), np.float32); r5[:, 0] = f; r5[:, 1:] = union
        boxes.append(b5); relb.append(r5); bounds.append(bnd); labels.append(lab)
        ixs.append(s + off); ixo.append(o + off); counts.append(lab.shape[0]); off += gt.shape[0]
    if not counts:
        return None
    cat = np.concatenate
    return dict(boxes=cat(boxes), relb=cat(relb), labels=cat(labels).astype(np.float32), ixs=cat(ixs).astype(np.int64),
                ixo=cat(ixo).astype(np.int64), bounds=cat(bounds).astype(np.int32),
                wrow=cat([np.full((c,), 1.0 / (c * len(counts)), np.float32) for c in counts]))


def _rasterize_host(bounds, channels=4):
    """(n,2,4) integer [x1,y1,x2,y2) -> (n,channels,32,32) float32 dual masks (resnet_SGG_emb.py:246-256); channels 2.. are
    the zero pad that keeps conv_lo.0's gathers 16-byte wide."""
    n = bounds.shape[0]
    m = np.zeros((n, channels, 32, 32), np.float32)
    ar = np.arange(32)
    b = bounds.reshape(n, 2, 4, 1)
    xs = (ar[None, None, :] >= b[:, :, 0]) & (ar[None, None, :] < b[:, :, 2])          # (n,2,32)
    ys = (ar[None, None, :] >= b[:, :, 1]) & (ar[None, None, :] < b[:, :, 3])
    m[:, :2] = (ys[:, :, :, None] & xs[:, :, None, :]).astype(np.float32)
    return m


class _Slot:
    """One minibatch worth of head inputs packed into ONE device buffer (256-B aligned fields), so that moving a
    batch between pipeline stages is a single copy whatever the number of fields.  ``layout``: name -> (shape, dtype).
    ``host=True`` adds two pinned host mirrors of the same layout: a batch is assembled in one of them and crosses PCIe as
    ONE asynchronous copy."""

    def __init__(self, layout, device, host=False):
        self.layout = {k: (tuple(sh), dt) for k, (sh, dt) in layout.items()}
        self.spec, off = [], 0
        for name, (shape, dt) in self.layout.items():
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            self.spec.append((name, off, nbytes, dt, shape))
            off += (nbytes + 255) // 256 * 256
        self.nbytes = max(off, 256)
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.views = {name: self.buf[o:o + n].view(dt).view(shape) for name, o, n, dt, shape in self.spec}
        self._host, self._turn = [], 0
        if host:
            for _ in range(2):
                hb = torch.zeros(self.nbytes, dtype=torch.uint8).pin_memory()
                hv = {name: hb[o:o + n].view(dt).view(shape).numpy() for name, o, n, dt, shape in self.spec}
                self._host.append((hb, hv, torch.cuda.Event()))

    def same_layout(self, layout):
        return self.layout == {k: (tuple(sh), dt) for k, (sh, dt) in layout.items()}

    def write(self, fields):
        """Device tensors of exactly the slot's shapes (one small copy per field)."""
        for name, t in fields.items():
            self.views[name].copy_(t)

    def write_host(self, fields):
        """numpy arrays, each at most as large as its field along axis 0: zero-padded to the slot's capacity in a pinned
        mirror, then ONE asynchronous H2D copy on the current stream."""
        hb, hv, ev = self._host[self._turn]
        self._turn ^= 1
        ev.synchronize()                         # the copy that last read this mirror has finished (two calls ago)
        for name, a in fields.items():
            dst = hv[name]
            n = a.shape[0] if a.ndim else 0
            if a.ndim and n > dst.shape[0]:
                raise ValueError("field %s: %d rows exceed the slot's capacity %d" % (name, n, dst.shape[0]))
            if a.ndim:
                dst[:n] = a
                dst[n:] = 0
            else:
                dst[...] = a
        self.buf.copy_(hb, non_blocking=True)
        ev.record()


class _Uploader:
    """Host frames -> device on the process's COPY stream (launch.role_stream), two staging buffers and event edges both ways: the
    transfer of minibatch k+1 runs beside the step that is still computing (a 2 x 3 x 600 x 1000 fp32 minibatch is 14.4 MB;
    bench.py --data loader over four alternating frame sizes: 5.00 -> 4.82 ms per step, uint8 frames 4.83 -> 4.77).
    ``I2V_UPLOAD_STREAM=0``: the transfer on the caller's stream, in front of the step (the default of round 3, which had met
    a host segfault in hipGraphLaunch with the copy stream and blamed stream aliasing).  The same file order with pooled
    streams and every alias logged -- the copy stream WAS a captured branch, the side stream WAS torch's capture stream --
    neither crashes (profiles/r04_alias_repro.txt; that record stopped on a bookkeeping KeyError of the test before the numeric
    comparison) nor changes a loss or a weight (profiles/r05_alias_repro.txt: run to the end, 18 passed) once no graph is
    dropped while a replay of it may be in flight (``invalidate_graphs`` synchronises first; stage() grew the head capacity
    and dropped every graph right behind an asynchronous replay).  The aliases cost the overlap, not correctness; they are gone too (launch.role_stream),
    and tests/test_gpu_data_layer.py runs the loader loop both ways, in the order that crashed.
    ``upload`` returns a device tensor that is valid on the caller's CURRENT stream, ``consumed`` marks the point after which
    its buffer may be overwritten."""

    def __init__(self, device):
        self.dev = torch.device(device)
        # Normal priority.  Measured (tools/loader_probe.py, relation step, 14.4 MB of frames per step): the transfer costs the
        # step 0.35-0.4 ms although it is queued a step ahead on its own stream -- it runs as a blit kernel and only gets its
        # turn when the step's branches drain.  A HIGH-priority copy stream (I2V_UPLOAD_PRIORITY=-1) hides it when every
        # minibatch has one size (4.74 -> 4.86 ms instead of 5.15) but doubles the step (8.7-9.5 ms) as soon as the loop
        # alternates between the graphs of two sizes -- so it is not the default.
        import os
        self.enabled = os.environ.get("I2V_UPLOAD_STREAM", "1") == "1"
        # the copy stream exists only when asked for, and is the process's ONE copy stream (launch.role_stream): a handle of the
        # library's own, never an alias of a branch / capture / communicator stream out of torch's pool
        self.stream = launch.role_stream(self.dev, "copy", 0) if self.enabled else None      # normal priority: a high one doubles the step when the loop alternates between the graphs of two sizes
        self.rings = {}

    def upload(self, frames):
        if not self.enabled:                 # the transfer on the caller's stream, in front of the step (the round-2 form)
            return frames.to(self.dev, non_blocking=True), None
        return self._upload(frames)

    def _upload(self, frames):
        # ONE ring of two byte buffers for every shape: upload k+2 waits for the consumer of upload k whatever their shapes, so
        # at most two transfers are ever queued ahead of the step
        nbytes = frames.numel() * frames.element_size()
        ring = self.rings.setdefault("ring", {"i": 0, "buf": [None, None], "free": [None, None]})
        i = ring["i"]
        ring["i"] ^= 1
        cur = torch.cuda.current_stream(self.dev)
        if ring["free"][i] is not None:
            self.stream.wait_event(ring["free"][i])          # the copy that last READ this buffer (two uploads ago) is done
        with torch.cuda.stream(self.stream):
            if ring["buf"][i] is None or ring["buf"][i].numel() < nbytes:
                # allocated ON the copy stream (the caching allocator hands a block only to work ordered behind its previous
                # use on the stream it was allocated for) and known to the consumer's stream, so that a release -- growth
                # here, or the end of the step object -- waits for both
                ring["buf"][i] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=self.dev)
            ring["buf"][i].record_stream(cur)
            dst = ring["buf"][i][:nbytes].view(frames.dtype).view(frames.shape)
            dst.copy_(frames, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        cur.wait_event(done)
        return dst, (ring, i)

    def consumed(self, token):
        if token is None:
            return
        ring, i = token
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        ring["free"][i] = ev


def step_uploader(step):
    """The uploader of a step object, created on first use: one per step, so the frames of one step share one ring."""
    if getattr(step, "_uploader", None) is None:
        step._uploader = _Uploader(step.dev)
    return step._uploader


def place_frames(dst, frames, owner=None):
    """A minibatch of n frames into the first n of ``dst`` (.., 4, H, W) channels_last, on the caller's stream: the (n,4,H,W)
    blob of the device front-end by a plain copy, (n,3,H,W) float frames by ONE strided copy NCHW3 -> NHWC4 (channel 3 stays
    zero).  Host frames cross PCIe through the uploader of the step ``owner`` (the copy stream, beside the running step) when
    one is given, else directly on the caller's stream (pinned memory asynchronously)."""
    n, c = frames.shape[:2]
    dst = dst[:n] if c == 4 else dst[:n, :3]
    if frames.is_cuda or owner is None:
        dst.copy_(frames, non_blocking=True)
    else:
        uploader = step_uploader(owner)
        src, token = uploader.upload(frames.float())
        dst.copy_(src)
        uploader.consumed(token)


def parse_u8_meta(meta):
    """The meta rows [flipped, canvas_h, canvas_w, scale, target] of a ``roibatchLoader(device_prep=True)`` minibatch ->
    (rows (n,5) float64, (H, W), im_info (n,3) float32 rows [H, W, scale]).  The frames of one call share their canvas
    (ValueError otherwise); (H, W) is None for a canvas <= 0, a minibatch the device front-end does not take (the square trim:
    the host form stages it)."""
    rows = np.asarray(meta.cpu() if torch.is_tensor(meta) else meta, np.float64).reshape(-1, 5)
    sizes = {(int(m[1]), int(m[2])) for m in rows}
    if len(sizes) != 1:
        raise ValueError("the frames of one call must share their resized size, got %s" % sorted(sizes))
    (H, W), = sizes
    return rows, ((H, W) if H > 0 and W > 0 else None), rows[:, 1:4].astype(np.float32)


def _place_u8(uploader, frames_u8, meta, dst):
    """The device front-end of a ``roibatchLoader(device_prep=True)`` minibatch: every decoded uint8 frame crosses PCIe as it
    is (copy stream) and ``i2v_image_prep`` writes the mean-subtracted, resized BGR image into its slot of ``dst`` (n,4,H,W)
    channels_last, which is cleared first (the canvas around an image is zero padding, roibatchLoader.py:162-181)."""
    dst.zero_()
    for f, u8 in enumerate(frames_u8):
        flipped, target = bool(meta[f][0]), int(meta[f][4])
        src, token = uploader.upload(u8.reshape(u8.shape[-3:]))          # (1,H,W,3): an item of a batch_size-1 loader
        ops.image_prep(src, cfg.PIXEL_MEANS, target, flipped=flipped, rgb=True, blob=dst[f:f + 1])
        uploader.consumed(token)
