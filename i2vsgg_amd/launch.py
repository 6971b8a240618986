"""Which buffers and which stream a launch may touch.

Launches that share a scratch buffer, a split-K workspace or a pre-zeroed arena must be ordered on the device.  So there is
always ONE current ``LaunchContext`` that owns the three, and the wrappers in ``ops`` ask it for them (``arena``,
``split_buffer``, ``split_args``, ``workspace``): the innermost context a step object has entered (``with ctx:``), else the
launch stream's own default context; ``SideBranch.run`` enters a child of the context current at its fork.  The streams such
pieces of work run on come from ``role_stream`` and are forked and joined through ``branch`` / ``join``."""
import ctypes
import os

import torch

from . import _lib
from ._lib import check, lib, ptr, stream


class ZeroArena:
    """Pre-zeroed output arena for the split-K convolutions of one step: ONE clear per step instead of one
    hipMemsetAsync per launch (~70 per SGG_emb step).  ``reset()`` at the top of a step clears the prefix used
    last step and rewinds; ``take()`` hands out channels_last tensors.  When it runs out it reports the size
    it would have needed (``wanted``) and the conv falls back to clearing its own output."""

    def __init__(self, nbytes, device):
        self.buf = torch.zeros(max(int(nbytes), 1024) // 4, dtype=torch.float32, device=device)
        self.off = self.used = self.wanted = 0

    def reset(self):
        # while a graph is being captured the clear must cover everything the captured step will take, whatever the
        # eager steps before it used (an arena that was just re-sized has used == 0: a captured step without a clear
        # node would accumulate into its own outputs of the previous replay)
        n = self.buf.numel() if torch.cuda.is_current_stream_capturing() else self.used
        if n:
            self.buf[:n].zero_()
        self.off = self.wanted = 0

    def take(self, B, C, H, W):
        n = B * C * H * W
        n_al = (n + 63) // 64 * 64
        self.wanted += n_al
        if self.off + n_al > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n].view(B, H, W, C).permute(0, 3, 1, 2)
        self.off += n_al
        self.used = max(self.used, self.off)
        return t

    def take_flat(self, n):
        """n zeros, contiguous (bias-gradient sums, small filter gradients that are accumulated atomically)."""
        n_al = (n + 63) // 64 * 64
        self.wanted += n_al
        if self.off + n_al > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n]
        self.off += n_al
        self.used = max(self.used, self.off)
        return t


class SplitWorkspace:
    """Caller-owned split-K scratch of the implicit-GEMM kernels (include/i2vsgg_hip.h, i2v_conv_fwd): arrival counters
    (zero between launches) + a slab of partial tiles, and what the ordered cross-workgroup sums (bias column sums, split
    filter gradients) go through.  One per ``LaunchContext``."""
    BYTES = (48 << 20) + 4096

    def __init__(self, device, nbytes=None):
        self.buf = torch.zeros(int(nbytes or self.BYTES), dtype=torch.uint8, device=device)


_TUNE_SPLIT_ATOMICS = 4                 # include/i2vsgg_hip.h I2V_TUNE_SPLIT_ATOMICS
ORDERED_SUMS = os.environ.get("I2V_ORDERED_SUMS", "1") != "0"     # 0: LaunchContext(ordered=True) is ignored (A/B of its cost)
_ENTERED = []           # the contexts entered and not yet left, innermost last (process-wide: autograd's threads see it too)
_DEFAULTS = {}          # (device index, stream handle) -> the context of launches made with none entered


class LaunchContext:
    """What one independently scheduled piece of work owns exclusively: the pre-zeroed arena of its atomically accumulated
    outputs, its split-K workspace and its tagged scratch buffers.  ``with ctx:`` makes it the current context for the calls
    made inside (forward AND the autograd backward triggered inside the block); leaving restores the one around it."""

    def __init__(self, device, arena=True, ordered=False, lazy_split=False):
        self.device = torch.device(device)
        self.arena = ZeroArena(1024, self.device) if arena else None      # sized after the first eager step (fit())
        # lazy_split (default and side contexts): the slab is allocated by the first launch that asks for it
        self.split = None if lazy_split else SplitWorkspace(self.device)
        self.scratch = {}
        # ordered: every reduction the launches of this context split across workgroups -- split-K GEMMs of any split count,
        # small filter gradients, bias column sums -- is summed in a fixed order through ``split`` (I2V_TUNE_SPLIT_ATOMICS = 0
        # while the context is entered): bit-reproducible results.  The relation step's head asks for it (free there); the
        # instance_styleD step does not (+4 % of its step: DESIGN.md 5.10)
        self.ordered = bool(ordered)
        self.borrows_arena, self._side = False, None

    def fit(self):
        """After an eager step: re-size the arena to what the step asked for."""
        a = self.arena
        if a is not None and a.wanted * 4 > a.buf.numel() * 4:
            self.arena = ZeroArena(int(a.wanted * 4 * 1.05) + 4096, self.device)

    def side(self):
        """The context of a side branch forked under this one (created once): the SAME arena, taken from without a reset, a
        split workspace and scratch buffers of its own.  (It holds no reference to this one: both go with the step.)"""
        if self._side is None:
            self._side = LaunchContext(self.device, arena=False, lazy_split=True)
            self._side.borrows_arena = True
        self._side.arena = self.arena       # whatever fit() has made of it; this context's entry cleared it
        return self._side

    def __enter__(self):
        self._tune = None
        if self.ordered and ORDERED_SUMS:
            self._tune = lib.i2v_get_tuning(_TUNE_SPLIT_ATOMICS)
            if self._tune == 2:             # an explicit I2V_SPLIT_ATOMICS=1 (always atomics) is the user's to keep
                lib.i2v_set_tuning(_TUNE_SPLIT_ATOMICS, 0)
        if self.arena is not None and not self.borrows_arena:
            self.arena.reset()          # one clear for every atomically accumulated output of this piece of work
        _ENTERED.append(self)
        return self

    def __exit__(self, *exc):
        _ENTERED.pop()
        if self._tune == 2:
            lib.i2v_set_tuning(_TUNE_SPLIT_ATOMICS, 2)
        return False


def current(device=None):
    """The context in force: the innermost one entered, else the default context of the launch stream (torch's current stream)
    on ``device``: two streams never share a buffer by default either."""
    if _ENTERED:
        return _ENTERED[-1]
    index = device.index if device is not None and device.index is not None else torch.cuda.current_device()
    key = (index, stream())
    ctx = _DEFAULTS.get(key)
    if ctx is None:
        ctx = _DEFAULTS[key] = LaunchContext(torch.device("cuda", index), arena=False, lazy_split=True)
    return ctx


def arena():
    """The current context's ``ZeroArena``, or None when it has none (the caller then clears its own output)."""
    return current().arena


def split_buffer(device):
    """The current context's split-K workspace (a uint8 tensor)."""
    ctx = current(device)
    if ctx.split is None:
        ctx.split = SplitWorkspace(ctx.device)
    return ctx.split.buf


def split_args(device=None):
    """(pointer, bytes) of ``split_buffer``: what the ordered cross-workgroup sums take next to the split-K GEMMs."""
    t = split_buffer(device)
    return ptr(t), t.numel()


def workspace(nbytes, device, tag="default"):
    """Grow-only scratch buffer per tag of the current context."""
    cache = current(device).scratch
    buf = cache.get(tag)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        cache[tag] = buf
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# Streams.  ``torch.cuda.Stream()`` does not create a stream: it deals the next of 32 pooled streams per device and priority,
# round robin -- and torch.cuda.graph's capture stream, ProcessGroupNCCL's streams and every caller's own streams come out of the
# same pool.  A process that has built a few step objects therefore holds "different" stream objects with the SAME handle, and
# a fork onto an alias of the forking stream (or of a sibling branch) is no fork at all.  The step objects take their streams
# from this registry instead: one HIP stream per (device, role), created ONCE per process by the library
# (``i2v_stream_create``: hipStreamCreateWithPriority, non-blocking), wrapped as a ``torch.cuda.ExternalStream`` and never
# destroyed.  Such a handle cannot come out of torch's pool, two roles never share one, and step objects built one after the
# other reuse the same few streams (a stream is an ordered queue: sharing a role between objects that run one after the other
# costs nothing).
_ROLE_STREAMS = {}
STREAM_REQUESTS = []    # every request in order (capped): with torch.cuda.Stream() each of them drew the next pooled handle


def role_stream(device, role, priority=0):
    """The process-wide stream of ``role`` (any hashable: "side", ("frame", 0), "copy", ...) on ``device``."""
    dev = torch.device(device)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (index, role, int(priority))
    if len(STREAM_REQUESTS) < 4096:
        STREAM_REQUESTS.append(role)
    st = _ROLE_STREAMS.get(key)
    if st is None:
        torch.cuda.init()
        out = ctypes.c_void_p()
        check(lib.i2v_stream_create(index, int(priority), ctypes.byref(out)), "i2v_stream_create")
        taken = {t.cuda_stream for t in _ROLE_STREAMS.values()}
        if not out.value or out.value in taken:
            raise _lib.I2VError("role_stream: the runtime handed out stream handle %r twice" % out.value)
        st = _ROLE_STREAMS[key] = torch.cuda.ExternalStream(out.value, device=torch.device("cuda", index))
    return st


def stream_table():
    """{(device, role, priority): handle} of every stream the registry has created (tools/stream_handles.py, tests)."""
    return {k: v.cuda_stream for k, v in _ROLE_STREAMS.items()}


_BRANCH_DEPTH = 0
_FORKED = {}            # handle -> origin handle of every branch forked and not yet joined (join)


def open_branches():
    """{branch handle: origin handle} of every branch forked and not yet joined (a copy: tools)."""
    return dict(_FORKED)


class branch:
    """``with launch.branch(stream, origin):`` -- the body runs on ``stream`` as a fork of ``origin`` (stream.wait_stream(origin)
    first; the caller joins with ``launch.join(origin, stream, ...)``).  The step objects fork their graph branches through this
    so that the capture-time failures the schedule must avoid are error messages instead:
      * a fork made INSIDE a forked branch ends ``hipStreamEndCapture`` in a host segfault on ROCm 7.2 -- every
        branch forks from the capturing stream itself;
      * a branch stream whose HANDLE equals the origin's, or that of a sibling branch still open, is not a branch (the work is
        silently serialised, and events recorded "between" the two are edges of a stream onto itself)."""

    def __init__(self, stream, origin):
        self.stream, self.origin = stream, origin

    def refuse(self, h, ho):
        """Raise on a fork the schedule must avoid (a tool that studies such forks overrides this)."""
        if _BRANCH_DEPTH > 0 and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("launch.branch: a fork inside a forked graph branch (hipStreamEndCapture crashes on it): fork every "
                               "branch from the capturing stream")
        if h == ho:
            raise RuntimeError("launch.branch: the branch stream IS the forking stream (handle %#x): take branch streams from "
                               "launch.role_stream, torch.cuda.Stream() deals pooled handles round robin" % h)
        if h in _FORKED:
            raise RuntimeError("launch.branch: stream %#x is already an open branch (a sibling's alias?); join it first" % h)

    def __enter__(self):
        global _BRANCH_DEPTH
        h, ho = self.stream.cuda_stream, self.origin.cuda_stream
        self.refuse(h, ho)
        self.stream.wait_stream(self.origin)
        self._ctx = torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        _FORKED[h] = ho
        _BRANCH_DEPTH += 1
        return self

    def __exit__(self, *exc):
        global _BRANCH_DEPTH
        _BRANCH_DEPTH -= 1
        if exc and exc[0] is not None:
            _FORKED.pop(self.stream.cuda_stream, None)       # a failed body: whoever handles the error owns the clean-up
        return self._ctx.__exit__(*exc)


def reset_branches():
    """After a failed capture: forget the branches it left open."""
    global _BRANCH_DEPTH
    _FORKED.clear()
    _BRANCH_DEPTH = 0


def join(origin, *streams):
    """``origin`` waits for every branch in ``streams`` (the join of ``branch``)."""
    for st in streams:
        origin.wait_stream(st)
        _FORKED.pop(st.cuda_stream, None)


class SideBranch:
    """The filter-gradient side branch of a step (train.InstanceStyleDStep.wgrad_branch): nothing in the backward depends on the
    block nodes' filter gradients, so they can fill the chip beside the data-gradient chain.  One edge per ``run``, one ``join``
    before the gradient exchange.  A run's launches are made under ``LaunchContext.side()`` of the context current at the fork:
    they never share a workspace with the chain they run beside.  The tensors a run reads are kept referenced until the join:
    in a captured step a block freed on the main branch would otherwise be reused there while the side branch still reads it."""

    def __init__(self, stream):
        self.stream = stream
        self.kept = []

    def run(self, fn, *keep):
        """``fn()`` on the side stream, behind the current stream's work so far; ``keep``: the tensors it reads."""
        ctx = current().side()
        self.stream.wait_stream(torch.cuda.current_stream())
        self.kept.append(keep)
        with torch.cuda.stream(self.stream), ctx:
            return fn()

    def join(self):
        """Called by the step after backward(): the current (capturing) stream waits for the side stream."""
        cur = torch.cuda.current_stream()
        if self.stream.cuda_stream == cur.cuda_stream:
            raise RuntimeError("SideBranch.join: the filter-gradient stream is the current stream")
        cur.wait_stream(self.stream)
        self.kept.clear()


WGRAD_BRANCH = None     # the SideBranch a step has set around its backward(), else None: filter gradients on the launch stream
