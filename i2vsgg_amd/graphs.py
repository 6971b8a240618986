"""HIP-graph plumbing of the step objects: replaying a graph on the caller's stream, and the ONE copy of the code that warms a
step up, records it into a graph, keeps a bounded set of graphs in one memory pool and puts the training state back.
A graph holder (``train._FrameSet``, ``train._DomainSet``) carries ``graph`` (None: not captured yet; False: capture failed,
eager launches; else the graph), ``tick`` (its last use) and ``drop_graphs()``."""
import gc

import torch

from . import launch, parallel


_REPLAY_STREAMS = {}
REDIRECT_DEFAULT_STREAM = True      # nothing in the tree switches this off; a probe of the runtime's own default-stream path may


def replay_graph(graph, device=None):
    """``graph.replay()`` on the caller's current stream -- except on the LEGACY DEFAULT stream, where the replay runs on a
    private stream between two event edges (the caller's stream order is kept).  ROCm 7.2's HIP runtime replays a graph through
    pre-built AQL packet batches (``DEBUG_CLR_GRAPH_PACKET_CAPTURE``, on by default); on the legacy default stream that path loses
    the order between a graph's nodes and the stream's other work while a second stream is busy (losses
    off by 2e-2 from the second step on, NaN weights; the same graphs are correct on any created stream).
    i2vsgg_amd/__init__.py switches the path off before the runtime initialises WHEN IT CAN -- but what the runtime actually
    read cannot be told from os.environ (``torch.cuda.is_available()`` / ``device_count()`` bring the runtime up without setting
    ``torch.cuda.is_initialized()``; a script may set the variable after its first HIP call), so the variable is not trusted
    as proof (round-3 advice): every replay asked for on the default stream is redirected.  Cost: two event edges per step."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    cur = torch.cuda.current_stream(dev)
    if not REDIRECT_DEFAULT_STREAM or cur.cuda_stream != torch.cuda.default_stream(dev).cuda_stream:
        graph.replay()
        return
    s = _REPLAY_STREAMS.get(dev.index)
    if s is None:
        s = _REPLAY_STREAMS[dev.index] = launch.role_stream(dev, "replay")
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        graph.replay()
    cur.wait_stream(s)


class GraphRecorder:
    """Owner of one graph memory pool (``_pool``, None until the first recording; the graphs of one owner never run at the
    same time, so they share it) on device ``dev``; ``graph_error`` holds the reason of the last failed recording."""

    def _record_graph(self, body):
        """Record ``body()`` on the current stream into a new graph of the owner's pool -> the graph, or False (``graph_error``
        says why; the open branches are closed and the device is idle again).  The device is idle when the recording starts
        and, with a process group, the watchdog's work list is empty (``parallel.wait_for_collectives``)."""
        try:
            g = torch.cuda.CUDAGraph()
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            torch.cuda.synchronize(self.dev)
            parallel.wait_for_collectives(self.dev)
            with torch.cuda.graph(g, pool=self._pool, **parallel.capture_kwargs()):
                body()
            return g
        except Exception as e:      # report; the caller keeps the eager form
            self.graph_error = repr(e)
            launch.reset_branches()
            torch.cuda.synchronize(self.dev)
            return False


class CapturedStep(GraphRecorder):
    """A training step that can be recorded into HIP graphs.  The subclass provides ``dev``, ``opt``, ``max_graphs``,
    ``_graph_holders()`` (every object of the step that holds graphs) and ``_step()`` (one step on the caller's stream)."""

    def _snapshot(self):
        """Parameters, optimizer state and the device's RNG state, as ``_restore`` takes them."""
        state = [it["p"].data for it in self.opt.items] + self.opt.state_tensors()
        return (state, [t.clone() for t in state], torch.cuda.get_rng_state(self.dev))

    def _restore(self, saved):
        torch.cuda.synchronize(self.dev)
        with torch.no_grad():
            for t, sv in zip(saved[0], saved[1]):
                t.copy_(sv)
        torch.cuda.set_rng_state(saved[2], self.dev)
        self.opt.bump()

    def invalidate_graphs(self):
        """Drop every captured graph (a learning-rate change -- rates live in the captured kernel arguments --, a capacity
        change, new buffers behind captured addresses).  They are captured again on first use."""
        holders = list(self._graph_holders())
        dropped = any(h.graph for h in holders)
        if dropped:
            torch.cuda.synchronize(self.dev)      # a replay may still be running: its executable graph goes only after it
        for h in holders:
            h.drop_graphs()
        if dropped:
            gc.collect()
            torch.cuda.synchronize(self.dev)
        self._pool = None             # the allocator releases a pool with its last graph: the next capture opens a new one

    def _evict_lru(self, live):
        """Make room for one more graph.  ``live``: a (holder, slot) per graph kept -- slot None for ``holder.graph``, else a
        key of ``holder.graphs``.  At ``max_graphs`` the one whose holder was used longest ago (``tick``) goes, after whatever
        is still running; -> its holder, or None when there was room."""
        if len(live) < self.max_graphs:
            return None
        torch.cuda.synchronize(self.dev)
        holder, slot = min(live, key=lambda hs: hs[0].tick)
        if slot is None:
            holder.graph = None
        else:
            holder.graphs[slot] = None
        return holder

    def _warm_up(self, n, body, after_first):
        """``n`` eager ``body()`` calls on the "warmup" role stream, ordered behind the caller's stream and joined back into it;
        ``after_first()`` right behind the first one (arenas are sized by what it launched); the device is idle afterwards."""
        cur = torch.cuda.current_stream(self.dev)
        s = launch.role_stream(self.dev, "warmup")
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            for i in range(n):
                body()
                if i == 0:
                    after_first()
        cur.wait_stream(s)
        torch.cuda.synchronize(self.dev)

    def __call__(self):
        """One step on the caller's current stream (any stream, the legacy default stream included: see ``replay_graph``)."""
        try:
            return self._step()
        except BaseException:
            # an eager body that raised between a branch and its join leaves process-wide role streams marked open
            # (launch.open_branches()): every later step object on this device would be refused its branches
            launch.reset_branches()
            raise
