"""The optimizers of the two reference loops on the fused HIP update kernels: SGD(momentum) and Adam with the reference's
param groups, in torch.optim's checkpoint layout."""
import torch

from . import ops, parallel
from .model.utils.config import cfg


class FusedSGD:
    """SGD(momentum) with the reference's param groups (bias: lr x2 and no weight decay when
    cfg.TRAIN.DOUBLE_BIAS / not BIAS_DECAY) on the fused HIP kernel; one launch per tensor."""

    def __init__(self, named_params, lr, momentum=None, weight_decay=None):
        T = cfg.TRAIN
        self.momentum = T.MOMENTUM if momentum is None else momentum
        wd = T.WEIGHT_DECAY if weight_decay is None else weight_decay
        self.items = []
        self._fused_keys = []
        for name, p in named_params:
            if not p.requires_grad:
                continue
            is_bias = "bias" in name
            p._i2v_trained = True        # updated through raw device pointers: caches keyed on p._version also key on ops.PARAM_EPOCH
            self.items.append(dict(
                name=name, p=p, m=torch.zeros_like(p),
                lr=lr * ((T.DOUBLE_BIAS + 1) if is_bias else 1),
                wd=(wd if T.BIAS_DECAY else 0.0) if is_bias else wd))

    def fuse_wgrad(self, min_numel=1 << 24):
        """Fuse the update of large filters into their wgrad epilogue (single-GPU only: with data
        parallelism the gradient must be all-reduced before the update).  Returns the fused names.
        (Rounds 3-5 carried a second form, ``defer``: the update applied by the NEXT forward on its pass over the filter --
        parity-tested, 1.41 ms against 0.43 + 0.79 as two kernels, never used; it left the tree in round 6, DESIGN_HISTORY.md 5.6.)"""
        names = []
        for it in self.items:
            p = it["p"]
            if parallel.exchange_enabled() and not parallel.is_local(p):
                continue              # its gradient has to cross the ranks first
            if p.dim() >= 2 and p.numel() >= min_numel:
                # keyed by storage pointer (what the autograd node sees); ``owner`` says whose entry it is -- a pointer is
                # reused by the allocator, and an optimizer that is collected late must not remove (or act on) the entry a
                # newer optimizer made for a new filter at the same address
                ops.FUSED_SGD[p.data_ptr()] = ops.FusedEntry(it["m"], it["lr"], self.momentum, it["wd"], self)
                self._fused_keys.append(p.data_ptr())
                names.append(it["name"])
        return names

    def _mine(self, table, k):
        ent = table.get(k)
        return ent if ent is not None and getattr(ent, "owner", None) is self else None

    def flush_pending(self):
        """Nothing is pending: every update is applied inside the step (rounds 3-5 had a deferred form for fc6 / fc7; callers that
        read filters outside the step keep calling this)."""

    def unfuse(self):
        for k in self._fused_keys:
            if self._mine(ops.FUSED_SGD, k) is not None:      # not an entry a newer optimizer made at a reused address
                del ops.FUSED_SGD[k]
        self._fused_keys = []

    def __del__(self):
        try:
            self.unfuse()
        except Exception:
            pass

    def params(self):
        return [it["p"] for it in self.items]

    def state_tensors(self):
        """Every tensor of the optimizer's own state (a step object snapshots / restores them around warm-up steps)."""
        return [it["m"] for it in self.items]

    @staticmethod
    def bump():
        """The parameters changed (an eager ``step()``, a fused wgrad+SGD epilogue or a graph replay that contains
        them): whatever is derived from trained parameters and cached (Winograd-domain filters) is stale."""
        ops.PARAM_EPOCH += 1

    def state_dict(self):
        """torch.optim.SGD's layout (param_groups + state[i]['momentum_buffer']) in named_parameters order, so that a
        checkpoint written here resumes under torch.optim.SGD and vice versa."""
        return {"state": {i: {"momentum_buffer": it["m"].detach().clone()} for i, it in enumerate(self.items)},
                "param_groups": [{"lr": it["lr"], "momentum": self.momentum, "weight_decay": it["wd"], "params": [i],
                                  "name": it["name"]} for i, it in enumerate(self.items)]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        flat = [pi for g in groups for pi in g["params"]]
        if len(flat) != len(self.items):
            raise ValueError("optimizer state holds %d parameters, this optimizer %d" % (len(flat), len(self.items)))
        by_param = {pi: g for g in groups for pi in g["params"]}
        for i, it in enumerate(self.items):
            g = by_param[flat[i]]
            it["lr"], it["wd"] = float(g["lr"]), float(g.get("weight_decay", it["wd"]))
            self.momentum = float(g.get("momentum", self.momentum))
            st = sd["state"].get(flat[i], sd["state"].get(str(flat[i])))
            if st is not None and st.get("momentum_buffer") is not None:
                it["m"].copy_(st["momentum_buffer"].reshape(it["m"].shape))
            else:
                it["m"].zero_()
        for k in list(self._fused_keys):       # fused entries hold (momentum, lr, ...) by value
            for it in self.items:
                if it["p"].data_ptr() == k and self._mine(ops.FUSED_SGD, k) is not None:
                    ops.FUSED_SGD[k] = ops.FusedEntry(it["m"], it["lr"], self.momentum, it["wd"], self)

    def zero_grad(self):
        for it in self.items:
            it["p"].grad = None

    def lr_of(self, name):
        """The learning rate the optimizer holds for parameter ``name`` (what a resumed run shows and decays from)."""
        for it in self.items:
            if it["name"] == name:
                return it["lr"]
        return self.items[0]["lr"]

    def scale_lr(self, k):
        for it in self.items:
            it["lr"] *= k
            ent = self._mine(ops.FUSED_SGD, it["p"].data_ptr())
            if ent is not None:                 # fused entries hold the rate by value (a captured graph holds it too:
                ops.FUSED_SGD[it["p"].data_ptr()] = ops.FusedEntry(ent[0], it["lr"], ent[2], ent[3], self)   # re-capture after a decay)

    MULTI_BELOW = 1 << 20       # tensors under 1 Mi elements share one launch

    @torch.no_grad()
    def step(self):
        small = []
        for it in self.items:
            p, g = it["p"], it["p"].grad
            if g is None:
                continue
            if g.stride() != p.stride() and not _same_memory_order(p, g):
                g = torch.empty_like(p).copy_(g)
            if p.numel() < self.MULTI_BELOW:
                small.append((p, g, it))
            else:
                ops.sgd_momentum_(p, g, it["m"], it["lr"], self.momentum, it["wd"])
        if small:
            ops.sgd_momentum_multi_([p for p, _, _ in small], [g for _, g, _ in small], [it["m"] for _, _, it in small],
                                    [it["lr"] for _, _, it in small], [it["wd"] for _, _, it in small], self.momentum)
        self.bump()


class FusedAdam(FusedSGD):
    """torch.optim.Adam with the reference's param groups (``--o adam``: trainval_net_instance_styleD_bilinear.py:143-145,
    trainval_net_SGG_emb.py:146-147) on ``i2v_adam_multi``: same interface as ``FusedSGD`` towards the step objects, no fusion
    into the filter-gradient kernels (the second-moment update needs the finished gradient).  The step count sits in device
    memory, so a captured step replays with the right bias corrections; ``state_dict`` is torch.optim.Adam's layout."""

    def __init__(self, named_params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=None):
        super().__init__(named_params, lr, momentum=0.0, weight_decay=weight_decay)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        for it in self.items:
            it["v"] = torch.zeros_like(it["p"])
        dev = self.items[0]["p"].device if self.items else "cpu"
        self.t = torch.zeros(1, dtype=torch.int32, device=dev)

    def fuse_wgrad(self, min_numel=1 << 24):
        return []

    def state_tensors(self):
        return [it["m"] for it in self.items] + [it["v"] for it in self.items] + [self.t]

    def state_dict(self):
        # torch.optim.Adam holds state only for parameters that have received a gradient (round-3 advice); its per-parameter
        # ``step`` is one shared device counter here -- every trained parameter of the two reference models gets a gradient
        # every step, so the two agree
        step = float(self.t.item())
        return {"state": {i: {"step": torch.tensor(step), "exp_avg": it["m"].detach().clone(), "exp_avg_sq": it["v"].detach().clone()}
                          for i, it in enumerate(self.items) if it.get("seen")},
                "param_groups": [{"lr": it["lr"], "betas": self.betas, "eps": self.eps, "weight_decay": it["wd"], "amsgrad": False,
                                  "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                                  "params": [i], "name": it["name"]} for i, it in enumerate(self.items)]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        flat = [pi for g in groups for pi in g["params"]]
        if len(flat) != len(self.items):
            raise ValueError("optimizer state holds %d parameters, this optimizer %d" % (len(flat), len(self.items)))
        by_param = {pi: g for g in groups for pi in g["params"]}
        step = 0.0
        for i, it in enumerate(self.items):
            g = by_param[flat[i]]
            it["lr"], it["wd"] = float(g["lr"]), float(g.get("weight_decay", it["wd"]))
            self.betas, self.eps = tuple(float(b) for b in g.get("betas", self.betas)), float(g.get("eps", self.eps))
            st = sd["state"].get(flat[i], sd["state"].get(str(flat[i])))
            if st is not None and st.get("exp_avg") is not None:
                it["m"].copy_(st["exp_avg"].reshape(it["m"].shape))
                it["v"].copy_(st["exp_avg_sq"].reshape(it["v"].shape))
                step = max(step, float(st.get("step", 0.0)))
                it["seen"] = True
            else:
                it["m"].zero_()
                it["v"].zero_()
                it["seen"] = False
        self.t.fill_(int(step))

    def scale_lr(self, k):
        for it in self.items:
            it["lr"] *= k

    @torch.no_grad()
    def step(self):
        live = []
        for it in self.items:
            p, g = it["p"], it["p"].grad
            if g is None:                        # torch.optim.Adam skips parameters without a gradient
                continue
            if g.stride() != p.stride() and not _same_memory_order(p, g):
                g = torch.empty_like(p).copy_(g)
            it["seen"] = True
            live.append((p, g, it))
        if not live:
            return
        ops.adam_step_(self.t)
        ops.adam_multi_([p for p, _, _ in live], [g for _, g, _ in live], [it["m"] for _, _, it in live],
                        [it["v"] for _, _, it in live], [it["lr"] for _, _, it in live], [it["wd"] for _, _, it in live],
                        self.betas, self.eps, self.t)
        self.bump()


def make_optimizer(kind, named_params, lr):
    """``--o sgd | adam`` of the reference loops."""
    if kind == "sgd":
        return FusedSGD(named_params, lr)
    if kind == "adam":
        return FusedAdam(named_params, lr)
    raise ValueError("optimizer %r: the reference loops know 'sgd' and 'adam'" % (kind,))


def _same_memory_order(p, g):
    """Two dense tensors of one shape whose strides agree on every axis longer than 1 hold their elements in the same order
    in memory (a (Cout,Cin,1,1) filter gradient in channels_last strides against the parameter's plain strides): the flat
    update kernels may read both as they are.  Without this every 1x1 filter gradient of the trunk was copied once per step
    (45 launches, 0.2 ms of the instance_styleD step: tools/glue_trace.py)."""
    if p.shape != g.shape or p.numel() != g.numel():
        return False
    for n, sp, sg in zip(p.shape, p.stride(), g.stride()):
        if n > 1 and sp != sg:
            return False
    dense = lambda t: t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))
    return dense(p) and dense(g)
