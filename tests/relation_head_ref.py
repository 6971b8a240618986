"""A float64 reference of one relation-head training step (no tests here): a hand-planted head-only batch, the conditioning
that moves every ReLU decision of the reference away from zero, and the step -- loss, all gradients, SGD(momentum) update --
written out in float64 on the CPU.  The forward is ``oracle.nets.vrd_head(dtype=float64)``; nothing here imports a kernel,
``i2vsgg_amd.ops`` or ``i2vsgg_amd.optim``: the param-group rules are written out again from ``cfg.TRAIN``."""
import numpy as np
import torch
import torch.nn.functional as F

from i2vsgg_amd import synthetic as syn
from i2vsgg_amd.model.utils.config import cfg
from oracle import nets

N_REL = 62
IM_H, IM_W = 192, 320                  # a 12 x 20 C4 map
N_BOXES, N_PAIRS = (5, 6), (7, 8)      # per frame: 11 + 15 = 26 rows through fc6 / fc7, a multiple of no tile
SEED = 0                               # the committed seed: ``condition`` meets its two conditions on it, every variant
VARIANTS = {"default": (True, 2), "nov_s2": (False, 2), "ov_s1": (True, 1), "ov_s0": (True, 0)}

# the ReLU / LeakyReLU layers in forward order (the keys ``oracle.nets.vrd_head`` fills ``taps`` with)
RELU_LAYERS = ("fc6", "fc7", "fc8", "fc_so", "conv_lo.0", "conv_lo.1", "conv_lo.2", "fc_lov", "fc_fusion", "prd_sem_embeddings.0")
MAX_MOVED, MAX_ROUNDS = 256, 12


def bias_key(layer):
    return "vrd.%s.%s" % (layer, "bias" if layer.startswith("prd_sem") else ("conv.bias" if layer.startswith("conv_lo") else "fc.bias"))


# ---------------------------------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------------------------------
def make_batch(seed=SEED):
    """Two frames of 192 x 320 with 5 / 6 boxes and 7 / 8 pairs; no backbone: the feature map is |N(0, 1)|.
    Planted by hand (global row numbers): box 1 is smaller than one feature cell, box 2 touches the right and lower image
    border, box 10 is referred to by no pair, box 0 is the subject of pairs 0, 1 and the object of pairs 2, 3; pair 2 has no
    positive label, pair 9 has three; the subject mask of pair 5 is all zeros."""
    rng = np.random.default_rng(seed)
    fmap = np.abs(rng.standard_normal((2, 1024, IM_H // 16, IM_W // 16))).astype(np.float32)
    boxes = np.zeros((sum(N_BOXES), 5), np.float32)
    row = 0
    for f, n in enumerate(N_BOXES):
        x1, y1 = rng.uniform(0, IM_W - 64, n), rng.uniform(0, IM_H - 64, n)
        bw, bh = rng.uniform(24, 200, n), rng.uniform(24, 150, n)
        boxes[row:row + n, 0] = f
        boxes[row:row + n, 1:] = np.floor(np.stack([x1, y1, np.minimum(x1 + bw, IM_W - 1), np.minimum(y1 + bh, IM_H - 1)], 1))
        row += n
    boxes[1, 1:] = (100, 50, 108, 57)                       # 8 x 7 px: inside one 16 px cell
    boxes[2, 1:] = (250, 100, IM_W - 1, IM_H - 1)           # on the border
    pairs = [[(0, 1), (0, 2), (3, 0), (4, 0), (1, 2), (2, 3), (4, 1)],
             [(0, 1), (1, 0), (2, 3), (3, 4), (4, 2), (0, 4), (1, 3), (2, 0)]]          # frame 1's box 5 (row 10): nobody's
    ixs, ixo, relb, masks, relloc, wrow, off = [], [], [], [], [], [], 0
    for f, pp in enumerate(pairs):
        assert len(pp) == N_PAIRS[f]
        for s, o in pp:
            sb, ob = boxes[off + s, 1:], boxes[off + o, 1:]
            ixs.append(off + s)
            ixo.append(off + o)
            relb.append([f] + nets.union_box(sb, ob, IM_H, IM_W))
            masks.append([nets.dual_mask(IM_H, IM_W, sb), nets.dual_mask(IM_H, IM_W, ob)])
            relloc.append(nets.relative_loc(sb, ob))
            wrow.append(1.0 / (len(pairs) * len(pp)))       # SGGEmbStep's wrow for frames of unequal pair counts
        off += N_BOXES[f]
    masks = np.asarray(masks, np.float32)
    masks[5, 0] = 0
    labels = (rng.random((sum(N_PAIRS), N_REL)) < 0.05).astype(np.float32)
    labels[2] = 0
    labels[9] = 0
    labels[9, [3, 17, 40]] = 1
    return dict(fmap=fmap, boxes=boxes, relb=np.asarray(relb, np.float32), masks=masks, relloc=np.asarray(relloc, np.float32),
                ixs=np.asarray(ixs, np.int64), ixo=np.asarray(ixo, np.int64), labels=labels, wrow=np.asarray(wrow, np.float32),
                prd=syn.word_vectors(21, N_REL))


def make_params(use_obj_visual=True, spatial_type=2):
    return syn.vrd_params(13, use_obj_visual=use_obj_visual, spatial_type=spatial_type)


def as_dtype(params, dtype):
    return {k: v.detach().to(dtype).clone() for k, v in params.items()}


def forward(p, batch, dtype, taps=None, use_obj_visual=True, spatial_type=2):
    spatial = batch["relloc"] if spatial_type == 1 else batch["masks"]
    return nets.vrd_head(batch["fmap"], batch["boxes"], batch["relb"], spatial, batch["ixs"], batch["ixo"], batch["prd"], p,
                         training=True, use_obj_visual=use_obj_visual, spatial_type=spatial_type, dtype=dtype, taps=taps)


def loss_of(score, batch):
    t = torch.as_tensor(batch["labels"], dtype=score.dtype)
    w = torch.as_tensor(batch["wrow"], dtype=score.dtype)
    return (F.binary_cross_entropy_with_logits(score, t, reduction="none").mean(1) * w).sum()


# ---------------------------------------------------------------------------------------------------------------------
# conditioning
# ---------------------------------------------------------------------------------------------------------------------
def _unit_axis_max(a):
    """(units,) -> reduce a (rows, units) or (rows, channels, h, w) boolean / magnitude array over everything but the unit."""
    return a.transpose(0, 1).reshape(a.shape[1], -1)


def measure_tau(params, batch, p64=None, **variant):
    """64 x the float32 CPU reference's largest pre-activation error against float64, relative to the layer's largest |z|."""
    t32, t64 = {}, {}
    with torch.no_grad():
        forward(params, batch, torch.float32, t32, **variant)
        forward(p64 if p64 is not None else as_dtype(params, torch.float64), batch, torch.float64, t64, **variant)
    e = max(float((t32[k].double() - t64[k]).abs().max() / t64[k].abs().max()) for k in t64)
    return 64.0 * e


def condition(params, batch, tau=None, use_obj_visual=True, spatial_type=2, p64=None):
    """Move every ReLU decision of the float64 reference at least ``tau * max|z|`` away from zero by nudging biases.
    CPU and float64 only; no device result is ever looked at.  Layer by layer in forward order: while a pre-activation lies
    within the band, add ``4 * tau * max|z| * round`` to the bias of every unit / channel that owns one, and recompute.
    The nudged biases are rounded to float32 (what the device loads) before they are used.
    -> (params with new float32 bias tensors -- the weights are the same objects --, info dict: tau, moved, rounds, margin).
    ``p64``: a float64 copy of ``params`` to work on (its biases are updated in place), else one is made."""
    variant = dict(use_obj_visual=use_obj_visual, spatial_type=spatial_type)
    p64 = as_dtype(params, torch.float64) if p64 is None else p64
    if tau is None:
        tau = measure_tau(params, batch, p64, **variant)
    out = dict(params)
    moved, rounds = set(), {}
    with torch.no_grad():
        taps = {}
        forward(p64, batch, torch.float64, taps, **variant)
        for layer in [k for k in RELU_LAYERS if k in taps]:
            bk, rnd = bias_key(layer), 0
            while True:
                z = taps[layer]
                top = float(z.abs().max())
                close = _unit_axis_max(z.abs() < tau * top).any(1)
                if not bool(close.any()) or rnd >= MAX_ROUNDS:
                    break
                rnd += 1
                b = p64[bk].clone()
                b[close] += 4.0 * tau * top * rnd
                out[bk] = b.float()
                p64[bk].copy_(out[bk].double())
                moved.update((bk, int(i)) for i in torch.nonzero(close).flatten())
                taps = {}
                forward(p64, batch, torch.float64, taps, **variant)
            rounds[layer] = rnd
        margin = {k: float(z.abs().min() / z.abs().max()) for k, z in taps.items()}
    return out, dict(tau=tau, moved=len(moved), rounds=rounds, margin=margin)


def conditions_hold(info):
    """The two conditions every user of a conditioned reference asserts before it relies on it."""
    assert all(m >= info["tau"] for m in info["margin"].values()), info
    assert info["moved"] <= MAX_MOVED and max(info["rounds"].values()) <= MAX_ROUNDS, info


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------
def group_of(name, lr, wd=None):
    """(lr_k, wd_k) of the reference's param groups (trainval_net_SGG_emb.py:133-141): a bias takes the rate times
    (DOUBLE_BIAS + 1) and decays only with BIAS_DECAY."""
    T = cfg.TRAIN
    wd = T.WEIGHT_DECAY if wd is None else wd
    if "bias" in name:
        return lr * (T.DOUBLE_BIAS + 1), (wd if T.BIAS_DECAY else 0.0)
    return lr, wd


def grads(params, batch, dtype, use_obj_visual=True, spatial_type=2, convert=True):
    """loss, logits, relation feature and every gradient in ``dtype`` arithmetic (returned as they are, detached)."""
    p = {k: v.detach().to(dtype).requires_grad_() for k, v in params.items()} if convert else params
    score, feat = forward(p, batch, dtype, None, use_obj_visual, spatial_type)
    loss = loss_of(score, batch)
    loss.backward()
    g = {k: v.grad for k, v in p.items()}
    for v in p.values():
        v.grad = None
    return loss.detach(), score.detach(), feat.detach(), g


def step_ref(params, batch, m0, lr, momentum=None, wd=None, use_obj_visual=True, spatial_type=2):
    """One SGD(momentum) step in float64: g by autograd of the float64 head, m1 = momentum m0 + (g + wd_k p),
    p1 = p - lr_k m1.  ``params`` / ``m0``: name -> tensor (any float type; converted).  -> dict(loss, score, feat, g, m1, p1)."""
    momentum = cfg.TRAIN.MOMENTUM if momentum is None else momentum
    loss, score, feat, g = grads(params, batch, torch.float64, use_obj_visual, spatial_type)
    m1, p1 = {}, {}
    for k, gk in g.items():
        lr_k, wd_k = group_of(k, lr, wd)
        p = params[k].detach().double()
        m1[k] = momentum * m0[k].detach().double() + (gk + wd_k * p)
        p1[k] = p - lr_k * m1[k]
    return dict(loss=loss, score=score, feat=feat, g=g, m1=m1, p1=p1)


def momentum_like(g, seed=5):
    """Momentum buffers (float32: what an optimizer holds) drawn at the scale of the gradients: N(0, 1) x max|g_k|."""
    gen = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(v.shape, generator=gen, dtype=torch.float32) * float(v.abs().max())) for k, v in g.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """Every measure of one tensor against its float64 reference, as {name: value}:
      peak   max|got - ref| / max|ref|
      row    the largest relative L2 error of an output row (an out-feature, an output channel)
      tap    (4-d filters) the largest relative L2 error of a filter tap (ky, kx)
    and the number of reference rows / taps that are exactly zero but not exactly zero in ``got`` (``zero_rows``)."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    out = {"peak": float(d.abs().max() / ref.abs().max().clamp_min(1e-300))}
    bad = 0

    def groups(t2, d2, g2):
        n_ref = torch.linalg.vector_norm(t2, dim=1)
        live = n_ref > 0
        wrong = int((torch.linalg.vector_norm(g2[~live], dim=1) != 0).sum()) if bool((~live).any()) else 0
        e = torch.linalg.vector_norm(d2[live], dim=1) / n_ref[live]
        return (float(e.max()) if e.numel() else 0.0), wrong

    if ref.dim() >= 2:
        out["row"], w = groups(ref.reshape(ref.shape[0], -1), d.reshape(ref.shape[0], -1), got.reshape(ref.shape[0], -1))
        bad += w
    elif ref.dim() == 1:
        bad += int(((ref == 0) & (got != 0)).sum())
    if ref.dim() == 4:
        perm = lambda t: t.permute(2, 3, 0, 1).reshape(t.shape[2] * t.shape[3], -1)
        out["tap"], w = groups(perm(ref), perm(d), perm(got))
        bad += w
    out["zero_rows"] = bad
    return out
