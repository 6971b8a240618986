"""A float64 reference of the trunk ``C4Base.forward(im, tap=True)`` under GIVEN ReLU masks (no tests here), on the CPU, in plain
torch: nothing here imports a kernel or ``i2vsgg_amd``.

The forward is  stem = max_pool2d(relu(bn(conv 7x7 s2 p3 (im))), 3, 2, 0, ceil_mode=True)  (frozen: no gradient; its ReLU and its
max pick their own sides, nothing differentiates through them and a max is continuous),  feat1 = layer2(layer1(stem)),
feat = layer3(feat1).  The blocks are those of tests/bottleneck_ref.py, composed through ``chain_forward`` one block at a time with
the block's output mask handed in as all-true, so that the pre-activation p3 is in the graph and  out = p3 * mo  is applied here:
that is where the wiring of C4Base lives (who masks the gradient of whom, what is added at the tap) and where ``plant`` breaks it.
The objective is  sum(feat * g_feat) + sum(feat1 * g_feat1);  the gradient of every layer1-3 filter comes from autograd.

``plant`` plants ONE wiring error -- in the backward only, the forward values stay bit for bit -- for the host test
(tests/test_trunk_ref_host.py) that shows the bounds of tests/test_gpu_trunk.py would catch it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import bottleneck_ref as B

BLOCKS = (3, 2, 2)                                          # miniature block counts of layer1, layer2, layer3
LAYERS = ((64, 64, 1), (256, 128, 2), (512, 256, 2))        # (cin, planes, stride of the first block) of C4Base's three layers
# frames (B, H, W) -> stem 38x54 / pool 19x27 / layer2 10x14 / layer3 5x7: 4x4-tile residues 3/3, 2/2, 1/3, odd maps halved;
#                  -> stem 32x48 / pool 16x24 (the last pool window is partial) / 8x12 / 4x6: residues 0
GEOMETRIES = {"75x107": (4, 75, 107), "64x96": (4, 64, 96)}
POOL_HW = ((9, 11), (10, 12), (3, 3), (38, 54))             # the max pool alone: odd, even (partial last window), one window, the stem's
KIND_BOUND = 1e-4           # tests/test_gpu_bottleneck_bwd.py: DIRECT_REL and test_gpu_kernels.WINOGRAD_REL, the same number
E32_FACTOR = 16.0           # tests/detector_head_ref.gpu_bound: the device's other summation order and the Winograd transforms
PLANTS = ("tap_term_dropped",                   # g_feat1 is not added at layer2's output
          "tap_premasked",                      # the tap's gradient skips l2[-1]'s output mask (l2[-1] taken as pre-masked by l3[0])
          "l3_in_relu_missing_mask",            # the gradient l3[0] returns reaches l2[-1] without the mask feat1 > 0
          "l1_l2_handover_mask_dropped",        # l2[0] does not mask the gradient it hands to l1[-1]
          "middle_block_handover_dropped",      # l1[1] (in_relu AND pre-masked) does not mask the gradient it hands to l1[0]
          "halves_swapped",                     # the source and target halves of g_feat exchanged
          "l1_0_wd_from_masked_g")              # l1[0]'s projection filter gradient from a gradient that lacks the output mask


def bound(e32, kind_bound=KIND_BOUND):
    """What a device tensor is held to: the block test's bound for its kind, or 16 x the float32 CPU reference's own error under
    the same masks where a chain of seven blocks legitimately exceeds that."""
    return max(kind_bound, E32_FACTOR * e32)


def block_specs(blocks=BLOCKS):
    """[(name, cin, planes, stride, projection)] of the blocks in forward order: 'layer1.0', ..."""
    out = []
    for li, ((cin, planes, stride), n) in enumerate(zip(LAYERS, blocks)):
        out.append(("layer%d.0" % (li + 1), cin, planes, stride, True))
        out += [("layer%d.%d" % (li + 1, i), planes * 4, planes, 1, False) for i in range(1, n)]
    return out


def stem_hw(hw):
    return tuple((d + 6 - 7) // 2 + 1 for d in hw)           # 7x7 / stride 2 / pad 3


def pool_hw(hw):
    out = []
    for d in hw:                                             # 3x3 / stride 2 / pad 0 / ceil_mode: the last window starts inside
        o = -(-(d - 3) // 2) + 1
        out.append(o - 1 if (o - 1) * 2 >= d else o)
    return tuple(out)


def make_trunk(name, seed=0, blocks=BLOCKS):
    """The float32 inputs of a geometry, the same on the host and on the device: frames = randn, the stem filter (ConvParams' He
    init) and its raw BatchNorm buffers, per block the filters and raw BatchNorm buffers in bottleneck_ref.make_case's
    distributions, and four distinct upstream gradients: g[0], g[1] for the source / target half of feat, g[2], g[3] of feat1."""
    nb, H, W = GEOMETRIES[name]
    g = torch.Generator().manual_seed(7000 + 1000 * seed + sorted(GEOMETRIES).index(name))
    randn = lambda *s: torch.randn(*s, generator=g)
    rand = lambda *s: torch.rand(*s, generator=g)

    def conv(cout, cin, k):
        return randn(cout, cin, k, k) * math.sqrt(2.0 / (k * k * cout))

    def bn(c):
        return dict(weight=rand(c) + 0.5, bias=randn(c) * 0.2, running_mean=randn(c) * 0.2, running_var=rand(c) * 1.5 + 0.5)

    im = randn(nb, 3, H, W)
    stem = dict(w=conv(64, 3, 7), bn=bn(64))
    raws, hw = [], pool_hw(stem_hw((H, W)))
    for _, cin, planes, stride, proj in block_specs(blocks):
        raws.append(dict(stride=stride, w1=conv(planes, cin, 1), w2=conv(planes, planes, 3), w3=conv(planes * 4, planes, 1),
                         wd=conv(planes * 4, cin, 1) if proj else None, bn1=bn(planes), bn2=bn(planes), bn3=bn(planes * 4),
                         bnd=bn(planes * 4) if proj else None))
        hw = B.out_hw(hw, stride)
        if len(raws) == blocks[0] + blocks[1]:
            hw1 = hw
    half = nb // 2
    grads = [randn(half, LAYERS[2][1] * 4, *hw), randn(half, LAYERS[2][1] * 4, *hw),
             randn(half, LAYERS[1][1] * 4, *hw1), randn(half, LAYERS[1][1] * 4, *hw1)]
    return dict(im=im, stem=stem, blocks=raws, g=grads, counts=tuple(blocks))


def folded_stem(raw):
    s, b = B.fold(raw["bn"])
    return dict(w=raw["w"], s=s, b=b)


def _bwd(value, grad_of):
    """``value`` in the forward BIT FOR BIT (x + 0 is x), the gradient of ``grad_of`` in the backward."""
    return value.detach() + (grad_of - grad_of.detach())


def _vec(t):
    return t.view(1, -1, 1, 1)


def stem_forward(im, stem, dtype=torch.float64):
    with torch.no_grad():
        w, s, b = (stem[k].detach().to(dtype) for k in ("w", "s", "b"))
        x = F.conv2d(im.detach().to(dtype), w, None, 2, 3) * _vec(s) + _vec(b)
        return F.max_pool2d(torch.relu(x), 3, 2, 0, ceil_mode=True)


def trunk(im, stem, blocks, counts, g_feat, g_feat1, masks=None, plant=None, dtype=torch.float64):
    """im (B,3,H,W); ``stem``: dict(w, s, b) with the folded BatchNorm; ``blocks``: the layer1-3 blocks in forward order as
    bottleneck_ref.chain takes them (w1 w2 w3 wd s1 b1 .. sd bd stride); ``counts``: blocks per layer; g_feat / g_feat1: the given
    gradients of layer3's / layer2's output (source frames first); ``masks``: per block (m1, m2, mo) boolean, or None (``pre > 0``:
    the ordinary ReLU network).
    -> dict(feat, feat1, x0 = the stem's output, pre = [(p1, p2, p3)], masks = [(m1, m2, mo)], gw = [{name: gradient}]) in ``dtype``."""
    if plant is not None and plant not in PLANTS:
        raise ValueError("unknown plant %r" % (plant,))
    n1, n2 = counts[0], counts[0] + counts[1]
    assert len(blocks) == sum(counts) and counts[0] >= 3
    x0 = stem_forward(im, stem, dtype)
    params, wanted = [], []
    for i, blk in enumerate(blocks):
        p = {k: (v.detach().to(dtype) if torch.is_tensor(v) else v) for k, v in blk.items()}
        for name in B.NAMES:
            if p[name] is not None:
                p[name].requires_grad_(True)
                wanted.append((i, name, p[name]))
        params.append(p)
    if masks is None:                   # the ordinary network's own choice, from a pass of its own
        with torch.no_grad():
            _, _, masks = B.chain_forward(x0, params)
    h, pres, feat1, tap = x0, [], None, None
    for i, p in enumerate(params):
        m1, m2, mo = masks[i]
        open_masks = [(m1, m2, torch.ones_like(mo, dtype=torch.bool))]
        p3, pre, _ = B.chain_forward(h, [p], open_masks)          # the output mask all true: this is p3, in the graph
        mo_t = mo.to(dtype)
        out = p3 * mo_t
        pres.append(pre[0])
        if (plant == "l1_l2_handover_mask_dropped" and i == n1 - 1) or (plant == "middle_block_handover_dropped" and i == 0):
            out = _bwd(out, p3)
        if plant == "l1_0_wd_from_masked_g" and i == 0:
            rest, _, _ = B.chain_forward(h, [dict(p, wd=p["wd"].detach())], open_masks)
            out = _bwd(out, rest * mo_t + F.conv2d(h, p["wd"], None, p["stride"]) * _vec(p["sd"]))
        if i == n2 - 1:                 # the tap: layer3 and the objective both read feat1
            feat1 = out.detach()
            tap = _bwd(out, p3) if plant == "tap_premasked" else out
            out = _bwd(out, p3) if plant == "l3_in_relu_missing_mask" else out
        h = out
    g_feat, g_feat1 = g_feat.to(dtype), g_feat1.to(dtype)
    if plant == "halves_swapped":
        half = g_feat.shape[0] // 2
        g_feat = torch.cat([g_feat[half:], g_feat[:half]])
    objective = (h * g_feat).sum()
    if plant != "tap_term_dropped":
        objective = objective + (tap * g_feat1).sum()
    grads = torch.autograd.grad(objective, [w for _, _, w in wanted])
    gw = [dict.fromkeys(B.NAMES) for _ in blocks]
    for (i, name, _), g in zip(wanted, grads):
        gw[i][name] = g
    return dict(feat=h.detach(), feat1=feat1, x0=x0, pre=pres, masks=[tuple(m.bool() for m in mk) for mk in masks], gw=gw)


def tensors(result, counts=BLOCKS):
    """{'feat': ..., 'feat1': ..., 'layer1.0.w1': ...} of a ``trunk`` result: what the tests compare, by name."""
    out = {"feat": result["feat"], "feat1": result["feat1"]}
    for (name, *_), g in zip(block_specs(counts), result["gw"]):
        out.update({"%s.%s" % (name, n): g[n] for n in B.NAMES if g[n] is not None})
    return out


def e32_table(im, stem, blocks, counts, g_feat, g_feat1, ref64):
    """The reference in float32 under the float64 run's masks -> {tensor name: its error over the float64 tensor's largest element}."""
    r32 = tensors(trunk(im, stem, blocks, counts, g_feat, g_feat1, masks=ref64["masks"], dtype=torch.float32), counts)
    return {k: B.rel_max(r32[k], v) for k, v in tensors(ref64, counts).items()}


# ---------------------------------------------------------------------------------------------------------------------
# the stem's max pool alone
# ---------------------------------------------------------------------------------------------------------------------
def pool_input(hw, tied, seed=0):
    """(2, 8, H, W) float32: ``tied`` -> randn quantised to multiples of 0.25, two standard deviations per step (most windows tie,
    and overlapping windows choose the same pixel), else randn."""
    g = torch.Generator().manual_seed(100 * hw[0] + hw[1] + 10000 * seed + int(tied))
    x = torch.randn(2, 8, *hw, generator=g)
    return torch.round(x / 2.0) / 4.0 if tied else x


def pool_naive(x, gy):
    """max_pool2d(3, 2, 0, ceil_mode=True) with indices and its backward as three plain loops in numpy, float64: the first element
    in window order (rows, then columns) wins a tie; a window reaches past the input only at the far edge and is cut there.
    -> (y, flat index iy * W + ix per plane, gx)."""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    nb, c, H, W = x.shape
    ho, wo = pool_hw((H, W))
    y, idx, gx = np.empty((nb, c, ho, wo)), np.empty((nb, c, ho, wo), np.int64), np.zeros_like(x)
    for plane in np.ndindex(nb, c):
        for oy in range(ho):
            for ox in range(wo):
                best, at = -np.inf, -1
                for iy in range(2 * oy, min(2 * oy + 3, H)):
                    for ix in range(2 * ox, min(2 * ox + 3, W)):
                        if x[plane][iy, ix] > best:
                            best, at = x[plane][iy, ix], iy * W + ix
                y[plane][oy, ox], idx[plane][oy, ox] = best, at
                gx[plane][at // W, at % W] += gy[plane][oy, ox]
    return y, idx, gx


def tied_windows(x):
    """The share of pool windows whose largest value occurs more than once."""
    H, W = x.shape[2:]
    ho, wo = pool_hw((H, W))
    full = F.pad(x.double(), (0, 2 * wo + 1 - W, 0, 2 * ho + 1 - H), value=-math.inf)          # windows cut at the far edge made whole
    win = F.unfold(full, 3, stride=2).view(x.shape[0], x.shape[1], 9, ho * wo)
    return float(((win == win.max(2, keepdim=True).values).sum(2) > 1).double().mean())


def shared_winners(idx):
    """How many input pixels more than one window of their plane chose (``idx``: (B, C, Ho, Wo) flat indices)."""
    flat = np.asarray(idx).reshape(idx.shape[0] * idx.shape[1], -1)
    return int(sum(len(row) - len(np.unique(row)) for row in flat))
