"""A float64 reference of a chain of trained bottlenecks under GIVEN ReLU masks (no tests here), on the CPU, in plain torch:
nothing here imports a kernel or ``i2vsgg_amd``.

A block is  a1 = bn1(conv1 x) * m1,  a2 = bn2(conv2 a1) * m2,  out = (bn3(conv3 a2) + skip) * mo  with frozen BatchNorms folded to
(scale, shift), the stride on conv1 and on the projection of the skip branch (caffe style), and three boolean masks of the shape of
a1 / a2 / out.  With the masks given this is a polynomial in the input and the filters: no ReLU, no pixel whose side a rounding
error can change, so a float32 computation under the SAME masks sits at float32 rounding from it (tests/
test_bottleneck_ref_host.py measures 1e-6) where two computations that each pick their own ReLU sides differ by whole taps.  With
``masks=None`` the masks are ``pre > 0``: the ordinary network.  The gradients of sum(out * gout) come from float64 autograd.

``mutate`` plants ONE deliberate error of the kind a fused backward can make -- in the backward only, the forward values stay --
for the host test that shows the bounds of tests/test_gpu_bottleneck_bwd.py would catch it."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5                      # FrozenBN's
NAMES = ("w1", "w2", "w3", "wd")
MUTATIONS = ("s3_1pct",                     # s3 off by 1 % in the backward (data gradient and gw3)
             "s1_one_channel_5pct",         # channel 0 of s1 off by 5 %
             "m1_last_column_on",           # m1's last image column read as true
             "mo_not_applied_to_skip",      # the output mask on the conv3 branch but not on the skip gradient
             "proj_scale_dropped",          # sd missing in the projection's data gradient
             "handover_mask_dropped",       # block k + 1's input mask missing on the gradient handed to block k
             "wgrad_row_scale_dropped")     # s3 missing in gw3

# case -> blocks (cin, planes, stride, projection), batch, input H x W, whether the chain input is a ReLU output whose mask the
# first block applies to the gradient it returns (``in_relu`` of ops._BottleneckFn).  The smallest shapes that reach each form of
# the fused backward (tests/test_gpu_bottleneck_bwd.py has the table)
CASES = {
    "identity": dict(blocks=[(256, 64, 1, False)], batch=2, hw=(9, 14), in_relu=False),
    "identity_in_relu": dict(blocks=[(256, 64, 1, False)], batch=2, hw=(9, 14), in_relu=True),
    "projection": dict(blocks=[(64, 64, 1, True)], batch=2, hw=(7, 11), in_relu=False),
    "strided": dict(blocks=[(128, 64, 2, True)], batch=2, hw=(11, 15), in_relu=False),
    "direct": dict(blocks=[(128, 32, 1, False)], batch=2, hw=(9, 11), in_relu=False),
    "tiny_map": dict(blocks=[(256, 64, 1, False)], batch=3, hw=(3, 5), in_relu=False),
    "hand_over": dict(blocks=[(128, 64, 2, True), (256, 64, 1, False)], batch=2, hw=(11, 15), in_relu=False),
}


def mutation_applies(mutation, case):
    """Whether the term ``mutation`` breaks exists in ``case``."""
    blocks = CASES[case]["blocks"]
    if mutation == "proj_scale_dropped":
        return any(b[3] for b in blocks)
    if mutation == "handover_mask_dropped":
        return len(blocks) > 1
    return True


def out_hw(hw, stride):
    return tuple((d - 1) // stride + 1 for d in hw)          # 1x1 / stride s / pad 0


def make_case(name, seed=0):
    """The float32 inputs of a case, the same on the host and on the device: x = relu(randn), gout = randn, per block the filters
    (ConvParams' He init) and the raw BatchNorm buffers, spread as tests/test_gpu_kernels.py spreads them for the block stack."""
    case = CASES[name]
    g = torch.Generator().manual_seed(1000 * seed + sorted(CASES).index(name))
    randn = lambda *s: torch.randn(*s, generator=g)
    rand = lambda *s: torch.rand(*s, generator=g)

    def conv(cout, cin, k):
        return randn(cout, cin, k, k) * math.sqrt(2.0 / (k * k * cout))

    def bn(c):
        return dict(weight=rand(c) + 0.5, bias=randn(c) * 0.2, running_mean=randn(c) * 0.2, running_var=rand(c) * 1.5 + 0.5)

    blocks, hw = [], case["hw"]
    x = torch.relu(randn(case["batch"], case["blocks"][0][0], *hw))
    for cin, planes, stride, proj in case["blocks"]:
        b = dict(stride=stride, w1=conv(planes, cin, 1), w2=conv(planes, planes, 3), w3=conv(planes * 4, planes, 1),
                 wd=conv(planes * 4, cin, 1) if proj else None, bn1=bn(planes), bn2=bn(planes), bn3=bn(planes * 4),
                 bnd=bn(planes * 4) if proj else None)
        blocks.append(b)
        hw = out_hw(hw, stride)
    gout = randn(case["batch"], case["blocks"][-1][1] * 4, *hw)
    return dict(x=x, gout=gout, blocks=blocks, in_relu=case["in_relu"])


def fold(bn):
    """FrozenBN.folded(): the float32 (scale, shift) of an eval-mode BatchNorm."""
    scale = bn["weight"] / torch.sqrt(bn["running_var"] + EPS)
    return scale, bn["bias"] - bn["running_mean"] * scale


def folded_block(raw):
    """A block of ``make_case`` as ``chain`` takes it: filters + (s, b) per conv."""
    blk = dict(stride=raw["stride"], w1=raw["w1"], w2=raw["w2"], w3=raw["w3"], wd=raw["wd"])
    for k, name in (("1", "bn1"), ("2", "bn2"), ("3", "bn3"), ("d", "bnd")):
        blk["s" + k], blk["b" + k] = fold(raw[name]) if raw[name] is not None else (None, None)
    return blk


def _bwd(value, grad_of):
    """``value`` in the forward, the gradient of ``grad_of`` in the backward."""
    return grad_of + (value - grad_of).detach()


def _vec(t):
    return t.view(1, -1, 1, 1)


def _block(x, p, masks, mutate, last):
    st = p["stride"]
    c1 = F.conv2d(x, p["w1"], None, st)
    p1 = c1 * _vec(p["s1"]) + _vec(p["b1"])
    if mutate == "s1_one_channel_5pct":
        s1 = p["s1"].clone()
        s1[0] *= 1.05
        p1 = _bwd(p1, c1 * _vec(s1) + _vec(p["b1"]))
    m1 = masks[0] if masks is not None else p1.detach() > 0
    a1 = p1 * m1
    if mutate == "m1_last_column_on":
        wrong = m1.clone()
        wrong[..., -1] = True
        a1 = _bwd(a1, p1 * wrong)
    p2 = F.conv2d(a1, p["w2"], None, 1, 1) * _vec(p["s2"]) + _vec(p["b2"])
    m2 = masks[1] if masks is not None else p2.detach() > 0
    a2 = p2 * m2
    h = F.conv2d(a2, p["w3"]) * _vec(p["s3"])
    if mutate == "s3_1pct":
        h = _bwd(h, h * 1.01)
    if mutate == "wgrad_row_scale_dropped":
        h = _bwd(h, F.conv2d(a2, p["w3"].detach()) * _vec(p["s3"]) + F.conv2d(a2.detach(), p["w3"]))
    if p["wd"] is not None:
        skip = F.conv2d(x, p["wd"], None, st) * _vec(p["sd"]) + _vec(p["bd"])
        if mutate == "proj_scale_dropped":
            skip = _bwd(skip, F.conv2d(x.detach(), p["wd"], None, st) * _vec(p["sd"]) + F.conv2d(x, p["wd"].detach(), None, st))
    else:
        skip = x
    p3 = h + _vec(p["b3"]) + skip
    mo = masks[2] if masks is not None else p3.detach() > 0
    out = p3 * mo
    if mutate == "mo_not_applied_to_skip":
        out = _bwd(out, (h + _vec(p["b3"])) * mo + skip)
    if mutate == "handover_mask_dropped" and not last:
        out = _bwd(out, p3)
    return out, (p1.detach(), p2.detach(), p3.detach()), (m1, m2, mo)


def chain_forward(h, params, masks=None, mutate=None):
    """The blocks of ``chain`` as a differentiable function of ``h`` and of ``params`` (block dicts whose tensors already have
    h's type; the caller decides which are leaves) -> (out, pre = [(p1, p2, p3)], masks = [(m1, m2, mo)] as booleans).  A larger
    reference (tests/detector_head_ref.py: layer4 behind RoIAlign) composes this inside its own graph."""
    pres, used = [], []
    for i, p in enumerate(params):
        m = None if masks is None else tuple(t.to(h.dtype) for t in masks[i])
        h, pre, mk = _block(h, p, m, mutate, i == len(params) - 1)
        pres.append(pre)
        used.append(tuple(t > 0 for t in mk))
    return h, pres, used


def chain(x, blocks, gout, masks=None, in_mask=None, mutate=None, frozen=(), dtype=torch.float64):
    """x (B,C,H,W), ``blocks``: dicts of w1 w2 w3 wd (None: identity skip) s1 b1 .. sd bd stride, gout of the chain output's shape;
    ``masks``: per block (m1, m2, mo) boolean or None (``pre > 0``); ``in_mask``: the mask of the ReLU that produced x, applied to
    the returned gx (the block protocol's ``in_relu``); ``frozen``: (block index, filter name) pairs that get no gradient.
    -> dict(out, pre = [(p1, p2, p3)], masks = [(m1, m2, mo)], gx, gw = [{name: gradient or None}]) in ``dtype``."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError("unknown mutation %r" % (mutate,))
    leaf = x.detach().to(dtype).requires_grad_(True)
    h = leaf if in_mask is None else leaf * in_mask.to(dtype)
    params, wanted = [], []
    for i, blk in enumerate(blocks):
        p = {k: (v.detach().to(dtype) if torch.is_tensor(v) else v) for k, v in blk.items()}
        for name in NAMES:
            if p[name] is not None and (i, name) not in frozen:
                p[name].requires_grad_(True)
                wanted.append((i, name, p[name]))
        params.append(p)
    h, pres, used = chain_forward(h, params, masks, mutate)
    grads = torch.autograd.grad((h * gout.to(dtype)).sum(), [leaf] + [w for _, _, w in wanted])
    gw = [dict.fromkeys(NAMES) for _ in blocks]
    for (i, name, _), g in zip(wanted, grads[1:]):
        gw[i][name] = g
    return dict(out=h.detach(), pre=pres, masks=used, gx=grads[0], gw=gw)


def gradients(result):
    """{'gx': ..., 'b0.w1': ...} of a ``chain`` result: the tensors the tests compare, by name (frozen filters left out)."""
    out = {"gx": result["gx"]}
    for i, g in enumerate(result["gw"]):
        out.update({"b%d.%s" % (i, n): g[n] for n in NAMES if g[n] is not None})
    return out


def rel_max(got, want):
    """max |got - want| over max |want|, in float64."""
    want = want.double()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))
