"""The backward of the trunk -- ``C4Base.forward(im, tap=True)`` with miniature block counts (3, 2, 2) -- against the masked float64
reference of tests/trunk_ref.py: the wiring BETWEEN the bottleneck nodes that tests/test_gpu_bottleneck_bwd.py holds one by one.

What a case reaches that no block case does: a block that is ``in_relu`` AND pre-masked (layer1[1]); the layer1 -> layer2 hand-over
(a strided block with a projection that is ``in_relu`` and pre-masks a block of another layer); the tap (layer2's output feeds
layer3 and the caller: layer2[-1] masks for itself, layer3[0] returns an unmasked gradient, autograd adds the two);
``needs_input_grad[0] == False`` on layer1[0] behind the frozen stem; ``train._SplitBatch``, whose backward writes two halves into
one buffer; and ``ops._MaxPoolFn``'s saved argmax and scatter backward.

The ReLU masks of all seven blocks are taken from the device -- the nodes' own saved activations -- and handed to the reference, so
both sides compute the same polynomial.  Every tensor is held to  max(1e-4, 16 e32)  of its largest element: the block test's bound
for its kind, or 16 x the float32 CPU reference's own error under the same masks should seven blocks in a row exceed it (they do
not: e32 <= 2.3e-6, the bound in force is 1e-4 everywhere).  tests/test_trunk_ref_host.py shows on the CPU that seven wiring errors
(a dropped tap term, a mask skipped on either side of the tap, a dropped hand-over mask between layers and at the middle block,
exchanged halves, a projection filter gradient from the wrong gradient) each move a tensor by at least 10 x that bound.

Largest observed error, one run on an MI355X, both geometries (profiles/r20_trunk_margins.txt), over the tensor's largest element:
feat / feat1 2.3e-6; a filter gradient that has crossed a Winograd data gradient 9.6e-6 (layer1.0.w1: 0.10 of its bound), the last
block's gw3 (direct pieces alone) 8.5e-7; plain indexing against _SplitBatch 1.1e-5; mask flips 2.7e-7 of the pixels against a
band of 4.5e-4; the max pool's argmax 0 entries differing, its backward 6.6e-8.  With layer2[-1] wired as pre-masked by layer3[0]
on the device (tried once, by hand) layer2.1.w3 moves by 0.68 of its largest element: 6800 bounds, and within 1e-5 of the
reference's plant ``tap_premasked``.
Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bottleneck_ref as B  # noqa: E402
import trunk_ref as R  # noqa: E402
from conftest import record_margin  # noqa: E402
from test_gpu_bottleneck_bwd import DIRECT_REL, FLIP_BAND, _cl, _filters  # noqa: E402
from test_gpu_kernels import DEV, WINOGRAD_REL  # noqa: E402

# (in_relu, out_premasked) of the seven nodes: layer1 | layer2 | layer3.  layer2[-1] is NOT pre-masked and layer3[0] NOT in_relu:
# the tap has two consumers
FLAGS = [(False, True), (True, True), (True, True), (True, True), (True, False), (False, True), (True, False)]
NAMES = [s[0] for s in R.block_specs()]
HALF = 2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import ops as o
    return o


class _LibSpy:
    """ops.lib with the max pool's argmax pointer recorded."""

    def __init__(self, real, seen):
        self._real, self._seen = real, seen

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "i2v_maxpool3x3s2_fwd":
            return fn

        def call(x, y, arg, *rest):
            self._seen.append(arg)
            return fn(x, y, arg, *rest)
        return call


def _build(name):
    """C4Base((3, 2, 2)) holding the geometry's filters and BatchNorm buffers, the stem frozen as resnet._init_modules freezes it
    -> (base on the device, its seven blocks, the case, the reference's stem and blocks made of the DEVICE's folded scales)."""
    from i2vsgg_amd.model.faster_rcnn.layers import C4Base
    case = R.make_trunk(name)
    with torch.random.fork_rng(devices=[]):             # ConvParams' init draws from the global generator: leave it as found
        base = C4Base(R.BLOCKS)
    for p in base[0].parameters():
        p.requires_grad = False
    blks = [blk for layer in (base[4], base[5], base[6]) for blk in layer]
    assert len(blks) == len(case["blocks"]) == 7
    with torch.no_grad():
        base[0].weight.copy_(case["stem"]["w"])
        for k, v in case["stem"]["bn"].items():
            getattr(base[1], k).copy_(v)
        base[1].invalidate()
        for blk, raw, (_, cin, planes, stride, proj) in zip(blks, case["blocks"], R.block_specs()):
            assert (blk.conv1.cin, blk.conv1.cout, blk.stride, blk.downsample is not None) == (cin, planes, stride, proj)
            for n, w in _filters(blk):
                w.copy_(raw[n])
            for n, bn in [("bn1", blk.bn1), ("bn2", blk.bn2), ("bn3", blk.bn3)] + ([("bnd", blk.downsample[1])] if proj else []):
                for k, v in raw[n].items():
                    getattr(bn, k).copy_(v)
                bn.invalidate()
    base = base.to(DEV)
    s, b = (t.cpu() for t in base[1].folded())
    stem = dict(w=base[0].weight.detach().cpu(), s=s, b=b)
    blocks = []
    for blk in blks:
        d = dict(stride=blk.stride, wd=None, sd=None, bd=None)
        d.update({n: w.detach().cpu() for n, w in _filters(blk)})
        for k, bn in (("1", blk.bn1), ("2", blk.bn2), ("3", blk.bn3)) + ((("d", blk.downsample[1]),) if blk.downsample is not None else ()):
            d["s" + k], d["b" + k] = (t.cpu() for t in bn.folded())
        blocks.append(d)
    return base, blks, case, stem, blocks


def _block_nodes(feat, feat1):
    """The seven _BottleneckFnBackward nodes in forward order, reached from feat.grad_fn along the gradient of each block's input."""
    nodes, fn = [], feat.grad_fn
    while fn is not None and type(fn).__name__ == "_BottleneckFnBackward":
        nodes.append(fn)
        fn = fn.next_functions[0][0]
    assert fn is None and len(nodes) == 7, (fn, len(nodes))          # the chain ends at layer1[0]: its input asks for no gradient
    nodes.reverse()
    assert feat1.grad_fn is nodes[R.BLOCKS[0] + R.BLOCKS[1] - 1]       # the tap IS layer2[-1]'s output
    return nodes


def _run(ops, monkeypatch, base, blks, case, split):
    """One forward + backward of the trunk under the four given gradients -> dict(feat, feat1, masks, grads, what ran).
    ``split``: the halves through train._SplitBatch (the one-pass step's form), else by plain indexing."""
    from i2vsgg_amd import train
    for p in base.parameters():
        p.grad = None
    pool_args = []
    real_lib = ops.lib
    monkeypatch.setattr(ops, "lib", _LibSpy(real_lib, pool_args))
    try:
        feat, feat1 = base(case["im"].to(DEV), tap=True)
    finally:
        monkeypatch.setattr(ops, "lib", real_lib)
    nodes = _block_nodes(feat, feat1)
    masks = [tuple((t.detach() > 0).cpu() for t in n.saved_tensors[1:4]) for n in nodes]
    ran = dict(flags=[n.flags[:2] for n in nodes], has_ds=[n.flags[3] for n in nodes], needs_x=[n.needs_input_grad[0] for n in nodes],
               pool_args=pool_args, fused=[blk._fused() for blk in blks])
    g = [_cl(t.to(DEV)) for t in case["g"]]
    if split:
        (fs, ft), (f1s, f1t) = train._SplitBatch.apply(feat, HALF), train._SplitBatch.apply(feat1, HALF)
        assert type(fs.grad_fn).__name__ == "_SplitBatchBackward" and type(f1t.grad_fn).__name__ == "_SplitBatchBackward"
    else:
        fs, ft, f1s, f1t = feat[:HALF], feat[HALF:], feat1[:HALF], feat1[HALF:]
    ((fs * g[0]).sum() + (ft * g[1]).sum() + (f1s * g[2]).sum() + (f1t * g[3]).sum()).backward()
    grads = {}
    for name, blk in zip(NAMES, blks):
        grads.update({"%s.%s" % (name, n): w.grad.clone() for n, w in _filters(blk) if w.grad is not None})
    ran["stem_grads"] = [k for k, p in list(base[0].named_parameters()) + list(base[1].named_parameters()) if p.grad is not None]
    return dict(feat=feat.detach().clone(), feat1=feat1.detach().clone(), masks=masks, grads=grads, ran=ran)


def _kind(name):
    """gw3 of the last block is the direct pieces' alone (its incoming gradient is given); every other gradient has crossed a
    Winograd data gradient on its way."""
    last = NAMES[-1]
    return ("direct", DIRECT_REL) if name == last + ".w3" else ("winograd", WINOGRAD_REL)


def _hold_to_reference(test, run, ref, e32):
    """Every figure is recorded before anything is asserted -> the failures."""
    failures = []
    for k in ("feat", "feat1"):
        err, bound = B.rel_max(run[k], ref[k]), R.bound(e32[k], WINOGRAD_REL)
        record_margin(test, "%s (e32 %.3g)" % (k, e32[k]), err, bound)
        if not err <= bound:
            failures.append((k, err, bound))
    # the masks are the device's; they may differ from the reference's own choice only within rounding of zero
    n_flip = n_band = n_all = 0
    for name, pres, mine in zip(NAMES, ref["pre"], run["masks"]):
        for what, pre, m in zip(("a1", "a2", "out"), pres, mine):
            flips, band = m != (pre > 0), pre.abs() <= FLIP_BAND * pre.abs().max()
            n_flip, n_band, n_all = n_flip + int(flips.sum()), n_band + int(band.sum()), n_all + pre.numel()
            if bool((flips & ~band).any()):
                failures.append(("%s.%s mask flips away from zero" % (name, what), float((pre.abs() * flips).max() / pre.abs().max())))
    record_margin(test, "mask flips (fraction; bound: the band's share)", n_flip / n_all, n_band / n_all)
    if not n_flip <= n_band:
        failures.append(("mask flips exceed the band's share", n_flip, n_band))
    want = {k: v for k, v in R.tensors(ref).items() if k not in ("feat", "feat1")}
    assert sorted(run["grads"]) == sorted(want) and len(want) == 24, sorted(set(run["grads"]) ^ set(want))
    for n in want:
        kind, kb = _kind(n)
        err, bound = B.rel_max(run["grads"][n], want[n]), R.bound(e32[n], kb)
        record_margin(test, "grad %s (%s, e32 %.3g)" % (n, kind, e32[n]), err, bound)
        if not err <= bound:
            failures.append((n, err, bound))
    return failures


@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_trunk_backward_vs_masked_float64_reference(ops, monkeypatch, name):
    from i2vsgg_amd import launch
    # ---- the preconditions the case relies on: it cannot pass by silently taking another path
    assert ops.BLOCK_FUSED and ops.WINOGRAD_TRAIN and launch.WGRAD_BRANCH is None
    base, blks, case, stem, blocks = _build(name)
    l1, l2, l3 = base[4], base[5], base[6]
    assert [len(l) for l in (l1, l2, l3)] == list(R.BLOCKS)
    assert not l2[-1]._next and not l3[0].in_relu and not l3[-1]._next and not l1[0].in_relu          # the tap, the two ends
    assert l1[-1]._next[0] is l2[0] and l2[0].in_relu                                                # the layer1 -> layer2 hand-over
    assert not any(p.requires_grad for p in list(base[0].parameters()) + list(base[1].parameters()))

    test = "test_trunk_backward[%s]" % name
    run = _run(ops, monkeypatch, base, blks, case, split=True)
    ran = run["ran"]
    assert all(ran["fused"]), ran["fused"]
    assert ran["flags"] == FLAGS, ran["flags"]
    assert ran["has_ds"] == [s[4] for s in R.block_specs()]
    assert ran["needs_x"] == [False] + [True] * 6, ran["needs_x"]          # layer1[0] reads the frozen stem's output
    assert ran["stem_grads"] == [], ran["stem_grads"]
    assert ran["pool_args"] == [None], ran["pool_args"]                    # one max pool, and no argmax tensor asked for
    nb, H, W = R.GEOMETRIES[name]
    hw1 = B.out_hw(R.pool_hw(R.stem_hw((H, W))), 2)
    assert tuple(run["feat1"].shape) == (nb, 512) + hw1 and tuple(run["feat"].shape) == (nb, 1024) + B.out_hw(hw1, 2)

    args = (case["im"], stem, blocks, case["counts"], torch.cat(case["g"][:2]), torch.cat(case["g"][2:]))
    ref = R.trunk(*args, masks=run["masks"])
    e32 = R.e32_table(*args, ref)
    failures = _hold_to_reference(test, run, ref, e32)

    if name == "75x107":
        # ---- the same step with the halves by plain indexing: autograd's own slice backward in place of _SplitBatch's one buffer
        plain = _run(ops, monkeypatch, base, blks, case, split=False)
        assert plain["ran"]["flags"] == FLAGS
        for n, g in run["grads"].items():
            kind, kb = _kind(n)
            err, bound = B.rel_max(plain["grads"][n], g.double().cpu()), R.bound(e32[n], kb)
            record_margin(test + " plain indexing", "grad %s against the _SplitBatch run (%s)" % (n, kind), err, bound)
            if not err <= bound:
                failures.append(("plain indexing", n, err, bound))
        if not all(torch.equal(a, b) for m, p in zip(run["masks"], plain["masks"]) for a, b in zip(m, p)):
            ref = R.trunk(*args, masks=plain["masks"])          # (a forward sum finished in another order flipped a pixel at zero)
            e32 = R.e32_table(*args, ref)
        failures += [("plain indexing",) + tuple(f) for f in _hold_to_reference(test + " plain indexing", plain, ref, e32)]
    assert not failures, failures


@pytest.mark.parametrize("used", ["first", "second"])
def test_split_batch_backward_with_one_half_used(ops, used):
    """train._SplitBatch alone when only one half reaches the objective: the gradient it returns (seen by a hook on the non-leaf it
    split, before autograd stores it anywhere) is channels_last, holds the given gradient in the used half bit for bit and exact
    zeros in the other."""
    from i2vsgg_amd import train
    gen = torch.Generator().manual_seed(11)
    leaf = _cl(torch.randn(4, 8, 5, 6, generator=gen).to(DEV)).requires_grad_(True)
    x = leaf * 1.0
    seen = []
    x.register_hook(seen.append)
    a, b = train._SplitBatch.apply(x, HALF)
    assert a.shape[0] == HALF and b.shape[0] == 4 - HALF and torch.equal(a, x[:HALF]) and torch.equal(b, x[HALF:])
    g = _cl(torch.randn(2, 8, 5, 6, generator=gen).to(DEV))
    assert bool((g != 0).all())
    ((a if used == "first" else b) * g).sum().backward()
    assert len(seen) == 1 and seen[0].shape == x.shape and seen[0].is_contiguous(memory_format=torch.channels_last)
    mine, other = (seen[0][:HALF], seen[0][HALF:]) if used == "first" else (seen[0][HALF:], seen[0][:HALF])
    assert torch.equal(mine, g) and bool((other == 0).all())
    assert torch.equal(leaf.grad, seen[0]) and leaf.grad.is_contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------------------------------------------------------------
# the stem's max pool with an input that asks for a gradient: the saved argmax and the scatter backward
# ---------------------------------------------------------------------------------------------------------------------
# A pixel lies in at most 2 x 2 windows (3 wide, stride 2), so an element of gx is a sum of at most 4 floats of gy in whatever
# order the scatter's atomics land: 3 additions, each rounding by at most 2^-24 of a partial sum that is at most 4 max|gy|, i.e.
# |error| <= 3 * 4 * 2^-24 max|gy| = 7.2e-7 max|gy| <= 1e-6 max|gx| once max|gx| >= max|gy| (asserted on the seeded data below).
POOL_BWD_REL = 1e-6


@pytest.mark.parametrize("tied", [True, False], ids=["tied", "random"])
@pytest.mark.parametrize("hw", R.POOL_HW, ids=lambda hw: "%dx%d" % hw)
def test_maxpool_argmax_and_backward_vs_float64(ops, hw, tied):
    x = R.pool_input(hw, tied)
    want_y, want_idx = F.max_pool2d(x, 3, 2, 0, ceil_mode=True, return_indices=True)
    gy = torch.randn(want_y.shape, generator=torch.Generator().manual_seed(3))
    x64 = x.double().requires_grad_(True)
    (want_gx,) = torch.autograd.grad((F.max_pool2d(x64, 3, 2, 0, ceil_mode=True) * gy.double()).sum(), x64)

    xd = _cl(x.to(DEV)).requires_grad_(True)
    y = ops.maxpool3x3s2(xd)
    assert type(y.grad_fn).__name__ == "_MaxPoolFnBackward"
    (arg,) = y.grad_fn.saved_tensors
    assert arg is not None and arg.dtype == torch.int32 and arg.shape == want_idx.shape
    assert torch.equal(y.detach().cpu(), want_y)
    # both break a tie to the first element in window order (rows, then columns)
    wrong = int((arg.cpu().long() != want_idx).sum())
    record_margin("test_maxpool_argmax_and_backward[%dx%d-%s]" % (hw + ("tied" if tied else "random",)), "argmax entries differing", wrong, 0)
    assert wrong == 0, wrong
    y.backward(_cl(gy.to(DEV)))
    assert xd.grad.shape == x.shape
    shared = R.shared_winners(want_idx.numpy())
    if tied and hw != (3, 3):
        # overlapping windows choose the same pixel: its gradient is the sum of theirs (the float64 backward adds them too)
        assert R.tied_windows(x) > 0.5 and shared > 0
        counts = torch.zeros(x.shape[0] * x.shape[1], hw[0] * hw[1]).scatter_add_(1, want_idx.view(x.shape[0] * x.shape[1], -1),
                                                                                  torch.ones(x.shape[0] * x.shape[1], want_idx[0, 0].numel()))
        assert int(counts.max()) >= 2 and bool((want_gx.view_as(counts)[counts == 0] == 0).all())
    assert float(want_gx.abs().max()) >= float(gy.abs().max())           # the premise of POOL_BWD_REL
    assert bool((xd.grad.cpu()[want_gx == 0] == 0).all())                 # pixels no window chose
    err = B.rel_max(xd.grad, want_gx)
    record_margin("test_maxpool_argmax_and_backward[%dx%d-%s]" % (hw + ("tied" if tied else "random",)), "gx (%d shared winners)" % shared, err, POOL_BWD_REL)
    assert err <= POOL_BWD_REL, err
