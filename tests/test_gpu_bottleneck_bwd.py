"""The backward of a trained bottleneck as one autograd node (ops._BottleneckFn) against the masked float64 reference
(tests/bottleneck_ref.py), and the kernel forms it is folded into, each alone.

The block's ReLU masks are taken from the device -- the node's own saved activations -- and handed to the reference, so both sides
compute the same polynomial and the comparison has no knife edge: every gradient tensor is held to 1e-4 of its largest element,
where the block stack test of test_gpu_kernels.py (references that pick their own ReLU sides) has to allow 5e-2.
tests/test_bottleneck_ref_host.py shows on the CPU that a wrong scale vector, a mask column, a dropped skip term or a dropped
hand-over mask each move a gradient by at least 10 x that bound.  Needs a real MI355X: `pytest -m gpu`."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bottleneck_ref as R  # noqa: E402
from conftest import record_margin  # noqa: E402
from test_gpu_kernels import DEV, WINOGRAD_REL  # noqa: E402

# the direct kernels alone (test_conv_dgrad_fused_and_wgrad_scaled_vs_torch) and the Winograd filter gradient alone
# (test_winograd_filter_gradient_vs_torch): the bounds those tests hold them to
DIRECT_REL = 1e-4
WINOGRAD_WGRAD_REL = 2e-4
FLIP_BAND = 1e-4            # a device mask may differ from ``pre64 > 0`` only where |pre64| <= FLIP_BAND * max |pre64|
_CL = torch.channels_last


def _cl(t):
    return t.contiguous(memory_format=_CL)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import ops as o
    return o


# ---------------------------------------------------------------------------------------------------------------------
# the block against the reference
# ---------------------------------------------------------------------------------------------------------------------
# id -> (case of bottleneck_ref.CASES, frozen filters, which blocks run as one node, conv2's route family in those)
#   identity          256 -> 64, no projection, 9 x 14: Winograd conv2, partial 4x4 tiles (residues 1 and 2)
#   identity_in_relu  the same with ``in_relu``: the mask of the block input on gx only
#   projection        64 -> 64 with the projection, 7 x 11: layer1[0]'s form, tile residues 3 and 3
#   strided           128 -> 64 stride 2, 11 x 15 -> 6 x 8: strided conv1 / projection data gradients with res + mask at odd sizes,
#                     row_scale on a strided filter gradient
#   direct            128 -> 32: planes < WINOGRAD_TRAIN_MIN_C, conv2 direct, the 3x3 _dgrad_fused with out_scale + mask
#   tiny_map          256 -> 64 at 3 x 5, B = 3: H below one tile
#   hand_over         make_layer(128, 64, 2, 2): out_premasked on block 0, in_relu on block 1
#   mixed_a           the same, block 1's conv2 frozen: block 1 layer by layer, block 0 masks for itself
#   mixed_b           block 0's conv2 frozen: block 1 fused and pre-masking its gx into a layer-by-layer block 0
BLOCK_CASES = {
    "identity": ("identity", (), (True,), "winograd"),
    "identity_in_relu": ("identity_in_relu", (), (True,), "winograd"),
    "projection": ("projection", (), (True,), "winograd"),
    "strided": ("strided", (), (True,), "winograd"),
    "direct": ("direct", (), (True,), "direct"),
    "tiny_map": ("tiny_map", (), (True,), "winograd"),
    "hand_over": ("hand_over", (), (True, True), "winograd"),
    "mixed_a": ("hand_over", ((1, "w2"),), (True, False), "winograd"),
    "mixed_b": ("hand_over", ((0, "w2"),), (False, True), "winograd"),
}
_CONVS = (("w1", "conv1"), ("w2", "conv2"), ("w3", "conv3"))


def _filters(blk):
    out = [(n, getattr(blk, attr).weight) for n, attr in _CONVS]
    return out + ([("wd", blk.downsample[0].weight)] if blk.downsample is not None else [])


def _build(case_name, frozen):
    """make_layer() blocks holding the case's filters and BatchNorm buffers -> (layer on the device, x, gout, reference blocks
    made of the DEVICE's folded scales: what the kernels read, in float64)."""
    from i2vsgg_amd.model.faster_rcnn.layers import make_layer
    case, spec = R.make_case(case_name), R.CASES[case_name]["blocks"]
    with torch.random.fork_rng(devices=[]):             # ConvParams' init draws from the global generator: leave it as found
        layer, cout = make_layer(spec[0][0], spec[0][1], len(spec), spec[0][2])
    assert cout == spec[-1][1] * 4
    for blk, raw, (cin, planes, stride, proj) in zip(layer, case["blocks"], spec):
        assert (blk.conv1.cin, blk.conv1.cout, blk.stride, blk.downsample is not None) == (cin, planes, stride, proj)
        bns = [("bn1", blk.bn1), ("bn2", blk.bn2), ("bn3", blk.bn3)] + ([("bnd", blk.downsample[1])] if proj else [])
        with torch.no_grad():
            for n, w in _filters(blk):
                w.copy_(raw[n])
            for n, bn in bns:
                for k, v in raw[n].items():
                    getattr(bn, k).copy_(v)
                bn.invalidate()
    layer = layer.to(DEV)
    if case["in_relu"]:
        layer[0].in_relu = True
    for i, n in frozen:
        dict(_filters(layer[i]))[n].requires_grad_(False)
    blocks = []
    for blk in layer:
        b = dict(stride=blk.stride, wd=None, sd=None, bd=None)
        b.update({n: w.detach().cpu() for n, w in _filters(blk)})
        for k, bn in (("1", blk.bn1), ("2", blk.bn2), ("3", blk.bn3)) + ((("d", blk.downsample[1]),) if blk.downsample is not None else ()):
            b["s" + k], b["b" + k] = (t.cpu() for t in bn.folded())
        blocks.append(b)
    return layer, _cl(case["x"].to(DEV)), _cl(case["gout"].to(DEV)), blocks


def _run(layer, x0, gout, fused, seen):
    """One forward + backward, block by block -> (out, per block the three masks its own activations give, gradients by name).
    ``seen``: the outputs of the ops.conv2d calls so far (the spy of the test): a layer-by-layer block's activations."""
    for blk in layer:
        for _, w in _filters(blk):
            w.grad = None
    x = x0.clone().requires_grad_(True)
    h, masks, nodes = x, [], []
    for blk, one_node in zip(layer, fused):
        del seen[:]
        shape_in = h.shape
        h = blk(h)
        ho, wo = R.out_hw(shape_in[2:], blk.stride)
        inner, outer = (shape_in[0], blk.conv1.cout, ho, wo), (shape_in[0], blk.conv3.cout, ho, wo)
        if one_node:
            assert type(h.grad_fn).__name__ == "_BottleneckFnBackward" and not seen
            a1, a2, out = h.grad_fn.saved_tensors[1:4]
            nodes.append(h.grad_fn)
        else:
            assert len(seen) == 3 + (blk.downsample is not None)         # conv1, conv2, (projection,) conv3
            a1, a2, out = seen[0], seen[1], seen[-1]
            nodes.append(None)
        assert (tuple(a1.shape), tuple(a2.shape), tuple(out.shape)) == (inner, inner, outer) and tuple(h.shape) == outer
        masks.append(tuple((t.detach() > 0).cpu() for t in (a1, a2, out)))
    flags = [n.flags if n is not None else None for n in nodes]
    (h * gout).sum().backward()
    grads = {"gx": x.grad.clone()}
    for i, blk in enumerate(layer):
        grads.update({"b%d.%s" % (i, n): w.grad.clone() for n, w in _filters(blk) if w.grad is not None})
    return h.detach().clone(), masks, grads, flags


def _grad_bound(name, family):
    """WINOGRAD_REL for a gradient whose path crosses a Winograd kernel (gx, gw1, gw2 of a block whose conv2 is Winograd), the
    direct pieces' bound for gw3, gwd and everything of a direct-route block."""
    crosses = family == "winograd" and (name == "gx" or name.endswith((".w1", ".w2")))
    return ("winograd", WINOGRAD_REL) if crosses else ("direct", DIRECT_REL)


def _hold_to_reference(test, run, blocks, x0, gout, in_relu, frozen, family):
    """The reference under the run's own masks; every figure is recorded before anything is asserted."""
    out, masks, grads, _ = run
    ref = R.chain(x0.cpu(), blocks, gout.cpu(), masks=masks, in_mask=(x0 > 0).cpu() if in_relu else None, frozen=frozen)
    failures = []
    err = R.rel_max(out, ref["out"])
    record_margin(test, "out", err, WINOGRAD_REL)
    if not err <= WINOGRAD_REL:
        failures.append(("out", err))
    # the masks are the device's; they may differ from the reference's own choice only within rounding of zero
    n_flip = n_band = n_all = 0
    for i, (pres, mine) in enumerate(zip(ref["pre"], masks)):
        for what, pre, m in zip(("a1", "a2", "out"), pres, mine):
            flips, band = m != (pre > 0), pre.abs() <= FLIP_BAND * pre.abs().max()
            n_flip, n_band, n_all = n_flip + int(flips.sum()), n_band + int(band.sum()), n_all + pre.numel()
            if bool((flips & ~band).any()):
                failures.append(("b%d.%s mask flips away from zero" % (i, what), float((pre.abs() * flips).max() / pre.abs().max())))
    record_margin(test, "mask flips (fraction; bound: the band's share)", n_flip / n_all, n_band / n_all)
    want = R.gradients(ref)
    assert sorted(grads) == sorted(want), (sorted(grads), sorted(want))          # a frozen filter's gradient is absent on both sides
    for n in want:
        kind, bound = _grad_bound(n, family)
        err = R.rel_max(grads[n], want[n])
        record_margin(test, "%s (%s)" % (n, kind), err, bound)
        if not err <= bound:
            failures.append((n, err, bound))
    assert not failures, failures


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_bottleneck_backward_vs_masked_float64_reference(ops, monkeypatch, name):
    from i2vsgg_amd import conv_route, launch
    case_name, frozen, fused, family = BLOCK_CASES[name]
    layer, x0, gout, blocks = _build(case_name, frozen)
    seen = []
    real = ops.conv2d

    def spy(*a, **k):
        y = real(*a, **k)
        seen.append(y)
        return y
    monkeypatch.setattr(ops, "conv2d", spy)              # layers.py looks ops.conv2d up by attribute

    # ---- the preconditions the case relies on: it cannot pass by silently taking another path
    assert ops.BLOCK_FUSED and ops.WINOGRAD_TRAIN and ops.WINOGRAD_WGRAD and ops.WINOGRAD_KEEP_V and launch.WGRAD_BRANCH is None
    assert tuple(b._fused() for b in layer) == fused
    in_relu = R.CASES[case_name]["in_relu"]
    assert layer[0].in_relu == in_relu
    if len(layer) > 1:
        assert layer[0]._next[0] is layer[1] and layer[1].in_relu and not layer[1]._next
    hw = x0.shape[2:]
    for blk, one_node in zip(layer, fused):
        hw = R.out_hw(hw, blk.stride)
        if one_node:        # conv2's route as ops.bottleneck asks for it
            route = ops._plan((x0.shape[0], blk.conv2.cin) + hw, blk.conv2.weight.shape, 1, 1, scale=True, shift=True, relu=True,
                              needs_w=blk.conv2.weight.requires_grad, in_block=True)
            want = ((conv_route.WINOGRAD, conv_route.WINOGRAD, conv_route.WINOGRAD_V) if family == "winograd" else
                    (conv_route.DIRECT, conv_route.DIRECT, conv_route.DIRECT))
            assert (route.fwd, route.dgrad, route.wgrad) == want, route

    test = "test_bottleneck_backward[%s]" % name
    run = _run(layer, x0, gout, fused, seen)
    # what the nodes were told: (in_relu, out_premasked, ...) -- the hand-over happens only between two fused blocks
    for i, fl in enumerate(run[3]):
        if fl is not None:
            nxt_fused = i + 1 < len(layer) and fused[i + 1]
            assert fl[:2] == (layer[i].in_relu, nxt_fused) and fl[3] == (layer[i].downsample is not None), (i, fl)
    _hold_to_reference(test, run, blocks, x0, gout, in_relu, frozen, family)

    # ---- ordered sums: the same figures, and the same bits twice (the second and third run take their small filter gradients
    # from the context's arena, sized by fit() after the first)
    ctx = launch.LaunchContext(DEV, ordered=True)
    runs = []
    for _ in range(3):
        with ctx:
            runs.append(_run(layer, x0, gout, fused, seen))
            torch.cuda.synchronize()
        ctx.fit()
    _hold_to_reference(test + " ordered", runs[1], blocks, x0, gout, in_relu, frozen, family)
    assert torch.equal(runs[1][0], runs[2][0])
    for n in runs[1][2]:
        assert torch.equal(runs[1][2][n], runs[2][2][n]), (n, float((runs[1][2][n] - runs[2][2][n]).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# the pieces alone
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return (lambda *s: torch.randn(*s, generator=g)), (lambda *s: torch.rand(*s, generator=g))


@pytest.mark.parametrize("cin,cout", [(128, 64), (64, 256)])
@pytest.mark.parametrize("hw", [(11, 15), (10, 14)])
def test_dgrad_fused_strided_1x1_vs_float64(ops, hw, cin, cout):
    """ops._dgrad_fused at stride 2 alone -- conv1 and the projection of a strided block: gy_scale only (the projection's call),
    res + mask (conv1's), res only, all four.  gx is exactly zero off the stride grid and where the mask is not positive; the
    rest is where(mask > 0, conv_transpose2d(gy * gs, w, stride 2) * os + res, 0) in float64."""
    B, (H, W) = 2, hw
    ho, wo = R.out_hw(hw, 2)
    randn, rand = _gen(H * cin)
    w, gy = randn(cout, cin, 1, 1) * 0.05, randn(B, cout, ho, wo)
    gs, osc = rand(cout) + 0.5, rand(cin) + 0.5
    on_grid = torch.zeros(H, W, dtype=torch.bool)
    on_grid[::2, ::2] = True
    res, mask = randn(B, cin, H, W) * on_grid, randn(B, cin, H, W)         # res is zero off the stride grid: the contract
    dev = lambda t: _cl(t.to(DEV)) if t.dim() == 4 else t.to(DEV)
    sets = {"gy_scale": dict(gy_scale=gs), "res+mask": dict(res=res, mask=mask), "res": dict(res=res),
            "all": dict(gy_scale=gs, out_scale=osc, res=res, mask=mask)}
    failures = []
    for tag, kw in sets.items():
        got = ops._dgrad_fused(dev(gy), dev(w), (B, cin, H, W), 0, stride=2, **{k: dev(v) for k, v in kw.items()}).cpu()
        g64 = gy.double() * (kw["gy_scale"].double().view(1, -1, 1, 1) if "gy_scale" in kw else 1.0)
        want = F.conv_transpose2d(g64, w.double(), None, 2, 0, output_padding=(H - 1 - 2 * (ho - 1), W - 1 - 2 * (wo - 1)))
        assert want.shape == got.shape
        if "out_scale" in kw:
            want = want * osc.double().view(1, -1, 1, 1)
        if "res" in kw:
            want = want + res.double()
        assert bool((got[:, :, ~on_grid] == 0).all()), tag
        if "mask" in kw:
            want = torch.where(mask > 0, want, torch.zeros_like(want))
            assert bool((got[~(mask > 0)] == 0).all()), tag
        err = R.rel_max(got, want)
        record_margin("test_dgrad_fused_strided_1x1[%dx%d-%d-%d]" % (H, W, cin, cout), tag, err, DIRECT_REL)
        if not err <= DIRECT_REL:
            failures.append((tag, err))
    assert not failures, failures


@pytest.mark.parametrize("B,cout,cin,H,W", [(2, 64, 64, 9, 14), (1, 64, 128, 3, 5), (3, 128, 64, 4, 4)])
def test_winograd_dgrad_fused_vs_float64_and_row_split_bits(ops, B, cout, cin, H, W):
    """i2v_conv3x3_winograd4_dgrad alone with out_scale and mask: exactly zero where the mask is not positive, float64 elsewhere;
    and the row-split transforms (I2V_WINO_ROWS = 3) give the one-thread form's bits -- "every value is computed by the same
    expression" (csrc/winograd.hip), on partial tiles too."""
    from i2vsgg_amd._lib import TUNE, lib
    randn, rand = _gen(B * cin + H)
    w, g = randn(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5, randn(B, cout, H, W)
    osc, mask = rand(cin) + 0.5, randn(B, cin, H, W)
    want = F.conv_transpose2d(g.double(), w.double(), None, 1, 1) * osc.double().view(1, -1, 1, 1)
    want = torch.where(mask > 0, want, torch.zeros_like(want))
    gd, md, od = _cl(g.to(DEV)), _cl(mask.to(DEV)), osc.to(DEV)
    U = ops.winograd_filter_dgrad(_cl(w.to(DEV)))
    key = TUNE["I2V_WINO_ROWS"]
    old = lib.i2v_get_tuning(key)
    assert old == 0
    plain = ops._winograd_dgrad_fused(gd, U, od, md).clone()
    try:
        assert lib.i2v_set_tuning(key, 3) == 0
        rows = ops._winograd_dgrad_fused(gd, U, od, md).clone()
    finally:
        lib.i2v_set_tuning(key, old)
    assert bool((plain.cpu()[~(mask > 0)] == 0).all())
    err = R.rel_max(plain, want)
    record_margin("test_winograd_dgrad_fused[%d-%d-%d-%dx%d]" % (B, cout, cin, H, W), "gx", err, WINOGRAD_REL)
    assert err <= WINOGRAD_REL
    assert torch.equal(plain, rows), float((plain - rows).abs().max())


@pytest.mark.parametrize("B,C,N,H,W", [(2, 64, 64, 9, 14), (1, 128, 64, 13, 21)])
def test_winograd_filter_gradient_from_kept_v_equals_from_x(ops, B, C, N, H, W):
    """i2v_conv3x3_winograd4_wgrad_v on the V the forward kept against i2v_conv3x3_winograd4_wgrad transforming x again: V is written
    by the same transform kernel either way, so with ordered sums the two are the same bits (and both within the Winograd filter
    gradient's bound of float64)."""
    from i2vsgg_amd import launch
    from i2vsgg_amd.conv_route import WINOGRAD_V, WINOGRAD_X
    randn, rand = _gen(B + C)
    x, g, w = randn(B, C, H, W), randn(B, N, H, W), randn(N, C, 3, 3) * (2.0 / (9 * C)) ** 0.5
    s, b, rs = rand(N) + 0.5, rand(N) - 0.5, rand(N) + 0.5
    xd, gd = _cl(x.to(DEV)), _cl(g.to(DEV))
    want = torch.nn.grad.conv2d_weight(x.double(), (N, C, 3, 3), g.double(), 1, 1) * rs.double().view(-1, 1, 1, 1)
    with launch.LaunchContext(DEV, ordered=True), torch.no_grad():
        _, v = ops._winograd_fwd(xd, ops.winograd_filter(_cl(w.to(DEV)), 4), s.to(DEV), b.to(DEV), True, keep_v=True)
        assert v is not None
        from_v = ops._conv_wgrad_raw(xd, gd, (N, C, 3, 3), 1, 1, route=WINOGRAD_V, v=v, row_scale=rs.to(DEV)).clone()
        from_x = ops._conv_wgrad_raw(xd, gd, (N, C, 3, 3), 1, 1, route=WINOGRAD_X, row_scale=rs.to(DEV)).clone()
    err = R.rel_max(from_x, want)
    record_margin("test_winograd_filter_gradient_v_vs_x[%d-%d-%d-%dx%d]" % (B, C, N, H, W), "gw", err, WINOGRAD_WGRAD_REL)
    assert err <= WINOGRAD_WGRAD_REL
    assert torch.equal(from_v, from_x), float((from_v - from_x).abs().max())


# k, Cin, Cout, H, W (B = 2): a 1x1 layer 64 -> 256 and a 3x3 layer 64 -> 64 at 9 x 14 (252 pixels), the 1x1 layer again at
# 19 x 23 (874 pixels: above the 224-pixel cut, the pixel reduction splits)
@pytest.mark.parametrize("k,cin,cout,H,W", [(1, 64, 256, 9, 14), (3, 64, 64, 9, 14), (1, 64, 256, 19, 23)])
@pytest.mark.parametrize("atomics", [2, 0], ids=["default", "ordered"])
def test_filter_gradient_beta_one_adds_onto_a_nonzero_gradient(ops, atomics, k, cin, cout, H, W):
    """beta = 1 of i2v_conv_wgrad, i2v_conv_wgrad_scaled and i2v_conv3x3_winograd4_wgrad, called directly, onto a gradient that is
    NOT zero (in the steps it only ever meets the pre-zeroed arena): prefill + float64; beta = 0 ignores a NaN prefill; and the
    Winograd entry's final transform adds beta * gw in one rounding: with ordered sums, prefill + (the beta = 0 result) exactly."""
    from i2vsgg_amd import launch
    from i2vsgg_amd._lib import TUNE, check, lib, ptr, stream
    B, pad = 2, k // 2
    randn, rand = _gen(H + k)
    x, g, rs, prefill = randn(B, cin, H, W), randn(B, cout, H, W), rand(cout) + 0.5, randn(cout, cin, k, k)
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), g.double(), 1, pad)
    ref_rs = ref * rs.double().view(-1, 1, 1, 1)
    xd, gd, rsd = _cl(x.to(DEV)), _cl(g.to(DEV)), rs.to(DEV)

    def call(entry, gw, beta):
        sws = launch.split_buffer(xd.device)
        if entry == "conv_wgrad":
            rc = lib.i2v_conv_wgrad(ptr(xd), ptr(gd), ptr(gw), B, H, W, cin, cout, k, k, 1, pad, beta, ptr(sws), sws.numel(), stream())
        elif entry == "conv_wgrad_scaled":
            rc = lib.i2v_conv_wgrad_scaled(ptr(xd), ptr(gd), ptr(rsd), ptr(gw), B, H, W, cin, cout, k, k, 1, pad, beta, ptr(sws),
                                           sws.numel(), stream())
        else:
            ws = launch.workspace(lib.i2v_conv3x3_winograd4_wgrad_workspace_bytes(B, H, W, cin, cout), xd.device, "winograd_wgrad")
            rc = lib.i2v_conv3x3_winograd4_wgrad(ptr(xd), ptr(gd), ptr(rsd), ptr(gw), B, H, W, cin, cout, beta, ptr(ws), ws.numel(),
                                                 stream())
        check(rc, entry)
        return gw

    entries = [("conv_wgrad", ref, DIRECT_REL), ("conv_wgrad_scaled", ref_rs, DIRECT_REL)]
    if k == 3:
        entries.append(("conv3x3_winograd4_wgrad", ref_rs, WINOGRAD_WGRAD_REL))
    key = TUNE["I2V_SPLIT_ATOMICS"]
    old = lib.i2v_get_tuning(key)
    assert old == 2
    failures = []
    try:
        assert lib.i2v_set_tuning(key, atomics) == 0
        for entry, want, bound in entries:
            test = "test_filter_gradient_beta_one[%s-%d-%d-%d-%dx%d]" % ("ordered" if atomics == 0 else "default", k, cin, cout, H, W)
            pre = _cl(prefill.to(DEV))
            assert pre.abs().min() > 0
            fresh = call(entry, _cl(torch.full((cout, cin, k, k), float("nan"), device=DEV)), 0.0)
            added = call(entry, pre.clone(), 1.0)
            assert bool(torch.isfinite(fresh).all()), entry               # beta = 0 never reads gw
            scale = float(want.abs().max())
            e0 = float((fresh.double().cpu() - want).abs().max()) / scale
            e1 = float((added.double().cpu() - (prefill.double() + want)).abs().max()) / scale
            record_margin(test, entry + " beta 0", e0, bound)
            record_margin(test, entry + " beta 1 onto randn", e1, bound)
            if not (e0 <= bound and e1 <= bound):
                failures.append((entry, e0, e1, bound))
            if entry == "conv3x3_winograd4_wgrad" and atomics == 0:
                assert torch.equal(added, pre + fresh), float((added - (pre + fresh)).abs().max())
    finally:
        lib.i2v_set_tuning(key, old)
    assert not failures, failures
