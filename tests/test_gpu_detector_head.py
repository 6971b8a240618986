"""The detector head of the instance_styleD step -- ``forward_features`` behind ``extract_feature`` and the loss of
``InstanceStyleDStep._body`` -- against the float64 reference of tests/detector_head_ref.py: every loss term and output, the gradient of
every parameter and of both feature maps, and one SGD(momentum) update on those gradients.

The reference is handed what the device drew (anchor targets, sampled rois and their targets, or the target-domain proposals) and
every ReLU mask of the device's own activations (RPN_Conv, netD_pixel's h1 / h2, the nine of layer4), so both sides compute the same
polynomial and each tensor can be held to  min(1e-4, max(16 e32, 1e-6))  of its largest element, e32 being the float32 CPU reference's
own error under the same masks.  tests/test_detector_head_ref_host.py shows on the CPU that fifteen wiring errors (a reversal layer's
sign or factor, a missing detach, a loss normalised over the wrong count, the wrong sigma, the class gather, a missing term of
base_feat.grad, the bias groups) each move a tensor by at least 10 x that bound.  Needs a real MI355X: `pytest -m gpu`."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detector_head_ref as R  # noqa: E402
from conftest import record_margin  # noqa: E402
from test_gpu_bottleneck_bwd import FLIP_BAND  # noqa: E402
from test_gpu_kernels import DEV  # noqa: E402

_CL = torch.channels_last
SAMPLE_SEED = 5
LR = 0.1


def _cl(t):
    return t.contiguous(memory_format=_CL)


@pytest.fixture(scope="module")
def head_cfg():
    """The head's config on the global cfg singleton, put back afterwards."""
    from i2vsgg_amd.model.utils import config as c
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    saved = copy.deepcopy(dict(c.cfg))
    c.cfg_from_file(c.default_cfg_file("res101"))
    c.cfg_from_list(R.CFG_LIST)
    yield c.cfg
    c._merge_a_into_b(c.AttrDict(saved), c.cfg)


def _node(fn, name, depth=6):
    """The nearest autograd node called ``name`` at or above ``fn``."""
    if fn is None or depth < 0:
        return None
    if type(fn).__name__ == name:
        return fn
    for nxt, _ in fn.next_functions:
        found = _node(nxt, name, depth - 1)
        if found is not None:
            return found
    return None


def _build(case):
    """The product's net holding the case's parameters -> (net, inputs, the reference's view of the DEVICE's parameters: state_dict
    values and layer4's folded scales as the kernels read them)."""
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.faster_rcnn.resnet_instance_styleD_bilinear import resnet
    c = R.CASES[case]
    params, inputs = R.make_params(case), R.make_inputs(0)
    with torch.random.fork_rng(devices=[]):             # the init draws from the global generator: leave it as found
        net = resnet(tuple(range(R.N_CLS)), 50, class_agnostic=c["agnostic"], ic=c["ic"], gc=c["gc"])
        net.create_architecture()
    r = load_reference_state(net, params, strict=False)
    assert not r.unexpected_keys and all(k.startswith("RCNN_base.") or "num_batches" in k for k in r.missing_keys), r
    net.to(DEV).train()
    dev_params = {k: v.detach().cpu() for k, v in net.state_dict().items() if k in params}
    assert all(torch.equal(dev_params[k], params[k]) for k in params)
    blocks = []
    for blk in net.RCNN_top[0]:
        b = dict(stride=blk.stride, wd=None, sd=None, bd=None, w1=blk.conv1.weight.detach().cpu(), w2=blk.conv2.weight.detach().cpu(),
                 w3=blk.conv3.weight.detach().cpu())
        bns = [("1", blk.bn1), ("2", blk.bn2), ("3", blk.bn3)]
        if blk.downsample is not None:
            b["wd"] = blk.downsample[0].weight.detach().cpu()
            bns.append(("d", blk.downsample[1]))
        for k, bn in bns:
            b["s" + k], b["b" + k] = (t.cpu() for t in bn.folded())
        blocks.append(b)
    return net, inputs, dev_params, blocks


def _run(net, case, inputs, ops, monkeypatch):
    """One forward + backward exactly as ``InstanceStyleDStep._body`` makes them for one domain -> dict(values, grads, masks, samples,
    nodes: what ran).  The host sampling path on a seeded ``np.random``."""
    from i2vsgg_amd import train
    c = R.CASES[case]
    for p in net.parameters():
        p.grad = None
    feat = _cl(inputs["feat"].to(DEV)).requires_grad_(True)
    feat1 = _cl(inputs["feat1"].to(DEV)).requires_grad_(True)
    info = torch.from_numpy(inputs["info"]).to(DEV)
    if c["target"]:
        gt, nb = torch.zeros((R.B, 1, 5), device=DEV), torch.zeros((R.B,), device=DEV)
    else:
        gt, nb = torch.from_numpy(inputs["gt"]).to(DEV), torch.from_numpy(inputs["num_boxes"]).to(DEV)
    seen = dict(rpn_conv=[], anchor=[], proposal=[], rois=[], pixel=[], top=[])
    real_conv = ops.conv2d

    def conv_spy(x, w, *a, **k):
        y = real_conv(x, w, *a, **k)
        if tuple(w.shape) == (512, 1024, 3, 3):
            seen["rpn_conv"].append(y)
        return y
    monkeypatch.setattr(ops, "conv2d", conv_spy)              # rpn.py looks ops.conv2d up by attribute
    atl = net.RCNN_rpn.RPN_anchor_target
    real_targets = atl.targets_yxa

    def targets_spy(*a, **k):
        out = real_targets(*a, **k)
        seen["anchor"].append(tuple(t.detach().cpu().numpy() for t in out))
        return out
    atl.targets_yxa = targets_spy
    hooks = [net.RCNN_proposal_target.register_forward_hook(lambda m, i, o: seen["proposal"].append(tuple(t.detach().cpu().numpy() for t in o))),
             net.RCNN_rpn.register_forward_hook(lambda m, i, o: seen["rois"].append(o[0].detach().cpu().numpy())),
             net.netD_pixel.register_forward_hook(lambda m, i, o: seen["pixel"].append((o[0] if isinstance(o, tuple) else o).grad_fn))]
    hooks += [blk.register_forward_hook(lambda m, i, o: seen["top"].append(o.grad_fn)) for blk in net.RCNN_top[0]]
    np.random.seed(SAMPLE_SEED)
    try:
        out = net.forward_features(feat, feat1, info, gt, nb, c["target"], R.ETA, R.ETA_STYLE)
    finally:
        del atl.targets_yxa
        for h in hooks:
            h.remove()
        monkeypatch.setattr(ops, "conv2d", real_conv)
    values = {}
    if c["target"]:
        d_inst, d_style = out
        values["dloss_t"], values["dloss_t_style"] = ops.half_mse(d_inst, 1.0), ops.half_mse(d_style, 1.0)
        total = values["dloss_t"] + R.STYLE_LAMBDA * values["dloss_t_style"]
        samples = dict(rois=seen["rois"][0])
        assert samples["rois"].shape == (R.B, R.ROIS, 5) and not seen["anchor"] and not seen["proposal"]
    else:
        _, cls_prob, bbox_pred, l_rpn_cls, l_rpn_box, l_cls, l_box, _, d_inst, d_style = out
        m1 = train._mean1
        values.update(rpn_cls=m1(l_rpn_cls), rpn_box=m1(l_rpn_box), rcnn_cls=m1(l_cls), rcnn_box=m1(l_box), cls_prob=cls_prob, bbox_pred=bbox_pred)
        loss = values["rpn_cls"] + values["rpn_box"] + values["rcnn_cls"] + values["rcnn_box"]
        values["dloss_s"], values["dloss_s_style"] = ops.half_mse(d_inst), ops.half_mse(d_style)
        total = loss + values["dloss_s"] + R.STYLE_LAMBDA * values["dloss_s_style"]
        assert len(seen["anchor"]) == 1 and len(seen["proposal"]) == 1
        samples = dict(anchor=seen["anchor"][0], proposal=seen["proposal"][0], rois=seen["proposal"][0][0])
    values.update(d_instance=d_inst, d_style=d_style, total=total)

    # ---- what ran, and every ReLU mask from the device's own activations (before the backward frees them)
    n_pixel = 2 if (c["ic"] and not c["target"]) else 1
    pix = [_node(fn, "_DPixelFnBackward") for fn in seen["pixel"]]
    assert len(pix) == n_pixel and all(n is not None for n in pix), "netD_pixel did not take the fused kernel"
    rows = R.B * R.ROIS
    masks = {}
    for n in pix:
        h1, h2 = n.saved_tensors[4], n.saved_tensors[5]
        assert tuple(h1.shape) == (rows * 49, 512) and tuple(h2.shape) == (rows * 49, 128)
        mk = tuple((h.detach() > 0).view(rows, 7, 7, -1).permute(0, 3, 1, 2).cpu() for h in (h1, h2))
        if "h1" in masks:
            assert torch.equal(mk[0], masks["h1"]) and torch.equal(mk[1], masks["h2"])           # the context call sees the same rows
        masks["h1"], masks["h2"] = mk
    if not c["target"]:
        assert len(seen["rpn_conv"]) == 1 and tuple(seen["rpn_conv"][0].shape) == (R.B, 512) + R.FEAT[2:]
        masks["rpn"] = (seen["rpn_conv"][0].detach() > 0).cpu()
        assert len(seen["top"]) == 3 and all(type(fn).__name__ == "_BottleneckFnBackward" for fn in seen["top"]), \
            "layer4's blocks did not run as single nodes"
        masks["top"] = [tuple((t.detach() > 0).cpu() for t in fn.saved_tensors[1:4]) for fn in seen["top"]]
        assert tuple(masks["top"][0][2].shape) == (rows, 2048, 4, 4)
    else:
        assert not seen["top"]
    total.backward()
    grads = {"base_feat": feat.grad, "base_feat1": feat1.grad}
    grads.update({k: p.grad for k, p in net.named_parameters()})
    return dict(values={k: v.detach().clone() for k, v in values.items()}, masks=masks, samples=samples,
                grads={k: (None if g is None else g.detach().clone()) for k, g in grads.items()})


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        keys = lambda d: {k for k in d if not k.startswith("_")}          # ("_mats": the reference's cached RoIAlign matrices)
        return keys(a) == keys(b) and all(_same(a[k], b[k]) for k in keys(a))
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def _reference(case, inputs, params, blocks, run, cache):
    """The float64 reference under the run's samples and masks with its e32 table; the ordered runs draw the same samples and
    (nearly always) make the same masks, and then take the first run's reference."""
    for samples, masks, ref, e32 in cache:
        if _same(samples, run["samples"]) and _same(masks, run["masks"]):
            return ref, e32
    ref = R.run(case, inputs, params, blocks, run["samples"], masks=run["masks"])
    e32 = R.e32_table(case, inputs, params, blocks, run["samples"], ref)
    cache.append((run["samples"], run["masks"], ref, e32))
    return ref, e32


def _hold_to_reference(test, case, run, ref, e32):
    """Every figure is recorded before anything is asserted -> the failures."""
    c, failures = R.CASES[case], []
    record_margin(test, "netD_style |z| / rms, smallest (bound: at least)", ref["margins"]["style_z"], R.Z_MARGIN)
    if not c["target"]:
        record_margin(test, "smooth-L1 distance from the switch, smallest (bound: at least)", ref["margins"]["smooth_l1"], R.SL1_MARGIN)
    if not R.conditions_hold(ref):
        failures.append(("the case's conditions do not hold on the device's samples", ref["margins"]))
    if not c["target"]:
        R.check_anchor_labels(run["samples"]["anchor"][0])
    # ---- forward values
    assert set(run["values"]) == set(ref["values"]), (sorted(run["values"]), sorted(ref["values"]))
    for k in sorted(ref["values"]):
        err, bound = R.rel_max(run["values"][k], ref["values"][k]), R.gpu_bound(e32[k])
        record_margin(test, "value %s (e32 %.3g)" % (k, e32[k]), err, bound)
        if not err <= bound:
            failures.append((k, err, bound))
    # ---- the masks are the device's; they may differ from the reference's own choice only within rounding of zero
    pres = [("rpn", ref["pre"].get("rpn"), run["masks"].get("rpn")), ("h1", ref["pre"]["h1"], run["masks"]["h1"]),
            ("h2", ref["pre"]["h2"], run["masks"]["h2"])]
    for i, (pr, mk) in enumerate(zip(ref["pre"].get("top", []), run["masks"].get("top", []))):
        pres += [("top%d.%s" % (i, n), p, m) for n, p, m in zip(("a1", "a2", "out"), pr, mk)]
    n_flip = n_band = n_all = 0
    for what, pre, m in pres:
        if pre is None:
            continue
        flips, band = m != (pre > 0), pre.abs() <= FLIP_BAND * pre.abs().max()
        n_flip, n_band, n_all = n_flip + int(flips.sum()), n_band + int(band.sum()), n_all + pre.numel()
        if bool((flips & ~band).any()):
            failures.append(("%s mask flips away from zero" % what, float((pre.abs() * flips).max() / pre.abs().max())))
    record_margin(test, "mask flips (fraction; bound: the band's share)", n_flip / n_all, n_band / n_all)
    # ---- gradients: presence, exact zeros, size
    want = {k: v for k, v in ref["grads"].items() if v is not None}
    have = {k: v for k, v in run["grads"].items() if v is not None}
    if sorted(want) != sorted(have):
        failures.append(("gradient presence", sorted(set(want) ^ set(have))))
    for k in sorted(set(want) & set(have)):
        got = have[k].double().cpu()
        zero = want[k] == 0
        # Exact zeros as zeros: bbox_pred rows of classes no sampled row carries; base_feat.grad at the pixels no ROI reaches, in the
        # target cases, where RoIAlign's backward is its only contributor.  In a source case the RPN's 3x3 data gradient reaches
        # every pixel, and it is the Winograd F(4x4,3x3) form (conv_route.plan_conv: "even where the forward may not"): a pixel whose
        # 3x3 neighbourhood holds only unlabelled anchors is an exact zero in float64 and cancellation residue of its 6x6 tile on the
        # device (999 of 1024 such entries not zero, all below 3e-6 of the tensor's largest element: the tensor's own bound holds them)
        if (k == "RCNN_bbox_pred.weight" or (k == "base_feat" and c["target"])) and bool(zero.any()):
            wrong = int((got[zero] != 0).sum())
            record_margin(test, "grad %s: entries not zero where float64 is exactly zero (of %d)" % (k, int(zero.sum())), wrong, 0)
            if wrong:
                failures.append((k, "not zero where the reference is exactly zero", wrong))
        err, bound = R.rel_max(got, want[k]), R.gpu_bound(e32[k])
        record_margin(test, "grad %s (e32 %.3g)" % (k, e32[k]), err, bound)
        if not err <= bound:
            failures.append((k, err, bound))
    if not c["target"] and not c["agnostic"]:
        labels = set(int(v) for v in np.asarray(run["samples"]["proposal"][1]).reshape(-1)) - {0}     # a background row has no box loss
        rows = want["RCNN_bbox_pred.weight"].view(R.N_CLS, 4, -1)
        unused = [k for k in range(R.N_CLS) if k not in labels]
        assert unused and all(bool((rows[k] == 0).all()) for k in unused) and all(bool((rows[k] != 0).any()) for k in labels)
    if c["target"]:
        assert bool((want["base_feat"] == 0).any())                 # pixels no proposal reaches
    return failures


def _hold_update(test, net, run, ref, e32):
    """One FusedSGD step on the gradients just checked, from a loaded non-zero momentum, against float64 SGD -> the failures."""
    from i2vsgg_amd.optim import make_optimizer
    failures = []
    named = list(net.named_parameters())
    opt = make_optimizer("sgd", named, lr=LR)
    g_ref = {k: v for k, v in ref["grads"].items() if v is not None and k not in ("base_feat", "base_feat1")}
    m0 = R.momentum_like(g_ref)
    gen = torch.Generator().manual_seed(9)
    sd = opt.state_dict()
    names = [grp["name"] for grp in sd["param_groups"]]
    for i, k in enumerate(names):
        if k not in m0:                                              # a parameter without a gradient: its momentum must stay as loaded
            m0[k] = torch.randn(sd["state"][i]["momentum_buffer"].shape, generator=gen) * 1e-3
        sd["state"][i]["momentum_buffer"] = m0[k].to(DEV)
    opt.load_state_dict(sd)
    params = dict(named)
    p0 = {k: p.detach().clone() for k, p in named}
    other_order = 0
    for k, p in named:
        g = run["grads"][k]
        p.grad = None if g is None else g.clone()
        other_order += int(g is not None and g.stride() != p.stride())
    opt.step()
    torch.cuda.synchronize()
    m1_ref, p1_ref = R.sgd({k: p0[k].cpu() for k in g_ref}, g_ref, m0, LR)
    moment = {it["name"]: it["m"] for it in opt.items}
    for k in sorted(g_ref):
        bound = R.gpu_bound(e32[k]) * float(g_ref[k].abs().max())
        bm = bound + 2.0 ** -23 * float(m0[k].abs().max())
        em = float((moment[k].double().cpu() - m1_ref[k]).abs().max())
        record_margin(test, "m1 %s (absolute)" % k, em, bm)
        lr_k = R.group_of(k, LR)[0]
        bp = lr_k * bm + 2.0 ** -23 * float(p0[k].abs().max())
        ep = float(((params[k].detach().double() - p0[k].double()).cpu() - (p1_ref[k] - p0[k].double().cpu())).abs().max())
        record_margin(test, "p1 - p0 %s (absolute)" % k, ep, bp)
        if not (em <= bm and ep <= bp):
            failures.append(("update", k, em, bm, ep, bp))
    still = [k for k, p in named if k not in g_ref]
    moved = [k for k in still if not torch.equal(params[k].detach(), p0[k])]
    moved += ["momentum of " + k for k in still if k in moment and not torch.equal(moment[k].cpu(), m0[k])]
    if moved:
        failures.append(("parameters without a gradient changed", moved[:8]))
    print("%s: %d gradients reach the update in other strides than their parameter's" % (test, other_order))
    for p in net.parameters():
        p.grad = None
    return failures


@pytest.mark.parametrize("case", list(R.CASES))
def test_detector_head_vs_masked_float64_reference(head_cfg, monkeypatch, case):
    from i2vsgg_amd import launch, ops
    from i2vsgg_amd.model.faster_rcnn import resnet_instance_styleD_bilinear as model
    # ---- the preconditions the case relies on: it cannot pass by silently taking another path
    assert ops.BLOCK_FUSED and ops.WINOGRAD_TRAIN and model.FUSED_STYLE and launch.WGRAD_BRANCH is None
    net, inputs, params, blocks = _build(case)
    assert not net.RCNN_rpn.RPN_anchor_target.device_sampling and not net.RCNN_proposal_target.device_sampling
    test = "test_detector_head[%s]" % case
    cache = []
    run = _run(net, case, inputs, ops, monkeypatch)
    ref, e32 = _reference(case, inputs, params, blocks, run, cache)
    failures = _hold_to_reference(test, case, run, ref, e32)

    # ---- ordered sums: the same figures, and the same bits twice
    ctx = launch.LaunchContext(DEV, ordered=True)
    runs = []
    for _ in range(3):
        with ctx:
            runs.append(_run(net, case, inputs, ops, monkeypatch))
            torch.cuda.synchronize()
        ctx.fit()
    ref_o, e32_o = _reference(case, inputs, params, blocks, runs[1], cache)
    failures += [("ordered",) + tuple(f) for f in _hold_to_reference(test + " ordered", case, runs[1], ref_o, e32_o)]
    for kind in ("values", "grads"):
        for k, a in runs[1][kind].items():
            b = runs[2][kind][k]
            if (a is None) != (b is None) or (a is not None and not torch.equal(a, b)):
                failures.append(("ordered runs differ in bits", kind, k))

    # ---- the update
    failures += _hold_update(test, net, run, ref, e32)
    assert not failures, failures
