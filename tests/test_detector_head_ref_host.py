"""The float64 reference of the detector head (tests/detector_head_ref.py) checked on its own, on the CPU: without masks it is the
composition of the ``oracle.nets`` functions; its gradients agree with central differences; evaluated in float32 under the float64
run's masks it sits at float32 rounding (``e32``, the figure the GPU bound is made of); and every planted error moves a gradient, or
the update, by at least 10 x the bound tests/test_gpu_detector_head.py holds the device to."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detector_head_ref as R
from oracle import cops, nets, rpn as orpn


@pytest.fixture(scope="module")
def head_cfg():
    """The head's config on the global cfg singleton, put back afterwards."""
    from i2vsgg_amd.model.utils import config as c
    saved = copy.deepcopy(dict(c.cfg))
    c.cfg_from_file(c.default_cfg_file("res101"))
    c.cfg_from_list(R.CFG_LIST)
    yield c.cfg
    c._merge_a_into_b(c.AttrDict(saved), c.cfg)


@pytest.fixture(scope="module")
def built(head_cfg):
    """case -> (the built case, its float64 run with gradients under its own masks, its e32 table), each made once."""
    cache = {}

    def get(case):
        if case not in cache:
            b = R.build_case(case)
            ref = R.run(case, b["inputs"], b["params"], b["blocks"], b["samples"])
            assert R.conditions_hold(ref), ref["margins"]
            cache[case] = (b, ref, R.e32_table(case, b["inputs"], b["params"], b["blocks"], b["samples"], ref))
        return cache[case]
    yield get
    cache.clear()


def test_cases_hold_what_they_are_built_for(built):
    for case, c in R.CASES.items():
        b, ref, _ = built(case)
        s = b["samples"]
        assert tuple(b["inputs"]["feat"].shape) == R.FEAT and tuple(b["inputs"]["feat1"].shape) == R.FEAT1
        zeros = float((b["inputs"]["feat"] == 0).float().mean())
        assert 0.45 < zeros < 0.55 and float(b["inputs"]["feat"].min()) == 0.0
        assert np.asarray(s["rois"]).reshape(-1, 5).shape == (R.B * R.ROIS, 5)
        assert ref["values"]["d_instance"].shape == (16, 1, 7, 7)                    # 784 rows: a ragged last 32-row tile
        if not c["target"]:
            R.check_anchor_labels(s["anchor"][0])
            labels = np.asarray(s["proposal"][1]).reshape(-1)
            assert (labels > 0).any() and (labels == 0).any() and len(set(labels[labels > 0])) < R.N_CLS - 1
            assert b["params"]["RCNN_cls_score.weight"].shape[1] == R.feat_d(case)
        print("%-15s seed %d  margins %s  total %.4f" % (case, b["seed"], ref["margins"], float(ref["values"]["total"])))


# ---------------------------------------------------------------------------------------------------------------------
# unmasked == the oracle's functions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_unmasked_reference_equals_the_composition_of_oracle_functions(built, case):
    """``oracle.nets`` (rpn_head, netd_style, netd_pixel, head_to_tail with the raw BatchNorms) fed float64 parameters,
    ``F.cross_entropy`` in the reference's own (a, y, x) anchor order and ``oracle.rpn.smooth_l1``, on the host's stored samples: 1e-12
    relative.  Two exceptions, both of the yardstick's making: ``oracle.rpn.smooth_l1`` rounds its argument to float32 (its F32 casts),
    so the two box losses are held to 2^-20; and the pooled rows, a float64 matrix product here, are compared with the float32
    ``cops.roi_align_avg_fwd`` at 2^-20 and then handed on, so that everything behind them is again a 1e-12 comparison."""
    c = R.CASES[case]
    b, _, _ = built(case)
    inputs, params, samples = b["inputs"], b["params"], b["samples"]
    with torch.no_grad():
        out = R.run(case, inputs, params, R.top_blocks(params, torch.float64), samples, want_grad=False)
    v = out["values"]
    p = {k: t.double() for k, t in params.items()}
    feat, feat1 = inputs["feat"].double(), inputs["feat1"].double()
    tol, tol32 = 1e-12, 2.0 ** -20
    close = lambda got, want, t=tol: R.rel_max(got, want) <= t
    with torch.no_grad():
        sty = nets.netd_style(feat1, p, R.ETA_STYLE, context=c["gc"])
        d_style, z = sty if c["gc"] else (sty, None)
        assert close(v["d_style"], d_style)
        rois = np.asarray(samples["rois"], np.float32).reshape(-1, 5)
        pooled = out["stages"]["pool"]
        assert close(pooled, torch.from_numpy(cops.roi_align_avg_fwd(inputs["feat"].numpy(), rois, 7, 7, 1 / 16.0)), tol32)
        pix = nets.netd_pixel(pooled, p, R.ETA, context=c["ic"])
        d_inst, fi = pix if c["ic"] else (pix, None)
        assert close(v["d_instance"], d_inst)
        if c["target"]:
            assert close(v["dloss_t"], 0.5 * torch.mean((1 - d_inst) ** 2)) and close(v["dloss_t_style"], 0.5 * torch.mean((1 - d_style) ** 2))
            assert close(v["total"], 0.5 * torch.mean((1 - d_inst) ** 2) + R.STYLE_LAMBDA * 0.5 * torch.mean((1 - d_style) ** 2))
            return
        cls, _, box = nets.rpn_head(feat, p)
        Bn, A2, H, W = cls.shape
        A = A2 // 2
        labels, tg, inw, outw = (np.asarray(t) for t in samples["anchor"])
        score = cls.view(Bn, 2, A * H * W).permute(0, 2, 1).reshape(-1, 2)                 # rpn.py:76-84: (a, y, x) order
        lab = torch.from_numpy(labels).reshape(Bn, H, W, A).permute(0, 3, 1, 2).reshape(-1).long()
        assert close(v["rpn_cls"], F.cross_entropy(score[lab >= 0], lab[lab >= 0]))
        nchw = lambda t: np.ascontiguousarray(t.reshape(Bn, H, W, 4 * A).transpose(0, 3, 1, 2))
        rep = lambda t: np.repeat(t[:, :, None], 4, 2)
        want = orpn.smooth_l1(box.numpy(), nchw(tg), nchw(rep(inw)), nchw(rep(outw)), sigma=3.0, sum_dims=(1, 2, 3))
        assert abs(float(v["rpn_box"]) - float(want)) <= tol32 * abs(float(want))
        x = nets.head_to_tail(pooled, p)
        if c["gc"]:
            x = torch.cat((z.unsqueeze(1).repeat(1, R.ROIS, 1).view(-1, z.size(1)), x), 1)
        if c["ic"]:
            x = torch.cat((fi.view(fi.size(0), -1), x), 1)
        _, plabels, ptg, pinw, poutw = (np.asarray(t) for t in samples["proposal"])
        plab = torch.from_numpy(plabels).reshape(-1).long()
        bp = F.linear(x, p["RCNN_bbox_pred.weight"], p["RCNN_bbox_pred.bias"])
        if not c["agnostic"]:
            bp = torch.stack([bp[i, 4 * int(k):4 * int(k) + 4] for i, k in enumerate(plab)])
        score = F.linear(x, p["RCNN_cls_score.weight"], p["RCNN_cls_score.bias"])
        assert close(v["bbox_pred"], bp) and close(v["cls_prob"], F.softmax(score, 1))
        assert close(v["rcnn_cls"], F.cross_entropy(score, plab))
        want = orpn.smooth_l1(bp.numpy(), ptg.reshape(-1, 4), pinw.reshape(-1, 4), poutw.reshape(-1, 4), sigma=1.0, sum_dims=(1,))
        assert abs(float(v["rcnn_box"]) - float(want)) <= tol32 * abs(float(want))
        assert close(v["dloss_s"], 0.5 * torch.mean(d_inst ** 2)) and close(v["dloss_s_style"], 0.5 * torch.mean(d_style ** 2))
        parts = sum(float(v[k]) for k in ("rpn_cls", "rpn_box", "rcnn_cls", "rcnn_box", "dloss_s")) + R.STYLE_LAMBDA * float(v["dloss_s_style"])
        assert abs(float(v["total"]) - parts) <= tol * parts


# ---------------------------------------------------------------------------------------------------------------------
# central differences
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["context", "target_context"])
def test_float64_gradients_against_central_differences(built, case):
    """Two entries of every parameter tensor and of both maps: (L(t + h) - L(t - h)) / 2h of the float64 loss, evaluated under the
    run's own masks and choices (so L is smooth: sums, products, a root away from zero, sigmoids, softmaxes), against float64 autograd.
    Only the stages behind the moved tensor are computed again (``dirty_stages``).

    What a gradient is the derivative OF.  For a parameter: the total loss.  For an entry of a map, autograd's answer is by design
    not the derivative of the total: the reversal layers turn the adversarial terms' share round and scale it, and ``.detach()``
    cuts the context vectors.  It is the derivative of  total - (1 + eta) d_inst term - (1 + eta_style) style_lambda d_style term
    with the context vectors held constant, and that is what is differenced along a map.

    The bound.  D(h) = L' + h^2 L''' / 6 + O(h^4), so D(2h) - D(h) = h^2 L''' / 2 + O(h^4): a third of that difference is the
    third-derivative term of D(h), measured; it is allowed twice, which covers the O(h^4) remainder as long as that is smaller than
    the leading term.  Rounding: each loss is a float64 evaluation whose longest reduction is RPN_Conv's 9216 terms, n u |L| at
    worst (u = 2^-53), two of them divided by 2h:  9216 u max(1, |L|) / h.  h is 1e-3 of the tensor's largest entry."""
    b, ref, _ = built(case)
    inputs = {k: (v.double() if torch.is_tensor(v) else v) for k, v in b["inputs"].items()}
    params = {k: v.double() for k, v in b["params"].items()}
    blocks = [{k: (v.double() if torch.is_tensor(v) else v) for k, v in blk.items()} for blk in b["blocks"]]
    tensors = {"base_feat": inputs["feat"], "base_feat1": inputs["feat1"]}
    tensors.update({k: v for k, v in params.items() if not k.startswith("RCNN_top.")})
    for i, blk in enumerate(blocks):
        tensors.update({"RCNN_top.0.%d.%s" % (i, R.TOP_NAMES[n]): blk[n] for n in R.TOP_NAMES if blk[n] is not None})
    g = {k: v for k, v in ref["grads"].items() if v is not None}
    assert set(g) <= set(tensors)

    adv = ("dloss_t", "dloss_t_style") if R.CASES[case]["target"] else ("dloss_s", "dloss_s_style")

    def loss_at(name, idx, h):
        t = tensors[name]
        old = float(t[idx])
        a_map = name in ("base_feat", "base_feat1")
        try:
            t[idx] = old + h
            with torch.no_grad():
                out = R.run(case, inputs, params, blocks, b["samples"], masks=ref["masks"], choices=ref["choices"], want_grad=False,
                            reuse=ref["stages"], dirty=R.dirty_stages(name), context=ref["context"] if a_map else None)
        finally:
            t[idx] = old
        v = {k: float(x) for k, x in out["values"].items() if x.numel() == 1}
        if not a_map:
            return v["total"]
        return v["total"] - (1 + R.ETA) * v[adv[0]] - (1 + R.ETA_STYLE) * R.STYLE_LAMBDA * v[adv[1]]

    assert abs(loss_at("netD_pixel.conv3.weight", (0, 0, 0, 0), 0.0) -float(ref["values"]["total"])) <= 1e-13        # the staged route is the plain route
    u, L = 2.0 ** -53, abs(float(ref["values"]["total"]))
    rng = np.random.default_rng(11)
    worst, n = 0.0, 0
    for name in sorted(g):
        gk = g[name]
        live = torch.nonzero(gk.abs() >= 0.1 * gk.abs().max())          # entries that carry gradient: 0 == 0 checks nothing
        for k in rng.choice(len(live), min(2, len(live)), replace=False):
            idx = tuple(int(v) for v in live[k])
            h = 1e-3 * float(tensors[name].abs().max())
            d1 = (loss_at(name, idx, h) - loss_at(name, idx, -h)) / (2 * h)
            d2 = (loss_at(name, idx, 2 * h) - loss_at(name, idx, -2 * h)) / (4 * h)
            bound = 2 * abs(d2 - d1) / 3 + 9216 * u * max(1.0, L) / h
            an = float(gk[idx])
            worst, n = max(worst, bound / abs(an)), n + 1
            if bound > 0.01 * abs(an):
                print("wide: %s %s h %.3g  truncation %.3g rounding %.3g entry %.3g" % (name, idx, h, 2 * abs(d2 - d1) / 3,
                                                                                       9216 * u * max(1.0, L) / h, an))
            assert abs(d1 - an) <= bound, (name, idx, h, d1, d2, an, bound)
    print("%s: %d entries of %d tensors, largest bound / |gradient entry| %.3g" % (case, n, len(g), worst))
    assert worst < 0.05          # the check has teeth: a bound never wider than 5 % of the entry it holds


# ---------------------------------------------------------------------------------------------------------------------
# float32 against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_float32_reference_under_the_float64_masks(built, case):
    """e32 per tensor: at most 1e-5, or the case is ill-conditioned."""
    _, ref, e32 = built(case)
    for k in sorted(e32):
        print("e32 %-15s %-40s %.3g   gpu bound %.3g" % (case, k, e32[k], R.gpu_bound(e32[k])))
    assert set(e32) == set(ref["values"]) | {k for k, v in ref["grads"].items() if v is not None}
    bad = {k: v for k, v in e32.items() if not v <= 1e-5}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------------------------------------
def test_sgd_equals_torch_sgd_in_float64(built, head_cfg):
    """``R.sgd`` against torch.optim.SGD on float64 copies carrying the reference's own gradients, with the loop's two param groups
    (trainval_net_instance_styleD_bilinear.py:134-148 through cfg.TRAIN) and a loaded non-zero momentum: the same expression, one
    of the two may fuse a product into its sum, 4 u of the operands' magnitudes per element (u = 2^-53)."""
    T = head_cfg.TRAIN
    b, ref, _ = built("target_context")
    g = {k: v for k, v in ref["grads"].items() if v is not None and k in b["params"]}
    names, m0 = sorted(g), R.momentum_like(g)
    m1, p1 = R.sgd(b["params"], g, m0, 0.1)
    ps = [b["params"][k].double().clone().requires_grad_() for k in names]
    groups = [{"params": [q], "lr": 0.1 * (T.DOUBLE_BIAS + 1) if "bias" in k else 0.1,
               "weight_decay": (T.WEIGHT_DECAY if T.BIAS_DECAY else 0.0) if "bias" in k else T.WEIGHT_DECAY} for k, q in zip(names, ps)]
    opt = torch.optim.SGD(groups, lr=0.1, momentum=T.MOMENTUM)
    sd = opt.state_dict()
    sd["state"] = {i: {"momentum_buffer": m0[k].double().clone()} for i, k in enumerate(names)}
    opt.load_state_dict(sd)
    for k, q in zip(names, ps):
        q.grad = g[k].clone()
    opt.step()
    assert T.MOMENTUM > 0 and T.WEIGHT_DECAY > 0 and any("bias" in k for k in names)
    u = 2.0 ** -53
    for k, q in zip(names, ps):
        lr_k, wd_k = R.group_of(k, 0.1)
        p0, m_t = b["params"][k].double(), opt.state[q]["momentum_buffer"]
        size_m = (T.MOMENTUM * m0[k].double()).abs() + g[k].abs() + (wd_k * p0).abs()
        assert bool(((m1[k] - m_t).abs() <= 4 * u * size_m).all()), k
        assert bool(((p1[k] - q.detach()).abs() <= 4 * u * (p0.abs() + lr_k * m_t.abs() + lr_k * size_m)).all()), k     # (m1's own 4 u, times lr)


# ---------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------
# the cases a plant is looked for in, in order (the first that shows it at 10 x ends the search)
_ORDER = ("target_plain", "target_context", "context", "agnostic_ic", "plain")


@pytest.mark.parametrize("plant", R.PLANTS)
def test_planted_error_moves_a_tensor_by_ten_times_its_gpu_bound(built, plant):
    rows, shown = [], False
    for case in [c for c in _ORDER if R.plant_applies(plant, c)]:
        b, ref, e32 = built(case)
        g = {k: v for k, v in ref["grads"].items() if v is not None}
        if plant in R.OPTIMISER_PLANTS:
            p0 = {k: v for k, v in b["params"].items()}
            m0 = R.momentum_like(g)
            m1, p1 = R.sgd(p0, g, m0, 0.1)
            m1w, p1w = R.sgd(p0, g, m0, 0.1, plant)
            moved = {}
            for k in m1:
                bound = R.gpu_bound(e32[k])
                bm = bound + 2.0 ** -23 * float(m0[k].abs().max()) / float(g[k].abs().max())
                moved["m1 " + k] = R.rel_max(m1w[k], m1[k]) * float(m1[k].abs().max()) / float(g[k].abs().max()) / bm
                step, stepw = p1[k] - p0[k].double(), p1w[k] - p0[k].double()
                lr_k = R.group_of(k, 0.1)[0]
                bp = lr_k * bound * float(g[k].abs().max()) + 2.0 ** -23 * float(p0[k].abs().max())
                moved["p1 " + k] = float((stepw - step).abs().max()) / bp
        else:
            wrong = R.run(case, b["inputs"], b["params"], b["blocks"], b["samples"], masks=ref["masks"], choices=ref["choices"], plant=plant)
            # a gradient the plant removes altogether counts as moved by the whole tensor
            moved = {k: (R.rel_max(wrong["grads"][k], g[k]) if wrong["grads"][k] is not None else 1.0) / R.gpu_bound(e32[k]) for k in g}
        k = max(moved, key=moved.get)
        rows.append((case, k, moved[k]))
        print("plant %-34s %-15s %-44s moved by %.3g x its bound" % (plant, case, k, moved[k]))
        if moved[k] >= 10.0:
            shown = True
            break
    assert shown, rows
