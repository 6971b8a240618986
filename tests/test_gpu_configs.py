"""The BASELINE.json configs at FULL size on the GPU (600x1000 frames), through size-independent properties and, where a
CPU restatement finishes in seconds, against the oracle.

configs[2]  cfgs/res101.yml, instance_styleD D+G adversarial step, 4 source + 4 target frames
            (trainval_net_instance_styleD_bilinear.py:262-341)
configs[0]  cfgs/res50.yml, one 1x3x600x1000 frame, Faster-RCNN forward + SGG_emb head (cfgs/res50.yml:1-17)
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from i2vsgg_amd import synthetic as syn  # noqa: E402

from conftest import record_margin  # noqa: E402

DEV = "cuda:0"
TARGET_SET_OVERLAP = 30 / 32     # of the oracle's 32 target proposals at most two may differ (observed 31 / 32: profiles/r06_parity_margins.txt; rounds 1-5: 0.9)
SET = ["ANCHOR_SCALES", "[8, 16, 32]", "ANCHOR_RATIOS", "[0.5,1,2]", "MAX_NUM_GT_BOXES", "30"]


@pytest.fixture()
def fresh_cfg():
    """A test here loads its own yml; the global cfg singleton is put back afterwards (other modules load res101)."""
    from i2vsgg_amd.model.utils import config as c
    saved = copy.deepcopy(dict(c.cfg))

    def load(net, extra=()):
        c.cfg_from_file(c.default_cfg_file(net))
        c.cfg_from_list(SET + list(extra))
        return c.cfg
    yield load
    c._merge_a_into_b(c.AttrDict(saved), c.cfg)


def _finite(d):
    return all(np.isfinite(float(v)) for v in d.values())


def test_instance_styled_step_full_size(fresh_cfg):
    _step_full_size(fresh_cfg, 32)


def test_instance_styled_step_full_size_at_128_rois(fresh_cfg):
    """The same at the yml's own TRAIN.BATCH_SIZE = RPN_POST_NMS_TOP_N_TARGET = 128: 512 ROIs (25 088 pooled rows) per branch,
    keep buffers of (4, 128) with up to 32 foreground rows per frame.  The plain form is handed the fused form's proposals
    (see _step_full_size)."""
    _step_full_size(fresh_cfg, 128)


def _step_full_size(fresh_cfg, R):
    """configs[2] at full size, B = 4 + 4 frames of 600x1000, ResNet-101, R ROI / frame:
      * every loss of the step is finite and the trained parameters of every group move (layer1-3, layer4, RPN, both
        discriminators, the detection heads);
      * the step on the fused kernels (one-kernel netD_pixel, Winograd forward / data gradient for the trained 3x3 layers,
        stride-1 bottlenecks as single autograd nodes with the BN-scale / ReLU-mask / skip-gradient passes folded into the
        gradient kernels, multi-tensor fused SGD) reproduces the losses of the same step on the plain forms (layer-by-layer netD_pixel,
        direct 3x3 kernels, torch.optim.SGD with the reference's parameter groups) for two consecutive steps -- the second
        one sees the first one's update -- within 1e-3 relative, same np.random stream;
      * the captured form (device-side target sampling, ONE HIP graph) replays to finite losses close to the host-sampled
        ones and keeps training.
    At R = 128 the plain form's RPN hands on the fused form's proposals of the same step (its own RPN losses still count).
    The two backbones differ in the last bits (Winograd against direct 3x3 kernels: 1e-5 against 1e-6 per layer), which
    moves proposal corners by ~1e-4 px and lets a score near-tie swap a box.  At 4 x 128 sampled rows such a swapped box is
    sampled: at step 0, 503 of 504 distinct sampled boxes agree, and the one that differs moves RCNN_loss_cls by 7.9e-5 and
    every gradient behind the ROIs by ~2e-3.  After the update, 443 of 505 agree and RCNN_loss_cls differs by 6.4e-3.  That is
    sampling, not arithmetic, so the forms are compared on equal proposals."""
    cfg = fresh_cfg("res101", ["TRAIN.BATCH_SIZE", str(R), "TRAIN.RPN_POST_NMS_TOP_N_TARGET", str(R)])
    from i2vsgg_amd import ops, train
    names = ["RCNN_base.4.0.conv1.weight", "RCNN_base.6.22.conv2.weight", "RCNN_top.0.2.conv3.weight",
             "RCNN_rpn.RPN_Conv.weight", "netD_pixel.conv1.weight", "netD_style.fc_1.weight", "RCNN_cls_score.weight",
             "RCNN_bbox_pred.bias"]

    def run(plain, proposals=None):
        torch.manual_seed(0)
        np.random.seed(cfg.RNG_SEED)
        net = train.build_instance_styled_net(101, device=DEV)
        before = {k: v.detach().clone() for k, v in net.named_parameters() if k in names}
        step = train.InstanceStyleDStep(net, 4, seed=3, device=DEV)
        seen = []
        if R != 32:                          # record the proposals (fused form) or hand on the recorded ones (plain form)
            rpn_forward = net.RCNN_rpn.forward

            def spy(*a, **k):
                out = rpn_forward(*a, **k)
                if proposals is not None:
                    out = (proposals[len(seen)],) + tuple(out[1:])
                seen.append(out[0].detach().clone())
                return out
            net.RCNN_rpn.forward = spy
        saved = (ops.WINOGRAD_TRAIN, net.netD_pixel.forward, ops.BLOCK_FUSED)      # WINOGRAD_TRAIN off: direct wgrad too
        if plain:
            ops.WINOGRAD_TRAIN = False
            ops.BLOCK_FUSED = False          # every conv its own autograd node, separate scale / mask passes
            net.netD_pixel.forward = net.netD_pixel._forward_layers
            T = cfg.TRAIN
            groups = [{"params": [p], "lr": 5e-4 * ((T.DOUBLE_BIAS + 1) if "bias" in n else 1),
                       "weight_decay": (T.WEIGHT_DECAY if T.BIAS_DECAY else 0.0) if "bias" in n else T.WEIGHT_DECAY}
                      for n, p in net.named_parameters() if p.requires_grad]        # trainval_net_instance...:134-148
            sgd = torch.optim.SGD(groups, momentum=T.MOMENTUM)

            class Plain:
                params = staticmethod(lambda: [g["params"][0] for g in groups])
                zero_grad = staticmethod(lambda: sgd.zero_grad(set_to_none=True))
                step = staticmethod(sgd.step)
                bump = staticmethod(lambda: None)
            step.opt = Plain
        try:
            out = []
            for _ in range(2):
                step()
                out.append({k: float(v) for k, v in step.losses.items()})
            moved = {k: float((dict(net.named_parameters())[k].detach() - before[k]).abs().max()) for k in names}
        finally:
            ops.WINOGRAD_TRAIN, net.netD_pixel.forward, ops.BLOCK_FUSED = saved
            if R != 32:
                del net.RCNN_rpn.forward
        return out, moved, net, step, seen

    fused, moved, net, step, proposals = run(False)
    assert all(_finite(d) for d in fused), fused
    assert all(v > 0 for v in moved.values()), moved
    plain, _, net2, step2, _ = run(True, proposals if R != 32 else None)
    del net2, step2
    tag = "step_full_size" + ("" if R == 32 else "[R=%d]" % R)
    for i, (a, b) in enumerate(zip(fused, plain)):
        if R != 32:
            record_margin(tag, "fused vs plain, equal proposals, step %d: max rel. loss diff" % i,
                          max(abs(a[k] - b[k]) / max(abs(b[k]), 1e-6) for k in a), 1e-3)
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-3 * max(abs(b[k]), 1e-6), (k, fused, plain)
    # ---- captured form (device-side sampling, ONE graph) against the host form AT EQUAL SAMPLES (round-3 review: the 25 % band
    # that stood here could hide a labelling error).  The target layers record what the device samplers drew inside the replay
    # (anchor labels after subsampling; kept roi indices + foreground counts); the training state is rewound to where the replay
    # started and the same step runs on eager launches with the host-side code path of both layers fed those samples instead of
    # np.random draws: all ten losses agree to 1e-3.
    atl, ptl = net.RCNN_rpn.RPN_anchor_target, net.RCNN_proposal_target
    atl.sample_record, ptl.sample_record = {}, {}
    assert step.capture(warmup=1, restore=True), step.graph_error      # the warm-up step (eager, device samplers) makes the buffers
    w0 = net.RCNN_base[6][22].conv2.weight.detach().clone()
    saved = step._snapshot()
    step()
    torch.cuda.synchronize()
    got = {k: float(v) for k, v in step.losses.items()}
    drawn_a = {k: v.clone() for k, v in atl.sample_record.items()}
    drawn_p = {k: v.clone() for k, v in ptl.sample_record.items()}
    assert _finite(got), got
    assert not torch.equal(w0, net.RCNN_base[6][22].conv2.weight.detach())
    # what the device samplers drew is a legal draw of the reference's rules (anchor_target_layer.py:123-143,
    # proposal_target_layer_cascade.py:140-182): <= 128 fg and exactly RPN_BATCHSIZE labelled anchors per frame (there are far
    # more than 256 candidates at this size), R rois per frame of which <= round(FG_FRACTION * R) foreground, every kept fg roi
    # above FG_THRESH and every kept bg roi below it
    lab = drawn_a["labels"]
    assert lab.shape[0] == 4 and bool(((lab == 1).sum(1) <= 128).all()) and bool(((lab >= 0).sum(1) == cfg.TRAIN.RPN_BATCHSIZE).all())
    keep, nfg, mo = drawn_p["keep"], drawn_p["nfg"], drawn_p["max_ov"]
    n_fg = int(round(cfg.TRAIN.FG_FRACTION * R))
    assert tuple(keep.shape) == (4, R) and bool((nfg <= n_fg).all()) and bool((nfg >= 1).all())
    kept_ov = torch.gather(mo, 1, keep)
    slot = torch.arange(R, device=DEV).view(1, R)
    assert bool((kept_ov[slot < nfg] >= cfg.TRAIN.FG_THRESH).all()) and bool((kept_ov[slot >= nfg] < cfg.TRAIN.BG_THRESH_HI).all())
    step._restore(saved)
    atl.sample_record = ptl.sample_record = None
    atl.sample_replay, ptl.sample_replay = drawn_a, drawn_p
    step._device_sampling(False)                       # the host code path of both layers, its draws replaced by the recorded ones
    try:
        (step._body_branches if step.branches else step._body)()       # the same launches the graph replays, eagerly
        torch.cuda.synchronize()
        want = {k: float(v) for k, v in step.losses.items()}
    finally:
        atl.sample_replay = ptl.sample_replay = None
    assert len(want) == 10 and set(want) == set(got)
    if R != 32:
        record_margin(tag, "captured vs eager at equal samples: max rel. loss diff",
                      max(abs(got[k] - want[k]) / max(abs(want[k]), 1e-6) for k in want), 1e-3)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-3 * max(abs(want[k]), 1e-6), (k, got, want)
    assert abs(got["det"] - (got["rpn_cls"] + got["rpn_box"] + got["rcnn_cls"] + got["rcnn_box"])) <= 1e-5 * got["det"]
    # and the captured step keeps training
    for _ in range(2):
        step()
    assert _finite({k: float(v) for k, v in step.losses.items()})
    step.opt.unfuse()


def test_instance_styled_step_full_size_is_bit_reproducible_at_128_rois(fresh_cfg):
    """The captured two-branch step at full size and the yml's own 128 ROIs per frame (4 + 4 frames of 600x1000, ResNet-101,
    512 ROIs per branch), run twice from equal weights on the same minibatch: the same bits in every loss of every step and in
    every trained tensor, and no reduction that was asked to be ordered fell back to atomics.  The split counts of the filter
    gradients here (netD_pixel's at 25 088 rows, layer4's at 8192) are not the ones of the small-frame test in test_gpu_models."""
    cfg = fresh_cfg("res101")
    assert cfg.TRAIN.BATCH_SIZE == 128 and cfg.TRAIN.RPN_POST_NMS_TOP_N_TARGET == 128
    from i2vsgg_amd import train
    from i2vsgg_amd._lib import lib

    def run():
        torch.manual_seed(0)
        np.random.seed(cfg.RNG_SEED)
        net = train.build_instance_styled_net(101, device=DEV)
        step = train.InstanceStyleDStep(net, 4, seed=3, device=DEV)
        assert step.branches
        lib.i2v_ordered_fallbacks(1)
        assert step.capture(warmup=1, restore=True), step.graph_error
        losses = []
        for _ in range(3):
            step()
            losses.append(step._loss_buf.clone())
        torch.cuda.synchronize()
        assert lib.i2v_ordered_fallbacks(1) == 0, "a reduction that was asked to be ordered ran on atomics"
        w = {k: v.detach().clone() for k, v in net.named_parameters() if v.requires_grad}
        step.opt.unfuse()
        return torch.stack(losses), w

    la, wa = run()
    lb, wb = run()
    assert bool(torch.isfinite(la).all()), la
    assert torch.equal(la, lb), (la - lb).abs().max(dim=0).values.tolist()
    assert float(la[0, 0]) != float(la[2, 0])                # the weights do move
    diff = [k for k in wa if not torch.equal(wa[k], wb[k])]
    assert not diff, (diff[:8], len(diff))


def test_instance_styled_consistency_terms_at_128_rois_full_size(fresh_cfg):
    """--cr at full size and the yml's 128 ROIs per frame, the one size at which the reference's hard-coded ``repeat(1,128)``
    (trainval_net_instance_styleD_bilinear.py:300-311) and consistency_terms' actual ROI count agree: the step's
    source_adv_cst / target_adv_cst against the reference's literal expression evaluated in float64 on the step's own
    discriminator outputs (caught as the step's forward returns them).  Both bodies: the one-pass eager step
    (train.consistency_terms) and the two-branch body a captured step records (train._consistency_term), run on eager launches
    so that the outputs can be caught."""
    cfg = fresh_cfg("res101")
    assert cfg.TRAIN.BATCH_SIZE == 128 and cfg.TRAIN.RPN_POST_NMS_TOP_N_TARGET == 128
    from i2vsgg_amd import train
    torch.manual_seed(0)
    np.random.seed(cfg.RNG_SEED)
    net = train.build_instance_styled_net(101, device=DEV)
    step = train.InstanceStyleDStep(net, 4, seed=3, device=DEV, cr=True)
    assert step.branches
    seen = {}
    forward_features = net.forward_features

    def spy(*a, **k):
        out = forward_features(*a, **k)
        target = a[5] if len(a) > 5 else k["target"]
        d_inst, d_style = out if target else out[8:10]
        seen[bool(target)] = (d_inst.detach().clone(), d_style.detach().clone())
        return out
    net.forward_features = spy
    consistency_loss = torch.nn.MSELoss()
    try:
        for body, run in (("one pass", step), ("two branches", step._body_branches)):
            seen.clear()
            run()
            torch.cuda.synchronize()
            got = {k: float(v) for k, v in step.losses.items()}
            assert set(seen) == {False, True}, body
            for name, (out_d_instance, out_d_style) in (("source_adv_cst", seen[False]), ("target_adv_cst", seen[True])):
                assert tuple(out_d_instance.shape) == (4 * 128, 1, 7, 7) and tuple(out_d_style.shape) == (4, 1)
                out_d_instance_consist = torch.mean(out_d_instance.double(), dim=3)
                out_d_instance_consist = torch.mean(out_d_instance_consist, dim=2)
                consistency_prob = out_d_style.double().repeat(1, 128).view(-1, 1)
                want = float(consistency_loss(out_d_instance_consist, consistency_prob.detach()))
                err = abs(got[name] - want) / abs(want)
                record_margin("consistency_terms_at_128_rois_full_size", "%s, %s rel. error vs float64" % (body, name), err, 1e-5)
                assert err <= 1e-5, (body, name, got[name], want)
    finally:
        del net.forward_features
    step.opt.unfuse()


def test_instance_styled_target_half_full_size_vs_oracle(fresh_cfg):
    _target_half_full_size_vs_oracle(fresh_cfg, 32)


def test_instance_styled_target_half_full_size_vs_oracle_at_128_rois(fresh_cfg):
    """The same at the yml's own RPN_POST_NMS_TOP_N_TARGET = 128 (config.py:51): 12000 -> 128 proposals, 128 pooled ROIs."""
    _target_half_full_size_vs_oracle(fresh_cfg, 128)


def _target_half_full_size_vs_oracle(fresh_cfg, R):
    """configs[2], the TARGET half at full size against the CPU oracle (round-3 review: the oracle comparison of this config
    existed only at 320x480 / ResNet-50): one 600x1000 frame through ResNet-101 C4 -> netD_style -> RPN head -> proposal layer
    (12000 -> R, NMS 0.7) -> RoIAlignAvg -> netD_pixel, no backward (trainval_net_instance_styleD_bilinear.py:293-296 reads
    exactly these two outputs).  Same seeded weights; dloss_t and dloss_t_style within 1e-3 relative, the instance map
    element-wise, the proposals as a set (score near-ties between two conv implementations may swap neighbours)."""
    fresh_cfg("res101", ["TRAIN.BATCH_SIZE", str(R), "TRAIN.RPN_POST_NMS_TOP_N_TARGET", str(R)])
    tag = "target_half_full_size_vs_oracle" + ("" if R == 32 else "[R=%d]" % R)
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.faster_rcnn.resnet_instance_styleD_bilinear import resnet
    from oracle import cops, nets, rpn
    H, W, n_cls = 600, 1000, 16
    p = {}
    p.update(syn.backbone_params(1, 101, top=True))
    p.update(syn.rpn_params(10, std=0.02))
    p.update(syn.det_head_params(11, n_cls))
    p.update(syn.netd_params(12))
    net = resnet(tuple(range(n_cls)), 101)
    net.create_architecture()
    r = load_reference_state(net, p, strict=False)
    assert not r.unexpected_keys and all("num_batches" in k for k in r.missing_keys)
    net.to(DEV).train()
    im, info = syn.frames(21, 1, H, W)
    stash = {}
    rpn_forward = net.RCNN_rpn.forward

    def spy(*a, **k):
        out = rpn_forward(*a, **k)
        stash["rois"] = out[0].detach().cpu().numpy()
        return out
    net.RCNN_rpn.forward = spy
    with torch.no_grad():
        d_inst_t, d_sty_t = net(torch.from_numpy(im).to(DEV), torch.from_numpy(info).to(DEV), torch.zeros(1, 1, 5, device=DEV),
                                torch.zeros(1, device=DEV), target=True, eta=0.1, eta_style=0.001)
    rois = stash["rois"]
    assert rois.shape == (1, R, 5)
    po = {k: v.clone() for k, v in p.items()}
    with torch.no_grad():
        feat, feat1 = nets.extract_feature(torch.from_numpy(im), po, blocks=(3, 4, 23))
        assert tuple(feat.shape) == (1, 1024, 38, 63) and tuple(feat1.shape) == (1, 512, 75, 125)
        d_sty_o = nets.netd_style(feat1, po, 0.001)
        cls, prob, box = nets.rpn_head(feat, po)
    rois_o, _ = rpn.proposal_layer(prob[:, 9:].numpy(), box.numpy(), info, 12000, R, 0.7)
    a = {tuple(np.round(x, 1)) for x in rois[0] if x[1:].any()}
    o = {tuple(np.round(x, 1)) for x in rois_o[0] if x[1:].any()}
    record_margin(tag, "proposal set overlap (of %d)" % len(o), len(a & o) / len(o), TARGET_SET_OVERLAP)
    assert len(a & o) >= TARGET_SET_OVERLAP * len(o), (len(a & o), len(o))
    pooled = torch.from_numpy(cops.roi_align_avg_fwd(feat.numpy(), rois.reshape(-1, 5), 7, 7, 1.0 / 16.0))      # the HIP path's own rois
    with torch.no_grad():
        d_inst_o = nets.netd_pixel(pooled, po, 0.1)
    rel = lambda x, y: abs(float(x) - float(y)) / max(abs(float(y)), 1e-12)
    got_t, want_t = 0.5 * torch.mean((1 - d_inst_t) ** 2).item(), 0.5 * torch.mean((1 - d_inst_o) ** 2).item()
    got_s, want_s = 0.5 * torch.mean((1 - d_sty_t) ** 2).item(), 0.5 * torch.mean((1 - d_sty_o) ** 2).item()
    if R != 32:
        record_margin(tag, "dloss_t rel. error", rel(got_t, want_t), 1e-3)
        record_margin(tag, "dloss_t_style rel. error", rel(got_s, want_s), 1e-3)
        assert d_inst_t.shape[0] == R
    assert rel(got_t, want_t) < 1e-3 and rel(got_s, want_s) < 1e-3, (got_t, want_t, got_s, want_s)
    np.testing.assert_allclose(d_inst_t.cpu().numpy(), d_inst_o.numpy(), rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(d_sty_t.cpu().numpy(), d_sty_o.numpy(), rtol=1e-3, atol=1e-7)


def test_device_sampling_statistics(fresh_cfg):
    """The device-side samplers draw what the reference's host code draws (anchor_target_layer.py:123-143,
    proposal_target_layer_cascade.py:140-182): subsample sizes, class of every kept index, replacement rules."""
    cfg = fresh_cfg("res101", ["TRAIN.BATCH_SIZE", "32"])
    from i2vsgg_amd.model.rpn.anchor_target_layer import _AnchorTargetLayer
    from i2vsgg_amd.model.rpn.proposal_target_layer_cascade import _ProposalTargetLayer
    torch.manual_seed(1)
    B, N = 3, 5000
    lab = torch.full((B, N), -1.0, device=DEV)
    lab[0, :300] = 1; lab[0, 300:4000] = 0             # more fg than 128, more bg than the rest
    lab[1, :40] = 1; lab[1, 40:4000] = 0               # few fg: bg fills up to 256 - 40
    lab[2, :10] = 1; lab[2, 10:60] = 0                 # fewer candidates than the batch: everything kept
    perm = torch.stack([torch.randperm(N, device=DEV) for _ in range(B)])
    lab = torch.gather(lab, 1, perm)
    out = _AnchorTargetLayer._subsample_device(lab, 128, 256)
    fg, bg = (out == 1).sum(1).tolist(), (out == 0).sum(1).tolist()
    assert fg == [128, 40, 10] and bg == [128, 216, 50]
    assert bool(((out == 1) <= (lab == 1)).all()) and bool(((out == 0) <= (lab == 0)).all())      # kept only from its class
    out2 = _AnchorTargetLayer._subsample_device(lab, 128, 256)
    assert not torch.equal(out, out2)                                                               # random, not a prefix
    # proposals: image 0 both classes, image 1 only fg, image 2 only bg
    mo = torch.zeros(3, 400, device=DEV)
    mo[0, :50] = 0.8; mo[0, 50:] = 0.2
    mo[1, :] = 0.9
    mo[2, :] = 0.1
    keep, nfg = _ProposalTargetLayer._sample_device(mo, 32, 8)
    assert nfg.view(-1).tolist() == [8, 32, 0]
    k0 = keep[0].tolist()
    assert all(i < 50 for i in k0[:8]) and len(set(k0[:8])) == 8 and all(i >= 50 for i in k0[8:])
    assert all(0 <= i < 400 for i in keep[1].tolist() + keep[2].tolist())
    assert len(set(keep[2].tolist())) > 16                                                           # spread over the candidates
    # unbiased: over many draws every candidate of a class is kept equally often (round-2 review: a biased sampler would pass
    # the size checks above).  z = (count - T p) / sqrt(T p (1 - p)) per candidate: mean z^2 ~ 1, no candidate beyond 5 sigma
    T = 300
    cnt_fg = torch.zeros(N, device=DEV)
    cnt_bg = torch.zeros(N, device=DEV)
    for _ in range(T):
        o = _AnchorTargetLayer._subsample_device(lab[:1], 128, 256)[0]
        cnt_fg += (o == 1)
        cnt_bg += (o == 0)
    for cnt, cand, k in ((cnt_fg, lab[0] == 1, 128), (cnt_bg, lab[0] == 0, 128)):
        n = int(cand.sum())
        pr = k / n
        z = (cnt[cand] - T * pr) / (T * pr * (1 - pr)) ** 0.5
        assert float(cnt[~cand].sum()) == 0 and abs(float(cnt[cand].sum()) - T * k) < 0.5
        assert 0.75 < float((z * z).mean()) < 1.3 and float(z.abs().max()) < 5.0, (n, float((z * z).mean()), float(z.abs().max()))
    cnt = torch.zeros(400, device=DEV)
    for _ in range(T):
        kp, _n = _ProposalTargetLayer._sample_device(mo[:1], 32, 8)
        cnt += torch.bincount(kp[0].long(), minlength=400).float()
    for cand, k in ((slice(0, 50), 8), (slice(50, 400), 24)):
        n = cand.stop - cand.start
        pr = k / n
        z = (cnt[cand] - T * pr) / (T * pr * (1 - pr)) ** 0.5
        assert abs(float(cnt[cand].sum()) - T * k) < 0.5
        assert 0.7 < float((z * z).mean()) < 1.4 and float(z.abs().max()) < 5.0, (n, float((z * z).mean()), float(z.abs().max()))


def test_device_sampling_statistics_at_128_rois(fresh_cfg):
    """The device-side proposal sampler at the yml's own TRAIN.BATCH_SIZE = 128 (cfgs/res101.yml:12): keep buffers of (B, 128),
    round(FG_FRACTION * 128) = 32 foreground rows where both classes exist, all 128 from the one class an image has, every kept
    index of its class, and over many draws every candidate kept as often as the reference's rules make it: foreground without
    replacement (Binomial(T, 32 / n) per candidate), background with replacement (Binomial(96 T, 1 / n))."""
    cfg = fresh_cfg("res101")
    from i2vsgg_amd.model.rpn.proposal_target_layer_cascade import _ProposalTargetLayer
    R = cfg.TRAIN.BATCH_SIZE
    fg_per = int(round(cfg.TRAIN.FG_FRACTION * R))
    assert (R, fg_per) == (128, 32)
    torch.manual_seed(1)
    mo = torch.zeros(3, 400, device=DEV)
    mo[0, :200] = 0.8; mo[0, 200:] = 0.2               # both classes
    mo[1, :] = 0.9                                     # only fg
    mo[2, :] = 0.1                                     # only bg
    keep, nfg = _ProposalTargetLayer._sample_device(mo, R, fg_per)
    assert tuple(keep.shape) == (3, R) and nfg.view(-1).tolist() == [32, 128, 0]
    k0 = keep[0].tolist()
    assert all(i < 200 for i in k0[:32]) and len(set(k0[:32])) == 32 and all(i >= 200 for i in k0[32:])
    assert all(0 <= i < 400 for i in keep[1].tolist() + keep[2].tolist())
    assert len(set(keep[1].tolist())) > 64 and len(set(keep[2].tolist())) > 64                      # spread over the candidates
    T = 300
    cnt = torch.zeros(400, device=DEV)
    for _ in range(T):
        kp, _n = _ProposalTargetLayer._sample_device(mo[:1], R, fg_per)
        cnt += torch.bincount(kp[0].long(), minlength=400).float()
    for cand, k, draws, pr in ((slice(0, 200), 32, T, 32 / 200), (slice(200, 400), 96, 96 * T, 1 / 200)):
        z = (cnt[cand] - draws * pr) / (draws * pr * (1 - pr)) ** 0.5
        assert abs(float(cnt[cand].sum()) - T * k) < 0.5
        assert 0.7 < float((z * z).mean()) < 1.4 and float(z.abs().max()) < 5.0, (k, float((z * z).mean()), float(z.abs().max()))


def test_res50_yml_full_frame_plumbing(fresh_cfg):
    """configs[0]: cfgs/res50.yml (RPN_BATCHSIZE 128, BATCH_SIZE 128, DOUBLE_BIAS False) on ONE 1x3x600x1000 frame:
    detector forward in eval mode (TEST proposal settings: 6000 -> 300) and the SGG_emb relation head forward on the same
    frame's feature map; the head's scores equal the CPU oracle's on the same feature map within 1e-3."""
    cfg = fresh_cfg("res50")
    assert cfg.TRAIN.RPN_BATCHSIZE == 128 and cfg.TRAIN.BATCH_SIZE == 128 and cfg.TRAIN.DOUBLE_BIAS is False
    from i2vsgg_amd import train
    from oracle import nets
    det = train.build_instance_styled_net(50, device=DEV).eval()
    im, info = syn.frames(0, 1, 600, 1000)
    gt, nb = syn.gt_boxes(0, 1, 8, det.n_classes, cfg.MAX_NUM_GT_BOXES, 600, 1000)
    to = lambda x: torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        rois, cls_prob, bbox_pred, *_rest, d_inst, d_style = det(to(im), to(info), to(gt), to(nb))
    P = cfg.TEST.RPN_POST_NMS_TOP_N
    assert tuple(rois.shape) == (1, P, 5) and tuple(cls_prob.shape) == (1, P, det.n_classes)
    assert tuple(bbox_pred.shape) == (1, P, 4 * det.n_classes)
    assert bool(torch.isfinite(cls_prob).all()) and bool(torch.isfinite(bbox_pred).all())
    np.testing.assert_allclose(cls_prob.sum(2).cpu().numpy(), 1.0, rtol=1e-5)
    r = rois[0].cpu().numpy()
    assert (r[:, 1] >= 0).all() and (r[:, 3] <= 999).all() and (r[:, 2] >= 0).all() and (r[:, 4] <= 599).all()
    assert (r[:, 3] >= r[:, 1]).all() and (r[:, 4] >= r[:, 2]).all()
    # relation head on the same frame: 8 boxes, 8 pairs
    sgg = train.build_sgg_net(50, device=DEV).eval()
    step = train.SGGEmbStep(sgg, 1, seed=0, device=DEV, n_boxes=8, n_pairs=8, use_graph=False)
    with torch.no_grad():
        fmap = sgg.RCNN_base(step.im)
        score, feat = sgg.vrd.forward_device(fmap, step.boxes, step.relb, step.masks, step.ixs, step.ixo)
    assert tuple(fmap.shape) == (1, 1024, 38, 63) and tuple(score.shape) == (8, 62)
    np.testing.assert_allclose(score.sum(1).cpu().numpy(), 1.0, rtol=1e-5)           # eval: softmax over predicates
    p = {k: v.detach().cpu() for k, v in sgg.state_dict().items()}
    with torch.no_grad():
        ref, _ = nets.vrd_head(fmap.contiguous().cpu(), step.boxes.cpu().numpy(), step.relb.cpu().numpy(),
                               step.masks[:, :2].cpu().numpy(), step.ixs.cpu().numpy(), step.ixo.cpu().numpy(),
                               sgg.vrd.prd_vecs, p, training=False)
    np.testing.assert_allclose(score.cpu().numpy(), ref.numpy(), rtol=1e-3, atol=1e-6)
    step.opt.unfuse()


def test_instance_styled_staged_batch_equals_fresh_step(fresh_cfg):
    """stage() on a captured step: the losses of the replay on a newly staged minibatch equal those of a fresh step object
    built on that minibatch with the same parameters (device-side sampling draws differ: detection loss within 25 %,
    discriminator losses within 1e-3)."""
    fresh_cfg("res101", ["TRAIN.BATCH_SIZE", "16", "TRAIN.RPN_POST_NMS_TOP_N_TARGET", "16"])
    from i2vsgg_amd import train
    net = train.build_instance_styled_net(101, device=DEV)
    step = train.InstanceStyleDStep(net, 2, lr=0.0, seed=3, device=DEV, h=256, w=320)
    assert step.capture(warmup=1, restore=True), step.graph_error
    step()
    first = {k: float(v) for k, v in step.losses.items()}
    step.reseed(11)
    step()
    got = {k: float(v) for k, v in step.losses.items()}
    ref = train.InstanceStyleDStep(net, 2, lr=0.0, seed=11, device=DEV, h=256, w=320)
    ref()
    want = {k: float(v) for k, v in ref.losses.items()}
    assert abs(got["dloss_t_style"] - want["dloss_t_style"]) <= 1e-3 * abs(want["dloss_t_style"]), (got, want)
    assert abs(got["dloss_s_style"] - want["dloss_s_style"]) <= 1e-3 * abs(want["dloss_s_style"]), (got, want)
    assert abs(got["det"] - want["det"]) <= 0.25 * want["det"], (got, want)
    assert got != first


def test_instance_styled_filter_gradients_on_a_side_branch(fresh_cfg):
    """I2V_WGRAD_BRANCH (off by default: -1 % of the step for +2.4 GB): the bottleneck nodes' filter gradients on
    a second stream, one edge per block, joined before the update -- the same losses and the same parameter UPDATE as on one
    stream.  One step from identical weights (eager, host-side sampling from the same np.random stream): later steps sample
    other proposals as soon as a score moves in its last bit, which is not what this test is about."""
    cfg = fresh_cfg("res101", ["TRAIN.BATCH_SIZE", "16", "TRAIN.RPN_POST_NMS_TOP_N_TARGET", "16"])
    from i2vsgg_amd import train
    names = ["RCNN_base.4.0.conv1.weight", "RCNN_base.4.0.downsample.0.weight", "RCNN_base.5.0.conv2.weight",
             "RCNN_base.6.5.conv2.weight", "RCNN_base.6.22.conv3.weight", "RCNN_top.0.1.conv1.weight"]

    def run(branch):
        torch.manual_seed(0)
        np.random.seed(cfg.RNG_SEED)
        net = train.build_instance_styled_net(101, device=DEV)
        before = {k: v.detach().clone() for k, v in net.named_parameters() if k in names}
        step = train.InstanceStyleDStep(net, 2, seed=3, device=DEV, h=256, w=320)
        if branch:
            step.wgrad_branch, step._wgrad_stream = True, torch.cuda.Stream()
        step()
        torch.cuda.synchronize()
        losses = {k: float(v) for k, v in step.losses.items()}
        delta = {k: dict(net.named_parameters())[k].detach() - before[k] for k in names}
        return losses, delta

    a, da = run(False)
    b, db = run(True)
    for k in a:
        assert abs(a[k] - b[k]) <= 1e-5 * max(abs(a[k]), 1e-6), (k, a, b)
    for k in names:
        assert float(da[k].abs().max()) > 0
        # the update is ~1e-5 on weights of ~0.1: one ulp of a weight is 1e-3 of it
        assert float((da[k] - db[k]).abs().max()) <= 1e-2 * float(da[k].abs().max()) + 3e-8, k


def test_instance_styled_two_branches_equal_one_pass(fresh_cfg):
    """The captured step's default form -- source and target forward / backward as two branches of the graph, their
    gradients added after the join (``InstanceStyleDStep._body_branches``) -- against the one-pass form on one stream: one
    step from identical weights, eager with host-side sampling (same np.random stream): same losses, same parameter update;
    and the captured two-branch step keeps training."""
    cfg = fresh_cfg("res101", ["TRAIN.BATCH_SIZE", "16", "TRAIN.RPN_POST_NMS_TOP_N_TARGET", "16"])
    from i2vsgg_amd import train
    names = ["RCNN_base.4.0.conv1.weight", "RCNN_base.5.0.conv2.weight", "RCNN_base.6.22.conv3.weight",
             "RCNN_top.0.1.conv1.weight", "RCNN_rpn.RPN_Conv.weight", "netD_pixel.conv1.weight", "netD_style.fc_1.weight",
             "RCNN_cls_score.weight", "RCNN_bbox_pred.bias"]

    def run(branches):
        torch.manual_seed(0)
        np.random.seed(cfg.RNG_SEED)
        net = train.build_instance_styled_net(101, device=DEV)
        before = {k: v.detach().clone() for k, v in net.named_parameters() if k in names}
        step = train.InstanceStyleDStep(net, 2, seed=3, device=DEV, h=256, w=320, cr=True)
        assert step.branches
        (step._body_branches if branches else step._body)()
        torch.cuda.synchronize()
        losses = {k: float(v) for k, v in step.losses.items()}
        delta = {k: dict(net.named_parameters())[k].detach() - before[k] for k in names}
        return losses, delta, step

    a, da, _ = run(False)
    b, db, step = run(True)
    for k in a:
        assert abs(a[k] - b[k]) <= 1e-5 * max(abs(a[k]), 1e-6), (k, a, b)
    for k in names:
        assert float(da[k].abs().max()) > 0, k
        assert float((da[k] - db[k]).abs().max()) <= 1e-2 * float(da[k].abs().max()) + 3e-8, k
    assert step.capture(warmup=1), step.graph_error
    w0 = step.net.RCNN_base[6][22].conv3.weight.detach().clone()
    for _ in range(2):
        step()
    got = {k: float(v) for k, v in step.losses.items()}
    assert all(np.isfinite(v) for v in got.values()), got
    assert not torch.equal(w0, step.net.RCNN_base[6][22].conv3.weight.detach())


def test_joint_step_full_size_on_one_gpu(fresh_cfg):
    """configs[4] on ONE rank (its 8-GPU form shards these frames): bench.py's ``run_joint`` composition
    at full size -- one instance_styleD D+G step (4 source + 4 target frames of 600x1000, ResNet-101) followed by one SGG_emb
    step on 4 frames, both nets, both graphs, both optimizers resident in one process: finite losses, both nets train, the
    line carries a roofline block and the peak memory."""
    import argparse
    import bench
    fresh_cfg("res101", bench.SET_CFGS[6:])
    a = argparse.Namespace(layers=101, no_graph=False, warmup=1, steps=3, full=True, dump_outputs="")     # --full: the roofline block
    line, (dstep, sstep), (det, sgg) = bench.run_joint(a, 0, 1, torch.device(DEV))
    try:
        cfgd = line["config"]
        assert cfgd["hip_graph"] == [True, True], (dstep.graph_error, sstep.graph_error)
        assert all(np.isfinite(v) for v in cfgd["losses_det"].values()) and np.isfinite(cfgd["loss_sgg"]), cfgd
        assert 0.0 < cfgd["loss_sgg"] < 1.0 and cfgd["loss_det"] > 0.0
        assert line["value"] > 0 and line["unit"] == "frames/s" and line["n_gpus"] == 1
        r = line["roofline"]
        assert r["bound"] == "mfma" and 0.05 < r["frac"] < 1.0 and r["launches_per_step"] > 100, r
        assert 5.0 < cfgd["max_mem_GB"] < 120.0, cfgd["max_mem_GB"]
        # both nets train: one more joint step moves a trunk filter of the detector and the relation head
        w_det = det.RCNN_base[6][22].conv3.weight.detach().clone()
        w_sgg = sgg.vrd.fc7.fc.weight.detach().clone()
        frozen = sgg.RCNN_base[6][22].conv3.weight.detach().clone()
        dstep(); sstep()
        torch.cuda.synchronize()
        assert not torch.equal(w_det, det.RCNN_base[6][22].conv3.weight.detach())
        assert not torch.equal(w_sgg, sgg.vrd.fc7.fc.weight.detach())
        assert torch.equal(frozen, sgg.RCNN_base[6][22].conv3.weight.detach())      # the relation net's trunk is frozen (:148)
    finally:
        sstep.opt.unfuse()


def test_bench_plain_headline_run_and_its_outputs(fresh_cfg, tmp_path):
    """bench.py's plain run of the headline (configs[1]) as main() drives it: the timed steps and the line -- no roofline block --
    and --dump-outputs: the loss, the backbone's feature maps and a fixed sample of every trained head parameter, as the last
    timed step left them, in float32, within 64 MB."""
    import argparse
    import os
    import bench
    fresh_cfg("res101", bench.SET_CFGS[6:])
    bench._OUTPUTS.clear()
    a = argparse.Namespace(layers=101, no_graph=False, warmup=1, steps=3, full=False, dump_outputs=str(tmp_path))
    line, step, net = bench.run_sgg(a, 0, 1, torch.device(DEV))
    try:
        assert line["steps"] == 3 and line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 2.0) < 1e-6      # 2 frames per timed step
        assert "roofline" not in line and line["config"]["hip_graph"], line["config"]["graph_error"]
        bench.write_outputs(str(tmp_path))
        got = {f[:-len(".npy")]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
        assert set(got) == {"loss", "fmap"} | {n for n, _ in net.named_parameters() if n.startswith("vrd.")}
        assert all(v.dtype == np.float32 for v in got.values()) and sum(v.nbytes for v in got.values()) <= 64 << 20
        assert got["loss"].shape == (1,) and got["loss"][0] == float(step.loss) and np.isfinite(got["loss"][0])
        assert got["fmap"].shape == (2, 1024, 38, 63)
        np.testing.assert_array_equal(got["fmap"], step.fmap.cpu().numpy())
        np.testing.assert_array_equal(got["vrd.fc7.fc.bias"], net.vrd.fc7.fc.bias.detach().cpu().numpy())   # whole: below the cap
        assert 600000 < got["vrd.fc6.fc.weight"].size <= 1 << 20                                       # a sample of 205M elements
    finally:
        step.opt.unfuse()
        bench._OUTPUTS.clear()


def test_sgg_step_full_size_vs_oracle(fresh_cfg):
    """configs[1] AT FULL SIZE against the CPU oracle (round-4 review: full-size coverage was self-consistency plus the backbone
    golden; the oracle comparison of the step ran at 200x320 / res50 / 6 boxes): cfgs/res101.yml, 2 frames of 600x1000,
    32 boxes + 32 pairs per frame, dropout off.  The eager step's loss, relation logits, ``fc7.bias.grad`` and a strided slice
    of ``fc6.weight.grad`` within 1e-3 (north_star's tolerance) of ``oracle.nets`` on the same seeded batch
    (trainval_net_SGG_emb.py:230-255: forward, BCE-with-logits, backward); then the captured / overlapped step -- the form
    bench.py times -- gives the eager step's loss on the same batch and the same head weights after three steps."""
    import torch.nn.functional as F
    from i2vsgg_amd import ops, train
    from i2vsgg_amd.model.utils import config as c
    from oracle import nets
    from test_gpu_models import _weights_close
    c.cfg_from_file(c.default_cfg_file("res101"))
    REL = 1e-3

    def make(graph):
        net = train.build_sgg_net(layers=101, seed=5, device=DEV)
        net.vrd.dropout = False
        step = train.SGGEmbStep(net, 2, seed=3, device=DEV, h=600, w=1000, n_boxes=32, n_pairs=32, fuse_sgd=graph,
                                use_graph=graph)
        return net, step

    net, step = make(False)
    assert step.boxes.shape[0] == 64 and step.relb.shape[0] == 64
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    got_score = {}
    fwd = net.vrd.forward_device

    def spy(*a, **k):
        out = fwd(*a, **k)
        got_score["s"] = out[0].detach().cpu().numpy()
        return out
    net.vrd.forward_device = spy
    loss = float(step())
    net.vrd.forward_device = fwd
    g_b7 = net.vrd.fc7.fc.bias.grad.detach().cpu().numpy().copy()
    g_w6 = net.vrd.fc6.fc.weight.grad.detach().reshape(4096, -1)[::64, ::97].cpu().numpy().copy()
    g_rel = net.vrd.fc_rel.fc.weight.grad.detach().cpu().numpy().copy()

    # ---------------- oracle: same weights, same batch (CPU, ~10 s)
    for k in ("vrd.fc6.fc.weight", "vrd.fc7.fc.bias", "vrd.fc_rel.fc.weight"):
        p[k].requires_grad_(True)
    with torch.no_grad():
        fm, _ = nets.extract_feature(step.im[:, :3].contiguous().cpu(), p, blocks=(3, 4, 23))
    sc, _ = nets.vrd_head(fm, step.boxes.cpu().numpy(), step.relb.cpu().numpy(), step.masks[:, :2].cpu().numpy(),
                          step.ixs.cpu().numpy(), step.ixo.cpu().numpy(), net.vrd.prd_vecs, p, training=True)
    labels, wrow = step.labels.cpu(), step.wrow.cpu()
    ref = (F.binary_cross_entropy_with_logits(sc, labels, reduction="none").mean(1) * wrow).sum()
    # equal pair counts per frame: the weighted sum IS the reference's plain mean (resnet_SGG_emb.py:93)
    assert abs(ref.item() - F.binary_cross_entropy_with_logits(sc, labels).item()) < 1e-6
    ref.backward()
    assert abs(loss - ref.item()) <= REL * abs(ref.item()), (loss, ref.item())
    np.testing.assert_allclose(got_score["s"][:64], sc.detach().numpy(), rtol=0, atol=REL)          # cosine logits in [-1, 1]

    def rel(a, b):
        return np.abs(a - b).max() / np.abs(b).max()
    assert rel(g_b7, p["vrd.fc7.fc.bias"].grad.numpy()) < REL
    assert rel(g_w6, p["vrd.fc6.fc.weight"].grad.reshape(4096, -1)[::64, ::97].numpy()) < REL
    assert rel(g_rel, p["vrd.fc_rel.fc.weight"].grad.numpy()) < REL
    del p, fm, sc

    # ---------------- the captured / overlapped step on the same batch
    eager = [loss] + [float(step()) for _ in range(2)]
    w_eager = {n: p.detach().clone() for n, p in net.named_parameters() if n.startswith("vrd.")}      # all 26, on the device
    step.opt.unfuse()
    del step, net
    torch.cuda.empty_cache()
    net, step = make(True)
    assert step.capture(warmup=1, restore=True), step.graph_error      # the warm-up step is undone: same start as the eager run
    cap = [float(step()) for _ in range(3)]
    step.opt.flush_pending()
    torch.cuda.synchronize()
    for a, b in zip(eager, cap):
        assert abs(a - b) <= 1e-5 * abs(a), (eager, cap)
    assert len(w_eager) == 26
    for n, p in net.named_parameters():
        if n.startswith("vrd."):
            _weights_close(p, w_eager[n], "configs[1] captured vs eager, " + n)
    step.opt.unfuse()
