"""Every gradient of the relation head ``vrd`` and its SGD(momentum) update against a float64 reference of the same step
(tests/relation_head_ref.py), on a 26-row batch whose ReLU decisions were moved away from zero on the reference alone.

Measure and bound, for tensor k:  err_k = max|gpu - ref64| / max|ref64|  <=  min(16 e32_k, 1e-5), where e32_k is the same measure
of the float32 CPU reference against float64, computed here, and never taken below 2^-24 (a correctly rounded float32 result is
already that far off; a smaller measured value is luck).  The factor 16 is for float32 reduction orders the BLAS does not use
(32-deep stage sums, split-K partials summed in split order, ordered column sums).  The relative L2 error of every output row
(out-feature / output channel) and, for the convolutions, of every filter tap is held to 16 x the float32 CPU reference's own
value of that measure, so that a wrong row or tap cannot hide under a large neighbour; rows whose float64 gradient is exactly
zero must be exactly zero.  Every observed value goes to parity_margins.txt next to its bound.

The library is imported inside the tests, as in the other GPU modules."""
import argparse

import numpy as np
import pytest
import torch

import relation_head_ref as R
from conftest import record_margin
from i2vsgg_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32 = 2.0 ** -24
CAP = 1e-5
CAP_BOXES, CAP_PAIRS = 2 * 8, 2 * 12


@pytest.fixture(scope="module")
def cfg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from i2vsgg_amd.model.utils import config as c
    c.cfg_from_file(c.default_cfg_file("res101"))
    return c.cfg


def _build(tag):
    """Conditioned parameters, the float64 and float32 CPU results of the step's forward + backward, and the head on the
    device with those parameters loaded and dropout off.  The 1.8 GB float64 parameter copy lives only inside this call."""
    from i2vsgg_amd.model.faster_rcnn.layers import load_reference_state
    from i2vsgg_amd.model.faster_rcnn.resnet_SGG_emb import vrd
    ov, st = R.VARIANTS[tag]
    batch = R.make_batch(R.SEED)
    params, info = R.condition(R.make_params(ov, st), batch, use_obj_visual=ov, spatial_type=st)
    R.conditions_hold(info)                                   # before anything is launched
    r64 = dict(zip(("loss", "score", "feat", "g"), R.grads(params, batch, torch.float64, ov, st)))
    r32 = dict(zip(("loss", "score", "feat", "g"), R.grads(params, batch, torch.float32, ov, st)))
    args = argparse.Namespace(num_relations=R.N_REL, num_classes=16, emb_dim=300, use_obj_visual=ov, spatial_type=st, vrd_task="pre_det")
    head = vrd(args, syn.word_vectors(22, 16), batch["prd"])
    res = load_reference_state(head, {k[len("vrd."):]: v for k, v in params.items()}, strict=True)
    assert not res.unexpected_keys and not res.missing_keys
    head.to(DEV).train()
    head.dropout = False
    return dict(tag=tag, variant=(ov, st), batch=batch, params=params, info=info, r64=r64, r32=r32, head=head)


@pytest.fixture(scope="module")
def default(cfg):
    s = _build("default")
    yield s
    s.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=["nov_s2", "ov_s1", "ov_s0"])
def variant(cfg, request):
    s = _build(request.param)
    yield s
    s.clear()
    torch.cuda.empty_cache()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(a).to(device=DEV, dtype=dtype)


def _restore(s):
    """The conditioned parameters back into the head (a step test has moved them)."""
    from i2vsgg_amd import optim
    with torch.no_grad():
        for n, p in s["head"].named_parameters():
            p.copy_(s["params"]["vrd." + n])
            p.grad = None
    optim.FusedSGD.bump()


def _check(test, what, got, ref64, ref32, fails, cache, cap=CAP):
    """One tensor: every measure of ``got`` against float64 under 16 x the float32 CPU reference's own (module docstring).
    ``cache``: the float32 CPU reference's measures, computed once per head."""
    if what not in cache:
        cache[what] = R.errors(ref32, ref64)
    e_gpu, e_cpu = R.errors(got, ref64), cache[what]
    for name in ("peak", "row", "tap"):
        if name not in e_gpu:
            continue
        bound = 16 * max(e_cpu[name], U32)
        if name == "peak":
            bound = min(bound, cap)
        record_margin(test, "%s %s" % (what, name), e_gpu[name], bound)
        if not e_gpu[name] <= bound:
            fails.append("%s %s: %.3g > %.3g" % (what, name, e_gpu[name], bound))
    if e_gpu["zero_rows"]:
        fails.append("%s: %d rows / taps / elements are exactly zero in float64 and not on the device" % (what, e_gpu["zero_rows"]))


def _check_all(test, s, loss, score, feat, grads):
    r64, r32 = s["r64"], s["r32"]
    fails, cache = [], s.setdefault("e32", {})
    _check(test, "loss", loss.reshape(1), r64["loss"].reshape(1), r32["loss"].reshape(1), fails, cache)
    _check(test, "logits", score, r64["score"], r32["score"], fails, cache)
    _check(test, "relation feature", feat, r64["feat"], r32["feat"], fails, cache)
    assert set(grads) == set(r64["g"]), set(grads) ^ set(r64["g"])
    for k in sorted(grads):
        if r64["g"][k] is None:               # so_vis_embeddings without the object-visual branch: no gradient on either side
            assert grads[k] is None and not s["variant"][0] and "so_vis_embeddings" in k, k
            continue
        assert grads[k] is not None, k
        _check(test, k, grads[k], r64["g"][k], r32["g"][k], fails, cache)
    assert not fails, "\n".join(fails)


def _pool_ref(batch, rois):
    from oracle import cops
    return cops.roi_pool_fwd(batch["fmap"], np.asarray(rois, np.float32), 7, 7, 1.0 / 16.0)[0]


def _eager(s):
    """One eager forward + backward of the head on the ragged batch -> loss, logits, feature, {name: grad}, extras."""
    from i2vsgg_amd import ops
    head, b = s["head"], s["batch"]
    st = s["variant"][1]
    fm = _dev(b["fmap"]).contiguous(memory_format=torch.channels_last)
    spatial = _dev(b["relloc"] if st == 1 else b["masks"])
    kept = []
    hook = head.so_vis_embeddings.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.append(o))[0]) \
        if s["variant"][0] else None
    try:
        head.zero_grad(set_to_none=True)
        score, x = head.forward_device(fm, _dev(b["boxes"]), _dev(b["relb"]), spatial, _dev(b["ixs"], torch.long), _dev(b["ixo"], torch.long))
        loss = ops.bce_rows(score, _dev(b["labels"]), _dev(b["wrow"]))
        loss.backward()
    finally:
        if hook is not None:
            hook.remove()
    torch.cuda.synchronize()
    grads = {"vrd." + n: p.grad for n, p in head.named_parameters()}
    return loss.detach(), score.detach(), x.detach(), grads, (kept[0].grad if kept else None), fm


def test_all_gradients_eager(default):
    s = default
    _restore(s)
    b = s["batch"]
    loss, score, x, grads, g_obj, fm = _eager(s)
    assert len(grads) == 26
    rois = np.concatenate((b["boxes"], b["relb"]))
    with torch.no_grad():
        pooled = s["head"].roi_pool(fm, _dev(rois))
    assert np.array_equal(pooled.cpu().numpy(), _pool_ref(b, rois))                  # the pooled rows, bit for bit
    # box 10 is in no pair: its embedding row gets no gradient at all; every other box is in one
    assert g_obj.shape == (11, 300) and not bool(g_obj[10].any()) and bool((g_obj[:10] != 0).any(1).all())
    _check_all("test_all_gradients_eager", s, loss, score, x, grads)


def test_all_gradients_in_the_captured_steps_head_form(default):
    """What ``SGGEmbStep._head`` runs: an ordered launch context with an arena, the feature maps packed at the start of a larger
    buffer with their extent in device memory, boxes and pairs zero-padded to a capacity, ``rois=`` / ``ix12=`` in one buffer
    each.  Same float64 targets: padding changes nothing, and a pad pair's rows get a gradient of exactly zero."""
    from i2vsgg_amd import launch, ops
    s = default
    _restore(s)
    head, b = s["head"], s["batch"]
    nb, npair = b["boxes"].shape[0], b["relb"].shape[0]
    h, w = b["fmap"].shape[2:]
    cap_cells = 16 * 24
    buf = torch.full((2 * cap_cells * 1024,), 1e30, device=DEV)                     # nothing past the extent may be read
    buf[:2 * h * w * 1024] = _dev(np.ascontiguousarray(b["fmap"].transpose(0, 2, 3, 1))).reshape(-1)
    extent = torch.tensor([h, w], dtype=torch.int32, device=DEV)
    rois = np.zeros((CAP_BOXES + CAP_PAIRS, 5), np.float32)
    rois[:nb], rois[CAP_BOXES:CAP_BOXES + npair] = b["boxes"], b["relb"]
    ix12 = np.zeros((2 * CAP_PAIRS,), np.int64)
    ix12[:npair], ix12[CAP_PAIRS:CAP_PAIRS + npair] = b["ixs"], b["ixo"]
    masks = np.zeros((CAP_PAIRS, 4, 32, 32), np.float32)
    masks[:npair, :2] = b["masks"]
    labels = np.zeros((CAP_PAIRS, R.N_REL), np.float32)
    labels[:npair] = b["labels"]
    wrow = np.zeros((CAP_PAIRS,), np.float32)
    wrow[:npair] = b["wrow"]
    rois_d, ix12_d = _dev(rois), _dev(ix12, torch.long)
    kept = []
    hook = head.so_vis_embeddings.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.append(o))[0])
    ctx = launch.LaunchContext(torch.device(DEV), arena=True, ordered=True)
    try:
        with ctx:
            fmap = ops.PackedMaps(buf, 2, 1024, extent)
            head.zero_grad(set_to_none=True)
            score, x = head.forward_device(fmap, rois_d[:CAP_BOXES], rois_d[CAP_BOXES:], _dev(masks), ix12_d[:CAP_PAIRS],
                                           ix12_d[CAP_PAIRS:], rois=rois_d, ix12=ix12_d)
            score.retain_grad()
            x.retain_grad()
            loss = ops.bce_rows(score, _dev(labels), _dev(wrow))
            loss.backward()
            pooled = head.roi_pool(fmap, rois_d)
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert score.shape == (CAP_PAIRS, R.N_REL)
    want = _pool_ref(b, rois)
    assert np.array_equal(pooled.cpu().numpy(), want)            # pad rois pool cell (0, 0) of frame 0 like the plain kernel
    assert not bool(score.grad[npair:].any()) and not bool(x.grad[npair:].any())        # pad pairs: exactly zero
    assert bool(score.grad[:npair].any(1).all())
    g_obj = kept[0].grad
    assert g_obj.shape == (CAP_BOXES, 300) and not bool(g_obj[10:].any()) and not bool(g_obj[0].eq(0).all())
    grads = {"vrd." + n: p.grad for n, p in head.named_parameters()}
    _check_all("test_all_gradients_in_the_captured_steps_head_form", s, loss.detach(), score.detach()[:npair], x.detach()[:npair], grads)


def test_variant_heads_all_gradients_eager(variant):
    """``use_obj_visual=False``; ``spatial_type=1`` (``fc_lov = FC(8, 256)``: a K of 8, below any stage depth); no spatial branch.
    Each conditioned on its own, every parameter against float64."""
    s = variant
    ov, st = s["variant"]
    head = s["head"]
    assert hasattr(head, "fc_so") == ov and hasattr(head, "conv_lo") == (st == 2) and hasattr(head, "fc_lov") == (st in (1, 2))
    if st == 1:
        assert tuple(head.fc_lov.fc.weight.shape) == (256, 8)
    loss, score, x, grads, _, _ = _eager(s)
    assert len(grads) == 26 - (0 if ov else 2) - {2: 0, 1: 6, 0: 8}[st]       # fc_so; the three convs; fc_lov
    _check_all("test_variant_heads_all_gradients_eager[%s]" % s["tag"], s, loss, score, x, grads)


LR = 0.1


@pytest.fixture(scope="module")
def sgd_ref(default):
    """The float64 step and its bounds, once for both schedules, on the device in float64 (the comparison of 226M elements
    then costs nothing): per tensor m1_ref, p1_ref, the m1 bound and the element-wise p1 bound E_p."""
    from i2vsgg_amd.model.utils.config import cfg as C
    s = default
    params, mom = s["params"], C.TRAIN.MOMENTUM
    m0 = R.momentum_like(s["r64"]["g"])
    ref = R.step_ref(params, s["batch"], m0, LR)
    assert all(torch.equal(ref["g"][k], s["r64"]["g"][k]) for k in ref["g"])
    out = {"m0": m0, "t": {}}
    seen = set()
    for n in params:
        lr_k, wd_k = R.group_of(n, LR)
        p0 = params[n]
        if "bias" in n:
            assert (lr_k, wd_k) == (2 * LR, 0.0)              # twice the rate, no decay
        else:
            assert lr_k == LR and wd_k > 0
        seen.add("bias" in n)
        m_ref, p_ref = ref["m1"][n], ref["p1"][n]
        m_cpu32 = mom * m0[n] + (s["r32"]["g"][n] + wd_k * p0)                            # the same update in float32 on the CPU
        top = float(m_ref.abs().max())
        assert mom > 0 and float((mom * m0[n].double()).abs().max()) > 0.1 * top         # the momentum term is a real share of m1
        bound = min(16 * max(float((m_cpu32.double() - m_ref).abs().max()) / top, U32), CAP)
        e_p = lr_k * bound * top + 2 * U32 * (p0.double().abs() + lr_k * m_ref.abs())
        # a dead update cannot pass: the float64 p1 is more than 100 float32 ulps away from p somewhere in the tensor
        ulps = float(((p_ref - p0.double()).abs() / torch.from_numpy(np.spacing(np.abs(p0.numpy()))).double()).max())
        assert ulps > 100, (n, ulps)
        out["t"][n] = dict(m=m_ref.to(DEV), p=p_ref.to(DEV), e_p=e_p.to(DEV), top=top, bound=bound)
    assert seen == {True, False}
    yield out
    out.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_one_sgd_step_with_loaded_momentum(default, sgd_ref, fused):
    """One step of SGD(momentum) at lr = 0.1 (lr m1 is then hundreds of float32 ulps of a weight, not a fraction of one) from
    momentum buffers loaded through ``load_state_dict``, once with fc6 / fc7 updated inside their filter-gradient kernel
    (``fuse_wgrad``: their ``.grad`` stays None) and once with every update separate.
      m1 against float64: the gradient bound, relative to max|m1_ref|  (e32: the float32 CPU update against float64);
      |p1 - p1_ref| <= lr_k bound_k max|m1_ref| + 2 u (|p| + lr_k |m1_ref|), u = 2^-24: lr times the error of m1, plus the
      roundings of lr m1 and of the difference (the form test_fc_update_against_float64 derives).
    Weight decay acts on the weights, the biases take twice the rate and no decay, and the loaded momentum enters m1: the
    float64 update is built from those rules written out in tests/relation_head_ref.py (``sgd_ref`` asserts that each is in
    force and that p1 has moved)."""
    from i2vsgg_amd import ops, optim
    s = default
    head, b = s["head"], s["batch"]
    test = "test_one_sgd_step_with_loaded_momentum[%s]" % ("fused" if fused else "separate")
    _restore(s)
    named = [("vrd." + n, p) for n, p in head.named_parameters()]
    opt = optim.make_optimizer("sgd", named, LR)
    fails = []
    try:
        sd = opt.state_dict()
        assert [g["name"] for g in sd["param_groups"]] == [n for n, _ in named]
        for i, (n, _) in enumerate(named):
            sd["state"][i]["momentum_buffer"] = sgd_ref["m0"][n]
        opt.load_state_dict(sd)
        names = opt.fuse_wgrad() if fused else []
        assert names == (["vrd.fc6.fc.weight", "vrd.fc7.fc.weight"] if fused else [])
        fm = _dev(b["fmap"]).contiguous(memory_format=torch.channels_last)
        opt.zero_grad()
        score, _ = head.forward_device(fm, _dev(b["boxes"]), _dev(b["relb"]), _dev(b["masks"]), _dev(b["ixs"], torch.long),
                                       _dev(b["ixo"], torch.long))
        loss = ops.bce_rows(score, _dev(b["labels"]), _dev(b["wrow"]))
        loss.backward()
        for n, p in named:
            assert (p.grad is None) == (n in names), n
        opt.step()
        torch.cuda.synchronize()
        got_m = {it["name"]: it["m"] for it in opt.items}
        for n, p in named:
            t = sgd_ref["t"][n]
            e_gpu = float((got_m[n].double() - t["m"]).abs().max()) / t["top"]
            record_margin(test, n + " m1", e_gpu, t["bound"])
            if not e_gpu <= t["bound"]:
                fails.append("%s m1: %.3g > %.3g" % (n, e_gpu, t["bound"]))
            r_p = float(((p.detach().double() - t["p"]).abs() / t["e_p"]).max())
            record_margin(test, n + " |p1 - float64| / E_p", r_p, 1.0)
            if not r_p <= 1.0:
                fails.append("%s p1: %.3g of its bound" % (n, r_p))
    finally:
        opt.unfuse()
        _restore(s)
    assert not fails, "\n".join(fails)
