"""The float64 reference of the relation-head step (tests/relation_head_ref.py) checked on its own, on the CPU: its gradients
against central differences, its conditioning against the two conditions the GPU tests rely on, ``oracle.nets.vrd_head``'s
default against the golden it had before it learnt ``dtype`` / ``taps``, and its update against ``torch.optim.SGD``."""
import numpy as np
import pytest
import torch

import relation_head_ref as R
from i2vsgg_amd import synthetic as syn
from oracle import nets


@pytest.fixture(scope="module")
def ref():
    """The conditioned default head in float64, built once for the module and freed after it."""
    batch = R.make_batch(R.SEED)
    raw = R.make_params()
    p64 = R.as_dtype(raw, torch.float64)
    params, info = R.condition(raw, batch, p64=p64)
    state = dict(batch=batch, raw=raw, params=params, p64=p64, info=info)
    yield state
    state.clear()


def test_conditioning_meets_its_conditions_and_moves_only_biases(ref):
    info, raw, params = ref["info"], ref["raw"], ref["params"]
    print("tau %.3g, %d biases moved, rounds %s" % (info["tau"], info["moved"], info["rounds"]))
    R.conditions_hold(info)
    assert 64 * 1e-8 < info["tau"] < 64 * 1e-5          # 64 x a float32 rounding error of a few thousand terms, nothing else
    n_diff = 0
    for k in raw:
        if "bias" in k:
            n_diff += int((raw[k] != params[k]).sum())
            assert params[k].dtype == torch.float32
        else:
            assert params[k] is raw[k]                  # not a weight is touched
    assert n_diff == info["moved"] > 0
    # the float64 copy the reference runs on holds exactly the float32 values the device will load
    assert all(torch.equal(ref["p64"][k], params[k].double()) for k in params)
    again, info2 = R.condition(params, ref["batch"], info["tau"], p64=ref["p64"])
    assert info2["moved"] == 0 and not any(info2["rounds"].values())
    assert all(again[k] is params[k] for k in params)


def test_batch_holds_the_planted_rows():
    b = R.make_batch(R.SEED)
    assert b["boxes"].shape == (11, 5) and b["relb"].shape == (15, 5) and b["fmap"].shape == (2, 1024, 12, 20)
    assert list(b["boxes"][:, 0]) == [0] * 5 + [1] * 6 and list(b["relb"][:, 0]) == [0] * 7 + [1] * 8
    w, h = b["boxes"][1, 3] - b["boxes"][1, 1], b["boxes"][1, 4] - b["boxes"][1, 2]
    assert w < 16 and h < 16 and b["boxes"][2, 3] == R.IM_W - 1 and b["boxes"][2, 4] == R.IM_H - 1
    used = set(b["ixs"]) | set(b["ixo"])
    assert 10 not in used and used == set(range(10))
    assert (b["ixs"] == 0).sum() == 2 and (b["ixo"] == 0).sum() == 2
    assert (b["ixs"][:7] < 5).all() and (b["ixo"][:7] < 5).all() and (b["ixs"][7:] >= 5).all() and (b["ixo"][7:] >= 5).all()
    assert b["labels"][2].sum() == 0 and b["labels"][9].sum() == 3
    assert b["masks"][5, 0].sum() == 0 and b["masks"][5, 1].sum() > 0 and set(np.unique(b["masks"])) == {0.0, 1.0}
    np.testing.assert_allclose(b["wrow"], [1 / 14.0] * 7 + [1 / 16.0] * 8, rtol=1e-7)
    assert abs(b["wrow"].sum() - 1.0) < 1e-6


def test_float64_gradients_against_central_differences(ref, monkeypatch):
    """Three entries of each of the 26 tensors: (L(t + h) - L(t - h)) / 2h of the float64 loss against float64 autograd.

    fc6's forward is linear in its weight and bias, so its pre-activation is computed once; a perturbed entry (i, j) adds
    h x[:, j] to column i of the cached product (no second 205M-element product; every evaluation takes this route).

    The bound.  A parameter enters one layer linearly, and as long as no pre-activation changes sign (asserted for both
    evaluations) everything behind it is linear too: a relation-feature row (or a predicate embedding) moves on a line,
    v(t) = v0 + t a.  Its cosine logit is then an analytic function of t whose k-th derivative is at most k! (|a| / |v0|)^k
    in size, and with softplus' derivatives (<= 1, 1/4, 1/8) the chain rule gives |L'''| <= 8 r^3, r = max |a| / |v0|, the
    weights of the loss summing to 1.  r is measured from the two evaluations: rho = r h = max |v(+h) - v(-h)| / (2 |v0|).
      truncation of a central difference:   h^2 / 6 |L'''|  <=  (4 / 3) rho^3 / h  <  2 rho^3 / h
      rounding:  both losses carry a float64 evaluation error; the longest reduction behind the cached product is fc7's
                 4096 terms, n u at worst with u = 2^-53, on a loss below 1:  2 * 4096 u / (2 h) = 4096 u / h
    h starts at 1e-3 of the tensor's largest entry and is halved while an evaluation flips a ReLU."""
    batch, p64 = ref["batch"], ref["p64"]
    loss, _, _, g = R.grads(ref["params"], batch, torch.float64)
    taps0 = {}
    with torch.no_grad():
        _, feat0 = R.forward(p64, batch, torch.float64, taps0)
        sem0 = _sem(p64, batch)
    z6_nobias = taps0["fc6"] - p64["vrd.fc6.fc.bias"]
    signs0 = {k: z > 0 for k, z in taps0.items()}
    fc_plain = nets._fc
    delta = {"row": 0, "ij": None, "h": 0.0}

    def fc_cached(x, p, k, relu=True, taps=None):
        if k != "vrd.fc6":
            return fc_plain(x, p, k, relu, taps)
        n = x.shape[0]
        y = z6_nobias[delta["row"]:delta["row"] + n] + p["vrd.fc6.fc.bias"]
        delta["row"] = (delta["row"] + n) % z6_nobias.shape[0]
        if delta["ij"] is not None:
            i, j = delta["ij"]
            y = y.clone()
            y[:, i] += delta["h"] * x[:, j]
        nets._tap(taps, k, y)
        return torch.relu(y)

    monkeypatch.setattr(nets, "_fc", fc_cached)
    with torch.no_grad():                                    # the cached route is the plain route
        s_plain, _ = R.forward(p64, batch, torch.float64)
        assert abs(float(R.loss_of(s_plain, batch)) - float(loss)) <= 1e-14

    def evaluate(key, idx, h):
        """loss, rho contribution and ReLU signs with entry ``idx`` of tensor ``key`` moved by ``h``."""
        t = p64[key]
        old = float(t[idx])
        taps = {}
        try:
            if key == "vrd.fc6.fc.weight":
                delta["ij"], delta["h"] = idx, h
            else:
                t[idx] = old + h
            with torch.no_grad():
                score, feat = R.forward(p64, batch, torch.float64, taps)
                sem = _sem(p64, batch)
        finally:
            t[idx] = old
            delta["ij"] = None
        same = all(torch.equal(taps[k] > 0, signs0[k]) for k in signs0)
        return float(R.loss_of(score, batch)), feat, sem, same

    u = 2.0 ** -53
    rng = np.random.default_rng(11)
    worst = 0.0
    for key in sorted(g):
        gk = g[key]
        live = torch.nonzero(gk.abs() >= 0.01 * gk.abs().max())          # entries that carry gradient: 0 == 0 checks nothing
        for n in rng.choice(len(live), 3, replace=False):
            idx = tuple(int(v) for v in live[n])
            h = 1e-3 * float(p64[key].abs().max())
            for _ in range(24):
                lp, fp, sp, ok_p = evaluate(key, idx, h)
                lm, fm, sm, ok_m = evaluate(key, idx, -h)
                if ok_p and ok_m:
                    break
                h /= 2
            assert ok_p and ok_m, (key, idx, h)
            rho = max(float((torch.linalg.vector_norm(fp - fm, dim=1) / (2 * torch.linalg.vector_norm(feat0, dim=1))).max()),
                      float((torch.linalg.vector_norm(sp - sm, dim=1) / (2 * torch.linalg.vector_norm(sem0, dim=1))).max()))
            bound = 2 * rho ** 3 / h + 4096 * u / h
            fd, an = (lp - lm) / (2 * h), float(gk[idx])
            worst = max(worst, bound / abs(an))
            assert abs(fd - an) <= bound, (key, idx, h, fd, an, bound, rho)
    print("largest bound / |gradient entry| of the 78 entries: %.3g" % worst)
    assert worst < 0.05          # the check has teeth: a bound never wider than 5 % of the entry it holds


def _sem(p, batch):
    """The predicate embeddings before their normalisation (the second moving vector of the logits)."""
    import torch.nn.functional as F
    sem = torch.as_tensor(batch["prd"], dtype=torch.float64)
    sem = F.leaky_relu(F.linear(sem, p["vrd.prd_sem_embeddings.0.weight"], p["vrd.prd_sem_embeddings.0.bias"]), 0.1)
    return F.linear(sem, p["vrd.prd_sem_embeddings.2.weight"], p["vrd.prd_sem_embeddings.2.bias"])


def test_vrd_head_default_is_bit_identical_to_its_golden(gold):
    """Without ``dtype`` the function returns float32 tensors with the bits it returned before: its logits on the
    ``vrd_head`` golden inputs equal the float32 forward written out here with plain torch calls, bit for bit, with and
    without ``taps``; and the golden's own numbers still hold to the tolerance test_oracle_golden.py asserts."""
    import torch.nn.functional as F
    from oracle import cops
    g = gold("vrd_head")
    p = syn.vrd_params(13)
    prd = syn.word_vectors(21, 62)
    anno = syn.relation_annotation(31, 8, 8, 62, 16)
    boxes, rel_boxes, spatial, labels, ixs, ixo = nets.build_pairs(anno["boxes"], anno["rels"], 1.0, 600.0, 1000.0, 62)
    fmap = np.abs(np.random.default_rng(32).standard_normal((1, 1024, 38, 63), dtype=np.float32))
    taps = {}
    with torch.no_grad():
        score, feat = nets.vrd_head(fmap, boxes, rel_boxes, spatial, ixs, ixo, prd, p, training=True)
        score_t, feat_t = nets.vrd_head(fmap, boxes, rel_boxes, spatial, ixs, ixo, prd, p, training=True, taps=taps)
        # the forward as it stood, statement by statement
        pool = lambda r: torch.from_numpy(cops.roi_pool_fwd(fmap, np.asarray(r, np.float32), 7, 7, 1.0 / 16.0)[0]).reshape(len(r), -1)
        fc = lambda x, k: F.linear(x, p["vrd.%s.fc.weight" % k], p["vrd.%s.fc.bias" % k])
        cv = lambda x, i, s, pad: F.relu(F.conv2d(x, p["vrd.conv_lo.%d.conv.weight" % i], p["vrd.conv_lo.%d.conv.bias" % i], stride=s, padding=pad))
        obj = fc(F.relu(fc(F.relu(fc(pool(boxes), "fc6")), "fc7")), "so_vis_embeddings")
        x = F.relu(fc(F.relu(fc(F.relu(fc(pool(rel_boxes), "fc6")), "fc7")), "fc8"))
        so = torch.cat((obj.index_select(0, torch.as_tensor(ixs)), obj.index_select(0, torch.as_tensor(ixo))), 1)
        lo = cv(cv(cv(torch.as_tensor(spatial, dtype=torch.float32), 0, 2, 2), 1, 2, 2), 2, 1, 0)
        x = torch.cat((x, F.relu(fc(so, "fc_so")), F.relu(fc(lo.reshape(lo.size(0), -1), "fc_lov"))), 1)
        x = fc(F.relu(fc(x, "fc_fusion")), "fc_rel")
        sem = F.linear(torch.as_tensor(prd, dtype=torch.float32), p["vrd.prd_sem_embeddings.0.weight"], p["vrd.prd_sem_embeddings.0.bias"])
        sem = F.linear(F.leaky_relu(sem, 0.1), p["vrd.prd_sem_embeddings.2.weight"], p["vrd.prd_sem_embeddings.2.bias"])
        want = F.normalize(x, p=2, dim=1) @ F.normalize(sem, p=2, dim=1).t()
    assert score.dtype == torch.float32 and feat.dtype == torch.float32
    assert torch.equal(score, want) and torch.equal(feat, x)
    assert torch.equal(score, score_t) and torch.equal(feat, feat_t)
    assert set(taps) == set(R.RELU_LAYERS) and taps["fc6"].shape == (len(boxes) + len(rel_boxes), 4096)
    np.testing.assert_allclose(score.numpy(), g["scores"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(feat.numpy(), g["rel_feat"], rtol=1e-4, atol=1e-6)


def test_step_ref_update_equals_torch_sgd_in_float64(ref):
    """``step_ref``'s m1 and p1 against torch.optim.SGD on float64 parameters carrying ``step_ref``'s own gradients, with the
    reference's two param groups (trainval_net_SGG_emb.py:133-141 through cfg.TRAIN) and a loaded, non-zero momentum buffer.
    The two write the same expression; one may fuse a product into its sum where the other rounds it: 4 u (u = 2^-53) of the
    operands' magnitudes, per element."""
    from i2vsgg_amd.model.utils.config import cfg
    T = cfg.TRAIN
    batch, params = ref["batch"], ref["params"]
    lr = 0.1
    g = R.grads(params, batch, torch.float64)[3]
    m0 = R.momentum_like(g)
    out = R.step_ref(params, batch, m0, lr)
    assert all(torch.equal(out["g"][k], g[k]) for k in g)                 # the reference is deterministic
    names = list(params)
    ps = [params[k].double().clone().requires_grad_() for k in names]
    groups = [{"params": [q], "lr": lr * (T.DOUBLE_BIAS + 1) if "bias" in k else lr,
               "weight_decay": (T.WEIGHT_DECAY if T.BIAS_DECAY else 0.0) if "bias" in k else T.WEIGHT_DECAY} for k, q in zip(names, ps)]
    opt = torch.optim.SGD(groups, lr=lr, momentum=T.MOMENTUM)
    sd = opt.state_dict()
    sd["state"] = {i: {"momentum_buffer": m0[k].double().clone()} for i, k in enumerate(names)}
    opt.load_state_dict(sd)
    for k, q in zip(names, ps):
        q.grad = g[k].clone()
    opt.step()
    assert T.MOMENTUM > 0 and T.WEIGHT_DECAY > 0
    if T.DOUBLE_BIAS:
        assert R.group_of("vrd.fc7.fc.bias", lr)[0] == 2 * lr
    if not T.BIAS_DECAY:
        assert R.group_of("vrd.fc7.fc.bias", lr)[1] == 0.0
    assert R.group_of("vrd.fc7.fc.weight", lr) == (lr, T.WEIGHT_DECAY)
    u = 2.0 ** -53
    for k, q in zip(names, ps):
        lr_k, wd_k = R.group_of(k, lr)
        p0, m_t = params[k].double(), opt.state[q]["momentum_buffer"]
        size_m = (T.MOMENTUM * m0[k].double()).abs() + g[k].abs() + (wd_k * p0).abs()
        size_p = p0.abs() + lr_k * m_t.abs()
        for got, want, size in ((out["m1"][k], m_t, size_m), (out["p1"][k], q.detach(), size_p)):
            assert got.dtype == torch.float64
            assert bool(((got - want).abs() <= 4 * u * size).all()), k
        assert not torch.equal(out["p1"][k], p0)
