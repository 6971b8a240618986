"""The ranking kernels (i2v_sort_desc of csrc/sort.hip and what is built on it: i2v_rpn_proposal of csrc/rpn.hip,
i2v_det_postprocess[_info] and i2v_relation_topk of csrc/det_post.hip) on ties, saturated scores, signed zeros, non-finite keys and at the edges of the 4096-key sort tile.
Every comparison is exact: integer orders, bit-equal boxes and scores against the CPU oracles.  Keys are NaN-free (the NaN
order of i2v_sort_desc is unspecified).  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from i2vsgg_amd import ops as o
    return o


@pytest.fixture(scope="module")
def oracle():
    from oracle import cops, rpn
    return cops, rpn


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ----------------------------------------------------------------------------- 1. sort_desc
SORT_SIZES = [1, 2, 4095, 4096, 4097, 8192, 8193, 65536, 65537, 130944, 131073]
SORT_FAMILIES = ["all_equal", "two_valued", "quantised", "runs_of_one", "specials", "signed_zeros"]
_FLT_MAX, _FLT_MIN = np.finfo(F32).max, np.finfo(F32).tiny


def _sort_keys(family, rng, n):
    """One segment of n NaN-free fp32 keys; every call draws new data, so the segments of one case differ."""
    if family == "all_equal":
        return np.full(n, np.round(rng.standard_normal() * 64) / 64, F32)
    if family == "two_valued":
        return rng.choice(np.array([0.25, 1.0], F32), n)
    if family == "quantised":          # thousands of ties; np.round leaves -0.0 for (-1/16, 0), so both zeros occur too
        return (np.round(rng.standard_normal(n) * 8) / 8).astype(F32)
    if family == "runs_of_one":         # runs of exactly 1.0 (a saturated softmax) over a tie-free tail below 1
        keys = ((rng.permutation(n).astype(F32) + F32(1.0)) / F32(n + 2)).astype(F32)
        run = max(1, n // 16)
        keys[np.repeat(rng.random(-(-n // run)) < 0.4, run)[:n]] = 1.0
        return keys
    if family == "specials":
        sp = np.array([np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -3e-39, _FLT_MAX, -_FLT_MAX, _FLT_MIN, -_FLT_MIN], F32)
        assert np.all(np.abs(sp[2:6]) < _FLT_MIN) and np.all(sp[2:6] != 0)       # the denormals are denormal
        keys = rng.standard_normal(n).astype(F32)
        pick = rng.random(n) < 0.5
        keys[pick] = rng.choice(sp, int(pick.sum()))
        return keys
    if family == "signed_zeros":
        keys = (rng.standard_normal(n) * 1e-3).astype(F32)
        pick = rng.random(n) < 0.6
        keys[pick] = rng.choice(np.array([0.0, -0.0], F32), int(pick.sum()))
        return keys
    raise ValueError(family)


def _stable_desc(keys):
    """Descending, ties (+0.0 and -0.0 among them) by ascending index: the two statements of the rule agree."""
    n = keys.size
    ref = np.lexsort((np.arange(n), -keys.astype(np.float64)))
    assert np.array_equal(ref, np.argsort(-keys, kind="stable"))
    return ref


def _sort_case(family, n_seg, n):
    rng = np.random.default_rng([SORT_FAMILIES.index(family), n_seg, n])
    keys = np.stack([_sort_keys(family, rng, n) for _ in range(n_seg)])
    assert not np.isnan(keys).any()
    if n_seg > 1 and n > 2 and family != "all_equal":
        assert all(not np.array_equal(keys[0], keys[s]) for s in range(1, n_seg))
    return keys, np.stack([_stable_desc(k) for k in keys])


def _check_sort(ops, family, n_seg, n):
    keys, ref = _sort_case(family, n_seg, n)
    if family == "all_equal":
        assert np.array_equal(ref, np.tile(np.arange(n), (n_seg, 1)))
    if family == "signed_zeros" and n >= 300:
        assert (_bits(keys) == 0x80000000).any() and (_bits(keys) == 0).any()
    order = ops.sort_desc(_dev(keys)).cpu().numpy()
    assert order.shape == (n_seg, n) and order.dtype == np.int32
    for s in range(n_seg):
        bad = np.nonzero(order[s] != ref[s])[0]
        assert bad.size == 0, "segment %d: %d ranks differ, first at rank %d (got index %d, want %d)" % (
            s, bad.size, bad[0], order[s, bad[0]], ref[s, bad[0]])


@pytest.mark.parametrize("n", SORT_SIZES)
@pytest.mark.parametrize("family", SORT_FAMILIES)
def test_sort_desc_is_the_stable_descending_order(ops, family, n):
    """n up to and past the 4096-key tile, powers of two (no padding keys) and 2^16 / 2^17 (the relation grid's sizes),
    one and three segments of different data."""
    for n_seg in (1, 3):
        _check_sort(ops, family, n_seg, n)


@pytest.mark.parametrize("family", SORT_FAMILIES)
def test_sort_desc_many_short_segments(ops, family):
    """The detection shape: 35 segments of 300 keys, each padded to one 4096-key tile of its own."""
    _check_sort(ops, family, 35, 300)


# ----------------------------------------------------------------------------- 2. proposal layer
PROPOSAL_SHAPES = {          # H, W, pre, post, im_info (one row per frame, so the clip differs per frame)
    "5x91": (5, 91, 1000, 300, [[80, 1456, 1], [64, 1200, 1]]),              # 4095 anchors: one key below the tile
    "8x57": (8, 57, 1000, 300, [[128, 912, 1], [100, 800, 1]]),              # 4104 anchors: just past the tile
    "38x63": (38, 63, 6000, 300, [[600, 1000, 1], [540, 960, 1]]),
}


def _proposal_inputs(shape, scores):
    H, W, pre, post, info = PROPOSAL_SHAPES[shape]
    B = 2
    rng = np.random.default_rng([sorted(PROPOSAL_SHAPES).index(shape), int(scores == "saturated")])
    n = B * 9 * H * W
    fg = ((rng.permutation(n).astype(F32) + F32(1.0)) / F32(n + 2)).reshape(B, 9, H, W)
    deltas = (rng.standard_normal((B, 36, H, W)) * 0.25).astype(F32)
    if scores == "quantised":
        fg = (np.round(fg * 16) / 16).astype(F32)
    else:                                           # the upper 30 % of every frame saturate to exactly 1.0
        for b in range(B):
            fg[b][fg[b] >= np.quantile(fg[b], 0.7)] = 1.0
    for b in range(B):                              # the cut at `pre` falls inside a run of ties, in every frame
        sc = -np.sort(-np.ascontiguousarray(fg[b].transpose(1, 2, 0)).reshape(-1), kind="stable")
        assert sc[pre - 1] == sc[pre], (shape, scores, b)
    return fg, deltas, np.array(info, F32), pre, post


@pytest.mark.parametrize("scores", ["quantised", "saturated"])
@pytest.mark.parametrize("shape", sorted(PROPOSAL_SHAPES))
def test_rpn_proposal_with_tied_scores_at_the_pre_nms_cut(ops, oracle, shape, scores):
    """Which of the tied anchors survive the pre_nms_top_n cut is decided by "descending score, then ascending anchor
    index": same rois (bit-equal), same kept anchors, same count as the oracle."""
    _, rpn = oracle
    fg, deltas, info, pre, post = _proposal_inputs(shape, scores)
    ref_rois, ref_kept = rpn.proposal_layer(fg, deltas, info, pre, post, 0.7)
    prob = np.concatenate([1.0 - fg, fg], 1).astype(F32)
    base = _dev(rpn.base_anchors().astype(F32))
    rois, kept, num = ops.rpn_proposal(_dev(prob), _dev(deltas), _dev(info), base, 16, pre, post, 0.7, is_prob=True,
                                       want_index=True)
    rois, kept, num = rois.cpu().numpy(), kept.cpu().numpy(), num.cpu().numpy()
    for b in range(2):
        assert num[b] == ref_kept[b].size, (b, num[b], ref_kept[b].size)
        assert np.array_equal(kept[b, :num[b]], ref_kept[b]), b
    assert np.array_equal(rois, ref_rois)


# ----------------------------------------------------------------------------- 3. detection post-processing
DET_R, DET_C = 300, 8
DET_STDS, DET_MEANS = (0.1, 0.1, 0.2, 0.2), (0.0, 0.0, 0.0, 0.0)


def _quantised_prob(rng, q):
    """Rows of multiples of 1/q that sum to 1 by construction (q draws over the classes): exact in fp32, many ties."""
    return (rng.multinomial(q, rng.dirichlet(np.ones(DET_C), size=DET_R)) / float(q)).astype(F32)


def _det_case(case):
    """-> rois, prob, pred, (im_h, im_w, scale), thresh, max_per_image, also_info_form"""
    R, C = DET_R, DET_C
    rng = np.random.default_rng(["quantised", "cut_in_ties", "empty_full_single", "thresh_on_a_score", "no_cut"].index(case))
    im_h, im_w = 600.0, 1000.0
    xy = rng.uniform(0, 1, (R, 2)) * [im_w - 120, im_h - 120]
    wh = rng.uniform(16, 300, (R, 2))
    rois = np.concatenate([np.zeros((R, 1)), xy, np.minimum(xy + wh, [im_w - 1, im_h - 1])], 1).astype(F32)
    rois[R // 2:, 1:] = rois[:R - R // 2, 1:] + rng.uniform(-6, 6, (R - R // 2, 4)).astype(F32)   # clusters: the NMS has work
    pred = (rng.standard_normal((R, 4 * C)) * 0.5).astype(F32)
    if case == "quantised":
        return rois, _quantised_prob(rng, 64), pred, (im_h, im_w, 1.0), 0.0, 100, False
    if case == "cut_in_ties":
        return rois, _quantised_prob(rng, 16), pred, (im_h, im_w, 0.75), 0.0, 20, True
    if case == "empty_full_single":
        prob = _quantised_prob(rng, 64)
        prob[:, 3] = 1.0 / 128                                       # class 3: nothing above the threshold
        prob[:, 4] = (0.25 + (rng.permutation(R) + 1.0) / (2 * R)).astype(F32)      # class 4: all R rows above it
        prob[:, 5] = 1.0 / 128                                       # class 5: exactly one row above it
        prob[R // 3, 5] = 0.5
        return rois, prob, pred, (im_h, im_w, 1.6), 1.0 / 64, 100, True
    if case == "thresh_on_a_score":
        prob = _quantised_prob(rng, 64)
        assert all((prob[:, j] == F32(4.0 / 64)).any() for j in range(1, C))
        return rois, prob, pred, (im_h, im_w, 1.6), 4.0 / 64, 0, False       # no cut: the lowest kept scores stay visible
    if case == "no_cut":
        return rois, _quantised_prob(rng, 64), pred, (im_h, im_w, 1.25), 0.0, 0, False
    raise ValueError(case)


def _det_reference(orpn, case):
    rois, prob, pred, (im_h, im_w, scale), thresh, maxdet, _ = _det_case(case)
    want = orpn.detection_postprocess(rois, prob, pred, im_h, im_w, scale, False, DET_STDS, DET_MEANS, thresh, 0.3, maxdet)
    n = [len(w) for w in want]
    scores = np.concatenate([w[:, 4] for w in want])
    assert max(np.unique(w[:, 4], return_counts=True)[1].max() for w in want if len(w)) > 1      # tied scores inside a class
    if case == "cut_in_ties":
        # the 20th largest kept score is shared by >= 3 kept detections of >= 2 classes, so `>= image_thresh` returns > 20
        cut = np.sort(scores)[-maxdet]
        assert sum(n) > maxdet and (scores == cut).sum() >= 3 and sum((w[:, 4] == cut).any() for w in want) >= 2
        assert (scores > cut).sum() < maxdet
    if case == "empty_full_single":
        assert n[3] == 0 and n[5] == 1 and (prob[:, 4] > F32(thresh)).all() and (prob[:, 3] <= F32(thresh)).all()
        assert n[4] > 1
    if case == "thresh_on_a_score":
        assert (scores > F32(thresh)).all() and (scores == F32(5.0 / 64)).any()
    if case == "no_cut":
        assert sum(n) > 100
    return want


@pytest.mark.parametrize("case", ["quantised", "cut_in_ties", "empty_full_single", "thresh_on_a_score", "no_cut"])
def test_detection_postprocess_at_its_decision_boundaries(ops, oracle, case):
    """Tied scores inside classes, the image-wide cut inside a run of ties (more than max_per_image come back), an
    empty class beside a full one beside a single-row one, a threshold equal to a score (strict >), and no cut at all.
    Same per-class counts and bit-equal rows as the oracle; the im_info form returns what the host-scalar form does."""
    _, orpn = oracle
    want = _det_reference(orpn, case)
    rois, prob, pred, (im_h, im_w, scale), thresh, maxdet, info_form = _det_case(case)
    args = tuple(_dev(a) for a in (rois, prob, pred))
    dets, counts = ops.detection_postprocess(*args, im_h, im_w, scale, False, DET_STDS, DET_MEANS, thresh, 0.3, maxdet)
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    assert counts[0] == 0
    for j in range(1, DET_C):
        assert counts[j] == len(want[j]), (j, counts[j], len(want[j]))
        assert np.array_equal(dets[j, :counts[j]], want[j]), j
    if info_form:
        dets2, counts2 = ops.detection_postprocess(*args, 0.0, 0.0, 0.0, False, DET_STDS, DET_MEANS, thresh, 0.3, maxdet,
                                                   im_info=_dev(np.array([im_h, im_w, scale], F32)))
        dets2, counts2 = dets2.cpu().numpy(), counts2.cpu().numpy()
        assert np.array_equal(counts2, counts)
        for j in range(1, DET_C):
            assert np.array_equal(dets2[j, :counts[j]], dets[j, :counts[j]]), j


# ----------------------------------------------------------------------------- 4. relation_topk
REL_SHAPES = [(9, 26), (32, 132), (33, 125)]           # (32, 132): 130944 cells, below 2^17; (33, 125): 132000, above
REL_VARIANTS = ["plain", "padded_boxes", "twin_rows", "logits_and_zero_conf"]


def _rel_case(n_boxes, n_rel, variant):
    rng = np.random.default_rng([n_boxes, n_rel, REL_VARIANTS.index(variant)])
    ixs, ixo = (a.ravel() for a in np.nonzero(~np.eye(n_boxes, dtype=bool)))            # all ordered pairs
    n_pairs = ixs.size
    assert n_pairs == n_boxes * (n_boxes - 1)
    rel = rng.uniform(0.0, 1.0, (n_pairs, n_rel)).astype(F32)
    conf = rng.uniform(0.1, 0.9, n_boxes).astype(F32)
    if variant in ("padded_boxes", "logits_and_zero_conf"):
        conf[n_boxes - n_boxes // 3:] = 0.0                 # RelationStep's spare boxes: whole rows of the grid are 0
    if variant == "logits_and_zero_conf":
        rel = rng.standard_normal((n_pairs, n_rel)).astype(F32)
    if variant == "twin_rows":                              # two pairs of equal confidence with the same predicate row,
        conf[:3] = 1.0                                      # both among the best cells
        a = int(np.nonzero((ixs == 0) & (ixo == 1))[0][0])
        b = int(np.nonzero((ixs == 1) & (ixo == 2))[0][0])
        rel[b] = rel[a]
    # lib/utils.py:584-628: float32_row * python_float * python_float, two fp32 roundings
    p = (rel * conf[ixs][:, None]).astype(F32)
    p = (p * conf[ixo][:, None]).astype(F32)
    flat = p.ravel()
    order = np.argsort(-flat, kind="stable")
    if variant == "padded_boxes":
        assert (_bits(flat) == 0).sum() >= n_rel and not (_bits(flat) == 0x80000000).any()
    if variant == "logits_and_zero_conf":
        assert (_bits(flat) == 0).any() and (_bits(flat) == 0x80000000).any()          # -0.0 among the +0.0 cells
    if variant == "twin_rows":
        assert a != b and np.array_equal(p[a], p[b])
        top = order[:100] // n_rel
        assert (top == a).any() and (top == b).any()
    return rel, conf, ixs.astype(np.int64), ixo.astype(np.int64), flat, order


@pytest.mark.parametrize("variant", REL_VARIANTS)
@pytest.mark.parametrize("n_boxes,n_rel", REL_SHAPES)
def test_relation_topk_vs_stable_numpy_ranking(ops, n_boxes, n_rel, variant):
    """i2v_relation_topk called directly: the first k cells of the stable descending order of the scaled grid, for k = 1,
    100 and the whole grid (which reaches into the rows of zeros, whose order is then checked too)."""
    rel, conf, ixs, ixo, flat, order = _rel_case(n_boxes, n_rel, variant)
    dev = tuple(_dev(a) for a in (rel, conf, ixs, ixo))
    for k in (1, 100, flat.size):
        pair, pred, out = (t.cpu().numpy() for t in ops.relation_topk(*dev, k=k))
        assert pair.shape == pred.shape == out.shape == (k,)
        assert np.array_equal(pair, order[:k] // n_rel), k
        assert np.array_equal(pred, order[:k] % n_rel), k
        assert np.array_equal(_bits(out), _bits(flat[order[:k]])), k
