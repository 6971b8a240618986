"""Box voting, host side (no GPU): the host form of i2vsgg_amd/box_vote.py -- the specification a device kernel is to be held
to -- on a hand-worked case, on the properties the rules promise, against planted wrong variants, and on a seeded set where voting
must localise better than the top-scoring candidate."""
import numpy as np
import pytest

import box_vote_cases as bc
from i2vsgg_amd import box_vote as bv
from i2vsgg_amd import soft_nms as sn

F32 = np.float32


def _vote(kept, cands, thresh=bc.T, stats=None):
    return bv.box_vote_host(kept, None, cands, None, thresh, stats)[0]


def _iou(a, b):
    """float32 IoU of two boxes through soft_nms.iou_row."""
    t = np.array([np.asarray(a, F32)[:4], np.asarray(b, F32)[:4]], F32)
    area = (t[:, 2] - t[:, 0] + F32(1)) * (t[:, 3] - t[:, 1] + F32(1))
    return sn.iou_row(t, area, 0)[1]


def variant(kept, cands, thresh, strict=False, acc=np.float64, weighted=True, weights=None):
    """The rules written a second time, row by row in scalars, with the planted mistakes as switches: ``strict`` votes on > instead
    of >=, ``acc`` accumulates in another type, ``weighted=False`` takes the plain mean, ``weights`` replaces the candidate scores."""
    out = np.array(kept, F32)
    w = np.asarray(cands[:, 4] if weights is None else weights, F32)
    for r in range(len(kept)):
        den, num = acc(0), [acc(0)] * 4
        for c in range(len(cands)):
            iou = _iou(kept[r], cands[c])
            if not (iou > F32(thresh) if strict else iou >= F32(thresh)):
                continue
            s = acc(w[c]) if weighted else acc(1)
            den = den + s
            num = [num[q] + s * acc(cands[c, q]) for q in range(4)]
        if den != 0:
            out[r, :4] = [F32(num[q] / den) for q in range(4)]
    return out


# ---------------------------------------------------------------------------------------------- a hand-worked case
def test_hand_worked_three_candidates():
    # kept A = [0, 0, 9, 9] (10 x 10, area 100).  Candidates: A itself, s = 0.9; B = [0, 0, 9, 8] (area 90, inter 90:
    # IoU = 90 / (100 + 90 - 90) = 0.9 >= 0.8, votes), s = 0.6; C = [0, 0, 9, 6] (area 70: IoU = 0.7, does not vote), s = 0.5.
    # x1, y1 and x2 are the same in A and B and stay; y2 = (0.9f * 9 + 0.6f * 8) / (0.9f + 0.6f) in float64, rounded once.
    kept = np.array([[0, 0, 9, 9, 0.9]], F32)
    cands = np.array([[0, 0, 9, 9, 0.9], [0, 0, 9, 8, 0.6], [0, 0, 9, 6, 0.5]], F32)
    assert _iou(kept[0], cands[1]) == F32(90) / F32(100) and _iou(kept[0], cands[2]) == F32(70) / F32(100)
    a, b = np.float64(F32(0.9)), np.float64(F32(0.6))
    y2 = F32((a * 9.0 + b * 8.0) / (a + b))
    assert abs(float(y2) - 8.6) < 1e-6
    stats = {}
    out = _vote(kept, cands, stats=stats)
    assert stats["voters"][0].tolist() == [2]
    assert out.view(np.int32).tolist() == np.array([[0, 0, 9, y2, 0.9]], F32).view(np.int32).tolist()
    assert np.array_equal(variant(kept, cands, bc.T), out)
    # at a threshold of 0.7 C votes too (>=); at 0.95 only A itself, and the row keeps its bits
    y2c = F32((a * 9.0 + b * 8.0 + 0.5 * 6.0) / (a + b + 0.5))
    assert _vote(kept, cands, 0.7)[0, 3] == y2c and _vote(kept, cands, 0.95).tobytes() == kept.tobytes()


# ---------------------------------------------------------------------------------------------- the properties
def test_threshold_pairs_vote_as_stated():
    """PAIRS: the float32 IoU is the stated fraction; a pair exactly on float32(0.8) votes under >=, and stops voting one
    float32 step above."""
    assert F32(bc.T_UP) > F32(0.8) and F32(bc.T_UP) == np.nextafter(F32(0.8), F32(1))
    for a, b, (p, q), at_t, at_up in bc.PAIRS:
        iou = _iou(a, b)
        assert iou == F32(p) / F32(q)
        assert (iou == F32(0.8)) == (at_t and not at_up)
        kept = np.array([a + [0.9]], F32)
        cands = np.array([a + [0.9], b + [0.7]], F32)
        for thresh, votes in ((bc.T, at_t), (bc.T_UP, at_up)):
            stats = {}
            out = _vote(kept, cands, thresh, stats)
            assert stats["voters"][0].tolist() == [2 if votes else 1], (a, b, thresh)
            assert (out.tobytes() != kept.tobytes()) == votes
            assert np.array_equal(out[:, 4], kept[:, 4])


@pytest.mark.parametrize("n", (2, 65, 300))
def test_properties_of_every_family(n):
    seen = set()
    for thresh, batch in bc.batches(n):
        for c in batch:
            what = (c.family, n, len(c.cands), thresh)
            seen.add(c.family)
            assert c.want.shape == c.kept.shape and np.array_equal(c.want[:, 4].view(np.int32), c.kept[:, 4].view(np.int32)), what
            none = c.voters == 0
            assert c.want[none].tobytes() == c.kept[none].tobytes(), what           # no voter: the bits stay
            if len(c.cands):                                                         # a mean lies inside its voters' range
                lo, hi = c.cands[:, :4].min(0), c.cands[:, :4].max(0)
                assert (c.want[~none, :4] >= lo).all() and (c.want[~none, :4] <= hi).all(), what
            if c.family == "stack" and len(c.cands):
                assert (c.voters == len(c.cands)).all() and c.want.tobytes() == c.kept.tobytes(), what      # the same box, exactly
            if c.family == "self":
                assert (c.voters == 1).all() and c.want.tobytes() == c.kept.tobytes(), what                 # s * q / s rounds back to q
                if n >= 300:
                    assert len(c.kept) == bc.KEPT_MAX
            if c.family == "degenerate" and len(c.cands) >= 40:
                area = (c.kept[:, 2] - c.kept[:, 0] + F32(1)) * (c.kept[:, 3] - c.kept[:, 1] + F32(1))
                assert (area == 0).sum() >= 3 and (c.voters[area == 0] == 0).all() and (c.voters[area > 0] > 0).all(), what
            if c.family == "crowd" and len(c.cands) >= 63:
                assert (c.voters > len(c.cands) // 2).all() and (bc.ulps(c.want[:, :4], c.kept[:, :4]) > 1).any(), what
            if c.family == "threshold" and len(c.cands) >= 10:
                exact = np.array([bc.PAIRS[j % len(bc.PAIRS)][3] and not bc.PAIRS[j % len(bc.PAIRS)][4] for j in range(len(c.kept))])
                assert (c.voters[exact] == (2 if thresh == bc.T else 1)).all(), what
            if c.family == "large" and len(c.cands) >= 63:
                assert c.kept[:, :4].min() > 3700 and c.cands[:, 4].min() < 0.002 and c.cands[:, 4].max() > 0.9, what
    assert seen == set(bc.FAMILIES)


def test_the_capacity_case_has_more_than_2048_voters_for_one_row():
    c = bc.case("crowd", 4096)
    assert len(c.cands) == 4096 and (c.voters > 2048).all()
    c = bc.case("clustered", 4096)
    assert len(c.kept) == bc.KEPT_MAX and c.voters.max() > 100


def test_counts_clamp_and_rows_behind_them_are_ignored():
    batch = bc.batches(65)[0][1]
    kept, kc, cands, cc = bc.pack(batch, 65)
    out = bv.box_vote_host(kept, kc, cands, cc, bc.T)
    for i, c in enumerate(batch):
        assert out[i, :kc[i]].tobytes() == c.want.tobytes() and out[i, kc[i]:].tobytes() == kept[i, kc[i]:].tobytes()
    assert np.array_equal(bv.box_vote_host(kept, kc + 1000, cands, cc * 0 - 5, bc.T), kept)       # no candidate: nothing moves
    assert bv.box_vote_host(np.zeros((2, 0, 5), F32), None, cands[:2], None).shape == (2, 0, 5)
    with pytest.raises(ValueError):
        bv.box_vote_host(kept, kc, cands[:2], cc[:2])


@pytest.mark.parametrize("family,count", [("clustered2", 65), ("crowd", 63), ("large", 128), ("threshold", 20)])
def test_the_scalar_form_agrees_with_the_host_form(family, count):
    c = bc.case(family, count)
    assert variant(c.kept, c.cands, c.thresh).tobytes() == c.want.tobytes()


def test_planted_wrong_variants_are_told_apart():
    def differs(c, **kw):
        return variant(c.kept, c.cands, c.thresh, **kw).tobytes() != c.want.tobytes()

    thr, crowd, large, clus = bc.case("threshold", 20), bc.case("crowd", 63), bc.case("large", 128), bc.case("clustered2", 65)
    assert differs(thr, strict=True)                        # > for >=: the pairs exactly on float32(0.8) stop voting
    assert differs(large, acc=np.float32) and differs(crowd, acc=np.float32)       # float32 accumulation
    assert differs(crowd, weighted=False) and differs(clus, weighted=False)        # an unweighted mean
    # decayed scores as weights: linear Soft-NMS of the candidates, every row kept (min_score below any score), scattered back
    for c in (crowd, clus):
        out, src, num = sn.soft_nms_host(c.cands, None, "linear", 0.3, min_score=-1.0)
        assert int(num[0]) == len(c.cands)
        decayed = np.zeros(len(c.cands), F32)
        decayed[src[0]] = out[0, :, 4]
        assert (decayed < c.cands[:, 4]).any()
        assert differs(c, weights=decayed)
    for c in (thr, crowd, large, clus):                     # and the switches off give the host form
        assert not differs(c)


def test_voting_localises_better_than_the_top_candidate():
    """200 objects of 200 x 150 px, 12 candidates each with every coordinate jittered by N(0, 6 px), scores U(0.3, 1): the voted box
    of the top-scoring candidate has a higher mean IoU with the object than that candidate itself."""
    rng = np.random.default_rng(0)
    n_obj, n_c = 200, 12
    xy = rng.uniform([50, 50], [700, 400], (n_obj, 2))
    obj = np.concatenate([xy, xy + [199.0, 149.0]], 1).astype(F32)
    boxes = (obj[:, None, :] + rng.normal(0, 6.0, (n_obj, n_c, 4))).astype(F32)
    scores = rng.uniform(0.3, 1.0, (n_obj, n_c)).astype(F32)
    order = np.argsort(-scores, 1, kind="stable")
    cands = np.concatenate([np.take_along_axis(boxes, order[:, :, None], 1), np.take_along_axis(scores, order, 1)[:, :, None]], 2)
    kept = cands[:, :1].copy()
    stats = {}
    out = bv.box_vote_host(kept, None, cands, None, bc.T, stats)
    before = np.array([float(_iou(obj[i], kept[i, 0])) for i in range(n_obj)])
    after = np.array([float(_iou(obj[i], out[i, 0])) for i in range(n_obj)])
    assert np.mean([v[0] for v in stats["voters"]]) > 6
    print("mean IoU with the object: top candidate %.4f, voted %.4f; better for %d of %d" % (before.mean(), after.mean(),
                                                                                          (after > before).sum(), n_obj))
    assert after.mean() > before.mean()


def test_options():
    assert bv.options(None) is None
    assert bv.options(0.8) == float(F32(0.8)) and bv.options(1) == 1.0 and bv.options(np.float32(0.5)) == 0.5
    for bad in (0.0, -0.1, 1.0001, float("nan"), "0.8", True, (0.8,), [0.8]):
        with pytest.raises(ValueError):
            bv.options(bad)
