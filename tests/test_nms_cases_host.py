"""The NMS edge cases of tests/nms_cases.py, host side (no GPU): every case is held to the oracle through both host helpers, and
the regime it was built for is asserted here -- the sweeps each 1024-row super-block needs, the pairs inside and just outside the
mask kernel's band, the exact hits of the threshold -- so that a case which drifts out of its regime fails on the CPU instead of
passing silently on the GPU (tests/test_gpu_nms_edges.py)."""
import functools

import numpy as np
import pytest

import nms_cases as nc

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _ladders():
    return {c.name: c for c in nc.ladder_cases()}


@functools.lru_cache(maxsize=None)
def _threshold(thresh):
    return nc.threshold_case(thresh)


def _check_against_oracle(case, parts=True):
    from oracle import cops
    S = nc.suppression_matrix(case.dets, case.thresh)[0] if parts else nc.suppression_matrix(case.dets, case.thresh, parts=False)
    ref = cops.nms_sorted(case.dets, case.thresh)
    T, keep = nc.sweeps_to_settle(S)
    assert np.array_equal(keep, ref), case.name
    assert np.array_equal(nc.greedy_keep(S), ref), case.name
    s = case.dets[:, 4]
    assert case.dets.dtype == F32 and (np.diff(s) < 0).all()
    return S, T, ref


LADDER_T = {"cap48_L47": [47], "cap48_L48": [48], "cap48_L49": [49], "cap5_L4": [4], "cap5_L5": [5], "cap5_L6": [6],
            "whole_super_block": [1, 1024, 1], "straddle": [24, 76, 1], "three_regimes": [10, 60, 20],
            "end_n1023": [40], "end_n1024": [40], "end_n1025": [39, 1], "end_n2047": [1, 100], "end_n2048": [1, 100],
            "end_n2049": [1, 99, 1], "end_n12352": [1] * 11 + [36, 64], "end_n12353": [1] * 11 + [35, 64]}


def test_ladder_table_is_complete():
    assert sorted(LADDER_T) == sorted(_ladders())
    assert nc.NMS_SWEEPS == 48 and nc.SUPER_ROWS == 1024
    # 12352 rows are the last n the super-block scan takes (nblk - 1 <= 192), 12353 the first of the generic scan
    assert (12352 + 63) // 64 - 1 == 192 and (12353 + 63) // 64 - 1 == 193
    # ... and so says the library's own plan (csrc/roi_plan.h through i2v_nms_plan; fields: include/i2vsgg_hip.h)
    import ctypes
    from i2vsgg_amd import build
    build.build()
    from i2vsgg_amd._lib import lib
    out = (ctypes.c_int32 * 11)()
    forms = []
    for n in (12352, 12353):
        assert lib.i2v_nms_plan(1, n, out, 11) == 0 and out[0] == 0 and out[1] == (n + 63) // 64
        forms.append((out[6], out[7]))
    assert forms == [(0, nc.NMS_SWEEPS), (2, 0)]             # SUPER with the default sweeps, then GENERIC


@pytest.mark.parametrize("name", sorted(LADDER_T))
def test_ladder_case_needs_the_intended_sweeps(name):
    """Per super-block: T as written down above, as the builder predicts, and as the fixed-point iteration measures; the keep list
    is the oracle's and keeps every other ladder row."""
    case = _ladders()[name]
    n = case.dets.shape[0]
    S, T, ref = _check_against_oracle(case, parts=n <= 3000)
    assert T == LADDER_T[name] == case.T, (name, T, case.T)
    kept = np.zeros(n, bool)
    kept[ref] = True
    for start, L in case.ladders:
        assert kept[start:start + L:2].all() and not kept[start + 1:start + L:2].any()
        assert np.abs(case.dets[start:start + L, :4]).max() < 2 ** 24
    rest = np.ones(n, bool)
    for start, L in case.ladders:
        rest[start:start + L] = False
    assert kept[rest].all() and not S[rest].any() and not S[:, rest].any()           # the filler overlaps nothing
    caps = nc.caps_for(case, ref)
    k1 = int((ref < nc.SUPER_ROWS).sum())
    assert caps[0] == 0 and 1 in caps and k1 in caps and k1 + 1 in caps and (k1 - 1 in caps or k1 == 1)
    for start, L in case.ladders:                            # a cut whose last kept row lies inside the ladder
        assert any(c and start < ref[c - 1] < start + L - 1 for c in caps if c <= ref.size), (name, start)


def test_ladder_regimes_per_scan_form():
    """What each sweep cap does with the cases built around it: one sweep to spare, settled on the last, fallen back."""
    c = _ladders()
    for cap, names in ((48, ("cap48_L47", "cap48_L48", "cap48_L49")), (5, ("cap5_L4", "cap5_L5", "cap5_L6"))):
        t = [c[k].T[0] for k in names]
        assert t == [cap - 1, cap, cap + 1]
    T = c["three_regimes"].T
    assert T[0] <= 48 < T[1] and T[2] <= 48                  # settled / fallback / settled in one launch
    assert max(c["whole_super_block"].T) == 1024
    assert c["straddle"].ladders == ((1000, 100),)           # rows 1000 .. 1099 over the edge at 1024


def test_batched_case():
    imgs = nc.batched_case()
    assert len({c.dets.shape for c in imgs}) == 1
    T = []
    for c in imgs:
        _, t, _ = _check_against_oracle(c)
        assert t == c.T
        T.append(t)
    assert T == [[10, 1], [24, 76], [1, 1]]


def test_detection_ladder_decodes_to_the_ladder():
    """Zero deltas and im_scale 1: the boxes detection_postprocess hands to the NMS are the 60-row ladder plus filler, for every
    class in roi order -- 60 sweeps, past the default cap."""
    from oracle import cops, rpn
    rois, prob, pred, want, (im_h, im_w) = nc.detection_ladder()
    assert rois.shape == (128, 5) and prob.shape == (128, 4) and not pred.any()
    assert np.array_equal(cops.decode_clip(rois[:, 1:], pred[:, :4], im_h, im_w), want)
    case = nc.Case("det", nc.with_scores(want), nc.LADDER_THRESH, None, (), None)
    _, T, ref = _check_against_oracle(case)
    assert T == [60] and T[0] > nc.NMS_SWEEPS and ref.size == 128 - 30
    out = rpn.detection_postprocess(rois, prob, pred, im_h, im_w, 1.0, False, None, None, 0.0, nc.LADDER_THRESH, 0)
    for j in range(1, 4):
        assert np.array_equal(out[j][:, :4], want[ref]) and np.array_equal(out[j][:, 4], prob[ref, j])


@pytest.mark.parametrize("thresh", nc.THRESHOLDS)
def test_threshold_pairs_surround_the_band(thresh):
    """Every pair of families (a) and (b) classified by the kernel's own band constants, compares in float32."""
    case = _threshold(thresh)
    S, inter, d, ovr = nc.suppression_matrix(case.dets, thresh)
    _check_against_oracle(case)
    ra, rb, fam = (np.array(v) for v in zip(*case.pairs))
    assert (ra < rb).all() and len(set(ra.tolist() + rb.tolist())) == 2 * len(ra)
    # no pair interacts with another: the only suppressions of the case are inside pairs
    own = np.zeros_like(S)
    own[ra, rb] = True
    assert not (S & ~own).any()
    # the placements: rows (r, r + 1) inside a tile, across the tile edge 63 / 64, and (r, r + 64)
    gap = rb - ra
    assert set(gap.tolist()) == {1, 64}
    assert ((gap == 1) & (ra % 64 == 63)).sum() >= 4 and ((gap == 1) & (ra % 64 != 63)).sum() >= 200 and (gap == 64).sum() >= 200
    pi, pd, po, ps = inter[ra, rb], d[ra, rb], ovr[ra, rb], S[ra, rb]
    cls = nc.band_class(pi, pd, thresh)
    dist = nc.band_distance(pi, pd, thresh)
    assert (ps[cls == 1]).all() and not (ps[cls == -1]).any()                # the proof of rpn.hip on these pairs
    inside = cls == 0
    near_over = (cls == 1) & (dist <= 5.0)
    near_under = (cls == -1) & (dist >= -5.0)
    exact = po == F32(thresh)
    counts = dict(inside=int(inside.sum()), near_over=int(near_over.sum()), near_under=int(near_under.sum()), exact=int(exact.sum()),
                  inside_suppressed=int(ps[inside].sum()), inside_kept=int((~ps[inside]).sum()))
    print("thresh %.1f: %d pairs, %s" % (thresh, len(ra), counts))
    assert counts["inside"] >= 32 and counts["near_over"] >= 32 and counts["near_under"] >= 32 and counts["exact"] >= 8, counts
    assert counts["inside_suppressed"] >= 1 and counts["inside_kept"] >= 1, counts
    assert not ps[exact].any()                                               # ovr == thresh is kept (nms_cpu.py:31)
    # one ulp to either side of the threshold, too
    up, down = np.nextafter(F32(thresh), F32(2)), np.nextafter(F32(thresh), F32(0))
    assert (po == up).any() and (po == down).any()
    # family (a): the operations were exact -- inter = wa, d = wb for the one-pixel-high boxes
    a = fam == "a"
    one_high = a & (case.dets[ra, 3] == case.dets[ra, 1]) & (pd > 1.0e6)
    assert one_high.sum() == 12 * 17
    wa = np.minimum(case.dets[ra, 2], case.dets[rb, 2]).astype(np.float64) + 1.0
    wb = np.maximum(case.dets[ra, 2], case.dets[rb, 2]).astype(np.float64) + 1.0
    assert (pi[one_high] == wa[one_high]).all() and (pd[one_high] == wb[one_high]).all()
    # thi, tlo and their products with d round (2^-24 each, an eighth of the half-width 2^-21): the band's edge is where it
    # should be to a quarter of its half-width, and the seventeen k of a wb lie on both sides of both edges
    assert inside[one_high & (np.abs(dist) <= 0.7)].all() and not inside[one_high & (np.abs(dist) >= 1.3)].any()
    for sign in (-1, 1):
        assert (one_high & (cls == sign)).sum() >= 12 * 4 and (one_high & inside & (np.sign(dist) == sign)).sum() >= 12
    # family (b): two adjacent shifts, two decisions; some areas beyond 2^24
    b = np.nonzero(fam == "b")[0]
    assert b.size == 2 * nc.N_BASE
    area = (case.dets[:, 2] - case.dets[:, 0] + F32(1)) * (case.dets[:, 3] - case.dets[:, 1] + F32(1))
    assert (np.minimum(area[ra[b]], area[rb[b]]) > 2 ** 24).sum() >= nc.N_LARGE
    twins = {}
    for k in b:                                  # twins share the base box's x1 / x2 and height
        lo = ra[k] if case.dets[ra[k], 0] <= case.dets[rb[k], 0] else rb[k]
        key = (case.dets[lo, 0].tobytes(), case.dets[lo, 2].tobytes(), (case.dets[lo, 3] - case.dets[lo, 1]).tobytes())
        twins.setdefault(key, []).append(k)
    assert len(twins) == nc.N_BASE
    for key, (k0, k1) in twins.items():
        assert ps[k0] != ps[k1]
        p0, p1 = (case.dets[max(ra[k], rb[k], key=lambda r: case.dets[r, 0]), 0:3:2] for k in (k0, k1))
        assert not np.array_equal(p0, p1) and np.abs(p0 - p1).max() <= 2 * np.spacing(np.abs(p0).max())


@pytest.mark.parametrize("k", range(3))
def test_degenerate_cases(k):
    """The degenerate boxes do what the issue lists in the reference arithmetic: 0 / 0 suppresses, 0 / negative keeps, a NaN row
    that is alive removes everything behind it.  The truth stays the oracle."""
    case = nc.degenerate_cases()[k]
    S, _, ref = _check_against_oracle(case)
    b = case.dets[:, :4]
    _, inter, d, ovr = nc.suppression_matrix(case.dets, case.thresh)
    with np.errstate(all="ignore"):
        w, h = b[:, 2] - b[:, 0] + F32(1), b[:, 3] - b[:, 1] + F32(1)
    bad = ~((w > 0) & (h > 0))
    if case.name == "mixed":
        up = np.triu(np.ones_like(S), 1)
        assert bad.sum() >= 10 and bad[63] and bad[64]
        assert (np.isnan(ovr) & up & (d == 0)).any()                         # 0 / 0
        assert ((ovr == 0) & np.signbit(ovr) & up).any()                     # 0 / negative = -0: kept
        assert (np.isinf(b).any(1)).sum() >= 4 and np.isnan(b).any()
        assert ((w < 0) & (h < 0)).sum() >= 3                              # both sides negative: positive area
        assert 20 < ref.size < case.dets.shape[0] - 20
    elif case.name == "nan_first":
        assert np.isnan(b[0]).any() and ref.tolist() == [0]
    else:
        r = int(np.nonzero(np.isnan(b).any(1))[0][0])
        assert r == 70 and r not in ref and S[:r, r].all() and ref.size > 10
