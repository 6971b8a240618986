"""The built cases of tests/target_cases.py have the properties they claim, the oracle's numpy statement of the target path
(oracle.rpn.iou_matrix / box_targets / anchor_target_layer / proposal_target_layer) agrees on them with the exact and the
plain statements there, and with what the reference itself returned (tests/golden/target_edges.npz, tools/gen_golden.py
gen_target_edges).  CPU only.  The GPU test (tests/test_gpu_target_edges.py) compares the kernels and layers with the oracle
on the same cases; that those comparisons have teeth is shown here: every deliberately wrong variant of the plain rules
(``>`` for ``>=``, last-index argmax, the fills in the other order, a fused multiply-subtract in the union) is told apart by
at least one case."""
import functools

import numpy as np
import pytest

import target_cases as tc
from conftest import golden, record_margin
from oracle import rpn

F32 = np.float32
Fr = tc.Fr


@functools.lru_cache(maxsize=None)
def gold():
    return golden("target_edges")


def oracle_overlaps(boxes, gt):
    ov = rpn.iou_matrix(boxes, gt)
    return ov, ov.max(1), ov.argmax(1).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------- overlaps
def test_anchor_grid_is_the_oracles():
    assert np.array_equal(tc.anchor_grid(), rpn.anchor_grid(38, 63))
    assert np.array_equal(tc.anchor_grid(20, 20), rpn.anchor_grid(20, 20))
    g = tc.anchor_grid()
    assert np.array_equal(g, np.round(g))                                  # integer corners
    sides = {(int(b[2] - b[0] + 1), int(b[3] - b[1] + 1)) for b in tc.base_anchors()}
    assert all(w % 8 == 0 and h % 8 == 0 and w % 5 and h % 5 for w, h in sides), sides


def test_threshold_pairs_sit_where_they_claim():
    """Fractions: "at" pairs equal the constant, "low" / "high" pairs are strictly to either side (at 0.0 the low side is 0
    again); in fp32 the "at" IoU is the fp32 constant bit for bit and compares with the python constant as the rational does
    with the rational."""
    case = tc.threshold_case()
    pairs = tc.threshold_pairs()
    ov, _, _ = oracle_overlaps(case.boxes, case.gt[0])
    inside = {tuple(int(v) for v in a) for a in tc.anchor_grid()[tc.inside_mask(tc.anchor_grid(), tc.IM_H, tc.IM_W)]}
    seen = set()
    for (i, key, side, fam), (_, _, _, box, gt) in zip(case.prop["pairs"], pairs):
        c, v = tc.CONSTANTS[key], tc.iou_fraction(box, gt)
        assert v == tc.iou_fraction(case.boxes[i], case.gt[0, i])
        if side == "at":
            assert v == c, (key, fam, v)
            assert ov[i, i] == F32(float(c)) and ov[i, i].dtype == F32
        elif side == "high":
            assert v > c and ov[i, i] > F32(float(c)), (key, fam, v)
        elif c == 0:
            assert v == 0 and ov[i, i] == 0
        else:
            assert v < c and ov[i, i] < F32(float(c)), (key, fam, v)
        for const in tc.CONSTANTS.values():                                # fp32 value against python float, as the layers compare
            assert (ov[i, i] >= float(const)) == (v >= const) and (ov[i, i] < float(const)) == (v < const), (key, side, fam, const)
        if fam.startswith("anchor"):
            assert tuple(box) in inside
            iw = min(box[2], gt[2]) - max(box[0], gt[0]) + 1
            ih = min(box[3], gt[3]) - max(box[1], gt[1]) + 1
            if key != "0.0":
                assert 0 < ih < min(box[3] - box[1] + 1, gt[3] - gt[1] + 1) and iw == box[2] - box[0] + 1      # a partial overlap
            seen.add((key, side))
    assert {("0.7", "at"), ("0.3", "at")} <= seen
    assert len(pairs) == 5 * 3 * 3


def test_zero_area_rules():
    case = tc.zero_area_case()
    ov, mx, am = oracle_overlaps(case.boxes, case.gt[0])
    normal = [r for r in range(len(case.boxes)) if r not in case.prop["minus_rows"]]
    for k in case.prop["zero_cols"]:
        assert (ov[normal, k] == 0).all()
    for r in case.prop["minus_rows"]:
        assert (ov[r] == -1).all() and mx[r] == -1 and am[r] == 0          # the -1 fill comes last, even on a unit gt
    assert np.array_equal(case.boxes[2], case.gt[0, 2, :4]) and tc.iou_fraction(case.boxes[2], case.gt[0, 2]) == -1
    assert tc.iou_fraction(case.boxes[3], case.gt[0, 2]) == 0              # a real unit gt inside a roi still counts 0
    for r in case.prop["all_zero_rows"]:
        assert (ov[r] == 0).all() and am[r] == 0


def test_tie_rules():
    case = tc.tie_case()
    ov, mx, am = oracle_overlaps(case.boxes, case.gt[0])
    assert am.tolist() == case.prop["argmax"]
    for r, (cols, val) in enumerate(zip(case.prop["tied"], case.prop["value"])):
        assert all(tc.iou_fraction(case.boxes[r], case.gt[0, k]) == val for k in cols)
        assert all(ov[r, k] == mx[r] for k in cols) and am[r] == min(cols)
        assert all(ov[r, k] < mx[r] for k in range(4) if k not in cols)
    assert case.gt[0, 0, 4] != case.gt[0, 1, 4]


def _all_overlap_cases():
    yield from tc.edge_overlap_cases()
    for form in tc.SHAPE_FORMS:
        for B in tc.SHAPE_B:
            for N in tc.SHAPE_N:
                for K in tc.SHAPE_K:
                    if K == 1024 and N not in (1, 257):
                        continue
                    yield tc.shape_case(B, N, K, form)


def test_oracle_overlaps_equal_the_plain_and_the_exact_statement():
    n = 0
    for case in _all_overlap_cases():
        for boxes, gt in tc.case_images(case):
            ov, mx, am = oracle_overlaps(boxes, gt)
            pov, pmx, pam = tc.plain_overlaps(boxes, gt)
            assert np.array_equal(ov, pov) and np.array_equal(mx, pmx) and np.array_equal(am, pam), case.name
            if case.name != "fractional":
                v = tc.exact_values(tc.exact_iu(boxes, gt))
                assert np.array_equal(v.astype(F32), ov), case.name       # float64 I / U rounded once more: the fp32 quotient
                assert np.array_equal(v.argmax(1), am), case.name         # no two different rationals collapse onto one fp32 maximum
            n += 1
    assert n > 100


def test_shape_cases_hold_what_they_plant():
    c = tc.shape_case(3, 257, 30, "b5")
    assert c.boxes.shape == (3, 257, 5) and c.gt.shape == (3, 30, 5) and (c.boxes[:, :, 0] == np.arange(3)[:, None]).all()
    assert (c.gt[:, 23:] == 0).all() and np.array_equal(c.gt[:, 0, :4], c.gt[:, 1, :4])
    ov, mx, am = oracle_overlaps(c.boxes[0, :, 1:], c.gt[0])
    assert mx[0] == 1 and am[0] == 0 and ov[0, 1] == 1 and (ov[-1] == -1).all() and (ov[:-1, 23:] == 0).all()
    assert tc.shape_case(1, 513, 1024, "shared").boxes.shape == (513, 4)
    assert tc.shape_case(3, 1, 1, "b4").boxes.shape == (3, 1, 4)


def test_oracle_overlaps_equal_the_reference():
    g = gold()
    for case in tc.edge_overlap_cases():
        ov, mx, am = oracle_overlaps(case.boxes, case.gt[0])
        assert np.array_equal(ov, g["ov_%s_ov" % case.name][0]), case.name
        assert np.array_equal(mx, g["ov_%s_max" % case.name][0]) and np.array_equal(am, g["ov_%s_argmax" % case.name][0]), case.name
    for N in tc.SHAPE_N:
        for K in tc.SHAPE_K:
            case = tc.shape_case(1, N, K, "shared")
            _, mx, am = oracle_overlaps(case.boxes, case.gt[0])
            assert np.array_equal(mx, g["sh_%s_max" % case.name][0]) and np.array_equal(am, g["sh_%s_argmax" % case.name][0]), case.name


# ----------------------------------------------------------------------------------------------------------- bbox_transform
def _ex_of(case):
    return np.broadcast_to(case.ex if case.ex.ndim == 3 else case.ex[None], case.gt.shape[:2] + (4,))


def test_box_targets_against_float64_and_the_reference():
    """dx, dy of the oracle within the fp32 evaluation bound of the float64 statement and bit-equal to the reference; dw, dh
    within numpy's own log error (measured here, recorded, and required to stay below the 4 ulp numpy documents for its fp32
    log) of the float64 log of the fp32 quotient; the reference's fp32 log within twice that of the oracle's."""
    g = gold()
    worst = tc.numpy_log_ulp()
    record_margin("test_box_targets_against_float64_and_the_reference", "numpy fp32 log vs float64 log (ulp)", worst, 4.0)
    assert worst < 4.0
    for case in tc.transform_cases():
        ex = _ex_of(case)
        got = np.stack([rpn.box_targets(ex[b], case.gt[b, :, :4]) for b in range(ex.shape[0])])
        want = tc.plain_box_targets(ex, case.gt)
        assert (np.abs(got[..., :2] - want[..., :2]) <= tc.dxdy_bound(ex, case.gt)).all(), case.name
        assert tc.log_ulp_of(got, ex, case.gt) <= worst
        assert (np.abs(got[..., 2:] - want[..., 2:]) <= (worst + 2) * np.spacing(np.abs(got[..., 2:])) + 2.0 ** -22).all()
        for r in case.prop["zero_rows"]:
            assert (got[:, r] == 0).all() and (want[:, r] == 0).all()
        ref = g["tf_%s_targets" % case.name]
        assert np.array_equal(got[..., :2], ref[..., :2]), case.name
        assert tc.log_ulp_of(ref, ex, case.gt) <= 2 * max(worst, 0.5), case.name
    mixed = tc.transform_cases()[0]
    assert mixed.gt.shape[2] == 5 and mixed.ex.ndim == 3 and tc.transform_cases()[1].ex.ndim == 2
    e, t = mixed.ex[0], mixed.gt[0]
    assert (t[2, 2] - t[2, 0] == 0) and (t[2, 3] - t[2, 1] == 0) and (t[4, 2] == t[4, 0]) and (e[5, 2] == e[5, 0]) and (e[5, 3] == e[5, 1])
    assert e[7, 0] == 0 and e[7, 1] == 0 and e[8, 2] == 999 and e[8, 3] == 599


# ----------------------------------------------------------------------------------------------------------- anchor scenes
def _inside_order(x, scene, inside):
    """(B, C*A*H*W...) maps back to the inside anchors: labels (B,1,A*H,W) -> (B,n); 4A-channel maps -> (B,n,4)."""
    H, W = scene.feat
    B = x.shape[0]
    if x.shape[1] == 1:
        return x.reshape(B, 9, H, W).transpose(0, 2, 3, 1).reshape(B, -1)[:, inside]
    return x.reshape(B, 9, 4, H, W).transpose(0, 3, 4, 1, 2).reshape(B, -1, 4)[:, inside]


@functools.lru_cache(maxsize=None)
def _scene_labels(name):
    scene = {s.name: s for s in tc.anchor_scenes()}[name]
    anc, inside, total = tc.scene_anchors(scene)
    exact = [tc.exact_anchor_labels(anc, scene.gt[b]) for b in range(scene.gt.shape[0])]
    return scene, anc, inside, total, exact


SCENES = [s.name for s in tc.anchor_scenes()]


@pytest.mark.parametrize("name", SCENES)
def test_anchor_scene_regimes_and_oracle(name):
    """Before subsampling: the oracle's labels (a batch size nothing exceeds) are the exact and the plain statement's; each scene
    lands in the regime it is built for.  With the reference's batch size and seed the oracle is the reference
    (labels, weights; targets where an anchor is labelled) -- on EVERY scene: the reference raises on none of them, frames
    without ground truth included."""
    scene, anc, inside, total, exact = _scene_labels(name)
    B = scene.gt.shape[0]
    L, T, IW, OW = rpn.anchor_target_layer(*scene.feat, scene.gt, scene.im_info, np.random.RandomState(3), rpn_batch=10 ** 9)
    lab = _inside_order(L, scene, inside)
    outside = np.setdiff1d(np.arange(total), inside)
    H, W = scene.feat
    assert (L.reshape(B, 9, H, W).transpose(0, 2, 3, 1).reshape(B, -1)[:, outside] == -1).all()
    tg = _inside_order(T, scene, inside)
    for b in range(B):
        plain, pam = tc.plain_anchor_labels(anc, scene.gt[b])
        assert np.array_equal(exact[b][0], plain) and np.array_equal(exact[b][0], lab[b]), (name, b)
        assert np.array_equal(exact[b][1], pam)
        assert np.array_equal(tg[b, :, :2], rpn.box_targets(anc, scene.gt[b, pam, :4])[:, :2])
    p = scene.prop
    n_fg = [int((e[0] == 1).sum()) for e in exact]
    n_bg = [int((e[0] == 0).sum()) for e in exact]
    for b in p.get("empty", []):
        assert n_fg[b] == 0 and n_bg[b] == anc.shape[0] > 256              # all background: the bg subsample runs, 256 are kept
    if name.startswith("empty"):
        other = 1 - p["empty"][0]
        assert 0 < n_fg[other] <= 128 and n_bg[other] > 256
    if "equal" in p:
        b, cell = p["equal"]
        i = np.nonzero(inside == tc.anchor_index(*cell))[0][0]
        assert tc.iou_fraction(anc[i], scene.gt[b, 0]) == 1 == tc.iou_fraction(anc[i], scene.gt[b, 1])
        assert exact[b][0][i] == 1 and exact[b][1][i] == 0 and scene.gt[b, 0, 4] != scene.gt[b, 1, 4]
    if "tiny" in p:
        b, k = p["tiny"]
        v = tc.exact_values(tc.exact_iu(anc, scene.gt[b]))
        tied = np.nonzero(v[:, k] == v[:, k].max())[0]
        assert tied.size >= 2 and Fr(64, 88 * 176) == tc.iou_fraction(anc[tied[0]], scene.gt[b, k]) < Fr(3, 10)
        assert (exact[b][0][tied] == 1).all()
        assert (v[tied].max(1) == v[tied, k]).all()                        # foreground only through ``ov == gt_max``
        b, k = p["outside"]
        iu = tc.exact_iu(anc, scene.gt[b])
        assert (iu[0][:, k] == 0).all() and n_fg[b] == 0 and n_bg[b] == anc.shape[0]
        grid = tc.anchor_grid(*scene.feat)
        assert (tc.exact_iu(grid, scene.gt[b])[0][:, k] > 0).any()          # outside anchors do overlap it
    for b, key, side, cell in p.get("pairs", []):
        i = np.nonzero(inside == tc.anchor_index(*cell, feat_w=scene.feat[1]))[0][0]
        best = max(tc.iou_fraction(anc[i], g) for g in scene.gt[b])
        c = tc.CONSTANTS[key]
        assert (best == c) if side == "at" else (best < c), (key, side, best)
        k = exact[b][1][i]
        v = tc.exact_values(tc.exact_iu(anc, scene.gt[b]))
        assert v[:, k].max() > v[i, k]                                     # not the box's best anchor: labelled by the threshold alone
        assert exact[b][0][i] == {("0.7", "at"): 1, ("0.7", "low"): -1, ("0.3", "at"): -1, ("0.3", "low"): 0}[key, side]
    for b in p.get("many", []):
        assert n_fg[b] > 128                                               # the foreground subsample runs
    if name == "small_map":
        assert anc.shape[0] < total // 4
    # the reference, at its own batch size and seed
    g = gold()
    assert "at_%s_error" % name not in g.files
    L, T, IW, OW = rpn.anchor_target_layer(*scene.feat, scene.gt, scene.im_info, np.random.RandomState(3))
    assert np.array_equal(L, g["at_%s_labels" % name]) and np.array_equal(IW > 0, g["at_%s_inw" % name])
    assert np.array_equal(IW, (IW > 0).astype(F32)) and np.array_equal(OW, g["at_%s_outw" % name])
    # the golden holds the reference's T[OW > 0] (the masks are equal: asserted above); channel 4a + j is component j of anchor a
    sel = OW > 0
    full = np.zeros_like(T)
    full[sel] = g["at_%s_targets_labelled" % name]
    dxdy = np.zeros(T.shape, bool)
    dxdy[:, [c for c in range(T.shape[1]) if c % 4 < 2]] = True
    assert np.array_equal(T[sel & dxdy], full[sel & dxdy])
    worst = tc.numpy_log_ulp()
    assert (tc.ulp_error(full[sel & ~dxdy], T[sel & ~dxdy].astype(np.float64)) <= 2 * max(worst, 0.5)).all()
    last = int((_inside_order(L, scene, inside)[B - 1] >= 0).sum())
    assert set(np.unique(OW)) <= {F32(0), F32(1.0 / last)}                  # the weight comes from the LAST image's count


# ----------------------------------------------------------------------------------------------------------- proposal scenes
PSCENES = [s.name for s in tc.proposal_scenes()]


def _pscene(name):
    return {s.name: s for s in tc.proposal_scenes()}[name]


@pytest.mark.parametrize("name", PSCENES)
def test_proposal_scene_regimes(name):
    """Exact classes = plain classes; every image lands in the branch its scene declares under both BG_THRESH_LO; the decision
    rois are on the side of each constant they are built for; padding rows belong to no class."""
    scene = _pscene(name)
    cand = tc.proposal_candidates(scene)
    P = scene.rois.shape[1]
    for lo, lo_fr in zip(tc.BG_LO, (Fr(0), Fr(1, 10))):
        for b in range(cand.shape[0]):
            fg, bg, am = tc.exact_proposal_classes(cand[b, :, 1:], scene.gt[b], lo_fr)
            pfg, pbg, pam = tc.plain_proposal_classes(cand[b, :, 1:], scene.gt[b], lo)
            assert np.array_equal(fg, pfg) and np.array_equal(bg, pbg) and np.array_equal(am, pam), (name, lo, b)
            regime = "both" if fg.any() and bg.any() else "fg" if fg.any() else "bg" if bg.any() else "none"
            assert regime == scene.prop["regime"][lo][b], (name, lo, b, regime)
            n_real, n_gt = scene.prop["n_real"][b], int((scene.gt[b, :, 2] > 0).sum())
            pad = np.r_[np.arange(n_real, P), np.arange(P + n_gt, cand.shape[1])]
            assert not fg[pad].any() and not bg[pad].any() and pad.size > 0                     # overlap -1: never a candidate
            assert (tc.exact_values(tc.exact_iu(cand[b, pad, 1:], scene.gt[b])) == -1).all()
            m = scene.prop["marks"][b]
            if "at_0.5" in m:
                g1 = scene.gt[b, 0]
                vals = {k: tc.iou_fraction(cand[b, r, 1:], g1) for k, r in m.items()}
                assert vals == {"at_0.5": Fr(1, 2), "below_0.5": Fr(49, 100), "at_0.1": Fr(1, 10), "below_0.1": Fr(9, 100), "at_0.0": Fr(0)}
                assert fg[m["at_0.5"]] and not bg[m["at_0.5"]] and bg[m["below_0.5"]] and not fg[m["below_0.5"]]
                assert bg[m["at_0.1"]] and bg[m["below_0.1"]] == (lo == 0.0) and bg[m["at_0.0"]] == (lo == 0.0)
                assert fg.sum() > 32                                                             # more than round(0.25 * 128)
            if "bg_row" in m:
                assert bg.sum() == 1 and bg[m["bg_row"]]
    if name == "thresholds_mix":
        fg, _, am = tc.exact_proposal_classes(cand[1, :, 1:], scene.gt[1], Fr(0))
        assert fg.sum() == 3 < 8                                                                 # fewer than round(0.25 * 32)
        fg, _, am = tc.exact_proposal_classes(cand[2, :, 1:], scene.gt[2], Fr(0))
        assert np.array_equal(scene.gt[2, 0, :4], scene.gt[2, 1, :4]) and scene.gt[2, 0, 4] != scene.gt[2, 1, 4]
        assert (am[fg] != 1).all() and (am[fg] == 0).sum() >= 10                                 # the duplicate is never assigned


@pytest.mark.parametrize("R", tc.PROPOSAL_R)
@pytest.mark.parametrize("lo", tc.BG_LO)
@pytest.mark.parametrize("name", PSCENES)
def test_proposal_oracle_against_plain_and_reference(name, lo, R):
    """The oracle with the reference's seed: equal to the plain float64 statement (rois, labels, weights; targets to the
    bbox_transform bounds) and to the reference's five outputs.  Scenes with an image of neither class ("neither" under both
    BG_THRESH_LO, "no_gt" under 0.1: without ground truth every overlap is 0, which 0.1 excludes) make the reference raise
    ValueError by design; its text is in the golden and those scenes are pinned against the oracle and the plain statement
    alone: both raise ValueError too."""
    scene, g = _pscene(name), gold()
    key = "pt_%s_lo%02d_R%d" % (name, int(lo * 10), R)
    if tc.raises(scene, lo):
        assert str(g[key + "_error"]).startswith("ValueError") and key + "_rois" not in g.files
        with pytest.raises(ValueError):
            rpn.proposal_target_layer(scene.rois, scene.gt, np.random.RandomState(3), batch_size=R, bg_lo=lo)
        with pytest.raises(ValueError):
            tc.plain_proposal_target(scene.rois, scene.gt, np.random.RandomState(3), R, lo)
        return
    assert key + "_error" not in g.files
    rois, labels, targets, inw, outw = rpn.proposal_target_layer(scene.rois, scene.gt, np.random.RandomState(3), batch_size=R, bg_lo=lo)
    p_rois, p_lab, p_tg, p_inw, p_outw, keep, nfg = tc.plain_proposal_target(scene.rois, scene.gt, np.random.RandomState(3), R, lo)
    assert np.array_equal(rois, p_rois) and np.array_equal(labels, p_lab) and np.array_equal(inw, p_inw) and np.array_equal(outw, p_outw)
    cand = tc.proposal_candidates(scene)
    worst = tc.numpy_log_ulp()
    stds = np.asarray((0.1, 0.1, 0.2, 0.2), F32).astype(np.float64)
    for b in range(rois.shape[0]):
        fg = labels[b] > 0
        assert (targets[b][~fg] == 0).all()
        bound = tc.dxdy_bound(rois[b, :, 1:], p_rois[b, :, 1:] * 0 + _assigned_gt(scene, cand, keep, b)) / stds[:2] * 2
        assert (np.abs(targets[b, fg, :2] - p_tg[b, fg, :2]) <= bound[fg]).all()
        if fg.any():
            assert float(tc.ulp_error(targets[b, fg, 2:], _log_norm(scene, cand, keep, b)[fg]).max()) <= tc.normalised_bound(worst)
        regime = scene.prop["regime"][lo][b]
        fg_per = int(round(0.25 * R))
        n_fg_all = int(tc.plain_proposal_classes(cand[b, :, 1:], scene.gt[b], lo)[0].sum())
        assert nfg[b] == {"both": min(fg_per, n_fg_all), "fg": R, "bg": 0}[regime]
        if "bg_row" in scene.prop["marks"][b]:
            assert (keep[b, nfg[b]:] == scene.prop["marks"][b]["bg_row"]).all() and R - nfg[b] > 1    # one candidate, repeated
    for nm, got in zip(("rois", "labels", "inw", "outw"), (rois, labels, inw, outw)):
        assert np.array_equal(got, g["%s_%s" % (key, nm)]), nm
    ref = g[key + "_targets"]
    assert np.array_equal(targets[..., :2], ref[..., :2])
    live = labels > 0
    assert (ref[~live] == 0).all()
    if live.any():
        assert (tc.ulp_error(ref[live][:, 2:], targets[live][:, 2:].astype(np.float64)) <= 2 * tc.normalised_bound(max(worst, 0.5))).all()


def _assigned_gt(scene, cand, keep, b):
    am = tc.plain_overlaps(cand[b, :, 1:], scene.gt[b])[2]
    return scene.gt[b, am[keep[b]], :4]


def _log_norm(scene, cand, keep, b):
    stds = np.asarray((0.2, 0.2), F32).astype(np.float64)
    return tc.plain_log_targets(cand[b, keep[b], 1:], _assigned_gt(scene, cand, keep, b)) / stds


# ----------------------------------------------------------------------------------------------------------- teeth
def _overlap_tells(variant):
    for case in tc.edge_overlap_cases() + [tc.shape_case(3, 257, 30, "b5")]:
        for boxes, gt in tc.case_images(case):
            a, b = tc.plain_overlaps(boxes, gt), tc.plain_overlaps(boxes, gt, variant)
            if not all(np.array_equal(x, y) for x, y in zip(a, b)):
                return case.name
    return None


def _anchor_tells(variant):
    for scene in tc.anchor_scenes():
        anc, _, _ = tc.scene_anchors(scene)
        for b in range(scene.gt.shape[0]):
            if not np.array_equal(tc.plain_anchor_labels(anc, scene.gt[b])[0], tc.plain_anchor_labels(anc, scene.gt[b], variant)[0]):
                return scene.name
    return None


def _proposal_tells(variant):
    for scene in tc.proposal_scenes():
        cand = tc.proposal_candidates(scene)
        for lo in tc.BG_LO:
            for b in range(cand.shape[0]):
                a = tc.plain_proposal_classes(cand[b, :, 1:], scene.gt[b], lo)
                w = tc.plain_proposal_classes(cand[b, :, 1:], scene.gt[b], lo, variant)
                lab_a, lab_w = scene.gt[b, a[2], 4], scene.gt[b, w[2], 4]
                if not (np.array_equal(a[0], w[0]) and np.array_equal(a[1], w[1]) and np.array_equal(lab_a[a[0]], lab_w[a[0]])):
                    return scene.name
    return None


def test_every_wrong_variant_is_told_apart():
    """The comparisons of the GPU test are with the oracle, which equals the plain rules on every case (above); so a kernel or
    layer that computed one of these wrong forms would differ from the oracle wherever the wrong form differs from the plain
    rules.  Which cases do: ``>`` for ``>=`` -- the anchor on exactly 0.7 and the rois on exactly 0.5 / 0.1 / 0.0; last-index
    argmax -- duplicate ground truth (overlap kernel and the proposal labels); the fills in the other order -- the unit roi on
    the unit ground truth; a fused multiply-subtract -- the fractional boxes (and only them: integer boxes are exact either
    way)."""
    assert tc.VARIANTS == ("strict_ge", "last_argmax", "fill_swapped", "fused")
    assert _anchor_tells("strict_ge") == "thresholds" and _proposal_tells("strict_ge") == "thresholds_mix"
    assert _overlap_tells("last_argmax") is not None and _proposal_tells("last_argmax") == "thresholds_mix"
    assert tc.plain_overlaps(tc.tie_case().boxes, tc.tie_case().gt[0], "last_argmax")[2].tolist() == [1, 3, 3]
    assert _overlap_tells("fill_swapped") == "zero_area"
    z = tc.zero_area_case()
    assert tc.plain_overlaps(z.boxes, z.gt[0], "fill_swapped")[0][2, 2] == 0 and tc.plain_overlaps(z.boxes, z.gt[0])[0][2, 2] == -1
    assert _overlap_tells("fused") == "fractional"
    f = tc.fractional_case()
    diff = tc.plain_overlaps(f.boxes, f.gt[0], "fused")[0] != tc.plain_overlaps(f.boxes, f.gt[0])[0]
    assert 0 < diff.sum()
    for case in (tc.threshold_case(), tc.tie_case(), tc.zero_area_case()):                       # integer boxes: fusing changes nothing
        assert np.array_equal(tc.plain_overlaps(case.boxes, case.gt[0], "fused")[0], tc.plain_overlaps(case.boxes, case.gt[0])[0])
