"""The rel_det targets on the host (i2vsgg_amd/relation_targets.py): the numpy form against a plain triple-loop restatement of
the reference's branch, bit for bit; against the annotated-box task's own tables; the distribution of the draws against exact
successive-sampling probabilities; and what ``pack`` and the training script refuse."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relation_target_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    from i2vsgg_amd import relation_targets
    return relation_targets


def test_host_form_equals_the_restatement_on_every_case(rt):
    assert (rt.P, rt.B, rt.DRAWS, rt.CAP) == (cases.P, cases.B, cases.DRAWS, cases.CAP)
    cand, ndet, frames, dropped, merged = set(), set(), set(), 0, 0
    for name, t, n_rel in cases.all_cases():
        stats = {}
        want = cases.restatement(*t, n_rel=n_rel, stats=stats)
        cases.same(rt.relation_targets_host(*t, n_rel=n_rel), want, name)
        cand |= set(stats["candidates"])
        ndet |= set(np.diff(t[0]).tolist())
        frames.add(len(t[9]))
        dropped += int(want["n_dropped"].sum())
        merged += int((want["labels"].sum(1) > 1).sum())
        draws = int((want["samp"][:, :, 0] >= 0).sum())
        assert draws >= int(want["n_pairs"].sum()) + int(want["n_dropped"].sum())
    # the case set covers what it claims
    assert {0, 1, 9, 10, 11, 64 * 63} <= cand and {0, 1, 63, 64} <= ndet and {1, 3} <= frames and dropped > 0 and merged > 0


def test_named_cases_are_what_their_names_say(rt):
    by = {name: t for name, t, _ in cases.all_cases()}
    run = lambda name: rt.relation_targets_host(*by[name], n_rel=cases.N_REL)
    o = run("no_relation_no_match_self_only")
    assert o["n_pairs"][:3].tolist() == [0, 0, 0] and o["n_pairs"][3] > 0 and not o["w"][:3 * cases.P].any()
    assert (o["samp"][by["no_relation_no_match_self_only"][6][2]] == -1).all()       # the a == b candidate is none
    o = run("iou_exactly_half")                           # 0.5 is accepted: both relations have their one candidate
    assert o["samp"][:, 0].tolist() == [[0, 1], [1, 0]] and o["n_pairs"][0] == 2
    assert o["labels"][0].tolist() == [0, 0, 0, 0, 1, 0, 0] and o["labels"][1].tolist() == [1, 0, 0, 0, 0, 0, 0]
    o = run("same_pair_two_predicates")                   # two relations on one box pair: one row, two labels
    assert o["n_pairs"].tolist() == [1, 8] and o["labels"][0].tolist() == [0, 0, 1, 0, 0, 1, 0]
    assert sorted(set(o["labels"][cases.P:cases.P + 4].sum(1).tolist())) == [2.0]   # (0,1,1) and (0,1,6) reach the same four pairs; (1,0,1) four more
    o = run("two_relations_reach_one_pair")
    n = int(o["n_pairs"][0])
    assert n == 12 and (o["labels"][:n, 0] * o["labels"][:n, 3]).sum() == 6         # relations 0 and 1 share their 3 x 2 pairs
    o = run("more_than_64_pairs")
    assert o["n_pairs"][0] == 64 and o["n_dropped"][0] > 0 and o["w"][63] == np.float32(1.0 / 128)
    # u = 0 draws the first alive candidate every time, u = 2^32 - 1 the last
    t = by["candidates_1_9_10_11_4032_u_zero"]
    o = run("candidates_1_9_10_11_4032_u_zero")
    r = int(t[6][4])                                      # the relation with 64 x 63 candidates
    assert o["samp"][r].tolist() == [[0, b] for b in range(1, 11)]
    o = run("candidates_1_9_10_11_4032_u_max")
    assert o["samp"][r].tolist() == [[63, b] for b in range(62, 52, -1)]


def test_cap_keeps_the_64_best_in_row_order(rt):
    dets, annos, info, u = cases.capped_case()
    pk = rt.pack(dets, annos, info, cases.N_REL, u=u)
    assert pk.det_off.tolist() == [0, 64] and len(pk.kept[0]) == 64
    worst = int(np.argmin(dets[0]["scores"]))
    assert sorted(set(range(65)) - set(pk.kept[0].tolist())) == [worst] and (np.diff(pk.kept[0]) > 0).all()
    assert pk.boxes5.shape == (64, 5) and np.array_equal(pk.boxes5[:, 1:], pk.det_box.astype(np.float32))
    cases.same(rt.relation_targets(pk, cases.N_REL), cases.restatement(*pk.tables(), n_rel=cases.N_REL), "capped")


def test_pack_filters_clips_and_scales_like_the_reference(rt):
    # :465-474 on a 100 x 200 image at scale 1.5: boxes outside are dropped, the rest clipped to [0, w] x [0, h], then scaled
    boxes = [[-5, -5, 50, 40], [200, 10, 220, 30], [10, 100, 30, 120], [-9, 3, 0, 20], [150, 60, 260, 130], [20, 20, 60, 60]]
    dets = [{"boxes": boxes, "box_classes": [1, 2, 3, 4, 5, 6], "scores": [0.9] * 6}]
    annos = [{"boxes": [[0, 0, 10, 10]], "box_classes": [1], "rels": []}]
    pk = rt.pack(dets, annos, np.array([[150.0, 300.0, 1.5]]), cases.N_REL)
    assert pk.kept[0].tolist() == [0, 4, 5] and pk.det_cls.tolist() == [1, 5, 6]
    assert pk.det_box.tolist() == [[0, 0, 75, 60], [225, 90, 300, 150], [30, 30, 90, 90]] and pk.gt_box.tolist() == [[0, 0, 15, 15]]
    assert pk.u.shape == (0, 10) and pk.u.dtype == np.uint32


def test_uniforms_come_from_the_global_stream(rt):
    fr = cases.random_frame(1, 20, 6, 12)
    dets = [{"boxes": fr["det"].tolist(), "box_classes": fr["det_cls"].tolist(), "scores": [0.9] * 20}]
    annos = [{"boxes": fr["gt"].tolist(), "box_classes": fr["gt_cls"].tolist(), "rels": fr["rels"].tolist()}]
    np.random.seed(3)
    a = rt.pack(dets, annos, [[200.0, 320.0, 1.0]], cases.N_REL).u
    np.random.seed(3)
    want = np.random.randint(0, 2 ** 32, size=(12, 10), dtype=np.uint32)
    assert a.dtype == np.uint32 and np.array_equal(a, want)


def test_detections_equal_to_the_annotated_boxes_give_the_annotated_box_tables(rt):
    """Every annotated box is its own detection (overlap 1 with itself; any other box of its class overlaps it by < 0.5): each
    relation has one candidate, so the rows are ``build_pair_tables``' own, in its order, bit for bit."""
    from i2vsgg_amd import synthetic as syn
    from i2vsgg_amd.model.faster_rcnn.faster_rcnn_SGG_emb import build_pair_tables
    checked = 0
    for seed, sc, (h, w) in ((40, 1.0, (200, 320)), (41, 1.0, (200, 320)), (7, 1.7, (300, 500))):
        anno = syn.relation_annotation(seed, 6, 5, cases.N_REL, 16, h, w)
        dets = syn.detections_for(seed, anno, exact=True)
        ih, iw = float(np.float32(h * sc)), float(np.float32(w * sc))
        pk = rt.pack([dets], [anno], [[ih, iw, sc]], cases.N_REL)
        got = rt.relation_targets(pk, cases.N_REL)
        gt, union, bnd, lab, ixs, ixo = build_pair_tables(anno, sc, ih, iw, cases.N_REL)
        n = len(ixs)
        assert got["n_pairs"][0] == n and got["n_dropped"][0] == 0 and n >= 5
        assert np.array_equal(pk.det_box, gt) and np.array_equal(got["ixs"][:n], ixs) and np.array_equal(got["ixo"][:n], ixo)
        assert np.array_equal(got["rel5"][:n, 1:].view(np.uint32), union.astype(np.float32).view(np.uint32))
        assert np.array_equal(got["bounds"][:n], bnd) and np.array_equal(got["labels"][:n], lab)
        assert (got["w"][:n] == np.float32(1.0 / n)).all() and not got["w"][n:].any()
        checked += n
    assert checked >= 15


def _exact_probabilities(weights, K):
    """Inclusion and first-pick probability of every candidate under successive sampling, by enumeration."""
    n, tot = len(weights), float(sum(weights))
    incl = np.zeros(n)
    for seq in itertools.permutations(range(n), K):
        p, rest = 1.0, tot
        for c in seq:
            p *= weights[c] / rest
            rest -= weights[c]
        incl[list(seq)] += p
    return incl, np.asarray(weights, np.float64) / tot


def test_draws_follow_successive_sampling(rt):
    """Nine candidates from overlaps [0.5, 0.62, 0.71] x [0.83, 0.97, 0.55], K = 3, 40 000 draws of u from default_rng(7): every
    candidate's inclusion and first-pick frequency lies within 5 standard deviations sqrt(p (1 - p) / N) of the exact
    probability (tried with this input: the largest deviations were 1.3 and 1.4 sigma)."""
    ia, ib = [0.5, 0.62, 0.71], [0.83, 0.97, 0.55]
    weights = [x * y for x in ia for y in ib]
    incl_p, first_p = _exact_probabilities(weights, 3)
    assert abs(incl_p.sum() - 3.0) < 1e-12
    # detections whose overlaps with their annotated box are exactly the wanted values cannot be built from boxes in general:
    # the rule's arithmetic from the weights on is what is tested, through the same host function the tables go through
    N = 40000
    u = np.random.default_rng(7).integers(0, 2 ** 32, size=(N, 10), dtype=np.uint32)
    wt = np.floor(np.asarray(weights) * 65536.0).astype(np.int64)
    incl, first = np.zeros(9), np.zeros(9)
    for i in range(N):
        picks = rt.draw(wt, u[i], 3)
        incl[picks] += 1
        first[picks[0]] += 1
    for got, p in ((incl / N, incl_p), (first / N, first_p)):
        sigma = np.sqrt(p * (1 - p) / N)
        dev = np.abs(got - p) / sigma
        print("largest deviation %.2f sigma" % dev.max())
        assert (dev < 5.0).all(), dev


def test_pack_refuses_malformed_input_and_names_the_frame(rt):
    good_d = {"boxes": [[0, 0, 10, 10], [20, 20, 40, 40]], "box_classes": [1, 2], "scores": [0.9, 0.8]}
    good_a = {"boxes": [[0, 0, 10, 10], [20, 20, 40, 40]], "box_classes": [1, 2], "rels": [[0, 1, 3]]}
    info = [[100.0, 100.0, 1.0], [100.0, 100.0, 1.0]]
    rt.pack([good_d, good_d], [good_a, good_a], info, cases.N_REL)

    def refused(d=None, a=None, info=info, match="frame 1"):
        with pytest.raises(ValueError, match=match):
            rt.pack([good_d, dict(good_d, **(d or {}))], [good_a, dict(good_a, **(a or {}))], info, cases.N_REL, names=["x.jpg", "y.jpg"])

    refused(d={"scores": [0.9]})
    refused(d={"box_classes": [1]})
    refused(d={"boxes": [[0, 0, 10, 10], [20, 20, 40, float("nan")]]})
    refused(d={"boxes": [[0, 0, 10], [1, 2, 3]]})
    refused(a={"rels": [[0, 2, 3]]}, match=r"frame 1 \(y.jpg\).*outside its 2 annotated boxes")
    refused(a={"rels": [[0, 1, cases.N_REL]]}, match="frame 1.*predicate")
    refused(a={"box_classes": [1]})
    refused(info=[[100.0, 100.0, 1.0], [0.0, 100.0, 1.0]])
    with pytest.raises(ValueError, match="frames"):
        rt.pack([good_d], [good_a, good_a], info, cases.N_REL)
    with pytest.raises(ValueError, match="u is"):
        rt.pack([good_d], [good_a], info[:1], cases.N_REL, u=np.zeros((2, 10), np.uint32))


def test_host_form_reports_malformed_tables_like_the_kernel(rt):
    for name, t, bad in cases.malformed_cases():
        cases.check_malformed(rt.relation_targets_host(*t, n_rel=cases.N_REL), t, bad)


def test_synthetic_detections_are_seeded_and_controlled(rt):
    from i2vsgg_amd import synthetic as syn
    anno = syn.relation_annotation(5, 8, 6, cases.N_REL, 16, 200, 320)
    d1, d2 = syn.detections_for(9, anno, im_h=200, im_w=320), syn.detections_for(9, anno, im_h=200, im_w=320)
    assert d1 == d2 and set(d1) == {"boxes", "box_classes", "scores"} and len(d1["boxes"]) > 8
    pk = rt.pack([d1], [anno], [[200.0, 320.0, 1.0]], cases.N_REL)
    got = rt.relation_targets(pk, cases.N_REL)
    assert got["n_pairs"][0] >= 6                          # every annotated pair has a detected one at the default jitter


def test_cli_without_detections_exits_naming_the_flag():
    sys.path.insert(0, ROOT)
    import trainval_sgg_emb as cli
    with pytest.raises(SystemExit) as e:
        cli.check_task_args(cli.parse_args(["--vrd_task", "rel_det"]))
    assert "--source_det_boxes_path" in str(e.value)
    cli.check_task_args(cli.parse_args(["--vrd_task", "pre_det"]))
    with pytest.raises(SystemExit) as e:
        cli.check_task_args(cli.parse_args(["--vrd_task", "other"]))
    assert "vrd_task" in str(e.value)
