"""Inputs for the track-stitching tests (no tests here): the hand-worked cases with their expected results, a second, naive
statement of the rules of ``seqnms.stitch_arrays_host`` in plain Python floats over explicit tracklet lists, and the seeded
end-to-end scenario (objects that are missed for a few frames now and then)."""
import numpy as np

import seqnms_cases as cases


# ---------------------------------------------------------------------------------------------------------------------
# the rules again: explicit tracklets, the visiting loop in plain Python
# ---------------------------------------------------------------------------------------------------------------------
def naive_stitch(frame_no, slots, max_gap=3, stitch_iou=0.3, rescore="avg"):
    """One group.  ``slots[t]``: the slot's rows as (box [x1, y1, x2, y2], np.float32 score, tid).  Returns (tid2 per slot,
    score2 per slot (np.float32), number of chains, new rows [(slot, tid, np.float32 box (4), np.float32 score)])."""
    members = {}                                         # tid -> [(slot, row)] in frame order
    for t, rows in enumerate(slots):
        for a, (_, _, k) in enumerate(rows):
            if k >= 0:
                members.setdefault(k, []).append((t, a))
    for m in members.values():                           # a Seq-NMS track: consecutive slots with consecutive numbers
        assert all(t1 == t0 + 1 and frame_no[t1] == frame_no[t0] + 1 for (t0, _), (t1, _) in zip(m[:-1], m[1:]))
    succ, pred, links = {}, {}, []
    for b in sorted(members, key=lambda k: (frame_no[members[k][0][0]], k)):
        tb, ab = members[b][0]
        best = None
        for a in sorted(members):
            ta, aa = members[a][-1]
            gap = frame_no[tb] - frame_no[ta] - 1
            if a in succ or not 1 <= gap <= max_gap:
                continue
            ov = cases.overlap(slots[ta][aa][0], slots[tb][ab][0])
            if ov >= stitch_iou and (best is None or (-ov, gap, a) < best[0]):
                best = ((-ov, gap, a), a)
        if best is not None:
            succ[best[1]], pred[b] = b, best[1]
            links.append((best[1], b))
    roots = sorted(k for k in members if k not in pred)
    tid2 = [[-1] * len(rows) for rows in slots]
    score2 = [[np.float32(s) for _, s, _ in rows] for rows in slots]
    chain_of, chain_score = {}, {}
    for new, r in enumerate(roots):
        chain, k = [], r
        while k is not None:
            chain += members[k]
            chain_of[k] = new
            k = succ.get(k)
        if rescore == "max":
            ns = max(np.float32(slots[t][a][1]) for t, a in chain)
        else:
            s = 0.0
            for t, a in chain:
                s += float(slots[t][a][1])
            ns = np.float32(s / len(chain))
        chain_score[new] = ns
        for t, a in chain:
            tid2[t][a], score2[t][a] = new, ns
    fills = []
    for a, b in links:
        (ta, aa), (tb, ab) = members[a][-1], members[b][0]
        pa, pb = [float(x) for x in slots[ta][aa][0]], [float(x) for x in slots[tb][ab][0]]
        e, s = frame_no[ta], frame_no[tb]
        for t in range(ta + 1, tb):
            w = float(frame_no[t] - e) / float(s - e)
            fills.append((t, chain_of[b], np.array([pa[c] + (pb[c] - pa[c]) * w for c in range(4)], np.float32), chain_score[chain_of[b]]))
    return tid2, score2, len(roots), fills


def group_slots(pk, tid, g):
    """Group g of packed tables as ``naive_stitch`` takes it: (frame numbers, slots)."""
    f0, f1 = int(pk.group_off[g]), int(pk.group_off[g + 1])
    slots = [[(pk.box[n].tolist(), pk.score[n], int(tid[n])) for n in range(int(pk.box_off[f]), int(pk.box_off[f + 1]))]
             for f in range(f0, f1)]
    return [int(x) for x in pk.frame_no[f0:f1]], slots


def check_against_naive(pk, tid, res, **kw):
    """Every group of ``res`` (the eight arrays of ``stitch_arrays``) against ``naive_stitch``, bit for bit.  Returns the number
    of new rows compared."""
    tid2, score2, n_tracks2, fill_off, fill_slot, fill_tid, fill_box, fill_score = res
    for g in range(len(pk.group_off) - 1):
        frame_no, slots = group_slots(pk, tid, g)
        wt, ws, wk, wf = naive_stitch(frame_no, slots, **kw)
        f0 = int(pk.group_off[g])
        for t in range(len(slots)):
            p, q = int(pk.box_off[f0 + t]), int(pk.box_off[f0 + t + 1])
            assert tid2[p:q].tolist() == wt[t], (g, t)
            assert score2[p:q].view(np.uint32).tolist() == [int(np.float32(x).view(np.uint32)) for x in ws[t]], (g, t)
        assert int(n_tracks2[g]) == wk, g
        r0, r1 = int(fill_off[g]), int(fill_off[g + 1])
        assert r1 - r0 == len(wf), (g, r1 - r0, len(wf))
        for r, (t, k, box, s) in zip(range(r0, r1), wf):
            assert int(fill_slot[r]) == f0 + t and int(fill_tid[r]) == k, (g, r)
            assert np.array_equal(fill_box[r].view(np.uint32), box.view(np.uint32)), (g, r, fill_box[r], box)
            assert fill_score[r].view(np.uint32) == np.float32(s).view(np.uint32), (g, r)
    return int(fill_off[-1])


def same_bits(got, want):
    """Two results of ``stitch_arrays``: every array equal, float32 compared as bits."""
    assert len(got) == len(want) == 8
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases: one video, one class, the boxes of seqnms_cases ([x, y, x + 20, y + 20]; a shift of 5 overlaps 0.615, of
# 7 exactly 294 / 588 = 0.5, of 8 273 / 609 = 0.448, of 10 231 / 651 = 0.355, of 13 168 / 714 = 0.235, of 16 105 / 777 =
# 0.135).  Scores are dyadic and every interpolation weight is k / 2 or k / 4, so sums, means and new boxes are exact.
# "nms": Seq-NMS's arguments, "stitch": the stitching step's (max_gap = 3, stitch_iou = 0.3 unless given).  "seq": the ids
# Seq-NMS gives (worked out in the comment), "tid" / "score" / "n_tracks" / "fills": what the stitching step gives;
# fills are (slot, tid, box, score) in emission order.
# ---------------------------------------------------------------------------------------------------------------------
_b = cases._b
_X = lambda s: [10, 10, 30, 30, s]

HAND = {
    # one miss: Seq-NMS numbers the later box 0 (0.75) and the earlier 1; gap 1, overlap 0.448: joined, root is the earlier
    # box, one chain; the empty slot 1 gets the midpoint; (0.5 + 0.75) / 2
    "bridge": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.5)], [], [_b(8, 0, 0.75)]], seq=[[1], [], [0]],
                   tid=[[0], [], [0]], score=[[0.625], [], [0.625]], n_tracks=1, fills=[(1, 0, [4, 0, 24, 20], 0.625)],
                   stats=dict(links=1, chains_of_three=0, claimed_met=0, multi=0, links_over_absent_numbers=0, ties=0)),
    "bridge_max": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.5)], [], [_b(8, 0, 0.75)]], seq=[[1], [], [0]],
                       nms=dict(rescore="max"), stitch=dict(rescore="max"),
                       tid=[[0], [], [0]], score=[[0.75], [], [0.75]], n_tracks=1, fills=[(1, 0, [4, 0, 24, 20], 0.75)]),
    # three missing numbers at max_gap = 3: joined, weights 1/4, 2/4, 3/4
    "gap_equal": dict(frame_no=[0, 1, 2, 3, 4], cells=[[_b(0, 0, 0.5)], [], [], [], [_b(8, 0, 0.75)]], seq=[[1], [], [], [], [0]],
                      tid=[[0], [], [], [], [0]], score=[[0.625], [], [], [], [0.625]], n_tracks=1,
                      fills=[(1, 0, [2, 0, 22, 20], 0.625), (2, 0, [4, 0, 24, 20], 0.625), (3, 0, [6, 0, 26, 20], 0.625)]),
    # four missing numbers: not joined, everything is Seq-NMS's
    "gap_over": dict(frame_no=[0, 1, 2, 3, 4, 5], cells=[[_b(0, 0, 0.5)], [], [], [], [], [_b(8, 0, 0.75)]],
                     seq=[[1], [], [], [], [], [0]], tid=[[1], [], [], [], [], [0]], score=[[0.5], [], [], [], [], [0.75]],
                     n_tracks=2, fills=[]),
    # consecutive frames, overlap 0.355: below link_iou, so two tracks; above stitch_iou, but adjacent tracklets are never joined
    "adjacent": dict(frame_no=[0, 1], cells=[[_b(0, 0, 0.5)], [_b(10, 0, 0.75)]], seq=[[1], [0]],
                     tid=[[1], [0]], score=[[0.5], [0.75]], n_tracks=2, fills=[]),
    # overlap 294 / 588 == 0.5 == stitch_iou: joined (>=); the next double above 0.5: not joined
    "iou_equal": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.5)], [], [_b(7, 0, 0.75)]], seq=[[1], [], [0]], stitch=dict(stitch_iou=0.5),
                      tid=[[0], [], [0]], score=[[0.625], [], [0.625]], n_tracks=1, fills=[(1, 0, [3.5, 0, 23.5, 20], 0.625)]),
    "iou_above": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.5)], [], [_b(7, 0, 0.75)]], seq=[[1], [], [0]],
                      stitch=dict(stitch_iou=float(np.nextafter(0.5, 1.0))),
                      tid=[[1], [], [0]], score=[[0.5], [], [0.75]], n_tracks=2, fills=[]),
    # A (0.25: id 2) is wanted by B1 (0.75: id 0; overlap 0.448) and B2 (0.625: id 1; overlap 0.615) of frame 2, which do not
    # suppress each other (0.235).  B1 is visited first and takes A although B2 overlaps more; B2 meets a claimed candidate.
    # Roots: B2 (1) -> 0, A (2) -> 1.  (0.25 + 0.75) / 2
    "two_successors": dict(frame_no=[0, 1, 2], cells=[[_b(20, 0, 0.25)], [], [_b(28, 0, 0.75), _b(15, 0, 0.625)]],
                           seq=[[2], [], [0, 1]], tid=[[1], [], [1, 0]], score=[[0.5], [], [0.5, 0.625]], n_tracks=2,
                           fills=[(1, 1, [24, 0, 44, 20], 0.5)],
                           stats=dict(links=1, chains_of_three=0, claimed_met=1, multi=0, links_over_absent_numbers=0, ties=0)),
    # B (0.875: id 0) has two free predecessors: A1 (0.25: id 2; overlap 0.615) and A2 (0.5: id 1; overlap 0.448): the larger
    # overlap wins over the lower id.  Roots: A2 (1) -> 0, A1 (2) -> 1.  (0.25 + 0.875) / 2
    "larger_overlap": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.25), _b(13, 0, 0.5)], [], [_b(5, 0, 0.875)]],
                           seq=[[2, 1], [], [0]], tid=[[1, 0], [], [1]], score=[[0.5625, 0.5], [], [0.5625]], n_tracks=2,
                           fills=[(1, 1, [2.5, 0, 22.5, 20], 0.5625)],
                           stats=dict(links=1, chains_of_three=0, claimed_met=0, multi=1, links_over_absent_numbers=0, ties=0)),
    # link_iou = 2 links nothing: three one-box tracks P (0.75: id 0, frame 1), Q (0.5: id 1, frame 2), B (0.25: id 2, frame 4),
    # identical boxes.  P and Q are adjacent: not joined.  B sees both at overlap 1: the smaller gap (Q, the higher id) wins.
    "smaller_gap": dict(frame_no=[1, 2, 3, 4], cells=[[_X(0.75)], [_X(0.5)], [], [_X(0.25)]], nms=dict(link_iou=2.0),
                        seq=[[0], [1], [], [2]], tid=[[0], [1], [], [1]], score=[[0.75], [0.375], [], [0.375]], n_tracks=2,
                        fills=[(2, 1, [10, 10, 30, 30], 0.375)],
                        stats=dict(links=1, chains_of_three=0, claimed_met=0, multi=1, links_over_absent_numbers=0, ties=1)),
    # nms_iou = 1 keeps twins: row 1 (0.75) is id 0, row 0 (0.5) id 1, the box of frame 2 (0.5, the later frame) id 2.  Equal
    # overlap, equal gap: the lower id -- the higher row -- wins.  (0.75 + 0.5) / 2
    "lower_tid": dict(frame_no=[0, 1, 2], cells=[[_X(0.5), _X(0.75)], [], [_X(0.5)]], nms=dict(nms_iou=1.0),
                      seq=[[1, 0], [], [2]], tid=[[1, 0], [], [0]], score=[[0.5, 0.625], [], [0.625]], n_tracks=2,
                      fills=[(1, 0, [10, 10, 30, 30], 0.625)],
                      stats=dict(links=1, chains_of_three=0, claimed_met=0, multi=1, links_over_absent_numbers=0, ties=1)),
    # Y (0.875, every frame) is track 0.  X is seen in frames 0, 2, 4 (0.5, 0.75, 0.25: ids 2, 1, 3) 8 pixels further each
    # time: a chain of three with root id 2 -> new id 1, ids 0..1 dense.  X at frame 4 also reaches back to frame 0 (gap 3)
    # but overlaps it by 0.135 only.  1.5 / 3; the new rows land in cells that hold Y.
    "chain3": dict(frame_no=[0, 1, 2, 3, 4],
                   cells=[[_b(0, 0, 0.5), _b(0, 100, 0.875)], [_b(0, 100, 0.875)], [_b(8, 0, 0.75), _b(0, 100, 0.875)],
                          [_b(0, 100, 0.875)], [_b(16, 0, 0.25), _b(0, 100, 0.875)]],
                   seq=[[2, 0], [0], [1, 0], [0], [3, 0]], tid=[[1, 0], [0], [1, 0], [0], [1, 0]],
                   score=[[0.5, 0.875], [0.875], [0.5, 0.875], [0.875], [0.5, 0.875]], n_tracks=2,
                   fills=[(1, 1, [4, 0, 24, 20], 0.5), (3, 1, [12, 0, 32, 20], 0.5)],
                   stats=dict(links=2, chains_of_three=1, claimed_met=0, multi=0, links_over_absent_numbers=0, ties=0)),
    # frame numbers 0 1 2 | 5 6: two missing numbers, no slot between them: joined, zero rows.  3.25 / 5
    "absent_numbers": dict(frame_no=[0, 1, 2, 5, 6], cells=[[_b(0, 0, 0.75)]] * 3 + [[_b(0, 0, 0.5)]] * 2, seq=[[0]] * 3 + [[1]] * 2,
                           tid=[[0]] * 5, score=[[np.float32(3.25 / 5.0)]] * 5, n_tracks=1, fills=[],
                           stats=dict(links=1, chains_of_three=0, claimed_met=0, multi=0, links_over_absent_numbers=1, ties=0)),
}


def hand_nested(name):
    case = HAND[name]
    return cases.nested([("v", case["frame_no"], {1: case["cells"]})], 2)


def check_hand(name, seq_tid, res, pk):
    """``seq_tid``: Seq-NMS's ids, ``res``: the eight arrays of the stitching step, on ``pack(hand_nested(name))`` (group 0 is
    the background: empty; group 1 the case)."""
    case = HAND[name]
    tid2, score2, n_tracks2, fill_off, fill_slot, fill_tid, fill_box, fill_score = res
    f0 = int(pk.group_off[1])
    for t in range(len(case["cells"])):
        p, q = int(pk.box_off[f0 + t]), int(pk.box_off[f0 + t + 1])
        assert seq_tid[p:q].tolist() == case["seq"][t], (name, "seq", t, seq_tid[p:q].tolist())
        assert tid2[p:q].tolist() == case["tid"][t], (name, "tid", t, tid2[p:q].tolist())
        assert score2[p:q].view(np.uint32).tolist() == [int(np.float32(x).view(np.uint32)) for x in case["score"][t]], (name, t, score2[p:q])
    assert n_tracks2.tolist() == [0, case["n_tracks"]], (name, n_tracks2)
    assert fill_off.tolist() == [0, 0, len(case["fills"])], (name, fill_off)
    for r, (t, k, box, s) in enumerate(case["fills"]):
        assert int(fill_slot[r]) == f0 + t and int(fill_tid[r]) == k, (name, r, fill_slot[r], fill_tid[r])
        assert np.array_equal(fill_box[r].view(np.uint32), np.asarray(box, np.float32).view(np.uint32)), (name, r, fill_box[r])
        assert fill_score[r].view(np.uint32) == np.float32(s).view(np.uint32), (name, r, fill_score[r])


# ---------------------------------------------------------------------------------------------------------------------
# the end-to-end scenario: four objects over 48 frames, each missed for runs of 1-3 frames every 5-8 frames
# ---------------------------------------------------------------------------------------------------------------------
def scenario(seed, n_frames=48, n_obj=4):
    """(all_boxes, frame_index, groundtruth): one video "v", one class.  The ground truth is the true box in every frame."""
    rng = np.random.default_rng(seed)
    cells, gts = [[] for _ in range(n_frames)], []
    for o in range(n_obj):
        x, y = 30.0 + 150.0 * o, rng.uniform(20, 120)
        w, h = rng.uniform(40, 60, 2)
        vx, vy = rng.uniform(-2, 2, 2)
        base = rng.uniform(0.5, 0.95)
        missed, t = set(), int(rng.integers(5, 9))
        while t < 44:
            r = int(rng.integers(1, 4))
            missed.update(range(t, t + r))
            t += r + int(rng.integers(5, 9))
        boxes = []
        for f in range(n_frames):
            true = [x + vx * f, y + vy * f, x + vx * f + w, y + vy * f + h]
            boxes.append(true)
            if f in missed:
                continue
            d = rng.uniform(-1.5, 1.5, 4)
            cells[f].append([true[k] + d[k] for k in range(4)] + [float(np.clip(base + rng.normal(0, 0.03), 0.05, 1.0))])
        gts.append({"category": 1, "frames": list(range(n_frames)), "boxes": boxes})
    all_boxes, frame_index = cases.nested([("v", list(range(n_frames)), {1: cells})], 2)
    return all_boxes, frame_index, {"v": gts}
