"""Inputs for the trajectory-mAP tests (no tests here): hand-worked cases with their expected ``ov`` / ``hit`` written out, a
seeded generator of a batch that holds every shape at which the kernels take another path, and the ground truth of the
objects that ``seqnms_cases.device_batch`` plants (recovered from its seed: the generator does not hand them out)."""
import numpy as np

import seqnms_cases

THRESHOLDS = (0.5, 0.7, 0.9)

# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases: one video "v".  B is 10 x 10 pixels in the +1 convention (area 100), HALF its upper half (area 50), FAR a
# box that meets neither.  Every volume and intersection is a small integer, so every sum is exact in any order.
# ---------------------------------------------------------------------------------------------------------------------
B, HALF, FAR = [0, 0, 9, 9], [0, 0, 9, 4], [100, 100, 109, 109]


def _t(cls, frames, box=B, score=None):
    tr = {"category": cls, "frames": list(frames), "boxes": [list(box) for _ in frames]}
    if score is not None:
        tr["score"] = score
    return tr


# name: predictions, ground truths; ov[p] = the prediction's row over the ground truths of its cell; hit[k][p] at THRESHOLDS[k]
HAND = {
    # the same trajectory: 300 / (600 - 300)
    "identical": dict(pred=[_t(1, [0, 1, 2], score=0.5)], gt=[_t(1, [0, 1, 2])], ov=[[1.0]], hit=[[0], [0], [0]]),
    # no common frame number: 0, although the boxes coincide
    "disjoint_frames": dict(pred=[_t(1, [0, 1], score=0.5)], gt=[_t(1, [5, 6])], ov=[[0.0]], hit=[[-1], [-1], [-1]]),
    # one of two equal-area frames, the identical box: 100 / (100 + 200 - 100) = 0.5 exactly: a hit at 0.5 (>=), a miss at 0.7
    "half": dict(pred=[_t(1, [0], score=0.5)], gt=[_t(1, [0, 1])], ov=[[0.5]], hit=[[0], [-1], [-1]]),
    # three of four frames: 300 / (300 + 400 - 300) = 0.75 exactly
    "three_quarters": dict(pred=[_t(1, [0, 1, 2], score=0.5)], gt=[_t(1, [0, 1, 2, 3])], ov=[[0.75]], hit=[[0], [0], [-1]]),
    # two predictions over one ground truth: the higher score (packed second) takes it, the other is a false positive
    "contested": dict(pred=[_t(1, [0, 1], score=0.75), _t(1, [0, 1], score=0.875)], gt=[_t(1, [0, 1])], ov=[[1.0], [1.0]],
                      hit=[[-1, 0]] * 3),
    # equal scores: the packed order decides
    "equal_scores": dict(pred=[_t(1, [0, 1], score=0.5), _t(1, [0, 1], score=0.5)], gt=[_t(1, [0, 1])], ov=[[1.0], [1.0]],
                         hit=[[0, -1]] * 3),
    # equal ov over two ground truths: the lowest index; the next prediction takes the other one
    "equal_ov": dict(pred=[_t(1, [0, 1], score=0.25), _t(1, [0, 1], score=0.5)], gt=[_t(1, [0, 1]), _t(1, [0, 1])],
                     ov=[[1.0, 1.0], [1.0, 1.0]], hit=[[1, 0]] * 3),
    # the ground truth leaves for two frames, the prediction bridges the gap: 400 / (600 + 400 - 400)
    "gt_gap": dict(pred=[_t(1, range(6), score=0.5)], gt=[_t(1, [0, 1, 4, 5])], ov=[[400.0 / 600.0]], hit=[[0], [-1], [-1]]),
    # the prediction has a gap and half the height: 2 * 50 / (100 + 300 - 100)
    "pred_gap": dict(pred=[_t(1, [0, 2], HALF, score=0.5)], gt=[_t(1, [0, 1, 2])], ov=[[100.0 / 300.0]], hit=[[-1], [-1], [-1]]),
    # another class in the same video is another cell; boxes that do not meet on common frames: 0
    "classes_apart": dict(pred=[_t(2, [0, 1], score=0.5), _t(1, [0, 1], FAR, score=0.25)], gt=[_t(1, [0, 1]), _t(2, [0, 1])],
                          ov=[[1.0], [0.0]], hit=[[0, -1]] * 3),
}


def hand(name):
    case = HAND[name]
    return {"v": case["pred"]}, {"v": case["gt"]}


def check_hand(name, pk, ov, hit):
    """Compare flat results with the case's expectation (rows of ``ov`` / columns of ``hit`` are in packed order)."""
    case = HAND[name]
    by_class = {}
    for k, tr in enumerate(case["pred"]):
        by_class.setdefault(tr["category"], []).append(k)
    packed = [k for _, c in pk.cells for k in by_class.get(c, [])]             # packed prediction -> its index in the case
    assert list(pk.pred_src) == packed, (name, list(pk.pred_src), packed)
    n_gt = np.diff(pk.cell_gt_off)[np.repeat(np.arange(len(pk.cells)), np.diff(pk.cell_pred_off))]
    for row, k, n in zip(ov, packed, n_gt):
        assert list(row[:n]) == case["ov"][k] and (row[n:] == -1).all(), (name, k, list(row), case["ov"][k])
    for t in range(len(THRESHOLDS)):
        assert [int(x) for x in hit[t]] == [case["hit"][t][k] for k in packed], (name, t, list(hit[t]), case["hit"][t])


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
def _gt(rng, cls, frames, integer, size=320):
    frames = np.asarray(frames, np.int64)
    w, h = rng.integers(20, 60, 2)
    x, y = rng.integers(0, size - 80, 2)
    vx, vy = rng.integers(-2, 3, 2)
    t = (frames - frames[0]).astype(np.float64)
    boxes = np.stack([x + vx * t, y + vy * t, x + vx * t + w, y + vy * t + h], 1)
    if not integer:
        boxes = (boxes + rng.uniform(-0.5, 0.5, boxes.shape)).astype(np.float32)
    return {"category": cls, "frames": frames.tolist(), "boxes": boxes}


def _pred(rng, gt, integer, noise, gapfree=False):
    """A detection of ``gt``: a sub-span of its frames with a few dropped (``gapfree``: none), the boxes off by up to ``noise``
    pixels."""
    n = len(gt["frames"])
    lo = int(rng.integers(0, max(n // 4, 1)))
    hi = n - int(rng.integers(0, max(n // 4, 1)))
    keep = np.arange(lo, hi)
    if len(keep) > 4 and not gapfree:
        keep = keep[rng.random(len(keep)) >= 0.1]
    boxes = np.asarray(gt["boxes"])[keep]
    if integer:
        boxes = boxes + rng.integers(-noise, noise + 1, boxes.shape)
    else:
        boxes = (boxes + rng.uniform(-noise, noise, boxes.shape).astype(np.float32)).astype(np.float32)
    return {"category": gt["category"], "score": float(rng.integers(1, 64)) / 64.0, "frames": [gt["frames"][k] for k in keep],
            "boxes": boxes}


def _cell(rng, cls, frames, n_gt, integer, short=False, full=False, gaps=False, predictions=True, gapfree=False, rivals=False):
    """The trajectories of one cell over a video's ``frames``: (predictions, ground truths)."""
    gts, preds = [], []
    for g in range(n_gt):
        if short:                                                # many objects: one to three frames each
            s = int(rng.integers(0, len(frames)))
            fr = frames[s:s + int(rng.integers(1, 4))]
        elif full and g == 0:
            fr = frames
        else:
            s = int(rng.integers(0, max(len(frames) // 3, 1)))
            fr = frames[s:len(frames) - int(rng.integers(0, max(len(frames) // 3, 1)))]
            if gaps and len(fr) > 8:                             # the object leaves the frame and comes back
                a = int(rng.integers(2, len(fr) // 2))
                fr = fr[:a] + fr[a + int(rng.integers(1, len(fr) // 4 + 1)):]
        gts.append(_gt(rng, cls, fr, integer))
        if integer and g % 7 == 3:                               # a duplicate annotation: equal ov over two ground truths
            gts[-1] = dict(gts[g - 1], boxes=np.array(gts[g - 1]["boxes"]))
        elif rivals and g % 3 == 2:                              # a neighbour a few pixels off: two unequal ov to choose from
            near = np.asarray(gts[g - 1]["boxes"])
            gts[-1] = dict(gts[g - 1], boxes=(near + rng.integers(-4, 5, 4)).astype(near.dtype))
    if predictions:
        for g, gt in enumerate(gts):
            if full and g == 0:
                preds.append(dict(_gt(rng, cls, gt["frames"], integer), boxes=np.array(gt["boxes"]), score=0.984375))
            for _ in range(int(rng.integers(0, 3)) if not short else int(rng.random() < 0.6)):
                preds.append(_pred(rng, gt, integer, int(rng.choice([0, 1, 3, 6])), gapfree))
        for _ in range(int(rng.integers(0, 3)) or int(n_gt == 0)):       # clutter; a cell without ground truth has some
            s = int(rng.integers(0, len(frames)))
            preds.append(dict(_gt(rng, cls, frames[s:s + int(rng.integers(1, 12))], integer), score=float(rng.integers(1, 32)) / 64.0))
        order = rng.permutation(len(preds))
        preds = [preds[i] for i in order]
    return preds, gts


def batch(seed=2024):
    """(prediction, groundtruth, facts).  Videos of 1, 63, 64, 65, 129 and 300 frames, each with a gap-free full-length ground
    truth and its prediction; cells with 0 predictions, with 0 ground truths and with 1, 63, 64 and 65 ground truths; video "g"
    has no prediction at all, video "h" predictions but no ground truth (it takes no part); class 9 has predictions only;
    cells with integer boxes (every sum exact) next to cells of float32 draws; scores on a grid of 1/64, so ties occur."""
    rng = np.random.default_rng(seed)
    prediction, groundtruth = {}, {}

    def video(vid, n_frames, cells):
        first = int(rng.integers(0, 50))
        frames = list(range(first, first + n_frames))
        prediction[vid], groundtruth[vid] = [], []
        for cls, kw in cells:
            p, g = _cell(rng, cls, frames, **kw)
            prediction[vid] += p
            groundtruth[vid] += g

    video("a", 1, [(1, dict(n_gt=1, integer=True, full=True)), (2, dict(n_gt=2, integer=False, full=True))])
    video("b", 63, [(1, dict(n_gt=63, integer=True, short=True)), (2, dict(n_gt=2, integer=False, full=True))])
    video("c", 64, [(1, dict(n_gt=64, integer=False, short=True)), (3, dict(n_gt=3, integer=True, full=True))])
    video("d", 65, [(1, dict(n_gt=65, integer=True, short=True)), (2, dict(n_gt=1, integer=False, full=True)),
                    (3, dict(n_gt=2, integer=True, predictions=False))])
    video("e", 129, [(2, dict(n_gt=3, integer=False, full=True, gaps=True)), (9, dict(n_gt=0, integer=True))])
    video("f", 300, [(3, dict(n_gt=3, integer=False, full=True, gaps=True)), (1, dict(n_gt=1, integer=True, full=True))])
    video("g", 10, [(1, dict(n_gt=2, integer=True, predictions=False)), (2, dict(n_gt=1, integer=False, predictions=False))])
    video("h", 12, [(1, dict(n_gt=0, integer=True))])
    for k in range(8):
        video("r%d" % k, int(rng.integers(2, 40)), [(int(c), dict(n_gt=int(rng.integers(1, 6)), integer=bool((k + c) % 2), gaps=True, rivals=True))
                                                    for c in rng.choice([1, 2, 3, 4], size=int(rng.integers(2, 4)), replace=False)])
    del prediction["g"]
    assert not groundtruth["h"] and prediction["h"]
    return prediction, groundtruth


GOLDEN_CASES = 12            # tests/golden/track_eval.npz: the even ones integer boxes, the odd ones float32 draws
GOLDEN_SEED = 5000           # case k starts at seed GOLDEN_SEED + 100 k; the file records the seed it ended on


def golden_case(seed, integer):
    """One video of gap-free trajectories (what the reference's ``viou`` takes) in three or four classes, one of them without
    ground truth: (prediction, groundtruth)."""
    rng = np.random.default_rng(seed)
    frames = list(range(int(rng.integers(0, 20)), int(rng.integers(25, 100))))
    preds, gts = [], []
    for cls in range(1, int(rng.integers(4, 6))):
        p, g = _cell(rng, cls, frames, n_gt=int(rng.integers(1, 7)) if cls > 1 else 0, integer=integer, gapfree=True, rivals=True)
        preds += p
        gts += g
    return {"g": preds}, {"g": gts}


def check_batch_facts(pk, hit):
    """What the generated batch must hold (the shapes at which a wave-of-64 form takes another path): a generator change cannot
    silently drop an edge."""
    lengths = set(np.diff(pk.traj_off).tolist())
    assert {1, 63, 64, 65, 129, 300} <= lengths, sorted(lengths)
    n_gt, n_pred = np.diff(pk.cell_gt_off), np.diff(pk.cell_pred_off)
    assert {0, 1, 63, 64, 65} <= set(n_gt.tolist()) and (n_pred == 0).any() and ((n_pred > 0) & (n_gt == 0)).any()
    assert 24 <= len(pk.cells) <= 64 and 2000 <= len(pk.frame) <= 9000, (len(pk.cells), len(pk.frame))
    vids = set(v for v, _ in pk.cells)
    assert "g" in vids and "h" not in vids
    assert all(n_gt[c] == 0 for c, (_, cls) in enumerate(pk.cells) if cls == 9) and any(cls == 9 for _, cls in pk.cells)
    n_hit = [(hit[k] >= 0).sum() for k in range(3)]
    assert n_hit[0] > n_hit[1] > n_hit[2] > 0, n_hit              # three thresholds, three hit sets
    assert (hit >= 64).any()                                     # a detected ground truth in a lane's second bit
    gaps = [t for t in range(len(pk.traj_off) - 1)
            if (np.diff(pk.frame[pk.traj_off[t]:pk.traj_off[t + 1]]) > 1).any()]
    assert any(t < pk.n_pred for t in gaps) and any(t >= pk.n_pred for t in gaps)


# ---------------------------------------------------------------------------------------------------------------------
# the objects seqnms_cases.device_batch plants
# ---------------------------------------------------------------------------------------------------------------------
def seqnms_batch_with_groundtruth(seed=77):
    """``seqnms_cases.device_batch(seed)`` again, draw for draw, keeping what it does not hand out: the planted objects.
    Returns (all_boxes, frame_index, groundtruth) with one ground-truth trajectory per object over all frames of its video
    (the object's noise-free box; ``gen_cells`` draws the objects first, so a copy of the generator's state yields them).  The
    caller compares ``all_boxes`` with ``device_batch``'s: a change of that generator cannot go unnoticed."""
    rng = np.random.default_rng(seed)
    videos, groundtruth = [], {}
    width, height = 320, 240
    for v, (nf, gaps) in enumerate([(1, 0), (2, 0), (3, 0), (37, 3), (64, 0), (65, 1), (130, 4)]):
        frame_no = seqnms_cases.frame_numbers(rng, nf, gaps)
        per_class, gts = {}, []
        for j in range(1, 5):
            if nf == 37 and j == 4:
                continue
            counts = None
            if nf == 37 and j == 1:
                counts = {5: 0, 6: 1, 7: 63, 8: 64, 9: 64, 36: 64}
            if nf == 3 and j == 2:
                counts = {0: 64, 1: 63, 2: 0}
            if nf == 1 and j == 3:
                counts = {0: 0}
            n_obj = int(rng.integers(1, 5))
            clutter = int(rng.integers(0, 3))
            peek = np.random.default_rng(0)
            peek.bit_generator.state = rng.bit_generator.state
            objs = [(peek.uniform(20, width - 80), peek.uniform(20, height - 80), peek.uniform(24, 60), peek.uniform(24, 60),
                     peek.uniform(-3, 3), peek.uniform(-2, 2), peek.uniform(0.4, 0.95)) for _ in range(n_obj)]
            per_class[j] = seqnms_cases.gen_cells(rng, nf, n_obj=n_obj, clutter=clutter, counts=counts)
            for x, y, w, h, vx, vy, _ in objs:
                gts.append({"category": j, "frames": [int(f) for f in frame_no],
                            "boxes": [[x + vx * t, y + vy * t, x + vx * t + w, y + vy * t + h] for t in range(nf)]})
        videos.append(("v%d" % v, frame_no, per_class))
        groundtruth["v%d" % v] = gts
    all_boxes, frame_index = seqnms_cases.nested(videos, 5)
    return all_boxes, frame_index, groundtruth


def one_frame_tracks(all_boxes, frame_index):
    """The track ids that make every box of ``all_boxes`` a track of its own (numbered per video and class, as Seq-NMS does)."""
    tracks = [[None] * len(frame_index) for _ in all_boxes]
    nxt = {}
    for j in range(len(all_boxes)):
        for i, (vid, _) in enumerate(frame_index):
            n = len(np.asarray(all_boxes[j][i]).reshape(-1, 5))
            k = nxt.get((vid, j), 0)
            tracks[j][i] = np.arange(k, k + n, dtype=np.int32)
            nxt[(vid, j)] = k + n
    return tracks
