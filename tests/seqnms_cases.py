"""Inputs for the Seq-NMS tests (no tests here): a seeded generator of groups, the hand-worked cases with their expected
results, and two independent restatements of the rules -- a brute-force enumerator of all link paths for tiny inputs and a
plain full-recomputation Seq-NMS in Python floats.  Nothing here imports i2vsgg_amd.seqnms: the overlap is written out again."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------------
# the rules again, scalar Python floats (IEEE double), no shortcut
# ---------------------------------------------------------------------------------------------------------------------
def overlap(a, b):
    a, b = [float(x) for x in a[:4]], [float(x) for x in b[:4]]
    iw = (min(a[2], b[2]) - max(a[0], b[0])) + 1.0
    ih = (min(a[3], b[3]) - max(a[1], b[1])) + 1.0
    if iw <= 0.0 or ih <= 0.0:
        return 0.0
    inter = iw * ih
    return inter / ((((a[2] - a[0]) + 1.0) * ((a[3] - a[1]) + 1.0) + ((b[2] - b[0]) + 1.0) * ((b[3] - b[1]) + 1.0)) - inter)


def linked(frame_no, cells, t, a, b, link_iou):
    return int(frame_no[t + 1]) == int(frame_no[t]) + 1 and overlap(cells[t][a], cells[t + 1][b]) >= link_iou


def brute_force_best_sum(frame_no, cells, link_iou=0.5):
    """The largest sum of scores over ALL link paths of one group (every start, every continuation, every stop)."""
    best = [-np.inf]

    def walk(t, a, s):
        s = s + float(cells[t][a][4])
        best[0] = max(best[0], s)
        if t + 1 < len(cells):
            for b in range(len(cells[t + 1])):
                if linked(frame_no, cells, t, a, b, link_iou):
                    walk(t + 1, b, s)

    for t in range(len(cells)):
        for a in range(len(cells[t])):
            walk(t, a, 0.0)
    return best[0]


def naive_seq_nms(frame_no, cells, link_iou=0.5, nms_iou=0.3, rescore="avg"):
    """One group, every pass recomputed in full.  Returns per frame (tid list, score list as np.float32)."""
    nf = len(cells)
    alive = [[True] * len(c) for c in cells]
    tid = [[-1] * len(c) for c in cells]
    new = [[np.float32(r[4]) for r in c] for c in cells]
    k = 0
    while any(any(al) for al in alive):
        best = [[0.0] * len(c) for c in cells]
        ptr = [[-1] * len(c) for c in cells]
        for t in range(nf - 1, -1, -1):
            for a in range(len(cells[t])):
                if not alive[t][a]:
                    continue
                mx, pb = 0.0, -1
                if t + 1 < nf:
                    for b in range(len(cells[t + 1])):
                        if alive[t + 1][b] and linked(frame_no, cells, t, a, b, link_iou) and (pb < 0 or best[t + 1][b] > mx):
                            mx, pb = best[t + 1][b], b
                best[t][a] = float(cells[t][a][4]) + mx if pb >= 0 else float(cells[t][a][4])
                ptr[t][a] = pb
        start = None
        for t in range(nf):
            for a in range(len(cells[t])):
                if alive[t][a] and (start is None or best[t][a] > best[start[0]][start[1]]):
                    start = (t, a)
        path = [start]
        while ptr[path[-1][0]][path[-1][1]] >= 0:
            t, a = path[-1]
            path.append((t + 1, ptr[t][a]))
        if rescore == "max":
            ns = max(np.float32(cells[t][a][4]) for t, a in path)
        else:
            s = 0.0
            for t, a in path:
                s += float(cells[t][a][4])
            ns = np.float32(s / len(path))
        for t, a in path:
            for b in range(len(cells[t])):
                if alive[t][b] and (b == a or overlap(cells[t][a], cells[t][b]) > nms_iou):
                    alive[t][b] = False
            tid[t][a], new[t][a] = k, ns
        k += 1
    return tid, new, k


# ---------------------------------------------------------------------------------------------------------------------
# nested layouts
# ---------------------------------------------------------------------------------------------------------------------
def cell(rows):
    return np.asarray(rows, np.float32).reshape(-1, 5)


def nested(videos, n_classes):
    """``videos``: [(vid, frame_no list, {class j: cells (one (n,5) array per frame)})].  Returns (all_boxes, frame_index) in
    the layout of ``detections.pkl``: class 0 (background) holds ``[]`` everywhere, a class a video says nothing about is
    empty in its frames."""
    frame_index = [(vid, int(fno)) for vid, frame_no, _ in videos for fno in frame_no]
    all_boxes = [[[] for _ in frame_index] for _ in range(n_classes)]
    i0 = 0
    for vid, frame_no, per_class in videos:
        for j in range(1, n_classes):
            for t in range(len(frame_no)):
                all_boxes[j][i0 + t] = cell(per_class[j][t]) if j in per_class else cell([])
        i0 += len(frame_no)
    return all_boxes, frame_index


# ---------------------------------------------------------------------------------------------------------------------
# the generator: a few objects move linearly with jitter, are sometimes missed, sometimes detected twice; clutter
# ---------------------------------------------------------------------------------------------------------------------
def gen_cells(rng, n_frames, n_obj=3, clutter=2, p_miss=0.15, p_dup=0.2, width=320, height=240, counts=None):
    """Cells of one group.  ``counts`` {frame: n} forces a frame to exactly n rows (non-overlapping grid boxes when n is
    large, so that all of them survive)."""
    objs = [(rng.uniform(20, width - 80), rng.uniform(20, height - 80), rng.uniform(24, 60), rng.uniform(24, 60),
             rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(0.4, 0.95)) for _ in range(n_obj)]
    out = []
    for t in range(n_frames):
        rows = []
        for x, y, w, h, vx, vy, base in objs:
            if rng.random() < p_miss:
                continue
            jx, jy = rng.uniform(-2, 2, 2)
            box = [x + vx * t + jx, y + vy * t + jy, x + vx * t + jx + w, y + vy * t + jy + h]
            rows.append(box + [float(np.clip(base + rng.normal(0, 0.05), 0.02, 1.0))])
            if rng.random() < p_dup:
                d = rng.uniform(-4, 4, 4)
                rows.append([box[k] + d[k] for k in range(4)] + [float(np.clip(base - rng.uniform(0.05, 0.3), 0.01, 1.0))])
        for _ in range(int(rng.integers(0, clutter + 1))):
            x, y = rng.uniform(0, width - 40), rng.uniform(0, height - 40)
            rows.append([x, y, x + rng.uniform(10, 40), y + rng.uniform(10, 40), float(rng.uniform(0.01, 0.3))])
        if counts is not None and t in counts:
            rows = rows[:counts[t]]
            k = 0
            while len(rows) < counts[t]:                 # a grid of small boxes far from each other
                gx, gy = (k % 16) * 20.0, 400.0 + (k // 16) * 20.0
                rows.append([gx, gy, gx + 8.0, gy + 8.0, float(rng.uniform(0.05, 0.9))])
                k += 1
        order = rng.permutation(len(rows))
        out.append(cell([rows[i] for i in order]))
    return out


def frame_numbers(rng, n_frames, gaps=0):
    """Ascending frame numbers starting somewhere, with ``gaps`` jumps of 2..4 at random places."""
    step = np.ones(n_frames, np.int64)
    if n_frames > 1 and gaps:
        step[rng.choice(np.arange(1, n_frames), size=min(gaps, n_frames - 1), replace=False)] = rng.integers(2, 5)
    step[0] = int(rng.integers(0, 50))
    return np.cumsum(step).tolist()


def tiny_groups(n=300, seed=1234):
    """[(frame_no, cells)]: 1-5 frames, at most 6 boxes per frame, every third group with a gap.  Boxes sit around two
    centres so that many links exist."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n):
        nf = int(rng.integers(1, 6))
        frame_no = frame_numbers(rng, nf, gaps=1 if g % 3 == 0 else 0)
        cells = []
        for t in range(nf):
            rows = []
            for _ in range(int(rng.integers(0, 7))):
                cx, cy = (40.0, 40.0) if rng.random() < 0.5 else (120.0, 60.0)
                x, y = cx + rng.uniform(-12, 12), cy + rng.uniform(-12, 12)
                rows.append([x, y, x + rng.uniform(25, 45), y + rng.uniform(25, 45), float(rng.uniform(0.05, 1.0))])
            cells.append(cell(rows))
        out.append((frame_no, cells))
    return out


def tiny_nested(groups):
    """The tiny groups as one nested layout: every group is its own video with one class."""
    return nested([("t%d" % g, frame_no, {1: cells}) for g, (frame_no, cells) in enumerate(groups)], 2)


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases: one video, one class.  Boxes are 21 x 21 pixels in the +1 convention ([x, y, x + 20, y + 20]); a shift of
# 5 pixels along one axis overlaps 16*21 / (882 - 336) = 0.615, a shift of 2 overlaps 19*21 / (882 - 399) = 0.826, a shift of
# 12 overlaps 9*21 / (882 - 189) = 0.273, shifts of (5, 12) overlap 16*9 / (882 - 144) = 0.195.  Scores are dyadic, so
# every sum and every mean of equal scores is exact.
# ---------------------------------------------------------------------------------------------------------------------
def _b(x, y, s):
    return [x, y, x + 20, y + 20, s]


HAND = {
    # A moves right (score .75), B moves left 12 pixels lower (score .5); they meet at x = 10 in frame 2.  Neither links to
    # the other (0.195 < 0.5) and neither suppresses the other (0.273 <= 0.3): A is track 0 (sum 3.75), B is track 1.
    "crossing": dict(frame_no=[0, 1, 2, 3, 4],
                     cells=[[_b(5 * t, 0, 0.75), _b(20 - 5 * t, 12, 0.5)] for t in range(5)],
                     tid=[[0, 1]] * 5, score=[[0.75, 0.5]] * 5, n_tracks=2),
    # one frame: every box is its own track, in descending score
    "one_frame": dict(frame_no=[7], cells=[[_b(0, 0, 0.5), _b(100, 0, 0.875), _b(200, 0, 0.25)]],
                      tid=[[1, 0, 2]], score=[[0.5, 0.875, 0.25]], n_tracks=3),
    # a static object, frame numbers 0 1 2 | 4 5 6: the gap breaks the link; the later half has the larger sum
    "gap": dict(frame_no=[0, 1, 2, 4, 5, 6], cells=[[_b(0, 0, 0.5)]] * 3 + [[_b(0, 0, 0.75)]] * 3,
                tid=[[1]] * 3 + [[0]] * 3, score=[[0.5]] * 3 + [[0.75]] * 3, n_tracks=2),
    # an empty frame in the middle: links join neighbouring frames only
    "empty_frame": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.5)], [], [_b(0, 0, 0.25)]],
                        tid=[[0], [], [1]], score=[[0.5], [], [0.25]], n_tracks=2),
    # a duplicate 2 pixels off (0.826 > 0.3) leaves with its twin and keeps its score
    "duplicate": dict(frame_no=[3, 4], cells=[[_b(2, 0, 0.625), _b(0, 0, 0.875)], [_b(0, 0, 0.875), _b(2, 0, 0.625)]],
                      tid=[[-1, 0], [0, -1]], score=[[0.625, 0.875], [0.875, 0.625]], n_tracks=1),
    # all scores equal, identical boxes: frame 0's boxes both point at b = 0 (lowest b) and both have best 1.0; the start is
    # (0, 0) (lowest a); identical boxes overlap 1.0 > 0.3, so the twins are suppressed.  The lone box of frame 3 (after a
    # gap) has best 1.0 as well and loses the start to frame 0 (lowest t).
    "ties": dict(frame_no=[0, 1, 3], cells=[[_b(10, 10, 0.5)] * 2, [_b(10, 10, 0.5)] * 2, [_b(10, 10, 1.0)]],
                 tid=[[0, -1], [0, -1], [1]], score=[[0.5, 0.5], [0.5, 0.5], [1.0]], n_tracks=2),
    # the same with nms_iou = 1.0 (1.0 > 1.0 is false: nothing but the path leaves): the twins form track 1 -- its start
    # (0, 1) again beats frame 3 on the frame number -- and frame 3 is track 2
    "ties_keep": dict(frame_no=[0, 1, 3], cells=[[_b(10, 10, 0.5)] * 2, [_b(10, 10, 0.5)] * 2, [_b(10, 10, 1.0)]],
                      kwargs=dict(nms_iou=1.0), tid=[[0, 1], [0, 1], [2]], score=[[0.5, 0.5], [0.5, 0.5], [1.0]], n_tracks=3),
    # avg against max: 0.25 + 0.5 + 1.0 = 1.75 exactly; 1.75 / 3 rounded to double, then to float32
    "avg": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.25)], [_b(0, 0, 0.5)], [_b(0, 0, 1.0)]],
                tid=[[0]] * 3, score=[[np.float32(1.75 / 3.0)]] * 3, n_tracks=1),
    "max": dict(frame_no=[0, 1, 2], cells=[[_b(0, 0, 0.25)], [_b(0, 0, 0.5)], [_b(0, 0, 1.0)]],
                kwargs=dict(rescore="max"), tid=[[0]] * 3, score=[[1.0]] * 3, n_tracks=1),
}


def hand_nested(name):
    case = HAND[name]
    return nested([("v", case["frame_no"], {1: case["cells"]})], 2)


def check_hand(name, tid, new_score, n_tracks, box_off):
    """Compare flat results (one group's boxes start at 0 of the flat arrays) with the case's expectation."""
    case = HAND[name]
    for t, (et, es) in enumerate(zip(case["tid"], case["score"])):
        p, q = int(box_off[t]), int(box_off[t + 1])
        assert list(tid[p:q]) == list(et), (name, t, list(tid[p:q]), et)
        assert [np.float32(x) for x in new_score[p:q]] == [np.float32(x) for x in es], (name, t, list(new_score[p:q]), es)
    assert int(n_tracks) == case["n_tracks"], (name, int(n_tracks))


# ---------------------------------------------------------------------------------------------------------------------
# the device test's launch: 6 videos x 4 classes (class 0 is the background and stays empty: 24 groups)
# ---------------------------------------------------------------------------------------------------------------------
def device_batch(seed=77):
    """Videos of 1, 2, 3, 37, 65 and 130 frames with 5 classes (4 real ones) -- and one more of 64 frames.  Class 4 of the
    37-frame video has no boxes at all; the 37- and 130-frame videos have gaps; frames with 0, 1, 63 and 64 boxes are forced."""
    rng = np.random.default_rng(seed)
    videos = []
    for v, (nf, gaps) in enumerate([(1, 0), (2, 0), (3, 0), (37, 3), (64, 0), (65, 1), (130, 4)]):
        frame_no = frame_numbers(rng, nf, gaps)
        per_class = {}
        for j in range(1, 5):
            if nf == 37 and j == 4:
                continue                                  # a group without boxes
            counts = None
            if nf == 37 and j == 1:
                counts = {5: 0, 6: 1, 7: 63, 8: 64, 9: 64, 36: 64}
            if nf == 3 and j == 2:
                counts = {0: 64, 1: 63, 2: 0}
            if nf == 1 and j == 3:
                counts = {0: 0}
            n_obj = int(rng.integers(1, 5))
            per_class[j] = gen_cells(rng, nf, n_obj=n_obj, clutter=int(rng.integers(0, 3)), counts=counts)
        videos.append(("v%d" % v, frame_no, per_class))
    return nested(videos, 5)
