"""Built cases of the video relation NMS (i2vsgg_amd.video.suppress), shared by the host tests, the GPU tests and
tools/gen_golden.py (gen_video_nms).  A case is (name, prediction, T, pool, cap); the hand cases also carry the answer that
follows from the rules by hand.  Everything is seeded; nothing here imports the package."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name prediction T pool cap")
CELL_SIZES = (1, 2, 63, 64, 65, 129, 200)
TRAJ_FRAMES = (1, 10, 63, 64, 65, 130)
GOLDEN_SEED, GOLDEN_CASES = 7100, 12             # cases 10 and 11 have fractional boxes
GOLDEN_T = (0.7, 0.5, 0.3, 0.7, 0.5, 0.9, 0.7, 0.5, 0.0, 1.0, 0.7, 0.5)


def rel(triplet, score, fstart, sub, obj, **extra):
    r = {"triplet": list(triplet), "score": float(score), "duration": [int(fstart), int(fstart) + len(sub)],
         "sub_traj": [list(map(float, b)) for b in sub], "obj_traj": [list(map(float, b)) for b in obj]}
    r.update(extra)
    return r


def walk(rng, frames, integer=True):
    """A box that drifts: (frames, 4) float64, x2 >= x1 and y2 >= y1."""
    x, y = rng.integers(0, 200, 2)
    w, h = rng.integers(20, 90, 2)
    step = np.cumsum(rng.integers(-2, 3, (frames, 2)), 0)
    b = np.stack([x + step[:, 0], y + step[:, 1], x + step[:, 0] + w, y + step[:, 1] + h], 1).astype(np.float64)
    return b if integer else b + rng.random((frames, 1)) * 0.5


def cluster_cell(rng, triplet, n, frames, n_objects=4, integer=True, grid=64):
    """n relations of one triplet: each follows one of ``n_objects`` (subject, object) trajectory pairs with 0-2 px of jitter
    per frame, starts 0-2 frames late and ends 0-2 frames early; scores lie on a coarse grid, so some are equal."""
    base = [(walk(rng, frames, integer), walk(rng, frames, integer)) for _ in range(n_objects)]
    out = []
    for _ in range(n):
        s, o = base[int(rng.integers(n_objects))]
        head = int(rng.integers(0, 3)) if frames > 4 else 0
        tail = frames - (int(rng.integers(0, 3)) if frames > 4 else 0)

        def jit(b):
            j = rng.integers(0, 3, (tail - head, 4)) if integer else rng.random((tail - head, 4)) * 2.0
            b = b[head:tail] + j * np.array([-1.0, -1.0, 1.0, 1.0])      # grows outwards: x2 >= x1 stays
            return b
        out.append(rel(triplet, rng.integers(1, grid) / float(grid), 100 + head, jit(s), jit(o)))
    return out


def size_cases():
    """One video per cell size, the trajectory lengths going round; T = 0.7."""
    rng = np.random.default_rng(7001)
    pred = {}
    for k, n in enumerate(CELL_SIZES):
        pred["size%d" % n] = cluster_cell(rng, (1, k, 2), n, TRAJ_FRAMES[k % len(TRAJ_FRAMES)], n_objects=1 + n // 40)
    return Case("sizes", pred, 0.7, 2048, 200)


def frame_cases():
    """One cell of 40 per trajectory length, one video: six triplets."""
    rng = np.random.default_rng(7002)
    rels = []
    for k, f in enumerate(TRAJ_FRAMES):
        rels += cluster_cell(rng, (3, k, 4), 40, f, n_objects=3)
    order = rng.permutation(len(rels))                   # the cells interleave in the input
    return Case("frames", {"v": [rels[i] for i in order]}, 0.5, 2048, 200)


def big_case():
    """One cell of 1025 relations of 12 frames: more than 16 words of 64 columns, more than four strides of 256 lanes."""
    rng = np.random.default_rng(7003)
    return Case("big", {"big": cluster_cell(rng, (5, 6, 7), 1025, 12, n_objects=40, grid=4096)}, 0.6, 2048, 200)


def edge_cases():
    """Cells at the kernel's stride of 256 lanes: two cells of 256 rows (every column of a kept row in exactly one pass), and
    cells of 256 and 255."""
    rng = np.random.default_rng(7006)
    two = lambda n: cluster_cell(rng, (1, 1, 2), 256, 8, n_objects=30, grid=4096) + cluster_cell(rng, (2, 1, 1), n, 8, n_objects=30, grid=4096)
    return [Case("edge_wide", {"e": two(256)}, 0.6, 2048, 200), Case("edge_narrow", {"e": two(255)}, 0.6, 2048, 200)]


def multi_case():
    """Several videos and cells in one call: a video with no relation, a triplet with one member, names as triplets."""
    rng = np.random.default_rng(7004)
    a = cluster_cell(rng, ("dog", "chase", "cat"), 30, 20) + cluster_cell(rng, ("cat", "watch", "dog"), 1, 20) + \
        cluster_cell(rng, ("dog", "near", "cat"), 17, 11, n_objects=2)
    b = cluster_cell(rng, ("dog", "chase", "cat"), 70, 15, n_objects=5)
    order = rng.permutation(len(a))
    return Case("multi", {"a": [a[i] for i in order], "empty": [], "b": b, "one": cluster_cell(rng, (1, 1, 1), 1, 1)}, 0.7, 2048, 200)


def fractional_case(seed=7005):
    rng = np.random.default_rng(seed)
    rels = cluster_cell(rng, (1, 2, 3), 60, 25, n_objects=3, integer=False, grid=1 << 20) + \
        cluster_cell(rng, (3, 2, 1), 45, 9, n_objects=2, integer=False, grid=1 << 20)
    return Case("fractional", {"f": rels}, 0.7, 2048, 200)


def _box_traj(box, n):
    return [list(box)] * n


# ---- hand cases: (Case, expected) with expected = {vid: indices into the video's input list, in output order} and, where it
# matters, by / by_ov by input index -----------------------------------------------------------------------------------------
def hand_cases():
    out = []
    A, B, C = [0, 0, 19, 9], [4, 0, 23, 9], [8, 0, 27, 9]        # 20 wide at x = 0, 4, 8: ov AB = BC = 2/3, AC = 3/7
    far = [500, 500, 520, 520]
    t = (1, 2, 3)
    # equal scores: the lower input index ranks first and suppresses the other
    out.append((Case("tie", {"v": [rel(t, 0.5, 0, _box_traj(A, 3), _box_traj(A, 3)), rel(t, 0.5, 0, _box_traj(A, 3), _box_traj(A, 3)),
                                   rel(t, 0.9, 0, _box_traj(far, 3), _box_traj(far, 3))]}, 0.7, 2048, 200), {"v": [2, 0]}))
    # identical relations: ov = 1 > T for every T < 1; at T = 1 nothing is suppressed (strict)
    same = lambda: {"v": [rel(t, 0.9, 5, _box_traj(A, 10), _box_traj(B, 10)), rel(t, 0.8, 5, _box_traj(A, 10), _box_traj(B, 10))]}
    out.append((Case("identical", same(), 0.99, 2048, 200), {"v": [0]}))
    out.append((Case("identical_T1", same(), 1.0, 2048, 200), {"v": [0, 1]}))
    # durations that only touch: [0, 5) and [5, 10) share no frame, ov = 0 (and T = 0 suppresses nothing: 0 > 0 is false)
    out.append((Case("touch", {"v": [rel(t, 0.9, 0, _box_traj(A, 5), _box_traj(A, 5)), rel(t, 0.8, 5, _box_traj(A, 5), _box_traj(A, 5))]},
                     0.0, 2048, 200), {"v": [0, 1]}))
    # the subject overlaps, the object does not: min is 0
    out.append((Case("subject_only", {"v": [rel(t, 0.9, 0, _box_traj(A, 4), _box_traj(A, 4)), rel(t, 0.8, 0, _box_traj(A, 4), _box_traj(far, 4))]},
                     0.1, 2048, 200), {"v": [0, 1]}))
    # different triplets with identical trajectories: different cells
    out.append((Case("triplets", {"v": [rel((1, 2, 3), 0.9, 0, _box_traj(A, 4), _box_traj(B, 4)), rel((1, 2, 4), 0.8, 0, _box_traj(A, 4), _box_traj(B, 4)),
                                        rel((1, 2, 3), 0.7, 0, _box_traj(A, 4), _box_traj(B, 4))]}, 0.5, 2048, 200), {"v": [0, 1]}))
    # ov exactly at T: [0,0,9,9] against [0,0,9,4] on one frame is 50 / 100 = 0.5
    at = lambda: {"v": [rel(t, 0.9, 0, [[0, 0, 9, 9]], [[0, 0, 9, 9]]), rel(t, 0.8, 0, [[0, 0, 9, 4]], [[0, 0, 9, 4]])]}
    out.append((Case("at_T", at(), 0.5, 2048, 200), {"v": [0, 1]}))
    out.append((Case("below_T", at(), float(np.nextafter(0.5, 0.0)), 2048, 200), {"v": [0]}))
    # the chain: A suppresses B (2/3 > 0.5); C stays, because B is not kept and AC = 3/7
    chain = {"v": [rel(t, 0.9, 0, _box_traj(A, 3), _box_traj(A, 3)), rel(t, 0.8, 0, _box_traj(B, 3), _box_traj(B, 3)),
                   rel(t, 0.7, 0, _box_traj(C, 3), _box_traj(C, 3))]}
    out.append((Case("chain", chain, 0.5, 2048, 200), {"v": [0, 2]}))
    # the pool cuts a cell: of five duplicates and one far relation of lowest score, pool = 3 sees three duplicates only
    dup = lambda s: rel(t, s, 0, _box_traj(A, 3), _box_traj(A, 3))
    pool = {"v": [dup(0.5), dup(0.9), dup(0.8), dup(0.7), dup(0.6), rel(t, 0.1, 0, _box_traj(far, 3), _box_traj(far, 3))]}
    out.append((Case("pool", pool, 0.7, 3, 200), {"v": [1]}))
    out.append((Case("pool_all", pool, 0.7, 6, 200), {"v": [1, 5]}))
    # the cap cuts the kept list: five far-apart relations, cap 2 -> the two best, in descending score
    boxes = [[100 * k, 0, 100 * k + 20, 20] for k in range(5)]
    cap = {"v": [rel(t, s, 0, _box_traj(b, 2), _box_traj(b, 2)) for s, b in zip((0.3, 0.9, 0.5, 0.7, 0.1), boxes)]}
    out.append((Case("cap", cap, 0.7, 2048, 2), {"v": [1, 3]}))
    return out


def built_cases():
    """Every case the host and device forms are compared on."""
    return [size_cases(), frame_cases(), big_case(), multi_case(), fractional_case()] + edge_cases() + [c for c, _ in hand_cases()]


def golden_case(k, seed=None):
    """Case k of tests/golden/video_nms.npz; ``seed``: the one the generator ended on (fractional cases may be redrawn)."""
    integer = k < GOLDEN_CASES - 2
    rng = np.random.default_rng(GOLDEN_SEED + 100 * k if seed is None else seed)
    pred = {}
    for v in range(1 + k % 3):
        rels = []
        for c in range(1 + (k + v) % 3):
            rels += cluster_cell(rng, (c, k, v), int(rng.integers(1, 40)), int(rng.integers(1, 26)), n_objects=1 + c, integer=integer,
                                 grid=64 if integer else 1 << 20)
        order = rng.permutation(len(rels))
        pred["g%d_%d" % (k, v)] = [rels[i] for i in order]
    return Case("golden%d" % k, pred, GOLDEN_T[k], 2048, 200)


def frame_results(frames):
    """One video's frames ([[fno, predictions], ...] of synthetic.video_frames) as the pickle of the relation test loop: {path:
    (labels, confs, sub_boxes, obj_boxes, rel_idex)}."""
    out = {}
    for fno, preds in frames:
        out["data/frames/%06d.jpg" % fno] = (np.asarray([p[1] for p in preds], np.float64), np.asarray([p[0] for p in preds], np.float64),
                                             np.asarray([p[2][0] for p in preds], np.float64), np.asarray([p[2][1] for p in preds], np.float64),
                                             np.asarray([p[3] for p in preds], np.int64))
    return out


def duplicates_case(n_videos=6, n_gt=4, copies=60, frames=20, seed=7200):
    """The end-to-end case: every annotated relation predicted ``copies`` times with 0-2 px of jitter -> (prediction,
    groundtruth).  Without suppression the 200 slots of a video hold 200 of its 240 duplicates."""
    rng = np.random.default_rng(seed)
    pred, gt = {}, {}
    for v in range(n_videos):
        vid = "vid%d" % v
        gts, preds = [], []
        for g in range(n_gt):
            s, o = walk(rng, frames), walk(rng, frames) + 300.0 * (g + 1)
            trip = (g, 1, g + 10)
            gts.append({"triplet": list(trip), "duration": [0, frames], "sub_traj": s.tolist(), "obj_traj": o.tolist()})
            for _ in range(copies):
                j = lambda b: b + rng.integers(0, 3, b.shape) * np.array([-1.0, -1.0, 1.0, 1.0])
                preds.append(rel(trip, 0.9 - 0.15 * g + 0.2 * rng.random(), 0, j(s), j(o)))     # bands that overlap by a quarter
        order = rng.permutation(len(preds))
        pred[vid], gt[vid] = [preds[i] for i in order], gts
    return pred, gt
