"""Support code of the proposal-recall tests (not a test): a seeded case generator, the cover restated as the plain step loop
on a dense matrix, and the hand-worked cases.  Written from the rules in i2vsgg_amd/proposal_eval.py's docstring."""
import numpy as np

from i2vsgg_amd.packing import overlap_plus1


def entry(boxes, classes=None, areas=None, crowd=()):
    """A roidb entry of the fields the evaluation reads.  ``crowd``: rows whose gt_overlaps maximum is below 1 (no ground truth)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = len(boxes)
    classes = np.ones(n, np.int32) if classes is None else np.asarray(classes, np.int32)
    n_cls = int(classes.max()) + 1 if n else 2
    ov = np.zeros((n, max(n_cls, 2)), np.float32)
    ov[np.arange(n), classes] = 1.0
    for r in crowd:
        ov[r] = 0.5 * ov[r]
    e = {"boxes": boxes.astype(np.float32), "gt_classes": classes, "gt_overlaps": ov}
    if areas is not None:
        e["seg_areas"] = np.asarray(areas, np.float32)
    return e


def cover_plain(cand, gt):
    """The cover of one cell as the plain loop: the dense float64 overlap matrix (ground truths x candidates), per step the
    first maximum of what is still free.  -> (ov (m), cand (m), step (m)) at the ground truths' positions."""
    cand, gt = np.asarray(cand, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    m, k = len(gt), len(cand)
    ov, pick, step = np.zeros(m, np.float64), np.full(m, -1, np.int32), np.full(m, -1, np.int32)
    table = overlap_plus1(gt, cand)
    g_free, c_free = np.ones(m, bool), np.ones(k, bool)
    for t in range(m):
        rows, cols = np.flatnonzero(g_free), np.flatnonzero(c_free)
        if len(cols) == 0:
            for s, g in enumerate(rows):                 # no candidate left: misses in ascending position
                ov[g], pick[g], step[g] = 0.0, -1, t + s
            break
        sub = table[np.ix_(rows, cols)]
        r, c = np.unravel_index(np.argmax(sub), sub.shape)           # row-major first maximum: lowest row, then lowest column
        g, c = rows[r], cols[c]
        ov[g], pick[g], step[g] = sub.max(), c, t
        g_free[g], c_free[c] = False, False
    return ov, pick, step


def cover_cells_plain(pk):
    """``cover_plain`` on every (limit, area, image) cell of packed arrays -> the three (L, A, G) arrays."""
    L, A, G = len(pk.limits), len(pk.ranges), len(pk.gt_area)
    ov, cand, step = np.full((L, A, G), -1.0), np.full((L, A, G), -1, np.int32), np.full((L, A, G), -1, np.int32)
    for i in range(len(pk.cand_off) - 1):
        c0, c1, g0, g1 = pk.cand_off[i], pk.cand_off[i + 1], pk.gt_off[i], pk.gt_off[i + 1]
        for l in range(L):
            k = min(int(pk.limits[l]), c1 - c0)
            for a in range(A):
                rows = g0 + np.flatnonzero((pk.gt_area[g0:g1] >= pk.ranges[a, 0]) & (pk.gt_area[g0:g1] <= pk.ranges[a, 1]))
                ov[l, a, rows], cand[l, a, rows], step[l, a, rows] = cover_plain(pk.cand_box[c0:c0 + k], pk.gt_box[rows])
    return ov, cand, step


def random_boxes(rng, n, size, fractional, lo=4, hi=None):
    """n boxes inside a size x size canvas, widths and heights in [lo, hi]."""
    hi = size // 2 if hi is None else hi
    wh = rng.integers(lo, hi + 1, size=(n, 2)).astype(np.float64)
    xy = rng.integers(0, size - hi, size=(n, 2)).astype(np.float64)
    b = np.concatenate([xy, xy + wh - 1], 1)
    if fractional:
        b = b + np.round(rng.random((n, 4)), 3) * [0.0, 0.0, 1.0, 1.0]
    return b


def random_image(rng, n, m, size=600, fractional=False, duplicates=True, near=0.5):
    """(candidates (n, 4), roidb entry with m ground truths).  A share ``near`` of the candidates are jittered ground truths (so
    overlaps of every size occur), some are exact copies of a ground truth or of another candidate."""
    gt = random_boxes(rng, m, size, fractional, lo=8, hi=size // 2)
    cand = random_boxes(rng, n, size, fractional)
    if m and n:
        src = rng.integers(0, m, size=n)
        jit = rng.integers(-12, 13, size=(n, 4)).astype(np.float64)
        use = rng.random(n) < near
        cand[use] = gt[src[use]] + jit[use]
        cand[:, 2:] = np.maximum(cand[:, 2:], cand[:, :2])
        if duplicates:
            exact = rng.random(n) < 0.1
            cand[exact] = gt[src[exact]]
            twin = np.flatnonzero(rng.random(n) < 0.1)
            cand[twin] = cand[rng.integers(0, n, size=len(twin))]
    if duplicates and m > 1:
        twin = np.flatnonzero(rng.random(m) < 0.15)
        gt[twin] = gt[rng.integers(0, m, size=len(twin))]
    classes = rng.integers(1, 6, size=m).astype(np.int32)
    return cand, entry(gt, classes)


def random_batch(seed, counts, size=600, fractional=None, **kw):
    """``counts``: (n, m) per image.  fractional None: every other image has fractional coordinates."""
    rng = np.random.default_rng(seed)
    cands, roidb = [], []
    for i, (n, m) in enumerate(counts):
        c, e = random_image(rng, n, m, size, (i % 2 == 1) if fractional is None else fractional, **kw)
        cands.append(c)
        roidb.append(e)
    return cands, roidb


ALL_AREAS = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")


# ---- hand-worked cases: the overlaps are worked out by hand with the +1 convention (a box x1 y1 x2 y2 holds (x2 - x1 + 1) *
# (y2 - y1 + 1) pixels)


def hand_cases():
    """name -> (cand (k, 4), gt (m, 4), ov, cand index, step), written out."""
    c = {}
    # Two ground truths, three candidates; 10x10 boxes on one row, named by their left edge.  g0 at 0, g1 at 4.
    # Candidates at 3, 9, 30.  Overlap of two such boxes d pixels apart (d < 10): (10 - d) * 10 / (200 - (10 - d) * 10).
    #   g0: c0 (d 3) 70/130 = 7/13;  c1 (d 9) 10/190 = 1/19;  c2 none -> 0
    #   g1: c0 (d 1) 90/110 = 9/11;  c1 (d 5) 50/150 = 1/3;   c2 none -> 0
    # Per-column best: both g0 and g1 want c0.  Greedy: the largest entry is (g1, c0) = 9/11, step 0; g0 is left with c1 = 1/19.
    c["best_taken_first"] = (np.float64([[3, 0, 12, 9], [9, 0, 18, 9], [30, 0, 39, 9]]), np.float64([[0, 0, 9, 9], [4, 0, 13, 9]]),
                             [1.0 / 19.0, 9.0 / 11.0], [1, 0], [1, 0])
    # The same with the roles of the ground truths as the issue words it: the best candidate of g1 is taken by g0 first.
    #   g0 at 4, g1 at 0 -> (g0, c0) = 9/11 at step 0, g1 gets c1 = 1/19.
    c["g0_takes_g1s_best"] = (np.float64([[3, 0, 12, 9], [9, 0, 18, 9], [30, 0, 39, 9]]), np.float64([[4, 0, 13, 9], [0, 0, 9, 9]]),
                              [9.0 / 11.0, 1.0 / 19.0], [0, 1], [0, 1])
    # Duplicates: two equal ground truths, three equal candidates 5 pixels to the right (overlap 1/3 everywhere).  Ties go to the
    # lowest ground truth, then the lowest candidate: (g0, c0) at step 0, (g1, c1) at step 1.
    c["duplicates"] = (np.float64([[5, 0, 14, 9]] * 3), np.float64([[0, 0, 9, 9]] * 2), [1.0 / 3.0, 1.0 / 3.0], [0, 1], [0, 1])
    # g1 is touched by no candidate: step 0 is (g0, c1) = 1 (an exact copy); step 1 has only zeros left, the first of them is
    # (g1, c0): overlap 0 recorded, candidate 0 retired all the same.
    c["untouched"] = (np.float64([[2, 0, 11, 9], [0, 0, 9, 9], [1, 0, 10, 9]]), np.float64([[0, 0, 9, 9], [100, 100, 109, 109]]),
                      [1.0, 0.0], [1, 0], [0, 1])
    # No candidate touches anything: every overlap is 0, the steps go by position and retire candidates 0, 1.
    c["all_zero"] = (np.float64([[50, 50, 59, 59], [60, 60, 69, 69], [70, 70, 79, 79]]), np.float64([[0, 0, 9, 9], [20, 0, 29, 9]]),
                     [0.0, 0.0], [0, 1], [0, 1])
    # k < m: one candidate (g1's copy) for three ground truths.  Step 0: (g1, c0) = 1.  Then no candidate is left: g0 and g2 record
    # 0, -1 and the steps 1, 2 in ascending position.
    c["k_lt_m"] = (np.float64([[20, 0, 29, 9]]), np.float64([[0, 0, 9, 9], [20, 0, 29, 9], [40, 0, 49, 9]]),
                   [0.0, 1.0, 0.0], [-1, 0, -1], [1, 0, 2])
    # k == 0
    c["k_zero"] = (np.zeros((0, 4)), np.float64([[0, 0, 9, 9], [20, 0, 29, 9]]), [0.0, 0.0], [-1, -1], [0, 1])
    return c
