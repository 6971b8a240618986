"""Built cases of box voting (i2vsgg_amd/box_vote.py: the rules and the host form), for the host test and for the test of a
device form (the kernel is not in the library yet).  Seeded numpy on top of tests/nms_cases.py (its filler) and tests/soft_nms_cases.py (its scores).

A case is one set: ``kept`` rows and ``cands`` rows [x1, y1, x2, y2, score], the candidates in descending score order with
strictly positive scores, every coordinate a non-negative finite float32, and the host form's answer for them.  Families:

``clustered``     candidates jittered around a few objects, plus filler that overlaps nothing; kept = what the greedy NMS keeps
``threshold``     the pairs whose float32 IoU is exactly float32(0.8) (they vote under >=), 0.81 (votes) and 0.72 (does not);
                  also run at vote_thresh = nextafter(0.8f, 1), where the exact pairs stop voting
``clustered2``    every candidate jittered around an object, more loosely
``stack``         identical boxes with different scores: the voted box is that box, exactly
``degenerate``    zero-area kept boxes among zero-area candidates (0 / 0: no voter, the bits stay) and ordinary ones
``self``          boxes that overlap nothing: each kept row's only voter is itself, and its bits stay; 100 kept rows, more than
                  one pass of a one-wave-per-row launch covers
``large``         coordinates around 4000 px, scores of 1e-3 beside scores near 1
``crowd``         every candidate within a few pixels of one box: more than half of them vote for each kept row"""
import collections
import functools

import numpy as np

import nms_cases as nc
import soft_nms_cases as sc
from i2vsgg_amd import box_vote as bv
from i2vsgg_amd import soft_nms as sn

F32 = np.float32
T = 0.8                                                     # Detectron's VOTE_TH
T_UP = float(np.nextafter(F32(0.8), F32(1)))
FAMILIES = ("clustered", "threshold", "stack", "degenerate", "self", "large", "crowd", "clustered2")
# the calls of a candidate capacity: three families and the vote_thresh their three sets share
TRIOS = ((("clustered", "degenerate", "clustered2"), T), (("threshold", "self", "stack"), T), (("threshold", "large", "crowd"), T_UP),
         (("large", "crowd", "stack"), T))
SIZES = (1, 2, 63, 64, 65, 128, 300, 1025, 4096)            # lane and wave edges, the test loop's own size, 1024 + 1, the capacity
KEPT_MAX = 100                                              # kept rows of a case at most
DECOY = np.array([0.0, 0.0, 500.0, 500.0, 0.999], F32)      # behind the counts: must never be read

# (kept box, candidate, float32 IoU as a fraction, votes at T, votes at T_UP); checked with soft_nms.iou_row in the host test
PAIRS = (
    ([0, 0, 9, 9], [0, 0, 9, 7], (80, 100), True, False),                 # exactly float32(0.8)
    ([100, 50, 199, 149], [100, 50, 199, 129], (8000, 10000), True, False),
    ([3, 3, 7, 7], [3, 3, 7, 6], (20, 25), True, False),
    ([0, 0, 9, 9], [0, 0, 8, 8], (81, 100), True, True),
    ([0, 0, 9, 9], [0, 0, 8, 7], (72, 100), False, False),
)

Case = collections.namedtuple("Case", "family thresh kept cands want voters")


def ulps(a, b):
    """|a - b| in float32 ulps, element by element (finite values; -0 and +0 are 0 apart)."""
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _rows(boxes, scores):
    return np.concatenate([np.asarray(boxes, F32).reshape(-1, 4), np.asarray(scores, F32).reshape(-1, 1)], 1).astype(F32)


def _objects(rng, count, n_obj, jitter):
    """count boxes jittered around n_obj objects in a 1000 x 600 frame, clipped at 0."""
    c = rng.uniform([20, 20], [700, 350], (n_obj, 2))
    wh = rng.uniform(60, 260, (n_obj, 2))
    pick = rng.integers(0, n_obj, count)
    b = np.concatenate([c[pick], c[pick] + wh[pick]], 1) + rng.normal(0, jitter, (count, 4))
    return np.maximum(b, 0).astype(F32)


def build(family, count, seed):
    """(kept (k, 5), cands (count, 5)) of the family for ``count`` candidates.  No candidate: two kept rows that find no voter,
    or (``self``) no kept row either."""
    rng = np.random.default_rng(seed)
    if count == 0:
        return _rows(nc.filler(0 if family == "self" else 2), [0.5, 0.4][:0 if family == "self" else 2]), np.zeros((0, 5), F32)
    scores = sc._scores(rng, count)
    boxes = nc.filler(count)
    if family in ("clustered", "clustered2"):
        k = (count + 1) // 2 if family == "clustered" else count
        at = np.sort(rng.choice(count, k, replace=False))
        boxes[at] = _objects(rng, k, max(1, min(8, k // 10)), 4.0 if family == "clustered" else 8.0)
        cands = _rows(boxes, scores)
        out, _, num = sn.soft_nms_host(cands, None, "hard", 0.3)
        return out[0, :min(int(num[0]), KEPT_MAX)].copy(), cands
    if family == "threshold":
        kept_at = []
        for j in range(min(count // 2, 40)):                # pair j: the kept box, then its partner, 1000 px from the pair before
            a, b = PAIRS[j % len(PAIRS)][:2]
            shift = np.array([1000.0 * j, 0, 1000.0 * j, 0], F32)
            boxes[2 * j], boxes[2 * j + 1] = np.asarray(a, F32) + shift, np.asarray(b, F32) + shift
            kept_at.append(2 * j)
        cands = _rows(boxes, scores)
        return cands[kept_at or [0]].copy(), cands
    if family == "stack":
        boxes[:] = [100.0, 50.0, 260.0, 170.0]
        cands = _rows(boxes, scores)
        return cands[sorted({0, count // 2, count - 1})].copy(), cands
    if family == "degenerate":
        special = np.array([[100, 100, 99, 150], [100, 100, 99, 150], [300, 200, 360, 199], [40, 40, 40, 39]], F32)[:count]
        k = len(special)
        rest = min(count - k, 30)
        at = np.sort(rng.choice(count, k + rest, replace=False))
        perm = rng.permutation(k + rest)
        boxes[at[perm[:k]]] = special
        boxes[at[perm[k:]]] = _objects(rng, rest, 2, 3.0) + F32(250)         # ordinary boxes around the zero-area ones
        cands = _rows(boxes, scores)
        return cands[np.sort(at[perm[:k + min(rest, 4)]])].copy(), cands
    if family == "self":
        cands = _rows(boxes, scores)
        return cands[:KEPT_MAX].copy(), cands
    if family == "large":
        k = min(count, 64)
        at = np.sort(rng.choice(count, k, replace=False))
        boxes[at] = np.array([3800.0, 3900.0, 4090.0, 4095.0], F32) + rng.integers(-2, 3, (k, 4)).astype(F32)
        s = np.where(rng.random(count) < 0.5, rng.uniform(0.001, 0.002, count), rng.uniform(0.9, 0.999, count))
        cands = _rows(boxes, np.sort(s.astype(F32))[::-1])
        return cands[at[sorted({0, k // 2, k - 1})]].copy(), cands
    if family == "crowd":
        boxes = np.array([100.0, 50.0, 300.0, 200.0], F32) + rng.integers(-3, 4, (count, 4)).astype(F32) + rng.random((count, 4)).astype(F32)
        cands = _rows(boxes, scores)
        return cands[sorted({0, count // 3, count - 1})].copy(), cands
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def case(family, count, thresh=T):
    """The case and the host form's answer for it at ``thresh``, computed once and left unchanged."""
    kept, cands = build(family, count, 8100 + 97 * FAMILIES.index(family) + count)
    assert np.isfinite(cands).all() and (cands[:, :4] >= 0).all() and (cands[:, 4] > 0).all() and (np.diff(cands[:, 4]) <= 0).all()
    stats = {}
    want = bv.box_vote_host(kept, None, cands, None, thresh, stats)[0]
    voters = stats["voters"][0]
    for a in (kept, cands, want, voters):
        a.setflags(write=False)
    return Case(family, thresh, kept, cands, want, voters)


def batches(n):
    """The sets of one candidate capacity n, three per call of a batched form, as (vote_thresh, [three cases]): sets of n, 2n / 3 and n / 3 candidates, every
    family of a trio at every level."""
    levels = (n, (2 * n) // 3, n // 3)
    out = []
    for trio, thresh in TRIOS:
        for r in range(3):
            out.append((thresh, [case(f, levels[(i + r) % 3], thresh) for i, f in enumerate(trio)]))
    return out


def pack(cases, n):
    """kept (3, n_kept, 5), kept_counts, cands (3, n, 5), cand_counts of one call; rows past a count hold a decoy that would
    vote for, or be voted on by, everything near the origin if it were read."""
    n_kept = max(1, max(len(c.kept) for c in cases))
    kept = np.tile(DECOY, (len(cases), n_kept, 1))
    cands = np.tile(DECOY, (len(cases), max(n, 1), 1))
    kc, cc = np.zeros(len(cases), np.int32), np.zeros(len(cases), np.int32)
    for i, c in enumerate(cases):
        kept[i, :len(c.kept)], cands[i, :len(c.cands)] = c.kept, c.cands
        kc[i], cc[i] = len(c.kept), len(c.cands)
    return kept, kc, cands, cc
