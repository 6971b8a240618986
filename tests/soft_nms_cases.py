"""Built cases of Soft-NMS (i2vsgg_amd/soft_nms.py: the rules and the host form; csrc/soft_nms.hip: the kernel), shared by the
host test and the GPU test.  Seeded numpy on top of tests/nms_cases.py (its filler, ladder, clustered and degenerate boxes).

A case is one set: ``count`` rows [x1, y1, x2, y2, score] in descending score order, built for a capacity ``n`` and a method.
Families:

``random``      clustered ordinary boxes
``threshold``   pairs whose float32 IoU is exactly Nt, one ulp above and one ulp below it (hard and linear decide with a strict >)
``equal``       scores in groups of four equal values
``stack``       identical boxes: every pick decays every other row
``degenerate``  zero-area boxes (``nms_cases.degenerate_cases``, its finite rows of non-negative extent) among ordinary ones
``ladder``      a chain of overlapping boxes at neighbouring scores: each pick's decay changes which row is picked next

hard and linear are compared bit for bit, so any case serves them and every row takes part.  gaussian is compared in order only
where the host form's own decisions keep the margin of soft_nms.py ("Exactness": n * 2^-22); scores that random decays have
moved crowd closer than that when many rows overlap, so a gaussian case keeps the overlapping rows few (ACTIVE) among filler that
overlaps nothing, and the generator walks its seed until the host form reports both gaps above the margin.  The host test
asserts the margin of every gaussian case again."""
import collections
import functools

import numpy as np

import nms_cases as nc
from i2vsgg_amd import soft_nms as sn

F32 = np.float32
NT = 0.3                                     # cfg.TEST.NMS
SIGMA, MIN_SCORE = 0.5, 0.001
FAMILIES = ("random", "threshold", "equal", "stack", "degenerate", "ladder")
SIZES = (1, 2, 63, 64, 65, 128, 300, 1025)   # lane and wave edges, the test loop's own size, one past a 1024 boundary
MAX_TRIES = 60

Case = collections.namedtuple("Case", "family n method rows out src num decays stats")


def active_budget(n, method):
    """Rows of a case that may overlap another row."""
    if method != "gaussian":
        return n
    return 40 if n <= 512 else 16


def _scores(rng, count, ties=False):
    """count descending float32 scores, log-uniform in [0.01, 0.99]; ``ties``: groups of four equal values."""
    k = (count + 3) // 4 if ties else count
    while True:
        s = np.unique(np.exp(rng.uniform(np.log(0.01), np.log(0.99), k)).astype(F32))
        if len(s) == k:
            break
    s = s[::-1]
    return np.repeat(s, 4)[:count].copy() if ties else s.copy()


@functools.lru_cache(maxsize=None)
def threshold_pairs():
    """[(wa, wb, which)]: boxes one pixel high sharing their left edge, wa and wb pixels wide, wa + wb < 2^24, so inter = wa and
    d = wb exactly and the IoU is fl(wa / wb): == Nt (which 0), its float32 successor (+1), its predecessor (-1)."""
    t0 = F32(NT)
    out = []
    wb = np.arange(6000000, 6004000)
    for which, t in ((0, t0), (1, np.nextafter(t0, F32(1))), (-1, np.nextafter(t0, F32(0)))):
        wa = np.rint(np.float64(t) * wb).astype(np.int64)
        hit = np.nonzero((wa.astype(F32) / wb.astype(F32)) == t)[0]
        assert len(hit) >= 40, (which, len(hit))
        out.append([(int(wa[i]), int(wb[i]), which) for i in hit[:200]])
    return [p for trio in zip(*out) for p in trio]


@functools.lru_cache(maxsize=None)
def _degenerate_boxes():
    """(the zero-area rows, the ordinary rows) of nms_cases' ``mixed`` case that are finite with non-negative extents."""
    b = nc.degenerate_cases()[0].dets[:, :4]
    with np.errstate(all="ignore"):
        w, h = b[:, 2] - b[:, 0] + F32(1), b[:, 3] - b[:, 1] + F32(1)
        ok = np.isfinite(b).all(1) & (w >= 0) & (h >= 0)
    zero = ok & ((w == 0) | (h == 0))
    assert zero.sum() >= 4
    return b[zero], b[ok & ~zero]


def _active_boxes(family, count, budget, rng):
    """(boxes of the rows that overlap, keep_together): in the order they take in the set."""
    k = min(count, budget)
    if family == "random" or family == "equal":
        return nc._ordinary(rng, k), False
    if family == "stack":
        return np.tile(np.array([[100.0, 50.0, 260.0, 170.0]], F32), (k, 1)), False
    if family == "ladder":
        return nc.ladder(min(k, 60), x0=300.0, y0=200.0), True
    if family == "degenerate":
        zero, ordinary = _degenerate_boxes()
        nz = min(len(zero), max(k // 3, min(k, 2)))
        rest = ordinary[rng.permutation(len(ordinary))[:max(k - nz, 0)]]
        b = np.concatenate([zero[:nz], rest], 0)
        return b[rng.permutation(len(b))], False
    if family == "threshold":
        pairs = threshold_pairs()
        b = []
        for j in range(k // 2):
            wa, wb, _ = pairs[j % len(pairs)]
            y = 10.0 * j
            first, second = [0, y, wa - 1, y], [0, y, wb - 1, y]
            b += [first, second] if j % 2 == 0 else [second, first]
        return np.asarray(b, F32).reshape(-1, 4), True
    raise KeyError(family)


def build_rows(family, count, budget, seed):
    """count rows of the family: the active boxes at rows of their own among nms_cases' filler (which overlaps nothing)."""
    rng = np.random.default_rng(seed)
    boxes = nc.filler(count)
    if count:
        act, together = _active_boxes(family, count, count if family == "stack" else budget, rng)
        k = len(act)
        if together:                        # neighbours in score order
            at = int(rng.integers(0, count - k + 1)) + np.arange(k)
        else:
            at = np.sort(rng.choice(count, k, replace=False))
        boxes[at] = act
    rows = np.concatenate([boxes, _scores(rng, count, ties=family == "equal")[:, None]], 1).astype(F32)
    assert np.isfinite(rows).all() and (np.diff(rows[:, 4]) <= 0).all()
    return rows


def fit(stats, n):
    return min(stats.get("pick_gap", np.inf), stats.get("min_score_gap", np.inf)) > sn.margin(n)


@functools.lru_cache(maxsize=None)
def case(family, n, count, method):
    """The case and the host form's answer for it, computed once.  gaussian: the first seed whose decisions keep the margin."""
    base = 7000 + 131 * FAMILIES.index(family) + 17 * n + count
    for k in range(MAX_TRIES):
        rows = build_rows(family, count, active_budget(n, method), base + 100000 * k)
        stats = {}
        out, src, num = sn.soft_nms_host(rows, None, method, NT, SIGMA, MIN_SCORE, stats)
        if method != "gaussian" or fit(stats, n):
            break
    else:
        raise AssertionError("no seed of %s n=%d count=%d keeps the gaussian margin" % (family, n, count))
    decays = stats.pop("decays")[0]
    for a in (rows, out, src, num, decays):
        a.setflags(write=False)
    return Case(family, n, method, rows, out[0, :num[0]], src[0, :num[0]], int(num[0]), decays, stats)


BANDS = (0.6, 0.3, 0.05)                    # banded_gaussian_case: where the filler's scores sit
BAND_WIDTH = 1.0e-3                          # relative


@functools.lru_cache(maxsize=None)
def banded_gaussian_case(n=4096, active=24):
    """gaussian at the capacity (16 waves, four rows per lane), every row valid.  At n = 4096 the margin is 2^-10, which random
    scores of thousands of rows cannot keep once decays move them.  So the filler -- rows that overlap nothing, hence only ever
    decayed with weight 1, their bits the host's -- has its scores packed into three narrow bands (relative width 1e-3 at 0.6, 0.3
    and 0.05: a third of the filler each, distinct float32 values), and ``active`` clustered boxes that do decay one another start
    away from the bands: they take the first rows, rows between the bands and the last rows.  The seed walks until the host form
    reports the margin, that is, until no decayed score comes to rest within 2^-10 of a band, of another decayed score or of
    min_score at a decision."""
    base = 9400
    n_fill = n - active
    for k in range(MAX_TRIES):
        rng = np.random.default_rng(base + k)
        per = [n_fill // 3, n_fill // 3, n_fill - 2 * (n_fill // 3)]
        fill = []
        for c, m in zip(BANDS, per):
            lo = np.float32(c)
            v = np.unique(rng.uniform(float(lo), float(lo) * (1.0 + BAND_WIDTH), 2 * m).astype(F32))
            fill.append(rng.permutation(v)[:m])
        fill = np.concatenate(fill)
        assert len(np.unique(fill)) == n_fill
        act = np.exp(rng.uniform(np.log(0.02), np.log(0.99), active)).astype(F32)
        near = np.abs(act[:, None] / np.asarray(BANDS, F32)[None, :] - 1.0).min(1) < 0.02
        if near.any():
            continue
        score = np.concatenate([fill, act])
        boxes = np.concatenate([nc.filler(n_fill), nc._ordinary(rng, active)], 0)
        order = np.argsort(-score, kind="stable")
        rows = np.concatenate([boxes[order], score[order][:, None]], 1).astype(F32)
        stats = {}
        out, src, num = sn.soft_nms_host(rows, None, "gaussian", NT, SIGMA, MIN_SCORE, stats)
        if fit(stats, n):
            break
    else:
        raise AssertionError("no seed of the banded case keeps the gaussian margin")
    decays = stats.pop("decays")[0]
    for a in (rows, out, src, num, decays):
        a.setflags(write=False)
    return Case("banded", n, "gaussian", rows, out[0, :num[0]], src[0, :num[0]], int(num[0]), decays, stats)


def batches(n, method):
    """The calls of one (n, method): three sets of different counts each (n, 2n / 3, n / 3), every family at every level."""
    levels = (n, (2 * n) // 3, n // 3)
    out = []
    for trio in (FAMILIES[:3], FAMILIES[3:]):
        for r in range(3):
            out.append([case(f, n, levels[(i + r) % 3], method) for i, f in enumerate(trio)])
    return out


def pack(cases, n):
    """dets (3, n, 5) and counts (3,) of one call; rows past a set's count hold a live-looking decoy that must be ignored."""
    dets = np.zeros((len(cases), n, 5), F32)
    dets[:, :, :] = np.array([0.0, 0.0, 500.0, 500.0, 0.999], F32)
    counts = np.zeros(len(cases), np.int32)
    for i, c in enumerate(cases):
        dets[i, :len(c.rows)] = c.rows
        counts[i] = len(c.rows)
    return dets, counts
