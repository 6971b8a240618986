"""Built cases of greedy NMS (i2v_nms_sorted: nms_mask_kernel and the three scan kernels of csrc/nms.hip), shared by the host test
and the GPU test, plus the two host helpers the cases are designed with.  Which regime a case lands in -- how many fixed-point
sweeps a 1024-row super-block needs, whether a pair lies inside the mask kernel's band around the threshold -- is decided here and
asserted on the CPU (tests/test_nms_cases_host.py); the GPU test only compares keep lists.  Everything is seeded numpy; nothing
here imports the package.

A case's ``dets`` are (n, 5) float32 rows [x1, y1, x2, y2, score] in strictly descending, tie-free score order (the score column
is not read by the kernel)."""
import collections

import numpy as np

F32 = np.float32
SUPER_ROWS = 1024                       # rows of a super-block of nms_scan_super_kernel
NMS_SWEEPS = 48                         # its default sweep cap (I2V_NMS_SCAN = 2); a value >= 3 of the key is the cap itself
BAND = 2.0 ** -21                       # nms_mask_kernel: thi / tlo = thresh (1 +- 2^-21)
THRESHOLDS = (0.7, 0.5, 0.3)
LADDER_THRESH = 0.7

# name, dets, thresh; T: the sweeps each super-block is built to need (None: not a ladder case); ladders: (first row, length);
# pairs: (row of the earlier member, row of the later one, family) for the threshold cases
Case = collections.namedtuple("Case", "name dets thresh T ladders pairs")


# ----------------------------------------------------------------------------------------------------------- helpers
def scores(n):
    """n strictly descending float32 scores in (0, 1): (n - i) / (n + 1), distinct for n < 2^23."""
    return (np.arange(n, 0, -1).astype(F32) / F32(n + 1)).astype(F32)


def with_scores(boxes):
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    return np.concatenate([boxes, scores(boxes.shape[0])[:, None]], 1).astype(F32)


def _terms(b, area, r0, r1, c0):
    """inter, d, ovr of rows r0..r1 against columns c0.. -- nms_cpu.py:20-29 as oracle_ops.c:59-64 states it, in float32, one
    rounding per operation, +1 extents; fmaxf / fminf return the other operand on a NaN (np.fmax / np.fmin)."""
    a, c = b[r0:r1, None, :], b[None, c0:, :]
    one, zero = F32(1), F32(0)
    w = np.fmax(zero, np.fmin(a[..., 2], c[..., 2]) - np.fmax(a[..., 0], c[..., 0]) + one)
    h = np.fmax(zero, np.fmin(a[..., 3], c[..., 3]) - np.fmax(a[..., 1], c[..., 1]) + one)
    inter = w * h
    d = area[r0:r1, None] + area[None, c0:] - inter
    ovr = inter / d
    assert inter.dtype == F32 and d.dtype == F32 and ovr.dtype == F32
    return inter, d, ovr


def suppression_matrix(dets, thresh, parts=True, chunk=512):
    """S[i, j] = row i suppresses row j when kept: ``!(ovr <= thresh)`` (nms_cpu.py:31 keeps ovr <= thresh; a NaN suppresses), strict
    upper triangle.  Returns (S, inter, d, ovr), all (n, n); ``parts=False``: S alone, built a block of rows at a time (large n)."""
    b = np.ascontiguousarray(np.asarray(dets, F32)[:, :4])
    n = b.shape[0]
    th = F32(thresh)
    with np.errstate(all="ignore"):
        area = (b[:, 2] - b[:, 0] + F32(1)) * (b[:, 3] - b[:, 1] + F32(1))
        if parts:
            inter, d, ovr = _terms(b, area, 0, n, 0)
            S = ~(ovr <= th) & np.triu(np.ones((n, n), bool), 1)
            return S, inter, d, ovr
        S = np.zeros((n, n), bool)
        for r0 in range(0, n, chunk):
            r1 = min(n, r0 + chunk)
            _, _, ovr = _terms(b, area, r0, r1, r0)
            blk = ~(ovr <= th)
            blk &= np.arange(r0, n)[None, :] > np.arange(r0, r1)[:, None]
            S[r0:r1, r0:] = blk
    return S


def greedy_keep(S):
    """nms_cpu.py:18-32 on the suppression matrix: rows in order, a kept row removes what it suppresses."""
    n = S.shape[0]
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if not dead[i]:
            keep.append(i)
            dead |= S[i]
    return np.asarray(keep, np.int32)


def sweeps_to_settle(S, super_rows=SUPER_ROWS):
    """The fixed-point resolve of nms_scan_super_kernel, per super-block: K_0 = alive, K_t = alive & ~OR_{j in K_(t-1)} S[j]; T is
    the first t with K_t == K_(t-1) (the kernel's sweep t - 1 is the first that changes nothing, so the super-block settles iff
    T <= fixed_point).  ``alive`` leaves out what the rows kept in earlier super-blocks removed.  Returns (T per super-block,
    keep rows)."""
    n = S.shape[0]
    removed = np.zeros(n, bool)
    T, keep = [], []
    for r0 in range(0, n, super_rows):
        r1 = min(n, r0 + super_rows)
        alive = ~removed[r0:r1]
        Sb = S[r0:r1, r0:r1]
        K, t = alive.copy(), 0
        while True:
            t += 1
            Kn = alive & ~Sb[K].any(0)
            if np.array_equal(Kn, K):
                break
            K = Kn
        T.append(t)
        kept = r0 + np.nonzero(K)[0]
        keep.append(kept)
        removed |= S[kept].any(0)
    return T, np.concatenate(keep).astype(np.int32) if keep else np.zeros(0, np.int32)


def band_constants(thresh):
    """thi, tlo as nms_mask_kernel forms them: float32 products of the float32 threshold."""
    th = F32(thresh)
    return th * F32(1.0 + BAND), th * F32(1.0 - BAND)


def band_class(inter, d, thresh):
    """The kernel's own two compares, in float32: +1 ``inter > thi d`` (suppressed without a division), -1 ``inter < tlo d``
    (kept without one), 0 neither: inside the band, decided by the division.  Arrays or scalars."""
    thi, tlo = band_constants(thresh)
    inter, d = np.asarray(inter, F32), np.asarray(d, F32)
    with np.errstate(all="ignore"):
        over, under = inter > thi * d, inter < tlo * d
    return np.where(over, 1, np.where(under, -1, 0))


def band_distance(inter, d, thresh):
    """inter / (thresh d) - 1 in units of the band's half-width 2^-21 (float64 of the float32 values): |.| <= 1 is about the band."""
    t = np.float64(F32(thresh))
    return (np.asarray(inter, np.float64) / (t * np.asarray(d, np.float64)) - 1.0) / BAND


def caps_for(case, keep):
    """max_keep values for a ladder case, from its greedy keep list: none (0), 1, the number kept in the first super-block and
    one to either side, and per ladder a cut that lands in its middle."""
    keep = np.asarray(keep)
    k1 = int((keep < SUPER_ROWS).sum())
    caps = {1, k1 - 1, k1, k1 + 1}
    for start, L in case.ladders:
        caps.add(int((keep < start + L // 2).sum()) + 1)
    return [0] + sorted(c for c in caps if c > 0)


# ----------------------------------------------------------------------------------------------------------- ladders
FILLER_Y, PAD_Y = 100000.0, 200000.0


def filler(n, y=FILLER_Y):
    """n 50 x 50 boxes 200 px apart on a far row: they overlap nothing, each other included."""
    x = 200.0 * np.arange(n)
    return np.stack([x, np.full(n, y), x + 49.0, np.full(n, y + 49.0)], 1).astype(F32)


def ladder(L, x0=0.0, y0=0.0):
    """L boxes of 101 x 101, each 10 px right of the one before.  At threshold 0.7 a box suppresses the next (IoU 91/111) and not
    the one after (81/121): greedy keeps every other box, and the fixed-point resolve needs L sweeps."""
    x = x0 + 10.0 * np.arange(L)
    return np.stack([x, np.full(L, y0), x + 100.0, np.full(L, y0 + 100.0)], 1).astype(F32)


def ladder_T(n, ladders):
    """The sweeps every super-block needs: the longest run of ladder rows in it, a run starting at the first alive one (a ladder's
    odd rows are suppressed; one that opens a super-block is gone before the resolve starts).  A super-block without a chain: 1."""
    T = []
    for r0 in range(0, n, SUPER_ROWS):
        r1 = min(n, r0 + SUPER_ROWS)
        t = 1
        for start, L in ladders:
            a, b = max(start, r0), min(start + L, r1)
            if a < b:
                t = max(t, b - a - ((a - start) & 1))
        T.append(t)
    return T


def ladder_case(name, n, ladders):
    """n rows of filler with ladders at the given (first row, length); every ladder on ground of its own."""
    boxes = filler(n)
    for k, (start, L) in enumerate(ladders):
        assert 0 <= start and start + L <= n
        boxes[start:start + L] = ladder(L, x0=20000.0 * k)
    assert np.abs(boxes).max() < 2 ** 24
    return Case(name, with_scores(boxes), LADDER_THRESH, ladder_T(n, ladders), tuple(ladders), None)


END_N = (1023, 1024, 1025, 2047, 2048, 2049, 12352, 12353)        # 12352: nblk - 1 = 192, the last n of the super-block scan


def ladder_cases():
    cases = []
    for L in (47, 48, 49):          # 48 sweeps: one to spare, settles on the last sweep, falls back to the serial resolve
        cases.append(ladder_case("cap48_L%d" % L, 300, [(30, L)]))
    for L in (4, 5, 6):             # the same three regimes under a cap of five sweeps
        cases.append(ladder_case("cap5_L%d" % L, 300, [(61, L)]))
    cases.append(ladder_case("whole_super_block", 2100, [(1024, 1024)]))
    cases.append(ladder_case("straddle", 2100, [(1000, 100)]))
    cases.append(ladder_case("three_regimes", 3000, [(100, 10), (1500, 60), (2500, 20)]))
    for n in END_N:                 # a ladder ending at the last row; 40 settles by default, 100 does not
        L = 40 if n < 2000 else 100
        cases.append(ladder_case("end_n%d" % n, n, [(n - L, L)]))
    return cases


def batched_case():
    """Three images in one launch, padded to one n: a ladder that settles, one that falls back, filler alone."""
    n = 1100
    imgs = []
    for k, (m, ladders) in enumerate([(700, [(50, 10)]), (1100, [(1000, 100)]), (900, [])]):
        c = ladder_case("batched%d" % k, m, ladders)
        boxes = np.concatenate([c.dets[:, :4], filler(n - m, PAD_Y)], 0)
        imgs.append(Case(c.name, with_scores(boxes), LADDER_THRESH, ladder_T(n, ladders), c.ladders, None))
    return imgs


def detection_ladder(R=128, L=60, C=4):
    """rois / cls_prob / bbox_pred for detection_postprocess: rois whose decode under zero deltas (width + 1: bbox_transform_inv's
    x2 = cx + w / 2) is a 60-row ladder plus filler, every class scoring the rois in strictly descending order.  Also returns the
    boxes the decode must give and (im_h, im_w)."""
    want = filler(R, 1000.0)
    want[10:10 + L] = ladder(L, x0=300.0, y0=200.0)
    rois = np.zeros((R, 5), F32)
    rois[:, 1:] = want - np.array([0, 0, 1, 1], F32)
    i = np.arange(R, dtype=np.float64)[:, None]
    j = np.arange(C, dtype=np.float64)[None, :]
    prob = ((R - i) * (j + 1.0) / ((R + 1.0) * (C + 1.0))).astype(F32)           # distinct within a class, all > 0
    assert (np.diff(prob, axis=0) < 0).all()
    pred = np.zeros((R, 4 * C), F32)
    return rois, prob, pred, want, (2000.0, 30000.0)


# ----------------------------------------------------------------------------------------------------------- threshold pairs
def _pair_decision(a, b, thresh):
    """One pair through the reference expression: (suppressed, inter, d, ovr)."""
    _, inter, d, ovr = suppression_matrix(np.stack([a, b]), thresh)
    return bool(~(ovr[0, 1] <= F32(thresh))), inter[0, 1], d[0, 1], ovr[0, 1]


def _bits(x):
    return int(np.asarray(x, F32).view(np.int32))


def _from_bits(i):
    return np.asarray(i, np.int32).view(F32)[()]


def exact_pairs(thresh, rng, y):
    """Family (a), every operation exact.  Boxes one pixel high sharing their left edge, wb near 9.5e6 (wa + wb < 2^24) and
    wa = round(thresh wb) + k, k = -8 .. 8: inter = wa, d = wb, ovr = fl(wa / wb) -- |k| <= 3 inside the band, the rest just
    outside.  Then small exact hits of fl(inter / d) == thresh: m (W, dx) wide boxes shifted by dx, (17, 3) -> 14/20,
    (3, 1) -> 2/4, (13, 7) -> 6/20.  Returns [(box, box, family)], y moving on by 3 px per pair so that pairs never meet."""
    out = []
    for wb in rng.integers(9000000, 9800000, 12):
        for k in range(-8, 9):
            wa = int(round(float(F32(thresh)) * int(wb))) + k
            out.append(([0, y[0], wa - 1, y[0]], [0, y[0], int(wb) - 1, y[0]], "a"))
            y[0] += 3
    W, dx = {0.7: (17, 3), 0.5: (3, 1), 0.3: (13, 7)}[thresh]
    for m in range(1, 13):
        h = int(rng.integers(1, 40))
        x = int(rng.integers(0, 500))
        out.append(([x, y[0], x + W * m - 1, y[0] + h - 1], [x + dx * m, y[0], x + dx * m + W * m - 1, y[0] + h - 1], "a"))
        y[0] += h + 2
    return out


N_BASE, N_LARGE = 256, 48


def rounded_pairs(thresh, rng, y):
    """Family (b), rounded arithmetic.  256 base boxes with arbitrary float32 x coordinates and sides 20 .. 900 (the last 48: x and
    the width 1e4 .. 1e5, 1000 .. 3600 high: areas beyond 2^24), the partner the same box moved right by s.  s = 0 suppresses, s = width
    does not; bisection over the bit pattern of s ends at two adjacent float32 shifts on which the reference decides
    differently, and both partners are kept, each with a copy of the base of its own.  y1 and the height are multiples of 1/4
    below 2^22, so that the copy moved down by whole pixels has the same heights and areas to the bit."""
    out = []
    for k in range(N_BASE):
        if k < N_BASE - N_LARGE:
            x1 = F32(rng.uniform(0.0, 1000.0))
            x2 = F32(x1 + F32(rng.uniform(20.0, 900.0)))
            h = int(rng.integers(80, 3601)) / 4.0
        else:
            x1 = F32(rng.uniform(1.0e4, 1.0e5))
            x2 = F32(x1 + F32(rng.uniform(2.0e4, 1.0e5)))
            h = int(rng.integers(4000, 14401)) / 4.0
        fy = int(rng.integers(0, 4)) / 4.0

        def pair(s, y1):
            return [x1, y1, x2, y1 + h - 1.0], [F32(x1 + s), y1, F32(x2 + s), y1 + h - 1.0]

        lo, hi = 0, _bits(x2 - x1 + F32(1))
        assert _pair_decision(*pair(_from_bits(lo), fy), thresh)[0] and not _pair_decision(*pair(_from_bits(hi), fy), thresh)[0]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _pair_decision(*pair(_from_bits(mid), fy), thresh)[0]:
                lo = mid
            else:
                hi = mid
        for s in (lo, hi):
            y1 = y[0] + fy
            assert y1 + h < 2 ** 22
            out.append(pair(_from_bits(s), y1) + ("b",))
            y[0] += int(h) + 4
    return out


def place_pairs(pairs, rng):
    """Rows for the pairs, behind one filler row: groups of 64 pairs, alternately at rows (r, r + 1) -- with the filler row in front
    that is (1, 2) .. (63, 64): inside a 64-column tile of the diagonal and across its edge -- and at (r, r + 64): the tile right
    of the diagonal.  Which member comes first alternates; the order of the pairs is shuffled so that the families mix."""
    order = rng.permutation(len(pairs))
    groups = (len(pairs) + 63) // 64
    n = 1 + 128 * groups
    boxes = np.stack([np.arange(n), -1000.0 - 3.0 * np.arange(n), np.arange(n), -1000.0 - 3.0 * np.arange(n)], 1).astype(F32)
    rows = []
    for q, p in enumerate(order):
        g, i = divmod(q, 64)
        ra, rb = (1 + 128 * g + 2 * i, 2 + 128 * g + 2 * i) if g % 2 == 0 else (1 + 128 * g + i, 65 + 128 * g + i)
        a, b, fam = pairs[p]
        if q % 2:
            a, b = b, a
        boxes[ra], boxes[rb] = np.asarray(a, F32), np.asarray(b, F32)
        rows.append((ra, rb, fam))
    return boxes, rows


def threshold_case(thresh):
    rng = np.random.default_rng(9100 + int(round(thresh * 10)))
    y = [0]
    pairs = exact_pairs(thresh, rng, y) + rounded_pairs(thresh, rng, y)
    boxes, rows = place_pairs(pairs, rng)
    assert np.abs(boxes).max() < 2 ** 24
    return Case("thresh%02d" % int(round(thresh * 10)), with_scores(boxes), thresh, None, (), tuple(rows))


# ----------------------------------------------------------------------------------------------------------- degenerate boxes
def _ordinary(rng, n):
    """Loosely clustered ordinary boxes in a 1000 x 600 frame, so that the NMS around the degenerate ones has work to do."""
    k = max(1, n // 6)
    c = np.concatenate([rng.uniform(0, 800, (k, 1)), rng.uniform(0, 450, (k, 1))], 1)
    wh = rng.uniform(30, 180, (k, 2))
    pick = rng.integers(0, k, n)
    b = np.concatenate([c[pick], c[pick] + wh[pick]], 1) + rng.normal(0, 5.0, (n, 4))
    return b.astype(F32)


def degenerate_cases():
    """Ordinary boxes with degenerate ones among them (the mask kernel sends a row or a column with a non-positive side or a NaN
    through the division as a whole); the answer is the oracle's, whatever it is.  ``nan_first``: a NaN row alive (row 0);
    ``mixed``: everything else, the NaN box in mid-list where it is a column of the rows before it."""
    rng = np.random.default_rng(9200)
    n = 200
    inf, nan = np.inf, np.nan
    special = [
        [100, 100, 99, 150], [100, 100, 99, 150],           # zero area (x2 == x1 - 1), twice the same: 0 / 0
        [300, 200, 360, 199],                               # zero area through the height, inside ordinary boxes
        [400, 100, 400 - 51, 149],                          # width -50, height 50: area -2500 ...
        [400, 300, 449, 349],                               # ... against area +2500: d == 0 with inter == 0
        [500, 100, 500 - 101, 149],                         # area -5000 against the same +2500: d < 0, 0 / negative = -0
        [600, 400, 600 - 31, 400 - 21],                     # both sides negative: area +600
        [600, 400, 600 - 31, 400 - 21],
        [50.5, 60.25, 50.0, 200.0],                         # width 0.5: positive, stays on the fast path
        [0, 0, inf, 50], [10, 10, inf, 40],                 # +inf extents: inf against inf, inf against finite
        [200, 500, 260, inf], [700, 0, inf, 20],            # ... and inf * 0
        [150, 150, 250, nan],                               # a NaN coordinate
        [-inf, 0, 5, 5],
    ]
    with np.errstate(all="ignore"):
        special = np.asarray(special, F32)
    boxes = _ordinary(rng, n)
    at = rng.choice(np.setdiff1d(np.arange(1, n), [63, 64]), len(special), replace=False)
    boxes[at] = special
    boxes[63] = [boxes[3, 0], boxes[3, 1], boxes[3, 0] - 1, boxes[3, 3]]      # one degenerate box on each side of a tile edge:
    boxes[64] = [boxes[5, 2], boxes[5, 3], boxes[5, 0], boxes[5, 1]]          # zero area on row 3's edge; row 5 inside out
    mixed = Case("mixed", with_scores(boxes), 0.7, None, (), None)
    b2 = _ordinary(rng, 130)
    b2[0] = [nan, 10, 60, 80]
    nan_first = Case("nan_first", with_scores(b2), 0.7, None, (), None)
    b3 = _ordinary(rng, 130)
    b3[70] = [20, nan, 90, 100]                             # a NaN column in the second tile, no other degenerate box around
    nan_column = Case("nan_column", with_scores(b3), 0.3, None, (), None)
    return [mixed, nan_first, nan_column]
