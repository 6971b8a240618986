"""Seeded case sets for predicate recognition (i2vsgg_amd.recognition), shared by tests/test_recognition_host.py,
tests/test_gpu_recognition.py and tools/gen_golden.py (``gen_recognition``).

A video is a list of segment specs; every segment is one ordered track pair with one duration and one or two predicates.  The
rows of a segment are drawn together, so that a segment in which two of the 11 largest means of a column group are equal can be
drawn again (``np.argsort(-x)`` leaves the order of equal values open, so such a segment cannot be compared with the
reference); the set counts its draws and its re-draws.  Planted ties are exempt: they are compared with the host form only."""
import numpy as np

TOP = 10


def names(C, R):
    return ["__background__"] + ["class%d" % c for c in range(1, C)], ["pred%d" % r for r in range(R)]


def segment_mean(rows):
    """One add per row and column in row order, one division: the rule of recognition.align_arrays_host."""
    acc = rows[0].astype(np.float64)
    for r in rows[1:]:
        acc = acc + r.astype(np.float64)
    return acc / np.float64(len(rows))


def has_tie(mean, C, R):
    """Two of the 11 largest means of a group are equal (then the first 10 of a ranking are not well defined)."""
    for off, width in ((0, C), (C, C), (2 * C, R)):
        big = np.sort(mean[off:off + width])[::-1][:TOP + 1]
        if len(np.unique(big)) != len(big):
            return True
    return False


def draw_rows(rng, n, C, R, ls, lp, lo):
    """(n, 2C+R) float32 rows: class probabilities with column 0 zero and some mass on the true class, predicate scores as
    a probability plus a log prior (negative, a few units wide), some mass on the true predicate."""
    def probs(width, true, boost):
        z = rng.standard_normal((n, width)).astype(np.float32)
        z[:, true] += np.float32(boost)
        e = np.exp(z - z.max(1, keepdims=True))
        return (e / e.sum(1, keepdims=True)).astype(np.float32)
    sub, obj = probs(C, ls, 1.5), probs(C, lo, 1.0)
    sub[:, 0] = 0.0
    obj[:, 0] = 0.0
    pre = (probs(R, lp, 4.0).astype(np.float64) + np.log(0.5 * (rng.uniform(0.2, 0.8, (n, R)) + 1.0 / 15))).astype(np.float32)
    return np.hstack([sub, obj, pre])


def build(seed, C, R, videos, ties=None, check_ties=True):
    """``videos``: {vid: {"n_frames", "dropped": frames recorded as {}, "missing": frames without a key, "segments": [(stid,
    otid, start, end, omitted frames, n_predicates)], "twice": [(segment index, frame)] -- the pair is listed a second time in
    that frame, with other scores}}.  ``ties``: {(vid, segment index): [(group 0..2, columns, value)]} -- those columns hold
    ``value`` in every row of the segment.  -> dict(frame_recognitions, groundtruth, classes, predicates, draws, redraws,
    row_counts {(vid, segment index): rows}).  Every second video has its frame numbers as strings, as JSON returns them."""
    rng = np.random.default_rng(seed)
    classes, predicates = names(C, R)
    ties = ties or {}
    fr, gt, row_counts = {}, {}, {}
    draws = redraws = 0
    for v, (vid, spec) in enumerate(videos.items()):
        nf = spec["n_frames"]
        dropped, missing = set(spec.get("dropped", ())), set(spec.get("missing", ()))
        per_frame = dict((f, []) for f in range(nf) if f not in dropped and f not in missing)
        gt[vid] = []
        for k, (stid, otid, start, end, omitted, n_pred) in enumerate(spec["segments"]):
            ls, lo = int(rng.integers(1, C)) if C > 1 else 0, int(rng.integers(1, C)) if C > 1 else 0
            lps = [int(p) for p in rng.choice(R, size=min(n_pred, R), replace=False)]
            present = [f for f in range(start, end) if f in per_frame and f not in omitted]
            row_counts[(vid, k)] = len(present)
            if present:
                while True:
                    rows = draw_rows(rng, len(present), C, R, ls, lps[0], lo)
                    for g, cols, value in ties.get((vid, k), ()):
                        rows[:, [(0, C, 2 * C)[g] + c for c in cols]] = np.float32(value)
                    draws += 1
                    if (vid, k) in ties or not check_ties or not has_tie(segment_mean(rows), C, R):
                        break
                    redraws += 1
                for f, row in zip(present, rows):
                    per_frame[f].append(([stid, otid], row))
            for f in [f for s, f in spec.get("twice", ()) if s == k]:
                per_frame[f].append(([stid, otid], draw_rows(rng, 1, C, R, ls, lps[0], lo)[0]))     # never the first occurrence
            for i, lp in enumerate(lps):
                # names and integer labels both occur; extra keys are ignored
                trip = [classes[ls], predicates[lp], classes[lo]] if (k + i) % 3 else [ls, lp, lo]
                gt[vid].append({"triplet": trip, "subject_tid": stid, "object_tid": otid, "duration": [start, end],
                                "sub_traj": [], "obj_traj": []})
        fr[vid] = {}
        string_keys = v % 2 == 1                                   # frame numbers as JSON returns them
        for f in range(nf):
            if f in missing:
                continue
            key = str(f) if string_keys else f
            entries = per_frame.get(f, [])
            if f in dropped or not entries:
                fr[vid][key] = {}
                continue
            first = [e for i, e in enumerate(entries) if e[0] not in [x[0] for x in entries[:i]]]
            later = [e for i, e in enumerate(entries) if e[0] in [x[0] for x in entries[:i]]]
            order = [first[i] for i in rng.permutation(len(first))] + later
            rows = np.stack([e[1] for e in order])
            fr[vid][key] = {"sub_scores": rows[:, :C].copy(), "obj_scores": rows[:, C:2 * C].copy(),
                            "pre_scores": rows[:, 2 * C:].copy(), "tids": [list(e[0]) for e in order]}
    return {"frame_recognitions": fr, "groundtruth": gt, "classes": classes, "predicates": predicates, "draws": draws,
            "redraws": redraws, "row_counts": row_counts}


def random_videos(seed, n_videos, n_frames=24, n_tracks=5, n_segments=12):
    """Video specs with skipped, dropped and missing frames, segments without rows and doubled pairs."""
    rng = np.random.default_rng(seed)
    out = {}
    for v in range(n_videos):
        pairs = [(s, o) for s in range(n_tracks) for o in range(n_tracks) if s != o]
        chosen = [pairs[i] for i in rng.permutation(len(pairs))[:n_segments]]
        dropped = set(int(f) for f in rng.choice(n_frames, 2, replace=False))
        missing = set(int(f) for f in rng.choice(n_frames, 2, replace=False)) - dropped
        segs, twice = [], []
        for k, (s, o) in enumerate(chosen):
            start = int(rng.integers(0, n_frames - 1))
            end = int(rng.integers(start + 1, n_frames + 3))             # a duration may run past the last frame
            omitted = set(int(f) for f in range(start, end) if rng.random() < 0.15)
            if k % 7 == 5:
                omitted = set(range(start, end))                         # a segment without rows
            elif k % 5 == 2:
                free = [f for f in range(start, min(end, n_frames)) if f not in omitted | dropped | missing]
                if free:
                    twice.append((k, free[0]))
            segs.append((s, o, start, end, omitted, 2 if k % 4 == 1 else 1))
        out["vid%03d" % v] = {"n_frames": n_frames, "dropped": dropped, "missing": missing, "segments": segs, "twice": twice}
    return out


def golden_set():
    """The set behind tests/golden/recognition.npz: 30 videos x 12 segments at C = 16, R = 62, no planted ties."""
    return build(7301, 16, 62, random_videos(7302, 30))


def edge_videos():
    """Segments of 1, 2, 63, 64, 65 and 300 rows, with a skipped frame inside the longer ones, an empty segment, a doubled
    pair and a missing frame."""
    segs, start = [], 0
    for k, n in enumerate((1, 2, 63, 64, 65, 300)):
        skip = {start + n // 2} if n > 2 else set()                      # one frame without the pair: duration n + 1
        end = start + n + len(skip)
        segs.append((2 * k, 2 * k + 1, start, end, skip, 2 if k == 3 else 1))
        start = end
    segs.append((20, 21, 0, 40, set(range(0, 40)), 1))                   # no rows at all
    segs.append((22, 23, 500, 520, set(), 1))                            # a duration past the video: no rows
    n_frames = start + 2
    return {"edges": {"n_frames": n_frames, "dropped": set(), "missing": {n_frames - 1}, "segments": segs,
                      "twice": [(2, segs[2][2]), (5, segs[5][2] + 7)]}}


def device_set(C, R, seed=7400):
    """The GPU case set at (C, R): the edge video, 25 random videos (more than 256 segments in all) and planted equal means:
    two equal maxima, and equal values inside the top 10 (inside the top 5 for the classes)."""
    videos = edge_videos()
    videos.update(random_videos(seed + 1, 25))
    hi = lambda w: [c for c in (1, w - 1) if 0 <= c < w]                 # two columns where the group has two
    ties = {("edges", 0): [(0, hi(C), 0.9375), (2, hi(R), 0.5)],        # one row: two equal maxima in sub and pre
            ("edges", 3): [(1, hi(C), 0.96875)],                         # 64 rows, two predicates: equal maxima in obj
            ("vid000", 0): [(2, [c for c in (0, 3, 5, 9) if c < R], -0.25)],
            ("vid001", 1): [(0, [c for c in (2, 4, 6) if c < C], 0.03125), (1, [c for c in (1, 2) if c < C], 2.0 ** -20)]}
    return build(seed, C, R, videos, ties=ties)


def hand_case():
    """The hand-worked case of tests/test_recognition_host.py: C = 3, R = 6; two videos, three segments; the pair (1, 2) of
    video "a" carries two predicates; frame 1 of "a" lacks the pair; the segment of video "b" has no rows; the predicate
    means of the first segment hold a tie inside the top 5."""
    classes, predicates = ["bg", "cat", "dog"], ["p0", "p1", "p2", "p3", "p4", "p5"]
    f32 = lambda *rows: np.array(rows, np.float32)
    fr = {"a": {0: {"sub_scores": f32([0, 0.75, 0.25], [0, 0.5, 0.5]), "obj_scores": f32([0, 0.25, 0.75], [0, 0.125, 0.875]),
                    "pre_scores": f32([-1, -2, -3, -4, -5, -6], [-6, -5, -4, -3, -2, -1]), "tids": [[1, 2], [2, 1]]},
                1: {"sub_scores": f32([0, 0.25, 0.75]), "obj_scores": f32([0, 0.5, 0.25]),
                    "pre_scores": f32([-6, -5, -4, -3, -2, -1.5]), "tids": [[2, 1]]},
                "2": {"sub_scores": f32([0, 0.25, 0.5], [0, 0.25, 0.75]), "obj_scores": f32([0, 0.5, 0.25], [0, 0.25, 0.5]),
                      "pre_scores": f32([-5, -4, -3, -2, -1, -2.5], [-3, -2, -5, -2, -5, -6]), "tids": [[2, 1], [1, 2]]},
                3: {}},
          "b": {0: {"sub_scores": f32([0, 0.5, 0.25]), "obj_scores": f32([0, 0.5, 0.25]),
                    "pre_scores": f32([-1, -2, -3, -4, -5, -6]), "tids": [[7, 8]]}}}
    gt = {"a": [{"triplet": ["cat", "p0", "dog"], "subject_tid": 1, "object_tid": 2, "duration": [0, 4]},
                {"triplet": ["cat", "p3", "dog"], "subject_tid": 1, "object_tid": 2, "duration": [0, 4]},
                {"triplet": ["cat", "p5", "cat"], "subject_tid": 2, "object_tid": 1, "duration": [0, 3]}],
          "b": [{"triplet": [1, 0, 2], "subject_tid": 8, "object_tid": 7, "duration": [0, 1]}],
          "c": [{"triplet": [1, 0, 2], "subject_tid": 0, "object_tid": 1, "duration": [0, 1]}]}
    return fr, gt, classes, predicates


def frame_record(seed=7500, n_boxes=6, C=16, R=62):
    """One seeded frame record in the layout ``forward_predicate`` returns in eval mode, rel_scores as a numpy array (the
    caller wraps it as a tensor for the reference's ``.data.cpu().numpy()``)."""
    rng = np.random.default_rng(seed)
    prob = rng.dirichlet(np.ones(C), n_boxes).astype(np.float32)
    pairs = [(0, 1), (1, 0), (2, 4), (5, 3), (3, 0)]
    ixs, ixo = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    rel = rng.dirichlet(np.ones(R), len(pairs)).astype(np.float32)
    prior = rng.uniform(0, 1, (len(pairs), R)) * (rng.random((len(pairs), R)) < 0.4)      # many exact zeros, as a count table has
    return {"ixs": ixs, "ixo": ixo, "boxes": rng.uniform(0, 300, (n_boxes, 4)).tolist(), "sub_scores": prob[ixs], "obj_scores": prob[ixo],
            "rel_scores": rel, "rel_so_prior": prior, "tids": [[10 + s, 10 + o] for s, o in pairs]}
