"""Inputs of the track-mode association tests (video.associate_tracks): the crossing case of two objects of one class, a
hand-built video for the gap rules, seeded videos whose objects never overlap one another (so the box mode has nothing to
choose), the mixed batch the device form is compared on, and the table at its bound.  numpy only."""
import numpy as np

VID = "v"


def pair_index(i, j, n):
    """The ordered-pair index of (subject box i, object box j) among n boxes: i-major over i != j."""
    return i * (n - 1) + j - (1 if j > i else 0)


# ----------------------------------------------------------------------------------------------------------------------
# written out by hand
# ----------------------------------------------------------------------------------------------------------------------
def crossing_case(numbered_0_1=False):
    """A and B (class 1) pass each other in front of O (class 2, fixed); both hold predicate 7 with O, A-O at 0.9 and B-O at
    0.8, at frame 12 only B-O at 0.95.  The frame's boxes are [A, B, O], so A-O is pair 1 and B-O pair 3.
    ``numbered_0_1``: ``rel_idex`` 0 and 1 instead, for the box mode, which does not read it as a pair index.
    -> (frame_relations, tracks keyed by (vid, fno), {name: [box per frame]})."""
    frames, tracks = [], {}
    box = {"A": [], "B": [], "O": []}
    for t in range(24):
        a = [100.0 + 10 * t, 50.0, 200.0 + 10 * t, 250.0]
        b = [330.0 - 10 * t, 50.0, 430.0 - 10 * t, 250.0]
        o = [400.0, 100.0, 500.0, 200.0]
        box["A"].append(a), box["B"].append(b), box["O"].append(o)
        tracks[(VID, t)] = {"boxes": [a, b, o], "box_classes": [1, 1, 2], "tids": [0, 1, 0], "rels": []}
        frames.append([t, [[0.9, [1, 7, 2], [a, o], 0 if numbered_0_1 else pair_index(0, 2, 3)],
                           [0.95 if t == 12 else 0.8, [1, 7, 2], [b, o], 1 if numbered_0_1 else pair_index(1, 2, 3)]]])
    return {VID: frames}, tracks, box


class World(object):
    """A hand-built video: named objects (class, tid, corner), per frame the objects present IN BOX ORDER and the predictions
    (subject, predicate, object, score)."""

    def __init__(self, objects):
        self.objects = objects                           # name -> (class, tid, x0, y0)
        self.frames, self.tracks = [], {}

    def box(self, name, fno):
        _, _, x0, y0 = self.objects[name]
        return [x0 + 2.0 * fno, y0, x0 + 2.0 * fno + 60.0, y0 + 50.0]

    def frame(self, fno, present, preds):
        boxes = [self.box(n, fno) for n in present]
        self.tracks[(VID, fno)] = {"boxes": boxes, "box_classes": [self.objects[n][0] for n in present],
                                   "tids": [self.objects[n][1] for n in present], "rels": []}
        rows = []
        for s, p, o, score in preds:
            i, j = present.index(s), present.index(o)
            rows.append([score, [self.objects[s][0], p, self.objects[o][0]], [boxes[i], boxes[j]], pair_index(i, j, len(present))])
        self.frames.append([fno, rows])
        return self

    def relations(self):
        return {VID: self.frames}


def gap_world():
    return World({"S": (1, 0, 10.0, 10.0), "O": (2, 0, 10.0, 100.0), "X": (3, 0, 10.0, 200.0)})


# ----------------------------------------------------------------------------------------------------------------------
# seeded videos
# ----------------------------------------------------------------------------------------------------------------------
def draw_video(rng, n_frames, n_obj, vanish=False, number_gaps=False, quantise=False, counts=None, n_pool=130, n_pred=6):
    """One video of ``n_obj`` objects, each in a horizontal band of its own (boxes of different objects never overlap) and
    moving at most 4 pixels per frame at a width of 100 or more (consecutive boxes of one object overlap at IoU > 0.9).  A
    pool of ``n_pool`` (subject, predicate, object) keys with a base score each; per frame about 92 % of the keys whose
    objects are both present are candidates (about 120), scored 0.7 * base + 0.3 * noise, and the 100 best are the frame's
    predictions, in pool order.  ``vanish``: objects leave for 1-9 frames; ``number_gaps``: frame numbers skip; ``quantise``:
    scores on a grid of 1/64 (ties); ``counts``: {frame position: the number of predictions the frame is cut to}.
    -> (frames [[fno, predictions], ...], {fno: annotation})."""
    cls = rng.integers(1, 4, n_obj)
    tid = np.array([int((cls[:k] == cls[k]).sum()) for k in range(n_obj)])
    width = 100.0 + 20.0 * rng.random(n_obj)
    x = 50.0 + 40.0 * rng.random(n_obj)[None, :] + np.cumsum(rng.uniform(-4.0, 4.0, (n_frames, n_obj)), 0)
    y = np.broadcast_to(120.0 * np.arange(n_obj) + 10.0, x.shape)
    boxes = np.stack([x, y, x + width, y + 80.0], 2)                     # (frames, objects, 4)
    present = np.ones((n_frames, n_obj), bool)
    if vanish:
        for _ in range(max(2, n_frames // 12)):
            t0, k = int(rng.integers(1, max(2, n_frames - 1))), int(rng.integers(0, n_obj))
            present[t0:t0 + int(rng.integers(1, 10)), k] = False
    numbers = np.arange(n_frames)
    if number_gaps:
        numbers = np.cumsum(np.where(rng.random(n_frames) < 0.04, rng.integers(2, 5, n_frames), 1)) + 3
    combos = [(a, p, b) for a in range(n_obj) for b in range(n_obj) if a != b for p in range(1, n_pred + 1)]
    pool = np.array([combos[i] for i in rng.permutation(len(combos))[:n_pool]])
    pa, pp, pb = pool[:, 0], pool[:, 1], pool[:, 2]
    base = rng.random(len(pool))
    frames, annos = [], {}
    for t in range(n_frames):
        fno = int(numbers[t])
        here = np.nonzero(present[t])[0]
        n = len(here)
        pos = np.full(n_obj, -1)
        pos[here] = np.arange(n)
        rows = boxes[t, here].tolist()
        annos[fno] = {"boxes": rows, "box_classes": cls[here].tolist(), "tids": tid[here].tolist(), "rels": []}
        cand = np.nonzero(present[t, pa] & present[t, pb] & (rng.random(len(pool)) < 0.92))[0]
        score = 0.7 * base[cand] + 0.3 * rng.random(len(cand))
        if quantise:
            score = np.round(score * 64.0) / 64.0
        cut = 100 if counts is None or t not in counts else counts[t]
        best = np.sort(np.argsort(-score, kind="stable")[:cut])
        cand, score = cand[best], score[best].tolist()
        i, j = pos[pa[cand]], pos[pb[cand]]
        idex = (i * (n - 1) + j - (j > i)).tolist()
        i, j, ca, cp, cb = i.tolist(), j.tolist(), cls[pa[cand]].tolist(), pp[cand].tolist(), cls[pb[cand]].tolist()
        frames.append([fno, [[score[k], [ca[k], cp[k], cb[k]], [rows[i[k]], rows[j[k]]], idex[k]] for k in range(len(cand))]])
    return frames, annos


def unambiguous_videos(seed=20261, n_videos=8):
    """8 videos of 30-150 frames and 5-8 objects, every object present in every frame, no empty frame, consecutive frame
    numbers: the inputs on which the box mode and the track mode must agree.  -> (frame_relations, tracks by (vid, fno))."""
    rng = np.random.default_rng(seed)
    rel, tracks = {}, {}
    for v in range(n_videos):
        frames, annos = draw_video(rng, int(rng.integers(30, 151)), int(rng.integers(5, 9)))
        rel[str(v)] = frames
        tracks.update(((str(v), fno), a) for fno, a in annos.items())
    return rel, tracks


def mixed_batch(seed=20262, n_videos=24):
    """The batch the device form is compared on: 24 videos, about 2400 frames.  Videos 0-20 have 30-300 frames, objects that
    leave for 1-9 frames, frame numbers that skip in every third video, scores on a grid of 1/64 in every second video, and
    frames cut to 0, 1 and 99 predictions (100 comes by itself); object indices are dense per video, so keys repeat across
    videos.  Video 21 has no frame, video 22 one frame, video 23 ten frames without a prediction."""
    rng = np.random.default_rng(seed)
    rel, tracks = {}, {}
    lengths = [300, 30] + [int(x) for x in rng.integers(30, 181, n_videos - 5)]
    for v, n_frames in enumerate(lengths + [0, 1, 10]):
        counts = dict(zip(rng.integers(0, max(n_frames, 1), 6).tolist(), [0, 1, 99, 0, 1, 99]))
        if v == len(lengths) + 2:
            counts = dict((t, 0) for t in range(n_frames))
        frames, annos = draw_video(rng, n_frames, int(rng.integers(5, 9)), vanish=True, number_gaps=v % 3 == 0,
                                   quantise=v % 2 == 1, counts=counts)
        rel[str(v)] = frames
        tracks.update(((str(v), fno), a) for fno, a in annos.items())
    return rel, tracks


class Tables(object):
    """Packed tables written out by hand (what video.associate_tracks_arrays_host and ops.video_associate_tracks read)."""

    def __init__(self, frames):
        """``frames``: per video a list of (frame number, [(key triple, since, score), ...])."""
        self.frame_off = np.cumsum([0] + [len(f) for f in frames]).astype(np.int32)
        flat = [fr for f in frames for fr in f]
        self.frame_no = np.array([fr[0] for fr in flat], np.int32)
        self.pred_off = np.cumsum([0] + [len(fr[1]) for fr in flat]).astype(np.int32)
        rows = [p for fr in flat for p in fr[1]]
        self.key = np.array([p[0] for p in rows], np.int32).reshape(-1, 3)
        self.since = np.array([p[1] for p in rows], np.int32).reshape(-1)
        self.score = np.array([p[2] for p in rows], np.float64).reshape(-1)

    def args(self):
        return self.frame_off, self.frame_no, self.pred_off, self.score, self.key, self.since


def bound_video(n_frames=26, period=8):
    """One video whose frame t holds the 100 keys (t % period, k, 0), k < 100, all with since 0: at max_gap = period - 1 every
    key's relation spans the video and period * 100 entries are open at once; at max_gap = period - 2 no relation gets a
    second member.  Scores are k-dependent dyadic fractions, so every sum is exact."""
    return [(t, [((t % period, k, 0), 0, (k + 1) / 128.0) for k in range(100)]) for t in range(n_frames)]
