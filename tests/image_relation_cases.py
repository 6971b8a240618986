"""Cases for image relation recall@K (i2vsgg_amd.image_relations): the rules restated in scalar Python floats -- overlap,
union, the greedy walk, the counters --, a seeded generator of ``relations``-shaped records built on
``synthetic.relation_annotation`` / ``synthetic.detections_for``, and hand-worked cases with their expected outputs.  Nothing
here imports the module under test: the restatement is the independent side of every comparison."""
import numpy as np

from i2vsgg_amd import synthetic as syn

PAD = 100                    # rows of rlp_labels / sub_bboxes / obj_bboxes the test loop writes (eval.detection_output)


# ---------------------------------------------------------------------------------------------------------------------
# the rules, in scalar Python floats (IEEE doubles: one rounding per operation, like numpy's and the kernel's)
# ---------------------------------------------------------------------------------------------------------------------
def overlap(a, b):
    iw = (min(a[2], b[2]) - max(a[0], b[0])) + 1.0
    ih = (min(a[3], b[3]) - max(a[1], b[1])) + 1.0
    if iw <= 0.0 or ih <= 0.0:
        return 0.0
    inter = iw * ih
    aa = ((a[2] - a[0]) + 1.0) * ((a[3] - a[1]) + 1.0)
    ab = ((b[2] - b[0]) + 1.0) * ((b[3] - b[1]) + 1.0)
    return inter / ((aa + ab) - inter)


def union(s, o):
    return [min(s[0], o[0]), min(s[1], o[1]), max(s[2], o[2]), max(s[3], o[3])]


def score(mode, pred, gt):
    """pred / gt: (triplet, subject box, object box).  -1 where the triplets differ."""
    if tuple(pred[0]) != tuple(gt[0]):
        return -1.0
    if mode == 0:
        return min(overlap(pred[1], gt[1]), overlap(pred[2], gt[2]))
    return overlap(union(pred[1], pred[2]), union(gt[1], gt[2]))


def ranked_rows(record, max_pred, k_per_pair=None):
    """The rows of one record in rank order: descending float32 confidence, file order on ties, the per-pair cap, the cut.
    -> (rows, number before the cut)."""
    if record is None or record[1] is None:
        return [], 0
    conf = [float(np.float32(c)) for c in record[1]]
    rows = sorted(range(len(conf)), key=lambda r: (-conf[r], r))
    if k_per_pair is not None:
        kept, seen = [], {}
        for r in rows:
            pair = int(record[4][r])
            if seen.get(pair, 0) < k_per_pair:
                seen[pair] = seen.get(pair, 0) + 1
                kept.append(r)
        rows = kept
    return rows[:max_pred], len(rows)


def walk(mode, preds, gts, thr):
    """The greedy walk of one image in one mode.  -> (hit, hit_ov, gt_rank, predictions that took a ground truth other than
    their best one, hits whose overlap equals the threshold)."""
    taken = [False] * len(gts)
    hit, hit_ov, gt_rank = [-1] * len(preds), [-1.0] * len(preds), [-1] * len(gts)
    second = exact = 0
    for q, p in enumerate(preds):
        ov = [score(mode, p, g) for g in gts]
        best = best_any = -1
        for g in range(len(gts)):
            if ov[g] >= thr and ov[g] >= 0.0:
                if best_any < 0 or ov[g] > ov[best_any]:
                    best_any = g
                if not taken[g] and (best < 0 or ov[g] > ov[best]):
                    best = g
        if best >= 0:
            taken[best] = True
            hit[q], hit_ov[q], gt_rank[best] = best, ov[best], q
            second += 1 if best != best_any else 0
            exact += 1 if ov[best] == thr else 0
    return hit, hit_ov, gt_rank, second, exact


def reference(relations, annotations, n_rel, nreturns=(50, 100), iou_threshold=0.5, k_per_pair=None, seen_triplets=None):
    """Everything ``image_relations`` computes, image by image: dict of keys, pred_off, gt_off, pred_row, hit, hit_ov, gt_rank
    (mode-major lists), totals, zs_totals, per_predicate (nested lists of [hits, n_gt]), the three recalls per mode and K, and the
    counts the tests assert about their own inputs."""
    ks = list(nreturns)
    max_pred = max(ks)
    keys = sorted(k for k, a in annotations.items() if len(a["rels"]) > 0)
    out = {"keys": keys, "pred_off": [0], "gt_off": [0], "pred_row": [], "hit": [[], []], "hit_ov": [[], []], "gt_rank": [[], []],
           "n_second": [0, 0], "n_exact": [0, 0], "n_over_cut": 0, "gt_pred": [], "gt_zs": [],
           "n_ignored": sum(1 for k in relations if k not in annotations)}
    for key in keys:
        a = annotations[key]
        gts = []
        for s, o, p in a["rels"]:
            trip = (int(a["box_classes"][s]), int(p), int(a["box_classes"][o]))
            gts.append((trip, [float(v) for v in a["boxes"][s]], [float(v) for v in a["boxes"][o]]))
            out["gt_pred"].append(int(p))
            out["gt_zs"].append(0 if seen_triplets is None or trip in seen_triplets else 1)
        rec = relations.get(key)
        rows, before = ranked_rows(rec, max_pred, k_per_pair)
        out["n_over_cut"] += 1 if before > max_pred else 0
        preds = [(tuple(int(v) for v in rec[0][r]), [float(v) for v in rec[2][r]], [float(v) for v in rec[3][r]]) for r in rows]
        out["pred_row"] += rows
        out["pred_off"].append(out["pred_off"][-1] + len(rows))
        out["gt_off"].append(out["gt_off"][-1] + len(gts))
        for m in range(2):
            hit, hit_ov, gt_rank, second, exact = walk(m, preds, gts, float(iou_threshold))
            out["hit"][m] += hit
            out["hit_ov"][m] += hit_ov
            out["gt_rank"][m] += gt_rank
            out["n_second"][m] += second
            out["n_exact"][m] += exact
    G = len(out["gt_pred"])
    out["totals"] = [[[0, 0] for _ in ks] for _ in range(2)]
    out["zs_totals"] = [[[0, 0] for _ in ks] for _ in range(2)]
    out["per_predicate"] = [[[[0, 0] for _ in range(n_rel)] for _ in ks] for _ in range(2)]
    for m in range(2):
        for j, k in enumerate(ks):
            for g in range(G):
                h = 1 if 0 <= out["gt_rank"][m][g] < k else 0
                out["totals"][m][j][0] += h
                out["totals"][m][j][1] += 1
                if out["gt_zs"][g]:
                    out["zs_totals"][m][j][0] += h
                    out["zs_totals"][m][j][1] += 1
                out["per_predicate"][m][j][out["gt_pred"][g]][0] += h
                out["per_predicate"][m][j][out["gt_pred"][g]][1] += 1
    nan = float("nan")
    out["recall"] = [[t[0] / t[1] if t[1] else nan for t in out["totals"][m]] for m in range(2)]
    out["zero_shot_recall"] = [[t[0] / t[1] if t[1] else nan for t in out["zs_totals"][m]] for m in range(2)]
    out["mean_recall"] = []
    for m in range(2):
        row = []
        for j in range(len(ks)):
            acc, n = 0.0, 0
            for h, t in out["per_predicate"][m][j]:
                if t:
                    acc, n = acc + h / t, n + 1
            row.append(acc / n if n else nan)
        out["mean_recall"].append(row)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------
def record(rows, pad=PAD):
    """rows: [(triplet, confidence, subject box, object box, pair id)] in file order -> the five values of
    ``eval.detection_output``: label and box arrays zero-padded to ``pad`` rows, confidences and pair ids of the rows alone."""
    n, k = len(rows), max(pad, len(rows))
    rlp, sub, obj = np.zeros((k, 3), np.float64), np.zeros((k, 4), np.float64), np.zeros((k, 4), np.float64)
    for r, (trip, _, s, o, _) in enumerate(rows):
        rlp[r], sub[r], obj[r] = trip, s, o
    return (rlp, np.asarray([r[1] for r in rows], np.float32).reshape(n), sub, obj, np.asarray([r[4] for r in rows], np.int64).reshape(n))


NONES = (None, None, None, None, None)


def image(seed, n_gt, n_pred, n_rel=12, n_classes=6, n_boxes=14, dup_rows=0, near_dup=0, exact=False, tie_share=0.3, jitter=0.12):
    """One annotated image with exactly ``n_gt`` ground truths and its record of exactly ``n_pred`` rows.  The rows pair
    detections of ``synthetic.detections_for`` (two jittered copies of every annotated box -- at this jitter some overlap it by
    less than 0.5 --, wrong-class copies, distractors): for annotated relations the copies of their boxes under the annotated or
    another predicate, several rows per pair, and pairs of arbitrary detections.  ``dup_rows`` annotation rows are repeated;
    ``near_dup`` relations get a twin on a shifted copy of their subject box (equal triplets, different overlaps); ``exact``
    plants a pair of integer boxes with a prediction whose score is exactly 0.5 in both modes; ``tie_share`` of the
    confidences are multiples of 1/8."""
    rng = np.random.default_rng(seed)
    extra = dup_rows + near_dup + (1 if exact else 0)
    base = max(n_gt - extra, 0)
    anno = syn.relation_annotation(seed, n_boxes=n_boxes, n_pairs=max(base, 1), n_rel=n_rel, n_classes=n_classes)
    boxes, cls, rels = [list(b) for b in anno["boxes"]], list(anno["box_classes"]), [list(r) for r in anno["rels"][:base]]
    for _ in range(near_dup if rels else 0):
        s, o, p = rels[int(rng.integers(0, len(rels)))]
        b = boxes[s]
        d = float(rng.integers(2, 12))
        boxes.append([b[0] + d, b[1], b[2] + d, b[3]])
        cls.append(cls[s])
        rels.append([len(boxes) - 1, o, p])
    for _ in range(dup_rows if rels else 0):
        rels.append(list(rels[int(rng.integers(0, len(rels)))]))
    rng.shuffle(rels)
    det = syn.detections_for(seed, {"boxes": boxes, "box_classes": cls}, jitter=jitter, copies=2, n_wrong=3, n_distractors=4, n_classes=n_classes)
    dbox, dcls = det["boxes"], det["box_classes"]
    near = [max(range(len(boxes)), key=lambda b: overlap(d, boxes[b])) for d in dbox]      # the annotated box a detection copies
    of = dict((b, [j for j in range(len(dbox)) if near[j] == b]) for b in range(len(boxes)))
    rows = []
    row = lambda js, jo, p: ((dcls[js], p, dcls[jo]), 0.0, dbox[js], dbox[jo], js * len(dbox) + jo)
    for s, o, p in rels:
        for js in of[s]:
            for jo in of[o]:
                rows.append(row(js, jo, p if rng.random() < 0.8 else int(rng.integers(0, n_rel))))
                if rng.random() < 0.3:                           # the pair's second row: another predicate
                    rows.append(row(js, jo, int(rng.integers(0, n_rel))))
    rng.shuffle(rows)
    while len(rows) < n_pred:
        js, jo = (int(v) for v in rng.integers(0, len(dbox), 2))
        rows.insert(int(rng.integers(0, len(rows) + 1)), row(js, jo, int(rng.integers(0, n_rel))))
    rows = rows[:n_pred]
    if exact:                                                    # 100 of 200 pixels of each box and of the union: ov = 0.5
        boxes += [[700.0, 400.0, 709.0, 409.0], [710.0, 400.0, 719.0, 409.0]]
        cls += [1, 2]
        rels.insert(int(rng.integers(0, len(rels) + 1)), [len(boxes) - 2, len(boxes) - 1, 0])
        if rows:
            rows[int(rng.integers(0, len(rows)))] = ((1, 0, 2), 0.0, [700.0, 400.0, 709.0, 404.0], [710.0, 400.0, 719.0, 404.0], 10 ** 6)
    conf = rng.uniform(0.01, 1.0, len(rows))
    conf = np.where(rng.random(len(rows)) < tie_share, np.ceil(conf * 8) / 8, conf)
    rows = [(r[0], float(c)) + r[2:] for r, c in zip(rows, conf)]
    assert len(rels) == n_gt, (len(rels), n_gt)
    return {"boxes": boxes, "box_classes": cls, "rels": rels}, record(rows)


def generated_set(seed, n_images, gt_counts=None, pred_counts=None, n_rel=12, n_classes=6):
    """(relations, annotations) of ``n_images`` images ("g0000", ...).  Without explicit counts: 3 to 40 ground truths and 0 to
    140 rows, a fifth of the images over the loop's 100."""
    rng = np.random.default_rng(seed)
    relations, annotations = {}, {}
    for i in range(n_images):
        n_gt = int(gt_counts[i]) if gt_counts is not None else int(rng.integers(3, 41))
        n_pred = int(pred_counts[i]) if pred_counts is not None else int(rng.integers(101, 141) if i % 5 == 0 else rng.integers(0, 101))
        extra = min(max(n_gt - 1, 0), 3)
        dup, nd, ex = (1 if extra >= 1 and i % 3 == 0 else 0), (1 if extra >= 2 and i % 2 == 0 else 0), extra >= 3 and i % 7 == 0
        key = "g%04d" % i
        annotations[key], relations[key] = image(seed * 1000 + i, n_gt, n_pred, n_rel, n_classes, dup_rows=dup, near_dup=nd, exact=ex)
    return relations, annotations


DEVICE_GT = [1, 63, 64, 65, 130, 2, 5, 17, 33, 40]
DEVICE_PRED = [0, 1, 99, 100, 37, 64, 65, 128]


def device_set(seed=77, n_images=40):
    """About 40 images whose ground-truth counts include 1, 63, 64, 65 and 130 (one, one and more than two passes of a wave)
    and whose row counts include 0, 1, 99 and 100; a few images without predictions, one mapped to Nones."""
    gt = [DEVICE_GT[i % len(DEVICE_GT)] for i in range(n_images)]
    pr = [DEVICE_PRED[(i + i // len(DEVICE_PRED)) % len(DEVICE_PRED)] for i in range(n_images)]
    relations, annotations = generated_set(seed, n_images, gt, pr)
    relations["g0006"] = NONES
    del relations["g0011"]
    relations["stray"] = relations["g0002"]
    return relations, annotations


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------
def hand_cases():
    """name -> dict(relations, annotations, n_rel, kwargs of evaluate, and what is expected: ``pred_row``, per mode ``hit`` and
    ``gt_rank`` (relation first), ``recall`` {mode: {K: (hits, n_gt)}} and further counts), all worked out by hand."""
    cases = {}
    # (a) 100 of each box's 200 union pixels, and 100 of the union boxes' 200: ov is exactly 0.5 in both modes
    anno = {"a": {"boxes": [[0, 0, 9, 9], [10, 0, 19, 9]], "box_classes": [1, 2], "rels": [[0, 1, 3]]}}
    rel = {"a": record([((1, 3, 2), 0.9, [0, 0, 9, 4], [10, 0, 19, 4], 1)])}
    cases["a_at_threshold"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={"iou_threshold": 0.5}, pred_row=[0],
                                   hit=[[0], [0]], hit_ov=[[0.5], [0.5]], gt_rank=[[0], [0]], totals={50: [(1, 1), (1, 1)]})
    cases["a_above_threshold"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={"iou_threshold": 0.5000001}, pred_row=[0],
                                      hit=[[-1], [-1]], hit_ov=[[-1.0], [-1.0]], gt_rank=[[-1], [-1]], totals={50: [(0, 1), (0, 1)]})
    # (b) two ground truths with equal triplets; row 0 (subject = GT 0's) scores 1 and 2/3, row 1 scores 100/110 and 90/120:
    # both prefer GT 0, so row 1 takes GT 1 at 0.75.  Phrase: the union boxes score 1 and 3480/3600 for both rows.
    anno = {"b": {"boxes": [[0, 0, 9, 9], [2, 0, 11, 9], [50, 50, 59, 59]], "box_classes": [1, 1, 3], "rels": [[0, 2, 2], [1, 2, 2]]}}
    rel = {"b": record([((1, 2, 3), 0.9, [0, 0, 9, 9], [50, 50, 59, 59], 0), ((1, 2, 3), 0.8, [0, 0, 10, 9], [50, 50, 59, 59], 1)])}
    cases["b_second_best"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={}, pred_row=[0, 1], hit=[[0, 1], [0, 1]],
                                  hit_ov=[[1.0, 0.75], [1.0, 3480.0 / 3600.0]], gt_rank=[[0, 1], [0, 1]], totals={50: [(2, 2), (2, 2)]})
    # (c) row 0: subject and object swapped in position inside one union (phrase 1, relation 0); row 1: both boxes at 0.5
    # (100 of 200) but the union boxes at 1100 of 3300
    anno = {"c": {"boxes": [[0, 0, 9, 19], [10, 0, 19, 19], [0, 110, 9, 119], [100, 110, 109, 119]], "box_classes": [1, 2, 3, 4],
                  "rels": [[0, 1, 0], [2, 3, 1]]}}
    rel = {"c": record([((1, 0, 2), 0.9, [10, 0, 19, 19], [0, 0, 9, 19], 0), ((3, 1, 4), 0.8, [0, 100, 9, 119], [100, 110, 109, 129], 1)])}
    cases["c_modes_differ"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={}, pred_row=[0, 1], hit=[[-1, 1], [0, -1]],
                                   hit_ov=[[-1.0, 0.5], [1.0, -1.0]], gt_rank=[[-1, 1], [0, -1]], totals={50: [(1, 2), (1, 2)]})
    # (d) a relation annotated twice, predicted three times: one ground truth each, the third row none
    anno = {"d": {"boxes": [[5, 5, 50, 60], [40, 10, 90, 80]], "box_classes": [2, 4], "rels": [[0, 1, 2], [0, 1, 2]]}}
    same = lambda c: ((2, 2, 4), c, [5, 5, 50, 60], [40, 10, 90, 80], 0)
    cases["d_duplicates"] = dict(relations={"d": record([same(0.9), same(0.8), same(0.7)])}, annotations=anno, n_rel=5, kwargs={},
                                 pred_row=[0, 1, 2], hit=[[0, 1, -1], [0, 1, -1]], hit_ov=[[1.0, 1.0, -1.0], [1.0, 1.0, -1.0]],
                                 gt_rank=[[0, 1], [0, 1]], totals={50: [(2, 2), (2, 2)], 1: [(1, 2), (1, 2)]}, nreturns=(50, 1))
    # (e) rows 0 and 1 have one confidence: file order, so row 0 (the looser box: 46 * 51 of 46 * 56) takes the ground truth and
    # the exact row 1 finds it taken; row 2, a wrong triplet with the largest confidence, ranks first
    anno = {"e": {"boxes": [[5, 5, 50, 60], [40, 10, 90, 80]], "box_classes": [2, 4], "rels": [[0, 1, 2]]}}
    rel = {"e": record([((2, 2, 4), 0.5, [5, 5, 50, 55], [40, 10, 90, 80], 0), ((2, 2, 4), 0.5, [5, 5, 50, 60], [40, 10, 90, 80], 0),
                        ((2, 3, 4), 0.75, [5, 5, 50, 60], [40, 10, 90, 80], 0)])}
    cases["e_ties_in_file_order"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={}, pred_row=[2, 0, 1], hit=[[-1, 0, -1], [-1, 0, -1]],
                                         hit_ov=[[-1.0, 51.0 / 56.0, -1.0], [-1.0, 1.0, -1.0]], gt_rank=[[1], [1]],
                                         totals={50: [(1, 1), (1, 1)], 1: [(0, 1), (0, 1)]}, nreturns=(50, 1))
    # (f) a pair with two annotated predicates, both predicted; k_per_pair = 1 drops the pair's second row
    anno = {"f": {"boxes": [[5, 5, 50, 60], [40, 10, 90, 80], [100, 100, 150, 150]], "box_classes": [2, 4, 1], "rels": [[0, 1, 2], [0, 1, 4]]}}
    rel = {"f": record([((2, 4, 4), 0.9, [5, 5, 50, 60], [40, 10, 90, 80], 7), ((2, 2, 4), 0.8, [5, 5, 50, 60], [40, 10, 90, 80], 7),
                        ((2, 2, 1), 0.7, [5, 5, 50, 60], [100, 100, 150, 150], 3)])}
    cases["f_uncapped"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={}, pred_row=[0, 1, 2], hit=[[1, 0, -1], [1, 0, -1]],
                               hit_ov=[[1.0, 1.0, -1.0], [1.0, 1.0, -1.0]], gt_rank=[[1, 0], [1, 0]], totals={50: [(2, 2), (2, 2)]})
    cases["f_one_per_pair"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={"k_per_pair": 1}, pred_row=[0, 2], hit=[[1, -1], [1, -1]],
                                   hit_ov=[[1.0, -1.0], [1.0, -1.0]], gt_rank=[[-1, 0], [-1, 0]], totals={50: [(1, 2), (1, 2)]})
    # (g) img_a annotated and not predicted, img_b mapped to Nones, img_c predicted and hit, img_e annotated without relations
    # (not evaluated), img_d predicted and not annotated (ignored)
    two = {"boxes": [[5, 5, 50, 60], [40, 10, 90, 80]], "box_classes": [2, 4]}
    anno = {"img_a": dict(two, rels=[[0, 1, 2], [1, 0, 3]]), "img_b": dict(two, rels=[[0, 1, 2]]), "img_c": dict(two, rels=[[0, 1, 2]]),
            "img_e": dict(two, rels=[])}
    one = record([((2, 2, 4), 0.9, [5, 5, 50, 60], [40, 10, 90, 80], 0)])
    rel = {"img_b": NONES, "img_c": one, "img_d": one, "img_e": one}
    cases["g_missing_images"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={}, pred_row=[0], hit=[[0], [0]], hit_ov=[[1.0], [1.0]],
                                     gt_rank=[[-1, -1, -1, 0], [-1, -1, -1, 0]], totals={50: [(1, 4), (1, 4)]},
                                     counts={"n_images": 3, "n_gt": 4, "n_ignored": 1, "n_gt_zero_shot": 0})
    # (h) seen: (2, 2, 4) alone.  Ground truths (2, 2, 4) hit, (2, 3, 4) hit, (4, 2, 2) missed: zero-shot 1 of 2
    anno = {"h": dict(two, rels=[[0, 1, 2], [0, 1, 3], [1, 0, 2]])}
    rel = {"h": record([((2, 2, 4), 0.9, [5, 5, 50, 60], [40, 10, 90, 80], 0), ((2, 3, 4), 0.8, [5, 5, 50, 60], [40, 10, 90, 80], 0)])}
    cases["h_zero_shot"] = dict(relations=rel, annotations=anno, n_rel=5, kwargs={"seen_triplets": {(2, 2, 4)}}, pred_row=[0, 1],
                                hit=[[0, 1], [0, 1]], hit_ov=[[1.0, 1.0], [1.0, 1.0]], gt_rank=[[0, 1, -1], [0, 1, -1]],
                                totals={50: [(2, 3), (2, 3)]}, zs_totals={50: [(1, 2), (1, 2)]},
                                counts={"n_images": 1, "n_gt": 3, "n_ignored": 0, "n_gt_zero_shot": 2},
                                train={"t": dict(two, rels=[[0, 1, 2]])})
    return cases


def fractions_case():
    """Seven ground truths on three pairs: predicate 0 twice (one hit), 1 and 2 once (hit), 3, 4, 5 once (missed).  3 hits of 7
    at K = 50; per predicate 1/2, 1, 1, 0, 0, 0, so the mean recall is 2.5 / 6; at K = 1 only the first row counts: 1 of 7, mean
    (1/2) / 6.  The last row names predicate 5's pair with subject and object swapped: the boxes overlap by a tenth, the union boxes
    are equal, so phrase mode has a fourth hit."""
    boxes = [[5, 5, 50, 60], [40, 10, 90, 80], [100, 100, 150, 150], [200, 50, 260, 120]]
    anno = {"x": {"boxes": boxes, "box_classes": [1, 2, 3, 4],
                  "rels": [[0, 1, 0], [2, 3, 0], [0, 1, 1], [0, 1, 2], [0, 1, 3], [2, 3, 4], [1, 0, 5]]}}
    r = lambda s, o, cs, co, p, c: ((cs, p, co), c, boxes[s], boxes[o], s * 4 + o)
    rel = {"x": record([r(0, 1, 1, 2, 0, 0.9), r(0, 1, 1, 2, 1, 0.8), r(0, 1, 1, 2, 2, 0.7), r(0, 1, 1, 2, 4, 0.6), r(2, 3, 3, 4, 3, 0.5),
                        r(0, 2, 1, 3, 0, 0.4), r(0, 1, 2, 1, 5, 0.3)])}
    return rel, anno, 7
