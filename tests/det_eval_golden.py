"""Inputs of the detection-evaluation tests: tests/golden/det_eval.npz (tools/gen_golden.py --only det_eval) back as
``all_boxes`` / roidb, and a larger seeded set that has no reference result (kernels against the host form)."""
import numpy as np

from conftest import golden


def golden_inputs():
    """(g, all_boxes, roidb, classes) of the golden file."""
    g = golden("det_eval")
    classes = tuple(str(c) for c in g["classes"])
    n_img = int(g["n_images"])
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(n_img)] for _ in classes]
    all_boxes[0] = [[] for _ in range(n_img)]
    det, det_cls, det_img = g["det"], g["det_cls"], g["det_img"]
    for c in range(1, len(classes)):
        for i in np.unique(det_img[det_cls == c]):
            all_boxes[c][i] = det[(det_cls == c) & (det_img == i)]
    roidb = []
    for i in range(n_img):
        m = g["gt_img"] == i
        roidb.append({"boxes": g["gt_box"][m].astype(np.uint16), "gt_classes": g["gt_cls"][m], "gt_ishard": g["gt_hard"][m]})
    return g, all_boxes, roidb, classes


def reference_curves(g, pk, t):
    """Per class k of threshold t: (rec, prec, ap_area, ap_11pt) of the reference."""
    out = []
    for k in range(pk.n_classes):
        a, b = int(pk.cls_off[k]), int(pk.cls_off[k + 1])
        out.append((g["rec_%d" % t][a:b], g["prec_%d" % t][a:b], g["ap_area_%d" % t][k], g["ap_11pt_%d" % t][k]))
    return out


def ap_bound(rec):
    """n_terms * 2^-52: the reference's np.sum adds the area terms pairwise, this package in index order; each order is within
    (n - 1) * 2^-53 * sum of the exact sum of the same terms, and the sum is at most 1."""
    return (len(np.unique(rec)) + 1) * 2.0 ** -52


def check_against_reference(g, pk, t, cur):
    """The asserts of the golden comparison, for the host form and for the kernels alike.  ``cur``: the curves dict.
    Cumulative tp (recovered as rec * npos) and prec bit-equal; the area ap within n_terms * 2^-52 (the reference's np.sum
    adds pairwise, this package in index order: each order is within (n - 1) * 2^-53 * sum of the exact sum of the same
    terms, and the sum is at most 1); the 11-point ap is 11 sequential additions of the same numbers: equal."""
    for k, (rec, prec, ap_area, ap_11pt) in enumerate(reference_curves(g, pk, t)):
        a, b = int(pk.cls_off[k]), int(pk.cls_off[k + 1])
        npos = int(pk.npos[k])
        assert npos == int(g["npos"][k])
        if npos > 0:
            assert np.array_equal(np.round(rec * npos).astype(np.int64), cur["cum_tp"][a:b]), k
            assert np.array_equal(rec.view(np.int64), cur["rec"][a:b].view(np.int64)), k
        else:
            assert np.isnan(rec).all() and np.isnan(cur["rec"][a:b]).all(), k
        assert np.array_equal(prec.view(np.int64), cur["prec"][a:b].view(np.int64)), k
        ref_tp = cur["cum_tp"][a:b] if npos > 0 else np.zeros(b - a, np.int64)        # npos 0: no true positive can exist
        assert npos > 0 or not cur["cum_tp"][a:b].any(), k
        # cumulative fp recovered from the reference's prec = tp / (tp + fp) where tp > 0 (tp / prec is within 1e-9 of an
        # integer there); where tp == 0, prec is 0 whatever fp is, and fp is then the count of non-ignored detections so far,
        # which the bit-equal prec of the first true positive behind it pins down
        pos = ref_tp > 0
        ref_fp = np.round(ref_tp[pos] / prec[pos] - ref_tp[pos]).astype(np.int64)
        assert np.array_equal(ref_fp, cur["cum_fp"][a:b][pos]), k
        bound = ap_bound(rec)
        print("class %d: %d detections, npos %d, ap %r (reference %r), |diff| %.3g, bound %.3g"
              % (k + 1, b - a, npos, float(cur["ap_area"][k]), float(ap_area), abs(float(cur["ap_area"][k]) - float(ap_area)), bound))
        if np.isnan(ap_area):
            assert np.isnan(cur["ap_area"][k]), k
        else:
            assert abs(cur["ap_area"][k] - ap_area) <= bound, (k, cur["ap_area"][k], ap_area)
        assert cur["ap_11pt"][k] == ap_11pt, (k, cur["ap_11pt"][k], ap_11pt)


def fresh_set(seed=77, n_images=2400, n_classes=16):
    """(all_boxes, roidb, classes): generic float32 boxes, scores on a grid of 0.005 (heavy ties), segments of 0-100
    detections and 0-80 ground truths, class 1 with more than 200 000 detections, class 14 without detections, class 15
    without ground truth."""
    rng = np.random.default_rng(seed)
    classes = tuple(["__background__"] + ["kind%d" % c for c in range(1, n_classes)])
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in classes]
    all_boxes[0] = [[] for _ in range(n_images)]
    roidb = []
    for i in range(n_images):
        per = []
        for c in range(1, n_classes - 1):
            r = rng.random()
            n = int(rng.integers(65, 81)) if r < 0.004 else (int(rng.integers(1, 7)) if r < 0.5 else 0)
            xy = rng.integers(0, 900, (n, 2))
            wh = rng.integers(8, 240, (n, 2))
            per.append(np.concatenate([xy, xy + wh, np.full((n, 1), c), (rng.random((n, 1)) < 0.12).astype(np.int64)], 1))
        g = np.concatenate(per)
        roidb.append({"boxes": g[:, :4].astype(np.uint16), "gt_classes": g[:, 4].astype(np.int32), "gt_ishard": g[:, 5].astype(np.int32)})
        for c in range(1, n_classes):
            if c == n_classes - 2:
                continue
            n = int(rng.integers(70, 101)) if c == 1 else (0 if rng.random() < 0.3 else int(rng.integers(1, 41)))
            if n == 0:
                continue
            gc = g[g[:, 4] == c][:, :4].astype(np.float64)
            box = np.empty((n, 4))
            xy = rng.uniform(0, 900, (n, 2))
            box[:, :2], box[:, 2:] = xy, xy + rng.uniform(8, 240, (n, 2))
            if len(gc):                                  # two thirds sit near a ground truth (duplicates included)
                near = rng.random(n) < 0.67
                src = gc[rng.integers(0, len(gc), n)]
                jit = src + rng.normal(0, 0.08, (n, 4)) * (src[:, 2:] - src[:, :2]).repeat(2).reshape(n, 4)[:, [0, 1, 0, 1]]
                box[near] = jit[near]
                box[:, 2:] = np.maximum(box[:, 2:], box[:, :2])
            score = rng.integers(0, 201, n) / 200.0
            all_boxes[c][i] = np.concatenate([box, score[:, None]], 1).astype(np.float32)
    return all_boxes, roidb, classes
