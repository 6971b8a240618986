#!/usr/bin/env python3
"""Time image relation recall@K (i2vsgg_amd.image_relations), host form against device form, on a seeded synthetic set: 5 000
images x 100 written triplets x about 30 annotated relations (20 to 40) at 35 classes / 132 predicates; six of ten rows are
jittered copies of annotated pairs under the annotated predicate, the rest pair arbitrary boxes.  Packing (host, shared by both
forms); host: one process, numpy (``match_host`` + ``count_host``); device: upload .. download (``evaluate_packed``), and HIP
events around the two launches alone with the arrays resident.  Median of ``--reps`` after a warm-up.  Not bench.py: the flagship
workload is the training step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def workload(seed, images, rows, C, R, n_boxes=12):
    rng = np.random.default_rng(seed)
    relations, annotations = {}, {}
    for i in range(images):
        x1, y1 = rng.uniform(0, 800, n_boxes), rng.uniform(0, 450, n_boxes)
        boxes = np.floor(np.stack([x1, y1, x1 + rng.uniform(40, 190, n_boxes), y1 + rng.uniform(40, 140, n_boxes)], 1))
        cls = rng.integers(1, C, n_boxes)
        n_gt = int(rng.integers(20, 41))
        so = rng.integers(0, n_boxes, (n_gt, 2))
        so[:, 1] = np.where(so[:, 1] == so[:, 0], (so[:, 1] + 1) % n_boxes, so[:, 1])
        rels = np.concatenate([so, rng.integers(0, R, (n_gt, 1))], 1)
        key = "%06d.jpg" % i
        annotations[key] = {"boxes": boxes.tolist(), "box_classes": cls.tolist(), "rels": rels.tolist()}
        good = rng.random(rows) < 0.6
        of = rng.integers(0, n_gt, rows)
        s = np.where(good, rels[of, 0], rng.integers(0, n_boxes, rows))
        o = np.where(good, rels[of, 1], rng.integers(0, n_boxes, rows))
        p = np.where(good, rels[of, 2], rng.integers(0, R, rows))
        side = lambda b: np.stack([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]] * 2, 1)
        sub = boxes[s] + rng.uniform(-0.1, 0.1, (rows, 4)) * side(boxes[s])
        obj = boxes[o] + rng.uniform(-0.1, 0.1, (rows, 4)) * side(boxes[o])
        relations[key] = (np.stack([cls[s], p, cls[o]], 1).astype(np.float64), np.sort(rng.random(rows).astype(np.float32))[::-1].copy(),
                          sub, obj, (s * n_boxes + o).astype(np.int64))
    return relations, annotations


def med(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--classes", type=int, default=35)
    ap.add_argument("--predicates", type=int, default=132)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    import torch
    from i2vsgg_amd import image_relations as ir, ops
    R, ks = a.predicates, (50, 100)
    relations, annotations = workload(9200, a.images, a.rows, a.classes, R)
    t0 = time.perf_counter()
    pk = ir.pack(relations, annotations, R, ks)
    t_pack = 1e3 * (time.perf_counter() - t0)
    print("workload: %d images x %d rows, %d classes, %d predicates: %d predictions, %d ground truths (%.1f per image)" % (
        a.images, a.rows, a.classes, R, len(pk.pred_trip), len(pk.gt_trip), len(pk.gt_trip) / max(a.images, 1)))
    print("pack (host, shared by both forms)              %10.1f ms" % t_pack)
    host, dev = [None], [None]

    def run_host():
        host[0] = ir.evaluate_packed(pk, ks, 0.5)
    t_host = med(run_host, a.host_reps) if a.host_reps > 0 else float("nan")
    print("match + count, host form                       %10.1f ms  (median of %d)" % (t_host, a.host_reps))

    def run_dev():
        dev[0] = ir.evaluate_packed(pk, ks, 0.5, device="cuda:0")
    t_dev = med(run_dev, a.reps)
    print("match + count, device form (upload .. download)%10.1f ms  (median of %d)" % (t_dev, a.reps))
    if host[0] is not None:
        same = all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                   for x, y in zip(dev[0], host[0]))
        print("  same bits as the host form in every output: %s" % same)
    tot = dev[0][3]
    print("  relation hits@50 / @100 %d / %d, phrase %d / %d of %d" % (tot[0, 0, 0], tot[0, 1, 0], tot[1, 0, 0], tot[1, 1, 0], tot[0, 0, 1]))
    d = "cuda:0"
    T = [torch.as_tensor(x).to(d) for x in (pk.pred_off, pk.gt_off, pk.pred_trip, pk.pred_box, pk.gt_trip, pk.gt_box)]
    zs = torch.as_tensor(pk.gt_zs).to(d)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_k = []
    for _ in range(a.reps + 1):
        ev[0].record()
        rank = ops.image_relation_match(*T, 0.5, device=d)[2]
        ops.image_relation_count(rank, T[4], zs, ks, R, device=d)
        ev[1].record()
        torch.cuda.synchronize()
        t_k.append(ev[0].elapsed_time(ev[1]))
    print("  of which the two launches (HIP events, incl. output allocation and the status reads) %8.2f ms" % statistics.median(t_k[1:]))


if __name__ == "__main__":
    main()
