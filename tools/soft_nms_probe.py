#!/usr/bin/env python3
"""Time the detection post-processing of one frame (``ops.detection_postprocess``: decode, per class threshold / sort / NMS, the
image-wide cut) with the greedy NMS and with each Soft-NMS method, at the test loop's R = 300 rois with 36 and with 81 classes.

HIP events around ``--iters`` back-to-back calls on one stream (no host synchronisation inside the window), after a warm-up of
the same calls; the median of ``--reps`` such windows, per call, and their spread.  Twice: launched call by call (the host's
enqueue of the seven to nine launches bounds this one from below) and with twenty calls recorded into a graph and replayed, the
way ``eval.DetectStep`` runs them (the device's own time).  The methods alternate within a repetition, so a
drift of the machine reaches all of them.  The inputs are seeded: rois clustered around a dozen objects, so that a class has
overlapping candidates, softmax scores, the reference's thresholds (score > 0, NMS 0.3, 100 per image).

On a tree without Soft-NMS (the commit before it) the tool times the greedy path alone: the same file serves both sides of the
comparison in profiles/.

    python tools/soft_nms_probe.py [--out FILE.json]"""
import argparse
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


GRAPH_CALLS = 20


def frame(R, C, seed):
    rng = np.random.default_rng(seed)
    k = 12
    c = rng.uniform([50, 50], [850, 450], (k, 2))
    size = rng.uniform(60, 260, (k, 2))
    pick = rng.integers(0, k, R)
    xy = c[pick] + rng.normal(0, 12.0, (R, 2))
    wh = size[pick] * rng.uniform(0.8, 1.25, (R, 2))
    rois = np.zeros((R, 5), np.float32)
    rois[:, 1:3], rois[:, 3:5] = xy, xy + wh
    logits = rng.normal(0, 1.0, (R, C)) + 4.0 * (rng.integers(1, C, k)[pick][:, None] == np.arange(C)[None, :])
    prob = np.exp(logits - logits.max(1, keepdims=True))
    prob = (prob / prob.sum(1, keepdims=True)).astype(np.float32)
    pred = rng.normal(0, 0.1, (R, 4 * C)).astype(np.float32)
    return rois, prob, pred, (600.0, 1000.0, 1.6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from i2vsgg_amd import ops
    from i2vsgg_amd.graphs import replay_graph
    dev = torch.device("cuda:0")
    soft = "soft_nms" in inspect.signature(ops.detection_postprocess).parameters
    methods = [("hard", None)] + ([("linear", ("linear", 0.5, 0.001)), ("gaussian", ("gaussian", 0.5, 0.001))] if soft else [])
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "reps": a.reps, "soft_nms": soft, "cases": []}
    for C in (36, 81):
        R = 300
        rois, prob, pred, (h, w, s) = frame(R, C, 1000 + C)
        t = [torch.from_numpy(x).to(dev) for x in (rois, prob, pred)]
        info = torch.tensor([h, w, s], device=dev)
        out = (torch.zeros((C, R, 5), device=dev), torch.zeros((C,), device=dev, dtype=torch.int32))

        def call(opt):
            kw = {"soft_nms": opt} if opt is not None else {}
            ops.detection_postprocess(*t, 0.0, 0.0, 0.0, score_thresh=0.0, nms_thresh=0.3, max_per_image=100, im_info=info, out=out, **kw)

        times, kept = {m: [] for m, _ in methods}, {}
        for m, opt in methods:
            for _ in range(20):
                call(opt)
            torch.cuda.synchronize()
            kept[m] = int(out[1].sum().item())
        for _ in range(a.reps):
            for m, opt in methods:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    call(opt)
                e1.record()
                e1.synchronize()
                times[m].append(1e3 * e0.elapsed_time(e1) / a.iters)
        # the same calls recorded into a graph (GRAPH_CALLS per replay), as eval.DetectStep runs them: no enqueue cost per launch
        graphs_us = {}
        for m, opt in methods:
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                for _ in range(GRAPH_CALLS):
                    call(opt)
            for _ in range(3):
                replay_graph(g, dev)
            torch.cuda.synchronize()
            graphs_us[m] = (g, [])
        replays = max(1, a.iters // GRAPH_CALLS)
        for _ in range(a.reps):
            for m, _ in methods:
                g, v = graphs_us[m]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(replays):
                    replay_graph(g, dev)
                e1.record()
                e1.synchronize()
                v.append(1e3 * e0.elapsed_time(e1) / (replays * GRAPH_CALLS))
        for m, _ in methods:
            v, gv = np.asarray(times[m]), np.asarray(graphs_us[m][1])
            row = {"R": R, "C": C, "method": m, "us_per_frame": float(np.median(v)), "us_min": float(v.min()), "us_max": float(v.max()),
                   "graph_us_per_frame": float(np.median(gv)), "graph_us_min": float(gv.min()), "graph_us_max": float(gv.max()),
                   "detections": kept[m]}
            res["cases"].append(row)
            print("R %d  C %2d  %-8s  launched %8.2f us per frame (min %.2f, max %.2f)   in a graph %8.2f (min %.2f, max %.2f)   "
                  "%d windows of %d calls, %d detections" % (R, C, m, row["us_per_frame"], row["us_min"], row["us_max"],
                                                             row["graph_us_per_frame"], row["graph_us_min"], row["graph_us_max"],
                                                             a.reps, a.iters, kept[m]))
        del graphs_us
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
