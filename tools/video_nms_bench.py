#!/usr/bin/env python3
"""Time the video relation NMS (i2vsgg_amd.video.suppress), host form against device form on the same tables: seeded synthetic
candidates (tests/video_nms_cases.cluster_cell), by default 16 videos x 2000 candidates x 30 frames, 20 triplets per video and 5
distinct (subject, object) pairs per triplet, the rest duplicates with 0-2 px of jitter.  The host form is timed once; the device
form after one warm-up launch on a small table, several times, with the spread.  A cost record, no criterion.  Not bench.py:
the flagship workload is the training step."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--candidates", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--triplets", type=int, default=20)
    ap.add_argument("--objects", type=int, default=5)
    ap.add_argument("--viou", type=float, default=0.7)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import torch
    import video_nms_cases as nc
    from i2vsgg_amd import ops, video
    if not torch.cuda.is_available():
        raise SystemExit("video_nms_bench: no GPU (a time taken without one says nothing)")
    rng = np.random.default_rng(9100)
    pred = {}
    for v in range(a.videos):
        rels = []
        for t in range(a.triplets):
            rels += nc.cluster_cell(rng, (t, 1, v), a.candidates // a.triplets, a.frames, n_objects=a.objects, grid=1 << 16)
        pred["v%d" % v] = [rels[i] for i in rng.permutation(len(rels))]
    d = "cuda:0"
    t0 = time.perf_counter()
    pk = video.pack_nms(pred, video.NMS_MAX_POOL)
    t_pack = 1e3 * (time.perf_counter() - t0)
    print("workload: %d videos x %d candidates x %d frames: %d relations in %d cells (largest %d), %d boxes; vIoU %g" % (
        a.videos, a.candidates, a.frames, len(pk.rel), len(pk.cell_off) - 1, int(np.diff(pk.cell_off).max()), len(pk.boxes), a.viou))
    small = video.pack_nms(nc.hand_cases()[0][0].prediction)
    ops.video_relation_nms(small.cell_off, small.rel, small.boxes, a.viou, device=d)      # warm-up: one launch on a three-row table
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = video.suppress_arrays_host(pk, a.viou)
    t_host = 1e3 * (time.perf_counter() - t0)
    t_dev, t_res = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        dev = [x.cpu().numpy() for x in ops.video_relation_nms(pk.cell_off, pk.rel, pk.boxes, a.viou, device=d)]
        t_dev.append(1e3 * (time.perf_counter() - t0))
    T = [torch.as_tensor(x).to(d) for x in (pk.cell_off, pk.rel, pk.boxes)]
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ops.video_relation_nms(*T, a.viou, device=d)
        torch.cuda.synchronize()
        t_res.append(1e3 * (time.perf_counter() - t0))
    same = all(x.tobytes() == y.tobytes() for x, y in zip(host, dev))
    spread = lambda t: "%10.2f ms  (median of %d; %.2f .. %.2f)" % (float(np.median(t)), len(t), min(t), max(t))
    print("pack (checks, ranking, cells, float64 tables; host, both forms) %10.2f ms  (single measurement)" % t_pack)
    print("suppression, host form                                          %10.2f ms  (single measurement)" % t_host)
    print("suppression, device form (upload .. download)                   " + spread(t_dev))
    print("suppression, device form, tables resident                       " + spread(t_res) +
          "  (one launch, the output allocation, the status read)")
    print("  %d kept, %d suppressed; every output equal in bits: %s" % (int(host[0].sum()), int((host[0] == 0).sum()), same))
    if not same:
        raise SystemExit("video_nms_bench: the device form differs from the host form")


if __name__ == "__main__":
    main()
