#!/usr/bin/env python3
"""Time Seq-NMS (i2vsgg_amd.seqnms), host form against device form, on seeded synthetic detections at the detector test loop's
own size: one video of 300 frames, the synthetic imdb's 15 object classes, up to 100 detections per frame (max_per_image).
Per class a few objects move linearly with jitter, are sometimes missed and sometimes detected twice, plus low-score clutter.
Host: one process, numpy, vectorised per frame.  Device: upload .. download, and HIP events around the launch alone.  Median
of ``--reps`` after a warm-up.  Not bench.py: the flagship workload is the training step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def detections(seed, n_frames, n_classes, per_frame=100, width=1000, height=600):
    """``all_boxes[j][i]`` like detections.pkl: at most ``per_frame`` rows per frame over all classes (the weakest go)."""
    rng = np.random.default_rng(seed)
    rows = [[] for _ in range(n_frames)]                 # per frame: (class, x1, y1, x2, y2, score)
    for j in range(1, n_classes):
        for _ in range(int(rng.integers(1, 5))):
            x, y, w, h = rng.uniform(0, width - 200), rng.uniform(0, height - 200), rng.uniform(40, 200), rng.uniform(40, 200)
            vx, vy, base = rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), rng.uniform(0.3, 0.95)
            t0, t1 = sorted(rng.integers(0, n_frames + 1, 2))
            for t in range(t0, t1):
                if rng.random() < 0.1:
                    continue
                jit = rng.uniform(-3, 3, 4)
                box = np.array([x + vx * t, y + vy * t, x + vx * t + w, y + vy * t + h]) + jit
                rows[t].append([j] + box.tolist() + [float(np.clip(base + rng.normal(0, 0.05), 0.02, 1.0))])
                for _ in range(int(rng.integers(0, 3))):    # the detector's near-duplicates that its own NMS let through
                    rows[t].append([j] + (box + rng.uniform(-12, 12, 4)).tolist() + [float(np.clip(base - rng.uniform(0.1, 0.4), 0.01, 1.0))])
        for t in range(n_frames):
            for _ in range(int(rng.integers(0, 8))):
                x, y = rng.uniform(0, width - 100), rng.uniform(0, height - 100)
                rows[t].append([j, x, y, x + rng.uniform(20, 100), y + rng.uniform(20, 100), float(rng.uniform(0.01, 0.3))])
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(n_frames)] for _ in range(n_classes)]
    for t in range(n_frames):
        r = np.asarray(rows[t], np.float64).reshape(-1, 6)
        r = r[np.argsort(-r[:, 5], kind="stable")[:per_frame]]
        for j in range(1, n_classes):
            all_boxes[j][t] = r[r[:, 0] == j, 1:].astype(np.float32)
    all_boxes[0] = [[] for _ in range(n_frames)]
    return all_boxes


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
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--videos", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    import torch
    from i2vsgg_amd import ops, seqnms
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    n_classes = get_imdb("synthetic_16_v").num_classes
    vids = [detections(9000 + v, a.frames, n_classes) for v in range(a.videos)]
    all_boxes = [[c for v in vids for c in v[j]] for j in range(n_classes)]
    frame_index = [(str(v), t) for v in range(a.videos) for t in range(a.frames)]
    t0 = time.perf_counter()
    pk = seqnms.pack(all_boxes, frame_index)
    t_pack = 1e3 * (time.perf_counter() - t0)
    counts = np.diff(pk.box_off)
    per_frame = counts.reshape(a.videos, n_classes, a.frames).sum(1)
    print("workload: %d video(s) x %d frames x %d classes, %d boxes (per frame: mean %.1f, max %d; per frame and class: max %d)" % (
        a.videos, a.frames, n_classes - 1, len(pk.score), per_frame.mean(), per_frame.max(), counts.max()))
    print("pack (host, shared by both forms)            %10.1f ms" % t_pack)
    host, stats = [None], {}

    def run_host():
        host[0] = seqnms.seq_nms_arrays_host(pk, stats=stats)
    t_host = med(run_host, a.host_reps) if a.host_reps > 0 else float("nan")
    print("seq-nms, host form                           %10.1f ms  (median of %d)" % (t_host, a.host_reps))
    dev = [None]

    def run_dev():
        dev[0] = [t.cpu().numpy() for t in ops.seq_nms(pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score, device="cuda:0")]
    t_dev = med(run_dev, a.reps)
    print("seq-nms, device form (upload .. download)    %10.1f ms  (median of %d)" % (t_dev, a.reps))
    print("  passes (tracks): %d over %d groups with boxes, at most %d in one group; %d boxes suppressed" % (
        int(dev[0][2].sum()), int((dev[0][2] > 0).sum()), int(dev[0][2].max()), int((dev[0][0] < 0).sum())))
    if host[0] is not None:
        print("  same ids / score bits / track counts as the host form: %s" % (
            np.array_equal(dev[0][0], host[0][0]) and np.array_equal(dev[0][1].view(np.uint32), host[0][1].view(np.uint32))
            and np.array_equal(dev[0][2], host[0][2])))
    d = "cuda:0"
    T = [torch.as_tensor(x).to(d) for x in (pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ks = []
    for _ in range(a.reps + 1):
        ev[0].record()
        ops.seq_nms(*T, device=d)
        ev[1].record()
        torch.cuda.synchronize()
        ks.append(ev[0].elapsed_time(ev[1]))
    print("  of which the launch (HIP events, incl. output allocation and the status read) %8.2f ms" % statistics.median(ks[1:]))


if __name__ == "__main__":
    main()
