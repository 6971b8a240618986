#!/usr/bin/env python3
"""Time the stitching step after Seq-NMS (i2vsgg_amd.seqnms.stitch_arrays), host form against device form on the same tables:
the workload of tools/seqnms_bench.py (seeded synthetic detections, objects missed in 10 % of their frames), Seq-NMS's ids from
the device.  Every figure is a single measurement after one warm-up launch on a small table; it is a cost record, no criterion.
Not bench.py: the flagship workload is the training step."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--videos", type=int, default=1)
    ap.add_argument("--max_gap", type=int, default=3)
    ap.add_argument("--stitch_iou", type=float, default=0.3)
    a = ap.parse_args()
    import torch
    from seqnms_bench import detections
    from i2vsgg_amd import ops, seqnms
    from i2vsgg_amd.roi_data_layer.roidb import get_imdb
    n_classes = get_imdb("synthetic_16_v").num_classes
    vids = [detections(9000 + v, a.frames, n_classes) for v in range(a.videos)]
    all_boxes = [[c for v in vids for c in v[j]] for j in range(n_classes)]
    frame_index = [(str(v), t) for v in range(a.videos) for t in range(a.frames)]
    pk = seqnms.pack(all_boxes, frame_index)
    d = "cuda:0"
    tid, _, n_tracks = seqnms.seq_nms_arrays(pk, device=d)
    print("workload: %d video(s) x %d frames x %d classes, %d boxes, %d Seq-NMS tracks; max_gap %d, stitch_iou %g" % (
        a.videos, a.frames, n_classes - 1, len(pk.score), int(n_tracks.sum()), a.max_gap, a.stitch_iou))
    small = seqnms.pack([[[]], [np.array([[0, 0, 20, 20, 0.5]], np.float32)]], [("w", 0)])
    seqnms.stitch_arrays(small, np.zeros(1, np.int32), device=d)                 # warm-up: one launch on a one-box table
    torch.cuda.synchronize()
    stats = {}
    t0 = time.perf_counter()
    host = seqnms.stitch_arrays_host(pk, tid, a.max_gap, a.stitch_iou, stats=stats)
    t_host = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    dev = seqnms.stitch_arrays(pk, tid, a.max_gap, a.stitch_iou, device=d)
    t_dev = 1e3 * (time.perf_counter() - t0)
    T = [torch.as_tensor(x).to(d) for x in (pk.group_off, pk.frame_no, pk.box_off, pk.box, pk.score, tid)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.track_stitch(*T, max_gap=a.max_gap, stitch_iou=a.stitch_iou, device=d)
    torch.cuda.synchronize()
    t_res = 1e3 * (time.perf_counter() - t0)
    same = all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(host, dev))
    print("stitching, host form                               %10.2f ms  (single measurement)" % t_host)
    print("stitching, device form (upload .. download)        %10.2f ms  (single measurement)" % t_dev)
    print("stitching, device form, tables resident            %10.2f ms  (single measurement; three launches, output allocation, "
          "the status and row-count reads)" % t_res)
    print("  %d links, %d chains of three or more, %d rows added, %d chains left; every output equal in bits: %s" % (
        stats["links"], stats["chains_of_three"], len(host[4]), int(host[2].sum()), same))


if __name__ == "__main__":
    main()
