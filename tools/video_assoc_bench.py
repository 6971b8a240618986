#!/usr/bin/env python3
"""Time the video association and the detection matching of i2vsgg_amd.video, host form against device form, on a workload
of the VidVRD test split's order of magnitude: 200 videos x 300 frames x 100 predictions; evaluation with 200 predictions x
~30 ground truths per video.  Host: one process, numpy.  Device: end to end (packing is shared and timed on its own; upload,
launch, download, selection and gather), with HIP events around the launch alone.  Median of ``--reps`` after a warm-up.
Not bench.py: the flagship workload is the training step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


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
    ap.add_argument("--videos", type=int, default=200)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1, help="the host association takes minutes on the full workload")
    a = ap.parse_args()
    import torch
    from i2vsgg_amd import ops, synthetic as syn, video
    t0 = time.perf_counter()
    frames = dict(("b%03d" % k, syn.video_frames(5000 + k, a.frames, p_break=0.01)) for k in range(a.videos))
    print("workload: %d videos x %d frames x 100 predictions (drawn in %.1f s)" % (a.videos, a.frames, time.perf_counter() - t0))
    t0 = time.perf_counter()
    pk = video.pack_frames(frames)
    t_pack = 1e3 * (time.perf_counter() - t0)
    print("pack (host, shared by both forms)          %10.1f ms" % t_pack)
    host = [None]

    def run_host():
        host[0] = video.associate_arrays_host(pk)
    t_host = med(run_host, a.host_reps) if a.host_reps > 0 else float("nan")
    print("association, host form                     %10.1f ms  (median of %d)" % (t_host, a.host_reps))
    dev = [None]

    def run_dev():
        dev[0] = [t.cpu().numpy() for t in ops.video_associate(pk.frame_off, pk.frame_no, pk.pred_off, pk.score, pk.triplet,
                                                                pk.boxes, device="cuda:0")]
    t_dev = med(run_dev, a.reps)
    print("association, device form (upload .. download)%8.1f ms  (median of %d)" % (t_dev, a.reps))
    if host[0] is not None:
        print("  same ids / lengths / scores as the host form: %s" % all((x == y).all() for x, y in zip(
            [dev[0][0], dev[0][4]], [host[0][0], host[0][4]])))
    # the launch alone
    d = "cuda:0"
    T = [torch.as_tensor(x).to(d) for x in (pk.frame_off, pk.frame_no, pk.pred_off, pk.score, pk.triplet, pk.boxes)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ks = []
    for _ in range(a.reps + 1):
        ev[0].record()
        ops.video_associate(*T, device=d)
        ev[1].record()
        torch.cuda.synchronize()
        ks.append(ev[0].elapsed_time(ev[1]))
    print("  of which the launch (HIP events, incl. output allocation and the status read) %8.2f ms" % statistics.median(ks[1:]))
    t_gather = med(lambda: video.gather_relations(pk, *dev[0]), a.reps)
    print("selection + gather (host, shared)          %10.1f ms" % t_gather)
    rel = video.gather_relations(pk, *dev[0])
    # evaluation
    gts = dict((vid, syn.video_groundtruth(r, 7000 + k)) for k, (vid, r) in enumerate(rel.items()))
    t0 = time.perf_counter()
    pe = video.pack_eval(rel, gts)
    print("evaluation: %d predictions, %d ground truths, %d boxes; pack %.1f ms" % (
        len(pe.pred_rel), len(pe.gt_rel), len(pe.boxes), 1e3 * (time.perf_counter() - t0)))
    hm = [None]

    def match_host():
        hm[0] = video.match_arrays_host(pe, 0.5)
    t_mh = med(match_host, a.reps)
    dm = [None]

    def match_dev():
        dm[0] = [t.cpu().numpy() for t in ops.video_viou_match(pe.pred_off, pe.pred_rel, pe.pred_score, pe.gt_off, pe.gt_rel,
                                                               pe.boxes, 0.5, device=d)]
    t_md = med(match_dev, a.reps)
    print("matching, host form                        %10.1f ms" % t_mh)
    print("matching, device form (upload .. download) %10.1f ms   same hits: %s" % (t_md, (dm[0][1] == hm[0][1]).all()))
    E = [torch.as_tensor(x).to(d) for x in (pe.pred_off, pe.pred_rel, pe.pred_score, pe.gt_off, pe.gt_rel, pe.boxes)]
    ks = []
    for _ in range(a.reps + 1):
        ev[0].record()
        ops.video_viou_match(*E, 0.5, device=d)
        ev[1].record()
        torch.cuda.synchronize()
        ks.append(ev[0].elapsed_time(ev[1]))
    print("  of which the three launches (HIP events)  %9.2f ms" % statistics.median(ks[1:]))


if __name__ == "__main__":
    main()
