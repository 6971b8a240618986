#!/usr/bin/env python3
"""Time the video level of predicate recognition (i2vsgg_amd.recognition), host form against device form, on seeded synthetic
per-frame scores: 200 videos x 300 frames x 8 track pairs at VidVRD's 35 classes / 132 predicates, every pair annotated over
the whole video with one predicate (1600 segments of 300 rows, 480 000 rows of 202 float64).  Host: one process, numpy
(``align_arrays_host``).  Device: upload .. download (``align_arrays``), and HIP events around the launches alone with the
arrays resident.  Median of ``--reps`` after a warm-up.  Not bench.py: the flagship workload is the training step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def workload(seed, videos, frames, pairs, C, R):
    rng = np.random.default_rng(seed)
    fr, gt = {}, {}
    tids = [[2 * p, 2 * p + 1] for p in range(pairs)]
    for v in range(videos):
        vid = "v%04d" % v
        scores = rng.random((frames, pairs, 2 * C + R), dtype=np.float32)
        scores[:, :, 0] = 0.0
        scores[:, :, C] = 0.0
        scores[:, :, 2 * C:] -= np.float32(3.0)
        fr[vid] = dict((f, {"sub_scores": scores[f, :, :C], "obj_scores": scores[f, :, C:2 * C], "pre_scores": scores[f, :, 2 * C:],
                            "tids": tids}) for f in range(frames))
        gt[vid] = [{"triplet": [int(rng.integers(1, C)), int(rng.integers(0, R)), int(rng.integers(1, C))], "subject_tid": s,
                    "object_tid": o, "duration": [0, frames]} for s, o in tids]
    return fr, gt


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
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--classes", type=int, default=35)
    ap.add_argument("--predicates", type=int, default=132)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    import torch
    from i2vsgg_amd import ops, recognition
    C, R = a.classes, a.predicates
    fr, gt = workload(9100, a.videos, a.frames, a.pairs, C, R)
    t0 = time.perf_counter()
    pk = recognition.pack(fr, gt, list(range(C)), list(range(R)))
    t_pack = 1e3 * (time.perf_counter() - t0)
    del fr
    print("workload: %d videos x %d frames x %d pairs, C = %d, R = %d: %d segments, %d rows of %d float64 (%.0f MB), %d instances" % (
        a.videos, a.frames, a.pairs, C, R, len(pk.segments), len(pk.rows), pk.rows.shape[1], pk.rows.nbytes / 1e6, len(pk.inst)))
    print("pack (host, shared by both forms)              %10.1f ms" % t_pack)
    host, dev = [None], [None]

    def run_host():
        host[0] = recognition.align_arrays_host(pk)
    t_host = med(run_host, a.host_reps) if a.host_reps > 0 else float("nan")
    print("align, host form                               %10.1f ms  (median of %d)" % (t_host, a.host_reps))

    def run_dev():
        dev[0] = recognition.align_arrays(pk, "cuda:0")
    t_dev = med(run_dev, a.reps)
    print("align, device form (upload .. download)        %10.1f ms  (median of %d)" % (t_dev, a.reps))
    if host[0] is not None:
        same = all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                   for x, y in zip(dev[0], host[0]))
        print("  same bits as the host form in every output: %s" % same)
    print("  aligned instances %d, sub@1 hits %d, pre@5 hits %d" % (int(dev[0][4][7]), int(dev[0][4][0]), int(dev[0][4][5])))
    d = "cuda:0"

    def upload():
        torch.as_tensor(pk.rows).to(d)
        torch.cuda.synchronize()
    t_up = med(upload, a.reps)
    print("  of which the upload of the rows alone          %8.2f ms  (%.1f GB/s from pageable host memory)" % (
        t_up, pk.rows.nbytes / 1e6 / max(t_up, 1e-9)))
    T = [torch.as_tensor(x).to(d) for x in (pk.rows, pk.seg_off, pk.seg_row, pk.inst)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ks = []
    for _ in range(a.reps + 1):
        ev[0].record()
        ops.recognition_align(*T, C, R, device=d)
        ev[1].record()
        torch.cuda.synchronize()
        ks.append(ev[0].elapsed_time(ev[1]))
    print("  of which the launches (HIP events, incl. output allocation and the status read) %8.2f ms" % statistics.median(ks[1:]))


if __name__ == "__main__":
    main()
