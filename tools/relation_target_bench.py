#!/usr/bin/env python3
"""Time the rel_det targets (i2vsgg_amd.relation_targets), host form against device form, on seeded tables at F = 2 and 8 frames
with 64 detections, 30 annotated boxes and 60 annotated relations per frame; and the eager rel_det training step against the
eager pre_det step (``trainval_sgg_emb.py --no-graph --bs 2`` on the synthetic set, each in a child process started before this
one opens the GPU; the last display interval's frames/s).  Host: one process, numpy, vectorised per relation.  Device: upload ..
download, and HIP events around the two launches alone.  Median of ``--reps`` after a warm-up.  Not bench.py: the flagship
workload is the captured pre_det step."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N_REL = 62


def frame_tables(seed, n_frames, n_det=64, n_gt=30, n_relations=60, n_cls=15, h=600.0, w=1000.0):
    """Annotated boxes of 15 classes; two of three detections are annotated boxes with their corners moved by up to 12 % of the
    side (some fall below an overlap of 0.5), the rest wrong-class copies and boxes anywhere."""
    rng = np.random.default_rng(seed)
    off = lambda n: (np.arange(n_frames + 1) * n).astype(np.int32)
    det, dcl, gt, gcl, rel = [], [], [], [], []
    for _ in range(n_frames):
        x1, y1 = rng.uniform(0, w - 200, n_gt), rng.uniform(0, h - 200, n_gt)
        g = np.floor(np.stack([x1, y1, x1 + rng.uniform(60, 199, n_gt), y1 + rng.uniform(60, 199, n_gt)], 1))
        c = rng.integers(1, n_cls + 1, n_gt)
        pick = rng.integers(0, n_gt, n_det)
        side = np.stack([g[pick, 2] - g[pick, 0], g[pick, 3] - g[pick, 1]] * 2, 1)
        d = np.clip(g[pick] + rng.uniform(-0.12, 0.12, (n_det, 4)) * side, 0, [w, h, w, h])
        kind = rng.random(n_det)
        far = kind > 0.85
        d[far] = np.stack([rng.uniform(0, w - 150, far.sum()), rng.uniform(0, h - 150, far.sum())] * 2, 1) + [0, 0, 120, 120]
        dc = np.where(kind > 0.67, c[pick] % n_cls + 1, c[pick])
        so = rng.integers(0, n_gt, (n_relations, 2))
        so[:, 1] = np.where(so[:, 1] == so[:, 0], (so[:, 1] + 1) % n_gt, so[:, 1])
        det.append(d); dcl.append(dc); gt.append(g); gcl.append(c)
        rel.append(np.concatenate([so, rng.integers(0, N_REL, (n_relations, 1))], 1))
    u = rng.integers(0, 2 ** 32, size=(n_frames * n_relations, 10), dtype=np.uint32)
    return (off(n_det), np.concatenate(det), np.concatenate(dcl).astype(np.int32), off(n_gt), np.concatenate(gt),
            np.concatenate(gcl).astype(np.int32), off(n_relations), np.concatenate(rel).astype(np.int32), u,
            np.full(n_frames, h), np.full(n_frames, w))


def med(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def step_rate(task, iters, timeout):
    """frames/s of the last display interval of an eager run of the training script, in a child process."""
    cmd = [sys.executable, os.path.join(ROOT, "trainval_sgg_emb.py"), "--bs", "2", "--no-graph", "--no-save", "--iters_per_epoch", str(iters),
           "--disp_interval", str(iters // 3), "--vrd_task", task]
    if task == "rel_det":
        cmd += ["--source_det_boxes_path", "synthetic"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, cwd=ROOT).stdout.decode()
    rates = re.findall(r"([0-9.]+) frames/s", out)
    if not rates:
        raise SystemExit("no rate in the output of %s:\n%s" % (" ".join(cmd), out[-2000:]))
    return [float(r) for r in rates], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=24, help="0: leave the two training runs out")
    a = ap.parse_args()
    if a.step_iters:
        for task in ("pre_det", "rel_det"):
            rates, _ = step_rate(task, a.step_iters, 400)
            print("eager %s step, res101, --bs 2, synthetic set: %s frames/s per display interval of %d steps (last: %.1f ms per step)" % (
                task, " ".join("%.1f" % r for r in rates), a.step_iters // 3, 2e3 / rates[-1]))
    import torch
    from i2vsgg_amd import ops, relation_targets as rt
    for F in (2, 8):
        t = frame_tables(100 + F, F)
        host = [None]

        def run_host():
            host[0] = rt.relation_targets_host(*t, n_rel=N_REL)
        t0 = time.perf_counter()
        run_host()
        t_host = 1e3 * (time.perf_counter() - t0)
        h = host[0]
        draws = int((h["samp"][:, :, 0] >= 0).sum())
        print("workload: F = %d frames x 64 detections, 30 annotated boxes, 60 relations: %d draws, pairs per frame %s, dropped %s" % (
            F, draws, h["n_pairs"].tolist(), h["n_dropped"].tolist()))
        print("  host form (once)                          %9.2f ms" % t_host)
        dev = [None]

        def run_dev():
            res = ops.relation_targets(*t, n_rel=N_REL, device="cuda:0", read_status=False)
            dev[0] = {k: v.cpu().numpy() for k, v in res.items()}
        print("  device form (upload .. download)          %9.2f ms  (median of %d)" % (med(run_dev, a.reps), a.reps))
        same = all(np.array_equal(dev[0][k].view(np.uint32) if dev[0][k].dtype == np.float32 else dev[0][k],
                                  h[k].view(np.uint32) if h[k].dtype == np.float32 else h[k]) for k in rt.OUTPUTS)
        print("  same bits as the host form, every output: %s" % same)
        T = [torch.as_tensor(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0") for x in t]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ks = []
        for _ in range(a.reps + 1):
            ev[0].record()
            ops.relation_targets(*T, n_rel=N_REL, device="cuda:0", read_status=False)
            ev[1].record()
            torch.cuda.synchronize()
            ks.append(1e3 * ev[0].elapsed_time(ev[1]))
        print("  of which the launches (HIP events, incl. output allocation, two clears, two kernels) %8.1f us" % statistics.median(ks[1:]))


if __name__ == "__main__":
    main()
