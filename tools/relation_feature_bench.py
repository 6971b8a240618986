#!/usr/bin/env python3
"""Time the pooling of video relation features (i2vsgg_amd.relation_features, csrc/relation_features.hip) on seeded tables:
``--videos`` videos of ``--frames`` frames with ``--pairs`` pair rows of ``--dim`` floats each, ``--relations`` relations per video
of 10 to ``--frames`` members (uniform), one member in ``--skip`` without a slot.  Kernel: HIP events around the launch alone,
the arrays resident and the outputs allocated, median of ``--reps`` after a warm-up.  Bytes gathered = valid members x dim x 4
(every member's row is read once by its relation; rows shared between relations count once per read), and the fraction of the
8 TB/s HBM peak those bytes give (the convention of bench.py's ``roofline_hbm``) -- the table is smaller than the bytes read
from it, so part of the reads are served by the caches.  Host form once.  Not bench.py: the flagship workload is the training
step."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8e12


def workload(seed, videos, frames, pairs, relations, skip):
    """The tables alone (the rows are made on the device): slot_off, mem_off, mem_slot, mem_idx."""
    rng = np.random.default_rng(seed)
    n_slots = videos * frames
    slot_off = (np.arange(n_slots + 1, dtype=np.int64) * pairs).astype(np.int32)
    R = videos * relations
    length = rng.integers(10, frames + 1, size=R)
    start = (rng.random(R) * (frames - length + 1)).astype(np.int64)
    mem_off = np.zeros(R + 1, np.int64)
    np.cumsum(length, out=mem_off[1:])
    M = int(mem_off[-1])
    rel = np.repeat(np.arange(R), length)
    j = np.arange(M) - mem_off[rel]
    mem_slot = ((rel // relations) * frames + start[rel] + j).astype(np.int32)       # member j lies on frame start + j of its video
    mem_slot[rng.random(M) < skip] = -1
    mem_idx = rng.integers(0, pairs, size=M).astype(np.int32)
    return slot_off, mem_off.astype(np.int32), mem_slot, mem_idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=200)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--relations", type=int, default=200)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--skip", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    from i2vsgg_amd import _lib, relation_features as rf
    d = "cuda:0"
    slot_off, mem_off, mem_slot, mem_idx = workload(9300, a.videos, a.frames, a.pairs, a.relations, a.skip)
    n_rows, R, M = int(slot_off[-1]), len(mem_off) - 1, len(mem_slot)
    valid = int((mem_slot >= 0).sum())
    gathered = valid * a.dim * 4
    g = torch.Generator(device=d).manual_seed(9301)
    feat = torch.randn((n_rows, a.dim), device=d, generator=g) * 100.0
    print("workload: %d videos x %d frames x %d pairs x %d floats = %d rows (%.0f MB); %d relations, %d members, %d valid; "
          "%.2f GB gathered per launch" % (a.videos, a.frames, a.pairs, a.dim, n_rows, n_rows * a.dim * 4 / 1e6, R, M, valid,
                                           gathered / 1e9))
    T = [torch.as_tensor(x).to(d) for x in (slot_off, mem_off, mem_slot, mem_idx)]
    pooled = torch.zeros((R, a.dim), device=d)
    count = torch.zeros((R,), device=d, dtype=torch.int32)
    ws = torch.zeros(int(_lib.lib.i2v_relation_feature_pool_workspace_bytes(R)), device=d, dtype=torch.uint8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ks = []
    for _ in range(a.reps + 1):
        ev[0].record()
        _lib.check(_lib.lib.i2v_relation_feature_pool(feat.data_ptr(), *(t.data_ptr() for t in T), n_rows, len(slot_off) - 1, R, M,
                                                      a.dim, pooled.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _lib.stream()), "relation_feature_pool")
        ev[1].record()
        torch.cuda.synchronize()
        ks.append(ev[0].elapsed_time(ev[1]))
    t_k = statistics.median(ks[1:])
    assert int(ws[:4].view(torch.int32).item()) == 0
    print("pool, kernel (HIP events, median of %d)         %10.3f ms   %.2f TB/s of gathered bytes = %.3f of the %.0f TB/s HBM peak" % (
        a.reps, t_k, gathered / t_k / 1e9, gathered / (t_k * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
    print("  all launches, ms: %s" % " ".join("%.3f" % k for k in ks))
    if not a.no_host:
        host_feat = feat.cpu().numpy()
        t0 = time.perf_counter()
        hp, hc, status = rf.pool_arrays_host(host_feat, slot_off, mem_off, mem_slot, mem_idx)
        t_host = 1e3 * (time.perf_counter() - t0)
        same = (np.array_equal(pooled.cpu().numpy().view(np.uint32), hp.view(np.uint32)) and np.array_equal(count.cpu().numpy(), hc)
                and status == 0)
        print("pool, host form (numpy, one process, once)      %10.1f ms   same bits as the kernel: %s" % (t_host, same))


if __name__ == "__main__":
    main()
