#!/usr/bin/env python3
"""Time the proposal-recall cover on one large seeded set (tests/proposal_eval_cases.py random_batch): packing (host, shared),
the host form, and the device form -- upload to download (wall clock, synchronised) and the launch alone (HIP events) --
median of 5 after a warm-up, one process.  The default workload is the test loop's: 2000 images x 2000 candidates x 3-30
ground truths, 5 limits x 4 ranges.  The host form is timed once (it runs for a while).  ``--cpu``: host side only."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import numpy as np  # noqa: E402


def median_ms(fn, n=5):
    fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--candidates", type=int, default=2000)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import proposal_eval_cases as pc
    from i2vsgg_amd import proposal_eval as pe
    rng = np.random.default_rng(1)
    cands, roidb = pc.random_batch(2, [(a.candidates, int(m)) for m in rng.integers(3, 31, a.images)], size=1200, near=0.05)
    t0 = time.perf_counter()
    pk = pe.pack(cands, roidb)
    t_pack = 1e3 * (time.perf_counter() - t0)
    I, N, G, L, A = len(pk.cand_off) - 1, len(pk.cand_box), len(pk.gt_area), len(pk.limits), len(pk.ranges)
    print("set: %d images, %d candidates, %d ground truths (3-30 per image), %d limits x %d ranges = %d cells" % (I, N, G, L, A, I * L * A))
    print("pack (float64 conversion, ground-truth selection, offset tables; host, both forms) %10.1f ms" % t_pack)
    t0 = time.perf_counter()
    host = pe.cover_arrays_host(pk)
    t_host = 1e3 * (time.perf_counter() - t0)
    print("host form: cover %10.1f ms   (numpy, one thread, one run)" % t_host)
    if a.cpu:
        return
    import torch
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    t_e2e = median_ms(lambda: pe.cover_arrays(pk, device="cuda:0"))         # uploads, the launch, downloads (.cpu() synchronises)
    to = lambda x, dt: torch.as_tensor(x).to(dev, dt).contiguous()
    i32, f64 = torch.int32, torch.float64
    d = dict(cand_off=to(pk.cand_off, i32), cand_box=to(pk.cand_box, f64), gt_off=to(pk.gt_off, i32), gt_box=to(pk.gt_box, f64),
             gt_area=to(pk.gt_area, f64), limits=to(pk.limits, i32), ranges=to(pk.ranges, f64))
    from i2vsgg_amd._lib import check, lib, ptr, stream
    max_gt, max_cand = int(np.diff(pk.gt_off).max()), int(np.diff(pk.cand_off).max())
    ov = torch.full((L, A, G), -1.0, device=dev, dtype=f64)
    cand, step = (torch.full((L, A, G), -1, device=dev, dtype=i32) for _ in range(2))
    ws = torch.zeros(lib.i2v_proposal_cover_workspace_bytes(I), device=dev, dtype=torch.uint8)

    def launch():                                            # the C entry point alone: outputs and workspace allocated before
        check(lib.i2v_proposal_cover(ptr(d["cand_off"]), ptr(d["cand_box"]), ptr(d["gt_off"]), ptr(d["gt_box"]), ptr(d["gt_area"]),
                                     ptr(d["limits"]), ptr(d["ranges"]), I, N, G, L, A, max_gt, max_cand, ptr(ov), ptr(cand), ptr(step),
                                     ptr(ws), ws.numel(), stream()), "proposal_cover")
    launch()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    t_k = float(np.median(t))
    assert int(ws[:4].view(i32).item()) == 0
    print("device form: upload to download %10.1f ms" % t_e2e)
    print("device form, the launch alone (i2v_proposal_cover on resident inputs, outputs preallocated; HIP events):")
    print("    i2v_proposal_cover  (1 launch, %d workgroups of 4 waves)   %10.3f ms" % (I * L * A, t_k))
    same = (ov.cpu().numpy().tobytes() == host[0].tobytes() and np.array_equal(cand.cpu().numpy(), host[1])
            and np.array_equal(step.cpu().numpy(), host[2]))
    print("device == host (ov bits, cand, step): %s" % same)
    print("end to end with packing: host %.1f ms, device %.1f ms -- packing is %.0f %% of the device path"
          % (t_pack + t_host, t_pack + t_e2e, 100 * t_pack / (t_pack + t_e2e)))


if __name__ == "__main__":
    main()
