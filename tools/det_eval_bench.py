#!/usr/bin/env python3
"""Time the detection evaluation on one large seeded set (tests/det_eval_golden.py fresh_set): packing (host, shared), the
host form, and the device form -- upload to download (wall clock, synchronised) and the kernels alone (HIP events) --
median of 5 after a warm-up, one process.  ``--cpu``: host form only (what profiles/r10_det_eval.txt holds so far)."""
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
    ap.add_argument("--images", type=int, default=6000)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    import det_eval_golden as dg
    from i2vsgg_amd import detection_eval as de
    all_boxes, roidb, classes = dg.fresh_set(n_images=a.images)
    t0 = time.perf_counter()
    pk = de.pack(all_boxes, roidb, len(classes))
    t_pack = 1e3 * (time.perf_counter() - t0)
    D, S, G = len(pk.det_key), len(pk.seg_gt), len(pk.gt_hard)
    print("set: %d images, %d classes, %d detections (largest class %d), %d segments, %d ground truths"
          % (pk.n_images, pk.n_classes, D, int(np.diff(pk.cls_off).max()), S, G))
    print("pack (string formatting of %d numbers, offset tables; host, both forms)   %10.1f ms" % (5 * D, t_pack))
    t_match = median_ms(lambda: de.match_arrays_host(pk, 0.5))
    flag = de.match_arrays_host(pk, 0.5)[0]
    t_curve = median_ms(lambda: de.curve_arrays_host(pk, flag))
    print("host form: match %10.1f ms   curves %10.1f ms   (numpy, one thread)" % (t_match, t_curve))
    if a.cpu:
        return
    import torch
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))

    def end_to_end():
        r = de.evaluate_packed(pk, 0.5, device="cuda:0")   # uploads, both launches, downloads (.cpu() synchronises)
        return r
    t_e2e = median_ms(end_to_end)
    to = lambda x, dt: torch.as_tensor(x).to(dev, dt).contiguous()
    i32, f64 = torch.int32, torch.float64
    d = dict(seg_det_off=to(pk.seg_det_off, i32), seg_gt=to(pk.seg_gt, i32), gt_off=to(pk.gt_off, i32), det_key=to(pk.det_key, i32),
             det_box=to(pk.det_box, f64), gt_box=to(pk.gt_box, f64), gt_hard=to(pk.gt_hard, i32), cls_off=to(pk.cls_off, i32),
             npos=to(pk.npos, i32))
    from i2vsgg_amd._lib import check, lib, ptr, stream
    max_gt = int(np.diff(pk.gt_off).max())
    C = pk.n_classes
    flag, jmax = torch.zeros(D, device=dev, dtype=i32), torch.zeros(D, device=dev, dtype=i32)
    ovmax = torch.zeros(D, device=dev, dtype=f64)
    perm, ctp, cfp = (torch.zeros(D, device=dev, dtype=i32) for _ in range(3))
    rec, prec = (torch.zeros(D, device=dev, dtype=f64) for _ in range(2))
    ap_a, ap_11 = (torch.zeros(C, device=dev, dtype=f64) for _ in range(2))
    ws_m = torch.zeros(lib.i2v_det_eval_match_workspace_bytes(D), device=dev, dtype=torch.uint8)
    ws_c = torch.zeros(lib.i2v_det_eval_curve_workspace_bytes(D), device=dev, dtype=torch.uint8)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return float(np.median(t))

    def k_match():                                       # the C entry point alone: outputs and workspace allocated before
        check(lib.i2v_det_eval_match(ptr(d["seg_det_off"]), ptr(d["seg_gt"]), ptr(d["gt_off"]), ptr(d["det_key"]), ptr(d["det_box"]),
                                     ptr(d["gt_box"]), ptr(d["gt_hard"]), S, D, pk.n_classes * pk.n_images, G, max_gt, 0.5, ptr(flag),
                                     ptr(ovmax), ptr(jmax), ptr(ws_m), ws_m.numel(), stream()), "det_eval_match")

    def k_curve():
        check(lib.i2v_det_eval_curve(ptr(d["det_key"]), ptr(d["cls_off"]), ptr(flag), ptr(d["npos"]), C, D, ptr(perm), ptr(ctp),
                                     ptr(cfp), ptr(rec), ptr(prec), ptr(ap_a), ptr(ap_11), ptr(ws_c), ws_c.numel(), stream()),
              "det_eval_curve")
    t_km = timed(k_match)
    t_kc = timed(k_curve)
    assert int(ws_m[:4].view(i32).item()) == 0 and int(ws_c[:4].view(i32).item()) == 0
    print("device form: upload to download %10.1f ms" % t_e2e)
    print("device form, kernels alone (the C entry points on resident inputs, outputs preallocated; HIP events):")
    print("    i2v_det_eval_match  (1 launch, %d waves)                  %10.3f ms" % (S, t_km))
    print("    i2v_det_eval_curve  (keys + bitonic sort + one workgroup per class) %10.3f ms" % t_kc)
    res = {"m": (flag, ovmax, jmax), "c": (perm, ctp, cfp, rec, prec, ap_a, ap_11)}
    hm = de.match_arrays_host(pk, 0.5)
    hc = de.curve_arrays_host(pk, hm[0])
    same = (np.array_equal(res["m"][0].cpu().numpy(), hm[0]) and res["m"][1].cpu().numpy().tobytes() == hm[1].tobytes()
            and np.array_equal(res["c"][0].cpu().numpy(), hc["perm"]) and np.array_equal(res["c"][3].cpu().numpy(), hc["rec"], equal_nan=True))
    print("device == host (flags, ovmax bits, permutation, rec): %s" % same)
    print("end to end with packing: host %.1f ms, device %.1f ms -- packing is %.0f %% of the device path"
          % (t_pack + t_match + t_curve, t_pack + t_e2e, 100 * t_pack / (t_pack + t_e2e)))


if __name__ == "__main__":
    main()
