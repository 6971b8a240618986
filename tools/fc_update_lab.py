"""The fused filter-gradient + SGD-momentum update of the relation head's linear layers, alone, through the C-ABI.

    python tools/fc_update_lab.py [--reps 20] [--out FILE]

Times i2v_conv_wgrad_sgd at the fc6 (128 x 50176 -> 4096) and fc7 (128 x 4096 -> 4096) shapes of configs[1] with the
persistent streaming kernel (I2V_TUNE_FC_UPDATE = 1) and the tiled kernel of rounds 3-6 (= 0), alternating the two, and checks
that both leave the same W and momentum bits.  Device events around `reps` back-to-back launches; the median of 5 such
windows.  TB/s counts the bytes the update must move (W and m read and written, x and gy read once); TF the 2 M N K FLOP.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from i2vsgg_amd._lib import TUNE, lib, ptr  # noqa: E402

SHAPES = (("fc6", 128, 4096, 50176), ("fc7", 128, 4096, 4096))
KEY = TUNE["I2V_FC_UPDATE"]


def update(x, gy, w, m, lr=1e-2, mom=0.9, wd=5e-4):
    M, K = x.shape
    N = gy.shape[1]
    rc = lib.i2v_conv_wgrad_sgd(ptr(x), ptr(gy), ptr(w), ptr(m), M, 1, 1, K, N, 1, 1, 1, 0, lr, mom, wd,
                                torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("i2v_conv_wgrad_sgd: %s" % lib.i2v_last_error().decode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    lines = ["shape      kernel      us/update    TB/s     TF   (median of %d windows of %d launches; min..max)" % (a.windows, a.reps)]
    saved = lib.i2v_get_tuning(KEY)
    try:
        for name, M, N, K in SHAPES:
            g = torch.Generator(device=dev).manual_seed(7)
            x = torch.randn(M, K, device=dev, generator=g)
            gy = torch.randn(M, N, device=dev, generator=g)
            w0 = torch.randn(N, K, device=dev, generator=g) / 96
            m0 = torch.randn(N, K, device=dev, generator=g) * 0.01
            outs = {}
            for mode in (0, 1):                          # one update each from the same state: identical bits
                assert lib.i2v_set_tuning(KEY, mode) == 0
                w, m = w0.clone(), m0.clone()
                update(x, gy, w, m)
                torch.cuda.synchronize()
                outs[mode] = (w, m)
            same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
            del outs
            w, m = w0.clone(), m0.clone()
            times = {0: [], 1: []}
            for _ in range(a.windows):
                for mode in (0, 1):                      # alternate the two kernels
                    assert lib.i2v_set_tuning(KEY, mode) == 0
                    update(x, gy, w, m)                  # warm
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        update(x, gy, w, m)
                    e1.record()
                    e1.synchronize()
                    times[mode].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            nbytes = 4.0 * (4 * N * K + M * K + M * N)
            flop = 2.0 * M * N * K
            for mode in (0, 1):
                t = np.array(times[mode])
                med = float(np.median(t))
                lines.append("%-6s %-14s %8.1f    %5.2f  %6.1f   (%.1f..%.1f)" % (
                    name, "persistent" if mode else "tiled (old)", med, nbytes / med / 1e6, flop / med / 1e6, t.min(), t.max()))
            lines.append("%-6s bit-equal W and m (old vs new): %s" % (name, same))
    finally:
        lib.i2v_set_tuning(KEY, saved)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
