// launch_nms (nms.hip) for the library's own callers: the checked entry point i2v_nms_sorted and the RPN proposal path
// (rpn.hip), which brings a workspace it has sized itself.  Internal to the library: C++ linkage, not in include/i2vsgg_hip.h.
#pragma once
#include "common.h"

constexpr int SCAN_MAX_BLK = 1024;      // n <= 65536

// mask, then the greedy scan, on st: dets (n_img, n, 5) in descending score -> keep (n_img, n), num (n_img);
// mask: n_img * n * ceil(n / 64) words
int32_t launch_nms(const float* dets, int n_img, int n, float thresh, int max_keep, int* keep, int* num,
                   unsigned long long* mask, hipStream_t st);
