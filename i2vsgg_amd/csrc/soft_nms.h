// launch_soft_nms (soft_nms.hip) for the library's own callers: the checked entry point i2v_soft_nms and the detection
// post-processing (det_post.hip).  Internal to the library: C++ linkage, not in include/i2vsgg_hip.h.
#pragma once
#include "common.h"

// One workgroup per set on st: dets (n_set, n, 5) rows in descending score, counts (n_set) valid rows or nullptr (all n) ->
// out_dets (n_set, n, 5) the emitted rows in emission order with their final scores, out_src (n_set, n) the input row of
// each, out_num (n_set).  For det_post.hip: all_scores (n_set, n), when given, gets the emitted scores and -inf behind
// them, and *total the sum of out_num (zeroed by the caller).  Checks method and the planner's status (I2V_ERR_ARG).
int32_t launch_soft_nms(const float* dets, const int* counts, int n_set, int n, int method, float nt, float sigma,
                        float min_score, float* out_dets, int* out_src, int* out_num, float* all_scores, int* total,
                        hipStream_t st);
