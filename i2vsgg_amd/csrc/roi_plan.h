// The launch plans of RoIAlign forward / backward in csrc/roi_ops.hip, of launch_nms in csrc/nms.hip and of launch_soft_nms in
// csrc/soft_nms.hip (tests/test_soft_nms_host.py holds its cases):
// which kernel form, template selectors, grid, threads and dynamic LDS a shape takes.  The counterpart of conv_plan.h --
// host-only and pure: no HIP, no globals; the tuning table (g_i2v_tuning, indexed by I2V_TUNE_*) and the CU count come in as
// arguments, so the host tests check every decision without a GPU (tests/test_roi_plan_host.py against
// tests/golden/roi_plans.json).  The launchers check their arguments, ask for the plan and switch on it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/i2vsgg_hip.h"

namespace roiplan {

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// status of a plan: 0, or why the entry point refuses the shape (I2V_ERR_ARG with refusal_text); form, grid, ... are
// valid for PLAN_OK only
enum Status {
    PLAN_OK = 0,
    RAB_CHANNELS = 1,        // gather backward: C % 128 != 0
    RAB_COLUMNS = 2,         // gather backward: more than RAB_MAXA sample columns
    RAB_ROW_LDS = 3,         // gather backward: the row buffer of a W-wide map exceeds kRabLdsMax
    RAB_PAIRS = 4,           // gather backward: R * (PH + avg) >= 2^29 (roi, sample row) pairs
    RAB_GRID = 5,            // gather backward: B * H * (C / 128) workgroups do not fit a launch
    RAB_GOUT_2GIB = 6,       // gather backward: grad_out beyond a 32-bit buffer offset
};

inline const char* refusal_text(int status) {
    switch (status) {
    case RAB_CHANNELS: return "roi_align_bwd_gather: C must be a multiple of 128 (NHWC in and out)";
    case RAB_COLUMNS: return "roi_align_bwd_gather: at most 8 sample columns (pooled_w + avg <= 8)";
    case RAB_ROW_LDS:
    case RAB_PAIRS: return "roi_align_bwd_gather: map too wide for the LDS row buffer";
    case RAB_GRID: return "roi_align_bwd_gather: grid too large";
    case RAB_GOUT_2GIB: return "roi_align_bwd_gather: grad_out beyond the 2 GiB a 32-bit buffer offset reaches";
    }
    return "";
}

// ---------------------------------------------------------------- RoIAlign forward
enum AlignFwdForm { AF_ROI128 = 0, AF_ROI64 = 1, AF_COLS = 2, AF_ROWS = 3, AF_GENERIC = 4 };

struct AlignFwdPlan {
    int status;              // always PLAN_OK: the forward has a kernel for every shape its entry point accepts
    int form;                // AlignFwdForm
    int avg;                 // template selector <AVG>
    unsigned grid;
    int threads;
    size_t lds;              // dynamic LDS (none of the forward forms uses any)
};

inline AlignFwdPlan plan_roi_align_fwd(int feat_layout, int B, int C, int H, int W, int R, int PH, int PW, int avg, int out_layout,
                                       const int* tuning) {
    AlignFwdPlan q = {};
    q.avg = avg;
    q.threads = 256;
    const int cols = tuning[I2V_TUNE_ROIALIGN_COLS];
    if (feat_layout == I2V_LAYOUT_NHWC && C % 4 == 0) {
        // one ROI x 128 channels per workgroup (each tap through the L2 once): NHWC output, <= 64 sample points, 32-bit offsets;
        // I2V_TUNE_ROIALIGN_COLS = 1 keeps the column-pair kernel, 0 the round-1 row kernel
        const bool per_roi = cols == 2 && out_layout == I2V_LAYOUT_NHWC && C % 128 == 0 && (PH + avg) * (PW + avg) <= 64 &&
                             (long long)B * H * W * C * 4 < (1ll << 31);
        if (per_roi && R * (C / 128) < 512) {       // a small launch: 64 channels per workgroup, one pass
            q.form = AF_ROI64;
            q.grid = (unsigned)(R * (C / 64));
        } else if (per_roi) {
            q.form = AF_ROI128;
            q.grid = (unsigned)(R * (C / 128));
        } else if (!cols) {
            q.form = AF_ROWS;
            q.grid = (unsigned)(R * PH);
        } else {
            q.form = AF_COLS;                       // eight ROIs x one output row x one column pair
            q.grid = (unsigned)((R + 7) / 8 * 8 * PH * ((PW + 1) / 2));
        }
    } else {
        q.form = AF_GENERIC;                        // a thread per output element, grid-stride
        const long long blocks = cdiv((long long)R * C * PH * PW, 256);
        q.grid = (unsigned)(blocks < 65535 * 4 ? blocks : 65535 * 4);
    }
    return q;
}

// ---------------------------------------------------------------- RoIAlign backward
constexpr int RAB_SEG = 1024;           // (roi, sample row) pairs examined per list pass: 256 per wave
constexpr int RAB_BATCH = 4;            // listed pairs whose sample gradients are staged in LDS together (one per wave's record lanes)
constexpr int RAB_MAXA = 8;             // sample columns per row the gather kernels take
constexpr size_t kRabLdsMax = 60 * 1024;        // dynamic LDS the gather kernels may ask for (beside their static arrays)
// The widest map the autograd route hands to the gather; wider maps take the scatter.  The kernels' LDS would allow more:
// (W + 2) * 512 + 2048 <= kRabLdsMax is W <= 114 for GATHER_ROW2, and with GATHER_ROW's 16384 bytes of staged batches
// W <= 82 (the entry point i2v_roi_align_bwd_gather itself accepts those).  78 is the bound the route has always had.
constexpr int kRabRouteMaxW = 78;

enum AlignBwdRoute { ROUTE_SCATTER = 0, ROUTE_GATHER = 1 };
enum AlignBwdForm { AB_SCATTER = 0, AB_GATHER_ROW = 1, AB_GATHER_ROW2 = 2 };

struct AlignBwdPlan {
    int status;
    int route;               // AlignBwdRoute: what ops._RoIAlignFn.backward takes (when ops.ROIALIGN_BWD_GATHER)
    int form;                // AlignBwdForm
    int groups;              // GATHER_ROW2: pair groups per workgroup <.., GROUPS> (2: 64 channels each), else 0
    int avg, p7;             // template selectors <AVG, P7>; p7 (the 7 x 7 average grid as constants) is 0 for the scatter
    unsigned grid;
    int threads;
    size_t lds;
};

// bytes of dynamic LDS of a gather kernel: the row buffer (W + 2 cells of 128 channels), GATHER_ROW's staged batches, the list segment
inline size_t rab_lds_bytes(int W, bool row2) {
    return (size_t)(W + 2) * 128 * sizeof(float) + (row2 ? 0 : (size_t)RAB_BATCH * RAB_MAXA * 128 * sizeof(float)) +
           RAB_SEG * sizeof(unsigned short);
}

// The launch of i2v_roi_align_bwd_gather (NHWC in and out; route is GATHER).
inline AlignBwdPlan plan_roi_align_bwd_gather(int R, int PH, int PW, int avg, int B, int C, int H, int W, const int* tuning, int num_cu) {
    AlignBwdPlan q = {};
    q.route = ROUTE_GATHER;
    const bool row2 = tuning[I2V_TUNE_ROIALIGN_BWD] != 0;       // round 6: waves that never meet (0: round 5's staged batches)
    q.lds = rab_lds_bytes(W, row2);
    if (C % 128 != 0) q.status = RAB_CHANNELS;
    else if (PW + avg > RAB_MAXA) q.status = RAB_COLUMNS;
    else if (q.lds > kRabLdsMax) q.status = RAB_ROW_LDS;
    else if ((long long)R * (PH + avg) >= (1ll << 29)) q.status = RAB_PAIRS;
    else if ((long long)B * H * (C / 128) >= (1ll << 31)) q.status = RAB_GRID;
    else if ((long long)R * PH * PW * C * 4 >= (1ll << 31)) q.status = RAB_GOUT_2GIB;
    if (q.status) return q;
    q.form = row2 ? AB_GATHER_ROW2 : AB_GATHER_ROW;
    // GATHER_ROW2 with one pair group per workgroup (128 channels) or two (64 channels, half the dependent chain): two where
    // the launch fits the chip at once -- four workgroups on each CU -- (its time is then its longest list's), one where it
    // runs in rounds (the sum counts)
    q.groups = !row2 ? 0 : (long long)B * H * (C / 64) <= 4ll * num_cu ? 2 : 1;
    q.avg = avg;
    q.p7 = avg && PH == 7 && PW == 7;
    q.grid = (unsigned)(B * H * (C / (q.groups == 2 ? 64 : 128)));
    q.threads = 256;
    return q;
}

// The launch of i2v_roi_align_bwd: atomics into a zeroed map, any layout.
inline AlignBwdPlan plan_roi_align_bwd_scatter(int R, int PH, int avg) {
    AlignBwdPlan q = {};
    q.route = ROUTE_SCATTER;
    q.form = AB_SCATTER;
    q.avg = avg;
    q.grid = (unsigned)(R * (PH + avg));            // one sample row of one ROI per workgroup
    q.threads = 256;
    return q;
}

// Route and launch of a RoIAlign backward: the gather for NHWC maps and gradients of C % 128 == 0 channels, at most
// kRabRouteMaxW wide and RAB_MAXA sample columns; the scatter for everything else.  A status on a GATHER route is an error
// (the entry point refuses the shape), not a reason to scatter.
inline AlignBwdPlan plan_roi_align_bwd(int out_layout, int R, int PH, int PW, int avg, int feat_layout, int B, int C, int H, int W,
                                       const int* tuning, int num_cu) {
    const bool gather = feat_layout == I2V_LAYOUT_NHWC && out_layout == I2V_LAYOUT_NHWC && C % 128 == 0 && W <= kRabRouteMaxW &&
                        PW + avg <= RAB_MAXA && R > 0;
    return gather ? plan_roi_align_bwd_gather(R, PH, PW, avg, B, C, H, W, tuning, num_cu) : plan_roi_align_bwd_scatter(R, PH, avg);
}

// ---------------------------------------------------------------- NMS (mask + greedy scan)
constexpr int NMS_MASK_WAVES = 1;        // row blocks (waves) per workgroup sharing one column block's boxes: measured 1 / 2 / 4 waves 47.2 / 47.6 / 52.5 us at N = 12000 (18.0 / 19.4 / 18.4 at 6000)
constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_PIPE_WORDS = 3;      // words per lane: covers nblk - 1 <= 192 columns
constexpr int SUPER_ROWS = 1024, SUPER_WORDS = 16, NMS_SWEEPS = 48;

enum NmsScanForm { NS_SUPER = 0, NS_PIPELINED = 1, NS_GENERIC = 2 };

struct NmsPlan {
    int status;              // always PLAN_OK (the entry points bound n themselves)
    int nblk;                // 64-box blocks
    unsigned mask_grid[3];   // nms_mask_kernel: (column block, group of row blocks, image)
    int mask_threads;
    int form;                // NmsScanForm
    int sweeps;              // SUPER: fixed-point sweeps before the serial resolve (0: serial only)
    unsigned grid;           // the scan: one workgroup per image
    int threads;
    size_t lds;              // the scan's dynamic LDS (SUPER: a super-block's triangle of the mask)
};

inline NmsPlan plan_nms(int n_img, int n, const int* tuning) {
    NmsPlan q = {};
    const int nblk = (n + 63) / 64, key = tuning[I2V_TUNE_NMS_SCAN];
    q.nblk = nblk;
    q.mask_grid[0] = (unsigned)nblk;
    q.mask_grid[1] = (unsigned)cdiv(nblk, NMS_MASK_WAVES);
    q.mask_grid[2] = (unsigned)n_img;
    q.mask_threads = 64 * NMS_MASK_WAVES;
    q.grid = (unsigned)n_img;
    q.threads = SCAN_THREADS;
    // the super-block and the pipelined scan hold a row's words past the diagonal in SCAN_PIPE_WORDS registers per lane:
    // nblk - 1 <= 192, that is n <= 12352
    const bool in_registers = nblk - 1 <= 64 * SCAN_PIPE_WORDS;
    if (in_registers && key && (long long)n * nblk * 8 < (1ll << 31)) {
        q.form = NS_SUPER;
        q.sweeps = key < 2 ? 0 : key == 2 ? NMS_SWEEPS : key;
        q.lds = (size_t)SUPER_ROWS * SUPER_WORDS * 8;
    } else {
        q.form = in_registers ? NS_PIPELINED : NS_GENERIC;
    }
    return q;
}

// ---------------------------------------------------------------- Soft-NMS (one set per workgroup, rows on chip)
constexpr int SOFT_NMS_MAX_N = 4096;     // rows of a set: 16 waves x 64 lanes x 4 rows in registers, their boxes in 64 KiB of LDS
constexpr int SOFT_NMS_WAVE_MAX_N = 512; // up to here one wave holds the set (8 rows per lane) and never meets a barrier
constexpr int SOFT_NMS_BLOCK_WAVES = 16;

enum SoftNmsStatus { SOFT_NMS_ROWS = 1 };        // more than SOFT_NMS_MAX_N rows per set
enum SoftNmsForm { SN_WAVE = 0, SN_BLOCK = 1 };

inline const char* soft_nms_refusal_text(int status) {
    return status == SOFT_NMS_ROWS ? "soft_nms: at most 4096 rows per set" : "";
}

struct SoftNmsPlan {
    int status;
    int form;                // SoftNmsForm
    int waves;               // 1 (WAVE) or SOFT_NMS_BLOCK_WAVES
    int rows;                // rows per lane <K>: row k * threads + thread sits in register k
    unsigned grid;           // one workgroup per set
    int threads;
    size_t lds;              // dynamic LDS: a float4 per row, BLOCK: and two rounds of one 64-bit key per wave
};

inline SoftNmsPlan plan_soft_nms(int n_set, int n) {
    SoftNmsPlan q = {};
    if (n > SOFT_NMS_MAX_N) {
        q.status = SOFT_NMS_ROWS;
        return q;
    }
    q.form = n <= SOFT_NMS_WAVE_MAX_N ? SN_WAVE : SN_BLOCK;
    q.waves = q.form == SN_WAVE ? 1 : SOFT_NMS_BLOCK_WAVES;
    q.threads = 64 * q.waves;
    const int need = (int)cdiv(n, q.threads);
    // the instantiated register counts: 1, 2, 4, 5 (300 rows, the test loop's own size, in one wave), 8
    q.rows = need <= 2 ? (need < 1 ? 1 : need) : need <= 4 ? 4 : need == 5 ? 5 : 8;
    q.grid = (unsigned)n_set;
    q.lds = (size_t)n * 16 + (q.form == SN_BLOCK ? (size_t)2 * q.waves * 8 : 0);
    return q;
}

}  // namespace roiplan
