// Video relation NMS: duplicate relations of one (video, triplet) cell are suppressed greedily by the trajectory overlap
// min(subject vIoU, object vIoU) (lib/utils.py:221-262 is the overlap).  The rules are stated once, in i2vsgg_amd/video.py
// (suppress); the host form there (suppress_arrays_host) and this kernel evaluate the same float64 expressions in the same
// order (-ffp-contract=off -fno-fast-math), so they agree bit for bit.  Every sum is one lane's sequential loop over frames
// from 0.0: no reduction across lanes, no floating-point atomics.
//
// The cut: a scan without a mask.  One workgroup per cell goes through the cell's rows in rank order; only a row that is
// still alive when its turn comes (a kept one) is compared, against the later rows that are still alive, one lane per
// column.  The n x n mask of all pairs is never formed: a cell of duplicates costs kept x n overlaps instead of n^2 / 2, and
// by / by_ov fall out of the one evaluation that decides.  What it gives up is parallelism across the rows of one cell.
#include "table_common.h"

#define RN_COLS 10           // the matcher's relation row (video.REL_COLS)
#define RN_MAXCELL 4096      // relations of one cell (video.NMS_MAX_POOL; VM_MAXG of the matcher)
#define RN_MAXLEN (1 << 20)  // frames of one trajectory (video.NMS_MAX_FRAMES)
#define RN_THREADS 256

// vIoU of trajectory `which` (0 subject, 1 object) of two rows whose spans and durations have been checked: the
// intersection over the common frames, ascending, one accumulator; vi / vj are the whole trajectories' volumes
__device__ __forceinline__ double rn_viou(const int* __restrict__ ri, const int* __restrict__ rj, int which,
                                          const double* __restrict__ boxes, double vi, double vj) {
    const int a0 = ri[4], a1 = ri[5], b0 = rj[4], b1 = rj[5];
    const int lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    if (hi <= lo) return 0.0;
    const double* x = boxes + ((size_t)ri[6 + 2 * which] + (size_t)(lo - a0)) * 4;     // lo - a0 < len_i, lo - b0 < len_j
    const double* y = boxes + ((size_t)rj[6 + 2 * which] + (size_t)(lo - b0)) * 4;
    double acc = 0.0;
    for (int f = lo; f < hi; ++f, x += 4, y += 4) {
        const double w = ((x[2] < y[2] ? x[2] : y[2]) - (x[0] > y[0] ? x[0] : y[0])) + 1.0;
        const double h = ((x[3] < y[3] ? x[3] : y[3]) - (x[1] > y[1] ? x[1] : y[1])) + 1.0;
        acc += (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
    }
    return acc / ((vi + vj) - acc);
}

// One workgroup per cell.  s_by[k]: -1 while row k is alive, else the row of the cell that suppressed it.  A malformed cell
// (offsets out of range, more than 4096 rows, a trajectory span outside `boxes`, a length that is not fend - fstart or is
// past 2^20) raises the status word and writes nothing: none of its offsets is followed.
__global__ void __launch_bounds__(RN_THREADS)
relation_nms_kernel(const int* __restrict__ cell_off, const int* __restrict__ rel, const double* __restrict__ boxes, int n_rel,
                    long long n_boxes, double thr, int* __restrict__ keep, int* __restrict__ by, double* __restrict__ by_ov,
                    double* vol, int* status) {
    __shared__ int s_by[RN_MAXCELL];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int r0 = cell_off[c], r1 = cell_off[c + 1];
    int bad = (i2v_range_bad(r0, r1, n_rel) || r1 - r0 > RN_MAXCELL) ? 1 : 0;
    const int n = bad ? 0 : r1 - r0;
    for (int k = tid; k < n; k += RN_THREADS) {
        const int* r = rel + (size_t)(r0 + k) * RN_COLS;
        const long long d = (long long)r[5] - (long long)r[4];
        for (int which = 0; which < 2; ++which) {
            const int off = r[6 + 2 * which], len = r[7 + 2 * which];
            if (i2v_span_bad(off, len, n_boxes) || (long long)len != d || len > RN_MAXLEN) bad = 1;
        }
        s_by[k] = -1;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) atomicMax(status, c + 1);
        return;
    }
    // volumes: one lane per (row, subject / object), the frames in order
    for (int k = tid; k < 2 * n; k += RN_THREADS) {
        const int* r = rel + (size_t)(r0 + (k >> 1)) * RN_COLS;
        const int which = k & 1, len = r[7 + 2 * which];
        const double* b = boxes + (size_t)r[6 + 2 * which] * 4;
        double acc = 0.0;
        for (int f = 0; f < len; ++f, b += 4) acc += ((b[2] - b[0]) + 1.0) * ((b[3] - b[1]) + 1.0);
        vol[2 * (size_t)r0 + k] = acc;
    }
    __syncthreads();                                     // the cell's volumes are written
    // the scan: i is the same in every lane, and s_by[i] is settled (its last store lies before a barrier)
    for (int i = 0; i + 1 < n; ++i) {
        if (s_by[i] >= 0) continue;                      // suppressed: it suppresses nothing; no store, so no barrier
        const int* ri = rel + (size_t)(r0 + i) * RN_COLS;
        const double vs = vol[2 * (size_t)(r0 + i)], vo = vol[2 * (size_t)(r0 + i) + 1];
        for (int j = i + 1 + tid; j < n; j += RN_THREADS) {
            if (s_by[j] >= 0) continue;
            const int* rj = rel + (size_t)(r0 + j) * RN_COLS;
            const double s = rn_viou(ri, rj, 0, boxes, vs, vol[2 * (size_t)(r0 + j)]);
            if (!(s > thr)) continue;                    // min(s, o) <= s: the object cannot change the decision
            const double o = rn_viou(ri, rj, 1, boxes, vo, vol[2 * (size_t)(r0 + j) + 1]);
            const double ov = o < s ? o : s;
            if (ov > thr) {
                s_by[j] = i;
                by_ov[r0 + j] = ov;
            }
        }
        __syncthreads();                                 // row i's stores to s_by are done before row i + 1 is looked at
    }
    for (int k = tid; k < n; k += RN_THREADS) {
        const int b = s_by[k];
        keep[r0 + k] = b < 0 ? 1 : 0;
        by[r0 + k] = b < 0 ? -1 : r0 + b;
        if (b < 0) by_ov[r0 + k] = -1.0;
    }
}

extern "C" size_t i2v_video_relation_nms_workspace_bytes(int32_t n_cells, int32_t n_rel) {
    (void)n_cells;
    (void)n_rel;
    return I2V_STATUS_BYTES;                             // the status word; this cut keeps no mask
}

extern "C" int32_t i2v_video_relation_nms(const int32_t* cell_off, const int32_t* rel, const double* boxes, int32_t n_cells,
                                          int32_t n_rel, int64_t n_boxes, double viou_threshold, int32_t* keep, int32_t* by,
                                          double* by_ov, double* vol, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_cells >= 0 && n_rel >= 0 && n_boxes >= 0, "video_relation_nms: negative count");
    I2V_CHECK_ARG(viou_threshold >= 0.0 && viou_threshold <= 1.0, "video_relation_nms: the threshold lies in [0, 1] (got %g)",
                  viou_threshold);
    I2V_CHECK_ARG(cell_off, "video_relation_nms: null pointer");
    I2V_CHECK_ARG(n_rel == 0 || (rel && keep && by && by_ov && vol), "video_relation_nms: null pointer");
    I2V_CHECK_ARG(n_boxes == 0 || boxes, "video_relation_nms: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_video_relation_nms_workspace_bytes(n_cells, n_rel), "video_relation_nms: workspace too small");
    if (n_cells == 0 || n_rel == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "video_relation_nms: clearing the status word failed");
    relation_nms_kernel<<<n_cells, RN_THREADS, 0, st>>>(cell_off, rel, boxes, n_rel, n_boxes, viou_threshold, keep, by, by_ov, vol,
                                                        (int*)ws);
    I2V_CHECK_LAUNCH("video_relation_nms");
    return I2V_OK;
}
