// VOC detection evaluation that ends the detector test loop (lib/datasets/voc_eval.py:132-212 behind
// imdb.evaluate_detections): the greedy match of every detection against the ground truths of its class and image, and per
// class the score order, the cumulative tp / fp, recall, precision, the precision envelope and both AP forms.
// Everything that decides something is float64 in the reference's operation order (the library is built with
// -ffp-contract=off -fno-fast-math: every + - * / rounds once, like the CPU's).  No floating-point atomics and no
// order that depends on scheduling: two runs give the same bits.
//
// Layout (i2vsgg_amd/detection_eval.py pack()): detections lie in results-file order -- class, then image, then row --
// so class c owns [cls_off[c], cls_off[c+1]) and a (class, image) pair with detections is one contiguous segment.
#include "table_common.h"
#include "sort.h"

#define DE_MAXG 4096         // ground truths of one (class, image): 64 lanes x 64 claimed bits in registers
#define DE_TP 1
#define DE_FP 2              // 0: neither (the best ground truth is hard)
#define DE_NONE 0x7fffffff
#define DE_MAXC 255          // classes: 8 bits of the sort key
#define DE_MAXPOS (1 << 24)  // detections of one class: 24 bits of the sort key
#define DE_CURVE_THREADS 1024

// numpy's order for max / argmax: a nan beats every number, the first of equals stays
__device__ __forceinline__ bool de_better(double a, double b) { return (a != a && b == b) || a > b; }

// One wave per (class, image) segment.  ``order`` (workspace, one int per detection) holds the segment's detections in
// descending key, equal keys in results-file order.
__global__ void __launch_bounds__(64)
det_eval_match_kernel(const int* __restrict__ seg_det_off, const int* __restrict__ seg_gt, const int* __restrict__ gt_off,
                      const int* __restrict__ det_key, const double* __restrict__ det_box, const double* __restrict__ gt_box,
                      const int* __restrict__ gt_hard, int n_det, int n_slots, int n_gt, int max_gt, double thr,
                      int* __restrict__ flag, double* __restrict__ ovmax, int* __restrict__ jmax, int* __restrict__ order,
                      int* status) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int d0 = seg_det_off[s], nd = seg_det_off[s + 1] - d0;
    const int slot = seg_gt[s];
    bool bad = i2v_span_bad(d0, nd, n_det) || slot < 0 || slot >= n_slots;
    int g0 = 0, ng = 0;
    if (!bad) {
        g0 = gt_off[slot];
        ng = gt_off[slot + 1] - g0;
        bad = i2v_span_bad(g0, ng, n_gt) || ng > max_gt || ng > DE_MAXG;
    }
    if (bad) {                                           // a malformed table: say so, touch nothing
        if (lane == 0) atomicMax(status, s + 1);
        return;
    }
    // 1. rank by (key descending, position ascending); any number of detections, 64 at a time
    for (int i = lane; i < nd; i += 64) order[d0 + i2v_rank_desc(det_key + d0, nd, i)] = i;
    __syncthreads();                                     // one wave: makes ``order`` visible to all its lanes
    // 2. walk them; lane l owns ground truths l, l + 64, ... and bit k of ``claimed`` is ground truth l + 64k
    unsigned long long claimed = 0;
    for (int q = 0; q < nd; ++q) {
        const int d = d0 + order[d0 + q];
        const double* bb = det_box + (size_t)d * 4;
        const double b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
        double best = -INFINITY;
        int bi = DE_NONE;
        for (int g = lane; g < ng; g += 64) {
            const double* gb = gt_box + (size_t)(g0 + g) * 4;       // voc_eval's order, clamped: not i2v_overlap_plus1's arithmetic
            const double ixmin = gb[0] > b0 ? gb[0] : b0;
            const double iymin = gb[1] > b1 ? gb[1] : b1;
            const double ixmax = gb[2] < b2 ? gb[2] : b2;
            const double iymax = gb[3] < b3 ? gb[3] : b3;
            double iw = ixmax - ixmin + 1.0, ih = iymax - iymin + 1.0;
            iw = iw > 0.0 ? iw : 0.0;
            ih = ih > 0.0 ? ih : 0.0;
            const double inters = iw * ih;
            const double uni = (b2 - b0 + 1.0) * (b3 - b1 + 1.0) + (gb[2] - gb[0] + 1.0) * (gb[3] - gb[1] + 1.0) - inters;
            const double ov = inters / uni;
            if (bi == DE_NONE || de_better(ov, best)) best = ov, bi = g;
        }
        for (int o = 32; o > 0; o >>= 1) {               // arg-max over the wave, the lowest index on equal overlap
            const double ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != DE_NONE && (bi == DE_NONE || de_better(ob, best) || (!de_better(best, ob) && oi < bi))) best = ob, bi = oi;
        }
        int f = DE_FP;
        if (bi != DE_NONE && best > thr) {
            const int mine = (int)((claimed >> (bi >> 6)) & 1ull);
            const int taken = __shfl(mine, bi & 63);
            if (gt_hard[g0 + bi]) f = 0;
            else if (!taken) {
                f = DE_TP;
                if (lane == (bi & 63)) claimed |= 1ull << (bi >> 6);
            }
        }
        if (lane == 0) {
            flag[d] = f;
            ovmax[d] = best;
            jmax[d] = bi != DE_NONE ? bi : -1;
        }
    }
}

extern "C" size_t i2v_det_eval_match_workspace_bytes(int32_t n_det) {
    if (n_det < 0) return I2V_STATUS_BYTES;
    return I2V_STATUS_BYTES + i2v_align((size_t)n_det * sizeof(int));    // status word, per-segment order
}

extern "C" int32_t i2v_det_eval_match(const int32_t* seg_det_off, const int32_t* seg_gt, const int32_t* gt_off,
                                      const int32_t* det_key, const double* det_box, const double* gt_box,
                                      const int32_t* gt_hard, int32_t n_seg, int32_t n_det, int32_t n_slots, int32_t n_gt,
                                      int32_t max_gt, double ovthresh, int32_t* flag, double* ovmax, int32_t* jmax, void* ws,
                                      size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_seg >= 0 && n_det >= 0 && n_slots >= 0 && n_gt >= 0, "det_eval_match: negative count");
    I2V_CHECK_ARG(max_gt >= 0 && max_gt <= DE_MAXG, "det_eval_match: at most %d ground truths of one class in one image (got %d)",
                  DE_MAXG, max_gt);
    I2V_CHECK_ARG(seg_det_off && gt_off, "det_eval_match: null pointer");
    I2V_CHECK_ARG(n_seg == 0 || seg_gt, "det_eval_match: null pointer");
    I2V_CHECK_ARG(n_det == 0 || (det_key && det_box && flag && ovmax && jmax), "det_eval_match: null pointer");
    I2V_CHECK_ARG(n_gt == 0 || (gt_box && gt_hard), "det_eval_match: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_det_eval_match_workspace_bytes(n_det), "det_eval_match: workspace too small");
    if (n_seg == 0 || n_det == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "det_eval_match: clearing the status word failed");
    det_eval_match_kernel<<<n_seg, 64, 0, st>>>(seg_det_off, seg_gt, gt_off, det_key, det_box, gt_box, gt_hard, n_det, n_slots,
                                                n_gt, max_gt, ovthresh, flag, ovmax, jmax, (int*)((char*)ws + I2V_STATUS_BYTES),
                                                (int*)ws);
    I2V_CHECK_LAUNCH("det_eval_match");
    return I2V_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Curve: one stable sort of all classes at once, then one workgroup per class
// ---------------------------------------------------------------------------------------------------------------------
// Sort key, ASCENDING: class (8 bits) | 0xFFFFFFFF - (key as order-preserving u32) (32 bits) | position in class (24 bits):
// classes stay where they are, within a class the key descends and equal keys keep their results-file order.  Padding
// is all ones and sorts last.  The sort itself is the library's (sort.hip), one segment.
__global__ void __launch_bounds__(256)
det_eval_keys_kernel(const int* __restrict__ det_key, const int* __restrict__ cls_off, int n_cls, int n_det, int P,
                     unsigned long long* __restrict__ out, int* status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    unsigned long long k = ~0ull;
    if (i < n_det) {
        int lo = 0, hi = n_cls;                          // the class c with cls_off[c] <= i < cls_off[c + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cls_off[mid] <= i) lo = mid; else hi = mid;
        }
        const int a = cls_off[lo], b = cls_off[lo + 1];
        if (a <= i && i < b && i - a < DE_MAXPOS) {
            const unsigned int u = (unsigned int)det_key[i] ^ 0x80000000u;
            k = ((unsigned long long)lo << 56) | ((unsigned long long)(0xFFFFFFFFu - u) << 24) | (unsigned long long)(i - a);
        } else {
            atomicMax(status, lo + 1);                   // the class table does not cover the detections
        }
    }
    out[i] = k;
}

// inclusive scans over the 1024 threads of a workgroup, in thread order; ``red`` holds one entry per wave
__device__ __forceinline__ unsigned long long de_block_scan_add(unsigned long long v, unsigned long long* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    __syncthreads();                                     // ``red`` of the previous call has been read
    if (lane == 63) red[w] = v;
    __syncthreads();
    unsigned long long off = 0;
    for (int k = 0; k < w; ++k) off += red[k];
    return v + off;
}

__device__ __forceinline__ double de_block_scan_max(double v, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o);
        if (lane >= o) v = u > v ? u : v;
    }
    __syncthreads();
    if (lane == 63) red[w] = v;
    __syncthreads();
    for (int k = 0; k < w; ++k) v = red[k] > v ? red[k] : v;
    return v;
}

// One workgroup per class, three passes over the class's detections in sorted order:
//   forward   perm, integer inclusive sums of tp and fp, rec = tp / npos, prec = tp / max(tp + fp, eps)
//   backward  the envelope (suffix maximum of prec) and how many rec reach each of the 11 thresholds
//   forward   ap = sum of (rec[i] - rec[i-1]) * envelope[i], added strictly in order by one wave
__global__ void __launch_bounds__(DE_CURVE_THREADS)
det_eval_curve_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ cls_off, const int* __restrict__ flag,
                      const int* __restrict__ npos, int n_det, int* __restrict__ perm, int* __restrict__ cum_tp,
                      int* __restrict__ cum_fp, double* __restrict__ rec, double* __restrict__ prec, double* __restrict__ env,
                      double* __restrict__ ap_area, double* __restrict__ ap_11pt, int* status) {
    __shared__ unsigned long long s_red[DE_CURVE_THREADS / 64];
    __shared__ double s_redd[DE_CURVE_THREADS / 64];
    __shared__ int s_cnt[11];
    const int c = blockIdx.x, t = threadIdx.x;
    const int a = cls_off[c], b = cls_off[c + 1];
    if (a < 0 || b < a || b > n_det || b - a > DE_MAXPOS) {
        if (t == 0) {
            atomicMax(status, c + 1);
            ap_area[c] = 0.0;
            ap_11pt[c] = 0.0;
        }
        return;
    }
    const int n = b - a;
    const double np_d = (double)npos[c];
    const double eps = 2.220446049250313e-16;            // np.finfo(np.float64).eps
    if (t < 11) s_cnt[t] = 0;
    // forward: sums
    unsigned long long carry = 0;                        // tp in the high word, fp in the low one
    for (int i0 = 0; i0 < n; i0 += DE_CURVE_THREADS) {
        const int i = i0 + t;
        unsigned long long v = 0;
        int p = 0;
        if (i < n) {
            const unsigned long long k = keys[a + i];
            p = a + (int)(k & (DE_MAXPOS - 1));
            if ((int)(k >> 56) != c || p >= b) {         // cannot happen with a table the key kernel accepted
                atomicMax(status, c + 1);
                p = a;
            }
            const int f = flag[p];
            v = f == DE_TP ? (1ull << 32) : (f == DE_FP ? 1ull : 0ull);
        }
        const unsigned long long incl = de_block_scan_add(v, s_red) + carry;
        if (i < n) {
            const int tp = (int)(incl >> 32), fp = (int)(incl & 0xFFFFFFFFull);
            const double tpd = (double)tp, den = (double)tp + (double)fp;
            perm[a + i] = p;
            cum_tp[a + i] = tp;
            cum_fp[a + i] = fp;
            rec[a + i] = tpd / np_d;
            prec[a + i] = tpd / (den > eps ? den : eps);
        }
        __syncthreads();
        if (t == DE_CURVE_THREADS - 1) s_red[0] = incl;  // the last thread's sum carries on (v = 0 past the end)
        __syncthreads();
        carry = s_red[0];
    }
    __syncthreads();                                     // rec / prec of this class are written (same workgroup reads them)
    // backward: envelope, threshold counts
    double run = 0.0;                                    // the sentinel behind the last precision
    int cnt[11];
    for (int k = 0; k < 11; ++k) cnt[k] = 0;
    for (int i0 = 0; i0 < n; i0 += DE_CURVE_THREADS) {
        const int i = n - 1 - (i0 + t);
        double v = 0.0;
        if (i >= 0) {
            v = prec[a + i];
            const double r = rec[a + i];
            for (int k = 0; k < 11; ++k) cnt[k] += r >= (double)k * 0.1 ? 1 : 0;
        }
        double m = de_block_scan_max(v, s_redd);
        m = run > m ? run : m;
        if (i >= 0) env[a + i] = m;
        __syncthreads();
        if (t == DE_CURVE_THREADS - 1) s_redd[0] = m;
        __syncthreads();
        run = s_redd[0];
    }
    for (int k = 0; k < 11; ++k) {
        int x = cnt[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if ((t & 63) == 0 && x) atomicAdd(&s_cnt[k], x);         // integers: any order gives the same sum
    }
    __syncthreads();                                     // env of this class is written, the counts are complete
    if (t >= 64) return;
    // forward, one wave: 64 terms at a time, added one by one in index order (a zero term changes nothing: skipped)
    double acc = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + t;
        double term = 0.0;
        if (i < n) {
            const double r = rec[a + i], prev = i > 0 ? rec[a + i - 1] : 0.0;
            if (r != prev) term = (r - prev) * env[a + i];
        }
        unsigned long long todo = __ballot(term != 0.0);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            acc += __shfl(term, l);
            todo &= todo - 1;
        }
    }
    if (t == 0) {
        // the closing term (1 - rec[n-1]) * 0 is +0 for every finite rec and nan for a nan rec, which acc already is
        ap_area[c] = acc;
        double ap = 0.0;
        for (int k = 0; k < 11; ++k) {
            const int m = s_cnt[k];                      // rec is non-decreasing: those that reach the threshold are the last m
            const double p = m > 0 ? env[a + n - m] : 0.0;
            ap = ap + p / 11.0;
        }
        ap_11pt[c] = ap;
    }
}

extern "C" size_t i2v_det_eval_curve_workspace_bytes(int32_t n_det) {
    if (n_det <= 0) return I2V_STATUS_BYTES;
    // status, keys, envelope
    return I2V_STATUS_BYTES + i2v_align((size_t)sort_padded(n_det) * 8) + i2v_align((size_t)n_det * sizeof(double));
}

extern "C" int32_t i2v_det_eval_curve(const int32_t* det_key, const int32_t* cls_off, const int32_t* flag, const int32_t* npos,
                                      int32_t n_cls, int32_t n_det, int32_t* perm, int32_t* cum_tp, int32_t* cum_fp, double* rec,
                                      double* prec, double* ap_area, double* ap_11pt, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_cls >= 0 && n_det >= 0, "det_eval_curve: negative count");
    I2V_CHECK_ARG(n_cls <= DE_MAXC, "det_eval_curve: at most %d classes (got %d)", DE_MAXC, n_cls);
    I2V_CHECK_ARG(n_det <= (1 << 30), "det_eval_curve: at most 2^30 detections (got %d)", n_det);
    I2V_CHECK_ARG(cls_off, "det_eval_curve: null pointer");
    I2V_CHECK_ARG(n_cls == 0 || (npos && ap_area && ap_11pt), "det_eval_curve: null pointer");
    I2V_CHECK_ARG(n_det == 0 || (det_key && flag && perm && cum_tp && cum_fp && rec && prec), "det_eval_curve: null pointer");
    I2V_CHECK_ARG(n_det == 0 || n_cls > 0, "det_eval_curve: detections without a class");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_det_eval_curve_workspace_bytes(n_det), "det_eval_curve: workspace too small");
    if (n_cls == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    int* status = (int*)ws;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "det_eval_curve: clearing the status word failed");
    unsigned long long* keys = (unsigned long long*)((char*)ws + I2V_STATUS_BYTES);
    double* env = nullptr;
    if (n_det > 0) {
        const int P = sort_padded(n_det);
        env = (double*)((char*)ws + I2V_STATUS_BYTES + i2v_align((size_t)P * 8));
        det_eval_keys_kernel<<<i2v_cdiv(P, 256), 256, 0, st>>>(det_key, cls_off, n_cls, n_det, P, keys, status);
        i2v_launch_sort_u64(keys, 1, P, st);
    }
    det_eval_curve_kernel<<<n_cls, DE_CURVE_THREADS, 0, st>>>(keys, cls_off, flag, npos, n_det, perm, cum_tp, cum_fp, rec, prec,
                                                              env, ap_area, ap_11pt, status);
    I2V_CHECK_LAUNCH("det_eval_curve");
    return I2V_OK;
}
