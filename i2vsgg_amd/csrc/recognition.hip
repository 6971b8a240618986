// Predicate recognition (the pre_det branch of the reference's test loop, test_net_SGG_emb.py:213-228, 318-324): the per-frame
// tail of recognition_output (lib/utils.py:570-582) and the video-level alignment + accuracy@n of alignment /
// evaluate_recognition (:529-568, :335-372).  The rules are stated once, in i2vsgg_amd/recognition.py; the host forms there and
// in i2vsgg_amd/eval.py evaluate the same expressions in the same order (the library is built with -ffp-contract=off
// -fno-fast-math), so device and host agree bit for bit.  No floating-point atomics: every sum has a fixed order; the counters
// are integer atomics, whose result does not depend on the order.
#include "table_common.h"

#define REC_TOP 10           // slots of a ranking (np.argsort(-x)[:10])
#define REC_MAX_W I2V_RECOGNITION_MAX_WIDTH

// arg-max of a probability row with column 0 read as zero, the lower index winning ties; every lane returns it
__device__ __forceinline__ int rec_argmax(const float* __restrict__ row, int C, int lane) {
    float v = 0.0f;
    int vi = 0x7fffffff;
    for (int c = lane; c < C; c += I2V_WAVE) {
        const float x = c == 0 ? 0.0f : row[c];
        if (vi == 0x7fffffff || x > v) v = x, vi = c;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(vi, o);
        if (oi != 0x7fffffff && (vi == 0x7fffffff || ov > v || (ov == v && oi < vi))) v = ov, vi = oi;
    }
    return vi;
}

// One wave per pair (blocks [0, P)) and one per box (blocks [P, P + B): the box's class).
__global__ void __launch_bounds__(I2V_WAVE)
recognition_rows_kernel(const float* __restrict__ cls_prob, const float* __restrict__ rel_prob, const long long* __restrict__ ixs,
                        const long long* __restrict__ ixo, const double* __restrict__ L, int B, int P, int C, int R,
                        float* __restrict__ sub, float* __restrict__ obj, float* __restrict__ pre, int* __restrict__ cls,
                        int* status) {
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= P) {
        const int b = blockIdx.x - P;
        const int k = rec_argmax(cls_prob + (long long)b * C, C, lane);
        if (lane == 0) cls[b] = k;
        return;
    }
    const int p = blockIdx.x;
    const long long s = ixs[p], o = ixo[p];
    if (s < 0 || s >= B || o < 0 || o >= B) {                    // a malformed table: say so, write nothing for this pair
        if (lane == 0) atomicMax(status, p + 1);
        return;
    }
    const float* rs = cls_prob + s * C;
    const float* ro = cls_prob + o * C;
    for (int c = lane; c < C; c += I2V_WAVE) {
        sub[(long long)p * C + c] = c == 0 ? 0.0f : rs[c];
        obj[(long long)p * C + c] = c == 0 ? 0.0f : ro[c];
    }
    // L[cs - 1, co - 1, :] as numpy indexes it: class 0 (every other column zero) wraps to the last row
    int cs = rec_argmax(rs, C, lane) - 1, co = rec_argmax(ro, C, lane) - 1;
    if (cs < 0) cs += C - 1;
    if (co < 0) co += C - 1;
    const double* l = L + ((long long)cs * (C - 1) + co) * R;
    for (int r = lane; r < R; r += I2V_WAVE)
        pre[(long long)p * R + r] = (float)((double)rel_prob[(long long)p * R + r] + l[r]);
}

// One workgroup of one wave per segment: the mean of its rows, then the three rankings over the means staged in LDS.
__global__ void __launch_bounds__(I2V_WAVE)
recognition_segments_kernel(const double* __restrict__ rows, const int* __restrict__ seg_off, const int* __restrict__ seg_row,
                            int N, int M, int C, int R, double* __restrict__ mean, int* __restrict__ count,
                            int* __restrict__ top, int* status) {
    __shared__ double s_mean[REC_MAX_W];
    __shared__ int s_top[3 * REC_TOP];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int W = 2 * C + R;
    const int o0 = seg_off[s], o1 = seg_off[s + 1];
    int bad = i2v_range_bad(o0, o1, M) ? 1 : 0;
    if (!bad) {
        for (int i = o0 + lane; i < o1; i += I2V_WAVE) {
            const int r = seg_row[i];
            if (r < 0 || r >= N) bad = 1;
        }
    }
    bad = __syncthreads_or(bad);                                 // the same value in every lane
    if (bad && lane == 0) atomicMax(status, s + 1);
    const int n = bad ? 0 : o1 - o0;                             // a malformed segment comes out as an empty one
    for (int c = lane; c < W; c += I2V_WAVE) {
        double m = 0.0;
        if (n > 0) {
            double acc = rows[(long long)seg_row[o0] * W + c];
            for (int i = o0 + 1; i < o1; ++i) acc += rows[(long long)seg_row[i] * W + c];
            m = acc / (double)n;
        }
        mean[(long long)s * W + c] = m;
        s_mean[c] = m;
    }
    if (lane < 3 * REC_TOP) s_top[lane] = -1;
    if (lane == 0) count[s] = n;
    __syncthreads();                                             // s_mean and s_top are written
    if (n > 0) {
        for (int g = 0; g < 3; ++g) {
            const int off = g == 0 ? 0 : (g == 1 ? C : 2 * C), width = g == 2 ? R : C;
            for (int c = lane; c < width; c += I2V_WAVE) {
                const double v = s_mean[off + c];
                int rank = 0;                                    // columns that are greater, or equal with a lower index
                for (int j = 0; j < width && rank < REC_TOP; ++j) {
                    const double x = s_mean[off + j];
                    rank += (x > v || (x == v && j < c)) ? 1 : 0;
                }
                if (rank < REC_TOP) s_top[g * REC_TOP + rank] = c;
            }
        }
    }
    __syncthreads();                                             // every slot of s_top has its last value
    if (lane < 3 * REC_TOP) top[(long long)s * 3 * REC_TOP + lane] = s_top[lane];
}

__device__ __forceinline__ int rec_among(const int* __restrict__ t, int n, int label) {
    int h = 0;
    for (int i = 0; i < n; ++i) h |= t[i] == label ? 1 : 0;
    return h;
}

// One thread per instance, after the segments kernel on the same stream.
__global__ void __launch_bounds__(256)
recognition_hits_kernel(const int* __restrict__ inst, const int* __restrict__ count, const int* __restrict__ top, int S, int T,
                        int C, int R, int* __restrict__ hit, unsigned long long* totals, unsigned long long* per_class,
                        int* status) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    int h[8] = {0, 0, 0, 0, 0, 0, 0, 0};                         // the seven hits and "aligned"
    if (t < T) {
        const int seg = inst[4 * t], ls = inst[4 * t + 1], lp = inst[4 * t + 2], lo = inst[4 * t + 3];
        if (seg < 0 || seg >= S || ls < 0 || ls >= C || lo < 0 || lo >= C || lp < 0 || lp >= R) {
            atomicMax(status + 1, t + 1);
        } else if (count[seg] > 0) {
            const int* tp = top + (long long)seg * 3 * REC_TOP;
            h[0] = rec_among(tp, 1, ls);
            h[1] = rec_among(tp, 5, ls);
            h[2] = rec_among(tp + REC_TOP, 1, lo);
            h[3] = rec_among(tp + REC_TOP, 5, lo);
            h[4] = rec_among(tp + 2 * REC_TOP, 1, lp);
            h[5] = rec_among(tp + 2 * REC_TOP, 5, lp);
            h[6] = h[0] * h[2] * h[4];
            h[7] = 1;
            // objects[n][c] of evaluate_recognition: the subject's hit under the subject's class, the object's under the object's
            atomicAdd(per_class + 4 * ls + 0, (unsigned long long)h[0]);
            atomicAdd(per_class + 4 * ls + 1, 1ull);
            atomicAdd(per_class + 4 * ls + 2, (unsigned long long)h[1]);
            atomicAdd(per_class + 4 * ls + 3, 1ull);
            atomicAdd(per_class + 4 * lo + 0, (unsigned long long)h[2]);
            atomicAdd(per_class + 4 * lo + 1, 1ull);
            atomicAdd(per_class + 4 * lo + 2, (unsigned long long)h[3]);
            atomicAdd(per_class + 4 * lo + 3, 1ull);
        }
        for (int k = 0; k < 7; ++k) hit[7 * t + k] = h[k];
    }
    for (int k = 0; k < 8; ++k) {                                // every lane takes part; lanes past T hold zeros
        int v = h[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & (I2V_WAVE - 1)) == 0 && v) atomicAdd(totals + k, (unsigned long long)v);
    }
}

extern "C" size_t i2v_recognition_rows_workspace_bytes(int32_t n_pairs) {
    (void)n_pairs;
    return I2V_STATUS_BYTES;                                     // the status word
}

extern "C" int32_t i2v_recognition_rows(const float* cls_prob, const float* rel_prob, const int64_t* ixs, const int64_t* ixo,
                                        const double* L, int32_t n_boxes, int32_t n_pairs, int32_t n_classes, int32_t n_rel,
                                        float* sub, float* obj, float* pre, int32_t* cls, void* ws, size_t ws_bytes,
                                        void* stream) {
    I2V_CHECK_ARG(n_boxes >= 0 && n_pairs >= 0, "recognition_rows: negative count");
    I2V_CHECK_ARG(n_classes >= 2 && n_rel >= 1, "recognition_rows: needs at least 2 classes and 1 predicate, got %d / %d", n_classes,
                  n_rel);
    I2V_CHECK_ARG(n_boxes == 0 || (cls_prob && cls), "recognition_rows: null pointer");
    I2V_CHECK_ARG(n_pairs == 0 || (cls_prob && rel_prob && ixs && ixo && L && sub && obj && pre), "recognition_rows: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_recognition_rows_workspace_bytes(n_pairs), "recognition_rows: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 8, st, "recognition_rows: clearing the status word failed");
    if (n_pairs + n_boxes == 0) return I2V_OK;
    recognition_rows_kernel<<<n_pairs + n_boxes, I2V_WAVE, 0, st>>>(cls_prob, rel_prob, (const long long*)ixs, (const long long*)ixo,
                                                                   L, n_boxes, n_pairs, n_classes, n_rel, sub, obj, pre, cls,
                                                                   (int*)ws);
    I2V_CHECK_LAUNCH("recognition_rows");
    return I2V_OK;
}

extern "C" size_t i2v_recognition_align_workspace_bytes(int32_t n_segments, int32_t n_instances) {
    (void)n_segments;
    (void)n_instances;
    return I2V_STATUS_BYTES;                                     // two status words: segments, instances
}

extern "C" int32_t i2v_recognition_align(const double* rows, const int32_t* seg_off, const int32_t* seg_row, const int32_t* inst,
                                         int32_t n_rows, int32_t n_entries, int32_t n_segments, int32_t n_instances,
                                         int32_t n_classes, int32_t n_rel, double* mean, int32_t* count, int32_t* top,
                                         int32_t* hit, int64_t* totals, int64_t* per_class, void* ws, size_t ws_bytes,
                                         void* stream) {
    I2V_CHECK_ARG(n_rows >= 0 && n_entries >= 0 && n_segments >= 0 && n_instances >= 0, "recognition_align: negative count");
    I2V_CHECK_ARG(n_classes >= 2 && n_rel >= 1, "recognition_align: needs at least 2 classes and 1 predicate, got %d / %d",
                  n_classes, n_rel);
    I2V_CHECK_ARG((long long)2 * n_classes + n_rel <= REC_MAX_W, "recognition_align: row width 2 * %d + %d is over the limit of %d",
                  n_classes, n_rel, REC_MAX_W);
    I2V_CHECK_ARG(seg_off && totals && per_class, "recognition_align: null pointer");
    I2V_CHECK_ARG(n_rows == 0 || rows, "recognition_align: null pointer");
    I2V_CHECK_ARG(n_entries == 0 || seg_row, "recognition_align: null pointer");
    I2V_CHECK_ARG(n_segments == 0 || (mean && count && top), "recognition_align: null pointer");
    I2V_CHECK_ARG(n_instances == 0 || (inst && hit), "recognition_align: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_recognition_align_workspace_bytes(n_segments, n_instances),
                  "recognition_align: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 8, st, "recognition_align: clearing the counters failed");
    if (hipMemsetAsync(totals, 0, 8 * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(per_class, 0, (size_t)n_classes * 4 * sizeof(int64_t), st) != hipSuccess) {
        i2v_set_error("recognition_align: clearing the counters failed");
        return I2V_ERR_LAUNCH;
    }
    if (n_segments > 0) {
        recognition_segments_kernel<<<n_segments, I2V_WAVE, 0, st>>>(rows, seg_off, seg_row, n_rows, n_entries, n_classes, n_rel,
                                                                     mean, count, top, (int*)ws);
        I2V_CHECK_LAUNCH("recognition_align (segments)");
    }
    if (n_instances > 0) {
        recognition_hits_kernel<<<i2v_cdiv(n_instances, 256), 256, 0, st>>>(inst, count, top, n_segments, n_instances, n_classes,
                                                                           n_rel, hit, (unsigned long long*)totals,
                                                                           (unsigned long long*)per_class, (int*)ws);
        I2V_CHECK_LAUNCH("recognition_align (instances)");
    }
    return I2V_OK;
}
