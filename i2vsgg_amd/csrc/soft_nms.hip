// Soft-NMS (Bodla et al., ICCV 2017) over sets of score-sorted detections: pick the best live row, emit it, decay its
// neighbours' scores by their IoU with it (linear, gaussian) or drop them (hard), repeat.  i2vsgg_amd/soft_nms.py states
// the rules and is the specification (soft_nms_host); hard and linear agree with it bit for bit.
//
// One set per workgroup, and the set stays on chip for the whole loop: thread t holds rows t, t + T, t + 2T, ... (box, area,
// current score, a live bit) in registers, and every row's box also sits in LDS, where the pick's box is read by all lanes at
// once.  Global memory is read once (the load) and written once (each emitted row, as it is emitted).
//
// A pick is a maximum over 64-bit keys (score mapped to an unsigned that orders like the float, then ~row: equal scores go to
// the lowest row); a dead row's key is 0, below every live one.  Lanes reduce with __shfl_xor; with more than one wave, the
// waves' maxima meet in LDS: wave w writes slot [t & 1][w] of pick t, ONE barrier, every thread reads all the slots.  Two
// rounds of slots, so a wave that has gone on to pick t + 1 writes the other round, and it cannot reach pick t + 2 before
// every wave has passed the barrier of pick t + 1, that is, has read round t.  "No live row left" is the reduced key being 0:
// one value every thread has computed from the same slots after the barrier, so all threads leave the loop in the same pick
// and every wave meets every barrier the same number of times.  The loop itself is bounded by the valid count (<= n).
//
// IoU is nms_cpu.py:14-29 in fp32, one rounding per operation (-ffp-contract=off), +1 extents, inter / ((a_m + a_i) - inter).
#include "soft_nms.h"
#include "roi_plan.h"
#include <algorithm>

using namespace roiplan;

namespace {
constexpr int M_HARD = I2V_SOFT_NMS_HARD, M_LINEAR = I2V_SOFT_NMS_LINEAR, M_GAUSSIAN = I2V_SOFT_NMS_GAUSSIAN;

__device__ __forceinline__ unsigned long long soft_key(float s, int row) {
    unsigned u = __float_as_uint(s + 0.0f);                  // -0 -> +0: equal scores, equal keys
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)row);
}
__device__ __forceinline__ float soft_key_score(unsigned long long key) {
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long key) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    return key;
}

template <int METHOD, int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void soft_nms_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                              int n, float nt, float sigma, float min_score,
                                                              float* __restrict__ out_dets, int* __restrict__ out_src,
                                                              int* __restrict__ out_num, float* __restrict__ all_scores,
                                                              int* __restrict__ total) {
    constexpr int T = 64 * WAVES;
    extern __shared__ __align__(16) unsigned char s_raw[];
    float4* s_box = (float4*)s_raw;                                            // n boxes
    unsigned long long* s_part = (unsigned long long*)(s_raw + (size_t)n * 16);   // WAVES > 1: [2][WAVES]
    const int set = blockIdx.x, tid = threadIdx.x;
    int cnt = counts ? counts[set] : n;
    cnt = cnt < 0 ? 0 : cnt > n ? n : cnt;
    const long long base = (long long)set * n;

    float x1[K], y1[K], x2[K], y2[K], area[K], s[K];
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int row = k * T + tid;
        x1[k] = y1[k] = x2[k] = y2[k] = area[k] = s[k] = 0.f;
        if (row < cnt) {
            const float* d = dets + 5 * (base + row);
            x1[k] = d[0]; y1[k] = d[1]; x2[k] = d[2]; y2[k] = d[3]; s[k] = d[4];
            area[k] = (x2[k] - x1[k] + 1.0f) * (y2[k] - y1[k] + 1.0f);
            s_box[row] = make_float4(x1[k], y1[k], x2[k], y2[k]);
            live |= 1u << k;
        }
    }
    __syncthreads();

    int emitted = 0;
    for (int t = 0; t < cnt; ++t) {
        unsigned long long key = 0ull;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (live >> k & 1u) {
                const unsigned long long mine = soft_key(s[k], k * T + tid);
                key = mine > key ? mine : key;
            }
        key = wave_max(key);
        if (WAVES > 1) {
            unsigned long long* part = s_part + (t & 1) * WAVES;
            if ((tid & 63) == 0) part[tid >> 6] = key;
            __syncthreads();
            key = part[0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) key = part[w] > key ? part[w] : key;
        }
        if (key == 0ull) break;                               // the same value in every thread
        const int m = (int)(0xFFFFFFFFu - (unsigned)key);
        const float sm = soft_key_score(key);
        const float4 bm = s_box[m];
        if (tid < 6) {
            if (tid < 5) out_dets[5 * (base + t) + tid] = tid == 0 ? bm.x : tid == 1 ? bm.y : tid == 2 ? bm.z : tid == 3 ? bm.w : sm;
            else out_src[base + t] = m;
        }
        if (all_scores && tid == 6) all_scores[base + t] = sm;
        emitted = t + 1;
        if (tid == m % T) live &= ~(1u << (m / T));           // retire the pick
        const float area_m = (bm.z - bm.x + 1.0f) * (bm.w - bm.y + 1.0f);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!(live >> k & 1u)) continue;
            const float w = fmaxf(0.0f, fminf(bm.z, x2[k]) - fmaxf(bm.x, x1[k]) + 1.0f);
            const float h = fmaxf(0.0f, fminf(bm.w, y2[k]) - fmaxf(bm.y, y1[k]) + 1.0f);
            const float inter = w * h;
            const float iou = inter / ((area_m + area[k]) - inter);
            bool applied;
            if (METHOD == M_GAUSSIAN) {
                applied = iou == iou;                         // 0 / 0 of two zero-area boxes: no decay
                if (applied && iou != 0.0f)                   // exp(-0) is exactly 1: the score stays as it is
                    s[k] = (float)((double)s[k] * exp(-((double)iou * (double)iou) / (double)sigma));
            } else {
                applied = iou > nt;
                if (METHOD == M_LINEAR && applied) s[k] = s[k] * (1.0f - iou);
            }
            if (applied && (METHOD == M_HARD || s[k] < min_score)) live &= ~(1u << k);
        }
    }
    if (all_scores)
        for (int t = emitted + tid; t < n; t += T) all_scores[base + t] = -INFINITY;
    if (tid == 0) {
        out_num[set] = emitted;
        if (total) atomicAdd(total, emitted);                 // an integer sum: the same whatever the order
    }
}

template <int METHOD, int K, int WAVES>
int32_t launch_form(const float* dets, const int* counts, int n, float nt, float sigma, float min_score, float* out_dets,
                    int* out_src, int* out_num, float* all_scores, int* total, const SoftNmsPlan& pl, hipStream_t st) {
    if (pl.lds > 48 * 1024)       // the most this form ever asks for: SOFT_NMS_MAX_N boxes and the slots
        I2V_ALLOW_LDS("soft_nms_kernel", (size_t)SOFT_NMS_MAX_N * 16 + 2 * WAVES * 8, soft_nms_kernel<METHOD, K, WAVES>);
    soft_nms_kernel<METHOD, K, WAVES><<<dim3(pl.grid), dim3(pl.threads), pl.lds, st>>>(dets, counts, n, nt, sigma, min_score, out_dets,
                                                                                   out_src, out_num, all_scores, total);
    return I2V_OK;
}

template <int METHOD>
int32_t launch_method(const float* dets, const int* counts, int n, float nt, float sigma, float min_score, float* out_dets,
                      int* out_src, int* out_num, float* all_scores, int* total, const SoftNmsPlan& pl, hipStream_t st) {
#define SOFT_FORM(K, W)                                                                                                        \
    if (pl.rows == K && pl.waves == W)                                                                                         \
        return launch_form<METHOD, K, W>(dets, counts, n, nt, sigma, min_score, out_dets, out_src, out_num, all_scores, total, pl, st);
    SOFT_FORM(1, 1) SOFT_FORM(2, 1) SOFT_FORM(4, 1) SOFT_FORM(5, 1) SOFT_FORM(8, 1)
    SOFT_FORM(1, SOFT_NMS_BLOCK_WAVES) SOFT_FORM(2, SOFT_NMS_BLOCK_WAVES) SOFT_FORM(4, SOFT_NMS_BLOCK_WAVES)
#undef SOFT_FORM
    i2v_set_error("soft_nms: no kernel for %d rows per lane in %d waves", pl.rows, pl.waves);
    return I2V_ERR_ARG;
}
}  // namespace

int32_t launch_soft_nms(const float* dets, const int* counts, int n_set, int n, int method, float nt, float sigma,
                        float min_score, float* out_dets, int* out_src, int* out_num, float* all_scores, int* total,
                        hipStream_t st) {
    I2V_CHECK_ARG(method == M_HARD || method == M_LINEAR || method == M_GAUSSIAN, "soft_nms: method must be I2V_SOFT_NMS_HARD, _LINEAR or _GAUSSIAN");
    I2V_CHECK_ARG(method != M_GAUSSIAN || sigma > 0.f, "soft_nms: sigma must be positive");
    const SoftNmsPlan pl = plan_soft_nms(n_set, n);
    I2V_CHECK_ARG(pl.status == PLAN_OK, "%s", soft_nms_refusal_text(pl.status));
    switch (method) {
    case M_HARD: return launch_method<M_HARD>(dets, counts, n, nt, sigma, min_score, out_dets, out_src, out_num, all_scores, total, pl, st);
    case M_LINEAR: return launch_method<M_LINEAR>(dets, counts, n, nt, sigma, min_score, out_dets, out_src, out_num, all_scores, total, pl, st);
    default: return launch_method<M_GAUSSIAN>(dets, counts, n, nt, sigma, min_score, out_dets, out_src, out_num, all_scores, total, pl, st);
    }
}

extern "C" size_t i2v_soft_nms_workspace_bytes(int32_t n_set, int32_t n) {
    (void)n_set; (void)n;
    return 0;                     // the sets live in registers and LDS
}

extern "C" int32_t i2v_soft_nms(const float* dets, const int32_t* counts, int32_t n_set, int32_t n, int32_t method, float nt,
                                float sigma, float min_score, float* out_dets, int32_t* out_src, int32_t* out_num, void* ws,
                                size_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    I2V_CHECK_ARG(n_set > 0 && n >= 0, "soft_nms: bad shape");
    I2V_CHECK_ARG(out_num, "soft_nms: null out_num");
    I2V_CHECK_ARG(n <= SOFT_NMS_MAX_N, "%s", soft_nms_refusal_text(SOFT_NMS_ROWS));
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        hipMemsetAsync(out_num, 0, sizeof(int) * n_set, st);
        return I2V_OK;
    }
    I2V_CHECK_ARG(dets && out_dets && out_src, "soft_nms: null pointer");
    const int32_t rc = launch_soft_nms(dets, counts, n_set, n, method, nt, sigma, min_score, out_dets, out_src, out_num, nullptr,
                                       nullptr, st);
    if (rc) return rc;
    I2V_CHECK_LAUNCH("soft_nms");
    return I2V_OK;
}

// plan_soft_nms as numbers (include/i2vsgg_hip.h has the field order)
extern "C" int32_t i2v_soft_nms_plan(int32_t n_set, int32_t n, int32_t* out, int32_t n_out) {
    I2V_CHECK_ARG(out && n_out >= I2V_SOFT_NMS_PLAN_FIELDS, "soft_nms_plan: out needs room for I2V_SOFT_NMS_PLAN_FIELDS values");
    I2V_CHECK_ARG(n_set > 0 && n > 0, "soft_nms_plan: bad shape");
    const SoftNmsPlan pl = plan_soft_nms(n_set, n);
    const int32_t v[I2V_SOFT_NMS_PLAN_FIELDS] = {pl.status, pl.form, pl.waves, pl.rows, (int32_t)pl.grid, pl.threads, (int32_t)pl.lds};
    std::copy(v, v + I2V_SOFT_NMS_PLAN_FIELDS, out);
    return I2V_OK;
}
