// The library's one sort: a segmented bitonic sort of unsigned 64-bit keys, ascending, in place (sort.h), and the float front
// end i2v_sort_desc on top of it.  Users: the RPN proposal path (rpn.hip), the detector's eval post-processing and the relation
// triplet ranking (det_post.hip, through i2v_sort_desc) and the detection evaluation's curve (det_eval.hip, keys of its own).
#include "sort.h"

namespace {
// all stages with partner distance < SORT_TILE, for k from k_lo up to k_hi (inclusive).  The loop counter is unsigned:
// k_hi may be 2^30 (det_eval.hip allows 2^30 detections), and an int would wrap at the shift that has to end the loop.
__global__ void __launch_bounds__(SORT_THREADS)
sort_local(unsigned long long* __restrict__ data, int P, int k_lo, int k_hi) {
    __shared__ unsigned long long s[SORT_TILE];
    const long long base = (long long)blockIdx.y * P + (long long)blockIdx.x * SORT_TILE;
    for (int i = threadIdx.x; i < SORT_TILE; i += SORT_THREADS) s[i] = data[base + i];
    __syncthreads();
    const int gbase = blockIdx.x * SORT_TILE;
    for (unsigned k = k_lo; k <= (unsigned)k_hi; k <<= 1) {
        int j0 = (k >> 1) < SORT_TILE ? (int)(k >> 1) : (SORT_TILE >> 1);
        for (int j = j0; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < SORT_TILE / 2; t += SORT_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // lower index of the pair
                const bool asc = (((gbase + i) & k) == 0);
                const unsigned long long a = s[i], b = s[i | j];
                if ((a > b) == asc) { s[i] = b; s[i | j] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < SORT_TILE; i += SORT_THREADS) data[base + i] = s[i];
}

__global__ void sort_global_step(unsigned long long* __restrict__ data, int P, int k, int j) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P / 2) return;
    unsigned long long* d = data + (long long)blockIdx.y * P;
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const bool asc = ((i & k) == 0);
    const unsigned long long a = d[i], b = d[i | j];
    if ((a > b) == asc) { d[i] = b; d[i | j] = a; }
}

// ------------------------------------------------------------------ float front end
// key = ~(order-preserving u32 of the score) << 32 | index: sorting keys ASCENDING gives descending score with ascending
// index on ties; padding keys are all ones.
// -0.0f is mapped as +0.0f, so the two zeros tie as they do in an IEEE comparison (their bit
// patterns alone would rank every +0.0 ahead of every -0.0).  NaN keys land wherever their bits
// put them: their order is unspecified.
__device__ inline unsigned int f2ord(float f) {
    unsigned int u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void sort_make_keys(const float* __restrict__ keys, int n, int P, unsigned long long* __restrict__ out) {
    const int seg = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    unsigned long long k = ~0ull;
    if (i < n) k = ((unsigned long long)~f2ord(keys[(long long)seg * n + i]) << 32) | (unsigned)i;
    out[(long long)seg * P + i] = k;
}

__global__ void sort_emit_order(const unsigned long long* __restrict__ keys, int n, int P, int* __restrict__ order) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    order[(long long)blockIdx.y * n + i] = sort_key_index(keys[(long long)blockIdx.y * P + i]);
}
}  // namespace

// the schedule: every tile on its own, then per doubling of the sorted runs the steps whose partners lie in different tiles
// (one launch each) and the rest of that merge inside the tiles.  k and j are 64 bits wide for P = 2^30, as in sort_local.
void i2v_launch_sort_u64(unsigned long long* keys, int n_seg, int P, hipStream_t st) {
    const dim3 tiles(P / SORT_TILE, n_seg), pairs(i2v_cdiv(P / 2, 256), n_seg);
    sort_local<<<tiles, SORT_THREADS, 0, st>>>(keys, P, 2, SORT_TILE);
    for (long long k = (long long)SORT_TILE * 2; k <= P; k <<= 1) {
        for (long long j = k >> 1; j >= SORT_TILE; j >>= 1)
            sort_global_step<<<pairs, 256, 0, st>>>(keys, P, (int)k, (int)j);
        sort_local<<<tiles, SORT_THREADS, 0, st>>>(keys, P, (int)k, (int)k);
    }
}

int i2v_launch_sort_desc(const float* keys, int n_seg, int n, unsigned long long* buf, hipStream_t st) {
    const int P = sort_padded(n);
    sort_make_keys<<<dim3(i2v_cdiv(P, 256), n_seg), 256, 0, st>>>(keys, n, P, buf);
    i2v_launch_sort_u64(buf, n_seg, P, st);
    return P;
}

extern "C" size_t i2v_sort_desc_workspace_bytes(int32_t n_seg, int32_t n) {
    if (n_seg <= 0 || n <= 0) return 256;
    return i2v_align((size_t)n_seg * sort_padded(n) * 8);
}

extern "C" int32_t i2v_sort_desc(const float* keys, int32_t n_seg, int32_t n, int32_t* order, void* ws,
                                 size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_seg > 0 && n >= 0, "sort_desc: bad shape");
    if (n == 0) return I2V_OK;
    I2V_CHECK_ARG(keys && order, "sort_desc: null pointer");
    I2V_CHECK_ARG(n <= (1 << 24), "sort_desc: n too large");
    if (!ws || ws_bytes < i2v_sort_desc_workspace_bytes(n_seg, n)) {
        i2v_set_error("sort_desc: workspace too small");
        return I2V_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    int P = i2v_launch_sort_desc(keys, n_seg, n, (unsigned long long*)ws, st);
    sort_emit_order<<<dim3(i2v_cdiv(n, 256), n_seg), 256, 0, st>>>((unsigned long long*)ws, n, P, order);
    I2V_CHECK_LAUNCH("sort_desc");
    return I2V_OK;
}
