// Video relation features (lib/utils.py:100-132, generate_static_relation_feat): one feature vector per video relation, the
// mean of the per-frame pair features (pre_feat) its members point at.  The rules are stated once, in
// i2vsgg_amd/relation_features.py; the host form there (pool_arrays_host) adds the same float32 values in the same order, so
// device and host agree bit for bit (the library is built with -ffp-contract=off -fno-fast-math).  No floating-point atomics,
// no LDS, no barrier: a relation belongs to one wave, its rows are added in member order, two runs give the same bits.
#include "table_common.h"

#define RF_WAVES 4           // relations of one workgroup, one per wave; the waves never meet
#define RF_BATCH 4           // rows whose loads are in flight together (the adds stay in member order)
#define RF_SLOTS 2           // column groups of one lane per pass: columns (lane + 64 s) * V .. + V, V floats wide

template <int V> struct RfVec;
template <> struct RfVec<4> { typedef float4 type; };
template <> struct RfVec<1> { typedef float type; };

__device__ __forceinline__ void rf_add(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void rf_add(float& a, const float& b) { a += b; }
// one float32 division per column: the fp64 quotient of two float32 values rounded once is that division (53 >= 2 * 24 + 2)
__device__ __forceinline__ float rf_div1(float a, double n) { return (float)((double)a / n); }
__device__ __forceinline__ float4 rf_div(const float4& a, double n) {
    return make_float4(rf_div1(a.x, n), rf_div1(a.y, n), rf_div1(a.z, n), rf_div1(a.w, n));
}
__device__ __forceinline__ float rf_div(const float& a, double n) { return rf_div1(a, n); }
__device__ __forceinline__ float4 rf_zero(const float4&) { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float rf_zero(const float&) { return 0.0f; }

// the row of member i, or -1 for a member without a slot; the tables were validated before (rf_validate)
__device__ __forceinline__ int rf_row(const int* __restrict__ slot_off, const int* __restrict__ mem_slot,
                                      const int* __restrict__ mem_idx, int i, int m1) {
    if (i >= m1) return -1;
    const int s = mem_slot[i];
    return s < 0 ? -1 : slot_off[s] + mem_idx[i];
}

// Every table entry of the relation against the array sizes, each before anything is read through it: mem_off against
// n_members by the caller, mem_slot against n_slots, slot_off against n_rows, mem_idx against its slot.  Returns the number of
// valid members, or -1 for a malformed relation; the same value in every lane.
__device__ __forceinline__ int rf_validate(const int* __restrict__ slot_off, const int* __restrict__ mem_slot,
                                           const int* __restrict__ mem_idx, int m0, int m1, int n_rows, int n_slots, int lane) {
    int bad = 0, cnt = 0;
    for (int i = m0 + lane; i < m1; i += I2V_WAVE) {
        const int s = mem_slot[i];
        if (s == -1) continue;
        if (s < -1 || s >= n_slots) {
            bad = 1;
            continue;
        }
        const int b = slot_off[s], e = slot_off[s + 1];
        if (i2v_range_bad(b, e, n_rows)) {
            bad = 1;
            continue;
        }
        const int k = mem_idx[i];
        if (k < 0 || k >= e - b) bad = 1;
        else ++cnt;
    }
    if (__ballot(bad) != 0ull) return -1;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);              // integers: the order plays no part
    return cnt;
}

// One wave per relation.  Lane l owns the column groups l and l + 64 of a pass (a pass is 128 V columns: 512 with 16-byte
// loads, so dim 300 = 75 float4 is one pass); a wider dim takes further passes over the member list.  The members are
// resolved 64 at a time, one per lane; the valid ones are walked in member order through the ballot mask, their rows handed
// to the whole wave by v_readlane.
template <int V>
__global__ void __launch_bounds__(RF_WAVES * I2V_WAVE)
relation_feature_pool_kernel(const float* __restrict__ feat, const int* __restrict__ slot_off, const int* __restrict__ mem_off,
                             const int* __restrict__ mem_slot, const int* __restrict__ mem_idx, int n_rows, int n_slots,
                             int n_relations, int n_members, int dim, float* __restrict__ pooled, int* __restrict__ count,
                             int* status) {
    typedef typename RfVec<V>::type vec;
    const int lane = threadIdx.x & (I2V_WAVE - 1);
    const int r = blockIdx.x * RF_WAVES + (threadIdx.x >> 6);
    if (r >= n_relations) return;                                            // a whole wave leaves: no barrier follows
    const int m0 = mem_off[r], m1 = mem_off[r + 1];
    int n = -1;
    if (!i2v_range_bad(m0, m1, n_members)) n = rf_validate(slot_off, mem_slot, mem_idx, m0, m1, n_rows, n_slots, lane);
    if (n < 0) {                                                             // a malformed relation: say so, read nothing more
        if (lane == 0) atomicMax(status, r + 1);
        n = 0;
    }
    if (lane == 0) count[r] = n;
    const int groups = dim / V;                                              // column groups of a row
    const vec* __restrict__ src = (const vec*)feat;
    vec* __restrict__ dst = (vec*)(pooled + (size_t)r * dim);
    const double dn = (double)n;
    for (int g0 = 0; g0 < groups; g0 += RF_SLOTS * I2V_WAVE) {
        const int ga = g0 + lane, gb = g0 + I2V_WAVE + lane;
        const bool ina = ga < groups, inb = gb < groups;
        vec a0, a1;
        a0 = a1 = rf_zero(a0);
        bool have = false;                                                   // wave-uniform: a valid row has been seen
        for (int c = m0; n > 0 && c < m1; c += I2V_WAVE) {
            const int row = rf_row(slot_off, mem_slot, mem_idx, c + lane, m1);
            unsigned long long mask = __ballot(row >= 0);
            while (mask) {
                int rows[RF_BATCH];
                int nb = 0;
#pragma unroll
                for (int k = 0; k < RF_BATCH; ++k) {
                    rows[k] = 0;
                    if (mask) {
                        rows[k] = __builtin_amdgcn_readlane(row, __builtin_ctzll(mask));
                        mask &= mask - 1;
                        nb = k + 1;
                    }
                }
                vec va[RF_BATCH], vb[RF_BATCH];
#pragma unroll
                for (int k = 0; k < RF_BATCH; ++k) {                         // the loads of the batch, all before the first add
                    va[k] = vb[k] = rf_zero(a0);
                    if (k < nb) {
                        const vec* p = src + (size_t)rows[k] * groups;
                        if (ina) va[k] = p[ga];
                        if (inb) vb[k] = p[gb];
                    }
                }
#pragma unroll
                for (int k = 0; k < RF_BATCH; ++k) {                         // one add per row, in member order
                    if (k < nb) {
                        if (have) {
                            rf_add(a0, va[k]);
                            rf_add(a1, vb[k]);
                        } else {                                             // the sum starts from the first row: -0.0 survives
                            a0 = va[k];
                            a1 = vb[k];
                            have = true;
                        }
                    }
                }
            }
        }
        if (ina) dst[ga] = have ? rf_div(a0, dn) : rf_zero(a0);
        if (inb) dst[gb] = have ? rf_div(a1, dn) : rf_zero(a1);
    }
}

extern "C" size_t i2v_relation_feature_pool_workspace_bytes(int32_t n_relations) {
    (void)n_relations;
    return I2V_STATUS_BYTES;                                                 // the status word
}

extern "C" int32_t i2v_relation_feature_pool(const float* feat, const int32_t* slot_off, const int32_t* mem_off,
                                             const int32_t* mem_slot, const int32_t* mem_idx, int32_t n_rows, int32_t n_slots,
                                             int32_t n_relations, int32_t n_members, int32_t dim, float* pooled, int32_t* count,
                                             void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_rows >= 0 && n_slots >= 0 && n_relations >= 0 && n_members >= 0, "relation_feature_pool: negative count");
    I2V_CHECK_ARG(dim > 0, "relation_feature_pool: dim must be positive (got %d)", dim);
    I2V_CHECK_ARG(slot_off && mem_off, "relation_feature_pool: null pointer");
    I2V_CHECK_ARG(n_rows == 0 || feat, "relation_feature_pool: null pointer");
    I2V_CHECK_ARG(n_members == 0 || (mem_slot && mem_idx), "relation_feature_pool: null pointer");
    I2V_CHECK_ARG(n_relations == 0 || (pooled && count), "relation_feature_pool: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_relation_feature_pool_workspace_bytes(n_relations),
                  "relation_feature_pool: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "relation_feature_pool: clearing the status word failed");
    if (n_relations == 0) return I2V_OK;
    const int blocks = i2v_cdiv(n_relations, RF_WAVES);
    // 16-byte loads need rows that start on 16 bytes: dim a multiple of 4 and both bases aligned
    const bool wide = dim % 4 == 0 && ((uintptr_t)feat & 15) == 0 && ((uintptr_t)pooled & 15) == 0;
    if (wide)
        relation_feature_pool_kernel<4><<<blocks, RF_WAVES * I2V_WAVE, 0, st>>>(feat, slot_off, mem_off, mem_slot, mem_idx, n_rows,
                                                                               n_slots, n_relations, n_members, dim, pooled,
                                                                               count, (int*)ws);
    else
        relation_feature_pool_kernel<1><<<blocks, RF_WAVES * I2V_WAVE, 0, st>>>(feat, slot_off, mem_off, mem_slot, mem_idx, n_rows,
                                                                               n_slots, n_relations, n_members, dim, pooled,
                                                                               count, (int*)ws);
    I2V_CHECK_LAUNCH("relation_feature_pool");
    return I2V_OK;
}
