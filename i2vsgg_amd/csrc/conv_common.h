// What conv.hip (forward / data gradient), wgrad.hip (filter gradient) and elementwise.hip (pool, optimizers, backward
// epilogue) share, and nothing else: anything one file uses alone lives in that file.  Kernels and their parameter structs
// stay in the anonymous namespace of the file that launches them.
#pragma once
#include "common.h"
#include "conv_plan.h"
#include <algorithm>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;

// One 16-byte-per-lane LDS-DMA request (conv_gemm_f32<.., STG>, conv_wgrad2_f32<.., DMA>): global memory to LDS at the
// wave-uniform base ``dst`` + lane x 16 bytes, without passing through registers.
// The requests are inline asm: hipcc counts a builtin LDS-DMA as a pending LDS write and drains vmcnt(0) in front of every
// ds_read.  Its own loads (epilogue operands) may sit in the same queue: returns are in order, so an extra load can only make a
// counted wait wait longer, never shorter.
__device__ inline void lds_dma16(unsigned dst, unsigned voff, __amdgpu_buffer_rsrc_t r, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(dst), "v"(voff), "s"(r), "s"(soff) : "memory");
}

inline int ilog2_exact(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

inline int32_t clamp32(size_t v) { return (int32_t)std::min<size_t>(v, 0x7FFFFFFF); }

inline int check_conv(const char* who, const void* a, const void* b, const void* c, int B, int H, int W, int Cin,
                      int Cout, int KH, int KW, int stride, int pad) {
    if (!a || !b || !c) { i2v_set_error("%s: null pointer", who); return I2V_ERR_ARG; }
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) {
        i2v_set_error("%s: bad shape", who); return I2V_ERR_ARG;
    }
    if (Cin % 4) { i2v_set_error("%s: Cin must be a multiple of 4 (pad the stem input to 4 channels)", who); return I2V_ERR_ARG; }
    if ((H + 2 * pad - KH) < 0 || (W + 2 * pad - KW) < 0) { i2v_set_error("%s: kernel larger than input", who); return I2V_ERR_ARG; }
    return I2V_OK;
}

// unsupported outcomes of a plan as the library's error
inline int plan_error(int status, const convplan::ConvShape& s) {
    using namespace convplan;
    if (status == PLAN_TAP_TABLE) i2v_set_error("conv: filter %dx%dx%d too large for the tap table", s.KH, s.KW, s.Cin);
    else if (status == PLAN_OPERAND_2GIB) i2v_set_error("conv: operand larger than 2 GiB (32-bit buffer offsets)");
    else if (status == PLAN_ROW_SCALE_NEEDS_V2) i2v_set_error("conv_wgrad_scaled: shape outside the v2 kernel (Cout % 4, 2 GiB operands)");
    else if (status == PLAN_FUSED_NEEDS_SPLIT) i2v_set_error("conv_wgrad_sgd: shape needs a split over pixels; use i2v_conv_wgrad + i2v_sgd_momentum");
    return status == PLAN_OK ? I2V_OK : I2V_ERR_UNSUPPORTED;
}

// Host state, defined once in conv.hip.
extern unsigned long long* g_clk;       // i2v_conv_debug_clock(): the diagnostic instantiations stamp into it
extern int g_ablate;                    // i2v_conv_set_tile(): ablation bits of the diagnostic instantiations
extern int g_ordered_fallbacks;         // i2v_ordered_fallbacks(): counted by the launches, never by the planning entry points

// wgrad.hip, for winograd.hip: the ordered 36-plane filter gradient of the Winograd domain
int32_t i2v_internal_gemm_tn_batched_parts(const float* x, const float* gy, float* parts, int32_t M, int32_t N, int32_t K,
                                           int32_t nbatch, long long stride_x, long long stride_gy, int cap, int* splits, void* stream);
int32_t i2v_internal_reduce_parts(float* parts, int nparts, int planes, long long nk, void* stream);
// wgrad.hip, for elementwise.hip: out[e] = (acc ? out[e] : 0) + part[0][e] + part[1][e] + ... in part order, e < n, on ``blocks``
// workgroups (wgrad_reduce_scalar_kernel: the ordered column sums of i2v_epilogue_bwd for N % 4 != 0)
void i2v_internal_reduce_scalar(const float* part, float* out, int nparts, long long n, int acc, unsigned blocks, void* stream);
