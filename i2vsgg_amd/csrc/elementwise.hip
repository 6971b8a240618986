// The passes of a training step that are no GEMM: the stem's 3x3 stride-2 max pool, the optimizers (SGD with momentum
// for one tensor or a table of tensors, torch.optim.Adam for a table), and the backward epilogue of a conv / linear layer
// (ReLU mask, frozen-BN scale, bias-gradient column sums).  Streaming kernels, bound by HBM; no matrix cores.
// The column sums of epilogue_bwd are ordered (bit-reproducible) through the caller's split workspace: in one or two
// levels inside the kernel (colsum_finish4), or, for N % 4 != 0, by the scalar reduce pass of wgrad.hip.
#include "conv_common.h"

using namespace convplan;

namespace {

// ---------------------------------------------------------------- small elementwise pieces
__global__ void maxpool3x3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int* __restrict__ arg, int B,
                                    int H, int W, int C, int Ho, int Wo) {
    const long long total = (long long)B * Ho * Wo * (C / 4);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (i % (C / 4)) * 4;
        long long t = i / (C / 4);
        const int ox = t % Wo; t /= Wo;
        const int oy = t % Ho;
        const int b = t / Ho;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        int4 a = make_int4(-1, -1, -1, -1);
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 + ky;
            if (iy >= H) break;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 + kx;
                if (ix >= W) break;
                float4 v = *(const float4*)(x + (((long long)b * H + iy) * W + ix) * C + c);
                const int id = iy * W + ix;
                if (v.x > m.x) { m.x = v.x; a.x = id; }
                if (v.y > m.y) { m.y = v.y; a.y = id; }
                if (v.z > m.z) { m.z = v.z; a.z = id; }
                if (v.w > m.w) { m.w = v.w; a.w = id; }
            }
        }
        const long long o = (((long long)b * Ho + oy) * Wo + ox) * C + c;
        *(float4*)(y + o) = m;
        if (arg) *(int4*)(arg + o) = a;
    }
}

__global__ void sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    long long n4, long long n, float lr, float mom, float wd) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4;
         i += (long long)gridDim.x * blockDim.x) {
        float4 pv = ((float4*)p)[i], gv = ((const float4*)g)[i], mv = ((float4*)m)[i];
        mv.x = mom * mv.x + (gv.x + wd * pv.x); mv.y = mom * mv.y + (gv.y + wd * pv.y);
        mv.z = mom * mv.z + (gv.z + wd * pv.z); mv.w = mom * mv.w + (gv.w + wd * pv.w);
        pv.x -= lr * mv.x; pv.y -= lr * mv.y; pv.z -= lr * mv.z; pv.w -= lr * mv.w;
        ((float4*)m)[i] = mv;
        ((float4*)p)[i] = pv;
    }
    // tail (n not a multiple of 4)
    const long long i = n4 * 4 + blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n) {
        float mv = mom * m[i] + (g[i] + wd * p[i]);
        m[i] = mv;
        p[i] -= lr * mv;
    }
}

// Many small tensors in one launch (the per-tensor launch, not the bytes, is what a 300-float bias costs).  The
// table travels by value in the kernel arguments; block b works on the tensor whose block range contains it.
constexpr int SGD_MULTI_MAX = 48;
struct SgdMulti {
    float* p[SGD_MULTI_MAX]; const float* g[SGD_MULTI_MAX]; float* m[SGD_MULTI_MAX];
    long long n[SGD_MULTI_MAX];
    float lr[SGD_MULTI_MAX], wd[SGD_MULTI_MAX];
    int first_block[SGD_MULTI_MAX + 1];
    int count;
    float mom;
};
constexpr int SGD_MULTI_PER_BLOCK = 256 * 16;     // elements per block
__global__ void __launch_bounds__(256) sgd_momentum_multi_kernel(const SgdMulti t) {
    int k = 0;
    while (k + 1 < t.count && (int)blockIdx.x >= t.first_block[k + 1]) ++k;
    const long long base = (long long)(blockIdx.x - t.first_block[k]) * SGD_MULTI_PER_BLOCK;
    float* p = t.p[k]; const float* g = t.g[k]; float* m = t.m[k];
    const float lr = t.lr[k], wd = t.wd[k], mom = t.mom;
    for (int j = threadIdx.x; j < SGD_MULTI_PER_BLOCK; j += 256) {
        const long long i = base + j;
        if (i >= t.n[k]) break;
        const float mv = mom * m[i] + (g[i] + wd * p[i]);       // same order as sgd_momentum_kernel
        m[i] = mv;
        p[i] -= lr * mv;
    }
}

// torch.optim.Adam (amsgrad off) for up to SGD_MULTI_MAX tensors per launch, in torch's operation order:
//   g' = g + wd p;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g' g';  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The step count t lives in DEVICE memory (adam_step_kernel increments it once per optimizer step), so a captured training step
// replays with the right bias corrections.
struct AdamMulti {
    float* p[SGD_MULTI_MAX]; const float* g[SGD_MULTI_MAX]; float* m[SGD_MULTI_MAX]; float* v[SGD_MULTI_MAX];
    long long n[SGD_MULTI_MAX];
    double lr[SGD_MULTI_MAX];
    float wd[SGD_MULTI_MAX];
    int first_block[SGD_MULTI_MAX + 1];
    int count;
    double b1, b2, eps;          // the betas / eps as the host holds them (Python floats are doubles)
    const int* step;
};
__global__ void adam_step_kernel(int* step) { *step += 1; }
__global__ void __launch_bounds__(256) adam_multi_kernel(const AdamMulti t) {
    int k = 0;
    while (k + 1 < t.count && (int)blockIdx.x >= t.first_block[k + 1]) ++k;
    const long long base = (long long)(blockIdx.x - t.first_block[k]) * SGD_MULTI_PER_BLOCK;
    float* p = t.p[k]; const float* g = t.g[k]; float* m = t.m[k]; float* v = t.v[k];
    // torch.optim.Adam (_single_tensor_adam) computes the scalars of a step on the host in DOUBLE: bias_correction = 1 - beta ** step,
    // step_size = lr / bias_correction1, bias_correction2_sqrt = bias_correction2 ** 0.5 -- and hands the tensor kernels their
    // float roundings.  The same here, once per workgroup (round-3 advice: powf on float betas is off by ~3e-5 at small t).
    const double st = (double)*t.step;
    const double bc1 = 1.0 - pow(t.b1, st), bc2 = 1.0 - pow(t.b2, st);
    const float step_size = (float)(t.lr[k] / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - t.b1), b2 = (float)t.b2, w2 = (float)(1.0 - t.b2), eps = (float)t.eps, wd = t.wd[k];
    for (int j = threadIdx.x; j < SGD_MULTI_PER_BLOCK; j += 256) {
        const long long i = base + j;
        if (i >= t.n[k]) break;
        const float gp = g[i] + wd * p[i];                    // grad.add(param, alpha=weight_decay)
        const float mv = m[i] + w1 * (gp - m[i]);             // exp_avg.lerp_(grad, 1 - beta1)
        const float vv = b2 * v[i] + w2 * gp * gp;            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        m[i] = mv;
        v[i] = vv;
        p[i] -= step_size * (mv / (sqrtf(vv) / bc2_sqrt + eps));      // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
}

// Ordered finish of per-workgroup column sums (round 5): ``s`` = this workgroup's sum of four columns n..n+3 over ITS rows.
// With a workspace the sums of one column block (blockIdx.y) meet there: every workgroup stores its row of partials (sc1),
// counts its arrival, and the LAST one adds the gridDim.x partials of every column in block order -- eight in flight per round --
// onto gbias: bit-reproducible where fp32 atomics (the workspace-free form) add in arrival order.  Every thread of the
// workgroup must call it (barriers inside); ``live`` = the thread owns four columns.
// Round 6: TWO LEVELS when there are more than kColsumGroup row blocks (netD_style's 37500-row projections keep their hundreds
// of row blocks -- they must stream at full rate -- and were left on atomics): the blocks of a group of kColsumGroup meet first,
// the group's last arriver adds the group's partials in block order and stores the group sum; the last GROUP to finish adds
// the group sums in group order.  Nobody reads more than kColsumGroup + #groups rows, the order of every addition is fixed by
// the block indices.  Counters: cnt[blockIdx.y * (1 + groups)] for the groups' meeting, + 1 + g for group g; rows of partials:
// part[block] then part2 = part + gridDim.x rows: [group].
constexpr int kColsumGroup = 32;
__device__ inline void colsum_finish4(float4 s, int n, int N, bool live, float* __restrict__ gbias, float* part, int* cnt) {
    if (!part) {
        if (live) {
            atomicAdd(gbias + n, s.x); atomicAdd(gbias + n + 1, s.y);
            atomicAdd(gbias + n + 2, s.z); atomicAdd(gbias + n + 3, s.w);
        }
        return;
    }
    constexpr int SC01 = 16;
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc((void*)part, 0, 0x7FFFFFF0, 0x00020000);
    const unsigned rowb = (unsigned)N * 4u, off = (unsigned)n * 4u;
    const int nb = gridDim.x, my = blockIdx.x;
    const int ngroups = (nb + kColsumGroup - 1) / kColsumGroup, grp = my / kColsumGroup;
    const int g0 = grp * kColsumGroup, gn = min(kColsumGroup, nb - g0);          // my group: blocks g0 .. g0 + gn - 1
    int* cbase = cnt + blockIdx.y * (1 + ngroups);
    if (live) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, s), pr, (unsigned)my * rowb + off, 0, SC01);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    __shared__ int cs_last;
    if (threadIdx.x == 0) {
        int* c = ngroups > 1 ? cbase + 1 + grp : cbase;
        const int arrived = __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = arrived == gn - 1;
        if (last) __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cs_last = last;
    }
    __syncthreads();
    if (!cs_last) return;
    // the group's partials in block order (mine from its register); one level: onto gbias directly, as in round 5
    float4 t = ngroups > 1 ? make_float4(0.f, 0.f, 0.f, 0.f) : (live ? *(const float4*)(gbias + n) : make_float4(0.f, 0.f, 0.f, 0.f));
    if (live) {
        for (int b0 = 0; b0 < gn; b0 += 8) {
            float4 u[8];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                u[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                    pr, (b0 + k < gn && g0 + b0 + k != my) ? (unsigned)(g0 + b0 + k) * rowb + off : 0xFFFFFFF0u, 0, SC01));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 v = g0 + b0 + k == my ? s : u[k];       // slots beyond the group were read out of range: zeros
                t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
            }
        }
    }
    if (ngroups == 1) {
        if (live) *(float4*)(gbias + n) = t;
        return;
    }
    // second level: my group's sum to row (nb + grp); the last group to arrive adds the group sums in group order onto gbias
    if (live) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t), pr, (unsigned)(nb + grp) * rowb + off, 0, SC01);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int arrived = __hip_atomic_fetch_add(cbase, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = arrived == ngroups - 1;
        if (last) __hip_atomic_store(cbase, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cs_last = last;
    }
    __syncthreads();
    if (!cs_last || !live) return;
    float4 r = *(const float4*)(gbias + n);
    for (int b0 = 0; b0 < ngroups; b0 += 8) {
        float4 u[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            u[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                pr, (b0 + k < ngroups && b0 + k != grp) ? (unsigned)(nb + b0 + k) * rowb + off : 0xFFFFFFF0u, 0, SC01));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 v = b0 + k == grp ? t : u[k];
            r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
        }
    }
    *(float4*)(gbias + n) = r;
}

// g_pre = gy * (y > 0); g = g_pre * scale[n]; gbias[n] += sum_m g_pre.  One streaming pass: thread = 4 columns
// (float4), a workgroup covers rows_per_blk rows x 1024 columns; either output may be NULL.
__global__ void __launch_bounds__(256)
epilogue_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y, const float* __restrict__ scale,
                    float* __restrict__ g, float* __restrict__ gpre, float* __restrict__ gbias, long long M, int N,
                    int relu, int rows_per_blk, float* __restrict__ g_t, float* part, int* cnt) {
    const int n = (blockIdx.y * 256 + threadIdx.x) * 4;
    const bool live = n < N;
    const long long r0 = (long long)blockIdx.x * rows_per_blk;
    const long long r1 = !live ? r0 : (r0 + rows_per_blk < M ? r0 + rows_per_blk : M);
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
    if (scale && live) sc = *(const float4*)(scale + n);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (long long r = r0; r < r1; ++r) {
        float4 v = *(const float4*)(gy + r * N + n);
        if (relu) {
            const float4 yy = *(const float4*)(y + r * N + n);
            v.x = yy.x > 0.f ? v.x : 0.f; v.y = yy.y > 0.f ? v.y : 0.f;
            v.z = yy.z > 0.f ? v.z : 0.f; v.w = yy.w > 0.f ? v.w : 0.f;
        }
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        if (gpre) *(float4*)(gpre + r * N + n) = v;
        if (g) *(float4*)(g + r * N + n) = make_float4(v.x * sc.x, v.y * sc.y, v.z * sc.z, v.w * sc.w);
        if (g_t) {          // the same gradient column-major, (N x M): what a linear layer's dgrad on the wgrad kernel reads
            g_t[(long long)n * M + r] = v.x * sc.x; g_t[(long long)(n + 1) * M + r] = v.y * sc.y;
            g_t[(long long)(n + 2) * M + r] = v.z * sc.z; g_t[(long long)(n + 3) * M + r] = v.w * sc.w;
        }
    }
    if (gbias) colsum_finish4(s, n, N, live, gbias, part, cnt);
}

// Narrow tensors (N <= 1024 columns, tall M: the conv_lo feature maps of the relation head are 16384 x 96):
// the 256 threads split into N/4 column groups x row lanes, a lane strides over the rows of the block, and the
// column sums are reduced across the lanes in LDS -> ONE atomic per column per workgroup.  (With one thread per
// 4 columns only 24 of 256 threads had work and 512 workgroups hammered the same 96 addresses: 58 us.)
__global__ void __launch_bounds__(256)
epilogue_bwd_narrow_kernel(const float* __restrict__ gy, const float* __restrict__ y, const float* __restrict__ scale,
                           float* __restrict__ g, float* __restrict__ gpre, float* __restrict__ gbias, long long M,
                           int N, int relu, int rows_per_blk, float* part, int* cnt) {
    __shared__ float red[256 * 4];
    const int cg = N >> 2;                       // column groups (<= 256)
    const int lanes = 256 / cg;                  // row lanes (>= 1)
    const int c = threadIdx.x % cg, lane = threadIdx.x / cg;
    const int n = c * 4;
    const long long r0 = (long long)blockIdx.x * rows_per_blk;
    const long long r1 = r0 + rows_per_blk < M ? r0 + rows_per_blk : M;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < lanes) {
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
        if (scale) sc = *(const float4*)(scale + n);
#pragma unroll 4
        for (long long r = r0 + lane; r < r1; r += lanes) {
            float4 v = *(const float4*)(gy + r * N + n);
            if (relu) {
                const float4 yy = *(const float4*)(y + r * N + n);
                v.x = yy.x > 0.f ? v.x : 0.f; v.y = yy.y > 0.f ? v.y : 0.f;
                v.z = yy.z > 0.f ? v.z : 0.f; v.w = yy.w > 0.f ? v.w : 0.f;
            }
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            if (gpre) *(float4*)(gpre + r * N + n) = v;
            if (g) *(float4*)(g + r * N + n) = make_float4(v.x * sc.x, v.y * sc.y, v.z * sc.z, v.w * sc.w);
        }
    }
    if (!gbias) return;
    *(float4*)&red[threadIdx.x * 4] = s;
    __syncthreads();
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x < cg) {
        for (int l = 0; l < lanes; ++l) {
            const float4 u = *(const float4*)&red[(l * cg + threadIdx.x) * 4];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
    }
    colsum_finish4(t, (int)(threadIdx.x % cg) * 4, N, threadIdx.x < cg, gbias, part, cnt);
}

__global__ void __launch_bounds__(256)
epilogue_bwd_scalar_kernel(const float* __restrict__ gy, const float* __restrict__ y, const float* __restrict__ scale,
                           float* __restrict__ g, float* __restrict__ gpre, float* __restrict__ gbias, long long M,
                           int N, int relu, int rows_per_blk, float* __restrict__ g_t, float* __restrict__ part) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= N) return;
    const long long r0 = (long long)blockIdx.x * rows_per_blk;
    const long long r1 = r0 + rows_per_blk < M ? r0 + rows_per_blk : M;
    const float sc = scale ? scale[n] : 1.f;
    float s = 0.f;
    for (long long r = r0; r < r1; ++r) {
        float v = gy[r * N + n];
        if (relu && !(y[r * N + n] > 0.f)) v = 0.f;
        s += v;
        if (gpre) gpre[r * N + n] = v;
        if (g) g[r * N + n] = v * sc;
        if (g_t) g_t[(long long)n * M + r] = v * sc;
    }
    if (gbias && part) part[(long long)blockIdx.x * N + n] = s;       // ordered: the row blocks' sums side by side, added in block order by a reduce pass
    else if (gbias) atomicAdd(gbias + n, s);
}

}  // namespace

extern "C" int32_t i2v_epilogue_bwd(const float* gy, const float* y, const float* scale, float* g, float* gpre,
                                    float* gbias, int64_t M, int32_t N, int32_t relu, float* g_t, void* split_ws,
                                    size_t split_ws_bytes, void* stream) {
    I2V_CHECK_ARG(gy && M >= 0 && N > 0, "epilogue_bwd: bad argument");
    I2V_CHECK_ARG(!relu || y, "epilogue_bwd: relu needs y");
    if (M == 0) return I2V_OK;
    const bool vec = (N & 3) == 0;
    const int cols = vec ? 1024 : 256;
    // ordered column sums (round 5): with the caller's split workspace (i2v_conv_fwd's: zeroed counters + slab) the row
    // blocks' partial sums are added in block order by the last block to arrive -- few blocks then, the finisher reads them all
    // ... and small tensors only (at most 2^21 elements: the relation head's layers): a large one (netD_style's 37500 x 2560
    // projections) needs its hundreds of row blocks to stream at full rate (measured: configs[2] 46.3 -> 48.1 ms with every
    // tensor held to <= 32 row blocks), so it keeps the atomics
    // round 6: large tensors too -- they keep their row blocks (full streaming rate) and the sums meet in two levels
    // (colsum_finish4); `small` = the tensors round 5 ordered by cutting them into few row blocks
    const bool want_ord = gbias && vec && g_i2v_tuning[I2V_TUNE_SPLIT_ATOMICS] == 0;
    const bool small = M * (long long)N <= (1ll << 21);
    auto ordered = [&](long long nblk, int ncolblk, float*& part, int*& cnt) {
        part = nullptr; cnt = nullptr;
        if (!want_ord || nblk < 2) return;
        const long long groups = (nblk + kColsumGroup - 1) / kColsumGroup;
        const size_t need = kSplitCounterBytes + (size_t)(nblk + groups) * N * sizeof(float);
        if (!split_ws || (long long)ncolblk * (1 + groups) > kSplitCounters || need > split_ws_bytes || need >= (1ull << 31)) {
            ++g_ordered_fallbacks;
            return;
        }
        cnt = reinterpret_cast<int*>(split_ws);
        part = reinterpret_cast<float*>(static_cast<char*>(split_ws) + kSplitCounterBytes);
    };
    float* part; int* cnt;
    // enough workgroups to cover the chip even for the 64..128-row tensors of the relation head
    int rows = 64;
    while (rows > 4 && (long long)i2v_cdiv(M, rows) * i2v_cdiv(N, cols) < 2 * NUM_CU) rows >>= 1;
    if (vec && N <= 512 && M >= 1024 && !g_t) {
        // tall and narrow: all 256 threads on one row block, one atomic per column per workgroup
        const int lanes = 256 / (N >> 2);
        // few workgroups: same-address atomics retire one per ~150 ns, so 256 contenders cost more than the rows
        int rpb = lanes * 64;
        while (rpb > lanes && i2v_cdiv(M, rpb) < 48) rpb >>= 1;
        if (want_ord && small) while (i2v_cdiv(M, rpb) > 64) rpb <<= 1;  // small tensors: at most 64 partials per column (two groups)
        ordered(i2v_cdiv(M, rpb), 1, part, cnt);
        epilogue_bwd_narrow_kernel<<<(unsigned)i2v_cdiv(M, rpb), 256, 0, (hipStream_t)stream>>>(gy, y, scale, g, gpre,
                                                                                              gbias, M, N, relu, rpb, part, cnt);
        I2V_CHECK_LAUNCH("epilogue_bwd");
        return I2V_OK;
    }
    if (want_ord && vec && small) while (i2v_cdiv(M, rows) > 32 && rows < 1024) rows <<= 1;   // small tensors: at most 32 row blocks (one level)
    dim3 grid(i2v_cdiv(M, rows), i2v_cdiv(N, cols));
    ordered(grid.x, (int)grid.y, part, cnt);
    if (vec) {
        epilogue_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(gy, y, scale, g, gpre, gbias, M, N, relu, rows, g_t, part, cnt);
    } else {
        // N % 4 != 0 (the RPN's 18-channel cls_score): ordered = partial rows + the reduce pass of the filter gradients
        float* sp = nullptr;
        if (gbias && grid.x > 1 && g_i2v_tuning[I2V_TUNE_SPLIT_ATOMICS] == 0) {
            if (split_ws && kSplitCounterBytes + (size_t)grid.x * N * sizeof(float) <= split_ws_bytes)
                sp = reinterpret_cast<float*>(static_cast<char*>(split_ws) + kSplitCounterBytes);
            else ++g_ordered_fallbacks;
        }
        epilogue_bwd_scalar_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(gy, y, scale, g, gpre, gbias, M, N, relu, rows, g_t, sp);
        if (sp) i2v_internal_reduce_scalar(sp, gbias, (int)grid.x, N, 1, (unsigned)i2v_cdiv(N, 256), stream);
    }
    I2V_CHECK_LAUNCH("epilogue_bwd");
    return I2V_OK;
}

extern "C" int32_t i2v_maxpool3x3s2_fwd(const float* x, float* y, int32_t* argmax, int32_t B, int32_t H, int32_t W,
                                        int32_t C, void* stream) {
    I2V_CHECK_ARG(x && y && B > 0 && H >= 3 && W >= 3 && C > 0 && C % 4 == 0, "maxpool: bad argument");
    // ceil_mode, pad 0: Ho = ceil((H-3)/2)+1, and the last window must start inside the input
    int Ho = (H - 3 + 1) / 2 + 1, Wo = (W - 3 + 1) / 2 + 1;
    if ((Ho - 1) * 2 >= H) --Ho;
    if ((Wo - 1) * 2 >= W) --Wo;
    const long long total = (long long)B * Ho * Wo * (C / 4);
    maxpool3x3s2_kernel<<<(int)fmin((double)i2v_cdiv(total, 256), 8192.0), 256, 0, (hipStream_t)stream>>>(
        x, y, argmax, B, H, W, C, Ho, Wo);
    I2V_CHECK_LAUNCH("maxpool3x3s2");
    return I2V_OK;
}

extern "C" int32_t i2v_sgd_momentum_multi(float* const* p, const float* const* g, float* const* m, const int64_t* n,
                                          const float* lr, const float* weight_decay, int32_t count, float momentum,
                                          void* stream) {
    I2V_CHECK_ARG(count >= 0 && (count == 0 || (p && g && m && n && lr && weight_decay)), "sgd_momentum_multi: bad argument");
    for (int32_t c0 = 0; c0 < count; c0 += SGD_MULTI_MAX) {
        SgdMulti t;
        t.count = 0;
        t.mom = momentum;
        int blocks = 0;
        for (int32_t c = c0; c < count && t.count < SGD_MULTI_MAX; ++c) {
            I2V_CHECK_ARG(p[c] && g[c] && m[c] && n[c] >= 0, "sgd_momentum_multi: bad tensor");
            if (n[c] == 0) continue;
            const int k = t.count++;
            t.p[k] = p[c]; t.g[k] = g[c]; t.m[k] = m[c]; t.n[k] = n[c]; t.lr[k] = lr[c]; t.wd[k] = weight_decay[c];
            t.first_block[k] = blocks;
            blocks += (int)i2v_cdiv(n[c], (long long)SGD_MULTI_PER_BLOCK);
        }
        t.first_block[t.count] = blocks;
        if (blocks == 0) continue;
        sgd_momentum_multi_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(t);
        I2V_CHECK_LAUNCH("sgd_momentum_multi");
    }
    return I2V_OK;
}

extern "C" int32_t i2v_adam_step(int32_t* step_counter, void* stream) {
    I2V_CHECK_ARG(step_counter, "adam_step: null counter");
    adam_step_kernel<<<1, 1, 0, (hipStream_t)stream>>>(step_counter);
    I2V_CHECK_LAUNCH("adam_step");
    return I2V_OK;
}

extern "C" int32_t i2v_adam_multi(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                                  const double* lr, const float* weight_decay, int32_t count, double beta1, double beta2,
                                  double eps, const int32_t* step_counter, void* stream) {
    I2V_CHECK_ARG(count >= 0 && step_counter && (count == 0 || (p && g && m && v && n && lr && weight_decay)), "adam_multi: bad argument");
    for (int32_t c0 = 0; c0 < count;) {
        AdamMulti t;
        t.count = 0;
        t.b1 = beta1; t.b2 = beta2; t.eps = eps; t.step = step_counter;
        int blocks = 0;
        int32_t c = c0;
        for (; c < count && t.count < SGD_MULTI_MAX; ++c) {
            I2V_CHECK_ARG(p[c] && g[c] && m[c] && v[c] && n[c] >= 0, "adam_multi: bad tensor");
            if (n[c] == 0) continue;
            const long long nb = i2v_cdiv(n[c], (long long)SGD_MULTI_PER_BLOCK);
            if (t.count && blocks + nb > (1 << 20)) break;        // a very large tensor starts its own launch
            const int k = t.count++;
            t.p[k] = p[c]; t.g[k] = g[c]; t.m[k] = m[c]; t.v[k] = v[c]; t.n[k] = n[c]; t.lr[k] = lr[c]; t.wd[k] = weight_decay[c];
            t.first_block[k] = blocks;
            blocks += (int)nb;
        }
        c0 = c;
        t.first_block[t.count] = blocks;
        if (blocks == 0) continue;
        adam_multi_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(t);
        I2V_CHECK_LAUNCH("adam_multi");
    }
    return I2V_OK;
}

extern "C" int32_t i2v_sgd_momentum(float* p, const float* g, float* m, int64_t n, float lr, float momentum,
                                    float weight_decay, void* stream) {
    I2V_CHECK_ARG(p && g && m && n >= 0, "sgd_momentum: bad argument");
    if (n == 0) return I2V_OK;
    const long long n4 = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) ? 0 : n / 4;
    long long work = n4 > 0 ? n4 : n;
    int grid = (int)fmin((double)i2v_cdiv(work, 256), 8192.0);
    if (n4 == 0) grid = i2v_cdiv(n, 256);
    sgd_momentum_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(p, g, m, n4, n, lr, momentum, weight_decay);
    I2V_CHECK_LAUNCH("sgd_momentum");
    return I2V_OK;
}
