// fp32 implicit-GEMM convolution / linear layers on the CDNA4 matrix cores: the forward pass and the data gradient.
//
//   y[m][n] = epi( sum_k  A[m][k] * Wt[n][k] )      m = (b,oy,ox) output pixel
//                                                     k = (ky,kx,c) filter tap, c fastest
// conv_igemm_f32 never materialises A: each workgroup gathers its BM x 32 slice of the im2col matrix straight from the
// NHWC activation (16 B per lane, channel-contiguous) through a per-filter tap table, stages it in LDS next to the
// BN x 32 weight slice, and the waves feed v_mfma_f32_16x16x4_f32 (exact fp32, fp32 accumulate) from ds_read_b128
// fragments.  LDS rows are 128 B, unpadded, the 16-B column XOR-swizzled by the row.  conv_gemm_f32 is the
// specialisation for operands that ARE matrices (1x1 stride-1 layers, linear layers, Winograd planes): no tap table,
// a register epilogue, an intra-workgroup K split (KG) and LDS-DMA staging (STG).
// The frozen-BatchNorm scale/shift, the bias, the residual add, the ReLU and a data gradient's ReLU mask are fused
// into the accumulator epilogue, so a Bottleneck is 3-4 launches instead of ~10.  A data gradient is the same GEMM on
// a flipped / transposed filter (weight_dgrad_layout, conv_dgrad_impl).  What a launch does -- tile, split, finish,
// form -- is planned in conv_plan.h; run_conv binds pointers, clears and switches on the plan.
// The filter gradient is wgrad.hip; the pool, the optimizers and the backward epilogue are elementwise.hip.
#include "conv_common.h"

using namespace convplan;

// Host state that wgrad.hip and elementwise.hip see too (conv_common.h).
int g_ablate = 0;
unsigned long long* g_clk = nullptr;   // i2v_conv_debug_clock()
int g_ordered_fallbacks = 0;           // i2v_ordered_fallbacks(): reductions asked to be ordered that ran on fp32 atomics

namespace {

struct ConvP {
    const float* x; const float* w; const float* scale; const float* shift; const float* res; float* y;
    const float* mask;           // I2V_EPI_MASK: y = mask > 0 ? y : 0, same shape as y (the ReLU of the tensor a data gradient flows into)
    int B, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;    // pad = top padding; may be negative (a crop)
    int pad_x;                   // left padding (run_conv callers set both; the sub-filters of a strided dgrad differ)
    int M, N, K;                 // GEMM sizes
    int flags;
    int splitk, k_per_split;     // k_per_split multiple of BK
    int ostride;                 // output pixel stride (dgrad of strided 1x1): y is (B,Ho*os..,Wo*os..,N)
    int Hy, Wy;                  // spatial size of the y buffer
    int lgCin;                   // log2(Cin) if power of two else -1
    int reserved0;               // unused (held the forced tile index; kept so that the argument offsets stay)
    unsigned x_bytes, w_bytes;   // sizes of x and w for the buffer descriptors (< 2 GiB each)
    int ablate;                  // diagnostic (i2v_conv_set_tile bits 10-11): 1 = skip staging in the K loop, 2 = skip MFMAs
    int ktab_entries;            // tap-table entries in LDS (>= 1; K/4 rounded up to whole stages for KxK filters)
    int reserved1;               // unused (held the plan-only mode; kept so that the argument offsets stay)
    unsigned long long* clk;     // diagnostic only (i2v_conv_debug_clock): per-workgroup {shader cycles, 100 MHz ticks}
    float* ws;                   // split-K partial tiles [split][tile][BM*BN] (nullptr: fp32 atomics into y)
    int* cnt;                    // split-K arrival counters, one per tile, zero between launches
    int nbatch;                  // > 1: blockIdx.z selects one of nbatch independent GEMMs (Winograd planes)
    long long bsx, bsw, bsy;     // element strides between the batches of x, w and y
};

__device__ inline void split_k(const ConvP& p, int k, int& ky, int& kx, int& c) {
    int kpos;
    if (p.lgCin >= 0) { kpos = k >> p.lgCin; c = k & (p.Cin - 1); }
    else { kpos = k / p.Cin; c = k - kpos * p.Cin; }
    if (p.KW == 1) { ky = kpos; kx = 0; }
    else { ky = kpos / p.KW; kx = kpos - ky * p.KW; }
}

// Tile = (WAVES_M*TM*16) x (WAVES_N*TN*16) outputs, 4 waves, v_mfma_f32_16x16x4_f32.
// A 32-deep K stage is staged per buffer; a lane (i = lane&15, g = lane>>4) owns k = 4g..4g+3 of
// each 16-deep half, so one ds_read_b128 feeds four MFMAs (A and B use the same permutation).
// LDS rows are 128 B, unpadded, with the 16-B column XOR-swizzled by (row>>1)&7: the four
// 16-lane groups of a ds_read_b128 then touch 16 distinct slots of the 256-B bank row.
template <int WAVES_M, int WAVES_N, int TM, int TN>
__global__ void __launch_bounds__(THREADS)
conv_igemm_f32(const ConvP p_in) {
    ConvP p = p_in;
    if (p.nbatch > 1) {              // batched GEMM: same shapes, different operands (uniform: blockIdx.z)
        p.x += (long long)blockIdx.z * p.bsx;
        p.w += (long long)blockIdx.z * p.bsw;
        p.y += (long long)blockIdx.z * p.bsy;
    }
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16;
    constexpr int NT = THREADS;      // threads per workgroup
    constexpr int A_LD = (BM * 8 + THREADS - 1) / THREADS, B_LD = (BN * 8 + THREADS - 1) / THREADS;
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
    // one LDS block: [A stage 0 | A stage 1 | B stage 0 | B stage 1 | tap table]; after the K loop the
    // same bytes stage the BM x BN output tile (row stride BN+4 floats) for a coalesced epilogue
    constexpr int STAGE_FLOATS = 2 * (BM + BN) * BKS;       // + the tap table (p.ktab_entries), dynamic
    constexpr int CROW = BN + 4;
    constexpr int SMEM_FLOATS = STAGE_FLOATS > BM * CROW ? STAGE_FLOATS : BM * CROW;
    // dynamic: max(stage buffers + tap table of THIS filter, epilogue tile).  A 3x3x256 filter needs 2.3 KB of
    // table, not the 10 KB worst case: 39 KB per workgroup instead of 47 -> four workgroups per CU instead of three
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float (*As)[BM * BKS] = reinterpret_cast<float (*)[BM * BKS]>(smem);
    float (*Bs)[BN * BKS] = reinterpret_cast<float (*)[BN * BKS]>(smem + 2 * BM * BKS);
    unsigned* ktab = reinterpret_cast<unsigned*>(smem + 2 * (BM + BN) * BKS);

    const int gtid = threadIdx.x;                 // 0..NT-1
    unsigned long long t0c = 0, t0r = 0;
    if (p.clk) { t0c = __builtin_amdgcn_s_memtime(); t0r = __builtin_amdgcn_s_memrealtime(); }
    const int tid = gtid & (THREADS - 1);         // staging role / epilogue lane
    const int lane = gtid & 63, wave = (gtid >> 6) & 3;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int tiles_n = (p.N + BN - 1) / BN;
    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one), so
    // give each XCD a contiguous run of tiles -- the n-tiles of one m-tile then share an L2 and the
    // activation rows cross the fabric once instead of once per XCD.  (Bijective for any grid size;
    // placement only affects speed.)
    int tile;
    {
        const int nt = gridDim.x, q = nt >> 3, r = nt & 7, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    const int kbeg = blockIdx.y * p.k_per_split;
    const int kend = min(p.K, kbeg + p.k_per_split);

    // staging roles: slot = tid + q*256 -> row = slot>>3, 16-B column = slot&7 (= tid&7 for every q)
    const int kc = tid & 7, kg = kc * 4;
    const bool is1x1 = (p.KH == 1 && p.KW == 1 && p.pad == 0 && p.pad_x == 0);
    const unsigned m1x1 = is1x1 ? 0xFFFFFFFFu : 0u;
    // filter-tap table (only for KHxKW > 1): entry e = k/4 -> (byte offset of tap (ky,kx,c)) << 6 | tap id.
    // Built once per workgroup, so the K loop has no integer division and no per-tap bounds math.
    if (!is1x1) {
        const int n_e = p.ktab_entries;
        for (int e = gtid; e < n_e; e += NT) {
            unsigned v = 0;
            if ((e << 2) < p.K) {
                int ky, kx, c;
                split_k(p, e << 2, ky, kx, c);
                v = (unsigned)((((ky * p.W + kx) * p.Cin + c) * 4) << 6) | (unsigned)(ky * p.KW + kx);
            }
            ktab[e] = v;
        }
    }
    // Loads go through buffer resources: a masked lane gets an out-of-range offset and the hardware
    // returns zeros -- no branches, no select-of-loads, 32-bit byte offsets instead of 64-bit pointers.
    // INV (2 GiB) + any in-tile delta stays beyond every buffer (< 2 GiB), so rows outside the tile need
    // no per-stage test at all.
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    constexpr unsigned INV = 0x80000000u, OOB = 0xFFFFFFF0u;
    unsigned a_off4[A_LD];            // byte offset of x[b][iy0][ix0][0] (mod 2^32: padded taps are masked)
    unsigned a_mlo[A_LD], a_mhi[A_LD];  // bit t: tap t of this output pixel reads inside the image
    const bool ident = is1x1 && p.stride == 1 && p.Ho == p.H && p.Wo == p.W;      // no index arithmetic at all
#pragma unroll
    for (int q = 0; q < A_LD; ++q) {
        const int row = (tid >> 3) + q * (THREADS / 8);
        const int m = m0 + row;
        const bool ok = row < BM && m < p.M;
        const int mm = ok ? m : 0;
        if (ident) {                  // pointwise, stride 1, same grid: input pixel index == output pixel index
            a_off4[q] = ok ? (unsigned)(mm * p.Cin) * 4u : INV;
            a_mlo[q] = ok ? 1u : 0u;
            a_mhi[q] = 0u;
            continue;
        }
        const int ox = mm % p.Wo, t = mm / p.Wo, oy = t % p.Ho, b = t / p.Ho;
        const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad_x;
        // 1x1 filters have no tap mask: a window that starts outside the input (possible for the sub-filters of
        // a strided dgrad, whose output grid can overhang gy) reads zeros through an invalid row offset
        const bool inside = !is1x1 || (iy0 >= 0 && ix0 >= 0 && iy0 < p.H && ix0 < p.W);
        a_off4[q] = (ok && inside) ? (unsigned)(((b * p.H + iy0) * p.W + ix0) * p.Cin) * 4u : INV;
        unsigned long long mask = 0;
        if (ok && is1x1 && inside) mask = 1;
        if (ok && !is1x1) {
            // taps (ky,kx) inside the image form a rectangle: kx in [kx_lo,kx_hi) for ky in [ky_lo,ky_hi)
            const int kx_lo = max(0, -ix0), kx_hi = min(p.KW, p.W - ix0);
            const int ky_lo = max(0, -iy0), ky_hi = min(p.KH, p.H - iy0);
            if (kx_hi > kx_lo) {
                const unsigned long long rowbits = ((1ull << kx_hi) - 1ull) & ~((1ull << kx_lo) - 1ull);
                for (int ky = ky_lo; ky < ky_hi; ++ky) mask |= rowbits << (ky * p.KW);
            }
        }
        a_mlo[q] = (unsigned)mask;
        a_mhi[q] = (unsigned)(mask >> 32);
    }
    unsigned b_off4[B_LD];
#pragma unroll
    for (int q = 0; q < B_LD; ++q) {
        const int row = (tid >> 3) + q * (THREADS / 8);
        const int n = n0 + row;
        b_off4[q] = (row < BN && n < p.N) ? (unsigned)(n * p.K) * 4u : INV;
    }
    if (!is1x1) __syncthreads();      // ktab visible

    // one stage of global loads into a register set.  Masking is pure integer arithmetic (OR-ing INV
    // into the offset): with `cond ? offset : OOB` the compiler threads the condition into divergent
    // branches that each hold a copy of the load writing the same registers, and guards the second copy
    // with s_waitcnt vmcnt(0) -- which drains every stage still in flight.
    // Fast path (whole stages of the 4-wave kernel): the k-dependent part of every address is UNIFORM across
    // the workgroup -- k0*4 for 1x1 filters and for the weights, the tap's byte offset for KxK filters whose
    // Cin is a multiple of 32 (a stage is then 32 channels of ONE tap) -- so it rides in the scalar offset
    // operand of the buffer load and the per-lane offsets are loop invariants: no address VALU in the K loop
    // (it was ~45 of the ~64 vector instructions per stage, and vector instructions of co-resident waves
    // delay MFMA issue).  The buffer base is moved back by the largest negative halo offset so that the
    // per-lane part is never negative (the hardware range-checks it before adding the scalar part).
    const bool tap_uni = !is1x1 && (p.Cin % BKS) == 0 && p.KH * p.KW <= 32;
    const unsigned halo = (unsigned)max(0, (p.pad * p.W + p.pad_x) * p.Cin) * 4u;
    const __amdgpu_buffer_rsrc_t xrb =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.x - halo), 0, p.x_bytes + halo, 0x00020000);
    unsigned a_vk[A_LD], b_vk[B_LD];
#pragma unroll
    for (int q = 0; q < A_LD; ++q) a_vk[q] = a_off4[q] == INV ? INV : a_off4[q] + halo + (unsigned)kg * 4u;
#pragma unroll
    for (int q = 0; q < B_LD; ++q) b_vk[q] = b_off4[q] == INV ? INV : b_off4[q] + (unsigned)kg * 4u;
    auto stage_load = [&](float4 (&A)[A_LD], float4 (&Bq)[B_LD], int k0) {
            if (k0 + BKS <= kend && (is1x1 || tap_uni)) {
                unsigned so_a = (unsigned)k0 * 4u, kp = 0;
                if (!is1x1) {
                    const unsigned e = __builtin_amdgcn_readfirstlane(ktab[k0 >> 2]);
                    so_a = e >> 6;
                    kp = e & 31u;
                }
#pragma unroll
                for (int q = 0; q < A_LD; ++q) {
                    const unsigned tinv = (((a_mlo[q] >> kp) & 1u) - 1u) & INV;     // 1x1: bit 0 is set for valid rows
                    A[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xrb, a_vk[q] | tinv, so_a, 0));
                }
#pragma unroll
                for (int q = 0; q < B_LD; ++q)
                    Bq[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, b_vk[q], (unsigned)k0 * 4u, 0));
                return;
            }
        
        const int k = k0 + kg;
        const unsigned kinv = ~(unsigned)((k - kend) >> 31) & INV;      // INV when k >= kend
        const unsigned k4 = (unsigned)k * 4u;
        // 1x1 filters have no tap table: their "entry" is (k*4) << 6 | tap 0.  One load sequence serves
        // both cases (selected by mask arithmetic, not a branch: two copies of the loads under a branch
        // write the same registers and cost a vmcnt(0) each)
        const unsigned e = ktab[(unsigned)min(k >> 2, p.ktab_entries - 1) & ~m1x1];
        const unsigned ee = (e & ~m1x1) | ((k4 << 6) & m1x1);
        const unsigned d4 = ee >> 6, kp = ee & 63u;
#pragma unroll
        for (int q = 0; q < A_LD; ++q) {
            const unsigned long long m64 = ((unsigned long long)a_mhi[q] << 32) | a_mlo[q];
            const unsigned tinv = (((unsigned)(m64 >> kp) & 1u) - 1u) & INV;  // INV when the tap is padding
            A[q] = __builtin_bit_cast(float4,
                                      __builtin_amdgcn_raw_buffer_load_b128(xr, (a_off4[q] + d4) | tinv | kinv, 0, 0));
        }
#pragma unroll
        for (int q = 0; q < B_LD; ++q)
            Bq[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, (b_off4[q] + k4) | kinv, 0, 0));
    };
    // register prefetch: the loads of stage k+1 are in flight while stage k computes.  (A second
    // register set, two stages in flight, measured slower in the 4-wave kernel: the extra VGPRs cost more
    // occupancy than the deeper prefetch hides.)
    float4 ra[A_LD], rb[B_LD];
    auto gload = [&](int k0) { stage_load(ra, rb, k0); };
    auto sstore = [&](int S) {
#pragma unroll
        for (int q = 0; q < A_LD; ++q) {
            const int row = (tid >> 3) + q * (THREADS / 8);
            if (row < BM) *(float4*)&As[S][row * BKS + ((kc ^ ((row >> 1) & 7)) << 2)] = ra[q];
        }
#pragma unroll
        for (int q = 0; q < B_LD; ++q) {
            const int row = (tid >> 3) + q * (THREADS / 8);
            if (row < BN) *(float4*)&Bs[S][row * BKS + ((kc ^ ((row >> 1) & 7)) << 2)] = rb[q];
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fg = lane >> 4;
    // fragment reads of one 16-deep half (h = 0/1) of a stage, and the 4*TM*TN MFMAs that consume them
    auto rd = [&](float4 (&av)[TM], float4 (&bv)[TN], int buf, int h) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = (wm * TM + i) * 16 + fr;
                av[i] = *(const float4*)&As[buf][row * BKS + (((h * 4 + fg) ^ ((row >> 1) & 7)) << 2)];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = (wn * TN + j) * 16 + fr;
                bv[j] = *(const float4*)&Bs[buf][row * BKS + (((h * 4 + fg) ^ ((row >> 1) & 7)) << 2)];
            }
        
    };
    auto mm = [&](const float4 (&av)[TM], const float4 (&bv)[TN]) {
        // k component outermost: consecutive MFMAs hit DIFFERENT accumulators (the 16x16x4 f32
        // MFMA issues every 32 cycles but a dependent one waits 40)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const float a = t == 0 ? av[i].x : t == 1 ? av[i].y : t == 2 ? av[i].z : av[i].w;
                    const float b = t == 0 ? bv[j].x : t == 1 ? bv[j].y : t == 2 ? bv[j].z : bv[j].w;
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i][j], 0, 0, 0);
                }
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 av[TM], bv[TN];
            rd(av, bv, buf, h);
            mm(av, bv);
        }
    };
    // residual tile: issued before the K loop so that its latency hides behind the MFMAs (small
    // tiles only: C_LD float4 registers per thread)
    constexpr int C_LD = (BM * (BN / 4) + NT - 1) / NT;
    constexpr bool PREFETCH_RES = C_LD <= 8;
    const bool vec_epi = p.splitk <= 1 && (p.N & 3) == 0;
    float4 rres[PREFETCH_RES ? C_LD : 1];
    if (PREFETCH_RES && vec_epi && (p.flags & I2V_EPI_RESIDUAL) && p.ostride == 1) {
#pragma unroll
        for (int it = 0; it < C_LD; ++it) {
            const int e = gtid + it * NT;
            const int row = e / (BN / 4), col = (e % (BN / 4)) * 4;
            const int m = m0 + row, n = n0 + col;
            // non-temporal: in a bottleneck this is the last use of the block input
            rres[it] = (e < BM * (BN / 4) && m < p.M && n < p.N)
                           ? __builtin_bit_cast(float4, __builtin_nontemporal_load((const f32x4*)(p.res + (long long)m * p.N + n)))
                           : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    unsigned long long t1c = 0;
    if (p.clk) t1c = __builtin_amdgcn_s_memtime();
    gload(kbeg);
    sstore(0);
    // one fragment register set: 118 VGPRs -> four waves per SIMD (a software-pipelined two-set form needed 138 -> three, and
    // measured no faster with four co-resident waves: DESIGN_HISTORY.md)
    __syncthreads();
    int buf = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BKS) {
        const bool more = k0 + BKS < kend;
        if (more) gload(k0 + BKS);
        compute(buf);
        if (more) sstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    if (p.clk && gtid == 0) {     // diagnostic build path: stamps go to their own buffer, never to an output
        const unsigned long long t2c = __builtin_amdgcn_s_memtime();
        unsigned long long* o = p.clk + 8 * (blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = t2c - t1c;                                  // K loop (incl. its prologue stage)
        o[1] = __builtin_amdgcn_s_memrealtime() - t0r;     // 100 MHz ticks, whole kernel so far
        o[2] = t1c - t0c;                                  // setup: tap table, row masks, residual prefetch
        o[3] = t2c - t0c;
    }
    // epilogue.  C/D map of the 16x16 MFMA: col = lane&15, row = 4*(lane>>4) + r.  The tile goes
    // through LDS so that global stores (and the residual loads) are whole 16-B-per-lane rows
    // instead of 64-B fragments of a line.  (Every wave's last fragment reads completed before the
    // barrier of the last loop iteration, so the stage buffers are free.)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                smem[((wm * TM + i) * 16 + 4 * fg + r) * CROW + (wn * TN + j) * 16 + fr] = acc[i][j][r];

    __syncthreads();
    const bool split = p.splitk > 1;
    auto out_index = [&](int m) -> long long {
        if (p.ostride == 1) return (long long)m * p.N;
        const int ox = m % p.Wo, t = m / p.Wo, oy = t % p.Ho, b = t / p.Ho;
        return (((long long)b * p.Hy + oy * p.ostride) * p.Wy + ox * p.ostride) * p.N;
    };
    if (split && p.ws) {
        // Split-K finish inside the kernel: every split stores its partial tile (plain 16-B stores, tile-
        // contiguous), the last one to arrive at the tile's counter adds the partials in split order and
        // runs the fused epilogue.  No clear of y, no atomics on y (fp32 atomics move ~1.3 TB/s chip-wide),
        // no separate epilogue pass, and the sum no longer depends on arrival order.
        //
        // The 8 XCDs have private, mutually non-coherent L2s: a release/acquire fence pair at agent scope
        // writes back and invalidates a whole L2 per fence (measured: the layer3 3x3 went 65 -> 153 us with
        // __threadfence()).  Instead the partials are stored and re-read at agent scope (sc1, the cache policy of
        // a relaxed agent-scope atomic: coherent across the XCDs without fences) -- so only these 20-64 KB tiles pay
        // for coherence; s_waitcnt vmcnt(0) orders the stores before the (device-scope) arrival count.
        constexpr int SC01 = 16;          // buffer aux bit 4 = sc1: agent scope (sc0 sc1 = system scope is not needed)
        const size_t split_stride = (size_t)gridDim.x * (BM * BN);      // floats between splits of a tile
        const __amdgpu_buffer_rsrc_t wsr = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.ws + (size_t)tile * (BM * BN)), 0, 0x7FFFFFF0, 0x00020000);
        const unsigned mine = (unsigned)(blockIdx.y * split_stride * sizeof(float));
        for (int e = gtid; e < BM * (BN / 4); e += NT) {
            const int row = e / (BN / 4), col = (e % (BN / 4)) * 4;
            const float4 v = *(const float4*)&smem[row * CROW + col];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), wsr,
                                                   mine + (unsigned)(row * BN + col) * 4u, 0, SC01);
        }
        __builtin_amdgcn_s_waitcnt(0);    // vmcnt(0): my stores have been acknowledged by memory
        __syncthreads();
        __shared__ int last_flag;
        int* flag = &last_flag;
        if (gtid == 0) {
            const int arrived = __hip_atomic_fetch_add(p.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = arrived == (int)gridDim.y - 1;
            if (last) __hip_atomic_store(p.cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
            *flag = last;
        }
        __syncthreads();
        if (!*flag) {
            if (p.clk && gtid == 0)
                p.clk[8 * (blockIdx.y * gridDim.x + blockIdx.x) + 4] = __builtin_amdgcn_s_memtime() - t0c;
            return;
        }
        // The finisher's reads come from beyond the L2 (~2 us a round trip): every partial of up to FIN_CH
        // elements per thread, and their residuals, are put in flight before the first sum.  Its own
        // partial is still in LDS.  Summation is in split order whichever workgroup arrives last.
        const int nsplit = gridDim.y, my = blockIdx.y;
        constexpr int FIN_CH = C_LD < 6 ? C_LD : 6;
        const bool vec = (p.N & 3) == 0;
        for (int it0 = 0; it0 < C_LD; it0 += FIN_CH) {
            float4 u[FIN_CH][kSplitInKernelMax], rr[FIN_CH], acc4[FIN_CH] = {};
            // rounds of kSplitInKernelMax splits, summed in split order: ((((p0 + p1) + p2) + p3) + p4) + ... -- one round for
            // the backbone's splits (<= 4), more for the long skinny GEMMs of the relation head (round 5: they took the
            // atomic finish before, whose sum depends on arrival order)
            for (int s0 = 0; s0 < nsplit; s0 += kSplitInKernelMax) {
#pragma unroll
                for (int c = 0; c < FIN_CH; ++c) {
                    const int e = gtid + (it0 + c) * NT;
                    const int row = e / (BN / 4), col = (e % (BN / 4)) * 4;
                    const int m = m0 + row, n = n0 + col;
                    const bool ok = e < BM * (BN / 4) && m < p.M && n < p.N;
                    const unsigned off = (unsigned)(row * BN + col) * 4u;
#pragma unroll
                    for (int sp = 0; sp < kSplitInKernelMax; ++sp)
                        u[c][sp] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                            wsr, (ok && s0 + sp < nsplit && s0 + sp != my) ? off + (unsigned)((s0 + sp) * split_stride * sizeof(float)) : 0xFFFFFFF0u,
                            0, SC01));
                    if (s0 == 0) {
                        rr[c] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (ok && vec && (p.flags & I2V_EPI_RESIDUAL)) rr[c] = __builtin_bit_cast(float4, __builtin_nontemporal_load((const f32x4*)(p.res + (long long)m * p.N + n)));
                    }
                }
#pragma unroll
                for (int c = 0; c < FIN_CH; ++c) {
                    const int e = gtid + (it0 + c) * NT;
                    const int row = e / (BN / 4), col = (e % (BN / 4)) * 4;
                    const float4 mine4 = (e < BM * (BN / 4)) ? *(const float4*)&smem[row * CROW + col] : make_float4(0.f, 0.f, 0.f, 0.f);
                    float4 v = acc4[c];
#pragma unroll
                    for (int sp = 0; sp < kSplitInKernelMax; ++sp) {   // slots >= nsplit were read out of range: zeros
                        const float4 t = s0 + sp == my ? mine4 : u[c][sp];
                        if (s0 == 0 && sp == 0) v = t;
                        else { v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
                    }
                    acc4[c] = v;
                }
            }
#pragma unroll
            for (int c = 0; c < FIN_CH; ++c) {
                const int e = gtid + (it0 + c) * NT;
                const int row = e / (BN / 4), col = (e % (BN / 4)) * 4;
                const int m = m0 + row, n = n0 + col;
                if (e >= BM * (BN / 4) || m >= p.M || n >= p.N) continue;
                const float4 v = acc4[c];
                const long long o = (long long)m * p.N + n;      // split-K only runs with ostride == 1
                float vv[4] = {v.x, v.y, v.z, v.w};
                if (vec) {
                    if (p.flags & I2V_EPI_SCALE) {
                        const float4 sc = *(const float4*)(p.scale + n);
                        vv[0] *= sc.x; vv[1] *= sc.y; vv[2] *= sc.z; vv[3] *= sc.w;
                    }
                    if ((p.flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && p.shift) {
                        const float4 sh = *(const float4*)(p.shift + n);
                        vv[0] += sh.x; vv[1] += sh.y; vv[2] += sh.z; vv[3] += sh.w;
                    }
                    if (p.flags & I2V_EPI_RESIDUAL) {
                        vv[0] += rr[c].x; vv[1] += rr[c].y; vv[2] += rr[c].z; vv[3] += rr[c].w;
                    }
                    if (p.flags & I2V_EPI_RELU) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) vv[q] = fmaxf(vv[q], 0.f);
                    }
                    if (p.flags & I2V_EPI_MASK) {
                        const float4 mk = *(const float4*)(p.mask + o);
                        vv[0] = mk.x > 0.f ? vv[0] : 0.f; vv[1] = mk.y > 0.f ? vv[1] : 0.f;
                        vv[2] = mk.z > 0.f ? vv[2] : 0.f; vv[3] = mk.w > 0.f ? vv[3] : 0.f;
                    }
                    *(float4*)(p.y + o) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (n + q >= p.N) break;
                        float t = vv[q];
                        if (p.flags & I2V_EPI_SCALE) t *= p.scale[n + q];
                        if ((p.flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && p.shift) t += p.shift[n + q];
                        if (p.flags & I2V_EPI_RESIDUAL) t += p.res[o + q];
                        if (p.flags & I2V_EPI_RELU) t = fmaxf(t, 0.f);
                        if ((p.flags & I2V_EPI_MASK) && !(p.mask[o + q] > 0.f)) t = 0.f;
                        p.y[o + q] = t;
                    }
                }
            }
        }
    } else if (split) {               // fallback: fp32 atomics into a zeroed y (64 lanes = 256 contiguous bytes)
        for (int e = gtid; e < BM * BN; e += NT) {
            const int row = e / BN, col = e % BN;
            const int m = m0 + row, n = n0 + col;
            if (m < p.M && n < p.N) atomicAdd(p.y + out_index(m) + n, smem[row * CROW + col]);
        }
    } else if ((p.N & 3) == 0) {
#pragma unroll
        for (int it = 0; it < C_LD; ++it) {
            const int e = gtid + it * NT;
            if (e >= BM * (BN / 4)) break;
            const int row = e / (BN / 4), col = (e % (BN / 4)) * 4;
            const int m = m0 + row, n = n0 + col;
            if (m >= p.M || n >= p.N) continue;           // N % 4 == 0: a float4 never straddles N
            float4 v = *(const float4*)&smem[row * CROW + col];
            if (p.flags & I2V_EPI_SCALE) {
                const float4 sc = *(const float4*)(p.scale + n);
                v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
            }
            if ((p.flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && p.shift) {
                const float4 sh = *(const float4*)(p.shift + n);
                v.x += sh.x; v.y += sh.y; v.z += sh.z; v.w += sh.w;
            }
            const long long o = out_index(m) + n;
            if (p.flags & I2V_EPI_RESIDUAL) {
                const float4 rr = (PREFETCH_RES && p.ostride == 1) ? rres[PREFETCH_RES ? it : 0]
                                                                   : *(const float4*)(p.res + o);
                v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
            }
            if (p.flags & I2V_EPI_RELU) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
            if (p.flags & I2V_EPI_MASK) {
                const float4 mk = *(const float4*)(p.mask + o);
                v.x = mk.x > 0.f ? v.x : 0.f; v.y = mk.y > 0.f ? v.y : 0.f; v.z = mk.z > 0.f ? v.z : 0.f; v.w = mk.w > 0.f ? v.w : 0.f;
            }
            *(float4*)(p.y + o) = v;
        }
    } else {
        for (int e = gtid; e < BM * BN; e += NT) {
            const int row = e / BN, col = e % BN;
            const int m = m0 + row, n = n0 + col;
            if (m >= p.M || n >= p.N) continue;
            float v = smem[row * CROW + col];
            if (p.flags & I2V_EPI_SCALE) v *= p.scale[n];
            if ((p.flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && p.shift) v += p.shift[n];
            const long long o = out_index(m) + n;
            if (p.flags & I2V_EPI_RESIDUAL) v += p.res[o];
            if (p.flags & I2V_EPI_RELU) v = fmaxf(v, 0.f);
            if ((p.flags & I2V_EPI_MASK) && !(p.mask[o] > 0.f)) v = 0.f;
            p.y[o] = v;
        }
    }
    if (p.clk && gtid == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        unsigned long long* o = p.clk + 8 * (blockIdx.y * gridDim.x + blockIdx.x);
        o[4] = __builtin_amdgcn_s_memtime() - t0c;           // whole kernel, this workgroup
        o[5] = 1;                                            // this workgroup ran the epilogue (split-K: the last arrival)
    }
}

// ---------------------------------------------------------------- pointwise / plain-GEMM specialisation
// y[m][n] = epi(sum_k A[m][k] * Wt[n][k]) where row m of A IS row m of x (1x1 filter, stride 1, same grid; linear layers;
// the element-wise planes of a Winograd convolution).  The layer3 bottleneck GEMMs are short (K = 256: 8 stages of MFMA
// work, ~12k cycles), so what a workgroup does OUTSIDE the K loop decides: this kernel has no tap table, no row masks, no
// integer division per row, prefetches the epilogue's operands (residual tile, BN scale / shift) before the K loop, and
// its epilogue never touches LDS: the MFMA operands are swapped (weights as the row operand), so a lane's four
// accumulator registers are four CONSECUTIVE output channels of one pixel -- scale/shift/residual/ReLU in registers, one
// 16-B store per fragment, no LDS round trip, no barrier.  Staging, swizzled LDS image and the K loop are conv_igemm_f32's.
// Split-K (<= kSplitInKernelMax): partial tiles go to the caller's workspace in REGISTER order (fragment, wave, lane), the
// last workgroup to arrive sums them in split order -- same protocol as conv_igemm_f32, whole-wave 1-KB rows.
// KG > 1 (round 4): INTRA-WORKGROUP K split.  A GEMM too short in M x N to fill the chip (layer3 conv1 of a frame pair: 240
// tiles of 80x64 for 1024 slots, K = 1024) used to run as 3 K-splits of 4 waves whose partial tiles crossed the fabric
// (sc1 write-through + re-read by the last arriver: 14.7 + 9.8 MB per launch beside the layer's own 25.6 MB).  Here ONE
// workgroup of KG x 4 waves owns the tile: wave group g stages and multiplies k in [g K/KG, (g+1) K/KG) in an LDS region of
// its own, the groups' partial tiles meet in LDS (register order, conflict-free 16-byte rows) and group 0 adds them IN GROUP
// ORDER ((p0 + p1) + p2) + p3 -- deterministic -- and runs the one fused epilogue.  Same waves per SIMD as four co-resident
// split workgroups, no partial ever leaves the CU, no arrival counter.  K must be a multiple of KG x 32 (the host checks).
// STG (round 6): how a stage reaches LDS.  0: global -> VGPR -> ds_write_b128 (rounds 2-5).  1 / 2: LDS-DMA
// (buffer_load_dwordx4 ... lds): no staging registers, no ds_write, no LDS store-path cycles; the DMA lands lane-linear
// (wave-uniform base + lane x 16 bytes), so the image's column swizzle rides on the SOURCE address -- each 128-byte (64-byte)
// row piece is still one contiguous run of the operand row, its 16-byte columns permuted among the lanes that fetch it.
// Two buffers, one raw s_barrier per stage: [vmcnt(0): my pieces of stage i have landed | barrier: everyone's have, and everyone
// is done with the other buffer | request stage i + 1 into it | multiply stage i].  1: 32-k stages in the rounds-2-5 image
// (128-byte rows, column ^ (row >> 1) & 7).  2: 16-k stages, 64-byte rows, column ^ (-(row >> 2)) & 3 (the four 16-lane groups of
// a ds_read_b128 still touch 16 distinct 16-byte slots): half the LDS per workgroup, twice the barriers.  Same fragment
// ownership, same k order per accumulator: bit-equal to STG 0 (tools/micro/gemm_lab.hip measured the forms side by side).
// The requests are lds_dma16 (conv_common.h).

template <int WAVES_M, int WAVES_N, int TM, int TN, bool CLK = false, bool MASK = false, int KG = 1, int STG = 0>
__global__ void __launch_bounds__(THREADS * KG)
conv_gemm_f32(const ConvP p_in) {
    ConvP p = p_in;
    // CLK: diagnostic instantiation (i2v_conv_debug_clock): per workgroup {start, end in 100 MHz ticks, prologue / K-loop /
    // epilogue shader cycles, HW_ID, XCC_ID} into a buffer of their own; the product instantiation has no stamp
    unsigned long long c_rt0 = 0, c_t0 = 0, c_t1 = 0, c_t2 = 0;
    if constexpr (CLK) { c_rt0 = __builtin_amdgcn_s_memrealtime(); c_t0 = __builtin_amdgcn_s_memtime(); }
    if (p.nbatch > 1) {
        p.x += (long long)blockIdx.z * p.bsx;
        p.w += (long long)blockIdx.z * p.bsw;
        p.y += (long long)blockIdx.z * p.bsy;
    }
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16;
    constexpr int A_LD = (BM * 8 + THREADS - 1) / THREADS, B_LD = (BN * 8 + THREADS - 1) / THREADS;
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
    static_assert(KG == 1 || !CLK, "the K-group form has no diagnostic instantiation");
    static_assert(STG == 0 || (KG == 1 && !CLK), "the LDS-DMA form is the plain 4-wave kernel");
    constexpr int BKL = STG == 2 ? 16 : BKS;                   // k per LDS stage
    // KG > 1: the four waves of a K group synchronise among THEMSELVES between stages (an arrival counter in LDS: release,
    // add, poll, acquire) -- an s_barrier would march all 16 waves in lock step, every SIMD's four waves staging together and
    // multiplying together; free-running groups drift apart like co-resident workgroups do, one group's staging under another's
    // MFMAs.  The counters only grow (4 per barrier), so a fast wave's next arrival cannot release a slow wave early.
    __shared__ int kcnt[KG > 1 ? KG : 1];
    int kphase = 0;
    auto stage_barrier = [&]() {
        if constexpr (KG == 1) {
            __syncthreads();
        } else {
            kphase += 4;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");          // my LDS stores have landed
            if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&kcnt[threadIdx.x >> 8], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            while (__hip_atomic_load(&kcnt[threadIdx.x >> 8], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < kphase)
                __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    };
    if constexpr (KG > 1) {
        if (threadIdx.x < KG) kcnt[threadIdx.x] = 0;
    }
    constexpr int GROUP_FLOATS = 2 * (BM + BN) * BKL;          // one K group's two stage buffers
    extern __shared__ __attribute__((aligned(16))) float smem_all[];
    const int gid = KG > 1 ? (int)(threadIdx.x >> 8) : 0;      // K group of this wave (4 waves per group)
    float* smem = smem_all + gid * GROUP_FLOATS;
    float (*As)[BM * BKL] = reinterpret_cast<float (*)[BM * BKL]>(smem);
    float (*Bs)[BN * BKL] = reinterpret_cast<float (*)[BN * BKL]>(smem + 2 * BM * BKL);

    const int tid = KG > 1 ? (int)(threadIdx.x & (THREADS - 1)) : (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int fr = lane & 15, fg = lane >> 4;
    const int tiles_n = (p.N + BN - 1) / BN;
    int tile;
    {       // XCD-aware tile order (conv_igemm_f32)
        const int nt = gridDim.x, q = nt >> 3, r = nt & 7, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    const int kbeg = KG > 1 ? gid * (p.K / KG) : blockIdx.y * p.k_per_split;
    const int kend = KG > 1 ? kbeg + p.K / KG : min(p.K, kbeg + p.k_per_split);
    const int kc = tid & 7, kg = kc * 4;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    constexpr unsigned INV = 0x80000000u;
    const unsigned g0_inv = gid == 0 ? 0u : INV;               // only K group 0 runs the epilogue: the others fetch no operand of it
    unsigned a_vk[A_LD], b_vk[B_LD];
#pragma unroll
    for (int q = 0; q < A_LD; ++q) {
        const int row = (tid >> 3) + q * (THREADS / 8);
        const int m = m0 + row;
        a_vk[q] = (row < BM && m < p.M) ? ((unsigned)(m * p.K) + (unsigned)kg) * 4u : INV;
    }
#pragma unroll
    for (int q = 0; q < B_LD; ++q) {
        const int row = (tid >> 3) + q * (THREADS / 8);
        const int n = n0 + row;
        b_vk[q] = (row < BN && n < p.N) ? ((unsigned)(n * p.K) + (unsigned)kg) * 4u : INV;
    }
    float4 ra[A_LD], rb[B_LD];
    // the k offset of a stage is uniform: it rides in the scalar offset of the buffer load; a lane beyond kend (the last,
    // partial stage of a K that is not a multiple of 32) gets the 2 GiB bit OR-ed in and reads zeros
    auto gload = [&](int k0) {
        const unsigned so = (unsigned)k0 * 4u;
        const unsigned kinv = ~(unsigned)((k0 + kg - kend) >> 31) & INV;
#pragma unroll
        for (int q = 0; q < A_LD; ++q)
            ra[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, a_vk[q] | kinv, so, 0));
#pragma unroll
        for (int q = 0; q < B_LD; ++q)
            rb[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, b_vk[q] | kinv, so, 0));
    };
    auto sstore = [&](int S) {
#pragma unroll
        for (int q = 0; q < A_LD; ++q) {
            const int row = (tid >> 3) + q * (THREADS / 8);
            if (row < BM) *(float4*)&As[S][row * BKS + ((kc ^ ((row >> 1) & 7)) << 2)] = ra[q];
        }
#pragma unroll
        for (int q = 0; q < B_LD; ++q) {
            const int row = (tid >> 3) + q * (THREADS / 8);
            if (row < BN) *(float4*)&Bs[S][row * BKS + ((kc ^ ((row >> 1) & 7)) << 2)] = rb[q];
        }
    };
    // ---- LDS-DMA staging (STG > 0).  A stage = NP 1-KB pieces (PR rows of the A tile, then of the B tile); wave w requests
    // pieces w, w + 4, ...  A lane's logical 16-byte column is the same for all pieces of its wave: the swizzle term of a row
    // repeats with the piece stride (8 rows x an even piece count for the 128-byte rows; 16 rows for the 64-byte rows).
    constexpr int PR = 256 / BKL, CPR = BKL / 4;
    constexpr int NPA = BM / PR, NPB = BN / PR, NP = NPA + NPB, PMAX = (NP + 3) / 4, REM = NP % 4;
    static_assert(STG == 0 || (BM % PR == 0 && BN % PR == 0 && (BKL == 16 || NPA % 2 == 0)), "whole pieces, one swizzle term per wave");
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lchunk = BKL == 32 ? ((lane & 7) ^ ((wave_s * 4 + (lane >> 4)) & 7)) : ((lane & 3) ^ ((-(lane >> 4)) & 3));
    unsigned d_vk[STG > 0 ? PMAX : 1];
    __amdgpu_buffer_rsrc_t d_rs[STG > 0 ? PMAX : 1];
    if constexpr (STG > 0) {
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            const int pc = q * 4 + wave_s;
            const bool isA = pc < NPA;                                      // wave-uniform
            const int row = (isA ? pc : pc - NPA) * PR + lane / CPR;
            const int g = (isA ? m0 : n0) + row;
            d_vk[q] = (pc < NP && g < (isA ? p.M : p.N)) ? ((unsigned)(g * p.K) + (unsigned)(lchunk * 4)) * 4u : INV;
            d_rs[q] = isA ? xr : wr;
        }
    }
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;
    auto dma_issue = [&](int k0, int S) {
        const unsigned so = (unsigned)k0 * 4u;
        const unsigned kinv = ~(unsigned)((k0 + lchunk * 4 - kend) >> 31) & INV;      // a partial last stage: lanes beyond kend read zeros
        const unsigned a_dst = lds_base + (unsigned)(S * BM * BKL * 4), b_dst = lds_base + (unsigned)((2 * BM + S * BN) * BKL * 4);
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            const int pc = q * 4 + wave_s;
            if (REM == 0 || q < PMAX - 1 || wave_s < REM)
                lds_dma16(pc < NPA ? a_dst + (unsigned)(pc * 1024) : b_dst + (unsigned)((pc - NPA) * 1024), d_vk[q] | kinv, d_rs[q], so);
        }
    };
    auto dma_wait_barrier = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my pieces of the stage have landed ...
        __builtin_amdgcn_s_barrier();                          // ... everyone's have; and everyone is done with the other buffer
    };
    if constexpr (STG > 0) dma_issue(kbeg, 0);
    else gload(kbeg);                     // first: everything below hides behind this round trip

    // Operands of the epilogue.  A lane owns channels n .. n+3 of pixel m for every fragment (i, j):
    //   m = m0 + (wm*TM + i)*16 + (lane & 15),   n = n0 + (wn*TN + j)*16 + 4*(lane >> 4)
    // They are fetched by buffer loads that are ALWAYS issued (an absent operand or an out-of-range lane gets the 2 GiB
    // offset and reads zeros without traffic): a load under a condition makes the number of loads in flight unknowable
    // to the compiler, which then drains everything (s_waitcnt vmcnt(0)) in front of the first LDS store -- with the
    // 19.6 MB residual of a layer3 conv3 in flight that cost 4.5k of 8.1k prologue cycles (tools/gemm_phase.py).
    // The residual tile is requested one stage before the last, behind that stage's operand loads (returns are in
    // order): its latency lies under the last stage's MFMAs, and no operand load ever waits for it.
    const bool split = p.splitk > 1;
    constexpr bool PREFETCH_RES = TM * TN <= 8;
    const unsigned n_bytes = (unsigned)p.N * 4u;
    const __amdgpu_buffer_rsrc_t scr = __builtin_amdgcn_make_buffer_rsrc((void*)(p.scale ? p.scale : p.shift ? p.shift : (const float*)p.x), 0, n_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t shr = __builtin_amdgcn_make_buffer_rsrc((void*)(p.shift ? p.shift : (const float*)p.x), 0, n_bytes, 0x00020000);
    const unsigned long long y_bytes = (unsigned long long)p.M * p.N * 4ull;
    const __amdgpu_buffer_rsrc_t resr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.res ? p.res : (const float*)p.x), 0, (unsigned)(y_bytes < 0x7FFFFFF0ull ? y_bytes : 0x7FFFFFF0ull), 0x00020000);
    const unsigned sc_inv = ((p.flags & I2V_EPI_SCALE) ? 0u : INV) | g0_inv;
    const unsigned sh_inv = (((p.flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && p.shift) ? 0u : INV) | g0_inv;     // scale without shift: the data-gradient epilogue
    const unsigned res_inv = (((p.flags & I2V_EPI_RESIDUAL) && !split) ? 0u : INV) | g0_inv;
    const __amdgpu_buffer_rsrc_t mskr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.mask ? p.mask : (const float*)p.x), 0, (unsigned)(y_bytes < 0x7FFFFFF0ull ? y_bytes : 0x7FFFFFF0ull), 0x00020000);
    float4 sc[TN], sh[TN], rres[PREFETCH_RES ? TM : 1][PREFETCH_RES ? TN : 1];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * 16 + 4 * fg;
        const unsigned off = n < p.N ? (unsigned)n * 4u : INV;
        sc[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(scr, off | sc_inv, 0, 0));
        sh[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(shr, off | sh_inv, 0, 0));
    }
    auto issue_res = [&]() {
        if constexpr (PREFETCH_RES) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int m = m0 + (wm * TM + i) * 16 + fr, n = n0 + (wn * TN + j) * 16 + 4 * fg;
                    const unsigned off = (m < p.M && n < p.N) ? (unsigned)(m * p.N + n) * 4u : INV;
                    rres[i][j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(resr, off | res_inv, 0, 2));   // nt: last use of the block input
                }
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int buf) {
        auto swzl = [](int row) { return BKL == 32 ? ((row >> 1) & 7) : ((-(row >> 2)) & 3); };
#pragma unroll
        for (int h = 0; h < BKL / 16; ++h) {
            float4 av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = (wm * TM + i) * 16 + fr;
                av[i] = *(const float4*)&As[buf][row * BKL + (((h * 4 + fg) ^ swzl(row)) << 2)];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = (wn * TN + j) * 16 + fr;
                bv[j] = *(const float4*)&Bs[buf][row * BKL + (((h * 4 + fg) ^ swzl(row)) << 2)];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const float a = t == 0 ? av[i].x : t == 1 ? av[i].y : t == 2 ? av[i].z : av[i].w;
                        const float b = t == 0 ? bv[j].x : t == 1 ? bv[j].y : t == 2 ? bv[j].z : bv[j].w;
                        // weights are the ROW operand: D[row = channel][col = pixel], a lane holds 4 consecutive channels
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b, a, acc[i][j], 0, 0, 0);
                    }
        }
    };
    int buf = 0, k0 = kbeg;
    if constexpr (STG > 0) {
        for (; k0 + 2 * BKL < kend; k0 += BKL) {      // every stage but the last two
            dma_wait_barrier();
            dma_issue(k0 + BKL, buf ^ 1);
            compute(buf);
            buf ^= 1;
        }
        if (k0 + BKL < kend) {                        // two stages left: the last one's operands, then the residual tile
            dma_wait_barrier();
            dma_issue(k0 + BKL, buf ^ 1);
            issue_res();
            compute(buf);
            buf ^= 1;
        } else {
            issue_res();
        }
        dma_wait_barrier();
        compute(buf);
    } else {
    if constexpr (KG > 1) __syncthreads();           // the arrival counters are zero (the first stage's loads are in flight)
    sstore(0);
    stage_barrier();
    if constexpr (CLK) c_t1 = __builtin_amdgcn_s_memtime();
    for (; k0 + 2 * BKS < kend; k0 += BKS) {          // every stage but the last two
        gload(k0 + BKS);
        // the next stage's loads are REQUESTED here: left alone the scheduler sinks them below 35 of the stage's 40 MFMAs (shorter
        // live ranges), and a wave then waits out the L2 round trip between its last MFMA and its LDS stores.  With four waves
        // per SIMD the others cover that (the step did not move: 4.45-4.47 against 4.49-4.53 ms, box noise); pinned, a wave
        // covers it alone, which is what the source meant
        __builtin_amdgcn_sched_barrier(0);
        compute(buf);
        sstore(buf ^ 1);
        stage_barrier();
        buf ^= 1;
    }
    if (k0 + BKS < kend) {                            // two stages left: operands of the last one, then the residual tile
        gload(k0 + BKS);
        issue_res();
        __builtin_amdgcn_sched_barrier(0);
        compute(buf);
        sstore(buf ^ 1);
        stage_barrier();
        buf ^= 1;
    } else {
        issue_res();
    }
    compute(buf);                                     // last stage (no barrier: nothing is staged after it)
    }
    if constexpr (CLK) c_t2 = __builtin_amdgcn_s_memtime();
    if constexpr (KG > 1) {
        // the K groups' partial tiles meet in LDS: every group but the first leaves its accumulators in its own (now idle)
        // stage region, in register order -- (fragment, wave, lane) x 16 bytes: whole-wave 1-KB rows both ways -- and group 0
        // adds them in group order
        static_assert(TM * TN * THREADS * 4 <= GROUP_FLOATS, "a partial tile fits a group's stage buffers");
        __syncthreads();                              // every wave has read its last stage
        if (gid > 0) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    *(f32x4*)&smem[(((i * TN + j) * 4 + wave) * 64 + lane) * 4] = acc[i][j];
        }
        __syncthreads();
        if (gid > 0) return;
#pragma unroll
        for (int g = 1; g < KG; ++g)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const f32x4 t = *(const f32x4*)&smem_all[g * GROUP_FLOATS + (((i * TN + j) * 4 + wave) * 64 + lane) * 4];
                    acc[i][j] = (f32x4){acc[i][j][0] + t[0], acc[i][j][1] + t[1], acc[i][j][2] + t[2], acc[i][j][3] + t[3]};
                }
    }
    auto stamp = [&]() {
        if constexpr (CLK) {
            __builtin_amdgcn_s_waitcnt(0);
            if (tid == 0) {
                unsigned long long* o = p.clk + 8 * ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
                o[0] = c_rt0; o[1] = __builtin_amdgcn_s_memrealtime();
                o[2] = c_t1 - c_t0; o[3] = c_t2 - c_t1; o[4] = __builtin_amdgcn_s_memtime() - c_t2;
                o[5] = __builtin_amdgcn_s_getreg(63492); o[6] = __builtin_amdgcn_s_getreg(63508); o[7] = 1;
            }
        }
    };

    auto finish = [&](int i, int j, f32x4 v, float4 rr, float4 mk) {
        const int m = m0 + (wm * TM + i) * 16 + fr, n = n0 + (wn * TN + j) * 16 + 4 * fg;
        if (m >= p.M || n >= p.N) return;
        float4 o = make_float4(v[0], v[1], v[2], v[3]);
        if (p.flags & I2V_EPI_SCALE) { o.x *= sc[j].x; o.y *= sc[j].y; o.z *= sc[j].z; o.w *= sc[j].w; }   // an absent operand was read as zeros
        if ((p.flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && p.shift) { o.x += sh[j].x; o.y += sh[j].y; o.z += sh[j].z; o.w += sh[j].w; }
        if (p.flags & I2V_EPI_RESIDUAL) { o.x += rr.x; o.y += rr.y; o.z += rr.z; o.w += rr.w; }
        if (p.flags & I2V_EPI_RELU) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        if constexpr (MASK) { o.x = mk.x > 0.f ? o.x : 0.f; o.y = mk.y > 0.f ? o.y : 0.f; o.z = mk.z > 0.f ? o.z : 0.f; o.w = mk.w > 0.f ? o.w : 0.f; }
        *(float4*)(p.y + (long long)m * p.N + n) = o;
    };
    auto res_at = [&](int i, int j) -> float4 {
        const int m = m0 + (wm * TM + i) * 16 + fr, n = n0 + (wn * TN + j) * 16 + 4 * fg;
        const unsigned off = (m < p.M && n < p.N && (p.flags & I2V_EPI_RESIDUAL)) ? (unsigned)(m * p.N + n) * 4u : INV;
        return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(resr, off, 0, 2));
    };
    auto mask_at = [&](int i, int j) -> float4 {
        const int m = m0 + (wm * TM + i) * 16 + fr, n = n0 + (wn * TN + j) * 16 + 4 * fg;
        const unsigned off = (m < p.M && n < p.N && (p.flags & I2V_EPI_MASK)) ? (unsigned)(m * p.N + n) * 4u : INV;
        return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(mskr, off, 0, 0));
    };
    if (!split) {
        // the mask tile (data gradients only) is fetched here, all fragments at once, into registers the K loop no longer
        // needs: prefetched beside the residual it would cost the forward layers 4 x TM x TN registers they never use
        float4 mk[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) mk[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MASK) {                   // the MASK instantiation serves data gradients only (launch_tile)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) mk[i][j] = mask_at(i, j);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float4 rr;
                if constexpr (PREFETCH_RES) rr = rres[PREFETCH_RES ? i : 0][PREFETCH_RES ? j : 0];
                else rr = res_at(i, j);
                finish(i, j, acc[i][j], rr, mk[i][j]);
            }
        stamp();
        return;
    }
    // ---- split-K: partials in register order through the caller's workspace (sc1 stores / loads: coherent across the
    // XCDs without fences; conv_igemm_f32 has the protocol's rationale)
    constexpr int SC01 = 16;
    const size_t split_stride = (size_t)gridDim.x * (BM * BN);
    const __amdgpu_buffer_rsrc_t wsr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.ws + (size_t)tile * (BM * BN)), 0, 0x7FFFFFF0, 0x00020000);
    const unsigned mine = (unsigned)(blockIdx.y * split_stride * sizeof(float));
    auto slot = [&](int i, int j) { return (unsigned)((((i * TN + j) * 4 + wave) * 64 + lane) * 16); };
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), wsr, mine + slot(i, j), 0, SC01);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    __shared__ int last_flag;
    if (tid == 0) {
        const int arrived = __hip_atomic_fetch_add(p.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = arrived == (int)gridDim.y - 1;
        if (last) __hip_atomic_store(p.cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = last;
    }
    __syncthreads();
    if (!last_flag) { stamp(); return; }
    const int nsplit = gridDim.y, my = blockIdx.y;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        float4 u[TN][kSplitInKernelMax], rr[TN], mk[TN], v4[TN] = {};
        // rounds of kSplitInKernelMax splits, summed in split order (conv_igemm_f32 has the rationale): one round for the
        // backbone's splits, more for the relation head's skinny GEMMs
        for (int s0 = 0; s0 < nsplit; s0 += kSplitInKernelMax) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int sp = 0; sp < kSplitInKernelMax; ++sp)
                    u[j][sp] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                        wsr, (s0 + sp < nsplit && s0 + sp != my) ? slot(i, j) + (unsigned)((s0 + sp) * split_stride * sizeof(float)) : 0xFFFFFFF0u, 0, SC01));
                if (s0 == 0) {
                    rr[j] = res_at(i, j);
                    if constexpr (MASK) mk[j] = mask_at(i, j);
                    else mk[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float4 m4 = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                float4 v = v4[j];
#pragma unroll
                for (int sp = 0; sp < kSplitInKernelMax; ++sp) {      // slots >= nsplit were read out of range: zeros
                    const float4 t = s0 + sp == my ? m4 : u[j][sp];
                    if (s0 == 0 && sp == 0) v = t;
                    else { v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
                }
                v4[j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) finish(i, j, (f32x4){v4[j].x, v4[j].y, v4[j].z, v4[j].w}, rr[j], mk[j]);
    }
    stamp();
}


// epilogue of the split-K path (partials were accumulated with fp32 atomics)
__global__ void conv_epilogue_kernel(float* __restrict__ y, const float* __restrict__ scale,
                                     const float* __restrict__ shift, const float* __restrict__ res,
                                     const float* __restrict__ mask, long long total4, int N, int flags) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4;
         i += (long long)gridDim.x * blockDim.x) {
        float4 v = ((float4*)y)[i];
        const int n = (int)((i * 4) % N);
        float4 sc = make_float4(1, 1, 1, 1), sh = make_float4(0, 0, 0, 0);
        if (flags & I2V_EPI_SCALE) sc = *(const float4*)(scale + n);
        if ((flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && shift) sh = *(const float4*)(shift + n);
        v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
        if (flags & I2V_EPI_RESIDUAL) {
            float4 r = ((const float4*)res)[i];
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        if (flags & I2V_EPI_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        if (flags & I2V_EPI_MASK) {
            const float4 mk = ((const float4*)mask)[i];
            v.x = mk.x > 0.f ? v.x : 0.f; v.y = mk.y > 0.f ? v.y : 0.f; v.z = mk.z > 0.f ? v.z : 0.f; v.w = mk.w > 0.f ? v.w : 0.f;
        }
        ((float4*)y)[i] = v;
    }
}

__global__ void conv_epilogue_scalar_kernel(float* __restrict__ y, const float* __restrict__ scale,
                                            const float* __restrict__ shift, const float* __restrict__ res,
                                            const float* __restrict__ mask, long long total, int N, int flags) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(i % N);
        float v = y[i];
        if (flags & I2V_EPI_SCALE) v *= scale[n];
        if ((flags & (I2V_EPI_SCALE | I2V_EPI_BIAS)) && shift) v += shift[n];
        if (flags & I2V_EPI_RESIDUAL) v += res[i];
        if (flags & I2V_EPI_RELU) v = fmaxf(v, 0.f);
        if ((flags & I2V_EPI_MASK) && !(mask[i] > 0.f)) v = 0.f;
        y[i] = v;
    }
}

int g_force_tile = -1;           // i2v_conv_set_tile(): tuning hook (the tile index)
// Tuning knobs live in g_i2v_tuning (i2v_set_tuning; the library itself reads no environment variable); conv_plan.h reads them.

// One launch of a forward kernel that asks for up to 96 KB of dynamic LDS (allowed once per instantiation).
template <auto Kernel>
void launch_conv(dim3 grid, int threads, size_t lds, const ConvP& p, hipStream_t st) {
    static const bool once = [] {
        (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        return true;
    }();
    (void)once;
    Kernel<<<grid, threads, lds, st>>>(p);
}

// the kernels of one tile shape, by form and mask
template <int WAVES_M, int WAVES_N, int TM, int TN>
void launch_tile(int form, const ConvP& p, hipStream_t st) {
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16;
    const dim3 grid(i2v_cdiv(p.M, BM) * i2v_cdiv(p.N, BN), p.splitk, p.nbatch > 1 ? p.nbatch : 1);
    const size_t lds_g = (size_t)(2 * (BM + BN) * BKS) * sizeof(float);
    const bool mask = (p.flags & I2V_EPI_MASK) != 0;      // the MASK instantiations serve data gradients only
    switch (form) {
    case FORM_GEMM:
        if (mask) launch_conv<conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, true>>(grid, THREADS, lds_g, p, st);
        else if (p.clk) launch_conv<conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, true>>(grid, THREADS, lds_g, p, st);
        else launch_conv<conv_gemm_f32<WAVES_M, WAVES_N, TM, TN>>(grid, THREADS, lds_g, p, st);
        break;
    case FORM_GEMM_DMA32:
        if (mask) launch_conv<conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, true, 1, 1>>(grid, THREADS, lds_g, p, st);
        else launch_conv<conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, false, 1, 1>>(grid, THREADS, lds_g, p, st);
        break;
    case FORM_GEMM_DMA16:
        if (mask) launch_conv<conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, true, 1, 2>>(grid, THREADS, lds_g / 2, p, st);
        else launch_conv<conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, false, 1, 2>>(grid, THREADS, lds_g / 2, p, st);
        break;
    default: {
        const size_t stage = lds_g + p.ktab_entries * sizeof(float), epi = (size_t)BM * (BN + 4) * sizeof(float);
        launch_conv<conv_igemm_f32<WAVES_M, WAVES_N, TM, TN>>(grid, THREADS, stage > epi ? stage : epi, p, st);
    }
    }
}

// The intra-workgroup K split (conv_gemm_f32<.., KG>): one workgroup of KG x 4 waves per tile, KG stage-buffer sets in LDS.
template <int WAVES_M, int WAVES_N, int TM, int TN, int KG>
int launch_kgroups(const ConvP& p, hipStream_t st) {
    constexpr int BM = WAVES_M * TM * 16, BN = WAVES_N * TN * 16;
    constexpr int need = KG * 2 * (BM + BN) * BKS * 4;
    static_assert(need <= 159 * 1024, "the stage-buffer sets fit the CU's LDS");
    // exactly what the launch asks for: the kernel also has a few bytes of static LDS, and the attribute call fails (leaving
    // the 64 KB default in force) when dynamic + static would exceed the CU's 160 KB
    static const hipError_t once_k = [] {
        hipError_t e = hipFuncSetAttribute((const void*)conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, false, KG>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, need);
        hipError_t e2 = hipFuncSetAttribute((const void*)conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, true, KG>,
                                            hipFuncAttributeMaxDynamicSharedMemorySize, need);
        return e != hipSuccess ? e : e2;
    }();
    if (once_k != hipSuccess) {
        (void)hipGetLastError();
        i2v_set_error("conv: %d bytes of LDS refused for the K-group kernel: %s", need, hipGetErrorString(once_k));
        return I2V_ERR_LAUNCH;
    }
    const int tiles = i2v_cdiv(p.M, BM) * i2v_cdiv(p.N, BN);
    if (p.flags & I2V_EPI_MASK)
        conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, true, KG><<<dim3(tiles, 1, 1), THREADS * KG, need, st>>>(p);
    else
        conv_gemm_f32<WAVES_M, WAVES_N, TM, TN, false, false, KG><<<dim3(tiles, 1, 1), THREADS * KG, need, st>>>(p);
    return I2V_OK;
}

ConvShape shape_of(const ConvP& p) {
    return {p.B, p.H, p.W, p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.pad_x, p.ostride, p.Ho, p.Wo, p.nbatch, p.flags};
}

// plan (conv_plan.h), bind the workspace and clear, launch
int run_conv(ConvP p, hipStream_t st, void* split_ws = nullptr, size_t split_ws_bytes = 0) {
    const ConvShape shape = shape_of(p);
    const FwdPlan pl = plan_conv_fwd(shape, g_i2v_tuning, g_force_tile, g_clk != nullptr, split_ws ? split_ws_bytes : 0);
    if (pl.status != PLAN_OK) return plan_error(pl.status, shape);
    p.M = p.B * p.Ho * p.Wo;
    p.N = p.Cout;
    p.K = p.KH * p.KW * p.Cin;
    p.lgCin = ilog2_exact(p.Cin);
    p.ktab_entries = pl.ktab_entries;
    p.x_bytes = pl.x_bytes;
    p.w_bytes = pl.w_bytes;
    p.clk = g_clk;
    p.ablate = g_ablate;
    p.splitk = pl.splitk;
    p.k_per_split = pl.k_per_split;
    p.ws = nullptr;
    p.cnt = nullptr;
    if (pl.finish == FIN_IN_KERNEL) {
        p.cnt = reinterpret_cast<int*>(split_ws);
        p.ws = reinterpret_cast<float*>(static_cast<char*>(split_ws) + kSplitCounterBytes);
    }
    if (pl.ordered_fallback) ++g_ordered_fallbacks;
    const long long ytotal = (long long)p.M * p.N;
    if (pl.clear_y) hipMemsetAsync(p.y, 0, (size_t)ytotal * sizeof(float), st);
    switch (pl.form == FORM_GEMM_KGROUPS2 ? 10 + pl.kg_tile : pl.form == FORM_GEMM_KGROUPS4 ? 20 + pl.kg_tile : pl.tile) {
        case 0: launch_tile<2, 2, 4, 4>(pl.form, p, st); break;
        case 1: launch_tile<2, 2, 4, 2>(pl.form, p, st); break;
        case 2: launch_tile<2, 2, 3, 2>(pl.form, p, st); break;
        case 3: launch_tile<1, 4, 5, 1>(pl.form, p, st); break;
        case 4: launch_tile<2, 2, 2, 2>(pl.form, p, st); break;
        case 5: launch_tile<2, 2, 1, 2>(pl.form, p, st); break;
        case 10: return launch_kgroups<1, 4, 5, 1, 2>(p, st);
        case 11: return launch_kgroups<2, 2, 2, 2, 2>(p, st);
        case 12: return launch_kgroups<1, 4, 3, 1, 2>(p, st);
        case 13: return launch_kgroups<2, 2, 1, 2, 2>(p, st);
        case 20: return launch_kgroups<1, 4, 5, 1, kKGroups>(p, st);
        case 21: return launch_kgroups<2, 2, 2, 2, kKGroups>(p, st);
        case 22: return launch_kgroups<1, 4, 3, 1, kKGroups>(p, st);
        case 23: return launch_kgroups<2, 2, 1, 2, kKGroups>(p, st);
    }
    if (pl.epilogue_pass == PASS_VEC4)
        conv_epilogue_kernel<<<(int)fmin((double)i2v_cdiv(ytotal / 4, 256), 4096.0), 256, 0, st>>>(
            p.y, p.scale, p.shift, p.res, p.mask, ytotal / 4, p.N, p.flags);
    else if (pl.epilogue_pass == PASS_SCALAR)
        conv_epilogue_scalar_kernel<<<(int)fmin((double)i2v_cdiv(ytotal, 256), 4096.0), 256, 0, st>>>(
            p.y, p.scale, p.shift, p.res, p.mask, ytotal, p.N, p.flags);
    return I2V_OK;
}

// ---------------------------------------------------------------- dgrad helper
// wt[c][KH-1-ky][KW-1-kx][n] = w[n][ky][kx][c]: the filter of the transposed conv.
__global__ void weight_dgrad_layout(const float* __restrict__ w, float* __restrict__ wt, int Cout, int KH, int KW,
                                    int Cin, const float* __restrict__ nscale = nullptr) {
    const long long total = (long long)Cout * KH * KW * Cin;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        // i indexes wt: (c, ky', kx', n) with n fastest (coalesced writes)
        int n = i % Cout;
        long long t = i / Cout;
        int kx = t % KW; t /= KW;
        int ky = t % KH;
        int c = t / KH;
        // nscale: a per-filter factor on gy (the frozen-BN scale between the conv and the tensor gy belongs to) folded into
        // the transposed filter: dgrad(gy * s, w) == dgrad(gy, diag(s) w)
        const float v = w[(((long long)n * KH + (KH - 1 - ky)) * KW + (KW - 1 - kx)) * Cin + c];
        wt[i] = nscale ? v * nscale[n] : v;
    }
}

// Sub-filter of a strided dgrad: the input pixels of one parity class (iy % s, ix % s) only see the taps
// ky = ky0 + s*t: wt[c][Ty-1-ty][Tx-1-tx][n] = w[n][ky0 + s*ty][kx0 + s*tx][c].
__global__ void weight_dgrad_sub_layout(const float* __restrict__ w, float* __restrict__ wt, int Cout, int KH, int KW,
                                        int Cin, int s, int ky0, int kx0, int Ty, int Tx) {
    const long long total = (long long)Cin * Ty * Tx * Cout;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        int n = i % Cout;
        long long t = i / Cout;
        int ux = t % Tx; t /= Tx;
        int uy = t % Ty;
        int c = t / Ty;
        const int ky = ky0 + s * (Ty - 1 - uy), kx = kx0 + s * (Tx - 1 - ux);
        wt[i] = w[(((long long)n * KH + ky) * KW + kx) * Cin + c];
    }
}

}  // namespace

// Reductions that were asked to be ordered (I2V_TUNE_SPLIT_ATOMICS == 0) and fell back to fp32 atomics because the caller's
// workspace was absent or too small (round-5 advice: the fallback was silent).  i2v_ordered_fallbacks() reads / resets it.
extern "C" int32_t i2v_ordered_fallbacks(int32_t reset) {
    const int n = g_ordered_fallbacks;
    if (reset) g_ordered_fallbacks = 0;
    return n;
}

extern "C" int32_t i2v_conv_debug_clock(void* buf) {
    g_clk = (unsigned long long*)buf;      // device buffer of 2 u64 per workgroup, or NULL to switch off
    return I2V_OK;
}

namespace {
__global__ void clock_stamp_kernel(unsigned long long* out) {
    if (threadIdx.x == 0) { out[0] = __builtin_amdgcn_s_memtime(); out[1] = __builtin_amdgcn_s_memrealtime(); }
}
}  // namespace

extern "C" int32_t i2v_debug_clock_stamp(void* out2, void* stream) {
    clock_stamp_kernel<<<1, 64, 0, (hipStream_t)stream>>>((unsigned long long*)out2);
    I2V_CHECK_LAUNCH("i2v_debug_clock_stamp");
    return I2V_OK;
}

extern "C" int32_t i2v_conv_set_tile(int32_t cfg) {
    if (cfg < 0) { g_force_tile = -1; g_ablate = 0; return I2V_OK; }
    if (cfg >> 8) {         // rounds 1-5: bits 8-9 selected the 8-wave loader / MFMA specialisation, bits 10+ ablation instantiations
        i2v_set_error("conv_set_tile: bits above the tile index selected experiment kernels that left the library in round 6");
        return I2V_ERR_UNSUPPORTED;
    }
    g_force_tile = (cfg & 0xFF) == 0xFF ? -1 : (cfg & 0xFF);
    return I2V_OK;
}

// the plan of i2v_conv_fwd (nbatch <= 1) or i2v_gemm_nt_batched (its M x K operand as a 1 x M x 1 x K activation) for a shape
static int plan_conv(const char* who, FwdPlan& pl, size_t ws_bytes, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                     int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t nbatch = 0, int32_t flags = 0) {
    int dummy = 0;
    int rc = check_conv(who, &dummy, &dummy, &dummy, B, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    const ConvShape s = {B, H, W, Cin, Cout, KH, KW, stride, pad, pad, 1, (H + 2 * pad - KH) / stride + 1, (W + 2 * pad - KW) / stride + 1,
                         nbatch, flags};
    pl = plan_conv_fwd(s, g_i2v_tuning, g_force_tile, g_clk != nullptr, ws_bytes);
    return plan_error(pl.status, s);
}

// 1 if i2v_conv_fwd, given a split-K workspace of ws_bytes, will accumulate split-K partials with atomics for this
// shape (its output must then start at zero: the call clears it itself unless the caller passes I2V_EPI_ZEROED),
// 0 otherwise, < 0 on error.
extern "C" int32_t i2v_conv_fwd_splits(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH,
                                       int32_t KW, int32_t stride, int32_t pad, size_t ws_bytes) {
    FwdPlan pl = {};
    const int rc = plan_conv("conv_fwd_splits", pl, ws_bytes, B, H, W, Cin, Cout, KH, KW, stride, pad);
    return rc < 0 ? rc : pl.finish == FIN_ATOMICS;
}

// Bytes of split-K workspace i2v_conv_fwd would use for this shape (0: it does not split K, or it splits into so many
// parts / so small an output that fp32 atomics are the better finish).
extern "C" size_t i2v_conv_split_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH,
                                                 int32_t KW, int32_t stride, int32_t pad) {
    FwdPlan pl = {};
    return plan_conv("conv_fwd_splits", pl, 0, B, H, W, Cin, Cout, KH, KW, stride, pad) ? 0 : pl.ws_wanted;
}

// The forward plan as numbers (include/i2vsgg_hip.h has the field order): what the launch of this shape would do.
extern "C" int32_t i2v_conv_fwd_plan(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                                     int32_t stride, int32_t pad, int32_t nbatch, int32_t flags, size_t ws_bytes, int32_t* out,
                                     int32_t n_out) {
    I2V_CHECK_ARG(out && n_out >= I2V_FWD_PLAN_FIELDS, "conv_fwd_plan: out needs room for I2V_FWD_PLAN_FIELDS values");
    FwdPlan pl = {};
    const int rc = plan_conv("conv_fwd_plan", pl, ws_bytes, B, H, W, Cin, Cout, KH, KW, stride, pad, nbatch, flags);
    if (rc && pl.status == PLAN_OK) return rc;      // a bad argument; an unsupported shape is reported in out[0]
    const int32_t v[I2V_FWD_PLAN_FIELDS] = {pl.status, pl.tile, pl.splitk, pl.k_per_split, pl.ktab_entries, pl.form, pl.kg_tile,
                                            pl.finish, clamp32(pl.ws_wanted), clamp32(pl.ws_used), pl.clear_y, pl.epilogue_pass,
                                            pl.ordered_fallback};
    std::copy(v, v + I2V_FWD_PLAN_FIELDS, out);
    return I2V_OK;
}

extern "C" int32_t i2v_conv_fwd(const float* x, const float* w, const float* scale, const float* shift,
                                const float* res, float* y, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t flags,
                                void* split_ws, size_t split_ws_bytes, void* stream) {
    int rc = check_conv("conv_fwd", x, w, y, B, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    I2V_CHECK_ARG(!(flags & I2V_EPI_SCALE) || (scale && shift), "conv_fwd: EPI_SCALE needs scale and shift");
    I2V_CHECK_ARG(!(flags & I2V_EPI_BIAS) || shift, "conv_fwd: EPI_BIAS needs shift");
    I2V_CHECK_ARG(!(flags & I2V_EPI_RESIDUAL) || res, "conv_fwd: EPI_RESIDUAL needs res");
    ConvP p = {};
    p.x = x; p.w = w; p.scale = scale; p.shift = shift; p.res = res; p.y = y;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad; p.pad_x = pad;
    p.Ho = (H + 2 * pad - KH) / stride + 1;
    p.Wo = (W + 2 * pad - KW) / stride + 1;
    p.flags = flags; p.ostride = 1; p.Hy = p.Ho; p.Wy = p.Wo;
    rc = run_conv(p, (hipStream_t)stream, split_ws, split_ws_bytes);
    if (rc) return rc;
    I2V_CHECK_LAUNCH("conv_fwd");
    return I2V_OK;
}

// nbatch independent GEMMs of one shape in ONE launch: C_z (M x N) = A_z (M x K) * B_z (N x K)^T, fp32, operand z at
// base + z * stride (elements).  The 16 element-wise planes of a Winograd convolution are such a batch.
extern "C" int32_t i2v_gemm_nt_batched(const float* a, const float* b, float* c, int32_t M, int32_t N, int32_t K,
                                       int32_t nbatch, int64_t stride_a, int64_t stride_b, int64_t stride_c,
                                       void* split_ws, size_t split_ws_bytes, void* stream) {
    I2V_CHECK_ARG(a && b && c && M > 0 && N > 0 && K > 0 && nbatch > 0 && nbatch <= 65535, "gemm_nt_batched: bad argument");
    I2V_CHECK_ARG(K % 4 == 0, "gemm_nt_batched: K must be a multiple of 4");
    ConvP p = {};
    p.x = a; p.w = b; p.y = c;
    p.B = 1; p.H = M; p.W = 1; p.Cin = K; p.Cout = N; p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0; p.pad_x = 0;
    p.Ho = M; p.Wo = 1; p.flags = 0; p.ostride = 1; p.Hy = M; p.Wy = 1;
    p.nbatch = nbatch; p.bsx = stride_a; p.bsw = stride_b; p.bsy = stride_c;
    int rc = run_conv(p, (hipStream_t)stream, split_ws, split_ws_bytes);
    if (rc) return rc;
    I2V_CHECK_LAUNCH("gemm_nt_batched");
    return I2V_OK;
}

extern "C" size_t i2v_conv_dgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t KH, int32_t KW) {
    return i2v_align((size_t)Cout * KH * KW * Cin * sizeof(float));
}

// dgrad = forward conv of gy with the flipped/transposed filter (staged in the workspace).
//
// stride s > 1, KxK filter: an input pixel iy = s*a + r only receives taps ky = (r + pad) % s + s*t, from
// output rows a + c0 - t with c0 = (r + pad - ky0) / s.  So every parity class (ry, rx) is its own stride-1
// correlation of gy with a flipped sub-filter, written to every s-th pixel of gx: s*s launches whose MACs add up
// to exactly the dense count (the zero-insertion form did s*s times that).
static int conv_dgrad_impl(const float* gy, const float* w, const float* gy_scale, const float* out_scale,
                           const float* res, const float* mask, float* gx, int32_t B, int32_t H, int32_t W,
                           int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                           void* ws, size_t ws_bytes, void* split_ws, size_t split_ws_bytes, void* stream) {
    int rc = check_conv("conv_dgrad", gy, w, gx, B, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    const bool fused = gy_scale || out_scale || res || mask;
    if (fused && stride != 1 && !(KH == 1 && KW == 1 && pad == 0)) {
        i2v_set_error("conv_dgrad_fused: stride 1, or a strided 1x1 layer (other strided layers take i2v_conv_dgrad and separate passes)");
        return I2V_ERR_UNSUPPORTED;
    }
    I2V_CHECK_ARG(Cout % 4 == 0, "conv_dgrad: Cout must be a multiple of 4");
    if (!ws || ws_bytes < (size_t)Cout * KH * KW * Cin * sizeof(float)) {
        i2v_set_error("conv_dgrad: workspace too small");
        return I2V_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    ConvP p = {};
    p.x = gy; p.y = gx;
    p.B = B; p.H = Ho; p.W = Wo; p.Cin = Cout; p.Cout = Cin; p.stride = 1;
    p.flags = 0;
    if (out_scale) { p.scale = out_scale; p.shift = nullptr; p.flags |= I2V_EPI_SCALE; }
    if (res) { p.res = res; p.flags |= I2V_EPI_RESIDUAL; }
    if (mask) { p.mask = mask; p.flags |= I2V_EPI_MASK; }
    p.Hy = H; p.Wy = W;
    const bool pointwise = KH == 1 && KW == 1 && pad == 0;
    if (stride == 1 || pointwise) {
        const long long wn = (long long)Cout * KH * KW * Cin;
        weight_dgrad_layout<<<(int)fmin((double)i2v_cdiv(wn, 256), 4096.0), 256, 0, st>>>(w, (float*)ws, Cout, KH, KW, Cin, gy_scale);
        p.w = (const float*)ws;
        p.KH = KH; p.KW = KW;
        if (stride == 1) {
            I2V_CHECK_ARG(KH - 1 - pad >= 0 && KW - 1 - pad >= 0, "conv_dgrad: padding larger than the filter");
            p.pad = KH - 1 - pad; p.pad_x = KW - 1 - pad;
            p.Ho = H; p.Wo = W; p.ostride = 1;
        } else {                    // strided 1x1: every s-th pixel gets a value (epilogue operands are read at that pixel), the
            p.pad = 0; p.pad_x = 0; p.Ho = Ho; p.Wo = Wo; p.ostride = stride;       // rest are zero -- res must be zero there too
            hipMemsetAsync(gx, 0, (size_t)B * H * W * Cin * sizeof(float), st);
        }
        rc = run_conv(p, st, split_ws, split_ws_bytes);
        if (rc) return rc;
        I2V_CHECK_LAUNCH("conv_dgrad");
        return I2V_OK;
    }
    // parity decomposition
    bool all_written = true;
    for (int r = 0; r < stride; ++r) {
        if ((r + pad) % stride >= KH || (r + pad) % stride >= KW) all_written = false;
    }
    // pixels beyond the last window (iy + pad - ky > s*(Ho-1) for every tap) still get zeros from the masked taps
    if (!all_written) hipMemsetAsync(gx, 0, (size_t)B * H * W * Cin * sizeof(float), st);
    float* wsub = (float*)ws;
    for (int ry = 0; ry < stride && ry < H; ++ry) {
        const int ky0 = (ry + pad) % stride;
        if (ky0 >= KH) continue;
        const int Ty = (KH - ky0 + stride - 1) / stride, c0y = (ry + pad - ky0) / stride;
        for (int rx = 0; rx < stride && rx < W; ++rx) {
            const int kx0 = (rx + pad) % stride;
            if (kx0 >= KW) continue;
            const int Tx = (KW - kx0 + stride - 1) / stride, c0x = (rx + pad - kx0) / stride;
            const long long wn = (long long)Cin * Ty * Tx * Cout;
            weight_dgrad_sub_layout<<<(int)fmin((double)i2v_cdiv(wn, 256), 4096.0), 256, 0, st>>>(
                w, wsub, Cout, KH, KW, Cin, stride, ky0, kx0, Ty, Tx);
            ConvP q = p;
            q.w = wsub;
            q.KH = Ty; q.KW = Tx;
            q.pad = Ty - 1 - c0y; q.pad_x = Tx - 1 - c0x;          // may be negative: the window starts inside gy
            q.Ho = (H - ry + stride - 1) / stride;                    // pixels of this parity class
            q.Wo = (W - rx + stride - 1) / stride;
            q.ostride = stride;
            q.y = gx + ((long long)ry * W + rx) * Cin;
            rc = run_conv(q, st, split_ws, split_ws_bytes);
            if (rc) return rc;
            wsub += wn;
        }
    }
    I2V_CHECK_LAUNCH("conv_dgrad");
    return I2V_OK;
}

extern "C" int32_t i2v_conv_dgrad(const float* gy, const float* w, float* gx, int32_t B, int32_t H, int32_t W,
                                  int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                  void* ws, size_t ws_bytes, void* split_ws, size_t split_ws_bytes, void* stream) {
    return conv_dgrad_impl(gy, w, nullptr, nullptr, nullptr, nullptr, gx, B, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes,
                           split_ws, split_ws_bytes, stream);
}

extern "C" int32_t i2v_conv_dgrad_fused(const float* gy, const float* w, const float* gy_scale, const float* out_scale,
                                        const float* res, const float* mask, float* gx, int32_t B, int32_t H, int32_t W,
                                        int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                        void* ws, size_t ws_bytes, void* split_ws, size_t split_ws_bytes, void* stream) {
    return conv_dgrad_impl(gy, w, gy_scale, out_scale, res, mask, gx, B, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes,
                           split_ws, split_ws_bytes, stream);
}
