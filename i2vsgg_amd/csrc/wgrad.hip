// The filter gradient of the fp32 convolutions / linear layers (conv.hip) on the CDNA4 matrix cores.
//
//   gw[n][k] (+)= sum_m gy[m][n] * A[m][k]     reduction over the output pixels m, A = the im2col matrix of x
// Both operands arrive reduction-major from HBM (gy rows are n-contiguous, im2col rows are c-contiguous), so the staging
// pass transposes them into the [row][kk] LDS image the MFMA fragments want; the reduction is split over m.
// conv_wgrad2_f32 is the product kernel: 16x16x4 MFMAs, 32 pixels per stage, swizzled 128-B LDS rows, register-staged or
// LDS-DMA (pointwise problems), with the SGD update fused into its epilogue where the reduction fits one pass.  A split
// over pixels ends in fp32 atomics, in an ordered in-kernel finish, or in partial filters summed in split order by
// wgrad_reduce_kernel / _scalar_kernel.  conv_wgrad_f32 is the first-generation kernel, kept for the shapes the second
// does not take (Cout % 4 != 0).  fc_update_f32 is the persistent fused gradient + SGD update of a linear layer of at
// most 256 rows.  plan_wgrad (conv_plan.h) picks among them; launch_wgrad binds the workspace, clears and switches.
#include "conv_common.h"

using namespace convplan;

namespace {

constexpr int BK = 16;          // k per LDS stage of the wgrad kernel
constexpr int LDS_ROW = 20;     // floats per staged row (16 + 4 pad)

struct WgP {
    const float* x; const float* gy; float* gw; int direct;
    const float* row_scale;                // gw[n][:] = row_scale[n] * sum (a frozen-BN scale on gy applied where the sum ends), or NULL
    int xcd_remap;                         // (tile, split, plane) from the dispatch index so that a split's tiles share an XCD (launch_wgrad)
    int r_tiles, r_splits, r_total;        // with xcd_remap: the logical grid (tiles x splits x planes = r_total workgroups) behind the 1-D launch
    int nbatch;                            // > 1: blockIdx.z selects one of nbatch independent GEMMs (the planes of a Winograd filter gradient)
    long long bsx, bsg, bsw;               // element strides between the batches of x, gy and gw
    float* sgd_m; float lr, mom, wd;       // sgd_m != NULL: gw is the PARAMETER, updated in place (fused SGD)
    unsigned x_bytes, gy_bytes;            // buffer descriptor sizes (v2 kernel)
    int B, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo, M, N, K, m_per_split, lgCin;
    unsigned long long* clk;               // diagnostic (i2v_conv_debug_clock): per-workgroup stamps, CLK instantiation only
    int abl;                               // diagnostic instantiation only: ablation bits (i2v_conv_set_tile bits 10-12)
    // ordered finish of a split over pixels (round 5): partial tiles through the caller's split workspace, summed in split
    // order by the last workgroup to arrive at the tile's counter (the protocol of conv_igemm_f32's split-K finish): the sum
    // does not depend on arrival order, no clear of gw in front.  ord_ws == NULL: fp32 atomics into a cleared gw.
    float* ord_ws; int* ord_cnt; int ord_splits, ord_tiles, ord_acc;      // ord_acc: gw += sum (beta = 1) instead of gw = sum
    // two-pass ordered finish (round 6): a split of MORE parts than one finisher should read (or of the first-generation kernel,
    // which has no in-kernel finish): every split stores its partial filter in gw's own layout at part_ws[(split * planes + plane)
    // * N * K ...] with plain stores, and a reduce pass (wgrad_reduce_kernel, or the Winograd filter gradient's final transform)
    // sums the parts in split order.  No counter, no clear of gw, all of the chip reads the parts.
    float* part_ws;
    int part_cap;                          // a caller-owned part_ws (launch_wgrad's ext_part): the parts it has room for
};

// First generation: v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulate) from ds_read_b128 fragments of a 16-deep stage.
// LDS tile rows are 16 floats + 4 pad (80 B): a 16-lane ds_read_b128 group then hits 16 distinct 16-B slots of the
// 256-B bank row (row*5 mod 16 is a bijection) - conflict free.  K order inside a 8-deep step is permuted (lane half h
// owns k = 4h..4h+3) so a fragment is ONE b128 read; A and B use the same permutation, so the sum is unchanged.
template <int BM, int BN>   // BM over n (Cout), BN over k; 4 waves as 2x2, 64x64 tiles: BM=BN=64 -> wave 32x32
__global__ void __launch_bounds__(THREADS)
conv_wgrad_f32(const WgP p) {
    constexpr int MI = BM / 64, NI = BN / 64;
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_ROW];   // [n][mm]
    __shared__ __attribute__((aligned(16))) float Bs[BN * LDS_ROW];   // [k][mm]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_k = (p.K + BN - 1) / BN;
    const int n0 = (blockIdx.x / tiles_k) * BM, k0 = (blockIdx.x % tiles_k) * BN;
    const int mbeg = blockIdx.y * p.m_per_split, mend = min(p.M, mbeg + p.m_per_split);

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // staging roles: a stage is 16 reduction rows (m) x BM (or BN) columns; one float4 = 4 columns
    constexpr int A_V = 16 * BM / 4 / THREADS, B_V = 16 * BN / 4 / THREADS;
    const int fr = lane & 31, fh = lane >> 5;
    for (int ms = mbeg; ms < mend; ms += 16) {
        float4 ra[A_V], rb[B_V];
#pragma unroll
        for (int q = 0; q < A_V; ++q) {
            const int slot = tid + q * THREADS;
            const int mm = slot / (BM / 4), col = (slot % (BM / 4)) * 4;
            const int m = ms + mm, n = n0 + col;
            ra[q] = make_float4(0, 0, 0, 0);
            if (m < mend && n < p.N) {
                const float* g = p.gy + (long long)m * p.N + n;
                if (n + 3 < p.N && (p.N & 3) == 0) ra[q] = *(const float4*)g;
                else { ra[q].x = g[0]; if (n + 1 < p.N) ra[q].y = g[1]; if (n + 2 < p.N) ra[q].z = g[2]; if (n + 3 < p.N) ra[q].w = g[3]; }
            }
        }
#pragma unroll
        for (int q = 0; q < B_V; ++q) {
            const int slot = tid + q * THREADS;
            const int mm = slot / (BN / 4), col = (slot % (BN / 4)) * 4;
            const int m = ms + mm, k = k0 + col;
            rb[q] = make_float4(0, 0, 0, 0);
            if (m < mend && k < p.K) {
                int kpos, c;
                if (p.lgCin >= 0) { kpos = k >> p.lgCin; c = k & (p.Cin - 1); } else { kpos = k / p.Cin; c = k - kpos * p.Cin; }
                const int ky = kpos / p.KW, kx = kpos - ky * p.KW;
                const int ox = m % p.Wo, t = m / p.Wo, oy = t % p.Ho, b = t / p.Ho;
                const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
                if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                    rb[q] = *(const float4*)(p.x + (((long long)b * p.H + iy) * p.W + ix) * p.Cin + c);
            }
        }
        __syncthreads();      // previous stage fully consumed
#pragma unroll
        for (int q = 0; q < A_V; ++q) {
            const int slot = tid + q * THREADS;
            const int mm = slot / (BM / 4), col = (slot % (BM / 4)) * 4;
            As[(col + 0) * LDS_ROW + mm] = ra[q].x; As[(col + 1) * LDS_ROW + mm] = ra[q].y;
            As[(col + 2) * LDS_ROW + mm] = ra[q].z; As[(col + 3) * LDS_ROW + mm] = ra[q].w;
        }
#pragma unroll
        for (int q = 0; q < B_V; ++q) {
            const int slot = tid + q * THREADS;
            const int mm = slot / (BN / 4), col = (slot % (BN / 4)) * 4;
            Bs[(col + 0) * LDS_ROW + mm] = rb[q].x; Bs[(col + 1) * LDS_ROW + mm] = rb[q].y;
            Bs[(col + 2) * LDS_ROW + mm] = rb[q].z; Bs[(col + 3) * LDS_ROW + mm] = rb[q].w;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float4 av[MI], bv[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) av[i] = *(const float4*)&As[(wm * (BM / 2) + i * 32 + fr) * LDS_ROW + s * 8 + fh * 4];
#pragma unroll
            for (int j = 0; j < NI; ++j) bv[j] = *(const float4*)&Bs[(wn * (BN / 2) + j * 32 + fr) * LDS_ROW + s * 8 + fh * 4];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int k = k0 + wn * (BN / 2) + j * 32 + fr;
        if (k >= p.K) continue;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (n < p.N) {
                    const long long o = (long long)n * p.K + k;
                    if (p.sgd_m) {          // g' = g + wd*p ; m = mom*m + g' ; p -= lr*m   (same order as sgd_momentum_kernel)
                        const float pv = p.gw[o];
                        const float mv = p.mom * p.sgd_m[o] + (acc[i][j][r] + p.wd * pv);
                        p.sgd_m[o] = mv;
                        p.gw[o] = pv - p.lr * mv;
                    } else if (p.direct) {
                        p.gw[o] = acc[i][j][r];
                    } else if (p.part_ws) {
                        p.part_ws[(long long)blockIdx.y * p.N * p.K + o] = acc[i][j][r];
                    } else {
                        atomicAdd(p.gw + o, acc[i][j][r]);
                    }
                }
            }
    }
}

// ---------------------------------------------------------------- wgrad v2
// Same GEMM as conv_wgrad_f32 on the conv_igemm_f32 machinery: 16x16x4 MFMAs, 32 reduction rows per
// stage, swizzled 128-B LDS rows, register prefetch + double-buffered LDS.  Both operands arrive
// reduction-major, so every thread owns 4x4 blocks (4 consecutive pixels x 4 columns): four 16-B loads,
// an in-register transpose, four ds_write_b128 -- no scalar LDS traffic, no bank-conflicted transposes.
// FUSED_SGD: the instantiation that runs the SGD update in its epilogue (prefetches the filter / momentum tiles:
// +34 VGPRs, four waves per SIMD instead of five -- which the plain gradient kernel should not pay)
// LDS column swizzle of the filter-gradient kernel.  A fragment read touches 16 consecutive rows of one 16-row group: any
// bijection of (row >> 1) & 7 keeps it conflict-free, and a term in row >> 4 is constant there.  The transposing stores of a
// 16-lane group go to rows 4 cg + i (cg = 0..15, four columns per thread): (row >> 1) & 7 alone takes FOUR values there -- a
// four-way bank conflict on every ds_write_b128; with bit 4 of the row folded in it takes eight (two-way, the best a
// 4-column block allows: the rows of a group share their parity, which picks the half of the 256-byte bank row).
__device__ inline int wswz(int row) { return ((row >> 1) & 7) ^ ((row >> 4) & 1); }
constexpr bool WGRAD_ROWMAJOR = false;     // LDS image of the filter-gradient kernel: the transposed [column][pixel] one (false), or [pixel][column] as the operands
                                           // arrive (true: no register transposes, conflict-free 16-byte stores, one-float fragment reads merged into
                                           // ds_read2st64_b32 -- bit-equal, measured 3 % slower on the layer3 shapes: 113.8 vs 110.3 us)

// DMA (round 6, I2V_TUNE_WGRAD_DMA; pointwise / linear problems only: pixel index in == pixel index out): the stage tiles go
// from global memory to LDS without passing through registers (lds_dma16), as in conv_gemm_f32.  The DMA lands lane-linear, so the
// LDS image is the [pixel][column] one (WGRAD_ROWMAJOR's) with its 16-column-group swizzle applied to the SOURCE column: a 1-KB
// piece is 4 (2) consecutive pixel rows of a 64- (128-) column tile.  No staging registers (64 of the 128 VGPRs of the 64x64
// form), no register transposes, no ds_write; the stage offset rides in the scalar offset of the request, the per-lane offsets
// are loop constants.  Same MFMA order per accumulator: bit-equal to the register-staged forms.
template <int TM, int TN, bool FUSED_SGD = false, bool CLK = false, bool DMA = false>       // tile = (2*TM*16) filters x (2*TN*16) taps, 4 waves as 2x2
__global__ void __launch_bounds__(THREADS)
conv_wgrad2_f32(const WgP p_in) {
    WgP p = p_in;
    unsigned long long c_rt0 = 0, c_t0 = 0, c_t1 = 0, c_t2 = 0;
    if constexpr (CLK) { c_rt0 = __builtin_amdgcn_s_memrealtime(); c_t0 = __builtin_amdgcn_s_memtime(); }
    // XCD-aware order (p.xcd_remap): workgroups are dealt to the 8 XCDs round robin in dispatch order, and every XCD has its own
    // L2.  All tiles of one pixel range (one split of one plane: a GROUP) read the same rows of gy and x; dealt in (tile, split)
    // order they land on all 8 XCDs and every L2 fetches those rows again (PMC: 3.6x the algorithmic bytes on the layer3
    // shapes).  Round 2 put group s on XCD s % 8 -- possible only when the group count is a multiple of 8, which the
    // pixel split rarely is (254 splits for layer1's expansion at 8 frames).  Round 4: the launch is 1-D and XCD g owns the
    // CONTIGUOUS range [g W / 8, (g + 1) W / 8) of the group-major workgroup order (W = tiles x groups): every XCD gets the
    // same number of workgroups (+-1) whatever the group count, a group lives on one XCD (two where a range boundary cuts
    // it).  The launch is padded to a multiple of 8; the <= 7 surplus workgroups leave at once.
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (p.xcd_remap) {
        const int L = (int)blockIdx.x, g = L & 7, r = L >> 3;
        const long long W = p.r_total;
        const int start = (int)((g * W) >> 3), count = (int)(((g + 1) * W) >> 3) - start;
        if (r >= count) return;
        const int idx = start + r, grp = idx / p.r_tiles;
        bx = idx - grp * p.r_tiles;
        by = grp % p.r_splits;
        bz = grp / p.r_splits;
    }
    if (p.nbatch > 1) {
        p.x += (long long)bz * p.bsx;
        p.gy += (long long)bz * p.bsg;
        p.gw += (long long)bz * p.bsw;
    }
    constexpr int BMW = 2 * TM * 16, BNW = 2 * TN * 16;
    constexpr bool ROWMAJOR = WGRAD_ROWMAJOR || DMA;
    static_assert(!DMA || (!FUSED_SGD && !CLK), "the LDS-DMA form is the plain gradient kernel");
    constexpr int A_BLK = BMW * 2, B_BLK = BNW * 2;             // (cols/4) * 8 row-groups
    constexpr int NBLK = DMA ? 1 : (A_BLK + B_BLK + THREADS - 1) / THREADS;     // (DMA: the register-staging roles below are dead code)
    constexpr int STAGE_FLOATS = 2 * (BMW + BNW) * BKS;
    constexpr int CROW = BNW + 4;
    constexpr int SMEM_FLOATS = STAGE_FLOATS > BMW * CROW ? STAGE_FLOATS : BMW * CROW;
    __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
    float (*As)[BMW * BKS] = reinterpret_cast<float (*)[BMW * BKS]>(smem);
    float (*Bs)[BNW * BKS] = reinterpret_cast<float (*)[BNW * BKS]>(smem + 2 * BMW * BKS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_k = (p.K + BNW - 1) / BNW;
    const int n0 = (bx / tiles_k) * BMW, k0 = (bx % tiles_k) * BNW;
    const int mbeg = by * p.m_per_split, mend = min(p.M, mbeg + p.m_per_split);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc((void*)p.gy, 0, p.gy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    constexpr unsigned OOB = 0xFFFFFFF0u;

    // per-thread block roles (fixed over the m loop)
    bool is_a[NBLK], live[NBLK];
    int cg[NBLK], m4[NBLK], coff[NBLK], ky[NBLK], kx[NBLK];
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
        const int id = tid + q * THREADS;
        is_a[q] = id < A_BLK;
        const int j = is_a[q] ? id : id - A_BLK;
        const int groups = (is_a[q] ? BMW : BNW) / 4;
        live[q] = id < A_BLK + B_BLK;
        cg[q] = j % groups;
        m4[q] = j / groups;
        ky[q] = kx[q] = 0;
        if (is_a[q]) {
            const int n = n0 + 4 * cg[q];
            coff[q] = n;
            live[q] = live[q] && n < p.N;
        } else {
            const int k = k0 + 4 * cg[q];
            live[q] = live[q] && k < p.K;
            int kpos, c;
            const int kk = live[q] ? k : 0;
            if (p.lgCin >= 0) { kpos = kk >> p.lgCin; c = kk & (p.Cin - 1); } else { kpos = kk / p.Cin; c = kk - kpos * p.Cin; }
            ky[q] = kpos / p.KW;
            kx[q] = kpos - ky[q] * p.KW;
            coff[q] = c;
        }
    }
    float4 r[NBLK][4];
    // pointwise layers on the same grid (and linear layers): input pixel index == output pixel index, no pixel arithmetic
    const bool lin = p.KH == 1 && p.KW == 1 && p.pad == 0 && p.stride == 1;     // uniform
    // other filters: the (ox, oy, b) of a block's first pixel is divided out ONCE and then carried from stage to stage
    // (stages advance by 32 pixels; one conditional wrap suffices while a row holds at least 32 pixels) -- the three
    // integer divisions per stage and block were ~100 of the ~250 vector instructions a stage issues beside its 32 MFMAs
    // (tools/wgrad_phase.py: 6.2k cycles per stage against 4.1k of MFMA time at 4 workgroups per CU)
    const bool carry = p.Wo >= BKS;
    int sx[NBLK], sy[NBLK], sb[NBLK];
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
        sx[q] = sy[q] = sb[q] = 0;
        if (lin) continue;                   // uniform: the skinny GEMMs of the relation head live ~4 stages, set-up counts
        const int m0 = mbeg + 4 * m4[q];
        sx[q] = m0 % p.Wo;
        const int tt = m0 / p.Wo;
        sy[q] = tt % p.Ho;
        sb[q] = tt / p.Ho;
    }
    // No divergent control flow around the loads: the A/B role of a block is uniform per wave (A_BLK is a multiple of
    // 128), so the descriptor is picked with a scalar select, and a masked element gets the 2 GiB bit OR-ed into its
    // offset (the buffer returns 0) -- written as `cond ? off : OOB` the compiler wraps every load in its own branch.
    auto gload = [&](int ms) {
#pragma unroll
        for (int q = 0; q < NBLK; ++q) {
            const bool a_u = __builtin_amdgcn_readfirstlane((int)is_a[q]) != 0;
            const __amdgpu_buffer_rsrc_t rs = a_u ? gr : xr;
            const int m0 = ms + 4 * m4[q];
            int ox = sx[q], oy = sy[q], b = sb[q];
            if (!a_u && !lin) {
                if (carry) {                // next stage: 32 pixels on
                    int nx = ox + BKS, ny = oy, nb = b;
                    if (nx >= p.Wo) { nx -= p.Wo; ++ny; if (ny == p.Ho) { ny = 0; ++nb; } }
                    sx[q] = nx; sy[q] = ny; sb[q] = nb;
                } else {                    // short rows (the 7x7 / 4x4 maps of the ROI head): divide
                    ox = m0 % p.Wo;
                    const int tt = m0 / p.Wo;
                    oy = tt % p.Ho;
                    b = tt / p.Ho;
                }
            }
            // The offsets are computed under uniform branches, the LOADS are not: a load inside a branch makes the number of
            // loads in flight unknowable to the compiler, which then drains everything (vmcnt(0)) before the first LDS
            // store -- the fused-SGD form would wait for its prefetched filter / momentum tiles there (fc6: +17 %).
            unsigned offs[4];
            if (a_u || lin) {               // row m of gy / of x: no pixel arithmetic
                const int rowlen = a_u ? p.N : p.Cin;
#pragma unroll
                for (int t = 0; t < 4; ++t) offs[t] = (unsigned)((m0 + t) * rowlen + coff[q]) * 4u;
            } else if (p.Wo >= 4) {
                // the block's 4 consecutive pixels: offsets from the first one's by increments (a pixel past the end of the
                // row moves to the next row -- or the next image -- by one precomputed delta: rows hold >= 4 pixels)
                const int iy0 = oy * p.stride - p.pad + ky[q], ix0 = ox * p.stride - p.pad + kx[q];
                const int base = ((b * p.H + iy0) * p.W + ix0) * p.Cin + coff[q];
                const bool last_row = oy + 1 == p.Ho;
                const int iy1 = last_row ? ky[q] - p.pad : iy0 + p.stride;                     // row of the pixels after a wrap
                const int wrap_delta = ((last_row ? p.H - (p.Ho - 1) * p.stride : p.stride) * p.W - p.Wo * p.stride) * p.Cin;
                const bool y0_in = iy0 >= 0 && iy0 < p.H, y1_in = iy1 >= 0 && iy1 < p.H;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const bool w = ox + t >= p.Wo;
                    const int ix = ix0 + t * p.stride - (w ? p.Wo * p.stride : 0);
                    const bool inside = (w ? y1_in : y0_in) && ix >= 0 && ix < p.W;
                    offs[t] = ((unsigned)(base + t * p.stride * p.Cin + (w ? wrap_delta : 0)) * 4u) | (inside ? 0u : 0x80000000u);
                }
            } else {                        // rows shorter than a block: pixel by pixel
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int iy = oy * p.stride - p.pad + ky[q], ix = ox * p.stride - p.pad + kx[q];
                    const bool inside = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                    offs[t] = ((unsigned)(((b * p.H + iy) * p.W + ix) * p.Cin + coff[q]) * 4u) | (inside ? 0u : 0x80000000u);
                    const bool wx = ox + 1 == p.Wo;
                    const bool wy = wx && oy + 1 == p.Ho;
                    ox = wx ? 0 : ox + 1;
                    oy = wy ? 0 : (wx ? oy + 1 : oy);
                    b += wy ? 1 : 0;
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned off = offs[t] | ((live[q] && m0 + t < mend) ? 0u : 0x80000000u);
                r[q][t] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
            }
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NBLK; ++q) {
            if (tid + q * THREADS >= A_BLK + B_BLK) continue;
            float* base = is_a[q] ? As[buf] : Bs[buf];
            if constexpr (ROWMAJOR) {
                // [pixel][column] image, as the operands arrive: no transposition, four conflict-free 16-byte stores (the 16 lanes
                // of a store cover one 256-byte row segment); the 16-column groups of a row are XOR-ed with (pixel >> 2) & 3 so
                // that the four pixel rows a fragment read touches fall into four different bank quarters
                const int cols = is_a[q] ? BMW : BNW;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    *(float4*)&base[(4 * m4[q] + t) * cols + ((((cg[q] >> 2) ^ (m4[q] & 3)) << 4) | ((cg[q] & 3) << 2))] = r[q][t];
                continue;
            }
            const float4 c0 = make_float4(r[q][0].x, r[q][1].x, r[q][2].x, r[q][3].x);
            const float4 c1 = make_float4(r[q][0].y, r[q][1].y, r[q][2].y, r[q][3].y);
            const float4 c2 = make_float4(r[q][0].z, r[q][1].z, r[q][2].z, r[q][3].z);
            const float4 c3 = make_float4(r[q][0].w, r[q][1].w, r[q][2].w, r[q][3].w);
            const int row = 4 * cg[q];
            *(float4*)&base[(row + 0) * BKS + ((m4[q] ^ wswz(row + 0)) << 2)] = c0;
            *(float4*)&base[(row + 1) * BKS + ((m4[q] ^ wswz(row + 1)) << 2)] = c1;
            *(float4*)&base[(row + 2) * BKS + ((m4[q] ^ wswz(row + 2)) << 2)] = c2;
            *(float4*)&base[(row + 3) * BKS + ((m4[q] ^ wswz(row + 3)) << 2)] = c3;
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fg = lane >> 4;
    auto compute = [&](int buf) {
        if constexpr (ROWMAJOR) {
            // the MFMA (s2, t) reduces over the pixels 16 s2 + 4 fg + t (the same sets, in the same order, as the transposed
            // image's float4 columns): a lane reads ONE float per fragment and MFMA, 16 lanes a 64-byte run of one pixel row
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int m = 16 * s2 + 4 * fg + t;
                    float a[TM], b[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) a[i] = As[buf][m * BMW + ((((wm * TM + i) ^ fg) << 4) | fr)];
#pragma unroll
                    for (int j = 0; j < TN; ++j) b[j] = Bs[buf][m * BNW + ((((wn * TN + j) ^ fg) << 4) | fr)];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
                }
            return;
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            float4 av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = (wm * TM + i) * 16 + fr;
                av[i] = *(const float4*)&As[buf][row * BKS + (((s2 * 4 + fg) ^ wswz(row)) << 2)];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = (wn * TN + j) * 16 + fr;
                bv[j] = *(const float4*)&Bs[buf][row * BKS + (((s2 * 4 + fg) ^ wswz(row)) << 2)];
            }
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
        }
    };

    // fused SGD: the filter and momentum tiles are fetched NOW, so their HBM latency hides behind the pixel
    // reduction (read in the epilogue loop they cost one exposed round trip per iteration: the stores of one
    // iteration alias the loads of the next as far as the compiler knows)
    constexpr int W_LD = (BMW * (BNW / 4) + THREADS - 1) / THREADS;
    constexpr bool PREFETCH_W = FUSED_SGD && W_LD <= 8;
    float4 pw[PREFETCH_W ? W_LD : 1], pm[PREFETCH_W ? W_LD : 1];
    if (PREFETCH_W && p.sgd_m) {
#pragma unroll
        for (int it = 0; it < W_LD; ++it) {
            const int e = tid + it * THREADS;
            const int row = e / (BNW / 4), col = (e % (BNW / 4)) * 4;
            const int n = n0 + row, k = k0 + col;
            const bool ok = e < BMW * (BNW / 4) && n < p.N && k < p.K;
            const long long o = (long long)n * p.K + k;
            // streamed once: non-temporal, so the filter / momentum tiles do not evict the x and gy slices that the
            // other workgroups of this XCD re-read from L2
            pw[it] = ok ? __builtin_bit_cast(float4, __builtin_nontemporal_load((const f32x4*)(p.gw + o))) : make_float4(0.f, 0.f, 0.f, 0.f);
            pm[it] = ok ? __builtin_bit_cast(float4, __builtin_nontemporal_load((const f32x4*)(p.sgd_m + o))) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }

    int buf = 0;
    if constexpr (DMA) {
        // A stage = NPA + NPB pieces of 1 KB (RP pixel rows of the gy tile, then of the x tile); wave w requests pieces w, w + 4, ...
        constexpr int NPA = BMW / 8, NPB = BNW / 8, NP = NPA + NPB, PMAX = NP / 4;
        static_assert(NP % 4 == 0, "whole rounds of four pieces");
        constexpr unsigned INV = 0x80000000u;
        const int wave_s = __builtin_amdgcn_readfirstlane(wave);
        unsigned d_vk[PMAX];
        int d_row[PMAX];
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            const int pc = q * 4 + wave_s;
            const bool isA = pc < NPA;                                   // wave-uniform
            const int cols = isA ? BMW : BNW, cp = cols / 4, rp = 256 / cols;
            const int mi = (isA ? pc : pc - NPA) * rp + lane / cp, ch = lane % cp;
            const int col = ((((ch >> 2) ^ ((mi >> 2) & 3)) << 4) | ((ch & 3) << 2));
            const int g = (isA ? n0 : k0) + col;
            d_row[q] = mi;
            d_vk[q] = g < (isA ? p.N : p.K) ? (unsigned)(mi * (isA ? p.N : p.Cin) + g) * 4u : INV;
        }
        const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)smem;
        auto dma_issue = [&](int ms, int S) {
            const unsigned so_a = (unsigned)ms * (unsigned)p.N * 4u, so_b = (unsigned)ms * (unsigned)p.Cin * 4u;
            const unsigned a_dst = lds_base + (unsigned)(S * BMW * BKS * 4), b_dst = lds_base + (unsigned)((2 * BMW + S * BNW) * BKS * 4);
            const bool tail = ms + BKS > mend;                           // uniform: only a split's last stage can be partial
#pragma unroll
            for (int q = 0; q < PMAX; ++q) {
                const int pc = q * 4 + wave_s;
                const bool isA = pc < NPA;
                const unsigned v = tail ? (d_vk[q] | (ms + d_row[q] < mend ? 0u : INV)) : d_vk[q];
                lds_dma16(isA ? a_dst + (unsigned)(pc * 1024) : b_dst + (unsigned)((pc - NPA) * 1024), v, isA ? gr : xr, isA ? so_a : so_b);
            }
        };
        dma_issue(mbeg, 0);
        for (int ms = mbeg; ms < mend; ms += BKS) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my pieces of this stage have landed ...
            __builtin_amdgcn_s_barrier();                          // ... everyone's have; and everyone is done with the other buffer
            if (ms + BKS < mend) dma_issue(ms + BKS, buf ^ 1);
            compute(buf);
            buf ^= 1;
        }
        __syncthreads();                                           // the epilogue reuses the stage buffers
    } else {
    gload(mbeg);
    sstore(0);
    __syncthreads();
    if constexpr (CLK) c_t1 = __builtin_amdgcn_s_memtime();
    for (int ms = mbeg; ms < mend; ms += BKS) {
        const bool more = ms + BKS < mend;
        if constexpr (CLK) {        // diagnostic instantiation only (tools/wgrad_phase.py ABL=..): 1 = no staging after the first stage, 2 = no MFMAs
            if (more && !(p.abl & 1)) gload(ms + BKS);
            if (!(p.abl & 2)) compute(buf);
            if (more && !(p.abl & 1)) sstore(buf ^ 1);
            if (!(p.abl & 4)) __syncthreads();
            buf ^= (p.abl & 1) ? 0 : 1;
            continue;
        }
        if (more) gload(ms + BKS);
        compute(buf);
        if (more) sstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    }
    if constexpr (CLK) c_t2 = __builtin_amdgcn_s_memtime();

    // epilogue through LDS: rows = filters n, columns = taps k (contiguous in gw)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = (wm * TM + i) * 16 + 4 * fg + rr;
            float rsc = 1.f;
            if (p.row_scale) rsc = n0 + row < p.N ? p.row_scale[n0 + row] : 0.f;      // uniform branch
#pragma unroll
            for (int j = 0; j < TN; ++j)
                smem[row * CROW + (wn * TN + j) * 16 + fr] = p.row_scale ? acc[i][j][rr] * rsc : acc[i][j][rr];
        }
    __syncthreads();
    if (PREFETCH_W && p.sgd_m) {
#pragma unroll
        for (int it = 0; it < W_LD; ++it) {
            const int e = tid + it * THREADS;
            const int row = e / (BNW / 4), col = (e % (BNW / 4)) * 4;
            const int n = n0 + row, k = k0 + col;
            if (e >= BMW * (BNW / 4) || n >= p.N || k >= p.K) continue;
            const long long o = (long long)n * p.K + k;
            const float4 g = *(const float4*)&smem[row * CROW + col];
            float4 pv = pw[it], mv = pm[it];      // g' = g + wd*p ; m = mom*m + g' ; p -= lr*m   (same order as sgd_momentum_kernel)
            mv.x = p.mom * mv.x + (g.x + p.wd * pv.x); mv.y = p.mom * mv.y + (g.y + p.wd * pv.y);
            mv.z = p.mom * mv.z + (g.z + p.wd * pv.z); mv.w = p.mom * mv.w + (g.w + p.wd * pv.w);
            pv.x -= p.lr * mv.x; pv.y -= p.lr * mv.y; pv.z -= p.lr * mv.z; pv.w -= p.lr * mv.w;
            __builtin_nontemporal_store(__builtin_bit_cast(f32x4, mv), (f32x4*)(p.sgd_m + o));
            __builtin_nontemporal_store(__builtin_bit_cast(f32x4, pv), (f32x4*)(p.gw + o));
        }
    } else if (p.sgd_m || p.direct) {
        for (int e = tid; e < BMW * (BNW / 4); e += THREADS) {
            const int row = e / (BNW / 4), col = (e % (BNW / 4)) * 4;
            const int n = n0 + row, k = k0 + col;
            if (n >= p.N || k >= p.K) continue;                     // K % 4 == 0
            const long long o = (long long)n * p.K + k;
            float4 g = *(const float4*)&smem[row * CROW + col];
            if (p.sgd_m) {      // g' = g + wd*p ; m = mom*m + g' ; p -= lr*m   (same order as sgd_momentum_kernel)
                float4 pv = *(const float4*)(p.gw + o), mv = *(const float4*)(p.sgd_m + o);
                mv.x = p.mom * mv.x + (g.x + p.wd * pv.x); mv.y = p.mom * mv.y + (g.y + p.wd * pv.y);
                mv.z = p.mom * mv.z + (g.z + p.wd * pv.z); mv.w = p.mom * mv.w + (g.w + p.wd * pv.w);
                pv.x -= p.lr * mv.x; pv.y -= p.lr * mv.y; pv.z -= p.lr * mv.z; pv.w -= p.lr * mv.w;
                *(float4*)(p.sgd_m + o) = mv;
                *(float4*)(p.gw + o) = pv;
            } else {
                *(float4*)(p.gw + o) = g;
            }
        }
    } else if (p.part_ws) {
        // ---- two-pass ordered finish: my partial tile in gw's layout, slot (split, plane); the reduce pass sums the slots in order
        float* dst = p.part_ws + ((long long)by * (p.nbatch > 1 ? p.nbatch : 1) + bz) * ((long long)p.N * p.K);
        for (int e = tid; e < BMW * (BNW / 4); e += THREADS) {
            const int row = e / (BNW / 4), col = (e % (BNW / 4)) * 4;
            const int n = n0 + row, k = k0 + col;
            if (n >= p.N || k >= p.K) continue;                     // K % 4 == 0
            *(float4*)(dst + (long long)n * p.K + k) = *(const float4*)&smem[row * CROW + col];
        }
    } else if (p.ord_ws) {
        // ---- ordered finish: my partial tile to the workspace (sc1: coherent across the XCDs without fences), arrival count,
        // the last workgroup of the tile sums the partials in split order -- four in flight per round -- and writes gw
        constexpr int SC01 = 16;
        const int tile_lin = bz * p.ord_tiles + bx, nsplit = p.ord_splits, my = by;
        const size_t split_stride = (size_t)p.ord_tiles * (p.nbatch > 1 ? p.nbatch : 1) * (BMW * BNW);      // floats between splits
        const __amdgpu_buffer_rsrc_t wsr = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(p.ord_ws + (size_t)tile_lin * (BMW * BNW)), 0, 0x7FFFFFF0, 0x00020000);
        for (int e = tid; e < BMW * (BNW / 4); e += THREADS) {
            const int row = e / (BNW / 4), col = (e % (BNW / 4)) * 4;
            const float4 v = *(const float4*)&smem[row * CROW + col];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), wsr,
                                                   (unsigned)(my * split_stride * sizeof(float)) + (unsigned)(row * BNW + col) * 4u, 0, SC01);
        }
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        __shared__ int ord_last;
        if (tid == 0) {
            const int arrived = __hip_atomic_fetch_add(p.ord_cnt + tile_lin, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = arrived == nsplit - 1;
            if (last) __hip_atomic_store(p.ord_cnt + tile_lin, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch
            ord_last = last;
        }
        __syncthreads();
        if (ord_last) {
            for (int e = tid; e < BMW * (BNW / 4); e += THREADS) {
                const int row = e / (BNW / 4), col = (e % (BNW / 4)) * 4;
                const int n = n0 + row, k = k0 + col;
                if (n >= p.N || k >= p.K) continue;                     // K % 4 == 0
                const long long o = (long long)n * p.K + k;
                const unsigned off = (unsigned)(row * BNW + col) * 4u;
                const float4 mine4 = *(const float4*)&smem[row * CROW + col];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.ord_acc) v = *(const float4*)(p.gw + o);
                for (int s0 = 0; s0 < nsplit; s0 += 8) {               // eight parts in flight (round 5: four -- twice the round trips)
                    float4 u[8];
#pragma unroll
                    for (int sp = 0; sp < 8; ++sp)
                        u[sp] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                            wsr, (s0 + sp < nsplit && s0 + sp != my) ? off + (unsigned)((s0 + sp) * split_stride * sizeof(float)) : 0xFFFFFFF0u, 0, SC01));
#pragma unroll
                    for (int sp = 0; sp < 8; ++sp) {                    // slots >= nsplit were read out of range: zeros
                        const float4 t = s0 + sp == my ? mine4 : u[sp];
                        if (s0 == 0 && sp == 0 && !p.ord_acc) v = t;
                        else { v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
                    }
                }
                *(float4*)(p.gw + o) = v;
            }
        }
    } else {
        for (int e = tid; e < BMW * BNW; e += THREADS) {
            const int row = e / BNW, col = e % BNW;
            const int n = n0 + row, k = k0 + col;
            if (n < p.N && k < p.K) atomicAdd(p.gw + (long long)n * p.K + k, smem[row * CROW + col]);
        }
    }
    if constexpr (CLK) {
        __builtin_amdgcn_s_waitcnt(0);
        if (tid == 0 && p.clk) {
            unsigned long long* o = p.clk + 8 * (blockIdx.y * gridDim.x + blockIdx.x);
            o[0] = c_rt0; o[1] = __builtin_amdgcn_s_memrealtime();
            o[2] = c_t1 - c_t0; o[3] = c_t2 - c_t1; o[4] = __builtin_amdgcn_s_memtime() - c_t2;
            o[5] = __builtin_amdgcn_s_getreg(63492); o[6] = __builtin_amdgcn_s_getreg(63508); o[7] = 1;
        }
    }
}

// second pass of the two-pass ordered filter gradient: gw[plane][i] = (acc ? gw : 0) + part[0][plane][i] + part[1][plane][i] + ...
__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, int splits, int planes, long long nk4, long long bsw, int acc) {
    const long long total = (long long)planes * nk4;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += 256ll * gridDim.x) {
        const long long plane = e / nk4, i = e - plane * nk4;
        float4* o = (float4*)(gw + plane * bsw) + i;
        float4 v = acc ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* src = (const float4*)part + plane * nk4 + i;
        for (int s0 = 0; s0 < splits; s0 += 8) {
            float4 u[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) u[k] = s0 + k < splits ? src[(long long)(s0 + k) * planes * nk4] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (s0 + k < splits) { v.x += u[k].x; v.y += u[k].y; v.z += u[k].z; v.w += u[k].w; }
        }
        *o = v;
    }
}
__global__ void __launch_bounds__(256)
wgrad_reduce_scalar_kernel(const float* __restrict__ part, float* __restrict__ gw, int splits, long long nk, int acc) {
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < nk; e += 256ll * gridDim.x) {
        float v = acc ? gw[e] : 0.f;
        for (int s0 = 0; s0 < splits; s0 += 16) {           // sixteen loads in flight, added in split order
            float u[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) u[k] = s0 + k < splits ? part[(long long)(s0 + k) * nk + e] : 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (s0 + k < splits) v += u[k];
        }
        gw[e] = v;
    }
}
// ---------------------------------------------------------------- fused update of a linear layer (round 7)
// i2v_conv_wgrad_sgd on a linear / pointwise problem (1x1 filter, stride 1, no padding: x is [M][K], gy [M][N], W and its
// momentum [N][K]) of at most 256 rows: the relation head's fc6 (4096 x 50176) and fc7 (4096 x 4096) at M = 128.  The tiled
// fused kernel (conv_wgrad2_f32<4, 2, true>) ran fc6 as 25 088 workgroups of four K-stages each: every one re-fetched its
// 64 KB gy strip and 32 KB x tile, paid its own W / m prefetch and LDS epilogue, and overlapped HBM with MFMA only by chance
// (0.845 ms = 3.9 TB/s of the 3.29 GB it must move).  Here one 8-wave workgroup per CU stays:
//  - it owns 128 filters (16 per wave) and a contiguous range of 64-tap tiles; the workgroups of one tap range are dealt to
//    one XCD (the 32 filter strips of fc6 = the 32 CUs of an XCD), so an x tile comes from HBM once and from that L2 32 times;
//  - its gy^T strip lives in registers for the whole launch (a wave's 16 filters x M rows = M / 4 VGPRs);
//  - per tile: the x tile goes global -> registers -> LDS (double-buffered, loaded one tile ahead), the W / m tiles of tile
//    t + 2 are loaded (16-byte non-temporal buffer loads) while tile t + 1 computes, W' / m' leave as 16-byte non-temporal stores.
// Bit-equal to conv_wgrad2_f32 (any tile form): every output has one accumulator chain of v_mfma_f32_16x16x4_f32 over the
// same four-row sets {32 st + 16 s2 + 4 k + t : k = 0..3}, in the same (st, s2, t) order, A = the gy side, B = the x side,
// zero rows past M on both sides, the same number of 32-row stages, and the same SGD expression.  Only the column a tap takes
// inside a 16x16 block differs (MFMA column c of block j = tap 4 c + j), which no output's arithmetic sees: a lane's four
// accumulators then hold four CONSECUTIVE taps of one filter row, so the epilogue moves float4s without an LDS transpose.
constexpr int FCU_WAVES = 8, FCU_THREADS = 64 * FCU_WAVES, FCU_BN = 16 * FCU_WAVES, FCU_TK = 64;
struct FcuP {
    const float* x; const float* gy; float* w; float* m;
    float lr, mom, wd;
    int M, N, K;
    int strips, chunks, tiles, groups;       // filter strips x tap chunks = groups workgroups with work; tiles = 64-tap tiles of K
    unsigned x_bytes, gy_bytes, w_bytes;     // each < 2 GiB: a masked offset carries the 2 GiB bit (the buffer returns zeros / drops the store)
};

template <int NS>       // NS 32-row stages (ceil(M / 32), as many as the tiled kernel runs): a constant, so that no branch in
__global__ void __launch_bounds__(FCU_THREADS) fc_update_f32(const FcuP p) {     // the loop muddles the compiler's vmcnt accounting
    // the launch is padded to a multiple of 8; XCD g (= blockIdx.x % 8 under round-robin dispatch) takes the contiguous range
    // [g G / 8, (g + 1) G / 8) of the chunk-major work order, as conv_wgrad2_f32's xcd_remap
    const int L = (int)blockIdx.x, g = L & 7, r = L >> 3;
    const int start = (int)(((long long)g * p.groups) >> 3), count = (int)(((long long)(g + 1) * p.groups) >> 3) - start;
    if (r >= count) return;
    const int idx = start + r, chunk = idx / p.strips, strip = idx - chunk * p.strips;
    const int t0 = (int)((long long)chunk * p.tiles / p.chunks), t1 = (int)((long long)(chunk + 1) * p.tiles / p.chunks);

    constexpr unsigned MASK = 0x80000000u, NT = 2;      // NT: the cache-policy bit of a non-temporal buffer access
    constexpr int ROWS = 32 * NS;
    __shared__ __attribute__((aligned(16))) float xs[2][ROWS * FCU_TK];     // x tile, [row][tap]: the fragment reads are conflict-free as it stands
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
    const int n0 = strip * FCU_BN;
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc((void*)p.gy, 0, p.gy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t mr = __builtin_amdgcn_make_buffer_rsrc((void*)p.m, 0, p.w_bytes, 0x00020000);

    // A fragments of the whole reduction: lane (fr, fg) holds gy[32 st + 16 s2 + 4 fg + t][n0 + 16 wave + fr], q = 4 s2 + t
    float a[NS * 8];
    {
        const unsigned na = (unsigned)(n0 + 16 * wave + fr);
        const bool nin = (int)na < p.N;
#pragma unroll
        for (int st = 0; st < NS; ++st)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned row = (unsigned)(32 * st + 16 * (q >> 2) + 4 * fg + (q & 3));
                const unsigned off = ((row * (unsigned)p.N + na) * 4u) | ((nin && (int)row < p.M) ? 0u : MASK);
                a[st * 8 + q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(gr, off, 0, 0));
            }
    }

    // x staging: thread = (rows tid / 16 + 32 q, taps 4 (tid % 16) ..); rows past M and taps past K read as zeros (the B side of
    // a zero row must be 0, not whatever the LDS held: 0 * NaN is NaN)
    float4 xv[NS];
    auto xload = [&](int t) {                            // t >= t1: nothing to stage, the masked loads move no bytes
        const unsigned k = (unsigned)(t * FCU_TK + 4 * (tid & 15));
        const bool kin = t < t1 && (int)k < p.K;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const unsigned row = (unsigned)((tid >> 4) + 32 * q);
            const unsigned off = ((row * (unsigned)p.K + k) * 4u) | ((kin && (int)row < p.M) ? 0u : MASK);
            xv[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
        }
    };
    auto xstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NS; ++q) *(float4*)&xs[buf][((tid >> 4) + 32 * q) * FCU_TK + 4 * (tid & 15)] = xv[q];
    };
    // W / m of a tile: lane (fr, fg), q = 0..3 -> filter n0 + 16 wave + 4 fg + q, taps t * 64 + 4 fr ..  (K % 4 == 0)
    auto wm_offsets = [&](int t, unsigned (&off)[4]) {
        const unsigned k = (unsigned)(t * FCU_TK + 4 * fr);
        const bool kin = t < t1 && (int)k < p.K;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned n = (unsigned)(n0 + 16 * wave + 4 * fg + q);
            off[q] = ((n * (unsigned)p.K + k) * 4u) | ((kin && (int)n < p.N) ? 0u : MASK);
        }
    };
    auto wm_load = [&](int t, float4 (&wv)[4], float4 (&mv)[4]) {
        unsigned off[4];
        wm_offsets(t, off);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            wv[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, off[q], 0, NT));
            mv[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(mr, off[q], 0, NT));
        }
    };

    int buf = 0;
    auto body = [&](int t, float4 (&wv)[4], float4 (&mv)[4]) {
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            float4 b[8];                                 // B fragments of a stage: a ds_read_b128 per lane feeds four MFMAs
#pragma unroll
            for (int q = 0; q < 8; ++q) b[q] = *(const float4*)&xs[buf][(32 * st + 16 * (q >> 2) + 4 * fg + (q & 3)) * FCU_TK + 4 * fr];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st * 8 + q], b[q].x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st * 8 + q], b[q].y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st * 8 + q], b[q].z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st * 8 + q], b[q].w, acc[3], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);               // the update's arithmetic stays behind the MFMAs: hoisted, it waits for W / m there
        unsigned off[4];
        wm_offsets(t, off);
#pragma unroll
        for (int q = 0; q < 4; ++q) {                    // g' = g + wd*p ; m = mom*m + g' ; p -= lr*m   (same order as sgd_momentum_kernel)
            float4 pv = wv[q], m4 = mv[q];
            m4.x = p.mom * m4.x + (acc[0][q] + p.wd * pv.x); m4.y = p.mom * m4.y + (acc[1][q] + p.wd * pv.y);
            m4.z = p.mom * m4.z + (acc[2][q] + p.wd * pv.z); m4.w = p.mom * m4.w + (acc[3][q] + p.wd * pv.w);
            pv.x -= p.lr * m4.x; pv.y -= p.lr * m4.y; pv.z -= p.lr * m4.z; pv.w -= p.lr * m4.w;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, m4), mr, off[q], 0, NT);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pv), wr, off[q], 0, NT);
        }
        xstore(buf ^ 1);                                 // x of tile t + 1, loaded a tile ago (the other buffer is free since the last barrier)
        xload(t + 2);
        wm_load(t + 2, wv, mv);                          // the registers just consumed, two tiles ahead
        __syncthreads();
        buf ^= 1;
    };

    float4 wA[4], mA[4], wB[4], mB[4];
    xload(t0);
    // the A fragments and the first x tile: the one drain of the launch.  Without it the compiler, unsure across the loop's back
    // edge how many loads are younger than the A fragments, waits with vmcnt(0) in front of every tile's first MFMA
    __builtin_amdgcn_s_waitcnt(0);
    xstore(0);
    xload(t0 + 1);
    wm_load(t0, wA, mA);
    wm_load(t0 + 1, wB, mB);
    __syncthreads();
    // unrolled by two: each register set is reloaded in place, never copied.  Both ways back to the top pass through both
    // bodies (an odd last tile leaves the loop), so the compiler counts the same loads in flight on each
    for (int t = t0;; t += 2) {
        body(t, wA, mA);
        if (t + 1 >= t1) break;
        body(t + 1, wB, mB);
        if (t + 2 >= t1) break;
    }
}
}  // namespace

// the persistent fused update (fc_update_f32), for the shapes plan_wgrad gives WG_FC_UPDATE
static void launch_fc_update(const WgP& p, hipStream_t st) {
    const long long xb = (long long)p.M * p.K * 4, gb = (long long)p.M * p.N * 4, wb = (long long)p.N * p.K * 4;
    FcuP q = {};
    q.x = p.x; q.gy = p.gy; q.w = p.gw; q.m = p.sgd_m; q.lr = p.lr; q.mom = p.mom; q.wd = p.wd;
    q.M = p.M; q.N = p.N; q.K = p.K;
    q.strips = i2v_cdiv(p.N, FCU_BN);
    q.tiles = i2v_cdiv(p.K, FCU_TK);
    q.chunks = std::min(std::max(NUM_CU / q.strips, 1), q.tiles);      // one workgroup per CU
    q.groups = q.strips * q.chunks;
    q.x_bytes = (unsigned)xb; q.gy_bytes = (unsigned)gb; q.w_bytes = (unsigned)wb;
    const unsigned grid = (unsigned)((q.groups + 7) / 8 * 8);
    switch (i2v_cdiv(p.M, 32)) {
    case 1: fc_update_f32<1><<<grid, FCU_THREADS, 0, st>>>(q); break;
    case 2: fc_update_f32<2><<<grid, FCU_THREADS, 0, st>>>(q); break;
    case 3: fc_update_f32<3><<<grid, FCU_THREADS, 0, st>>>(q); break;
    case 4: fc_update_f32<4><<<grid, FCU_THREADS, 0, st>>>(q); break;
    case 5: fc_update_f32<5><<<grid, FCU_THREADS, 0, st>>>(q); break;
    case 6: fc_update_f32<6><<<grid, FCU_THREADS, 0, st>>>(q); break;
    case 7: fc_update_f32<7><<<grid, FCU_THREADS, 0, st>>>(q); break;
    default: fc_update_f32<8><<<grid, FCU_THREADS, 0, st>>>(q); break;
    }
}

static ConvShape shape_of(const WgP& p) {
    return {p.B, p.H, p.W, p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.pad, 1, p.Ho, p.Wo, p.nbatch, 0};
}

// plan one filter-gradient problem (conv_plan.h); ext_part: p.part_ws is the caller's own slab of p.part_cap parts
static WgradPlan plan_of(const WgP& p, float beta, bool fused, void* split_ws, size_t split_ws_bytes) {
    return plan_wgrad(shape_of(p), beta != 0.f, fused, p.row_scale != nullptr, p.part_ws ? p.part_cap : -1, g_i2v_tuning,
                      g_clk != nullptr, split_ws ? split_ws_bytes : 0);
}

// bind the workspace and clear, launch the planned kernel, then the reduce pass if the plan has one
static void launch_wgrad(WgP& p, const WgradPlan& pl, float beta, hipStream_t st, void* split_ws = nullptr) {
    if (pl.kernel == WG_FC_UPDATE) return launch_fc_update(p, st);
    const int planes = p.nbatch > 1 ? p.nbatch : 1;
    p.m_per_split = pl.m_per_split;
    p.direct = pl.direct;
    p.x_bytes = pl.x_bytes;
    p.gy_bytes = pl.gy_bytes;
    if (pl.finish == WFIN_ORDERED_TILES) {
        p.ord_cnt = reinterpret_cast<int*>(split_ws);
        p.ord_ws = reinterpret_cast<float*>(static_cast<char*>(split_ws) + kSplitCounterBytes);
        p.ord_splits = pl.splits; p.ord_tiles = pl.tiles; p.ord_acc = beta != 0.f;
    } else if (pl.finish == WFIN_ORDERED_PARTS) {
        p.part_ws = reinterpret_cast<float*>(static_cast<char*>(split_ws) + kSplitCounterBytes);      // the counters in front stay zero
    } else if (pl.finish != WFIN_EXTERNAL_PARTS) {
        p.part_ws = nullptr;                          // a caller's slab of one part: written straight to gw (its slot 0)
    }
    if (pl.ordered_fallback) ++g_ordered_fallbacks;
    if (pl.clear_bytes) hipMemsetAsync(p.gw, 0, pl.clear_bytes, st);
    p.xcd_remap = pl.xcd_remap;
    if (pl.xcd_remap) { p.r_tiles = pl.tiles; p.r_splits = pl.splits; p.r_total = pl.tiles * pl.splits * planes; }
    const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]);
    switch (pl.kernel) {
    case WG_V1_64x64: conv_wgrad_f32<64, 64><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_DMA_128x128: conv_wgrad2_f32<4, 4, false, false, true><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_DMA_128x64: conv_wgrad2_f32<4, 2, false, false, true><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_DMA_64x64: conv_wgrad2_f32<2, 2, false, false, true><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_FUSED_128x64: conv_wgrad2_f32<4, 2, true><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_128x128: conv_wgrad2_f32<4, 4><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_128x64: conv_wgrad2_f32<4, 2><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_FUSED_64x64: conv_wgrad2_f32<2, 2, true><<<grid, THREADS, 0, st>>>(p); break;
    case WG_V2_CLK_64x64: p.clk = g_clk; p.abl = g_ablate; conv_wgrad2_f32<2, 2, false, true><<<grid, THREADS, 0, st>>>(p); break;
    default: conv_wgrad2_f32<2, 2><<<grid, THREADS, 0, st>>>(p); break;
    }
    const long long nk = (long long)p.N * p.K;
    if (pl.reduce_pass == PASS_VEC4) {
        const long long total = (long long)planes * (nk / 4);
        wgrad_reduce_kernel<<<(unsigned)std::min<long long>(i2v_cdiv(total, 256), 2048), 256, 0, st>>>(
            p.part_ws, p.gw, pl.splits, planes, nk / 4, planes > 1 ? p.bsw : nk, beta != 0.f);
    } else if (pl.reduce_pass == PASS_SCALAR) {
        wgrad_reduce_scalar_kernel<<<(unsigned)std::min<long long>(i2v_cdiv(nk, 256), 2048), 256, 0, st>>>(p.part_ws, p.gw, pl.splits, nk, beta != 0.f);
    }
}

// The filter-gradient plan as numbers: i2v_conv_wgrad / _scaled (fused = 0), i2v_conv_wgrad_sgd (fused = 1), or, with
// nbatch > 1, the plane batch of i2v_gemm_tn_batched (B = H = 1, W = M, Cin = K, Cout = N, 1x1).
extern "C" int32_t i2v_conv_wgrad_plan(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                                       int32_t stride, int32_t pad, int32_t nbatch, int32_t beta_nonzero, int32_t fused,
                                       int32_t has_row_scale, int32_t ext_part_cap, size_t ws_bytes, int32_t* out, int32_t n_out) {
    I2V_CHECK_ARG(out && n_out >= I2V_WGRAD_PLAN_FIELDS, "conv_wgrad_plan: out needs room for I2V_WGRAD_PLAN_FIELDS values");
    int dummy = 0;
    const int rc = check_conv("conv_wgrad_plan", &dummy, &dummy, &dummy, B, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    const ConvShape s = {B, H, W, Cin, Cout, KH, KW, stride, pad, pad, 1, (H + 2 * pad - KH) / stride + 1, (W + 2 * pad - KW) / stride + 1,
                         nbatch, 0};
    const WgradPlan pl = plan_wgrad(s, beta_nonzero != 0, fused != 0, has_row_scale != 0, ext_part_cap, g_i2v_tuning, g_clk != nullptr, ws_bytes);
    const int32_t v[I2V_WGRAD_PLAN_FIELDS] = {pl.status, pl.v2, pl.kernel, pl.tm, pl.tk, pl.splits, pl.m_per_split, pl.finish, pl.direct,
                                              pl.xcd_remap, (int32_t)pl.grid[0], (int32_t)pl.grid[1], (int32_t)pl.grid[2], pl.dma,
                                              clamp32(pl.clear_bytes), pl.reduce_pass, pl.ordered_fallback};
    std::copy(v, v + I2V_WGRAD_PLAN_FIELDS, out);
    return I2V_OK;
}

extern "C" size_t i2v_conv_wgrad_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                                 int32_t KH, int32_t KW, int32_t stride, int32_t pad) {
    (void)B; (void)H; (void)W; (void)stride; (void)pad;
    (void)Cin; (void)Cout; (void)KH; (void)KW;
    return 256;   // reserved (the split-m reduction uses atomics directly into gw)
}

static int conv_wgrad_impl(const float* x, const float* gy, float* gw, const float* row_scale, int32_t B, int32_t H,
                           int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                           float beta, void* stream, void* split_ws = nullptr, size_t split_ws_bytes = 0) {
    int rc = check_conv("conv_wgrad", x, gy, gw, B, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    WgP p = {};
    p.x = x; p.gy = gy; p.gw = gw; p.row_scale = row_scale;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
    p.Ho = (H + 2 * pad - KH) / stride + 1;
    p.Wo = (W + 2 * pad - KW) / stride + 1;
    p.M = B * p.Ho * p.Wo; p.N = Cout; p.K = KH * KW * Cin;
    p.lgCin = ilog2_exact(Cin);
    I2V_CHECK_ARG(beta == 0.f || beta == 1.f, "conv_wgrad: beta must be 0 or 1");
    const WgradPlan pl = plan_of(p, beta, false, split_ws, split_ws_bytes);
    if (pl.status != PLAN_OK) return plan_error(pl.status, shape_of(p));
    launch_wgrad(p, pl, beta, st, split_ws);
    I2V_CHECK_LAUNCH("conv_wgrad");
    return I2V_OK;
}

// gw[z] (N x K) = gy[z]^T (M x N) . x[z] (M x K) for z < nbatch: the element-wise planes of a Winograd filter gradient
// (csrc/winograd.hip).  gw is overwritten; the batches of gw must be contiguous when the reduction is split (one clear).
// beta is an explicit argument of the shared implementation (round-3 advice: the accumulating entry point used to pass it
// through a thread_local global, where an early return could have left it at 1).
static int32_t gemm_tn_batched_impl(const float* x, const float* gy, float* gw, int32_t M, int32_t N, int32_t K, int32_t nbatch,
                                    long long stride_x, long long stride_gy, long long stride_gw, float beta, void* stream,
                                    int part_cap = 0, int* part_splits = nullptr) {
    I2V_CHECK_ARG(x && gy && gw && M > 0 && N > 0 && K > 0 && nbatch > 0, "gemm_tn_batched: bad argument");
    I2V_CHECK_ARG(N % 4 == 0 && K % 4 == 0, "gemm_tn_batched: N and K must be multiples of 4");
    I2V_CHECK_ARG(nbatch == 1 || stride_gw == (long long)N * K, "gemm_tn_batched: gw batches must be contiguous");
    WgP p = {};
    p.x = x; p.gy = gy; p.gw = gw;
    p.B = 1; p.H = 1; p.W = M; p.Cin = K; p.Cout = N; p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0;
    p.Ho = 1; p.Wo = M;
    p.M = M; p.N = N; p.K = K;
    p.lgCin = ilog2_exact(K);
    p.nbatch = nbatch; p.bsx = stride_x; p.bsg = stride_gy; p.bsw = stride_gw;
    if (part_splits) {          // i2v_internal_gemm_tn_batched_parts: gw = a slab of part_cap slots of nbatch x (N x K); slot s = split s
        p.part_ws = gw; p.part_cap = part_cap;
    }
    const WgradPlan pl = plan_of(p, beta, false, nullptr, 0);
    if (!pl.v2) {               // N % 4 == 0 was checked: the first-generation kernel is selected, or an operand reaches 2 GiB
        i2v_set_error("gemm_tn_batched: operand larger than 2 GiB per batch");
        return I2V_ERR_UNSUPPORTED;
    }
    launch_wgrad(p, pl, beta, (hipStream_t)stream);
    if (part_splits) *part_splits = pl.splits;      // what the caller's reduce pass must sum (1: the result itself)
    I2V_CHECK_LAUNCH("gemm_tn_batched");
    return I2V_OK;
}

// (csrc/winograd.hip) parts[0] = parts[0] + parts[1] + ... in part order, all planes in parallel (in place: an element is read and
// written by one thread)
int32_t i2v_internal_reduce_parts(float* parts, int nparts, int planes, long long nk, void* stream) {
    const long long total = (long long)planes * (nk / 4);
    wgrad_reduce_kernel<<<(unsigned)std::min<long long>(i2v_cdiv(total, 256), 4096), 256, 0, (hipStream_t)stream>>>(
        parts, parts, nparts, planes, nk / 4, nk, 0);
    return I2V_OK;
}

// (csrc/elementwise.hip) the scalar reduce pass on a grid of the caller's choosing
void i2v_internal_reduce_scalar(const float* part, float* out, int nparts, long long n, int acc, unsigned blocks, void* stream) {
    wgrad_reduce_scalar_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(part, out, nparts, n, acc);
}

// (csrc/winograd.hip) the same GEMMs with the split parts left SIDE BY SIDE in ``parts`` ([split][plane][N x K], room for
// ``cap`` splits) for the caller's own ordered sum; *splits = how many were written (1: the result itself)
int32_t i2v_internal_gemm_tn_batched_parts(const float* x, const float* gy, float* parts, int32_t M, int32_t N, int32_t K,
                                           int32_t nbatch, long long stride_x, long long stride_gy, int cap, int* splits, void* stream) {
    return gemm_tn_batched_impl(x, gy, parts, M, N, K, nbatch, stride_x, stride_gy, (long long)N * K, 0.f, stream, cap, splits);
}

extern "C" int32_t i2v_gemm_tn_batched(const float* x, const float* gy, float* gw, int32_t M, int32_t N, int32_t K,
                                       int32_t nbatch, long long stride_x, long long stride_gy, long long stride_gw,
                                       void* stream) {
    return gemm_tn_batched_impl(x, gy, gw, M, N, K, nbatch, stride_x, stride_gy, stride_gw, 0.f, stream);
}

// The same accumulating into gw (gw += sum; the caller has cleared or pre-loaded it): no memset node in front.
extern "C" int32_t i2v_gemm_tn_batched_acc(const float* x, const float* gy, float* gw, int32_t M, int32_t N, int32_t K,
                                           int32_t nbatch, long long stride_x, long long stride_gy, long long stride_gw,
                                           void* stream) {
    return gemm_tn_batched_impl(x, gy, gw, M, N, K, nbatch, stride_x, stride_gy, stride_gw, 1.f, stream);
}

extern "C" int32_t i2v_conv_wgrad(const float* x, const float* gy, float* gw, int32_t B, int32_t H, int32_t W,
                                  int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                                  float beta, void* ws, size_t ws_bytes, void* stream) {
    // ws: the caller's split workspace (i2v_conv_fwd's: zeroed counters + slab; NULL: splits are summed with fp32 atomics)
    return conv_wgrad_impl(x, gy, gw, nullptr, B, H, W, Cin, Cout, KH, KW, stride, pad, beta, stream, ws, ws_bytes);
}

extern "C" int32_t i2v_conv_wgrad_scaled(const float* x, const float* gy, const float* row_scale, float* gw, int32_t B,
                                         int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW,
                                         int32_t stride, int32_t pad, float beta, void* ws, size_t ws_bytes, void* stream) {
    // ws: as i2v_conv_wgrad's (round 6: the trained bottlenecks' 1x1 filter gradients are ordered through it too)
    return conv_wgrad_impl(x, gy, gw, row_scale, B, H, W, Cin, Cout, KH, KW, stride, pad, beta, stream, ws, ws_bytes);
}

// wgrad with the SGD(momentum) update of that filter fused into the accumulator epilogue: the gradient
// never goes to HBM (for vrd.fc6 that is 822 MB written + 822 MB read back per step).  Only when the whole
// reduction over the pixels fits one workgroup pass (no split over m), i.e. the skinny relation-head GEMMs.
extern "C" int32_t i2v_conv_wgrad_sgd(const float* x, const float* gy, float* w, float* m, int32_t B, int32_t H,
                                      int32_t W, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                                      int32_t pad, float lr, float momentum, float weight_decay, void* stream) {
    int rc = check_conv("conv_wgrad_sgd", x, gy, w, B, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    I2V_CHECK_ARG(m, "conv_wgrad_sgd: null momentum buffer");
    WgP p = {};
    p.x = x; p.gy = gy; p.gw = w; p.sgd_m = m; p.lr = lr; p.mom = momentum; p.wd = weight_decay;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
    p.Ho = (H + 2 * pad - KH) / stride + 1;
    p.Wo = (W + 2 * pad - KW) / stride + 1;
    p.M = B * p.Ho * p.Wo; p.N = Cout; p.K = KH * KW * Cin;
    p.lgCin = ilog2_exact(Cin);
    const WgradPlan pl = plan_of(p, 0.f, true, nullptr, 0);      // the persistent update, or a shape it does not cover on the tiled kernel
    if (pl.status != PLAN_OK) return plan_error(pl.status, shape_of(p));
    launch_wgrad(p, pl, 0.f, (hipStream_t)stream);
    I2V_CHECK_LAUNCH("conv_wgrad_sgd");
    return I2V_OK;
}
