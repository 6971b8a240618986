// Greedy NMS on the device: a bitmask kernel over 64x64 tiles of the upper triangle, then a suppression scan that runs in a
// single workgroup per image (no host round trip), in one of three forms; which one is plan_nms's decision (roi_plan.h).
// Replaces nms/nms_cpu.py:6-34.
//
// Box arithmetic is fp32 with one rounding per operation (built with
// -ffp-contract=off) so IoU threshold decisions match the reference's CPU path bit
// for bit on the same boxes.
#include "nms.h"
#include "roi_plan.h"
#include <algorithm>

namespace {
using namespace roiplan;

// ------------------------------------------------------------------ NMS
// (1) mask kernel: 64x64 tiles of the upper triangle; one wave per tile, lane = row.
//     nms_cpu.py:13,20-29: areas with +1, IoU = inter / (area_i + area_j - inter); a column suppresses when !(IoU <= thresh).
//
// The kernel is VALU-bound (72 M pairs at N = 12000: the loop was 40 instructions per pair, 11 of them the IEEE division, 4
// canonicalising moves in front of fmaxf / fminf, 6 for a variable 64-bit shift).  Round 5: the 64 columns are a compile-time
// loop (bit positions are constants), max / min are the hardware instructions, and the division is replaced by an EXACT test
// that needs it only inside a band of 2^-21 around the threshold:
//     ovr_f = fl(inter / d), d = fl(fl(area_i + area_j) - inter) > 0; rounding is monotone, so inter/d <= thresh implies
//     ovr_f <= thresh, and inter/d >= thresh (1 + 2^-22) implies ovr_f > thresh.  With thi = fl(thresh (1 + 2^-21)),
//     tlo = fl(thresh (1 - 2^-21)) (the 2^-21 absorbs the two roundings of each product):
//     inter < fl(tlo d)  =>  inter < thresh d  =>  not suppressed;
//     inter > fl(thi d)  =>  inter > thresh d (1 + 2^-22)  =>  suppressed;
//     otherwise (or a box with a non-positive side, or a NaN): the division, as before, after the loop.
//     The keep lists stay bit-exact against nms_cpu (golden vectors: 36 cases, uniform and clustered).
__device__ inline float hw_max(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ inline float hw_min(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// NMS_MASK_WAVES (row blocks per workgroup), SCAN_THREADS, SCAN_PIPE_WORDS, SUPER_ROWS, SUPER_WORDS, NMS_SWEEPS: roi_plan.h

__global__ void __launch_bounds__(64 * NMS_MASK_WAVES)
nms_mask_kernel(const float* __restrict__ dets, int n, int nblk, float thresh,
                unsigned long long* __restrict__ mask) {
    const int cb = blockIdx.x, img = blockIdx.z;
    const int lane = threadIdx.x & 63, rb = blockIdx.y * NMS_MASK_WAVES + (threadIdx.x >> 6);
    if (cb < (int)blockIdx.y * NMS_MASK_WAVES) return;            // the whole group lies below the diagonal (uniform)
    __shared__ __attribute__((aligned(16))) float sc[5][64];      // column boxes, one field per row: x1, y1, x2, y2, area
    const float* D = dets + (long long)img * n * 5;
    const int ccount = min(64, n - cb * 64);
    __shared__ unsigned long long s_cbad;                         // columns whose box has a non-positive side (or a NaN): decided by the division
    if (threadIdx.x < 64) {
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
        if (lane < ccount) {
            const float* p = D + ((long long)cb * 64 + lane) * 5;
            c0 = p[0]; c1 = p[1]; c2 = p[2]; c3 = p[3];
        }
        const float cw = c2 - c0 + 1.0f, ch = c3 - c1 + 1.0f;
        sc[0][lane] = c0; sc[1][lane] = c1; sc[2][lane] = c2; sc[3][lane] = c3;
        sc[4][lane] = cw * ch;
        const unsigned long long bad = __ballot(!(cw > 0.f && ch > 0.f));
        if (lane == 0) s_cbad = bad;
    }
    __syncthreads();
    const int row = rb * 64 + lane;
    if (cb < rb || rb >= nblk || row >= n) return;
    const float* p = D + (long long)row * 5;
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const float rw = x2 - x1 + 1.0f, rh = y2 - y1 + 1.0f;
    const float area = rw * rh;
    // For boxes with positive sides d = fl(fl(area_i + area_j) - inter) > 0 always (inter <= min of the two areas: the clipped
    // extents are not larger than either box's, and rounding is monotone), so the loop need not test it; a row or a column
    // with a non-positive side or a NaN goes to the division as a whole.
    const float thi = thresh * 1.000000476837158203125f, tlo = thresh * 0.999999523162841796875f;     // thresh (1 +- 2^-21)
    unsigned w[2] = {0u, 0u}, unc[2] = {0u, 0u};          // suppression bits; pairs the band test could not decide
#pragma unroll
    for (int j4 = 0; j4 < 64; j4 += 4) {
        const float4 X1 = *(const float4*)&sc[0][j4], Y1 = *(const float4*)&sc[1][j4], X2 = *(const float4*)&sc[2][j4],
                     Y2 = *(const float4*)&sc[3][j4], AR = *(const float4*)&sc[4][j4];
        const float cx1[4] = {X1.x, X1.y, X1.z, X1.w}, cy1[4] = {Y1.x, Y1.y, Y1.z, Y1.w}, cx2[4] = {X2.x, X2.y, X2.z, X2.w},
                    cy2[4] = {Y2.x, Y2.y, Y2.z, Y2.w}, car[4] = {AR.x, AR.y, AR.z, AR.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j4 + u;
            const unsigned bit = 1u << (j & 31);
            const float xx1 = hw_max(x1, cx1[u]), yy1 = hw_max(y1, cy1[u]);
            const float xx2 = hw_min(x2, cx2[u]), yy2 = hw_min(y2, cy2[u]);
            const float ww = hw_max(0.0f, xx2 - xx1 + 1.0f), hh = hw_max(0.0f, yy2 - yy1 + 1.0f);
            const float inter = ww * hh;
            const float d = area + car[u] - inter;
            // two compares, two selects; nothing in this loop branches
            const int over = inter > thi * d, under = inter < tlo * d;
            w[j >> 5] |= over ? bit : 0u;
            unc[j >> 5] |= (over | under) ? 0u : bit;
        }
    }
    {
        const unsigned long long bad = !(rw > 0.f && rh > 0.f) ? ~0ull : s_cbad;
        unc[0] |= (unsigned)bad; unc[1] |= (unsigned)(bad >> 32);
    }
    // the undecided pairs (inter within 2^-21 of thresh * d, or d <= 0 / NaN): the reference's own expression
    for (int h = 0; h < 2; ++h) {
        unsigned m = unc[h];
        while (m) {
            const int jj = __builtin_ctz(m), j = 32 * h + jj;
            m &= m - 1;
            const float xx1 = fmaxf(x1, sc[0][j]), yy1 = fmaxf(y1, sc[1][j]);
            const float xx2 = fminf(x2, sc[2][j]), yy2 = fminf(y2, sc[3][j]);
            const float ww = fmaxf(0.0f, xx2 - xx1 + 1.0f), hh = fmaxf(0.0f, yy2 - yy1 + 1.0f);
            const float inter = ww * hh;
            const float ovr = inter / (area + sc[4][j] - inter);
            if (!(ovr <= thresh)) w[h] |= 1u << jj;         // nms_cpu.py:31 keeps ovr <= thresh
            else w[h] &= ~(1u << jj);
        }
    }
    unsigned long long bits = ((unsigned long long)w[1] << 32) | w[0];
    if (cb == rb) bits &= lane == 63 ? 0ull : (~0ull << (lane + 1));      // the diagonal tile: columns after the row
    if (ccount < 64) bits &= (1ull << ccount) - 1ull;                                     // columns past the end
    mask[((long long)img * n + row) * nblk + cb] = bits;
}

// (2) scan kernel: one 1024-thread workgroup per image walks the 64-row blocks in score
//     order.  Wave 0 resolves the block's diagonal word serially (64 readlane steps);
//     all 16 waves then OR the mask rows of the rows just kept into the LDS "removed"
//     bitmap.  Stops after max_keep kept rows.  Replaces the host scan of
//     nms_cuda_kernel.cu:132-144 and the Python while-loop of nms_cpu.py:18-32.
//     SCAN_MAX_BLK (nms.h) blocks at the most.
__global__ void __launch_bounds__(SCAN_THREADS)
nms_scan_kernel(const unsigned long long* __restrict__ mask, int n, int nblk, int max_keep,
                int* __restrict__ keep_out, int* __restrict__ num_out) {
    __shared__ unsigned long long removed[SCAN_MAX_BLK];
    __shared__ unsigned long long s_kept;
    __shared__ int s_count;
    const int img = blockIdx.x;
    const unsigned long long* M = mask + (long long)img * n * nblk;
    int* keep = keep_out + (long long)img * n;
    for (int i = threadIdx.x; i < nblk; i += SCAN_THREADS) removed[i] = 0;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int limit = max_keep > 0 ? max_keep : n;
    for (int rb = 0; rb < nblk; ++rb) {
        if (wave == 0) {
            const int row = rb * 64 + lane;
            unsigned long long diag = (row < n) ? M[(long long)row * nblk + rb] : 0ull;
            unsigned long long cur = removed[rb];
            const int valid = min(64, n - rb * 64);
            if (valid < 64) cur |= ~0ull << valid;
            unsigned long long kept = 0;
            int count = s_count;
            for (int i = 0; i < valid && count < limit; ++i) {
                unsigned long long d = __shfl(diag, i);
                if (!((cur >> i) & 1ull)) { kept |= 1ull << i; cur |= d; ++count; }
            }
            if ((kept >> lane) & 1ull) {
                int pos = s_count + __popcll(kept & ((1ull << lane) - 1ull));
                keep[pos] = row;
            }
            if (lane == 0) { s_kept = kept; s_count = count; }
        }
        __syncthreads();
        const unsigned long long kept = s_kept;
        const int count = s_count;
        if (count >= limit) break;
        // OR the kept rows' masks into the columns to the right of the diagonal
        for (int i = wave; i < 64; i += SCAN_THREADS / 64) {
            if (!((kept >> i) & 1ull)) continue;
            const unsigned long long* mr = M + (long long)(rb * 64 + i) * nblk;
            for (int j = rb + 1 + lane; j < nblk; j += 64) {
                unsigned long long v = mr[j];
                if (v) atomicOr(&removed[j], v);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) num_out[img] = s_count;
}

// Round 5 built and measured a form with the ROLES SPLIT (wave 0 only resolves and carries the next three verdict words of the
// rows it keeps in scalar registers; the other 15 waves fetch the KEPT rows' words only and fold them two blocks later; one
// barrier per block, then none: LDS counters polled both ways): bit-exact on every golden case and SLOWER -- 264 us with one
// barrier, 370-420 us polling, against 186 us for the form below (N = 12000 clustered; DESIGN.md 5.10 has the stamps).  Neither
// the barrier count nor a drained prefetch (LDS-only barriers: 185 us) is what a block's ~2k cycles are made of.
// Pipelined variant for n <= 12352 (every RPN case): the mask rows of block rb+1 are fetched into
// registers (4 rows per wave x 3 words per lane) while block rb is being resolved and folded in, so
// global-load latency is off the serial chain; the chain per 64-row block is the 64-step resolve in
// wave 0 plus two workgroup barriers.

// a value every lane holds alike (read from LDS: the compiler must assume otherwise), moved to scalar registers
__device__ inline unsigned long long uniform64(unsigned long long v) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
}

__global__ void __launch_bounds__(SCAN_THREADS)
nms_scan_pipelined_kernel(const unsigned long long* __restrict__ mask, int n, int nblk, int max_keep,
                          int* __restrict__ keep_out, int* __restrict__ num_out) {
    __shared__ unsigned long long removed[64 * SCAN_PIPE_WORDS + 1];
    __shared__ unsigned long long s_kept;
    __shared__ int s_count;
    const int img = blockIdx.x;
    const unsigned long long* M = mask + (long long)img * n * nblk;
    int* keep = keep_out + (long long)img * n;
    for (int i = threadIdx.x; i < nblk; i += SCAN_THREADS) removed[i] = 0;
    if (threadIdx.x == 0) s_count = 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int limit = max_keep > 0 ? max_keep : n;
    unsigned long long pc[4][SCAN_PIPE_WORDS], pn[4][SCAN_PIPE_WORDS], dc = 0, dn = 0;
    // A row that is already suppressed when its block is fetched can never be kept, so its mask words are never used: they
    // are not fetched.  ``removed[rb]`` holds, at that point, the verdict of every block but the one being resolved; with
    // clustered proposals (12000 -> 2000 kept) most rows are gone by then, and the scan workgroup's ingest -- one CU pulling
    // 96 KB per block, 18 MB per image, was ~40 % of its time -- shrinks with them.  (Uniform per wave: a row is a wave's.)
    // The fetch itself must be cheap: 16 waves issue 13 loads each per block, and written as ``live ? M[row * nblk + j] : 0`` every
    // load carried a 64-bit multiply-add, a bounds compare and a branch of its own -- ~400 instructions per wave and block, four
    // waves per SIMD: the chain per block (2.4k cycles) was instruction ISSUE, not the resolve, the barriers or memory latency
    // (a deeper prefetch and a one-barrier form both measured slower: they added instructions).  Now: one buffer descriptor over
    // the image's mask (the launcher keeps it below 2 GiB), byte offsets carried from block to block (+ (64 nblk + 1) * 8), the
    // three words of a row through the instruction's immediate offset, a word past the end of its row = the 2 GiB bit (zeros, no traffic;
    // rows past n fall off the descriptor by themselves).
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc((void*)M, 0, (unsigned)((long long)n * nblk * 8), 0x00020000);
    const unsigned ostep = (unsigned)(64 * nblk + 1) * 8u;
    unsigned noff[4], ndiag = (unsigned)(lane * nblk) * 8u;          // offsets of the NEXT block to fetch
#pragma unroll
    for (int r = 0; r < 4; ++r) noff[r] = (unsigned)((wave * 4 + r) * nblk + 1 + lane) * 8u;
    auto fetch = [&](int rb, unsigned long long (&P)[4][SCAN_PIPE_WORDS], unsigned long long& diag) {
        const unsigned long long gone = removed[rb];
        const int wgone = __builtin_amdgcn_readfirstlane((int)((gone >> (wave * 4)) & 15ull));      // my four rows' verdicts: scalar
        unsigned past[SCAN_PIPE_WORDS];                                   // a word past the end of its row
#pragma unroll
        for (int c = 0; c < SCAN_PIPE_WORDS; ++c) past[c] = (rb + 1 + lane + 64 * c < nblk) ? 0u : 0x80000000u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int c = 0; c < SCAN_PIPE_WORDS; ++c) {
                P[r][c] = 0ull;
                // a dead row or a column group past the end of the rows issues NO instruction (scalar branches): one CU's
                // memory pipe takes these 16 x 13 wave-loads per block one after the other -- issued unconditionally, with
                // the 2 GiB bit on the dead ones, the scan took 410 us instead of 280
                if (!((wgone >> r) & 1) && rb + 1 + 64 * c < nblk)
                    P[r][c] = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(mrs, (noff[r] | past[c]) + 512u * c, 0, 0));
            }
            noff[r] += ostep;
        }
        if (wave == 0) {
            const unsigned dead = ((gone >> lane) & 1ull) ? 0x80000000u : 0u;
            diag = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(mrs, ndiag | dead, 0, 0));
        }
        ndiag += ostep;
    };
    __syncthreads();                                         // ``removed`` is clear (fetch reads it)
    fetch(0, pc, dc);
    // The wait for a block's words is written out, HERE and at the end of every iteration, where the loads have had a whole
    // iteration to land.  Left to the compiler it sat at the first use of dc / pc in the NEXT iteration -- behind the fetch that
    // iteration had just issued, and vector loads return in order: vmcnt(0) there waited for the NEW block's words, a full memory
    // round trip on the serial chain of every block (in-kernel clocks: 950 of a block's 2.5k cycles in wave 0's resolve, for
    // three kept rows).
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0)
    __syncthreads();
    for (int rb = 0; rb < nblk; ++rb) {
        if (rb + 1 < nblk) fetch(rb + 1, pn, dn);            // lands during this iteration
        if (wave == 0) {
            const int row = rb * 64 + lane;
            // ``removed[rb]`` and ``s_count`` come from LDS: without the readfirstlane the compiler keeps them (and everything
            // derived: todo, kept, count) in VECTOR registers and runs the loop below under exec masks -- 950 cycles per block
            // for three kept rows (in-kernel clocks), the largest phase of the chain
            unsigned long long cur = uniform64(removed[rb]);
            const int valid = min(64, n - rb * 64);
            if (valid < 64) cur |= ~0ull << valid;
            unsigned long long kept = 0;
            const int count0 = __builtin_amdgcn_readfirstlane(s_count);
            int count = count0;
            // serial greedy resolve of the 64 rows of this block, entirely in scalar registers: jump
            // to the next unsuppressed row with ffs, fetch its diagonal word with v_readlane
            const unsigned dlo = (unsigned)dc, dhi = (unsigned)(dc >> 32);
            unsigned long long todo = ~cur;
            while (todo && count < limit) {
                const int i = __builtin_ctzll(todo);
                const unsigned long long d = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)dhi, i) << 32) |
                                             (unsigned)__builtin_amdgcn_readlane((int)dlo, i);
                kept |= 1ull << i;
                ++count;
                cur |= d;
                todo = ~cur & ~((2ull << i) - 1ull);       // rows after i that are still alive
            }
            if ((kept >> lane) & 1ull) keep[count0 + __popcll(kept & ((1ull << lane) - 1ull))] = row;
            if (lane == 0) { s_kept = kept; s_count = count; }
        }
        __syncthreads();
        const unsigned long long kept = uniform64(s_kept);
        if (__builtin_amdgcn_readfirstlane(s_count) >= limit) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!((kept >> (wave * 4 + r)) & 1ull)) continue;                  // scalar
#pragma unroll
            for (int c = 0; c < SCAN_PIPE_WORDS; ++c) {
                const int j = rb + 1 + lane + 64 * c;
                if (j < nblk && pc[r][c]) atomicOr(&removed[j], pc[r][c]);
            }
        }
        __syncthreads();
        __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0): the next block's words, requested an iteration ago
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < SCAN_PIPE_WORDS; ++c) pc[r][c] = pn[r][c];
        dc = dn;
    }
    if (threadIdx.x == 0) num_out[img] = s_count;
}

// Round 6 (the one algorithmic experiment round 5's review left open): the scan in SUPER-BLOCKS of 1024 rows whose 1024 x 1024
// triangle of the mask (16 words per row, 128 KB) sits in LDS.  The workgroup meets a handful of times per 1024 rows instead of
// twice per 64: to resolve the super-block, to fold the kept rows' words for LATER columns into the ``removed`` bitmap (kept rows
// only, from the mask in global memory: sixteen waves, a 64-row block each) and to bring the next triangle in (requested a
// super-block ahead, into registers).
//   ``fixed_point`` > 0 (the default): the super-block is resolved by fixed-point sweeps over the triangle, at most that many;
//   ``fixed_point`` = 0, or a super-block that has not settled: ONE wave walks the sixteen 64-row blocks serially -- the verdict
//   words of the super-block's own columns live in its lanes (lane w = word w), a block's rows are resolved in scalar registers
//   as in the pipelined kernel, the rows just kept are folded into those lanes by one LDS read each.  Alone this form is no
//   faster than the pipelined kernel (181.8 against 185.2 us): what the scan costs is the resolve's ~190 cycles of dependent
//   scalar instructions per KEPT row, not the barriers, the fetch or the fold.
// Either way the greedy keep set, row by row: bit-exact.

__global__ void __launch_bounds__(SCAN_THREADS)
nms_scan_super_kernel(const unsigned long long* __restrict__ mask, int n, int nblk, int max_keep,
                      int* __restrict__ keep_out, int* __restrict__ num_out, int fixed_point /* sweeps at most; 0: serial resolve */) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long tri[];       // [1024][16]
    __shared__ unsigned long long removed[64 * SCAN_PIPE_WORDS + SUPER_WORDS + 1];
    __shared__ unsigned long long s_kept[SUPER_WORDS];
    __shared__ int s_count;
    const int img = blockIdx.x;
    const unsigned long long* M = mask + (long long)img * n * nblk;
    int* keep = keep_out + (long long)img * n;
    for (int i = threadIdx.x; i < 64 * SCAN_PIPE_WORDS + SUPER_WORDS + 1; i += SCAN_THREADS) removed[i] = 0;
    if (threadIdx.x == 0) s_count = 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int limit = max_keep > 0 ? max_keep : n;
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc((void*)M, 0, (unsigned)((long long)n * nblk * 8), 0x00020000);
    const int nsuper = (n + SUPER_ROWS - 1) / SUPER_ROWS;
    // the triangle of super-block sb, 16 of its 16384 words per thread: pass p brings rows 64 p .. 64 p + 63, a thread one word of
    // one row (16 lanes = one row's 128 contiguous bytes: four cache lines per wave instruction.  One ROW per thread -- 64 lines
    // per instruction -- made the fetch 8 of a super-block's 12.5 us).  Words left of the row's own block were never written by
    // nms_mask_kernel (below the diagonal), words past the end of the row do not exist: both read as zero (the 2 GiB bit); a
    // row past n falls off the descriptor by itself
    unsigned long long tw[SUPER_WORDS];
    auto fetch_tri = [&](int sb) {
        const int w = (int)threadIdx.x & (SUPER_WORDS - 1), wa = sb * SUPER_WORDS + w;
#pragma unroll
        for (int p = 0; p < SUPER_ROWS / 64; ++p) {
            const int row = sb * SUPER_ROWS + 64 * p + ((int)threadIdx.x >> 4), rb = row >> 6;
            const unsigned dead = (row < n && wa >= rb && wa < nblk) ? 0u : 0x80000000u;
            tw[p] = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(mrs, ((unsigned)(row * nblk + wa) * 8u) | dead, 0, 0));
        }
    };
    fetch_tri(0);
    __syncthreads();                                         // ``removed`` is clear
    for (int sb = 0; sb < nsuper; ++sb) {
        const int r0 = sb * SUPER_ROWS, w0 = sb * SUPER_WORDS;
        __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0): my row's words, requested a super-block ago
#pragma unroll
        for (int p = 0; p < SUPER_ROWS / 64; ++p) tri[(64 * p) * SUPER_WORDS + threadIdx.x] = tw[p];
        __syncthreads();
        if (sb + 1 < nsuper) fetch_tri(sb + 1);              // lands while this super-block is resolved
        // ---- fixed-point resolve (round 5's review: "cluster-NMS"): keep <- alive & ~OR_{j kept} row_j, from keep = alive, until it
        // stops moving.  A row's verdict is final once the rows before it are (induction from row 0), so the fixed point is the
        // greedy keep set, reached after as many sweeps as the longest suppress-release chain in the 1024 rows is deep; a sweep is
        // 16 LDS reads per thread, two shuffles and one LDS atomic per 16 lanes.  The serial resolve a kept row at a time costs
        // ~190 cycles of one wave's dependent scalar instructions per KEPT row (2000 of them: the 182 us of either scan kernel).
        // Not settled after NMS_SWEEPS sweeps: the serial resolve below does the super-block (same answer, by construction).
        int settled = 0;
        if (fixed_point) {
            __shared__ unsigned long long s_alive[SUPER_WORDS], s_keepw[SUPER_WORDS], s_supp[SUPER_WORDS];
            // ``s_changed``: two slots, sweep s owns slot s & 1.  With one slot, cleared for sweep s + 1 before the first barrier of
            // that sweep, a wave that had not yet read sweep s's verdict could see the cleared flag, call the super-block settled
            // and meet the keep-list barrier while the others stood at the sweep's.  Now slot s & 1 is set (changed words) and slot
            // (s + 1) & 1 cleared (thread 0) only between the two barriers of sweep s: the readers of the cleared slot, sweep s - 1's,
            // have all passed the first of them, and the readers of the set slot come after the second.
            __shared__ int s_changed[2];
            if (threadIdx.x < SUPER_WORDS) {
                if (threadIdx.x < 2) s_changed[threadIdx.x] = 0;
                const int rb = w0 + (int)threadIdx.x;
                unsigned long long a = 0ull;
                if (rb < nblk) {
                    a = ~removed[rb];
                    const int valid = n - rb * 64;
                    if (valid < 64) a &= (1ull << valid) - 1ull;
                }
                s_alive[threadIdx.x] = a; s_keepw[threadIdx.x] = a; s_supp[threadIdx.x] = 0ull;
            }
            __syncthreads();
            const int w = threadIdx.x & (SUPER_WORDS - 1), g = threadIdx.x >> 4;         // my word; my 16 rows (16 g .. 16 g + 15)
            for (int sweep = 0; sweep < fixed_point; ++sweep) {
                const unsigned kb = (unsigned)(s_keepw[g >> 2] >> ((g & 3) * 16)) & 0xFFFFu;
                unsigned long long acc = 0ull;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned long long v = tri[(16 * g + r) * SUPER_WORDS + w];
                    acc |= ((kb >> r) & 1u) ? v : 0ull;
                }
                acc |= __shfl_xor(acc, 16);
                acc |= __shfl_xor(acc, 32);
                if (lane < SUPER_WORDS && acc) atomicOr(&s_supp[w], acc);
                __syncthreads();
                if (threadIdx.x < SUPER_WORDS) {
                    const unsigned long long nk = s_alive[threadIdx.x] & ~s_supp[threadIdx.x];
                    if (nk != s_keepw[threadIdx.x]) s_changed[sweep & 1] = 1;
                    s_keepw[threadIdx.x] = nk;
                    s_supp[threadIdx.x] = 0ull;
                    if (threadIdx.x == 0) s_changed[(sweep + 1) & 1] = 0;
                }
                __syncthreads();
                if (!s_changed[sweep & 1]) { settled = 1; break; }
            }
            if (settled) {
                // the keep list: rows in order, cut at the limit
                const int count0 = s_count;
                int before = 0;
                for (int q = 0; q < wave; ++q) before += __popcll(s_keepw[q]);
                const unsigned long long mine = s_keepw[wave];
                const int rank = before + __popcll(mine & ((1ull << lane) - 1ull));
                const bool k = ((mine >> lane) & 1ull) && count0 + rank < limit;
                __syncthreads();                             // everyone has read s_count / s_keepw
                if (k) keep[count0 + rank] = r0 + 64 * wave + lane;
                const unsigned long long cut = __ballot(k);
                if (lane == 0) s_kept[wave] = cut;
                if (threadIdx.x == 0) {
                    int total = 0;
                    for (int q = 0; q < SUPER_WORDS; ++q) total += __popcll(s_keepw[q]);
                    s_count = min(limit, count0 + total);
                }
            }
        }
        if (!settled && wave == 0) {
            // the verdicts on this super-block's columns so far: lane w holds word w0 + w
            unsigned long long rem = lane < SUPER_WORDS ? removed[min(w0 + lane, nblk)] : 0ull;
            int count = __builtin_amdgcn_readfirstlane(s_count);
            for (int q = 0; q < SUPER_WORDS && r0 + 64 * q < n; ++q) {
                const int rb = w0 + q;
                unsigned long long cur = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(rem >> 32), q) << 32) |
                                         (unsigned)__builtin_amdgcn_readlane((int)(unsigned)rem, q);
                const int valid = min(64, n - rb * 64);
                if (valid < 64) cur |= ~0ull << valid;
                const unsigned long long dq = tri[(64 * q + lane) * SUPER_WORDS + q];       // my row's diagonal word
                const unsigned dlo = (unsigned)dq, dhi = (unsigned)(dq >> 32);
                unsigned long long kept = 0, todo = ~cur;
                const int count0 = count;
                while (todo && count < limit) {              // serial greedy resolve in scalar registers (as the pipelined kernel's)
                    const int i = __builtin_ctzll(todo);
                    const unsigned long long d = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)dhi, i) << 32) |
                                                 (unsigned)__builtin_amdgcn_readlane((int)dlo, i);
                    kept |= 1ull << i;
                    ++count;
                    cur |= d;
                    todo = ~cur & ~((2ull << i) - 1ull);
                }
                if ((kept >> lane) & 1ull) keep[count0 + __popcll(kept & ((1ull << lane) - 1ull))] = rb * 64 + lane;
                if (lane == 0) s_kept[q] = kept;
                // the kept rows' words for the REST of this super-block's columns: one LDS read per row, all issued before the
                // first is used (lane w reads word w; words up to q are zero or already applied)
                unsigned long long k2 = kept;
                while (k2) {
                    unsigned long long v[8];
                    int m = 0;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        v[u] = 0ull;
                        if (k2) {
                            const int i = __builtin_ctzll(k2);
                            k2 &= k2 - 1ull;
                            v[u] = tri[(64 * q + i) * SUPER_WORDS + (lane & (SUPER_WORDS - 1))];
                            ++m;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) rem |= v[u];
                    (void)m;
                }
                if (count >= limit) {                        // the blocks behind keep nothing
                    for (int q2 = q + 1; q2 < SUPER_WORDS; ++q2) if (lane == 0) s_kept[q2] = 0ull;
                    break;
                }
            }
            for (int q2 = (n - r0 + 63) / 64; q2 < SUPER_WORDS; ++q2) if (lane == 0 && q2 >= 0) s_kept[q2] = 0ull;
            if (lane == 0) s_count = count;
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(s_count) >= limit || sb + 1 == nsuper) break;
        // fold: the kept rows of block w0 + wave, their words for the columns after this super-block (kept rows only; sixteen
        // rows' loads in flight per pass), OR-ed in registers and added to the bitmap once per wave
        {
            unsigned long long kk = uniform64(s_kept[wave]);
            unsigned long long acc[SCAN_PIPE_WORDS];
            unsigned past[SCAN_PIPE_WORDS];
#pragma unroll
            for (int c = 0; c < SCAN_PIPE_WORDS; ++c) { acc[c] = 0ull; past[c] = (w0 + SUPER_WORDS + lane + 64 * c < nblk) ? 0u : 0x80000000u; }
            while (kk) {
                unsigned long long v[8][SCAN_PIPE_WORDS];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
#pragma unroll
                    for (int c = 0; c < SCAN_PIPE_WORDS; ++c) v[u][c] = 0ull;
                    if (kk) {
                        const int i = __builtin_ctzll(kk);
                        kk &= kk - 1ull;
                        const unsigned off = (unsigned)((r0 + 64 * wave + i) * nblk + w0 + SUPER_WORDS + lane) * 8u;
#pragma unroll
                        for (int c = 0; c < SCAN_PIPE_WORDS; ++c)
                            if (w0 + SUPER_WORDS + 64 * c < nblk)
                                v[u][c] = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(mrs, (off | past[c]) + 512u * c, 0, 0));
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int c = 0; c < SCAN_PIPE_WORDS; ++c) acc[c] |= v[u][c];
            }
#pragma unroll
            for (int c = 0; c < SCAN_PIPE_WORDS; ++c) {
                const int j = w0 + SUPER_WORDS + lane + 64 * c;
                if (j < nblk && acc[c]) atomicOr(&removed[j], acc[c]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) num_out[img] = s_count;
}
}  // namespace

// mask, then the greedy scan; which scan is plan_nms's decision (roi_plan.h)
int32_t launch_nms(const float* dets, int n_img, int n, float thresh, int max_keep, int* keep, int* num,
                   unsigned long long* mask, hipStream_t st) {
    const NmsPlan pl = plan_nms(n_img, n, g_i2v_tuning);
    const dim3 mgrid(pl.mask_grid[0], pl.mask_grid[1], pl.mask_grid[2]), grid(pl.grid), thr(pl.threads);
    nms_mask_kernel<<<mgrid, dim3(pl.mask_threads), 0, st>>>(dets, n, pl.nblk, thresh, mask);
    switch (pl.form) {
    case NS_SUPER:
        I2V_ALLOW_LDS("nms_scan_super_kernel", pl.lds, nms_scan_super_kernel);
        nms_scan_super_kernel<<<grid, thr, pl.lds, st>>>(mask, n, pl.nblk, max_keep, keep, num, pl.sweeps);
        break;
    case NS_PIPELINED: nms_scan_pipelined_kernel<<<grid, thr, 0, st>>>(mask, n, pl.nblk, max_keep, keep, num); break;
    case NS_GENERIC: nms_scan_kernel<<<grid, thr, 0, st>>>(mask, n, pl.nblk, max_keep, keep, num); break;
    }
    return I2V_OK;
}

extern "C" size_t i2v_nms_workspace_bytes(int32_t n_img, int32_t n) {
    if (n_img <= 0 || n <= 0) return 256;
    return i2v_align((size_t)n_img * n * ((n + 63) / 64) * 8);
}

extern "C" int32_t i2v_nms_sorted(const float* dets, int32_t n_img, int32_t n, float thresh, int32_t max_keep,
                                  int32_t* keep_out, int32_t* num_out, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_img > 0 && n >= 0, "nms_sorted: bad shape");
    I2V_CHECK_ARG(num_out, "nms_sorted: null num_out");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {            // nms_wrapper.py:15-16: empty input -> empty keep
        hipMemsetAsync(num_out, 0, sizeof(int) * n_img, st);
        return I2V_OK;
    }
    I2V_CHECK_ARG(dets && keep_out, "nms_sorted: null pointer");
    I2V_CHECK_ARG(n <= 64 * SCAN_MAX_BLK, "nms_sorted: n > 65536 unsupported");
    if (ws_bytes < i2v_nms_workspace_bytes(n_img, n) || !ws) {
        i2v_set_error("nms_sorted: workspace %zu < %zu", ws_bytes, i2v_nms_workspace_bytes(n_img, n));
        return I2V_ERR_WORKSPACE;
    }
    const int32_t rc = launch_nms(dets, n_img, n, thresh, max_keep, keep_out, num_out, (unsigned long long*)ws, st);
    if (rc) return rc;
    I2V_CHECK_LAUNCH("nms_sorted");
    return I2V_OK;
}

// The plan of launch_nms as numbers (include/i2vsgg_hip.h has the field order): the launches i2v_nms_sorted,
// i2v_rpn_proposal (n = its pre-NMS top-n) and i2v_det_postprocess make for n boxes of n_img images.
extern "C" int32_t i2v_nms_plan(int32_t n_img, int32_t n, int32_t* out, int32_t n_out) {
    I2V_CHECK_ARG(out && n_out >= I2V_NMS_PLAN_FIELDS, "nms_plan: out needs room for I2V_NMS_PLAN_FIELDS values");
    I2V_CHECK_ARG(n_img > 0 && n > 0 && n <= 64 * SCAN_MAX_BLK, "nms_plan: bad shape");
    const NmsPlan pl = plan_nms(n_img, n, g_i2v_tuning);
    const int32_t v[I2V_NMS_PLAN_FIELDS] = {pl.status, pl.nblk, (int32_t)pl.mask_grid[0], (int32_t)pl.mask_grid[1], (int32_t)pl.mask_grid[2],
                                            pl.mask_threads, pl.form, pl.sweeps, (int32_t)pl.grid, pl.threads, (int32_t)pl.lds};
    std::copy(v, v + I2V_NMS_PLAN_FIELDS, out);
    return I2V_OK;
}
