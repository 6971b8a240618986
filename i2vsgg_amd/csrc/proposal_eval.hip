// Proposal / detection recall (i2vsgg_amd/proposal_eval.py states the rules in full): the greedy cover of every (image, limit,
// area range) cell -- repeatedly the best-covered ground truth still free takes the candidate that covers it, both retire.
// Overlaps are i2v_overlap_plus1 (float64, one rounding per operation: the library is built with -ffp-contract=off
// -fno-fast-math); every choice after that is an integer comparison.  No floating-point atomics and no order that depends on
// scheduling: two runs give the same bits, and the host form (proposal_eval.cover_arrays_host) gives them too.
//
// One workgroup of four waves per cell; cells are independent.  No candidates x ground truths matrix exists anywhere: an
// overlap is a dozen float64 operations and is recomputed.  What a cell keeps, in LDS:
//   best_ov / best_c   per ground truth of the cell (a "column") the largest overlap with a free candidate and the lowest
//                      candidate that has it; best_c is PE_NONE while no candidate is free, PE_RETIRED once the column is
//   gpos               the column's position among the image's ground truths (the cell's columns are those inside the range)
//   ret                one bit per candidate: retired
// Phases, each closed by a barrier that every wave reaches (the trip counts below depend only on m and k, which every thread
// reads from the same words; no wave leaves early):
//   0  wave 0 compacts the ground truths inside the range into gpos (ballot + prefix count, roidb row order); all threads
//      clear ``ret`` and write -1 for the ground truths outside the range.                                   -- barrier --
//   1  start: the waves divide the columns, lanes stride the candidates, a fixed butterfly on (overlap descending,
//      candidate ascending) leaves each column's best in best_ov / best_c.                                   -- barrier --
//   2  min(m, k) steps.  (a) wave 0 reduces over the columns on (overlap descending, position ascending), lane 0 records the
//      pick, sets the candidate's bit, marks the column retired and publishes the candidate in ``pick``.    -- barrier --
//      (b) the waves divide the columns, 64 at a time; a column whose stored best is the picked candidate is recomputed
//      over the free candidates (the others' bests are still free, hence still right).                       -- barrier --
//   3  wave 0 hands the columns still free (k < m) their misses in ascending position.
// Barrier argument: best_* written in 1 / 2b are read in 2a behind a barrier, and 2a's one write to them (the retired mark)
// is read in 2b behind the next; ``pick`` and ``ret`` are written in 2a only, read in 2b only, and the barrier that ends 2b
// stands between those reads and the next step's writes; ``m`` is written once, in phase 0.
#include "table_common.h"

#define PE_MAXG 4096         // ground truths of one image
#define PE_MAXC 65535        // candidates of one image
#define PE_MAXL 8            // limits of one call
#define PE_MAXA 8            // area ranges of one call
#define PE_THREADS 256
#define PE_WAVES (PE_THREADS / 64)
#define PE_NONE (-1)
#define PE_RETIRED (-2)

// dynamic LDS of a cell: best_ov (8 B), best_c (4 B), gpos (2 B) per ground truth, one bit per candidate, two control words.
// At both caps 57344 + 8192 + 8 = 65544 bytes: over 64 KB, inside the 160 KB a gfx950 workgroup may hold.
__host__ __device__ inline size_t pe_lds_bytes(int max_gt, int max_cand) {
    const size_t g = ((size_t)max_gt + 3) & ~(size_t)3;                  // keeps every array 8-byte aligned
    return g * 8 + g * 4 + g * 2 + (((size_t)max_cand + 63) / 64) * 8 + 8;
}

// (overlap descending, index ascending) over the wave, a fixed butterfly; every lane ends with the same pair
__device__ __forceinline__ void pe_wave_best(double& ov, int& ix) {
    for (int o = 32; o > 0; o >>= 1) {
        const double oo = __shfl_xor(ov, o);
        const int oi = __shfl_xor(ix, o);
        if (oi >= 0 && (ix < 0 || oo > ov || (oo == ov && oi < ix))) ov = oo, ix = oi;
    }
}

// the best free candidate of one ground truth: lanes stride the candidates in ascending order, so a lane keeps its first maximum
__device__ __forceinline__ void pe_column_best(const double* __restrict__ gb, const double* __restrict__ cand_box, int k,
                                               const unsigned int* ret, int lane, double& ov, int& ix) {
    const double g[4] = {gb[0], gb[1], gb[2], gb[3]};
    ov = 0.0;
    ix = PE_NONE;
    for (int c = lane; c < k; c += 64) {
        if ((ret[c >> 5] >> (c & 31)) & 1u) continue;
        const double o = i2v_overlap_plus1(g, cand_box + (size_t)c * 4);
        if (ix < 0 || o > ov) ov = o, ix = c;
    }
    pe_wave_best(ov, ix);
}

__global__ void __launch_bounds__(PE_THREADS)
proposal_cover_kernel(const int* __restrict__ cand_off, const double* __restrict__ cand_box, const int* __restrict__ gt_off,
                      const double* __restrict__ gt_box, const double* __restrict__ gt_area, const int* __restrict__ limits,
                      const double* __restrict__ ranges, int n_cand, int n_gt, int n_limits, int n_areas, int max_gt, int max_cand,
                      double* __restrict__ out_ov, int* __restrict__ out_cand, int* __restrict__ out_step, int* status) {
    extern __shared__ double pe_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cell = blockIdx.x;
    const int a = cell % n_areas, l = (cell / n_areas) % n_limits, img = cell / (n_areas * n_limits);
    const int c0 = cand_off[img], c1 = cand_off[img + 1], g0 = gt_off[img], g1 = gt_off[img + 1];
    // the same words for every thread: the whole workgroup leaves, or none of it
    if (i2v_range_bad(c0, c1, n_cand) || i2v_range_bad(g0, g1, n_gt) || c1 - c0 > max_cand || c1 - c0 > PE_MAXC || g1 - g0 > max_gt ||
        g1 - g0 > PE_MAXG) {
        if (tid == 0) atomicMax(status, img + 1);        // a malformed table: say so, touch nothing
        return;
    }
    const int nc = c1 - c0, ng = g1 - g0;
    const int lim = limits[l];
    const int k = lim < 1 ? 0 : (nc < lim ? nc : lim);           // a limit below 1 is the caller's mistake: no candidates, not a negative count
    const double lo = ranges[2 * a], hi = ranges[2 * a + 1];
    const size_t gcap = ((size_t)max_gt + 3) & ~(size_t)3;
    double* best_ov = pe_lds;
    int* best_c = (int*)(best_ov + gcap);
    unsigned short* gpos = (unsigned short*)(best_c + gcap);
    unsigned int* ret = (unsigned int*)(gpos + gcap);
    int* ctl = (int*)(ret + ((size_t)max_cand + 63) / 64 * 2);          // ctl[0]: m, ctl[1]: the candidate picked in this step
    const size_t out0 = ((size_t)l * n_areas + a) * (size_t)n_gt + g0;
    const double* cbox = cand_box + (size_t)c0 * 4;
    const double* gbox = gt_box + (size_t)g0 * 4;

    // ---- 0: the columns of the cell
    if (wave == 0) {
        int m = 0;
        for (int base = 0; base < ng; base += 64) {
            const int g = base + lane;
            bool in = false;
            if (g < ng) {
                const double ar = gt_area[g0 + g];
                in = ar >= lo && ar <= hi;
            }
            const unsigned long long mask = __ballot(in);
            if (in) gpos[m + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)g;
            m += __popcll(mask);
        }
        if (lane == 0) ctl[0] = m;
    }
    for (int w = tid; w < (k + 31) / 32; w += PE_THREADS) ret[w] = 0u;
    for (int g = tid; g < ng; g += PE_THREADS) {
        const double ar = gt_area[g0 + g];
        if (!(ar >= lo && ar <= hi)) {
            out_ov[out0 + g] = -1.0;
            out_cand[out0 + g] = -1;
            out_step[out0 + g] = -1;
        }
    }
    __syncthreads();
    const int m = ctl[0];

    // ---- 1: every column's best candidate
    for (int j = wave; j < m; j += PE_WAVES) {
        double ov;
        int ix;
        pe_column_best(gbox + (size_t)gpos[j] * 4, cbox, k, ret, lane, ov, ix);
        if (lane == 0) best_ov[j] = ov, best_c[j] = ix;
    }
    __syncthreads();

    // ---- 2: the steps; every free column has a free candidate while t < k
    const int n_steps = m < k ? m : k;
    for (int t = 0; t < n_steps; ++t) {
        if (wave == 0) {
            double ov = 0.0;
            int jx = PE_NONE;
            for (int j = lane; j < m; j += 64) {
                if (best_c[j] < 0) continue;
                const double o = best_ov[j];
                if (jx < 0 || o > ov) ov = o, jx = j;
            }
            pe_wave_best(ov, jx);
            if (lane == 0) {
                int c = PE_NONE;
                if (jx >= 0) {                           // always, by the trip count; a guard all the same
                    c = best_c[jx];
                    const size_t o = out0 + gpos[jx];
                    out_ov[o] = ov;
                    out_cand[o] = c;
                    out_step[o] = t;
                    best_c[jx] = PE_RETIRED;
                    ret[c >> 5] |= 1u << (c & 31);
                }
                ctl[1] = c;
            }
        }
        __syncthreads();
        const int picked = ctl[1];
        for (int base = wave * 64; base < m; base += PE_THREADS) {
            const int j = base + lane;
            unsigned long long redo = __ballot(picked >= 0 && j < m && best_c[j] == picked);
            while (redo) {                               // wave-uniform: every lane holds the same mask
                const int jj = base + __ffsll((long long)redo) - 1;
                redo &= redo - 1ull;
                double ov;
                int ix;
                pe_column_best(gbox + (size_t)gpos[jj] * 4, cbox, k, ret, lane, ov, ix);
                if (lane == 0) best_ov[jj] = ov, best_c[jj] = ix;
            }
        }
        __syncthreads();
    }

    // ---- 3: no candidate left for the columns still free
    if (wave == 0 && m > n_steps) {
        int s = n_steps;
        for (int base = 0; base < m; base += 64) {
            const int j = base + lane;
            const bool freecol = j < m && best_c[j] != PE_RETIRED;
            const unsigned long long mask = __ballot(freecol);
            if (freecol) {
                const size_t o = out0 + gpos[j];
                out_ov[o] = 0.0;
                out_cand[o] = -1;
                out_step[o] = s + __popcll(mask & ((1ull << lane) - 1ull));
            }
            s += __popcll(mask);
        }
    }
}

extern "C" size_t i2v_proposal_cover_workspace_bytes(int32_t n_images) {
    (void)n_images;
    return I2V_STATUS_BYTES;                             // the status header; the cells keep their state in LDS
}

extern "C" int32_t i2v_proposal_cover(const int32_t* cand_off, const double* cand_box, const int32_t* gt_off, const double* gt_box,
                                      const double* gt_area, const int32_t* limits, const double* ranges, int32_t n_images,
                                      int32_t n_cand, int32_t n_gt, int32_t n_limits, int32_t n_areas, int32_t max_gt,
                                      int32_t max_cand, double* ov, int32_t* cand, int32_t* step, void* ws, size_t ws_bytes,
                                      void* stream) {
    I2V_CHECK_ARG(n_images >= 0 && n_cand >= 0 && n_gt >= 0, "proposal_cover: negative count");
    I2V_CHECK_ARG(n_limits >= 1 && n_limits <= PE_MAXL, "proposal_cover: 1 to %d limits (got %d)", PE_MAXL, n_limits);
    I2V_CHECK_ARG(n_areas >= 1 && n_areas <= PE_MAXA, "proposal_cover: 1 to %d area ranges (got %d)", PE_MAXA, n_areas);
    I2V_CHECK_ARG(max_gt >= 0 && max_gt <= PE_MAXG, "proposal_cover: at most %d ground truths of one image (got %d)", PE_MAXG, max_gt);
    I2V_CHECK_ARG(max_cand >= 0 && max_cand <= PE_MAXC, "proposal_cover: at most %d candidates of one image (got %d)", PE_MAXC,
                  max_cand);
    I2V_CHECK_ARG(cand_off && gt_off && limits && ranges, "proposal_cover: null pointer");
    I2V_CHECK_ARG(n_cand == 0 || cand_box, "proposal_cover: null pointer");
    I2V_CHECK_ARG(n_gt == 0 || (gt_box && gt_area && ov && cand && step), "proposal_cover: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_proposal_cover_workspace_bytes(n_images), "proposal_cover: workspace too small");
    I2V_CHECK_ARG((long long)n_images * n_limits * n_areas < (1ll << 31), "proposal_cover: too many cells");
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "proposal_cover: clearing the status word failed");
    if (n_images == 0) return I2V_OK;
    const size_t lds = pe_lds_bytes(max_gt, max_cand);
    // once, for the largest cell the entry accepts (just over the 64 KB a launch gets by default)
    if (lds > 48 * 1024) I2V_ALLOW_LDS("proposal_cover_kernel", pe_lds_bytes(PE_MAXG, PE_MAXC), proposal_cover_kernel);
    proposal_cover_kernel<<<n_images * n_limits * n_areas, PE_THREADS, lds, st>>>(
        cand_off, cand_box, gt_off, gt_box, gt_area, limits, ranges, n_cand, n_gt, n_limits, n_areas, max_gt, max_cand, ov, cand,
        step, (int*)ws);
    I2V_CHECK_LAUNCH("proposal_cover");
    return I2V_OK;
}
