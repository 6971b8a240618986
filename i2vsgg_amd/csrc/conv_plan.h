// The launch plans of csrc/conv.hip and csrc/wgrad.hip: which tile, split, finish and kernel form a forward / data-gradient GEMM
// (plan_conv_fwd) or a filter-gradient GEMM (plan_wgrad) takes.  Host-only and pure: no HIP, no globals -- the tuning
// table (g_i2v_tuning, indexed by I2V_TUNE_*) and the forced tile come in as arguments, so a plan is a function of its
// arguments that the host tests check without a GPU (tests/test_conv_plan_host.py against tests/golden/conv_plans.json).
// The launchers (run_conv in conv.hip, launch_wgrad in wgrad.hip) only bind pointers, clear and switch on what these functions return.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/i2vsgg_hip.h"
#include "chip.h"

namespace convplan {

using i2v::NUM_CU;
constexpr int KTAB_MAX = 2560;  // filter-tap table entries (K/4): KH*KW*Cin <= 10240 for non-1x1 filters
constexpr int BKS = 32;         // k per LDS stage of the forward/dgrad kernel (= floats per LDS row)
constexpr int kSplitInKernelMax = 4;   // most splits the in-kernel split-K finish sums (else: atomics)
constexpr int kKGroups = 4;      // wave groups of the intra-workgroup K split (16 waves = 4 per SIMD, one workgroup per CU)
constexpr int kWgradOrderedMax = 16;     // most splits the ordered finish of a filter gradient sums (one workgroup reads them all)
// Split-K workspace, provided by the CALLER (i2v_conv_split_workspace_bytes): [kSplitCounters arrival counters | slab of
// partial tiles].  The counters must be zero before the first launch that uses the workspace; every launch leaves them
// zero again (the last workgroup to arrive at a tile resets its counter).  Launches that share a workspace must be
// ordered on the device (same stream, or graph edges): two concurrently running launches need two workspaces.
constexpr int kSplitCounters = 1024;
constexpr size_t kSplitCounterBytes = sizeof(int) * kSplitCounters;

struct TileCfg { int bm, bn; float eff; };
// eff: relative MFMA efficiency of the tile shape (operand reuse per LDS byte), from measurements
constexpr TileCfg kTiles[] = {{128, 128, 1.00f}, {128, 64, 0.97f}, {96, 64, 0.95f}, {80, 64, 0.95f}, {64, 64, 0.93f},
                              {32, 64, 0.80f}};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);
constexpr int kKgroupBm[4] = {80, 64, 48, 32};      // rows of the K-group tiles (all 64 columns), by K-group tile index

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// One convolution as a GEMM: M = B*Ho*Wo output pixels, N = Cout filters, K = KH*KW*Cin taps.  pad = top, pad_x = left padding
// (the sub-filters of a strided data gradient differ; may be negative: a crop); ostride = output pixel stride (the data
// gradient of a strided 1x1 layer); nbatch > 1: that many independent GEMMs in one launch (Winograd planes).
struct ConvShape {
    int B, H, W, Cin, Cout, KH, KW, stride, pad, pad_x, ostride, Ho, Wo, nbatch, flags;
    int M() const { return B * Ho * Wo; }
    int N() const { return Cout; }
    int K() const { return KH * KW * Cin; }
    int planes() const { return nbatch > 1 ? nbatch : 1; }
};

// a single tap read in place: no tap table, no halo in front of the activation
inline bool is_untapped(const ConvShape& s) { return s.KH == 1 && s.KW == 1 && s.pad == 0 && s.pad_x == 0; }
// the pointwise layers / plain GEMMs conv_gemm_f32 serves (when their split-K, if any, does not end in atomics)
inline bool is_pointwise(const ConvShape& s) {
    return is_untapped(s) && s.stride == 1 && s.ostride == 1 && s.Ho == s.H && s.Wo == s.W && (s.N() & 3) == 0 && (s.K() & 3) == 0;
}
// a filter gradient whose activations are read as a plain (pixels x Cin) matrix
inline bool is_linear(const ConvShape& s) { return s.KH == 1 && s.KW == 1 && s.pad == 0 && s.stride == 1; }

enum PlanStatus { PLAN_OK = 0, PLAN_TAP_TABLE = 1, PLAN_OPERAND_2GIB = 2, PLAN_ROW_SCALE_NEEDS_V2 = 3, PLAN_FUSED_NEEDS_SPLIT = 4 };
enum FwdForm { FORM_IGEMM = 0, FORM_GEMM = 1, FORM_GEMM_DMA32 = 2, FORM_GEMM_DMA16 = 3, FORM_GEMM_KGROUPS2 = 4, FORM_GEMM_KGROUPS4 = 5 };
enum FwdFinish { FIN_NONE = 0, FIN_IN_KERNEL = 1, FIN_ATOMICS = 2 };
enum EpiloguePass { PASS_NONE = 0, PASS_VEC4 = 1, PASS_SCALAR = 2 };     // also the form of a filter gradient's reduce pass

struct FwdPlan {
    int status;                  // PlanStatus; the other fields are valid for PLAN_OK only
    int tile;                    // index into kTiles
    int splitk, k_per_split;     // k_per_split multiple of BKS
    int ktab_entries;            // tap-table entries in LDS (>= 1; K/4 rounded up to whole stages for KxK filters)
    int form;                    // FwdForm
    int kg_tile;                 // K-group forms: index into kKgroupBm, else -1
    int finish;                  // FwdFinish
    size_t ws_wanted;            // split workspace the shape would use (0: none), whatever the caller offers
    size_t ws_used;              // what it uses of the ws_bytes offered (0: too small, or none wanted)
    int clear_y;                 // the atomics need a cleared y and the caller did not pass I2V_EPI_ZEROED
    int epilogue_pass;           // EpiloguePass: the atomics leave the epilogue to a pass of its own
    int ordered_fallback;        // order was asked for (SPLIT_ATOMICS == 0); the workspace (or a size cap) refused
    unsigned x_bytes, w_bytes;   // sizes of x and w for the buffer descriptors (< 2 GiB each)
};

// clk: the per-workgroup clock diagnostic is on (i2v_conv_debug_clock), which only the plain kernel forms carry.
// ws_bytes: the split workspace the caller offers (0: none).
inline FwdPlan plan_conv_fwd(const ConvShape& s, const int* tuning, int force_tile, bool clk, size_t ws_bytes) {
    FwdPlan q = {};
    const int M = s.M(), N = s.N(), K = s.K();
    if (!is_untapped(s) && (K > KTAB_MAX * 4 || s.KH * s.KW > 64 || ((long long)(s.KH * s.W + s.KW) * s.Cin) >= (1ll << 24))) {
        q.status = PLAN_TAP_TABLE;
        return q;
    }
    const long long xb = (long long)s.B * s.H * s.W * s.Cin * 4, wb = (long long)N * K * 4;
    const long long lead = (long long)(s.pad * s.W + s.pad_x) * s.Cin * 4;    // the kernel's descriptor starts this much earlier
    if (xb + (lead > 0 ? lead : 0) >= (1ll << 31) || wb >= (1ll << 31)) {
        q.status = PLAN_OPERAND_2GIB;
        return q;
    }
    q.ktab_entries = is_untapped(s) ? 4 : ((K + BKS - 1) / BKS) * (BKS / 4);
    q.x_bytes = (unsigned)xb;
    q.w_bytes = (unsigned)wb;
    const int split_atomics = tuning[I2V_TUNE_SPLIT_ATOMICS];
    const int ksteps = cdiv(K, BKS);
    // tile + split-K choice: minimise (rounds over the 256 CUs) x (MACs per workgroup) / efficiency.
    // The M of a 600x1000 frame pair at stride 16 is only 4788 rows, so wave quantisation decides
    // the shape; skinny GEMMs (vrd FCs: M = 128 rows) fill the chip by splitting K.
    // SPLIT_TARGET (workgroups per CU a split-K launch aims for), measured inside the step: 3 for the skinny FC GEMMs makes the
    // step 1 % faster (4.89 vs 4.94 ms) although fc6 forward alone goes from 410 to 556 us and its time becomes unstable; 3
    // for everything the same, 4 slower (5.21).  The default (2) is the setting that is best for the kernels on their own.
    auto cost_of = [&](int c, int& splitk) {
        const long long t = (long long)cdiv(M, kTiles[c].bm) * cdiv(N, kTiles[c].bn) * s.planes();
        splitk = 1;
        if (t < tuning[I2V_TUNE_SPLIT_BELOW] && ksteps >= 8 && s.ostride == 1 && s.nbatch <= 1) {
            const int skinny = tuning[I2V_TUNE_SPLIT_TARGET_SKINNY];
            const int target = (M <= 256 && skinny > 0) ? skinny : tuning[I2V_TUNE_SPLIT_TARGET];
            splitk = (int)((target * NUM_CU + t - 1) / t);
            splitk = splitk > ksteps / 4 ? ksteps / 4 : splitk;
            if (splitk < 1) splitk = 1;
            // Under round 4's rule (SPLIT_ATOMICS == 2) a large output split more than kSplitInKernelMax ways leaves the in-kernel
            // finish: fp32 atomics, a clear in front, a separate epilogue pass and the generic kernel -- none of which the 1.05
            // below prices.  Found on 600x801 frames (round 6, tools/size_probe.py): layer3 conv1 of ONE frame (M = 1900) took
            // 128x128 tiles x 8 splits = 240 workgroups, "one round", and ran at 42 TF on conv_igemm_f32 where the 64x64 x 4 plan
            // runs at 80 on conv_gemm_f32 -- the loader-fed step was 7 % slower on the SMALLER frames.  Such outputs split at most
            // kSplitInKernelMax ways.
            if (split_atomics == 2 && splitk > kSplitInKernelMax && (long long)M * N >= (1 << 18)) splitk = kSplitInKernelMax;
        }
        const long long blocks = t * splitk;
        const long long rounds = (blocks + NUM_CU - 1) / NUM_CU;
        // beyond ~4 rounds several workgroups share a CU and the tail matters less
        const double r = rounds <= 4 ? (double)rounds : (double)blocks / NUM_CU + 0.5;
        double cost = r * kTiles[c].bm * kTiles[c].bn * (double)cdiv(ksteps, splitk) / kTiles[c].eff;
        if (splitk > 1) cost *= 1.05;     // memset + atomics + separate epilogue pass
        return cost;
    };
    int cfg = 0, splitk = 1;
    double best = 1e300;
    for (int c = 0; c < kNumTiles; ++c) {
        int sk;
        const double cost = cost_of(c, sk);
        if (cost < best) { best = cost; cfg = c; splitk = sk; }
    }
    // HBM-bound pointwise layers (at most four K stages over many rows: the 64 -> 256 / 128 -> 512 expansions of layer1 / layer2 and
    // their data gradients): the model's MAC count cannot tell the tiles apart (all within 2 %) and picks 128x64; measured, the
    // 80x64 tile streams best (tools/pers_bench.py, two frames: layer1 conv3 44.0 against 50.7 us, layer2 conv3 33.3 against 37.6)
    if (tuning[I2V_TUNE_STREAM_TILE] && s.KH == 1 && s.KW == 1 && s.stride == 1 && s.nbatch <= 1 && ksteps <= 4 && M >= 16384) {
        cfg = 3;
        cost_of(cfg, splitk);
    }
    // batched launches with at most four K stages (the Winograd planes of the 64- and 128-channel layers): per-workgroup
    // set-up and epilogue dominate and the model underrates the smallest tile (measured 23.5 vs 27.4 us at 64 channels)
    if (s.nbatch > 1 && ksteps <= 4) { cfg = kNumTiles - 1; cost_of(cfg, splitk); }
    // the long skinny GEMM of the relation head (fc6 forward: 128 rows, K = 50176): 128x64 tiles instead of the 128x128 the
    // model picks -- twice the workgroups, each half as heavy.  Alone 436 vs 412 us, inside the two-stream step 4.88 vs
    // 4.93 ms (the same effect as with the fused update's tile: lighter workgroups give the other stream its turn sooner)
    const int big_fc_tile = tuning[I2V_TUNE_BIG_FC_TILE];
    if (big_fc_tile >= 0 && big_fc_tile < kNumTiles && M <= 256 && K >= 16384) { cfg = big_fc_tile; cost_of(cfg, splitk); }
    if (force_tile >= 0 && force_tile < kNumTiles) { cfg = force_tile; cost_of(cfg, splitk); }
    q.tile = cfg;
    q.k_per_split = cdiv(ksteps, splitk) * BKS;
    q.splitk = cdiv(K, q.k_per_split);
    // Intra-workgroup K split (conv_gemm_f32<.., KG>): a pointwise GEMM the plan would split over K through memory runs as ONE
    // 16-wave workgroup per tile whose four wave groups each take a quarter of K and meet in LDS -- same waves per SIMD, no partial
    // tile leaves the CU.  Its four stage-buffer sets leave room for one workgroup per CU, so it pays when the tiles of ONE round
    // cover most of the chip: of the tiles 80x64 / 64x64 / 48x64 / 32x64 the smallest (least work per CU) with at most 256 tiles,
    // if that is at least 180 (70 % of the CUs); otherwise the split across workgroups stays (layer3 conv1: 240 tiles of 80x64 for
    // a frame pair, 200 of 48x64 for one frame; tools/kgroup_bench.py).  K a multiple of 4 x 32 with >= 2 stages per group.
    // KG = 4 (round 4): 16 waves, 115-156 KB -- the workgroup owns its CU.  KG = 2 (round 5): 8 waves, 58-78 KB -- two of them, or
    // one and the 4-wave workgroups of the step's other branches, share a CU.
    const bool gemm_kernel = is_pointwise(s) && tuning[I2V_TUNE_CONV_GEMM];
    const int kgroups = tuning[I2V_TUNE_KGROUPS];
    q.kg_tile = -1;
    const int kgn = kgroups == 2 ? 2 : kKGroups;       // wave groups: 2 (round 5), or 4 (1 / 4)
    if (kgroups && gemm_kernel && !clk && s.nbatch <= 1 && q.splitk >= 2 && force_tile < 0 && K % (kgn * BKS) == 0 &&
        K / kgn >= 2 * BKS && (long long)M * N >= (1 << 18)) {
        const int nt = cdiv(N, 64);
        for (int c = 3; c >= 0; --c) {                       // smallest tile first
            const int t = cdiv(M, kKgroupBm[c]) * nt;
            if (t <= NUM_CU) { if (t >= (NUM_CU * 7) / 10) q.kg_tile = c; break; }
        }
        if (q.kg_tile >= 0) { q.splitk = 1; q.k_per_split = K; }
    }
    const long long ntiles = (long long)cdiv(M, kTiles[cfg].bm) * cdiv(N, kTiles[cfg].bn);
    const size_t ws_need = (size_t)q.splitk * ntiles * kTiles[cfg].bm * kTiles[cfg].bn * sizeof(float);
    // in-kernel finish pays where the output is large (atomics and the extra epilogue pass scale with it);
    // for the small FC outputs of the vrd head the atomics are cheap and a serial sum of many splits is not
    // round 5: the ordered finish takes ANY number of splits (rounds of kSplitInKernelMax) and any output size, so that no
    // forward or data-gradient GEMM of the relation head depends on arrival order (SPLIT_ATOMICS = 2 restores round 4's rule
    // everywhere: atomics beyond four splits and for outputs under 2^18 elements; 1: atomics always)
    // SPLIT_ATOMICS == 0 (what the relation step's head context selects, launch.LaunchContext(ordered=True)): ordered for every
    // shape.  The process default is 2, round 4's rule: measured on configs[2], ordering every reduction of the step -- its
    // 8-16-way filter-gradient splits, the bias sums of netD_style's 37500-row projections -- costs 46.2 -> 48.1 ms.
    const bool r4_ok = q.splitk <= kSplitInKernelMax && (long long)M * N >= (1 << 18);
    const bool wants_ws = q.splitk > 1 && split_atomics != 1 && (r4_ok || split_atomics == 0) && ntiles <= kSplitCounters &&
                          ws_need < (1ull << 31) - (64u << 20);
    const bool in_kernel = wants_ws && kSplitCounterBytes + ws_need <= ws_bytes;
    q.ws_wanted = wants_ws ? (kSplitCounterBytes + ws_need < 0x7FFFFFFF ? kSplitCounterBytes + ws_need : 0x7FFFFFFF) : 0;
    q.ws_used = in_kernel ? kSplitCounterBytes + ws_need : 0;
    q.finish = q.splitk <= 1 ? FIN_NONE : in_kernel ? FIN_IN_KERNEL : FIN_ATOMICS;
    q.ordered_fallback = q.finish == FIN_ATOMICS && split_atomics == 0;
    q.clear_y = q.finish == FIN_ATOMICS && !(s.flags & I2V_EPI_ZEROED);
    if (q.finish == FIN_ATOMICS && (s.flags & (I2V_EPI_SCALE | I2V_EPI_BIAS | I2V_EPI_RESIDUAL | I2V_EPI_RELU | I2V_EPI_MASK)))
        q.epilogue_pass = N % 4 == 0 ? PASS_VEC4 : PASS_SCALAR;
    // round 6: LDS-DMA staging of conv_gemm_f32 (I2V_TUNE_GEMM_DMA: 1 = 32-k stages, 2 = 16-k stages / half the LDS; 0 = through
    // registers)
    const int dma = tuning[I2V_TUNE_GEMM_DMA];
    if (q.kg_tile >= 0) q.form = kgroups == 2 ? FORM_GEMM_KGROUPS2 : FORM_GEMM_KGROUPS4;
    else if (!gemm_kernel || q.finish == FIN_ATOMICS) q.form = FORM_IGEMM;
    else if (dma > 0 && !clk) q.form = dma == 2 ? FORM_GEMM_DMA16 : FORM_GEMM_DMA32;
    else q.form = FORM_GEMM;
    return q;
}

// ---------------------------------------------------------------- filter gradients
enum WgradKernel {           // the instantiations launch_wgrad switches over
    WG_V1_64x64 = 0, WG_V2_DMA_128x128, WG_V2_DMA_128x64, WG_V2_DMA_64x64, WG_V2_FUSED_128x64, WG_V2_128x128, WG_V2_128x64,
    WG_V2_FUSED_64x64, WG_V2_CLK_64x64, WG_V2_64x64,
    WG_FC_UPDATE             // the persistent fused update (fc_update_f32) instead of a tiled kernel
};
enum WgradFinish { WFIN_DIRECT = 0, WFIN_ATOMICS = 1, WFIN_ORDERED_TILES = 2, WFIN_ORDERED_PARTS = 3, WFIN_EXTERNAL_PARTS = 4 };

struct WgradPlan {
    int status;                  // PlanStatus; the other fields are valid for PLAN_OK only
    int v2;                      // the second-generation kernel serves the shape (Cout % 4 == 0, operands under 2 GiB, WGRAD_V2)
    int kernel;                  // WgradKernel
    int tm, tk;                  // filters x taps per workgroup
    int splits, m_per_split;     // parts of the pixel reduction; m_per_split a multiple of the kernel's stage depth
    int finish;                  // WgradFinish
    int direct;                  // the kernel stores (or, fused, updates) instead of adding to gw
    int xcd_remap;               // (tile, split, plane) from a 1-D dispatch index so that a split's tiles share an XCD
    int tiles;                   // output tiles per plane
    unsigned grid[3];
    int dma;                     // LDS-DMA staging
    size_t clear_bytes;          // gw is cleared in front (atomics that overwrite): this many bytes, else 0
    int reduce_pass;             // EpiloguePass: ORDERED_PARTS are summed by a reduce pass of this form
    int ordered_fallback;        // order was asked for and the workspace refused: fp32 atomics
    unsigned x_bytes, gy_bytes;  // buffer descriptor sizes (v2 kernel)
};

// the pixel split an unfused problem of `planes` x (N x K) filters over M reduction rows gets
// one round of workgroups: floor, not ceil (144 tiles x 8 splits = 1152 workgroups on 1024 slots ran 1.5 rounds)
inline int wgrad_split_count(long long M, int N, int K, int planes, int tm, int tk, int rs, const int* tuning) {
    const long long tiles = (long long)cdiv(N, tm) * cdiv(K, tk), all_tiles = tiles * planes;
    const int msteps = cdiv(M, rs), per_cu = tuning[I2V_TUNE_WGRAD_PER_CU];
    int splits = (int)((long long)per_cu * NUM_CU / all_tiles);
    if (splits < 2) splits = (int)(((long long)per_cu * NUM_CU + all_tiles - 1) / all_tiles);
    if (splits > msteps / 4) splits = msteps / 4;
    if (splits < 1) splits = 1;
    return splits;
}

// (csrc/winograd.hip) the parts a 36-plane Winograd filter gradient is split into when its sum is ordered: what its workspace holds
inline int wgrad_plane_splits(long long T, int Cout, int Cin, const int* tuning) {
    const int s = wgrad_split_count(T, Cout, Cin, 36, 64, 64, BKS, tuning);
    const int mps = cdiv(cdiv(T, BKS), s) * BKS;
    return cdiv(T, mps);
}

// beta_nonzero: gw += sum instead of gw = sum.  fused: the SGD update happens in the kernel's epilogue (i2v_conv_wgrad_sgd; no
// split).  ext_part_cap >= 0: the caller owns a slab of that many parts and sums them itself (the Winograd filter gradient's
// final transform); < 0: none.  ws_bytes: the split workspace the caller offers (0: none).
inline WgradPlan plan_wgrad(const ConvShape& s, bool beta_nonzero, bool fused, bool has_row_scale, int ext_part_cap, const int* tuning,
                            bool clk, size_t ws_bytes) {
    WgradPlan q = {};
    const int M = s.M(), N = s.N(), K = s.K(), planes = s.planes();
    const int wgrad_v2 = tuning[I2V_TUNE_WGRAD_V2];
    const long long xb = (long long)s.B * s.H * s.W * s.Cin * 4, gb = (long long)M * N * 4;
    const bool lin = is_linear(s);
    if (fused) {
        // only when the whole reduction over the pixels fits one workgroup pass (no split over m), i.e. the skinny relation-head GEMMs
        if ((long long)cdiv(N, 64) * cdiv(K, 64) < 2 * NUM_CU || M > 4096) { q.status = PLAN_FUSED_NEEDS_SPLIT; return q; }
        // the persistent fused update; not for filters of more than one tap, more than 256 rows, Cout % 4 != 0 or the
        // first-generation wgrad selected (their MFMA chain differs: bit-equality holds against conv_wgrad2_f32 only), operands
        // of 2 GiB or more -- those take the tiled kernel
        if (tuning[I2V_TUNE_FC_UPDATE] && wgrad_v2 && lin && M <= 256 && N % 4 == 0 && K % 4 == 0 && (long long)M * K * 4 < (1ll << 31) &&
            gb < (1ll << 31) && (long long)N * K * 4 < (1ll << 31)) {
            q.v2 = 1; q.kernel = WG_FC_UPDATE; q.splits = 1; q.direct = 1; q.finish = WFIN_DIRECT;
            return q;
        }
    }
    const bool v2 = (N % 4 == 0) && xb < (1ll << 31) && gb < (1ll << 31) && wgrad_v2;
    q.v2 = v2;
    if (has_row_scale && !v2) { q.status = PLAN_ROW_SCALE_NEEDS_V2; return q; }
    // bigger tiles raise the FLOP per staged byte (the reduction dim is streamed): 128x128 = 32 FLOP/B vs 16
    int tm = 64, tk = 64;
    // fused update: 128 filters x 64 taps -- the x tile is shared by twice the filters and half as many workgroups go
    // through the dispatcher.  Alone the kernel is slower than the 64x64 form (fc6: 792 vs 736 us), inside the step it is
    // faster (4.93 vs 5.00 ms, four alternating pairs): the rest of the step gets the chip back sooner
    if (v2 && fused && tuning[I2V_TUNE_WGRAD_FUSED_TILE] == 128 && N >= 128) tm = 128;
    if (v2 && wgrad_v2 >= 2) {
        if (N >= 128) tm = 128;
        if (K >= 128 && tm == 128 && wgrad_v2 == 2) tk = 128;
    }
    const long long tiles = (long long)cdiv(N, tm) * cdiv(K, tk);
    const int rs = v2 ? BKS : 16;
    const int msteps = cdiv(M, rs);
    int splits = fused ? 1 : wgrad_split_count(M, N, K, planes, tm, tk, rs, tuning);
    // Every split a caller wants ordered (SPLIT_ATOMICS == 0, below I2V_TUNE_WGRAD_ORDERED_GFLOP) IS ordered, whatever its
    // size.  Up to kWgradOrderedMax parts of the second-generation kernel meet in the workspace as tiles and the tile's last
    // workgroup sums them (round 5): bit-reproducible, no clear of gw.  More parts -- the instance_styleD backbone splits up to
    // 254 ways to fill the chip -- and the first-generation kernel (Cout % 4 != 0) store their partial FILTERS side by side and a
    // reduce pass adds them in split order (round 6; round 5 left these on atomics, and ran the first-generation kernel UNSPLIT
    // when order was asked for: the RPN's 18-row cls_score gradient over 9576 pixels on eight workgroups, 300 us instead of 9
    // -- that alone was the "+4 %" ordered sums cost configs[2]).
    const bool ext_part = ext_part_cap >= 0;      // the caller reduces (the Winograd filter gradient's final transform): its own slab
    const bool has_ws = ws_bytes > 0;
    const double ord_flops = 1e9 * tuning[I2V_TUNE_WGRAD_ORDERED_GFLOP], flops = 2.0 * M * N * K * planes;
    const bool want_ord = !fused && !ext_part && splits > 1 && tuning[I2V_TUNE_SPLIT_ATOMICS] == 0 && flops < ord_flops;
    // a split beyond kWgradOrderedMax parts is capped where that costs nothing (under 1 GFLOP: conv_lo.0's 128-way split of a
    // 0.3 GFLOP problem): the in-kernel finish needs no second launch
    if (want_ord && has_ws && v2 && splits > kWgradOrderedMax && flops < 1e9) splits = kWgradOrderedMax;
    if (ext_part && splits > ext_part_cap) splits = ext_part_cap > 0 ? ext_part_cap : 1;
    q.m_per_split = cdiv(msteps, splits) * rs;
    splits = cdiv(M, q.m_per_split);
    q.direct = (splits == 1 && !beta_nonzero) || fused;
    q.finish = q.direct ? WFIN_DIRECT : WFIN_ATOMICS;
    if (ext_part) {
        if (splits > 1) q.finish = WFIN_EXTERNAL_PARTS;      // one part: written straight to gw (the caller passed its slot 0 as gw)
    } else if (want_ord && splits > 1) {
        const size_t need_ord = kSplitCounterBytes + (size_t)splits * tiles * planes * (size_t)(tm * tk) * sizeof(float);
        const size_t need_part = kSplitCounterBytes + (size_t)splits * planes * (size_t)N * K * sizeof(float);
        if (has_ws && v2 && splits <= kWgradOrderedMax && tiles * planes <= kSplitCounters && need_ord <= ws_bytes && need_ord < (1ull << 31))
            q.finish = WFIN_ORDERED_TILES;
        else if (has_ws && need_part <= ws_bytes) {
            q.finish = WFIN_ORDERED_PARTS;                   // behind the counters, which stay zero
            q.reduce_pass = (((long long)N * K) & 3) == 0 ? PASS_VEC4 : PASS_SCALAR;
        } else q.ordered_fallback = 1;                       // no workspace, or too small: fp32 atomics (i2v_ordered_fallbacks() tells)
    }
    if (!beta_nonzero && q.finish == WFIN_ATOMICS) q.clear_bytes = (size_t)planes * N * K * sizeof(float);
    q.x_bytes = (unsigned)xb;
    q.gy_bytes = (unsigned)gb;
    q.tm = tm; q.tk = tk; q.splits = splits; q.tiles = (int)tiles;
    q.grid[0] = (unsigned)tiles; q.grid[1] = (unsigned)splits; q.grid[2] = (unsigned)planes;
    const long long groups = (long long)splits * planes, total = tiles * groups;
    // v2 kernels only (the remap lives there); one group needs no grouping; the 1-D launch must fit an int
    q.xcd_remap = (v2 && groups >= 2 && total < (1ll << 30) && tuning[I2V_TUNE_WGRAD_XCD]) ? 1 : 0;
    if (q.xcd_remap) { q.grid[0] = (unsigned)((total + 7) / 8 * 8); q.grid[1] = 1; q.grid[2] = 1; }
    // round 6: LDS-DMA staging for the pointwise / linear problems (most of a backbone's filter-gradient time: the 1x1 layers and
    // the Winograd-domain plane GEMMs)
    const bool dma = v2 && !fused && !clk && lin && (K % 4 == 0) && tuning[I2V_TUNE_WGRAD_DMA];
    q.dma = dma;
    if (!v2) q.kernel = WG_V1_64x64;
    else if (dma && tm == 128 && tk == 128) q.kernel = WG_V2_DMA_128x128;
    else if (dma && tm == 128) q.kernel = WG_V2_DMA_128x64;
    else if (dma) q.kernel = WG_V2_DMA_64x64;
    else if (fused && tm == 128 && tk == 64) q.kernel = WG_V2_FUSED_128x64;
    else if (tm == 128 && tk == 128) q.kernel = WG_V2_128x128;
    else if (tm == 128) q.kernel = WG_V2_128x64;
    else if (fused) q.kernel = WG_V2_FUSED_64x64;
    else if (clk) q.kernel = WG_V2_CLK_64x64;
    else q.kernel = WG_V2_64x64;
    return q;
}

}  // namespace convplan
