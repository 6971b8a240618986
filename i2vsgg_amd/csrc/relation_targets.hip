// rel_det training targets: the detections of a minibatch are matched to the annotated boxes, every annotated relation draws up
// to 10 (subject detection, object detection) candidates without replacement, equal pairs merge into multi-hot rows of fixed
// shape.  The rules are stated once, in i2vsgg_amd/relation_targets.py; the host form there and these kernels evaluate the same
// float64 expressions in the same order (the library is built with -ffp-contract=off -fno-fast-math) and every decision of a
// draw is integer arithmetic, so they agree bit for bit.  No floating-point atomics; two runs give the same bits.
#include "table_common.h"

#define RT_CAP 64            // detections of one frame: lane a is detection a (relation_targets.CAP)
#define RT_DRAWS 10          // draws per annotated relation
#define RT_P 64              // pair rows per frame
#define RT_B 64              // rows of a frame in the padded box table
#define RT_EMIT_THREADS 256
#define RT_MARGIN 10.0       // of the union box (build_pair_tables)

// the integer weight of a candidate: both overlaps are in [0.5, 1], so it lies in [16384, 65536]
__device__ __forceinline__ unsigned long long rt_weight(double ia, double ib) {
    return (unsigned long long)floor((ia * ib) * 65536.0);
}

// inclusive sum over the 64 lanes; every lane takes part in every shuffle
__device__ __forceinline__ unsigned long long rt_scan(unsigned long long v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

struct RtTables {
    const int* det_off; const double* det_box; const int* det_cls;
    const int* gt_off; const double* gt_box; const int* gt_cls;
    const int* rel_off; const int* rel; const unsigned int* u;
    const double* ih; const double* iw;
    int n_frames, n_det, n_gt, n_relations, n_pred;
};

// Is frame f malformed?  Called by every thread of the block (it holds barriers); the answer is block-uniform.
//   each of the three offset tables: 0 <= off[f] <= off[f+1] <= size, and no earlier entry lies above off[f] (so the ranges of
//   two well-formed frames never overlap);  at most RT_CAP detections;  a finite positive image size;  every relation's boxes
//   inside the frame's annotated boxes and its predicate inside [0, n_pred).
__device__ int rt_frame_bad(const RtTables& T, int f) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int d0 = T.det_off[f], d1 = T.det_off[f + 1], g0 = T.gt_off[f], g1 = T.gt_off[f + 1];
    const int r0 = T.rel_off[f], r1 = T.rel_off[f + 1];
    int bad = 0;
    if (i2v_range_bad(d0, d1, T.n_det) || d1 - d0 > RT_CAP) bad = 1;
    if (i2v_range_bad(g0, g1, T.n_gt)) bad = 1;
    if (i2v_range_bad(r0, r1, T.n_relations)) bad = 1;
    const double h = T.ih[f], w = T.iw[f];
    if (!(h > 0.0) || !(w > 0.0) || !(h <= 1.0e9) || !(w <= 1.0e9)) bad = 1;
    for (int j = tid; j < f; j += nt)
        if (T.det_off[j] > d0 || T.gt_off[j] > g0 || T.rel_off[j] > r0) bad = 1;
    if (__syncthreads_or(bad)) return 1;
    const int ng = g1 - g0;
    for (int r = r0 + tid; r < r1; r += nt) {
        const int s = T.rel[(long long)r * 3], o = T.rel[(long long)r * 3 + 1], p = T.rel[(long long)r * 3 + 2];
        if (s < 0 || s >= ng || o < 0 || o >= ng || p < 0 || p >= T.n_pred) bad = 1;
    }
    return __syncthreads_or(bad);
}

// One wave per annotated relation: block (x, f) takes the relations rel_off[f] + x, + gridDim.x, ... of frame f.
__global__ void __launch_bounds__(RT_CAP)
relation_sample_kernel(RtTables T, int* __restrict__ samp) {
    __shared__ double s_iou[RT_CAP];                     // every lane's overlap with the relation's object box
    const int f = blockIdx.y, lane = threadIdx.x;
    if (rt_frame_bad(T, f)) return;                      // the emit kernel raises the status word
    const int d0 = T.det_off[f], nd = T.det_off[f + 1] - d0, g0 = T.gt_off[f];
    const int r0 = T.rel_off[f], r1 = T.rel_off[f + 1];
    double box[4] = {0.0, 0.0, 0.0, 0.0};
    int cls = 0;
    if (lane < nd) {
        for (int k = 0; k < 4; ++k) box[k] = T.det_box[(long long)(d0 + lane) * 4 + k];
        cls = T.det_cls[d0 + lane];
    }
    for (int r = r0 + (int)blockIdx.x; r < r1; r += (int)gridDim.x) {        // wave-uniform
        const int gs = g0 + T.rel[(long long)r * 3], go = g0 + T.rel[(long long)r * 3 + 1];
        double bs[4], bo[4];
        for (int k = 0; k < 4; ++k) bs[k] = T.gt_box[(long long)gs * 4 + k], bo[k] = T.gt_box[(long long)go * 4 + k];
        const double is = lane < nd ? i2v_overlap_plus1(box, bs) : 0.0;
        const double io = lane < nd ? i2v_overlap_plus1(box, bo) : 0.0;
        const bool ms = lane < nd && cls == T.gt_cls[gs] && is >= 0.5;
        const bool mo = lane < nd && cls == T.gt_cls[go] && io >= 0.5;
        const unsigned long long word_o = __ballot(mo);  // the subject side needs no word: lane a holds its own bit, ms
        __syncthreads();                                 // the previous relation's reads of s_iou are done
        s_iou[lane] = io;
        __syncthreads();
        unsigned long long alive = ms ? (word_o & ~(1ull << lane)) : 0ull;   // my row of the candidate matrix
        int ncand = __popcll(alive);
        for (int o = 32; o > 0; o >>= 1) ncand += __shfl_xor(ncand, o);
        const int K = ncand < RT_DRAWS ? ncand : RT_DRAWS;
        for (int k = 0; k < K; ++k) {
            unsigned long long row = 0ull, m = alive;
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1ull;
                row += rt_weight(is, s_iou[b]);
            }
            const unsigned long long incl = rt_scan(row, lane);
            const unsigned long long total = __shfl(incl, 63);
            const unsigned long long t = ((unsigned long long)T.u[(long long)r * RT_DRAWS + k] * total) >> 32;
            const unsigned long long rows = __ballot(incl > t);
            if (!rows) break;                            // cannot happen: t < total (every lane holds the same word)
            const int ra = __builtin_ctzll(rows);
            const unsigned long long before = __shfl(incl - row, ra);
            const unsigned long long word = __shfl(alive, ra);
            const double ia = __shfl(is, ra);
            const unsigned long long col = ((word >> lane) & 1ull) ? rt_weight(ia, io) : 0ull;
            const unsigned long long incl2 = rt_scan(col, lane);
            const unsigned long long cols = __ballot(incl2 > t - before);
            if (!cols) break;
            const int cb = __builtin_ctzll(cols);
            if (lane == ra) alive &= ~(1ull << cb);
            if (lane == 0) {
                samp[((long long)r * RT_DRAWS + k) * 2] = ra;
                samp[((long long)r * RT_DRAWS + k) * 2 + 1] = cb;
            }
        }
    }
}

// One workgroup per frame: the frame's entries (relation in annotation order, draw in draw order) merge by (a, b) in first-seen
// order into at most RT_P rows; every row of the frame is written, padding included.
__global__ void __launch_bounds__(RT_EMIT_THREADS)
relation_emit_kernel(RtTables T, const int* __restrict__ samp, float* __restrict__ rel5, int* __restrict__ bounds,
                     float* __restrict__ labels, long long* __restrict__ ixs, long long* __restrict__ ixo, float* __restrict__ w,
                     int* __restrict__ n_pairs, int* __restrict__ n_dropped, int* status) {
    __shared__ int s_first[RT_CAP * RT_CAP];             // the first entry that holds pair (a, b)
    __shared__ int s_pair[RT_CAP * RT_CAP];              // the pair's index in first-seen order
    __shared__ int s_wave[RT_EMIT_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bad = rt_frame_bad(T, f);
    if (bad && tid == 0) atomicMax(status, f + 1);
    const int d0 = bad ? 0 : T.det_off[f], nd = bad ? 0 : T.det_off[f + 1] - d0;
    const int r0 = bad ? 0 : T.rel_off[f], nr = bad ? 0 : T.rel_off[f + 1] - r0;
    const long long E = (long long)nr * RT_DRAWS;        // < 2^31: the host entry bounds n_relations
    const long long row0 = (long long)f * RT_P;

    // 0. tables, and every row of the frame as a padding row
    for (int k = tid; k < RT_CAP * RT_CAP; k += RT_EMIT_THREADS) s_first[k] = 0x7fffffff, s_pair[k] = 0x7fffffff;
    for (long long i = tid; i < (long long)RT_P * T.n_pred; i += RT_EMIT_THREADS) labels[row0 * T.n_pred + i] = 0.0f;
    for (int p = tid; p < RT_P; p += RT_EMIT_THREADS) {
        rel5[(row0 + p) * 5] = (float)f;
        for (int k = 1; k < 5; ++k) rel5[(row0 + p) * 5 + k] = 0.0f;
        for (int k = 0; k < 8; ++k) bounds[(row0 + p) * 8 + k] = 0;
        ixs[row0 + p] = (long long)f * RT_B;
        ixo[row0 + p] = (long long)f * RT_B;
        w[row0 + p] = 0.0f;
    }
    __syncthreads();
    // 1. first occurrences (an integer minimum: any order gives the same word)
    for (long long e = tid; e < E; e += RT_EMIT_THREADS) {
        const int a = samp[((long long)r0 * RT_DRAWS + e) * 2], b = samp[((long long)r0 * RT_DRAWS + e) * 2 + 1];
        if (a >= 0 && a < nd && b >= 0 && b < nd) atomicMin(&s_first[a * RT_CAP + b], (int)e);
    }
    __syncthreads();
    // 2. pair index = the number of first occurrences before the entry, by an ordered count over chunks of entries
    int n_unique = 0;
    const int chunks = (int)((E + RT_EMIT_THREADS - 1) / RT_EMIT_THREADS);
    for (int c = 0; c < chunks; ++c) {
        const long long e = (long long)c * RT_EMIT_THREADS + tid;
        int key = -1;
        if (e < E) {
            const int a = samp[((long long)r0 * RT_DRAWS + e) * 2], b = samp[((long long)r0 * RT_DRAWS + e) * 2 + 1];
            if (a >= 0 && a < nd && b >= 0 && b < nd && s_first[a * RT_CAP + b] == (int)e) key = a * RT_CAP + b;
        }
        const unsigned long long word = __ballot(key >= 0);
        if (lane == 0) s_wave[wave] = __popcll(word);
        __syncthreads();
        int before = n_unique, all = 0;
        for (int v = 0; v < RT_EMIT_THREADS / 64; ++v) {
            if (v < wave) before += s_wave[v];
            all += s_wave[v];
        }
        if (key >= 0) s_pair[key] = before + __popcll(word & ((1ull << lane) - 1ull));
        n_unique += all;
        __syncthreads();                                 // s_wave is free for the next chunk; s_pair is written
    }
    const int np = n_unique < RT_P ? n_unique : RT_P;
    // 3. rows and labels
    const double h = bad ? 1.0 : T.ih[f], wd = bad ? 1.0 : T.iw[f];
    const double rh = 32.0 / h, rw = 32.0 / wd;
    for (long long e = tid; e < E; e += RT_EMIT_THREADS) {
        const int a = samp[((long long)r0 * RT_DRAWS + e) * 2], b = samp[((long long)r0 * RT_DRAWS + e) * 2 + 1];
        if (!(a >= 0 && a < nd && b >= 0 && b < nd)) continue;
        const int key = a * RT_CAP + b, p = s_pair[key];
        if (p >= RT_P) continue;                         // beyond the capacity: dropped, counted below
        labels[(row0 + p) * T.n_pred + T.rel[((long long)r0 + e / RT_DRAWS) * 3 + 2]] = 1.0f;
        if (s_first[key] != (int)e) continue;
        double sb[4], ob[4];
        for (int k = 0; k < 4; ++k) sb[k] = T.det_box[(long long)(d0 + a) * 4 + k], ob[k] = T.det_box[(long long)(d0 + b) * 4 + k];
        // build_pair_tables' float64 expressions
        const double u0 = (sb[0] < ob[0] ? sb[0] : ob[0]) - RT_MARGIN, u1 = (sb[1] < ob[1] ? sb[1] : ob[1]) - RT_MARGIN;
        const double u2 = (sb[2] > ob[2] ? sb[2] : ob[2]) + RT_MARGIN, u3 = (sb[3] > ob[3] ? sb[3] : ob[3]) + RT_MARGIN;
        rel5[(row0 + p) * 5 + 1] = (float)(u0 > 0.0 ? u0 : 0.0);
        rel5[(row0 + p) * 5 + 2] = (float)(u1 > 0.0 ? u1 : 0.0);
        rel5[(row0 + p) * 5 + 3] = (float)(u2 < wd ? u2 : wd);
        rel5[(row0 + p) * 5 + 4] = (float)(u3 < h ? u3 : h);
        for (int side = 0; side < 2; ++side) {
            const double* bb = side ? ob : sb;
            const double x1 = floor(bb[0] * rw), y1 = floor(bb[1] * rh), x2 = ceil(bb[2] * rw), y2 = ceil(bb[3] * rh);
            int* out = bounds + (row0 + p) * 8 + side * 4;
            out[0] = (int)(x1 > 0.0 ? x1 : 0.0);
            out[1] = (int)(y1 > 0.0 ? y1 : 0.0);
            out[2] = (int)(x2 < 32.0 ? x2 : 32.0);
            out[3] = (int)(y2 < 32.0 ? y2 : 32.0);
        }
        ixs[row0 + p] = (long long)f * RT_B + a;
        ixo[row0 + p] = (long long)f * RT_B + b;
    }
    if (np > 0) {
        const float wt = (float)(1.0 / (double)((long long)np * T.n_frames));
        for (int p = tid; p < np; p += RT_EMIT_THREADS) w[row0 + p] = wt;
    }
    if (tid == 0) {
        n_pairs[f] = np;
        n_dropped[f] = n_unique - np;
    }
}

extern "C" size_t i2v_relation_targets_workspace_bytes(int32_t n_frames) {
    (void)n_frames;
    return I2V_STATUS_BYTES;                             // the status word
}

extern "C" int32_t i2v_relation_targets(const int32_t* det_off, const double* det_box, const int32_t* det_cls,
                                        const int32_t* gt_off, const double* gt_box, const int32_t* gt_cls,
                                        const int32_t* rel_off, const int32_t* rel, const uint32_t* u, const double* ih,
                                        const double* iw, int32_t n_frames, int32_t n_det, int32_t n_gt, int32_t n_relations,
                                        int32_t n_pred, float* rel5, int32_t* bounds, float* labels, int64_t* ixs, int64_t* ixo,
                                        float* w, int32_t* n_pairs, int32_t* n_dropped, int32_t* samp, void* ws, size_t ws_bytes,
                                        void* stream) {
    I2V_CHECK_ARG(n_frames >= 0 && n_det >= 0 && n_gt >= 0 && n_relations >= 0 && n_pred >= 0, "relation_targets: negative count");
    I2V_CHECK_ARG(n_frames <= 65535, "relation_targets: at most 65535 frames in one launch, got %d", n_frames);
    I2V_CHECK_ARG(n_relations <= 0x7fffffff / (2 * RT_DRAWS), "relation_targets: too many relations (%d)", n_relations);
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_relation_targets_workspace_bytes(n_frames), "relation_targets: workspace too small");
    I2V_CHECK_ARG(n_relations == 0 || (rel && u && samp), "relation_targets: null pointer");
    if (n_frames == 0) return I2V_OK;
    I2V_CHECK_ARG(det_off && gt_off && rel_off && ih && iw, "relation_targets: null pointer");
    I2V_CHECK_ARG(n_det == 0 || (det_box && det_cls), "relation_targets: null pointer");
    I2V_CHECK_ARG(n_gt == 0 || (gt_box && gt_cls), "relation_targets: null pointer");
    I2V_CHECK_ARG(rel5 && bounds && ixs && ixo && w && n_pairs && n_dropped && (n_pred == 0 || labels), "relation_targets: null pointer");
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "relation_targets: clearing the status word / the draws failed");
    if (n_relations > 0 && hipMemsetAsync(samp, 0xff, (size_t)n_relations * RT_DRAWS * 2 * sizeof(int32_t), st) != hipSuccess) {
        i2v_set_error("relation_targets: clearing the status word / the draws failed");
        return I2V_ERR_LAUNCH;
    }
    RtTables T = {det_off, det_box, det_cls, gt_off, gt_box, gt_cls, rel_off, rel, u, ih, iw, n_frames, n_det, n_gt, n_relations, n_pred};
    if (n_relations > 0) {
        relation_sample_kernel<<<dim3(64, n_frames), RT_CAP, 0, st>>>(T, samp);
        I2V_CHECK_LAUNCH("relation_sample");
    }
    relation_emit_kernel<<<n_frames, RT_EMIT_THREADS, 0, st>>>(T, samp, rel5, bounds, labels, (long long*)ixs, (long long*)ixo, w,
                                                               n_pairs, n_dropped, (int*)ws);
    I2V_CHECK_LAUNCH("relation_emit");
    return I2V_OK;
}
