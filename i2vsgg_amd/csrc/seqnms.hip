// Seq-NMS (Han et al., 2016): the per-frame, per-class detections of a video are linked into tracks, every track's boxes are
// rescored together and what they overlap is suppressed.  The rules are stated once, in i2vsgg_amd/seqnms.py; the host form
// there and this kernel evaluate the same float64 expressions in the same order on exactly widened float32 inputs (the
// library is built with -ffp-contract=off -fno-fast-math), so they agree bit for bit.  No floating-point atomics; every
// reduction has a fixed order, so two runs give the same bits.
#include "table_common.h"

#define SQ_CAP 64            // boxes of one frame that take part in a group: lane a is box a (seqnms.CAP)
#define SQ_NONE 0x7fffffff

__device__ __forceinline__ void sq_widen(const float* __restrict__ box, long long i, double* out) {
    for (int k = 0; k < 4; ++k) out[k] = (double)box[i * 4 + k];
}

// One workgroup of one wave per group (video, class), persistent over the group's passes.
//   link (N u64): bit b of box (t, a) = box b of frame t + 1 is a successor (built once);  best (N f64), ptr (N int):
//   the dynamic programme's state of every alive box;  alive (F u64);  fmax / farg (F): the largest best among a frame's
//   alive boxes and the lowest lane that has it (-1: none alive), so that a pass finds its start in F / 64 steps.
__global__ void __launch_bounds__(SQ_CAP)
seqnms_kernel(const int* __restrict__ group_off, const int* __restrict__ frame_no, const int* __restrict__ box_off,
              const float* __restrict__ box, const float* __restrict__ score, int n_frames, int n_boxes, double link_iou,
              double nms_iou, int rescore, unsigned long long* link, double* best, int* ptr, unsigned long long* alive,
              double* fmax, int* farg, int* tid, float* new_score, int* n_tracks, int* status) {
    __shared__ double s_box[SQ_CAP][4];                  // the next frame's boxes while the links are built
    __shared__ double s_best[2][SQ_CAP];                 // best of frame t + 1 (read) and of frame t (written)
    const int g = blockIdx.x, lane = threadIdx.x;
    const int f0 = group_off[g], f1 = group_off[g + 1];
    int bad = i2v_range_bad(f0, f1, n_frames) ? 1 : 0;
    if (!bad) {
        for (int f = f0 + lane; f < f1; f += SQ_CAP) {
            const int p0 = box_off[f], n = box_off[f + 1] - p0;
            // i2v_span_bad's test with the cap in its middle, spelled out: through the helper the kernel measured 1.3 % slower
            if (p0 < 0 || n < 0 || n > SQ_CAP || (long long)p0 + n > n_boxes) bad = 1;
        }
    }
    if (__syncthreads_or(bad)) {                         // a malformed table: say so, touch nothing else
        if (lane == 0) {
            atomicMax(status, g + 1);
            n_tracks[g] = 0;
        }
        return;
    }
    const int nf = f1 - f0;
    const int nbox = nf > 0 ? box_off[f1] - box_off[f0] : 0;     // every count is >= 0 and every end <= n_boxes

    // 0. links, and the start state: every box alive, no track, its own score
    for (int f = f0; f < f1; ++f) {
        const int p0 = box_off[f], n = box_off[f + 1] - p0;
        const bool linked = f + 1 < f1 && (long long)frame_no[f + 1] == (long long)frame_no[f] + 1;   // a gap breaks every link
        const int q0 = linked ? box_off[f + 1] : 0;
        const int m = linked ? box_off[f + 2] - q0 : 0;
        if (lane < m) sq_widen(box, (long long)q0 + lane, s_box[lane]);
        __syncthreads();
        if (lane < n) {
            double a[4];
            sq_widen(box, (long long)p0 + lane, a);
            unsigned long long mask = 0;
            for (int b = 0; b < m; ++b)
                if (i2v_overlap_plus1(a, s_box[b]) >= link_iou) mask |= 1ull << b;
            link[p0 + lane] = mask;
            best[p0 + lane] = 0.0;
            ptr[p0 + lane] = -1;
            tid[p0 + lane] = -1;
            new_score[p0 + lane] = score[p0 + lane];
        }
        if (lane == 0) {
            alive[f] = n == SQ_CAP ? ~0ull : (1ull << n) - 1ull;
            fmax[f] = 0.0;
            farg[f] = -1;
        }
        __syncthreads();                                 // s_box is free for the next frame
    }

    int ts = f1, te = f1 - 1;                            // the last path's first and last frame: only frames <= te can change
    int k = 0;
    for (; k < nbox; ++k) {                              // a pass takes at least one box
        // 1. best / ptr backwards from te (the first pass: every frame); below ts, the first frame that comes out unchanged
        //    ends it: frame t reads only alive[t + 1] and best[t + 1], and alive changed in [ts, te] alone
        if (te + 1 < f1) {
            const int q0 = box_off[te + 1], m = box_off[te + 2] - q0;
            if (lane < m) s_best[1][lane] = best[q0 + lane];
        }
        __syncthreads();
        int cur = 0;
        for (int t = te; t >= f0; --t) {
            const int p0 = box_off[t], n = box_off[t + 1] - p0;
            const unsigned long long al = alive[t];
            const unsigned long long aln = t + 1 < f1 ? alive[t + 1] : 0ull;
            const bool me = lane < n && ((al >> lane) & 1ull);
            double b = 0.0;
            int changed = 0;
            if (me) {
                const double sc = (double)score[p0 + lane];
                unsigned long long m = link[p0 + lane] & aln;
                double mx = 0.0;
                int pb = -1;
                while (m) {                              // ascending b: the lowest b wins a tie
                    const int j = __builtin_ctzll(m);
                    m &= m - 1ull;
                    const double v = s_best[cur ^ 1][j];
                    if (pb < 0 || v > mx) mx = v, pb = j;
                }
                b = pb >= 0 ? sc + mx : sc;
                changed = (b != best[p0 + lane] || pb != ptr[p0 + lane]) ? 1 : 0;
                best[p0 + lane] = b;
                ptr[p0 + lane] = pb;
            }
            s_best[cur][lane] = b;
            double v = b;
            int vi = me ? lane : SQ_CAP;
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(v, o);
                const int oi = __shfl_xor(vi, o);
                if (oi < SQ_CAP && (vi == SQ_CAP || ov > v || (ov == v && oi < vi))) v = ov, vi = oi;
            }
            if (lane == 0) {
                fmax[t] = v;
                farg[t] = vi < SQ_CAP ? vi : -1;
            }
            const int any = __syncthreads_or(changed);   // also: s_best[cur] is written, s_best[cur ^ 1] has been read
            cur ^= 1;
            if (k > 0 && t < ts && !any) break;
        }
        // 2. the start: largest best, then lowest frame, then lowest box
        double v = 0.0;
        int vt = SQ_NONE;
        for (int f = f0 + lane; f < f1; f += SQ_CAP) {
            if (farg[f] >= 0) {
                const double x = fmax[f];
                if (vt == SQ_NONE || x > v) v = x, vt = f;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o);
            const int ot = __shfl_xor(vt, o);
            if (ot != SQ_NONE && (vt == SQ_NONE || ov > v || (ov == v && ot < vt))) v = ov, vt = ot;
        }
        if (vt == SQ_NONE) break;                        // nothing alive (every lane holds the same vt)
        // 3. the path: score sum in frame order, suppression per frame
        ts = vt;
        const int a0 = farg[ts];
        int a = a0, t = ts, len = 0;
        double sum = 0.0;
        float mxs = 0.0f;
        for (int step = 0; step < nf; ++step) {
            const int p0 = box_off[t], n = box_off[t + 1] - p0;
            if (a < 0 || a >= n) break;
            const float s = score[p0 + a];
            sum += (double)s;
            mxs = (len == 0 || s > mxs) ? s : mxs;
            ++len;
            te = t;
            const unsigned long long al = alive[t];
            bool kill = false;
            if (lane < n && ((al >> lane) & 1ull)) {
                if (lane == a) {
                    kill = true;
                } else {
                    double pa[4], pb[4];
                    sq_widen(box, (long long)p0 + a, pa);
                    sq_widen(box, (long long)p0 + lane, pb);
                    kill = i2v_overlap_plus1(pa, pb) > nms_iou;
                }
            }
            const unsigned long long word = __ballot(kill);
            const int nx = ptr[p0 + a];
            __syncthreads();                             // every lane has read alive[t]
            if (lane == 0) alive[t] = al & ~word;
            if (lane == a) tid[p0 + a] = k;
            if (nx < 0 || t + 1 >= f1) break;
            a = nx;
            ++t;
        }
        // 4. one new score for the path's boxes
        if (lane == 0) {
            const float ns = rescore == 1 ? mxs : (float)(sum / (double)len);
            int aa = a0;
            for (int i = 0, tt = ts; i < len; ++i, ++tt) {
                const int p0 = box_off[tt];
                new_score[p0 + aa] = ns;
                aa = ptr[p0 + aa];
            }
        }
        __syncthreads();                                 // alive is written before the next pass reads it
    }
    if (lane == 0) n_tracks[g] = k;
}

extern "C" size_t i2v_seqnms_workspace_bytes(int32_t n_groups, int32_t n_frames, int32_t n_boxes) {
    (void)n_groups;
    if (n_frames < 0 || n_boxes < 0) return I2V_STATUS_BYTES;
    const size_t N = (size_t)n_boxes, F = (size_t)n_frames;
    // status word; link, best, ptr per box; alive, fmax, farg per frame
    return I2V_STATUS_BYTES + i2v_align(8 * N) + i2v_align(8 * N) + i2v_align(4 * N) + i2v_align(8 * F) + i2v_align(8 * F) +
           i2v_align(4 * F);
}

extern "C" int32_t i2v_seqnms(const int32_t* group_off, const int32_t* frame_no, const int32_t* box_off, const float* box,
                              const float* score, int32_t n_groups, int32_t n_frames, int32_t n_boxes, double link_iou,
                              double nms_iou, int32_t rescore, int32_t* tid, float* new_score, int32_t* n_tracks, void* ws,
                              size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_groups >= 0 && n_frames >= 0 && n_boxes >= 0, "seqnms: negative count");
    I2V_CHECK_ARG(rescore == 0 || rescore == 1, "seqnms: rescore is 0 (avg) or 1 (max), got %d", rescore);
    I2V_CHECK_ARG(link_iou == link_iou && nms_iou == nms_iou, "seqnms: a threshold is not a number");
    I2V_CHECK_ARG(group_off && box_off, "seqnms: null pointer");
    I2V_CHECK_ARG(n_groups == 0 || n_tracks, "seqnms: null pointer");
    I2V_CHECK_ARG(n_frames == 0 || frame_no, "seqnms: null pointer");
    I2V_CHECK_ARG(n_boxes == 0 || (box && score && tid && new_score), "seqnms: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_seqnms_workspace_bytes(n_groups, n_frames, n_boxes), "seqnms: workspace too small");
    if (n_groups == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "seqnms: clearing the status word failed");
    const size_t N = (size_t)n_boxes, F = (size_t)n_frames;
    char* p = (char*)ws + I2V_STATUS_BYTES;
    unsigned long long* link = (unsigned long long*)p;  p += i2v_align(8 * N);
    double* best = (double*)p;                          p += i2v_align(8 * N);
    int* ptr = (int*)p;                                 p += i2v_align(4 * N);
    unsigned long long* alive = (unsigned long long*)p; p += i2v_align(8 * F);
    double* fmax = (double*)p;                          p += i2v_align(8 * F);
    int* farg = (int*)p;
    seqnms_kernel<<<n_groups, SQ_CAP, 0, st>>>(group_off, frame_no, box_off, box, score, n_frames, n_boxes, link_iou, nms_iou,
                                               rescore, link, best, ptr, alive, fmax, farg, tid, new_score, n_tracks, (int*)ws);
    I2V_CHECK_LAUNCH("seqnms");
    return I2V_OK;
}
