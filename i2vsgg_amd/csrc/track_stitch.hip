// Track stitching: the second step after Seq-NMS.  Tracklets (Seq-NMS tracks) of one group are joined across short runs of
// missed frames, the chain's boxes are rescored together and the boxes of the missed frames are interpolated.  The rules are
// stated once, in i2vsgg_amd/seqnms.py (stitch_arrays_host); the host form there and this kernel evaluate the same float64
// expressions in the same order on exactly widened float32 inputs (-ffp-contract=off -fno-fast-math), so they agree bit for
// bit.  No floating-point atomics: a chain's running sum travels with the chain's one box per slot, in frame order.
#include "table_common.h"

#define TS_CAP 64            // boxes of one slot: lane a is box a (seqnms.CAP)
#define TS_MAXGAP 7          // missing frame numbers a link may bridge (seqnms.MAX_STITCH_GAP)
#define TS_RING 8            // slots of history: frame numbers ascend strictly, so the candidates of a start box at frame number
                             // f -- end boxes at [f - max_gap - 1, f - 2] -- lie in the 8 slots before its own

// One workgroup of one wave per group (video, class), persistent over the group's slots in ascending order.  The last TS_RING
// slots live in LDS (r_*): per box its widened coordinates, Seq-NMS id, chain root (the global index of the chain's first
// box), the chain's running score sum / count / maximum up to and including this box, and r_free (1: a free end box, 2: an end
// box that has its successor, 0: neither, or not known yet -- a slot's end boxes are known when the next slot is read).
//   troot (N): per (group, Seq-NMS id) 0 = not seen, 1 = started and a root, 2 = started and linked to a predecessor;
//   newid (N): per (group, Seq-NMS id) the number of roots with a lower id;  root (N): per box its chain's root;
//   csum / ccnt / cmax (N): at a root's index the chain's sum, count and maximum so far (stores only: the running values are
//   read from the ring);  raw_* : per group a region of max_gap rows per box for the interpolated rows, n_fill (G) its fill.
__global__ void __launch_bounds__(TS_CAP)
track_stitch_kernel(const int* __restrict__ group_off, const int* __restrict__ frame_no, const int* __restrict__ box_off,
                    const float* __restrict__ box, const float* __restrict__ score, const int* __restrict__ tid, int n_frames,
                    int n_boxes, int max_gap, double stitch_iou, int rescore, int* troot, int* newid, int* root, double* csum,
                    int* ccnt, float* cmax, int* n_fill, int* raw_slot, int* raw_tid, float* raw_score, float* raw_box,
                    int* tid2, float* score2, int* n_tracks2, int* status) {
    __shared__ double r_box[TS_RING][TS_CAP][4];
    __shared__ double r_sum[TS_RING][TS_CAP];
    __shared__ int r_tid[TS_RING][TS_CAP], r_root[TS_RING][TS_CAP], r_cnt[TS_RING][TS_CAP], r_free[TS_RING][TS_CAP];
    __shared__ float r_max[TS_RING][TS_CAP];
    __shared__ double s_box[TS_CAP][4];                  // the slot's boxes
    __shared__ int s_tid[TS_CAP];                        // the slot's ids (-1: none)
    __shared__ int s_hit[TS_CAP];                        // box j of the previous slot goes on in this one
    __shared__ int s_order[TS_CAP];                      // the slot's start boxes in ascending id
    const int g = blockIdx.x, lane = threadIdx.x;
    const int f0 = group_off[g], f1 = group_off[g + 1];
    int bad = i2v_range_bad(f0, f1, n_frames) ? 1 : 0;
    if (!bad) {
        for (int f = f0 + lane; f < f1; f += TS_CAP) {
            const int p0 = box_off[f], n = box_off[f + 1] - p0;
            if (p0 < 0 || n < 0 || n > TS_CAP || (long long)p0 + n > n_boxes) bad = 1;
            if (f + 1 < f1 && frame_no[f + 1] <= frame_no[f]) bad = 1;       // the ring's bound rests on ascending numbers
        }
    }
    if (__syncthreads_or(bad)) {                         // a malformed table: say so, write nothing else
        if (lane == 0) {
            atomicMax(status, g + 1);
            n_tracks2[g] = 0;
            n_fill[g] = 0;
        }
        return;
    }
    const int nf = f1 - f0;
    const int gb0 = nf > 0 ? box_off[f0] : 0;            // every count is >= 0 and every end <= n_boxes
    const int nbox = nf > 0 ? box_off[f1] - gb0 : 0;
    const long long rb = (long long)max_gap * gb0;       // the group's region of new rows: max_gap per box (checked: int32)
    const long long rcap = (long long)max_gap * nbox;
    for (int i = lane; i < nbox; i += TS_CAP) troot[gb0 + i] = 0;
    for (int k = 0; k < TS_RING; ++k) {
        r_tid[k][lane] = -1;
        r_free[k][lane] = 0;
    }
    __syncthreads();                                     // troot and the ring are cleared

    int cursor = 0;                                      // new rows of the group so far (the same in every lane)
    for (int f = f0; f < f1; ++f) {
        const int p0 = box_off[f], n = box_off[f + 1] - p0, fno = frame_no[f];
        const int kc = (f - f0) & (TS_RING - 1), kp = (f - f0 - 1) & (TS_RING - 1);
        const bool follows = f > f0 && (long long)frame_no[f - 1] + 1 == (long long)fno;
        const int m = f > f0 ? p0 - box_off[f - 1] : 0;  // boxes of the previous slot
        // 0. the slot: ids, scores, widened boxes
        int t = -1;
        float sc = 0.0f;
        double b[4] = {0.0, 0.0, 0.0, 0.0};
        if (lane < n) {
            t = tid[p0 + lane];
            sc = score[p0 + lane];
            for (int c = 0; c < 4; ++c) b[c] = (double)box[(long long)(p0 + lane) * 4 + c];
            if (t < -1 || t >= nbox) bad = 1, t = -1;    // an id indexes troot: no such id comes from Seq-NMS
        }
        s_tid[lane] = t;
        s_hit[lane] = 0;
        for (int c = 0; c < 4; ++c) s_box[lane][c] = b[c];
        __syncthreads();                                 // (A) the slot's ids and boxes are written
        // 1. start boxes: no box of the id in the previous slot, or that slot is not the preceding frame number
        int pr = -1;
        if (t >= 0) {
            for (int j = 0; j < lane; ++j)
                if (s_tid[j] == t) bad = 1;              // an id twice in one slot
            if (follows)
                for (int j = 0; j < m; ++j)
                    if (r_tid[kp][j] == t) pr = j;       // at most one: the previous slot passed the test above
            if (pr >= 0) s_hit[pr] = 1;                  // ids of a slot are distinct: the word is this lane's alone
        }
        const bool start = t >= 0 && pr < 0;
        if (start && troot[gb0 + t] != 0) bad = 1;       // the id ran before: not one run of consecutive frame numbers
        if (__syncthreads_or(bad)) {                     // (B) s_hit is written; nothing of the group has left the workspace
            if (lane == 0) {
                atomicMax(status, g + 1);
                n_tracks2[g] = 0;
                n_fill[g] = 0;
            }
            return;
        }
        if (start) troot[gb0 + t] = 1;
        // 2. end boxes of the previous slot: the mirror image
        if (lane < m) r_free[kp][lane] = (r_tid[kp][lane] >= 0 && !s_hit[lane]) ? 1 : 0;
        // what the box inherits along its tracklet
        int my_root = p0 + lane, cnt = 0, linked = 0;
        double sum = 0.0;
        float mx = sc;
        if (pr >= 0) {
            my_root = r_root[kp][pr];
            sum = r_sum[kp][pr];
            cnt = r_cnt[kp][pr];
            mx = r_max[kp][pr];
        }
        const unsigned long long smask = __ballot(start);
        const int nstart = __popcll(smask);
        if (start) {
            int r = 0;
            for (int j = 0; j < n; ++j) r += (((smask >> j) & 1ull) && s_tid[j] < t) ? 1 : 0;
            s_order[r] = lane;
        }
        __syncthreads();                                 // (C) r_free of the previous slot and s_order are written
        // 3. every start box in ascending id takes the free end box of largest overlap (then smaller gap, then lower id)
        for (int r = 0; r < nstart; ++r) {
            const int bl = __builtin_amdgcn_readfirstlane(s_order[r]);
            double bb[4];
            for (int c = 0; c < 4; ++c) bb[c] = s_box[bl][c];
            double bo = -1.0;                            // this lane's best: overlap, end frame number, id, lane, slot
            int be = 0, bt = 0, bi = -1, bs = 0;
            for (int s = f - 1; s >= f0 && s >= f - TS_RING; --s) {     // descending end number: the smaller gap first
                const long long e = frame_no[s];
                if (e > (long long)fno - 2) continue;    // adjacent: Seq-NMS decided
                if (e < (long long)fno - max_gap - 1) break;
                const int ms = box_off[s + 1] - box_off[s], k = (s - f0) & (TS_RING - 1);
                if (lane < ms && r_free[k][lane] == 1) {
                    const double ov = i2v_overlap_plus1(r_box[k][lane], bb);
                    if (ov >= stitch_iou && (bi < 0 || ov > bo)) bo = ov, be = (int)e, bt = r_tid[k][lane], bi = lane, bs = s;
                }
            }
            for (int o = 32; o > 0; o >>= 1) {           // (overlap, end number, id) is a strict order: every lane ends equal
                const double oo = __shfl_xor(bo, o);
                const int oe = __shfl_xor(be, o), ot = __shfl_xor(bt, o), oi = __shfl_xor(bi, o), os = __shfl_xor(bs, o);
                if (oi >= 0 && (bi < 0 || oo > bo || (oo == bo && (oe > be || (oe == be && ot < bt)))))
                    bo = oo, be = oe, bt = ot, bi = oi, bs = os;
            }
            const int k = (bs - f0) & (TS_RING - 1);
            if (bi >= 0) {
                // 4. the link's rows: the slots strictly between, at most max_gap of them
                const int rows = f - 1 - bs;
                if (lane < rows && (long long)cursor + lane < rcap) {
                    const int s = bs + 1 + lane;
                    const double w = (double)(frame_no[s] - be) / (double)(fno - be);
                    const long long row = rb + cursor + lane;
                    raw_slot[row] = s;
                    raw_tid[row] = r_root[k][bi];        // the root for now: the new id is known after the last slot
                    for (int c = 0; c < 4; ++c) raw_box[row * 4 + c] = (float)(r_box[k][bi][c] + (bb[c] - r_box[k][bi][c]) * w);
                }
                cursor += rows;
                if (lane == bl) {                        // B's tracklet inherits A's root and running score
                    my_root = r_root[k][bi];
                    sum = r_sum[k][bi];
                    cnt = r_cnt[k][bi];
                    mx = r_max[k][bi];
                    linked = 1;
                }
            }
            __syncthreads();                             // (D1) every lane has read r_free
            if (bi >= 0 && lane == 0) r_free[k][bi] = 2; // claimed: first come, first served
            __syncthreads();                             // (D2) the claim is written before the next start box looks
        }
        // 5. the box's own score joins its chain: one lane per chain and slot, frame order by construction
        if (t >= 0) {
            sum = sum + (double)sc;
            cnt += 1;
            mx = sc > mx ? sc : mx;
            root[p0 + lane] = my_root;
            csum[my_root] = sum;
            ccnt[my_root] = cnt;
            cmax[my_root] = mx;
            if (linked) troot[gb0 + t] = 2;
        }
        // the slot enters the ring in the place of slot f - 8, which no later slot can reach (read last before C / D2)
        r_tid[kc][lane] = t;
        r_root[kc][lane] = my_root;
        r_sum[kc][lane] = sum;
        r_cnt[kc][lane] = cnt;
        r_max[kc][lane] = mx;
        r_free[kc][lane] = 0;
        for (int c = 0; c < 4; ++c) r_box[kc][lane][c] = b[c];
        __syncthreads();                                 // (E) the ring holds the slot; this slot's global stores are done
    }

    // dense ids: the number of roots with a lower Seq-NMS id
    int running = 0;
    for (int base = 0; base < nbox; base += TS_CAP) {
        const int i = base + lane;
        const unsigned long long mask = __ballot(i < nbox && troot[gb0 + i] == 1);
        if (i < nbox) newid[gb0 + i] = running + __popcll(mask & ((1ull << lane) - 1ull));
        running += __popcll(mask);
    }
    __syncthreads();                                     // newid is written
    for (int i = gb0 + lane; i < gb0 + nbox; i += TS_CAP) {
        const int t = tid[i];
        if (t >= 0) {
            const int r = root[i];
            tid2[i] = newid[gb0 + tid[r]];
            score2[i] = rescore == 1 ? cmax[r] : (float)(csum[r] / (double)ccnt[r]);
        } else {
            tid2[i] = -1;
            score2[i] = score[i];
        }
    }
    for (long long j = rb + lane; j < rb + cursor && j < rb + rcap; j += TS_CAP) {
        const int r = raw_tid[j];
        raw_tid[j] = newid[gb0 + tid[r]];
        raw_score[j] = rescore == 1 ? cmax[r] : (float)(csum[r] / (double)ccnt[r]);
    }
    if (lane == 0) {
        n_tracks2[g] = running;
        n_fill[g] = cursor < rcap ? cursor : (int)rcap;
    }
}

// fill_off (G + 1): the exclusive scan of n_fill, one wave, 64 groups per step
__global__ void __launch_bounds__(64) track_stitch_offsets_kernel(const int* __restrict__ n_fill, int n_groups, int* __restrict__ fill_off) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n_groups; base += 64) {
        const int i = base + lane;
        const int v = i < n_groups ? n_fill[i] : 0;
        int incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (i < n_groups) fill_off[i] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) fill_off[n_groups] = carry;
}

// the groups' regions, compacted into fill_off order
__global__ void __launch_bounds__(64)
track_stitch_compact_kernel(const int* __restrict__ group_off, const int* __restrict__ box_off, const int* __restrict__ n_fill,
                            const int* __restrict__ fill_off, int max_gap, const int* __restrict__ raw_slot,
                            const int* __restrict__ raw_tid, const float* __restrict__ raw_score, const float* __restrict__ raw_box,
                            int* __restrict__ fill_slot, int* __restrict__ fill_tid, float* __restrict__ fill_box,
                            float* __restrict__ fill_score) {
    const int g = blockIdx.x, n = n_fill[g];
    if (n <= 0) return;                                  // also every malformed group: its offsets are not read
    const long long rb = (long long)max_gap * box_off[group_off[g]], dst = fill_off[g];
    for (int j = threadIdx.x; j < n; j += 64) {
        fill_slot[dst + j] = raw_slot[rb + j];
        fill_tid[dst + j] = raw_tid[rb + j];
        fill_score[dst + j] = raw_score[rb + j];
        for (int c = 0; c < 4; ++c) fill_box[(dst + j) * 4 + c] = raw_box[(rb + j) * 4 + c];
    }
}

extern "C" size_t i2v_track_stitch_workspace_bytes(int32_t n_groups, int32_t n_frames, int32_t n_boxes, int32_t max_gap) {
    (void)n_frames;
    if (n_groups < 0 || n_boxes < 0 || max_gap < 1 || max_gap > TS_MAXGAP) return I2V_STATUS_BYTES;
    const size_t N = (size_t)n_boxes, G = (size_t)n_groups, R = (size_t)max_gap * N;
    // status word; troot, newid, root, ccnt, cmax (4 N each), csum (8 N); n_fill; raw_slot, raw_tid, raw_score, raw_box
    return I2V_STATUS_BYTES + 5 * i2v_align(4 * N) + i2v_align(8 * N) + i2v_align(4 * G) + 3 * i2v_align(4 * R) + i2v_align(16 * R);
}

extern "C" int32_t i2v_track_stitch(const int32_t* group_off, const int32_t* frame_no, const int32_t* box_off, const float* box,
                                    const float* score, const int32_t* tid, int32_t n_groups, int32_t n_frames, int32_t n_boxes,
                                    int32_t max_gap, double stitch_iou, int32_t rescore, int32_t* tid2, float* score2,
                                    int32_t* n_tracks2, int32_t* fill_off, int32_t* fill_slot, int32_t* fill_tid, float* fill_box,
                                    float* fill_score, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_groups >= 0 && n_frames >= 0 && n_boxes >= 0, "track_stitch: negative count");
    I2V_CHECK_ARG(max_gap >= 1 && max_gap <= TS_MAXGAP, "track_stitch: max_gap lies in [1, %d] (got %d)", TS_MAXGAP, max_gap);
    I2V_CHECK_ARG(rescore == 0 || rescore == 1, "track_stitch: rescore is 0 (avg) or 1 (max), got %d", rescore);
    I2V_CHECK_ARG(stitch_iou == stitch_iou, "track_stitch: the threshold is not a number");
    I2V_CHECK_ARG((long long)max_gap * n_boxes <= 0x7fffffffLL, "track_stitch: max_gap * n_boxes does not fit int32");
    I2V_CHECK_ARG(group_off && box_off && fill_off, "track_stitch: null pointer");
    I2V_CHECK_ARG(n_groups == 0 || n_tracks2, "track_stitch: null pointer");
    I2V_CHECK_ARG(n_frames == 0 || frame_no, "track_stitch: null pointer");
    I2V_CHECK_ARG(n_boxes == 0 || (box && score && tid && tid2 && score2 && fill_slot && fill_tid && fill_box && fill_score),
                  "track_stitch: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_track_stitch_workspace_bytes(n_groups, n_frames, n_boxes, max_gap),
                  "track_stitch: workspace too small");
    if (n_groups == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "track_stitch: clearing the status word failed");
    const size_t N = (size_t)n_boxes, G = (size_t)n_groups, R = (size_t)max_gap * N;
    char* p = (char*)ws + I2V_STATUS_BYTES;
    int* troot = (int*)p;       p += i2v_align(4 * N);
    int* newid = (int*)p;       p += i2v_align(4 * N);
    int* root = (int*)p;        p += i2v_align(4 * N);
    int* ccnt = (int*)p;        p += i2v_align(4 * N);
    float* cmax = (float*)p;    p += i2v_align(4 * N);
    double* csum = (double*)p;  p += i2v_align(8 * N);
    int* n_fill = (int*)p;      p += i2v_align(4 * G);
    int* raw_slot = (int*)p;    p += i2v_align(4 * R);
    int* raw_tid = (int*)p;     p += i2v_align(4 * R);
    float* raw_score = (float*)p; p += i2v_align(4 * R);
    float* raw_box = (float*)p;
    track_stitch_kernel<<<n_groups, TS_CAP, 0, st>>>(group_off, frame_no, box_off, box, score, tid, n_frames, n_boxes, max_gap,
                                                     stitch_iou, rescore, troot, newid, root, csum, ccnt, cmax, n_fill, raw_slot,
                                                     raw_tid, raw_score, raw_box, tid2, score2, n_tracks2, (int*)ws);
    I2V_CHECK_LAUNCH("track_stitch");
    track_stitch_offsets_kernel<<<1, 64, 0, st>>>(n_fill, n_groups, fill_off);
    I2V_CHECK_LAUNCH("track_stitch (offsets)");
    track_stitch_compact_kernel<<<n_groups, 64, 0, st>>>(group_off, box_off, n_fill, fill_off, max_gap, raw_slot, raw_tid, raw_score,
                                                         raw_box, fill_slot, fill_tid, fill_box, fill_score);
    I2V_CHECK_LAUNCH("track_stitch (compact)");
    return I2V_OK;
}
