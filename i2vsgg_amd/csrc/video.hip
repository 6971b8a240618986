// Video level of the relation test loop: frame-to-video association of per-frame triplets and the trajectory overlap /
// matching of the VidVRD detection metric (lib/utils.py: greedy_relational_association, viou, eval_detection_scores).
// All arithmetic that decides something is float64 in the reference's operation order (the library is built with
// -ffp-contract=off -fno-fast-math, so every + - * / rounds once, like the CPU's).  No floating-point atomics; every
// reduction has a fixed order, so two runs give the same bits.
#include "table_common.h"

#define VA_MAXP 100          // predictions of one frame that take part (max_traj_num_in_clip)
#define VA_THREADS 256       // thread (p, h) = (t & 127, t >> 7): prediction p against the ranked candidates 64h .. 64h+63
#define VM_MAXP 200          // predicted relations of one video (max_num_per_video)
#define VM_MAXG 4096         // ground-truth relations of one video (64 lanes x 64 "detected" bits)
#define VM_COLS 10           // relation row: video, s_cid, pid, o_cid, fstart, fend, sub_off, sub_len, obj_off, obj_len

// ---------------------------------------------------------------------------------------------------------------------
// Association
// ---------------------------------------------------------------------------------------------------------------------

// lib/utils.py:20-32 in its own operation order (no +1; empty or touching intersection: 0): not i2v_overlap_plus1's arithmetic
__device__ __forceinline__ double va_iou(const double* a, const double* b) {
    const double left = a[0] > b[0] ? a[0] : b[0];
    const double right = a[2] < b[2] ? a[2] : b[2];
    const double up = a[1] > b[1] ? a[1] : b[1];
    const double down = a[3] < b[3] ? a[3] : b[3];
    if (left >= right || down <= up) return 0.0;
    const double s1 = (a[2] - a[0]) * (a[3] - a[1]);
    const double s2 = (b[2] - b[0]) * (b[3] - b[1]);
    const double sc = (down - up) * (right - left);
    return sc / (s1 + s2 - sc);
}

// One frame's predictions in descending score order.  After the frame they ARE the open relations of the next frame: entry
// j is the relation that prediction j joined or opened (its last boxes are j's boxes, its triplet is j's triplet).
struct VaFrame {
    double score[VA_MAXP];
    double sum[VA_MAXP];         // the relation's running sum of scores, in member order
    double box[VA_MAXP][8];      // subject box, object box
    int trip[VA_MAXP][3];
    int cnt[VA_MAXP];
    int id[VA_MAXP];             // relation id within the video (creation order)
    int src[VA_MAXP];            // position of the prediction in the caller's frame list
};

// One workgroup per video, persistent over its frames.
__global__ void __launch_bounds__(VA_THREADS)
video_associate_kernel(const int* __restrict__ frame_off, const int* __restrict__ frame_no, const int* __restrict__ pred_off,
                       const double* __restrict__ score, const int* __restrict__ trip, const double* __restrict__ boxes,
                       int n_frames, int n_preds, int max_per_frame, int* __restrict__ rel_id, int* __restrict__ rel_start,
                       int* __restrict__ rel_len, double* __restrict__ rel_score, int* __restrict__ n_rel, int* status) {
    __shared__ VaFrame fr[2];
    __shared__ double s_key[VA_MAXP];                    // the frame's scores as given, then the open relations' means
    __shared__ int s_order[2 * 64];                      // candidate rank -> entry of the previous frame
    __shared__ unsigned long long s_compat[VA_MAXP][2];  // prediction p may extend the candidate of rank r: bit r
    __shared__ int s_assign[VA_MAXP];                    // entry of the previous frame it extends, or ~(new relation id)
    __shared__ int s_next;
    const int v = blockIdx.x, t = threadIdx.x;
    int f0 = frame_off[v], f1 = frame_off[v + 1];
    if (i2v_range_bad(f0, f1, n_frames)) {               // a malformed table: say so, touch nothing
        if (t == 0) {
            atomicMax(status, n_frames + 1);
            n_rel[v] = 0;
        }
        return;
    }
    int base = 0;                                        // the video's relations live at [base, base + its predictions)
    int next = 0, m = 0, prev_no = 0, cur = 0;
    for (int f = f0; f < f1; ++f) {
        int p0 = pred_off[f];
        int n = pred_off[f + 1] - p0;
        if (n > max_per_frame || n > VA_MAXP || i2v_span_bad(p0, n, n_preds)) {
            if (t == 0) atomicMax(status, f + 1);        // the frame is skipped as if empty; the caller reads the status
            n = 0;
            p0 = 0;
        }
        if (f == f0) base = p0;
        const int fno = frame_no[f];
        if (f == f0 || fno != prev_no + 1) m = 0;        // every open relation ends at prev_no + 1: a gap closes them all
        VaFrame& C = fr[cur];
        const VaFrame& P = fr[cur ^ 1];
        // 1. the frame's predictions, in descending score (stable)
        if (t < n) s_key[t] = score[p0 + t];
        __syncthreads();
        if (t < n) {
            const int r = i2v_rank_desc(s_key, n, t);
            C.score[r] = s_key[t];
            C.src[r] = t;
            for (int k = 0; k < 3; ++k) C.trip[r][k] = trip[(size_t)(p0 + t) * 3 + k];
            for (int k = 0; k < 8; ++k) C.box[r][k] = boxes[(size_t)(p0 + t) * 8 + k];
        }
        __syncthreads();                                 // s_key has been read by every rank
        // 2. the open relations by their current mean, descending, stable in the order the last frame touched them
        if (t < m) s_key[t] = P.sum[t] / (double)P.cnt[t];
        __syncthreads();
        if (t < m) s_order[i2v_rank_desc(s_key, m, t)] = t;
        __syncthreads();
        // 3. compatibility of every prediction with every candidate: equal triplet, both boxes IoU >= 0.5
        {
            const int p = t & 127, h = t >> 7;
            if (p < n) {
                unsigned long long mask = 0;
                const int r1 = m < 64 * h + 64 ? m : 64 * h + 64;
                for (int r = 64 * h; r < r1; ++r) {
                    const int j = s_order[r];
                    if (P.trip[j][0] == C.trip[p][0] && P.trip[j][1] == C.trip[p][1] && P.trip[j][2] == C.trip[p][2]) {
                        if (va_iou(&P.box[j][0], &C.box[p][0]) >= 0.5 && va_iou(&P.box[j][4], &C.box[p][4]) >= 0.5)
                            mask |= 1ull << (r - 64 * h);
                    }
                }
                s_compat[p][h] = mask;
            }
        }
        __syncthreads();
        // 4. the greedy pick: a candidate serves one prediction per frame, the best-ranked compatible one wins
        if (t == 0) {
            unsigned long long a0 = ~0ull, a1 = ~0ull;
            int nx = next;
            for (int p = 0; p < n; ++p) {
                const unsigned long long c0 = s_compat[p][0] & a0, c1 = s_compat[p][1] & a1;
                if (c0) {
                    const int r = __builtin_ctzll(c0);
                    a0 &= ~(1ull << r);
                    s_assign[p] = s_order[r];
                } else if (c1) {
                    const int r = __builtin_ctzll(c1);
                    a1 &= ~(1ull << r);
                    s_assign[p] = s_order[64 + r];
                } else {
                    s_assign[p] = ~nx;
                    ++nx;
                }
            }
            s_next = nx;
        }
        __syncthreads();
        // 5. extend or open; this frame's entries become the next frame's open relations
        if (t < n) {
            const int a = s_assign[t];
            int id, cnt;
            double sum;
            if (a >= 0) {
                id = P.id[a];
                cnt = P.cnt[a] + 1;
                sum = P.sum[a] + C.score[t];
            } else {
                id = ~a;
                cnt = 1;
                sum = C.score[t];
            }
            C.id[t] = id;
            C.cnt[t] = cnt;
            C.sum[t] = sum;
            if (base + id < n_preds) {                   // id < predictions seen so far in this video
                if (a < 0) rel_start[base + id] = fno;
                rel_len[base + id] = cnt;
                rel_score[base + id] = sum / (double)cnt;
            }
            rel_id[p0 + C.src[t]] = id;
        }
        next = s_next;
        __syncthreads();                                 // s_next, s_assign and P are free for the next frame
        m = n;
        prev_no = fno;
        cur ^= 1;
    }
    if (t == 0) n_rel[v] = next;
}

extern "C" size_t i2v_video_associate_workspace_bytes(int32_t n_videos, int32_t n_frames, int32_t n_preds) {
    (void)n_videos; (void)n_frames; (void)n_preds;
    return I2V_STATUS_BYTES;                             // the status word
}

extern "C" int32_t i2v_video_associate(const int32_t* frame_off, const int32_t* frame_no, const int32_t* pred_off,
                                       const double* score, const int32_t* triplet, const double* boxes,
                                       int32_t n_videos, int32_t n_frames, int32_t n_preds, int32_t max_per_frame,
                                       int32_t* rel_id, int32_t* rel_start, int32_t* rel_len, double* rel_score,
                                       int32_t* n_rel, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_videos >= 0 && n_frames >= 0 && n_preds >= 0, "video_associate: negative count");
    I2V_CHECK_ARG(max_per_frame >= 0 && max_per_frame <= VA_MAXP,
                  "video_associate: at most %d predictions of a frame take part (got %d): cut each frame's list first", VA_MAXP,
                  max_per_frame);
    I2V_CHECK_ARG(frame_off && pred_off && (n_frames == 0 || frame_no) && (n_videos == 0 || n_rel), "video_associate: null pointer");
    I2V_CHECK_ARG(n_preds == 0 || (score && triplet && boxes && rel_id && rel_start && rel_len && rel_score),
                  "video_associate: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_video_associate_workspace_bytes(n_videos, n_frames, n_preds),
                  "video_associate: workspace too small");
    if (n_videos == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "video_associate: clearing the status word failed");
    video_associate_kernel<<<n_videos, VA_THREADS, 0, st>>>(frame_off, frame_no, pred_off, score, triplet, boxes, n_frames,
                                                            n_preds, max_per_frame, rel_id, rel_start, rel_len, rel_score,
                                                            n_rel, (int*)ws);
    I2V_CHECK_LAUNCH("video_associate");
    return I2V_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Association along object tracks (the rules: i2vsgg_amd/video.py, associate_tracks)
// ---------------------------------------------------------------------------------------------------------------------

#define VT_MAXGAP 7                          // frames a relation may stay out of its frames' lists and still go on
#define VT_CAP (VA_MAXP * (VT_MAXGAP + 1))   // open relations: last member within max_gap + 1 frame numbers, 100 per frame
#define VT_PER 4                             // entries a thread moves when the table is compacted: 256 x 4 >= VT_CAP

// One workgroup per video, persistent over its frames.  The open table holds at most one relation per key (a prediction
// that opens a relation replaces the open one of its key), so a prediction has at most one entry to look at and the
// table's order decides nothing.  Per frame: rank the predictions; find each one's entry; extend it in place or open a
// relation; drop the entries no later frame can reach, stably; append the relations whose key had no entry.
__global__ void __launch_bounds__(VA_THREADS)
video_associate_tracks_kernel(const int* __restrict__ frame_off, const int* __restrict__ frame_no, const int* __restrict__ pred_off,
                              const double* __restrict__ score, const int* __restrict__ key, const int* __restrict__ since,
                              int n_frames, int n_preds, int max_gap, int* __restrict__ rel_id, int* __restrict__ rel_start,
                              int* __restrict__ rel_end, int* __restrict__ rel_len, double* __restrict__ rel_score,
                              int* __restrict__ n_rel, int* status) {
    __shared__ double o_sum[VT_CAP];                     // the open relations: running sum of scores in member order,
    __shared__ int o_key[3][VT_CAP];                     // key (subject object index, predicate, object object index),
    __shared__ int o_last[VT_CAP], o_cnt[VT_CAP], o_id[VT_CAP];      // last member frame number, members, id
    __shared__ double s_key[VA_MAXP];                    // the frame's scores as given
    __shared__ double c_score[VA_MAXP];                  // the frame in descending score (stable)
    __shared__ int c_key[VA_MAXP][3], c_since[VA_MAXP], c_src[VA_MAXP];
    __shared__ int s_found[VA_MAXP][2];                  // the entry of the prediction's key in either half of the table, or -1
    __shared__ int s_new[VA_MAXP], s_app[VA_MAXP];       // the prediction opens a relation / its key has no entry
    __shared__ int s_wsum[VA_THREADS / 64];
    __shared__ int s_dup;
    const int v = blockIdx.x, t = threadIdx.x;
    const int f0 = frame_off[v], f1 = frame_off[v + 1];
    if (i2v_range_bad(f0, f1, n_frames)) {               // a malformed table: say so, touch nothing
        if (t == 0) {
            atomicMax(status, n_frames + 1);
            n_rel[v] = 0;
        }
        return;
    }
    int base = 0;                                        // the video's relations live at [base, base + its predictions)
    int next = 0, m = 0, prev_no = 0;
    bool any = false;                                    // a frame number has been taken
    for (int f = f0; f < f1; ++f) {
        int p0 = pred_off[f];
        int n = pred_off[f + 1] - p0;
        const int fno = frame_no[f];
        bool bad = n > VA_MAXP || i2v_span_bad(p0, n, n_preds);
        if (bad) p0 = 0;
        if (f == f0) base = p0;
        if (any && fno <= prev_no) bad = true;           // frame numbers ascend strictly: the bound of the table rests on it
        if (bad) n = 0;
        // 1. the frame's predictions, in descending score (stable)
        if (t == 0) s_dup = 0;
        if (t < n) s_key[t] = score[p0 + t];
        __syncthreads();
        if (t < n) {
            const int r = i2v_rank_desc(s_key, n, t);
            c_score[r] = s_key[t];
            c_src[r] = t;
            for (int k = 0; k < 3; ++k) c_key[r][k] = key[(size_t)(p0 + t) * 3 + k];
            c_since[r] = since[p0 + t];
        }
        __syncthreads();                                 // the ranked frame is written
        if (t < n) {
            for (int j = 0; j < t; ++j)
                if (c_key[j][0] == c_key[t][0] && c_key[j][1] == c_key[t][1] && c_key[j][2] == c_key[t][2]) s_dup = 1;
        }
        __syncthreads();
        if (s_dup) {                                     // a repeated key: no such frame comes from the packer
            bad = true;
            n = 0;
        }
        if (bad && t == 0) atomicMax(status, f + 1);     // the frame is skipped as if empty; the caller reads the status
        // 2. the entry of every prediction's key: thread (p, h) looks through half h of the table
        {
            const int p = t & 127, h = t >> 7;
            if (p < n) {
                const int half = (m + 1) >> 1;
                const int e1 = m < (h + 1) * half ? m : (h + 1) * half;
                const int k0 = c_key[p][0], k1 = c_key[p][1], k2 = c_key[p][2];
                int found = -1;
                for (int e = h * half; e < e1; ++e)
                    if (o_key[0][e] == k0 && o_key[1][e] == k1 && o_key[2][e] == k2) found = e;       // at most one
                s_found[p][h] = found;
            }
        }
        __syncthreads();                                 // matches found
        // 3. extend or open
        int e = -1;
        bool ext = false;
        if (t < n) {
            e = s_found[t][0] >= 0 ? s_found[t][0] : s_found[t][1];
            if (e >= 0) {
                const long long d = (long long)fno - o_last[e];
                ext = d >= 1 && d <= (long long)max_gap + 1 && c_since[t] <= o_last[e];
            }
            s_new[t] = ext ? 0 : 1;
            s_app[t] = e < 0 ? 1 : 0;
        }
        __syncthreads();
        int n_new = 0, n_app = 0, my_new = 0, my_app = 0;   // new relations take ids in ranked order
        for (int q = 0; q < n; ++q) {
            if (q == t) my_new = n_new, my_app = n_app;
            n_new += s_new[q];
            n_app += s_app[q];
        }
        int id = 0, cnt = 1;
        double sum = 0.0;
        if (t < n) {
            sum = c_score[t];
            if (ext) {
                id = o_id[e];
                cnt = o_cnt[e] + 1;
                sum = o_sum[e] + c_score[t];
            } else {
                id = next + my_new;
            }
            if (e >= 0) {                                // keys of a frame are distinct: the entry is this thread's alone
                o_id[e] = id;
                o_cnt[e] = cnt;
                o_sum[e] = sum;
                o_last[e] = fno;
            }
            if ((long long)base + id < n_preds) {        // id < predictions seen so far in this video
                if (!ext) rel_start[base + id] = fno;
                rel_end[base + id] = fno + 1;
                rel_len[base + id] = cnt;
                rel_score[base + id] = sum / (double)cnt;
            }
            rel_id[p0 + c_src[t]] = id;
        }
        next += n_new;
        __syncthreads();                                 // the table is updated in place
        // 4. drop what no later frame can reach (the next frame number is at least fno + 1), keeping the order
        int kept = 0;
        int q_key[VT_PER][3], q_last[VT_PER], q_cnt[VT_PER], q_id[VT_PER];
        double q_sum[VT_PER];
        unsigned keep = 0;                               // bit i: entry t * VT_PER + i stays
        if (!bad) {
#pragma unroll
            for (int i = 0; i < VT_PER; ++i) {
                const int s = t * VT_PER + i;
                if (s < m && (long long)o_last[s] >= (long long)fno - max_gap) {
                    q_key[i][0] = o_key[0][s], q_key[i][1] = o_key[1][s], q_key[i][2] = o_key[2][s];
                    q_last[i] = o_last[s], q_cnt[i] = o_cnt[s], q_id[i] = o_id[s];
                    q_sum[i] = o_sum[s];
                    keep |= 1u << i;
                    ++kept;
                }
            }
        }
        int incl = kept;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if ((t & 63) >= o) incl += y;
        }
        if ((t & 63) == 63) s_wsum[t >> 6] = incl;
        __syncthreads();                                 // every kept entry is in a register: the table may be overwritten
        if (!bad) {
            int dst = incl - kept, total = 0;
            for (int w = 0; w < VA_THREADS / 64; ++w) {
                if (w < (t >> 6)) dst += s_wsum[w];
                total += s_wsum[w];
            }
#pragma unroll
            for (int i = 0; i < VT_PER; ++i) {
                if (!((keep >> i) & 1u)) continue;
                const int s = dst++;                     // dst <= t * VT_PER + i: never past what was read
                o_key[0][s] = q_key[i][0], o_key[1][s] = q_key[i][1], o_key[2][s] = q_key[i][2];
                o_last[s] = q_last[i], o_cnt[s] = q_cnt[i], o_id[s] = q_id[i];
                o_sum[s] = q_sum[i];
            }
            if (t < n && e < 0) {                        // 5. the relations whose key had no entry
                const int s = total + my_app;
                if (s < VT_CAP) {
                    o_key[0][s] = c_key[t][0], o_key[1][s] = c_key[t][1], o_key[2][s] = c_key[t][2];
                    o_last[s] = fno, o_cnt[s] = 1, o_id[s] = id;
                    o_sum[s] = sum;
                } else {
                    atomicMax(status, f + 1);            // past the bound that ascending frame numbers give: not reached
                }
            }
            m = total + n_app < VT_CAP ? total + n_app : VT_CAP;
            prev_no = fno;
            any = true;
        }
        __syncthreads();                                 // the table is compacted; the frame's arrays are free
    }
    if (t == 0) n_rel[v] = next;
}

extern "C" size_t i2v_video_associate_tracks_workspace_bytes(int32_t n_videos, int32_t n_frames, int32_t n_preds) {
    (void)n_videos; (void)n_frames; (void)n_preds;
    return I2V_STATUS_BYTES;                             // the status word
}

extern "C" int32_t i2v_video_associate_tracks(const int32_t* frame_off, const int32_t* frame_no, const int32_t* pred_off,
                                              const double* score, const int32_t* key, const int32_t* since,
                                              int32_t n_videos, int32_t n_frames, int32_t n_preds, int32_t max_gap,
                                              int32_t* rel_id, int32_t* rel_start, int32_t* rel_end, int32_t* rel_len,
                                              double* rel_score, int32_t* n_rel, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_videos >= 0 && n_frames >= 0 && n_preds >= 0, "video_associate_tracks: negative count");
    I2V_CHECK_ARG(max_gap >= 0 && max_gap <= VT_MAXGAP, "video_associate_tracks: max_gap lies in [0, %d] (got %d)", VT_MAXGAP,
                  max_gap);
    I2V_CHECK_ARG(frame_off && pred_off && (n_frames == 0 || frame_no) && (n_videos == 0 || n_rel),
                  "video_associate_tracks: null pointer");
    I2V_CHECK_ARG(n_preds == 0 || (score && key && since && rel_id && rel_start && rel_end && rel_len && rel_score),
                  "video_associate_tracks: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_video_associate_tracks_workspace_bytes(n_videos, n_frames, n_preds),
                  "video_associate_tracks: workspace too small");
    if (n_videos == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 4, st, "video_associate_tracks: clearing the status word failed");
    video_associate_tracks_kernel<<<n_videos, VA_THREADS, 0, st>>>(frame_off, frame_no, pred_off, score, key, since, n_frames,
                                                                   n_preds, max_gap, rel_id, rel_start, rel_end, rel_len, rel_score,
                                                                   n_rel, (int*)ws);
    I2V_CHECK_LAUNCH("video_associate_tracks");
    return I2V_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Trajectory overlap (viou) and the greedy matching of eval_detection_scores
// ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double vm_wave_sum(double x) {       // fixed butterfly: every lane ends with the same bits
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// clamp a trajectory (off, len) to the box array
__device__ __forceinline__ void vm_span(const int* row, int which, long long n_boxes, long long& off, int& len) {
    off = row[6 + 2 * which];
    len = row[7 + 2 * which];
    if (off < 0 || len < 0 || off + len > n_boxes) len = 0, off = 0;
}

// one wave per trajectory: the +1 pixel volume over the WHOLE trajectory (viou's v1 / v2)
__global__ void __launch_bounds__(256)
video_volume_kernel(const int* __restrict__ pred_rel, const int* __restrict__ gt_rel, const double* __restrict__ boxes,
                    int n_pred, int n_gt, long long n_boxes, double* __restrict__ vol) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= 2ll * (n_pred + n_gt)) return;
    const int r = (int)(w >> 1), which = (int)(w & 1);
    const int* row = r < n_pred ? pred_rel + (size_t)r * VM_COLS : gt_rel + (size_t)(r - n_pred) * VM_COLS;
    long long off;
    int len;
    vm_span(row, which, n_boxes, off, len);
    double acc = 0.0;
    for (int i = lane; i < len; i += 64) {
        const double* b = boxes + (size_t)(off + i) * 4;
        acc += (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0);
    }
    acc = vm_wave_sum(acc);
    if (lane == 0) vol[w] = acc;
}

// lib/utils.py:221-262 for one trajectory pair; the whole wave calls it
__device__ double vm_viou(const int* pr, const int* gr, int which, const double* __restrict__ boxes, long long n_boxes,
                          double v1, double v2, int lane) {
    const int a0 = pr[4], a1 = pr[5], b0 = gr[4], b1 = gr[5];
    if (a0 >= b1 || a1 <= b0) return 0.0;
    const int lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    long long off1, off2;
    int len1, len2;
    vm_span(pr, which, n_boxes, off1, len1);
    vm_span(gr, which, n_boxes, off2, len2);
    const int h1 = lo - a0, h2 = lo - b0;
    int cnt = hi - lo;
    if (cnt > len1 - h1) cnt = len1 - h1;
    if (cnt > len2 - h2) cnt = len2 - h2;
    double acc = 0.0;
    for (int i = lane; i < cnt; i += 64) {
        const double* x = boxes + (size_t)(off1 + h1 + i) * 4;
        const double* y = boxes + (size_t)(off2 + h2 + i) * 4;
        const double left = x[0] > y[0] ? x[0] : y[0];
        const double top = x[1] > y[1] ? x[1] : y[1];
        const double right = x[2] < y[2] ? x[2] : y[2];
        const double bottom = x[3] < y[3] ? x[3] : y[3];
        const double w = right - left + 1.0, h = bottom - top + 1.0;
        acc += (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
    }
    acc = vm_wave_sum(acc);
    return acc / (v1 + v2 - acc);
}

// one wave per (prediction, ground-truth slot): ov = min(subject viou, object viou), -1 where the triplets differ or the
// video has no such ground truth (those waves leave at once)
__global__ void __launch_bounds__(256)
video_viou_kernel(const int* __restrict__ pred_rel, const int* __restrict__ gt_off, const int* __restrict__ gt_rel,
                  const double* __restrict__ boxes, const double* __restrict__ vol, int n_videos, int n_pred, int n_gt,
                  long long n_boxes, int max_gt, double* __restrict__ ov) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)n_pred * max_gt) return;
    const int p = (int)(w / max_gt), g = (int)(w % max_gt);
    const int* pr = pred_rel + (size_t)p * VM_COLS;
    double out = -1.0;
    const int v = pr[0];
    if (v >= 0 && v < n_videos) {
        const int g0 = gt_off[v], ng = gt_off[v + 1] - g0;
        if (g0 >= 0 && g < ng && (long long)g0 + ng <= n_gt) {
            const int* gr = gt_rel + (size_t)(g0 + g) * VM_COLS;
            if (pr[1] == gr[1] && pr[2] == gr[2] && pr[3] == gr[3]) {
                const double* vp = vol + 2 * (size_t)p;
                const double* vg = vol + 2 * ((size_t)n_pred + g0 + g);
                const double s = vm_viou(pr, gr, 0, boxes, n_boxes, vp[0], vg[0], lane);
                const double o = vm_viou(pr, gr, 1, boxes, n_boxes, vp[1], vg[1], lane);
                out = o < s ? o : s;
            }
        }
    }
    if (lane == 0) ov[w] = out;
}

// one wave per video: predictions in descending score (stable); each takes the not yet detected ground truth of largest
// ov >= threshold, the first index on equal ov
__global__ void __launch_bounds__(64)
video_match_kernel(const int* __restrict__ pred_off, const double* __restrict__ pred_score, const int* __restrict__ gt_off,
                   const double* __restrict__ ov, int n_pred, int n_gt, int max_pred, int max_gt, double thr,
                   int* __restrict__ hit, double* __restrict__ hit_ov, int* status) {
    __shared__ double s_score[VM_MAXP];
    __shared__ int s_order[VM_MAXP];
    const int v = blockIdx.x, lane = threadIdx.x;
    const int p0 = pred_off[v], np = pred_off[v + 1] - p0;
    const int g0 = gt_off[v];
    int ng = gt_off[v + 1] - g0;
    if (np > max_pred || np > VM_MAXP || i2v_span_bad(p0, np, n_pred) || ng > max_gt || ng > VM_MAXG || i2v_span_bad(g0, ng, n_gt)) {
        if (lane == 0) atomicMax(status, v + 1);
        return;
    }
    for (int i = lane; i < np; i += 64) s_score[i] = pred_score[p0 + i];
    __syncthreads();
    for (int i = lane; i < np; i += 64) s_order[i2v_rank_desc(s_score, np, i)] = i;
    __syncthreads();
    unsigned long long det = 0;                          // bit k: ground truth lane + 64k is detected
    for (int q = 0; q < np; ++q) {
        const int p = p0 + s_order[q];
        const double* row = ov + (size_t)p * max_gt;
        double best = -1.0;
        int bi = 0x7fffffff;
        for (int k = 0, g = lane; g < ng; ++k, g += 64) {
            const double o = row[g];
            if (!((det >> k) & 1ull) && o >= 0.0 && o >= thr && o > best) best = o, bi = g;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ob > best || (ob == best && oi < bi)) best = ob, bi = oi;
        }
        if (bi != 0x7fffffff && (bi & 63) == lane) det |= 1ull << (bi >> 6);
        if (lane == 0) {
            hit[p] = bi != 0x7fffffff ? bi : -1;
            hit_ov[p] = best;
        }
    }
}

extern "C" size_t i2v_video_viou_match_workspace_bytes(int32_t n_pred, int32_t n_gt) {
    if (n_pred < 0 || n_gt < 0) return I2V_STATUS_BYTES;
    return I2V_STATUS_BYTES + i2v_align(2 * ((size_t)n_pred + n_gt) * sizeof(double));     // status word, trajectory volumes
}

extern "C" int32_t i2v_video_viou_match(const int32_t* pred_off, const int32_t* pred_rel, const double* pred_score,
                                        const int32_t* gt_off, const int32_t* gt_rel, const double* boxes,
                                        int32_t n_videos, int32_t n_pred, int32_t n_gt, int64_t n_boxes, int32_t max_pred,
                                        int32_t max_gt, double viou_threshold, double* ov, int32_t* hit, double* hit_ov,
                                        void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_videos >= 0 && n_pred >= 0 && n_gt >= 0 && n_boxes >= 0, "video_viou_match: negative count");
    I2V_CHECK_ARG(max_pred >= 0 && max_pred <= VM_MAXP, "video_viou_match: at most %d predictions per video (got %d)", VM_MAXP,
                  max_pred);
    I2V_CHECK_ARG(max_gt >= 0 && max_gt <= VM_MAXG, "video_viou_match: at most %d ground truths per video (got %d)", VM_MAXG,
                  max_gt);
    I2V_CHECK_ARG(pred_off && gt_off, "video_viou_match: null pointer");
    I2V_CHECK_ARG(n_pred == 0 || (pred_rel && pred_score && hit && hit_ov), "video_viou_match: null pointer");
    I2V_CHECK_ARG(n_gt == 0 || gt_rel, "video_viou_match: null pointer");
    I2V_CHECK_ARG(n_boxes == 0 || boxes, "video_viou_match: null pointer");
    I2V_CHECK_ARG((long long)n_pred * max_gt == 0 || ov, "video_viou_match: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_video_viou_match_workspace_bytes(n_pred, n_gt), "video_viou_match: workspace too small");
    if (n_videos == 0 || n_pred == 0) return I2V_OK;
    hipStream_t st = (hipStream_t)stream;
    int* status = (int*)ws;
    double* vol = (double*)((char*)ws + I2V_STATUS_BYTES);
    I2V_CLEAR_STATUS(ws, 0, 4, st, "video_viou_match: clearing the status word failed");
    video_volume_kernel<<<i2v_cdiv(2ll * ((long long)n_pred + n_gt), 4), 256, 0, st>>>(pred_rel, gt_rel, boxes, n_pred, n_gt,
                                                                                       n_boxes, vol);
    if (max_gt > 0)
        video_viou_kernel<<<i2v_cdiv((long long)n_pred * max_gt, 4), 256, 0, st>>>(pred_rel, gt_off, gt_rel, boxes, vol,
                                                                                   n_videos, n_pred, n_gt, n_boxes, max_gt, ov);
    video_match_kernel<<<n_videos, 64, 0, st>>>(pred_off, pred_score, gt_off, ov, n_pred, n_gt, max_pred, max_gt,
                                                viou_threshold, hit, hit_ov, status);
    I2V_CHECK_LAUNCH("video_viou_match");
    return I2V_OK;
}
