// RPN proposal path on the device: anchors + box decode + clip, per-image descending
// sort (sort.hip: bitonic, 64-bit score|index keys), greedy NMS (nms.hip), top-N gather and zero padding; and the overlaps
// of boxes with the ground truth.  Replaces rpn/proposal_layer.py:49-163.
//
// Box arithmetic is fp32 with one rounding per operation (built with
// -ffp-contract=off) so IoU threshold decisions match the reference's CPU path bit
// for bit on the same boxes.
#include "common.h"
#include "nms.h"
#include "sort.h"

namespace {
// ------------------------------------------------------------------ decode + clip
// One thread per anchor (b, y, x, a); NHWC inputs make (y,x,a) the memory order of both
// the scores and the deltas, which is exactly the reference's permute(0,2,3,1) order
// (proposal_layer.py:99-104).
__global__ void rpn_decode_kernel(const float* __restrict__ cls, int is_prob, const float* __restrict__ bbox,
                                  const float* __restrict__ im_info, const float* __restrict__ base, int B, int H,
                                  int W, int A, int stride, float* __restrict__ prop, float* __restrict__ score) {
    const long long n_per = (long long)H * W * A;
    const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (idx >= n_per * B) return;
    const int b = idx / n_per;
    const long long i = idx % n_per;
    const int a = i % A;
    const long long cell = i / A;
    const int x = cell % W, y = cell / W;
    // fg probability: rpn.py:69-71 reshapes to (B,2,A*H,W) and softmaxes the pair
    const float* cp = cls + ((long long)b * H * W + cell) * 2 * A;
    float fg;
    if (is_prob) {
        fg = cp[A + a];
    } else {
        float s0 = cp[a], s1 = cp[A + a], m = fmaxf(s0, s1);
        float e0 = expf(s0 - m), e1 = expf(s1 - m);
        fg = e1 / (e0 + e1);
    }
    score[idx] = fg;
    // anchor = base[a] + (x*stride, y*stride, x*stride, y*stride)   proposal_layer.py:81-95
    const float sx = (float)(x * stride), sy = (float)(y * stride);
    const float ax1 = base[4 * a] + sx, ay1 = base[4 * a + 1] + sy;
    const float ax2 = base[4 * a + 2] + sx, ay2 = base[4 * a + 3] + sy;
    const float* d = bbox + ((long long)b * H * W + cell) * 4 * A + 4 * a;
    // bbox_transform.py:77-103
    const float w = ax2 - ax1 + 1.0f, h = ay2 - ay1 + 1.0f;
    const float cx = ax1 + 0.5f * w, cy = ay1 + 0.5f * h;
    const float pcx = d[0] * w + cx, pcy = d[1] * h + cy;
    const float pw = (float)exp((double)d[2]) * w, ph = (float)exp((double)d[3]) * h;
    const float xmax = im_info[3 * b + 1] - 1.0f, ymax = im_info[3 * b] - 1.0f;
    // clip_boxes :125-133
    float4 o;
    o.x = fminf(fmaxf(pcx - 0.5f * pw, 0.f), xmax);
    o.y = fminf(fmaxf(pcy - 0.5f * ph, 0.f), ymax);
    o.z = fminf(fmaxf(pcx + 0.5f * pw, 0.f), xmax);
    o.w = fminf(fmaxf(pcy + 0.5f * ph, 0.f), ymax);
    *(float4*)(prop + 4 * idx) = o;
}

// ------------------------------------------------------------------ gather sorted dets
__global__ void gather_dets(const unsigned long long* __restrict__ keys, int P, const float* __restrict__ prop,
                            const float* __restrict__ score, int n_all, int n_top, float* __restrict__ dets,
                            int* __restrict__ src_idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= n_top) return;
    unsigned long long k = keys[(long long)b * P + i];
    int idx = sort_key_index(k);
    float4 p = *(const float4*)(prop + ((long long)b * n_all + idx) * 4);
    float* d = dets + ((long long)b * n_top + i) * 5;
    d[0] = p.x; d[1] = p.y; d[2] = p.z; d[3] = p.w; d[4] = score[(long long)b * n_all + idx];
    src_idx[(long long)b * n_top + i] = idx;
}

// ------------------------------------------------------------------ emit rois
__global__ void write_rois(const float* __restrict__ dets, const int* __restrict__ src_idx,
                           const int* __restrict__ keep, const int* __restrict__ num, int n_top, int post,
                           float* __restrict__ rois, int* __restrict__ kept_idx, int* __restrict__ num_kept) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (k >= post) return;
    const int cnt = min(num[b], post);
    float* r = rois + ((long long)b * post + k) * 5;
    r[0] = (float)b;
    int src = -1;
    if (k < cnt) {
        const int row = keep[(long long)b * n_top + k];
        const float* d = dets + ((long long)b * n_top + row) * 5;
        r[1] = d[0]; r[2] = d[1]; r[3] = d[2]; r[4] = d[3];
        src = src_idx[(long long)b * n_top + row];
    } else {
        r[1] = r[2] = r[3] = r[4] = 0.f;
    }
    if (kept_idx) kept_idx[(long long)b * post + k] = src;
    if (num_kept && k == 0) num_kept[b] = cnt;
}

// ------------------------------------------------------------------ IoU vs ground truth
// bbox_transform.py:168-257.  One thread per box row, loops the K gt boxes (K <= 64).
__global__ void bbox_overlaps_kernel(const float* __restrict__ boxes, int box_stride, int box_off, int batched,
                                     const float* __restrict__ gt, int N, int K, float* __restrict__ ov,
                                     float* __restrict__ max_ov, int* __restrict__ arg_ov) {
    extern __shared__ float sg[];          // K x 6: x1,y1,x2,y2,area,zero
    const int b = blockIdx.y;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float* g = gt + ((long long)b * K + k) * 5;
        float gw = g[2] - g[0] + 1.0f, gh = g[3] - g[1] + 1.0f;
        sg[k * 6] = g[0]; sg[k * 6 + 1] = g[1]; sg[k * 6 + 2] = g[2]; sg[k * 6 + 3] = g[3];
        sg[k * 6 + 4] = gw * gh;
        sg[k * 6 + 5] = (gw == 1.0f && gh == 1.0f) ? 1.f : 0.f;
    }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* p = boxes + ((long long)(batched ? b : 0) * N + i) * box_stride + box_off;
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const float bw = x2 - x1 + 1.0f, bh = y2 - y1 + 1.0f;
    const float area = bw * bh;
    const bool bzero = (bw == 1.0f && bh == 1.0f);
    float best = -INFINITY;
    int besti = 0;
    for (int k = 0; k < K; ++k) {
        float iw = fminf(x2, sg[k * 6 + 2]) - fmaxf(x1, sg[k * 6]) + 1.0f;
        float ih = fminf(y2, sg[k * 6 + 3]) - fmaxf(y1, sg[k * 6 + 1]) + 1.0f;
        iw = iw < 0.f ? 0.f : iw;
        ih = ih < 0.f ? 0.f : ih;
        float inter = iw * ih;
        float o = inter / (area + sg[k * 6 + 4] - inter);
        if (sg[k * 6 + 5] != 0.f) o = 0.f;
        if (bzero) o = -1.f;
        if (ov) ov[((long long)b * N + i) * K + k] = o;
        if (o > best) { best = o; besti = k; }
    }
    if (max_ov) max_ov[(long long)b * N + i] = best;
    if (arg_ov) arg_ov[(long long)b * N + i] = besti;
}

struct ProposalWs {
    float* prop; float* score; unsigned long long* keys; float* dets; int* src; int* keep; int* num;
    unsigned long long* mask; size_t total;
};

ProposalWs carve(void* ws, int B, long long n_all, int n_top) {
    ProposalWs w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* q = p ? (void*)(p + off) : nullptr; off += i2v_align(bytes); return q; };
    const int P = sort_padded((int)n_all);
    const int nblk = (n_top + 63) / 64;
    w.prop = (float*)take((size_t)B * n_all * 16);
    w.score = (float*)take((size_t)B * n_all * 4);
    w.keys = (unsigned long long*)take((size_t)B * P * 8);
    w.dets = (float*)take((size_t)B * n_top * 20);
    w.src = (int*)take((size_t)B * n_top * 4);
    w.keep = (int*)take((size_t)B * n_top * 4);
    w.num = (int*)take((size_t)B * 4);
    w.mask = (unsigned long long*)take((size_t)B * n_top * nblk * 8);
    w.total = off;
    return w;
}
}  // namespace

extern "C" int32_t i2v_rpn_decode(const float* cls, int32_t is_prob, const float* bbox, const float* im_info,
                                  const float* base, int32_t B, int32_t H, int32_t W, int32_t A, int32_t stride,
                                  float* prop, float* score, void* stream) {
    I2V_CHECK_ARG(cls && bbox && im_info && base && prop && score, "rpn_decode: null pointer");
    I2V_CHECK_ARG(B > 0 && H > 0 && W > 0 && A > 0 && A <= 64, "rpn_decode: bad shape");
    long long total = (long long)B * H * W * A;
    rpn_decode_kernel<<<i2v_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(cls, is_prob, bbox, im_info, base, B, H,
                                                                              W, A, stride, prop, score);
    I2V_CHECK_LAUNCH("rpn_decode");
    return I2V_OK;
}

extern "C" size_t i2v_rpn_proposal_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t A, int32_t pre) {
    if (B <= 0 || H <= 0 || W <= 0 || A <= 0) return 256;
    long long n_all = (long long)H * W * A;
    // proposal_layer.py:140: truncate only when 0 < pre < B*N (numel of the whole batch)
    int n_top = (pre > 0 && pre < (long long)B * n_all && pre < n_all) ? pre : (int)n_all;
    return carve(nullptr, B, n_all, n_top).total;
}

extern "C" int32_t i2v_rpn_proposal(const float* cls, int32_t is_prob, const float* bbox, const float* im_info,
                                    const float* base, int32_t B, int32_t H, int32_t W, int32_t A, int32_t stride,
                                    int32_t pre, int32_t post, float thresh, float* rois, int32_t* kept_idx,
                                    int32_t* num_kept, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(cls && bbox && im_info && base && rois, "rpn_proposal: null pointer");
    I2V_CHECK_ARG(B > 0 && H > 0 && W > 0 && A > 0 && A <= 64 && post > 0, "rpn_proposal: bad shape");
    const long long n_all = (long long)H * W * A;
    I2V_CHECK_ARG(n_all <= 64 * SCAN_MAX_BLK, "rpn_proposal: more than 65536 anchors per image");
    const int n_top = (pre > 0 && pre < (long long)B * n_all && pre < n_all) ? pre : (int)n_all;
    if (!ws || ws_bytes < carve(nullptr, B, n_all, n_top).total) {
        i2v_set_error("rpn_proposal: workspace too small");
        return I2V_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    ProposalWs w = carve(ws, B, n_all, n_top);
    rpn_decode_kernel<<<i2v_cdiv(B * n_all, 256), 256, 0, st>>>(cls, is_prob, bbox, im_info, base, B, H, W, A,
                                                               stride, w.prop, w.score);
    const int P = i2v_launch_sort_desc(w.score, B, (int)n_all, w.keys, st);
    gather_dets<<<dim3(i2v_cdiv(n_top, 256), B), 256, 0, st>>>(w.keys, P, w.prop, w.score, (int)n_all, n_top,
                                                               w.dets, w.src);
    const int32_t rc = launch_nms(w.dets, B, n_top, thresh, post, w.keep, w.num, w.mask, st);
    if (rc) return rc;
    write_rois<<<dim3(i2v_cdiv(post, 256), B), 256, 0, st>>>(w.dets, w.src, w.keep, w.num, n_top, post, rois,
                                                             kept_idx, num_kept);
    I2V_CHECK_LAUNCH("rpn_proposal");
    return I2V_OK;
}

extern "C" int32_t i2v_bbox_overlaps(const float* boxes, int32_t box_stride, int32_t box_off, int32_t batched,
                                     const float* gt, int32_t B, int32_t N, int32_t K, float* ov, float* max_ov,
                                     int32_t* arg_ov, void* stream) {
    I2V_CHECK_ARG(boxes && gt, "bbox_overlaps: null pointer");
    I2V_CHECK_ARG(B > 0 && N >= 0 && K > 0 && K <= 1024 && box_stride >= box_off + 4, "bbox_overlaps: bad shape");
    if (N == 0) return I2V_OK;
    bbox_overlaps_kernel<<<dim3(i2v_cdiv(N, 256), B), 256, (size_t)K * 24, (hipStream_t)stream>>>(
        boxes, box_stride, box_off, batched, gt, N, K, ov, max_ov, arg_ov);
    I2V_CHECK_LAUNCH("bbox_overlaps");
    return I2V_OK;
}
