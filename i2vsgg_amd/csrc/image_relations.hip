// Image relation recall@K (Lu et al., ECCV 2016: predicate / phrase / relation detection): the greedy match of an image's
// ranked triplets against its annotated relations, in relation mode (both boxes overlap) and in phrase mode (the union boxes
// overlap), and the integer counters behind recall, zero-shot recall and per-predicate recall.  The rules are stated once, in
// i2vsgg_amd/image_relations.py; the host form there evaluates the same float64 expressions in the same order (the library
// is built with -ffp-contract=off -fno-fast-math), so device and host agree bit for bit.  No floating-point atomics; the
// counters are integer atomics, whose result does not depend on the order.
#include "table_common.h"

#define IR_MAXG I2V_IMAGE_RELATION_MAX_GT    // ground truths of one image: one taken-bit each in LDS
#define IR_MAXK I2V_IMAGE_RELATION_MAX_K     // values of K in one count
#define IR_NONE 0x7fffffff

// the union of a row's subject and object box: min of x1 / y1, max of x2 / y2 (exact)
__device__ __forceinline__ void ir_union(const double* r, double* u) {
    u[0] = r[0] < r[4] ? r[0] : r[4];
    u[1] = r[1] < r[5] ? r[1] : r[5];
    u[2] = r[2] > r[6] ? r[2] : r[6];
    u[3] = r[3] > r[7] ? r[3] : r[7];
}

// One workgroup of one wave per (image, mode): blockIdx.x the image, blockIdx.y 0 relation / 1 phrase.  Lane l owns ground
// truths l, l + 64, ...; bit g of s_taken says that ground truth g of the image is taken.  Every loop bound comes from the
// offset tables, so it is the same in all 64 lanes and every lane reaches every shuffle and every barrier.
__global__ void __launch_bounds__(I2V_WAVE)
image_relation_match_kernel(const int* __restrict__ pred_off, const int* __restrict__ gt_off, const int* __restrict__ pred_trip,
                            const double* __restrict__ pred_box, const int* __restrict__ gt_trip,
                            const double* __restrict__ gt_box, int n_pred, int n_gt, int max_gt, double thr,
                            int* __restrict__ hit, double* __restrict__ hit_ov, int* __restrict__ gt_rank, int* status) {
    __shared__ unsigned int s_taken[IR_MAXG / 32];
    const int im = blockIdx.x, mode = blockIdx.y, lane = threadIdx.x;
    const int p0 = pred_off[im], p1 = pred_off[im + 1], g0 = gt_off[im], g1 = gt_off[im + 1];
    const bool pred_ok = !i2v_range_bad(p0, p1, n_pred);
    const bool gt_ok = !i2v_range_bad(g0, g1, n_gt);
    int* hit_m = hit + (size_t)mode * n_pred;
    double* hov_m = hit_ov + (size_t)mode * n_pred;
    int* rank_m = gt_rank + (size_t)mode * n_gt;
    if (!pred_ok || !gt_ok || g1 - g0 > max_gt || g1 - g0 > IR_MAXG) {      // a malformed image: say so, read nothing through it
        if (pred_ok)
            for (int p = p0 + lane; p < p1; p += I2V_WAVE) hit_m[p] = -1, hov_m[p] = -1.0;
        if (gt_ok)
            for (int g = g0 + lane; g < g1; g += I2V_WAVE) rank_m[g] = -1;
        if (lane == 0 && mode == 0) atomicMax(status, im + 1);
        return;
    }
    const int ng = g1 - g0;
    for (int w = lane; w < IR_MAXG / 32; w += I2V_WAVE) s_taken[w] = 0u;
    __syncthreads();                                             // one wave: the cleared flags are visible to all its lanes
    for (int p = p0; p < p1; ++p) {
        const int* pt = pred_trip + (size_t)p * 3;
        const int ts = pt[0], tp = pt[1], to = pt[2];
        const double* pb = pred_box + (size_t)p * 8;
        double pu[4];
        ir_union(pb, pu);
        double best = -1.0;
        int bi = IR_NONE;
        for (int g = lane; g < ng; g += I2V_WAVE) {
            const int* gt = gt_trip + (size_t)(g0 + g) * 3;
            if (gt[0] != ts || gt[1] != tp || gt[2] != to) continue;
            if ((s_taken[g >> 5] >> (g & 31)) & 1u) continue;
            const double* gb = gt_box + (size_t)(g0 + g) * 8;
            double ov;
            if (mode == 0) {
                const double a = i2v_overlap_plus1(pb, gb), b = i2v_overlap_plus1(pb + 4, gb + 4);
                ov = a < b ? a : b;
            } else {
                double gu[4];
                ir_union(gb, gu);
                ov = i2v_overlap_plus1(pu, gu);
            }
            if (ov >= thr && (bi == IR_NONE || ov > best)) best = ov, bi = g;   // ascending g: the lower index stays on equal ov
        }
        for (int o = 32; o > 0; o >>= 1) {                       // the larger overlap, then the lower index; all 64 lanes
            const double ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != IR_NONE && (bi == IR_NONE || ob > best || (ob == best && oi < bi))) best = ob, bi = oi;
        }
        if (lane == 0) {                                         // every output address is written once, by one lane
            hit_m[p] = bi != IR_NONE ? bi : -1;
            hov_m[p] = bi != IR_NONE ? best : -1.0;
            if (bi != IR_NONE) {
                s_taken[bi >> 5] |= 1u << (bi & 31);
                rank_m[g0 + bi] = p - p0;
            }
        }
        __syncthreads();                                         // the flag of prediction p is written before p + 1 reads it
    }
    for (int g = lane; g < ng; g += I2V_WAVE)                    // the ground truths nobody took
        if (!((s_taken[g >> 5] >> (g & 31)) & 1u)) rank_m[g0 + g] = -1;
}

struct IrKs {
    int n;
    int k[IR_MAXK];
};

// One thread per (mode, ground truth), after the match kernel on the same stream: blockIdx.y is the mode.  Counter tables
// (int64): totals / zs_totals [mode][k][hits, n_gt]; per_predicate [mode][k][predicate][hits, n_gt].
__global__ void __launch_bounds__(256)
image_relation_count_kernel(const int* __restrict__ gt_rank, const int* __restrict__ gt_trip, const int* __restrict__ gt_zs,
                            int n_gt, int n_rel, IrKs ks, unsigned long long* totals, unsigned long long* zs_totals,
                            unsigned long long* per_predicate, int* status) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x, mode = blockIdx.y;
    int h[IR_MAXK], counted = 0, zs = 0;
    for (int k = 0; k < IR_MAXK; ++k) h[k] = 0;
    if (g < n_gt) {
        const int pr = gt_trip[(size_t)g * 3 + 1];
        if (pr < 0 || pr >= n_rel) {
            atomicMax(status + 1, g + 1);                        // a predicate outside the table: not counted
        } else {
            const int r = gt_rank[(size_t)mode * n_gt + g];
            counted = 1;
            zs = gt_zs[g] != 0 ? 1 : 0;
            for (int k = 0; k < IR_MAXK; ++k)
                if (k < ks.n) {
                    h[k] = (r >= 0 && r < ks.k[k]) ? 1 : 0;
                    unsigned long long* pp = per_predicate + (((size_t)mode * ks.n + k) * n_rel + pr) * 2;
                    if (h[k]) atomicAdd(pp, 1ull);
                    atomicAdd(pp + 1, 1ull);
                }
        }
    }
    for (int k = 0; k < IR_MAXK; ++k) {                          // every lane takes part; lanes past n_gt hold zeros
        if (k >= ks.n) break;                                    // the same in every lane
        int v = h[k], vz = h[k] * zs, c = counted, cz = zs;
        for (int o = 32; o > 0; o >>= 1) {
            v += __shfl_xor(v, o);
            vz += __shfl_xor(vz, o);
            c += __shfl_xor(c, o);
            cz += __shfl_xor(cz, o);
        }
        if ((threadIdx.x & (I2V_WAVE - 1)) == 0) {
            const size_t at = ((size_t)mode * ks.n + k) * 2;
            if (v) atomicAdd(totals + at, (unsigned long long)v);
            if (c) atomicAdd(totals + at + 1, (unsigned long long)c);
            if (vz) atomicAdd(zs_totals + at, (unsigned long long)vz);
            if (cz) atomicAdd(zs_totals + at + 1, (unsigned long long)cz);
        }
    }
}

extern "C" size_t i2v_image_relation_match_workspace_bytes(int32_t n_images) {
    (void)n_images;
    return I2V_STATUS_BYTES;                                     // two status words: match, count
}

extern "C" int32_t i2v_image_relation_match(const int32_t* pred_off, const int32_t* gt_off, const int32_t* pred_trip,
                                            const double* pred_box, const int32_t* gt_trip, const double* gt_box,
                                            int32_t n_images, int32_t n_pred, int32_t n_gt, int32_t max_gt, double iou_threshold,
                                            int32_t* hit, double* hit_ov, int32_t* gt_rank, void* ws, size_t ws_bytes,
                                            void* stream) {
    I2V_CHECK_ARG(n_images >= 0 && n_pred >= 0 && n_gt >= 0, "image_relation_match: negative count");
    I2V_CHECK_ARG(max_gt >= 0 && max_gt <= IR_MAXG, "image_relation_match: at most %d ground truths in one image (got %d)", IR_MAXG,
                  max_gt);
    I2V_CHECK_ARG(pred_off && gt_off, "image_relation_match: null pointer");
    I2V_CHECK_ARG(n_pred == 0 || (pred_trip && pred_box && hit && hit_ov), "image_relation_match: null pointer");
    I2V_CHECK_ARG(n_gt == 0 || (gt_trip && gt_box && gt_rank), "image_relation_match: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_image_relation_match_workspace_bytes(n_images), "image_relation_match: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    I2V_CLEAR_STATUS(ws, 0, 8, st, "image_relation_match: clearing the status words failed");
    if (n_images == 0) return I2V_OK;
    image_relation_match_kernel<<<dim3(n_images, 2), I2V_WAVE, 0, st>>>(pred_off, gt_off, pred_trip, pred_box, gt_trip, gt_box, n_pred,
                                                                       n_gt, max_gt, iou_threshold, hit, hit_ov, gt_rank, (int*)ws);
    I2V_CHECK_LAUNCH("image_relation_match");
    return I2V_OK;
}

extern "C" int32_t i2v_image_relation_count(const int32_t* gt_rank, const int32_t* gt_trip, const int32_t* gt_zs,
                                            const int32_t* nreturns, int32_t n_gt, int32_t n_rel, int32_t n_k, int64_t* totals,
                                            int64_t* zs_totals, int64_t* per_predicate, void* ws, size_t ws_bytes, void* stream) {
    I2V_CHECK_ARG(n_gt >= 0 && n_rel >= 1, "image_relation_count: needs a count >= 0 and at least 1 predicate, got %d / %d", n_gt, n_rel);
    I2V_CHECK_ARG(n_k >= 1 && n_k <= IR_MAXK, "image_relation_count: 1 to %d values of K (got %d)", IR_MAXK, n_k);
    I2V_CHECK_ARG(nreturns && totals && zs_totals && per_predicate, "image_relation_count: null pointer");
    I2V_CHECK_ARG(n_gt == 0 || (gt_rank && gt_trip && gt_zs), "image_relation_count: null pointer");
    I2V_CHECK_ARG(ws && ws_bytes >= i2v_image_relation_match_workspace_bytes(0), "image_relation_count: workspace too small");
    IrKs ks;
    ks.n = n_k;
    for (int k = 0; k < IR_MAXK; ++k) ks.k[k] = k < n_k ? nreturns[k] : 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = (size_t)2 * n_k * 2 * sizeof(int64_t);
    I2V_CLEAR_STATUS(ws, 4, 4, st, "image_relation_count: clearing the counters failed");
    if (hipMemsetAsync(totals, 0, cells, st) != hipSuccess || hipMemsetAsync(zs_totals, 0, cells, st) != hipSuccess ||
        hipMemsetAsync(per_predicate, 0, cells * n_rel, st) != hipSuccess) {
        i2v_set_error("image_relation_count: clearing the counters failed");
        return I2V_ERR_LAUNCH;
    }
    if (n_gt == 0) return I2V_OK;
    image_relation_count_kernel<<<dim3(i2v_cdiv(n_gt, 256), 2), 256, 0, st>>>(gt_rank, gt_trip, gt_zs, n_gt, n_rel, ks,
                                                                             (unsigned long long*)totals,
                                                                             (unsigned long long*)zs_totals,
                                                                             (unsigned long long*)per_predicate, (int*)ws);
    I2V_CHECK_LAUNCH("image_relation_count");
    return I2V_OK;
}
