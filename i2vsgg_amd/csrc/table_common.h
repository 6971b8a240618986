// What the packed-table ops share (seqnms, video, det_eval, recognition, relation_features, relation_targets,
// image_relations): the workspace's status header, the tests of an offset table's entries, the +1 overlap and the counting rank.  The rules the
// device and host forms keep bit for bit are stated here once; the host side is i2vsgg_amd/packing.py.
#pragma once
#include "common.h"

// Every workspace starts with a header of status words (int32; 0: the tables are well formed, else 1 + the first malformed
// entry, raised by atomicMax); an op's scratch arrays follow it.
#define I2V_STATUS_BYTES 256

// Clears n status bytes at byte offset off of the workspace on the stream, ahead of the launches that raise them.
#define I2V_CLEAR_STATUS(ws, off, n, st, what)                                  \
    do {                                                                        \
        if (hipMemsetAsync((char*)(ws) + (off), 0, (n), (st)) != hipSuccess) {  \
            i2v_set_error(what);                                                \
            return I2V_ERR_LAUNCH;                                              \
        }                                                                       \
    } while (0)

// rows [p0, p0 + n) do not lie inside a table of total rows; an op's own limits on n stay at the call site
__device__ __forceinline__ bool i2v_span_bad(int p0, int n, long long total) {
    return p0 < 0 || n < 0 || (long long)p0 + n > total;
}

// the same for a table entry given as [begin, end): no difference is formed before it is known to be safe
__device__ __forceinline__ bool i2v_range_bad(int begin, int end, int total) {
    return begin < 0 || end < begin || end > total;
}

// lib/model/nms/nms_cpu.py:14,26-31 in its own operation order (+1 convention; an empty intersection: 0)
__device__ __forceinline__ double i2v_overlap_plus1(const double* a, const double* b) {
    const double iw = ((a[2] < b[2] ? a[2] : b[2]) - (a[0] > b[0] ? a[0] : b[0])) + 1.0;
    const double ih = ((a[3] < b[3] ? a[3] : b[3]) - (a[1] > b[1] ? a[1] : b[1])) + 1.0;
    if (iw <= 0.0 || ih <= 0.0) return 0.0;
    const double inter = iw * ih;
    const double aa = ((a[2] - a[0]) + 1.0) * ((a[3] - a[1]) + 1.0);
    const double ab = ((b[2] - b[0]) + 1.0) * ((b[3] - b[1]) + 1.0);
    return inter / ((aa + ab) - inter);
}

// position of key[i] in a stable descending order of key[0 .. n): keys larger than it, and equal keys in front of it.  Counted,
// so for short tables only (a frame's predictions, a segment's detections); the keys lie in LDS or in global memory.
template <typename T>
__device__ __forceinline__ int i2v_rank_desc(const T* key, int n, int i) {
    const T k = key[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const T kj = key[j];
        r += (kj > k || (kj == k && j < i)) ? 1 : 0;
    }
    return r;
}
