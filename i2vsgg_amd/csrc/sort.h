// The library's one sort (sort.hip): a segmented bitonic sort of unsigned 64-bit keys, ASCENDING, in place.  Its callers
// build keys whose ascending order is the order they want (the float front end below, det_eval.hip's class | key | position)
// and pad every segment to sort_padded(n) keys with all ones, which sort last.  Internal to the library: C++ linkage, not in
// include/i2vsgg_hip.h.
#pragma once
#include "common.h"

constexpr int SORT_TILE = 4096;     // u64 keys per LDS tile (32 KiB of the 160 KiB: occupancy is not bound by it)
constexpr int SORT_THREADS = 512;

// keys per segment: the power of two that holds n, one tile at the least
inline int sort_padded(int n) {
    int p = SORT_TILE;
    while (p < n) p <<= 1;
    return p;
}

// the index a sorted key of the float front end carries in its low word
__host__ __device__ inline int sort_key_index(unsigned long long k) { return (int)(k & 0xFFFFFFFFull); }

// n_seg segments of P keys each, one behind the other; P = sort_padded(n) of the caller's n
void i2v_launch_sort_u64(unsigned long long* keys, int n_seg, int P, hipStream_t st);

// The float front end without i2v_sort_desc's argument checks: n_seg segments of n scores -> buf (n_seg * sort_padded(n)
// keys), sorted by descending score, equal scores by ascending index.  Returns P, the keys per segment.
int i2v_launch_sort_desc(const float* keys, int n_seg, int n, unsigned long long* buf, hipStream_t st);
