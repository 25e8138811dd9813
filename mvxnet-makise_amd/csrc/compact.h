// Order-preserving stream compaction: the part that happens inside one workgroup of NW waves.
//
// A compaction is: count the kept threads of every block (block_kept_count), scan the block counts
// (mvxi_scan_block_counts, or whatever the caller does instead), then store every kept element at block offset + its rank
// among the kept threads of its block (block_kept_rank).
//
// Barrier contract: every thread of the block calls the helper; each helper contains exactly ONE __syncthreads, between the
// waves' writes of their counts to s[0..NW) and the reads.  There is no barrier after the reads, so `s` must not be written
// again -- a second call with the same `s` included -- before the block has passed another barrier; a caller that ranks
// several times in a row alternates two rows (call k reads row k & 1 before the barrier of call k + 1, which call k + 2's
// writes follow).  NW = 1: no barrier and `s` is not touched (may be null); the calling wave must be wave 0 of its block.
#pragma once
#include "common.h"

template <int NW>
__device__ __forceinline__ int block_kept_count(bool keep, int *s) {
    const int mine = __popcll(__ballot(keep));
    if (NW == 1) return mine;
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = mine;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) total += s[w];
    return total;
}

// this thread's exclusive rank among the kept threads of the block, in thread order; total = block_kept_count
template <int NW>
__device__ __forceinline__ int block_kept_rank(bool keep, int *s, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bits = __ballot(keep);
    int before = 0;
    total = __popcll(bits);
    if (NW > 1) {
        if (lane == 0) s[wv] = total;
        __syncthreads();
        total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int c = s[w];
            before += w < wv ? c : 0;
            total += c;
        }
    }
    return before + __popcll(bits & ((1ull << lane) - 1ull));
}
