// What the anchor-target kernels share (anchors.hip, assign.hip, ignore.hip): the ground-truth offsets of the frames as a by-value
// kernel argument, and the second half of an order-preserving compaction (compact.h) of a per-anchor map into the lists every
// loss reads -- pos_idx / neg_idx i64 [F][3][cap] index triples, gi i64 [F][cap], counts i32 [F][2].  An anchor's entry of the
// map decodes to flags (bit 0 = not negative, bit 1 = positive) and the ground-truth id of a positive; the decoding is the caller's.
#pragma once
#include "compact.h"

struct FrameOffsets { int off[MVX_MAX_FRAMES + 1]; };

// the host list gt_off_host [n_frames + 1] by value (the last offset repeated up to MVX_MAX_FRAMES); false = it does not start at
// 0 or decreases
inline bool frame_offsets(const int32_t *gt_off_host, int n_frames, FrameOffsets &o) {
    for (int f = 0; f <= MVX_MAX_FRAMES; ++f) o.off[f] = gt_off_host[f < n_frames ? f : n_frames];
    bool ok = o.off[0] == 0;
    for (int f = 0; f < n_frames; ++f) ok = ok && o.off[f + 1] >= o.off[f];
    return ok;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// bcount i32 [2F][nblocks]: row 2f = positives, row 2f + 1 = not negatives of frame f among the 256 anchors of this block.
// s: two rows (compact.h's barrier contract); every thread of the block calls.
__device__ __forceinline__ void list_block_counts(int flags, int f, int nblocks, int (*s)[4], int *__restrict__ bcount) {
    const int np = block_kept_count<4>((flags & 2) != 0, s[0]);
    const int nn = block_kept_count<4>((flags & 1) != 0, s[1]);
    if (threadIdx.x == 0) {
        bcount[(size_t)(2 * f) * nblocks + blockIdx.x] = np;
        bcount[(size_t)(2 * f + 1) * nblocks + blockIdx.x] = nn;
    }
}

// Anchor a (flat index (x * W + y) * A + z, thread blockIdx.x * 256 + threadIdx.x of frame f) goes to its rank in the lists its
// flags name, entries from cap on dropped; boff = the scanned bcount, totals i32 [2F].  Thread 0 of block 0 writes the frame's
// counts clipped to cap and raises status bit 2 when a list was cut.  s as above.
__device__ __forceinline__ void list_write(int flags, long long g, int f, long long a, int W, int A, int nblocks, int (*s)[4],
                                           const int *__restrict__ boff, const int *__restrict__ totals,
                                           long long *__restrict__ pos_idx, long long *__restrict__ neg_idx,
                                           long long *__restrict__ gi, long long cap, int *__restrict__ counts,
                                           int *__restrict__ status) {
    int tp, tn;
    const long long op = boff[(size_t)(2 * f) * nblocks + blockIdx.x] + block_kept_rank<4>((flags & 2) != 0, s[0], tp);
    const long long on = boff[(size_t)(2 * f + 1) * nblocks + blockIdx.x] + block_kept_rank<4>((flags & 1) != 0, s[1], tn);
    const long long x = a / ((long long)W * A), y = (a / A) % W, z = a % A;
    if ((flags & 2) && op < cap) {
        long long *p = pos_idx + (size_t)f * 3 * cap;
        p[op] = x; p[cap + op] = y; p[2 * cap + op] = z;
        gi[(size_t)f * cap + op] = g;
    }
    if ((flags & 1) && on < cap) {
        long long *n = neg_idx + (size_t)f * 3 * cap;
        n[on] = x; n[cap + on] = y; n[2 * cap + on] = z;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long np = totals[2 * f], nn = totals[2 * f + 1];
        counts[2 * f] = (int)(np < cap ? np : cap);
        counts[2 * f + 1] = (int)(nn < cap ? nn : cap);
        if (np > cap || nn > cap) atomicOr(status, 2);
    }
}
