// kv_copy_kernels.h - session-to-session KV copy (sd_session_copy_kv): positions [lo, hi) of every (layer, K|V, KV head)
// plane of one session's arena go to up to 16 other sessions' arenas in ONE launch.  The prompt queue copies a shared
// prompt prefix from its donor sessions with it, sampling/multi.py the winner's rows between replicas.
#pragma once
#include "multi_kernels.h"

// The destinations of one launch, passed by value.  Every arena is [planes][max_seq][row_bytes]; the max_seq of source and
// destinations may differ, the row size is the model's.
struct KvCopyTab {
    char *dst[16];
    int dst_max_seq[16];
    int lo[16], hi[16];
};

enum { KV_COPY_THREADS = 256, KV_COPY_CHUNK_MAX = KV_COPY_THREADS * 4 * 16 };     // four 16-byte accesses per lane

// Grid (x, y, z) = (chunk of the byte run, plane, item).  A plane's positions are contiguous, so item z's range is one run
// of (hi - lo) * row_bytes bytes per plane, whatever the element type; workgroup x moves bytes [x * chunk_bytes,
// (x + 1) * chunk_bytes) of it with adopt_copy_bytes (16-byte vector accesses where source and destination are congruent
// mod 16, bytes otherwise).  chunk_bytes is a multiple of 16, so every chunk of a run has the alignment of its first.  The
// host sizes the grid by the longest run of the launch; the workgroups past a shorter item's run exit.
__global__ __launch_bounds__(KV_COPY_THREADS) void session_copy_kv_kernel(const char *__restrict__ src, int src_max_seq,
                                                                          int row_bytes, int chunk_bytes, KvCopyTab t) {
    const int z = blockIdx.z, lo = t.lo[z];
    const size_t run = (size_t)(t.hi[z] - lo) * row_bytes, b0 = (size_t)blockIdx.x * chunk_bytes;
    if (b0 >= run) return;
    const int n = (int)min((size_t)chunk_bytes, run - b0);
    const size_t plane = blockIdx.y;
    adopt_copy_bytes(t.dst[z] + (plane * t.dst_max_seq[z] + lo) * row_bytes + b0,
                     src + (plane * src_max_seq + lo) * row_bytes + b0, n);
}
