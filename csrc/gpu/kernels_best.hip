/*
 * Keep the best validation pass inside the captured epoch graph ([keep_best], [patience], gfx950).
 *
 *   hpnn_best_commit   judges the record hpnn_validate_commit has just filed against the best
 *                      one so far and sets a device flag: take this pass or not
 *   hpnn_snapshot_if   copies the master weights (and the momentum) into the snapshot buffers
 *                      when that flag is set, and returns at once when it is not
 *
 * One graph replay holds several epochs and so several validation passes; when the host reads
 * the history every earlier pass's weights are gone.  So the decision and the copy happen on the
 * device, behind the commit on the compute stream.  Like the cursor of kernels_validate.hip and
 * the epoch word of kernels_shuffle.hip the state lives in device memory: the captured launches
 * are the same every replay, what they do is read at run time.
 *
 * The decision is a launch of its own (one thread) and the copy is the next launch on the
 * stream: no thread of the copy decides, none waits for another workgroup.
 *
 * Improvement rule (docs/DESIGN.md 3.2g), on the record {double loss_sum, uint hits}:
 *   loss : loss_sum < best.loss_sum
 *   acc  : hits > best.hits || (hits == best.hits && loss_sum < best.loss_sum)
 *   nothing is best before the first pass: loss takes the first pass whose loss is not a NaN,
 *   acc takes the first pass; ties and (under loss) NaNs do not improve.
 * An improving pass sets stale = 0, any other pass stale += 1; with patience > 0 the pass at which
 * stale == patience sets stop, and from then on the state is frozen (take = 0 every pass).
 * An empty history (cursor == 0) is a no-op.  The record read is hist[*cursor - 1]: a commit that
 * dropped its record (full history) is judged as the last filed record again, a tie.
 *
 * The copy: a device table of up to HPNN_SNAP_MAX_SEGS segments {src, dst, bytes}; workgroup
 * (x, y) copies the 16-byte vectors x, x + X, ... of segment y, four loads in flight per lane,
 * and workgroup (0, y) the 4-byte words of the tail (bytes is a multiple of 4).  A segment whose
 * pointers are not 16-byte aligned or whose size is no multiple of 4 is skipped (the table
 * builder refuses it first).  Plain vector loads and stores, no atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

HPNN_CO_PROBE(best)

namespace {

__global__ __launch_bounds__(64) void best_commit_kernel(const hpnn_val_record *__restrict__ hist,
                                                         const unsigned int *__restrict__ cursor,
                                                         hpnn_best_state *__restrict__ st, int metric,
                                                         unsigned int patience) {
    if (threadIdx.x != 0) return;
    const unsigned int c = *cursor;
    hpnn_best_state b = *st;
    if (c == 0 || b.stop) {
        st->take = 0u;
        return;
    }
    const double loss = hist[c - 1].loss_sum;
    const unsigned int hits = hist[c - 1].hits;
    bool better;
    if (!b.valid)
        better = metric == HPNN_BEST_ACC || loss == loss;
    else if (metric == HPNN_BEST_ACC)
        better = hits > b.hits || (hits == b.hits && loss < b.loss_sum);
    else
        better = loss < b.loss_sum;
    if (better) {
        b.loss_sum = loss;
        b.hits = hits;
        b.index = c - 1;
        b.stale = 0u;
        b.valid = 1u;
        b.take = 1u;
    } else {
        b.stale += 1u;
        b.take = 0u;
    }
    if (patience && b.stale == patience) b.stop = 1u;
    *st = b;
}

constexpr int SNAP_THREADS = 256;
constexpr int SNAP_GRID_X = 64;

__global__ __launch_bounds__(SNAP_THREADS) void snapshot_if_kernel(const hpnn_snap_seg *__restrict__ segs,
                                                                   const unsigned int *__restrict__ take) {
    if (*take == 0u) return;
    const hpnn_snap_seg sg = segs[blockIdx.y];
    if ((((uintptr_t)sg.src | (uintptr_t)sg.dst) & 15u) || (sg.bytes & 3ull)) return;
    const uint4 *__restrict__ s = (const uint4 *)sg.src;
    uint4 *__restrict__ d = (uint4 *)sg.dst;
    const size_t nv = (size_t)(sg.bytes >> 4);
    const size_t stride = (size_t)gridDim.x * SNAP_THREADS;
    size_t i = (size_t)blockIdx.x * SNAP_THREADS + threadIdx.x;
    for (; i + 3 * stride < nv; i += 4 * stride) {
        const uint4 a0 = s[i], a1 = s[i + stride], a2 = s[i + 2 * stride], a3 = s[i + 3 * stride];
        d[i] = a0;
        d[i + stride] = a1;
        d[i + 2 * stride] = a2;
        d[i + 3 * stride] = a3;
    }
    for (; i < nv; i += stride) d[i] = s[i];
    const unsigned int tail = (unsigned int)(sg.bytes & 15ull) >> 2;
    if (blockIdx.x == 0 && threadIdx.x < tail)
        ((unsigned int *)sg.dst)[nv * 4 + threadIdx.x] = ((const unsigned int *)sg.src)[nv * 4 + threadIdx.x];
}

int snapshot_segs_ok(const hpnn_snap_seg *host_segs, int n_segs) {
    if (n_segs < 0 || n_segs > HPNN_SNAP_MAX_SEGS || (n_segs && !host_segs)) return 0;
    for (int i = 0; i < n_segs; i++) {
        const hpnn_snap_seg &g = host_segs[i];
        if (g.bytes == 0) continue;
        if (!g.src || !g.dst || (((uintptr_t)g.src | (uintptr_t)g.dst) & 15u) || (g.bytes & 3ull)) return 0;
    }
    return 1;
}

}  // namespace

/* an empty one-thread launch (the yardstick scripts/keep_best_bench.py holds a flag-0 pass
 * against); with a synchronise it is the launch that loads this unit's code object, once per
 * device before a capture (the other units are loaded by hpnn_preload_code_objects) */
extern "C" int hpnn_best_empty_launch(hipStream_t stream) {
    hipLaunchKernelGGL(hpnn_co_probe_kernel_best, dim3(1), dim3(1), 0, stream);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_best_preload(hipStream_t stream) {
    if (hpnn_best_empty_launch(stream)) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_best_commit(const hpnn_val_record *hist, const unsigned int *cursor, hpnn_best_state *state,
                                int metric, unsigned int patience, hipStream_t stream) {
    if (!hist || !cursor || !state || (metric != HPNN_BEST_LOSS && metric != HPNN_BEST_ACC)) return -1;
    if (((uintptr_t)hist & 7u) || ((uintptr_t)cursor & 3u) || ((uintptr_t)state & 7u)) return -1;
    hipLaunchKernelGGL(best_commit_kernel, dim3(1), dim3(1), 0, stream, hist, cursor, state, metric, patience);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_snapshot_table(hpnn_snap_seg *segs, const hpnn_snap_seg *host_segs, int n_segs,
                                   hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 15u) || !snapshot_segs_ok(host_segs, n_segs)) return -1;
    if (n_segs == 0) return 0;
    /* pageable source: the copy has left host_segs when the call returns */
    if (hipMemcpyAsync(segs, host_segs, (size_t)n_segs * sizeof(hpnn_snap_seg), hipMemcpyHostToDevice, stream) !=
        hipSuccess)
        return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_snapshot_if(const hpnn_snap_seg *segs, int n_segs, const unsigned int *take,
                                hipStream_t stream) {
    if (n_segs < 0 || n_segs > HPNN_SNAP_MAX_SEGS || !take || ((uintptr_t)take & 3u)) return -1;
    if (n_segs == 0) return 0;
    if (!segs || ((uintptr_t)segs & 15u)) return -1;
    hipLaunchKernelGGL(snapshot_if_kernel, dim3(SNAP_GRID_X, n_segs), dim3(SNAP_THREADS), 0, stream, segs, take);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
