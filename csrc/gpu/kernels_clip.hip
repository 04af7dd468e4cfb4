/*
 * Gradient clipping by global norm inside the captured epoch graph ([clip], gfx950; rule and
 * order in <libhpnn/clip.h>, docs/DESIGN.md 3.2k).
 *
 *   hpnn_gnorm_partials     one workgroup of 256 lanes per block of 1024 elements over a device
 *                           table of segments (one per layer): the element as the update rule sees
 *                           it, squared in FP64, four per lane, the fixed tree in LDS, one double
 *                           per block into partials[]
 *   hpnn_clip_finalize_dev  one workgroup: partials[] in the same lane order and tree, then
 *                           hpnn_clip_finalize on the device state (norm, factor, the counters)
 *   hpnn_clip_commit_dev    one thread, the last launch of an epoch: the epoch record appended to
 *                           a device history, the counters zeroed
 *
 * ONE kernel template, on the master type T (float | double) and on the slab order (sequential:
 * the segment walker of upd_common.h; 8-way interleaved: its sub-tile update), serves the FP64 /
 * FP32 engines and the BF16 plan's padded [Np, Kp] FP32 slabs (the zero padding adds 0).
 *
 * The order of every sum is a function of the element index only: it depends on neither the grid
 * nor the alignment nor timing.  A lane's four elements are one 16-byte load per slab (two for
 * double) where the address and the slab stride allow it, otherwise element by element through the
 * same arithmetic.  The gradients are read only.  Like kernels_adam.hip and kernels_lrsched.hip
 * every number that changes lives in device memory and is read when the launch runs; the thread
 * that changes the state is a launch of its own and its consumers later launches on the same
 * stream.  No atomics, no workgroup waits for another, plain vector loads and stores.
 *
 * This unit is compiled with FP contraction off: nothing is fused, and the square root and the
 * division of the finalize are the correctly rounded ones, as on the host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <libhpnn/clip.h>

#include "kernels.h"
#include "upd_common.h"

HPNN_CO_PROBE(clip)

namespace {

using hpnn_upd::VecT;

constexpr int LANES = (int)HPNN_CLIP_LANES, BLOCK = (int)HPNN_CLIP_BLOCK;
static_assert(BLOCK == 4 * LANES, "four elements per lane");
static_assert(HPNN_GNORM_MAX_SEGS == hpnn_upd::SEG_MAX, "one table size");

/* the 256 partials of a workgroup through the fixed tree; the sum is in p[0] for every lane */
__device__ inline double tree(double *p, int t, double a) {
    p[t] = a;
    __syncthreads();
#pragma unroll
    for (int s = LANES / 2; s >= 1; s >>= 1) {
        if (t < s) p[t] = p[t] + p[t + s];
        __syncthreads();
    }
    return p[0];
}

/* the elements [i, i + 4) of one slab (cnt of them exist): o[k] for k < cnt */
template <typename T>
__device__ inline void load4(const T *__restrict__ p, bool vec, int cnt, T *o) {
    typedef VecT<T> A;
    if (vec) {
#pragma unroll
        for (int v = 0; v < 4 / A::W; v++) A::get(*(const typename A::vec *)(p + v * A::W), o + v * A::W);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = k < cnt ? p[k] : (T)0;
    }
}

template <typename T, bool IL>
__global__ __launch_bounds__(LANES) void gnorm_kernel(const hpnn_gnorm_seg *__restrict__ segs, int n_segs, T scale,
                                                      double *__restrict__ partials) {
    __shared__ double p[LANES];
    int y = 0;
    while (y < n_segs &&
           (unsigned long long)segs[y].first_block + hpnn_clip_blocks(segs[y].n) <= (unsigned long long)blockIdx.x)
        y++;
    if (y >= n_segs) return; /* past the table's last block: uniform for the workgroup */
    const hpnn_gnorm_seg sg = segs[y];
    const T *__restrict__ g = (const T *)sg.g;
    const size_t n = (size_t)sg.n, gs = (size_t)sg.gstride;
    const int t = threadIdx.x;
    const size_t i0 = (size_t)(blockIdx.x - sg.first_block) * BLOCK + 4 * (size_t)t;
    const int cnt = i0 >= n ? 0 : (n - i0 < 4 ? (int)(n - i0) : 4);
    const bool vec = cnt == 4 && ((uintptr_t)(g + i0) & 15u) == 0 && (sg.S <= 1 || (gs * sizeof(T)) % 16 == 0);
    T a[4] = {(T)0, (T)0, (T)0, (T)0};
    if (cnt > 0) {
        if constexpr (!IL) {
            for (int sl = 0; sl < sg.S; sl++) {
                T v[4];
                load4(g + (size_t)sl * gs + i0, vec, cnt, v);
#pragma unroll
                for (int k = 0; k < 4; k++) a[k] += v[k];
            }
        } else {
            /* p_w = the slabs w, w + 8, ... added in that order to 0, then ((p_0 + p_1) + ...) + p_7 */
            T pw[8][4];
#pragma unroll
            for (int w = 0; w < 8; w++)
#pragma unroll
                for (int k = 0; k < 4; k++) pw[w][k] = (T)0;
            for (int base = 0; base < sg.S; base += 8) {
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    if (base + w < sg.S) {
                        T v[4];
                        load4(g + (size_t)(base + w) * gs + i0, vec, cnt, v);
#pragma unroll
                        for (int k = 0; k < 4; k++) pw[w][k] += v[k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                a[k] = pw[0][k];
#pragma unroll
                for (int w = 1; w < 8; w++) a[k] += pw[w][k];
            }
        }
    }
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < cnt) {
            const T e = a[k] * scale;
            q += (double)e * (double)e;
        }
    }
    const double sum = tree(p, t, q);
    if (t == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(LANES) void clip_finalize_kernel(const double *__restrict__ partials, int count,
                                                              hpnn_clip_state *__restrict__ st) {
    __shared__ double p[LANES];
    if (blockIdx.x) return;
    const int t = threadIdx.x;
    double a = 0.0;
    for (int i = t; i < count; i += LANES) a += partials[i];
    const double sumsq = tree(p, t, a);
    if (t == 0) hpnn_clip_finalize(st, sumsq);
}

__global__ __launch_bounds__(64) void clip_commit_kernel(hpnn_clip_state *__restrict__ st,
                                                         hpnn_clip_record *__restrict__ hist,
                                                         unsigned int *__restrict__ cursor, unsigned int cap) {
    if (blockIdx.x || threadIdx.x) return;
    hpnn_clip_commit(st, hist, cursor, cap);
}

template <typename T>
int gnorm_launch(int interleaved, const hpnn_gnorm_seg *segs, int n_segs, int count, T scale, double *partials,
                 hipStream_t stream) {
    if (interleaved)
        hipLaunchKernelGGL((gnorm_kernel<T, true>), dim3(count), dim3(LANES), 0, stream, segs, n_segs, scale, partials);
    else
        hipLaunchKernelGGL((gnorm_kernel<T, false>), dim3(count), dim3(LANES), 0, stream, segs, n_segs, scale,
                           partials);
    return hpnn_upd::launched();
}

}  // namespace

extern "C" int hpnn_clip_preload(hipStream_t stream) {
    hipLaunchKernelGGL(hpnn_co_probe_kernel_clip, dim3(1), dim3(1), 0, stream);
    if (hipGetLastError() != hipSuccess) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_gnorm_table(int f64, hpnn_gnorm_seg *segs, const hpnn_gnorm_seg *host_segs, int n_segs, int *count,
                                hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || !host_segs || !count || n_segs < 1 || n_segs > HPNN_GNORM_MAX_SEGS)
        return -1;
    const int esize = f64 ? 8 : 4;
    hpnn_gnorm_seg h[HPNN_GNORM_MAX_SEGS];
    unsigned long long first = 0;
    for (int i = 0; i < n_segs; i++) {
        h[i] = host_segs[i];
        const hpnn_gnorm_seg &g = h[i];
        if (!g.g || ((uintptr_t)g.g & (uintptr_t)(esize - 1)) || g.S < 1 || g.gstride < 0 || g.n == 0) return -1;
        if (g.S > 1 && (unsigned long long)g.gstride < g.n) return -1; /* the slabs must not overlap */
        h[i].first_block = (int)first;
        first += hpnn_clip_blocks(g.n);
        if (first > 0x7fffffffull) return -1;
    }
    if (hipMemcpyAsync(segs, h, (size_t)n_segs * sizeof(hpnn_gnorm_seg), hipMemcpyHostToDevice, stream) != hipSuccess)
        return -5;
    if (hipStreamSynchronize(stream) != hipSuccess) return -5; /* h leaves scope: setup synchronises */
    *count = (int)first;
    return 0;
}

extern "C" int hpnn_gnorm_partials(int f64, int interleaved, const hpnn_gnorm_seg *segs, int n_segs, int count,
                                   double scale, double *partials, hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || n_segs < 1 || n_segs > HPNN_GNORM_MAX_SEGS || count < 1 || !partials ||
        ((uintptr_t)partials & 7u))
        return -1;
    if (f64) return gnorm_launch<double>(interleaved, segs, n_segs, count, scale, partials, stream);
    return gnorm_launch<float>(interleaved, segs, n_segs, count, (float)scale, partials, stream);
}

extern "C" int hpnn_clip_finalize_dev(const double *partials, int count, hpnn_clip_state *state, hipStream_t stream) {
    if (!partials || ((uintptr_t)partials & 7u) || count < 1 || !state || ((uintptr_t)state & 7u)) return -1;
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(LANES), 0, stream, partials, count, state);
    return hpnn_upd::launched();
}

extern "C" int hpnn_clip_commit_dev(hpnn_clip_state *state, hpnn_clip_record *hist, unsigned int *cursor,
                                    unsigned int cap, hipStream_t stream) {
    if (!state || ((uintptr_t)state & 7u) || ((uintptr_t)hist & 7u) || ((uintptr_t)cursor & 3u) || (hist && !cursor))
        return -1;
    hipLaunchKernelGGL(clip_commit_kernel, dim3(1), dim3(64), 0, stream, state, hist, cursor, cap);
    return hpnn_upd::launched();
}
