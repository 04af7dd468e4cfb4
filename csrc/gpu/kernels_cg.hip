/*
 * The conjugate-gradient trainer inside the captured epoch graph ([train] CG, gfx950).
 *
 *   hpnn_cg_accumulate  g = ((first ? 0 : g) + slab[0] + slab[1] + ...) * scale, in slab order
 *   hpnn_cg_dots        <g,g>, <g,g_prev>, <g,d> over every layer as FP64 sums of FP64 products
 *   hpnn_cg_direction   one thread: beta, the restart test and the trial steps (libhpnn/cg.h)
 *   hpnn_cg_begin       d = g + beta d, g_prev = g, W0 = W in one pass
 *   hpnn_cg_trial       W = W0 + a_j d
 *   hpnn_cg_loss        the output layer forward only: loss and argmax hits of a chunk of rows
 *                       added into CG's own stat slots, without atomics
 *   hpnn_cg_file        one trial's loss -> phi[j]; behind trial K-1 the choice of j* and of the
 *                       seventh point, behind the seventh trial a* and the history record
 *
 * Like kernels_best.hip and kernels_shuffle.hip every number the host would otherwise decide
 * (beta, the steps a_j, j*, a*) lives in a device hpnn_cg_state and is read from memory when the
 * launch runs, never baked in at capture: a replayed graph of several iterations takes a new
 * decision every iteration.  A decision is a launch of its own (one thread or one 64-lane
 * workgroup) and its consumer is a later launch on the same stream: no thread of a consumer
 * decides, no workgroup waits for another.  No atomics; plain vector loads and stores.
 *
 * The layers are the segments of a device table (at most HPNN_CG_MAX_SEGS, uploaded at setup):
 * workgroup (x, y) of an elementwise launch handles elements x * 256 + t, + X * 256, ... of
 * segment y.
 *
 * Rounding: begin and trial are ONE fma in T per element, d = fma((T)beta, d, g) and
 * W = fma((T)a_j, d, W0); beta = 0 gives d = g and a_j = 0 gives W = W0 as copies, bit for bit
 * (also for -0 and for a d that is not finite).  This unit is compiled with FP contraction off,
 * so the only fused operations are the ones written as fma.
 *
 * Dots: HPNN_CG_DOT_WGS workgroups of 256 threads.  The elements of a segment are cut into
 * chunks of 16 bytes; chunk c belongs to thread c mod (WGS * 256), which adds the chunk's
 * products in element order to three FP64 sums that run over all segments in table order.  A
 * workgroup adds its 256 sums with a fixed tree in LDS and writes one partial triple; the
 * finishing launch adds the partials in index order.  Nothing depends on timing or on the
 * alignment of the pointers (an unaligned chunk is loaded element by element, in the same
 * order), so the result is bitwise reproducible for any n.
 *
 * Loss: the line search compares sums of per-sample losses, so they must not depend on timing
 * either (the engines' output kernels add theirs with atomics).  hpnn_cg_loss runs exactly
 * HPNN_STAT_SLOTS workgroups of sixteen waves; wave w of workgroup s takes rows 16 s + w,
 * 16 s + w + 1024, ... of the chunk one after the other (the output layer and the loss exactly as
 * hpnn_output_fp computes them, one wave per row), adds their losses in that order in FP64, the
 * sixteen waves' sums meet in LDS in wave order, and thread 0 adds the result to slot s with a
 * plain load and store: slot s has one writer per launch, and the launches of a pass are in
 * stream order.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <libhpnn/cg.h>

#include "kernels.h"

HPNN_CO_PROBE(cg)

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_GRID_X = 64;

__device__ inline double cg_step(double a, double x, double y) { return hpnn_cg_step_f64(a, x, y); }
__device__ inline float cg_step(float a, float x, float y) { return hpnn_cg_step_f32(a, x, y); }

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void cg_accumulate_kernel(const hpnn_cg_seg *__restrict__ segs, int first,
                                                                   T scale) {
    const hpnn_cg_seg sg = segs[blockIdx.y];
    T *__restrict__ g = (T *)sg.g;
    const T *__restrict__ slab = (const T *)sg.slab;
    const size_t n = (size_t)sg.n, stride = (size_t)gridDim.x * CG_THREADS;
    for (size_t i = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += stride) {
        T acc = first ? (T)0 : g[i];
        for (int s = 0; s < sg.S; s++) acc += slab[(size_t)s * (size_t)sg.sstride + i];
        g[i] = acc * scale;
    }
}

template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
    typedef float4 type;
    static constexpr int W = 4;
    static __device__ void get(const float4 &v, float *o) { o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w; }
};
template <>
struct Vec16<double> {
    typedef double2 type;
    static constexpr int W = 2;
    static __device__ void get(const double2 &v, double *o) { o[0] = v.x, o[1] = v.y; }
};

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void cg_dots_kernel(const hpnn_cg_seg *__restrict__ segs, int n_segs,
                                                             double *__restrict__ partials) {
    typedef typename Vec16<T>::type V;
    constexpr int W = Vec16<T>::W;
    __shared__ double red[3][CG_THREADS];
    double gg = 0.0, gp = 0.0, gd = 0.0;
    const size_t stride = (size_t)gridDim.x * CG_THREADS;
    for (int y = 0; y < n_segs; y++) {
        const hpnn_cg_seg sg = segs[y];
        const T *__restrict__ g = (const T *)sg.g;
        const T *__restrict__ p = (const T *)sg.gprev;
        const T *__restrict__ d = (const T *)sg.d;
        const size_t n = (size_t)sg.n, chunks = (n + W - 1) / W;
        const bool aligned = ((((uintptr_t)g) | ((uintptr_t)p) | ((uintptr_t)d)) & 15u) == 0;
        for (size_t c = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; c < chunks; c += stride) {
            const size_t i0 = c * W;
            T a[W], b[W], e[W];
            if (aligned && i0 + W <= n) {
                Vec16<T>::get(*(const V *)(g + i0), a);
                Vec16<T>::get(*(const V *)(p + i0), b);
                Vec16<T>::get(*(const V *)(d + i0), e);
            } else {
#pragma unroll
                for (int k = 0; k < W; k++) {
                    const bool in = i0 + k < n;
                    a[k] = in ? g[i0 + k] : (T)0;
                    b[k] = in ? p[i0 + k] : (T)0;
                    e[k] = in ? d[i0 + k] : (T)0;
                }
            }
#pragma unroll
            for (int k = 0; k < W; k++) {
                if (i0 + k >= n) break;
                const double x = (double)a[k];
                gg += x * x;
                gp += x * (double)b[k];
                gd += x * (double)e[k];
            }
        }
    }
    red[0][threadIdx.x] = gg;
    red[1][threadIdx.x] = gp;
    red[2][threadIdx.x] = gd;
    __syncthreads();
    for (int h = CG_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
            red[2][threadIdx.x] += red[2][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partials[(size_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void cg_dots_finish_kernel(const double *__restrict__ partials, int n_partials,
                                                            hpnn_cg_state *__restrict__ st) {
    if (threadIdx.x != 0) return;
    double gg = 0.0, gp = 0.0, gd = 0.0;
    for (int i = 0; i < n_partials; i++) {
        gg += partials[(size_t)i * 3];
        gp += partials[(size_t)i * 3 + 1];
        gd += partials[(size_t)i * 3 + 2];
    }
    st->gg = gg;
    st->gp = gp;
    st->gd = gd;
}

__global__ __launch_bounds__(64) void cg_direction_kernel(hpnn_cg_state *__restrict__ st) {
    if (threadIdx.x != 0) return;
    hpnn_cg_state s = *st;
    hpnn_cg_rule_direction(&s);
    *st = s;
}

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void cg_begin_kernel(const hpnn_cg_seg *__restrict__ segs,
                                                              const hpnn_cg_state *__restrict__ st) {
    const hpnn_cg_seg sg = segs[blockIdx.y];
    const T beta = (T)st->beta;
    const T *__restrict__ g = (const T *)sg.g;
    const T *__restrict__ w = (const T *)sg.w;
    T *__restrict__ d = (T *)sg.d;
    T *__restrict__ gp = (T *)sg.gprev;
    T *__restrict__ w0 = (T *)sg.w0;
    const size_t n = (size_t)sg.n, stride = (size_t)gridDim.x * CG_THREADS;
    for (size_t i = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += stride) {
        const T gi = g[i];
        d[i] = cg_step(beta, d[i], gi);
        gp[i] = gi;
        w0[i] = w[i];
    }
}

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void cg_trial_kernel(const hpnn_cg_seg *__restrict__ segs,
                                                              const hpnn_cg_state *__restrict__ st, int j) {
    const hpnn_cg_seg sg = segs[blockIdx.y];
    const T a = (T)st->a[j];
    const T *__restrict__ d = (const T *)sg.d;
    const T *__restrict__ w0 = (const T *)sg.w0;
    T *__restrict__ w = (T *)sg.w;
    const size_t n = (size_t)sg.n, stride = (size_t)gridDim.x * CG_THREADS;
    for (size_t i = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += stride)
        w[i] = cg_step(a, d[i], w0[i]);
}

constexpr double CG_TINY = 1e-14, CG_LOG_TINY = -32.236191301916641; /* common.h TINY, ln(1e-14) */

template <typename T>
__device__ __forceinline__ T cg_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

/* sixteen waves a workgroup: a chunk of 4096 rows is four rows a wave */
constexpr int CG_LOSS_THREADS = 1024, CG_LOSS_WAVES = CG_LOSS_THREADS / 64;

template <typename T>
__global__ __launch_bounds__(CG_LOSS_THREADS) void cg_loss_kernel(const T *__restrict__ Z, int ldz,
                                                             const T *__restrict__ Tg, int ldt,
                                                             float *__restrict__ slots, int n_valid, int n_out,
                                                             int type) {
    __shared__ double wl[CG_LOSS_WAVES];
    __shared__ unsigned int wh[CG_LOSS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    unsigned int hits = 0u;
    for (int row = blockIdx.x * (CG_LOSS_WAVES) + wave; row < n_valid; row += HPNN_STAT_SLOTS * (CG_LOSS_WAVES)) {
        const T *z = Z + (size_t)row * ldz;
        const T *t_ = Tg + (size_t)row * ldt;
        T zmax = -INFINITY, den = 0;
        if (type == 2) {
            for (int c = lane; c < n_out; c += 64) zmax = fmax(zmax, z[c]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) zmax = fmax(zmax, __shfl_xor(zmax, o, 64));
            for (int c = lane; c < n_out; c += 64) den += exp(z[c] - zmax);
            den = cg_wave_sum(den);
            /* e^{z-1} / (TINY + sum e^{z-1}) in the max-shifted frame, as hpnn_output_fp */
            den += exp(fmin((T)CG_LOG_TINY + (T)1 - zmax, (T)(sizeof(T) == 8 ? 700 : 80)));
        }
        T loss = 0, bo = -INFINITY, bt = -INFINITY;
        int io = 1 << 30, it = 1 << 30;
        for (int c = lane; c < n_out; c += 64) {
            T o;
            if (type == 2) o = exp(z[c] - zmax) / den;
            else if (type == 0) o = (T)2 / ((T)1 + exp(-z[c])) - (T)1;
            else o = z[c];
            const T t = t_[c];
            if (type == 2) {
                if (o > (T)0) loss += t * log(o + (T)CG_TINY);
            } else {
                loss += (t - o) * (t - o);
            }
            if (t > bt) { bt = t; it = c; }
            if (o > bo) { bo = o; io = c; }
        }
        /* first maximum over the row (lowest index on ties) */
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const T ob = __shfl_xor(bo, o, 64), tb = __shfl_xor(bt, o, 64);
            const int oi = __shfl_xor(io, o, 64), ti = __shfl_xor(it, o, 64);
            if (ob > bo || (ob == bo && oi < io)) { bo = ob; io = oi; }
            if (tb > bt || (tb == bt && ti < it)) { bt = tb; it = ti; }
        }
        loss = cg_wave_sum(loss);
        acc += (double)(type == 2 ? -loss / (T)n_out : (T)0.5 * loss);
        hits += io == it ? 1u : 0u;
    }
    if (lane == 0) {
        wl[wave] = acc;
        wh[wave] = hits;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float *p = slots + (size_t)blockIdx.x * HPNN_STAT_STRIDE;
    double sum = ((const double *)p)[1];
    unsigned int h = ((const unsigned int *)p)[1];
    for (int w = 0; w < CG_LOSS_WAVES; w++) {
        sum += wl[w];
        h += wh[w];
    }
    ((double *)p)[1] = sum;
    ((unsigned int *)p)[1] = h;
}

/* the hpnn_validate_commit pattern on CG's own stat slots */
__global__ __launch_bounds__(64) void cg_file_kernel(float *__restrict__ slots, hpnn_cg_state *__restrict__ st,
                                                     hpnn_cg_record *__restrict__ hist, unsigned int j) {
    __shared__ double sl[HPNN_STAT_SLOTS];
    __shared__ unsigned int sh[HPNN_STAT_SLOTS];
    const unsigned int i = threadIdx.x;
    float *p = slots + (size_t)i * HPNN_STAT_STRIDE;
    sl[i] = (double)p[0] + ((const double *)p)[1];
    sh[i] = ((const unsigned int *)p)[1];
    p[0] = 0.f;
    ((unsigned int *)p)[1] = 0u;
    ((double *)p)[1] = 0.0;
    __syncthreads();
    if (i != 0) return;
    double loss = 0.0;
    unsigned int hits = 0;
    for (int k = 0; k < HPNN_STAT_SLOTS; k++) {
        loss += sl[k];
        hits += sh[k];
    }
    /* on the state in memory: a local copy indexed by j and j* would live in scratch */
    hpnn_cg_rule_file(st, hist, j, loss, hits);
}

int segs_ok(const hpnn_cg_seg *h, int n_segs, int esize) {
    if (n_segs < 1 || n_segs > HPNN_CG_MAX_SEGS || !h) return 0;
    for (int i = 0; i < n_segs; i++) {
        const hpnn_cg_seg &g = h[i];
        const uintptr_t all = (uintptr_t)g.w | (uintptr_t)g.w0 | (uintptr_t)g.g | (uintptr_t)g.gprev | (uintptr_t)g.d |
                              (uintptr_t)g.slab;
        if (all & (uintptr_t)(esize - 1)) return 0; /* element alignment; a null pointer is the caller's choice */
        if (g.S < 0 || g.sstride < 0) return 0;
    }
    return 1;
}

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -5; }

}  // namespace

extern "C" int hpnn_cg_preload(hipStream_t stream) {
    hipLaunchKernelGGL(hpnn_co_probe_kernel_cg, dim3(1), dim3(1), 0, stream);
    if (hipGetLastError() != hipSuccess) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_cg_table(int f64, hpnn_cg_seg *segs, const hpnn_cg_seg *host_segs, int n_segs,
                             hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || !segs_ok(host_segs, n_segs, f64 ? 8 : 4)) return -1;
    if (hipMemcpyAsync(segs, host_segs, (size_t)n_segs * sizeof(hpnn_cg_seg), hipMemcpyHostToDevice, stream) !=
        hipSuccess)
        return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

#define CG_SEG_ARGS_OK(segs, n_segs) ((segs) && !((uintptr_t)(segs) & 7u) && (n_segs) >= 1 && (n_segs) <= HPNN_CG_MAX_SEGS)
#define CG_STATE_OK(st) ((st) && !((uintptr_t)(st) & 7u))

extern "C" int hpnn_cg_accumulate(int f64, const hpnn_cg_seg *segs, int n_segs, int first, double scale,
                                  hipStream_t stream) {
    if (!CG_SEG_ARGS_OK(segs, n_segs)) return -1;
    const dim3 grid(CG_GRID_X, n_segs);
    if (f64)
        hipLaunchKernelGGL(cg_accumulate_kernel<double>, grid, dim3(CG_THREADS), 0, stream, segs, first, scale);
    else
        hipLaunchKernelGGL(cg_accumulate_kernel<float>, grid, dim3(CG_THREADS), 0, stream, segs, first, (float)scale);
    return launched();
}

extern "C" int hpnn_cg_dots(int f64, const hpnn_cg_seg *segs, int n_segs, double *partials, hpnn_cg_state *state,
                            hipStream_t stream) {
    if (!CG_SEG_ARGS_OK(segs, n_segs) || !partials || ((uintptr_t)partials & 7u) || !CG_STATE_OK(state)) return -1;
    if (f64)
        hipLaunchKernelGGL(cg_dots_kernel<double>, dim3(HPNN_CG_DOT_WGS), dim3(CG_THREADS), 0, stream, segs, n_segs,
                           partials);
    else
        hipLaunchKernelGGL(cg_dots_kernel<float>, dim3(HPNN_CG_DOT_WGS), dim3(CG_THREADS), 0, stream, segs, n_segs,
                           partials);
    if (launched()) return -5;
    hipLaunchKernelGGL(cg_dots_finish_kernel, dim3(1), dim3(64), 0, stream, partials, HPNN_CG_DOT_WGS, state);
    return launched();
}

extern "C" int hpnn_cg_direction(hpnn_cg_state *state, hipStream_t stream) {
    if (!CG_STATE_OK(state)) return -1;
    hipLaunchKernelGGL(cg_direction_kernel, dim3(1), dim3(64), 0, stream, state);
    return launched();
}

extern "C" int hpnn_cg_begin(int f64, const hpnn_cg_seg *segs, int n_segs, const hpnn_cg_state *state,
                             hipStream_t stream) {
    if (!CG_SEG_ARGS_OK(segs, n_segs) || !CG_STATE_OK(state)) return -1;
    const dim3 grid(CG_GRID_X, n_segs);
    if (f64) hipLaunchKernelGGL(cg_begin_kernel<double>, grid, dim3(CG_THREADS), 0, stream, segs, state);
    else hipLaunchKernelGGL(cg_begin_kernel<float>, grid, dim3(CG_THREADS), 0, stream, segs, state);
    return launched();
}

extern "C" int hpnn_cg_trial(int f64, const hpnn_cg_seg *segs, int n_segs, const hpnn_cg_state *state, int j,
                             hipStream_t stream) {
    if (!CG_SEG_ARGS_OK(segs, n_segs) || !CG_STATE_OK(state) || j < 0 || j > HPNN_CG_FINAL) return -1;
    const dim3 grid(CG_GRID_X, n_segs);
    if (f64) hipLaunchKernelGGL(cg_trial_kernel<double>, grid, dim3(CG_THREADS), 0, stream, segs, state, j);
    else hipLaunchKernelGGL(cg_trial_kernel<float>, grid, dim3(CG_THREADS), 0, stream, segs, state, j);
    return launched();
}

extern "C" int hpnn_cg_loss(int f64, const void *Z, int ldz, const void *T, int ldt, float *slots, int n_valid,
                            int n_out, int type, hipStream_t stream) {
    if (!Z || !T || !slots || ((uintptr_t)slots & 7u) || n_valid < 0 || n_out < 1 || ldz < n_out || ldt < n_out ||
        type < 0 || type > 2)
        return -1;
    if (f64)
        hipLaunchKernelGGL(cg_loss_kernel<double>, dim3(HPNN_STAT_SLOTS), dim3(CG_LOSS_THREADS), 0, stream,
                           (const double *)Z, ldz, (const double *)T, ldt, slots, n_valid, n_out, type);
    else
        hipLaunchKernelGGL(cg_loss_kernel<float>, dim3(HPNN_STAT_SLOTS), dim3(CG_LOSS_THREADS), 0, stream, (const float *)Z,
                           ldz, (const float *)T, ldt, slots, n_valid, n_out, type);
    return launched();
}

extern "C" int hpnn_cg_file(float *slots, hpnn_cg_state *state, hpnn_cg_record *hist, int j,
                                   hipStream_t stream) {
    if (!slots || ((uintptr_t)slots & 7u) || !CG_STATE_OK(state) || ((uintptr_t)hist & 7u) || j < 0 ||
        j > HPNN_CG_FINAL)
        return -1;
    hipLaunchKernelGGL(cg_file_kernel, dim3(1), dim3(HPNN_STAT_SLOTS), 0, stream, slots, state, hist, (unsigned int)j);
    return launched();
}
