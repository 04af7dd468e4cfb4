/*
 * Learning-rate schedules inside the captured epoch graph ([lr_schedule], gfx950; rule in
 * <libhpnn/lrsched.h>, docs/DESIGN.md 3.2j).
 *
 *   hpnn_lr_advance_dev    one thread, the first launch of an epoch: hpnn_lr_advance on the device
 *                          state, the new rate appended to a device history and, under [train]
 *                          ADAM, stored into hpnn_adam_state::lr (the Adam advance of the next
 *                          step derives c1 and wd from it)
 *   hpnn_lr_plateau_dev    one thread, behind hpnn_validate_commit: hpnn_lr_plateau on the loss
 *                          sum of the pass just filed
 *   hpnn_sgd_sched_fp      the BP / BPM step of the FP64 / FP32 engines, every layer in one
 *                          launch: g = (slab[0] + ... + slab[S-1]) * scale in slab order, then the
 *                          element rule with the rate READ FROM THE STATE
 *   hpnn_sgd_sched_multi   the BF16 plan's BP / BPM step, every layer in one launch: the S split-K
 *                          slabs summed, the rule on the FP32 W32 / V32, then the BF16 W, W^T and
 *                          (where the layer has one) fragment-major W0f
 *
 * Like kernels_best.hip and kernels_adam.hip every number that changes (the rate) lives in a
 * device hpnn_lr_state and is read from memory when the launch runs, never baked in at capture: a
 * replayed graph of several epochs takes a new rate every epoch.  The thread that changes the
 * state is a launch of its own and its consumers later launches on the same stream: no thread of
 * an update advances, no workgroup waits for another.  No atomics; plain vector loads and stores.
 *
 * hpnn_sgd_sched_fp walks a device segment table built like hpnn_adam_table (at most
 * HPNN_SCHED_MAX_SEGS segments; segment y owns workgroups [first_block[y], first_block[y + 1]) of
 * the launch, at most SCHED_CAP each, and walks its chunks with a stride of its own workgroup
 * count).  A chunk is 16 bytes (float4 / double2).  The first chunk of a segment is the unaligned
 * head (the elements in front of W's first 16-byte boundary), the last one the tail; both, and
 * every chunk of a segment whose V, slab pointers or slab stride are not aligned like W, go
 * element by element through the same arithmetic, so the bits do not depend on the alignment.
 *
 * hpnn_sgd_sched_multi works on the 8 x 32 sub-tiles of hpnn_adam_update_multi, in its one
 * summation order whatever S is: wave w adds the slabs w, w + 8, w + 16, ... in that order to a
 * partial p_w that starts at 0, the partials meet in LDS and wave 0 adds them in wave order,
 * g = ((((((p_0 + p_1) + p_2) + p_3) + p_4) + p_5) + p_6) + p_7.  Wave 0 then applies the rule and
 * writes the BF16 copies at the addresses sgd_update_multi_sub_kernel writes them.  The zero
 * padding of W32 stays zero: g = 0 and v = 0 there.
 *
 * This unit is compiled with FP contraction off: nothing is fused, as on the host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <libhpnn/adam.h>
#include <libhpnn/lrsched.h>

#include "kernels.h"

HPNN_CO_PROBE(lrsched)

namespace {

constexpr int SCHED_THREADS = 256;

template <typename T>
struct SchedT;
template <>
struct SchedT<float> {
    typedef float4 vec;
    static constexpr int W = 4;
    static __device__ void elem(float lr, float alpha, int mom, float g, float *w, float *v) {
        hpnn_sgd_sched_elem_f32(lr, alpha, mom, g, w, v);
    }
    static __device__ void get(const vec &x, float *o) { o[0] = x.x, o[1] = x.y, o[2] = x.z, o[3] = x.w; }
    static __device__ vec put(const float *o) { return make_float4(o[0], o[1], o[2], o[3]); }
};
template <>
struct SchedT<double> {
    typedef double2 vec;
    static constexpr int W = 2;
    static __device__ void elem(double lr, double alpha, int mom, double g, double *w, double *v) {
        hpnn_sgd_sched_elem_f64(lr, alpha, mom, g, w, v);
    }
    static __device__ void get(const vec &x, double *o) { o[0] = x.x, o[1] = x.y; }
    static __device__ vec put(const double *o) { return make_double2(o[0], o[1]); }
};

/* workgroups of one segment per pass: one pass of the widest grid covers 4096 * 256 elements */
template <typename T>
constexpr int sched_cap() {
    return 4096 / SchedT<T>::W;
}

__global__ __launch_bounds__(64) void lr_advance_kernel(hpnn_lr_state *__restrict__ st,
                                                        hpnn_adam_state *__restrict__ adam, double *__restrict__ hist,
                                                        unsigned int *__restrict__ cursor, unsigned int cap) {
    if (blockIdx.x || threadIdx.x) return;
    hpnn_lr_advance(st);
    const double lr = st->lr;
    if (adam) adam->lr = lr;
    if (hist && cursor) {
        const unsigned int c = *cursor;
        if (c < cap) { /* a full history drops the record */
            hist[c] = lr;
            *cursor = c + 1u;
        }
    }
}

__global__ __launch_bounds__(64) void lr_plateau_kernel(const hpnn_val_record *__restrict__ vhist,
                                                        const unsigned int *__restrict__ vcursor,
                                                        hpnn_lr_state *__restrict__ st) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned int c = *vcursor;
    if (c == 0u) return;
    hpnn_lr_plateau(st, vhist[c - 1u].loss_sum);
}

template <typename T>
__global__ __launch_bounds__(SCHED_THREADS) void sgd_sched_fp_kernel(const hpnn_sched_seg *__restrict__ segs,
                                                                     int n_segs, T scale, T alpha, int momentum,
                                                                     const hpnn_lr_state *__restrict__ st) {
    typedef SchedT<T> A;
    typedef typename A::vec V;
    constexpr int W = A::W;
    int y = 0;
    while (y < n_segs && (unsigned int)segs[y].first_block + (unsigned int)segs[y].blocks <= blockIdx.x) y++;
    if (y >= n_segs) return;
    const hpnn_sched_seg sg = segs[y];
    T *__restrict__ w = (T *)sg.w;
    T *__restrict__ v = (T *)sg.v;
    const T *__restrict__ g = (const T *)sg.g;
    const int mom = momentum && v != nullptr;
    const size_t n = (size_t)sg.n, gs = (size_t)sg.gstride;
    /* head: the elements in front of W's first 16-byte boundary; chunk 0 is the head (it may be
     * empty), chunk c >= 1 the elements [head + (c - 1) W, + W) cut at n */
    const size_t head_max = (size_t)((16u - ((uintptr_t)w & 15u)) & 15u) / sizeof(T);
    const size_t head = head_max < n ? head_max : n;
    const size_t chunks = 1 + (n - head + W - 1) / W;
    const bool same = (((mom ? ((uintptr_t)v ^ (uintptr_t)w) : (uintptr_t)0) | ((uintptr_t)g ^ (uintptr_t)w)) & 15u) == 0 &&
                      (sg.S <= 1 || (gs * sizeof(T)) % 16 == 0);
    const T lr = (T)st->lr; /* the rate of this epoch, read when the launch runs */
    const size_t stride = (size_t)sg.blocks * SCHED_THREADS;
    for (size_t c = (size_t)(blockIdx.x - sg.first_block) * SCHED_THREADS + threadIdx.x; c < chunks; c += stride) {
        const size_t i0 = c ? head + (c - 1) * W : 0;
        const size_t end = c ? (i0 + W < n ? i0 + W : n) : head;
        const int cnt = (int)(end - i0);
        if (cnt <= 0) continue;
        if (c && same && cnt == W) {
            T ww[W], vv[W], gg[W];
            A::get(*(const V *)(w + i0), ww);
#pragma unroll
            for (int k = 0; k < W; k++) vv[k] = (T)0, gg[k] = (T)0;
            if (mom) A::get(*(const V *)(v + i0), vv);
            for (int s = 0; s < sg.S; s++) {
                T t[W];
                A::get(*(const V *)(g + (size_t)s * gs + i0), t);
#pragma unroll
                for (int k = 0; k < W; k++) gg[k] += t[k];
            }
#pragma unroll
            for (int k = 0; k < W; k++) A::elem(lr, alpha, mom, gg[k] * scale, &ww[k], &vv[k]);
            *(V *)(w + i0) = A::put(ww);
            if (mom) *(V *)(v + i0) = A::put(vv);
        } else {
#pragma unroll
            for (int k = 0; k < W; k++) {
                if (k >= cnt) break;
                const size_t i = i0 + k;
                T a = (T)0;
                for (int s = 0; s < sg.S; s++) a += g[(size_t)s * gs + i];
                T x = w[i], p = mom ? v[i] : (T)0;
                A::elem(lr, alpha, mom, a * scale, &x, &p);
                w[i] = x;
                if (mom) v[i] = p;
            }
        }
    }
}

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

struct SchedUpdArgs {
    hpnn_upd_layer L[HPNN_UPD_MAX];
    int tile0[HPNN_UPD_MAX + 1]; /* in sub-tiles */
    int n;
    int momentum;
    float alpha, scale;
};

__global__ __launch_bounds__(512) void sgd_sched_multi_kernel(SchedUpdArgs a, const hpnn_lr_state *__restrict__ st) {
    __shared__ f32x4 part[8][64];
    __shared__ float tilebuf[8][33];
    int l = 0;
    while (l + 1 < a.n && (int)blockIdx.x >= a.tile0[l + 1]) l++;
    const hpnn_upd_layer &L = a.L[l];
    const int local = blockIdx.x - a.tile0[l];
    const int tile = local >> 2, sub = local & 3;
    const int tiles_k = L.K / 32;
    const int tn = tile / tiles_k, tk = tile % tiles_k;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ty = lane >> 3, tx = lane & 7;
    const int n = tn * 32 + sub * 8 + ty, k = tk * 32 + tx * 4;
    const size_t idx = (size_t)n * L.K + k;
    /* the updating wave fetches its weights and momentum first: in flight with the slab loads */
    f32x4 wv = {0.f, 0.f, 0.f, 0.f}, mv = wv;
    if (w == 0) {
        wv = *(const f32x4 *)(L.W32 + idx);
        if (a.momentum) mv = *(const f32x4 *)(L.V32 + idx);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = w; s < L.S; s += 8) acc += *(const f32x4 *)(L.G + (long)s * L.gstride + idx);
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        f32x4 g = part[0][lane];
#pragma unroll
        for (int ww = 1; ww < 8; ww++) g += part[ww][lane];
        const float lr = (float)st->lr; /* the rate of this epoch, read when the launch runs */
        bf16x4 wb;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float x = wv[r], p = mv[r];
            hpnn_sgd_sched_elem_f32(lr, a.alpha, a.momentum, g[r] * a.scale, &x, &p);
            wv[r] = x, mv[r] = p;
            wb[r] = (__bf16)x;
            tilebuf[ty][tx * 4 + r] = x;
        }
        *(f32x4 *)(L.W32 + idx) = wv;
        if (a.momentum) *(f32x4 *)(L.V32 + idx) = mv;
        *(bf16x4 *)((__bf16 *)L.Wbf + idx) = wb;
        if (L.Wf) {
            /* MFMA-fragment-major copy (kernels.h): 4 consecutive k stay contiguous */
            const size_t fo = (((size_t)(n >> 4) * tiles_k + (k >> 5)) * 64 + (n & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7);
            *(bf16x4 *)((__bf16 *)L.Wf + fo) = wb;
        }
    }
    __syncthreads();
    if (w == 0) {
        /* transposed: lane writes Wt[k = tk*32 + lane/2][n = tn*32 + sub*8 + 4(lane&1) .. +3] */
        const int kk = lane >> 1, nh = (lane & 1) * 4;
        bf16x4 tb;
#pragma unroll
        for (int r = 0; r < 4; r++) tb[r] = (__bf16)tilebuf[nh + r][kk];
        *(bf16x4 *)((__bf16 *)L.Wt + (size_t)(tk * 32 + kk) * L.N + tn * 32 + sub * 8 + nh) = tb;
    }
}

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -5; }

/* the checks of one group of hpnn_sgd_sched_multi (nothing is launched before every group passed) */
int check_layers(const hpnn_upd_layer *layers, int n, int momentum) {
    for (int l = 0; l < n; l++) {
        const hpnn_upd_layer &L = layers[l];
        if (L.N < 32 || L.K < 32 || L.N % 32 || L.K % 32 || L.S < 1 || L.gstride < 0) return -2;
        /* 16-byte f32x4 vectors at s * gstride, 8-byte BF16 vectors */
        if (L.S > 1 && L.gstride % 4) return -2;
        if (!L.W32 || (momentum && !L.V32) || !L.G || !L.Wbf || !L.Wt) return -1;
        if ((((uintptr_t)L.W32 | (uintptr_t)(momentum ? L.V32 : L.W32) | (uintptr_t)L.G) & 15u) ||
            (((uintptr_t)L.Wbf | (uintptr_t)L.Wt | (uintptr_t)L.Wf) & 7u))
            return -2;
    }
    return 0;
}

}  // namespace

extern "C" int hpnn_lrsched_preload(hipStream_t stream) {
    hipLaunchKernelGGL(hpnn_co_probe_kernel_lrsched, dim3(1), dim3(1), 0, stream);
    if (hipGetLastError() != hipSuccess) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_lr_advance_dev(hpnn_lr_state *state, hpnn_adam_state *adam, double *hist,
                                   unsigned int *hist_cursor, unsigned int hist_cap, hipStream_t stream) {
    if (!state || ((uintptr_t)state & 7u) || ((uintptr_t)adam & 7u) || ((uintptr_t)hist & 7u) ||
        ((uintptr_t)hist_cursor & 3u) || (hist && !hist_cursor))
        return -1;
    hipLaunchKernelGGL(lr_advance_kernel, dim3(1), dim3(64), 0, stream, state, adam, hist, hist_cursor, hist_cap);
    return launched();
}

extern "C" int hpnn_lr_plateau_dev(const hpnn_val_record *vhist, const unsigned int *vcursor, hpnn_lr_state *state,
                                   hipStream_t stream) {
    if (!vhist || ((uintptr_t)vhist & 7u) || !vcursor || ((uintptr_t)vcursor & 3u) || !state ||
        ((uintptr_t)state & 7u))
        return -1;
    hipLaunchKernelGGL(lr_plateau_kernel, dim3(1), dim3(64), 0, stream, vhist, vcursor, state);
    return launched();
}

extern "C" int hpnn_sgd_sched_table(int f64, hpnn_sched_seg *segs, const hpnn_sched_seg *host_segs, int n_segs,
                                    int momentum, hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || !host_segs || n_segs < 1 || n_segs > HPNN_SCHED_MAX_SEGS) return -1;
    const int esize = f64 ? 8 : 4, Wd = 16 / esize, cap = 4096 / Wd;
    hpnn_sched_seg h[HPNN_SCHED_MAX_SEGS];
    int first = 0;
    for (int i = 0; i < n_segs; i++) {
        h[i] = host_segs[i];
        const hpnn_sched_seg &g = h[i];
        if (!g.w || (momentum && !g.v) || !g.g || g.S < 1 || g.gstride < 0 || g.n == 0) return -1;
        if (((uintptr_t)g.w | (uintptr_t)g.v | (uintptr_t)g.g) & (uintptr_t)(esize - 1)) return -1;
        if (g.S > 1 && (unsigned long long)g.gstride < g.n) return -1; /* the slabs must not overlap */
        /* the head chunk plus the chunks behind it, 256 per workgroup */
        const unsigned long long chunks = 1 + (g.n + Wd - 1) / Wd;
        const unsigned long long nb = (chunks + SCHED_THREADS - 1) / SCHED_THREADS;
        h[i].blocks = (int)(nb < (unsigned long long)cap ? nb : (unsigned long long)cap);
        h[i].first_block = first;
        first += h[i].blocks;
    }
    if (hipMemcpyAsync(segs, h, (size_t)n_segs * sizeof(hpnn_sched_seg), hipMemcpyHostToDevice, stream) != hipSuccess)
        return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5; /* h leaves scope: setup synchronises */
}

extern "C" int hpnn_sgd_sched_fp(int f64, const hpnn_sched_seg *segs, int n_segs, double scale, double alpha,
                                 int momentum, const hpnn_lr_state *state, hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || n_segs < 1 || n_segs > HPNN_SCHED_MAX_SEGS || !state ||
        ((uintptr_t)state & 7u))
        return -1;
    if (f64)
        hipLaunchKernelGGL(sgd_sched_fp_kernel<double>, dim3(n_segs * sched_cap<double>()), dim3(SCHED_THREADS), 0,
                           stream, segs, n_segs, scale, alpha, momentum, state);
    else
        hipLaunchKernelGGL(sgd_sched_fp_kernel<float>, dim3(n_segs * sched_cap<float>()), dim3(SCHED_THREADS), 0,
                           stream, segs, n_segs, (float)scale, (float)alpha, momentum, state);
    return launched();
}

extern "C" int hpnn_sgd_sched_multi(const hpnn_upd_layer *layers, int n, float alpha, float scale, int momentum,
                                    const hpnn_lr_state *state, hipStream_t stream) {
    if (!layers || n < 1 || n > 2 * HPNN_UPD_MAX || !state || ((uintptr_t)state & 7u)) return -1;
    const int rc = check_layers(layers, n, momentum);
    if (rc) return rc;
    /* nets deeper than HPNN_UPD_MAX layers go in groups, one launch each */
    for (int i0 = 0; i0 < n; i0 += HPNN_UPD_MAX) {
        SchedUpdArgs a;
        a.n = n - i0 < HPNN_UPD_MAX ? n - i0 : HPNN_UPD_MAX;
        a.momentum = momentum ? 1 : 0;
        a.alpha = alpha;
        a.scale = scale;
        int t = 0;
        for (int l = 0; l < a.n; l++) {
            a.L[l] = layers[i0 + l];
            a.tile0[l] = t;
            t += 4 * (a.L[l].N / 32) * (a.L[l].K / 32);
        }
        a.tile0[a.n] = t;
        hipLaunchKernelGGL(sgd_sched_multi_kernel, dim3(t), dim3(512), 0, stream, a, state);
        if (launched()) return -5;
    }
    return 0;
}
