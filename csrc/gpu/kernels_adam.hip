/*
 * The Adam trainer inside the captured epoch graph ([train] ADAM, gfx950; rule in
 * <libhpnn/adam.h>, docs/DESIGN.md 3.2i).
 *
 *   hpnn_adam_advance_dev  one thread: t += 1, p1 *= beta1, p2 *= beta2, then c1, s2, wd
 *   hpnn_adam_fp           one launch over every layer of the FP64 / FP32 engines:
 *                          g = (slab[0] + ... + slab[S-1]) * scale in slab order, then the rule
 *                          on W, M (first moment) and V (second moment)
 *   hpnn_adam_update_multi the BF16 plan's update, every layer in one launch: the S split-K
 *                          slabs summed, the rule on the FP32 W32 / V32 (= m) / A32 (= v), then
 *                          the BF16 W, W^T and (where the layer has one) fragment-major W0f
 *
 * Like kernels_best.hip and kernels_cg.hip every number that changes per step (c1, s2) lives in a
 * device hpnn_adam_state and is read from memory when the launch runs, never baked in at capture:
 * a replayed graph of about 32 steps takes a new bias correction every step.  The advance is a
 * launch of its own and its consumer a later launch on the same stream: no thread of the update
 * advances, no workgroup waits for another.  No atomics; plain vector loads and stores.
 *
 * The layers are the segments of a device table (at most HPNN_ADAM_MAX_SEGS, uploaded at setup by
 * hpnn_adam_table, which also fills the prefix of workgroups: segment y owns workgroups
 * [first_block[y], first_block[y + 1]) of the launch, at most ADAM_CAP each, and walks its
 * chunks with a stride of its own workgroup count).  The launch has n_segs * ADAM_CAP workgroups;
 * those past the last prefix entry return at once.
 *
 * A chunk is 16 bytes (float4 / double2).  The first chunk of a segment is the unaligned head
 * (the elements in front of W's first 16-byte boundary), the last one the tail; both, and every
 * chunk of a segment whose M, V, slab pointers or slab stride are not aligned like W, go element
 * by element through the same arithmetic, so the bits do not depend on the alignment.
 *
 * hpnn_adam_update_multi works on the 8 x 32 sub-tiles of sgd_update_multi_sub_kernel
 * (kernels_misc.hip): four workgroups of eight waves per 32 x 32 tile, one f32x4 per lane.  The
 * slab sum has ONE fixed order, whatever S is and independent of timing: wave w adds the slabs
 * w, w + 8, w + 16, ... in that order to a partial p_w that starts at 0, the partials meet in LDS
 * and wave 0 adds them in wave order, g = ((((((p_0 + p_1) + p_2) + p_3) + p_4) + p_5) + p_6) +
 * p_7 (a wave without a slab adds 0).  That is the order of neither SGD update kernel.  Wave 0
 * then applies the rule and writes the BF16 copies at the addresses sgd_update_multi_sub_kernel
 * writes them.  The zero padding of W32 stays zero: g = 0 there, so m = v = 0 and the step is 0.
 *
 * This unit is compiled with FP contraction off: nothing is fused, and the division and the
 * square root are the correctly rounded ones, as on the host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <libhpnn/adam.h>

#include "kernels.h"

HPNN_CO_PROBE(adam)

namespace {

constexpr int ADAM_THREADS = 256;

template <typename T>
struct AdamT;
template <>
struct AdamT<float> {
    typedef float4 vec;
    typedef hpnn_adam_coef_f32 coef;
    static constexpr int W = 4;
    static __device__ coef coef_of(const hpnn_adam_state *s) { return hpnn_adam_coef_f32_of(s); }
    static __device__ void elem(const coef &c, float g, float *w, float *m, float *v) {
        hpnn_adam_elem_f32(&c, g, w, m, v);
    }
    static __device__ void get(const vec &x, float *o) { o[0] = x.x, o[1] = x.y, o[2] = x.z, o[3] = x.w; }
    static __device__ vec put(const float *o) { return make_float4(o[0], o[1], o[2], o[3]); }
};
template <>
struct AdamT<double> {
    typedef double2 vec;
    typedef hpnn_adam_coef_f64 coef;
    static constexpr int W = 2;
    static __device__ coef coef_of(const hpnn_adam_state *s) { return hpnn_adam_coef_f64_of(s); }
    static __device__ void elem(const coef &c, double g, double *w, double *m, double *v) {
        hpnn_adam_elem_f64(&c, g, w, m, v);
    }
    static __device__ void get(const vec &x, double *o) { o[0] = x.x, o[1] = x.y; }
    static __device__ vec put(const double *o) { return make_double2(o[0], o[1]); }
};

/* workgroups of one segment per pass: one pass of the widest grid covers 4096 * 256 elements */
template <typename T>
constexpr int adam_cap() {
    return 4096 / AdamT<T>::W;
}

__global__ __launch_bounds__(64) void adam_advance_kernel(hpnn_adam_state *__restrict__ st) {
    if (blockIdx.x == 0 && threadIdx.x == 0) hpnn_adam_advance(st);
}

template <typename T>
__global__ __launch_bounds__(ADAM_THREADS) void adam_fp_kernel(const hpnn_adam_seg *__restrict__ segs, int n_segs,
                                                               T scale, const hpnn_adam_state *__restrict__ st) {
    typedef AdamT<T> A;
    typedef typename A::vec V;
    constexpr int W = A::W;
    int y = 0;
    while (y < n_segs && (unsigned int)segs[y].first_block + (unsigned int)segs[y].blocks <= blockIdx.x) y++;
    if (y >= n_segs) return;
    const hpnn_adam_seg sg = segs[y];
    T *__restrict__ w = (T *)sg.w;
    T *__restrict__ m = (T *)sg.m;
    T *__restrict__ v = (T *)sg.v;
    const T *__restrict__ g = (const T *)sg.g;
    const size_t n = (size_t)sg.n, gs = (size_t)sg.gstride;
    /* head: the elements in front of W's first 16-byte boundary; chunk 0 is the head (it may be
     * empty), chunk c >= 1 the elements [head + (c - 1) W, + W) cut at n */
    const size_t head_max = (size_t)((16u - ((uintptr_t)w & 15u)) & 15u) / sizeof(T);
    const size_t head = head_max < n ? head_max : n;
    const size_t chunks = 1 + (n - head + W - 1) / W;
    const bool same = ((((uintptr_t)m ^ (uintptr_t)w) | ((uintptr_t)v ^ (uintptr_t)w) | ((uintptr_t)g ^ (uintptr_t)w)) &
                       15u) == 0 &&
                      (sg.S <= 1 || (gs * sizeof(T)) % 16 == 0);
    const typename A::coef cf = A::coef_of(st);
    const size_t stride = (size_t)sg.blocks * ADAM_THREADS;
    for (size_t c = (size_t)(blockIdx.x - sg.first_block) * ADAM_THREADS + threadIdx.x; c < chunks; c += stride) {
        const size_t i0 = c ? head + (c - 1) * W : 0;
        const size_t end = c ? (i0 + W < n ? i0 + W : n) : head;
        const int cnt = (int)(end - i0);
        if (cnt <= 0) continue;
        T ww[W], mm[W], vv[W], gg[W];
        if (c && same && cnt == W) {
            A::get(*(const V *)(w + i0), ww);
            A::get(*(const V *)(m + i0), mm);
            A::get(*(const V *)(v + i0), vv);
#pragma unroll
            for (int k = 0; k < W; k++) gg[k] = (T)0;
            for (int s = 0; s < sg.S; s++) {
                T t[W];
                A::get(*(const V *)(g + (size_t)s * gs + i0), t);
#pragma unroll
                for (int k = 0; k < W; k++) gg[k] += t[k];
            }
#pragma unroll
            for (int k = 0; k < W; k++) A::elem(cf, gg[k] * scale, &ww[k], &mm[k], &vv[k]);
            *(V *)(w + i0) = A::put(ww);
            *(V *)(m + i0) = A::put(mm);
            *(V *)(v + i0) = A::put(vv);
        } else {
#pragma unroll
            for (int k = 0; k < W; k++) {
                if (k >= cnt) break;
                const size_t i = i0 + k;
                T a = (T)0;
                for (int s = 0; s < sg.S; s++) a += g[(size_t)s * gs + i];
                T x = w[i], p = m[i], q = v[i];
                A::elem(cf, a * scale, &x, &p, &q);
                w[i] = x;
                m[i] = p;
                v[i] = q;
            }
        }
    }
}

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

struct AdamUpdArgs {
    hpnn_adam_upd_layer L[HPNN_UPD_MAX];
    int tile0[HPNN_UPD_MAX + 1]; /* in sub-tiles */
    int n;
    float scale;
};

__global__ __launch_bounds__(512) void adam_update_multi_kernel(AdamUpdArgs a, const hpnn_adam_state *__restrict__ st) {
    __shared__ f32x4 part[8][64];
    __shared__ float tilebuf[8][33];
    int l = 0;
    while (l + 1 < a.n && (int)blockIdx.x >= a.tile0[l + 1]) l++;
    const hpnn_upd_layer &L = a.L[l].u;
    float *__restrict__ A32 = a.L[l].A32;
    const int local = blockIdx.x - a.tile0[l];
    const int tile = local >> 2, sub = local & 3;
    const int tiles_k = L.K / 32;
    const int tn = tile / tiles_k, tk = tile % tiles_k;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ty = lane >> 3, tx = lane & 7;
    const int n = tn * 32 + sub * 8 + ty, k = tk * 32 + tx * 4;
    const size_t idx = (size_t)n * L.K + k;
    /* the updating wave fetches its weights and moments first: in flight with the slab loads */
    f32x4 wv = {0.f, 0.f, 0.f, 0.f}, mv = wv, vv = wv;
    if (w == 0) {
        wv = *(const f32x4 *)(L.W32 + idx);
        mv = *(const f32x4 *)(L.V32 + idx);
        vv = *(const f32x4 *)(A32 + idx);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = w; s < L.S; s += 8) acc += *(const f32x4 *)(L.G + (long)s * L.gstride + idx);
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        f32x4 g = part[0][lane];
#pragma unroll
        for (int ww = 1; ww < 8; ww++) g += part[ww][lane];
        const hpnn_adam_coef_f32 cf = hpnn_adam_coef_f32_of(st);
        bf16x4 wb;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float x = wv[r], p = mv[r], q = vv[r];
            hpnn_adam_elem_f32(&cf, g[r] * a.scale, &x, &p, &q);
            wv[r] = x, mv[r] = p, vv[r] = q;
            wb[r] = (__bf16)x;
            tilebuf[ty][tx * 4 + r] = x;
        }
        *(f32x4 *)(L.W32 + idx) = wv;
        *(f32x4 *)(L.V32 + idx) = mv;
        *(f32x4 *)(A32 + idx) = vv;
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

}  // namespace

extern "C" int hpnn_adam_preload(hipStream_t stream) {
    hipLaunchKernelGGL(hpnn_co_probe_kernel_adam, dim3(1), dim3(1), 0, stream);
    if (hipGetLastError() != hipSuccess) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_adam_advance_dev(hpnn_adam_state *state, hipStream_t stream) {
    if (!state || ((uintptr_t)state & 7u)) return -1;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, stream, state);
    return launched();
}

extern "C" int hpnn_adam_table(int f64, hpnn_adam_seg *segs, const hpnn_adam_seg *host_segs, int n_segs,
                               hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || !host_segs || n_segs < 1 || n_segs > HPNN_ADAM_MAX_SEGS) return -1;
    const int esize = f64 ? 8 : 4, Wd = 16 / esize, cap = 4096 / Wd;
    hpnn_adam_seg h[HPNN_ADAM_MAX_SEGS];
    int first = 0;
    for (int i = 0; i < n_segs; i++) {
        h[i] = host_segs[i];
        const hpnn_adam_seg &g = h[i];
        if (!g.w || !g.m || !g.v || !g.g || g.S < 1 || g.gstride < 0 || g.n == 0) return -1;
        if (((uintptr_t)g.w | (uintptr_t)g.m | (uintptr_t)g.v | (uintptr_t)g.g) & (uintptr_t)(esize - 1)) return -1;
        if (g.S > 1 && (unsigned long long)g.gstride < g.n) return -1; /* the slabs must not overlap */
        /* the head chunk plus the chunks behind it, 256 per workgroup */
        const unsigned long long chunks = 1 + (g.n + Wd - 1) / Wd;
        const unsigned long long nb = (chunks + ADAM_THREADS - 1) / ADAM_THREADS;
        h[i].blocks = (int)(nb < (unsigned long long)cap ? nb : (unsigned long long)cap);
        h[i].first_block = first;
        first += h[i].blocks;
    }
    if (hipMemcpyAsync(segs, h, (size_t)n_segs * sizeof(hpnn_adam_seg), hipMemcpyHostToDevice, stream) != hipSuccess)
        return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5; /* h leaves scope: setup synchronises */
}

extern "C" int hpnn_adam_fp(int f64, const hpnn_adam_seg *segs, int n_segs, double scale,
                            const hpnn_adam_state *state, hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || n_segs < 1 || n_segs > HPNN_ADAM_MAX_SEGS || !state ||
        ((uintptr_t)state & 7u))
        return -1;
    if (f64)
        hipLaunchKernelGGL(adam_fp_kernel<double>, dim3(n_segs * adam_cap<double>()), dim3(ADAM_THREADS), 0, stream,
                           segs, n_segs, scale, state);
    else
        hipLaunchKernelGGL(adam_fp_kernel<float>, dim3(n_segs * adam_cap<float>()), dim3(ADAM_THREADS), 0, stream, segs,
                           n_segs, (float)scale, state);
    return launched();
}

extern "C" int hpnn_adam_update_multi(const hpnn_adam_upd_layer *layers, int n, float scale,
                                      const hpnn_adam_state *state, hipStream_t stream) {
    if (!layers || n < 1 || n > HPNN_UPD_MAX || !state || ((uintptr_t)state & 7u)) return -1;
    AdamUpdArgs a;
    a.n = n;
    a.scale = scale;
    int t = 0;
    for (int l = 0; l < n; l++) {
        const hpnn_upd_layer &L = layers[l].u;
        if (L.N < 32 || L.K < 32 || L.N % 32 || L.K % 32 || L.S < 1 || L.gstride < 0) return -2;
        /* 16-byte f32x4 vectors at s * gstride, 8-byte BF16 vectors */
        if (L.S > 1 && L.gstride % 4) return -2;
        if (!L.W32 || !L.V32 || !layers[l].A32 || !L.G || !L.Wbf || !L.Wt) return -1;
        if ((((uintptr_t)L.W32 | (uintptr_t)L.V32 | (uintptr_t)layers[l].A32 | (uintptr_t)L.G) & 15u) ||
            (((uintptr_t)L.Wbf | (uintptr_t)L.Wt | (uintptr_t)L.Wf) & 7u))
            return -2;
        a.L[l] = layers[l];
        a.tile0[l] = t;
        t += 4 * (L.N / 32) * (L.K / 32);
    }
    a.tile0[n] = t;
    hipLaunchKernelGGL(adam_update_multi_kernel, dim3(t), dim3(512), 0, stream, a, state);
    return launched();
}
