/*
 * The machinery the update kernels share (gfx950; docs/DESIGN.md 3.2i): one segment walker for the
 * FP64 / FP32 engines, one 8 x 32 sub-tile update for the BF16 plan, and their host sides.
 * kernels_adam.hip and kernels_lrsched.hip each add a RULE and thin wrappers.
 *
 * A rule R<T> (T the master type, float or double) names
 *   seg, layer, state   its segment struct, its BF16-plan layer descriptor (base(): the
 *                       hpnn_upd_layer inside), its device state
 *   args                what a launch takes by value; args::scale multiplies the slab sum
 *   NS, arrays()        the state arrays beside W of a segment / a layer, and whether this launch
 *                       uses them (false: they are neither loaded nor stored and the rule sees 0)
 *   coef, read()        its per-launch numbers, read from the device state WHEN THE LAUNCH RUNS
 *   elem()              the element rule on w and the NS state values e[]
 * Everything else is here, once.
 *
 * The segment walker.  The segments are a device table (at most SEG_MAX, uploaded at setup by
 * seg_table, which also fills the prefix of workgroups: segment y owns workgroups [first_block[y],
 * first_block[y + 1]) of the launch, at most seg_cap each, and walks its chunks with a stride of
 * its own workgroup count).  The launch has n_segs * seg_cap workgroups; those past the last
 * prefix entry return at once.  A chunk is 16 bytes (float4 / double2).  The first chunk of a
 * segment is the unaligned head (the elements in front of W's first 16-byte boundary), the last
 * one the tail; both, and every chunk of a segment whose state arrays, slab pointer or slab stride
 * are not aligned like W, go element by element through the same arithmetic, so the bits do not
 * depend on the alignment.  g = (slab[0] + ... + slab[S-1]) * scale, in slab order from 0.
 *
 * The sub-tile update works on the 8 x 32 sub-tiles of sgd_update_multi_sub_kernel
 * (kernels_misc.hip, which keeps its own copy of the geometry and of the BF16 epilogue: its
 * machine code must not move): four workgroups of eight waves per 32 x 32 tile, one f32x4 per
 * lane.  The slab sum has ONE fixed order, whatever S is and independent of timing: wave w adds
 * the slabs w, w + 8, w + 16, ... in that order to a partial p_w that starts at 0, the partials
 * meet in LDS and wave 0 adds them in wave order, g = ((((((p_0 + p_1) + p_2) + p_3) + p_4) + p_5)
 * + p_6) + p_7 (a wave without a slab adds 0).  That is the order of neither SGD update kernel.
 * Wave 0 then applies the rule in FP32 and writes the BF16 W, the fragment-major Wf and, through
 * LDS, W^T, at the addresses sgd_update_multi_sub_kernel writes them.  The zero padding of W32
 * stays zero as long as the rule keeps w at g = 0 with zero state.
 *
 * No thread advances a state, no workgroup waits for another, no atomics; plain vector loads and
 * stores.  The two units that instantiate the kernels are compiled with FP contraction off.
 */
#ifndef HPNN_GPU_UPD_COMMON_H
#define HPNN_GPU_UPD_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frag_major.h"
#include "kernels.h"

namespace hpnn_upd {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -5; }

/* ------------------------------------------------------------------ the segment walker */
constexpr int SEG_THREADS = 256;
constexpr int SEG_MAX = 16;

template <typename T>
struct VecT;
template <>
struct VecT<float> {
    typedef float4 vec;
    static constexpr int W = 4;
    static __device__ void get(const vec &x, float *o) { o[0] = x.x, o[1] = x.y, o[2] = x.z, o[3] = x.w; }
    static __device__ vec put(const float *o) { return make_float4(o[0], o[1], o[2], o[3]); }
};
template <>
struct VecT<double> {
    typedef double2 vec;
    static constexpr int W = 2;
    static __device__ void get(const vec &x, double *o) { o[0] = x.x, o[1] = x.y; }
    static __device__ vec put(const double *o) { return make_double2(o[0], o[1]); }
};

/* workgroups of one segment per pass: one pass of the widest grid covers 4096 * 256 elements */
constexpr int seg_cap(int esize) { return 4096 / (16 / esize); }

template <class R>
__global__ __launch_bounds__(SEG_THREADS) void seg_walk_kernel(const typename R::seg *__restrict__ segs, int n_segs,
                                                               typename R::args ra,
                                                               const typename R::state *__restrict__ st) {
    typedef typename R::type T;
    typedef VecT<T> A;
    typedef typename A::vec V;
    constexpr int W = A::W, NS = R::NS;
    int y = 0;
    while (y < n_segs && (unsigned int)segs[y].first_block + (unsigned int)segs[y].blocks <= blockIdx.x) y++;
    if (y >= n_segs) return;
    const typename R::seg sg = segs[y];
    T *__restrict__ w = (T *)sg.w;
    const T *__restrict__ g = (const T *)sg.g;
    T *s[NS];
    const bool on = R::arrays(sg, ra, s);
    const size_t n = (size_t)sg.n, gs = (size_t)sg.gstride;
    /* head: the elements in front of W's first 16-byte boundary; chunk 0 is the head (it may be
     * empty), chunk c >= 1 the elements [head + (c - 1) W, + W) cut at n */
    const size_t head_max = (size_t)((16u - ((uintptr_t)w & 15u)) & 15u) / sizeof(T);
    const size_t head = head_max < n ? head_max : n;
    const size_t chunks = 1 + (n - head + W - 1) / W;
    uintptr_t off = 0; /* the arrays in use against W, modulo 16 bytes */
#pragma unroll
    for (int j = 0; j < NS; j++) off |= on ? (uintptr_t)s[j] ^ (uintptr_t)w : (uintptr_t)0;
    const bool same = ((off | ((uintptr_t)g ^ (uintptr_t)w)) & 15u) == 0 && (sg.S <= 1 || (gs * sizeof(T)) % 16 == 0);
    const typename R::coef cf = R::read(ra, on, st);
    const T scale = ra.scale;
    const size_t stride = (size_t)sg.blocks * SEG_THREADS;
    for (size_t c = (size_t)(blockIdx.x - sg.first_block) * SEG_THREADS + threadIdx.x; c < chunks; c += stride) {
        const size_t i0 = c ? head + (c - 1) * W : 0;
        const size_t end = c ? (i0 + W < n ? i0 + W : n) : head;
        const int cnt = (int)(end - i0);
        if (cnt <= 0) continue;
        if (c && same && cnt == W) {
            T ww[W], gg[W], ss[W][NS]; /* ss[k]: the state values of element k */
            A::get(*(const V *)(w + i0), ww);
#pragma unroll
            for (int k = 0; k < W; k++) gg[k] = (T)0;
#pragma unroll
            for (int j = 0; j < NS; j++) {
                T t[W];
#pragma unroll
                for (int k = 0; k < W; k++) t[k] = (T)0;
                if (on) A::get(*(const V *)(s[j] + i0), t);
#pragma unroll
                for (int k = 0; k < W; k++) ss[k][j] = t[k];
            }
            for (int sl = 0; sl < sg.S; sl++) {
                T t[W];
                A::get(*(const V *)(g + (size_t)sl * gs + i0), t);
#pragma unroll
                for (int k = 0; k < W; k++) gg[k] += t[k];
            }
#pragma unroll
            for (int k = 0; k < W; k++) R::elem(cf, gg[k] * scale, &ww[k], ss[k]);
            *(V *)(w + i0) = A::put(ww);
            if (on) {
#pragma unroll
                for (int j = 0; j < NS; j++) {
                    T t[W];
#pragma unroll
                    for (int k = 0; k < W; k++) t[k] = ss[k][j];
                    *(V *)(s[j] + i0) = A::put(t);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < W; k++) {
                if (k >= cnt) break;
                const size_t i = i0 + k;
                T a = (T)0;
                for (int sl = 0; sl < sg.S; sl++) a += g[(size_t)sl * gs + i];
                T x = w[i], e[NS];
#pragma unroll
                for (int j = 0; j < NS; j++) e[j] = on ? s[j][i] : (T)0;
                R::elem(cf, a * scale, &x, e);
                w[i] = x;
                if (on) {
#pragma unroll
                    for (int j = 0; j < NS; j++) s[j][i] = e[j];
                }
            }
        }
    }
}

/* the launch of the walker over a device table; -1: refused */
template <class R>
int seg_walk(const typename R::seg *segs, int n_segs, const typename R::args &ra, const typename R::state *state,
             hipStream_t stream) {
    if (!segs || ((uintptr_t)segs & 7u) || n_segs < 1 || n_segs > SEG_MAX || !state || ((uintptr_t)state & 7u))
        return -1;
    hipLaunchKernelGGL(seg_walk_kernel<R>, dim3(n_segs * seg_cap(sizeof(typename R::type))), dim3(SEG_THREADS), 0,
                       stream, segs, n_segs, ra, state);
    return launched();
}

/* checks a host table (-1: refused, nothing written), fills blocks / first_block and copies it to
 * the device.  ptrs(seg, all) ORs every pointer of the segment into `all` (for the element
 * alignment) and returns whether each one that must not be null is set. */
template <class Seg, class Ptrs>
int seg_table(int f64, Seg *segs, const Seg *host_segs, int n_segs, hipStream_t stream, Ptrs ptrs) {
    if (!segs || ((uintptr_t)segs & 7u) || !host_segs || n_segs < 1 || n_segs > SEG_MAX) return -1;
    const int esize = f64 ? 8 : 4, Wd = 16 / esize, cap = seg_cap(esize);
    Seg h[SEG_MAX];
    int first = 0;
    for (int i = 0; i < n_segs; i++) {
        h[i] = host_segs[i];
        const Seg &g = h[i];
        uintptr_t all = 0;
        if (!ptrs(g, all) || g.S < 1 || g.gstride < 0 || g.n == 0) return -1;
        if (all & (uintptr_t)(esize - 1)) return -1;
        if (g.S > 1 && (unsigned long long)g.gstride < g.n) return -1; /* the slabs must not overlap */
        /* the head chunk plus the chunks behind it, 256 per workgroup */
        const unsigned long long chunks = 1 + (g.n + Wd - 1) / Wd;
        const unsigned long long nb = (chunks + SEG_THREADS - 1) / SEG_THREADS;
        h[i].blocks = (int)(nb < (unsigned long long)cap ? nb : (unsigned long long)cap);
        h[i].first_block = first;
        first += h[i].blocks;
    }
    if (hipMemcpyAsync(segs, h, (size_t)n_segs * sizeof(Seg), hipMemcpyHostToDevice, stream) != hipSuccess) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5; /* h leaves scope: setup synchronises */
}

/* ------------------------------------------------------------------ the 8 x 32 sub-tile update */
template <class R>
struct TileArgs {
    typename R::layer L[HPNN_UPD_MAX];
    int tile0[HPNN_UPD_MAX + 1]; /* the prefix of workgroups (sub-tiles) over the n layers */
    int n;
    typename R::args ra;
};

template <class R>
__global__ __launch_bounds__(512) void upd_tile_kernel(TileArgs<R> a, const typename R::state *__restrict__ st) {
    constexpr int NS = R::NS;
    __shared__ f32x4 part[8][64];
    __shared__ float tilebuf[8][33];
    int l = 0;
    while (l + 1 < a.n && (int)blockIdx.x >= a.tile0[l + 1]) l++;
    const hpnn_upd_layer &L = R::base(a.L[l]);
    float *s[NS];
    const bool on = R::arrays(a.L[l], a.ra, s);
    /* workgroup `local` of the layer: sub-tile `sub` (8 rows) of the 32 x 32 tile (tn, tk); lane
     * (ty, tx) of wave w owns row n, columns k .. k + 3 */
    const int local = blockIdx.x - a.tile0[l];
    const int tile = local >> 2, sub = local & 3;
    const int tiles_k = L.K / 32;
    const int tn = tile / tiles_k, tk = tile % tiles_k;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ty = lane >> 3, tx = lane & 7;
    const int n = tn * 32 + sub * 8 + ty, k = tk * 32 + tx * 4;
    const size_t idx = (size_t)n * L.K + k;
    /* the updating wave fetches its weights and state first: in flight with the slab loads */
    f32x4 wv = {0.f, 0.f, 0.f, 0.f}, sv[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) sv[j] = wv;
    if (w == 0) {
        wv = *(const f32x4 *)(L.W32 + idx);
        if (on) {
#pragma unroll
            for (int j = 0; j < NS; j++) sv[j] = *(const f32x4 *)(s[j] + idx);
        }
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int sl = w; sl < L.S; sl += 8) acc += *(const f32x4 *)(L.G + (long)sl * L.gstride + idx);
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0) {
        f32x4 g = part[0][lane];
#pragma unroll
        for (int ww = 1; ww < 8; ww++) g += part[ww][lane];
        const typename R::coef cf = R::read(a.ra, on, st);
        bf16x4 wb;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float x = wv[r], e[NS];
#pragma unroll
            for (int j = 0; j < NS; j++) e[j] = sv[j][r];
            R::elem(cf, g[r] * a.ra.scale, &x, e);
            wv[r] = x;
#pragma unroll
            for (int j = 0; j < NS; j++) sv[j][r] = e[j];
            wb[r] = (__bf16)x;
            tilebuf[ty][tx * 4 + r] = x;
        }
        *(f32x4 *)(L.W32 + idx) = wv;
        if (on) {
#pragma unroll
            for (int j = 0; j < NS; j++) *(f32x4 *)(s[j] + idx) = sv[j];
        }
        *(bf16x4 *)((__bf16 *)L.Wbf + idx) = wb;
        /* MFMA-fragment-major copy (frag_major.h): 4 consecutive k stay contiguous */
        if (L.Wf) *(bf16x4 *)((__bf16 *)L.Wf + hpnn_frag_major_offset(n, k, L.K)) = wb;
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

/* every layer checked (-1 a null pointer, -2 shape / alignment; nothing is launched before every
 * layer passed), then groups of HPNN_UPD_MAX layers, one launch each */
template <class R>
int upd_tile(const typename R::layer *layers, int n, const typename R::args &ra, const typename R::state *state,
             hipStream_t stream) {
    for (int l = 0; l < n; l++) {
        const hpnn_upd_layer &L = R::base(layers[l]);
        if (L.N < 32 || L.K < 32 || L.N % 32 || L.K % 32 || L.S < 1 || L.gstride < 0) return -2;
        /* 16-byte f32x4 vectors at s * gstride, 8-byte BF16 vectors */
        if (L.S > 1 && L.gstride % 4) return -2;
        float *s[R::NS];
        uintptr_t f32 = (uintptr_t)L.W32 | (uintptr_t)L.G;
        bool null = !L.W32 || !L.G || !L.Wbf || !L.Wt;
        if (R::arrays(layers[l], ra, s))
            for (int j = 0; j < R::NS; j++) null |= !s[j], f32 |= (uintptr_t)s[j];
        if (null) return -1;
        if ((f32 & 15u) || (((uintptr_t)L.Wbf | (uintptr_t)L.Wt | (uintptr_t)L.Wf) & 7u)) return -2;
    }
    for (int i0 = 0; i0 < n; i0 += HPNN_UPD_MAX) {
        TileArgs<R> a;
        a.n = n - i0 < HPNN_UPD_MAX ? n - i0 : HPNN_UPD_MAX;
        a.ra = ra;
        int t = 0;
        for (int l = 0; l < a.n; l++) {
            a.L[l] = layers[i0 + l];
            a.tile0[l] = t;
            t += 4 * (R::base(a.L[l]).N / 32) * (R::base(a.L[l]).K / 32);
        }
        a.tile0[a.n] = t;
        hipLaunchKernelGGL(upd_tile_kernel<R>, dim3(t), dim3(512), 0, stream, a, state);
        if (launched()) return -5;
    }
    return 0;
}

}  // namespace hpnn_upd

#endif /* HPNN_GPU_UPD_COMMON_H */
