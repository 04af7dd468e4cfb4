/*
 * The Adam trainer inside the captured epoch graph ([train] ADAM, gfx950; rule in
 * <libhpnn/adam.h>, docs/DESIGN.md 3.2i).
 *
 *   hpnn_adam_advance_dev  one thread: t += 1, p1 *= beta1, p2 *= beta2, then c1, s2, wd
 *   hpnn_adam_fp           the segment walker of upd_common.h over every layer of the FP64 / FP32
 *                          engines with the rule on W, M (first moment) and V (second moment)
 *   hpnn_adam_update_multi the sub-tile update of upd_common.h, the BF16 plan's update: the rule
 *                          on the FP32 W32 / V32 (= m) / A32 (= v)
 *
 * Like kernels_best.hip and kernels_cg.hip every number that changes per step (c1, s2) lives in a
 * device hpnn_adam_state and is read from memory when the launch runs, never baked in at capture:
 * a replayed graph of about 32 steps takes a new bias correction every step.  The advance is a
 * launch of its own and its consumer a later launch on the same stream.
 *
 * The zero padding of W32 stays zero: g = 0 there, so m = v = 0 and the step is 0.
 *
 * This unit is compiled with FP contraction off: nothing is fused, and the division and the
 * square root are the correctly rounded ones, as on the host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include <libhpnn/adam.h>
#include <libhpnn/clip.h>

#include "kernels.h"
#include "upd_common.h"

HPNN_CO_PROBE(adam)

namespace {

static_assert(HPNN_ADAM_MAX_SEGS == hpnn_upd::SEG_MAX, "one table size");

template <typename T>
struct AdamRule {
    typedef T type;
    typedef hpnn_adam_seg seg;
    typedef hpnn_adam_upd_layer layer;
    typedef hpnn_adam_state state;
    struct coef {
        std::conditional_t<sizeof(T) == 8, hpnn_adam_coef_f64, hpnn_adam_coef_f32> c;
        T clipf; /* (T)clip->factor, in use when clip */
        int clip;
    };
    struct args {
        T scale;
        const hpnn_clip_state *clip; /* [clip]: NULL = off */
    };
    static constexpr int NS = 2; /* the first and the second moment, always in use */
    /* a segment's arrays: the walker alone asks (the table builder has its own pointer check) */
    static __device__ bool arrays(const seg &g, const args &, T **s) {
        s[0] = (T *)g.m;
        s[1] = (T *)g.v;
        return true;
    }
    /* a layer's arrays: the sub-tile kernel and, on the host, the layer check of upd_tile */
    static __host__ __device__ bool arrays(const layer &L, const args &, float **s) {
        s[0] = L.u.V32;
        s[1] = L.A32;
        return true;
    }
    static __host__ __device__ const hpnn_upd_layer &base(const layer &L) { return L.u; }
    /* the coefficients the last advance left in the state */
    static __device__ coef read(const args &a, bool, const state *st) {
        const T clipf = a.clip ? (T)a.clip->factor : (T)1;
        if constexpr (sizeof(T) == 8)
            return {hpnn_adam_coef_f64_of(st), clipf, a.clip != nullptr};
        else
            return {hpnn_adam_coef_f32_of(st), clipf, a.clip != nullptr};
    }
    static __device__ void elem(const coef &c, T g, T *w, T *e) {
        if (c.clip) g = g * c.clipf;
        if constexpr (sizeof(T) == 8)
            hpnn_adam_elem_f64(&c.c, g, w, e, e + 1);
        else
            hpnn_adam_elem_f32(&c.c, g, w, e, e + 1);
    }
};

__global__ __launch_bounds__(64) void adam_advance_kernel(hpnn_adam_state *__restrict__ st) {
    if (blockIdx.x == 0 && threadIdx.x == 0) hpnn_adam_advance(st);
}

}  // namespace

extern "C" int hpnn_adam_preload(hipStream_t stream) {
    hipLaunchKernelGGL(hpnn_co_probe_kernel_adam, dim3(1), dim3(1), 0, stream);
    if (hipGetLastError() != hipSuccess) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_adam_advance_dev(hpnn_adam_state *state, hipStream_t stream) {
    if (!state || ((uintptr_t)state & 7u)) return -1;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, stream, state);
    return hpnn_upd::launched();
}

extern "C" int hpnn_adam_table(int f64, hpnn_adam_seg *segs, const hpnn_adam_seg *host_segs, int n_segs,
                               hipStream_t stream) {
    return hpnn_upd::seg_table(f64, segs, host_segs, n_segs, stream, [](const hpnn_adam_seg &g, uintptr_t &all) {
        all = (uintptr_t)g.w | (uintptr_t)g.m | (uintptr_t)g.v | (uintptr_t)g.g;
        return g.w && g.m && g.v && g.g;
    });
}

extern "C" int hpnn_adam_fp_clip(int f64, const hpnn_adam_seg *segs, int n_segs, double scale,
                                 const hpnn_adam_state *state, const hpnn_clip_state *clip, hipStream_t stream) {
    if ((uintptr_t)clip & 7u) return -1;
    if (f64) return hpnn_upd::seg_walk<AdamRule<double>>(segs, n_segs, {scale, clip}, state, stream);
    return hpnn_upd::seg_walk<AdamRule<float>>(segs, n_segs, {(float)scale, clip}, state, stream);
}

extern "C" int hpnn_adam_fp(int f64, const hpnn_adam_seg *segs, int n_segs, double scale,
                            const hpnn_adam_state *state, hipStream_t stream) {
    return hpnn_adam_fp_clip(f64, segs, n_segs, scale, state, nullptr, stream);
}

extern "C" int hpnn_adam_update_multi_clip(const hpnn_adam_upd_layer *layers, int n, float scale,
                                           const hpnn_adam_state *state, const hpnn_clip_state *clip,
                                           hipStream_t stream) {
    if (!layers || n < 1 || n > HPNN_UPD_MAX || !state || (((uintptr_t)state | (uintptr_t)clip) & 7u)) return -1;
    return hpnn_upd::upd_tile<AdamRule<float>>(layers, n, {scale, clip}, state, stream);
}

extern "C" int hpnn_adam_update_multi(const hpnn_adam_upd_layer *layers, int n, float scale,
                                      const hpnn_adam_state *state, hipStream_t stream) {
    return hpnn_adam_update_multi_clip(layers, n, scale, state, nullptr, stream);
}
