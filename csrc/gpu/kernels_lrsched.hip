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
 *   hpnn_sgd_sched_fp      the segment walker of upd_common.h: the BP / BPM step of the FP64 /
 *                          FP32 engines with the rate READ FROM THE STATE
 *   hpnn_sgd_sched_multi   the sub-tile update of upd_common.h, the BF16 plan's BP / BPM step: the
 *                          rule on the FP32 W32 / V32
 *
 * Like kernels_best.hip and kernels_adam.hip every number that changes (the rate) lives in a
 * device hpnn_lr_state and is read from memory when the launch runs, never baked in at capture: a
 * replayed graph of several epochs takes a new rate every epoch.  The thread that changes the
 * state is a launch of its own and its consumers later launches on the same stream.
 *
 * The zero padding of W32 stays zero: g = 0 and v = 0 there.
 *
 * This unit is compiled with FP contraction off: nothing is fused, as on the host.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <libhpnn/adam.h>
#include <libhpnn/clip.h>
#include <libhpnn/lrsched.h>

#include "kernels.h"
#include "upd_common.h"

HPNN_CO_PROBE(lrsched)

namespace {

static_assert(HPNN_SCHED_MAX_SEGS == hpnn_upd::SEG_MAX, "one table size");

template <typename T>
struct SchedRule {
    typedef T type;
    typedef hpnn_sched_seg seg;
    typedef hpnn_upd_layer layer;
    typedef hpnn_lr_state state;
    struct args {
        T scale, alpha;
        int momentum;
        const hpnn_clip_state *clip; /* [clip]: NULL = off */
    };
    struct coef {
        T lr, alpha;
        int mom;
        T clipf; /* (T)clip->factor, in use when clip */
        int clip;
    };
    static constexpr int NS = 1; /* the momentum: in use under BPM only (a segment's may be NULL under BP) */
    /* a segment's array: the walker alone asks (the table builder has its own pointer check) */
    static __device__ bool arrays(const seg &g, const args &a, T **s) {
        s[0] = (T *)g.v;
        return a.momentum && s[0];
    }
    /* a layer's array: the sub-tile kernel and, on the host, the layer check of upd_tile */
    static __host__ __device__ bool arrays(const layer &L, const args &a, float **s) {
        s[0] = L.V32;
        return a.momentum;
    }
    static __host__ __device__ const hpnn_upd_layer &base(const layer &L) { return L; }
    /* the rate of this epoch */
    static __device__ coef read(const args &a, bool on, const state *st) {
        return {(T)st->lr, a.alpha, on, a.clip ? (T)a.clip->factor : (T)1, a.clip != nullptr};
    }
    static __device__ void elem(const coef &c, T g, T *w, T *e) {
        if (c.clip) g = g * c.clipf;
        if constexpr (sizeof(T) == 8)
            hpnn_sgd_sched_elem_f64(c.lr, c.alpha, c.mom, g, w, e);
        else
            hpnn_sgd_sched_elem_f32(c.lr, c.alpha, c.mom, g, w, e);
    }
};

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
    return hpnn_upd::launched();
}

extern "C" int hpnn_lr_plateau_dev(const hpnn_val_record *vhist, const unsigned int *vcursor, hpnn_lr_state *state,
                                   hipStream_t stream) {
    if (!vhist || ((uintptr_t)vhist & 7u) || !vcursor || ((uintptr_t)vcursor & 3u) || !state ||
        ((uintptr_t)state & 7u))
        return -1;
    hipLaunchKernelGGL(lr_plateau_kernel, dim3(1), dim3(64), 0, stream, vhist, vcursor, state);
    return hpnn_upd::launched();
}

extern "C" int hpnn_sgd_sched_table(int f64, hpnn_sched_seg *segs, const hpnn_sched_seg *host_segs, int n_segs,
                                    int momentum, hipStream_t stream) {
    auto ptrs = [momentum](const hpnn_sched_seg &g, uintptr_t &all) {
        all = (uintptr_t)g.w | (uintptr_t)g.v | (uintptr_t)g.g;
        return g.w && (g.v || !momentum) && g.g; /* BP: no momentum array */
    };
    return hpnn_upd::seg_table(f64, segs, host_segs, n_segs, stream, ptrs);
}

extern "C" int hpnn_sgd_sched_fp_clip(int f64, const hpnn_sched_seg *segs, int n_segs, double scale, double alpha,
                                      int momentum, const hpnn_lr_state *state, const hpnn_clip_state *clip,
                                      hipStream_t stream) {
    if ((uintptr_t)clip & 7u) return -1;
    if (f64)
        return hpnn_upd::seg_walk<SchedRule<double>>(segs, n_segs, {scale, alpha, momentum, clip}, state, stream);
    return hpnn_upd::seg_walk<SchedRule<float>>(segs, n_segs, {(float)scale, (float)alpha, momentum, clip}, state,
                                                stream);
}

extern "C" int hpnn_sgd_sched_fp(int f64, const hpnn_sched_seg *segs, int n_segs, double scale, double alpha,
                                 int momentum, const hpnn_lr_state *state, hipStream_t stream) {
    return hpnn_sgd_sched_fp_clip(f64, segs, n_segs, scale, alpha, momentum, state, nullptr, stream);
}

extern "C" int hpnn_sgd_sched_multi_clip(const hpnn_upd_layer *layers, int n, float alpha, float scale, int momentum,
                                         const hpnn_lr_state *state, const hpnn_clip_state *clip,
                                         hipStream_t stream) {
    if (!layers || n < 1 || n > 2 * HPNN_UPD_MAX || !state || (((uintptr_t)state | (uintptr_t)clip) & 7u)) return -1;
    return hpnn_upd::upd_tile<SchedRule<float>>(layers, n, {scale, alpha, momentum ? 1 : 0, clip}, state, stream);
}

extern "C" int hpnn_sgd_sched_multi(const hpnn_upd_layer *layers, int n, float alpha, float scale, int momentum,
                                    const hpnn_lr_state *state, hipStream_t stream) {
    return hpnn_sgd_sched_multi_clip(layers, n, alpha, scale, momentum, state, nullptr, stream);
}
