/*
 * libhpnn learning-rate schedules on the host ([lr_schedule]): the entry points of
 * <libhpnn/lrsched.h> that the FP64 CPU oracle runs and that hpnn_amd.ops.lr_* / sgd_sched_* run
 * on CPU tensors -- the oracle of the device-side form (kernels_lrsched.hip).
 */
#include <libhpnn/ann.h>
#include <stddef.h>

#include "../gpu/engine.h"
#include "upd_host.h"

extern "C" int hpnn_lr_host_init(hpnn_lr_state *s, unsigned int kind, double lr0, double gamma, unsigned int period,
                                 unsigned int span, double lr_end, double lr_min, unsigned int patience,
                                 unsigned int warmup, unsigned int epoch) {
    hpnn_lr_state_init(s, kind, lr0, gamma, period, span, lr_end, lr_min, patience, warmup, epoch);
    return hpnn_lr_valid(s);
}

extern "C" int hpnn_lr_host_valid(const hpnn_lr_state *s) { return hpnn_lr_valid(s); }

extern "C" void hpnn_lr_host_advance(hpnn_lr_state *s) { hpnn_lr_advance(s); }

extern "C" void hpnn_lr_host_plateau(hpnn_lr_state *s, double loss_sum) { hpnn_lr_plateau(s, loss_sum); }

extern "C" void hpnn_sgd_sched_host_update_clip(int f64, void *W, void *V, const void *G, int S, long gstride, long n,
                                                double scale, double alpha, int momentum, const hpnn_lr_state *s,
                                                const hpnn_clip_state *clip) {
    const int mom = momentum && V;
    if (f64) {
        const double lr = s->lr, cf = clip ? clip->factor : 1.0;
        double *const v[1] = {(double *)V};
        auto elem = [=](double g, double *w, double *e) {
            hpnn_sgd_sched_elem_f64(lr, alpha, mom, clip ? g * cf : g, w, e);
        };
        hpnn_host_slab_update((double *)W, v, mom, (const double *)G, S, gstride, n, scale, elem);
    } else {
        const float lr = (float)s->lr, al = (float)alpha, cf = clip ? (float)clip->factor : 1.f;
        float *const v[1] = {(float *)V};
        auto elem = [=](float g, float *w, float *e) {
            hpnn_sgd_sched_elem_f32(lr, al, mom, clip ? g * cf : g, w, e);
        };
        hpnn_host_slab_update((float *)W, v, mom, (const float *)G, S, gstride, n, (float)scale, elem);
    }
}

extern "C" void hpnn_sgd_sched_host_update(int f64, void *W, void *V, const void *G, int S, long gstride, long n,
                                           double scale, double alpha, int momentum, const hpnn_lr_state *s) {
    hpnn_sgd_sched_host_update_clip(f64, W, V, G, S, gstride, n, scale, alpha, momentum, s, NULL);
}
