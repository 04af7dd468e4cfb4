/*
 * libhpnn learning-rate schedules on the host ([lr_schedule]): the entry points of
 * <libhpnn/lrsched.h> that the FP64 CPU oracle runs and that hpnn_amd.ops.lr_* / sgd_sched_* run
 * on CPU tensors -- the oracle of the device-side form (kernels_lrsched.hip).
 */
#include <libhpnn/ann.h>
#include <stddef.h>

#include "../gpu/engine.h"

extern "C" int hpnn_lr_host_init(hpnn_lr_state *s, unsigned int kind, double lr0, double gamma, unsigned int period,
                                 unsigned int span, double lr_end, double lr_min, unsigned int patience,
                                 unsigned int warmup, unsigned int epoch) {
    hpnn_lr_state_init(s, kind, lr0, gamma, period, span, lr_end, lr_min, patience, warmup, epoch);
    return hpnn_lr_valid(s);
}

extern "C" int hpnn_lr_host_valid(const hpnn_lr_state *s) { return hpnn_lr_valid(s); }

extern "C" void hpnn_lr_host_advance(hpnn_lr_state *s) { hpnn_lr_advance(s); }

extern "C" void hpnn_lr_host_plateau(hpnn_lr_state *s, double loss_sum) { hpnn_lr_plateau(s, loss_sum); }

extern "C" void hpnn_sgd_sched_host_update(int f64, void *W, void *V, const void *G, int S, long gstride, long n,
                                           double scale, double alpha, int momentum, const hpnn_lr_state *s) {
    const int mom = momentum && V;
    if (f64) {
        double *w = (double *)W, *v = (double *)V;
        const double *g = (const double *)G;
        const double lr = s->lr;
        for (long i = 0; i < n; i++) {
            double a = 0.0, p = mom ? v[i] : 0.0;
            for (int k = 0; k < S; k++) a += g[(size_t)k * gstride + i];
            hpnn_sgd_sched_elem_f64(lr, alpha, mom, a * scale, w + i, &p);
            if (mom) v[i] = p;
        }
    } else {
        float *w = (float *)W, *v = (float *)V;
        const float *g = (const float *)G;
        const float lr = (float)s->lr, al = (float)alpha, sc = (float)scale;
        for (long i = 0; i < n; i++) {
            float a = 0.f, p = mom ? v[i] : 0.f;
            for (int k = 0; k < S; k++) a += g[(size_t)k * gstride + i];
            hpnn_sgd_sched_elem_f32(lr, al, mom, a * sc, w + i, &p);
            if (mom) v[i] = p;
        }
    }
}
