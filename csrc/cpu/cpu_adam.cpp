/*
 * libhpnn FP64 CPU batched engine: the Adam trainer ([train] ADAM), the oracle of the GPU
 * engines' device-side form (kernels_adam.hip), and the host entry points of <libhpnn/adam.h>
 * that hpnn_amd.ops.adam_* run on CPU tensors.
 *
 * One step = the gradient sum of hpnn_cpu_batched_grad over the minibatch, the advance of the
 * state and the elementwise rule with scale = 1 / B, all by the functions of adam.h.
 */
#include <libhpnn/ann.h>
#include <math.h>
#include <vector>

#include "../gpu/engine.h"
#include "upd_host.h"

extern "C" void hpnn_adam_host_init(hpnn_adam_state *s, double lr, double beta1, double beta2, double eps,
                                    double decay) {
    hpnn_adam_state_init(s, lr, beta1, beta2, eps, decay);
}

extern "C" void hpnn_adam_host_advance(hpnn_adam_state *s) { hpnn_adam_advance(s); }

extern "C" void hpnn_adam_host_update_clip(int f64, void *W, void *M, void *V, const void *G, int S, long gstride,
                                           long n, double scale, const hpnn_adam_state *s,
                                           const hpnn_clip_state *clip) {
    if (f64) {
        const hpnn_adam_coef_f64 c = hpnn_adam_coef_f64_of(s);
        const double cf = clip ? clip->factor : 1.0;
        double *const mv[2] = {(double *)M, (double *)V};
        hpnn_host_slab_update((double *)W, mv, true, (const double *)G, S, gstride, n, scale,
                              [&c, clip, cf](double g, double *w, double *e) {
                                  hpnn_adam_elem_f64(&c, clip ? g * cf : g, w, e, e + 1);
                              });
    } else {
        const hpnn_adam_coef_f32 c = hpnn_adam_coef_f32_of(s);
        const float cf = clip ? (float)clip->factor : 1.f;
        float *const mv[2] = {(float *)M, (float *)V};
        hpnn_host_slab_update((float *)W, mv, true, (const float *)G, S, gstride, n, (float)scale,
                              [&c, clip, cf](float g, float *w, float *e) {
                                  hpnn_adam_elem_f32(&c, clip ? g * cf : g, w, e, e + 1);
                              });
    }
}

extern "C" void hpnn_adam_host_update(int f64, void *W, void *M, void *V, const void *G, int S, long gstride, long n,
                                      double scale, const hpnn_adam_state *s) {
    hpnn_adam_host_update_clip(f64, W, M, V, G, S, gstride, n, scale, s, NULL);
}

extern "C" DOUBLE hpnn_cpu_adam_step(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT B,
                                     hpnn_adam_state *s, UINT *hits) {
    if (!k || !k->dw || !k->dv || B == 0) return NAN;
    const UINT L = k->n_hiddens + 1;
    std::vector<std::vector<DOUBLE>> G(L);
    std::vector<DOUBLE *> Gp(L);
    auto layer = [&](UINT l) { return l + 1 < L ? &k->hiddens[l] : &k->output; };
    for (UINT l = 0; l < L; l++) {
        G[l].resize((size_t)layer(l)->n_neurons * layer(l)->n_inputs);
        Gp[l] = G[l].data();
    }
    const DOUBLE sum = hpnn_cpu_batched_grad(k, type, X, T, B, Gp.data(), TRUE, hits);
    hpnn_adam_advance(s);
    for (UINT l = 0; l < L; l++)
        hpnn_adam_host_update(1, layer(l)->weights, k->dw[l], k->dv[l], Gp[l], 1, 0, (long)G[l].size(),
                              1.0 / (DOUBLE)B, s);
    k->adam_t = s->t;
    k->adam_p1 = s->p1;
    k->adam_p2 = s->p2;
    return sum / (DOUBLE)B;
}
