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

extern "C" void hpnn_adam_host_init(hpnn_adam_state *s, double lr, double beta1, double beta2, double eps,
                                    double decay) {
    hpnn_adam_state_init(s, lr, beta1, beta2, eps, decay);
}

extern "C" void hpnn_adam_host_advance(hpnn_adam_state *s) { hpnn_adam_advance(s); }

extern "C" void hpnn_adam_host_update(int f64, void *W, void *M, void *V, const void *G, int S, long gstride, long n,
                                      double scale, const hpnn_adam_state *s) {
    if (f64) {
        const hpnn_adam_coef_f64 c = hpnn_adam_coef_f64_of(s);
        double *w = (double *)W, *m = (double *)M, *v = (double *)V;
        const double *g = (const double *)G;
        for (long i = 0; i < n; i++) {
            double a = 0.0;
            for (int k = 0; k < S; k++) a += g[(size_t)k * gstride + i];
            hpnn_adam_elem_f64(&c, a * scale, w + i, m + i, v + i);
        }
    } else {
        const hpnn_adam_coef_f32 c = hpnn_adam_coef_f32_of(s);
        float *w = (float *)W, *m = (float *)M, *v = (float *)V;
        const float *g = (const float *)G;
        const float sc = (float)scale;
        for (long i = 0; i < n; i++) {
            float a = 0.f;
            for (int k = 0; k < S; k++) a += g[(size_t)k * gstride + i];
            hpnn_adam_elem_f32(&c, a * sc, w + i, m + i, v + i);
        }
    }
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
