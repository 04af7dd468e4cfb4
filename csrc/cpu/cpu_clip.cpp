/*
 * libhpnn gradient clipping by global norm on the host ([clip]): the entry points of
 * <libhpnn/clip.h> that the FP64 CPU oracle runs and that hpnn_amd.ops.gnorm_partials /
 * clip_finalize / clip_commit run on CPU tensors -- the oracle of the device-side form
 * (kernels_clip.hip), bit for bit: the same element, the same order.
 *
 * One clipped step = the gradient sum of hpnn_cpu_batched_grad over the minibatch, the sum of
 * squares of g / B over every layer and the finalize in the order of clip.h, then the clipped host
 * update of BP / BPM (lrsched.h's element rule at the step's rate) or ADAM.
 */
#include <libhpnn/ann.h>
#include <math.h>
#include <stddef.h>
#include <vector>

#include "../gpu/engine.h"
#include "upd_host.h"

extern "C" int hpnn_clip_host_init(hpnn_clip_state *s, double max_norm) {
    hpnn_clip_state_init(s, max_norm);
    return hpnn_clip_valid(max_norm);
}

extern "C" long hpnn_clip_host_sumsq(int f64, int interleaved, const void *G, int S, long gstride, long n,
                                     double scale, double *partials) {
    if (f64) return hpnn_host_sumsq((const double *)G, S, gstride, n, scale, interleaved != 0, partials);
    return hpnn_host_sumsq((const float *)G, S, gstride, n, (float)scale, interleaved != 0, partials);
}

extern "C" void hpnn_clip_host_finalize(hpnn_clip_state *s, const double *partials, long count) {
    hpnn_clip_finalize(s, hpnn_host_sumsq_total(partials, count));
}

extern "C" void hpnn_clip_host_commit(hpnn_clip_state *s, hpnn_clip_record *hist, unsigned int *cursor,
                                      unsigned int cap) {
    hpnn_clip_commit(s, hist, cursor, cap);
}

extern "C" DOUBLE hpnn_cpu_clip_step(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT B, DOUBLE lr,
                                     BOOL momentum, DOUBLE alpha, hpnn_adam_state *adam, hpnn_clip_state *clip,
                                     UINT *hits) {
    if (!k || !clip || B == 0 || (momentum && !k->dw) || (adam && (!k->dw || !k->dv))) return NAN;
    const UINT L = k->n_hiddens + 1;
    std::vector<std::vector<DOUBLE>> G(L);
    std::vector<DOUBLE *> Gp(L);
    auto layer = [&](UINT l) { return l + 1 < L ? &k->hiddens[l] : &k->output; };
    size_t blocks = 0;
    for (UINT l = 0; l < L; l++) {
        G[l].resize((size_t)layer(l)->n_neurons * layer(l)->n_inputs);
        Gp[l] = G[l].data();
        blocks += (size_t)hpnn_clip_blocks(G[l].size());
    }
    const DOUBLE sum = hpnn_cpu_batched_grad(k, type, X, T, B, Gp.data(), TRUE, hits);
    const DOUBLE scale = 1.0 / (DOUBLE)B;
    std::vector<double> part(blocks);
    long at = 0;
    for (UINT l = 0; l < L; l++) at += hpnn_clip_host_sumsq(1, 0, Gp[l], 1, 0, (long)G[l].size(), scale, &part[at]);
    hpnn_clip_host_finalize(clip, part.data(), at);
    if (adam) {
        hpnn_adam_advance(adam);
        for (UINT l = 0; l < L; l++)
            hpnn_adam_host_update_clip(1, layer(l)->weights, k->dw[l], k->dv[l], Gp[l], 1, 0, (long)G[l].size(), scale,
                                       adam, clip);
        k->adam_t = adam->t;
        k->adam_p1 = adam->p1;
        k->adam_p2 = adam->p2;
    } else {
        hpnn_lr_state rate;
        hpnn_lr_state_init(&rate, HPNN_LR_CONSTANT, lr, HPNN_LR_GAMMA, HPNN_LR_PERIOD, 0u, 0.0, 0.0, HPNN_LR_PATIENCE,
                           0u, 0u);
        for (UINT l = 0; l < L; l++)
            hpnn_sgd_sched_host_update_clip(1, layer(l)->weights, momentum ? k->dw[l] : NULL, Gp[l], 1, 0,
                                            (long)G[l].size(), scale, alpha, momentum ? 1 : 0, &rate, clip);
    }
    return sum / (DOUBLE)B;
}
