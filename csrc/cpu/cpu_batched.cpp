/*
 * libhpnn FP64 CPU batched engine: the oracle for minibatch semantics.
 *
 * Batched mode (new; the reference only trains online):
 *   for a minibatch of B samples, deltas are computed per sample exactly as
 *   in the online engine, the weight "gradient" is the mean
 *   G_l = (1/B) sum_b d_l^b (x) h_{l-1}^b, and the update reuses the
 *   reference rules with G in place of d (x) h:
 *     BP : W += lr G
 *     BPM: dW += lr G; W += dW; dW *= alpha    (momentum persists across
 *          minibatches; it is zeroed once at the start of training)
 *   With B = 1 one BP step equals one reference BP iteration.
 * Reductions run in a fixed order (sample index ascending) so results do
 * not depend on the OpenMP thread count.
 */
#include <libhpnn/ann.h>
#include <libhpnn/observe.h>
#include <libhpnn/shuffle.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>

#include "../core/export_records.h"
#include "../core/runtime_internal.h"
#include "../gpu/engine.h"
#include "cpu_cg.h"

static inline DOUBLE act(DOUBLE x) { return 2.0 / (1.0 + exp(-1.0 * x)) - 1.0; }
static inline DOUBLE dact(DOUBLE y) { return -0.5 * (y * y - 1.0); }

extern "C" DOUBLE hpnn_cpu_batched_step(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T,
                                        UINT B, DOUBLE lr, BOOL momentum, DOUBLE alpha, UINT *hits) {
    const UINT L = k->n_hiddens + 1;
    std::vector<const layer_ann *> layers(L);
    for (UINT l = 0; l + 1 < L; l++) layers[l] = &k->hiddens[l];
    layers[L - 1] = &k->output;
    /* activations A[l]: B x N_l ; A[-1] = X */
    std::vector<std::vector<DOUBLE>> A(L), D(L);
    for (UINT l = 0; l < L; l++) {
        A[l].assign((size_t)B * layers[l]->n_neurons, 0.0);
        D[l].assign((size_t)B * layers[l]->n_neurons, 0.0);
    }
    const UINT n_out = k->n_outputs;
    std::vector<DOUBLE> loss(B, 0.0);
    std::vector<unsigned char> hit(B, 0);
    const int nt = _NN(return, omp_threads)();
#pragma omp parallel for num_threads(nt) schedule(static)
    for (long b = 0; b < (long)B; b++) {
        const DOUBLE *x = X + (size_t)b * k->n_inputs;
        for (UINT l = 0; l < L; l++) {
            const layer_ann *ly = layers[l];
            DOUBLE *y = A[l].data() + (size_t)b * ly->n_neurons;
            const bool last = (l == L - 1);
            for (UINT j = 0; j < ly->n_neurons; j++) {
                const DOUBLE *w = ly->weights + _2D_IDX(ly->n_inputs, j, 0);
                DOUBLE s = 0.0;
                for (UINT i = 0; i < ly->n_inputs; i++) s += w[i] * x[i];
                y[j] = (!last || type == NN_TYPE_ANN) ? act(s) : s;
            }
            if (last && type == NN_TYPE_SNN) {
                DOUBLE dv = HPNN_TINY;
                for (UINT j = 0; j < ly->n_neurons; j++) {
                    y[j] = exp(y[j] - 1.0);
                    dv += y[j];
                }
                for (UINT j = 0; j < ly->n_neurons; j++) y[j] /= dv;
            }
            x = y;
        }
        /* loss + output delta */
        const DOUBLE *o = A[L - 1].data() + (size_t)b * n_out;
        const DOUBLE *t = T + (size_t)b * n_out;
        DOUBLE *d = D[L - 1].data() + (size_t)b * n_out;
        DOUBLE Ep = 0.0;
        if (type == NN_TYPE_SNN) {
            for (UINT i = 0; i < n_out; i++)
                if (o[i] > 0.) Ep += t[i] * log(o[i] + HPNN_TINY);
            Ep *= -1.0 / (DOUBLE)n_out;
        } else {
            for (UINT i = 0; i < n_out; i++) Ep += (t[i] - o[i]) * (t[i] - o[i]);
            Ep *= 0.5;
        }
        loss[b] = Ep;
        UINT g = 0, tr = 0; /* argmax hit (first maximum, as the GPU kernels) */
        for (UINT i = 1; i < n_out; i++) {
            if (o[i] > o[g]) g = i;
            if (t[i] > t[tr]) tr = i;
        }
        hit[b] = g == tr;
        for (UINT i = 0; i < n_out; i++) d[i] = (type == NN_TYPE_ANN) ? (t[i] - o[i]) * dact(o[i]) : (t[i] - o[i]);
        /* hidden deltas */
        for (long l = (long)L - 2; l >= 0; l--) {
            const layer_ann *up = layers[l + 1];
            const UINT N = up->n_neurons, M = up->n_inputs;
            const DOUBLE *dn = D[l + 1].data() + (size_t)b * N;
            const DOUBLE *h = A[l].data() + (size_t)b * M;
            DOUBLE *dl = D[l].data() + (size_t)b * M;
            for (UINT m = 0; m < M; m++) {
                DOUBLE s = 0.0;
                for (UINT n = 0; n < N; n++) s += up->weights[_2D_IDX(M, n, m)] * dn[n];
                dl[m] = s * dact(h[m]);
            }
        }
    }
    /* gradient + update per layer */
    const DOUBLE inv_b = 1.0 / (DOUBLE)B;
    const bool mom = momentum && k->dw;
    for (UINT l = 0; l < L; l++) {
        layer_ann *ly = (layer_ann *)layers[l];
        const UINT N = ly->n_neurons, M = ly->n_inputs;
        const DOUBLE *H = l ? A[l - 1].data() : X;
        const DOUBLE *Dl = D[l].data();
        DOUBLE *dw = mom ? k->dw[l] : NULL;
#pragma omp parallel for num_threads(nt) schedule(static)
        for (long j = 0; j < (long)N; j++) {
            DOUBLE *w = ly->weights + _2D_IDX(M, j, 0);
            for (UINT i = 0; i < M; i++) {
                DOUBLE g = 0.0;
                for (UINT b = 0; b < B; b++) g += Dl[(size_t)b * N + j] * H[(size_t)b * M + i];
                g *= inv_b;
                if (dw) {
                    DOUBLE *v = dw + _2D_IDX(M, j, 0);
                    v[i] += lr * g;
                    w[i] += v[i];
                    v[i] *= alpha;
                } else {
                    w[i] += lr * g;
                }
            }
        }
    }
    DOUBLE s = 0.0;
    UINT c = 0;
    for (UINT b = 0; b < B; b++) {
        s += loss[b];
        c += hit[b];
    }
    if (hits) *hits += c;
    return s * inv_b;
}

extern "C" UINT hpnn_validation_schedule(UINT epoch0, UINT epochs, UINT validate, UINT *out) {
    UINT c = 0;
    if (!validate) return 0;
    for (UINT e = 0; e < epochs; e++) {
        const UINT a = epoch0 + e + 1;
        if (a % validate && e + 1 != epochs) continue;
        if (out) out[c] = a;
        c++;
    }
    return c;
}

/* [validate]: forward only over the held-out set with the current weights (FP64; the oracle of
 * the GPU engines' validation pass): mean loss per sample and argmax hits (first maximum) */
/* M (may be NULL; [confusion]): the pass's matrix [n_out][n_out + 1], zero on entry */
static void cpu_validate(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT n,
                         hpnn_validation_record *r, DOUBLE *loss_sum, unsigned int *M = NULL) {
    DOUBLE sum = 0.0;
    UINT hits = 0;
    for (UINT s = 0; s < n; s++) {
        memcpy(k->in, X + (size_t)s * k->n_inputs, sizeof(DOUBLE) * k->n_inputs);
        hpnn_cpu_forward(k, type);
        const DOUBLE *t = T + (size_t)s * k->n_outputs;
        sum += hpnn_cpu_error(k, type, t);
        UINT g = 0, tr = 0;
        for (UINT i = 1; i < k->n_outputs; i++) {
            if (k->output.vec[i] > k->output.vec[g]) g = i;
            if (t[i] > t[tr]) tr = i;
        }
        hits += (g == tr);
        if (M) hpnn_confusion_count(M, (int)tr, (int)g, (int)k->n_outputs);
    }
    r->loss = sum / (DOUBLE)n;
    r->correct = hits;
    r->n = n;
    if (loss_sum) *loss_sum = sum;
}

extern "C" BOOL hpnn_cpu_train_batched(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n,
                                       const hpnn_batched_opts *o, hpnn_batched_stats *st) {
    if (!k || n == 0) return FALSE;
    const bool mom = o->train == NN_TRAIN_BPM;
    if (mom) {
        const bool keep = o->resume && k->dw;
        ann_momentum_init(k);
        if (!keep) ann_raz_momentum(k);
    }
    /* [train] ADAM: the moments in k->dw (first) and k->dv (second), the running state in the
     * kernel; zero unless the call resumes a loaded state */
    const bool adam = o->train == NN_TRAIN_ADAM;
    const bool cg = o->train == NN_TRAIN_CG;
    hpnn_adam_state ast;
    hpnn_adam_state_init(&ast, o->lr, o->beta1, o->beta2, o->eps, o->decay);
    if (adam) {
        if (!hpnn_adam_valid(o->lr, o->beta1, o->beta2, o->eps, o->decay)) {
            NN_ERROR(stderr, "[train] ADAM: needs 0 <= beta1, beta2 < 1, epsilon > 0, decay >= 0\n");
            return FALSE;
        }
        const bool keep = o->resume && k->dw && k->dv;
        if (!keep) ann_adam_free(k);
        ann_adam_init(k);
        if (!keep) ann_raz_momentum(k);
        ast.t = k->adam_t;
        ast.p1 = k->adam_p1;
        ast.p2 = k->adam_p2;
    }
    /* [lr_schedule]: the state of <libhpnn/lrsched.h>, advanced before the first step of every epoch
     * and shown every validation loss (the oracle of kernels_lrsched.hip); the step size of an
     * epoch is the state's lr */
    const bool sched = o->sched != 0;
    hpnn_lr_state lrs = o->lrs;
    std::vector<DOUBLE> lrh;
    if (sched && (cg || !hpnn_lr_valid(&lrs))) {
        NN_ERROR(stderr, "[lr_schedule]: %s\n", cg ? "not supported by [train] CG (it chooses its own step)"
                                                   : "the schedule's keys are out of range");
        return FALSE;
    }
    /* [clip]: the state of <libhpnn/clip.h>; every step is the gradient, its global norm in the
     * fixed order, the factor and the clipped host update (the oracle of kernels_clip.hip) */
    const bool clip = o->clip > 0.0;
    hpnn_clip_state cls;
    hpnn_clip_state_init(&cls, o->clip);
    std::vector<hpnn_clip_record> clh;
    if (!hpnn_clip_valid(o->clip) || (clip && cg)) {
        NN_ERROR(stderr, "[clip]: %s\n", cg ? "not supported by [train] CG (it chooses its own step); it applies to "
                                              "BP, BPM and ADAM"
                                            : "needs a finite value >= 0 (0 = off)");
        return FALSE;
    }
    const UINT B = o->batch ? o->batch : 1;
    /* [shuffle] epoch: epoch e trains on a permuted copy, position i = sample src(i) of
     * <libhpnn/shuffle.h> for (n, seed, epochs completed); one batch per epoch: nothing to do */
    /* [train] CG: one epoch = one conjugate-gradient iteration over the whole set (cpu_cg.cpp);
     * the sample order only changes a summation order, so nothing is reshuffled */
    const bool shuffle = o->shuffle && B < n && !cg;
    if (o->shuffle && cg) NN_OUT(stdout, "batched CPU training: CG sums over the whole set, no reshuffle\n");
    else if (o->shuffle && !shuffle) NN_OUT(stdout, "batched CPU training: one batch per epoch, no reshuffle\n");
    HpnnCpuCg cgs;
    if (cg) cgs.init(k, o->lr, n, o->epochs);
    std::vector<DOUBLE> Xs, Ts;
    std::vector<unsigned int> perm;
    if (shuffle) {
        NN_OUT(stdout, "batched CPU training: samples reshuffled every epoch\n");
        Xs.resize((size_t)n * k->n_inputs);
        Ts.resize((size_t)n * k->n_outputs);
        perm.resize(n);
    }
    const DOUBLE *Xe = shuffle ? Xs.data() : X, *Te = shuffle ? Ts.data() : T;
    const bool validate = o->validate && o->Xv && o->Tv && o->nv;
    std::vector<hpnn_validation_record> val;
    /* [keep_best] / [patience] (the oracle of the GPU engines' device-side form, kernels_best.hip):
     * the rule and the counters on the pass's loss sum and hits; the snapshot is a host copy of
     * the weights and the momentum; training stops at the stopping pass */
    const bool keep = validate && o->keep_best != 0;
    const UINT L = k->n_hiddens + 1;
    auto layer = [&](UINT l) { return l + 1 < L ? &k->hiddens[l] : &k->output; };
    std::vector<std::vector<DOUBLE>> bestW, bestV, bestA;
    hpnn_adam_state best_ast = ast;
    hpnn_lr_state best_lrs = lrs;
    /* [confusion]: the oracle of kernels_confusion.hip -- the matrix of every pass through the rule
     * header, its per-class record, the last and the best pass's matrix */
    const bool confusion = validate && o->confusion != 0;
    const size_t cells = (size_t)hpnn_confusion_cells(k->n_outputs);
    std::vector<unsigned int> cm, cm_best, pch;
    if (confusion) NN_OUT(stdout, "batched CPU training: per-class metrics of every validation pass\n");
    bool have_best = false, stop = false;
    DOUBLE best_sum = 0.0;
    UINT best_hits = 0, best_index = 0, stale = 0, epochs_run = 0;
    auto t0 = std::chrono::steady_clock::now();
    UINT64 samples = 0;
    DOUBLE last = 0.0;
    for (UINT e = 0; e < o->epochs && !stop; e++) {
        DOUBLE acc = 0.0;
        UINT nb = 0, hits = 0;
        if (shuffle) {
            hpnn_shuffle_perm(n, o->seed, o->epoch0 + e, perm.data());
            for (UINT i = 0; i < n; i++) {
                memcpy(&Xs[(size_t)i * k->n_inputs], X + (size_t)perm[i] * k->n_inputs, sizeof(DOUBLE) * k->n_inputs);
                memcpy(&Ts[(size_t)i * k->n_outputs], T + (size_t)perm[i] * k->n_outputs, sizeof(DOUBLE) * k->n_outputs);
            }
        }
        if (sched) {
            hpnn_lr_advance(&lrs);
            lrh.push_back(lrs.lr);
            if (adam) ast.lr = lrs.lr; /* the Adam advance of the next step derives c1 and wd from it */
        }
        const DOUBLE lr_e = sched ? lrs.lr : o->lr;
        if (cg) {
            cgs.iterate(k, o->type, X, T, n, B, [&](DOUBLE *sum, UINT *h) {
                hpnn_validation_record r;
                cpu_validate(k, o->type, X, T, n, &r, sum);
                *h = r.correct;
            });
            last = acc = cgs.hist[e].f0;
            hits = cgs.st.hits0;
            nb = 1;
            samples += n;
        }
        for (UINT s = 0; s < n && !cg; s += B) {
            UINT b = (n - s < B) ? n - s : B;
            const DOUBLE *xb = Xe + (size_t)s * k->n_inputs, *tb = Te + (size_t)s * k->n_outputs;
            if (clip)
                last = hpnn_cpu_clip_step(k, o->type, xb, tb, b, lr_e, mom, o->alpha, adam ? &ast : NULL, &cls, &hits);
            else
                last = adam ? hpnn_cpu_adam_step(k, o->type, xb, tb, b, &ast, &hits)
                            : hpnn_cpu_batched_step(k, o->type, xb, tb, b, lr_e, mom, o->alpha, &hits);
            acc += last;
            nb++;
            samples += b;
        }
        if (clip) { /* the end of the epoch: its record, the counters back to zero */
            clh.resize(clh.size() + 1);
            unsigned int cur = 0;
            hpnn_clip_commit(&cls, &clh.back(), &cur, 1u);
        }
        if (st) st->epoch_loss = acc / (nb ? nb : 1);
        if (hpnn_metrics_active())
            hpnn_metrics_epoch("cpu", o->epoch0 + e + 1, acc / (nb ? nb : 1), hits, n,
                               std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), samples);
        if (validate && ((o->epoch0 + e + 1) % o->validate == 0 || e + 1 == o->epochs)) {
            hpnn_validation_record r;
            r.epoch = o->epoch0 + e + 1;
            DOUBLE sum = 0.0;
            if (confusion) cm.assign(cells, 0u);
            cpu_validate(k, o->type, o->Xv, o->Tv, o->nv, &r, &sum, confusion ? cm.data() : NULL);
            hpnn_metrics_validation("cpu", r.epoch, r.loss, r.correct, r.n);
            val.push_back(r);
            if (confusion) {
                pch.resize(pch.size() + 3 * (size_t)k->n_outputs);
                unsigned int *rec = pch.data() + pch.size() - 3 * (size_t)k->n_outputs;
                hpnn_confusion_classes(cm.data(), (int)k->n_outputs, rec);
                hpnn_metrics_classes("cpu", r.epoch, rec, k->n_outputs);
            }
            if (sched) hpnn_lr_plateau(&lrs, sum); /* before the snapshot: the best state holds this pass */
            if (keep && hpnn_best_improves((int)o->keep_best, have_best, sum, r.correct, best_sum, best_hits)) {
                have_best = true;
                best_sum = sum;
                best_hits = r.correct;
                best_index = (UINT)val.size() - 1;
                stale = 0;
                cm_best = cm;
                bestW.resize(L);
                bestV.resize(mom || adam ? L : 0);
                bestA.resize(adam ? L : 0);
                best_ast = ast;
                best_lrs = lrs;
                for (UINT l = 0; l < L; l++) {
                    const size_t nw = (size_t)layer(l)->n_neurons * layer(l)->n_inputs;
                    bestW[l].assign(layer(l)->weights, layer(l)->weights + nw);
                    if (mom || adam) bestV[l].assign(k->dw[l], k->dw[l] + nw);
                    if (adam) bestA[l].assign(k->dv[l], k->dv[l] + nw);
                }
            } else if (keep) {
                stale++;
            }
            if (keep && o->patience && stale == o->patience) stop = true;
        }
        epochs_run = e + 1;
    }
    auto t1 = std::chrono::steady_clock::now();
    if (st) {
        st->last_loss = last;
        st->samples = samples;
        st->seconds = std::chrono::duration<double>(t1 - t0).count();
        /* accuracy of the final weights on the training set */
        UINT correct = 0;
        for (UINT s = 0; s < n; s++) {
            memcpy(k->in, X + (size_t)s * k->n_inputs, sizeof(DOUBLE) * k->n_inputs);
            hpnn_cpu_forward(k, o->type);
            const DOUBLE *t = T + (size_t)s * k->n_outputs;
            UINT g = 0, tr = 0;
            for (UINT i = 1; i < k->n_outputs; i++)
                if (k->output.vec[i] > k->output.vec[g]) g = i;
            for (UINT i = 1; i < k->n_outputs; i++)
                if (t[i] > t[tr]) tr = i;
            correct += (g == tr);
        }
        st->correct = correct;
        st->epochs_run = epochs_run;
        st->best_epoch = have_best ? val[best_index].epoch : 0;
        st->best_index = best_index;
        st->stop_epoch = stop ? val.back().epoch : 0;
        st->lrs = have_best ? best_lrs : lrs;
        std::vector<hpnn_cg_record> cgh;
        if (cg) cgh.assign(cgs.hist.begin(), cgs.hist.begin() + epochs_run);
        if (!export_records(val, &st->val, &st->n_val) || !export_records(lrh, &st->lr_hist, &st->n_lr) ||
            !export_records(clh, &st->clip_hist, &st->n_clip) || !export_records(cgh, &st->cg, &st->n_cg))
            return FALSE;
        if (confusion) {
            UINT words = 0, n_cells = 0;
            st->n_classes = k->n_outputs;
            if (!export_records(pch, &st->class_hist, &words) ||
                !export_records(cm, &st->confusion_last, &n_cells) ||
                !export_records(have_best ? cm_best : std::vector<unsigned int>(), &st->confusion_best, &n_cells))
                return FALSE;
            st->n_class_hist = (UINT)val.size(); /* records of 3 n_outputs words */
        }
    }
    /* [keep_best]: the kernel as it was after the best pass's epoch */
    for (UINT l = 0; have_best && l < L; l++) {
        memcpy(layer(l)->weights, bestW[l].data(), bestW[l].size() * sizeof(DOUBLE));
        if (mom || adam) memcpy(k->dw[l], bestV[l].data(), bestV[l].size() * sizeof(DOUBLE));
        if (adam) memcpy(k->dv[l], bestA[l].data(), bestA[l].size() * sizeof(DOUBLE));
    }
    if (adam && have_best) {
        k->adam_t = best_ast.t;
        k->adam_p1 = best_ast.p1;
        k->adam_p2 = best_ast.p2;
    }
    /* the momentum stays in k->dw: nn_dump_state saves it for an exact resume */
    return TRUE;
}

extern "C" void hpnn_epoch_perm(UINT n, UINT seed, UINT epoch, UINT *out) {
    if (out) hpnn_shuffle_perm(n, seed, epoch, out);
}
