/*
 * libhpnn FP64 CPU batched engine: the conjugate-gradient trainer ([train] CG), the oracle of
 * the GPU engines' device-side form (kernels_cg.hip), and the host entry points of
 * <libhpnn/cg.h> that hpnn_amd.ops.cg_* run on CPU tensors.
 *
 * One epoch = one CG iteration over the whole set (docs/DESIGN.md 3.2h): the gradient
 * accumulated batch by batch in batch order, f0, the three dot products, the direction, six
 * forward-only trials, the seventh trial and the step -- every decision taken by the functions
 * of cg.h, every weight written by hpnn_cg_step_f64.
 */
#include <libhpnn/ann.h>
#include <math.h>
#include <string.h>
#include <vector>

#include "../core/runtime_internal.h"
#include "../gpu/engine.h"
#include "cpu_cg.h"

static inline DOUBLE act(DOUBLE x) { return 2.0 / (1.0 + exp(-1.0 * x)) - 1.0; }
static inline DOUBLE dact(DOUBLE y) { return -0.5 * (y * y - 1.0); }

/* the forward, loss and deltas of hpnn_cpu_batched_step (same order of operations per sample);
 * the gradient is the SUM over the batch and nothing is updated */
extern "C" DOUBLE hpnn_cpu_batched_grad(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT B,
                                        DOUBLE **G, BOOL first, UINT *hits) {
    const UINT L = k->n_hiddens + 1;
    std::vector<const layer_ann *> layers(L);
    for (UINT l = 0; l + 1 < L; l++) layers[l] = &k->hiddens[l];
    layers[L - 1] = &k->output;
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
        UINT g = 0, tr = 0;
        for (UINT i = 1; i < n_out; i++) {
            if (o[i] > o[g]) g = i;
            if (t[i] > t[tr]) tr = i;
        }
        hit[b] = g == tr;
        for (UINT i = 0; i < n_out; i++) d[i] = (type == NN_TYPE_ANN) ? (t[i] - o[i]) * dact(o[i]) : (t[i] - o[i]);
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
    for (UINT l = 0; l < L; l++) {
        const UINT N = layers[l]->n_neurons, M = layers[l]->n_inputs;
        const DOUBLE *H = l ? A[l - 1].data() : X;
        const DOUBLE *Dl = D[l].data();
        DOUBLE *Gl = G[l];
#pragma omp parallel for num_threads(nt) schedule(static)
        for (long j = 0; j < (long)N; j++)
            for (UINT i = 0; i < M; i++) {
                DOUBLE g = 0.0;
                for (UINT b = 0; b < B; b++) g += Dl[(size_t)b * N + j] * H[(size_t)b * M + i];
                Gl[_2D_IDX(M, j, i)] = first ? g : Gl[_2D_IDX(M, j, i)] + g;
            }
    }
    DOUBLE s = 0.0;
    UINT c = 0;
    for (UINT b = 0; b < B; b++) {
        s += loss[b];
        c += hit[b];
    }
    if (hits) *hits += c;
    return s;
}

/* ---- host entry points of <libhpnn/cg.h> ---- */
namespace {
inline double step(double a, double x, double y) { return hpnn_cg_step_f64(a, x, y); }
inline float step(float a, float x, float y) { return hpnn_cg_step_f32(a, x, y); }

template <typename T>
void accumulate(T *g, const T *slab, int S, long sstride, long n, int first, T scale) {
    for (long i = 0; i < n; i++) {
        T acc = first ? (T)0 : g[i];
        for (int s = 0; s < S; s++) acc += slab[(size_t)s * sstride + i];
        g[i] = acc * scale;
    }
}
template <typename T>
void dots(const T *g, const T *p, const T *d, long n, double *out) {
    for (long i = 0; i < n; i++) {
        const double x = (double)g[i];
        out[0] += x * x;
        out[1] += x * (double)p[i];
        out[2] += x * (double)d[i];
    }
}
template <typename T>
void begin(const T *w, T *w0, const T *g, T *gp, T *d, long n, T beta) {
    for (long i = 0; i < n; i++) {
        d[i] = step(beta, d[i], g[i]);
        gp[i] = g[i];
        w0[i] = w[i];
    }
}
template <typename T>
void trial(T *w, const T *w0, const T *d, long n, T a) {
    for (long i = 0; i < n; i++) w[i] = step(a, d[i], w0[i]);
}
}  // namespace

extern "C" void hpnn_cg_host_init(hpnn_cg_state *s, double a_init, unsigned int n, unsigned int cap) {
    hpnn_cg_state_init(s, a_init, n, cap);
}
extern "C" void hpnn_cg_host_accumulate(int f64, void *g, const void *slab, int S, long sstride, long n, int first,
                                        double scale) {
    if (f64) accumulate((double *)g, (const double *)slab, S, sstride, n, first, scale);
    else accumulate((float *)g, (const float *)slab, S, sstride, n, first, (float)scale);
}
extern "C" void hpnn_cg_host_dots(int f64, const void *g, const void *gprev, const void *d, long n, double *out) {
    if (f64) dots((const double *)g, (const double *)gprev, (const double *)d, n, out);
    else dots((const float *)g, (const float *)gprev, (const float *)d, n, out);
}
extern "C" void hpnn_cg_host_direction(hpnn_cg_state *s) { hpnn_cg_rule_direction(s); }
extern "C" void hpnn_cg_host_begin(int f64, const void *w, void *w0, const void *g, void *gprev, void *d, long n,
                                   double beta) {
    if (f64) begin((const double *)w, (double *)w0, (const double *)g, (double *)gprev, (double *)d, n, beta);
    else begin((const float *)w, (float *)w0, (const float *)g, (float *)gprev, (float *)d, n, (float)beta);
}
extern "C" void hpnn_cg_host_trial(int f64, void *w, const void *w0, const void *d, long n, double a) {
    if (f64) trial((double *)w, (const double *)w0, (const double *)d, n, a);
    else trial((float *)w, (const float *)w0, (const float *)d, n, (float)a);
}
extern "C" void hpnn_cg_host_file(hpnn_cg_state *s, hpnn_cg_record *hist, unsigned int j, double loss_sum,
                                  unsigned int hits) {
    hpnn_cg_rule_file(s, hist, j, loss_sum, hits);
}

/* ---- the oracle's iteration ---- */
void HpnnCpuCg::init(kernel_ann *k, double lr, UINT n, UINT epochs) {
    L = k->n_hiddens + 1;
    g.resize(L), gp.resize(L), d.resize(L), w0.resize(L), nw.resize(L);
    for (UINT l = 0; l < L; l++) {
        const layer_ann *ly = l + 1 < L ? &k->hiddens[l] : &k->output;
        nw[l] = (size_t)ly->n_neurons * ly->n_inputs;
        g[l].assign(nw[l], 0.0), gp[l].assign(nw[l], 0.0), d[l].assign(nw[l], 0.0), w0[l].assign(nw[l], 0.0);
    }
    hist.assign(epochs, hpnn_cg_record());
    hpnn_cg_state_init(&st, lr, n, epochs);
}

void HpnnCpuCg::iterate(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT n, UINT B,
                        const std::function<void(DOUBLE *, UINT *)> &loss_of) {
    auto W = [&](UINT l) { return (l + 1 < L ? &k->hiddens[l] : &k->output)->weights; };
    std::vector<DOUBLE *> G(L);
    std::vector<std::vector<DOUBLE>> Gb(L);
    for (UINT l = 0; l < L; l++) {
        Gb[l].assign(nw[l], 0.0);
        G[l] = Gb[l].data();
    }
    /* step 1: g = (1/n) sum over the batches, in batch order; f0 */
    for (UINT s = 0; s < n; s += B) {
        const UINT b = (n - s < B) ? n - s : B;
        hpnn_cpu_batched_grad(k, type, X + (size_t)s * k->n_inputs, T + (size_t)s * k->n_outputs, b, G.data(), TRUE,
                              NULL);
        for (UINT l = 0; l < L; l++)
            hpnn_cg_host_accumulate(1, g[l].data(), G[l], 1, 0, (long)nw[l], s == 0, s + b >= n ? 1.0 / (double)n : 1.0);
    }
    DOUBLE sum = 0.0;
    UINT hits = 0;
    loss_of(&sum, &hits);
    hpnn_cg_rule_file(&st, hist.data(), HPNN_CG_FINAL, sum, hits);
    /* steps 2, 3 */
    double dot[3] = {0.0, 0.0, 0.0};
    for (UINT l = 0; l < L; l++) hpnn_cg_host_dots(1, g[l].data(), gp[l].data(), d[l].data(), (long)nw[l], dot);
    st.gg = dot[0], st.gp = dot[1], st.gd = dot[2];
    hpnn_cg_rule_direction(&st);
    for (UINT l = 0; l < L; l++)
        hpnn_cg_host_begin(1, W(l), w0[l].data(), g[l].data(), gp[l].data(), d[l].data(), (long)nw[l], st.beta);
    /* steps 4, 5: six trials, the seventh, the step */
    for (unsigned int j = 0; j <= HPNN_CG_FINAL; j++) {
        for (UINT l = 0; l < L; l++) hpnn_cg_host_trial(1, W(l), w0[l].data(), d[l].data(), (long)nw[l], st.a[j]);
        if (j == HPNN_CG_FINAL) break;
        loss_of(&sum, &hits);
        hpnn_cg_rule_file(&st, hist.data(), j, sum, hits);
    }
}
