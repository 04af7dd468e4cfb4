/*
 * libhpnn -- the rule of the Adam trainer ([train] ADAM, batched mode).
 *
 * One definition for the CPU oracle, the device kernels (kernels_adam.hip) and the tests: plain
 * C++ here, __host__ __device__ under hipcc.  Every translation unit that includes this header
 * is compiled with FP contraction off, so the host and the device round the same operations.
 *
 * g is the project's descent direction (1/n) sum delta (x) h, the quantity BP adds to W, so the
 * rule is torch.optim.Adam / AdamW with maximize=True.
 *
 * State (FP64 on the host and in device memory):
 *   set once per call   lr, beta1, beta2, eps, decay
 *   running             t (starts 0), p1 = beta1^t, p2 = beta2^t (start 1, kept as running products)
 *   derived by advance  c1 = lr / (1 - p1), s2 = sqrt(1 - p2), wd = lr * decay
 *
 * advance runs once per step, before the update: t += 1, p1 *= beta1, p2 *= beta2, then the three
 * derived numbers -- multiplications, one division and one square root, all correctly rounded on
 * the host and on the device, so both hold the same bits.
 *
 * Per element, in the engine's master type T (float for bf16 / f32, double for f64); the
 * coefficients are cast to T once (hpnn_adam_coef), nothing is fused:
 *   m = (T)beta1 m + (T)(1 - beta1) g
 *   v = (T)beta2 v + ((T)(1 - beta2) g) g
 *   w = w - (T)wd w                               only when decay != 0 (decoupled: AdamW)
 *   w = w + (T)c1 (m / (sqrt(v) / (T)s2 + (T)eps))
 * An element whose gradient is always 0 keeps m = v = 0 and, at decay 0, its bits: the step is
 * c1 * (0 / eps) = 0.  A g whose square overflows T gives v = inf and a step of 0.
 */
#ifndef LIBHPNN_ADAM_H
#define LIBHPNN_ADAM_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HPNN_ADAM_FN __host__ __device__ static inline
#else
#include <math.h>
#define HPNN_ADAM_FN static inline
#endif

#define HPNN_ADAM_BETA1 0.9
#define HPNN_ADAM_BETA2 0.999
#define HPNN_ADAM_EPS 1e-8

typedef struct {
    double lr, beta1, beta2, eps, decay;
    unsigned long long t;
    double p1, p2;
    double c1, s2, wd;
} hpnn_adam_state;

/* 0 <= beta < 1, eps > 0, decay >= 0, lr finite (a NaN fails every test) */
HPNN_ADAM_FN int hpnn_adam_valid(double lr, double beta1, double beta2, double eps, double decay) {
    return lr == lr && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0 && decay >= 0.0;
}

HPNN_ADAM_FN void hpnn_adam_state_init(hpnn_adam_state *s, double lr, double beta1, double beta2, double eps,
                                       double decay) {
    s->lr = lr;
    s->beta1 = beta1;
    s->beta2 = beta2;
    s->eps = eps;
    s->decay = decay;
    s->t = 0ull;
    s->p1 = s->p2 = 1.0;
    s->c1 = s->s2 = s->wd = 0.0;
}

HPNN_ADAM_FN void hpnn_adam_advance(hpnn_adam_state *s) {
    s->t += 1ull;
    s->p1 *= s->beta1;
    s->p2 *= s->beta2;
    s->c1 = s->lr / (1.0 - s->p1);
    s->s2 = sqrt(1.0 - s->p2);
    s->wd = s->lr * s->decay;
}

/* the coefficients of one step in T, cast once */
#define HPNN_ADAM_COEF(NAME, T)                                                  \
    typedef struct {                                                             \
        T b1, omb1, b2, omb2, c1, s2, eps, wd;                                   \
        int decay;                                                               \
    } NAME;                                                                      \
    HPNN_ADAM_FN NAME NAME##_of(const hpnn_adam_state *s) {                      \
        NAME c;                                                                  \
        c.b1 = (T)s->beta1;                                                      \
        c.omb1 = (T)(1.0 - s->beta1);                                            \
        c.b2 = (T)s->beta2;                                                      \
        c.omb2 = (T)(1.0 - s->beta2);                                            \
        c.c1 = (T)s->c1;                                                         \
        c.s2 = (T)s->s2;                                                         \
        c.eps = (T)s->eps;                                                       \
        c.wd = (T)s->wd;                                                         \
        c.decay = s->decay != 0.0;                                               \
        return c;                                                                \
    }
HPNN_ADAM_COEF(hpnn_adam_coef_f64, double)
HPNN_ADAM_COEF(hpnn_adam_coef_f32, float)
#undef HPNN_ADAM_COEF

HPNN_ADAM_FN void hpnn_adam_elem_f64(const hpnn_adam_coef_f64 *c, double g, double *w, double *m, double *v) {
    const double mm = c->b1 * *m + c->omb1 * g;
    const double vv = c->b2 * *v + (c->omb2 * g) * g;
    double ww = *w;
    if (c->decay) ww = ww - c->wd * ww;
    *w = ww + c->c1 * (mm / (sqrt(vv) / c->s2 + c->eps));
    *m = mm;
    *v = vv;
}

HPNN_ADAM_FN void hpnn_adam_elem_f32(const hpnn_adam_coef_f32 *c, float g, float *w, float *m, float *v) {
    const float mm = c->b1 * *m + c->omb1 * g;
    const float vv = c->b2 * *v + (c->omb2 * g) * g;
    float ww = *w;
    if (c->decay) ww = ww - c->wd * ww;
    *w = ww + c->c1 * (mm / (sqrtf(vv) / c->s2 + c->eps));
    *m = mm;
    *v = vv;
}

#endif /* LIBHPNN_ADAM_H */
