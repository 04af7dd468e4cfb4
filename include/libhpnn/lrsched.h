/*
 * libhpnn -- the rule of the learning-rate schedules ([lr_schedule], batched mode).
 *
 * One definition for the CPU oracle, the device kernels (kernels_lrsched.hip) and the tests: plain
 * C++ here, __host__ __device__ under hipcc.  Every translation unit that includes this header
 * is compiled with FP contraction off, so the host and the device round the same operations.
 *
 * Only + - * / on doubles and integer-to-double conversions: every one of them is correctly
 * rounded on the host and on the device, so a device state equals the host's bit for bit.  pow,
 * exp and cos are not, which is why there is no cosine or exponential form.
 *
 * State (FP64 and unsigned, 96 bytes):
 *   set once per call   kind, lr0 (= [lr]), gamma, period, span, lr_end, lr_min, patience, warmup
 *   running             epoch (absolute 0-based index of the NEXT epoch, starts at epochs_done),
 *                       scale (starts 1), best, stale, cuts, valid
 *   derived by advance  lr
 *
 * advance runs once per epoch, before its first step.  With e = epoch the base rate is
 *   constant   lr0
 *   step       lr0 * gamma^(e / period): a factor that starts at 1.0 times gamma, e / period times
 *   linear     e < span ? lr0 + (lr_end - lr0) * ((double)e / (double)span) : lr_end
 *   plateau    max(lr_min, lr0 * scale)
 * then, for e < warmup, base * ((double)(e + 1) / (double)warmup); lr = that, epoch += 1.
 *
 * plateau runs behind a validation pass (a no-op for the other kinds): a loss sum that is not a
 * NaN and < best (the first such loss is always taken) sets best, valid = 1, stale = 0; anything
 * else, ties and NaNs included, stale += 1.  When stale == patience: scale *= gamma, stale = 0,
 * cuts += 1.  The new scale takes effect at the next advance.
 *
 * The scheduled step per element, in the engine's master type T (float for bf16 / f32, double for
 * f64); lr is cast to T once, nothing is fused, g = (T)scale * (the slab sum):
 *   BP    w = w + lr * g
 *   BPM   v = v + lr * g;  w = w + v;  v = v * alpha
 * A g of 0 with v = 0 keeps w's bits (the zero padding of the BF16 plan stays zero).
 */
#ifndef LIBHPNN_LRSCHED_H
#define LIBHPNN_LRSCHED_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HPNN_LR_FN __host__ __device__ static inline
#else
#define HPNN_LR_FN static inline
#endif

#define HPNN_LR_CONSTANT 0u
#define HPNN_LR_STEP 1u
#define HPNN_LR_LINEAR 2u
#define HPNN_LR_PLATEAU 3u
#define HPNN_LR_KINDS 4u

#define HPNN_LR_GAMMA 0.5
#define HPNN_LR_PERIOD 10u
#define HPNN_LR_PATIENCE 2u

typedef struct {
    double lr0, gamma, lr_end, lr_min; /* set once */
    double scale, best;                /* running */
    double lr;                         /* derived */
    unsigned int kind, period, span, patience, warmup; /* set once */
    unsigned int epoch, stale, cuts, valid;            /* running */
    unsigned int pad;
} hpnn_lr_state;

HPNN_LR_FN int hpnn_lr_finite(double x) { return x - x == 0.0; }

/* lr0 and lr_end finite, 0 < gamma <= 1, period >= 1, span >= 1 for linear, lr_min >= 0,
 * patience >= 1 for plateau (a NaN fails every test) */
HPNN_LR_FN int hpnn_lr_valid(const hpnn_lr_state *s) {
    if (s->kind >= HPNN_LR_KINDS) return 0;
    if (!hpnn_lr_finite(s->lr0) || !hpnn_lr_finite(s->lr_end)) return 0;
    if (!(s->gamma > 0.0 && s->gamma <= 1.0)) return 0;
    if (s->period < 1u) return 0;
    if (s->kind == HPNN_LR_LINEAR && s->span < 1u) return 0;
    if (!(s->lr_min >= 0.0)) return 0;
    if (s->kind == HPNN_LR_PLATEAU && s->patience < 1u) return 0;
    return 1;
}

/* a fresh state: the next epoch is `epoch` (the epochs done so far), scale 1, nothing judged */
HPNN_LR_FN void hpnn_lr_state_init(hpnn_lr_state *s, unsigned int kind, double lr0, double gamma, unsigned int period,
                                   unsigned int span, double lr_end, double lr_min, unsigned int patience,
                                   unsigned int warmup, unsigned int epoch) {
    s->lr0 = lr0;
    s->gamma = gamma;
    s->lr_end = lr_end;
    s->lr_min = lr_min;
    s->scale = 1.0;
    s->best = 0.0;
    s->lr = lr0;
    s->kind = kind;
    s->period = period;
    s->span = span;
    s->patience = patience;
    s->warmup = warmup;
    s->epoch = epoch;
    s->stale = s->cuts = s->valid = 0u;
    s->pad = 0u;
}

HPNN_LR_FN void hpnn_lr_advance(hpnn_lr_state *s) {
    const unsigned int e = s->epoch;
    double base = s->lr0;
    if (s->kind == HPNN_LR_STEP) {
        double f = 1.0;
        for (unsigned int i = 0, k = e / s->period; i < k; i++) f = f * s->gamma;
        base = s->lr0 * f;
    } else if (s->kind == HPNN_LR_LINEAR) {
        base = e < s->span ? s->lr0 + (s->lr_end - s->lr0) * ((double)e / (double)s->span) : s->lr_end;
    } else if (s->kind == HPNN_LR_PLATEAU) {
        base = s->lr0 * s->scale;
        if (base < s->lr_min) base = s->lr_min;
    }
    if (e < s->warmup) base = base * ((double)(e + 1u) / (double)s->warmup);
    s->lr = base;
    s->epoch = e + 1u;
}

HPNN_LR_FN void hpnn_lr_plateau(hpnn_lr_state *s, double loss_sum) {
    if (s->kind != HPNN_LR_PLATEAU) return;
    if (loss_sum == loss_sum && (!s->valid || loss_sum < s->best)) {
        s->best = loss_sum;
        s->valid = 1u;
        s->stale = 0u;
    } else {
        s->stale += 1u;
    }
    if (s->stale == s->patience) {
        s->scale = s->scale * s->gamma;
        s->stale = 0u;
        s->cuts += 1u;
    }
}

/* the scheduled BP / BPM step of one element; lr and alpha already cast to T */
#define HPNN_LR_ELEM(NAME, T)                                                       \
    HPNN_LR_FN void NAME(T lr, T alpha, int momentum, T g, T *w, T *v) {            \
        const T d = lr * g;                                                         \
        if (momentum) {                                                             \
            const T vv = *v + d;                                                    \
            *w = *w + vv;                                                           \
            *v = vv * alpha;                                                        \
        } else {                                                                    \
            *w = *w + d;                                                            \
        }                                                                           \
    }
HPNN_LR_ELEM(hpnn_sgd_sched_elem_f64, double)
HPNN_LR_ELEM(hpnn_sgd_sched_elem_f32, float)
#undef HPNN_LR_ELEM

#endif /* LIBHPNN_LRSCHED_H */
