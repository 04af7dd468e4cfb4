/*
 * libhpnn -- the decisions of the conjugate-gradient trainer ([train] CG, batched mode).
 *
 * One definition for the CPU oracle, the device kernels (kernels_cg.hip) and the tests: plain
 * C++ here, __host__ __device__ under hipcc.  Every translation unit that includes this header
 * is compiled with FP contraction off, so the host and the device take the same decision from
 * the same numbers.
 *
 * One epoch = one nonlinear CG iteration over the whole training set.  g is the project's
 * descent direction (1/n) sum delta (x) h, the quantity BP adds to W.
 *
 *   direction   beta = max(0, (gg - gp) / gg_prev)                     (Polak-Ribiere+)
 *               beta = 0 on the first iteration of a call, after a failed search, when
 *               gg_prev is not > 0, and when gg + beta gd > 0 does not hold (d = g + beta d
 *               would not descend); then a_j = a_init 2^(j-2), j < K = 6
 *   choose      phi_j = loss(W0 + a_j d), f0 = loss(W0).  j* = the lowest index of the
 *               smallest phi_j that is not a NaN.  The search FAILS unless phi_j* < f0 (a NaN
 *               anywhere that matters lands here).  Else b = a_j*, and for j* < K-1 the vertex
 *               of the parabola through (a, b, c) -- a = a_{j*-1}, or (0, f0) for j* = 0;
 *               c = a_{j*+1} -- is the seventh trial point when its denominator is not 0 and
 *               it is finite and strictly inside (a, c); otherwise the seventh trial is b
 *               itself (a failed search: 0)
 *   settle      a* = the seventh point if its loss is smaller than phi_j*, else b; a_init = a*.
 *               Failed: a* = 0 (W = W0 bit for bit), a_init /= 16, the next direction is g.
 *               One record {f0, f1, beta, alpha, trial, flags} is appended to the history.
 *
 * All losses are means: a sum over the set divided by n.
 */
#ifndef LIBHPNN_CG_H
#define LIBHPNN_CG_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HPNN_CG_FN __host__ __device__ static inline
#else
#include <math.h>
#define HPNN_CG_FN static inline
#endif

#define HPNN_CG_TRIALS 6                    /* K: the trials of the fixed-work search */
#define HPNN_CG_PARABOLA HPNN_CG_TRIALS     /* index of the seventh trial */
#define HPNN_CG_FINAL (HPNN_CG_TRIALS + 1)  /* index of the final step a*; phi[FINAL] = f0 */
#define HPNN_CG_NONE 0xffffffffu            /* jstar when every trial loss is a NaN */

#define HPNN_CG_FAILED 1u   /* the search failed: W = W0, a_init /= 16 */
#define HPNN_CG_RESTART 2u  /* beta was forced to 0 (first iteration, after a failure, no descent) */
#define HPNN_CG_VERTEX 4u   /* the seventh trial was a valid parabola vertex */
#define HPNN_CG_TOOK7 8u    /* the seventh trial replaced b */

typedef struct {
    double f0, f1;      /* mean loss before and after the iteration */
    double beta, alpha; /* the direction's beta and the step a* taken along it */
    unsigned int trial; /* j* (HPNN_CG_NONE: none) */
    unsigned int flags;
} hpnn_cg_record;

typedef struct {
    double gg, gp, gd; /* <g,g>, <g,g_prev>, <g,d> of this iteration */
    double gg_prev;
    double beta;
    double a_init;
    double a[HPNN_CG_TRIALS + 2];   /* the trial steps, the seventh point, a* */
    double phi[HPNN_CG_TRIALS + 2]; /* their mean losses; phi[HPNN_CG_FINAL] = f0 */
    unsigned int hits0;             /* argmax hits of W0 */
    unsigned int first;             /* 1: the next direction is steepest descent */
    unsigned int jstar;
    unsigned int flags;
    unsigned int cursor, cap; /* records filed / capacity of the history */
    unsigned int n;           /* samples of the training set */
    unsigned int pad;
} hpnn_cg_state;

HPNN_CG_FN void hpnn_cg_state_init(hpnn_cg_state *s, double a_init, unsigned int n, unsigned int cap) {
    s->gg = s->gp = s->gd = s->gg_prev = s->beta = 0.0;
    s->a_init = a_init;
    for (int j = 0; j < HPNN_CG_TRIALS + 2; j++) s->a[j] = s->phi[j] = 0.0;
    s->hits0 = 0u;
    s->first = 1u;
    s->jstar = HPNN_CG_NONE;
    s->flags = 0u;
    s->cursor = 0u;
    s->cap = cap;
    s->n = n;
    s->pad = 0u;
}

/* after the dot products: beta, the restart flag and the trial steps */
HPNN_CG_FN void hpnn_cg_rule_direction(hpnn_cg_state *s) {
    double beta = 0.0;
    unsigned int flags = 0u;
    if (s->first || !(s->gg_prev > 0.0)) {
        flags = HPNN_CG_RESTART;
    } else {
        beta = (s->gg - s->gp) / s->gg_prev;
        if (!(beta > 0.0)) beta = 0.0; /* max(0, .); a NaN is 0 too */
        const double slope = s->gg + beta * s->gd;
        if (!(slope > 0.0)) {
            beta = 0.0;
            flags = HPNN_CG_RESTART;
        }
    }
    s->beta = beta;
    s->flags = flags;
    s->gg_prev = s->gg;
    s->jstar = HPNN_CG_NONE;
    s->a[0] = s->a_init * 0.25;
    s->a[1] = s->a_init * 0.5;
    s->a[2] = s->a_init;
    s->a[3] = s->a_init * 2.0;
    s->a[4] = s->a_init * 4.0;
    s->a[5] = s->a_init * 8.0;
    s->a[HPNN_CG_PARABOLA] = 0.0;
    s->a[HPNN_CG_FINAL] = 0.0;
}

/* after trial K-1: j*, the failure test and the seventh trial point */
HPNN_CG_FN void hpnn_cg_rule_choose(hpnn_cg_state *s) {
    const double f0 = s->phi[HPNN_CG_FINAL];
    unsigned int js = HPNN_CG_NONE;
    for (unsigned int j = 0; j < HPNN_CG_TRIALS; j++) {
        const double p = s->phi[j];
        if (p != p) continue;
        if (js == HPNN_CG_NONE || p < s->phi[js]) js = j;
    }
    s->jstar = js;
    if (js == HPNN_CG_NONE || !(s->phi[js] < f0)) {
        s->flags |= HPNN_CG_FAILED;
        s->a[HPNN_CG_PARABOLA] = 0.0;
        return;
    }
    const double b = s->a[js], fb = s->phi[js];
    s->a[HPNN_CG_PARABOLA] = b;
    if (js + 1 >= HPNN_CG_TRIALS) return;
    const double a = js ? s->a[js - 1] : 0.0, fa = js ? s->phi[js - 1] : f0;
    const double c = s->a[js + 1], fc = s->phi[js + 1];
    const double ba = b - a, bc = b - c;
    const double p = ba * (fb - fc), q = bc * (fb - fa);
    const double den = p - q;
    if (den == 0.0 || den != den) return;
    const double x = b - 0.5 * (ba * p - bc * q) / den;
    if (!(x > a && x < c)) return; /* outside the bracket, infinite or a NaN */
    s->a[HPNN_CG_PARABOLA] = x;
    s->flags |= HPNN_CG_VERTEX;
}

/* after the seventh trial: a*, the next a_init, the record */
HPNN_CG_FN void hpnn_cg_rule_settle(hpnn_cg_state *s, hpnn_cg_record *hist) {
    const double f0 = s->phi[HPNN_CG_FINAL];
    double astar = 0.0, f1 = f0;
    if (s->flags & HPNN_CG_FAILED) {
        s->a_init = s->a_init / 16.0;
        s->first = 1u;
    } else {
        astar = s->a[s->jstar];
        f1 = s->phi[s->jstar];
        if (s->phi[HPNN_CG_PARABOLA] < f1) {
            astar = s->a[HPNN_CG_PARABOLA];
            f1 = s->phi[HPNN_CG_PARABOLA];
            s->flags |= HPNN_CG_TOOK7;
        }
        s->a_init = astar;
        s->first = 0u;
    }
    s->a[HPNN_CG_FINAL] = astar;
    if (hist && s->cursor < s->cap) {
        hpnn_cg_record *r = hist + s->cursor;
        r->f0 = f0;
        r->f1 = f1;
        r->beta = s->beta;
        r->alpha = astar;
        r->trial = s->jstar;
        r->flags = s->flags;
        s->cursor += 1u;
    }
}

/* file a loss sum and its hits as phi[j] (j = HPNN_CG_FINAL: f0 and hits0) and run the decision
 * that follows trial j */
HPNN_CG_FN void hpnn_cg_rule_file(hpnn_cg_state *s, hpnn_cg_record *hist, unsigned int j, double loss_sum,
                             unsigned int hits) {
    if (j > HPNN_CG_FINAL) return;
    s->phi[j] = loss_sum / (double)s->n;
    if (j == HPNN_CG_FINAL) s->hits0 = hits;
    if (j == HPNN_CG_TRIALS - 1) hpnn_cg_rule_choose(s);
    if (j == HPNN_CG_PARABOLA) hpnn_cg_rule_settle(s, hist);
}

/* the elementwise rule of the direction (d = step(beta, d, g)) and of a trial (W = step(a, d,
 * W0)): ONE fma in the engine's type; a factor of 0 returns the addend itself, bit for bit, also
 * for -0 and for an x that is not finite */
HPNN_CG_FN double hpnn_cg_step_f64(double a, double x, double y) { return a == 0.0 ? y : fma(a, x, y); }
HPNN_CG_FN float hpnn_cg_step_f32(float a, float x, float y) { return a == 0.f ? y : fmaf(a, x, y); }

#endif /* LIBHPNN_CG_H */
