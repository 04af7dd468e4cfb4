/*
 * libhpnn -- the rule of gradient clipping by global norm ([clip], batched mode).
 *
 * One definition for the CPU oracle, the device kernels (kernels_clip.hip) and the tests: plain
 * C++ here, __host__ __device__ under hipcc.  Every translation unit that includes this header
 * is compiled with FP contraction off, so the host and the device round the same operations.
 *
 * Element.  gs is the gradient element exactly as the update rule of the engine sees it: the slab
 * sum in that engine's own order (the FP walker: slabs 0 .. S-1 in order from 0; the BF16 plan:
 * p_w = the slabs w, w + 8, ... from 0, then ((((((p0 + p1) + p2) + p3) + p4) + p5) + p6) + p7)
 * times (T)scale.  It contributes q = (double)gs * (double)gs (exact for T = float).
 *
 * Order: a function of the element index only.  A segment (one layer's gradient, n elements,
 * linear index) is cut into consecutive blocks of HPNN_CLIP_BLOCK = 1024 elements.  In a block
 * lane t of 256 adds the q of the elements 4t, 4t + 1, 4t + 2, 4t + 3 in that order to a partial
 * that starts at 0 (elements past n add nothing); the 256 partials meet in a fixed binary tree,
 * p[t] += p[t + s] for s = 128, 64, ..., 1, and p[0] is the block's sum.  The block sums are stored
 * in block order, segment after segment, into double partials[].
 *
 * Finalize.  Lane t of 256 adds partials[t], partials[t + 256], ... in order to 0, the same tree
 * gives sumsq; norm = sqrt(sumsq) (FP64, correctly rounded on both sides);
 *   factor = norm > max_norm ? max_norm / norm : 1.0
 * No epsilon: a NaN norm gives factor 1 (the NaN propagates as without clipping), an infinite
 * norm factor 0.  Then the running counters of the epoch: steps += 1, clipped += (factor != 1),
 * norm_max = max(norm_max, norm) (a NaN never enters), norm_last = norm.
 *
 * Use.  With a clip state attached the element rule receives gs * (T)factor: one product in T,
 * the factor cast once per launch.  Factor 1 leaves gs's bits.
 *
 * State (FP64 and unsigned, 64 bytes):
 *   set once    max_norm
 *   per step    sumsq, norm, factor
 *   per epoch   norm_max, norm_last, steps, clipped
 */
#ifndef LIBHPNN_CLIP_H
#define LIBHPNN_CLIP_H

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HPNN_CLIP_FN __host__ __device__ static inline
#else
#define HPNN_CLIP_FN static inline
#endif

#define HPNN_CLIP_BLOCK 1024u /* elements of a block */
#define HPNN_CLIP_LANES 256u  /* lanes of a block and of the finalize */

typedef struct {
    double max_norm;            /* set once */
    double sumsq, norm, factor; /* per step */
    double norm_max, norm_last; /* per epoch */
    unsigned int steps, clipped;
    unsigned int pad[2];
} hpnn_clip_state;

/* what an epoch leaves behind (hpnn_clip_commit) */
typedef struct {
    unsigned int steps, clipped;
    double norm_max, norm_last;
} hpnn_clip_record;

/* a finite max_norm > 0 clips; 0 is "off" and valid too (a NaN fails every test) */
HPNN_CLIP_FN int hpnn_clip_valid(double max_norm) { return max_norm >= 0.0 && max_norm - max_norm == 0.0; }

HPNN_CLIP_FN void hpnn_clip_state_init(hpnn_clip_state *s, double max_norm) {
    s->max_norm = max_norm;
    s->sumsq = s->norm = 0.0;
    s->factor = 1.0;
    s->norm_max = s->norm_last = 0.0;
    s->steps = s->clipped = 0u;
    s->pad[0] = s->pad[1] = 0u;
}

/* the blocks of a segment of n elements */
HPNN_CLIP_FN unsigned long long hpnn_clip_blocks(unsigned long long n) {
    return (n + (HPNN_CLIP_BLOCK - 1u)) / HPNN_CLIP_BLOCK;
}

/* the tree over HPNN_CLIP_LANES partials, for one thread (the host); p[0] is the sum */
HPNN_CLIP_FN double hpnn_clip_tree(double *p) {
    for (unsigned int s = HPNN_CLIP_LANES / 2u; s >= 1u; s >>= 1)
        for (unsigned int t = 0; t < s; t++) p[t] = p[t] + p[t + s];
    return p[0];
}

/* the step's numbers from its sum of squares, then the epoch's counters */
HPNN_CLIP_FN void hpnn_clip_finalize(hpnn_clip_state *s, double sumsq) {
    const double norm = sqrt(sumsq);
    const double factor = norm > s->max_norm ? s->max_norm / norm : 1.0;
    s->sumsq = sumsq;
    s->norm = norm;
    s->factor = factor;
    s->steps += 1u;
    if (factor != 1.0) s->clipped += 1u;
    if (norm > s->norm_max) s->norm_max = norm;
    s->norm_last = norm;
}

/* the end of an epoch: its record (a full history drops it) and the counters back to zero */
HPNN_CLIP_FN void hpnn_clip_commit(hpnn_clip_state *s, hpnn_clip_record *hist, unsigned int *cursor,
                                   unsigned int cap) {
    if (hist && cursor) {
        const unsigned int c = *cursor;
        if (c < cap) {
            hist[c].steps = s->steps;
            hist[c].clipped = s->clipped;
            hist[c].norm_max = s->norm_max;
            hist[c].norm_last = s->norm_last;
            *cursor = c + 1u;
        }
    }
    s->steps = s->clipped = 0u;
    s->norm_max = s->norm_last = 0.0;
}

#endif /* LIBHPNN_CLIP_H */
