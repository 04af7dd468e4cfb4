/*
 * The host form of the update kernels' element loop (csrc/gpu/upd_common.h), shared by
 * hpnn_adam_host_update and hpnn_sgd_sched_host_update: per element the S slabs summed in slab
 * order from 0, g = sum * scale, then the rule on w and the NS state values beside it.  `on`
 * false: the state arrays are neither read nor written and the rule sees 0.
 */
#ifndef HPNN_CPU_UPD_HOST_H
#define HPNN_CPU_UPD_HOST_H
#include <stddef.h>

#include <libhpnn/clip.h>

template <typename T, int NS, class Elem>
inline void hpnn_host_slab_update(T *w, T *const (&s)[NS], bool on, const T *g, int S, long gstride, long n, T scale,
                                  Elem elem) {
    for (long i = 0; i < n; i++) {
        T a = (T)0, e[NS];
        for (int k = 0; k < S; k++) a += g[(size_t)k * gstride + i];
        for (int j = 0; j < NS; j++) e[j] = on ? s[j][i] : (T)0;
        elem(a * scale, w + i, e);
        if (on)
            for (int j = 0; j < NS; j++) s[j][i] = e[j];
    }
}

/*
 * The host form of the global-norm reduction (csrc/gpu/kernels_clip.hip, rule and order in
 * <libhpnn/clip.h>): the element as the update rule sees it -- the slab sum in slab order from 0
 * (interleaved: the 8-way order of the BF16 plan's sub-tile update) times scale -- squared in FP64,
 * four elements per lane, 256 lanes per block of 1024 elements, the fixed tree per block.  One
 * double per block into partials[]; returns the number of blocks.
 */
template <typename T>
inline T hpnn_host_slab_sum(const T *g, int S, long gstride, long i, bool interleaved) {
    if (!interleaved) {
        T a = (T)0;
        for (int k = 0; k < S; k++) a += g[(size_t)k * gstride + i];
        return a;
    }
    T p[8];
    for (int w = 0; w < 8; w++) {
        p[w] = (T)0;
        for (int k = w; k < S; k += 8) p[w] += g[(size_t)k * gstride + i];
    }
    T a = p[0];
    for (int w = 1; w < 8; w++) a += p[w];
    return a;
}

template <typename T>
inline long hpnn_host_sumsq(const T *g, int S, long gstride, long n, T scale, bool interleaved, double *partials) {
    const long B = (long)HPNN_CLIP_BLOCK, nb = (long)hpnn_clip_blocks((unsigned long long)n);
    for (long b = 0; b < nb; b++) {
        double p[HPNN_CLIP_LANES];
        for (long t = 0; t < (long)HPNN_CLIP_LANES; t++) {
            double a = 0.0;
            for (long k = 0; k < 4; k++) {
                const long i = b * B + 4 * t + k;
                if (i >= n) break;
                const T gs = hpnn_host_slab_sum(g, S, gstride, i, interleaved) * scale;
                a += (double)gs * (double)gs;
            }
            p[t] = a;
        }
        partials[b] = hpnn_clip_tree(p);
    }
    return nb;
}

/* partials[0 .. count) in the finalize's order: lane t adds t, t + 256, ..., then the tree */
inline double hpnn_host_sumsq_total(const double *partials, long count) {
    double p[HPNN_CLIP_LANES];
    for (long t = 0; t < (long)HPNN_CLIP_LANES; t++) {
        double a = 0.0;
        for (long i = t; i < count; i += (long)HPNN_CLIP_LANES) a += partials[i];
        p[t] = a;
    }
    return hpnn_clip_tree(p);
}

#endif /* HPNN_CPU_UPD_HOST_H */
