/*
 * The host form of the update kernels' element loop (csrc/gpu/upd_common.h), shared by
 * hpnn_adam_host_update and hpnn_sgd_sched_host_update: per element the S slabs summed in slab
 * order from 0, g = sum * scale, then the rule on w and the NS state values beside it.  `on`
 * false: the state arrays are neither read nor written and the rule sees 0.
 */
#ifndef HPNN_CPU_UPD_HOST_H
#define HPNN_CPU_UPD_HOST_H
#include <stddef.h>

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

#endif /* HPNN_CPU_UPD_HOST_H */
