/*
 * [lr_schedule] plateau: the five running fields of <libhpnn/lrsched.h> (scale, best, stale, cuts,
 * valid) as the kernel keeps them between batched calls and a state file keeps them between runs.
 * The one place that copies them, in either direction (host only: api.cpp, state.cpp).
 */
#ifndef HPNN_LR_RUNNING_H
#define HPNN_LR_RUNNING_H
#include <libhpnn/ann.h>
#include <libhpnn/lrsched.h>

/* the kernel's running fields into a schedule state */
static inline void hpnn_lr_running_get(const kernel_ann *k, hpnn_lr_state *s) {
    s->scale = k->lr_scale;
    s->best = k->lr_best;
    s->stale = k->lr_stale;
    s->cuts = k->lr_cuts;
    s->valid = k->lr_valid;
}

/* a schedule state's running fields into the kernel */
static inline void hpnn_lr_running_put(kernel_ann *k, const hpnn_lr_state *s) {
    k->lr_scale = s->scale;
    k->lr_best = s->best;
    k->lr_stale = s->stale;
    k->lr_cuts = s->cuts;
    k->lr_valid = s->valid;
}

#endif
