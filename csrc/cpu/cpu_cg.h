/*
 * libhpnn FP64 CPU batched engine -- the state of one [train] CG call (cpu_cg.cpp): the
 * direction, the previous gradient and the line search's a_init live for the call only.
 */
#ifndef HPNN_CPU_CG_H
#define HPNN_CPU_CG_H
#include <libhpnn/ann.h>
#include <libhpnn/cg.h>
#include <functional>
#include <vector>

struct HpnnCpuCg {
    UINT L = 0;
    std::vector<std::vector<DOUBLE>> g, gp, d, w0;
    std::vector<size_t> nw;
    std::vector<hpnn_cg_record> hist;
    hpnn_cg_state st;
    void init(kernel_ann *k, double lr, UINT n, UINT epochs);
    /* one iteration in place on k's weights; loss_of(&sum, &hits): the forward-only loss sum and
     * argmax hits of the current weights over the training set */
    void iterate(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT n, UINT B,
                 const std::function<void(DOUBLE *, UINT *)> &loss_of);
};
#endif
