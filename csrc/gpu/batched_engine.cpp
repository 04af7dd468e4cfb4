/*
 * libhpnn batched GPU engine -- entry: routes a training call to the tensor-parallel engine
 * (tp_engine.cpp) or to one of the three drivers by the options, the environment and the world.
 */
#include <libhpnn/bootstrap.h>

#include "batched_common.h"

using namespace hpnn::eng;

/* rank `rank`'s rows of global minibatch b (B samples of n, Bg = ceil(B / world) per rank):
 * [*start, *start + *nv) and *total, the samples of the whole minibatch (pure: unit-tested on
 * the CPU through ctypes, tests/test_capi_cpu.py).  One device: rank 0, Bg = B. */
extern "C" void hpnn_dp_shard(int b, int B, int n, int rank, int Bg, int *start, int *nv, int *total) {
    const int end = (b * B + B < n) ? b * B + B : n;
    *start = b * B + rank * Bg;
    const int v = end - *start;
    *nv = v < 0 ? 0 : (v > Bg ? Bg : v);
    *total = end - b * B;
}

extern "C" BOOL hpnn_gpu_train_batched(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n,
                                       const hpnn_batched_opts *o, hpnn_batched_stats *st) {
    if (o->dtype != NN_DTYPE_BF16 && o->dtype != NN_DTYPE_F32 && o->dtype != NN_DTYPE_F64) {
        NN_ERROR(stderr, "GPU batched engine: unsupported dtype %d\n", (int)o->dtype);
        return FALSE;
    }
    const char *lb = getenv("HPNN_LOOPBACK_RANKS");
    const int lbr = lb ? atoi(lb) : 0;
    const char *fr = getenv("HPNN_FORCE_RCCL");
    const char *nd = getenv("HPNN_NATIVE_DP");
    if (o->train == NN_TRAIN_CG) {
        /* [train] CG exists on one device only: its decisions live in one device's memory
         * (train_single refuses [dtype] bf16) */
        if (o->tp) {
            NN_ERROR(stderr, "[train] CG is not supported by tensor-parallel batched training; use one GPU "
                             "([parallel] dp, 1 GPU) or [train] BP / BPM\n");
            return FALSE;
        }
        if (lbr >= 2 || hpnn_boot_world() > 1 || o->n_gpu > 1 || (fr && fr[0] == '1') || getenv("HPNN_DP_FORCE")) {
            NN_ERROR(stderr, "[train] CG is not supported by data-parallel batched training; use one GPU or "
                             "[train] BP / BPM\n");
            return FALSE;
        }
        return train_single(k, X, T, n, o, st);
    }
    if (o->clip > 0.0) {
        /* [clip] exists on one device only: the norm is reduced over one device's gradient */
        if (o->tp) {
            NN_ERROR(stderr, "[clip] is not supported by tensor-parallel batched training; it applies to [train] BP, "
                             "BPM and ADAM on one GPU ([parallel] dp, 1 GPU) and to the CPU engine\n");
            return FALSE;
        }
        if (lbr >= 2 || hpnn_boot_world() > 1 || o->n_gpu > 1 || (fr && fr[0] == '1') || getenv("HPNN_DP_FORCE")) {
            NN_ERROR(stderr, "[clip] is not supported by data-parallel batched training; it applies to [train] BP, "
                             "BPM and ADAM on one GPU and to the CPU engine\n");
            return FALSE;
        }
    }
    if (o->train == NN_TRAIN_ADAM) {
        /* [train] ADAM exists on one device only: its moments and its step count live beside one
         * device's masters */
        if (o->tp) {
            NN_ERROR(stderr, "[train] ADAM is not supported by tensor-parallel batched training; use one GPU "
                             "([parallel] dp, 1 GPU) or [train] BP / BPM\n");
            return FALSE;
        }
        if (lbr >= 2 || hpnn_boot_world() > 1 || o->n_gpu > 1 || (fr && fr[0] == '1') || getenv("HPNN_DP_FORCE")) {
            NN_ERROR(stderr, "[train] ADAM is not supported by data-parallel batched training; use one GPU or "
                             "[train] BP / BPM\n");
            return FALSE;
        }
        return train_single(k, X, T, n, o, st);
    }
    if (o->sched) {
        /* [lr_schedule] exists on one device only: the rate lives in one device's memory */
        if (o->tp) {
            NN_ERROR(stderr, "[lr_schedule] is not supported by tensor-parallel batched training; use one GPU "
                             "([parallel] dp, 1 GPU)\n");
            return FALSE;
        }
        if (lbr >= 2 || hpnn_boot_world() > 1 || o->n_gpu > 1 || (fr && fr[0] == '1') || getenv("HPNN_DP_FORCE")) {
            NN_ERROR(stderr, "[lr_schedule] is not supported by data-parallel batched training; use one GPU\n");
            return FALSE;
        }
        return train_single(k, X, T, n, o, st);
    }
    if (o->tp) return hpnn_gpu_train_tp(k, X, T, n, o, st);
    if (lbr >= 2) return train_dp(k, X, T, n, o, st, lbr, true);
    /* one process per GPU under a launcher (torchrun --no-python bin/train_nn ...);
     * HPNN_DP_FORCE=1: the same path with ONE rank under a launcher (its step structure and
     * exchange kernels timed on a single GPU, as bench.py's HPNN_DP_FORCE) */
    const char *dpf = getenv("HPNN_DP_FORCE");
    const bool dp_one = dpf && dpf[0] == '1' && getenv("LOCAL_WORLD_SIZE") && hpnn_boot_world() == 1;
    if ((hpnn_boot_world() > 1 || dp_one) && !(nd && nd[0] == '0')) return train_dp_mp(k, X, T, n, o, st);
    if (o->n_gpu > 1 || (fr && fr[0] == '1')) return train_dp(k, X, T, n, o, st, (int)(o->n_gpu ? o->n_gpu : 1), false);
    return train_single(k, X, T, n, o, st);
}
