/*
 * Validation inside the captured epoch graph ([validate] N, gfx950).
 *
 *   hpnn_argmax_rows       the guess of the per-layer evaluation path: per row of the logits
 *                          the lowest index of the largest value (one thread per row)
 *   hpnn_validate_commit   one evaluation pass's statistics -> the next record of a device
 *                          history, the slots zeroed for the next pass, a device cursor advanced
 *
 * The evaluation kernels (hpnn_mlp3_eval, or the per-layer forward and the output kernel) add
 * loss and hits into 64 stat slots of their own.  This launch follows them on the same stream:
 * one 64-lane workgroup, lane i loads slot i, lane 0 adds the 64 values in slot order (FP64 for
 * the loss, so the sum does not depend on anything but the slot contents), writes the record at
 * hist[*cursor] and advances the cursor; every lane zeroes its slot.  Like the epoch word of
 * kernels_shuffle.hip the cursor lives on the device, so a replayed graph of several epochs
 * files its records one after the other and the host reads the history once, after the last
 * replay.  A cursor at the capacity drops the record (the host sizes the history from the
 * schedule, so that does not happen).  Plain vector loads and stores; no workgroup waits for
 * another.
 */
#include <hip/hip_runtime.h>

#include "kernels.h"

HPNN_CO_PROBE(validate)

namespace {

__global__ __launch_bounds__(64) void validate_commit_kernel(float *__restrict__ slots,
                                                             hpnn_val_record *__restrict__ hist,
                                                             unsigned int *__restrict__ cursor, unsigned int cap) {
    __shared__ double sl[HPNN_STAT_SLOTS];
    __shared__ unsigned int sh[HPNN_STAT_SLOTS];
    const unsigned int i = threadIdx.x;
    float *p = slots + (size_t)i * HPNN_STAT_STRIDE;
    /* the BF16 kernels add a float at [0], the FP64 / FP32 engines a double at floats 2..3 */
    sl[i] = (double)p[0] + ((const double *)p)[1];
    sh[i] = ((const unsigned int *)p)[1];
    p[0] = 0.f;
    ((unsigned int *)p)[1] = 0u;
    ((double *)p)[1] = 0.0;
    __syncthreads();
    if (i != 0) return;
    double loss = 0.0;
    unsigned int hits = 0;
    for (int k = 0; k < HPNN_STAT_SLOTS; k++) {
        loss += sl[k];
        hits += sh[k];
    }
    const unsigned int c = *cursor;
    if (c >= cap) return;
    hist[c].loss_sum = loss;
    hist[c].hits = hits;
    hist[c].pad = 0;
    *cursor = c + 1;
}

__global__ __launch_bounds__(256) void argmax_rows_kernel(const float *__restrict__ Z, int ldz, int n_out, int rows,
                                                          int n_valid, int *__restrict__ guess) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int bi = -1;
    if (r < n_valid) {
        const float *z = Z + (size_t)r * ldz;
        float bz = -INFINITY;
        bi = 1 << 30; /* what the fused kernel leaves when no logit compares (NaN rows) */
        for (int c = 0; c < n_out; c++)
            if (z[c] > bz) bz = z[c], bi = c;
    }
    guess[r] = bi;
}

}  // namespace

extern "C" int hpnn_argmax_rows(const float *Z, int ldz, int n_out, int rows, int n_valid, int *guess,
                                hipStream_t stream) {
    if (!Z || !guess || rows < 1 || n_out < 1 || ldz < n_out) return -1;
    hipLaunchKernelGGL(argmax_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, Z, ldz, n_out, rows, n_valid,
                       guess);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_validate_commit(float *slots, hpnn_val_record *hist, unsigned int *cursor, unsigned int cap,
                                    hipStream_t stream) {
    if (!slots || !hist || !cursor) return -1;
    hipLaunchKernelGGL(validate_commit_kernel, dim3(1), dim3(HPNN_STAT_SLOTS), 0, stream, slots, hist, cursor, cap);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
