/*
 * The MFMA-fragment-major layout of a BF16 weight matrix (Wf of hpnn_upd_layer, kernels.h), the
 * operand layout of the register-resident first-layer weights: element (n, k) of a [N][K] layer
 * lies at
 *   (((n / 16) * (K / 32) + k / 32) * 64 + n % 16 + 16 * ((k / 8) % 4)) * 8 + k % 8
 * so the 8 (and any aligned 4) consecutive k of one n stay contiguous.  The kernels of csrc/gpu
 * that write a Wf take the offset from here; xar_update4 (csrc/dist/xgmi_ar.hip) spells the same
 * expression out.
 */
#ifndef HPNN_GPU_FRAG_MAJOR_H
#define HPNN_GPU_FRAG_MAJOR_H
#include <hip/hip_runtime.h>
#include <stddef.h>

__host__ __device__ inline size_t hpnn_frag_major_offset(int n, int k, int K) {
    return (((size_t)(n >> 4) * (K / 32) + (k >> 5)) * 64 + (n & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7);
}

#endif /* HPNN_GPU_FRAG_MAJOR_H */
