/*
 * Per-epoch reshuffle of the device-resident training set ([shuffle] epoch, gfx950).
 *
 *   hpnn_epoch_perm_dev   perm[i] = src(i) of <libhpnn/shuffle.h>, the epoch read from a
 *                         device word
 *   hpnn_epoch_advance    that word += 1, a one-thread launch of its own behind the readers
 *   hpnn_gather_rows      row-major dst row i = src row perm[i]; zero rows from n up
 *   hpnn_gather_fm        row-major src -> fragment-major dst (ops.to_fragment_major) of the
 *                         permuted rows; zero rows from n up
 *
 * Everything is a plain launch on the caller's stream (capturable into the epoch graph);
 * no workgroup waits for another.
 *
 * hpnn_gather_fm: one 256-thread workgroup per 32-row destination tile, looping over column
 * chunks of CB = 1024 bytes per row.  Load: wave w stages rows 8 w .. 8 w + 7 of the tile,
 * one row chunk per wave instruction (16 B per lane, 1 KiB coalesced), into an LDS image
 * [32][CB].  Store: wave w assembles the fragments cb = w, w + 4, .. of the chunk: lane
 * 16 g + r reads its 8 elements from rows 8 g + j, column 16 cb + r, and stores 8 (u8) or 16
 * (bf16) contiguous bytes, so a wave writes one whole 512 B / 1 KiB fragment.
 * LDS banks (the bank of byte address a is (a/4) % 32 for these sub-dword reads and for every
 * write, per 32-lane half): the lanes of one half read rows 8 g + j for two values of g.  With
 * any 16-byte-aligned pitch P, 8 P is a multiple of 32 dwords, so padding the pitch cannot
 * separate them; instead row R is stored rotated by 32 (R / 8) bytes within its chunk
 * (byte c of row R at R CB + (c + 32 (R >> 3)) % CB).  The 16 columns of a fragment span 4
 * (u8) or 8 (bf16) banks, so g and g + 1 read disjoint banks, and a row's 16-byte writes stay
 * contiguous and conflict-free.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <libhpnn/shuffle.h>

#include "kernels.h"

HPNN_CO_PROBE(shuffle)

namespace {

__global__ __launch_bounds__(256) void epoch_perm_kernel(int *__restrict__ perm, unsigned int n, unsigned int seed,
                                                         const unsigned int *__restrict__ epoch_word,
                                                         unsigned int *__restrict__ err) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    hpnn_shuffle_keys k;
    hpnn_shuffle_setup(&k, n, seed, *epoch_word);
    int over = 0;
    const unsigned int v = hpnn_shuffle_src(&k, i, HPNN_SHUFFLE_MAX_WALK, &over);
    if (over) atomicOr(err, 1u);
    perm[i] = (int)v;
}

/* a launch of its own behind epoch_perm_kernel: no thread reads the word while it changes
 * (stream order) */
__global__ void epoch_advance_kernel(unsigned int *epoch_word) { *epoch_word += 1u; }

/* V = uint4 (16-byte rows and pointers) or unsigned int; vpr = V's per row.  A workgroup
 * takes 256 / vpr whole rows per pass (one row when vpr >= 256): the only division is one per
 * thread, and a row's index is read once per thread */
template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(V *__restrict__ dst, const V *__restrict__ src,
                                                          const int *__restrict__ perm, unsigned int n, long rows_p,
                                                          unsigned int vpr) {
    const unsigned int tid = threadIdx.x;
    const unsigned int rpb = vpr >= 256u ? 1u : 256u / vpr;
    const unsigned int lr = vpr >= 256u ? 0u : tid / vpr;
    const unsigned int lc = tid - lr * vpr;
    if (lr >= rpb) return;
    for (long row = (long)blockIdx.x * rpb + lr; row < rows_p; row += (long)gridDim.x * rpb) {
        const V *s = nullptr;
        if (row < (long)n) {
            const unsigned int p = (unsigned int)perm[row];
            if (p < n) s = src + (size_t)p * vpr;
        }
        V *d = dst + (size_t)row * vpr;
        for (unsigned int c = lc; c < vpr; c += 256u) d[c] = s ? s[c] : V();
    }
}

constexpr int FM_CB = 1024; /* chunk bytes per row */

template <int EB>
__global__ __launch_bounds__(256) void gather_fm_kernel(unsigned char *__restrict__ dst,
                                                        const unsigned char *__restrict__ src,
                                                        const int *__restrict__ perm, unsigned int n, int Kp) {
    __shared__ __attribute__((aligned(16))) unsigned char img[32 * FM_CB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long t = blockIdx.x;
    const long row_bytes = (long)Kp * EB;
    const int nbc = Kp / 16;
    const int g = lane >> 4, r = lane & 15;
    for (long c0 = 0; c0 < row_bytes; c0 += FM_CB) {
        const int cb_bytes = (int)(row_bytes - c0 < FM_CB ? row_bytes - c0 : FM_CB);
        if (c0) __syncthreads(); /* the previous chunk's reads are done */
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int R = wave * 8 + j;
            const long i = t * 32 + R;
            const int off = lane * 16;
            if (off < cb_bytes) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (i < (long)n) {
                    const unsigned int p = (unsigned int)perm[i];
                    if (p < n) v = *(const uint4 *)(src + (size_t)p * row_bytes + c0 + off);
                }
                *(uint4 *)(img + R * FM_CB + ((off + 32 * (R >> 3)) & (FM_CB - 1))) = v;
            }
        }
        __syncthreads();
        const int nfrag = cb_bytes / (16 * EB);
        const int cb0 = (int)(c0 / (16 * EB));
        for (int f = wave; f < nfrag; f += 4) {
            const int colb = (f * 16 + r) * EB; /* byte column within the chunk */
            unsigned int w[2 * EB];
#pragma unroll
            for (int q = 0; q < 2 * EB; q++) w[q] = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int R = 8 * g + j;
                const unsigned char *a = img + R * FM_CB + ((colb + 32 * g) & (FM_CB - 1));
                if constexpr (EB == 1) w[j >> 2] |= (unsigned int)a[0] << (8 * (j & 3));
                else w[j >> 1] |= (unsigned int)*(const unsigned short *)a << (16 * (j & 1));
            }
            unsigned char *o = dst + (((size_t)t * nbc + cb0 + f) * 64 + lane) * (8 * EB);
            if constexpr (EB == 1) *(uint2 *)o = make_uint2(w[0], w[1]);
            else *(uint4 *)o = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

}  // namespace

extern "C" int hpnn_epoch_perm_dev(int *perm, int n, unsigned int seed, const unsigned int *epoch_word,
                                   unsigned int *err, hipStream_t stream) {
    if (!perm || !epoch_word || !err || n < 0) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(epoch_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, perm,
                       (unsigned int)n, seed, epoch_word, err);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_epoch_advance(unsigned int *epoch_word, hipStream_t stream) {
    if (!epoch_word) return -1;
    hipLaunchKernelGGL(epoch_advance_kernel, dim3(1), dim3(1), 0, stream, epoch_word);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_gather_rows(void *dst, const void *src, const int *perm, int n, long rows_p, long row_bytes,
                                hipStream_t stream) {
    if (!dst || !src || !perm || n < 0 || rows_p < n || row_bytes <= 0 || row_bytes % 4) return -1;
    if (rows_p == 0) return 0;
    const bool v16 = row_bytes % 16 == 0 && (((uintptr_t)dst | (uintptr_t)src) & 15) == 0;
    const long vpr = row_bytes / (v16 ? 16 : 4);
    if (vpr > 0x7fffffffL) return -1;
    const long rpb = vpr >= 256 ? 1 : 256 / vpr;
    long blocks = (rows_p + rpb - 1) / rpb;
    if (blocks > 65536) blocks = 65536;
    if (v16)
        hipLaunchKernelGGL(gather_rows_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, stream, (uint4 *)dst,
                           (const uint4 *)src, perm, (unsigned int)n, rows_p, (unsigned int)vpr);
    else
        hipLaunchKernelGGL(gather_rows_kernel<unsigned int>, dim3((unsigned)blocks), dim3(256), 0, stream,
                           (unsigned int *)dst, (const unsigned int *)src, perm, (unsigned int)n, rows_p,
                           (unsigned int)vpr);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_gather_fm(void *dst, const void *src_rowmajor, const int *perm, int n, long rows_p, int Kp,
                              int elem_bytes, hipStream_t stream) {
    if (!dst || !src_rowmajor || !perm || n < 0 || rows_p < n || rows_p % 32 || Kp <= 0 || Kp % 16) return -1;
    if (elem_bytes != 1 && elem_bytes != 2) return -1;
    if ((((uintptr_t)dst | (uintptr_t)src_rowmajor) & 15) != 0) return -1;
    const long tiles = rows_p / 32;
    if (tiles == 0) return 0;
    if (tiles > 0x7fffffffL) return -1;
    if (elem_bytes == 1)
        hipLaunchKernelGGL(gather_fm_kernel<1>, dim3((unsigned)tiles), dim3(256), 0, stream, (unsigned char *)dst,
                           (const unsigned char *)src_rowmajor, perm, (unsigned int)n, Kp);
    else
        hipLaunchKernelGGL(gather_fm_kernel<2>, dim3((unsigned)tiles), dim3(256), 0, stream, (unsigned char *)dst,
                           (const unsigned char *)src_rowmajor, perm, (unsigned int)n, Kp);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
