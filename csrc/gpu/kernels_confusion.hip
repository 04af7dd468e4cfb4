/*
 * Per-class validation metrics inside the captured epoch graph ([confusion], gfx950): the
 * confusion matrix of a validation pass, tallied on the device (docs/DESIGN.md 3.2l; the rule is
 * <libhpnn/confusion.h>).
 *
 *   hpnn_confusion_add      adds the rows of one evaluation chunk -- the guess the evaluation
 *                           kernels wrote and the chunk's targets -- into M[n_out][n_out + 1]
 *   hpnn_confusion_commit   files the pass: the per-class record into pc_hist[*cursor], M copied
 *                           to `last`, M zeroed for the next pass
 *
 * One graph replay holds several validation passes; like the history of kernels_validate.hip and
 * the snapshot of kernels_best.hip everything a pass leaves behind stays in device memory, and the
 * captured launches are the same every replay.  The commit runs in front of hpnn_validate_commit
 * and reads the cursor that launch advances; `last` -> `best` is one more segment of the
 * hpnn_snapshot_if table under [keep_best].
 *
 * add: a workgroup of 256 lanes takes 256 / lpr rows at a time, lpr = 1 for int labels, else the
 * power of two >= n_out (at most 64) lanes per row: lane j of a row loads t[j], t[j + lpr], ...
 * (consecutive lanes, consecutive addresses) and keeps its first maximum, a butterfly over the lpr
 * lanes keeps the larger value and, of equal values, the lower index.  NaNs never compare, and a
 * NaN at t[0] gives class 0 -- the serial rule of hpnn_confusion_target_*.  The tally is one
 * unsigned integer atomic add per sample into M in global memory, nothing else: unsigned adds
 * commute, so the sums are the same bits whatever the grid.  There is one form for every n_out
 * (docs/DESIGN.md 3.2l, "One form").  No workgroup waits for another; plain vector stores only.
 *
 * commit: one workgroup.  Thread c derives class c's support (row sum), hit (diagonal) and
 * predicted (column sum); behind a barrier every thread copies its cells to `last` and zeroes
 * them.  A cursor at the capacity drops the record and nothing else, as hpnn_validate_commit.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include <libhpnn/confusion.h>

#include "kernels.h"

HPNN_CO_PROBE(confusion)

namespace {

constexpr int ADD_THREADS = 256;
constexpr int ADD_MAX_WGS = 256;
constexpr int COMMIT_THREADS = 1024;
constexpr int NO_INDEX = 0x7fffffff;

/* the target class of row r: lane `sub` of the row's lpr lanes; every lane of the row returns it */
template <typename TT>
__device__ __forceinline__ int target_of(const TT *__restrict__ tgt, int ldt, long r, int n_out, int sub, int lpr) {
    if constexpr (std::is_same<TT, int>::value) {
        return tgt[r];
    } else {
        const TT *__restrict__ t = tgt + (size_t)r * ldt;
        TT v = (TT)-INFINITY;
        int idx = NO_INDEX;
        for (int c = sub; c < n_out; c += lpr) {
            const TT x = t[c];
            if (x > v) v = x, idx = c;
        }
        const int first_nan = (sub == 0 && !(t[0] == t[0])) ? 1 : 0;
        for (int m = lpr >> 1; m >= 1; m >>= 1) {
            const TT ov = __shfl_xor(v, m, 64);
            const int oi = __shfl_xor(idx, m, 64);
            if (ov > v || (ov == v && oi < idx)) v = ov, idx = oi;
        }
        /* lane 0 of the row's lanes holds t[0] */
        const int nan0 = __shfl(first_nan, (threadIdx.x & 63) & ~(lpr - 1), 64);
        return (nan0 || idx == NO_INDEX) ? 0 : idx;
    }
}

template <typename TT>
__global__ __launch_bounds__(ADD_THREADS) void confusion_add_kernel(const int *__restrict__ guess,
                                                                    const TT *__restrict__ tgt, int ldt, int rows,
                                                                    int n_out, int lpr_log2,
                                                                    unsigned int *__restrict__ M) {
    const int lpr = 1 << lpr_log2, rpw = ADD_THREADS >> lpr_log2;
    const int sub = threadIdx.x & (lpr - 1), rl = threadIdx.x >> lpr_log2;
    for (long base = (long)blockIdx.x * rpw; base < rows; base += (long)gridDim.x * rpw) {
        const long r = base + rl;
        /* a row past the end is computed on the last row (its lanes stay in the butterfly) and
         * counts nowhere */
        const long rc = r < rows ? r : (long)rows - 1;
        const int g = guess[rc];
        const int t = target_of<TT>(tgt, ldt, rc, n_out, sub, lpr);
        const long long cell = (r < rows && sub == 0) ? hpnn_confusion_cell(t, g, n_out) : -1;
        if (cell >= 0) atomicAdd(&M[cell], 1u);
    }
}

__global__ __launch_bounds__(COMMIT_THREADS) void confusion_commit_kernel(unsigned int *__restrict__ M, int n_out,
                                                                          unsigned int *__restrict__ pc_hist,
                                                                          unsigned int *__restrict__ last,
                                                                          const unsigned int *__restrict__ cursor,
                                                                          unsigned int cap) {
    const unsigned int cur = *cursor;
    const size_t w = (size_t)n_out + 1;
    if (pc_hist && cur < cap) {
        unsigned int *__restrict__ rec = pc_hist + (size_t)cur * 3u * (size_t)n_out;
        for (int c = threadIdx.x; c < n_out; c += COMMIT_THREADS) {
            unsigned int row = 0u, col = 0u;
            for (int g = 0; g <= n_out; g++) row += M[(size_t)c * w + g];
            for (int t = 0; t < n_out; t++) col += M[(size_t)t * w + c];
            rec[c] = row;
            rec[n_out + c] = M[(size_t)c * w + c];
            rec[2 * n_out + c] = col;
        }
    }
    /* every sum above has read M before any cell is zeroed */
    __syncthreads();
    const size_t cells = (size_t)n_out * w;
    for (size_t i = threadIdx.x; i < cells; i += COMMIT_THREADS) {
        if (last) last[i] = M[i];
        M[i] = 0u;
    }
}

template <typename TT>
int launch_add(const int *guess, const void *tgt, int ldt, int rows, int n_out, unsigned int *M, hipStream_t stream) {
    int lpr_log2 = 0;
    if (!std::is_same<TT, int>::value)
        while ((1 << lpr_log2) < n_out && lpr_log2 < 6) lpr_log2++;
    const int rpw = ADD_THREADS >> lpr_log2;
    int grid = (rows + rpw - 1) / rpw;
    grid = grid < ADD_MAX_WGS ? grid : ADD_MAX_WGS;
    hipLaunchKernelGGL(confusion_add_kernel<TT>, dim3(grid), dim3(ADD_THREADS), 0, stream, guess, (const TT *)tgt, ldt,
                       rows, n_out, lpr_log2, M);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace

/* loads the unit's code object (an empty launch and a synchronise) before a capture */
extern "C" int hpnn_confusion_preload(hipStream_t stream) {
    hipLaunchKernelGGL(hpnn_co_probe_kernel_confusion, dim3(1), dim3(1), 0, stream);
    if (hipGetLastError() != hipSuccess) return -5;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_confusion_add(const int *guess, const void *targets, int ldt, int t_kind, int rows, int n_out,
                                  unsigned int *M, hipStream_t stream) {
    if (!guess || !targets || !M || rows < 0 || n_out < 1 || n_out > HPNN_CONFUSION_MAX_NOUT) return -1;
    if (((uintptr_t)guess & 3u) || ((uintptr_t)M & 3u)) return -1;
    if (t_kind == HPNN_CONFUSION_LABELS) {
        if ((uintptr_t)targets & 3u) return -1;
    } else if (t_kind == HPNN_CONFUSION_F32 || t_kind == HPNN_CONFUSION_F64) {
        if (ldt < n_out || ((uintptr_t)targets & (t_kind == HPNN_CONFUSION_F64 ? 7u : 3u))) return -1;
    } else {
        return -1;
    }
    if (rows == 0) return 0;
    switch (t_kind) {
        case HPNN_CONFUSION_LABELS: return launch_add<int>(guess, targets, ldt, rows, n_out, M, stream);
        case HPNN_CONFUSION_F32: return launch_add<float>(guess, targets, ldt, rows, n_out, M, stream);
        default: return launch_add<double>(guess, targets, ldt, rows, n_out, M, stream);
    }
}

extern "C" int hpnn_confusion_commit(unsigned int *M, int n_out, unsigned int *pc_hist, unsigned int *last,
                                     const unsigned int *cursor, unsigned int cap, hipStream_t stream) {
    if (!M || !cursor || n_out < 1 || n_out > HPNN_CONFUSION_MAX_NOUT) return -1;
    if (((uintptr_t)M | (uintptr_t)pc_hist | (uintptr_t)last | (uintptr_t)cursor) & 3u) return -1;
    hipLaunchKernelGGL(confusion_commit_kernel, dim3(1), dim3(COMMIT_THREADS), 0, stream, M, n_out, pc_hist, last,
                       cursor, cap);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
