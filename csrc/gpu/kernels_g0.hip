/*
 * Weight-gradient GEMM over fragment-major operands, direct-to-register loads (gfx950).
 *
 *   slab[s][n][m] = sum over the batch rows b of split s of  D[b][n] * H[b][m]
 *
 * (the product of hpnn_gemm_tn_bf16) with both operands stored FRAGMENT-MAJOR:
 * A[b][c] -> [b / 32][c / 16][64 lanes][8], lane l = 16 g + r of fragment (t, cb) holding
 * A[32 t + 8 g + j][16 cb + r], j < 8 -- exactly the per-lane operand of
 * v_mfma_f32_16x16x32_bf16 with k running over the batch (A[row = l&15][k = 8(l>>4)+j]).
 * Every operand fragment is then one contiguous 1 KiB wave load straight into VGPRs; no
 * LDS, no transposes.  Reference: the per-sample weight update of ann_kernel_train /
 * snn_kernel_train (ann.c:1279-1592, cuda_ann.cu ger_acc), batched.
 *
 * Used for MNIST's first-layer gradient G0 = delta1^T X (800 x 128 over 65536 rows): the
 * fused front (kernels_mlp3x.hip, d1fm) writes delta1 in this layout, and an 8-bit pixel
 * batch keeps a fragment-major copy of its bytes, made once when it is prepared
 * (MLP.prepare_input): half the bytes of the BF16 batch, converted in registers to the
 * same bf16(pixel * scale) values the front computes with (8 waves hide the conversion).
 * In the step: 72.5-72.7 us with it vs 74.8-75.6 us for the LDS-DMA TN kernel on the
 * BF16 batch; cold 26.5 us vs 34 standalone (round-2 A/B scripts, since pruned).
 * Measured (48 splits): LDS-staged TN kernel 31.2 us (its LDS-DMA
 * fill, ~27 GB/s per CU, is the bound); this kernel 23.8 us, ~5.1 TB/s of HBM reads --
 * it streams at the memory rate.  Round 4, again: that round's 160 x 128 tiles with the operands
 * LDS-DMA staged (two k-steps of contiguous fragments per stage, 3-4 stages in flight, no VGPR
 * staging) took 72.9-74.1 vs 61.3-62.0 us per MNIST step (profiles/r4).  Rejected on the way: the same kernel on plain
 * batch-contiguous (transposed row-major) operands, 51 us -- each wave load then hits
 * 16 rows x 64 B, 64 L1 tag lookups per instruction instead of 8, and the vector L1 tag
 * rate (~1 lookup per clock per CU, TCP_TOTAL_CACHE_ACCESSES) is the limit; grouping 2-4
 * k-steps per row visit or padding the row pitch did not change that.
 *
 * Workgroup: WM x WN x KW waves.  The WM x WN waves (wm, wn) of a k-group cover a
 * 16 WF WM x 16 WH WN output tile (wave tile 16 WF x 16 WH); group kg of KW takes the 32-row
 * k-steps kg, kg + KW, ... of the workgroup's split and the groups' partial tiles meet in LDS
 * at the end (fixed order).  Each wave keeps PD k-steps of operands in flight in a register
 * ring (PD + 1 slots; the loop is unrolled by PD + 1 so every slot index is static).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>

#include "frag_major.h"
#include "kernels.h"

HPNN_CO_PROBE(g0)
#include "mfma_common.h"

namespace {

/* HPNN_G0_PROTO hand-off diagnostics exist only in make ABLATIONS=1 builds */
#ifdef HPNN_ABLATIONS
#define G0_PROTO(u, bit) ((u).proto & (bit))
#else
#define G0_PROTO(u, bit) 0
#endif

using hpnn::bf16x8;
using hpnn::f32x4;
using hpnn::TnTail;
using hpnn::gu32;
using hpnn::sum_sc1_x8;
using hpnn::st_sc1;

/* Dg: [Bt/32][N/16][64][8], Hg: [Bt/32][M/16][64][8]; nbd = N / 16, nbh = M / 16.
 * HU8: Hg holds unsigned bytes (8 per lane per fragment), multiplied as exact integers;
 * hscale scales the FP32 result (G = hscale * D^T H) */
/* the workgroup's partial product over its split of the batch: on return the waves of group
 * kg == 0 hold the 16 WF WM x 16 WH WN tile (wave tile 16 WF x 16 WH) in acc; tile, split and
 * m0 / n0 (this wave's tile origin) are set.  Every wave returns (the caller's barriers need
 * them). */
/* workgroup role: (virtual) block b -> output tile and batch split.  xcd_map: the tiles of
 * one batch slice share b % 8, i.e. one XCD under the observed round-robin placement, so the
 * slice's Dt rows are fetched once into that L2 -- a speed assumption only: every result is
 * the same whichever block takes which role (fixed-order sums; tests permute the order).
 * 8 * (splits / 8) splits map that way; the rest (splits not a multiple of 8) take the last
 * blocks in plain order */
__device__ __forceinline__ void fm_role(int b, int splits, int tiles, int xcd_map, int &tile, int &split) {
    if (xcd_map) {
        const int main = (splits / 8) * 8 * tiles;
        if (b < main) {
            const int xcd = b & 7, j = b >> 3;
            tile = j % tiles;
            split = xcd + 8 * (j / tiles);
        } else {
            tile = (b - main) % tiles;
            split = (splits / 8) * 8 + (b - main) / tiles;
        }
    } else {
        tile = b % tiles;
        split = b / tiles;
    }
}

template <bool WIDE, int WF, int WH, int PD, int KW, bool HU8, int WM = 2, int WN = 2, bool X16 = false>
__device__ __forceinline__ void fm_partial(const __bf16 *__restrict__ Dg, int nbd, const void *__restrict__ Hg, int nbh,
                                           int ksteps, int splits, int tiles_n, int tiles, int xcd_map, int vb,
                                           f32x4 (&acc)[WF][WH], int &tile, int &split, int &m0, int &n0) {
    constexpr int R = PD + 1;
    constexpr int GW = WM * WN;                   /* waves per k-group */
    constexpr int TMF = 16 * WF * WM, TNH = 16 * WH * WN; /* workgroup tile: features x delta columns */
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kg = wave / GW, wm = (wave % GW) / WN, wn = wave % WN;
    fm_role(vb, splits, tiles, xcd_map, tile, split);
    m0 = (tile / tiles_n) * TMF + wm * 16 * WF;
    n0 = (tile % tiles_n) * TNH + wn * 16 * WH;
    const int k0 = (int)((long)split * ksteps / splits), k1 = (int)((long)(split + 1) * ksteps / splits);
    /* this wave group's k-steps: k0 + kg, k0 + kg + KW, ... */
    const int nk = (k1 - k0 - kg + KW - 1) / KW;
    const int r16 = lane & 15;
    constexpr int ES = HU8 ? 1 : 2; /* bytes per H element */
    using HT = typename std::conditional<HU8, uint2, bf16x8>::type;
    const char *pa = (const char *)Hg + (((size_t)(k0 + kg) * nbh + m0 / 16) * 512 + lane * 8) * ES;
    const __bf16 *pb = Dg + ((size_t)(k0 + kg) * nbd + n0 / 16) * 512 + lane * 8;
    const size_t step_a = (size_t)KW * nbh * 512 * ES, step_b = (size_t)KW * nbd * 512; /* this group's next k-step */

#pragma unroll
    for (int i = 0; i < WF; i++)
#pragma unroll
        for (int j = 0; j < WH; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    HT ra[R][WF];
    bf16x8 rb[R][WH];
    auto load = [&](int slot_, int t) __attribute__((always_inline)) {
        const int tc = t < nk - 1 ? t : nk - 1; /* clamped: the ring tail re-reads the last step */
        if constexpr (X16 && HU8) {
            /* timing ablation (make ABLATIONS=1, HPNN_G0_X16=1; wrong results): fragment pairs
             * through one 16-byte load per lane instead of two 8-byte loads */
            typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
#pragma unroll
            for (int i = 0; i + 1 < WF; i += 2) {
                const u32x4 v = *(const u32x4 *)(pa - lane * 8 + lane * 16 + i * 512 + (size_t)tc * step_a);
                ra[slot_][i] = HT{v.x, v.y};
                ra[slot_][i + 1] = HT{v.z, v.w};
            }
            if constexpr (WF % 2) ra[slot_][WF - 1] = *(const HT *)(pa + (WF - 1) * 512 + (size_t)tc * step_a);
        } else {
#pragma unroll
            for (int i = 0; i < WF; i++) ra[slot_][i] = *(const HT *)(pa + i * 512 * ES + (size_t)tc * step_a);
        }
#pragma unroll
        for (int j = 0; j < WH; j++) rb[slot_][j] = *(const bf16x8 *)(pb + j * 512 + (size_t)tc * step_b);
    };
    auto mma = [&](int slot_) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < WF; i++) {
            bf16x8 a;
            if constexpr (HU8) a = hpnn::u8x8_int_bf16(ra[slot_][i].x, ra[slot_][i].y);
            else a = ra[slot_][i];
#pragma unroll
            for (int j = 0; j < WH; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, rb[slot_][j], acc[i][j], 0, 0, 0);
        }
    };
    if (nk > 0) {
#pragma unroll
        for (int p = 0; p < PD; p++) load(p, p);
        int t = 0;
        for (; t + R <= nk; t += R) {
#pragma unroll
            for (int u = 0; u < R; u++) {
                /* program order = issue order: the loads of step t+u+PD go out before the
                 * MFMAs of step t+u, so waiting for step t+u leaves PD steps in flight
                 * (without the barriers the scheduler sinks loads below MFMAs and the
                 * waitcnt pass drains the ring to vmcnt(0) every step) */
                load((u + PD) % R, t + u + PD);
                __builtin_amdgcn_sched_barrier(0);
                mma(u);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        /* remaining nk - t < R steps sit in slots 0.. already (PD = R - 1 loads ahead) */
#pragma unroll
        for (int u = 0; u < R - 1; u++)
            if (t + u < nk) mma(u);
    }

    if constexpr (KW > 1) {
        /* groups 1.. hand their partial tiles to group 0 through LDS (dynamic: fm_meet_bytes).
         * WIDE: every group has an area of its own, all write at once and ONE barrier follows;
         * else one area, a write / barrier / add / barrier round per group.  Group 0 adds in
         * the order g = 1, 2, ... either way: the same bits */
        extern __shared__ __attribute__((aligned(16))) char fm_meet[];
        constexpr int AREA = GW * WF * WH * 64; /* f32x4 per group */
        f32x4 *const part = (f32x4 *)fm_meet + (wave % GW) * (WF * WH * 64) + lane;
        if constexpr (WIDE) {
            if (kg > 0) {
#pragma unroll
                for (int i = 0; i < WF; i++)
#pragma unroll
                    for (int j = 0; j < WH; j++) part[(kg - 1) * AREA + (i * WH + j) * 64] = acc[i][j];
            }
            __syncthreads();
            if (kg == 0) {
                /* one row of WH accumulators at a time, its (KW - 1) WH reads in flight together
                 * (all WF rows at once would cost the registers of a second accumulator tile) */
#pragma unroll
                for (int i = 0; i < WF; i++) {
                    f32x4 p[KW - 1][WH];
#pragma unroll
                    for (int g = 1; g < KW; g++)
#pragma unroll
                        for (int j = 0; j < WH; j++) p[g - 1][j] = part[(g - 1) * AREA + (i * WH + j) * 64];
#pragma unroll
                    for (int g = 1; g < KW; g++)
#pragma unroll
                        for (int j = 0; j < WH; j++) acc[i][j] += p[g - 1][j];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
#pragma unroll
            for (int g = 1; g < KW; g++) {
                if (kg == g) {
#pragma unroll
                    for (int i = 0; i < WF; i++)
#pragma unroll
                        for (int j = 0; j < WH; j++) part[(i * WH + j) * 64] = acc[i][j];
                }
                __syncthreads();
                if (kg == 0) {
#pragma unroll
                    for (int i = 0; i < WF; i++)
#pragma unroll
                        for (int j = 0; j < WH; j++) acc[i][j] += part[(i * WH + j) * 64];
                }
                if (g + 1 < KW) __syncthreads();
            }
        }
    }
}

/* dynamic LDS of a launch whose k-groups meet through fm_partial: one 16 WF WM x 16 WH WN FP32
 * tile per area, KW - 1 areas when wide */
template <int WF, int WH, int KW, int WM, int WN>
constexpr size_t fm_meet_bytes(bool wide) {
    return KW > 1 ? (size_t)(wide ? KW - 1 : 1) * WM * WN * WF * WH * 64 * sizeof(f32x4) : 0;
}

int g0_cus() {
    static const int cus = [] {
        int dev = 0, n = 0;
        return hipGetDevice(&dev) == hipSuccess &&
                       hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess
                   ? n
                   : 0;
    }();
    return cus;
}

/* more than 64 KiB of dynamic LDS needs the attribute, once per kernel and device */
template <auto KERN>
void fm_allow_lds(size_t bytes) {
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 63; /* unknown: set it every time */
    const unsigned long long bit = 1ull << dev;
    if (dev < 63 && (done.load(std::memory_order_relaxed) & bit)) return;
    (void)hipFuncSetAttribute((const void *)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    done.fetch_or(bit, std::memory_order_relaxed);
}

template <bool WIDE, int WF, int WH, int PD, int KW, bool HU8 = false, int WM = 2, int WN = 2>
/* (3 waves per SIMD: the register budget the meeting's static LDS used to imply) */
__global__ __launch_bounds__(64 * WM * WN * KW, KW > 1 ? 3 : 1) void gemm_fm_direct_kernel(
                                                                  const __bf16 *__restrict__ Dg, int nbd,
                                                                  const void *__restrict__ Hg, int nbh, float hscale,
                                                                  float *__restrict__ slab, int ldg, int N, int ksteps,
                                                                  int splits, int tiles_n, int tiles, int xcd_map,
                                                                  TnTail tail) {
    if ((int)blockIdx.x >= tiles * splits) {
        if (threadIdx.x < 256) hpnn::tn_tail_reduce(tail, (int)blockIdx.x - tiles * splits);
        return;
    }
    f32x4 acc[WF][WH];
    int tile, split, m0, n0;
    fm_partial<WIDE, WF, WH, PD, KW, HU8, WM, WN>(Dg, nbd, Hg, nbh, ksteps, splits, tiles_n, tiles, xcd_map,
                                                  (int)blockIdx.x, acc, tile, split, m0, n0);
    if ((threadIdx.x >> 6) >= WM * WN) return;
    const int lane = threadIdx.x & 63, r16 = lane & 15, q = lane >> 4;
    float *out = slab + (size_t)split * N * ldg;
#pragma unroll
    for (int i = 0; i < WF; i++)
#pragma unroll
        for (int j = 0; j < WH; j++)
            *(f32x4 *)(out + (size_t)(n0 + j * 16 + r16) * ldg + m0 + i * 16 + 4 * q) =
                HU8 ? acc[i][j] * hscale : acc[i][j];
}

/* ---- G0 with its split-K reduction and the optimizer step in the same launch ----------
 * (the single-GPU MNIST step: front, then this, two launches).  Every GEMM workgroup
 * publishes its FP32 partial tile with write-through (sc1) stores, drains them and adds one
 * ticket to its tile's monotonic counter (agent scope); it then waits (sc1 polls, bounded)
 * until all `splits` partials of the tile have arrived, reduces its 1/splits share of the
 * tile over the splits in a FIXED order (sc1 loads; bitwise repeatable whatever the arrival
 * order) and applies the BP / BPM step to those elements: FP32 master, momentum, BF16 W,
 * W^T and the fragment-major copy the front reads (a copy whose pointer is NULL is not kept:
 * the tile path's plain step leaves W0, W0^T and W1^T to BPlan::sync_copies).  The front's
 * [G1 | G2] block slabs are
 * summed completely (fixed order) and layers 1 and 2 stepped by TAIL workgroups appended to
 * the grid, on the CUs the GEMM grid leaves idle (MNIST: 240 GEMM workgroups + 16 tails on 256
 * CUs): the 9 MB of slab reads run beside the GEMM instead of after every workgroup's publish
 * (-2.7 us per step on a slow box, profiles/r6).  A launch without tails (no idle CU, or
 * HPNN_G0_TAILS=0) leaves [G1 | G2] to the GEMM workgroups, a 1 / (tiles x splits) share
 * each between their ticket and their wait.  Tails wait for nothing, so any dispatch order is
 * deadlock-free.  Output tiles are 80 x 128 (10 tiles x 24 splits on MNIST): half the
 * split-K partial bytes of 160 x 128 tiles x 48 splits (profiles/r6/SUMMARY.md).  Replaces
 * the separate sgd_update_multi launch (6.2 us) and its kernel boundary behind 20 MB of dirty
 * slabs.  All GEMM workgroups are co-resident (grid <= CUs; a wait that times out sets *err
 * instead of hanging).  An XCD-local first level of the split-K reduction was tried and
 * measured slower (profiles/r6/SUMMARY.md).  Reference: the per-layer update of
 * snn_kernel_train_momentum / cuda_snn.cu:2726-3717 (GER into dW, W += dW, dW *= alpha),
 * batched. */
constexpr unsigned long long G0_TIMEOUT = 1000000000ULL; /* wall-clock ticks (~10 s) */

/* the master weight / momentum of the first element a thread steps, loaded right after the
 * GEMM so the load is in flight through the publish, ticket and split-sum waits instead of
 * in series after them (passed by value with a flag: a pointer to it would put it on the
 * stack) */
struct Pre4 {
    f32x4 w, v;
};

__device__ __forceinline__ void bpm_step4(float *__restrict__ W32, float *__restrict__ V32, size_t idx, f32x4 g,
                                          const hpnn_g0_update &u, f32x4 &w, bool use = false, Pre4 pre = {}) {
    w = use ? pre.w : *(const f32x4 *)(W32 + idx);
    if (u.momentum) {
        f32x4 v = use ? pre.v : *(const f32x4 *)(V32 + idx);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            v[r] += u.lr * (g[r] * u.scale);
            w[r] += v[r];
            v[r] *= u.alpha;
        }
        *(f32x4 *)(V32 + idx) = v;
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++) w[r] += u.lr * (g[r] * u.scale);
    }
    *(f32x4 *)(W32 + idx) = w;
}

/* element (n, k..k+3) of a [N][K] layer: FP32 master + the BF16 copies the caller keeps current
 * (W, fragment-major Wf, W^T; a NULL one is left alone: four scattered 2-byte stores for W^T) */
__device__ __forceinline__ void step_elem4(float *W32, float *V32, __bf16 *Wb, __bf16 *Wt, __bf16 *Wf, int N, int K,
                                           int n, int k, f32x4 g, const hpnn_g0_update &u, bool use = false,
                                           Pre4 pre = {}) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    const size_t idx = (size_t)n * K + k;
    f32x4 w;
    bpm_step4(W32, V32, idx, g, u, w, use, pre);
    bf16x4 wb;
#pragma unroll
    for (int r = 0; r < 4; r++) wb[r] = (__bf16)w[r];
    if (Wb) *(bf16x4 *)(Wb + idx) = wb;
    if (Wf) { /* MFMA-fragment-major copy (frag_major.h): 4 consecutive k stay contiguous */
        *(bf16x4 *)(Wf + hpnn_frag_major_offset(n, k, K)) = wb;
    }
    if (Wt && !G0_PROTO(u, 2048)) /* 2048: timing ablation, no W^T stores */
#pragma unroll
        for (int r = 0; r < 4; r++) Wt[(size_t)(k + r) * N + n] = wb[r];
}

/* element i of a small array inside the by-value kernel argument, as a chain of selects: a
 * DYNAMIC index into the argument makes the compiler copy the whole 440-byte struct into every
 * thread's scratch at kernel start (seen in the ISA: scratch_store_dwordx4 x 28 per thread) */
template <class T, int N>
__device__ __forceinline__ T pick(const T (&a)[N], int i) {
    T r = a[0];
#pragma unroll
    for (int k = 1; k < N; k++) r = i == k ? a[k] : r;
    return r;
}

/* float4 e4 of [G1 | G2] -> layer l, row n, column k */
__device__ __forceinline__ int g12_elem(const hpnn_g0_update &u, long e4, int &n, int &k) {
    long i = e4 * 4;
    const long n1 = (long)u.Nb[0] * u.Kb[0];
    const int l = i < n1 ? 0 : 1;
    if (l) i -= n1;
    const int kb = pick(u.Kb, l);
    n = (int)(i / kb), k = (int)(i % kb);
    return l;
}
__device__ __forceinline__ Pre4 pre_load(const float *W32, const float *V32, size_t idx, int momentum) {
    Pre4 p;
    p.w = *(const f32x4 *)(W32 + idx);
    p.v = momentum ? *(const f32x4 *)(V32 + idx) : f32x4{0.f, 0.f, 0.f, 0.f};
    return p;
}

/* [G1 | G2]: float4 columns [c0, c1) of the front's block slabs summed over all mrows rows in
 * a fixed order, then layers 1 / 2 stepped at those elements (or the sums stored into g12out).
 * A pass takes C4 columns x RG = NT / C4 row groups, each thread with RB rows' loads in flight
 * (a dependent one-at-a-time walk over the rows is latency-bound: a pass is one L2 / Infinity
 * Cache round trip); the row groups meet in LDS in order.  GEMM workgroups (a launch without
 * tails: ~11 columns each on MNIST, between their ticket and their wait): 16 x 8, and the
 * first element's prefetched W / V (use, pre).  Tail workgroups (blocks past the GEMM grid,
 * on the CUs it leaves idle, beside the GEMM instead of after it), 1 / ntail of all columns
 * each: 32 columns (512 contiguous bytes of a row) x 16 rows */
template <int NT, int C4, int RB>
__device__ __forceinline__ void g12_share(const hpnn_g0_update &u, long c0, long c1, f32x4 *red, float *g12out,
                                          bool use = false, Pre4 pre = {}) {
    constexpr int RG = NT / C4;
    const int t = threadIdx.x, c = t % C4, rg = t / C4;
    for (long b0 = c0; b0 < c1; b0 += C4) {
        const long e4 = b0 + c;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (e4 < c1) {
            const float *col = u.mslab + e4 * 4;
            for (int r0 = rg; r0 < u.mrows; r0 += RB * RG) {
                f32x4 v[RB];
#pragma unroll
                for (int k = 0; k < RB; k++) {
                    const int r = r0 + k * RG;
                    v[k] = r < u.mrows ? *(const f32x4 *)(col + (long)r * u.mstride) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int k = 0; k < RB; k++) a += v[k];
            }
        }
        red[t] = a;
        __syncthreads();
        if (rg == 0 && e4 < c1) {
            f32x4 g = red[c];
            for (int r = 1; r < RG; r++) g += red[r * C4 + c];
            if (g12out) {
                *(f32x4 *)(g12out + e4 * 4) = g;
            } else {
                int n, k;
                const int l = g12_elem(u, e4, n, k);
                step_elem4(pick(u.W32b, l), pick(u.V32b, l), (__bf16 *)pick(u.Wbb, l), (__bf16 *)pick(u.Wtb, l), nullptr,
                           pick(u.Nb, l), pick(u.Kb, l), n,
                           k, g, u, use && b0 == c0 /* this thread's prefetched element */, pre);
            }
        }
        __syncthreads();
    }
}

/* sum of float4 at offset o over the first `world` ranks' buffers, rank order (identical bits
 * on every rank); all loads in flight at once, system-coherent (sc0 sc1: no cache can serve a
 * stale line, so no acquire fence -- an invalidating acquire per workgroup, while the other
 * workgroups still stream their split sums, cost ~10 us per step) */
static_assert(HPNN_XAR_MAX_RANKS == 8, "one ld_sc1_x8 per element");
__device__ __forceinline__ f32x4 xsum_peers(const hpnn_xar_view &v, long o) {
    const float *q[8];
#pragma unroll
    for (int p = 0; p < 8; p++) q[p] = pick(v.buf, p < v.world ? p : v.rank) + o; /* spare slots: local */
    f32x4 x[8];
    hpnn::ld_sc1_x8<true>(x, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
    f32x4 a = x[0];
#pragma unroll
    for (int p = 1; p < HPNN_XAR_MAX_RANKS; p++)
        if (p < v.world) a += x[p];
    return a;
}

/* data-parallel tail (u.xchg): this workgroup's reduced G0 share (float4 [e0, e1) of its
 * tile) and [G1 | G2] share sit in its half of this rank's exchange buffer (fine-grained,
 * uncached: no cache maintenance between ranks).  One-shot barrier of workgroup b (the
 * protocol of xgmi_ar.hip, release = waiting for the store acknowledgements), then the
 * rank-order sums over the peers' copies of exactly those elements and their steps: the
 * exchange and the update need no launch of their own. */
template <int NT>
__device__ __forceinline__ void g0_exchange_step(const hpnn_g0_update &u, unsigned int e, int N, int ldg, int e0, int e1,
                                              int nt0, int mt0, int TMF, bool pf, Pre4 pg0, Pre4 pg12, int b, long c0,
                                              long c1) {
    const hpnn_xar_view &v = u.xv;
    const int t = threadIdx.x;
    /* the exchanged sums: stepped, or (self-test, u.xres) stored at their flat offsets; the
     * fault hook (u.xfault, tests) corrupts the first G0 element of role 0 on this rank */
    auto out0 = [&](int c, f32x4 g, bool use, Pre4 pre) __attribute__((always_inline)) {
        const int row = c / (TMF / 4), col = mt0 + 4 * (c % (TMF / 4));
        if (u.xfault && b == 0 && c == e0) g[0] += 1.0f;
        if (u.xres) *(f32x4 *)(u.xres + (size_t)(nt0 + row) * ldg + col) = g;
        else step_elem4(u.W32, u.V32, (__bf16 *)u.Wb, (__bf16 *)u.Wt, (__bf16 *)u.Wf, N, ldg, nt0 + row, col, g, u,
                        use, pre);
    };
    auto out12 = [&](long e4, f32x4 g, bool use, Pre4 pre) __attribute__((always_inline)) {
        if (u.xres) {
            *(f32x4 *)(u.xres + (size_t)N * ldg + e4 * 4) = g;
            return;
        }
        int n, k;
        const int l = g12_elem(u, e4, n, k);
        step_elem4(pick(u.W32b, l), pick(u.V32b, l), (__bf16 *)pick(u.Wbb, l), (__bf16 *)pick(u.Wtb, l), nullptr,
                           pick(u.Nb, l), pick(u.Kb, l), n, k, g,
                   u, use, pre);
    };
    const long hoff = (e & 1) ? v.half : 0;
    /* flag barrier `which` of workgroup b with every peer: this workgroup's stores to its buffer
     * acknowledged first (uncached memory: no writeback needed) */
    auto barrier = [&](int which) __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t < v.world && !G0_PROTO(u, 16)) { /* proto & 16: no barrier (one-rank timing ablation only) */
            unsigned int *const sm = pick(v.sig, v.rank), *const sp = pick(v.sig, t);
            unsigned int *const mine = which ? HPNN_XAR_FLAG_B(sm, b, t) : HPNN_XAR_FLAG_A(sm, b, t);
            __hip_atomic_store(which ? HPNN_XAR_FLAG_B(sp, b, v.rank) : HPNN_XAR_FLAG_A(sp, b, v.rank), e,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const unsigned long long t0 = wall_clock64();
            while (__hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < e) {
                __builtin_amdgcn_s_sleep(1);
                if (wall_clock64() - t0 > v.timeout) {
                    __hip_atomic_store(pick(v.sig, v.rank) + HPNN_XAR_ERROR_WORD, 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
            }
        }
        __syncthreads();
        if (G0_PROTO(u, 8)) /* diagnostics: the invalidating system acquire as well */
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    };
    auto g0_off = [&](int c) __attribute__((always_inline)) {
        return (long)(nt0 + c / (TMF / 4)) * ldg + mt0 + 4 * (c % (TMF / 4));
    };
    const bool two = u.xchg == 2 && v.world > 1;
    barrier(0);
    if (two) {
        /* reduce-scatter: element j of each part belongs to rank j % world, which sums it over
         * all ranks (rank order) into its own buffer; a second barrier; every rank then reads
         * each element from its owner -- each link carries 2 / world of the slice, not all */
        for (int c = e0 + t; c < e1; c += NT)
            if ((c - e0) % v.world == v.rank) {
                const long o = hoff + g0_off(c);
                *(f32x4 *)(pick(v.buf, v.rank) + o) = xsum_peers(v, o);
            }
        for (long e4 = c0 + t; e4 < c1; e4 += NT)
            if ((int)((e4 - c0) % v.world) == v.rank) {
                const long o = hoff + (long)N * ldg + e4 * 4;
                *(f32x4 *)(pick(v.buf, v.rank) + o) = xsum_peers(v, o);
            }
        barrier(1);
    }
    /* at most one G0 and one [G1 | G2] element per thread (the MNIST grid: ~107 and ~11 float4
     * per workgroup): both elements' remote loads go out in ONE block and one wait -- over xGMI
     * each wait is a link round trip, so two in series would cost the step a second one */
    if (e1 - e0 <= NT && c1 - c0 <= NT && (two || v.world <= 4) && !G0_PROTO(u, 32)) { /* 32: ablation */
        const bool h0 = e0 + t < e1, h12 = c0 + t < c1;
        const long oa = h0 ? hoff + g0_off(e0 + t) : hoff, ob = h12 ? hoff + (long)N * ldg + (c0 + t) * 4 : hoff;
        f32x4 ga, gb;
        if (two) { /* the owners' sums (owner of element j = t: rank t % world) */
            const float *qa = pick(v.buf, h0 ? t % v.world : v.rank) + oa;
            const float *qb = pick(v.buf, h12 ? t % v.world : v.rank) + ob;
            asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\t"
                         "global_load_dwordx4 %1, %3, off sc0 sc1\n\t"
                         "s_waitcnt vmcnt(0)"
                         : "=&v"(ga), "=&v"(gb)
                         : "v"(qa), "v"(qb)
                         : "memory");
        } else { /* one-shot, world <= 4: rank-order sums of both, 4 slots each (spares local) */
            f32x4 x[8];
            const float *q[8];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                q[p] = pick(v.buf, p < v.world ? p : v.rank) + oa;
                q[4 + p] = pick(v.buf, p < v.world ? p : v.rank) + ob;
            }
            hpnn::ld_sc1_x8<true>(x, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
            ga = x[0];
            gb = x[4];
#pragma unroll
            for (int p = 1; p < 4; p++)
                if (p < v.world) {
                    ga += x[p];
                    gb += x[4 + p];
                }
        }
        if (h0) out0(e0 + t, ga, pf && t < 128, pg0);
        if (h12) out12(c0 + t, gb, pf && t < 16, pg12);
        return;
    }
    /* one-shot: the rank-order sum over every peer; two-shot: the owner's sum */
    auto fetch = [&](long o, long j) __attribute__((always_inline)) -> f32x4 {
        if (!two) return xsum_peers(v, o);
        const float *q = pick(v.buf, (int)(j % v.world)) + o;
        f32x4 x; /* one system-coherent load and its wait in one asm block (see ld_sc1_x8) */
        asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(x) : "v"(q) : "memory");
        return x;
    };
    for (int c = e0 + t; c < e1; c += NT) out0(c, fetch(hoff + g0_off(c), c - e0), pf && c == e0 + t && t < 128, pg0);
    for (long e4 = c0 + t; e4 < c1; e4 += NT)
        out12(e4, fetch(hoff + (long)N * ldg + e4 * 4, e4 - c0), pf && e4 == c0 + t && t < 16, pg12);
}

/* self-test pattern of the in-kernel exchange: rank r, flat gradient index i ->
 * (r + 1) (i % 97 + 1) / 16 -- every partial sum over <= 8 ranks exact in FP32 */
__device__ __forceinline__ f32x4 xtest_pattern(int rank, long i) {
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = (float)((rank + 1) * ((i + r) % 97 + 1)) * 0.0625f;
    return v;
}

/* HPNN_G0_TRACE=1 (profiling only): s_memtime stamps of every workgroup's thread 0 at the
 * phase boundaries, [block][mark]; read back with hpnn_g0_trace */
constexpr int G0TR_BLOCKS = 512, G0TR_MARKS = 8;
__device__ unsigned long long g_g0_trace[G0TR_BLOCKS][G0TR_MARKS];

template <bool WIDE, int WF, int WH, int PD, int KW, bool HU8, bool TRACE = false, int WM = 2, int WN = 2,
          bool X16 = false>
__global__ __launch_bounds__(64 * WM * WN * KW, 3) void g0_fused_kernel(const __bf16 *__restrict__ Dg, int nbd,
                                                            const void *__restrict__ Hg, int nbh, float hscale,
                                                            float *__restrict__ slab, int ldg, int N, int ksteps,
                                                            int splits, int tiles_n, int tiles, int xcd_map,
                                                            hpnn_g0_update u) {
    constexpr int GW = WM * WN, NT = 64 * GW * KW, TMF = 16 * WF * WM, TNH = 16 * WH * WN, NE4 = TMF * TNH / 4,
                  PARTS = NT / 128;
    auto mark = [&](int i) __attribute__((always_inline)) {
        if constexpr (TRACE) {
            const unsigned long long tt = __builtin_amdgcn_s_memtime();
            if (threadIdx.x == 0 && blockIdx.x < G0TR_BLOCKS) g_g0_trace[blockIdx.x][i] = tt;
        }
    };
    mark(0);
    __shared__ f32x4 red[NT];
    f32x4 acc[WF][WH];
    int tile, split, m0, n0;
    const long nb = (long)tiles * splits, nf = u.n12 / 4;
    /* [G1 | G2] float4 columns [0, nt4) belong to the tail workgroups (blocks nb..): all of them
     * when the launch has tails, else the GEMM workgroups take them after their publish */
    const int ntail = (int)gridDim.x - (int)nb;
    const long nt4 = ntail > 0 ? nf : 0;
    /* the exchange's parameters, set by whichever path this workgroup takes */
    bool xdo = false, xpf = false;
    int xb = 0, xe0 = 0, xe1 = 0, xnt0 = 0, xmt0 = 0;
    unsigned int xep = 0;
    long xc0 = 0, xc1 = 0;
    Pre4 xpg0 = {}, xpg12 = {};
    if ((long)blockIdx.x >= nb) {
        const int tb = (int)blockIdx.x - (int)nb;
        const long tc0 = (long)tb * nt4 / ntail, tc1 = (long)(tb + 1) * nt4 / ntail;
        __shared__ unsigned int txe_s;
        float *gout = u.gout && u.gsel && !(*u.gsel & 1) ? u.gout + u.galt : u.gout;
        if (u.xchg) {
            if (threadIdx.x == 0) {
                const unsigned int e = u.xv.ep[blockIdx.x] + 1; /* exchange slot: the block itself */
                u.xv.ep[blockIdx.x] = e;
                txe_s = e;
            }
            __syncthreads();
            gout = pick(u.xv.buf, u.xv.rank) + ((txe_s & 1) ? u.xv.half : 0);
        }
        if (u.xtest) {
            if (u.xchg) {
                for (long e4 = tc0 + threadIdx.x; e4 < tc1; e4 += NT) {
                    const long i = (long)N * ldg + e4 * 4;
                    *(f32x4 *)(gout + i) = xtest_pattern(u.xv.rank, i);
                }
            }
        } else {
            g12_share<NT, 32, 16>(u, tc0, tc1, red, gout ? gout + (size_t)N * ldg : nullptr);
        }
        xdo = u.xchg != 0, xb = (int)blockIdx.x, xep = txe_s, xc0 = tc0, xc1 = tc1;
    } else {
        /* the workgroup's role: virtual block vb (u.perm > 0, tests: reversed and rotated order --
         * every result must stay bitwise the same) */
        const int vb = u.perm > 0 ? (int)((nb - 1 - (long)blockIdx.x + u.perm) % nb) : (int)blockIdx.x;
        if (u.xtest) /* self-test of the in-kernel exchange: no GEMM (the role only) */
            fm_role(vb, splits, tiles, xcd_map, tile, split);
        else
            fm_partial<WIDE, WF, WH, PD, KW, HU8, WM, WN, X16>(Dg, nbd, Hg, nbh, ksteps, splits, tiles_n, tiles,
                                                               xcd_map, vb, acc, tile, split, m0, n0);
        mark(1);
        const int t = threadIdx.x, lane = t & 63;
        /* where the reduced gradient goes instead of a step: the plan's buffer, the xGMI
         * all-reduce's next half (gsel), or -- exchanging here -- this workgroup's epoch's half of
         * this rank's exchange buffer */
        __shared__ unsigned int xe_s;
        float *gout = u.gout && u.gsel && !(*u.gsel & 1) ? u.gout + u.galt : u.gout;
        if (u.xchg) {
            if (t == 0) {
                const unsigned int e = u.xv.ep[vb] + 1; /* only this workgroup touches it */
                u.xv.ep[vb] = e;
                xe_s = e;
            }
            __syncthreads();
            gout = pick(u.xv.buf, u.xv.rank) + ((xe_s & 1) ? u.xv.half : 0);
        }
        /* this split's share of the tile (float4 [e0, e1)) and of [G1 | G2] ([c0, c1)); the first
         * element of each that this thread will step: its W / V loads go out now (HPNN_G0_PROTO
         * bit 64 turns the prefetch off) */
        const int e0 = (int)((long)split * NE4 / splits), e1 = (int)((long)(split + 1) * NE4 / splits);
        const int nt0 = (tile % tiles_n) * TNH, mt0 = (tile / tiles_n) * TMF;
        const long c0 = nt4 + vb * (nf - nt4) / nb, c1 = nt4 + (vb + 1) * (nf - nt4) / nb;
        if (u.xtest) {
            /* the known pattern in place of this workgroup's reduced G0 / [G1 | G2] shares, then the
             * exchange with its sums stored (u.xres) for the host to check */
            if (u.xchg) {
                for (int c = e0 + t; c < e1; c += NT) {
                    const long i = (long)(nt0 + c / (TMF / 4)) * ldg + mt0 + 4 * (c % (TMF / 4));
                    *(f32x4 *)(gout + i) = xtest_pattern(u.xv.rank, i);
                }
                for (long e4 = c0 + t; e4 < c1; e4 += NT) {
                    const long i = (long)N * ldg + e4 * 4;
                    *(f32x4 *)(gout + i) = xtest_pattern(u.xv.rank, i);
                }
                xdo = true, xb = vb, xep = xe_s, xe0 = e0, xe1 = e1, xnt0 = nt0, xmt0 = mt0, xc0 = c0, xc1 = c1;
            }
        } else {
            const bool steps = !u.gout || u.xchg, pf = steps && !G0_PROTO(u, 64);
            Pre4 pg0 = {}, pg12 = {};
            if (pf && t < 128 && e0 + t < e1) {
                const int e = e0 + t, row = e / (TMF / 4), col = mt0 + 4 * (e % (TMF / 4));
                pg0 = pre_load(u.W32, u.V32, (size_t)(nt0 + row) * ldg + col, u.momentum);
            }
            if (pf && t < 16 && c0 + t < c1) {
                int n, k;
                const int l = g12_elem(u, c0 + t, n, k);
                pg12 = pre_load(pick(u.W32b, l), pick(u.V32b, l), (size_t)n * pick(u.Kb, l) + k, u.momentum);
            }
            /* publish this split's partial tile (write-through), then one ticket for the workgroup */
            if ((t >> 6) < GW) {
                const int r16 = lane & 15, q = lane >> 4;
                float *out = slab + (size_t)split * N * ldg;
                if (G0_PROTO(u, 256)) {
                    /* timing ablation: no publish at all (wrong results) */
                } else {
#pragma unroll
                    for (int i = 0; i < WF; i++)
#pragma unroll
                        for (int j = 0; j < WH; j++)
                            st_sc1(out + (size_t)(n0 + j * 16 + r16) * ldg + m0 + i * 16 + 4 * q,
                                   HU8 ? acc[i][j] * hscale : acc[i][j]);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            __shared__ unsigned long long want_s;
            unsigned int *const tcnt = u.cnt + 32 * tile;
            if (t == 0) {
                if (G0_PROTO(u, 1)) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                want_s = hpnn::ticket_arrive(tcnt, (unsigned)splits); /* this launch's last ticket */
            }
            mark(2);
            /* while the other splits finish: this workgroup's share of [G1 | G2] (no dependency on G0) */
            if (!G0_PROTO(u, 512) && c1 > c0) /* 512: timing ablation, no [G1 | G2] share */
                g12_share<NT, 16, 8>(u, c0, c1, red, gout ? gout + (size_t)N * ldg : nullptr, pf && t < 16, pg12);
            mark(3);
            if (t == 0) {
                /* fault hook: this launch reports a timed-out wait (and, like one, reduces what is there) */
                if (u.fault) __hip_atomic_store((gu32 *)u.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else hpnn::ticket_wait(tcnt, want_s, u.err, G0_TIMEOUT);
                if (G0_PROTO(u, 2)) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
            }
            __syncthreads();
            mark(4);
            /* this split's share of the tile: float4 e in [e0, e1), 128 at a time; PARTS threads per
             * float4, each summing a fixed run of splits; the runs meet in LDS in order */
            const int f = t % 128, part = t / 128;
            const int s0 = part * splits / PARTS, s1 = (part + 1) * splits / PARTS;
            const size_t ss = (size_t)N * ldg;
            for (int cc = e0; cc < e1; cc += 128) {
                const int e = cc + f;
                const int row = e / (TMF / 4), col = mt0 + 4 * (e % (TMF / 4));
                f32x4 sum = {0.f, 0.f, 0.f, 0.f};
                if (e < e1 && !G0_PROTO(u, 1024)) { /* 1024: timing ablation, no split loads */
                    const float *p = slab + (size_t)(nt0 + row) * ldg + col;
                    if (G0_PROTO(u, 4))
                        for (int s = s0; s < s1; s += 8) sum += sum_sc1_x8<true>(p + (size_t)s * ss, ss, s1 - s);
                    else
                        for (int s = s0; s < s1; s += 8) sum += sum_sc1_x8(p + (size_t)s * ss, ss, s1 - s);
                }
                red[t] = sum;
                __syncthreads();
                if (part == 0 && e < e1) {
                    f32x4 g = red[f];
#pragma unroll
                    for (int pp = 1; pp < PARTS; pp++) g += red[pp * 128 + f];
                    if (gout)
                        *(f32x4 *)(gout + (size_t)(nt0 + row) * ldg + col) = g;
                    else
                        step_elem4(u.W32, u.V32, (__bf16 *)u.Wb, (__bf16 *)u.Wt, (__bf16 *)u.Wf, N, ldg, nt0 + row, col, g, u,
                                   pf && cc == e0, pg0);
                }
                __syncthreads();
            }
            mark(5);
            xdo = u.xchg != 0, xb = vb, xep = xe_s, xe0 = e0, xe1 = e1, xnt0 = nt0, xmt0 = mt0, xc0 = c0, xc1 = c1;
            xpf = pf, xpg0 = pg0, xpg12 = pg12;
        }  /* not the self-test */
    }  /* GEMM workgroups */
    /* ONE inlined copy of the exchange for every path (several copies made the compiler keep the
     * by-value kernel argument in scratch) */
    if (xdo) g0_exchange_step<NT>(u, xep, N, ldg, xe0, xe1, xnt0, xmt0, TMF, xpf, xpg0, xpg12, xb, xc0, xc1);
    if ((long)blockIdx.x >= nb) mark(6);
}

template <int WF, int WH, int PD, int KW, bool HU8 = false, int WM = 2, int WN = 2>
int launch_fm(const void *Dg, const void *Hg, float hscale, float *slab, int ldg, int N, int M, int Bt, int splits,
              hipStream_t s, const TnTail &tail) {
    constexpr int TMF = 16 * WF * WM, TNH = 16 * WH * WN;
    const int tiles_n = N / TNH, tiles = (M / TMF) * tiles_n;
    const int xcd_map = (splits >= 8 && tiles > 1) ? 1 : 0;
    /* one area per k-group while every workgroup has a CU to itself anyway; a larger grid keeps
     * the small footprint (more workgroups per CU) */
    const bool wide = KW > 1 && tiles * splits + tail.blocks <= g0_cus();
    const size_t lds = fm_meet_bytes<WF, WH, KW, WM, WN>(wide);
#define HPNN_FMK(W_)                                                                                               \
    hipLaunchKernelGGL((gemm_fm_direct_kernel<W_, WF, WH, PD, KW, HU8, WM, WN>), dim3(tiles * splits + tail.blocks), \
                       dim3(64 * WM * WN * KW), lds, s, (const __bf16 *)Dg, N / 16, Hg, M / 16, hscale, slab, ldg, N, \
                       Bt / 32, splits, tiles_n, tiles, xcd_map, tail)
    if constexpr (KW > 1) {
        if (wide) {
            fm_allow_lds<gemm_fm_direct_kernel<true, WF, WH, PD, KW, HU8, WM, WN>>(lds);
            HPNN_FMK(true);
            return hipGetLastError() == hipSuccess ? 0 : -5;
        }
    }
    HPNN_FMK(false);
#undef HPNN_FMK
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

int fm_dispatch(const void *Dg, const void *Hg, int h_u8, float hscale, float *slab, int ldg, int N, int M, int Bt,
                int splits, hipStream_t s, const TnTail &t) {
    if (N <= 0 || M <= 0 || Bt <= 0 || splits <= 0) return -1;
    if (Bt % 32 || splits > Bt / 32 || M % 32 || N % 32) return -2;
    if (ldg % 4 || ldg < M) return -3;
#define HPNN_FM(...)                                                                                              \
    return h_u8 ? launch_fm<__VA_ARGS__, true>(Dg, Hg, hscale, slab, ldg, N, M, Bt, splits, s, t)                  \
                : launch_fm<__VA_ARGS__, false>(Dg, Hg, hscale, slab, ldg, N, M, Bt, splits, s, t)
    /* 80 x 128: four k-interleaved groups of 1 x 2 waves; half the split-K partial bytes of
     * 160 x 128 tiles (profiles/r6/SUMMARY.md) */
    if (M % 80 == 0 && N % 128 == 0) {
        return h_u8 ? launch_fm<5, 4, 1, 4, true, 1, 2>(Dg, Hg, hscale, slab, ldg, N, M, Bt, splits, s, t)
                    : launch_fm<5, 4, 1, 4, false, 1, 2>(Dg, Hg, hscale, slab, ldg, N, M, Bt, splits, s, t);
    }
    if (M % 64 == 0 && N % 64 == 0) { HPNN_FM(2, 2, 2, 1); }
    HPNN_FM(1, 1, 3, 1);
#undef HPNN_FM
}

}  // namespace

/* the fused G0 grid (tiles x splits workgroups of 512 threads) fits on the device at once,
 * with the LDS of the k-groups' meeting (wide: an area per group); both instantiations checked
 * (they differ in the operand conversion) */
static bool g0_fused_resident(int blocks, bool wide = false) {
    constexpr auto k8 = g0_fused_kernel<false, 5, 4, 1, 4, true, false, 1, 2>;
    constexpr auto k16 = g0_fused_kernel<false, 5, 4, 1, 4, false, false, 1, 2>;
    constexpr auto k8w = g0_fused_kernel<true, 5, 4, 1, 4, true, false, 1, 2>;
    constexpr auto k16w = g0_fused_kernel<true, 5, 4, 1, 4, false, false, 1, 2>;
    int dev = 0;
    (void)hipGetDevice(&dev);
    static std::mutex mu;
    static std::map<int, std::pair<int, int>> caps; /* device -> {one area, wide} */
    std::lock_guard<std::mutex> g(mu);
    auto it = caps.find(dev);
    if (it == caps.end()) {
        const size_t l1 = fm_meet_bytes<5, 4, 4, 1, 2>(false), lw = fm_meet_bytes<5, 4, 4, 1, 2>(true);
        fm_allow_lds<k8w>(lw);
        fm_allow_lds<k16w>(lw);
        const int c1 = std::min(hpnn_resident_capacity((const void *)k8, 512, l1),
                                hpnn_resident_capacity((const void *)k16, 512, l1));
        const int cw = std::min(hpnn_resident_capacity((const void *)k8w, 512, lw),
                                hpnn_resident_capacity((const void *)k16w, 512, lw));
        it = caps.emplace(dev, std::make_pair(c1, cw)).first;
    }
    return blocks <= (wide ? it->second.second : it->second.first);
}

static bool g0_fused_on() {
    static const bool on = [] { const char *e = getenv("HPNN_G0_FUSED"); return !(e && e[0] == '0'); }();
    return on;
}

/* the fused launch's output tiles: 80 feature columns x 128, as fm_dispatch's first choice */
extern "C" int hpnn_g0_tiles(int N, int M) { return (M % 80 || N % 128) ? 0 : (M / 80) * (N / 128); }

extern "C" int hpnn_gemm_fm_direct_update(const void *Dg, const void *Hg, int h_u8, float hscale, float *slab,
                                          int ldg, int N, int M, int Bt, int splits, const hpnn_g0_update *u,
                                          hipStream_t stream) {
    const int tiles = hpnn_g0_tiles(N, M), tiles_n = N / 128;
    if (!g0_fused_on() || !u || !tiles || Bt % 32 || splits < 1 || splits > Bt / 32 || ldg != M) return -1;
    if (!u->cnt || !u->err) return -1;
    const bool steps = !u->gout || u->xchg;
    if (u->n12 % 4 || !u->mslab || u->mrows < 1 || (steps && u->momentum && (!u->V32 || !u->V32b[0] || !u->V32b[1])))
        return -2;
    if (tiles > HPNN_G0_MAX_TILES) return -1; /* 64-bit counters 32 words apart, below the error word */
    /* every workgroup waits for the other splits of its tile: all must be resident at once
     * (more splits than that, e.g. forced by HPNN_TN_SPLITS, take the slab form instead of
     * stalling to the timeout) */
    if (!g0_fused_resident(tiles * splits)) return -1;
    /* an LDS area per k-group (one barrier instead of a round per group) wherever the grid is
     * resident with that footprint too -- one workgroup per CU.  Not with the exchange in the
     * launch: ranks that share one GPU must fit their waiting grids side by side */
    const bool wide = !u->xchg && g0_fused_resident(tiles * splits, true);
    /* tail workgroups for the [G1 | G2] share on the CUs the GEMM grid leaves idle (MNIST: 240
     * GEMM workgroups, 16 tails on a 256-CU MI355X); HPNN_G0_TAILS overrides the count (0: none,
     * the GEMM workgroups sum [G1 | G2] after their publish -- the form for a device with no
     * idle CU) */
    const int cus = g0_cus();
    static const int tails_env = [] { const char *e = getenv("HPNN_G0_TAILS"); return e ? atoi(e) : -1; }();
    /* one tail per 16 slab rows (each sums ~16 x the [G1 | G2] block, 563 KB on MNIST), at most
     * the CUs the GEMM grid leaves idle: ranks sharing one GPU (tests, rehearsals) keep their
     * grids small enough to co-run */
    int ntail = tails_env >= 0 ? tails_env : std::min(cus - tiles * splits, std::max(1, u->mrows / 16));
    if (ntail < 0) ntail = 0;
    if (ntail > 64) ntail = 64;
    while (ntail > 0 && !g0_fused_resident(tiles * splits + ntail, wide)) ntail--;
    if (u->xchg && tiles * splits + ntail > HPNN_XAR_MAX_BLOCKS) ntail = HPNN_XAR_MAX_BLOCKS - tiles * splits;
    if (ntail < 0) ntail = 0;
    if (u->xchg) {
        /* the exchange buffer holds [G0 | G1 | G2]; one epoch / flag slot per workgroup */
        if (tiles * splits + ntail > HPNN_XAR_MAX_BLOCKS || u->xv.world < 1 || u->xv.world > HPNN_XAR_MAX_RANKS ||
            !u->xv.ep || (long)N * ldg + u->n12 > u->xv.half)
            return -1;
        for (int p = 0; p < u->xv.world; p++)
            if (!u->xv.buf[p] || !u->xv.sig[p]) return -1;
    }
    const int xcd_map = (splits >= 8 && tiles > 1) ? 1 : 0;
    hpnn_g0_update uu = *u;
    const size_t lds = fm_meet_bytes<5, 4, 4, 1, 2>(wide);
#ifdef HPNN_ABLATIONS
    static const int proto = [] { const char *e = getenv("HPNN_G0_PROTO"); return e ? atoi(e) : 0; }();
    uu.proto |= proto;
#endif
    static const bool trace = [] { const char *e = getenv("HPNN_G0_TRACE"); return e && e[0] == '1'; }();
#define HPNN_G0F(...)                                                                                              \
    do {                                                                                                           \
        if (wide) {                                                                                                \
            fm_allow_lds<g0_fused_kernel<true, __VA_ARGS__>>(lds);                                                 \
            HPNN_G0L(true, __VA_ARGS__);                                                                           \
        } else {                                                                                                   \
            HPNN_G0L(false, __VA_ARGS__);                                                                          \
        }                                                                                                          \
    } while (0)
#define HPNN_G0L(...)                                                                                              \
    hipLaunchKernelGGL((g0_fused_kernel<__VA_ARGS__>), dim3(tiles * splits + ntail), dim3(512), lds, stream,         \
                       (const __bf16 *)Dg, N / 16, Hg, M / 16, hscale, slab, ldg, N, Bt / 32, splits, tiles_n,     \
                       tiles, xcd_map, uu)
    /* HPNN_G0_PD=2 (ABLATIONS builds, tuning): two k-steps of operands in flight */
#ifdef HPNN_ABLATIONS
    static const int pd = [] { const char *e = getenv("HPNN_G0_PD"); return e ? atoi(e) : 1; }();
    static const bool x16 = [] { const char *e = getenv("HPNN_G0_X16"); return e && e[0] == '1'; }();
    if (h_u8 && pd == 2) HPNN_G0F(5, 4, 2, 4, true, false, 1, 2);
    else if (h_u8 && x16) HPNN_G0F(5, 4, 1, 4, true, false, 1, 2, true);
    else
#endif
    if (h_u8 && trace) HPNN_G0F(5, 4, 1, 4, true, true, 1, 2);
    else if (h_u8) HPNN_G0F(5, 4, 1, 4, true, false, 1, 2);
    else HPNN_G0F(5, 4, 1, 4, false, false, 1, 2);
#undef HPNN_G0F
#undef HPNN_G0L
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int hpnn_gemm_fm_direct_update_ok(int ldg, int N, int M, int Bt, int splits) {
    const int tiles = hpnn_g0_tiles(N, M);
    if (!(g0_fused_on() && tiles > 0 && Bt % 32 == 0 && splits >= 1 && splits <= Bt / 32 && ldg == M &&
          tiles <= HPNN_G0_MAX_TILES))
        return 0;
    return g0_fused_resident(tiles * splits) ? 1 : 0;
}

extern "C" int hpnn_gemm_fm_direct(const void *Dg, const void *Hg, int h_u8, float hscale, float *slab, int ldg, int N,
                                   int M, int Bt, int splits, hipStream_t stream) {
    const TnTail none = {nullptr, nullptr, 0, 0, 0, 0, 1, 1, 0};
    return fm_dispatch(Dg, Hg, h_u8, hscale, slab, ldg, N, M, Bt, splits, stream, none);
}

extern "C" int hpnn_gemm_fm_direct_reduce(const void *Dg, const void *Hg, int h_u8, float hscale, float *slab,
                                          int ldg, int N, int M, int Bt, int splits, const float *rslab, int rS,
                                          long rstride, long rn, int rgroups, float *rout, hipStream_t stream) {
    if (rn % 4 || rstride % 4 || rS < 1 || rgroups < 1 || rgroups > rS || !rslab || !rout) return -2;
    const long n4 = rn / 4;
    const int bx = (int)((n4 + 255) / 256);
    const TnTail t = {rslab, rout, rstride, n4, rn, rS, (rS + rgroups - 1) / rgroups, bx, bx * rgroups};
    return fm_dispatch(Dg, Hg, h_u8, hscale, slab, ldg, N, M, Bt, splits, stream, t);
}

/* HPNN_G0_TRACE=1 stamps: out[512][8] shader-clock ticks (thread 0 of each workgroup) */
extern "C" int hpnn_g0_trace(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_g0_trace), sizeof(g_g0_trace)) == hipSuccess ? 0 : -5;
}
