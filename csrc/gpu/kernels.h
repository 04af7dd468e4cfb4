/*
 * libhpnn HIP kernel launchers (gfx950).  Plain C ABI: device pointers +
 * hipStream_t, so the native engines and the Python binding share them.
 *
 * Layout conventions (see docs/DESIGN.md):
 *   activations  [rows = samples][cols = features], row-major, BF16
 *   weights      W [N][K] row-major (one row per neuron, as the reference),
 *                plus a transposed BF16 copy Wt [K][N] for the dX GEMM
 *   every feature dimension is padded to a multiple of 32 and every batch
 *   dimension to a multiple of 128 on the device; padded weights/inputs are
 *   zero so they never contribute.
 * Return value of every launcher: 0 = launched, <0 = shape not supported
 * (caller bug: the kernels never guess).
 */
#ifndef HPNN_GPU_KERNELS_H
#define HPNN_GPU_KERNELS_H
#include <hip/hip_runtime_api.h>
#include <libhpnn/cg.h>
#include <libhpnn/adam.h>
#include <libhpnn/lrsched.h>
#include <libhpnn/clip.h>
#include <libhpnn/xar.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Loss / accuracy statistics are accumulated into HPNN_STAT_SLOTS slots spaced
 * HPNN_STAT_STRIDE floats apart (one 64-byte line each) -- block b adds into slot
 * b % HPNN_STAT_SLOTS -- so thousands of workgroups never serialise on a single
 * atomic address.  `loss_acc` / `correct` arguments point at slot 0; readers sum
 * the slots. */
#define HPNN_STAT_SLOTS 64
#define HPNN_STAT_STRIDE 16
#define HPNN_STAT_SLOT(b) ((size_t)((b) % HPNN_STAT_SLOTS) * HPNN_STAT_STRIDE)

enum {
    HPNN_EPI_NONE = 0,   /* C = acc                                   */
    HPNN_EPI_ACT = 1,    /* C = 2/(1+e^-acc) - 1                      */
    HPNN_EPI_DACT = 2,   /* C = acc * (-0.5)(aux^2 - 1)  (f'(h))      */
};

/* C[M x N] = epi(A[M x K] . B[N x K]^T), A/B BF16, C BF16 (c_f32=0) or
 * FP32 (c_f32=1).  M % 128 == 0, N % 32 == 0, K % 32 == 0. */
int hpnn_gemm_nt_bf16(const void *A, int lda, const void *B, int ldb, void *C, int ldc,
                      const void *aux, int ldaux, int M, int N, int K, int epi, int c_f32,
                      hipStream_t stream);

/* weight-stationary variant for N <= 128, K in {512, 800, 1024}: returns 1 if no instance */
/* the same product on the 8-phase 256x256-tile kernel (kernels_8ph.hip): M % 256 == 0,
 * N % 256 == 0, K % 128 == 0, else -1.  hpnn_gemm_nt_bf16 routes large GEMMs here when
 * HPNN_NT_8PH is not 0. */
/* split-K form of the same (S FP32 slabs in a library workspace, then one epilogue pass):
 * M % 256 == 0, N % 256 == 0, K % (128 S) == 0; -1 when it does not apply */
int hpnn_gemm_nt8_splitk_bf16(const void *A, int lda, const void *B, int ldb, void *C, int ldc, const void *aux,
                              int ldaux, int M, int N, int K, int epi, int c_f32, int splits, hipStream_t stream);
/* weight gradient of one layer over the whole batch with the optimizer step fused into the
 * 8-phase TN kernel's epilogue (no gradient in memory): the step of hpnn_sgd_update with one
 * slab.  N % 256 == 0, M % 256 == 0, Bt % 128 == 0, else -1. */
/* G = D^T H (one split) rounded to BF16 into G16 [N][ldg] (8-phase kernel); -1: shape not covered */
int hpnn_gemm_tn8_bf16out_ok(int N, int M, int Bt, int ldd, int ldh);
int hpnn_gemm_tn8_bf16out(const void *D, int ldd, const void *H, int ldh, void *G16, int ldg, int N, int M, int Bt,
                          hipStream_t stream);
int hpnn_gemm_tn8_update(const void *D, int ldd, const void *H, int ldh, int N, int M, int Bt, float *W32, float *V32,
                         void *Wbf, void *Wt, float lr, float alpha, float scale, int momentum, hipStream_t stream);
/* the same with the gradient over `splits` (>= 2) split-K slabs reduced inside the launch (each
 * split publishes its partial write-through; the splits of a tile meet through tickets in
 * cnt, 1024 words zeroed once; err set on a timeout): -1 when not covered */
int hpnn_gemm_tn8_fused_update(const void *D, int ldd, const void *H, int ldh, int N, int M, int Bt, int splits,
                               float *slab, float *W32, float *V32, void *Wbf, void *Wt, float lr, float alpha,
                               float scale, int momentum, unsigned int *cnt, unsigned int *err, hipStream_t stream);
/* the next layer's weight gradient D^T H (N x M over the same Bt rows, S splits of 64 x 64
 * pieces into slab [S][N][M], the pieces of gemm_tn_pipe at 64 x 64) and its step (same lr /
 * alpha / scale / momentum), carried by the fused launch above (kernels_8ph.hip): bitwise the
 * result of hpnn_gemm_tn_bf16 + hpnn_sgd_update.  cnt: a 64-bit counter zeroed once, used by
 * this launch shape only. */
typedef struct {
    const void *D, *H;
    int ldd, ldh;
    float *slab;
    int N, M, S;
    float *W32, *V32;
    void *Wb, *Wt;
    unsigned int *cnt;
} hpnn_tn8_side;
/* hpnn_gemm_tn8_fused_update plus that side job: -1 as above, -2 when the side job does not
 * fit this grid (its pieces must split evenly over the half-workgroups) */
int hpnn_gemm_tn8_fused_update_side(const void *D, int ldd, const void *H, int ldh, int N, int M, int Bt, int splits,
                                    float *slab, float *W32, float *V32, void *Wbf, void *Wt, float lr, float alpha,
                                    float scale, int momentum, unsigned int *cnt, unsigned int *err,
                                    const hpnn_tn8_side *side, hipStream_t stream);
void hpnn_gemm_nt_set_8ph(int on);
void hpnn_gemm_tn_set_8ph(int on); /* same switch for the large weight-gradient GEMMs */
void hpnn_gemm_nt_set_pp(int on);  /* the pipelined 128 x 128 NT kernel for under-filled grids */
/* C[M x N] = epi(A[M x K] . W[K x N]), W row-major [K][N]: the NT product on W^T without the
 * transposed copy (same bits); M, N % 128, K % 64, else -1.  _ok: 1 when the shape fits */
int hpnn_gemm_nn_ok(int M, int N, int K, int lda, int ldw, int ldc);
int hpnn_gemm_nn_bf16(const void *A, int lda, const void *W, int ldw, void *C, int ldc, const void *aux, int ldaux,
                      int M, int N, int K, int epi, int c_f32, hipStream_t stream);
int hpnn_gemm_nt8_bf16(const void *A, int lda, const void *B, int ldb, void *C, int ldc, const void *aux, int ldaux,
                       int M, int N, int K, int epi, int c_f32, hipStream_t stream);
int hpnn_gemm_nt_ws_bf16(const void *X, int ldx, const void *W, int ldw, void *C, int ldc, int M, int N, int K,
                         int epi, int c_f32, hipStream_t stream);
/* host only: the ring depth of the weight-stationary instance for this call, 0 where
 * hpnn_gemm_nt_ws_bf16 returns 1 (no instance) */
int hpnn_gemm_nt_ws_plan(int M, int N, int K, int ldx, int ldw, int ldc, int epi);
/* host only: which kernel hpnn_gemm_nt_bf16 / hpnn_gemm_tn_bf16 (and _reduce) run for these
 * arguments under the current toggles: the arm (index of hpnn_gemm_*_arm_name) and, in *stages,
 * the ring depth of its instantiation (0: the 8-phase schedule), or the refusal code (< 0) */
int hpnn_gemm_nt_plan(int M, int N, int K, int lda, int ldb, int ldc, int epi, int has_aux, int ldaux, int *stages);
int hpnn_gemm_tn_plan(int N, int M, int Bt, int splits, int ldd, int ldh, int ldg, int *stages);
const char *hpnn_gemm_nt_arm_name(int i); /* NULL past the last arm */
const char *hpnn_gemm_tn_arm_name(int i);

/* slab[s][N x M] = sum_{b in slice s} D[b][n] H[b][m] (FP32 out).
 * D: [Bt x N] BF16, H: [Bt x M] BF16. Bt % 64 == 0, 1 <= splits <= Bt/64, N,M % 32 == 0.
 * Slice s = rows [64*floor(s*U/S), 64*floor((s+1)*U/S)), U = Bt/64 (uneven splits allowed).
 * ldg: row stride of a slab row (>= M); slab stride = N*ldg. */
int hpnn_gemm_tn_bf16(const void *D, int ldd, const void *H, int ldh, float *slab, int ldg, int N,
                      int M, int Bt, int splits, hipStream_t stream);
/* the same GEMM plus, in the same launch, hpnn_reduce_groups(rslab, rS, rstride, rn, rgroups,
 * rout) run by extra workgroups appended to the grid (they fill the CUs the GEMM tiles
 * leave idle; one launch less per fused training step) */
int hpnn_gemm_tn_bf16_reduce(const void *D, int ldd, const void *H, int ldh, float *slab, int ldg, int N, int M,
                             int Bt, int splits, const float *rslab, int rS, long rstride, long rn, int rgroups,
                             float *rout, hipStream_t stream);

/* weight gradient of hpnn_gemm_tn_bf16 over FRAGMENT-MAJOR operands (kernels_g0.hip):
 * Dg [Bt/32][N/16][64][8], Hg [Bt/32][M/16][64][8], lane l = 16 g + r of fragment (t, cb)
 * holding A[32 t + 8 g + j][16 cb + r] (j < 8); slab[s][n][m] as hpnn_gemm_tn_bf16.
 * Bt, M, N multiples of 32.  h_u8: Hg holds unsigned bytes in the same layout, used as
 * bf16(h * hscale) (pixel data).  _reduce: plus hpnn_reduce_groups on appended workgroups. */
int hpnn_gemm_fm_direct(const void *Dg, const void *Hg, int h_u8, float hscale, float *slab, int ldg, int N, int M,
                        int Bt, int splits, hipStream_t stream);
int hpnn_gemm_fm_direct_reduce(const void *Dg, const void *Hg, int h_u8, float hscale, float *slab, int ldg, int N,
                               int M, int Bt, int splits, const float *rslab, int rS, long rstride, long rn,
                               int rgroups, float *rout, hipStream_t stream);

/* the same GEMM with its split-K reduction and the optimizer step of layer 0 in the same
 * launch, plus the [G1 | G2] block-slab reduction and the steps of layers 1, 2 on tail
 * workgroups (the single-GPU fused MNIST step; kernels_g0.hip).  slab: scratch for the
 * published partials.  Returns -1 when the shape is not covered (caller: the 3-launch form),
 * HPNN_G0_FUSED=0 disables it. */
typedef struct {
    float *W32, *V32; /* layer 0 [N][M] FP32 master / momentum (V32 NULL for BP) */
    void *Wb, *Wt, *Wf; /* BF16 W [N][M], W^T [M][N], fragment-major copy (each may be NULL: not kept) */
    unsigned int *cnt;  /* HPNN_G0CNT_WORDS words, zeroed once: 64-bit tile counters, 32 words apart (monotonic) */
    unsigned int *err;  /* set when a wait for the other splits timed out */
    float lr, alpha, scale;
    int momentum;
    const float *mslab; /* [G1 | G2] block slabs: mrows rows of n12 floats, mstride apart */
    int mrows;
    long mstride, n12;
    float *W32b[2], *V32b[2]; /* layers 1, 2 */
    void *Wbb[2], *Wtb[2]; /* (each may be NULL: that copy is not kept) */
    int Nb[2], Kb[2];
    /* non-NULL: no step -- the fully reduced gradients are stored instead, G0 [N][M] at gout,
     * [G1 | G2] right after it (the flat layout of the plan's gradient buffer; data parallel) */
    float *gout;
    /* non-NULL (with gout): gout + galt instead of gout when *gsel is even -- gout is then the
     * xGMI all-reduce's own data buffer and *gsel its epoch word, so the gradient lands in the
     * half the next call reads (hpnn_xar_local) and that call needs no copy-in */
    const unsigned int *gsel;
    long galt;
    /* xchg != 0: data parallel with the exchange in this launch -- each workgroup writes its
     * reduced G0 / [G1 | G2] elements into its half of xv's buffer, runs the one-shot flag
     * barrier of workgroup b with every peer (include/libhpnn/xar.h hpnn_xar_view), sums the
     * peers' copies in rank order and steps those elements (scale includes 1 / world) */
    int xchg; /* 1 one-shot, 2 two-shot (each rank reduces 1 / world of every slice, then gathers) */
    hpnn_xar_view xv;
    int proto; /* hand-off diagnostics (HPNN_G0_PROTO, make ABLATIONS=1 builds only): 1 producer agent
                * release, 2 consumer agent acquire, 4 system-scope (sc0 sc1) partial loads, 8 system
                * acquire after the exchange barrier, 16 no exchange barrier, 32 one exchange load
                * block per element (not one for both), 64 no W / V prefetch; timing ablations (wrong
                * results): 256 no partial publish, 512 no [G1 | G2] share, 1024 no split-sum loads */
    /* tests / diagnostics: perm > 0 runs the grid in another block -> role order (reversed,
     * rotated by perm: results must not change); xtest: self-test of the in-kernel exchange
     * (no GEMM: a known pattern is exchanged, the sums land in xres, [G0 | G1 | G2] flat);
     * xfault: corrupt one element of this rank's exchanged sum (HPNN_FAULT=xsum:n) */
    int perm, xtest, xfault;
    float *xres;
    int fault; /* test hook (HPNN_FAULT=handoff:n): the split-K wait of that launch reports a
                * timeout (sets *err) as a real one would */
} hpnn_g0_update;
int hpnn_gemm_fm_direct_update(const void *Dg, const void *Hg, int h_u8, float hscale, float *slab, int ldg, int N,
                               int M, int Bt, int splits, const hpnn_g0_update *u, hipStream_t stream);
/* 1 when hpnn_gemm_fm_direct_update covers the shape (launch-free check), including the
 * residency its in-kernel hand-offs need: every workgroup of the grid co-resident */
int hpnn_gemm_fm_direct_update_ok(int ldg, int N, int M, int Bt, int splits);
/* output tiles (80 feature columns x 128) of the fused G0 launch for an N x M gradient, 0 if
 * not covered; the launch's grid is tiles x splits GEMM workgroups plus its tail workgroups */
int hpnn_g0_tiles(int N, int M);
/* hpnn_g0_update.cnt: HPNN_G0CNT_WORDS words, 64-bit tile counters 32 words apart (tile <
 * HPNN_G0_MAX_TILES), the error word at HPNN_G0_ERR_WORD */
#define HPNN_G0CNT_WORDS 1024
#define HPNN_G0_MAX_TILES 31
#define HPNN_G0_ERR_WORD 1000
/* workgroups of `kernel` (threads per workgroup, dynamic LDS bytes) the device can hold at once:
 * the occupancy API's blocks per CU x CUs (cached per kernel).  Kernels whose workgroups wait
 * for each other inside one launch (split-K tickets, tile-pair hand-offs, the in-kernel DP
 * exchange) refuse grids above it: the first wave of workgroups would spin on partners that
 * cannot be scheduled until the wait times out. */
int hpnn_resident_capacity(const void *kernel, int threads, size_t dyn_lds);
/* (Best effort: the count assumes the launch has the device to itself.  Kernels of another
 * stream or process on the same GPU -- a side-stream collective, ranks sharing one GPU in
 * tests / rehearsals -- can hold CUs meanwhile; a waiting grid then stretches until they
 * finish, and a wait that outlives its bound sets the error word read by BPlan::health.) */
/* *out += order-independent 64-bit digest of the nbytes / 4 words at p (word index offset by
 * base, so several buffers can be folded into one digest); *out must be initialised */
int hpnn_hash_words(const void *p, long nbytes, long base, unsigned long long *out, hipStream_t stream);
/* load every kernel translation unit's code object onto the current device now (HIP loads a
 * code object at its first launch): training loops call it before their clock starts, so a
 * first eager step does not pay for it.  Once per device; 0 on success. */
int hpnn_preload_code_objects(void);

/* ---- per-epoch reshuffle of the resident training set (kernels_shuffle.hip) ----
 * perm[i] = src(i) of <libhpnn/shuffle.h> for (n, seed, *epoch_word); a walk that passes
 * HPNN_SHUFFLE_MAX_WALK iterations sets *err (never with a correct build) */
int hpnn_epoch_perm_dev(int *perm, int n, unsigned int seed, const unsigned int *epoch_word, unsigned int *err,
                        hipStream_t stream);
/* *epoch_word += 1 in a one-thread launch: ordered behind the launches that read the word, so
 * a replayed graph of several epochs sees e, e + 1, .. with no host involvement */
int hpnn_epoch_advance(unsigned int *epoch_word, hipStream_t stream);
/* row-major: dst row i = src row perm[i] (i < n), zero rows n .. rows_p - 1; row_bytes % 4 == 0
 * (16-byte accesses when rows and pointers allow); an index outside [0, n) gives a zero row */
int hpnn_gather_rows(void *dst, const void *src, const int *perm, int n, long rows_p, long row_bytes,
                     hipStream_t stream);
/* row-major src [n][Kp] (elem_bytes 1 or 2) -> fragment-major dst [rows_p/32][Kp/16][64][8]
 * (lane 16 g + r of fragment (t, cb) holds A[32 t + 8 g + j][16 cb + r]) of the permuted rows,
 * zero rows from n up; rows_p % 32 == 0, Kp % 16 == 0, 16-byte aligned pointers */
int hpnn_gather_fm(void *dst, const void *src_rowmajor, const int *perm, int n, long rows_p, int Kp, int elem_bytes,
                   hipStream_t stream);

/* output layer: logits Z [B x ldz] FP32 (n_out valid columns) ->
 *   delta  D [B x ldd] BF16  (zero in padded rows/cols)
 *   loss_acc[slot] += sum of per-sample loss over valid rows (slot array, above)
 *   correct[slot]  += argmax hits
 *   optional O [B x ldo] FP32 network output (NULL to skip)
 * targets: dense T [B x ldt] FP32 (labels == NULL) or int32 labels with
 * one-hot values (t_hi at the label, t_lo elsewhere).
 * type: 0 ANN, 1 LNN, 2 SNN (nn_type). */
int hpnn_output_delta(const float *Z, int ldz, const float *T, int ldt, const int *labels, float t_hi,
                      float t_lo, void *D, int ldd, float *O, int ldo, float *loss_acc,
                      unsigned int *correct, int B, int n_valid, int n_out, int type,
                      hipStream_t stream);

/* sum S slabs of n floats: out[i] = sum_s slab[s*stride + i] */
int hpnn_reduce_slabs(const float *slab, int S, long stride, long n, float *out, hipStream_t stream);

/* optimizer step for one layer, W32/V32 FP32 master [N x K]:
 *   g = scale * sum_s G[s*gstride + i]
 *   BP : w += lr g              (momentum == 0)
 *   BPM: v += lr g; w += v; v *= alpha
 * then writes BF16 W [N x K] and BF16 Wt [K x N] (ldwt = N). */
int hpnn_sgd_update(float *W32, float *V32, const float *G, int S, long gstride, void *Wbf, void *Wt,
                    int N, int K, float lr, float alpha, float scale, int momentum,
                    hipStream_t stream);

/* all layers' optimizer steps in ONE launch (same math as hpnn_sgd_update per layer).
 * Wf (optional, may be NULL): BF16 copy of W in MFMA-fragment-major order, the operand
 * layout of the register-resident first-layer weights (hpnn_mlp3_fused):
 *   element (n, k) at (((n/16)*(K/32) + k/32)*64 + n%16 + 16*((k/8)%4))*8 + k%8 */
#define HPNN_UPD_MAX 8
typedef struct {
    float *W32;
    float *V32;
    const float *G;
    long gstride;
    void *Wbf;
    void *Wt;
    void *Wf;
    int S, N, K;
} hpnn_upd_layer;
int hpnn_sgd_update_multi(const hpnn_upd_layer *layers, int n, float lr, float alpha, float scale, int momentum,
                          hipStream_t stream);

/* dense FP64/FP32 host-layout matrix -> padded BF16 device matrix:
 * dst[r][c] = src[r][c] for r<rows,c<cols, 0 in the padding.
 * src_f64 selects double vs float input. */
int hpnn_pack_bf16(const void *src, int src_f64, int rows, int cols, int lds, void *dst, int prow,
                   int pcol, int ldd, hipStream_t stream);

/* FP32 master <-> BF16 copies without an update (after load/broadcast) */
int hpnn_cast_weights(const float *W32, void *Wbf, void *Wt, int N, int K, hipStream_t stream);

/* BF16 reduce-scatter data parallelism (csrc/dist/dp_exchange.cpp): dst = bf16(src), n % 4 == 0;
 * the step of n consecutive master elements from a BF16 gradient sum (W32, V32, Wbf rows);
 * Wt [K][N] = Wbf^T */
int hpnn_cast_f32_bf16(const float *src, void *dst, long n, hipStream_t stream);
int hpnn_sgd_update_rows_bf16g(float *W32, float *V32, const void *G16, long n, float lr, float alpha, float scale,
                               int momentum, void *Wbf, hipStream_t stream);
int hpnn_transpose_bf16(const void *Wbf, void *Wt, int N, int K, hipStream_t stream);

/* BF16 row-sharded tensor parallelism (tp_engine.cpp): dst [rows][P n] <- src [P][rows][n]
 * (n % 8 == 0); out = bf16(in * f'(H)) elementwise (n % 4 == 0) */
int hpnn_block_permute_bf16(const void *src, void *dst, int P, long rows, int n, hipStream_t stream);
int hpnn_dact_f32_bf16(void *out, const float *in, const void *H, long n, hipStream_t stream);

/* zero-fill helper usable inside graphs */
int hpnn_fill_f32(float *p, long n, float v, hipStream_t stream);

/* fused middle of a 3-layer MLP (kernels_mlp3.hip): H1 [Bp x 128] -> delta1
 * [Bp x 128] + per-block [G1 (64 x 128) | G2 (32 x 64)] FP32 slabs (grid of them),
 * loss / accuracy.  Dims must be h1=128, h2=64, no=32 (padded), n_out <= 32,
 * Bp % 64 == 0.  W1t / W2t are unused (transposed LDS reads of W1 / W2). */
int hpnn_mlp3_mid(const void *H1g, const void *W1, const void *W1t, const void *W2, const void *W2t,
                  const int *labels, const float *T, int ldt, float t_hi, float t_lo, void *D1, float *gslab,
                  float *loss_acc, unsigned int *correct, int Bp, int n_valid, int n_out, int type, int h1, int h2,
                  int no, int grid, hipStream_t stream);
/* the whole 3-layer step up to delta1 in one persistent kernel (kernels_mlp3.hip):
 *   X [Bp x K0] -> H1 = f(X W0^T) -> H2 -> output/loss -> delta3 -> delta2 -> delta1 (D1)
 * plus per-block [G1 | G2] slabs (grid of them, same layout as hpnn_mlp3_mid).  W0 is
 * read once per workgroup into registers from its fragment-major copy W0f (see
 * hpnn_sgd_update_multi); K0 in {256, 512, 800, 832, 896}, Bp % 32 == 0.  grid <= 0:
 * one workgroup per CU.  d1fm: delta1 written fragment-major ([Bp/32][8][64][8], the
 * operand layout of hpnn_gemm_fm_direct) instead of row-major [Bp x 128].  Returns the
 * grid used (> 0) or an error (< 0). */
int hpnn_mlp3_fused(const void *X, int ldx, int K0, const void *W0f, const void *W1, const void *W2,
                    const int *labels, const float *T, int ldt, float t_hi, float t_lo, void *D1, float *gslab,
                    float *loss_acc, unsigned int *correct, int Bp, int n_valid, int n_out, int type, int grid,
                    int d1fm, hipStream_t stream);
/* grid hpnn_mlp3_fused will use for Bp samples (slab rows to allocate) */
int hpnn_mlp3_fused_grid(int Bp, int grid);
/* the same step up to delta1 with 256-sample tiles (kernels_mlp3t.hip): X given
 * FRAGMENT-MAJOR ([Bp/32][K0/16][64][8], ops.to_fragment_major), 8-bit (xu8: used as
 * bf16(byte * xscale)) or BF16; W0f fragment-major BF16 W0, W1 [64][128], W2 [32][64] and
 * W2t [64][32] BF16; delta1 written fragment-major ([Bp/32][8][64][8]); per-block
 * [G1 | G2] slabs as hpnn_mlp3_mid.  Bp % 256 == 0, K0 in {256, 800}.  grid <= 0: one
 * workgroup per CU (capped at Bp / 256).  Returns the grid used (> 0) or an error (< 0). */
int hpnn_mlp3_tile(const void *Xg, int xu8, float xscale, int K0, const void *W0f, const void *W1, const void *W2,
                   const void *W2t, const int *labels, const float *T, int ldt, float t_hi, float t_lo, void *D1,
                   float *gslab, float *loss_acc, unsigned int *correct, int Bp, int n_valid, int n_out, int type,
                   int grid, hipStream_t stream);
int hpnn_mlp3_tile_grid(int Bp, int grid);
/* forward-only form of hpnn_mlp3_tile (validation): the same input, W0f / W1 / W2, rounding
 * points and summation order, so a batch's loss and hits are the numbers the training front
 * reports for it; added into the caller's stat slots (HPNN_STAT_SLOTS layout).  guess (may be
 * NULL) [Bp] int32: the lowest index of the largest logit, -1 for rows >= n_valid.  No delta,
 * no slab, no W2t.  Same shapes, alignment checks and return values as hpnn_mlp3_tile. */
int hpnn_mlp3_eval(const void *Xg, int xu8, float xscale, int K0, const void *W0f, const void *W1, const void *W2,
                   const int *labels, const float *T, int ldt, float t_hi, float t_lo, float *loss_acc,
                   unsigned int *correct, int *guess, int Bp, int n_valid, int n_out, int type, int grid,
                   hipStream_t stream);
/* commit one validation pass (kernels_validate.hip), one workgroup, capturable: the 64 stat
 * slots summed in slot order (float loss at [0] plus the double at floats 2..3 the FP engines'
 * hpnn_output_fp_eval adds into) -> hist[*cursor] = {double loss_sum, uint hits}, the slots zeroed,
 * *cursor += 1; a full history (cursor == cap) drops the record and only zeroes the slots */
typedef struct {
    double loss_sum;
    unsigned int hits, pad;
} hpnn_val_record;
/* guess[r] = lowest index of the largest of Z[r][0 .. n_out) for r < n_valid, -1 for the rows up
 * to `rows` (the per-layer evaluation path's guess) */
int hpnn_argmax_rows(const float *Z, int ldz, int n_out, int rows, int n_valid, int *guess, hipStream_t stream);
int hpnn_validate_commit(float *slots, hpnn_val_record *hist, unsigned int *cursor, unsigned int cap,
                         hipStream_t stream);
/* ---- keep the best validation pass (kernels_best.hip; [keep_best], [patience]) ----
 * best_commit: one thread, capturable, behind hpnn_validate_commit on the same stream: judges
 * hist[*cursor - 1] against the best record so far (metric HPNN_BEST_LOSS: a smaller loss sum;
 * HPNN_BEST_ACC: more hits, the loss breaking ties; nothing is best before the first pass, a
 * NaN loss is never taken under LOSS, ties do not improve) and sets state->take for this pass.
 * An improving pass zeroes stale, any other adds one; patience > 0: the pass at which stale ==
 * patience sets stop, after which the state is frozen (take = 0).  cursor == 0: a no-op. */
typedef struct {
    double loss_sum;
    unsigned int hits, index, stale, stop, valid, take;
} hpnn_best_state;
#define HPNN_BEST_LOSS 1
#define HPNN_BEST_ACC 2
int hpnn_best_commit(const hpnn_val_record *hist, const unsigned int *cursor, hpnn_best_state *state, int metric,
                     unsigned int patience, hipStream_t stream);
/* snapshot_if: one capturable launch that copies every segment of a DEVICE table {src, dst,
 * bytes} (n_segs <= HPNN_SNAP_MAX_SEGS) when the device word *take, read when the launch runs,
 * is not 0, and returns at once when it is 0; writes nothing outside [dst, dst + bytes).  bytes: any multiple of
 * 4; src / dst 16-byte aligned.  hpnn_snapshot_table checks a host table (-1: a pointer is not
 * aligned, a size no multiple of 4, too many segments; nothing is written) and copies it to the
 * device table `segs` (16-byte aligned; synchronises: setup, not for a capture).  The launch
 * itself checks segs / take and skips a segment that breaks the rules.  Neither launch
 * allocates, copies or synchronises. */
typedef struct {
    const void *src;
    void *dst;
    unsigned long long bytes;
} hpnn_snap_seg;
#define HPNN_SNAP_MAX_SEGS 32
int hpnn_snapshot_table(hpnn_snap_seg *segs, const hpnn_snap_seg *host_segs, int n_segs, hipStream_t stream);
int hpnn_snapshot_if(const hpnn_snap_seg *segs, int n_segs, const unsigned int *take, hipStream_t stream);
/* an empty one-thread launch of kernels_best.hip (capturable), and the same followed by a
 * synchronise: loads the unit's code object before a capture */
int hpnn_best_empty_launch(hipStream_t stream);
int hpnn_best_preload(hipStream_t stream);
/* ---- per-class validation metrics (kernels_confusion.hip; [confusion], rule in
 * <libhpnn/confusion.h>) ----
 * Every launch is capturable and allocates nothing.  M: uint32 [n_out][n_out + 1], zero before the
 * first add of a pass.
 * add: the rows of one evaluation chunk into M.  guess [rows] int32 as the evaluation kernels write
 * it (-1: not a sample, >= n_out: the "none" column); targets by t_kind: int32 labels [rows] (ldt
 * unused; a label outside [0, n_out) skips its row), or dense FP32 / FP64 rows ldt elements apart
 * (the target class is the lowest index of the largest value).  One unsigned atomic add per sample
 * into M in global memory: the result does not depend on the grid.  -1: refused. */
#define HPNN_CONFUSION_MAX_NOUT 4096
#define HPNN_CONFUSION_LABELS 0
#define HPNN_CONFUSION_F32 1
#define HPNN_CONFUSION_F64 2
int hpnn_confusion_add(const int *guess, const void *targets, int ldt, int t_kind, int rows, int n_out,
                       unsigned int *M, hipStream_t stream);
/* commit: one workgroup, in front of hpnn_validate_commit on the same stream (*cursor = the index
 * of the pass being filed; it is not advanced here): the per-class record support[n_out],
 * hit[n_out], predicted[n_out] into pc_hist[*cursor] (records of 3 n_out words; dropped when
 * *cursor >= cap or pc_hist is NULL), M copied to last (may be NULL), M zeroed */
int hpnn_confusion_commit(unsigned int *M, int n_out, unsigned int *pc_hist, unsigned int *last,
                          const unsigned int *cursor, unsigned int cap, hipStream_t stream);
/* loads the unit's code object (an empty launch and a synchronise) before a capture */
int hpnn_confusion_preload(hipStream_t stream);
/* ---- conjugate-gradient trainer (kernels_cg.hip; [train] CG, rules in <libhpnn/cg.h>) ----
 * Every launch is capturable, allocates nothing and reads its scalars (beta, the steps a_j) from
 * the DEVICE state when it runs.  f64 selects double, else float.  A segment is one layer:
 * n elements of W, W0, g, g_prev, d (element aligned; only the pointers a launch uses need be
 * set) and the S gradient slabs sstride elements apart that accumulate adds.  hpnn_cg_table
 * checks a host table (-1: refused, nothing written) and copies it to the device (synchronises:
 * setup).  Return: 0 launched, -1 refused, -5 launch error. */
typedef struct {
    void *w, *w0, *g, *gprev, *d;
    const void *slab;
    int S;
    long sstride;
    unsigned long long n;
} hpnn_cg_seg;
#define HPNN_CG_MAX_SEGS 16
#define HPNN_CG_DOT_WGS 64 /* partial triples of hpnn_cg_dots: partials holds 3 * 64 doubles */
int hpnn_cg_table(int f64, hpnn_cg_seg *segs, const hpnn_cg_seg *host_segs, int n_segs, hipStream_t stream);
/* g = ((first ? 0 : g) + slab[0] + ... + slab[S-1]) * scale, in slab order */
int hpnn_cg_accumulate(int f64, const hpnn_cg_seg *segs, int n_segs, int first, double scale, hipStream_t stream);
/* state->gg, gp, gd = <g,g>, <g,g_prev>, <g,d> over all segments: FP64 sums of FP64 products,
 * bitwise reproducible (two launches: the partials, then their sum in index order) */
int hpnn_cg_dots(int f64, const hpnn_cg_seg *segs, int n_segs, double *partials, hpnn_cg_state *state,
                 hipStream_t stream);
/* one thread: hpnn_cg_rule_direction on the device state */
int hpnn_cg_direction(hpnn_cg_state *state, hipStream_t stream);
/* d = fma(beta, d, g) (beta = 0: d = g), g_prev = g, W0 = W */
int hpnn_cg_begin(int f64, const hpnn_cg_seg *segs, int n_segs, const hpnn_cg_state *state, hipStream_t stream);
/* W = fma(a[j], d, W0), one fma in T; a[j] = 0: W = W0 bit for bit.  j <= HPNN_CG_FINAL */
int hpnn_cg_trial(int f64, const hpnn_cg_seg *segs, int n_segs, const hpnn_cg_state *state, int j,
                  hipStream_t stream);
/* the output layer forward only over rows [0, n_valid) of the logits Z (type 0 ANN, 1 LNN, 2 SNN,
 * as hpnn_output_fp): loss sum (FP64, floats 2..3 of a slot) and argmax hits (word 1) added into
 * the 64 stat slots, bitwise reproducible: 64 workgroups, one writer per slot, no atomics */
int hpnn_cg_loss(int f64, const void *Z, int ldz, const void *T, int ldt, float *slots, int n_valid, int n_out,
                 int type, hipStream_t stream);
/* one 64-lane workgroup: the 64 stat slots (layout of hpnn_validate_commit) summed in slot order
 * and zeroed, then hpnn_cg_rule_file(state, hist, j, sum, hits); hist may be NULL */
int hpnn_cg_file(float *slots, hpnn_cg_state *state, hpnn_cg_record *hist, int j, hipStream_t stream);
/* loads the unit's code object (an empty launch and a synchronise) before a capture */
int hpnn_cg_preload(hipStream_t stream);
/* ---- Adam trainer (kernels_adam.hip; [train] ADAM, rule in <libhpnn/adam.h>) ----
 * Every launch is capturable, allocates nothing and reads the state (the bias corrections of the
 * step) from DEVICE memory when it runs.  f64 selects double, else float.  A segment is one
 * layer: the weights, the two moments, n elements each, and the S gradient slabs gstride
 * elements apart.  hpnn_adam_table checks a host table (-1: refused, nothing written), fills
 * first_block / blocks (the workgroups of the launch that own the segment) and copies it to the
 * device (synchronises: setup).  Return: 0 launched, -1 refused, -5 launch error. */
typedef struct {
    void *w, *m, *v;
    const void *g;
    int S;
    int blocks;      /* filled by hpnn_adam_table */
    int first_block; /* filled by hpnn_adam_table */
    int pad;
    long gstride;
    unsigned long long n;
} hpnn_adam_seg;
#define HPNN_ADAM_MAX_SEGS 16
int hpnn_adam_table(int f64, hpnn_adam_seg *segs, const hpnn_adam_seg *host_segs, int n_segs, hipStream_t stream);
/* one thread: hpnn_adam_advance on the device state */
int hpnn_adam_advance_dev(hpnn_adam_state *state, hipStream_t stream);
/* every segment in one launch: g = (slab[0] + ... + slab[S-1]) * scale in slab order, then the
 * rule of adam.h in T with the coefficients the last advance left in *state */
int hpnn_adam_fp(int f64, const hpnn_adam_seg *segs, int n_segs, double scale, const hpnn_adam_state *state,
                 hipStream_t stream);
/* the BF16 plan's update, every layer (n <= HPNN_UPD_MAX) in one launch: the layer descriptor
 * of hpnn_sgd_update_multi (V32 = the first moment) plus the second moment A32.  g = scale * the
 * S slabs summed in the kernel's one fixed order (upd_common.h), the rule of adam.h in FP32,
 * then BF16 W, W^T and Wf exactly where hpnn_sgd_update_multi writes them */
typedef struct {
    hpnn_upd_layer u;
    float *A32;
} hpnn_adam_upd_layer;
int hpnn_adam_update_multi(const hpnn_adam_upd_layer *layers, int n, float scale, const hpnn_adam_state *state,
                           hipStream_t stream);
/* loads the unit's code object (an empty launch and a synchronise) before a capture */
int hpnn_adam_preload(hipStream_t stream);
/* ---- learning-rate schedules (kernels_lrsched.hip; [lr_schedule], rule in <libhpnn/lrsched.h>) ----
 * Every launch is capturable, allocates nothing and reads the rate from the DEVICE hpnn_lr_state
 * when it runs.  Return: 0 launched, -1 refused, -2 bad shape / alignment, -5 launch error.
 * advance: one thread runs hpnn_lr_advance, appends the new rate to hist[*hist_cursor] (a full
 * history, *hist_cursor == hist_cap, drops the record; hist may be NULL) and, when adam is not
 * NULL, stores it into adam->lr for the Adam advance of the next step. */
int hpnn_lr_advance_dev(hpnn_lr_state *state, hpnn_adam_state *adam, double *hist, unsigned int *hist_cursor,
                        unsigned int hist_cap, hipStream_t stream);
/* one thread, behind hpnn_validate_commit on the same stream: hpnn_lr_plateau on
 * vhist[*vcursor - 1].loss_sum; *vcursor == 0: a no-op */
int hpnn_lr_plateau_dev(const hpnn_val_record *vhist, const unsigned int *vcursor, hpnn_lr_state *state,
                        hipStream_t stream);
/* a segment is one layer of the FP64 / FP32 engines: the weights, the momentum (NULL under BP),
 * n elements each, and the S gradient slabs gstride elements apart.  hpnn_sgd_sched_table checks
 * a host table (-1: refused, nothing written), fills first_block / blocks and copies it to the
 * device (synchronises: setup), as hpnn_adam_table does */
typedef struct {
    void *w, *v;
    const void *g;
    int S;
    int blocks;      /* filled by hpnn_sgd_sched_table */
    int first_block; /* filled by hpnn_sgd_sched_table */
    int pad;
    long gstride;
    unsigned long long n;
} hpnn_sched_seg;
#define HPNN_SCHED_MAX_SEGS 16
int hpnn_sgd_sched_table(int f64, hpnn_sched_seg *segs, const hpnn_sched_seg *host_segs, int n_segs, int momentum,
                         hipStream_t stream);
/* every segment in one launch: g = (slab[0] + ... + slab[S-1]) * scale in slab order, then
 * BP  w += lr g   or   BPM  v += lr g; w += v; v *= alpha   with lr = (T)state->lr */
int hpnn_sgd_sched_fp(int f64, const hpnn_sched_seg *segs, int n_segs, double scale, double alpha, int momentum,
                      const hpnn_lr_state *state, hipStream_t stream);
/* the BF16 plan's BP / BPM step with the device rate, every layer in one launch (n > HPNN_UPD_MAX:
 * groups of HPNN_UPD_MAX, at most 16 layers): the slab sum in the one order of
 * hpnn_adam_update_multi, the rule in FP32, then BF16 W, W^T and Wf exactly where
 * hpnn_sgd_update_multi writes them */
int hpnn_sgd_sched_multi(const hpnn_upd_layer *layers, int n, float alpha, float scale, int momentum,
                         const hpnn_lr_state *state, hipStream_t stream);
/* loads the unit's code object (an empty launch and a synchronise) before a capture */
int hpnn_lrsched_preload(hipStream_t stream);
/* ---- gradient clipping by global norm (kernels_clip.hip; [clip], rule in <libhpnn/clip.h>) ----
 * Every launch is capturable, allocates nothing, reads the gradients only and reads / writes the
 * DEVICE hpnn_clip_state when it runs.  Return: 0 launched, -1 refused (nothing written), -5 launch
 * error.  A segment is one layer's gradient: n elements (linear index), S slabs gstride elements
 * apart.  hpnn_gnorm_table checks a host table (at most 16 segments), fills first_block (segment y
 * owns the blocks [first_block, first_block + ceil(n / 1024)) of the launch and the same entries of
 * partials[]), stores the total into *count and copies the table to the device (synchronises:
 * setup). */
typedef struct {
    const void *g;
    long gstride;
    unsigned long long n;
    int S;
    int first_block; /* filled by hpnn_gnorm_table */
} hpnn_gnorm_seg;
#define HPNN_GNORM_MAX_SEGS 16
int hpnn_gnorm_table(int f64, hpnn_gnorm_seg *segs, const hpnn_gnorm_seg *host_segs, int n_segs, int *count,
                     hipStream_t stream);
/* one workgroup per block of 1024 elements (count = the table's total): the element gs = (the slab
 * sum) * (T)scale -- slabs 0 .. S-1 in order from 0, or, interleaved, the 8-way order of the BF16
 * plan's sub-tile update -- squared in FP64 and summed in the order of clip.h into partials[block] */
int hpnn_gnorm_partials(int f64, int interleaved, const hpnn_gnorm_seg *segs, int n_segs, int count, double scale,
                        double *partials, hipStream_t stream);
/* one workgroup: partials[0 .. count) summed in the finalize's order, then hpnn_clip_finalize */
int hpnn_clip_finalize_dev(const double *partials, int count, hpnn_clip_state *state, hipStream_t stream);
/* one thread, the last launch of an epoch: hpnn_clip_commit (a full history, *cursor == cap, drops
 * the record; hist may be NULL) */
int hpnn_clip_commit_dev(hpnn_clip_state *state, hpnn_clip_record *hist, unsigned int *cursor, unsigned int cap,
                         hipStream_t stream);
/* the update launches above with the element gs * (T)clip->factor, the factor read when the launch
 * runs; clip NULL: exactly the launches above */
int hpnn_sgd_sched_fp_clip(int f64, const hpnn_sched_seg *segs, int n_segs, double scale, double alpha, int momentum,
                           const hpnn_lr_state *state, const hpnn_clip_state *clip, hipStream_t stream);
int hpnn_sgd_sched_multi_clip(const hpnn_upd_layer *layers, int n, float alpha, float scale, int momentum,
                              const hpnn_lr_state *state, const hpnn_clip_state *clip, hipStream_t stream);
int hpnn_adam_fp_clip(int f64, const hpnn_adam_seg *segs, int n_segs, double scale, const hpnn_adam_state *state,
                      const hpnn_clip_state *clip, hipStream_t stream);
int hpnn_adam_update_multi_clip(const hpnn_adam_upd_layer *layers, int n, float scale, const hpnn_adam_state *state,
                                const hpnn_clip_state *clip, hipStream_t stream);
/* loads the unit's code object (an empty launch and a synchronise) before a capture */
int hpnn_clip_preload(hipStream_t stream);
/* profiling (HPNN_TILE_TRACE=1): per-workgroup s_memtime stamps [1024][12] */
int hpnn_mlp3_tile_trace(unsigned long long *out);
/* HPNN_G0_TRACE=1 phase stamps of the fused G0 launch: out[512][8] */
int hpnn_g0_trace(unsigned long long *out);
/* ---- wide-input one-hidden-layer front (kernels_wide.hip): K0 (4096) -> 256 -> 256 ----
 * X [Bp][ldx] bf16 row-major, W0 [256][K0], W1 / W1t [256][256] bf16; outputs H0, D2 (delta
 * of the output layer), D1 (delta of the hidden layer), all [Bp][256] bf16 row-major; labels
 * or T [Bp][ldt]; with 2 workgroups per 128-sample tile (hpnn_wide2_ksplit) pbuf
 * (hpnn_wide2_pbuf_bytes), cnt / flag (Bp / 128 words each, zero once, self-resetting) and
 * err (one word, set on a hand-over timeout) are required. */
typedef struct {
    const void *X, *W0, *W1, *W1t;
    int ldx, K0;
    const int *labels;
    const float *T;
    int ldt;
    float t_hi, t_lo;
    void *H0, *D2, *D1, *pbuf;
    unsigned int *cnt, *flag, *err;
    float *loss_acc;
    unsigned int *correct;
    int Bp, n_valid, n_out, type;
    int ksplit; /* workgroups per tile: 1, 2, or 0 = hpnn_wide2_ksplit */
} hpnn_wide2_args;
int hpnn_wide2_front(const hpnn_wide2_args *a, hipStream_t stream);
int hpnn_wide2_ksplit(int Bp, int K0);
long hpnn_wide2_pbuf_bytes(int Bp);
/* profiling (HPNN_WIDE_TRACE=1): per-workgroup s_memtime stamps [512][12] */
int hpnn_wide2_trace(unsigned long long *out);
int hpnn_tn8_trace(unsigned long long *out); /* HPNN_TN8_TRACE=1: [512][8] MODE-2 phase stamps */
/* ---- FP64 / FP32 batched engine (kernels_fp.hip): f64 selects double, else float ----
 * gemm_fp: C[M x N] (ldc) = sum_k A(m, k) B(n, k) with A(m, k) = A[m*lda + k] (ta = 0) or
 * A[k*lda + m] (ta = 1), B(n, k) = B[n*ldb + k] (tb = 0) or B[k*ldb + n] (tb = 1), on the FP64 /
 * FP32 MFMA; epi as hpnn_gemm_nt_bf16 (aux [M x N], ldaux); splits > 1: split-K into
 * hpnn_gemm_fp_splits(K, splits) slabs slab_stride elements apart.  Any sizes. */
int hpnn_gemm_fp(int f64, const void *A, int lda, int ta, const void *B, int ldb, int tb, void *C, int ldc,
                 const void *aux, int ldaux, int M, int N, int K, int epi, int splits, long slab_stride,
                 hipStream_t stream);
int hpnn_gemm_fp_splits(int K, int splits);
/* output layer in FP64 / FP32: O (optional) = output, D (optional) = delta, guess (optional)
 * = argmax per row (first maximum), loss / hits into the stat slots for rows < n_valid
 * (T required for D, loss, hits) */
int hpnn_output_fp(int f64, const void *Z, int ldz, const void *T, int ldt, void *D, int ldd, void *O, int ldo,
                   int *guess, float *loss_acc, unsigned int *correct, int B, int n_valid, int n_out, int type,
                   hipStream_t stream);
/* the same output layer forward only (validation): no delta, no O; hits into slots[.][1], the
 * loss as a DOUBLE into floats 2..3 of each slot (hpnn_validate_commit adds both forms) */
int hpnn_output_fp_eval(int f64, const void *Z, int ldz, const void *T, int ldt, int *guess, float *slots, int B,
                        int n_valid, int n_out, int type, hipStream_t stream);
/* W += step(scale * sum_s G[s]) (BP / BPM), n elements */
int hpnn_update_fp(int f64, void *W, void *V, const void *G, int S, long gstride, long n, double lr, double alpha,
                   double scale, int momentum, hipStream_t stream);
/* out = sum_s G[s] */
int hpnn_reduce_fp(int f64, void *out, const void *G, int S, long gstride, long n, hipStream_t stream);
/* out[i] = in[i] * f'(aux[i]) (in place allowed): f' applied to reduced partial deltas */
int hpnn_dact_fp(int f64, void *out, const void *in, const void *aux, long n, hipStream_t stream);

/* floats per block slab written by hpnn_mlp3_mid */
int hpnn_mlp3_slab_floats(void);
/* deterministic 2-pass slab reduction: groups of slabs into tmp (>= 16*n floats,
 * NULL = single pass), then the groups into out */
int hpnn_reduce_slabs2(const float *slab, int S, long stride, long n, float *tmp, float *out,
                       hipStream_t stream);

/* first pass of hpnn_reduce_slabs2 only: out[g*n + i], g < groups (groups <= S) */
int hpnn_reduce_groups(const float *slab, int S, long stride, long n, int groups, float *out, hipStream_t stream);

/* online (batch-1) FP64 persistent engine, see online.hip */
typedef struct {
    int L;
    int n_in;
    int N[16];
    int M[16];
    double *W[16];
    double *dW[16];
    int type;     /* 0 ANN 1 LNN 2 SNN */
    int momentum;
    double lr;
    double alpha;
    double delta;
    int min_iter;
    int max_iter;
    const double *x;
    const double *t;
    double *out;       /* n_out, final network output */
    double *scratch;   /* vectors when they do not fit in LDS */
    double *result;    /* [0]=dEp [1]=init_err [2]=iter [3]=ok [4]=first_ok */
    int use_lds;
    int forward_only;
    /* multi-workgroup (cooperative) variant, online.hip: exchange vectors + partials
     * (hpnn_online_coop_xch_bytes) and the control words (HPNN_ONLINE_CTL_BYTES) */
    double *xch;
    unsigned int *ctl;
    /* device-spanning cooperative grid (online training over several GPUs, the reference's
     * row sharding of cuda_ann.cu:533-1275 over n_gpu x n_streams): this launch is slot
     * `dev_slot` of `n_slots` launches of `grid` workgroups each (one per GPU, or several
     * virtual slots on one GPU); workgroup g = dev_slot * grid + blockIdx.x of
     * n_slots * grid owns rows j == g (mod n_slots * grid) of every layer, and only those
     * rows of its slot's W / dW are read or written.  xch / ctl are ONE allocation that
     * every slot's device maps (fine-grained), accessed at system scope.  n_slots <= 1:
     * the single-device kernel. */
    int dev_slot, n_slots;
} hpnn_online_args;

#define HPNN_ONLINE_CTL_BYTES 1024
/* grid of the cooperative online kernel (0: not applicable -> single-workgroup kernel) */
int hpnn_online_coop_grid(const hpnn_online_args *a);
long hpnn_online_coop_xch_bytes(const hpnn_online_args *a, int grid);
/* one sample on `grid` workgroups (all resident): every layer's rows are spread over the
 * workgroups, vectors and delta partials are exchanged through write-through stores and
 * a counter barrier; returns 0, or < 0 (launch error) */
int hpnn_online_coop_launch(const hpnn_online_args *a, int grid, hipStream_t stream);
/* device-spanning form: workgroups per slot for n_slots slots (0: not applicable);
 * per_device_cap bounds one device's share of resident workgroups */
int hpnn_online_coop_grid_slots(const hpnn_online_args *a, int n_slots, int per_device_cap);
/* 0, or -1 when a barrier of the last cooperative launch timed out (ctl read back) */
int hpnn_online_coop_status(const hpnn_online_args *a);

int hpnn_online_launch(const hpnn_online_args *a, hipStream_t stream);
/* bytes of vector storage the online kernel needs */
long hpnn_online_vec_bytes(const hpnn_online_args *a);

#ifdef __cplusplus
}
#endif

/* one probe kernel per translation unit: hpnn_preload_code_objects() queries its attributes,
 * which loads that unit's code object onto the device */
#define HPNN_CO_PROBE(tu)                                                                  \
    __global__ void hpnn_co_probe_kernel_##tu() {}                                         \
    extern "C" const void *hpnn_co_probe_##tu(void) { return (const void *)hpnn_co_probe_kernel_##tu; }
#endif
