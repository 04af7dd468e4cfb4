/*
 * The batched BF16 training plan: ONE orchestrator of the gfx950 kernels, used by the C
 * library's batched engine (train_nn -m batched: train_single.cpp / train_dp.cpp /
 * train_dp_mp.cpp, infer_batched.cpp) and, through the pybind11 module, by hpnn_amd.models.MLP
 * (bench.py, the data-parallel driver, the tests).  Reference being replaced: the per-layer
 * GEMV / GER sequence of nn_train_kernel -> {ann,snn}_train_BP[M] (libhpnn.c:1149-1302,
 * cuda_snn.cu:2726-3717), here over a minibatch.
 *
 * A plan is
 *   - a configuration (host only, no device needed): padded dims, the step structure
 *     ("mode"), split-K factors, grids, and the table of device buffers it needs;
 *   - memory: either allocated by the plan (C engine) or bound to buffers the host
 *     framework allocated from that table (Python: torch tensors, so they are views);
 *   - launches on a caller-given HIP stream, all capturable in a HIP graph.
 *
 * Modes (the step's kernel sequence):
 *   't'  MNIST-shaped n_in(800|256)-128-64-(<=32): mlp3_tile front (X -> delta1 + [G1|G2]
 *        block slabs) -> G0 with its split-K reduction and every layer's optimizer step in
 *        the same launch (kernels_g0.hip g0_fused_kernel): two launches per step.  Input
 *        fragment-major (8-bit pixels or BF16).
 *   'x'  same shape, 32-sample pipelined front (mlp3_fused), row-major BF16 input (plus an
 *        optional fragment-major 8-bit copy for G0).
 *   'm'  same shape, gemm_nt layer 0 + mlp3_mid.
 *   'w'  K0 = 4096 -> 256 -> 256 (padded): wide2_front, then per-layer weight gradients
 *        (8-phase TN with the update in its epilogue where it applies) and updates.
 *   0    any net: per-layer gemm_nt forward / output_delta / gemm_nt deltas / gemm_tn
 *        gradients / one multi-layer update.
 */
#ifndef HPNN_GPU_BPLAN_H
#define HPNN_GPU_BPLAN_H
#include <hip/hip_runtime_api.h>
#include <stdlib.h>

#include <functional>
#include <string>
#include <vector>

#include "kernels.h"

namespace hpnn {

enum BDtype { BD_F32 = 0, BD_BF16 = 1, BD_U8 = 2, BD_I32 = 3 };

/* one device buffer of the plan */
struct BufSpec {
    std::string name; /* "W32", "V32", "Wb", "Wt", "slab", "gflat", "H", "D", "Z", "stats", ... */
    int layer;        /* -1: not per layer */
    int dtype;        /* BDtype */
    int ndim;
    long shape[4];
    bool zero; /* must start zeroed */
    size_t bytes() const;
};

/* one prepared minibatch: x = the front's input (row-major [Bp][Kp0] BF16, or fragment-major
 * [Bp/32][Kp0/16][64][8] for mode 't', 8-bit when u8), xg = fragment-major 8-bit copy for the
 * first-layer gradient (mode 'x' only, may be null); the network sees bf16(byte * scale) */
struct XIn {
    const void *x = nullptr;
    const void *xg = nullptr;
    int u8 = 0;
    float scale = 1.f;
    /* evaluate() only: x is row-major BF16 [rows][Kp0] whatever the plan's layout (the
     * per-layer path of a mode 't' plan) */
    int rowmajor = 0;
};

/* gradient ready for exchange: layers lo..hi (contiguous in gflat) are final */
typedef std::function<bool(int lo, int hi)> ReadyFn;

/* the gradient of a step left in its unreduced form (the xGMI all-reduce sums the slabs in its
 * copy-in): segment i = sum over cnt[i] slabs of n[i] floats, stride[i] apart, at base[i] */
struct SlabSegs {
    int count = 0;
    const float *base[2];
    int cnt[2];
    long n[2], stride[2];
};

class BPlan {
  public:
    /* ---- configuration ---- */
    int L = 0, type = 2, batch = 0, Bp = 0, n_out = 0;
    bool momentum = false, on_device = true;
    int M[16], N[16], Kp[16], Np[16], S[16];
    char mode = 0;
    int mid_grid = 0, mid_groups = 1, wide_ksplit = 1, slab_f = 0;
    bool g0_fused = true; /* modes t / x: G0 + reduction + every step in one launch when it applies */
    int g0_perm = 0;      /* tests: > 0 runs the fused G0 grid in a permuted block -> role order */
    /* mode 't': the fused G0 step does not store the BF16 copies that neither the tile front nor
     * hpnn_mlp3_eval reads -- W0, W0^T and W1^T; they go stale (stale_copies) until sync_copies
     * re-derives them from the FP32 masters, which every reader of them does first.  false
     * (tests): every step stores them */
    bool lazy_copies = true;
    /* bit l: Wb[l] is behind W32[l]; bit 16 + l: Wt[l] is */
    unsigned stale_copies() const { return stale_; }
    /* brings the stale copies up to date on s (a cast of layer 0, a transpose of layer 1); nothing
     * is launched when none is stale.  Steps captured into a graph run again without the plan
     * knowing: after such a capture the copies count as stale for good */
    int sync_copies(hipStream_t s);
    bool tn_update = true; /* the step in the 8-phase TN gradient's epilogue where it applies */
    /* two-layer nets: layer 1's gradient + step as the side job of layer 0's fused TN launch */
    bool tn8_side = [] { const char *e = getenv("HPNN_TN8_SIDE"); return !(e && e[0] == '0'); }();
    long side_launches = 0; /* launches issued with that side job (tests) */
    /* [train] ADAM (set_adam): the optimizer of every step; V32 is then the first moment, A32
     * the second, "adam" the device hpnn_adam_state the update reads when it runs */
    bool adam = false;
    hpnn_adam_state adam0;  /* the state a fresh plan starts from (allocate uploads it) */
    long adam_launches = 0; /* launches of kernels_adam.hip issued by this plan (tests) */
    /* [lr_schedule] (set_schedule): the BP / BPM step reads its rate from "lrs", the device
     * hpnn_lr_state, when it runs; under ADAM the advance of the schedule stores it into "adam" */
    bool sched = false;
    hpnn_lr_state lrs0;      /* the state a fresh plan starts from (allocate uploads it) */
    long sched_launches = 0; /* launches of kernels_lrsched.hip issued by this plan (tests) */
    /* [clip] (set_clip): every optimizer step is gnorm_partials -> finalize -> update with the
     * factor of "clip", the device hpnn_clip_state, read when the update runs */
    bool clip = false;
    hpnn_clip_state clip0;  /* the state a fresh plan starts from (allocate uploads it) */
    double clip_lr = 0.0;   /* the rate of plain BP / BPM under [clip] (no schedule, no ADAM) */
    long clip_launches = 0; /* launches of kernels_clip.hip issued by this plan (tests) */
    int clip_count = 0;     /* entries of "clip_part": the 1024-element blocks of every layer */
    /* per-layer: the delta GEMM reads W (NN form, hpnn_gemm_nn_bf16) instead of W^T, which is
     * then not kept current (the sharded data-parallel step sets it: no transpose per update) */
    bool nn_bwd[16] = {false};
    size_t goff[17] = {0};
    std::vector<BufSpec> specs;

    /* [train] ADAM, before configure: Adam / AdamW (<libhpnn/adam.h>) takes the place of BP / BPM.
     * Forces the moments on (V32, plus the specs "A32" per layer and "adam", the state) and turns
     * off the three places where a BP / BPM step is fused into a gradient launch (g0_fused,
     * tn_update, tn8_side), so every mode runs its unfused sequence and ends in the advance plus
     * ONE hpnn_adam_update_multi over all layers.  step() / update_flat() then ignore their lr and
     * alpha; update_layer() is refused (one advance per step).  -1: coefficients out of range. */
    int set_adam(double lr, double beta1, double beta2, double eps, double decay);
    /* [lr_schedule], before configure: adds the buffer spec "lrs" (the device hpnn_lr_state, which
     * starts as st) and turns off the fused BP / BPM epilogues exactly as set_adam does, so every
     * mode ends in ONE hpnn_sgd_sched_multi over all layers with the rate read from the device
     * (<libhpnn/lrsched.h>, docs/DESIGN.md 3.2j).  step() / update_flat() then ignore their lr;
     * update_layer() and xchg_step() are refused.  The caller launches advance_schedule() once
     * per epoch, before its first step.  -1: hpnn_lr_valid fails. */
    int set_schedule(const hpnn_lr_state &st);
    /* one hpnn_lr_advance_dev on the plan's state (and its Adam state, if any); hist / cursor /
     * cap: the device history of rates, may be null */
    int advance_schedule(double *hist, unsigned int *cursor, unsigned int cap, hipStream_t s);
    /* [clip], before configure: gradient clipping by global norm (<libhpnn/clip.h>, docs/DESIGN.md
     * 3.2k).  Adds the buffer specs "clip" (the device hpnn_clip_state), "clip_part" (one double per
     * 1024-element block of every layer) and "clip_tab" (the segment table) and turns off the fused
     * BP / BPM epilogues exactly as set_schedule does, so every mode ends in apply_optimizer:
     * hpnn_gnorm_partials -> hpnn_clip_finalize_dev -> the update launch of ADAM / [lr_schedule]
     * with the factor.  Plain BP / BPM runs hpnn_sgd_sched_multi on a constant-kind "lrs" that
     * holds lr (step() / update_flat() then ignore their lr); update_layer() and xchg_step() are
     * refused.  -1: max_norm is not a finite number > 0. */
    int set_clip(double max_norm, double lr);
    /* behind allocate / bind: uploads the segment table of step()'s optimizer launch (synchronises;
     * a step whose layers differ from the uploaded table uploads its own, which a capture refuses) */
    int prepare_clip(hipStream_t s);
    /* one hpnn_clip_commit_dev on the plan's state, the last launch of an epoch; hist / cursor /
     * cap: the device history of epoch records, may be null */
    int commit_clip(hpnn_clip_record *hist, unsigned int *cursor, unsigned int cap, hipStream_t s);
    /* the steps that are fused into a gradient launch are off: the optimizer runs on its own */
    bool unfused() const { return adam || sched || clip; }
    /* fused: -1 auto (the fastest eligible mode), 0 per-layer only, or 't' / 'x' / 'm' / 'w'
     * (an error when not eligible); splits: per-layer split-K override (null / 0 = pick);
     * mid_grid_req: block slabs of mode 'm'; on_device = false: a host-only configuration
     * (CPU emulation: grids of 1).  Returns 0 or a negative error (message in err). */
    int configure(const int *sizes, int n_layers, int net_type, int batch_size, bool momentum_, int fused,
                  const int *splits, int mid_grid_req, bool device, std::string *err = nullptr);
    /* the layout prepare_input must produce: 1 = fragment-major main input (mode 't'),
     * 2 = row-major BF16 plus a fragment-major 8-bit copy when the data are 8-bit (mode 'x'),
     * 0 = row-major BF16 */
    int input_layout() const { return mode == 't' ? 1 : (mode == 'x' ? 2 : 0); }
    /* split-K factor of a weight gradient (N x K over Bp rows) for this plan's kernels */
    static int pick_splits(int Np, int Kp, int Bp);

    /* ---- memory ---- */
    int allocate(hipStream_t s); /* every spec via hpnn_dev_malloc, zeroed where required */
    int bind(void *const *ptrs); /* one pointer per spec, in spec order (caller owns them) */
    ~BPlan();
    void *buf(const char *name, int layer = -1) const;

    /* ---- launches (stream s) ---- */
    int cast_weights(hipStream_t s); /* BF16 copies (and W0f) from the FP32 masters */
    int zero_stats(hipStream_t s);
    /* per-layer building blocks */
    int forward(const void *X, hipStream_t s); /* row-major BF16 input -> H[], Z */
    int output(const int *labels, const float *T, int ldt, int n_valid, float *O, int ldo, bool stats,
               hipStream_t s, float *slots = nullptr); /* slots: the statistics go there, not to stats */
    int backward_layer(int l, hipStream_t s);                                 /* D[l-1] from D[l] */
    int grad_layer(int l, const XIn &x, bool reduce, hipStream_t s);         /* slab[l] / G[l] */
    int update_layer(int l, float lr, float alpha, float scale, bool from_g, hipStream_t s);
    /* fused front of modes t / x / m / w (X -> deltas, [G1|G2] block slabs) */
    int front(const XIn &x, const int *labels, const float *T, int ldt, int n_valid, hipStream_t s);
    /* whole training step: fwd + bwd + update (no host sync) */
    int step(const XIn &x, const int *labels, const float *T, int ldt, int n_valid, float lr, float alpha,
             hipStream_t s);
    /* data parallel: gradients summed over this replica's samples into gflat, ready(lo, hi) as
     * each bucket becomes final (last layers first) */
    int grads(const XIn &x, const int *labels, const float *T, int ldt, int n_valid, const ReadyFn &ready,
              hipStream_t s);
    std::vector<std::pair<int, int>> buckets() const;
    /* fused modes: front + G0 with the gradient left in slabs (the xGMI all-reduce's copy-in
     * sums them); segs[0] = G0 slabs, segs[1] = [G1|G2] groups -- or, when the G0 launch
     * reduces in-kernel, ONE segment: gflat itself, fully reduced.  dst (with sel / alt, see
     * hpnn_g0_update.gsel): the in-kernel reduced gradient goes there instead (the xGMI
     * all-reduce's own buffer half) and segs->count = 0 */
    int grads_slabs(const XIn &x, const int *labels, const float *T, int ldt, int n_valid, SlabSegs *segs,
                    hipStream_t s, float *dst = nullptr, const unsigned int *sel = nullptr, long alt = 0);
    /* fused modes: front + every layer's gradient summed over this replica's samples into
     * gflat, with G0's split-K and [G1|G2] reductions inside the G0 launch when it applies
     * (two launches; the exchange then moves one copy) */
    int grads_local(const XIn &x, const int *labels, const float *T, int ldt, int n_valid, hipStream_t s);
    /* fused modes, data parallel: front, then G0 with its split-K reduction, the exchange over
     * xv (one-shot xGMI protocol inside the launch, kernels_g0.hip) and every layer's step --
     * the single-GPU step's two launches; scale includes 1 / world.  -1 (nothing launched)
     * when the fused G0 does not cover the shape or the input. */
    int xchg_step(const XIn &x, const int *labels, const float *T, int ldt, int n_valid, float lr, float alpha,
                  float scale, const hpnn_xar_view &xv, hipStream_t s);
    /* collective self-test of that in-kernel exchange on xv (known pattern, exact sums checked
     * on the host): 0 when every float arrived right, > 0 wrong floats, -1 not covered */
    int xchg_self_test(const hpnn_xar_view &xv, hipStream_t s);
    int update_flat(const float *G, float lr, float alpha, float scale, hipStream_t s);
    /* layer l's weight gradient and step run as ONE 8-phase TN launch */
    bool tn_update_ok(int l) const;
    /* forward only (validation): loss and argmax hits of the first n_valid rows of x added
     * into the caller's 64 stat slots (vstats, or any buffer of that layout); guess (may be
     * null): int32 per row, the lowest index of the largest output, -1 from n_valid up.
     * Mode 't' with a fragment-major x: one hpnn_mlp3_eval launch over n_valid rows padded to
     * 256 (any number of tiles; guess holds that many); every other input: forward() + the
     * output kernel on one chunk, n_valid <= Bp (guess holds Bp).  Changes nothing a training
     * step reads later: H, Z and D[L-1] are scratch the next step rewrites.  eval_fused
     * (HPNN_EVAL_FUSED=0: off) selects the per-layer path in mode 't' too; x must then be
     * row-major (x.rowmajor).  -2 when the input's layout does not fit the path. */
    int evaluate(const XIn &x, const int *labels, const float *T, int ldt, int n_valid, float *slots, int *guess,
                 hipStream_t s);
    bool eval_fused = [] { const char *e = getenv("HPNN_EVAL_FUSED"); return !(e && e[0] == '0'); }();
    bool eval_is_fused() const { return mode == 't' && eval_fused; }
    /* network outputs O [Bp][ldo] FP32 of a row-major BF16 batch */
    int predict(const void *X, int n_valid, float *O, int ldo, hipStream_t s);
    /* 0, or -9 when an in-kernel hand-over (wide front partials, fused G0 splits) timed out
     * since the plan was created (synchronises s) */
    int health(hipStream_t s);
    /* the same words copied into dst[0..2] (pinned host memory, zeroed by the caller) on s
     * without waiting: a training loop checks them one replay later, so the check never
     * leaves the GPU idle; any non-zero word = a timed-out hand-off */
    int health_enqueue(hipStream_t s, unsigned int *dst);
    /* 64-bit digest of the weights (bit 1: BF16 copies W / W^T of every layer, bit 2: the FP32
     * masters); data-parallel replicas must agree on it bit for bit (synchronises s) */
    int weights_digest(int which, unsigned long long *out, hipStream_t s);
    /* (loss sum, hits) summed over the stat slots (synchronises s) */
    int read_stats(double *loss, unsigned int *hits, hipStream_t s);

    /* named pointers (valid after allocate / bind) */
    float *W32[16] = {0}, *V32[16] = {0}, *A32[16] = {0}, *slab[16] = {0};
    hpnn_adam_state *adam_dev = nullptr;
    hpnn_lr_state *lrs_dev = nullptr;
    hpnn_clip_state *clip_dev = nullptr;
    double *clip_part = nullptr;
    hpnn_gnorm_seg *clip_tab = nullptr;
    void *Wb[16] = {0}, *Wt[16] = {0}, *H[16] = {0}, *D[16] = {0};
    float *Z = nullptr, *stats = nullptr, *vstats = nullptr, *gflat = nullptr, *midslab = nullptr, *midtmp = nullptr;
    void *W0f = nullptr;
    float *wpbuf = nullptr;
    unsigned int *wwords = nullptr, *g0cnt = nullptr, *tncnt = nullptr;
    int *lab0 = nullptr;
    /* data-parallel BF16 exchange (csrc/dist/dp_exchange.cpp): where grad_layer(reduce) may
     * write layer l's gradient as BF16 instead of FP32 into gflat (NULL: FP32), and whether the
     * last call did (shapes the 8-phase kernel does not cover stay FP32) */
    void *g16[16] = {0};
    bool g16_used[16] = {0};

  private:
    std::vector<void *> ptr_;
    bool owns_ = false;
    unsigned long long *digest_ = nullptr; /* device word of weights_digest */
    unsigned stale_ = 0;                   /* stale_copies() */
    bool stale_captured_ = false;          /* a lazy step sits in a captured graph */
    /* the one place a step's optimizer is applied to layers whose gradients are in memory:
     * hpnn_sgd_update_multi, or under ADAM the advance plus hpnn_adam_update_multi */
    int apply_optimizer(const hpnn_upd_layer *u, int n, float lr, float alpha, float scale, hipStream_t s);
    int grad_and_update_layers(const XIn &x, float lr, float alpha, float scale, hipStream_t s);
    int g0_reduce(const XIn &x, hipStream_t s);
    int g0_fused_step(const XIn &x, float lr, float alpha, float scale, hipStream_t s, float *gout = nullptr,
                      const unsigned int *gsel = nullptr, long galt = 0, const hpnn_xar_view *xv = nullptr);
    const void *fm_input(const XIn &x) const;
    /* [clip]: the table of the layers u on the device (uploaded when it differs from the last) */
    int clip_table(const hpnn_upd_layer *u, int n, hipStream_t s);
    hpnn_gnorm_seg clip_host_[16];
    int clip_host_n_ = 0, clip_blocks_ = 0;
    void name_pointers();
};

}  // namespace hpnn

#endif
