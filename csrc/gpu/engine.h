/*
 * libhpnn GPU engines (HIP, gfx950) -- host-side interface.
 *
 * Two engines live behind this header:
 *   online  : the reference's batch-1, iterate-to-convergence training
 *              in FP64.  The WHOLE per-sample convergence loop
 *             (train step, re-forward, error, argmax, stop test) runs inside
 *             one persistent single-workgroup kernel, so there is no host
 *             round trip per iteration (the reference synchronised the host
 *             on every iteration: ann.c:2329-2332, cuda_ann.cu:1294).
 *   batched : minibatch SGD / momentum with MFMA GEMMs (BF16 in, FP32
 *             accumulate, FP32 master weights) or FP32/FP64 MFMA.
 */
#ifndef HPNN_GPU_ENGINE_H
#define HPNN_GPU_ENGINE_H
#include <libhpnn/ann.h>
#include <libhpnn/cg.h>
#include <libhpnn/adam.h>
#include <libhpnn/lrsched.h>
#include <libhpnn/clip.h>
#include <libhpnn/confusion.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- online (reference semantics) ---- */
/* uploads the host weights if the device copy is stale */
BOOL hpnn_gpu_online_prepare(kernel_ann *k, UINT gpu);
DOUBLE hpnn_gpu_train_sample(kernel_ann *k, nn_type type, nn_train train, const DOUBLE *in,
                             const DOUBLE *out, DOUBLE lr, DOUBLE alpha, DOUBLE delta, UINT *n_iter,
                             BOOL *ok, DOUBLE *init_err, BOOL *first_ok);
/* forward only; result copied to k->output.vec (host) */
BOOL hpnn_gpu_forward(kernel_ann *k, nn_type type, const DOUBLE *in);
/* device weights -> host master copy (no-op if host is current) */
void hpnn_gpu_sync_host(kernel_ann *k);
/* TRUE once a device state was lost (a grid barrier timed out mid-sample): the caller
 * stops training; the host weights are the last consistent ones */
BOOL hpnn_gpu_failed(const kernel_ann *k);
/* online slot layout (pure): n_gpu, -S streams, runtime memory model, HPNN_ONLINE_SLOTS */
int hpnn_online_slot_plan(int n_gpu, int n_streams, int mem_model, int env_slots, int *spd);
/* host master copy changed: mark device copy stale */
void hpnn_gpu_mark_host_dirty(kernel_ann *k);

/* ---- batched ---- */
typedef struct {
    nn_type type;
    nn_train train;
    nn_dtype dtype;
    UINT batch;
    UINT epochs;
    DOUBLE lr;
    DOUBLE alpha;
    UINT seed;
    UINT n_gpu;       /* data-parallel replicas driven by this process */
    BOOL resume;      /* BPM: start from the momentum in k->dw (exact resume)  */
    UINT epoch0;      /* epochs completed before this call (metrics numbering) */
    UINT tp;          /* 1: row-sharded tensor parallelism ([parallel] tp; f64 / f32 / bf16) */
    UINT shuffle;     /* 1: a new sample order every epoch (<libhpnn/shuffle.h>, epoch = epoch0 + e;
                       * single-device engines only); 0: the order drawn once */
    /* [validate] N: the held-out set (host, row-major FP64, nv x n_in / nv x n_out), evaluated
     * forward-only after every epoch whose absolute number epoch0 + e + 1 is a multiple of
     * validate and after the last epoch of the call; validate = 0: off (single-device engines) */
    const DOUBLE *Xv;
    const DOUBLE *Tv;
    UINT nv;
    UINT validate;
    /* [keep_best] loss | acc (nn_keep_best; 0: off): the call returns the weights and momentum of
     * its best validation pass; [patience] P (0: never): stop once P passes in a row have not
     * improved.  Both need validate > 0 (single-device engines). */
    UINT keep_best;
    UINT patience;
    /* [train] ADAM: the coefficients (lr is the step size, alpha is unused); resume: start from
     * the moments k->dw, k->dv and k->adam_t, adam_p1, adam_p2 */
    DOUBLE beta1, beta2, eps, decay;
    /* [lr_schedule] (sched = 1; single-device engines and the CPU oracle): the state the call starts
     * from -- lr0 = lr, epoch = epoch0, and under plateau the running fields of a loaded state file.
     * The step size of every epoch is then the state's lr (<libhpnn/lrsched.h>), not `lr` */
    UINT sched;
    hpnn_lr_state lrs;
    /* [clip] c (single-device engines and the CPU oracle; 0: off): the gradient of every step is
     * rescaled when its global L2 norm exceeds c (<libhpnn/clip.h>); BP, BPM and ADAM */
    DOUBLE clip;
    /* [confusion] (1: on; single-device engines and the CPU oracle; needs validate > 0): every
     * validation pass also tallies its confusion matrix and per-class record
     * (<libhpnn/confusion.h>) */
    UINT confusion;
} hpnn_batched_opts;

/* one validation pass: the absolute epoch it followed, the mean loss per sample and the argmax
 * hits over the n held-out samples */
typedef struct {
    UINT epoch;
    DOUBLE loss;
    UINT correct;
    UINT n;
} hpnn_validation_record;

typedef struct {
    DOUBLE last_loss;   /* mean loss of the last minibatch            */
    DOUBLE epoch_loss;  /* mean loss over the last epoch              */
    UINT64 samples;     /* samples processed                          */
    DOUBLE seconds;     /* wall time spent in the training loop       */
    UINT correct;       /* argmax hits in the last epoch              */
    /* [validate]: n_val records in epoch order, malloc'ed by the engine (the caller frees val) */
    hpnn_validation_record *val;
    UINT n_val;
    /* [keep_best]: the absolute epoch of the best pass (0: none was taken) and its index in val;
     * the epochs the call ran (after a stop the GPU engine may have run some past the stopping
     * pass: they change nothing that is returned); [patience]: the absolute epoch of the
     * stopping pass (0: no stop), always val[n_val - 1].epoch */
    UINT best_epoch;
    UINT best_index;
    UINT epochs_run;
    UINT stop_epoch;
    /* [train] CG: one record per iteration (= epoch) of the call up to the last one that counts,
     * malloc'ed by the engine (the caller frees cg) */
    hpnn_cg_record *cg;
    UINT n_cg;
    /* [lr_schedule]: the rate of every epoch of the call up to the last one that counts (the
     * stopping pass's epoch after an early stop), malloc'ed by the engine (the caller frees
     * lr_hist), and the schedule state of the returned kernel (the best pass's under [keep_best]) */
    DOUBLE *lr_hist;
    UINT n_lr;
    hpnn_lr_state lrs;
    /* [clip]: one record per epoch of the call up to the last one that counts (steps, clipped
     * steps, the largest and the last norm), malloc'ed by the engine (the caller frees clip_hist) */
    hpnn_clip_record *clip_hist;
    UINT n_clip;
    /* [confusion]: n_classes = the net's outputs (0: off); one per-class record (support, hit,
     * predicted: 3 n_classes words) per validation record of val; the matrix
     * [n_classes][n_classes + 1] of the last pass reported and of the best pass (NULL: none); all
     * malloc'ed by the engine (the caller frees them); confusion_launches: the tally launches the
     * driver issued, captured ones once per capture and not per replay (0 when off) */
    UINT n_classes;
    UINT *class_hist;
    UINT n_class_hist;
    UINT *confusion_last;
    UINT *confusion_best;
    UINT confusion_launches;
} hpnn_batched_stats;

/* the improvement rule of [keep_best] (one definition for every engine; the device form is
 * hpnn_best_commit): does a pass with (loss_sum, hits) improve on the best one so far? */
static inline int hpnn_best_improves(int metric, int have_best, double loss_sum, unsigned int hits,
                                     double best_loss_sum, unsigned int best_hits) {
    if (!have_best) return metric == 2 /* NN_KEEP_ACC */ || loss_sum == loss_sum;
    if (metric == 2) return hits > best_hits || (hits == best_hits && loss_sum < best_loss_sum);
    return loss_sum < best_loss_sum;
}

/* the epochs (absolute numbers, ascending) a call of `epochs` epochs after `epoch0` completed
 * ones validates at; out may be NULL; returns the count */
UINT hpnn_validation_schedule(UINT epoch0, UINT epochs, UINT validate, UINT *out);

/* data-parallel shard (pure): rank's rows [*start, *start + *nv) of global minibatch b (B samples
 * of n, Bg = ceil(B / world) per rank) and *total, the samples of the whole minibatch */
void hpnn_dp_shard(int b, int B, int n, int rank, int Bg, int *start, int *nv, int *total);

/* X: n x n_in, T: n x n_out (host, row-major FP64). Weights are read from
 * and written back to the host kernel; with BPM the final momentum is written to
 * k->dw (allocated if needed) so that nn_dump_state can save it. */
BOOL hpnn_gpu_train_batched(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n,
                            const hpnn_batched_opts *o, hpnn_batched_stats *st);
/* the same with every hidden layer's rows sharded over the ranks (tp_engine.cpp): ranks =
 * HPNN_LOOPBACK_RANKS threads on GPU 0, the launcher's processes, or o->n_gpu GPUs */
BOOL hpnn_gpu_train_tp(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                       hpnn_batched_stats *st);
/* batched inference: Y = net(X), n x n_out (host) */
BOOL hpnn_gpu_infer_batched(kernel_ann *k, nn_type type, nn_dtype dtype, const DOUBLE *X, UINT n,
                            DOUBLE *Y);

/* CPU batched engine (FP64 oracle for the batched semantics) */
BOOL hpnn_cpu_train_batched(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n,
                            const hpnn_batched_opts *o, hpnn_batched_stats *st);
/* one minibatch step on the CPU: returns mean loss before the update */
DOUBLE hpnn_cpu_batched_step(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT b,
                             DOUBLE lr, BOOL momentum, DOUBLE alpha, UINT *hits /* may be NULL: += argmax hits */);

/* ---- [train] CG on the host (the FP64 oracle and the CPU form of hpnn_amd.ops.cg_*): the
 * rules of <libhpnn/cg.h> on host memory; f64 selects double, else float ---- */
/* G[l] (+)= sum_b delta_l^b (x) h_{l-1}^b over the B samples, in sample order (first: G is
 * overwritten); returns the loss SUM of the batch, *hits += argmax hits */
DOUBLE hpnn_cpu_batched_grad(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT b, DOUBLE **G,
                             BOOL first, UINT *hits);
void hpnn_cg_host_init(hpnn_cg_state *s, double a_init, unsigned int n, unsigned int cap);
void hpnn_cg_host_accumulate(int f64, void *g, const void *slab, int S, long sstride, long n, int first, double scale);
/* out[0..2] += <g,g>, <g,g_prev>, <g,d>: FP64 products added in element order */
void hpnn_cg_host_dots(int f64, const void *g, const void *gprev, const void *d, long n, double *out);
void hpnn_cg_host_direction(hpnn_cg_state *s);
void hpnn_cg_host_begin(int f64, const void *w, void *w0, const void *g, void *gprev, void *d, long n, double beta);
void hpnn_cg_host_trial(int f64, void *w, const void *w0, const void *d, long n, double a);
void hpnn_cg_host_file(hpnn_cg_state *s, hpnn_cg_record *hist, unsigned int j, double loss_sum, unsigned int hits);

/* ---- [train] ADAM on the host (the FP64 oracle and the CPU form of hpnn_amd.ops.adam_*): the
 * rule of <libhpnn/adam.h> on host memory; f64 selects double, else float ---- */
void hpnn_adam_host_init(hpnn_adam_state *s, double lr, double beta1, double beta2, double eps, double decay);
void hpnn_adam_host_advance(hpnn_adam_state *s);
/* g = (G[0] + G[1] + ... + G[S-1]) * scale, slabs gstride elements apart, in slab order; then the
 * rule on W, M (first moment), V (second moment) with the coefficients the last advance derived */
void hpnn_adam_host_update(int f64, void *W, void *M, void *V, const void *G, int S, long gstride, long n,
                           double scale, const hpnn_adam_state *s);
/* one minibatch Adam step on the CPU (FP64; k->dw, k->dv allocated: ann_adam_init): advances s,
 * mirrors t, p1, p2 into the kernel; returns the mean loss before the update */
DOUBLE hpnn_cpu_adam_step(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT b, hpnn_adam_state *s,
                          UINT *hits /* may be NULL: += argmax hits */);

/* ---- [lr_schedule] on the host (the CPU form of hpnn_amd.ops.lr_* / sgd_sched_*): the rule of
 * <libhpnn/lrsched.h> on host memory; f64 selects double, else float ---- */
/* fills a fresh state (scale 1, nothing judged, the next epoch = epoch); returns hpnn_lr_valid */
int hpnn_lr_host_init(hpnn_lr_state *s, unsigned int kind, double lr0, double gamma, unsigned int period,
                      unsigned int span, double lr_end, double lr_min, unsigned int patience, unsigned int warmup,
                      unsigned int epoch);
int hpnn_lr_host_valid(const hpnn_lr_state *s);
void hpnn_lr_host_advance(hpnn_lr_state *s);
void hpnn_lr_host_plateau(hpnn_lr_state *s, double loss_sum);
/* g = (G[0] + G[1] + ... + G[S-1]) * scale, slabs gstride elements apart, in slab order; then the
 * scheduled BP / BPM element rule with lr = (T)s->lr on W and V (V may be NULL under BP) */
void hpnn_sgd_sched_host_update(int f64, void *W, void *V, const void *G, int S, long gstride, long n, double scale,
                                double alpha, int momentum, const hpnn_lr_state *s);

/* ---- [clip] on the host (the CPU form of hpnn_amd.ops.gnorm_partials / clip_*): the rule of
 * <libhpnn/clip.h> on host memory; f64 selects double, else float ---- */
/* fills a fresh state (factor 1, counters 0); returns hpnn_clip_valid */
int hpnn_clip_host_init(hpnn_clip_state *s, double max_norm);
/* one segment: the element gs = (the slab sum, slabs 0 .. S-1 in order, or the 8-way order of the
 * BF16 plan when interleaved) * scale, gs^2 in FP64, one double per block of 1024 elements into
 * partials[] in the order of clip.h; returns the number of blocks */
long hpnn_clip_host_sumsq(int f64, int interleaved, const void *G, int S, long gstride, long n, double scale,
                          double *partials);
/* partials[0 .. count) summed in the finalize's order, then hpnn_clip_finalize */
void hpnn_clip_host_finalize(hpnn_clip_state *s, const double *partials, long count);
void hpnn_clip_host_commit(hpnn_clip_state *s, hpnn_clip_record *hist, unsigned int *cursor, unsigned int cap);
/* the update entry points with the element gs * (T)clip->factor (clip NULL: the forms above) */
void hpnn_sgd_sched_host_update_clip(int f64, void *W, void *V, const void *G, int S, long gstride, long n,
                                     double scale, double alpha, int momentum, const hpnn_lr_state *s,
                                     const hpnn_clip_state *clip);
void hpnn_adam_host_update_clip(int f64, void *W, void *M, void *V, const void *G, int S, long gstride, long n,
                                double scale, const hpnn_adam_state *s, const hpnn_clip_state *clip);
/* one clipped minibatch step on the CPU (FP64): the gradient, its global norm and the factor into
 * *clip, then BP / BPM at the rate lr (momentum: k->dw allocated) or, with adam not NULL, the Adam
 * step (advances *adam; k->dw, k->dv allocated); returns the mean loss before the update */
DOUBLE hpnn_cpu_clip_step(kernel_ann *k, nn_type type, const DOUBLE *X, const DOUBLE *T, UINT b, DOUBLE lr,
                          BOOL momentum, DOUBLE alpha, hpnn_adam_state *adam, hpnn_clip_state *clip,
                          UINT *hits /* may be NULL: += argmax hits */);

#ifdef __cplusplus
}
#endif
#endif
