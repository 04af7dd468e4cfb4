/*
 * libhpnn -- MI355X-native feed-forward neural network library.
 *
 * Public C API.  Every symbol, enum value and struct name of the reference
 * header (ovhpa/hpnn include/libhpnn.h:26-215) is provided with the same
 * meaning, so a program written against libhpnn links against this library
 * unchanged.  Extensions (batched training, precision selection, learning
 * rate / momentum / epoch control, GPU selection) are appended after the
 * reference surface and never change the reference semantics.
 */
#ifndef LIBHPNN_H
#define LIBHPNN_H
#include <libhpnn/common.h>
#include <libhpnn/cg.h>
#include <libhpnn/adam.h>
#include <libhpnn/lrsched.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- capabilities (reference libhpnn.h:26-35) ---- */
typedef enum {
    NN_CAP_NONE = 0,
    NN_CAP_OMP = (1 << 0),    /* host thread pool                          */
    NN_CAP_MPI = (1 << 1),    /* multi-process (torch.distributed / RCCL)  */
    NN_CAP_CUDA = (1 << 2),   /* GPU (HIP on MI355X)                        */
    NN_CAP_CUBLAS = (1 << 3), /* never set: no vendor BLAS is used          */
    /* (1<<4) reserved (OCL in the reference) */
    NN_CAP_PBLAS = (1 << 5),  /* never set                                  */
    NN_CAP_SBLAS = (1 << 6),  /* never set                                  */
    NN_CAP_RCCL = (1 << 7),   /* extension: RCCL collectives available      */
    NN_CAP_MFMA = (1 << 8),   /* extension: gfx950 MFMA kernels loaded      */
} nn_cap;

typedef struct {
    nn_cap capability;
    SHORT nn_verbose;
    BOOL nn_dry;
    UINT nn_num_threads;
    UINT nn_num_blas;
    UINT nn_num_tasks;
    cudastreams cudas;
} nn_runtime;

/* ---- network / training types (reference libhpnn.h:51-66) ---- */
typedef enum {
    NN_TYPE_ANN = 0, /* bipolar sigmoid on every layer, MSE               */
    NN_TYPE_LNN = 1, /* sigmoid hidden + linear output (extension: works) */
    NN_TYPE_SNN = 2, /* sigmoid hidden + softmax output, cross-entropy    */
    NN_TYPE_UKN = -1,
} nn_type;

typedef enum {
    NN_TRAIN_BP = 0,
    NN_TRAIN_BPM = 1,
    NN_TRAIN_CG = 2,   /* extension: nonlinear conjugate gradient, one iteration per epoch of
                        * batched training, [dtype] f64 | f32 (<libhpnn/cg.h>; the reference
                        * parses it and implements nothing) */
    NN_TRAIN_SPLX = 3, /* parsed, not implemented (as in the reference)  */
    NN_TRAIN_ADAM = 4, /* extension: Adam / AdamW on one device in batched training, every [dtype]
                        * (<libhpnn/adam.h>) */
    NN_TRAIN_UKN = -1,
} nn_train;

/* reference hyper-parameters (libhpnn.h:67-74) */
#define BP_LEARN_RATE 0.001
#define MIN_BP_ITER 31
#define MAX_BP_ITER 102399
#define DELTA_BP 1E-6
#define BPM_LEARN_RATE 0.0005
#define MIN_BPM_ITER 15
#define MAX_BPM_ITER 102399
#define DELTA_BPM 1E-6
/* learning rate used by every GPU path and the CPU SNN path of the
 * reference (cuda_ann.cu:2094, cuda_snn.cu:1918, snn.c:799) */
#define GPU_LEARN_RATE 0.01
#define BPM_MOMENTUM 0.2
/* [train] ADAM with [lr] unset */
#define ADAM_LEARN_RATE 0.001

/* ---- extensions: execution mode and precision ---- */
typedef enum {
    NN_MODE_ONLINE = 0,  /* reference semantics: batch 1, per-sample loop */
    NN_MODE_BATCHED = 1, /* minibatch SGD / momentum, one pass per sample */
} nn_mode;

typedef enum {
    NN_DTYPE_F64 = 0,  /* FP64 everywhere (reference precision)          */
    NN_DTYPE_F32 = 1,  /* FP32 compute                                   */
    NN_DTYPE_BF16 = 2, /* BF16 MFMA, FP32 accumulate + FP32 master       */
} nn_dtype;

typedef enum {
    NN_DEVICE_AUTO = 0, /* GPU when present, else CPU                     */
    NN_DEVICE_CPU = 1,
    NN_DEVICE_GPU = 2,
} nn_device;

typedef enum {
    NN_PARALLEL_DP = 0,
    NN_PARALLEL_TP = 1,
} nn_parallel;

typedef enum {
    NN_SHUFFLE_ONCE = 0,  /* the sample order drawn once from [seed], replayed every epoch */
    NN_SHUFFLE_EPOCH = 1, /* a new order every epoch of batched training (libhpnn/shuffle.h) */
} nn_shuffle;

typedef enum {
    NN_KEEP_OFF = 0,  /* the weights after the last epoch are returned */
    NN_KEEP_LOSS = 1, /* those of the validation pass with the smallest loss */
    NN_KEEP_ACC = 2,  /* those of the pass with the most hits (the loss breaks ties) */
} nn_keep_best;

/* [lr_schedule]: the learning rate of every epoch of batched training on one device
 * (<libhpnn/lrsched.h>; the values are HPNN_LR_*) */
typedef enum {
    NN_LR_NONE = -1,    /* not set: [lr] for the whole call */
    NN_LR_CONSTANT = 0, /* [lr] (with [warmup]: the ramp, then [lr]) */
    NN_LR_STEP = 1,     /* [lr] * [lr_gamma]^(epoch / [lr_period]) */
    NN_LR_LINEAR = 2,   /* from [lr] to [lr_end] over [lr_span] epochs, then [lr_end] */
    NN_LR_PLATEAU = 3,  /* * [lr_gamma] after [lr_patience] validation passes without a smaller loss,
                         * not below [lr_min] (needs [validate]) */
} nn_lr_schedule;

typedef struct {
    nn_runtime *rr;  /* link to the runtime parameters */
    CHAR *name;
    nn_type type;
    BOOL need_init;
    UINT seed;
    void *kernel;    /* kernel_ann* */
    CHAR *f_kernel;
    nn_train train;
    CHAR *samples;
    CHAR *tests;
    /* -- extensions (optional conf keys, see docs/FORMATS.md) -- */
    nn_mode mode;
    nn_dtype dtype;
    nn_device device;
    UINT batch;      /* minibatch size in batched mode (default 256) */
    UINT epochs;     /* passes over the sample directory (default 1) */
    DOUBLE lr;       /* <=0: reference default for the path          */
    DOUBLE momentum; /* <0 : reference default 0.2                   */
    /* -- training progress (exact resume, nn_dump_state / nn_load_state) -- */
    UINT epochs_done;    /* batched epochs completed on this kernel       */
    UINT64 samples_seen; /* training samples processed on this kernel     */
    BOOL resume;         /* start batched training from the saved momentum */
    /* -- batched multi-GPU layout: [parallel] dp (replicas) | tp (rows of every hidden
     *    layer sharded over the GPUs / ranks; [dtype] f64 or f32) -- */
    nn_parallel parallel;
    /* -- batched sample order: [shuffle] once (default) | epoch -- */
    nn_shuffle shuffle;
    /* -- [validate] N: batched training evaluates [test_dir] every N epochs (0: off); the
     *    records of the last nn_train_kernel call (nn_get_validation) -- */
    UINT validate;
    UINT n_validation;
    void *validation;
    /* -- [keep_best] loss | acc, [patience] P: batched training returns the state of its best
     *    validation pass and stops after P passes without improvement; the best record of the
     *    last nn_train_kernel call (nn_get_best; best_epoch 0: none) -- */
    nn_keep_best keep_best;
    UINT patience;
    UINT best_epoch;
    DOUBLE best_loss;
    UINT best_correct;
    UINT best_n;
    /* -- [train] CG: the records of the last nn_train_kernel call, one per iteration
     *    (nn_get_cg_history) -- */
    UINT n_cg_history;
    void *cg_history;
    /* -- [train] ADAM: [beta1], [beta2], [epsilon], [decay]; a NaN: not set (0.9, 0.999, 1e-8, 0) -- */
    DOUBLE beta1, beta2, epsilon, decay;
    /* -- [lr_schedule] constant | step | linear | plateau with [lr_gamma], [lr_period], [lr_span],
     *    [lr_end], [lr_min], [lr_patience], [warmup] (<libhpnn/lrsched.h>); NN_LR_NONE, a NaN and 0:
     *    not set; the rate of every epoch of the last nn_train_kernel call (nn_get_lr_history) -- */
    nn_lr_schedule lr_schedule;
    DOUBLE lr_gamma, lr_end, lr_min;
    UINT lr_period, lr_span, lr_patience, warmup;
    UINT n_lr_history;
    DOUBLE *lr_history;
    /* -- [clip] c: batched training rescales the gradient of a step whose global L2 norm exceeds c
     *    (<libhpnn/clip.h>); 0: off; one record per epoch of the last nn_train_kernel call
     *    (nn_get_clip_history) -- */
    DOUBLE clip;
    UINT n_clip_history;
    void *clip_history;
    /* -- [confusion] on | off: every validation pass of batched training, and nn_run_kernel, also
     *    tally the confusion matrix (<libhpnn/confusion.h>); of the last call: the classes, one
     *    per-class record (3 n_classes words) per validation record, the matrix of the last pass
     *    and of the best one (NULL: none), the tally launches the GPU driver issued
     *    (nn_get_confusion_matrix, nn_get_class_history) -- */
    int confusion;
    UINT n_classes;
    UINT n_class_history;
    UINT *class_history;
    UINT *confusion_last;
    UINT *confusion_best;
    UINT confusion_launches;
} nn_def;

#define _NN(a, b) nn_##a##_##b

/* logging (reference libhpnn.h:95-122) */
#define NN_DBG(_file, ...)                                                 \
    do {                                                                   \
        if ((_NN(return, verbose)()) > 2) {                                \
            _OUT((_file), "NN(DBG): ");                                   \
            _OUT((_file), __VA_ARGS__);                                    \
        }                                                                  \
    } while (0)
#define NN_OUT(_file, ...)                                                 \
    do {                                                                   \
        if ((_NN(return, verbose)()) > 1) {                                \
            _OUT((_file), "NN: ");                                        \
            _OUT((_file), __VA_ARGS__);                                    \
        }                                                                  \
    } while (0)
#define NN_COUT(_file, ...)                                                \
    do {                                                                   \
        if ((_NN(return, verbose)()) > 1) { _OUT((_file), __VA_ARGS__); }  \
    } while (0)
#define NN_WARN(_file, ...)                                                \
    do {                                                                   \
        if ((_NN(return, verbose)()) > 0) {                                \
            _OUT((_file), "NN(WARN): ");                                  \
            _OUT((_file), __VA_ARGS__);                                    \
        }                                                                  \
    } while (0)
#define NN_ERROR(_file, ...)                                               \
    do {                                                                   \
        _OUT((_file), "NN(ERR): ");                                       \
        _OUT((_file), __VA_ARGS__);                                        \
    } while (0)
#define NN_WRITE _OUT

/* ---- library init / runtime ---- */
void _NN(inc, verbose)(void);
void _NN(dec, verbose)(void);
void _NN(set, verbose)(SHORT verbosity);
void _NN(get, verbose)(SHORT *verbosity);
SHORT _NN(return, verbose)(void);
void _NN(toggle, dry)(void);
BOOL _NN(return, dry)(void);
void _NN(get, capabilities)(nn_cap *capabilities);
void _NN(unset, capability)(nn_cap capability);
nn_cap _NN(return, capabilities)(void);
BOOL _NN(init, OMP)(void);
BOOL _NN(init, MPI)(void);
BOOL _NN(init, CUDA)(void);
BOOL _NN(init, BLAS)(void);
int _NN(init, all)(UINT init_verbose);
BOOL _NN(deinit, OMP)(void);
BOOL _NN(deinit, MPI)(void);
BOOL _NN(deinit, CUDA)(void);
BOOL _NN(deinit, BLAS)(void);
int _NN(deinit, all)(void);

BOOL _NN(set, omp_threads)(UINT n_threads);
BOOL _NN(get, omp_threads)(UINT *n_threads);
int _NN(return, omp_threads)(void);
BOOL _NN(set, mpi_tasks)(UINT n_tasks);
BOOL _NN(get, mpi_tasks)(UINT *n_tasks);
BOOL _NN(get, curr_mpi_task)(UINT *task);
BOOL _NN(set, n_gpu)(UINT n_gpu);
BOOL _NN(get, n_gpu)(UINT *n_gpu);
BOOL _NN(set, cuda_streams)(UINT n_streams);
BOOL _NN(get, cuda_streams)(UINT *n_streams);
BOOL _NN(set, omp_blas)(UINT n_blas);
BOOL _NN(get, omp_blas)(UINT *n_blas);
cudastreams *_NN(return, cudas)(void);

/* ---- configuration ---- */
void _NN(init, conf)(nn_def *conf);
void _NN(deinit, conf)(nn_def *conf);
void _NN(set, name)(nn_def *conf, const CHAR *name);
void _NN(get, name)(nn_def *conf, CHAR **name);
char *_NN(return, name)(nn_def *conf);
void _NN(set, type)(nn_def *conf, nn_type type);
void _NN(get, type)(nn_def *conf, nn_type *type);
nn_type _NN(return, type)(nn_def *conf);
void _NN(set, need_init)(nn_def *conf, BOOL need_init);
void _NN(get, need_init)(nn_def *conf, BOOL *need_init);
BOOL _NN(return, need_init)(nn_def *conf);
void _NN(set, seed)(nn_def *conf, UINT seed);
void _NN(get, seed)(nn_def *conf, UINT *seed);
UINT _NN(return, seed)(nn_def *conf);
void _NN(set, kernel_filename)(nn_def *conf, CHAR *f_kernel);
void _NN(get, kernel_filename)(nn_def *conf, CHAR **f_kernel);
char *_NN(return, kernel_filename)(nn_def *conf);
void _NN(set, train)(nn_def *conf, nn_train train);
void _NN(get, train)(nn_def *conf, nn_train *train);
nn_train _NN(return, train)(nn_def *conf);
void _NN(set, samples_directory)(nn_def *conf, CHAR *samples);
void _NN(get, samples_directory)(nn_def *conf, CHAR **samples);
char *_NN(return, samples_directory)(nn_def *conf);
void _NN(set, tests_directory)(nn_def *conf, CHAR *tests);
void _NN(get, tests_directory)(nn_def *conf, CHAR **tests);
char *_NN(return, tests_directory)(nn_def *conf);
nn_def *_NN(load, conf)(const CHAR *filename);
void _NN(dump, conf)(nn_def *conf, FILE *fp);

/* ---- kernel (weights) ---- */
void _NN(free, kernel)(nn_def *conf);
BOOL _NN(generate, kernel)(nn_def *conf, ...);
BOOL _NN(load, kernel)(nn_def *conf);
void _NN(dump, kernel)(nn_def *conf, FILE *output);

UINT _NN(get, n_inputs)(nn_def *conf);
UINT _NN(get, n_hiddens)(nn_def *conf);
UINT _NN(get, n_outputs)(nn_def *conf);
UINT _NN(get, h_neurons)(nn_def *conf, UINT layer);

/* ---- samples / execution ---- */
BOOL _NN(read, sample)(CHAR *filename, DOUBLE **in, DOUBLE **out);
BOOL _NN(train, kernel)(nn_def *conf);
void _NN(run, kernel)(nn_def *conf);

/* ---- extensions ---- */
void _NN(set, mode)(nn_def *conf, nn_mode mode);
nn_mode _NN(return, mode)(nn_def *conf);
void _NN(set, dtype)(nn_def *conf, nn_dtype dtype);
nn_dtype _NN(return, dtype)(nn_def *conf);
void _NN(set, device)(nn_def *conf, nn_device device);
nn_device _NN(return, device)(nn_def *conf);
void _NN(set, batch)(nn_def *conf, UINT batch);
UINT _NN(return, batch)(nn_def *conf);
void _NN(set, epochs)(nn_def *conf, UINT epochs);
UINT _NN(return, epochs)(nn_def *conf);
void _NN(set, learning_rate)(nn_def *conf, DOUBLE lr);
DOUBLE _NN(return, learning_rate)(nn_def *conf);
void _NN(set, momentum)(nn_def *conf, DOUBLE alpha);
DOUBLE _NN(return, momentum)(nn_def *conf);
/* batched sample order: once (default) or a new permutation every epoch */
void _NN(set, shuffle)(nn_def *conf, nn_shuffle shuffle);
void _NN(get, shuffle)(nn_def *conf, nn_shuffle *shuffle);
nn_shuffle _NN(return, shuffle)(nn_def *conf);
/* [validate] N: batched training evaluates the held-out set ([test_dir], a directory or a pack
 * file, in name order) forward-only after every epoch whose absolute number is a multiple of
 * N and after the last epoch of the call; 0 = off.  nn_train_kernel prints one
 * "VALIDATION: epoch E loss=L acc=C/N" line per pass and keeps the records for
 * nn_get_validation: up to max records of the last call into the arrays (any may be NULL),
 * returns the number of records the call made */
void _NN(set, validate)(nn_def *conf, UINT every);
void _NN(get, validate)(nn_def *conf, UINT *every);
UINT _NN(return, validate)(nn_def *conf);
UINT _NN(get, validation)(nn_def *conf, UINT max, UINT *epoch, DOUBLE *loss, UINT *correct, UINT *n);
/* [keep_best] loss | acc (needs [validate]): nn_train_kernel returns the kernel exactly as it was
 * after the epoch of its best validation pass -- weights, momentum, epochs_done -- so the call is
 * indistinguishable from one given that many epochs.  loss: the pass with the smallest loss; acc:
 * the most hits, the loss breaking ties; ties do not improve, a NaN loss is never the smallest.
 * The best is per call.  [patience] P (needs [keep_best]; 0 = never): training stops at the pass
 * at which P passes in a row have not improved.  nn_train_kernel prints "BEST: epoch E loss=L
 * acc=C/N" and, after a stop, "EARLY STOP: epoch E (no improvement in P passes)"; nn_get_best
 * returns the record of the last call (any pointer may be NULL), FALSE when there is none */
void _NN(set, keep_best)(nn_def *conf, nn_keep_best keep);
void _NN(get, keep_best)(nn_def *conf, nn_keep_best *keep);
nn_keep_best _NN(return, keep_best)(nn_def *conf);
void _NN(set, patience)(nn_def *conf, UINT passes);
void _NN(get, patience)(nn_def *conf, UINT *passes);
UINT _NN(return, patience)(nn_def *conf);
BOOL _NN(get, best)(nn_def *conf, UINT *epoch, DOUBLE *loss, UINT *correct, UINT *n);
/* [train] CG (batched mode, [dtype] f64 | f32, one device): every epoch is one nonlinear
 * conjugate-gradient iteration over the whole sample set -- Polak-Ribiere+ direction, a line
 * search of six fixed trials a_init 2^(j-2) and a parabola point, all forward-only
 * (<libhpnn/cg.h>).  [batch] is the chunk the gradient is accumulated in, [lr] the first a_init
 * of a call, [momentum] is unused.  The direction and a_init live for one call: a resumed run
 * continues epochs_done and starts with a steepest-descent iteration.  nn_train_kernel prints
 * "CG: epoch E loss=L beta=B alpha=A trial=j" per iteration; nn_get_cg_history returns the
 * records of the last call (owned by conf; *n = their number, NULL when there is none) */
const hpnn_cg_record *_NN(get, cg_history)(nn_def *conf, UINT *n);
/* [train] ADAM (batched mode, one device): W += c1 m / (sqrt(v) / s2 + eps) with the moments
 * m, v of the mean gradient and the bias corrections of <libhpnn/adam.h>; decay > 0 is the
 * decoupled weight decay of AdamW.  [lr] defaults to ADAM_LEARN_RATE, [momentum] is unused.  A NaN
 * argument of nn_set_adam unsets that key (its default); nn_get_adam returns the values a
 * training call would use (any pointer may be NULL).  0 <= beta < 1, epsilon > 0 and
 * decay >= 0 are checked by nn_train_kernel.  The moments and the step count persist through
 * the state file (nn_dump_state / nn_load_state), not across two calls in one process */
void _NN(set, adam)(nn_def *conf, DOUBLE beta1, DOUBLE beta2, DOUBLE epsilon, DOUBLE decay);
void _NN(get, adam)(nn_def *conf, DOUBLE *beta1, DOUBLE *beta2, DOUBLE *epsilon, DOUBLE *decay);
/* [lr_schedule] (batched mode, one device, BP / BPM / ADAM): the rate of epoch e (absolute, 0-based)
 * is a function of e and, for plateau, of the validation losses (<libhpnn/lrsched.h>); [warmup] W
 * multiplies the first W epochs' rates by (e + 1) / W and composes with every kind (alone it
 * schedules a constant rate).  There is no cosine form: the rule uses only operations that are
 * correctly rounded on the host and on the device.  nn_set_lr_schedule: a NaN gamma / lr_end /
 * lr_min and a 0 period / span / patience unset that key (defaults 0.5, 0, 0, 10, none, 2);
 * nn_get_lr_schedule returns the values a training call would use (any pointer may be NULL).
 * step and linear continue through nn_load_state with nothing stored; plateau's running state
 * persists through the state file, not across two calls in one process.  nn_train_kernel prints
 * "LR: epoch E lr=X" per epoch at -vv; nn_get_lr_history returns the rates of the last call (owned
 * by conf; *n = their number, NULL when there is none) */
void _NN(set, lr_schedule)(nn_def *conf, nn_lr_schedule kind, DOUBLE gamma, UINT period, UINT span, DOUBLE lr_end,
                           DOUBLE lr_min, UINT patience, UINT warmup);
void _NN(get, lr_schedule)(nn_def *conf, nn_lr_schedule *kind, DOUBLE *gamma, UINT *period, UINT *span,
                           DOUBLE *lr_end, DOUBLE *lr_min, UINT *patience, UINT *warmup);
const DOUBLE *_NN(get, lr_history)(nn_def *conf, UINT *n);
/* [clip] c (batched mode, one device or the CPU engine, BP / BPM / ADAM, any [dtype], with or
 * without [lr_schedule]): when the L2 norm of the whole net's minibatch gradient exceeds c the
 * gradient is multiplied by c / norm before the update rule sees it (<libhpnn/clip.h>: a
 * deterministic FP64 reduction in a fixed order, the same bits on the host and on the device).
 * c must be finite and >= 0; 0 or an absent key: off.  Nothing is carried from step to step, so
 * the state file does not change and -r resumes exactly.  [train] CG and the multi-GPU engines
 * refuse [clip]; online mode ignores it with one warning.  The log has one "gradient clipping:
 * max norm c" line and "CLIP: epoch E steps=N clipped=M max_norm=X last_norm=Y" per epoch at -vv;
 * nn_get_clip_history returns the records of the last call (owned by conf; *n = 0: none). */
typedef struct {
    UINT steps, clipped;         /* the steps of the epoch and those whose gradient was rescaled */
    DOUBLE norm_max, norm_last;  /* the largest and the last gradient norm of the epoch */
} nn_clip_record;
void _NN(set, clip)(nn_def *conf, DOUBLE max_norm);
DOUBLE _NN(get, clip)(nn_def *conf);
const nn_clip_record *_NN(get, clip_history)(nn_def *conf, UINT *n);
/* [confusion] on | off: per-class validation metrics (<libhpnn/confusion.h>).  In batched training
 * (one device or the CPU engine; needs [validate]) every validation pass also tallies its confusion
 * matrix M[n_out][n_out + 1] -- M[t][g] = held-out samples of target class t guessed g, column
 * n_out ("none") the rows in which no output compared -- on the device, inside the captured
 * epochs; nn_train_kernel prints "CLASSES: epoch E bacc=B worst=c recall=h/s" behind every
 * "VALIDATION:" line (B the balanced accuracy, c the supported class of lowest recall, lowest index
 * on ties).  nn_run_kernel tallies the (truth, guess) pairs of its PASS / FAIL lines.  Online
 * training ignores the key with one warning.
 * nn_get_confusion_matrix: which = NN_CONFUSION_LAST (the last pass reported, or the last
 * nn_run_kernel call) | NN_CONFUSION_BEST (the pass [keep_best] kept); copies at most max_cells
 * cells (row-major, n_out (n_out + 1) of them) and returns n_out, 0 when there is nothing to report
 * (after an early stop the GPU engine may have validated past the stopping pass: it then reports
 * no last matrix).  nn_get_class_history: support (row sums), hit (diagonal) and predicted (column
 * sums) of validation pass `pass` of the last nn_train_kernel call, n_out words each (any pointer
 * may be NULL); returns n_out, 0 when there is no such pass. */
#define NN_CONFUSION_LAST 0
#define NN_CONFUSION_BEST 1
void _NN(set, confusion)(nn_def *conf, BOOL on);
void _NN(get, confusion)(nn_def *conf, BOOL *on);
BOOL _NN(return, confusion)(nn_def *conf);
UINT _NN(get, confusion_matrix)(nn_def *conf, int which, UINT max_cells, UINT *cells);
UINT _NN(get, class_history)(nn_def *conf, UINT pass, UINT *support, UINT *hit, UINT *predicted);
/* the tally launches the last nn_train_kernel call issued on the GPU: a launch captured into an
 * epoch graph counts once, however often the graph is replayed (0 with the key off) */
UINT _NN(return, confusion_launches)(nn_def *conf);
/* the matrix as text: "# n_out", then one line per target class with n_out + 1 counts */
BOOL _NN(dump, confusion_matrix)(nn_def *conf, int which, const CHAR *filename);
/* the [shuffle] epoch permutation (libhpnn/shuffle.h): out[i] = index, in the order drawn once
 * from [seed], of the sample at position i of epoch `epoch` (epochs completed before it) */
void hpnn_epoch_perm(UINT n, UINT seed, UINT epoch, UINT *out);
/* write the kernel with %.17g (bit-exact round trip) instead of %17.15f */
void _NN(dump, kernel_exact)(nn_def *conf, FILE *output);
/* number of accurate predictions of the last nn_run_kernel call */
UINT _NN(return, last_pass)(void);
UINT _NN(return, last_total)(void);
/* library version string */
const char *_NN(return, version)(void);
/* exact training state sidecar (bit-exact FP64 weights, momentum, seed, progress,
 * checksum): kernel.opt stays the interchange format, the state file resumes exactly */
BOOL _NN(dump, state)(nn_def *conf, const CHAR *filename);
BOOL _NN(load, state)(nn_def *conf, const CHAR *filename);
UINT _NN(return, epochs_done)(nn_def *conf);
/* pack a directory of sample files into one binary file; train / run accept a pack
 * file wherever a sample or test directory is expected */
BOOL _NN(pack, samples)(const CHAR *dir, const CHAR *filename);
/* the same file from n records in memory (X: n x n_in, T: n x n_out, row-major) */
BOOL _NN(pack, arrays)(const CHAR *filename, const DOUBLE *X, const DOUBLE *T, UINT n, UINT n_in, UINT n_out);

#ifdef __cplusplus
}
#endif
#endif /* LIBHPNN_H */
