/*
 * Shared option parsing for train_nn / run_nn.
 *
 * Reference flags (tests/train_nn.c:33-58, tests/run_nn.c:39-65):
 *   -h help, -v verbose (repeatable, combinable: -vvv), -x dry run
 *   (train_nn only), -O N host threads, -B N BLAS threads (accepted, no
 *   BLAS here), -S N streams per GPU.  Numeric flags take "-O4" or "-O 4".
 * Extensions: -G N GPUs, -b N minibatch (implies batched mode), -e N epochs,
 *   -m online|batched, -d f64|f32|bf16, -c force the CPU engine,
 *   -l LR learning rate, -a ALPHA momentum,
 *   -R (train_nn only) reshuffle the samples every epoch of batched training (same as
 *   [shuffle] epoch),
 *   -V N (train_nn only) validate on [test_dir] every N epochs of batched training and after
 *   the last one (same as [validate] N),
 *   -K loss|acc (train_nn only) return the state of the best validation pass (same as
 *   [keep_best]), -P P (train_nn only) stop after P passes without improvement ([patience] P),
 *   -L constant|step|linear|plateau (train_nn only) the learning-rate schedule of batched
 *   training (same as [lr_schedule]; its other keys come from the conf),
 *   -C c (train_nn only) clip the gradient of every batched step to the global norm c (same as
 *   [clip] c),
 *   -X FILE per-class metrics: sets [confusion] on and writes the confusion matrix to FILE (train_nn:
 *   of the best validation pass under -K, else of the last; run_nn: of its PASS / FAIL lines),
 *   -r FILE exact-resume state (loaded when present, written after training),
 *   -M FILE JSON-lines metrics (same as HPNN_METRICS=FILE),
 *   -T trace ranges + timing table (same as HPNN_TRACE=1).
 */
#ifndef HPNN_CLI_COMMON_H
#define HPNN_CLI_COMMON_H
#include <libhpnn.h>
#include <libhpnn/observe.h>
#include <ctype.h>
#include <string.h>
#include <stdlib.h>

typedef struct {
    const char *conf;
    int dry;
    UINT threads, blas, streams, gpus, batch, epochs;
    int mode;  /* -1 = from conf */
    int dtype; /* -1 = from conf */
    int force_cpu;
    int reshuffle; /* -R */
    unsigned validate; /* -V N */
    int keep_best;     /* -K loss|acc */
    unsigned patience; /* -P P */
    int lr_schedule;   /* -L kind; -1 = from conf */
    double clip;       /* -C c; < 0 = from conf */
    double lr, alpha;
    const char *state;   /* -r */
    const char *metrics; /* -M */
    const char *matrix;  /* -X */
    int help;
} cli_opts;

/* returns 0 on success, -1 on a syntax error */
static int cli_parse(int argc, char **argv, cli_opts *o, int allow_x) {
    memset(o, 0, sizeof(*o));
    o->conf = "./nn.conf";
    o->mode = -1;
    o->dtype = -1;
    o->lr_schedule = -1;
    o->clip = -1.0;
    o->lr = -1.0;
    o->alpha = -1.0;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        if (a[0] != '-' || a[1] == 0) {
            o->conf = a;
            continue;
        }
        for (int j = 1; a[j];) {
            char c = a[j];
            if (c == 'h') {
                o->help = 1;
                return 0;
            }
            if (c == 'v') {
                _NN(inc, verbose)();
                j++;
                continue;
            }
            if (c == 'x' && allow_x) {
                o->dry = 1;
                j++;
                continue;
            }
            if (c == 'c') {
                o->force_cpu = 1;
                j++;
                continue;
            }
            if (c == 'R' && allow_x) {
                o->reshuffle = 1;
                j++;
                continue;
            }
            if (c == 'T') {
                hpnn_trace_enable(1);
                j++;
                continue;
            }
            if (strchr("OBSGbemdlarMX", c) || (strchr("VKPLC", c) && allow_x)) {
                const char *val = a[j + 1] ? &a[j + 1] : (i + 1 < argc ? argv[++i] : NULL);
                if (!val) {
                    _OUT(stderr, "syntax error: missing -%c parameter!\n", c);
                    return -1;
                }
                if (strchr("OBSGbeVP", c)) {
                    if (!isdigit((unsigned char)*val) || atoi(val) <= 0) {
                        _OUT(stderr, "syntax error: bad -%c parameter!\n", c);
                        return -1;
                    }
                    UINT v = (UINT)atoi(val);
                    switch (c) {
                        case 'O': o->threads = v; break;
                        case 'B': o->blas = v; break;
                        case 'S': o->streams = v; break;
                        case 'G': o->gpus = v; break;
                        case 'b': o->batch = v; o->mode = NN_MODE_BATCHED; break;
                        case 'e': o->epochs = v; break;
                        case 'V': o->validate = v; break;
                        case 'P': o->patience = v; break;
                    }
                } else if (c == 'K') {
                    o->keep_best = !strcmp(val, "loss") ? NN_KEEP_LOSS : (!strcmp(val, "acc") ? NN_KEEP_ACC : -1);
                    if (o->keep_best < 0) {
                        _OUT(stderr, "syntax error: bad -K parameter (loss | acc)!\n");
                        return -1;
                    }
                } else if (c == 'L') {
                    static const char *kinds[] = {"constant", "step", "linear", "plateau"};
                    for (int q = 0; q < 4; q++)
                        if (!strcmp(val, kinds[q])) o->lr_schedule = q;
                    if (o->lr_schedule < 0) {
                        _OUT(stderr, "syntax error: bad -L parameter (constant | step | linear | plateau)!\n");
                        return -1;
                    }
                } else if (c == 'C') {
                    char *end = NULL;
                    o->clip = strtod(val, &end);
                    if (end == val || *end || !(o->clip >= 0.0) || o->clip - o->clip != 0.0) {
                        _OUT(stderr, "syntax error: bad -C parameter (a finite norm > 0; 0: off)!\n");
                        return -1;
                    }
                } else if (c == 'm') {
                    o->mode = (val[0] == 'b' || val[0] == 'B') ? NN_MODE_BATCHED : NN_MODE_ONLINE;
                } else if (c == 'd') {
                    o->dtype = !strcmp(val, "bf16") ? NN_DTYPE_BF16 : (!strcmp(val, "f32") ? NN_DTYPE_F32 : NN_DTYPE_F64);
                } else if (c == 'l') {
                    o->lr = atof(val);
                } else if (c == 'a') {
                    o->alpha = atof(val);
                } else if (c == 'r') {
                    o->state = val;
                } else if (c == 'M') {
                    o->metrics = val;
                } else if (c == 'X') {
                    o->matrix = val;
                }
                break; /* a value consumes the rest of the argument */
            }
            _OUT(stderr, "syntax error: unknown option -%c\n", c);
            return -1;
        }
    }
    return 0;
}

static void cli_apply_runtime(const cli_opts *o) {
    if (o->threads) _NN(set, omp_threads)(o->threads);
    if (o->blas) _NN(set, omp_blas)(o->blas);
    if (o->gpus) _NN(set, n_gpu)(o->gpus);
    _NN(set, cuda_streams)(o->streams ? o->streams : 1);
    if (o->dry) _NN(toggle, dry)();
    if (o->metrics) hpnn_metrics_open(o->metrics);
}

static void cli_apply_conf(const cli_opts *o, nn_def *conf) {
    if (o->mode >= 0) _NN(set, mode)(conf, (nn_mode)o->mode);
    if (o->dtype >= 0) _NN(set, dtype)(conf, (nn_dtype)o->dtype);
    if (o->batch) _NN(set, batch)(conf, o->batch);
    if (o->epochs) _NN(set, epochs)(conf, o->epochs);
    if (o->force_cpu) _NN(set, device)(conf, NN_DEVICE_CPU);
    if (o->reshuffle) _NN(set, shuffle)(conf, NN_SHUFFLE_EPOCH);
    if (o->validate) _NN(set, validate)(conf, o->validate);
    if (o->keep_best) _NN(set, keep_best)(conf, (nn_keep_best)o->keep_best);
    if (o->patience) _NN(set, patience)(conf, o->patience);
    if (o->lr_schedule >= 0) conf->lr_schedule = (nn_lr_schedule)o->lr_schedule; /* the other keys: the conf's */
    if (o->clip >= 0.0) _NN(set, clip)(conf, o->clip);
    if (o->matrix) _NN(set, confusion)(conf, TRUE);
    if (o->lr > 0) _NN(set, learning_rate)(conf, o->lr);
    if (o->alpha >= 0) _NN(set, momentum)(conf, o->alpha);
}

/* -X FILE behind a training or evaluation call that went well: the best pass's matrix when one was
 * kept, else the last.  A call that tallied nothing (online training ignores the key; after an
 * early stop without -K the GPU engine may report no last matrix) writes no file and says so: that
 * is no failure of the call.  Returns 0 unless the file could not be written */
static int cli_write_matrix(const cli_opts *o, nn_def *conf) {
    const int which = _NN(get, confusion_matrix)(conf, NN_CONFUSION_BEST, 0, NULL) ? NN_CONFUSION_BEST : NN_CONFUSION_LAST;
    if (!_NN(get, confusion_matrix)(conf, which, 0, NULL)) {
        _OUT(stderr, "-X: the call tallied no confusion matrix; %s is not written\n", o->matrix);
        return 0;
    }
    if (_NN(dump, confusion_matrix)(conf, which, o->matrix)) return 0;
    _OUT(stderr, "FAILED to write the confusion matrix to %s!\n", o->matrix);
    return -1;
}
#endif
