/*
 * libhpnn C API: configuration, kernel management, sample I/O and the
 * train / run workflows.
 *
 * Parity map (reference src/libhpnn.c):
 *   conf setters/getters          :544-657
 *   nn_load_conf / nn_dump_conf   :658-937  (same keys; values are read
 *                                  after the closing ']' so both "[input]"
 *                                  and the dumped "[inputs]" parse)
 *   kernel generate/load/dump     :941-1009
 *   accessors                     :1013-1066 (work for generated kernels
 *                                  too; the reference returned 0 there)
 *   nn_read_sample                :1070-1145
 *   nn_train_kernel               :1149-1302 (same file walk, same seeded
 *                                  permutation, same log lines; the file
 *                                  list is sorted first so the order does
 *                                  not depend on readdir, and the
 *                                  random()*n/RAND_MAX == n overflow is
 *                                  rejected instead of indexing past the end)
 *   nn_run_kernel                 :1306-1536
 * Extensions: batched training on the CPU (FP64) or the GPU, and the conf keys that go with it.
 * Every conf key, the reference's and the extensions', is one row of CONF_KEYS (conf_keys.h): the
 * row is what nn_load_conf reads the key with and what nn_dump_conf writes it with.
 */
#include <libhpnn/ann.h>
#include <ctype.h>
#include <dirent.h>
#include <math.h>
#include <stdarg.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <string>
#include <vector>

#include <libhpnn/observe.h>
#include <omp.h>

#include "conf_keys.h"
#include "dataset.h"
#include "export_records.h"
#include "lr_running.h"
#include "runtime_internal.h"
#include "../gpu/engine.h"

#define KERN(conf) ((kernel_ann *)((conf)->kernel))

static UINT g_last_pass = 0, g_last_total = 0;

/* ------------------------------------------------------------------ */
/* configuration                                                       */
/* ------------------------------------------------------------------ */
extern "C" void _NN(init, conf)(nn_def *conf) {
    memset(conf, 0, sizeof(*conf));
    conf->rr = hpnn_rt_get();
    conf->type = NN_TYPE_UKN;
    conf->train = NN_TRAIN_UKN;
    conf->need_init = FALSE;
    conf->seed = 0;
    conf->mode = NN_MODE_ONLINE;
    conf->dtype = NN_DTYPE_F64;
    conf->device = NN_DEVICE_AUTO;
    conf->batch = 256;
    conf->epochs = 1;
    conf->lr = -1.0;
    conf->momentum = -1.0;
    conf->beta1 = conf->beta2 = conf->epsilon = conf->decay = NAN; /* not set */
    conf->lr_schedule = NN_LR_NONE;
    conf->lr_gamma = conf->lr_end = conf->lr_min = NAN; /* not set */
}

/* The per-epoch histories of the last nn_train_kernel call ([validate], [train] CG, [lr_schedule],
 * [clip]): malloc'ed by the engine, owned by the conf from adopt_histories until drop_histories. */
template <class T>
static void drop(T *&array, UINT &count) {
    free(array);
    array = NULL;
    count = 0;
}

/* [confusion]: what the last nn_train_kernel or nn_run_kernel call tallied */
static void drop_confusion(nn_def *conf) {
    UINT cells = 0;
    drop(conf->class_history, conf->n_class_history);
    drop(conf->confusion_last, cells);
    drop(conf->confusion_best, cells);
    conf->n_classes = conf->confusion_launches = 0;
}

static void drop_histories(nn_def *conf) {
    drop(conf->validation, conf->n_validation);
    drop(conf->cg_history, conf->n_cg_history);
    drop(conf->lr_history, conf->n_lr_history);
    drop(conf->clip_history, conf->n_clip_history);
    drop_confusion(conf);
}

static void adopt_histories(nn_def *conf, const hpnn_batched_stats *st) {
    drop_histories(conf);
    conf->validation = st->val;
    conf->n_validation = st->n_val;
    conf->cg_history = st->cg;
    conf->n_cg_history = st->n_cg;
    conf->lr_history = st->lr_hist;
    conf->n_lr_history = st->n_lr;
    conf->clip_history = st->clip_hist;
    conf->n_clip_history = st->n_clip;
    conf->n_classes = st->n_classes;
    conf->class_history = st->class_hist;
    conf->n_class_history = st->n_class_hist;
    conf->confusion_last = st->confusion_last;
    conf->confusion_best = st->confusion_best;
    conf->confusion_launches = st->confusion_launches;
}

extern "C" void _NN(free, kernel)(nn_def *conf) {
    if (!conf || !conf->kernel) return;
    ann_kernel_free(KERN(conf));
    conf->kernel = NULL;
}

extern "C" void _NN(deinit, conf)(nn_def *conf) {
    if (!conf) return;
    _NN(free, kernel)(conf);
    free(conf->name);
    free(conf->f_kernel);
    free(conf->samples);
    free(conf->tests);
    drop_histories(conf);
    conf->name = conf->f_kernel = conf->samples = conf->tests = NULL;
}

extern "C" void _NN(set, name)(nn_def *c, const CHAR *n) {
    set_str(&c->name, n);
    if (c->kernel) set_str(&KERN(c)->name, n);
}
extern "C" void _NN(get, name)(nn_def *c, CHAR **n) { *n = c->name ? strdup(c->name) : NULL; }
extern "C" char *_NN(return, name)(nn_def *c) { return c->name; }
extern "C" void _NN(set, type)(nn_def *c, nn_type t) { c->type = t; }
extern "C" void _NN(get, type)(nn_def *c, nn_type *t) { *t = c->type; }
extern "C" nn_type _NN(return, type)(nn_def *c) { return c->type; }
extern "C" void _NN(set, need_init)(nn_def *c, BOOL v) { c->need_init = v; }
extern "C" void _NN(get, need_init)(nn_def *c, BOOL *v) { *v = c->need_init; }
extern "C" BOOL _NN(return, need_init)(nn_def *c) { return c->need_init; }
extern "C" void _NN(set, seed)(nn_def *c, UINT s) { c->seed = s; }
extern "C" void _NN(get, seed)(nn_def *c, UINT *s) { *s = c->seed; }
extern "C" UINT _NN(return, seed)(nn_def *c) { return c->seed; }
extern "C" void _NN(set, kernel_filename)(nn_def *c, CHAR *f) { set_str(&c->f_kernel, f); }
extern "C" void _NN(get, kernel_filename)(nn_def *c, CHAR **f) { *f = c->f_kernel ? strdup(c->f_kernel) : NULL; }
extern "C" char *_NN(return, kernel_filename)(nn_def *c) { return c->f_kernel; }
extern "C" void _NN(set, train)(nn_def *c, nn_train t) { c->train = t; }
extern "C" void _NN(get, train)(nn_def *c, nn_train *t) { *t = c->train; }
extern "C" nn_train _NN(return, train)(nn_def *c) { return c->train; }
extern "C" void _NN(set, samples_directory)(nn_def *c, CHAR *s) { set_str(&c->samples, s); }
extern "C" void _NN(get, samples_directory)(nn_def *c, CHAR **s) { *s = c->samples ? strdup(c->samples) : NULL; }
extern "C" char *_NN(return, samples_directory)(nn_def *c) { return c->samples; }
extern "C" void _NN(set, tests_directory)(nn_def *c, CHAR *s) { set_str(&c->tests, s); }
extern "C" void _NN(get, tests_directory)(nn_def *c, CHAR **s) { *s = c->tests ? strdup(c->tests) : NULL; }
extern "C" char *_NN(return, tests_directory)(nn_def *c) { return c->tests; }
extern "C" void _NN(set, mode)(nn_def *c, nn_mode m) { c->mode = m; }
extern "C" nn_mode _NN(return, mode)(nn_def *c) { return c->mode; }
extern "C" void _NN(set, dtype)(nn_def *c, nn_dtype d) { c->dtype = d; }
extern "C" nn_dtype _NN(return, dtype)(nn_def *c) { return c->dtype; }
extern "C" void _NN(set, shuffle)(nn_def *c, nn_shuffle v) { c->shuffle = v == NN_SHUFFLE_EPOCH ? NN_SHUFFLE_EPOCH : NN_SHUFFLE_ONCE; }
extern "C" void _NN(get, shuffle)(nn_def *c, nn_shuffle *v) { *v = c->shuffle; }
extern "C" nn_shuffle _NN(return, shuffle)(nn_def *c) { return c->shuffle; }
extern "C" void _NN(set, validate)(nn_def *c, UINT v) { c->validate = v; }
extern "C" void _NN(get, validate)(nn_def *c, UINT *v) { *v = c->validate; }
extern "C" UINT _NN(return, validate)(nn_def *c) { return c->validate; }
extern "C" UINT _NN(get, validation)(nn_def *c, UINT max, UINT *epoch, DOUBLE *loss, UINT *correct, UINT *n) {
    if (!c) return 0;
    const hpnn_validation_record *r = (const hpnn_validation_record *)c->validation;
    for (UINT i = 0; r && i < c->n_validation && i < max; i++) {
        if (epoch) epoch[i] = r[i].epoch;
        if (loss) loss[i] = r[i].loss;
        if (correct) correct[i] = r[i].correct;
        if (n) n[i] = r[i].n;
    }
    return r ? c->n_validation : 0;
}
extern "C" const hpnn_cg_record *_NN(get, cg_history)(nn_def *c, UINT *n) {
    if (n) *n = c && c->cg_history ? c->n_cg_history : 0;
    return c ? (const hpnn_cg_record *)c->cg_history : NULL;
}
extern "C" void _NN(set, keep_best)(nn_def *c, nn_keep_best v) {
    c->keep_best = (v == NN_KEEP_LOSS || v == NN_KEEP_ACC) ? v : NN_KEEP_OFF;
}
extern "C" void _NN(get, keep_best)(nn_def *c, nn_keep_best *v) { *v = c->keep_best; }
extern "C" nn_keep_best _NN(return, keep_best)(nn_def *c) { return c->keep_best; }
extern "C" void _NN(set, patience)(nn_def *c, UINT v) { c->patience = v; }
extern "C" void _NN(get, patience)(nn_def *c, UINT *v) { *v = c->patience; }
extern "C" UINT _NN(return, patience)(nn_def *c) { return c->patience; }
extern "C" BOOL _NN(get, best)(nn_def *c, UINT *epoch, DOUBLE *loss, UINT *correct, UINT *n) {
    if (!c || !c->best_epoch) return FALSE;
    if (epoch) *epoch = c->best_epoch;
    if (loss) *loss = c->best_loss;
    if (correct) *correct = c->best_correct;
    if (n) *n = c->best_n;
    return TRUE;
}
extern "C" void _NN(set, device)(nn_def *c, nn_device d) { c->device = d; }
extern "C" nn_device _NN(return, device)(nn_def *c) { return c->device; }
extern "C" void _NN(set, batch)(nn_def *c, UINT b) { c->batch = b ? b : 1; }
extern "C" UINT _NN(return, batch)(nn_def *c) { return c->batch; }
extern "C" void _NN(set, epochs)(nn_def *c, UINT e) { c->epochs = e ? e : 1; }
extern "C" UINT _NN(return, epochs)(nn_def *c) { return c->epochs; }
extern "C" void _NN(set, learning_rate)(nn_def *c, DOUBLE lr) { c->lr = lr; }
extern "C" DOUBLE _NN(return, learning_rate)(nn_def *c) { return c->lr; }
extern "C" void _NN(set, momentum)(nn_def *c, DOUBLE a) { c->momentum = a; }
extern "C" DOUBLE _NN(return, momentum)(nn_def *c) { return c->momentum; }
extern "C" void _NN(set, adam)(nn_def *c, DOUBLE beta1, DOUBLE beta2, DOUBLE epsilon, DOUBLE decay) {
    if (!c) return;
    c->beta1 = beta1;
    c->beta2 = beta2;
    c->epsilon = epsilon;
    c->decay = decay;
}
extern "C" void _NN(get, adam)(nn_def *c, DOUBLE *beta1, DOUBLE *beta2, DOUBLE *epsilon, DOUBLE *decay) {
    if (!c) return;
    if (beta1) *beta1 = c->beta1 == c->beta1 ? c->beta1 : HPNN_ADAM_BETA1;
    if (beta2) *beta2 = c->beta2 == c->beta2 ? c->beta2 : HPNN_ADAM_BETA2;
    if (epsilon) *epsilon = c->epsilon == c->epsilon ? c->epsilon : HPNN_ADAM_EPS;
    if (decay) *decay = c->decay == c->decay ? c->decay : 0.0;
}
extern "C" void _NN(set, lr_schedule)(nn_def *c, nn_lr_schedule kind, DOUBLE gamma, UINT period, UINT span,
                                      DOUBLE lr_end, DOUBLE lr_min, UINT patience, UINT warmup) {
    if (!c) return;
    c->lr_schedule = (kind >= NN_LR_CONSTANT && kind <= NN_LR_PLATEAU) ? kind : NN_LR_NONE;
    c->lr_gamma = gamma;
    c->lr_period = period;
    c->lr_span = span;
    c->lr_end = lr_end;
    c->lr_min = lr_min;
    c->lr_patience = patience;
    c->warmup = warmup;
}
extern "C" void _NN(get, lr_schedule)(nn_def *c, nn_lr_schedule *kind, DOUBLE *gamma, UINT *period, UINT *span,
                                      DOUBLE *lr_end, DOUBLE *lr_min, UINT *patience, UINT *warmup) {
    if (!c) return;
    /* [warmup] alone schedules a constant rate */
    if (kind) *kind = (c->lr_schedule == NN_LR_NONE && c->warmup) ? NN_LR_CONSTANT : c->lr_schedule;
    if (gamma) *gamma = c->lr_gamma == c->lr_gamma ? c->lr_gamma : HPNN_LR_GAMMA;
    if (period) *period = c->lr_period ? c->lr_period : HPNN_LR_PERIOD;
    if (span) *span = c->lr_span;
    if (lr_end) *lr_end = c->lr_end == c->lr_end ? c->lr_end : 0.0;
    if (lr_min) *lr_min = c->lr_min == c->lr_min ? c->lr_min : 0.0;
    if (patience) *patience = c->lr_patience ? c->lr_patience : HPNN_LR_PATIENCE;
    if (warmup) *warmup = c->warmup;
}
extern "C" void _NN(set, clip)(nn_def *c, DOUBLE max_norm) {
    if (c) c->clip = max_norm;
}
extern "C" DOUBLE _NN(get, clip)(nn_def *c) { return c ? c->clip : 0.0; }
extern "C" const nn_clip_record *_NN(get, clip_history)(nn_def *c, UINT *n) {
    if (n) *n = c && c->clip_history ? c->n_clip_history : 0;
    return c ? (const nn_clip_record *)c->clip_history : NULL;
}
extern "C" void _NN(set, confusion)(nn_def *c, BOOL on) {
    if (c) c->confusion = on ? 1 : 0;
}
extern "C" void _NN(get, confusion)(nn_def *c, BOOL *on) {
    if (c && on) *on = c->confusion ? TRUE : FALSE;
}
extern "C" BOOL _NN(return, confusion)(nn_def *c) { return c && c->confusion ? TRUE : FALSE; }
extern "C" UINT _NN(get, confusion_matrix)(nn_def *c, int which, UINT max_cells, UINT *cells) {
    if (!c || !c->n_classes || (which != NN_CONFUSION_LAST && which != NN_CONFUSION_BEST)) return 0;
    const UINT *m = which == NN_CONFUSION_BEST ? c->confusion_best : c->confusion_last;
    if (!m) return 0;
    const unsigned long long all = hpnn_confusion_cells(c->n_classes);
    if (cells) memcpy(cells, m, sizeof(UINT) * (size_t)(all < max_cells ? all : max_cells));
    return c->n_classes;
}
extern "C" UINT _NN(get, class_history)(nn_def *c, UINT pass, UINT *support, UINT *hit, UINT *predicted) {
    if (!c || !c->class_history || pass >= c->n_class_history) return 0;
    const UINT n = c->n_classes, *r = c->class_history + (size_t)pass * 3 * n;
    if (support) memcpy(support, r, sizeof(UINT) * n);
    if (hit) memcpy(hit, r + n, sizeof(UINT) * n);
    if (predicted) memcpy(predicted, r + 2 * (size_t)n, sizeof(UINT) * n);
    return n;
}
extern "C" UINT _NN(return, confusion_launches)(nn_def *c) { return c ? c->confusion_launches : 0; }
extern "C" BOOL _NN(dump, confusion_matrix)(nn_def *c, int which, const CHAR *filename) {
    const UINT n = _NN(get, confusion_matrix)(c, which, 0, NULL);
    if (!n || !filename) return FALSE;
    FILE *fp = fopen(filename, "w");
    if (!fp) return FALSE;
    const UINT *m = which == NN_CONFUSION_BEST ? c->confusion_best : c->confusion_last;
    _OUT(fp, "# %u\n", n);
    for (UINT t = 0; t < n; t++)
        for (UINT g = 0; g <= n; g++) _OUT(fp, "%u%c", m[(size_t)t * (n + 1) + g], g == n ? '\n' : ' ');
    return fclose(fp) == 0;
}
extern "C" const DOUBLE *_NN(get, lr_history)(nn_def *c, UINT *n) {
    if (n) *n = c && c->lr_history ? c->n_lr_history : 0;
    return c ? c->lr_history : NULL;
}
extern "C" UINT _NN(return, last_pass)(void) { return g_last_pass; }
extern "C" UINT _NN(return, last_total)(void) { return g_last_total; }

/* ------------------------------------------------------------------ */
/* the conf keys                                                       */
/* ------------------------------------------------------------------ */
extern "C" nn_def *_NN(load, conf)(const CHAR *filename) {
    FILE *fp = fopen(filename, "r");
    if (!fp) {
        NN_ERROR(stderr, "Error opening configuration file: %s\n", filename);
        return NULL;
    }
    ConfLoad l = {(nn_def *)calloc(1, sizeof(nn_def)), 0, 0, {}, NULL};
    _NN(init, conf)(l.conf);
    char *buf = NULL;
    size_t cap = 0;
    bool ok = true;
    while (ok && hpnn_readline(fp, &buf, &cap)) {
        const char *lb = strchr(buf, '[');
        const char *rb = lb ? strchr(lb, ']') : NULL;
        if (!rb) continue;
        const std::string key(lb + 1, rb - lb - 1);
        l.line = buf;
        if (const ConfKey *row = find_key(key)) ok = load_key(l, *row, key, value_of(rb + 1));
    }
    fclose(fp);
    ok = ok && finish_load(l);
    free(buf);
    if (ok) return l.conf;
    _NN(deinit, conf)(l.conf);
    free(l.conf);
    return NULL;
}

extern "C" void _NN(dump, conf)(nn_def *conf, FILE *fp) {
    if (!conf) return;
    _OUT(fp, "# NN configuration (libhpnn-mi355x)\n");
    for (const ConfKey &row : CONF_KEYS) {
        if (row.batched && conf->mode != NN_MODE_BATCHED) continue;
        if (row.kind == OTHER) {
            if (row.dump) row.dump(conf, fp);
        } else if (row.kind == COUNT) {
            if (field_of<UINT>(conf, row)) _OUT(fp, "[%s] %u\n", row.name, field_of<UINT>(conf, row));
        } else if (row.kind == REAL) {
            if (row.set(field_of<DOUBLE>(conf, row))) _OUT(fp, "[%s] %.17g\n", row.name, field_of<DOUBLE>(conf, row));
        } else {
            const int value = field_of<int>(conf, row);
            const char *w = value != row.unset ? word_of(row.words, value) : NULL;
            if (w) _OUT(fp, "[%s] %s\n", row.name, w);
        }
    }
}

/* ------------------------------------------------------------------ */
/* kernel management                                                   */
/* ------------------------------------------------------------------ */
extern "C" BOOL _NN(generate, kernel)(nn_def *conf, ...) {
    va_list ap;
    va_start(ap, conf);
    UINT n_in = va_arg(ap, UINT);
    UINT n_hid = va_arg(ap, UINT);
    UINT n_out = va_arg(ap, UINT);
    UINT *hiddens = va_arg(ap, UINT *);
    va_end(ap);
    if (conf->type == NN_TYPE_UKN) return FALSE;
    _NN(free, kernel)(conf);
    kernel_ann *k = ann_generate(&conf->seed, n_in, n_hid, n_out, hiddens);
    if (!k) return FALSE;
    k->name = strdup(conf->name ? conf->name : "noname");
    conf->kernel = k;
    conf->need_init = TRUE;
    NN_OUT(stdout, "generated kernel: %llu parameters\n", (unsigned long long)ann_n_params(k));
    return TRUE;
}

extern "C" BOOL _NN(load, kernel)(nn_def *conf) {
    if (!conf->f_kernel) return FALSE;
    if (conf->type == NN_TYPE_UKN) return FALSE;
    _NN(free, kernel)(conf);
    kernel_ann *k = ann_load(conf->f_kernel);
    if (!k) return FALSE;
    if (conf->name) {
        free(k->name);
        k->name = strdup(conf->name);
    } else {
        conf->name = strdup(k->name);
    }
    conf->kernel = k;
    return TRUE;
}

extern "C" void _NN(dump, kernel)(nn_def *conf, FILE *out) {
    if (!conf || !conf->kernel) {
        NN_ERROR(stderr, "CAN'T SAVE KERNEL! kernel=NULL\n");
        return;
    }
    hpnn_gpu_sync_host(KERN(conf));
    ann_dump(KERN(conf), out, FALSE);
}

extern "C" void _NN(dump, kernel_exact)(nn_def *conf, FILE *out) {
    if (!conf || !conf->kernel) return;
    hpnn_gpu_sync_host(KERN(conf));
    ann_dump(KERN(conf), out, TRUE);
}

extern "C" UINT _NN(get, n_inputs)(nn_def *c) { return c && c->kernel ? KERN(c)->n_inputs : 0; }
extern "C" UINT _NN(get, n_hiddens)(nn_def *c) { return c && c->kernel ? KERN(c)->n_hiddens : 0; }
extern "C" UINT _NN(get, n_outputs)(nn_def *c) { return c && c->kernel ? KERN(c)->n_outputs : 0; }
extern "C" UINT _NN(get, h_neurons)(nn_def *c, UINT layer) {
    if (!c || !c->kernel || layer >= KERN(c)->n_hiddens) return 0;
    return KERN(c)->hiddens[layer].n_neurons;
}

/* ------------------------------------------------------------------ */
/* samples                                                             */
/* ------------------------------------------------------------------ */
static bool read_vector(FILE *fp, char **buf, size_t *cap, UINT n, DOUBLE *dst) {
    UINT got = 0;
    while (got < n && hpnn_readline(fp, buf, cap)) {
        const char *p = *buf;
        char *e;
        while (got < n) {
            DOUBLE v = strtod(p, &e);
            if (e == p) break;
            dst[got++] = v;
            p = e;
        }
        if (got < n) {
            /* values may be wrapped: continue only if the line was numeric */
            const char *q = p;
            while (*q && isspace((unsigned char)*q)) q++;
            if (*q) break;
        }
    }
    return got == n;
}

extern "C" BOOL _NN(read, sample)(CHAR *filename, DOUBLE **in, DOUBLE **out) {
    *in = NULL;
    *out = NULL;
    if (!filename) return FALSE;
    FILE *fp = fopen(filename, "r");
    if (!fp) return FALSE;
    char *buf = NULL;
    size_t cap = 0;
    BOOL ok = TRUE;
    while (ok && hpnn_readline(fp, &buf, &cap)) {
        const char *p = strchr(buf, '[');
        if (!p) continue;
        bool is_in = !strncmp(p, "[input", 6), is_out = !strncmp(p, "[output", 7);
        if (!is_in && !is_out) continue;
        const char *rb = strchr(p, ']');
        UINT n = 0;
        if (rb) {
            const char *q = rb + 1;
            while (*q && isspace((unsigned char)*q)) q++;
            if (isdigit((unsigned char)*q)) n = (UINT)strtoul(q, NULL, 10);
        }
        if (n == 0) {
            NN_ERROR(stderr, "sample %s %s read failed!\n", filename, is_in ? "input" : "output");
            ok = FALSE;
            break;
        }
        DOUBLE **dst = is_in ? in : out;
        free(*dst);
        *dst = (DOUBLE *)malloc(sizeof(DOUBLE) * n);
        if (!read_vector(fp, &buf, &cap, n, *dst)) {
            NN_ERROR(stderr, "sample %s %s read failed!\n", filename, is_in ? "input" : "output");
            ok = FALSE;
        }
    }
    fclose(fp);
    free(buf);
    if (!ok || !*in || !*out) {
        free(*in);
        free(*out);
        *in = *out = NULL;
        return FALSE;
    }
    return TRUE;
}

/* ------------------------------------------------------------------ */
/* workflow helpers                                                    */
/* ------------------------------------------------------------------ */
/* seeded permutation without replacement (reference libhpnn.c:1218-1229) */
static std::vector<UINT> seeded_order(UINT n, UINT seed) {
    srandom(seed);
    std::vector<UINT> order;
    std::vector<char> used(n, 0);
    order.reserve(n);
    for (UINT j = 0; j < n; j++) {
        UINT idx;
        do {
            idx = (UINT)((DOUBLE)random() * n / RAND_MAX);
        } while (idx >= n || used[idx]);
        used[idx] = 1;
        order.push_back(idx);
    }
    return order;
}

static bool use_gpu(const nn_def *conf) {
    if (conf->device == NN_DEVICE_CPU) return false;
    bool avail = hpnn_rt_gpu_available();
    if (conf->device == NN_DEVICE_GPU && !avail) {
        NN_ERROR(stderr, "GPU requested but no GPU available!\n");
    }
    return avail;
}

static DOUBLE default_lr(const nn_def *conf, bool gpu) {
    if (conf->lr > 0) return conf->lr;
    if (conf->train == NN_TRAIN_ADAM) return ADAM_LEARN_RATE;
    if (gpu || conf->mode == NN_MODE_BATCHED) return GPU_LEARN_RATE;
    if (conf->type == NN_TYPE_ANN) return conf->train == NN_TRAIN_BPM ? BPM_LEARN_RATE : BP_LEARN_RATE;
    return GPU_LEARN_RATE;
}

static DOUBLE default_alpha(const nn_def *conf) { return conf->momentum >= 0 ? conf->momentum : BPM_MOMENTUM; }

/* ------------------------------------------------------------------ */
/* training                                                            */
/* ------------------------------------------------------------------ */
/* one metrics event; engine ("gpu" | "cpu") leads its fields, NULL: the event has no engine field */
__attribute__((format(printf, 3, 4))) static void emit_event(const char *event, const char *engine,
                                                             const char *fmt, ...) {
    if (!hpnn_metrics_active()) return;
    char buf[384];
    const int n = engine ? snprintf(buf, sizeof buf, "\"engine\": \"%s\", ", engine) : 0;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf + n, sizeof buf - n, fmt, ap);
    va_end(ap);
    hpnn_metrics_emit(event, buf);
}

static nn_lr_schedule schedule_kind(nn_def *conf) {
    nn_lr_schedule kind = NN_LR_NONE;
    _NN(get, lr_schedule)(conf, &kind, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    return kind;
}

#define REFUSE(...)                                                        \
    do {                                                                   \
        NN_ERROR(stderr, __VA_ARGS__);                                     \
        return true;                                                       \
    } while (0)

/* step 1: what a call is refused for before a sample is read ... */
static bool refused(nn_def *conf) {
    const bool batched = conf->mode == NN_MODE_BATCHED, cg = conf->train == NN_TRAIN_CG;
    if (conf->train != NN_TRAIN_BP && conf->train != NN_TRAIN_BPM && !cg && conf->train != NN_TRAIN_ADAM) {
        NN_ERROR(stdout, "unimplemented training type!\n");
        return true;
    }
    /* one CG iteration sums over the whole sample set: there is none in online mode */
    if (cg && !batched)
        REFUSE("[train] CG needs [mode] batched (one iteration per epoch over the whole sample set); "
               "online mode trains with BP or BPM\n");
    if (cg && conf->dtype == NN_DTYPE_BF16)
        REFUSE("[train] CG: the line search compares losses that the BF16 forward cannot resolve; "
               "use [dtype] f32 or f64\n");
    if (conf->train == NN_TRAIN_ADAM) {
        /* the moments are those of a minibatch sequence: there is none in online mode */
        if (!batched)
            REFUSE("[train] ADAM needs [mode] batched (its moments run over minibatch steps); "
                   "online mode trains with BP or BPM\n");
        DOUBLE beta1, beta2, epsilon, decay;
        _NN(get, adam)(conf, &beta1, &beta2, &epsilon, &decay);
        if (!hpnn_adam_valid(0.0, beta1, beta2, epsilon, decay))
            REFUSE("[train] ADAM: beta1 %g, beta2 %g, epsilon %g, decay %g are out of range "
                   "(0 <= beta < 1, epsilon > 0, decay >= 0)\n", beta1, beta2, epsilon, decay);
        if (conf->momentum >= 0) NN_OUT(stdout, "[train] ADAM: [momentum] is unused (the moments decay with [beta1], [beta2])\n");
    }
    const nn_lr_schedule kind = schedule_kind(conf);
    if (kind != NN_LR_NONE && batched && cg)
        REFUSE("[lr_schedule] is not supported by [train] CG (the line search chooses its own step); "
               "use [train] BP, BPM or ADAM\n");
    if (kind == NN_LR_PLATEAU && batched && !conf->validate)
        REFUSE("[lr_schedule] plateau needs [validate] N: there is no validation loss to watch\n");
    /* [clip]: a finite bound >= 0 (0: off); batched BP / BPM / ADAM on one device or the CPU */
    if (!hpnn_clip_valid(conf->clip))
        REFUSE("[clip] %g is out of range (the largest gradient norm, finite and > 0; 0: off)\n", conf->clip);
    if (conf->clip > 0.0 && batched && cg)
        REFUSE("[clip] is not supported by [train] CG (the line search chooses its own step); "
               "use [train] BP, BPM or ADAM\n");
    return false;
}

/* ... and, in batched mode, once the training samples are loaded; [validate] N: the held-out set of
 * [test_dir] (directory or pack file), in name order */
static bool refused_validation(const nn_def *conf, const kernel_ann *k, std::vector<DOUBLE> &Xv,
                               std::vector<DOUBLE> &Tv, UINT &nv) {
    if (conf->keep_best && !conf->validate)
        REFUSE("[keep_best] needs [validate] N: there is no validation pass to keep the best of\n");
    if (conf->patience && !conf->keep_best)
        REFUSE("[patience] needs [keep_best] loss | acc: the metric that has to improve\n");
    if (conf->confusion && !conf->validate)
        REFUSE("[confusion] needs [validate] N: there is no validation pass to tally\n");
    if (!conf->validate) return false;
    HpnnSamples vsrc;
    if (!conf->tests || !vsrc.open(conf->tests))
        REFUSE("[validate] needs a [test_dir] that can be opened: %s\n", conf->tests ? conf->tests : "(not set)");
    std::vector<UINT> vorder(vsrc.size());
    for (UINT i = 0; i < (UINT)vorder.size(); i++) vorder[i] = i;
    HpnnTraceRange tl("load_validation_samples");
    nv = (UINT)vsrc.load(vorder, k->n_inputs, k->n_outputs, _NN(return, omp_threads)(), Xv, Tv);
    if (nv == 0) REFUSE("[validate]: no usable sample in [test_dir] %s\n", conf->tests);
    return false;
}

/* step 2: the engine's options from the conf, the schedule state and its announcement included;
 * false: the schedule keys do not make a schedule */
static bool batched_opts(nn_def *conf, kernel_ann *k, bool gpu, DOUBLE lr, DOUBLE alpha, hpnn_batched_opts &o) {
    memset(&o, 0, sizeof(o));
    o.type = conf->type;
    o.train = conf->train;
    o.dtype = conf->dtype;
    o.batch = conf->batch;
    o.epochs = conf->epochs;
    o.lr = lr;
    o.alpha = conf->train == NN_TRAIN_BPM ? alpha : 0.0;
    o.seed = conf->seed;
    o.resume = conf->resume && k->dw != NULL;
    if (conf->train == NN_TRAIN_ADAM) _NN(get, adam)(conf, &o.beta1, &o.beta2, &o.eps, &o.decay);
    o.epoch0 = conf->epochs_done;
    o.shuffle = conf->shuffle == NN_SHUFFLE_EPOCH ? 1 : 0;
    o.validate = conf->validate;
    o.keep_best = (UINT)conf->keep_best;
    o.patience = conf->patience;
    nn_lr_schedule kind;
    DOUBLE gamma, lr_end, lr_min;
    UINT period, span, patience, warmup;
    _NN(get, lr_schedule)(conf, &kind, &gamma, &period, &span, &lr_end, &lr_min, &patience, &warmup);
    if (kind != NN_LR_NONE) {
        o.sched = 1;
        hpnn_lr_state_init(&o.lrs, (unsigned int)kind, lr, gamma, period, span, lr_end, lr_min, patience, warmup,
                           conf->epochs_done);
        if (!hpnn_lr_valid(&o.lrs)) {
            NN_ERROR(stderr, "[lr_schedule]: needs finite [lr] and [lr_end], 0 < [lr_gamma] <= 1, [lr_period] >= 1, "
                             "[lr_min] >= 0, [lr_span] >= 1 for linear and [lr_patience] >= 1 for plateau\n");
            return false;
        }
        /* plateau continues from the running fields a state file left in the kernel */
        if (kind == NN_LR_PLATEAU && k->lr_loaded) hpnn_lr_running_get(k, &o.lrs);
        NN_OUT(stdout, "batched %s training: learning rate schedule %s, lr %g gamma %g period %u span %u end %g "
                       "min %g patience %u warmup %u\n", gpu ? "GPU" : "CPU", word_of(LR_WORDS, kind), lr, gamma, period,
               span, lr_end, lr_min, patience, warmup);
    }
    o.confusion = conf->confusion ? 1 : 0;
    o.clip = conf->clip;
    if (o.clip > 0.0)
        NN_OUT(stdout, "batched %s training: gradient clipping: max norm %g\n", gpu ? "GPU" : "CPU", o.clip);
    k->lr_loaded = 0;
    UINT ng = 1;
    _NN(get, n_gpu)(&ng);
    o.n_gpu = ng ? ng : 1;
    const char *pe = getenv("HPNN_PARALLEL");
    o.tp = (pe ? (pe[0] == 't' || pe[0] == 'T') : conf->parallel == NN_PARALLEL_TP) ? 1 : 0;
    return true;
}
#undef REFUSE

/* [keep_best]: the record of the best pass, NULL when none was taken */
static const hpnn_validation_record *best_record(const nn_def *conf, const hpnn_batched_stats &st) {
    return conf->keep_best && st.best_epoch && st.best_index < st.n_val ? &st.val[st.best_index] : NULL;
}

/* step 3: the progress of the returned kernel after a call that went well */
static void book_progress(nn_def *conf, const hpnn_batched_stats &st, UINT n) {
    if (conf->keep_best && st.best_epoch) {
        /* the kernel is the one of the best pass's epoch: the progress is that epoch's too */
        conf->samples_seen += (UINT64)n * (st.best_epoch - conf->epochs_done);
        conf->epochs_done = st.best_epoch;
    } else if (conf->keep_best) {
        NN_WARN(stderr, "[keep_best]: no validation pass could be taken (every loss a NaN); "
                        "the weights after the last epoch run are returned\n");
        conf->epochs_done += st.epochs_run;
        conf->samples_seen += (UINT64)n * st.epochs_run;
    } else {
        conf->epochs_done += conf->epochs;
        conf->samples_seen += st.samples;
    }
    if (const hpnn_validation_record *b = best_record(conf, st)) {
        conf->best_epoch = b->epoch;
        conf->best_loss = b->loss;
        conf->best_correct = b->correct;
        conf->best_n = b->n;
    }
}

/* step 4: the report of a call that went well: one function per kind of record writes its stdout
 * line and its metrics event (the engines emit the "validation" events themselves) */
static void report_cg(const char *engine, UINT epoch, const hpnn_cg_record &r) {
    const int trial = r.trial == HPNN_CG_NONE ? -1 : (int)r.trial;
    NN_OUT(stdout, "CG: epoch %u loss=%.10f beta=%.10g alpha=%.10g trial=%d%s\n", epoch, r.f0, r.beta, r.alpha, trial,
           (r.flags & HPNN_CG_FAILED) ? " FAILED" : "");
    emit_event("cg", engine, "\"epoch\": %u, \"f0\": %.17g, \"f1\": %.17g, \"beta\": %.17g, \"alpha\": %.17g, "
               "\"trial\": %d, \"flags\": %u", epoch, r.f0, r.f1, r.beta, r.alpha, trial, r.flags);
}
static void report_lr(const char *engine, UINT epoch, DOUBLE lr) {
    NN_OUT(stdout, "LR: epoch %u lr=%.17g\n", epoch, lr);
    emit_event("lr", engine, "\"epoch\": %u, \"lr\": %.17g", epoch, lr);
}
static void report_clip(const char *engine, UINT epoch, const hpnn_clip_record &r) {
    NN_OUT(stdout, "CLIP: epoch %u steps=%u clipped=%u max_norm=%.17g last_norm=%.17g\n", epoch, r.steps, r.clipped,
           r.norm_max, r.norm_last);
    emit_event("clip", engine, "\"epoch\": %u, \"steps\": %u, \"clipped\": %u, \"max_norm\": %.17g, \"last_norm\": %.17g",
               epoch, r.steps, r.clipped, r.norm_max, r.norm_last);
}
static void report_validation(const hpnn_validation_record &r) {
    NN_OUT(stdout, "VALIDATION: epoch %u loss=%.10f acc=%u/%u\n", r.epoch, r.loss, r.correct, r.n);
}
/* rec: support, hit, predicted of the pass (n words each) */
static void report_classes(UINT epoch, const UINT *rec, UINT n) {
    const int w = hpnn_worst_class(rec, rec + n, (int)n);
    NN_OUT(stdout, "CLASSES: epoch %u bacc=%.10f worst=%d recall=%u/%u\n", epoch,
           hpnn_balanced_accuracy(rec, rec + n, (int)n), w, w < 0 ? 0 : rec[n + w], w < 0 ? 0 : rec[w]);
}
static void report_best(const char *engine, const hpnn_validation_record &b, nn_keep_best metric) {
    NN_OUT(stdout, "BEST: epoch %u loss=%.10f acc=%u/%u\n", b.epoch, b.loss, b.correct, b.n);
    emit_event("best", engine, "\"epoch\": %u, \"loss\": %.17g, \"correct\": %u, \"n\": %u, \"metric\": \"%s\"", b.epoch,
               b.loss, b.correct, b.n, word_of(KEEP_WORDS, metric));
}
static void report_early_stop(const char *engine, UINT epoch, UINT patience) {
    NN_OUT(stdout, "EARLY STOP: epoch %u (no improvement in %u passes)\n", epoch, patience);
    emit_event("early_stop", engine, "\"epoch\": %u, \"patience\": %u", epoch, patience);
}
static void report_batched(const nn_def *conf, const hpnn_batched_stats &st, const char *engine, UINT epoch0) {
    for (UINT i = 0; i < st.n_cg; i++) report_cg(engine, epoch0 + i + 1, st.cg[i]);
    for (UINT i = 0; i < st.n_lr; i++) report_lr(engine, epoch0 + i + 1, st.lr_hist[i]);
    for (UINT i = 0; i < st.n_clip; i++) report_clip(engine, epoch0 + i + 1, st.clip_hist[i]);
    for (UINT i = 0; i < st.n_val; i++) {
        report_validation(st.val[i]);
        if (st.class_hist && i < st.n_class_hist)
            report_classes(st.val[i].epoch, st.class_hist + (size_t)i * 3 * st.n_classes, st.n_classes);
    }
    if (const hpnn_validation_record *b = best_record(conf, st)) report_best(engine, *b, conf->keep_best);
    if (st.stop_epoch) report_early_stop(engine, st.stop_epoch, conf->patience);
}

static BOOL train_batched(nn_def *conf, HpnnSamples &src, bool gpu, DOUBLE lr, DOUBLE alpha) {
    kernel_ann *k = KERN(conf);
    const char *engine = gpu ? "gpu" : "cpu";
    std::vector<UINT> order = seeded_order((UINT)src.size(), conf->seed);
    std::vector<DOUBLE> X, T, Xv, Tv;
    UINT n, nv = 0;
    {
        HpnnTraceRange tl("load_samples");
        n = (UINT)src.load(order, k->n_inputs, k->n_outputs, _NN(return, omp_threads)(), X, T);
    }
    if (n == 0) return FALSE;
    drop_histories(conf);
    conf->best_epoch = 0;
    hpnn_batched_opts o;
    if (refused_validation(conf, k, Xv, Tv, nv) || !batched_opts(conf, k, gpu, lr, alpha, o)) return FALSE;
    o.Xv = nv ? Xv.data() : NULL;
    o.Tv = nv ? Tv.data() : NULL;
    o.nv = nv;
    hpnn_batched_stats st;
    memset(&st, 0, sizeof(st));
    BOOL ok;
    {
        HpnnTraceRange tb(gpu ? "train_batched_gpu" : "train_batched_cpu");
        ok = gpu ? hpnn_gpu_train_batched(k, X.data(), T.data(), n, &o, &st)
                 : hpnn_cpu_train_batched(k, X.data(), T.data(), n, &o, &st);
    }
    adopt_histories(conf, &st);
    if (!ok) drop_histories(conf); /* a failed call leaves none; st's arrays are gone with them */
    if (ok) book_progress(conf, st, n);
    /* the schedule state of the returned kernel: nn_dump_state saves plateau's */
    if (ok && o.sched) hpnn_lr_running_put(k, &st.lrs);
    NN_OUT(stdout, "BATCHED TRAINING: %llu samples in %.6f s (%.1f samples/s) loss=%.10f acc=%u/%u\n",
           (unsigned long long)st.samples, st.seconds, st.seconds > 0 ? st.samples / st.seconds : 0.0, st.epoch_loss,
           st.correct, n);
    if (ok) report_batched(conf, st, engine, o.epoch0);
    emit_event("train_batched", engine, "\"ok\": %s, \"samples\": %llu, \"seconds\": %.6f, \"samples_per_s\": %.3f, "
               "\"loss\": %.10g, \"correct\": %u, \"n\": %u, \"epochs_done\": %u", ok ? "true" : "false",
               (unsigned long long)st.samples, st.seconds, st.seconds > 0 ? st.samples / st.seconds : 0.0, st.epoch_loss,
               st.correct, n, conf->epochs_done);
    return ok;
}

/* the keys of batched training mean nothing in online (reference) mode: no epochs to validate,
 * reshuffle or change the rate between, no minibatch gradient whose norm could be bounded.  Each
 * is said once per process. */
static void warn_ignored_online(nn_def *conf) {
    const struct {
        bool set;
        const char *key;
    } ignored[] = {{conf->validate != 0, "[validate]"},
                   {conf->keep_best != NN_KEEP_OFF, "[keep_best]"},
                   {conf->patience != 0, "[patience]"},
                   {schedule_kind(conf) != NN_LR_NONE, "[lr_schedule]"},
                   {conf->clip > 0.0, "[clip]"},
                   {conf->confusion != 0, "[confusion]"},
                   {conf->shuffle == NN_SHUFFLE_EPOCH, "[shuffle] epoch"}};
    static bool warned[sizeof ignored / sizeof ignored[0]];
    for (size_t i = 0; i < sizeof ignored / sizeof ignored[0]; i++) {
        if (!ignored[i].set) continue;
        if (!warned[i]) NN_WARN(stderr, "%s has no effect in online mode (ignored)\n", ignored[i].key);
        warned[i] = true;
    }
}

static BOOL train_online(nn_def *conf, HpnnSamples &src, bool gpu, DOUBLE lr, DOUBLE alpha) {
    kernel_ann *k = KERN(conf);
    warn_ignored_online(conf);
    std::vector<UINT> order = seeded_order((UINT)src.size(), conf->seed);
    UINT n_ok = 0, n_done = 0;
    for (UINT idx : order) {
        const std::string &f = src.names[idx];
        NN_OUT(stdout, "TRAINING FILE: %16.16s\t", f.c_str());
        DOUBLE *in = NULL, *out = NULL;
        if (!src.get(idx, &in, &out)) continue;
        HpnnTraceRange ts("train_sample");
        UINT it = 0;
        BOOL ok = FALSE, first = FALSE;
        DOUBLE e0 = 0.0, r;
        if (gpu)
            r = hpnn_gpu_train_sample(k, conf->type, conf->train, in, out, lr, alpha, -1., &it, &ok, &e0, &first);
        else
            r = hpnn_cpu_train_sample(k, conf->type, conf->train, in, out, lr, alpha, -1., &it, &ok, &e0, &first);
        NN_COUT(stdout, " init=%15.10f", e0);
        NN_COUT(stdout, first ? " OK" : " NO");
        NN_COUT(stdout, " N_ITER=%8u", it);
        NN_COUT(stdout, " final=%15.10f", r);
        NN_COUT(stdout, ok ? " SUCCESS!\n" : " FAIL!\n");
        fflush(stdout);
        if (r > 0.1) NN_DBG(stdout, "bad optimization!\n");
        emit_event("train_sample", NULL, "\"file\": \"%s\", \"init\": %.10g, \"first_ok\": %s, \"n_iter\": %u, "
                   "\"final\": %.10g, \"success\": %s", f.c_str(), e0, first ? "true" : "false", it, r,
                   ok ? "true" : "false");
        n_ok += ok ? 1 : 0;
        n_done++;
        conf->samples_seen++;
        free(in);
        free(out);
        if (gpu && hpnn_gpu_failed(k)) {
            NN_ERROR(stderr, "GPU device state lost after %u samples: training aborted\n", n_done);
            return FALSE;
        }
    }
    if (gpu) hpnn_gpu_sync_host(k);
    emit_event("train_online", NULL, "\"samples\": %u, \"success\": %u", n_done, n_ok);
    return TRUE;
}

extern "C" BOOL _NN(train, kernel)(nn_def *conf) {
    if (!conf || !conf->kernel || !conf->samples || conf->type == NN_TYPE_UKN) return FALSE;
    if (refused(conf)) return FALSE;
    HpnnTraceRange tr("nn_train_kernel");
    HpnnSamples src;
    if (!src.open(conf->samples)) {
        NN_ERROR(stderr, "can't open sample directory: %s\n", conf->samples);
        return FALSE;
    }
    if (conf->seed == 0) conf->seed = (UINT)time(NULL);
    const bool gpu = use_gpu(conf);
    const DOUBLE lr = default_lr(conf, gpu), alpha = default_alpha(conf);
    return conf->mode == NN_MODE_BATCHED ? train_batched(conf, src, gpu, lr, alpha)
                                         : train_online(conf, src, gpu, lr, alpha);
}

/* ------------------------------------------------------------------ */
/* evaluation                                                          */
/* ------------------------------------------------------------------ */
extern "C" void _NN(run, kernel)(nn_def *conf) {
    g_last_pass = g_last_total = 0;
    if (!conf || !conf->kernel || !conf->tests || conf->type == NN_TYPE_UKN) return;
    kernel_ann *k = KERN(conf);
    /* [confusion]: the (truth, guess) pairs of the PASS / FAIL lines below, tallied on the host
     * through the rule header and kept as the "last" matrix */
    std::vector<UINT> tally;
    if (conf->confusion) {
        drop_confusion(conf);
        tally.assign((size_t)hpnn_confusion_cells(k->n_outputs), 0u);
    }
    HpnnSamples src;
    if (!src.open(conf->tests)) {
        NN_ERROR(stderr, "can't open test directory: %s\n", conf->tests);
        return;
    }
    HpnnTraceRange tr("nn_run_kernel");
    if (conf->seed == 0) conf->seed = (UINT)time(NULL);
    const bool gpu = use_gpu(conf);
    std::vector<UINT> order = seeded_order((UINT)src.size(), conf->seed);
    /* GPU: the whole test set goes through the batched engine of the model's precision
     * ([dtype], default f64 = the reference's) in one call -- one launch sequence and one
     * device-to-host copy per block of samples instead of one kernel launch, copy and host
     * sync per file; the per-file lines below are then produced from the outputs.
     * HPNN_RUN_ONLINE=1 keeps the reference's one-forward-per-file loop. */
    const char *ro = getenv("HPNN_RUN_ONLINE");
    const bool batched = gpu && !(ro && ro[0] == '1');
    std::vector<DOUBLE> Xall, Tall, Yall;
    std::vector<long> row_of(order.size(), -1);
    if (batched) {
        long rows = 0;
        for (size_t p = 0; p < order.size(); p++) {
            DOUBLE *in = NULL, *out = NULL;
            if (!src.get(order[p], &in, &out)) continue;
            Xall.insert(Xall.end(), in, in + k->n_inputs);
            Tall.insert(Tall.end(), out, out + k->n_outputs);
            row_of[p] = rows++;
            free(in);
            free(out);
        }
        Yall.assign((size_t)rows * k->n_outputs, 0.0);
        if (rows > 0 && !hpnn_gpu_infer_batched(k, conf->type, conf->dtype, Xall.data(), (UINT)rows, Yall.data())) {
            NN_ERROR(stderr, "batched GPU evaluation failed\n");
            return;
        }
    }
    for (size_t p = 0; p < order.size(); p++) {
        const UINT idx = order[p];
        const std::string &f = src.names[idx];
        NN_OUT(stdout, "TESTING FILE: %16.16s\t", f.c_str());
        DOUBLE *in = NULL, *out = NULL;
        const DOUBLE *o;
        if (batched) {
            if (row_of[p] < 0) continue;
            o = Yall.data() + (size_t)row_of[p] * k->n_outputs;
            out = Tall.data() + (size_t)row_of[p] * k->n_outputs;
        } else {
            if (!src.get(idx, &in, &out)) continue;
            if (gpu) {
                hpnn_gpu_forward(k, conf->type, in);
            } else {
                memcpy(k->in, in, sizeof(DOUBLE) * k->n_inputs);
                hpnn_cpu_forward(k, conf->type);
            }
            o = k->output.vec;
        }
        UINT guess, truth = 0;
        DOUBLE res;
        if (conf->type == NN_TYPE_ANN) {
            res = -1.;
            guess = k->n_outputs;
            truth = 0;
            for (UINT i = 0; i < k->n_outputs; i++) {
                if (res < o[i]) {
                    guess = i;
                    res = o[i];
                }
                if (out[i] > 0.5) truth = i;
            }
        } else {
            res = 0.;
            guess = 0;
            NN_DBG(stdout, " CLASS | PROBABILITY (%%)\n");
            NN_DBG(stdout, "-------|----------------\n");
            for (UINT i = 0; i < k->n_outputs; i++) {
                NN_DBG(stdout, " %5u | %15.10f\n", i + 1, o[i] * 100.);
                if (o[i] > res) {
                    res = o[i];
                    guess = i;
                }
                if (out[i] > 0.1) truth = i;
            }
            NN_DBG(stdout, "-------|----------------\n");
            NN_COUT(stdout, " BEST CLASS idx=%u P=%15.10f", guess + 1, res * 100);
        }
        g_last_total++;
        if (conf->confusion) hpnn_confusion_count(tally.data(), (int)truth, (int)guess, (int)k->n_outputs);
        if (guess == truth) {
            g_last_pass++;
            NN_COUT(stdout, " [PASS]\n");
        } else {
            NN_COUT(stdout, " [FAIL idx=%u]\n", truth + 1);
        }
        fflush(stdout);
        if (!batched) {
            free(in);
            free(out);
        }
    }
    emit_event("run", NULL, "\"pass\": %u, \"total\": %u, \"accuracy\": %.6f", g_last_pass, g_last_total,
               g_last_total ? (double)g_last_pass / g_last_total : 0.0);
    UINT cells = 0;
    if (conf->confusion && export_records(tally, &conf->confusion_last, &cells)) conf->n_classes = k->n_outputs;
}
