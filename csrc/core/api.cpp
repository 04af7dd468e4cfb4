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
 * Extensions: [mode] online|batched, [dtype], [device], [batch], [epochs], [shuffle], [validate],
 * [keep_best], [patience], [lr], [momentum] conf keys; batched training on CPU (FP64) or GPU.
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

#include "dataset.h"
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
    free(conf->validation);
    conf->validation = NULL;
    conf->n_validation = 0;
    free(conf->cg_history);
    conf->cg_history = NULL;
    conf->n_cg_history = 0;
    free(conf->lr_history);
    conf->lr_history = NULL;
    conf->n_lr_history = 0;
    free(conf->clip_history);
    conf->clip_history = NULL;
    conf->n_clip_history = 0;
    conf->name = conf->f_kernel = conf->samples = conf->tests = NULL;
}

static void set_str(CHAR **dst, const CHAR *src) {
    free(*dst);
    *dst = src ? strdup(src) : NULL;
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
extern "C" const DOUBLE *_NN(get, lr_history)(nn_def *c, UINT *n) {
    if (n) *n = c && c->lr_history ? c->n_lr_history : 0;
    return c ? c->lr_history : NULL;
}
extern "C" UINT _NN(return, last_pass)(void) { return g_last_pass; }
extern "C" UINT _NN(return, last_total)(void) { return g_last_total; }

/* ---- conf parsing helpers ---- */
static std::string trim(const std::string &s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) a++;
    while (b > a && isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}
/* strip a trailing '#' comment */
static std::string value_of(const char *after) {
    std::string v(after);
    size_t h = v.find('#');
    if (h != std::string::npos) v = v.substr(0, h);
    return trim(v);
}

static bool parse_uint_list(const std::string &v, std::vector<UINT> &out) {
    const char *p = v.c_str();
    char *e;
    out.clear();
    while (*p) {
        while (*p && isspace((unsigned char)*p)) p++;
        if (!*p) break;
        if (!isdigit((unsigned char)*p)) return false;
        out.push_back((UINT)strtoul(p, &e, 10));
        p = e;
    }
    return !out.empty();
}

extern "C" nn_def *_NN(load, conf)(const CHAR *filename) {
    nn_def *conf = (nn_def *)calloc(1, sizeof(nn_def));
    _NN(init, conf)(conf);
    UINT n_in = 0, n_out = 0;
    std::vector<UINT> hid;
    FILE *fp = fopen(filename, "r");
    char *buf = NULL;
    size_t cap = 0;
    if (!fp) {
        NN_ERROR(stderr, "Error opening configuration file: %s\n", filename);
        free(conf);
        return NULL;
    }
#define CONF_FAIL(...)                                                     \
    do {                                                                   \
        NN_ERROR(stderr, "Malformed NN configuration file!\n");            \
        NN_ERROR(stderr, __VA_ARGS__);                                     \
        goto fail;                                                         \
    } while (0)
    while (hpnn_readline(fp, &buf, &cap)) {
        const char *lb = strchr(buf, '[');
        if (!lb) continue;
        const char *rb = strchr(lb, ']');
        if (!rb) continue;
        std::string key(lb + 1, rb - lb - 1);
        std::string v = value_of(rb + 1);
        auto is = [&](const char *k) { return key.compare(0, strlen(k), k) == 0; };
        if (is("name")) {
            set_str(&conf->name, v.c_str());
        } else if (is("type")) {
            switch (v.empty() ? 'A' : toupper(v[0])) {
                case 'L': conf->type = NN_TYPE_LNN; break;
                case 'S': conf->type = NN_TYPE_SNN; break;
                default: conf->type = NN_TYPE_ANN; break;
            }
        } else if (is("init")) {
            if (v.find("generate") != std::string::npos || v.find("GENERATE") != std::string::npos) {
                NN_OUT(stdout, "generating kernel!\n");
                conf->need_init = TRUE;
            } else {
                NN_OUT(stdout, "loading kernel!\n");
                conf->need_init = FALSE;
                if (v.empty()) CONF_FAIL("[init] can't read filename: %s\n", buf);
                set_str(&conf->f_kernel, v.c_str());
            }
        } else if (is("seed")) {
            if (v.empty() || !isdigit((unsigned char)v[0])) CONF_FAIL("[seed] value: %s\n", v.c_str());
            conf->seed = (UINT)strtoul(v.c_str(), NULL, 10);
        } else if (is("input")) {
            if (v.empty() || !isdigit((unsigned char)v[0])) CONF_FAIL("[input] value: %s\n", v.c_str());
            n_in = (UINT)strtoul(v.c_str(), NULL, 10);
        } else if (is("hidden")) {
            if (!parse_uint_list(v, hid)) CONF_FAIL("[hidden] value: %s\n", v.c_str());
        } else if (is("output")) {
            if (v.empty() || !isdigit((unsigned char)v[0])) CONF_FAIL("[output] value: %s\n", v.c_str());
            n_out = (UINT)strtoul(v.c_str(), NULL, 10);
        } else if (is("train")) {
            std::string u = v;
            for (auto &ch : u) ch = (char)toupper(ch);
            if (!u.empty() && u[0] == 'B') conf->train = (u.size() > 2 && u[2] == 'M') ? NN_TRAIN_BPM : NN_TRAIN_BP;
            else if (!u.empty() && u[0] == 'C') conf->train = NN_TRAIN_CG;
            else if (!u.empty() && u[0] == 'A') conf->train = NN_TRAIN_ADAM;
            else if (!u.empty() && u[0] == 'S') conf->train = NN_TRAIN_SPLX;
            else conf->train = NN_TRAIN_UKN;
        } else if (is("sample_dir") || is("samples")) {
            set_str(&conf->samples, v.c_str());
        } else if (is("test_dir") || is("tests")) {
            set_str(&conf->tests, v.c_str());
        } else if (is("mode")) {
            conf->mode = (!v.empty() && toupper(v[0]) == 'B') ? NN_MODE_BATCHED : NN_MODE_ONLINE;
        } else if (is("dtype")) {
            std::string u = v;
            for (auto &ch : u) ch = (char)tolower(ch);
            if (u == "bf16") conf->dtype = NN_DTYPE_BF16;
            else if (u == "f32" || u == "fp32" || u == "float") conf->dtype = NN_DTYPE_F32;
            else if (u == "f64" || u == "fp64" || u == "double") conf->dtype = NN_DTYPE_F64;
            else CONF_FAIL("[dtype] unknown: %s (f64 | f32 | bf16)\n", v.c_str()); /* docs/PARITY.md */
        } else if (is("shuffle")) {
            std::string u = v;
            for (auto &ch : u) ch = (char)tolower(ch);
            if (u == "epoch") conf->shuffle = NN_SHUFFLE_EPOCH;
            else if (u == "once") conf->shuffle = NN_SHUFFLE_ONCE;
            else CONF_FAIL("[shuffle] unknown: %s (once | epoch)\n", v.c_str());
        } else if (is("validate")) {
            char *end = NULL;
            const unsigned long every = strtoul(v.c_str(), &end, 10);
            if (v.empty() || !isdigit((unsigned char)v[0]) || every == 0 || every > 0xffffffffUL)
                CONF_FAIL("[validate] value: %s (epochs between validation passes, >= 1)\n", v.c_str());
            conf->validate = (UINT)every;
        } else if (is("keep_best")) {
            std::string u = v;
            for (auto &ch : u) ch = (char)tolower(ch);
            if (u == "loss") conf->keep_best = NN_KEEP_LOSS;
            else if (u == "acc") conf->keep_best = NN_KEEP_ACC;
            else CONF_FAIL("[keep_best] unknown: %s (loss | acc)\n", v.c_str());
        } else if (is("patience")) {
            const unsigned long passes = strtoul(v.c_str(), NULL, 10);
            if (v.empty() || !isdigit((unsigned char)v[0]) || passes == 0 || passes > 0xffffffffUL)
                CONF_FAIL("[patience] value: %s (validation passes without improvement, >= 1)\n", v.c_str());
            conf->patience = (UINT)passes;
        } else if (is("device")) {
            std::string u = v;
            for (auto &ch : u) ch = (char)tolower(ch);
            conf->device = u == "cpu" ? NN_DEVICE_CPU : (u == "gpu" ? NN_DEVICE_GPU : NN_DEVICE_AUTO);
        } else if (is("batch")) {
            conf->batch = (UINT)strtoul(v.c_str(), NULL, 10);
            if (!conf->batch) conf->batch = 1;
        } else if (is("epochs")) {
            conf->epochs = (UINT)strtoul(v.c_str(), NULL, 10);
            if (!conf->epochs) conf->epochs = 1;
        } else if (is("parallel")) {
            std::string u = v;
            for (auto &ch : u) ch = (char)tolower(ch);
            conf->parallel = u == "tp" ? NN_PARALLEL_TP : NN_PARALLEL_DP;
        } else if (is("clip")) {
            char *end = NULL;
            const DOUBLE x = strtod(v.c_str(), &end);
            if (v.empty() || end == v.c_str() || !hpnn_clip_valid(x))
                CONF_FAIL("[clip] value: %s (the largest gradient norm, finite and > 0; 0: off)\n", v.c_str());
            conf->clip = x;
        } else if (is("lr_schedule")) {
            std::string u = v;
            for (auto &ch : u) ch = (char)tolower(ch);
            if (u == "constant") conf->lr_schedule = NN_LR_CONSTANT;
            else if (u == "step") conf->lr_schedule = NN_LR_STEP;
            else if (u == "linear") conf->lr_schedule = NN_LR_LINEAR;
            else if (u == "plateau") conf->lr_schedule = NN_LR_PLATEAU;
            else CONF_FAIL("[lr_schedule] unknown: %s (constant | step | linear | plateau)\n", v.c_str());
        } else if (is("lr_gamma") || is("lr_end") || is("lr_min")) {
            /* checked before [lr]: the keys are matched by prefix */
            char *end = NULL;
            const DOUBLE x = strtod(v.c_str(), &end);
            const bool gam = key[3] == 'g', fin = x - x == 0.0;
            if (v.empty() || end == v.c_str() || !fin || (gam ? !(x > 0.0 && x <= 1.0) : key[3] == 'm' && x < 0.0))
                CONF_FAIL("[%s] value: %s (%s)\n", key.c_str(), v.c_str(),
                          gam ? "0 < gamma <= 1" : key[3] == 'm' ? ">= 0" : "a finite rate");
            (gam ? conf->lr_gamma : key[3] == 'm' ? conf->lr_min : conf->lr_end) = x;
        } else if (is("lr_period") || is("lr_span") || is("lr_patience") || is("warmup")) {
            char *end = NULL;
            const unsigned long x = strtoul(v.c_str(), &end, 10);
            const bool wu = key[0] == 'w';
            if (v.empty() || !isdigit((unsigned char)v[0]) || (!wu && x == 0) || x > 0xffffffffUL)
                CONF_FAIL("[%s] value: %s (epochs%s)\n", key.c_str(), v.c_str(), wu ? ", >= 0" : ", >= 1");
            (wu ? conf->warmup : key[4] == 'e' ? conf->lr_period : key[3] == 's' ? conf->lr_span : conf->lr_patience) =
                (UINT)x;
        } else if (is("lr")) {
            conf->lr = strtod(v.c_str(), NULL);
        } else if (is("momentum")) {
            conf->momentum = strtod(v.c_str(), NULL);
        } else if (is("beta1") || is("beta2") || is("epsilon") || is("decay")) {
            /* [train] ADAM; no earlier key is a prefix of these ([batch] is not one of [beta1]) */
            char *end = NULL;
            const DOUBLE x = strtod(v.c_str(), &end);
            const bool beta = key[0] == 'b';
            const bool bad = v.empty() || end == v.c_str() || x != x ||
                             (beta ? (x < 0.0 || x >= 1.0) : key[0] == 'e' ? !(x > 0.0) : x < 0.0);
            if (bad)
                CONF_FAIL("[%s] value: %s (%s)\n", key.c_str(), v.c_str(),
                          beta ? "0 <= beta < 1" : key[0] == 'e' ? "> 0" : ">= 0");
            (beta ? (key.compare(0, 5, "beta1") == 0 ? conf->beta1 : conf->beta2)
                  : key[0] == 'e' ? conf->epsilon : conf->decay) = x;
        }
    }
    fclose(fp);
    fp = NULL;
    if (conf->type == NN_TYPE_UKN) CONF_FAIL("[type] unknown or missing...\n");
    if (conf->need_init) {
        if (n_in == 0) CONF_FAIL("[input] wrong or missing...\n");
        if (hid.empty()) CONF_FAIL("[hidden] wrong or missing...\n");
        if (n_out == 0) CONF_FAIL("[output] wrong or missing...\n");
        for (UINT h : hid)
            if (h == 0) CONF_FAIL("[hidden] some have a 0 neuron content!\n");
        if (!_NN(generate, kernel)(conf, n_in, (UINT)hid.size(), n_out, hid.data())) {
            NN_ERROR(stderr, "FAILED to generate NN kernel!\n");
            goto fail;
        }
    } else {
        if (!_NN(load, kernel)(conf)) {
            NN_ERROR(stderr, "FAILED to load the NN kernel!\n");
            goto fail;
        }
    }
    free(buf);
    return conf;
fail:
#undef CONF_FAIL
    if (fp) fclose(fp);
    free(buf);
    _NN(deinit, conf)(conf);
    free(conf);
    return NULL;
}

extern "C" void _NN(dump, conf)(nn_def *conf, FILE *fp) {
    if (!conf) return;
    static const char *tn[] = {"ANN", "LNN", "SNN"};
    static const char *trn[] = {"BP", "BPM", "CG", "SPLX", "ADAM"};
    _OUT(fp, "# NN configuration (libhpnn-mi355x)\n");
    _OUT(fp, "[name] %s\n", conf->name ? conf->name : "noname");
    _OUT(fp, "[type] %s\n", (conf->type >= 0 && conf->type <= 2) ? tn[conf->type] : "UKN");
    if (conf->need_init || !conf->f_kernel) _OUT(fp, "[init] generate\n");
    else _OUT(fp, "[init] %s\n", conf->f_kernel);
    _OUT(fp, "[seed] %u\n", conf->seed);
    kernel_ann *k = KERN(conf);
    if (k) {
        _OUT(fp, "[inputs] %u\n", k->n_inputs);
        _OUT(fp, "[hiddens]");
        for (UINT i = 0; i < k->n_hiddens; i++) _OUT(fp, " %u", k->hiddens[i].n_neurons);
        _OUT(fp, "\n[outputs] %u\n", k->n_outputs);
    }
    _OUT(fp, "[train] %s\n", (conf->train >= 0 && conf->train <= 4) ? trn[conf->train] : "UKN");
    if (conf->samples) _OUT(fp, "[sample_dir] %s\n", conf->samples);
    if (conf->tests) _OUT(fp, "[test_dir] %s\n", conf->tests);
    if (conf->mode == NN_MODE_BATCHED) {
        static const char *dn[] = {"f64", "f32", "bf16"};
        _OUT(fp, "[mode] batched\n[batch] %u\n[epochs] %u\n[dtype] %s\n", conf->batch, conf->epochs,
             dn[conf->dtype]);
        if (conf->parallel == NN_PARALLEL_TP) _OUT(fp, "[parallel] tp\n");
    }
    if (conf->shuffle == NN_SHUFFLE_EPOCH) _OUT(fp, "[shuffle] epoch\n");
    if (conf->validate) _OUT(fp, "[validate] %u\n", conf->validate);
    if (conf->keep_best) _OUT(fp, "[keep_best] %s\n", conf->keep_best == NN_KEEP_ACC ? "acc" : "loss");
    if (conf->patience) _OUT(fp, "[patience] %u\n", conf->patience);
    if (conf->lr > 0) _OUT(fp, "[lr] %.17g\n", conf->lr);
    if (conf->momentum >= 0) _OUT(fp, "[momentum] %.17g\n", conf->momentum);
    if (conf->beta1 == conf->beta1) _OUT(fp, "[beta1] %.17g\n", conf->beta1);
    if (conf->beta2 == conf->beta2) _OUT(fp, "[beta2] %.17g\n", conf->beta2);
    if (conf->epsilon == conf->epsilon) _OUT(fp, "[epsilon] %.17g\n", conf->epsilon);
    if (conf->decay == conf->decay) _OUT(fp, "[decay] %.17g\n", conf->decay);
    static const char *lrn[] = {"constant", "step", "linear", "plateau"};
    if (conf->lr_schedule >= NN_LR_CONSTANT && conf->lr_schedule <= NN_LR_PLATEAU)
        _OUT(fp, "[lr_schedule] %s\n", lrn[conf->lr_schedule]);
    if (conf->lr_gamma == conf->lr_gamma) _OUT(fp, "[lr_gamma] %.17g\n", conf->lr_gamma);
    if (conf->lr_period) _OUT(fp, "[lr_period] %u\n", conf->lr_period);
    if (conf->lr_span) _OUT(fp, "[lr_span] %u\n", conf->lr_span);
    if (conf->lr_end == conf->lr_end) _OUT(fp, "[lr_end] %.17g\n", conf->lr_end);
    if (conf->lr_min == conf->lr_min) _OUT(fp, "[lr_min] %.17g\n", conf->lr_min);
    if (conf->lr_patience) _OUT(fp, "[lr_patience] %u\n", conf->lr_patience);
    if (conf->warmup) _OUT(fp, "[warmup] %u\n", conf->warmup);
    if (conf->clip > 0.0) _OUT(fp, "[clip] %.17g\n", conf->clip);
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
extern "C" BOOL _NN(train, kernel)(nn_def *conf) {
    if (!conf || !conf->kernel || !conf->samples || conf->type == NN_TYPE_UKN) return FALSE;
    kernel_ann *k = KERN(conf);
    if (conf->train != NN_TRAIN_BP && conf->train != NN_TRAIN_BPM && conf->train != NN_TRAIN_CG &&
        conf->train != NN_TRAIN_ADAM) {
        NN_ERROR(stdout, "unimplemented training type!\n");
        return FALSE;
    }
    if (conf->train == NN_TRAIN_CG) {
        /* one CG iteration sums over the whole sample set: there is none in online mode */
        if (conf->mode != NN_MODE_BATCHED) {
            NN_ERROR(stderr, "[train] CG needs [mode] batched (one iteration per epoch over the whole sample set); "
                             "online mode trains with BP or BPM\n");
            return FALSE;
        }
        if (conf->dtype == NN_DTYPE_BF16) {
            NN_ERROR(stderr, "[train] CG: the line search compares losses that the BF16 forward cannot resolve; "
                             "use [dtype] f32 or f64\n");
            return FALSE;
        }
    }
    DOUBLE beta1 = 0.0, beta2 = 0.0, epsilon = 0.0, decay = 0.0;
    if (conf->train == NN_TRAIN_ADAM) {
        /* the moments are those of a minibatch sequence: there is none in online mode */
        if (conf->mode != NN_MODE_BATCHED) {
            NN_ERROR(stderr, "[train] ADAM needs [mode] batched (its moments run over minibatch steps); "
                             "online mode trains with BP or BPM\n");
            return FALSE;
        }
        _NN(get, adam)(conf, &beta1, &beta2, &epsilon, &decay);
        if (!hpnn_adam_valid(0.0, beta1, beta2, epsilon, decay)) {
            NN_ERROR(stderr, "[train] ADAM: beta1 %g, beta2 %g, epsilon %g, decay %g are out of range "
                             "(0 <= beta < 1, epsilon > 0, decay >= 0)\n", beta1, beta2, epsilon, decay);
            return FALSE;
        }
        if (conf->momentum >= 0) NN_OUT(stdout, "[train] ADAM: [momentum] is unused (the moments decay with [beta1], [beta2])\n");
    }
    /* [lr_schedule]: the keys as a training call uses them; the state itself is filled below, once
     * the rate and the progress are known */
    nn_lr_schedule lr_kind = NN_LR_NONE;
    DOUBLE lr_gamma = 0.0, lr_end = 0.0, lr_min = 0.0;
    UINT lr_period = 0, lr_span = 0, lr_patience = 0, lr_warmup = 0;
    _NN(get, lr_schedule)(conf, &lr_kind, &lr_gamma, &lr_period, &lr_span, &lr_end, &lr_min, &lr_patience, &lr_warmup);
    if (lr_kind != NN_LR_NONE && conf->mode == NN_MODE_BATCHED) {
        if (conf->train == NN_TRAIN_CG) {
            NN_ERROR(stderr, "[lr_schedule] is not supported by [train] CG (the line search chooses its own step); "
                             "use [train] BP, BPM or ADAM\n");
            return FALSE;
        }
        if (lr_kind == NN_LR_PLATEAU && !conf->validate) {
            NN_ERROR(stderr, "[lr_schedule] plateau needs [validate] N: there is no validation loss to watch\n");
            return FALSE;
        }
    }
    /* [clip]: a finite bound >= 0 (0: off); batched BP / BPM / ADAM on one device or the CPU */
    if (!hpnn_clip_valid(conf->clip)) {
        NN_ERROR(stderr, "[clip] %g is out of range (the largest gradient norm, finite and > 0; 0: off)\n", conf->clip);
        return FALSE;
    }
    if (conf->clip > 0.0 && conf->mode == NN_MODE_BATCHED && conf->train == NN_TRAIN_CG) {
        NN_ERROR(stderr, "[clip] is not supported by [train] CG (the line search chooses its own step); "
                         "use [train] BP, BPM or ADAM\n");
        return FALSE;
    }
    HpnnTraceRange tr("nn_train_kernel");
    HpnnSamples src;
    if (!src.open(conf->samples)) {
        NN_ERROR(stderr, "can't open sample directory: %s\n", conf->samples);
        return FALSE;
    }
    if (conf->seed == 0) conf->seed = (UINT)time(NULL);
    const bool gpu = use_gpu(conf);
    const DOUBLE lr = default_lr(conf, gpu);
    const DOUBLE alpha = default_alpha(conf);

    if (conf->mode == NN_MODE_BATCHED) {
        std::vector<UINT> order = seeded_order((UINT)src.size(), conf->seed);
        std::vector<DOUBLE> X, T;
        UINT n;
        {
            HpnnTraceRange tl("load_samples");
            n = (UINT)src.load(order, k->n_inputs, k->n_outputs, _NN(return, omp_threads)(), X, T);
        }
        if (n == 0) return FALSE;
        /* [validate] N: the held-out set of [test_dir] (directory or pack file), in name order */
        std::vector<DOUBLE> Xv, Tv;
        UINT nv = 0;
        free(conf->validation);
        conf->validation = NULL;
        conf->n_validation = 0;
        conf->best_epoch = 0;
        free(conf->cg_history);
        conf->cg_history = NULL;
        conf->n_cg_history = 0;
        free(conf->lr_history);
        conf->lr_history = NULL;
        conf->n_lr_history = 0;
        free(conf->clip_history);
        conf->clip_history = NULL;
        conf->n_clip_history = 0;
        if (conf->keep_best && !conf->validate) {
            NN_ERROR(stderr, "[keep_best] needs [validate] N: there is no validation pass to keep the best of\n");
            return FALSE;
        }
        if (conf->patience && !conf->keep_best) {
            NN_ERROR(stderr, "[patience] needs [keep_best] loss | acc: the metric that has to improve\n");
            return FALSE;
        }
        if (conf->validate) {
            HpnnSamples vsrc;
            if (!conf->tests || !vsrc.open(conf->tests)) {
                NN_ERROR(stderr, "[validate] needs a [test_dir] that can be opened: %s\n",
                         conf->tests ? conf->tests : "(not set)");
                return FALSE;
            }
            std::vector<UINT> vorder(vsrc.size());
            for (UINT i = 0; i < (UINT)vorder.size(); i++) vorder[i] = i;
            HpnnTraceRange tl("load_validation_samples");
            nv = (UINT)vsrc.load(vorder, k->n_inputs, k->n_outputs, _NN(return, omp_threads)(), Xv, Tv);
            if (nv == 0) {
                NN_ERROR(stderr, "[validate]: no usable sample in [test_dir] %s\n", conf->tests);
                return FALSE;
            }
        }
        hpnn_batched_opts o;
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
        o.beta1 = beta1;
        o.beta2 = beta2;
        o.eps = epsilon;
        o.decay = decay;
        o.epoch0 = conf->epochs_done;
        o.shuffle = conf->shuffle == NN_SHUFFLE_EPOCH ? 1 : 0;
        o.validate = conf->validate;
        o.Xv = nv ? Xv.data() : NULL;
        o.Tv = nv ? Tv.data() : NULL;
        o.nv = nv;
        o.keep_best = (UINT)conf->keep_best;
        o.patience = conf->patience;
        if (lr_kind != NN_LR_NONE) {
            o.sched = 1;
            hpnn_lr_state_init(&o.lrs, (unsigned int)lr_kind, lr, lr_gamma, lr_period, lr_span, lr_end, lr_min,
                               lr_patience, lr_warmup, conf->epochs_done);
            if (!hpnn_lr_valid(&o.lrs)) {
                NN_ERROR(stderr, "[lr_schedule]: needs finite [lr] and [lr_end], 0 < [lr_gamma] <= 1, [lr_period] >= 1, "
                                 "[lr_min] >= 0, [lr_span] >= 1 for linear and [lr_patience] >= 1 for plateau\n");
                return FALSE;
            }
            /* plateau continues from the running fields a state file left in the kernel */
            if (lr_kind == NN_LR_PLATEAU && k->lr_loaded) {
                o.lrs.scale = k->lr_scale;
                o.lrs.best = k->lr_best;
                o.lrs.stale = k->lr_stale;
                o.lrs.cuts = k->lr_cuts;
                o.lrs.valid = k->lr_valid;
            }
            static const char *lrn[] = {"constant", "step", "linear", "plateau"};
            NN_OUT(stdout, "batched %s training: learning rate schedule %s, lr %g gamma %g period %u span %u end %g "
                           "min %g patience %u warmup %u\n", gpu ? "GPU" : "CPU", lrn[lr_kind], lr, lr_gamma,
                   lr_period, lr_span, lr_end, lr_min, lr_patience, lr_warmup);
        }
        o.clip = conf->clip;
        if (o.clip > 0.0)
            NN_OUT(stdout, "batched %s training: gradient clipping: max norm %g\n", gpu ? "GPU" : "CPU", o.clip);
        k->lr_loaded = 0;
        UINT ng = 1;
        _NN(get, n_gpu)(&ng);
        o.n_gpu = ng ? ng : 1;
        {
            const char *pe = getenv("HPNN_PARALLEL");
            o.tp = (pe ? (pe[0] == 't' || pe[0] == 'T') : conf->parallel == NN_PARALLEL_TP) ? 1 : 0;
        }
        hpnn_batched_stats st;
        memset(&st, 0, sizeof(st));
        BOOL ok;
        {
            HpnnTraceRange tb(gpu ? "train_batched_gpu" : "train_batched_cpu");
            ok = gpu ? hpnn_gpu_train_batched(k, X.data(), T.data(), n, &o, &st)
                     : hpnn_cpu_train_batched(k, X.data(), T.data(), n, &o, &st);
        }
        if (ok && conf->keep_best && st.best_epoch) {
            /* the kernel is the one of the best pass's epoch: the progress is that epoch's too */
            conf->samples_seen += (UINT64)n * (st.best_epoch - conf->epochs_done);
            conf->epochs_done = st.best_epoch;
        } else if (ok && conf->keep_best) {
            NN_WARN(stderr, "[keep_best]: no validation pass could be taken (every loss a NaN); "
                            "the weights after the last epoch run are returned\n");
            conf->epochs_done += st.epochs_run;
            conf->samples_seen += (UINT64)n * st.epochs_run;
        } else if (ok) {
            conf->epochs_done += conf->epochs;
            conf->samples_seen += st.samples;
        }
        NN_OUT(stdout, "BATCHED TRAINING: %llu samples in %.6f s (%.1f samples/s) loss=%.10f acc=%u/%u\n",
               (unsigned long long)st.samples, st.seconds, st.seconds > 0 ? st.samples / st.seconds : 0.0,
               st.epoch_loss, st.correct, n);
        for (UINT i = 0; ok && i < st.n_cg; i++) {
            const hpnn_cg_record &r = st.cg[i];
            NN_OUT(stdout, "CG: epoch %u loss=%.10f beta=%.10g alpha=%.10g trial=%d%s\n", o.epoch0 + i + 1, r.f0, r.beta,
                   r.alpha, r.trial == HPNN_CG_NONE ? -1 : (int)r.trial, (r.flags & HPNN_CG_FAILED) ? " FAILED" : "");
            if (hpnn_metrics_active()) {
                char buf[384];
                snprintf(buf, sizeof buf,
                         "\"engine\": \"%s\", \"epoch\": %u, \"f0\": %.17g, \"f1\": %.17g, \"beta\": %.17g, "
                         "\"alpha\": %.17g, \"trial\": %d, \"flags\": %u",
                         gpu ? "gpu" : "cpu", o.epoch0 + i + 1, r.f0, r.f1, r.beta, r.alpha,
                         r.trial == HPNN_CG_NONE ? -1 : (int)r.trial, r.flags);
                hpnn_metrics_emit("cg", buf);
            }
        }
        for (UINT i = 0; ok && i < st.n_lr; i++) {
            NN_OUT(stdout, "LR: epoch %u lr=%.17g\n", o.epoch0 + i + 1, st.lr_hist[i]);
            if (hpnn_metrics_active()) {
                char buf[128];
                snprintf(buf, sizeof buf, "\"engine\": \"%s\", \"epoch\": %u, \"lr\": %.17g", gpu ? "gpu" : "cpu",
                         o.epoch0 + i + 1, st.lr_hist[i]);
                hpnn_metrics_emit("lr", buf);
            }
        }
        for (UINT i = 0; ok && i < st.n_clip; i++) {
            const hpnn_clip_record &r = st.clip_hist[i];
            NN_OUT(stdout, "CLIP: epoch %u steps=%u clipped=%u max_norm=%.17g last_norm=%.17g\n", o.epoch0 + i + 1,
                   r.steps, r.clipped, r.norm_max, r.norm_last);
            if (hpnn_metrics_active()) {
                char buf[256];
                snprintf(buf, sizeof buf,
                         "\"engine\": \"%s\", \"epoch\": %u, \"steps\": %u, \"clipped\": %u, \"max_norm\": %.17g, "
                         "\"last_norm\": %.17g",
                         gpu ? "gpu" : "cpu", o.epoch0 + i + 1, r.steps, r.clipped, r.norm_max, r.norm_last);
                hpnn_metrics_emit("clip", buf);
            }
        }
        if (ok && o.sched) {
            /* the schedule state of the returned kernel: nn_dump_state saves plateau's */
            k->lr_scale = st.lrs.scale;
            k->lr_best = st.lrs.best;
            k->lr_stale = st.lrs.stale;
            k->lr_cuts = st.lrs.cuts;
            k->lr_valid = st.lrs.valid;
        }
        for (UINT i = 0; ok && i < st.n_val; i++)
            NN_OUT(stdout, "VALIDATION: epoch %u loss=%.10f acc=%u/%u\n", st.val[i].epoch, st.val[i].loss,
                   st.val[i].correct, st.val[i].n);
        if (ok && conf->keep_best && st.best_epoch && st.best_index < st.n_val) {
            const hpnn_validation_record &b = st.val[st.best_index];
            conf->best_epoch = b.epoch;
            conf->best_loss = b.loss;
            conf->best_correct = b.correct;
            conf->best_n = b.n;
            NN_OUT(stdout, "BEST: epoch %u loss=%.10f acc=%u/%u\n", b.epoch, b.loss, b.correct, b.n);
            if (hpnn_metrics_active()) {
                char buf[256];
                snprintf(buf, sizeof buf,
                         "\"engine\": \"%s\", \"epoch\": %u, \"loss\": %.17g, \"correct\": %u, \"n\": %u, "
                         "\"metric\": \"%s\"",
                         gpu ? "gpu" : "cpu", b.epoch, b.loss, b.correct, b.n,
                         conf->keep_best == NN_KEEP_ACC ? "acc" : "loss");
                hpnn_metrics_emit("best", buf);
            }
        }
        if (ok && st.stop_epoch) {
            NN_OUT(stdout, "EARLY STOP: epoch %u (no improvement in %u passes)\n", st.stop_epoch, conf->patience);
            if (hpnn_metrics_active()) {
                char buf[128];
                snprintf(buf, sizeof buf, "\"engine\": \"%s\", \"epoch\": %u, \"patience\": %u", gpu ? "gpu" : "cpu",
                         st.stop_epoch, conf->patience);
                hpnn_metrics_emit("early_stop", buf);
            }
        }
        if (ok) {
            conf->validation = st.val;
            conf->n_validation = st.n_val;
            conf->cg_history = st.cg;
            conf->n_cg_history = st.n_cg;
            conf->lr_history = st.lr_hist;
            conf->n_lr_history = st.n_lr;
            conf->clip_history = st.clip_hist;
            conf->n_clip_history = st.n_clip;
        } else {
            free(st.val);
            free(st.cg);
            free(st.lr_hist);
            free(st.clip_hist);
        }
        if (hpnn_metrics_active()) {
            char buf[384];
            snprintf(buf, sizeof buf,
                     "\"engine\": \"%s\", \"ok\": %s, \"samples\": %llu, \"seconds\": %.6f, \"samples_per_s\": %.3f, "
                     "\"loss\": %.10g, \"correct\": %u, \"n\": %u, \"epochs_done\": %u",
                     gpu ? "gpu" : "cpu", ok ? "true" : "false", (unsigned long long)st.samples, st.seconds,
                     st.seconds > 0 ? st.samples / st.seconds : 0.0, st.epoch_loss, st.correct, n, conf->epochs_done);
            hpnn_metrics_emit("train_batched", buf);
        }
        return ok;
    }

    /* online (reference) mode */
    if (conf->validate) {
        static bool warned_v = false; /* no epochs here to validate between */
        if (!warned_v) NN_WARN(stderr, "[validate] has no effect in online mode (ignored)\n");
        warned_v = true;
    }
    if (conf->keep_best) {
        static bool warned_k = false; /* no validation pass here */
        if (!warned_k) NN_WARN(stderr, "[keep_best] has no effect in online mode (ignored)\n");
        warned_k = true;
    }
    if (conf->patience) {
        static bool warned_p = false;
        if (!warned_p) NN_WARN(stderr, "[patience] has no effect in online mode (ignored)\n");
        warned_p = true;
    }
    if (lr_kind != NN_LR_NONE) {
        static bool warned_l = false; /* no epochs here to change the rate between */
        if (!warned_l) NN_WARN(stderr, "[lr_schedule] has no effect in online mode (ignored)\n");
        warned_l = true;
    }
    if (conf->clip > 0.0) {
        static bool warned_c = false; /* no minibatch gradient here whose norm could be bounded */
        if (!warned_c) NN_WARN(stderr, "[clip] has no effect in online mode (ignored)\n");
        warned_c = true;
    }
    if (conf->shuffle == NN_SHUFFLE_EPOCH) {
        static bool warned = false; /* no epochs here: every sample is trained to convergence once */
        if (!warned) NN_WARN(stderr, "[shuffle] epoch has no effect in online mode (ignored)\n");
        warned = true;
    }
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
        if (hpnn_metrics_active()) {
            char buf[384];
            snprintf(buf, sizeof buf,
                     "\"file\": \"%s\", \"init\": %.10g, \"first_ok\": %s, \"n_iter\": %u, \"final\": %.10g, "
                     "\"success\": %s",
                     f.c_str(), e0, first ? "true" : "false", it, r, ok ? "true" : "false");
            hpnn_metrics_emit("train_sample", buf);
        }
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
    if (hpnn_metrics_active()) {
        char buf[128];
        snprintf(buf, sizeof buf, "\"samples\": %u, \"success\": %u", n_done, n_ok);
        hpnn_metrics_emit("train_online", buf);
    }
    return TRUE;
}

/* ------------------------------------------------------------------ */
/* evaluation                                                          */
/* ------------------------------------------------------------------ */
extern "C" void _NN(run, kernel)(nn_def *conf) {
    g_last_pass = g_last_total = 0;
    if (!conf || !conf->kernel || !conf->tests || conf->type == NN_TYPE_UKN) return;
    kernel_ann *k = KERN(conf);
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
    if (hpnn_metrics_active()) {
        char buf[128];
        snprintf(buf, sizeof buf, "\"pass\": %u, \"total\": %u, \"accuracy\": %.6f", g_last_pass, g_last_total,
                 g_last_total ? (double)g_last_pass / g_last_total : 0.0);
        hpnn_metrics_emit("run", buf);
    }
}
