/*
 * libhpnn -- the conf keys: one table, CONF_KEYS, that nn_load_conf and nn_dump_conf both walk
 * (host only; api.cpp is the one file that includes this).
 *
 * A new key is one row here: its name, its nn_def field, its kind with the rule of a valid value,
 * the hint of its error message and how nn_dump_conf knows that it is set.
 */
#ifndef HPNN_CONF_KEYS_H
#define HPNN_CONF_KEYS_H
#include <libhpnn/ann.h>
#include <libhpnn/clip.h>
#include <ctype.h>
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>

static void set_str(CHAR **dst, const CHAR *src) {
    free(*dst);
    *dst = src ? strdup(src) : NULL;
}

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

static std::string lower(std::string s) {
    for (auto &ch : s) ch = (char)tolower(ch);
    return s;
}

/* what nn_load_conf gathers besides the conf itself: the topology of an [init] generate */
struct ConfLoad {
    nn_def *conf;
    UINT n_in, n_out;
    std::vector<UINT> hid;
    const char *line; /* the whole line of the key at hand */
};

/* the two lines of a malformed value; the function at hand gives up */
#define CONF_FAIL(...)                                                     \
    do {                                                                   \
        NN_ERROR(stderr, "Malformed NN configuration file!\n");            \
        NN_ERROR(stderr, __VA_ARGS__);                                     \
        return false;                                                      \
    } while (0)

/* a word and the value it stands for; of several words with one value the first is the one dumped */
struct ConfWord {
    const char *word;
    int value;
};
static constexpr ConfWord DTYPE_WORDS[] = {{"f64", NN_DTYPE_F64}, {"f32", NN_DTYPE_F32},  {"bf16", NN_DTYPE_BF16},
                                           {"fp64", NN_DTYPE_F64}, {"double", NN_DTYPE_F64}, {"fp32", NN_DTYPE_F32},
                                           {"float", NN_DTYPE_F32}, {NULL, 0}};
static constexpr ConfWord SHUFFLE_WORDS[] = {{"once", NN_SHUFFLE_ONCE}, {"epoch", NN_SHUFFLE_EPOCH}, {NULL, 0}};
static constexpr ConfWord KEEP_WORDS[] = {{"loss", NN_KEEP_LOSS}, {"acc", NN_KEEP_ACC}, {NULL, 0}};
static constexpr ConfWord ONOFF_WORDS[] = {{"on", 1}, {"off", 0}, {NULL, 0}};
static constexpr ConfWord LR_WORDS[] = {{"constant", NN_LR_CONSTANT}, {"step", NN_LR_STEP}, {"linear", NN_LR_LINEAR},
                                        {"plateau", NN_LR_PLATEAU}, {NULL, 0}};

/* the word of a value, NULL when it has none */
static const char *word_of(const ConfWord *words, int value) {
    for (; words->word; words++)
        if (words->value == value) return words->word;
    return NULL;
}

/* ---- the reference's keys: lenient by design (first letter decides, 0 becomes 1, a number is
 *      whatever strtoul / strtod make of the text); one small reader each ---- */
static bool lenient_uint(const char *name, const std::string &v, UINT *dst) {
    if (v.empty() || !isdigit((unsigned char)v[0])) CONF_FAIL("[%s] value: %s\n", name, v.c_str());
    *dst = (UINT)strtoul(v.c_str(), NULL, 10);
    return true;
}
static UINT at_least_one(const std::string &v) {
    const UINT x = (UINT)strtoul(v.c_str(), NULL, 10);
    return x ? x : 1;
}
static bool load_name(ConfLoad &l, const std::string &v) { return set_str(&l.conf->name, v.c_str()), true; }
static bool load_type(ConfLoad &l, const std::string &v) {
    switch (v.empty() ? 'A' : toupper(v[0])) {
        case 'L': l.conf->type = NN_TYPE_LNN; break;
        case 'S': l.conf->type = NN_TYPE_SNN; break;
        default: l.conf->type = NN_TYPE_ANN; break;
    }
    return true;
}
static bool load_init(ConfLoad &l, const std::string &v) {
    if (v.find("generate") != std::string::npos || v.find("GENERATE") != std::string::npos) {
        NN_OUT(stdout, "generating kernel!\n");
        l.conf->need_init = TRUE;
        return true;
    }
    NN_OUT(stdout, "loading kernel!\n");
    l.conf->need_init = FALSE;
    if (v.empty()) CONF_FAIL("[init] can't read filename: %s\n", l.line);
    set_str(&l.conf->f_kernel, v.c_str());
    return true;
}
static bool load_seed(ConfLoad &l, const std::string &v) { return lenient_uint("seed", v, &l.conf->seed); }
static bool load_input(ConfLoad &l, const std::string &v) { return lenient_uint("input", v, &l.n_in); }
static bool load_hidden(ConfLoad &l, const std::string &v) {
    if (!parse_uint_list(v, l.hid)) CONF_FAIL("[hidden] value: %s\n", v.c_str());
    return true;
}
static bool load_output(ConfLoad &l, const std::string &v) { return lenient_uint("output", v, &l.n_out); }
static bool load_train(ConfLoad &l, const std::string &v) {
    std::string u = v;
    for (auto &ch : u) ch = (char)toupper(ch);
    switch (u.empty() ? 0 : u[0]) {
        case 'B': l.conf->train = (u.size() > 2 && u[2] == 'M') ? NN_TRAIN_BPM : NN_TRAIN_BP; break;
        case 'C': l.conf->train = NN_TRAIN_CG; break;
        case 'A': l.conf->train = NN_TRAIN_ADAM; break;
        case 'S': l.conf->train = NN_TRAIN_SPLX; break;
        default: l.conf->train = NN_TRAIN_UKN; break;
    }
    return true;
}
static bool load_samples(ConfLoad &l, const std::string &v) { return set_str(&l.conf->samples, v.c_str()), true; }
static bool load_tests(ConfLoad &l, const std::string &v) { return set_str(&l.conf->tests, v.c_str()), true; }
static bool load_mode(ConfLoad &l, const std::string &v) {
    l.conf->mode = (!v.empty() && toupper(v[0]) == 'B') ? NN_MODE_BATCHED : NN_MODE_ONLINE;
    return true;
}
static bool load_device(ConfLoad &l, const std::string &v) {
    const std::string u = lower(v);
    l.conf->device = u == "cpu" ? NN_DEVICE_CPU : (u == "gpu" ? NN_DEVICE_GPU : NN_DEVICE_AUTO);
    return true;
}
static bool load_batch(ConfLoad &l, const std::string &v) { return l.conf->batch = at_least_one(v), true; }
static bool load_epochs(ConfLoad &l, const std::string &v) { return l.conf->epochs = at_least_one(v), true; }
static bool load_parallel(ConfLoad &l, const std::string &v) {
    l.conf->parallel = lower(v) == "tp" ? NN_PARALLEL_TP : NN_PARALLEL_DP;
    return true;
}
static bool load_lr(ConfLoad &l, const std::string &v) { return l.conf->lr = strtod(v.c_str(), NULL), true; }
static bool load_momentum(ConfLoad &l, const std::string &v) { return l.conf->momentum = strtod(v.c_str(), NULL), true; }

/* and what nn_dump_conf writes for those of them that are not a plain count, real or word */
static void dump_name(const nn_def *c, FILE *fp) { _OUT(fp, "[name] %s\n", c->name ? c->name : "noname"); }
static void dump_type(const nn_def *c, FILE *fp) {
    static const char *tn[] = {"ANN", "LNN", "SNN"};
    _OUT(fp, "[type] %s\n", (c->type >= 0 && c->type <= 2) ? tn[c->type] : "UKN");
}
static void dump_init(const nn_def *c, FILE *fp) {
    if (c->need_init || !c->f_kernel) _OUT(fp, "[init] generate\n");
    else _OUT(fp, "[init] %s\n", c->f_kernel);
}
static void dump_seed(const nn_def *c, FILE *fp) { _OUT(fp, "[seed] %u\n", c->seed); }
/* [inputs], [hiddens] and [outputs] are the kernel's */
static void dump_topology(const nn_def *c, FILE *fp) {
    const kernel_ann *k = (const kernel_ann *)c->kernel;
    if (!k) return;
    _OUT(fp, "[inputs] %u\n", k->n_inputs);
    _OUT(fp, "[hiddens]");
    for (UINT i = 0; i < k->n_hiddens; i++) _OUT(fp, " %u", k->hiddens[i].n_neurons);
    _OUT(fp, "\n[outputs] %u\n", k->n_outputs);
}
static void dump_train(const nn_def *c, FILE *fp) {
    static const char *trn[] = {"BP", "BPM", "CG", "SPLX", "ADAM"};
    _OUT(fp, "[train] %s\n", (c->train >= 0 && c->train <= 4) ? trn[c->train] : "UKN");
}
static void dump_samples(const nn_def *c, FILE *fp) {
    if (c->samples) _OUT(fp, "[sample_dir] %s\n", c->samples);
}
static void dump_tests(const nn_def *c, FILE *fp) {
    if (c->tests) _OUT(fp, "[test_dir] %s\n", c->tests);
}
static void dump_mode(const nn_def *, FILE *fp) { _OUT(fp, "[mode] batched\n"); }
static void dump_batch(const nn_def *c, FILE *fp) { _OUT(fp, "[batch] %u\n", c->batch); }
static void dump_epochs(const nn_def *c, FILE *fp) { _OUT(fp, "[epochs] %u\n", c->epochs); }
static void dump_parallel(const nn_def *c, FILE *fp) {
    if (c->parallel == NN_PARALLEL_TP) _OUT(fp, "[parallel] tp\n");
}

/* ---- the rules of the reals: what a value must be, and when nn_dump_conf takes it for set ---- */
static bool is_number(DOUBLE x) { return x == x; }
static bool is_finite(DOUBLE x) { return x - x == 0.0; }
static bool is_positive(DOUBLE x) { return x > 0.0; }
static bool is_not_negative(DOUBLE x) { return x >= 0.0; }
static bool is_finite_not_negative(DOUBLE x) { return is_finite(x) && x >= 0.0; }
static bool is_gamma(DOUBLE x) { return x > 0.0 && x <= 1.0; }
static bool is_beta(DOUBLE x) { return x >= 0.0 && x < 1.0; }
static bool is_clip(DOUBLE x) { return hpnn_clip_valid(x); }

/*
 * One row per conf key, in the order nn_dump_conf writes them.
 *
 * A key matches the row whose name is the longest prefix of it, so "[inputs]", "[samples]" and
 * "[lr_gamma_x]" are read as [input], [samples] and [lr_gamma].  No name is a prefix of another
 * one except "lr" of the "lr_*" names (the static_assert below), where the longer one wins: the
 * order of the rows decides nothing about reading.
 *
 *   OTHER  a reference key with a reader and a writer of its own (above)
 *   COUNT  a UINT: decimal, first character a digit, min <= value <= 2^32-1; set when not 0
 *   REAL   a DOUBLE through strtod: something consumed and valid(value); set when set(value)
 *   WORD   an enum: the lower-cased value is one of words; set when it differs from unset
 * lenient(row, load): a reference key that is dumped by its kind and read by its own lenient reader.
 * hint: the text in brackets of "[key] value: ... (hint)" or "[key] unknown: ... (hint)";
 * typed: the message names the key as the file spelled it, not as the row does;
 * batched: nn_dump_conf writes the key in batched mode only.
 */
enum ConfKind { OTHER, COUNT, REAL, WORD };
struct ConfKey {
    const char *name;
    ConfKind kind;
    size_t field; /* offsetof(nn_def, ...) of a COUNT, a REAL or a WORD */
    UINT min;
    bool (*valid)(DOUBLE);
    bool (*set)(DOUBLE);
    const ConfWord *words;
    int unset;
    const char *hint;
    bool typed, batched;
    bool (*load)(ConfLoad &, const std::string &);
    void (*dump)(const nn_def *, FILE *);
};
#define FIELD(member) offsetof(nn_def, member)
static constexpr ConfKey other(const char *name, bool (*load)(ConfLoad &, const std::string &),
                               void (*dump)(const nn_def *, FILE *)) {
    return {name, OTHER, 0, 0, NULL, NULL, NULL, 0, NULL, false, false, load, dump};
}
static constexpr ConfKey count(const char *name, size_t field, UINT min, const char *hint) {
    return {name, COUNT, field, min, NULL, NULL, NULL, 0, hint, false, false, NULL, NULL};
}
static constexpr ConfKey real(const char *name, size_t field, bool (*valid)(DOUBLE), const char *hint,
                              bool (*set)(DOUBLE) = is_number) {
    return {name, REAL, field, 0, valid, set, NULL, 0, hint, false, false, NULL, NULL};
}
static constexpr ConfKey word(const char *name, size_t field, const ConfWord *words, const char *hint, int unset) {
    return {name, WORD, field, 0, NULL, NULL, words, unset, hint, false, false, NULL, NULL};
}
static constexpr ConfKey lenient(ConfKey row, bool (*load)(ConfLoad &, const std::string &)) {
    return row.load = load, row;
}
static constexpr ConfKey typed(ConfKey row) { return row.typed = true, row; }
static constexpr ConfKey batched(ConfKey row) { return row.batched = true, row; }

static constexpr ConfKey CONF_KEYS[] = {
    other("name", load_name, dump_name),
    other("type", load_type, dump_type),
    other("init", load_init, dump_init),
    other("seed", load_seed, dump_seed),
    other("input", load_input, dump_topology),
    other("hidden", load_hidden, NULL),
    other("output", load_output, NULL),
    other("train", load_train, dump_train),
    other("sample_dir", load_samples, dump_samples),
    other("samples", load_samples, NULL),
    other("test_dir", load_tests, dump_tests),
    other("tests", load_tests, NULL),
    other("device", load_device, NULL), /* never dumped */
    batched(other("mode", load_mode, dump_mode)),
    batched(other("batch", load_batch, dump_batch)),
    batched(other("epochs", load_epochs, dump_epochs)),
    batched(word("dtype", FIELD(dtype), DTYPE_WORDS, "f64 | f32 | bf16", -1)), /* strict: docs/PARITY.md */
    batched(other("parallel", load_parallel, dump_parallel)),
    word("shuffle", FIELD(shuffle), SHUFFLE_WORDS, "once | epoch", NN_SHUFFLE_ONCE),
    count("validate", FIELD(validate), 1, "epochs between validation passes, >= 1"),
    word("keep_best", FIELD(keep_best), KEEP_WORDS, "loss | acc", NN_KEEP_OFF),
    count("patience", FIELD(patience), 1, "validation passes without improvement, >= 1"),
    lenient(real("lr", FIELD(lr), NULL, NULL, is_positive), load_lr),
    lenient(real("momentum", FIELD(momentum), NULL, NULL, is_not_negative), load_momentum),
    typed(real("beta1", FIELD(beta1), is_beta, "0 <= beta < 1")),
    typed(real("beta2", FIELD(beta2), is_beta, "0 <= beta < 1")),
    typed(real("epsilon", FIELD(epsilon), is_positive, "> 0")),
    typed(real("decay", FIELD(decay), is_not_negative, ">= 0")),
    word("lr_schedule", FIELD(lr_schedule), LR_WORDS, "constant | step | linear | plateau", NN_LR_NONE),
    typed(real("lr_gamma", FIELD(lr_gamma), is_gamma, "0 < gamma <= 1")),
    typed(count("lr_period", FIELD(lr_period), 1, "epochs, >= 1")),
    typed(count("lr_span", FIELD(lr_span), 1, "epochs, >= 1")),
    typed(real("lr_end", FIELD(lr_end), is_finite, "a finite rate")),
    typed(real("lr_min", FIELD(lr_min), is_finite_not_negative, ">= 0")),
    typed(count("lr_patience", FIELD(lr_patience), 1, "epochs, >= 1")),
    typed(count("warmup", FIELD(warmup), 0, "epochs, >= 0")),
    real("clip", FIELD(clip), is_clip, "the largest gradient norm, finite and > 0; 0: off", is_positive),
    word("confusion", FIELD(confusion), ONOFF_WORDS, "on | off", 0),
};

static constexpr bool name_is_prefix(const char *a, const char *b) {
    while (*a)
        if (*a++ != *b++) return false;
    return true;
}
static constexpr bool only_lr_is_a_prefix() {
    for (const ConfKey &a : CONF_KEYS)
        for (const ConfKey &b : CONF_KEYS)
            if (&a != &b && name_is_prefix(a.name, b.name) && !(a.name[0] == 'l' && a.name[1] == 'r' && !a.name[2]))
                return false;
    return true;
}
static_assert(only_lr_is_a_prefix(), "a conf key name is a prefix of another one: which row reads the longer key?");

template <class T>
static T &field_of(const nn_def *conf, const ConfKey &row) {
    return *(T *)((char *)conf + row.field);
}

static const ConfKey *find_key(const std::string &key) {
    const ConfKey *found = NULL;
    size_t len = 0;
    for (const ConfKey &row : CONF_KEYS) {
        const size_t n = strlen(row.name);
        if (n > len && key.compare(0, n, row.name) == 0) {
            found = &row;
            len = n;
        }
    }
    return found;
}

/* one "[key] value" line through its row */
static bool load_key(ConfLoad &l, const ConfKey &row, const std::string &key, const std::string &v) {
    const char *name = row.typed ? key.c_str() : row.name;
    if (row.load) return row.load(l, v);
    if (row.kind == COUNT) {
        const unsigned long x = strtoul(v.c_str(), NULL, 10);
        if (v.empty() || !isdigit((unsigned char)v[0]) || x < row.min || x > 0xffffffffUL)
            CONF_FAIL("[%s] value: %s (%s)\n", name, v.c_str(), row.hint);
        field_of<UINT>(l.conf, row) = (UINT)x;
    } else if (row.kind == REAL) {
        char *end = NULL;
        const DOUBLE x = strtod(v.c_str(), &end);
        if (v.empty() || end == v.c_str() || !row.valid(x)) CONF_FAIL("[%s] value: %s (%s)\n", name, v.c_str(), row.hint);
        field_of<DOUBLE>(l.conf, row) = x;
    } else {
        const std::string u = lower(v);
        const ConfWord *w = row.words;
        while (w->word && u != w->word) w++;
        if (!w->word) CONF_FAIL("[%s] unknown: %s (%s)\n", name, v.c_str(), row.hint);
        field_of<int>(l.conf, row) = w->value;
    }
    return true;
}

/* what has to hold once every line is read; generates or loads the kernel */
static bool finish_load(ConfLoad &l) {
    nn_def *conf = l.conf;
    if (conf->type == NN_TYPE_UKN) CONF_FAIL("[type] unknown or missing...\n");
    if (!conf->need_init) {
        if (_NN(load, kernel)(conf)) return true;
        NN_ERROR(stderr, "FAILED to load the NN kernel!\n");
        return false;
    }
    if (l.n_in == 0) CONF_FAIL("[input] wrong or missing...\n");
    if (l.hid.empty()) CONF_FAIL("[hidden] wrong or missing...\n");
    if (l.n_out == 0) CONF_FAIL("[output] wrong or missing...\n");
    for (UINT h : l.hid)
        if (h == 0) CONF_FAIL("[hidden] some have a 0 neuron content!\n");
    if (_NN(generate, kernel)(conf, l.n_in, (UINT)l.hid.size(), l.n_out, l.hid.data())) return true;
    NN_ERROR(stderr, "FAILED to generate NN kernel!\n");
    return false;
}
#undef CONF_FAIL

#endif /* HPNN_CONF_KEYS_H */
