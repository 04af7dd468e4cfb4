/*
 * libhpnn -- the rule of the per-class validation metrics ([confusion], docs/DESIGN.md 3.2l).
 *
 * One definition for the CPU oracle, the device kernels (kernels_confusion.hip), nn_run_kernel and
 * the tests: plain C++ here, __host__ __device__ under hipcc.
 *
 * Target class of a sample.  With int labels: the label.  With dense targets: the lowest index of
 * the largest target value (t[i] > t[best] moves best, so a NaN never wins and ties keep the
 * lowest index) -- the `tr` of the CPU engines and the `it` of the output kernels.
 *
 * Guess.  What the evaluation kernels write per row: the lowest index of the largest output;
 * HPNN_GUESS_PAD (-1) marks a row at or past n_valid, HPNN_GUESS_NONE (1 << 30) a row in which no
 * output compared (a NaN row).
 *
 * Matrix.  uint32 M[n_out][n_out + 1], row-major: M[t][g] counts the valid samples of target t
 * guessed g; column n_out ("none") takes every guess that is no class (>= n_out).  A row with
 * guess < 0 is not a sample.  A target outside [0, n_out) is a caller bug: the row is skipped and
 * nothing is written for it.
 *
 * Per-class record of a pass: support[c] (row sum), hit[c] (diagonal), predicted[c] (column sum
 * without the "none" column), uint32 each, 3 * n_out words in that order.
 *
 * Balanced accuracy: the mean of hit[c] / support[c] over the classes with support[c] > 0, in FP64,
 * in class order, additions and divisions only (correctly rounded on the host and on the device, as
 * in lrsched.h); 0 when no class has support.
 */
#ifndef LIBHPNN_CONFUSION_H
#define LIBHPNN_CONFUSION_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HPNN_CONF_FN __host__ __device__ static inline
#else
#define HPNN_CONF_FN static inline
#endif

#define HPNN_GUESS_PAD (-1)
#define HPNN_GUESS_NONE (1 << 30)

/* words of a matrix */
HPNN_CONF_FN unsigned long long hpnn_confusion_cells(unsigned int n_out) {
    return (unsigned long long)n_out * ((unsigned long long)n_out + 1ull);
}

/* the target class of a dense row: the lowest index of the largest value */
#define HPNN_CONF_TARGET(name, T)                       \
    HPNN_CONF_FN int name(const T *t, int n_out) {      \
        int tr = 0;                                     \
        for (int i = 1; i < n_out; i++)                 \
            if (t[i] > t[tr]) tr = i;                   \
        return tr;                                      \
    }
HPNN_CONF_TARGET(hpnn_confusion_target_f64, double)
HPNN_CONF_TARGET(hpnn_confusion_target_f32, float)
#undef HPNN_CONF_TARGET

/* the cell of (target, guess) in M, -1: the row counts nowhere */
HPNN_CONF_FN long long hpnn_confusion_cell(int target, int guess, int n_out) {
    if (guess < 0 || target < 0 || target >= n_out) return -1;
    const int col = guess < n_out ? guess : n_out;
    return (long long)target * (n_out + 1) + col;
}

/* one sample into a host matrix */
HPNN_CONF_FN void hpnn_confusion_count(unsigned int *M, int target, int guess, int n_out) {
    const long long c = hpnn_confusion_cell(target, guess, n_out);
    if (c >= 0) M[c] += 1u;
}

/* the per-class record of a matrix: rec = support[n_out], hit[n_out], predicted[n_out] */
HPNN_CONF_FN void hpnn_confusion_classes(const unsigned int *M, int n_out, unsigned int *rec) {
    for (int c = 0; c < n_out; c++) {
        unsigned int row = 0u, col = 0u;
        for (int g = 0; g <= n_out; g++) row += M[(long long)c * (n_out + 1) + g];
        for (int t = 0; t < n_out; t++) col += M[(long long)t * (n_out + 1) + c];
        rec[c] = row;
        rec[n_out + c] = M[(long long)c * (n_out + 1) + c];
        rec[2 * n_out + c] = col;
    }
}

HPNN_CONF_FN double hpnn_balanced_accuracy(const unsigned int *support, const unsigned int *hit, int n_out) {
    double sum = 0.0, classes = 0.0;
    for (int c = 0; c < n_out; c++) {
        if (!support[c]) continue;
        sum = sum + (double)hit[c] / (double)support[c];
        classes = classes + 1.0;
    }
    return classes > 0.0 ? sum / classes : 0.0;
}

/* the supported class of lowest recall (lowest index on ties; hit/support compared as exact
 * cross products), -1 when no class has support */
HPNN_CONF_FN int hpnn_worst_class(const unsigned int *support, const unsigned int *hit, int n_out) {
    int w = -1;
    for (int c = 0; c < n_out; c++) {
        if (!support[c]) continue;
        if (w < 0 || (unsigned long long)hit[c] * support[w] < (unsigned long long)hit[w] * support[c]) w = c;
    }
    return w;
}

#endif /* LIBHPNN_CONFUSION_H */
