/*
 * libhpnn -- the per-epoch sample permutation of batched training ([shuffle] epoch).
 *
 * One definition for the host engines, the device kernel and the tests: plain C++ here,
 * __host__ __device__ under hipcc.  All arithmetic is on 32-bit unsigned integers.
 *
 *   mix(x):  x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16
 *   bits = max(2, bit_length(n-1));  hb = (bits+1)/2;  mask = (1<<hb)-1
 *   key[r] = mix(seed ^ mix(epoch + 0x9e3779b9*(r+1)))          r = 0..3
 *   src(i):  x = i
 *            repeat: L = x>>hb; R = x&mask
 *                    for r in 0..3: (L,R) = (R, L ^ (mix(R ^ key[r]) & mask))
 *                    x = (L<<hb)|R
 *            until x < n
 *
 * A 4-round Feistel network on 2 hb bits is a bijection of [0, 2^(2 hb)); following it until
 * the value falls below n (cycle walking) restricts it to a bijection of [0, n).  The domain
 * is below 4 n, so a walk takes 4 iterations on average at worst.  src(i) is the index, in the order
 * drawn once from [seed], of the sample that stands at position i in epoch `epoch` (epochs
 * completed before it, so a resumed run continues the sequence).  n <= 1: identity.
 */
#ifndef LIBHPNN_SHUFFLE_H
#define LIBHPNN_SHUFFLE_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HPNN_SHUFFLE_FN __host__ __device__ static inline
#else
#define HPNN_SHUFFLE_FN static inline
#endif

/* the device kernel gives up after this many walk iterations (and reports it): no kernel
 * may spin without a bound */
#define HPNN_SHUFFLE_MAX_WALK 1024u

typedef struct {
    unsigned int n, hb, mask;
    unsigned int key[4];
} hpnn_shuffle_keys;

HPNN_SHUFFLE_FN unsigned int hpnn_shuffle_mix(unsigned int x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

HPNN_SHUFFLE_FN void hpnn_shuffle_setup(hpnn_shuffle_keys *k, unsigned int n, unsigned int seed, unsigned int epoch) {
    unsigned int bits = 0;
    for (unsigned int v = n ? n - 1 : 0; v; v >>= 1) bits++;
    if (bits < 2) bits = 2;
    k->n = n;
    k->hb = (bits + 1) / 2;
    k->mask = (1u << k->hb) - 1u;
    for (unsigned int r = 0; r < 4; r++) k->key[r] = hpnn_shuffle_mix(seed ^ hpnn_shuffle_mix(epoch + 0x9e3779b9u * (r + 1)));
}

/* src(i); at most max_walk iterations: past them *overflow is set (when given) and i itself
 * is returned, which is in range */
HPNN_SHUFFLE_FN unsigned int hpnn_shuffle_src(const hpnn_shuffle_keys *k, unsigned int i, unsigned int max_walk,
                                              int *overflow) {
    if (k->n <= 1) return i;
    unsigned int x = i;
    for (unsigned int w = 0; w < max_walk; w++) {
        unsigned int L = x >> k->hb, R = x & k->mask;
        for (int r = 0; r < 4; r++) {
            const unsigned int t = L ^ (hpnn_shuffle_mix(R ^ k->key[r]) & k->mask);
            L = R;
            R = t;
        }
        x = (L << k->hb) | R;
        if (x < k->n) return x;
    }
    if (overflow) *overflow = 1;
    return i;
}

/* the whole permutation on the host: out[i] = src(i), i < n */
static inline void hpnn_shuffle_perm(unsigned int n, unsigned int seed, unsigned int epoch, unsigned int *out) {
    hpnn_shuffle_keys k;
    hpnn_shuffle_setup(&k, n, seed, epoch);
    for (unsigned int i = 0; i < n; i++) out[i] = hpnn_shuffle_src(&k, i, 0xffffffffu, (int *)0);
}

#endif /* LIBHPNN_SHUFFLE_H */
