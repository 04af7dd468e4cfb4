/*
 * libhpnn batched GPU engine -- the pieces its drivers share (train_*.cpp, infer_batched.cpp,
 * tp_engine.cpp).  All launches of a driver go to one HIP stream; nothing synchronises the
 * host inside an epoch (the reference synchronised every iteration).  Besides the
 * owners of device memory, graphs and resident sets: StateSeg, the element of a net's one ordered
 * list of state segments; BestSnap, the [keep_best] snapshot of that list; DevHistory, the
 * records-plus-cursor buffer behind the rate, clip and validation histories.
 */
#ifndef HPNN_GPU_BATCHED_COMMON_H
#define HPNN_GPU_BATCHED_COMMON_H
#include <hip/hip_runtime_api.h>
#include <libhpnn/ann.h>
#include <libhpnn/comm.h>
#include <libhpnn/devmem.h>
#include <libhpnn/observe.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "../core/runtime_internal.h"
#include "engine.h"
#include "kernels.h"

#define HIPCHK(x)                                                                           \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                             \
            NN_ERROR(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            return FALSE;                                                                   \
        }                                                                                   \
    } while (0)

namespace hpnn {
namespace eng {

inline layer_ann *layer_of(kernel_ann *k, int l) { return l < (int)k->n_hiddens ? &k->hiddens[l] : &k->output; }
inline int pad_rows(int v, int m) { return (v + m - 1) / m * m; }
/* nn_type -> the kernels' output-layer type */
inline int plan_type(nn_type t) { return t == NN_TYPE_ANN ? 0 : (t == NN_TYPE_LNN ? 1 : 2); }

/* owns one hpnn_dev_malloc allocation: every return of a driver releases it */
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) : p(o.p) { o.p = nullptr; }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t count) {
        reset();
        return hpnn_dev_malloc(&p, count * sizeof(T));
    }
    void reset() {
        if (p) hpnn_dev_free(p);
        p = nullptr;
    }
    T *get() const { return p; }
};

/* owns one instantiated graph (null: the launches run eagerly) */
struct GraphFree {
    void operator()(hipGraphExec_t x) const { hipGraphExecDestroy(x); }
};
typedef std::unique_ptr<std::remove_pointer<hipGraphExec_t>::type, GraphFree> GraphExec;

/* HIP graph of one epoch's steps (HPNN_GRAPH=0: eager launches): the epoch's minibatches
 * are the same every epoch (the sample order is drawn once, libhpnn.c:1218-1229), so one
 * capture is replayed per epoch and the host launches nothing per step.  With [shuffle] epoch
 * the launches are still the same every epoch: the captured epoch starts with the permutation
 * kernel (its epoch read from a device word a captured one-thread launch advances) and the
 * gathers into the staging set the steps read.  Returns false when
 * the launches cannot be captured (the caller then runs them eagerly: nothing of a failed
 * capture was executed). */
template <class Launch>
bool capture_epoch(hipStream_t s, Launch &&launch, GraphExec *exec) {
    exec->reset();
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) return false;
    const bool ok = launch();
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (!ok || e != hipSuccess || !g) {
        if (g) hipGraphDestroy(g);
        hipGetLastError();
        return false;
    }
    hipGraphExec_t x = nullptr;
    const bool inst = hipGraphInstantiate(&x, g, nullptr, nullptr, 0) == hipSuccess;
    hipGraphDestroy(g);
    if (inst) exec->reset(x);
    else hipGetLastError();
    return inst;
}

inline bool graphs_enabled() {
    const char *e = getenv("HPNN_GRAPH");
    return !(e && e[0] == '0') && !hpnn_debug_enabled();
}

/* the resident training set on one device, in the layout the engine's kernels read: x =
 * the main input (row-major, or fragment-major for the tile front), xg = an optional
 * fragment-major 8-bit copy (first-layer gradient of mode 'x'); row r of a minibatch starts
 * r * row_bytes in (fragment-major layouts keep that for r % 32 == 0).  Owns its buffers:
 * a second user of the same set (loopback replicas) takes a reference, never a copy. */
struct XSet {
    void *x = nullptr, *xg = nullptr;
    int *lab = nullptr; /* class index per row when every target row is one-hot (else null) */
    size_t row_bytes = 0, row_bytes_g = 0;
    int u8 = 0;
    float scale = 1.f;
    XSet() = default;
    XSet(const XSet &) = delete;
    XSet &operator=(const XSet &) = delete;
    ~XSet() { release(); }
    void release() {
        hpnn_dev_free(x);
        hpnn_dev_free(xg);
        hpnn_dev_free(lab);
        x = xg = nullptr;
        lab = nullptr;
    }
};

/* one-hot targets (1 at the class, t_lo = 0 for SNN / -1 otherwise, every row of the set) ->
 * int32 class indices on the device (rows_p entries, 0 past n): the BF16 plan then takes the
 * label form of its output layer (no dense target rows to read).  FALSE only on a device
 * error; xs->lab stays null when the targets are not one-hot. */
inline BOOL attach_labels(XSet *xs, const DOUBLE *T, UINT n, int n_out, int rows_p, nn_type type, hipStream_t s) {
    const char *e = getenv("HPNN_LABELS");
    if (e && e[0] == '0') return TRUE;
    const DOUBLE t_lo = type == NN_TYPE_SNN ? 0.0 : -1.0;
    std::vector<int> lab((size_t)rows_p, 0);
    for (UINT i = 0; i < n; i++) {
        int c = -1;
        for (int j = 0; j < n_out; j++) {
            const DOUBLE t = T[(size_t)i * n_out + j];
            if (t == 1.0 && c < 0) c = j;
            else if (t != t_lo) return TRUE; /* dense targets */
        }
        if (c < 0) return TRUE;
        lab[i] = c;
    }
    if (hpnn_dev_malloc(&xs->lab, lab.size() * sizeof(int)) != hipSuccess) return FALSE;
    return hipMemcpyAsync(xs->lab, lab.data(), lab.size() * sizeof(int), hipMemcpyHostToDevice, s) == hipSuccess &&
           hipStreamSynchronize(s) == hipSuccess;
}

/* one sample set resident on a device: the inputs in the net's layout, the labels (one-hot
 * targets) and the dense targets, zero-padded to *rows_p rows.  held_out: the layout of
 * net.upload_val, which chooses its own padding and returns it in *rows_p. */
template <typename TT>
struct ResidentSet {
    XSet xs;
    DevBuf<TT> T;
    template <class Net>
    BOOL upload(Net &net, const DOUBLE *X, const DOUBLE *Tg, UINT n, int n_in, int n_out, int *rows_p, nn_type type,
                hipStream_t s, bool held_out = false) {
        if (!(held_out ? net.upload_val(X, (int)n, n_in, &xs, rows_p) : net.upload_x(X, (int)n, n_in, *rows_p, &xs)))
            return FALSE;
        if (!attach_labels(&xs, Tg, n, n_out, *rows_p, type, s)) return FALSE;
        std::vector<TT> tf((size_t)*rows_p * n_out, (TT)0);
        for (size_t i = 0; i < (size_t)n * n_out; i++) tf[i] = (TT)Tg[i];
        HIPCHK(T.alloc(tf.size()));
        HIPCHK(hipMemcpy(T.get(), tf.data(), tf.size() * sizeof(TT), hipMemcpyHostToDevice));
        return TRUE;
    }
    void release() {
        xs.release();
        T.reset();
    }
};

/* a device history: cap records a one-workgroup launch files one at a time, and the cursor word
 * it advances; the host reads both once, after the last replay */
template <typename Rec>
struct DevHistory {
    DevBuf<Rec> buf;
    DevBuf<unsigned int> cur;
    size_t n = 0;
    /* extra: records allocated behind the cap the launches are given */
    BOOL init(size_t cap, size_t extra = 0) {
        n = cap;
        HIPCHK(buf.alloc(cap + extra ? cap + extra : 1));
        HIPCHK(cur.alloc(1));
        HIPCHK(hipMemset(cur.get(), 0, sizeof(unsigned int)));
        return TRUE;
    }
    Rec *hist() const { return buf.get(); }
    unsigned int *cursor() const { return cur.get(); }
    unsigned int cap() const { return (unsigned int)n; }
    /* synchronises; *out = the cap records, *filed = how many of them the launches filed */
    BOOL read(hipStream_t s, std::vector<Rec> *out, unsigned int *filed) const {
        out->resize(n);
        return hipStreamSynchronize(s) == hipSuccess &&
               hipMemcpy(filed, cur.get(), sizeof *filed, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(out->data(), buf.get(), n * sizeof(Rec), hipMemcpyDeviceToHost) == hipSuccess;
    }
};

/* the training state of a net adapter is ONE ordered list of device segments, built once at the
 * end of its init: per layer the weights, then the momentum / first moment and the second moment
 * where the net has them, then the Adam state, then the schedule state.  Everything that walks the
 * state (NetState, batched_net.h) walks this list and finds a segment by kind and layer */
enum SegKind { SEG_W, SEG_V, SEG_A, SEG_ADAM, SEG_LRS };
struct StateSeg {
    SegKind kind;
    int layer; /* SEG_W, SEG_V, SEG_A; 0 otherwise */
    void *dev;
    size_t bytes;
};

/* [keep_best]: the snapshot of a net's state segments in one allocation beside them, the device
 * segment table hpnn_snapshot_if copies by, and the best state hpnn_best_commit keeps; dst[i] is
 * the copy of segment i */
struct BestSnap {
    DevBuf<char> mem;
    DevBuf<hpnn_snap_seg> table;
    DevBuf<hpnn_best_state> state;
    std::vector<hpnn_snap_seg> segs;
    std::vector<void *> dst;
    /* extra (may be null): one more segment behind the net's, with a destination of its own (the
     * matrix of the kept pass under [confusion]) */
    BOOL init(const std::vector<StateSeg> &src, hipStream_t s, const hpnn_snap_seg *extra = nullptr) {
        size_t total = 0;
        for (const StateSeg &g : src) total += (g.bytes + 255) / 256 * 256;
        HIPCHK(mem.alloc(total ? total : 256));
        const size_t n_segs = src.size() + (extra ? 1 : 0);
        HIPCHK(table.alloc(n_segs ? n_segs : 1));
        HIPCHK(state.alloc(1));
        HIPCHK(hipMemsetAsync(state.get(), 0, sizeof(hpnn_best_state), s));
        size_t off = 0;
        for (const StateSeg &g : src) {
            segs.push_back({g.dev, mem.get() + off, (unsigned long long)g.bytes});
            dst.push_back(mem.get() + off);
            off += (g.bytes + 255) / 256 * 256;
        }
        if (extra) segs.push_back(*extra);
        if (hpnn_snapshot_table(table.get(), segs.data(), (int)segs.size(), s)) {
            NN_ERROR(stderr, "[keep_best]: the snapshot table was refused (alignment, or more than %d segments: the "
                             "layers' weights and moments%s)\n", HPNN_SNAP_MAX_SEGS,
                     extra ? " and the [confusion] matrix" : "");
            return FALSE;
        }
        return hpnn_best_preload(s) == 0;
    }
    unsigned int *take() const { return &state.get()->take; }
    unsigned int *stop() const { return &state.get()->stop; }
};

/* [confusion]: the matrix of the pass being tallied (M), of the last pass filed (last) and of the
 * kept pass (best, under [keep_best]), the per-class history (cap records of 3 n_out words, filed
 * at the validation cursor) and the guess of every held-out row; allocated only when the key is on */
struct ClassTally {
    DevBuf<unsigned int> M, last, best, hist;
    DevBuf<int> guess;
    int n_out = 0;
    size_t cap = 0;
    unsigned int launches = 0; /* issued by add / commit: a captured launch counts once, not per replay */
    hipStream_t s = nullptr;
    size_t cells() const { return (size_t)n_out * ((size_t)n_out + 1); }
    BOOL init(int n_out_, size_t passes, size_t guess_rows, bool keep, hipStream_t st) {
        n_out = n_out_;
        cap = passes;
        s = st;
        HIPCHK(M.alloc(cells()));
        HIPCHK(last.alloc(cells()));
        HIPCHK(hist.alloc(passes ? passes * 3 * (size_t)n_out : 1));
        HIPCHK(guess.alloc(guess_rows ? guess_rows : 1));
        HIPCHK(hipMemsetAsync(M.get(), 0, cells() * sizeof(unsigned int), s));
        HIPCHK(hipMemsetAsync(last.get(), 0, cells() * sizeof(unsigned int), s));
        if (keep) {
            HIPCHK(best.alloc(cells()));
            HIPCHK(hipMemsetAsync(best.get(), 0, cells() * sizeof(unsigned int), s));
        }
        return hpnn_confusion_preload(s) == 0;
    }
    /* the segment last -> best of the [keep_best] snapshot table */
    hpnn_snap_seg seg() const { return {last.get(), best.get(), (unsigned long long)(cells() * sizeof(unsigned int))}; }
    bool add(long row, int rows, const int *labels, const void *T, int ldt, int t_kind) {
        launches++;
        const void *t = labels ? (const void *)(labels + row) : (const void *)((const char *)T + (size_t)row * ldt *
                                                                             (t_kind == HPNN_CONFUSION_F64 ? 8 : 4));
        return hpnn_confusion_add(guess.get() + row, t, ldt, labels ? HPNN_CONFUSION_LABELS : t_kind, rows, n_out,
                                  M.get(), s) == 0;
    }
    bool commit(const unsigned int *cursor) {
        launches++;
        return hpnn_confusion_commit(M.get(), n_out, hist.get(), last.get(), cursor, (unsigned int)cap, s) == 0;
    }
    /* synchronises; the first `passes` records and the matrices (best: only when asked for) */
    BOOL read(size_t passes, std::vector<unsigned int> *rec, std::vector<unsigned int> *mlast,
              std::vector<unsigned int> *mbest) const {
        HIPCHK(hipStreamSynchronize(s));
        rec->resize(passes * 3 * (size_t)n_out);
        if (passes) HIPCHK(hipMemcpy(rec->data(), hist.get(), rec->size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        if (mlast) {
            mlast->resize(cells());
            HIPCHK(hipMemcpy(mlast->data(), last.get(), cells() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        }
        if (mbest) {
            mbest->resize(cells());
            HIPCHK(hipMemcpy(mbest->data(), best.get(), cells() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        }
        return TRUE;
    }
};

/* data-parallel step over RCCL: one bucket per layer goes into an async all-reduce on the
 * communicator's side stream as soon as it is final (last layer first), so it overlaps the
 * backward of the layers below; the update waits on a join.  ok_so_far = false: this replica
 * has already failed and only keeps its peers in step. */
template <class Net, typename TT>
bool rccl_bucket_step(Net &net, hpnn_comm *comm, hipStream_t s, const XSet &xs, long start, const TT *tb, int n_out,
                      int nv, int total, double lr, double alpha, bool mom, bool ok_so_far = true) {
    const std::vector<std::pair<int, int>> seq = net.buckets();
    size_t issued = 0;
    auto ready = [&](int lo, int hi) {
        issued++;
        return hpnn_comm_all_reduce_async(comm, net.gflat + net.goff[lo], (long)(net.goff[hi + 1] - net.goff[lo]),
                                          Net::comm_dt, s) == 0;
    };
    /* after a local failure every remaining bucket is still all-reduced (same
     * sizes, same order on every replica), so no peer is left waiting */
    bool okb = ok_so_far && net.grads(xs, start, tb, n_out, nv, ready);
    for (size_t i = issued; i < seq.size(); i++) ready(seq[i].first, seq[i].second);
    okb = (hpnn_comm_join(comm, s) == 0) && okb;
    return okb && net.update_flat(net.gflat, lr, alpha, 1.0 / (double)(total > 0 ? total : 1), mom);
}

/* hand-off health after every replay (<= ~32 steps): a small readback into pinned words,
 * enqueued behind the replay and judged one replay later (the host has already queued the next
 * replay, so the GPU never waits).  Two slots of 8 words: [0..2] the plan's, [3..] the driver's. */
struct HealthRing {
    unsigned int *hw = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    HealthRing() {
        if (hipHostMalloc((void **)&hw, 16 * sizeof(unsigned int), hipHostMallocDefault) != hipSuccess) hw = nullptr;
        for (hipEvent_t &e : ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    }
    HealthRing(const HealthRing &) = delete;
    HealthRing &operator=(const HealthRing &) = delete;
    ~HealthRing() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        if (hw) hipHostFree(hw);
    }
    bool ok() const { return hw && ev[0] && ev[1]; }
    /* extra(d): enqueues the driver's words from d[3] on; true on success */
    template <class Net, class Extra>
    bool post(int slot, hipStream_t s, Net &net, Extra &&extra) {
        unsigned int *d = hw + 8 * slot;
        for (int i = 0; i < 8; i++) d[i] = 0;
        return net.health_enqueue(d) && extra(d) && hipEventRecord(ev[slot], s) == hipSuccess;
    }
    /* the slot's words once its readback has completed (null: the wait failed) */
    const unsigned int *judge(int slot) {
        return hipEventSynchronize(ev[slot]) == hipSuccess ? hw + 8 * slot : nullptr;
    }
};

/* mean loss and argmax hits of the statistics slots the output kernels accumulate into */
inline BOOL read_stat_slots(const float *acc, hipStream_t s, double *loss, unsigned int *hits) {
    std::vector<float> h(HPNN_STAT_SLOTS * HPNN_STAT_STRIDE);
    HIPCHK(hipMemcpyAsync(h.data(), acc, h.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *loss = 0.0;
    *hits = 0;
    for (int i = 0; i < HPNN_STAT_SLOTS; i++) {
        unsigned int u;
        memcpy(&u, &h[(size_t)i * HPNN_STAT_STRIDE + 1], 4);
        *loss += h[(size_t)i * HPNN_STAT_STRIDE];
        *hits += u;
    }
    return TRUE;
}

/* split-K factor of an FP64 / FP32 weight gradient over the batch: ~256 workgroups, >= 256 rows each */
inline int fp_splits(int Nn, int Mm, int B) {
    const int tiles = ((Nn + 63) / 64) * ((Mm + 63) / 64);
    int sp = (256 + tiles - 1) / tiles;
    const int maxs = B / 256 > 0 ? B / 256 : 1;
    sp = sp < maxs ? sp : maxs;
    return hpnn_gemm_fp_splits(B, sp < 1 ? 1 : sp);
}

/* [shuffle] epoch and [validate] N exist in train_single only: the other drivers refuse them */
inline bool single_device_only(const hpnn_batched_opts *o, const char *who) {
    if (o->shuffle)
        NN_ERROR(stderr, "[shuffle] epoch is not supported by %s batched training (one device only)\n", who);
    else if (o->validate)
        NN_ERROR(stderr, "[validate] is not supported by %s batched training (one device only)\n", who);
    return o->shuffle || o->validate;
}

inline void fill_stats(hpnn_batched_stats *st, double seconds, UINT n, UINT epochs, double ep_loss,
                       unsigned int ep_hits) {
    st->seconds = seconds;
    st->samples = (UINT64)n * epochs;
    st->epoch_loss = ep_loss / (double)n;
    st->correct = ep_hits;
    st->last_loss = st->epoch_loss;
}

/* the three training drivers (one file each; each switches on o->dtype itself);
 * hpnn_gpu_train_batched (batched_engine.cpp) routes to one of them */
BOOL train_single(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                  hpnn_batched_stats *st);
BOOL train_dp(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
              hpnn_batched_stats *st, int G, bool loopback);
BOOL train_dp_mp(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                 hpnn_batched_stats *st);

}  // namespace eng
}  // namespace hpnn
#endif
