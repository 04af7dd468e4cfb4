/*
 * libhpnn batched GPU engine -- the two net adapters the drivers are templated over:
 * Batched (BF16 MFMA, FP32 masters: the library's BPlan) and BatchedFP<T> (FP64 / FP32).
 * Per minibatch
 *     forward   gemm_nt(act) per layer          (MFMA bf16)
 *     output    output_delta (act/softmax+loss+delta+accuracy)
 *     backward  gemm_nt(W^T, * f'(h)) per layer (MFMA bf16)
 *     gradient  gemm_tn split-K FP32 slabs      (MFMA bf16, tr-LDS reads)
 *     update    sgd_update (slab reduce + BP/BPM + BF16 W / W^T refresh)
 * Weights: host FP64 kernel_ann is the I/O master; the device keeps FP32 masters.
 * Both adapters have ONE step entry point for every optimizer (step) and list their training
 * state once, at the end of init, as ordered segments; NetState walks that list for the
 * [keep_best] snapshot, the downloads, the replica state and the exact resume.
 */
#ifndef HPNN_GPU_BATCHED_NET_H
#define HPNN_GPU_BATCHED_NET_H
#include <libhpnn/xar.h>
#include <algorithm>
#include <memory>
#include <string>

#include "batched_common.h"
#include "bplan.h"
#include "../dist/dp_exchange.h"

namespace hpnn {
namespace eng {

/* upload n host rows (FP64) as a padded BF16 matrix [rows_p x cols_p] */
inline BOOL upload_bf16(const DOUBLE *src, int rows, int cols, int rows_p, int cols_p, void **dst, hipStream_t s) {
    DevBuf<char> tmp;
    HIPCHK(hpnn_dev_malloc(dst, (size_t)rows_p * cols_p * 2));
    HIPCHK(tmp.alloc((size_t)rows * cols * 8));
    HIPCHK(hipMemcpyAsync(tmp.get(), src, (size_t)rows * cols * 8, hipMemcpyHostToDevice, s));
    if (hpnn_pack_bf16(tmp.get(), 1, rows, cols, cols, *dst, rows_p, cols_p, cols_p, s)) return FALSE;
    HIPCHK(hipStreamSynchronize(s));
    return TRUE;
}

/* a new device buffer *dst holding the bytes host bytes at h */
inline BOOL upload_bytes(const void *h, size_t bytes, void **dst, hipStream_t s) {
    HIPCHK(hpnn_dev_malloc(dst, bytes));
    HIPCHK(hipMemcpyAsync(*dst, h, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return TRUE;
}

/* round-to-nearest-even FP32 -> BF16 bits (the kernels' rounding) */
inline uint16_t bf16_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((u + 0x7FFF + ((u >> 16) & 1)) >> 16);
}

/* host [rows][cols] -> fragment-major [rows_p/32][cols_p/16][64][8] (hpnn_amd.ops.to_fragment_major:
 * lane 16 g + r of fragment (t, cb) holds A[32 t + 8 g + j][16 cb + r], j < 8), zero padded */
template <typename E, typename Cvt>
std::vector<E> to_fragment_major(const DOUBLE *src, int rows, int cols, int rows_p, int cols_p, Cvt cvt) {
    std::vector<E> out((size_t)rows_p * cols_p, (E)0);
    const int nbc = cols_p / 16;
    for (int r = 0; r < rows; r++) {
        const int t = r / 32, g = (r % 32) / 8, j = r % 8;
        for (int c = 0; c < cols; c++) {
            const size_t idx = ((((size_t)t * nbc + c / 16) * 64) + 16 * g + c % 16) * 8 + j;
            out[idx] = cvt(src[(size_t)r * cols + c]);
        }
    }
    return out;
}

/* the training state of an adapter, written once over its segment list (StateSeg, batched_common.h;
 * the adapter lists it at the end of init).  Net gives the stream s and two per-layer converters:
 *     to_host(host FP64 [N][M], device matrix, layer, l)    to_dev(device matrix, host FP64, layer, l)
 * Two layouts are contracts: segment i of the list pairs with BestSnap::dst[i], and get_state is
 * the bytes of the segments in list order without the schedule state (train_dp_mp all-gathers them) */
template <class Net>
struct NetState {
    std::vector<StateSeg> segs;
    Net &self() { return *static_cast<Net *>(this); }
    void list_layer(int l, void *W, void *V, void *A, size_t bytes) {
        void *const b[3] = {W, V, A};
        const SegKind kinds[3] = {SEG_W, SEG_V, SEG_A};
        for (int i = 0; i < 3; i++)
            if (b[i]) segs.push_back({kinds[i], l, b[i], bytes});
    }
    void list_tail(hpnn_adam_state *adam, hpnn_lr_state *lrs) {
        if (adam) segs.push_back({SEG_ADAM, 0, adam, sizeof *adam});
        if (lrs) segs.push_back({SEG_LRS, 0, lrs, sizeof *lrs});
    }
    /* the index of a segment in the list (and in a snapshot's dst); -1: the net has none */
    int seg(SegKind kind, int layer = 0) const {
        for (size_t i = 0; i < segs.size(); i++)
            if (segs[i].kind == kind && segs[i].layer == layer) return (int)i;
        return -1;
    }
    /* the host FP64 array of a per-layer segment */
    static DOUBLE *host_of(kernel_ann *k, const StateSeg &g) {
        return g.kind == SEG_W ? layer_of(k, g.layer)->weights : (g.kind == SEG_V ? k->dw : k->dv)[g.layer];
    }

    /* masters (the momentum into k->dw, Adam's second moment into k->dv and t, p1, p2) -> host
     * FP64, from the live segments or from their copies in a [keep_best] snapshot (src) */
    BOOL download(kernel_ann *k) { return download_from(k, nullptr); }
    BOOL download_from(kernel_ann *k, void *const *src) {
        HIPCHK(hipStreamSynchronize(self().s));
        if (seg(SEG_V) >= 0) ann_momentum_init(k);
        if (seg(SEG_ADAM) >= 0) ann_adam_init(k);
        for (size_t i = 0; i < segs.size(); i++) {
            const StateSeg &g = segs[i];
            const void *from = src ? src[i] : g.dev;
            if (g.kind == SEG_ADAM) {
                hpnn_adam_state st;
                HIPCHK(hipMemcpy(&st, from, sizeof st, hipMemcpyDeviceToHost));
                k->adam_t = st.t;
                k->adam_p1 = st.p1;
                k->adam_p2 = st.p2;
            } else if (g.kind != SEG_LRS && !self().to_host(host_of(k, g), from, layer_of(k, g.layer), g.layer)) {
                return FALSE;
            }
        }
        return TRUE;
    }
    /* the schedule state of the live net, or of a snapshot */
    BOOL read_schedule(void *const *src, hpnn_lr_state *out) {
        const int i = seg(SEG_LRS);
        if (i < 0) return FALSE;
        HIPCHK(hipStreamSynchronize(self().s));
        HIPCHK(hipMemcpy(out, src ? src[i] : segs[i].dev, sizeof *out, hipMemcpyDeviceToHost));
        return TRUE;
    }

    /* the replica state as bytes, and back: rank 0's state re-broadcast after an exchange fallback */
    BOOL get_state(std::vector<char> &out) {
        out.clear();
        HIPCHK(hipStreamSynchronize(self().s));
        for (const StateSeg &g : segs) {
            if (g.kind == SEG_LRS) continue;
            const size_t o = out.size();
            out.resize(o + g.bytes);
            HIPCHK(hipMemcpy(out.data() + o, g.dev, g.bytes, hipMemcpyDeviceToHost));
        }
        return TRUE;
    }
    BOOL set_state(const char *in) {
        for (const StateSeg &g : segs) {
            if (g.kind == SEG_LRS) continue;
            HIPCHK(hipMemcpy(g.dev, in, g.bytes, hipMemcpyHostToDevice));
            in += g.bytes;
        }
        return TRUE;
    }

    /* exact resume: host FP64 -> every segment of one kind */
    BOOL upload_kind(const kernel_ann *k, SegKind kind) {
        kernel_ann *kk = (kernel_ann *)k;
        for (const StateSeg &g : segs)
            if (g.kind == kind && !self().to_dev(g.dev, host_of(kk, g), layer_of(kk, g.layer), g.layer)) return FALSE;
        return TRUE;
    }
    /* the BPM momentum k->dw */
    BOOL upload_momentum(const kernel_ann *k) { return !k->dw || upload_kind(k, SEG_V); }
    /* under ADAM: both moments k->dw, k->dv and t, p1, p2 into the device state */
    BOOL upload_moments(const kernel_ann *k) {
        const int i = seg(SEG_ADAM);
        if (i < 0 || !k->dw || !k->dv) return TRUE;
        if (!upload_kind(k, SEG_V) || !upload_kind(k, SEG_A)) return FALSE;
        hpnn_adam_state st;
        HIPCHK(hipStreamSynchronize(self().s));
        HIPCHK(hipMemcpy(&st, segs[i].dev, sizeof st, hipMemcpyDeviceToHost));
        st.t = k->adam_t;
        st.p1 = k->adam_p1;
        st.p2 = k->adam_p2;
        HIPCHK(hipMemcpy(segs[i].dev, &st, sizeof st, hipMemcpyHostToDevice));
        return TRUE;
    }
};

/* BF16 batched engine: an adapter of the library's batched plan (bplan.h, the same object
 * hpnn_amd.models.MLP binds) to the precision-generic drivers below */
struct Batched : NetState<Batched> {
    typedef float target_t; /* dense targets, uploaded once */
    typedef float grad_t;   /* flat gradient buffer (the all-reduce payload) */
    static constexpr hpnn_comm_dtype comm_dt = HPNN_DT_F32;
    static const char *name() { return "bf16"; }
    static constexpr bool has_cg = false; /* [train] CG: FP64 / FP32 only (its losses need their precision) */
    /* [train] ADAM: the plan's optimizer (BPlan::set_adam, before init): V32 is the first moment,
     * A32 the second, the device state one more buffer of the plan */
    static constexpr bool has_adam = true;
    bool adam = false;
    BOOL set_adam(const hpnn_adam_state &a) {
        adam = p.set_adam(a.lr, a.beta1, a.beta2, a.eps, a.decay) == 0;
        return adam ? TRUE : FALSE;
    }
    /* [lr_schedule]: the plan's BP / BPM step reads its rate from the device state (BPlan::
     * set_schedule, before init; the buffer "lrs"); the driver launches the advance per epoch */
    bool sched = false;
    BOOL set_schedule(const hpnn_lr_state &l) {
        sched = p.set_schedule(l) == 0;
        return sched ? TRUE : FALSE;
    }
    hpnn_lr_state *lr_dev() const { return sched ? p.lrs_dev : nullptr; }
    hpnn_adam_state *adam_dev() const { return adam ? p.adam_dev : nullptr; }
    /* [clip]: the plan's optimizer step becomes partials -> finalize -> update (BPlan::set_clip,
     * behind set_adam / set_schedule and before init); the clip state is no snapshot segment */
    bool clip = false;
    BOOL set_clip(double max_norm, double lr) {
        clip = p.set_clip(max_norm, lr) == 0;
        return clip ? TRUE : FALSE;
    }
    BOOL clip_commit(hpnn_clip_record *hist, unsigned int *cursor, unsigned int cap) {
        return clip && p.commit_clip(hist, cursor, cap, s) == 0;
    }
    static constexpr size_t ACC_BYTES = HPNN_STAT_SLOTS * HPNN_STAT_STRIDE * 4;
    static int reduce_sum(grad_t *buf, int G, size_t count, hipStream_t st) {
        return hpnn_reduce_slabs(buf, G, (long)count, (long)count, buf, st);
    }
    hpnn::BPlan p;
    int L = 0, Bp = 0;
    float *acc = nullptr, *gflat = nullptr;
    size_t goff[17] = {0};
    bool fm_ok = true; /* minibatch starts are multiples of 32 rows: fragment-major inputs */
    bool own_flat = false; /* the plan owns its flat buffer (loopback re-points it) */
    hipStream_t s = nullptr;

    ~Batched() {
        if (s) hipStreamSynchronize(s);
    }

    BOOL read_stats(double *loss, unsigned int *hits) { return p.read_stats(loss, hits, s) == 0; }

    /* layer l: host FP64 [N][M] -> the zero-padded FP32 [Np][Kp] device buffer, and back */
    BOOL to_dev(void *dev, const DOUBLE *host, const layer_ann *ly, int l) {
        const int M = (int)ly->n_inputs, N = (int)ly->n_neurons, Kp = p.Kp[l];
        std::vector<float> tmp((size_t)p.Np[l] * Kp, 0.f);
        for (int n = 0; n < N; n++)
            for (int m = 0; m < M; m++) tmp[(size_t)n * Kp + m] = (float)host[(size_t)n * M + m];
        HIPCHK(hipMemcpyAsync(dev, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return TRUE;
    }
    BOOL to_host(DOUBLE *host, const void *dev, const layer_ann *ly, int l) {
        const int M = (int)ly->n_inputs, N = (int)ly->n_neurons, Kp = p.Kp[l];
        std::vector<float> tmp((size_t)p.Np[l] * Kp);
        HIPCHK(hipMemcpy(tmp.data(), dev, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (int n = 0; n < N; n++)
            for (int m = 0; m < M; m++) host[(size_t)n * M + m] = tmp[(size_t)n * Kp + m];
        return TRUE;
    }

    /* allow_fm: every minibatch (shard) this net trains starts at a row multiple of 32;
     * fused: the plan's structure request (-1 auto, 0 per-layer only) */
    BOOL init(kernel_ann *k, int B, nn_type t, bool momentum, hipStream_t st, bool allow_fm = true, int fused = -1) {
        s = st;
        L = (int)k->n_hiddens + 1;
        std::vector<int> sizes(L + 1);
        sizes[0] = (int)k->n_inputs;
        for (int l = 0; l < L; l++) sizes[l + 1] = (int)layer_of(k, l)->n_neurons;
        const int type = plan_type(t);
        std::string err;
        int rc = p.configure(sizes.data(), L, type, B, momentum, fused, nullptr, 512, true, &err);
        if (!rc && !allow_fm && p.mode == 't') /* the tile front reads fragment-major rows only */
            rc = p.configure(sizes.data(), L, type, B, momentum, 'x', nullptr, 512, true, &err);
        if (rc) {
            NN_ERROR(stderr, "batched plan: %s (%d)\n", err.c_str(), rc);
            return FALSE;
        }
        fm_ok = allow_fm;
        if (p.allocate(s)) return FALSE;
        Bp = p.Bp;
        for (int l = 0; l < L; l++) {
            const layer_ann *ly = layer_of(k, l);
            if (!to_dev(p.W32[l], ly->weights, ly, l)) return FALSE;
        }
        if (p.cast_weights(s)) return FALSE;
        if (adam && hpnn_adam_preload(s)) return FALSE;
        if ((sched || clip) && hpnn_lrsched_preload(s)) return FALSE;
        if (clip && (hpnn_clip_preload(s) || p.prepare_clip(s))) return FALSE;
        acc = p.stats;
        gflat = p.gflat;
        memcpy(goff, p.goff, sizeof goff);
        NN_DBG(stdout, "batched plan: mode %c, Bp %d, G0 splits %d\n", p.mode ? p.mode : '-', p.Bp, p.S[0]);
        segs.clear();
        for (int l = 0; l < L; l++) list_layer(l, p.W32[l], p.V32[l], p.A32[l], (size_t)p.Np[l] * p.Kp[l] * 4);
        list_tail(adam_dev(), lr_dev());
        return TRUE;
    }

    /* the training set in the plan's input layout: fragment-major for the tile front, plus a
     * fragment-major byte copy for mode 'x'; data that are all integers 0..255 (the reference's
     * pmnist pixels) go as bytes -- the same values, half the bytes of BF16 */
    BOOL upload_x(const DOUBLE *src, int rows, int cols, int rows_p, XSet *xs) {
        const int lay = fm_ok ? p.input_layout() : 0, Kp0 = p.Kp[0];
        rows_p = pad_rows(rows_p, 32);
        bool u8 = lay != 0;
        for (size_t i = 0; u8 && i < (size_t)rows * cols; i++) {
            const DOUBLE v = src[i];
            u8 = v >= 0.0 && v <= 255.0 && v == (DOUBLE)(int)v;
        }
        xs->u8 = u8 ? 1 : 0;
        xs->scale = 1.f;
        auto put = [&](const void *h, size_t bytes, void **dst) { return upload_bytes(h, bytes, dst, s); };
        if (lay == 1) {
            if (u8) {
                auto h = to_fragment_major<uint8_t>(src, rows, cols, rows_p, Kp0, [](DOUBLE v) { return (uint8_t)v; });
                xs->row_bytes = Kp0;
                return put(h.data(), h.size(), &xs->x);
            }
            auto h = to_fragment_major<uint16_t>(src, rows, cols, rows_p, Kp0,
                                                 [](DOUBLE v) { return bf16_bits((float)v); });
            xs->row_bytes = (size_t)Kp0 * 2;
            return put(h.data(), h.size() * 2, &xs->x);
        }
        if (!upload_bf16(src, rows, cols, rows_p, Kp0, &xs->x, s)) return FALSE;
        xs->row_bytes = (size_t)Kp0 * 2;
        if (lay == 2 && u8) {
            auto h = to_fragment_major<uint8_t>(src, rows, cols, rows_p, Kp0, [](DOUBLE v) { return (uint8_t)v; });
            xs->row_bytes_g = Kp0;
            return put(h.data(), h.size(), &xs->xg);
        }
        xs->u8 = 0;
        return TRUE;
    }
    /* [shuffle] epoch: the row-major canonical copies (cn) the gathers read; xs, from upload_x,
     * is the staging set in the plan's layout that the steps read */
    static constexpr bool dense_always = false; /* with labels the dense targets are not read */
    BOOL upload_canon(const DOUBLE *src, int rows, int cols, const XSet &xs, XSet *cn) {
        const int lay = fm_ok ? p.input_layout() : 0, Kp0 = p.Kp[0];
        if (xs.u8) {
            std::vector<uint8_t> h((size_t)rows * Kp0, 0);
            for (int r = 0; r < rows; r++)
                for (int c = 0; c < cols; c++) h[(size_t)r * Kp0 + c] = (uint8_t)src[(size_t)r * cols + c];
            if (!upload_bytes(h.data(), h.size(), lay == 1 ? &cn->x : &cn->xg, s)) return FALSE;
            if (lay == 1) return TRUE;
        }
        return upload_bf16(src, rows, cols, rows, Kp0, &cn->x, s);
    }
    BOOL gather(const XSet &cn, const XSet &xs, const int *perm, int n, int rows_p) {
        const int lay = fm_ok ? p.input_layout() : 0, Kp0 = p.Kp[0];
        rows_p = pad_rows(rows_p, 32);
        if (lay == 1) return hpnn_gather_fm(xs.x, cn.x, perm, n, rows_p, Kp0, xs.u8 ? 1 : 2, s) == 0;
        if (hpnn_gather_rows(xs.x, cn.x, perm, n, rows_p, (long)Kp0 * 2, s)) return FALSE;
        return !xs.xg || hpnn_gather_fm(xs.xg, cn.xg, perm, n, rows_p, Kp0, 1, s) == 0;
    }
    /* [validate]: the held-out set as BPlan::evaluate reads it -- the plan's fragment-major
     * layout padded to whole 256-row tiles on the tile path (one launch over the set), else
     * row-major BF16 padded to whole Bp-row chunks (forward + output kernel per chunk) */
    BOOL upload_val(const DOUBLE *src, int rows, int cols, XSet *vs, int *rows_p) {
        if (p.eval_is_fused()) {
            *rows_p = pad_rows(rows, 256);
            return upload_x(src, rows, cols, *rows_p, vs);
        }
        *rows_p = pad_rows(rows, p.Bp);
        vs->row_bytes = (size_t)p.Kp[0] * 2;
        return upload_bf16(src, rows, cols, *rows_p, p.Kp[0], &vs->x, s);
    }
    float *vacc() { return p.vstats; }
    /* guess (may be null): [the rows upload_val padded the set to] int32, the guess of every row;
     * chunk(row, rows): called behind the launches of every chunk ([confusion] tallies it) */
    template <class Chunk>
    BOOL evaluate(const XSet &vs, const float *T, int ldt, int nv, int *guess, Chunk &&chunk) {
        int r = 0;
        if (p.eval_is_fused()) {
            r = p.evaluate(at(vs, 0), vs.lab, vs.lab ? nullptr : T, ldt, nv, p.vstats, guess, s);
            if (!r && !chunk(0L, nv)) r = -5;
        } else {
            for (long row = 0; row < nv && !r; row += p.Bp) {
                hpnn::XIn v;
                v.x = (const char *)vs.x + row * vs.row_bytes;
                v.rowmajor = 1;
                const int *lb = vs.lab ? vs.lab + row : nullptr;
                const int rows = (int)std::min((long)p.Bp, nv - row);
                r = p.evaluate(v, lb, lb ? nullptr : T + (size_t)row * ldt, ldt, rows, p.vstats,
                               guess ? guess + row : nullptr, s);
                if (!r && !chunk(row, rows)) r = -5;
            }
        }
        if (r) NN_ERROR(stderr, "batched validation pass failed: %d\n", r);
        return r == 0;
    }
    hpnn::XIn at(const XSet &xs, long row) const {
        hpnn::XIn v;
        v.x = (const char *)xs.x + row * xs.row_bytes;
        v.xg = xs.xg ? (const char *)xs.xg + row * xs.row_bytes_g : nullptr;
        v.u8 = xs.u8;
        v.scale = xs.scale;
        return v;
    }

    BOOL step(const XSet &xs, long row, const float *T, int ldt, int n_valid, float lr, float alpha, bool) {
        const int *L = xs.lab ? xs.lab + row : nullptr;
        const int r = p.step(at(xs, row), L, L ? nullptr : T, ldt, n_valid, lr, alpha, s);
        if (r) NN_ERROR(stderr, "batched step failed: %d\n", r);
        return r == 0 && hpnn_debug_check("batched training step") == 0;
    }

    /* data parallel: gradients into the flat FP32 buffer (the all-reduce payload) */
    BOOL alloc_flat(float *external = nullptr) {
        if (external) p.gflat = external; /* loopback: replicas' buffers in one allocation */
        gflat = p.gflat;
        return TRUE;
    }
    size_t flat_count() const { return p.goff[L]; }
    template <class Ready>
    BOOL grads(const XSet &xs, long row, const float *T, int ldt, int n_valid, Ready &&ready) {
        const int *L = xs.lab ? xs.lab + row : nullptr;
        const int r = p.grads(at(xs, row), L, L ? nullptr : T, ldt, n_valid, hpnn::ReadyFn(ready), s);
        if (r) NN_ERROR(stderr, "batched gradients failed: %d\n", r);
        return r == 0;
    }
    BOOL grads(const XSet &xs, long row, const float *T, int ldt, int n_valid) {
        /* no exchange to overlap (the xGMI all-reduce of the whole buffer follows): the fused
         * modes reduce G0 and [G1|G2] inside the G0 launch */
        const int *L = xs.lab ? xs.lab + row : nullptr;
        const int r = p.grads_local(at(xs, row), L, L ? nullptr : T, ldt, n_valid, s);
        if (r != -1) {
            if (r) NN_ERROR(stderr, "batched gradients failed: %d\n", r);
            return r == 0;
        }
        return grads(xs, row, T, ldt, n_valid, [](int, int) { return true; });
    }
    std::vector<std::pair<int, int>> buckets() const { return p.buckets(); }
    BOOL update_flat(const float *G, float lr, float alpha, float scale, bool) {
        return p.update_flat(G, lr, alpha, scale, s) == 0;
    }

    /* one process per GPU: the library's data-parallel step (dp_exchange.h) */
    std::unique_ptr<hpnn::DpExchange> dpx;
    bool attach_dpx(hpnn_comm *c, int mode) {
        dpx.reset(new hpnn::DpExchange());
        if (dpx->init(&p, c, mode)) dpx.reset();
        return (bool)dpx;
    }
    BOOL dp_step(const XSet &xs, long row, const float *T, int ldt, int nv, int total, float lr, float alpha) {
        const int *L = xs.lab ? xs.lab + row : nullptr;
        return dpx && dpx->step(at(xs, row), L, L ? nullptr : T, ldt, nv, total, lr, alpha, s) == 0;
    }
    BOOL gather_masters() { return !dpx || dpx->gather_masters(s) == 0; }
    /* fused modes: front + G0 with the exchange over xk and every layer's step in the same
     * launch (BPlan::xchg_step, the Python DataParallel's path); -1 = not covered */
    int xchg_step(const XSet &xs, long row, const float *T, int ldt, int nv, float lr, float alpha, float scale,
                  hpnn_xar *xk) {
        hpnn_xar_view v;
        if (hpnn_xar_view_get(xk, &v)) return -2;
        const int *L = xs.lab ? xs.lab + row : nullptr;
        return p.xchg_step(at(xs, row), L, L ? nullptr : T, ldt, nv, lr, alpha, scale, v, s);
    }
    bool has_dpx() const { return (bool)dpx; }
    void detach_dpx() { dpx.reset(); }

    /* FALSE when an in-kernel hand-off (fused G0 split-K tickets, fused TN tickets, the wide
     * front's tile pair) timed out since the plan was made: that launch stepped with partial
     * sums, so training must not go on from those weights (reference: CHK_ERR after every
     * launch, common.h:324-335) */
    static BOOL handoff_timed_out() {
        NN_ERROR(stderr, "batched GPU training: an in-kernel split-K / tile hand-off timed out "
                         "(the step used partial sums); stopping\n");
        return FALSE;
    }
    BOOL healthy() { return p.health(s) == 0 ? TRUE : handoff_timed_out(); }
    /* healthy() in two halves: enqueue the readback into d[0..2] (pinned, zeroed), judge it
     * once an event after it has completed */
    bool health_enqueue(unsigned int *d) { return p.health_enqueue(s, d) == 0; }
    BOOL health_ok(const unsigned int *d) { return (d[0] || d[1] || d[2]) ? handoff_timed_out() : TRUE; }
    /* digest of the weights every data-parallel replica must hold bit for bit: the BF16 copies,
     * plus the FP32 masters unless the BF16 reduce-scatter step keeps them sharded */
    BOOL digest(unsigned long long *d) {
        bool sh = false;
        for (int l = 0; dpx && l < L; l++) sh = sh || dpx->sharded(l);
        return p.weights_digest(sh ? 1 : 3, d, s) == 0;
    }

    /* a state from another replica: the BF16 copies are re-derived from the masters */
    BOOL set_state(const char *in) {
        return NetState::set_state(in) && p.cast_weights(s) == 0 && hipStreamSynchronize(s) == hipSuccess;
    }
};

/* FP64 / FP32 batched engine ([dtype] f64 | f32): the reference's precision (the
 * reference computes in double throughout, cuda_ann.cu:41-148, 546-548, 2139-2142) on the
 * FP64 / FP32 MFMA kernels of kernels_fp.hip.  Same minibatch semantics as the FP64 CPU
 * oracle (cpu_batched.cpp) and as Batched: forward, output delta, deltas with the
 * pre-update weights, G = sum over the batch, W updated with scale = 1 / n_valid.  No
 * padding: the kernels take any shape; the backward delta reads W itself (transposed
 * operand), so no W^T copy is kept. */
template <typename T>
struct BatchedFP : NetState<BatchedFP<T>> {
    typedef T target_t;
    typedef T grad_t;
    static constexpr int F64 = sizeof(T) == 8 ? 1 : 0;
    static constexpr hpnn_comm_dtype comm_dt = sizeof(T) == 8 ? HPNN_DT_F64 : HPNN_DT_F32;
    static const char *name() { return sizeof(T) == 8 ? "f64" : "f32"; }
    static constexpr size_t ACC_BYTES = Batched::ACC_BYTES;
    int L = 0, Bp = 0, n_out = 0, type = 2;
    int M[16], N[16], S[16];
    int Kp[16]; /* Kp[0] = n_in: the row pitch of the uploaded input (drivers index rows by it) */
    T *W[16] = {0}, *V[16] = {0}, *slab[16] = {0}, *H[16] = {0}, *D[16] = {0};
    T *Z = nullptr, *gflat = nullptr;
    float *acc = nullptr;
    bool own_flat = false;
    size_t goff[17] = {0};
    hipStream_t s = nullptr;

    BOOL upload_x(const DOUBLE *src, int rows, int cols, int rows_p, XSet *xs) {
        std::vector<T> h((size_t)rows_p * cols, (T)0);
        for (size_t i = 0; i < (size_t)rows * cols; i++) h[i] = (T)src[i];
        xs->row_bytes = (size_t)cols * sizeof(T);
        return upload_bytes(h.data(), h.size() * sizeof(T), &xs->x, s);
    }
    static constexpr bool dense_always = true;
    BOOL upload_canon(const DOUBLE *src, int rows, int cols, const XSet &, XSet *cn) {
        return upload_x(src, rows, cols, rows, cn);
    }
    BOOL gather(const XSet &cn, const XSet &xs, const int *perm, int n, int rows_p) {
        return hpnn_gather_rows(xs.x, cn.x, perm, n, rows_p, (long)xs.row_bytes, s) == 0;
    }
    static const void *at(const XSet &xs, long row) { return (const char *)xs.x + row * xs.row_bytes; }
    static int reduce_sum(grad_t *buf, int G, size_t count, hipStream_t st) {
        return hpnn_reduce_fp(F64, buf, buf, G, (long)count, (long)count, st);
    }
    /* [validate]: the held-out rows as they are (the kernels take any shape) and stat slots of
     * the pass's own; forward + the output kernel without a delta, in chunks of Bp rows */
    float *vslots = nullptr;
    BOOL upload_val(const DOUBLE *src, int rows, int cols, XSet *vs, int *rows_p) {
        *rows_p = rows;
        if (!vslots) {
            HIPCHK(hpnn_dev_malloc(&vslots, ACC_BYTES));
            HIPCHK(hipMemsetAsync(vslots, 0, ACC_BYTES, s));
        }
        return upload_x(src, rows, cols, rows, vs);
    }
    float *vacc() { return vslots; }

    /* [train] CG (kernels_cg.hip, docs/DESIGN.md 3.2h): g, g_prev, d and W0 beside the weights in
     * one allocation (each layer's piece 256-byte aligned), the segment table, the device state
     * and history, the partials of the dot products and stat slots of CG's own -- allocated by
     * init_cg only */
    static constexpr bool has_cg = true;
    DevBuf<char> cg_mem;
    DevBuf<hpnn_cg_seg> cg_table;
    DevBuf<hpnn_cg_state> cg_state;
    DevBuf<hpnn_cg_record> cg_hist;
    DevBuf<double> cg_part;
    DevBuf<float> cg_slots;
    BOOL init_cg(double a_init, UINT n, UINT iterations) {
        size_t off[17] = {0};
        for (int l = 0; l < L; l++) off[l + 1] = off[l] + ((size_t)N[l] * M[l] * sizeof(T) + 255) / 256 * 256;
        HIPCHK(cg_mem.alloc(4 * off[L]));
        HIPCHK(hipMemsetAsync(cg_mem.get(), 0, 4 * off[L], s)); /* g_prev = d = 0: the first dots are finite */
        HIPCHK(cg_table.alloc(L));
        HIPCHK(cg_state.alloc(1));
        HIPCHK(cg_hist.alloc(iterations ? iterations : 1));
        HIPCHK(cg_part.alloc(3 * HPNN_CG_DOT_WGS));
        HIPCHK(cg_slots.alloc(ACC_BYTES / sizeof(float)));
        HIPCHK(hipMemsetAsync(cg_slots.get(), 0, ACC_BYTES, s));
        HIPCHK(hipMemsetAsync(cg_hist.get(), 0, (iterations ? iterations : 1) * sizeof(hpnn_cg_record), s));
        std::vector<hpnn_cg_seg> h(L);
        for (int l = 0; l < L; l++) {
            char *b = cg_mem.get() + off[l];
            h[l] = {W[l], b, b + off[L], b + 2 * off[L], b + 3 * off[L], slab[l], S[l], (long)N[l] * M[l],
                    (unsigned long long)N[l] * M[l]};
        }
        hpnn_cg_state st;
        hpnn_cg_state_init(&st, a_init, n, iterations);
        HIPCHK(hipMemcpyAsync(cg_state.get(), &st, sizeof st, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        if (hpnn_cg_table(F64, cg_table.get(), h.data(), L, s)) {
            NN_ERROR(stderr, "[train] CG: the segment table was refused (alignment or too many layers)\n");
            return FALSE;
        }
        return hpnn_cg_preload(s) == 0;
    }
    /* the forward-only loss of the training set into CG's slots: whole Bp-row chunks, as the
     * gradient pass forwards them, so f0 and a trial at the same weights are the same number */
    BOOL evaluate_cg(const XSet &xs, const T *Tt, int ldt, int n) {
        for (long row = 0; row < n; row += Bp) {
            if (!forward(at(xs, row), Bp)) return FALSE;
            if (hpnn_cg_loss(F64, Z, N[L - 1], Tt + (size_t)row * ldt, ldt, cg_slots.get(),
                             (int)std::min((long)Bp, n - row), n_out, type, s))
                return FALSE;
        }
        return TRUE;
    }
    /* one CG iteration over the n resident samples (xs / Tt padded to whole Bp-row chunks): every
     * launch on the stream, every decision on the device */
    BOOL iterate_cg(const XSet &xs, const T *Tt, int ldt, int n) {
        hpnn_cg_seg *tb = cg_table.get();
        hpnn_cg_state *st = cg_state.get();
        for (long row = 0; row < n; row += Bp) {
            const int nv = (int)std::min((long)Bp, n - row);
            const T *tr = Tt + (size_t)row * ldt;
            if (!backprop(at(xs, row), tr, ldt, nv)) return FALSE;
            if (hpnn_cg_loss(F64, Z, N[L - 1], tr, ldt, cg_slots.get(), nv, n_out, type, s) ||
                hpnn_cg_accumulate(F64, tb, L, row == 0, row + Bp >= n ? 1.0 / (double)n : 1.0, s))
                return FALSE;
        }
        if (hpnn_cg_file(cg_slots.get(), st, cg_hist.get(), HPNN_CG_FINAL, s) ||
            hpnn_cg_dots(F64, tb, L, cg_part.get(), st, s) || hpnn_cg_direction(st, s) ||
            hpnn_cg_begin(F64, tb, L, st, s))
            return FALSE;
        for (int j = 0; j <= HPNN_CG_FINAL; j++) {
            if (hpnn_cg_trial(F64, tb, L, st, j, s)) return FALSE;
            if (j == HPNN_CG_FINAL) break;
            if (!evaluate_cg(xs, Tt, ldt, n) || hpnn_cg_file(cg_slots.get(), st, cg_hist.get(), j, s)) return FALSE;
        }
        return hpnn_debug_check("batched CG iteration (fp)") == 0;
    }
    /* the records filed so far (synchronises) */
    BOOL read_cg(std::vector<hpnn_cg_record> &out) {
        hpnn_cg_state st;
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(&st, cg_state.get(), sizeof st, hipMemcpyDeviceToHost));
        out.resize(std::min(st.cursor, st.cap));
        if (!out.empty())
            HIPCHK(hipMemcpy(out.data(), cg_hist.get(), out.size() * sizeof(hpnn_cg_record), hipMemcpyDeviceToHost));
        return TRUE;
    }

    /* [train] ADAM (kernels_adam.hip, docs/DESIGN.md 3.2i): V[l] is the first moment, A2[l] the
     * second, both zeroed; the segment table and the device state -- allocated by init_adam only
     * (init was given momentum = true, so V exists) */
    static constexpr bool has_adam = true;
    T *A2[16] = {0};
    DevBuf<hpnn_adam_seg> adam_table;
    DevBuf<hpnn_adam_state> adam_state;
    bool adam = false, adam_req = false;
    hpnn_adam_state adam_cfg;
    BOOL set_adam(const hpnn_adam_state &a) { /* before init (given momentum = true): it ends in init_adam */
        adam_cfg = a;
        adam_req = true;
        return TRUE;
    }
    BOOL init_adam(const hpnn_adam_state &st0) {
        std::vector<hpnn_adam_seg> h(L);
        for (int l = 0; l < L; l++) {
            const size_t nw = (size_t)N[l] * M[l];
            if (!V[l]) return FALSE;
            HIPCHK(hpnn_dev_malloc(&A2[l], nw * sizeof(T)));
            HIPCHK(hipMemsetAsync(A2[l], 0, nw * sizeof(T), s));
            h[l] = {W[l], V[l], A2[l], slab[l], S[l], 0, 0, 0, (long)nw, (unsigned long long)nw};
        }
        HIPCHK(adam_table.alloc(L));
        HIPCHK(adam_state.alloc(1));
        HIPCHK(hipMemcpyAsync(adam_state.get(), &st0, sizeof st0, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        if (hpnn_adam_table(F64, adam_table.get(), h.data(), L, s)) {
            NN_ERROR(stderr, "[train] ADAM: the segment table was refused (alignment or too many layers)\n");
            return FALSE;
        }
        adam = true;
        return hpnn_adam_preload(s) == 0;
    }

    /* [lr_schedule] (kernels_lrsched.hip, docs/DESIGN.md 3.2j): the device state, and for BP / BPM
     * the segment table of the one update launch that reads its rate from it -- allocated only
     * when scheduled (init_schedule, at the end of init) */
    DevBuf<hpnn_sched_seg> sched_table;
    DevBuf<hpnn_lr_state> sched_state;
    bool sched = false, sched_req = false;
    hpnn_lr_state sched_cfg;
    BOOL set_schedule(const hpnn_lr_state &l) { /* before init */
        if (!hpnn_lr_valid(&l)) return FALSE;
        sched_cfg = l;
        sched_req = true;
        return TRUE;
    }
    hpnn_lr_state *lr_dev() const { return sched ? sched_state.get() : nullptr; }
    hpnn_adam_state *adam_dev() const { return adam ? adam_state.get() : nullptr; }
    /* the device state and, for BP / BPM, the table of the scheduled update ([clip] alone: a constant rate) */
    BOOL init_sched_buffers(const hpnn_lr_state &cfg, bool momentum) {
        HIPCHK(sched_state.alloc(1));
        HIPCHK(hipMemcpyAsync(sched_state.get(), &cfg, sizeof cfg, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!adam_req) {
            std::vector<hpnn_sched_seg> h(L);
            for (int l = 0; l < L; l++) {
                const size_t nw = (size_t)N[l] * M[l];
                h[l] = {W[l], momentum ? V[l] : nullptr, slab[l], S[l], 0, 0, 0, (long)nw, (unsigned long long)nw};
            }
            HIPCHK(sched_table.alloc(L));
            if (hpnn_sgd_sched_table(F64, sched_table.get(), h.data(), L, momentum ? 1 : 0, s)) {
                NN_ERROR(stderr, "[lr_schedule]: the segment table was refused (alignment or too many layers)\n");
                return FALSE;
            }
        }
        return hpnn_lrsched_preload(s) == 0;
    }
    BOOL init_schedule(bool momentum) {
        if (!init_sched_buffers(sched_cfg, momentum)) return FALSE;
        sched = true;
        return TRUE;
    }

    /* [clip] (kernels_clip.hip, docs/DESIGN.md 3.2k): the device state, the partials and the
     * segment table of the global-norm reduction -- allocated only when clipping (init_clip, at the
     * end of init).  The step is backprop -> partials -> finalize -> the update launch of
     * [lr_schedule] / ADAM with the factor; plain BP / BPM runs the scheduled launch on a
     * constant-kind state that holds lr.  Nothing here is carried from step to step: the clip
     * state is no snapshot segment */
    DevBuf<hpnn_gnorm_seg> clip_table;
    DevBuf<hpnn_clip_state> clip_state;
    DevBuf<double> clip_part;
    int clip_count = 0;
    bool clip = false, clip_req = false;
    double clip_max = 0.0, clip_lr = 0.0;
    long clip_launches = 0;
    BOOL set_clip(double max_norm, double lr) { /* before init */
        if (!hpnn_clip_valid(max_norm) || max_norm == 0.0) return FALSE;
        clip_max = max_norm;
        clip_lr = lr;
        clip_req = true;
        return TRUE;
    }
    hpnn_clip_state *clip_dev() const { return clip ? clip_state.get() : nullptr; }
    BOOL init_clip(bool momentum) {
        if (!adam_req && !sched_req) {
            hpnn_lr_state c;
            hpnn_lr_state_init(&c, HPNN_LR_CONSTANT, clip_lr, HPNN_LR_GAMMA, HPNN_LR_PERIOD, 0u, 0.0, 0.0,
                               HPNN_LR_PATIENCE, 0u, 0u);
            if (!init_sched_buffers(c, momentum)) return FALSE;
        }
        std::vector<hpnn_gnorm_seg> h(L);
        for (int l = 0; l < L; l++) {
            const size_t nw = (size_t)N[l] * M[l];
            h[l] = {slab[l], (long)nw, (unsigned long long)nw, S[l], 0};
        }
        hpnn_clip_state c0;
        hpnn_clip_state_init(&c0, clip_max);
        HIPCHK(clip_table.alloc(L));
        HIPCHK(clip_state.alloc(1));
        HIPCHK(hipMemcpyAsync(clip_state.get(), &c0, sizeof c0, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        if (hpnn_gnorm_table(F64, clip_table.get(), h.data(), L, &clip_count, s)) {
            NN_ERROR(stderr, "[clip]: the segment table was refused (alignment or too many layers)\n");
            return FALSE;
        }
        HIPCHK(clip_part.alloc(clip_count));
        clip = true;
        return hpnn_clip_preload(s) == 0;
    }
    /* behind backprop: the global norm of the gradient as the update sees it, and the factor */
    BOOL clip_factor(double scale) {
        if (!clip) return TRUE;
        clip_launches += 2;
        return hpnn_gnorm_partials(F64, 0, clip_table.get(), L, clip_count, scale, clip_part.get(), s) == 0 &&
               hpnn_clip_finalize_dev(clip_part.get(), clip_count, clip_state.get(), s) == 0;
    }
    BOOL clip_commit(hpnn_clip_record *hist, unsigned int *cursor, unsigned int cap) {
        clip_launches++;
        return clip && hpnn_clip_commit_dev(clip_state.get(), hist, cursor, cap, s) == 0;
    }

    /* guess (may be null): [nv] int32, the guess of every row; chunk(row, rows): called behind the
     * launches of every chunk ([confusion] tallies it) */
    template <class Chunk>
    BOOL evaluate(const XSet &vs, const T *Tt, int ldt, int nv, int *guess, Chunk &&chunk) {
        for (long row = 0; row < nv; row += Bp) {
            const int rows = (int)std::min((long)Bp, nv - row);
            if (!forward(at(vs, row), rows)) return FALSE;
            if (hpnn_output_fp_eval(F64, Z, N[L - 1], Tt + (size_t)row * ldt, ldt, guess ? guess + row : nullptr,
                                    vslots, rows, rows, n_out, type, s))
                return FALSE;
            if (!chunk(row, rows)) return FALSE;
        }
        return TRUE;
    }

    ~BatchedFP() {
        if (s) hipStreamSynchronize(s);
        if (dig) hpnn_dev_free(dig);
        for (int l = 0; l < 16; l++) {
            hpnn_dev_free(W[l]);
            hpnn_dev_free(V[l]);
            hpnn_dev_free(A2[l]);
            hpnn_dev_free(slab[l]);
            hpnn_dev_free(H[l]);
            hpnn_dev_free(D[l]);
        }
        hpnn_dev_free(Z);
        hpnn_dev_free(acc);
        hpnn_dev_free(vslots);
        if (own_flat) hpnn_dev_free(gflat);
    }

    BOOL read_stats(double *loss, unsigned int *hits) { return read_stat_slots(acc, s, loss, hits); }

    BOOL init(kernel_ann *k, int B, nn_type t, bool momentum, hipStream_t st, bool = true, int = -1) {
        s = st;
        L = (int)k->n_hiddens + 1;
        Bp = B;
        n_out = (int)k->n_outputs;
        type = plan_type(t);
        for (int l = 0; l < L; l++) {
            layer_ann *ly = layer_of(k, l);
            M[l] = (int)ly->n_inputs;
            N[l] = (int)ly->n_neurons;
            Kp[l] = M[l];
            S[l] = fp_splits(N[l], M[l], Bp);
            const size_t nw = (size_t)N[l] * M[l];
            HIPCHK(hpnn_dev_malloc(&W[l], nw * sizeof(T)));
            HIPCHK(hpnn_dev_malloc(&slab[l], nw * sizeof(T) * S[l]));
            if (momentum) {
                HIPCHK(hpnn_dev_malloc(&V[l], nw * sizeof(T)));
                HIPCHK(hipMemsetAsync(V[l], 0, nw * sizeof(T), s));
            }
            HIPCHK(hpnn_dev_malloc(&D[l], (size_t)Bp * N[l] * sizeof(T)));
            if (l < L - 1) HIPCHK(hpnn_dev_malloc(&H[l], (size_t)Bp * N[l] * sizeof(T)));
            if (!to_dev(W[l], ly->weights, ly, l)) return FALSE;
        }
        HIPCHK(hpnn_dev_malloc(&Z, (size_t)Bp * N[L - 1] * sizeof(T)));
        HIPCHK(hpnn_dev_malloc(&acc, ACC_BYTES));
        HIPCHK(hipMemsetAsync(acc, 0, ACC_BYTES, s));
        if (adam_req && !init_adam(adam_cfg)) return FALSE;
        if (sched_req && !init_schedule(momentum)) return FALSE;
        if (clip_req && !init_clip(momentum)) return FALSE;
        this->segs.clear();
        for (int l = 0; l < L; l++) this->list_layer(l, W[l], V[l], A2[l], (size_t)N[l] * M[l] * sizeof(T));
        this->list_tail(adam_dev(), lr_dev());
        return TRUE;
    }

    /* layer l: host FP64 [N][M] -> the device matrix of T (a cast; no padding), and back */
    BOOL to_dev(void *dev, const DOUBLE *host, const layer_ann *, int l) {
        const size_t nw = (size_t)N[l] * M[l];
        std::vector<T> tmp(nw);
        for (size_t i = 0; i < nw; i++) tmp[i] = (T)host[i];
        HIPCHK(hipMemcpyAsync(dev, tmp.data(), nw * sizeof(T), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return TRUE;
    }
    BOOL to_host(DOUBLE *host, const void *dev, const layer_ann *, int l) {
        const size_t nw = (size_t)N[l] * M[l];
        std::vector<T> tmp(nw);
        HIPCHK(hipMemcpy(tmp.data(), dev, nw * sizeof(T), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nw; i++) host[i] = (DOUBLE)tmp[i];
        return TRUE;
    }

    BOOL forward(const void *X, int rows) {
        for (int l = 0; l < L; l++) {
            const T *A = l ? H[l - 1] : (const T *)X;
            const bool last = l == L - 1;
            int r = hpnn_gemm_fp(F64, A, M[l], 0, W[l], M[l], 0, last ? (void *)Z : H[l], N[l], nullptr, 0, rows, N[l],
                                 M[l], last ? HPNN_EPI_NONE : HPNN_EPI_ACT, 1, 0, s);
            if (r) {
                NN_ERROR(stderr, "gemm_fp (fwd layer %d) failed: %d\n", l, r);
                return FALSE;
            }
        }
        return TRUE;
    }

    /* forward + output delta + hidden deltas + weight gradients (slab[l], S[l] slabs) */
    BOOL backprop(const void *X, const T *Tt, int ldt, int n_valid) {
        if (!forward(X, Bp)) return FALSE;
        if (hpnn_output_fp(F64, Z, N[L - 1], Tt, ldt, D[L - 1], N[L - 1], nullptr, 0, nullptr, acc,
                           (unsigned int *)(acc + 1), Bp, n_valid, n_out, type, s))
            return FALSE;
        for (int l = L - 1; l >= 1; l--) {
            /* D[l-1] = (D[l] W_l) * f'(H[l-1]): B(n = input m, k = neuron j) = W_l[j][m] */
            if (hpnn_gemm_fp(F64, D[l], N[l], 0, W[l], M[l], 1, D[l - 1], N[l - 1], H[l - 1], N[l - 1], Bp, M[l], N[l],
                             HPNN_EPI_DACT, 1, 0, s))
                return FALSE;
        }
        for (int l = 0; l < L; l++) {
            /* G[n][m] = sum_b D[b][n] H[b][m]: both operands transposed (k = the batch row) */
            const T *Hin = l ? H[l - 1] : (const T *)X;
            if (hpnn_gemm_fp(F64, D[l], N[l], 1, Hin, M[l], 1, slab[l], M[l], nullptr, 0, N[l], M[l], Bp,
                             HPNN_EPI_NONE, S[l], (long)N[l] * M[l], s))
                return FALSE;
        }
        return TRUE;
    }

    /* one minibatch under every optimizer: backprop -> the clip factor ([clip]) -> the update */
    BOOL step(const XSet &xs, long row, const T *Tt, int ldt, int n_valid, double lr, double alpha, bool mom) {
        const double scale = 1.0 / (double)n_valid;
        return backprop(at(xs, row), Tt, ldt, n_valid) && clip_factor(scale) && update(scale, lr, alpha, mom);
    }
    /* ADAM: the advance plus one launch over every layer; a device rate ([lr_schedule], [clip]):
     * one launch over every layer; plain BP / BPM: one launch per layer with the host's rate */
    BOOL update(double scale, double lr, double alpha, bool mom) {
        if (adam) {
            if (hpnn_adam_advance_dev(adam_state.get(), s) ||
                hpnn_adam_fp_clip(F64, adam_table.get(), L, scale, adam_state.get(), clip_dev(), s))
                return FALSE;
            return hpnn_debug_check("batched Adam step (fp)") == 0;
        }
        if (sched || clip) {
            if (hpnn_sgd_sched_fp_clip(F64, sched_table.get(), L, scale, alpha, mom ? 1 : 0, sched_state.get(),
                                       clip_dev(), s))
                return FALSE;
            return hpnn_debug_check("batched scheduled step (fp)") == 0;
        }
        for (int l = 0; l < L; l++)
            if (hpnn_update_fp(F64, W[l], V[l], slab[l], S[l], (long)N[l] * M[l], (long)N[l] * M[l], lr, alpha, scale,
                               mom ? 1 : 0, s))
                return FALSE;
        return hpnn_debug_check("batched training step (fp)") == 0;
    }

    BOOL alloc_flat(T *external = nullptr) {
        goff[0] = 0;
        for (int l = 0; l < L; l++) goff[l + 1] = goff[l] + (size_t)N[l] * M[l];
        if (external) {
            gflat = external;
            own_flat = false;
            return TRUE;
        }
        HIPCHK(hpnn_dev_malloc(&gflat, goff[L] * sizeof(T)));
        own_flat = true;
        return TRUE;
    }
    size_t flat_count() const { return goff[L]; }

    template <class Ready>
    BOOL grads(const XSet &xs, long row, const T *Tt, int ldt, int n_valid, Ready &&ready) {
        const void *X = at(xs, row);
        if (!forward(X, Bp)) return FALSE;
        if (hpnn_output_fp(F64, Z, N[L - 1], Tt, ldt, D[L - 1], N[L - 1], nullptr, 0, nullptr, acc,
                           (unsigned int *)(acc + 1), Bp, n_valid, n_out, type, s))
            return FALSE;
        for (int l = L - 1; l >= 0; l--) {
            if (l >= 1 && hpnn_gemm_fp(F64, D[l], N[l], 0, W[l], M[l], 1, D[l - 1], N[l - 1], H[l - 1], N[l - 1], Bp,
                                       M[l], N[l], HPNN_EPI_DACT, 1, 0, s))
                return FALSE;
            const T *Hin = l ? H[l - 1] : (const T *)X;
            if (hpnn_gemm_fp(F64, D[l], N[l], 1, Hin, M[l], 1, slab[l], M[l], nullptr, 0, N[l], M[l], Bp,
                             HPNN_EPI_NONE, S[l], (long)N[l] * M[l], s) ||
                hpnn_reduce_fp(F64, gflat + goff[l], slab[l], S[l], (long)N[l] * M[l], (long)N[l] * M[l], s))
                return FALSE;
            if (!ready(l, l)) return FALSE;
        }
        return TRUE;
    }
    BOOL grads(const XSet &xs, long row, const T *Tt, int ldt, int n_valid) {
        return grads(xs, row, Tt, ldt, n_valid, [](int, int) { return true; });
    }
    std::vector<std::pair<int, int>> buckets() const {
        std::vector<std::pair<int, int>> v;
        for (int l = L - 1; l >= 0; l--) v.push_back({l, l});
        return v;
    }

    BOOL update_flat(const T *G, double lr, double alpha, double scale, bool mom) {
        for (int l = 0; l < L; l++)
            if (hpnn_update_fp(F64, W[l], V[l], G + goff[l], 1, 0, (long)N[l] * M[l], lr, alpha, scale, mom ? 1 : 0, s))
                return FALSE;
        return TRUE;
    }

    bool attach_dpx(hpnn_comm *, int) { return false; } /* FP32 / FP64: the generic bucket loop */
    BOOL dp_step(const XSet &, long, const T *, int, int, int, double, double) { return FALSE; }
    int xchg_step(const XSet &, long, const T *, int, int, double, double, double, hpnn_xar *) { return -1; }
    BOOL gather_masters() { return TRUE; }
    BOOL healthy() { return TRUE; } /* no in-kernel hand-offs in the FP64 / FP32 kernels */
    bool health_enqueue(unsigned int *) { return true; }
    BOOL health_ok(const unsigned int *) { return TRUE; }
    unsigned long long *dig = nullptr; /* device word of digest() */
    BOOL digest(unsigned long long *d) {
        if (!dig && hpnn_dev_malloc((void **)&dig, 8) != hipSuccess) return FALSE;
        if (hipMemsetAsync(dig, 0, 8, s) != hipSuccess) return FALSE;
        long base = 0;
        for (int l = 0; l < L; l++) {
            const long nb = (long)N[l] * M[l] * (long)sizeof(T);
            if (hpnn_hash_words(W[l], nb, base, dig, s) != 0) return FALSE;
            base += nb / 4;
        }
        return hipMemcpyAsync(d, dig, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    bool has_dpx() const { return false; }
    void detach_dpx() {}
};

/* the one dtype switch: calls f(NetTag<Net>()) with the adapter of `dt` */
template <class N>
struct NetTag {
    typedef N type;
};
template <class F>
BOOL with_net(nn_dtype dt, F &&f) {
    if (dt == NN_DTYPE_BF16) return f(NetTag<Batched>());
    if (dt == NN_DTYPE_F32) return f(NetTag<BatchedFP<float>>());
    return f(NetTag<BatchedFP<double>>());
}

}  // namespace eng
}  // namespace hpnn
#endif
