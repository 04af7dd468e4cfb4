/*
 * libhpnn batched GPU engine -- training on ONE device: the resident sample set, [shuffle]
 * epoch, [validate] N, [keep_best] / [patience], the epochs as HIP graph replays and the
 * deferred health readback.
 */
#include <algorithm>
#include <chrono>
#include <map>

#include "../core/export_records.h"
#include "batched_net.h"

using namespace hpnn::eng;

namespace {

/* the device side of a run that collect() reads back (no two members of one type) */
template <class Net>
struct RunDev {
    Net &net;
    hipStream_t s;
    const hpnn_batched_opts *o;
    const std::vector<UINT> &vsched; /* the absolute epoch of every scheduled validation pass */
    const BestSnap *best;            /* null without [keep_best] */
    const DevHistory<hpnn_val_record> &vh;
    const DevHistory<double> &lrh;
    const DevHistory<hpnn_clip_record> &clh;
    const ClassTally *tally; /* null without [confusion] */
};

/* what collect() reads: the best state and the histories, each up to the last epoch that counts */
struct RunRecords {
    hpnn_best_state hb = {};
    std::vector<hpnn_val_record> vrec; /* with per-epoch metrics the replay loop reads pass vdone itself */
    size_t vdone = 0;
    std::vector<hpnn_cg_record> crec;
    double cg_f0 = 0.0; /* [train] CG: the FP64 loss of the last iteration run */
    std::vector<double> lrec;
    std::vector<hpnn_clip_record> clrec;
    hpnn_lr_state lrs; /* the schedule state of the returned kernel */
    /* [confusion]: one per-class record per pass of vrec; the matrix of the last of them (empty when
     * the device went on past it after a stop) and of the best pass (empty: none) */
    std::vector<unsigned int> pcrec, mlast, mbest;
};

/* after the last of the e epochs run: every read-back, once, with its "filed" check */
template <class Net>
BOOL collect(const RunDev<Net> &d, int e, bool metrics, RunRecords *r) {
    const hpnn_batched_opts *o = d.o;
    hpnn_best_state &hb = r->hb;
    std::vector<hpnn_val_record> &vrec = r->vrec;
    r->lrs = o->lrs;
    if (d.best && (hipStreamSynchronize(d.s) != hipSuccess ||
                   hipMemcpy(&hb, d.best->state.get(), sizeof hb, hipMemcpyDeviceToHost) != hipSuccess))
        return FALSE;
    /* the passes up to the stopping one: the best pass and the stale ones behind it (those the
     * replays filed after it are not reported) */
    const size_t judged = hb.valid ? (size_t)hb.index + 1 + hb.stale : (size_t)hb.stale;
    const bool validate = !d.vsched.empty();
    if (validate && !metrics) {
        /* the whole history, once; the cursor tells how many passes were filed */
        unsigned int filed = 0;
        if (!d.vh.read(d.s, &vrec, &filed)) return FALSE;
        if (hb.stop ? filed < judged || judged > vrec.size() : filed != vrec.size()) {
            NN_ERROR(stderr, "batched GPU training: %u validation records filed, %zu scheduled%s\n", filed,
                     vrec.size(), hb.stop ? " (stopped early)" : "");
            return FALSE;
        }
        r->vdone = hb.stop ? judged : vrec.size();
    }
    if (validate) vrec.resize(std::min(r->vdone, vrec.size()));
    /* the epochs of the call that count: after a stop those up to the stopping pass's */
    const size_t counted = hb.stop && !vrec.empty() ? d.vsched[vrec.size() - 1] - o->epoch0 : (size_t)e;
    if constexpr (Net::has_cg) {
        if (o->train == NN_TRAIN_CG) {
            if (!d.net.read_cg(r->crec)) return FALSE;
            if (r->crec.size() < (size_t)e) {
                NN_ERROR(stderr, "batched GPU training: %zu CG records filed, %d iterations run\n", r->crec.size(), e);
                return FALSE;
            }
            if (e > 0) r->cg_f0 = r->crec[e - 1].f0;
            r->crec.resize(counted);
        }
    }
    auto read = [&](const auto &h, auto *rec, const char *what) {
        unsigned int filed = 0;
        if (!h.read(d.s, rec, &filed)) return false;
        if (filed < (unsigned int)e) {
            NN_ERROR(stderr, "batched GPU training: %u %s filed, %d epochs run\n", filed, what, e);
            return false;
        }
        rec->resize(counted);
        return true;
    };
    /* [lr_schedule]: the rates, and the state of the best pass under [keep_best]; [clip]: the records */
    if (o->sched && !(read(d.lrh, &r->lrec, "learning rates") &&
                      d.net.read_schedule(hb.valid ? d.best->dst.data() : nullptr, &r->lrs)))
        return FALSE;
    if (o->clip > 0.0 && !read(d.clh, &r->clrec, "clip records")) return FALSE;
    if (d.tally) {
        /* the device cursor after the last replay: `last` is the pass of that cursor, which is the
         * last pass reported unless the replays ran on past a stopping pass */
        unsigned int filed = 0;
        if (hipStreamSynchronize(d.s) != hipSuccess ||
            hipMemcpy(&filed, d.vh.cursor(), sizeof filed, hipMemcpyDeviceToHost) != hipSuccess)
            return FALSE;
        const bool last_is_reported = !vrec.empty() && filed == vrec.size();
        if (!d.tally->read(vrec.size(), &r->pcrec, &r->mlast, hb.valid ? &r->mbest : nullptr)) return FALSE;
        if (!last_is_reported) r->mlast.clear();
    }
    return TRUE;
}


template <class Net>
BOOL train_single_t(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                    hpnn_batched_stats *st) {
    typedef typename Net::target_t TT;
    if (k->n_hiddens + 1 > 16) return FALSE;
    hpnn_gpu_sync_host(k);
    HIPCHK(hipSetDevice(hpnn_rt_device(0)));
    hipStream_t s = hpnn_rt_stream(0, 0);
    const int B = (int)(o->batch ? o->batch : 256);
    const bool mom = o->train == NN_TRAIN_BPM;
    const bool cg = o->train == NN_TRAIN_CG;
    if (cg && !Net::has_cg) {
        NN_ERROR(stderr, "[train] CG: the line search compares losses that the BF16 forward cannot resolve; "
                         "use [dtype] f32 or f64\n");
        return FALSE;
    }
    const bool adam = o->train == NN_TRAIN_ADAM;
    if (adam && !hpnn_adam_valid(o->lr, o->beta1, o->beta2, o->eps, o->decay)) {
        NN_ERROR(stderr, "[train] ADAM: needs 0 <= beta1, beta2 < 1, epsilon > 0, decay >= 0\n");
        return FALSE;
    }
    const int n_in = (int)k->n_inputs, n_out = (int)k->n_outputs;
    Net net;
    /* [train] ADAM: the moments beside the masters and the device state the update launches read
     * when they run; zero and t = 0 unless the call resumes a loaded state */
    if (adam) {
        hpnn_adam_state ast;
        hpnn_adam_state_init(&ast, o->lr, o->beta1, o->beta2, o->eps, o->decay);
        if (!net.set_adam(ast)) return FALSE;
    }
    /* [lr_schedule]: the device state every update launch reads its rate from, a history of one
     * rate per epoch; allocated only when scheduled */
    const bool sched = o->sched != 0;
    if (sched && cg) {
        NN_ERROR(stderr, "[lr_schedule] is not supported by [train] CG (the line search chooses its own step)\n");
        return FALSE;
    }
    if (sched && !net.set_schedule(o->lrs)) {
        NN_ERROR(stderr, "[lr_schedule]: the schedule's keys are out of range\n");
        return FALSE;
    }
    /* [clip]: the global-norm reduction and the factor in front of every update launch, the epoch
     * record filed by the last launch of every epoch; allocated only when clipping */
    const bool clip = o->clip > 0.0;
    if (!hpnn_clip_valid(o->clip)) {
        NN_ERROR(stderr, "[clip]: needs a finite value >= 0 (0 = off)\n");
        return FALSE;
    }
    if (clip && cg) {
        NN_ERROR(stderr, "[clip] is not supported by [train] CG (the line search chooses its own step); it applies "
                         "to BP, BPM and ADAM\n");
        return FALSE;
    }
    if (clip && !net.set_clip(o->clip, o->lr)) return FALSE;
    if (!net.init(k, B, o->type, mom || adam, s, B % 32 == 0)) return FALSE;
    NN_OUT(stdout, "batched GPU training: %s, %d samples per step\n", Net::name(), B);
    if (mom && o->resume && !net.upload_momentum(k)) return FALSE;
    if (adam) {
        if (o->resume && k->dv && !net.upload_moments(k)) return FALSE;
        NN_OUT(stdout, "batched GPU training: Adam, beta1 %g beta2 %g epsilon %g decay %g\n", o->beta1, o->beta2,
               o->eps, o->decay);
    }
    /* one rate ([lr_schedule]) and one clip record ([clip]) per epoch of the call */
    DevHistory<double> lrh;
    DevHistory<hpnn_clip_record> clh;
    if (sched && !lrh.init(o->epochs)) return FALSE;
    if (clip && !clh.init(o->epochs)) return FALSE;
    const int n_batches = (int)((n + B - 1) / B);
    int rows_p = (n_batches - 1) * B + net.Bp; /* last batch reads Bp rows */
    ResidentSet<TT> tr;
    if (!tr.upload(net, X, T, n, n_in, n_out, &rows_p, o->type, s)) return FALSE;
    XSet &xs = tr.xs;
    TT *const Td = tr.T.get();
    /* [shuffle] epoch: xs / Td are a staging set; every epoch starts with the permutation of
     * (n, seed, epochs completed) and the gathers of the canonical row-major copies into it,
     * all on the compute stream (so inside the captured epoch).  One batch per epoch: the
     * order only changes the summation order, nothing is reshuffled. */
    const bool shuffle = o->shuffle && n_batches > 1 && !cg;
    if (o->shuffle && cg) NN_OUT(stdout, "batched GPU training: CG sums over the whole set, no reshuffle\n");
    else if (o->shuffle && !shuffle) NN_OUT(stdout, "batched GPU training: one batch per epoch, no reshuffle\n");
    ResidentSet<TT> cn;
    DevBuf<int> perm;
    DevBuf<unsigned int> shw; /* [0] the epoch word, [1] the permutation kernel's error word */
    const bool dense = Net::dense_always || !xs.lab;
    if (shuffle) {
        NN_OUT(stdout, "batched GPU training: samples reshuffled every epoch\n");
        const unsigned int w0[2] = {o->epoch0, 0u};
        if (!net.upload_canon(X, (int)n, n_in, xs, &cn.xs)) return FALSE;
        HIPCHK(perm.alloc(n));
        HIPCHK(shw.alloc(2));
        HIPCHK(hipMemcpy(shw.get(), w0, sizeof w0, hipMemcpyHostToDevice));
        if (xs.lab) {
            HIPCHK(hpnn_dev_malloc(&cn.xs.lab, (size_t)n * sizeof(int)));
            HIPCHK(hipMemcpy(cn.xs.lab, xs.lab, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice));
        }
        if (dense) {
            HIPCHK(cn.T.alloc((size_t)n * n_out));
            HIPCHK(hipMemcpy(cn.T.get(), Td, (size_t)n * n_out * sizeof(TT), hipMemcpyDeviceToDevice));
        }
    }
    auto reshuffle = [&]() -> bool {
        unsigned int *w = shw.get();
        if (hpnn_epoch_perm_dev(perm.get(), (int)n, o->seed, w, w + 1, s) || hpnn_epoch_advance(w, s)) return false;
        if (!net.gather(cn.xs, xs, perm.get(), (int)n, rows_p)) return false;
        if (xs.lab && hpnn_gather_rows(xs.lab, cn.xs.lab, perm.get(), (int)n, rows_p, 4, s)) return false;
        return !dense ||
               hpnn_gather_rows(Td, cn.T.get(), perm.get(), (int)n, rows_p, (long)n_out * sizeof(TT), s) == 0;
    };
    /* [validate] N: the held-out set, uploaded once; a pass = the evaluation launches into the
     * validation stat slots plus the one-workgroup commit that files them as the next record
     * of a device history -- all on the compute stream, so inside the captured replay; the host
     * reads the history once after the last replay (per record with per-epoch metrics) */
    const bool validate = o->validate && o->Xv && o->Tv && o->nv;
    const int nval = validate ? (int)o->nv : 0;
    ResidentSet<TT> va;
    DevHistory<hpnn_val_record> vh;
    std::vector<UINT> vsched;
    int vrows_p = 0; /* the rows the held-out set is padded to */
    if (validate) {
        vsched.resize(hpnn_validation_schedule(o->epoch0, o->epochs, o->validate, nullptr));
        hpnn_validation_schedule(o->epoch0, o->epochs, o->validate, vsched.data());
        if (!va.upload(net, o->Xv, o->Tv, o->nv, n_in, n_out, &vrows_p, o->type, s, true)) return FALSE;
        if (!vh.init(vsched.size(), 1)) return FALSE;
        NN_OUT(stdout, "batched GPU training: %d held-out samples validated every %u epochs\n", nval, o->validate);
    }
    /* [keep_best]: behind the commit a one-thread launch judges the record just filed against
     * the best so far and sets a device flag, and one more launch copies the masters (and the
     * momentum) into the snapshot when the flag is set -- both part of the captured replay, so
     * the best of the several passes of one replay is kept while its weights still exist.
     * [patience]: the same launch sets a stop word; the host reads it with the health words of
     * the replay (so one replay later) and launches no further replay: at most the rest of the
     * stopping pass's replay plus one more replay run past it, changing nothing that is returned */
    const bool keep = validate && o->keep_best != 0;
    BestSnap best;
    /* [confusion]: the evaluation also writes every row's guess, a tally launch behind every chunk
     * adds guess and target class into the pass's matrix, and in front of the commit one launch
     * files the per-class record at the validation cursor, keeps the matrix as "last" and zeroes
     * it; under [keep_best] last -> best is one more segment of the snapshot */
    const bool confusion = validate && o->confusion != 0;
    ClassTally tally;
    if (confusion && !tally.init(n_out, vsched.size(), (size_t)vrows_p, keep, s)) return FALSE;
    const hpnn_snap_seg tally_seg = confusion && keep ? tally.seg() : hpnn_snap_seg{};
    if (keep) {
        if (!best.init(net.segs, s, confusion ? &tally_seg : nullptr)) return FALSE;
        NN_OUT(stdout, "batched GPU training: the best validation pass (%s) is kept\n",
               o->keep_best == NN_KEEP_ACC ? "acc" : "loss");
    }
    if (confusion) NN_OUT(stdout, "batched GPU training: per-class metrics of every validation pass\n");
    const int t_kind = sizeof(TT) == 8 ? HPNN_CONFUSION_F64 : HPNN_CONFUSION_F32;
    auto tally_chunk = [&](long row, int rows) -> bool {
        return !confusion || tally.add(row, rows, va.xs.lab, va.T.get(), n_out, t_kind);
    };
    auto validation = [&]() -> bool {
        if (net.evaluate(va.xs, va.T.get(), n_out, nval, confusion ? tally.guess.get() : nullptr, tally_chunk) &&
            (!confusion || tally.commit(vh.cursor())) &&
            hpnn_validate_commit(net.vacc(), vh.hist(), vh.cursor(), vh.cap(), s) == 0 &&
            /* plateau sees the pass before the snapshot: the best state holds this pass */
            (!sched || hpnn_lr_plateau_dev(vh.hist(), vh.cursor(), net.lr_dev(), s) == 0) &&
            (!keep || (hpnn_best_commit(vh.hist(), vh.cursor(), best.state.get(), (int)o->keep_best, o->patience, s) ==
                           0 &&
                       hpnn_snapshot_if(best.table.get(), (int)best.segs.size(), best.take(), s) == 0)))
            return true;
        NN_ERROR(stderr, "batched GPU training: the validation pass could not be launched\n");
        return false;
    };
    /* [train] CG: one epoch = one conjugate-gradient iteration over the whole set (the gradient
     * in chunks of B rows, then the fixed-work line search: kernels_cg.hip); its state, like the
     * best of [keep_best], lives for this call only */
    if constexpr (Net::has_cg) {
        if (cg) {
            if (!net.init_cg(o->lr, n, o->epochs)) return FALSE;
            NN_OUT(stdout, "batched GPU training: conjugate gradient, one iteration per epoch\n");
        }
    }
    auto epoch = [&]() -> bool {
        if constexpr (Net::has_cg) {
            if (cg) return net.iterate_cg(xs, Td, n_out, (int)n);
        }
        /* the first launch of every epoch: the rate of this epoch into the device state */
        if (sched && hpnn_lr_advance_dev(net.lr_dev(), net.adam_dev(), lrh.hist(), lrh.cursor(), lrh.cap(), s)) {
            NN_ERROR(stderr, "batched GPU training: the schedule advance could not be launched\n");
            return false;
        }
        if (shuffle && !reshuffle()) {
            NN_ERROR(stderr, "batched GPU training: the epoch reshuffle could not be launched\n");
            return false;
        }
        for (int b = 0; b < n_batches; b++) {
            int start, nv, total;
            hpnn_dp_shard(b, B, (int)n, 0, B, &start, &nv, &total);
            if (!net.step(xs, start, Td + (size_t)start * n_out, n_out, nv, o->lr, o->alpha, mom)) return false;
        }
        /* the last launch of every epoch: its clip record into the device history */
        if (clip && !net.clip_commit(clh.hist(), clh.cursor(), clh.cap())) {
            NN_ERROR(stderr, "batched GPU training: the clip commit could not be launched\n");
            return false;
        }
        return true;
    };
    const bool metrics = hpnn_metrics_active() != 0;
    const int E = (int)o->epochs;
    /* epoch e of this call (0-based) is followed by a validation pass; with per-epoch metrics
     * the pass runs eagerly behind the epoch's replay (that loop synchronises every epoch anyway) */
    auto val_due = [&](int e) { return validate && ((o->epoch0 + e + 1) % o->validate == 0 || e + 1 == E); };
    /* ne epochs from epoch e0 of the call, back to back; the statistics are zeroed before the
     * last (the only one read) */
    auto epochs = [&](int ne, int e0) -> bool {
        for (int i = 0; i < ne; i++) {
            if ((i + 1 == ne && hipMemsetAsync(net.acc, 0, Net::ACC_BYTES, s) != hipSuccess) || !epoch()) return false;
            if (!metrics && val_due(e0 + i) && !validation()) return false;
        }
        return true;
    };
    /* one graph replays epg epochs (about 32 steps: the host launches once per replay); with
     * per-epoch metrics every epoch is its own replay followed by a statistics read.  With
     * [validate] N the replay is a whole number of validation periods where that fits a graph,
     * so every replay has the same pattern of passes; a graph is keyed by its epochs and the
     * offsets of its passes (the last replay, shorter or with the closing pass, is another key) */
    /* a CG iteration (a gradient pass and seven forward passes) launches about as much as three
     * epochs of steps */
    int epg = metrics ? 1 : std::max(1, std::min(E, 32 / (std::max(1, n_batches) * (cg ? 3 : 1))));
    if (validate && !metrics && (long)o->validate * n_batches <= 4096)
        epg = std::min(E, (int)((epg + o->validate - 1) / o->validate * o->validate));
    auto gkey = [&](int ne, int e0) {
        std::vector<int> key{ne};
        for (int i = 0; i < ne && !metrics; i++)
            if (val_due(e0 + i)) key.push_back(i);
        return key;
    };
    hpnn_preload_code_objects();
    std::map<std::vector<int>, GraphExec> graphs;
    if (graphs_enabled() && n_batches <= 4096)
        for (int e0 = 0; e0 < E; e0 += epg) {
            const int ne = std::min(epg, E - e0);
            const std::vector<int> key = gkey(ne, e0);
            if (graphs.count(key)) continue;
            if (!capture_epoch(s, [&]() { return epochs(ne, e0); }, &graphs[key]))
                NN_DBG(stdout, "batched GPU training: epochs not capturable, eager launches\n");
        }
    /* setup (data upload and layout conversions) is finished before the clock starts */
    HIPCHK(hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    double ep_loss = 0.0;
    unsigned int ep_hits = 0;
    /* the health of every replay (HealthRing), plus a final check after the last replay; word
     * [3] is the permutation kernel's error word, word [4] the stop word of [patience] */
    HealthRing ring;
    BOOL ok = ring.ok();
    int pend = -1, slot = 0;
    const bool patient = keep && o->patience > 0;
    bool stopped = false; /* the host has seen the stop word: no further replay */
    unsigned int hstop = 0;
    auto judge = [&](int sl) -> bool {
        const unsigned int *d = ring.judge(sl);
        if (!d || !net.health_ok(d)) return false;
        if (d[3]) {
            NN_ERROR(stderr,
                     "batched GPU training: the epoch permutation did not terminate within its bound; stopping\n");
            return false;
        }
        if (d[4]) stopped = true;
        return true;
    };
    RunRecords rec;
    std::vector<hpnn_val_record> &vrec = rec.vrec;
    size_t &vdone = rec.vdone;
    vrec.resize(vsched.size());
    int e = 0;
    while (e < E && ok && !stopped) {
        const int ne = std::min(epg, E - e);
        auto g = graphs.find(gkey(ne, e));
        ok = (g != graphs.end() && g->second) ? hipGraphLaunch(g->second.get(), s) == hipSuccess : epochs(ne, e);
        e += ne;
        if (ok)
            ok = ring.post(slot, s, net, [&](unsigned int *d) {
                return (!shuffle || hipMemcpyAsync(d + 3, shw.get() + 1, 4, hipMemcpyDeviceToHost, s) == hipSuccess) &&
                       (!patient || hipMemcpyAsync(d + 4, best.stop(), 4, hipMemcpyDeviceToHost, s) == hipSuccess);
            });
        if (ok && pend >= 0) ok = judge(pend);
        pend = ok ? slot : -1;
        slot ^= 1;
        if (ok && (metrics || e == E)) {
            ok = judge(pend); /* statistics read = a synchronisation anyway: judge this replay now */
            pend = -1;
            if (ok) ok = net.read_stats(&ep_loss, &ep_hits);
        }
        if (ok && metrics)
            hpnn_metrics_epoch("gpu", o->epoch0 + e, ep_loss / (double)n, ep_hits, n,
                               std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                               (UINT64)n * e);
        if (ok && metrics && val_due(e - 1) && vdone < vrec.size()) {
            ok = validation() && hipMemcpyAsync(&vrec[vdone], vh.hist() + vdone, sizeof(hpnn_val_record),
                                                hipMemcpyDeviceToHost, s) == hipSuccess &&
                 (!patient || hipMemcpyAsync(&hstop, best.stop(), 4, hipMemcpyDeviceToHost, s) == hipSuccess) &&
                 hipStreamSynchronize(s) == hipSuccess;
            if (ok)
                hpnn_metrics_validation("gpu", o->epoch0 + e, vrec[vdone].loss_sum / (double)nval, vrec[vdone].hits,
                                        (UINT)nval);
            if (ok && confusion) {
                std::vector<unsigned int> pc((size_t)3 * n_out);
                ok = hipMemcpy(pc.data(), tally.hist.get() + vdone * pc.size(), pc.size() * sizeof(unsigned int),
                               hipMemcpyDeviceToHost) == hipSuccess;
                if (ok) hpnn_metrics_classes("gpu", o->epoch0 + e, pc.data(), (UINT)n_out);
            }
            vdone++;
            if (ok && hstop) stopped = true;
        }
    }
    if (ok && pend >= 0) ok = judge(pend);
    /* stopped before the last epoch: the statistics of the last epoch that ran */
    if (ok && !metrics && e < E) ok = net.read_stats(&ep_loss, &ep_hits);
    auto t1 = std::chrono::steady_clock::now();
    const RunDev<Net> dev{net, s, o, vsched, keep ? &best : nullptr, vh, lrh, clh, confusion ? &tally : nullptr};
    if (ok) ok = collect(dev, e, metrics, &rec);
    const hpnn_best_state &hb = rec.hb;
    graphs.clear();
    if (ok) ok = net.download_from(k, hb.valid ? best.dst.data() : nullptr);
    if (ok && st) {
        if (cg && e > 0) ep_loss = rec.cg_f0 * (double)n;
        fill_stats(st, std::chrono::duration<double>(t1 - t0).count(), n, (UINT)e, ep_loss, ep_hits);
        st->epochs_run = (UINT)e;
        st->best_epoch = hb.valid ? vsched[hb.index] : 0;
        st->best_index = hb.valid ? hb.index : 0;
        st->stop_epoch = hb.stop && !vrec.empty() ? vsched[vrec.size() - 1] : 0;
        st->lrs = rec.lrs;
        std::vector<hpnn_validation_record> val(vrec.size());
        for (size_t i = 0; i < val.size(); i++)
            val[i] = {vsched[i], vrec[i].loss_sum / (double)nval, vrec[i].hits, (UINT)nval};
        ok = export_records(rec.crec, &st->cg, &st->n_cg);
        ok = export_records(rec.lrec, &st->lr_hist, &st->n_lr) && ok;
        ok = export_records(rec.clrec, &st->clip_hist, &st->n_clip) && ok;
        ok = export_records(val, &st->val, &st->n_val) && ok;
        if (confusion) {
            UINT words = 0, cells = 0;
            st->n_classes = (UINT)n_out;
            ok = export_records(rec.pcrec, &st->class_hist, &words) && ok;
            st->n_class_hist = (UINT)val.size(); /* records of 3 n_out words */
            ok = export_records(rec.mlast, &st->confusion_last, &cells) && ok;
            ok = export_records(rec.mbest, &st->confusion_best, &cells) && ok;
            st->confusion_launches = tally.launches;
        }
    }
    /* device FP64 copy of the online engine (if any) is now stale */
    hpnn_gpu_mark_host_dirty(k);
    return ok;
}

}  // namespace

BOOL hpnn::eng::train_single(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                             hpnn_batched_stats *st) {
    return with_net(o->dtype, [&](auto t) { return train_single_t<typename decltype(t)::type>(k, X, T, n, o, st); });
}
