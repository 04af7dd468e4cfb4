/*
 * libhpnn batched GPU engine -- data parallelism with ONE process per GPU (any launcher exporting RANK / WORLD_SIZE /
 * LOCAL_RANK; the reference ran `mpirun -np N train_nn` and replicated the same sample on
 * every rank).  Rank r trains rows [b*B + r*ceil(B/W), ...) of every global
 * minibatch b; the FP32 gradients are summed with the one-shot xGMI all-reduce (all
 * ranks on one node, gradients <= 4 MiB) or RCCL, the bootstrap exchange (IPC handles /
 * unique id / epoch statistics) goes through include/libhpnn/bootstrap.h; every rank
 * applies the same update, so the weights stay identical (rank 0 writes the files).
 */
#include <libhpnn/bootstrap.h>
#include <chrono>

#include "batched_net.h"

using namespace hpnn::eng;

namespace {

struct XarFree {
    void operator()(hpnn_xar *x) const { hpnn_xar_destroy(x); }
};
struct CommFree {
    void operator()(hpnn_comm *c) const { hpnn_comm_destroy(c); }
};

template <class Net>
BOOL train_dp_mp_t(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                 hpnn_batched_stats *st) {
    typedef typename Net::target_t TT;
    const int W = hpnn_boot_world(), R = hpnn_boot_rank();
    if (k->n_hiddens + 1 > 16 || W < 1 || W > 64) return FALSE;
    if (single_device_only(o, "data-parallel")) return FALSE;
    hpnn_gpu_sync_host(k);
    const int dev = hpnn_rt_device(0);
    HIPCHK(hipSetDevice(dev));
    hipStream_t s = hpnn_rt_stream(0, 0);
    const int B = (int)(o->batch ? o->batch : 256);
    const int Bg = (B + W - 1) / W;
    const bool mom = o->train == NN_TRAIN_BPM;
    const int n_out = (int)k->n_outputs;
    /* HPNN_GRAD_COMM=bf16rs: BF16 reduce-scatter + sharded step + BF16 all-gather (RCCL,
     * per-layer plan); fp32: the FP32 all-reduce; auto (default): bf16rs for the BF16 engine
     * when the net takes the per-layer plan and its FP32 gradients exceed 4 MB (bandwidth-
     * bound exchange: half the bytes, each rank steps 1 / world of the rows), else fp32.
     * Every rank reads the same environment and net, so all decide alike. */
    const char *gce = getenv("HPNN_GRAD_COMM");
    bool bf16rs = gce && !strcmp(gce, "bf16rs");
    if (!gce || !strcmp(gce, "auto")) {
        double gbytes = 0.0;
        const int nl = (int)k->n_hiddens + 1;
        std::vector<int> sizes(nl + 1);
        sizes[0] = (int)k->n_inputs;
        for (int l = 0; l < nl; l++) {
            sizes[l + 1] = (int)layer_of(k, l)->n_neurons;
            gbytes += 4.0 * sizes[l] * sizes[l + 1];
        }
        hpnn::BPlan probe; /* host-only configuration: which step structure the net gets */
        const bool per_layer =
            probe.configure(sizes.data(), nl, plan_type(o->type), Bg, mom, -1, nullptr, 512, false) == 0 && probe.mode == 0;
        bf16rs = W > 1 && !strcmp(Net::name(), "bf16") && per_layer && gbytes > (double)(4 << 20);
    }
    /* the exchange's owners come before the net, so a failed setup releases them after it
     * (the net's DpExchange never outlives its communicator) */
    std::unique_ptr<hpnn_xar, XarFree> xar, xark;
    std::unique_ptr<hpnn_comm, CommFree> comm;
    Net net;
    if (!net.init(k, Bg, o->type, mom, s, B % 32 == 0 && Bg % 32 == 0, bf16rs ? 0 : -1) || !net.alloc_flat())
        return FALSE;
    if (mom && o->resume && !net.upload_momentum(k)) return FALSE;
    const size_t count = net.flat_count();
    /* gradient exchange: one-shot xGMI all-reduce when every rank is on this node and the
     * gradients are small, else RCCL; every rank takes the same decision */
    const char *xe = getenv("HPNN_XAR");
    const char *lws = getenv("LOCAL_WORLD_SIZE");
    /* the xGMI all-reduce sums FP32; FP64 gradients go through RCCL */
    bool use_xar = Net::comm_dt == HPNN_DT_F32 && !(xe && xe[0] == '0') && lws && atoi(lws) == W &&
                   W <= HPNN_XAR_MAX_RANKS && count * 4 <= ((size_t)4 << 20) && !bf16rs;
    /* collective: create, exchange the IPC handles, open, self-test on the real links; every
     * rank agrees, else all get nullptr (-1: bootstrap failure) */
    auto open_xar = [&](size_t bytes, std::unique_ptr<hpnn_xar, XarFree> *out) -> int {
        out->reset();
        std::unique_ptr<hpnn_xar, XarFree> x(hpnn_xar_create(R, W, bytes));
        std::vector<char> h(HPNN_XAR_HANDLE_BYTES, 0), all((size_t)W * HPNN_XAR_HANDLE_BYTES);
        int ok = x && hpnn_xar_handles(x.get(), h.data()) == 0;
        if (hpnn_boot_allgather(h.data(), h.size(), all.data()) != 0) return -1;
        if (ok) ok = hpnn_xar_open(x.get(), all.data()) == 0;
        std::vector<int> oks(W);
        if (hpnn_boot_allgather(&ok, sizeof ok, oks.data()) != 0) return -1;
        bool all_ok = true;
        for (int v : oks) all_ok = all_ok && v;
        if (all_ok) { /* known sums over the real links before any gradient goes through */
            const int rc = hpnn_xar_self_test(x.get(), s);
            ok = rc == 0;
            if (!ok) NN_WARN(stderr, "xGMI all-reduce self-test failed (%d) on rank %d\n", rc, R);
            if (hpnn_boot_allgather(&ok, sizeof ok, oks.data()) != 0) return -1;
            for (int v : oks) all_ok = all_ok && v;
        }
        if (all_ok) *out = std::move(x);
        return 0;
    };
    if (use_xar) {
        if (open_xar(count * 4, &xar)) return FALSE;
        use_xar = xar != nullptr;
        /* fused modes: a second communicator whose protocol runs inside the G0 launch
         * (HPNN_XAR_G0=0: the all-reduce launch instead) */
        const char *xg = getenv("HPNN_XAR_G0");
        if (use_xar && !(xg && xg[0] == '0') && open_xar(count * 4, &xark)) return FALSE;
    }
    /* collective: the RCCL communicator (rank 0's unique id through the bootstrap) */
    auto open_rccl = [&]() -> bool {
        unsigned char id[HPNN_COMM_ID_BYTES] = {0};
        std::vector<unsigned char> all((size_t)W * HPNN_COMM_ID_BYTES);
        if (R == 0 && hpnn_comm_unique_id(id) != 0) return false;
        if (hpnn_boot_allgather(id, sizeof id, all.data()) != 0) return false;
        comm.reset(hpnn_comm_init_rank(all.data(), W, R, dev)); /* rank 0's id */
        if (!comm) return false;
        /* BF16 batched engine: the library's overlapped data-parallel step (dp_exchange.h);
         * FP32 / FP64 engines: the bucket loop below */
        if (!net.attach_dpx(comm.get(), bf16rs ? hpnn::DpExchange::BF16RS : hpnn::DpExchange::FP32) && bf16rs)
            NN_WARN(stderr, "bf16rs exchange unavailable for this net: FP32 all-reduce\n");
        return true;
    };
    if (!use_xar && !open_rccl()) return FALSE;
    NN_OUT(stdout, "data-parallel batched training: %d processes (%s, %s), %d samples per rank per step\n", W,
           use_xar ? "xGMI all-reduce" : "RCCL all-reduce", Net::name(), Bg);
    /* the gradient exchange chosen (HPNN_GRAD_COMM; auto picks bf16rs for large per-layer nets) */
    if (R == 0 && W > 1)
        NN_OUT(stdout, "data-parallel gradient exchange: %s\n",
               bf16rs ? "bf16rs (BF16 reduce-scatter, sharded FP32 step, BF16 all-gather)" : "fp32 (all-reduce)");
    const int n_batches = (int)((n + B - 1) / B);
    int rows_p = n_batches * B + Bg + 128;
    ResidentSet<TT> rs;
    BOOL ok = rs.upload(net, X, T, n, (int)k->n_inputs, n_out, &rows_p, o->type, s);
    const XSet &Xd = rs.xs;
    const TT *const Td = rs.T.get();
    hpnn_preload_code_objects();
    /* per-replay health (HealthRing): the exchange's error words are [3..4] of a slot */
    HealthRing ring;
    if (!ring.ok()) ok = FALSE;
    int pend = -1; /* slot whose readback is in flight */
    auto enqueue_check = [&](int slot) -> bool {
        return ring.post(slot, s, net, [&](unsigned int *d) {
            return (!use_xar || hpnn_xar_status_enqueue(xar.get(), d + 3, s) == 0) &&
                   (!xark || hpnn_xar_status_enqueue(xark.get(), d + 4, s) == 0);
        });
    };
    auto finish_check = [&](int slot) -> bool {
        const unsigned int *d = ring.judge(slot);
        if (!d || !net.health_ok(d)) return false;
        return use_xar ? d[3] == 0 && d[4] == 0 : hpnn_comm_check(comm.get()) == 0;
    };
    /* preflight: the plan and the exchange start clean (and the first reads of their words, a
     * few ms while the runtime maps them, stay out of the training time) */
    if (ok) ok = enqueue_check(0) && finish_check(0);
    {
        /* ... and every other readback of the agreement points once (statistics, digest):
         * their first calls set up host staging and copy paths (ms) */
        double l0 = 0.0;
        unsigned int h0 = 0;
        unsigned long long d0 = 0;
        if (ok) ok = net.read_stats(&l0, &h0) && net.digest(&d0);
    }
    /* setup (data upload and layout conversions) is finished before the clock starts */
    if (hipDeviceSynchronize() != hipSuccess) ok = FALSE;
    auto t0 = std::chrono::steady_clock::now();
    double ep_loss = 0.0;
    unsigned int ep_hits = 0;
    /* one epoch's steps: the same launches on every rank, every epoch (the minibatch order is
     * fixed), so from the second epoch on they replay as ONE HIP graph per epoch -- the
     * launches bench.py times (the first epoch runs eagerly: it settles the exchange form) */
    /* reset: zero the statistics first (only the last epoch of a replay group is ever read) */
    auto epoch_steps = [&](UINT e, bool reset = true) -> bool {
        if (reset && hipMemsetAsync(net.acc, 0, Net::ACC_BYTES, s) != hipSuccess) return false;
        for (int b = 0; b < n_batches; b++) {
            int start, nv, total;
            hpnn_dp_shard(b, B, (int)n, R, Bg, &start, &nv, &total);
            const TT *tb = Td + (size_t)start * n_out;
            if (net.has_dpx()) {
                if (!net.dp_step(Xd, start, tb, n_out, nv, total, o->lr, o->alpha)) return false;
                continue;
            }
            if (xark) {
                /* the exchange and every step inside the first-layer gradient launch */
                const int r = net.xchg_step(Xd, start, tb, n_out, nv, o->lr, o->alpha,
                                            1.0 / (double)(total > 0 ? total : 1), xark.get());
                if (r == 0) {
                    if (e == 0 && b == 0 && R == 0)
                        NN_OUT(stdout, "data-parallel step: exchange inside the first-layer gradient launch\n");
                    continue;
                }
                if (r != -1) {
                    NN_ERROR(stderr, "data-parallel fused step failed: %d\n", r);
                    return false;
                }
                /* not covered (same on every rank): the all-reduce launch from here on */
                xark.reset();
            }
            if (!use_xar) { /* RCCL: the overlapped bucket step */
                if (!rccl_bucket_step(net, comm.get(), s, Xd, start, tb, n_out, nv, total, o->lr, o->alpha, mom))
                    return false;
                continue;
            }
            /* small gradients: ONE latency-bound xGMI all-reduce of the whole buffer */
            if (!net.grads(Xd, start, tb, n_out, nv) ||
                hpnn_xar_all_reduce_f32(xar.get(), (float *)net.gflat, (float *)net.gflat, (long)count, s) != 0 ||
                !net.update_flat(net.gflat, o->lr, o->alpha, 1.0 / (double)(total > 0 ? total : 1), mom))
                return false;
        }
        return true;
    };
    /* Epoch 0 runs eagerly; then one HIP graph replays epg epochs (about 32 steps, as
     * train_single).  After every replay a rank checks its own health (one small readback);
     * the ranks agree (one host all-gather) after the first epoch, the last, every epoch under
     * metrics and every 16th replay otherwise.  Between agreements a rank that saw a failure
     * keeps launching -- the exchange needs every rank in step -- and reports it at the next
     * one.  Graph capture is setup, not training: its time is left out of the training time,
     * as train_single captures before its clock starts. */
    const bool metrics = hpnn_metrics_active() != 0;
    const UINT E = o->epochs;
    const UINT epg = metrics ? 1u : std::max(1u, std::min(E > 1 ? E - 1 : 1u, 32u / (UINT)std::max(1, n_batches)));
    GraphExec gx;
    double setup_s = 0.0;
    bool local_ok = true;
    bool recheck = false; /* digests compared again at the next agreement point (after a fallback) */
    UINT replays = 0;
    for (UINT e = 0; e < E && ok;) {
        if (e == 1 && graphs_enabled() && n_batches <= 4096 && E - 1 >= epg) {
            /* every rank captures; all replay only if all captured (a failed capture ran
             * nothing, so eager epochs stay in step) */
            const auto c0 = std::chrono::steady_clock::now();
            int cap = capture_epoch(s, [&]() {
                for (UINT i = 0; i < epg; i++)
                    if (!epoch_steps(e + i, i + 1 == epg)) return false;
                return true;
            }, &gx) ? 1 : 0;
            std::vector<int> caps(W);
            if (hpnn_boot_allgather(&cap, sizeof cap, caps.data()) != 0) ok = FALSE;
            for (int v : caps) cap = cap && v;
            if (!cap) gx.reset();
            if (ok && R == 0)
                NN_OUT(stdout, "data-parallel epochs: %s\n", gx ? "HIP graph replays" : "eager launches (capture failed)");
            setup_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
            if (!ok) break;
        }
        const UINT ne = e == 0 ? 1u : std::min(epg, E - e);
        bool lok;
        if (gx && e > 0 && ne == epg) {
            lok = hipGraphLaunch(gx.get(), s) == hipSuccess;
        } else {
            lok = true;
            for (UINT i = 0; i < ne && lok; i++) lok = epoch_steps(e + i, i + 1 == ne);
        }
        e += ne;
        if (e > 1) replays++;
        /* this replay's health words are read back behind it; the previous replay's are judged
         * now (the host waits for that replay only, with this one queued behind it) */
        const int slot = (int)(replays & 1);
        if (lok) lok = enqueue_check(slot);
        if (pend >= 0) local_ok = finish_check(pend) && local_ok;
        pend = lok ? slot : -1;
        local_ok = local_ok && lok;
        const bool first = e == 1, last = e == E;
        if (!(first || last || metrics || recheck || replays % 16 == 0)) continue;
        /* agreement point */
        if (pend >= 0) local_ok = finish_check(pend) && local_ok;
        pend = -1;
        double l = 0.0;
        unsigned int h = 0;
        if (local_ok && !net.read_stats(&l, &h)) local_ok = false;
        /* replicas must hold bitwise-identical weights: a wrong-but-timely exchange (a sum that
         * arrived in time but is not every rank's) shows here, after the first epoch and the last */
        unsigned long long dig = 0;
        const bool check_dig = first || last || recheck;
        if (local_ok && check_dig && !net.digest(&dig)) local_ok = false;
        if (local_ok && check_dig && R == W - 1 && hpnn_fault_hit("digest")) dig ^= 1; /* test hook */
        if (local_ok && check_dig && first && R == W - 1 && use_xar && hpnn_fault_hit("xdigest"))
            dig ^= 1; /* test hook: the first xGMI epoch looks wrong on one rank -> fallback */
        struct {
            double loss;
            unsigned long long digest;
            unsigned int hits, ok;
        } mine = {l, dig, h, (unsigned)local_ok};
        std::vector<decltype(mine)> every(W);
        if (hpnn_boot_allgather(&mine, sizeof mine, every.data()) != 0) ok = FALSE;
        ep_loss = 0.0;
        ep_hits = 0;
        bool same = true;
        for (int r = 0; r < W && ok; r++) {
            ep_loss += every[r].loss;
            ep_hits += every[r].hits;
            ok = ok && every[r].ok;
            same = same && every[r].digest == every[0].digest;
        }
        if (first && R == 0)
            NN_DBG(stdout, "data-parallel: epoch 1 (eager, with the weight digest) %.3f ms\n",
                   1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        if (ok && check_dig && !same && first && use_xar) {
            /* a wrong-but-timely xGMI sum: degrade instead of stopping -- every rank leaves the
             * xGMI exchange for RCCL, rank 0's weights and momentum are re-broadcast, and the
             * digests are compared again after the next epoch (a mismatch there stops the run).
             * Reference: the P2P -> CMM -> EXP fallback chain, libhpnn.c:245-302 */
            if (R == 0)
                NN_WARN(stderr, "data-parallel training: the replicas' weights differ after epoch 1 over the "
                                "xGMI exchange; falling back to RCCL from rank 0's weights\n");
            std::vector<char> mine_st, all_st;
            ok = net.get_state(mine_st);
            if (ok) {
                all_st.resize(mine_st.size() * (size_t)W);
                ok = hpnn_boot_allgather(mine_st.data(), mine_st.size(), all_st.data()) == 0 &&
                     net.set_state(all_st.data()); /* rank 0's block */
            }
            xark.reset();
            xar.reset();
            use_xar = false;
            if (ok && !open_rccl()) ok = FALSE;
            recheck = true;
            same = true;
        } else if (ok && check_dig && recheck) {
            recheck = false;
        }
        if (ok && check_dig && !same) {
            if (R == 0)
                NN_ERROR(stderr, "data-parallel training: the replicas' weights differ after epoch %u "
                                 "(exchange error); stopping\n", e);
            ok = FALSE;
        }
        if (ok && metrics)
            hpnn_metrics_epoch("gpu-dp-mp", o->epoch0 + e, ep_loss / (double)n, ep_hits, n,
                               std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() - setup_s,
                               (UINT64)n * e);
    }
    auto t1 = std::chrono::steady_clock::now();
    gx.reset();
    hipStreamSynchronize(s);
    if (ok) ok = net.gather_masters(); /* bf16rs: every rank's rows of the FP32 masters */
    if (ok) ok = net.download(k);
    if (ok && st)
        fill_stats(st, std::chrono::duration<double>(t1 - t0).count() - setup_s, n, o->epochs, ep_loss, ep_hits);
    hipStreamSynchronize(s);
    net.detach_dpx(); /* before the communicator goes */
    hpnn_boot_finish(); /* every rank is past its last all-reduce before any buffer goes */
    rs.release();
    xar.reset();
    xark.reset();
    comm.reset();
    if (ok) hpnn_gpu_mark_host_dirty(k);
    return ok;
}

}  // namespace

BOOL hpnn::eng::train_dp_mp(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                            hpnn_batched_stats *st) {
    return with_net(o->dtype, [&](auto t) { return train_dp_mp_t<typename decltype(t)::type>(k, X, T, n, o, st); });
}
