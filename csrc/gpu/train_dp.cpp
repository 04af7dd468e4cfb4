/*
 * libhpnn batched GPU engine.  Data-parallel batched training driven by ONE process over G
 * replicas (the reference's single-process multi-GPU design, libhpnn.c:201-305, hub copies replaced by an
 * RCCL all-reduce over xGMI): every global minibatch of B samples is split into G shards
 * of ceil(B/G); each replica computes the gradient sum of its shard into a flat FP32
 * buffer; one grouped ncclAllReduce sums them; every replica applies the identical update
 * with scale 1/(samples of the minibatch), so the weights stay replicated and the result
 * equals the single-GPU step up to summation order.
 * loopback: G virtual replicas on ONE device (CI without a multi-GPU node): the buffers
 * live in one allocation and the all-reduce is a deterministic slab sum.
 */
#include <chrono>
#include <memory>
#include <thread>

#include "batched_net.h"

using namespace hpnn::eng;

namespace {

template <class Net>
BOOL train_dp_t(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                hpnn_batched_stats *st, int G, bool loopback) {
    typedef typename Net::target_t TT;
    typedef typename Net::grad_t GT;
    if (k->n_hiddens + 1 > 16 || G < 1) return FALSE;
    if (single_device_only(o, "data-parallel")) return FALSE;
    if (!loopback && !hpnn_comm_available()) return FALSE;
    hpnn_gpu_sync_host(k);
    const int B = (int)(o->batch ? o->batch : 256);
    const int Bg = (B + G - 1) / G;
    const bool mom = o->train == NN_TRAIN_BPM;
    const int n_out = (int)k->n_outputs;
    std::vector<int> dev(G);
    std::vector<hipStream_t> str(G);
    std::vector<std::unique_ptr<Net>> nets(G);
    DevBuf<GT> lb_flat; /* loopback: [G][count] in one allocation */
    /* one resident set per device: the loopback replicas all read set 0 */
    std::vector<ResidentSet<TT>> sets(loopback ? 1 : G);
    auto set_of = [&](int g) -> const ResidentSet<TT> & { return sets[loopback ? 0 : g]; };
    std::vector<hpnn_comm *> comms(G, nullptr);
    std::vector<GraphExec> gexec(G);
    BOOL ok = TRUE;
    const int n_batches = (int)((n + B - 1) / B);
    /* every replica's state goes with its device current */
    auto cleanup = [&]() {
        for (int g = 0; g < G; g++) {
            hipSetDevice(dev[g]);
            gexec[g].reset();
            if (!loopback || g == 0) sets[g].release();
            nets[g].reset();
            if (comms[g]) hpnn_comm_destroy(comms[g]);
        }
        lb_flat.reset();
        hipSetDevice(hpnn_rt_device(0));
    };
    for (int g = 0; g < G; g++) {
        dev[g] = loopback ? hpnn_rt_device(0) : hpnn_rt_device((UINT)g);
        str[g] = loopback ? hpnn_rt_stream(0, 0) : hpnn_rt_stream((UINT)g, 0);
        if (!str[g]) return FALSE;
    }
    /* replicas + data (rows padded so every shard of the last minibatch reads Bp rows) */
    int rows_p = n_batches * B + Bg + 128;
    for (int g = 0; g < G && ok; g++) {
        ok = hipSetDevice(dev[g]) == hipSuccess;
        if (!ok) break;
        nets[g].reset(new Net());
        /* fragment-major inputs need every shard to start at a multiple of 32 rows */
        ok = nets[g]->init(k, Bg, o->type, mom, str[g], B % 32 == 0 && Bg % 32 == 0);
        if (ok && mom && o->resume) ok = nets[g]->upload_momentum(k);
        if (!ok) break;
        if (loopback) {
            if (g == 0) {
                size_t tot = 0;
                if (!nets[0]->alloc_flat(nullptr)) ok = FALSE; /* sizes only; re-pointed below */
                if (ok) tot = nets[0]->flat_count();
                if (ok && lb_flat.alloc(tot * G) != hipSuccess) ok = FALSE;
            }
            if (ok) {
                const size_t tot = nets[0]->flat_count();
                if (g == 0 && nets[0]->own_flat) {
                    hpnn_dev_free(nets[0]->gflat);
                    nets[0]->own_flat = false;
                }
                ok = nets[g]->alloc_flat(lb_flat.get() + tot * g);
            }
        } else {
            ok = nets[g]->alloc_flat();
        }
        if (!ok) break;
        if (!loopback || g == 0)
            ok = sets[g].upload(*nets[g], X, T, n, (int)k->n_inputs, n_out, &rows_p, o->type, str[g]);
    }
    if (ok && !loopback) {
        if (hpnn_comm_init_all(comms.data(), G, dev.data()) != 0) ok = FALSE;
    }
    if (!ok) {
        cleanup();
        return FALSE;
    }
    const size_t count = nets[0]->flat_count();
    NN_OUT(stdout, "data-parallel batched training: %d replicas (%s, %s), %d samples per replica per step\n", G,
           loopback ? "loopback on one GPU" : "RCCL all-reduce", Net::name(), Bg);
    for (int g = 0; g < G; g++) {
        hipSetDevice(dev[g]);
        hpnn_preload_code_objects();
    }
    hipSetDevice(dev[0]);
    auto t0 = std::chrono::steady_clock::now();
    double ep_loss = 0.0;
    unsigned int ep_hits = 0;
    /* RCCL replicas: one HIP graph per replica epoch (HPNN_GRAPH=0: eager) */
    const bool dp_graphs = !loopback && graphs_enabled() && n_batches <= 4096;
    std::vector<int> gtried(G, 0);
    for (UINT e = 0; e < o->epochs && ok; e++) {
        for (int g = 0; g < G; g++) {
            hipSetDevice(dev[g]);
            hipMemsetAsync(nets[g]->acc, 0, Net::ACC_BYTES, str[g]);
        }
        if (loopback) {
            for (int b = 0; b < n_batches && ok; b++) {
                int start, nv, total = 0;
                for (int g = 0; g < G && ok; g++) {
                    hpnn_dp_shard(b, B, (int)n, g, Bg, &start, &nv, &total);
                    ok = nets[g]->grads(set_of(g).xs, start, set_of(g).T.get() + (size_t)start * n_out, n_out, nv);
                }
                if (!ok) break;
                /* virtual replicas share one stream: sum the G buffers into replica 0's */
                ok = Net::reduce_sum(lb_flat.get(), G, count, str[0]) == 0;
                const double scale = 1.0 / (double)(total > 0 ? total : 1);
                for (int g = 0; g < G && ok; g++) ok = nets[g]->update_flat(lb_flat.get(), o->lr, o->alpha, scale, mom);
            }
        } else {
            /* one host thread per GPU for the whole epoch (no serial hipSetDevice + launch
             * loop over the replicas); the step is rccl_bucket_step */
            std::vector<int> tok(G, 1);
            std::vector<std::thread> th;
            for (int g = 0; g < G; g++)
                th.emplace_back([&, g]() {
                    if (hipSetDevice(dev[g]) != hipSuccess) {
                        tok[g] = 0;
                        return;
                    }
                    Net &net = *nets[g];
                    /* the replica's epoch (HIP graph: captured on the first epoch, the RCCL
                     * collectives and the side-stream fork / join included; replayed after) */
                    auto epoch_body = [&]() -> bool {
                        for (int b = 0; b < n_batches; b++) {
                            int start, nv, total;
                            hpnn_dp_shard(b, B, (int)n, g, Bg, &start, &nv, &total);
                            const TT *tb = set_of(g).T.get() + (size_t)start * n_out;
                            if (!rccl_bucket_step(net, comms[g], str[g], set_of(g).xs, start, tb, n_out, nv, total,
                                                  o->lr, o->alpha, mom, tok[g] != 0) &&
                                tok[g]) {
                                NN_ERROR(stderr, "data-parallel step failed on replica %d\n", g);
                                tok[g] = 0;
                            }
                        }
                        return tok[g] != 0;
                    };
                    if (dp_graphs && !gtried[g]) {
                        gtried[g] = 1;
                        if (!capture_epoch(str[g], epoch_body, &gexec[g]))
                            NN_DBG(stdout, "data-parallel replica %d: epoch not capturable, eager launches\n", g);
                    }
                    if (gexec[g]) {
                        if (hipGraphLaunch(gexec[g].get(), str[g]) != hipSuccess) tok[g] = 0;
                    } else {
                        epoch_body();
                    }
                    if (hipStreamSynchronize(str[g]) != hipSuccess) tok[g] = 0;
                });
            for (auto &t : th) t.join();
            for (int g = 0; g < G; g++) ok = ok && tok[g];
        }
        if (!ok) break;
        ep_loss = 0.0;
        ep_hits = 0;
        for (int g = 0; g < G && ok; g++) {
            hipSetDevice(dev[g]);
            double l = 0.0;
            unsigned int h = 0;
            ok = nets[g]->read_stats(&l, &h) && nets[g]->healthy();
            ep_loss += l;
            ep_hits += h;
        }
        if (!loopback && ok) {
            /* surface asynchronous communicator failures (a peer died, link error) */
            for (int g = 0; g < G; g++)
                if (hpnn_comm_check(comms[g]) != 0) ok = FALSE;
        }
        if (ok && hpnn_metrics_active())
            hpnn_metrics_epoch(loopback ? "gpu-dp-loopback" : "gpu-dp", o->epoch0 + e + 1, ep_loss / (double)n,
                               ep_hits, n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                               (UINT64)n * (e + 1));
    }
    auto t1 = std::chrono::steady_clock::now();
    if (ok) {
        hipSetDevice(dev[0]);
        ok = nets[0]->download(k);
    }
    if (ok && st) fill_stats(st, std::chrono::duration<double>(t1 - t0).count(), n, o->epochs, ep_loss, ep_hits);
    cleanup();
    if (ok) hpnn_gpu_mark_host_dirty(k);
    return ok;
}

}  // namespace

BOOL hpnn::eng::train_dp(kernel_ann *k, const DOUBLE *X, const DOUBLE *T, UINT n, const hpnn_batched_opts *o,
                         hpnn_batched_stats *st, int G, bool loopback) {
    return with_net(o->dtype,
                    [&](auto t) { return train_dp_t<typename decltype(t)::type>(k, X, T, n, o, st, G, loopback); });
}
