/*
 * libhpnn batched GPU engine -- inference (run_nn on the GPU): the whole test set through
 * the forward pass of the batched net of the requested precision.
 */
#include <thread>

#include "batched_net.h"

using namespace hpnn::eng;

namespace {

BOOL infer_bf16(kernel_ann *k, nn_type type, const DOUBLE *X, UINT n, DOUBLE *Y, hipStream_t s) {
    const int B = 4096;
    Batched net;
    if (!net.init(k, B, type, false, s, false, 0)) return FALSE; /* forward only: per-layer plan */
    const int n_batches = (int)((n + B - 1) / B);
    const int rows_p = (n_batches - 1) * B + net.Bp;
    const int no = net.p.Np[net.L - 1];
    XSet xs;
    DevBuf<float> O;
    if (!net.upload_x(X, (int)n, (int)k->n_inputs, rows_p, &xs)) return FALSE;
    HIPCHK(O.alloc((size_t)net.Bp * no));
    std::vector<float> h((size_t)net.Bp * no);
    BOOL ok = TRUE;
    for (int b = 0; b < n_batches && ok; b++) {
        int start, nv, total;
        hpnn_dp_shard(b, B, (int)n, 0, B, &start, &nv, &total);
        ok = net.p.predict(net.at(xs, (long)b * B).x, nv, O.get(), no, s) == 0;
        ok = ok && hipMemcpyAsync(h.data(), O.get(), h.size() * 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
        for (int r = 0; ok && r < nv; r++)
            for (UINT c = 0; c < k->n_outputs; c++) Y[((size_t)b * B + r) * k->n_outputs + c] = h[(size_t)r * no + c];
    }
    return ok;
}

/* FP64 / FP32 inference: the forward GEMMs and the output activation in the model's
 * precision, one device-to-host copy of the outputs per block of samples */
template <typename T>
BOOL infer_fp(kernel_ann *k, nn_type type, const DOUBLE *X, UINT n, DOUBLE *Y, hipStream_t s) {
    const int B = (int)(n < 16384 ? n : 16384);
    BatchedFP<T> net;
    if (!net.init(k, B, type, false, s)) return FALSE;
    const int n_batches = (int)((n + B - 1) / B);
    const int rows_p = n_batches * B;
    const int no = (int)k->n_outputs;
    XSet xs;
    DevBuf<T> O;
    if (!net.upload_x(X, (int)n, (int)k->n_inputs, rows_p, &xs)) return FALSE;
    HIPCHK(O.alloc((size_t)B * no));
    std::vector<T> h((size_t)B * no);
    BOOL ok = TRUE;
    for (int b = 0; b < n_batches && ok; b++) {
        int start, nv, total;
        hpnn_dp_shard(b, B, (int)n, 0, B, &start, &nv, &total);
        ok = net.forward(BatchedFP<T>::at(xs, (long)b * B), B);
        if (ok)
            ok = hpnn_output_fp(BatchedFP<T>::F64, net.Z, no, nullptr, 0, nullptr, 0, O.get(), no, nullptr, nullptr, nullptr,
                                B, 0, no, net.type, s) == 0;
        ok = ok && hipMemcpyAsync(h.data(), O.get(), (size_t)nv * no * sizeof(T), hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
        for (size_t i = 0; ok && i < (size_t)nv * no; i++) Y[(size_t)b * B * no + i] = (DOUBLE)h[i];
    }
    return ok;
}

}  // namespace

/* batched evaluation (run_nn on the GPU): the whole test set through the batched engine
 * of the requested precision instead of one online forward per file.  With n_gpu x
 * n_streams > 1 (run_nn -G N -S M, the reference's forward over n_gpu x n_streams,
 * cuda_ann.cu:426-1276) the samples are split into N M contiguous shards, one host thread
 * each on its own (device, stream) (forward only: no communication; outputs land in
 * place).  HPNN_INFER_SHARDS = V runs V shards on device 0, each on its own new stream
 * (tests on one GPU). */
extern "C" BOOL hpnn_gpu_infer_batched(kernel_ann *k, nn_type type, nn_dtype dtype, const DOUBLE *X, UINT n,
                                       DOUBLE *Y) {
    if (!k || n == 0) return FALSE;
    if (dtype != NN_DTYPE_BF16 && dtype != NN_DTYPE_F32 && dtype != NN_DTYPE_F64) {
        NN_ERROR(stderr, "GPU inference: unsupported dtype %d\n", (int)dtype);
        return FALSE;
    }
    hpnn_gpu_sync_host(k);
    const nn_runtime *rt = hpnn_rt_get();
    const int G = rt && rt->cudas.n_gpu > 1 ? (int)rt->cudas.n_gpu : 1;
    const int NS = rt && rt->cudas.cuda_n_streams > 1 ? (int)rt->cudas.cuda_n_streams : 1;
    const char *vs = getenv("HPNN_INFER_SHARDS");
    const int V = vs ? atoi(vs) : 0;
    const bool virt = V >= 2;
    int P = virt ? V : G * NS;
    if ((UINT)P > n) P = (int)n;
    const UINT ni = k->n_inputs, no = k->n_outputs;
    auto shard = [&](int g, hipStream_t s) -> BOOL {
        const UINT lo = (UINT)((UINT64)n * g / P), hi = (UINT)((UINT64)n * (g + 1) / P);
        if (hi == lo) return TRUE;
        const DOUBLE *Xs = X + (size_t)lo * ni;
        DOUBLE *Ys = Y + (size_t)lo * no;
        switch (dtype) {
        case NN_DTYPE_BF16: return infer_bf16(k, type, Xs, hi - lo, Ys, s);
        case NN_DTYPE_F32: return infer_fp<float>(k, type, Xs, hi - lo, Ys, s);
        default: return infer_fp<double>(k, type, Xs, hi - lo, Ys, s);
        }
    };
    if (P <= 1) {
        HIPCHK(hipSetDevice(hpnn_rt_device(0)));
        return shard(0, hpnn_rt_stream(0, 0));
    }
    NN_DBG(stdout, "batched evaluation: %u samples over %d %s\n", n, P,
           virt ? "shards on one GPU" : "(GPU, stream) shards");
    std::vector<int> ok(P, 0);
    std::vector<std::thread> th;
    for (int g = 0; g < P; g++)
        th.emplace_back([&, g]() {
            /* shard g: device g / NS, stream g % NS (consecutive shards on one device) */
            const int dev = hpnn_rt_device(virt ? 0 : (UINT)(g / NS));
            if (hipSetDevice(dev) != hipSuccess) return;
            hipStream_t s = nullptr;
            if (virt) {
                if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return;
            } else {
                s = hpnn_rt_stream((UINT)(g / NS), (UINT)(g % NS));
            }
            ok[g] = shard(g, s) ? 1 : 0;
            if (virt) hipStreamDestroy(s);
        });
    for (auto &t : th) t.join();
    hipSetDevice(hpnn_rt_device(0));
    for (int g = 0; g < P; g++)
        if (!ok[g]) {
            NN_ERROR(stderr, "batched GPU evaluation: shard %d failed\n", g);
            return FALSE;
        }
    return TRUE;
}
