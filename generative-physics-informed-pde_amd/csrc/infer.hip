// Inference (eval-mode) helpers of libgpi_hip.so.
//
// Eval-mode BatchNorm is a per-channel affine map from the layer's running statistics.  The conv
// kernels (conv.hip) already apply relu(BN) on load from the fp64 (sum, sum^2) records of their input
// channels, so an eval forward needs no kernel of its own: gpi_bn_eval_seed writes, for every BN layer,
// the records whose mean and biased variance ARE the running statistics, and the unchanged forward
// kernels (epilogue GPI_EPI_STORE: no statistics of their own) consume them.
//
// gpi_affine is the surrogate predictor's gp mean (effective-property map without noise).
#include "common.h"

namespace {

// One thread per (BN layer, channel): replica 0 of group 0 gets the seeded sums, the other replicas of
// group 0 are cleared (the readers sum all GPI_REPLICAS copies).  One thread owns one record of every
// replica: plain stores, no atomics.
__global__ __launch_bounds__(256) void bn_eval_seed_kernel(const gpi_bn_eval_item* items, int n_items, int max_ch,
                                                           gpi_stat* stats, int64_t n_stats) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int li = t / max_ch, c = t - li * max_ch;
    if (li >= n_items) return;
    const gpi_bn_eval_item it = items[li];
    if (c >= it.channels || it.stat < 0 || it.stat + c >= n_stats) return;
    const double n = it.count;
    const double m = (double)it.running_mean[c], v = (double)it.running_var[c];
    // sum / n == m exactly (n m is exact in fp64 for an fp32 m and n < 2^29), sumsq / n - m^2 == v to fp64
    // rounding: bn_mean_invstd returns (running_mean, 1 / sqrt(running_var + eps))
    const double s = n * m, s2 = n * (v + m * m);
    for (int r = 0; r < GPI_REPLICAS; ++r) {
        gpi_stat& st = stats[(int64_t)r * GPI_MAX_GROUPS * n_stats + it.stat + c];
        st.sum = r == 0 ? s : 0.0;
        st.sumsq = r == 0 ? s2 : 0.0;
    }
}

// out[r][m] = b[m] + sum_k W[m][k] in[r][k]; one thread per output, fp64 accumulation (d_in is a
// latent dimension: tens of terms).
__global__ __launch_bounds__(256) void affine_kernel(const float* __restrict__ W, const float* __restrict__ b,
                                                     const float* __restrict__ in, float* __restrict__ out,
                                                     int rows, int d_out, int d_in) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)rows * d_out) return;
    const int r = (int)(t / d_out), m = (int)(t - (int64_t)r * d_out);
    const float* w = W + (int64_t)m * d_in;
    const float* x = in + (int64_t)r * d_in;
    double acc = b ? (double)b[m] : 0.0;
    for (int k = 0; k < d_in; ++k) acc = fma((double)w[k], (double)x[k], acc);
    out[t] = (float)acc;
}

}  // namespace

extern "C" int gpi_bn_eval_seed(const gpi_bn_eval_item* items, int n_items, int max_channels, gpi_stat* stats,
                                int64_t n_stats, void* stream) {
    if (!items || !stats || n_items <= 0 || max_channels < 1 || n_stats < 1) return GPI_ERR_ARG;
    if ((int64_t)n_items * max_channels > (int64_t)1 << 30) return GPI_ERR_ARG;
    const int threads = n_items * max_channels;
    hipLaunchKernelGGL(bn_eval_seed_kernel, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, items,
                       n_items, max_channels, stats, n_stats);
    GPI_CHECK_LAUNCH();
    return GPI_OK;
}

extern "C" int gpi_affine(const float* W, const float* b, const float* in, float* out, int rows, int d_out, int d_in,
                          void* stream) {
    if (!W || !in || !out || rows <= 0 || d_out <= 0 || d_in <= 0) return GPI_ERR_ARG;
    const int64_t n = (int64_t)rows * d_out;
    if (n > (int64_t)1 << 30) return GPI_ERR_ARG;
    hipLaunchKernelGGL(affine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, b, in,
                       out, rows, d_out, d_in);
    GPI_CHECK_LAUNCH();
    return GPI_OK;
}
