// Nonlinear effective-property map: gp as a ReLU MLP (lamp/neuralnets.py:7-44, components.py:207-210).
//
// Batched over rows: one workgroup of 256 threads takes a tile of TR = 16 rows through every layer.  The
// activations (forward) / deltas (backward) of the tile live in two LDS row buffers that alternate between the
// layers; a layer's weights stream through a 32 x 64 LDS tile (reduction x output index), loaded once per
// workgroup with the lanes along the matrix's contiguous index and bounds-checked element by element, so a
// layer of any size (288 x 512 does not fit LDS) and any row length (21, 26: rows not 16-byte aligned) runs
// the same code.  Wave w owns rows 4 w .. 4 w + 3 of the tile, lane l output 64 t + l of output tile t: four
// fmaf chains per lane over the reduction index in order, starting from the bias -- plain f32 VALU (the f32
// MFMA has the same peak rate and the same chain numerics; here the work is a few MFLOP per step and the odd
// widths would need padded operand images).
//
// The forward's last layer keeps mu_X in registers and finishes the gp term per element with head.hip's own
// expressions (dense_terms.h: X~, logL_X, entropy); the backward starts from the same header's per-element
// gradients (dJ/dmu_X, the q_X rows' and logsigmas_X's) and ends by adding W_1^T delta_1 to the q_z rows'
// gradients (that tail has no KL term: its own expression, not the header's).
#include "common.h"
#include "dense_terms.h"

using namespace gpi;

namespace {

constexpr int TR = 16;            // rows per workgroup
constexpr int NT = 256;           // threads per workgroup
constexpr int OT = 64;            // outputs per weight tile (one per lane)
constexpr int RT = 32;            // reduction indices per weight tile
constexpr int WP = OT + 1;        // LDS pitch of the weight tile
constexpr int VMAX = 512;         // max width
constexpr int ML = GPI_GPMLP_MAX_HIDDEN;

// The network of a launch, read straight from the by-value kernel argument (a runtime layer index is a
// scalar load from the argument segment; a local copy of the per-layer arrays would live in scratch).
struct NetE {                      // ELBO form: parameter offsets into the flat buffer
    const gpi_gpmlp_desc& d;
    const float* P;
    __device__ __forceinline__ int L() const { return d.n_layers; }
    __device__ __forceinline__ int w(int k) const { return d.width[k]; }
    __device__ __forceinline__ const float* W(int k) const { return P + d.w[k]; }
    __device__ __forceinline__ const float* b(int k) const { return P + d.b[k]; }
};
struct NetS {                      // sampling form: plain device pointers
    const gpi_gpmlp_sample_desc& d;
    __device__ __forceinline__ int L() const { return d.n_layers; }
    __device__ __forceinline__ int w(int k) const { return d.width[k]; }
    __device__ __forceinline__ const float* W(int k) const { return d.w[k]; }
    __device__ __forceinline__ const float* b(int k) const { return d.b[k]; }
};

// Ws[rr][oo] = A(o0 + oo, r0 + rr), zero outside the matrix.  W is a torch Linear weight [J][K].
// T = false: output index j, reduction index k (A(j, k) = W[j K + k], lanes along k);
// T = true:  output index k, reduction index j (the transposed product, lanes along k as well).
template <bool T>
__device__ __forceinline__ void stage(float* Ws, const float* __restrict__ W, int J, int K, int o0, int r0) {
    for (int e = threadIdx.x; e < OT * RT; e += NT) {
        int oo, rr;
        float v = 0.f;
        if constexpr (!T) {
            rr = e & (RT - 1);
            oo = e >> 5;
            const int j = o0 + oo, k = r0 + rr;
            if (j < J && k < K) v = W[(int64_t)j * K + k];
        } else {
            oo = e & (OT - 1);
            rr = e >> 6;
            const int j = r0 + rr, k = o0 + oo;
            if (j < J && k < K) v = W[(int64_t)j * K + k];
        }
        Ws[rr * WP + oo] = v;
    }
}

// Y[r][o] = bias[o] + sum_red A(o, red) X[r][red] for the tile's TR rows; epi(row, o, value) for o in range.
// Every thread of the workgroup must call it (barriers inside); the first barrier also orders the previous
// layer's writes of X before this layer's reads.
template <bool T, typename Epi>
__device__ __forceinline__ void layer(const float* __restrict__ W, const float* __restrict__ bias, int J, int K,
                                      const float* X, int px, float* Ws, Epi epi) {
    const int nout = T ? K : J, nred = T ? J : K;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* x0 = X + (4 * wv) * px;
    for (int o0 = 0; o0 < nout; o0 += OT) {
        const int o = o0 + lane;
        const float init = (bias && o < nout) ? bias[o] : 0.f;
        float acc[4] = {init, init, init, init};
        for (int r0 = 0; r0 < nred; r0 += RT) {
            __syncthreads();
            stage<T>(Ws, W, J, K, o0, r0);
            __syncthreads();
            const int nr = min(RT, nred - r0);
            for (int rr = 0; rr < nr; ++rr) {
                const float w = Ws[rr * WP + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(w, x0[i * px + r0 + rr], acc[i]);
            }
        }
        if (o < nout) {
#pragma unroll
            for (int i = 0; i < 4; ++i) epi(4 * wv + i, o, acc[i]);
        }
    }
}

// LDS row buffers: A holds the even members of the layer sequence h_0 .. h_L, B the odd ones
template <typename Net>
__device__ __forceinline__ int pitch_of(const Net& net, int parity) {
    int m = 1;
    for (int k = parity; k <= net.L(); k += 2) m = max(m, net.w(k));
    return m;
}

int host_pitch(const int* seq, int n, int parity) {
    int m = 1;
    for (int k = parity; k < n; k += 2) m = m > seq[k] ? m : seq[k];
    return m;
}

// hidden layers of the forward: h_0 in bufA; returns the buffer and pitch holding h_L.  store(k, row, o, v)
// receives every hidden activation.
template <typename Net, typename Store>
__device__ __forceinline__ void hidden_layers(const Net& net, float* bufA, int pA, float* bufB, int pB, float* Ws,
                                              const float*& X, int& px, Store store) {
    X = bufA;
    px = pA;
    for (int k = 1; k <= net.L(); ++k) {
        float* Y = (k & 1) ? bufB : bufA;
        const int py = (k & 1) ? pB : pA;
        layer<false>(net.W(k - 1), net.b(k - 1), net.w(k), net.w(k - 1), X, px, Ws,
                     [&](int row, int o, float v) {
            const float h = fmaxf(v, 0.f);
            Y[row * py + o] = h;
            store(k, row, o, h);
        });
        X = Y;
        px = py;
    }
}

struct Seg {
    int row;
    int64_t qx_mu, qx_ls, qz_mu, qz_ls;
    float lx_scale;
    int second;
};

__device__ __forceinline__ Seg seg_of(const gpi_gpmlp_desc& d, int q) {
    Seg g;
    if (q >= d.n1) {
        g.row = q - d.n1;
        g.qx_mu = d.qx_mu2; g.qx_ls = d.qx_ls2; g.qz_mu = d.qz_mu2; g.qz_ls = d.qz_ls2;
        g.lx_scale = d.lx_scale2;
        g.second = 1;
    } else {
        g.row = q;
        g.qx_mu = d.qx_mu; g.qx_ls = d.qx_ls; g.qz_mu = d.qz_mu; g.qz_ls = d.qz_ls;
        g.lx_scale = d.lx_scale;
        g.second = 0;
    }
    return g;
}

__global__ __launch_bounds__(NT) void gpmlp_fwd_kernel(gpi_gpmlp_desc d, const float* __restrict__ P, float* ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float scratch[16], red[4];
    const NetE net{d, P};
    const int L = net.L(), dz = net.w(0), dx = net.w(L + 1);
    const int pA = pitch_of(net, 0), pB = pitch_of(net, 1);
    float* bufA = lds;
    float* bufB = bufA + TR * pA;
    float* Ws = bufB + TR * pB;
    const int n = d.n1 + d.n2, q0 = blockIdx.x * TR, nt = min(TR, n - q0);
    const bool lockx = d.flags & GPI_GPMLP_LOCKX;
    for (int e = threadIdx.x; e < TR * dz; e += NT) {
        const int r = e / dz, k = e - r * dz;
        bufA[r * pA + k] = r < nt ? ws[d.z + (int64_t)(q0 + r) * dz + k] : 0.f;
    }
    const float* X;
    int px;
    hidden_layers(net, bufA, pA, bufB, pB, Ws, X, px, [&](int k, int row, int o, float h) {
        if (row < nt) ws[d.h[k - 1] + (int64_t)(q0 + row) * net.w(k) + o] = h;
    });
    float acc4[4] = {0.f, 0.f, 0.f, 0.f};   // logL_X, entropy of segment 1; of segment 2
    layer<false>(net.W(L), net.b(L), dx, net.w(L), X, px, Ws, [&](int row, int t, float a) {
        if (row >= nt) return;
        const int q = q0 + row;
        const int64_t qi = (int64_t)q * dx + t;
        if (lockx) {                                            // X~ = gp(z) (generative.py:432)
            ws[d.mux + qi] = a;
            ws[d.xs + qi] = a;
            return;
        }
        const Seg sg = seg_of(d, q);
        const int64_t pi = (int64_t)sg.row * dx + t;            // q_X parameter row
        const float lsq = P[sg.qx_ls + pi];
        const GpElemFwd E(P[sg.qx_mu + pi], lsq, ws[d.eps_x + qi]);
        ws[d.mux + qi] = a;
        ws[d.xs + qi] = E.xs;
        const float lx = E.loglik(a, P[d.gp_ls + t]);
        acc4[0] += sg.second ? 0.f : lx;
        acc4[1] += sg.second ? 0.f : lsq;
        acc4[2] += sg.second ? lx : 0.f;
        acc4[3] += sg.second ? lsq : 0.f;
    });
    if (lockx) return;   // uniform
    block_sum<4>(acc4, scratch, red);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int r = blockIdx.x % GPI_REPLICAS;
        if (q0 < d.n1) {
            atomicAdd(d.terms + 0 * GPI_REPLICAS + r, (double)red[0]);
            atomicAdd(d.terms + 1 * GPI_REPLICAS + r, (double)red[1]);
        }
        if (q0 + nt > d.n1) {
            atomicAdd(d.terms2 + 0 * GPI_REPLICAS + r, (double)red[2]);
            atomicAdd(d.terms2 + 1 * GPI_REPLICAS + r, (double)red[3]);
        }
    }
}

__global__ __launch_bounds__(NT) void gpmlp_bwd_kernel(gpi_gpmlp_desc d, const float* __restrict__ P, float* ws,
                                                       double* gacc) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const NetE net{d, P};
    const int L = net.L(), dz = net.w(0), dx = net.w(L + 1);
    // delta sequence: delta_{L+1} (width d_x) in buffer A, delta_L in B, delta_{L-1} in A, ...
    int pA = 1, pB = 1;
    for (int j = 1; j <= L + 1; ++j) {
        if (((L + 1 - j) & 1) == 0) pA = max(pA, net.w(j));
        else pB = max(pB, net.w(j));
    }
    float* bufA = lds;
    float* bufB = bufA + TR * pA;
    float* Ws = bufB + TR * pB;
    const int n = d.n1 + d.n2, q0 = blockIdx.x * TR, nt = min(TR, n - q0);
    const bool lockx = d.flags & GPI_GPMLP_LOCKX;
    // delta_{L+1} = dJ/dmu_X -> bufA (and gmux), the q_X rows' and logsigmas_X's gradients: one thread per
    // feature t runs over the tile's rows in order (head_bwd_mfma's form)
    for (int t = threadIdx.x; t < dx; t += NT) {
        double gls_sum = 0.0;
#pragma unroll 4
        for (int si = 0; si < TR; ++si) {
            if (si >= nt) {
                bufA[si * pA + t] = 0.f;
                continue;
            }
            const int q = q0 + si;
            const int64_t qi = (int64_t)q * dx + t;
            if (lockx) {                                       // dJ/dmu_X = dJ/dX~ (the ROM adjoint)
                const float gm = ws[d.gxs + qi];
                bufA[si * pA + t] = gm;
                ws[d.gmux + qi] = gm;
                continue;
            }
            const Seg sg = seg_of(d, q);
            const int64_t pi = (int64_t)sg.row * dx + t;
            const float gls = P[d.gp_ls + t];
            const GpElemBwd G(ws[d.xs + qi], ws[d.mux + qi], gls, sg.lx_scale);
            const float gm = G.gmux();
            bufA[si * pA + t] = gm;
            ws[d.gmux + qi] = gm;
            gls_sum += (double)G.gls();
            const float dxs = G.gqx_mu(ws[d.gxs + qi]);
            const float lsq = P[sg.qx_ls + pi];
            atomicAdd(gacc + sg.qx_mu + pi, (double)dxs);
            atomicAdd(gacc + sg.qx_ls + pi, (double)G.gqx_ls(dxs, lsq, ws[d.eps_x + qi]));
        }
        if (!lockx) atomicAdd(gacc + d.gp_ls + t, gls_sum);
    }
    // delta_k = (W_{k+1}^T delta_{k+1}) * [h_k > 0], k = L .. 1
    const float* X = bufA;
    int px = pA;
    for (int k = L; k >= 1; --k) {
        const int step = L + 1 - k;                            // position of delta_k in the sequence
        float* Y = (step & 1) ? bufB : bufA;
        const int py = (step & 1) ? pB : pA;
        const int wk = net.w(k);
        const int64_t hk = d.h[k - 1], dhk = d.dh[k - 1];
        layer<true>(net.W(k), nullptr, net.w(k + 1), wk, X, px, Ws, [&](int row, int o, float v) {
            float g = 0.f;
            if (row < nt) {
                const int64_t hi = (int64_t)(q0 + row) * wk + o;
                g = ws[hk + hi] > 0.f ? v : 0.f;
                ws[dhk + hi] = g;
            }
            Y[row * py + o] = g;
        });
        X = Y;
        px = py;
    }
    // W_1^T delta_1 into the q_z rows' gradients
    layer<true>(net.W(0), nullptr, net.w(1), dz, X, px, Ws, [&](int row, int k, float v) {
        if (row >= nt) return;
        const int q = q0 + row;
        const int64_t zi = (int64_t)q * dz + k;
        if (d.dz >= 0) ws[d.dz + zi] = v;
        const Seg sg = seg_of(d, q);
        if (sg.qz_mu < 0) return;
        const int64_t qi = (int64_t)sg.row * dz + k;
        const float ex = expf(P[sg.qz_ls + qi]);
        atomicAdd(gacc + sg.qz_mu + qi, (double)v);
        atomicAdd(gacc + sg.qz_ls + qi, (double)(v * ex * ws[d.eps_z + zi]));
    });
}

__global__ __launch_bounds__(NT) void gpmlp_sample_kernel(gpi_gpmlp_sample_desc d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const NetS net{d};
    const int L = net.L(), dz = net.w(0), dx = net.w(L + 1);
    const int pA = pitch_of(net, 0), pB = pitch_of(net, 1);
    float* bufA = lds;
    float* bufB = bufA + TR * pA;
    float* Ws = bufB + TR * pB;
    const int64_t r0 = (int64_t)blockIdx.x * TR;
    const int nt = (int)min((int64_t)TR, (int64_t)d.rows - r0);
    const uint64_t base = d.offset ? *d.offset : 0;
    for (int e = threadIdx.x; e < TR * dz; e += NT) {
        const int ri = e / dz, k = e - ri * dz;
        float z = 0.f;
        if (ri < nt) {
            const int64_t r = r0 + ri, j = r / d.rep;
            z = d.qz_mu[j * dz + k];
            if (d.qz_ls) {
                const int64_t ee = r * dz + k;
                const float ez = d.eps_z ? d.eps_z[ee] : normal_at(base + (uint64_t)ee, d.sub, d.seed);
                z = fmaf(expf(d.qz_ls[j * dz + k]), ez, z);
            }
        }
        bufA[ri * pA + k] = z;
    }
    const float* X;
    int px;
    hidden_layers(net, bufA, pA, bufB, pB, Ws, X, px, [](int, int, int, float) {});
    layer<false>(net.W(L), net.b(L), dx, net.w(L), X, px, Ws, [&](int row, int t, float a) {
        if (row >= nt) return;
        const int64_t e = (r0 + row) * dx + t;
        if (d.gp_ls) {
            const float ex = d.eps_x ? d.eps_x[e] : normal_at(base + (uint64_t)e, d.sub + 1, d.seed);
            a = fmaf(expf(d.gp_ls[t]), ex, a);
        }
        d.x[e] = a;
    });
}

int widths_ok(int L, const int32_t* w) {
    if (L < 1) return GPI_ERR_ARG;
    if (L > ML) return GPI_ERR_UNSUPPORTED;
    for (int k = 0; k <= L + 1; ++k)
        if (w[k] < 1 || w[k] > VMAX) return GPI_ERR_ARG;
    return GPI_OK;
}

// dynamic LDS of a launch over the row-buffer sequence seq[0..n); kernels above 64 KB need the attribute
template <typename K>
int lds_bytes(K kernel, const int* seq, int n, size_t& bytes) {
    bytes = sizeof(float) * ((size_t)TR * (host_pitch(seq, n, 0) + host_pitch(seq, n, 1)) + RT * WP);
    if (bytes > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bytes) != hipSuccess)
        return GPI_ERR_LAUNCH;
    return GPI_OK;
}

int desc_ok(const gpi_gpmlp_desc* d, const float* params, float* ws) {
    if (!d || !params || !ws) return GPI_ERR_ARG;
    const int rc = widths_ok(d->n_layers, d->width);
    if (rc != GPI_OK) return rc;
    if (d->n1 < 0 || d->n2 < 0) return GPI_ERR_ARG;
    const bool lockx = d->flags & GPI_GPMLP_LOCKX;
    if (!lockx && (d->gp_ls < 0 || (d->n1 > 0 && (d->qx_mu < 0 || d->qx_ls < 0 || !d->terms)) ||
                   (d->n2 > 0 && (d->qx_mu2 < 0 || d->qx_ls2 < 0 || !d->terms2))))
        return GPI_ERR_ARG;
    for (int k = 0; k <= d->n_layers; ++k)
        if (d->w[k] < 0 || d->b[k] < 0) return GPI_ERR_ARG;
    // workspace buffers in use (-1 = absent in the header's convention: never a valid offset here)
    if (d->z < 0 || d->xs < 0 || d->mux < 0) return GPI_ERR_ARG;
    if (!lockx && d->eps_x < 0) return GPI_ERR_ARG;
    for (int k = 0; k < d->n_layers; ++k)
        if (d->h[k] < 0) return GPI_ERR_ARG;
    return GPI_OK;
}

// what only the backward touches
int desc_ok_bwd(const gpi_gpmlp_desc* d) {
    if (d->gxs < 0 || d->gmux < 0) return GPI_ERR_ARG;
    for (int k = 0; k < d->n_layers; ++k)
        if (d->dh[k] < 0) return GPI_ERR_ARG;
    const bool qz = (d->n1 > 0 && d->qz_mu >= 0) || (d->n2 > 0 && d->qz_mu2 >= 0);
    if ((d->n1 > 0 && (d->qz_mu >= 0) != (d->qz_ls >= 0)) || (d->n2 > 0 && (d->qz_mu2 >= 0) != (d->qz_ls2 >= 0)))
        return GPI_ERR_ARG;
    if (qz && d->eps_z < 0) return GPI_ERR_ARG;
    return GPI_OK;
}

}  // namespace

extern "C" int gpi_gpmlp_forward(const gpi_gpmlp_desc* d, const float* params, float* ws, void* stream) {
    const int rc = desc_ok(d, params, ws);
    if (rc != GPI_OK) return rc;
    const int n = d->n1 + d->n2;
    if (n == 0) return GPI_OK;
    size_t bytes;
    const int lc = lds_bytes(gpmlp_fwd_kernel, d->width, d->n_layers + 1, bytes);
    if (lc != GPI_OK) return lc;
    hipLaunchKernelGGL(gpmlp_fwd_kernel, dim3((n + TR - 1) / TR), dim3(NT), bytes, (hipStream_t)stream, *d, params, ws);
    GPI_CHECK_LAUNCH();
    return GPI_OK;
}

extern "C" int gpi_gpmlp_backward(const gpi_gpmlp_desc* d, const float* params, float* ws, double* gacc,
                                  void* stream) {
    const int rc = desc_ok(d, params, ws);
    if (rc != GPI_OK) return rc;
    if (!gacc || desc_ok_bwd(d) != GPI_OK) return GPI_ERR_ARG;
    const int n = d->n1 + d->n2;
    if (n == 0) return GPI_OK;
    int seq[ML + 1];
    for (int k = 0; k <= d->n_layers; ++k) seq[k] = d->width[d->n_layers + 1 - k];
    size_t bytes;
    const int lc = lds_bytes(gpmlp_bwd_kernel, seq, d->n_layers + 1, bytes);
    if (lc != GPI_OK) return lc;
    hipLaunchKernelGGL(gpmlp_bwd_kernel, dim3((n + TR - 1) / TR), dim3(NT), bytes, (hipStream_t)stream, *d, params, ws,
                       gacc);
    GPI_CHECK_LAUNCH();
    return GPI_OK;
}

extern "C" int gpi_gpmlp_sample(const gpi_gpmlp_sample_desc* d, void* stream) {
    if (!d) return GPI_ERR_ARG;
    const int rc = widths_ok(d->n_layers, d->width);
    if (rc != GPI_OK) return rc;
    if (!d->qz_mu || !d->x || d->rows < 0 || d->rep < 1 || d->rows % d->rep != 0) return GPI_ERR_ARG;
    if ((d->eps_z && !d->qz_ls) || (d->eps_x && !d->gp_ls)) return GPI_ERR_ARG;    // noise for a draw that is not made
    for (int k = 0; k <= d->n_layers; ++k)
        if (!d->w[k] || !d->b[k]) return GPI_ERR_ARG;
    if (d->rows == 0) return GPI_OK;
    size_t bytes;
    const int lc = lds_bytes(gpmlp_sample_kernel, d->width, d->n_layers + 1, bytes);
    if (lc != GPI_OK) return lc;
    hipLaunchKernelGGL(gpmlp_sample_kernel, dim3((d->rows + TR - 1) / TR), dim3(NT), bytes, (hipStream_t)stream, *d);
    GPI_CHECK_LAUNCH();
    return GPI_OK;
}
