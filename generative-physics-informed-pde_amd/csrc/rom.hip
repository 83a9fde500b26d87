// Coarse-grained model (ROM) solve for gfx950: one wave64 per sample.
//
// Reference: ROM.__call__ / GetStiffness / _solve_eqs (bottleneck/ROM.py:59-100)
// builds a dense K(x) = M x^T from the FEniCS tensor M, overwrites the
// Dirichlet rows with identity rows and calls a batched dense LU solve;
// ReducedOrderModelOperator (components.py:296-298) then prolongates with the
// dense P1 matrix W.  Here:
//   * K is the closed-form 5-point stencil of the coarse "/" mesh
//     (physics/grid.py), assembled directly into banded LDS storage;
//   * the Dirichlet nodes are eliminated (u_B = F_B, rhs -= K_IB F_B): the
//     SPD interior system has the same solution as the row-replaced one;
//   * banded Cholesky (bandwidth nc-1) in LDS, no pivoting needed (SPD);
//   * mu_y = W u is evaluated from the closed-form P1 interpolation weights;
//   * LOGLIK mode fuses DiagonalGaussianLogLikelihood(Y, mu_y, 2 logsigma_y)
//     and its adjoint: lambda = K_II^{-1} W^T dmu,
//     dJ/dc_pq = -(lambda_p - lambda_q)(u_p - u_q), dJ/dkappa_t = 1/2 sum over
//     its two legs, dJ/dx = dJ/dkappa * exp(x); optional 0/1 observation weights of the label entries (y_weight:
//     partially observed labels; an entry with weight 0 is never read into a result), as instantiations of their
//     own (YW), so that a launch without weights runs the kernels it ran before;
//   * nc = 4 / 8: rom_kernel_fast (Z = L^{-1} by one wave) and rom_lane_kernel; nc = 16: rom_kernel_fast<16> with
//     the factorisation and the band sweeps by one wave whose lanes share the window (chol16_wave, band_sweep16)
//     and rom16_coarse_kernel; any other nc <= 16, and GPI_ROM_SLOW=1: the barrier-per-step rom_kernel;
//   * gpi_rom_fit (rom_fit_kernel<4 | 8 | 16>, below): OptimizeEffectiveProperties' whole Adam loop over x
//     in one launch.
// Every kernel is put together from one statement of each block of the mathematics:
//   kappa_of                    kappa from x, with the bad-value flag
//   band_row                    one interior row of K and its right-hand side (c_h, c_v, Dirichlet lift of F),
//                               returned as values; put_band_row stores it in the band layout L[ii * W + t]
//   interior_node, u_node,      the interior <-> node index maps: u from (b, F), lambda from b with 0 on the
//   lam_node                    Dirichlet nodes
//   dk_edge, dx_of_dk           dJ/dkappa of a coarse triangle by the edge formula, and dJ/dx from it
//   loglik_sum, gx_store        the workgroup's log-likelihood sum; dJ/dx per triangle into the gx row
//   win_load, win_step,         the register-window Cholesky step and the substitutions' sliding window
//   win_shift, win_row, h_push  (chol_band_seq, chol_inv_wave, solve_band_seq)
//   fit_square_sums, fit_node_gather, fit_gu_row, adam_step, fit_update     the pieces of the fit
// and every kernel family takes its dynamic-LDS carve-up and its launch size from one layout (rom_lds,
// RomFastLds, Rom16CoarseLds, RomLaneLds, RomFitLds).
#include "common.h"
#include <stdlib.h>
#include <type_traits>

using namespace gpi;

namespace {

// the log effective property of sample row `row` (x rows at d.x_stride), element t: stored, or drawn here
// from q_X (x_draw: the head's fmaf(expf(logsigma), eps, mu), so both hold the same value)
__device__ __forceinline__ float rom_x(const gpi_rom_desc& d, int64_t row, int t) {
    const int64_t o = row * d.x_stride + t;
    if (d.x_draw) return fmaf(expf(d.x_ls[o]), d.x_eps[o], d.x_mu[o]);
    return d.x[o];
}

// Phase stamps of the timing build (make timing; tools/rom_probe.py): thread 0 of workgroup b writes
// the shader clock at phase boundary i to g_rom_phase[b % 256][i].  Compiled out of the product.
#ifdef GPI_PHASE_TIMING
__device__ unsigned long long g_rom_phase[256 * 8];
#define RPHASE(i)                                                                                       \
    do {                                                                                                \
        if (threadIdx.x == 0) g_rom_phase[(blockIdx.x & 255) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define RPHASE(i) \
    do {          \
    } while (0)
#endif

struct RomDims {
    int nc, nn, nT, nI, bw, n, dy, r;
};

// kappa of one triangle from its x; `bad` collects the values that are not positive numbers (d.flag)
__device__ __forceinline__ float kappa_of(float xv, bool input_kappa, bool& bad) {
    const float kv = input_kappa ? xv : expf(xv) + 1e-8f;
    bad |= !(kv > 1e-12f);
    return kv;
}

// kappa accessor of band_row: triangle t -> kappa, from the LDS image kp[]
struct LdsKappa {
    const float* kp;
    __device__ __forceinline__ float operator()(int t) const { return kp[t]; }
};

// horizontal edge (I,J)-(I+1,J); triangle (I, J, ul) is element 2 (I + nc J) + ul
template <class K>
__device__ __forceinline__ float c_h(const K& kap, int nc, int I, int J) {
    float c = 0.f;
    if (J < nc) c += kap(2 * (I + nc * J));
    if (J > 0) c += kap(2 * (I + nc * (J - 1)) + 1);
    return 0.5f * c;
}
// vertical edge (I,J)-(I,J+1)
template <class K>
__device__ __forceinline__ float c_v(const K& kap, int nc, int I, int J) {
    float c = 0.f;
    if (I > 0) c += kap(2 * (I - 1 + nc * J));
    if (I < nc) c += kap(2 * (I + nc * J) + 1);
    return 0.5f * c;
}

// Interior row ii of K (lower band) and of the right-hand side: the diagonal, the first and the (nc-1)-th
// sub-diagonal, and F at the node with the Dirichlet neighbours lifted (rhs -= K_IB F_B).  Every kernel
// stores these in its own layout.
struct BandRow {
    float dg, o1, on, rhs;
};
template <class K>
__device__ __forceinline__ BandRow band_row(int nc, int ii, const float* F, const K& kap) {
    const int J = ii / (nc - 1), I = ii - J * (nc - 1) + 1;
    const int p = I + (nc + 1) * J;
    const float chl = c_h(kap, nc, I - 1, J), chr = c_h(kap, nc, I, J);
    const float cvd = J > 0 ? c_v(kap, nc, I, J - 1) : 0.f;
    const float cvu = J < nc ? c_v(kap, nc, I, J) : 0.f;
    BandRow r;
    r.dg = chl + chr + cvd + cvu;
    r.o1 = I - 1 >= 1 ? -chl : 0.f;
    r.on = J >= 1 ? -cvd : 0.f;
    r.rhs = F[p];
    if (I - 1 == 0) r.rhs += chl * F[p - 1];
    if (I + 1 == nc) r.rhs += chr * F[p + 1];
    return r;
}
// ... in the band layout: row[t] = K(ii, ii - t), t < w = nc
__device__ __forceinline__ void put_band_row(float* row, int w, const BandRow& r) {
    for (int t = 0; t < w; ++t) row[t] = 0.f;
    row[0] = r.dg;
    row[1] += r.o1;
    row[w - 1] += r.on;
}

// node of interior unknown ii (rows of nc - 1 interior nodes; the columns I = 0, nc are Dirichlet)
__device__ __forceinline__ int interior_node(int nc, int ii) {
    const int J = ii / (nc - 1), I = ii - J * (nc - 1) + 1;
    return I + (nc + 1) * J;
}
__device__ __forceinline__ int interior_of(int nc, int I, int J) { return J * (nc - 1) + (I - 1); }
// coarse solution at node e from the interior solution b and the boundary values F
__device__ __forceinline__ float u_node(int nc, int e, const float* F, const float* b) {
    const int I = e % (nc + 1), J = e / (nc + 1);
    return (I == 0 || I == nc) ? F[e] : b[interior_of(nc, I, J)];
}
// its adjoint twin: lambda at node e, 0 on the Dirichlet nodes
__device__ __forceinline__ float lam_node(int nc, int e, const float* b) {
    const int I = e % (nc + 1), J = e / (nc + 1);
    return (I == 0 || I == nc) ? 0.f : b[interior_of(nc, I, J)];
}

// dJ/dkappa_t of coarse triangle t (times 2): -(lambda_p - lambda_q)(u_p - u_q) over its two legs
__device__ __forceinline__ float dk_edge(const float* lam, const float* u, int nc, int t) {
    const int q = t >> 1, ul = t & 1;
    const int I = q % nc, J = q / nc;
    const int v0 = I + (nc + 1) * J, v1 = v0 + 1, v2 = v0 + (nc + 1), v3 = v2 + 1;
    if (!ul)   // legs v0-v1 (bottom), v1-v3 (right)
        return -(lam[v0] - lam[v1]) * (u[v0] - u[v1]) - (lam[v1] - lam[v3]) * (u[v1] - u[v3]);
    // legs v2-v3 (top), v0-v2 (left)
    return -(lam[v2] - lam[v3]) * (u[v2] - u[v3]) - (lam[v0] - lam[v2]) * (u[v0] - u[v2]);
}
// dJ/dx_t from it: dkappa/dx = exp(x) = kappa - 1e-8
__device__ __forceinline__ float dx_of_dk(float dk, float kv, bool input_kappa) {
    return 0.5f * dk * (input_kappa ? 1.f : (kv - 1e-8f));
}

__device__ void chol_band(float* L, const RomDims& D) {
    const int w = D.bw + 1;
    const int lane = threadIdx.x, NT = blockDim.x;
    for (int k = 0; k < D.nI; ++k) {
        const float dkk = sqrtf(L[k * w]);
        __syncthreads();
        for (int t = 1 + lane; t <= D.bw; t += NT)
            if (k + t < D.nI) L[(k + t) * w + t] /= dkk;
        if (lane == 0) L[k * w] = dkk;
        __syncthreads();
        const int np = D.bw * (D.bw + 1) / 2;
        for (int e = lane; e < np; e += NT) {
            // decode e -> (t1 >= t2) in [1, bw]
            int t1 = 1, rem = e;
            while (rem >= t1) { rem -= t1; ++t1; }
            const int t2 = rem + 1;
            const int i = k + t1, j = k + t2;
            if (i < D.nI) L[i * w + (t1 - t2)] -= L[i * w + t1] * L[j * w + t2];
        }
        __syncthreads();
    }
}

// solve L L^T x = b in place (b -> x)
__device__ void solve_band(const float* L, float* b, const RomDims& D) {
    const int w = D.bw + 1;
    const int lane = threadIdx.x, NT = blockDim.x;
    for (int k = 0; k < D.nI; ++k) {
        const float yk = b[k] / L[k * w];
        __syncthreads();
        for (int t = 1 + lane; t <= D.bw; t += NT)
            if (k + t < D.nI) b[k + t] -= L[(k + t) * w + t] * yk;
        if (lane == 0) b[k] = yk;
        __syncthreads();
    }
    for (int k = D.nI - 1; k >= 0; --k) {
        const float xk = b[k] / L[k * w];
        __syncthreads();
        for (int t = 1 + lane; t <= D.bw; t += NT)
            if (k - t >= 0) b[k - t] -= L[k * w + t] * xk;
        if (lane == 0) b[k] = xk;
        __syncthreads();
    }
}

// Single-thread banded Cholesky / solves for the common coarse grids (nc = 4, 8): the band
// is only bw + 1 = nc wide, so the factorisation is a chain of nI dependent sqrt / scale /
// rank-1-update steps.  Run by one lane with the active (bw+1) x (bw+1) window in registers
// and the loop fully unrolled (every window index static: the window shift is register
// renaming), it costs ~40 VALU instructions per step instead of three LDS round trips and
// three workgroup barriers (78 -> ~10 us for the 63-unknown system at nc = 8).
// dinv[k] = 1 / L(k,k) is kept for the solves, which run as partially unrolled loops (a full
// unroll lets the scheduler hoist every band load and spill).
// The window win[a][t] = L(k + a, k + a - t) and its moves, shared by chol_band_seq, chol_inv_wave and
// (written out once more in) rom_lane_kernel.
// row k of the band (zero past the end)
template <int W>
__device__ __forceinline__ void win_row(float (&row)[W], const float* L, int k, int NI) {
#pragma unroll
    for (int t = 0; t < W; ++t) row[t] = (k < NI) ? L[k * W + t] : 0.f;
}
template <int W>
__device__ __forceinline__ void win_load(float (&win)[W][W], const float* L, int NI) {
#pragma unroll
    for (int a = 0; a < W; ++a)
#pragma unroll
        for (int t = 0; t < W; ++t) win[a][t] = a < NI ? L[a * W + t] : 0.f;
}
// factorisation step k with inv = 1 / L(k,k): scale column k, rank-1 update of the trailing window
template <int W>
__device__ __forceinline__ void win_step(float (&win)[W][W], float inv) {
#pragma unroll
    for (int a = 1; a < W; ++a) win[a][a] *= inv;                       // L(k+a, k)
#pragma unroll
    for (int a = 1; a < W; ++a)
#pragma unroll
        for (int b = 1; b <= a; ++b) win[a][a - b] = fmaf(-win[a][a], win[b][b], win[a][a - b]);
}
// row k leaves: rows move up (register renaming), the caller refills win[W - 1]
template <int W>
__device__ __forceinline__ void win_shift(float (&win)[W][W]) {
#pragma unroll
    for (int a = 0; a + 1 < W; ++a)
#pragma unroll
        for (int t = 0; t < W; ++t) win[a][t] = win[a + 1][t];
}
// the substitutions' sliding window of the last BW values: h[t-1] = y[k - t] (forward), x[k + t] (backward)
template <int BW>
__device__ __forceinline__ void h_clear(float (&h)[BW]) {
#pragma unroll
    for (int t = 0; t < BW; ++t) h[t] = 0.f;
}
template <int BW>
__device__ __forceinline__ void h_push(float (&h)[BW], float a) {
#pragma unroll
    for (int t = BW - 1; t > 0; --t) h[t] = h[t - 1];
    h[0] = a;
}

template <int NC>
__device__ __forceinline__ void chol_band_seq(float* __restrict__ L, float* __restrict__ dinv) {
    constexpr int W = NC, NI = (NC - 1) * (NC + 1);
    float win[W][W];
    win_load<W>(win, L, NI);
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const float dk = sqrtf(win[0][0]);
        const float inv = 1.f / dk;
        win[0][0] = dk;
        dinv[k] = inv;
        win_step<W>(win, inv);
#pragma unroll
        for (int t = 0; t < W; ++t) L[k * W + t] = win[0][t];
        win_shift<W>(win);
        win_row<W>(win[W - 1], L, k + W, NI);
    }
}

// L L^T x = b in place, single lane (see chol_band_seq)
template <int NC>
__device__ __forceinline__ void solve_band_seq(const float* __restrict__ L, const float* __restrict__ dinv,
                                               float* __restrict__ b) {
    constexpr int BW = NC - 1, W = NC, NI = (NC - 1) * (NC + 1);
    float h[BW];
    h_clear(h);
#pragma unroll 8
    for (int k = 0; k < NI; ++k) {
        float a = b[k];
#pragma unroll
        for (int t = 1; t <= BW; ++t)
            if (k - t >= 0) a = fmaf(-L[k * W + t], h[t - 1], a);
        a *= dinv[k];
        b[k] = a;
        h_push(h, a);
    }
    h_clear(h);
#pragma unroll 8
    for (int k = NI - 1; k >= 0; --k) {
        float a = b[k];
#pragma unroll
        for (int t = 1; t <= BW; ++t)
            if (k + t < NI) a = fmaf(-L[(k + t) * W + t], h[t - 1], a);
        a *= dinv[k];
        b[k] = a;
        h_push(h, a);
    }
}

__device__ __forceinline__ void interp(int i, int j, int r, int nc, int& n00, int& n10, int& n11, float& w0,
                                       float& w1, float& w2) {
    int I = i / r, J = j / r;
    if (I > nc - 1) I = nc - 1;
    if (J > nc - 1) J = nc - 1;
    const float xi = (float)(i - I * r) / (float)r, eta = (float)(j - J * r) / (float)r;
    n00 = I + (nc + 1) * J;
    n11 = n00 + (nc + 1) + 1;
    if (xi >= eta) { n10 = n00 + 1; w0 = 1.f - xi; w1 = xi - eta; w2 = eta; }
    else { n10 = n00 + (nc + 1); w0 = 1.f - eta; w1 = eta - xi; w2 = xi; }
}

#ifndef GPI_ROM_NT
#define GPI_ROM_NT 256
#endif
constexpr int ROM_NT = GPI_ROM_NT;   // threads per sample
constexpr int ROM_U = 8;         // fine nodes per batch of global loads
#ifndef GPI_ROM_FAST_NT_DEFAULT
#define GPI_ROM_FAST_NT_DEFAULT 512
#endif

// observation weight of label entry (row s, fine free node pp) of a launch that has weights (d.y_weight:
// one shared row at yw_stride = 0, or rows [n, d_y])
__device__ __forceinline__ float rom_yw(const gpi_rom_desc& d, int64_t s, int pp) {
    return d.y_weight[s * d.yw_stride + pp];
}

// the workgroup's log-likelihood: per-wave sums through lred[NW], in wave order, into the sample's replica
template <int NW>
__device__ __forceinline__ void loglik_sum(const gpi_rom_desc& d, float Lsum, double* lred) {
    const int tid = threadIdx.x;
    Lsum = wave_sum(Lsum);
    if ((tid & 63) == 0) lred[tid >> 6] = (double)Lsum;
    __syncthreads();
    if (tid == 0 && d.loss_acc) {
        double t = lred[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += lred[w];
        atomicAdd(d.loss_acc + blockIdx.x % GPI_REPLICAS, t);
    }
}
// dJ/dx per coarse triangle into the sample's gx row (NT threads)
template <int NT>
__device__ __forceinline__ void gx_store(const gpi_rom_desc& d, int s, int nc, int nT, const float* lam,
                                         const float* u, const float* kp) {
    for (int t = threadIdx.x; t < nT; t += NT) {
        const float g = dx_of_dk(dk_edge(lam, u, nc, t), kp[t], d.input_kappa);
        float* gp = d.gx + (int64_t)s * d.gx_stride + t;
        *gp = (d.gx_accumulate ? *gp : 0.f) + g;
    }
}

// rom_kernel's dynamic LDS: float offsets (the fp64 block at an even one) and the launch size
struct RomLds {
    int kp, L, u, b, lam, du, lred, dinv;
    size_t bytes;
};
__host__ __device__ __forceinline__ RomLds rom_lds(const RomDims& D) {
    RomLds o;
    o.kp = 0;                              // [nT] kappa
    o.L = o.kp + D.nT;                     // [nI * w]
    o.u = o.L + D.nI * (D.bw + 1);         // [nn]
    o.b = o.u + D.nn;                      // [nI]
    o.lam = o.b + D.nI;                    // [nn]
    const int fl = o.lam + D.nn;
    o.du = (fl + 1) & ~1;                  // [nn] fp64 W^T dmu
    o.lred = o.du + 2 * D.nn;              // [ROM_NT / 64] fp64 per-wave log-likelihood sums
    o.dinv = o.lred + 2 * (ROM_NT / 64);   // [nI] 1 / L(k,k) (nc = 4, 8 path)
    o.bytes = sizeof(float) * (fl + 4 + 2 * D.nn + 2 * (ROM_NT / 64) + D.nI);   // 4 floats of alignment slack
    return o;
}

// YW: the launch has observation weights (d.y_weight).  The weighted form is its own instantiation, so a
// launch without weights runs the code it ran before there were any.
template <bool YW>
__global__ __launch_bounds__(ROM_NT) void rom_kernel(gpi_rom_desc d, RomDims D) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const RomLds o = rom_lds(D);
    float *kp = sm + o.kp, *L = sm + o.L, *u = sm + o.u, *b = sm + o.b, *lam = sm + o.lam, *dinv = sm + o.dinv;
    double *du = (double*)(sm + o.du), *lred = (double*)(sm + o.lred);
    const int s = blockIdx.x;
    const int tid = threadIdx.x, NT = ROM_NT;
    const int nc = D.nc;
    const float* F = d.F + (int64_t)s * D.nn;
    RPHASE(0);

    bool bad = false;
    for (int t = tid; t < D.nT; t += NT) kp[t] = kappa_of(rom_x(d, s, t), d.input_kappa, bad);
    if (bad && d.flag) atomicOr(d.flag, 1);
    for (int e = tid; e < D.nn; e += NT) {
        du[e] = (d.mode == GPI_ROM_BACKWARD && d.duc) ? (double)d.duc[(int64_t)s * D.nn + e] : 0.0;
        lam[e] = 0.f;
    }
    __syncthreads();

    // ---- assemble interior system (banded lower) + rhs
    for (int ii = tid; ii < D.nI; ii += NT) {
        const BandRow row = band_row(nc, ii, F, LdsKappa{kp});
        put_band_row(L + ii * nc, nc, row);
        b[ii] = row.rhs;
    }
    __syncthreads();
    RPHASE(1);
    if (nc == 8 || nc == 4) {
        if (tid == 0) {
            if (nc == 8) { chol_band_seq<8>(L, dinv); solve_band_seq<8>(L, dinv, b); }
            else { chol_band_seq<4>(L, dinv); solve_band_seq<4>(L, dinv, b); }
        }
        __syncthreads();
    } else {
        chol_band(L, D);
        solve_band(L, b, D);
    }
    for (int e = tid; e < D.nn; e += NT) u[e] = u_node(nc, e, F, b);
    __syncthreads();
    RPHASE(2);
    if (d.uc) for (int e = tid; e < D.nn; e += NT) d.uc[(int64_t)s * D.nn + e] = u[e];
    if (d.mode == GPI_ROM_FORWARD && !d.mu_y) return;   // coarse solutions only (VO MC predictive)

    // ---- prolongation (+ log-likelihood, + W^T of the output gradient), by coarse square:
    // four threads share square q = (I, J) and its corner values; each takes every fourth
    // fine free node the square owns (interp()'s partition), loads its Y / logsigma / dmu
    // in batches of ROM_U, and accumulates its W^T contributions to the four corners in
    // registers; one fp64 LDS atomic per corner per square at the end.
    const int nf = D.n, r = D.r;
    const float rinv = 1.f / (float)r;
    float Lsum = 0.f;
    const bool want_g = d.mode == GPI_ROM_LOGLIK || (d.mode == GPI_ROM_BACKWARD && d.dmu);
    for (int qb = 0; qb < nc * nc; qb += NT / 4) {
        const int q = qb + (tid >> 2), sub = tid & 3;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};   // corners v0, v1 (+x), v2 (+y), v3 (+x+y)
        int v0 = 0;
        if (q < nc * nc) {
            const int I = q % nc, J = q / nc;
            v0 = I + (nc + 1) * J;
            const float u0 = u[v0], u1 = u[v0 + 1], u2 = u[v0 + nc + 1], u3 = u[v0 + nc + 2];
            const int i0 = I == 0 ? 1 : I * r, i1 = (I + 1) * r - 1;           // free columns (inclusive)
            const int rows = J == nc - 1 ? r + 1 : r;
            const int ncol = i1 - i0 + 1, total = rows * ncol;
            for (int e0 = sub; e0 < total; e0 += 4 * ROM_U) {
                int pp[ROM_U];
                float yv[ROM_U], lv[ROM_U], gv[ROM_U], wv[YW ? ROM_U : 1];
#pragma unroll
                for (int k = 0; k < ROM_U; ++k) {
                    const int e = min(e0 + 4 * k, total - 1);
                    const int jj = e / ncol, ii = e - jj * ncol;
                    pp[k] = (J * r + jj) * (nf - 1) + (i0 + ii - 1);
                }
                if (d.mode == GPI_ROM_LOGLIK) {
#pragma unroll
                    for (int k = 0; k < ROM_U; ++k) {
                        yv[k] = d.Y[(int64_t)s * D.dy + pp[k]];
                        lv[k] = d.logsig_y[pp[k]];
                        if constexpr (YW) wv[k] = rom_yw(d, s, pp[k]);
                    }
                } else if (want_g) {
#pragma unroll
                    for (int k = 0; k < ROM_U; ++k) gv[k] = d.dmu[(int64_t)s * D.dy + pp[k]];
                }
#pragma unroll
                for (int k = 0; k < ROM_U; ++k) {
                    const int e = e0 + 4 * k;
                    if (e >= total) break;
                    const int jj = e / ncol, ii = e - jj * ncol;
                    const float xi = (float)(i0 + ii - I * r) * rinv, eta = (float)jj * rinv;
                    float w0, w1, w2, w3;
                    if (xi >= eta) { w0 = 1.f - xi; w1 = xi - eta; w2 = 0.f; w3 = eta; }
                    else { w0 = 1.f - eta; w1 = 0.f; w2 = eta - xi; w3 = xi; }
                    const float mu = w0 * u0 + (w1 * u1 + w2 * u2) + w3 * u3;
                    if (d.mu_y) d.mu_y[(int64_t)s * D.dy + pp[k]] = mu;
                    if (!want_g) continue;
                    float g;
                    if (d.mode == GPI_ROM_LOGLIK) {
                        const float ee = expf(-2.f * lv[k]);
                        const float rr = yv[k] - mu;
                        if constexpr (YW) {
                            // an unobserved entry contributes exactly 0, whatever Y holds there (a select: 0 * NaN
                            // would not do); w = 1 leaves every value as the unweighted form computes it.  That form
                            // rounds every product on its own (rr^2 ee feeds two sums, so it is never fused into
                            // either); written here with contraction off, or the compiler fuses these into other bits
#pragma clang fp contract(off)
                            const bool obs = wv[k] != 0.f;
                            const float r2e = rr * rr * ee;
                            const float ll = -0.5f * (2.f * lv[k] + r2e + GPI_LOG2PI);
                            Lsum += obs ? wv[k] * ll : 0.f;
                            g = obs ? wv[k] * (-d.loss_scale * rr * ee) : 0.f;
                            const float gl = obs ? wv[k] * (d.loss_scale * (1.f - r2e)) : 0.f;
                            if (d.gls_part) d.gls_part[(int64_t)s * D.dy + pp[k]] = gl;
                            else if (obs) atomicAdd(d.gacc_logsig + pp[k], (double)gl);
                        } else {
                            Lsum += -0.5f * (2.f * lv[k] + rr * rr * ee + GPI_LOG2PI);
                            g = -d.loss_scale * rr * ee;
                            const float gl = d.loss_scale * (1.f - rr * rr * ee);
                            if (d.gls_part) d.gls_part[(int64_t)s * D.dy + pp[k]] = gl;
                            else atomicAdd(d.gacc_logsig + pp[k], (double)gl);
                        }
                    } else {
                        g = gv[k];
                    }
                    acc[0] += w0 * g;
                    acc[1] += w1 * g;
                    acc[2] += w2 * g;
                    acc[3] += w3 * g;
                }
            }
        }
        if (want_g) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[c] += __shfl_xor(acc[c], 1, 64);
                acc[c] += __shfl_xor(acc[c], 2, 64);
            }
            if (q < nc * nc && sub == 0) {
                atomicAdd(&du[v0], (double)acc[0]);
                atomicAdd(&du[v0 + 1], (double)acc[1]);
                atomicAdd(&du[v0 + nc + 1], (double)acc[2]);
                atomicAdd(&du[v0 + nc + 2], (double)acc[3]);
            }
        }
    }
    if (d.mode == GPI_ROM_LOGLIK) loglik_sum<ROM_NT / 64>(d, Lsum, lred);
    if (d.mode == GPI_ROM_FORWARD) return;
    __syncthreads();
    RPHASE(3);

    // ---- adjoint
    for (int ii = tid; ii < D.nI; ii += NT) b[ii] = (float)du[interior_node(nc, ii)];
    __syncthreads();
    if (nc == 8 || nc == 4) {
        if (tid == 0) {
            if (nc == 8) solve_band_seq<8>(L, dinv, b);
            else solve_band_seq<4>(L, dinv, b);
        }
        __syncthreads();
    } else {
        solve_band(L, b, D);
    }
    RPHASE(4);
    for (int ii = tid; ii < D.nI; ii += NT) lam[interior_node(nc, ii)] = b[ii];
    __syncthreads();
    gx_store<ROM_NT>(d, s, nc, D.nT, lam, u, kp);
    RPHASE(5);
}

// ---------------------------------------------------------------------------------------------
// rom_kernel_fast<NC> (nc = 4 / 8, one 256-thread workgroup per sample): the same result as
// rom_kernel with the sequential chains cut (r03 phase stamps of rom_kernel at C64: Cholesky + solve
// 83 k cycles, adjoint solve 55 k, prolongation 19 k of 162 k; 72.8 us per launch):
//   * wave 0 factors K = L L^T and forms Z = L^{-1} in ONE pass (chol_inv_wave): the factorisation runs
//     redundantly in every lane and lane j takes the forward substitution of e_j as each row of L
//     becomes final; u = K^{-1} b and the adjoint lambda = K^{-1} W^T dmu are then Z^T (Z v) mat-vecs
//     over the four waves (kinv_apply) instead of sequential triangular sweeps;
//   * the Y / logsigma_y loads of the prolongation are issued at entry (in flight during the
//     factorisation);
//   * d/dlogsigma_y per sample and node goes to a row of gls_part (plain stores) when given, reduced
//     with the decoder slabs, instead of 4095 same-address fp64 atomics per sample.
// (r03 A/B: a wave-parallel factorisation with rotating window rows and ds_bpermute took 23.7 k cycles,
// the redundant form 13.9 k; 64 independent register solves with v_readlane coefficients 17.5 k for the
// sweeps vs 3.7 k for the two Z mat-vecs.)  21.3 us per launch at C64.

constexpr int KINV_P = 65;     // pitch of the Z = L^{-1} image (conflict-free row and column access)

// Z = L^{-1} (K = L L^T) by ONE wave: every lane runs the same banded factorisation (chol_band_seq's
// register window, the pivot by v_rsq instead of IEEE sqrt + division; the values are uniform, the band
// rows come by broadcast LDS reads) and, as row k of L becomes final at step k, lane j takes
// forward-substitution step k of L y = e_j -- the factorisation instructions serve all 64 right-hand
// sides at once (SIMT: an instruction costs the same with one lane active or 64), no LDS or cross-lane
// traffic in the substitution.  Column j of Z goes to z[k][j] (pitch KINV_P).  Then
// K^{-1} v = Z^T (Z v): two parallel triangular mat-vecs per solve.
template <int NC>
__device__ __forceinline__ void chol_inv_wave(const float* __restrict__ L, float* __restrict__ z) {
    constexpr int W = NC, BW = NC - 1, NI = (NC - 1) * (NC + 1);
    const int j = threadIdx.x & 63;
    float win[W][W];
    float nxt[2][W];   // rows k + W, k + W + 1 (prefetched)
    win_load<W>(win, L, NI);
    win_row<W>(nxt[0], L, W, NI);
    win_row<W>(nxt[1], L, W + 1, NI);
    float h[BW];       // h[t-1] = y[k - t] of this lane's right-hand side e_j
    h_clear(h);
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const float inv = __builtin_amdgcn_rsqf(win[0][0]);
        // forward substitution step k (row k of L is final: L(k, k - t) = win[0][t], 1 / L(k,k) = inv)
        float y = j == k ? 1.f : 0.f, y2 = 0.f;
#pragma unroll
        for (int t = 1; t <= BW; ++t) {
            if (k - t < 0) continue;
            if (t & 1) y = fmaf(-win[0][t], h[t - 1], y);
            else y2 = fmaf(-win[0][t], h[t - 1], y2);
        }
        y = (y + y2) * inv;
        z[k * KINV_P + j] = y;
        h_push(h, y);
        // factorisation step k
        win_step<W>(win, inv);
        win_shift<W>(win);
#pragma unroll
        for (int t = 0; t < W; ++t) {
            win[W - 1][t] = nxt[0][t];
            nxt[0][t] = nxt[1][t];
            nxt[1][t] = (k + W + 2 < NI) ? L[(k + W + 2) * W + t] : 0.f;
        }
    }
}

// out[i] = (Z^T (Z v))_i = (K^{-1} v)_i for i < NI (v, out in LDS; out may alias v; part: NW x 64 + 64
// floats of scratch).  All NT = 64 NW threads call it: wave p sums the terms k = p (mod NW) of every row
// i = lane (fully unrolled, conflict-free: bank (i + k) mod 64), the NW partial sums meet in LDS (pairwise,
// in a fixed order); three barriers.
template <int NW>
__device__ __forceinline__ float part_sum(const float* part, int i) {
    if constexpr (NW == 4) return (part[i] + part[64 + i]) + (part[128 + i] + part[192 + i]);
    else return part_sum<NW / 2>(part, i) + part_sum<NW / 2>(part + 64 * (NW / 2), i);
}

template <int NC, int NT>
__device__ __forceinline__ void kinv_apply(const float* __restrict__ z, const float* v, float* part, float* out) {
    constexpr int NW = NT / 64, NI = (NC - 1) * (NC + 1), NM = (NI + NW - 1) / NW;
    const int i = threadIdx.x & 63, p = threadIdx.x >> 6;
    float a = 0.f;
#pragma unroll
    for (int m = 0; m < NM; ++m) {            // (Z v)_i = sum_{k <= i} Z[i][k] v_k
        const int k = NW * m + p;
        if (k < NI) a = fmaf((k <= i && i < NI) ? z[i * KINV_P + k] : 0.f, v[k], a);
    }
    part[p * 64 + i] = a;
    __syncthreads();
    float* w = part + 64 * NW;                // (Z v), 64 floats
    if (threadIdx.x < 64) w[i] = part_sum<NW>(part, i);
    __syncthreads();
    a = 0.f;
#pragma unroll
    for (int m = 0; m < NM; ++m) {            // (Z^T w)_i = sum_{k >= i} Z[k][i] w_k
        const int k = NW * m + p;
        if (k < NI) a = fmaf((k >= i && i < NI) ? z[k * KINV_P + i] : 0.f, w[k], a);
    }
    part[p * 64 + i] = a;
    __syncthreads();
    if (threadIdx.x < NI) out[i] = part_sum<NW>(part, i);
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// nc = 16 (NI = 255 unknowns, bandwidth 15): the factorisation and the band sweeps by ONE WAVE, the
// window of the right-looking band Cholesky distributed over its lanes.
//   * chol16_wave: the 16 x 16 window of the trailing matrix lives in circular slots (row i mod 16,
//     column j mod 16), four column slots per lane: lane = 4 (i mod 16) + q holds columns 4 q .. 4 q + 3
//     of row i.  Step k (slot c = k mod 16, static: the steps are 16 template instances): the pivot by
//     v_readlane + v_rsq, column k scaled in place (every lane gets its row's entry by a quad broadcast
//     DPP), the column entries of the lane's four column slots by ds_bpermute, four FMAs, and row
//     k + 16 enters the slots row k leaves.  No LDS round trip and no barrier on the chain.  Column k
//     goes to LDS in both orientations (Lc[k][t] = L(k + t, k), Lr[i][t] = L(i, i - t), slot 0 of
//     either = 1 / L(k,k)) for the sweeps, and step k of the forward substitution of the right-hand
//     side rides along (column k is final).
//   * band_sweep16: forward (L y = b, axpy form over Lc) or backward (L^T x = y, axpy form over Lr)
//     substitution; lane (i mod 16) owns element i of the moving 16-window, so a step is
//     v_readlane, a multiply and one FMA, the band column prefetched from LDS off the chain.
constexpr int R16_NI = 255;
constexpr int R16_LR = (R16_NI + 16) * 16;   // Lr rows k + t of the last steps run past NI (never read)
constexpr int R16_LC = R16_NI * 16;

// LDS written by some lanes of this wave is read by others: order it for the compiler and the hardware
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

struct Chol16 {
    float s[4];   // slots (ri, 4 q + m)
    float bw;     // right-hand side entry of row slot ri (the same in the quad's four lanes)
    int bp[4];    // ds_bpermute byte address of a lane of row slot 4 q + m
    int lane, ri, q;
};

// the system's rows: diagonal, first sub-diagonal, 15th sub-diagonal at dg[i * as], o1[i * as], o15[i * as]
struct Band16 {
    const float *dg, *o1, *o15;
    int as;
};

template <int C>
__device__ __forceinline__ void chol16_step(Chol16& w, int k, const Band16& A, float* __restrict__ Lr,
                                            float* __restrict__ Lc, float* b) {
    if (k >= R16_NI) return;
    // row k + 16 (identity past the end), read ahead of the chain
    const bool has = k + 16 < R16_NI;
    const int kn = has ? k + 16 : k;
    float dg = A.dg[kn * A.as], o1 = A.o1[kn * A.as], o15 = A.o15[kn * A.as], bn = b[kn];
    dg = has ? dg : 1.f;
    o1 = has ? o1 : 0.f;
    o15 = has ? o15 : 0.f;
    bn = has ? bn : 0.f;
    const float piv = readlane_f(w.s[C & 3], 4 * C + (C >> 2));
    const float inv = __builtin_amdgcn_rsqf(piv);
    // this lane's row entry of column k: slot (ri, C) is register C & 3 of the quad's lane C >> 2
    const float xc = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(w.s[C & 3]), (C >> 2) * 0x55, 0xf, 0xf, false));
    const float li = xc * inv;                      // L(i, k) of this lane's row (row k itself: L(k,k))
    float l[4];                                     // L(j, k) of this lane's four column slots
#pragma unroll
    for (int m = 0; m < 4; ++m) l[m] = __int_as_float(__builtin_amdgcn_ds_bpermute(w.bp[m], __float_as_int(li)));
    const float yk = readlane_f(w.bw, 4 * C) * inv; // forward substitution step k
    w.bw = fmaf(-li, yk, w.bw);
    const int t = (w.ri - C) & 15;                  // this lane's row is k + t
    const float val = t == 0 ? inv : li;
    if (w.q == 0) {
        Lr[(k + t) * 16 + t] = val;
        if (Lc) Lc[k * 16 + t] = val;
    }
    if (w.lane == 0) b[k] = yk;
    const bool inq = w.ri == C;                     // row k leaves, row k + 16 enters its slots
#pragma unroll
    for (int m = 0; m < 4; ++m) w.s[m] = inq ? 0.f : fmaf(-li, l[m], w.s[m]);
    constexpr int C1 = (C + 15) & 15, C15 = (C + 1) & 15;   // column slots of k + 15 and k + 1
    if (w.lane == 4 * C + (C >> 2)) w.s[C & 3] = dg;
    if (w.lane == 4 * C + (C1 >> 2)) w.s[C1 & 3] = o1;
    if (w.lane == 4 * C + (C15 >> 2)) w.s[C15 & 3] = o15;
    w.bw = inq ? bn : w.bw;
}

// K = L L^T of the 255 x 255 band system A and y = L^{-1} b (in place of b), by the calling wave.
// Lc may be null (no forward sweep will follow).
__device__ __forceinline__ void chol16_wave(const Band16& A, float* __restrict__ Lr, float* __restrict__ Lc, float* b) {
    Chol16 w;
    w.lane = threadIdx.x & 63;
    w.ri = w.lane >> 2;
    w.q = w.lane & 3;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = 4 * w.q + m, t = w.ri - j;
        w.bp[m] = 4 * (4 * j);
        float v = 0.f;
        if (t == 0) v = A.dg[w.ri * A.as];
        if (t == 1) v = A.o1[w.ri * A.as];
        if (t == 15) v = A.o15[w.ri * A.as];
        w.s[m] = v;
    }
    w.bw = b[w.ri];
    for (int k0 = 0; k0 < R16_NI; k0 += 16) {
        chol16_step<0>(w, k0 + 0, A, Lr, Lc, b);
        chol16_step<1>(w, k0 + 1, A, Lr, Lc, b);
        chol16_step<2>(w, k0 + 2, A, Lr, Lc, b);
        chol16_step<3>(w, k0 + 3, A, Lr, Lc, b);
        chol16_step<4>(w, k0 + 4, A, Lr, Lc, b);
        chol16_step<5>(w, k0 + 5, A, Lr, Lc, b);
        chol16_step<6>(w, k0 + 6, A, Lr, Lc, b);
        chol16_step<7>(w, k0 + 7, A, Lr, Lc, b);
        chol16_step<8>(w, k0 + 8, A, Lr, Lc, b);
        chol16_step<9>(w, k0 + 9, A, Lr, Lc, b);
        chol16_step<10>(w, k0 + 10, A, Lr, Lc, b);
        chol16_step<11>(w, k0 + 11, A, Lr, Lc, b);
        chol16_step<12>(w, k0 + 12, A, Lr, Lc, b);
        chol16_step<13>(w, k0 + 13, A, Lr, Lc, b);
        chol16_step<14>(w, k0 + 14, A, Lr, Lc, b);
        chol16_step<15>(w, k0 + 15, A, Lr, Lc, b);
    }
    wave_sync();
}

// FWD: b <- L^{-1} b over Lc; else b <- L^{-T} b over Lr.  By the calling wave (its four rows of 16
// lanes run the same sweep; lane k mod 16 of row 0 stores).
template <bool FWD>
__device__ __forceinline__ void band_sweep16(const float* __restrict__ Lb, float* b) {
    const int lane = threadIdx.x & 63, l16 = lane & 15;
    float w = b[FWD ? l16 : (R16_NI - 1) - ((R16_NI - 1 - l16) & 15)];
#pragma unroll 4
    for (int n = 0; n < R16_NI; ++n) {
        const int k = FWD ? n : R16_NI - 1 - n;
        const int t = (FWD ? l16 - k : k - l16) & 15;       // this lane's element is k + t (FWD) / k - t
        const float lv = Lb[k * 16 + t], inv = Lb[k * 16];
        const int kn = FWD ? k + 16 : k - 16;
        const bool has = FWD ? kn < R16_NI : kn >= 0;
        const float bn = b[has ? kn : k];
        const float xk = readlane_f(w, k & 15) * inv;
        w = fmaf(-lv, xk, w);
        if (t == 0) w = has ? bn : 0.f;
        if (lane == (k & 15)) b[k] = xk;
    }
    wave_sync();
}

// NT threads per sample (256 / 512 / 1024): SUB = NT / 64 threads share one coarse square of the
// prolongation (nc = 8: 64 squares; nc = 4 uses 16 of them), so a wider workgroup has more waves in flight
// over the 4095 fine nodes; the factorisation stays in wave 0.
template <int NC, int NT>
struct RomFastLds {   // float offsets; the fp64 block (du [NN], lred [NW]) at the even offset DU
    static constexpr int W = NC, NI = (NC - 1) * (NC + 1), NN = (NC + 1) * (NC + 1), NT2 = 2 * NC * NC, NW = NT / 64;
    static constexpr int FACTOR = NC == 16 ? R16_LR + R16_LC : NI * KINV_P;   // Lr, Lc of chol16_wave / Z = L^{-1}
    // (DINV: NI floats no kernel reads any more, kept so that the size and every offset stay what they were)
    static constexpr int KP = 0, L = KP + NT2, U = L + NI * W, B = U + NN, LAM = B + NI, DINV = LAM + NN,
                         KINV = DINV + NI, PART = KINV + FACTOR, DU = (PART + 64 * NW + 64 + 1) & ~1;
    static constexpr size_t bytes = sizeof(float) * DU + sizeof(double) * (NN + NW);
};

// YW: the launch has observation weights; they join the prefetched Y / logsigma_y operands (rom_kernel's note).
template <int NC, int NT, bool YW>
__global__ __launch_bounds__(NT) void rom_kernel_fast(gpi_rom_desc d, RomDims D) {
    using S = RomFastLds<NC, NT>;
    constexpr int NI = S::NI, NN = S::NN, NT2 = S::NT2, SUB = NT / 64, NW = S::NW;
    constexpr int PF = (SUB >= 8 ? 1 : 3) * ROM_U;   // prefetched fine nodes per thread (a square holds <= (r+1) r)
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* kp = sm + S::KP;           // [NT2] kappa
    float* L = sm + S::L;             // [NI * W]
    float* u = sm + S::U;             // [NN]
    float* b = sm + S::B;             // [NI]
    float* lam = sm + S::LAM;         // [NN]
    float* kinv = sm + S::KINV;       // [NI][KINV_P]: Z = L^{-1} (NC = 16: Lr, then Lc of chol16_wave)
    float* part = sm + S::PART;       // [64 NW + 64] kinv_apply scratch
    double* du = (double*)(sm + S::DU);   // [NN]
    double* lred = du + NN;           // [NW]
    const int s = blockIdx.x;
    const int tid = threadIdx.x;
    const float* F = d.F + (int64_t)s * NN;
    const int nf = D.n, r = D.r;
    RPHASE(0);

    // ---- entry: every global read in flight (kappa, F, and this thread's first PF fine nodes)
    const int q0 = tid / SUB, sub = tid & (SUB - 1);
    float ypf[PF], lpf[PF], wpf[YW ? PF : 1];
    {
        const bool okq = q0 < NC * NC && d.mode == GPI_ROM_LOGLIK;
        const int I = q0 % NC, J = q0 / NC;
        const int i0 = I == 0 ? 1 : I * r, i1 = (I + 1) * r - 1;
        const int rows = J == NC - 1 ? r + 1 : r;
        const int ncol = i1 - i0 + 1, total = rows * ncol;
        const uint32_t mcol = (ncol > 1 ? (uint32_t)(((1ull << 32) + ncol - 1) / ncol) : 0u);   // e / ncol = umulhi(e, mcol), e < 2^16
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int e = sub + SUB * k;
            const bool ok = okq && e < total;
            const int jj = ok ? (mcol ? (int)__umulhi((uint32_t)e, mcol) : e) : 0, ii = ok ? e - jj * ncol : 0;
            const int pp = (J * r + jj) * (nf - 1) + (i0 + ii - 1);
            ypf[k] = ok ? d.Y[(int64_t)s * D.dy + pp] : 0.f;
            lpf[k] = ok ? d.logsig_y[pp] : 0.f;
            if constexpr (YW) wpf[k] = ok ? rom_yw(d, s, pp) : 0.f;
        }
    }
    bool bad = false;
    for (int t = tid; t < NT2; t += NT) kp[t] = kappa_of(rom_x(d, s, t), d.input_kappa, bad);
    if (bad && d.flag) atomicOr(d.flag, 1);
    for (int e = tid; e < NN; e += NT) {
        du[e] = (d.mode == GPI_ROM_BACKWARD && d.duc) ? (double)d.duc[(int64_t)s * NN + e] : 0.0;
        lam[e] = 0.f;
    }
    __syncthreads();
    // ---- assemble the interior system (banded lower) + rhs
    for (int ii = tid; ii < NI; ii += NT) {
        const BandRow row = band_row(NC, ii, F, LdsKappa{kp});
        put_band_row(L + ii * NC, NC, row);
        b[ii] = row.rhs;
    }
    __syncthreads();
    RPHASE(1);
    // the prefetched Y / logsigma_y values in registers from here on (issued at entry, they arrived with
    // kappa and F): otherwise the compiler sinks the loads to the prolongation, a round trip there
#pragma unroll
    for (int k = 0; k < PF; ++k) asm volatile("" : : "v"(ypf[k]), "v"(lpf[k]));
    if constexpr (YW) {
#pragma unroll
        for (int k = 0; k < PF; ++k) asm volatile("" : : "v"(wpf[k]));
    }
    if constexpr (NC == 16) {
        // wave 0: band factorisation with the forward substitution of b riding along, then the back sweep
        if (tid < 64) {
            const Band16 A = {L, L + 1, L + NC - 1, NC};
            chol16_wave(A, kinv, kinv + R16_LR, b);
            RPHASE(6);
            band_sweep16<false>(kinv, b);
        }
        __syncthreads();
    } else {
        static_assert(NC * NC <= 64, "window per wave");
        // every lane of wave 0: the factorisation (uniform) + forward substitution of e_lane -> Z = L^{-1}
        if (tid < 64) chol_inv_wave<NC>(L, kinv);
        RPHASE(6);
        __syncthreads();
        // interior coarse solution u_I = K^{-1} b = Z^T (Z b), in place of b
        kinv_apply<NC, NT>(kinv, b, part, b);
    }
    RPHASE(2);
    for (int e = tid; e < NN; e += NT) u[e] = u_node(NC, e, F, b);
    __syncthreads();
    if (d.uc) for (int e = tid; e < NN; e += NT) d.uc[(int64_t)s * NN + e] = u[e];

    // ---- prolongation (+ log-likelihood, + W^T of the output gradient), rom_kernel's loop with SUB threads per
    // coarse square, e / ncol by umulhi (exact for e < 2^16, which these shapes guarantee), and the first
    // PF nodes of every thread's square from the entry prefetch
    const float rinv = 1.f / (float)r;
    float Lsum = 0.f;
    const bool want_g = d.mode == GPI_ROM_LOGLIK || (d.mode == GPI_ROM_BACKWARD && d.dmu);
    for (int qb = 0; qb < NC * NC; qb += NT / SUB) {
        const int q = qb + q0;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int v0 = 0;
        if (q < NC * NC) {
            const int I = q % NC, J = q / NC;
            v0 = I + (NC + 1) * J;
            const float u0 = u[v0], u1 = u[v0 + 1], u2 = u[v0 + NC + 1], u3 = u[v0 + NC + 2];
            const int i0 = I == 0 ? 1 : I * r, i1 = (I + 1) * r - 1;
            const int rows = J == NC - 1 ? r + 1 : r;
            const int ncol = i1 - i0 + 1, total = rows * ncol;
            const uint32_t mcol = (ncol > 1 ? (uint32_t)(((1ull << 32) + ncol - 1) / ncol) : 0u);
            for (int e0 = sub; e0 < total; e0 += SUB * ROM_U) {
                const int bi = (e0 - sub) / (SUB * ROM_U);
                const bool pre = qb == 0 && bi < PF / ROM_U;
                int pp[ROM_U];
                float yv[ROM_U], lv[ROM_U], gv[ROM_U], wv[YW ? ROM_U : 1];
#pragma unroll
                for (int k = 0; k < ROM_U; ++k) {
                    const int e = min(e0 + SUB * k, total - 1);
                    const int jj = (mcol ? (int)__umulhi((uint32_t)e, mcol) : e), ii = e - jj * ncol;
                    pp[k] = (J * r + jj) * (nf - 1) + (i0 + ii - 1);
                }
                if (d.mode == GPI_ROM_LOGLIK) {
                    if (pre) {
#pragma unroll
                        for (int k = 0; k < ROM_U; ++k) {
                            if constexpr (PF == ROM_U) {
                                yv[k] = ypf[k];
                                lv[k] = lpf[k];
                                if constexpr (YW) wv[k] = wpf[k];
                            } else {
                                yv[k] = bi == 0 ? ypf[k] : (bi == 1 ? ypf[ROM_U + k] : ypf[2 * ROM_U + k]);
                                lv[k] = bi == 0 ? lpf[k] : (bi == 1 ? lpf[ROM_U + k] : lpf[2 * ROM_U + k]);
                                if constexpr (YW) wv[k] = bi == 0 ? wpf[k] : (bi == 1 ? wpf[ROM_U + k] : wpf[2 * ROM_U + k]);
                            }
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < ROM_U; ++k) {
                            yv[k] = d.Y[(int64_t)s * D.dy + pp[k]];
                            lv[k] = d.logsig_y[pp[k]];
                            if constexpr (YW) wv[k] = rom_yw(d, s, pp[k]);
                        }
                    }
                } else if (want_g) {
#pragma unroll
                    for (int k = 0; k < ROM_U; ++k) gv[k] = d.dmu[(int64_t)s * D.dy + pp[k]];
                }
#pragma unroll
                for (int k = 0; k < ROM_U; ++k) {
                    const int e = e0 + SUB * k;
                    if (e >= total) break;
                    const int jj = (mcol ? (int)__umulhi((uint32_t)e, mcol) : e), ii = e - jj * ncol;
                    const float xi = (float)(i0 + ii - I * r) * rinv, eta = (float)jj * rinv;
                    float w0, w1, w2, w3;
                    if (xi >= eta) { w0 = 1.f - xi; w1 = xi - eta; w2 = 0.f; w3 = eta; }
                    else { w0 = 1.f - eta; w1 = 0.f; w2 = eta - xi; w3 = xi; }
                    const float mu = w0 * u0 + (w1 * u1 + w2 * u2) + w3 * u3;
                    if (d.mu_y) d.mu_y[(int64_t)s * D.dy + pp[k]] = mu;
                    if (!want_g) continue;
                    float g;
                    if (d.mode == GPI_ROM_LOGLIK) {
                        const float ee = expf(-2.f * lv[k]);
                        const float rr = yv[k] - mu;
                        if constexpr (YW) {
                            // an unobserved entry contributes exactly 0, whatever Y holds there (a select: 0 * NaN
                            // would not do); w = 1 leaves every value as the unweighted form computes it.  That form
                            // rounds every product on its own (rr^2 ee feeds two sums, so it is never fused into
                            // either); written here with contraction off, or the compiler fuses these into other bits
#pragma clang fp contract(off)
                            const bool obs = wv[k] != 0.f;
                            const float r2e = rr * rr * ee;
                            const float ll = -0.5f * (2.f * lv[k] + r2e + GPI_LOG2PI);
                            Lsum += obs ? wv[k] * ll : 0.f;
                            g = obs ? wv[k] * (-d.loss_scale * rr * ee) : 0.f;
                            const float gl = obs ? wv[k] * (d.loss_scale * (1.f - r2e)) : 0.f;
                            if (d.gls_part) d.gls_part[(int64_t)s * D.dy + pp[k]] = gl;
                            else if (obs) atomicAdd(d.gacc_logsig + pp[k], (double)gl);
                        } else {
                            Lsum += -0.5f * (2.f * lv[k] + rr * rr * ee + GPI_LOG2PI);
                            g = -d.loss_scale * rr * ee;
                            const float gl = d.loss_scale * (1.f - rr * rr * ee);
                            if (d.gls_part) d.gls_part[(int64_t)s * D.dy + pp[k]] = gl;
                            else atomicAdd(d.gacc_logsig + pp[k], (double)gl);
                        }
                    } else {
                        g = gv[k];
                    }
                    acc[0] += w0 * g;
                    acc[1] += w1 * g;
                    acc[2] += w2 * g;
                    acc[3] += w3 * g;
                }
            }
        }
        if (want_g) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int o = 1; o < SUB; o <<= 1) acc[c] += __shfl_xor(acc[c], o, 64);
            if (q < NC * NC && sub == 0) {
                atomicAdd(&du[v0], (double)acc[0]);
                atomicAdd(&du[v0 + 1], (double)acc[1]);
                atomicAdd(&du[v0 + NC + 1], (double)acc[2]);
                atomicAdd(&du[v0 + NC + 2], (double)acc[3]);
            }
        }
    }
    RPHASE(7);
    if (d.mode == GPI_ROM_LOGLIK) loglik_sum<NW>(d, Lsum, lred);
    if (d.mode == GPI_ROM_FORWARD) return;
    __syncthreads();
    RPHASE(3);
    // ---- adjoint lambda = K^{-1} (W^T dmu)_interior = Z^T (Z r)
    for (int ii = tid; ii < NI; ii += NT) b[ii] = (float)du[interior_node(NC, ii)];
    __syncthreads();
    if constexpr (NC == 16) {
        if (tid < 64) {
            band_sweep16<true>(kinv + R16_LR, b);
            band_sweep16<false>(kinv, b);
        }
        __syncthreads();
    } else {
        kinv_apply<NC, NT>(kinv, b, part, b);
    }
    for (int ii = tid; ii < NI; ii += NT) lam[interior_node(NC, ii)] = b[ii];
    __syncthreads();
    RPHASE(4);
    gx_store<NT>(d, s, NC, NT2, lam, u, kp);
    RPHASE(5);
}

// Coarse solutions only at nc = 16: ONE WAVE PER SAMPLE, R16C_SPW samples per workgroup (the waves never
// talk: no workgroup barrier, so the waves past n of a ragged last workgroup simply leave).  Each wave
// assembles its system as three diagonals, factors it with the forward substitution riding along
// (chol16_wave, no Lc: no forward sweep follows) and runs the one back sweep.
constexpr int R16C_SPW = 2;
struct Rom16CoarseLds {   // float offsets within a wave's block
    static constexpr int KP = 0, DG = KP + 512, O1 = DG + 256, O15 = O1 + 256, B = O15 + 256, LR = B + 256,
                         FLOATS = LR + R16_LR;
    static constexpr size_t bytes = sizeof(float) * R16C_SPW * FLOATS;
};

__global__ __launch_bounds__(64 * R16C_SPW) void rom16_coarse_kernel(gpi_rom_desc d) {
    using S = Rom16CoarseLds;
    constexpr int NC = 16, NN = 289, NT2 = 512;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * R16C_SPW + (threadIdx.x >> 6);
    if (s >= d.n) return;
    float* base = sm + (threadIdx.x >> 6) * S::FLOATS;          // this wave's block
    float* kp = base + S::KP;                                   // [512] kappa
    float* dg = base + S::DG;                                   // [256] each: diagonal, sub-diagonals, rhs
    float* o1 = base + S::O1;
    float* o15 = base + S::O15;
    float* b = base + S::B;
    float* Lr = base + S::LR;                                   // [R16_LR]
    const float* __restrict__ F = d.F + (int64_t)s * NN;
    bool bad = false;
#pragma unroll
    for (int t = lane; t < NT2; t += 64) kp[t] = kappa_of(rom_x(d, s, t), d.input_kappa, bad);
    if (bad && d.flag) atomicOr(d.flag, 1);
    wave_sync();
#pragma unroll
    for (int ii = lane; ii < R16_NI; ii += 64) {
        const BandRow row = band_row(NC, ii, F, LdsKappa{kp});
        dg[ii] = row.dg;
        o1[ii] = row.o1;
        o15[ii] = row.on;
        b[ii] = row.rhs;
    }
    wave_sync();
    const Band16 A = {dg, o1, o15, 1};
    chol16_wave(A, Lr, nullptr, b);
    band_sweep16<false>(Lr, b);
    float* uc = d.uc + (int64_t)s * NN;
    for (int e = lane; e < NN; e += 64) uc[e] = u_node(NC, e, F, b);
}

// Coarse solutions only (FORWARD without mu_y: the VO MC predictive, N_vo x N_mc samples), nc = 4 / 8:
// ONE LANE PER SAMPLE.  rom_kernel runs the banded Cholesky in one lane of a 256-thread workgroup per
// sample; here every lane of a wave64 factors its own sample's system with the same register window
// (chol_band_seq), the forward substitution fused into the factorisation (row k of L is final when the window
// reaches it) and the band rows / right-hand side in LDS interleaved by lane ([entry][64]: conflict-free).
// Slot 0 of each stored L row holds 1 / L(k,k).  This kernel keeps its own statement of the band row, the window
// step and the back substitution: its 63 fully unrolled steps compile to other code, and a measurably slower
// solve, through every form of the shared helpers that was tried (profiles/rom_refactor_isa.txt).
template <int NC>
struct RomLaneLds {   // float offsets
    static constexpr int W = NC, NI = (NC - 1) * (NC + 1);
    static constexpr int LS = 0, BS = LS + NI * W * 64;          // [NI * W][64], [NI][64]
    static constexpr size_t bytes = sizeof(float) * (BS + NI * 64);
};

template <int NC>
__global__ __launch_bounds__(64) void rom_lane_kernel(gpi_rom_desc d) {
    constexpr int W = NC, BW = NC - 1, NI = (NC - 1) * (NC + 1), NN = (NC + 1) * (NC + 1);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ls = sm + RomLaneLds<NC>::LS;  // [NI * W][64]
    float* Bs = sm + RomLaneLds<NC>::BS;  // [NI][64]
    const int lane = threadIdx.x;
    const int s = blockIdx.x * 64 + lane;
    const bool act = s < d.n;
    const int sc = act ? s : 0;
    const float* __restrict__ F = d.F + (int64_t)sc * NN;
    auto kap = [&](int I, int J, int ul) -> float {
        const float v = rom_x(d, sc, 2 * (I + NC * J) + ul);
        return d.input_kappa ? v : expf(v) + 1e-8f;
    };
    auto ch = [&](int I, int J) -> float {        // horizontal edge (I,J)-(I+1,J)
        float c = 0.f;
        if (J < NC) c += kap(I, J, 0);
        if (J > 0) c += kap(I, J - 1, 1);
        return 0.5f * c;
    };
    auto cv = [&](int I, int J) -> float {        // vertical edge (I,J)-(I,J+1)
        float c = 0.f;
        if (I > 0) c += kap(I - 1, J, 0);
        if (I < NC) c += kap(I, J, 1);
        return 0.5f * c;
    };
    bool bad = false;
#pragma unroll
    for (int t = 0; t < 2 * NC * NC; ++t) {
        const float v = rom_x(d, sc, t);
        bad |= !((d.input_kappa ? v : expf(v) + 1e-8f) > 1e-12f);
    }
    if (act && bad && d.flag) atomicOr(d.flag, 1);
    // ---- assemble the interior rows (banded lower) + rhs
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int J = k / (NC - 1), I = k - J * (NC - 1) + 1, p = I + (NC + 1) * J;
        const float chl = ch(I - 1, J), chr = ch(I, J);
        const float cvd = J > 0 ? cv(I, J - 1) : 0.f, cvu = J < NC ? cv(I, J) : 0.f;
#pragma unroll
        for (int t = 0; t < W; ++t) {
            float v = 0.f;
            if (t == 0) v = chl + chr + cvd + cvu;
            if (t == 1 && I - 1 >= 1) v += -chl;
            if (t == BW && J >= 1) v += -cvd;
            Ls[(k * W + t) * 64 + lane] = v;
        }
        float rhs = F[p];
        if (I - 1 == 0) rhs += chl * F[p - 1];
        if (I + 1 == NC) rhs += chr * F[p + 1];
        Bs[k * 64 + lane] = rhs;
    }
    // ---- factorisation + forward substitution (register window, see chol_band_seq)
    float win[W][W];   // win[a][t] = L(k + a, k + a - t)
    float h[BW];       // h[t-1] = y[k - t]
#pragma unroll
    for (int a = 0; a < W; ++a)
#pragma unroll
        for (int t = 0; t < W; ++t) win[a][t] = a < NI ? Ls[(a * W + t) * 64 + lane] : 0.f;
#pragma unroll
    for (int t = 0; t < BW; ++t) h[t] = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const float dk = sqrtf(win[0][0]);
        const float inv = 1.f / dk;
#pragma unroll
        for (int a = 1; a < W; ++a) win[a][a] *= inv;                       // L(k+a, k)
#pragma unroll
        for (int a = 1; a < W; ++a)
#pragma unroll
            for (int b = 1; b <= a; ++b) win[a][a - b] = fmaf(-win[a][a], win[b][b], win[a][a - b]);
        float y = Bs[k * 64 + lane];
#pragma unroll
        for (int t = 1; t <= BW; ++t)
            if (k - t >= 0) y = fmaf(-win[0][t], h[t - 1], y);
        y *= inv;
        Bs[k * 64 + lane] = y;
#pragma unroll
        for (int t = BW - 1; t > 0; --t) h[t] = h[t - 1];
        h[0] = y;
        Ls[(k * W) * 64 + lane] = inv;
#pragma unroll
        for (int t = 1; t < W; ++t) Ls[(k * W + t) * 64 + lane] = win[0][t];
#pragma unroll
        for (int a = 0; a + 1 < W; ++a)
#pragma unroll
            for (int t = 0; t < W; ++t) win[a][t] = win[a + 1][t];
#pragma unroll
        for (int t = 0; t < W; ++t) win[W - 1][t] = (k + W < NI) ? Ls[((k + W) * W + t) * 64 + lane] : 0.f;
    }
    // ---- back substitution L^T x = y
#pragma unroll
    for (int t = 0; t < BW; ++t) h[t] = 0.f;        // h[t-1] = x[k + t]
#pragma unroll
    for (int k = NI - 1; k >= 0; --k) {
        float a = Bs[k * 64 + lane];
#pragma unroll
        for (int t = 1; t <= BW; ++t)
            if (k + t < NI) a = fmaf(-Ls[((k + t) * W + t) * 64 + lane], h[t - 1], a);
        a *= Ls[(k * W) * 64 + lane];
        Bs[k * 64 + lane] = a;
#pragma unroll
        for (int t = BW - 1; t > 0; --t) h[t] = h[t - 1];
        h[0] = a;
    }
    if (!act) return;
    float* uc = d.uc + (int64_t)s * NN;
#pragma unroll
    for (int e = 0; e < NN; ++e) {
        const int I = e % (NC + 1), J = e / (NC + 1);
        uc[e] = (I == 0 || I == NC) ? F[e] : Bs[(J * (NC - 1) + (I - 1)) * 64 + lane];
    }
}

// ---------------------------------------------------------------------------------------------
// rom_fit_kernel<NC> (gpi_rom_fit; nc = 4 / 8 / 16): ONE WAVE64 PER SAMPLE runs every Adam iteration of
// OptimizeEffectiveProperties (bottleneck/utils.py:250-282) in one launch.  Row n of the gradient
// depends on row n alone (the MSE mean's 1 / (n_total d_y) is a constant), so the workgroups never talk.
//   setup      one pass over Y_n: a lane owns the coarse squares q = lane + 64 k (in that order: c_n's partial
//              is one chain per lane; interp()'s partition of the fine free nodes) and sums, in fp64 and in a
//              fixed order, its nodes' shares of b_n = W^T Y_n, c_n = |Y_n|^2 and G = W^T W (fit_square_sums;
//              per square: 4 diagonal and 5 edge entries -- the "/" triangles never couple a square's +x and
//              +y corners, hence <= 7 non-zeros per row); the squares' shares meet per coarse node in LDS
//              (fit_node_gather, fixed order: no atomics).  They are staged over the solver's factor storage,
//              which is free until the first iteration.
//   iteration  kappa = exp(x) + 1e-8 -> band_row -> the solver's factorisation and u = K^{-1} rhs ->
//              fp64: G u (fit_gu_row), ss = u^T (G u - 2 b) + c, g_u = gscale (G u - b) -> lambda = K^{-1} g_u
//              -> dJ/dx by dk_edge -> adam_element on the lane's x, m, v (fit_update).
// x, m, v live in registers (triangle t = lane + 64 k); an iteration touches coarse quantities only, its
// cost does not depend on the refinement.  No cross-workgroup traffic, no waits.
// The solver (FitSolverZ at nc = 4 / 8, FitSolver16 at nc = 16) brings its scratch layout, the storage the
// row assembly writes to, the two solves and its synchronisation primitive: the workgroup is one wave, and
// every LDS hand-off between lanes is followed by the solver's sync().

// out = Z^T (Z v) = K^{-1} v for one wave (kinv_apply's two triangular mat-vecs without the split over
// waves): lane i owns row i; v (in / out) and w are 64-float LDS vectors.  Four partial sums in a fixed
// order.  Ends with a barrier.
template <int NC>
__device__ __forceinline__ void kinv_apply_wave(const float* __restrict__ z, float* v, float* w) {
    constexpr int NI = (NC - 1) * (NC + 1);
    const int i = threadIdx.x, ic = i < NI ? i : NI - 1;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NI; ++k)              // (Z v)_i = sum_{k <= i} Z[i][k] v_k
        a[k & 3] = fmaf(k <= i ? z[ic * KINV_P + k] : 0.f, v[k], a[k & 3]);
    w[i] = i < NI ? (a[0] + a[1]) + (a[2] + a[3]) : 0.f;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k)              // (Z^T w)_i = sum_{k >= i} Z[k][i] w_k
        a[k & 3] = fmaf(k >= i ? z[k * KINV_P + i] : 0.f, w[k], a[k & 3]);
    if (i < NI) v[i] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
}

// nc = 4 / 8: Z = L^{-1} by chol_inv_wave, the solves by kinv_apply_wave; workgroup barriers.
template <int NC>
struct FitSolverZ {   // float offsets of its scratch (every block a multiple of 4 floats)
    static constexpr int W = NC, NI = (NC - 1) * (NC + 1);
    static constexpr int L = 0, BV = L + ((NI * W + 3) & ~3), WV = BV + 64, Z = WV + 64,
                         FLOATS = Z + ((NI * KINV_P + 3) & ~3);
    static constexpr int STAGE = Z, STAGE_FLOATS = NI * KINV_P;   // free before the first factorisation
    float* m;
    __device__ __forceinline__ static void sync() { __syncthreads(); }
    __device__ __forceinline__ float* b() const { return m + BV; }   // [64] right-hand side / solution
    __device__ __forceinline__ void assemble(const float* kp, const float* Fs) const {
        const int ii = threadIdx.x;
        if (ii < NI) {
            const BandRow row = band_row(NC, ii, Fs, LdsKappa{kp});
            put_band_row(m + L + ii * W, W, row);
            m[BV + ii] = row.rhs;
        }
    }
    __device__ __forceinline__ void solve_primal() const {
        chol_inv_wave<NC>(m + L, m + Z);
        __syncthreads();
        kinv_apply_wave<NC>(m + Z, m + BV, m + WV);
    }
    __device__ __forceinline__ void solve_adjoint() const { kinv_apply_wave<NC>(m + Z, m + BV, m + WV); }
};
// nc = 16: 255 unknowns have no Z = L^{-1} image: the three diagonals -> chol16_wave (forward substitution
// riding along) -> back sweep; the adjoint by a forward sweep over Lc and a back sweep over Lr; wave_sync.
struct FitSolver16 {
    static constexpr int DG = 0, O1 = DG + 256, O15 = O1 + 256, B = O15 + 256, LR = B + 256, LC = LR + R16_LR,
                         FLOATS = LC + R16_LC;
    static constexpr int STAGE = LR, STAGE_FLOATS = R16_LR + R16_LC;
    float* m;
    __device__ __forceinline__ static void sync() { wave_sync(); }
    __device__ __forceinline__ float* b() const { return m + B; }
    __device__ __forceinline__ void assemble(const float* kp, const float* Fs) const {
#pragma unroll
        for (int ii = threadIdx.x; ii < R16_NI; ii += 64) {
            const BandRow row = band_row(16, ii, Fs, LdsKappa{kp});
            m[DG + ii] = row.dg;
            m[O1 + ii] = row.o1;
            m[O15 + ii] = row.on;
            m[B + ii] = row.rhs;
        }
    }
    __device__ __forceinline__ void solve_primal() const {
        const Band16 A = {m + DG, m + O1, m + O15, 1};
        chol16_wave(A, m + LR, m + LC, m + B);
        band_sweep16<false>(m + LR, m + B);
    }
    __device__ __forceinline__ void solve_adjoint() const {
        band_sweep16<true>(m + LC, m + B);
        band_sweep16<false>(m + LR, m + B);
    }
};

template <int NC>
struct RomFitLds {   // float offsets after the fp64 block (every block a multiple of 4 floats)
    using Solver = std::conditional_t<NC == 16, FitSolver16, FitSolverZ<NC>>;
    static constexpr int NN = (NC + 1) * (NC + 1), NT2 = 2 * NC * NC, NNP = (NN + 3) & ~3;
    static constexpr int ND = 5 * NN + (NN & 1);                 // doubles: G [4][NN], b [NN]
    static constexpr int KP = 0, U = KP + NT2, LAM = U + NNP, FS = LAM + NNP, SOLVER = FS + NNP,
                         END = SOLVER + Solver::FLOATS;
    static constexpr size_t bytes = sizeof(double) * ND + sizeof(float) * END;
    static_assert(sizeof(double) * 13 * NC * NC <= sizeof(float) * Solver::STAGE_FLOATS, "setup partials fit in the factor");
    static_assert((SOLVER + Solver::STAGE) % 2 == 0, "the fp64 staging area is 8-byte aligned");
    static_assert(bytes <= 64 * 1024, "within the default dynamic-LDS limit");
};

// Setup, square q: the fp64 sums over its fine free nodes (Y: the sample's row) of W^T Y (4 corners), W^T W
// (9 entries: 00 11 22 33 01 02 03 13 23) into sq[13], and of |Y|^2 onto cc.
// Yw: the sample's row of observation weights, or null.  An entry with weight 0 is never read into a sum
// (y by a select); weight 1 multiplies exactly, so all-ones weights give the bits of a setup without weights.
__device__ __forceinline__ void fit_square_sums(int nc, int r, int q, const float* Y, const float* Yw, double& cc,
                                                double* sq) {
    const int nf = nc * r;
    const int I = q % nc, J = q / nc;
    const int i0 = I == 0 ? 1 : I * r, i1 = (I + 1) * r - 1;     // free columns (inclusive)
    const int rows = J == nc - 1 ? r + 1 : r;
    const double rinv = 1.0 / (double)r;
    double pb[4] = {0.0, 0.0, 0.0, 0.0};
    double pg[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int jj = 0; jj < rows; ++jj) {
        const int64_t ro = (int64_t)(J * r + jj) * (nf - 1) - 1;
        const float* yrow = Y + ro;
        const double eta = (double)jj * rinv;
        for (int i = i0; i <= i1; ++i) {
            const double ow = Yw ? (double)Yw[ro + i] : 1.0;
            const double y = ow != 0.0 ? (double)yrow[i] : 0.0, yw = ow * y;
            const double xi = (double)(i - I * r) * rinv;
            double w0, w1, w2, w3;                               // corners v0, +x, +y, +x+y
            if (xi >= eta) { w0 = 1.0 - xi; w1 = xi - eta; w2 = 0.0; w3 = eta; }
            else { w0 = 1.0 - eta; w1 = 0.0; w2 = eta - xi; w3 = xi; }
            const double a0 = ow * w0, a1 = ow * w1, a2 = ow * w2, a3 = ow * w3;
            cc = fma(yw, y, cc);
            pb[0] = fma(w0, yw, pb[0]); pb[1] = fma(w1, yw, pb[1]);
            pb[2] = fma(w2, yw, pb[2]); pb[3] = fma(w3, yw, pb[3]);
            pg[0] = fma(a0, w0, pg[0]); pg[1] = fma(a1, w1, pg[1]);
            pg[2] = fma(a2, w2, pg[2]); pg[3] = fma(a3, w3, pg[3]);
            pg[4] = fma(a0, w1, pg[4]); pg[5] = fma(a0, w2, pg[5]); pg[6] = fma(a0, w3, pg[6]);
            pg[7] = fma(a1, w3, pg[7]); pg[8] = fma(a2, w3, pg[8]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) sq[c] = pb[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) sq[4 + c] = pg[c];
}
// Setup, coarse node e: the shares of the (up to four) squares that hold it, in a fixed order, into
// bn = W^T Y and the rows G [4][NN] = (p,p), (p,p+1), (p,p+nc+1), (p,p+nc+2) of W^T W.
__device__ __forceinline__ void fit_node_gather(int nc, int e, const double* sq, double* bn, double* G) {
    const int nn = (nc + 1) * (nc + 1);
    const int I = e % (nc + 1), J = e / (nc + 1);
    // the squares that hold node e, as their corner 3, 2, 1, 0
    const int q3 = (I - 1) + nc * (J - 1), q2 = I + nc * (J - 1), q1 = (I - 1) + nc * J, q0 = I + nc * J;
    const bool h3 = I > 0 && J > 0, h2 = I < nc && J > 0, h1 = I > 0 && J < nc, h0 = I < nc && J < nc;
    double b = 0.0, gd = 0.0, gx = 0.0, gy = 0.0, gxy = 0.0;
    if (h3) { b += sq[q3 * 13 + 3]; gd += sq[q3 * 13 + 4 + 3]; }
    if (h2) { b += sq[q2 * 13 + 2]; gd += sq[q2 * 13 + 4 + 2]; gx += sq[q2 * 13 + 4 + 8]; }
    if (h1) { b += sq[q1 * 13 + 1]; gd += sq[q1 * 13 + 4 + 1]; gy += sq[q1 * 13 + 4 + 7]; }
    if (h0) {
        b += sq[q0 * 13 + 0]; gd += sq[q0 * 13 + 4 + 0]; gx += sq[q0 * 13 + 4 + 4];
        gy += sq[q0 * 13 + 4 + 5]; gxy = sq[q0 * 13 + 4 + 6];
    }
    bn[e] = b;
    G[e] = gd; G[nn + e] = gx; G[2 * nn + e] = gy; G[3 * nn + e] = gxy;
}
// (G u)_e in fp64 (<= 7 non-zeros of the row)
__device__ __forceinline__ double fit_gu_row(int nc, int e, const double* G, const float* u) {
    const int nn = (nc + 1) * (nc + 1);
    const int I = e % (nc + 1), J = e / (nc + 1);
    double gu = G[e] * (double)u[e];
    if (I > 0) gu = fma(G[nn + e - 1], (double)u[e - 1], gu);
    if (I < nc) gu = fma(G[nn + e], (double)u[e + 1], gu);
    if (J > 0) gu = fma(G[2 * nn + e - (nc + 1)], (double)u[e - (nc + 1)], gu);
    if (J < nc) gu = fma(G[2 * nn + e], (double)u[e + (nc + 1)], gu);
    if (I > 0 && J > 0) gu = fma(G[3 * nn + e - (nc + 2)], (double)u[e - (nc + 2)], gu);
    if (I < nc && J < nc) gu = fma(G[3 * nn + e], (double)u[e + (nc + 2)], gu);
    return gu;
}
// Adam's bias corrections of iteration `it` (torch.optim.Adam, step = step0 + it + 1)
struct AdamStep {
    float step_size, bc2_sqrt;
};
__device__ __forceinline__ AdamStep adam_step(const gpi_rom_fit_desc& d, int it) {
    const int64_t step = d.step0 + it + 1;
    const double bc1 = 1.0 - pow((double)d.beta1, (double)step);
    const double bc2 = 1.0 - pow((double)d.beta2, (double)step);
    return {(float)((double)d.lr / bc1), (float)sqrt(bc2)};
}
// triangle t: dJ/dx by the edge formula, one Adam step on its x, m, v
__device__ __forceinline__ void fit_update(const gpi_rom_fit_desc& d, const AdamStep& a, int nc, int t,
                                           const float* lam, const float* u, const float* kp, float& x, float& m,
                                           float& v) {
    const float g = dx_of_dk(dk_edge(lam, u, nc, t), kp[t], false);
    adam_element(g, x, m, v, d.beta1, d.beta2, d.eps, a.step_size, a.bc2_sqrt);
}

template <int NC>
__global__ __launch_bounds__(64) void rom_fit_kernel(gpi_rom_fit_desc d, double gscale) {
    using S = RomFitLds<NC>;
    using Solver = typename S::Solver;
    constexpr int NN = S::NN, NT2 = S::NT2, NQ = NC * NC;
    constexpr int KX = (NT2 + 63) / 64, KQ = (NQ + 63) / 64;     // triangles, squares per lane
    extern __shared__ __attribute__((aligned(16))) double smd[];
    double* G = smd;                   // [4][NN]: (p,p), (p,p+1), (p,p+nc+1), (p,p+nc+2)
    double* bn = G + 4 * NN;           // [NN] W^T Y
    float* sm = (float*)(smd + S::ND);
    float* kp = sm + S::KP;            // [NT2] kappa
    float* u = sm + S::U;              // [NN] coarse solution
    float* lam = sm + S::LAM;          // [NN] adjoint (0 on the Dirichlet nodes)
    float* Fs = sm + S::FS;            // [NN] F_ROM_BC
    const Solver slv = {sm + S::SOLVER};
    float* bv = slv.b();               // right-hand side / solution of the interior system
    const int lane = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int r = d.refine, nf = NC * r;
    const int64_t dy = (int64_t)(nf + 1) * (nf - 1);

    // ---- setup: b = W^T Y, c = |Y|^2, G = W^T W (fp64, fixed order)
    for (int e = lane; e < NN; e += 64) Fs[e] = d.F[s * NN + e];
    double cc = 0.0;
    {
        double* sq = (double*)(slv.m + Solver::STAGE);   // [NQ][13]
        for (int k = 0; k < KQ; ++k) {
            const int q = lane + 64 * k;
            if (q < NQ) fit_square_sums(NC, r, q, d.Y + s * dy, d.y_weight ? d.y_weight + s * d.yw_stride : nullptr, cc, sq + q * 13);
        }
        cc = wave_sum_d(cc);
        Solver::sync();
        for (int e = lane; e < NN; e += 64) fit_node_gather(NC, e, sq, bn, G);
        Solver::sync();                // the solver's storage is free from here on
    }
    if (lane == 0 && d.ynorm2) d.ynorm2[s] = cc;
    if (d.iters <= 0) return;

    float xr[KX], mr[KX], vr[KX];
#pragma unroll
    for (int k = 0; k < KX; ++k) {
        const int t = lane + 64 * k;
        const bool ok = t < NT2;
        xr[k] = ok ? d.x[s * d.x_stride + t] : 0.f;
        mr[k] = ok && d.m ? d.m[s * NT2 + t] : 0.f;
        vr[k] = ok && d.v ? d.v[s * NT2 + t] : 0.f;
    }
    bool bad = false;
    for (int it = 0; it < d.iters; ++it) {
        const bool last = it == d.iters - 1;
#pragma unroll
        for (int k = 0; k < KX; ++k) {
            const int t = lane + 64 * k;
            if (t < NT2) {
                kp[t] = kappa_of(xr[k], false, bad);
                if (last && d.x_eval) d.x_eval[s * NT2 + t] = xr[k];
            }
        }
        Solver::sync();
        // ---- the interior system + rhs, the factorisation and u = K^{-1} rhs
        slv.assemble(kp, Fs);
        Solver::sync();
        slv.solve_primal();
        for (int e = lane; e < NN; e += 64) {
            const float ue = u_node(NC, e, Fs, bv);
            u[e] = ue;
            if (last && d.uc) d.uc[s * NN + e] = ue;
        }
        Solver::sync();
        // ---- fp64: G u, the squared residual and its gradient
        double ssp = 0.0;
        for (int e = lane; e < NN; e += 64) {
            const int I = e % (NC + 1), J = e / (NC + 1);
            const double gu = fit_gu_row(NC, e, G, u);
            ssp = fma((double)u[e], gu - 2.0 * bn[e], ssp);
            if (I > 0 && I < NC) bv[interior_of(NC, I, J)] = (float)(gscale * (gu - bn[e]));
        }
        const double ss = wave_sum_d(ssp) + cc;
        bad |= !(fabs(ss) <= 1.7976931348623157e308);
        if (lane == 0 && d.sumsq) d.sumsq[(int64_t)it * d.n + s] = ss;
        Solver::sync();
        // ---- adjoint lambda = K^{-1} g_u (interior), dJ/dx per coarse triangle, Adam
        slv.solve_adjoint();
        for (int e = lane; e < NN; e += 64) lam[e] = lam_node(NC, e, bv);
        Solver::sync();
        const AdamStep as = adam_step(d, it);
#pragma unroll
        for (int k = 0; k < KX; ++k) {
            const int t = lane + 64 * k;
            if (t < NT2) fit_update(d, as, NC, t, lam, u, kp, xr[k], mr[k], vr[k]);
        }
        Solver::sync();                // kp, u, lam, bv are rewritten by the next iteration
    }
#pragma unroll
    for (int k = 0; k < KX; ++k) {
        const int t = lane + 64 * k;
        if (t < NT2) {
            d.x[s * d.x_stride + t] = xr[k];
            if (d.m) d.m[s * NT2 + t] = mr[k];
            if (d.v) d.v[s * NT2 + t] = vr[k];
        }
    }
    if (bad && d.flag) atomicOr(d.flag, 1);
}

template <int NC, int NT>
void launch_fast(const gpi_rom_desc* d, const RomDims& D, void* stream) {
    if (d->y_weight)
        hipLaunchKernelGGL((rom_kernel_fast<NC, NT, true>), dim3(d->n), dim3(NT), (RomFastLds<NC, NT>::bytes), (hipStream_t)stream, *d, D);
    else
        hipLaunchKernelGGL((rom_kernel_fast<NC, NT, false>), dim3(d->n), dim3(NT), (RomFastLds<NC, NT>::bytes), (hipStream_t)stream, *d, D);
}

}  // namespace

#ifdef GPI_PHASE_TIMING
// timing build only (not declared in gpi.h): copy the ROM phase stamps out and clear them
extern "C" int gpi_debug_rom_stamps(unsigned long long* out) {
    static unsigned long long zeros[256 * 8];
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rom_phase), sizeof(zeros)) != hipSuccess) return GPI_ERR_LAUNCH;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_rom_phase), zeros, sizeof(zeros)) != hipSuccess) return GPI_ERR_LAUNCH;
    return GPI_OK;
}
#endif

extern "C" int gpi_rom_fit(const gpi_rom_fit_desc* d, void* stream) {
    if (!d || d->nc < 2 || d->refine < 1 || d->n < 0 || d->iters < 0 || d->n_total < 0 || d->step0 < 0) return GPI_ERR_ARG;
    if ((d->nc != 4 && d->nc != 8 && d->nc != 16) || (int64_t)d->nc * d->refine > 4096) return GPI_ERR_UNSUPPORTED;
    if (d->n == 0) return GPI_OK;
    if (!d->Y || !d->F || !d->x || d->x_stride < 2 * d->nc * d->nc || !d->m != !d->v) return GPI_ERR_ARG;
    const int64_t nf = (int64_t)d->nc * d->refine, dy = (nf + 1) * (nf - 1);
    if (!(d->n_obs >= 0.0) || (d->y_weight && d->yw_stride != 0 && d->yw_stride != dy)) return GPI_ERR_ARG;
    // d/du of the MSE mean: 2 / (n_total d_y) (G u - b); with observation weights 2 / n_obs
    const double gscale = 2.0 / (d->n_obs > 0.0 ? d->n_obs : (double)(d->n_total ? d->n_total : d->n) * (double)dy);
    if (d->nc == 16)
        hipLaunchKernelGGL(rom_fit_kernel<16>, dim3(d->n), dim3(64), RomFitLds<16>::bytes, (hipStream_t)stream, *d, gscale);
    else if (d->nc == 8)
        hipLaunchKernelGGL(rom_fit_kernel<8>, dim3(d->n), dim3(64), RomFitLds<8>::bytes, (hipStream_t)stream, *d, gscale);
    else
        hipLaunchKernelGGL(rom_fit_kernel<4>, dim3(d->n), dim3(64), RomFitLds<4>::bytes, (hipStream_t)stream, *d, gscale);
    GPI_CHECK_LAUNCH();
    return GPI_OK;
}

extern "C" int gpi_rom(const gpi_rom_desc* d, void* stream) {
    if (!d || !d->x || !d->F || d->nc < 2 || d->nc > 16 || d->refine < 1 || d->n < 0) return GPI_ERR_ARG;
    if (d->mode == GPI_ROM_LOGLIK && (!d->Y || !d->logsig_y || (!d->gacc_logsig && !d->gls_part) || !d->gx))
        return GPI_ERR_ARG;
    if (d->mode == GPI_ROM_BACKWARD && ((!d->dmu && !d->duc) || !d->gx)) return GPI_ERR_ARG;
    {   // observation weights: LOGLIK only, one shared row or one row per sample
        const int64_t nf = (int64_t)d->nc * d->refine;
        if (d->y_weight && (d->mode != GPI_ROM_LOGLIK || (d->yw_stride != 0 && d->yw_stride != (nf + 1) * (nf - 1))))
            return GPI_ERR_ARG;
    }
    if (d->n == 0) return GPI_OK;
    RomDims D;
    D.nc = d->nc;
    D.nn = (d->nc + 1) * (d->nc + 1);
    D.nT = 2 * d->nc * d->nc;
    D.nI = (d->nc - 1) * (d->nc + 1);
    D.bw = d->nc - 1;
    D.r = d->refine;
    D.n = d->nc * d->refine;
    D.dy = (D.n + 1) * (D.n - 1);
    if (d->mode == GPI_ROM_FORWARD && !d->mu_y && d->uc && (d->nc == 4 || d->nc == 8)) {
        const size_t lds = d->nc == 8 ? RomLaneLds<8>::bytes : RomLaneLds<4>::bytes;
        const void* k = d->nc == 8 ? (const void*)rom_lane_kernel<8> : (const void*)rom_lane_kernel<4>;
        if (lds > 64 * 1024 && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return GPI_ERR_LAUNCH;
        const dim3 grid((d->n + 63) / 64);
        if (d->nc == 8) hipLaunchKernelGGL(rom_lane_kernel<8>, grid, dim3(64), lds, (hipStream_t)stream, *d);
        else hipLaunchKernelGGL(rom_lane_kernel<4>, grid, dim3(64), lds, (hipStream_t)stream, *d);
        GPI_CHECK_LAUNCH();
        return GPI_OK;
    }
    static const bool slow = getenv("GPI_ROM_SLOW") && atoi(getenv("GPI_ROM_SLOW"));   // A/B: the r02 kernel
    if (d->nc == 16 && !slow) {
        if (d->mode == GPI_ROM_FORWARD && !d->mu_y && d->uc) {
            const dim3 grid((d->n + R16C_SPW - 1) / R16C_SPW);
            hipLaunchKernelGGL(rom16_coarse_kernel, grid, dim3(64 * R16C_SPW), Rom16CoarseLds::bytes, (hipStream_t)stream, *d);
        } else {
            launch_fast<16, 512>(d, D, stream);
        }
        GPI_CHECK_LAUNCH();
        return GPI_OK;
    }
    if ((d->nc == 8 || d->nc == 4) && !slow) {
        // nc = 8: the workgroup width (GPI_ROM_FAST_NT = 256 / 512 / 1024; r03 A/B in DESIGN.md)
        static const int fnt = getenv("GPI_ROM_FAST_NT") ? atoi(getenv("GPI_ROM_FAST_NT")) : GPI_ROM_FAST_NT_DEFAULT;
        if (d->nc == 8 && fnt == 1024) launch_fast<8, 1024>(d, D, stream);
        else if (d->nc == 8 && fnt == 512) launch_fast<8, 512>(d, D, stream);
        else if (d->nc == 8) launch_fast<8, 256>(d, D, stream);
        else launch_fast<4, 256>(d, D, stream);
        GPI_CHECK_LAUNCH();
        return GPI_OK;
    }
    if (d->y_weight) hipLaunchKernelGGL(rom_kernel<true>, dim3(d->n), dim3(ROM_NT), rom_lds(D).bytes, (hipStream_t)stream, *d, D);
    else hipLaunchKernelGGL(rom_kernel<false>, dim3(d->n), dim3(ROM_NT), rom_lds(D).bytes, (hipStream_t)stream, *d, D);
    GPI_CHECK_LAUNCH();
    return GPI_OK;
}
