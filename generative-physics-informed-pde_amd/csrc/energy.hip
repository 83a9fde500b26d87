// Energy virtual observables (EnergyVirtualObservable.update, VirtualObservables.py:769-788) for gfx950.
//
// Reference: per VO sample and inner iteration, numpy builds the dense A = diag(prec) + beta K
// [d_y, d_y], multiplies it by the test functions V [d_y, m_aux] and solves the m_aux x m_aux system
//   mean <- mean - V (V^T A V)^-1 V^T (A mean - b),   b = beta f + prec * g.
// Here nothing is assembled: K is the 5-point stencil of edge conductances (ch_ / cv_), f lives on the
// two Dirichlet-adjacent columns and the RBF test functions are products of per-axis tables
//   V_a(i, j) = tx[a][i] ty[a][j],  tx[a][i] = exp(-(i/n - cx_a)^2 / l^2),
// so (A V_a) at a node is a handful of table products.  Two forms share every device function below:
//   vo_energy_fused_kernel    one workgroup per sample, all iterations in one launch; mean, conductances and
//                             tables LDS-resident
//   vo_energy_{prep,vars,partial,solve,update}_kernel
//                             any grid: per iteration partial sums per (row tile, sample), one solve per
//                             sample, one update per (row tile, sample); state in the caller's workspace
// Per iteration V^T (A mean - b) and the lower EN_CH x EN_CH blocks of V^T A V are accumulated per thread
// over its nodes in node order, summed over the wave by a fixed butterfly and over the waves (and tiles)
// in index order: no atomics on floating-point data, the same bits on every run.
#include "common.h"
#include "vo_grid.h"

using namespace gpi;

namespace {

constexpr int EN_CH = 8;                        // chunk of test functions per accumulator block
constexpr int EN_NV = EN_CH * EN_CH + EN_CH;    // values reduced per pass: the block and its share of V^T r
constexpr int EN_NT_FUSED = 256;
constexpr int EN_NT_TILED = 256;
constexpr int EN_LDS_MAX = 160 * 1024;
// A pivot of V^T A V at or below this share of its diagonal entry marks a degenerate subspace: with two
// coincident centres the pivot is x - (x / sqrt(x))^2, a few ulp of x of either sign, never reliably <= 0.
constexpr double EN_PIVOT_TOL = 1e-12;

inline int round_up_ch(int m) { return (m + EN_CH - 1) / EN_CH * EN_CH; }

// row tiling of the free nodes (rows j = 0..n of n - 1 nodes) for the tiled form
struct EnergyTiling {
    int rows, tiles, mp;
    int64_t off_cv, off_part, off_coef, per_sample;   // workspace offsets per sample (doubles)
    size_t lds;
};

inline void tiling_of(int n, int m, EnergyTiling& T) {
    T.mp = round_up_ch(m);
    T.rows = (EN_NT_TILED + n - 2) / (n - 1);
    if (T.rows > n + 1) T.rows = n + 1;
    T.tiles = (n + 1 + T.rows - 1) / T.rows;
    T.off_cv = (int64_t)(n + 1) * n;
    T.off_part = T.off_cv + (int64_t)n * (n - 1);
    T.off_coef = T.off_part + (int64_t)T.tiles * (T.mp * T.mp + T.mp);
    T.per_sample = T.off_coef + T.mp;
    T.lds = sizeof(double) * ((size_t)T.mp * (n + 1) + (size_t)T.mp * (T.rows + 2) + (EN_NT_TILED / 64) * EN_NV +
                              2 * T.mp);
}

inline size_t fused_lds(int n, int m) {
    const size_t mp = round_up_ch(m), dy = (size_t)(n + 1) * (n - 1);
    return sizeof(double) * (dy + (size_t)(n + 1) * n + (size_t)n * (n - 1) + 2 * mp * (n + 1) +
                             (EN_NT_FUSED / 64) * EN_NV + mp * mp + 4 * mp);
}

// ---------------------------------------------------------------- shared device functions
// ch[j n + i] = conductance of edge (i,j)-(i+1,j), i < n, j <= n;  cv[j (n-1) + i - 1] = edge (i,j)-(i,j+1),
// 1 <= i <= n - 1, j < n (the vertical edges of the free columns)
__device__ __forceinline__ void energy_fill_conductances(const double* lk, int n, double* ch, double* cv, int t0,
                                                         int nt) {
    for (int e = t0; e < (n + 1) * n; e += nt) {
        const int j = e / n, i = e - j * n;
        ch[e] = ch_(lk, n, i, j);
    }
    for (int e = t0; e < n * (n - 1); e += nt) {
        const int j = e / (n - 1), i = e - j * (n - 1) + 1;
        cv[e] = cv_(lk, n, i, j);
    }
}

// row of K_ff at free node (ii, jj): diagonal, the weights of the free neighbours (0 where there is none)
// and the node's entry of f_eff
struct EnergyNode {
    double diag, wl, wr, wd, wu, f;
};

__device__ __forceinline__ EnergyNode energy_node(const double* ch, const double* cv, const double* u, int n, int ii,
                                                  int jj) {
    const double cl = ch[jj * n + ii - 1], cr = ch[jj * n + ii];
    const double cd = jj > 0 ? cv[(jj - 1) * (n - 1) + ii - 1] : 0.0;
    const double cu = jj < n ? cv[jj * (n - 1) + ii - 1] : 0.0;
    EnergyNode nd;
    nd.diag = cl + cr + cd + cu;
    nd.wl = ii > 1 ? cl : 0.0;
    nd.wr = ii < n - 1 ? cr : 0.0;
    nd.wd = cd;
    nd.wu = cu;
    nd.f = 0.0;
    if (ii == 1) nd.f += cl * bc_value(u, 0, jj, n);
    if (ii == n - 1) nd.f += cr * bc_value(u, n, jj, n);
    return nd;
}

// (K mean) at node p = jj (n - 1) + ii - 1
__device__ __forceinline__ double energy_stencil(const EnergyNode& nd, const double* mean, int p, int n, int ii,
                                                 int jj) {
    double s = nd.diag * mean[p];
    if (ii > 1) s -= nd.wl * mean[p - 1];
    if (ii < n - 1) s -= nd.wr * mean[p + 1];
    if (jj > 0) s -= nd.wd * mean[p - (n - 1)];
    if (jj < n) s -= nd.wu * mean[p + (n - 1)];
    return s;
}

__device__ __forceinline__ void energy_store_vars(const gpi_vo_energy_desc& d, int64_t o, double prec, double beta,
                                                  double diag) {
    const double v = 1.0 / (prec + beta * diag);
    d.vars[o] = v;
    // the log in fp64, rounded once: the float log of the device library is only good to an ulp, this is exact
    if (d.logsig32) d.logsig32[o] = (float)(0.5 * log((double)(float)v));
}

// centres of iteration `it` of sample s into cen[2 a], cen[2 a + 1] (0 for the padding a >= m_aux)
__device__ __forceinline__ void energy_centres(const gpi_vo_energy_desc& d, int it, int s, int mp, uint64_t base,
                                               double* cen, bool record) {
    const int a = threadIdx.x;
    if (a >= mp) return;
    double cx = 0.0, cy = 0.0;
    if (a < d.m_aux) {
        const int64_t e = ((int64_t)it * d.n + s) * d.m_aux + a;
        if (d.centers) {
            cx = d.centers[2 * e];
            cy = d.centers[2 * e + 1];
        } else {
            const uint4_ q = philox(base + (uint64_t)e, d.sub, d.seed);
            cx = (double)q.x * 2.3283064365386963e-10;
            cy = (double)q.y * 2.3283064365386963e-10;
        }
        if (record && d.centers_out) {
            d.centers_out[2 * e] = cx;
            d.centers_out[2 * e + 1] = cy;
        }
    }
    cen[2 * a] = cx;
    cen[2 * a + 1] = cy;
}

// tx[a (n + 1) + i], i = 0..n;  ty[a nj + j - j0], j = j0..j0 + nj - 1 (rows outside the grid carry weight 0
// wherever they are read); zero for the padding a >= m
__device__ __forceinline__ void energy_tables(double* tx, double* ty, const double* cen, double length, int n, int m,
                                              int mp, int j0, int nj) {
    const double il2 = 1.0 / (length * length);
    for (int e = threadIdx.x; e < mp * (n + 1); e += blockDim.x) {
        const int a = e / (n + 1), i = e - a * (n + 1);
        const double x = (double)i / (double)n - cen[2 * a];
        tx[e] = a < m ? exp(-(x * x) * il2) : 0.0;
    }
    for (int e = threadIdx.x; e < mp * nj; e += blockDim.x) {
        const int a = e / nj, j = j0 + e - a * nj;
        const double y = (double)j / (double)n - cen[2 * a + 1];
        ty[e] = a < m ? exp(-(y * y) * il2) : 0.0;
    }
}

// one node's share of block (ca, cb) of V^T A V and of chunk ca of V^T r.  txa / tya, txb / tyb: the tables at
// the first test function of chunk ca / cb; jl, jd, ju: the table columns of rows jj, jj - 1, jj + 1 (clamped
// into the table; their weights are 0 where the row does not exist)
__device__ __forceinline__ void energy_node_accumulate(const EnergyNode& nd, double prec, double beta, double r,
                                                       const double* txa, const double* tya, const double* txb,
                                                       const double* tyb, int txs, int tys, int ii, int jl, int jd,
                                                       int ju, double (&acc)[EN_CH][EN_CH], double (&vr)[EN_CH]) {
    double va[EN_CH], avb[EN_CH];
#pragma unroll
    for (int t = 0; t < EN_CH; ++t) {
        va[t] = txa[t * txs + ii] * tya[t * tys + jl];
        const double* x = txb + t * txs;
        const double* y = tyb + t * tys;
        const double xc = x[ii], yc = y[jl];
        const double kv = yc * (nd.diag * xc - nd.wl * x[ii - 1] - nd.wr * x[ii + 1]) -
                          xc * (nd.wd * y[jd] + nd.wu * y[ju]);
        avb[t] = prec * (xc * yc) + beta * kv;
    }
#pragma unroll
    for (int i = 0; i < EN_CH; ++i) {
#pragma unroll
        for (int j = 0; j < EN_CH; ++j) acc[i][j] = fma(va[i], avb[j], acc[i][j]);
        vr[i] = fma(va[i], r, vr[i]);
    }
}

// block sum of the EN_NV per-thread values; thread v < EN_NV returns value v (block entry v / EN_CH, v % EN_CH,
// then the EN_CH entries of V^T r).  The caller synchronises before sred is written again.
__device__ __forceinline__ double energy_block_reduce(double (&acc)[EN_CH][EN_CH], double (&vr)[EN_CH], double* sred) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < EN_CH; ++i)
#pragma unroll
        for (int j = 0; j < EN_CH; ++j) {
            const double s = wave_sum_d(acc[i][j]);
            if (lane == 0) sred[w * EN_NV + i * EN_CH + j] = s;
        }
#pragma unroll
    for (int i = 0; i < EN_CH; ++i) {
        const double s = wave_sum_d(vr[i]);
        if (lane == 0) sred[w * EN_NV + EN_CH * EN_CH + i] = s;
    }
    __syncthreads();
    double t = 0.0;
    if ((int)threadIdx.x < EN_NV)
        for (int k = 0; k < nw; ++k) t += sred[k * EN_NV + threadIdx.x];
    return t;
}

// In-place lower Cholesky of A [m, m] (LDS, row-major, lower triangle read) and A x = b by the whole block
// (b <- x).  Returns false, with A and b in an undefined state, at the first pivot <= EN_PIVOT_TOL of its
// diagonal entry (dg: m doubles of scratch).  Uniform: every thread takes the same way out.
__device__ bool energy_chol_solve(double* A, double* b, double* dg, int m) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < m; e += nt) dg[e] = A[e * m + e];
    __syncthreads();
    for (int k = 0; k < m; ++k) {
        const double akk = A[k * m + k];
        if (!(akk > 0.0 && akk > EN_PIVOT_TOL * dg[k])) return false;
        const double dk = sqrt(akk);
        __syncthreads();
        for (int i = k + 1 + tid; i < m; i += nt) A[i * m + k] /= dk;
        if (tid == 0) A[k * m + k] = dk;
        __syncthreads();
        for (int e = tid; e < m * m; e += nt) {
            const int i = e / m, j = e - i * m;
            if (j > k && j <= i) A[e] -= A[i * m + k] * A[j * m + k];
        }
        __syncthreads();
    }
    for (int k = 0; k < m; ++k) {                    // L z = b
        const double zk = b[k] / A[k * m + k];
        __syncthreads();
        for (int i = k + 1 + tid; i < m; i += nt) b[i] -= A[i * m + k] * zk;
        if (tid == 0) b[k] = zk;
        __syncthreads();
    }
    for (int k = m - 1; k >= 0; --k) {               // L^T x = z
        const double xk = b[k] / A[k * m + k];
        __syncthreads();
        for (int i = tid; i < k; i += nt) b[i] -= A[k * m + i] * xk;
        if (tid == 0) b[k] = xk;
        __syncthreads();
    }
    return true;
}

// (V c) at a node
__device__ __forceinline__ double energy_combine(const double* tx, const double* ty, int txs, int tys, int ii, int jl,
                                                 const double* c, int m) {
    double s = 0.0;
    for (int a = 0; a < m; ++a) s = fma(tx[a * txs + ii] * ty[a * tys + jl], c[a], s);
    return s;
}

// ---------------------------------------------------------------- fused form
__global__ __launch_bounds__(EN_NT_FUSED) void vo_energy_fused_kernel(gpi_vo_energy_desc d, int mp) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int s = blockIdx.x, n = d.n_fine, dy = (n + 1) * (n - 1), m = d.m_aux;
    const int tid = threadIdx.x;
    double* smean = sm;                                   // [dy]
    double* sch = smean + dy;                             // [(n + 1) n]
    double* scv = sch + (n + 1) * n;                      // [n (n - 1)]
    double* stx = scv + n * (n - 1);                      // [mp][n + 1]
    double* sty = stx + mp * (n + 1);                     // [mp][n + 1]
    double* sred = sty + mp * (n + 1);                    // [waves][EN_NV]
    double* sM = sred + (EN_NT_FUSED / 64) * EN_NV;       // [m][m]
    double* sb = sM + mp * mp;                            // [mp] V^T r, then the coefficients
    double* sdg = sb + mp;                                // [mp]
    double* scen = sdg + mp;                              // [mp][2]
    const double* lk = d.logkappa + (int64_t)s * 2 * n * n;
    const double* u = d.bc + 4 * s;
    const float* g = d.g + (int64_t)s * dy;
    const float* prec = d.prec + (int64_t)s * dy;
    double* mean = d.mean + (int64_t)s * dy;
    const double beta = 1.0 / d.temperature;
    const uint64_t base = d.offset ? *d.offset : 0;
    const int txs = n + 1;

    energy_fill_conductances(lk, n, sch, scv, tid, EN_NT_FUSED);
    for (int p = tid; p < dy; p += EN_NT_FUSED) smean[p] = mean[p];
    __syncthreads();
    for (int p = tid; p < dy; p += EN_NT_FUSED) {
        const int jj = p / (n - 1), ii = p - jj * (n - 1) + 1;
        const EnergyNode nd = energy_node(sch, scv, u, n, ii, jj);
        energy_store_vars(d, (int64_t)s * dy + p, (double)prec[p], beta, nd.diag);
    }
    for (int it = 0; it < d.n_iter; ++it) {
        energy_centres(d, it, s, mp, base, scen, true);
        __syncthreads();
        energy_tables(stx, sty, scen, d.length, n, m, mp, 0, n + 1);
        __syncthreads();
        for (int ca = 0; ca < mp / EN_CH; ++ca)
            for (int cb = 0; cb <= ca; ++cb) {
                double acc[EN_CH][EN_CH], vr[EN_CH];
#pragma unroll
                for (int i = 0; i < EN_CH; ++i) {
                    vr[i] = 0.0;
#pragma unroll
                    for (int j = 0; j < EN_CH; ++j) acc[i][j] = 0.0;
                }
                const double* txa = stx + ca * EN_CH * txs;
                const double* tya = sty + ca * EN_CH * txs;
                const double* txb = stx + cb * EN_CH * txs;
                const double* tyb = sty + cb * EN_CH * txs;
                for (int p = tid; p < dy; p += EN_NT_FUSED) {
                    const int jj = p / (n - 1), ii = p - jj * (n - 1) + 1;
                    const EnergyNode nd = energy_node(sch, scv, u, n, ii, jj);
                    const double pr = (double)prec[p];
                    double r = 0.0;
                    if (cb == 0)
                        r = pr * smean[p] + beta * (energy_stencil(nd, smean, p, n, ii, jj) - nd.f) -
                            pr * (double)g[p];
                    energy_node_accumulate(nd, pr, beta, r, txa, tya, txb, tyb, txs, txs, ii, jj, max(jj - 1, 0),
                                           min(jj + 1, n), acc, vr);
                }
                const double t = energy_block_reduce(acc, vr, sred);
                if (tid < EN_CH * EN_CH) {
                    const int a = ca * EN_CH + tid / EN_CH, b = cb * EN_CH + tid % EN_CH;
                    if (a < m && b < m) sM[a * m + b] = t;
                } else if (tid < EN_NV && cb == 0) {
                    const int a = ca * EN_CH + tid - EN_CH * EN_CH;
                    if (a < m) sb[a] = t;
                }
                __syncthreads();
            }
        if (energy_chol_solve(sM, sb, sdg, m)) {
            for (int p = tid; p < dy; p += EN_NT_FUSED) {
                const int jj = p / (n - 1), ii = p - jj * (n - 1) + 1;
                smean[p] -= energy_combine(stx, sty, txs, txs, ii, jj, sb, m);
            }
        } else if (tid == 0 && d.flag) {
            atomicOr(d.flag, 1);
        }
        __syncthreads();
    }
    for (int p = tid; p < dy; p += EN_NT_FUSED) {
        const double v = smean[p];
        if (d.n_iter > 0) mean[p] = v;
        if (d.mean32) d.mean32[(int64_t)s * dy + p] = (float)v;
    }
}

// ---------------------------------------------------------------- tiled form
__global__ __launch_bounds__(256) void vo_energy_prep_kernel(gpi_vo_energy_desc d, EnergyTiling T) {
    const int s = blockIdx.y, n = d.n_fine;
    double* ws = d.work + (int64_t)s * T.per_sample;
    energy_fill_conductances(d.logkappa + (int64_t)s * 2 * n * n, n, ws, ws + T.off_cv,
                             blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

__global__ __launch_bounds__(256) void vo_energy_vars_kernel(gpi_vo_energy_desc d, EnergyTiling T) {
    const int s = blockIdx.y, n = d.n_fine, dy = (n + 1) * (n - 1);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= dy) return;
    const double* ws = d.work + (int64_t)s * T.per_sample;
    const int jj = p / (n - 1), ii = p - jj * (n - 1) + 1;
    const EnergyNode nd = energy_node(ws, ws + T.off_cv, d.bc + 4 * s, n, ii, jj);
    const int64_t o = (int64_t)s * dy + p;
    energy_store_vars(d, o, (double)d.prec[o], 1.0 / d.temperature, nd.diag);
    if (d.n_iter == 0 && d.mean32) d.mean32[o] = (float)d.mean[o];
}

// LDS of the partial and update kernels: tx [mp][n + 1], ty [mp][rows + 2] (rows j0 - 1 .. j0 + rows), the
// reduction scratch, the centres
__global__ __launch_bounds__(EN_NT_TILED) void vo_energy_partial_kernel(gpi_vo_energy_desc d, EnergyTiling T, int it) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tile = blockIdx.x, s = blockIdx.y, n = d.n_fine, dy = (n + 1) * (n - 1), m = d.m_aux, mp = T.mp;
    const int tid = threadIdx.x;
    const int txs = n + 1, tys = T.rows + 2;
    double* stx = sm;
    double* sty = stx + mp * txs;
    double* sred = sty + mp * tys;
    double* scen = sred + (EN_NT_TILED / 64) * EN_NV;
    const double* ws = d.work + (int64_t)s * T.per_sample;
    const double* ch = ws;
    const double* cv = ws + T.off_cv;
    double* part = d.work + (int64_t)s * T.per_sample + T.off_part + (int64_t)tile * (mp * mp + mp);
    const double* u = d.bc + 4 * s;
    const float* g = d.g + (int64_t)s * dy;
    const float* prec = d.prec + (int64_t)s * dy;
    const double* mean = d.mean + (int64_t)s * dy;
    const double beta = 1.0 / d.temperature;
    const int j0 = tile * T.rows, j1 = min(j0 + T.rows, n + 1);
    const int p0 = j0 * (n - 1), p1 = j1 * (n - 1);
    energy_centres(d, it, s, mp, d.offset ? *d.offset : 0, scen, tile == 0);
    __syncthreads();
    energy_tables(stx, sty, scen, d.length, n, m, mp, j0 - 1, tys);
    __syncthreads();
    for (int ca = 0; ca < mp / EN_CH; ++ca)
        for (int cb = 0; cb <= ca; ++cb) {
            double acc[EN_CH][EN_CH], vr[EN_CH];
#pragma unroll
            for (int i = 0; i < EN_CH; ++i) {
                vr[i] = 0.0;
#pragma unroll
                for (int j = 0; j < EN_CH; ++j) acc[i][j] = 0.0;
            }
            for (int p = p0 + tid; p < p1; p += EN_NT_TILED) {
                const int jj = p / (n - 1), ii = p - jj * (n - 1) + 1;
                const EnergyNode nd = energy_node(ch, cv, u, n, ii, jj);
                const double pr = (double)prec[p];
                double r = 0.0;
                if (cb == 0)
                    r = pr * mean[p] + beta * (energy_stencil(nd, mean, p, n, ii, jj) - nd.f) - pr * (double)g[p];
                const int jl = jj - j0 + 1;
                energy_node_accumulate(nd, pr, beta, r, stx + ca * EN_CH * txs, sty + ca * EN_CH * tys,
                                       stx + cb * EN_CH * txs, sty + cb * EN_CH * tys, txs, tys, ii, jl, jl - 1,
                                       jl + 1, acc, vr);
            }
            const double t = energy_block_reduce(acc, vr, sred);
            if (tid < EN_CH * EN_CH) {
                const int a = ca * EN_CH + tid / EN_CH, b = cb * EN_CH + tid % EN_CH;
                part[a * mp + b] = t;
            } else if (tid < EN_NV && cb == 0) {
                part[mp * mp + ca * EN_CH + tid - EN_CH * EN_CH] = t;
            }
            __syncthreads();
        }
}

// sums the tiles' partial sums in tile order, factors and solves; coefficients (zeros for a skipped
// iteration) into the workspace
__global__ __launch_bounds__(EN_NT_TILED) void vo_energy_solve_kernel(gpi_vo_energy_desc d, EnergyTiling T) {
    __shared__ double sM[GPI_VO_ENERGY_MAX_AUX * GPI_VO_ENERGY_MAX_AUX];
    __shared__ double sb[GPI_VO_ENERGY_MAX_AUX], sdg[GPI_VO_ENERGY_MAX_AUX];
    const int s = blockIdx.x, m = d.m_aux, mp = T.mp, tid = threadIdx.x;
    const double* part = d.work + (int64_t)s * T.per_sample + T.off_part;
    double* coef = d.work + (int64_t)s * T.per_sample + T.off_coef;
    const int stride = mp * mp + mp;
    for (int e = tid; e < m * m + m; e += EN_NT_TILED) {
        const int a = e < m * m ? e / m : e - m * m, b = e < m * m ? e - a * m : 0;
        if (e < m * m && b > a) continue;                 // only the lower blocks were accumulated
        const int src = e < m * m ? a * mp + b : mp * mp + a;
        double t = 0.0;
        for (int k = 0; k < T.tiles; ++k) t += part[(int64_t)k * stride + src];
        if (e < m * m) sM[e] = t;
        else sb[a] = t;
    }
    __syncthreads();
    const bool ok = energy_chol_solve(sM, sb, sdg, m);
    if (!ok && tid == 0 && d.flag) atomicOr(d.flag, 1);
    __syncthreads();
    for (int a = tid; a < mp; a += EN_NT_TILED) coef[a] = (ok && a < m) ? sb[a] : 0.0;
}

__global__ __launch_bounds__(EN_NT_TILED) void vo_energy_update_kernel(gpi_vo_energy_desc d, EnergyTiling T, int it) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tile = blockIdx.x, s = blockIdx.y, n = d.n_fine, dy = (n + 1) * (n - 1), m = d.m_aux, mp = T.mp;
    const int tid = threadIdx.x;
    const int txs = n + 1, tys = T.rows + 2;
    double* stx = sm;
    double* sty = stx + mp * txs;
    double* sc = sty + mp * tys;                          // coefficients (in the reduction scratch's place)
    double* scen = sc + (EN_NT_TILED / 64) * EN_NV;
    const double* coef = d.work + (int64_t)s * T.per_sample + T.off_coef;
    double* mean = d.mean + (int64_t)s * dy;
    const int j0 = tile * T.rows, j1 = min(j0 + T.rows, n + 1);
    energy_centres(d, it, s, mp, d.offset ? *d.offset : 0, scen, false);
    for (int a = tid; a < mp; a += EN_NT_TILED) sc[a] = coef[a];
    __syncthreads();
    energy_tables(stx, sty, scen, d.length, n, m, mp, j0 - 1, tys);
    __syncthreads();
    const bool last = it == d.n_iter - 1;
    for (int p = j0 * (n - 1) + tid; p < j1 * (n - 1); p += EN_NT_TILED) {
        const int jj = p / (n - 1), ii = p - jj * (n - 1) + 1;
        const double v = mean[p] - energy_combine(stx, sty, txs, tys, ii, jj - j0 + 1, sc, m);
        mean[p] = v;
        if (last && d.mean32) d.mean32[(int64_t)s * dy + p] = (float)v;
    }
}

bool args_ok(const gpi_vo_energy_desc* d) {
    return d && d->logkappa && d->bc && d->g && d->prec && d->mean && d->vars && d->n >= 0 && d->n_fine >= 2 &&
           d->m_aux >= 1 && d->m_aux <= GPI_VO_ENERGY_MAX_AUX && d->n_iter >= 0 &&
           d->n_iter <= GPI_VO_ENERGY_MAX_ITER && d->temperature > 0.0 && d->length > 0.0 &&
           d->form >= GPI_VO_ENERGY_AUTO && d->form <= GPI_VO_ENERGY_TILED;
}

}  // namespace

extern "C" int gpi_vo_energy_form(int32_t n_fine, int32_t m_aux) {
    if (n_fine < 2 || m_aux < 1 || m_aux > GPI_VO_ENERGY_MAX_AUX) return GPI_ERR_ARG;
    if (n_fine > 4096) return GPI_ERR_UNSUPPORTED;
    if (fused_lds(n_fine, m_aux) <= (size_t)EN_LDS_MAX) return GPI_VO_ENERGY_FUSED;
    EnergyTiling T;
    tiling_of(n_fine, m_aux, T);
    return T.lds <= (size_t)EN_LDS_MAX ? GPI_VO_ENERGY_TILED : GPI_ERR_UNSUPPORTED;
}

extern "C" int64_t gpi_vo_energy_workspace(int32_t n_fine, int32_t n, int32_t m_aux) {
    if (n_fine < 2 || n_fine > 4096 || n < 0 || m_aux < 1 || m_aux > GPI_VO_ENERGY_MAX_AUX) return GPI_ERR_ARG;
    EnergyTiling T;
    tiling_of(n_fine, m_aux, T);
    return T.per_sample * (int64_t)n;
}

extern "C" int gpi_vo_energy(const gpi_vo_energy_desc* d, void* stream) {
    if (!args_ok(d)) return GPI_ERR_ARG;
    const int n = d->n_fine, m = d->m_aux;
    if (n > 4096) return GPI_ERR_UNSUPPORTED;
    EnergyTiling T;
    tiling_of(n, m, T);
    const bool fused_fits = fused_lds(n, m) <= (size_t)EN_LDS_MAX;
    const bool tiled_fits = T.lds <= (size_t)EN_LDS_MAX && d->n <= 65535;
    int form = d->form;
    if (form == GPI_VO_ENERGY_AUTO) form = fused_fits ? GPI_VO_ENERGY_FUSED : GPI_VO_ENERGY_TILED;
    if (form == GPI_VO_ENERGY_FUSED ? !fused_fits : !tiled_fits) return GPI_ERR_UNSUPPORTED;
    if (form == GPI_VO_ENERGY_TILED && !d->work) return GPI_ERR_ARG;
    if (d->n == 0) return GPI_OK;
    const hipStream_t st = (hipStream_t)stream;
    if (form == GPI_VO_ENERGY_FUSED) {
        static bool attr = false;
        if (!attr) {
            if (hipFuncSetAttribute((const void*)vo_energy_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    EN_LDS_MAX) != hipSuccess)
                return GPI_ERR_LAUNCH;
            attr = true;
        }
        hipLaunchKernelGGL(vo_energy_fused_kernel, dim3(d->n), dim3(EN_NT_FUSED), fused_lds(n, m), st, *d, T.mp);
        GPI_CHECK_LAUNCH();
        return GPI_OK;
    }
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)vo_energy_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                EN_LDS_MAX) != hipSuccess ||
            hipFuncSetAttribute((const void*)vo_energy_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                EN_LDS_MAX) != hipSuccess)
            return GPI_ERR_LAUNCH;
        attr = true;
    }
    const int dy = (n + 1) * (n - 1);
    const int edges = ((n + 1) * n + 255) / 256, prep_blocks = edges < 64 ? edges : 64;
    hipLaunchKernelGGL(vo_energy_prep_kernel, dim3(prep_blocks, d->n), dim3(256), 0, st, *d, T);
    GPI_CHECK_LAUNCH();
    hipLaunchKernelGGL(vo_energy_vars_kernel, dim3((dy + 255) / 256, d->n), dim3(256), 0, st, *d, T);
    GPI_CHECK_LAUNCH();
    for (int it = 0; it < d->n_iter; ++it) {
        hipLaunchKernelGGL(vo_energy_partial_kernel, dim3(T.tiles, d->n), dim3(EN_NT_TILED), T.lds, st, *d, T, it);
        GPI_CHECK_LAUNCH();
        hipLaunchKernelGGL(vo_energy_solve_kernel, dim3(d->n), dim3(EN_NT_TILED), 0, st, *d, T);
        GPI_CHECK_LAUNCH();
        hipLaunchKernelGGL(vo_energy_update_kernel, dim3(T.tiles, d->n), dim3(EN_NT_TILED), T.lds, st, *d, T, it);
        GPI_CHECK_LAUNCH();
    }
    return GPI_OK;
}
