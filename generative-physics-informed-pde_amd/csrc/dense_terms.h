// Per-element expressions of the dense ELBO terms, shared by every kernel form of head.hip and by gpmlp.hip.
// Plain floats in and out: each caller fetches its operands its own way (from global memory at use, from LDS, or
// prefetched into registers at kernel entry) and stores / accumulates the results its own way.  The operand
// order and the fmaf use of every expression are part of the kernels' output bits.
//
// Each block is a small struct whose results are members, asked for one at a time, not one function with several
// results.  That keeps every caller's statement order -- which operand is loaded before which store, which of two
// results is formed first -- and with it the code the compiler made before: as single functions the same
// expressions moved global loads above stores (gpmlp_bwd_kernel: 71 -> 76 VGPRs), fused the other product of
// ZDrawBwd::dls into its add (a last-bit change in the q_z rows' gradient that tools/head_digest.py caught) and
// put the head's launches 0.2 us of 23 above the parent's spread (profiles/head_refactor_ab.txt).
#pragma once
#include "common.h"

namespace gpi {

// Reparametrised draw z = mu + exp(logsigma) eps (bottleneck/utils.py:216-219, components.py:167-172) and the
// summand of -2 KL(q(z) || N(0, I)) (utils.py:246-248, components.py:192-193).
struct ZDraw {
    float mu, ls, e;
    __device__ __forceinline__ ZDraw(float mu_, float ls_) : mu(mu_), ls(ls_), e(expf(ls_)) {}
    __device__ __forceinline__ float z(float eps) const { return fmaf(e, eps, mu); }
    __device__ __forceinline__ float kl() const { return 1.f + 2.f * ls - mu * mu - e * e; }
};

// d/dmu and d/dlogsigma of a drawn z's row (a q_z row, or an encoder sample's heads): the draw's part of dJ/dz
// and the KL term's, scaled by kl_scale.  (The q_z rows form dmu first, the encoder rows dls.)
struct ZDrawBwd {
    float kl_scale, e;
    __device__ __forceinline__ ZDrawBwd(float ls, float kl_scale_) : kl_scale(kl_scale_), e(expf(ls)) {}
    __device__ __forceinline__ float dmu(float dz, float mu) const { return dz + kl_scale * mu; }
    __device__ __forceinline__ float dls(float dz, float eps) const {
        return dz * e * eps + kl_scale * (e * e - 1.f);
    }
};

// gp term of one element, free X: X~ = q_X mean + exp(q_X logsigma) eps and the summand of
// log N(X~; a, exp(logsigma_X)) with a = gp(z) (generative.py:464-478, components.py:195-197,224-229).  The
// entropy summand is the q_X logsigma itself.
struct GpElemFwd {
    float xs;   // X~
    __device__ __forceinline__ GpElemFwd(float qx_mu, float qx_ls, float eps) : xs(fmaf(expf(qx_ls), eps, qx_mu)) {}
    __device__ __forceinline__ float loglik(float a, float gls) const {
        const float r = xs - a;
        return -0.5f * (2.f * gls + r * r * expf(-2.f * gls) + GPI_LOG2PI);
    }
};

// gp term backward of one element, free X, from the stored X~ and mu_X = gp(z); lx_scale is the segment's scale
// of logL_X and of the entropy.  The q_X rows' gradients need the ROM adjoint gxs (dJ/dX~ from the likelihood's
// side), the q_X logsigma and the noise: a caller that reads them from global memory does so after it has stored
// dJ/dmu_X.
struct GpElemBwd {
    float lx_scale, e2, r;
    __device__ __forceinline__ GpElemBwd(float xs, float mux, float gls, float lx_scale_)
        : lx_scale(lx_scale_), e2(expf(-2.f * gls)), r(xs - mux) {}
    // dJ/dmu_X
    __device__ __forceinline__ float gmux() const { return -lx_scale * r * e2; }
    // the element's contribution to dJ/dlogsigma_X
    __device__ __forceinline__ float gls() const { return lx_scale * (1.f - r * r * e2); }
    // dJ/d(q_X mean) = the whole dJ/dX~
    __device__ __forceinline__ float gqx_mu(float gxs) const { return gxs + lx_scale * r * e2; }
    // dJ/d(q_X logsigma) from dxs = gqx_mu(gxs), the entropy's -lx_scale included
    __device__ __forceinline__ float gqx_ls(float dxs, float qx_ls, float eps) const {
        return dxs * expf(qx_ls) * eps - lx_scale;
    }
};

}  // namespace gpi
