// Fine-grid P1 helpers shared by the virtual-observable kernels (vo.hip, energy.hip).
#pragma once
#include "common.h"

namespace gpi {

__device__ __forceinline__ double kcell(const double* lk, int n, int i, int j, int ul) {
    return exp(lk[2 * (i + n * j) + ul]);
}
// conductance of the horizontal edge (i,j)-(i+1,j): the lower-right triangle of square (i,j)
// and the upper-left triangle of square (i,j-1) (P1 on right triangles: -1/2 kappa per leg)
__device__ __forceinline__ double ch_(const double* lk, int n, int i, int j) {
    double c = 0.0;
    if (j < n) c += kcell(lk, n, i, j, 0);
    if (j > 0) c += kcell(lk, n, i, j - 1, 1);
    return 0.5 * c;
}
// vertical edge (i,j)-(i,j+1): upper-left of square (i,j), lower-right of square (i-1,j)
__device__ __forceinline__ double cv_(const double* lk, int n, int i, int j) {
    double c = 0.0;
    if (i < n) c += kcell(lk, n, i, j, 1);
    if (i > 0) c += kcell(lk, n, i - 1, j, 0);
    return 0.5 * c;
}

__device__ __forceinline__ double bc_value(const double* u, int i, int j, int n) {
    const double y = (double)j / (double)n;
    return i == 0 ? u[0] * (1.0 - y) + u[1] * y : u[2] * (1.0 - y) + u[3] * y;
}

}  // namespace gpi
