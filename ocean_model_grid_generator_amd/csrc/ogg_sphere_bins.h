// The counting sort of a list of unit vectors into a uniform grid of G^3 cubes over [-1, 1]^3, shared by the runoff mapping and the
// distance to the coast (include/ogg_hip.h, "Runoff mapping" and "Distance to the coast").
#pragma once
#include "ogg_blocks.h"
#include "ogg_sphere.h"

namespace {

__device__ inline int cube_of(double v, int G) {
    const int k = (int)floor((v + 1.0) * (0.5 * (double)G));
    return k < 0 ? 0 : (k >= G ? G - 1 : k);
}

__global__ __launch_bounds__(BLOCKS_NT) void bin_count_kernel(const double* __restrict__ u, long n, int G, int* __restrict__ cnt,
                                                              int* __restrict__ bin) {
    for (long k = (long)blockIdx.x * BLOCKS_NT + threadIdx.x; k < n; k += (long)gridDim.x * BLOCKS_NT) {
        const int b = cube_of(u[3 * k], G) + G * (cube_of(u[3 * k + 1], G) + G * cube_of(u[3 * k + 2], G));
        bin[k] = b;
        atomicAdd(&cnt[b], 1);
    }
}

// every point copied into its cube's range (the order inside a cube does not matter: the key breaks ties)
__global__ __launch_bounds__(BLOCKS_NT) void bin_fill_kernel(const double* __restrict__ u, const int* __restrict__ cell, long n,
                                                             const int* __restrict__ bin, const int* __restrict__ start,
                                                             int* __restrict__ cursor, double* __restrict__ bu, int* __restrict__ bc) {
    for (long k = (long)blockIdx.x * BLOCKS_NT + threadIdx.x; k < n; k += (long)gridDim.x * BLOCKS_NT) {
        const int b = bin[k];
        const long q = (long)start[b] + atomicAdd(&cursor[b], 1);
        bu[3 * q] = u[3 * k];
        bu[3 * q + 1] = u[3 * k + 1];
        bu[3 * q + 2] = u[3 * k + 2];
        bc[q] = cell[k];
    }
}

}  // namespace
