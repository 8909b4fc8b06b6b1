// The counting sort of a list of unit vectors into a uniform grid of G^3 cubes over [-1, 1]^3, shared by the runoff mapping and the
// distance to the coast (include/ogg_hip.h, "Runoff mapping" and "Distance to the coast"): the two kernels, the index's workspace
// sections and the host sequence that builds it.  Which G, and how the cubes are searched, is each caller's own.
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

// ---- the index as a whole ------------------------------------------------------------------------------------------
// cube b holds the targets start[b] .. start[b + 1] - 1 of bu / bc (start: G^3 + 1 entries); cnt and bin are the sort's scratch
struct CubeIndex {
    int *cnt, *start, *bin;
    double* bu;
    int* bc;
};

struct CubeIndexLayout {
    long cnt, start, bin, bu, bc;
};

// its five sections, for at most nt targets and nbins_max = (the largest G)^3 + 1 cubes (a braced list is evaluated left to right)
inline CubeIndexLayout cube_index_sections(ogg::Sections& s, long nt, long nbins_max) {
    return CubeIndexLayout{s.take(nbins_max * 4), s.take(nbins_max * 4), s.take(nt * 4), s.take(nt * 24), s.take(nt * 4)};
}

inline CubeIndex cube_index_at(void* ws, const CubeIndexLayout& l) {
    return CubeIndex{ogg::at<int>(ws, l.cnt), ogg::at<int>(ws, l.start), ogg::at<int>(ws, l.bin), ogg::at<double>(ws, l.bu),
                     ogg::at<int>(ws, l.bc)};
}

// the nt targets tu / tc sorted into G^3 cubes; bsum and total: the scan's scratch (ogg_blocks.h)
inline int build_cube_index(const double* tu, const int* tc, long nt, int G, const CubeIndex& ix, long long* bsum, long long* total,
                            hipStream_t st) {
    const long nb1 = (long)G * G * G + 1;
    OGG_HIP_CHECK(hipMemsetAsync(ix.cnt, 0, (size_t)nb1 * 4, st));
    bin_count_kernel<<<ogg::grid_for<BLOCKS_NT>(nt, 4096), BLOCKS_NT, 0, st>>>(tu, nt, G, ix.cnt, ix.bin);
    OGG_LAUNCH_CHECK();
    // starts: the exclusive prefix of the counts over G^3 + 1 cubes (the last count is 0, so the last start is nt)
    if (int e = exclusive_scan<false>(ix.cnt, nb1, bsum, total, ix.start, st)) return e;
    OGG_HIP_CHECK(hipMemsetAsync(ix.cnt, 0, (size_t)nb1 * 4, st));   // the cursors of the fill
    bin_fill_kernel<<<ogg::grid_for<BLOCKS_NT>(nt, 4096), BLOCKS_NT, 0, st>>>(tu, tc, nt, ix.bin, ix.start, ix.cnt, ix.bu, ix.bc);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

}  // namespace
