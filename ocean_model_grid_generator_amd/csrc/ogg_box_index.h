// The padded-box index of great-circle cells over cubes of the unit sphere (include/ogg_hip.h, "Point location", box), shared by point
// location (ogg_locate.hip: the model cells, searched by points) and the curvilinear exchange grid (ogg_xgrid_curv.hip: the source
// cells, searched by the boxes of the model cells): the per-cell record with its box, the choice of cubes, the two touch_kernel passes
// that register every cell in every cube its box touches, and the large-cells list.
//
// A record is BOX_NF doubles: twelve that are the owner's (both owners keep the four edge normals there), the box's lower corner at
// BOX_LO and its upper corner at BOX_HI.  A cell that holds no point has an empty box (lo = +inf, hi = -inf) and is never registered.
// p in a cell's box implies cube_of(lo) <= cube_of(p) <= cube_of(hi) on every axis (cube_of is monotone), so the cubes a box touches
// together with the large list hold every cell whose box contains p.
#pragma once
#include <algorithm>
#include <cmath>

#include "ogg_blocks.h"
#include "ogg_common.h"
#include "ogg_sphere_bins.h"

#pragma clang fp contract(off)

namespace {

constexpr int BOX_NF = 18;                  // doubles of a cell record: four edge normals, box lo, box hi
constexpr int BOX_LO = 12, BOX_HI = 15;
constexpr long BOX_HEAD = 256;
constexpr long BOX_NBMAX = (long)OGG_LOCATE_MAX_CUBES * OGG_LOCATE_MAX_CUBES * OGG_LOCATE_MAX_CUBES;
constexpr double BOX_PAD0 = 9.094947017729282e-13;  // 2^-40

struct BoxHead {
    long long total;                    // the last scan's total (unused with TAIL scans)
    long long nlarge;                   // cells on the large list
    long long G;                        // cubes per axis of the index in use
    long long magic;                    // the owner's magic + G once the index is built
};
static_assert(sizeof(BoxHead) <= BOX_HEAD, "workspace head");

// the padded box of a cell's four corner vectors: lo into r[BOX_LO ..], hi into r[BOX_HI ..]
__device__ inline void padded_box(const double (&q)[4][3], double* r) {
    double L2 = 0.0;
    for (int v = 0; v < 4; ++v)
        for (int w = v + 1; w < 4; ++w) L2 = fmax(L2, dist2(q[v][0], q[v][1], q[v][2], q[w][0], q[w][1], q[w][2]));
    const double pad = 0.25 * L2 + BOX_PAD0;
    for (int a = 0; a < 3; ++a) {
        r[BOX_LO + a] = fmin(fmin(q[0][a], q[1][a]), fmin(q[2][a], q[3][a])) - pad;
        r[BOX_HI + a] = fmax(fmax(q[0][a], q[1][a]), fmax(q[2][a], q[3][a])) + pad;
    }
}

__device__ inline void empty_box(double* r) {
    for (int a = 0; a < 3; ++a) r[BOX_LO + a] = INFINITY, r[BOX_HI + a] = -INFINITY;
}

// cubes per axis for nc cells when no knob fixes it: about eight cells across a cube
inline int box_default_cubes(long nc) {
    return (int)std::min<long>(std::max<long>((long)ceil(sqrt((double)nc) / 8.0), 1), OGG_LOCATE_MAX_CUBES);
}

// FILL = false: the cubes' counts and the large list; FILL = true: the entries (cnt holds the cursors), and the index's head with the
// two counts of the owner's counts struct
template <bool FILL>
__global__ __launch_bounds__(BLOCKS_NT) void touch_kernel(long n, const double* __restrict__ rec, int G, int brute, BoxHead* head,
                                                          long long magic, int* __restrict__ cnt, const int* __restrict__ start,
                                                          int* __restrict__ entries, int* __restrict__ large, long long* out_large,
                                                          long long* out_cubes) {
    for (long c = (long)blockIdx.x * BLOCKS_NT + threadIdx.x; c < n; c += (long)gridDim.x * BLOCKS_NT) {
        const double* r = rec + c * BOX_NF;
        if (!(r[BOX_LO] <= r[BOX_HI])) continue;   // holds no point
        int b0[3], b1[3];
        for (int a = 0; a < 3; ++a) b0[a] = cube_of(r[BOX_LO + a], G), b1[a] = cube_of(r[BOX_HI + a], G);
        const long touch = (long)(b1[0] - b0[0] + 1) * (b1[1] - b0[1] + 1) * (b1[2] - b0[2] + 1);
        if (brute || touch > OGG_LOCATE_MAX_TOUCH) {
            if (!FILL) large[atomicAdd(ull(&head->nlarge), 1ull)] = (int)c;
            continue;
        }
        for (int kz = b0[2]; kz <= b1[2]; ++kz)
            for (int ky = b0[1]; ky <= b1[1]; ++ky)
                for (int kx = b0[0]; kx <= b1[0]; ++kx) {
                    const int b = kx + G * (ky + G * kz);
                    if (FILL)
                        entries[(long)start[b] + atomicAdd(&cnt[b], 1)] = (int)c;
                    else
                        atomicAdd(&cnt[b], 1);
                }
    }
    if (FILL && blockIdx.x == 0 && threadIdx.x == 0) {   // the count pass, an earlier launch, has finished the large list
        head->G = G;
        head->magic = magic + G;
        *out_large = head->nlarge;
        *out_cubes = brute ? 0 : G;
    }
}

// the sections of an index over nc cells inside a workspace
struct BoxIndexLayout {
    long cnt, start, entries, large;
};

inline BoxIndexLayout box_index_sections(ogg::Sections& s, long nc) {
    BoxIndexLayout l;
    l.cnt = s.take((BOX_NBMAX + 1) * 4);
    l.start = s.take((BOX_NBMAX + 1) * 4);
    l.entries = s.take(nc * OGG_LOCATE_MAX_TOUCH * 4);
    l.large = s.take(nc * 4);
    return l;
}

// the index of the nc records rec with G cubes per axis (brute: G = 1 and every cell that holds a point on the large list); bsum: the
// scan's scratch, (BOX_NBMAX + 1) / SCAN_CH + 2 words
inline int build_box_index(long nc, const double* rec, int G, int brute, BoxHead* head, long long magic, void* ws, const BoxIndexLayout& l,
                           long long* bsum, long long* out_large, long long* out_cubes, hipStream_t st) {
    const long nb = (long)G * G * G;
    int *cnt = ogg::at<int>(ws, l.cnt), *start = ogg::at<int>(ws, l.start), *entries = ogg::at<int>(ws, l.entries);
    int* large = ogg::at<int>(ws, l.large);
    OGG_HIP_CHECK(hipMemsetAsync(head, 0, BOX_HEAD, st));
    OGG_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)(nb + 1) * 4, st));
    touch_kernel<false><<<ogg::grid_for<BLOCKS_NT>(nc, 4096), BLOCKS_NT, 0, st>>>(nc, rec, G, brute, head, magic, cnt, start, entries, large,
                                                                                  out_large, out_cubes);
    OGG_LAUNCH_CHECK();
    if (int e = exclusive_scan<true>(cnt, nb, bsum, &head->total, start, st)) return e;
    OGG_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)(nb + 1) * 4, st));   // the cursors of the fill
    touch_kernel<true><<<ogg::grid_for<BLOCKS_NT>(nc, 4096), BLOCKS_NT, 0, st>>>(nc, rec, G, brute, head, magic, cnt, start, entries, large,
                                                                                 out_large, out_cubes);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

}  // namespace
