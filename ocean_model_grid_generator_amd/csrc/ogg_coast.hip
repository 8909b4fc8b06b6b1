// Distance to the coast (include/ogg_hip.h, "Distance to the coast"): for every valid wet cell the nearest coastal land cell, for
// every valid land cell the nearest coastal wet cell, by the runoff mapping's key (d2 bits, cell).
//
// sets      one flag byte (wet, coastal, valid) and the unit vector of every cell, then the two coastal lists by the ordered
//           compaction of ogg_blocks.h (a membership byte, one exclusive scan, a list kernel), as the runoff targets step.
// search    every cell is a query, and index-space neighbours are usually neighbours on the sphere, so one workgroup takes a tile of
//           TY x TX cells and does the pruning once for all of them.  The targets are sorted into G^3 cubes (ogg_sphere_bins.h); a
//           coastline is one-dimensional, so only the non-empty cubes are kept, as a compact list in ascending cube order with the
//           TIGHT box of each cube's contents (the exact minimum and maximum of the coordinates held: no rounding enters a box).
//           The tile's queries lie in a ball: centre m (the middle of their bounding box), radius r (the largest |p - m|).
//             pass 1   U = min over the listed cubes of maxdist(m, box): some target t has |m - t| <= U.
//             pass 2   every cube with mindist(m, box) <= U + 2 r is streamed through LDS in chunks, and every lane tests every
//                      candidate with the key, as the runoff's brute_kernel does.
//           Why that is enough: for a query p of the tile and its nearest target t*, |p - t*| <= |p - t| <= r + U, so
//           |m - t*| <= 2 r + U, and the box of t*'s cube is at most that far from m; the same holds for every target tied with t*.
//           Chordal distance is Euclidean distance in 3-D, so the triangle inequality has no pole or seam case.  A tile that
//           straddles the seam or the fold, or holds scattered centres, has a large ball and tests (nearly) everything: slower, as exact.
//           A lane skips a cube whose box is farther from its own p than its best so far.
//           Rounding: a difference of two doubles, a product and a square root are each correctly rounded, so every computed
//           distance is within a few 2^-53 of its value RELATIVELY, however small; MARGIN = 1 + 1e-12 (ogg_sphere.h) on every
//           comparison of two computed distances covers that a million times over.
// OGG_COAST_BRUTE=1 streams the whole target list through every tile instead (no index, no pruning): the cross-check.
//
// nearest and d2 are a function of the unit vectors and the wet bytes alone: the key makes the order in which targets are met
// immaterial, and tiles, cubes and chunks only decide which targets are never looked at, all of them strictly farther.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "ogg_blocks.h"
#include "ogg_cells.h"
#include "ogg_common.h"
#include "ogg_sphere_bins.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int NT = 256;                 // threads per workgroup (four wavefronts)
constexpr int MAX_CHUNK = 512;          // the largest OGG_COAST_CHUNK: targets of one LDS chunk
constexpr long HEAD = 256;
constexpr int F_WET = 1, F_COAST = 2, F_VALID = 4;

static_assert(sizeof(ogg_coast_params) == 24, "ogg_coast_params layout");
static_assert(sizeof(ogg_coast_counts) == 56, "ogg_coast_counts layout");
static_assert(NT == BLOCKS_NT, "block_add and block_scan work over a workgroup of BLOCKS_NT threads");

struct Head {
    long long total;                    // the last scan's total
    long long ncubes;                   // non-empty cubes of the index in use
};
static_assert(sizeof(Head) <= HEAD, "workspace head");

// ---- sets ----------------------------------------------------------------------------------------------------------
struct Cells {
    CellTopo t;
    int sides;
};

__global__ __launch_bounds__(NT) void flag_kernel(Cells g, const double* __restrict__ x, const double* __restrict__ y, long ld,
                                                  const unsigned char* __restrict__ wet, unsigned char* __restrict__ flags,
                                                  double* __restrict__ u, ogg_coast_counts* counts) {
    const long n = g.t.ny * g.t.nx;
    long long v[3] = {0, 0, 0};
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const long k = centre_point(c, g.t.nx, ld);
        const double lon = x[k], lat = y[k];
        const bool valid = isfinite(lon) && isfinite(lat);
        const bool w = wet[c] != 0;
        // a neighbour that does not exist is not a neighbour: the grid's edge is no coast
        long nb[4];
        face_neighbours(g.t, c, nb);
        const bool coast = (nb[0] >= 0 && (wet[nb[0]] != 0) != w) || (nb[1] >= 0 && (wet[nb[1]] != 0) != w) ||
                           (nb[2] >= 0 && (wet[nb[2]] != 0) != w) || (nb[3] >= 0 && (wet[nb[3]] != 0) != w);
        flags[c] = (unsigned char)((w ? F_WET : 0) | (coast ? F_COAST : 0) | (valid ? F_VALID : 0));
        double t[3];
        unit(lon, lat, t);
        u[3 * c] = t[0];
        u[3 * c + 1] = t[1];
        u[3 * c + 2] = t[2];
        v[0] += valid && coast && w;
        v[1] += valid && coast && !w;
        v[2] += valid && (g.sides & (w ? OGG_COAST_WET : OGG_COAST_LAND)) != 0;
    }
    long long* const dst[3] = {&counts->coast_wet, &counts->coast_land, &counts->queries};
    block_add<3>(v, dst);
}

// member[c] = 1 for the valid coastal cells whose wet bit is ``w``
__global__ __launch_bounds__(NT) void member_kernel(const unsigned char* __restrict__ flags, long n, int w, unsigned char* __restrict__ member) {
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT)
        member[c] = (flags[c] & (F_COAST | F_VALID)) == (F_COAST | F_VALID) && (flags[c] & F_WET) == w ? 1 : 0;
}

__global__ __launch_bounds__(NT) void list_kernel(const unsigned char* __restrict__ member, const int* __restrict__ pos, long n,
                                                  const double* __restrict__ u, int* __restrict__ cell, double* __restrict__ lu) {
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        if (!member[c]) continue;
        const long q = pos[c];
        cell[q] = (int)c;
        lu[3 * q] = u[3 * c];
        lu[3 * q + 1] = u[3 * c + 1];
        lu[3 * q + 2] = u[3 * c + 2];
    }
}

// ---- index ---------------------------------------------------------------------------------------------------------
// ne[b] = 1 for the cubes that hold a target (start: G^3 + 1 entries)
__global__ __launch_bounds__(NT) void nonempty_kernel(const int* __restrict__ start, long nb, unsigned char* __restrict__ ne) {
    for (long b = (long)blockIdx.x * NT + threadIdx.x; b < nb; b += (long)gridDim.x * NT) ne[b] = start[b + 1] > start[b] ? 1 : 0;
}

// the compact list: for the k-th non-empty cube (ascending cube order) its range of binned targets
__global__ __launch_bounds__(NT) void cube_list_kernel(const int* __restrict__ start, const unsigned char* __restrict__ ne,
                                                       const int* __restrict__ cpos, long nb, int2* __restrict__ range, Head* head) {
    for (long b = (long)blockIdx.x * NT + threadIdx.x; b < nb; b += (long)gridDim.x * NT)
        if (ne[b]) range[cpos[b]] = make_int2(start[b], start[b + 1]);
    if (blockIdx.x == 0 && threadIdx.x == 0) head->ncubes = head->total;
}

// the tight box of every listed cube, one wavefront per cube: box[6 k ..] = min x, y, z, max x, y, z of its targets (exact)
__global__ __launch_bounds__(NT) void cube_box_kernel(const Head* head, const int2* __restrict__ range, const double* __restrict__ bu,
                                                      double* __restrict__ box) {
    const int lane = threadIdx.x & 63;
    const long nk = head->ncubes;
    for (long k = (long)blockIdx.x * (NT / 64) + threadIdx.x / 64; k < nk; k += (long)gridDim.x * (NT / 64)) {
        const int2 r = range[k];
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int t = r.x + lane; t < r.y; t += 64)
            for (int a = 0; a < 3; ++a) {
                const double v = bu[3 * (long)t + a];
                lo[a] = fmin(lo[a], v);
                hi[a] = fmax(hi[a], v);
            }
        for (int a = 0; a < 3; ++a)
            for (int off = 32; off > 0; off >>= 1) {
                lo[a] = fmin(lo[a], __shfl_xor(lo[a], off, 64));
                hi[a] = fmax(hi[a], __shfl_xor(hi[a], off, 64));
            }
        if (lane == 0)
            for (int a = 0; a < 3; ++a) box[6 * k + a] = lo[a], box[6 * k + 3 + a] = hi[a];
    }
}

// ---- search --------------------------------------------------------------------------------------------------------
struct Search {
    long ny, nx;
    int TX, TY;                 // the tile: TY x TX cells, thread t takes cell (t / TX, t % TX) of it (TX * TY <= NT)
    int wet;                    // the wet bit of the queries: F_WET (against the coastal land) or 0 (against the coastal wet)
    int chunk;                  // targets per LDS chunk
    int brute;                  // 1: tu / tc is the whole target list and every chunk of it is tested
    long nt;                    // targets
    const Head* head;           // ncubes
    const int2* range;
    const double* box;
    const double* tu;           // the binned targets (brute: the list itself)
    const int* tc;
};

// min of K values over the workgroup, the same in every thread
template <int K>
__device__ inline void block_min(double (&v)[K]) {
    __shared__ double part[NT / 64][K];
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] = fmin(v[k], __shfl_xor(v[k], off, 64));
    __syncthreads();   // part may still be read from an earlier call
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) part[threadIdx.x / 64][k] = v[k];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        double t = part[0][k];
        for (int w = 1; w < NT / 64; ++w) t = fmin(t, part[w][k]);
        v[k] = t;
    }
}

// squared distance from p to the nearest (mind2) and to the farthest (maxd2) point of the box lo .. hi
__device__ inline double mind2(const double* p, const double* lo, const double* hi) {
    double g[3];
    for (int a = 0; a < 3; ++a) g[a] = lo[a] > p[a] ? lo[a] - p[a] : (p[a] > hi[a] ? p[a] - hi[a] : 0.0);
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}
__device__ inline double maxd2(const double* p, const double* lo, const double* hi) {
    double g[3];
    for (int a = 0; a < 3; ++a) g[a] = fmax(fabs(p[a] - lo[a]), fabs(hi[a] - p[a]));
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

struct Chunk {
    double u[3][MAX_CHUNK];
    int c[MAX_CHUNK];
};

// the targets s0 .. s1 of tu / tc through LDS, chunk by chunk; the lanes with ``act`` test every one of them.  Called by the whole
// workgroup with the same s0, s1.
__device__ inline void stream(const Search& s, Chunk& ch, int s0, int s1, bool act, const double* p, Nearest& best,
                              long long& tests) {
    for (int base = s0; base < s1; base += s.chunk) {
        const int m = s1 - base < s.chunk ? s1 - base : s.chunk;
        __syncthreads();   // the chunk before this one has been read
        for (int t = threadIdx.x; t < m; t += NT) {
            const long q = (long)base + t;
            ch.u[0][t] = s.tu[3 * q];
            ch.u[1][t] = s.tu[3 * q + 1];
            ch.u[2][t] = s.tu[3 * q + 2];
            ch.c[t] = s.tc[q];
        }
        __syncthreads();
        if (act) {
            for (int k = 0; k < m; ++k) best.offer(bits_of(dist2(p[0], p[1], p[2], ch.u[0][k], ch.u[1][k], ch.u[2][k])), ch.c[k]);
            tests += m;
        }
    }
}

__global__ __launch_bounds__(NT) void search_kernel(Search s, const unsigned char* __restrict__ flags, const double* __restrict__ u,
                                                    int* __restrict__ nearest, double* __restrict__ d2, ogg_coast_counts* counts) {
    __shared__ Chunk ch;
    __shared__ double qbox[NT][6];      // the boxes and ranges of up to NT candidate cubes
    __shared__ int2 qrange[NT];
    __shared__ int wcount[NT / 64];
    const long tiles_x = (s.nx + s.TX - 1) / s.TX;
    const long tj = blockIdx.x / tiles_x, ti = blockIdx.x % tiles_x;
    const int ty = threadIdx.x / s.TX, tx = threadIdx.x % s.TX;
    const long j = tj * s.TY + ty, i = ti * s.TX + tx;
    const bool inb = ty < s.TY && j < s.ny && i < s.nx;
    const long c = inb ? j * s.nx + i : 0;
    const int f = inb ? flags[c] : 0;
    const bool q = inb && (f & F_VALID) && (f & F_WET) == s.wet;
    if (__syncthreads_count(q) == 0) return;   // no query of this side in the tile
    double p[3] = {0.0, 0.0, 0.0};
    if (q) p[0] = u[3 * c], p[1] = u[3 * c + 1], p[2] = u[3 * c + 2];
    Nearest best{ULLONG_MAX, INT_MAX};
    long long tests = 0;
    if (s.brute) {
        stream(s, ch, 0, (int)s.nt, q, p, best, tests);
    } else {
        // the ball of the tile's queries: m the middle of their bounding box, r2 the largest squared distance from m
        double bb[6];
        for (int a = 0; a < 3; ++a) bb[a] = q ? p[a] : INFINITY, bb[3 + a] = q ? -p[a] : INFINITY;
        block_min<6>(bb);
        const double m[3] = {0.5 * (bb[0] - bb[3]), 0.5 * (bb[1] - bb[4]), 0.5 * (bb[2] - bb[5])};
        double rr[1] = {q ? -dist2(p[0], p[1], p[2], m[0], m[1], m[2]) : 0.0};
        block_min<1>(rr);
        const double r = sqrt(-rr[0]);
        // pass 1: some target is no farther from m than U
        const long nk = s.head->ncubes;
        double uu[1] = {INFINITY};
        for (long k = threadIdx.x; k < nk; k += NT) uu[0] = fmin(uu[0], maxd2(m, s.box + 6 * k, s.box + 6 * k + 3));
        block_min<1>(uu);
        const double T = (sqrt(uu[0]) + 2.0 * r) * MARGIN, T2 = (T * T) * MARGIN;
        // pass 2: the cubes within T of m, NT cubes of the list at a time, compacted in list order
        const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
        for (long base = 0; base < nk; base += NT) {
            const long k = base + threadIdx.x;
            double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
            bool cand = false;
            if (k < nk) {
                for (int a = 0; a < 3; ++a) lo[a] = s.box[6 * k + a], hi[a] = s.box[6 * k + 3 + a];
                cand = mind2(m, lo, hi) <= T2;
            }
            const unsigned long long bal = __ballot(cand);
            __syncthreads();   // the queue of the round before has been read
            if (lane == 0) wcount[w] = __popcll(bal);
            __syncthreads();
            int off = 0, total = 0;
            for (int v = 0; v < NT / 64; ++v) {
                if (v < w) off += wcount[v];
                total += wcount[v];
            }
            if (cand) {
                const int slot = off + __popcll(bal & ((1ull << lane) - 1ull));
                for (int a = 0; a < 3; ++a) qbox[slot][a] = lo[a], qbox[slot][3 + a] = hi[a];
                qrange[slot] = s.range[k];
            }
            __syncthreads();
            for (int e = 0; e < total; ++e) {
                // a lane leaves out a cube whose box is farther from its own p than its best (strictly: ties are still met)
                bool act = q;
                if (act && best.found()) {
                    double bd;   // read from the key itself, before the box: profiles/nearest_kit_kernel_resources.md
                    memcpy(&bd, &best.bits, 8);
                    act = !(mind2(p, qbox[e], qbox[e] + 3) > bd * MARGIN);
                }
                stream(s, ch, qrange[e].x, qrange[e].y, act, p, best, tests);
            }
        }
    }
    if (q && best.found()) {
        nearest[c] = best.cell;
        d2[c] = best.d2();
    }
    long long v[2] = {q && best.found() ? 1 : 0, tests};
    long long* const dst[2] = {&counts->answered, &counts->tests};
    block_add<2>(v, dst);
}

// nearest = -1 and d2 = +inf everywhere, and the search step's counts from zero
__global__ __launch_bounds__(NT) void init_kernel(long n, int* __restrict__ nearest, double* __restrict__ d2, ogg_coast_counts* counts,
                                                  long long tiles, long long cubes) {
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        nearest[c] = -1;
        d2[c] = INFINITY;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts->answered = 0;
        counts->tests = 0;
        counts->tiles = tiles;
        counts->cubes = cubes;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_coast_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "coast distance: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "coast distance: %ld x %ld cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "coast distance: topology flags %d", p->topology);
    OGG_REQUIRE(p->sides >= 1 && p->sides <= (OGG_COAST_WET | OGG_COAST_LAND), OGG_EARG, "coast distance: sides %d (1: wet, 2: land, 3: both)",
                p->sides);
    return OGG_OK;
}

long ncell_of(const ogg_coast_params& p) { return p.ny * p.nx; }
long nbins_max() { return (long)OGG_COAST_MAX_CUBES * OGG_COAST_MAX_CUBES * OGG_COAST_MAX_CUBES + 1; }

// workspace: head | member / non-empty bytes | positions | block sums | cube counts | cube starts | cube of target | binned u |
// binned cells | cube ranges | cube boxes
struct Layout {
    long flag, pos, bsum, range, box, total;
    CubeIndexLayout index;
};

Layout layout(const ogg_coast_params& p) {
    Layout l;
    const long nc = ncell_of(p), nb = nbins_max(), ni = std::max(nc, nb), nk = std::min(nc, nb);
    ogg::Sections s{HEAD};
    l.flag = s.take(ni);
    l.pos = s.take(ni * 4);
    l.bsum = s.take((ni / SCAN_CH + 2) * 8);
    l.index = cube_index_sections(s, nc, nb);
    l.range = s.take(nk * 8);
    l.box = s.take(nk * 48);
    l.total = s.off;
    return l;
}

struct Knobs {
    int brute, cubes, tx, ty, chunk;
};

int read_knobs(Knobs* k) {
    // OGG_COAST_BRUTE=1: every target for every query (the cross-check of the index)
    if (int e = knob("OGG_COAST_BRUTE", 0, 0, 1, &k->brute)) return e;
    // OGG_COAST_CUBES: cubes per axis of the index; 0: from the cell count, about six cells across a cube
    if (int e = knob("OGG_COAST_CUBES", 0, 0, OGG_COAST_MAX_CUBES, &k->cubes)) return e;
    // OGG_COAST_TILE_X, OGG_COAST_TILE_Y: the cells of a tile along i and j, one thread each (TX * TY <= 256).  A square tile has
    // the smallest ball
    if (int e = knob("OGG_COAST_TILE_X", 16, 1, NT, &k->tx)) return e;
    if (int e = knob("OGG_COAST_TILE_Y", 16, 1, NT, &k->ty)) return e;
    OGG_REQUIRE(k->tx * k->ty <= NT, OGG_EARG, "OGG_COAST_TILE_X=%d, OGG_COAST_TILE_Y=%d: at most %d cells in a tile", k->tx, k->ty, NT);
    // OGG_COAST_CHUNK: targets staged in LDS at a time (a cube of more targets takes several chunks)
    if (int e = knob("OGG_COAST_CHUNK", 256, 1, MAX_CHUNK, &k->chunk)) return e;
    return OGG_OK;
}

// one side of the search: the queries with wet bit ``wet`` against the list tc / tu of nt targets
int search_side(const ogg_coast_params& p, const Knobs& kn, int G, int wet, const int* tc, const double* tu, long nt,
                const unsigned char* flags, const double* u, void* ws, int* nearest, double* d2, ogg_coast_counts* counts, hipStream_t st) {
    if (nt == 0) return OGG_OK;   // an empty opposite set: -1 and +inf stay
    const Layout l = layout(p);
    Head* head = at<Head>(ws, 0);
    Search s{p.ny, p.nx, kn.tx, kn.ty, wet, kn.chunk, kn.brute, nt, head, nullptr, nullptr, tu, tc};
    if (!kn.brute) {
        const long nb = (long)G * G * G;
        const CubeIndex ci = cube_index_at(ws, l.index);
        unsigned char* ne = at<unsigned char>(ws, l.flag);
        int* cpos = at<int>(ws, l.pos);
        int2* range = at<int2>(ws, l.range);
        double* box = at<double>(ws, l.box);
        long long* bsum = at<long long>(ws, l.bsum);
        if (int e = build_cube_index(tu, tc, nt, G, ci, bsum, &head->total, st)) return e;
        nonempty_kernel<<<grid_for<NT>(nb, 4096), NT, 0, st>>>(ci.start, nb, ne);
        OGG_LAUNCH_CHECK();
        if (int e = exclusive_scan<false>(ne, nb, bsum, &head->total, cpos, st)) return e;
        cube_list_kernel<<<grid_for<NT>(nb, 4096), NT, 0, st>>>(ci.start, ne, cpos, nb, range, head);
        OGG_LAUNCH_CHECK();
        cube_box_kernel<<<grid_for<NT / 64>(std::min(nt, nb), 4096), NT, 0, st>>>(head, range, ci.bu, box);
        OGG_LAUNCH_CHECK();
        s.range = range;
        s.box = box;
        s.tu = ci.bu;
        s.tc = ci.bc;
    }
    const long tiles = ((p.ny + kn.ty - 1) / kn.ty) * ((p.nx + kn.tx - 1) / kn.tx);
    search_kernel<<<(unsigned)tiles, NT, 0, st>>>(s, flags, u, nearest, d2, counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

}  // namespace

extern "C" long ogg_coast_workspace_bytes(const ogg_coast_params* p) {
    if (!p || check_params(p) != OGG_OK) return -1;
    return layout(*p).total;
}

extern "C" int ogg_coast_check(const ogg_coast_params* p) { return check_params(p); }

extern "C" int ogg_coast_sets_dev(const ogg_coast_params* p, const double* x, const double* y, long ld, const unsigned char* wet,
                                  void* workspace, long workspace_bytes, unsigned char* flags, double* u, int* land_cell, double* land_u,
                                  int* wet_cell, double* wet_u, ogg_coast_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_coast_sets", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(x && y && wet && flags && u && land_cell && land_u && wet_cell && wet_u && counts, OGG_EARG,
                "ogg_coast_sets: null x / y / wet / flags / u / land_cell / land_u / wet_cell / wet_u / counts");
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_coast_sets: row stride %ld < 2 nx + 1", ld);
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    const long nc = ncell_of(*p);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_coast_counts), st));
    const Cells g{cell_topo(p->ny, p->nx, p->topology), p->sides};
    flag_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(g, x, y, ld, wet, flags, u, counts);
    OGG_LAUNCH_CHECK();
    unsigned char* member = at<unsigned char>(workspace, l.flag);
    int* pos = at<int>(workspace, l.pos);
    for (int w = 0; w < 2; ++w) {   // the coastal land, then the coastal wet
        member_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(flags, nc, w ? F_WET : 0, member);
        OGG_LAUNCH_CHECK();
        if (int e = exclusive_scan<false>(member, nc, at<long long>(workspace, l.bsum), &at<Head>(workspace, 0)->total, pos, st)) return e;
        list_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(member, pos, nc, u, w ? wet_cell : land_cell, w ? wet_u : land_u);
        OGG_LAUNCH_CHECK();
    }
    return OGG_OK;
}

extern "C" int ogg_coast_search_dev(const ogg_coast_params* p, const unsigned char* flags, const double* u, const int* land_cell,
                                    const double* land_u, long n_land, const int* wet_cell, const double* wet_u, long n_wet,
                                    void* workspace, long workspace_bytes, int* nearest, double* d2, ogg_coast_counts* counts,
                                    void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_coast_search", workspace, workspace_bytes, layout(*p).total)) return e;
    const long nc = ncell_of(*p);
    OGG_REQUIRE(n_land >= 0 && n_wet >= 0 && n_land + n_wet <= nc, OGG_EARG, "ogg_coast_search: %ld coastal land and %ld coastal wet of %ld cells",
                n_land, n_wet, nc);
    OGG_REQUIRE(flags && u && nearest && d2 && counts && ((land_cell && land_u) || n_land == 0) && ((wet_cell && wet_u) || n_wet == 0),
                OGG_EARG, "ogg_coast_search: null flags / u / land_cell / land_u / wet_cell / wet_u / nearest / d2 / counts");
    Knobs kn;
    if (int e = read_knobs(&kn)) return e;
    hipStream_t st = ogg::as_stream(stream);
    int G = 0;
    if (!kn.brute)
        G = kn.cubes > 0 ? kn.cubes : (int)std::min<long>(std::max<long>((long)ceil(sqrt((double)nc) / 16.0), 1), OGG_COAST_MAX_CUBES);
    const long tiles = ((p->ny + kn.ty - 1) / kn.ty) * ((p->nx + kn.tx - 1) / kn.tx);
    init_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(nc, nearest, d2, counts, tiles, G);
    OGG_LAUNCH_CHECK();
    if (p->sides & OGG_COAST_WET)
        if (int e = search_side(*p, kn, G, F_WET, land_cell, land_u, n_land, flags, u, workspace, nearest, d2, counts, st)) return e;
    if (p->sides & OGG_COAST_LAND)
        if (int e = search_side(*p, kn, G, 0, wet_cell, wet_u, n_wet, flags, u, workspace, nearest, d2, counts, st)) return e;
    return OGG_OK;
}

// the host-pointer form: everything copied to device memory, the two steps, the results copied back (synchronous)
extern "C" int ogg_coast_distance(const ogg_coast_params* p, const double* x, const double* y, const unsigned char* wet, int* nearest,
                                  double* d2, unsigned char* flags, ogg_coast_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(x && y && wet && nearest && d2 && flags && counts, OGG_EARG, "ogg_coast_distance: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t nc = (size_t)ncell_of(*p), npt = (size_t)(2 * p->ny + 1) * (2 * p->nx + 1);
    const long wsb = layout(*p).total;
    double *dx, *dy, *du, *lu, *wu, *dd;
    unsigned char *dw, *df;
    char* ws;
    int *lc, *wc, *dn;
    ogg_coast_counts* ct;
    if (int e = bufs.put(&dx, x, npt)) return e;
    if (int e = bufs.put(&dy, y, npt)) return e;
    if (int e = bufs.put(&dw, wet, nc)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&df, nc)) return e;
    if (int e = bufs.alloc(&du, nc * 3)) return e;
    if (int e = bufs.alloc(&lc, nc)) return e;
    if (int e = bufs.alloc(&lu, nc * 3)) return e;
    if (int e = bufs.alloc(&wc, nc)) return e;
    if (int e = bufs.alloc(&wu, nc * 3)) return e;
    if (int e = bufs.alloc(&dn, nc)) return e;
    if (int e = bufs.alloc(&dd, nc)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = ogg_coast_sets_dev(p, dx, dy, 2 * p->nx + 1, dw, ws, wsb, df, du, lc, lu, wc, wu, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = ogg_coast_search_dev(p, df, du, lc, lu, (long)counts->coast_land, wc, wu, (long)counts->coast_wet, ws, wsb, dn, dd, ct, nullptr))
        return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(nearest, dn, nc)) return e;
    if (int e = bufs.get(d2, dd, nc)) return e;
    if (int e = bufs.get(flags, df, nc)) return e;
    return OGG_OK;
}
