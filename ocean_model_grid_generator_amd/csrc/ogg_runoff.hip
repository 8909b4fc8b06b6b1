// Runoff mapping (include/ogg_hip.h, "Runoff mapping"): every mapped source cell of a lat-lon runoff field to its nearest target
// cell of the model grid, then a per-cell, in-order sum of the discharge.
//
// targets / sources   one flag byte per cell (target) or per source cell (mapped), then an ordered compaction: a block count over
//                     2048 items, one exclusive scan of the block counts, a block scan that writes each flagged item's slot.  The
//                     lists come out in ascending index with their unit vectors (and A_s for the sources).
// search              one thread per mapped source.  The index is a uniform grid of G^3 cubes of side h = 2 / G over [-1, 1]^3,
//                     filled by an atomic counting sort: chordal distance is 3-D Euclidean distance, so the distance from a point
//                     to a cube is an exact lower bound with no pole or seam case.  Shells of cubes at Chebyshev distance k = 0, 1,
//                     .. are visited outward, skipping cubes that miss the unit sphere or lie farther than the best so far; after
//                     shell k every unvisited target is at least k h away, and the walk stops when (k h)^2 > best (1 + 1e-12), a
//                     margin that covers the rounding of a computed d2.  The best is kept as the key (d2 bits, cell), so the order
//                     in which targets are met does not matter.  OGG_RUNOFF_BRUTE=1 tests every target instead (LDS tiles).
// segments            keys (target cell << 32 | source position) sorted by a rank sort of 256 keys in LDS and merge passes whose
//                     slots come from a binary search in the partner run (the keys are unique); a boundary pass gives every
//                     cell its [start, end) in the sorted keys, in ascending source order because the positions ascend.
// accumulate          one wavefront per 64 consecutive cells of a model row looping over the records (remap_kernel's shape): a
//                     cell of at most REG sources keeps their offsets and areas in registers, a cell of more than LONG sources is
//                     walked by the whole wavefront with the products taken in order by shuffles.  Almost every store is +0.0.
//
// Every result is a fixed function of the unit vectors, the source and the order of the source index: nothing depends on the launch
// geometry or on the order in which the atomics land.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ogg_blocks.h"
#include "ogg_cells.h"
#include "ogg_common.h"
#include "ogg_keysort.h"
#include "ogg_sphere_bins.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int NT = 256;                 // threads per workgroup (four wavefronts)
constexpr int REG = 8;                  // sources a lane keeps in registers across records
constexpr int LONG_N = 32;              // cells with more sources are walked by the whole wavefront
constexpr long HEAD = 256;
constexpr double D = SPHERE_D;
constexpr double PAD = 1e-9;            // cubes widened by this much: covers the rounding of a point's cube index

static_assert(sizeof(ogg_runoff_params) == 80, "ogg_runoff_params layout");
static_assert(sizeof(ogg_runoff_counts) == 64, "ogg_runoff_counts layout");
static_assert(NT == BLOCKS_NT, "block_add and block_scan work over a workgroup of BLOCKS_NT threads");
static_assert(NT == KEYSORT_NT, "the block sort makes the runs the merge passes take");

struct Head {
    long long total;                    // the last scan's total
};
static_assert(sizeof(Head) <= HEAD, "workspace head");

// ---- targets -------------------------------------------------------------------------------------------------------
struct Cells {
    CellTopo t;
    int coast;
};

__global__ __launch_bounds__(NT) void target_flag_kernel(Cells g, const unsigned char* __restrict__ wet, unsigned char* __restrict__ flag,
                                                         ogg_runoff_counts* counts) {
    const long n = g.t.ny * g.t.nx;
    long long v[1] = {0};
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        unsigned char t = 0;
        if (wet[c]) {
            if (!g.coast) {
                t = 1;
            } else {   // a neighbour that does not exist is land: the grid's edge is a coast
                long nb[4];
                face_neighbours(g.t, c, nb);
                t = (nb[0] < 0 || !wet[nb[0]] || nb[1] < 0 || !wet[nb[1]] || nb[2] < 0 || !wet[nb[2]] || nb[3] < 0 || !wet[nb[3]]) ? 1 : 0;
            }
        }
        flag[c] = t;
        v[0] += t;
    }
    long long* const dst[1] = {&counts->targets};
    block_add<1>(v, dst);
}

__global__ __launch_bounds__(NT) void target_list_kernel(long ny, long nx, const unsigned char* __restrict__ flag, const int* __restrict__ pos,
                                                         const double* __restrict__ x, const double* __restrict__ y, long ld,
                                                         int* __restrict__ cell, double* __restrict__ u) {
    const long n = ny * nx;
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        if (!flag[c]) continue;
        const long q = pos[c];
        double v[3];
        centre_unit(x, y, c, nx, ld, v);
        cell[q] = (int)c;
        u[3 * q] = v[0];
        u[3 * q + 1] = v[1];
        u[3 * q + 2] = v[2];
    }
}

// ---- sources -------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void source_flag_kernel(const T* __restrict__ f, long nsrc, long nrec, int nf, double fill0, double fill1,
                                                         unsigned char* __restrict__ flag, ogg_runoff_counts* counts) {
    const T f0 = static_cast<T>(fill0), f1 = static_cast<T>(fill1);
    long long v[3] = {0, 0, 0};
    for (long s = (long)blockIdx.x * NT + threadIdx.x; s < nsrc; s += (long)gridDim.x * NT) {
        bool any = false, nz = false;
        for (long r = 0; r < nrec; ++r) {
            const T x = f[r * nsrc + s];
            if (!missing(x, f0, f1, nf)) {
                any = true;
                nz = nz || x != T(0);
            }
        }
        flag[s] = nz ? 1 : 0;
        v[0] += nz;
        v[1] += any && !nz;
        v[2] += !any;
    }
    long long* const dst[3] = {&counts->mapped, &counts->skipped, &counts->missing};
    block_add<3>(v, dst);
}

__global__ __launch_bounds__(NT) void source_ds_kernel(const double* __restrict__ lat, long NB, double* __restrict__ ds) {
    for (long J = (long)blockIdx.x * NT + threadIdx.x; J < NB; J += (long)gridDim.x * NT) {
        const double b1 = lat[J] * D, b2 = lat[J + 1] * D;
        ds[J] = 2.0 * cos((b1 + b2) / 2.0) * sin((b2 - b1) / 2.0);
    }
}

__global__ __launch_bounds__(NT) void source_list_kernel(long NA, long NB, const unsigned char* __restrict__ flag, const int* __restrict__ pos,
                                                         const double* __restrict__ lon, const double* __restrict__ lat,
                                                         const double* __restrict__ ds, double Re, int* __restrict__ cell,
                                                         double* __restrict__ u, double* __restrict__ As) {
    const long n = NA * NB;
    for (long s = (long)blockIdx.x * NT + threadIdx.x; s < n; s += (long)gridDim.x * NT) {
        if (!flag[s]) continue;
        const long J = s / NA, I = s % NA;
        const long q = pos[s];
        double v[3];
        unit((lon[I] + lon[I + 1]) / 2.0, (lat[J] + lat[J + 1]) / 2.0, v);
        cell[q] = (int)s;
        u[3 * q] = v[0];
        u[3 * q + 1] = v[1];
        u[3 * q + 2] = v[2];
        As[q] = (Re * Re) * (lon[I + 1] * D - lon[I] * D) * ds[J];
    }
}

// ---- search --------------------------------------------------------------------------------------------------------
struct Index {
    int G;
    double h;
    const int* start;   // G^3 + 1
    const double* bu;
    const int* bc;
};

// the targets of cube (a, b, c) against the point (px, py, pz), unless the cube misses the sphere or lies beyond the best
__device__ inline void visit(const Index& ix, int a, int b, int c, double px, double py, double pz, Nearest& best,
                             long long& tests) {
    const double lx = -1.0 + a * ix.h - PAD, hx = -1.0 + (a + 1) * ix.h + PAD;
    const double ly = -1.0 + b * ix.h - PAD, hy = -1.0 + (b + 1) * ix.h + PAD;
    const double lz = -1.0 + c * ix.h - PAD, hz = -1.0 + (c + 1) * ix.h + PAD;
    const double ox = lx > 0.0 ? lx : (hx < 0.0 ? -hx : 0.0), oy = ly > 0.0 ? ly : (hy < 0.0 ? -hy : 0.0),
                 oz = lz > 0.0 ? lz : (hz < 0.0 ? -hz : 0.0);
    const double fx = fmax(lx * lx, hx * hx), fy = fmax(ly * ly, hy * hy), fz = fmax(lz * lz, hz * hz);
    if ((ox * ox + oy * oy) + oz * oz > 1.0 + 1e-6 || (fx + fy) + fz < 1.0 - 1e-6) return;   // misses the unit sphere
    const double gx = lx > px ? lx - px : (px > hx ? px - hx : 0.0), gy = ly > py ? ly - py : (py > hy ? py - hy : 0.0),
                 gz = lz > pz ? lz - pz : (pz > hz ? pz - hz : 0.0);
    if (best.beyond((gx * gx + gy * gy) + gz * gz)) return;
    const int cube = a + ix.G * (b + ix.G * c);
    const int s0 = ix.start[cube], s1 = ix.start[cube + 1];
    for (int t = s0; t < s1; ++t)
        best.offer(bits_of(dist2(px, py, pz, ix.bu[3 * t], ix.bu[3 * t + 1], ix.bu[3 * t + 2])), ix.bc[t]);
    tests += s1 - s0;
}

__global__ __launch_bounds__(NT) void search_kernel(Index ix, const double* __restrict__ su, long n, int* __restrict__ tgt,
                                                    double* __restrict__ d2, ogg_runoff_counts* counts) {
    long long v[1] = {0};
    for (long s = (long)blockIdx.x * NT + threadIdx.x; s < n; s += (long)gridDim.x * NT) {
        const double px = su[3 * s], py = su[3 * s + 1], pz = su[3 * s + 2];
        const int ca = cube_of(px, ix.G), cb = cube_of(py, ix.G), cc = cube_of(pz, ix.G);
        Nearest best{ULLONG_MAX, INT_MAX};
        long long tests = 0;
        for (int k = 0; k <= ix.G; ++k) {
            for (int da = -k; da <= k; ++da) {
                const int a = ca + da;
                if (a < 0 || a >= ix.G) continue;
                for (int db = -k; db <= k; ++db) {
                    const int b = cb + db;
                    if (b < 0 || b >= ix.G) continue;
                    const bool rim = da == -k || da == k || db == -k || db == k;
                    const int step = rim ? 1 : (k > 0 ? 2 * k : 1);
                    for (int dc = -k; dc <= k; dc += step) {
                        const int c = cc + dc;
                        if (c >= 0 && c < ix.G) visit(ix, a, b, c, px, py, pz, best, tests);
                    }
                }
            }
            const double lb = k * ix.h - 2.0 * PAD;   // every target not yet visited is at least this far
            if (lb > 0.0 && best.beyond(lb * lb)) break;
        }
        tgt[s] = best.cell;
        d2[s] = best.d2();
        v[0] += tests;
    }
    long long* const dst[1] = {&counts->tests};
    block_add<1>(v, dst);
}

// every target for every source, tiles of NT targets through LDS
__global__ __launch_bounds__(NT) void brute_kernel(const int* __restrict__ cell, const double* __restrict__ tu, long nt,
                                                   const double* __restrict__ su, long n, int* __restrict__ tgt, double* __restrict__ d2,
                                                   ogg_runoff_counts* counts) {
    __shared__ double lu[3][NT];
    __shared__ int lc[NT];
    const long s = (long)blockIdx.x * NT + threadIdx.x;
    const bool act = s < n;
    const double px = act ? su[3 * s] : 0.0, py = act ? su[3 * s + 1] : 0.0, pz = act ? su[3 * s + 2] : 0.0;
    Nearest best{ULLONG_MAX, INT_MAX};
    for (long base = 0; base < nt; base += NT) {
        const long t = base + threadIdx.x;
        if (t < nt) {
            lu[0][threadIdx.x] = tu[3 * t];
            lu[1][threadIdx.x] = tu[3 * t + 1];
            lu[2][threadIdx.x] = tu[3 * t + 2];
            lc[threadIdx.x] = cell[t];
        }
        __syncthreads();
        const int m = nt - base < NT ? (int)(nt - base) : NT;
        for (int k = 0; k < m; ++k) best.offer(bits_of(dist2(px, py, pz, lu[0][k], lu[1][k], lu[2][k])), lc[k]);
        __syncthreads();
    }
    long long v[1] = {act ? (long long)nt : 0};
    if (act) {
        tgt[s] = best.cell;
        d2[s] = best.d2();
    }
    long long* const dst[1] = {&counts->tests};
    block_add<1>(v, dst);
}

// the cubes per axis the host chose, into the counts: one thread, in the stream's order
__global__ void bins_kernel(ogg_runoff_counts* __restrict__ counts, long long G) { counts->bins = G; }

// ---- segments ------------------------------------------------------------------------------------------------------
// keys of NT consecutive sources sorted in LDS by rank (the keys are unique)
__global__ __launch_bounds__(NT) void sort_block_kernel(const int* __restrict__ tgt, long n, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long lk[NT];
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    const unsigned long long key = i < n ? ((unsigned long long)(unsigned)tgt[i] << 32) | (unsigned long long)i : ULLONG_MAX;
    lk[threadIdx.x] = key;
    __syncthreads();
    int rank = 0;
    for (int k = 0; k < NT; ++k) rank += lk[k] < key;
    if (i < n) out[(long)blockIdx.x * NT + rank] = key;
}

__global__ __launch_bounds__(NT) void seg_kernel(const unsigned long long* __restrict__ key, long n, long ncell, int2* __restrict__ seg) {
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        const unsigned c = (unsigned)(key[k] >> 32);
        if ((long)c >= ncell) continue;   // no target (refused before the search): never written
        if (k == 0 || (unsigned)(key[k - 1] >> 32) != c) seg[c].x = (int)k;
        if (k + 1 == n || (unsigned)(key[k + 1] >> 32) != c) seg[c].y = (int)(k + 1);
    }
}

// ---- accumulate ----------------------------------------------------------------------------------------------------
struct Geo {
    long ny, nx, nsrc, nrec, lda;
    int n_fill;
    double fill0, fill1;
};

template <typename T>
__global__ __launch_bounds__(NT) void accumulate_kernel(Geo g, const T* __restrict__ f, const int2* __restrict__ seg,
                                                        const unsigned long long* __restrict__ key, const int* __restrict__ src_cell,
                                                        const double* __restrict__ As, const double* __restrict__ area,
                                                        double* __restrict__ out, int* __restrict__ nsrc_out, ogg_runoff_counts* counts) {
    const int lane = threadIdx.x & 63;
    const long tiles = (g.nx + 63) / 64;
    const long wave = (long)blockIdx.x * (NT / 64) + threadIdx.x / 64;
    const long row = wave / tiles, i = (wave % tiles) * 64 + lane;
    const bool inb = row < g.ny && i < g.nx;
    const long c = row * g.nx + i, ncell = g.ny * g.nx;
    const T f0 = static_cast<T>(g.fill0), f1 = static_cast<T>(g.fill1);
    int s = 0, n = 0;
    double Ac = 1.0;
    if (inb) {
        const int2 sg = seg[c];
        s = sg.x;
        n = sg.y - sg.x;
        if (n < 0) n = 0;
        nsrc_out[c] = n;
        if (n > 0) {
            const double* a0 = area + 2 * row * g.lda + 2 * i;
            const double* a1 = a0 + g.lda;
            Ac = (a0[0] + a1[1]) + (a0[1] + a1[0]);
        }
    }
    double ca[REG];
    long co[REG];
#pragma unroll
    for (int t = 0; t < REG; ++t) {
        ca[t] = 0.0;
        co[t] = -1;
        if (t < n && n <= REG) {
            const int q = (int)(key[s + t] & 0xFFFFFFFFull);
            ca[t] = As[q];
            co[t] = src_cell[q];
        }
    }
    const bool is_long = n > LONG_N;
    const unsigned long long longmask = __ballot(is_long);
    for (long r = 0; r < g.nrec; ++r) {
        const T* fr = f + r * g.nsrc;
        double S = 0.0;
        if (n <= REG) {
#pragma unroll
            for (int t = 0; t < REG; ++t) {
                if (co[t] >= 0) {
                    const T v = fr[co[t]];
                    if (!missing(v, f0, f1, g.n_fill)) S += (double)v * ca[t];
                }
            }
        } else if (!is_long) {
            for (int k = s; k < s + n; ++k) {
                const int q = (int)(key[k] & 0xFFFFFFFFull);
                const T v = fr[src_cell[q]];
                if (!missing(v, f0, f1, g.n_fill)) S += (double)v * As[q];
            }
        }
        // the long cells, one after the other, by the whole wavefront (longmask is the same in every lane)
        for (unsigned long long m = longmask; m; m &= m - 1) {
            const int L = __ffsll((long long)m) - 1;
            const int sL = __shfl(s, L, 64), nL = __shfl(n, L, 64);
            double sum = 0.0;
            for (int base = 0; base < nL; base += 64) {
                double p = 0.0;
                int ok = 0;
                if (base + lane < nL) {
                    const int q = (int)(key[sL + base + lane] & 0xFFFFFFFFull);
                    const T v = fr[src_cell[q]];
                    ok = !missing(v, f0, f1, g.n_fill);
                    p = (double)v * As[q];
                }
                const int cnt = nL - base < 64 ? nL - base : 64;
                for (int t = 0; t < cnt; ++t) {
                    const double pt = __shfl(p, t, 64);
                    if (__shfl(ok, t, 64)) sum += pt;
                }
            }
            if (lane == L) S = sum;
        }
        if (inb) out[r * ncell + c] = n > 0 ? S / Ac : 0.0;
    }
    long long mx = inb ? n : 0;
    for (int off = 32; off > 0; off >>= 1) {
        const long long t = __shfl_xor(mx, off, 64);
        mx = t > mx ? t : mx;
    }
    if (lane == 0 && mx > 0) atomicMax(ull(&counts->max_sources), (unsigned long long)mx);
    long long v[1] = {inb && n > 0 ? 1 : 0};
    long long* const dst[1] = {&counts->cells};
    block_add<1>(v, dst);
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_runoff_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "runoff: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "runoff: %ld x %ld cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE(p->NA >= 1 && p->NB >= 1 && p->NA <= (long)INT_MAX && p->NB <= (long)INT_MAX && p->NA * p->NB < (1L << 31), OGG_EARG,
                "runoff: %ld x %ld source cells: NA, NB >= 1 and NA * NB < 2^31", p->NA, p->NB);
    OGG_REQUIRE(p->nrec >= 1 && p->nrec <= (long)INT_MAX && p->nrec * p->ny * p->nx < (1L << 32) && p->nrec * p->NA * p->NB < (1L << 40),
                OGG_EARG, "runoff: %ld records of %ld x %ld cells and %ld x %ld source cells: nrec >= 1, nrec * ny * nx < 2^32 and "
                "nrec * NA * NB < 2^40", p->nrec, p->ny, p->nx, p->NA, p->NB);
    OGG_REQUIRE(p->dtype == OGG_REMAP_FLOAT32 || p->dtype == OGG_REMAP_FLOAT64, OGG_EARG, "runoff: source dtype %d (0: float32, 1: float64)",
                p->dtype);
    OGG_REQUIRE(p->n_fill >= 0 && p->n_fill <= OGG_REMAP_MAX_FILLS, OGG_EARG, "runoff: %d fill values (at most %d)", p->n_fill,
                OGG_REMAP_MAX_FILLS);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "runoff: topology flags %d", p->topology);
    OGG_REQUIRE(p->targets == OGG_RUNOFF_COAST || p->targets == OGG_RUNOFF_WET, OGG_EARG, "runoff: targets %d (0: coast, 1: wet)",
                p->targets);
    OGG_REQUIRE(std::isfinite(p->Re) && p->Re > 0.0, OGG_EARG, "runoff: radius %g", p->Re);
    return OGG_OK;
}

long ncell_of(const ogg_runoff_params& p) { return p.ny * p.nx; }
long nsrc_of(const ogg_runoff_params& p) { return p.NA * p.NB; }
long nitem(const ogg_runoff_params& p) { return std::max(ncell_of(p), nsrc_of(p)); }
long nbins_max() { return (long)OGG_RUNOFF_MAX_BINS * OGG_RUNOFF_MAX_BINS * OGG_RUNOFF_MAX_BINS + 1; }

// workspace: head | flag bytes | positions | block sums | A_s | cube counts | cube starts | cube of target | binned u | binned cells |
// keys (two buffers) | segments
struct Layout {
    long flag, pos, bsum, As, key0, key1, seg, total;
    CubeIndexLayout index;
};

Layout layout(const ogg_runoff_params& p) {
    Layout l;
    const long ni = nitem(p), nc = ncell_of(p), ns = nsrc_of(p), nb = nbins_max();
    ogg::Sections s{HEAD};
    l.flag = s.take(ni);
    l.pos = s.take(ni * 4);
    l.bsum = s.take((std::max(ni, nb) / SCAN_CH + 2) * 8);
    l.As = s.take(ns * 8);
    l.index = cube_index_sections(s, nc, nb);
    l.key0 = s.take(ns * 8);
    l.key1 = s.take(ns * 8);
    l.seg = s.take(nc * 8);
    l.total = s.off;
    return l;
}

}  // namespace

extern "C" long ogg_runoff_workspace_bytes(const ogg_runoff_params* p) {
    if (!p || check_params(p) != OGG_OK) return -1;
    return layout(*p).total;
}

extern "C" int ogg_runoff_check(const ogg_runoff_params* p) { return check_params(p); }

extern "C" int ogg_runoff_targets_dev(const ogg_runoff_params* p, const double* x, const double* y, long ld, const unsigned char* wet,
                                      void* workspace, long workspace_bytes, int* tgt_cell, double* tgt_u, ogg_runoff_counts* counts,
                                      void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_runoff_targets", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(x && y && wet && tgt_cell && tgt_u && counts, OGG_EARG, "ogg_runoff_targets: null x / y / wet / tgt_cell / tgt_u / counts");
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_runoff_targets: row stride %ld < 2 nx + 1", ld);
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    const long nc = ncell_of(*p);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_runoff_counts), st));
    const Cells g{cell_topo(p->ny, p->nx, p->topology), p->targets == OGG_RUNOFF_COAST ? 1 : 0};
    unsigned char* flag = at<unsigned char>(workspace, l.flag);
    int* pos = at<int>(workspace, l.pos);
    target_flag_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(g, wet, flag, counts);
    OGG_LAUNCH_CHECK();
    if (int e = exclusive_scan<false>(flag, nc, at<long long>(workspace, l.bsum), &at<Head>(workspace, 0)->total, pos, st)) return e;
    target_list_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(p->ny, p->nx, flag, pos, x, y, ld, tgt_cell, tgt_u);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_runoff_sources_dev(const ogg_runoff_params* p, const void* f, const double* lon, const double* lat, void* workspace,
                                      long workspace_bytes, int* src_cell, double* src_u, double* ds, ogg_runoff_counts* counts,
                                      void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_runoff_sources", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(f && lon && lat && src_cell && src_u && ds && counts, OGG_EARG,
                "ogg_runoff_sources: null f / lon / lat / src_cell / src_u / ds / counts");
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    const long ns = nsrc_of(*p);
    unsigned char* flag = at<unsigned char>(workspace, l.flag);
    int* pos = at<int>(workspace, l.pos);
    if (p->dtype == OGG_REMAP_FLOAT32)
        source_flag_kernel<float><<<grid_for<NT>(ns, 4096), NT, 0, st>>>(static_cast<const float*>(f), ns, p->nrec, p->n_fill, p->fill[0],
                                                                    p->fill[1], flag, counts);
    else
        source_flag_kernel<double><<<grid_for<NT>(ns, 4096), NT, 0, st>>>(static_cast<const double*>(f), ns, p->nrec, p->n_fill, p->fill[0],
                                                                     p->fill[1], flag, counts);
    OGG_LAUNCH_CHECK();
    source_ds_kernel<<<grid_for<NT>(p->NB, 64), NT, 0, st>>>(lat, p->NB, ds);
    OGG_LAUNCH_CHECK();
    if (int e = exclusive_scan<false>(flag, ns, at<long long>(workspace, l.bsum), &at<Head>(workspace, 0)->total, pos, st)) return e;
    source_list_kernel<<<grid_for<NT>(ns, 4096), NT, 0, st>>>(p->NA, p->NB, flag, pos, lon, lat, ds, p->Re, src_cell, src_u,
                                                          at<double>(workspace, l.As));
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_runoff_search_dev(const ogg_runoff_params* p, const int* tgt_cell, const double* tgt_u, long n_targets, const double* src_u,
                                     long n_mapped, void* workspace, long workspace_bytes, int* src_target, double* src_d2,
                                     ogg_runoff_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_runoff_search", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(n_targets >= 0 && n_targets <= ncell_of(*p) && n_mapped >= 0 && n_mapped <= nsrc_of(*p), OGG_EARG,
                "ogg_runoff_search: %ld targets of %ld cells, %ld mapped of %ld source cells", n_targets, ncell_of(*p), n_mapped,
                nsrc_of(*p));
    OGG_REQUIRE(n_targets > 0 || n_mapped == 0, OGG_EARG,
                "runoff: no target cell (no wet cell%s) while %ld source cells hold runoff", p->targets == OGG_RUNOFF_COAST ? " on a coast" : "",
                n_mapped);
    OGG_REQUIRE(counts && ((tgt_cell && tgt_u) || n_targets == 0) && ((src_u && src_target && src_d2) || n_mapped == 0), OGG_EARG,
                "ogg_runoff_search: null tgt_cell / tgt_u / src_u / src_target / src_d2 / counts");
    int brute = 0, bins = 0;
    if (int e = knob("OGG_RUNOFF_BRUTE", 0, 0, 1, &brute)) return e;
    if (int e = knob("OGG_RUNOFF_BINS", 0, 0, OGG_RUNOFF_MAX_BINS, &bins)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    long long G = 0;
    if (!brute) G = bins > 0 ? bins : std::min<long>(std::max<long>((long)ceil(sqrt((double)n_targets / 24.0)), 1), OGG_RUNOFF_MAX_BINS);
    bins_kernel<<<1, 1, 0, st>>>(counts, G);   // G as a kernel argument: no copy from this frame, so no wait for the stream
    OGG_LAUNCH_CHECK();
    if (n_mapped == 0) return OGG_OK;
    if (brute) {
        brute_kernel<<<(unsigned)((n_mapped + NT - 1) / NT), NT, 0, st>>>(tgt_cell, tgt_u, n_targets, src_u, n_mapped, src_target, src_d2,
                                                                          counts);
        OGG_LAUNCH_CHECK();
        return OGG_OK;
    }
    const CubeIndex ci = cube_index_at(workspace, l.index);
    if (int e = build_cube_index(tgt_u, tgt_cell, n_targets, (int)G, ci, at<long long>(workspace, l.bsum), &at<Head>(workspace, 0)->total, st))
        return e;
    const Index ix{(int)G, 2.0 / (double)G, ci.start, ci.bu, ci.bc};
    search_kernel<<<grid_for<NT>(n_mapped, 1L << 20), NT, 0, st>>>(ix, src_u, n_mapped, src_target, src_d2, counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_runoff_segments_dev(const ogg_runoff_params* p, const int* src_target, long n_mapped, void* workspace,
                                       long workspace_bytes, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_runoff_segments", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(n_mapped >= 0 && n_mapped <= nsrc_of(*p), OGG_EARG, "ogg_runoff_segments: %ld mapped of %ld source cells", n_mapped,
                nsrc_of(*p));
    OGG_REQUIRE(src_target || n_mapped == 0, OGG_EARG, "ogg_runoff_segments: null src_target");
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    int2* seg = at<int2>(workspace, l.seg);
    OGG_HIP_CHECK(hipMemsetAsync(seg, 0, (size_t)ncell_of(*p) * 8, st));
    if (n_mapped == 0) return OGG_OK;
    unsigned long long* buf[2] = {at<unsigned long long>(workspace, l.key0), at<unsigned long long>(workspace, l.key1)};
    sort_block_kernel<<<(unsigned)((n_mapped + NT - 1) / NT), NT, 0, st>>>(src_target, n_mapped, buf[0]);
    OGG_LAUNCH_CHECK();
    int k = 0;
    for (long w = NT; w < n_mapped; w *= 2, ++k) {
        keysort_merge_kernel<<<grid_for<NT>(n_mapped, 1L << 20), NT, 0, st>>>(buf[k & 1], n_mapped, w, buf[(k + 1) & 1]);
        OGG_LAUNCH_CHECK();
    }
    seg_kernel<<<grid_for<NT>(n_mapped, 1L << 20), NT, 0, st>>>(buf[k & 1], n_mapped, ncell_of(*p), seg);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_runoff_accumulate_dev(const ogg_runoff_params* p, const void* f, const int* src_cell, long n_mapped, const double* area,
                                         long lda, const void* workspace, long workspace_bytes, double* values, int* n_sources,
                                         ogg_runoff_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_runoff_accumulate", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(n_mapped >= 0 && n_mapped <= nsrc_of(*p), OGG_EARG, "ogg_runoff_accumulate: %ld mapped of %ld source cells", n_mapped,
                nsrc_of(*p));
    OGG_REQUIRE(f && area && values && n_sources && counts && (src_cell || n_mapped == 0), OGG_EARG,
                "ogg_runoff_accumulate: null f / src_cell / area / values / n_sources / counts");
    OGG_REQUIRE(lda >= 2 * p->nx, OGG_EARG, "ogg_runoff_accumulate: area row stride %ld < 2 nx", lda);
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    const unsigned long long* key = at<unsigned long long>(workspace, (keysort_passes(n_mapped) & 1) ? l.key1 : l.key0);
    const Geo g{p->ny, p->nx, nsrc_of(*p), p->nrec, lda, p->n_fill, p->fill[0], p->fill[1]};
    const long waves = p->ny * ((p->nx + 63) / 64);
    const unsigned grid = (unsigned)((waves + NT / 64 - 1) / (NT / 64));
    const int2* seg = at<int2>(workspace, l.seg);
    const double* As = at<double>(workspace, l.As);
    if (p->dtype == OGG_REMAP_FLOAT32)
        accumulate_kernel<float><<<grid, NT, 0, st>>>(g, static_cast<const float*>(f), seg, key, src_cell, As, area, values, n_sources, counts);
    else
        accumulate_kernel<double><<<grid, NT, 0, st>>>(g, static_cast<const double*>(f), seg, key, src_cell, As, area, values, n_sources,
                                                       counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: everything copied to device memory, the five steps, the results copied back (synchronous)
extern "C" int ogg_runoff(const ogg_runoff_params* p, const double* x, const double* y, const double* area, const unsigned char* wet,
                          const void* f, const double* lon, const double* lat, double* values, int* n_sources, int* src_cell, int* src_target,
                          double* src_d2, ogg_runoff_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(x && y && area && wet && f && lon && lat && values && n_sources && src_cell && src_target && src_d2 && counts, OGG_EARG,
                "ogg_runoff: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t nc = (size_t)ncell_of(*p), ns = (size_t)nsrc_of(*p), npt = (size_t)(2 * p->ny + 1) * (2 * p->nx + 1);
    const size_t fbytes = (size_t)p->nrec * ns * (p->dtype == OGG_REMAP_FLOAT32 ? 4 : 8);
    const long wsb = layout(*p).total;
    double *dx, *dy, *da, *dlon, *dlat, *tu, *su, *sds, *sd, *dv;
    unsigned char* dw;
    char *df, *ws;
    int *tc, *sc, *st, *dn;
    ogg_runoff_counts* ct;
    if (int e = bufs.alloc(&dx, npt)) return e;
    if (int e = bufs.alloc(&dy, npt)) return e;
    if (int e = bufs.alloc(&da, nc * 4)) return e;
    if (int e = bufs.alloc(&dw, nc)) return e;
    if (int e = bufs.alloc(&df, fbytes)) return e;
    if (int e = bufs.alloc(&dlon, (size_t)p->NA + 1)) return e;
    if (int e = bufs.alloc(&dlat, (size_t)p->NB + 1)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&tc, nc)) return e;
    if (int e = bufs.alloc(&tu, nc * 3)) return e;
    if (int e = bufs.alloc(&sc, ns)) return e;
    if (int e = bufs.alloc(&su, ns * 3)) return e;
    if (int e = bufs.alloc(&sds, (size_t)p->NB)) return e;
    if (int e = bufs.alloc(&st, ns)) return e;
    if (int e = bufs.alloc(&sd, ns)) return e;
    if (int e = bufs.alloc(&dv, (size_t)p->nrec * nc)) return e;
    if (int e = bufs.alloc(&dn, nc)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = bufs.send(dx, x, npt)) return e;
    if (int e = bufs.send(dy, y, npt)) return e;
    if (int e = bufs.send(da, area, nc * 4)) return e;
    if (int e = bufs.send(dw, wet, nc)) return e;
    if (int e = bufs.send(df, static_cast<const char*>(f), fbytes)) return e;
    if (int e = bufs.send(dlon, lon, (size_t)p->NA + 1)) return e;
    if (int e = bufs.send(dlat, lat, (size_t)p->NB + 1)) return e;
    if (int e = ogg_runoff_targets_dev(p, dx, dy, 2 * p->nx + 1, dw, ws, wsb, tc, tu, ct, nullptr)) return e;
    if (int e = ogg_runoff_sources_dev(p, df, dlon, dlat, ws, wsb, sc, su, sds, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    const long nt = (long)counts->targets, nm = (long)counts->mapped;
    if (int e = ogg_runoff_search_dev(p, tc, tu, nt, su, nm, ws, wsb, st, sd, ct, nullptr)) return e;
    if (int e = ogg_runoff_segments_dev(p, st, nm, ws, wsb, nullptr)) return e;
    if (int e = ogg_runoff_accumulate_dev(p, df, sc, nm, da, 2 * p->nx, ws, wsb, dv, dn, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(values, dv, (size_t)p->nrec * nc)) return e;
    if (int e = bufs.get(n_sources, dn, nc)) return e;
    if (nm > 0) {
        if (int e = bufs.get(src_cell, sc, (size_t)nm)) return e;
        if (int e = bufs.get(src_target, st, (size_t)nm)) return e;
        if (int e = bufs.get(src_d2, sd, (size_t)nm)) return e;
    }
    return OGG_OK;
}
