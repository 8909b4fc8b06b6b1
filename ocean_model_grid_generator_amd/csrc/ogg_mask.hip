// Ocean mask: minimum depth and connected basins (include/ogg_hip.h, "Ocean mask").  Connected components of the wet cells by
// union-find, in three launches, so the number of launches does not grow with a component's diameter (a serpentine channel is one
// component of millions of cells):
//
// mask_tile_kernel     one workgroup per tile of TW x th cells: the wet rule, then a union-find in LDS over the faces inside the tile
//                      (link the larger root under the smaller by an LDS atomicMin, retried); every cell's parent becomes the GLOBAL
//                      index of its tile-local root.  Row-major local indices map monotonically to global ones, so that root is the
//                      smallest global index of the tile-local component.
// mask_merge_kernel    one thread per face that crosses a tile edge, the periodic seam or the fold: the same union on the global
//                      parents, with agent-scope atomicMin links.  Other workgroups write parent words in this launch, so every read
//                      of one is an agent-scope relaxed atomic load (a plain load may return a stale line of another XCD's L2).
//                      Parents only ever decrease, so there is no cycle; the retry is lock-free and no workgroup waits on another.
// mask_flatten_kernel  its own launch (every link is in place): root[c] = find(c) and the cells per root.  Inside a tile the cells
//                      follow their parents in LDS to a representative; only representatives walk the global chains (halving them
//                      as they go), and the cells are counted per representative in LDS, then one atomicAdd per (tile,
//                      representative), so the world ocean does not serialise millions of atomics on one word.
// mask_list_kernel     the component list ((cells << 32) | (INT32_MAX - root) of every root) and the largest entry: each block owns a
//                      contiguous chunk, reduces its count and maximum, and adds to each shared word once.
// mask_apply_kernel    the edited depth and the final wet mask from the roots kept (a short sorted list chosen on the host, and
//                      keep_min_cells against the per-root counts), and the wet-rule and selection counts, one add per block.
// mask_seed_kernel     the nearest model-cell centre of each seed: the smallest squared chordal distance (its bits: positive doubles
//                      order as integers), then the smallest index at that distance; both reduced per wavefront first.
//
// Every result is an integer or a copy, so nothing depends on the order in which the atomics land.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ogg_blocks.h"
#include "ogg_common.h"
#include "ogg_unionfind.h"

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;
using ogg::round256;

constexpr int TW = 64;       // tile width: one wavefront across a tile row
constexpr int NT = 256;      // threads per workgroup
constexpr int TH_DEFAULT = 32;   // tile rows (OGG_MASK_TILE_ROWS)
constexpr int TH_MAX = 64;
constexpr long LIST_BLOCKS = 1024;   // blocks of the list and apply kernels: each block adds once to a shared counter word
constexpr long APPLY_BLOCKS = 1024;

static_assert(NT == BLOCKS_NT, "block_add sums over a workgroup of BLOCKS_NT threads");
static_assert(sizeof(ogg_mask_params) == 48, "ogg_mask_params layout");
static_assert(sizeof(ogg_mask_counts) == 64, "ogg_mask_counts layout");

struct Geo {
    const double* depth;
    long ny, nx;
    int th, nbx;
    double fill, min_depth;
    int mode;
};

// ---- tile-local labelling in LDS (lds_find, lds_unite: ogg_unionfind.h) ----------------------------------------------
__global__ __launch_bounds__(NT) void mask_tile_kernel(Geo g, int* par) {
    extern __shared__ int lab[];
    const int n = TW * g.th;
    const long i0 = (long)(blockIdx.x % g.nbx) * TW, j0 = (long)(blockIdx.x / g.nbx) * g.th;
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        int v = -1;
        if (j < g.ny && i < g.nx) {
            const double d = g.depth[j * g.nx + i];
            if (d > 0.0 && d != g.fill && !(d < g.min_depth && g.mode == OGG_MASK_MASK)) v = l;
        }
        lab[l] = v;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT) {
        if (__hip_atomic_load(&lab[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 0) continue;   // land stays -1
        const int tx = l % TW, ty = l / TW;
        if (tx + 1 < TW && __hip_atomic_load(&lab[l + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0) lds_unite(lab, l, l + 1);
        if (ty + 1 < g.th && __hip_atomic_load(&lab[l + TW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0)
            lds_unite(lab, l, l + TW);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        if (j >= g.ny || i >= g.nx) continue;
        int p = -1;
        if (lab[l] >= 0) {
            const int r = lds_find(lab, l);
            p = (int)((j0 + r / TW) * g.nx + i0 + r % TW);
        }
        par[j * g.nx + i] = p;
    }
}

// ---- merge across tile edges, the seam and the fold --------------------------------------------------------------
// (glb_load, glb_find, glb_find_halving, glb_unite: ogg_unionfind.h)
struct Faces {
    long ny, nx;
    int th;
    long n_v, n_h, n_p, n_f;   // faces across vertical tile edges, horizontal tile edges, the seam, the fold
};

__global__ __launch_bounds__(NT) void mask_merge_kernel(Faces f, int* par) {
    const long total = f.n_v + f.n_h + f.n_p + f.n_f;
    for (long t = (long)blockIdx.x * NT + threadIdx.x; t < total; t += (long)gridDim.x * NT) {
        long a, b, u = t;
        if (u < f.n_v) {   // (j, i - 1) ~ (j, i), i = (k + 1) * TW
            const long k = u / f.ny, j = u % f.ny;
            a = j * f.nx + (k + 1) * TW - 1;
            b = a + 1;
        } else if ((u -= f.n_v) < f.n_h) {   // (j - 1, i) ~ (j, i), j = (k + 1) * th
            const long k = u / f.nx, i = u % f.nx;
            a = ((k + 1) * f.th - 1) * f.nx + i;
            b = a + f.nx;
        } else if ((u -= f.n_h) < f.n_p) {   // (j, nx - 1) ~ (j, 0)
            a = u * f.nx + f.nx - 1;
            b = u * f.nx;
        } else {   // (ny - 1, i) ~ (ny - 1, nx - 1 - i), i < nx - 1 - i
            u -= f.n_p;
            a = (f.ny - 1) * f.nx + u;
            b = (f.ny - 1) * f.nx + f.nx - 1 - u;
        }
        if (glb_load(&par[a]) >= 0 && glb_load(&par[b]) >= 0) glb_unite(par, (int)a, (int)b);   // land stays -1
    }
}

// ---- flatten, cells per root ---------------------------------------------------------------------------------------
// The tile's parents go to LDS; every cell follows them inside the tile to its representative (the first cell whose parent is
// itself or lies outside the tile).  Only the representatives walk the global chains; the other cells take their representative's
// root from LDS.
__global__ __launch_bounds__(NT) void mask_flatten_kernel(Geo g, int* par, int* root, int* size) {
    extern __shared__ int sh[];
    const int n = TW * g.th;
    int* lp = sh;          // the parent of each tile cell as a tile-local index, -1 outside the tile, -2 for land / off the grid
    int* rt = sh + n;      // the root of each representative
    int* cnt = sh + 2 * n; // cells per representative
    const long i0 = (long)(blockIdx.x % g.nbx) * TW, j0 = (long)(blockIdx.x / g.nbx) * g.th;
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        int v = -2;
        if (j < g.ny && i < g.nx) {
            const int p = glb_load(&par[j * g.nx + i]);   // (another tile's walk may halve it: any value read is an ancestor)
            if (p >= 0) {
                const long pj = p / g.nx, pi = p % g.nx;
                v = (pj >= j0 && pj < j0 + g.th && pi >= i0 && pi < i0 + TW) ? (int)((pj - j0) * TW + (pi - i0)) : -1;
                if (v == l) v = -1;   // a root: its own representative
            }
        }
        lp[l] = v;
        cnt[l] = 0;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT)
        if (lp[l] == -1) rt[l] = glb_find_halving(par, (int)((j0 + l / TW) * g.nx + i0 + l % TW));
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        if (j >= g.ny || i >= g.nx) continue;
        if (lp[l] == -2) {
            root[j * g.nx + i] = -1;
            continue;
        }
        int x = l;
        while (lp[x] >= 0) x = lp[x];   // in-tile parents have smaller local indices: this ends
        root[j * g.nx + i] = rt[x];
        atomicAdd(&cnt[x], 1);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT)
        if (cnt[l] > 0) atomicAdd(&size[rt[l]], cnt[l]);
}

// ---- component list and the largest ------------------------------------------------------------------------------
// Each block owns one contiguous chunk of cells: it counts its roots and takes their room in the list with ONE atomicAdd, then writes
// them in order (a ballot per wavefront, the wavefronts' counts through LDS); the largest entry goes through one atomicMax per block.
__global__ __launch_bounds__(NT) void mask_list_kernel(long n, long chunk, const int* root, const int* size, long long* list,
                                                       ogg_mask_counts* counts) {
    __shared__ unsigned long long wmax[NT / 64];
    __shared__ unsigned wcnt[NT / 64];
    __shared__ unsigned long long base;
    const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
    const long c0 = (long)blockIdx.x * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
    unsigned long long best = 0;
    unsigned mine = 0;
    for (long c = c0 + threadIdx.x; c < c1; c += NT) {
        if (root[c] != (int)c) continue;
        ++mine;
        const unsigned long long key = ((unsigned long long)(unsigned)size[c] << 32) | (unsigned long long)(INT_MAX - (int)c);
        best = key > best ? key : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(best, o, 64);
        best = v > best ? v : best;
        mine += __shfl_xor(mine, o, 64);
    }
    if (lane == 0) wmax[w] = best, wcnt[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0, t = 0;
        for (int k = 0; k < NT / 64; ++k) m = wmax[k] > m ? wmax[k] : m, t += wcnt[k];
        if (m) atomicMax(ull(&counts->largest), m);
        base = t ? atomicAdd(ull(&counts->components), t) : 0;
    }
    __syncthreads();
    unsigned long long off = base;
    for (long c00 = c0; c00 < c1; c00 += NT) {   // the same trip count for every thread of the block
        const long c = c00 + threadIdx.x;
        const bool is = c < c1 && root[c] == (int)c;
        const unsigned long long m = __ballot(is);
        __syncthreads();   // (the previous round's reads of wcnt are done)
        if (lane == 0) wcnt[w] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned long long before = off;
        for (int k = 0; k < w; ++k) before += wcnt[k];
        for (int k = 0; k < NT / 64; ++k) off += wcnt[k];
        if (is)
            list[before + __popcll(m & ((1ull << lane) - 1ull))] =
                (long long)(((unsigned long long)(unsigned)size[c] << 32) | (unsigned long long)(INT_MAX - (int)c));
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mask_apply_kernel(Geo g, const int* root, const int* size, const int* kept, int n_kept,
                                                        long long kmin, double* out, unsigned char* wet, ogg_mask_counts* counts) {
    const long n = g.ny * g.nx;
    long long v[6] = {0, 0, 0, 0, 0, 0};   // wet_in, masked, deepened, kept, removed, wet_out
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const double d = g.depth[c];
        const int r = root[c];
        bool keep = false;
        if (r >= 0) {
            int lo = 0, hi = n_kept;   // kept[] is sorted
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (kept[mid] < r) lo = mid + 1; else hi = mid;
            }
            keep = (lo < n_kept && kept[lo] == r) || (kmin > 0 && (long long)size[r] >= kmin);
        }
        const bool wet0 = d > 0.0 && d != g.fill, shallow = wet0 && d < g.min_depth;
        double o = d;
        if (keep)
            o = shallow ? g.min_depth : d;   // a kept shallow cell exists only in mode deepen
        else if (wet0)
            o = 0.0;
        out[c] = o;
        wet[c] = keep ? 1 : 0;
        v[0] += wet0;
        v[1] += shallow && g.mode == OGG_MASK_MASK;
        v[2] += shallow && g.mode == OGG_MASK_DEEPEN;
        v[3] += keep && r == (int)c;
        v[4] += r >= 0 && !keep;
        v[5] += keep;
    }
    long long* const dst[6] = {&counts->wet_in, &counts->masked, &counts->deepened, &counts->kept, &counts->removed, &counts->wet_out};
    block_add<6>(v, dst);
}

// ---- seeds ---------------------------------------------------------------------------------------------------------
__device__ inline double chord2(double lon, double lat, double sx, double sy, double sz) {
    const double D = 0.017453292519943295;   // pi / 180
    const double cl = cos(lat * D);
    const double dx = cl * cos(lon * D) - sx, dy = cl * sin(lon * D) - sy, dz = sin(lat * D) - sz;
    return dx * dx + dy * dy + dz * dz;
}

template <bool SECOND>
__global__ __launch_bounds__(NT) void mask_seed_kernel(long ny, long nx, const double* x, const double* y, long ld, int ns,
                                                       const double* lonlat, unsigned long long* out) {
    const long n = ny * nx;
    const double D = 0.017453292519943295;
    for (int s = 0; s < ns; ++s) {
        const double slon = lonlat[2 * s] * D, slat = lonlat[2 * s + 1] * D;
        const double sx = cos(slat) * cos(slon), sy = cos(slat) * sin(slon), sz = sin(slat);
        const unsigned long long want = SECOND ? out[2 * s] : 0ull;   // written by the first launch
        unsigned long long best = ULLONG_MAX;
        for (long base = (long)blockIdx.x * NT; base < n; base += (long)gridDim.x * NT) {
            const long c = base + threadIdx.x;
            if (c >= n) continue;
            const long j = c / nx, i = c % nx, k = (2 * j + 1) * ld + 2 * i + 1;
            double d2 = chord2(x[k], y[k], sx, sy, sz);
            unsigned long long bits;
            memcpy(&bits, &d2, 8);
            const unsigned long long v = SECOND ? (bits == want ? (unsigned long long)c : ULLONG_MAX) : bits;
            best = v < best ? v : best;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(best, o, 64);
            best = v < best ? v : best;
        }
        if ((threadIdx.x & 63) == 0 && best != ULLONG_MAX) atomicMin(&out[2 * s + (SECOND ? 1 : 0)], best);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_mask_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "ocean mask: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1, OGG_EARG, "ocean mask: %ld x %ld cells", p->ny, p->nx);
    OGG_REQUIRE(p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "ocean mask: %ld x %ld cells: ny * nx must be < 2^31", p->ny, p->nx);
    OGG_REQUIRE(p->mode == OGG_MASK_MASK || p->mode == OGG_MASK_DEEPEN, OGG_EARG, "ocean mask: mode %d (0: mask, 1: deepen)", p->mode);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "ocean mask: topology flags %d", p->topology);
    OGG_REQUIRE(std::isfinite(p->min_depth) && p->min_depth >= 0.0, OGG_EARG, "ocean mask: min_depth must be >= 0 (%g)", p->min_depth);
    OGG_REQUIRE(!std::isnan(p->fill), OGG_EARG, "ocean mask: the fill value is NaN");
    OGG_REQUIRE(p->keep_min_cells >= 0, OGG_EARG, "ocean mask: keep_min_cells must be >= 0 (%lld)", p->keep_min_cells);
    return OGG_OK;
}

long ws_bytes(const ogg_mask_params& p) { return 2 * round256(p.ny * p.nx * 4); }

Geo make_geo(const ogg_mask_params& p, const double* depth, int th) {
    return Geo{depth, p.ny, p.nx, th, (int)((p.nx + TW - 1) / TW), p.fill, p.min_depth, p.mode};
}

}  // namespace

extern "C" long ogg_mask_struct_bytes(int which) {
    return which == OGG_MASK_PARAMS ? (long)sizeof(ogg_mask_params) : (which == OGG_MASK_COUNTS ? (long)sizeof(ogg_mask_counts) : -1L);
}

extern "C" long ogg_mask_workspace_bytes(const ogg_mask_params* p) {
    if (!p || p->ny < 1 || p->nx < 1 || p->ny > (long)INT_MAX || p->nx > (long)INT_MAX || p->ny * p->nx >= (1L << 31)) return -1;
    return ws_bytes(*p);
}

extern "C" int ogg_mask_check(const ogg_mask_params* p) { return check_params(p); }

extern "C" int ogg_mask_label_dev(const ogg_mask_params* p, const double* depth, void* workspace, long workspace_bytes, int* root,
                                  long long* components, ogg_mask_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(depth && root && components && counts, OGG_EARG, "ogg_mask_label: null depth / root / components / counts");
    OGG_REQUIRE(workspace && workspace_bytes >= ws_bytes(*p), OGG_EARG, "ogg_mask_label: workspace of %ld bytes, %ld needed",
                workspace_bytes, ws_bytes(*p));
    int th = 0;
    if (int e = knob("OGG_MASK_TILE_ROWS", TH_DEFAULT, 1, TH_MAX, &th)) return e;
    const long n = p->ny * p->nx;
    int* par = static_cast<int*>(workspace);
    int* size = at<int>(workspace, round256(n * 4));
    hipStream_t st = ogg::as_stream(stream);
    const Geo g = make_geo(*p, depth, th);
    const long nby = (p->ny + th - 1) / th;
    const long tiles = (long)g.nbx * nby;
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_mask_counts), st));
    OGG_HIP_CHECK(hipMemsetAsync(size, 0, (size_t)n * 4, st));
    mask_tile_kernel<<<(unsigned)tiles, NT, TW * th * sizeof(int), st>>>(g, par);
    OGG_LAUNCH_CHECK();
    Faces f{p->ny, p->nx, th, (long)(g.nbx - 1) * p->ny, (nby - 1) * p->nx, 0, 0};
    if ((p->topology & OGG_MASK_PERIODIC) && p->nx > 2) f.n_p = p->ny;
    if (p->topology & OGG_MASK_FOLD) f.n_f = p->nx / 2;
    const long faces = f.n_v + f.n_h + f.n_p + f.n_f;
    if (faces > 0) {
        mask_merge_kernel<<<grid_for<NT>(faces, 4096), NT, 0, st>>>(f, par);
        OGG_LAUNCH_CHECK();
    }
    mask_flatten_kernel<<<(unsigned)tiles, NT, 3 * TW * th * sizeof(int), st>>>(g, par, root, size);
    OGG_LAUNCH_CHECK();
    const long blocks = grid_for<NT>(n, LIST_BLOCKS), chunk = (n + blocks - 1) / blocks;
    mask_list_kernel<<<(unsigned)blocks, NT, 0, st>>>(n, chunk, root, size, components, counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_mask_seed_dev(const ogg_mask_params* p, const double* x, const double* y, long ld, int n_seeds, const double* lonlat,
                                 long long* out, void* stream) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(n_seeds >= 0 && n_seeds <= OGG_MASK_MAX_SEEDS, OGG_EARG, "ocean mask: %d seeds (at most %d)", n_seeds, OGG_MASK_MAX_SEEDS);
    if (n_seeds == 0) return OGG_OK;
    OGG_REQUIRE(x && y && lonlat && out, OGG_EARG, "ogg_mask_seed: null x / y / lonlat / out");
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_mask_seed: point rows of %ld, %ld needed", ld, 2 * p->nx + 1);
    hipStream_t st = ogg::as_stream(stream);
    const long n = p->ny * p->nx;
    OGG_HIP_CHECK(hipMemsetAsync(out, 0xFF, (size_t)n_seeds * 16, st));
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    mask_seed_kernel<false><<<grid_for<NT>(n, 4096), NT, 0, st>>>(p->ny, p->nx, x, y, ld, n_seeds, lonlat, o);
    OGG_LAUNCH_CHECK();
    mask_seed_kernel<true><<<grid_for<NT>(n, 4096), NT, 0, st>>>(p->ny, p->nx, x, y, ld, n_seeds, lonlat, o);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_mask_apply_dev(const ogg_mask_params* p, const double* depth, const int* root, const void* workspace,
                                  long workspace_bytes, const int* kept, int n_kept, double* depth_out, unsigned char* wet,
                                  ogg_mask_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(depth && root && depth_out && wet && counts, OGG_EARG, "ogg_mask_apply: null depth / root / depth_out / wet / counts");
    OGG_REQUIRE(n_kept >= 0 && (kept || n_kept == 0), OGG_EARG, "ogg_mask_apply: %d kept roots", n_kept);
    OGG_REQUIRE(workspace && workspace_bytes >= ws_bytes(*p), OGG_EARG, "ogg_mask_apply: workspace of %ld bytes, %ld needed",
                workspace_bytes, ws_bytes(*p));
    const long n = p->ny * p->nx;
    const int* size = at<int>(workspace, round256(n * 4));
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(&counts->wet_in, 0, 3 * sizeof(long long), st));
    OGG_HIP_CHECK(hipMemsetAsync(&counts->kept, 0, 3 * sizeof(long long), st));
    mask_apply_kernel<<<grid_for<NT>(n, APPLY_BLOCKS), NT, 0, st>>>(make_geo(*p, depth, 1), root, size, kept, n_kept, p->keep_min_cells, depth_out, wet,
                                                  counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: inputs copied to device memory, label, seeds, the choice of kept roots, apply, results copied back
extern "C" int ogg_ocean_mask(const ogg_mask_params* p, const double* depth, const double* x, const double* y, int n_seeds,
                              const double* lonlat, double* depth_out, unsigned char* wet, int* root, long long* seed_cells,
                              long long* components, long capacity, ogg_mask_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(depth && depth_out && wet && root && counts, OGG_EARG, "ogg_ocean_mask: null depth / depth_out / wet / root / counts");
    OGG_REQUIRE(n_seeds >= 0 && n_seeds <= OGG_MASK_MAX_SEEDS, OGG_EARG, "ocean mask: %d seeds (at most %d)", n_seeds, OGG_MASK_MAX_SEEDS);
    OGG_REQUIRE(n_seeds == 0 || (x && y && lonlat && seed_cells), OGG_EARG, "ogg_ocean_mask: seeds need x, y, lonlat and seed_cells");
    for (int s = 0; s < n_seeds; ++s)
        OGG_REQUIRE(std::isfinite(lonlat[2 * s]) && std::isfinite(lonlat[2 * s + 1]) && fabs(lonlat[2 * s + 1]) <= 90.0, OGG_EARG,
                    "ocean mask: seed %d (%g, %g) is not a point on the sphere", s, lonlat[2 * s], lonlat[2 * s + 1]);
    OGG_REQUIRE(capacity >= 0 && (components || capacity == 0), OGG_EARG, "ogg_ocean_mask: component capacity %ld", capacity);
    int th = 0;
    if (int e = knob("OGG_MASK_TILE_ROWS", TH_DEFAULT, 1, TH_MAX, &th)) return e;
    ogg::Buffers bufs;   // freed on every exit path
    const long n = p->ny * p->nx, wsb = ws_bytes(*p);
    void *dd = nullptr, *ws = nullptr, *dr = nullptr, *dc = nullptr, *ct = nullptr, *dout = nullptr, *dwet = nullptr, *dk = nullptr;
    if (int e = bufs.alloc(&dd, (size_t)n * 8)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&dr, (size_t)n * 4)) return e;
    if (int e = bufs.alloc(&dc, (size_t)n * 8)) return e;
    if (int e = bufs.alloc(&ct, sizeof(ogg_mask_counts))) return e;
    OGG_HIP_CHECK(hipMemcpy(dd, depth, (size_t)n * 8, hipMemcpyHostToDevice));
    ogg_mask_counts* dct = static_cast<ogg_mask_counts*>(ct);
    if (int e = ogg_mask_label_dev(p, static_cast<const double*>(dd), ws, wsb, static_cast<int*>(dr), static_cast<long long*>(dc), dct,
                                   nullptr))
        return e;
    OGG_HIP_CHECK(hipMemcpy(counts, ct, sizeof(ogg_mask_counts), hipMemcpyDeviceToHost));
    OGG_HIP_CHECK(hipMemcpy(root, dr, (size_t)n * 4, hipMemcpyDeviceToHost));
    std::vector<int> kept;
    if (n_seeds > 0) {
        const long np = (2 * p->ny + 1) * (2 * p->nx + 1);
        void *px = nullptr, *py = nullptr, *ps = nullptr, *po = nullptr;
        if (int e = bufs.alloc(&px, (size_t)np * 8)) return e;
        if (int e = bufs.alloc(&py, (size_t)np * 8)) return e;
        if (int e = bufs.alloc(&ps, (size_t)n_seeds * 16)) return e;
        if (int e = bufs.alloc(&po, (size_t)n_seeds * 16)) return e;
        OGG_HIP_CHECK(hipMemcpy(px, x, (size_t)np * 8, hipMemcpyHostToDevice));
        OGG_HIP_CHECK(hipMemcpy(py, y, (size_t)np * 8, hipMemcpyHostToDevice));
        OGG_HIP_CHECK(hipMemcpy(ps, lonlat, (size_t)n_seeds * 16, hipMemcpyHostToDevice));
        if (int e = ogg_mask_seed_dev(p, static_cast<const double*>(px), static_cast<const double*>(py), 2 * p->nx + 1, n_seeds,
                                      static_cast<const double*>(ps), static_cast<long long*>(po), nullptr))
            return e;
        std::vector<long long> so(2 * (size_t)n_seeds);
        OGG_HIP_CHECK(hipMemcpy(so.data(), po, (size_t)n_seeds * 16, hipMemcpyDeviceToHost));
        for (int s = 0; s < n_seeds; ++s) {
            const long long c = so[2 * s + 1];
            OGG_REQUIRE(c >= 0 && c < n, OGG_EARG, "ocean mask: seed %d (%g, %g) found no cell centre", s, lonlat[2 * s], lonlat[2 * s + 1]);
            seed_cells[s] = c;
            OGG_REQUIRE(root[c] >= 0, OGG_EARG, "ocean mask: seed %d (%g, %g) lies on land: cell (j, i) = (%lld, %lld) has depth %.17g", s,
                        lonlat[2 * s], lonlat[2 * s + 1], c / p->nx, c % p->nx, depth[c]);
            kept.push_back(root[c]);
        }
    } else if (counts->components > 0) {
        kept.push_back(INT_MAX - (int)(counts->largest & 0xFFFFFFFFll));
    }
    std::sort(kept.begin(), kept.end());
    kept.erase(std::unique(kept.begin(), kept.end()), kept.end());
    if (!kept.empty()) {
        if (int e = bufs.alloc(&dk, kept.size() * 4)) return e;
        OGG_HIP_CHECK(hipMemcpy(dk, kept.data(), kept.size() * 4, hipMemcpyHostToDevice));
    }
    if (int e = bufs.alloc(&dout, (size_t)n * 8)) return e;
    if (int e = bufs.alloc(&dwet, (size_t)n)) return e;
    if (int e = ogg_mask_apply_dev(p, static_cast<const double*>(dd), static_cast<const int*>(dr), ws, wsb, static_cast<const int*>(dk),
                                   (int)kept.size(), static_cast<double*>(dout), static_cast<unsigned char*>(dwet), dct, nullptr))
        return e;
    OGG_HIP_CHECK(hipMemcpy(counts, ct, sizeof(ogg_mask_counts), hipMemcpyDeviceToHost));
    OGG_HIP_CHECK(hipMemcpy(depth_out, dout, (size_t)n * 8, hipMemcpyDeviceToHost));
    OGG_HIP_CHECK(hipMemcpy(wet, dwet, (size_t)n, hipMemcpyDeviceToHost));
    if (capacity > 0 && counts->components > 0) {
        std::vector<long long> list((size_t)counts->components);
        OGG_HIP_CHECK(hipMemcpy(list.data(), dc, list.size() * 8, hipMemcpyDeviceToHost));
        std::sort(list.begin(), list.end(), [](long long a, long long b) { return a > b; });
        std::copy(list.begin(), list.begin() + std::min<long>(capacity, (long)list.size()), components);
    }
    return OGG_OK;
}
