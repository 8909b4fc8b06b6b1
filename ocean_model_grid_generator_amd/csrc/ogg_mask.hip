// Ocean mask: minimum depth and connected basins (include/ogg_hip.h, "Ocean mask").  The connected components of the wet cells are
// those of ogg_label.h under one class, with the cells per root; what is left here:
//
// mask_tile_kernel     the wet rule of a tile's cells, then label_tile.
// mask_list_kernel     the component list ((cells << 32) | (INT32_MAX - root) of every root) and the largest entry: each block owns a
//                      contiguous chunk, reduces its count and maximum, and adds to each shared word once.
// mask_apply_kernel    the edited depth and the final wet mask from the roots kept (a short sorted list chosen on the host, and
//                      keep_min_cells against the per-root counts), and the wet-rule and selection counts, one add per block.
// mask_seed_kernel     the nearest model-cell centre of each seed: the smallest squared chordal distance (unit, dist2 and bits_of of
//                      ogg_sphere.h, the basin codes' own; positive doubles order as integers), then the smallest index at that
//                      distance; both reduced per wavefront first.
//
// Every result is an integer or a copy, so nothing depends on the order in which the atomics land.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ogg_blocks.h"
#include "ogg_common.h"
#include "ogg_label.h"
#include "ogg_sphere.h"

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr long LIST_BLOCKS = 1024;   // blocks of the list and apply kernels: each block adds once to a shared counter word
constexpr long APPLY_BLOCKS = 1024;

static_assert(sizeof(ogg_mask_params) == 48, "ogg_mask_params layout");
static_assert(sizeof(ogg_mask_counts) == 64, "ogg_mask_counts layout");

struct Geo {
    const double* depth;
    double fill, min_depth;
    int mode;
};

// ---- the wet rule and the tile-local labelling (ogg_label.h) -------------------------------------------------------
__global__ __launch_bounds__(NT) void mask_tile_kernel(Grid t, Geo g, int* par) {
    extern __shared__ int lab[];
    const int n = TW * t.th;
    const long i0 = (long)(blockIdx.x % t.nbx) * TW, j0 = (long)(blockIdx.x / t.nbx) * t.th;
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        int v = -1;
        if (j < t.ny && i < t.nx) {
            const double d = g.depth[j * t.nx + i];
            if (d > 0.0 && d != g.fill && !(d < g.min_depth && g.mode == OGG_MASK_MASK)) v = l;
        }
        lab[l] = v;
    }
    label_tile<false>(t, j0, i0, lab, 1, par);
}

struct BothWet {   // the merge predicate of one class: land stays -1
    __device__ bool operator()(const int* par, long a, long b) const { return glb_load(&par[a]) >= 0 && glb_load(&par[b]) >= 0; }
};

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
__global__ __launch_bounds__(NT) void mask_apply_kernel(Geo g, long n, const int* root, const int* size, const int* kept, int n_kept,
                                                        long long kmin, double* out, unsigned char* wet, ogg_mask_counts* counts) {
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
template <bool SECOND>
__global__ __launch_bounds__(NT) void mask_seed_kernel(long ny, long nx, const double* x, const double* y, long ld, int ns,
                                                       const double* lonlat, unsigned long long* out) {
    const long n = ny * nx;
    for (int s = 0; s < ns; ++s) {
        double su[3], cu[3];
        unit(lonlat[2 * s], lonlat[2 * s + 1], su);
        const unsigned long long want = SECOND ? out[2 * s] : 0ull;   // written by the first launch
        unsigned long long best = ULLONG_MAX;
        for (long base = (long)blockIdx.x * NT; base < n; base += (long)gridDim.x * NT) {
            const long c = base + threadIdx.x;
            if (c >= n) continue;
            centre_unit(x, y, c, nx, ld, cu);
            const unsigned long long bits = bits_of(dist2(cu[0], cu[1], cu[2], su[0], su[1], su[2]));
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

// workspace: parents | cells per root
struct Layout {
    long par, size, total;
};

Layout layout(const ogg_mask_params& p) {
    ogg::Sections s{0};
    return Layout{s.take(p.ny * p.nx * 4), s.take(p.ny * p.nx * 4), s.off};   // a braced list is evaluated left to right
}

long ws_bytes(const ogg_mask_params& p) { return layout(p).total; }

}  // namespace

extern "C" long ogg_mask_workspace_bytes(const ogg_mask_params* p) {
    if (!p || p->ny < 1 || p->nx < 1 || p->ny > (long)INT_MAX || p->nx > (long)INT_MAX || p->ny * p->nx >= (1L << 31)) return -1;
    return ws_bytes(*p);
}

extern "C" int ogg_mask_check(const ogg_mask_params* p) { return check_params(p); }

extern "C" int ogg_mask_label_dev(const ogg_mask_params* p, const double* depth, void* workspace, long workspace_bytes, int* root,
                                  long long* components, ogg_mask_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(depth && root && components && counts, OGG_EARG, "ogg_mask_label: null depth / root / components / counts");
    if (int e = ogg::check_workspace("ogg_mask_label", workspace, workspace_bytes, ws_bytes(*p))) return e;
    int th = 0;
    if (int e = knob("OGG_MASK_TILE_ROWS", TH_DEFAULT, 1, TH_MAX, &th)) return e;
    const long n = p->ny * p->nx;
    int* par = at<int>(workspace, layout(*p).par);
    int* size = at<int>(workspace, layout(*p).size);
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_mask_counts), st));
    OGG_HIP_CHECK(hipMemsetAsync(size, 0, (size_t)n * 4, st));
    const Geo geo{depth, p->fill, p->min_depth, p->mode};
    const auto tile = [&](const Grid& g, unsigned tiles) { mask_tile_kernel<<<tiles, NT, TW * th * sizeof(int), st>>>(g, geo, par); };
    if (int e = label_components<true>(p->ny, p->nx, th, p->topology, tile, BothWet{}, par, root, size, st)) return e;
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
    if (int e = ogg::check_workspace("ogg_mask_apply", workspace, workspace_bytes, ws_bytes(*p))) return e;
    const long n = p->ny * p->nx;
    const int* size = at<int>(workspace, layout(*p).size);
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(&counts->wet_in, 0, 3 * sizeof(long long), st));
    OGG_HIP_CHECK(hipMemsetAsync(&counts->kept, 0, 3 * sizeof(long long), st));
    mask_apply_kernel<<<grid_for<NT>(n, APPLY_BLOCKS), NT, 0, st>>>(Geo{depth, p->fill, p->min_depth, p->mode}, n, root, size, kept, n_kept,
                                                                    p->keep_min_cells, depth_out, wet, counts);
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
    double *dd, *dout;
    char* ws;
    int *dr, *dk = nullptr;
    long long* dc;
    unsigned char* dwet;
    ogg_mask_counts* ct;
    if (int e = bufs.alloc(&dd, (size_t)n)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&dr, (size_t)n)) return e;
    if (int e = bufs.alloc(&dc, (size_t)n)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = bufs.send(dd, depth, (size_t)n)) return e;
    if (int e = ogg_mask_label_dev(p, dd, ws, wsb, dr, dc, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(root, dr, (size_t)n)) return e;
    std::vector<int> kept;
    if (n_seeds > 0) {
        const size_t np = (size_t)(2 * p->ny + 1) * (2 * p->nx + 1);
        double *px, *py, *ps;
        long long* po;
        if (int e = bufs.alloc(&px, np)) return e;
        if (int e = bufs.alloc(&py, np)) return e;
        if (int e = bufs.alloc(&ps, (size_t)n_seeds * 2)) return e;
        if (int e = bufs.alloc(&po, (size_t)n_seeds * 2)) return e;
        if (int e = bufs.send(px, x, np)) return e;
        if (int e = bufs.send(py, y, np)) return e;
        if (int e = bufs.send(ps, lonlat, (size_t)n_seeds * 2)) return e;
        if (int e = ogg_mask_seed_dev(p, px, py, 2 * p->nx + 1, n_seeds, ps, po, nullptr)) return e;
        std::vector<long long> so(2 * (size_t)n_seeds);
        if (int e = bufs.get(so.data(), po, so.size())) return e;
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
    if (!kept.empty())
        if (int e = bufs.put(&dk, kept.data(), kept.size())) return e;
    if (int e = bufs.alloc(&dout, (size_t)n)) return e;
    if (int e = bufs.alloc(&dwet, (size_t)n)) return e;
    if (int e = ogg_mask_apply_dev(p, dd, dr, ws, wsb, dk, (int)kept.size(), dout, dwet, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(depth_out, dout, (size_t)n)) return e;
    if (int e = bufs.get(wet, dwet, (size_t)n)) return e;
    if (capacity > 0 && counts->components > 0) {
        std::vector<long long> list((size_t)counts->components);
        if (int e = bufs.get(list.data(), dc, list.size())) return e;
        std::sort(list.begin(), list.end(), [](long long a, long long b) { return a > b; });
        std::copy(list.begin(), list.begin() + std::min<long>(capacity, (long)list.size()), components);
    }
    return OGG_OK;
}
