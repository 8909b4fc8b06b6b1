// Sill depths: the widest-path ("bottleneck") depth of every model cell with respect to a set of seed cells, its regions and the gate
// faces that limit them (include/ogg_hip.h, "Sill depths").  b is decided bit by bit from the top; the state is lo[c], the bits decided
// so far (a seed holds OGG_SILL_SEED).  One round, bit k: T(c) = lo[c] | (1 << k); the cells are labelled over the passages with equal
// lo (not SEED) and w >= T; a component is REACHED when one of its cells has a passage with w >= T to a cell of a greater lo; every
// cell of a reached component sets bit k (DESIGN.md has the argument).  The labelling is ogg_label.h's: its lock-free unite and find,
// its merge launch and its flatten launch as they are; the tile body is new, because a passage here depends on an int per cell and on
// the weight of the face, not on a class byte.  Every round is five launches on the caller's stream, whatever a component's diameter,
// and nothing comes back to the host between rounds:
//
// sill_prep_kernel     once: the clamped weight of every cell's EAST passage (we: the u face to the east, the seam's min(wu[j][0],
//                      wu[j][nx]) in the last column, 0 where there is none) and NORTH passage (wn: the v face to the north, the fold's
//                      min(wv[ny][i], wv[ny][nx - 1 - i]) in the last row for both partners, 0 where there is none), lo = 0, and
//                      n_clamped.  Every later kernel reads we and wn only, so no later kernel knows the topology but the merge
//                      predicate and the gates.
// sill_seed_kernel     once: lo = OGG_SILL_SEED at every seed, n_bad_seeds.
// sill_tile_kernel     per round: lo, we, wn and the parents of a tile in LDS (16 bytes per tile cell), the union over the passages
//                      inside the tile, the parents as global indices (-1 for a seed), and the reach words of the tile's cells zeroed.
//                      <true>: the last labelling, T = lo and only cells with 0 < lo < SEED, whose roots are the regions.
// label_merge_kernel   (ogg_label.h) with the predicate Passage: the passages across tile edges, the seam and the fold.
// label_flatten_kernel<false>  (ogg_label.h) root[c].
// sill_reach_kernel    per round: a cell with a passage w >= T to a cell of a greater lo stores 1 to reach[root] (plain stores of 1).
// sill_apply_kernel    per round: lo |= 1 << k where reach[root] is set.
// sill_finish_kernel   once: region at seeds and dry cells, and the cell counts.
// sill_gate_kernel     once: one thread per u and v face, the gate codes and n_gate_faces.
//
// Every result is an integer and every count a sum of integers, so nothing depends on the order in which the atomics land, on the
// tile height or on the launch shape.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; LDS is dynamic, at the default tile of 64 x 32):
//   kernel                          VGPRs  SGPRs  LDS bytes  scratch  waves/SIMD
//   sill_prep_kernel                    24     64         32        0           8
//   sill_seed_kernel                    10     26         32        0           8
//   sill_tile_kernel<false>             16     43  32768 dyn        0           8
//   sill_tile_kernel<true>              16     42  32768 dyn        0           8
//   label_merge_kernel<Passage>         16     67          0        0           8
//   label_flatten_kernel<false>         24     53  16384 dyn        0           8
//   sill_reach_kernel                   26     58          0        0           8
//   sill_apply_kernel                    8     23          0        0           8
//   sill_finish_kernel                  22     52         96        0           8
//   sill_gate_kernel                    20     70         32        0           8
#include <climits>
#include <cstdlib>

#include "ogg_blocks.h"
#include "ogg_common.h"
#include "ogg_label.h"

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int SEED = OGG_SILL_SEED;
constexpr long ELEMENT_BLOCKS = 4096;   // workgroups of the elementwise kernels (grid-stride)
constexpr long COUNT_BLOCKS = 1024;     // of the kernels that count: each block adds once to a shared counter word

struct Params {   // the six scalars every entry takes first
    long ny, nx;
    int topology, bits, n_seeds, tile_rows;
};

struct Counts {   // the OGG_SILL_COUNT_WORDS words of the header, in its order
    long long rounds, n_clamped, n_bad_seeds, n_connected, n_cut_off, n_regions, n_gate_faces;
};

static_assert(sizeof(Counts) == OGG_SILL_COUNT_WORDS * sizeof(long long), "the counts are OGG_SILL_COUNT_WORDS int64 words");

__device__ inline int clamp_w(int w, int wmax, long long* changed) {
    const int c = w < 0 ? 0 : (w > wmax ? wmax : w);
    *changed += c != w;
    return c;
}

// ---- once per call: the passages of every cell -----------------------------------------------------------------------
__global__ __launch_bounds__(NT) void sill_prep_kernel(long ny, long nx, int topology, int wmax, const int* __restrict__ wu,
                                                       const int* __restrict__ wv, int* __restrict__ we, int* __restrict__ wn,
                                                       int* __restrict__ lo, Counts* counts) {
    const long n = ny * nx;
    const bool seam = (topology & OGG_MASK_PERIODIC) && nx > 2, fold = (topology & OGG_MASK_FOLD) != 0;
    long long v[1] = {0};
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const long j = c / nx, i = c % nx;
        int e = 0, t = 0;
        if (i + 1 < nx) {
            e = clamp_w(wu[j * (nx + 1) + i + 1], wmax, v);
        } else if (seam) {   // both columns of the seam are counted here, once per row
            const int a = clamp_w(wu[j * (nx + 1)], wmax, v), b = clamp_w(wu[j * (nx + 1) + nx], wmax, v);
            e = a < b ? a : b;
        }
        if (j + 1 < ny) {
            t = clamp_w(wv[(j + 1) * nx + i], wmax, v);
        } else if (fold && i != nx - 1 - i) {   // every cell of the last row counts its own face; the partner's is the partner's
            long long other = 0;
            const int a = clamp_w(wv[ny * nx + i], wmax, v), b = clamp_w(wv[ny * nx + nx - 1 - i], wmax, &other);
            t = a < b ? a : b;
        }
        we[c] = e;
        wn[c] = t;
        lo[c] = 0;
    }
    long long* const dst[1] = {&counts->n_clamped};
    block_add<1>(v, dst);
}

__global__ __launch_bounds__(NT) void sill_seed_kernel(long n, int n_seeds, const long long* __restrict__ seeds, int* lo,
                                                       Counts* counts) {
    long long v[1] = {0};
    for (long s = (long)blockIdx.x * NT + threadIdx.x; s < n_seeds; s += (long)gridDim.x * NT) {
        const long long c = seeds[s];
        if (c >= 0 && c < n)
            lo[c] = SEED;   // duplicates store the same word
        else
            ++v[0];
    }
    long long* const dst[1] = {&counts->n_bad_seeds};
    block_add<1>(v, dst);
}

// ---- per round: the tile-local labelling -----------------------------------------------------------------------------
// sh: TW * th parents | lo | east weights | north weights.  A cell joins its east neighbour when both are eligible, their lo are equal
// and the east weight reaches T; the same to the north.  The last column and row of the grid have a neighbour off the grid (parent -1).
template <bool FINAL>
__global__ __launch_bounds__(NT) void sill_tile_kernel(Grid g, int bit, const int* __restrict__ lo, const int* __restrict__ we,
                                                       const int* __restrict__ wn, int* par, int* __restrict__ reach) {
    extern __shared__ int sh[];
    const int n = TW * g.th;
    int *lab = sh, *slo = sh + n, *se = sh + 2 * n, *sn = sh + 3 * n;
    const long i0 = (long)(blockIdx.x % g.nbx) * TW, j0 = (long)(blockIdx.x / g.nbx) * g.th;
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        int p = -1, v = 0, e = 0, t = 0;
        if (j < g.ny && i < g.nx) {
            const long c = j * g.nx + i;
            v = lo[c];
            e = we[c];
            t = wn[c];
            if (v != SEED && (!FINAL || v > 0)) p = l;
            if (!FINAL) reach[c] = 0;
        }
        lab[l] = p;
        slo[l] = v;
        se[l] = e;
        sn[l] = t;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT) {
        if (lds_load(&lab[l]) < 0) continue;
        const int v = slo[l], T = FINAL ? v : (v | bit);
        const int tx = l % TW, ty = l / TW;
        if (tx + 1 < TW && se[l] >= T && slo[l + 1] == v && lds_load(&lab[l + 1]) >= 0) lds_unite(lab, l, l + 1);
        if (ty + 1 < g.th && sn[l] >= T && slo[l + TW] == v && lds_load(&lab[l + TW]) >= 0) lds_unite(lab, l, l + TW);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        if (j >= g.ny || i >= g.nx) continue;
        int p = -1;
        if (lds_load(&lab[l]) >= 0) {
            const int r = lds_find(lab, l);
            p = (int)((j0 + r / TW) * g.nx + i0 + r % TW);
        }
        par[j * g.nx + i] = p;
    }
}

// The merge predicate.  label_merge_kernel names a face by its two cells (a, b); the weight is that of the passage between them: b == a
// + nx is a horizontal tile edge (wn[a]); b < a is the seam (a is the row's last cell: we[a]); b == a + 1 is a vertical tile edge
// (we[a]); anything else is the fold (wn[a], a the partner of the smaller index).  On an even fold row the two middle cells are
// neighbours AND partners, b == a + 1 for both faces: either face then joins on the larger of the two weights, which is the same union,
// because the other passage joins the same two cells (inside the tile or through its own face of this launch).
struct Passage {
    const int *lo, *we, *wn;
    long nx, top;   // top: the first cell of the last row with FOLD, LONG_MAX without
    int bit, final;
    __device__ bool operator()(const int*, long a, long b) const {
        const int v = lo[a];
        if (v != lo[b] || v == SEED || (final && v == 0)) return false;
        int w;
        if (b == a + nx)
            w = wn[a];
        else if (b < a)
            w = we[a];
        else if (b == a + 1) {
            w = we[a];
            if (a >= top && a + b == 2 * top + nx - 1 && wn[a] > w) w = wn[a];
        } else
            w = wn[a];
        return w >= (final ? v : (v | bit));
    }
};

// ---- per round: reach and apply ----------------------------------------------------------------------------------------
// The four passages of cell c: east we[c], north wn[c], west we[west cell], south wn[south cell].  The west cell of column 0 is the
// row's last cell (its we is the seam's weight, or 0); the north cell of the last row is the fold partner (wn is the fold's weight,
// or 0); row 0 has no south passage.
__global__ __launch_bounds__(NT) void sill_reach_kernel(long ny, long nx, int bit, const int* __restrict__ lo, const int* __restrict__ we,
                                                        const int* __restrict__ wn, const int* __restrict__ root, int* reach) {
    const long n = ny * nx;
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const int r = root[c];
        if (r < 0) continue;
        const long j = c / nx, i = c % nx;
        const int v = lo[c], T = v | bit;
        const long qe = i + 1 < nx ? c + 1 : c - (nx - 1), qw = i > 0 ? c - 1 : c + (nx - 1);
        const long qn = j + 1 < ny ? c + nx : j * nx + (nx - 1 - i);
        bool hit = (we[c] >= T && lo[qe] > v) || (wn[c] >= T && lo[qn] > v) || (we[qw] >= T && lo[qw] > v);
        if (j > 0) hit = hit || (wn[c - nx] >= T && lo[c - nx] > v);
        if (hit) reach[r] = 1;
    }
}

__global__ __launch_bounds__(NT) void sill_apply_kernel(long n, int bit, const int* __restrict__ root, const int* __restrict__ reach,
                                                        int* __restrict__ lo) {
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const int r = root[c];
        if (r >= 0 && reach[r] != 0) lo[c] |= bit;
    }
}

// ---- once per call: regions at seeds, counts, gates --------------------------------------------------------------------
__global__ __launch_bounds__(NT) void sill_finish_kernel(long ny, long nx, int rounds, const int* __restrict__ b, const int* __restrict__ we,
                                                         const int* __restrict__ wn, int* __restrict__ region, Counts* counts) {
    const long n = ny * nx;
    long long v[3] = {0, 0, 0};   // n_connected, n_cut_off, n_regions
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const int d = b[c];
        if (d == SEED) region[c] = (int)c;   // (the last labelling left -1 at seeds and where b = 0)
        if (d == 0) {
            const long j = c / nx, i = c % nx;
            const long qw = i > 0 ? c - 1 : c + (nx - 1);
            v[1] += we[c] > 0 || wn[c] > 0 || we[qw] > 0 || (j > 0 && wn[c - nx] > 0);
        }
        v[0] += d > 0 && d != SEED;
        v[2] += region[c] == (int)c;
    }
    long long* const dst[3] = {&counts->n_connected, &counts->n_cut_off, &counts->n_regions};
    block_add<3>(v, dst);
    if (blockIdx.x == 0 && threadIdx.x == 0) counts->rounds = rounds;
}

__device__ inline int gate_code(int ba, int bb, int w) { return (0 < ba && ba == w && w < bb) ? 1 : ((0 < bb && bb == w && w < ba) ? 2 : 0); }

// faces 0 .. ny (nx + 1) - 1 are the u faces, then the (ny + 1) nx v faces
__global__ __launch_bounds__(NT) void sill_gate_kernel(long ny, long nx, int topology, const int* __restrict__ b, const int* __restrict__ we,
                                                       const int* __restrict__ wn, unsigned char* __restrict__ gate_u,
                                                       unsigned char* __restrict__ gate_v, Counts* counts) {
    const long nu = ny * (nx + 1), total = nu + (ny + 1) * nx;
    const bool seam = (topology & OGG_MASK_PERIODIC) && nx > 2, fold = (topology & OGG_MASK_FOLD) != 0;
    long long v[1] = {0};
    for (long f = (long)blockIdx.x * NT + threadIdx.x; f < total; f += (long)gridDim.x * NT) {
        int code = 0;
        if (f < nu) {
            const long j = f / (nx + 1), I = f % (nx + 1);
            if (I > 0 && I < nx) {
                const long a = j * nx + I - 1;
                code = gate_code(b[a], b[a + 1], we[a]);
            } else if (seam) {
                const long a = j * nx + nx - 1;
                code = gate_code(b[a], b[j * nx], we[a]);
            }
            gate_u[f] = (unsigned char)code;
        } else {
            const long g = f - nu, J = g / nx, i = g % nx;
            if (J > 0 && J < ny) {
                const long a = (J - 1) * nx + i;
                code = gate_code(b[a], b[a + nx], wn[a]);
            } else if (J == ny && fold && i != nx - 1 - i) {
                const long m = i < nx - 1 - i ? i : nx - 1 - i, a = (ny - 1) * nx + m, q = (ny - 1) * nx + nx - 1 - m;
                code = gate_code(b[a], b[q], wn[a]);
                if (i != m && code != 0) code = 3 - code;   // seen from the partner's face: the roles swapped
            }
            gate_v[g] = (unsigned char)code;
        }
        v[0] += code != 0;
    }
    long long* const dst[1] = {&counts->n_gate_faces};
    block_add<1>(v, dst);
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const Params* p) {
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "sill depths: %ld x %ld cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "sill depths: topology flags %d", p->topology);
    OGG_REQUIRE(p->bits >= 1 && p->bits <= OGG_SILL_MAX_BITS, OGG_EARG, "sill depths: %d bits (1 .. %d)", p->bits, OGG_SILL_MAX_BITS);
    OGG_REQUIRE(p->n_seeds >= 1, OGG_EARG, "sill depths: %d seeds (at least 1)", p->n_seeds);
    OGG_REQUIRE(p->tile_rows >= 0 && p->tile_rows <= TH_MAX, OGG_EARG, "sill depths: tile_rows %d (0: OGG_SILL_TILE_ROWS, or 1 .. %d)",
                p->tile_rows, TH_MAX);
    return OGG_OK;
}

// workspace: parents | east weights | north weights | reach words
struct Layout {
    long par, we, wn, reach, total;
};

Layout layout(const Params& p) {
    const long n = p.ny * p.nx;
    ogg::Sections s{0};
    Layout l;
    l.par = s.take(n * 4);
    l.we = s.take(n * 4);
    l.wn = s.take(n * 4);
    l.reach = s.take(n * 4);
    l.total = s.off;
    return l;
}

}  // namespace

extern "C" long ogg_sill_workspace_bytes(long ny, long nx) {
    if (ny < 1 || nx < 1 || ny > (long)INT_MAX || nx > (long)INT_MAX || ny * nx >= (1L << 31)) return -1;
    return layout(Params{ny, nx, 0, 1, 1, 0}).total;
}

extern "C" int ogg_sill_check(long ny, long nx, int topology, int bits, int n_seeds, int tile_rows) {
    const Params p{ny, nx, topology, bits, n_seeds, tile_rows};
    return check_params(&p);
}

extern "C" int ogg_sill_depth_dev(long ny_, long nx_, int topology, int bits, int n_seeds, int tile_rows, const int* wu, const int* wv,
                                  const long long* seeds, void* workspace, long workspace_bytes, int* b, int* region,
                                  unsigned char* gate_u, unsigned char* gate_v, long long* counts_, void* stream) {
    const Params params{ny_, nx_, topology, bits, n_seeds, tile_rows}, *p = &params;
    Counts* counts = reinterpret_cast<Counts*>(counts_);
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(wu && wv && seeds && b && region && gate_u && gate_v && counts, OGG_EARG,
                "ogg_sill_depth: null wu / wv / seeds / b / region / gate_u / gate_v / counts");
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_sill_depth", workspace, workspace_bytes, l.total)) return e;
    int th = p->tile_rows;
    if (th == 0)
        if (int e = knob("OGG_SILL_TILE_ROWS", TH_DEFAULT, 1, TH_MAX, &th)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const long ny = p->ny, nx = p->nx, n = ny * nx;
    int* par = at<int>(workspace, l.par);
    int* we = at<int>(workspace, l.we);
    int* wn = at<int>(workspace, l.wn);
    int* reach = at<int>(workspace, l.reach);
    int* lo = b;         // the state is the output itself
    int* root = region;  // and the rounds' roots live where the regions will
    const int wmax = (int)((1L << p->bits) - 1);
    const size_t lds = (size_t)TW * th * 4 * sizeof(int);
    const long top = (p->topology & OGG_MASK_FOLD) ? (ny - 1) * nx : LONG_MAX;
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(Counts), st));
    sill_prep_kernel<<<grid_for<NT>(n, COUNT_BLOCKS), NT, 0, st>>>(ny, nx, p->topology, wmax, wu, wv, we, wn, lo, counts);
    OGG_LAUNCH_CHECK();
    sill_seed_kernel<<<grid_for<NT>(p->n_seeds, COUNT_BLOCKS), NT, 0, st>>>(n, p->n_seeds, seeds, lo, counts);
    OGG_LAUNCH_CHECK();
    for (int k = p->bits - 1; k >= 0; --k) {
        const int bit = 1 << k;
        const auto tile = [&](const Grid& g, unsigned tiles) { sill_tile_kernel<false><<<tiles, NT, lds, st>>>(g, bit, lo, we, wn, par, reach); };
        if (int e = label_components<false>(ny, nx, th, p->topology, tile, Passage{lo, we, wn, nx, top, bit, 0}, par, root, nullptr, st))
            return e;
        sill_reach_kernel<<<grid_for<NT>(n, ELEMENT_BLOCKS), NT, 0, st>>>(ny, nx, bit, lo, we, wn, root, reach);
        OGG_LAUNCH_CHECK();
        sill_apply_kernel<<<grid_for<NT>(n, ELEMENT_BLOCKS), NT, 0, st>>>(n, bit, root, reach, lo);
        OGG_LAUNCH_CHECK();
    }
    const auto tile = [&](const Grid& g, unsigned tiles) { sill_tile_kernel<true><<<tiles, NT, lds, st>>>(g, 0, lo, we, wn, par, reach); };
    if (int e = label_components<false>(ny, nx, th, p->topology, tile, Passage{lo, we, wn, nx, top, 0, 1}, par, region, nullptr, st)) return e;
    sill_finish_kernel<<<grid_for<NT>(n, COUNT_BLOCKS), NT, 0, st>>>(ny, nx, p->bits, b, we, wn, region, counts);
    OGG_LAUNCH_CHECK();
    sill_gate_kernel<<<grid_for<NT>(ny * (nx + 1) + (ny + 1) * nx, COUNT_BLOCKS), NT, 0, st>>>(ny, nx, p->topology, b, we, wn, gate_u, gate_v,
                                                                                                 counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: everything copied to device memory, the call, the results copied back (synchronous)
extern "C" int ogg_sill_depth(long ny, long nx, int topology, int bits, int n_seeds, int tile_rows, const int* wu, const int* wv,
                              const long long* seeds, int* b, int* region, unsigned char* gate_u, unsigned char* gate_v,
                              long long* counts) {
    const Params params{ny, nx, topology, bits, n_seeds, tile_rows}, *p = &params;
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(wu && wv && seeds && b && region && gate_u && gate_v && counts, OGG_EARG, "ogg_sill_depth: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t nc = (size_t)(p->ny * p->nx), nu = (size_t)(p->ny * (p->nx + 1)), nv = (size_t)((p->ny + 1) * p->nx);
    const long wsb = layout(*p).total;
    int *du, *dv, *db, *dr;
    long long* ds;
    unsigned char *gu, *gv;
    char* ws;
    long long* ct;
    if (int e = bufs.put(&du, wu, nu)) return e;
    if (int e = bufs.put(&dv, wv, nv)) return e;
    if (int e = bufs.put(&ds, seeds, (size_t)p->n_seeds)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&db, nc)) return e;
    if (int e = bufs.alloc(&dr, nc)) return e;
    if (int e = bufs.alloc(&gu, nu)) return e;
    if (int e = bufs.alloc(&gv, nv)) return e;
    if (int e = bufs.alloc(&ct, (size_t)OGG_SILL_COUNT_WORDS)) return e;
    if (int e = ogg_sill_depth_dev(ny, nx, topology, bits, n_seeds, tile_rows, du, dv, ds, ws, wsb, db, dr, gu, gv, ct, nullptr)) return e;
    if (int e = bufs.get(b, db, nc)) return e;
    if (int e = bufs.get(region, dr, nc)) return e;
    if (int e = bufs.get(gate_u, gu, nu)) return e;
    if (int e = bufs.get(gate_v, gv, nv)) return e;
    if (int e = bufs.get(counts, ct, (size_t)OGG_SILL_COUNT_WORDS)) return e;
    return OGG_OK;
}
