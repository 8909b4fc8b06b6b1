// Processor layouts and mask tables (include/ogg_hip.h, "Processor layouts and mask tables"): the summed-area table of the wet bytes,
// the record of every candidate layout (one workgroup per candidate) and the per-block counts of one layout.
//
// Table: S is (ny + 1) x (nx + 1) int32, S[j][i] the wet cells in rows < j and columns < i.  row_scan_kernel writes the prefix of
// every row (one wavefront per row: shuffles within 64 columns, a carry along the row); the column pass then runs over tiles of
// TILE rows: band_sum_kernel sums a tile's rows per column, band_scan_kernel turns the tile sums into the sums of the tiles below
// (one thread per column, serial over the tiles), band_add_kernel runs down the rows of a tile from that base.  All integers.
//
// Sweep: a workgroup forms the begins of both axes in LDS (lane 0 of wavefront 0 the x axis, lane 0 of wavefront 1 the y axis: the
// rule is serial), its threads walk the blocks, each reading the table at the corners of its own rectangle and of its neighbourhood's
// rectangles; the record is reduced per wavefront, then in LDS, then written once.  No waiting between workgroups, no atomics.
#include <climits>
#include <cstring>
#include <vector>

#include "ogg_common.h"

using ogg::at;
using ogg::grid_for;
using ogg::knob;

namespace {

constexpr int NT = 256;
constexpr int MAXD = OGG_LAYOUT_MAX_DIV;
constexpr long HEAD = 256;
constexpr int TILE_MIN = 4, TILE_MAX = 1024, TILE_DEFAULT = 32;

static_assert(sizeof(ogg_layout_params) == 24, "ogg_layout_params layout");
static_assert(sizeof(ogg_layout_candidate) == 8, "ogg_layout_candidate layout");
static_assert(sizeof(ogg_layout_record) == 40, "ogg_layout_record layout");

// ---- the extent rule ---------------------------------------------------------------------------------------------------
// ceil(a / d) for a >= 0, d >= 1, without the overflow of a + d - 1
__host__ __device__ inline int ceil_div(int a, int d) {
    const int q = (int)((unsigned)a / (unsigned)d);
    return q * d == a ? q : q + 1;
}

__host__ __device__ inline int imax2(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline int imin2(int a, int b) { return a < b ? a : b; }
__device__ inline long lmax2(long a, long b) { return a > b ? a : b; }
__device__ inline long lmin2(long a, long b) { return a < b ? a : b; }

struct ExtentStats {
    int max_size, min_size;
};

// The rule of the header with the begins alone: begin has ndivs + 1 entries, begin[ndivs] = npts, and end[nd] is begin[nd + 1] - 1
// (the rule gives a partition).  1 <= ndivs <= npts.  The one body of ogg_layout_extent and of the sweep kernel.
__host__ __device__ inline ExtentStats extent_begins(int npts, int ndivs, int* begin) {
    const int ieg = npts - 1;
    const bool sym = ((ndivs & 1) && !(npts & 1)) ? (ndivs < npts / 2) : ((ndivs & 1) == (npts & 1));
    int is = 0, imax = ieg, ndmax = ndivs;
    ExtentStats st{0, INT_MAX};
    begin[ndivs] = npts;
    for (int nd = 0; nd < ndivs; ++nd) {
        int ie;
        if (nd < (ndivs - 1) / 2 + 1) {
            ie = is + ceil_div(imax - is + 1, ndmax - nd) - 1;
            const int m = ndivs - 1 - nd;
            if (m > nd && sym) {
                begin[m] = imax2(ieg - ie, ie + 1);   // its end, max(ieg - is, ie + 1), is begin[m + 1] - 1
                imax = begin[m] - 1;
                --ndmax;
            }
        } else if (sym) {
            is = begin[nd];
            ie = begin[nd + 1] - 1;
        } else {
            ie = is + ceil_div(imax - is + 1, ndmax - nd) - 1;
        }
        begin[nd] = is;
        st.max_size = imax2(st.max_size, ie - is + 1);
        st.min_size = imin2(st.min_size, ie - is + 1);
        is = ie + 1;
    }
    return st;
}

// ---- the table -----------------------------------------------------------------------------------------------------------
// the prefix of every row of wet into rows 1 .. ny of S, zeros into row 0 and column 0: one wavefront per row at a time
__global__ __launch_bounds__(NT) void row_scan_kernel(const unsigned char* __restrict__ wet, int ny, int nx, int* __restrict__ S) {
    const int lane = threadIdx.x & 63, ld = nx + 1;
    const long wave = (long)blockIdx.x * (NT / 64) + threadIdx.x / 64, nwaves = (long)gridDim.x * (NT / 64);
    for (long j = wave; j <= ny; j += nwaves) {
        int* row = S + j * ld;
        if (j == 0) {
            for (int i = lane; i < ld; i += 64) row[i] = 0;
            continue;
        }
        const unsigned char* w = wet + (j - 1) * (long)nx;
        if (lane == 0) row[0] = 0;
        int carry = 0;
        for (int c0 = 0; c0 < nx; c0 += 64) {
            const int i = c0 + lane;
            int v = (i < nx && w[i] != 0) ? 1 : 0;
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
            }
            if (i < nx) row[i + 1] = carry + v;
            carry += __shfl(v, 63, 64);
        }
    }
}

// band[t][i] = the sum over the rows of tile t (rows 1 + t * tile .. of S) of the row prefixes in column i
__global__ __launch_bounds__(NT) void band_sum_kernel(const int* __restrict__ S, int ny, int ld, int tile, int nt, int* __restrict__ band) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= ld) return;
    for (int t = blockIdx.y; t < nt; t += gridDim.y) {
        const int j0 = 1 + t * tile, j1 = min(j0 + tile, ny + 1);
        int s = 0;
        for (int j = j0; j < j1; ++j) s += S[(long)j * ld + i];
        band[(long)t * ld + i] = s;
    }
}

// band[t][i] = the sum of the tiles below t, per column
__global__ __launch_bounds__(NT) void band_scan_kernel(int nt, int ld, int* __restrict__ band) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= ld) return;
    int run = 0;
    for (int t = 0; t < nt; ++t) {
        const int v = band[(long)t * ld + i];
        band[(long)t * ld + i] = run;
        run += v;
    }
}

// down the rows of a tile from its base: the row prefixes become the table
__global__ __launch_bounds__(NT) void band_add_kernel(int* __restrict__ S, int ny, int ld, int tile, int nt, const int* __restrict__ band) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= ld) return;
    for (int t = blockIdx.y; t < nt; t += gridDim.y) {
        const int j0 = 1 + t * tile, j1 = min(j0 + tile, ny + 1);
        int run = band[(long)t * ld + i];
        for (int j = j0; j < j1; ++j) {
            run += S[(long)j * ld + i];
            S[(long)j * ld + i] = run;
        }
    }
}

// ---- counts from the table -------------------------------------------------------------------------------------------------
struct Grid {
    int ny, nx, periodic, fold, halo;
    const int* S;
};

// the wet cells of rows j0 .. j1, columns i0 .. i1 (inside the grid; an empty range gives 0)
__device__ inline int rect(const Grid& g, int j0, int j1, int i0, int i1) {
    if (j1 < j0 || i1 < i0) return 0;
    const long ld = g.nx + 1;
    const int* lo = g.S + j0 * ld;
    const int* hi = g.S + (j1 + 1) * ld;
    return (hi[i1 + 1] - lo[i1 + 1]) - (hi[i0] - lo[i0]);
}

// the wet cells of the neighbourhood of the block of rows by .. ey and columns bx .. ex, each cell once
__device__ inline int neighbourhood(const Grid& g, int by, int ey, int bx, int ex) {
    const long h = g.halo;
    const int r0 = (int)lmax2((long)by - h, 0L), r1 = (int)lmin2((long)ey + h, (long)g.ny - 1);
    // the columns: at most two intervals
    int a0[2], a1[2], na = 1;
    const long cl = bx - h, cr = ex + h;
    if (!g.periodic) {
        a0[0] = (int)lmax2(cl, 0L);
        a1[0] = (int)lmin2(cr, (long)g.nx - 1);
    } else if (cr - cl + 1 >= g.nx) {
        a0[0] = 0;
        a1[0] = g.nx - 1;
    } else {   // narrower than the grid, so -nx < cl and cr < 2 nx
        const int l = (int)(cl < 0 ? cl + g.nx : cl), r = (int)(cr >= g.nx ? cr - g.nx : cr);
        if (l <= r) {
            a0[0] = l;
            a1[0] = r;
        } else {
            a0[0] = l;
            a1[0] = g.nx - 1;
            a0[1] = 0;
            a1[1] = r;
            na = 2;
        }
    }
    int n = 0;
    for (int k = 0; k < na; ++k) n += rect(g, r0, r1, a0[k], a1[k]);
    const long past = (long)ey + h - g.ny;   // rows ny .. ny + past lie past the fold
    if (g.fold && past >= 0) {
        const int f0 = (int)lmax2((long)g.ny - 1 - past, 0L), f1 = g.ny - 1;   // they map to rows f0 .. f1, columns mirrored
        const int o0 = max(f0, r0);                                         // r1 = ny - 1 here: rows o0 .. f1 are in both parts
        for (int k = 0; k < na; ++k) {
            const int m0 = g.nx - 1 - a1[k], m1 = g.nx - 1 - a0[k];
            n += rect(g, f0, f1, m0, m1);
            for (int q = 0; q < na; ++q) n -= rect(g, o0, f1, max(m0, a0[q]), min(m1, a1[q]));
        }
    }
    return n;
}

// ---- the sweep -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void sweep_kernel(Grid g, const ogg_layout_candidate* __restrict__ cand, long n,
                                                   ogg_layout_record* __restrict__ rec) {
    __shared__ int bx[MAXD + 1], by[MAXD + 1];
    __shared__ ExtentStats stat[2];
    __shared__ int asym;
    __shared__ int part[NT / 64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid / 64;
    for (long c = blockIdx.x; c < n; c += gridDim.x) {
        const int px = cand[c].px, py = cand[c].py;
        if (px < 1 || py < 1 || px > g.nx || py > g.ny || px > MAXD || py > MAXD) {   // the same for every thread
            if (tid == 0) {
                ogg_layout_record r = {};
                r.status = OGG_LAYOUT_TOO_FINE;
                rec[c] = r;
            }
            continue;
        }
        if (tid == 0) {
            stat[0] = extent_begins(g.nx, px, bx);
            asym = 0;
        }
        if (tid == 64) stat[1] = extent_begins(g.ny, py, by);
        __syncthreads();
        if (g.fold)
            for (int a = tid; a < px; a += NT)
                if (bx[a] + (bx[px - a] - 1) != g.nx - 1) asym = 1;   // every writer writes the same value
        const int nblk = px * py;
        int masked = 0, max_wet = 0, masked_cells = 0;
        for (int k = tid; k < nblk; k += NT) {
            const int b = k / px, a = k - b * px;
            const int x0 = bx[a], x1 = bx[a + 1] - 1, y0 = by[b], y1 = by[b + 1] - 1;
            const int own = rect(g, y0, y1, x0, x1);
            const int nbr = g.halo == 0 ? own : neighbourhood(g, y0, y1, x0, x1);
            max_wet = max(max_wet, own);
            if (nbr == 0) {
                ++masked;
                masked_cells += (x1 - x0 + 1) * (y1 - y0 + 1);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            masked += __shfl_xor(masked, off, 64);
            masked_cells += __shfl_xor(masked_cells, off, 64);
            max_wet = max(max_wet, __shfl_xor(max_wet, off, 64));
        }
        if (lane == 0) {
            part[wave][0] = masked;
            part[wave][1] = masked_cells;
            part[wave][2] = max_wet;
        }
        __syncthreads();
        if (tid == 0) {
            ogg_layout_record r = {};
            for (int w = 0; w < NT / 64; ++w) {
                r.masked += part[w][0];
                r.masked_cells += part[w][1];
                r.max_wet = max(r.max_wet, part[w][2]);
            }
            r.blocks = nblk;
            r.pes = nblk - r.masked;
            r.max_block_cells = stat[0].max_size * stat[1].max_size;
            r.max_block_edge = stat[0].max_size + stat[1].max_size;
            r.min_block_size = min(stat[0].min_size, stat[1].min_size);
            r.wet_total = g.S[(long)g.ny * (g.nx + 1) + g.nx];
            r.status = asym ? OGG_LAYOUT_FOLD_ASYMMETRIC : 0;
            rec[c] = r;
        }
        __syncthreads();   // the LDS is formed anew for the next candidate
    }
}

// wet(a, b) and nbr(a, b) of the blocks of one layout whose begins (px + 1 and py + 1 entries) lie in device memory
__global__ __launch_bounds__(NT) void blocks_kernel(Grid g, int px, int py, const int* __restrict__ bx, const int* __restrict__ by,
                                                    int* __restrict__ block_wet, int* __restrict__ block_nbr) {
    const long nblk = (long)px * py;
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < nblk; k += (long)gridDim.x * NT) {
        const int b = (int)(k / px), a = (int)(k - (long)b * px);
        const int x0 = bx[a], x1 = bx[a + 1] - 1, y0 = by[b], y1 = by[b + 1] - 1;
        const int own = rect(g, y0, y1, x0, x1);
        block_wet[k] = own;
        block_nbr[k] = g.halo == 0 ? own : neighbourhood(g, y0, y1, x0, x1);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int check_params(const ogg_layout_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "layouts: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "layouts: %ld x %ld cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "layouts: topology flags %d", p->topology);
    OGG_REQUIRE(p->halo >= 0, OGG_EARG, "layouts: halo %d: it must be >= 0", p->halo);
    return OGG_OK;
}

int check_candidates(const ogg_layout_candidate* c, long n) {
    OGG_REQUIRE(n >= 0 && n <= (long)OGG_LAYOUT_MAX_CANDIDATES, OGG_EARG, "layouts: %ld candidates: 0 .. %d", n, OGG_LAYOUT_MAX_CANDIDATES);
    OGG_REQUIRE(c || n == 0, OGG_EARG, "layouts: null candidates");
    for (long k = 0; k < n; ++k)
        OGG_REQUIRE(c[k].px >= 1 && c[k].py >= 1, OGG_EARG, "layouts: candidate %ld is %d x %d: px, py >= 1", k, c[k].px, c[k].py);
    return OGG_OK;
}

// workspace: head | table | tile sums (for the smallest tile) | the begins of ogg_layout_blocks_dev
struct Layout {
    long table, band, begins, total;
};

Layout layout(const ogg_layout_params& p) {
    Layout l;
    ogg::Sections s{HEAD};
    l.table = s.take((p.ny + 1) * (p.nx + 1) * 4);
    l.band = s.take(((p.ny + TILE_MIN - 1) / TILE_MIN) * (p.nx + 1) * 4);
    l.begins = s.take(2L * (MAXD + 1) * 4);
    l.total = s.off;
    return l;
}

Grid grid_of(const ogg_layout_params& p, const void* ws) {
    return Grid{(int)p.ny, (int)p.nx, (p.topology & OGG_MASK_PERIODIC) ? 1 : 0, (p.topology & OGG_MASK_FOLD) ? 1 : 0, p.halo,
                at<int>(ws, layout(p).table)};
}

// the begins (ndivs + 1 entries) of one axis: the rule's, or the caller's after their checks
int axis_begins(const char* axis, long npts, int ndivs, const int* given, std::vector<int>* out) {
    OGG_REQUIRE(ndivs >= 1 && ndivs <= MAXD && ndivs <= npts, OGG_EARG, "ogg_layout_blocks: %d blocks along %s of %ld cells: 1 .. min(%d, cells)",
                ndivs, axis, npts, MAXD);
    out->assign(ndivs + 1, 0);
    if (!given) {
        (void)extent_begins((int)npts, ndivs, out->data());
        return OGG_OK;
    }
    for (int k = 0; k < ndivs; ++k) {
        OGG_REQUIRE(given[k] < npts && (k == 0 ? given[k] == 0 : given[k] > given[k - 1]), OGG_EARG,
                    "ogg_layout_blocks: %s begin %d is %d: the begins rise strictly from 0 and stay below %ld", axis, k, given[k], npts);
        (*out)[k] = given[k];
    }
    (*out)[ndivs] = (int)npts;
    return OGG_OK;
}

}  // namespace

extern "C" int ogg_layout_extent(long npts, long ndivs, int* begin, int* end) {
    OGG_REQUIRE(npts >= 1 && npts <= (long)INT_MAX && ndivs >= 1 && ndivs <= npts, OGG_EARG,
                "ogg_layout_extent: %ld blocks of %ld points: 1 <= ndivs <= npts < 2^31", ndivs, npts);
    OGG_REQUIRE(begin, OGG_EARG, "ogg_layout_extent: null begin");
    std::vector<int> b((size_t)ndivs + 1);
    (void)extent_begins((int)npts, (int)ndivs, b.data());
    for (long k = 0; k < ndivs; ++k) {
        begin[k] = b[k];
        if (end) end[k] = b[k + 1] - 1;
    }
    return OGG_OK;
}

extern "C" int ogg_layout_check(const ogg_layout_params* p, const ogg_layout_candidate* candidates, long n) {
    if (int e = check_params(p)) return e;
    return check_candidates(candidates, n);
}

extern "C" long ogg_layout_workspace_bytes(const ogg_layout_params* p) {
    if (!p || check_params(p) != OGG_OK) return -1;
    return layout(*p).total;
}

extern "C" int ogg_layout_table_dev(const ogg_layout_params* p, const unsigned char* wet, void* workspace, long workspace_bytes,
                                    void* stream) {
    if (int e = check_params(p)) return e;
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_layout_table", workspace, workspace_bytes, l.total)) return e;
    OGG_REQUIRE(wet, OGG_EARG, "ogg_layout_table: null wet");
    int tile;
    if (int e = knob("OGG_LAYOUT_TILE_ROWS", TILE_DEFAULT, TILE_MIN, TILE_MAX, &tile)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const int ny = (int)p->ny, nx = (int)p->nx, ld = nx + 1, nt = (ny + tile - 1) / tile;
    int* S = at<int>(workspace, l.table);
    int* band = at<int>(workspace, l.band);
    row_scan_kernel<<<grid_for<NT / 64>(ny + 1, 8192), NT, 0, st>>>(wet, ny, nx, S);
    OGG_LAUNCH_CHECK();
    const dim3 tiles((unsigned)((ld + NT - 1) / NT), (unsigned)std::min(nt, 65535));
    band_sum_kernel<<<tiles, NT, 0, st>>>(S, ny, ld, tile, nt, band);
    OGG_LAUNCH_CHECK();
    band_scan_kernel<<<tiles.x, NT, 0, st>>>(nt, ld, band);
    OGG_LAUNCH_CHECK();
    band_add_kernel<<<tiles, NT, 0, st>>>(S, ny, ld, tile, nt, band);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_layout_sweep_dev(const ogg_layout_params* p, const ogg_layout_candidate* candidates, long n, const void* workspace,
                                    long workspace_bytes, ogg_layout_record* records, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_layout_sweep", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(n >= 0 && n <= (long)OGG_LAYOUT_MAX_CANDIDATES, OGG_EARG, "ogg_layout_sweep: %ld candidates: 0 .. %d", n,
                OGG_LAYOUT_MAX_CANDIDATES);
    OGG_REQUIRE((candidates && records) || n == 0, OGG_EARG, "ogg_layout_sweep: null candidates / records");
    int groups;
    if (int e = knob("OGG_LAYOUT_GRID", 0, 0, OGG_LAYOUT_MAX_CANDIDATES, &groups)) return e;
    if (n == 0) return OGG_OK;
    const long grid = groups > 0 ? std::min<long>(groups, n) : n;
    sweep_kernel<<<(unsigned)grid, NT, 0, ogg::as_stream(stream)>>>(grid_of(*p, workspace), candidates, n, records);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_layout_blocks_dev(const ogg_layout_params* p, int px, int py, const int* xbegin, const int* ybegin, void* workspace,
                                     long workspace_bytes, int* block_wet, int* block_nbr, void* stream) {
    if (int e = check_params(p)) return e;
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_layout_blocks", workspace, workspace_bytes, l.total)) return e;
    OGG_REQUIRE(block_wet && block_nbr, OGG_EARG, "ogg_layout_blocks: null block_wet / block_nbr");
    std::vector<int> bx, by;
    if (int e = axis_begins("x", p->nx, px, xbegin, &bx)) return e;
    if (int e = axis_begins("y", p->ny, py, ybegin, &by)) return e;
    hipStream_t st = ogg::as_stream(stream);
    int* dbx = at<int>(workspace, l.begins);
    int* dby = dbx + (MAXD + 1);
    OGG_HIP_CHECK(hipMemcpyAsync(dbx, bx.data(), bx.size() * sizeof(int), hipMemcpyHostToDevice, st));
    OGG_HIP_CHECK(hipMemcpyAsync(dby, by.data(), by.size() * sizeof(int), hipMemcpyHostToDevice, st));
    OGG_HIP_CHECK(hipStreamSynchronize(st));   // bx, by are this call's own: they must outlive the copies
    blocks_kernel<<<grid_for<NT>((long)px * py, 4096), NT, 0, st>>>(grid_of(*p, workspace), px, py, dbx, dby, block_wet, block_nbr);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: everything copied to device memory, the steps, the results copied back (synchronous)
extern "C" int ogg_layouts(const ogg_layout_params* p, const unsigned char* wet, const ogg_layout_candidate* candidates, long n,
                           ogg_layout_record* records, int px, int py, const int* xbegin, const int* ybegin, int* block_wet,
                           int* block_nbr) {
    if (int e = check_params(p)) return e;
    if (int e = check_candidates(candidates, n)) return e;
    OGG_REQUIRE(wet && (records || n == 0), OGG_EARG, "ogg_layouts: null wet / records");
    OGG_REQUIRE((block_wet == nullptr) == (block_nbr == nullptr), OGG_EARG, "ogg_layouts: block_wet and block_nbr go together");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t nc = (size_t)(p->ny * p->nx);
    const long wsb = layout(*p).total;
    unsigned char* dw;
    char* ws;
    if (int e = bufs.put(&dw, wet, nc)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = ogg_layout_table_dev(p, dw, ws, wsb, nullptr)) return e;
    if (n > 0) {
        ogg_layout_candidate* dc;
        ogg_layout_record* dr;
        if (int e = bufs.put(&dc, candidates, (size_t)n)) return e;
        if (int e = bufs.alloc(&dr, (size_t)n)) return e;
        if (int e = ogg_layout_sweep_dev(p, dc, n, ws, wsb, dr, nullptr)) return e;
        if (int e = bufs.get(records, dr, (size_t)n)) return e;
    }
    if (block_wet) {
        int *dbw, *dbn;
        OGG_REQUIRE(px >= 1 && py >= 1 && px <= MAXD && py <= MAXD, OGG_EARG, "ogg_layouts: the layout %d x %d: 1 .. %d", px, py, MAXD);
        const size_t nb = (size_t)px * py;
        if (int e = bufs.alloc(&dbw, nb)) return e;
        if (int e = bufs.alloc(&dbn, nb)) return e;
        if (int e = ogg_layout_blocks_dev(p, px, py, xbegin, ybegin, ws, wsb, dbw, dbn, nullptr)) return e;
        if (int e = bufs.get(block_wet, dbw, nb)) return e;
        if (int e = bufs.get(block_nbr, dbn, nb)) return e;
    }
    OGG_HIP_CHECK(hipDeviceSynchronize());
    return OGG_OK;
}
