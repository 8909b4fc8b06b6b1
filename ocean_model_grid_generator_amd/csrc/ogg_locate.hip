// Point location and sampling (include/ogg_hip.h, "Point location"): for every query point the model cell that holds it by the key
// m_c(p) = min over the cell's four great-circle edges of sigma T(p; edge), its fractional position (s, t), and a model field there.
//
// sets      the corner table cu (unit() of ogg_sphere.h at the canonical copy of every corner) and one record per cell: sigma times
//           the four edge normals (T(p; sigma n) = sigma T(p; n) up to the sign of an exact zero, so the search needs no sigma; the
//           winner's m is formed again as sigma T(p; n) at the end) and the padded box.  A cell
//           that holds no point (O zero or not finite) gets an empty box and is never registered.
// index     the cube grid of ogg_box_index.h (shared with the curvilinear exchange grid): every cell registered in every cube its box touches, by count -> exclusive_scan ->
//           fill (ogg_blocks.h); a cell that touches more than OGG_LOCATE_MAX_TOUCH cubes goes on the large-cells list, which every
//           query tests.  p in a cell's box implies cube_of(lo) <= cube_of(p) <= cube_of(hi) on every axis (cube_of is monotone), so
//           the cube of p together with the large list holds every candidate of p: the search equals the brute-force argmax.
//           OGG_LOCATE_BRUTE=1 puts every cell on the large list.
// search    the queries' unit vectors, a counting sort of the query indices by cube, then one workgroup per NT consecutive sorted
//           queries: the cubes met in that run are taken one after the other, the cube's records staged through LDS in chunks, and
//           the lanes of that cube test every record (box first, then the four measures) and keep the best (m, c).  The key makes the
//           order in which cells are met immaterial.  The winners' (s, t) are formed from cu at the end, by original query index.
// sample    one thread per point forms the four cells and weights once and walks the records.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "ogg_blocks.h"
#include "ogg_box_index.h"
#include "ogg_cells.h"
#include "ogg_common.h"
#include "ogg_sphere_bins.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int NT = 256;                 // threads per workgroup (four wavefronts)
constexpr int CH = 128;                 // cell records of one LDS chunk
constexpr int NF = BOX_NF;              // doubles of a cell record: sigma n_S, sigma n_E, sigma n_N, sigma n_W, box lo, box hi
constexpr long HEAD = BOX_HEAD;
constexpr long NBMAX = BOX_NBMAX;
constexpr long long MAGIC = 0x6c6f63617465ll;   // the head of a workspace whose index is built

static_assert(sizeof(ogg_locate_params) == 64, "ogg_locate_params layout");
static_assert(sizeof(ogg_locate_counts) == 80, "ogg_locate_counts layout");
static_assert(NT == BLOCKS_NT, "block_add and block_scan work over a workgroup of BLOCKS_NT threads");

using Head = BoxHead;   // magic: MAGIC + G once the index is built

// ---- the definition's arithmetic -----------------------------------------------------------------------------------
__device__ inline void cross(const double* a, const double* b, double* n) {
    n[0] = a[1] * b[2] - a[2] * b[1];
    n[1] = a[2] * b[0] - a[0] * b[2];
    n[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline double dot3(const double* p, const double* n) { return (p[0] * n[0] + p[1] * n[1]) + p[2] * n[2]; }
__device__ inline bool same_bits(const double* a, const double* b) {
    return bits_of(a[0]) == bits_of(b[0]) && bits_of(a[1]) == bits_of(b[1]) && bits_of(a[2]) == bits_of(b[2]);
}

// the corner index (row stride nx + 1) of the canonical copy of corner (J, I)
__device__ inline long canonical_corner(const CellTopo& t, long J, long I) {
    if (t.periodic && I == t.nx) I = 0;
    if (t.fold && J == t.ny) {
        long M = t.nx - I;
        if (t.periodic && M == t.nx) M = 0;
        if (M < I) I = M;
    }
    return J * (t.nx + 1) + I;
}

// the corners a, b, c, d of cell c0 from the table, the four normals n[0..3] = n_S, n_E, n_N, n_W, and sigma (0: holds no point)
__device__ inline double cell_geometry(const double* __restrict__ cu, long nx, long c0, double (&q)[4][3], double (&n)[4][3]) {
    const long j = c0 / nx, i = c0 % nx, ld = nx + 1;
    const long k[4] = {j * ld + i, j * ld + i + 1, (j + 1) * ld + i + 1, (j + 1) * ld + i};
    for (int v = 0; v < 4; ++v)
        for (int a = 0; a < 3; ++a) q[v][a] = cu[3 * k[v] + a];
    for (int v = 0; v < 4; ++v) cross(q[v], q[(v + 1) & 3], n[v]);
    double sv[3], sn[3];
    for (int a = 0; a < 3; ++a) {
        sv[a] = (q[0][a] + q[1][a]) + (q[2][a] + q[3][a]);
        sn[a] = (n[0][a] + n[1][a]) + (n[2][a] + n[3][a]);
    }
    const double O = dot3(sv, sn);
    if (!isfinite(O)) return 0.0;
    return O > 0.0 ? 1.0 : (O < 0.0 ? -1.0 : 0.0);
}

// ---- sets ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void corner_kernel(CellTopo t, const double* __restrict__ x, const double* __restrict__ y, long ld,
                                                    double* __restrict__ cu) {
    const long n = (t.ny + 1) * (t.nx + 1);
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        const long s = canonical_corner(t, k / (t.nx + 1), k % (t.nx + 1));
        const long J = s / (t.nx + 1), I = s % (t.nx + 1);
        double u[3];
        unit(x[2 * J * ld + 2 * I], y[2 * J * ld + 2 * I], u);
        cu[3 * k] = u[0];
        cu[3 * k + 1] = u[1];
        cu[3 * k + 2] = u[2];
    }
}

__global__ __launch_bounds__(NT) void record_kernel(long ny, long nx, const double* __restrict__ cu, double* __restrict__ rec) {
    const long n = ny * nx;
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        double q[4][3], nn[4][3];
        const double sigma = cell_geometry(cu, nx, c, q, nn);
        double* r = rec + c * NF;
        if (sigma == 0.0) {   // holds no point: an empty box
            for (int f = 0; f < 12; ++f) r[f] = 0.0;
            empty_box(r);
            continue;
        }
        for (int v = 0; v < 4; ++v)
            for (int a = 0; a < 3; ++a) r[3 * v + a] = sigma * nn[v][a];
        padded_box(q, r);
    }
}

// ---- search --------------------------------------------------------------------------------------------------------
// nothing found anywhere, and the search step's counts from zero
__global__ __launch_bounds__(NT) void init_kernel(long n, int* __restrict__ cell, double* __restrict__ s, double* __restrict__ t,
                                                  double* __restrict__ m, ogg_locate_counts* counts) {
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        cell[k] = -1;
        s[k] = t[k] = m[k] = NAN;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts->located = counts->outside = counts->invalid = counts->tests = 0;
}

// qu, and the cube of every query (-1: a coordinate is not finite, or the workspace holds no index) with the cubes' counts
__global__ __launch_bounds__(NT) void query_kernel(long n, const double* __restrict__ lon, const double* __restrict__ lat,
                                                   const Head* head, double* __restrict__ qu, int* __restrict__ qbin,
                                                   int* __restrict__ qcnt, ogg_locate_counts* counts) {
    const long long G = head->G;
    const bool built = G >= 1 && G <= OGG_LOCATE_MAX_CUBES && head->magic == MAGIC + G;
    long long v[1] = {0};
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        double u[3];
        unit(lon[k], lat[k], u);
        qu[3 * k] = u[0];
        qu[3 * k + 1] = u[1];
        qu[3 * k + 2] = u[2];
        const bool ok = isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]);
        int b = -1;
        if (ok && built) {
            b = cube_of(u[0], (int)G) + (int)G * (cube_of(u[1], (int)G) + (int)G * cube_of(u[2], (int)G));
            atomicAdd(&qcnt[b], 1);
        }
        qbin[k] = b;
        v[0] += !ok;
    }
    long long* const dst[1] = {&counts->invalid};
    block_add<1>(v, dst);
}

__global__ __launch_bounds__(NT) void query_fill_kernel(long n, const int* __restrict__ qbin, const int* __restrict__ qstart,
                                                        int* __restrict__ cursor, int* __restrict__ qsorted) {
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        const int b = qbin[k];
        if (b >= 0) qsorted[(long)qstart[b] + atomicAdd(&cursor[b], 1)] = (int)k;
    }
}

struct Chunk {
    double r[NF][CH];
    int c[CH];
};

struct Best {
    double m;
    int cell;
    __device__ inline void offer(double v, int c) { if (v > m || (v == m && c < cell)) m = v, cell = c; }
    __device__ inline bool found() const { return cell != INT_MAX; }
};

// the cells list[s0 .. s1) through LDS, chunk by chunk; the lanes with ``act`` test every one of them.  Called by the whole workgroup
// with the same list, s0 and s1.
__device__ inline void stream(const double* __restrict__ rec, const int* __restrict__ list, Chunk& ch, long s0, long s1, bool act,
                              const double* p, Best& best, long long& tests) {
    for (long base = s0; base < s1; base += CH) {
        const int m = s1 - base < CH ? (int)(s1 - base) : CH;
        __syncthreads();   // the chunk before this one has been read
        for (int r = threadIdx.x; r < m; r += NT) ch.c[r] = list[base + r];
        for (int idx = threadIdx.x; idx < m * NF; idx += NT) {
            const int r = idx / NF, f = idx - r * NF;
            ch.r[f][r] = rec[(long)list[base + r] * NF + f];
        }
        __syncthreads();
        if (act) {
            for (int r = 0; r < m; ++r) {
                if (p[0] >= ch.r[12][r] && p[0] <= ch.r[15][r] && p[1] >= ch.r[13][r] && p[1] <= ch.r[16][r] && p[2] >= ch.r[14][r] &&
                    p[2] <= ch.r[17][r]) {
                    double v = (p[0] * ch.r[0][r] + p[1] * ch.r[1][r]) + p[2] * ch.r[2][r];
                    const double e = (p[0] * ch.r[3][r] + p[1] * ch.r[4][r]) + p[2] * ch.r[5][r];
                    const double nn = (p[0] * ch.r[6][r] + p[1] * ch.r[7][r]) + p[2] * ch.r[8][r];
                    const double w = (p[0] * ch.r[9][r] + p[1] * ch.r[10][r]) + p[2] * ch.r[11][r];
                    if (e < v) v = e;
                    if (nn < v) v = nn;
                    if (w < v) v = w;
                    if (v >= -OGG_LOCATE_TOL) best.offer(v, ch.c[r]);
                }
            }
            tests += m;
        }
    }
}

__device__ inline double fraction(double lo, double hi, bool lo_collapsed, bool hi_collapsed, double lo_sub, double hi_sub) {
    if (lo_collapsed && hi_collapsed) return 0.5;
    if (hi_collapsed) hi = hi_sub - lo;
    if (lo_collapsed) lo = lo_sub - hi;
    const double den = lo + hi;
    if (!(den > 0.0)) return 0.5;
    const double v = lo / den;
    return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

struct Search {
    long nx;
    const Head* head;
    const double* rec;
    const int *start, *entries, *large;
    const int *qstart, *qsorted, *qbin;   // qstart[NBMAX]: the queries that were sorted
};

__global__ __launch_bounds__(NT) void search_kernel(Search g, const double* __restrict__ cu, const double* __restrict__ qu,
                                                    int* __restrict__ cell, double* __restrict__ so, double* __restrict__ to,
                                                    double* __restrict__ mo, ogg_locate_counts* counts) {
    __shared__ Chunk ch;
    __shared__ int cur_s;
    const long nq = g.qstart[NBMAX];
    const long first = (long)blockIdx.x * NT;
    if (first >= nq) return;
    const int mblk = nq - first < NT ? (int)(nq - first) : NT;
    const bool have = (int)threadIdx.x < mblk;
    const long k = have ? g.qsorted[first + threadIdx.x] : 0;
    const int mycube = have ? g.qbin[k] : -1;
    double p[3] = {0.0, 0.0, 0.0};
    if (have) p[0] = qu[3 * k], p[1] = qu[3 * k + 1], p[2] = qu[3 * k + 2];
    Best best{-INFINITY, INT_MAX};
    long long tests = 0;
    stream(g.rec, g.large, ch, 0, (long)g.head->nlarge, have, p, best, tests);
    // the run's queries are sorted by cube: the lanes of the cube of lane e are e .. e + their count - 1
    int e = 0;
    while (e < mblk) {
        if ((int)threadIdx.x == e) cur_s = mycube;
        __syncthreads();
        const int cur = cur_s;
        const bool act = have && mycube == cur;
        stream(g.rec, g.entries, ch, g.start[cur], g.start[cur + 1], act, p, best, tests);
        e += __syncthreads_count(act);
    }
    const bool found = have && best.found();
    if (found) {
        double q[4][3], n[4][3];
        const double sigma = cell_geometry(cu, g.nx, best.cell, q, n);
        const double S = sigma * dot3(p, n[0]), E = sigma * dot3(p, n[1]), N = sigma * dot3(p, n[2]), W = sigma * dot3(p, n[3]);
        const bool cS = same_bits(q[0], q[1]), cE = same_bits(q[1], q[2]), cN = same_bits(q[2], q[3]), cW = same_bits(q[3], q[0]);
        // the key again as the header writes it, sigma T(p; n): T(p; sigma n) of the search is the same number, but an exact zero
        // may carry the other sign
        double mk = S;
        if (E < mk) mk = E;
        if (N < mk) mk = N;
        if (W < mk) mk = W;
        cell[k] = best.cell;
        mo[k] = mk;
        so[k] = fraction(W, E, cW, cE, sigma * dot3(q[0], n[1]), sigma * dot3(q[1], n[3]));
        to[k] = fraction(S, N, cS, cN, sigma * dot3(q[0], n[2]), sigma * dot3(q[2], n[0]));
    }
    long long v[3] = {found ? 1 : 0, have && !found ? 1 : 0, tests};
    long long* const dst[3] = {&counts->located, &counts->outside, &counts->tests};
    block_add<3>(v, dst);
}

// ---- sample --------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void sample_kernel(CellTopo t, long n, long nrec, int mode, const int* __restrict__ cell,
                                                    const double* __restrict__ s, const double* __restrict__ tt,
                                                    const T* __restrict__ f, const unsigned char* __restrict__ wet, T f0, T f1, int nf,
                                                    double* __restrict__ values, unsigned char* __restrict__ flags,
                                                    ogg_locate_counts* counts) {
    const long nc = t.ny * t.nx;
    long long v[4] = {0, 0, 0, 0};
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        const long c = cell[k];
        long idx[4] = {c, -1, -1, -1};
        double w[4] = {1.0, 0.0, 0.0, 0.0};
        const int ncell = mode == OGG_LOCATE_BILINEAR ? 4 : 1;
        if (c >= 0 && mode == OGG_LOCATE_BILINEAR) {
            const double sk = s[k], tk = tt[k];
            const double fx = fabs(sk - 0.5), fy = fabs(tk - 0.5);
            const int ydir = tk >= 0.5 ? 3 : 0;
            long nb[4];
            face_neighbours(t, c, nb);
            idx[1] = nb[sk >= 0.5 ? 2 : 1];
            idx[2] = nb[ydir];
            if (idx[1] >= 0) {
                face_neighbours(t, idx[1], nb);
                idx[3] = nb[ydir];
            }
            const double gx = 1.0 - fx, gy = 1.0 - fy;
            w[0] = gx * gy, w[1] = fx * gy, w[2] = gx * fy, w[3] = fx * fy;
        }
        const bool dry = c >= 0 && wet && !wet[c];
        bool there[4];   // the cell exists and is wet: the same for every record
        for (int q = 0; q < 4; ++q) there[q] = q < ncell && idx[q] >= 0 && !(wet && !wet[idx[q]]);
        for (long r = 0; r < nrec; ++r) {
            int flag = 0;
            double val = OGG_REMAP_FILL;
            if (c >= 0) {
                double W = 0.0, S = 0.0;
                int used = 0;
                if (!dry)
                    for (int q = 0; q < ncell; ++q) {
                        if (!there[q]) continue;
                        const T fv = f[r * nc + idx[q]];
                        if (missing<T>(fv, f0, f1, nf)) continue;
                        W += w[q];
                        S += w[q] * (double)fv;
                        ++used;
                    }
                if (used == 0 || !(W > 0.0))
                    flag = 3;
                else {
                    flag = used == ncell ? 1 : 2;
                    val = S / W;
                }
            }
            values[r * n + k] = val;
            flags[r * n + k] = (unsigned char)flag;
            ++v[flag];
        }
    }
    long long* const dst[4] = {&counts->flag0, &counts->flag1, &counts->flag2, &counts->flag3};
    block_add<4>(v, dst);
}

__global__ void zero_flags_kernel(ogg_locate_counts* counts) { counts->flag0 = counts->flag1 = counts->flag2 = counts->flag3 = 0; }

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_locate_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "locate: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX &&
                    p->ny * p->nx < (1L << 31) / OGG_LOCATE_MAX_TOUCH,
                OGG_EARG, "locate: %ld x %ld cells: ny, nx >= 1 and ny * nx * %d < 2^31", p->ny, p->nx, OGG_LOCATE_MAX_TOUCH);
    OGG_REQUIRE(p->n >= 0 && p->n < (1L << 31), OGG_EARG, "locate: %ld queries: 0 <= n < 2^31", p->n);
    OGG_REQUIRE(p->nrec >= 0, OGG_EARG, "locate: %ld records", p->nrec);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "locate: topology flags %d", p->topology);
    OGG_REQUIRE(p->mode == OGG_LOCATE_CELL || p->mode == OGG_LOCATE_BILINEAR, OGG_EARG, "locate: mode %d (0: cell, 1: bilinear)", p->mode);
    OGG_REQUIRE(p->dtype == OGG_REMAP_FLOAT32 || p->dtype == OGG_REMAP_FLOAT64, OGG_EARG, "locate: dtype %d (0: float32, 1: float64)",
                p->dtype);
    OGG_REQUIRE(p->n_fill >= 0 && p->n_fill <= 2, OGG_EARG, "locate: %d fill values: 0 .. 2", p->n_fill);
    return OGG_OK;
}

long ncell_of(const ogg_locate_params& p) { return p.ny * p.nx; }

// workspace: head | cell records | cube counts | cube starts | block sums | entries | large list | cube of query | sorted queries |
// query cube counts | query cube starts
struct Layout {
    long rec, cnt, start, bsum, entries, large, qbin, qsorted, qcnt, qstart, total;
};

Layout layout(const ogg_locate_params& p) {
    Layout l;
    const long nc = ncell_of(p);
    ogg::Sections s{HEAD};
    l.rec = s.take(nc * NF * 8);
    l.cnt = s.take((NBMAX + 1) * 4);
    l.start = s.take((NBMAX + 1) * 4);
    l.bsum = s.take(((NBMAX + 1) / SCAN_CH + 2) * 8);
    l.entries = s.take(nc * OGG_LOCATE_MAX_TOUCH * 4);
    l.large = s.take(nc * 4);
    l.qbin = s.take(p.n * 4);
    l.qsorted = s.take(p.n * 4);
    l.qcnt = s.take((NBMAX + 1) * 4);
    l.qstart = s.take((NBMAX + 1) * 4);
    l.total = s.off;
    return l;
}

template <typename T>
void launch_sample(const ogg_locate_params* p, const int* cell, const double* s, const double* t, const void* f,
                   const unsigned char* wet, double* values, unsigned char* flags, ogg_locate_counts* counts, hipStream_t st) {
    sample_kernel<T><<<grid_for<NT>(p->n, 1 << 20), NT, 0, st>>>(cell_topo(p->ny, p->nx, p->topology), p->n, p->nrec, p->mode, cell, s, t,
                                                                 static_cast<const T*>(f), wet, (T)p->fill[0], (T)p->fill[1], p->n_fill,
                                                                 values, flags, counts);
}

}  // namespace

extern "C" long ogg_locate_workspace_bytes(const ogg_locate_params* p) {
    if (!p || check_params(p) != OGG_OK) return -1;
    return layout(*p).total;
}

extern "C" int ogg_locate_check(const ogg_locate_params* p) { return check_params(p); }

extern "C" int ogg_locate_sets_dev(const ogg_locate_params* p, const double* x, const double* y, long ld, void* workspace,
                                   long workspace_bytes, double* cu, ogg_locate_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_locate_sets", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(x && y && cu && counts, OGG_EARG, "ogg_locate_sets: null x / y / cu / counts");
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_locate_sets: row stride %ld < 2 nx + 1", ld);
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_locate_counts), st));
    OGG_HIP_CHECK(hipMemsetAsync(workspace, 0, HEAD, st));   // no index yet
    corner_kernel<<<grid_for<NT>((p->ny + 1) * (p->nx + 1), 4096), NT, 0, st>>>(cell_topo(p->ny, p->nx, p->topology), x, y, ld, cu);
    OGG_LAUNCH_CHECK();
    record_kernel<<<grid_for<NT>(ncell_of(*p), 4096), NT, 0, st>>>(p->ny, p->nx, cu, at<double>(workspace, l.rec));
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_locate_index_dev(const ogg_locate_params* p, void* workspace, long workspace_bytes, ogg_locate_counts* counts,
                                    void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_locate_index", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(counts, OGG_EARG, "ogg_locate_index: null counts");
    int brute, cubes;
    // OGG_LOCATE_BRUTE=1: every cell that can hold a point is tested for every query (the cross-check of the index)
    if (int e = knob("OGG_LOCATE_BRUTE", 0, 0, 1, &brute)) return e;
    // OGG_LOCATE_CUBES: cubes per axis of the index; 0: from the cell count, about eight cells across a cube
    if (int e = knob("OGG_LOCATE_CUBES", 0, 0, OGG_LOCATE_MAX_CUBES, &cubes)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    const long nc = ncell_of(*p);
    const int G = brute ? 1 : (cubes > 0 ? cubes : box_default_cubes(nc));
    return build_box_index(nc, at<double>(workspace, l.rec), G, brute, at<Head>(workspace, 0), MAGIC, workspace,
                           BoxIndexLayout{l.cnt, l.start, l.entries, l.large}, at<long long>(workspace, l.bsum), &counts->large_cells,
                           &counts->cubes, st);
}

extern "C" int ogg_locate_search_dev(const ogg_locate_params* p, const double* cu, const double* lon, const double* lat, void* workspace,
                                     long workspace_bytes, double* qu, int* cell, double* s, double* t, double* m,
                                     ogg_locate_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_locate_search", workspace, workspace_bytes, layout(*p).total)) return e;
    OGG_REQUIRE(cu && counts && ((lon && lat && qu && cell && s && t && m) || p->n == 0), OGG_EARG,
                "ogg_locate_search: null cu / lon / lat / qu / cell / s / t / m / counts");
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p);
    const Head* head = at<Head>(workspace, 0);
    int *qbin = at<int>(workspace, l.qbin), *qsorted = at<int>(workspace, l.qsorted), *qcnt = at<int>(workspace, l.qcnt);
    int* qstart = at<int>(workspace, l.qstart);
    init_kernel<<<grid_for<NT>(p->n, 4096), NT, 0, st>>>(p->n, cell, s, t, m, counts);
    OGG_LAUNCH_CHECK();
    if (p->n == 0) return OGG_OK;
    OGG_HIP_CHECK(hipMemsetAsync(qcnt, 0, (size_t)(NBMAX + 1) * 4, st));
    query_kernel<<<grid_for<NT>(p->n, 4096), NT, 0, st>>>(p->n, lon, lat, head, qu, qbin, qcnt, counts);
    OGG_LAUNCH_CHECK();
    // the cubes' starts in the sorted list; entry NBMAX: the queries that have a cube
    if (int e = exclusive_scan<true>(qcnt, NBMAX, at<long long>(workspace, l.bsum), nullptr, qstart, st)) return e;
    OGG_HIP_CHECK(hipMemsetAsync(qcnt, 0, (size_t)(NBMAX + 1) * 4, st));   // the cursors of the fill
    query_fill_kernel<<<grid_for<NT>(p->n, 4096), NT, 0, st>>>(p->n, qbin, qstart, qcnt, qsorted);
    OGG_LAUNCH_CHECK();
    const Search g{p->nx, head, at<double>(workspace, l.rec), at<int>(workspace, l.start), at<int>(workspace, l.entries),
                   at<int>(workspace, l.large), qstart, qsorted, qbin};
    search_kernel<<<(unsigned)((p->n + NT - 1) / NT), NT, 0, st>>>(g, cu, qu, cell, s, t, m, counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_locate_sample_dev(const ogg_locate_params* p, const int* cell, const double* s, const double* t, const void* f,
                                     const unsigned char* wet, double* values, unsigned char* flags, ogg_locate_counts* counts,
                                     void* stream) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(p->nrec >= 1, OGG_EARG, "ogg_locate_sample: %ld records: at least one", p->nrec);
    OGG_REQUIRE(f && counts && ((cell && s && t && values && flags) || p->n == 0), OGG_EARG,
                "ogg_locate_sample: null cell / s / t / f / values / flags / counts");
    hipStream_t st = ogg::as_stream(stream);
    zero_flags_kernel<<<1, 1, 0, st>>>(counts);
    OGG_LAUNCH_CHECK();
    if (p->n == 0) return OGG_OK;
    if (p->dtype == OGG_REMAP_FLOAT32)
        launch_sample<float>(p, cell, s, t, f, wet, values, flags, counts, st);
    else
        launch_sample<double>(p, cell, s, t, f, wet, values, flags, counts, st);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer forms: everything copied to device memory, the steps, the results copied back (synchronous)
extern "C" int ogg_locate(const ogg_locate_params* p, const double* x, const double* y, const double* lon, const double* lat, int* cell,
                          double* s, double* t, double* m, double* cu, double* qu, ogg_locate_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(x && y && counts && ((lon && lat && cell && s && t && m) || p->n == 0), OGG_EARG, "ogg_locate: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t n = (size_t)p->n, npt = (size_t)(2 * p->ny + 1) * (2 * p->nx + 1), ncor = (size_t)(p->ny + 1) * (p->nx + 1);
    const long wsb = layout(*p).total;
    double *dx, *dy, *dlon, *dlat, *dcu, *dqu, *ds, *dt, *dm;
    int* dc;
    char* ws;
    ogg_locate_counts* ct;
    if (int e = bufs.put(&dx, x, npt)) return e;
    if (int e = bufs.put(&dy, y, npt)) return e;
    if (int e = bufs.put(&dlon, lon, n)) return e;
    if (int e = bufs.put(&dlat, lat, n)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&dcu, ncor * 3)) return e;
    if (int e = bufs.alloc(&dqu, n * 3)) return e;
    if (int e = bufs.alloc(&dc, n)) return e;
    if (int e = bufs.alloc(&ds, n)) return e;
    if (int e = bufs.alloc(&dt, n)) return e;
    if (int e = bufs.alloc(&dm, n)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = ogg_locate_sets_dev(p, dx, dy, 2 * p->nx + 1, ws, wsb, dcu, ct, nullptr)) return e;
    if (int e = ogg_locate_index_dev(p, ws, wsb, ct, nullptr)) return e;
    if (int e = ogg_locate_search_dev(p, dcu, dlon, dlat, ws, wsb, dqu, dc, ds, dt, dm, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(cell, dc, n)) return e;
    if (int e = bufs.get(s, ds, n)) return e;
    if (int e = bufs.get(t, dt, n)) return e;
    if (int e = bufs.get(m, dm, n)) return e;
    if (cu)
        if (int e = bufs.get(cu, dcu, ncor * 3)) return e;
    if (qu)
        if (int e = bufs.get(qu, dqu, n * 3)) return e;
    return OGG_OK;
}

extern "C" int ogg_locate_sample(const ogg_locate_params* p, const int* cell, const double* s, const double* t, const void* f,
                                 const unsigned char* wet, double* values, unsigned char* flags, ogg_locate_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(p->nrec >= 1, OGG_EARG, "ogg_locate_sample: %ld records: at least one", p->nrec);
    OGG_REQUIRE(f && counts && ((cell && s && t && values && flags) || p->n == 0), OGG_EARG, "ogg_locate_sample: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t n = (size_t)p->n, nc = (size_t)ncell_of(*p), esz = p->dtype == OGG_REMAP_FLOAT32 ? 4 : 8;
    double *ds, *dt, *dv;
    int* dc;
    char* df;
    unsigned char *dw = nullptr, *dfl;
    ogg_locate_counts* ct;
    if (int e = bufs.put(&dc, cell, n)) return e;
    if (int e = bufs.put(&ds, s, n)) return e;
    if (int e = bufs.put(&dt, t, n)) return e;
    if (int e = bufs.put(&df, static_cast<const char*>(f), nc * (size_t)p->nrec * esz)) return e;
    if (wet)
        if (int e = bufs.put(&dw, wet, nc)) return e;
    if (int e = bufs.alloc(&dv, n * (size_t)p->nrec)) return e;
    if (int e = bufs.alloc(&dfl, n * (size_t)p->nrec)) return e;
    if (int e = bufs.put(&ct, counts, 1)) return e;
    if (int e = ogg_locate_sample_dev(p, dc, ds, dt, df, dw, dv, dfl, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(values, dv, n * (size_t)p->nrec)) return e;
    if (int e = bufs.get(flags, dfl, n * (size_t)p->nrec)) return e;
    return OGG_OK;
}
