// Runoff spreading (include/ogg_hip.h, "Runoff spreading"): the mapped runoff of every mouth cell spread over the candidate cells
// within a chordal radius, by integer weights, and summed per receiving cell in ascending mouth order.
//
// sets        one thread per cell: its unit vector, A_c, the candidate flag and the mouth flag; two ordered compactions (ogg_blocks.h)
//             give the mouth list in ascending c and the candidate list, which is sorted into G^3 cubes (ogg_sphere_bins.h).  A mouth
//             that is no candidate leaves the smallest such cell in the workspace head, read back before anything else runs.
// count       one workgroup per mouth.  The cubes that the ball of the radius can touch form a box of cube indices; the box's cubes
//             are dealt to the four wavefronts, a cube farther than the radius is skipped (chordal distance is 3-D Euclidean distance,
//             so the distance from a point to a cube is an exact lower bound with no pole or seam case), the lanes stride over a
//             cube's candidates.  The receivers are counted and their q summed in integers: shuffles, LDS, and the workgroup's one
//             thread writes mouth_n and mouth_W; pairs, tests and the largest set reach the counts by one atomic per workgroup.
// pairs       the same walk writes the key (t << 32 | mouth index) of every pair at the mouth's offset plus an LDS cursor; the order
//             inside a mouth is arbitrary and the sort (ogg_keysort.h) removes it: the keys are unique, and within a cell they ascend
//             with the mouth index, which ascends with the mouth's cell.  A boundary pass gives every cell its [start, end).
// apply       one thread per cell over its segment: q from the same function of the same u and A as the count step, s = q / W_m,
//             the records four at a time in registers.  Every other cell gets +0.0.
//
// Every result is a fixed function of u, A, wet, cls, load and v: the cube count, the order in which the atomics land and the launch
// geometry change no bit.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "ogg_blocks.h"
#include "ogg_common.h"
#include "ogg_keysort.h"
#include "ogg_sphere_bins.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int NT = 256;                 // threads per workgroup (four wavefronts)
constexpr int NW = NT / 64;
constexpr int REC = 4;                  // records a thread of the apply step sums at a time
constexpr long HEAD = 256;
constexpr double PAD = 1e-9;            // cubes widened by this much: covers the rounding of a point's cube index
constexpr unsigned long long NONE = ULLONG_MAX;

static_assert(sizeof(ogg_spread_params) == 40, "ogg_spread_params layout");
static_assert(sizeof(ogg_spread_counts) == 64, "ogg_spread_counts layout");
static_assert(NT == BLOCKS_NT, "block_add and block_scan work over a workgroup of BLOCKS_NT threads");
static_assert(NT == KEYSORT_NT, "the block sort makes the runs the merge passes take");

struct Head {
    long long total;                    // the last scan's total
    unsigned long long bad;             // the smallest mouth cell that is no candidate, NONE without one
};
static_assert(sizeof(Head) <= HEAD, "workspace head");

// ---- the weight ----------------------------------------------------------------------------------------------------
// q(m, t) of the definition: correctly rounded + - * / only, so numpy gives the same bits
__device__ inline long long weight_q(double At, double Am, double d2, double r2, int shape) {
    const double ratio = At / Am;
    const double a = ratio < 256.0 ? ratio : 256.0;
    double g = 1.0;
    if (shape == OGG_SPREAD_BIWEIGHT) {
        const double h = 1.0 - d2 / r2;
        g = h * h;
    }
    return (long long)floor((a * g) * 16777216.0);
}

// ---- sets ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void sets_kernel(long ny, long nx, const double* __restrict__ x, const double* __restrict__ y, long ld,
                                                  const double* __restrict__ area, long lda, const unsigned char* __restrict__ wet,
                                                  const int* __restrict__ load, double* __restrict__ u, double* __restrict__ A,
                                                  unsigned char* __restrict__ cand, unsigned char* __restrict__ mflag, Head* head,
                                                  ogg_spread_counts* counts) {
    const long n = ny * nx;
    long long v[2] = {0, 0};
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const long j = c / nx, i = c % nx;
        const long k = centre_ji(j, i, ld);
        const double lon = x[k], lat = y[k];
        double w[3];
        unit(lon, lat, w);
        u[3 * c] = w[0];
        u[3 * c + 1] = w[1];
        u[3 * c + 2] = w[2];
        const double* a0 = area + 2 * j * lda + 2 * i;
        const double* a1 = a0 + lda;
        const double Ac = (a0[0] + a1[1]) + (a0[1] + a1[0]);
        A[c] = Ac;
        const bool ok = wet[c] != 0 && isfinite(lon) && isfinite(lat) && Ac > 0.0 && isfinite(Ac);
        const bool m = load[c] > 0;
        cand[c] = ok ? 1 : 0;
        mflag[c] = m ? 1 : 0;
        v[0] += ok;
        v[1] += m;
        if (m && !ok) atomicMin(&head->bad, (unsigned long long)c);
    }
    long long* const dst[2] = {&counts->candidates, &counts->mouths};
    block_add<2>(v, dst);
}

__global__ __launch_bounds__(NT) void mouth_list_kernel(long n, const unsigned char* __restrict__ flag, const int* __restrict__ pos,
                                                        int* __restrict__ mouth_cell) {
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT)
        if (flag[c]) mouth_cell[pos[c]] = (int)c;
}

__global__ __launch_bounds__(NT) void cand_list_kernel(long n, const unsigned char* __restrict__ flag, const int* __restrict__ pos,
                                                       const double* __restrict__ u, int* __restrict__ cell, double* __restrict__ cu) {
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        if (!flag[c]) continue;
        const long q = pos[c];
        cell[q] = (int)c;
        cu[3 * q] = u[3 * c];
        cu[3 * q + 1] = u[3 * c + 1];
        cu[3 * q + 2] = u[3 * c + 2];
    }
}

// ---- the walk ------------------------------------------------------------------------------------------------------
struct Index {
    int G;
    double h;
    const int* start;   // G^3 + 1
    const double* bu;
    const int* bc;
};

struct Shape {
    double r2;
    int shape;
};

// every candidate t with d2(p, u_t) <= r2 handed to f(t, d2), by the whole workgroup: the cubes of the box that the ball can touch
// dealt to the wavefronts, a cube's candidates to the lanes.  Returns this thread's distance tests.
template <typename F>
__device__ inline long long walk(const Index& ix, double r2, double px, double py, double pz, F f) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double rr = sqrt(r2) * (1.0 + 1e-9) + 2.0 * PAD;
    const int a0 = cube_of(px - rr, ix.G), b0 = cube_of(py - rr, ix.G), c0 = cube_of(pz - rr, ix.G);
    const long na = cube_of(px + rr, ix.G) - a0 + 1, nb = cube_of(py + rr, ix.G) - b0 + 1, nc = cube_of(pz + rr, ix.G) - c0 + 1;
    const long total = na * nb * nc;
    long long tests = 0;
    for (long q = wave; q < total; q += NW) {
        const int a = a0 + (int)(q % na), b = b0 + (int)((q / na) % nb), c = c0 + (int)(q / (na * nb));
        const double lx = -1.0 + a * ix.h - PAD, hx = -1.0 + (a + 1) * ix.h + PAD;
        const double ly = -1.0 + b * ix.h - PAD, hy = -1.0 + (b + 1) * ix.h + PAD;
        const double lz = -1.0 + c * ix.h - PAD, hz = -1.0 + (c + 1) * ix.h + PAD;
        const double gx = lx > px ? lx - px : (px > hx ? px - hx : 0.0), gy = ly > py ? ly - py : (py > hy ? py - hy : 0.0),
                     gz = lz > pz ? lz - pz : (pz > hz ? pz - hz : 0.0);
        if ((gx * gx + gy * gy) + gz * gz > r2 * MARGIN) continue;
        const int cube = a + ix.G * (b + ix.G * c);
        const int s0 = ix.start[cube], s1 = ix.start[cube + 1];
        for (int t = s0 + lane; t < s1; t += 64) {
            const double d2 = dist2(px, py, pz, ix.bu[3 * t], ix.bu[3 * t + 1], ix.bu[3 * t + 2]);
            ++tests;
            if (d2 <= r2) f(ix.bc[t], d2);
        }
    }
    return tests;
}

// ---- count ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void count_kernel(Index ix, Shape sh, const double* __restrict__ u, const double* __restrict__ A,
                                                   const int* __restrict__ cls, const int* __restrict__ mouth_cell, long nm,
                                                   int* __restrict__ mouth_n, long long* __restrict__ mouth_W, ogg_spread_counts* counts) {
    __shared__ long long red[NW][3];
    long long pairs = 0, tests_all = 0, most = 0;   // thread 0's
    for (long m = blockIdx.x; m < nm; m += gridDim.x) {
        const long cm = mouth_cell[m];
        const double px = u[3 * cm], py = u[3 * cm + 1], pz = u[3 * cm + 2], Am = A[cm];
        const int km = cls ? cls[cm] : 0;
        long long n = 0, W = 0;
        long long tests = walk(ix, sh.r2, px, py, pz, [&](int t, double d2) {
            if (cls && cls[t] != km) return;
            ++n;
            W += weight_q(A[t], Am, d2, sh.r2, sh.shape);
        });
        for (int off = 32; off > 0; off >>= 1) {
            n += __shfl_xor(n, off, 64);
            W += __shfl_xor(W, off, 64);
            tests += __shfl_xor(tests, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6][0] = n;
            red[threadIdx.x >> 6][1] = W;
            red[threadIdx.x >> 6][2] = tests;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long tn = 0, tW = 0, tt = 0;
            for (int w = 0; w < NW; ++w) {
                tn += red[w][0];
                tW += red[w][1];
                tt += red[w][2];
            }
            mouth_n[m] = (int)tn;
            mouth_W[m] = tW;
            pairs += tn;
            tests_all += tt;
            most = tn > most ? tn : most;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (pairs) atomicAdd(ull(&counts->pairs), (unsigned long long)pairs);
        if (tests_all) atomicAdd(ull(&counts->tests), (unsigned long long)tests_all);
        if (most) atomicMax(ull(&counts->max_receivers), (unsigned long long)most);
    }
}

// ---- pairs ---------------------------------------------------------------------------------------------------------
// off: the exclusive prefix of mouth_n, nm + 1 entries.  A slot beyond the mouth's count or beyond n_pairs is never written.
__global__ __launch_bounds__(NT) void pairs_kernel(Index ix, Shape sh, const double* __restrict__ u, const int* __restrict__ cls,
                                                   const int* __restrict__ mouth_cell, long nm, const int* __restrict__ off, long n_pairs,
                                                   unsigned long long* __restrict__ key) {
    __shared__ int cursor;
    for (long m = blockIdx.x; m < nm; m += gridDim.x) {
        if (threadIdx.x == 0) cursor = 0;
        __syncthreads();
        const long cm = mouth_cell[m];
        const int km = cls ? cls[cm] : 0;
        const long o = off[m], cnt = (long)off[m + 1] - o;
        (void)walk(ix, sh.r2, u[3 * cm], u[3 * cm + 1], u[3 * cm + 2], [&](int t, double) {
            if (cls && cls[t] != km) return;
            const long slot = atomicAdd(&cursor, 1);
            if (slot < cnt && o + slot < n_pairs) key[o + slot] = ((unsigned long long)(unsigned)t << 32) | (unsigned long long)m;
        });
        __syncthreads();
    }
}

// runs of NT keys sorted in LDS by rank (the keys are unique)
__global__ __launch_bounds__(NT) void sort_block_kernel(const unsigned long long* __restrict__ in, long n, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long lk[NT];
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    const unsigned long long key = i < n ? in[i] : ULLONG_MAX;
    lk[threadIdx.x] = key;
    __syncthreads();
    int rank = 0;
    for (int k = 0; k < NT; ++k) rank += lk[k] < key || (lk[k] == key && k < (int)threadIdx.x);
    if (i < n && (long)blockIdx.x * NT + rank < n) out[(long)blockIdx.x * NT + rank] = key;
}

__global__ __launch_bounds__(NT) void seg_kernel(const unsigned long long* __restrict__ key, long n, long ncell, int2* __restrict__ seg) {
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        const unsigned c = (unsigned)(key[k] >> 32);
        if ((long)c >= ncell) continue;   // a slot that no pair took: never written
        if (k == 0 || (unsigned)(key[k - 1] >> 32) != c) seg[c].x = (int)k;
        if (k + 1 == n || (unsigned)(key[k + 1] >> 32) != c) seg[c].y = (int)(k + 1);
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void apply_kernel(long ncell, long nrec, Shape sh, const double* __restrict__ v, const double* __restrict__ u,
                                                   const double* __restrict__ A, const int* __restrict__ mouth_cell,
                                                   const long long* __restrict__ mouth_W, long nm, const int2* __restrict__ seg,
                                                   const unsigned long long* __restrict__ key, double* __restrict__ out,
                                                   int* __restrict__ n_out, ogg_spread_counts* counts) {
    const long c = (long)blockIdx.x * NT + threadIdx.x;
    const bool inb = c < ncell;
    int s0 = 0, n = 0;
    double tx = 0.0, ty = 0.0, tz = 0.0, At = 1.0;
    if (inb) {
        const int2 sg = seg[c];
        s0 = sg.x;
        n = sg.y - sg.x;
        if (n < 0) n = 0;
        n_out[c] = n;
        if (n > 0) {
            tx = u[3 * c];
            ty = u[3 * c + 1];
            tz = u[3 * c + 2];
            At = A[c];
        }
    }
    for (long r0 = 0; r0 < nrec; r0 += REC) {
        double T[REC];
#pragma unroll
        for (int j = 0; j < REC; ++j) T[j] = 0.0;
        for (int k = s0; k < s0 + n; ++k) {
            const long idx = (long)(key[k] & 0xFFFFFFFFull);
            if (idx >= nm) continue;
            const long m = mouth_cell[idx];
            const double Am = A[m];
            const double d2 = dist2(u[3 * m], u[3 * m + 1], u[3 * m + 2], tx, ty, tz);
            const double s = (double)weight_q(At, Am, d2, sh.r2, sh.shape) / (double)mouth_W[idx];
#pragma unroll
            for (int j = 0; j < REC; ++j) {
                if (r0 + j < nrec) {
                    const double F = v[(r0 + j) * ncell + m] * Am;
                    T[j] += F * s;
                }
            }
        }
        if (inb) {
#pragma unroll
            for (int j = 0; j < REC; ++j)
                if (r0 + j < nrec) out[(r0 + j) * ncell + c] = n > 0 ? T[j] / At : 0.0;
        }
    }
    long long mx = n;
    for (int off = 32; off > 0; off >>= 1) {
        const long long t = __shfl_xor(mx, off, 64);
        mx = t > mx ? t : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(ull(&counts->max_mouths), (unsigned long long)mx);
    long long w[1] = {n > 0 ? 1 : 0};
    long long* const dst[1] = {&counts->loaded};
    block_add<1>(w, dst);
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_spread_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "spread: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "spread: %ld x %ld cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE(p->nrec >= 1 && p->nrec <= (long)INT_MAX && p->nrec * p->ny * p->nx < (1L << 32), OGG_EARG,
                "spread: %ld records of %ld x %ld cells: nrec >= 1 and nrec * ny * nx < 2^32", p->nrec, p->ny, p->nx);
    OGG_REQUIRE(p->shape == OGG_SPREAD_UNIFORM || p->shape == OGG_SPREAD_BIWEIGHT, OGG_EARG, "spread: shape %d (0: uniform, 1: biweight)",
                p->shape);
    OGG_REQUIRE(p->use_classes == 0 || p->use_classes == 1, OGG_EARG, "spread: use_classes %d (0 or 1)", p->use_classes);
    OGG_REQUIRE(p->r2 > 0.0 && p->r2 <= 4.0, OGG_EARG, "spread: squared chordal radius %g: 0 < r2 <= 4", p->r2);
    return OGG_OK;
}

long ncell_of(const ogg_spread_params& p) { return p.ny * p.nx; }
long nbins_max() { return (long)OGG_SPREAD_MAX_CUBES * OGG_SPREAD_MAX_CUBES * OGG_SPREAD_MAX_CUBES + 1; }

// the pairs a call may hold: OGG_SPREAD_MAX_PAIRS, or the smaller OGG_SPREAD_MAX_PAIRS_TEST (for tests: it can only lower the limit)
int pairs_limit(long* out) {
    int t = 0;
    if (int e = knob("OGG_SPREAD_MAX_PAIRS_TEST", (int)OGG_SPREAD_MAX_PAIRS, 1, (int)OGG_SPREAD_MAX_PAIRS, &t)) return e;
    *out = t;
    return OGG_OK;
}

int check_pairs(long n_pairs) {
    long limit = 0;
    if (int e = pairs_limit(&limit)) return e;
    OGG_REQUIRE(n_pairs >= 0, OGG_EARG, "spread: %ld pairs", n_pairs);
    OGG_REQUIRE(n_pairs < limit, OGG_EARG,
                "spread: P = %ld mouth-receiver pairs, the limit is %ld: a smaller radius, or fewer loaded cells", n_pairs, limit);
    return OGG_OK;
}

// cubes per axis of the index; brute force is one cube that holds every candidate
struct Plan {
    int G, brute;
};

int plan_of(const ogg_spread_params& p, Plan* out) {
    int brute = 0, cubes = 0;
    if (int e = knob("OGG_SPREAD_BRUTE", 0, 0, 1, &brute)) return e;
    if (int e = knob("OGG_SPREAD_CUBES", 0, 0, OGG_SPREAD_MAX_CUBES, &cubes)) return e;
    long G = cubes > 0 ? cubes : std::min<long>(std::max<long>((long)floor(2.0 / sqrt(p.r2)), 1), OGG_SPREAD_MAX_CUBES);
    *out = Plan{brute ? 1 : (int)G, brute};
    return OGG_OK;
}

// workspace: head | mouth flag bytes | positions | block sums | candidate cells | candidate u | the cube index | mouth offsets |
// segments | keys (two buffers).  Everything before the keys does not depend on n_pairs: the workspace of the steps before the
// pairs are known is a prefix of the whole.
struct Layout {
    long mflag, pos, bsum, ccell, cu, moff, seg, key0, key1, total;
    CubeIndexLayout index;
};

Layout layout(const ogg_spread_params& p, long n_pairs) {
    Layout l;
    const long nc = ncell_of(p), nb = nbins_max();
    ogg::Sections s{HEAD};
    l.mflag = s.take(nc);
    l.pos = s.take(nc * 4);
    l.bsum = s.take((std::max(nc + 1, nb) / SCAN_CH + 2) * 8);
    l.ccell = s.take(nc * 4);
    l.cu = s.take(nc * 24);
    l.index = cube_index_sections(s, nc, nb);
    l.moff = s.take((nc + 1) * 4);
    l.seg = s.take(nc * 8);
    l.key0 = s.take(n_pairs * 8);
    l.key1 = s.take(n_pairs * 8);
    l.total = s.off;
    return l;
}

Index index_at(void* ws, const Layout& l, int G) {
    const CubeIndex ci = cube_index_at(ws, l.index);
    return Index{G, 2.0 / (double)G, ci.start, ci.bu, ci.bc};
}

unsigned mouth_grid(long nm) { return (unsigned)std::min<long>(std::max<long>(nm, 1), 1L << 20); }

}  // namespace

extern "C" long ogg_spread_workspace_bytes(const ogg_spread_params* p, long n_pairs) {
    if (!p || check_params(p) != OGG_OK || check_pairs(n_pairs) != OGG_OK) return -1;
    return layout(*p, n_pairs).total;
}

extern "C" int ogg_spread_check(const ogg_spread_params* p) { return check_params(p); }

extern "C" int ogg_spread_sets_dev(const ogg_spread_params* p, const double* x, const double* y, long ld, const double* area, long lda,
                                   const unsigned char* wet, const int* load, void* workspace, long workspace_bytes, double* u, double* A,
                                   unsigned char* cand, int* mouth_cell, ogg_spread_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_spread_sets", workspace, workspace_bytes, layout(*p, 0).total)) return e;
    OGG_REQUIRE(x && y && area && wet && load && u && A && cand && mouth_cell && counts, OGG_EARG,
                "ogg_spread_sets: null x / y / area / wet / load / u / A / cand / mouth_cell / counts");
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_spread_sets: row stride %ld < 2 nx + 1", ld);
    OGG_REQUIRE(lda >= 2 * p->nx, OGG_EARG, "ogg_spread_sets: area row stride %ld < 2 nx", lda);
    Plan plan;
    if (int e = plan_of(*p, &plan)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p, 0);
    const long nc = ncell_of(*p);
    Head* head = at<Head>(workspace, 0);
    unsigned char* mflag = at<unsigned char>(workspace, l.mflag);
    int* pos = at<int>(workspace, l.pos);
    long long* bsum = at<long long>(workspace, l.bsum);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_spread_counts), st));
    OGG_HIP_CHECK(hipMemsetAsync(head, 0xFF, sizeof(Head), st));
    sets_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(p->ny, p->nx, x, y, ld, area, lda, wet, load, u, A, cand, mflag, head, counts);
    OGG_LAUNCH_CHECK();
    if (int e = exclusive_scan<false>(mflag, nc, bsum, &head->total, pos, st)) return e;
    mouth_list_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(nc, mflag, pos, mouth_cell);
    OGG_LAUNCH_CHECK();
    if (int e = exclusive_scan<false>(cand, nc, bsum, &head->total, pos, st)) return e;
    int* ccell = at<int>(workspace, l.ccell);
    double* cu = at<double>(workspace, l.cu);
    cand_list_kernel<<<grid_for<NT>(nc, 4096), NT, 0, st>>>(nc, cand, pos, u, ccell, cu);
    OGG_LAUNCH_CHECK();
    const long long cubes = plan.brute ? 0 : plan.G;
    unsigned long long bad = NONE;
    long long ncand = 0;
    OGG_HIP_CHECK(hipMemcpyAsync(&counts->cubes, &cubes, sizeof(cubes), hipMemcpyHostToDevice, st));
    OGG_HIP_CHECK(hipMemcpyAsync(&bad, &head->bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    OGG_HIP_CHECK(hipMemcpyAsync(&ncand, &counts->candidates, sizeof(ncand), hipMemcpyDeviceToHost, st));
    OGG_HIP_CHECK(hipStreamSynchronize(st));   // the three words live on this frame
    OGG_REQUIRE(bad == NONE, OGG_EARG,
                "spread: mouth cell %llu (j = %llu, i = %llu) is no candidate: it is land, or its centre or its area is not finite and positive",
                bad, bad / (unsigned long long)p->nx, bad % (unsigned long long)p->nx);
    OGG_REQUIRE(ncand >= 0 && ncand <= nc, OGG_EARG, "ogg_spread_sets: %lld candidates of %ld cells", ncand, nc);
    return build_cube_index(cu, ccell, (long)ncand, plan.G, cube_index_at(workspace, l.index), bsum, &head->total, st);
}

extern "C" int ogg_spread_count_dev(const ogg_spread_params* p, const double* u, const double* A, const int* cls, const int* mouth_cell,
                                    long n_mouths, void* workspace, long workspace_bytes, int* mouth_n, long long* mouth_W,
                                    ogg_spread_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_spread_count", workspace, workspace_bytes, layout(*p, 0).total)) return e;
    OGG_REQUIRE(n_mouths >= 0 && n_mouths <= ncell_of(*p), OGG_EARG, "ogg_spread_count: %ld mouths of %ld cells", n_mouths, ncell_of(*p));
    OGG_REQUIRE(u && A && counts && ((mouth_cell && mouth_n && mouth_W) || n_mouths == 0) && (cls || !p->use_classes), OGG_EARG,
                "ogg_spread_count: null u / A / cls / mouth_cell / mouth_n / mouth_W / counts");
    Plan plan;
    if (int e = plan_of(*p, &plan)) return e;
    if (n_mouths == 0) return OGG_OK;
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p, 0);
    count_kernel<<<mouth_grid(n_mouths), NT, 0, st>>>(index_at(workspace, l, plan.G), Shape{p->r2, p->shape}, u, A,
                                                      p->use_classes ? cls : nullptr, mouth_cell, n_mouths, mouth_n, mouth_W, counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_spread_pairs_dev(const ogg_spread_params* p, const double* u, const int* cls, const int* mouth_cell, const int* mouth_n,
                                    long n_mouths, long n_pairs, void* workspace, long workspace_bytes, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = check_pairs(n_pairs)) return e;
    if (int e = ogg::check_workspace("ogg_spread_pairs", workspace, workspace_bytes, layout(*p, n_pairs).total)) return e;
    OGG_REQUIRE(n_mouths >= 0 && n_mouths <= ncell_of(*p), OGG_EARG, "ogg_spread_pairs: %ld mouths of %ld cells", n_mouths, ncell_of(*p));
    OGG_REQUIRE(n_pairs >= n_mouths, OGG_EARG, "ogg_spread_pairs: %ld pairs of %ld mouths (every mouth receives from itself)", n_pairs,
                n_mouths);
    OGG_REQUIRE(u && ((mouth_cell && mouth_n) || n_mouths == 0) && (cls || !p->use_classes), OGG_EARG,
                "ogg_spread_pairs: null u / cls / mouth_cell / mouth_n");
    Plan plan;
    if (int e = plan_of(*p, &plan)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p, n_pairs);
    int2* seg = at<int2>(workspace, l.seg);
    OGG_HIP_CHECK(hipMemsetAsync(seg, 0, (size_t)ncell_of(*p) * 8, st));
    if (n_mouths == 0 || n_pairs == 0) return OGG_OK;
    int* moff = at<int>(workspace, l.moff);
    if (int e = exclusive_scan<true>(mouth_n, n_mouths, at<long long>(workspace, l.bsum), nullptr, moff, st)) return e;
    unsigned long long* buf[2] = {at<unsigned long long>(workspace, l.key0), at<unsigned long long>(workspace, l.key1)};
    OGG_HIP_CHECK(hipMemsetAsync(buf[1], 0xFF, (size_t)n_pairs * 8, st));   // a slot that no pair takes sorts behind every cell
    pairs_kernel<<<mouth_grid(n_mouths), NT, 0, st>>>(index_at(workspace, l, plan.G), Shape{p->r2, p->shape}, u,
                                                      p->use_classes ? cls : nullptr, mouth_cell, n_mouths, moff, n_pairs, buf[1]);
    OGG_LAUNCH_CHECK();
    sort_block_kernel<<<(unsigned)((n_pairs + NT - 1) / NT), NT, 0, st>>>(buf[1], n_pairs, buf[0]);
    OGG_LAUNCH_CHECK();
    int k = 0;
    for (long w = NT; w < n_pairs; w *= 2, ++k) {
        keysort_merge_kernel<<<grid_for<NT>(n_pairs, 1L << 20), NT, 0, st>>>(buf[k & 1], n_pairs, w, buf[(k + 1) & 1]);
        OGG_LAUNCH_CHECK();
    }
    seg_kernel<<<grid_for<NT>(n_pairs, 1L << 20), NT, 0, st>>>(buf[k & 1], n_pairs, ncell_of(*p), seg);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_spread_apply_dev(const ogg_spread_params* p, const double* v, const double* u, const double* A, const int* mouth_cell,
                                    const long long* mouth_W, long n_mouths, long n_pairs, const void* workspace, long workspace_bytes,
                                    double* out, int* n_mouths_out, ogg_spread_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = check_pairs(n_pairs)) return e;
    if (int e = ogg::check_workspace("ogg_spread_apply", workspace, workspace_bytes, layout(*p, n_pairs).total)) return e;
    OGG_REQUIRE(n_mouths >= 0 && n_mouths <= ncell_of(*p), OGG_EARG, "ogg_spread_apply: %ld mouths of %ld cells", n_mouths, ncell_of(*p));
    OGG_REQUIRE(v && u && A && out && n_mouths_out && counts && ((mouth_cell && mouth_W) || n_mouths == 0), OGG_EARG,
                "ogg_spread_apply: null v / u / A / mouth_cell / mouth_W / out / n_mouths / counts");
    hipStream_t st = ogg::as_stream(stream);
    const Layout l = layout(*p, n_pairs);
    const long nc = ncell_of(*p);
    const unsigned long long* key = at<unsigned long long>(workspace, (keysort_passes(n_pairs) & 1) ? l.key1 : l.key0);
    apply_kernel<<<(unsigned)((nc + NT - 1) / NT), NT, 0, st>>>(nc, p->nrec, Shape{p->r2, p->shape}, v, u, A, mouth_cell, mouth_W, n_mouths,
                                                               at<int2>(workspace, l.seg), key, out, n_mouths_out, counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: everything copied to device memory, the four steps, the results copied back (synchronous)
extern "C" int ogg_runoff_spread(const ogg_spread_params* p, const double* x, const double* y, const double* area, const unsigned char* wet,
                                 const int* cls, const int* load, const double* v, double* out, int* n_mouths, int* mouth_cell, int* mouth_n,
                                 long long* mouth_W, ogg_spread_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(x && y && area && wet && load && v && out && n_mouths && mouth_cell && mouth_n && mouth_W && counts &&
                    (cls || !p->use_classes),
                OGG_EARG, "ogg_runoff_spread: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t nc = (size_t)ncell_of(*p), npt = (size_t)(2 * p->ny + 1) * (2 * p->nx + 1);
    const long wsb0 = layout(*p, 0).total;
    double *dx, *dy, *da, *dv, *du, *dA, *dout;
    unsigned char *dw, *dcand;
    char *ws0, *ws;
    int *dcls = nullptr, *dload, *dmc, *dmn, *dnm;
    long long* dmW;
    ogg_spread_counts* ct;
    if (int e = bufs.put(&dx, x, npt)) return e;
    if (int e = bufs.put(&dy, y, npt)) return e;
    if (int e = bufs.put(&da, area, nc * 4)) return e;
    if (int e = bufs.put(&dw, wet, nc)) return e;
    if (int e = bufs.put(&dload, load, nc)) return e;
    if (p->use_classes)
        if (int e = bufs.put(&dcls, cls, nc)) return e;
    if (int e = bufs.put(&dv, v, (size_t)p->nrec * nc)) return e;
    if (int e = bufs.alloc(&du, nc * 3)) return e;
    if (int e = bufs.alloc(&dA, nc)) return e;
    if (int e = bufs.alloc(&dcand, nc)) return e;
    if (int e = bufs.alloc(&dmc, nc)) return e;
    if (int e = bufs.alloc(&dmn, nc)) return e;
    if (int e = bufs.alloc(&dmW, nc)) return e;
    if (int e = bufs.alloc(&dout, (size_t)p->nrec * nc)) return e;
    if (int e = bufs.alloc(&dnm, nc)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = bufs.alloc(&ws0, (size_t)wsb0)) return e;
    if (int e = ogg_spread_sets_dev(p, dx, dy, 2 * p->nx + 1, da, 2 * p->nx, dw, dload, ws0, wsb0, du, dA, dcand, dmc, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    const long nm = (long)counts->mouths;
    if (int e = ogg_spread_count_dev(p, du, dA, dcls, dmc, nm, ws0, wsb0, dmn, dmW, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    const long np = (long)counts->pairs;
    if (int e = check_pairs(np)) return e;   // before the keys are allocated
    const long wsb = layout(*p, np).total;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    OGG_HIP_CHECK(hipMemcpy(ws, ws0, (size_t)wsb0, hipMemcpyDeviceToDevice));   // the earlier steps' workspace is a prefix
    if (int e = ogg_spread_pairs_dev(p, du, dcls, dmc, dmn, nm, np, ws, wsb, nullptr)) return e;
    if (int e = ogg_spread_apply_dev(p, dv, du, dA, dmc, dmW, nm, np, ws, wsb, dout, dnm, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(out, dout, (size_t)p->nrec * nc)) return e;
    if (int e = bufs.get(n_mouths, dnm, nc)) return e;
    if (nm > 0) {
        if (int e = bufs.get(mouth_cell, dmc, (size_t)nm)) return e;
        if (int e = bufs.get(mouth_n, dmn, (size_t)nm)) return e;
        if (int e = bufs.get(mouth_W, dmW, (size_t)nm)) return e;
    }
    return OGG_OK;
}
