// Conservative regrid of model-cell fields onto a lat-lon grid (include/ogg_hip.h, "Conservative regrid to a lat-lon grid"): the
// exchange list transposed from model-cell order to target-cell order, then a segmented, masked, weighted sum per target cell.
//
// transpose          count_kernel counts the entries of every target cell (atomicAdd) and a three-kernel exclusive scan turns the
//                    counts into segment starts.  The entries themselves are ordered by their keys (k << 32) | position with the
//                    shared key sort (ogg_keysort.h): key_block_kernel sorts runs of 256 keys in LDS, keysort_merge_kernel merges runs
//                    in pairs, O(n log n) whatever the lengths of the segments (a zonal or one-cell target puts the whole list in a
//                    few).  The keys are unique and sort by cell, then position, so every segment comes out in ascending list
//                    position; entries outside the cells or the target take k = NA * NB and sort last.  pairs_kernel writes the
//                    sorted (model cell, area) pairs.
// regrid_kernel<T,R> one lane per target cell of at most OGG_REGRID_LONG entries, 64 consecutive cells per wavefront; a lane walks its
//                    own segment left to right for R records at once (OGG_REGRID_RECORDS): each entry's (cell, area) is read once
//                    for the R records, whose R gathers are independent loads in flight together.
// regrid_long_kernel one wavefront per longer target cell and group of R records (blockIdx.y), the cells taken from a list the static
//                    step builds: 64 entries at a time, every lane gathers one entry's R values, and the sums take them in list order
//                    through shuffles (the remap's long path), so no lane walks a long cell alone.
// static_kernel      one lane per target cell: n_entries, the long-cell list, and for the other cells W0 (every entry, in order) and
//                    ocean_frac = W0 / A_atm; static_long_kernel the same sum for the long cells by whole wavefronts.
//
// Every value is a fixed function of the list, the field and A_atm: the in-order sums are the definition's on either path, so nothing
// depends on the launch geometry, the knobs or the order in which the atomics land (the long-cell list's order decides only which
// wavefront takes a cell).
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ogg_blocks.h"
#include "ogg_common.h"
#include "ogg_keysort.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int NT = 256;                 // threads per workgroup of the list passes (four wavefronts)
constexpr int LONG_DEFAULT = 512;       // cells with more entries are walked by whole wavefronts (OGG_REGRID_LONG)
constexpr int LONG_WAVES = 4096;        // wavefronts of the long-cell kernels (per record group)
constexpr int RECORDS_DEFAULT = 4;      // records a lane sums at once (OGG_REGRID_RECORDS)
constexpr long HEAD = 256;              // workspace head: the length of the long-cell list (int64)

static_assert(NT == BLOCKS_NT, "block_add and block_scan work over a workgroup of BLOCKS_NT threads");
static_assert(sizeof(ogg_regrid_params) == 72, "ogg_regrid_params layout");
static_assert(sizeof(ogg_regrid_counts) == 48, "ogg_regrid_counts layout");

// ---- transpose -----------------------------------------------------------------------------------------------------
struct List {
    long n, ny, nx, NA, NB;
};

// the target cell of entry e, -1 when the entry lies outside the cells or the target
__device__ inline long target_of(const List& l, const int* atm, const int* ocn, long e) {
    const long I = atm[2 * e], J = atm[2 * e + 1], i = ocn[2 * e], m = ocn[2 * e + 1];
    if (I < 0 || I >= l.NA || J < 0 || J >= l.NB || i < 0 || i >= l.nx || m < 0 || m >= l.ny) return -1;
    return J * l.NA + I;
}

__global__ __launch_bounds__(NT) void count_kernel(List l, const int* __restrict__ atm, const int* __restrict__ ocn, int* __restrict__ cnt,
                                                   ogg_regrid_counts* counts) {
    long long v[2] = {0, 0};
    for (long e = (long)blockIdx.x * NT + threadIdx.x; e < l.n; e += (long)gridDim.x * NT) {
        const long k = target_of(l, atm, ocn, e);
        if (k < 0) {
            ++v[1];
            continue;
        }
        atomicAdd(&cnt[k], 1);
        ++v[0];
    }
    long long* const dst[2] = {&counts->entries, &counts->bad_entries};
    block_add<2>(v, dst);
}

// keys (k << 32) | position of KEYSORT_NT consecutive entries sorted in LDS by rank (the keys are unique)
__global__ __launch_bounds__(KEYSORT_NT) void key_block_kernel(List l, long nk, const int* __restrict__ atm, const int* __restrict__ ocn,
                                                               unsigned long long* __restrict__ out) {
    __shared__ unsigned long long lk[KEYSORT_NT];
    const long e = (long)blockIdx.x * KEYSORT_NT + threadIdx.x;
    unsigned long long key = ULLONG_MAX;
    if (e < l.n) {
        const long k = target_of(l, atm, ocn, e);
        key = ((unsigned long long)(k < 0 ? nk : k) << 32) | (unsigned long long)e;
    }
    lk[threadIdx.x] = key;
    __syncthreads();
    int rank = 0;
    for (int q = 0; q < KEYSORT_NT; ++q) rank += lk[q] < key;
    if (e < l.n) out[(long)blockIdx.x * KEYSORT_NT + rank] = key;
}

// the (model cell, area) pair of every sorted key of the cells and the target (they come first: the others have k = nk)
__global__ __launch_bounds__(NT) void pairs_kernel(long n, long nk, long nx, const unsigned long long* __restrict__ key,
                                                   const int* __restrict__ ocn, const double* __restrict__ area, int* __restrict__ pc,
                                                   double* __restrict__ pa) {
    for (long t = (long)blockIdx.x * NT + threadIdx.x; t < n; t += (long)gridDim.x * NT) {
        const unsigned long long kt = key[t];
        if ((long)(kt >> 32) >= nk) continue;
        const long e = (long)(kt & 0xFFFFFFFFull);
        pc[t] = ocn[2 * e + 1] * (int)nx + ocn[2 * e];
        pa[t] = area[e];
    }
}

// ---- regrid --------------------------------------------------------------------------------------------------------
struct Geo {
    long nk, ncell, nrec;
    int n_fill, cell_norm, long_n;
    double fill0, fill1;
};

template <typename T, int R>
__global__ __launch_bounds__(NT) void regrid_kernel(Geo g, const T* __restrict__ f, const int* __restrict__ seg, const int* __restrict__ pc,
                                                    const double* __restrict__ pa, const double* __restrict__ a_atm,
                                                    double* __restrict__ out, double* __restrict__ cover, ogg_regrid_counts* counts) {
    const long k = (long)blockIdx.x * NT + threadIdx.x;
    const bool inb = k < g.nk;
    const T f0 = static_cast<T>(g.fill0), f1 = static_cast<T>(g.fill1);
    int s = 0, e = 0;
    double A = 1.0;
    bool mine = false;   // not a long cell: regrid_long_kernel takes those
    if (inb) {
        s = seg[k];
        e = seg[k + 1];
        A = a_atm[k];
        mine = e - s <= g.long_n;
        if (!mine) e = s;
    }
    long long v_ok = 0, v_empty = 0;
    for (long r0 = 0; r0 < g.nrec; r0 += R) {
        const int nr = g.nrec - r0 < R ? (int)(g.nrec - r0) : R;
        double W[R], S[R];
#pragma unroll
        for (int q = 0; q < R; ++q) W[q] = 0.0, S[q] = 0.0;
        const T* fr = f + r0 * g.ncell;
        for (int t = s; t < e; ++t) {
            const long c = pc[t];
            const double a = pa[t];
            T v[R];
#pragma unroll
            for (int q = 0; q < R; ++q) v[q] = q < nr ? fr[q * g.ncell + c] : T(0);
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (!missing(v[q], f0, f1, g.n_fill)) {
                    W[q] += a;
                    S[q] += a * (double)v[q];
                }
            }
        }
        if (mine) {
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q >= nr) break;
                const long o = (r0 + q) * g.nk + k;
                double val;
                if (g.cell_norm) val = W[q] > 0.0 ? S[q] / A : 0.0;
                else val = W[q] > 0.0 ? S[q] / W[q] : OGG_REMAP_FILL;
                out[o] = val;
                if (cover) cover[o] = W[q] / A;
                if (W[q] > 0.0) ++v_ok;
                else ++v_empty;
            }
        }
    }
    long long v[2] = {v_ok, v_empty};
    long long* const dst[2] = {&counts->valid, &counts->empty};
    block_add<2>(v, dst);
}

// one wavefront per long cell and group of R records: the entries 64 at a time, the sums in list order through shuffles
template <typename T, int R>
__global__ __launch_bounds__(64) void regrid_long_kernel(Geo g, const T* __restrict__ f, const int* __restrict__ seg, const int* __restrict__ pc,
                                                         const double* __restrict__ pa, const double* __restrict__ a_atm,
                                                         const int* __restrict__ longs, const long long* __restrict__ n_long,
                                                         double* __restrict__ out, double* __restrict__ cover, ogg_regrid_counts* counts) {
    const int lane = threadIdx.x;
    const T f0 = static_cast<T>(g.fill0), f1 = static_cast<T>(g.fill1);
    const long nl = *n_long;
    long long v_ok = 0, v_empty = 0;
    for (long r0 = (long)blockIdx.y * R; r0 < g.nrec; r0 += (long)gridDim.y * R)
    for (long i = blockIdx.x; i < nl; i += gridDim.x) {
        const int nr = g.nrec - r0 < R ? (int)(g.nrec - r0) : R;
        const T* fr = f + r0 * g.ncell;
        const long k = longs[i];
        const int s = seg[k], n = seg[k + 1] - s;
        double W[R], S[R];
#pragma unroll
        for (int q = 0; q < R; ++q) W[q] = 0.0, S[q] = 0.0;
        for (int base = 0; base < n; base += 64) {
            double a = 0.0, p[R];
            unsigned ok = 0;
#pragma unroll
            for (int q = 0; q < R; ++q) p[q] = 0.0;
            if (base + lane < n) {
                const long c = pc[s + base + lane];
                a = pa[s + base + lane];
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    if (q < nr) {
                        const T v = fr[q * g.ncell + c];
                        if (!missing(v, f0, f1, g.n_fill)) ok |= 1u << q;
                        p[q] = a * (double)v;
                    }
                }
            }
            const int cnt = n - base < 64 ? n - base : 64;
            for (int t = 0; t < cnt; ++t) {
                const double at = __shfl(a, t, 64);
                const unsigned ot = __shfl(ok, t, 64);
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const double pt = __shfl(p[q], t, 64);
                    if ((ot >> q) & 1u) {
                        W[q] += at;
                        S[q] += pt;
                    }
                }
            }
        }
        if (lane == 0) {
            const double A = a_atm[k];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q >= nr) break;
                const long o = (r0 + q) * g.nk + k;
                double val;
                if (g.cell_norm) val = W[q] > 0.0 ? S[q] / A : 0.0;
                else val = W[q] > 0.0 ? S[q] / W[q] : OGG_REMAP_FILL;
                out[o] = val;
                if (cover) cover[o] = W[q] / A;
                if (W[q] > 0.0) ++v_ok;
                else ++v_empty;
            }
        }
    }
    if (lane == 0) {
        if (v_ok) atomicAdd(ull(&counts->valid), (unsigned long long)v_ok);
        if (v_empty) atomicAdd(ull(&counts->empty), (unsigned long long)v_empty);
    }
}

// one lane per target cell: n_entries, the counts, the long cells into the list, W0 and ocean_frac of the others
__global__ __launch_bounds__(NT) void static_kernel(long nk, int long_n, const int* __restrict__ seg, const double* __restrict__ pa,
                                                    const double* __restrict__ a_atm, double* __restrict__ frac, int* __restrict__ nent,
                                                    int* __restrict__ longs, long long* __restrict__ n_long, ogg_regrid_counts* counts) {
    const long k = (long)blockIdx.x * NT + threadIdx.x;
    long long n = 0;
    if (k < nk) {
        const int s = seg[k], e = seg[k + 1];
        n = e - s;
        if (n > long_n) {
            longs[atomicAdd(ull(n_long), 1ull)] = (int)k;
        } else if (frac) {
            double w = 0.0;
            for (int t = s; t < e; ++t) w += pa[t];
            frac[k] = w / a_atm[k];
        }
        if (nent) nent[k] = (int)n;
    }
    long long mx = n;
    for (int off = 32; off > 0; off >>= 1) {
        const long long t = __shfl_xor(mx, off, 64);
        mx = t > mx ? t : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(ull(&counts->max_entries), (unsigned long long)mx);
    long long v[1] = {n > 0 ? 1 : 0};
    long long* const dst[1] = {&counts->cells};
    block_add<1>(v, dst);
}

// W0 and ocean_frac of the long cells: one wavefront per cell, 64 areas at a time added in list order through shuffles
__global__ __launch_bounds__(64) void static_long_kernel(const int* __restrict__ seg, const double* __restrict__ pa,
                                                         const double* __restrict__ a_atm, const int* __restrict__ longs,
                                                         const long long* __restrict__ n_long, double* __restrict__ frac) {
    const int lane = threadIdx.x;
    const long nl = *n_long;
    for (long i = blockIdx.x; i < nl; i += gridDim.x) {
        const long k = longs[i];
        const int s = seg[k], n = seg[k + 1] - s;
        double w = 0.0;
        for (int base = 0; base < n; base += 64) {
            const double a = base + lane < n ? pa[s + base + lane] : 0.0;
            const int cnt = n - base < 64 ? n - base : 64;
            for (int t = 0; t < cnt; ++t) w += __shfl(a, t, 64);
        }
        if (lane == 0) frac[k] = w / a_atm[k];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_regrid_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "regrid: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "regrid: %ld x %ld model cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE(p->NA >= 1 && p->NB >= 1 && p->NA <= (long)INT_MAX && p->NB <= (long)INT_MAX && p->NA * p->NB < (1L << 31), OGG_EARG,
                "regrid: %ld x %ld target cells: NA, NB >= 1 and NA * NB < 2^31", p->NA, p->NB);
    OGG_REQUIRE(p->nrec >= 1 && p->nrec <= (long)INT_MAX && p->nrec * p->NA * p->NB < (1L << 32), OGG_EARG,
                "regrid: %ld records of %ld x %ld target cells: nrec >= 1 and nrec * NB * NA < 2^32", p->nrec, p->NB, p->NA);
    OGG_REQUIRE(p->dtype == OGG_REMAP_FLOAT32 || p->dtype == OGG_REMAP_FLOAT64, OGG_EARG, "regrid: field dtype %d (0: float32, 1: float64)",
                p->dtype);
    OGG_REQUIRE(p->n_fill >= 0 && p->n_fill <= OGG_REMAP_MAX_FILLS, OGG_EARG, "regrid: %d fill values (at most %d)", p->n_fill,
                OGG_REMAP_MAX_FILLS);
    OGG_REQUIRE(p->normalize == OGG_REGRID_AREA || p->normalize == OGG_REGRID_CELL, OGG_EARG, "regrid: normalize %d (0: area, 1: cell)",
                p->normalize);
    return OGG_OK;
}

// workspace: head | counts (nk ints) | segments (nk + 1 ints) | scan block sums | long cells (nk ints) | keys (two buffers of n) |
// cells (n ints) | areas (n doubles)
struct Layout {
    long cur, seg, bsum, longs, key0, key1, pc, pa, total;
};

Layout layout(const ogg_regrid_params& p, long n) {
    Layout l;
    const long nk = p.NA * p.NB;
    ogg::Sections s{HEAD};
    l.cur = s.take(nk * 4);
    l.seg = s.take((nk + 1) * 4);
    l.bsum = s.take(((nk + 1) / SCAN_CH + 2) * 8);
    l.longs = s.take(nk * 4);
    l.key0 = s.take(n * 8);
    l.key1 = s.take(n * 8);
    l.pc = s.take(n * 4);
    l.pa = s.take(n * 8);
    l.total = s.off;
    return l;
}

struct Bufs {
    const int *seg, *pc, *longs;
    const double *pa, *a_atm;
    const long long* n_long;
    double *out, *cover;
    ogg_regrid_counts* counts;
};

template <typename T, int R>
void launch_regrid(hipStream_t st, const Geo& g, const void* f, const Bufs& b) {
    const T* ft = static_cast<const T*>(f);
    regrid_kernel<T, R><<<(unsigned)((g.nk + NT - 1) / NT), NT, 0, st>>>(g, ft, b.seg, b.pc, b.pa, b.a_atm, b.out, b.cover, b.counts);
    const dim3 grid((unsigned)std::min<long>(g.nk, LONG_WAVES), (unsigned)std::min<long>((g.nrec + R - 1) / R, 65535));
    regrid_long_kernel<T, R><<<grid, 64, 0, st>>>(g, ft, b.seg, b.pc, b.pa, b.a_atm, b.longs, b.n_long, b.out, b.cover, b.counts);
}

template <typename T>
int launch_regrid_r(int rec, hipStream_t st, const Geo& g, const void* f, const Bufs& b) {
    switch (rec) {
        case 1: launch_regrid<T, 1>(st, g, f, b); break;
        case 2: launch_regrid<T, 2>(st, g, f, b); break;
        case 4: launch_regrid<T, 4>(st, g, f, b); break;
        case 8: launch_regrid<T, 8>(st, g, f, b); break;
        default: return ogg::set_error(OGG_EARG, "OGG_REGRID_RECORDS=%d: 1, 2, 4 or 8", rec);
    }
    return OGG_OK;
}

}  // namespace

extern "C" long ogg_regrid_workspace_bytes(const ogg_regrid_params* p, long n_entries) {
    if (!p || check_params(p) != OGG_OK || n_entries < 0 || n_entries >= (long)INT_MAX) return -1;
    return layout(*p, n_entries).total;
}

extern "C" int ogg_regrid_check(const ogg_regrid_params* p) { return check_params(p); }

extern "C" int ogg_regrid_transpose_dev(const ogg_regrid_params* p, const int* atm_ij, const int* ocn_ij, const double* area, long n_entries,
                                        void* workspace, long workspace_bytes, ogg_regrid_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(n_entries >= 0 && n_entries < (long)INT_MAX, OGG_EARG, "ogg_regrid_transpose: %ld entries (< 2^31)", n_entries);
    OGG_REQUIRE((atm_ij && ocn_ij && area) || n_entries == 0, OGG_EARG, "ogg_regrid_transpose: null atm_ij / ocn_ij / area");
    OGG_REQUIRE(counts, OGG_EARG, "ogg_regrid_transpose: null counts");
    const Layout l = layout(*p, n_entries);
    if (int e = ogg::check_workspace("ogg_regrid_transpose", workspace, workspace_bytes, l.total)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const long nk = p->NA * p->NB;
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_regrid_counts), st));
    int* cur = at<int>(workspace, l.cur);
    int* seg = at<int>(workspace, l.seg);
    long long* bsum = at<long long>(workspace, l.bsum);
    OGG_HIP_CHECK(hipMemsetAsync(cur, 0, (size_t)nk * 4, st));
    const List li{n_entries, p->ny, p->nx, p->NA, p->NB};
    if (n_entries > 0) {
        count_kernel<<<grid_for<NT>(n_entries, 8192), NT, 0, st>>>(li, atm_ij, ocn_ij, cur, counts);
        OGG_LAUNCH_CHECK();
    }
    if (int e = exclusive_scan<true>(cur, nk, bsum, nullptr, seg, st)) return e;   // seg[nk]: the total
    if (n_entries == 0) return OGG_OK;
    unsigned long long* key[2] = {at<unsigned long long>(workspace, l.key0), at<unsigned long long>(workspace, l.key1)};
    key_block_kernel<<<(unsigned)((n_entries + KEYSORT_NT - 1) / KEYSORT_NT), KEYSORT_NT, 0, st>>>(li, nk, atm_ij, ocn_ij, key[0]);
    OGG_LAUNCH_CHECK();
    int k = 0;
    for (long w = KEYSORT_NT; w < n_entries; w *= 2, ++k) {
        keysort_merge_kernel<<<grid_for<NT>(n_entries, 1L << 20), KEYSORT_NT, 0, st>>>(key[k & 1], n_entries, w, key[(k + 1) & 1]);
        OGG_LAUNCH_CHECK();
    }
    pairs_kernel<<<grid_for<NT>(n_entries, 8192), NT, 0, st>>>(n_entries, nk, p->nx, key[keysort_passes(n_entries) & 1], ocn_ij, area,
                                                           at<int>(workspace, l.pc), at<double>(workspace, l.pa));
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_regrid_dev(const ogg_regrid_params* p, const void* f, const double* a_atm, long n_list, void* workspace,
                              long workspace_bytes, double* values, double* cover, double* frac, int* n_entries, ogg_regrid_counts* counts,
                              void* stream) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(a_atm && counts, OGG_EARG, "ogg_regrid: null a_atm / counts");
    OGG_REQUIRE((f == nullptr) == (values == nullptr), OGG_EARG, "ogg_regrid: f and values are given together or not at all");
    OGG_REQUIRE(values || !cover, OGG_EARG, "ogg_regrid: cover needs values");
    OGG_REQUIRE(n_list >= 0 && n_list < (long)INT_MAX, OGG_EARG, "ogg_regrid: %ld entries (< 2^31)", n_list);
    const Layout l = layout(*p, n_list);
    if (int e = ogg::check_workspace("ogg_regrid", workspace, workspace_bytes, l.total)) return e;
    // OGG_REGRID_RECORDS: records a lane sums at once.  Their gathers are independent loads, so more records keep more of them in
    // flight per lane.  Measured at 1/8 degree (profiles/r12_regrid_time.json, ms for 1, 2, 4, 8): 57 levels onto 1 degree 21.3, 14.4,
    // 11.8, 10.5; onto 0.25 degree 18.0, 11.0, 8.5, 7.0; 12 records onto 1 degree 5.2, 3.5, 3.2, 4.2.
    int rec = 0, long_n = 0;
    if (int e = knob("OGG_REGRID_RECORDS", RECORDS_DEFAULT, 1, 8, &rec)) return e;
    // OGG_REGRID_LONG: cells of more entries are walked by whole wavefronts (a lane's walk costs its entry count, a wavefront's about
    // as much in shuffles but with the gathers 64 at a time and no other lane waiting).  Measured as above (ms for 128, 512, 4096): 57
    // levels onto 1 degree 8.9, 11.8, 30.7; onto 0.25 degree 5.5, 8.4, 15.6; 12 records onto 1 degree 2.9, 3.2, 6.8.
    if (int e = knob("OGG_REGRID_LONG", LONG_DEFAULT, 0, INT_MAX, &long_n)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const long nk = p->NA * p->NB;
    const int* seg = at<int>(workspace, l.seg);
    const int* pc = at<int>(workspace, l.pc);
    const double* pa = at<double>(workspace, l.pa);
    int* longs = at<int>(workspace, l.longs);
    long long* n_long = at<long long>(workspace, 0);
    // this step's counts start from zero on every call (entries and bad_entries are the transpose step's)
    OGG_HIP_CHECK(hipMemsetAsync(&counts->cells, 0, sizeof(ogg_regrid_counts) - offsetof(ogg_regrid_counts, cells), st));
    OGG_HIP_CHECK(hipMemsetAsync(n_long, 0, sizeof(long long), st));
    const unsigned blocks = (unsigned)((nk + NT - 1) / NT);
    static_kernel<<<blocks, NT, 0, st>>>(nk, long_n, seg, pa, a_atm, frac, n_entries, longs, n_long, counts);
    OGG_LAUNCH_CHECK();
    if (frac) {
        static_long_kernel<<<(unsigned)std::min<long>(nk, LONG_WAVES), 64, 0, st>>>(seg, pa, a_atm, longs, n_long, frac);
        OGG_LAUNCH_CHECK();
    }
    if (!values) return OGG_OK;
    const Geo g{nk, p->ny * p->nx, p->nrec, p->n_fill, p->normalize == OGG_REGRID_CELL ? 1 : 0, long_n, p->fill[0], p->fill[1]};
    const Bufs b{seg, pc, longs, pa, a_atm, n_long, values, cover, counts};
    int e = p->dtype == OGG_REMAP_FLOAT32 ? launch_regrid_r<float>(rec, st, g, f, b) : launch_regrid_r<double>(rec, st, g, f, b);
    if (e) return e;
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: field, list and areas copied to device memory, both steps, the results copied back (synchronous)
extern "C" int ogg_regrid(const ogg_regrid_params* p, const void* f, const int* atm_ij, const int* ocn_ij, const double* area, long n_entries,
                          const double* a_atm, double* values, double* cover, double* frac, int* n_out, ogg_regrid_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(n_entries >= 0 && n_entries < (long)INT_MAX, OGG_EARG, "ogg_regrid: %ld entries (< 2^31)", n_entries);
    OGG_REQUIRE(a_atm && counts && ((atm_ij && ocn_ij && area) || n_entries == 0), OGG_EARG,
                "ogg_regrid: null a_atm / atm_ij / ocn_ij / area / counts");
    OGG_REQUIRE((f == nullptr) == (values == nullptr), OGG_EARG, "ogg_regrid: f and values are given together or not at all");
    OGG_REQUIRE(values || !cover, OGG_EARG, "ogg_regrid: cover needs values");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t nk = (size_t)p->NA * p->NB, nout = (size_t)p->nrec * nk;
    const size_t fbytes = (size_t)p->nrec * p->ny * p->nx * (p->dtype == OGG_REMAP_FLOAT32 ? 4 : 8);
    const long wsb = layout(*p, n_entries).total;
    char *df = nullptr, *ws;
    int *da, *dox, *dn = nullptr;
    double *dar, *daa, *dv = nullptr, *dc = nullptr, *dfr = nullptr;
    ogg_regrid_counts* ct;
    if (int e = bufs.alloc(&da, (size_t)n_entries * 2)) return e;
    if (int e = bufs.alloc(&dox, (size_t)n_entries * 2)) return e;
    if (int e = bufs.alloc(&dar, (size_t)n_entries)) return e;
    if (int e = bufs.alloc(&daa, nk)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (values) {
        if (int e = bufs.alloc(&df, fbytes)) return e;
        if (int e = bufs.alloc(&dv, nout)) return e;
        if (int e = bufs.send(df, static_cast<const char*>(f), fbytes)) return e;
    }
    if (cover)
        if (int e = bufs.alloc(&dc, nout)) return e;
    if (frac)
        if (int e = bufs.alloc(&dfr, nk)) return e;
    if (n_out)
        if (int e = bufs.alloc(&dn, nk)) return e;
    if (n_entries > 0) {
        if (int e = bufs.send(da, atm_ij, (size_t)n_entries * 2)) return e;
        if (int e = bufs.send(dox, ocn_ij, (size_t)n_entries * 2)) return e;
        if (int e = bufs.send(dar, area, (size_t)n_entries)) return e;
    }
    if (int e = bufs.send(daa, a_atm, nk)) return e;
    if (int e = ogg_regrid_transpose_dev(p, da, dox, dar, n_entries, ws, wsb, ct, nullptr)) return e;
    if (int e = ogg_regrid_dev(p, df, daa, n_entries, ws, wsb, dv, dc, dfr, dn, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (values)
        if (int e = bufs.get(values, dv, nout)) return e;
    if (cover)
        if (int e = bufs.get(cover, dc, nout)) return e;
    if (frac)
        if (int e = bufs.get(frac, dfr, nk)) return e;
    if (n_out)
        if (int e = bufs.get(n_out, dn, nk)) return e;
    return OGG_OK;
}
