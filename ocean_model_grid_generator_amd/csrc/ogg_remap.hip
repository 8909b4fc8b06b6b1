// Conservative remap of lat-lon fields onto the model cells (include/ogg_hip.h, "Conservative remap"): a segmented, masked,
// weighted sum over the exchange list of ogg_xgrid for every record, then a fill of the wet cells the source leaves empty.
//
// remap_seg_kernel     one thread per list entry: an entry whose cell differs from its predecessor's starts the cell's segment, one
//                      whose cell differs from its successor's ends it (the list is sorted by cell: one pass, no sort).
// remap_kernel<T, C>   one wavefront per 64 consecutive cells of a model row, looping over a chunk of records (OGG_REMAP_RECORDS;
//                      default all), so every record's stores are 64 consecutive values and flags.  With C, a cell of at most
//                      REG entries keeps their areas and source offsets in registers for all records (the list is read from HBM
//                      once); longer cells re-read their entries per record (from cache: the wavefront's entries are a few KB).  A
//                      cell of more than OGG_REMAP_LONG entries (next to a pole) is walked by the whole wavefront, 64 entries at a
//                      time: every lane gathers one entry's area, value and product, and the sums take them in list order by
//                      shuffles, so the order of the additions is the definition's and no lane waits on one long cell alone.
// remap_fill_*         the fill front by front over frontier lists of (record, cell) pairs, all records in one launch per front.
//                      The flags are the state: a queued pair holds 4 + d mod 3 (d its distance) until the last launch sets it to
//                      OGG_REMAP_FILLED; neighbours of a cell at distance d lie at d - 1 .. d + 1, so d mod 3 tells them apart.  The
//                      first front comes from one scan of the flags; every later front from the previous one: a launch fills
//                      its front's pairs (the mean of the neighbours at d - 1, in the order S, W, E, N) and queues their
//                      unvisited wet neighbours with a 32-bit compare-and-swap on the flag byte (each pair is queued once), one
//                      atomicAdd per wavefront for the room.  Three slots of (start, length) in the workspace rotate through
//                      the launches, so no launch waits on the host; the host reads the next front's length every
//                      OGG_REMAP_FRONTS_PER_READ launches, and a launch on an empty front returns at once.
//
// Every value is a fixed function of the list, the source and the values at smaller distance: the result does not depend on the
// launch geometry or on the order in which the atomics land.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ogg_blocks.h"
#include "ogg_cells.h"
#include "ogg_common.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int NT = 256;                 // threads per workgroup (four wavefronts)
constexpr int REG = 8;                  // entries a lane keeps in registers across records
constexpr int LONG_DEFAULT = 32;        // cells with more entries are walked by the whole wavefront (OGG_REMAP_LONG)
constexpr int FRONTS_PER_READ_DEFAULT = 8;
constexpr int FILL_BLOCKS_DEFAULT = 1024;
constexpr long HEAD = 256;              // workspace: Head, then the segments, then the queue
constexpr unsigned char Q0 = 4;         // a queued pair at distance d holds Q0 + d % 3

static_assert(NT == BLOCKS_NT, "block_add sums over a workgroup of BLOCKS_NT threads");
static_assert(sizeof(ogg_remap_params) == 80, "ogg_remap_params layout");
static_assert(sizeof(ogg_remap_counts) == 64, "ogg_remap_counts layout");

struct Slot {
    unsigned long long lo, count;       // a front: queue[lo, lo + count)
};
struct Head {
    Slot slot[3];
    long long max_distance;
    unsigned long long seg_bad;         // entries of the segment step outside the cells
};
static_assert(sizeof(Head) <= HEAD, "workspace head");

// ---- segments ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void remap_seg_kernel(long n, const int* __restrict__ ocn, long m0, long ny, long nx, int2* seg,
                                                       unsigned long long* bad) {
    for (long k = (long)blockIdx.x * NT + threadIdx.x; k < n; k += (long)gridDim.x * NT) {
        const long i = ocn[2 * k], m = ocn[2 * k + 1] - m0;
        if (i < 0 || i >= nx || m < 0 || m >= ny) {
            atomicAdd(bad, 1ull);
            continue;
        }
        const long c = m * nx + i;
        const long prev = k > 0 ? (ocn[2 * k - 1] - m0) * nx + ocn[2 * k - 2] : -1;
        const long next = k + 1 < n ? (ocn[2 * k + 3] - m0) * nx + ocn[2 * k + 2] : -1;
        if (prev != c) seg[c].x = (int)k;
        if (next != c) seg[c].y = (int)(k + 1);
    }
}

// ---- remap -------------------------------------------------------------------------------------------------------
struct Geo {
    long ny, nx, NA, NB, nrec, rchunk;
    int n_fill, long_n;
    double fill0, fill1;
    const unsigned long long* seg_bad;
};

template <typename T, bool CACHE>
__global__ __launch_bounds__(NT) void remap_kernel(Geo g, const T* __restrict__ f, const int2* __restrict__ seg,
                                                   const int* __restrict__ atm_ij, const double* __restrict__ area,
                                                   const unsigned char* __restrict__ mask, double* __restrict__ out,
                                                   unsigned char* __restrict__ flags, ogg_remap_counts* counts) {
    const int lane = threadIdx.x & 63;
    const long tiles = (g.nx + 63) / 64;
    const long wave = (long)blockIdx.x * (NT / 64) + threadIdx.x / 64;
    const long row = wave / tiles, i = (wave % tiles) * 64 + lane;
    const bool inb = row < g.ny && i < g.nx;
    const long c = row * g.nx + i, ncell = g.ny * g.nx, nsrc = g.NA * g.NB;
    const T f0 = static_cast<T>(g.fill0), f1 = static_cast<T>(g.fill1);
    int s = 0, n = 0;
    bool wet = false;
    if (inb) {
        const int2 sg = seg[c];
        s = sg.x;
        n = sg.y - sg.x;
        wet = mask ? mask[c] != 0 : true;
        if (!wet || n < 0) n = 0;
    }
    const long r0 = (long)blockIdx.y * g.rchunk, r1 = r0 + g.rchunk < g.nrec ? r0 + g.rchunk : g.nrec;
    long long bad = 0;
    double ca[REG];
    int co[REG];
    if (CACHE) {
#pragma unroll
        for (int t = 0; t < REG; ++t) {
            ca[t] = 0.0;
            co[t] = -1;
            if (t < n && n <= REG && n <= g.long_n) {
                const int I = atm_ij[2 * (s + t)], J = atm_ij[2 * (s + t) + 1];
                if (I >= 0 && I < g.NA && J >= 0 && J < g.NB) {
                    ca[t] = area[s + t];
                    co[t] = (int)(J * g.NA + I);
                } else if (r0 == 0) {
                    ++bad;
                }
            }
        }
    }
    const bool is_long = n > g.long_n, cached = CACHE && n <= REG && !is_long;
    const unsigned long long longmask = __ballot(is_long);
    long long v_dry = 0, v_rem = 0, v_unf = 0;
    for (long r = r0; r < r1; ++r) {
        const T* fr = f + r * nsrc;
        double W = 0.0, S = 0.0;
        if (cached) {
#pragma unroll
            for (int t = 0; t < REG; ++t) {
                if (co[t] >= 0) {
                    const T v = fr[co[t]];
                    if (!missing(v, f0, f1, g.n_fill)) {
                        W += ca[t];
                        S += ca[t] * (double)v;
                    }
                }
            }
        } else if (!is_long) {
            for (int k = s; k < s + n; ++k) {
                const int I = atm_ij[2 * k], J = atm_ij[2 * k + 1];
                if (I < 0 || I >= g.NA || J < 0 || J >= g.NB) {
                    bad += r == 0;
                    continue;
                }
                const double a = area[k];
                const T v = fr[(long)J * g.NA + I];
                if (!missing(v, f0, f1, g.n_fill)) {
                    W += a;
                    S += a * (double)v;
                }
            }
        }
        // the long cells, one after the other, by the whole wavefront (uniform control flow: longmask is the same in every lane)
        for (unsigned long long m = longmask; m; m &= m - 1) {
            const int L = __ffsll((long long)m) - 1;
            const int sL = __shfl(s, L, 64), nL = __shfl(n, L, 64);
            double w = 0.0, sum = 0.0;
            for (int base = 0; base < nL; base += 64) {
                const int k = sL + base + lane;
                double a = 0.0, p = 0.0;
                int ok = 0;
                if (base + lane < nL) {
                    const int I = atm_ij[2 * k], J = atm_ij[2 * k + 1];
                    if (I >= 0 && I < g.NA && J >= 0 && J < g.NB) {
                        const T v = fr[(long)J * g.NA + I];
                        a = area[k];
                        ok = !missing(v, f0, f1, g.n_fill);
                        p = a * (double)v;
                    } else {
                        bad += r == 0;
                    }
                }
                const int cnt = nL - base < 64 ? nL - base : 64;
                for (int t = 0; t < cnt; ++t) {
                    const double at = __shfl(a, t, 64), pt = __shfl(p, t, 64);
                    if (__shfl(ok, t, 64)) {
                        w += at;
                        sum += pt;
                    }
                }
            }
            if (lane == L) W = w, S = sum;
        }
        if (inb) {
            double v = OGG_REMAP_FILL;
            unsigned char fl = OGG_REMAP_DRY;
            if (!wet) {
                ++v_dry;
            } else if (W > 0.0) {
                v = S / W;
                fl = OGG_REMAP_REMAPPED;
                ++v_rem;
            } else {
                fl = OGG_REMAP_UNFILLED;
                ++v_unf;
            }
            out[r * ncell + c] = v;
            flags[r * ncell + c] = fl;
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) bad += (long long)*g.seg_bad;
    long long v[4] = {v_dry, v_rem, v_unf, bad};
    long long* const dst[4] = {&counts->dry, &counts->remapped, &counts->unfilled, &counts->bad_entries};
    block_add<4>(v, dst);
}

// ---- fill --------------------------------------------------------------------------------------------------------
struct Topo {
    CellTopo cells;
    long ncell;
    unsigned long long total;           // nrec * ncell
};

// the flag byte at idx from `want` to `to` by a compare-and-swap of its 32-bit word (flags: 4-byte aligned, rounded up to 4 bytes)
__device__ inline bool claim(unsigned char* flags, unsigned long long idx, unsigned want, unsigned to) {
    unsigned* w = reinterpret_cast<unsigned*>(flags + (idx & ~3ull));
    const int sh = (int)(idx & 3) * 8;
    unsigned old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        if (((old >> sh) & 0xFFu) != want) return false;
        const unsigned nw = (old & ~(0xFFu << sh)) | (to << sh);
        if (__hip_atomic_compare_exchange_strong(w, &old, nw, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return true;
    }
}

// room for cnt items of every lane of the (converged) wavefront in one atomicAdd: the lane's first position
__device__ inline unsigned long long wave_reserve(unsigned cnt, unsigned long long* counter) {
    const int lane = threadIdx.x & 63;
    unsigned incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const unsigned total = __shfl(incl, 63, 64);
    unsigned long long base = 0;
    if (lane == 63 && total) base = atomicAdd(counter, (unsigned long long)total);
    base = __shfl(base, 63, 64);
    return base + incl - cnt;
}

__device__ inline unsigned long long load_agent(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the first front: every unvisited pair (flag OGG_REMAP_UNFILLED) with a remapped neighbour, four flags per thread
__global__ __launch_bounds__(NT) void remap_fill_first_kernel(Topo t, unsigned char* flags, unsigned* queue, Head* h) {
    const int lane = threadIdx.x & 63;
    const unsigned long long words = (t.total + 3) / 4;
    for (unsigned long long b = (unsigned long long)blockIdx.x * NT + (threadIdx.x & ~63u); b < words;
         b += (unsigned long long)gridDim.x * NT) {
        const unsigned long long wi = b + lane;
        unsigned cnt = 0, take = 0;
        if (wi < words) {
            const unsigned w = reinterpret_cast<const unsigned*>(flags)[wi];
            for (int q = 0; q < 4; ++q) {
                const unsigned long long idx = wi * 4 + q;
                if (idx >= t.total || ((w >> (8 * q)) & 0xFFu) != OGG_REMAP_UNFILLED) continue;
                const long r = (long)(idx / t.ncell), c = (long)(idx % t.ncell);
                long nb[4];
                face_neighbours(t.cells, c, nb);   // a neighbour that does not exist is skipped
                bool any = false;
                for (int k = 0; k < 4; ++k) any = any || (nb[k] >= 0 && flags[r * t.ncell + nb[k]] == OGG_REMAP_REMAPPED);
                if (any) take |= 1u << q, ++cnt;
            }
        }
        unsigned long long pos = wave_reserve(cnt, &h->slot[1].count);
        for (int q = 0; q < 4; ++q)
            if (take & (1u << q)) {
                const unsigned long long idx = wi * 4 + q;
                flags[idx] = Q0 + 1;   // only this thread changes this pair in this launch
                queue[pos++] = (unsigned)idx;
            }
    }
}

// front k (k >= 1): fill its pairs, queue front k + 1
__global__ __launch_bounds__(NT) void remap_fill_front_kernel(Topo t, int k, double* val, unsigned char* flags, unsigned* queue, Head* h) {
    const unsigned long long lo = load_agent(&h->slot[k % 3].lo), n = load_agent(&h->slot[k % 3].count);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h->slot[(k + 1) % 3].lo = lo + n;   // read by launch k + 1
        h->slot[(k + 2) % 3].count = 0;     // the front of launch k - 1, the append counter of launch k + 1
        if (n) h->max_distance = k;
    }
    if (n == 0) return;
    const int lane = threadIdx.x & 63;
    const unsigned prev = k == 1 ? (unsigned)OGG_REMAP_REMAPPED : Q0 + (unsigned)((k - 1) % 3), next = Q0 + (unsigned)((k + 1) % 3);
    for (unsigned long long b = (unsigned long long)blockIdx.x * NT + (threadIdx.x & ~63u); b < n; b += (unsigned long long)gridDim.x * NT) {
        const unsigned long long q = b + lane;
        unsigned cnt = 0, take = 0;
        long nb[4] = {-1, -1, -1, -1};
        unsigned long long rb = 0;
        if (q < n) {
            const unsigned long long idx = queue[lo + q];
            const long r = (long)(idx / t.ncell), c = (long)(idx % t.ncell);
            rb = (unsigned long long)r * t.ncell;
            face_neighbours(t.cells, c, nb);
            double s = 0.0;
            int m = 0;
            for (int d = 0; d < 4; ++d)
                if (nb[d] >= 0 && flags[rb + nb[d]] == prev) {
                    s += val[rb + nb[d]];
                    ++m;
                }
            val[idx] = s / (double)m;   // m >= 1: the pair was queued by a neighbour at distance k - 1
            for (int d = 0; d < 4; ++d)
                if (nb[d] >= 0 && claim(flags, rb + nb[d], OGG_REMAP_UNFILLED, next)) take |= 1u << d, ++cnt;
        }
        unsigned long long pos = lo + n + wave_reserve(cnt, &h->slot[(k + 1) % 3].count);
        for (int d = 0; d < 4; ++d)
            if (take & (1u << d)) queue[pos++] = (unsigned)(rb + nb[d]);
    }
}

// the queued pairs: filled below n_done, back to unfilled above (the front beyond fill_max); the counts
__global__ __launch_bounds__(NT) void remap_fill_last_kernel(unsigned long long n_done, unsigned long long n_total, const unsigned* queue,
                                                             unsigned char* flags, ogg_remap_counts* counts, long long max_distance,
                                                             long long launches) {
    long long v[2] = {0, 0};
    for (unsigned long long q = (unsigned long long)blockIdx.x * NT + threadIdx.x; q < n_total; q += (unsigned long long)gridDim.x * NT) {
        const bool done = q < n_done;
        flags[queue[q]] = done ? OGG_REMAP_FILLED : OGG_REMAP_UNFILLED;
        v[0] += done;
    }
    v[1] = -v[0];
    long long* const dst[2] = {&counts->filled, &counts->unfilled};
    block_add<2>(v, dst);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts->max_distance = max_distance;
        counts->fronts = max_distance;
        counts->launches = launches;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_remap_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "remap: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "remap: %ld x %ld cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE(p->m0 >= 0 && p->m0 <= (long)INT_MAX, OGG_EARG, "remap: first row %ld", p->m0);
    OGG_REQUIRE(p->NA >= 1 && p->NB >= 1 && p->NA <= (long)INT_MAX && p->NB <= (long)INT_MAX && p->NA * p->NB < (1L << 31), OGG_EARG,
                "remap: %ld x %ld source cells: NA, NB >= 1 and NA * NB < 2^31", p->NA, p->NB);
    OGG_REQUIRE(p->nrec >= 1 && p->nrec <= (long)INT_MAX && p->nrec * p->ny * p->nx < (1L << 32), OGG_EARG,
                "remap: %ld records of %ld x %ld cells: nrec >= 1 and nrec * ny * nx < 2^32", p->nrec, p->ny, p->nx);
    OGG_REQUIRE(p->dtype == OGG_REMAP_FLOAT32 || p->dtype == OGG_REMAP_FLOAT64, OGG_EARG, "remap: source dtype %d (0: float32, 1: float64)",
                p->dtype);
    OGG_REQUIRE(p->n_fill >= 0 && p->n_fill <= OGG_REMAP_MAX_FILLS, OGG_EARG, "remap: %d fill values (at most %d)", p->n_fill,
                OGG_REMAP_MAX_FILLS);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "remap: topology flags %d", p->topology);
    return OGG_OK;
}

struct Layout {
    long seg, queue, total;
};

Layout layout(const ogg_remap_params& p) {
    ogg::Sections s{HEAD};
    return Layout{s.take(p.ny * p.nx * 8), s.take(p.nrec * p.ny * p.nx * 4), s.off};   // a braced list is evaluated left to right
}

long ws_bytes(const ogg_remap_params& p) { return layout(p).total; }

template <typename T, bool C>
void launch_remap(dim3 grid, hipStream_t st, const Geo& g, const void* f, const int2* seg, const int* atm_ij, const double* area,
                  const unsigned char* mask, double* out, unsigned char* flags, ogg_remap_counts* counts) {
    remap_kernel<T, C><<<grid, NT, 0, st>>>(g, static_cast<const T*>(f), seg, atm_ij, area, mask, out, flags, counts);
}

}  // namespace

extern "C" long ogg_remap_workspace_bytes(const ogg_remap_params* p) {
    if (!p || check_params(p) != OGG_OK) return -1;
    return ws_bytes(*p);
}

extern "C" int ogg_remap_check(const ogg_remap_params* p) { return check_params(p); }

extern "C" int ogg_remap_segments_dev(const ogg_remap_params* p, const int* ocn_ij, long n_entries, void* workspace, long workspace_bytes,
                                      void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_remap_segments", workspace, workspace_bytes, ws_bytes(*p))) return e;
    OGG_REQUIRE(n_entries >= 0 && n_entries < (long)INT_MAX, OGG_EARG, "ogg_remap_segments: %ld entries", n_entries);
    OGG_REQUIRE(ocn_ij || n_entries == 0, OGG_EARG, "ogg_remap_segments: null ocn_ij");
    hipStream_t st = ogg::as_stream(stream);
    Head* h = static_cast<Head*>(workspace);
    int2* seg = at<int2>(workspace, layout(*p).seg);
    OGG_HIP_CHECK(hipMemsetAsync(&h->seg_bad, 0, sizeof(h->seg_bad), st));
    OGG_HIP_CHECK(hipMemsetAsync(seg, 0, (size_t)p->ny * p->nx * 8, st));
    if (n_entries == 0) return OGG_OK;
    remap_seg_kernel<<<grid_for<NT>(n_entries, 4096), NT, 0, st>>>(n_entries, ocn_ij, p->m0, p->ny, p->nx, seg, &h->seg_bad);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_remap_dev(const ogg_remap_params* p, const void* f, const int* atm_ij, const double* area, long n_entries,
                             const unsigned char* mask, const void* workspace, long workspace_bytes, double* values, unsigned char* flags,
                             ogg_remap_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_remap", workspace, workspace_bytes, ws_bytes(*p))) return e;
    OGG_REQUIRE(n_entries >= 0 && n_entries < (long)INT_MAX, OGG_EARG, "ogg_remap: %ld entries", n_entries);
    OGG_REQUIRE(f && values && flags && counts && ((atm_ij && area) || n_entries == 0), OGG_EARG,
                "ogg_remap: null f / atm_ij / area / values / flags / counts");
    OGG_REQUIRE(((uintptr_t)flags & 3) == 0, OGG_EARG, "ogg_remap: flags must be 4-byte aligned");
    int rec = 0, long_n = 0, cache = 0;
    if (int e = knob("OGG_REMAP_RECORDS", 0, 0, INT_MAX, &rec)) return e;
    if (int e = knob("OGG_REMAP_LONG", LONG_DEFAULT, 1, 1 << 20, &long_n)) return e;
    if (int e = knob("OGG_REMAP_CACHE", 1, 0, 1, &cache)) return e;
    const long rchunk = rec == 0 ? p->nrec : std::min<long>(rec, p->nrec);
    const long nchunk = (p->nrec + rchunk - 1) / rchunk;
    OGG_REQUIRE(nchunk <= 65535, OGG_EARG, "ogg_remap: %ld record chunks (OGG_REMAP_RECORDS=%d): at most 65535", nchunk, rec);
    hipStream_t st = ogg::as_stream(stream);
    const Head* h = static_cast<const Head*>(workspace);
    const int2* seg = at<int2>(workspace, layout(*p).seg);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_remap_counts), st));
    const Geo g{p->ny, p->nx, p->NA, p->NB, p->nrec, rchunk, p->n_fill, long_n, p->fill[0], p->fill[1], &h->seg_bad};
    const long waves = p->ny * ((p->nx + 63) / 64);
    const dim3 grid((unsigned)((waves + NT / 64 - 1) / (NT / 64)), (unsigned)nchunk);
    if (p->dtype == OGG_REMAP_FLOAT32)
        (cache ? launch_remap<float, true> : launch_remap<float, false>)(grid, st, g, f, seg, atm_ij, area, mask, values, flags, counts);
    else
        (cache ? launch_remap<double, true> : launch_remap<double, false>)(grid, st, g, f, seg, atm_ij, area, mask, values, flags, counts);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_remap_fill_dev(const ogg_remap_params* p, void* workspace, long workspace_bytes, double* values, unsigned char* flags,
                                  ogg_remap_counts* counts, void* stream) {
    if (int e = check_params(p)) return e;
    if (int e = ogg::check_workspace("ogg_remap_fill", workspace, workspace_bytes, ws_bytes(*p))) return e;
    OGG_REQUIRE(p->m0 == 0, OGG_EARG, "ogg_remap_fill: the fill needs the whole grid (m0 = %ld)", p->m0);
    OGG_REQUIRE(values && flags && counts, OGG_EARG, "ogg_remap_fill: null values / flags / counts");
    OGG_REQUIRE(((uintptr_t)flags & 3) == 0, OGG_EARG, "ogg_remap_fill: flags must be 4-byte aligned");
    int per_read = 0, blocks = 0;
    if (int e = knob("OGG_REMAP_FRONTS_PER_READ", FRONTS_PER_READ_DEFAULT, 1, 1 << 16, &per_read)) return e;
    if (int e = knob("OGG_REMAP_FILL_BLOCKS", FILL_BLOCKS_DEFAULT, 1, 1 << 16, &blocks)) return e;
    hipStream_t st = ogg::as_stream(stream);
    Head* h = static_cast<Head*>(workspace);
    unsigned* queue = at<unsigned>(workspace, layout(*p).queue);
    const Topo t{cell_topo(p->ny, p->nx, p->topology), p->ny * p->nx, (unsigned long long)(p->nrec * p->ny * p->nx)};
    OGG_HIP_CHECK(hipMemsetAsync(h, 0, sizeof(Slot) * 3 + sizeof(long long), st));
    remap_fill_first_kernel<<<grid_for<NT>((long)((t.total + 3) / 4), blocks), NT, 0, st>>>(t, flags, queue, h);
    OGG_LAUNCH_CHECK();
    int k = 1;
    long long launches = 0;
    Head hh;
    for (;;) {
        for (int j = 0; j < per_read && !(p->fill_max >= 0 && k > p->fill_max); ++j, ++k, ++launches) {
            remap_fill_front_kernel<<<(unsigned)blocks, NT, 0, st>>>(t, k, values, flags, queue, h);
            OGG_LAUNCH_CHECK();
        }
        OGG_HIP_CHECK(hipMemcpyAsync(&hh, h, sizeof(Head), hipMemcpyDeviceToHost, st));
        OGG_HIP_CHECK(hipStreamSynchronize(st));
        if (hh.slot[k % 3].count == 0 || (p->fill_max >= 0 && k > p->fill_max)) break;
    }
    const unsigned long long n_done = hh.slot[k % 3].lo, n_total = n_done + hh.slot[k % 3].count;
    remap_fill_last_kernel<<<grid_for<NT>((long)std::max<unsigned long long>(n_total, 1), blocks), NT, 0, st>>>(
        n_done, n_total, queue, flags, counts, hh.max_distance, launches);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: source, list and mask copied to device memory, the three steps, the results copied back (synchronous)
extern "C" int ogg_remap(const ogg_remap_params* p, const void* f, const int* atm_ij, const int* ocn_ij, const double* area, long n_entries,
                         const unsigned char* mask, int do_fill, double* values, unsigned char* flags, ogg_remap_counts* counts) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(n_entries >= 0 && n_entries < (long)INT_MAX, OGG_EARG, "ogg_remap: %ld entries", n_entries);
    OGG_REQUIRE(f && values && flags && counts && ((atm_ij && ocn_ij && area) || n_entries == 0), OGG_EARG,
                "ogg_remap: null f / atm_ij / ocn_ij / area / values / flags / counts");
    OGG_REQUIRE(!do_fill || p->m0 == 0, OGG_EARG, "ogg_remap: the fill needs the whole grid (m0 = %ld)", p->m0);
    ogg::Buffers bufs;   // freed on every exit path
    const size_t ncell = (size_t)p->ny * p->nx, npair = (size_t)p->nrec * ncell;
    const size_t fbytes = (size_t)p->nrec * p->NA * p->NB * (p->dtype == OGG_REMAP_FLOAT32 ? 4 : 8);
    const long wsb = ws_bytes(*p);
    char *df, *ws;
    int *da, *dox;
    double *dar, *dv;
    unsigned char *dm = nullptr, *dfl;
    ogg_remap_counts* ct;
    if (int e = bufs.alloc(&df, fbytes)) return e;
    if (int e = bufs.alloc(&da, (size_t)n_entries * 2)) return e;
    if (int e = bufs.alloc(&dox, (size_t)n_entries * 2)) return e;
    if (int e = bufs.alloc(&dar, (size_t)n_entries)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&dv, npair)) return e;
    if (int e = bufs.alloc(&dfl, (npair + 3) / 4 * 4)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = bufs.send(df, static_cast<const char*>(f), fbytes)) return e;
    if (n_entries > 0) {
        if (int e = bufs.send(da, atm_ij, (size_t)n_entries * 2)) return e;
        if (int e = bufs.send(dox, ocn_ij, (size_t)n_entries * 2)) return e;
        if (int e = bufs.send(dar, area, (size_t)n_entries)) return e;
    }
    if (mask)
        if (int e = bufs.put(&dm, mask, ncell)) return e;
    if (int e = ogg_remap_segments_dev(p, dox, n_entries, ws, wsb, nullptr)) return e;
    if (int e = ogg_remap_dev(p, df, da, dar, n_entries, dm, ws, wsb, dv, dfl, ct, nullptr)) return e;
    if (do_fill)
        if (int e = ogg_remap_fill_dev(p, ws, wsb, dv, dfl, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(values, dv, npair)) return e;
    if (int e = bufs.get(flags, dfl, npair)) return e;
    return OGG_OK;
}
