// Curvilinear source x ocean exchange grid (include/ogg_hip.h, "Exchange grid with a curvilinear source grid"): every non-empty
// overlap of a cell of a logically rectangular great-circle mesh with a MOM6 h-cell of the stitched supergrid, with its area.
//
// sets      src_record_kernel: one thread per source cell forms its corner vectors, status, A_src, the four normals of the oriented
//           cell and its padded box, in the record layout of ogg_box_index.h; build_box_index registers the valid unmasked cells in
//           the cubes their boxes touch (or on the large-cells list).  tgt_record_kernel: the same for the band's model cells (the
//           twelve owner's doubles hold the corner vectors, A_poly follows the box).
// pairs     pair_kernel: one thread per model cell walks the cubes its box touches and the large list.  A source cell registered in
//           several of those cubes is taken once, in the cube that holds max(lo_target, lo_source) by component: that point lies in both
//           boxes, so both cells are registered there.  First pass: the candidates of every cell, then an exclusive scan; second
//           pass: the keys (cell << 32) | q at the cell's offset, in the order the cubes gave them.
// sort      runs of KEYSORT_NT keys by rank in LDS, then the merge passes of ogg_keysort.h: the list is (cell, q) ascending whatever
//           the index and the atomics' order.  Nothing per cell is sized by its number of candidates.
// clip      clip_kernel: one lane per candidate of the flattened sorted list (a coarse cell under a fine source and the reverse both
//           balance).  The Sutherland-Hodgman chain lives in registers as in ogg_clip.h; that chain is written for two coordinates and
//           an axis-aligned line per pass (its crossing sets one coordinate to the line's value), so this is its 3-D twin: a vertex
//           is a unit vector, a pass a half-space T >= 0 (T exactly 0 at the edge's own ends), a crossing is normalised.  The last
//           pass feeds the O3 fan.  A_x per candidate (-1 when the pair is not kept), the kept pairs per wavefront by ballot,
//           xgrid_scan_kernel for their offsets.
// write     write_kernel: the kept pairs compacted in list order.
//
// clip_kernel's registers: four passes of two vertices with their measures, the fan's two vertices and the vertex in flight.  The
// source cell's normals and corners are read from its records where a vertex is measured (L1 hits): held in registers they cost 48
// VGPRs, and the kernel then spilled.  The compiler's resource usage is in profiles/r22_xgrid_curv_kernels.md.
#include <algorithm>
#include <climits>
#include <cmath>

#include "ogg_box_index.h"
#include "ogg_clip.h"
#include "ogg_keysort.h"

#pragma clang fp contract(off)

namespace {

using namespace ogg::xg;
using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int NT = BLOCKS_NT;
constexpr int TNF = BOX_NF + 1;          // doubles of a model cell's record: P0 .. P3, box lo, box hi, A_poly
constexpr long long MAGIC = 0x78637572766cll;
constexpr long CUBES_WORD = 64;          // byte offset in the sets workspace's head of the index's cubes per axis (a long long)

static_assert(sizeof(ogg_xgrid_curv_src) == 48, "ogg_xgrid_curv_src layout");
static_assert(sizeof(ogg_xgrid_curv_counts) == 112, "ogg_xgrid_curv_counts layout");
static_assert(KEYSORT_NT == NT, "the key runs are sorted by workgroups of NT threads");

enum { ST_OK = 0, ST_DEGENERATE = 1, ST_WIDE = 2, ST_INVERTED = 3, ST_FLAT = 4 };

struct V3 {
    double x, y, z;
};

// a.b summed x, y, z left to right: the cubed-sphere section's dot product and point location's T(p; n) are the same expression
OGG_DEV double dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

OGG_DEV V3 cross3(const V3& a, const V3& b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// Omega3(a, b, c) = 2 atan2(a . ((b - a) x (c - a)), 1 + a.b + b.c + c.a)
OGG_DEV double omega3(const V3& a, const V3& b, const V3& c) {
    const V3 u{b.x - a.x, b.y - a.y, b.z - a.z}, v{c.x - a.x, c.y - a.y, c.z - a.z};
    return 2.0 * atan2(dot(a, cross3(u, v)), 1.0 + dot(a, b) + dot(b, c) + dot(c, a));
}

OGG_DEV double fan4(const V3* P, double Re2) { return Re2 * (omega3(P[0], P[1], P[2]) + omega3(P[0], P[2], P[3])); }

// the corner vectors, the status DEGENERATE / WIDE / INVERTED / OK and the area (NaN for the first two) of four corners in degrees
OGG_DEV int cell_vectors(const double* cx, const double* cy, double Re2, V3* P, double* A) {
    *A = NAN;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) finite = finite && isfinite(cx[k]) && isfinite(cy[k]);
    if (!finite) return ST_DEGENERATE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double lam = mod360(cx[k]) * D2R, phi = cy[k] * D2R;
        const double cp = cos(phi);
        P[k] = V3{cp * cos(lam), cp * sin(lam), sin(phi)};
    }
    bool wide = false;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i + 1; j < 4; ++j) wide = wide || dot(P[i], P[j]) < OGG_XGRID_CS_COS_WIDE;
    if (wide) return ST_WIDE;
    *A = fan4(P, Re2);
    return *A > 0.0 ? ST_OK : ST_INVERTED;
}

// the record of a valid cell: twelve doubles of the caller's, then the padded box of the corner vectors
OGG_DEV void box_of(const V3* P, double* r) {
    const double q[4][3] = {{P[0].x, P[0].y, P[0].z}, {P[1].x, P[1].y, P[1].z}, {P[2].x, P[2].y, P[2].z}, {P[3].x, P[3].y, P[3].z}};
    padded_box(q, r);
}

struct SrcD {
    const double *x, *y;
    const unsigned char* mask;
    long NA, NB, ld;
};

// ---- sets ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void src_record_kernel(SrcD s, double Re2, double* __restrict__ rec, double* __restrict__ sq,
                                                        double* __restrict__ asrc, double* __restrict__ a_src,
                                                        ogg_xgrid_curv_counts* counts) {
    const long nq = s.NA * s.NB;
    long long v[6] = {0, 0, 0, 0, 0, 0};   // cells, degenerate, wide, reversed, flat, masked
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < nq; q += (long)gridDim.x * NT) {
        const long J = q / s.NA, I = q - J * s.NA;
        const long k[4] = {J * s.ld + I, J * s.ld + I + 1, (J + 1) * s.ld + I + 1, (J + 1) * s.ld + I};
        double cx[4], cy[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) cx[c] = s.x[k[c]], cy[c] = s.y[k[c]];
        V3 Q[4] = {};
        double A;
        int st = cell_vectors(cx, cy, Re2, Q, &A);
        bool reversed = false;
        if (st == ST_INVERTED) {
            if (A < 0.0) {   // REVERSED: the corners in the order 0, 3, 2, 1
                const V3 t = Q[1];
                Q[1] = Q[3], Q[3] = t;
                A = fan4(Q, Re2);
                reversed = true;
            }
            st = A > 0.0 ? ST_OK : ST_FLAT;
        }
        const bool masked = s.mask && s.mask[q] == 0;
        double* r = rec + q * BOX_NF;
        if (st == ST_OK && !masked) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const V3 n = cross3(Q[e], Q[(e + 1) & 3]);
                r[3 * e] = n.x, r[3 * e + 1] = n.y, r[3 * e + 2] = n.z;
            }
            box_of(Q, r);
        } else {
            for (int f = 0; f < 12; ++f) r[f] = 0.0;
            empty_box(r);
        }
        const bool valid = st == ST_OK && !masked;   // (only a valid cell's corners are read)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            sq[12 * q + 3 * c] = valid ? Q[c].x : 0.0, sq[12 * q + 3 * c + 1] = valid ? Q[c].y : 0.0, sq[12 * q + 3 * c + 2] = valid ? Q[c].z : 0.0;
        asrc[q] = A;
        a_src[q] = A;
        v[0] += 1, v[1] += st == ST_DEGENERATE, v[2] += st == ST_WIDE, v[3] += st == ST_OK && reversed, v[4] += st == ST_FLAT;
        v[5] += masked;
    }
    long long* const dst[6] = {&counts->src_cells, &counts->src_degenerate, &counts->src_wide, &counts->src_reversed, &counts->src_flat,
                               &counts->src_masked};
    block_add<6>(v, dst);
}

__global__ __launch_bounds__(NT) void tgt_record_kernel(Geo g, double* __restrict__ rec, double* __restrict__ a_poly,
                                                        ogg_xgrid_curv_counts* counts) {
    long long v[5] = {0, 0, 0, 0, 0};   // cells, degenerate, wide, inverted, masked
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < g.ncells; c += (long)gridDim.x * NT) {
        double cx[4], cy[4];
        cell_corners(g, c, cx, cy);
        V3 P[4];
        double A;
        const int st = cell_vectors(cx, cy, g.Re2, P, &A);
        const bool masked = g.mask && g.mask[c] == 0;
        double* r = rec + c * TNF;
        if (st == ST_OK && !masked) {
#pragma unroll
            for (int k = 0; k < 4; ++k) r[3 * k] = P[k].x, r[3 * k + 1] = P[k].y, r[3 * k + 2] = P[k].z;
            box_of(P, r);
        } else {
            for (int f = 0; f < 12; ++f) r[f] = 0.0;
            empty_box(r);
        }
        r[BOX_NF] = A;
        a_poly[c] = A;
        v[0] += 1, v[1] += st == ST_DEGENERATE, v[2] += st == ST_WIDE, v[3] += st == ST_INVERTED, v[4] += masked;
    }
    long long* const dst[5] = {&counts->cells, &counts->degenerate, &counts->wide, &counts->inverted, &counts->masked};
    block_add<5>(v, dst);
}

// ---- pairs ---------------------------------------------------------------------------------------------------------
struct Index {
    const double* rec;
    const BoxHead* head;
    const int *start, *entries, *large;   // the cubes per axis are the head's G, which the index step wrote: every later step walks
                                          // the geometry that was built, whatever the knobs say by then
};

OGG_DEV bool boxes_meet(const double* t, const double* s) {
    return t[BOX_LO] <= s[BOX_HI] && s[BOX_LO] <= t[BOX_HI] && t[BOX_LO + 1] <= s[BOX_HI + 1] && s[BOX_LO + 1] <= t[BOX_HI + 1] &&
           t[BOX_LO + 2] <= s[BOX_HI + 2] && s[BOX_LO + 2] <= t[BOX_HI + 2];
}

// WRITE = false: cnt[c] the candidates of model cell c; WRITE = true: their keys from keys[off[c]] on
template <bool WRITE>
__global__ __launch_bounds__(NT) void pair_kernel(long ncells, const double* __restrict__ trec, Index ix, int* __restrict__ cnt,
                                                  const int* __restrict__ off, unsigned long long* __restrict__ keys) {
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < ncells; c += (long)gridDim.x * NT) {
        const double* t = trec + c * TNF;
        int n = 0;
        const long base = WRITE ? (long)off[c] : 0;
        if (t[BOX_LO] <= t[BOX_HI]) {
            const long nlarge = (long)ix.head->nlarge;
            for (long k = 0; k < nlarge; ++k) {
                const int q = ix.large[k];
                if (boxes_meet(t, ix.rec + (long)q * BOX_NF)) {
                    if (WRITE) keys[base + n] = ((unsigned long long)c << 32) | (unsigned)q;
                    ++n;
                }
            }
            const int G = (int)ix.head->G;
            int b0[3], b1[3];
            for (int a = 0; a < 3; ++a) b0[a] = cube_of(t[BOX_LO + a], G), b1[a] = cube_of(t[BOX_HI + a], G);
            for (int kz = b0[2]; kz <= b1[2]; ++kz)
                for (int ky = b0[1]; ky <= b1[1]; ++ky)
                    for (int kx = b0[0]; kx <= b1[0]; ++kx) {
                        const int b = kx + G * (ky + G * kz);
                        for (long e = ix.start[b]; e < ix.start[b + 1]; ++e) {
                            const int q = ix.entries[e];
                            const double* s = ix.rec + (long)q * BOX_NF;
                            if (!boxes_meet(t, s)) continue;
                            // once: in the cube of the larger of the two lower corners
                            if (cube_of(fmax(t[BOX_LO], s[BOX_LO]), G) != kx || cube_of(fmax(t[BOX_LO + 1], s[BOX_LO + 1]), G) != ky ||
                                cube_of(fmax(t[BOX_LO + 2], s[BOX_LO + 2]), G) != kz)
                                continue;
                            if (WRITE) keys[base + n] = ((unsigned long long)c << 32) | (unsigned)q;
                            ++n;
                        }
                    }
        }
        if (!WRITE) cnt[c] = n;
    }
}

// ---- sort ----------------------------------------------------------------------------------------------------------
// runs of KEYSORT_NT consecutive keys sorted in LDS by rank (the keys are unique)
__global__ __launch_bounds__(KEYSORT_NT) void key_run_kernel(const unsigned long long* __restrict__ in, long n,
                                                             unsigned long long* __restrict__ out) {
    __shared__ unsigned long long lk[KEYSORT_NT];
    const long e = (long)blockIdx.x * KEYSORT_NT + threadIdx.x;
    const unsigned long long key = e < n ? in[e] : ULLONG_MAX;
    lk[threadIdx.x] = key;
    __syncthreads();
    int rank = 0;
    for (int q = 0; q < KEYSORT_NT; ++q) rank += lk[q] < key;
    if (e < n) out[(long)blockIdx.x * KEYSORT_NT + rank] = key;
}

// ---- clip ----------------------------------------------------------------------------------------------------------
// One pass of the chain: its first vertex and the vertex before the current one, each with its measure.
struct Pass3 {
    V3 f, p;
    double fd, pd;
    bool started, fin, pin;
};

// the O3 fan from vertex 0 of a polygon, its vertices pushed one by one
struct Fan3 {
    V3 v0, vk;
    double s;
    int n;
    OGG_DEV void push(const V3& v) {
        if (n == 0)
            v0 = v, s = 0.0;
        else if (n >= 2)
            s = s + omega3(v0, vk, v);
        vk = v, ++n;
    }
};

struct Chain {
    Pass3 ps[4];
    const double *nrm, *q;   // the four normals and the four corners of the oriented source cell, twelve doubles each
    Fan3 fan;
};

// the measure of v against edge E = (Q_E, Q_E+1): exactly 0 at the edge's own ends (shared corners)
template <int E>
OGG_DEV double measure(const Chain& k, const V3& v) {
    const double *a = k.q + 3 * E, *b = k.q + 3 * ((E + 1) & 3);
    const bool end = (v.x == a[0] && v.y == a[1] && v.z == a[2]) || (v.x == b[0] && v.y == b[1] && v.z == b[2]);
    return end ? 0.0 : dot(v, V3{k.nrm[3 * E], k.nrm[3 * E + 1], k.nrm[3 * E + 2]});
}

// the crossing of the edge (a, b) whose measures da, db lie on two sides: the ends in lexicographic order
OGG_DEV V3 crossing3(const V3& a, double da, const V3& b, double db) {
    const bool fwd = a.x < b.x || (a.x == b.x && (a.y < b.y || (a.y == b.y && a.z <= b.z)));
    const V3 e = fwd ? a : b, f = fwd ? b : a;
    const double de = fwd ? da : db, df = fwd ? db : da;
    const double t = de / (de - df);
    const V3 w{e.x + t * (f.x - e.x), e.y + t * (f.y - e.y), e.z + t * (f.z - e.z)};
    const double r = sqrt((w.x * w.x + w.y * w.y) + w.z * w.z);
    return V3{w.x / r, w.y / r, w.z / r};
}

template <int S>
OGG_DEV void chain_push(Chain& k, const V3& v) {
    if constexpr (S == 4) {
        k.fan.push(v);
    } else {
        Pass3& s = k.ps[S];
        const double d = measure<S>(k, v);
        const bool in = d >= 0.0;
        V3 x{0.0, 0.0, 0.0};
        int nx = 0;
        if (!s.started) {
            s.started = true, s.f = v, s.fd = d, s.fin = in;
        } else if (in != s.pin) {
            x = crossing3(s.p, s.pd, v, d);
            nx = 1;
        }
        s.p = v, s.pd = d, s.pin = in;
        const int n_out = nx + (in ? 1 : 0);
#pragma unroll 1
        for (int j = 0; j < n_out; ++j) {   // one call site: the chain does not multiply the code
            const bool cr = j == 0 && nx == 1;   // (by component: a choice between two objects would put both in scratch)
            chain_push<S + 1>(k, V3{cr ? x.x : v.x, cr ? x.y : v.y, cr ? x.z : v.z});
        }
    }
}

template <int S>
OGG_DEV void chain_close(Chain& k) {
    if constexpr (S < 4) {
        Pass3& s = k.ps[S];
        if (s.started && s.fin != s.pin) chain_push<S + 1>(k, crossing3(s.p, s.pd, s.f, s.fd));
        chain_close<S + 1>(k);
    }
}

// one lane per candidate: ax[i] = A_x when the pair is kept, else -1; kept[w] the kept pairs of wavefront w
__global__ __launch_bounds__(TT) void clip_kernel(long n, const unsigned long long* __restrict__ keys, const double* __restrict__ trec,
                                                  const double* __restrict__ srec, const double* __restrict__ sq,
                                                  const double* __restrict__ asrc, double Re2, double thr,
                                                  double* __restrict__ ax_out, long long* __restrict__ kept) {
    const long i = (long)blockIdx.x * TT + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const unsigned long long key = keys[i];
        const long c = (long)(key >> 32), q = (long)(key & 0xffffffffull);
        const double* t = trec + c * TNF;
        const double* s = srec + q * BOX_NF;
        V3 P[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) P[v] = V3{t[3 * v], t[3 * v + 1], t[3 * v + 2]};
        Chain k{};
        k.nrm = s, k.q = sq + 12 * q;
        const double ap = t[BOX_NF];
        bool all_in = true;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            all_in = all_in && measure<0>(k, P[v]) >= 0.0 && measure<1>(k, P[v]) >= 0.0 && measure<2>(k, P[v]) >= 0.0 &&
                     measure<3>(k, P[v]) >= 0.0;
        double ax;
        if (all_in) {
            ax = ap;   // every vertex inside every half-space: the clip returns the polygon as it is
        } else {
            // the corners from the record again: a runtime index into P would put P in scratch
#pragma unroll 1
            for (int v = 0; v < 4; ++v) chain_push<0>(k, V3{t[3 * v], t[3 * v + 1], t[3 * v + 2]});
            chain_close<0>(k);
            ax = k.fan.n >= 3 ? Re2 * k.fan.s : 0.0;
        }
        keep = ax > 0.0 && ax > thr * fmin(ap, asrc[q]);
        ax_out[i] = keep ? ax : -1.0;
    }
    const unsigned long long bal = __ballot(keep);
    if (threadIdx.x == 0) kept[blockIdx.x] = __popcll(bal);
}

// ---- write ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT) void write_kernel(long n, const unsigned long long* __restrict__ keys, const double* __restrict__ ax,
                                                   const long long* __restrict__ wave_off, long nxo, long m0, long NA,
                                                   int* __restrict__ src_ij, int* __restrict__ ocn_ij, double* __restrict__ area) {
    const long i = (long)blockIdx.x * TT + threadIdx.x;
    const double a = i < n ? ax[i] : -1.0;
    const bool keep = a > 0.0;
    const unsigned long long bal = __ballot(keep);
    if (keep) {
        const long long pos = wave_off[blockIdx.x] + __popcll(bal & ((1ull << threadIdx.x) - 1ull));
        const unsigned long long key = keys[i];
        const long c = (long)(key >> 32), q = (long)(key & 0xffffffffull);
        const long mr = c / nxo, J = q / NA;
        src_ij[2 * pos] = (int)(q - J * NA), src_ij[2 * pos + 1] = (int)J;
        ocn_ij[2 * pos] = (int)(c - mr * nxo), ocn_ij[2 * pos + 1] = (int)(m0 + mr);
        area[pos] = a;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_src(const ogg_xgrid_curv_src* s) {
    OGG_REQUIRE(s, OGG_EARG, "curvilinear exchange grid: null source");
    OGG_REQUIRE(s->NA >= 1 && s->NB >= 1 && s->NA <= (long)INT_MAX && s->NB <= (long)INT_MAX &&
                    s->NA * s->NB < (1L << 31) / OGG_LOCATE_MAX_TOUCH,
                OGG_EARG, "curvilinear exchange grid: %ld x %ld source cells: NA, NB >= 1 and NA * NB * %d < 2^31", s->NB, s->NA,
                OGG_LOCATE_MAX_TOUCH);
    OGG_REQUIRE(s->ld >= s->NA + 1, OGG_EARG, "curvilinear exchange grid: row stride %ld < NA + 1", s->ld);
    return OGG_OK;
}

// sets workspace: head | source records | the oriented source corners | A_src | index (cube counts, cube starts, entries, large list) | block sums | model cell
// records | candidates per model cell | their offsets
struct SetsLayout {
    long srec, sq, asrc, bsum, trec, tcnt, toff, total;
    BoxIndexLayout ix;
};

SetsLayout sets_layout(const ogg_xgrid_band& b, const ogg_xgrid_curv_src& s) {
    SetsLayout l;
    const long nq = s.NA * s.NB, nc = out_rows(b) * (b.nx / 2);
    ogg::Sections sec{BOX_HEAD};
    l.srec = sec.take(nq * BOX_NF * 8);
    l.sq = sec.take(nq * 12 * 8);
    l.asrc = sec.take(nq * 8);
    l.ix = box_index_sections(sec, nq);
    l.bsum = sec.take((std::max(BOX_NBMAX + 1, nc + 1) / SCAN_CH + 2) * 8);
    l.trec = sec.take(nc * TNF * 8);
    l.tcnt = sec.take((nc + 1) * 4);
    l.toff = sec.take((nc + 1) * 4);
    l.total = sec.off;
    return l;
}

// pair workspace: keys | keys (the other buffer of the sort) | A_x | kept per wavefront | their offsets
struct PairLayout {
    long key0, key1, ax, kept, off, total;
};

PairLayout pair_layout(long n) {
    PairLayout l;
    const long nw = (n + TT - 1) / TT;
    ogg::Sections sec{0};
    l.key0 = sec.take(n * 8);
    l.key1 = sec.take(n * 8);
    l.ax = sec.take(n * 8);
    l.kept = sec.take(nw * 8);
    l.off = sec.take(nw * 8);
    l.total = std::max(sec.off, 256L);
    return l;
}

int check_candidates(long n) {
    OGG_REQUIRE(n >= 0 && n < (1L << 31), OGG_EARG, "curvilinear exchange grid: %ld candidates: 0 <= candidates < 2^31", n);
    return OGG_OK;
}

int check_band_src(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src) {
    OGG_REQUIRE(band && src, OGG_EARG, "ogg_xgrid_curv: null pointer");
    if (int e = check_band(*band)) return e;
    return check_src(src);
}

}  // namespace

extern "C" int ogg_xgrid_curv_check(const ogg_xgrid_curv_src* src) { return check_src(src); }

extern "C" long ogg_xgrid_curv_workspace_bytes(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, long candidates) {
    if (!band || !src || check_band(*band) != OGG_OK || check_src(src) != OGG_OK) return -1;
    if (candidates < 0) return sets_layout(*band, *src).total;
    if (candidates >= (1L << 31)) return -1;
    return pair_layout(candidates).total;
}

extern "C" int ogg_xgrid_curv_sets_dev(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, void* workspace, long workspace_bytes,
                                       double* a_poly, double* a_src, ogg_xgrid_curv_counts* counts, void* stream) {
    if (int e = check_band_src(band, src)) return e;
    const SetsLayout l = sets_layout(*band, *src);
    if (int e = ogg::check_workspace("ogg_xgrid_curv_sets", workspace, workspace_bytes, l.total)) return e;
    const Geo g = make_geo(*band);
    OGG_REQUIRE(src->x && src->y && a_src && counts, OGG_EARG, "ogg_xgrid_curv_sets: null source x / y / a_src / counts");
    if (g.ncells > 0)
        OGG_REQUIRE(band->x && band->y && band->x_next && band->y_next && a_poly, OGG_EARG,
                    "ogg_xgrid_curv_sets: null x / y / x_next / y_next / a_poly");
    int brute, cubes;
    // OGG_XGRID_CURV_BRUTE=1: every valid source cell is tested against every model cell (the cross-check of the index)
    if (int e = knob("OGG_XGRID_CURV_BRUTE", 0, 0, 1, &brute)) return e;
    // OGG_XGRID_CURV_CUBES: cubes per axis of the index; 0: from the number of source cells, about eight cells across a cube
    if (int e = knob("OGG_XGRID_CURV_CUBES", 0, 0, OGG_LOCATE_MAX_CUBES, &cubes)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const long nq = src->NA * src->NB;
    const int G = brute ? 1 : (cubes > 0 ? cubes : box_default_cubes(nq));
    double* srec = at<double>(workspace, l.srec);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_xgrid_curv_counts), st));
    const SrcD sd{src->x, src->y, src->mask, src->NA, src->NB, src->ld};
    src_record_kernel<<<grid_for<NT>(nq, 4096), NT, 0, st>>>(sd, g.Re2, srec, at<double>(workspace, l.sq), at<double>(workspace, l.asrc), a_src,
                                                             counts);
    OGG_LAUNCH_CHECK();
    BoxHead* head = at<BoxHead>(workspace, 0);
    if (int e = build_box_index(nq, srec, G, brute, head, MAGIC, workspace, l.ix, at<long long>(workspace, l.bsum), &counts->src_large,
                                at<long long>(workspace, CUBES_WORD), st))
        return e;
    if (g.ncells == 0) return OGG_OK;
    double* trec = at<double>(workspace, l.trec);
    tgt_record_kernel<<<grid_for<NT>(g.ncells, 4096), NT, 0, st>>>(g, trec, a_poly, counts);
    OGG_LAUNCH_CHECK();
    const Index ix{srec, head, at<int>(workspace, l.ix.start), at<int>(workspace, l.ix.entries), at<int>(workspace, l.ix.large)};
    int* tcnt = at<int>(workspace, l.tcnt);
    pair_kernel<false><<<grid_for<NT>(g.ncells, 1L << 20), NT, 0, st>>>(g.ncells, trec, ix, tcnt, nullptr, nullptr);
    OGG_LAUNCH_CHECK();
    return exclusive_scan<false>(tcnt, g.ncells, at<long long>(workspace, l.bsum), &counts->candidates, at<int>(workspace, l.toff), st);
}

extern "C" int ogg_xgrid_curv_clip_dev(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, const void* workspace,
                                       long workspace_bytes, long candidates, void* pair_workspace, long pair_workspace_bytes,
                                       ogg_xgrid_curv_counts* counts, void* stream) {
    if (int e = check_band_src(band, src)) return e;
    if (int e = check_candidates(candidates)) return e;
    const SetsLayout l = sets_layout(*band, *src);
    const PairLayout p = pair_layout(candidates);
    if (int e = ogg::check_workspace("ogg_xgrid_curv_clip", workspace, workspace_bytes, l.total)) return e;
    if (int e = ogg::check_workspace("ogg_xgrid_curv_clip (pairs)", pair_workspace, pair_workspace_bytes, p.total)) return e;
    OGG_REQUIRE(counts, OGG_EARG, "ogg_xgrid_curv_clip: null counts");
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(&counts->kept, 0, sizeof(long long), st));
    const Geo g = make_geo(*band);
    if (candidates == 0 || g.ncells == 0) return OGG_OK;
    const double *srec = at<double>(workspace, l.srec), *trec = at<double>(workspace, l.trec);
    const Index ix{srec, at<BoxHead>(workspace, 0), at<int>(workspace, l.ix.start), at<int>(workspace, l.ix.entries),
                   at<int>(workspace, l.ix.large)};
    unsigned long long* key[2] = {at<unsigned long long>(pair_workspace, p.key0), at<unsigned long long>(pair_workspace, p.key1)};
    pair_kernel<true><<<grid_for<NT>(g.ncells, 1L << 20), NT, 0, st>>>(g.ncells, trec, ix, nullptr, at<int>(workspace, l.toff), key[1]);
    OGG_LAUNCH_CHECK();
    key_run_kernel<<<(unsigned)((candidates + KEYSORT_NT - 1) / KEYSORT_NT), KEYSORT_NT, 0, st>>>(key[1], candidates, key[0]);
    OGG_LAUNCH_CHECK();
    int k = 0;
    for (long w = KEYSORT_NT; w < candidates; w *= 2, ++k) {
        keysort_merge_kernel<<<grid_for<NT>(candidates, 1L << 20), KEYSORT_NT, 0, st>>>(key[k & 1], candidates, w, key[(k + 1) & 1]);
        OGG_LAUNCH_CHECK();
    }
    const long nw = (candidates + TT - 1) / TT;
    long long* kept = at<long long>(pair_workspace, p.kept);
    clip_kernel<<<(unsigned)nw, TT, 0, st>>>(candidates, key[k & 1], trec, srec, at<double>(workspace, l.sq), at<double>(workspace, l.asrc),
                                             g.Re2, g.thr,
                                             at<double>(pair_workspace, p.ax), kept);
    OGG_LAUNCH_CHECK();
    xgrid_scan_kernel<<<1, SCAN_T, 0, st>>>(kept, nw, at<long long>(pair_workspace, p.off), &counts->kept);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_xgrid_curv_write_dev(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, long candidates,
                                        const void* pair_workspace, long pair_workspace_bytes, int* src_ij, int* ocn_ij, double* area,
                                        void* stream) {
    if (int e = check_band_src(band, src)) return e;
    if (int e = check_candidates(candidates)) return e;
    const PairLayout p = pair_layout(candidates);
    if (int e = ogg::check_workspace("ogg_xgrid_curv_write", pair_workspace, pair_workspace_bytes, p.total)) return e;
    const Geo g = make_geo(*band);
    if (candidates == 0 || g.ncells == 0) return OGG_OK;
    OGG_REQUIRE(src_ij && ocn_ij && area, OGG_EARG, "ogg_xgrid_curv_write: null src_ij / ocn_ij / area");
    const unsigned long long* keys = at<unsigned long long>(pair_workspace, keysort_passes(candidates) & 1 ? p.key1 : p.key0);
    write_kernel<<<(unsigned)((candidates + TT - 1) / TT), TT, 0, ogg::as_stream(stream)>>>(
        candidates, keys, at<double>(pair_workspace, p.ax), at<long long>(pair_workspace, p.off), g.nxo, g.m0, src->NA, src_ij, ocn_ij, area);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: rows, masks and corners copied to device memory, the three steps, the results copied back (synchronous)
extern "C" int ogg_xgrid_curv(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, long capacity, int* src_ij, int* ocn_ij,
                              double* area, double* a_poly, double* a_src, ogg_xgrid_curv_counts* counts) {
    if (int e = check_band_src(band, src)) return e;
    OGG_REQUIRE(counts && src->x && src->y && a_src, OGG_EARG, "ogg_xgrid_curv: null counts / source x / y / a_src");
    const ogg_xgrid_band& h = *band;
    const long rows = out_rows(h), nc = rows * (h.nx / 2), nq = src->NA * src->NB;
    *counts = ogg_xgrid_curv_counts{};
    if (rows > 0) OGG_REQUIRE(h.x && h.y && a_poly, OGG_EARG, "ogg_xgrid_curv: null x / y / a_poly");
    ogg::Buffers bufs;   // freed on every exit path
    double *sx, *sy, *ap, *as, *la;
    char *ws, *pw;
    int *li, *lo;
    ogg_xgrid_curv_counts* ct;
    ogg_xgrid_band d = h;
    if (rows > 0)
        if (int e = stage_band(bufs, h, &d)) return e;
    const size_t npt = (size_t)(src->NB + 1) * (size_t)src->ld - (size_t)(src->ld - src->NA - 1);   // the last row ends at its last corner
    if (int e = bufs.put(&sx, src->x, npt)) return e;
    if (int e = bufs.put(&sy, src->y, npt)) return e;
    ogg_xgrid_curv_src ds = *src;
    ds.x = sx, ds.y = sy;
    if (src->mask) {
        unsigned char* pm;
        if (int e = bufs.put(&pm, src->mask, (size_t)nq)) return e;
        ds.mask = pm;
    }
    const long wsb = sets_layout(d, ds).total;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&ap, (size_t)nc)) return e;
    if (int e = bufs.alloc(&as, (size_t)nq)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = ogg_xgrid_curv_sets_dev(&d, &ds, ws, wsb, ap, as, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(a_src, as, (size_t)nq)) return e;
    if (nc > 0)
        if (int e = bufs.get(a_poly, ap, (size_t)nc)) return e;
    const long cand = (long)counts->candidates;
    if (cand == 0) return OGG_OK;
    if (int e = check_candidates(cand)) return e;
    const long pwb = pair_layout(cand).total;
    if (int e = bufs.alloc(&pw, (size_t)pwb)) return e;
    if (int e = ogg_xgrid_curv_clip_dev(&d, &ds, ws, wsb, cand, pw, pwb, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    const long long kept = counts->kept;
    OGG_REQUIRE(kept <= capacity, OGG_ESHAPE, "ogg_xgrid_curv: %lld exchange cells, capacity %ld", kept, capacity);
    if (kept == 0) return OGG_OK;
    OGG_REQUIRE(src_ij && ocn_ij && area, OGG_EARG, "ogg_xgrid_curv: null src_ij / ocn_ij / area");
    if (int e = bufs.alloc(&li, (size_t)kept * 2)) return e;
    if (int e = bufs.alloc(&lo, (size_t)kept * 2)) return e;
    if (int e = bufs.alloc(&la, (size_t)kept)) return e;
    if (int e = ogg_xgrid_curv_write_dev(&d, &ds, cand, pw, pwb, li, lo, la, nullptr)) return e;
    if (int e = bufs.get(src_ij, li, (size_t)kept * 2)) return e;
    if (int e = bufs.get(ocn_ij, lo, (size_t)kept * 2)) return e;
    if (int e = bufs.get(area, la, (size_t)kept)) return e;
    return OGG_OK;
}
