// What the exchange-grid kernels share (ogg_xgrid.hip: a lat-lon atmosphere; ogg_xgrid_cs.hip: a cubed sphere): the band of model cells
// and its staging, the axis-aligned Sutherland-Hodgman chain of include/ogg_hip.h ("clip"), the binary search, the wavefront sum and the
// scan of the kept pairs per wavefront.  The chain is templated on what its last pass feeds: a type with push(l, p), the vertex's two
// coordinates in the plane the clip works in ((lambda, phi) in degrees there, the face's gnomonic (xi, eta) here).
#pragma once
#include <algorithm>
#include <cmath>

#include "ogg_common.h"
#include "ogg_math.h"

#pragma clang fp contract(off)

namespace ogg {
namespace xg {

constexpr int TT = 64;                    // threads per workgroup: one wavefront
constexpr int SCAN_T = 1024;
constexpr double D2R = 3.14159265358979323846 / 180.0;
constexpr long WS_HEAD = 64;              // a workspace starts with the total of the kept pairs (int64)

struct Geo {
    const double *x, *y, *xn, *yn;
    const unsigned char* mask;
    long nxp, nxo, j0, n, m0, ncells;
    double Re2, thr;
};

// x mod 360 with numpy's % semantics (as ogg_topog.hip)
OGG_DEV double mod360(double x) {
    double m = fmod(x, 360.0);
    if (m != 0.0) {
        if (m < 0.0) m += 360.0;
    } else {
        m = 0.0;
    }
    return m;
}

// first k in [lo, hi) with pred(k) (pred false .. true over the range), hi when none
template <typename P>
OGG_DEV long lower_bound(long lo, long hi, P pred) {
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (pred(mid))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// Sutherland-Hodgman against S: 0 lam >= c, 1 lam <= c, 2 phi >= c, 3 phi <= c, the four passes chained: every vertex a pass emits
// goes straight into the next pass, and the last pass's into the accumulator, all in registers.  A pass emits its first vertex when
// inside, then for each edge (v_k, v_k+1) its crossing (ends on two sides) and v_k+1 when inside; the closing edge gives its crossing only.
template <int S>
OGG_DEV bool inside(double l, double p, double c) {
    return S == 0 ? l >= c : (S == 1 ? l <= c : (S == 2 ? p >= c : p <= c));
}

template <int S>
OGG_DEV void crossing(double al, double ap, double bl, double bp, double c, double& ol, double& op) {
    if (S < 2) {   // the edge's ends in canonical order (lam, phi)
        const bool fwd = al < bl || (al == bl && ap <= bp);
        const double le = fwd ? al : bl, pe = fwd ? ap : bp, lf = fwd ? bl : al, pf = fwd ? bp : ap;
        ol = c, op = pe + (c - le) * ((pf - pe) / (lf - le));
    } else {       // (phi, lam)
        const bool fwd = ap < bp || (ap == bp && al <= bl);
        const double le = fwd ? al : bl, pe = fwd ? ap : bp, lf = fwd ? bl : al, pf = fwd ? bp : ap;
        ol = le + (c - pe) * ((lf - le) / (pf - pe)), op = c;
    }
}

struct Pass {
    double fl, fp, pl, pp;
    bool started, fin, pin;
};

template <typename Acc>
struct Clip {
    Pass ps[4];
    double c[4];
    Acc acc;
};

template <int S, typename Acc>
OGG_DEV void clip_push(Clip<Acc>& k, double l, double p) {
    if constexpr (S == 4) {
        k.acc.push(l, p);
    } else {
        Pass& s = k.ps[S];
        const bool in = inside<S>(l, p, k.c[S]);
        double xl = 0.0, xp = 0.0;
        int nx = 0;
        if (!s.started) {
            s.started = true, s.fl = l, s.fp = p, s.fin = in;
        } else if (in != s.pin) {
            crossing<S>(s.pl, s.pp, l, p, k.c[S], xl, xp);
            nx = 1;
        }
        s.pl = l, s.pp = p, s.pin = in;
        const int n_out = nx + (in ? 1 : 0);
#pragma unroll 1
        for (int j = 0; j < n_out; ++j) {   // one call site: the chain does not multiply the code
            const bool x = j == 0 && nx == 1;
            clip_push<S + 1>(k, x ? xl : l, x ? xp : p);
        }
    }
}

template <int S, typename Acc>
OGG_DEV void clip_close(Clip<Acc>& k) {
    if constexpr (S < 4) {
        Pass& s = k.ps[S];
        if (s.started && s.fin != s.pin) {
            double xl, xp;
            crossing<S>(s.pl, s.pp, s.fl, s.fp, k.c[S], xl, xp);
            clip_push<S + 1>(k, xl, xp);
        }
        clip_close<S + 1>(k);
    }
}

OGG_DEV const double* row_of(const double* p, const double* pn, const Geo& g, long r) {
    return r < g.n ? p + r * g.nxp : pn + (r - g.n) * g.nxp;
}

// the corners C0 .. C3 of model cell c of the band (row-major over its model rows)
OGG_DEV void cell_corners(const Geo& g, long c, double cx[4], double cy[4]) {
    const long mr = c / g.nxo, n = c - mr * g.nxo;
    const long r0 = 2 * (g.m0 + mr) - g.j0;
    const double *x0 = row_of(g.x, g.xn, g, r0), *y0 = row_of(g.y, g.yn, g, r0);
    const double *x2 = row_of(g.x, g.xn, g, r0 + 2), *y2 = row_of(g.y, g.yn, g, r0 + 2);
    cx[0] = x0[2 * n], cx[1] = x0[2 * n + 2], cx[2] = x2[2 * n + 2], cx[3] = x2[2 * n];
    cy[0] = y0[2 * n], cy[1] = y0[2 * n + 2], cy[2] = y2[2 * n + 2], cy[3] = y2[2 * n];
}

template <typename T>
OGG_DEV T wave_sum(T v) {
    for (int o = TT / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, TT);
    return v;
}

// inclusive scan of one value per lane over the wavefront
OGG_DEV long long wave_scan(long long v, int lane) {
    for (int o = 1; o < TT; o <<= 1) {
        const long long u = __shfl_up(v, o, TT);
        if (lane >= o) v += u;
    }
    return v;
}

// the first of the wavefront's 64 cells whose inclusive candidate count exceeds t
OGG_DEV int owner_of(const long long* incl, long long t) {
    int lo = 0, hi = TT;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (incl[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

OGG_DEV void count_add(long long* p, long long v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// exclusive offsets of the kept pairs of every wavefront, and their total: one workgroup, contiguous chunks per thread
static __global__ __launch_bounds__(SCAN_T) void xgrid_scan_kernel(const long long* in, long n, long long* out, long long* total) {
    __shared__ long long part[SCAN_T];
    const int t = threadIdx.x;
    const long chunk = (n + SCAN_T - 1) / SCAN_T;
    const long lo = t * chunk, hi = std::min(n, lo + chunk);
    long long s = 0;
    for (long i = lo; i < hi; ++i) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {
        const long long v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long r = t ? part[t - 1] : 0;
    for (long i = lo; i < hi; ++i) {
        out[i] = r;
        r += in[i];
    }
    if (t == SCAN_T - 1) *total = part[SCAN_T - 1];
}

// ---- the band (host) -------------------------------------------------------------------------------------------
inline int check_band(const ogg_xgrid_band& b) {
    OGG_REQUIRE(b.nx >= 2 && b.ny >= 2 && b.nx % 2 == 0 && b.ny % 2 == 0, OGG_EARG,
                "exchange grid: model cells are 2 x 2 supergrid cells, but the supergrid has %ld x %ld cells; generate it with "
                "--ensure_nj_even", b.ny, b.nx);
    OGG_REQUIRE(b.j0 >= 0 && b.n_cell_rows >= 0 && b.j0 + b.n_cell_rows <= b.ny, OGG_EARG,
                "ogg_xgrid_band: cell rows %ld .. %ld of a grid of %ld", b.j0, b.j0 + b.n_cell_rows - 1, b.ny);
    OGG_REQUIRE(b.Re > 0.0 && std::isfinite(b.Re), OGG_EARG, "ogg_xgrid_band: Re = %g", b.Re);
    OGG_REQUIRE(b.threshold >= 0.0 && std::isfinite(b.threshold), OGG_EARG, "ogg_xgrid_band: threshold = %g", b.threshold);
    return OGG_OK;
}

inline long first_row(const ogg_xgrid_band& b) { return (b.j0 + 1) / 2; }
inline long end_row(const ogg_xgrid_band& b) { return (b.j0 + b.n_cell_rows + 1) / 2; }
inline long out_rows(const ogg_xgrid_band& b) { return std::max(0L, end_row(b) - first_row(b)); }
inline long next_rows(const ogg_xgrid_band& b) { return out_rows(b) > 0 ? 2 * end_row(b) - (b.j0 + b.n_cell_rows) + 1 : 0; }
inline long n_waves(const ogg_xgrid_band& b) { return (out_rows(b) * (b.nx / 2) + TT - 1) / TT; }

inline Geo make_geo(const ogg_xgrid_band& b) {
    Geo g{b.x, b.y, b.x_next, b.y_next, b.mask, b.nx + 1, b.nx / 2, b.j0, b.n_cell_rows, first_row(b), 0, b.Re * b.Re, b.threshold};
    g.ncells = out_rows(b) * g.nxo;
    return g;
}

// the band of a host-pointer entry in device memory: its rows (x, y hold n_cell_rows + next_rows point rows when x_next is NULL) and
// its mask copied into bufs, *d the band with device pointers
inline int stage_band(Buffers& bufs, const ogg_xgrid_band& h, ogg_xgrid_band* d) {
    const long nxp = h.nx + 1, n = h.n_cell_rows, nn = next_rows(h);
    const size_t body = (size_t)n * nxp, tail = (size_t)nn * nxp;   // doubles
    double *px, *py;
    if (int e = bufs.alloc(&px, body + tail)) return e;
    if (int e = bufs.alloc(&py, body + tail)) return e;
    if (int e = bufs.send(px, h.x, body)) return e;
    if (int e = bufs.send(py, h.y, body)) return e;
    if (int e = bufs.send(px + body, h.x_next ? h.x_next : h.x + n * nxp, tail)) return e;
    if (int e = bufs.send(py + body, h.y_next ? h.y_next : h.y + n * nxp, tail)) return e;
    *d = h;
    d->x = px, d->y = py;
    d->x_next = d->x + n * nxp, d->y_next = d->y + n * nxp;
    if (h.mask) {
        unsigned char* pm;
        if (int e = bufs.put(&pm, h.mask, (size_t)(out_rows(h) * (h.nx / 2)))) return e;
        d->mask = pm;
    }
    return OGG_OK;
}

}  // namespace xg
}  // namespace ogg
