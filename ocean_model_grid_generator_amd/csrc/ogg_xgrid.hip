// Atmosphere x ocean exchange grid (include/ogg_hip.h, "Atmosphere x ocean exchange grid"): every non-empty overlap of a
// rectilinear atmosphere cell with a MOM6 h-cell of the stitched supergrid, with its area.
//
// xgrid_kernel<WRITE>: one wavefront per workgroup, one wavefront per 64 consecutive model cells (row-major).  Each lane sets up
// its own cell (unwrapped corners, pole substitution, winding test, A_poly, bounding box, the range of candidate rows J and
// unrolled columns u = k NA + I by binary search) and leaves the polygon in LDS.  The wavefront then walks the flattened
// (cell, candidate) pairs of its 64 cells, lane l taking pairs l, l + 64, ...: a polar cell with hundreds of candidates is spread
// over all lanes instead of holding up one, and the common cell with one to four candidates leaves no lane idle.  A pair whose
// atmosphere cell contains the whole polygon takes A_poly (the clip would return the polygon unchanged); the others are clipped
// (Sutherland-Hodgman, the four passes chained vertex by vertex in registers into the area) and their area evaluated.  The keep flags are counted with a ballot.
// Count step (WRITE = false): A_poly, the counts (integer atomics), the kept pairs per wavefront; xgrid_scan_kernel turns those
// into offsets.  Write step (WRITE = true): the same pairs again, each kept one written at its wavefront's offset plus the kept
// pairs before it in the wavefront's order -- the list is in cell-major, candidate order whatever the launch geometry.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ogg_clip.h"

#pragma clang fp contract(off)

namespace {

using namespace ogg::xg;

constexpr int PV = 6;                     // polygon vertices at most: two runs of one pole corner

enum { ST_OK = 0, ST_DEGENERATE = 1, ST_POLE = 2, ST_INVERTED = 3 };

struct AtmD {
    const double *a, *b, *dsin;
    long NA, NB;
};

OGG_DEV double wrap180(double d) { return mod360(d + 180.0) - 180.0; }

OGG_DEV long floor_div(long u, long n) { return u >= 0 ? u / n : -((-u + n - 1) / n); }

// E(h) = 1 - sin(h) / h
OGG_DEV double efun(double h) {
    if (fabs(h) < 0.1) {
        const double h2 = h * h;
        return h2 * (1.0 / 6.0 - h2 * (1.0 / 120.0 - h2 * (1.0 / 5040.0 - h2 / 362880.0)));
    }
    return 1.0 - sin(h) / h;
}

// the mean of sin(phi) - sin(pr) along an edge straight in (lambda, phi), radians.  h == 0 (an edge along a parallel) skips sin(pm):
// E(0) = 0, and the term it multiplies cannot change the difference
OGG_DEV double gfun(double p1, double p2, double pr) {
    const double pm = (p1 + p2) / 2.0, h = (p2 - p1) / 2.0;
    const double a = 2.0 * cos((pm + pr) / 2.0) * sin((pm - pr) / 2.0);
    return h == 0.0 ? a : a - sin(pm) * efun(h);
}

// A of a polygon in degrees, its vertices pushed one by one (so the clip below feeds it without storing a vertex list).  An edge
// along a meridian (dlam == 0) adds an exact zero and is skipped.
struct AreaAcc {
    double l0, p0, lk, pk, s;
    int n;
    OGG_DEV void push(double l, double p) {
        const double ln = l * D2R, pn = p * D2R;
        if (n == 0) {
            l0 = ln, p0 = pn, s = 0.0;
        } else {
            const double dl = ln - lk;
            if (dl != 0.0) s = s + dl * gfun(pk, pn, p0);
        }
        lk = ln, pk = pn, ++n;
    }
};

OGG_DEV double area_close(AreaAcc& a, double Re2) {
    if (a.n == 0) return 0.0;
    const double dl = a.l0 - a.lk;
    if (dl != 0.0) a.s = a.s + dl * gfun(a.pk, a.p0, a.p0);
    return -Re2 * a.s;
}

OGG_DEV double col_edge(const AtmD& a, long u, int hi) {
    const long k = floor_div(u, a.NA);
    return a.a[u - k * a.NA + hi] + 360.0 * (double)k;
}

template <bool WRITE>
__global__ __launch_bounds__(TT) void xgrid_kernel(Geo g, AtmD a, double* a_poly, ogg_xgrid_counts* counts, long long* wave_kept,
                                                   const long long* wave_off, const long long* total, int* atm_ij, int* ocn_ij,
                                                   double* area) {
    __shared__ double vl[PV][TT], vp[PV][TT];
    __shared__ double s_apoly[TT], s_box[4][TT];
    __shared__ long long s_incl[TT];
    __shared__ int s_nv[TT], s_jlo[TT], s_ncol[TT], s_ulo[TT];
    const int lane = threadIdx.x;
    const long w = blockIdx.x;
    const long c = w * TT + lane;
    const bool live = c < g.ncells;
    long long cnt = 0;
    int st = ST_DEGENERATE, npole = 0, masked = 0;
    if (live) {
        double cx[4], cy[4];
        cell_corners(g, c, cx, cy);
        masked = g.mask ? (g.mask[c] == 0) : 0;
        bool pc[4];
        double L[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pc[k] = fabs(cy[k]) >= 90.0 - OGG_TOPOG_POLE_EPS;
            npole += pc[k] ? 1 : 0;
            L[k] = cx[0] + wrap180(cx[k] - cx[0]);
        }
        double A = NAN;
        if (npole < 3) {
            int nv = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!pc[k]) {
                    vl[nv][lane] = L[k], vp[nv][lane] = cy[k], ++nv;
                } else if (!pc[(k + 3) & 3]) {   // a run of pole corners starts here
                    const double lb = L[(k + 3) & 3], la = pc[(k + 1) & 3] ? L[(k + 2) & 3] : L[(k + 1) & 3];
                    const double p = cy[k] > 0.0 ? 90.0 : -90.0;
                    vl[nv][lane] = lb, vp[nv][lane] = p, ++nv;
                    vl[nv][lane] = la, vp[nv][lane] = p, ++nv;
                }
            }
            double wsum = 0.0, lmin = vl[0][lane], lmax = lmin, pmin = vp[0][lane], pmax = pmin;
            for (int k = 0; k < nv; ++k) {
                const double l = vl[k][lane], p = vp[k][lane];
                wsum = wsum + wrap180(vl[k + 1 < nv ? k + 1 : 0][lane] - l);
                lmin = fmin(lmin, l), lmax = fmax(lmax, l), pmin = fmin(pmin, p), pmax = fmax(pmax, p);
            }
            if (fabs(wsum) > 180.0) {
                st = ST_POLE;
            } else {
                AreaAcc acc{};
                for (int k = 0; k < nv; ++k) acc.push(vl[k][lane], vp[k][lane]);
                A = area_close(acc, g.Re2);
                st = A > 0.0 ? ST_OK : ST_INVERTED;
            }
            s_nv[lane] = nv;
            s_box[0][lane] = lmin, s_box[1][lane] = lmax, s_box[2][lane] = pmin, s_box[3][lane] = pmax;
            if (st == ST_OK && !masked) {
                const long jlo = lower_bound(0, a.NB, [&](long J) { return a.b[J + 1] > pmin; });
                const long jhi = lower_bound(0, a.NB, [&](long J) { return a.b[J] >= pmax; });
                const double kd = floor((lmin - a.a[0]) / 360.0);
                const long kf = fabs(kd) < 1.0e6 ? (long)kd : 0;   // (a longitude beyond 3.6e8 degrees finds no column)
                const long U0 = (kf - 2) * a.NA, U1 = (kf + 3) * a.NA;
                const long ulo = lower_bound(U0, U1, [&](long u) { return col_edge(a, u, 1) > lmin; });
                const long uhi = lower_bound(U0, U1, [&](long u) { return col_edge(a, u, 0) >= lmax; });
                const long nj = jhi > jlo ? jhi - jlo : 0, nc = uhi > ulo ? uhi - ulo : 0;
                cnt = (long long)nj * nc;
                s_jlo[lane] = (int)jlo, s_ulo[lane] = (int)ulo, s_ncol[lane] = (int)nc;
            }
        }
        s_apoly[lane] = A;
        if (!WRITE) a_poly[c] = A;
    }
    // inclusive scan of the candidate counts over the wavefront
    const long long incl = wave_scan(cnt, lane);
    s_incl[lane] = incl;
    const long long T = __shfl(incl, TT - 1, TT);
    __syncthreads();
    long long run = 0, base = 0, limit = 0;
    if (WRITE) base = wave_off[w], limit = *total;
    for (long long t0 = 0; t0 < T; t0 += TT) {
        const long long t = t0 + lane;
        bool keep = false;
        int I = 0, J = 0, o = 0;
        double ax = 0.0;
        if (t < T) {
            o = owner_of(s_incl, t);
            const long long q = t - (o ? s_incl[o - 1] : 0);
            const int nc = s_ncol[o];
            J = s_jlo[o] + (int)(q / nc);
            const long u = (long)s_ulo[o] + (long)(q % nc);
            const long k = floor_div(u, a.NA);
            I = (int)(u - k * a.NA);
            const double sh = 360.0 * (double)k;
            const double clo = a.a[I] + sh, chi = a.a[I + 1] + sh, blo = a.b[J], bhi = a.b[J + 1];
            const double ap = s_apoly[o];
            if (s_box[0][o] >= clo && s_box[1][o] <= chi && s_box[2][o] >= blo && s_box[3][o] <= bhi) {
                ax = ap;   // every vertex inside every half-plane: the clip returns the polygon as it is
            } else {
                Clip<AreaAcc> k{};
                k.c[0] = clo, k.c[1] = chi, k.c[2] = blo, k.c[3] = bhi;
                const int nv = s_nv[o];
                for (int v = 0; v < nv; ++v) clip_push<0>(k, vl[v][o], vp[v][o]);
                clip_close<0>(k);
                ax = area_close(k.acc, g.Re2);
            }
            const double aatm = g.Re2 * (a.a[I + 1] * D2R - a.a[I] * D2R) * a.dsin[J];
            keep = ax > 0.0 && ax > g.thr * fmin(ap, aatm);
        }
        const unsigned long long bal = __ballot(keep);
        if (WRITE && keep) {
            const long long pos = base + run + __popcll(bal & ((1ull << lane) - 1ull));
            if (pos < limit) {
                const long cc = w * TT + o, mr = cc / g.nxo;
                atm_ij[2 * pos] = I, atm_ij[2 * pos + 1] = J;
                ocn_ij[2 * pos] = (int)(cc - mr * g.nxo), ocn_ij[2 * pos + 1] = (int)(g.m0 + mr);
                area[pos] = ax;
            }
        }
        run += __popcll(bal);
    }
    if (!WRITE) {
        const int n_live = wave_sum(live ? 1 : 0);
        const int n_pole = wave_sum(live && npole > 0 && npole < 3 ? 1 : 0);
        const int n_deg = wave_sum(live && npole >= 3 ? 1 : 0);
        const int n_enc = wave_sum(live && st == ST_POLE ? 1 : 0);
        const int n_inv = wave_sum(live && st == ST_INVERTED ? 1 : 0);
        const int n_mask = wave_sum(live && masked ? 1 : 0);
        const long long n_cand = wave_sum(cnt);
        if (lane == 0) {
            count_add(&counts->cells, n_live), count_add(&counts->pole_cells, n_pole), count_add(&counts->degenerate, n_deg);
            count_add(&counts->pole_enclosing, n_enc), count_add(&counts->inverted, n_inv), count_add(&counts->masked, n_mask);
            count_add(&counts->candidates, n_cand), count_add(&counts->kept, run);
            wave_kept[w] = run;
        }
    }
}

// sin(b_J+1) - sin(b_J) without cancellation: 2 cos((b_J + b_J+1) / 2) sin((b_J+1 - b_J) / 2), radians
__global__ void xgrid_dsin_kernel(const double* b, long n, double* out) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) {
        const double b1 = b[k] * D2R, b2 = b[k + 1] * D2R;
        out[k] = 2.0 * cos((b1 + b2) / 2.0) * sin((b2 - b1) / 2.0);
    }
}

int check_atm_shape(const ogg_xgrid_atm& a) {
    OGG_REQUIRE(a.lon && a.lat, OGG_EARG, "exchange grid: null atmosphere edges");
    OGG_REQUIRE(a.NA >= 1 && a.NB >= 1 && a.NA < (1L << 28) && a.NB < (1L << 28), OGG_EARG, "exchange grid: %ld x %ld atmosphere cells",
                a.NB, a.NA);
    return OGG_OK;
}

int check_atm_host(const ogg_xgrid_atm& a) {
    if (int e = check_atm_shape(a)) return e;
    for (long k = 0; k <= a.NA; ++k)
        OGG_REQUIRE(std::isfinite(a.lon[k]) && (k == 0 || a.lon[k] > a.lon[k - 1]), OGG_EARG,
                    "exchange grid: atmosphere lon edges must increase strictly (edge %ld)", k);
    OGG_REQUIRE(fabs(a.lon[a.NA] - a.lon[0] - 360.0) <= 1e-9, OGG_EARG,
                "exchange grid: atmosphere lon edges must span 360 degrees (they span %.17g)", a.lon[a.NA] - a.lon[0]);
    for (long k = 0; k <= a.NB; ++k)
        OGG_REQUIRE(std::isfinite(a.lat[k]) && (k == 0 || a.lat[k] > a.lat[k - 1]), OGG_EARG,
                    "exchange grid: atmosphere lat edges must increase strictly (edge %ld)", k);
    OGG_REQUIRE(a.lat[0] >= -90.0 && a.lat[a.NB] <= 90.0, OGG_EARG, "exchange grid: atmosphere lat edges %g .. %g leave [-90, 90]",
                a.lat[0], a.lat[a.NB]);
    return OGG_OK;
}

// workspace: head (the total) | dsin (NB + 1 doubles) | kept per wave | offsets per wave; sections rounded to 64 bytes
struct Layout {
    long long* total;
    double* dsin;
    long long *kept, *off;
};

struct Offsets {
    long dsin, kept, off, total;
};

Offsets offsets(const ogg_xgrid_band& b, const ogg_xgrid_atm& a) {
    ogg::Sections s{WS_HEAD, 64};
    return Offsets{s.take((a.NB + 1) * 8), s.take(n_waves(b) * 8), s.take(n_waves(b) * 8), s.off};   // evaluated left to right
}

long ws_bytes(const ogg_xgrid_band& b, const ogg_xgrid_atm& a) { return offsets(b, a).total; }

Layout layout(void* ws, const ogg_xgrid_band& b, const ogg_xgrid_atm& a) {
    const Offsets o = offsets(b, a);
    return Layout{ogg::at<long long>(ws, 0), ogg::at<double>(ws, o.dsin), ogg::at<long long>(ws, o.kept), ogg::at<long long>(ws, o.off)};
}

int check_dev_args(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm, const void* workspace, long workspace_bytes) {
    OGG_REQUIRE(band && atm, OGG_EARG, "ogg_xgrid: null pointer");
    if (int e = check_band(*band)) return e;
    if (int e = check_atm_shape(*atm)) return e;
    if (out_rows(*band) > 0)
        OGG_REQUIRE(band->x && band->y && band->x_next && band->y_next, OGG_EARG, "ogg_xgrid_band: null x / y / x_next / y_next");
    return ogg::check_workspace("ogg_xgrid", workspace, workspace_bytes, ws_bytes(*band, *atm));
}

}  // namespace

extern "C" long ogg_xgrid_band_first_row(const ogg_xgrid_band* band) {
    if (!band || band->j0 < 0 || band->n_cell_rows < 0) return -1;
    return first_row(*band);
}

extern "C" long ogg_xgrid_band_out_rows(const ogg_xgrid_band* band) {
    if (!band || band->j0 < 0 || band->n_cell_rows < 0) return -1;
    return out_rows(*band);
}

extern "C" long ogg_xgrid_band_next_rows(const ogg_xgrid_band* band) {
    if (!band || band->j0 < 0 || band->n_cell_rows < 0) return -1;
    return next_rows(*band);
}

extern "C" long ogg_xgrid_workspace_bytes(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm) {
    if (!band || !atm || band->j0 < 0 || band->n_cell_rows < 0 || band->nx < 2 || atm->NB < 1) return -1;
    return ws_bytes(*band, *atm);
}

extern "C" int ogg_xgrid_check_atm(const ogg_xgrid_atm* atm) {
    OGG_REQUIRE(atm, OGG_EARG, "ogg_xgrid_check_atm: null pointer");
    return check_atm_host(*atm);
}

extern "C" int ogg_xgrid_count_dev(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm, void* workspace, long workspace_bytes,
                                   double* a_poly, ogg_xgrid_counts* counts, void* stream) {
    if (int e = check_dev_args(band, atm, workspace, workspace_bytes)) return e;
    OGG_REQUIRE(counts, OGG_EARG, "ogg_xgrid_count: null counts");
    const Geo g = make_geo(*band);
    OGG_REQUIRE(a_poly || g.ncells == 0, OGG_EARG, "ogg_xgrid_count: null a_poly");
    const Layout l = layout(workspace, *band, *atm);
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_xgrid_counts), st));
    OGG_HIP_CHECK(hipMemsetAsync(l.total, 0, sizeof(long long), st));
    if (g.ncells == 0) return OGG_OK;
    const long nb = atm->NB;
    xgrid_dsin_kernel<<<(unsigned)((nb + 255) / 256), 256, 0, st>>>(atm->lat, nb, l.dsin);
    OGG_LAUNCH_CHECK();
    const AtmD a{atm->lon, atm->lat, l.dsin, atm->NA, atm->NB};
    const long nw = n_waves(*band);
    xgrid_kernel<false><<<(unsigned)nw, TT, 0, st>>>(g, a, a_poly, counts, l.kept, nullptr, nullptr, nullptr, nullptr, nullptr);
    OGG_LAUNCH_CHECK();
    xgrid_scan_kernel<<<1, SCAN_T, 0, st>>>(l.kept, nw, l.off, l.total);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_xgrid_write_dev(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm, const void* workspace, long workspace_bytes,
                                   int* atm_ij, int* ocn_ij, double* area, void* stream) {
    if (int e = check_dev_args(band, atm, workspace, workspace_bytes)) return e;
    const Geo g = make_geo(*band);
    if (g.ncells == 0) return OGG_OK;
    OGG_REQUIRE(atm_ij && ocn_ij && area, OGG_EARG, "ogg_xgrid_write: null atm_ij / ocn_ij / area");
    const Layout l = layout(const_cast<void*>(workspace), *band, *atm);
    const AtmD a{atm->lon, atm->lat, l.dsin, atm->NA, atm->NB};
    xgrid_kernel<true><<<(unsigned)n_waves(*band), TT, 0, ogg::as_stream(stream)>>>(g, a, nullptr, nullptr, nullptr, l.off, l.total,
                                                                                      atm_ij, ocn_ij, area);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: rows, mask and edges copied to device memory, both steps, the results copied back (synchronous)
extern "C" int ogg_xgrid(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm, long capacity, int* atm_ij, int* ocn_ij, double* area,
                         double* a_poly, ogg_xgrid_counts* counts) {
    OGG_REQUIRE(band && atm && counts, OGG_EARG, "ogg_xgrid: null pointer");
    if (int e = check_band(*band)) return e;
    if (int e = check_atm_host(*atm)) return e;
    const ogg_xgrid_band& h = *band;
    const long rows = out_rows(h), nxo = h.nx / 2, nc = rows * nxo;
    *counts = ogg_xgrid_counts{};
    if (rows == 0) return OGG_OK;
    OGG_REQUIRE(h.x && h.y && a_poly, OGG_EARG, "ogg_xgrid: null x / y / a_poly");
    ogg::Buffers bufs;   // freed on every exit path
    double *pa, *pb, *ap, *la;
    char* ws;
    int *li, *lo;
    ogg_xgrid_counts* ct;
    ogg_xgrid_band d;
    if (int e = stage_band(bufs, h, &d)) return e;
    if (int e = bufs.alloc(&pa, (size_t)atm->NA + 1)) return e;
    if (int e = bufs.alloc(&pb, (size_t)atm->NB + 1)) return e;
    if (int e = bufs.send(pa, atm->lon, (size_t)atm->NA + 1)) return e;
    if (int e = bufs.send(pb, atm->lat, (size_t)atm->NB + 1)) return e;
    const ogg_xgrid_atm da{pa, pb, atm->NA, atm->NB};
    const long wsb = ws_bytes(d, da);
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&ap, (size_t)nc)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = ogg_xgrid_count_dev(&d, &da, ws, wsb, ap, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(a_poly, ap, (size_t)nc)) return e;
    const long long kept = counts->kept;
    OGG_REQUIRE(kept <= capacity, OGG_ESHAPE, "ogg_xgrid: %lld exchange cells, capacity %ld", kept, capacity);
    if (kept == 0) return OGG_OK;
    OGG_REQUIRE(atm_ij && ocn_ij && area, OGG_EARG, "ogg_xgrid: null atm_ij / ocn_ij / area");
    if (int e = bufs.alloc(&li, (size_t)kept * 2)) return e;
    if (int e = bufs.alloc(&lo, (size_t)kept * 2)) return e;
    if (int e = bufs.alloc(&la, (size_t)kept)) return e;
    if (int e = ogg_xgrid_write_dev(&d, &da, ws, wsb, li, lo, la, nullptr)) return e;
    if (int e = bufs.get(atm_ij, li, (size_t)kept * 2)) return e;
    if (int e = bufs.get(ocn_ij, lo, (size_t)kept * 2)) return e;
    if (int e = bufs.get(area, la, (size_t)kept)) return e;
    return OGG_OK;
}
