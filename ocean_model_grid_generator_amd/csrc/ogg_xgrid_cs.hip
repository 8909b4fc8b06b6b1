// Cubed-sphere atmosphere x ocean exchange grid (include/ogg_hip.h, "Exchange grid with a cubed-sphere atmosphere"): every non-empty
// overlap of a gnomonic cubed-sphere cell with a MOM6 h-cell of the stitched supergrid, with its area.
//
// xgrid_cs_kernel<WRITE> follows xgrid_kernel<WRITE> of ogg_xgrid.hip: one wavefront per workgroup and per 64 consecutive model cells.
// Each lane sets up its own cell (unit vectors of the corners, the DEGENERATE / WIDE / INVERTED tests, A_poly, and for every candidate
// face the gnomonic polygon (xi, eta) with its range of rows and columns by binary search) and leaves the polygons in LDS, one slot
// per candidate face: a pair never projects again (the two fp64 divides per corner are the expensive part).  The wavefront then walks the
// flattened (cell, face, J, I) candidates of its 64 cells, lane l taking pairs l, l + 64, ...  On a face every atmosphere grid line and
// every great-circle edge is straight in (xi, eta), so the clip is the axis-aligned chain of ogg_clip.h; its last pass feeds a fan of
// spherical triangles from the first vertex.  A pair whose atmosphere cell holds the whole polygon takes A_poly.  Count step: A_poly,
// the counts, the kept pairs per wavefront (a ballot); xgrid_scan_kernel turns those into offsets.  Write step: the same pairs again,
// each kept one written at its wavefront's offset plus the kept pairs before it: the list is in cell, face, J, I order whatever the launch.
//
// A cell has at most three candidate faces: the six normals of a checked atmosphere are three opposite pairs (check_frames), a face and
// its opposite have P . e_n of opposite signs, and a candidate needs P . e_n > 0.05 at every corner.  (The test can still admit a face
// the polygon misses; such pairs clip to nothing.)  So three slots per lane hold every polygon: 3 x 8 doubles x 64 lanes = 12 KB, and
// with 4.3 KB of per-slot and per-cell words the workgroup's LDS leaves the registers (two waves per SIMD) as the limit of occupancy.
#include <algorithm>
#include <cmath>

#include "ogg_clip.h"

#pragma clang fp contract(off)

namespace {

using namespace ogg::xg;

constexpr int NF = 6;
constexpr int NS = 3;            // slots: candidate faces of one cell at most (see above)
constexpr double W_MIN = 0.05;   // a candidate face has every corner's P . e_n above this
constexpr double TOL = 1e-12;
constexpr long N_MAX = 4096;

enum { ST_OK = 0, ST_DEGENERATE = 1, ST_WIDE = 2, ST_INVERTED = 3 };

struct Frames {
    double f[NF][9];   // e_u, e_v, e_n of every face
};

struct CsD {
    const double *t, *aatm;
    long N;
};

struct V3 {
    double x, y, z;
};

OGG_DEV double dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// Omega3(a, b, c) = 2 atan2(a . ((b - a) x (c - a)), 1 + a.b + b.c + c.a)
OGG_DEV double omega3(const V3& a, const V3& b, const V3& c) {
    const V3 u{b.x - a.x, b.y - a.y, b.z - a.z}, v{c.x - a.x, c.y - a.y, c.z - a.z};
    const V3 n{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
    return 2.0 * atan2(dot(a, n), 1.0 + dot(a, b) + dot(b, c) + dot(c, a));
}

// a point of the gnomonic plane with r = sqrt(1 + xi^2 + eta^2)
struct G2 {
    double xi, eta, r;
};

OGG_DEV G2 g2(double xi, double eta) { return G2{xi, eta, sqrt(1.0 + xi * xi + eta * eta)}; }

OGG_DEV double dot2(const G2& p, const G2& q) { return (p.xi * q.xi + p.eta * q.eta + 1.0) / (p.r * q.r); }

// Omega2 of the triangle (a, b, c) given d(a, b); *dca takes d(c, a), the next fan triangle's d(a, b)
OGG_DEV double omega2(const G2& a, const G2& b, const G2& c, double dab, double* dca) {
    const double num = ((b.xi - a.xi) * (c.eta - a.eta) - (b.eta - a.eta) * (c.xi - a.xi)) / (a.r * b.r * c.r);
    const double d = dot2(c, a);
    *dca = d;
    return 2.0 * atan2(num, 1.0 + dab + dot2(b, c) + d);
}

// the fan from vertex 0 of a polygon in (xi, eta), its vertices pushed one by one
struct FanAcc {
    G2 v0, vk;
    double d0k, s;
    int n;
    OGG_DEV void push(double xi, double eta) {
        const G2 v = g2(xi, eta);
        if (n == 0) {
            v0 = v, s = 0.0;
        } else if (n == 1) {
            d0k = dot2(v0, v);
        } else {
            double d;
            s = s + omega2(v0, vk, v, d0k, &d);
            d0k = d;
        }
        vk = v, ++n;
    }
};

OGG_DEV double a_atm_of(const double* t, long J, long I, double Re2) {
    const G2 c00 = g2(t[I], t[J]), c10 = g2(t[I + 1], t[J]), c11 = g2(t[I + 1], t[J + 1]), c01 = g2(t[I], t[J + 1]);
    double d1, d2;
    const double o1 = omega2(c00, c10, c11, dot2(c00, c10), &d1);
    const double o2 = omega2(c00, c11, c01, d1, &d2);
    return Re2 * (o1 + o2);
}

// A_atm(J, I) of the N x N cells of one face (the same on every face)
__global__ void xgrid_cs_aatm_kernel(const double* t, long N, double Re2, double* out) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < N * N) {
        const long J = k / N;
        out[k] = a_atm_of(t, J, k - J * N, Re2);
    }
}

template <bool WRITE>
__global__ __launch_bounds__(TT) void xgrid_cs_kernel(Geo g, CsD a, Frames fr, double* a_poly, ogg_xgrid_cs_counts* counts,
                                                      long long* wave_kept, const long long* wave_off, const long long* total,
                                                      int* atm_fij, int* ocn_ij, double* area) {
    __shared__ double pxi[NS][4][TT], peta[NS][4][TT];
    __shared__ double s_apoly[TT];
    __shared__ long long s_incl[TT];
    __shared__ int s_cum[NS][TT];   // candidates of the cell's slots 0 .. s, inclusive
    __shared__ int s_fj[NS][TT], s_ilo[NS][TT], s_ni[NS][TT];   // s_fj: the slot's face (bits 16 ..) and first row (J <= N_MAX < 2^16)
    __shared__ int s_ns[TT];
    const int lane = threadIdx.x;
    const long w = blockIdx.x;
    const long c = w * TT + lane;
    const bool live = c < g.ncells;
    long long cnt = 0;
    int st = ST_DEGENERATE, masked = 0, ns = 0;
    if (live) {
        double cx[4], cy[4];
        cell_corners(g, c, cx, cy);
        masked = g.mask ? (g.mask[c] == 0) : 0;
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) finite = finite && isfinite(cx[k]) && isfinite(cy[k]);
        double A = NAN;
        if (finite) {
            V3 P[4];
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
            if (wide) {
                st = ST_WIDE;
            } else {
                A = g.Re2 * (omega3(P[0], P[1], P[2]) + omega3(P[0], P[2], P[3]));
                st = A > 0.0 ? ST_OK : ST_INVERTED;
            }
            if (st == ST_OK && !masked) {
                int cum = 0;
#pragma unroll 1
                for (int f = 0; f < NF; ++f) {
                    const V3 eu{fr.f[f][0], fr.f[f][1], fr.f[f][2]}, ev{fr.f[f][3], fr.f[f][4], fr.f[f][5]};
                    const V3 en{fr.f[f][6], fr.f[f][7], fr.f[f][8]};
                    double wk[4];
                    bool cand = true;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        wk[k] = dot(P[k], en);
                        cand = cand && wk[k] > W_MIN;
                    }
                    if (!cand) continue;
                    if (ns == NS) break;   // (never: at most NS faces pass the test)
                    double xmin = 0.0, xmax = 0.0, emin = 0.0, emax = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double xi = dot(P[k], eu) / wk[k], eta = dot(P[k], ev) / wk[k];
                        pxi[ns][k][lane] = xi, peta[ns][k][lane] = eta;
                        xmin = k ? fmin(xmin, xi) : xi, xmax = k ? fmax(xmax, xi) : xi;
                        emin = k ? fmin(emin, eta) : eta, emax = k ? fmax(emax, eta) : eta;
                    }
                    const long jlo = lower_bound(0, a.N, [&](long J) { return a.t[J + 1] > emin; });
                    const long jhi = lower_bound(0, a.N, [&](long J) { return a.t[J] >= emax; });
                    const long ilo = lower_bound(0, a.N, [&](long I) { return a.t[I + 1] > xmin; });
                    const long ihi = lower_bound(0, a.N, [&](long I) { return a.t[I] >= xmax; });
                    const long nj = jhi > jlo ? jhi - jlo : 0, ni = ihi > ilo ? ihi - ilo : 0;
                    cum += (int)(nj * ni);   // at most N_MAX^2 per face
                    s_fj[ns][lane] = (f << 16) | (int)jlo, s_ilo[ns][lane] = (int)ilo, s_ni[ns][lane] = (int)ni;
                    s_cum[ns][lane] = cum;
                    ++ns;
                }
                cnt = cum;
            }
        }
        s_apoly[lane] = A;
        if (!WRITE) a_poly[c] = A;
    }
    s_ns[lane] = ns;
    const long long incl = wave_scan(cnt, lane);
    s_incl[lane] = incl;
    const long long T = __shfl(incl, TT - 1, TT);
    __syncthreads();
    long long run = 0, base = 0, limit = 0;
    if (WRITE) base = wave_off[w], limit = *total;
    for (long long t0 = 0; t0 < T; t0 += TT) {
        const long long t = t0 + lane;
        bool keep = false;
        int I = 0, J = 0, f = 0, o = 0;
        double ax = 0.0;
        if (t < T) {
            o = owner_of(s_incl, t);
            int q = (int)(t - (o ? s_incl[o - 1] : 0));
            int s = 0;
            const int nso = s_ns[o];
            while (s + 1 < nso && s_cum[s][o] <= q) ++s;   // the slot: the first whose inclusive count exceeds q
            if (s) q -= s_cum[s - 1][o];
            const int ni = s_ni[s][o];
            const int fj = s_fj[s][o];
            f = fj >> 16, J = (fj & 0xffff) + q / ni, I = s_ilo[s][o] + q % ni;
            const double clo = a.t[I], chi = a.t[I + 1], blo = a.t[J], bhi = a.t[J + 1];
            const double ap = s_apoly[o];
            bool all_in = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double xi = pxi[s][k][o], eta = peta[s][k][o];
                all_in = all_in && xi >= clo && xi <= chi && eta >= blo && eta <= bhi;
            }
            if (all_in) {
                ax = ap;   // every vertex inside every half-plane: the clip returns the polygon as it is
            } else {
                Clip<FanAcc> k{};
                k.c[0] = clo, k.c[1] = chi, k.c[2] = blo, k.c[3] = bhi;
                for (int v = 0; v < 4; ++v) clip_push<0>(k, pxi[s][v][o], peta[s][v][o]);
                clip_close<0>(k);
                ax = k.acc.n >= 3 ? g.Re2 * k.acc.s : 0.0;
            }
            keep = ax > 0.0 && ax > g.thr * fmin(ap, a.aatm[(long)J * a.N + I]);
        }
        const unsigned long long bal = __ballot(keep);
        if (WRITE && keep) {
            const long long pos = base + run + __popcll(bal & ((1ull << lane) - 1ull));
            if (pos < limit) {
                const long cc = w * TT + o, mr = cc / g.nxo;
                atm_fij[3 * pos] = I, atm_fij[3 * pos + 1] = J, atm_fij[3 * pos + 2] = f;
                ocn_ij[2 * pos] = (int)(cc - mr * g.nxo), ocn_ij[2 * pos + 1] = (int)(g.m0 + mr);
                area[pos] = ax;
            }
        }
        run += __popcll(bal);
    }
    if (!WRITE) {
        const int n_live = wave_sum(live ? 1 : 0);
        const int n_deg = wave_sum(live && st == ST_DEGENERATE ? 1 : 0);
        const int n_wide = wave_sum(live && st == ST_WIDE ? 1 : 0);
        const int n_inv = wave_sum(live && st == ST_INVERTED ? 1 : 0);
        const int n_mask = wave_sum(live && masked ? 1 : 0);
        const int n_face = wave_sum(ns);
        const long long n_cand = wave_sum(cnt);
        if (lane == 0) {
            count_add(&counts->cells, n_live), count_add(&counts->degenerate, n_deg), count_add(&counts->wide, n_wide);
            count_add(&counts->inverted, n_inv), count_add(&counts->masked, n_mask), count_add(&counts->face_candidates, n_face);
            count_add(&counts->candidates, n_cand), count_add(&counts->kept, run);
            wave_kept[w] = run;
        }
    }
}

int check_atm_shape(const ogg_xgrid_cs_atm& a) {
    OGG_REQUIRE(a.t, OGG_EARG, "cubed-sphere exchange grid: null table");
    OGG_REQUIRE(a.N >= 1 && a.N <= N_MAX, OGG_EARG, "cubed-sphere exchange grid: N = %ld, 1 .. %ld accepted", a.N, N_MAX);
    return OGG_OK;
}

int check_frames(const ogg_xgrid_cs_atm& a) {
    auto d3 = [](const double* p, const double* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
    for (int f = 0; f < NF; ++f) {
        const double *u = a.frames[f], *v = u + 3, *n = u + 6;
        for (int k = 0; k < 9; ++k) OGG_REQUIRE(std::isfinite(u[k]), OGG_EARG, "cubed-sphere exchange grid: frame %d is not finite", f);
        const bool ortho = fabs(d3(u, u) - 1.0) <= TOL && fabs(d3(v, v) - 1.0) <= TOL && fabs(d3(n, n) - 1.0) <= TOL &&
                           fabs(d3(u, v)) <= TOL && fabs(d3(v, n)) <= TOL && fabs(d3(n, u)) <= TOL;
        OGG_REQUIRE(ortho, OGG_EARG, "cubed-sphere exchange grid: frame %d is not orthonormal", f);
        const double cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        OGG_REQUIRE(fabs(cr[0] - n[0]) <= TOL && fabs(cr[1] - n[1]) <= TOL && fabs(cr[2] - n[2]) <= TOL, OGG_EARG,
                    "cubed-sphere exchange grid: frame %d is not right-handed (e_u x e_v != e_n)", f);
    }
    for (int f = 0; f < NF; ++f)
        for (int h = f + 1; h < NF; ++h) {
            const double d = d3(a.frames[f] + 6, a.frames[h] + 6);
            OGG_REQUIRE(fabs(d) <= TOL || fabs(d + 1.0) <= TOL, OGG_EARG,
                        "cubed-sphere exchange grid: the normals of faces %d and %d are neither orthogonal nor opposite", f, h);
        }
    for (int f = 0; f < NF; ++f)
        for (int e = 0; e < 2; ++e) {
            const double* p = a.frames[f] + 3 * e;
            bool found = false;
            for (int h = 0; h < NF && !found; ++h) {
                const double* n = a.frames[h] + 6;
                const bool plus = fabs(p[0] - n[0]) <= TOL && fabs(p[1] - n[1]) <= TOL && fabs(p[2] - n[2]) <= TOL;
                const bool minus = fabs(p[0] + n[0]) <= TOL && fabs(p[1] + n[1]) <= TOL && fabs(p[2] + n[2]) <= TOL;
                found = plus || minus;
            }
            OGG_REQUIRE(found, OGG_EARG, "cubed-sphere exchange grid: %s of face %d is no face's normal", e ? "e_v" : "e_u", f);
        }
    return OGG_OK;
}

int check_atm_host(const ogg_xgrid_cs_atm& a) {
    if (int e = check_atm_shape(a)) return e;
    for (long k = 0; k <= a.N; ++k)
        OGG_REQUIRE(std::isfinite(a.t[k]) && (k == 0 || a.t[k] > a.t[k - 1]), OGG_EARG,
                    "cubed-sphere exchange grid: the table must increase strictly (entry %ld)", k);
    OGG_REQUIRE(a.t[0] == -1.0 && a.t[a.N] == 1.0, OGG_EARG, "cubed-sphere exchange grid: the table runs %.17g .. %.17g, not -1 .. 1",
                a.t[0], a.t[a.N]);
    return check_frames(a);
}

// workspace: head (the total) | A_atm (N x N doubles) | kept per wave | offsets per wave; sections rounded to 64 bytes
struct Layout {
    long long* total;
    double* aatm;
    long long *kept, *off;
};

struct Offsets {
    long aatm, kept, off, total;
};

Offsets offsets(const ogg_xgrid_band& b, const ogg_xgrid_cs_atm& a) {
    ogg::Sections s{WS_HEAD, 64};
    return Offsets{s.take(a.N * a.N * 8), s.take(n_waves(b) * 8), s.take(n_waves(b) * 8), s.off};   // evaluated left to right
}

long ws_bytes(const ogg_xgrid_band& b, const ogg_xgrid_cs_atm& a) { return offsets(b, a).total; }

Layout layout(void* ws, const ogg_xgrid_band& b, const ogg_xgrid_cs_atm& a) {
    const Offsets o = offsets(b, a);
    return Layout{ogg::at<long long>(ws, 0), ogg::at<double>(ws, o.aatm), ogg::at<long long>(ws, o.kept), ogg::at<long long>(ws, o.off)};
}

int check_dev_args(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm, const void* workspace, long workspace_bytes) {
    OGG_REQUIRE(band && atm, OGG_EARG, "ogg_xgrid_cs: null pointer");
    if (int e = check_band(*band)) return e;
    if (int e = check_atm_shape(*atm)) return e;
    if (int e = check_frames(*atm)) return e;   // the frames are in the struct itself: host memory
    if (out_rows(*band) > 0)
        OGG_REQUIRE(band->x && band->y && band->x_next && band->y_next, OGG_EARG, "ogg_xgrid_band: null x / y / x_next / y_next");
    return ogg::check_workspace("ogg_xgrid_cs", workspace, workspace_bytes, ws_bytes(*band, *atm));
}

Frames frames_of(const ogg_xgrid_cs_atm& a) {
    Frames fr;
    for (int f = 0; f < NF; ++f)
        for (int k = 0; k < 9; ++k) fr.f[f][k] = a.frames[f][k];
    return fr;
}

}  // namespace

extern "C" long ogg_xgrid_cs_workspace_bytes(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm) {
    if (!band || !atm || band->j0 < 0 || band->n_cell_rows < 0 || band->nx < 2 || atm->N < 1 || atm->N > N_MAX) return -1;
    return ws_bytes(*band, *atm);
}

extern "C" int ogg_xgrid_cs_check_atm(const ogg_xgrid_cs_atm* atm) {
    OGG_REQUIRE(atm, OGG_EARG, "ogg_xgrid_cs_check_atm: null pointer");
    return check_atm_host(*atm);
}

extern "C" int ogg_xgrid_cs_count_dev(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm, void* workspace, long workspace_bytes,
                                      double* a_poly, ogg_xgrid_cs_counts* counts, void* stream) {
    if (int e = check_dev_args(band, atm, workspace, workspace_bytes)) return e;
    OGG_REQUIRE(counts, OGG_EARG, "ogg_xgrid_cs_count: null counts");
    const Geo g = make_geo(*band);
    OGG_REQUIRE(a_poly || g.ncells == 0, OGG_EARG, "ogg_xgrid_cs_count: null a_poly");
    const Layout l = layout(workspace, *band, *atm);
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_xgrid_cs_counts), st));
    OGG_HIP_CHECK(hipMemsetAsync(l.total, 0, sizeof(long long), st));
    if (g.ncells == 0) return OGG_OK;
    const long nn = atm->N * atm->N;
    xgrid_cs_aatm_kernel<<<(unsigned)((nn + 255) / 256), 256, 0, st>>>(atm->t, atm->N, g.Re2, l.aatm);
    OGG_LAUNCH_CHECK();
    const CsD a{atm->t, l.aatm, atm->N};
    const long nw = n_waves(*band);
    xgrid_cs_kernel<false><<<(unsigned)nw, TT, 0, st>>>(g, a, frames_of(*atm), a_poly, counts, l.kept, nullptr, nullptr, nullptr, nullptr,
                                                         nullptr);
    OGG_LAUNCH_CHECK();
    xgrid_scan_kernel<<<1, SCAN_T, 0, st>>>(l.kept, nw, l.off, l.total);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_xgrid_cs_write_dev(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm, const void* workspace, long workspace_bytes,
                                      int* atm_fij, int* ocn_ij, double* area, void* stream) {
    if (int e = check_dev_args(band, atm, workspace, workspace_bytes)) return e;
    const Geo g = make_geo(*band);
    if (g.ncells == 0) return OGG_OK;
    OGG_REQUIRE(atm_fij && ocn_ij && area, OGG_EARG, "ogg_xgrid_cs_write: null atm_fij / ocn_ij / area");
    const Layout l = layout(const_cast<void*>(workspace), *band, *atm);
    const CsD a{atm->t, l.aatm, atm->N};
    xgrid_cs_kernel<true><<<(unsigned)n_waves(*band), TT, 0, ogg::as_stream(stream)>>>(g, a, frames_of(*atm), nullptr, nullptr, nullptr,
                                                                                         l.off, l.total, atm_fij, ocn_ij, area);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: rows, mask and table copied to device memory, both steps, the results copied back (synchronous)
extern "C" int ogg_xgrid_cs(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm, long capacity, int* atm_fij, int* ocn_ij,
                            double* area, double* a_poly, ogg_xgrid_cs_counts* counts) {
    OGG_REQUIRE(band && atm && counts, OGG_EARG, "ogg_xgrid_cs: null pointer");
    if (int e = check_band(*band)) return e;
    if (int e = check_atm_host(*atm)) return e;
    const ogg_xgrid_band& h = *band;
    const long rows = out_rows(h), nc = rows * (h.nx / 2);
    *counts = ogg_xgrid_cs_counts{};
    if (rows == 0) return OGG_OK;
    OGG_REQUIRE(h.x && h.y && a_poly, OGG_EARG, "ogg_xgrid_cs: null x / y / a_poly");
    ogg::Buffers bufs;   // freed on every exit path
    double *pt, *ap, *la;
    char* ws;
    int *li, *lo;
    ogg_xgrid_cs_counts* ct;
    ogg_xgrid_band d;
    if (int e = stage_band(bufs, h, &d)) return e;
    if (int e = bufs.put(&pt, atm->t, (size_t)atm->N + 1)) return e;
    ogg_xgrid_cs_atm da = *atm;
    da.t = pt;
    const long wsb = ws_bytes(d, da);
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&ap, (size_t)nc)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = ogg_xgrid_cs_count_dev(&d, &da, ws, wsb, ap, ct, nullptr)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    if (int e = bufs.get(a_poly, ap, (size_t)nc)) return e;
    const long long kept = counts->kept;
    OGG_REQUIRE(kept <= capacity, OGG_ESHAPE, "ogg_xgrid_cs: %lld exchange cells, capacity %ld", kept, capacity);
    if (kept == 0) return OGG_OK;
    OGG_REQUIRE(atm_fij && ocn_ij && area, OGG_EARG, "ogg_xgrid_cs: null atm_fij / ocn_ij / area");
    if (int e = bufs.alloc(&li, (size_t)kept * 3)) return e;
    if (int e = bufs.alloc(&lo, (size_t)kept * 2)) return e;
    if (int e = bufs.alloc(&la, (size_t)kept)) return e;
    if (int e = ogg_xgrid_cs_write_dev(&d, &da, ws, wsb, li, lo, la, nullptr)) return e;
    if (int e = bufs.get(atm_fij, li, (size_t)kept * 3)) return e;
    if (int e = bufs.get(ocn_ij, lo, (size_t)kept * 2)) return e;
    if (int e = bufs.get(area, la, (size_t)kept)) return e;
    return OGG_OK;
}
