// Stereographic regional grids (include/ogg_hip.h, "Stereographic regional grids"): the oblique stereographic lattice about a centre,
// which may hold a geographic pole, written as the six supergrid fields.  The first regional kind whose metrics depend on both indices.
//
// tables      one thread per column and per row (one more of each than the grid has, so that a cell's far side is an entry too).  A
//             line Z (a column's X_i or a row's Y_j) carries Z, Z^2/4 and Z q, the edge's constants e = 4 + Z^2, sqrt(e) d and
//             4 Re / sqrt(e), and the constants of the pair (Z, Z + d) that the area needs (below).
// band        the big launch: a wavefront owns 63 columns and its last lane the column after them, which only lends its dy to lane 62
//             (a DPP wave shift; the next wavefront computes the same column from the same table entries, so the bits are those of the
//             formula whatever the wavefront): 252 columns per workgroup of 256 threads, RB rows walked upward.  The column's values
//             stay in registers, the row's arrive by scalar loads, the arctangent's coefficients are scalar operands.  Per point:
//             n = X q2 + Y q3 + (1 - rho^2/4) q1 is p times m, and an arctangent of two arguments needs no common factor, so the
//             definition's one division by m is not made at all: x = atan2(n_y, n_x), y = atan2(n_z, sqrt(n_x^2 + n_y^2)).
//             angle_dx: with T = m t = (1 + (Y^2 - X^2)/4) q2 - X q1 - (X Y/2) q3 the cross product n x T is m S,
//             S = (1 + (X^2 - Y^2)/4) q3 - Y q1 - (X Y/2) q2 (the grid's y direction times m), so angle_dx = atan2(T_z, S_z): two
//             short fma chains, no p.  dx = (4 Re/a) A, A = atan(a d / (a^2 + X_i X_{i+1})): the argument is at most d/2 < 1, so it
//             is the reduced arctangent with no reciprocal.  A of row j + 1 is kept for the next row.  dy likewise.
// area        the definition's form differences neighbouring edges and loses eps |Y| / d.  Here each difference is taken apart: with
//             s = Z/sqrt(4 + Z^2) and A = the edge's arctangent,  Z1 dxh1 - Z0 dxh0 = 4 [(s1 - s0) A1 + s0 (A1 - A0)],
//               s1 - s0 = 4 d (Z0 + Z1) / (a0 a1 (Z1 a0 + Z0 a1))                 (Z0, Z1 never differ in sign: 0 is a mesh line)
//               A1 - A0 = atan(v),  v = d (a0 - a1) (a0 a1 - W) / (den0 den1 + a0 a1 d^2),  a0 - a1 = -d (Z0 + Z1) / (a0 + a1)
//             (W the product of the cell's two coordinates across, den = a^2 + W): no difference of near-equal numbers is left.
//             |v| <= tan(d^2/4): for d <= 1/16 its arctangent is v - v^3/3 + v^5/5 (the next term is below 2^-62 of it), else the
//             reduced arctangent; the choice depends on d alone.
//
// Every value is a function of the table entries of its (j, i) and of the parameters: the row chunk, the wavefront, the workgroup and the band
// change no bit.  Built for gfx950 with -O3 (the compiler's kernel-resource-usage remarks): stereo_band_kernel 70 VGPRs, 106 SGPRs (the
// forty of the arctangent's coefficients among them; the row's record and the kernel's arguments do not all fit beside them, and 62
// scalar values are kept in the lanes of vector registers), no scratch, no LDS, 7 waves per SIMD of 8; stereo_tables_kernel 48 VGPRs,
// 36 SGPRs, no scratch, 8 waves per SIMD.
#include <cmath>

#include "ogg_common.h"
#include "ogg_math.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;

constexpr int NT = 256;      // threads per workgroup
constexpr int CW = 63;       // columns a wavefront owns; its lane 63 computes the next column and writes nothing
constexpr int CB = 4 * CW;   // columns per workgroup
constexpr int RB = 8;        // rows a workgroup of the band kernel walks
constexpr double POLE_PAD = 1.0e-9;                  // degrees
constexpr double kPi180Lo = 0x1.5c1d8becdd291p-62;   // pi/180 - ogg::kPi180
constexpr double SERIES_D = 0x1p-4;                  // d at most this: atan(v) of the area by three terms

// the scalar arguments every entry takes, in the header's order
struct Params {
    long nx, ny;
    double lon_c, lat_c, tilt, delta, Re;
    int metrics;
};

struct Plan {
    double q1[3], q2[3], q3[3];
    double d;        // delta pi/180, rounded once
    int polar;       // lat_c = +-90 exactly: the centre point IS a pole and has its defined values
};

// a line's edge constants and the pair (Z, Z + d)'s area constants, the same for a column (Z = X_i) and a row (Z = Y_j)
struct Line {
    double e, ed, k;             // 4 + Z^2;  sqrt(e) d;  4 Re / sqrt(e)
    double W;                    // Z0 Z1
    double ds, s0, P, cr, Pd2;   // s1 - s0;  s0;  a0 a1;  d (a0 - a1);  a0 a1 d^2
};

// the column table, [NCOL][nx + 2]
enum { C_X, C_XS, C_Q2X, C_Q2Y, C_Q2Z, C_Q1Z, C_E, C_ED, C_K, C_W, C_DS, C_S0, C_P, C_CR, C_PD2, NCOL };

struct RowRec {
    double Y, wm, wp;            // Y_j, 1 - Y^2/4, 1 + Y^2/4
    double q3x, q3y, q3z;        // Y q3
    double q1z, hq2;             // Y q1_z, Y q2_z / 2
    Line l;
};

struct Tables {
    long nx, ny;
    double d, Re;
    double q1z, q2[3], q3[3];
    double* col;
    RowRec* row;
};

struct Band {
    long nx, ny, j0, nrows, ncb;   // ncb: workgroups per row chunk
    double q1x, q1z, q2z, q3z;
    double lon_c, lat_c, tilt, hR2;   // hR2: 2 Re^2
    int metrics, polar, series;
};

__device__ Line line_of(double Z0, double Z1, double d, double Re) {
    Line l;
    l.e = fma(Z0, Z0, 4.0);
    const double a0 = sqrt(l.e), a1 = sqrt(fma(Z1, Z1, 4.0));
    l.ed = a0 * d;
    l.k = (4.0 * Re) / a0;
    l.W = Z0 * Z1;
    const double sum = Z0 + Z1;
    l.P = a0 * a1;
    l.ds = ((4.0 * d) * sum) / (l.P * fma(Z1, a0, Z0 * a1));
    l.s0 = Z0 / a0;
    l.cr = -((d * d) * sum) / (a0 + a1);
    l.Pd2 = l.P * (d * d);
    return l;
}

__global__ __launch_bounds__(NT) void stereo_tables_kernel(Tables t) {
    const long k = (long)blockIdx.x * NT + threadIdx.x;
    const long nc = t.nx + 2;
    if (k < nc) {
        const double X = (double)(k - t.nx / 2) * t.d, X1 = (double)(k + 1 - t.nx / 2) * t.d;
        const Line l = line_of(X, X1, t.d, t.Re);
        double* c = t.col + k;
        c[C_X * nc] = X, c[C_XS * nc] = 0.25 * (X * X);
        c[C_Q2X * nc] = X * t.q2[0], c[C_Q2Y * nc] = X * t.q2[1], c[C_Q2Z * nc] = X * t.q2[2], c[C_Q1Z * nc] = X * t.q1z;
        c[C_E * nc] = l.e, c[C_ED * nc] = l.ed, c[C_K * nc] = l.k, c[C_W * nc] = l.W;
        c[C_DS * nc] = l.ds, c[C_S0 * nc] = l.s0, c[C_P * nc] = l.P, c[C_CR * nc] = l.cr, c[C_PD2 * nc] = l.Pd2;
    } else if (k < nc + t.ny + 2) {
        const long j = k - nc;
        const double Y = (double)(j - t.ny / 2) * t.d, Y1 = (double)(j + 1 - t.ny / 2) * t.d;
        RowRec r;
        r.Y = Y, r.wm = fma(-0.25 * Y, Y, 1.0), r.wp = fma(0.25 * Y, Y, 1.0);
        r.q3x = Y * t.q3[0], r.q3y = Y * t.q3[1], r.q3z = Y * t.q3[2];
        r.q1z = Y * t.q1z, r.hq2 = 0.5 * (Y * t.q2[2]);
        r.l = line_of(Y, Y1, t.d, t.Re);
        t.row[j] = r;
    }
}

// the arctangent of an edge: its argument is at most d/2 < 1
template <class C>
__device__ __forceinline__ double edge_atan(double ed, double den, const C& c) {
    return ogg::atanred_lib(ogg::div_ieee_normal(ed, den), c);
}

// A1 - A0 of the two edges of a pair: atan(v), |v| <= tan(d^2/4) <= 0.55
template <class C>
__device__ __forceinline__ double pair_atan(double cr, double P, double Pd2, double W, double den0, double den1, int series, const C& c) {
    const double v = ogg::div_ieee_normal(cr * (P - W), fma(den0, den1, Pd2));
    if (series) {
        const double v2 = v * v;
        return fma(v * v2, fma(v2, 0.2, -1.0 / 3.0), v);
    }
    return ogg::atanred_lib(v, c);
}

// the tables and the six outputs are arguments of their own: __restrict__ lets the row's record come by scalar loads between the stores
__global__ __launch_bounds__(NT) void stereo_band_kernel(Band b, const double* __restrict__ col, const RowRec* __restrict__ row,
                                                         double* __restrict__ x, double* __restrict__ y, double* __restrict__ dx,
                                                         double* __restrict__ dy, double* __restrict__ area, double* __restrict__ angle) {
    const long wg = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const long i = (wg % b.ncb) * CB + (threadIdx.x >> 6) * CW + lane;
    const long npc = b.nx + 1, nc = b.nx + 2;
    const bool own = lane < CW;
    const bool pt = own && i < npc, cell = own && i < b.nx;
    const long ic = i < npc ? i : b.nx;       // a lane beyond the row computes column nx and writes nothing
    const double* cc = col + ic;
    const double X = cc[C_X * nc], xs = cc[C_XS * nc], Xq2x = cc[C_Q2X * nc], Xq2y = cc[C_Q2Y * nc], Xq2z = cc[C_Q2Z * nc];
    double Xq1z = 0.0, ce = 0.0, ce1 = 0.0, ced = 0.0, ck = 0.0, cW = 0.0, cds = 0.0, cs0 = 0.0, cP = 0.0, ccr = 0.0, cPd2 = 0.0;
    if (b.metrics) {
        Xq1z = cc[C_Q1Z * nc], ce = cc[C_E * nc], ce1 = cc[C_E * nc + 1], ced = cc[C_ED * nc], ck = cc[C_K * nc], cW = cc[C_W * nc];
        cds = cc[C_DS * nc], cs0 = cc[C_S0 * nc], cP = cc[C_P * nc], ccr = cc[C_CR * nc], cPd2 = cc[C_PD2 * nc];
    }
    ogg::AtanCoefs c;
    c.load(ogg::kAtanRed);
    const long jb = b.j0 + (wg / b.ncb) * RB;
    const long je = jb + RB < b.j0 + b.nrows ? jb + RB : b.j0 + b.nrows;
    double A0 = 0.0;   // the arctangent of this row's dx edge, kept from the row below
    if (b.metrics) A0 = edge_atan(row[jb].l.ed, row[jb].l.e + cW, c);
    for (long j = jb; j < je; ++j) {
        const RowRec r = row[j];
        const long jj = j - b.j0;
        const bool cen = b.polar && j == b.ny / 2 && i == b.nx / 2;   // the centre of a grid about a pole: its values are defined
        const double w = r.wm - xs;
        const double nx_ = fma(w, b.q1x, Xq2x + r.q3x), ny_ = Xq2y + r.q3y, nz_ = fma(w, b.q1z, Xq2z + r.q3z);
        const double hh = fma(nx_, nx_, ny_ * ny_);
        const double h = ogg::sqrt_ieee_normal(cen ? 1.0 : hh);   // every other point is 1e-9 degrees or more from a pole: hh >= 3e-22
        const double lon = ogg::atan2_lib(ny_, nx_, c), lat = ogg::atan2_lib(nz_, h, c);
        if (pt) {
            x[jj * npc + i] = cen ? b.lon_c : b.lon_c + ogg::div_pi180(lon);
            y[jj * npc + i] = cen ? b.lat_c : ogg::div_pi180(lat);
        }
        if (b.metrics) {
            const double Tz = fma(-X, 0.5 * r.q3z, fma(r.wp - xs, b.q2z, -Xq1z));
            const double Sz = fma(-X, r.hq2, fma(r.wm + xs, b.q3z, -r.q1z));
            const double ang = ogg::atan2_lib(Tz, Sz, c);
            if (pt) angle[jj * npc + i] = cen ? b.tilt : ogg::div_pi180(ang);
            // the edges: dx of this row from the kept arctangent, that of the row above for the area and the next row
            const double e1 = row[j + 1].l.e, ed1 = row[j + 1].l.ed;
            const double den0 = r.l.e + cW, den1 = e1 + cW;
            const double A1 = edge_atan(ed1, den1, c);
            const double dB0 = ce + r.l.W, dB1 = ce1 + r.l.W;
            const double B0 = edge_atan(ced, dB0, c);
            const double B1 = ogg::wave_next(B0);   // lane 63 keeps its own, and owns no cell
            if (cell) dx[jj * b.nx + i] = r.l.k * A0;
            if (j < b.ny) {
                if (pt) dy[jj * npc + i] = ck * B0;
                const double gy = fma(r.l.ds, A1, r.l.s0 * pair_atan(r.l.cr, r.l.P, r.l.Pd2, cW, den0, den1, b.series, c));
                const double gx = fma(cds, B1, cs0 * pair_atan(ccr, cP, cPd2, r.l.W, dB0, dB1, b.series, c));
                if (cell) area[jj * b.nx + i] = b.hR2 * (gy + gx);
            }
            A0 = A1;
        }
    }
    c.keep();
}

// ---- host side -----------------------------------------------------------------------------------------------------
int plan_of(const Params* p, Plan* out) {
    OGG_REQUIRE(p->nx >= 2 && p->ny >= 2 && p->nx % 2 == 0 && p->ny % 2 == 0 && p->nx <= OGG_REGIONAL_MAX_CELLS && p->ny <= OGG_REGIONAL_MAX_CELLS,
                OGG_EARG, "regional stereo: %ld x %ld supergrid cells: nx and ny even, >= 2 and <= %d", p->nx, p->ny, OGG_REGIONAL_MAX_CELLS);
    OGG_REQUIRE(p->metrics == 0 || p->metrics == 1, OGG_EARG, "regional stereo: metrics %d (0 or 1)", p->metrics);
    OGG_REQUIRE(std::isfinite(p->lon_c) && std::isfinite(p->lat_c) && std::isfinite(p->tilt) && std::isfinite(p->delta) && std::isfinite(p->Re),
                OGG_EARG, "regional stereo: lon_c, lat_c, tilt, delta or Re is not finite");
    OGG_REQUIRE(p->delta > 0.0, OGG_EARG, "regional stereo: delta = %g degrees per supergrid step: delta > 0", p->delta);
    OGG_REQUIRE(p->Re > 0.0, OGG_EARG, "regional stereo: Re = %g: Re > 0", p->Re);
    OGG_REQUIRE(fabs(p->lat_c) <= 90.0, OGG_EARG, "regional stereo: lat_c = %g: |lat_c| <= 90", p->lat_c);
    OGG_REQUIRE(fabs(p->lon_c) <= 1.0e6 && fabs(p->tilt) <= 1.0e6, OGG_EARG, "regional stereo: lon_c = %g, tilt = %g: at most 1e6 in magnitude",
                p->lon_c, p->tilt);
    Plan& pl = *out;
    // delta pi/180 from pi/180 in two words, rounded once
    const double d = p->delta * ogg::kPi180;
    pl.d = d + (fma(p->delta, ogg::kPi180, -d) + p->delta * kPi180Lo);
    const double hx = (double)(p->nx / 2), hy = (double)(p->ny / 2);
    const double rho = pl.d * sqrt(hx * hx + hy * hy);
    OGG_REQUIRE(rho <= 2.0, OGG_EARG, "regional stereo: a corner lies %g degrees from the centre: at most 90 (a hemisphere)",
                2.0 * atan(0.5 * rho) / ogg::kPi180);
    pl.polar = fabs(p->lat_c) == 90.0;
    // the cosine of +-90 degrees is 0, which cos(pi/2 rounded) is not
    const double cl = pl.polar ? 0.0 : cos(p->lat_c * ogg::kPi180), sl = pl.polar ? copysign(1.0, p->lat_c) : sin(p->lat_c * ogg::kPi180);
    const double ct = cos(p->tilt * ogg::kPi180), st = sin(p->tilt * ogg::kPi180);
    pl.q1[0] = cl, pl.q1[1] = 0.0, pl.q1[2] = sl;
    pl.q2[0] = -sl * st, pl.q2[1] = ct, pl.q2[2] = cl * st;
    pl.q3[0] = -sl * ct, pl.q3[1] = -st, pl.q3[2] = cl * ct;
    // the poles in the plane: north at 2 (q2_z, q3_z) / (1 + q1_z), south at -2 (q2_z, q3_z) / (1 - q1_z); one of a hemisphere's domain
    // at most.  A pole may lie in the domain, but no mesh point on it, the centre of a grid about a pole apart
    for (int s = 1; s >= -1; s -= 2) {
        const double den = 1.0 + s * pl.q1[2];
        if (den < 0.25) continue;   // farther than 90 degrees from the centre
        const double Xp = s * 2.0 * pl.q2[2] / den, Yp = s * 2.0 * pl.q3[2] / den;
        const double fi = Xp / pl.d + hx, fj = Yp / pl.d + hy;
        if (fi < -1.0 || fi > (double)p->nx + 1.0 || fj < -1.0 || fj > (double)p->ny + 1.0) continue;
        long i = lround(fi), j = lround(fj);
        i = i < 0 ? 0 : (i > p->nx ? p->nx : i), j = j < 0 ? 0 : (j > p->ny ? p->ny : j);
        if (pl.polar && i == p->nx / 2 && j == p->ny / 2) continue;
        const double ex = Xp - (double)(i - p->nx / 2) * pl.d, ey = Yp - (double)(j - p->ny / 2) * pl.d;
        const double deg = sqrt(ex * ex + ey * ey) / (1.0 + 0.25 * (Xp * Xp + Yp * Yp)) / ogg::kPi180;
        OGG_REQUIRE(deg > POLE_PAD, OGG_EARG,
                    "regional stereo: the mesh point (j, i) = (%ld, %ld) lies %g degrees from the %s pole: only the centre of a grid with "
                    "lat_c = +-90 exactly may be a pole",
                    j, i, deg, s > 0 ? "north" : "south");
    }
    return OGG_OK;
}

struct Layout {
    long col, row, total;
};

Layout layout(const Params& p) {
    Layout l;
    ogg::Sections s{0};
    l.col = s.take(NCOL * (p.nx + 2) * (long)sizeof(double));
    l.row = s.take((p.ny + 2) * (long)sizeof(RowRec));
    l.total = s.off;
    return l;
}

}  // namespace

extern "C" int ogg_regional_stereo_check(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, metrics};
    const Params* p = &prm;
    Plan pl;
    return plan_of(p, &pl);
}

extern "C" long ogg_regional_stereo_workspace_bytes(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, metrics};
    const Params* p = &prm;
    Plan pl;
    if (plan_of(p, &pl) != OGG_OK) return -1;
    return layout(*p).total;
}

extern "C" int ogg_regional_stereo_tables_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics,
                                              void* workspace, long workspace_bytes, void* stream) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, metrics};
    const Params* p = &prm;
    Plan pl;
    if (int e = plan_of(p, &pl)) return e;
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_regional_stereo_tables", workspace, workspace_bytes, l.total)) return e;
    Tables t{};
    t.nx = p->nx, t.ny = p->ny, t.d = pl.d, t.Re = p->Re, t.q1z = pl.q1[2];
    for (int k = 0; k < 3; ++k) t.q2[k] = pl.q2[k], t.q3[k] = pl.q3[k];
    t.col = at<double>(workspace, l.col);
    t.row = at<RowRec>(workspace, l.row);
    const long n = p->nx + p->ny + 4;
    stereo_tables_kernel<<<(unsigned)((n + NT - 1) / NT), NT, 0, ogg::as_stream(stream)>>>(t);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_regional_stereo_band_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics,
                                            long j0, long nrows, const void* workspace, long workspace_bytes, double* x, double* y, double* dx,
                                            double* dy, double* area, double* angle_dx, void* stream) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, metrics};
    const Params* p = &prm;
    Plan pl;
    if (int e = plan_of(p, &pl)) return e;
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_regional_stereo_band", workspace, workspace_bytes, l.total)) return e;
    OGG_REQUIRE(j0 >= 0 && nrows >= 0 && j0 + nrows <= p->ny + 1, OGG_EARG, "ogg_regional_stereo_band: rows %ld .. %ld of %ld point rows", j0,
                j0 + nrows, p->ny + 1);
    const long cell_rows = (j0 + nrows <= p->ny ? j0 + nrows : p->ny) - j0;   // the band's rows below row ny
    OGG_REQUIRE(x && y && (!p->metrics || (dx && angle_dx && ((dy && area) || cell_rows <= 0))), OGG_EARG,
                "ogg_regional_stereo_band: null x / y / dx / dy / area / angle_dx");
    if (nrows == 0) return OGG_OK;
    Band b{};
    b.nx = p->nx, b.ny = p->ny, b.j0 = j0, b.nrows = nrows, b.ncb = (p->nx + 1 + CB - 1) / CB;
    b.q1x = pl.q1[0], b.q1z = pl.q1[2], b.q2z = pl.q2[2], b.q3z = pl.q3[2];
    b.lon_c = p->lon_c, b.lat_c = p->lat_c, b.tilt = p->tilt, b.hR2 = 2.0 * (p->Re * p->Re);
    b.metrics = p->metrics, b.polar = pl.polar, b.series = pl.d <= SERIES_D;
    const long chunks = (nrows + RB - 1) / RB;
    OGG_REQUIRE(b.ncb * chunks < (1L << 31), OGG_EARG, "ogg_regional_stereo_band: %ld rows of %ld columns in one launch: fewer rows per band",
                nrows, p->nx + 1);
    stereo_band_kernel<<<(unsigned)(b.ncb * chunks), NT, 0, ogg::as_stream(stream)>>>(b, at<double>(workspace, l.col),
                                                                                      at<RowRec>(workspace, l.row), x, y, dx, dy, area, angle_dx);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_regional_stereo_grid(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics, double* x,
                                        double* y, double* dx, double* dy, double* area, double* angle_dx) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, metrics};
    const Params* p = &prm;
    Plan pl;
    if (int e = plan_of(p, &pl)) return e;
    OGG_REQUIRE(x && y && (!p->metrics || (dx && dy && area && angle_dx)), OGG_EARG, "ogg_regional_stereo_grid: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t npr = (size_t)ny + 1, npc = (size_t)nx + 1, nyc = (size_t)ny, nxc = (size_t)nx;
    const long wsb = layout(*p).total;
    double *tx, *ty, *tdx = nullptr, *tdy = nullptr, *ta = nullptr, *tg = nullptr;
    char* ws;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&tx, npr * npc)) return e;
    if (int e = bufs.alloc(&ty, npr * npc)) return e;
    if (p->metrics) {
        if (int e = bufs.alloc(&tdx, npr * nxc)) return e;
        if (int e = bufs.alloc(&tdy, nyc * npc)) return e;
        if (int e = bufs.alloc(&ta, nyc * nxc)) return e;
        if (int e = bufs.alloc(&tg, npr * npc)) return e;
    }
    if (int e = ogg_regional_stereo_tables_dev(nx, ny, lon_c, lat_c, tilt, delta, Re, metrics, ws, wsb, nullptr)) return e;
    if (int e = ogg_regional_stereo_band_dev(nx, ny, lon_c, lat_c, tilt, delta, Re, metrics, 0, ny + 1, ws, wsb, tx, ty, tdx, tdy, ta, tg, nullptr)) return e;
    if (int e = bufs.get(x, tx, npr * npc)) return e;
    if (int e = bufs.get(y, ty, npr * npc)) return e;
    if (p->metrics) {
        if (int e = bufs.get(dx, tdx, npr * nxc)) return e;
        if (int e = bufs.get(dy, tdy, nyc * npc)) return e;
        if (int e = bufs.get(area, ta, nyc * nxc)) return e;
        if (int e = bufs.get(angle_dx, tg, npr * npc)) return e;
    }
    return OGG_OK;
}
