// Regional grids on a rotated pole (include/ogg_hip.h, "Regional grids"): a lat-lon or Mercator lattice in a frame whose equator runs
// through the domain, written as the six supergrid fields.
//
// tables      one thread per column and per row.  A column: the sincos of lam'_i folded into the rotation, a_i = cos lam' q1 + sin lam' q2
//             and e_z(i) (four doubles).  A row: cos phi', sin phi' (1/cosh and tanh of the Mercator ordinate) and the three metrics, which
//             are constants of a row: dx, dy, area, and phi' in degrees (six doubles).  The differences phi'_{j+1} - phi'_j and
//             sin phi'_{j+1} - sin phi'_j are formed without cancellation (the header gives the forms).
// band        the big launch: one thread per column of a workgroup's RB rows.  The column's four doubles stay in registers, the row's
//             five arrive by scalar loads (the row is uniform over the workgroup), and a point costs 9 fma and products, one sqrt and
//             three atan2 (ogg_math.h, coefficients as scalar operands) for 48 bytes written.  Workgroups are numbered columns first, so
//             consecutive workgroups write consecutive pieces of the same rows.  With lat_c = 0 and tilt = 0 the rotation is the
//             identity and the grid is the lattice: x = lon_c + lam'_i, y = phi'_j, angle_dx = 0 are written as such.
//
// Every value is a function of the two table entries of its (j, i) and of the parameters: the row chunk, the workgroup size and the band change no
// bit.  Built for gfx950 with -O3 (the compiler's kernel-resource-usage remarks): regional_band_kernel 39 VGPRs, 106 SGPRs (the
// forty of the arctangent's coefficients among them), no scratch, no LDS, 7 waves per SIMD of 8, the scalar registers being the
// limit; regional_tables_kernel 100 VGPRs, 68 SGPRs, no scratch, 4 waves per SIMD (one thread per row or column: a few workgroups).
#include <cmath>

#include "ogg_common.h"
#include "ogg_math.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;

constexpr int NT = 256;      // threads per workgroup: 256 columns
constexpr int RB = 8;        // rows a workgroup of the band kernel walks
constexpr double POLE_PAD = 1.0e-9;   // degrees
constexpr double kPi180Lo = 0x1.5c1d8becdd291p-62;   // pi/180 - ogg::kPi180

// the scalar arguments every entry takes, in the header's order
struct Params {
    long nx, ny;
    double lon_c, lat_c, tilt, delta, Re;
    int kind, metrics;
};

struct RowRec {
    double cp, sp, dx, dy, area, phi;   // phi: phi'_j in degrees, what y is under the identity rotation
};

struct Plan {
    double q1[3], q2[3], q3[3];
    double dl;                   // delta pi/180
    double lam_edge, phi_edge;   // degrees
};

struct Tables {
    long nx, ny;
    double delta, dl, Re;
    double q1[3], q2[3];
    int kind;
    double* col;                 // [4][nx + 1]: a_x, a_y, a_z, e_z
    RowRec* row;                 // [ny + 1]
};

struct Band {
    long nx, ny, j0, nrows, ncb;   // ncb: workgroups per row chunk
    double q3[3], lon_c;
    double delta;
    int metrics, identity;         // identity: lat_c = 0 and tilt = 0, the lattice itself is the grid
};

__global__ __launch_bounds__(NT) void regional_tables_kernel(Tables t) {
    const long k = (long)blockIdx.x * NT + threadIdx.x;
    const long npc = t.nx + 1;
    if (k < npc) {
        const double lam = ((double)(k - t.nx / 2) * t.delta) * ogg::kPi180;
        double s, c;
        sincos(lam, &s, &c);
        t.col[k] = fma(c, t.q1[0], s * t.q2[0]);
        t.col[npc + k] = fma(c, t.q1[1], s * t.q2[1]);
        t.col[2 * npc + k] = fma(c, t.q1[2], s * t.q2[2]);
        t.col[3 * npc + k] = fma(-s, t.q1[2], c * t.q2[2]);
    } else if (k < npc + t.ny + 1) {
        const long j = k - npc;
        const double jc = (double)(j - t.ny / 2);
        const double u = (jc * t.delta) * ogg::kPi180, um = ((jc + 0.5) * t.delta) * ogg::kPi180, h = 0.5 * t.dl;
        RowRec r;
        double dy, dsin;
        if (t.kind == OGG_REGIONAL_MERCATOR) {
            const double ch = cosh(u);
            const double u1 = ((jc + 1.0) * t.delta) * ogg::kPi180;
            r.cp = 1.0 / ch;
            r.sp = tanh(u);
            r.phi = atan(sinh(u)) / ogg::kPi180;
            dsin = sinh(t.dl) / (ch * cosh(u1));
            const double chm = cosh(um);
            if (h < 0x1p-5) {
                // dy = 2 Re atan(sinh h / cosh t_m) with h, the quotient and the product carried as a value and its rounding error, so
                // that cosh and the last sum are the only roundings left: h = delta pi/360 from pi/180 in two words; sinh h and the
                // arctangent of the quotient (at most sinh h) by their series, whose first terms left out are below 2^-60 of the result
                const double h_lo = 0.5 * (fma(t.delta, ogg::kPi180, -t.dl) + t.delta * kPi180Lo);
                const double h2 = h * h;
                const double ts = (h * h2) * fma(h2, fma(h2, fma(h2, 1.0 / 362880.0, 1.0 / 5040.0), 1.0 / 120.0), 1.0 / 6.0);   // sinh h - h
                const double s = h + ts;
                const double s_lo = ((h - s) + ts) + h_lo;
                const double q = s / chm;
                const double q_lo = (fma(-q, chm, s) + s_lo) / chm;
                const double q2 = q * q;
                const double ta = -(q * q2) * fma(q2, fma(q2, fma(q2, fma(q2, 1.0 / 11.0, -1.0 / 9.0), 1.0 / 7.0), -1.0 / 5.0), 1.0 / 3.0);   // atan q - q
                const double a = q + ta;
                const double a_lo = ((q - a) + ta) + q_lo;
                const double R2 = 2.0 * t.Re, prod = R2 * a;
                dy = prod + fma(R2, a_lo, fma(R2, a, -prod));
            } else {
                dy = t.Re * (2.0 * atan(sinh(h) / chm));
            }
        } else {
            sincos(u, &r.sp, &r.cp);
            r.phi = jc * t.delta;
            dy = t.Re * t.dl;
            dsin = (2.0 * cos(um)) * sin(h);
        }
        r.dx = (t.Re * r.cp) * t.dl;
        r.dy = j < t.ny ? dy : 0.0;
        r.area = j < t.ny ? ((t.Re * t.Re) * t.dl) * dsin : 0.0;
        t.row[j] = r;
    }
}

// the tables and the six outputs are arguments of their own: __restrict__ lets the row's record come by scalar loads between the stores
__global__ __launch_bounds__(NT) void regional_band_kernel(Band b, const double* __restrict__ col, const RowRec* __restrict__ row,
                                                           double* __restrict__ x, double* __restrict__ y, double* __restrict__ dx,
                                                           double* __restrict__ dy, double* __restrict__ area, double* __restrict__ angle) {
    const long wg = blockIdx.x;
    const long i = (wg % b.ncb) * NT + threadIdx.x;
    const long npc = b.nx + 1;
    const bool pt = i < npc, cell = i < b.nx;
    const long ic = pt ? i : b.nx;            // a lane beyond the row computes column nx and writes nothing
    const double ax = col[ic], ay = col[npc + ic], az = col[2 * npc + ic], ez = col[3 * npc + ic];
    ogg::AtanCoefs c;
    c.load(ogg::kAtanRed);
    const long jb = b.j0 + (wg / b.ncb) * RB;
    const long je = jb + RB < b.j0 + b.nrows ? jb + RB : b.j0 + b.nrows;
    for (long j = jb; j < je; ++j) {
        const RowRec r = row[j];
        const long jj = j - b.j0;
        if (b.identity) {   // p = p': x = lon_c + lam'_i, y = phi'_j, angle_dx = 0 -- the lattice itself, no arctangent of a sine and a cosine
            if (pt) {
                x[jj * npc + i] = b.lon_c + (double)(i - b.nx / 2) * b.delta;
                y[jj * npc + i] = r.phi;
                if (b.metrics) angle[jj * npc + i] = 0.0;
            }
        } else {
            const double px = fma(r.cp, ax, r.sp * b.q3[0]), py = fma(r.cp, ay, r.sp * b.q3[1]), pz = fma(r.cp, az, r.sp * b.q3[2]);
            const double h = ogg::sqrt_ieee_normal(fma(px, px, py * py));   // the poles are refused: h^2 is far inside the normal range
            const double lon = ogg::atan2_lib(py, px, c), lat = ogg::atan2_lib(pz, h, c);
            if (pt) {
                x[jj * npc + i] = b.lon_c + ogg::div_pi180(lon);
                y[jj * npc + i] = ogg::div_pi180(lat);
            }
            if (b.metrics) {
                const double ang = ogg::atan2_lib(ez, fma(r.cp, b.q3[2], -(r.sp * az)), c);
                if (pt) angle[jj * npc + i] = ogg::div_pi180(ang);
            }
        }
        if (b.metrics) {
            if (cell) dx[jj * b.nx + i] = r.dx;
            if (j < b.ny) {
                if (pt) dy[jj * npc + i] = r.dy;
                if (cell) area[jj * b.nx + i] = r.area;
            }
        }
    }
    c.keep();
}

// ---- host side -----------------------------------------------------------------------------------------------------
int plan_of(const Params* p, Plan* out) {
    OGG_REQUIRE(p->nx >= 2 && p->ny >= 2 && p->nx % 2 == 0 && p->ny % 2 == 0 && p->nx <= OGG_REGIONAL_MAX_CELLS && p->ny <= OGG_REGIONAL_MAX_CELLS,
                OGG_EARG, "regional: %ld x %ld supergrid cells: nx and ny even, >= 2 and <= %d", p->nx, p->ny, OGG_REGIONAL_MAX_CELLS);
    OGG_REQUIRE(p->kind == OGG_REGIONAL_LATLON || p->kind == OGG_REGIONAL_MERCATOR, OGG_EARG, "regional: kind %d (0: latlon, 1: mercator)",
                p->kind);
    OGG_REQUIRE(p->metrics == 0 || p->metrics == 1, OGG_EARG, "regional: metrics %d (0 or 1)", p->metrics);
    OGG_REQUIRE(std::isfinite(p->lon_c) && std::isfinite(p->lat_c) && std::isfinite(p->tilt) && std::isfinite(p->delta) && std::isfinite(p->Re),
                OGG_EARG, "regional: lon_c, lat_c, tilt, delta or Re is not finite");
    OGG_REQUIRE(p->delta > 0.0, OGG_EARG, "regional: delta = %g degrees per supergrid step: delta > 0", p->delta);
    OGG_REQUIRE(p->Re > 0.0, OGG_EARG, "regional: Re = %g: Re > 0", p->Re);
    OGG_REQUIRE(fabs(p->lat_c) <= 90.0, OGG_EARG, "regional: lat_c = %g: |lat_c| <= 90", p->lat_c);
    OGG_REQUIRE(fabs(p->lon_c) <= 1.0e6 && fabs(p->tilt) <= 1.0e6, OGG_EARG, "regional: lon_c = %g, tilt = %g: at most 1e6 in magnitude",
                p->lon_c, p->tilt);
    Plan& pl = *out;
    pl.dl = p->delta * ogg::kPi180;
    pl.lam_edge = (double)(p->nx / 2) * p->delta;
    OGG_REQUIRE(pl.lam_edge < 180.0, OGG_EARG, "regional: |lam'| = %g degrees at the edge (nx/2 * delta): below 180", pl.lam_edge);
    const double ye = (double)(p->ny / 2) * p->delta;
    pl.phi_edge = ye;
    if (p->kind == OGG_REGIONAL_MERCATOR) pl.phi_edge = ye * ogg::kPi180 < 700.0 ? atan(sinh(ye * ogg::kPi180)) / ogg::kPi180 : 90.0;
    OGG_REQUIRE(pl.phi_edge <= 89.0, OGG_EARG, "regional: |phi'| = %g degrees at the edge: at most 89", pl.phi_edge);
    const double cl = cos(p->lat_c * ogg::kPi180), sl = sin(p->lat_c * ogg::kPi180);
    const double ct = cos(p->tilt * ogg::kPi180), st = sin(p->tilt * ogg::kPi180);
    pl.q1[0] = cl, pl.q1[1] = 0.0, pl.q1[2] = sl;
    pl.q2[0] = -sl * st, pl.q2[1] = ct, pl.q2[2] = cl * st;
    pl.q3[0] = -sl * ct, pl.q3[1] = -st, pl.q3[2] = cl * ct;
    // the geographic north pole in the rotated frame is the third row of the rotation, the south pole its negative
    const double hz = sqrt(pl.q1[2] * pl.q1[2] + pl.q2[2] * pl.q2[2]);
    const double phi_n = atan2(pl.q3[2], hz) / ogg::kPi180;
    const double lam_n = atan2(pl.q2[2], pl.q1[2]) / ogg::kPi180, lam_s = atan2(-pl.q2[2], -pl.q1[2]) / ogg::kPi180;
    const bool in_phi = fabs(phi_n) <= pl.phi_edge + POLE_PAD;
    OGG_REQUIRE(!(in_phi && fabs(lam_n) <= pl.lam_edge + POLE_PAD), OGG_EARG,
                "regional: the domain holds the north pole (lam' = %g, phi' = %g in the rotated frame): pole-holding domains are not generated",
                lam_n, phi_n);
    OGG_REQUIRE(!(in_phi && fabs(lam_s) <= pl.lam_edge + POLE_PAD), OGG_EARG,
                "regional: the domain holds the south pole (lam' = %g, phi' = %g in the rotated frame): pole-holding domains are not generated",
                lam_s, -phi_n);
    return OGG_OK;
}

struct Layout {
    long col, row, total;
};

Layout layout(const Params& p) {
    Layout l;
    ogg::Sections s{0};
    l.col = s.take(4 * (p.nx + 1) * (long)sizeof(double));
    l.row = s.take((p.ny + 1) * (long)sizeof(RowRec));
    l.total = s.off;
    return l;
}

}  // namespace

extern "C" int ogg_regional_check(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics};
    const Params* p = &prm;
    Plan pl;
    return plan_of(p, &pl);
}

extern "C" long ogg_regional_workspace_bytes(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics};
    const Params* p = &prm;
    Plan pl;
    if (plan_of(p, &pl) != OGG_OK) return -1;
    return layout(*p).total;
}

extern "C" int ogg_regional_tables_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics,
                                       void* workspace, long workspace_bytes, void* stream) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics};
    const Params* p = &prm;
    Plan pl;
    if (int e = plan_of(p, &pl)) return e;
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_regional_tables", workspace, workspace_bytes, l.total)) return e;
    Tables t{};
    t.nx = p->nx, t.ny = p->ny, t.delta = p->delta, t.dl = pl.dl, t.Re = p->Re, t.kind = p->kind;
    for (int k = 0; k < 3; ++k) t.q1[k] = pl.q1[k], t.q2[k] = pl.q2[k];
    t.col = at<double>(workspace, l.col);
    t.row = at<RowRec>(workspace, l.row);
    const long n = p->nx + p->ny + 2;
    regional_tables_kernel<<<(unsigned)((n + NT - 1) / NT), NT, 0, ogg::as_stream(stream)>>>(t);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_regional_band_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics,
                                     long j0, long nrows, const void* workspace, long workspace_bytes, double* x, double* y, double* dx,
                                     double* dy, double* area, double* angle_dx, void* stream) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics};
    const Params* p = &prm;
    Plan pl;
    if (int e = plan_of(p, &pl)) return e;
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_regional_band", workspace, workspace_bytes, l.total)) return e;
    OGG_REQUIRE(j0 >= 0 && nrows >= 0 && j0 + nrows <= p->ny + 1, OGG_EARG, "ogg_regional_band: rows %ld .. %ld of %ld point rows", j0,
                j0 + nrows, p->ny + 1);
    const long cell_rows = (j0 + nrows <= p->ny ? j0 + nrows : p->ny) - j0;   // the band's rows below row ny
    OGG_REQUIRE(x && y && (!p->metrics || (dx && angle_dx && ((dy && area) || cell_rows <= 0))), OGG_EARG,
                "ogg_regional_band: null x / y / dx / dy / area / angle_dx");
    if (nrows == 0) return OGG_OK;
    Band b{};
    b.nx = p->nx, b.ny = p->ny, b.j0 = j0, b.nrows = nrows, b.ncb = (p->nx + 1 + NT - 1) / NT;
    for (int k = 0; k < 3; ++k) b.q3[k] = pl.q3[k];
    b.lon_c = p->lon_c, b.delta = p->delta, b.metrics = p->metrics;
    b.identity = pl.q1[0] == 1.0 && pl.q1[2] == 0.0 && pl.q2[1] == 1.0 && pl.q2[2] == 0.0;   // cl = ct = 1 and sl = st = 0
    const long chunks = (nrows + RB - 1) / RB;
    OGG_REQUIRE(b.ncb * chunks < (1L << 31), OGG_EARG, "ogg_regional_band: %ld rows of %ld columns in one launch: fewer rows per band", nrows,
                p->nx + 1);
    regional_band_kernel<<<(unsigned)(b.ncb * chunks), NT, 0, ogg::as_stream(stream)>>>(b, at<double>(workspace, l.col),
                                                                                        at<RowRec>(workspace, l.row), x, y, dx, dy, area, angle_dx);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_regional_grid(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics,
                                 double* x, double* y, double* dx, double* dy, double* area, double* angle_dx) {
    const Params prm{nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics};
    const Params* p = &prm;
    Plan pl;
    if (int e = plan_of(p, &pl)) return e;
    OGG_REQUIRE(x && y && (!p->metrics || (dx && dy && area && angle_dx)), OGG_EARG, "ogg_regional_grid: null argument");
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
    if (int e = ogg_regional_tables_dev(nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics, ws, wsb, nullptr)) return e;
    if (int e = ogg_regional_band_dev(nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics, 0, ny + 1, ws, wsb, tx, ty, tdx, tdy, ta, tg, nullptr)) return e;
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
