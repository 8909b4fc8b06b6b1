// Topography by refined sampling (include/ogg_hip.h, "Topography by refined sampling"): every output cell (a model cell = 2 x 2
// supergrid cells, or one supergrid cell) is filled with R x R samples per supergrid cell, each sample looks up its source raster
// element, and the cell keeps integer sums, extremes and counts.
//
// topog_walk: the one sampling walk, one wavefront per workgroup.  A wavefront takes runs of TR consecutive output cells of a row
// from a counter in the workspace (so the cells that need many samples -- R up to 256 next to a pole -- do not hold up a static
// share), and owns each output cell it takes: lanes 0..3 set up the (up to) four supergrid cells of it (unwrapped corners, R, pole
// test) into LDS, then the whole wavefront walks the flattened samples f = b * R + a of each supergrid cell, lane l taking f = l,
// l + 64, ...: consecutive lanes are consecutive a (along i, i.e. along a raster row), so one gather instruction touches a few 128-B
// lines.  s = (a + 0.5) / R and 1 - s come from a per-wavefront LDS table rebuilt when R changes (two fp64 divisions per sample would
// otherwise dominate).  Each lane keeps its own counts, sums and extremes in registers; the wavefront reduces them with shuffles
// (integers: exact, in any order) and lane 0 stores the record.  No atomics touch a result; the only atomic is the work counter.
// The positions of the samples are formed in the walk alone, so every entry point samples the same points bit for bit.  Where R comes
// from when the band does not fix it, what a sample is worth and what the record holds are a sampler's: the hooks listed at
// topog_walk, resolved at compile time, so that a hook a sampler has no use for is an empty function.
//
// SingleSampler<DT, PLANE> (topog_band_kernel; "Topography by refined sampling"): one lat-lon raster, its dtype a compile-time
// constant; R of a supergrid cell is the setting-up lane's own affair.  PLANE (ogg_topog_plane_band_dev) also keeps the integer
// moments of the least-squares plane of "Plane-fit topography".  Lane 0 sets up the output cell's origin (its raster column and row)
// into LDS; a sample's offsets from it are int32 differences of the indices the sample already has (the periodic column offset
// folded into [-Nx/2, Nx/2) with two conditional steps: the same residue as the definition's fold of the unreduced index), tested
// against the limit, and accumulated as int32 sums and 32 x 32 + 64-bit multiply-adds per lane.  PLANE = false carries none of it.
//
// LayerSampler<NL, STEREO> (topog_layers_kernel; "Layered topography"): every sample is offered to the layers in list order.  The
// layers are a kernel argument, so their descriptors arrive in scalar registers; the kernel is instantiated per number of layers and
// the loop over them is unrolled (no indexed copy of the argument, and a short list stays in registers), and kind and dtype are
// uniform over the wavefront.  A projected layer costs a sample two sincos, one division and the two short series of ogg_math.h; a
// sample that fails the gate costs one compare.  The refinement of a cell takes the layers' corner projections: lane 16 c + 4 k + p
// projects corner p of supergrid cell c in layer k, so the up to 64 projections of an output cell run side by side, and shuffles
// within the 16 lanes of a cell reduce them to its R.
#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>
#include <vector>

#include "ogg_common.h"
#include "ogg_math.h"

namespace {

constexpr int TT = 64;        // threads per workgroup: one wavefront
constexpr int TR = 4;         // output cells per take from the counter
constexpr int RMAX = OGG_TOPOG_MAX_REFINE;

constexpr int MAXO = OGG_TOPOG_PLANE_MAX_OFFSET;

static_assert(sizeof(ogg_topog_record) == 56, "ogg_topog_record layout");
static_assert(sizeof(ogg_topog_plane_record) == 120, "ogg_topog_plane_record layout");

struct Src {
    const void* data;
    int dtype;
    int fill0, fill1;   // int16 fill values as integers (INT_MIN: none, or a fill that no int16 equals); int32 sources: unused
    int wet_q;          // (double)q < wet_below  <=>  q < wet_q = ceil(wet_below) for an integer q (clamped to the int range)
    long Nx, Ny;
    double lon0, lat0, inv_dlon, inv_dlat, dlon, dlat;
    bool periodic;
};

struct Geo {
    const double *x, *y, *x_next, *y_next;
    long nx, nxp, j0, n, m0, nxo, total;
    int shift, refine;
    double oversample;
};

// one supergrid cell, set up once per output cell
struct Cell {
    double L00, L01, L10, L11, y00, y01, y10, y11;
    int R, pole;   // pole: 0, -1 south, +1 north
    int clamped, valid;
};

// x mod 360 with numpy's % semantics (the result takes the sign of the divisor; an exact zero is +0)
OGG_DEV double mod360(double x) {
    double m = fmod(x, 360.0);
    if (m != 0.0) {
        if (m < 0.0) m += 360.0;
    } else {
        m = 0.0;
    }
    return m;
}

OGG_DEV double wrap180(double d) { return mod360(d + 180.0) - 180.0; }

// the geometry of supergrid cell (j, i) of the band: corners with unwrapped longitudes, the pole test, R as the band fixes it (0: not)
OGG_DEV Cell cell_geometry(const Geo& g, long j, long i) {
    Cell c;
    c.valid = 1;
    const long r = j - g.j0;   // 0 .. n - 1
    const double* x0 = g.x + r * g.nxp;
    const double* y0 = g.y + r * g.nxp;
    const double* x1 = (r + 1 < g.n) ? g.x + (r + 1) * g.nxp : g.x_next;
    const double* y1 = (r + 1 < g.n) ? g.y + (r + 1) * g.nxp : g.y_next;
    const double x00 = x0[i], x01 = x0[i + 1], x10 = x1[i], x11 = x1[i + 1];
    c.y00 = y0[i], c.y01 = y0[i + 1], c.y10 = y1[i], c.y11 = y1[i + 1];
    const double l00 = x00 + wrap180(x00 - x00), l01 = x00 + wrap180(x01 - x00), l10 = x00 + wrap180(x10 - x00),
                 l11 = x00 + wrap180(x11 - x00);
    const double pl = 90.0 - OGG_TOPOG_POLE_EPS;
    c.L00 = fabs(c.y00) >= pl ? l01 : l00;
    c.L01 = fabs(c.y01) >= pl ? l00 : l01;
    c.L10 = fabs(c.y10) >= pl ? l11 : l10;
    c.L11 = fabs(c.y11) >= pl ? l10 : l11;
    c.R = g.refine, c.clamped = 0;
    const double w = wrap180(c.L01 - c.L00) + wrap180(c.L11 - c.L01) + wrap180(c.L10 - c.L11) + wrap180(c.L00 - c.L10);
    c.pole = fabs(w) > 180.0 ? ((c.y00 + c.y01 + c.y10 + c.y11 > 0.0) ? 1 : -1) : 0;
    return c;
}

// v of the header's "refine" for a lat-lon raster of spacing dlon x dlat
OGG_DEV double latlon_refine_value(const Cell& c, double dlon, double dlat, double oversample) {
    const double span_l = fmax(fmax(c.L00, c.L01), fmax(c.L10, c.L11)) - fmin(fmin(c.L00, c.L01), fmin(c.L10, c.L11));
    const double span_y = fmax(fmax(c.y00, c.y01), fmax(c.y10, c.y11)) - fmin(fmin(c.y00, c.y01), fmin(c.y10, c.y11));
    // fmax / fmin drop a NaN operand; a cell with a NaN corner has no span, and its R is clamped
    const double any = (c.L00 + c.L01) + (c.L10 + c.L11) + (c.y00 + c.y01) + (c.y10 + c.y11);
    return any != any ? any : ceil(oversample * fmax(span_l / dlon, span_y / dlat));
}

// R of a cell from its refinement value: not <= RMAX, or NaN: RMAX and clamped; below 1: 1
OGG_DEV void set_refine(Cell& c, double v) {
    if (!(v <= (double)RMAX)) {
        c.R = RMAX, c.clamped = 1;
    } else {
        c.R = v < 1.0 ? 1 : (int)v;
    }
}

// the origin of an output cell's plane fit, set up once per output cell.  valid = 0: the cell has no origin, or one so far outside
// a regional raster that every sample of it is far (the offsets below then stay within int32 whenever valid = 1)
struct Origin {
    int oI;      // periodic: (fI0 mod Nx) - (Nx div 2); regional: fI0
    int J0;      // fJ0
    int valid;
};

OGG_DEV Origin setup_origin(const Geo& g, const Src& s, long m, long io) {
    Origin o{0, 0, 0};
    const long jp = g.shift ? 2 * m + 1 : m, ip = g.shift ? 2 * io + 1 : io;   // a model cell's centre, a supergrid cell's P00
    const long r = jp - g.j0;                                                  // 0 .. n: n is the row that follows the band
    const double xO = (r < g.n ? g.x + r * g.nxp : g.x_next)[ip], yO = (r < g.n ? g.y + r * g.nxp : g.y_next)[ip];
    if (!(fabs(xO) < INFINITY && fabs(yO) < INFINITY)) return o;
    double fJ0 = floor((yO - s.lat0) * s.inv_dlat);
    const double dNx = (double)s.Nx, dNy = (double)s.Ny;
    if (s.periodic) {
        const double fI0 = floor((xO - s.lon0) * s.inv_dlon);
        if (!(fabs(fI0) < 4.0e15)) return o;
        double rI = fI0 - dNx * floor(fI0 * (1.0 / dNx));   // fI0 mod Nx, as the samples' fold
        rI = rI < 0.0 ? rI + dNx : rI;
        rI = rI >= dNx ? rI - dNx : rI;
        fJ0 = fJ0 < 0.0 ? 0.0 : (fJ0 > dNy - 1.0 ? dNy - 1.0 : fJ0);
        o.oI = (int)rI - (int)(s.Nx >> 1);
    } else {
        // a sample's indices lie in [0, 2^30): an origin index outside [-2^16, 2^30 + 2^16) puts every one of them beyond the limit
        const double fI0 = floor(mod360(xO - s.lon0) * s.inv_dlon);
        const double lo = -65536.0, hi = 1073741824.0 + 65536.0;
        if (!(fI0 >= lo && fI0 < hi && fJ0 >= lo && fJ0 < hi)) return o;
        o.oI = (int)fI0;
    }
    o.J0 = (int)fJ0;
    o.valid = 1;
    return o;
}

// the raster element (is, js) of a sample of a lat-lon source, by the index rules of the header; true when the sample is MISSING (no
// index is formed, or it lies outside a regional raster): is, js are then in range but mean nothing
OGG_DEV bool latlon_index(const Src& s, int pole, double lon, double lat, int& is, int& js) {
    const long Nx = s.Nx, Ny = s.Ny;
    const double dNx = (double)Nx, dNy = (double)Ny, inv_Nx = 1.0 / dNx;
    bool miss = false;
    if (s.periodic) {
        const double fi = floor((lon - s.lon0) * s.inv_dlon);
        // fi mod Nx without an integer division: fi is an integral double (|fi| < 2^52 below), so fi - Nx * floor(fi / Nx),
        // taken with the reciprocal and set right by one step either way, is exact
        miss = !(fabs(fi) < 4.0e15);   // a longitude that is not finite (or beyond any grid): no index is formed from it
        double r = miss ? 0.0 : fi - dNx * floor(fi * inv_Nx);
        r = r < 0.0 ? r + dNx : r;
        r = r >= dNx ? r - dNx : r;
        is = (int)r;
    } else {
        // a regional raster is met on its own longitude branch: d = (lon - lon0) mod 360 before the range test.  A d already in
        // [0, 360) is left as it is; one turn below or above, mod360(d) is d + 360 or d - 360 bit for bit (fmod(d, 360) = d for
        // |d| < 360 and = d - 360, exactly, for 360 <= d < 720), so only a grid stated further away pays the fmod
        double d = lon - s.lon0;
        if (!(d >= 0.0 && d < 360.0)) d = (d < 0.0 && d >= -360.0) ? d + 360.0 : ((d >= 360.0 && d < 720.0) ? d - 360.0 : mod360(d));
        const double fi = floor(d * s.inv_dlon);
        miss = !(fi >= 0.0 && fi < dNx);   // NaN (a longitude that is not finite) included
        is = miss ? 0 : (int)fi;
    }
    if (pole != 0) {
        js = pole < 0 ? 0 : (int)(Ny - 1);
    } else {
        double fj = floor((lat - s.lat0) * s.inv_dlat);
        if (s.periodic && fabs(fj) < INFINITY) {   // a latitude that is not finite is MISSING, not clamped
            fj = fj < 0.0 ? 0.0 : (fj > dNy - 1.0 ? dNy - 1.0 : fj);
        } else if (!(fj >= 0.0 && fj < dNy)) {
            miss = true, fj = 0.0;
        }
        js = (int)fj;
    }
    return miss;
}

// element (is, js) of a raster of int16 (with its fills) or int32 (with OGG_TOPOG_MISSING_Q) as an integer; true when it is MISSING.
// dtype is s.dtype, handed over apart so that a caller that knows it at compile time says so
OGG_DEV bool raster_value(const Src& s, int dtype, int is, int js, int& v) {
    if (dtype == OGG_TOPOG_INT16) {
        v = static_cast<const short*>(s.data)[(long)js * s.Nx + is];
        return v == s.fill0 || v == s.fill1;
    }
    v = static_cast<const int*>(s.data)[(long)js * s.Nx + is];
    return v == OGG_TOPOG_MISSING_Q;
}

// what a lane keeps of the samples it takes
struct Acc {
    int n, nm, nw, mn, mx;
    long long sum, sumsq;
};

OGG_DEV void count_valid(Acc& acc, int q, int wet_q) {
    acc.n += 1;
    acc.nw += q < wet_q ? 1 : 0;
    acc.sum += q;
    acc.sumsq += (long long)q * q;
    acc.mn = q < acc.mn ? q : acc.mn;
    acc.mx = q > acc.mx ? q : acc.mx;
}

OGG_DEV void count_missing(Acc& acc) { acc.nm += 1; }

OGG_DEV long long wave_sum(long long v) {
    for (int o = TT / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, TT);
    return v;
}
OGG_DEV int wave_sum(int v) {
    for (int o = TT / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, TT);
    return v;
}
OGG_DEV int wave_min(int v) {
    for (int o = TT / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, TT));
    return v;
}
OGG_DEV int wave_max(int v) {
    for (int o = TT / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, TT));
    return v;
}

// the position of sample (a, b) of supergrid cell c, S and U the tables of c.R: the one place a sample's position is formed
OGG_DEV void sample_position(const Cell& c, const double* S, const double* U, int a, int b, double& lon, double& lat) {
    const double sa = S[a], ua = U[a];
    lat = 0.0;
    if (c.pole == 0) {
        const double tb = S[b], vb = U[b];
        const double w00 = ua * vb, w01 = sa * vb, w10 = ua * tb, w11 = sa * tb;
        lon = w00 * c.L00 + w01 * c.L01 + w10 * c.L10 + w11 * c.L11;
        lat = w00 * c.y00 + w01 * c.y01 + w10 * c.y10 + w11 * c.y11;
    } else {
        lon = c.L00 + 360.0 * sa;
    }
}

// a lane's share of the R x R samples of supergrid cell c: their positions, each handed to the sampler
template <class Sampler>
OGG_DEV void sample_cell(Sampler& sm, const Cell& c, const double* S, const double* U, int lane, Acc& acc) {
    const int R = c.R;
    const int RR = R * R;
    int f = lane;
    if (f >= RR) return;
    int a = f % R, b = f / R;
    const int step_b = TT / R, step_a = TT % R;
    for (; f < RR; f += TT) {
        double lon, lat;
        sample_position(c, S, U, a, b, lon, lat);
        sm.sample(c, lon, lat, acc);
        a += step_a, b += step_b;
        if (a >= R) a -= R, b += 1;
    }
}

// The walk.  A Sampler has
//   lane_refine(g, cl)            R of supergrid cell cl by the lane that sets it up, where one lane can tell
//   stage(g, m, io, lane)         what the sampler keeps in LDS for output cell (m, io), before the barrier that publishes cells[]
//   begin(g, cells, side, lane)   after it: R of the cells where that takes the wavefront (then closed by a barrier of the sampler's
//                                 own), and the lane's state for the output cell
//   sample(c, lon, lat, acc)      one sample of supergrid cell c at (lon, lat), or at lon alone where c encloses a pole, counted in acc
//   finish(c, r, lane)            the record of output cell c; r, its base, is the same in every lane
template <class Sampler>
OGG_DEV void topog_walk(const Geo& g, unsigned long long* counter, Sampler& sm) {
    __shared__ double S[RMAX], U[RMAX];
    __shared__ Cell cells[4];
    __shared__ long long take;
    const int lane = threadIdx.x;
    int table_R = 0;
    const int side = 1 << g.shift;
    for (;;) {
        if (lane == 0) take = (long long)atomicAdd(counter, (unsigned long long)TR);
        __syncthreads();
        const long long c0 = take;
        __syncthreads();
        if (c0 >= g.total) break;
        const long long c1 = c0 + TR < g.total ? c0 + TR : g.total;
        for (long long c = c0; c < c1; ++c) {
            const long m = g.m0 + (long)(c / g.nxo), io = (long)(c % g.nxo);
            if (lane < side * side) {   // lane = 2 dj + di
                const long j = (m << g.shift) + (lane >> 1), i = (io << g.shift) + (lane & 1);
                Cell cl;
                if (j >= g.j0 && j < g.j0 + g.n) {
                    cl = cell_geometry(g, j, i);
                    sm.lane_refine(g, cl);
                } else {
                    cl.valid = 0, cl.R = 0, cl.pole = 0, cl.clamped = 0;
                }
                cells[lane] = cl;
            }
            sm.stage(g, m, io, lane);
            __syncthreads();
            sm.begin(g, cells, side, lane);
            Acc acc{0, 0, 0, INT_MAX, INT_MIN, 0, 0};
            int Rmax = 0, n_pole = 0, n_clamped = 0;
            for (int k = 0; k < side * side; ++k) {
                const Cell cl = cells[k];
                if (!cl.valid) continue;
                Rmax = cl.R > Rmax ? cl.R : Rmax;
                n_pole += cl.pole != 0;
                n_clamped += cl.clamped;
                if (cl.R != table_R) {   // s = (a + 0.5) / R and 1 - s for this R
                    __syncthreads();
                    for (int a = lane; a < cl.R; a += TT) {
                        const double sv = ((double)a + 0.5) / (double)cl.R;
                        S[a] = sv, U[a] = 1.0 - sv;
                    }
                    __syncthreads();
                    table_R = cl.R;
                }
                sample_cell(sm, cl, S, U, lane, acc);
            }
            ogg_topog_record r;
            r.n = wave_sum(acc.n), r.n_missing = wave_sum(acc.nm), r.n_wet = wave_sum(acc.nw);
            r.sum = wave_sum(acc.sum), r.sumsq = wave_sum(acc.sumsq);
            r.min = wave_min(acc.mn), r.max = wave_max(acc.mx);
            r.R = Rmax, r.n_pole = (short)n_pole, r.n_clamped = (short)n_clamped;
            sm.finish(c, r, lane);
            __syncthreads();   // cells[] is rewritten for the next output cell
        }
    }
}

// the moments of the plane fit: a lane sees at most 4 * 256 * 256 / 64 = 4096 samples of a record, |offset| <= 2^15, |q| <= 2^21
struct PAcc {
    int sx, sy, nfar;
    long long sxx, sxy, syy, sxq, syq;
};

// what a lane carries for the plane fit through the supergrid cells of one output cell.  PLANE = false: nothing -- no origin, no
// moments, no LDS behind it -- so the sampling without the plane cannot touch any of it
template <bool PLANE>
struct PlaneLane {};
template <>
struct PlaneLane<true> {
    PAcc acc;
    Origin o;       // the output cell's origin, read from LDS once
    Origin* lds;    // where lane 0 puts it
};

template <int DT, bool PLANE>
struct SingleSampler {
    using Record = std::conditional_t<PLANE, ogg_topog_plane_record, ogg_topog_record>;
    const Src& s;
    Record* out;
    PlaneLane<PLANE> pl;

    OGG_DEV void lane_refine(const Geo& g, Cell& cl) {
        if (g.refine <= 0) set_refine(cl, latlon_refine_value(cl, s.dlon, s.dlat, g.oversample));
    }
    OGG_DEV void stage(const Geo& g, long m, long io, int lane) {
        if constexpr (PLANE) {
            if (lane == 0) *pl.lds = setup_origin(g, s, m, io);
        }
    }
    OGG_DEV void begin(const Geo&, Cell*, int, int) {
        if constexpr (PLANE) pl.acc = PAcc{0, 0, 0, 0, 0, 0, 0, 0}, pl.o = *pl.lds;
    }
    OGG_DEV void sample(const Cell& c, double lon, double lat, Acc& acc) {
        int is, js, q;
        bool miss = latlon_index(s, c.pole, lon, lat, is, js);
        if (!miss) miss = raster_value(s, DT, is, js, q);
        if (miss) {
            count_missing(acc);
            return;
        }
        count_valid(acc, q, s.wet_q);
        if constexpr (PLANE) {
            // The definition forms the offsets as integral doubles and tests them against the limit before any cast.  Here
            // they are int32 differences, which is the same test: is, js and Nx, Ny lie in [0, 2^30) (check_source), a
            // periodic origin is a residue in [0, Nx) less Nx div 2 and its row is clamped to [0, Ny), and a regional origin
            // is admitted (valid) only in [-2^16, 2^30 + 2^16), so every difference and every step of the fold below stays
            // within +-(2^31 - 1); an origin outside that gate is more than 2^15 from every sample, which far_cell says.
            // With |dI|, |dJ| < 2^31 - 2^15 the unsigned compare of d + 2^15 against 2^16 is |d| > 2^15.
            const Origin& o = pl.o;
            PAcc& pacc = pl.acc;
            const bool far_cell = !o.valid || c.pole != 0;   // no origin, or a pole-enclosing cell (no latitude): every valid sample is far
            const int Nx = (int)s.Nx;
            int dI = is - o.oI;
            if (s.periodic) {   // ((fi - fI0 + hN) mod Nx) - hN from the two residues
                dI += dI < 0 ? Nx : 0;
                dI -= dI >= Nx ? Nx : 0;
                dI -= (int)(s.Nx >> 1);
            }
            const int dJ = js - o.J0;
            const bool far = far_cell || (unsigned)(dI + MAXO) > 2u * MAXO || (unsigned)(dJ + MAXO) > 2u * MAXO;
            const int eI = far ? 0 : dI, eJ = far ? 0 : dJ, eq = far ? 0 : q;
            pacc.nfar += far ? 1 : 0;
            pacc.sx += eI, pacc.sy += eJ;
            pacc.sxx += (long long)eI * eI, pacc.sxy += (long long)eI * eJ, pacc.syy += (long long)eJ * eJ;
            pacc.sxq += (long long)eI * eq, pacc.syq += (long long)eJ * eq;
        }
    }
    OGG_DEV void finish(long long c, const ogg_topog_record& r, int lane) {
        if constexpr (PLANE) {
            const PAcc& a = pl.acc;
            ogg_topog_plane_record p;   // the wavefront's moments; a lane's sums of offsets fit int32, the wavefront's need not
            p.base = r;
            p.sx = wave_sum((long long)a.sx), p.sy = wave_sum((long long)a.sy), p.n_far = wave_sum(a.nfar);
            p.sxx = wave_sum(a.sxx), p.sxy = wave_sum(a.sxy), p.syy = wave_sum(a.syy);
            p.sxq = wave_sum(a.sxq), p.syq = wave_sum(a.syq);
            if (lane == 0) out[c] = p;
        } else {
            if (lane == 0) out[c] = r;
        }
    }
};

template <int DT, bool PLANE>
__global__ __launch_bounds__(TT) void topog_band_kernel(Geo g, Src s, unsigned long long* counter, void* records) {
    SingleSampler<DT, PLANE> sm{s, static_cast<typename SingleSampler<DT, PLANE>::Record*>(records), {}};
    if constexpr (PLANE) {
        __shared__ Origin origin;
        sm.pl.lds = &origin;
    }
    topog_walk(g, counter, sm);
}

// ---- face topography (include/ogg_hip.h, "Face topography") ---------------------------------------------------------------------
// One wavefront per workgroup owns each face record and takes runs of TR faces of one family from a counter in the workspace, as the
// walk does.  Lanes 0 .. 3 set up the block's cells (lane = 2 d + side: d the line group dj or di, side 0 west / south, 1 east /
// north) with the walk's cell_geometry and refine rule; the block's R is their largest, and every present cell is walked at that R
// with the walk's sample_position, lane l taking the flattened samples f = b R + a = l, l + 64, ..., so consecutive lanes are
// consecutive a (along a raster row).  The ridge of line k lives in LDS (ridge[d R + k], INT_MIN: no sample yet) and takes every
// sample by an LDS integer max, exact in any order.  On a u face consecutive lanes share a line (b), and 64 lanes would hit a few LDS
// addresses: the run of equal b among the 64 samples of a step is first reduced across lanes by a segmented scan (shuffles by 1, 2,
// 4, .. below min(R, 64); lane - o lies in the same run exactly when a >= o), and the last lane of each run alone goes to LDS.  On a
// v face consecutive lanes are consecutive lines (a), and each goes to LDS itself.  After a barrier the wavefront reduces the 2 R
// lines with shuffles and lane 0 stores the record.  No atomic touches global memory but the work counter.
// the record as the header lays it out in OGG_TOPOG_FACE_WORDS int64 words (little-endian), and the call's parameters
struct FaceRecord {
    long long n, n_missing, ridge_sum;
    int n_lines, n_lines_missing, n_dry_lines, lo, hi, q_min, R;
    short n_clamped, flags;
};
static_assert(sizeof(FaceRecord) == 8 * OGG_TOPOG_FACE_WORDS && alignof(FaceRecord) == 8, "face record layout");
struct FaceParams {
    long nx, ny, ld;
    const double *x, *y;
    int topology, refine;
    double oversample;
    long ju0, ju1, jv0, jv1;
};

struct Faces {
    long nxm, nym, nx, ny;
    long r0, per_row, total;   // the first output row, faces per row, faces of this launch
    int periodic, fold;
};

// supergrid cell k = 2 d + side of the block of face (row, col) (a u face (jm, I) or a v face (J, im)): false when that side is
// absent; rev: the fold partner, whose lines are read reversed
template <bool VFACE>
OGG_DEV bool face_cell(const Faces& fc, long row, long col, int k, long& j, long& i, bool& partner) {
    const int d = k >> 1, side = k & 1;
    partner = false;
    if (!VFACE) {
        j = 2 * row + d;
        i = 2 * col - 1 + side;
        if (side == 0 && col == 0) i = fc.nx - 1, partner = true;
        if (side == 1 && col == fc.nxm) i = 0, partner = true;
        return !partner || fc.periodic;
    }
    i = 2 * col + d;
    j = 2 * row - 1 + side;
    if (side == 0 && row == 0) return false;
    if (side == 1 && row == fc.nym) {
        j = fc.ny - 1, i = fc.nx - 1 - i, partner = true;
        return fc.fold != 0;
    }
    return true;
}

template <int DT, bool VFACE>
__global__ __launch_bounds__(TT) void topog_faces_kernel(Geo g, Src s, Faces fc, unsigned long long* counter, FaceRecord* out) {
    __shared__ double S[RMAX], U[RMAX];
    __shared__ Cell cells[4];
    __shared__ int ridge[2 * RMAX];
    __shared__ long long take;
    const int lane = threadIdx.x;
    int table_R = 0;
    for (;;) {
        if (lane == 0) take = (long long)atomicAdd(counter, (unsigned long long)TR);
        __syncthreads();
        const long long c0 = take;
        __syncthreads();
        if (c0 >= fc.total) break;
        const long long c1 = c0 + TR < fc.total ? c0 + TR : fc.total;
        for (long long c = c0; c < c1; ++c) {
            const long row = fc.r0 + (long)(c / fc.per_row), col = (long)(c % fc.per_row);
            if (lane < 4) {
                long j, i;
                bool partner;
                Cell cl;
                if (face_cell<VFACE>(fc, row, col, lane, j, i, partner)) {
                    cl = cell_geometry(g, j, i);
                    if (g.refine <= 0) set_refine(cl, latlon_refine_value(cl, s.dlon, s.dlat, g.oversample));
                } else {
                    cl.valid = 0, cl.R = 0, cl.pole = 0, cl.clamped = 0;
                }
                cells[lane] = cl;
            }
            __syncthreads();
            int R = 0, n_pole = 0, n_clamped = 0, n_present = 0;
            for (int k = 0; k < 4; ++k) {
                const Cell& cl = cells[k];
                if (!cl.valid) continue;
                R = cl.R > R ? cl.R : R;
                n_pole += cl.pole != 0, n_clamped += cl.clamped, n_present += 1;
            }
            // the flags, from the face's place alone
            int flags = n_present < 4 ? OGG_FACE_ONE_SIDED : 0;
            if (!VFACE && (col == 0 || col == fc.nxm) && fc.periodic) flags |= OGG_FACE_SEAM;
            const bool on_fold = VFACE && row == fc.nym && fc.fold;
            if (on_fold) flags |= OGG_FACE_FOLD;
            if (n_pole) flags |= OGG_FACE_POLE;
            if (R != table_R) {   // s = (a + 0.5) / R and 1 - s for this R; the barrier above closed the last face's reads
                for (int a = lane; a < R; a += TT) {
                    const double sv = ((double)a + 0.5) / (double)R;
                    S[a] = sv, U[a] = 1.0 - sv;
                }
                table_R = R;
            }
            for (int k = lane; k < 2 * R; k += TT) ridge[k] = INT_MIN;
            __syncthreads();
            int n = 0, nm = 0, qmin = INT_MAX;
            const int RR = R * R;
            int scan_top = R < TT ? R : TT;   // the scan's shifts stay below the longest run of a step
            for (int k = 0; k < 4 && !n_pole; ++k) {
                Cell cl = cells[k];
                if (!cl.valid) continue;
                cl.R = R;
                const int d = k >> 1;
                const bool rev = on_fold && (k & 1);
                int a = lane % R, b = lane / R;
                const int step_b = TT / R, step_a = TT % R;
                for (int f0 = 0; f0 < RR; f0 += TT) {   // the same trips in every lane: the shuffles below need them all
                    const bool live = f0 + lane < RR;
                    int q = INT_MIN;
                    if (live) {
                        double lon, lat;
                        sample_position(cl, S, U, a, b, lon, lat);
                        int is, js, v;
                        bool miss = latlon_index(s, 0, lon, lat, is, js);
                        if (!miss) miss = raster_value(s, DT, is, js, v);
                        n += miss ? 0 : 1, nm += miss ? 1 : 0;
                        if (!miss) q = v, qmin = v < qmin ? v : qmin;
                    }
                    if (VFACE) {
                        if (q != INT_MIN) atomicMax(&ridge[d * R + (rev ? R - 1 - a : a)], q);
                    } else {
                        for (int o = 1; o < scan_top; o <<= 1) {
                            const int up = __shfl_up(q, o, TT);
                            if (lane >= o && a >= o) q = up > q ? up : q;
                        }
                        const bool last = lane == TT - 1 || a == R - 1;   // of its run in this step (a dead lane's q is INT_MIN)
                        if (live && last && q != INT_MIN) atomicMax(&ridge[d * R + b], q);
                    }
                    a += step_a, b += step_b;
                    if (a >= R) a -= R, b += 1;
                }
            }
            __syncthreads();
            int nl = 0, nlm = 0, ndry = 0, lo = INT_MAX, hi = INT_MIN;
            long long rsum = 0;
            for (int k = lane; k < 2 * R && !n_pole; k += TT) {
                const int r = ridge[k];
                const bool ok = r != INT_MIN;
                nl += ok ? 1 : 0, nlm += ok ? 0 : 1;
                ndry += ok && !(r < s.wet_q) ? 1 : 0;
                lo = ok && r < lo ? r : lo, hi = r > hi ? r : hi;
                rsum += ok ? r : 0;
            }
            FaceRecord r;
            r.n = wave_sum((long long)n), r.n_missing = wave_sum((long long)nm), r.ridge_sum = wave_sum(rsum);
            r.n_lines = wave_sum(nl), r.n_lines_missing = wave_sum(nlm), r.n_dry_lines = wave_sum(ndry);
            r.lo = wave_min(lo), r.hi = wave_max(hi), r.q_min = wave_min(qmin);
            r.R = R, r.n_clamped = (short)n_clamped, r.flags = (short)flags;
            if (lane == 0) out[c] = r;
            __syncthreads();   // cells[], ridge[] and the tables are rewritten for the next face
        }
    }
}

// ---- layered topography (include/ogg_hip.h, "Layered topography") ------------------------------------------------------------
constexpr int NLAY = OGG_TOPOG_MAX_SOURCES;
static_assert(NLAY == 4 && TT == 16 * NLAY, "one lane per (supergrid cell, layer, corner)");
static_assert(sizeof(ogg_topog_merge_record) == 88, "ogg_topog_merge_record layout");

struct Layer {
    Src s;   // a projected layer: lon0, lat0, inv_dlon, inv_dlat, dlon, dlat hold X0, Y0, 1 / dX, 1 / dY, dX, dY; periodic is false
    int kind, q_mul;
    double h, plon0, e, K, gate;
};
struct Layers {
    int n;
    Layer l[NLAY];
};

// X, Y of the header's projection; false (and nothing stored) when the point is not finite or fails the gate
OGG_DEV bool stereo_project(const Layer& L, double lon, double lat, double& X, double& Y) {
    if (!(fabs(lon) < INFINITY && fabs(lat) < INFINITY)) return false;
    const double hl = L.h * lat;
    if (!(hl >= L.gate)) return false;
    if (hl >= 90.0 - OGG_TOPOG_POLE_EPS) {
        X = 0.0, Y = 0.0;
        return true;
    }
    const double phi = hl * ogg::kPi180, lam = L.h * (lon - L.plon0) * ogg::kPi180;
    double sp, cp, sl, cl;
    sincos(phi, &sp, &cp);
    sincos(lam, &sl, &cl);
    double rho = (L.K * cp) / (1.0 + sp);
    if (L.e != 0.0) rho = rho * ogg::exp_small(L.e * ogg::atanh_small(L.e * sp));   // e = 0: the factor is exp(+0) = 1, which changes no bit
    X = L.h * (rho * sl), Y = -L.h * (rho * cl);
    return true;
}

// the raster element of a sample in a projected layer; true when the sample is MISSING in it (gated, or outside the raster)
OGG_DEV bool stereo_index(const Layer& L, int pole, double lon, double lat, int& is, int& js) {
    double X, Y;
    if (!stereo_project(L, lon, pole != 0 ? 90.0 * (double)pole : lat, X, Y)) return true;
    const double fi = floor((X - L.s.lon0) * L.s.inv_dlon), fj = floor((Y - L.s.lat0) * L.s.inv_dlat);
    if (!(fi >= 0.0 && fi < (double)L.s.Nx && fj >= 0.0 && fj < (double)L.s.Ny)) return true;
    is = (int)fi, js = (int)fj;
    return false;
}

// the value of a sample in one layer (times q_mul); true when it is MISSING there.  STEREO = false: the list has no projected layer
template <bool STEREO>
OGG_DEV bool layer_value(const Layer& L, int pole, double lon, double lat, int& q) {
    int is = 0, js = 0;
    const bool miss =
        (!STEREO || L.kind == OGG_TOPOG_LATLON) ? latlon_index(L.s, pole, lon, lat, is, js) : stereo_index(L, pole, lon, lat, is, js);
    if (miss) return true;   // is, js of a missing sample mean nothing: nothing is read
    int v;
    if (raster_value(L.s, L.s.dtype, is, js, v)) return true;
    q = v * L.q_mul;   // |q| <= OGG_TOPOG_MAX_Q: ogg_topog_layer_range_dev
    return false;
}

// shuffles within aligned groups of W lanes (W = 4: the corners of one layer; W = 16: the layers of one supergrid cell)
template <int W>
OGG_DEV double group_max(double v) {
    for (int o = W / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, TT));
    return v;
}

// v_k of the header's "refine" for the layer and corner of this lane (every lane of a group of four returns the layer's value):
// cl is the lane's supergrid cell (geometry only), lon and lat its corner (L, y)
template <bool STEREO>
OGG_DEV double layer_refine_value(const Layer& L, const Cell& cl, double lon, double lat, double oversample) {
    if (!STEREO || L.kind == OGG_TOPOG_LATLON) return latlon_refine_value(cl, L.s.dlon, L.s.dlat, oversample);
    double X = 0.0, Y = 0.0;
    const bool counts = stereo_project(L, lon, lat, X, Y);
    const double fi = floor((X - L.s.lon0) * L.s.inv_dlon), fj = floor((Y - L.s.lat0) * L.s.inv_dlat);
    const bool inside = counts && fi >= 0.0 && fi < (double)L.s.Nx && fj >= 0.0 && fj < (double)L.s.Ny;
    const double ninf = -INFINITY;   // a corner that does not count takes no part in a maximum
    const double xmax = group_max<4>(counts ? X : ninf), xmin = -group_max<4>(counts ? -X : ninf);
    const double ymax = group_max<4>(counts ? Y : ninf), ymin = -group_max<4>(counts ? -Y : ninf);
    const bool any_inside = group_max<4>(inside ? 1.0 : 0.0) > 0.0;
    return any_inside ? ceil(oversample * fmax((xmax - xmin) / L.s.dlon, (ymax - ymin) / L.s.dlat)) : 1.0;
}

// NL: the number of layers, so that a short list keeps its descriptors in scalar registers through the sample loop.  STEREO: whether
// any layer is projected; a list of lat-lon layers alone carries none of the projection's code or registers
template <int NL, bool STEREO>
struct LayerSampler {
    const Layers& ly;
    ogg_topog_merge_record* out;
    int from[NLAY];   // the samples each layer gave this lane

    OGG_DEV void lane_refine(const Geo&, Cell&) {}
    OGG_DEV void stage(const Geo&, long, long, int) {}
    OGG_DEV void begin(const Geo& g, Cell* cells, int side, int lane) {
        if (g.refine <= 0) {   // R from the layers: lane = 16 cell + 4 layer + corner
            const int ci = lane >> 4, k = (lane >> 2) & 3, p = lane & 3;
            const Cell& cl = cells[ci < side * side ? ci : 0];
            const bool live = ci < side * side && cl.valid;
            const double lon = (&cl.L00)[p], lat = (&cl.y00)[p];   // L00, L01, L10, L11 and y00 .. y11 lie in this order
            double v = 1.0;   // a layer that is not there asks for nothing
#pragma unroll
            for (int kk = 0; kk < NL; ++kk) {   // every lane takes part in the shuffles of every layer; it keeps its own layer's value
                const double vk = layer_refine_value<STEREO>(ly.l[kk], cl, lon, lat, g.oversample);
                v = kk == k ? vk : v;
            }
            const bool nan = group_max<16>(v != v ? 1.0 : 0.0) > 0.0;   // fmax drops a NaN, so it is carried apart
            const double vmax = group_max<16>(v != v ? 1.0 : v);
            if (live && (lane & 15) == 0) set_refine(cells[ci], nan ? (double)NAN : vmax);
            __syncthreads();
        }
        for (int k = 0; k < NLAY; ++k) from[k] = 0;
    }
    OGG_DEV void sample(const Cell& c, double lon, double lat, Acc& acc) {
        bool miss = true;
        int q = 0;
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            if (miss) {
                miss = layer_value<STEREO>(ly.l[k], c.pole, lon, lat, q);
                from[k] += miss ? 0 : 1;
            }
        }
        if (!miss) {
            count_valid(acc, q, ly.l[0].s.wet_q);
        } else {
            count_missing(acc);
        }
    }
    OGG_DEV void finish(long long c, const ogg_topog_record& r, int lane) {
        const int f0 = wave_sum(from[0]), f1 = wave_sum(from[1]), f2 = wave_sum(from[2]), f3 = wave_sum(from[3]);
        if (lane == 0) {
            out[c].base = r;
            out[c].n_from[0] = f0, out[c].n_from[1] = f1, out[c].n_from[2] = f2, out[c].n_from[3] = f3;
        }
    }
};

template <int NL, bool STEREO>
__global__ __launch_bounds__(TT) void topog_layers_kernel(Geo g, Layers ly, unsigned long long* counter, ogg_topog_merge_record* out) {
    LayerSampler<NL, STEREO> sm{ly, out, {}};
    topog_walk(g, counter, sm);
}

// |q_mul * q| <= OGG_TOPOG_MAX_Q of every stored value (DT: INT16 with its fills, INT32 with OGG_TOPOG_MISSING_Q)
template <typename T>
__global__ void topog_range_kernel(const T* v, long n, int fill0, int fill1, int q_mul, int* n_bad) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const int q = v[k];
        const bool missing = sizeof(T) == 2 ? (q == fill0 || q == fill1) : q == OGG_TOPOG_MISSING_Q;
        const long long p = (long long)q * q_mul;
        if (!missing && (p > OGG_TOPOG_MAX_Q || p < -(long long)OGG_TOPOG_MAX_Q)) *n_bad = 1;   // every writer stores the same value
    }
}

__global__ void topog_project_kernel(Layer L, long n, const double* lon, const double* lat, double* X, double* Y, int* gate_ok) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double x = 0.0, y = 0.0;
    const bool ok = stereo_project(L, lon[k], lat[k], x, y);
    X[k] = ok ? x : 0.0, Y[k] = ok ? y : 0.0, gate_ok[k] = ok ? 1 : 0;
}

template <typename T>
__global__ void topog_quantize_kernel(const T* v, long n, double quantum, int n_fill, double f0, double f1, int* q, int* n_bad) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const double d = (double)v[k];
        int out = OGG_TOPOG_MISSING_Q;
        if (!(d != d) && !(n_fill > 0 && d == f0) && !(n_fill > 1 && d == f1)) {
            const double r = rint(d / quantum);
            if (!(fabs(r) <= (double)OGG_TOPOG_MAX_Q)) {
                *n_bad = 1;   // every writer stores the same value
            } else {
                out = (int)r;
            }
        }
        q[k] = out;
    }
}

int check_source(const ogg_topog_source& s, bool sampled) {
    OGG_REQUIRE(s.Nx >= 1 && s.Ny >= 1 && s.Nx < (1L << 30) && s.Ny < (1L << 30), OGG_ESHAPE, "ogg_topog: source of %ld x %ld", s.Ny,
                s.Nx);
    OGG_REQUIRE(s.dlon > 0.0 && s.dlat > 0.0, OGG_EARG, "ogg_topog: dlon and dlat must be positive (%g, %g)", s.dlon, s.dlat);
    OGG_REQUIRE(s.n_fill >= 0 && s.n_fill <= 2, OGG_EARG, "ogg_topog: n_fill = %d", s.n_fill);
    OGG_REQUIRE(s.data, OGG_EARG, "ogg_topog: null source data");
    if (sampled)
        OGG_REQUIRE(s.dtype == OGG_TOPOG_INT16 || s.dtype == OGG_TOPOG_INT32, OGG_EARG,
                    "ogg_topog_band: source dtype %d: quantise a float source first (ogg_topog_quantize_dev)", s.dtype);
    else
        OGG_REQUIRE(s.dtype >= OGG_TOPOG_INT16 && s.dtype <= OGG_TOPOG_FLOAT64, OGG_EARG, "ogg_topog: source dtype %d", s.dtype);
    if (s.dtype >= OGG_TOPOG_FLOAT32)
        OGG_REQUIRE(s.quantum > 0.0 && std::isfinite(s.quantum), OGG_EARG, "ogg_topog: quantum must be positive (%g)", s.quantum);
    return OGG_OK;
}

int check_band(const ogg_topog_band& b) {
    OGG_REQUIRE(b.nx >= 1 && b.j0 >= 0 && b.n_cell_rows >= 0, OGG_ESHAPE, "ogg_topog_band: nx %ld, j0 %ld, %ld rows", b.nx, b.j0,
                b.n_cell_rows);
    OGG_REQUIRE(b.cells == OGG_TOPOG_MODEL_CELLS || b.cells == OGG_TOPOG_SUPERGRID_CELLS, OGG_EARG, "ogg_topog_band: cells = %d", b.cells);
    OGG_REQUIRE(b.cells != OGG_TOPOG_MODEL_CELLS || b.nx % 2 == 0, OGG_ESHAPE,
                "ogg_topog_band: model cells need an even number of supergrid columns (nx = %ld)", b.nx);
    OGG_REQUIRE(b.refine >= 0 && b.refine <= RMAX, OGG_EARG, "ogg_topog_band: refine = %d (0 or 1 .. %d)", b.refine, RMAX);
    OGG_REQUIRE(b.refine > 0 || (b.oversample > 0.0 && std::isfinite(b.oversample)), OGG_EARG, "ogg_topog_band: oversample = %g",
                b.oversample);
    return OGG_OK;
}

// fill[k] of an int16 source as the int an int16 v must equal ((double)v == fill[k]); INT_MIN when there is none or no int16 equals it
int int16_fill(const ogg_topog_source& s, int k) {
    if (s.dtype != OGG_TOPOG_INT16 || k >= s.n_fill) return INT_MIN;
    const double f = s.fill[k];
    return (f >= -32768.0 && f <= 32767.0 && f == floor(f)) ? (int)f : INT_MIN;
}

// the integer threshold of "wet": for an integer q, q < w <=> q < ceil(w); |q| <= 2^31 - 1 bounds what matters
int wet_threshold(double w) {
    if (w != w) return INT_MIN;   // NaN: nothing is wet
    const double c = ceil(w);
    return c > 2147483647.0 ? INT_MAX : (c < -2147483647.0 ? INT_MIN + 1 : (int)c);
}

Src make_src(const ogg_topog_source& q) {
    return Src{q.data, q.dtype, int16_fill(q, 0), int16_fill(q, 1), wet_threshold(q.wet_below), q.Nx, q.Ny, q.lon0, q.lat0, 1.0 / q.dlon,
               1.0 / q.dlat, q.dlon, q.dlat, fabs((double)q.Nx * q.dlon - 360.0) <= 1e-9};
}

long out_rows(const ogg_topog_band& b) {
    if (b.n_cell_rows == 0) return 0;
    const int sh = b.cells == OGG_TOPOG_MODEL_CELLS ? 1 : 0;
    return ((b.j0 + b.n_cell_rows - 1) >> sh) - (b.j0 >> sh) + 1;
}

Geo make_geo(const ogg_topog_band& b) {
    const int shift = b.cells == OGG_TOPOG_MODEL_CELLS ? 1 : 0;
    Geo g{b.x, b.y, b.x_next, b.y_next, b.nx, b.nx + 1, b.j0, b.n_cell_rows, b.j0 >> shift, b.nx >> shift, 0, shift, b.refine,
          b.oversample};
    g.total = out_rows(b) * g.nxo;
    return g;
}

// what a launch of the walk needs first: the counter at the head of the workspace cleared, and the number of persistent workgroups
int walk_launch(const Geo& g, void* workspace, hipStream_t st, unsigned long long** counter, unsigned* wgs) {
    OGG_HIP_CHECK(hipMemsetAsync(workspace, 0, sizeof(unsigned long long), st));
    int dev = 0, n_cu = 0;
    OGG_HIP_CHECK(hipGetDevice(&dev));
    OGG_HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const long takes = (g.total + TR - 1) / TR;
    *wgs = (unsigned)std::min(takes, (long)(n_cu > 0 ? n_cu : 256) * 32);   // 32 one-wave workgroups per CU, persistent
    *counter = static_cast<unsigned long long*>(workspace);
    return OGG_OK;
}

// HOST band h as device band d: its grid rows, and the row that follows them, copied to device memory
int stage_band(ogg::Buffers& bufs, const ogg_topog_band& h, ogg_topog_band* d) {
    const long nxp = h.nx + 1, n = h.n_cell_rows;
    *d = h;
    double *px, *py;
    if (int e = bufs.alloc(&px, (size_t)(n + 1) * nxp)) return e;
    if (int e = bufs.alloc(&py, (size_t)(n + 1) * nxp)) return e;
    const size_t body = (size_t)n * nxp, row = (size_t)nxp;   // doubles
    if (int e = bufs.send(px, h.x, body)) return e;
    if (int e = bufs.send(py, h.y, body)) return e;
    if (int e = bufs.send(px + body, h.x_next ? h.x_next : h.x + n * nxp, row)) return e;
    if (int e = bufs.send(py + body, h.y_next ? h.y_next : h.y + n * nxp, row)) return e;
    d->x = px, d->y = py;
    d->x_next = d->x + n * nxp, d->y_next = d->y + n * nxp;
    return OGG_OK;
}

}  // namespace

extern "C" long ogg_topog_workspace_bytes(void) { return 256; }

extern "C" long ogg_topog_band_out_rows(const ogg_topog_band* band) {
    if (!band || band->nx < 1 || band->j0 < 0 || band->n_cell_rows < 0) return -1;
    return out_rows(*band);
}

namespace {

// ogg_topog_band_dev (out: ogg_topog_record) and ogg_topog_plane_band_dev (plane: out holds ogg_topog_plane_record)
int band_dev(const ogg_topog_band* band, const ogg_topog_source* src, void* workspace, long workspace_bytes, void* out, void* stream,
             bool plane) {
    OGG_REQUIRE(band && src, OGG_EARG, "ogg_topog_band: null pointer");
    if (int e = check_band(*band)) return e;
    if (int e = check_source(*src, true)) return e;
    const ogg_topog_band& b = *band;
    const long rows = out_rows(b);
    if (rows == 0) return OGG_OK;
    OGG_REQUIRE(b.x && b.y && b.x_next && b.y_next && out, OGG_EARG, "ogg_topog_band: null x / y / x_next / y_next / out");
    if (int e = ogg::check_workspace("ogg_topog_band", workspace, workspace_bytes, ogg_topog_workspace_bytes())) return e;
    const ogg_topog_source& q = *src;
    const Geo g = make_geo(b);
    const Src s = make_src(q);
    hipStream_t st = ogg::as_stream(stream);
    unsigned long long* counter;
    unsigned wgs;
    if (int e = walk_launch(g, workspace, st, &counter, &wgs)) return e;
    if (plane) {
        if (q.dtype == OGG_TOPOG_INT16)
            topog_band_kernel<OGG_TOPOG_INT16, true><<<wgs, TT, 0, st>>>(g, s, counter, out);
        else
            topog_band_kernel<OGG_TOPOG_INT32, true><<<wgs, TT, 0, st>>>(g, s, counter, out);
    } else {
        if (q.dtype == OGG_TOPOG_INT16)
            topog_band_kernel<OGG_TOPOG_INT16, false><<<wgs, TT, 0, st>>>(g, s, counter, out);
        else
            topog_band_kernel<OGG_TOPOG_INT32, false><<<wgs, TT, 0, st>>>(g, s, counter, out);
    }
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

}  // namespace

extern "C" int ogg_topog_band_dev(const ogg_topog_band* band, const ogg_topog_source* src, void* workspace, long workspace_bytes,
                                  ogg_topog_record* out, void* stream) {
    return band_dev(band, src, workspace, workspace_bytes, out, stream, false);
}

extern "C" int ogg_topog_plane_band_dev(const ogg_topog_band* band, const ogg_topog_source* src, void* workspace, long workspace_bytes,
                                        ogg_topog_plane_record* out, void* stream) {
    return band_dev(band, src, workspace, workspace_bytes, out, stream, true);
}

extern "C" int ogg_topog_quantize_dev(const ogg_topog_source* src, int* q, int* n_bad, void* stream) {
    OGG_REQUIRE(src && q && n_bad, OGG_EARG, "ogg_topog_quantize: null pointer");
    if (int e = check_source(*src, false)) return e;
    OGG_REQUIRE(src->dtype == OGG_TOPOG_FLOAT32 || src->dtype == OGG_TOPOG_FLOAT64, OGG_EARG,
                "ogg_topog_quantize: source dtype %d is not a float type", src->dtype);
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(n_bad, 0, sizeof(int), st));
    const long n = src->Nx * src->Ny;
    const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 65536);
    const double f0 = src->n_fill > 0 ? src->fill[0] : 0.0, f1 = src->n_fill > 1 ? src->fill[1] : 0.0;
    if (src->dtype == OGG_TOPOG_FLOAT32)
        topog_quantize_kernel<float><<<blocks, 256, 0, st>>>(static_cast<const float*>(src->data), n, src->quantum, src->n_fill, f0, f1,
                                                             q, n_bad);
    else
        topog_quantize_kernel<double><<<blocks, 256, 0, st>>>(static_cast<const double*>(src->data), n, src->quantum, src->n_fill, f0,
                                                              f1, q, n_bad);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

namespace {

// HOST raster of *s as a device one that the walk samples: copied to device memory, a float one quantised there (the descriptor is
// then int32 without fills).  *n_bad != 0: a quantised value exceeds OGG_TOPOG_MAX_Q, and the caller says so in its own words
int stage_raster(ogg::Buffers& bufs, ogg_topog_source* s, int* n_bad) {
    const long nsrc = s->Nx * s->Ny;
    const size_t esize = s->dtype == OGG_TOPOG_INT16 ? 2 : (s->dtype == OGG_TOPOG_FLOAT64 ? 8 : 4);
    char* raw;
    if (int e = bufs.put(&raw, static_cast<const char*>(s->data), (size_t)nsrc * esize)) return e;
    s->data = raw;
    *n_bad = 0;
    if (s->dtype == OGG_TOPOG_FLOAT32 || s->dtype == OGG_TOPOG_FLOAT64) {
        int *qd, *bad;
        if (int e = bufs.alloc(&qd, (size_t)nsrc)) return e;
        if (int e = bufs.alloc(&bad, 1)) return e;
        if (int e = ogg_topog_quantize_dev(s, qd, bad, nullptr)) return e;
        if (int e = bufs.get(n_bad, bad, 1)) return e;
        s->data = qd, s->dtype = OGG_TOPOG_INT32, s->n_fill = 0;
    }
    return OGG_OK;
}

// the host-pointer forms: grid rows and raster copied to device memory, one band, the records (plane records when ``plane``) copied
// back (synchronous)
int topog_host(const ogg_topog_band* band, const ogg_topog_source* src, void* out, bool plane) {
    OGG_REQUIRE(band && src && out, OGG_EARG, "ogg_topog: null pointer");
    if (int e = check_band(*band)) return e;
    if (int e = check_source(*src, false)) return e;
    const ogg_topog_band& h = *band;
    OGG_REQUIRE(h.x && h.y, OGG_EARG, "ogg_topog: null x / y");
    const long rows = out_rows(h);
    if (rows == 0) return OGG_OK;
    ogg::Buffers bufs;   // freed on every exit path
    ogg_topog_band d;
    if (int e = stage_band(bufs, h, &d)) return e;
    ogg_topog_source ds = *src;
    int nb = 0;
    if (int e = stage_raster(bufs, &ds, &nb)) return e;
    OGG_REQUIRE(nb == 0, OGG_EARG, "ogg_topog: a quantised source value exceeds %d in magnitude (quantum %g too small)", OGG_TOPOG_MAX_Q,
                ds.quantum);
    const long nrec = rows * (h.nx >> (h.cells == OGG_TOPOG_MODEL_CELLS ? 1 : 0));
    char *ws, *res;
    if (int e = bufs.alloc(&ws, (size_t)ogg_topog_workspace_bytes())) return e;
    const size_t rec_bytes = plane ? sizeof(ogg_topog_plane_record) : sizeof(ogg_topog_record);
    if (int e = bufs.alloc(&res, (size_t)nrec * rec_bytes)) return e;
    if (int e = band_dev(&d, &ds, ws, ogg_topog_workspace_bytes(), res, nullptr, plane)) return e;
    if (int e = bufs.get(static_cast<char*>(out), res, (size_t)nrec * rec_bytes)) return e;
    return OGG_OK;
}

}  // namespace

extern "C" int ogg_topog(const ogg_topog_band* band, const ogg_topog_source* src, ogg_topog_record* out) {
    return topog_host(band, src, out, false);
}

extern "C" int ogg_topog_plane(const ogg_topog_band* band, const ogg_topog_source* src, ogg_topog_plane_record* out) {
    return topog_host(band, src, out, true);
}

// ---- layered topography: entry points ------------------------------------------------------------------------------------------
namespace {

int check_projection(const ogg_topog_projection& p, int k) {
    OGG_REQUIRE(p.h == 1 || p.h == -1, OGG_EARG, "ogg_topog_layers: layer %d: hemisphere h = %d (+1 or -1)", k, p.h);
    OGG_REQUIRE(p.e >= 0.0 && p.e < 0.2, OGG_EARG, "ogg_topog_layers: layer %d: eccentricity e = %g outside [0, 0.2)", k, p.e);
    OGG_REQUIRE(p.K > 0.0 && std::isfinite(p.K) && std::isfinite(p.lon0), OGG_EARG, "ogg_topog_layers: layer %d: K = %g, lon0 = %g", k,
                p.K, p.lon0);
    OGG_REQUIRE(p.lat_gate >= -80.0 && p.lat_gate <= 90.0, OGG_EARG,
                "ogg_topog_layers: layer %d: lat_gate = %g: the gate latitude (h * lat) must lie in [-80, 90]", k, p.lat_gate);
    return OGG_OK;
}

int check_layer(const ogg_topog_layer& l, int k, bool sampled) {
    OGG_REQUIRE(l.kind == OGG_TOPOG_LATLON || l.kind == OGG_TOPOG_POLAR_STEREO, OGG_EARG, "ogg_topog_layers: layer %d: kind = %d", k, l.kind);
    OGG_REQUIRE(l.q_mul >= 1 && l.q_mul <= OGG_TOPOG_MAX_Q, OGG_EARG, "ogg_topog_layers: layer %d: q_mul = %d (1 .. %d)", k, l.q_mul,
                OGG_TOPOG_MAX_Q);
    if (l.kind == OGG_TOPOG_POLAR_STEREO) {
        OGG_REQUIRE(l.src.dlon > 0.0 && l.src.dlat > 0.0, OGG_EARG, "ogg_topog_layers: layer %d: dX and dY must be positive (%g, %g)", k,
                    l.src.dlon, l.src.dlat);
        OGG_REQUIRE(std::isfinite(l.src.lon0) && std::isfinite(l.src.lat0) && std::isfinite(l.src.dlon) && std::isfinite(l.src.dlat), OGG_EARG,
                    "ogg_topog_layers: layer %d: X0, dX, Y0, dY must be finite", k);
        if (int e = check_projection(l.proj, k)) return e;
    }
    return check_source(l.src, sampled);
}

int check_layers(int n_layers, const ogg_topog_layer* layers, bool sampled) {
    OGG_REQUIRE(n_layers >= 1 && n_layers <= OGG_TOPOG_MAX_SOURCES, OGG_EARG, "ogg_topog_layers: n_layers = %d (1 .. %d)", n_layers,
                OGG_TOPOG_MAX_SOURCES);
    OGG_REQUIRE(layers, OGG_EARG, "ogg_topog_layers: null layers");
    for (int k = 0; k < n_layers; ++k)
        if (int e = check_layer(layers[k], k, sampled)) return e;
    return OGG_OK;
}

Layer make_layer(const ogg_topog_layer& l) {
    Layer L{make_src(l.src), l.kind, l.q_mul, 1.0, 0.0, 0.0, 1.0, 0.0};
    if (l.kind == OGG_TOPOG_POLAR_STEREO) {
        L.s.periodic = false;
        L.h = (double)l.proj.h, L.plon0 = l.proj.lon0, L.e = l.proj.e, L.K = l.proj.K, L.gate = l.proj.lat_gate;
    }
    return L;
}

}  // namespace

// DEVICE pointers.  The caller has run ogg_topog_layer_range_dev on every layer and read n_bad = 0: the kernel forms q_mul * q in
// int and does not look at its range again, so a layer that skipped that check can wrap silently (in the records, never in memory).
extern "C" int ogg_topog_layers_band_dev(const ogg_topog_band* band, int n_layers, const ogg_topog_layer* layers, void* workspace,
                                         long workspace_bytes, ogg_topog_merge_record* out, void* stream) {
    OGG_REQUIRE(band, OGG_EARG, "ogg_topog_layers: null band");
    if (int e = check_layers(n_layers, layers, true)) return e;
    if (int e = check_band(*band)) return e;
    const ogg_topog_band& b = *band;
    const long rows = out_rows(b);
    if (rows == 0) return OGG_OK;
    OGG_REQUIRE(b.x && b.y && b.x_next && b.y_next && out, OGG_EARG, "ogg_topog_layers: null x / y / x_next / y_next / out");
    if (int e = ogg::check_workspace("ogg_topog_layers", workspace, workspace_bytes, ogg_topog_workspace_bytes())) return e;
    const Geo g = make_geo(b);
    Layers ly;
    ly.n = n_layers;
    for (int k = 0; k < NLAY; ++k) ly.l[k] = make_layer(layers[k < n_layers ? k : 0]);   // the slots past n are never read
    hipStream_t st = ogg::as_stream(stream);
    unsigned long long* counter;
    unsigned nwg;
    if (int e = walk_launch(g, workspace, st, &counter, &nwg)) return e;
    bool stereo = false;
    for (int k = 0; k < n_layers; ++k) stereo = stereo || layers[k].kind == OGG_TOPOG_POLAR_STEREO;
#define OGG_LAYERS_LAUNCH(NL)                                                              \
    if (stereo)                                                                            \
        topog_layers_kernel<NL, true><<<nwg, TT, 0, st>>>(g, ly, counter, out);            \
    else                                                                                   \
        topog_layers_kernel<NL, false><<<nwg, TT, 0, st>>>(g, ly, counter, out);           \
    break
    switch (n_layers) {
        case 1: OGG_LAYERS_LAUNCH(1);
        case 2: OGG_LAYERS_LAUNCH(2);
        case 3: OGG_LAYERS_LAUNCH(3);
        default: OGG_LAYERS_LAUNCH(4);
    }
#undef OGG_LAYERS_LAUNCH
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_topog_layer_range_dev(const ogg_topog_layer* layer, int* n_bad, void* stream) {
    OGG_REQUIRE(layer && n_bad, OGG_EARG, "ogg_topog_layer_range: null pointer");
    if (int e = check_layer(*layer, 0, true)) return e;
    hipStream_t st = ogg::as_stream(stream);
    OGG_HIP_CHECK(hipMemsetAsync(n_bad, 0, sizeof(int), st));
    const ogg_topog_source& s = layer->src;
    const long n = s.Nx * s.Ny;
    const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 65536);
    if (s.dtype == OGG_TOPOG_INT16)
        topog_range_kernel<short><<<blocks, 256, 0, st>>>(static_cast<const short*>(s.data), n, int16_fill(s, 0), int16_fill(s, 1),
                                                          layer->q_mul, n_bad);
    else
        topog_range_kernel<int><<<blocks, 256, 0, st>>>(static_cast<const int*>(s.data), n, 0, 0, layer->q_mul, n_bad);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_topog_project_dev(const ogg_topog_projection* proj, long n, const double* lon, const double* lat, double* X, double* Y,
                                     int* gate_ok, void* stream) {
    OGG_REQUIRE(proj && n >= 0, OGG_EARG, "ogg_topog_project: null projection or n = %ld", n);
    if (int e = check_projection(*proj, 0)) return e;
    ogg_topog_layer l{};   // the kernel's Layer of the projection alone: no raster, which stereo_project does not read
    l.src.dlon = l.src.dlat = 1.0;
    l.kind = OGG_TOPOG_POLAR_STEREO, l.q_mul = 1, l.proj = *proj;
    if (n == 0) return OGG_OK;
    OGG_REQUIRE(lon && lat && X && Y && gate_ok, OGG_EARG, "ogg_topog_project: null array");
    topog_project_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ogg::as_stream(stream)>>>(make_layer(l), n, lon, lat, X, Y, gate_ok);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// HOST pointers: the grid rows and every layer's raster copied to device memory (a float raster quantised there), the range of
// q_mul * q checked, one band, the merge records copied back (synchronous)
extern "C" int ogg_topog_layers(const ogg_topog_band* band, int n_layers, const ogg_topog_layer* layers, ogg_topog_merge_record* out) {
    OGG_REQUIRE(band && out, OGG_EARG, "ogg_topog_layers: null pointer");
    if (int e = check_layers(n_layers, layers, false)) return e;
    if (int e = check_band(*band)) return e;
    const ogg_topog_band& h = *band;
    OGG_REQUIRE(h.x && h.y, OGG_EARG, "ogg_topog_layers: null x / y");
    const long rows = out_rows(h);
    if (rows == 0) return OGG_OK;
    ogg::Buffers bufs;   // freed on every exit path
    ogg_topog_band d;
    if (int e = stage_band(bufs, h, &d)) return e;
    ogg_topog_layer dl[OGG_TOPOG_MAX_SOURCES];
    int* bad;
    if (int e = bufs.alloc(&bad, 1)) return e;
    for (int k = 0; k < n_layers; ++k) {
        dl[k] = layers[k];
        int nb = 0;
        if (int e = stage_raster(bufs, &dl[k].src, &nb)) return e;
        OGG_REQUIRE(nb == 0, OGG_EARG, "ogg_topog_layers: layer %d: a quantised value exceeds %d in magnitude (quantum %g too small)", k,
                    OGG_TOPOG_MAX_Q, dl[k].src.quantum);
        if (int e = ogg_topog_layer_range_dev(&dl[k], bad, nullptr)) return e;
        if (int e = bufs.get(&nb, bad, 1)) return e;
        OGG_REQUIRE(nb == 0, OGG_EARG, "ogg_topog_layers: layer %d: q_mul = %d times a stored value exceeds %d in magnitude", k, dl[k].q_mul,
                    OGG_TOPOG_MAX_Q);
    }
    const long nrec = rows * (h.nx >> (h.cells == OGG_TOPOG_MODEL_CELLS ? 1 : 0));
    char* ws;
    ogg_topog_merge_record* res;
    if (int e = bufs.alloc(&ws, (size_t)ogg_topog_workspace_bytes())) return e;
    if (int e = bufs.alloc(&res, (size_t)nrec)) return e;
    if (int e = ogg_topog_layers_band_dev(&d, n_layers, dl, ws, ogg_topog_workspace_bytes(), res, nullptr)) return e;
    if (int e = bufs.get(out, res, (size_t)nrec)) return e;
    return OGG_OK;
}

// ---- face topography: entry points ---------------------------------------------------------------------------------------------
namespace {

int check_faces(const FaceParams* pp, const ogg_topog_source* src, bool sampled) {
    OGG_REQUIRE(pp && src, OGG_EARG, "ogg_topog_faces: null pointer");
    const FaceParams& p = *pp;
    OGG_REQUIRE(p.nx >= 2 && p.ny >= 2 && p.nx < (1L << 30) && p.ny < (1L << 30), OGG_EARG, "ogg_topog_faces: %ld x %ld supergrid cells",
                p.ny, p.nx);
    OGG_REQUIRE(p.nx % 2 == 0 && p.ny % 2 == 0, OGG_EARG,
                "ogg_topog_faces: faces lie between model cells of 2 x 2 supergrid cells, but the supergrid has %ld x %ld cells", p.ny, p.nx);
    OGG_REQUIRE(p.ld >= p.nx + 1, OGG_EARG, "ogg_topog_faces: row stride ld = %ld below nx + 1 = %ld", p.ld, p.nx + 1);
    const long nym = p.ny / 2;
    OGG_REQUIRE(p.ju0 >= 0 && p.ju0 <= p.ju1 && p.ju1 <= nym, OGG_EARG, "ogg_topog_faces: u-face rows [%ld, %ld) outside 0 .. %ld", p.ju0,
                p.ju1, nym);
    OGG_REQUIRE(p.jv0 >= 0 && p.jv0 <= p.jv1 && p.jv1 <= nym + 1, OGG_EARG, "ogg_topog_faces: v-face rows [%ld, %ld) outside 0 .. %ld",
                p.jv0, p.jv1, nym + 1);
    OGG_REQUIRE((p.topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "ogg_topog_faces: topology flags %d", p.topology);
    OGG_REQUIRE(p.refine >= 0 && p.refine <= RMAX, OGG_EARG, "ogg_topog_faces: refine = %d (0 or 1 .. %d)", p.refine, RMAX);
    OGG_REQUIRE(p.refine > 0 || (p.oversample > 0.0 && std::isfinite(p.oversample)), OGG_EARG, "ogg_topog_faces: oversample = %g",
                p.oversample);
    return check_source(*src, sampled);
}

template <bool VFACE>
int launch_faces(const Geo& g, const Src& s, const Faces& fc, int dtype, unsigned long long* counter, FaceRecord* out,
                 hipStream_t st) {
    if (fc.total == 0) return OGG_OK;
    int dev = 0, n_cu = 0;
    OGG_HIP_CHECK(hipGetDevice(&dev));
    OGG_HIP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const long takes = (fc.total + TR - 1) / TR;
    const unsigned wgs = (unsigned)std::min(takes, (long)(n_cu > 0 ? n_cu : 256) * 32);   // as walk_launch
    if (dtype == OGG_TOPOG_INT16)
        topog_faces_kernel<OGG_TOPOG_INT16, VFACE><<<wgs, TT, 0, st>>>(g, s, fc, counter, out);
    else
        topog_faces_kernel<OGG_TOPOG_INT32, VFACE><<<wgs, TT, 0, st>>>(g, s, fc, counter, out);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the parameters of a call: the whole stitched grid as one band of model cells (j0 = 0, n_cell_rows = ny; x_next, y_next not read)
int face_params(const ogg_topog_band* grid, long ld, int topology, long ju0, long ju1, long jv0, long jv1, FaceParams* p) {
    OGG_REQUIRE(grid, OGG_EARG, "ogg_topog_faces: null grid");
    OGG_REQUIRE(grid->j0 == 0 && grid->cells == OGG_TOPOG_MODEL_CELLS, OGG_EARG,
                "ogg_topog_faces: the grid is the whole stitched grid as one band of model cells (j0 = %ld, cells = %d)", grid->j0, grid->cells);
    *p = FaceParams{grid->nx, grid->n_cell_rows, ld, grid->x, grid->y, topology, grid->refine, grid->oversample, ju0, ju1, jv0, jv1};
    return OGG_OK;
}

}  // namespace

extern "C" int ogg_topog_faces_check(const ogg_topog_band* grid, long ld, int topology, long ju0, long ju1, long jv0, long jv1,
                                     const ogg_topog_source* src, int device) {
    FaceParams p;
    if (int e = face_params(grid, ld, topology, ju0, ju1, jv0, jv1, &p)) return e;
    return check_faces(&p, src, device != 0);
}

namespace {

int faces_dev(const FaceParams* pp, const ogg_topog_source* src, void* workspace, long workspace_bytes, FaceRecord* out_u, FaceRecord* out_v,
              void* stream) {
    if (int e = check_faces(pp, src, true)) return e;
    const FaceParams& p = *pp;
    const long nu = p.ju1 - p.ju0, nv = p.jv1 - p.jv0;
    if (nu == 0 && nv == 0) return OGG_OK;
    OGG_REQUIRE(p.x && p.y && (nu == 0 || out_u) && (nv == 0 || out_v), OGG_EARG, "ogg_topog_faces: null x / y / out_u / out_v");
    if (int e = ogg::check_workspace("ogg_topog_faces", workspace, workspace_bytes, ogg_topog_workspace_bytes())) return e;
    // the walk's geometry of the whole grid: rows 0 .. ny - 1 at stride ld, the row that follows them the grid's last point row
    const Geo g{p.x, p.y, p.x + p.ny * p.ld, p.y + p.ny * p.ld, p.nx, p.ld, 0, p.ny, 0, 0, 0, 0, p.refine, p.oversample};
    const Src s = make_src(*src);
    const long nxm = p.nx / 2, nym = p.ny / 2;
    const int periodic = (p.topology & OGG_MASK_PERIODIC) != 0, fold = (p.topology & OGG_MASK_FOLD) != 0;
    hipStream_t st = ogg::as_stream(stream);
    unsigned long long* counters = static_cast<unsigned long long*>(workspace);   // one per family
    OGG_HIP_CHECK(hipMemsetAsync(workspace, 0, 2 * sizeof(unsigned long long), st));
    const Faces fu{nxm, nym, p.nx, p.ny, p.ju0, nxm + 1, nu * (nxm + 1), periodic, fold};
    const Faces fv{nxm, nym, p.nx, p.ny, p.jv0, nxm, nv * nxm, periodic, fold};
    if (int e = launch_faces<false>(g, s, fu, src->dtype, counters, out_u, st)) return e;
    if (int e = launch_faces<true>(g, s, fv, src->dtype, counters + 1, out_v, st)) return e;
    return OGG_OK;
}

}  // namespace

extern "C" int ogg_topog_faces_dev(const ogg_topog_band* grid, long ld, int topology, long ju0, long ju1, long jv0, long jv1,
                                   const ogg_topog_source* src, void* workspace, long workspace_bytes, long long* out_u, long long* out_v,
                                   void* stream) {
    FaceParams p;
    if (int e = face_params(grid, ld, topology, ju0, ju1, jv0, jv1, &p)) return e;
    return faces_dev(&p, src, workspace, workspace_bytes, reinterpret_cast<FaceRecord*>(out_u), reinterpret_cast<FaceRecord*>(out_v), stream);
}

// HOST pointers: the grid and the raster copied to device memory (a float raster quantised there), both families in one device call,
// the records of the two ranges copied back (synchronous)
extern "C" int ogg_topog_faces(const ogg_topog_band* grid, long ld, int topology, long ju0, long ju1, long jv0, long jv1,
                               const ogg_topog_source* src, long long* out_u_words, long long* out_v_words) {
    FaceParams h;
    if (int e = face_params(grid, ld, topology, ju0, ju1, jv0, jv1, &h)) return e;
    if (int e = check_faces(&h, src, false)) return e;
    FaceRecord *out_u = reinterpret_cast<FaceRecord*>(out_u_words), *out_v = reinterpret_cast<FaceRecord*>(out_v_words);
    const long nxm = h.nx / 2;
    const long nu = (h.ju1 - h.ju0) * (nxm + 1), nv = (h.jv1 - h.jv0) * nxm;
    if (nu == 0 && nv == 0) return OGG_OK;
    OGG_REQUIRE(h.x && h.y && (nu == 0 || out_u) && (nv == 0 || out_v), OGG_EARG, "ogg_topog_faces: null x / y / out_u / out_v");
    ogg::Buffers bufs;   // freed on every exit path
    FaceParams d = h;
    const size_t npt = (size_t)h.ny * h.ld + (size_t)h.nx + 1;   // the last row ends at its last point
    double *px, *py;
    if (int e = bufs.put(&px, h.x, npt)) return e;
    if (int e = bufs.put(&py, h.y, npt)) return e;
    d.x = px, d.y = py;
    ogg_topog_source ds = *src;
    int nb = 0;
    if (int e = stage_raster(bufs, &ds, &nb)) return e;
    OGG_REQUIRE(nb == 0, OGG_EARG, "ogg_topog_faces: a quantised source value exceeds %d in magnitude (quantum %g too small)",
                OGG_TOPOG_MAX_Q, ds.quantum);
    char* ws;
    FaceRecord *ru, *rv;
    if (int e = bufs.alloc(&ws, (size_t)ogg_topog_workspace_bytes())) return e;
    if (int e = bufs.alloc(&ru, (size_t)std::max(nu, 1L))) return e;
    if (int e = bufs.alloc(&rv, (size_t)std::max(nv, 1L))) return e;
    if (int e = faces_dev(&d, &ds, ws, ogg_topog_workspace_bytes(), ru, rv, nullptr)) return e;
    if (nu)
        if (int e = bufs.get(out_u, ru, (size_t)nu)) return e;
    if (nv)
        if (int e = bufs.get(out_v, rv, (size_t)nv)) return e;
    return OGG_OK;
}
