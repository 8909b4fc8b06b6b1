// Bilinear interpolation of lat-lon fields at the h, u or v points of the grid, and the rotation of vectors to the grid's directions
// (include/ogg_hip.h, "Bilinear interpolation").
//
// bilinear_kernel<T, NC>  one wavefront per 64 consecutive points of a target row, the workgroups striding over the tiles so that a
//                         workgroup fills its tables once.  The tables are the source's centres (c[I] = lonc[I] - lonc[0], latc[J]) in
//                         LDS; when they do not fit (or with OGG_BILINEAR_LDS=0) every node is formed from the edges in global memory
//                         by the same two operations, so the comparisons are the same.  A point is located once, by binary search on
//                         the definition's own comparisons; its four source offsets and four weights stay in registers for all
//                         records.  The record loop takes UNR records at a time: the 4 * NC gathers of all of them are issued before
//                         the first is used, then the sums are formed in the definition's order.  Every record's stores are 64
//                         consecutive values and 64 consecutive flag bytes.  A vector's two components share the offsets, the weights
//                         and the validity of the corners.  OGG_BILINEAR_RECORDS splits the records over blockIdx.y (default: all in
//                         one; a chunk still gathers UNR records at a time, so a chunk of 1 .. 3 records, or a remainder, re-reads its
//                         last record: the same bits, wasted traffic -- use multiples of UNR), OGG_BILINEAR_BLOCKS caps the workgroups
//                         per chunk.
// rotate_kernel           one thread per point: (sa, ca) = sincospi(angle_dx / 180) once, then every record's pair of components.
//
// Every value is a fixed function of one point, the source and the angle there: no knob changes a bit.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ogg_blocks.h"
#include "ogg_common.h"

#pragma clang fp contract(off)

namespace {

using ogg::knob;

constexpr int NT = 256;                 // threads per workgroup (four wavefronts)
constexpr int UNR = 4;                  // records whose gathers are in flight together
constexpr int BLOCKS_DEFAULT = 2048;    // workgroups per record chunk (OGG_BILINEAR_BLOCKS): 8 per CU
constexpr long LDS_MAX = 64 * 1024;     // bytes of tables a workgroup may hold

static_assert(sizeof(ogg_bilinear_params) == 88, "ogg_bilinear_params layout");

// one set of target points: R rows of C points, point (j, i) at supergrid (2 j + oy, 2 i + ox)
struct Pts {
    long R, C;
    int oy, ox;
};

Pts points_of(const ogg_bilinear_params& p, int kind) {
    if (kind == OGG_BILINEAR_U) return Pts{p.ny, p.nx + 1, 1, 0};
    if (kind == OGG_BILINEAR_V) return Pts{p.ny + 1, p.nx, 0, 1};
    return Pts{p.ny, p.nx, 1, 1};
}

struct Geo {
    Pts pt;
    long ld, NA, NB, nrec, rchunk;
    int n_fill, lds;
    double fill0, fill1;
};

// the nodes: from LDS, or from the edges by the operations that filled the LDS
struct Nodes {
    const double *tc, *tl, *lon, *lat;
    double lonc0;
    bool lds;
    __device__ inline double c(long I) const { return lds ? tc[I] : (lon[I] + lon[I + 1]) / 2.0 - lonc0; }
    __device__ inline double l(long J) const { return lds ? tl[J] : (lat[J] + lat[J + 1]) / 2.0; }
};

template <typename T, int NC>
__global__ __launch_bounds__(NT) void bilinear_kernel(Geo g, const double* __restrict__ x, const double* __restrict__ y,
                                                      const double* __restrict__ lon, const double* __restrict__ lat,
                                                      const T* __restrict__ fa, const T* __restrict__ fb,
                                                      const unsigned char* __restrict__ mask, double* __restrict__ outa,
                                                      unsigned char* __restrict__ fla, double* __restrict__ outb,
                                                      unsigned char* __restrict__ flb) {
    extern __shared__ double tab[];
    Nodes nd{tab, tab + g.NA, lon, lat, (lon[0] + lon[1]) / 2.0, g.lds != 0};
    if (g.lds) {
        for (long I = threadIdx.x; I < g.NA; I += NT) tab[I] = (lon[I] + lon[I + 1]) / 2.0 - nd.lonc0;
        for (long J = threadIdx.x; J < g.NB; J += NT) tab[g.NA + J] = (lat[J] + lat[J + 1]) / 2.0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long tiles = (g.pt.C + 63) / 64, nwave = g.pt.R * tiles, npt = g.pt.R * g.pt.C, nsrc = g.NA * g.NB;
    const long r0 = (long)blockIdx.y * g.rchunk, r1 = r0 + g.rchunk < g.nrec ? r0 + g.rchunk : g.nrec;
    const T f0 = static_cast<T>(g.fill0), f1 = static_cast<T>(g.fill1);
    const double latc0 = nd.l(0), latc9 = nd.l(g.NB - 1);
    for (long wave = (long)blockIdx.x * (NT / 64) + threadIdx.x / 64; wave < nwave; wave += (long)gridDim.x * (NT / 64)) {
        const long row = wave / tiles, i = (wave % tiles) * 64 + lane;
        const bool inb = i < g.pt.C;
        const long pidx = row * g.pt.C + i;
        double w[4] = {0.0, 0.0, 0.0, 0.0};
        int o[4] = {0, 0, 0, 0};
        bool wet = true, nolat = false;
        if (inb) {
            const long gi = (2 * row + g.pt.oy) * g.ld + 2 * i + g.pt.ox;
            const double px = x[gi], py = y[gi];
            if (mask) wet = mask[pidx] != 0;
            nolat = py != py;   // a NaN latitude lies between no two nodes: the point is unfilled whatever the corners hold
            double t = px - nd.lonc0;
            t = t - 360.0 * floor(t / 360.0);
            if (!(t >= 0.0 && t < 360.0)) t = 0.0;
            long lo = 0, hi = g.NA;
            while (lo < hi) {   // the first index with c > t
                const long mid = (lo + hi) >> 1;
                if (nd.c(mid) <= t) lo = mid + 1; else hi = mid;
            }
            const long I = lo > 0 ? lo - 1 : 0, I1 = I + 1 < g.NA ? I + 1 : 0;
            const double cI = nd.c(I), c1 = I + 1 < g.NA ? nd.c(I + 1) : nd.c(0) + 360.0;
            const double wx = (t - cI) / (c1 - cI);
            long J, J1;
            double wy = 0.0;
            if (py <= latc0) {
                J = J1 = 0;
            } else if (py >= latc9) {
                J = J1 = g.NB - 1;
            } else {
                lo = 0, hi = g.NB;
                while (lo < hi) {
                    const long mid = (lo + hi) >> 1;
                    if (nd.l(mid) <= py) lo = mid + 1; else hi = mid;
                }
                J = lo - 1;
                if (J < 0) J = 0;                       // (only a NaN latitude gets here or below: the reads stay inside the source,
                                                        //  and nolat keeps their values out of the result)
                if (J > g.NB - 2) J = g.NB - 2;
                if (J < 0) J = 0;
                J1 = J + 1 < g.NB ? J + 1 : J;
                const double lJ = nd.l(J);
                wy = J1 > J ? (py - lJ) / (nd.l(J1) - lJ) : 0.0;
            }
            const double ux = 1.0 - wx, uy = 1.0 - wy;
            w[0] = ux * uy, w[1] = wx * uy, w[2] = ux * wy, w[3] = wx * wy;
            o[0] = (int)(J * g.NA + I), o[1] = (int)(J * g.NA + I1), o[2] = (int)(J1 * g.NA + I), o[3] = (int)(J1 * g.NA + I1);
        }
        for (long r = r0; r < r1; r += UNR) {
            T va[UNR][4], vb[UNR][4];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {   // every gather of UNR records before the first use (the last record again past the end)
                const long rr = r + u < r1 ? r + u : r1 - 1;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    va[u][k] = fa[rr * nsrc + o[k]];
                    vb[u][k] = NC == 2 ? fb[rr * nsrc + o[k]] : T(0);
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (r + u >= r1 || !inb) continue;
                double W = 0.0, Sa = 0.0, Sb = 0.0;
                int n = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool ok = !missing(va[u][k], f0, f1, g.n_fill) && (NC == 1 || !missing(vb[u][k], f0, f1, g.n_fill));
                    if (ok) {
                        W += w[k];
                        Sa += w[k] * (double)va[u][k];
                        if (NC == 2) Sb += w[k] * (double)vb[u][k];
                        ++n;
                    }
                }
                double a = OGG_REMAP_FILL, b = OGG_REMAP_FILL;
                unsigned char fl = OGG_REMAP_DRY;
                if (!wet) {
                } else if (nolat) {
                    fl = OGG_REMAP_UNFILLED;
                } else if (n == 4) {
                    a = Sa, b = Sb, fl = OGG_REMAP_REMAPPED;
                } else if (n > 0 && W > 0.0) {
                    a = Sa / W, b = Sb / W, fl = OGG_REMAP_REMAPPED;
                } else {
                    fl = OGG_REMAP_UNFILLED;
                }
                const long at = (r + u) * npt + pidx;
                if (outa) outa[at] = a;
                if (fla) fla[at] = fl;
                if (NC == 2 && outb) outb[at] = b;
                if (NC == 2 && flb) flb[at] = fl;
            }
        }
    }
}

// (ug, vg) of (uin, vin) at one point set; dst_u / dst_v NULL: that component is not wanted here.  In place when dst == in.
__global__ __launch_bounds__(NT) void rotate_kernel(Pts pt, long ld, long nrec, const double* __restrict__ angle, const double* uin,
                                                    const double* vin, const unsigned char* __restrict__ flags, double* dst_u,
                                                    double* dst_v, double* __restrict__ rot_cos, double* __restrict__ rot_sin,
                                                    int rotate) {
    const long npt = pt.R * pt.C;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < npt; q += (long)gridDim.x * NT) {
        const long j = q / pt.C, i = q % pt.C;
        double sa, ca;
        sincospi(angle[(2 * j + pt.oy) * ld + 2 * i + pt.ox] / 180.0, &sa, &ca);
        rot_cos[q] = ca;
        rot_sin[q] = sa;
        if (!rotate) continue;
        for (long r = 0; r < nrec; ++r) {
            const long at = r * npt + q;
            const unsigned char fl = flags[at];
            if (fl != OGG_REMAP_REMAPPED && fl != OGG_REMAP_FILLED) continue;
            const double U = uin[at], V = vin[at];
            const double ug = U * ca + V * sa, vg = V * ca - U * sa;
            if (dst_u) dst_u[at] = ug;
            if (dst_v) dst_v[at] = vg;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_bilinear_params* p, int has_mask) {
    OGG_REQUIRE(p, OGG_EARG, "bilinear: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny < (long)INT_MAX && p->nx < (long)INT_MAX && (p->ny + 1) * (p->nx + 1) < (1L << 31), OGG_EARG,
                "bilinear: %ld x %ld cells: ny, nx >= 1 and (ny + 1) * (nx + 1) < 2^31", p->ny, p->nx);
    OGG_REQUIRE(p->m0 >= 0 && p->m0 <= (long)INT_MAX, OGG_EARG, "bilinear: first row %ld", p->m0);
    OGG_REQUIRE(p->NA >= 1 && p->NB >= 1 && p->NA <= (long)INT_MAX && p->NB <= (long)INT_MAX && p->NA * p->NB < (1L << 31), OGG_EARG,
                "bilinear: %ld x %ld source cells: NA, NB >= 1 and NA * NB < 2^31", p->NA, p->NB);
    OGG_REQUIRE(p->nrec >= 1 && p->nrec <= (long)INT_MAX && p->nrec * (p->ny + 1) * (p->nx + 1) < (1L << 32), OGG_EARG,
                "bilinear: %ld records of %ld x %ld cells: nrec >= 1 and nrec * (ny + 1) * (nx + 1) < 2^32", p->nrec, p->ny, p->nx);
    OGG_REQUIRE(p->dtype == OGG_REMAP_FLOAT32 || p->dtype == OGG_REMAP_FLOAT64, OGG_EARG, "bilinear: source dtype %d (0: float32, 1: float64)",
                p->dtype);
    OGG_REQUIRE(p->n_fill >= 0 && p->n_fill <= OGG_REMAP_MAX_FILLS, OGG_EARG, "bilinear: %d fill values (at most %d)", p->n_fill,
                OGG_REMAP_MAX_FILLS);
    OGG_REQUIRE(p->points >= OGG_BILINEAR_H && p->points <= OGG_BILINEAR_C, OGG_EARG, "bilinear: point kind %d (0: h, 1: u, 2: v, 3: c)",
                p->points);
    OGG_REQUIRE(p->ncomp == 1 || p->ncomp == 2, OGG_EARG, "bilinear: %d components (1: a scalar, 2: a vector)", p->ncomp);
    OGG_REQUIRE(!(p->points == OGG_BILINEAR_C && p->ncomp == 1), OGG_EARG,
                "bilinear: c points are for vectors (the first component at u, the second at v); a scalar needs h, u or v");
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "bilinear: topology flags %d", p->topology);
    OGG_REQUIRE(!(has_mask && p->points != OGG_BILINEAR_H), OGG_EARG,
                "bilinear: a mask belongs to the h points (the model cells); u, v and c points have no mask and no fill");
    return OGG_OK;
}

struct Launch {
    dim3 grid;
    size_t lds_bytes;
    long rchunk;
    int lds;
};

int plan_launch(const ogg_bilinear_params& p, Launch* out) {
    int rec = 0, blocks = 0, lds = 0;
    if (int e = knob("OGG_BILINEAR_RECORDS", 0, 0, INT_MAX, &rec)) return e;
    if (int e = knob("OGG_BILINEAR_BLOCKS", BLOCKS_DEFAULT, 1, 1 << 20, &blocks)) return e;
    if (int e = knob("OGG_BILINEAR_LDS", 1, 0, 1, &lds)) return e;
    out->rchunk = rec == 0 ? p.nrec : std::min<long>(rec, p.nrec);
    const long nchunk = (p.nrec + out->rchunk - 1) / out->rchunk;
    OGG_REQUIRE(nchunk <= 65535, OGG_EARG, "ogg_bilinear: %ld record chunks (OGG_BILINEAR_RECORDS=%d): at most 65535", nchunk, rec);
    const long tab = (p.NA + p.NB) * 8;
    out->lds = lds && tab <= LDS_MAX;
    out->lds_bytes = out->lds ? (size_t)tab : 0;
    out->grid = dim3((unsigned)blocks, (unsigned)nchunk);
    return OGG_OK;
}

template <typename T, int NC>
void launch(const Launch& l, const Geo& g0, const Pts& pt, hipStream_t st, const double* x, const double* y, const double* lon,
            const double* lat, const void* fa, const void* fb, const unsigned char* mask, double* outa, unsigned char* fla, double* outb,
            unsigned char* flb) {
    Geo g = g0;
    g.pt = pt;
    const long nwave = pt.R * ((pt.C + 63) / 64);
    dim3 grid = l.grid;
    grid.x = (unsigned)std::min<long>(grid.x, (nwave + NT / 64 - 1) / (NT / 64));
    bilinear_kernel<T, NC><<<grid, NT, l.lds_bytes, st>>>(g, x, y, lon, lat, static_cast<const T*>(fa), static_cast<const T*>(fb), mask, outa,
                                                          fla, outb, flb);
}

ogg_remap_params fill_params(const ogg_bilinear_params& p) {
    ogg_remap_params q;
    memset(&q, 0, sizeof(q));
    q.ny = p.ny, q.nx = p.nx, q.m0 = p.m0, q.NA = p.NA, q.NB = p.NB, q.nrec = p.nrec;
    q.dtype = p.dtype, q.n_fill = p.n_fill, q.fill[0] = p.fill[0], q.fill[1] = p.fill[1];
    q.topology = p.topology, q.fill_max = p.fill_max;
    return q;
}

}  // namespace

extern "C" int ogg_bilinear_check(const ogg_bilinear_params* p, int has_mask) { return check_params(p, has_mask); }

extern "C" int ogg_bilinear_dev(const ogg_bilinear_params* p, const double* x, const double* y, long ld, const double* lon, const double* lat,
                                const void* f, const void* f2, const unsigned char* mask, double* values, unsigned char* flags,
                                double* values2, unsigned char* flags2, double* cross, double* cross2, void* stream) {
    if (int e = check_params(p, mask != nullptr)) return e;
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_bilinear: rows of %ld doubles for %ld points", ld, 2 * p->nx + 1);
    OGG_REQUIRE(x && y && lon && lat && f && values && flags, OGG_EARG, "ogg_bilinear: null x / y / lon / lat / f / values / flags");
    OGG_REQUIRE(p->ncomp == 1 || (f2 && values2 && flags2), OGG_EARG, "ogg_bilinear: a vector needs f2, values2 and flags2");
    Launch l;
    if (int e = plan_launch(*p, &l)) return e;
    hipStream_t st = ogg::as_stream(stream);
    const Geo g{Pts{0, 0, 0, 0}, ld, p->NA, p->NB, p->nrec, l.rchunk, p->n_fill, l.lds, p->fill[0], p->fill[1]};
    const bool f32 = p->dtype == OGG_REMAP_FLOAT32;
    if (p->ncomp == 1) {
        (f32 ? launch<float, 1> : launch<double, 1>)(l, g, points_of(*p, p->points), st, x, y, lon, lat, f, nullptr, mask, values, flags,
                                                     nullptr, nullptr);
    } else if (p->points != OGG_BILINEAR_C) {
        (f32 ? launch<float, 2> : launch<double, 2>)(l, g, points_of(*p, p->points), st, x, y, lon, lat, f, f2, mask, values, flags, values2,
                                                     flags2);
    } else {   // both components at the u points (the first kept, the second to cross), then at the v points
        (f32 ? launch<float, 2> : launch<double, 2>)(l, g, points_of(*p, OGG_BILINEAR_U), st, x, y, lon, lat, f, f2, nullptr, values, flags,
                                                     cross, nullptr);
        OGG_LAUNCH_CHECK();
        (f32 ? launch<float, 2> : launch<double, 2>)(l, g, points_of(*p, OGG_BILINEAR_V), st, x, y, lon, lat, f, f2, nullptr, cross2, nullptr,
                                                     values2, flags2);
    }
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

extern "C" int ogg_bilinear_rotate_dev(const ogg_bilinear_params* p, const double* angle, long ld, double* values, const unsigned char* flags,
                                       double* values2, const unsigned char* flags2, const double* cross, const double* cross2,
                                       double* rot_cos, double* rot_sin, double* rot_cos2, double* rot_sin2, int rotate, void* stream) {
    if (int e = check_params(p, 0)) return e;
    OGG_REQUIRE(p->ncomp == 2, OGG_EARG, "ogg_bilinear_rotate: a vector is needed (%d components)", p->ncomp);
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_bilinear_rotate: rows of %ld doubles for %ld points", ld, 2 * p->nx + 1);
    OGG_REQUIRE(angle && rot_cos && rot_sin, OGG_EARG, "ogg_bilinear_rotate: null angle / rot_cos / rot_sin");
    OGG_REQUIRE(!rotate || (values && flags && values2 && flags2), OGG_EARG, "ogg_bilinear_rotate: null values / flags");
    const bool c = p->points == OGG_BILINEAR_C;
    OGG_REQUIRE(!c || (rot_cos2 && rot_sin2), OGG_EARG, "ogg_bilinear_rotate: c points need rot_cos2 and rot_sin2 (the v points)");
    OGG_REQUIRE(!c || !rotate || (cross && cross2), OGG_EARG, "ogg_bilinear_rotate: c points need cross and cross2 of ogg_bilinear_dev");
    hipStream_t st = ogg::as_stream(stream);
    auto grid = [](const Pts& pt) { return (unsigned)std::min<long>(std::max<long>((pt.R * pt.C + NT - 1) / NT, 1), 1 << 16); };
    if (!c) {
        const Pts pt = points_of(*p, p->points);
        rotate_kernel<<<grid(pt), NT, 0, st>>>(pt, ld, p->nrec, angle, values, values2, flags, values, values2, rot_cos, rot_sin, rotate);
    } else {
        const Pts pu = points_of(*p, OGG_BILINEAR_U), pv = points_of(*p, OGG_BILINEAR_V);
        rotate_kernel<<<grid(pu), NT, 0, st>>>(pu, ld, p->nrec, angle, values, cross, flags, values, nullptr, rot_cos, rot_sin, rotate);
        OGG_LAUNCH_CHECK();
        rotate_kernel<<<grid(pv), NT, 0, st>>>(pv, ld, p->nrec, angle, cross2, values2, flags2, nullptr, values2, rot_cos2, rot_sin2, rotate);
    }
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: grid, source and mask copied to device memory, the steps, the results copied back (synchronous)
extern "C" int ogg_bilinear(const ogg_bilinear_params* p, const double* x, const double* y, const double* angle, const double* lon,
                            const double* lat, const void* f, const void* f2, const unsigned char* mask, int do_fill, int rotate,
                            double* values, unsigned char* flags, double* values2, unsigned char* flags2, double* rot_cos, double* rot_sin,
                            double* rot_cos2, double* rot_sin2) {
    if (int e = check_params(p, mask != nullptr)) return e;
    const bool vec = p->ncomp == 2, c = p->points == OGG_BILINEAR_C;
    OGG_REQUIRE(x && y && lon && lat && f && values && flags, OGG_EARG, "ogg_bilinear: null x / y / lon / lat / f / values / flags");
    OGG_REQUIRE(!vec || (f2 && values2 && flags2), OGG_EARG, "ogg_bilinear: a vector needs f2, values2 and flags2");
    OGG_REQUIRE(!do_fill || (p->points == OGG_BILINEAR_H && p->m0 == 0), OGG_EARG,
                "ogg_bilinear: the fill is for the h points of the whole grid (points %d, m0 = %ld)", p->points, p->m0);
    const bool rot = vec && angle;
    OGG_REQUIRE(!rot || (rot_cos && rot_sin && (!c || (rot_cos2 && rot_sin2))), OGG_EARG, "ogg_bilinear: null rot_cos / rot_sin");
    ogg::Buffers bufs;   // freed on every exit path
    const long ld = 2 * p->nx + 1;
    const size_t npt = (size_t)(2 * p->ny + 1) * ld;
    const size_t fbytes = (size_t)p->nrec * p->NA * p->NB * (p->dtype == OGG_REMAP_FLOAT32 ? 4 : 8);
    const Pts p1 = points_of(*p, c ? OGG_BILINEAR_U : p->points), p2 = points_of(*p, c ? OGG_BILINEAR_V : p->points);
    const size_t n1 = (size_t)p1.R * p1.C, n2 = (size_t)p2.R * p2.C, m1 = n1 * p->nrec, m2 = n2 * p->nrec;
    double *dx, *dy, *da = nullptr, *dlon, *dlat, *dv, *dv2 = nullptr, *dc = nullptr, *dc2 = nullptr;
    double *rc = nullptr, *rs = nullptr, *rc2 = nullptr, *rs2 = nullptr;
    char *df, *df2 = nullptr;
    unsigned char *dm = nullptr, *dfl, *dfl2 = nullptr;
    if (int e = bufs.put(&dx, x, npt)) return e;
    if (int e = bufs.put(&dy, y, npt)) return e;
    if (int e = bufs.put(&dlon, lon, (size_t)p->NA + 1)) return e;
    if (int e = bufs.put(&dlat, lat, (size_t)p->NB + 1)) return e;
    if (int e = bufs.put(&df, static_cast<const char*>(f), fbytes)) return e;
    if (vec)
        if (int e = bufs.put(&df2, static_cast<const char*>(f2), fbytes)) return e;
    if (mask)
        if (int e = bufs.put(&dm, mask, (size_t)p->ny * p->nx)) return e;
    if (int e = bufs.alloc(&dv, m1)) return e;
    if (int e = bufs.alloc(&dfl, (m1 + 3) / 4 * 4)) return e;
    if (vec) {
        if (int e = bufs.alloc(&dv2, m2)) return e;
        if (int e = bufs.alloc(&dfl2, (m2 + 3) / 4 * 4)) return e;
    }
    if (rot) {
        if (int e = bufs.put(&da, angle, npt)) return e;
        if (int e = bufs.alloc(&rc, n1)) return e;
        if (int e = bufs.alloc(&rs, n1)) return e;
        if (c) {
            if (int e = bufs.alloc(&rc2, n2)) return e;
            if (int e = bufs.alloc(&rs2, n2)) return e;
            if (rotate) {
                if (int e = bufs.alloc(&dc, m1)) return e;
                if (int e = bufs.alloc(&dc2, m2)) return e;
            }
        }
    }
    if (int e = ogg_bilinear_dev(p, dx, dy, ld, dlon, dlat, df, df2, dm, dv, dfl, dv2, dfl2, dc, dc2, nullptr)) return e;
    if (do_fill) {
        const ogg_remap_params q = fill_params(*p);
        const long wsb = ogg_remap_workspace_bytes(&q);
        OGG_REQUIRE(wsb >= 0, OGG_EARG, "ogg_bilinear: the fill does not take these sizes: %s", ogg_last_error());
        char* ws;
        ogg_remap_counts* ct;
        if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
        if (int e = bufs.alloc(&ct, 1)) return e;
        OGG_HIP_CHECK(hipMemset(ct, 0, sizeof(ogg_remap_counts)));
        if (int e = ogg_remap_fill_dev(&q, ws, wsb, dv, dfl, ct, nullptr)) return e;
        if (vec)
            if (int e = ogg_remap_fill_dev(&q, ws, wsb, dv2, dfl2, ct, nullptr)) return e;
    }
    if (rot)
        if (int e = ogg_bilinear_rotate_dev(p, da, ld, dv, dfl, dv2, dfl2, dc, dc2, rc, rs, rc2, rs2, rotate ? 1 : 0, nullptr)) return e;
    OGG_HIP_CHECK(hipDeviceSynchronize());
    if (int e = bufs.get(values, dv, m1)) return e;
    if (int e = bufs.get(flags, dfl, m1)) return e;
    if (vec) {
        if (int e = bufs.get(values2, dv2, m2)) return e;
        if (int e = bufs.get(flags2, dfl2, m2)) return e;
    }
    if (rot) {
        if (int e = bufs.get(rot_cos, rc, n1)) return e;
        if (int e = bufs.get(rot_sin, rs, n1)) return e;
        if (c) {
            if (int e = bufs.get(rot_cos2, rc2, n2)) return e;
            if (int e = bufs.get(rot_sin2, rs2, n2)) return e;
        }
    }
    return OGG_OK;
}
