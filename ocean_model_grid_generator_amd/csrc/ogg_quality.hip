// Grid-quality report (include/ogg_hip.h, "Grid-quality report"): one read-only pass over a band of the stitched supergrid, then a
// deterministic merge of the per-workgroup records.
//
// quality_band_kernel: a workgroup of QT = 128 threads owns QW = 127 point columns and walks up to QR point rows of them; thread t
// holds column c0 + t, and the last thread loads the first column of the next tile (its halo column) without evaluating anything
// there.  Each step issues the loads of row j+2 (x, y, dx, dy, area: 8-B loads, consecutive lanes on consecutive doubles -- rows of
// nx + 1 doubles are not 16-B aligned on every row), turns the point of row j+1, loaded one step earlier, into a unit vector ONCE
// (two fp64 sincospi) and puts it, with dx and dy, into one of two LDS rows; the i + 1 neighbours of row j come out of the other LDS
// row, the j + 1 ones are the thread's own registers.  The corner angle is kept as tan(delta) = |A'.B'| / |A' x B'| (one division
// instead of an atan2; delta is monotonic in it), so ext[OGG_Q_DELTA_MAX].value of a record is tan(delta).
// One barrier per row.  Every thread keeps running (value, key) extrema and integer counts; the workgroup reduces them across the
// wave (shuffles) and the two waves (LDS) and writes one ogg_grid_quality_result to the workspace.
// quality_merge_kernel: one workgroup per extremum / count merges the records of all workgroups; extrema compare (value, j, i),
// counts are integer sums, so the merged result does not depend on the order (nor on the split into bands and workgroups).
#include <cmath>
#include <vector>

#include "ogg_common.h"
#include "ogg_math.h"

namespace {

constexpr int QT = 128;       // threads per workgroup (2 waves)
constexpr int QW = QT - 1;    // point columns a workgroup owns
constexpr int QR = 32;        // point rows per workgroup
constexpr int MT = 256;       // threads of a merge workgroup
constexpr unsigned EMPTY = 0xffffffffu;
constexpr int NE = OGG_Q_N_EXTREMA, NC = OGG_Q_N_COUNTS;

static_assert(sizeof(ogg_quality_extremum) == 40, "ogg_quality_extremum layout");

OGG_DEV bool is_min(int e) { return e == OGG_Q_DX_MIN || e == OGG_Q_DY_MIN || e == OGG_Q_AREA_MIN; }

struct Band {
    long nx, nxp, j0, n_pt, n_cell, tiles_x;
    const double *x, *y, *dx, *dy, *area, *x_next, *y_next, *dx_next, *dy_next, *x_seam, *y_seam;
    double Re;
    int metrics;
    ogg_grid_quality_result* ws;
};

// tan of the bin edges of the corner-delta histogram, OGG_QUALITY_BIN_EDGES_DEG (numpy.tan(numpy.radians(edge)))
__constant__ double tan_edges[OGG_QUALITY_N_BINS - 1] = {1.7453292519943298e-08, 1.745329252171549e-05, 0.0017453310241888004,
                                                          0.017455064928217585, 0.08748866352592401, 0.36397023426620234};

// the loads of one row: point row jr (x, y, dx) and cell row jr (dy, area) of the band, or of the band that follows it (x_next ...,
// dy_next) one row past its end; zeros where the row does not exist or the workgroup does not need it (past r1)
struct Raw {
    double x, y, dx, dy, ar;
};

struct Unit {
    double x, y, z;
};

OGG_DEV Unit unit_vector(double lon, double lat) {
    double sl, cl, sp, cp;
    sincospi(lon * (1.0 / 180.0), &sl, &cl);
    sincospi(lat * (1.0 / 180.0), &sp, &cp);
    return Unit{cp * cl, cp * sl, sp};
}

OGG_DEV Raw load_row(const Band& b, long jr, long r1, long i, bool col, bool m) {
    Raw w{0.0, 0.0, 0.0, 0.0, 0.0};
    if (!col || jr > r1) return w;
    const long nx = b.nx, nxp = b.nxp;
    if (jr < b.n_pt) {
        w.x = b.x[jr * nxp + i], w.y = b.y[jr * nxp + i];
        if (m && i < nx) w.dx = b.dx[jr * nx + i];
    } else if (jr == b.n_pt && b.x_next) {
        w.x = b.x_next[i], w.y = b.y_next[i];
        if (m && i < nx) w.dx = b.dx_next[i];
    }
    if (m && jr < b.n_cell) {
        w.dy = b.dy[jr * nxp + i];
        if (i < nx) w.ar = b.area[jr * nx + i];
    } else if (m && jr == b.n_cell && b.dy_next) {
        w.dy = b.dy_next[i];
    }
    return w;
}

OGG_DEV void take_max(double& bv, unsigned& bk, double v, unsigned k) {
    if (v > bv || (v == bv && k < bk)) bv = v, bk = k;
}
OGG_DEV void take_min(double& bv, unsigned& bk, double v, unsigned k) {
    if (v < bv || (v == bv && k < bk)) bv = v, bk = k;
}
// max(p / q, q / p) with ONE division: the larger quotient is the one of the larger over the smaller value (rounding is monotonic)
OGG_DEV double ratio(double p, double q) { return p >= q ? p / q : q / p; }

__global__ __launch_bounds__(QT) void quality_band_kernel(Band b) {
    __shared__ double lds_p[2][3][QT], lds_dx[2][QT], lds_dy[2][QT];
    __shared__ double red_v[2][NE];
    __shared__ unsigned red_k[2][NE];
    __shared__ unsigned red_c[2][NC];

    const int t = threadIdx.x;
    const long tx = blockIdx.x % b.tiles_x, ty = blockIdx.x / b.tiles_x;
    const long c0 = tx * QW, i = c0 + t;
    const long r0 = ty * QR, r1 = (r0 + QR < b.n_pt) ? r0 + QR : b.n_pt;
    const long nx = b.nx, nxp = b.nxp;
    const bool col = i <= nx;                    // a point column of the grid
    const bool own = col && t < QW;              // ... that this workgroup evaluates
    const bool m = b.metrics != 0;
    const double Re = b.Re;
    const double small = OGG_QUALITY_DEGENERATE_M, small2 = (small / Re) * (small / Re);   // chords of unit vectors

    double ev[NE];
    unsigned ek[NE], cnt[NC];
#pragma unroll
    for (int e = 0; e < NE; ++e) ev[e] = is_min(e) ? INFINITY : -INFINITY, ek[e] = EMPTY;
#pragma unroll
    for (int c = 0; c < NC; ++c) cnt[c] = 0;

    // row r0 (the prologue); row r0 + 1 is in flight while row r0 goes through LDS
    Raw w0 = load_row(b, r0, r1, i, col, m);
    Raw w1 = load_row(b, r0 + 1, r1, i, col, m);
    Unit p0{0.0, 0.0, 0.0};
    if (col) p0 = unit_vector(w0.x, w0.y);
    double dx0 = w0.dx, dy0 = w0.dy, ar0 = w0.ar;
    lds_p[0][0][t] = p0.x, lds_p[0][1][t] = p0.y, lds_p[0][2][t] = p0.z;
    lds_dx[0][t] = dx0, lds_dy[0][t] = dy0;
    __syncthreads();

    for (long j = r0; j < r1; ++j) {
        const int s = (int)((j - r0) & 1);
        const unsigned key = (unsigned)(j - r0) * QT + t;
        const bool cell = j < b.n_cell;             // cell row j exists: point row j + 1 exists too
        const bool nxt = j + 1 == b.n_pt;           // row j + 1 comes from the band that follows
        const bool dy1_ok = m && (j + 1 < b.n_cell || (j + 1 == b.n_cell && b.dy_next));
        // row j + 1 was loaded one step ago; the loads of row j + 2 go out now and land behind the evaluation of row j
        const double dx1 = w1.dx, dy1 = w1.dy, ar1 = w1.ar;
        Unit p1{0.0, 0.0, 0.0};
        if (col && cell) p1 = unit_vector(w1.x, w1.y);
        w1 = load_row(b, j + 2, r1, i, col, m);
        double dxw = 0.0;
        if (own && m && i == nx - 1) dxw = b.dx[j * nx];   // the periodic partner of dx[j, nx-1]
        // i + 1 neighbours of row j
        const Unit pe{lds_p[s][0][t < QT - 1 ? t + 1 : t], lds_p[s][1][t < QT - 1 ? t + 1 : t], lds_p[s][2][t < QT - 1 ? t + 1 : t]};
        const double dxe = lds_dx[s][t < QT - 1 ? t + 1 : t], dye = lds_dy[s][t < QT - 1 ? t + 1 : t];

        if (own) {
            // point row j: dx and its i-direction ratio
            if (m && i < nx) {
                ++cnt[OGG_Q_N_DX];
                take_max(ev[OGG_Q_DX_MAX], ek[OGG_Q_DX_MAX], dx0, key);
                if (!(dx0 >= small)) {
                    if (dx0 == dx0) ++cnt[OGG_Q_N_DX_DEGENERATE];
                } else {
                    take_min(ev[OGG_Q_DX_MIN], ek[OGG_Q_DX_MIN], dx0, key);
                    const double dxr = (i == nx - 1) ? dxw : dxe;
                    if (dxr >= small) take_max(ev[OGG_Q_RX_MAX], ek[OGG_Q_RX_MAX], ratio(dxr, dx0), key);
                }
            }
            if (cell) {
                if (m) {
                    ++cnt[OGG_Q_N_DY];
                    take_max(ev[OGG_Q_DY_MAX], ek[OGG_Q_DY_MAX], dy0, key);
                    const bool dy_ok = dy0 >= small;
                    if (!dy_ok) {
                        if (dy0 == dy0) ++cnt[OGG_Q_N_DY_DEGENERATE];
                    } else {
                        take_min(ev[OGG_Q_DY_MIN], ek[OGG_Q_DY_MIN], dy0, key);
                        if (dy1_ok && dy1 >= small) {
                            const double r = ratio(dy1, dy0);
                            take_max(ev[OGG_Q_RY_MAX], ek[OGG_Q_RY_MAX], r, key);
                            if (j + 1 == b.n_cell) take_max(ev[OGG_Q_RY_NEXT_MAX], ek[OGG_Q_RY_NEXT_MAX], r, key);
                        }
                    }
                    if (i < nx) {
                        ++cnt[OGG_Q_N_AREA];
                        take_max(ev[OGG_Q_AREA_MAX], ek[OGG_Q_AREA_MAX], ar0, key);
                        if (ar0 == 0.0) {
                            ++cnt[OGG_Q_N_AREA_ZERO];
                        } else {
                            take_min(ev[OGG_Q_AREA_MIN], ek[OGG_Q_AREA_MIN], ar0, key);
                        }
                        if (dx0 >= small && dx1 >= small && dy_ok && dye >= small) {
                            const double a = (dx0 + dx1) / 2, bb = (dy0 + dye) / 2;
                            take_max(ev[OGG_Q_ASPECT_MAX], ek[OGG_Q_ASPECT_MAX], ratio(a, bb), key);
                        }
                    }
                }
                if (i < nx) {   // the SW corner of cell (j, i)
                    ++cnt[OGG_Q_N_CORNERS];
                    const double ax = pe.x - p0.x, ay = pe.y - p0.y, az = pe.z - p0.z;
                    const double bx = p1.x - p0.x, by = p1.y - p0.y, bz = p1.z - p0.z;
                    const double la2 = ax * ax + ay * ay + az * az, lb2 = bx * bx + by * by + bz * bz;
                    if (!(la2 >= small2 && lb2 >= small2)) {   // Re |A| < 1 mm or Re |B| < 1 mm
                        ++cnt[OGG_Q_N_CORNER_DEGENERATE];
                    } else {
                        const double ap = ax * p0.x + ay * p0.y + az * p0.z, bp = bx * p0.x + by * p0.y + bz * p0.z;
                        const double ux = ax - ap * p0.x, uy = ay - ap * p0.y, uz = az - ap * p0.z;
                        const double vx = bx - bp * p0.x, vy = by - bp * p0.y, vz = bz - bp * p0.z;
                        const double d = ux * vx + uy * vy + uz * vz;
                        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
                        const double c = sqrt(cx * cx + cy * cy + cz * cz);
                        // tan(delta) = |A'.B'| / |A' x B'|: delta = |atan2(|A' x B'|, A'.B') - 90 deg| without its cancellation near 90
                        // degrees; delta is monotonic in it, so extrema and bins are taken on tan(delta) (the record holds tan(delta))
                        const double tdelta = fabs(d) / c;
                        take_max(ev[OGG_Q_DELTA_MAX], ek[OGG_Q_DELTA_MAX], tdelta, key);
                        int bin = 0;
#pragma unroll
                        for (int k = 0; k < OGG_QUALITY_N_BINS - 1; ++k) bin += tdelta >= tan_edges[k];
#pragma unroll
                        for (int k = 0; k < OGG_QUALITY_N_BINS; ++k) cnt[OGG_Q_HIST + k] += bin == k;
                    }
                }
            }
            if (nxt && cell && b.x_seam) {   // the dropped last row of the sub-grid below against the first row of the one above
                const Unit q = unit_vector(b.x_seam[i], b.y_seam[i]);
                const double sx = q.x - p1.x, sy = q.y - p1.y, sz = q.z - p1.z;
                take_max(ev[OGG_Q_SEAM_MAX], ek[OGG_Q_SEAM_MAX], Re * sqrt(sx * sx + sy * sy + sz * sz), key + QT);
            }
        }
        // row j + 1 becomes row j
        lds_p[s ^ 1][0][t] = p1.x, lds_p[s ^ 1][1][t] = p1.y, lds_p[s ^ 1][2][t] = p1.z;
        lds_dx[s ^ 1][t] = dx1, lds_dy[s ^ 1][t] = dy1;
        p0 = p1, dx0 = dx1, dy0 = dy1, ar0 = ar1;
        __syncthreads();
    }

    // workgroup reduction: across the wave, then the two waves
    const int lane = t & 63, w = t >> 6;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        double v = ev[e];
        unsigned k = ek[e];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(v, off, 64);
            const unsigned okey = __shfl_xor(k, off, 64);
            if (is_min(e)) take_min(v, k, ov, okey);
            else take_max(v, k, ov, okey);
        }
        if (lane == 0) red_v[w][e] = v, red_k[w][e] = k;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        unsigned v = cnt[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red_c[w][c] = v;
    }
    __syncthreads();
    ogg_grid_quality_result* rec = b.ws + blockIdx.x;
    if (t < NE) {
        const int e = t;
        double v = red_v[0][e];
        unsigned k = red_k[0][e];
        if (is_min(e)) take_min(v, k, red_v[1][e], red_k[1][e]);
        else take_max(v, k, red_v[1][e], red_k[1][e]);
        ogg_quality_extremum out{0.0, 0.0, 0.0, -1, -1};
        if (k != EMPTY) {
            const long jb = r0 + k / QT, ib = c0 + k % QT;   // row of the band (n_pt: the row that follows it), column
            out.value = v;
            out.j = b.j0 + jb, out.i = ib;
            out.lon = jb < b.n_pt ? b.x[jb * nxp + ib] : b.x_next[ib];
            out.lat = jb < b.n_pt ? b.y[jb * nxp + ib] : b.y_next[ib];
        }
        rec->ext[e] = out;
    } else if (t >= 64 && t < 64 + NC) {
        rec->count[t - 64] = (long long)red_c[0][t - 64] + (long long)red_c[1][t - 64];
    }
}

OGG_DEV bool better(bool mn, double v, long long j, long long i, double bv, long long bj, long long bi) {
    if (j < 0) return false;
    if (bj < 0) return true;
    if (v != bv) return mn ? v < bv : v > bv;
    return j < bj || (j == bj && i < bi);
}

// workgroup q < NE merges extremum q of the n records, workgroup NE + c count c
__global__ __launch_bounds__(MT) void quality_merge_kernel(const ogg_grid_quality_result* __restrict__ rec, long n,
                                                           ogg_grid_quality_result* out) {
    __shared__ double sv[MT];
    __shared__ long long sj[MT], si[MT], sr[MT];
    const int t = threadIdx.x, q = blockIdx.x;
    if (q >= NE) {
        const int c = q - NE;
        long long s = 0;
        for (long r = t; r < n; r += MT) s += rec[r].count[c];
        sj[t] = s;
        __syncthreads();
        for (int h = MT / 2; h > 0; h >>= 1) {
            if (t < h) sj[t] += sj[t + h];
            __syncthreads();
        }
        if (t == 0) out->count[c] = sj[0];
        return;
    }
    const bool mn = is_min(q);
    double bv = 0.0;
    long long bj = -1, bi = -1, br = -1;
    for (long r = t; r < n; r += MT) {
        const ogg_quality_extremum& x = rec[r].ext[q];
        if (better(mn, x.value, x.j, x.i, bv, bj, bi)) bv = x.value, bj = x.j, bi = x.i, br = r;
    }
    sv[t] = bv, sj[t] = bj, si[t] = bi, sr[t] = br;
    __syncthreads();
    for (int h = MT / 2; h > 0; h >>= 1) {
        if (t < h && better(mn, sv[t + h], sj[t + h], si[t + h], sv[t], sj[t], si[t]))
            sv[t] = sv[t + h], sj[t] = sj[t + h], si[t] = si[t + h], sr[t] = sr[t + h];
        __syncthreads();
    }
    if (t == 0) out->ext[q] = sr[0] >= 0 ? rec[sr[0]].ext[q] : ogg_quality_extremum{0.0, 0.0, 0.0, -1, -1};
}

long band_blocks(long nx, long n_pt) { return ((nx + 1 + QW - 1) / QW) * ((n_pt + QR - 1) / QR); }

}  // namespace

extern "C" long ogg_grid_quality_workspace_bytes(long nx, long n_pt_rows) {
    if (nx < 1 || n_pt_rows < 0) return -1;
    return band_blocks(nx, n_pt_rows) * (long)sizeof(ogg_grid_quality_result);
}

extern "C" int ogg_grid_quality_band_dev(const ogg_quality_band* band, void* workspace, long workspace_bytes, ogg_grid_quality_result* out,
                                         void* stream) {
    OGG_REQUIRE(band && out, OGG_EARG, "ogg_grid_quality_band: null pointer");
    const ogg_quality_band& q = *band;
    OGG_REQUIRE(q.nx >= 1 && q.n_pt_rows >= 0 && q.Re > 0.0, OGG_EARG, "ogg_grid_quality_band: bad size or radius");
    OGG_REQUIRE(q.n_cell_rows == q.n_pt_rows || (q.n_pt_rows > 0 && q.n_cell_rows == q.n_pt_rows - 1), OGG_ESHAPE,
                "ogg_grid_quality_band: %ld cell rows for %ld point rows", q.n_cell_rows, q.n_pt_rows);
    OGG_REQUIRE(q.n_pt_rows == 0 || (q.x && q.y), OGG_EARG, "ogg_grid_quality_band: null x / y");
    OGG_REQUIRE(!q.metrics || q.n_pt_rows == 0 || (q.dx && (q.n_cell_rows == 0 || (q.dy && q.area))), OGG_EARG,
                "ogg_grid_quality_band: null dx / dy / area");
    const bool needs_next = q.n_cell_rows > 0 && q.n_cell_rows == q.n_pt_rows;
    OGG_REQUIRE(!needs_next || (q.x_next && q.y_next && (!q.metrics || q.dx_next)), OGG_EARG,
                "ogg_grid_quality_band: the last cell row needs the next point row (x_next, y_next, dx_next)");
    OGG_REQUIRE(!q.x_seam || (q.y_seam && needs_next), OGG_EARG, "ogg_grid_quality_band: a seam row needs y_seam and the next row");
    const long nb = band_blocks(q.nx, q.n_pt_rows);
    OGG_REQUIRE(nb == 0 || (workspace && workspace_bytes >= nb * (long)sizeof(ogg_grid_quality_result)), OGG_EARG,
                "ogg_grid_quality_band: workspace of %ld bytes, %ld needed", workspace_bytes, nb * (long)sizeof(ogg_grid_quality_result));
    hipStream_t st = ogg::as_stream(stream);
    Band b{q.nx, q.nx + 1, q.j0, q.n_pt_rows, q.n_cell_rows, (q.nx + 1 + QW - 1) / QW, q.x, q.y, q.dx, q.dy, q.area, q.x_next, q.y_next,
           q.dx_next, q.dy_next, q.x_seam, q.y_seam, q.Re, q.metrics, static_cast<ogg_grid_quality_result*>(workspace)};
    if (nb > 0) {
        OGG_REQUIRE(nb < (1L << 31), OGG_ESHAPE, "ogg_grid_quality_band: band too large (%ld workgroups)", nb);
        quality_band_kernel<<<(unsigned)nb, QT, 0, st>>>(b);
        OGG_LAUNCH_CHECK();
    }
    quality_merge_kernel<<<NE + NC, MT, 0, st>>>(b.ws, nb, out);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: every array of *band copied to device memory, one band, the result copied back (synchronous)
extern "C" int ogg_grid_quality(const ogg_quality_band* band, ogg_grid_quality_result* out) {
    OGG_REQUIRE(band && out, OGG_EARG, "ogg_grid_quality: null pointer");
    const ogg_quality_band& h = *band;
    OGG_REQUIRE(h.nx >= 1 && h.n_pt_rows >= 0 && h.n_cell_rows >= 0, OGG_EARG, "ogg_grid_quality: bad size");
    ogg::Buffers bufs;   // freed on every exit path
    const long nxp = h.nx + 1, np = h.n_pt_rows, nc = h.n_cell_rows;
    ogg_quality_band d = h;   // the same descriptor with device copies of every array it names
    auto up = [&bufs](const double* src, long n, const double** dst) -> int {
        *dst = nullptr;
        if (!src) return OGG_OK;
        double* p;
        if (int e = bufs.alloc(&p, (size_t)(n > 0 ? n : 0))) return e;
        *dst = p;
        return n > 0 ? bufs.send(p, src, (size_t)n) : OGG_OK;
    };
#define OGG_UP(src, n, dst)                   \
    do {                                      \
        if (int e__ = up((src), (n), (dst))) return e__; \
    } while (0)
    OGG_UP(h.x, np * nxp, &d.x);
    OGG_UP(h.y, np * nxp, &d.y);
    d.dx = d.dy = d.area = d.dx_next = d.dy_next = nullptr;
    if (h.metrics) {
        OGG_UP(h.dx, np * h.nx, &d.dx);
        OGG_UP(h.dy, nc * nxp, &d.dy);
        OGG_UP(h.area, nc * h.nx, &d.area);
        OGG_UP(h.dx_next, h.nx, &d.dx_next);
        OGG_UP(h.dy_next, nxp, &d.dy_next);
    }
    OGG_UP(h.x_next, nxp, &d.x_next);
    OGG_UP(h.y_next, nxp, &d.y_next);
    OGG_UP(h.x_seam, nxp, &d.x_seam);
    OGG_UP(h.y_seam, nxp, &d.y_seam);
#undef OGG_UP
    const long ws_bytes = ogg_grid_quality_workspace_bytes(h.nx, np);
    char* ws;
    ogg_grid_quality_result* res;
    if (int e = bufs.alloc(&ws, (size_t)(ws_bytes > 0 ? ws_bytes : 0))) return e;
    if (int e = bufs.alloc(&res, 1)) return e;
    if (int e = ogg_grid_quality_band_dev(&d, ws, ws_bytes, res, nullptr)) return e;
    return bufs.get(out, res, 1);
}
