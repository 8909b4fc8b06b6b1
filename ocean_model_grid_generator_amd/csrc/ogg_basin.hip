// Basin codes: ordered seeded floods of the wet cells (include/ogg_hip.h, "Basin codes").  Rule k floods, from its seed cell, the
// cells that are wet, valid, not yet coded and inside its longitude / latitude box.  A flood is a connected component under a per-cell
// class, so the floods are the components of ogg_label.h (its tile, merge and flatten launches, the ocean mask's) and the launches of a
// call do not grow with a basin's diameter.  Consecutive rules whose boxes are pairwise disjoint cannot see each other's cells and run
// as ONE pass (planned on the host); every pass is five launches on the caller's stream, and nothing comes back to the host between
// passes:
//
// basin_unit_kernel      once: the unit vector of every cell centre (NaN for an invalid centre), code = 0 and rule = -1 everywhere,
//                        and the wet count.
// basin_seed_kernel      once: the seed cell of every rule, the valid cell with the smallest (bits of dist2, cell).  A wavefront lane
//                        is a rule, the cells stream through LDS, every lane tests every cell: three subtractions and three products
//                        per test, no sin / cos beyond the seed's own.  One partial result per (block, rule), reduced by
// basin_seed_reduce_kernel  into the rule records.
// basin_tile_kernel      per pass: the class byte of every cell of a tile (the index inside the pass of the rule whose box holds it if
//                        the cell is wet, valid and uncoded; NONE = 255 otherwise), kept in cls[], then label_tile.
// basin_seedroot_kernel  one thread per rule of the pass: the status of the rule, and the root of its seed cell if it floods.
// basin_assign_kernel    every cell whose root is the kept root of its class's rule gets that rule's code and index; the cells taken
//                        are counted per wavefront and class, then in LDS, then one atomicAdd per block and rule.
//
// Every result is an integer, and the key of the seed search is total, so nothing depends on the launch geometry.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ogg_blocks.h"
#include "ogg_common.h"
#include "ogg_label.h"
#include "ogg_sphere.h"

#pragma clang fp contract(off)

namespace {

using ogg::at;
using ogg::grid_for;
using ogg::knob;

constexpr int PASS_MAX = OGG_BASIN_MAX_PASS_RULES;
constexpr long SEED_BLOCKS = 1024; // workgroups of the seed search, over cells and groups of 64 rules
constexpr double SEPARATION = 1.0e-9;   // degrees: two boxes closer than this are not disjoint for the planner

static_assert(PASS_MAX < NONE + 1 && PASS_MAX <= NT, "a class is a byte, and a thread per rule of a pass");
static_assert(sizeof(ogg_basin_params) == 32, "ogg_basin_params layout");
static_assert(sizeof(ogg_basin_rule) == 56, "ogg_basin_rule layout");
static_assert(sizeof(ogg_basin_rule_record) == 32, "ogg_basin_rule_record layout");
static_assert(sizeof(ogg_basin_counts) == 32, "ogg_basin_counts layout");

// ---- the box predicate: host and device, one rounding order --------------------------------------------------------
__host__ __device__ inline bool in_box(double lon, double lat, double lon_w, double W, double lat_s, double lat_n) {
    if (!(lat_s <= lat && lat <= lat_n)) return false;
    double t = lon - lon_w;
    t = t - 360.0 * floor(t / 360.0);
    return W == 360.0 || t <= W;
}

struct Pass {
    int r0, nr;   // the rules r0 .. r0 + nr - 1
};

// ---- once per call ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void basin_unit_kernel(long ny, long nx, const double* __restrict__ x, const double* __restrict__ y,
                                                        long ld, const unsigned char* __restrict__ wet, double* __restrict__ u,
                                                        unsigned char* __restrict__ code, short* __restrict__ rule,
                                                        ogg_basin_counts* counts) {
    const long n = ny * nx;
    long long v[1] = {0};
    for (long c = (long)blockIdx.x * NT + threadIdx.x; c < n; c += (long)gridDim.x * NT) {
        const long k = centre_point(c, nx, ld);
        const double lon = x[k], lat = y[k];
        double t[3] = {NAN, NAN, NAN};
        if (isfinite(lon) && isfinite(lat)) unit(lon, lat, t);
        u[3 * c] = t[0];
        u[3 * c + 1] = t[1];
        u[3 * c + 2] = t[2];
        code[c] = 0;
        rule[c] = -1;
        v[0] += wet[c] != 0;
    }
    long long* const dst[1] = {&counts->wet};
    block_add<1>(v, dst);
}

// part[(b * K + s) * 2 ..]: the smallest (d2 bits, cell) of rule s over the cells of block column b
__global__ __launch_bounds__(NT) void basin_seed_kernel(long n, const double* __restrict__ u, int K, const ogg_basin_rule* __restrict__ rules,
                                                        unsigned long long* __restrict__ part) {
    __shared__ double cu[3][NT];
    __shared__ unsigned long long wb[NT / 64][64];
    __shared__ int wc[NT / 64][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
    const int s = blockIdx.y * 64 + lane;
    double su[3] = {0.0, 0.0, 0.0};
    if (s < K) unit(rules[s].seed_lon, rules[s].seed_lat, su);
    Nearest best{ULLONG_MAX, INT_MAX};
    for (long base = (long)blockIdx.x * NT; base < n; base += (long)gridDim.x * NT) {
        __syncthreads();   // the chunk before this one has been read
        const long c = base + threadIdx.x;
        cu[0][threadIdx.x] = c < n ? u[3 * c] : NAN;
        cu[1][threadIdx.x] = c < n ? u[3 * c + 1] : NAN;
        cu[2][threadIdx.x] = c < n ? u[3 * c + 2] : NAN;
        __syncthreads();
        for (int k = 0; k < 64; ++k) {   // this wavefront's 64 cells of the chunk, in ascending order
            const int q = w * 64 + k;
            const double ax = cu[0][q];
            if (ax != ax) continue;   // an invalid centre (or past the end) is no candidate; the same for every lane
            best.offer(bits_of(dist2(ax, cu[1][q], cu[2][q], su[0], su[1], su[2])), (int)(base + q));
        }
    }
    wb[w][lane] = best.bits;
    wc[w][lane] = best.cell;
    __syncthreads();
    if (w == 0 && s < K) {
        for (int v = 1; v < NT / 64; ++v) best.offer(wb[v][lane], wc[v][lane]);
        part[((long)blockIdx.x * K + s) * 2] = best.bits;
        part[((long)blockIdx.x * K + s) * 2 + 1] = (unsigned long long)(unsigned)best.cell;
    }
}

__global__ __launch_bounds__(NT) void basin_seed_reduce_kernel(int K, int nparts, const unsigned long long* __restrict__ part,
                                                               ogg_basin_rule_record* __restrict__ rec) {
    const int s = blockIdx.x * NT + threadIdx.x;
    if (s >= K) return;
    Nearest best{ULLONG_MAX, INT_MAX};
    for (int b = 0; b < nparts; ++b) best.offer(part[((long)b * K + s) * 2], (int)(unsigned)part[((long)b * K + s) * 2 + 1]);
    rec[s].seed_cell = best.found() ? best.cell : -1;
    rec[s].d2_bits = best.found() ? (long long)best.bits : (long long)bits_of(INFINITY);
    rec[s].status = OGG_BASIN_TOOK;
    rec[s].blocking_rule = -1;
    rec[s].cells = 0;
}

// ---- per pass: the classes and the tile-local labelling (ogg_label.h) -----------------------------------------------
__global__ __launch_bounds__(NT) void basin_tile_kernel(Grid g, Pass ps, const ogg_basin_rule* __restrict__ rules,
                                                        const double* __restrict__ x, const double* __restrict__ y, long ld,
                                                        const unsigned char* __restrict__ wet, const unsigned char* __restrict__ code,
                                                        unsigned char* __restrict__ cls, int* par) {
    extern __shared__ int lab[];                 // TW * th parents, then TW * th class bytes
    __shared__ double box[PASS_MAX][4];          // the boxes of the pass's rules: lon_w, W = lon_e - lon_w, lat_s, lat_n
    const int n = TW * g.th;
    unsigned char* lc = reinterpret_cast<unsigned char*>(lab + n);
    const long i0 = (long)(blockIdx.x % g.nbx) * TW, j0 = (long)(blockIdx.x / g.nbx) * g.th;
    for (int r = threadIdx.x; r < ps.nr; r += NT) {
        const ogg_basin_rule q = rules[ps.r0 + r];
        box[r][0] = q.lon_w;
        box[r][1] = q.lon_e - q.lon_w;
        box[r][2] = q.lat_s;
        box[r][3] = q.lat_n;
    }
    __syncthreads();
    int any = 0;
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        int k = NONE;
        if (j < g.ny && i < g.nx) {
            const long c = j * g.nx + i;
            if (wet[c] != 0 && code[c] == 0) {
                const long q = centre_ji(j, i, ld);
                const double lon = x[q], lat = y[q];
                if (isfinite(lon) && isfinite(lat))
                    for (int r = 0; r < ps.nr; ++r)
                        if (in_box(lon, lat, box[r][0], box[r][1], box[r][2], box[r][3])) {
                            k = r;   // the first rule of the pass whose box holds the cell
                            break;
                        }
            }
            cls[c] = (unsigned char)k;
        }
        lc[l] = (unsigned char)k;
        lab[l] = k != NONE ? l : -1;
        any |= k != NONE;
    }
    label_tile<true>(g, j0, i0, lab, any, par);
}

struct SameClass {   // the merge predicate: equal classes only
    const unsigned char* __restrict__ cls;
    __device__ bool operator()(const int*, long a, long b) const { return cls[a] != NONE && cls[a] == cls[b]; }
};

// ---- seed roots and the assignment ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void basin_seedroot_kernel(long nx, Pass ps, double seed_max_d2, const ogg_basin_rule* __restrict__ rules,
                                                            const double* __restrict__ x, const double* __restrict__ y, long ld,
                                                            const unsigned char* __restrict__ wet, const unsigned char* __restrict__ code,
                                                            const short* __restrict__ rule, const int* __restrict__ root,
                                                            ogg_basin_rule_record* __restrict__ rec, int* __restrict__ keep) {
    const int r = threadIdx.x;
    if (r >= ps.nr) return;
    const int k = ps.r0 + r;
    const long long sc = rec[k].seed_cell;
    int status = OGG_BASIN_TOOK, blocking = -1, kept = -1;
    if (sc < 0) {
        status = OGG_BASIN_SEED_INVALID;
    } else {
        const double d2 = __longlong_as_double(rec[k].d2_bits);
        const long q = centre_point(sc, nx, ld);
        const ogg_basin_rule w = rules[k];
        if (d2 > seed_max_d2)
            status = OGG_BASIN_SEED_OFF_GRID;
        else if (wet[sc] == 0)
            status = OGG_BASIN_SEED_LAND;
        else if (!in_box(x[q], y[q], w.lon_w, w.lon_e - w.lon_w, w.lat_s, w.lat_n))
            status = OGG_BASIN_SEED_OUTSIDE;
        else if (code[sc] != 0)
            status = OGG_BASIN_SEED_CODED, blocking = rule[sc];
        else
            kept = root[sc];
    }
    rec[k].status = status;
    rec[k].blocking_rule = blocking;
    keep[r] = kept;
}

__global__ __launch_bounds__(NT) void basin_assign_kernel(long n, Pass ps, const ogg_basin_rule* __restrict__ rules,
                                                          const unsigned char* __restrict__ cls, const int* __restrict__ root,
                                                          const int* __restrict__ keep, unsigned char* __restrict__ code,
                                                          short* __restrict__ rule, ogg_basin_rule_record* rec, ogg_basin_counts* counts) {
    __shared__ int kp[NT], kc[NT], cnt[NT];
    kp[threadIdx.x] = (int)threadIdx.x < ps.nr ? keep[threadIdx.x] : -1;
    kc[threadIdx.x] = (int)threadIdx.x < ps.nr ? rules[ps.r0 + threadIdx.x].code : 0;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    long long v[1] = {0};
    for (long base = (long)blockIdx.x * NT; base < n; base += (long)gridDim.x * NT) {   // the same trip count for every thread
        const long c = base + threadIdx.x;
        const int k = c < n ? cls[c] : NONE;
        const bool take = k != NONE && kp[k] >= 0 && root[c] == kp[k];
        if (take) {
            code[c] = (unsigned char)kc[k];
            rule[c] = (short)(ps.r0 + k);
        }
        v[0] += take;
        unsigned long long m = __ballot(take);
        while (m) {   // one LDS add per wavefront and class met
            const int lead = __ffsll((long long)m) - 1;
            const int kl = __shfl(k, lead, 64);
            const unsigned long long same = __ballot(take && k == kl);
            if (lane == lead) atomicAdd(&cnt[kl], __popcll(same));
            m &= ~same;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < ps.nr && cnt[threadIdx.x] > 0)
        atomicAdd(ull(&rec[ps.r0 + threadIdx.x].cells), (unsigned long long)cnt[threadIdx.x]);   // one add per block and rule
    long long* const dst[1] = {&counts->coded};
    block_add<1>(v, dst);
}

__global__ void basin_finish_kernel(ogg_basin_counts* counts, long long passes) {
    counts->uncoded = counts->wet - counts->coded;
    counts->passes = passes;
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_params(const ogg_basin_params* p) {
    OGG_REQUIRE(p, OGG_EARG, "basin codes: null parameters");
    OGG_REQUIRE(p->ny >= 1 && p->nx >= 1 && p->ny <= (long)INT_MAX && p->nx <= (long)INT_MAX && p->ny * p->nx < (1L << 31), OGG_EARG,
                "basin codes: %ld x %ld cells: ny, nx >= 1 and ny * nx < 2^31", p->ny, p->nx);
    OGG_REQUIRE((p->topology & ~(OGG_MASK_PERIODIC | OGG_MASK_FOLD)) == 0, OGG_EARG, "basin codes: topology flags %d", p->topology);
    OGG_REQUIRE(p->n_rules >= 1 && p->n_rules <= OGG_BASIN_MAX_RULES, OGG_EARG, "basin codes: %d rules (1 .. %d)", p->n_rules,
                OGG_BASIN_MAX_RULES);
    OGG_REQUIRE(!std::isnan(p->seed_max_d2) && p->seed_max_d2 >= 0.0, OGG_EARG, "basin codes: seed_max_d2 must be >= 0 or +inf (%g)",
                p->seed_max_d2);
    return OGG_OK;
}

int check_rules(const ogg_basin_params* p, const ogg_basin_rule* rules) {
    if (int e = check_params(p)) return e;
    OGG_REQUIRE(rules, OGG_EARG, "basin codes: null rules");
    for (int k = 0; k < p->n_rules; ++k) {
        const ogg_basin_rule& r = rules[k];
        OGG_REQUIRE(std::isfinite(r.seed_lon) && std::isfinite(r.seed_lat) && std::isfinite(r.lon_w) && std::isfinite(r.lon_e) &&
                        std::isfinite(r.lat_s) && std::isfinite(r.lat_n),
                    OGG_EARG, "basin codes: rule %d holds a value that is not finite", k);
        OGG_REQUIRE(r.code >= 1 && r.code <= 255, OGG_EARG, "basin codes: rule %d has code %d (1 .. 255)", k, r.code);
        OGG_REQUIRE(-90.0 <= r.lat_s && r.lat_s <= r.lat_n && r.lat_n <= 90.0, OGG_EARG,
                    "basin codes: rule %d: -90 <= lat_s <= lat_n <= 90 (%.17g, %.17g)", k, r.lat_s, r.lat_n);
        const double W = r.lon_e - r.lon_w;
        OGG_REQUIRE(W > 0.0 && W <= 360.0, OGG_EARG, "basin codes: rule %d: 0 < lon_e - lon_w <= 360 (%.17g, %.17g)", k, r.lon_w, r.lon_e);
        OGG_REQUIRE(in_box(r.seed_lon, r.seed_lat, r.lon_w, W, r.lat_s, r.lat_n), OGG_EARG,
                    "basin codes: rule %d: the seed (%.17g, %.17g) lies outside its box", k, r.seed_lon, r.seed_lat);
    }
    return OGG_OK;
}

// Two boxes are disjoint for the planner only when their latitude intervals or their longitude arcs are separated by more than
// SEPARATION degrees: far more than the rounding of the predicate's t (a few 1e-14 degrees), so no cell centre is in both.
bool disjoint(const ogg_basin_rule& a, const ogg_basin_rule& b) {
    if (a.lat_n + SEPARATION < b.lat_s || b.lat_n + SEPARATION < a.lat_s) return true;
    const double WA = a.lon_e - a.lon_w, WB = b.lon_e - b.lon_w;
    if (WA >= 360.0 || WB >= 360.0) return false;
    double d = fmod(b.lon_w - a.lon_w, 360.0);   // b's west edge, degrees east of a's
    if (d < 0.0) d += 360.0;
    return d > WA + SEPARATION && d + WB + SEPARATION < 360.0;
}

// start[q] .. start[q + 1] - 1 are the rules of pass q: consecutive, pairwise disjoint, at most PASS_MAX
void plan_passes(const ogg_basin_rule* rules, int K, int batch, std::vector<int>* start) {
    start->assign(1, 0);
    for (int k = 1; k <= K; ++k) {
        bool cut = k == K || !batch || k - start->back() >= PASS_MAX;
        for (int q = start->back(); !cut && q < k; ++q) cut = !disjoint(rules[q], rules[k]);
        if (cut) start->push_back(k);
    }
}

// workspace: unit vectors | parents | roots | classes | kept roots of a pass | partial results of the seed search
struct Layout {
    long u, par, root, cls, keep, part, total;
    unsigned seed_bx, seed_by;
};

Layout layout(const ogg_basin_params& p) {
    Layout l;
    const long n = p.ny * p.nx;
    l.seed_by = (unsigned)((p.n_rules + 63) / 64);
    l.seed_bx = (unsigned)std::max<long>(1, std::min<long>((n + NT - 1) / NT, SEED_BLOCKS / l.seed_by));
    ogg::Sections s{0};
    l.u = s.take(n * 24);
    l.par = s.take(n * 4);
    l.root = s.take(n * 4);
    l.cls = s.take(n);
    l.keep = s.take(NT * 4);
    l.part = s.take((long)l.seed_bx * p.n_rules * 16);
    l.total = s.off;
    return l;
}

int read_knobs(int* th, int* batch) {
    // OGG_BASIN_TILE_ROWS: rows of a labelling tile; OGG_BASIN_BATCH=0: one rule per pass (the cross-check of the planner)
    if (int e = knob("OGG_BASIN_TILE_ROWS", TH_DEFAULT, 1, TH_MAX, th)) return e;
    return knob("OGG_BASIN_BATCH", 1, 0, 1, batch);
}

}  // namespace

extern "C" long ogg_basin_workspace_bytes(const ogg_basin_params* p) {
    if (!p || check_params(p) != OGG_OK) return -1;
    return layout(*p).total;
}

extern "C" int ogg_basin_check(const ogg_basin_params* p, const ogg_basin_rule* rules) { return check_rules(p, rules); }

extern "C" int ogg_basin_plan(const ogg_basin_params* p, const ogg_basin_rule* rules, int* pass_start, int* n_passes) {
    if (int e = check_rules(p, rules)) return e;
    OGG_REQUIRE(pass_start && n_passes, OGG_EARG, "ogg_basin_plan: null pass_start / n_passes");
    int th = 0, batch = 1;
    if (int e = read_knobs(&th, &batch)) return e;
    std::vector<int> start;
    plan_passes(rules, p->n_rules, batch, &start);
    std::copy(start.begin(), start.end(), pass_start);
    *n_passes = (int)start.size() - 1;
    return OGG_OK;
}

extern "C" int ogg_basin_codes_dev(const ogg_basin_params* p, const ogg_basin_rule* rules, const ogg_basin_rule* rules_dev,
                                   const double* x, const double* y, long ld, const unsigned char* wet, void* workspace,
                                   long workspace_bytes, unsigned char* code, short* rule, ogg_basin_rule_record* records,
                                   ogg_basin_counts* counts, void* stream) {
    if (int e = check_rules(p, rules)) return e;
    OGG_REQUIRE(rules_dev && x && y && wet && code && rule && records && counts, OGG_EARG,
                "ogg_basin_codes: null rules_dev / x / y / wet / code / rule / records / counts");
    OGG_REQUIRE(ld >= 2 * p->nx + 1, OGG_EARG, "ogg_basin_codes: point rows of %ld, %ld needed", ld, 2 * p->nx + 1);
    const Layout l = layout(*p);
    if (int e = ogg::check_workspace("ogg_basin_codes", workspace, workspace_bytes, l.total)) return e;
    int th = 0, batch = 1;
    if (int e = read_knobs(&th, &batch)) return e;
    std::vector<int> start;
    plan_passes(rules, p->n_rules, batch, &start);
    hipStream_t st = ogg::as_stream(stream);
    const long n = p->ny * p->nx;
    const int K = p->n_rules;
    double* u = at<double>(workspace, l.u);
    int* par = at<int>(workspace, l.par);
    int* root = at<int>(workspace, l.root);
    unsigned char* cls = at<unsigned char>(workspace, l.cls);
    int* keep = at<int>(workspace, l.keep);
    unsigned long long* part = at<unsigned long long>(workspace, l.part);
    OGG_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(ogg_basin_counts), st));
    basin_unit_kernel<<<grid_for<NT>(n, 4096), NT, 0, st>>>(p->ny, p->nx, x, y, ld, wet, u, code, rule, counts);
    OGG_LAUNCH_CHECK();
    basin_seed_kernel<<<dim3(l.seed_bx, l.seed_by), NT, 0, st>>>(n, u, K, rules_dev, part);
    OGG_LAUNCH_CHECK();
    basin_seed_reduce_kernel<<<grid_for<NT>(K, 4096), NT, 0, st>>>(K, (int)l.seed_bx, part, records);
    OGG_LAUNCH_CHECK();
    for (size_t q = 0; q + 1 < start.size(); ++q) {
        const Pass ps{start[q], start[q + 1] - start[q]};
        const auto tile = [&](const Grid& g, unsigned tiles) {
            basin_tile_kernel<<<tiles, NT, TW * th * (sizeof(int) + 1), st>>>(g, ps, rules_dev, x, y, ld, wet, code, cls, par);
        };
        if (int e = label_components<false>(p->ny, p->nx, th, p->topology, tile, SameClass{cls}, par, root, nullptr, st)) return e;
        basin_seedroot_kernel<<<1, NT, 0, st>>>(p->nx, ps, p->seed_max_d2, rules_dev, x, y, ld, wet, code, rule, root, records, keep);
        OGG_LAUNCH_CHECK();
        basin_assign_kernel<<<grid_for<NT>(n, 1024), NT, 0, st>>>(n, ps, rules_dev, cls, root, keep, code, rule, records, counts);
        OGG_LAUNCH_CHECK();
    }
    basin_finish_kernel<<<1, 1, 0, st>>>(counts, (long long)start.size() - 1);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

// the host-pointer form: everything copied to device memory, the call, the results copied back (synchronous)
extern "C" int ogg_basin_codes(const ogg_basin_params* p, const ogg_basin_rule* rules, const double* x, const double* y,
                               const unsigned char* wet, unsigned char* code, short* rule, ogg_basin_rule_record* records,
                               ogg_basin_counts* counts) {
    if (int e = check_rules(p, rules)) return e;
    OGG_REQUIRE(x && y && wet && code && rule && records && counts, OGG_EARG, "ogg_basin_codes: null argument");
    ogg::Buffers bufs;   // freed on every exit path
    const size_t nc = (size_t)(p->ny * p->nx), npt = (size_t)(2 * p->ny + 1) * (2 * p->nx + 1), K = (size_t)p->n_rules;
    const long wsb = layout(*p).total;
    double *dx, *dy;
    unsigned char *dw, *dc;
    ogg_basin_rule* dr;
    char* ws;
    short* du;
    ogg_basin_rule_record* dk;
    ogg_basin_counts* ct;
    if (int e = bufs.put(&dx, x, npt)) return e;
    if (int e = bufs.put(&dy, y, npt)) return e;
    if (int e = bufs.put(&dw, wet, nc)) return e;
    if (int e = bufs.put(&dr, rules, K)) return e;
    if (int e = bufs.alloc(&ws, (size_t)wsb)) return e;
    if (int e = bufs.alloc(&dc, nc)) return e;
    if (int e = bufs.alloc(&du, nc)) return e;
    if (int e = bufs.alloc(&dk, K)) return e;
    if (int e = bufs.alloc(&ct, 1)) return e;
    if (int e = ogg_basin_codes_dev(p, rules, dr, dx, dy, 2 * p->nx + 1, dw, ws, wsb, dc, du, dk, ct, nullptr)) return e;
    if (int e = bufs.get(code, dc, nc)) return e;
    if (int e = bufs.get(rule, du, nc)) return e;
    if (int e = bufs.get(records, dk, K)) return e;
    if (int e = bufs.get(counts, ct, 1)) return e;
    return OGG_OK;
}
