/* libogg_hip.so -- C ABI of the MI355X (gfx950) supergrid hot path.
 *
 * The reference (nikizadehgfdl/ocean_model_grid_generator, ocean_grid_generator.py, cited as OGG:<line>) has no
 * FFI: its boundary is the set of Python call sites in main() (OGG:1004-1170).  Each entry point below replaces
 * one of those callees; the Python host (ocean_model_grid_generator_amd/ocean_grid_generator.py) binds them
 * with ctypes under the reference's own function names.
 *
 * Conventions
 *   - all arrays are fp64, C order [j][i], i fastest, densely packed; sizes are given per argument;
 *   - entry points WITHOUT the _dev suffix take HOST pointers (caller-allocated, caller-owned; the library
 *     stages through device memory it allocates and frees inside the call);
 *   - entry points WITH the _dev suffix take DEVICE pointers and a hipStream_t (passed as void*), enqueue
 *     work on that stream alone and return without synchronising; no allocation, no host sync (graph-capturable).
 *     The exceptions, each with "Waits for the stream" in its own comment (tests/test_gpu_streams.py holds every
 *     other entry to the rule on a side stream, tests/test_stream_contract_cpu.py holds this list to its table):
 *       ogg_workspace_error_flag_dev, ogg_supergrid_pass_plan_flags_dev, ogg_supergrid_pass_dev,
 *       ogg_tripolar_pass_dev, ogg_remap_fill_dev, ogg_spread_sets_dev, ogg_layout_blocks_dev;
 *     and the displaced-pole entries when they are given no workspace (workspace = NULL: see their comments).
 *     ogg_supergrid_pass_plan_dev takes no stream: it allocates and waits for the device;
 *   - every function returns OGG_OK or an error code; ogg_last_error() gives the text (thread-local);
 *   - no C++ exception crosses this boundary; calls may come from any thread, one call at a time per stream.
 */
#ifndef OGG_HIP_H
#define OGG_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define OGG_OK 0
#define OGG_EORDER 1 /* "Uncoded order" (OGG:204,222,255) / "order not coded" (OGG:547,562) */
#define OGG_ESHAPE 2 /* "Input arrays do not have the same shape!" (OGG:722) and other size errors */
#define OGG_EHIP 3   /* a HIP runtime call failed (no device, launch failure, ...) */
#define OGG_ENOMEM 4 /* device allocation failed */
#define OGG_EARG 5   /* null pointer / invalid scalar */

#define OGG_DP_ARC_LITERAL 0 /* arc form of the displaced-pole quadrature: see ogg_displaced_pole_metrics_quad_form_sym_ws_dev */
#define OGG_DP_ARC_CHORD 1

/* Mirror symmetry of the two caps (the `symmetry` field of ogg_bipolar_band / ogg_dpole_band, the *_sym_* entry points).
 *   OGG_SYM_MIRROR  evaluate the columns that determine the rest and write their mirror images: the bipolar projection (OGG:33-100) is
 *                   symmetric about its two pole meridians and its fold lines, so a quarter of the columns determines a row; the
 *                   displaced-pole map (OGG:447-467) about the meridian through lon_dp, so half of them does.  The columns where the
 *                   reference's own results are not mirror images of each other to within its own rounding error (next to the fold
 *                   lines, the pole meridians of the mesh, the rows next to the pole points) are still evaluated one by one: DESIGN.md.
 *   OGG_SYM_NONE    every column evaluated, as the reference does (OGG:168-172, 583-584).
 *   OGG_SYM_DEFAULT (0, what a zero-initialised descriptor asks for) the library's default: OGG_SYM_MIRROR unless the environment says
 *                   OGG_CAP_SYMMETRY=0 / none. */
#define OGG_SYM_DEFAULT 0
#define OGG_SYM_MIRROR 1
#define OGG_SYM_NONE 2

const char* ogg_last_error(void);
/* "ogg_hip <version> (gfx950) src <hash>": <hash> = first 12 hex digits of the sha256 over the kernel sources the library was built
 * from (csrc/build.py source_hash()); profiles/valu_counters.json and hbm_traffic.json record the hash they were collected with */
const char* ogg_version(void);
/* sizeof of every struct this header defines, so that a binding can verify its layout: OGG_ABI_<NAME> is the code of ogg_<name>,
 * OGG_ABI_N one past the last; any other value gives -1.  A struct added to this header takes the next code. */
#define OGG_ABI_LATLON_BAND 0
#define OGG_ABI_BIPOLAR_BAND 1
#define OGG_ABI_DPOLE_BAND 2
#define OGG_ABI_QUALITY_EXTREMUM 3
#define OGG_ABI_GRID_QUALITY_RESULT 4
#define OGG_ABI_QUALITY_BAND 5
#define OGG_ABI_TOPOG_SOURCE 6
#define OGG_ABI_TOPOG_BAND 7
#define OGG_ABI_TOPOG_RECORD 8
#define OGG_ABI_TOPOG_PLANE_RECORD 9
#define OGG_ABI_XGRID_ATM 10
#define OGG_ABI_XGRID_BAND 11
#define OGG_ABI_XGRID_COUNTS 12
#define OGG_ABI_MASK_PARAMS 13
#define OGG_ABI_MASK_COUNTS 14
#define OGG_ABI_REMAP_PARAMS 15
#define OGG_ABI_REMAP_COUNTS 16
#define OGG_ABI_RUNOFF_PARAMS 17
#define OGG_ABI_RUNOFF_COUNTS 18
#define OGG_ABI_REGRID_PARAMS 19
#define OGG_ABI_REGRID_COUNTS 20
#define OGG_ABI_BILINEAR_PARAMS 21
#define OGG_ABI_COAST_PARAMS 22
#define OGG_ABI_COAST_COUNTS 23
#define OGG_ABI_BASIN_PARAMS 24
#define OGG_ABI_BASIN_RULE 25
#define OGG_ABI_BASIN_RULE_RECORD 26
#define OGG_ABI_BASIN_COUNTS 27
#define OGG_ABI_XGRID_CS_ATM 28
#define OGG_ABI_XGRID_CS_COUNTS 29
#define OGG_ABI_LAYOUT_PARAMS 30
#define OGG_ABI_LAYOUT_CANDIDATE 31
#define OGG_ABI_LAYOUT_RECORD 32
#define OGG_ABI_LOCATE_PARAMS 33
#define OGG_ABI_LOCATE_COUNTS 34
#define OGG_ABI_TOPOG_PROJECTION 35
#define OGG_ABI_TOPOG_LAYER 36
#define OGG_ABI_TOPOG_MERGE_RECORD 37
#define OGG_ABI_XGRID_CURV_SRC 38
#define OGG_ABI_XGRID_CURV_COUNTS 39
#define OGG_ABI_SPREAD_PARAMS 40
#define OGG_ABI_SPREAD_COUNTS 41
#define OGG_ABI_N 42
long ogg_abi_sizeof(int which);
int ogg_device_count(int* count);
int ogg_set_device(int device);
int ogg_device_name(char* buf, int buflen);

/* ------------------------------------------------------------------------------------------------------
 * Mercator / regular lat-lon builders
 * ---------------------------------------------------------------------------------------------------- */

/* y_mercator_rounded (OGG:309-311, with y_mercator OGG:292-295): y* = sign(y)*round_half_even(|y|),
 * y = R*log((1+sin(phi))/cos(phi)), R = Ni/(2*pi).  phi in radians.  ystar: int64[n]. */
int ogg_y_mercator_rounded(long Ni, long n, const double* phi_rad, long long* ystar);
int ogg_y_mercator_rounded_dev(long Ni, long n, const double* phi_rad, long long* ystar, void* stream);

/* y_mercator (OGG:292-295): the unrounded ordinate y = R*log((1+sin(phi))/cos(phi)) */
int ogg_y_mercator(long Ni, long n, const double* phi_rad, double* y);
int ogg_y_mercator_dev(long Ni, long n, const double* phi_rad, double* y, void* stream);

/* phi_mercator (OGG:298-301): phi = atan(sinh(y/R))*(180/pi), degrees, for arbitrary ordinates y[n]. */
int ogg_phi_mercator(long Ni, long n, const double* y, double* phi_deg);
int ogg_phi_mercator_dev(long Ni, long n, const double* y, double* phi_deg, void* stream);
/* same for the integer ordinates y0, y0+1, ..., y0+n-1 (the axis of OGG:336), no input array */
int ogg_mercator_axis_dev(long Ni, long long y0, long n, double* phi_deg, void* stream);

/* out[k] = a0 + (k*len)/denom, k = 0..n-1: the axes of OGG:113,115,431,834,835 */
int ogg_linear_axis_dev(long n, double a0, double len, double denom, double* out, void* stream);

/* out[k] = a0 + (idx[k]*len)/denom for arbitrary (fractional) indices idx[n]: OGG:126-127, 479-482 */
int ogg_affine_index(long n, const double* idx, double a0, double len, double denom, double* out);
int ogg_affine_index_dev(long n, const double* idx, double a0, double len, double denom, double* out, void* stream);

/* np.tile pair (OGG:430-432, OGG:840-841): x[j][i] = lon1d[i], y[j][i] = lat1d[j]; rows j0..j0+nrows-1 of the
 * lat axis are written to nrows x ni1 outputs. */
int ogg_tile_latlon(long nrows, long ni1, const double* lat1d, const double* lon1d, double* x, double* y);
int ogg_tile_latlon_dev(long nrows, long ni1, const double* lat1d, const double* lon1d, double* x, double* y,
                        void* stream);

/* generate_latlon_grid (OGG:832-846) incl. both axes; skip_first_row=1 reproduces the ensure_nj_even row drop
 * (OGG:836-838).  x, y: (lnj+1-skip_first_row) x (lni+1). */
int ogg_generate_latlon_grid(long lni, long lnj, double llon0, double llen_lon, double llat0, double llen_lat,
                             int skip_first_row, double* x, double* y);

/* ------------------------------------------------------------------------------------------------------
 * MIDAS stencil metrics (OGG:687-716) and grid orientation angle (OGG:719-729), fused
 * ---------------------------------------------------------------------------------------------------- */

/* mdist (OGG:682-684): min(mod(x1-x2,360), mod(x2-x1,360)) with numpy's sign-of-divisor mod, element-wise */
int ogg_mdist(long n, const double* x1, const double* x2, double* out);
int ogg_mdist_dev(long n, const double* x1, const double* x2, double* out, void* stream);

/* x, y: nrows_xy x ni1 point rows.  Writes
 *   dx    [n_pt_rows  ][ni1-1]   (rows 0..n_pt_rows-1)            if dx    != NULL
 *   angle [n_pt_rows  ][ni1  ]                                     if angle != NULL
 *   dy    [n_cell_rows][ni1  ]   (needs point row j+1: n_cell_rows+1 <= nrows_xy)   if dy != NULL
 *   area  [n_cell_rows][ni1-1]                                     if area  != NULL
 * A full sub-grid has n_pt_rows = nrows_xy = nj+1, n_cell_rows = nj.  A latitude band passes its own rows plus one
 * halo row (the first row of the band above) and n_pt_rows = n_cell_rows = nrows_xy-1. */
int ogg_grid_metrics_midas_dev(long nrows_xy, long ni1, const double* x, const double* y, long n_pt_rows,
                               long n_cell_rows, double Re, int latlon_areafix, double* dx, double* dy,
                               double* area, double* angle, void* stream);
/* The kernel ogg_grid_metrics_midas_dev would launch for ni1 columns and n_pt_rows point rows under the current environment (host only, no
 * device is touched): *tile_rows = the instantiation of the LDS-staged tile kernel (4, 6, 8 or 12), or 0 for the streaming kernel
 * (OGG_MIDAS_TILE_ROWS=0); *rows_per_block = the point rows one workgroup walks.  metrics: whether any of dx, dy, area is asked for (the
 * streaming kernel walks at least 4 rows then, at least 1 for an angle-only call).  Both branches aim at OGG_MIDAS_TARGET_WG workgroups
 * (default 2048). */
int ogg_grid_metrics_midas_plan(long ni1, long n_pt_rows, int metrics, int* tile_rows, int* rows_per_block);
/* generate_grid_metrics_MIDAS(x, y, Re, latlon_areafix): dx (nj1 x ni1-1), dy (nj1-1 x ni1), area (nj1-1 x ni1-1) */
int ogg_grid_metrics_midas(long nj1, long ni1, const double* x, const double* y, double Re, int latlon_areafix,
                           double* dx, double* dy, double* area);
/* angle_x(x, y): angle_dx (nj1 x ni1), degrees */
int ogg_angle_x(long nj1, long ni1, const double* x, const double* y, double* angle_dx);

/* Fused builder for sub-grids that are lat-lon by construction (x[j][i] = lon1d[i], y[j][i] = lat1d[j]): writes x, y,
 * angle_dx (n_pt_rows x ni1), dx (n_pt_rows x ni1-1) and dy (n_cell_rows x ni1), area (n_cell_rows x ni1-1) from the two
 * 1-D axes alone; bit-identical to ogg_tile_latlon_dev + ogg_grid_metrics_midas_dev.  lat1d must hold n_pt_rows entries,
 * plus one more when n_cell_rows == n_pt_rows (the row above the band).  metrics = 0 writes only x, y, angle_dx. */
typedef struct {
    int axis_kind;  /* 0: lat[k] = a0 + (k*len)/denom (OGG:835); 1: Mercator, lat[k] = atan(sinh((y0+k)/R))*(180/pi), R = Ni/(2 pi)
                       (OGG:336); 2: lat[k] = lat1d[k] (device array, e.g. the enhanced-equator axis) */
    double a0, len, denom;
    long long y0;
    const double* lat1d;
    long k0;           /* axis index of the band's first point row */
    long n_pt_rows;    /* point rows of the band (x, y, dx, angle_dx) */
    long n_cell_rows;  /* cell rows of the band (dy, area); row n_cell_rows of the axis must exist when == n_pt_rows */
    double *x, *y, *dx, *dy, *area, *angle;
} ogg_latlon_band;
/* Up to 4 lat-lon bands in one launch, axes evaluated in the kernel: lon[i] = lon0 + (i*lenlon)/(ni1-1) (OGG:431, 834). */
int ogg_latlon_supergrid_multi_dev(int n_bands, const ogg_latlon_band* bands, long ni1, double lon0, double lenlon, double Re,
                                   int metrics, void* stream);
/* The same fields, the same bits, for launches that carry nothing but lat-lon sub-grids: the unit of work is one ROW of one FIELD and
 * units are taken in (band, field, row) order, so the chip writes a compact window that sweeps through one array at a time -- the
 * pattern its HBM write path rewards -- fed from a row table and a column table built by a first small launch in the caller's
 * workspace (>= ogg_latlon_rows_workspace_bytes bytes of device memory).  Two launches, no allocation. */
long ogg_latlon_rows_workspace_bytes(int n_bands, const ogg_latlon_band* bands, long ni1);
int ogg_latlon_supergrid_rows_ws_dev(int n_bands, const ogg_latlon_band* bands, long ni1, double lon0, double lenlon, double Re,
                                     int metrics, void* workspace, long workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Murray bipolar Arctic cap
 * ---------------------------------------------------------------------------------------------------- */

/* bipolar_projection (OGG:33-100), element-wise over n points.  metrics_only != 0: lams, phis may be NULL. */
int ogg_bipolar_projection(long n, const double* lamg, const double* phig, double lon_bp, double rp,
                           int metrics_only, double* lams, double* phis, double* h_i_inv, double* h_j_inv);
int ogg_bipolar_projection_dev(long n, const double* lamg, const double* phig, double lon_bp, double rp,
                               int metrics_only, double* lams, double* phis, double* h_i_inv, double* h_j_inv,
                               void* stream);

/* generate_bipolar_cap_mesh (OGG:103-122), rows j0..j0+nrows-1 of the (Nj+1) x (Ni+1) mesh, one launch.
 *   lams, phis   nrows x (Ni+1)
 *   h_i_inv      nrows x Ni, h_j_inv: nrows x (Ni+1), already scaled as OGG:119-120 (h_j_inv row Nj is computed but dropped by the
 *                reference; rows >= Nj are not written); either may be NULL
 *   angle_dx     angle_x(lams, phis) (OGG:719-729) of the same rows, nrows x (Ni+1), without reading the mesh back; NULL to skip
 *   symmetry     OGG_SYM_* (top of this file).  Mirrored, the columns [0, Ni/4] (+ 2 degrees beyond the pole meridian) are evaluated and
 *                written to their three images, the columns next to the fold lines and within 2 degrees of the pole meridians at their
 *                own positions
 * No workspace, no allocation. */
int ogg_bipolar_cap_mesh_angle_sym_dev(long Ni, long Nj, double lat0_bp, double lon_bp, long j0, long nrows, int symmetry, double* lams,
                                       double* phis, double* h_i_inv, double* h_j_inv, double* angle_dx, void* stream);
/* the whole mesh into host arrays, under the reference's own name (symmetry = OGG_SYM_DEFAULT) and with the symmetry stated */
int ogg_bipolar_cap_mesh(long Ni, long Nj, double lat0_bp, double lon_bp, double* lams, double* phis,
                         double* h_i_inv, double* h_j_inv);
int ogg_bipolar_cap_mesh_sym(long Ni, long Nj, double lat0_bp, double lon_bp, int symmetry, double* lams, double* phis,
                             double* h_i_inv, double* h_j_inv);

/* bipolar_cap_ij_array (OGG:125-133): per-index arc lengths (radians) at fractional indices i[n_i], j[n_j];
 * h_i_inv, h_j_inv: n_j x n_i */
int ogg_bipolar_cap_ij_array(long n_i, const double* i, long n_j, const double* j, long Ni, long Nj, double lat0_bp,
                             double lon_bp, double rp, double* h_i_inv, double* h_j_inv);
int ogg_bipolar_cap_ij_array_dev(long n_i, const double* i, long n_j, const double* j, long Ni, long Nj, double lat0_bp,
                                 double lon_bp, double rp, double* h_i_inv, double* h_j_inv, void* stream);

/* bipolar_cap_metrics_quad_fast (OGG:136-188): Gauss-Lobatto quadrature (order 2..5) of the analytic scale factors of an
 * (ny+1) x (nx+1) cap.
 *   rows         a band: dxq rows j0..j0+n_dx_rows-1 of (ny+1) x nx; dyq rows j0..j0+n_cell_rows-1 of ny x (nx+1); daq rows
 *                j0..j0+n_cell_rows-1 of ny x nx.  n_dx_rows = n_cell_rows, or n_cell_rows + 1 on the band that holds row ny.  The whole
 *                cap is j0 = 0, n_dx_rows = ny + 1, n_cell_rows = ny
 *   workspace    device memory for the row / column tables, at least ogg_bipolar_quad_workspace_bytes bytes: no allocation of any kind
 *                inside the call, so it can be captured into a HIP graph.  workspace = NULL, workspace_bytes = 0: the tables come from
 *                the stream-ordered allocator (hipMallocAsync / hipFreeAsync)
 *   symmetry     OGG_SYM_* (top of this file).  Mirrored, the rows below 88.2 degrees are evaluated on the cells [0, nx/4) and next to
 *                the fold lines (6 degrees either side of the columns 0 and nx/2) and written to their images; replaces the column
 *                loop of OGG:168-172 for those rows */
long ogg_bipolar_quad_workspace_bytes(int order, long nx, long ny);
int ogg_bipolar_cap_metrics_quad_sym_ws_dev(int order, long nx, long ny, double lat0_bp, double lon_bp, double rp, double Re,
                                            long j0, long n_dx_rows, long n_cell_rows, int symmetry, double* dxq, double* dyq, double* daq,
                                            void* workspace, long workspace_bytes, void* stream);
/* the whole cap into host arrays, under the reference's own name (symmetry = OGG_SYM_DEFAULT) and with the symmetry stated */
int ogg_bipolar_cap_metrics_quad(int order, long nx, long ny, double lat0_bp, double lon_bp, double rp, double Re,
                                 double* dxq, double* dyq, double* daq);
int ogg_bipolar_cap_metrics_quad_sym(int order, long nx, long ny, double lat0_bp, double lon_bp, double rp, double Re, int symmetry,
                                     double* dxq, double* dyq, double* daq);

/* The band of a bipolar cap in a pass (ogg_tripolar_pass_dev, ogg_supergrid_pass_dev below): mesh, angle_dx and quadrature of its
 * rows.  Results are bit-identical to ogg_bipolar_cap_mesh_angle_sym_dev + ogg_bipolar_cap_metrics_quad_sym_ws_dev on the same band. */
typedef struct ogg_bipolar_band {
    long Ni, Nj;             /* the cap is (Nj+1) x (Ni+1) points */
    double lat0_bp, lon_bp;  /* OGG:103 */
    double rp, Re;           /* OGG:117; sphere radius */
    int order;               /* Gauss-Lobatto order of the quadrature, 2..5 (OGG:191-204) */
    int symmetry;            /* OGG_SYM_DEFAULT (0), OGG_SYM_MIRROR or OGG_SYM_NONE: mesh and quadrature from a quarter of the columns */
    long j0;                 /* first mesh row of the band */
    long n_pt_rows;          /* point rows: x, y, angle (n_pt_rows x (Ni+1)), dx (n_pt_rows x Ni) */
    long n_cell_rows;        /* cell rows: dy (n_cell_rows x (Ni+1)), area (n_cell_rows x Ni); n_pt_rows - 1 on the band that
                                holds row Nj, else n_pt_rows */
    double *x, *y, *angle, *dx, *dy, *area;
    void* workspace;         /* >= ogg_bipolar_quad_workspace_bytes(order, Ni, Nj) bytes of device memory (metrics only): tables,
                                fix-up list, claim counters of the lat-lon strips; one pass at a time per workspace */
    long workspace_bytes;
} ogg_bipolar_band;

/* ------------------------------------------------------------------------------------------------------
 * Displaced-pole Southern cap
 * ---------------------------------------------------------------------------------------------------- */

/* displacedPoleCap_mesh (OGG:488-506) at index vectors i[n_i], j[n_j] (may be fractional), including the
 * sequential 360-degree unwrap along i (monotonic_bounding, OGG:470-475).  lams, phis: n_j x n_i. */
int ogg_displaced_pole_mesh_dev(long n_i, const double* i, long n_j, const double* j, long ni, long nj, double lon0,
                                double lat0, double lam_pole, double r_pole, double* lams, double* phis,
                                void* stream);
int ogg_displaced_pole_mesh(long n_i, const double* i, long n_j, const double* j, long ni, long nj, double lon0,
                            double lat0, double lam_pole, double r_pole, double* lams, double* phis);
/* displacedPoleCap_projection (OGG:447-467) on explicit lon/lat grids (nj x ni) with z_0 = z0_re + i z0_im and
 * r_joint given; x_0 is the seed of the unwrap (the reference passes lon_grid[0,0], OGG:463). */
int ogg_displaced_pole_projection(long nj, long ni, const double* lon_grid, const double* lat_grid, double z0_re,
                                  double z0_im, double r_joint, double x_0, double* lam, double* phi);
int ogg_displaced_pole_projection_dev(long nj, long ni, const double* lon_grid, const double* lat_grid, double z0_re,
                                      double z0_im, double r_joint, double x_0, double* lam, double* phi, void* stream);
/* monotonic_bounding (OGG:470-475), in place on x (nj x ni) */
int ogg_monotonic_bounding(long nj, long ni, double* x, double x_0);
int ogg_monotonic_bounding_dev(long nj, long ni, double* x, double x_0, void* stream);
/* the haversine of great_arc_distance (OGG:527-532), element-wise; inputs in degrees, output in radians */
int ogg_haversine(long n, const double* lam0, const double* phi0, const double* lam1, const double* phi1, double* out);
int ogg_haversine_dev(long n, const double* lam0, const double* phi0, const double* lam1, const double* phi1, double* out,
                      void* stream);

/* generate_displaced_pole_grid (OGG:509-518), rows j0..j0+nrows-1 of (Nj+1) x (Ni+1), one launch after a small reset: projection and
 * the sequential unwrap of monotonic_bounding (a look-back scan over the column strips of a row).
 *   x, y         nrows x (Ni+1)
 *   angle_dx     angle_x (OGG:719-729) of the same rows, nrows x (Ni+1), without reading the mesh back; NULL to skip
 *   workspace    device memory, at least ogg_displaced_pole_grid_workspace_bytes bytes (its first two 32-bit words are the work counter
 *                and an error flag, see ogg_workspace_error_flag_dev): nothing is allocated.  workspace = NULL, workspace_bytes = 0: the
 *                stream-ordered allocator, and the call waits for the stream to check the flag itself
 * Every column is evaluated: the mesh has no mirrored form. */
long ogg_displaced_pole_grid_workspace_bytes(long Ni, long nrows);
int ogg_displaced_pole_grid_angle_ws_dev(long Ni, long Nj, double lon0, double lat0, double lon_dp, double r_dp, long j0,
                                         long nrows, double* x, double* y, double* angle_dx, void* workspace,
                                         long workspace_bytes, void* stream);
/* Error flag of a workspace used by a displaced-pole call (*flag != 0: a look-back wait gave up, the results of that call are
 * invalid; never observed, the spin is bounded so that a grid always drains).  Waits for the stream: the flag is read on the host. */
int ogg_workspace_error_flag_dev(const void* workspace, int* flag, void* stream);

/* numerical_hi / numerical_hj (OGG:535-562; great_arc_distance OGG:522-532) on the lattice j[n_j] x i[n_i].
 * fd_order in {2,4,6}.  h_i, h_j: n_j x n_i (either may be NULL). */
int ogg_displaced_pole_numerical_h_dev(long n_i, const double* i, long n_j, const double* j, long nx, long ny,
                                       double lon0, double lat0, double lon_dp, double r_dp, double eps,
                                       int fd_order, double* h_i, double* h_j, void* stream);
int ogg_displaced_pole_numerical_h(long n_i, const double* i, long n_j, const double* j, long nx, long ny,
                                   double lon0, double lat0, double lon_dp, double r_dp, double eps, int fd_order,
                                   double* h_i, double* h_j);

/* displacedPoleCap_metrics_quad (OGG:565-601) of an (ny+1) x (nx+1) cap: quadrature order (2..5) is also the finite-difference order,
 * as in the reference (OGG:583-584), so only orders 2 and 4 are valid.
 *   rows         a band, as for the bipolar cap: dxq rows j0..j0+n_dx_rows-1 of (ny+1) x nx; dyq rows j0..j0+n_cell_rows-1 of
 *                ny x (nx+1); daq rows j0..j0+n_cell_rows-1 of ny x nx; n_dx_rows = n_cell_rows, or n_cell_rows + 1 on the band that
 *                holds row ny.  Cell rows below j0 are simply not evaluated (main() discards the doughnut rows, OGG:1177-1186)
 *   workspace    device memory for the row / column tables and the look-back words, at least
 *                ogg_displaced_pole_quad_workspace_bytes(order, nx, n_cell_rows) bytes (a few MB -- the lattice itself is never
 *                stored): no allocation inside the call; one call at a time per workspace.  workspace = NULL, workspace_bytes = 0: the
 *                stream-ordered allocator; the literal form then waits for the stream to check the error flag itself
 *   symmetry     OGG_SYM_* (top of this file).  Mirrored (chord form only, when the meridian of the displaced pole is a node column,
 *                (lon_dp - lon0) nx / 360 an integer, and nx is even): the half of the columns on one side of that meridian is
 *                evaluated and written to its mirror images (OGG:583-584 evaluate every column)
 * arc_form selects how the great-arc distance between two probes of the finite-difference stencil is taken:
 *   OGG_DP_ARC_CHORD    the finite-difference stencil of the reference, distance of two probes from their positions on the sphere (no
 *                       atan2, no unwrap): ~6x less arithmetic than the literal form, and closer to what the reference's formula means
 *                       (below).  Since round 4 THE default: what ogg_displaced_pole_metrics_quad runs, and what the
 *                       Python host (main(), displacedPoleCap_metrics_quad, SupergridPlan, bench.py) asks for unless OGG_DP_ARC /
 *                       dp_arc / arc_form says literal;
 *   OGG_DP_ARC_LITERAL  the reference's operation sequence (haversine of the projected, unwrapped longitudes and latitudes,
 *                       OGG:522-532): opt-in through the arc_form argument and the band descriptor of the pass.
 * Measured on the 5760 x 560 cap of BASELINE config 4 (1/8 degree), max relative difference of dx / dy / area
 *   from the numpy oracle (profiles/dp_parity.json):             literal 1.3e-9 / 1.2e-9 / 7.6e-10   chord 1.5e-9 / 1.3e-9 / 9.8e-10
 *   from a 50-digit evaluation of the reference's own formula on 10 500 cells (tests/golden/truth_table.npz, tests/test_gpu_truth.py,
 *   profiles/r04_truth_table.json):   the fp64 reference itself 1.4e-9 / 9.0e-10 / 1.2e-9   literal 1.4e-9 / 8.5e-10 / 1.2e-9
 *                                     chord 7.6e-10 / 2.7e-10 / 8.3e-10
 * Both grow with the resolution (7e-12 at Ni = 72): the reference differentiates an arc of 2e-3 index units numerically, so ONE ulp of
 * atan2 is amplified by ~Ni / (4e-3 pi); the fp64 reference is itself that far from the exact value of its formula, and the chord form,
 * which never forms a longitude, is the closest of the three.  The literal form is not bit-identical to a CPU run either, because the
 * transcendental functions are not (the restatements of atan / atan2 used here reproduce the bits of the ROCm 7.2 device library,
 * ogg_libm_check_dev).
 * (OGG_DP_ARC_LITERAL = 0, OGG_DP_ARC_CHORD = 1: defined next to the error codes at the top of this file) */
long ogg_displaced_pole_quad_workspace_bytes(int order, long nx, long n_cell_rows);
int ogg_displaced_pole_metrics_quad_form_sym_ws_dev(int arc_form, int symmetry, int order, long nx, long ny, double lon0, double lat0,
                                                    double lon_dp, double r_dp, double Re, long j0, long n_dx_rows, long n_cell_rows,
                                                    double* dxq, double* dyq, double* daq, void* workspace, long workspace_bytes,
                                                    void* stream);
/* the whole cap into host arrays, under the reference's own name (arc_form = OGG_DP_ARC_CHORD, symmetry = OGG_SYM_DEFAULT) and with both
 * stated */
int ogg_displaced_pole_metrics_quad(int order, long nx, long ny, double lon0, double lat0, double lon_dp, double r_dp,
                                    double Re, double* dxq, double* dyq, double* daq);
int ogg_displaced_pole_metrics_quad_form_sym(int arc_form, int symmetry, int order, long nx, long ny, double lon0, double lat0, double lon_dp,
                                             double r_dp, double Re, double* dxq, double* dyq, double* daq);

/* The band of a displaced-pole southern cap in a pass (ogg_supergrid_pass_dev below): mesh, angle_dx and quadrature of its rows.
 * Results are bit-identical to ogg_displaced_pole_grid_angle_ws_dev + ogg_displaced_pole_metrics_quad_form_sym_ws_dev on the same band. */
typedef struct ogg_dpole_band {
    long Ni, Nj;                 /* the cap is (Nj+1) x (Ni+1) points (OGG:509) */
    double lon0, lat0;           /* OGG:478: first longitude, latitude of the joint with the Southern Ocean sub-grid */
    double lon_dp, r_dp;         /* OGG:495: longitude and radius of the displaced pole */
    double Re;
    int order;                   /* Gauss-Lobatto order of the quadrature = finite-difference order: 2 or 4 (OGG:583-584) */
    int arc_form;                /* OGG_DP_ARC_LITERAL or OGG_DP_ARC_CHORD */
    long j0;                     /* first mesh row of the band (rows below the doughnut cut are simply never asked for) */
    long n_pt_rows;              /* point rows: x, y, angle (n_pt_rows x (Ni+1)), dx (n_pt_rows x Ni) */
    long n_cell_rows;            /* cell rows: dy (n_cell_rows x (Ni+1)), area (n_cell_rows x Ni); n_pt_rows - 1 on the band that holds
                                    row Nj, else n_pt_rows */
    double *x, *y, *angle, *dx, *dy, *area;
    void* workspace;             /* >= ogg_dpole_band_workspace_bytes(order, Ni, n_pt_rows) bytes of device memory */
    long workspace_bytes;
    int symmetry;                /* OGG_SYM_DEFAULT (0), OGG_SYM_MIRROR or OGG_SYM_NONE: the chord-form quadrature from half of the columns */
} ogg_dpole_band;
long ogg_dpole_band_workspace_bytes(int order, long Ni, long n_pt_rows);
/* Host-side check of the mirrored kernels' column spaces (no GPU): replays the index arithmetic the kernels use for one row of a cap with n
 * cells -- which = 0 the bipolar quadrature, 1 the bipolar mesh, 2 the displaced-pole quadrature in the chord form (order 2 or 4; lon0,
 * lon_dp: the meridian of the displaced pole) -- and counts how often every cell (cell_writes[n]; NULL for which = 1) and every node column
 * (col_writes[n + 1]) is written, and how many are evaluated.  Every count must be 1 whatever `symmetry` (OGG_SYM_*). */
int ogg_symmetry_coverage(int which, int order, long n, double lon0, double lon_dp, int symmetry, int* cell_writes, int* col_writes,
                          long* evaluated);

/* The pass: one rank's share of a whole supergrid -- the lat-lon sub-grids, the bipolar cap and the displaced-pole southern cap generated
 * by the sub-grid loop of main() (OGG:1100-1313: generate_mercator_grid / generate_latlon_grid; generate_bipolar_cap_mesh + angle_x +
 * bipolar_cap_metrics_quad_fast; the SC branch, OGG:1158-1197: generate_displaced_pole_grid + angle_x + displacedPoleCap_metrics_quad)
 * -- in three launches on one stream: the HBM-bound lat-lon row strips and the VALU-bound cap workgroups share each launch, so nothing
 * waits on a cross-stream dependency.  The southern cap's tables and the reset of its look-back words join launch A, its mesh + angle
 * workgroups and -- in the chord form -- its quadrature strips join launch B; the literal form of its quadrature is a fourth launch (D).
 * Results are bit-identical to ogg_latlon_supergrid_multi_dev and the caps' own entry points (above each band struct) on the same bands.
 *   cap, south_cap  either may be NULL: no rows of that cap on this rank
 *   metrics         0 writes coordinates and angle_dx only
 *   events5         NULL, or 5 events from ogg_event_create (entries may be NULL), recorded on the stream before A and after A, B, C, D,
 *                   so that the caller can time the launches (ogg_event_elapsed_ms)
 *   alg_bytes4      NULL, or 4 doubles on the host: the bytes each launch writes (its share of the 48 B per cell)
 * Waits for the stream: the call is plan + run + destroy (below), and the destroy waits for the run before it frees the plan's own
 * workspaces.  A caller that must not wait keeps a plan (ogg_supergrid_pass_plan_dev, ogg_supergrid_pass_run_dev). */
int ogg_supergrid_pass_dev(int n_latlon, const ogg_latlon_band* latlon, long ni1, double lon0, double lenlon, double Re, int metrics,
                           const ogg_bipolar_band* cap, const ogg_dpole_band* south_cap, void** events5, double* alg_bytes4,
                           void* stream);
/* the pass without a southern cap: ogg_supergrid_pass_dev with south_cap, events5 and alg_bytes4 NULL.  Waits for the stream, as it does. */
int ogg_tripolar_pass_dev(int n_latlon, const ogg_latlon_band* latlon, long ni1, double lon0, double lenlon, double Re,
                          int metrics, const ogg_bipolar_band* cap, void* stream);
/* ogg_supergrid_pass_dev in two steps, for a caller that runs the pass of one set of bands many times (a rank's step loop): the plan holds the kernel
 * parameters of the launches, their grid sizes and the tiling knobs (the OGG_* environment variables are read when the plan is BUILT), so
 * that a run costs the host its launches and nothing else -- no validation, no planning, no getenv.  The band descriptors are copied:
 * they may be freed after ogg_supergrid_pass_plan_dev returns; the buffers and workspaces they point to must stay.  The runs of a plan
 * go to ONE stream at a time (switch streams only after synchronising the old one) and come from one host thread.
 * ogg_supergrid_pass_dev == plan + run + destroy, without what follows.
 *
 * The tables of the next pass ride in launch B.  With metrics (or a displaced-pole cap) the first launch of a pass writes only the cap
 * workspaces -- tables, cleared look-back words and counters -- and what it writes does not depend on the pass before it.  A plan
 * therefore owns TWO workspaces per cap (device allocations of its own, of the size of the caller's -- their contents outlive a run,
 * so the caller's workspace, which other entry points may use between two runs, is left alone; OGG_PASS_SLOTS=1, read when the plan is
 * built, turns this off: one slot, the caller's) and the last workgroups of launch B of one pass do launch A's work for
 * the next pass in the other slot; that pass then starts with launch B.  One packet less per pass on the stream (3-4.5 us), no second
 * stream, no flag and no wait: the stream's order is the dependence.  Every pass still builds one set of tables; the first pass of a
 * plan, and a pass that records events (events5 != NULL, so that they time it), run launch A themselves; the tables the LAST pass of a
 * plan built for a successor that never came are wasted (a few microseconds).  What the caller sees is unchanged: the outputs of a run
 * are complete when `stream` has executed it (a pass captured into a HIP graph: when a replay has executed; such a graph must not be
 * replayed after ogg_supergrid_pass_plan_destroy, which then waits for the whole device rather than for the last stream), and nothing of
 * pass k + 1 reaches an output array during pass k (the one output launch
 * A writes, the j = ny row of the bipolar dx, goes through the workspace and is copied by the tail launch); results are bit-identical
 * with one slot or two.  ogg_supergrid_pass_plan_destroy waits for the device. */
int ogg_supergrid_pass_plan_dev(int n_latlon, const ogg_latlon_band* latlon, long ni1, double lon0, double lenlon, double Re, int metrics,
                                const ogg_bipolar_band* cap, const ogg_dpole_band* south_cap, void** plan_out);
int ogg_supergrid_pass_run_dev(void* plan, void** events5, double* alg_bytes4, void* stream);
int ogg_supergrid_pass_plan_destroy(void* plan);
long ogg_supergrid_pass_plan_slots(const void* plan);          /* workspace slots of the plan: 2, or 1 (every pass runs its own launch A) */
long ogg_supergrid_pass_plan_carried_runs(const void* plan);   /* runs so far that started with launch B */
/* Waits for the stream, then *flags = bit 1 / bit 2: a look-back wait of the displaced-pole mesh / quadrature timed out, in either slot, in
 * a pass since the slot's words were last cleared.  Results of such a pass are invalid; never observed. */
int ogg_supergrid_pass_plan_flags_dev(const void* plan, int* flags, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Device utilities used by the band-sharded pipeline (bench / multi-GPU)
 * ---------------------------------------------------------------------------------------------------- */
int ogg_fill_dev(long n, double value, double* out, void* stream);
/* Byte-swap-on-copy for write_nc's big-endian output (NetCDF classic, OGG:773-829): dst[k] = bswap64(src[k]), k < n.  src is device
 * memory; dst is device memory or pinned host memory (hipHostMalloc / torch pin_memory), into which the kernel stores directly. */
int ogg_bswap64_dev(long n, const void* src, void* dst, void* stream);
/* Self-test of the device-library functions the kernels restate with their coefficients as scalar operands (ogg_math.h,
 * ogg_bipolar_dev.h): which = 0: asin on [0, 1] (x); 1: atan (x, any); 2: atan2(y, x), finite; 3: 1.0 / x and 4: sqrt(x) without
 * scaling and special cases, 2^-700 <= x <= 2^700; 5: y / x without scaling, 2^-300 <= |x|, |y| <= 2^300 or y = +-0; 6: atan (x) and
 * 7: atan2(y, x) with their coefficients in vector registers (the literal displaced-pole quadrature's forms); 9: atan2(y, x) for ANY
 * arguments, infinities and NaNs included (the generic stencil kernel's form; two NaNs count as equal); 13 / 14: mdist(x, y) (OGG:682-684) from
 * one reduction (the generic stencil kernel's form) / from two, against numpy.mod's own fmod form.  (8, 10, 11, 12 -- restatements that no kernel uses any more -- were removed with them in round 4: OGG_EARG.)  The number of k < n for which the
 * restatement differs IN ANY BIT from the library's own function is ADDED to *n_diff (device memory, 8 bytes, zeroed by the caller). */
int ogg_libm_check_dev(int which, long n, const double* x, const double* y, unsigned long long* n_diff, void* stream);
/* Test-only evaluation of the scalar device helpers that DEPART from the library on purpose (ogg_math.h, ogg_bipolar_dev.h,
 * ogg_dpole_dev.h), and of the library functions they fall back to: out[k] = helper(x[k] [, y[k]]), the helper's VALUE, so that a test can
 * hold it against an extended-precision truth (tests/test_gpu_math_helpers.py).  Element k is computed by thread k of 256-thread
 * workgroups: the 64 consecutive elements 64 w .. 64 w + 63 share wave w, so the caller decides what every wave sees -- several helpers
 * choose between their own form and the library's by one ballot per wave.  The threads behind n of the last wave recompute element n - 1
 * (they take part in the ballots and the lane shifts with a value the wave already holds); only OGG_MATH_WAVE_PREV_TAIL / _NEXT_TAIL let
 * them return first.  x, y, out: device memory, n doubles each (y may be NULL for the one-argument codes).
 *   OGG_MATH_XCD_CONTIGUOUS: b = x[k], n = y[k] (integers held in doubles); the result is an integer held in a double.
 *   OGG_MATH_HOM_ARC / _HOM_TAN: s = x[k], w = y[k], a power of two of either sign: homogeneous_arc (its tangent) of a = (0, 0, |w|) and
 *   b = (s |w|, 0, |w|) for w > 0, (0, s |w|, |w|) for w < 0 -- the family whose cross products are exact, tan(theta) = |s|. */
#define OGG_MATH_DIV_PI180 0
#define OGG_MATH_RCP_C3 1
#define OGG_MATH_RSQRT_C3 2
#define OGG_MATH_ATAN_SERIES14 3
#define OGG_MATH_ATAN_SERIES17 4
#define OGG_MATH_ATAN_CAP 5
#define OGG_MATH_ATAN2_ANGLE 6      /* atan2_angle(y[k], x[k]) */
#define OGG_MATH_WAVE_PREV 7
#define OGG_MATH_WAVE_NEXT 8
#define OGG_MATH_WAVE_PREV_TAIL 9   /* the threads behind n have returned before the shift */
#define OGG_MATH_WAVE_NEXT_TAIL 10
#define OGG_MATH_XCD_CONTIGUOUS 11
#define OGG_MATH_LIB_ATAN 12        /* the device library's atan */
#define OGG_MATH_ATAN_LIB 13        /* atan_lib, its restatement */
#define OGG_MATH_WAVE_NEXT_INT 14   /* the int overload of wave_next on (int)x[k] */
#define OGG_MATH_SIN_TINY 32
#define OGG_MATH_ASIN_TINY 33
#define OGG_MATH_COS_CAP 34
#define OGG_MATH_HOM_ARC 35
#define OGG_MATH_HOM_TAN 36         /* homogeneous_tan, the tangent homogeneous_arc forms */
#define OGG_MATH_LIB_SIN 37         /* the device library's sin, asin, cos (the out-of-line copies the helpers fall back to) */
#define OGG_MATH_LIB_ASIN 38
#define OGG_MATH_LIB_COS 39
int ogg_math_eval_dev(int which, long n, const double* x, const double* y, double* out, void* stream);
/* The five sums behind metrics_error (OGG:732-770) of one sub-grid band, on the device and deterministic:
 * out5 = { sum(area), sum(dy[:, col_a]), sum(dy[:, col_b]) (0 when col_b < 0), sum(dx[0, :]) if want_first_row,
 * sum(dx[n_dx_rows-1, :]) if want_last_row }.  dx: n_dx_rows x ni, dy: n_cell_rows x (ni+1), area: n_cell_rows x ni; out5 is a
 * device pointer.  A band-sharded run adds the out5 of all ranks (one all-reduce) and evaluates OGG:735-770 on the host. */
int ogg_metrics_sums_dev(long n_dx_rows, long n_cell_rows, long ni, const double* dx, const double* dy, const double* area,
                         long col_a, long col_b, int want_first_row, int want_last_row, double* out5, void* stream);
/* ------------------------------------------------------------------------------------------------------
 * Grid-quality report (an addition: the reference has no such check).  One read-only pass over the STITCHED supergrid as
 * written to the file: x, y, angle_dx nyp x nxp, dx nyp x nx, dy ny x nxp, area ny x nx (nxp = nx + 1, ny = nyp - 1).
 * P(j, i) = (cos y cos x, cos y sin x, sin y), x and y in degrees.  An edge or chord shorter than OGG_QUALITY_DEGENERATE_M is
 * degenerate: counted, and left out of every minimum, ratio and angle.  Items, each indexed (j, i) in the written arrays:
 *   sizes        min over non-degenerate (area: non-zero) values and max of dx, dy, area
 *   aspect       cell (j, i): a = (dx[j,i] + dx[j+1,i]) / 2, b = (dy[j,i] + dy[j,i+1]) / 2, max(a/b, b/a)
 *   corner       SW corner of cell (j, i): chords A = P(j,i+1) - P(j,i), B = P(j+1,i) - P(j,i) projected onto the tangent plane at
 *                P(j,i); delta = |angle(A', B') - 90 deg|, evaluated as atan2(|A'.B'|, |A' x B'|)
 *   rx           max(dx[j,i+1] / dx[j,i], inverse), i + 1 taken periodically (the pair (nx-1, 0) is reported at i = nx-1)
 *   ry           max(dy[j+1,i] / dy[j,i], inverse), reported at the lower row j
 *   ry_next      ry of the pair (last cell row of a band, first cell row of the band that follows it): at a sub-grid joint, the
 *                jump in dy across the joint
 *   seam         Re |P_seam(i) - P(next row, i)| in metres: the lower sub-grid's own last point row (which stitching drops) against
 *                the upper sub-grid's first one
 * Extrema tie to the smallest (j, i); no floating-point sum is taken anywhere, so a result is bit-identical whatever the split of the
 * grid into bands and blocks.
 * ---------------------------------------------------------------------------------------------------- */
#define OGG_QUALITY_DEGENERATE_M 1.0e-3
#define OGG_QUALITY_N_BINS 7 /* corner-delta histogram: [0, 1e-6), [1e-6, 1e-3), ..., [20, inf) degrees */
#define OGG_QUALITY_BIN_EDGES_DEG {1.0e-6, 1.0e-3, 0.1, 1.0, 5.0, 20.0}
enum {
    OGG_Q_DX_MIN = 0, OGG_Q_DX_MAX, OGG_Q_DY_MIN, OGG_Q_DY_MAX, OGG_Q_AREA_MIN, OGG_Q_AREA_MAX, OGG_Q_ASPECT_MAX, OGG_Q_DELTA_MAX,
    OGG_Q_RX_MAX, OGG_Q_RY_MAX, OGG_Q_RY_NEXT_MAX, OGG_Q_SEAM_MAX, OGG_Q_N_EXTREMA
};
enum {
    OGG_Q_N_DX = 0,           /* dx values seen */
    OGG_Q_N_DX_DEGENERATE,
    OGG_Q_N_DY,
    OGG_Q_N_DY_DEGENERATE,
    OGG_Q_N_AREA,
    OGG_Q_N_AREA_ZERO,
    OGG_Q_N_CORNERS,          /* corners seen (degenerate ones included) */
    OGG_Q_N_CORNER_DEGENERATE,
    OGG_Q_HIST,               /* OGG_QUALITY_N_BINS counts from here */
    OGG_Q_N_COUNTS = OGG_Q_HIST + OGG_QUALITY_N_BINS
};
/* one extremum: j < 0 when nothing was seen (value is then meaningless); lon, lat = x[j, i], y[j, i].  The corner extremum
 * (OGG_Q_DELTA_MAX) holds tan(delta) = |A'.B'| / |A' x B'|, which delta is monotonic in; degrees(atan(value)) is delta. */
typedef struct ogg_quality_extremum {
    double value, lon, lat;
    long long j, i;
} ogg_quality_extremum;
typedef struct ogg_grid_quality_result {
    ogg_quality_extremum ext[OGG_Q_N_EXTREMA];
    long long count[OGG_Q_N_COUNTS];
} ogg_grid_quality_result;
/* A band: point rows j0 .. j0 + n_pt_rows - 1 of the stitched grid (x, y, dx; row strides nx + 1, nx + 1, nx) and cell rows
 * j0 .. j0 + n_cell_rows - 1 (dy, area; strides nx + 1, nx), n_cell_rows = n_pt_rows, or n_pt_rows - 1 for the band that ends the
 * grid.  The cells of the last row need point row j0 + n_pt_rows (x_next, y_next, dx_next: required when n_cell_rows = n_pt_rows) and
 * cell row j0 + n_cell_rows (dy_next: NULL where the grid has no such row).  x_seam, y_seam (or NULL): the dropped last point row of
 * the sub-grid this band ends, compared with x_next, y_next.  metrics = 0 (--skip_metrics): dx, dy, area are not read and every item
 * that needs them is left empty. */
typedef struct ogg_quality_band {
    long nx, j0, n_pt_rows, n_cell_rows;
    const double *x, *y, *dx, *dy, *area;
    const double *x_next, *y_next, *dx_next, *dy_next;
    const double *x_seam, *y_seam;
    double Re;
    int metrics;
} ogg_quality_band;
long ogg_grid_quality_workspace_bytes(long nx, long n_pt_rows);
/* device pointers throughout: the band's result into *out (device memory); the workspace (device memory, at least
 * ogg_grid_quality_workspace_bytes) holds one record per workgroup, merged in workgroup order by a second kernel */
int ogg_grid_quality_band_dev(const ogg_quality_band* band, void* workspace, long workspace_bytes, ogg_grid_quality_result* out,
                              void* stream);
/* the same with HOST pointers in *band, staged through device memory; *out is host memory */
int ogg_grid_quality(const ogg_quality_band* band, ogg_grid_quality_result* out);

/* ------------------------------------------------------------------------------------------------------
 * Topography by refined sampling (an addition: the reference has no topography step).  Inputs: the STITCHED supergrid x, y
 * ((ny + 1) x (nx + 1), degrees) and a source raster S[js][is] (Ny x Nx, row 0 southmost) whose cell EDGES are lon0 + is * dlon and
 * lat0 + js * dlat (dlat > 0).  The raster is periodic in longitude when |Nx * dlon - 360| <= 1e-9, regional otherwise.
 * Values: int16 sources are used as they are (q = v); float32 / float64 sources are quantised by ogg_topog_quantize_dev,
 * q = rint(v / quantum), |q| <= 2^21 or the call fails.  NaN and the source's fill values are MISSING.  All accumulation is in
 * integers, so a record is exact and independent of any order.
 * Supergrid cell (j, i), corners P00 = (x, y)[j][i], P01 = [j][i+1], P10 = [j+1][i], P11 = [j+1][i+1], all in fp64 in this order:
 *   unwrap    l = x00 + (((x - x00 + 180) mod 360) - 180) for each corner x (mod with numpy's % semantics: the result has the sign
 *             of 360); then a corner with |y| >= 90 - 1e-10 takes the unwrapped longitude (before this substitution) of the other
 *             corner of its own row (P00 <-> P01, P10 <-> P11): L00 .. L11
 *   refine    R = clamp(ceil(oversample * max(spanL / dlon, spanY / dlat)), 1, 256), spans = max - min over the four corners; R
 *             above 256 (or not a number) is CLAMPED; refine > 0 replaces R for every cell (and nothing is clamped)
 *   pole      the cell ENCLOSES a pole when |w(L01 - L00) + w(L11 - L01) + w(L10 - L11) + w(L00 - L10)| > 180, w(d) =
 *             ((d + 180) mod 360) - 180, summed left to right; the north pole when y00 + y01 + y10 + y11 > 0 (summed left to
 *             right), else the south pole
 *   samples   a, b = 0 .. R-1; s = (a + 0.5) / R, t = (b + 0.5) / R, u = 1 - s, v = 1 - t;
 *             lon = (u * v) * L00 + (s * v) * L01 + (u * t) * L10 + (s * t) * L11 (left to right), lat the same of y00 .. y11;
 *             a pole-enclosing cell samples the polar raster row instead: lon = L00 + 360 * s, js = 0 (south) or Ny - 1 (north)
 *   index     js = floor((lat - lat0) * inv_dlat), inv_d = 1.0 / d once in fp64.  Periodic: is = floor((lon - lon0) * inv_dlon)
 *             mod Nx, js clamped to [0, Ny - 1].  Regional: the sample is met on the raster's own longitude branch, whatever
 *             multiple of 360 the grid or lon0 is stated at: d = lon - lon0, d' = d mod 360 (numpy's % semantics, as for unwrap:
 *             m = fmod(d, 360), m + 360 when m < 0, +0 when m = 0; d' is d itself, bit for bit, when 0 <= d < 360),
 *             is = floor(d' * inv_dlon); an index outside the raster (is outside [0, Nx - 1], d' = 360 included, or js outside
 *             [0, Ny - 1]) makes the sample MISSING.  A sample whose lon or lat is not finite (NaN or +-infinity, from a grid point
 *             that is not finite) is MISSING for periodic and regional sources alike: no index is formed from it, and an infinite
 *             latitude is not clamped to a polar row (a periodic source also refuses |floor((lon - lon0) * inv_dlon)| >= 4e15).
 *             Such a cell has no spans: its R is CLAMPED as above.  A pole-enclosing cell's samples have no lat; only lon counts
 *   record    n (samples that are not missing), n_missing, n_wet ((double)q < wet_below, wet_below = sea_level / quantum), sum q and
 *             sum q^2 (int64), min q, max q (INT32_MAX / INT32_MIN when n = 0), R
 * A MODEL cell (a MOM6 h-cell) is the 2 x 2 block of supergrid cells (2 jm + dj, 2 im + di): its record is the exact integer
 * combination of theirs (R the largest; n_pole, n_clamped counted over the four).  nx and ny must then be even.
 * Outputs (host side, from the integers): height = sum / n * quantum; h_std = sqrt((double)(n * sumsq - sum^2)) / n * quantum with
 * the difference formed exactly in 128 bits; h_min, h_max = q * quantum; wet_fraction = n_wet / n; depth = max(0, -height).
 * ---------------------------------------------------------------------------------------------------- */
#define OGG_TOPOG_MAX_REFINE 256
#define OGG_TOPOG_MAX_Q (1 << 21)                 /* |q| bound of a quantised source */
#define OGG_TOPOG_MISSING_Q ((int)0x80000000)     /* the missing value of an int32 (quantised) source */
#define OGG_TOPOG_POLE_EPS 1.0e-10
enum { OGG_TOPOG_INT16 = 0, OGG_TOPOG_INT32 = 1, OGG_TOPOG_FLOAT32 = 2, OGG_TOPOG_FLOAT64 = 3 };
enum { OGG_TOPOG_MODEL_CELLS = 0, OGG_TOPOG_SUPERGRID_CELLS = 1 };
/* the source raster.  dtype OGG_TOPOG_INT16 or OGG_TOPOG_INT32 for sampling (an int32 source holds quantised values, missing ones
 * OGG_TOPOG_MISSING_Q); the host-pointer ogg_topog also takes FLOAT32 / FLOAT64 and quantises them on the device.  n_fill (0..2)
 * values of fill[] mark missing raw values (compared as (double)v == fill[k]) in an int16 or a float source. */
typedef struct ogg_topog_source {
    const void* data;
    int dtype, n_fill;
    double fill[2];
    long Nx, Ny;
    double lon0, dlon, lat0, dlat;
    double quantum;      /* float sources: q = rint(v / quantum) */
    double wet_below;    /* a sample is wet when (double)q < wet_below (= sea_level / quantum) */
} ogg_topog_source;
/* a band: supergrid cell rows j0 .. j0 + n_cell_rows - 1 of the stitched grid (j0 counted in the whole grid: it decides the pairing
 * into model rows).  x, y hold the band's n_cell_rows point rows (stride nx + 1), x_next, y_next the point row that follows them
 * (the next band's first row).  Output rows: m = j >> shift for j in the band (shift = 1 for model cells, 0 for supergrid cells),
 * rows m0 = j0 >> shift .. m1 = (j0 + n_cell_rows - 1) >> shift, nx >> shift records each.  A model row whose two supergrid rows
 * lie in two bands gets a PARTIAL record from each (the cells of this band only); the two combine exactly (sums, min, max). */
typedef struct ogg_topog_band {
    long nx, j0, n_cell_rows;
    const double *x, *y, *x_next, *y_next;
    int cells;           /* OGG_TOPOG_MODEL_CELLS or OGG_TOPOG_SUPERGRID_CELLS */
    int refine;          /* 0: R from the spans; 1 .. 256: this R for every cell */
    double oversample;
} ogg_topog_band;
typedef struct ogg_topog_record {
    long long n, n_missing, n_wet, sum, sumsq;
    int min, max, R;
    short n_pole, n_clamped;   /* supergrid cells of this record that enclose a pole / whose R was clamped */
} ogg_topog_record;
long ogg_topog_band_out_rows(const ogg_topog_band* band);  /* m1 - m0 + 1 (0 for an empty band), -1 on a bad band */
long ogg_topog_workspace_bytes(void);                      /* the work counter of ogg_topog_band_dev */
/* device pointers throughout: the band's records, row-major (m - m0, i_out), into out (device memory, out_rows * (nx >> shift)
 * records).  One wavefront owns each output record and reduces its samples in registers; wavefronts take runs of records from a
 * counter in the workspace (work distribution only: no result is accumulated across wavefronts, so none depends on the order). */
int ogg_topog_band_dev(const ogg_topog_band* band, const ogg_topog_source* src, void* workspace, long workspace_bytes,
                       ogg_topog_record* out, void* stream);
/* a float32 / float64 raster (src->dtype) -> int32 q (device memory, Nx * Ny); *n_bad (device int) is set non-zero when some
 * |q| > OGG_TOPOG_MAX_Q, and the caller must then refuse the result (the host form does) */
int ogg_topog_quantize_dev(const ogg_topog_source* src, int* q, int* n_bad, void* stream);
/* HOST pointers in *band and *src (x, y hold n_cell_rows + 1 point rows when x_next is NULL), staged through device memory; out is
 * host memory.  A float source is quantised on the device first (OGG_EARG when |q| > OGG_TOPOG_MAX_Q). */
int ogg_topog(const ogg_topog_band* band, const ogg_topog_source* src, ogg_topog_record* out);

/* Plane-fit topography (opt-in; without it every record, output and file above is what it was): the least-squares plane
 * q ~ c + a * dI + b * dJ over the valid samples of every output cell, fitted in the raster's INDEX space: dI counts raster columns
 * and dJ raster rows from a per-cell origin.  The sub-grid roughness about that plane is h2, its slope the resolved bottom slope
 * (h_std is the spread about the MEAN: on a slope it is mostly resolved slope).  Samples, indices, missing values, R, the pole test and
 * the quantisation are exactly as above; the accumulation is in integers, so a plane record too is exact and bit-identical for any
 * split into bands or ranks.  The fit is a plane in (lon, lat); within a cell that is a plane in distance to first order in the
 * cell's size over its distance to the pole.  Cells that enclose a pole are refused.
 *   origin    O of an output cell: for a model cell (jm, im) the supergrid point (2 jm + 1, 2 im + 1), its centre; for a supergrid
 *             cell its P00.  A band that holds only one of a model row's two supergrid rows still holds this point (in its own rows or
 *             in x_next / y_next), so two partial records use the same origin and add up.
 *             Periodic raster: fI0 = floor((xO - lon0) * inv_dlon), fJ0 = floor((yO - lat0) * inv_dlat) clamped to [0, Ny - 1].
 *             Regional raster: fI0 = floor(((xO - lon0) mod 360) * inv_dlon) (numpy's % semantics and the branch rule of the
 *             samples), fJ0 = floor((yO - lat0) * inv_dlat), unclamped; neither index is range-tested.
 *             NO ORIGIN: xO or yO is not finite, or a periodic source has |fI0| >= 4e15 (or an index is not a number); every valid
 *             sample of the record is then FAR
 *   offsets   of a sample that is not missing, with its unreduced column index fi (before mod Nx on a periodic source, after the
 *             branch mapping on a regional one) and its row index fj (after the clamp on a periodic source):
 *             periodic dI = ((fi - fI0 + hN) mod Nx) - hN, hN = Nx div 2, a non-negative mod; regional dI = fi - fI0, with NO wrap: a
 *             cell whose origin and samples lie on either side of the raster's branch cut at lon0 has offsets of nearly a turn, and
 *             ends up FAR wherever a turn is more than OGG_TOPOG_PLANE_MAX_OFFSET columns (on a coarser raster the offsets are
 *             within the limit, all shifted alike, which the fit does not see); dJ = fj - fJ0.  All are integral doubles, exact.
 *             (The kernel forms the same values as int32 differences of the reduced indices and tests those: with Nx, Ny < 2^30 and
 *             a regional origin admitted only within 2^16 of the raster nothing overflows; csrc/ogg_topog.hip, at the far test.)
 *   far       a valid sample is FAR (counted in n_far) when |dI| > OGG_TOPOG_PLANE_MAX_OFFSET or |dJ| > OGG_TOPOG_PLANE_MAX_OFFSET,
 *             when it belongs to a pole-enclosing supergrid cell (which has no latitude), or when the cell has no origin.  Far samples
 *             enter n, sum, sumsq, min and max as above, but not the moments
 *   moments   int64, over the valid samples that are not far: sx = sum dI, sy = sum dJ, sxx = sum dI^2, sxy = sum dI dJ,
 *             syy = sum dJ^2, sxq = sum dI q, syq = sum dJ q.  n <= 4 * 256^2 = 2^18, |d| <= 2^15, |q| <= 2^21, so sxx <= 2^48 and
 *             |sxq| <= 2^54: nothing overflows.  Partial records combine by adding the eight new fields
 * Outputs (host side, from the integers): the centred moments Cxx = n sxx - sx^2, Cxy = n sxy - sx sy, Cyy = n syy - sy^2,
 * Cxq = n sxq - sx sum, Cyq = n syq - sy sum, Cqq = n sumsq - sum^2, each formed exactly in 128 bits and rounded once to fp64; then
 * in fp64, in this order: d = Cxx * Cyy - Cxy * Cxy, a = (Cxq * Cyy - Cyq * Cxy) / d, b = (Cyq * Cxx - Cxq * Cxy) / d,
 * r = Cqq - a * Cxq - b * Cyq (left to right).
 *   plane_flag (byte)  0: n = 0, every float output is the fill value; 1: fitted; 2: degenerate, n < 3 or d <= 0 (one raster column
 *             or row, collinear samples); 3: refused, n_far > 0
 *   h2        flag 1: max(0, r) / (n * n) * quantum^2; flags 2 and 3: Cqq / (n * n) * quantum^2, the variance about the mean
 *   plane_a, plane_b   flag 1: a, b in quanta per raster column / row; otherwise the fill value
 *   slope_east = a * quantum / (dlon * pi / 180 * Re * cos(latC * pi / 180)), slope_north = b * quantum / (dlat * pi / 180 * Re),
 *             Re the library's Earth radius (ogg_math.h); latC is yO for model cells and the mean of the four corner latitudes
 *             ((y00 + y01 + y10 + y11) / 4, summed left to right) for supergrid cells; slope_east is the fill value where
 *             |latC| >= 90 - OGG_TOPOG_POLE_EPS */
#define OGG_TOPOG_PLANE_MAX_OFFSET (1 << 15)
typedef struct ogg_topog_plane_record {
    ogg_topog_record base;
    long long sx, sy, sxx, sxy, syy, sxq, syq, n_far;
} ogg_topog_plane_record;
/* ogg_topog_band_dev with the plane moments: the same band, source and workspace contracts; out holds plane records */
int ogg_topog_plane_band_dev(const ogg_topog_band* band, const ogg_topog_source* src, void* workspace, long workspace_bytes,
                             ogg_topog_plane_record* out, void* stream);
/* ogg_topog with the plane moments (HOST pointers, the same staging); out holds plane records */
int ogg_topog_plane(const ogg_topog_band* band, const ogg_topog_source* src, ogg_topog_plane_record* out);

/* Layered topography (opt-in; without it every record, output and file above is what it was): the topography sampled from an ORDERED
 * list of 1 .. OGG_TOPOG_MAX_SOURCES layers, the first layer that has a value for a sample giving it.  A layer is a source raster
 * with a kind, a projection and an integer multiplier q_mul >= 1.  The usual use: a polar-stereographic raster in metres (BedMachine,
 * IBCSO) over a global lat-lon one.
 * The sample positions (unwrap, refine's a, b, the pole test, s, t, the bilinear lon and lat) are exactly those of "Topography by
 * refined sampling"; they depend on no layer.
 *   kinds     OGG_TOPOG_LATLON: the source as above.  OGG_TOPOG_POLAR_STEREO: the four box numbers of the source mean X0, dX, Y0, dY
 *             (src.lon0, dlon, lat0, dlat in that order): metres, cell EDGES X0 + I * dX and Y0 + J * dY, dX, dY > 0, row 0 the lowest Y
 *   project   polar stereographic on an ellipsoid (Snyder, Map Projections: A Working Manual, eqs. 21-33 / 21-34 with the t of 15-9),
 *             written so that numpy and the device evaluate one expression.  h = +1 (north) or -1 (south), lon0 the central meridian,
 *             a the semi-major axis, e the eccentricity (0: a sphere; 0 <= e < 0.2), K a constant the caller computes, all fp64:
 *               phi = h * lat * (pi / 180), lam = h * (lon - lon0) * (pi / 180) (left to right), s = sin phi, c = cos phi,
 *               rho = ((K * c) / (1 + s)) * exp(e * atanh(e * s)),   X = h * (rho * sin lam),   Y = -h * (rho * cos lam)
 *             K = a * m_ts / t_ts with m_ts = cos phi_ts / sqrt(1 - e^2 sin^2 phi_ts) and t_ts = c / (1 + s) * exp(e * atanh(e * s)) at
 *             phi_ts = h * lat_ts; for phi_ts = 90 degrees K = 2 a / sqrt((1 + e)^(1 + e) * (1 - e)^(1 - e)).  (c / (1 + s) is Snyder's
 *             tan(pi / 4 - phi / 2).)  The kernel takes exp and atanh from short series (csrc/ogg_math.h), sin and cos from the device
 *             library; a is not read on the device.  A sample with h * lat >= 90 - OGG_TOPOG_POLE_EPS has X = Y = +0 exactly
 *   gate      a sample is projected in a layer only when its lon and lat are finite and h * lat >= lat_gate (an input, >= -80: the
 *             projection grows without bound towards the other pole); otherwise it is MISSING in that layer, for one compare
 *   index     projected: I = floor((X - X0) * inv_dX), J = floor((Y - Y0) * inv_dY), inv_d = 1.0 / d once in fp64; outside
 *             [0, Nx) x [0, Ny) the sample is MISSING in that layer.  Lat-lon layers index as above (periodic and regional rules)
 *   pole      the samples of a pole-enclosing cell sit at that pole: a lat-lon layer reads its polar row as above; a projected layer
 *             takes lat = +-90 for them (lon as above, which only the finite test reads), so one of that hemisphere reads the element
 *             at (+0, +0) and one of the other hemisphere is refused by its gate
 *   merge     a sample takes q = q_mul_k * q_k from the first layer k, in list order, in which it is not MISSING (outside, gated,
 *             a fill value, NaN); n_from[k] counts the samples taken from layer k; a sample MISSING in every layer counts in n_missing.
 *             |q_mul_k * q_k| <= OGG_TOPOG_MAX_Q is demanded of every value stored in layer k, not only of the sampled ones:
 *             ogg_topog_layer_range_dev tells, ogg_topog_layers refuses; nothing is clamped.  n_wet counts (double)q < wet_below of
 *             layers[0].src (stated in the list's quantum); the other layers' wet_below is not read
 *   refine    refine > 0 replaces R as above.  Otherwise every layer k gives a value v_k and R = clamp(max_k v_k, 1, 256), CLAMPED
 *             when the maximum exceeds 256 or some v_k is not a number.  Lat-lon: v_k is the expression above, unconditionally (so a
 *             list of one lat-lon layer gives the records above bit for bit).  Projected: the four corners (L, y), after the unwrap
 *             and the polar substitution, are projected like samples; a corner COUNTS when it is finite and passes the gate; when at
 *             least one counting corner also indexes inside the raster, v_k = ceil(oversample * max(spanX / dX, spanY / dY)) with the
 *             spans (max - min) over the counting corners; otherwise v_k = 1
 *   record    ogg_topog_merge_record: base holds what ogg_topog_record holds, over the merged samples, then n_from[4].  A model
 *             cell's record is the exact integer combination of its four supergrid cells', and partial records of a model row split
 *             over two bands combine exactly (n_from adds).  All accumulation is in integers: the same bits for any split into
 *             bands and any number of ranks.
 * The plane fit lives in ONE raster's index space and has no meaning across layers or in a projected raster's: there is no plane
 * form of these entry points, and the Python layer refuses --topog_roughness with a list or a projected source. */
#define OGG_TOPOG_MAX_SOURCES 4
enum { OGG_TOPOG_LATLON = 0, OGG_TOPOG_POLAR_STEREO = 1 };
typedef struct ogg_topog_projection {
    int h;               /* +1 north, -1 south */
    int reserved;
    double lon0, a, e, K, lat_gate;
} ogg_topog_projection;
typedef struct ogg_topog_layer {
    ogg_topog_source src;
    int kind;            /* OGG_TOPOG_LATLON or OGG_TOPOG_POLAR_STEREO */
    int q_mul;           /* q = q_mul * (the source's q) */
    ogg_topog_projection proj;   /* read for OGG_TOPOG_POLAR_STEREO only */
} ogg_topog_layer;
typedef struct ogg_topog_merge_record {
    ogg_topog_record base;
    long long n_from[OGG_TOPOG_MAX_SOURCES];
} ogg_topog_merge_record;
/* ogg_topog_band_dev over layers: device pointers throughout, the same band and workspace contracts; out holds merge records.
 * Every argument is validated before any device work (OGG_EARG with a message): n_layers outside 1 .. 4, a bad kind, h not +-1,
 * e outside [0, 0.2), K not positive, dX or dY <= 0, lat_gate < -80, q_mul < 1.  The range of q_mul * q is NOT among them: it is
 * the caller's to check once per layer with ogg_topog_layer_range_dev (the host form and the Python layer do); a layer that was
 * not checked can wrap silently in the records (never in memory) */
int ogg_topog_layers_band_dev(const ogg_topog_band* band, int n_layers, const ogg_topog_layer* layers, void* workspace,
                              long workspace_bytes, ogg_topog_merge_record* out, void* stream);
/* *n_bad (device int) is set non-zero when some stored value of the layer's raster (device memory, INT16 or INT32) has
 * |q_mul * q| > OGG_TOPOG_MAX_Q; the caller must then refuse the layer (the host form does) */
int ogg_topog_layer_range_dev(const ogg_topog_layer* layer, int* n_bad, void* stream);
/* HOST pointers in *band and the layers, staged and quantised like ogg_topog; out is host memory */
int ogg_topog_layers(const ogg_topog_band* band, int n_layers, const ogg_topog_layer* layers, ogg_topog_merge_record* out);
/* the sampling kernel's own projection applied to n points (device pointers): X, Y as above and gate_ok[k] (int) = 1 when the point
 * is finite and passes the gate (0: X = Y = 0 are stored).  Test-only: it holds the device projection to a truth on its own */
int ogg_topog_project_dev(const ogg_topog_projection* proj, long n, const double* lon, const double* lat, double* X, double* Y,
                          int* gate_ok, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Face topography (opt-in; without it every record, output and file above is what it was): what lies BETWEEN two neighbouring model
 * cells, for MOM6's sub-grid topography at velocity points (its "porous barriers" read a lowest, a highest and an average depth on
 * every u and v face).  One lat-lon source (no list, no projected source), integer records only, no connectivity search ("Sill depths"
 * below searches: it takes these sills as face weights and gives the depth at which every cell is connected to a seed).  Where this
 * text and "Topography by refined sampling" above could disagree about a sample, that section wins: a face's samples are its samples.
 *   grid      the STITCHED supergrid x, y ((ny + 1) x (nx + 1), row stride ld >= nx + 1), ny and nx even; model cells nym = ny / 2 by
 *             nxm = nx / 2; topology = OGG_MASK_PERIODIC | OGG_MASK_FOLD, the ocean mask's flags
 *   u faces   (jm, I), jm = 0 .. nym - 1, I = 0 .. nxm, on supergrid point column 2 I.  The face's BLOCK is supergrid rows 2 jm + dj
 *             (dj = 0, 1) of column 2 I - 1 (west side) and column 2 I (east side).  At I = 0 the west side is absent, with PERIODIC it
 *             is column nx - 1; at I = nxm the east side is absent, with PERIODIC it is column 0: the faces I = 0 and I = nxm then
 *             hold the same record, byte for byte
 *   v faces   (J, im), J = 0 .. nym, im = 0 .. nxm - 1, on supergrid point row 2 J.  The block is supergrid columns 2 im + di
 *             (di = 0, 1) of row 2 J - 1 (south side) and row 2 J (north side).  At J = 0 the south side is absent.  At J = nym the
 *             north side is absent; with FOLD it is row ny - 1 of columns nx - 1 - (2 im + di), read with its lines reversed (below)
 *   refine    every present supergrid cell of the block gets its R by the topography's rule (spans, oversample, clamp at 256); the
 *             block's R is the largest of them, n_clamped counts the clamped cells; refine > 0 replaces R for every cell (nothing is
 *             clamped).  Every present cell of the block is then sampled at R x R: positions (unwrap, pole-corner substitution, s, t,
 *             the bilinear lon and lat), index and value are exactly the topography's for a cell of that R
 *   lines     a line runs across the face, from one side's cell centre line to the other's, along the grid's own coordinate.  u face,
 *             line (dj, b): the samples (a, b), a = 0 .. R - 1, of cell (2 jm + dj, west) and of cell (2 jm + dj, east).  v face, line
 *             (di, a): the samples (a, b), b = 0 .. R - 1, of cell (south, 2 im + di) and of cell (north, 2 im + di); on the fold the
 *             north side gives the samples (R - 1 - a, b) of cell (ny - 1, nx - 1 - (2 im + di)).  A two-sided face has 2 R lines of up
 *             to 2 R samples, a one-sided face 2 R lines of up to R samples.  The RIDGE of a line is the largest q among its samples
 *             that are not MISSING; a line none of whose samples has a value is a missing line
 *   pole      if a present cell of the block ENCLOSES a pole (the topography's pole test) the face has no lines: its record has the
 *             POLE flag, n = n_missing = n_lines = n_lines_missing = n_dry_lines = 0, ridge_sum = 0 and extremes as for "none" (R,
 *             n_clamped and the other flags as for any face).  Cells with pole corners are sampled like any other
 *   record    n, n_missing: samples of the block with and without a value; n_lines, n_lines_missing: lines with a ridge and missing
 *             lines; n_dry_lines: lines with a ridge that is not wet, !(ridge < wet_q), wet_q the topography's integer threshold of
 *             (double)q < wet_below; lo: the smallest ridge, the deepest way through the face (the SILL), INT32_MAX when none; hi: the
 *             largest ridge, INT32_MIN when none; ridge_sum (int64): the sum of the ridges; q_min: the smallest valid sample of the
 *             block, INT32_MAX when none; R, n_clamped; flags: OGG_FACE_ONE_SIDED (a side is absent), OGG_FACE_POLE, OGG_FACE_SEAM
 *             (the periodic partner was used), OGG_FACE_FOLD (the fold partner was used)
 * Everything is an integer, so a record is exact: no launch shape, work order or split of the output rows changes a bit of it.
 * Outputs (host side, quantum as in the topography): depth_max = -lo * quantum (the sill, the deepest passage), depth_min = -hi *
 * quantum (the shallowest), depth_ave = -(ridge_sum / n_lines) * quantum, open_fraction = 1 - n_dry_lines / n_lines.  Depths are not
 * clamped at zero: a face over land has negative depths, and n_dry_lines is the wet test.
 * Why lines: they are the paths a flow takes across the face if it follows the grid, and a line's highest point is what that path
 * must clear: a ridge anywhere between the two cell centres counts, not only one on the face line itself, and a gap in the ridge
 * one line wide still shows as lo.  It needs no search and no ordering.  It is NOT Adcroft's thin-wall coarsening, and it finds no
 * passage that runs diagonally through the block.
 * ---------------------------------------------------------------------------------------------------- */
#define OGG_FACE_ONE_SIDED 1
#define OGG_FACE_POLE 2
#define OGG_FACE_SEAM 4
#define OGG_FACE_FOLD 8
/* A face record is OGG_TOPOG_FACE_WORDS int64 words (56 bytes, little-endian), no struct of this header, so that the set of structs
 * and their OGG_ABI_* codes stays what it was.  Byte offsets: 0 n, 8 n_missing, 16 ridge_sum (int64 each); 24 n_lines, 28
 * n_lines_missing, 32 n_dry_lines, 36 lo, 40 hi, 44 q_min, 48 R (int32 each); 52 n_clamped, 54 flags (int16 each). */
#define OGG_TOPOG_FACE_WORDS 7
/* The grid of a call is the whole stitched grid as ONE band of model cells: grid->nx, grid->n_cell_rows = ny, grid->j0 = 0,
 * grid->cells = OGG_TOPOG_MODEL_CELLS, grid->x, grid->y of (ny + 1) rows of ld doubles (ld >= nx + 1), grid->refine and
 * grid->oversample as for a band; x_next and y_next are not read.  The output rows: u-face rows [ju0, ju1) of 0 .. nym and v-face rows
 * [jv0, jv1) of 0 .. nym + 1 (any slice; an empty range skips that family).
 * ogg_topog_faces_check: OGG_EARG with a reason for odd or empty sizes, ld < nx + 1, bad ranges, a bad topology, refine outside
 * 0 .. 256, a bad oversample and a bad source (device != 0: the source must be int16 or int32, as ogg_topog_faces_dev needs it).  No
 * device work, no pointer of *grid or *src is followed. */
int ogg_topog_faces_check(const ogg_topog_band* grid, long ld, int topology, long ju0, long ju1, long jv0, long jv1,
                          const ogg_topog_source* src, int device);
/* device pointers throughout: out_u holds (ju1 - ju0) x (nxm + 1) records, row-major (jm - ju0, I), out_v (jv1 - jv0) x nxm records,
 * (J - jv0, im); only the ranges' rows.  One wavefront owns each face record; wavefronts take runs of faces from the counters at the
 * head of the workspace (ogg_topog_workspace_bytes; work distribution only), the line ridges are combined in LDS by integer maxima. */
int ogg_topog_faces_dev(const ogg_topog_band* grid, long ld, int topology, long ju0, long ju1, long jv0, long jv1,
                        const ogg_topog_source* src, void* workspace, long workspace_bytes, long long* out_u, long long* out_v,
                        void* stream);
/* HOST pointers in *grid and *src, staged like ogg_topog; out_u, out_v are host memory.  A float source is quantised on the device
 * first (OGG_EARG when |q| > OGG_TOPOG_MAX_Q). */
int ogg_topog_faces(const ogg_topog_band* grid, long ld, int topology, long ju0, long ju1, long jv0, long jv1,
                    const ogg_topog_source* src, long long* out_u, long long* out_v);

/* ------------------------------------------------------------------------------------------------------
 * Atmosphere x ocean exchange grid (an addition: the reference has none).  First-order conservative overlaps of a rectilinear global
 * atmosphere with the MOM6 h-cells of the STITCHED supergrid x, y ((ny + 1) x (nx + 1), degrees; nx and ny even), as FMS's
 * make_coupler_mosaic lists them.  All arithmetic is fp64 without fused multiply-add.
 * Atmosphere: lon edges a_0 < .. < a_NA with |a_NA - a_0 - 360| <= 1e-9 (global, periodic), lat edges b_0 < .. < b_NB inside
 * [-90, 90]; cell (J, I) = [a_I, a_I+1] x [b_J, b_J+1].  ogg_xgrid and ogg_xgrid_check_atm refuse any other edges with OGG_EARG
 * before any device work (the _dev steps take the edges in device memory and do not read them on the host).
 * Ocean cell (m, n): corners C0 = (x, y)[2m][2n], C1 = [2m][2n+2], C2 = [2m+2][2n+2], C3 = [2m+2][2n] (counter-clockwise).
 *   unwrap    L_k = x_C0 + (((x_k - x_C0 + 180) mod 360) - 180), mod with numpy's % semantics (as for topography)
 *   pole      a corner with |y| >= 90 - OGG_TOPOG_POLE_EPS is a pole corner; 3 or 4 of them: the cell is DEGENERATE.  The polygon
 *             walks k = 0 .. 3: a non-pole corner gives (L_k, y_k); a pole corner whose cyclic predecessor is not a pole corner
 *             starts a run and gives (L_b, p), (L_a, p), L_b / L_a the longitudes of the non-pole corners just before / after
 *             the run, p = +90 when the corner's y > 0, else -90; a pole corner inside a run gives nothing
 *   encloses  w = sum over the polygon's edges of wrap(lambda_k+1 - lambda_k), wrap(d) = ((d + 180) mod 360) - 180, left to right;
 *             |w| > 180: the cell encloses a pole
 *   area      lam^ = lam * D, phi^ = phi * D, D = pi / 180 (one fp64 constant); phi_r = phi^_0;
 *             A = -(Re * Re) * S, S = sum_k (lam^_k+1 - lam^_k) * G(phi^_k, phi^_k+1) left to right (vertex V is vertex 0),
 *             G = 2 cos((pm + phi_r) / 2) sin((pm - phi_r) / 2) - sin(pm) E(h), pm = (p1 + p2) / 2, h = (p2 - p1) / 2,
 *             E(h) = h2 (1/6 - h2 (1/120 - h2 (1/5040 - h2 / 362880))), h2 = h * h, for |h| < 0.1, else 1 - sin(h) / h
 *             (the exact mean of sin(phi) - sin(phi_r) along an edge straight in (lambda, phi)); a cell with A_poly <= 0 is
 *             INVERTED.  Degenerate, pole-enclosing and inverted cells emit nothing; A_poly is NaN for the first two.
 *   rows      every J with b_J < phi_max and b_J+1 > phi_min (the polygon's latitude range)
 *   columns   every I and shift s in 360 Z with a_I + s < lam_max and a_I+1 + s > lam_min (fp64 sums), in order of a_I + s
 *   clip      Sutherland-Hodgman against lam >= a_I + s, lam <= a_I+1 + s, phi >= b_J, phi <= b_J+1, in this order, inclusive
 *             inside tests; a pass over v_0 .. v_n-1 emits v_0 when it is inside, then for k = 0 .. n-1 the crossing of the edge
 *             (v_k, v_k+1 mod n) when its ends are on two sides and, for k < n - 1, v_k+1 when it is inside.  A crossing of lam = c
 *             orders the edge's ends (e, f) by (lam, phi) and
 *             is (c, phi_e + (c - lam_e) * ((phi_f - phi_e) / (lam_f - lam_e))); of phi = c the same with the roles swapped
 *   keep      A_x (the area of the clipped polygon) > 0 and A_x > threshold * min(A_poly, A_atm), A_atm = (Re * Re) *
 *             (a_I+1 * D - a_I * D) * ds_J, ds_J = sin b^_J+1 - sin b^_J formed as 2 cos((b^_J + b^_J+1) / 2) sin((b^_J+1 - b^_J) / 2);
 *             an optional uint8 mask (0: the cell emits nothing)
 * Order: ocean cells row-major (m, n), then J ascending, then a_I + s ascending.  Nothing is summed across cells, so the list is
 * bit-identical for any band split.  The integer counts are over the band's cells; the first four ignore the mask.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct ogg_xgrid_atm {
    const double *lon, *lat;   /* NA + 1 and NB + 1 edges */
    long NA, NB;
} ogg_xgrid_atm;
/* a band: stitched supergrid cell rows j0 .. j0 + n_cell_rows - 1 of a grid of ny cell rows.  Its model rows are the m with
 * j0 <= 2 m < j0 + n_cell_rows (a model row belongs to the band that holds its cell row 2 m): m0 = (j0 + 1) / 2 ..
 * m1 = (j0 + n_cell_rows + 1) / 2 (exclusive).  x, y hold the band's n_cell_rows point rows (stride nx + 1); x_next, y_next the
 * ogg_xgrid_band_next_rows() point rows that follow them in stitched order (rows j0 + n_cell_rows .., contiguous, stride nx + 1).
 * mask: NULL, or one byte per model cell of rows m0 .. m1 - 1 (row-major, nx / 2 per row). */
typedef struct ogg_xgrid_band {
    long nx, ny, j0, n_cell_rows;
    const double *x, *y, *x_next, *y_next;
    const unsigned char* mask;
    double Re, threshold;
} ogg_xgrid_band;
/* per call; every count over the band's model cells */
typedef struct ogg_xgrid_counts {
    long long cells, pole_cells, pole_enclosing, inverted, degenerate, masked, candidates, kept;
} ogg_xgrid_counts;
long ogg_xgrid_band_first_row(const ogg_xgrid_band* band); /* m0, -1 on a bad band */
long ogg_xgrid_band_out_rows(const ogg_xgrid_band* band);  /* m1 - m0 (0 for a band without a model row), -1 on a bad band */
long ogg_xgrid_band_next_rows(const ogg_xgrid_band* band); /* point rows needed after the band: 0, 1 or 2; -1 on a bad band */
long ogg_xgrid_workspace_bytes(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm); /* of the count and write steps, -1 if bad */
/* the checks of the edges (HOST pointers in *atm): OGG_EARG unless they are as above */
int ogg_xgrid_check_atm(const ogg_xgrid_atm* atm);
/* count step, device pointers, on a stream: A_poly of the band's cells into a_poly ((m1 - m0) x nx / 2 doubles), the counts into
 * *counts (device memory), and into the workspace what the write step needs.  counts->kept is the length of the band's list. */
int ogg_xgrid_count_dev(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm, void* workspace, long workspace_bytes, double* a_poly,
                        ogg_xgrid_counts* counts, void* stream);
/* write step, after the count step on the same band, atmosphere and workspace: the list (counts->kept entries, device memory):
 * atm_ij[k] = (I, J), ocn_ij[k] = (n, m) (0-based, m counted in the whole grid), area[k] = A_x.  The step redoes the clipping and
 * uses the workspace's per-wavefront offsets. */
int ogg_xgrid_write_dev(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm, const void* workspace, long workspace_bytes, int* atm_ij,
                        int* ocn_ij, double* area, void* stream);
/* HOST pointers throughout (x, y hold n_cell_rows + next_rows point rows when x_next is NULL), staged through device memory: both
 * steps, then the list is copied into atm_ij / ocn_ij / area when counts->kept <= capacity (OGG_ESHAPE otherwise, with *counts and
 * a_poly filled: call again with that capacity). */
int ogg_xgrid(const ogg_xgrid_band* band, const ogg_xgrid_atm* atm, long capacity, int* atm_ij, int* ocn_ij, double* area,
              double* a_poly, ogg_xgrid_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Exchange grid with a cubed-sphere atmosphere (an addition: the reference has none).  First-order conservative overlaps of a gnomonic
 * cubed-sphere atmosphere (six faces of N x N cells) with the MOM6 h-cells of the STITCHED supergrid (an ogg_xgrid_band, as above).
 * All arithmetic is fp64 without fused multiply-add.
 * Atmosphere: a table t_0 < .. < t_N with t_0 = -1 and t_N = 1 exactly, 1 <= N <= 4096, the same on both axes and on all six faces,
 * and six frames F_f = (e_u, e_v, e_n)_f, f = 0 .. 5, rows of a 3 x 3 matrix.  Cell (f, J, I) is the set of unit vectors P with
 * P.e_n > 0, xi = P.e_u / P.e_n in [t_I, t_I+1] and eta = P.e_v / P.e_n in [t_J, t_J+1].  ogg_xgrid_cs_check_atm (HOST pointers, no
 * device work) returns OGG_EARG unless the table is strictly increasing with those ends, every frame is orthonormal and right-handed
 * (e_u x e_v = e_n) within 1e-12, the six normals are pairwise orthogonal or opposite within 1e-12, and every e_u, e_v is +- some
 * face's normal within 1e-12: together these make the frames a cube in any rotation.
 * Ocean cell (m, n): corners C0 .. C3 as above.
 *   vectors   P_k = (cos phi cos lam, cos phi sin lam, sin phi), lam = mod360(x_k) * D, phi = y_k * D, D = pi / 180 (one fp64
 *             constant), mod360 with numpy's % semantics: exact, so a grid stated whole turns away gives the same bits.  There is no
 *             pole substitution: a pole corner is a point like any other, and two pole corners make a triangle.
 *   edges     great circles (FMS's rule whenever one side of the exchange is a cubed sphere), NOT straight in (lambda, phi) as in
 *             the lat-lon section above
 *   skipped   a cell with a non-finite corner is DEGENERATE; a cell with two corners more than 30 degrees apart (P_i . P_j <
 *             OGG_XGRID_CS_COS_WIDE) is WIDE (no model cell is that large; the rule lets the faces below work without homogeneous
 *             clipping).  A_poly is NaN for both and they emit nothing.
 *   area      A_poly = (Re * Re) * (O3(P0, P1, P2) + O3(P0, P2, P3)), O3(a, b, c) = 2 atan2(a . ((b - a) x (c - a)),
 *             1 + a.b + b.c + c.a): the triple product over the differences, dot products summed x, y, z left to right.
 *             A_poly <= 0: the cell is INVERTED and emits nothing.
 *   faces     face f is a candidate of a cell when all four corners have w_k = P_k . e_n > 0.05 (necessary for overlap: a point of
 *             a face is within 54.74 degrees of its centre and a cell is at most 30 across, so an overlapping cell has every
 *             w >= cos 84.74 = 0.092).  The test can admit a face the polygon misses; such pairs clip to nothing.  A face and its
 *             opposite cannot both pass it, so a cell has at most three candidate faces.  On a candidate
 *             face the polygon is (xi_k, eta_k) = ((P_k . e_u) / w_k, (P_k . e_v) / w_k), k = 0 .. 3: great-circle edges and the
 *             atmosphere's grid lines are both straight in this plane.
 *   rows      every J with t_J < eta_max and t_J+1 > eta_min; columns: every I with t_I < xi_max and t_I+1 > xi_min (no shifts)
 *   clip      the Sutherland-Hodgman of the lat-lon section word for word, xi in the place of lambda and eta in the place of phi:
 *             xi >= t_I, xi <= t_I+1, eta >= t_J, eta <= t_J+1 in this order, inclusive inside tests, the same emission rule and
 *             the same canonical-order crossing with the clipped coordinate set to the line's value exactly
 *   A_x       a pair whose atmosphere cell contains all four (xi_k, eta_k), inclusive, takes A_x = A_poly (the two area formulas
 *             round differently).  Otherwise a fan from vertex 0 of the clipped polygon v_0 .. v_n-1 (0 when n < 3):
 *             A_x = (Re * Re) * sum_k=1..n-2 O2(v_0, v_k, v_k+1), left to right, with r = sqrt(1 + xi * xi + eta * eta),
 *             num = ((xi_b - xi_a) * (eta_c - eta_a) - (eta_b - eta_a) * (xi_c - xi_a)) / (r_a * r_b * r_c),
 *             d(p, q) = (xi_p * xi_q + eta_p * eta_q + 1) / (r_p * r_q), O2 = 2 atan2(num, 1 + d(a, b) + d(b, c) + d(c, a)):
 *             the 2-D cross product of exact differences is the well-conditioned form of the triple product
 *   keep      A_x > 0 and A_x > threshold * min(A_poly, A_atm(J, I)), A_atm(J, I) = (Re * Re) * (O2(c00, c10, c11) + O2(c00, c11,
 *             c01)) over the cell's table corners c00 = (t_I, t_J), c10 = (t_I+1, t_J), c11, c01 = (t_I, t_J+1), the same on every
 *             face; an optional uint8 mask (0: the cell emits nothing)
 * Order: ocean cells row-major (m, n), then f ascending, then J, then I.  Nothing is summed across cells, so the list is bit-identical
 * for any band split.  Counts over the band's cells: cells, degenerate, wide and inverted ignore the mask; face_candidates counts the
 * (cell, face) pairs that pass the w test and candidates sums rows x columns over them, both over unmasked cells with A_poly > 0.
 * ---------------------------------------------------------------------------------------------------- */
#define OGG_XGRID_CS_COS_WIDE 0.86602540378443864676 /* cos 30 degrees */
typedef struct ogg_xgrid_cs_atm {
    const double* t;      /* N + 1 table entries */
    long N;
    double frames[6][9];  /* e_u, e_v, e_n of faces 0 .. 5 (always host memory: part of the struct) */
} ogg_xgrid_cs_atm;
typedef struct ogg_xgrid_cs_counts {
    long long cells, degenerate, wide, inverted, masked, face_candidates, candidates, kept;
} ogg_xgrid_cs_counts;
/* of the count and write steps (it holds the N x N table of A_atm), -1 if bad */
long ogg_xgrid_cs_workspace_bytes(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm);
/* the checks of the table and the frames (HOST pointer in *atm): OGG_EARG unless they are as above */
int ogg_xgrid_cs_check_atm(const ogg_xgrid_cs_atm* atm);
/* count step, device pointers (band rows, mask, atm->t), on a stream: A_poly of the band's cells into a_poly, the counts into *counts
 * (device memory), and into the workspace what the write step needs.  The frames are checked on the host; the table is not read there. */
int ogg_xgrid_cs_count_dev(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm, void* workspace, long workspace_bytes,
                           double* a_poly, ogg_xgrid_cs_counts* counts, void* stream);
/* write step, after the count step on the same band, atmosphere and workspace: the list (counts->kept entries, device memory):
 * atm_fij[k] = (I, J, f), ocn_ij[k] = (n, m) (0-based, m counted in the whole grid), area[k] = A_x.  The step redoes the clipping. */
int ogg_xgrid_cs_write_dev(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm, const void* workspace, long workspace_bytes,
                           int* atm_fij, int* ocn_ij, double* area, void* stream);
/* HOST pointers throughout, staged through device memory, with the capacity protocol of ogg_xgrid (OGG_ESHAPE with *counts and a_poly
 * filled when counts->kept > capacity: call again with that capacity). */
int ogg_xgrid_cs(const ogg_xgrid_band* band, const ogg_xgrid_cs_atm* atm, long capacity, int* atm_fij, int* ocn_ij, double* area,
                 double* a_poly, ogg_xgrid_cs_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Exchange grid with a curvilinear source grid (an addition: the reference has none).  First-order conservative overlaps of the cells
 * of any logically rectangular mesh on the sphere (another model's tripolar grid, a sea-ice or land mosaic, a regional parent, a
 * rotated-pole reanalysis) with the MOM6 h-cells of the STITCHED supergrid (an ogg_xgrid_band, as above): the list that
 * ogg_remap_dev consumes, with (I, J) of the source cell in the place of the atmosphere's.  All arithmetic is fp64 without fused
 * multiply-add, every product rounded before it is added.
 * Target cell (m, n): corners C0 .. C3 as above.
 * Source: sx, sy in degrees, (NB + 1) x (NA + 1) cell corners of row stride ld >= NA + 1, NA * NB < 2^31 and NA * NB *
 * OGG_LOCATE_MAX_TOUCH < 2^31.  Source cell (J, I) has the corners (J, I), (J, I+1), (J+1, I+1), (J+1, I), and its list index is
 * q = J * NA + I.  An optional byte per source cell masks it: a masked source cell (0) emits nothing.
 *   vectors   of both grids by the cubed-sphere section's rule: mod360, then the unit vector (a mesh stated whole turns away gives
 *             the same bits); no pole substitution.  Edges are great circles.
 *   target    DEGENERATE, WIDE (OGG_XGRID_CS_COS_WIDE) and INVERTED word for word as in the cubed-sphere section; A_poly is that
 *             section's O3 fan, (Re * Re) * (O3(P0, P1, P2) + O3(P0, P2, P3)).  Only cells with A_poly > 0 are valid.
 *   source    DEGENERATE and WIDE as for the target; A_src the same O3 fan over the cell's corners Q0 .. Q3.  A_src < 0: the cell is
 *             REVERSED, its corners are taken in the order 0, 3, 2, 1 and A_src is formed again in that order (a mesh stored north
 *             to south works).  A_src not > 0 after that (0, or not finite): the cell is FLAT and emits nothing.  A_src is NaN for
 *             DEGENERATE and WIDE cells.  The other cells are valid.
 *   normals   n_e = n(a, b) of "Point location" for the edges S = (Q0, Q1), E = (Q1, Q2), N = (Q2, Q3), W = (Q3, Q0) of the oriented
 *             source cell, and the measure T(p; a, b) of that section, formula and rounding order.  The region of a source cell is
 *             the intersection of its four half-spaces T >= 0: for a convex cell, the cell.  A collapsed edge has a zero normal
 *             and clips nothing.  (The region of a non-convex cell is smaller than the cell; of a bow-tie, one lobe or nothing.)
 *   shared    T(a; a, b) and T(b; a, b) are 0 in exact arithmetic but a rounding-sized number of either sign as computed, and an
 *   corners   end that comes out negative would be cut off with a sliver of the cell (1e-12 of a half-degree cell).  So the measure
 *             d(v; e) of a vertex v against edge e = (Q_a, Q_b) is exactly 0 when the three components of v equal those of Q_a or of
 *             Q_b, and T(v; Q_a, Q_b) otherwise.  A mesh laid over itself, or over a mesh that shares its corners, then gives each
 *             cell whole: a cell that holds a target cell's four corners gives A_poly bit for bit.
 *   box       every valid cell of either grid has the padded box of "Point location": the component-wise min and max of its corner
 *             vectors, minus and plus 0.25 * L2 + 2^-40.  A pair is a CANDIDATE when both cells are valid and unmasked and the two
 *             boxes intersect, closed intervals on all three axes.  The box is part of the definition, so no index changes a bit.
 *   clip      Sutherland-Hodgman of the target polygon P0 .. P3 against the half-spaces of S, E, N, W in this order, inclusive inside
 *             tests (T >= 0), the emission rule of the lat-lon section: a pass emits its first vertex when inside, then per edge the
 *             crossing and then the end, and for the closing edge its crossing only.  The crossing of (v_k, v_k+1) with the measures
 *             d: order the ends as (e, f) lexicographically by (x, y, z); t = d_e / (d_e - d_f); w = e + t * (f - e) by component;
 *             the crossing is w / sqrt((w_x w_x + w_y w_y) + w_z w_z).  The result has at most 8 vertices.
 *   A_x       all sixteen measures of the target's corners >= 0: A_x = A_poly.  Otherwise (Re * Re) times the O3 fan from vertex 0
 *             of the clipped polygon, sum_k=1..n-2 O3(v_0, v_k, v_k+1) left to right from 0; 0 with fewer than 3 vertices.
 *   keep      A_x > 0 and A_x > threshold * min(A_poly, A_src)
 * Order: target cells row-major (m, n), then q ascending.  Nothing is summed across pairs, so the list is bit-identical for any band
 * split, any index (OGG_XGRID_CURV_CUBES: cubes per axis of the index over the source cells, 0: from their number;
 * OGG_XGRID_CURV_BRUTE=1: every valid source cell is tested against every target cell) and any launch geometry.
 * Counts: cells, degenerate, wide, inverted (they ignore the mask) and masked over the band's model cells; src_cells, src_degenerate,
 * src_wide, src_reversed, src_flat (they ignore the source mask), src_masked and src_large (valid unmasked source cells on the index's
 * large-cells list; every one of them with the brute knob) over the whole source, in every band's call; candidates and kept.
 * Out of scope: source cells wider than 30 degrees (they are WIDE), second-order weights, the reverse direction.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct ogg_xgrid_curv_src {
    const double *x, *y;       /* (NB + 1) rows of ld doubles: the corners in degrees */
    long NA, NB, ld;
    const unsigned char* mask; /* NULL, or one byte per source cell (NB x NA) */
} ogg_xgrid_curv_src;
typedef struct ogg_xgrid_curv_counts {
    long long cells, degenerate, wide, inverted, masked;
    long long src_cells, src_degenerate, src_wide, src_reversed, src_flat, src_masked, src_large;
    long long candidates, kept;
} ogg_xgrid_curv_counts;
/* the checks of the source's shape (no pointer is read): OGG_EARG unless it is as above */
int ogg_xgrid_curv_check(const ogg_xgrid_curv_src* src);
/* candidates < 0: the bytes of the sets workspace of a band and a source; candidates >= 0: the bytes of the pair workspace of a list of
 * that many candidates.  -1 on a bad band or source, or with 2^31 candidates or more. */
long ogg_xgrid_curv_workspace_bytes(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, long candidates);
/* sets step, device pointers, on a stream: the source cells' records and A_src (a_src, NB x NA doubles), their index, the band's
 * cells' records and A_poly (a_poly, (m1 - m0) x nx / 2 doubles), and the candidates of every model cell counted; every count but
 * kept into *counts (device memory).  counts->candidates sizes the pair workspace. */
int ogg_xgrid_curv_sets_dev(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, void* workspace, long workspace_bytes,
                            double* a_poly, double* a_src, ogg_xgrid_curv_counts* counts, void* stream);
/* clip step, after the sets step on the same band, source and workspace, with candidates = counts->candidates: the candidates as
 * sorted keys (target cell << 32) | q, A_x of every one and the kept pairs counted, into the pair workspace; counts->kept (the
 * length of the band's list) into *counts */
int ogg_xgrid_curv_clip_dev(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, const void* workspace, long workspace_bytes,
                            long candidates, void* pair_workspace, long pair_workspace_bytes, ogg_xgrid_curv_counts* counts,
                            void* stream);
/* write step, after the clip step on the same pair workspace: the list (counts->kept entries, device memory): src_ij[k] = (I, J),
 * ocn_ij[k] = (n, m) (0-based, m counted in the whole grid), area[k] = A_x */
int ogg_xgrid_curv_write_dev(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, long candidates, const void* pair_workspace,
                             long pair_workspace_bytes, int* src_ij, int* ocn_ij, double* area, void* stream);
/* HOST pointers throughout, staged through device memory, with the capacity protocol of ogg_xgrid (OGG_ESHAPE with *counts, a_poly and
 * a_src filled when counts->kept > capacity: call again with that capacity). */
int ogg_xgrid_curv(const ogg_xgrid_band* band, const ogg_xgrid_curv_src* src, long capacity, int* src_ij, int* ocn_ij, double* area,
                   double* a_poly, double* a_src, ogg_xgrid_curv_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Ocean mask: minimum depth and connected basins (an addition: the reference has none; GFDL's preprocessing calls this step "ice9").
 * Cells: the ny x nx cells of a topography result (model or supergrid cells), (j, i) with row 0 southmost, linear index c = j * nx + i,
 * ny * nx < 2^31.  Input: depth (ny x nx fp64), fill (topography's FILL), min_depth >= 0 and a mode.
 *   wet rule  a cell starts wet when depth > 0 and depth != fill (exchange_grid.wet_mask).  A wet cell with depth < min_depth
 *             becomes land in mode OGG_MASK_MASK, stays wet with depth min_depth in mode OGG_MASK_DEEPEN.  The rule is applied
 *             BEFORE connectivity: a sill made land cuts a basin off.
 *   topology  two wet cells are connected through a shared face only: (j, i) ~ (j, i+1), (j, i) ~ (j+1, i); with OGG_MASK_PERIODIC
 *             (j, nx-1) ~ (j, 0); with OGG_MASK_FOLD (ny-1, i) ~ (ny-1, nx-1-i).  Diagonal neighbours are not connected.  (The
 *             flags come from the grid's corner points, ocean_mask.detect_topology: periodic when every point row's first and last
 *             points are one point on the sphere, folded when the top point row maps onto itself reversed and is not one point;
 *             unit vectors compared, chordal distance <= 1e-9.)
 *   root      the root of a component is the smallest linear index among its cells: root[c] (-1 for land) does not depend on how
 *             the kernels ran
 *   seeds     (lon, lat) pairs; each picks the cell whose centre is nearest by chordal distance |u_c - u_s|^2 (unit vectors
 *             (cos lat cos lon, cos lat sin lon, sin lat), lon, lat * (pi / 180)), ties to the smaller index; the centre of a model
 *             cell is supergrid point (2j+1, 2i+1).  A seed on a land cell is an error (OGG_EARG naming the cell and its depth).
 *   keep      every component that holds a seed; without seeds the one with the most cells (ties: the smaller root); with
 *             keep_min_cells N > 0 also every component of at least N cells.  Every other wet cell becomes land.
 *   outputs   depth: removed and masked cells 0, deepened cells min_depth, kept cells and all others (land, fill, NaN) unchanged;
 *             wet (uint8) the final mask; root taken before selection; integer counts.  Everything is integer or a copy: the
 *             result is bit-identical for any launch geometry (OGG_MASK_TILE_ROWS).
 * A component list entry is (cells << 32) | (INT32_MAX - root): the largest entry is the largest component (ties: smaller root).
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_MASK_MASK = 0, OGG_MASK_DEEPEN = 1 };
#define OGG_MASK_PERIODIC 1
#define OGG_MASK_FOLD 2
#define OGG_MASK_MAX_SEEDS 1024
typedef struct ogg_mask_params {
    long ny, nx;
    int topology;             /* OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int mode;                 /* OGG_MASK_MASK or OGG_MASK_DEEPEN */
    double fill, min_depth;
    long long keep_min_cells; /* 0: off */
} ogg_mask_params;
typedef struct ogg_mask_counts {
    long long wet_in;         /* depth > 0 and != fill (apply step) */
    long long masked;         /* of those, made land by min_depth in mode mask (apply step) */
    long long deepened;       /* of those, deepened to min_depth in mode deepen (apply step) */
    long long components;     /* connected components of the wet set after the wet rule (= entries of the component list; label step) */
    long long largest;        /* the largest component list entry, 0 without a component (label step) */
    long long kept;           /* components kept (apply step) */
    long long removed;        /* wet cells made land by the selection (apply step) */
    long long wet_out;        /* wet cells of the final mask (apply step) */
} ogg_mask_counts;
long ogg_mask_workspace_bytes(const ogg_mask_params* p);      /* of the label and apply steps, -1 on bad sizes */
/* the checks of *p (sizes, mode, min_depth, fill, keep_min_cells): OGG_EARG with the reason, before any device work */
int ogg_mask_check(const ogg_mask_params* p);
/* label step, device pointers, on a stream: the wet rule, root[] (ny * nx), the component list into components (device memory, room
 * for ny * nx entries, in no particular order: sort it); *counts (device memory) is zeroed and gets components and largest.  The workspace
 * keeps what the apply step needs (the parents and the per-root cell counts). */
int ogg_mask_label_dev(const ogg_mask_params* p, const double* depth, void* workspace, long workspace_bytes, int* root,
                       long long* components, ogg_mask_counts* counts, void* stream);
/* seed lookup, device pointers: for seed s (lonlat[2 s], lonlat[2 s + 1] in degrees) the nearest model-cell centre, point (2j+1, 2i+1)
 * of x, y (point rows of ld doubles): out[2 s] the bits of the squared chordal distance, out[2 s + 1] the cell index */
int ogg_mask_seed_dev(const ogg_mask_params* p, const double* x, const double* y, long ld, int n_seeds, const double* lonlat,
                      long long* out, void* stream);
/* apply step, after the label step on the same workspace: kept[0 .. n_kept-1] the roots chosen on the host (sorted ascending, device
 * memory); also every root of at least keep_min_cells cells.  depth_out and wet (ny * nx); every count but components and largest
 * into *counts. */
int ogg_mask_apply_dev(const ogg_mask_params* p, const double* depth, const int* root, const void* workspace, long workspace_bytes,
                       const int* kept, int n_kept, double* depth_out, unsigned char* wet, ogg_mask_counts* counts, void* stream);
/* HOST pointers throughout, staged through device memory: both steps with the choice of kept roots in between.  x, y: the supergrid
 * points ((2 ny + 1) x (2 nx + 1)), needed only with seeds; seed_cells[n_seeds] the seeds' cells; components: the sorted component
 * list (largest first), at most capacity entries copied (counts->components says how many there are). */
int ogg_ocean_mask(const ogg_mask_params* p, const double* depth, const double* x, const double* y, int n_seeds, const double* lonlat,
                   double* depth_out, unsigned char* wet, int* root, long long* seed_cells, long long* components, long capacity,
                   ogg_mask_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Conservative remap (an addition: the reference has none).  First-order conservative remapping of fields on a global rectilinear
 * (lat-lon) source grid onto the model cells, with the exchange list of ogg_xgrid as the weights.
 *   source   edges lon (NA + 1) and lat (NB + 1) as ogg_xgrid_check_atm accepts them; values f[r][J][I], r < nrec (every dimension
 *            ahead of lat / lon), row 0 southmost, float32 or fp64 (dtype).  A value is MISSING when it is NaN or equals one of the
 *            n_fill <= 2 fill values, compared in the source's own type (the fill value converted to it).
 *   weights  the list of ogg_xgrid between the source edges (as the atmosphere) and the model cells, same threshold, optional uint8
 *            wet mask (dry cells have no entries), in list order: ocean cells row-major, then J, then a_I + s.
 *   remap    model cell c, record r, entries e_1 .. e_n of c in list order: W = sum A_e, S = sum (A_e * f_e) over the entries whose
 *            value is not missing, both left to right in fp64, each product rounded before it is added (no FMA).  W > 0: value S / W,
 *            flag OGG_REMAP_REMAPPED.
 *   fill     per record, by graph distance d through wet cells across faces: i +- 1 (with OGG_MASK_PERIODIC, (j, nx-1) ~ (j, 0)),
 *            j +- 1, and on the top row with OGG_MASK_FOLD the partner (ny-1, nx-1-i) (the ocean mask's topology).  Remapped cells
 *            have d = 0; a wet cell with W = 0 has d = 1 + min d(neighbour), and its value is the sum of the values of its neighbours
 *            with d = d(c) - 1, in the order S, W, E, N (N: the fold partner on the top row), left to right from 0, divided by
 *            their count: flag OGG_REMAP_FILLED.  Cells the fill does not reach, those with d > fill_max (fill_max >= 0) and every
 *            wet cell with W = 0 when the fill step is not run: flag OGG_REMAP_UNFILLED and value OGG_REMAP_FILL.
 *   dry      cells where the mask is 0: flag OGG_REMAP_DRY and value OGG_REMAP_FILL.
 * A value depends only on the list, the source and values at smaller distance, so the result is BIT-IDENTICAL for any launch geometry
 * (the OGG_REMAP_* environment knobs) and any split of the grid into ranks.  Output layout: values (fp64) and flags (uint8), both
 * (nrec, ny, nx), record-major.
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_REMAP_FLOAT32 = 0, OGG_REMAP_FLOAT64 = 1 };
enum { OGG_REMAP_DRY = 0, OGG_REMAP_REMAPPED = 1, OGG_REMAP_FILLED = 2, OGG_REMAP_UNFILLED = 3 };
#define OGG_REMAP_FILL 1.0e20
#define OGG_REMAP_MAX_FILLS 2
/* the cells are model rows m0 .. m0 + ny - 1 of a grid nx cells wide (the list's m are counted in the whole grid); the fill step
 * needs the whole grid (m0 = 0).  ny * nx < 2^31, nrec * ny * nx < 2^32, NA * NB < 2^31. */
typedef struct ogg_remap_params {
    long ny, nx, m0;
    long NA, NB, nrec;
    int dtype;                 /* OGG_REMAP_FLOAT32 / FLOAT64 */
    int n_fill;                /* 0 .. OGG_REMAP_MAX_FILLS */
    double fill[2];            /* the values that mark missing */
    int topology;              /* fill step: OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int fill_max;              /* fill step: the largest distance filled, < 0 for no limit */
} ogg_remap_params;
/* (record, cell) pairs by flag, and what the fill did */
typedef struct ogg_remap_counts {
    long long dry, remapped, filled, unfilled;
    long long bad_entries;     /* list entries outside the cells or the source (a list of other edges or rows): refuse the result */
    long long max_distance;    /* the largest distance filled */
    long long fronts;          /* fill fronts with cells (= max_distance) */
    long long launches;        /* fill launches, those on an empty frontier included */
} ogg_remap_counts;
long ogg_remap_workspace_bytes(const ogg_remap_params* p);  /* of the segment, remap and fill steps, -1 on a bad *p */
/* the checks of *p (sizes, dtype, n_fill, topology): OGG_EARG with the reason, before any device work */
int ogg_remap_check(const ogg_remap_params* p);
/* segment step, device pointers, on a stream: the [start, end) range of every cell's entries in the list (ocn_ij, n_entries pairs
 * (n, m) as ogg_xgrid_write_dev writes them), from the boundaries of ocn_ij (one pass, no sort), into the workspace */
int ogg_remap_segments_dev(const ogg_remap_params* p, const int* ocn_ij, long n_entries, void* workspace, long workspace_bytes,
                           void* stream);
/* remap step, after the segment step on the same workspace: f the source (nrec * NB * NA values of dtype), atm_ij / area the list,
 * mask NULL (every cell wet) or one byte per cell; values and flags (nrec * ny * nx) as above, wet cells with W = 0 flagged
 * OGG_REMAP_UNFILLED; *counts (device memory) is zeroed and gets dry, remapped, unfilled and bad_entries.  flags: an allocation
 * rounded up to a multiple of 4 bytes (the fill step changes flags by 32-bit compare-and-swap). */
int ogg_remap_dev(const ogg_remap_params* p, const void* f, const int* atm_ij, const double* area, long n_entries,
                  const unsigned char* mask, const void* workspace, long workspace_bytes, double* values, unsigned char* flags,
                  ogg_remap_counts* counts, void* stream);
/* fill step on the remap step's values and flags of the whole grid (m0 = 0): front by front, one launch per front for all records;
 * the host reads the frontier length every few fronts.  Updates filled, unfilled, max_distance, fronts and launches in *counts.
 * Waits for the stream: every OGG_REMAP_FRONTS_PER_READ fronts, to read the queue's head and stop when the front is empty. */
int ogg_remap_fill_dev(const ogg_remap_params* p, void* workspace, long workspace_bytes, double* values, unsigned char* flags,
                       ogg_remap_counts* counts, void* stream);
/* HOST pointers throughout, staged through device memory: the three steps (the fill when do_fill != 0) on the list atm_ij / ocn_ij /
 * area of n_entries entries; mask NULL or one byte per cell. */
int ogg_remap(const ogg_remap_params* p, const void* f, const int* atm_ij, const int* ocn_ij, const double* area, long n_entries,
              const unsigned char* mask, int do_fill, double* values, unsigned char* flags, ogg_remap_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Runoff mapping (an addition: the reference has none).  The discharge of every source cell of a global lat-lon runoff field moved to
 * the nearest wet coastal cell of the model grid, conserving the mass flux, as MOM6 set-ups do with river runoff and calving.
 *   cells    the ny x nx model cells of the stitched grid, c = j * nx + i.  Wet set: one byte per cell (0: land), depth > 0 of a
 *            topography or mask != 0 of an ocean mask.  Centre: supergrid point (2j+1, 2i+1), as the mask's seeds.  Area:
 *            A_c = (a[2j][2i] + a[2j+1][2i+1]) + (a[2j][2i+1] + a[2j+1][2i]) of the supergrid area (2 ny x 2 nx), fp64, in this order.
 *   targets  OGG_RUNOFF_COAST: the wet cells with at least one face neighbour that is land or does not exist; face neighbours are
 *            i +- 1 (with OGG_MASK_PERIODIC, (j, nx-1) ~ (j, 0)), j +- 1, and on the top row with OGG_MASK_FOLD the partner
 *            (ny-1, nx-1-i) (the ocean mask's topology).  OGG_RUNOFF_WET: every wet cell.  The target list is in ascending c.
 *   sources  edges lon (NA + 1) and lat (NB + 1) as ogg_xgrid_check_atm accepts them; values f[r][J][I], r < nrec, float32 or fp64,
 *            MISSING when NaN or equal to one of n_fill <= 2 fill values (compared in the source's type), as for the remap.  A
 *            source cell is MAPPED when some record holds a value there that is neither missing nor zero; every other source cell
 *            contributes nothing (SKIPPED when it has a non-missing value, MISSING when it has none).  Centre
 *            ((a_I + a_I+1) / 2, (b_J + b_J+1) / 2); area A_s = (Re * Re) * (a_I+1 * D - a_I * D) * ds_J, left to right, ds_J as
 *            for A_atm of the exchange grid.
 *   nearest  unit vectors u = (cos phi cos lam, cos phi sin lam, sin phi), lam = lon * D, phi = lat * D (D = pi / 180, one fp64
 *            constant); d2 = (dx * dx + dy * dy) + dz * dz, d = u_s - u_t, no FMA.  Every mapped source goes to the target with
 *            the smallest (d2, c): ties to the smaller cell.  The answer is a function of the unit vectors alone: the search index
 *            (OGG_RUNOFF_BINS, OGG_RUNOFF_BRUTE) changes no bit.  No target while a source is mapped: OGG_EARG.
 *   values   for cell c and record r, the mapped sources s with target c in ASCENDING s: S = sum (f_s * A_s), left to right from
 *            +0.0, missing values skipped, each product rounded before it is added; value S / A_c.  Every cell without a source,
 *            land included, is +0.0.  n_sources[c]: the number of mapped sources of c.
 * Nothing is summed across cells in an order that depends on the launch, so the result is BIT-IDENTICAL for any launch geometry and,
 * on the gathered grid, for any rank count.  Output layout: values (nrec, ny, nx) fp64, record-major; n_sources (ny, nx) int32.
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_RUNOFF_COAST = 0, OGG_RUNOFF_WET = 1 };
#define OGG_RUNOFF_MAX_BINS 160   /* the largest OGG_RUNOFF_BINS: cubes per axis of the search index */
/* ny * nx < 2^31, NA * NB < 2^31, nrec * ny * nx < 2^32, nrec * NA * NB < 2^40 */
typedef struct ogg_runoff_params {
    long ny, nx;               /* model cells */
    long NA, NB, nrec;         /* source cells and records */
    int dtype;                 /* OGG_REMAP_FLOAT32 / FLOAT64 */
    int n_fill;                /* 0 .. OGG_REMAP_MAX_FILLS */
    double fill[2];            /* the values that mark missing */
    int topology;              /* OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int targets;               /* OGG_RUNOFF_COAST / OGG_RUNOFF_WET */
    double Re;                 /* sphere radius of A_s */
} ogg_runoff_params;
typedef struct ogg_runoff_counts {
    long long targets;         /* target cells (targets step) */
    long long mapped, skipped, missing;   /* source cells by kind (sources step) */
    long long cells;           /* model cells with at least one source (accumulate step) */
    long long max_sources;     /* the largest n_sources (accumulate step) */
    long long tests;           /* distance tests of the search (search step) */
    long long bins;            /* cubes per axis of the search index, 0 for brute force (search step) */
} ogg_runoff_counts;
long ogg_runoff_workspace_bytes(const ogg_runoff_params* p); /* of every step, -1 on a bad *p */
/* the checks of *p (sizes, dtype, n_fill, topology, targets, Re): OGG_EARG with the reason, before any device work */
int ogg_runoff_check(const ogg_runoff_params* p);
/* targets step, device pointers, on a stream: x, y the supergrid points (2 ny + 1 rows of ld doubles), wet one byte per cell; the
 * target list tgt_cell (room for ny * nx) in ascending c with its unit vectors tgt_u (3 per target); *counts (device memory) is
 * zeroed and gets targets. */
int ogg_runoff_targets_dev(const ogg_runoff_params* p, const double* x, const double* y, long ld, const unsigned char* wet,
                           void* workspace, long workspace_bytes, int* tgt_cell, double* tgt_u, ogg_runoff_counts* counts, void* stream);
/* sources step: f (nrec * NB * NA values of dtype), lon / lat the edges (device memory); the mapped list src_cell (room for NA * NB,
 * J * NA + I) in ascending order with its unit vectors src_u (3 per source), ds (NB values of ds_J); mapped, skipped and missing into
 * *counts.  The workspace keeps A_s of every mapped source for the accumulate step. */
int ogg_runoff_sources_dev(const ogg_runoff_params* p, const void* f, const double* lon, const double* lat, void* workspace,
                           long workspace_bytes, int* src_cell, double* src_u, double* ds, ogg_runoff_counts* counts, void* stream);
/* search step, after the first two (n_targets, n_mapped their counts): for every mapped source its target cell src_target and the
 * bits of its d2 (src_d2); tests and bins into *counts. */
int ogg_runoff_search_dev(const ogg_runoff_params* p, const int* tgt_cell, const double* tgt_u, long n_targets, const double* src_u,
                          long n_mapped, void* workspace, long workspace_bytes, int* src_target, double* src_d2,
                          ogg_runoff_counts* counts, void* stream);
/* segments step: the mapped sources grouped by target cell, in ascending source order within a cell, into the workspace */
int ogg_runoff_segments_dev(const ogg_runoff_params* p, const int* src_target, long n_mapped, void* workspace, long workspace_bytes,
                            void* stream);
/* accumulate step, after the segments step: values (nrec * ny * nx) and n_sources (ny * nx) as above, from f, src_cell and the
 * supergrid area (2 ny rows of lda doubles); cells and max_sources into *counts. */
int ogg_runoff_accumulate_dev(const ogg_runoff_params* p, const void* f, const int* src_cell, long n_mapped, const double* area, long lda,
                              const void* workspace, long workspace_bytes, double* values, int* n_sources, ogg_runoff_counts* counts,
                              void* stream);
/* HOST pointers throughout, staged through device memory: the five steps on the supergrid x, y ((2 ny + 1) x (2 nx + 1)) and area
 * (2 ny x 2 nx).  src_cell, src_target, src_d2: room for NA * NB (counts->mapped are written). */
int ogg_runoff(const ogg_runoff_params* p, const double* x, const double* y, const double* area, const unsigned char* wet,
               const void* f, const double* lon, const double* lat, double* values, int* n_sources, int* src_cell, int* src_target,
               double* src_d2, ogg_runoff_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Runoff spreading (an addition: the reference has none).  The mapped runoff of every loaded cell (a MOUTH) spread over the wet cells
 * within a radius, conserving the mass flux, as MOM6, CESM and ACCESS set-ups do before they use a mapped runoff: the mapping alone
 * puts a whole river into one cell.
 *   cells       the runoff mapping's: ny x nx model cells, c = j * nx + i, ny * nx < 2^31; centre the supergrid point (2j+1, 2i+1),
 *               unit vector u_c by the mapping's formula, A_c as the mapping forms it; wet one byte per cell; cls NULL or one int32
 *               class per cell (a basin code; 0 is a class like any other); load one int32 per cell (the mapping's n_sources, or any
 *               array): load[c] > 0 makes c a MOUTH.  The mouth list is in ascending c.
 *   candidates  the cells that are wet, whose centre coordinates are both finite and with 0 < A_c < +inf.  A mouth that is no
 *               candidate is refused: OGG_EARG names the first such cell in ascending c, before any value is written.
 *   receivers   R(m): the candidates t with d2(u_m, u_t) <= r2, d2 = (dx * dx + dy * dy) + dz * dz, d = u_m - u_t, no FMA, and with
 *               cls also cls[t] == cls[m].  r2 is fp64, 0 < r2 <= 4: the squared chord of the radius, (2 sin(R / (2 Re)))^2.  m is
 *               in R(m).  Membership is a function of d2 alone: a receiver reachable both ways round a periodic band is one
 *               receiver, and the seam and the fold are no special cases.
 *   weights     from correctly rounded + - * / only.  a = min(A_t / A_m, 256.0); g = 1.0 (OGG_SPREAD_UNIFORM) or h * h with
 *               h = 1.0 - d2 / r2 (OGG_SPREAD_BIWEIGHT); q(m, t) = (long long) floor((a * g) * 16777216.0), so 0 <= q <= 2^32 and
 *               q(m, m) = 2^24; W_m = the sum of q(m, t) over R(m) in int64 (exact, so its order is free; W_m > 0);
 *               s(m, t) = (double) q / (double) W_m, each conversion rounded to nearest even.  A receiver with d2 == r2 has q = 0: it
 *               counts as a receiver and contributes its +0.0 term.
 *   values      F = v[r][m] * A_m; T[r][t] = the sum over the mouths m with t in R(m), in ASCENDING m, left to right from +0.0, of
 *               F * s(m, t), each product rounded before it is added; out[r][t] = T / A_t.  n_mouths[t]: the number of those
 *               mouths; a cell with none gets +0.0 whatever its input.  Input values are not inspected: NaN, negative values and
 *               -0.0 go through the arithmetic.
 *   limits      the pair count P = the sum of |R(m)| over the mouths must be below OGG_SPREAD_MAX_PAIRS, else OGG_EARG names P (the
 *               environment's OGG_SPREAD_MAX_PAIRS_TEST can lower the limit, never raise it).
 * Every output is a function of u, A, wet, cls, load and v alone: the cubes of the index (OGG_SPREAD_CUBES 1 .. OGG_SPREAD_MAX_CUBES
 * per axis, default clamp(floor(2 / sqrt(r2)), 1, OGG_SPREAD_MAX_CUBES); OGG_SPREAD_BRUTE=1 tests every candidate), the launch geometry
 * and, on the gathered grid, the rank count change no bit.  Caveats: a disc reaches across an isthmus narrower than the radius unless
 * classes keep it out; the biweight shape is not CESM's exponential e-folding (exp is not bit-reproducible between hosts and the
 * device); the area ratio is capped at 256.
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_SPREAD_UNIFORM = 0, OGG_SPREAD_BIWEIGHT = 1 };
#define OGG_SPREAD_MAX_CUBES 64          /* the largest OGG_SPREAD_CUBES: cubes per axis of the candidate index */
#define OGG_SPREAD_MAX_PAIRS (1L << 30)  /* P must be below this */
/* ny * nx < 2^31, nrec * ny * nx < 2^32 */
typedef struct ogg_spread_params {
    long ny, nx;               /* model cells */
    long nrec;                 /* records of v */
    int shape;                 /* OGG_SPREAD_UNIFORM / OGG_SPREAD_BIWEIGHT */
    int use_classes;           /* 1: receivers share their mouth's class (cls must be given) */
    double r2;                 /* squared chordal radius, 0 < r2 <= 4 */
} ogg_spread_params;
typedef struct ogg_spread_counts {
    long long candidates;      /* candidate cells (sets step) */
    long long mouths;          /* mouths (sets step) */
    long long pairs;           /* P (count step) */
    long long max_receivers;   /* the largest |R(m)| (count step) */
    long long loaded;          /* cells with n_mouths > 0 (apply step) */
    long long max_mouths;      /* the largest n_mouths (apply step) */
    long long tests;           /* distance tests of the count step */
    long long cubes;           /* cubes per axis of the index, 0 for brute force (sets step) */
} ogg_spread_counts;
/* of every step with n_pairs = P; with n_pairs = 0 of the sets and count steps, which run before P is known.  The smaller workspace is
 * a PREFIX of the larger: its bytes copied to the front of the larger one carry the sets step's index over.  -1 on a bad *p or when
 * n_pairs is not below the limit (ogg_last_error names P). */
long ogg_spread_workspace_bytes(const ogg_spread_params* p, long n_pairs);
/* the checks of *p (sizes, shape, use_classes, r2): OGG_EARG with the reason, before any device work */
int ogg_spread_check(const ogg_spread_params* p);
/* sets step, device pointers, on a stream: x, y the supergrid points (2 ny + 1 rows of ld doubles), area the supergrid area (2 ny rows
 * of lda doubles), wet and load per cell; u (3 per cell), A and the candidate flag cand (one byte) of EVERY cell, the mouth list
 * mouth_cell (room for ny * nx) in ascending c; the candidates sorted into cubes in the workspace; *counts (device memory) is zeroed
 * and gets candidates, mouths and cubes.  Waits for the stream: a mouth that is no candidate is OGG_EARG here. */
int ogg_spread_sets_dev(const ogg_spread_params* p, const double* x, const double* y, long ld, const double* area, long lda,
                        const unsigned char* wet, const int* load, void* workspace, long workspace_bytes, double* u, double* A,
                        unsigned char* cand, int* mouth_cell, ogg_spread_counts* counts, void* stream);
/* count step (n_mouths: the sets step's count): mouth_n = |R(m)| and mouth_W = W_m of every mouth; pairs, max_receivers and tests
 * into *counts.  cls: NULL unless use_classes. */
int ogg_spread_count_dev(const ogg_spread_params* p, const double* u, const double* A, const int* cls, const int* mouth_cell,
                         long n_mouths, void* workspace, long workspace_bytes, int* mouth_n, long long* mouth_W,
                         ogg_spread_counts* counts, void* stream);
/* pairs step (n_pairs: the count step's pairs, which the workspace must be sized for): every pair's key sorted, and every cell's
 * mouths as a segment in ascending mouth order, into the workspace */
int ogg_spread_pairs_dev(const ogg_spread_params* p, const double* u, const int* cls, const int* mouth_cell, const int* mouth_n,
                         long n_mouths, long n_pairs, void* workspace, long workspace_bytes, void* stream);
/* apply step, after the pairs step: out (nrec * ny * nx fp64, record-major) and n_mouths (ny * nx) as above from v (nrec * ny * nx
 * fp64); loaded and max_mouths into *counts. */
int ogg_spread_apply_dev(const ogg_spread_params* p, const double* v, const double* u, const double* A, const int* mouth_cell,
                         const long long* mouth_W, long n_mouths, long n_pairs, const void* workspace, long workspace_bytes, double* out,
                         int* n_mouths_out, ogg_spread_counts* counts, void* stream);
/* HOST pointers throughout, staged through device memory: the four steps on the supergrid x, y ((2 ny + 1) x (2 nx + 1)) and area
 * (2 ny x 2 nx).  mouth_cell, mouth_n, mouth_W: room for ny * nx (counts->mouths are written).  cls: NULL unless use_classes. */
int ogg_runoff_spread(const ogg_spread_params* p, const double* x, const double* y, const double* area, const unsigned char* wet,
                      const int* cls, const int* load, const double* v, double* out, int* n_mouths, int* mouth_cell, int* mouth_n,
                      long long* mouth_W, ogg_spread_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Conservative regrid to a lat-lon grid (an addition: the reference has none).  Fields on the model cells aggregated first-order
 * conservatively onto the cells of a global rectilinear grid: the remap's direction reversed, with the same exchange list as weights.
 *   target   edges lon (NA + 1) and lat (NB + 1) as ogg_xgrid_check_atm accepts them; cell k = J * NA + I; A_atm(J, I) its area by
 *            the keep step's formula of the exchange grid, passed in by the caller (a_atm, NB x NA fp64: exchange_grid.atm_area forms
 *            it on the host, so the device's fractions and the host's share it bit for bit).  The calls take neither the edges nor a
 *            check of a_atm: the CALLER is responsible for a_atm belonging to the edges the list was built with (it is used as given).
 *   field    g[r][m][n], r < nrec, (m, n) the ny x nx model cells of the stitched grid, float32 or fp64 (dtype; float32 converted
 *            exactly to fp64).  A value is MISSING when it is NaN or equals one of the n_fill <= 2 fill values, compared in the
 *            field's own type (the remap's rule).
 *   weights  the list of ogg_xgrid between the target edges (as the atmosphere) and the model cells, same threshold, optional uint8
 *            wet mask, in list order (the canonical order Supergrid.exchange_grid gathers).
 *   transpose  the entries of target cell k in ASCENDING list position (the keys (k << 32) | position are unique, so any correct
 *            sort gives this permutation).
 *   static   W0_k = sum A_e over every entry of k, left to right from +0.0 in fp64, no FMA (what np.bincount(k, weights=area) gives);
 *            ocean_frac_k = W0_k / A_atm; n_entries_k.
 *   records  W = sum A_e and S = sum (A_e * g_e) over the entries whose value is not missing, left to right from +0.0, each product
 *            rounded before it is added.  OGG_REGRID_AREA: value S / W when W > 0, else OGG_REMAP_FILL (the mean over the part of
 *            the cell with valid values).  OGG_REGRID_CELL: value S / A_atm, 0 where W = 0 (conserves a flux over the whole cell).
 *            cover (optional) = W / A_atm.
 * Every output is a fixed function of the list, the field and a_atm: BIT-IDENTICAL for any launch geometry (the OGG_REGRID_* knobs),
 * run and, on the gathered list, rank count.  Output layout: values and cover (nrec, NB, NA) fp64, record-major; frac (NB, NA) fp64 and
 * n_entries (NB, NA) int32.
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_REGRID_AREA = 0, OGG_REGRID_CELL = 1 };
/* ny * nx < 2^31, NA * NB < 2^31, nrec * NB * NA < 2^32; list length < 2^31 (the calls) */
typedef struct ogg_regrid_params {
    long ny, nx;               /* model cells */
    long NA, NB, nrec;         /* target cells and records */
    int dtype;                 /* OGG_REMAP_FLOAT32 / FLOAT64 */
    int n_fill;                /* 0 .. OGG_REMAP_MAX_FILLS */
    double fill[2];            /* the values that mark missing */
    int normalize;             /* OGG_REGRID_AREA / OGG_REGRID_CELL */
} ogg_regrid_params;
typedef struct ogg_regrid_counts {
    long long entries;         /* list entries transposed (transpose step) */
    long long bad_entries;     /* list entries outside the cells or the target (a list of other edges or rows): refuse the result */
    long long cells;           /* target cells with entries (regrid step) */
    long long max_entries;     /* the largest n_entries (regrid step) */
    long long valid;           /* (record, cell) pairs with W > 0 (regrid step) */
    long long empty;           /* (record, cell) pairs with W = 0 (regrid step) */
} ogg_regrid_counts;
long ogg_regrid_workspace_bytes(const ogg_regrid_params* p, long n_entries); /* of both steps, -1 on a bad *p or length */
/* the checks of *p (sizes, dtype, n_fill, normalize): OGG_EARG with the reason, before any device work */
int ogg_regrid_check(const ogg_regrid_params* p);
/* transpose step, device pointers, on a stream: the list (atm_ij, ocn_ij, area; n_entries entries as ogg_xgrid_write_dev writes
 * them) grouped by target cell in ascending list position, into the workspace; *counts (device memory) is zeroed and gets entries and
 * bad_entries. */
int ogg_regrid_transpose_dev(const ogg_regrid_params* p, const int* atm_ij, const int* ocn_ij, const double* area, long n_entries,
                             void* workspace, long workspace_bytes, ogg_regrid_counts* counts, void* stream);
/* regrid step, after the transpose step on the same workspace and list length n_list: f the field (nrec * ny * nx values of dtype;
 * NULL with values NULL), a_atm (NB * NA); values, cover, frac, n_entries each NULL or as above (values NULL: no record is read, the
 * static sums only).  Every call sets cells and max_entries in *counts, and valid and empty (0 without values), from zero; entries and
 * bad_entries stay the transpose step's.  The workspace keeps the transpose; the step also writes its list of long cells there. */
int ogg_regrid_dev(const ogg_regrid_params* p, const void* f, const double* a_atm, long n_list, void* workspace, long workspace_bytes,
                   double* values, double* cover, double* frac, int* n_entries, ogg_regrid_counts* counts, void* stream);
/* HOST pointers throughout, staged through device memory: both steps on the list atm_ij / ocn_ij / area of n_entries entries; f and
 * values NULL together (the static sums only), cover / frac / n_out NULL to skip. */
int ogg_regrid(const ogg_regrid_params* p, const void* f, const int* atm_ij, const int* ocn_ij, const double* area, long n_entries,
               const double* a_atm, double* values, double* cover, double* frac, int* n_out, ogg_regrid_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Bilinear interpolation (an addition: the reference has none).  Scalar and vector fields on a global rectilinear (lat-lon) source
 * interpolated between the source's cell centres at the h, u or v points of the grid, and vectors turned from (east, north) to the
 * grid's own x and y directions with angle_dx.
 *   source   as for the remap: edges lon (NA + 1, spanning 360 degrees) and lat (NB + 1, increasing), values f[r][J][I], float32 or
 *            fp64 (float32 converted exactly), MISSING when NaN or equal to one of n_fill <= 2 fill values in the source's own type.
 *            The nodes are the centres lonc[I] = (lon[I] + lon[I+1]) / 2 and latc[J] = (lat[J] + lat[J+1]) / 2.
 *   points   of a supergrid of (2 ny + 1) x (2 nx + 1) points: OGG_BILINEAR_H (2j+1, 2i+1), ny x nx; OGG_BILINEAR_U (2j+1, 2i),
 *            ny x (nx + 1); OGG_BILINEAR_V (2j, 2i+1), (ny + 1) x nx; OGG_BILINEAR_C (vectors only): the first component at the U
 *            points, the second at the V points.
 *   locate   point (x, y), all in fp64, no FMA.  c[I] = lonc[I] - lonc[0]; t = x - lonc[0]; t = t - 360 * floor(t / 360); t = 0
 *            unless 0 <= t < 360.  I: the last index with c[I] <= t; I1 = (I + 1) mod NA; c1 = c[I + 1], or c[0] + 360 after the last
 *            node; wx = (t - c[I]) / (c1 - c[I]).  y <= latc[0]: J = J1 = 0, wy = 0; y >= latc[NB-1]: J = J1 = NB - 1, wy = 0 (the
 *            clamps beyond the first and last centres); otherwise J the last index with latc[J] <= y, J1 = J + 1,
 *            wy = (y - latc[J]) / (latc[J1] - latc[J]).  A NaN latitude lies between no two nodes: the point has no corners (value
 *            OGG_REMAP_FILL, flag OGG_REMAP_UNFILLED, or OGG_REMAP_DRY under a dry mask cell), whatever the source holds; at the H
 *            points the fill treats it as any other unfilled point.  A NaN or infinite longitude is t = 0 by the rule above.
 *   value    weights (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy of the corners (J,I), (J,I1), (J1,I), (J1,I1), in that order.  S = sum
 *            (w * f) and W = sum w over the corners that are not missing, left to right from +0.0, each product rounded before it is
 *            added.  All four corners valid: value S; some valid and W > 0: S / W; both flag OGG_REMAP_REMAPPED.  Otherwise value
 *            OGG_REMAP_FILL and flag OGG_REMAP_UNFILLED.  With a mask (H points only), dry cells: OGG_REMAP_DRY and OGG_REMAP_FILL.
 *   vectors  a corner is valid only where both components are; both are interpolated with the same weights, so they have the same
 *            flags (two copies, one per component: the fill changes flags in place).
 *   fill     H points only: ogg_remap_fill_dev on each component's values and flags (same codes, fill_max and topology), while the
 *            components are still eastward and northward.  U, V and C points have no mask and no fill: a point with no valid corner
 *            stays OGG_REMAP_UNFILLED.
 *   rotate   last.  a = angle_dx at the point (degrees); (sa, ca) = sincospi(a / 180); ug = U * ca + V * sa, vg = V * ca - U * sa,
 *            products rounded, one addition each; points flagged OGG_REMAP_DRY or OGG_REMAP_UNFILLED keep OGG_REMAP_FILL.  ca and sa of
 *            every point are returned (rot_cos, rot_sin), so everything downstream of them is bit for bit.  At C points ug is formed
 *            at the U points and vg at the V points, each from both components interpolated there.
 * Every value is a function of one point, the source and the angle there: BIT-IDENTICAL for any launch geometry (the OGG_BILINEAR_*
 * environment knobs), run and rank count.  Output layout: values (fp64) and flags (uint8), (nrec, rows, columns), record-major.
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_BILINEAR_H = 0, OGG_BILINEAR_U = 1, OGG_BILINEAR_V = 2, OGG_BILINEAR_C = 3 };
/* ny * nx model cells, the supergrid rows given starting at model row m0 of the stitched grid (the fill needs m0 = 0);
 * (ny + 1) * (nx + 1) < 2^31, nrec * (ny + 1) * (nx + 1) < 2^32, NA * NB < 2^31 */
typedef struct ogg_bilinear_params {
    long ny, nx, m0;
    long NA, NB, nrec;
    int dtype;                 /* OGG_REMAP_FLOAT32 / FLOAT64 */
    int n_fill;                /* 0 .. OGG_REMAP_MAX_FILLS */
    double fill[2];            /* the values that mark missing */
    int points;                /* OGG_BILINEAR_H / U / V / C */
    int ncomp;                 /* 1: a scalar, 2: a vector (eastward, northward) */
    int topology;              /* fill step: OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int fill_max;              /* fill step: the largest distance filled, < 0 for no limit */
} ogg_bilinear_params;
/* the checks of *p (sizes, dtype, n_fill, points, ncomp, C for a scalar, topology) and of a mask away from the H points: OGG_EARG
 * with the reason, before any device work */
int ogg_bilinear_check(const ogg_bilinear_params* p, int has_mask);
/* locate and interpolate, device pointers, on a stream.  x, y: the supergrid points (2 ny + 1 rows of ld doubles); lon, lat: the
 * source's edges; f (and f2 for a vector): nrec * NB * NA values of dtype; mask: NULL or one byte per model cell (H points only).
 * values / flags: the scalar, or the first component; values2 / flags2: the second component (at C points on the V points' shape).
 * cross / cross2 (C points only, NULL to skip, needed by the rotation): the second component at the U points and the first at the V
 * points.  flags, flags2: allocations rounded up to a multiple of 4 bytes when the fill step follows. */
int ogg_bilinear_dev(const ogg_bilinear_params* p, const double* x, const double* y, long ld, const double* lon, const double* lat,
                     const void* f, const void* f2, const unsigned char* mask, double* values, unsigned char* flags, double* values2,
                     unsigned char* flags2, double* cross, double* cross2, void* stream);
/* the rotation of a vector's components (ncomp = 2) in place, after ogg_bilinear_dev (and the fill): angle the supergrid's angle_dx
 * (2 ny + 1 rows of ld doubles); rot_cos / rot_sin one value per point (at C points: of the U points, and rot_cos2 / rot_sin2 of the V
 * points; NULL otherwise).  rotate = 0: the cosines and sines only, the components stay eastward and northward. */
int ogg_bilinear_rotate_dev(const ogg_bilinear_params* p, const double* angle, long ld, double* values, const unsigned char* flags,
                            double* values2, const unsigned char* flags2, const double* cross, const double* cross2, double* rot_cos,
                            double* rot_sin, double* rot_cos2, double* rot_sin2, int rotate, void* stream);
/* HOST pointers throughout, staged through device memory: interpolate, the fill when do_fill != 0 (H points), the rotation for a
 * vector (angle NULL: no rotation and no rot_cos / rot_sin).  Arrays of a scalar's second component are NULL. */
int ogg_bilinear(const ogg_bilinear_params* p, const double* x, const double* y, const double* angle, const double* lon,
                 const double* lat, const void* f, const void* f2, const unsigned char* mask, int do_fill, int rotate, double* values,
                 unsigned char* flags, double* values2, unsigned char* flags2, double* rot_cos, double* rot_sin, double* rot_cos2,
                 double* rot_sin2);

/* ------------------------------------------------------------------------------------------------------
 * Distance to the coast (an addition: the reference has none).  For every model cell the nearest cell across the coast, as MOM6
 * set-ups need it to taper salinity restoring near land, to spread runoff and to build sponges.
 *   cells    the ny x nx model cells, c = j * nx + i, one wet byte per cell (0: land) and the centre at supergrid point (2j+1, 2i+1),
 *            as for the runoff mapping.  A cell is VALID when its centre's longitude and latitude are both finite.
 *   nearest  unit vectors and d2 = (dx * dx + dy * dy) + dz * dz exactly as "Runoff mapping" forms them (the same D, no FMA; one
 *            shared implementation), and nearest by the key (d2, c'): ties to the smaller cell.
 *   face neighbours  the ocean mask's: i +- 1 (with OGG_MASK_PERIODIC, (j, nx-1) ~ (j, 0)), j +- 1, and on the top row with
 *            OGG_MASK_FOLD the partner (ny-1, nx-1-i).  A neighbour that does not exist is NOT a neighbour: the grid's edge is no
 *            coast.  (This differs from OGG_RUNOFF_COAST, which counts a missing neighbour as land.)  On a fold of odd width the
 *            middle cell is its own partner and is not thereby coastal.
 *   coastal  a cell with at least one face neighbour of the other wetness.  Wetness alone decides this: an invalid neighbour still
 *            makes its neighbour coastal through its wet byte.  L: the VALID coastal land cells; W: the VALID coastal wet cells; both
 *            lists in ascending c.
 *   answer   a valid wet cell gets the member of L with the smallest (d2, c'), a valid land cell the member of W with the smallest
 *            (d2, c').  sides (OGG_COAST_WET | OGG_COAST_LAND) selects which cells are queried.  A cell that is not queried, is
 *            invalid, or whose opposite set is empty gets nearest = -1 and d2 = +inf.  A cell is never its own answer.
 *   flags    one byte per cell: bit 0 wet, bit 1 coastal, bit 2 valid.
 * nearest and d2 are a function of the unit vectors and the wet bytes alone: no search index, tile shape, launch geometry or knob
 * (OGG_COAST_BRUTE, OGG_COAST_CUBES, OGG_COAST_TILE_X, OGG_COAST_TILE_Y, OGG_COAST_CHUNK) changes a bit, and neither does the rank
 * count on the gathered grid.  The distance in metres is not a device output: coast_distance.py forms
 * Re * (2 * arcsin(minimum(1, 0.5 * sqrt(d2)))) with numpy from d2, and writes 1e20 where nearest = -1.
 * Output layout: nearest (ny, nx) int32; d2 (ny, nx) fp64.
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_COAST_WET = 1, OGG_COAST_LAND = 2 };
#define OGG_COAST_MAX_CUBES 128   /* the largest OGG_COAST_CUBES: cubes per axis of the search index */
/* ny * nx < 2^31 */
typedef struct ogg_coast_params {
    long ny, nx;               /* model cells */
    int topology;              /* OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int sides;                 /* OGG_COAST_WET | OGG_COAST_LAND: the cells that are queried */
} ogg_coast_params;
typedef struct ogg_coast_counts {
    long long coast_wet;       /* members of W (sets step) */
    long long coast_land;      /* members of L (sets step) */
    long long queries;         /* valid cells of the selected sides (sets step) */
    long long answered;        /* queries with an answer (search step) */
    long long tests;           /* distance tests (search step) */
    long long tiles;           /* tiles of cells, one workgroup each (search step) */
    long long cubes;           /* cubes per axis of the search index, 0 for brute force (search step) */
} ogg_coast_counts;
long ogg_coast_workspace_bytes(const ogg_coast_params* p);   /* of both steps, -1 on a bad *p */
/* the checks of *p (sizes, topology, sides): OGG_EARG with the reason, before any device work */
int ogg_coast_check(const ogg_coast_params* p);
/* sets step, device pointers, on a stream: x, y the supergrid points (2 ny + 1 rows of ld doubles), wet one byte per cell; flags
 * (ny * nx bytes) and u (3 doubles per cell) of every cell; the lists land_cell / wet_cell (room for ny * nx each) in ascending c with
 * their unit vectors land_u / wet_u (3 per member); *counts (device memory) is zeroed and gets coast_wet, coast_land and queries. */
int ogg_coast_sets_dev(const ogg_coast_params* p, const double* x, const double* y, long ld, const unsigned char* wet, void* workspace,
                       long workspace_bytes, unsigned char* flags, double* u, int* land_cell, double* land_u, int* wet_cell,
                       double* wet_u, ogg_coast_counts* counts, void* stream);
/* search step, after the sets step (n_land, n_wet its counts): nearest and the bits of d2 for every cell as above; answered, tests,
 * tiles and cubes into *counts, from zero. */
int ogg_coast_search_dev(const ogg_coast_params* p, const unsigned char* flags, const double* u, const int* land_cell,
                         const double* land_u, long n_land, const int* wet_cell, const double* wet_u, long n_wet, void* workspace,
                         long workspace_bytes, int* nearest, double* d2, ogg_coast_counts* counts, void* stream);
/* HOST pointers throughout, staged through device memory: both steps on the supergrid x, y ((2 ny + 1) x (2 nx + 1)); nearest, d2 and
 * flags one value per cell. */
int ogg_coast_distance(const ogg_coast_params* p, const double* x, const double* y, const unsigned char* wet, int* nearest, double* d2,
                       unsigned char* flags, ogg_coast_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Basin codes (an addition: the reference has none).  The integer basin of every wet model cell (Southern Ocean, Atlantic, Pacific,
 * ...), as MOM6 set-ups keep it in basin_codes.nc for transports by basin, regional restoring and analysis masks: an ordered list
 * of seeded floods, each confined to a longitude / latitude box, later floods taking only what earlier ones left.
 *   cells    the ocean mask's: ny x nx model cells, c = j * nx + i, ny * nx < 2^31; faces (j, i) ~ (j, i+1) and (j, i) ~ (j+1, i),
 *            with OGG_MASK_PERIODIC (j, nx-1) ~ (j, 0), with OGG_MASK_FOLD (ny-1, i) ~ (ny-1, nx-1-i); diagonal neighbours are not
 *            connected.  The centre of a cell is supergrid point (2j+1, 2i+1); a cell is VALID when both centre coordinates are
 *            finite.  wet: one byte per cell, non-zero wet.
 *   rules    K of them in order, 1 <= K <= OGG_BASIN_MAX_RULES; rule k = (code, seed_lon, seed_lat, lon_w, lon_e, lat_s, lat_n) with
 *            1 <= code <= 255 (several rules may share a code: an ocean usually needs several floods), -90 <= lat_s <= lat_n <= 90,
 *            0 < lon_e - lon_w <= 360, every value finite, and the seed in its own box by the predicate below (OGG_EARG names the
 *            rule otherwise).
 *   in the box  a valid centre (lon, lat) is in box k when lat_s <= lat <= lat_n and, with W = lon_e - lon_w, t = lon - lon_w and
 *            t = t - 360.0 * floor(t / 360.0): W == 360 or t <= W.  The operations are evaluated in exactly this order, each rounded
 *            on its own (no FMA), so the same bits come out of numpy.  Both edges belong to the box, and so does a centre stated any
 *            number of whole turns away.  A t that rounds to exactly 360.0 (lon a hair west of lon_w) is in the box only when
 *            W == 360.
 *   seed cell  of rule k: the valid cell whose centre is nearest to the seed by the key (bits of d2, c), d2 = dist2(u_c, u_seed) of
 *            "Runoff mapping" (unit vectors (cos lat cos lon, cos lat sin lon, sin lat), lon, lat * (pi / 180); d2 = (dx * dx + dy *
 *            dy) + dz * dz): ties to the smaller index.  It is the cell ogg_mask_seed_dev names, with the same d2 bits: the two
 *            searches share one definition of d2.  Invalid cells are no candidates.  A seed whose d2 is larger than seed_max_d2
 *            (+inf: off) is OFF THE GRID.
 *   order    before rule k, code[c] = 0 for every cell that no earlier rule took.  E_k: the cells that are wet, valid, uncoded and in
 *            box k.  If the seed cell is in E_k, its connected component inside E_k through the faces above gets code_k and rule[c]
 *            = k.  Otherwise the rule takes nothing, which is no error (a coarse or regional grid may have no Black Sea), and its
 *            status says why, the first of these that holds: OGG_BASIN_SEED_INVALID (5) the grid has no valid cell, so there is no
 *            seed cell (seed_cell -1, d2 +inf); OGG_BASIN_SEED_OFF_GRID (4); OGG_BASIN_SEED_LAND (1) the seed cell is not wet;
 *            OGG_BASIN_SEED_OUTSIDE (2) its centre is outside box k; OGG_BASIN_SEED_CODED (3) rule blocking_rule took it before.
 *            OGG_BASIN_TOOK (0): the rule took cells.
 *   outputs  code (ny, nx) uint8, 0 for land and for wet cells no rule took; rule (ny, nx) int16, -1 where code is 0; one record per
 *            rule; the counts.
 * Everything is an integer: no launch geometry or knob changes a bit.  Consecutive rules whose boxes are pairwise disjoint run as one
 * pass of at most OGG_BASIN_MAX_PASS_RULES rules; two boxes count as disjoint only when their latitude intervals or their longitude
 * arcs are separated by more than 1e-9 degrees.  OGG_BASIN_BATCH=0 gives one rule per pass; OGG_BASIN_TILE_ROWS (1 .. 64, default 32)
 * the rows of a labelling tile.
 * ---------------------------------------------------------------------------------------------------- */
#define OGG_BASIN_MAX_RULES 4096
#define OGG_BASIN_MAX_PASS_RULES 255
enum { OGG_BASIN_TOOK = 0, OGG_BASIN_SEED_LAND = 1, OGG_BASIN_SEED_OUTSIDE = 2, OGG_BASIN_SEED_CODED = 3, OGG_BASIN_SEED_OFF_GRID = 4,
       OGG_BASIN_SEED_INVALID = 5 };
typedef struct ogg_basin_params {
    long ny, nx;               /* model cells */
    int topology;              /* OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int n_rules;               /* K */
    double seed_max_d2;        /* squared chord beyond which a seed is off the grid; +inf: off */
} ogg_basin_params;
typedef struct ogg_basin_rule {
    int code;                  /* 1 .. 255 */
    int reserved;              /* not read */
    double seed_lon, seed_lat; /* degrees */
    double lon_w, lon_e;       /* 0 < lon_e - lon_w <= 360 */
    double lat_s, lat_n;
} ogg_basin_rule;
typedef struct ogg_basin_rule_record {
    long long seed_cell;       /* -1 when the grid has no valid cell */
    long long d2_bits;         /* the bits of the squared chord from the seed to the seed cell's centre */
    int status;                /* OGG_BASIN_TOOK ... OGG_BASIN_SEED_INVALID */
    int blocking_rule;         /* with OGG_BASIN_SEED_CODED the rule that took the seed cell, else -1 */
    long long cells;           /* cells taken */
} ogg_basin_rule_record;
typedef struct ogg_basin_counts {
    long long wet;             /* cells with a non-zero wet byte */
    long long coded;           /* cells some rule took */
    long long uncoded;         /* wet - coded */
    long long passes;          /* passes run */
} ogg_basin_counts;
long ogg_basin_workspace_bytes(const ogg_basin_params* p);   /* -1 on a bad *p */
/* the checks of *p and of the n_rules rules (HOST memory): OGG_EARG with the reason, before any device work */
int ogg_basin_check(const ogg_basin_params* p, const ogg_basin_rule* rules);
/* the passes the call would run (host only): pass q holds the rules pass_start[q] .. pass_start[q + 1] - 1; pass_start has room for
 * n_rules + 1 entries */
int ogg_basin_plan(const ogg_basin_params* p, const ogg_basin_rule* rules, int* pass_start, int* n_passes);
/* device pointers, on a stream, without a host round trip between the passes: rules in HOST memory (checked and planned there) and
 * rules_dev the same n_rules rules in device memory; x, y the supergrid points (2 ny + 1 rows of ld doubles); wet, code (ny * nx
 * bytes), rule (ny * nx int16), records (n_rules) and *counts in device memory. */
int ogg_basin_codes_dev(const ogg_basin_params* p, const ogg_basin_rule* rules, const ogg_basin_rule* rules_dev, const double* x,
                        const double* y, long ld, const unsigned char* wet, void* workspace, long workspace_bytes, unsigned char* code,
                        short* rule, ogg_basin_rule_record* records, ogg_basin_counts* counts, void* stream);
/* HOST pointers throughout, staged through device memory: x, y (2 ny + 1) x (2 nx + 1) */
int ogg_basin_codes(const ogg_basin_params* p, const ogg_basin_rule* rules, const double* x, const double* y, const unsigned char* wet,
                    unsigned char* code, short* rule, ogg_basin_rule_record* records, ogg_basin_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Sill depths (an addition: the reference has none).  The deepest connection of every model cell to a set of seed cells: the
 * widest-path ("bottleneck") depth over integer face weights, the regions of equal sill depth and the gate faces that limit them.  It
 * answers at what depth a marginal sea is connected to the open ocean on THIS grid, and at which face, without running the ocean mask
 * at one threshold after another.
 *   cells     c = j * nx + i of ny x nx model cells, ny * nx < 2^31; topology = OGG_MASK_PERIODIC | OGG_MASK_FOLD
 *   weights   int32, in quanta, positive down: wu[ny][nx + 1], wu[j][I] between cells (j, I - 1) and (j, I); wv[ny + 1][nx], wv[J][i]
 *             between cells (J - 1, i) and (J, i): the layout of the face topography's fields.  A weight is read as
 *             min(max(w, 0), 2^bits - 1), 1 <= bits <= OGG_SILL_MAX_BITS; every face that is read and whose weight that changes is
 *             counted in n_clamped
 *   passages  triples (a, b, w): every interior u face and every interior v face; with PERIODIC and nx > 2, (j, nx - 1) ~ (j, 0) with
 *             w = min(wu[j][0], wu[j][nx]) (with nx <= 2 the seam adds nothing); with FOLD, (ny - 1, i) ~ (ny - 1, nx - 1 - i) for
 *             i < nx - 1 - i with w = min(wv[ny][i], wv[ny][nx - 1 - i]).  wv[0][*] is never read; without the matching flag wu[*][0],
 *             wu[*][nx] and wv[ny][*] are never read either, nor is the middle face wv[ny][(nx - 1) / 2] of an odd fold row
 *   seeds     n_seeds >= 1 cell indices (int64, device memory); an index outside 0 .. ny * nx - 1 is ignored and counted in
 *             n_bad_seeds; duplicates are allowed
 *   b         int32 per cell: OGG_SILL_SEED at a seed; elsewhere the maximum over all paths of passages from the cell to any seed of
 *             the minimum w on the path; 0 when no path has a positive minimum (dry cells and cut-off water)
 *   region    int32 per cell: -1 where b = 0; the cell's own index at a seed; elsewhere the smallest cell index of the connected
 *             component of cells joined by a passage with b[a] == b[b] and w >= b[a]
 *   gates     one byte per face, gate_u[ny][nx + 1] and gate_v[ny + 1][nx]; for a passage (a, b, w), a the west / south / first-named
 *             cell: 1 if 0 < b[a] == w < b[b] (a is the enclosed side), 2 if 0 < b[b] == w < b[a] (b is), 0 otherwise.  The seam's code is
 *             written to columns 0 and nx alike; the fold's code at wv[ny][nx - 1 - i] has the roles swapped; faces that are never
 *             read hold 0.  Every region with 0 < b < OGG_SILL_SEED has at least one gate
 *   counts    OGG_SILL_COUNT_WORDS int64 words, in this order: rounds (= bits), n_clamped, n_bad_seeds, n_connected (cells with
 *             0 < b < OGG_SILL_SEED), n_cut_off (cells with b = 0 that have a passage of weight > 0), n_regions (cells with
 *             region[c] == c, seeds included), n_gate_faces (non-zero gate bytes: a seam gate counts in both of its columns, a fold
 *             gate at both of its faces)
 *   parameters  every entry takes the same six scalars first, by value: ny, nx, topology, bits, n_seeds (>= 1) and tile_rows.  No
 *             struct of this header, as for the face topography and the regional grids: the set of structs and their OGG_ABI_*
 *             codes stays what it was
 * b is decided bit by bit from the top, one labelling of the whole plane per bit with the ocean mask's union-find, so a call is
 * 5 * bits + 7 launches at most whatever a component's diameter, on the caller's stream without a host round trip.  Everything is an
 * integer: no tile height, launch shape or knob changes a bit.  tile_rows: the rows of a labelling tile, 1 .. 64, or 0 for
 * OGG_SILL_TILE_ROWS (default 32), read when the call is set up.
 * Connections go through faces only (right for a C-grid: a diagonal passage does not exist); a channel one cell wide counts as open;
 * b is relative to the chosen seeds.
 * ---------------------------------------------------------------------------------------------------- */
#define OGG_SILL_SEED (1 << 30)
#define OGG_SILL_MAX_BITS 30
#define OGG_SILL_COUNT_WORDS 7
long ogg_sill_workspace_bytes(long ny, long nx);   /* -1 unless ny, nx >= 1 and ny * nx < 2^31 */
/* the checks of the six scalars: OGG_EARG with the reason, before any device work */
int ogg_sill_check(long ny, long nx, int topology, int bits, int n_seeds, int tile_rows);
/* device pointers throughout, on a stream: wu (ny * (nx + 1) int32), wv ((ny + 1) * nx int32), seeds (n_seeds int64), b and region
 * (ny * nx int32 each), gate_u and gate_v (one byte per face), counts (OGG_SILL_COUNT_WORDS int64) */
int ogg_sill_depth_dev(long ny, long nx, int topology, int bits, int n_seeds, int tile_rows, const int* wu, const int* wv,
                       const long long* seeds, void* workspace, long workspace_bytes, int* b, int* region, unsigned char* gate_u,
                       unsigned char* gate_v, long long* counts, void* stream);
/* HOST pointers throughout, staged through device memory */
int ogg_sill_depth(long ny, long nx, int topology, int bits, int n_seeds, int tile_rows, const int* wu, const int* wv,
                   const long long* seeds, int* b, int* region, unsigned char* gate_u, unsigned char* gate_v, long long* counts);

/* ------------------------------------------------------------------------------------------------------
 * Processor layouts and mask tables (an addition: the reference has none).  For a decomposition of the model cells into px x py
 * blocks (MOM6's LAYOUT = px,py) the blocks that hold no ocean, which a model run leaves without a process (MASKTABLE =
 * mask_table.<n>.<px>x<py>), and for many candidate layouts at once the record from which one is chosen.
 *   cells    ny x nx model cells, one wet byte per cell (0: land), ny * nx < 2^31.  topology: OGG_MASK_PERIODIC | OGG_MASK_FOLD, the
 *            neighbour rule of csrc/ogg_cells.h: the fold partner of (ny-1, i) is (ny-1, nx-1-i).
 *   extents  ogg_layout_extent(npts, ndivs, begin, end) divides 0 .. npts-1 into ndivs blocks, 1 <= ndivs <= npts, by FMS's
 *            mpp_compute_extent restated in integers:
 *                isg = 0; ieg = npts-1
 *                sym = (ndivs odd and npts even) ? (ndivs < npts/2) : (ndivs%2 == npts%2)
 *                is = 0; imax = ieg; ndmax = ndivs
 *                for nd = 0 .. ndivs-1:
 *                    if nd < (ndivs-1)/2 + 1:
 *                        ie = is + ceil((imax-is+1) / (ndmax-nd)) - 1          # ceil(a/d) = (a+d-1)/d in integers
 *                        m = ndivs-1-nd
 *                        if m > nd and sym:
 *                            begin[m] = max(isg+ieg-ie, ie+1); end[m] = max(isg+ieg-is, ie+1)
 *                            imax = begin[m]-1; ndmax = ndmax-1
 *                    else if sym: is = begin[nd]; ie = end[nd]
 *                    else:        ie = is + ceil((imax-is+1) / (ndmax-nd)) - 1
 *                    begin[nd] = is; end[nd] = ie; is = ie+1
 *            The result is a partition into non-empty consecutive blocks (end[nd] + 1 = begin[nd + 1]), mirror-symmetric whenever
 *            sym holds, with block sizes that differ by at most 2.  One __host__ __device__ body serves this function and the sweep
 *            kernel; it keeps the begins alone and reads end[nd] as begin[nd + 1] - 1, which the partition allows.  FMS forms the
 *            quotient in single precision; for npts < 1e7 the integer ceiling is the same number, since the smallest fraction 1/d
 *            exceeds the quotient's rounding error.  CAVEAT: the rule is written from FMS's rule as understood here; no copy of FMS or
 *            FRE-NCtools was on hand to verify it against.  Explicit extents (ogg_layout_blocks_dev) therefore tie a table to a
 *            model's own decomposition, whatever its rule.
 *   layout   (px, py) with px <= nx, py <= ny, both <= OGG_LAYOUT_MAX_DIV: the x extents from (nx, px), the y extents from (ny, py).
 *            Block (a, b) holds columns bx[a] .. ex[a] and rows by[b] .. ey[b]; wet(a, b) is the number of wet cells in it.
 *   halo     h >= 0.  The neighbourhood of block (a, b) is the SET of cells reached from (j, i) with by-h <= j <= ey+h and
 *            bx-h <= i <= ex+h: a column outside 0 .. nx-1 wraps modulo nx on a periodic grid and is dropped otherwise; a row below 0
 *            is dropped; a row ny + k maps on a folded grid to row ny-1-k at column nx-1-i', i' the column after wrapping, and is
 *            dropped when k >= ny or without a fold.  nbr(a, b) is the number of wet cells in that set (each cell once); the kernels
 *            get it from a few rectangles of the summed-area table, the overlap of the rows past the fold with the rows below it
 *            taken off.
 *   masked   a block is MASKED when nbr(a, b) = 0; with h = 0, when all its own cells are land.
 *   record   of a layout: blocks = px * py; masked; pes = blocks - masked; max_block_cells = largest x size * largest y size;
 *            max_block_edge = largest x size + largest y size; min_block_size = the smallest size in either direction; max_wet = the
 *            largest wet(a, b); masked_cells = the cells in masked blocks; wet_total = the wet cells of the grid; status:
 *            OGG_LAYOUT_TOO_FINE: px > nx, py > ny, either above OGG_LAYOUT_MAX_DIV (or below 1, which ogg_layout_check refuses on
 *            the host): every other field is 0.  OGG_LAYOUT_FOLD_ASYMMETRIC: a folded grid whose x extents are not mirror images,
 *            bx[a] + ex[px-1-a] != nx-1 for some a; FMS refuses such a decomposition of a tripolar grid.  The other fields are
 *            filled all the same.
 *   ranking  (host code over the records, layout.py) for a target of T processes: among the records with status == 0 and pes == T
 *            the smallest key (max_block_cells, max_block_edge, blocks, px); the cost of a step goes with the block size, not the wet
 *            count.
 *   table    of one layout: the masked blocks in ascending (b, a), written 1-based as "a+1,b+1".
 * Everything is an integer: the result is bit-identical for any launch geometry (OGG_LAYOUT_TILE_ROWS, the rows of a tile of the
 * table's column pass, 4 .. 1024, default 32; OGG_LAYOUT_GRID, the workgroups of the sweep, 0: one per candidate) and any rank
 * count on the gathered wet set.
 * ---------------------------------------------------------------------------------------------------- */
#define OGG_LAYOUT_MAX_DIV 4096
#define OGG_LAYOUT_MAX_CANDIDATES (1 << 20)
enum { OGG_LAYOUT_TOO_FINE = 1, OGG_LAYOUT_FOLD_ASYMMETRIC = 2 };
/* ny * nx < 2^31 */
typedef struct ogg_layout_params {
    long ny, nx;               /* model cells */
    int topology;              /* OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int halo;                  /* h >= 0 */
} ogg_layout_params;
typedef struct ogg_layout_candidate {
    int px, py;
} ogg_layout_candidate;
typedef struct ogg_layout_record {
    int blocks, masked, pes;
    int max_block_cells, max_block_edge, min_block_size;
    int max_wet, masked_cells, wet_total;
    int status;                /* OGG_LAYOUT_TOO_FINE | OGG_LAYOUT_FOLD_ASYMMETRIC */
} ogg_layout_record;
/* the extents of the rule above (host only, no device work): begin and end have room for ndivs entries; end may be NULL */
int ogg_layout_extent(long npts, long ndivs, int* begin, int* end);
/* the checks of *p (sizes, topology, halo) and of the n candidates (HOST memory, NULL with n = 0; every px, py >= 1 and n <=
 * OGG_LAYOUT_MAX_CANDIDATES): OGG_EARG with the reason, before any device work.  A candidate finer than the grid is no error: its
 * record says OGG_LAYOUT_TOO_FINE. */
int ogg_layout_check(const ogg_layout_params* p, const ogg_layout_candidate* candidates, long n);
long ogg_layout_workspace_bytes(const ogg_layout_params* p);   /* -1 on a bad *p */
/* the summed-area table of wet (device memory, ny * nx bytes) into the workspace: (ny + 1) x (nx + 1) int32 counts */
int ogg_layout_table_dev(const ogg_layout_params* p, const unsigned char* wet, void* workspace, long workspace_bytes, void* stream);
/* after ogg_layout_table_dev on the same workspace: the records (device memory) of the n candidates (device memory, n <=
 * OGG_LAYOUT_MAX_CANDIDATES; a px or py below 1 counts as OGG_LAYOUT_TOO_FINE), one workgroup per candidate */
int ogg_layout_sweep_dev(const ogg_layout_params* p, const ogg_layout_candidate* candidates, long n, const void* workspace,
                         long workspace_bytes, ogg_layout_record* records, void* stream);
/* after ogg_layout_table_dev on the same workspace: wet(a, b) and nbr(a, b) of every block of one layout (device memory, py x px
 * int32 each).  xbegin, ybegin: HOST memory, NULL for the rule's extents, else the px (py) first columns (rows) of the blocks,
 * strictly increasing from 0 and below nx (ny); px, py <= OGG_LAYOUT_MAX_DIV.  Waits for the stream: the block begins are copied to the
 * device from memory of the call's own, before the one launch that reads them. */
int ogg_layout_blocks_dev(const ogg_layout_params* p, int px, int py, const int* xbegin, const int* ybegin, void* workspace,
                          long workspace_bytes, int* block_wet, int* block_nbr, void* stream);
/* HOST pointers throughout, staged through device memory: the table, then the records of the n candidates (records NULL with n = 0),
 * then, unless block_wet and block_nbr are NULL, the blocks of the layout (px, py) with xbegin, ybegin as above */
int ogg_layouts(const ogg_layout_params* p, const unsigned char* wet, const ogg_layout_candidate* candidates, long n,
                ogg_layout_record* records, int px, int py, const int* xbegin, const int* ybegin, int* block_wet, int* block_nbr);

/* ------------------------------------------------------------------------------------------------------
 * Point location (an addition: the reference has none).  The inverse of every other analysis here: given a longitude and a latitude,
 * the model cell that holds the point, where in the cell it lies, and a model field there (moorings, tide gauges, profiles, section
 * end points, mask and basin seeds, the depth at a river mouth).  The definition needs no walk over the grid: every cell has a key
 * for every point, and the answer is the best key.
 *   cells    those of the cell-set analyses: ny x nx model cells, c = j * nx + i; the corners of cell (j, i) are the supergrid points
 *            (2j, 2i) SW = a, (2j, 2i+2) SE = b, (2j+2, 2i+2) NE = c, (2j+2, 2i) NW = d.  Edges are GREAT CIRCLES between the corners'
 *            unit vectors, the rule of the cubed-sphere exchange grid (not the lat-lon polygons of the lat-lon exchange grid).
 *            ny * nx * OGG_LOCATE_MAX_TOUCH < 2^31 (the index's entries are counted in 32 bits), and fewer than 2^31 queries.
 *   corner table  cu[(ny+1)(nx+1)][3]: unit(x, y) of csrc/ogg_sphere.h (the one shared implementation, "Runoff mapping") of every
 *            corner (J, I).  With OGG_MASK_PERIODIC corner column nx takes the bits of column 0 of its row; with OGG_MASK_FOLD the
 *            top-row corner I takes the bits of the smallest I among its copies, I and nx - I after the periodic reduction.  (The
 *            table is formed from the canonical copy's x and y.)  A shared corner is therefore one set of bits in every cell that has
 *            it.  cu and the queries' vectors qu[n][3] (the same unit()) are device outputs.
 *   edge measure  n(a,b) = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx) and T(p; a,b) = (px*nx + py*ny) + pz*nz, every product
 *            rounded, no FMA.  In this order T(p; b,a) = -T(p; a,b) EXACTLY: what one cell sees across a face, its neighbour sees
 *            negated, bit for bit.  S = T(p; a,b), E = T(p; b,c), N = T(p; c,d), W = T(p; d,a).
 *   orientation  O = ((a+b)+(c+d)) . ((n_S+n_E)+(n_N+n_W)), the sums by component, the dot product in T's order; sigma = +1 when
 *            O > 0, -1 when O < 0.  A cell whose O is 0 or not finite holds no point (a NaN corner, a fully collapsed cell).
 *   box      L2 the largest dist2 ("Runoff mapping") between two of the cell's corners, pad = 0.25 * L2 + 2^-40; p is in the cell's
 *            box when every component of p lies within [min over the corners - pad, max over the corners + pad].  The box is part of
 *            the definition: it bounds what sliver and half-collapsed cells can claim, and it is what the search index registers.
 *   key      m_c(p) = min(sigma S, sigma E, sigma N, sigma W).  Cell c is a candidate of p when p is in its box and
 *            m_c >= -OGG_LOCATE_TOL.
 *   answer   the candidate with the largest m_c, ties to the smaller c.  No candidate, or a query vector with a component that is
 *            not finite (a longitude or latitude that is not finite): cell = -1 and s = t = m = NaN.
 *   position s = sigma W / (sigma W + sigma E) and t = sigma S / (sigma S + sigma N), each clamped to [0, 1], and 0.5 when the
 *            denominator is not > 0.  An edge whose two corners have the same bits has a zero normal; its measure is replaced
 *            through the opposite edge: N collapsed: sigma N := sigma (c . n_S) - sigma S; S collapsed: sigma S := sigma (a . n_N) -
 *            sigma N; E collapsed: sigma E := sigma (b . n_W) - sigma W; W collapsed: sigma W := sigma (a . n_E) - sigma E (the dot
 *            products in T's order); both of a pair collapsed: 0.5.  (s, t) is exact on parallelograms in the small-cell limit, s = 0
 *            on the W edge and 1 on the E edge; it is the inverse of no particular map.
 *   sampling a field on the model cells, f[r][j][i], r < nrec, OGG_REMAP_FLOAT32 or OGG_REMAP_FLOAT64; a value is MISSING by the
 *            remap's rule (NaN, or one of up to two fill values compared in the field's own type); an optional wet byte per cell.  A
 *            cell is USED when it exists, is wet and its value is not missing.
 *            OGG_LOCATE_CELL: the value of cell c.  OGG_LOCATE_BILINEAR: index-space bilinear between the four nearest centres:
 *            fx = |s - 0.5|, fy = |t - 0.5|; C00 = c; C10 c's E neighbour when s >= 0.5, else its W neighbour; C01 c's N neighbour
 *            when t >= 0.5, else its S neighbour; C11 the neighbour of C10 in that same y direction (none when C10 is none);
 *            neighbours are face_neighbours of csrc/ogg_cells.h, so across the fold this is "x first, then N".  Weights in the order
 *            C00, C10, C01, C11: (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.  Over the used cells, in that order, W = sum of w and
 *            S = sum of (w * f), in fp64 from 0; the value is S / W.
 *   flags    one byte per (record, point): 0 no cell; 1 all four used (CELL: the cell is used); 2 fewer than four used; 3 none
 *            used, or the containing cell is dry, or W is not > 0.  With flag 0 or 3 the value is OGG_REMAP_FILL.
 * Every output of a query is a function of cu, the topology flags and that query's own qu: no index, cube count, knob
 * (OGG_LOCATE_CUBES: cubes per axis of the index, 0: from the cell count; OGG_LOCATE_BRUTE=1: every cell that can hold a point is
 * tested for every query), query order or rank count changes a bit.
 * OGG_LOCATE_TOL: near a vertex the four rounded half-plane tests of the cells around it can disagree in a pinwheel, so that no cell
 * has m >= 0; on jittered lat-lon meshes of 0.01 to 3 degrees the worst best-m over corners, edge midpoints and their 1-ulp
 * neighbours is about -1e-17 (tests/test_locate_cpu.py measures it).  2^-50 covers that a hundred times over and stays below 4e-6
 * of a cell's own T scale for cells down to 100 m across; grids with cells of a few metres are outside its design.
 * Output layout: cell int32, s, t, m fp64, one per query; values (nrec, n) fp64 and flags (nrec, n) bytes.
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_LOCATE_CELL = 0, OGG_LOCATE_BILINEAR = 1 };
#define OGG_LOCATE_TOL 8.8817841970012523e-16   /* 2^-50 */
#define OGG_LOCATE_MAX_CUBES 128   /* the largest OGG_LOCATE_CUBES: cubes per axis of the search index */
#define OGG_LOCATE_MAX_TOUCH 27    /* a cell whose box touches more cubes than this is on the large-cells list */
typedef struct ogg_locate_params {
    long ny, nx;               /* model cells */
    long n;                    /* queries (>= 0) */
    long nrec;                 /* records of the sampled field (0: nothing is sampled) */
    int topology;              /* OGG_MASK_PERIODIC | OGG_MASK_FOLD */
    int mode;                  /* OGG_LOCATE_CELL / OGG_LOCATE_BILINEAR */
    int dtype;                 /* OGG_REMAP_FLOAT32 / OGG_REMAP_FLOAT64 */
    int n_fill;                /* 0 .. 2 fill values */
    double fill[2];
} ogg_locate_params;
typedef struct ogg_locate_counts {
    long long located;         /* queries with a cell (search step) */
    long long outside;         /* finite queries without a candidate (search step) */
    long long invalid;         /* queries with a coordinate that is not finite (search step) */
    long long large_cells;     /* cells on the large-cells list; with OGG_LOCATE_BRUTE every cell that can hold a point (index step) */
    long long cubes;           /* cubes per axis of the index, 0 for brute force (index step) */
    long long tests;           /* (query, cell) box tests (search step) */
    long long flag0, flag1, flag2, flag3;   /* (record, point) pairs by flag (sample step) */
} ogg_locate_counts;
long ogg_locate_workspace_bytes(const ogg_locate_params* p);   /* of the sets, index and search steps, -1 on a bad *p */
/* the checks of *p (sizes, topology, mode, dtype, fills): OGG_EARG with the reason, before any device work */
int ogg_locate_check(const ogg_locate_params* p);
/* sets step, device pointers, on a stream: x, y the supergrid points (2 ny + 1 rows of ld doubles); cu the corner table
 * ((ny + 1) * (nx + 1) * 3 doubles); the per-cell records (sigma times the four normals, the box) go into the workspace.  *counts
 * (device memory) is zeroed. */
int ogg_locate_sets_dev(const ogg_locate_params* p, const double* x, const double* y, long ld, void* workspace, long workspace_bytes,
                        double* cu, ogg_locate_counts* counts, void* stream);
/* index step, after the sets step on the same workspace: every cell that can hold a point registered in every cube its box touches, or
 * on the large-cells list; large_cells and cubes into *counts */
int ogg_locate_index_dev(const ogg_locate_params* p, void* workspace, long workspace_bytes, ogg_locate_counts* counts, void* stream);
/* search step, after the index step on the same workspace: lon, lat (n doubles each, degrees) -> qu (3 n doubles), cell, s, t, m as
 * above; located, outside, invalid and tests into *counts, from zero */
int ogg_locate_search_dev(const ogg_locate_params* p, const double* cu, const double* lon, const double* lat, void* workspace,
                          long workspace_bytes, double* qu, int* cell, double* s, double* t, double* m, ogg_locate_counts* counts,
                          void* stream);
/* sample step (nrec >= 1, no workspace): f (nrec, ny, nx) of p->dtype, wet one byte per cell or NULL, cell, s, t of n queries ->
 * values (nrec, n) and flags (nrec, n); flag0 .. flag3 into *counts, from zero */
int ogg_locate_sample_dev(const ogg_locate_params* p, const int* cell, const double* s, const double* t, const void* f,
                          const unsigned char* wet, double* values, unsigned char* flags, ogg_locate_counts* counts, void* stream);
/* HOST pointers throughout, staged through device memory: the three steps on the supergrid x, y ((2 ny + 1) x (2 nx + 1)); cu and qu
 * may be NULL */
int ogg_locate(const ogg_locate_params* p, const double* x, const double* y, const double* lon, const double* lat, int* cell, double* s,
               double* t, double* m, double* cu, double* qu, ogg_locate_counts* counts);
/* HOST pointers throughout: the sample step on located points; *counts gets flag0 .. flag3 and keeps its other fields */
int ogg_locate_sample(const ogg_locate_params* p, const int* cell, const double* s, const double* t, const void* f,
                      const unsigned char* wet, double* values, unsigned char* flags, ogg_locate_counts* counts);

/* ------------------------------------------------------------------------------------------------------
 * Regional grids (an addition: the reference makes the global tripolar grid only).  A patch of sphere with its own equator through
 * the domain: a lat-lon or a Mercator lattice in a ROTATED frame (lam', phi') whose point (0, 0) is the domain centre (lon_c, lat_c)
 * and whose x axis at the centre is turned by ``tilt`` degrees counter-clockwise from east.  Neither periodic nor pole-holding.
 *   rotation  with p' = (cos phi' cos lam', cos phi' sin lam', sin phi') the geographic unit vector relative to the centre meridian
 *            is p = Ry(-lat_c) Rx(tilt) p' = cos phi' (cos lam' q1 + sin lam' q2) + sin phi' q3 with, cl, sl the cosine and sine of
 *            lat_c and ct, st those of tilt,  q1 = (cl, 0, sl),  q2 = (-sl st, ct, cl st),  q3 = (-sl ct, -st, cl ct).
 *            a_i = cos lam'_i q1 + sin lam'_i q2 and e_i = -sin lam'_i q1 + cos lam'_i q2 (the grid's x direction, the same on every
 *            row) belong to a column, cos phi'_j and sin phi'_j to a row: p = cos phi'_j a_i + sin phi'_j q3.
 *   points   x = lon_c + atan2(p_y, p_x) in degrees: continuous over the domain whatever lon_c is, no jump at +-180, stated on
 *            lon_c's own turn.  y = atan2(p_z, sqrt(p_x^2 + p_y^2)) in degrees (no asin: conditioned next to the poles).
 *   lattice  nx by ny SUPERGRID cells, both even (nx/2 by ny/2 model cells); point (j, i), j = 0 .. ny, i = 0 .. nx, has
 *            lam'_i = (i - nx/2) delta, delta degrees per supergrid step, and
 *              OGG_REGIONAL_LATLON    phi'_j = (j - ny/2) delta: generate_latlon_grid (OGG:832-846), rotated;
 *              OGG_REGIONAL_MERCATOR  phi'_j = atan(sinh(t_j)), t_j = (j - ny/2) delta pi/180: the lattice of phi_mercator (OGG:298-301)
 *                                     with Ni = 360/delta, rotated: an oblique Mercator with isotropic cells.  cos phi' = 1/cosh(t)
 *                                     and sin phi' = tanh(t), not taken from phi'.
 *   metrics  the MIDAS lat-lon formulas (OGG:687-716 with latlon_areafix) stated in the rotated frame, where they are EXACT: a
 *            rotation is an isometry, so they hold on the sphere.
 *              dx(j, i)   = Re cos phi'_j delta pi/180                              (ny+1) x nx
 *              dy(j, i)   = Re (phi'_{j+1} - phi'_j)                                ny x (nx+1)
 *              area(j, i) = Re^2 delta pi/180 (sin phi'_{j+1} - sin phi'_j)         ny x nx
 *            The device forms the two differences without cancellation: lat-lon rows have phi'_{j+1} - phi'_j = delta pi/180 and
 *            sin phi'_{j+1} - sin phi'_j = 2 cos(phi'_{j+1/2}) sin(delta pi/360); Mercator rows, with h = delta pi/360 and t_m =
 *            t_j + h, have phi'_{j+1} - phi'_j = 2 atan(sinh h / cosh t_m) (phi' = 2 atan(tanh(t/2)) and the addition theorem of the
 *            tangent) and sin phi'_{j+1} - sin phi'_j = sinh(2 h) / (cosh t_j cosh t_{j+1}).
 *   identity with lat_c = 0 and tilt = 0 the rotation is the identity and the grid IS the lattice shifted by lon_c: the device writes
 *            x = lon_c + lam'_i, y = phi'_j (Mercator: atan(sinh(t_j)) in degrees) and angle_dx = 0 as such, which is what the statements
 *            above give in exact arithmetic; no arctangent of a sine and a cosine comes between.
 *   angle_dx(j, i) = atan2(e . n, e . ee) in degrees, (ny+1) x (nx+1), ee and n the geographic east and north at p.  This is the
 *            ANALYTIC angle of the grid's x direction, not the reference's finite difference angle_x (OGG:719-729) of the mesh; the
 *            two agree to O(delta^2).  (a_i, e_i, q3) is a right-handed orthonormal frame and e is perpendicular to p, which gives
 *            with h = sqrt(p_x^2 + p_y^2):  e . n = e_z / h  and  e . ee = (cos phi'_j q3_z - sin phi'_j a_z) / h,  so
 *            angle_dx = atan2(e_z(i), cos phi'_j q3_z - sin phi'_j a_z(i)): no product of small differences.
 *   refused  with OGG_EARG and the reason, before any device work: nx or ny odd or below 2 (or above 2^22); delta, Re not positive;
 *            an argument that is not finite, or lon_c or tilt above 1e6 in magnitude; |lam'| >= 180 at the edge; |phi'| > 89 at the edge; |lat_c| > 90; a domain whose rotated
 *            rectangle (widened by 1e-9 degrees) holds a geographic pole -- a point of the mesh could sit on it, a cell could have it
 *            as a corner, and the analyses treat such cells as special cases.
 * Every value is a function of (j, i) and the parameters alone: no launch geometry and no split into bands changes a bit.
 * Workspace: the column table (a_i, e_z(i)) and the row table (cos phi', sin phi', dx, dy, area per row), a few doubles per row and
 * column, filled by ogg_regional_tables_dev and read by every band of the same parameters.
 * Parameters: every entry takes the same nine scalars first, by value (no struct: the table of OGG_ABI_* size codes is unchanged):
 *   nx, ny        supergrid cells, both even and >= 2
 *   lon_c, lat_c  the domain centre, degrees;  tilt  degrees counter-clockwise from east
 *   delta         degrees per supergrid step in the rotated frame;  Re  sphere radius, metres
 *   kind          OGG_REGIONAL_LATLON / OGG_REGIONAL_MERCATOR;  metrics  0: x and y only, 1: all six fields
 * ---------------------------------------------------------------------------------------------------- */
enum { OGG_REGIONAL_LATLON = 0, OGG_REGIONAL_MERCATOR = 1 };
#define OGG_REGIONAL_MAX_CELLS 4194304   /* the largest nx, ny: 2^22 */
/* the checks of the parameters listed above: OGG_EARG with the reason, no device work */
int ogg_regional_check(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics);
/* -1 on bad parameters */
long ogg_regional_workspace_bytes(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics);
/* the two tables into the workspace (device memory): one small launch */
int ogg_regional_tables_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics,
                            void* workspace, long workspace_bytes, void* stream);
/* after ogg_regional_tables_dev on the same workspace with the same parameters: the point rows j0 .. j0 + nrows - 1 (0 <= j0, j0 +
 * nrows <= ny + 1) and the cell rows among them (j < ny) of the grid, one launch.  Every array begins at the band's first row:
 *   x, y, angle_dx   nrows x (nx+1)
 *   dx               nrows x nx
 *   dy               (cell rows of the band) x (nx+1);  area  (cell rows of the band) x nx
 * With metrics == 0 only x and y are written and the other four may be NULL. */
int ogg_regional_band_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics,
                          long j0, long nrows, const void* workspace, long workspace_bytes, double* x, double* y, double* dx, double* dy,
                          double* area, double* angle_dx, void* stream);
/* HOST pointers, staged through device memory: the whole grid, x, y, angle_dx (ny+1) x (nx+1), dx (ny+1) x nx, dy ny x (nx+1), area
 * ny x nx; with metrics == 0 only x and y */
int ogg_regional_grid(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int kind, int metrics,
                      double* x, double* y, double* dx, double* dy, double* area, double* angle_dx);

/* ------------------------------------------------------------------------------------------------------
 * Stereographic regional grids (an addition, as "Regional grids"): the oblique stereographic projection about the domain centre, the
 * conformal lattice for pan-Arctic and circum-Antarctic domains and every shelf domain that reaches a pole.  The domain MAY hold a
 * geographic pole -- as a mesh point (the centre of a grid with lat_c = +-90 only), as a cell corner or inside a cell.  Not periodic,
 * at most a hemisphere.
 *   frame    the rotation triple of "Regional grids", relative to the centre meridian: with cl, sl of lat_c and ct, st of tilt
 *              q1 = (cl, 0, sl) the centre,  q2 = (-sl st, ct, cl st) the grid's x direction at the centre,  q3 = (-sl ct, -st, cl ct).
 *   plane    d = delta pi/180;  X_i = (i - nx/2) d,  Y_j = (j - ny/2) d  in units of Re: delta is degrees per supergrid step AT THE
 *            CENTRE, where the scale is true.  nx by ny supergrid cells, both even; points j = 0 .. ny, i = 0 .. nx.
 *   points   rho2 = X^2 + Y^2,  m = 1 + rho2/4,  p = (X q2 + Y q3 + (1 - rho2/4) q1) / m: a unit vector, no sine or cosine per point.
 *            x = lon_c + atan2(p_y, p_x) in degrees,  y = atan2(p_z, sqrt(p_x^2 + p_y^2)) in degrees, as for the other kinds.
 *   angle_dx the grid's x direction at p is parallel to t = q2 - (X/2) (q1 + p);  angle_dx = atan2(t_z, p_x t_y - p_y t_x) in degrees:
 *            analytic, as for the other kinds.  (m t = (1 + (Y^2 - X^2)/4) q2 - X q1 - (X Y/2) q3, and m^2 (p_x t_y - p_y t_x) is m
 *            times the z component of (1 + (X^2 - Y^2)/4) q3 - Y q1 - (X Y/2) q2: the device evaluates these two.)
 *   metrics  exact on the sphere; the physical length is Re times the plane length over m, and the grid lines are circles:
 *              dx(j, i)   = Re (4/a) atan(a d / (a^2 + X_i X_{i+1})),  a = sqrt(4 + Y_j^2)                     (ny+1) x nx
 *              dy(j, i)   = Re (4/b) atan(b d / (b^2 + Y_j Y_{j+1})),  b = sqrt(4 + X_i^2)                     ny x (nx+1)
 *              area(j, i) = Re^2 [(Y_{j+1} dxh(j+1, i) - Y_j dxh(j, i)) + (X_{i+1} dyh(j, i+1) - X_i dyh(j, i))] / 2   ny x nx
 *            with dxh = dx/Re, dyh = dy/Re: Gauss-Bonnet for four circular edges of geodesic curvature Y_j/2, -X_{i+1}/2, -Y_{j+1}/2,
 *            X_i/2 that meet at right angles.  The area is a difference of neighbouring terms and loses eps |Y| / d when evaluated
 *            literally; the device takes each difference apart so that none is left (csrc/ogg_regional_stereo.hip, "area").
 *            The whole domain, A = (nx/2) d, B = (ny/2) d, a = sqrt(4 + B^2), b = sqrt(4 + A^2), has the area
 *              8 Re^2 [(B/a) atan(A/a) + (A/b) atan(B/b)],  which tends to 4 pi Re^2 as the domain grows.
 *   poles    x has its jump of 360 degrees on the meridian opposite lon_c BEYOND a pole of the domain: the cells across that half
 *            meridian have corners a turn apart (the file-based analyses unwrap each cell's corners on their own turn).  With lat_c =
 *            +-90 EXACTLY the centre point is the pole, p_x = p_y = 0, and has by definition x = lon_c, y = lat_c, angle_dx = tilt,
 *            the limit along the meridian lon_c: no bit depends on the sign of a zero.  (The device takes cl = 0 there, not the cosine
 *            of pi/2 rounded.)
 *   refused  with OGG_EARG and the reason, before any device work: nx or ny odd, below 2 or above 2^22; delta or Re not positive; an
 *            argument that is not finite, lon_c or tilt above 1e6 in magnitude, |lat_c| > 90; a corner farther than 90 degrees from the
 *            centre, d sqrt((nx/2)^2 + (ny/2)^2) > 2; a mesh point other than that exact centre within 1e-9 degrees of a pole (the
 *            north pole lies at 2 (q2_z, q3_z) / (1 + q1_z) in the plane, the south pole at -2 (q2_z, q3_z) / (1 - q1_z)).
 * Every value is a function of (j, i) and the parameters alone: no launch geometry and no split into bands changes a bit.
 * The entries take the scalars of "Regional grids" without kind: nx, ny, lon_c, lat_c, tilt, delta, Re, metrics; the workspace holds a
 * column and a row table, filled by ogg_regional_stereo_tables_dev and read by every band of the same parameters; the arrays of
 * ogg_regional_stereo_band_dev begin at the band's first row and have the extents of ogg_regional_band_dev.
 * ---------------------------------------------------------------------------------------------------- */
int ogg_regional_stereo_check(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics);
/* -1 on bad parameters */
long ogg_regional_stereo_workspace_bytes(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics);
int ogg_regional_stereo_tables_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics,
                                   void* workspace, long workspace_bytes, void* stream);
int ogg_regional_stereo_band_dev(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics, long j0,
                                 long nrows, const void* workspace, long workspace_bytes, double* x, double* y, double* dx, double* dy,
                                 double* area, double* angle_dx, void* stream);
/* HOST pointers, staged through device memory: the whole grid; with metrics == 0 only x and y */
int ogg_regional_stereo_grid(long nx, long ny, double lon_c, double lat_c, double tilt, double delta, double Re, int metrics, double* x,
                             double* y, double* dx, double* dy, double* area, double* angle_dx);

/* per-launch timing of the dominant kernels with HIP events on the given stream: start/stop bracket */
int ogg_event_create(void** ev);
int ogg_event_destroy(void* ev);
int ogg_event_record(void* ev, void* stream);
int ogg_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);
int ogg_stream_synchronize(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OGG_HIP_H */
