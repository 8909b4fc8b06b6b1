"""ctypes binding of libogg_hip.so (the C ABI declared in include/ogg_hip.h).

There is no fallback: if the shared library cannot be loaded, or a call returns an error code, an exception is
raised.  Error codes map to the reference's own exception texts where it has them (OGG:204, OGG:547, OGG:722).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# OGG_LIB_PATH: another build of the same library (A/B timing of two builds on one box, scripts/ab_libs.sh); it must export the same ABI
LIB_PATH = os.environ.get("OGG_LIB_PATH") or os.path.join(_HERE, "csrc", "libogg_hip.so")

OGG_OK, OGG_EORDER, OGG_ESHAPE, OGG_EHIP, OGG_ENOMEM, OGG_EARG = 0, 1, 2, 3, 4, 5
DP_ARC_LITERAL, DP_ARC_CHORD = 0, 1   # OGG_DP_ARC_* of include/ogg_hip.h
SYM_DEFAULT, SYM_MIRROR, SYM_NONE = 0, 1, 2   # OGG_SYM_* of include/ogg_hip.h

# OGG_MATH_* of include/ogg_hip.h: the codes of ogg_math_eval_dev (test-only)
MATH = {"div_pi180": 0, "rcp_c3": 1, "rsqrt_c3": 2, "atan_series14": 3, "atan_series17": 4, "atan_cap": 5, "atan2_angle": 6,
        "wave_prev": 7, "wave_next": 8, "wave_prev_tail": 9, "wave_next_tail": 10, "xcd_contiguous": 11, "lib_atan": 12, "atan_lib": 13, "wave_next_int": 14,
        "sin_tiny": 32, "asin_tiny": 33, "cos_cap": 34, "hom_arc": 35, "hom_tan": 36, "lib_sin": 37, "lib_asin": 38, "lib_cos": 39}

c_long, c_int, c_double, c_void_p, c_longlong = ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_longlong
_dp = ctypes.POINTER(ctypes.c_double)
_llp = ctypes.POINTER(ctypes.c_longlong)

class LatlonBand(ctypes.Structure):
    """ogg_latlon_band of include/ogg_hip.h"""
    _fields_ = [("axis_kind", c_int), ("a0", c_double), ("len", c_double), ("denom", c_double), ("y0", c_longlong),
                ("lat1d", c_void_p), ("k0", c_long), ("n_pt_rows", c_long), ("n_cell_rows", c_long), ("x", c_void_p),
                ("y", c_void_p), ("dx", c_void_p), ("dy", c_void_p), ("area", c_void_p), ("angle", c_void_p)]


class BipolarBand(ctypes.Structure):
    """ogg_bipolar_band of include/ogg_hip.h"""
    _fields_ = [("Ni", c_long), ("Nj", c_long), ("lat0_bp", c_double), ("lon_bp", c_double), ("rp", c_double), ("Re", c_double),
                ("order", c_int), ("symmetry", c_int), ("j0", c_long), ("n_pt_rows", c_long), ("n_cell_rows", c_long), ("x", c_void_p),
                ("y", c_void_p), ("angle", c_void_p), ("dx", c_void_p), ("dy", c_void_p), ("area", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_long)]


class DpoleBand(ctypes.Structure):
    """ogg_dpole_band of include/ogg_hip.h"""
    _fields_ = [("Ni", c_long), ("Nj", c_long), ("lon0", c_double), ("lat0", c_double), ("lon_dp", c_double), ("r_dp", c_double),
                ("Re", c_double), ("order", c_int), ("arc_form", c_int), ("j0", c_long), ("n_pt_rows", c_long), ("n_cell_rows", c_long),
                ("x", c_void_p), ("y", c_void_p), ("angle", c_void_p), ("dx", c_void_p), ("dy", c_void_p), ("area", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_long), ("symmetry", c_int)]


class QualityBand(ctypes.Structure):
    """ogg_quality_band of include/ogg_hip.h"""
    _fields_ = [("nx", c_long), ("j0", c_long), ("n_pt_rows", c_long), ("n_cell_rows", c_long)] + \
        [(f, c_void_p) for f in ("x", "y", "dx", "dy", "area", "x_next", "y_next", "dx_next", "dy_next", "x_seam", "y_seam")] + \
        [("Re", c_double), ("metrics", c_int)]


QUALITY_N_EXTREMA, QUALITY_N_COUNTS, QUALITY_N_BINS = 12, 15, 7   # OGG_Q_N_EXTREMA, OGG_Q_N_COUNTS, OGG_QUALITY_N_BINS
QUALITY_EXTREMA = ("dx_min", "dx_max", "dy_min", "dy_max", "area_min", "area_max", "aspect_max", "delta_max", "rx_max", "ry_max",
                   "ry_next_max", "seam_max")   # OGG_Q_DX_MIN ... OGG_Q_SEAM_MAX
QUALITY_COUNTS = ("n_dx", "n_dx_degenerate", "n_dy", "n_dy_degenerate", "n_area", "n_area_zero", "n_corners", "n_corner_degenerate") + \
    tuple("hist%d" % k for k in range(QUALITY_N_BINS))   # OGG_Q_N_DX ... OGG_Q_HIST + 6
QUALITY_DEGENERATE_M = 1.0e-3          # OGG_QUALITY_DEGENERATE_M
QUALITY_BIN_EDGES_DEG = (1.0e-6, 1.0e-3, 0.1, 1.0, 5.0, 20.0)   # OGG_QUALITY_BIN_EDGES_DEG


class QualityExtremum(ctypes.Structure):
    """ogg_quality_extremum of include/ogg_hip.h"""
    _fields_ = [("value", c_double), ("lon", c_double), ("lat", c_double), ("j", c_longlong), ("i", c_longlong)]


class QualityResult(ctypes.Structure):
    """ogg_grid_quality_result of include/ogg_hip.h"""
    _fields_ = [("ext", QualityExtremum * QUALITY_N_EXTREMA), ("count", c_longlong * QUALITY_N_COUNTS)]


class TopogSource(ctypes.Structure):
    """ogg_topog_source of include/ogg_hip.h"""
    _fields_ = [("data", c_void_p), ("dtype", c_int), ("n_fill", c_int), ("fill", c_double * 2), ("Nx", c_long), ("Ny", c_long),
                ("lon0", c_double), ("dlon", c_double), ("lat0", c_double), ("dlat", c_double), ("quantum", c_double),
                ("wet_below", c_double)]


class TopogBand(ctypes.Structure):
    """ogg_topog_band of include/ogg_hip.h"""
    _fields_ = [("nx", c_long), ("j0", c_long), ("n_cell_rows", c_long), ("x", c_void_p), ("y", c_void_p), ("x_next", c_void_p),
                ("y_next", c_void_p), ("cells", c_int), ("refine", c_int), ("oversample", c_double)]


TOPOG_INT16, TOPOG_INT32, TOPOG_FLOAT32, TOPOG_FLOAT64 = 0, 1, 2, 3   # OGG_TOPOG_INT16 ... of include/ogg_hip.h
TOPOG_MODEL_CELLS, TOPOG_SUPERGRID_CELLS = 0, 1
TOPOG_MAX_REFINE, TOPOG_MAX_Q = 256, 1 << 21                           # OGG_TOPOG_MAX_REFINE, OGG_TOPOG_MAX_Q
TOPOG_POLE_EPS = 1.0e-10                                               # OGG_TOPOG_POLE_EPS
# ogg_topog_record as a numpy record (56 bytes)
TOPOG_RECORD = np.dtype([("n", "<i8"), ("n_missing", "<i8"), ("n_wet", "<i8"), ("sum", "<i8"), ("sumsq", "<i8"), ("min", "<i4"),
                         ("max", "<i4"), ("R", "<i4"), ("n_pole", "<i2"), ("n_clamped", "<i2")])
TOPOG_PLANE_MAX_OFFSET = 1 << 15                                       # OGG_TOPOG_PLANE_MAX_OFFSET
TOPOG_MOMENT_FIELDS = ("sx", "sy", "sxx", "sxy", "syy", "sxq", "syq", "n_far")
# ogg_topog_plane_record as a numpy record (120 bytes): the fields of ogg_topog_record (its ``base``), then the moments
TOPOG_PLANE_RECORD = np.dtype(TOPOG_RECORD.descr + [(f, "<i8") for f in TOPOG_MOMENT_FIELDS])

TOPOG_MAX_SOURCES = 4                                                  # OGG_TOPOG_MAX_SOURCES
TOPOG_LATLON, TOPOG_POLAR_STEREO = 0, 1                                # OGG_TOPOG_LATLON, OGG_TOPOG_POLAR_STEREO


class TopogProjection(ctypes.Structure):
    """ogg_topog_projection of include/ogg_hip.h"""
    _fields_ = [("h", c_int), ("reserved", c_int), ("lon0", c_double), ("a", c_double), ("e", c_double), ("K", c_double),
                ("lat_gate", c_double)]


class TopogLayer(ctypes.Structure):
    """ogg_topog_layer of include/ogg_hip.h"""
    _fields_ = [("src", TopogSource), ("kind", c_int), ("q_mul", c_int), ("proj", TopogProjection)]


# ogg_topog_merge_record as a numpy record (88 bytes): the fields of ogg_topog_record (its ``base``), then n_from[4]
TOPOG_MERGE_RECORD = np.dtype(TOPOG_RECORD.descr + [("n_from", "<i8", (TOPOG_MAX_SOURCES,))])


FACE_ONE_SIDED, FACE_POLE, FACE_SEAM, FACE_FOLD = 1, 2, 4, 8           # OGG_FACE_* of include/ogg_hip.h
TOPOG_FACE_WORDS = 7                                                   # OGG_TOPOG_FACE_WORDS
# a face record (OGG_TOPOG_FACE_WORDS int64 words, 56 bytes) as a numpy record: the byte offsets of include/ogg_hip.h
TOPOG_FACE_RECORD = np.dtype([("n", "<i8"), ("n_missing", "<i8"), ("ridge_sum", "<i8"), ("n_lines", "<i4"), ("n_lines_missing", "<i4"),
                              ("n_dry_lines", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("q_min", "<i4"), ("R", "<i4"), ("n_clamped", "<i2"),
                              ("flags", "<i2")])


class XgridAtm(ctypes.Structure):
    """ogg_xgrid_atm of include/ogg_hip.h"""
    _fields_ = [("lon", c_void_p), ("lat", c_void_p), ("NA", c_long), ("NB", c_long)]


class XgridBand(ctypes.Structure):
    """ogg_xgrid_band of include/ogg_hip.h"""
    _fields_ = [("nx", c_long), ("ny", c_long), ("j0", c_long), ("n_cell_rows", c_long), ("x", c_void_p), ("y", c_void_p),
                ("x_next", c_void_p), ("y_next", c_void_p), ("mask", c_void_p), ("Re", c_double), ("threshold", c_double)]


XGRID_COUNT_FIELDS = ("cells", "pole_cells", "pole_enclosing", "inverted", "degenerate", "masked", "candidates", "kept")


class XgridCounts(ctypes.Structure):
    """ogg_xgrid_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in XGRID_COUNT_FIELDS]


class XgridCsAtm(ctypes.Structure):
    """ogg_xgrid_cs_atm of include/ogg_hip.h"""
    _fields_ = [("t", c_void_p), ("N", c_long), ("frames", (c_double * 9) * 6)]


XGRID_CS_COUNT_FIELDS = ("cells", "degenerate", "wide", "inverted", "masked", "face_candidates", "candidates", "kept")


class XgridCsCounts(ctypes.Structure):
    """ogg_xgrid_cs_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in XGRID_CS_COUNT_FIELDS]


class XgridCurvSrc(ctypes.Structure):
    """ogg_xgrid_curv_src of include/ogg_hip.h"""
    _fields_ = [("x", c_void_p), ("y", c_void_p), ("NA", c_long), ("NB", c_long), ("ld", c_long), ("mask", c_void_p)]


XGRID_CURV_COUNT_FIELDS = ("cells", "degenerate", "wide", "inverted", "masked", "src_cells", "src_degenerate", "src_wide", "src_reversed",
                           "src_flat", "src_masked", "src_large", "candidates", "kept")


class XgridCurvCounts(ctypes.Structure):
    """ogg_xgrid_curv_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in XGRID_CURV_COUNT_FIELDS]


class MaskParams(ctypes.Structure):
    """ogg_mask_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("topology", c_int), ("mode", c_int), ("fill", c_double), ("min_depth", c_double),
                ("keep_min_cells", c_longlong)]


MASK_COUNT_FIELDS = ("wet_in", "masked", "deepened", "components", "largest", "kept", "removed", "wet_out")


class MaskCounts(ctypes.Structure):
    """ogg_mask_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in MASK_COUNT_FIELDS]


MASK_MASK, MASK_DEEPEN = 0, 1                                          # OGG_MASK_MASK, OGG_MASK_DEEPEN
MASK_PERIODIC, MASK_FOLD = 1, 2                                        # OGG_MASK_PERIODIC, OGG_MASK_FOLD
MASK_MAX_SEEDS = 1024                                                  # OGG_MASK_MAX_SEEDS


class RemapParams(ctypes.Structure):
    """ogg_remap_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("m0", c_long), ("NA", c_long), ("NB", c_long), ("nrec", c_long), ("dtype", c_int),
                ("n_fill", c_int), ("fill", c_double * 2), ("topology", c_int), ("fill_max", c_int)]


REMAP_COUNT_FIELDS = ("dry", "remapped", "filled", "unfilled", "bad_entries", "max_distance", "fronts", "launches")


class RemapCounts(ctypes.Structure):
    """ogg_remap_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in REMAP_COUNT_FIELDS]


REMAP_FLOAT32, REMAP_FLOAT64 = 0, 1                                    # OGG_REMAP_FLOAT32, OGG_REMAP_FLOAT64
REMAP_DRY, REMAP_REMAPPED, REMAP_FILLED, REMAP_UNFILLED = 0, 1, 2, 3   # OGG_REMAP_DRY ... OGG_REMAP_UNFILLED
REMAP_FILL = 1.0e20                                                    # OGG_REMAP_FILL
REMAP_MAX_FILLS = 2                                                    # OGG_REMAP_MAX_FILLS


class RunoffParams(ctypes.Structure):
    """ogg_runoff_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("NA", c_long), ("NB", c_long), ("nrec", c_long), ("dtype", c_int), ("n_fill", c_int),
                ("fill", c_double * 2), ("topology", c_int), ("targets", c_int), ("Re", c_double)]


RUNOFF_COUNT_FIELDS = ("targets", "mapped", "skipped", "missing", "cells", "max_sources", "tests", "bins")


class RunoffCounts(ctypes.Structure):
    """ogg_runoff_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in RUNOFF_COUNT_FIELDS]


RUNOFF_COAST, RUNOFF_WET = 0, 1                                        # OGG_RUNOFF_COAST, OGG_RUNOFF_WET
RUNOFF_MAX_BINS = 160                                                  # OGG_RUNOFF_MAX_BINS


class SpreadParams(ctypes.Structure):
    """ogg_spread_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("nrec", c_long), ("shape", c_int), ("use_classes", c_int), ("r2", c_double)]


SPREAD_COUNT_FIELDS = ("candidates", "mouths", "pairs", "max_receivers", "loaded", "max_mouths", "tests", "cubes")


class SpreadCounts(ctypes.Structure):
    """ogg_spread_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in SPREAD_COUNT_FIELDS]


SPREAD_UNIFORM, SPREAD_BIWEIGHT = 0, 1                                 # OGG_SPREAD_UNIFORM, OGG_SPREAD_BIWEIGHT
SPREAD_MAX_CUBES, SPREAD_MAX_PAIRS = 64, 1 << 30                       # OGG_SPREAD_MAX_CUBES, OGG_SPREAD_MAX_PAIRS


# the nine scalars every ogg_regional_* entry takes first: nx, ny, lon_c, lat_c, tilt, delta, Re, kind, metrics
REGIONAL_ARGS = [c_long, c_long, c_double, c_double, c_double, c_double, c_double, c_int, c_int]
REGIONAL_STEREO_ARGS = REGIONAL_ARGS[:7] + [c_int]                     # the ogg_regional_stereo_* entries: the same without kind
REGIONAL_LATLON, REGIONAL_MERCATOR = 0, 1                             # OGG_REGIONAL_LATLON, OGG_REGIONAL_MERCATOR
REGIONAL_MAX_CELLS = 1 << 22                                           # OGG_REGIONAL_MAX_CELLS


class CoastParams(ctypes.Structure):
    """ogg_coast_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("topology", c_int), ("sides", c_int)]


COAST_COUNT_FIELDS = ("coast_wet", "coast_land", "queries", "answered", "tests", "tiles", "cubes")


class CoastCounts(ctypes.Structure):
    """ogg_coast_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in COAST_COUNT_FIELDS]


COAST_WET, COAST_LAND = 1, 2                                           # OGG_COAST_WET, OGG_COAST_LAND
COAST_F_WET, COAST_F_COAST, COAST_F_VALID = 1, 2, 4                    # the bits of a flag byte
COAST_MAX_CUBES = 128                                                  # OGG_COAST_MAX_CUBES


class BasinParams(ctypes.Structure):
    """ogg_basin_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("topology", c_int), ("n_rules", c_int), ("seed_max_d2", c_double)]


BASIN_COUNT_FIELDS = ("wet", "coded", "uncoded", "passes")


class BasinCounts(ctypes.Structure):
    """ogg_basin_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in BASIN_COUNT_FIELDS]


# ogg_basin_rule and ogg_basin_rule_record as numpy records (56 and 32 bytes)
BASIN_RULE = np.dtype([("code", "<i4"), ("reserved", "<i4"), ("seed_lon", "<f8"), ("seed_lat", "<f8"), ("lon_w", "<f8"), ("lon_e", "<f8"),
                       ("lat_s", "<f8"), ("lat_n", "<f8")])
BASIN_RECORD = np.dtype([("seed_cell", "<i8"), ("d2_bits", "<i8"), ("status", "<i4"), ("blocking_rule", "<i4"), ("cells", "<i8")])
BASIN_MAX_RULES, BASIN_MAX_PASS_RULES = 4096, 255                      # OGG_BASIN_MAX_RULES, OGG_BASIN_MAX_PASS_RULES
BASIN_TOOK, BASIN_SEED_LAND, BASIN_SEED_OUTSIDE, BASIN_SEED_CODED, BASIN_SEED_OFF_GRID, BASIN_SEED_INVALID = range(6)   # OGG_BASIN_TOOK ...


# the six scalars every ogg_sill_* entry takes first: ny, nx, topology, bits, n_seeds, tile_rows; the counts are int64 words
SILL_ARGS = [c_long, c_long, c_int, c_int, c_int, c_int]
SILL_COUNT_FIELDS = ("rounds", "n_clamped", "n_bad_seeds", "n_connected", "n_cut_off", "n_regions", "n_gate_faces")   # OGG_SILL_COUNT_WORDS
SILL_SEED, SILL_MAX_BITS = 1 << 30, 30                                 # OGG_SILL_SEED, OGG_SILL_MAX_BITS


class RegridParams(ctypes.Structure):
    """ogg_regrid_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("NA", c_long), ("NB", c_long), ("nrec", c_long), ("dtype", c_int), ("n_fill", c_int),
                ("fill", c_double * 2), ("normalize", c_int)]


REGRID_COUNT_FIELDS = ("entries", "bad_entries", "cells", "max_entries", "valid", "empty")


class RegridCounts(ctypes.Structure):
    """ogg_regrid_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in REGRID_COUNT_FIELDS]


REGRID_AREA, REGRID_CELL = 0, 1                                        # OGG_REGRID_AREA, OGG_REGRID_CELL


class BilinearParams(ctypes.Structure):
    """ogg_bilinear_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("m0", c_long), ("NA", c_long), ("NB", c_long), ("nrec", c_long), ("dtype", c_int),
                ("n_fill", c_int), ("fill", c_double * 2), ("points", c_int), ("ncomp", c_int), ("topology", c_int), ("fill_max", c_int)]


BILINEAR_H, BILINEAR_U, BILINEAR_V, BILINEAR_C = 0, 1, 2, 3            # OGG_BILINEAR_H ... OGG_BILINEAR_C
BILINEAR_POINTS = {"h": BILINEAR_H, "u": BILINEAR_U, "v": BILINEAR_V, "c": BILINEAR_C}

class LayoutParams(ctypes.Structure):
    """ogg_layout_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("topology", c_int), ("halo", c_int)]


# ogg_layout_candidate and ogg_layout_record as numpy records (8 and 40 bytes)
LAYOUT_CANDIDATE = np.dtype([("px", "<i4"), ("py", "<i4")])
LAYOUT_RECORD_FIELDS = ("blocks", "masked", "pes", "max_block_cells", "max_block_edge", "min_block_size", "max_wet", "masked_cells",
                        "wet_total", "status")
LAYOUT_RECORD = np.dtype([(f, "<i4") for f in LAYOUT_RECORD_FIELDS])
LAYOUT_MAX_DIV, LAYOUT_MAX_CANDIDATES = 4096, 1 << 20                  # OGG_LAYOUT_MAX_DIV, OGG_LAYOUT_MAX_CANDIDATES
LAYOUT_TOO_FINE, LAYOUT_FOLD_ASYMMETRIC = 1, 2                         # OGG_LAYOUT_TOO_FINE, OGG_LAYOUT_FOLD_ASYMMETRIC


class LocateParams(ctypes.Structure):
    """ogg_locate_params of include/ogg_hip.h"""
    _fields_ = [("ny", c_long), ("nx", c_long), ("n", c_long), ("nrec", c_long), ("topology", c_int), ("mode", c_int), ("dtype", c_int),
                ("n_fill", c_int), ("fill", c_double * 2)]


LOCATE_COUNT_FIELDS = ("located", "outside", "invalid", "large_cells", "cubes", "tests", "flag0", "flag1", "flag2", "flag3")


class LocateCounts(ctypes.Structure):
    """ogg_locate_counts of include/ogg_hip.h"""
    _fields_ = [(f, c_longlong) for f in LOCATE_COUNT_FIELDS]


LOCATE_CELL, LOCATE_BILINEAR = 0, 1                                    # OGG_LOCATE_CELL, OGG_LOCATE_BILINEAR
LOCATE_MODES = {"cell": LOCATE_CELL, "bilinear": LOCATE_BILINEAR}
LOCATE_TOL = 2.0 ** -50                                                # OGG_LOCATE_TOL
LOCATE_MAX_CUBES, LOCATE_MAX_TOUCH = 128, 27                           # OGG_LOCATE_MAX_CUBES, OGG_LOCATE_MAX_TOUCH

# OGG_ABI_* of include/ogg_hip.h, in code order: name -> the mirror of ogg_<name> (a ctypes.Structure or a numpy record), whose size
# ogg_abi_sizeof(code) must give (tests/test_abi.py)
ABI_MIRRORS = {"LATLON_BAND": LatlonBand, "BIPOLAR_BAND": BipolarBand, "DPOLE_BAND": DpoleBand, "QUALITY_EXTREMUM": QualityExtremum,
               "GRID_QUALITY_RESULT": QualityResult, "QUALITY_BAND": QualityBand, "TOPOG_SOURCE": TopogSource, "TOPOG_BAND": TopogBand,
               "TOPOG_RECORD": TOPOG_RECORD, "TOPOG_PLANE_RECORD": TOPOG_PLANE_RECORD, "XGRID_ATM": XgridAtm, "XGRID_BAND": XgridBand,
               "XGRID_COUNTS": XgridCounts, "MASK_PARAMS": MaskParams, "MASK_COUNTS": MaskCounts, "REMAP_PARAMS": RemapParams,
               "REMAP_COUNTS": RemapCounts, "RUNOFF_PARAMS": RunoffParams, "RUNOFF_COUNTS": RunoffCounts, "REGRID_PARAMS": RegridParams,
               "REGRID_COUNTS": RegridCounts, "BILINEAR_PARAMS": BilinearParams, "COAST_PARAMS": CoastParams, "COAST_COUNTS": CoastCounts,
               "BASIN_PARAMS": BasinParams, "BASIN_RULE": BASIN_RULE, "BASIN_RULE_RECORD": BASIN_RECORD, "BASIN_COUNTS": BasinCounts,
               "XGRID_CS_ATM": XgridCsAtm, "XGRID_CS_COUNTS": XgridCsCounts, "LAYOUT_PARAMS": LayoutParams, "LAYOUT_CANDIDATE": LAYOUT_CANDIDATE,
               "LAYOUT_RECORD": LAYOUT_RECORD, "LOCATE_PARAMS": LocateParams, "LOCATE_COUNTS": LocateCounts, "TOPOG_PROJECTION": TopogProjection,
               "TOPOG_LAYER": TopogLayer, "TOPOG_MERGE_RECORD": TOPOG_MERGE_RECORD, "XGRID_CURV_SRC": XgridCurvSrc,
               "XGRID_CURV_COUNTS": XgridCurvCounts, "SPREAD_PARAMS": SpreadParams, "SPREAD_COUNTS": SpreadCounts}
ABI = {name: code for code, name in enumerate(ABI_MIRRORS)}


# name -> argtypes; every function returns int except the two string getters.  Must list EVERY symbol of ogg_hip.h
# (tests/test_abi.py checks this list against the header).
SIGNATURES = {
    "ogg_device_count": [ctypes.POINTER(c_int)],
    "ogg_set_device": [c_int],
    "ogg_device_name": [ctypes.c_char_p, c_int],
    "ogg_y_mercator_rounded": [c_long, c_long, c_void_p, c_void_p],
    "ogg_y_mercator_rounded_dev": [c_long, c_long, c_void_p, c_void_p, c_void_p],
    "ogg_phi_mercator": [c_long, c_long, c_void_p, c_void_p],
    "ogg_phi_mercator_dev": [c_long, c_long, c_void_p, c_void_p, c_void_p],
    "ogg_mercator_axis_dev": [c_long, c_longlong, c_long, c_void_p, c_void_p],
    "ogg_linear_axis_dev": [c_long, c_double, c_double, c_double, c_void_p, c_void_p],
    "ogg_tile_latlon": [c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_tile_latlon_dev": [c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_generate_latlon_grid": [c_long, c_long, c_double, c_double, c_double, c_double, c_int, c_void_p, c_void_p],
    "ogg_grid_metrics_midas_dev": [c_long, c_long, c_void_p, c_void_p, c_long, c_long, c_double, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p],
    "ogg_grid_metrics_midas_plan": [c_long, c_long, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
    "ogg_grid_metrics_midas": [c_long, c_long, c_void_p, c_void_p, c_double, c_int, c_void_p, c_void_p, c_void_p],
    "ogg_angle_x": [c_long, c_long, c_void_p, c_void_p, c_void_p],
    "ogg_bipolar_projection": [c_long, c_void_p, c_void_p, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_bipolar_projection_dev": [c_long, c_void_p, c_void_p, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p],
    "ogg_bipolar_cap_mesh_sym": [c_long, c_long, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_bipolar_cap_metrics_quad_sym": [c_int, c_long, c_long, c_double, c_double, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p],
    "ogg_displaced_pole_metrics_quad_form_sym": [c_int, c_int, c_int, c_long, c_long, c_double, c_double, c_double, c_double, c_double, c_void_p,
                                                 c_void_p, c_void_p],
    "ogg_symmetry_coverage": [c_int, c_int, c_long, c_double, c_double, c_int, c_void_p, c_void_p, c_void_p],
    "ogg_bipolar_cap_mesh_angle_sym_dev": [c_long, c_long, c_double, c_double, c_long, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p],
    "ogg_bipolar_cap_mesh": [c_long, c_long, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_bipolar_cap_metrics_quad_sym_ws_dev": [c_int, c_long, c_long, c_double, c_double, c_double, c_double, c_long, c_long, c_long, c_int,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "ogg_bipolar_cap_metrics_quad": [c_int, c_long, c_long, c_double, c_double, c_double, c_double, c_void_p, c_void_p,
                                     c_void_p],
    "ogg_displaced_pole_mesh_dev": [c_long, c_void_p, c_long, c_void_p, c_long, c_long, c_double, c_double, c_double,
                                    c_double, c_void_p, c_void_p, c_void_p],
    "ogg_displaced_pole_mesh": [c_long, c_void_p, c_long, c_void_p, c_long, c_long, c_double, c_double, c_double, c_double,
                                c_void_p, c_void_p],
    "ogg_displaced_pole_numerical_h_dev": [c_long, c_void_p, c_long, c_void_p, c_long, c_long, c_double, c_double, c_double,
                                           c_double, c_double, c_int, c_void_p, c_void_p, c_void_p],
    "ogg_displaced_pole_numerical_h": [c_long, c_void_p, c_long, c_void_p, c_long, c_long, c_double, c_double, c_double,
                                       c_double, c_double, c_int, c_void_p, c_void_p],
    "ogg_displaced_pole_metrics_quad": [c_int, c_long, c_long, c_double, c_double, c_double, c_double, c_double, c_void_p,
                                        c_void_p, c_void_p],
    "ogg_displaced_pole_metrics_quad_form_sym_ws_dev": [c_int, c_int, c_int, c_long, c_long, c_double, c_double, c_double, c_double, c_double,
                                                        c_long, c_long, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "ogg_displaced_pole_grid_angle_ws_dev": [c_long, c_long, c_double, c_double, c_double, c_double, c_long, c_long, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "ogg_workspace_error_flag_dev": [c_void_p, ctypes.POINTER(c_int), c_void_p],
    "ogg_y_mercator": [c_long, c_long, c_void_p, c_void_p],
    "ogg_y_mercator_dev": [c_long, c_long, c_void_p, c_void_p, c_void_p],
    "ogg_affine_index": [c_long, c_void_p, c_double, c_double, c_double, c_void_p],
    "ogg_affine_index_dev": [c_long, c_void_p, c_double, c_double, c_double, c_void_p, c_void_p],
    "ogg_mdist": [c_long, c_void_p, c_void_p, c_void_p],
    "ogg_mdist_dev": [c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_haversine": [c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_haversine_dev": [c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_bipolar_cap_ij_array": [c_long, c_void_p, c_long, c_void_p, c_long, c_long, c_double, c_double, c_double, c_void_p,
                                 c_void_p],
    "ogg_bipolar_cap_ij_array_dev": [c_long, c_void_p, c_long, c_void_p, c_long, c_long, c_double, c_double, c_double,
                                     c_void_p, c_void_p, c_void_p],
    "ogg_displaced_pole_projection": [c_long, c_long, c_void_p, c_void_p, c_double, c_double, c_double, c_double, c_void_p,
                                      c_void_p],
    "ogg_displaced_pole_projection_dev": [c_long, c_long, c_void_p, c_void_p, c_double, c_double, c_double, c_double,
                                          c_void_p, c_void_p, c_void_p],
    "ogg_monotonic_bounding": [c_long, c_long, c_void_p, c_double],
    "ogg_monotonic_bounding_dev": [c_long, c_long, c_void_p, c_double, c_void_p],
    "ogg_latlon_supergrid_multi_dev": [c_int, ctypes.POINTER(LatlonBand), c_long, c_double, c_double, c_double, c_int, c_void_p],
    "ogg_latlon_supergrid_rows_ws_dev": [c_int, ctypes.POINTER(LatlonBand), c_long, c_double, c_double, c_double, c_int, c_void_p, c_long,
                                         c_void_p],
    "ogg_tripolar_pass_dev": [c_int, ctypes.POINTER(LatlonBand), c_long, c_double, c_double, c_double, c_int,
                              ctypes.POINTER(BipolarBand), c_void_p],
    "ogg_supergrid_pass_dev": [c_int, ctypes.POINTER(LatlonBand), c_long, c_double, c_double, c_double, c_int,
                               ctypes.POINTER(BipolarBand), ctypes.POINTER(DpoleBand), ctypes.POINTER(c_void_p), ctypes.POINTER(c_double),
                               c_void_p],
    "ogg_supergrid_pass_plan_dev": [c_int, ctypes.POINTER(LatlonBand), c_long, c_double, c_double, c_double, c_int,
                                    ctypes.POINTER(BipolarBand), ctypes.POINTER(DpoleBand), ctypes.POINTER(c_void_p)],
    "ogg_supergrid_pass_run_dev": [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_double), c_void_p],
    "ogg_supergrid_pass_plan_destroy": [c_void_p],
    "ogg_supergrid_pass_plan_flags_dev": [c_void_p, ctypes.POINTER(c_int), c_void_p],
    "ogg_fill_dev": [c_long, c_double, c_void_p, c_void_p],
    "ogg_bswap64_dev": [c_long, c_void_p, c_void_p, c_void_p],
    "ogg_libm_check_dev": [c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_math_eval_dev": [c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_metrics_sums_dev": [c_long, c_long, c_long, c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_void_p, c_void_p],
    "ogg_grid_quality_band_dev": [ctypes.POINTER(QualityBand), c_void_p, c_long, c_void_p, c_void_p],
    "ogg_grid_quality": [ctypes.POINTER(QualityBand), ctypes.POINTER(QualityResult)],
    "ogg_topog_band_dev": [ctypes.POINTER(TopogBand), ctypes.POINTER(TopogSource), c_void_p, c_long, c_void_p, c_void_p],
    "ogg_topog_quantize_dev": [ctypes.POINTER(TopogSource), c_void_p, c_void_p, c_void_p],
    "ogg_topog": [ctypes.POINTER(TopogBand), ctypes.POINTER(TopogSource), c_void_p],
    "ogg_topog_plane_band_dev": [ctypes.POINTER(TopogBand), ctypes.POINTER(TopogSource), c_void_p, c_long, c_void_p, c_void_p],
    "ogg_topog_plane": [ctypes.POINTER(TopogBand), ctypes.POINTER(TopogSource), c_void_p],
    "ogg_topog_layers_band_dev": [ctypes.POINTER(TopogBand), c_int, ctypes.POINTER(TopogLayer), c_void_p, c_long, c_void_p, c_void_p],
    "ogg_topog_layer_range_dev": [ctypes.POINTER(TopogLayer), c_void_p, c_void_p],
    "ogg_topog_layers": [ctypes.POINTER(TopogBand), c_int, ctypes.POINTER(TopogLayer), c_void_p],
    "ogg_topog_project_dev": [ctypes.POINTER(TopogProjection), c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_topog_faces_check": [ctypes.POINTER(TopogBand), c_long, c_int, c_long, c_long, c_long, c_long, ctypes.POINTER(TopogSource), c_int],
    "ogg_topog_faces_dev": [ctypes.POINTER(TopogBand), c_long, c_int, c_long, c_long, c_long, c_long, ctypes.POINTER(TopogSource), c_void_p, c_long, c_void_p,
                            c_void_p, c_void_p],
    "ogg_topog_faces": [ctypes.POINTER(TopogBand), c_long, c_int, c_long, c_long, c_long, c_long, ctypes.POINTER(TopogSource), c_void_p, c_void_p],
    "ogg_xgrid_check_atm": [ctypes.POINTER(XgridAtm)],
    "ogg_xgrid_count_dev": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridAtm), c_void_p, c_long, c_void_p, c_void_p, c_void_p],
    "ogg_xgrid_write_dev": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridAtm), c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                            c_void_p],
    "ogg_xgrid": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridAtm), c_long, c_void_p, c_void_p, c_void_p, c_void_p,
                  ctypes.POINTER(XgridCounts)],
    "ogg_xgrid_cs_check_atm": [ctypes.POINTER(XgridCsAtm)],
    "ogg_xgrid_cs_count_dev": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCsAtm), c_void_p, c_long, c_void_p, c_void_p, c_void_p],
    "ogg_xgrid_cs_write_dev": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCsAtm), c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                               c_void_p],
    "ogg_xgrid_cs": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCsAtm), c_long, c_void_p, c_void_p, c_void_p, c_void_p,
                     ctypes.POINTER(XgridCsCounts)],
    "ogg_xgrid_curv_check": [ctypes.POINTER(XgridCurvSrc)],
    "ogg_xgrid_curv_sets_dev": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCurvSrc), c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                                c_void_p],
    "ogg_xgrid_curv_clip_dev": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCurvSrc), c_void_p, c_long, c_long, c_void_p, c_long,
                                c_void_p, c_void_p],
    "ogg_xgrid_curv_write_dev": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCurvSrc), c_long, c_void_p, c_long, c_void_p, c_void_p,
                                 c_void_p, c_void_p],
    "ogg_xgrid_curv": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCurvSrc), c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                       ctypes.POINTER(XgridCurvCounts)],
    "ogg_mask_check": [ctypes.POINTER(MaskParams)],
    "ogg_mask_label_dev": [ctypes.POINTER(MaskParams), c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_mask_seed_dev": [ctypes.POINTER(MaskParams), c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p],
    "ogg_mask_apply_dev": [ctypes.POINTER(MaskParams), c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_void_p, c_void_p,
                           c_void_p, c_void_p],
    "ogg_ocean_mask": [ctypes.POINTER(MaskParams), c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_void_p, c_long, ctypes.POINTER(MaskCounts)],
    "ogg_remap_check": [ctypes.POINTER(RemapParams)],
    "ogg_remap_segments_dev": [ctypes.POINTER(RemapParams), c_void_p, c_long, c_void_p, c_long, c_void_p],
    "ogg_remap_dev": [ctypes.POINTER(RemapParams), c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                      c_void_p, c_void_p],
    "ogg_remap_fill_dev": [ctypes.POINTER(RemapParams), c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_remap": [ctypes.POINTER(RemapParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_void_p, c_void_p,
                  ctypes.POINTER(RemapCounts)],
    "ogg_runoff_check": [ctypes.POINTER(RunoffParams)],
    "ogg_runoff_targets_dev": [ctypes.POINTER(RunoffParams), c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                               c_void_p, c_void_p],
    "ogg_runoff_sources_dev": [ctypes.POINTER(RunoffParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p],
    "ogg_runoff_search_dev": [ctypes.POINTER(RunoffParams), c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_void_p,
                              c_void_p, c_void_p, c_void_p],
    "ogg_runoff_segments_dev": [ctypes.POINTER(RunoffParams), c_void_p, c_long, c_void_p, c_long, c_void_p],
    "ogg_runoff_accumulate_dev": [ctypes.POINTER(RunoffParams), c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_void_p,
                                  c_void_p, c_void_p, c_void_p],
    "ogg_runoff": [ctypes.POINTER(RunoffParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                   c_void_p, c_void_p, c_void_p, ctypes.POINTER(RunoffCounts)],
    "ogg_spread_check": [ctypes.POINTER(SpreadParams)],
    "ogg_spread_sets_dev": [ctypes.POINTER(SpreadParams), c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_long,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_spread_count_dev": [ctypes.POINTER(SpreadParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p,
                             c_void_p, c_void_p, c_void_p],
    "ogg_spread_pairs_dev": [ctypes.POINTER(SpreadParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_void_p, c_long,
                             c_void_p],
    "ogg_spread_apply_dev": [ctypes.POINTER(SpreadParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_void_p,
                             c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_runoff_spread": [ctypes.POINTER(SpreadParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(SpreadCounts)],
    "ogg_regional_check": REGIONAL_ARGS,
    "ogg_regional_tables_dev": REGIONAL_ARGS + [c_void_p, c_long, c_void_p],
    "ogg_regional_band_dev": REGIONAL_ARGS + [c_long, c_long, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p],
    "ogg_regional_grid": REGIONAL_ARGS + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_regional_stereo_check": REGIONAL_STEREO_ARGS,
    "ogg_regional_stereo_tables_dev": REGIONAL_STEREO_ARGS + [c_void_p, c_long, c_void_p],
    "ogg_regional_stereo_band_dev": REGIONAL_STEREO_ARGS + [c_long, c_long, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                            c_void_p, c_void_p],
    "ogg_regional_stereo_grid": REGIONAL_STEREO_ARGS + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_coast_check": [ctypes.POINTER(CoastParams)],
    "ogg_coast_sets_dev": [ctypes.POINTER(CoastParams), c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_coast_search_dev": [ctypes.POINTER(CoastParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long,
                             c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_coast_distance": [ctypes.POINTER(CoastParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           ctypes.POINTER(CoastCounts)],
    "ogg_sill_check": SILL_ARGS,
    "ogg_sill_depth_dev": SILL_ARGS + [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p],
    "ogg_sill_depth": SILL_ARGS + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_basin_check": [ctypes.POINTER(BasinParams), c_void_p],
    "ogg_basin_plan": [ctypes.POINTER(BasinParams), c_void_p, c_void_p, ctypes.POINTER(c_int)],
    "ogg_basin_codes_dev": [ctypes.POINTER(BasinParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_basin_codes": [ctypes.POINTER(BasinParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                        ctypes.POINTER(BasinCounts)],
    "ogg_regrid_check": [ctypes.POINTER(RegridParams)],
    "ogg_regrid_transpose_dev": [ctypes.POINTER(RegridParams), c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p],
    "ogg_regrid_dev": [ctypes.POINTER(RegridParams), c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_void_p],
    "ogg_regrid": [ctypes.POINTER(RegridParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p,
                   c_void_p, ctypes.POINTER(RegridCounts)],
    "ogg_bilinear_check": [ctypes.POINTER(BilinearParams), c_int],
    "ogg_bilinear_dev": [ctypes.POINTER(BilinearParams), c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_bilinear_rotate_dev": [ctypes.POINTER(BilinearParams), c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    "ogg_bilinear": [ctypes.POINTER(BilinearParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                     c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_layout_extent": [c_long, c_long, c_void_p, c_void_p],
    "ogg_layout_check": [ctypes.POINTER(LayoutParams), c_void_p, c_long],
    "ogg_layout_table_dev": [ctypes.POINTER(LayoutParams), c_void_p, c_void_p, c_long, c_void_p],
    "ogg_layout_sweep_dev": [ctypes.POINTER(LayoutParams), c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p],
    "ogg_layout_blocks_dev": [ctypes.POINTER(LayoutParams), c_int, c_int, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p,
                              c_void_p],
    "ogg_layouts": [ctypes.POINTER(LayoutParams), c_void_p, c_void_p, c_long, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                    c_void_p],
    "ogg_locate_check": [ctypes.POINTER(LocateParams)],
    "ogg_locate_sets_dev": [ctypes.POINTER(LocateParams), c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p, c_void_p],
    "ogg_locate_index_dev": [ctypes.POINTER(LocateParams), c_void_p, c_long, c_void_p, c_void_p],
    "ogg_locate_search_dev": [ctypes.POINTER(LocateParams), c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p],
    "ogg_locate_sample_dev": [ctypes.POINTER(LocateParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p],
    "ogg_locate": [ctypes.POINTER(LocateParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                   c_void_p, ctypes.POINTER(LocateCounts)],
    "ogg_locate_sample": [ctypes.POINTER(LocateParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          ctypes.POINTER(LocateCounts)],
    "ogg_event_create": [ctypes.POINTER(c_void_p)],
    "ogg_event_destroy": [c_void_p],
    "ogg_event_record": [c_void_p, c_void_p],
    "ogg_event_elapsed_ms": [c_void_p, c_void_p, ctypes.POINTER(ctypes.c_float)],
    "ogg_stream_synchronize": [c_void_p],
}
STRING_GETTERS = ("ogg_last_error", "ogg_version")
LONG_GETTERS = {"ogg_abi_sizeof": [c_int],
                "ogg_bipolar_quad_workspace_bytes": [c_int, c_long, c_long],
                "ogg_displaced_pole_quad_workspace_bytes": [c_int, c_long, c_long],
                "ogg_displaced_pole_grid_workspace_bytes": [c_long, c_long],
                "ogg_dpole_band_workspace_bytes": [c_int, c_long, c_long],
                "ogg_latlon_rows_workspace_bytes": [c_int, ctypes.POINTER(LatlonBand), c_long],
                "ogg_supergrid_pass_plan_slots": [c_void_p],
                "ogg_supergrid_pass_plan_carried_runs": [c_void_p],
                "ogg_grid_quality_workspace_bytes": [c_long, c_long],
                "ogg_topog_band_out_rows": [ctypes.POINTER(TopogBand)],
                "ogg_topog_workspace_bytes": [],
                "ogg_xgrid_band_first_row": [ctypes.POINTER(XgridBand)],
                "ogg_xgrid_band_out_rows": [ctypes.POINTER(XgridBand)],
                "ogg_xgrid_band_next_rows": [ctypes.POINTER(XgridBand)],
                "ogg_xgrid_workspace_bytes": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridAtm)],
                "ogg_xgrid_cs_workspace_bytes": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCsAtm)],
                "ogg_xgrid_curv_workspace_bytes": [ctypes.POINTER(XgridBand), ctypes.POINTER(XgridCurvSrc), c_long],
                "ogg_mask_workspace_bytes": [ctypes.POINTER(MaskParams)],
                "ogg_remap_workspace_bytes": [ctypes.POINTER(RemapParams)],
                "ogg_runoff_workspace_bytes": [ctypes.POINTER(RunoffParams)],
                "ogg_spread_workspace_bytes": [ctypes.POINTER(SpreadParams), c_long],
                "ogg_regional_workspace_bytes": REGIONAL_ARGS,
                "ogg_regional_stereo_workspace_bytes": REGIONAL_STEREO_ARGS,
                "ogg_coast_workspace_bytes": [ctypes.POINTER(CoastParams)],
                "ogg_basin_workspace_bytes": [ctypes.POINTER(BasinParams)],
                "ogg_sill_workspace_bytes": [c_long, c_long],
                "ogg_regrid_workspace_bytes": [ctypes.POINTER(RegridParams), c_long],
                "ogg_layout_workspace_bytes": [ctypes.POINTER(LayoutParams)],
                "ogg_locate_workspace_bytes": [ctypes.POINTER(LocateParams)]}

_lib = None


class OggHipError(Exception):
    """A libogg_hip.so call failed; .code is the OGG_E* value."""

    def __init__(self, code, text):
        Exception.__init__(self, text)
        self.code = code


def load():
    """Load libogg_hip.so (once).  Raises if it is missing: there is no CPU path behind this package."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libogg_hip.so is not built (%s). Run `python -m ocean_model_grid_generator_amd.csrc.build` "
                          "(needs hipcc); this package has no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64 / libhsa-runtime64, and whichever
    # runtime touches the GPU second sees no device.  Importing torch first makes libogg_hip.so bind to the runtime
    # torch already loaded (same SONAME), so torch tensors, streams and RCCL share one runtime with our kernels.
    # Without torch installed the system runtime under /opt/rocm is used.  OGG_NO_TORCH=1 skips the import.
    if not os.environ.get("OGG_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        if os.environ.get("OGG_LIB_PATH") and not hasattr(lib, name):
            continue   # an older build under A/B timing (scripts/ab_time.py): the entry points it lacks are not called there
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_int
    for name in STRING_GETTERS:
        getattr(lib, name).restype = ctypes.c_char_p
        getattr(lib, name).argtypes = []
    for name, argtypes in LONG_GETTERS.items():
        if os.environ.get("OGG_LIB_PATH") and not hasattr(lib, name):
            continue   # as above
        getattr(lib, name).restype = c_long
        getattr(lib, name).argtypes = argtypes
    _lib = lib
    return lib


def check(code):
    """Turn a non-zero return code into the exception the reference would raise."""
    if code == OGG_OK:
        return
    text = load().ogg_last_error().decode("utf-8", "replace")
    if code in (OGG_EORDER, OGG_ESHAPE):
        # reference texts: "Uncoded order", "order not coded", "Input arrays do not have the same shape!"
        raise Exception(text)
    raise OggHipError(code, "libogg_hip: %s" % text)


def call(name, *args):
    check(getattr(load(), name)(*args))


def checked(name, p, *args):
    """p after the library's ogg_*_check ``name`` took it; the reason of a refusal as a ValueError (no device is needed)"""
    lib = load()
    if getattr(lib, name)(ctypes.byref(p), *args) != OGG_OK:
        raise ValueError(lib.ogg_last_error().decode())
    return p


def counts_dict(fields, c):
    """{field: int} of a counts struct, or of the counts in the fields' order (a numpy array or a device tensor)"""
    if isinstance(c, ctypes.Structure):
        return {f: int(getattr(c, f)) for f in fields}
    return {f: int(v) for f, v in zip(fields, c.cpu().numpy() if hasattr(c, "cpu") else c)}


def ptr(a):
    """Host pointer of a C-contiguous float64/int64 numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def source_hash():
    """The kernel-source hash compiled into the loaded library (the tail of ogg_version())."""
    v = load().ogg_version().decode()
    return v.split(" src ")[1] if " src " in v else None


def device_count():
    n = c_int(0)
    rc = load().ogg_device_count(ctypes.byref(n))
    return n.value if rc == OGG_OK else 0


def device_name():
    buf = ctypes.create_string_buffer(256)
    call("ogg_device_name", buf, 256)
    return buf.value.decode()
