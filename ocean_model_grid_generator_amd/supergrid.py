"""Device-resident, latitude-band-sharded supergrid pass (the benchmark / multi-GPU path).

One process per GPU.  Every rank owns a contiguous band of rows of EACH sub-grid (southern cap, Southern Ocean,
Mercator, bipolar cap): cost per row differs by ~100x between the lat-lon sub-grids and the caps, so cutting the
stitched grid into contiguous slabs would not balance.  One pass (default pipeline, ``latlon="fused"``, ``launch="pass"``) is

  ogg_supergrid_pass_dev  three launches on the caller's stream (through a plan handle, as Supergrid calls it, the first of them rides
                          in the previous pass's second): the quadrature tables; then ONE launch that carries the
                          lat-lon row strips (x, y, dx, dy, area, angle_dx from the axis formulas: 48 B written per cell,
                          nothing read), the mesh + angle workgroups of both caps and their quadrature strips side by side; then
                          the literal fix-up of the guarded bipolar cells (a displaced-pole quadrature in the reference's literal
                          arc form, ``dp_arc="literal"``, is a fourth launch: it needs more registers than launch B should have)

with no exchange between ranks: the caps are analytic in (i, j) and the lat-lon kernel needs only the axis formulas.
``launch="kernels"`` runs one launch per sub-grid and phase instead (the caps on side streams when ``overlap`` is set) and gives
the same bits.  ``latlon="stencil"`` is the pipeline of BASELINE.json's north_star taken literally: tile x, y (K1); send the first
x/y row of every band to the rank below (neighbour send/recv over RCCL, torch.distributed backend "nccl"); generic 2x3-stencil
kernel (K2) that reads x, y back.  Same bits again.  ``metrics_error()`` is the one collective of the default pipeline.

All six fields of every band stay in HBM (torch tensors); ``bands_to_host()`` copies them out and ``stitch()`` assembles the
sub-grids on the host exactly as the reference does (OGG:1315-1365).

torch is used for device memory, streams, graphs and torch.distributed only; every number is produced by libogg_hip.so.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib as L
from . import ocean_grid_generator as ogg

FIELDS = ("x", "y", "dx", "dy", "area", "angle_dx")


def band(n_rows, rank, world):
    """Rows [lo, hi) of an n_rows-row sub-grid owned by `rank` (contiguous, balanced to within one row)."""
    return (n_rows * rank) // world, (n_rows * (rank + 1)) // world


def band_weighted(cost, rank, world, top_capacity=1.0, capacities=None):
    """Contiguous rows [lo, hi) of `rank` such that every rank gets about the same total cost; `cost` is the per-row
    cost array.  ``top_capacity``: the share of the LAST rank relative to the others' (it carries a fixed extra launch, the
    literal fix-up of the bipolar quadrature, and so takes a smaller share of EVERY sub-grid: the lat-lon strips and the cap
    workgroups of a rank finish together, so shortening one of them alone shortens nothing).  ``capacities``: one relative share
    per rank instead (refine_split: what every rank measured on its own GPU).  The boundaries are a function of (cost, world,
    top_capacity or capacities) only, identical on every rank."""
    c = np.concatenate(([0.0], np.cumsum(np.asarray(cost, dtype=np.float64))))
    total = c[-1]
    caps = [1.0] * (world - 1) + [float(top_capacity)] if capacities is None else [float(v) for v in capacities]
    if len(caps) != world or min(caps) <= 0.0:
        raise ValueError("band_weighted: %d capacities for %d ranks (all must be positive)" % (len(caps), world))
    before = np.concatenate(([0.0], np.cumsum(caps)))

    def edge(r):
        if r <= 0:
            return 0
        if r >= world:
            return len(cost)
        return int(np.searchsorted(c, total * before[r] / before[-1], side="left"))

    return edge(rank), edge(rank + 1)


class SubGridPlan(object):
    """Size and scalars of one sub-grid; `row0` is the first KEPT point row in the sub-grid's native numbering
    (e.g. the first row after the displaced-pole doughnut) and `nj1` the number of kept point rows."""

    def __init__(self, name, kind, nj1, row0=0, **scalars):
        self.name, self.kind, self.nj1, self.row0 = name, kind, int(nj1), int(row0)
        self.__dict__.update(scalars)


def all_reduce(t, op=None):
    """torch.distributed.all_reduce of a device tensor: over RCCL where the process group is one (backend "nccl"); through the host
    where it is gloo -- the CPU tests and the one-GPU rehearsal of bench.py, whose ranks share a card that RCCL will not share."""
    import torch.distributed as dist
    kw = {} if op is None else {"op": op}
    if t.is_cuda and dist.get_backend() == "gloo":
        c = t.cpu()
        dist.all_reduce(c, **kw)
        t.copy_(c)
    else:
        dist.all_reduce(t, **kw)
    return t


class SupergridPlan(object):
    """Host-side size logic of main() (OGG:969-1197, 1268-1313) for its whole flag surface: sub-grid selection (--grids), latitude
    overrides, --enhanced_equatorial (the spliced 1-D axis is built on the host, OGG:349-428, and handed to the lat-lon kernel as an
    explicit axis), --match_dy, --ensure_nj_even, the displaced pole, the doughnut and the south cuts (rows a cut removes are not
    generated when the cut follows from the sizes alone; a cut by angle of a displaced-pole cap is applied at stitch time).
    Needs the GPU unless ``mercator_axis`` is given: y* and the Mercator axis come from the device kernels, exactly as main() reads
    the joint latitudes off phiMerc."""

    def __init__(self, inverse_resolution, r_dp=0.0, lon_dp=80.0, lat_dp=-99.0, exfracdp=0.49, south_cutoff_row=0, south_cutoff_ang=-90.0,
                 skip_metrics=False, ensure_nj_even=False, no_south_cap=False, enhanced_equatorial=0, match_dy=(), grids="all",
                 shift_equator_to_u_point=True, bipolar_lower_lat=-99.0, mercator_lower_lat=-99.0, mercator_upper_lat=-99.0,
                 south_ocean_lower_lat=-99.0, Re=ogg._default_Re, mercator_axis=None, dp_arc=None, cap_symmetry=None):
        """``mercator_axis`` = (y0, phi_M) lets a caller that already holds the Mercator ordinate range and axis skip the
        two device calls (the CPU tests of the band / halo logic pass values computed elsewhere).  ``dp_arc``: arc form of
        the displaced-pole quadrature, "chord" (default, or OGG_DP_ARC: the form closer to the exact value of the reference's formula,
        DESIGN.md section 2) or "literal" (the reference's operation sequence; a fourth launch of the pass).  ``exfracdp=None``:
        main()'s own default 0.28*7/4 (OGG:891-892).  ``cap_symmetry``: None (the library's default: mirrored columns unless
        OGG_CAP_SYMMETRY=0), True / "mirror", False / "none" (every column of both caps evaluated, as the reference does)."""
        import contextlib
        import io

        refineS, refineR = 2, inverse_resolution
        self.Re = Re
        self.dp_arc = {"literal": L.DP_ARC_LITERAL, "chord": L.DP_ARC_CHORD}[dp_arc or ogg.default_dp_arc()]
        self.cap_symmetry = ogg._sym(cap_symmetry)   # OGG_SYM_* of include/ogg_hip.h
        self.skip_metrics = skip_metrics
        self.ensure_nj_even = ensure_nj_even
        self.south_cutoff_row, self.south_cutoff_ang = south_cutoff_row, south_cutoff_ang
        self.lon0, self.lenlon = -300.0, 360.0
        self.Ni = Ni = int(refineR * refineS * 360)
        doughnut = exfracdp if exfracdp is not None else 0.28 * 7 / 4

        def want(tok):   # OGG:1003,1035,1100,1140
            return (tok in grids) or ("all" in grids)

        # ---- Mercator (OGG:987-1030)
        phi_s, phi_n = -66.85954725, 64.05895973
        if mercator_upper_lat > -90:
            phi_n = mercator_upper_lat
        if mercator_lower_lat > -90:
            phi_s = mercator_lower_lat
        if refineR == 2:
            phi_s, phi_n = -68.0, 65.0
        if refineR == 1 and enhanced_equatorial:
            phi_s, phi_n = -77.8, 60.0
        merc = bp = so = sc = None
        phi_kept = None   # the Mercator latitudes main() sees as phiMerc[:, Ni//4]
        if want("mercator"):
            if mercator_axis is None:
                with contextlib.redirect_stdout(io.StringIO()):
                    phi_M, y_star = ogg.mercator_axis(Ni, phi_s, phi_n, refineR, shift_equator_to_u_point, ensure_nj_even, enhanced_equatorial,
                                                      return_y_star=True)
                y0 = int(y_star[0])
            else:
                y0, phi_M = int(mercator_axis[0]), np.asarray(mercator_axis[1], dtype=np.float64)
                if np.searchsorted(phi_M, 0.0) == 0:
                    raise Exception("   Ooops: Equator is not in the grid")
            skipM = 1 if (phi_M.size % 2 == 0 and ensure_nj_even) else 0                     # OGG:434-437
            merc = SubGridPlan("Merc", "mercator", phi_M.size - skipM, row0=skipM, y0=y0, n_axis=phi_M.size,
                               explicit_axis=(np.ascontiguousarray(phi_M) if enhanced_equatorial else None))
            phi_kept = phi_M[skipM:]
            dphi_so, dphi_no = phi_kept[1] - phi_kept[0], phi_kept[-1] - phi_kept[-2]        # OGG:1024-1025
            lat0_bp = float(phi_kept[-1])
        # ---- bipolar cap (OGG:1035-1062)
        if want("bipolar"):
            if bipolar_lower_lat > -90:
                lat0_bp = bipolar_lower_lat
            elif merc is None:
                raise Exception("the bipolar cap takes its lower latitude from the Mercator sub-grid (OGG:1030): add mercator to --grids "
                                "or give --bipolar_lower_lat")
            Nj_ncap = int(60 * refineR * refineS)
            if refineR == 2:
                Nj_ncap = 119 * refineS
            if refineR == 1 and enhanced_equatorial:
                Nj_ncap = 154
            if "bp" in match_dy:
                Nj_ncap = int(0.5 + (90.0 - lat0_bp) / dphi_no)
            if Nj_ncap % 2 != 0 and ensure_nj_even:
                Nj_ncap -= 1
            bp = SubGridPlan("BP", "bipolar", Nj_ncap + 1, Nj=Nj_ncap, lat0_bp=float(lat0_bp), lon_bp=self.lon0,
                             rp=float(np.tan(0.5 * (90 - lat0_bp) * ogg.PI_180)))
            # Row cost for the band split of the cap, in units of a plain cell row.  The quadrature guards its algebraic per-point form
            # near the two pole points (csrc/ogg_bipolar_dev.h, bp_point_fast): cell rows whose top edge lies above acos(2/sqrt(K))
            # carry the guard (1.3x a plain row).  The band that holds the last row also runs the tail launch (literal fix-up of the
            # guarded cells), a fixed cost of ~6.5 us whatever the resolution: that is taken off the last rank's share of EVERY sub-grid
            # (rows_of: tail_us / pass_us below), not off its cap rows alone -- a rank's lat-lon strips and cap workgroups end together
            # (timeline of launch B at 1/8 of the 1/8 degree grid: strips 35 us, quadrature 39 us), so a smaller cap share alone left the
            # last rank as slow as before.  (scripts/rank_sweep.py; OGG_BP_ROW_COST="fix,guard,lump" overrides the row weights: rows with
            # fix-up cells, guarded rows, a lump on the last row; OGG_TOP_RANK_TAIL_US the tail time.)
            import os
            K = float(os.environ.get("OGG_BP_GUARD_K", "4000"))
            if K > 4.0:
                lat_rows = lat0_bp + (np.arange(Nj_ncap + 1) + 1.0) * (90.0 - lat0_bp) / Nj_ncap   # top edge of each cell row
                guard_lat = math.degrees(math.acos(2.0 / math.sqrt(K)))
                fix_lat = math.degrees(math.acos(1.0 / math.sqrt(K)))
                # (With the cap's columns mirrored a guarded row costs 1.3 / 0.33 = 4 plain ones in arithmetic; weights of 3, 4 and 5 were
                # swept on the 8-way split of the 1/8 degree grid, one GPU: slowest rank 31.6 / 33.6 / 32.7 us against 31.7 with 1.3 and
                # the per-rank rebalancing step -- more ranks get guarded rows and each pays the fix-up launch.  1.3 stays.)
                w = [float(v) for v in os.environ.get("OGG_BP_ROW_COST", "1.3,1.3,0").split(",")]
                w_fix, w_guard, lump = w[0], w[1], (w[2] if len(w) > 2 else 0.0)
                bp.row_cost = np.where(lat_rows >= fix_lat, w_fix, np.where(lat_rows >= guard_lat, w_guard, 1.0))
                bp.row_cost[-1] += lump   # the tail launch (fix-up + j = ny row) only the top band runs, in plain-row equivalents
        # ---- Southern Ocean (OGG:1080-1103); like the reference this needs the Mercator sub-grid
        lat0_SO = -78.0
        if south_ocean_lower_lat > -90:
            lat0_SO = south_ocean_lower_lat
        if phi_kept is None:
            raise Exception("the Southern Ocean and southern cap sections read the Mercator sub-grid (OGG:1083): add mercator to --grids")
        latUp_SO = float(phi_kept[0])
        lenlat_SO = latUp_SO - lat0_SO
        Nj_SO = int(refineR * 55)
        if refineR == 2 and enhanced_equatorial:
            Nj_SO = 109
        if refineR == 1 and enhanced_equatorial:
            Nj_SO = 0
        if "so" in match_dy:
            Nj_SO = int(0.5 + lenlat_SO / dphi_so)
        skipS = 0
        if Nj_SO != 0 and want("so"):
            skipS = 1 if ((Nj_SO + 1) % 2 == 0 and ensure_nj_even) else 0
            so = SubGridPlan("SO", "latlon", Nj_SO + 1 - skipS, row0=skipS, lnj=Nj_SO, lat0=lat0_SO, lenlat=lenlat_SO)
        # ---- southern cap (OGG:1122-1197)
        if so is None:
            raise Exception("the southern cap section reads the Southern Ocean sub-grid (OGG:1122): it cannot be left out")
        lat0_SC = lat0_SO + (skipS * lenlat_SO) / float(Nj_SO) if skipS else lat0_SO        # phiSO[0, Ni//4]
        if "p125sc" in match_dy:
            lat0_SC = lat0_SO
        Nj_scap = int(refineR * 40) * 7 // 4
        if no_south_cap or (enhanced_equatorial and refineR in (1, 2)):
            Nj_scap = 0
        if Nj_scap != 0 and want("sc"):
            if r_dp == 0.0 and lat_dp <= -90.0:
                Nj_scap = int((lat0_SC + 90.0) / (1.0 / refineR / refineS))
                skipC = 1 if ((Nj_scap + 1) % 2 == 0 and ensure_nj_even) else 0
                sc = SubGridPlan("SC", "latlon", Nj_scap + 1 - skipC, row0=skipC, lnj=Nj_scap, lat0=-90.0, lenlat=90 + lat0_SO)
            else:
                if lat_dp > -90:
                    r_dp = float(np.tan((90 + lat_dp) * ogg.PI_180) / np.tan((90 + lat0_SC) * ogg.PI_180))
                jmint = 0
                if doughnut != 0.0:
                    jmin = np.ceil(doughnut * Nj_scap)
                    jmint = int(jmin + np.mod(jmin, 2))
                if (Nj_scap + 1 - jmint) % 2 == 0 and ensure_nj_even:
                    jmint += 1
                sc = SubGridPlan("SC", "dpole", Nj_scap + 1 - jmint, row0=jmint, Nj=Nj_scap, lat0=lat0_SC, lon_dp=lon_dp, r_dp=r_dp)
        self.Nj_scap = Nj_scap
        self.lat0_SO, self.latUp_SO = lat0_SO, latUp_SO
        self.subs = [s for s in (sc, so, merc, bp) if s is not None]  # south -> north
        if bp is not None and not skip_metrics:
            # the last rank's fix-up launch against a single-GPU pass of this grid (1.08e11 cells/s measured at 1/8 degree): see rows_of
            import os
            # measured (events, top rank of 8): 6.5 us at 1/8 degree, 17 us at 1/16 degree -- a launch plus the literal re-evaluation of the
            # guarded cells, whose number grows with the square of the resolution
            tail_us = float(os.environ.get("OGG_TOP_RANK_TAIL_US", "%.3f" % (2.9 + 0.0563 * refineR * refineR)))
            cells = sum(s.nj1 - 1 for s in self.subs) * Ni
            pass_us = cells / 1.08e5
            if sc is not None and sc.kind == "dpole":   # + the displaced-pole quadrature: 0.66 ns per cell literal (launch D), 0.10 ns chord
                pass_us += (sc.nj1 - 1) * Ni * (6.6e-4 if self.dp_arc == L.DP_ARC_LITERAL else 1.0e-4)
            self.set_split_times(tail_us, pass_us, "fitted constants (builder boxes, rounds 2-3): UNVALIDATED on a multi-GPU node; "
                                 "calibrate_split() replaces them by this box's own timings")
        # Rows that --south_cutoff_row / _ang remove from the stitched grid (OGG:1268-1313) are not generated when the cut is known from the
        # sizes alone -- by row always; by angle on a regular cap, whose latitudes are an axis formula -- just as the doughnut rows are not
        # (OM4: 82 of the displaced-pole cap's 143 kept rows).  The cut of a displaced-pole cap by ANGLE needs the cap's latitudes and is
        # applied after the pass (south_cut(sc_y0) / Supergrid.south_cut()).
        self.cut_applied = None
        by_angle_later = south_cutoff_row <= 0 and south_cutoff_ang > -90 and sc is not None and sc.kind != "latlon"
        if (south_cutoff_row > 0 or south_cutoff_ang > -90) and not by_angle_later:
            c_sc, c_so, gone = self.south_cut()
            if gone:
                self.subs = [s for s in self.subs if s.name != "SC"]
                so.row0, so.nj1 = so.row0 + min(c_so, so.nj1), max(so.nj1 - c_so, 0)
                if so.nj1 == 0:      # a cut beyond the Southern Ocean piece: nothing of it is stitched (its [jcut:] slice is empty)
                    self.subs = [s for s in self.subs if s.name != "SO"]
            elif c_sc > 0:
                sc.row0, sc.nj1 = sc.row0 + c_sc, sc.nj1 - c_sc
            self.cut_applied = (c_sc, c_so, gone)

    split_times = None

    def set_split_times(self, tail_us, pass_us, source, top_capacity=None, rank_capacity=None):
        """What the band split takes the last rank's share from (rows_of).  The MODEL: `tail_us`, what the bipolar quadrature's fix-up
        launch -- which only the rank with the top rows runs -- adds to that rank's pass, and `pass_us`, one pass of the whole grid on
        one GPU: share of the last rank = 1 - world * tail_us / pass_us of the others'.  A MEASURED share (`top_capacity`, from
        calibrate_split) takes precedence for the world size it was measured at.  The same values on every rank give the same edges."""
        for s in self.subs:
            s.tail_us, s.pass_us, s.top_capacity, s.rank_capacity = float(tail_us), float(pass_us), top_capacity, rank_capacity
        self.split_times = {"tail_us": float(tail_us), "pass_us": float(pass_us), "source": source}
        if top_capacity is not None:
            self.split_times["top_capacity"] = {"world": int(top_capacity[0]), "share_of_last_rank": float(top_capacity[1])}
        if rank_capacity is not None:   # (refine_split: one relative share per rank; takes precedence for its world size)
            self.split_times["rank_capacity"] = {"world": int(rank_capacity[0]), "shares": [float(v) for v in rank_capacity[1]]}

    def calibrate_split(self, device, rank=0, world=1, passes=40, broadcast=True, force=False, rounds=5):
        """Replace the fitted split constants by a measurement on THIS box, before any band buffer exists (rank 0 alone works, about a
        thousand passes; the others wait in the broadcast).  Rank 0 (i) runs the whole grid as one rank -- `passes` timed passes after
        100 warm ones: pass_us; eight more with the library's launch events: the fix-up launch less the cost of an event record, a first
        guess of tail_us and hence of the last rank's share c = 1 - world * tail_us / pass_us --, then (ii) up to `rounds` times (until the two agree to 1 %): times the share
        of a middle rank and of the last rank under the current split (on its one GPU, one after the other) and scales
        c <- c * T_middle / T_last, which equalises the two whatever makes the last rank slower (a fixed extra launch, or rows that cost
        more than the row weights say on this box); the share of the round whose slower rank was fastest is kept; and (iii) broadcasts (tail_us, pass_us, c).  Every rank then derives the same edges.
        Needs a GPU on rank 0 and, for world > 1 with ``broadcast``, an initialised process group.  Returns ``split_times`` (None when
        the split has no such term: one rank, no bipolar cap, --skip_metrics).  OGG_TOP_RANK_TAIL_US in the environment pins the
        model's tail time and skips (ii).  ``force``: measure and broadcast at world size 1 too (bench.py under OGG_FORCE_DIST=1: the
        RCCL broadcast on a one-GPU box)."""
        import os
        import time
        if (world <= 1 and not force) or self.split_times is None:
            return self.split_times
        vals = (0.0, 0.0, 0.0)
        if rank == 0:
            import torch

            def timed_us(g, warm, n):
                for _ in range(warm):
                    g.run_pass()
                torch.cuda.synchronize(g.device)
                t0 = time.perf_counter()
                for _ in range(n):
                    g.run_pass()
                torch.cuda.synchronize(g.device)
                return (time.perf_counter() - t0) / n * 1e6

            g = Supergrid(self, rank=0, world=1, device=device, halo="recompute")
            g.launch, g.overlap = "pass", False
            pass_us = timed_us(g, 100, passes)          # (the clocks of a fresh process take ~30 ms to ramp)
            g.reserve_pass_events(8)
            g.pass_events = []
            for _ in range(8):
                g.run_pass()
            tail_us = g.pass_launch_times_ms()["pass_tail"]["ms"] * 1e3
            g.pass_events = None
            # an interval between two event records holds the records' own cost besides the launch: two records back to back measure it
            st = g._stream()
            ev = g._new_events()
            gap = []
            for _ in range(8):
                L.call("ogg_event_record", ev[0], st)
                L.call("ogg_event_record", ev[1], st)
                L.call("ogg_stream_synchronize", st)
                ms = ctypes.c_float()
                L.call("ogg_event_elapsed_ms", ev[0], ev[1], ctypes.byref(ms))
                gap.append(ms.value * 1e3)
            for k in range(5):
                L.call("ogg_event_destroy", ev[k])
            g.close()
            del g
            tail_us = max(tail_us - min(gap), 1.0)
            cap = 0.0                                    # 0: no measured share (the model stands)
            if os.environ.get("OGG_TOP_RANK_TAIL_US"):
                tail_us = float(os.environ["OGG_TOP_RANK_TAIL_US"])
            elif world > 1:
                cap = 1.0 - world * tail_us / pass_us if world * tail_us / pass_us <= 0.5 else 1.0
                tried = []                               # (slower of the two shares, share of the last rank) of every round
                for _ in range(rounds):
                    self.set_split_times(tail_us, pass_us, "calibrating", top_capacity=(world, cap))
                    t = []
                    for r in ((world - 1) // 2, world - 1):
                        h = Supergrid(self, rank=r, world=world, device=device, halo="recompute")
                        h.launch, h.overlap = "pass", False
                        t.append(timed_us(h, 60, 150))
                        h.close()
                        del h
                    tried.append((max(t), cap))
                    if abs(t[0] / t[1] - 1.0) < 0.01:      # the two shares within 1 %: balanced as far as a timing can tell
                        break
                    cap = min(max(cap * t[0] / t[1], 0.3), 1.3)
                # the split whose slower share was fastest: a share's time is not always monotone in its size (tiling thresholds of the
                # pass, the write path of some boxes), and then the last step of the iteration need not be its best
                cap = min(tried)[1]
            torch.cuda.empty_cache()
            vals = (tail_us, pass_us, cap)
        if broadcast:   # three doubles from rank 0: a device tensor over RCCL, through the host where the group is gloo (as all_reduce does)
            import torch
            import torch.distributed as dist
            on_gpu = dist.get_backend() != "gloo"
            t = torch.tensor(list(vals), dtype=torch.float64, device=(device if on_gpu else "cpu"))
            dist.broadcast(t, src=0)
            vals = tuple(float(v) for v in t.tolist())
        tail_us, pass_us, cap = vals
        self.set_split_times(tail_us, pass_us, "measured by rank 0 at plan build (whole grid: %d passes + launch events of 8 more; then the shares "
                             "of a middle and of the last rank under the split, until they agree to 1 %% or %d times)" % (passes, rounds),
                             top_capacity=((world, cap) if cap > 0.0 else None))
        return self.split_times

    def refine_split(self, per_rank_us, world, deadband=0.03):
        """One rebalancing step from what every rank measured on its OWN GPU under the current split, all ranks running at once (the
        conditions of the job: calibrate_split times the shares one after the other on rank 0's idle chip).  ``per_rank_us``: every
        rank's time per pass in rank order -- the same list on every rank (bench.py all-gathers it), so every rank derives the same new
        edges and nothing is broadcast.  Every rank's share is scaled by mean(T) / T_rank (a rank whose rows cost more than the cost
        model says -- the rows next to the guarded ones, a GPU of the slower write-path class -- gets fewer); inside the ``deadband``
        (every rank within 3 % of the mean: a timing cannot tell) the split stays.  Returns True when the split changed (band buffers
        must be rebuilt).  The measured times and the shares before and after are recorded in ``split_times["self_calibration"]``."""
        if world <= 1 or self.split_times is None or len(per_rank_us) != world:
            return False
        t = [float(v) for v in per_rank_us]
        if min(t) <= 0.0:
            return False
        caps_old = self.rank_capacities(world)
        mean = sum(t) / world
        worst = max(abs(v / mean - 1.0) for v in t)
        rec = {"world": world, "per_rank_us": [round(v, 3) for v in t], "shares_before": [round(c, 5) for c in caps_old],
               "share_of_last_rank_before": caps_old[-1] / caps_old[0], "others_over_last": (sum(t[:-1]) / (world - 1)) / t[-1],
               "largest_deviation_from_mean": worst}
        changed = worst > deadband
        caps_new = caps_old
        if changed:
            caps_new = [min(max(c * mean / v, 0.3 * c), 1.5 * c) for c, v in zip(caps_old, t)]
            norm = caps_new[0]
            caps_new = [c / norm for c in caps_new]     # (relative shares: rank 0 = 1, as before)
        rec["shares_after"] = [round(c, 5) for c in caps_new]
        rec["share_of_last_rank_after"] = caps_new[-1] / caps_new[0]
        hist = list(self.split_times.get("self_calibration", []))
        self.set_split_times(self.split_times["tail_us"], self.split_times["pass_us"], self.split_times["source"],
                             top_capacity=(world, caps_new[-1] / caps_new[0]), rank_capacity=((world, caps_new) if changed else self._rank_capacity()))
        self.split_times["self_calibration"] = hist + [rec]
        return changed

    def _rank_capacity(self):
        return getattr(self.subs[0], "rank_capacity", None)

    def rank_capacities(self, world):
        """Relative shares of the ranks under the current split (rank 0 = 1 unless refine_split has set them)."""
        s0 = self.subs[0]
        rc = getattr(s0, "rank_capacity", None)
        if rc is not None and int(rc[0]) == world:
            return [float(v) for v in rc[1]]
        old = getattr(s0, "top_capacity", None)
        if old is not None and int(old[0]) == world:
            cap = float(old[1])
        else:
            tail, whole = self.split_times["tail_us"], self.split_times["pass_us"]
            cap = min(1.0, 1.0 - world * tail / whole) if (whole > 0 and world * tail / whole <= 0.5) else 1.0
        return [1.0] * (world - 1) + [cap]

    def south_cut(self, sc_y0=None):
        """(rows cut from the southern cap, rows cut from the Southern Ocean piece, cap removed) by --south_cutoff_row / _ang,
        OGG:1268-1313, including the parity bumps of --ensure_nj_even.  ``sc_y0``: column 0 of the cap's latitudes, needed for
        --south_cutoff_ang only.  (0, 0, False) once the plan has applied the cut to its own sub-grid sizes (``cut_applied``)."""
        if getattr(self, "cut_applied", None) is not None:
            return 0, 0, False
        first = self.subs[0]
        has_sc = first.name == "SC"
        n_sc = first.nj1 if has_sc else 0
        if self.south_cutoff_row > 0:
            jcut = self.south_cutoff_row - 1
        elif self.south_cutoff_ang > -90:
            if not has_sc:
                raise Exception("--south_cutoff_ang reads the southern cap's latitudes (OGG:1278): there is no southern cap")
            if sc_y0 is None:
                if first.kind != "latlon":
                    raise ValueError("south_cut: the cap's latitudes are needed for --south_cutoff_ang")
                sc_y0 = first.lat0 + (np.arange(first.row0, first.row0 + first.nj1) * first.lenlat) / float(first.lnj)
            jcut = 1 + int(np.nonzero(np.asarray(sc_y0) < self.south_cutoff_ang)[0][-1])
        else:
            return 0, 0, False
        if has_sc and jcut < n_sc:
            if (n_sc - jcut) % 2 == 0 and self.ensure_nj_even:
                jcut += 1
            return jcut, 0, False
        so = next((s for s in self.subs if s.name == "SO"), None)
        if so is None:
            return 0, 0, False
        if not has_sc:
            raise Exception("--south_cutoff_row without a southern cap: the reference reads lamSC here (OGG:1299)")
        jcut_so = jcut - n_sc
        if (so.nj1 - 1 - jcut_so - 1) % 2 == 0 and self.ensure_nj_even:
            jcut_so += 1
        return n_sc, jcut_so, True

    def rows_cut(self, sc_y0=None):
        """Rows removed at the south end of the stitched grid (stitching drops the cap's last row, so a cap that is cut away
        altogether takes nj1 - 1 stitched rows with it)."""
        c_sc, c_so, gone = self.south_cut(sc_y0)
        if not gone:
            return c_sc
        so = next(s for s in self.subs if s.name == "SO")
        return self.subs[0].nj1 - 1 + min(c_so, so.nj1 - 1)   # a cut beyond the Southern Ocean piece leaves none of its rows (OGG:1306-1311)

    @property
    def nyp(self):
        return sum(s.nj1 - 1 for s in self.subs) + 1 - self.rows_cut()

    @property
    def cells(self):
        """cells of the final stitched grid (the unit of BASELINE.json's metric): (nyp-1)*Ni"""
        return (self.nyp - 1) * self.Ni


class Supergrid(object):
    """Band-sharded device pass.  `halo` is "rccl" (neighbour send/recv through torch.distributed; needs an initialised
    process group when world > 1), "local" (world virtual ranks inside ONE process: the neighbour's row is copied
    device-to-device; used to test the band logic on a single GPU) or "recompute" (the halo row of a lat-lon sub-grid is
    re-tiled from the 1-D axis every rank already holds; bitwise identical)."""

    def __init__(self, plan, rank=0, world=1, device="cuda:0", halo="rccl", peers=None, latlon="fused"):
        """``latlon``: how the sub-grids that are lat-lon by construction (Mercator, Southern Ocean, regular southern
        cap) are produced.  "fused" (default): one kernel writes all six fields from the two 1-D axes -- 48 B written per
        cell, nothing read, and no halo (every rank holds the whole 1-D axis).  "stencil": tile x, y; exchange the halo
        row; run the generic 2x3-stencil kernel that reads x, y back -- the kernel the drop-in functions use for arbitrary
        meshes.  Both give the same bits."""
        import torch

        self.torch = torch
        self.plan, self.rank, self.world, self.halo, self.latlon = plan, rank, world, halo, latlon
        self.device = torch.device(device)
        self.peers = peers  # halo="local": list of all virtual ranks' Supergrid objects
        self.overlap = True
        # "pass": lat-lon sub-grids + bipolar cap through ogg_tripolar_pass_dev (three launches on one stream, the two kinds
        # of work sharing each launch); "kernels": one call per sub-grid and phase, on side streams when `overlap` is set
        self.launch = "pass" if latlon == "fused" else "kernels"
        self.pass_events = None  # a list: tripolar_pass() times its launches into it
        self._event_pool = []
        self._pass_args = None
        self._rows_ws = None
        self._side = None
        self.buf = {}
        self.timings = {}
        ni1 = plan.Ni + 1
        # device "cpu" allocates the same band buffers in host memory: only the partition and the halo exchange can
        # run there (tests over gloo); the phases need a GPU
        import contextlib
        with (torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()):
            self.lon1d = torch.empty(ni1, dtype=torch.float64, device=self.device)
            # Where the output arrays lie moves a write-bound pass by +-6 %: allocated one by one, the fields of a band land wherever the
            # allocator puts them, and the 1/8 degree pass runs 0.185 or 0.21 ms by the draw (four grids in one process: 0.185 / 0.207 /
            # 0.187 / 0.210; 1/16 degree 0.91 / 1.07).  OGG_FIELD_SLAB=<bytes> (experiment) takes the fields of all bands from ONE
            # allocation, every field at a multiple of that many bytes: 2 GiB apart all four grids ran 0.184-0.186 on one box and one of
            # two on another; 256 B ... 1 GiB apart no better than the draw (scripts/split_pass_probe.py --copies 4,
            # profiles/r05_split_pass_probe.md).  Not understood, so not a default: one allocation per field.
            def field_shapes():
                for s in plan.subs:
                    lo, hi = self.rows_of(s, rank, world)
                    n = hi - lo
                    n_cell = max(min(hi, s.nj1 - 1) - lo, 0)
                    halo = 1 if (latlon == "stencil" and s.kind in ("mercator", "latlon") and n_cell > 0 and hi < s.nj1) else 0
                    for r, c in ((n + halo, ni1), (n + halo, ni1), (n, ni1 - 1), (n_cell, ni1), (n_cell, ni1 - 1), (n, ni1)):
                        yield max(r, 0) * c * 8

            slab, slab_off, slab_align = None, 0, 0
            if self.device.type == "cuda":
                forced = os.environ.get("OGG_FIELD_SLAB")
                sizes = list(field_shapes())
                if forced is not None:
                    slab_align = int(forced)
                if slab_align > 0:
                    total = sum((b + slab_align - 1) // slab_align * slab_align for b in sizes) + slab_align
                    try:
                        free_bytes = torch.cuda.mem_get_info(self.device)[0]
                    except Exception:  # noqa: BLE001 -- no memory information: no slab
                        free_bytes = 0
                    if total > free_bytes * 9 // 10:   # (several grids in one process: the later ones fall back)
                        slab_align = 0
                    else:
                        slab = torch.empty(total, dtype=torch.uint8, device=self.device)
                        slab_off = (-slab.data_ptr()) % slab_align
                        self._slab = slab
            self.field_slab = {"spacing_bytes": slab_align, "bytes": int(slab.numel()) if slab is not None else 0}

            def field_buffer(r, c):
                nonlocal slab_off
                if slab is None:
                    return torch.empty((max(r, 0), c), dtype=torch.float64, device=self.device)
                nbytes = max(r, 0) * c * 8
                t = slab[slab_off:slab_off + nbytes].view(torch.float64).view(max(r, 0), c)
                slab_off += (nbytes + slab_align - 1) // slab_align * slab_align
                return t

            for s in plan.subs:
                lo, hi = self.rows_of(s, rank, world)
                n = hi - lo
                n_cell = min(hi, s.nj1 - 1) - lo  # cell rows owned (a cell row j belongs to the owner of point row j)
                needs_halo = latlon == "stencil" and s.kind in ("mercator", "latlon") and n_cell > 0 and hi < s.nj1
                b = {"lo": lo, "hi": hi, "n": n, "n_cell": max(n_cell, 0), "needs_halo": needs_halo}
                rows_xy = n + (1 if needs_halo else 0)
                for f, (r, c) in (("x", (rows_xy, ni1)), ("y", (rows_xy, ni1)), ("dx", (n, ni1 - 1)), ("dy", (b["n_cell"], ni1)),
                                  ("area", (b["n_cell"], ni1 - 1)), ("angle_dx", (n, ni1))):
                    b[f] = field_buffer(r, c)
                if s.kind == "mercator":
                    if getattr(s, "explicit_axis", None) is not None:   # enhanced-equator axis: spliced on the host (OGG:349-428)
                        b["axis"] = torch.from_numpy(s.explicit_axis).to(self.device)
                    else:
                        b["axis"] = torch.empty(s.n_axis, dtype=torch.float64, device=self.device)
                elif s.kind == "latlon":
                    b["axis"] = torch.empty(s.lnj + 1, dtype=torch.float64, device=self.device)
                elif s.kind == "bipolar":
                    b["ws_bytes"] = int(L.load().ogg_bipolar_quad_workspace_bytes(5, plan.Ni, s.Nj))
                    b["ws"] = torch.empty(b["ws_bytes"], dtype=torch.uint8, device=self.device)
                elif s.kind == "dpole":   # one workspace for the pass (mesh words + quadrature tables and words); the stand-alone
                    b["ws_bytes"] = int(L.load().ogg_dpole_band_workspace_bytes(4, plan.Ni, n))   # kernels use its two parts
                    b["ws"] = torch.zeros(max(b["ws_bytes"], 16), dtype=torch.uint8, device=self.device)
                    b["ws_mesh_bytes"] = (int(L.load().ogg_displaced_pole_grid_workspace_bytes(plan.Ni, n)) + 255) // 256 * 256
                self.buf[s.name] = b

    @staticmethod
    def rows_of(s, rank, world):
        """Point rows [lo, hi) of sub-grid `s` owned by `rank`: equal row counts, or equal cost where rows differ in cost; the
        last rank's share of every sub-grid is smaller by what the fix-up launch costs it (SubGridPlan.tail_us / pass_us, set by
        SupergridPlan when the grid has a bipolar cap with metrics)."""
        cost = getattr(s, "row_cost", None)
        tail_us, pass_us = getattr(s, "tail_us", 0.0), getattr(s, "pass_us", 0.0)
        measured = getattr(s, "top_capacity", None)
        per_rank = getattr(s, "rank_capacity", None)
        if world > 1 and per_rank is not None and int(per_rank[0]) == world:   # every rank's share as refine_split rebalanced them
            return band_weighted(np.ones(s.nj1) if cost is None else cost, rank, world, capacities=per_rank[1])
        cap = 1.0
        if world > 1 and measured is not None and int(measured[0]) == world:
            cap = float(measured[1])        # the last rank's share as calibrate_split measured it for this world size
        # (a grid so small, or ranks so many, that the fix-up launch is more than half of a rank's share: the linear correction no longer
        # describes anything -- equal shares then, rather than a last rank clamped to a sliver or to no rows at all)
        elif world > 1 and tail_us > 0.0 and pass_us > 0.0 and world * tail_us / pass_us <= 0.5:
            cap = min(1.0, 1.0 - world * tail_us / pass_us)
        if cost is None and cap == 1.0:
            return band(s.nj1, rank, world)
        return band_weighted(np.ones(s.nj1) if cost is None else cost, rank, world, cap)

    # -- helpers ---------------------------------------------------------------------------------------------
    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("the supergrid phases run on a GPU only (there is no CPU compute path)")
        return self.torch.cuda.current_stream(self.device).cuda_stream

    @staticmethod
    def _p(t, row=0):
        return t.data_ptr() + row * t.stride(0) * 8 if t.dim() == 2 else t.data_ptr() + row * 8

    def _timed(self, key, fn):
        """Run fn() bracketed by events on the launch stream when per-kernel timing is on."""
        if self._events is None:
            fn()
            return
        e0 = self.torch.cuda.Event(enable_timing=True)
        e1 = self.torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self._events.setdefault(key, []).append((e0, e1))

    _events = None

    # -- phases ----------------------------------------------------------------------------------------------
    @staticmethod
    def _selected(s, only, kinds):
        return (only is None or s.name == only) and (kinds is None or s.kind in kinds)

    def _latlon_bands(self, only=None, kinds=None):
        """ogg_latlon_band descriptors of this rank's lat-lon sub-grid bands."""
        bands = []
        for s in self.plan.subs:
            b = self.buf[s.name]
            if b["n"] == 0 or not self._selected(s, only, kinds) or s.kind not in ("mercator", "latlon"):
                continue
            band = L.LatlonBand()
            if s.kind == "mercator" and getattr(s, "explicit_axis", None) is not None:
                band.axis_kind, band.lat1d = 2, b["axis"].data_ptr()
            elif s.kind == "mercator":
                band.axis_kind, band.y0 = 1, s.y0
            else:
                band.axis_kind, band.a0, band.len, band.denom = 0, s.lat0, s.lenlat, float(s.lnj)
            band.k0, band.n_pt_rows, band.n_cell_rows = s.row0 + b["lo"], b["n"], b["n_cell"]
            band.x, band.y, band.angle = b["x"].data_ptr(), b["y"].data_ptr(), b["angle_dx"].data_ptr()
            band.dx = b["dx"].data_ptr()
            band.dy = b["dy"].data_ptr() if b["n_cell"] else None
            band.area = b["area"].data_ptr() if b["n_cell"] else None
            bands.append(band)
        return bands

    def tripolar_pass(self):
        """Lat-lon sub-grids and both caps of this rank through ogg_supergrid_pass_dev."""
        p, st = self.plan, self._stream()
        if self._pass_args is None:  # the descriptors only hold scalars and buffer addresses, which never change: build once
            bands = self._latlon_bands()
            arr = (L.LatlonBand * max(len(bands), 1))(*bands)
            cap = scap = None
            for s in p.subs:
                b = self.buf[s.name]
                if s.kind == "bipolar" and b["n"] > 0:
                    cap = L.BipolarBand()
                    cap.Ni, cap.Nj, cap.lat0_bp, cap.lon_bp, cap.rp, cap.Re, cap.order = p.Ni, s.Nj, s.lat0_bp, s.lon_bp, s.rp, p.Re, 5
                    cap.symmetry = p.cap_symmetry
                    cap.j0, cap.n_pt_rows, cap.n_cell_rows = b["lo"], b["n"], b["n_cell"]
                    cap.x, cap.y, cap.angle = b["x"].data_ptr(), b["y"].data_ptr(), b["angle_dx"].data_ptr()
                    cap.dx = b["dx"].data_ptr()
                    cap.dy = b["dy"].data_ptr() if b["n_cell"] else None
                    cap.area = b["area"].data_ptr() if b["n_cell"] else None
                    cap.workspace, cap.workspace_bytes = b["ws"].data_ptr(), b["ws_bytes"]
                elif s.kind == "dpole" and b["n"] > 0:
                    scap = L.DpoleBand()
                    scap.Ni, scap.Nj, scap.lon0, scap.lat0, scap.lon_dp, scap.r_dp, scap.Re = p.Ni, s.Nj, p.lon0, s.lat0, s.lon_dp, s.r_dp, p.Re
                    scap.order, scap.arc_form, scap.symmetry = 4, p.dp_arc, p.cap_symmetry
                    scap.j0, scap.n_pt_rows, scap.n_cell_rows = s.row0 + b["lo"], b["n"], b["n_cell"]
                    scap.x, scap.y, scap.angle = b["x"].data_ptr(), b["y"].data_ptr(), b["angle_dx"].data_ptr()
                    scap.dx = b["dx"].data_ptr()
                    scap.dy = b["dy"].data_ptr() if b["n_cell"] else None
                    scap.area = b["area"].data_ptr() if b["n_cell"] else None
                    scap.workspace, scap.workspace_bytes = b["ws"].data_ptr(), b["ws_bytes"]
            # ... and so is the plan of the launches (kernel parameters, grid sizes, tiling knobs read from the environment NOW):
            # a pass then costs the host one ctypes call and the launches
            capref = ctypes.byref(cap) if cap is not None else None
            scapref = ctypes.byref(scap) if scap is not None else None
            handle = ctypes.c_void_p()
            L.call("ogg_supergrid_pass_plan_dev", len(bands), arr, p.Ni + 1, p.lon0, p.lenlon, p.Re, 0 if p.skip_metrics else 1, capref, scapref,
                   ctypes.byref(handle))
            self._pass_args = (bands, arr, cap, scap, handle)
            self._pass_run = L.load().ogg_supergrid_pass_run_dev
        handle = self._pass_args[4]
        if self.pass_events is None:
            rc = self._pass_run(handle, None, None, st)
            if rc:
                L.check(rc)
            return
        # per-launch timing: five HIP events recorded by the library around its (up to) four launches
        evs = self._event_pool.pop() if self._event_pool else self._new_events()
        self.pass_bytes = (ctypes.c_double * 4)()
        L.call("ogg_supergrid_pass_run_dev", handle, evs, self.pass_bytes, st)
        self.pass_events.append(evs)

    def pass_plan_info(self):
        """(workspace slots of the fused pass's plan, passes so far that started with launch B because the previous pass's launch B had
        built their tables) -- (0, 0) before the first pass."""
        if self._pass_args is None:
            return 0, 0
        lib = L.load()
        return int(lib.ogg_supergrid_pass_plan_slots(self._pass_args[4])), int(lib.ogg_supergrid_pass_plan_carried_runs(self._pass_args[4]))

    def replan(self):
        """Drop the cached plan of the pass (rebuilt by the next pass: after a change of an OGG_* tiling knob in the environment)."""
        if self._pass_args is not None:
            L.call("ogg_supergrid_pass_plan_destroy", self._pass_args[4])
            self._pass_args = None

    def close(self):
        """Release the plan of the pass (its workspace slots are device allocations of the library) at a point of the caller's choosing
        rather than at garbage-collection time."""
        self.replan()

    def __del__(self):
        try:
            self.replan()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass

    @staticmethod
    def _new_events():
        evs = (ctypes.c_void_p * 5)()
        for k in range(5):
            e = ctypes.c_void_p()
            L.call("ogg_event_create", ctypes.byref(e))
            evs[k] = e
        return evs

    def reserve_pass_events(self, n):
        """Create the events for n timed passes ahead of a timed region."""
        self._event_pool = [self._new_events() for _ in range(n)]

    def pass_launch_times_ms(self):
        """Mean duration and algorithmic bytes of the four launches of the fused pass (the fourth exists only with a displaced-pole
        cap in the literal arc form) over the passes that ran while `pass_events` was a list; empties the list."""
        L.call("ogg_stream_synchronize", self._stream())
        tot = [0.0, 0.0, 0.0, 0.0]
        n = len(self.pass_events)
        for evs in self.pass_events:
            for k in range(4):
                ms = ctypes.c_float()
                L.call("ogg_event_elapsed_ms", evs[k], evs[k + 1], ctypes.byref(ms))
                tot[k] += ms.value
            for k in range(5):
                L.call("ogg_event_destroy", evs[k])
        self.pass_events = []
        by = list(self.pass_bytes) if n else [0.0, 0.0, 0.0, 0.0]
        out = {name: {"ms": tot[k] / max(n, 1), "alg_bytes": by[k]} for k, name in enumerate(("pass_a", "pass_b", "pass_tail", "pass_dpquad"))}
        out["sampled_passes"] = n
        return out

    def phase_a(self, only=None, kinds=None):
        """Coordinates of this rank's bands (optionally of one sub-grid / of some kinds of sub-grid only)."""
        p, st = self.plan, self._stream()
        ni1 = p.Ni + 1
        if only is None and self.latlon != "fused":
            L.call("ogg_linear_axis_dev", ni1, p.lon0, p.lenlon, float(p.Ni), self.lon1d.data_ptr(), st)
        if self.latlon == "fused":
            bands = self._latlon_bands(only, kinds)
            if bands:
                import os
                arr = (L.LatlonBand * len(bands))(*bands)
                if os.environ.get("OGG_LATLON_ROWS", "0") != "0":
                    # a launch with nothing but lat-lon sub-grids: (field, row)-ordered workgroups fed from row / column tables (an
                    # option: same bits, and within 4 % of the column-tile kernel either way on the same box)
                    need = int(L.load().ogg_latlon_rows_workspace_bytes(len(bands), arr, ni1))
                    if self._rows_ws is None or self._rows_ws.numel() < need:
                        self._rows_ws = self.torch.empty(need, dtype=self.torch.uint8, device=self.device)
                    ws = self._rows_ws
                    self._timed("latlon_fused", lambda: L.call("ogg_latlon_supergrid_rows_ws_dev", len(bands), arr, ni1, p.lon0, p.lenlon,
                                                               p.Re, 0 if p.skip_metrics else 1, ws.data_ptr(), ws.numel(), st))
                else:
                    self._timed("latlon_fused", lambda: L.call("ogg_latlon_supergrid_multi_dev", len(bands), arr, ni1, p.lon0, p.lenlon,
                                                               p.Re, 0 if p.skip_metrics else 1, st))
        for s in p.subs:
            b = self.buf[s.name]
            if b["n"] == 0 or not self._selected(s, only, kinds):
                continue
            if s.kind in ("mercator", "latlon"):
                if self.latlon == "fused":
                    continue
                if s.kind == "mercator":
                    if getattr(s, "explicit_axis", None) is None:
                        L.call("ogg_mercator_axis_dev", p.Ni, s.y0, s.n_axis, b["axis"].data_ptr(), st)
                else:
                    L.call("ogg_linear_axis_dev", s.lnj + 1, s.lat0, s.lenlat, float(s.lnj), b["axis"].data_ptr(), st)
                rows = b["n"] + (1 if (b["needs_halo"] and self.halo == "recompute") else 0)
                self._timed("tile_latlon", lambda: L.call("ogg_tile_latlon_dev", rows, ni1, self._p(b["axis"], s.row0 + b["lo"]),
                                                          self.lon1d.data_ptr(), b["x"].data_ptr(), b["y"].data_ptr(), st))
            elif s.kind == "bipolar":
                self._timed("bipolar_mesh", lambda: L.call("ogg_bipolar_cap_mesh_angle_sym_dev", p.Ni, s.Nj, s.lat0_bp, s.lon_bp, b["lo"], b["n"],
                                                           p.cap_symmetry, b["x"].data_ptr(), b["y"].data_ptr(), None, None,
                                                           b["angle_dx"].data_ptr(), st))
            elif s.kind == "dpole":   # mesh, unwrap and angle_dx in one launch (its look-back words: the head of the band's workspace)
                self._timed("dpole_mesh", lambda: L.call("ogg_displaced_pole_grid_angle_ws_dev", p.Ni, s.Nj, p.lon0, s.lat0, s.lon_dp, s.r_dp,
                                                         s.row0 + b["lo"], b["n"], b["x"].data_ptr(), b["y"].data_ptr(),
                                                         b["angle_dx"].data_ptr(), b["ws"].data_ptr(), b["ws_mesh_bytes"], st))

    def exchange_halo(self):
        """First x/y row of the band above -> halo row of this band (MIDAS sub-grids only)."""
        if self.world == 1 or self.halo == "recompute" or self.latlon == "fused":
            return
        torch = self.torch
        if self.halo == "local":
            for s in self.plan.subs:
                b = self.buf[s.name]
                if b["needs_halo"]:
                    up = self.peers[self.rank + 1].buf[s.name]
                    b["x"][b["n"]].copy_(up["x"][0])
                    b["y"][b["n"]].copy_(up["y"][0])
            return
        import torch.distributed as dist

        ops = []
        for s in self.plan.subs:
            if s.kind not in ("mercator", "latlon"):
                continue
            b = self.buf[s.name]
            if b["needs_halo"]:  # receive from the rank above
                ops.append(dist.P2POp(dist.irecv, b["x"][b["n"]], self.rank + 1))
                ops.append(dist.P2POp(dist.irecv, b["y"][b["n"]], self.rank + 1))
            # send my first row to the rank below if IT needs a halo: it does iff it owns cell rows and is not the top band
            if self.rank > 0 and b["n"] > 0:
                lo_b, hi_b = self.rows_of(s, self.rank - 1, self.world)
                if min(hi_b, s.nj1 - 1) - lo_b > 0 and hi_b < s.nj1:
                    ops.append(dist.P2POp(dist.isend, b["x"][0], self.rank - 1))
                    ops.append(dist.P2POp(dist.isend, b["y"][0], self.rank - 1))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()

    def phase_b(self, only=None, kinds=None):
        """Metrics and angle of this rank's bands."""
        p, st = self.plan, self._stream()
        ni1 = p.Ni + 1
        for s in p.subs:
            b = self.buf[s.name]
            if b["n"] == 0 or not self._selected(s, only, kinds):
                continue
            if p.skip_metrics:
                for f in ("dx", "dy", "area"):
                    L.call("ogg_fill_dev", b[f].numel(), -1.0, b[f].data_ptr(), st)
            if s.kind in ("mercator", "latlon") and self.latlon == "fused":
                continue  # all six fields were written in phase A
            if s.kind in ("mercator", "latlon"):
                rows_xy = b["x"].shape[0]
                if p.skip_metrics:
                    self._timed("angle_x", lambda: L.call("ogg_grid_metrics_midas_dev", rows_xy, ni1, b["x"].data_ptr(), b["y"].data_ptr(),
                                                          b["n"], 0, p.Re, 1, None, None, None, b["angle_dx"].data_ptr(), st))
                else:
                    self._timed("midas_angle", lambda: L.call("ogg_grid_metrics_midas_dev", rows_xy, ni1, b["x"].data_ptr(),
                                                              b["y"].data_ptr(), b["n"], b["n_cell"], p.Re, 1, b["dx"].data_ptr(),
                                                              b["dy"].data_ptr() if b["n_cell"] else None,
                                                              b["area"].data_ptr() if b["n_cell"] else None,
                                                              b["angle_dx"].data_ptr(), st))
            else:
                if not p.skip_metrics:
                    if s.kind == "bipolar":
                        self._timed("bipolar_quad", lambda: L.call("ogg_bipolar_cap_metrics_quad_sym_ws_dev", 5, p.Ni, s.Nj, s.lat0_bp,
                                                                   s.lon_bp, s.rp, p.Re, b["lo"], b["n"], b["n_cell"], p.cap_symmetry,
                                                                   b["dx"].data_ptr(), b["dy"].data_ptr(), b["area"].data_ptr(),
                                                                   b["ws"].data_ptr(), b["ws_bytes"], st))
                    else:
                        j0 = s.row0 + b["lo"]
                        self._timed("dpole_quad", lambda: L.call("ogg_displaced_pole_metrics_quad_form_sym_ws_dev", p.dp_arc, p.cap_symmetry, 4,
                                                                 p.Ni, s.Nj, p.lon0, s.lat0, s.lon_dp, s.r_dp, p.Re, j0, b["n"], b["n_cell"],
                                                                 b["dx"].data_ptr(), b["dy"].data_ptr() if b["n_cell"] else None,
                                                                 b["area"].data_ptr() if b["n_cell"] else None,
                                                                 b["ws"].data_ptr() + b["ws_mesh_bytes"],
                                                                 b["ws_bytes"] - b["ws_mesh_bytes"], st))

    def step(self, time_kernels=False):
        """One full pass of the hot path for this rank's bands; outputs stay in HBM."""
        self._events = {} if time_kernels else None
        self.run_pass()

    def run_pass(self):
        """Phases A and B.  launch == "pass": everything through ogg_supergrid_pass_dev, on the caller's stream.  launch == "kernels":
        one call per sub-grid and phase; with `overlap` the caps run on side streams next to the lat-lon sub-grids (the HBM-bound
        lat-lon kernel overlaps the VALU-bound quadratures) and everything joins back on the caller's stream before returning
        (under graph capture this becomes a forked graph)."""
        torch = self.torch
        if self.latlon == "fused" and self.launch == "pass":
            self.tripolar_pass()
            if self.plan.skip_metrics:
                self.phase_b()  # the -1 fill of OGG:1327-1329
            return
        if self.latlon != "fused" or self.device.type != "cuda" or not self.overlap:
            self.phase_a()
            self.exchange_halo()
            self.phase_b()
            return
        main = torch.cuda.current_stream(self.device)
        caps = [s for s in self.plan.subs if s.kind in ("bipolar", "dpole")]
        # independent pieces of work: mesh (+ angle) and quadrature of every cap, one stream each
        tasks = []
        for s in caps:  # the quadratures are the longest chains: enqueue them first
            tasks.append(lambda s=s: self.phase_b(only=s.name))
        for s in caps:
            tasks.append(lambda s=s: self.phase_a(only=s.name))
        if self._side is None or len(self._side) < len(tasks):
            self._side = [torch.cuda.Stream(self.device) for _ in tasks]
        fork = torch.cuda.Event()
        fork.record(main)
        joins = []
        for st, task in zip(self._side, tasks):
            st.wait_event(fork)
            with torch.cuda.stream(st):
                task()
                e = torch.cuda.Event()
                e.record(st)
                joins.append(e)
        self.phase_a(kinds=("mercator", "latlon"))
        self.phase_b(kinds=("mercator", "latlon"))
        for e in joins:
            main.wait_event(e)

    def capture(self):
        """Capture one pass (phases A and B) into a HIP graph; `replay()` then costs one graph launch instead of ~10 kernel
        launches from Python.  Not available when the pass contains an RCCL halo exchange (stencil mode, world > 1)."""
        torch = self.torch
        if self.world > 1 and self.latlon == "stencil" and self.halo == "rccl":
            raise RuntimeError("the RCCL halo exchange is not captured; use eager steps")
        self._events = None
        self.step()
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.run_pass()
        self.graph = g
        return g

    def replay(self):
        self.graph.replay()

    def kernel_times_ms(self):
        """Mean per-launch duration of each kernel over the events recorded since the last reset."""
        self.torch.cuda.synchronize(self.device)
        out = {}
        for k, evs in (self._events or {}).items():
            ts = [a.elapsed_time(b) for a, b in evs]
            out[k] = {"launches": len(ts), "total_ms": float(sum(ts)), "mean_ms": float(sum(ts) / len(ts))}
        return out

    # -- self-check --------------------------------------------------------------------------------------------
    def metrics_sums(self):
        """Device tensor (n_subs, 7): the five sums of ogg_metrics_sums_dev over this rank's band of every sub-grid, then the
        latitude of the sub-grid's first and of its last point row (each contributed by the one rank that owns that row)."""
        torch, p, st = self.torch, self.plan, self._stream()
        out = torch.zeros((len(p.subs), 7), dtype=torch.float64, device=self.device)
        for k, s in enumerate(p.subs):
            b = self.buf[s.name]
            if b["n"] == 0:
                continue
            first, last = b["lo"] == 0, b["hi"] == s.nj1
            col_a, col_b = ogg.metrics_error_columns(p.Ni, self._pole_column(s))
            L.call("ogg_metrics_sums_dev", b["n"], b["n_cell"], p.Ni, b["dx"].data_ptr(), b["dy"].data_ptr() if b["n_cell"] else None,
                   b["area"].data_ptr() if b["n_cell"] else None, col_a, col_b, int(first), int(last), out[k].data_ptr(), st)
            if first:
                out[k, 5].copy_(b["y"][0, 0])
            if last:
                out[k, 6].copy_(b["y"][b["n"] - 1, 0])
        return out

    def _pole_column(self, s):
        if s.kind != "dpole":
            return -999
        return int(self.plan.Ni * np.mod(s.lon_dp - self.plan.lon0, 360) / 360.0)   # OGG:1160 poles_i

    def metrics_error(self, sums=None):
        """The reference's CHECK_metrics lines (OGG:732-770) for every sub-grid of a band-sharded run: % errors of sum(area), of a
        meridian arc and of the parallel arc(s) against the sphere, from five sums per band taken on the device and ONE all-reduce
        (RCCL) of n_subs x 7 doubles over the ranks -- the only collective of the default pipeline.  Returns {sub-grid name:
        tuple as returned by the reference's metrics_error}.  ``sums``: precomputed metrics_sums() (tests)."""
        torch, p = self.torch, self.plan
        t = self.metrics_sums() if sums is None else sums
        if self.world > 1:
            if self.halo == "local":  # virtual ranks in one process
                if sums is None:
                    t = sum(g.metrics_sums() for g in self.peers if g is not self) + t
            else:
                all_reduce(t)
        v = t.cpu().numpy()
        out = {}
        for k, s in enumerate(p.subs):
            area, dy_a, dy_b, dx_first, dx_last, lat_first, lat_last = (float(x) for x in v[k])
            if s.kind == "bipolar":
                out[s.name] = ogg.metrics_error_from_sums(area, dy_a, dy_b, dx_first, dx_last, s.lat0_bp, 90.0, p.Re, bipolar=True)
            elif s.kind == "dpole":  # OGG:1161; with the doughnut rows skipped the area and dy sums are partial, as the reference warns
                e = ogg.metrics_error_from_sums(area, dy_a, dy_b, dx_first, dx_last, s.lat0, -90.0, p.Re,
                                                displaced_pole=self._pole_column(s))
                if s.row0 > 0:  # doughnut rows are not generated: area and meridian arc cannot be estimated (OGG:762-763 says so)
                    e = (float("nan"), float("nan"), e[2])
                out[s.name] = e
            elif s.name == "SC":     # regular southern cap, OGG:1146: (phiSC[-1, 0], phiSC[0, 0])
                out[s.name] = ogg.metrics_error_from_sums(area, dy_a, dy_b, dx_first, dx_last, lat_last, lat_first, p.Re)
            else:                    # Mercator, Southern Ocean: (phi[0, 0], phi[-1, 0])
                out[s.name] = ogg.metrics_error_from_sums(area, dy_a, dy_b, dx_first, dx_last, lat_first, lat_last, p.Re)
        return out

    # -- results ---------------------------------------------------------------------------------------------
    def check_lookback_flags(self):
        """Raise if a displaced-pole kernel of the last pass gave up waiting for a strip map (its results would be invalid; the wait
        is bounded so that a launch always drains -- never observed).  Synchronises the stream."""
        if self._pass_args is not None:   # the plan of the fused pass: the look-back words of BOTH its workspace slots
            flags = ctypes.c_int(0)
            L.call("ogg_supergrid_pass_plan_flags_dev", self._pass_args[4], ctypes.byref(flags), self._stream())
            if flags.value & 6:
                raise L.OggHipError(L.OGG_EHIP, "displaced-pole %s: a look-back wait timed out" % ("mesh" if flags.value & 2 else "quadrature"))
        for s in self.plan.subs:
            b = self.buf[s.name]
            if s.kind != "dpole" or b["n"] == 0:
                continue
            for off, what in ((0, "mesh"),) + (() if self.plan.skip_metrics else ((b["ws_mesh_bytes"], "quadrature"),)):
                flag = ctypes.c_int(0)
                L.call("ogg_workspace_error_flag_dev", b["ws"].data_ptr() + off, ctypes.byref(flag), self._stream())
                if flag.value != 0:
                    raise L.OggHipError(L.OGG_EHIP, "displaced-pole %s: a look-back wait timed out (flag %d)" % (what, flag.value))

    def south_cut(self):
        """plan.south_cut() with the cap's latitudes read from the device when --south_cutoff_ang needs them (world 1)."""
        first = self.plan.subs[0]
        y0 = None
        if first.name == "SC" and self.plan.south_cutoff_ang > -90 and self.plan.south_cutoff_row <= 0:
            assert self.world == 1
            y0 = self.buf["SC"]["y"][: self.buf["SC"]["n"], 0].cpu().numpy()
        return self.plan.south_cut(y0)

    def _pieces(self, cut, point_rows):
        """This rank's pieces of a stitched field, south -> north, as [(sub-grid, first band row, end band row, row of the stitched
        field where the piece starts)], and the field's total row count (OGG:1315-1365): fields on point rows (x, y, dx, angle_dx)
        drop the last row of every sub-grid but the northernmost; dy and area (cell rows) are concatenated whole.  cut: the triple
        of plan.south_cut().  Every band of every rank maps to ONE contiguous range of stitched rows."""
        c_sc, c_so, gone = cut
        subs = [s for s in self.plan.subs if not (s.name == "SC" and gone)]
        out, off = [], 0
        for k, s in enumerate(subs):
            b = self.buf[s.name]
            first = c_sc if s.name == "SC" else (c_so if (s.name == "SO" and gone) else 0)     # first kept row of the sub-grid
            last = (s.nj1 - (0 if k == len(subs) - 1 else 1)) if point_rows else s.nj1 - 1     # end of its kept rows
            kept = max(last - first, 0)
            r_lo, r_hi = b["lo"], (b["hi"] if point_rows else b["lo"] + b["n_cell"])             # this rank's rows of it
            lo, hi = max(r_lo, first), min(r_hi, last)
            if hi > lo:
                out.append((s, lo - b["lo"], hi - b["lo"], off + (lo - first)))
            off += kept
        return out, off

    def stitched_rows(self, cut):
        """nyp of the stitched grid"""
        return self._pieces(cut, True)[1]

    def stitched_column(self, field, col, cut, only=None):
        """One column of a stitched field (or of one sub-grid) as a host array: what main()'s guards and description need.  World 1."""
        assert self.world == 1
        torch = self.torch
        if only is not None:
            b = self.buf[only]
            return b[field][: b["n"], col].cpu().numpy()
        parts = [self.buf[s.name][field][lo:hi, col] for s, lo, hi, _ in self._pieces(cut, field in ("x", "y", "dx", "angle_dx"))[0]]
        return torch.cat(parts).cpu().numpy() if parts else np.zeros(0)

    def write_nc(self, fnam, cut, description=None, history=None, source=None, no_changing_meta=None, create=None, barrier=None):
        """write_nc of OGG:773-829 for the fields in HBM: the reference's layout (dimensions nyp, nxp, ny, nx, string(255); variables
        tile, y, x, dy, dx, area, angle_dx in that order; NetCDF-3 64-bit offset), every band streamed from the device into its byte
        range of the file (nc_stream).  Band-sharded runs write ONE file together: the rank with ``create`` (default: rank 0) writes
        the header and extends the file to its final size, then -- after ``barrier()`` (default: torch.distributed.barrier when a
        process group exists and world > 1) -- every rank streams its own bands to their offsets; no gather.  Returns (bytes this
        rank streamed, seconds)."""
        import os
        import time
        from . import nc_stream, netcdf3
        t0 = time.perf_counter()
        nyp, nx = self.stitched_rows(cut), self.plan.Ni
        ny = nyp - 1
        create = (self.rank == 0) if create is None else create
        if barrier is None:
            barrier = lambda: None   # noqa: E731
            if self.world > 1 and self.halo == "rccl":
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized():
                    barrier = dist.barrier
        gatts = []
        if not no_changing_meta:
            gatts = [("history", history or ""), ("description", description or ""), ("source", source or "")]
        ds = netcdf3.Dataset(fnam, [("nyp", nyp), ("nxp", nx + 1), ("ny", ny), ("nx", nx), ("string", 255)], gatts)
        ds.decl_var("tile", netcdf3.NC_CHAR, ("string",), [])
        spec = (("y", "y", ("nyp", "nxp"), "degrees"), ("x", "x", ("nyp", "nxp"), "degrees"), ("dy", "dy", ("ny", "nxp"), "meters"),
                ("dx", "dx", ("nyp", "nx"), "meters"), ("area", "area", ("ny", "nx"), "m2"), ("angle_dx", "angle_dx", ("nyp", "nxp"), "degrees"))
        for name, _, dims, units in spec:
            ds.decl_var(name, netcdf3.NC_DOUBLE, dims, [("units", units)])
        if create:
            print("   Writing netcdf file with ny,nx= ", ny, nx)
            fd = os.open(fnam, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                ds.write_header(fd)
                os.pwrite(fd, b"tile1".ljust(255, b"\0"), ds.var_begin("tile"))
            finally:
                os.close(fd)
        barrier()   # the file exists at its final size
        fd = os.open(fnam, os.O_RDWR)
        try:
            stream = nc_stream.DeviceToFile(fd, self.device)
            try:
                for name, f, _, _ in spec:
                    row_bytes = (nx + 1 if f in ("x", "y", "dy", "angle_dx") else nx) * 8
                    for s, lo, hi, row0 in self._pieces(cut, f in ("x", "y", "dx", "angle_dx"))[0]:
                        stream.put(self.buf[s.name][f][lo:hi], ds.var_begin(name) + row0 * row_bytes)
            finally:
                stream.finish()   # also after an error: no writer thread may outlive the file descriptor
        finally:
            os.close(fd)
        barrier()   # every rank's bytes are in the file
        return stream.bytes, time.perf_counter() - t0

    def _fetch_rows(self, pieces, wanted):
        """{(dst piece, key, field): 1-D row} of the entries of ``wanted`` whose destination piece is on THIS rank.  ``wanted``: (dst
        piece, key, field, src rank, src sub-grid name, src band row), built in the same order on every rank.  Rows of this rank are
        views of its buffers; rows of another rank come device-to-device from its Supergrid (halo="local") or over torch.distributed
        (batch_isend_irecv), as in exchange_halo.  A received row is nx wide for dx, nx + 1 for every other field."""
        torch = self.torch
        out, ops = {}, []
        for k, key, f, src, name, row in wanted:
            if pieces[k]["rank"] == self.rank:
                if src == self.rank:
                    t = self.buf[name][f][row]
                elif self.halo == "local":
                    t = self.peers[src].buf[name][f][row].clone()
                else:
                    t = torch.empty(self.plan.Ni + (0 if f == "dx" else 1), dtype=torch.float64, device=self.device)
                    ops.append(("recv", t, src))
                out[k, key, f] = t
            elif src == self.rank and self.halo != "local":
                ops.append(("send", self.buf[name][f][row].contiguous(), pieces[k]["rank"]))
        if ops:
            import torch.distributed as dist
            if all(t.is_cuda for _, t, _ in ops) and dist.get_backend() != "gloo":
                p2p = [dist.P2POp(dist.isend if d == "send" else dist.irecv, t, r) for d, t, r in ops]
                for w in dist.batch_isend_irecv(p2p):
                    w.wait()
            else:   # gloo (the CPU tests, the one-GPU rehearsal): through host copies, in the common order
                for d, t, r in ops:
                    if d == "send":
                        dist.send(t.cpu(), r)
                    else:
                        c = torch.empty(t.shape, dtype=t.dtype)
                        dist.recv(c, r)
                        t.copy_(c)
        return out

    def _bands(self, cut, make, skip=lambda q: False):
        """(piece index, piece, its buffers, band) of THIS rank's pieces but those ``skip`` names: band = make(q) with x and y set at the
        piece's first row."""
        for k, q in enumerate(self.quality_pieces(cut)):
            if q["rank"] == self.rank and not skip(q):
                b = self.buf[q["sub"].name]
                band = make(q)
                band.x, band.y = self._p(b["x"], q["row"]), self._p(b["y"], q["row"])
                yield k, q, b, band

    def _gather(self, pieces, records, send, recv):
        """Every rank's per-piece results on rank 0, None on the other ranks.  ``records(g)``: the list of Supergrid g's pieces; rank 0
        holds its own, then the peers' (halo="local") or what the other ranks send over torch.distributed: each sends the tensors of
        ``send(entry)`` for its entries in piece order, and rank 0 walks ``pieces`` calling ``recv(k, piece, take)``, which returns the
        piece's entry (None for a piece that sends nothing), ``take(shape, dtype)`` receiving the next tensor from the piece's rank
        (on the CPU under gloo, on the device otherwise)."""
        if self.world > 1 and self.halo == "local" and self.rank != 0:
            return None   # rank 0 does the pieces of every virtual rank through its peer objects
        got = records(self)
        if self.world > 1 and self.halo == "local":
            for g in self.peers:
                if g is not self:
                    got += records(g)
        elif self.world > 1:
            import torch.distributed as dist
            gloo = dist.get_backend() == "gloo"
            if self.rank != 0:
                for e in got:
                    for t in send(e):
                        dist.send(t.cpu() if gloo else t.contiguous(), 0)
                return None
            for k, q in enumerate(pieces):   # in piece order, as every other rank sends its own
                def take(shape, dtype, src=q["rank"]):
                    t = self.torch.empty(shape, dtype=dtype, device="cpu" if gloo else self.device)
                    dist.recv(t, src)
                    return t
                e = recv(k, q, take) if q["rank"] != 0 else None
                got += [e] if e is not None else []
        return got

    # -- grid-quality report ------------------------------------------------------------------------------------
    def quality_pieces(self, cut):
        """Every rank's pieces of the stitched grid, south -> north, for the quality report: dicts with the rank, the sub-grid, the
        band row the piece starts at ("row"), its point and cell rows (n_pt, n_cell) and its first stitched row (j0).  The same list on
        every rank (rows_of is a function of the plan and the world size only)."""
        c_sc, c_so, gone = cut
        subs = [s for s in self.plan.subs if not (s.name == "SC" and gone)]
        out, off = [], 0
        for k, s in enumerate(subs):
            first = c_sc if s.name == "SC" else (c_so if (s.name == "SO" and gone) else 0)
            last_pt = s.nj1 - (0 if k == len(subs) - 1 else 1)
            for r in range(self.world):
                blo, bhi = self.rows_of(s, r, self.world)
                lo, hi_pt, hi_c = max(blo, first), min(bhi, last_pt), min(bhi, s.nj1 - 1)
                if hi_pt > lo:
                    out.append({"rank": r, "sub": s, "row": lo - blo, "n_pt": hi_pt - lo, "n_cell": max(hi_c - lo, 0),
                                "j0": off + lo - first})
            off += max(last_pt - first, 0)
        return out

    def quality_halo(self, cut):
        """The rows the pieces of THIS rank need from elsewhere (_fetch_rows), as {piece index: {"next": {x, y, dx, dy}, "seam": {x,
        y}}} of 1-D tensors: the first point row (x, y, dx) and cell row (dy) of the piece that follows in stitched order, and at a
        sub-grid joint the lower sub-grid's own last point row (x, y), which stitching drops."""
        pieces = self.quality_pieces(cut)
        metrics = not self.plan.skip_metrics
        wanted = []
        for k, p in enumerate(pieces[:-1]):
            q = pieces[k + 1]
            for f in ("x", "y") + (("dx",) if metrics else ()) + (("dy",) if metrics and q["n_cell"] > 0 else ()):
                wanted.append((k, "next", f, q["rank"], q["sub"].name, q["row"]))
            s = p["sub"]
            if q["sub"] is not s:   # a joint: the lower sub-grid's row nj1 - 1
                src = next(r for r in range(self.world) if self.rows_of(s, r, self.world)[1] == s.nj1)
                row = s.nj1 - 1 - self.rows_of(s, src, self.world)[0]
                for f in ("x", "y"):
                    wanted.append((k, "seam", f, src, s.name, row))
        out = {}
        for (k, kind, f), t in self._fetch_rows(pieces, wanted).items():
            out.setdefault(k, {}).setdefault(kind, {})[f] = t
        return out

    def quality_records(self, cut, halo=None):
        """Device tensor (n_pieces, record words) of int64: the ogg_grid_quality_result of every piece of this rank, zeros elsewhere."""
        from . import grid_quality as Q
        torch, st = self.torch, self._stream()
        halo = self.quality_halo(cut) if halo is None else halo   # (held until the kernels have run: the bands point into it)
        bands = self.quality_bands(cut, halo)
        words = ctypes.sizeof(L.QualityResult) // 8
        out = torch.zeros((len(self.quality_pieces(cut)), words), dtype=torch.int64, device=self.device)
        keep = []
        for k, band in bands:
            rec, ws = Q.band_record_dev(band, st, self.device)
            out[k].copy_(rec)
            keep.append((rec, ws))
        self.torch.cuda.synchronize(self.device)
        return out

    def quality_bands(self, cut, halo):
        """[(piece index, ogg_quality_band of device pointers)] of this rank's pieces; `halo` from quality_halo (kept alive by the caller)."""
        p = self.plan
        metrics = not p.skip_metrics
        out = []
        for k, q, b, band in self._bands(cut, lambda q: L.QualityBand(nx=p.Ni, j0=q["j0"], n_pt_rows=q["n_pt"], n_cell_rows=q["n_cell"],
                                                                     Re=float(p.Re), metrics=int(metrics))):
            r = q["row"]
            if metrics:
                band.dx = self._p(b["dx"], r)
                band.dy = self._p(b["dy"], r) if q["n_cell"] else None
                band.area = self._p(b["area"], r) if q["n_cell"] else None
            nxt, seam = halo.get(k, {}).get("next", {}), halo.get(k, {}).get("seam", {})
            band.x_next, band.y_next, band.dx_next, band.dy_next = (nxt[f].data_ptr() if f in nxt else None for f in ("x", "y", "dx", "dy"))
            if seam:
                band.x_seam, band.y_seam = seam["x"].data_ptr(), seam["y"].data_ptr()
            out.append((k, band))
        return out

    def quality(self, cut):
        """The grid-quality report (grid_quality.report) of the stitched grid of every rank: a record per piece of every rank, one
        all-reduce of the int64 records (each piece is non-zero on one rank only, so the sum is a gather, bit for bit), merged on the
        host in stitched order."""
        from . import grid_quality as Q
        t = self.quality_records(cut)
        if self.world > 1:
            if self.halo == "local":
                t = sum(g.quality_records(cut) for g in self.peers if g is not self) + t
            else:
                all_reduce(t)
        host = t.cpu().numpy()
        pieces = self.quality_pieces(cut)
        recs = [(q["sub"].name, q["j0"], Q.record_from_bytes(host[k])) for k, q in enumerate(pieces)]
        return Q.report(recs, self.plan.Re, self.stitched_rows(cut), self.plan.Ni, not self.plan.skip_metrics)

    # -- topography by refined sampling -------------------------------------------------------------------------
    def topography_records(self, cut, source, refine=None, oversample=2.0, cells="model", halo=None, plane=False):
        """[(piece index, first output row, int64 device tensor of records)] of THIS rank's pieces of the stitched grid, sampled on the
        buffers the pass left in HBM.  A piece's last cell row takes its upper point row from the next piece (quality_halo); a model
        row whose two supergrid rows lie in two pieces gets a partial record from each, combined exactly by the caller.  ``plane``:
        plane records (ogg_topog_plane_band_dev).  ``source``: a topography.DeviceSource, or a DeviceSourceList (merge records,
        ogg_topog_layers_band_dev)."""
        from . import topography as T
        p, st = self.plan, self._stream()
        halo = self.quality_halo(cut) if halo is None else halo   # (held until the kernels have run: the bands point into it)
        kind = L.TOPOG_MODEL_CELLS if cells == "model" else L.TOPOG_SUPERGRID_CELLS
        out, keep = [], []
        for k, q, b, band in self._bands(cut, lambda q: L.TopogBand(nx=p.Ni, j0=q["j0"], n_cell_rows=q["n_cell"], refine=int(refine or 0),
                                                                   oversample=float(oversample), cells=kind),
                                         skip=lambda q: q["n_cell"] == 0):
            nxt = halo.get(k, {}).get("next")
            if nxt is not None:
                band.x_next, band.y_next = nxt["x"].data_ptr(), nxt["y"].data_ptr()
            else:   # the piece that ends the grid holds its own last point row
                band.x_next, band.y_next = self._p(b["x"], q["row"] + q["n_cell"]), self._p(b["y"], q["row"] + q["n_cell"])
            m0, rec, ws = T.band_records_dev(band, source.desc, st, self.device, plane)
            out.append((k, m0, rec))
            keep.append(ws)
        self.torch.cuda.synchronize(self.device)
        return out

    def topography(self, cut, source, refine=None, oversample=2.0, cells="model", plane=False):
        """Topography of the stitched grid of every rank (topography.result on rank 0, None on the other ranks): ``source`` a
        topography.DeviceSource (DeviceSourceList) on this rank's GPU, or a topography.Source (SourceList: layers in order of priority,
        every rank uploads every one) to upload there.  Every piece is sampled by the rank that holds it; rank 0 gathers the integer records
        (_gather) and combines them exactly, so the result is bit-identical for any number of ranks.  ``plane``: plane records through
        the same gather, and the stitched latitudes gathered on rank 0 (_stitched) for the slopes of the plane."""
        from . import topography as T
        if isinstance(source, T.Source):
            source = T.DeviceSource(source, self.device)
        elif isinstance(source, T.SourceList):
            source = T.DeviceSourceList(source, self.device)
        layered = isinstance(source, T.DeviceSourceList)
        if layered and plane:
            raise ValueError(T.NO_PLANE)
        nyp, nxp = self.stitched_rows(cut), self.plan.Ni + 1
        T.check_args(nyp, nxp, cells, refine, oversample)
        sh = 1 if cells == "model" else 0
        words = T.record_words(plane, layered)

        def recv(k, q, take):
            if q["n_cell"] == 0:
                return None
            rows = ((q["j0"] + q["n_cell"] - 1) >> sh) - (q["j0"] >> sh) + 1
            return k, q["j0"] >> sh, take((rows, self.plan.Ni >> sh, words), self.torch.int64)
        got = self._gather(self.quality_pieces(cut), lambda g: g.topography_records(cut, source, refine, oversample, cells, plane=plane),
                           lambda e: (e[2],), recv)
        lat = self._stitched(cut, ("y",), True) if plane else None   # every rank takes part
        if got is None:
            return None
        recs = T.assemble([(m0, T.records_to_host(t)) for _, m0, t in got], (nyp - 1) >> sh, (nxp - 1) >> sh, plane)
        lat_c = T.cell_latitudes(lat[0].cpu().numpy(), cells) if plane else None
        return T.result(recs, source.source.quantum, source.sea_level, cells, refine, oversample, source.source, lat_c)

    # -- atmosphere x ocean exchange grid --------------------------------------------------------------------------
    @staticmethod
    def _xgrid_rows(q):
        """(first model row, model rows, point rows needed after the piece) of a piece: its model rows are the m with 2 m in its cell
        rows (include/ogg_hip.h, ogg_xgrid_band)."""
        m0, m1 = (q["j0"] + 1) // 2, (q["j0"] + q["n_cell"] + 1) // 2
        rows = max(m1 - m0, 0)
        return m0, rows, (2 * m1 - (q["j0"] + q["n_cell"]) + 1) if rows else 0

    def xgrid_halo(self, cut):
        """{piece index: (x rows, y rows)} of THIS rank's pieces: the (one or two) stitched point rows that follow each piece, as
        contiguous (rows, nx + 1) tensors, fetched by _fetch_rows."""
        torch = self.torch
        pieces = self.quality_pieces(cut)
        wanted = []
        for k, p in enumerate(pieces):
            for t in range(self._xgrid_rows(p)[2]):
                R = p["j0"] + p["n_cell"] + t
                src = next(q for q in pieces if q["j0"] <= R < q["j0"] + q["n_pt"])
                for f in ("x", "y"):
                    wanted.append((k, t, f, src["rank"], src["sub"].name, src["row"] + R - src["j0"]))
        got = {}
        for (k, _, f), r in self._fetch_rows(pieces, wanted).items():   # (in the order of t)
            got.setdefault(k, {}).setdefault(f, []).append(r)
        return {k: (torch.stack(v["x"]).contiguous(), torch.stack(v["y"]).contiguous()) for k, v in got.items()}

    def xgrid_lists(self, cut, atm, mask=None, threshold=1e-6, halo=None):
        """[(piece index, first model row, counts, a_poly, atm, ocn, area)] of THIS rank's pieces (device tensors), the exchange grid
        of each piece computed on the buffers the pass left in HBM.  ``atm``: (lon, lat) edges as float64 device tensors, or a cubed
        sphere (a dict of exchange_grid_cs.cubed_sphere_atm with its table "t" a device tensor; atm then has three columns), or a
        curvilinear source (a dict {"curv": (corner lon, corner lat, mask or None)} of device tensors; atm is then the source cell
        (I, J) and the counts are ogg_xgrid_curv_counts); ``mask``: None or a uint8 device tensor of every model cell of the stitched
        grid."""
        p, st = self.plan, self._stream()
        halo = self.xgrid_halo(cut) if halo is None else halo   # (held until the kernels have run: the bands point into it)
        if isinstance(atm, dict) and "curv" in atm:
            from . import exchange_grid_curv as XV
            sx, sy, sm = atm["curv"]
            desc = XV.src_desc(sx.data_ptr(), sy.data_ptr(), sx.shape[1] - 1, sx.shape[0] - 1, ld=sx.stride(0),
                               mask_ptr=None if sm is None else sm.data_ptr())

            def lists(*a):   # without A_src, the same in every piece (exchange_grid_curv.source_areas_dev gives it once)
                m0, counts, a_poly, _, sij, ocn, area = XV.band_lists_dev(*a)
                return m0, counts, a_poly, sij, ocn, area
        elif isinstance(atm, dict):
            from . import exchange_grid_cs as X
            desc, lists = X.atm_desc(atm, atm["t"].data_ptr()), X.band_lists_dev
        else:
            from . import exchange_grid as X
            lon, lat = atm
            desc, lists = L.XgridAtm(lon=lon.data_ptr(), lat=lat.data_ptr(), NA=lon.numel() - 1, NB=lat.numel() - 1), X.band_lists_dev
        ny = self.stitched_rows(cut) - 1
        out = []
        for k, q, _, band in self._bands(cut, lambda q: L.XgridBand(nx=p.Ni, ny=ny, j0=q["j0"], n_cell_rows=q["n_cell"], Re=float(p.Re),
                                                                   threshold=float(threshold)),
                                         skip=lambda q: self._xgrid_rows(q)[1] == 0):
            band.x_next, band.y_next = halo[k][0].data_ptr(), halo[k][1].data_ptr()
            band.mask = None if mask is None else mask.data_ptr() + self._xgrid_rows(q)[0] * (p.Ni // 2)
            out.append((k,) + lists(band, desc, st, self.device))
        self.torch.cuda.synchronize(self.device)
        return out

    def _gather_xgrid(self, cut, lon, lat, hm, threshold, cs=None, curv=None):
        """Every rank's xgrid_lists on rank 0 in piece order, the canonical order of the list (None on the other ranks): [(piece index,
        first model row, counts, a_poly, atm, ocn, area)], on the device or, under gloo, the CPU.  ``hm``: None or a uint8 host
        array of every model cell.  ``cs``: a cubed-sphere atmosphere (host arrays) in the place of the edges lon, lat.  ``curv``:
        a curvilinear source (corner lon, corner lat, mask or None as host arrays) in their place."""
        torch = self.torch
        ncol = self.plan.Ni // 2
        fields, atm_cols = (L.XGRID_COUNT_FIELDS, 2) if cs is None else (L.XGRID_CS_COUNT_FIELDS, 3)
        if curv is not None:
            fields = L.XGRID_CURV_COUNT_FIELDS

        def records(g):
            to = lambda a: torch.from_numpy(a).to(g.device)   # noqa: E731
            if curv is not None:
                atm = {"curv": tuple(None if a is None else to(a) for a in curv)}
            else:
                atm = (to(lon), to(lat)) if cs is None else dict(cs, t=to(cs["t"]))
            return g.xgrid_lists(cut, atm, None if hm is None else to(hm), threshold)

        def send(e):   # counts first, then the arrays (when there are any), then a_poly
            _, _, counts, a_poly, atm_ij, ocn_ij, area = e
            return (counts,) + ((atm_ij, ocn_ij, area) if atm_ij.shape[0] else ()) + (a_poly,)

        def recv(k, q, take):
            m0, rows, _ = self._xgrid_rows(q)
            if rows == 0:
                return None
            counts = take(len(fields), torch.int64)
            n = int(counts[fields.index("kept")])
            lists = [take(s, d) if n else torch.empty(s, dtype=d, device=counts.device)
                     for s, d in (((n, atm_cols), torch.int32), ((n, 2), torch.int32), (n, torch.float64))]
            return (k, m0, counts, take((rows, ncol), torch.float64), *lists)
        got = self._gather(self.quality_pieces(cut), records, send, recv)
        if got is not None:
            got.sort(key=lambda e: e[0])
        return got

    def exchange_grid(self, cut, atm, mask=None, threshold=1e-6):
        """The atmosphere x ocean exchange grid of the stitched grid of every rank (exchange_grid.result on rank 0, None on the other
        ranks).  ``atm``: (lon_edges, lat_edges) of a global rectilinear atmosphere; ``mask``: None or one value per model cell (0:
        the cell emits nothing).  Every piece is done by the rank that holds it; rank 0 gathers the lists in piece order (_gather:
        the counts first, then the arrays), which is the canonical order, so the result is bit-identical for any number of ranks."""
        from . import exchange_grid as X
        torch = self.torch
        nyp, nxp = self.stitched_rows(cut), self.plan.Ni + 1
        X.check_grid(nyp, nxp)
        X.check_args(threshold, self.plan.Re)
        lon, lat = X.atm_edges(*atm)
        shape = ((nyp - 1) // 2, (nxp - 1) // 2)
        hm = None
        if mask is not None:
            hm = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if hm.shape != shape:
                raise ValueError("exchange grid: the mask is %s, the model cells %s" % (hm.shape, shape))

        got = self._gather_xgrid(cut, lon, lat, hm, threshold)
        if got is None:
            return None
        hostp = [(m0,) + tuple(t.cpu().numpy() for t in ts) for _, m0, *ts in got]
        return X.assemble(hostp, shape, lon, lat, float(self.plan.Re), threshold, mask is not None)

    def exchange_grid_cs(self, cut, atm, mask=None, threshold=1e-6):
        """exchange_grid with a cubed-sphere atmosphere (exchange_grid_cs.result on rank 0, None on the other ranks).  ``atm``: a
        cubed sphere of exchange_grid_cs.cubed_sphere_atm or cubed_sphere_from_corners.  The same pieces, halo rows and gather; the
        atmosphere index has three columns (I, J, face)."""
        from . import exchange_grid as X
        from . import exchange_grid_cs as XC
        nyp, nxp = self.stitched_rows(cut), self.plan.Ni + 1
        X.check_grid(nyp, nxp)
        X.check_args(threshold, self.plan.Re)
        atm = XC.checked_atm(atm)
        shape = ((nyp - 1) // 2, (nxp - 1) // 2)
        hm = XC.host_mask(mask, shape)
        got = self._gather_xgrid(cut, None, None, hm, threshold, cs=atm)
        if got is None:
            return None
        hostp = [(m0,) + tuple(t.cpu().numpy() for t in ts) for _, m0, *ts in got]
        return XC.assemble(hostp, shape, atm, float(self.plan.Re), threshold, mask is not None)

    def exchange_grid_curv(self, cut, src_lon, src_lat, mask=None, src_mask=None, threshold=1e-6):
        """exchange_grid with a curvilinear source grid (exchange_grid_curv.result on rank 0, None on the other ranks).  src_lon,
        src_lat: the source's cell corners ((NB + 1) x (NA + 1), degrees); src_mask: None or one value per source cell.  The source is
        whole on every rank, the target is banded as for the other lists: the same pieces, halo rows and gather."""
        from . import exchange_grid as X
        from . import exchange_grid_curv as XV
        nyp, nxp = self.stitched_rows(cut), self.plan.Ni + 1
        X.check_grid(nyp, nxp)
        X.check_args(threshold, self.plan.Re)
        lon, lat, sm = XV.checked_source(src_lon, src_lat, src_mask)
        XV.src_desc(None, None, lon.shape[1] - 1, lon.shape[0] - 1)
        shape = ((nyp - 1) // 2, (nxp - 1) // 2)
        hm = XV.host_mask(mask, shape)
        got = self._gather_xgrid(cut, None, None, hm, threshold, curv=(lon, lat, sm))
        if got is None:
            return None
        a_src, counts = XV.source_areas_dev(*(None if a is None else self.torch.from_numpy(a).to(self.device) for a in (lon, lat, sm)),
                                            Re=float(self.plan.Re), stream=self._stream())
        hostp = [(m0, c.cpu().numpy(), ap.cpu().numpy(), a_src) + tuple(t.cpu().numpy() for t in ts) for _, m0, c, ap, *ts in got]
        if not hostp:   # no piece holds a model row: the source's counts alone
            hostp = [(0, counts, np.zeros((0, shape[1])), a_src, np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), np.zeros(0))]
        return XV.assemble(hostp, shape, float(self.plan.Re), threshold, mask is not None, sm is not None)

    # -- ocean mask ---------------------------------------------------------------------------------------------------
    def _stitched(self, cut, fields, point_rows):
        """The stitched ``fields`` (float64 device tensors, contiguous) on rank 0's device, None on the other ranks: the point rows
        (x, y, angle_dx) or the cell rows (area) of every piece gathered in piece order, all the fields in one _gather."""
        torch, n = self.torch, "n_pt" if point_rows else "n_cell"

        def records(g):
            out = []
            for k, q in enumerate(g.quality_pieces(cut)):
                if q["rank"] == g.rank and q[n] > 0:
                    b = g.buf[q["sub"].name]
                    out.append((k,) + tuple(b[f][q["row"]:q["row"] + q[n]].to(self.device) for f in fields))
            return out

        def recv(k, q, take):
            if q[n] == 0:
                return None
            return (k,) + tuple(take((q[n], self.plan.Ni + (0 if f in ("dx", "area") else 1)), torch.float64) for f in fields)
        got = self._gather(self.quality_pieces(cut), records, lambda e: e[1:], recv)
        if got is None:
            return None
        got.sort(key=lambda e: e[0])
        return tuple(torch.cat([e[i].to(self.device) for e in got]).contiguous() for i in range(1, len(fields) + 1))

    def stitched_xy(self, cut):
        """The stitched x and y ((nyp, nxp) float64 device tensors) on rank 0's device, None on the other ranks (_stitched)."""
        return self._stitched(cut, ("x", "y"), True)

    def stitched_area(self, cut):
        """The stitched supergrid area ((nyp - 1, nxp - 1) float64 device tensor) on rank 0's device, None on the other ranks
        (_stitched, cell rows)."""
        if self.plan.skip_metrics:
            raise ValueError("the supergrid area is not computed with --skip_metrics")
        got = self._stitched(cut, ("area",), False)
        return None if got is None else got[0]

    def ocean_mask(self, cut, topo, min_depth=0.0, mode="mask", seeds=(), keep_min_cells=0):
        """The ocean mask (ocean_mask.result on rank 0, None on the other ranks) of the topography ``topo`` that topography() gathered on
        rank 0, computed on rank 0's GPU with the stitched grid gathered there: the same for any number of ranks by construction."""
        from . import ocean_mask as M
        from . import topography as T
        xy = self.stitched_xy(cut)
        if xy is None:
            return None
        depth = self.torch.from_numpy(np.ascontiguousarray(topo["depth"], dtype=np.float64)).to(self.device)
        res = M.ocean_mask_dev(depth, xy[0], xy[1], min_depth=min_depth, mode=mode, seeds=seeds, keep_min_cells=keep_min_cells,
                               fill=T.FILL)
        return res

    # -- conservative remap -------------------------------------------------------------------------------------------
    def remap(self, cut, source, mask=None, fill=True, fill_max=None, threshold=1e-6):
        """The conservative remap (remap.result on rank 0, None on the other ranks) of ``source`` (a remap.Source, or a
        remap.CurvilinearSource, whose list is that of exchange_grid_curv) onto the model cells
        of the stitched grid.  ``mask``: None or one value per model cell (0: dry).  Every rank builds the lists of its own pieces
        (xgrid_lists, the source's edges as the atmosphere) and remaps their cells on its GPU; rank 0 gathers the values, flags and
        counts in piece order (_gather) and fills on its GPU with the topology of the stitched grid, as ocean_mask does.  Nothing is
        summed across pieces, so the result is bit-identical for any number of ranks."""
        from . import exchange_grid as X
        from . import fields as F
        from . import ocean_mask as M
        from . import remap as R
        torch = self.torch
        nyp, nxp = self.stitched_rows(cut), self.plan.Ni + 1
        X.check_grid(nyp, nxp)
        shape = ((nyp - 1) // 2, (nxp - 1) // 2)
        hm = F.cell_mask(mask, shape, "remap: the mask")
        R.params(shape[0], shape[1], source, 0, False, False, fill_max)   # the checks, before any device work
        nrec = source.nrec

        def records(g):
            to = lambda a: torch.from_numpy(a).to(g.device)   # noqa: E731
            mt = None if hm is None else to(hm)
            f = to(source.records)
            out = []
            if isinstance(source, R.CurvilinearSource):
                atm_ = {"curv": tuple(None if a is None else to(a) for a in (source.corner_lon, source.corner_lat, source.mask))}
            else:
                atm_ = (to(source.lon), to(source.lat))
            for k, m0, _, a_poly, atm, ocn, area in g.xgrid_lists(cut, atm_, mt, threshold):
                p = R.params(a_poly.shape[0], shape[1], source, m0)
                rows = None if mt is None else mt[m0:m0 + a_poly.shape[0]]
                out.append((k,) + R.piece_dev(p, f, atm, ocn, area, rows, g._stream(), g.device))
            torch.cuda.synchronize(g.device)
            return out

        def recv(k, q, take):
            _, rows, _ = self._xgrid_rows(q)
            if rows == 0:
                return None
            return (k, take((nrec, rows, shape[1]), torch.float64), take((nrec, rows, shape[1]), torch.uint8),
                    take(len(L.REMAP_COUNT_FIELDS), torch.int64))
        got = self._gather(self.quality_pieces(cut), records, lambda e: (e[1].contiguous(), e[2].contiguous(), e[3]), recv)
        xy = self.stitched_xy(cut)
        if got is None:
            return None
        got.sort(key=lambda e: e[0])
        values = torch.cat([e[1].to(self.device) for e in got], dim=1).contiguous()
        flags = R.flags_buffer(torch, values.numel(), self.device).view(values.shape)
        flags.copy_(torch.cat([e[2].to(self.device) for e in got], dim=1))
        counts = torch.stack([e[3].to(self.device) for e in got]).sum(dim=0)
        periodic, fold = M.topology_of_device_grid(*xy)
        if fill:
            p = R.params(shape[0], shape[1], source, 0, periodic, fold, fill_max)
            R.fill_dev(p, values, flags, counts, self._stream(), self.device)
        return R.result(values.cpu().numpy(), flags.cpu().numpy(), R.counts_dict(counts.cpu().numpy()), source, periodic, fold, fill,
                        fill_max, hm is not None)

    # -- conservative regrid to a lat-lon grid ------------------------------------------------------------------------
    def regrid_to_latlon(self, cut, field, atm, mask=None, normalize="area", cover=False, threshold=1e-6, lists=None):
        """The conservative regrid (latlon_regrid.result on rank 0, None on the other ranks) of ``field`` (a latlon_regrid.Field, an
        array (..., ny, nx) of the stitched grid's model cells, or None for the static sums alone) onto the lat-lon cells of ``atm``
        = (lon_edges, lat_edges).  ``mask``: None or one value per model cell (0: the cell takes no part).  Every rank builds the
        lists of its own pieces (xgrid_lists); rank 0 gathers them in piece order (_gather), then transposes and sums on its GPU: the
        list is the canonical one whatever the rank count, and per-rank partial sums could not be combined bit-identically.  ``lists``:
        rank 0's exchange_grid() result for the same atm, mask and threshold, whose list is used instead of building and gathering it
        again (the call then runs on this rank alone)."""
        from . import exchange_grid as X
        from . import fields as F
        from . import latlon_regrid as G
        torch = self.torch
        nyp, nxp = self.stitched_rows(cut), self.plan.Ni + 1
        X.check_grid(nyp, nxp)
        X.check_args(threshold, self.plan.Re)
        lon, lat = X.atm_edges(*atm)
        shape = ((nyp - 1) // 2, (nxp - 1) // 2)
        if field is not None and not isinstance(field, G.Field):
            field = G.Field(field)
        p = G.params(shape, lon, lat, field, normalize)   # the checks, before any device work
        hm = F.cell_mask(mask, shape, "regrid: the mask")
        if lists is not None:
            atm_ij, ocn_ij, area = (torch.from_numpy(np.ascontiguousarray(lists[k])).to(self.device) for k in ("atm", "ocn", "area"))
        else:
            got = self._gather_xgrid(cut, lon, lat, hm, threshold)
            if got is None:
                return None
            cat = lambda i, s, d: torch.cat([e[i].to(self.device) for e in got]) if got else torch.empty(s, dtype=d, device=self.device)   # noqa: E731
            atm_ij, ocn_ij, area = cat(4, (0, 2), torch.int32), cat(5, (0, 2), torch.int32), cat(6, (0,), torch.float64)
        a_atm = np.ascontiguousarray(X.atm_area(lon, lat, float(self.plan.Re)))
        return G.finish_dev(p, atm_ij.contiguous(), ocn_ij.contiguous(), area.contiguous(), field, lon, lat, a_atm, normalize, cover,
                            hm is not None, shape, self._stream(), self.device)

    # -- runoff mapping -----------------------------------------------------------------------------------------------
    def runoff(self, cut, source, wet, targets="coast", spread_km=None, spread_shape="biweight", spread_classes=None, keep_lists=False):
        """The runoff mapping (runoff.result on rank 0, None on the other ranks) of ``source`` (a remap.Source) onto the model cells of
        the stitched grid with the wet set ``wet`` (one value per model cell, 0: land), on rank 0's GPU with the stitched points and
        area gathered there, as ocean_mask does: the same bits for any number of ranks by construction.  ``spread_km``: the mapped
        values spread over the wet cells within that radius (runoff.spread_dev; ``spread_classes``: one integer per model cell), on
        the same gathered grid."""
        from . import runoff as RO
        xy = self.stitched_xy(cut)
        area = self.stitched_area(cut)
        if xy is None:
            return None
        if spread_km is None:
            return RO.runoff_dev(xy[0], xy[1], area, source, wet, targets=targets, Re=float(self.plan.Re), keep_lists=keep_lists)
        return RO.runoff_dev(xy[0], xy[1], area, source, wet, targets=targets, Re=float(self.plan.Re), keep_lists=keep_lists,
                             spread_km=spread_km, spread_shape=spread_shape, spread_classes=spread_classes)

    # -- distance to the coast ----------------------------------------------------------------------------------------
    def coast_distance(self, cut, wet, sides="both"):
        """The distance to the coast (coast_distance.result on rank 0, None on the other ranks) of the model cells of the stitched grid
        with the wet set ``wet`` (one value per model cell, 0: land), on rank 0's GPU with the stitched points gathered there, as
        runoff does: the same bits for any number of ranks by construction."""
        from . import coast_distance as CD
        xy = self.stitched_xy(cut)
        if xy is None:
            return None
        return CD.coast_distance_dev(xy[0], xy[1], wet, sides=sides, Re=float(self.plan.Re))

    # -- face topography ----------------------------------------------------------------------------------------------
    def face_topography(self, cut, source, refine=None, oversample=2.0, sea_level=None):
        """The face topography (face_topography.result on rank 0, None on the other ranks) of the stitched grid from ``source`` (one
        lat-lon topography.Source or DeviceSource), on rank 0's GPU with the stitched points gathered there, as coast_distance does:
        the same bits for any number of ranks by construction.  Band-sharded face sampling is not done."""
        from . import face_topography as FT
        from . import topography as T
        if isinstance(source, (T.DeviceSourceList, T.SourceList)) or getattr(getattr(source, "source", source), "projection", None) is not None:
            raise ValueError(FT.NO_FACES)
        xy = self.stitched_xy(cut)
        if xy is None:
            return None
        return FT.face_topography_dev(xy[0], xy[1], source, refine=refine, oversample=oversample, sea_level=sea_level)

    # -- point location -----------------------------------------------------------------------------------------------
    def locate(self, cut, lon, lat, names=None):
        """The model cells of the stitched grid that hold the points lon, lat (locate.result on rank 0, None on the other ranks), on
        rank 0's GPU with the stitched points gathered there, as coast_distance does: the same bits for any number of ranks by
        construction."""
        return self.sample(cut, lon, lat, None, names=names)

    def sample(self, cut, lon, lat, field, wet=None, mode="bilinear", fill_values=(), names=None):
        """locate() with the field ``field`` (a fields.Field or an array (..., ny, nx) on the model cells; None: nothing is sampled)
        sampled at the points, under the optional wet set ``wet``: the result's "samples" holds the values and flags."""
        from . import locate as LOC
        xy = self.stitched_xy(cut)
        if xy is None:
            return None
        return LOC.locate_dev(xy[0], xy[1], lon, lat, names=names, field=field, wet=wet, mode=mode, fill_values=fill_values)

    # -- basin codes --------------------------------------------------------------------------------------------------
    def basin_codes(self, cut, wet, rules, seed_max_km=None):
        """The basin codes (basin_codes.result on rank 0, None on the other ranks) of the model cells of the stitched grid with the wet
        set ``wet`` (one value per model cell, 0: land) under ``rules`` (a basin_codes.Rules or rows), on rank 0's GPU with the stitched
        points gathered there, as coast_distance does: the same bits for any number of ranks by construction.  The area per code of
        the summary comes from the stitched area unless the plan skips the metrics."""
        from . import basin_codes as BC
        from . import runoff as RO
        xy = self.stitched_xy(cut)
        area = None if self.plan.skip_metrics else self.stitched_area(cut)
        if xy is None:
            return None
        return BC.basin_codes_dev(xy[0], xy[1], wet, rules, seed_max_distance=None if seed_max_km is None else 1000.0 * seed_max_km,
                                  Re=float(self.plan.Re), area=None if area is None else RO.cell_area(area.cpu().numpy()))

    # -- sill depths --------------------------------------------------------------------------------------------------
    def sill_depth(self, cut, depth, wet, faces=None, seeds=(), quantum=0.01, weights="cells", min_cells=16):
        """The sill depths (sill_depth.result on rank 0, None on the other ranks) of the model cells of the stitched grid with the cell
        depths ``depth`` and the wet set ``wet`` (one value per model cell each), on rank 0's GPU with the stitched points gathered
        there, as basin_codes does: integers of the gathered plane, so the same bits for any number of ranks.  ``faces``: rank 0's
        face_topography result, for weights='faces'.  The basins' areas come from the stitched area unless the plan skips the
        metrics.  Band-sharded search is not done."""
        from . import runoff as RO
        from . import sill_depth as SD
        xy = self.stitched_xy(cut)
        area = None if self.plan.skip_metrics else self.stitched_area(cut)
        if xy is None:
            return None
        d = self.torch.from_numpy(np.ascontiguousarray(depth.cpu().numpy() if hasattr(depth, "cpu") else depth, dtype=np.float64))
        return SD.sill_depth_dev(d.to(self.device), xy[0], xy[1], wet=wet, faces=faces, seeds=seeds, quantum=quantum, weights=weights,
                                 area=None if area is None else RO.cell_area(area.cpu().numpy()), min_cells=min_cells)

    # -- processor layouts and mask tables ----------------------------------------------------------------------------
    def _layout_table(self, cut, wet, halo):
        """The layout.DeviceTable of the wet set ``wet`` (one value per model cell, 0: land) on rank 0's GPU, None on the other ranks:
        the periodic seam and the fold come from the stitched points gathered there, as basin_codes gathers them."""
        from . import fields as F
        from . import layout as LY
        from . import ocean_mask as M
        xy = self.stitched_xy(cut)
        if xy is None:
            return None
        shape = ((xy[0].shape[0] - 1) // 2, (xy[0].shape[1] - 1) // 2)
        m = F.wet_mask(wet.cpu().numpy() if hasattr(wet, "cpu") else wet, shape, "layouts")
        periodic, fold = M.topology_of_device_grid(xy[0], xy[1])
        return LY.DeviceTable(self.torch.from_numpy(m).to(self.device), periodic, fold, halo)

    def layouts(self, cut, wet, candidates=None, max_blocks=None, halo=0, min_block=2):
        """The records of the candidate layouts (layout.layouts' dict on rank 0, None on the other ranks) of the stitched grid's model
        cells with the wet set ``wet``: integers of the gathered wet set, so the same bits for any number of ranks."""
        from . import layout as LY
        t = self._layout_table(cut, wet, halo)
        return None if t is None else LY.layouts_dev(None, candidates=candidates, max_blocks=max_blocks, min_block=min_block, table=t)

    def mask_table(self, cut, wet, px, py, halo=0, xextent=None, yextent=None):
        """The mask table of the layout (px, py) (layout.mask_table's dict on rank 0, None on the other ranks), as layouts()."""
        from . import layout as LY
        t = self._layout_table(cut, wet, halo)
        return None if t is None else LY.mask_table_dev(None, px, py, xextent=xextent, yextent=yextent, table=t)

    # -- bilinear interpolation ---------------------------------------------------------------------------------------
    def stitched_angle(self, cut):
        """The stitched angle_dx ((nyp, nxp) float64 device tensor) on rank 0's device, None on the other ranks (_stitched)."""
        if self.plan.skip_metrics:
            raise ValueError("angle_dx is not computed with --skip_metrics")
        got = self._stitched(cut, ("angle_dx",), True)
        return None if got is None else got[0]

    def bilinear(self, cut, source, source2=None, points="h", mask=None, fill=True, fill_max=None, rotate=True):
        """The bilinear interpolation (bilinear.result on rank 0, None on the other ranks) of ``source`` (a remap.Source; with
        ``source2`` the eastward and northward components of a vector) at the h, u, v or c points of the stitched grid, on rank 0's
        GPU with the stitched points (and angle_dx for a vector) gathered there, as runoff does.  Every value is a function of one
        point only, so the bits are the same for any number of ranks.  A vector needs angle_dx: ValueError with --skip_metrics."""
        from . import bilinear as B
        if source2 is not None and self.plan.skip_metrics:
            raise ValueError("a vector needs angle_dx, which is not computed with --skip_metrics")
        xy = self.stitched_xy(cut)
        angle = self.stitched_angle(cut) if source2 is not None else None
        if xy is None:
            return None
        return B.bilinear_dev(xy[0], xy[1], source, source2, angle_dx=angle, points=points, mask=mask, fill=fill, fill_max=fill_max,
                              rotate=rotate)

    def bands_to_host(self):
        """This rank's bands as numpy arrays (halo rows dropped): {sub: {field: array}}."""
        out = {}
        for s in self.plan.subs:
            b = self.buf[s.name]
            out[s.name] = {f: (b[f][: b["n"]] if f in ("x", "y") else b[f]).cpu().numpy() for f in FIELDS}
        return out


def stitch(plan, per_rank_bands, guards=False):
    """Concatenate the bands of all ranks per sub-grid, apply --south_cutoff_row / _ang to the southern pieces (OGG:1268-1313), then
    stitch the sub-grids south -> north as OGG:1315-1365 (x, y, dx, angle_dx drop the southern piece's last row; dy, area are
    concatenated whole).  ``guards``: raise like the reference on a grid it rejects (OGG:1371-1375, 1425-1436)."""
    subs = {}
    for s in plan.subs:
        subs[s.name] = {f: np.concatenate([bands[s.name][f] for bands in per_rank_bands], axis=0) for f in FIELDS}
    c_sc, c_so, gone = plan.south_cut(subs["SC"]["y"][:, 0] if "SC" in subs else None)
    if gone:
        del subs["SC"]
        subs["SO"] = {f: v[c_so:, :] for f, v in subs["SO"].items()}
    elif c_sc > 0:
        subs["SC"] = {f: v[c_sc:, :] for f, v in subs["SC"].items()}
    g = None
    for s in plan.subs:
        if s.name not in subs:
            continue
        piece = subs[s.name]
        if g is None:
            g = dict(piece)
        else:
            g = {f: np.concatenate((g[f] if f in ("dy", "area") else g[f][:-1, :], piece[f]), axis=0) for f in FIELDS}
    if guards:
        check_guards(g["y"][:, plan.Ni // 4], "BP" in subs)
    g["sub"] = subs
    return g


def check_guards(ycol, has_bp):
    """The reference's final checks on column Ni//4 of the stitched latitudes (OGG:1371-1375, 1425-1436)."""
    if has_bp and np.any((np.roll(ycol, shift=-1, axis=0) - ycol) == 0):
        raise Exception("lattitude array has repeated values along symmetry meridian!")
    equator_index = np.searchsorted(ycol, 0.0)
    if equator_index == 0:
        raise Exception("   Ooops: Equator is not in the grid")
    print("   Equator is at j=", equator_index)
    if equator_index % 2 == 0:
        raise Exception("Ooops: Equator is not going to be a u-point. Use option --south_cutoff_row to one more or on less row from south.")
    if ycol.shape[0] % 2 == 0:
        raise Exception("Ooops: The number of j's in the supergrid is not even. Use option --south_cutoff_row to one more or on less row from south.")
