"""Every radial knot-table kernel of csrc/e3k_rtable.hip (and e3k_edge_records) against float64 on the CPU, element by element.

One case per C-ABI call or short chain (bins -> consumers).  A case lays every operand out in ONE arena of 4-byte words with slack on
both sides of every block.  Outputs a call overwrites start as NaN (int outputs: a sentinel), accumulated outputs as random values.
After the calls the WHOLE arena is compared: elements a call writes against a float64 reference under the bounds below, everything
else bit for bit (slack, inputs, workspace past the size the library asks for, all of the arena when a call is refused).  Only the
inside of a workspace / scratch block (its contents are not part of the ABI) is left out.  No output element is masked: a row that
must be NaN (a NaN radius) is required to be NaN in full.  References are numpy float64 written from include/e3k.h and the header
comment of e3k_rtable.hip; consumers take the device's own fp32 bin / coef / perm as their inputs -- checked by the same case BEFORE
a consumer is launched (they index memory through bin and bin_perm), and required to be unchanged afterwards.

Bounds (u = 2^-24, the fp32 unit roundoff).

bins, coef.  bin, bin_ptr, bin_seg, bin_perm are integers: equal to floor / clamp in float64, bincount / cumsum, cumsum(ceil(cnt /
  64)) and the stable argsort.  x = r * h_inv is the fp32 product (exact when h_inv is a power of two: asserted), clamped to [0, K];
  t = x - i is exact in fp32 for x >= 1/2 (Sterbenz; also for t in [1, 2] on the last interval because K >= 4 gives i >= x / 2).  A
  weight is a product of three factors of which two carry one rounding (t - 1, t - 2, t + 1), two or three multiplications and the
  rounded constant 1/6: at most seven (1 + d), |d| <= u: |c - c64| <= 8 u |c64| -- and exactly 0 where c64 = 0 (t = 0, 1, 2).  Where
  x - i is NOT exact (0 < x < 1/2 with a power of two; anywhere the fp32 subtraction of the fp32 product rounds otherwise; decided
  with a float32 model of that one subtraction, a property of the format) t is off by at most 2^-25 (|t| <= 1) and the weight by
  2^-25 |dc_k/dt| more, an absolute term.  tests/test_rtable_inventory.py shows the bound to hold for a float32 model on the CPU.
interp_fwd, interp_fwd2.  Three FMAs and a product: |w - w64| <= 4 u sum_k |c_k| |T[i - 1 + k]|.  fwd2's w is bit-equal to fwd's.
interp_bwd.  g_T[j] is an ordered sum of n_j terms c_k(e) scale[e] g_w[e] (one rounding for the scale, FMA chains per segment, the
  segments added in order): (n_j + 8) u (sum |terms| + |old|); rows without a term: exactly 0 (accumulate: exactly the old value).
pack.  (ii) rows outside [1, K - 2]: zero words.  (iii) stored halves within one fp16 ulp (2^-24 in the subnormal range) of e2 2^10 and
  c3 2^16 formed in float64 from the fp32 rows; d0, d1 within one fp32 ulp of the header's formulas evaluated with the STORED halves
  (+ 2^-50 of the rows' magnitudes: the device's double arithmetic is contracted and the sums cancel).  (iv) the record evaluated in
  float64 on a grid of s against the float64 cubic through the four fp32 rows: what fp16 dropped is r2 s^2 + r3 s^3 with |r2| <=
  2^-11 |e2| + 2^-25 / 2^10, |r3| <= 2^-11 |c3| + 2^-25 / 2^16, economised into d0, d1: r2 (s^2 - 1/8) + r3 (s^3 - 3 s / 16), plus
  the fp32 rounding of d0 and d1, u (|d0| + |s| |d1|).  On |s| <= 1/2: max |s^2 - 1/8| = 1/8, max |s^3 - 3 s / 16| = 1/32 (at 1/4 and
  1/2) -- the header's 2^-11 (|e2| / 8 + |c3| / 32).  On the two clamped intervals, |s| <= 3/2: 17/8 and 99/32 (both at 3/2).
interp_packed.  Against the stored record in float64 at s = (c2 - c0 + 2 c3) - 1/2 from the device's coef: three FMAs and the three
  roundings of s: 4 u (|d0| + |s| |d1| + s^2 |D2| 2^-10 + |s|^3 |D3| 2^-16) + 4 u (|c0| + |c2| + 2 |c3| + 1/2) |dw/ds|.
guard.  The documented estimate in float64 on the same fp32 table.  The kernel differences in fp32: per window the error of the
  bound term is at most 8 u c4 (|v0| + 4 |v1| + 6 |v2| + 4 |v3| + |v4|) (+ 8 u 2^-11 ((|v1| + 2 |v2| + |v3|) / 16 + (|v0| + 3 |v1| +
  3 |v2| + |v3|) / 192) packed), ABSOLUTE; |max a - max b| <= max |a - b| carries it to the column maxima, each division adds 4 u of
  the quotient (the floor's product, the quotient, col_weight's product).  On a rough table and on the tables with a planted spike
  the bound is 1e-6 .. 1e-2 of the estimate; on the un-spiked SMOOTH tables (guard_smooth, the second tables of guard_rows_*, the
  healthy table of guard_non_finite) it is about the estimate itself, as the fp32 differencing allows: those pin an upper bound
  (a healthy table is not vetoed) and the untouched words, not the value.  Cases that rest on a term deciding the result assert that
  premise on the reference (`premise`): a kernel without the floor or without the col_weight term misses them by >= 100 bounds.

``CASES`` is a plain table; tests/test_rtable_inventory.py holds it to the kernels the library ships (no GPU needed there).
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.util import record_measured

pytestmark = pytest.mark.gpu

E3K_OK, E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED = 0, -1, -3
U24 = 2.0 ** -24
SENT = -77777777      # int outputs start as this

BINS_K = ("rtable_bins_rank_kernel", "rtable_bins_scan_kernel", "rtable_bins_place_kernel")
CONSUMER_K = {"fwd": ("rtable_interp_fwd_kernel",), "fwd2": ("rtable_interp_fwd_kernel",),
              "bwd": ("rtable_bwd_partial_kernel", "rtable_bwd_combine_kernel"),
              "packed": ("rtable_pack_kernel", "rtable_interp_packed_kernel")}
CONSUMER_F = {"fwd": ("e3k_rtable_interp_fwd",), "fwd2": ("e3k_rtable_interp_fwd", "e3k_rtable_interp_fwd2"),
              "bwd": ("e3k_rtable_interp_bwd", "e3k_rtable_bwd_workspace_floats"), "packed": ("e3k_rtable_pack", "e3k_rtable_interp_packed")}


# ---------------------------------------------------------------------------------------------------------------------------------
# the table's vocabulary
def chain(id_, why, E, K, W, rad, cons=(), h_inv=64.0, n_keys=0, keys=None, k0=None):
    """bins (n_keys > 0: bins_keyed) then consumers: "fwd", "fwd2", "bwd" with flags after a colon (s: scale, a: accumulate),
    "packed".  rad: the radii (see _radii); keys: "some" (a key absent), "bad" (-1 and n_keys among them), or an int (all edges)."""
    kern, funcs = set(BINS_K), {"e3k_rtable_bins_keyed" if n_keys else "e3k_rtable_bins", "e3k_rtable_bins_workspace_ints"}
    for c in cons:
        kern |= set(CONSUMER_K[c.split(":")[0]])
        funcs |= set(CONSUMER_F[c.split(":")[0]])
    return dict(id=id_, kind="chain", why=why, E=E, K=K, W=W, rad=rad, cons=cons, h_inv=h_inv, n_keys=n_keys, keys=keys, k0=k0,
                kernels=kern, funcs=funcs)


def pack(id_, why, K, widths, amp=1.0):
    return dict(id=id_, kind="pack", why=why, K=K, widths=widths, amp=amp, kernels={"rtable_pack_kernel", "rtable_pack_multi_kernel"},
                funcs={"e3k_rtable_pack", "e3k_rtable_pack_multi"})


def tab(W, kind="smooth", spikes=(), colscale=None, zero_col=None, poison=None):
    """One guard table.  spikes: (row, col, added value); colscale: (col, factor); poison: (row, col, value) set, inf or NaN."""
    return dict(W=W, kind=kind, spikes=list(spikes), colscale=colscale, zero_col=zero_col, poison=poison)


def guard(id_, why, rows, tables, floor_rel=1e-3, col_weight=0.25, packed=1, singles=False, then=None, premise=None):
    """One e3k_rtable_guard call over `tables`.  singles: every table again in a call of its own, bit-equal.  then: a second call on
    the same states with these tables (the running maximum stays, the launch's estimate is replaced).  premise: what the case rests
    on, asserted on the float64 reference of table 0 with a margin of 100 bounds (see _premise)."""
    return dict(id=id_, kind="guard", why=why, rows=rows, tables=tables, floor_rel=floor_rel, col_weight=col_weight, packed=packed,
                singles=singles, then=then, premise=premise, kernels={"rtable_guard_kernel", "rtable_guard_reduce_kernel"}, funcs={"e3k_rtable_guard"})


def records(id_, why, E, d_sh, with_bin):
    return dict(id=id_, kind="records", why=why, E=E, d_sh=d_sh, with_bin=with_bin, kernels=set(), funcs={"e3k_edge_records"})


def refuse(id_, why, fn, rc, **over):
    return dict(id=id_, kind="refuse", why=why, fn=fn, rc=rc, over=over, kernels=set(), funcs={"e3k_" + fn})


def _seam_tables(rows, W, first, n):
    """n smooth tables, table j with ONE spike whose largest fourth difference (the window two rows above it) is the first window of
    row range first + j of the guard's 32 (8 parts x 4 waves)"""
    per = -(-(rows - 4) // 32)
    return [tab(W, spikes=[(min((first + j) * per + 2, rows - 1), (37 * (first + j)) % W, 1e-3)]) for j in range(n)]


GUARD_WIDTHS = [1, 63, 64, 65, 1920, 4, 60, 100, 128, 129, 252, 256, 260, 640, 2, 191]

CASES = [
    # ---- edge counts: chunk (1 024) and wave-quarter (256) seams of the rank kernel, on six usable knots so that every knot has edges
    #      in every wave and chunk
    *[chain(f"edges_{E}", "E at a lane, wave-quarter and chunk seam of the rank kernel; every knot crowded (segments of 64)", E, 8, 4,
            "uniform", ("fwd", "bwd")) for E in (1, 63, 64, 65, 1023, 1024, 1025, 4 * 1024 + 17)],
    chain("edges_0", "no edges: pointers NULL, bin_ptr / bin_seg all zero, g_T all zero", 0, 8, 4, "uniform", ("fwd", "bwd")),
    chain("radii_edge_values", "0, -0, negative, 1e-7, x < 1/2, on knots, r_max - ulp, r_max, beyond, +-inf, one NaN (NaN weights, NaN w row)",
          200, 512, 64, "edge", ("fwd", "packed"), h_inv=128.0),
    chain("radii_on_knots", "every radius on a knot: t = 0, 1, 2: weights exactly 0 or 1", 300, 16, 8, "knots", ("fwd",), h_inv=4.0),
    chain("one_knot_128", "all edges in one knot, 64 m edges: two full segments", 128, 32, 60, "knot", ("fwd", "bwd:s"), k0=7),
    chain("one_knot_129", "all edges in one knot, 64 m + 1 edges: a third segment of one edge", 129, 32, 60, "knot", ("bwd",), k0=30),
    chain("every_knot_65", "every usable knot holds 65 edges: the most segments e3k_rtable_bwd_workspace_floats must hold", 65 * 38, 40,
          8, "fill65", ("bwd:s",)),
    chain("clustered", "thousands of edges in a handful of knots (bond lengths): long segment lists per knot", 6000, 512, 64,
          "clustered", ("fwd", "bwd:s"), h_inv=128.0),
    # ---- knot counts
    chain("knots_4", "K = 4: i clamped to {1, 2}, every stencil row of a five-row table; one NaN radius", 300, 4, 4, "edge",
          ("fwd", "packed"), h_inv=1.0),
    chain("knots_4_bwd", "K = 4, finite radii: every row of the five-row g_T carries a number", 300, 4, 4, "edge_finite", ("bwd:s",),
          h_inv=1.0),
    chain("knots_5", "K = 5, finite radii", 300, 5, 8, "edge_finite", ("fwd", "bwd:a"), h_inv=2.0),
    chain("knots_1023", "1 024 rows: exactly one pass of the scan kernel", 3000, 1023, 4, "uniform", ("fwd", "bwd"), h_inv=256.0),
    chain("knots_1024", "1 025 rows: the scan kernel's second pass holds ONE row (a table after one guard refinement)", 3000, 1024, 4,
          "uniform", ("fwd", "bwd"), h_inv=256.0),
    chain("knots_4000", "the largest table: four scan passes, 64 016 bytes of LDS in the rank kernel", 5000, 4000, 4, "uniform",
          ("fwd", "bwd:s"), h_inv=1024.0),
    chain("h_inv_not_a_power_of_two", "h_inv = 7.3: x is the fp32 product, x - i rounds", 2000, 64, 4, "edge", ("fwd",), h_inv=7.3),
    # ---- widths of the float4 kernels: lane tails of bwd_partial's 256-column chunk, more than one chunk
    *[chain(f"width_{W}", "W around the 64-lane float4 row and the 256-column chunk of bwd_partial; fwd2 == fwd; scale; accumulate", 150,
            16, W, "uniform", ("fwd2", cons), h_inv=4.0)
      for W, cons in ((60, "bwd:s"), (64, "bwd:a"), (252, "bwd:sa"), (256, "bwd"), (260, "bwd:s"), (1920, "bwd:sa"))],
    *[chain(f"packed_width_{W}", "interp_packed takes any W: scalar columns", 200, 64, W, "edge", ("packed",), h_inv=16.0)
      for W in (1, 63, 65)],
    # ---- keyed tables
    chain("keyed_4x999", "four blocks of 1 000 rows; key 1 absent; a flag that holds other bits stays as it is", 3000, 999, 8, "uniform",
          ("fwd", "bwd:s"), h_inv=256.0, n_keys=4, keys="some"),
    chain("keyed_1x4000", "n_keys (K + 1) - 1 = 4 000 through the keyed entry", 1500, 4000, 4, "uniform", ("fwd",), h_inv=1024.0, n_keys=1,
          keys=0),
    chain("keyed_bad_keys", "keys -1 and n_keys: bit 3 ORed into a flag holding other bits, the edges folded into block 0", 700, 16, 8,
          "edge", ("fwd", "bwd"), h_inv=4.0, n_keys=3, keys="bad"),
    chain("keyed_one_key", "every edge under the last key: border knots of the blocks hold nothing", 500, 12, 8, "uniform", ("fwd", "bwd:a"),
          h_inv=4.0, n_keys=5, keys=4),
    # ---- the packed record
    pack("pack_smooth_256", "the smooth table of test_gpu_ops (K = 256, h = 2^-6); pack_multi == pack for mixed widths in one launch "
         "(narrower tables' extra threads write nothing)", 256, [64, 1, 63, 65, 260, 4]),
    pack("pack_tiny_columns", "columns down to 1e-7 of the largest: halves in fp16's subnormal range", 64, [24, 7], amp=1e-2),
    pack("pack_knots_4", "K = 4: two live rows, both clamped intervals", 4, [5, 64]),
    pack("pack_16_tables", "sixteen tables, the most per launch", 5, list(range(1, 17))),
    # ---- the guard
    guard("guard_rough", "independent normal rows: the comparison is tight relatively; packed term on", 641, [tab(100, "rough")]),
    guard("guard_rough_unpacked", "packed = 0: the fourth difference alone", 641, [tab(100, "rough")], packed=0),
    guard("guard_smooth", "a smooth table (as shipped): rounding of d4 is a share of d4, absolute bound", 641, [tab(192)], packed=0),
    guard("guard_seams_0_15", "the worst difference at the start of row ranges 0 .. 15, one table each", 641, _seam_tables(641, 100, 0, 16)),
    guard("guard_seams_16_31", "... and of row ranges 16 .. 31", 641, _seam_tables(641, 100, 16, 16)),
    guard("guard_ends", "the worst difference in the first row, each of the last four rows, the last column of a partial 64-chunk", 641,
          [tab(100, spikes=[(0, 5, 1e-3)]), *[tab(100, spikes=[(641 - k, 70, 1e-3)]) for k in (1, 2, 3, 4)],
           tab(100, spikes=[(300, 99, 1e-3)]), tab(65, spikes=[(17, 64, 1e-3)]), tab(1, spikes=[(320, 0, 1e-3)])]),
    guard("guard_floor_decides", "a column 1e-6 of the largest carrying the worst difference: its ratio is taken against floor_rel max|T|, "
          "a thousand times below its ratio against itself; a column exactly zero beside it", 200,
          [tab(70, colscale=(66, 1e-6), spikes=[(100, 66, 1e-9)], zero_col=3)], floor_rel=1e-3, col_weight=1.0, premise="floor_decides"),
    guard("guard_floor_below_column", "the same table under a floor of 1e-8: the small column's own maximum is the denominator", 200,
          [tab(70, colscale=(66, 1e-6), spikes=[(100, 66, 1e-9)], zero_col=3)], floor_rel=1e-8, col_weight=1.0, premise="floor_idle"),
    guard("guard_zero_table_column", "the LAST column exactly zero: 0 / floor, not 0 / 0", 200, [tab(70, zero_col=69)], col_weight=1.0),
    guard("guard_small_column_decides", "col_weight * est_c above est_g: a column 1e-2 of the largest with a spike", 200,
          [tab(70, colscale=(11, 1e-2), spikes=[(100, 11, 1e-4)])], floor_rel=1e-4, col_weight=0.5, premise="column_term_decides"),
    guard("guard_col_weight_0", "col_weight = 0 on that table: [1] is the table-wide ratio, [3] still the per-column one, far above it", 200,
          [tab(70, colscale=(11, 1e-2), spikes=[(100, 11, 1e-4)])], floor_rel=0.0, col_weight=0.0, premise="column_term_dropped"),
    guard("guard_non_finite", "inf / NaN in the first, a middle and the last row: +inf in [0], [1], [3]", 133,
          [tab(70, poison=(r, c, v)) for r, c in ((0, 0), (66, 64), (132, 69)) for v in (np.inf, np.nan)] + [tab(70)], col_weight=0.0),
    guard("guard_second_call_tamer", "a second call on a tamer table: [0] keeps the maximum, [1] and [3] are replaced", 100,
          [tab(64, "rough")], then=[tab(64)]),
    guard("guard_16_widths", "sixteen tables of different widths in one launch (grid sized by the widest) == sixteen single calls", 133,
          [tab(W, spikes=[(60 + W % 7, W - 1, 1e-4)]) for W in GUARD_WIDTHS], singles=True),
    guard("guard_rows_4", "four rows: no fourth difference, E3K_OK, nothing written", 4, [tab(64)]),
    *[guard(f"guard_rows_{rows}", "row counts around the 32 row ranges: one window in all, one per range, 33 windows over 17 ranges",
            rows, [tab(65, "rough"), tab(64)]) for rows in (5, 36, 37)],
    # ---- edge records
    records("records_sh1", "d_sh = 1 without bin / coef: zero padded", 17, 1, False),
    records("records_sh4", "d_sh = 4 with bin / coef", 17, 4, True),
    records("records_sh9_one", "d_sh = 9, one edge", 1, 9, True),
    records("records_sh9_nobin", "d_sh = 9 without bin / coef", 17, 9, False),
    records("records_empty", "E = 0: nothing written", 0, 4, True),
    # ---- refusals: the return code, and every arena bit-identical
    refuse("refuse_bins_K3", "K < 4", "rtable_bins", E3K_ERR_INVALID, K=3),
    refuse("refuse_bins_E_negative", "E < 0", "rtable_bins", E3K_ERR_INVALID, E=-1),
    refuse("refuse_bins_h_inv_0", "h_inv <= 0", "rtable_bins", E3K_ERR_INVALID, h_inv=0.0),
    refuse("refuse_bins_h_inv_nan", "h_inv NaN", "rtable_bins", E3K_ERR_INVALID, h_inv=float("nan")),
    refuse("refuse_bins_K4001", "4 002 rows", "rtable_bins", E3K_ERR_UNSUPPORTED, K=4001),
    refuse("refuse_bins_E_2_31", "E >= 2^31 with small buffers: refused before any pointer is read", "rtable_bins", E3K_ERR_UNSUPPORTED,
           E=2 ** 31),
    refuse("refuse_bins_null_r", "r NULL with E > 0", "rtable_bins", E3K_ERR_INVALID, r=None),
    refuse("refuse_bins_null_ptr", "bin_ptr NULL", "rtable_bins", E3K_ERR_INVALID, ptr=None),
    refuse("refuse_keyed_n_keys_0", "n_keys < 1", "rtable_bins_keyed", E3K_ERR_INVALID, n_keys=0),
    refuse("refuse_keyed_rows_4002", "2 x 2 001 stacked rows: one over", "rtable_bins_keyed", E3K_ERR_UNSUPPORTED, n_keys=2, K=2000),
    refuse("refuse_keyed_null_key", "key NULL with E > 0", "rtable_bins_keyed", E3K_ERR_INVALID, key=None),
    refuse("refuse_fwd_W6", "W % 4 != 0", "rtable_interp_fwd", E3K_ERR_UNSUPPORTED, W=6),
    refuse("refuse_fwd_W0", "W <= 0", "rtable_interp_fwd", E3K_ERR_INVALID, W=0),
    refuse("refuse_fwd_K3", "K < 4", "rtable_interp_fwd", E3K_ERR_INVALID, K=3),
    refuse("refuse_fwd_null_T", "T NULL", "rtable_interp_fwd", E3K_ERR_INVALID, T=None),
    refuse("refuse_fwd_E_2_31", "E >= 2^31: bin_perm holds int32 edge ids", "rtable_interp_fwd", E3K_ERR_UNSUPPORTED, E=2 ** 31),
    refuse("refuse_fwd2_W6", "W % 4 != 0", "rtable_interp_fwd2", E3K_ERR_UNSUPPORTED, W=6),
    refuse("refuse_fwd2_null_T2", "T2 NULL", "rtable_interp_fwd2", E3K_ERR_INVALID, T2=None),
    refuse("refuse_fwd2_E_2_31", "E >= 2^31", "rtable_interp_fwd2", E3K_ERR_UNSUPPORTED, E=2 ** 31),
    refuse("refuse_bwd_W6", "W % 4 != 0", "rtable_interp_bwd", E3K_ERR_UNSUPPORTED, W=6),
    refuse("refuse_bwd_E_negative", "E < 0", "rtable_interp_bwd", E3K_ERR_INVALID, E=-5),
    refuse("refuse_bwd_null_ws", "workspace NULL", "rtable_interp_bwd", E3K_ERR_INVALID, wsb=None),
    refuse("refuse_bwd_E_2_31", "E >= 2^31", "rtable_interp_bwd", E3K_ERR_UNSUPPORTED, E=2 ** 31),
    refuse("refuse_pack_K3", "K < 4", "rtable_pack", E3K_ERR_INVALID, K=3),
    refuse("refuse_pack_W0", "W <= 0", "rtable_pack", E3K_ERR_INVALID, W=0),
    refuse("refuse_pack_null_P", "P NULL", "rtable_pack", E3K_ERR_INVALID, P=None),
    refuse("refuse_pack_multi_17", "n > 16", "rtable_pack_multi", E3K_ERR_INVALID, n=17),
    refuse("refuse_pack_multi_W0", "a table of width 0", "rtable_pack_multi", E3K_ERR_INVALID, W=0),
    refuse("refuse_packed_K3", "K < 4", "rtable_interp_packed", E3K_ERR_INVALID, K=3),
    refuse("refuse_packed_null_w", "w NULL", "rtable_interp_packed", E3K_ERR_INVALID, w=None),
    refuse("refuse_packed_E_2_31", "E >= 2^31", "rtable_interp_packed", E3K_ERR_UNSUPPORTED, E=2 ** 31),
    refuse("refuse_guard_n0", "n = 0", "rtable_guard", E3K_ERR_INVALID, n=0),
    refuse("refuse_guard_n17", "n = 17", "rtable_guard", E3K_ERR_INVALID, n=17),
    refuse("refuse_guard_floor_negative", "floor_rel < 0", "rtable_guard", E3K_ERR_INVALID, floor_rel=-1e-3),
    refuse("refuse_guard_floor_nan", "floor_rel NaN", "rtable_guard", E3K_ERR_INVALID, floor_rel=float("nan")),
    refuse("refuse_guard_col_weight_negative", "col_weight < 0", "rtable_guard", E3K_ERR_INVALID, col_weight=-0.5),
    refuse("refuse_guard_col_weight_nan", "col_weight NaN", "rtable_guard", E3K_ERR_INVALID, col_weight=float("nan")),
    refuse("refuse_guard_W0", "a table of width 0", "rtable_guard", E3K_ERR_INVALID, W=0),
    refuse("refuse_records_misaligned", "rec not 64-byte aligned", "edge_records", E3K_ERR_INVALID, rec_shift=4),
    refuse("refuse_records_bin_without_coef", "bin without coef", "edge_records", E3K_ERR_INVALID, coef=None),
    refuse("refuse_records_d_sh_10", "d_sh > 9", "edge_records", E3K_ERR_INVALID, d_sh=10),
    refuse("refuse_records_E_2_31", "E >= 2^31", "edge_records", E3K_ERR_UNSUPPORTED, E=2 ** 31),
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references (tests/test_rtable_inventory.py runs the first two against float32 models on the CPU)
def lagrange64(t):
    """the four cubic Lagrange weights on nodes -1, 0, 1, 2 at t, and their derivatives"""
    a, b, c, d = t + 1, t, t - 1, t - 2
    w = np.stack([-b * c * d / 6, a * c * d / 2, -a * b * d / 2, a * b * c / 6], -1)
    dw = np.stack([-(c * d + b * d + b * c) / 6, (c * d + a * d + a * c) / 2, -(b * d + a * d + a * b) / 2, (b * c + a * c + a * b) / 6], -1)
    return w, dw


def bins_reference(r32, h_inv, K):
    """knot i [E], weights [E, 4], bound [E, 4] and the NaN rows of e3k_rtable_bins' per-edge part"""
    with np.errstate(over="ignore", invalid="ignore"):      # (3e38 h_inv = +inf, as on the device; inf * h_inv, NaN)
        x32 = r32.astype(np.float32) * np.float32(h_inv)
    x32 = np.minimum(np.maximum(x32, np.float32(0)), np.float32(K))      # (NaN stays NaN)
    nan = np.isnan(x32)
    x = x32.astype(np.float64)
    i = np.clip(np.floor(np.where(nan, 1.0, x)), 1, K - 2)
    t = x - i
    c, dc = lagrange64(t)
    inexact = (x32 - i.astype(np.float32)).astype(np.float64) != t
    bound = 8 * U24 * np.abs(c) + np.where(inexact, 2.0 ** -25, 0.0)[:, None] * np.abs(dc)
    return i.astype(np.int64), c, bound, nan


def smooth_table(K, W, amp=1.0):
    """sin(r (1 + 5 c / W)) exp(-r / 5) on K + 1 knots of [0, 4] (test_gpu_ops' smooth table: K = 256, h = 2^-6), fp32; amp < 1: column c
    scaled by amp^(c % 4)"""
    r = np.arange(K + 1, dtype=np.float64)[:, None] * (4.0 / K)
    c = np.arange(W, dtype=np.float64)[None, :]
    return (np.sin(r * (1.0 + 5.0 * c / W)) * np.exp(-0.2 * r) * amp ** (np.arange(W) % 4)[None, :]).astype(np.float32)


def taylor64(T32, K):
    """rows 1 .. K - 2 of a table [K + 1, W]: (b, c1, c2, c3, e2, mag) of the cubic through rows i - 1 .. i + 2 in float64"""
    T = T32.astype(np.float64)
    a, b, c, d = T[0:K - 2], T[1:K - 1], T[2:K], T[3:K + 1]
    c1 = -a / 3 - b / 2 + c - d / 6
    c2 = a / 2 - b + c / 2
    c3 = -a / 6 + b / 2 - c / 2 + d / 6
    return b, c1, c2, c3, c2 + 1.5 * c3, np.abs(a) + np.abs(b) + np.abs(c) + np.abs(d)


def _ulp16(v):
    return np.maximum(np.spacing(np.abs(v).astype(np.float16)).astype(np.float64), 2.0 ** -24)


def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def decode_record(P_u32, K, W):
    """d0, d1 [K + 1, W] float64 and the halves D2, D3 (still scaled) of a packed table given as uint32 words [(K + 1) 3 W]"""
    P = P_u32.reshape(K + 1, 3 * W)
    pair = P[:, :2 * W].copy().view(np.float32).reshape(K + 1, W, 2).astype(np.float64)
    hh = P[:, 2 * W:]
    D2 = (hh & 0xffff).astype(np.uint16).view(np.float16).astype(np.float64)
    D3 = (hh >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    return pair[..., 0], pair[..., 1], D2, D3


def check_record(P_u32, T32, K, W):
    """Everything the header promises of a packed table; returns the worst error / bound of (iii) and (iv)"""
    P = P_u32.reshape(K + 1, 3 * W)
    for i in (0, K - 1, K):
        assert not P[i].any(), f"row {i} of the packed table is not all zero"
    d0, d1, D2, D3 = (v[1:K - 1] for v in decode_record(P_u32, K, W))
    b, c1, c2, c3, e2, mag = taylor64(T32, K)
    assert np.isfinite(D2).all() and np.isfinite(D3).all()
    # (iii) the stored halves, then d0 and d1 from the STORED halves
    r_h = max(float((np.abs(D2 - e2 * 1024.0) / _ulp16(e2 * 1024.0)).max()), float((np.abs(D3 - c3 * 65536.0) / _ulp16(c3 * 65536.0)).max()))
    assert r_h <= 1.0, f"a stored fp16 half is {r_h} ulp from its float64 value"
    r2, r3 = e2 - D2 / 1024.0, c3 - D3 / 65536.0
    d0_ref = b + c1 / 2 + c2 / 4 + c3 / 8 + r2 / 8
    d1_ref = c1 + c2 + 0.75 * c3 + 3.0 * r3 / 16
    r_d = max(float((np.abs(d0 - d0_ref) / (_ulp32(d0_ref) + 2.0 ** -50 * mag + 1e-300)).max()),
              float((np.abs(d1 - d1_ref) / (_ulp32(d1_ref) + 2.0 ** -50 * mag + 1e-300)).max()))
    assert r_d <= 1.0, f"d0 / d1 are {r_d} fp32 ulp from the header's formulas"
    # (iv) the promise: the record against the cubic.  Rows 1 and K - 2 also over their clamped interval.
    worst = 0.0
    q2, q3 = 2.0 ** -25 / 1024.0, 2.0 ** -25 / 65536.0
    for lo, hi, m2, m3, rows in ((-0.5, 0.5, 1 / 8, 1 / 32, slice(None)), (-1.5, -0.5, 17 / 8, 99 / 32, slice(0, 1)),
                                 (0.5, 1.5, 17 / 8, 99 / 32, slice(K - 3, K - 2))):
        for s in np.linspace(lo, hi, 17):
            t = s + 0.5
            rec = d0[rows] + s * (d1[rows] + s * (D2[rows] / 1024.0 + s * D3[rows] / 65536.0))
            cub = b[rows] + t * (c1[rows] + t * (c2[rows] + t * c3[rows]))
            bnd = (2.0 ** -11 * np.abs(e2[rows]) + q2) * m2 + (2.0 ** -11 * np.abs(c3[rows]) + q3) * m3 \
                + U24 * (np.abs(d0[rows]) + abs(s) * np.abs(d1[rows]))
            ratio = float((np.abs(rec - cub) / bnd).max())
            assert ratio <= 1.0, f"the packed record is {ratio} of its bound from the cubic at s = {s}"
            worst = max(worst, ratio)
    return max(r_h, r_d), worst


def _premise(kind, T32, floor_rel, col_weight, packed):
    """what a guard case rests on, on the float64 reference alone"""
    est, est_c, b_est, b_c = guard_reference(T32, floor_rel, col_weight, packed)
    if kind in ("floor_decides", "floor_idle"):
        other = 0.0 if kind == "floor_decides" else 1e-3      # (no floor at all / the floor of guard_floor_decides)
        _, alt_c, _, alt_b = guard_reference(T32, other, col_weight, packed)
        assert abs(alt_c - est_c) > 100 * (b_c + alt_b), f"the floor does not move est_c: {est_c} and {alt_c}"
        if kind == "floor_idle":
            assert est_c == guard_reference(T32, 0.0, col_weight, packed)[1], "the floor must lie below the column's own maximum"
    else:
        assert kind in ("column_term_decides", "column_term_dropped")
        cw = col_weight if kind == "column_term_decides" else 0.5      # (guard_small_column_decides' weight)
        with_term, _, b1, _ = guard_reference(T32, floor_rel, cw, packed)
        est_g, _, b0, _ = guard_reference(T32, floor_rel, 0.0, packed)
        assert with_term - est_g > 100 * (b0 + b1), f"col_weight * est_c does not decide: {with_term} over {est_g}"


def guard_table(t, rows, rng):
    W = t["W"]
    if t["kind"] == "rough":
        T = rng.standard_normal((rows, W)).astype(np.float32)
    else:
        r = np.arange(rows, dtype=np.float64)[:, None] * (5.0 / 640)
        c = np.arange(W, dtype=np.float64)[None, :]
        T = (np.sin(r * (1.0 + 5.0 * c / W) + c) * np.exp(-0.2 * r)).astype(np.float32)
    if t["colscale"]:
        T[:, t["colscale"][0]] *= np.float32(t["colscale"][1])
    if t["zero_col"] is not None:
        T[:, t["zero_col"]] = 0.0
    for r_, c_, v in t["spikes"]:
        T[r_, c_] += np.float32(v)
    if t["poison"]:
        T[t["poison"][0], t["poison"][1]] = t["poison"][2]
    return T


def guard_reference(T32, floor_rel, col_weight, packed):
    """(est, est_c) and their bounds for a table [rows, W], rows >= 5"""
    if not np.isfinite(T32).all():
        return np.inf, np.inf, 0.0, 0.0
    T = T32.astype(np.float64)
    A = np.abs(T)
    v0, v1, v2, v3, v4 = (T[k:len(T) - 4 + k] for k in range(5))
    a0, a1, a2, a3, a4 = (A[k:len(T) - 4 + k] for k in range(5))
    c4, pw = 3.0 / 128.0, (1.0 if packed else 0.0) / 2048.0
    term = c4 * np.abs(v4 + v0 - 4 * (v3 + v1) + 6 * v2) + pw * (np.abs(v1 + v3 - 2 * v2) / 16 + np.abs(v3 - v0 - 3 * (v2 - v1)) / 192)
    d_term = 8 * U24 * (c4 * (a0 + 4 * a1 + 6 * a2 + 4 * a3 + a4) + pw * ((a1 + 2 * a2 + a3) / 16 + (a0 + 3 * a1 + 3 * a2 + a3) / 192))
    dmax, d_dmax, cmax = term.max(0), d_term.max(0), A.max(0)
    g = cmax.max()
    fl = max(float(np.float32(floor_rel)) * g, 1e-30)
    den_c = np.maximum(cmax, fl)
    est_c, b_c = (dmax / den_c).max(), (d_dmax / den_c + 4 * U24 * dmax / den_c).max()
    est_g, b_g = dmax.max() / max(g, 1e-30), (d_dmax / max(g, 1e-30)).max() + 4 * U24 * dmax.max() / max(g, 1e-30)
    cw = float(np.float32(col_weight))
    est = max(est_g, cw * est_c)
    return est, est_c, max(b_g, cw * b_c) + 4 * U24 * est, b_c


# ---------------------------------------------------------------------------------------------------------------------------------
# the arena: blocks of 4-byte words, slack in front of every block and after the last
class Arena:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.n = 0
        self.blocks, self.inits = {}, []

    def alloc(self, name, n, init=None, align=4, shift=0):
        """n words; init: an array of 4-byte elements, or a scalar for the whole block; otherwise random floats"""
        self.n += 5 + int(self.rng.integers(0, 9))
        self.n = -(-self.n // align) * align + shift
        self.blocks[name] = (self.n, int(n))
        if init is not None:
            self.inits.append((name, init))
        self.n += int(n)
        return self

    def upload(self, dev):
        self.x0 = self.rng.standard_normal(self.n + 32).astype(np.float32).view(np.int32)
        for name, init in self.inits:
            off, n = self.blocks[name]
            v = np.asarray(init)
            self.x0[off:off + n] = v.ravel().view(np.int32) if v.ndim else np.full(n, v).astype(v.dtype).view(np.int32)
        self.buf = torch.from_numpy(self.x0.copy()).to(dev)
        self.base = self.buf.data_ptr()
        assert self.base % 64 == 0
        return self

    def p(self, name):
        return None if name is None else self.base + 4 * self.blocks[name][0]

    def host(self, name, dtype=np.float32):
        off, n = self.blocks[name]
        return self.x0[off:off + n].view(dtype)


class Check:
    """the arena after the calls: every word is claimed by exactly one comparison or must be unchanged"""

    def __init__(self, ar, case):
        torch.cuda.synchronize()
        self.ar, self.case = ar, case
        self.got = ar.buf.cpu().numpy()
        self.claimed = np.zeros(len(self.got), bool)
        self.ratios = {}

    def dev(self, name, dtype=np.int32):
        off, n = self.ar.blocks[name]
        return self.got[off:off + n].view(dtype)

    def _claim(self, name, n=None):
        off, size = self.ar.blocks[name]
        n = size if n is None else n
        assert n <= size and not self.claimed[off:off + n].any(), name
        self.claimed[off:off + n] = True

    def free(self, name, n):
        """the first n words of a workspace: contents not part of the ABI"""
        self._claim(name, n)

    def exact(self, name, want):
        want = np.ascontiguousarray(want).ravel().view(np.int32)
        self._claim(name, len(want))
        bad = np.flatnonzero(self.dev(name)[:len(want)] != want)
        assert len(bad) == 0, f"{name}: {len(bad)} of {len(want)} words differ, first at {bad[:5]}: got {self.dev(name)[bad[:5]]}, want {want[bad[:5]]}"

    def close(self, name, want, bound, family):
        """float outputs: |got - want| <= bound elementwise; where want is NaN the output must be NaN"""
        want, bound = np.asarray(want, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
        self._claim(name, len(want))
        got = self.dev(name, np.float32)[:len(want)].astype(np.float64)
        nan = np.isnan(want)
        err = np.abs(got - np.where(nan, 0.0, want))
        ok = np.where(nan, np.isnan(got), np.isfinite(got) & (err <= bound))
        if not ok.all():
            bad = np.flatnonzero(~ok)
            pytest.fail(f"{name}: {len(bad)} of {len(want)} outputs outside the bound; first at {bad[:5]}: got {got[bad[:5]]}, "
                        f"want {want[bad[:5]]}, bound {bound[bad[:5]]}")
        live = ~nan & (bound > 0)
        self.ratio(family, float((err[live] / bound[live]).max()) if live.any() else 0.0)

    def ratio(self, family, r):
        self.ratios[family] = max(self.ratios.get(family, 0.0), r)

    def unchanged(self):
        same = self.got[~self.claimed] == self.ar.x0[~self.claimed]
        assert same.all(), f"{int((~same).sum())} words outside the outputs changed, first at {np.flatnonzero(~self.claimed)[~same][:5]} " \
                           f"(blocks: {self.ar.blocks})"

    def finish(self):
        self.unchanged()
        for family, r in self.ratios.items():
            print(f"{self.case['id']}: {family} worst error / bound {r:.3f}")
            record_measured("test_gpu_rtable_matrix", case=self.case["id"], family=family, error_over_bound=r)


# ---------------------------------------------------------------------------------------------------------------------------------
def _radii(c, rng):
    E, K, h = c["E"], c["K"], 1.0 / c["h_inv"]
    r_max = np.float32(K * h)
    kind = c["rad"]
    if kind == "uniform":
        r = rng.uniform(0.0, 1.08 * K * h, E)
    elif kind == "knots":
        r = rng.integers(0, K + 1, E) * h
    elif kind == "knot":
        r = (c["k0"] + rng.uniform(0.0, 1.0, E)) * h
    elif kind == "fill65":
        r = rng.permutation(np.repeat(np.arange(1, K - 1), 65) + rng.uniform(0.0, 1.0, E)) * h
    elif kind == "clustered":
        r = rng.choice([0.27, 0.38, 0.36, 0.30, 0.62], E) * K * h + 0.001 * K * h * rng.standard_normal(E)
    else:
        assert kind in ("edge", "edge_finite")
        special = [0.0, -0.0, -1.0, 1e-7, 0.25 * h, 0.49 * h, 0.5 * h, h, 2 * h, (K - 2) * h, (K - 1) * h, np.nextafter(r_max, np.float32(0)),
                   r_max, np.nextafter(r_max, np.float32(np.inf)), 1.5 * K * h, 3e38, np.inf, -np.inf, np.nan]
        r = rng.uniform(0.0, 1.08 * K * h, E)
        if kind == "edge_finite":      # (no NaN: a NaN radius turns the four g_T rows of its stencil into NaN)
            special = special[:-1]
        r[rng.permutation(E)[:len(special)]] = special[:E]
    return r.astype(np.float32)


def _keys(c, rng):
    E, nk, kind = c["E"], c["n_keys"], c["keys"]
    if kind == "some":
        return rng.choice([k for k in range(nk) if k != 1], E).astype(np.int64)
    if kind == "bad":
        key = rng.integers(0, nk, E).astype(np.int64)
        key[rng.permutation(E)[:40]] = np.tile([-1, nk, -2 ** 40, 2 ** 33], 10)
        return key
    return np.full(E, kind, np.int64)


def run_chain(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    ar = Arena(zlib.crc32(c["id"].encode()))
    rng = ar.rng
    E, K, W, nk, h_inv = c["E"], c["K"], c["W"], max(c["n_keys"], 1), c["h_inv"]
    keyed = c["n_keys"] > 0
    KT = nk * (K + 1) - 1                      # the stacked table's last row: what every consumer takes as K
    r = _radii(c, rng)
    key = _keys(c, rng) if keyed else None
    ws_n = lib.e3k_rtable_bins_workspace_ints(E, KT)
    assert ws_n == E + -(-E // 1024) * (KT + 1)
    ar.alloc("r", E, r).alloc("bin", E, np.int32(SENT)).alloc("coef", 4 * E, np.float32(np.nan)).alloc("ptr", KT + 2, np.int32(SENT))
    ar.alloc("seg", KT + 2, np.int32(SENT)).alloc("perm", E, np.int32(SENT)).alloc("ws", ws_n)
    if keyed:
        ar.alloc("key", 2 * E, key.view(np.int32)).alloc("flag", 1, np.int32(0x15))
    cons = [(x.split(":")[0], x.split(":")[1] if ":" in x else "") for x in c["cons"]]
    names = [n for n, _ in cons]
    rows = KT + 1
    if "fwd" in names or "fwd2" in names:
        ar.alloc("T", rows * W).alloc("w", E * W, np.float32(np.nan))
    if "fwd2" in names:
        ar.alloc("T2", rows * W).alloc("wb", E * W, np.float32(np.nan)).alloc("w2", E * W, np.float32(np.nan))
    flags = dict(cons).get("bwd", "")
    if "bwd" in names:
        wsb_n = lib.e3k_rtable_bwd_workspace_floats(E, KT, W)
        assert wsb_n == (E // 64 + KT + 2) * 4 * W
        ar.alloc("gw", E * W).alloc("wsb", wsb_n)
        if "s" in flags:
            ar.alloc("scale", E)
        old = rng.standard_normal(rows * W).astype(np.float32) if "a" in flags else np.float32(np.nan)
        ar.alloc("gT", rows * W, old).alloc("gT_again", rows * W, old)
    if "packed" in names:
        ar.alloc("Ts", rows * W, smooth_table(KT, W)).alloc("P", rows * 3 * W, np.float32(np.nan)).alloc("wp", E * W, np.float32(np.nan))
    ar.upload(dev)
    nul = (lambda n: ar.p(n) if E > 0 else None)
    if keyed:
        rc = lib.e3k_rtable_bins_keyed(nul("r"), nul("key"), nk, E, h_inv, K, nul("bin"), nul("coef"), ar.p("ptr"), ar.p("seg"), nul("perm"),
                                       nul("ws"), ar.p("flag"), st)
    else:
        rc = lib.e3k_rtable_bins(nul("r"), E, h_inv, K, nul("bin"), nul("coef"), ar.p("ptr"), ar.p("seg"), nul("perm"), nul("ws"), st)
    assert rc == E3K_OK, f"bins: {rc}"
    # ---- bins: checked BEFORE any consumer is launched (the consumers index memory through bin and bin_perm)
    ck = Check(ar, c)
    i_ref, c_ref, c_bnd, nan = bins_reference(r, h_inv, K)
    if float(np.log2(h_inv)).is_integer():
        fin = np.abs(r) < 1e30      # (3e38 h_inv overflows to +inf in fp32, as on the device: x = K)
        assert np.array_equal((r[fin] * np.float32(h_inv)).astype(np.float64), r[fin].astype(np.float64) * h_inv)
    block = np.zeros(E, np.int64)
    if keyed:
        good = (key >= 0) & (key < nk)
        block = np.where(good, key, 0)
        ck.exact("flag", np.int32(0x15 if good.all() else 0x15 | 8))
    bin_dev = ck.dev("bin").astype(np.int64)
    if nan.any():      # (the knot of a NaN radius is whatever the cast gives, CLAMPED: any usable knot of its block)
        local = bin_dev[nan] - block[nan] * (K + 1)
        assert ((local >= 1) & (local <= K - 2)).all(), f"a NaN radius has knot {local}"
        i_ref[nan] = local
    bin_ref = block * (K + 1) + i_ref
    ck.exact("bin", bin_ref.astype(np.int32))
    ck.close("coef", np.where(nan[:, None], np.nan, c_ref), c_bnd, "bins")
    cnt = np.bincount(bin_ref, minlength=KT + 1)
    assert len(cnt) == KT + 1
    ck.exact("ptr", np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
    ck.exact("seg", np.concatenate([[0], np.cumsum(-(-cnt // 64))]).astype(np.int32))
    ck.exact("perm", np.argsort(bin_ref, kind="stable").astype(np.int32))
    ck.free("ws", ws_n)
    ck.unchanged()
    first = ck

    # ---- consumers, on the device's own bin / coef / perm
    if "fwd" in names or "fwd2" in names:
        assert lib.e3k_rtable_interp_fwd(nul("T"), nul("perm"), nul("bin"), nul("coef"), E, KT, W, nul("w"), st) == E3K_OK
    if "fwd2" in names:
        assert lib.e3k_rtable_interp_fwd2(ar.p("T"), ar.p("T2"), ar.p("perm"), ar.p("bin"), ar.p("coef"), E, KT, W, ar.p("wb"), ar.p("w2"),
                                          st) == E3K_OK
    if "bwd" in names:
        for out in ("gT", "gT_again"):
            assert lib.e3k_rtable_interp_bwd(nul("gw"), nul("coef"), ar.p("scale") if "s" in flags else None, ar.p("ptr"), ar.p("seg"),
                                             nul("perm"), E, KT, W, ar.p("wsb"), ar.p(out), 1 if "a" in flags else 0, st) == E3K_OK
    if "packed" in names:
        assert lib.e3k_rtable_pack(ar.p("Ts"), KT, W, ar.p("P"), st) == E3K_OK
        assert lib.e3k_rtable_interp_packed(ar.p("P"), nul("perm"), nul("bin"), nul("coef"), E, KT, W, nul("wp"), st) == E3K_OK
    ck = Check(ar, c)
    ck.ratios = first.ratios
    for name in ("bin", "coef", "ptr", "seg", "perm") + (("flag",) if keyed else ()):
        ck.exact(name, first.dev(name))
    ck.free("ws", ws_n)
    coef = ck.dev("coef", np.float32).reshape(E, 4).astype(np.float64)
    stencil = bin_ref[:, None] - 1 + np.arange(4)[None, :]
    assert E == 0 or (stencil.min() >= 0 and stencil.max() <= KT)

    def interp(table32):
        T = table32.reshape(rows, W).astype(np.float64)
        w, b = np.zeros((E, W)), np.zeros((E, W))
        for k in range(4):
            w += coef[:, k:k + 1] * T[stencil[:, k]]
            b += np.abs(coef[:, k:k + 1] * T[stencil[:, k]])
        return w, 4 * U24 * np.where(np.isnan(b), 0.0, b)

    if "fwd" in names or "fwd2" in names:
        ck.close("w", *interp(ar.host("T")), "interp_fwd")
    if "fwd2" in names:
        ck.exact("wb", ck.dev("w"))
        ck.close("w2", *interp(ar.host("T2")), "interp_fwd")
    if "bwd" in names:
        gw = ar.host("gw").reshape(E, W).astype(np.float64)
        sc = ar.host("scale").astype(np.float64) if "s" in flags else np.ones(E)
        old = ar.host("gT").reshape(rows, W).astype(np.float64) if "a" in flags else np.zeros((rows, W))
        want, mag, n_j = old.copy(), np.abs(old), np.zeros(rows)
        for k in range(4):
            term = (coef[:, k] * sc)[:, None] * gw
            np.add.at(want, stencil[:, k], term)
            np.add.at(mag, stencil[:, k], np.abs(term))
            np.add.at(n_j, stencil[:, k], 1.0)
        bnd = np.where((n_j[:, None] > 0) & ~np.isnan(mag), (n_j[:, None] + 8) * U24 * mag, 0.0)      # (a NaN radius: its four rows NaN)
        ck.close("gT", want, bnd, "interp_bwd")
        ck.exact("gT_again", ck.dev("gT"))
        ck.free("wsb", wsb_n)
    if "packed" in names:
        r_rec, r_cub = check_record(ck.dev("P", np.uint32), ar.host("Ts").reshape(rows, W), KT, W)
        ck.ratio("pack_stored", r_rec)
        ck.ratio("pack_promise", r_cub)
        ck._claim("P")
        d0, d1, D2, D3 = (v[bin_ref] for v in decode_record(ck.dev("P", np.uint32), KT, W))
        s = ((coef[:, 2] - coef[:, 0] + 2 * coef[:, 3]) - 0.5)[:, None]
        want = d0 + s * (d1 + s * (D2 / 1024.0 + s * D3 / 65536.0))
        dw = d1 + 2 * s * D2 / 1024.0 + 3 * s * s * D3 / 65536.0
        bnd = 4 * U24 * (np.abs(d0) + np.abs(s * d1) + s * s * np.abs(D2) / 1024.0 + np.abs(s) ** 3 * np.abs(D3) / 65536.0) \
            + 4 * U24 * (np.abs(coef[:, 0]) + np.abs(coef[:, 2]) + 2 * np.abs(coef[:, 3]) + 0.5)[:, None] * np.abs(dw)
        ck.close("wp", want, np.where(np.isnan(bnd), 0.0, bnd), "interp_packed")
    ck.finish()


def run_pack(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    ar = Arena(zlib.crc32(c["id"].encode()))
    K, widths = c["K"], c["widths"]
    for j, W in enumerate(widths):
        ar.alloc(f"T{j}", (K + 1) * W, smooth_table(K, W, c["amp"])).alloc(f"P{j}", (K + 1) * 3 * W, np.float32(np.nan))
        ar.alloc(f"M{j}", (K + 1) * 3 * W, np.float32(np.nan))
    ar.upload(dev)
    n = len(widths)
    for j, W in enumerate(widths):
        assert lib.e3k_rtable_pack(ar.p(f"T{j}"), K, W, ar.p(f"P{j}"), st) == E3K_OK
    Ts = (C.c_void_p * n)(*[ar.p(f"T{j}") for j in range(n)])
    Ms = (C.c_void_p * n)(*[ar.p(f"M{j}") for j in range(n)])
    Ws = (C.c_int32 * n)(*widths)
    assert lib.e3k_rtable_pack_multi(Ts, K, Ws, Ms, n, st) == E3K_OK
    assert lib.e3k_rtable_pack_multi(None, K, None, None, 0, st) == E3K_OK      # (no tables: nothing to do)
    ck = Check(ar, c)
    for j, W in enumerate(widths):
        r_rec, r_cub = check_record(ck.dev(f"P{j}", np.uint32), ar.host(f"T{j}").reshape(K + 1, W), K, W)
        ck.ratio("pack_stored", r_rec)
        ck.ratio("pack_promise", r_cub)
        ck._claim(f"P{j}")
        ck.exact(f"M{j}", ck.dev(f"P{j}"))
    ck.finish()


def run_guard(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    ar = Arena(zlib.crc32(c["id"].encode()))
    rows = c["rows"]
    rounds = [c["tables"]] + ([c["then"]] if c["then"] else [])
    n = len(c["tables"])
    state0 = np.array([1e-9, np.nan, 123.25, np.nan], np.float32)      # [0]: an old maximum below any estimate here; [2]: not ours
    tables = [[guard_table(t, rows, ar.rng) for t in tabs] for tabs in rounds]
    for k, tabs in enumerate(tables):
        for j, T in enumerate(tabs):
            ar.alloc(f"T{k}_{j}", T.size, T)
    for j, t in enumerate(c["tables"]):
        ar.alloc(f"state{j}", 4, state0).alloc(f"scratch{j}", 16 * t["W"])
        if c["singles"]:
            ar.alloc(f"state_single{j}", 4, state0).alloc(f"scratch_single{j}", 16 * t["W"])
    ar.upload(dev)

    def call(k, js, sfx=""):
        m = len(js)
        return lib.e3k_rtable_guard((C.c_void_p * m)(*[ar.p(f"T{k}_{j}") for j in js]), (C.c_void_p * m)(*[ar.p(f"state{sfx}{j}") for j in js]),
                                    (C.c_void_p * m)(*[ar.p(f"scratch{sfx}{j}") for j in js]),
                                    (C.c_int32 * m)(*[rounds[k][j]["W"] for j in js]), m, rows, c["floor_rel"], c["col_weight"], c["packed"], st)

    assert call(0, range(n)) == E3K_OK
    if c["singles"]:
        for j in range(n):
            assert call(0, [j], "_single") == E3K_OK
    mid = None
    if c["then"]:
        torch.cuda.synchronize()
        mid = ar.buf.cpu().numpy().copy()
        assert call(1, range(n)) == E3K_OK
    ck = Check(ar, c)
    for j in range(n):
        if rows < 5:
            continue      # (nothing written: the whole arena is compared bit for bit)
        got = ck.dev(f"state{j}", np.float32)
        k = len(rounds) - 1
        est, est_c, b_est, b_c = guard_reference(tables[k][j], c["floor_rel"], c["col_weight"], c["packed"])
        if c["premise"] and j == 0:
            _premise(c["premise"], tables[0][0], c["floor_rel"], c["col_weight"], c["packed"])
        first = state0[0]
        if mid is not None:      # (the first call's estimate: checked against the device's own value of that call, itself held below)
            off = ar.blocks[f"state{j}"][0]
            after_first = mid[off:off + 4].view(np.float32)
            e0, ec0, b0, bc0 = guard_reference(tables[0][j], c["floor_rel"], c["col_weight"], c["packed"])
            assert abs(float(after_first[1]) - e0) <= b0 and abs(float(after_first[3]) - ec0) <= bc0 and after_first[0] == after_first[1]
            assert e0 > est + b0 + b_est, "the second table must be the tamer one"
            first = after_first[0]
        if np.isinf(est):
            ck.exact(f"state{j}", np.array([np.inf, np.inf, state0[2], np.inf], np.float32))
        else:
            ck._claim(f"state{j}")
            assert got[0] == max(first, got[1]), f"table {j}: running maximum {got[0]} after {first} and {got[1]}"
            assert got[2:3].view(np.int32) == state0[2:3].view(np.int32), f"table {j}: state[2] changed"
            assert np.isfinite(got[1]) and abs(float(got[1]) - est) <= b_est, f"table {j}: est {got[1]}, want {est} +- {b_est}"
            assert np.isfinite(got[3]) and abs(float(got[3]) - est_c) <= b_c, f"table {j}: est_c {got[3]}, want {est_c} +- {b_c}"
            ck.ratio("guard", max(abs(float(got[1]) - est) / b_est, abs(float(got[3]) - est_c) / b_c))
        ck.free(f"scratch{j}", 16 * c["tables"][j]["W"])
        if c["singles"]:
            ck.exact(f"state_single{j}", got)
            ck.free(f"scratch_single{j}", 16 * c["tables"][j]["W"])
    ck.finish()


def _records_reference(perm, nbr, bin_, coef, sh, d_sh):
    E = len(perm)
    rec = np.zeros((E, 16), np.int32)
    rec[:, 0] = nbr[perm]
    if bin_ is not None:
        rec[:, 1] = bin_[perm]
        rec[:, 2:6] = coef.reshape(-1, 4)[perm].view(np.int32)
    rec[:, 6:6 + d_sh] = sh.reshape(-1, d_sh)[perm].view(np.int32)
    rec[:, 15] = perm
    return rec


def run_records(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    ar = Arena(zlib.crc32(c["id"].encode()))
    E, d_sh = c["E"], c["d_sh"]
    n_all = E + 5      # (the walk visits E of n_all edges)
    perm = ar.rng.permutation(n_all)[:E].astype(np.int32)
    nbr = ar.rng.integers(0, 1000, n_all).astype(np.int32)
    bin_ = ar.rng.integers(1, 500, n_all).astype(np.int32)
    ar.alloc("perm", E, perm).alloc("nbr", n_all, nbr).alloc("bin", n_all, bin_).alloc("coef", 4 * n_all).alloc("sh", n_all * d_sh)
    ar.alloc("rec", 16 * E, np.int32(SENT), align=16)
    ar.upload(dev)
    wb = c["with_bin"]
    rc = lib.e3k_edge_records(ar.p("perm"), ar.p("nbr"), ar.p("bin") if wb else None, ar.p("coef") if wb else None, ar.p("sh"), d_sh, E,
                              ar.p("rec"), st)
    assert rc == E3K_OK
    ck = Check(ar, c)
    if E:
        ck.exact("rec", _records_reference(perm, nbr, bin_ if wb else None, ar.host("coef"), ar.host("sh"), d_sh))
    ck.finish()


def run_refuse(dev, c, L):
    """A small valid problem of every entry point, one argument replaced: the return code, and the arena bit-identical."""
    lib, st = L.load(), L.stream_ptr()
    ar = Arena(zlib.crc32(c["id"].encode()))
    E, K, W, nk = 10, 8, 8, 2
    rows = nk * (K + 1)
    r = ar.rng.uniform(0.0, 2.0, E).astype(np.float32)
    i_ref, c_ref, _, _ = bins_reference(r, 4.0, K)
    cnt = np.bincount(i_ref, minlength=rows)
    ar.alloc("r", E, r).alloc("key", 2 * E, np.zeros(E, np.int64).view(np.int32)).alloc("bin", E, i_ref.astype(np.int32))
    ar.alloc("coef", 4 * E, c_ref.astype(np.float32)).alloc("ptr", rows + 1, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
    ar.alloc("seg", rows + 1, np.concatenate([[0], np.cumsum(-(-cnt // 64))]).astype(np.int32))
    ar.alloc("perm", E, np.argsort(i_ref, kind="stable").astype(np.int32)).alloc("ws", E + rows).alloc("flag", 1, np.int32(0))
    ar.alloc("T", rows * W).alloc("T2", rows * W).alloc("w", E * W).alloc("w2", E * W).alloc("gw", E * W).alloc("scale", E)
    ar.alloc("wsb", (E // 64 + rows + 2) * 4 * W).alloc("gT", rows * W).alloc("P", rows * 3 * W).alloc("state", 4).alloc("scratch", 16 * W)
    ar.alloc("nbr", E, np.arange(E, dtype=np.int32)).alloc("sh", 9 * E).alloc("rec", 16 * E + 16, align=16)
    ar.upload(dev)
    a = dict(E=E, K=K, W=W, h_inv=4.0, n_keys=nk, n=1, floor_rel=1e-3, col_weight=0.25, d_sh=9, rec_shift=0,
             **{k: k for k in ar.blocks})
    a.update(c["over"])
    p = lambda k: ar.p(a[k])
    fn = c["fn"]
    if fn == "rtable_bins":
        rc = lib.e3k_rtable_bins(p("r"), a["E"], a["h_inv"], a["K"], p("bin"), p("coef"), p("ptr"), p("seg"), p("perm"), p("ws"), st)
    elif fn == "rtable_bins_keyed":
        rc = lib.e3k_rtable_bins_keyed(p("r"), p("key"), a["n_keys"], a["E"], a["h_inv"], a["K"], p("bin"), p("coef"), p("ptr"), p("seg"),
                                       p("perm"), p("ws"), p("flag"), st)
    elif fn == "rtable_interp_fwd":
        rc = lib.e3k_rtable_interp_fwd(p("T"), p("perm"), p("bin"), p("coef"), a["E"], a["K"], a["W"], p("w"), st)
    elif fn == "rtable_interp_fwd2":
        rc = lib.e3k_rtable_interp_fwd2(p("T"), p("T2"), p("perm"), p("bin"), p("coef"), a["E"], a["K"], a["W"], p("w"), p("w2"), st)
    elif fn == "rtable_interp_bwd":
        rc = lib.e3k_rtable_interp_bwd(p("gw"), p("coef"), p("scale"), p("ptr"), p("seg"), p("perm"), a["E"], a["K"], a["W"], p("wsb"),
                                       p("gT"), 0, st)
    elif fn == "rtable_pack":
        rc = lib.e3k_rtable_pack(p("T"), a["K"], a["W"], p("P"), st)
    elif fn == "rtable_interp_packed":
        rc = lib.e3k_rtable_interp_packed(p("P"), p("perm"), p("bin"), p("coef"), a["E"], a["K"], a["W"], p("w"), st)
    elif fn == "rtable_pack_multi":
        m = 17
        rc = lib.e3k_rtable_pack_multi((C.c_void_p * m)(*[p("T")] * m), a["K"], (C.c_int32 * m)(*[a["W"]] * m), (C.c_void_p * m)(*[p("P")] * m),
                                       a["n"], st)
    elif fn == "rtable_guard":
        m = 17
        rc = lib.e3k_rtable_guard((C.c_void_p * m)(*[p("T")] * m), (C.c_void_p * m)(*[p("state")] * m), (C.c_void_p * m)(*[p("scratch")] * m),
                                  (C.c_int32 * m)(*[a["W"]] * m), a["n"], K + 1, a["floor_rel"], a["col_weight"], 1, st)
    else:
        assert fn == "edge_records"
        rec = ar.p("rec") + a["rec_shift"]
        rc = lib.e3k_edge_records(p("perm"), p("nbr"), p("bin"), p("coef"), p("sh"), a["d_sh"], a["E"], rec, st)
    assert rc == c["rc"], f"return code {rc}"
    Check(ar, c).finish()


RUNNERS = dict(chain=run_chain, pack=run_pack, guard=run_guard, records=run_records, refuse=run_refuse)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_rtable_case_against_float64(dev, c):
    from e3_layers_amd.backend import lib as L

    RUNNERS[c["kind"]](dev, c, L)
