"""The five kernels of csrc/e3k_md.hip -- md_drift_kernel, md_kick_kernel, fire_step_kernel, md_drift_shake_kernel,
md_kick_rattle_kernel -- through their six C entry points, every output word against float64, element by element.

``CASES`` is a plain table.  A case lays all its operands out in ONE arena (tests/test_gpu_rtable_matrix.py: slack round every block,
random words in between), calls the C ABI through backend/lib.py -- never run/md.py, never ``BondConstraints``: the constraint tables
are written by hand here, so that malformed ones can be expressed -- and ends with ``Check``: every word a call may write is claimed
by one ``exact`` or ``close`` comparison, every other word of the arena must keep its bits.  tests/test_md_inventory.py holds the
table to the kernels the library ships and the functions include/e3k.h declares, shows on the CPU that float32 models of the kernels
stay inside the bounds below (both ways the compiler may contract), that the decisions of the inputs are clear of their thresholds,
and that the bounds are sharp (planted mutants).  Everything below but the runners works without a GPU.

References and bounds.  One statement of every kernel (``drift_model``, ``ou_kick``, ``fire_graph``, ``shake_star``,
``rattle_star``), written against an arithmetic ``B``: ``BEV`` replays it in float64 on the fp32 numbers the kernel receives
(scalars rounded to fp32 first) with the running error analysis ``EV`` / ``fma`` / ``dot_ev`` / ``sum_ev`` of
tests/test_gpu_node_matrix.py; ``B32`` replays it in numpy float32 (the inventory's models).  The bound on an element is what ``EV``
returns for that element; there is no free tolerance.
  * the library is built with -ffp-contract=fast: a product that meets a sum may or may not fuse.  ``B.muladd`` is such a place: BEV
    charges the separate form (which covers the fused one), B32 takes either form by its ``contract`` flag.  ``rounded_product`` and
    a product that is divided before it is added never fuse; ``fmaf`` is ``B.fma``.
  * division and ``sqrtf`` are correctly rounded (no fast-math flag).
  * sums over a graph (kinetic energy, FIRE's P, |f|^2, |v|^2, |dr|^2): ``sum_ev`` / ``dot_ev`` -- any order, gamma_n; the kernel's
    order (lane l takes l, l + 64, ..., a butterfly) is fixed but no part of the contract.  B32 takes the kernel's order.
  * noise: xi is ``data/compute_edge.normal_draw(..., float64)`` with the absolute bound ``XI_BOUND`` of
    tests/test_gpu_md_integrator_kernels.py, which the amplitude s / sqrt(m_i) then scales like any other error.
  * clamps: the reference reads the raw tables and applies the header's clamps itself.

Branches.  FIRE's decisions are planted clear of their thresholds (|P| >= 1e-3 |f| |v| or exactly 0; |dr| 1 % off maxstep; fmax a
factor 2 off ftol; dt f_inc outside its own bound of dt_max) and asserted on the float64 side.  A SHAKE / RATTLE sweep's decisions
(|diff| <= 2 tol d0^2, |r.v_rel| <= tol d0 (|v_c| + |v_s|), r.r_old > 0, |r|^2 > 0) are DECIDED when the float64 quantity clears its
threshold by more than the two EV bounds; at an undecided one either branch is a correct fp32 execution, the reference forks and
carries both continuations (``continuations``).  A star passes if ALL its outputs lie within the bounds of one and the same
continuation; the counter must lie within the range the accepted continuations give.  A star with more than 3 undecided decisions on
one path is left out of the elementwise comparison and held to the stopping rule alone (the bounds of
tests/md_constraint_stubs.assert_constraints_hold); at most 5 % of a case's stars may be, none in a planted-failure case
(tests/test_md_inventory.py asserts both on the CPU).  |r|^2 > 0 is decided false where every component of r is below 2^-76 in
magnitude: each square is below 2^-152 and rounds to zero in fp32, denormals or not.

Findings of these cases.
  * fire_ftol0_empty: with ftol = 0 (accepted) fire_step_kernel did not freeze an empty graph -- fmax = 0 is not below 0 -- and its
    dt, alpha, n_pos went on adapting; the header says "An empty graph is frozen with fmax = 0".  Fixed in the kernel and in the
    torch path of run/md.py (tests/test_md_integrators_host.py holds the latter).
  * rattle_at_centre: a satellite stored AT its centre's position has r = 0, hence r.v_rel = 0, and meets RATTLE's stopping rule as
    the header states it: it is no failure and the counter does not move (star 0 of the case).  The kernel's |r|^2 > 0 guard is
    reached only where |r|^2 underflows while r.v_rel does not: star 1 of the case (|r| = 1e-25, d0 = 0) counts exactly one.

Worst error / bound per family on an MI355X: see MEASURED (a record, not a threshold; printed by test_zz_worst_ratio_per_family).
"""
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_node_matrix import EV, dot_ev, fma, sum_ev
from tests.test_gpu_rtable_matrix import Arena, Check as _Check
from tests.util import record_measured

pytestmark = pytest.mark.gpu

# worst error / bound per family as printed by a full run on an MI355X
MEASURED = {
    # single rounding chains: the float32 models of tests/test_md_inventory.py measure the same on the CPU
    "drift_x": 0.881, "drift_v": 0.912, "kick_v": 0.704, "fire_x": 0.970, "fire_v": 0.441, "fire_state": 0.639, "fire_frec": 0.639,
    "shake_x": 0.964, "shake_v": 0.943, "rattle_v": 0.808,
    # order-independent gamma_n over a graph's atoms: far from attained
    "kick_kinetic": 0.066, "rattle_kinetic": 0.135,
}

f32, f64 = np.float32, np.float64
E3K_OK, E3K_ERR_INVALID = 0, -1
STAR_MAX = 5
U24 = 2.0 ** -24
SEED = (977 << 32) + 20241017      # both seed words in use
FIRE = dict(ftol=1e-3, dt_max=0.5, maxstep=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)
K_DRIFT, K_KICK, K_FIRE, K_SHAKE, K_RATTLE = ("md_drift_kernel", "md_kick_kernel", "fire_step_kernel", "md_drift_shake_kernel",
                                              "md_kick_rattle_kernel")


def _xi_bound():
    from tests.test_gpu_md_integrator_kernels import XI_BOUND

    return XI_BOUND


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64))


def _clip(v, lo, hi):
    return int(min(max(int(v), lo), hi))


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
def drift(id_, why, n, dt=0.37):
    return dict(id=id_, kind="drift", why=why, n=n, dt=dt, kernels={K_DRIFT}, funcs={"e3k_md_drift"})


def kick(id_, why, sizes, c=1.0, s=0.0, fnull=False, kin=True, pot=True, word0=0, draw=41, plain=False, ptr=None):
    funcs = {"e3k_md_kick_langevin"} | ({"e3k_md_kick"} if plain else set())
    return dict(id=id_, kind="kick", why=why, sizes=list(sizes), c=c, s=s, fnull=fnull, kin=kin, pot=pot, word0=word0, draw=draw,
                plain=plain, ptr=ptr, dt=0.37, kernels={K_KICK}, funcs=funcs)


def fire(id_, why, sizes, plants, records=True, ftol=FIRE["ftol"], null_rows=False):
    return dict(id=id_, kind="fire", why=why, sizes=list(sizes), plants=list(plants), records=records, ftol=ftol, null_rows=null_rows,
                kernels={K_FIRE}, funcs={"e3k_fire_step"})


def shake(id_, why, graphs, masses="heavy", fnull=False, counter0=0, max_iter=32, plant=None, malform=None, drift_too=False,
          twice=False, spare=False, salt=0):
    return dict(id=id_, kind="shake", why=why, salt=salt, graphs=graphs, masses=masses, fnull=fnull, counter0=counter0, max_iter=max_iter,
                plant=plant, malform=malform, drift_too=drift_too, twice=twice, spare=spare, dt=0.05, tol=1e-5, kernels={K_SHAKE},
                funcs={"e3k_md_drift_shake"} | ({"e3k_md_drift"} if drift_too else set()))


def rattle(id_, why, graphs, masses="heavy", c=1.0, s=0.0, fnull=False, kin=True, pot=True, word0=0, draw=41, counter0=0, max_iter=32,
           plant=None, malform=None, kick_too=False, twice=False, tol=1e-5, raw_v=False, salt=0):
    return dict(id=id_, kind="rattle", raw_v=raw_v, salt=salt, why=why, graphs=graphs, masses=masses, c=c, s=s, fnull=fnull, kin=kin,
                pot=pot, word0=word0,
                draw=draw, counter0=counter0, max_iter=max_iter, plant=plant, malform=malform, kick_too=kick_too, twice=twice,
                spare=False, dt=0.05, tol=tol, kernels={K_RATTLE},
                funcs={"e3k_md_kick_rattle"} | ({"e3k_md_kick_langevin"} if kick_too else set()))


def refuse(id_, fn, why, **over):
    return dict(id="refuse_" + id_, kind="refuse", why=why, fn=fn, over=over, rc=E3K_ERR_INVALID, kernels=set(), funcs={FN[fn]})


def noop(id_, fn, why, **over):
    return dict(id="noop_" + id_, kind="refuse", why=why, fn=fn, over=over, rc=E3K_OK, kernels=set(), funcs={FN[fn]})


FN = dict(drift="e3k_md_drift", kick="e3k_md_kick", langevin="e3k_md_kick_langevin", fire="e3k_fire_step", shake="e3k_md_drift_shake",
          rattle="e3k_md_kick_rattle")
NAN = float("nan")
MIX = (4,) * 3 + (3,) * 4 + (2,) * 5 + (1,) * 6          # 18 stars, 59 atoms
G9 = [((1, 2, 3, 4), 3), ((), 0), ((2,), 1), ((), 70), ((1,) * 70, 0), ((4, 4), 0), ((), 1), ((3, 1), 2), ((), 0)]

CASES = [
    # ---- drift: 3n components, one per thread, 256 to a workgroup
    drift("drift_n1", "one atom: three threads", 1),
    drift("drift_n85", "3n = 255: one short of a workgroup", 85),
    drift("drift_n86", "3n = 258: across the 256-thread seam (an atom's components in two workgroups)", 86, dt=-0.37),
    drift("drift_n171", "3n = 513: two workgroups and one thread", 171),
    # ---- kick: one wave per graph, four graphs per workgroup
    kick("kick_G1", "one graph of 129 atoms (a lane takes three); e3k_md_kick beside e3k_md_kick_langevin(1, 0): the same bits",
         [129], plain=True),
    kick("kick_G4_friction", "four graphs fill a workgroup, the empty graph first; friction alone (c, 0)", [0, 1, 63, 64], c=0.8125,
         pot=False),
    kick("kick_G5_noise_only", "five graphs: a second workgroup with one wave; (0, s), f NULL (a Maxwell-Boltzmann draw), word0 = 4",
         [65, 1, 200, 64, 0], c=0.0, s=0.7, fnull=True, word0=4, draw=7, kin=False),
    kick("kick_G9_langevin", "nine graphs, the empty graph last; (c, s) with forces, both records", [200, 65, 1, 64, 63, 129, 1, 64, 0],
         c=0.9, s=0.45),
    kick("kick_G9_no_records", "kinetic and potential NULL: v alone is written", [64, 0, 65, 1, 1, 63, 129, 5, 2], c=0.9, s=0.45,
         kin=False, pot=False, draw=(1 << 32) - 3),
    kick("kick_bad_ptr", "node_ptr = (-2, 70, n + 2, 9): the walk is that of the clamped pointers -- [0, 70), [70, n), nothing -- and "
         "no row outside [0, n) changes; the last graph's energy is exactly 0", [70, 65, 0], c=0.9, s=0.45, ptr=(-2, 70, "n+2", 9)),
    # ---- FIRE
    fire("fire_G1", "one graph of 129 atoms, downhill and old: dt and alpha adapt, the step is clipped", [129], ["downhill_old"]),
    fire("fire_G5", "every branch in one call on 1, 64, 65, 129 atoms and an empty graph", [1, 64, 0, 65, 129],
         ["uphill", "at_rest_capped", "empty", "frozen", "downhill_young"]),
    fire("fire_G9", "nine graphs: every branch on another size", [65, 129, 1, 0, 64, 64, 129, 1, 65],
         ["downhill_young", "uphill", "downhill_old", "empty", "frozen", "downhill_old", "at_rest_capped", "frozen", "uphill"]),
    fire("fire_no_records", "energy_record, fmax_record and energy NULL", [64, 1, 0, 65, 129],
         ["downhill_old", "downhill_young", "empty", "at_rest_capped", "uphill"], records=False),
    fire("fire_ftol0_zero_forces", "all-zero forces with ftol = 0: not frozen (0 < 0 is false), P = 0 is downhill, mix = 0 (no 0 / 0), "
         "v <- (1 - alpha) v and x moves; nothing is NaN", [65, 1, 64], ["zero_forces", "zero_forces", "downhill_old"], ftol=0.0),
    fire("fire_ftol0_empty", "empty graphs with ftol = 0 and n_pos > n_min: frozen all the same -- (dt, alpha, n_pos) stay, fmax = 0 "
         "(failed before the kernel asked end <= beg)", [0, 65, 0], ["empty", "downhill_old", "empty"], ftol=0.0),
    fire("fire_n0", "n = 0 with G = 3: every graph is empty; x, v and f NULL", [0, 0, 0], ["empty"] * 3, null_rows=True),
    # ---- SHAKE: a thread per star, then a thread per free atom
    shake("shake_one_star", "S + F = 1: one star of two satellites, one thread", [((2,), 0)]),
    shake("shake_255", "S + F = 255: stars of 1, 2, 3 and 4 satellites (atoms shuffled) and 237 free atoms; the free atoms == "
          "e3k_md_drift on the same rows, bit for bit; a second call gives the same bits", [(MIX, 100), ((), 137)], drift_too=True,
          twice=True),
    shake("shake_256_free_only", "S = 0, F = 256: with no star e3k_md_drift_shake == e3k_md_drift, bit for bit", [((), 200), ((), 56)],
          drift_too=True),
    shake("shake_257_stars_only", "F = 0, S = 257: the last star alone in the second workgroup", [((1,) * 120 + MIX, 0), ((1,) * 119, 0)]),
    shake("shake_project", "f NULL, the projection: lengths enforced at the present positions (every bond 1 % too long); v and the "
          "free atoms untouched bit for bit", [(MIX, 9)], fnull=True, plant="stretched"),
    shake("shake_light_pairs", "comparable masses 0.5 .. 4, pairs only: the mass split of the correction", [((1,) * 40, 3)],
          masses="light"),
    shake("shake_max_iter1", "max_iter = 1, 260 pairs, five of them (threads 3, 100, 255, 256, 259: both workgroups) need a second "
          "correction; the counter starts at 7 and ends at exactly 12; each star is written as it stands",
          [((1,) * 260, 2)], max_iter=1, counter0=7, plant=("second_correction", (3, 100, 255, 256, 259))),
    shake("shake_turned", "one satellite whose dt v carries it through the centre (r.r_old < 0): exactly one failure, the star is "
          "written uncorrected", [(MIX, 4)], plant=("turned", 7), counter0=7, salt=1),
    shake("shake_bad_atoms", "a star_atom entry of -2 (a satellite: row 0) and one of n + 1 (a centre: row n - 1): clamped; rows 0 and "
          "n - 1 belong to no other thread", [(MIX, 6)], malform="bad_atoms", spare=True),
    shake("shake_bad_free", "a free_atom entry of -1 (row 0) and one of n + 1 (row n - 1): clamped", [(MIX, 6)], malform="bad_free",
          spare=True),
    shake("shake_row7", "a row of 7 slots: the first five are the star, the last two name atoms that must not move", [(MIX, 6)],
          malform="row7"),
    shake("shake_ptr_decreasing", "star_ptr[S] < star_ptr[S - 1]: an empty row, nothing written", [(MIX, 6)], malform="ptr_decreasing", salt=1),
    shake("shake_ptr_past_slots", "the last star's row runs two past n_slots: cut at n_slots (centre and one satellite of three)",
          [(MIX[::-1] + (3,), 6)], malform="ptr_past_slots"),
    # ---- RATTLE: a wave per graph; a lane takes its stars, then its free atoms
    rattle("rattle_G1", "one graph of 70 stars (lanes 0..5 take two) and 70 free atoms (the prefetched first, then the loop); the plain "
           "kick (1, 0); a second call gives the same bits", [(MIX * 3 + (1,) * 16, 70)], twice=True),
    rattle("rattle_G5_friction", "stars only, free atoms only, an empty graph, 70 stars; friction alone (c, 0), potential NULL",
           [((1,) * 64 + (2, 3, 4, 1, 2, 3), 3), ((), 70), (MIX, 0), ((), 5), ((), 0)], c=0.8125, pot=False),
    rattle("rattle_G9_noise", "nine graphs; (c, s) with forces: the draw follows the atom's ROW, not its place in the tables", G9,
           c=0.9, s=0.004),
    rattle("rattle_G9_thermalize", "(0, s) with f NULL, word0 = 4, kinetic NULL: a projected Maxwell-Boltzmann draw.  tol = 1e-3 here: at "
           "c = 0 every quantity of the sweep scales with s -- the threshold and XI_BOUND's share of the bound alike, 4.5e-6 against "
           "1e-5 -- so that at tol = 1e-5 no star can be decided at any s", G9, c=0.0, s=0.7, fnull=True, word0=4, draw=7, kin=False,
           tol=1e-3),
    rattle("rattle_light_pairs", "comparable masses, pairs only", [((1,) * 30, 3)], masses="light"),
    rattle("rattle_raw_pairs", "six pairs with velocities as drawn, far off the constraints (a pair is done after one correction all "
           "the same): the projection takes a fifth of the kinetic energy away -- in the other cases it takes next to nothing, and an "
           "energy summed before the projection stayed inside gamma_n of a graph of 300 atoms", [((1,) * 6, 0)], raw_v=True),
    rattle("rattle_no_star", "no star: e3k_md_kick_rattle == e3k_md_kick_langevin, velocities and kinetic energies, bit for bit",
           [((), 70), ((), 0), ((), 1), ((), 129), ((), 64)], c=0.9, s=0.45, kick_too=True),
    rattle("rattle_max_iter1", "max_iter = 1: a pair is done after one correction, a star of several satellites is not -- the counter "
           "starts at 7 and rises by exactly the 11 (of 12) such stars whose first pass leaves a residual",
           [((1,) * 20 + MIX[:12], 2), ((1,) * 5, 0)], max_iter=1, counter0=7),
    rattle("rattle_at_centre", "star 0: a satellite stored at its centre's position (r = 0) meets the stopping rule, no failure; star "
           "1: |r| = 1e-25 with d0 = 0, |r|^2 underflows: exactly one failure", [((2, 1) + MIX, 3)], plant=("at_centre",), counter0=7),
    rattle("rattle_bad_graph_ptrs", "graph_star_ptr = (-3, .., S + 2, 5) and graph_free_ptr = (-1, .., F + 3, 2): clamped; the "
           "decreasing pair is an empty graph with energy 0", [(MIX, 5), ((1, 2), 70)], malform="bad_graph_ptrs"),
    rattle("rattle_garbage_node_ptr", "node_ptr filled with garbage: checked for NULL and otherwise unused", [(MIX, 5), ((1, 2), 3)],
           malform="garbage_node_ptr", c=0.9, s=0.004),
    # ---- refusals: nothing is launched, the arena stays as it was
    refuse("drift_n_negative", "drift", "n < 0", n=-1),
    *[refuse(f"drift_null_{k}", "drift", f"{k} NULL", **{k: None}) for k in ("x", "v", "f", "mass")],
    refuse("kick_n_negative", "kick", "n < 0", n=-1),
    refuse("kick_G_negative", "kick", "G < 0", G=-1),
    *[refuse(f"kick_null_{k}", "kick", f"{k} NULL", **{k: None}) for k in ("v", "f", "mass", "node_ptr")],
    refuse("kick_potential_without_energy", "kick", "potential given, energy NULL", energy=None),
    refuse("langevin_n_negative", "langevin", "n < 0", n=-1),
    refuse("langevin_G_negative", "langevin", "G < 0", G=-1),
    refuse("langevin_c_negative", "langevin", "c < 0", c=-0.25),
    refuse("langevin_c_above_1", "langevin", "c > 1", c=1.5),
    refuse("langevin_c_nan", "langevin", "c NaN", c=NAN),
    refuse("langevin_s_negative", "langevin", "s < 0", s=-0.5),
    refuse("langevin_s_nan", "langevin", "s NaN", s=NAN),
    *[refuse(f"langevin_null_{k}", "langevin", f"{k} NULL", **{k: None}) for k in ("v", "mass", "node_ptr")],
    refuse("langevin_potential_without_energy", "langevin", "potential given, energy NULL", energy=None),
    refuse("fire_n_negative", "fire", "n < 0", n=-1),
    refuse("fire_G_negative", "fire", "G < 0", G=-1),
    refuse("fire_ftol_negative", "fire", "ftol < 0", ftol=-1e-3),
    refuse("fire_ftol_nan", "fire", "ftol NaN", ftol=NAN),
    refuse("fire_dt_max_zero", "fire", "dt_max <= 0", dt_max=0.0),
    refuse("fire_dt_max_nan", "fire", "dt_max NaN", dt_max=NAN),
    refuse("fire_maxstep_zero", "fire", "maxstep <= 0", maxstep=0.0),
    refuse("fire_maxstep_negative", "fire", "maxstep < 0", maxstep=-0.2),
    refuse("fire_n_min_negative", "fire", "n_min < 0", n_min=-1),
    *[refuse(f"fire_null_{k}", "fire", f"{k} NULL", **{k: None}) for k in ("node_ptr", "state", "x", "v", "f")],
    refuse("fire_record_without_energy", "fire", "energy_record given, energy NULL", energy=None),
    refuse("shake_n_negative", "shake", "n < 0", n=-1),
    refuse("shake_S_negative", "shake", "n_stars < 0", S=-1),
    refuse("shake_slots_negative", "shake", "n_slots < 0", n_slots=-1),
    refuse("shake_F_negative", "shake", "n_free < 0", F=-1),
    refuse("shake_too_many_threads", "shake", "n_stars + n_free = 2^31", S=2 ** 31 - 5),
    refuse("shake_tol_zero", "shake", "tol <= 0", tol=0.0),
    refuse("shake_tol_nan", "shake", "tol NaN", tol=NAN),
    refuse("shake_max_iter_zero", "shake", "max_iter < 1", max_iter=0),
    refuse("shake_null_counter", "shake", "counter NULL", counter=None),
    *[refuse(f"shake_null_{k}", "shake", f"stars with {k} NULL", **{k: None}) for k in ("star_ptr", "star_atom", "star_len")],
    refuse("shake_null_free_atom", "shake", "free atoms with free_atom NULL", free_atom=None),
    refuse("shake_tables_n0", "shake", "tables with n = 0", n=0),
    refuse("shake_f_with_dt0", "shake", "f given with dt = 0 (the velocity correction divides by dt)", dt=0.0),
    *[refuse(f"shake_null_{k}", "shake", f"{k} NULL", **{k: None}) for k in ("x", "v", "mass")],
    refuse("rattle_G_negative", "rattle", "G < 0", G=-1),
    refuse("rattle_n_negative", "rattle", "n < 0", n=-1),
    refuse("rattle_c_negative", "rattle", "c < 0", c=-1e-3),
    refuse("rattle_c_above_1", "rattle", "c > 1", c=1.0000001),
    refuse("rattle_c_nan", "rattle", "c NaN", c=NAN),
    refuse("rattle_s_negative", "rattle", "s < 0", s=-1e-3),
    refuse("rattle_s_nan", "rattle", "s NaN", s=NAN),
    refuse("rattle_tol_negative", "rattle", "tol <= 0", tol=-1e-5),
    refuse("rattle_tol_nan", "rattle", "tol NaN", tol=NAN),
    refuse("rattle_max_iter_zero", "rattle", "max_iter < 1", max_iter=0),
    refuse("rattle_null_counter", "rattle", "counter NULL", counter=None),
    *[refuse(f"rattle_null_{k}", "rattle", f"stars with {k} NULL", **{k: None}) for k in ("star_ptr", "star_atom", "star_len")],
    refuse("rattle_null_free_atom", "rattle", "free atoms with free_atom NULL", free_atom=None),
    refuse("rattle_tables_n0", "rattle", "tables with n = 0", n=0),
    *[refuse(f"rattle_null_{k}", "rattle", f"{k} NULL", **{k: None}) for k in ("v", "mass", "node_ptr", "graph_star_ptr",
                                                                                "graph_free_ptr")],
    refuse("rattle_null_x_with_stars", "rattle", "x NULL with stars", x=None),
    refuse("rattle_potential_without_energy", "rattle", "potential given, energy NULL", energy=None),
    # ---- no-op returns: E3K_OK, nothing launched, also with NULL pointers
    noop("drift_n0", "drift", "n = 0, every pointer NULL", n=0, x=None, v=None, f=None, mass=None),
    noop("kick_n0", "kick", "n = 0", n=0, v=None, f=None, mass=None),
    noop("kick_G0", "kick", "G = 0", G=0, node_ptr=None),
    noop("langevin_n0", "langevin", "n = 0", n=0, v=None, mass=None),
    noop("langevin_G0", "langevin", "G = 0", G=0, node_ptr=None),
    noop("fire_G0", "fire", "G = 0", G=0, node_ptr=None, state=None),
    noop("shake_nothing_to_do", "shake", "S + F = 0, every pointer but the counter NULL", S=0, F=0, x=None, v=None, mass=None,
         star_ptr=None, free_atom=None),
    noop("rattle_G0", "rattle", "G = 0", G=0, node_ptr=None, graph_star_ptr=None, graph_free_ptr=None),
    noop("rattle_n0", "rattle", "n = 0 with empty tables", n=0, S=0, F=0, v=None, mass=None, x=None),
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


# ---------------------------------------------------------------------------------------------------------------------------------
# the two arithmetics
def fma32(a, b, c):
    """fmaf: one rounding (the float64 product of two float32 is exact; the sum's double rounding is below 2^-52)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


class B32:
    """numpy float32, operation for operation; ``contract``: every product the compiler MAY fuse into a sum is fused"""
    ev = False

    def __init__(self, contract):
        self.contract = contract

    def lit(self, x):
        return np.asarray(x, f32)

    def noise(self, xi64):
        return np.asarray(xi64, f64).astype(f32)

    def muladd(self, a, b, c):
        return fma32(a, b, c) if self.contract else a * b + c

    def fma(self, a, b, c):
        return fma32(a, b, c)

    def sqrt(self, a):
        return np.sqrt(a)

    def abs(self, a):
        return np.abs(a)

    def ix(self, a, i):
        return a[..., i]

    def ix_row(self, a, i):
        return a[i]

    def val(self, a):
        return np.asarray(a, f64)

    def pair(self, a, shape=None):
        a = np.asarray(a)
        assert a.dtype == f32, a.dtype
        v = a.astype(f64) if shape is None else np.broadcast_to(a.astype(f64), shape)
        return np.array(v), np.zeros(v.shape)

    def wave(self, lanes, hm, q, explicit):
        """sum of hm q (q None: of hm) in the kernel's order: ``lanes[l]`` lists the terms of lane l, the 64 sums meet in wave_sum"""
        acc = np.zeros(64, f32)
        for l, items in enumerate(lanes):
            for i in items:
                if q is None:
                    acc[l] = acc[l] + hm[i]
                elif explicit or self.contract:
                    acc[l] = fma32(hm[i], q[i], acc[l])
                else:
                    acc[l] = hm[i] * q[i] + acc[l]
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[np.arange(64) ^ off]
        assert acc.dtype == f32
        return acc[0]

    def vmax(self, a):
        return a.max()


class BEV:
    """float64 with a bound on |fp32 result - value| (EV of tests/test_gpu_node_matrix.py)"""
    ev = True

    def lit(self, x):
        return EV(np.asarray(x, f32).astype(f64))

    def noise(self, xi64):
        return EV(np.asarray(xi64, f64), _xi_bound())

    def muladd(self, a, b, c):
        return EV.of(a) * b + c

    def fma(self, a, b, c):
        return fma(a, b, c)

    def sqrt(self, a):
        return a.sqrt()

    def abs(self, a):
        return a.abs()

    def ix(self, a, i):
        return EV(a.v[..., i], a.e[..., i])

    def ix_row(self, a, i):
        return EV(a.v[i], a.e[i])

    def val(self, a):
        return a.v

    def pair(self, a, shape=None):
        return a.pair(shape)

    def wave(self, lanes, hm, q, explicit):
        t = hm if q is None else hm * q
        return sum_ev(t, 0)

    def vmax(self, a):
        return EV(a.v.max(), a.e.max())


def dot3(B, a, b):
    """(a0 b0 + a1 b1) + a2 b2"""
    return B.muladd(B.ix(a, 2), B.ix(b, 2), B.muladd(B.ix(a, 0), B.ix(b, 0), B.ix(a, 1) * B.ix(b, 1)))


def _lanes(count):
    return [list(range(l, count, 64)) for l in range(64)]


def graph_dot(B, a, b):
    """sum over a graph's atoms of a_i . b_i: any order for the reference (dot_ev over the 3 k products), the kernel's for B32"""
    if B.ev:
        return dot_ev(EV(a.v.reshape(-1), a.e.reshape(-1)), EV(b.v.reshape(-1), b.e.reshape(-1)), 0)
    return B.wave(_lanes(a.shape[0]), dot3(B, a, b), None, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic, stated once
def drift_model(B, x, v, f, m, dt, mutant=None):
    """half_kick_drift on rows [k, 3] with masses [k, 1]: v += dt/2 f / m, x += dt v"""
    vn = v + (B.lit(0.5) * dt) * f / m
    return B.muladd(dt, v if mutant == "drift_old_v" else vn, x), vn


def ou_kick(B, v, f, m, dt, c, s, xi, mutant=None):
    """v <- c v + (s / sqrt(m)) xi (two rounded products, a plain add; s == 0: nothing drawn), then v += dt/2 f / m (f None: not)"""
    vn = c * v
    if xi is not None:
        a = s / (m if mutant == "noise_over_m" else B.sqrt(m))
        vn = vn + a * xi
    if f is not None:
        vn = B.muladd(B.lit(0.5) * dt / m, f, vn)
    return vn


def draws(B, inp, rows, mutant=None):
    """xi [k, 3] of the rows' draw: node = the atom's row, word = word0 + component"""
    from e3_layers_amd.data.compute_edge import normal_draw

    word = inp["word0"] + (torch.zeros(3, dtype=torch.int64) if mutant == "noise_word_without_component" else torch.arange(3))
    xi = normal_draw(SEED, inp["draw"], torch.as_tensor(np.asarray(rows, np.int64))[:, None], word[None, :], torch.float64)
    return B.noise(xi.numpy())


def ke_terms(B, v, m, explicit):
    """(0.5 m, vx^2 + vy^2 + vz^2): md_kick_kernel writes its contractions out, md_kick_rattle_kernel leaves them to the compiler"""
    vx, vy, vz = (B.ix(v, i) for i in range(3))
    q = B.fma(vz, vz, B.fma(vx, vx, vy * vy)) if explicit else dot3(B, v, v)
    return B.lit(0.5) * m, q


def fire_graph(B, x, v, f, state, p, mutant=None):
    """One graph of fire_step_kernel: x, v, f [k, 3]; state (dt, alpha, n_pos: a float, exact); p: the parameters.  Returns x, v
    (None: untouched), (dt, alpha, n_pos, fmax) and the branch's name."""
    k = x.shape[0] if not B.ev else x.v.shape[0]
    dt, alpha, n_pos = state
    if k == 0:
        return None, None, (dt, alpha, n_pos, B.lit(0.0)), "empty"
    fv, ff, vv = graph_dot(B, f, v), graph_dot(B, f, f), graph_dot(B, v, v)
    fmax = B.sqrt(B.vmax(dot3(B, f, f)))
    val = lambda t: float(B.val(t))
    ftol = val(p["ftol"])
    if B.ev:
        assert val(fmax) >= 2 * ftol or val(fmax) <= 0.5 * ftol, "fmax within a factor 2 of ftol"
    if val(fmax) < ftol:
        return None, B.lit(np.zeros((k, 3))), (dt, alpha, n_pos, fmax), "frozen"
    if B.ev:
        fn, vn_ = np.sqrt(val(ff)), np.sqrt(val(vv))
        assert (val(fv) == 0.0 and (vn_ == 0.0 or fn == 0.0)) or abs(val(fv)) >= 1e-3 * fn * vn_, "P near zero"
        assert val(ff) == 0.0 or val(ff) > 1e-12
    uphill = val(fv) < 0.0 or (mutant == "fire_p0_uphill" and val(fv) == 0.0)
    if uphill:
        keep = mix = B.lit(0.0)
        dt, alpha, n_pos = dt * p["f_dec"], p["alpha_start"], 0.0
    else:
        keep = B.lit(1.0) - alpha
        mix = alpha * (B.sqrt(vv) / B.sqrt(ff)) if val(ff) > 0.0 else B.lit(0.0)
        if mutant == "fire_mix_alpha":
            mix = alpha
        if n_pos > p["n_min"]:
            grown = dt * p["f_inc"]
            if B.ev:
                assert abs(val(grown) - val(p["dt_max"])) > float(grown.e), "dt f_inc within its bound of dt_max"
            dt = grown if val(grown) < val(p["dt_max"]) else p["dt_max"]
            alpha = alpha * p["f_alpha"]
        n_pos = n_pos + 1.0
    vn = B.muladd(dt, f, B.muladd(mix, f, keep * v))
    if mutant == "fire_clip_per_atom":
        norm_dr = dt * B.sqrt(dot3(B, vn, vn))
        clip = B.val(norm_dr) > val(p["maxstep"])
        move = np.where(clip, dt * (p["maxstep"] / norm_dr), dt).astype(f32)[:, None]
    else:
        norm_dr = dt * B.sqrt(graph_dot(B, vn, vn))
        if B.ev:
            assert abs(val(norm_dr) / val(p["maxstep"]) - 1.0) >= 0.01, "|dr| within 1 % of maxstep"
        clip = val(norm_dr) > val(p["maxstep"])
        move = dt * (p["maxstep"] / norm_dr) if clip else dt
    name = ("up" if uphill else "down") + ("_clipped" if np.any(clip) else "")
    return B.muladd(move, vn, x), vn, (dt, alpha, n_pos, fmax), name


class NeedChoice(Exception):
    pass


class Decide32:
    """fp32 decides by its own numbers"""

    def outside(self, lhs, thr):
        return not bool(lhs <= thr)

    def positive(self, a, r=None):
        return bool(a > 0)


class DecideEV:
    """float64 decides where the quantity clears its threshold by more than the two bounds; elsewhere the next forced choice"""

    def __init__(self, forced=()):
        self.forced, self.used = tuple(forced), 0

    def _fork(self):
        if self.used < len(self.forced):
            self.used += 1
            return self.forced[self.used - 1]
        raise NeedChoice

    def outside(self, lhs, thr):
        margin, slack = float(lhs.v) - float(thr.v), float(lhs.e) + float(thr.e)
        return margin > 0 if abs(margin) > slack else self._fork()

    def positive(self, a, r=None):
        if float(a.v) - float(a.e) > 0:
            return True
        if float(a.v) + float(a.e) < 0:
            return False
        if r is not None and (np.abs(r.v) + r.e < 2.0 ** -76).all():      # every square is below 2^-152: it rounds to zero
            return False
        return self._fork()


def continuations(run):
    """every execution ``run(DecideEV)`` fp32 may take: None where a path meets more than 3 undecided decisions"""
    out, stack = [], [()]
    while stack:
        forced = stack.pop()
        try:
            out.append(run(DecideEV(forced)))
        except NeedChoice:
            if len(forced) >= 3:
                return None
            stack += [forced + (True,), forced + (False,)]
    return out


def shake_star(B, D, X, V, F, M, d0, dt, tol, max_iter, mutant=None):
    """One star of md_drift_shake_kernel.  X, V, F (None: the projection), M: per atom (centre first) [3] / scalars; d0: per
    satellite.  Returns (x per atom, v per atom or None, failed)."""
    k = len(d0)
    zero = B.lit(np.zeros(3))
    ro = [X[a] - X[0] for a in range(1, k + 1)]
    if F is not None:
        half = B.lit(0.5) * dt
        vh = [V[a] + half * F[a] / M[a] for a in range(k + 1)]
        p = [dt * vh[0]] + [ro[a - 1] + dt * vh[a] for a in range(1, k + 1)]      # (rounded_product, then a plain add)
    else:
        vh, p = None, [zero] + list(ro)
    q = [zero] + list(ro) if mutant == "shake_v_from_old" else list(p)
    inv_m = [B.lit(1.0) / M[a] for a in range(k + 1)]
    two_tol = B.lit(2.0) * tol
    fail = False
    for it in range(max_iter + 1):
        moved = False
        for j in range(k):
            r = p[j + 1] - p[0]
            d02 = d0[j] * d0[j]
            diff = B.muladd(d0[j], d0[j], -dot3(B, r, r))
            if D.outside(B.abs(diff), two_tol * d02):
                moved = True
                along = r if mutant == "shake_present_bond" else ro[j]
                correcting = it < max_iter or mutant == "shake_last_pass_corrects"
                rr = dot3(B, r, along)
                if correcting and D.positive(rr):
                    g = diff / (B.lit(2.0) * rr * (inv_m[0] + inv_m[j + 1]))
                    gs, gc = g * inv_m[j + 1], g * inv_m[0]
                    if mutant == "shake_masses_swapped":
                        gs, gc = gc, gs
                    p[j + 1] = B.muladd(gs, along, p[j + 1])
                    if mutant != "shake_no_centre_share":
                        p[0] = B.muladd(-gc, along, p[0])
                else:
                    fail = True
        if not moved:
            break
    x = [X[0] + p[a] for a in range(k + 1)]
    v = None
    if F is not None:
        inv_dt = B.lit(1.0) / dt
        v = [B.muladd(p[a] - q[a], inv_dt, vh[a]) for a in range(k + 1)]
    return x, v, fail


def rattle_star(B, D, U0, X, M, d0, tol, max_iter, mutant=None):
    """One star of md_kick_rattle_kernel after ou_kick: U0, X, M per atom (centre first).  Returns (v per atom, failed)."""
    k = len(d0)
    u = list(U0)
    r = [X[a] - X[0] for a in range(1, k + 1)]
    r2 = [dot3(B, t, t) for t in r]
    inv_m = [B.lit(1.0) / M[a] for a in range(k + 1)]
    fail = False
    for it in range(max_iter + 1):
        moved = False
        for j in range(k):
            rv = dot3(B, r[j], u[j + 1] - u[0])
            speed = B.sqrt(dot3(B, u[0], u[0])) + B.sqrt(dot3(B, u[j + 1], u[j + 1]))
            if D.outside(B.abs(rv), tol * d0[j] * speed):
                moved = True
                if it < max_iter and D.positive(r2[j], r[j]):
                    gk = rv / (r2[j] * (inv_m[0] + inv_m[j + 1]))
                    gs, gc = gk * inv_m[j + 1], gk * inv_m[0]
                    u[j + 1] = B.muladd(-gs, r[j], u[j + 1])
                    u[0] = B.muladd(gc, r[j], u[0])
                else:
                    fail = True
        if not moved:
            break
    return u, fail


def load_star(tb, t, n, mutant=None):
    """(rows, satellites' lengths) of star t under the header's clamps; None: an empty row"""
    n_slots = int(tb["n_slots"])
    beg = _clip(tb["star_ptr"][t], 0, n_slots)
    end = _clip(tb["star_ptr"][t + 1], beg, n_slots)
    cnt = end - beg if mutant == "star_row_in_full" else min(end - beg, STAR_MAX)
    if cnt == 0:
        return None
    return [_clip(tb["star_atom"][beg + a], 0, n - 1) for a in range(cnt)], [f32(tb["star_len"][beg + a]) for a in range(1, cnt)]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (numpy, no device)
def _rng(c):
    """(``salt``: another draw of the inputs, where the first left more than 5 % of a small case's stars undecided)"""
    return np.random.default_rng((zlib.crc32(c["id"].encode()) ^ 0x3D) + c.get("salt", 0))


def star_system(rng, graphs, masses="heavy", spare=False, spread=8.0):
    """Graphs of stars and free atoms, the atoms of a graph shuffled: x, v, f [n, 3], mass [n] fp32 and the hand-written tables.
    Satellites 0.9 .. 1.5 from their centre; "heavy": centres 12 or 16, satellites 1 (the "hydrogen" masses of
    tests/md_constraint_stubs.py), "light": 0.5 .. 4; free atoms 0.5 .. 12.  The centre's length slot holds -5 (it is not read).
    ``spare``: rows 0 and n - 1 are atoms of no star and no free list (the rows a clamp lands on)."""
    xs, ms = [np.zeros((1, 3))] if spare else [], [np.full(1, 7.0)] if spare else []
    star_ptr, star_atom, free, gsp, gfp, node_ptr = [0], [], [], [0], [0], [0]
    base = 1 if spare else 0
    n_star = 0
    for stars, n_free in graphs:
        ng = sum(k + 1 for k in stars) + n_free
        perm = base + rng.permutation(ng)
        xg, mg, at = np.zeros((ng, 3)), np.zeros(ng), 0
        for k in stars:
            d = rng.standard_normal((k, 3))
            xg[at] = spread * rng.uniform(-1, 1, 3)
            xg[at + 1:at + 1 + k] = xg[at] + rng.uniform(0.9, 1.5, (k, 1)) * d / np.linalg.norm(d, axis=1, keepdims=True)
            if masses == "heavy":
                mg[at], mg[at + 1:at + 1 + k] = (12.0, 16.0)[n_star % 2], 1.0
            else:
                mg[at:at + 1 + k] = rng.uniform(0.5, 4.0, k + 1)
            star_atom += [int(i) for i in perm[at:at + 1 + k]]
            star_ptr.append(len(star_atom))
            at += k + 1
            n_star += 1
        xg[at:] = spread * rng.uniform(-1, 1, (n_free, 3))
        mg[at:] = rng.uniform(0.5, 12.0, n_free)
        free += sorted(int(i) for i in perm[at:])
        order = np.argsort(perm)
        xs.append(xg[order])
        ms.append(mg[order])
        base += ng
        gsp.append(len(star_ptr) - 1)
        gfp.append(len(free))
        node_ptr.append(base)
    if spare:
        xs.append(np.ones((1, 3)))
        ms.append(np.full(1, 3.0))
        node_ptr[-1] = base + 1
    x = np.concatenate(xs).astype(f32) if xs else np.zeros((0, 3), f32)
    mass = np.concatenate(ms).astype(f32) if ms else np.zeros(0, f32)
    n = len(x)
    v = (0.3 * rng.standard_normal((n, 3)) / np.sqrt(mass.astype(f64))[:, None]).astype(f32)
    f = rng.standard_normal((n, 3)).astype(f32)
    star_len = np.full(len(star_atom), -5.0, f32)
    for t in range(len(star_ptr) - 1):
        for a in range(star_ptr[t] + 1, star_ptr[t + 1]):
            star_len[a] = f32(np.linalg.norm(x[star_atom[a]].astype(f64) - x[star_atom[star_ptr[t]]].astype(f64)))
    return dict(x=x, v=v, f=f, mass=mass, n=n, G=len(graphs), star_ptr=_i64(star_ptr), star_atom=_i64(star_atom), star_len=star_len,
                free_atom=_i64(free), S=len(star_ptr) - 1, F=len(free), n_slots=len(star_atom), graph_star_ptr=_i64(gsp),
                graph_free_ptr=_i64(gfp), node_ptr=_i64(node_ptr))


def _star_rows(inp, t):
    a, b = int(inp["star_ptr"][t]), int(inp["star_ptr"][t + 1])
    return [int(i) for i in inp["star_atom"][a:b]]


def inputs_star(c):
    rng = _rng(c)
    inp = star_system(rng, c["graphs"], c["masses"], c["spare"])
    n, S, F = inp["n"], inp["S"], inp["F"]
    inp.update(dt=f32(c["dt"]), tol=f32(c["tol"]), max_iter=c["max_iter"], counter0=c["counter0"], word0=c.get("word0", 0),
               draw=c.get("draw", 0), c=f32(c.get("c", 1.0)), s=f32(c.get("s", 0.0)), energy=rng.standard_normal(inp["G"] + 2).astype(f32),
               planted=c["plant"] is not None and c["plant"] != "stretched" or c["max_iter"] == 1)
    plant, x, v = c["plant"], inp["x"], inp["v"]
    if c["kind"] == "rattle":
        # The velocities RATTLE meets in a step: on the constraints already (SHAKE's velocity correction left them there), then moved
        # off by the kick and the noise alone -- forces of 0.1, s of a few 1e-3: |r.v_rel| starts near 3e-3, three decades above its
        # threshold, and a star of several satellites is done in about 3 passes.  (From unprojected velocities it takes 5 and more,
        # and the EV bound, which doubles with every correction of a satellite -- it cannot see that the projection removes the
        # error along the bond --, passes the threshold itself: the star would be left out.)
        inp["f"] *= f32(0.1)
        for t in range(0 if not c["raw_v"] else S, S):
            rows = _star_rows(inp, t)
            for a in rows[1:]:
                r = x[a].astype(f64) - x[rows[0]].astype(f64)
                v[a] = (v[a].astype(f64) - ((v[a].astype(f64) - v[rows[0]].astype(f64)) @ r) / (r @ r) * r).astype(f32)
    if plant == "stretched":
        for t in range(S):
            rows = _star_rows(inp, t)
            x[rows[1:]] = (x[rows[0]].astype(f64) + 1.01 * (x[rows[1:]].astype(f64) - x[rows[0]].astype(f64))).astype(f32)
    elif plant and plant[0] == "second_correction":
        inp["f"] *= f32(0.01)
        for t in range(S):      # every satellite leaves along its bond: 3e-4 of its length per step, the planted ones 5e-2
            rows = _star_rows(inp, t)
            rel = (0.05 if t in plant[1] else 3e-4) / float(inp["dt"])
            v[rows[1:]] = (v[rows[0]].astype(f64) + rel * (x[rows[1:]].astype(f64) - x[rows[0]].astype(f64))).astype(f32)
    elif plant and plant[0] == "turned":
        rows = _star_rows(inp, plant[1])
        v[rows[1]] = (v[rows[0]].astype(f64) - 2.2 / float(inp["dt"]) * (x[rows[1]].astype(f64) - x[rows[0]].astype(f64))).astype(f32)
    elif plant and plant[0] == "at_centre":
        r0, r1 = _star_rows(inp, 0), _star_rows(inp, 1)
        x[r0[1]] = x[r0[0]]
        x[r1[0]] = 0.0
        x[r1[1]] = f32([1e-25, 0.0, 0.0])
        inp["star_len"][int(inp["star_ptr"][1]) + 1] = 0.0
    m = c["malform"]
    if m == "bad_atoms":      # rows 0 and n - 1 are spare: they take the place (and the values) of the atoms the entries named
        sp = inp["star_ptr"]
        for slot, bad, row in ((int(sp[2]) + 1, -2, 0), (int(sp[9]), n + 1, n - 1)):
            old = int(inp["star_atom"][slot])
            for k in ("x", "v", "f", "mass"):
                inp[k][row] = inp[k][old]
            inp["star_atom"][slot] = bad
    elif m == "bad_free":
        inp["free_atom"][0], inp["free_atom"][F - 1] = -1, n + 1
    elif m == "row7":      # star 1 (four satellites) gets two more slots: atoms of the free list's end, taken off that list
        sp, t = inp["star_ptr"], 1
        assert sp[t + 1] - sp[t] == 5
        extra = inp["free_atom"][-2:].copy()
        inp["free_atom"], inp["F"] = inp["free_atom"][:-2].copy(), F - 2
        inp["graph_free_ptr"][-1] -= 2
        at = int(sp[t + 1])
        inp["star_atom"] = _i64(np.insert(inp["star_atom"], at, extra))
        inp["star_len"] = np.insert(inp["star_len"], at, f32([1.0, 1.25])).astype(f32)
        inp["star_ptr"][t + 1:] += 2
        inp["n_slots"] += 2
    elif m == "ptr_decreasing":
        inp["star_ptr"][S] = inp["star_ptr"][S - 1] - 3
    elif m == "ptr_past_slots":
        assert inp["star_ptr"][S] - inp["star_ptr"][S - 1] == 4
        inp["n_slots"] -= 2
    elif m == "bad_graph_ptrs":      # one more graph behind the real ones: the decreasing pair
        inp["graph_star_ptr"] = _i64([-3] + list(inp["graph_star_ptr"][1:-1]) + [S + 2, 5])
        inp["graph_free_ptr"] = _i64([-1] + list(inp["graph_free_ptr"][1:-1]) + [F + 3, 2])
        inp["node_ptr"] = _i64(list(inp["node_ptr"]) + [n])
        inp["G"] += 1
    elif m == "garbage_node_ptr":
        inp["node_ptr"] = _i64(rng.integers(-2 ** 40, 2 ** 40, inp["G"] + 1))
    return inp


def inputs_drift(c):
    rng = _rng(c)
    n, behind = c["n"], 3
    x, v, f = (rng.standard_normal((n + behind, 3)).astype(f32) * f32(s) for s in (9.0, 1.0, 1.0))
    return dict(n=n, x=x, v=v, f=f, mass=rng.uniform(0.5, 12.0, n + behind).astype(f32), dt=f32(c["dt"]))


def inputs_kick(c):
    rng = _rng(c)
    sizes = c["sizes"]
    n, behind, G = sum(sizes), 3, len(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    if c["ptr"] is not None:
        ptr = [n + 2 if p == "n+2" else p for p in c["ptr"]]
        assert len(ptr) == G + 1
    v, f = (rng.standard_normal((n + behind, 3)).astype(f32) for _ in range(2))
    return dict(n=n, G=G, v=v, f=f, mass=rng.uniform(0.5, 12.0, n + behind).astype(f32), node_ptr=_i64(ptr), dt=f32(c["dt"]),
                c=f32(c["c"]), s=f32(c["s"]), word0=c["word0"], draw=c["draw"], energy=rng.standard_normal(G + 1).astype(f32))


# what is planted per graph: sign of P, |v|, |f|, state row (dt, alpha, n_pos); |dr| = dt' |v'| against maxstep = 0.2
FIRE_PLANTS = {"downhill_young": (+1, 0.5, 2.0, (0.1, 0.1, 2.0)),          # n_pos <= n_min: dt, alpha stay; 0.1 * ~0.6: not clipped
               "downhill_old": (+1, 5.0, 2.0, (0.1, 0.07, 9.0)),           # dt -> 0.11, alpha -> 0.0693; 0.11 * ~5: clipped
               "uphill": (-1, 5.0, 30.0, (0.2, 0.05, 9.0)),                # v <- 0, dt -> 0.1, alpha -> 0.1, n_pos -> 0; 0.1 * 3: clipped
               "at_rest_capped": (0, 0.0, 0.5, (0.47, 0.1, 7.0)),          # P = 0 is downhill; dt -> min(0.517, 0.5); 0.25 * 0.5: not clipped
               "frozen": (+1, 5.0, None, (0.1, 0.1, 3.0)),                 # fmax = ftol / 2: v <- 0, x and (dt, alpha, n_pos) stay
               "zero_forces": (None, 1.5, 0.0, (0.1, 0.07, 9.0)),          # (ftol = 0) f = 0: v <- (1 - alpha) v, dt -> 0.11; 0.165: not clipped
               "empty": (None, None, None, (0.3, 0.08, 9.0))}


def inputs_fire(c):
    rng = _rng(c)
    sizes = c["sizes"]
    n, behind, G = sum(sizes), 3, len(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    x, v, f = (rng.standard_normal((n + behind, 3)) for _ in range(3))
    x *= 9.0
    state = np.zeros((G, 4), f32)
    for g, name in enumerate(c["plants"]):
        a, b = int(ptr[g]), int(ptr[g + 1])
        sign, vnorm, fnorm, row = FIRE_PLANTS[name]
        assert (name == "empty") == (a == b)
        state[g] = row + (np.inf,)
        if a == b:
            continue
        fg = f[a:b]
        fg *= (0.5 * FIRE["ftol"] / np.linalg.norm(fg, axis=1).max()) if fnorm is None else fnorm / np.linalg.norm(fg)
        if sign == 0:
            v[a:b] = 0.0
        elif sign is None:
            v[a:b] *= vnorm / np.linalg.norm(v[a:b])
        else:      # cos(f, v) = +- 0.45
            r = v[a:b]
            r = r + sign * 0.5 * np.linalg.norm(r) * fg / np.linalg.norm(fg) - (r * fg).sum() * fg / (fg * fg).sum()
            v[a:b] = r * (vnorm / np.linalg.norm(r))
    p = {k: (f32(val) if k != "n_min" else val) for k, val in dict(FIRE, ftol=c["ftol"]).items()}
    return dict(n=n, G=G, x=x.astype(f32), v=v.astype(f32), f=f.astype(f32), node_ptr=_i64(ptr), state=state, p=p,
                energy=rng.standard_normal(G).astype(f32))


# a small valid problem of every entry point; a refusal replaces one argument
def inputs_refuse(c):
    rng = _rng(c)
    inp = star_system(rng, [((2, 1), 3), ((1,), 2)])
    inp.update(dt=0.05, tol=1e-5, max_iter=32, c=0.9, s=0.45, draw=3, word0=0, state=np.tile(f32([0.1, 0.1, 2.0, np.inf]), (2, 1)),
               energy=rng.standard_normal(2).astype(f32), **{k: float(v) for k, v in FIRE.items() if k != "n_min"}, n_min=FIRE["n_min"])
    return inp


INPUTS = dict(drift=inputs_drift, kick=inputs_kick, fire=inputs_fire, shake=inputs_star, rattle=inputs_star, refuse=inputs_refuse)


# ---------------------------------------------------------------------------------------------------------------------------------
# every kind's outputs under an arithmetic: {name: (value float64, bound)}; star kinds: see compute_shake / compute_rattle
def compute_drift(c, inp, B, mutant=None):
    n, mass = inp["n"], inp["mass"]
    m = mass[:n, None]
    if mutant == "drift_mass_by_component":
        m = mass[np.minimum(np.arange(3 * n), len(mass) - 1)].reshape(n, 3)
    x, v = drift_model(B, B.lit(inp["x"][:n]), B.lit(inp["v"][:n]), B.lit(inp["f"][:n]), B.lit(m), B.lit(inp["dt"]), mutant)
    return dict(x=B.pair(x), v=B.pair(v))


def compute_kick(c, inp, B, mutant=None):
    n, G, ptr = inp["n"], inp["G"], inp["node_ptr"]
    v_val, v_err = inp["v"][:n].astype(f64), np.zeros((n, 3))
    ke_val, ke_err = np.zeros(G), np.zeros(G)
    for g in range(G):
        beg, end = _clip(ptr[g], 0, n), _clip(ptr[g + 1], 0, n)
        rows = np.arange(beg, max(beg, end))
        if mutant == "kick_drops_nodes_from_64":
            rows = rows[:64]
        if len(rows) == 0:
            continue
        vin = B.lit(inp["v"][rows])
        vn = ou_kick(B, vin, None if c["fnull"] else B.lit(inp["f"][rows]), B.lit(inp["mass"][rows, None]), B.lit(inp["dt"]),
                     B.lit(inp["c"]), B.lit(inp["s"]), draws(B, inp, rows, mutant) if float(inp["s"]) != 0.0 else None, mutant)
        v_val[rows], v_err[rows] = B.pair(vn)
        hm, q = ke_terms(B, vin if mutant == "kick_ke_before_the_kick" else vn, B.lit(inp["mass"][rows]), True)
        ke_val[g], ke_err[g] = B.pair(B.wave(_lanes(len(rows)), hm, q, True))
    out = dict(v=(v_val, v_err))
    if c["kin"]:
        out["kinetic"] = (ke_val, ke_err)
    if c["pot"]:
        e = inp["energy"][1:G + 1] if mutant == "potential_from_the_next_graph" else inp["energy"][:G]
        out["potential"] = (e.astype(f64), np.zeros(G))
    return out


def compute_fire(c, inp, B, mutant=None):
    n, G, ptr = inp["n"], inp["G"], inp["node_ptr"]
    out = {k: (inp[k][:n].astype(f64), np.zeros((n, 3))) for k in ("x", "v")}
    st_val, st_err = inp["state"].astype(f64), np.zeros((G, 4))
    p = {k: (B.lit(val) if k != "n_min" else val) for k, val in inp["p"].items()}
    names = []
    for g in range(G):
        beg, end = _clip(ptr[g], 0, n), _clip(ptr[g + 1], 0, n)
        rows = np.arange(beg, max(beg, end))
        row = inp["state"][g]
        x, v, (dt, alpha, n_pos, fmax), name = fire_graph(B, *(B.lit(inp[k][rows]) for k in ("x", "v", "f")),
                                                          (B.lit(row[0]), B.lit(row[1]), float(row[2])), p, mutant)
        names.append(name)
        for k, t in (("x", x), ("v", v)):
            if t is not None:
                out[k][0][rows], out[k][1][rows] = B.pair(t, (len(rows), 3))
        for j, t in enumerate((dt, alpha, B.lit(n_pos), fmax)):
            st_val[g, j], st_err[g, j] = B.pair(t)
        if name in ("empty", "frozen"):      # (dt, alpha, n_pos) are not touched: no bound at all
            st_err[g, :3] = 0.0
        st_err[g, 2] = 0.0                   # n_pos: small integers, exact
        assert st_val[g, 2] == round(st_val[g, 2])
    out["state"] = (st_val, st_err)
    if c["records"]:
        out["erec"] = (inp["energy"].astype(f64), np.zeros(G))
        out["frec"] = (st_val[:, 3].copy(), st_err[:, 3].copy())
    out["_branches"] = names
    return out


def _atoms(B, inp, key, rows):
    return [B.lit(inp[key][i]) for i in rows]


def compute_shake(c, inp, B, mutant=None):
    """Free atoms: {"x", "v"} as (value, bound) on every row (rows no thread owns: their old value, bound 0).  Stars: ``stars`` =
    [(rows, runs)], runs = the executions fp32 may take, each (x [k, 3] pair, v pair or None, failed); None: left out."""
    n, S, F = inp["n"], inp["S"], inp["F"]
    out = {k: (inp[k].astype(f64), np.zeros((n, 3))) for k in ("x", "v")}
    if not c["fnull"] and F:
        rows = np.array([_clip(i, 0, n - 1) for i in inp["free_atom"][:F]])
        x, v = drift_model(B, *(B.lit(inp[k][rows]) for k in ("x", "v", "f")), B.lit(inp["mass"][rows, None]), B.lit(inp["dt"]), mutant)
        for k, t in (("x", x), ("v", v)):
            out[k][0][rows], out[k][1][rows] = B.pair(t)
    stars = []
    for t in range(S):
        star = load_star(inp, t, n, mutant)
        if star is None:
            continue
        rows, d0 = star

        def run(D):
            x, v, fail = shake_star(B, D, _atoms(B, inp, "x", rows), _atoms(B, inp, "v", rows),
                                    None if c["fnull"] else _atoms(B, inp, "f", rows), [B.lit(inp["mass"][i]) for i in rows],
                                    [B.lit(d) for d in d0], B.lit(inp["dt"]), B.lit(inp["tol"]), inp["max_iter"], mutant)
            return _stack(B, x), None if v is None else _stack(B, v), fail

        stars.append((rows, continuations(run) if B.ev else [run(Decide32())], d0))
    out["stars"] = stars
    return out


def _stack(B, items):
    pairs = [B.pair(t, (3,)) for t in items]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def compute_rattle(c, inp, B, mutant=None):
    """As compute_shake for "v"; ``graphs`` = per graph (stars' indices into ``stars``, free rows) in the kernel's lane order, for the
    kinetic energies (``rattle_energies``); "potential" as the kick's."""
    n, S, F, G = inp["n"], inp["S"], inp["F"], inp["G"]
    out = dict(v=(inp["v"].astype(f64), np.zeros((n, 3))))
    dt, cc, ss = B.lit(inp["dt"]), B.lit(inp["c"]), B.lit(inp["s"])
    noisy = float(inp["s"]) != 0.0

    def kicked(rows, places):
        rows = np.asarray(rows)
        xi = draws(B, inp, places if mutant == "rattle_noise_by_table_position" else rows, mutant) if noisy else None
        return ou_kick(B, B.lit(inp["v"][rows]), None if c["fnull"] else B.lit(inp["f"][rows]), B.lit(inp["mass"][rows, None]), dt, cc, ss,
                       xi, mutant)

    stars, graphs, free_u = [], [], {}
    for g in range(G):
        s_beg = _clip(inp["graph_star_ptr"][g], 0, S)
        s_end = _clip(inp["graph_star_ptr"][g + 1], s_beg, S)
        f_beg = _clip(inp["graph_free_ptr"][g], 0, F)
        f_end = _clip(inp["graph_free_ptr"][g + 1], f_beg, F)
        mine = []
        for t in range(s_beg, min(s_end, s_beg + 64) if mutant == "rattle_skips_the_second_round" else s_end):
            star = load_star(inp, t, n, mutant)
            if star is None:
                mine.append(None)
                continue
            rows, d0 = star
            beg = _clip(inp["star_ptr"][t], 0, int(inp["n_slots"]))
            u0 = kicked(rows, np.arange(beg, beg + len(rows)))

            def run(D):
                u, fail = rattle_star(B, D, [B.ix_row(u0, a) for a in range(len(rows))], _atoms(B, inp, "x", rows),
                                      [B.lit(inp["mass"][i]) for i in rows], [B.lit(d) for d in d0], B.lit(inp["tol"]), inp["max_iter"],
                                      mutant)
                return _stack(B, u0_rows(B, u0, len(rows)) if mutant == "rattle_ke_unprojected" else u), _stack(B, u), fail

            mine.append(len(stars))
            stars.append((rows, continuations(run) if B.ev else [run(Decide32())], d0))
        rows = np.array([_clip(i, 0, n - 1) for i in inp["free_atom"][f_beg:f_end]], np.int64)
        if len(rows):
            u = kicked(rows, np.arange(f_beg, f_end))
            out["v"][0][rows], out["v"][1][rows] = B.pair(u)
        graphs.append((mine, rows))
    out["stars"], out["graphs"] = stars, graphs
    if c["pot"]:
        out["potential"] = (inp["energy"][:G].astype(f64), np.zeros(G))
    return out


def u0_rows(B, u0, k):
    return [B.ix_row(u0, a) for a in range(k)]


def rattle_energies(c, inp, B, out, chosen):
    """kinetic [G] (value, bound) of the projected velocities: ``chosen[i]`` is star i's run (its first entry: the velocities the
    energy is taken from) or None (left out: no bound); the lane order of the kernel for B32, any order for the reference"""
    G = inp["G"]
    ke_val, ke_err = np.zeros(G), np.zeros(G)
    for g, (mine, free_rows) in enumerate(out["graphs"]):
        lanes, vals, errs, ms, left_out = [[] for _ in range(64)], [], [], [], False
        for j, i in enumerate(mine):
            if i is None:
                continue
            if chosen[i] is None:
                left_out = True
                continue
            rows = out["stars"][i][0]
            lanes[j % 64] += list(range(len(ms), len(ms) + len(rows)))
            vals.append(chosen[i][0][0])
            errs.append(chosen[i][0][1])
            ms += [inp["mass"][r] for r in rows]
        for j, r in enumerate(free_rows):
            lanes[j % 64].append(len(ms))
            vals.append(out["v"][0][r][None])
            errs.append(out["v"][1][r][None])
            ms.append(inp["mass"][r])
        if left_out:
            ke_val[g], ke_err[g] = np.nan, np.inf
        elif ms:
            v = EV(np.concatenate(vals), np.concatenate(errs)) if B.ev else np.concatenate(vals).astype(f32)
            hm, q = ke_terms(B, v, B.lit(np.array(ms, f32)), False)
            ke_val[g], ke_err[g] = B.pair(B.wave(lanes, hm, q, False))
    return ke_val, ke_err


COMPUTE = dict(drift=compute_drift, kick=compute_kick, fire=compute_fire, shake=compute_shake, rattle=compute_rattle,
               refuse=lambda c, inp, B, mutant=None: {})


def model32(c, inp, contract, mutant=None):
    """what a float32 model of the case's kernel writes: {name: array}, ``counter`` among them for the star kinds"""
    B = B32(contract)
    out = COMPUTE[c["kind"]](c, inp, B, mutant)
    got = {k: t[0] for k, t in out.items() if isinstance(t, tuple)}
    if c["kind"] in ("shake", "rattle"):
        fails = 0
        for rows, runs, _ in out["stars"]:
            xs, vs, fail = runs[0]
            fails += bool(fail)
            if c["kind"] == "shake":
                got["x"][rows] = xs[0]
                if vs is not None:
                    got["v"][rows] = vs[0]
            else:
                got["v"][rows] = vs[0]
        got["counter"] = inp["counter0"] + fails
        if c["kind"] == "rattle" and c["kin"]:
            got["kinetic"] = rattle_energies(c, inp, B, out, [runs[0] for _, runs, _ in out["stars"]])[0]
    return got


def stopping_rule_ratio(c, inp, rows, d0, x, v):
    """a left-out star against the stopping rule alone, with the bounds of tests/md_constraint_stubs.assert_constraints_hold"""
    tol, worst, xmax = float(inp["tol"]), 0.0, np.abs(x).max()
    for a in range(1, len(rows)):
        r, d = x[rows[a]] - x[rows[0]], float(d0[a - 1])
        if c["kind"] == "shake":
            worst = max(worst, abs(np.linalg.norm(r) / d - 1.0) / (tol * (1 + tol) + 2 * np.sqrt(3.0) * 2 * U24 * xmax / d))
        if c["kind"] == "rattle" or not c["fnull"]:
            speed = np.linalg.norm(v[rows[0]]) + np.linalg.norm(v[rows[a]])
            if c["kind"] == "rattle":
                worst = max(worst, abs(r @ (v[rows[a]] - v[rows[0]])) / (tol * d * speed + 8 * U24 * np.linalg.norm(r) * speed))
    return worst


def expected(c, inp, ref, got):
    """(close, counter range, left out): ``close`` = {name: (want, bound)} for every float output; for the star kinds the runs are
    chosen by ``got`` (x, v as float64 arrays): per star the first run within whose bounds ALL its outputs lie (none: the first, so
    that the comparison fails there); a left-out star is held to the stopping rule and gets no bound."""
    close = {k: (t[0].copy(), t[1].copy()) for k, t in ref.items() if isinstance(t, tuple)}
    if c["kind"] not in ("shake", "rattle"):
        return close, None, 0
    lo = hi = inp["counter0"]
    chosen, left_out = [], 0
    fields = (("x", 0), ("v", 1)) if c["kind"] == "shake" else (("v", 1),)
    for rows, runs, d0 in ref["stars"]:
        if runs is None:
            left_out += 1
            chosen.append(None)
            hi += 1
            ratio = stopping_rule_ratio(c, inp, rows, d0, got.get("x", inp["x"].astype(f64)), got["v"])
            for k, _ in fields:
                close[k][0][rows], close[k][1][rows] = got[k][rows], np.inf if ratio <= 1.0 else 0.0
            continue
        fits = [r for r in runs if all(r[j] is None or (np.abs(got[k][rows] - r[j][0]) <= r[j][1]).all() for k, j in fields)]
        lo += min(bool(r[2]) for r in (fits or runs[:1]))
        hi += max(bool(r[2]) for r in (fits or runs[:1]))
        run = (fits or runs)[0]
        chosen.append(run)
        for k, j in fields:
            if run[j] is not None:
                close[k][0][rows], close[k][1][rows] = run[j]
    if c["kind"] == "rattle" and c["kin"]:
        close["kinetic"] = rattle_energies(c, inp, BEV(), ref, chosen)
    return close, (lo, hi), left_out


def ratio_of(close, counter, got):
    """worst |got - want| / bound over a case's outputs (a moved word with no bound, or a counter out of range: inf)"""
    worst = 0.0
    for name, (want, bound) in close.items():
        err = np.abs(np.asarray(got[name], f64) - want)
        err = np.where(np.isnan(want) & np.isinf(bound), 0.0, err)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        worst = max(worst, float(np.nan_to_num(r, nan=np.inf, posinf=np.inf).max()) if r.size else 0.0)
    if counter is not None and not counter[0] <= got["counter"] <= counter[1]:
        worst = np.inf
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# running the cases
WORST = {}


class Check(_Check):
    def finish(self):
        self.unchanged()
        for family, r in self.ratios.items():
            print(f"{self.case['id']}: {family} worst error / bound {r:.3f}")
            WORST[family] = max(WORST.get(family, 0.0), r)
            record_measured("test_gpu_md_matrix", case=self.case["id"], family=family, error_over_bound=r)


def _arena(c):
    return Arena(zlib.crc32(c["id"].encode()))


def _rows(ar, inp, names, pads=False, copies=("",)):
    """x, v, f [n, 3] and mass [n] blocks (with their rows behind n where the inputs have them); pads: guard blocks of 8 words on
    both sides, so that an access two rows out of range still lands inside the arena"""
    for sfx in copies:
        for k in names:
            if sfx and k in ("f", "mass"):
                continue
            if pads:
                ar.alloc(f"pad_{k}{sfx}_lo", 8)
            ar.alloc(k + sfx, max(inp[k].size, 1), inp[k] if inp[k].size else None)
            if pads:
                ar.alloc(f"pad_{k}{sfx}_hi", 8)


def _ptr64(ar, name, a):
    ar.alloc(name, 2 * max(len(a), 1), _i64(a) if len(a) else None, align=2)


def _fam(c, name):
    return f"{c['kind']}_{name}"


def _close_all(ck, c, close, skip=()):
    for name, (want, bound) in close.items():
        if name not in skip and want.size:
            ck.close(name, want, bound, _fam(c, name))


def run_drift(dev, c, L):
    lib, st, inp = L.load(), L.stream_ptr(), INPUTS["drift"](c)
    ar = _arena(c)
    _rows(ar, inp, ("x", "v", "f", "mass"))
    ar.upload(dev)
    assert lib.e3k_md_drift(ar.p("x"), ar.p("v"), ar.p("f"), ar.p("mass"), inp["n"], float(inp["dt"]), st) == E3K_OK
    ck = Check(ar, c)
    _close_all(ck, c, expected(c, inp, reference(c, inp), None)[0])
    ck.finish()


def _langevin(lib, st, ar, inp, c, v="v", kin="kinetic", pot="potential"):
    lo, hi = L_seed()
    return lib.e3k_md_kick_langevin(ar.p(v), None if c["fnull"] else ar.p("f"), ar.p("mass"), ar.p("node_ptr"), inp["G"], inp["n"],
                                    float(inp["dt"]), float(inp["c"]), float(inp["s"]), lo, hi, inp["draw"] & 0xFFFFFFFF, inp["word0"],
                                    ar.p(kin) if c["kin"] else None, ar.p("energy") if c["pot"] else None,
                                    ar.p(pot) if c["pot"] else None, st)


def L_seed():
    return SEED & 0xFFFFFFFF, (SEED >> 32) & 0xFFFFFFFF


def _records(ar, inp, c, copies=("",)):
    G = inp["G"]
    ar.alloc("energy", len(inp["energy"]), inp["energy"])
    for sfx in copies:
        if c["kin"]:
            ar.alloc("kinetic" + sfx, G)
        if c["pot"]:
            ar.alloc("potential" + sfx, G)


def run_kick(dev, c, L):
    lib, st, inp = L.load(), L.stream_ptr(), INPUTS["kick"](c)
    ar = _arena(c)
    copies = ("", "_twice") + (("_plain",) if c["plain"] else ())
    _rows(ar, inp, ("v", "f", "mass"), pads=c["ptr"] is not None, copies=copies)
    _ptr64(ar, "node_ptr", inp["node_ptr"])
    _records(ar, inp, c, copies)
    ar.upload(dev)
    assert _langevin(lib, st, ar, inp, c) == E3K_OK
    assert _langevin(lib, st, ar, inp, c, "v_twice", "kinetic_twice", "potential_twice") == E3K_OK
    if c["plain"]:
        assert lib.e3k_md_kick(ar.p("v_plain"), ar.p("f"), ar.p("mass"), ar.p("node_ptr"), inp["G"], inp["n"], float(inp["dt"]),
                               ar.p("kinetic_plain"), ar.p("energy"), ar.p("potential_plain"), st) == E3K_OK
    ck = Check(ar, c)
    close = expected(c, inp, reference(c, inp), None)[0]
    _close_all(ck, c, close, skip=("potential",))
    if c["pot"]:
        ck.exact("potential", inp["energy"][:inp["G"]])
    n = inp["n"]
    for g in range(inp["G"]):      # an empty graph's energy is exactly zero
        if c["kin"] and _clip(inp["node_ptr"][g + 1], 0, n) <= _clip(inp["node_ptr"][g], 0, n):
            assert ck.dev("kinetic")[g] == 0
    for sfx in copies[1:]:         # the same bits: a second call; the plain kick
        for name in close:
            ck.exact(name + sfx, ck.dev(name)[:close[name][0].size])
    ck.finish()


def run_fire(dev, c, L):
    lib, st, inp = L.load(), L.stream_ptr(), INPUTS["fire"](c)
    ar, G, n, p = _arena(c), inp["G"], inp["n"], inp["p"]
    copies = ("", "_twice")
    _rows(ar, inp, ("x", "v", "f"), copies=copies)
    _ptr64(ar, "node_ptr", inp["node_ptr"])
    ar.alloc("energy", G, inp["energy"])
    for sfx in copies:
        ar.alloc("state" + sfx, 4 * G, inp["state"])
        if c["records"]:
            ar.alloc("erec" + sfx, G).alloc("frec" + sfx, G)
    ar.upload(dev)
    null = c["null_rows"]
    for sfx in copies:
        rc = lib.e3k_fire_step(None if null else ar.p("x" + sfx), None if null else ar.p("v" + sfx), None if null else ar.p("f"),
                               ar.p("node_ptr"), G, n, ar.p("state" + sfx), float(p["ftol"]), float(p["dt_max"]), float(p["maxstep"]),
                               p["n_min"], float(p["f_inc"]), float(p["f_dec"]), float(p["alpha_start"]), float(p["f_alpha"]),
                               ar.p("energy") if c["records"] else None, ar.p("erec" + sfx) if c["records"] else None,
                               ar.p("frec" + sfx) if c["records"] else None, st)
        assert rc == E3K_OK
    ck = Check(ar, c)
    ref = reference(c, inp)
    close = expected(c, inp, ref, None)[0]
    _close_all(ck, c, close, skip=("erec",))
    if c["records"]:
        ck.exact("erec", inp["energy"])
        assert np.array_equal(ck.dev("frec"), ck.dev("state").reshape(G, 4)[:, 3])      # one fmax, filed twice
    state = ck.dev("state", f32).reshape(G, 4)
    assert np.isfinite(state).all()
    for g, name in enumerate(ref["_branches"]):
        if name in ("empty", "frozen"):      # untouched, bit for bit (x: by Check.unchanged -- no bound was given)
            assert np.array_equal(state[g, :3].view(np.int32), inp["state"][g, :3].view(np.int32)), (name, state[g])
        if name == "empty":
            assert state[g, 3] == 0.0
    for sfx in copies[1:]:
        for name in close:
            if close[name][0].size:
                ck.exact(name + sfx, ck.dev(name)[:close[name][0].size])
    ck.finish()


def _tables(ar, inp):
    for k in ("star_ptr", "star_atom", "free_atom", "graph_star_ptr", "graph_free_ptr", "node_ptr"):
        _ptr64(ar, k, inp[k])
    ar.alloc("star_len", max(len(inp["star_len"]), 1), inp["star_len"] if len(inp["star_len"]) else None)


def _shake_call(lib, st, ar, inp, c, sfx=""):
    return lib.e3k_md_drift_shake(ar.p("x" + sfx), ar.p("v" + sfx), None if c["fnull"] else ar.p("f"), ar.p("mass"), inp["n"],
                                  float(inp["dt"]), ar.p("star_ptr"), ar.p("star_atom"), ar.p("star_len"), inp["S"], inp["n_slots"],
                                  ar.p("free_atom"), inp["F"], float(inp["tol"]), inp["max_iter"], ar.p("counter" + sfx), st)


def _star_verdict(ck, c, inp, got):
    close, counter, left_out = expected(c, inp, reference(c, inp), got)
    assert left_out <= 0.05 * inp["S"], f"{left_out} stars left out"
    assert not (inp["planted"] and left_out)
    value = int(ck.dev("counter")[0])
    assert counter[0] <= value <= counter[1], f"counter {value}, the accepted executions give {counter}"
    ck._claim("counter", 1)
    if inp["planted"]:
        assert counter[0] == counter[1]
    return close


def run_shake(dev, c, L):
    lib, st, inp = L.load(), L.stream_ptr(), INPUTS["shake"](c)
    ar, n = _arena(c), inp["n"]
    copies = ("",) + (("_twice",) if c["twice"] else ()) + (("_drift",) if c["drift_too"] else ())
    _rows(ar, inp, ("x", "v", "f", "mass"), pads=True, copies=copies)
    _tables(ar, inp)
    for sfx in copies:
        ar.alloc("counter" + sfx, 1, np.int32(inp["counter0"]))
    ar.upload(dev)
    assert _shake_call(lib, st, ar, inp, c) == E3K_OK
    if c["twice"]:
        assert _shake_call(lib, st, ar, inp, c, "_twice") == E3K_OK
    if c["drift_too"]:
        assert lib.e3k_md_drift(ar.p("x_drift"), ar.p("v_drift"), ar.p("f"), ar.p("mass"), n, float(inp["dt"]), st) == E3K_OK
    ck = Check(ar, c)
    got = {k: ck.dev(k, f32).reshape(n, 3).astype(f64) for k in ("x", "v")}
    _close_all(ck, c, _star_verdict(ck, c, inp, got))
    if c["twice"]:
        for k in ("x", "v", "counter"):
            ck.exact(k + "_twice", ck.dev(k))
    if c["drift_too"]:      # the free atoms: e3k_md_drift's bits on the same rows (with no star: every row)
        free = inp["free_atom"][:inp["F"]]
        for k in ("x", "v"):
            assert np.array_equal(ck.dev(k).reshape(n, 3)[free], ck.dev(k + "_drift").reshape(n, 3)[free]), k
            if inp["S"] == 0 and inp["F"] == n:
                ck.exact(k + "_drift", ck.dev(k))
            else:
                ck.free(k + "_drift", 3 * n)
        assert ck.dev("counter_drift")[0] == inp["counter0"]
    if c["fnull"]:
        assert np.array_equal(ck.dev("v"), ar.host("v", np.int32))      # v: not a bit moved
    ck.finish()


def _rattle_call(lib, st, ar, inp, c, sfx=""):
    lo, hi = L_seed()
    return lib.e3k_md_kick_rattle(ar.p("v" + sfx), None if c["fnull"] else ar.p("f"), ar.p("mass"), ar.p("node_ptr"), inp["G"], inp["n"],
                                  float(inp["dt"]), float(inp["c"]), float(inp["s"]), lo, hi, inp["draw"] & 0xFFFFFFFF, inp["word0"],
                                  ar.p("kinetic" + sfx) if c["kin"] else None, ar.p("energy") if c["pot"] else None,
                                  ar.p("potential" + sfx) if c["pot"] else None, ar.p("x"), ar.p("star_ptr"), ar.p("star_atom"),
                                  ar.p("star_len"), inp["S"], inp["n_slots"], ar.p("free_atom"), inp["F"], ar.p("graph_star_ptr"),
                                  ar.p("graph_free_ptr"), float(inp["tol"]), inp["max_iter"], ar.p("counter" + sfx), st)


def run_rattle(dev, c, L):
    lib, st, inp = L.load(), L.stream_ptr(), INPUTS["rattle"](c)
    ar, n, G = _arena(c), inp["n"], inp["G"]
    copies = ("",) + (("_twice",) if c["twice"] else ()) + (("_kick",) if c["kick_too"] else ())
    _rows(ar, inp, ("v", "f", "mass"), pads=True, copies=copies)
    _rows(ar, inp, ("x",), pads=True)
    _tables(ar, inp)
    _records(ar, inp, c, copies)
    for sfx in copies:
        ar.alloc("counter" + sfx, 1, np.int32(inp["counter0"]))
    ar.upload(dev)
    assert _rattle_call(lib, st, ar, inp, c) == E3K_OK
    if c["twice"]:
        assert _rattle_call(lib, st, ar, inp, c, "_twice") == E3K_OK
    if c["kick_too"]:
        assert _langevin(lib, st, ar, inp, c, "v_kick", "kinetic_kick", "potential_kick") == E3K_OK
    ck = Check(ar, c)
    got = dict(v=ck.dev("v", f32).reshape(n, 3).astype(f64), x=inp["x"].astype(f64))
    close = _star_verdict(ck, c, inp, got)
    _close_all(ck, c, close, skip=("potential",))
    if c["pot"]:
        ck.exact("potential", inp["energy"][:G])
    for g, (mine, free_rows) in enumerate(reference_graphs(c, inp)):
        if c["kin"] and not len(free_rows) and all(i is None for i in mine):
            assert ck.dev("kinetic")[g] == 0      # an empty graph: exactly zero
    names = ("v",) + (("kinetic",) if c["kin"] else ()) + (("potential",) if c["pot"] else ())
    for sfx in copies[1:]:
        for name in names:
            ck.exact(name + sfx, ck.dev(name))
    if c["twice"]:
        ck.exact("counter_twice", ck.dev("counter"))
    if c["kick_too"]:
        assert ck.dev("counter_kick")[0] == inp["counter0"]
    ck.finish()


_REF = {}


def reference(c, inp):
    """one float64 replay per case and process: the star kinds fork"""
    if c["id"] not in _REF:
        _REF.clear()
        _REF[c["id"]] = COMPUTE[c["kind"]](c, inp, BEV())
    return _REF[c["id"]]


def reference_graphs(c, inp):
    return reference(c, inp)["graphs"]


def _refuse_args(ar, inp, over):
    a = dict(inp, **{k: k for k in ar.blocks})
    a.update(over)
    return a, (lambda k: None if a[k] is None else ar.p(a[k]))


def run_refuse(dev, c, L):
    lib, st, inp = L.load(), L.stream_ptr(), INPUTS["refuse"](c)
    ar, G = _arena(c), inp["G"]
    _rows(ar, inp, ("x", "v", "f", "mass"))
    _tables(ar, inp)
    ar.alloc("energy", G, inp["energy"]).alloc("kinetic", G).alloc("potential", G).alloc("erec", G).alloc("frec", G)
    ar.alloc("state", 4 * G, inp["state"]).alloc("counter", 1, np.int32(0))
    ar.upload(dev)
    a, p = _refuse_args(ar, inp, c["over"])
    lo, hi = L_seed()
    fn = c["fn"]
    tables = lambda: (p("star_ptr"), p("star_atom"), p("star_len"), a["S"], a["n_slots"], p("free_atom"), a["F"])
    if fn == "drift":
        rc = lib.e3k_md_drift(p("x"), p("v"), p("f"), p("mass"), a["n"], a["dt"], st)
    elif fn == "kick":
        rc = lib.e3k_md_kick(p("v"), p("f"), p("mass"), p("node_ptr"), a["G"], a["n"], a["dt"], p("kinetic"), p("energy"), p("potential"), st)
    elif fn == "langevin":
        rc = lib.e3k_md_kick_langevin(p("v"), p("f"), p("mass"), p("node_ptr"), a["G"], a["n"], a["dt"], a["c"], a["s"], lo, hi, a["draw"],
                                      a["word0"], p("kinetic"), p("energy"), p("potential"), st)
    elif fn == "fire":
        rc = lib.e3k_fire_step(p("x"), p("v"), p("f"), p("node_ptr"), a["G"], a["n"], p("state"), a["ftol"], a["dt_max"], a["maxstep"],
                               a["n_min"], a["f_inc"], a["f_dec"], a["alpha_start"], a["f_alpha"], p("energy"), p("erec"), p("frec"), st)
    elif fn == "shake":
        rc = lib.e3k_md_drift_shake(p("x"), p("v"), p("f"), p("mass"), a["n"], a["dt"], *tables(), a["tol"], a["max_iter"], p("counter"), st)
    else:
        assert fn == "rattle"
        rc = lib.e3k_md_kick_rattle(p("v"), p("f"), p("mass"), p("node_ptr"), a["G"], a["n"], a["dt"], a["c"], a["s"], lo, hi, a["draw"],
                                    a["word0"], p("kinetic"), p("energy"), p("potential"), p("x"), *tables(), p("graph_star_ptr"),
                                    p("graph_free_ptr"), a["tol"], a["max_iter"], p("counter"), st)
    assert rc == c["rc"], f"return code {rc}"
    Check(ar, c).finish()


RUNNERS = dict(drift=run_drift, kick=run_kick, fire=run_fire, shake=run_shake, rattle=run_rattle, refuse=run_refuse)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_md_case_against_float64(dev, c):
    from e3_layers_amd.backend import lib as L

    RUNNERS[c["kind"]](dev, c, L)


def test_zz_worst_ratio_per_family(dev):
    """prints what the cases of this run measured (the module's MEASURED is a copy of a full run's)"""
    for family in sorted(WORST):
        print(f"worst error / bound, {family}: {WORST[family]:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
