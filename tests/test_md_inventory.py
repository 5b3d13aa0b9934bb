"""The kernels of csrc/e3k_md.hip that the library ships == the kernels the cases of tests/test_gpu_md_matrix.py name (no GPU needed);
the six functions of the header's MD section == the functions the cases call; and the bounds of that file shown on the CPU to hold
for float32 models of the kernels and to be sharp.

Models.  The kernels' arithmetic is stated once in tests/test_gpu_md_matrix.py (``drift_model``, ``ou_kick``, ``fire_graph``,
``shake_star``, ``rattle_star``) against an arithmetic; ``B32`` is numpy float32, operation for operation -- an ``fmaf`` is
``float32(float64 * float64 + float64)``, the sums over a graph run in the kernel's order (lane l takes l, l + 64, ..., the 64 partial
sums meet in wave_sum's butterfly) -- in two forms: no product fused, and every product the compiler may fuse under
-ffp-contract=fast fused.  Both forms of every case that launches a kernel must stay inside the case's own bounds; the normal draws
are the float64 draws rounded to fp32 (the device's logf and cospif are measured in tests/test_gpu_md_integrator_kernels.py).

Worst error / bound of the models (measured here; FLOORS asserts just under the single-chain families' values -- a bound that the
model comes nowhere near would say little): drift 0.912, kick without noise 0.704 (with noise 0.05 .. 0.23: XI_BOUND is an analytic
bound on the device's library, which numpy's float64 draw does not use up), FIRE 0.970, SHAKE 0.964, RATTLE 0.808.

Branch conditions, asserted here on the inputs: every FIRE decision is clear of its threshold (the float64 replay asserts it where it
decides) and every planted branch occurs; at most 5 % of a case's stars are left out of the elementwise comparison (none is, with
the inputs as they stand); every star of a planted-failure case is fully decided and the counter's range is one number.

Planted mutants.  Each is the model with one error; each must leave its case's own bounds.  Worst error / bound (the assertion is
> 1; printed by the test; inf: a word moved that has no bound at all, or the counter left its range):
    drift: mass[c] for mass[c / 3] 2.1e7, x moved with the old v 1.2e6;
    kick: nodes >= 64 of a graph dropped 4.2e6, kinetic energy from the velocities before the kick 380, noise amplitude s / m 3.8e5
    (in RATTLE 2.6e5), noise word without the component 1.1e6, potential[g] = energy[g + 1] inf;
    FIRE: mix = alpha 1.7e6, dr clipped per atom 1.2e5, P = 0 counted as uphill inf (n_pos);
    SHAKE: correction along the present bond 5.4e3, g / m_s and g / m_c swapped inf (the stars no longer converge; light pairs:
    4.5e4), no centre's share 2.5e4, v from p - old 1.2e6, last pass corrects (counter short by the five planted stars) inf, a row
    of 7 slots used in full inf;
    RATTLE: kinetic energy of the unprojected velocities 1.9e5, noise drawn by table position 4.2e5, second lane round skipped 3.5e5.
One mutant needed a case of its own: the RATTLE cases start from velocities that are on the constraints but for a half kick (so
that the sweeps can be decided, see inputs_star), the projection then changes a graph's kinetic energy by less than gamma_n of its
300 atoms allows, and "kinetic energy of the unprojected velocities" stayed inside every bound (0.74 on rattle_G1).  rattle_raw_pairs
-- six pairs with velocities as drawn, a graph of twelve atoms -- exposes it.
"""
import re

import numpy as np
import pytest

import tests.test_gpu_md_matrix as T
from tests.test_train_inventory import HEADER, _shipped_kernels

BY_ID = {c["id"]: c for c in T.CASES}
LAUNCHING = [c for c in T.CASES if c["kind"] != "refuse"]
FLOORS = {"drift": 0.85, "kick": 0.65, "fire": 0.9, "shake": 0.9, "rattle": 0.75}
MUTANTS = [
    ("drift_mass_by_component", "drift_n85"), ("drift_old_v", "drift_n85"),
    ("kick_drops_nodes_from_64", "kick_G1"), ("kick_ke_before_the_kick", "kick_G1"), ("noise_over_m", "kick_G9_langevin"),
    ("noise_word_without_component", "kick_G9_langevin"), ("potential_from_the_next_graph", "kick_G9_langevin"),
    ("fire_mix_alpha", "fire_G5"), ("fire_clip_per_atom", "fire_G1"), ("fire_p0_uphill", "fire_G5"),
    ("shake_present_bond", "shake_255"), ("shake_masses_swapped", "shake_255"), ("shake_masses_swapped", "shake_light_pairs"),
    ("shake_no_centre_share", "shake_255"), ("shake_v_from_old", "shake_255"), ("shake_last_pass_corrects", "shake_max_iter1"),
    ("star_row_in_full", "shake_row7"),
    ("rattle_ke_unprojected", "rattle_raw_pairs"), ("noise_over_m", "rattle_G9_noise"), ("rattle_noise_by_table_position", "rattle_G9_noise"),
    ("rattle_skips_the_second_round", "rattle_G1"),
]

_CACHE = {}


def _case(cid):
    """(case, inputs, float64 replay) -- once per case and module run"""
    if cid not in _CACHE:
        c = BY_ID[cid]
        inp = T.INPUTS[c["kind"]](c)
        _CACHE[cid] = (c, inp, T.COMPUTE[c["kind"]](c, inp, T.BEV()))
    return _CACHE[cid]


def _ratio(cid, contract, mutant=None):
    c, inp, ref = _case(cid)
    got = T.model32(c, inp, contract, mutant)
    close, counter, _ = T.expected(c, inp, ref, got)
    return T.ratio_of(close, counter, got)


def test_every_md_kernel_has_a_float64_checked_case(tmp_path):
    shipped = _shipped_kernels(tmp_path, "e3k_md.o") - {"zero_words_kernel"}      # (e3k_common.h's helper, in every object)
    assert len(shipped) == 5, sorted(shipped)
    assert shipped == T.table_kernels(), (sorted(shipped), sorted(T.table_kernels()))


def test_every_function_of_the_md_section_is_called_by_a_case():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(e3k_md_\w+|e3k_fire_step)\s*\(", f.read()))
    assert len(declared) == 6, sorted(declared)
    assert declared == T.table_functions(), (sorted(declared), sorted(T.table_functions()))
    for fn in T.FN.values():      # every entry point has launching cases, refusals and a no-op return
        kinds = {(c["kind"], c.get("rc")) for c in T.CASES if fn in c["funcs"]}
        assert {k for k, _ in kinds} - {"refuse"} and ("refuse", T.E3K_ERR_INVALID) in kinds and ("refuse", T.E3K_OK) in kinds, fn


def test_case_ids_are_unique_and_the_issue_values_all_appear():
    ids = [c["id"] for c in T.CASES]
    assert len(ids) == len(set(ids))
    assert all(c["why"] and "kernels" in c and "funcs" in c for c in T.CASES)
    of = lambda kind: [c for c in T.CASES if c["kind"] == kind]
    assert {c["n"] for c in of("drift")} == {1, 85, 86, 171} and any(c["dt"] < 0 for c in of("drift"))
    kicks = of("kick")
    assert {len(c["sizes"]) for c in kicks} >= {1, 4, 5, 9}
    assert set().union(*(c["sizes"] for c in kicks)) >= {0, 1, 63, 64, 65, 129, 200}
    assert any(c["sizes"][0] == 0 for c in kicks) and any(c["sizes"][-1] == 0 for c in kicks)
    for kind in ("kick", "rattle"):
        assert {(c["c"] == 1.0, c["c"] == 0.0, c["s"] == 0.0) for c in of(kind)} >= {(True, False, True), (False, False, True),
                                                                                    (False, True, False), (False, False, False)}, kind
        assert any(c["fnull"] for c in of(kind)) and {c["word0"] for c in of(kind)} == {0, 4}
        assert {(c["kin"], c["pot"]) for c in of(kind)} >= {(True, True), (False, True), (True, False)}
    assert (T.SEED >> 32) and (T.SEED & 0xFFFFFFFF)
    assert any(c["ptr"] is not None and min(p for p in c["ptr"] if p != "n+2") < 0 and "n+2" in c["ptr"] for c in kicks)
    fires = of("fire")
    assert {len(c["sizes"]) for c in fires} >= {1, 5, 9} and set().union(*(c["sizes"] for c in fires)) >= {0, 1, 64, 65, 129}
    assert set().union(*(c["plants"] for c in fires)) == set(T.FIRE_PLANTS)
    assert any(not c["records"] for c in fires) and any(c["null_rows"] for c in fires) and "fire_ftol0_empty" in BY_ID
    shakes = {c["id"]: T.INPUTS["shake"](c) for c in of("shake")}
    assert {i["S"] + i["F"] for i in shakes.values()} >= {1, 255, 256, 257}
    assert any(i["S"] == 0 for i in shakes.values()) and any(i["F"] == 0 for i in shakes.values())
    sats = {int(b - a) - 1 for i in shakes.values() for a, b in zip(i["star_ptr"][:-1], i["star_ptr"][1:])}
    assert sats >= {1, 2, 3, 4, 6}      # (6: the row of 7 slots)
    assert any(c["fnull"] for c in of("shake")) and {c["counter0"] for c in of("shake")} == {0, 7}
    assert {c["malform"] for c in of("shake")} == {None, "bad_atoms", "bad_free", "row7", "ptr_decreasing", "ptr_past_slots"}
    rattles = of("rattle")
    assert {len(c["graphs"]) for c in rattles} >= {1, 5, 9}
    assert any(sum(len(s) >= 70 for s, _ in c["graphs"]) and any(f >= 70 for _, f in c["graphs"]) for c in rattles)
    assert any(any(s and not f for s, f in c["graphs"]) and any(f and not s for s, f in c["graphs"]) and ((), 0) in c["graphs"]
               for c in rattles)
    assert {c["malform"] for c in rattles} == {None, "bad_graph_ptrs", "garbage_node_ptr"}
    assert {c["max_iter"] for c in rattles} == {1, 32} == {c["max_iter"] for c in of("shake")}


def test_malformed_tables_stay_within_two_rows_and_race_with_nobody():
    """every out-of-range table entry is off by at most 2 rows, and after the header's clamps no row has two owners"""
    for c in T.CASES:
        if c["kind"] not in ("shake", "rattle"):
            continue
        inp = T.INPUTS[c["kind"]](c)
        n = inp["n"]
        entries = np.concatenate([inp["star_atom"], inp["free_atom"][:inp["F"]]])
        assert entries.min() >= -2 and entries.max() <= n + 1, c["id"]
        owned = [T._clip(i, 0, n - 1) for i in inp["free_atom"][:inp["F"]]]
        for t in range(inp["S"]):
            star = T.load_star(inp, t, n)
            owned += star[0] if star else []
        assert len(owned) == len(set(owned)), c["id"]
        if c["malform"] in ("bad_atoms", "bad_free"):
            assert {0, n - 1} <= set(owned) and entries.min() < 0 and entries.max() >= n, c["id"]


@pytest.mark.parametrize("c", LAUNCHING, ids=[c["id"] for c in LAUNCHING])
def test_float32_models_stay_inside_the_bounds(c):
    c, inp, ref = _case(c["id"])
    if c["kind"] in ("shake", "rattle"):      # the conditions on the inputs
        left_out = sum(runs is None for _, runs, _ in ref["stars"])
        assert left_out <= 0.05 * inp["S"], f"{left_out} of {inp['S']} stars have more than 3 undecided decisions"
        if inp["planted"]:
            assert all(runs is not None and len(runs) == 1 for _, runs, _ in ref["stars"]), "a planted-failure case must be fully decided"
    for contract in (False, True):
        got = T.model32(c, inp, contract)
        close, counter, _ = T.expected(c, inp, ref, got)
        r = T.ratio_of(close, counter, got)
        print(f"{c['id']} contract {contract}: worst error / bound {r:.3f}" + (f", counter {got['counter']} in {counter}" if counter else ""))
        assert r <= 1.0
        if c["kind"] in ("shake", "rattle") and inp["planted"]:
            assert counter[0] == counter[1] == got["counter"]


def test_planted_counters_are_the_numbers_the_cases_state():
    want = {"shake_max_iter1": 12, "shake_turned": 8, "rattle_max_iter1": 18, "rattle_at_centre": 8}
    for cid, value in want.items():
        c, inp, ref = _case(cid)
        got = T.model32(c, inp, False)
        assert T.expected(c, inp, ref, got)[1] == (value, value), cid
    c, inp, ref = _case("rattle_at_centre")      # star 0 (a satellite AT its centre) does not fail, star 1 (|r|^2 underflows) does
    assert [runs[0][2] for _, runs, _ in ref["stars"][:2]] == [False, True]
    c, inp, ref = _case("shake_turned")
    assert [i for i, (_, runs, _) in enumerate(ref["stars"]) if runs[0][2]] == [7]


def test_every_fire_branch_occurs_and_is_clear_of_its_threshold():
    """(the float64 replay asserts the margins where it decides: fire_graph)"""
    seen = set()
    for c in T.CASES:
        if c["kind"] == "fire":
            _, inp, ref = _case(c["id"])
            seen |= set(ref["_branches"])
            for g, (plant, branch) in enumerate(zip(c["plants"], ref["_branches"])):
                want = {"downhill_young": "down", "downhill_old": "down_clipped", "uphill": "up_clipped", "at_rest_capped": "down",
                        "frozen": "frozen", "zero_forces": "down", "empty": "empty"}[plant]
                assert branch == want, (c["id"], g, plant, branch)
                if plant == "at_rest_capped":
                    assert ref["state"][0][g, 0] == float(inp["p"]["dt_max"])
    assert seen == {"empty", "frozen", "down", "down_clipped", "up_clipped"}
    _, inp, ref = _case("fire_ftol0_empty")
    for g in (0, 2):      # the header: an empty graph is frozen with fmax = 0 -- (dt, alpha, n_pos) stay although n_pos > n_min
        assert inp["state"][g, 2] > inp["p"]["n_min"] and (ref["state"][0][g] == [*inp["state"][g, :3].astype(np.float64), 0.0]).all()


def test_single_chain_families_come_near_their_bounds():
    worst = {}
    for c in LAUNCHING:
        if c["kind"] in ("kick", "rattle") and c["s"] != 0.0:
            continue
        worst[c["kind"]] = max(worst.get(c["kind"], 0.0), _ratio(c["id"], False), _ratio(c["id"], True))
    print({k: round(v, 3) for k, v in worst.items()})
    for kind, floor in FLOORS.items():
        assert floor <= worst[kind] <= 1.0, (kind, worst[kind])


@pytest.mark.parametrize("mutant,cid", MUTANTS, ids=[f"{m}-{cid}" for m, cid in MUTANTS])
def test_planted_mutants_leave_the_bounds(mutant, cid):
    assert _ratio(cid, False) <= 1.0
    r = min(_ratio(cid, contract, mutant) for contract in (False, True))
    print(f"{mutant} on {cid}: worst error / bound {r:.3g}")
    assert r > 1.0
