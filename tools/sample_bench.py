#!/usr/bin/env python3
"""Reverse-diffusion sampling throughput.

Molecules (the default): config_diffusion score network, B molecules, fully connected graphs; first `n_iter` steps of the N=1000
predictor-corrector schedule, eager launches vs one HIP graph per step.  Usage: python tools/sample_bench.py [B] [n_iter]

Proteins (``--protein``): config_diffusion_CA as shipped but built with the declarative pair criterion
(``config_diffusion_CA.pair_criterion()``), 4 x 384 synthetic residues, Euler-Maruyama predictor: the replayed loop of
``get_pc_sampler(graph=True, edge_capacity=...)`` (the model's own edge layer rebuilds the capped list inside the graph) against the
eager sampler loop on the same tree and start -- the only way to sample these nets before.

    python tools/sample_bench.py --protein --steps 100 --out profiles/protein_sampler_replay.json
    python tools/sample_bench.py --protein --seed 7 --corrector langevin --steps 100      (-> profiles/protein_sampler_pc.json)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/sample_bench.py --protein --trace-steps 40
    python tools/sample_bench.py --launches DIR_A/..._kernel_stats.csv 10 DIR_B/..._kernel_stats.csv 40    (launches per replayed step)

What is timed is the sampler, not a copy of it: every loop is built from the plan function of the sampler it stands for
(``run/sde_sampling.pc_plan`` / ``ode_plan``, ``run/likelihood.likelihood_plan``) and ``run/loops.make_loop``, as the sampler builds it,
and driven through the loops' one interface -- ``rewind()`` outside the timed region, ``run(n)`` inside, ``result()`` after it -- the
eager loops included.  Where a run starts: the seeded loops from the sampler's own counter-based prior at ``--seed`` (earlier
versions of this tool started every loop from one generator-drawn x_T, so a seeded loop's first list may differ by a few edges from
the figures recorded then); the unseeded loops from ``prior_sampling`` with the device's default generator seeded 1 -- the x_T bits
they always had -- which the plan also hands to the predictor (a captured step can draw from no other generator).

Protocol (tools/md_bench.py's): device events around ``--steps`` reverse steps after a warm-up, the two variants alternating in one
process, ``--reps`` repetitions each (min / median / max); host-busy time is the wall time of the enqueue loop before the closing
synchronisation.  No threshold is asserted: the numbers are quoted in README.md and DESIGN.md.

``--seed S`` times the seeded form (``get_pc_sampler(seed=S)``: counter-based noise, one launch per key around each model call, the
time and the step number in device cells): the seeded replay against the seeded eager loop and -- with ``--corrector none``, the only
corrector the unseeded replay serves -- against the unseeded replay, the three alternating in one process.  ``--trace-steps`` and
``--launches`` then count the seeded replay's launches.

``--fixed FRACTION`` (with ``--seed``) adds the conditioned replay (``get_pc_sampler(fixed=...)``: inpainting): the middle FRACTION of
every chain is kept on its known coordinates, the rest is sampled around it.  The conditioned seeded replay then alternates with the
unconditioned seeded replay of the same tree (and the other variants), ``--trace-steps`` counts ITS launches, and the result goes to
profiles/protein_sampler_fixed.json:

    python tools/sample_bench.py --protein --seed 7 --corrector langevin --fixed 0.25 --steps 100

``--ode euler|heun --ode-steps K`` (with ``--protein --seed S``) times the probability-flow ODE sampler's replayed step
(``get_ode_sampler(graph=True, edge_capacity=...)``: a grid of K steps from T to 1e-3) beside the seeded Euler-Maruyama + Langevin
replay of the same tree: the Heun replay, the Euler replay and the predictor-corrector replay alternate in one process, every
repetition from x_T over the first ``--steps`` (<= K) steps of its schedule.  ``--ode`` names the method ``--trace-steps`` replays
under rocprofv3.  What is timed is a STEP; how many steps a trained network needs is not assessed.  -> profiles/protein_sampler_ode.json

    python tools/sample_bench.py --protein --seed 7 --ode heun --ode-steps 100 --steps 100
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/sample_bench.py --protein --seed 7 --ode heun \
        --ode-steps 100 --trace-steps 40

``--likelihood heun|euler --ode-steps K`` (with ``--protein --seed S``) times the replayed step of the log-likelihood
(``run/likelihood.get_likelihood_fn(graph=True, edge_capacity=...)``: each model call is a forward AND a backward with respect to the
positions, plus one quadrature launch) beside the ODE sampler's replayed Heun step of the same process, alternating, both from the same
state so that both walk lists of one size.  The weights are untrained: the value of logp says nothing about a model and is not reported.
-> profiles/protein_likelihood.json

    python tools/sample_bench.py --protein --seed 7 --likelihood heun --ode-steps 100 --steps 100
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/sample_bench.py --protein --seed 7 \
        --likelihood heun --ode-steps 100 --trace-steps 40"""
import argparse, contextlib, csv, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "equivariant-nn-zoo_amd")):
    sys.path.insert(0, p)
import torch


def molecules(argv):
    from e3_layers_amd.configs import config_diffusion
    from e3_layers_amd.data.synthetic import synth_qm9_diffusion
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler
    from e3_layers_amd.run.sde_utils import VPSDE
    from e3_layers_amd.utils import build

    B = int(argv[0]) if len(argv) > 0 else 128
    n_iter = int(argv[1]) if len(argv) > 1 else 50
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build(config_diffusion.get_config().model_config).to(dev).eval()
    batch = synth_qm9_diffusion(1, B).to(dev)
    print(f"B={B} N={batch['pos'].shape[0]} E={batch['edge_index'].shape[1]}")
    for graph in (False, True):
        sde = VPSDE({"pos": 3}, N=1000)
        sampler = get_pc_sampler(sde, EulerMaruyamaPredictor, LangevinCorrector, snr=0.16, static_edges=True, graph=graph,
                                 n_iter=n_iter)
        sampler(model, batch)          # warm-up (plans, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, nfe = sampler(model, batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"graph={graph}: {dt / n_iter * 1e3:.2f} ms per reverse step ({nfe} network evaluations, incl. capture when graph), "
              f"{B * n_iter / dt:.0f} molecule-steps/s; finite={bool(torch.isfinite(out['pos']).all())}")


# ---- proteins: the replayed loop against the eager loop ---------------------------------------------------------------------------
def protein_setup(n_prot, n_res, dev):
    from e3_layers_amd.configs import config_diffusion_CA
    from e3_layers_amd.data.synthetic import synth_protein
    from e3_layers_amd.run.sde_utils import VPSDE
    from e3_layers_amd.utils import build

    torch.manual_seed(0)
    model = build(config_diffusion_CA.get_config(edge_criteria=config_diffusion_CA.pair_criterion()).model_config).to(dev).eval()
    return model, VPSDE({"CA": 3}, N=1000), synth_protein(1, n_prot, n_res=n_res).to(dev)


def pc(model, sde, batch, seed=None, corrector="none", fixed=None):
    """The plan of ``get_pc_sampler(sde, EulerMaruyamaPredictor, <corrector>, seed=seed, fixed=fixed)`` on ``batch``."""
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, NoneCorrector, pc_plan

    gen = None
    if seed is None:      # x_T first, from seed 1; the default generator: the one a captured step may draw from
        gen = torch.cuda.default_generators[batch["CA"].device.index]
        gen.manual_seed(1)
    return pc_plan(sde, EulerMaruyamaPredictor, LangevinCorrector if corrector == "langevin" else NoneCorrector, model, batch,
                   generator=gen, seed=seed, fixed=fixed)[0]


def first_edges(model, plan):
    """The edges of the list the model's own layer builds on the plan's start state (the draw of build 0; none is consumed)."""
    from e3_layers_amd.run.capped import builder_cells, edge_layer_of

    probe = plan.batch.view()
    probe.data["_nlist_rng"] = builder_cells(plan.cells.device)
    new, _ = edge_layer_of(model).layer(probe.data, probe.attrs)
    return int(new["edge_index"].shape[1])


def capacity(edges, slack):
    return -(-int(slack * edges) // 1024) * 1024


def loop_of(plan, model, e_cap=None, frozen=False):
    """``make_loop`` as the samplers call it on these nets: the capped replay at ``e_cap`` (sized, padded and captured here, outside any
    timed region), the eager loop without.  ``frozen``: inside ``frozen_parameters(model)``, as the likelihood builds and runs."""
    from e3_layers_amd.run.capped import edge_layer_of
    from e3_layers_amd.run.likelihood import frozen_parameters
    from e3_layers_amd.run.loops import edge_plumbing, make_loop

    with torch.no_grad(), (frozen_parameters(model) if frozen else contextlib.nullcontext()):
        return make_loop(plan, model, edge_plumbing((), False)[1], graph=e_cap is not None, edge_capacity=e_cap,
                         r_max=edge_layer_of(model).r_max, criteria=None)


def with_mask(clean, fraction):
    """``clean`` with the mask field ``fixed`` that ``get_pc_sampler(fixed="fixed")`` reads: the middle ``fraction`` of every chain of
    every protein (a contiguous stretch, chosen by the chain's length alone); the known values are the batch's own coordinates.
    -> (batch, fixed rows)"""
    b = clean.clone()
    chain = clean["chain_id"].reshape(-1) + (int(clean["chain_id"].max()) + 1) * clean.nodeSegment()
    mask = torch.zeros_like(chain, dtype=torch.bool)
    for c in torch.unique(chain).tolist():
        rows = torch.nonzero(chain == c).reshape(-1)
        k = int(round(fraction * rows.numel()))
        start = (rows.numel() - k) // 2
        mask[rows[start:start + k]] = True
    b.attrs["fixed"] = ("node", "1x0e")
    b["fixed"] = mask.reshape(-1, 1).to(torch.uint8)
    return b, int(mask.sum())


def run_of(loop, n):
    """``loop`` rewound; -> a callable that does ``n`` steps and returns the host's busy time"""
    loop.rewind()      # (outside the timed region)

    def run():
        t0 = time.perf_counter()
        with torch.no_grad():
            loop.run(n)
        return time.perf_counter() - t0
    return run


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    host = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def total_calls(path):
    with open(path) as f:
        return sum(int(r["Calls"]) for r in csv.DictReader(f))


def mmm(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def protein(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--protein", action="store_true")
    ap.add_argument("--proteins", type=int, default=4)
    ap.add_argument("--residues", type=int, default=384)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slack", type=float, default=1.15, help="edge capacity = slack x the first list, rounded up to 1024")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0, help="run this many replayed steps and nothing else (under rocprofv3)")
    ap.add_argument("--seed", type=int, default=None, help="time the seeded form (get_pc_sampler(seed=...)) as well")
    ap.add_argument("--corrector", choices=("none", "langevin"), default="none", help="with --seed: the corrector of the seeded loops")
    ap.add_argument("--fixed", type=float, default=0.0, help="with --seed: the conditioned replay too, this fraction of every chain fixed")
    ap.add_argument("--ode", choices=("euler", "heun"), default=None, help="with --seed: the ODE sampler's replays beside the seeded "
                    "Euler-Maruyama + Langevin replay; the method --trace-steps replays")
    ap.add_argument("--ode-steps", type=int, default=None, help="with --ode / --likelihood: the steps of the ODE grid (required)")
    ap.add_argument("--likelihood", choices=("euler", "heun"), default=None, help="with --seed: the likelihood's replays beside the ODE "
                    "sampler's Heun replays")
    args = ap.parse_args(argv)
    if args.likelihood is not None and (args.seed is None or args.ode_steps is None or args.fixed or args.ode is not None):
        raise SystemExit("--likelihood METHOD: with --seed and --ode-steps K, without --fixed and --ode")
    if args.ode is not None and (args.seed is None or args.ode_steps is None or args.fixed):
        raise SystemExit("--ode METHOD: with --seed and --ode-steps K, without --fixed")
    if not 0.0 <= args.fixed < 1.0 or (args.fixed and args.seed is None):
        raise SystemExit("--fixed FRACTION: in [0, 1), with --seed (the conditioned replay is the seeded form's)")
    model, sde, clean = protein_setup(args.proteins, args.residues, torch.device("cuda:0"))
    if args.likelihood is not None:
        return protein_likelihood(args, model, sde, clean)
    if args.ode is not None:
        return protein_ode(args, model, sde, clean)
    if args.seed is not None:
        return protein_seeded(args, model, sde, clean)
    if args.corrector != "none":
        raise SystemExit("--corrector langevin needs --seed: the unseeded replay serves NoneCorrector only")
    plan = pc(model, sde, clean)
    e_cap = capacity(first_edges(model, plan), args.slack)
    loop = loop_of(plan, model, e_cap)
    if args.trace_steps:
        run_of(loop, args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues}))
        return
    eager = loop_of(pc(model, sde, clean), model)
    run_of(loop, args.warmup)()
    run_of(eager, args.warmup)()
    rows = {"replay": [], "eager": [], "replay_host": [], "eager_host": []}
    edges = []
    for _ in range(args.reps):
        ms, host = timed(run_of(loop, args.steps))
        edges.append(int(loop.bucket.state[0]))
        loop.result()                               # (after the closing event: an overflowed repetition would raise here)
        rows["replay"].append(ms / args.steps)
        rows["replay_host"].append(1e3 * host / args.steps)
        ms, host = timed(run_of(eager, args.steps))
        rows["eager"].append(ms / args.steps)
        rows["eager_host"].append(1e3 * host / args.steps)

    doc = {"workload": "reverse diffusion (Euler-Maruyama, NoneCorrector, first steps of N=1000) on config_diffusion_CA as shipped, "
                       "built with pair_criterion(); synth_protein",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues,
           "nodes": int(clean["CA"].shape[0]), "edges_first_list": loop.first_edges, "edges_last_list": edges, "e_cap": e_cap,
           "n_cap": loop.bucket.n_cap, "steps": args.steps, "reps": args.reps, "recaptures": loop.step.recaptures,
           "replay_ms_per_step": mmm(rows["replay"]), "eager_ms_per_step": mmm(rows["eager"]),
           "replay_host_busy_ms_per_step": mmm(rows["replay_host"]), "eager_host_busy_ms_per_step": mmm(rows["eager_host"]),
           "speedup_median": round(statistics.median(rows["eager"]) / statistics.median(rows["replay"]), 3)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def protein_seeded(args, model, sde, clean):
    """The seeded replay, the seeded eager loop and (NoneCorrector only) the unseeded replay, alternating; with ``--fixed`` the
    conditioned seeded replay as well."""
    plan = pc(model, sde, clean, args.seed, args.corrector)
    e_cap = capacity(first_edges(model, plan), args.slack)
    if args.corrector == "langevin":      # (two model calls per step, and the corrector moves the nodes before the second list)
        e_cap = capacity(e_cap, 1.1)
    loop = loop_of(plan, model, e_cap)
    cond = n_fixed = None
    if args.fixed:      # (the same capacity: the fixed rows start near their clean places, the rest as before)
        masked, n_fixed = with_mask(clean, args.fixed)
        cond = loop_of(pc(model, sde, masked, args.seed, args.corrector, fixed="fixed"), model, e_cap)
    if args.trace_steps:
        run_of(loop if cond is None else cond, args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
                          "corrector": args.corrector, "fixed": args.fixed}))
        return
    loops = {"seeded_replay": loop, "seeded_eager": loop_of(pc(model, sde, clean, args.seed, args.corrector), model)}
    if cond is not None:
        loops["fixed_replay"] = cond
    if args.corrector == "none":
        loops["replay"] = loop_of(pc(model, sde, clean), model, e_cap)
    for which in loops.values():
        run_of(which, args.warmup)()
    rows = {name: [] for name in loops}
    host = {name: [] for name in loops}
    for _ in range(args.reps):
        for name, which in loops.items():
            ms, busy = timed(run_of(which, args.steps))
            if name != "seeded_eager":
                which.result()                      # (after the closing event: an overflowed repetition would raise here)
            rows[name].append(ms / args.steps)
            host[name].append(1e3 * busy / args.steps)

    doc = {"workload": f"reverse diffusion (Euler-Maruyama, corrector {args.corrector}, first steps of N=1000) on config_diffusion_CA as "
                       "shipped, built with pair_criterion(); synth_protein; seeded form",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
           "corrector": args.corrector, "nodes": int(clean["CA"].shape[0]), "edges_first_list": loop.first_edges, "e_cap": e_cap,
           "n_cap": loop.bucket.n_cap, "steps": args.steps, "reps": args.reps, "recaptures": loop.step.recaptures}
    for name in loops:
        doc[f"{name}_ms_per_step"] = mmm(rows[name])
        doc[f"{name}_host_busy_ms_per_step"] = mmm(host[name])
    if "replay" not in loops:
        doc["replay_ms_per_step"] = "not measured: the unseeded replay refuses the Langevin corrector"
    doc["speedup_median_seeded_replay_over_seeded_eager"] = round(statistics.median(rows["seeded_eager"]) / statistics.median(rows["seeded_replay"]), 3)
    if cond is not None:
        lo, hi = min(rows["seeded_replay"]), max(rows["seeded_replay"])
        med = statistics.median(rows["fixed_replay"])
        doc.update(fixed_fraction=args.fixed, fixed_nodes=n_fixed, fixed_recaptures=cond.step.recaptures,
                   fixed_replay_median_inside_seeded_replay_min_max=bool(lo <= med <= hi),
                   fixed_replay_over_seeded_replay_median=round(med / statistics.median(rows["seeded_replay"]), 4))
    text = json.dumps(doc, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", "protein_sampler_fixed.json" if cond is not None else "protein_sampler_pc.json")
    with open(out, "w") as f:
        f.write(text + "\n")


def ode(model, sde, batch, method, args):
    """The plan of ``get_ode_sampler(sde, method=method, n_steps=args.ode_steps, seed=args.seed)`` on ``batch``."""
    from e3_layers_amd.run.sde_sampling import ode_plan

    return ode_plan(sde, method, model, batch, n_steps=args.ode_steps, seed=args.seed)


def grid_checked(args):
    n_timed = args.trace_steps or args.steps
    if not 1 <= n_timed <= args.ode_steps or args.warmup > args.ode_steps:
        raise SystemExit(f"--steps / --trace-steps / --warmup: at most --ode-steps = {args.ode_steps} (a run stops at the end of its grid)")


def alternate(args, loops):
    """Warm-up, then ``--reps`` rounds over ``loops`` (name -> capped replay), each repetition from the loop's start state.
    -> (ms per step, host-busy ms per step, edges of the last list), each name -> list"""
    rows, host, edges = ({name: [] for name in loops} for _ in range(3))
    for name, loop in loops.items():
        run_of(loop, args.warmup)()
    for _ in range(args.reps):
        for name, loop in loops.items():
            ms, busy = timed(run_of(loop, args.steps))
            edges[name].append(int(loop.bucket.state[0]))
            loop.result()                                   # (after the closing event: an overflowed repetition would raise here)
            rows[name].append(ms / args.steps)
            host[name].append(1e3 * busy / args.steps)
    return rows, host, edges


def protein_ode(args, model, sde, clean):
    """The Heun replay, the Euler replay and the seeded Euler-Maruyama + Langevin replay, alternating, each repetition from x_T."""
    grid_checked(args)
    heun = ode(model, sde, clean, "heun", args)
    # (the seeded Langevin replay's capacity; the same for every loop here: all start from the x_T of one seed)
    e_cap = capacity(capacity(first_edges(model, heun), args.slack), 1.1)
    if args.trace_steps:
        run_of(loop_of(heun if args.ode == "heun" else ode(model, sde, clean, "euler", args), model, e_cap), args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
                          "ode": args.ode, "ode_steps": args.ode_steps}))
        return
    loops = {"ode_heun_replay": loop_of(heun, model, e_cap),
             "ode_euler_replay": loop_of(ode(model, sde, clean, "euler", args), model, e_cap),
             "pc_langevin_replay": loop_of(pc(model, sde, clean, args.seed, "langevin"), model, e_cap)}
    rows, host, edges = alternate(args, loops)

    doc = {"workload": f"probability-flow ODE (Heun, Euler; grid of {args.ode_steps} steps) beside reverse diffusion (Euler-Maruyama + "
                       "Langevin, first steps of N=1000, seeded) on config_diffusion_CA as shipped, built with pair_criterion(); "
                       "synth_protein; capped replays, every repetition from x_T",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
           "ode_steps": args.ode_steps, "nodes": int(clean["CA"].shape[0]), "edges_first_list": loops["ode_heun_replay"].first_edges,
           "e_cap": e_cap, "steps": args.steps, "reps": args.reps,
           "model_calls_per_step": {"ode_heun_replay": 2, "ode_euler_replay": 1, "pc_langevin_replay": 2},
           "sample_quality": "not assessed: untrained weights; only the time of a step is measured"}
    for name, loop in loops.items():
        doc[f"{name}_ms_per_step"] = mmm(rows[name])
        doc[f"{name}_host_busy_ms_per_step"] = mmm(host[name])
        doc[f"{name}_edges_last_list"] = edges[name]
        doc[f"{name}_recaptures"] = loop.step.recaptures
    pc_ms = statistics.median(rows["pc_langevin_replay"])
    doc["ode_heun_step_over_pc_step_median"] = round(statistics.median(rows["ode_heun_replay"]) / pc_ms, 4)
    doc["ode_euler_step_over_pc_step_median"] = round(statistics.median(rows["ode_euler_replay"]) / pc_ms, 4)
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out or os.path.join(ROOT, "profiles", "protein_sampler_ode.json"), "w") as f:
        f.write(text + "\n")


def protein_likelihood(args, model, sde, clean):
    """The likelihood's replayed step and the ODE sampler's replayed Heun step, alternating, each repetition from the same state."""
    from e3_layers_amd.run.likelihood import likelihood_plan

    grid_checked(args)
    name = f"likelihood_{args.likelihood}_replay"
    ode_heun = ode(model, sde, clean, "heun", args)
    e_cap = capacity(capacity(first_edges(model, ode_heun), args.slack), 1.1)
    # (the batch whose likelihood is taken: the ODE loop's x_T, so that both loops walk lists of one size)
    plan, acc, _ = likelihood_plan(sde, args.likelihood, model, ode_heun.batch, n_steps=args.ode_steps, seed=args.seed)
    lik = loop_of(plan, model, e_cap, frozen=True)      # (the capture records the backward: what it walks is decided here)
    if args.trace_steps:
        run_of(lik, args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
                          "likelihood": args.likelihood, "ode_steps": args.ode_steps}))
        return
    loops = {name: lik, "ode_heun_replay": loop_of(ode_heun, model, e_cap)}
    rows, host, edges = alternate(args, loops)
    finite = bool(torch.isfinite(acc).all()) and bool((acc != 0).all())

    calls = 2 if args.likelihood == "heun" else 1
    doc = {"workload": f"log-likelihood through the probability-flow ODE ({args.likelihood}; grid of {args.ode_steps} steps, one Rademacher "
                       "probe) beside the ODE sampler's Heun step on config_diffusion_CA as shipped, built with pair_criterion(); "
                       "synth_protein; capped replays, every repetition from the same state (the ODE loop's x_T, so that both loops "
                       "walk lists of one size)",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
           "ode_steps": args.ode_steps, "nodes": int(clean["CA"].shape[0]), "edges_first_list": lik.first_edges, "e_cap": e_cap,
           "steps": args.steps, "reps": args.reps,
           "model_calls_per_step": {name: f"{calls} (each a forward and one backward with respect to the positions)", "ode_heun_replay": 2},
           "logp": "not reported: untrained weights, the value says nothing about a model; the closed forms of "
                   "tests/test_likelihood_host.py pin that the number is a log-density",
           "delta_logp_finite_and_nonzero": finite}
    for k, loop in loops.items():
        doc[f"{k}_ms_per_step"] = mmm(rows[k])
        doc[f"{k}_host_busy_ms_per_step"] = mmm(host[k])
        doc[f"{k}_edges_last_list"] = edges[k]
        doc[f"{k}_recaptures"] = loop.step.recaptures
    ode_ms = statistics.median(rows["ode_heun_replay"])
    doc["likelihood_step_over_ode_heun_step_median"] = round(statistics.median(rows[name]) / ode_ms, 4)
    doc["likelihood_model_call_over_ode_model_call_median"] = round((statistics.median(rows[name]) / calls) / (ode_ms / 2), 4)
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out or os.path.join(ROOT, "profiles", "protein_likelihood.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if "--launches" in argv:
        a, na, b, nb = argv[argv.index("--launches") + 1:][:4]
        print(json.dumps({"launches_per_replayed_reverse_step": (total_calls(b) - total_calls(a)) / (int(nb) - int(na)),
                          "steps": [int(na), int(nb)]}))
    elif "--protein" in argv:
        protein(argv)
    else:
        molecules(argv)
