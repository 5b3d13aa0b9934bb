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
import argparse, csv, json, os, statistics, sys, time
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
    from e3_layers_amd.run.sde_utils import VPSDE, prior_sampling
    from e3_layers_amd.utils import build

    crit = config_diffusion_CA.pair_criterion()
    torch.manual_seed(0)
    model = build(config_diffusion_CA.get_config(edge_criteria=crit).model_config).to(dev).eval()
    sde = VPSDE({"CA": 3}, N=1000)
    sde.alphas = sde.alphas.to(dev)
    clean = synth_protein(1, n_prot, n_res=n_res).to(dev)
    batch = prior_sampling(sde, clean.clone(), torch.Generator(device=dev).manual_seed(1))      # x_T: where the sampler starts
    timesteps = torch.linspace(sde.T, 1e-3, sde.N, device=dev)
    return model, sde, batch, timesteps, crit, clean


def predictor(model, sde):
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor
    from e3_layers_amd.run.sde_utils import get_score_fn

    return EulerMaruyamaPredictor(sde, get_score_fn(sde, model, train=False))


def eager_loop(model, sde, batch, timesteps, crit, n_steps):
    """pc_sampler's eager path with NoneCorrector: set the time, predictor update (one model call: its edge layer builds the list,
    all pairs -> criterion -> edge count read back), drop the per-edge keys."""
    from e3_layers_amd.run.sde_sampling import SAMPLER_EDGE_KEYS

    pred = predictor(model, sde)
    state = {"b": batch.clone()}
    state["b"]["t"] = torch.empty(len(batch), 1, device=timesteps.device)
    crit.reset()

    def loop():
        b = state["b"]
        t_dev = b["t"]
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(n_steps):
                t_dev.copy_(timesteps[i].expand_as(t_dev))
                b = pred.update_fn(b)
                for k in SAMPLER_EDGE_KEYS:
                    b.pop(k)
        state["b"] = b
        return time.perf_counter() - t0

    return loop


def replay_loop(model, sde, batch, timesteps, slack):
    """The capped loop of get_pc_sampler(graph=True, edge_capacity=...): sized, padded and captured here, outside the timed region."""
    from e3_layers_amd.run.capped import builder_cells, edge_layer_of
    from e3_layers_amd.run.sde_sampling import CappedLoop

    b = batch.clone()
    b.attrs["t"] = ("graph", "1x0e")
    pred = predictor(model, sde)
    probe = b.clone()
    probe.data["_nlist_rng"] = builder_cells(timesteps.device)
    new, _ = edge_layer_of(model).layer(probe.data, probe.attrs)
    e_cap = -(-int(slack * new["edge_index"].shape[1]) // 1024) * 1024
    with torch.no_grad():
        return CappedLoop(b, model, [lambda w: w, lambda w: pred.update_fn(w)], ["CA"], float(timesteps[0]), e_cap, None), e_cap


def seeded_updates(model, sde, seed, cells, corrector, fixed=None):
    """[corrector, predictor] of the seeded form, as get_pc_sampler builds them (``fixed``: the mask field's name, or None)"""
    from functools import partial

    from e3_layers_amd.run.sde_utils import langevin_step_counter, reverse_step_counter

    corr = (partial(langevin_step_counter, sde, model, seed=seed, draw=cells, snr=0.16, fixed=fixed) if corrector == "langevin"
            else (lambda w: w))
    return [corr, partial(reverse_step_counter, sde, model, seed=seed, draw=cells, fixed=fixed)]


def seeded_replay_loop(model, sde, batch, timesteps, e_cap, seed, corrector, fixed=None):
    from e3_layers_amd.run.sde_sampling import CappedLoop

    b = batch.clone()
    b.attrs["t"] = ("graph", "1x0e")
    cells = torch.zeros(2, dtype=torch.int64, device=timesteps.device)
    extra = {} if fixed is None else {"fixed": fixed}      # (the unconditioned call: as before)
    with torch.no_grad():
        return CappedLoop(b, model, seeded_updates(model, sde, seed, cells, corrector, fixed), ["CA"], float(timesteps[0]), e_cap, None,
                          seeded=(timesteps, cells), **extra)


def ode_replay_loop(model, sde, batch, method, n_steps, e_cap):
    """The capped loop of get_ode_sampler(graph=True, edge_capacity=...), built as it builds it: the updates are the ODE's stages, the
    step header walks the first n_steps entries of the table."""
    from functools import partial

    from e3_layers_amd.run.sde_sampling import CappedLoop
    from e3_layers_amd.run.sde_utils import ode_euler_step, ode_heun_finish

    dev = batch["CA"].device
    b = batch.clone()
    b.attrs["t"] = ("graph", "1x0e")
    times = torch.linspace(sde.T, 1e-3, n_steps + 1, device=dev, dtype=torch.float32)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    if method == "euler":
        updates = [partial(ode_euler_step, sde, model, times=times, cells_or_step=cells)]
    else:
        kept = {}
        updates = [partial(ode_euler_step, sde, model, times=times, cells_or_step=cells, keep=kept),
                   partial(ode_heun_finish, sde, model, kept=kept, times=times, cells_or_step=cells)]
    with torch.no_grad():
        return CappedLoop(b, model, updates, ["CA"], float(times[0]), e_cap, None, seeded=(times[:n_steps], cells))


def likelihood_replay_loop(model, sde, batch, method, n_steps, e_cap, seed):
    """The capped loop of get_likelihood_fn(graph=True, edge_capacity=...), built as it builds it: the probes ride in the batch, the
    table ascends, the accumulators go back to zero with the cells.  -> (loop, acc)"""
    from e3_layers_amd.backend import ops
    from e3_layers_amd.run.likelihood import attach_probes, frozen_parameters, stage_updates
    from e3_layers_amd.run.sde_sampling import CappedLoop

    dev = batch["CA"].device
    b = batch.clone()
    b.attrs["t"] = ("graph", "1x0e")
    attach_probes(sde, b, seed, "rademacher", 1)
    times = torch.linspace(1e-3, sde.T, n_steps + 1, device=dev, dtype=torch.float32)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    acc = torch.zeros(len(b), dtype=torch.float64, device=dev)
    row_ptr = ops.graph_row_pointers(b["_n_nodes"].reshape(-1).contiguous())
    updates = stage_updates(sde, model, method, times, cells, acc, 1, row_ptr)
    with torch.no_grad(), frozen_parameters(model):      # (the capture records the backward: what it walks is decided here)
        return CappedLoop(b, model, updates, ["CA"], float(times[0]), e_cap, None, seeded=(times[:n_steps], cells), zero=(acc,)), acc


def conditioned(sde, batch, clean, fraction):
    """``batch`` (at x_T = z) with conditional sampling's fields, as get_pc_sampler(fixed="fixed") sets them up: the middle ``fraction``
    of every chain of every protein is fixed (a contiguous stretch, chosen by the chain's length alone), ``known_CA`` = the clean
    coordinates, and the fixed rows of x_T are m(T) x0 + s(T) z.  -> (batch, fixed rows)"""
    b = batch.clone()
    chain = clean["chain_id"].reshape(-1) + (int(clean["chain_id"].max()) + 1) * clean.nodeSegment()
    mask = torch.zeros_like(chain, dtype=torch.bool)
    for c in torch.unique(chain).tolist():
        rows = torch.nonzero(chain == c).reshape(-1)
        k = int(round(fraction * rows.numel()))
        start = (rows.numel() - k) // 2
        mask[rows[start:start + k]] = True
    b.attrs["fixed"], b.attrs["known_CA"] = ("node", "1x0e"), b.attrs["CA"]
    b["fixed"] = mask.reshape(-1, 1).to(torch.uint8)
    b["known_CA"] = clean["CA"].float()
    lm = sde.log_mean_coeff(torch.tensor(float(sde.T)))
    b["CA"] = torch.where(mask.reshape(-1, 1), torch.exp(lm) * b["known_CA"] + torch.sqrt(-torch.expm1(2.0 * lm)) * b["CA"], b["CA"])
    return b, int(mask.sum())


def seeded_eager_loop(model, sde, batch, timesteps, crit, n_steps, seed, corrector):
    """pc_sampler's eager path with a seed: the step header, corrector, predictor; the per-edge keys dropped after each"""
    from e3_layers_amd.run.sde_sampling import SAMPLER_EDGE_KEYS
    from e3_layers_amd.run.sde_utils import sampler_begin_step

    cells = torch.zeros(2, dtype=torch.int64, device=timesteps.device)
    updates = seeded_updates(model, sde, seed, cells, corrector)
    state = {"b": batch.clone()}
    state["b"].attrs["t"] = ("graph", "1x0e")
    state["b"]["t"] = torch.empty(len(batch), 1, device=timesteps.device)
    crit.reset()

    def loop():
        b = state["b"]
        t_dev = b["t"]
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(n_steps):
                sampler_begin_step(timesteps, cells, t_dev)
                for update in updates:
                    b = update(b)
                    for k in SAMPLER_EDGE_KEYS:
                        b.pop(k)
        state["b"] = b
        return time.perf_counter() - t0

    return loop


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
    dev = torch.device("cuda:0")
    model, sde, batch, timesteps, crit, clean = protein_setup(args.proteins, args.residues, dev)
    if args.likelihood is not None:
        return protein_likelihood(args, model, sde, batch, timesteps)
    if args.ode is not None:
        return protein_ode(args, model, sde, batch, timesteps)
    if args.seed is not None:
        return protein_seeded(args, model, sde, batch, timesteps, crit, clean)
    if args.corrector != "none":
        raise SystemExit("--corrector langevin needs --seed: the unseeded replay serves NoneCorrector only")
    loop, e_cap = replay_loop(model, sde, batch, timesteps, args.slack)

    def replay(n):
        def run():
            t0 = time.perf_counter()
            with torch.no_grad():
                loop.run(timesteps, n)
            return time.perf_counter() - t0
        return run

    if args.trace_steps:
        loop.rewind()
        replay(args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues}))
        return
    loop.rewind()
    replay(args.warmup)()
    eager_loop(model, sde, batch, timesteps, crit, args.warmup)()
    rows = {"replay": [], "eager": [], "replay_host": [], "eager_host": []}
    edges = []
    for _ in range(args.reps):
        loop.rewind()
        ms, host = timed(replay(args.steps))
        edges.append(int(loop.bucket.state[0]))
        loop.result()                               # (after the closing event: an overflowed repetition would raise here)
        rows["replay"].append(ms / args.steps)
        rows["replay_host"].append(1e3 * host / args.steps)
        ms, host = timed(eager_loop(model, sde, batch, timesteps, crit, args.steps))
        rows["eager"].append(ms / args.steps)
        rows["eager_host"].append(1e3 * host / args.steps)

    def mmm(v):
        return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}

    doc = {"workload": "reverse diffusion (Euler-Maruyama, NoneCorrector, first steps of N=1000) on config_diffusion_CA as shipped, "
                       "built with pair_criterion(); synth_protein",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues,
           "nodes": int(batch["CA"].shape[0]), "edges_first_list": loop.first_edges, "edges_last_list": edges, "e_cap": e_cap,
           "n_cap": loop.bucket.n_cap, "steps": args.steps, "reps": args.reps, "recaptures": loop.step.recaptures,
           "replay_ms_per_step": mmm(rows["replay"]), "eager_ms_per_step": mmm(rows["eager"]),
           "replay_host_busy_ms_per_step": mmm(rows["replay_host"]), "eager_host_busy_ms_per_step": mmm(rows["eager_host"]),
           "speedup_median": round(statistics.median(rows["eager"]) / statistics.median(rows["replay"]), 3)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def protein_seeded(args, model, sde, batch, timesteps, crit, clean):
    """The seeded replay, the seeded eager loop and (NoneCorrector only) the unseeded replay, alternating; with ``--fixed`` the
    conditioned seeded replay as well."""
    plain, e_cap = replay_loop(model, sde, batch, timesteps, args.slack)
    if args.corrector == "langevin":      # (two model calls per step, and the corrector moves the nodes before the second list)
        e_cap = -(-int(1.1 * e_cap) // 1024) * 1024
    loop = seeded_replay_loop(model, sde, batch, timesteps, e_cap, args.seed, args.corrector)
    cond = n_fixed = None
    if args.fixed:      # (the same capacity: the fixed rows start near their clean places, the rest as before)
        cond_batch, n_fixed = conditioned(sde, batch, clean, args.fixed)
        cond = seeded_replay_loop(model, sde, cond_batch, timesteps, e_cap, args.seed, args.corrector, fixed="fixed")

    def replay(which, n):
        def run():
            t0 = time.perf_counter()
            with torch.no_grad():
                which.run(timesteps, n)
            return time.perf_counter() - t0
        return run

    if args.trace_steps:
        traced = loop if cond is None else cond
        traced.rewind()
        replay(traced, args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
                          "corrector": args.corrector, "fixed": args.fixed}))
        return
    variants = {"seeded_replay": lambda n: (loop.rewind(), replay(loop, n))[1],
                "seeded_eager": lambda n: seeded_eager_loop(model, sde, batch, timesteps, crit, n, args.seed, args.corrector)}
    if cond is not None:
        variants["fixed_replay"] = lambda n: (cond.rewind(), replay(cond, n))[1]
    if args.corrector == "none":
        variants["replay"] = lambda n: (plain.rewind(), replay(plain, n))[1]
    for make in variants.values():
        make(args.warmup)()
    rows = {name: [] for name in variants}
    host = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, make in variants.items():
            ms, busy = timed(make(args.steps))
            if name == "seeded_replay":
                loop.result()                       # (after the closing event: an overflowed repetition would raise here)
            elif name == "fixed_replay":
                cond.result()
            elif name == "replay":
                plain.result()
            rows[name].append(ms / args.steps)
            host[name].append(1e3 * busy / args.steps)

    def mmm(v):
        return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}

    doc = {"workload": f"reverse diffusion (Euler-Maruyama, corrector {args.corrector}, first steps of N=1000) on config_diffusion_CA as "
                       "shipped, built with pair_criterion(); synth_protein; seeded form",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
           "corrector": args.corrector, "nodes": int(batch["CA"].shape[0]), "edges_first_list": loop.first_edges, "e_cap": e_cap,
           "n_cap": loop.bucket.n_cap, "steps": args.steps, "reps": args.reps, "recaptures": loop.step.recaptures}
    for name in variants:
        doc[f"{name}_ms_per_step"] = mmm(rows[name])
        doc[f"{name}_host_busy_ms_per_step"] = mmm(host[name])
    if "replay" not in variants:
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


def protein_ode(args, model, sde, batch, timesteps):
    """The Heun replay, the Euler replay and the seeded Euler-Maruyama + Langevin replay, alternating, each repetition from x_T."""
    n_timed = args.trace_steps or args.steps
    if not 1 <= n_timed <= args.ode_steps or args.warmup > args.ode_steps:
        raise SystemExit(f"--steps / --trace-steps / --warmup: at most --ode-steps = {args.ode_steps} (a replay past the grid stands still)")
    _, e_cap = replay_loop(model, sde, batch, timesteps, args.slack)
    e_cap = -(-int(1.1 * e_cap) // 1024) * 1024      # (the seeded Langevin replay's capacity; the same for every loop here)
    loops = {"ode_heun_replay": ode_replay_loop(model, sde, batch, "heun", args.ode_steps, e_cap),
             "ode_euler_replay": ode_replay_loop(model, sde, batch, "euler", args.ode_steps, e_cap)}

    def replay(which, n):
        which.rewind()      # (outside the timed region)

        def run():
            t0 = time.perf_counter()
            with torch.no_grad():
                which.run(timesteps, n)
            return time.perf_counter() - t0
        return run

    if args.trace_steps:
        replay(loops[f"ode_{args.ode}_replay"], args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
                          "ode": args.ode, "ode_steps": args.ode_steps}))
        return
    loops["pc_langevin_replay"] = seeded_replay_loop(model, sde, batch, timesteps, e_cap, args.seed, "langevin")
    for loop in loops.values():
        replay(loop, args.warmup)()
    rows = {name: [] for name in loops}
    host = {name: [] for name in loops}
    edges = {name: [] for name in loops}
    for _ in range(args.reps):
        for name, loop in loops.items():
            ms, busy = timed(replay(loop, args.steps))
            edges[name].append(int(loop.bucket.state[0]))
            loop.result()                                   # (after the closing event: an overflowed repetition would raise here)
            rows[name].append(ms / args.steps)
            host[name].append(1e3 * busy / args.steps)

    def mmm(v):
        return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}

    doc = {"workload": f"probability-flow ODE (Heun, Euler; grid of {args.ode_steps} steps) beside reverse diffusion (Euler-Maruyama + "
                       "Langevin, first steps of N=1000, seeded) on config_diffusion_CA as shipped, built with pair_criterion(); "
                       "synth_protein; capped replays, every repetition from x_T",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
           "ode_steps": args.ode_steps, "nodes": int(batch["CA"].shape[0]), "e_cap": e_cap, "steps": args.steps, "reps": args.reps,
           "model_calls_per_step": {"ode_heun_replay": 2, "ode_euler_replay": 1, "pc_langevin_replay": 2},
           "sample_quality": "not assessed: untrained weights; only the time of a step is measured"}
    for name, loop in loops.items():
        doc[f"{name}_ms_per_step"] = mmm(rows[name])
        doc[f"{name}_host_busy_ms_per_step"] = mmm(host[name])
        doc[f"{name}_edges_last_list"] = edges[name]
        doc[f"{name}_recaptures"] = loop.step.recaptures
    pc = statistics.median(rows["pc_langevin_replay"])
    doc["ode_heun_step_over_pc_step_median"] = round(statistics.median(rows["ode_heun_replay"]) / pc, 4)
    doc["ode_euler_step_over_pc_step_median"] = round(statistics.median(rows["ode_euler_replay"]) / pc, 4)
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out or os.path.join(ROOT, "profiles", "protein_sampler_ode.json"), "w") as f:
        f.write(text + "\n")


def protein_likelihood(args, model, sde, batch, timesteps):
    """The likelihood's replayed step and the ODE sampler's replayed Heun step, alternating, each repetition from the same state."""
    n_timed = args.trace_steps or args.steps
    if not 1 <= n_timed <= args.ode_steps or args.warmup > args.ode_steps:
        raise SystemExit(f"--steps / --trace-steps / --warmup: at most --ode-steps = {args.ode_steps} (a replay past the grid stands still)")
    _, e_cap = replay_loop(model, sde, batch, timesteps, args.slack)
    e_cap = -(-int(1.1 * e_cap) // 1024) * 1024
    name = f"likelihood_{args.likelihood}_replay"
    lik, acc = likelihood_replay_loop(model, sde, batch, args.likelihood, args.ode_steps, e_cap, args.seed)

    def replay(which, n):
        which.rewind()      # (outside the timed region)

        def run():
            t0 = time.perf_counter()
            with torch.no_grad():
                which.run(timesteps, n)
            return time.perf_counter() - t0
        return run

    if args.trace_steps:
        replay(lik, args.trace_steps)()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
                          "likelihood": args.likelihood, "ode_steps": args.ode_steps}))
        return
    loops = {name: lik, "ode_heun_replay": ode_replay_loop(model, sde, batch, "heun", args.ode_steps, e_cap)}
    for loop in loops.values():
        replay(loop, args.warmup)()
    rows = {k: [] for k in loops}
    host = {k: [] for k in loops}
    edges = {k: [] for k in loops}
    for _ in range(args.reps):
        for k, loop in loops.items():
            ms, busy = timed(replay(loop, args.steps))
            edges[k].append(int(loop.bucket.state[0]))
            loop.result()
            rows[k].append(ms / args.steps)
            host[k].append(1e3 * busy / args.steps)
    finite = bool(torch.isfinite(acc).all()) and bool((acc != 0).all())

    def mmm(v):
        return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}

    calls = 2 if args.likelihood == "heun" else 1
    doc = {"workload": f"log-likelihood through the probability-flow ODE ({args.likelihood}; grid of {args.ode_steps} steps, one Rademacher "
                       "probe) beside the ODE sampler's Heun step on config_diffusion_CA as shipped, built with pair_criterion(); "
                       "synth_protein; capped replays, every repetition from the same state (the ODE loop's x_T, so that both loops "
                       "walk lists of one size)",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues, "seed": args.seed,
           "ode_steps": args.ode_steps, "nodes": int(batch["CA"].shape[0]), "e_cap": e_cap, "steps": args.steps, "reps": args.reps,
           "model_calls_per_step": {name: f"{calls} (each a forward and one backward with respect to the positions)", "ode_heun_replay": 2},
           "logp": "not reported: untrained weights, the value says nothing about a model; the closed forms of "
                   "tests/test_likelihood_host.py pin that the number is a log-density",
           "delta_logp_finite_and_nonzero": finite}
    for k, loop in loops.items():
        doc[f"{k}_ms_per_step"] = mmm(rows[k])
        doc[f"{k}_host_busy_ms_per_step"] = mmm(host[k])
        doc[f"{k}_edges_last_list"] = edges[k]
        doc[f"{k}_recaptures"] = loop.step.recaptures
    ode = statistics.median(rows["ode_heun_replay"])
    doc["likelihood_step_over_ode_heun_step_median"] = round(statistics.median(rows[name]) / ode, 4)
    doc["likelihood_model_call_over_ode_model_call_median"] = round((statistics.median(rows[name]) / calls) / (ode / 2), 4)
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
