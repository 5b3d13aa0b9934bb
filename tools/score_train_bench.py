#!/usr/bin/env python3
"""The protein score net's training step: one replayed HIP graph per step on a capped neighbour list (run/score_step.py) against
the same steps taken eagerly (eager_score_step) on the same batches with the same draws.

Workload: config_diffusion_CA as shipped but built with the declarative pair criterion (``get_config(edge_criteria=pair_criterion())``),
4 x 384 synth_protein residues, Adam + EMA with max_grad_norm 1.0; the edge capacity is ``capacity_for(batches, 0.99)``.

    python tools/score_train_bench.py --out profiles/score_train_replay.json

Protocol (tools/md_bench.py's): device events around ``--steps`` steps after a warm-up, the two variants alternating in one process,
``--reps`` repetitions each (min / median / max); host-busy time is the wall time of the enqueue loop before the closing
synchronisation (the replayed loop's includes its window checks, which wait for the device, and whatever it redoes eagerly;
``replay_enqueue`` is the part spent issuing the replays).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/score_train_bench.py --trace-steps 40
  Nothing is asserted: the numbers are
quoted in README.md and DESIGN.md."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "equivariant-nn-zoo_amd")):
    sys.path.insert(0, p)
import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    host = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def main(argv):
    from e3_layers_amd.configs import config_diffusion_CA
    from e3_layers_amd.data.synthetic import synth_protein
    from e3_layers_amd.run.optim import FusedAdamEMA
    from e3_layers_amd.run.parallel import flat_param_order, param_names
    from e3_layers_amd.run.score_step import ReplayedScoreStep, edge_capacity_for
    from e3_layers_amd.run.sde_utils import VPSDE
    from e3_layers_amd.utils import build

    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=4)
    ap.add_argument("--residues", type=int, default=384)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0, help="run this many replayed steps and nothing else (under rocprofv3)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    cfg = config_diffusion_CA.get_config(edge_criteria=config_diffusion_CA.pair_criterion())
    torch.manual_seed(0)
    model = build(cfg.model_config).to(dev)
    order = flat_param_order(model)
    opt = FusedAdamEMA(order, lr=cfg.learning_rate, names=param_names(model, order), max_grad_norm=1.0, ema_decay=0.999)
    opt.grads.enable_direct_accumulation()
    sde = VPSDE({"CA": 3})
    host = [synth_protein(1 + 17 * k, args.proteins, n_res=args.residues) for k in range(args.batches)]
    resident = [b.to(dev) for b in host]
    e_cap = edge_capacity_for(model, sde, resident, args.quantile)      # (eager list builds at eight counter draws per batch)
    step = ReplayedScoreStep(model, sde, opt, resident[0], edge_capacity=e_cap, check_every=args.check_every)
    padded = [step.pad(b) for b in resident]
    counter = [0]
    enqueue = [0.0]      # host time inside the replayed step's own calls (copies + graph launch), without the window checks' waits
    issue = step.replay

    def timed_issue(batch):
        t0 = time.perf_counter()
        issue(batch)
        enqueue[0] += time.perf_counter() - t0

    step.replay = timed_issue
    if args.trace_steps:
        for _ in range(args.trace_steps):
            step(padded[counter[0] % len(padded)])
            counter[0] += 1
        step.flush()
        torch.cuda.synchronize()
        print(json.dumps({"trace_steps": args.trace_steps, "e_cap": step.e_cap, "n_cap": step.n_cap, "stats": step.stats}))
        return

    def replay(n):
        def run():
            t0 = time.perf_counter()
            for _ in range(n):
                step(padded[counter[0] % len(padded)])
                counter[0] += 1
            step.flush()
            return time.perf_counter() - t0
        return run

    def eager(n, first):
        def run():
            t0 = time.perf_counter()
            for s in range(first, first + n):
                step.eager_step(resident[s % len(resident)], s)
            return time.perf_counter() - t0
        return run

    replay(args.warmup)()
    eager(args.warmup, 0)()
    rows = {"replay": [], "eager": [], "replay_host": [], "eager_host": [], "replay_enqueue": []}
    ghost_share, before = [], dict(step.stats)
    for _ in range(args.reps):
        first = counter[0]      # the eager repetition takes the draws the replayed one just took
        enqueue[0] = 0.0
        ms, h = timed(replay(args.steps))
        rows["replay"].append(ms / args.steps)
        rows["replay_enqueue"].append(1e3 * enqueue[0] / args.steps)
        rows["replay_host"].append(1e3 * h / args.steps)
        ghost_share.append(1.0 - int(step.nlist_state[0]) / step.e_cap)
        ms, h = timed(eager(args.steps, first))
        rows["eager"].append(ms / args.steps)
        rows["eager_host"].append(1e3 * h / args.steps)
    stats = step.stats
    timed_steps = stats["steps"] - before["steps"]
    sizes = [e for b in resident for e in step.list_sizes(b, range(8))]

    def mmm(v):
        return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}

    doc = {"workload": "training step (VP-SDE denoising loss, Adam + EMA, max_grad_norm 1.0) of config_diffusion_CA as shipped, built with "
                       "pair_criterion(); synth_protein",
           "device": torch.cuda.get_device_name(0), "proteins": args.proteins, "residues": args.residues, "batches": args.batches,
           "nodes": int(resident[0]["CA"].shape[0]), "e_cap": step.e_cap, "n_cap": step.n_cap, "capacity_quantile": args.quantile,
           "eager_list_sizes_8_draws": {"min": min(sizes), "median": int(statistics.median(sizes)), "max": max(sizes)},
           "mean_ghost_edge_share": round(1.0 - statistics.mean(sizes) / step.e_cap, 4),
           "ghost_edge_share_last_list_of_each_repetition": [round(v, 4) for v in ghost_share],
           "steps": args.steps, "reps": args.reps, "check_every": args.check_every,
           "replay_ms_per_step": mmm(rows["replay"]), "eager_ms_per_step": mmm(rows["eager"]),
           "replay_host_busy_ms_per_step": mmm(rows["replay_host"]), "eager_host_busy_ms_per_step": mmm(rows["eager_host"]),
           "replay_enqueue_ms_per_step": mmm(rows["replay_enqueue"]),
           "speedup_median": round(statistics.median(rows["eager"]) / statistics.median(rows["replay"]), 3),
           "share_of_steps_redone": round((stats["steps_redone"] - before["steps_redone"]) / max(timed_steps, 1), 4),
           "stats": stats}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
