#!/usr/bin/env python3
"""The replayed training step fed from a dataset in HBM (``data/device_store.py``, ``run/graph_step.CollatedStep``) against the
replayed step on batches padded ahead of time (what ``bench.py --launch fixed`` times), in one process, in alternating blocks.

    (A) ``PipelinedBucketedStep`` over four batches padded once on the host and kept in HBM, used in turn (bench.py's line)
    (B) ``CollatedStep`` drawing shuffled batches of a ``DeviceDataset`` (a synthetic QM9 store of ``--store`` molecules), each
        batch collated on the device from its graph ids inside the preparation graph

Both arms pad to the same capacity (the loader's first-epoch bucket) and train the same model with the same optimizer.  Per arm:
ms per step from HIP events around each block (median and min over blocks), host busy ms per step (median wall time of one
step issued onto an idle device), buckets, recaptures, padding fraction.  One JSON line per configuration.

    python tools/device_loader_bench.py                          # config_energy (256), config_energy_force (64), config_diffusion (128)
    python tools/device_loader_bench.py --config energy --arms B --blocks 2      (the collating arm alone: rocprofv3 --kernel-trace)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "equivariant-nn-zoo_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch

BATCH = {"energy": 256, "energy_force": 64, "diffusion": 128}


def run_config(kind: str, args, dev) -> dict:
    from e3_layers_amd.backend import ops
    from e3_layers_amd.configs import config_diffusion, config_energy, config_energy_force
    from e3_layers_amd.data.device_store import DeviceDataset, DeviceLoader
    from e3_layers_amd.data.synthetic import synth_qm9, synth_qm9_diffusion
    from e3_layers_amd.run.graph_step import CollatedStep, PipelinedBucketedStep, pad_batch
    from e3_layers_amd.run.optim import FusedAdamEMA
    from e3_layers_amd.run.parallel import backward_parameters, flat_param_order, param_names
    from e3_layers_amd.run.sde_utils import VPSDE, sde_loss
    from e3_layers_amd.utils import build

    bs = args.batch or BATCH[kind]
    t0 = time.perf_counter()
    if kind == "energy":
        cfg = config_energy.get_config(l_max=2)
        store = synth_qm9(1000, args.store, config_energy.QM9_SHIFTS)
        opt_kw = dict(ema_decay=cfg.ema_decay if cfg.use_ema else None, ema_use_num_updates=cfg.ema_use_num_updates)
    elif kind == "energy_force":
        cfg = config_energy_force.get_config()
        store = synth_qm9(2000, args.store, config_energy_force.SHIFTS, r_max=5.0)
        store["forces_target"] = torch.randn(store["pos"].shape, generator=torch.Generator().manual_seed(5))
        store.attrs["forces_target"] = ("node", "1x1o")
        opt_kw = {}
    else:
        cfg = config_diffusion.get_config()
        store = synth_qm9_diffusion(1, args.store)
        opt_kw = dict(max_grad_norm=1.0)
    store_s = time.perf_counter() - t0
    torch.manual_seed(0)
    model = build(cfg.model_config).to(dev)
    order = flat_param_order(model)
    opt = FusedAdamEMA(order, lr=cfg.learning_rate, names=param_names(model, order), **opt_kw)
    flat = opt.grads
    flat.enable_direct_accumulation()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    sde = VPSDE({"pos": 3}) if kind == "diffusion" else None
    gens = (gen,) if kind == "diffusion" else ()
    prep = (lambda b: model.prepare_data(b, exclude=("pos",))) if kind == "diffusion" else model.prepare_data

    def train_on(batch):      # bench.py's replayed step (gradients_of + finish)
        if kind == "diffusion":
            loss, _ = sde_loss(sde, model, batch, generator=gen, node_weight=batch["_node_weight"])
            flat.zero()
            backward_parameters(loss, opt.params)
        else:
            target, weight = batch["total_energy"], batch["_graph_weight"]
            if kind == "energy":
                loss = ops.sq_error(model(batch)["total_energy"], target, weight, 1e3)
                flat.zero()
                loss.backward(gradient=ops.unit_gradient(loss))
            else:
                out = model(batch)
                loss = (ops.sq_error(out["energy"], target, weight, 1e3)
                        + ops.sq_error(out["forces"], batch["forces_target"], batch["_node_weight"], 3e4 / 3.0))
                flat.zero()
                backward_parameters(loss, opt.params)
        flat.all_reduce_mean()
        opt.step()
        return loss

    t0 = time.perf_counter()
    ds = DeviceDataset(store, dev)
    upload_s = time.perf_counter() - t0
    loader = DeviceLoader(ds, bs, shuffle=True, seed=0, epochs=None)
    n_cap, e_cap = loader.buckets[0]
    arms = {}
    if "A" in args.arms:      # four batches of the first epoch, padded once to the loader's bucket and kept in HBM
        first = [i for i, _ in zip(loader.id_batches(), range(4))]
        padded = [pad_batch(store.index_select(i), n_cap, e_cap).to(dev) for i in first]
        step_a = PipelinedBucketedStep(prep, train_on, padded[0], warmup=3, generators=gens)
        turn = [0]

        def run_a():
            k = turn[0]
            turn[0] += 1
            return step_a(padded[k % 4], nxt=padded[(k + 1) % 4])

        arms["A"] = (run_a, step_a)
    if "B" in args.arms:
        step_b = CollatedStep(loader, prep, train_on, warmup=3, generators=gens)
        arms["B"] = (step_b, step_b)
    main = torch.cuda.current_stream(dev)
    for run, _ in arms.values():      # warm-up steps outside the timed blocks
        for _ in range(args.warmup):
            run()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in arms}
    host = {k: [] for k in arms}
    for _ in range(args.blocks):
        for name, (run, _) in arms.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            ev0.record(main)
            for _ in range(args.block):
                run()
            ev1.record(main)
            ev1.synchronize()
            ms[name].append(ev0.elapsed_time(ev1) / args.block)
    for name, (run, _) in arms.items():      # host busy: one step issued onto an idle device (nothing it waits for is pending)
        for _ in range(24):
            torch.cuda.synchronize(dev)
            h0 = time.perf_counter()
            run()
            host[name].append((time.perf_counter() - h0) * 1e3)
    ops.join_side_streams()
    torch.cuda.synchronize(dev)
    out = {"config": kind, "molecules_per_step": bs, "store_molecules": args.store, "capacity": [n_cap, e_cap],
           "steps_per_arm": args.blocks * args.block, "block": args.block, "store_build_s": round(store_s, 2),
           "upload_s": round(upload_s, 3)}
    for name, (_, obj) in arms.items():
        out[name] = {"ms_per_step_median": round(statistics.median(ms[name]), 4), "ms_per_step_min": round(min(ms[name]), 4),
                     "ms_per_block": [round(v, 4) for v in ms[name]],
                     "host_busy_ms_per_step_median": round(statistics.median(host[name]), 4),
                     "recaptures": obj.recaptures}
    if "B" in arms:
        pn, pe = loader.padding_fraction
        out["B"].update({"buckets_recorded": arms["B"][1].n_buckets, "buckets_opened": loader.n_buckets,
                         "padding_fraction_nodes": round(float(pn), 4), "padding_fraction_edges": round(float(pe), 4)})
    if "A" in arms and "B" in arms:
        out["B_over_A"] = round(out["B"]["ms_per_step_median"] / out["A"]["ms_per_step_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=["energy", "energy_force", "diffusion", "all"], default="all")
    ap.add_argument("--store", type=int, default=16384, help="molecules in the synthetic store (default 16384)")
    ap.add_argument("--batch", type=int, default=None, help="molecules per step (default: 256 / 64 / 128 by config)")
    ap.add_argument("--arms", default="AB", help="A: pre-padded HBM batches, B: device collation (default AB)")
    ap.add_argument("--blocks", type=int, default=8, help="timed blocks per arm (alternating)")
    ap.add_argument("--block", type=int, default=32, help="steps per block")
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps per arm first")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_loader_bench.py needs a GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    kinds = ["energy", "energy_force", "diffusion"] if args.config == "all" else [args.config]
    for kind in kinds:
        print(json.dumps(run_config(kind, args, dev)), flush=True)


if __name__ == "__main__":
    main()
