"""Device collation (``data/device_store.py``, ``csrc/e3k_collate.hip``) and the step it feeds (``run/graph_step.CollatedStep``):
a batch built on the device from its graph ids is ``pad_batch(store.index_select(ids), n_cap, e_cap)`` bit for bit, eagerly and
replayed; bad ids and batches that do not fit reach the persistent flag; training through ``CollatedStep`` follows
``PipelinedBucketedStep`` fed the host-padded batches."""
import copy

import numpy as np
import pytest
import torch

from tests.util import rel_err

pytestmark = pytest.mark.gpu


def _energy_model(dev, n_dim=64, layers=3):
    from e3_layers_amd.configs.layer_configs import addEnergyOutput, featureModel
    from e3_layers_amd.utils import build

    torch.manual_seed(4)
    tree = addEnergyOutput(featureModel(n_dim=n_dim, l_max=2, edge_spherical="1x0e+1x1o+1x2e", node_attrs="20x0e", edge_radial="8x0e",
                                        num_types=10, num_layers=layers, r_max=4.0), None)
    return build(tree).to(dev).train()


def _padded(store, ids, n_cap, e_cap, dev):
    from e3_layers_amd.run.graph_step import pad_batch

    return pad_batch(store.index_select([int(i) for i in ids]), n_cap, e_cap).to(dev)


def _assert_same(got, want, keys=None):
    keys = list(want.keys()) if keys is None else keys
    assert [k for k in got.keys() if k in keys] == keys
    for k in keys:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a, b), k


def _sizes(store, ids):
    n = int(store["_n_nodes"].reshape(-1)[list(ids)].sum())
    e = int(store["_n_edges"].reshape(-1)[list(ids)].sum())
    return n, e


def _first_without_edges():
    """A diffusion store (bond_type per edge, t per graph) whose graph 0 has no edges."""
    from e3_layers_amd.data.data import Batch
    from e3_layers_amd.data.loader import samples_of
    from e3_layers_amd.data.synthetic import synth_qm9_diffusion

    d = synth_qm9_diffusion(5, 6)
    samples = [s.data for s in samples_of(d)]
    samples[0]["edge_index"] = torch.zeros(2, 0, dtype=torch.long)
    samples[0]["bond_type"] = torch.zeros(0, 1, dtype=torch.long)
    samples[0]["_n_edges"] = torch.zeros(1, 1, dtype=torch.long)
    return Batch.from_data_list(samples, dict(d.attrs))


def test_eager_collation_equals_pad_batch(dev):
    from e3_layers_amd.backend.graph import check_indices
    from e3_layers_amd.configs import config_energy
    from e3_layers_amd.data.device_store import DeviceDataset
    from e3_layers_amd.data.synthetic import synth_qm9, synth_qm9_diffusion
    from e3_layers_amd.run.graph_step import bucket_capacity

    qm9 = synth_qm9(3, 600, config_energy.QM9_SHIFTS)
    forces = synth_qm9(4, 80)
    forces["forces"] = torch.randn(forces["pos"].shape, generator=torch.Generator().manual_seed(0))
    forces.attrs["forces"] = ("node", "1x1o")
    diffusion = synth_qm9_diffusion(6, 60)
    no_edges = _first_without_edges()
    perm = torch.randperm(600, generator=torch.Generator().manual_seed(1)).tolist()
    cases = [(qm9, perm[:256], None), (qm9, perm[256:512], None), (forces, list(range(40, 72)), None),
             (diffusion, [7, 3, 59, 0, 12, 33], None), (qm9, [3, 3, 7, 3, 599, 3], None),
             (qm9, perm[:64], "tight"), (no_edges, [0, 4, 1, 5], None), (no_edges, [0], "tight")]
    stores = {}
    for store, ids, mode in cases:
        ds = stores.get(id(store))
        if ds is None:
            ds = stores[id(store)] = DeviceDataset(store, dev)
        n, e = _sizes(store, ids)
        n_cap, e_cap = (n + 2, e) if mode == "tight" else bucket_capacity([(n, e)])
        got = ds.collate(ids, n_cap, e_cap)
        want = _padded(store, ids, n_cap, e_cap, dev)
        _assert_same(got, want)
        assert {k: tuple(v) for k, v in got.attrs.items()} == {k: tuple(v) for k, v in want.attrs.items()}
        if mode == "tight":
            assert int(got["_n_nodes"][-1]) == 2 and int(got["_n_edges"][-1]) == 0
    check_indices()      # (no flag raised by any of them)


def test_replayed_collation_equals_eager_collation(dev):
    from e3_layers_amd.data.device_store import DeviceDataset
    from e3_layers_amd.data.synthetic import synth_qm9_diffusion
    from e3_layers_amd.run.graph_step import bucket_capacity

    store = synth_qm9_diffusion(8, 90)
    ds = DeviceDataset(store, dev)
    rng = np.random.default_rng(3)
    draws = [rng.choice(90, 16, replace=False) for _ in range(4)]
    n_cap, e_cap = bucket_capacity([_sizes(store, d) for d in draws])
    c = ds.collation(16, n_cap, e_cap)
    c.ids.copy_(torch.from_numpy(draws[0].astype(np.int32)))
    c()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c()
    for d in draws[1:] + draws[:1]:
        c.ids.copy_(torch.from_numpy(d.astype(np.int32)))
        g.replay()
        torch.cuda.synchronize()
        _assert_same(c.batch, ds.collate(d, n_cap, e_cap))
        _assert_same(c.batch, _padded(store, d, n_cap, e_cap, dev))


def test_bad_ids_and_batches_that_do_not_fit_are_reported(dev):
    """Rejection of bad input through the persistent flag (an id outside the store, a batch larger than its bucket): the batch is
    collated as empty graphs plus a ghost that fills the bucket -- nothing read through the id, nothing written past a capacity --
    and the next check raises, once."""
    from e3_layers_amd.backend.graph import check_indices, poll_capture_flags
    from e3_layers_amd.data.device_store import DeviceDataset
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import bucket_capacity

    store = synth_qm9(9, 40)
    ds = DeviceDataset(store, dev)
    before = {k: t.clone() for k, (_, t) in ds.fields.items()}
    ids = [1, 2, 3, 4]
    n, e = _sizes(store, ids)
    n_cap, e_cap = bucket_capacity([(n, e)])
    for bad_ids, caps in (([1, 2, 40, 4], (n_cap, e_cap)), ([1, -1, 3, 4], (n_cap, e_cap)), (ids, (n + 1, e_cap)),
                          (ids, (n_cap, e - 1))):
        got = ds.collate(bad_ids, *caps)
        with pytest.raises(ValueError, match="collated batch"):
            check_indices()
        assert got["_n_nodes"].reshape(-1).tolist() == [0] * 4 + [caps[0]]
        assert got["_n_edges"].reshape(-1).tolist() == [0] * 4 + [caps[1]]
        assert int(got["edge_index"].min()) >= 0 and int(got["edge_index"].max()) < caps[0]
        assert torch.equal(got["_node_segment"], torch.full((caps[0],), 4, dtype=torch.long, device=dev))
    check_indices()                                           # reported once: a later check is clean
    _assert_same(ds.collate(ids, n_cap, e_cap), _padded(store, ids, n_cap, e_cap, dev))
    check_indices()

    c = ds.collation(4, n_cap, e_cap)                         # ... and through a replay
    c.ids.copy_(torch.tensor(ids, dtype=torch.int32))
    c()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c()
    c.ids.copy_(torch.tensor([5, 6, 1000, 7], dtype=torch.int32))
    g.replay()
    poll_capture_flags(dev)
    with pytest.raises(ValueError, match="collated batch"):
        check_indices()
    c.ids.copy_(torch.tensor(ids, dtype=torch.int32))
    g.replay()
    poll_capture_flags(dev)
    check_indices()
    _assert_same(c.batch, _padded(store, ids, n_cap, e_cap, dev))
    for k, t in before.items():
        assert torch.equal(ds.fields[k][1], t), k             # (the store is read, never written)


def test_collated_step_follows_the_pipelined_step_on_host_padded_batches(dev):
    """Eight optimizer steps through ``CollatedStep`` (batches collated on the device from their ids) against the same eight
    through ``PipelinedBucketedStep`` fed ``pad_batch`` of the same ids, from the same initial weights: losses, parameter updates,
    EMA; the static batch of every step is the host-padded batch bit for bit."""
    from e3_layers_amd.backend import ops
    from e3_layers_amd.data.device_store import DeviceDataset, DeviceLoader
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import CollatedStep, PipelinedBucketedStep
    from e3_layers_amd.run.optim import FusedAdamEMA
    from e3_layers_amd.run.parallel import flat_param_order

    base = _energy_model(dev)
    store = synth_qm9(31, 400)
    ds = DeviceDataset(store, dev)
    n_steps = 8
    ids = [np.asarray(b) for b, _ in zip(DeviceLoader(ds, 48, seed=2).id_batches(), range(n_steps))]      # (the first epoch)
    first = DeviceLoader(ds, 48, seed=2)
    n_cap, e_cap = first.buckets[0]
    padded = [_padded(store, i, n_cap, e_cap, dev) for i in ids]
    keys = list(padded[0].keys())

    def trajectory(collated: bool):
        model = copy.deepcopy(base)
        opt = FusedAdamEMA(flat_param_order(model), lr=1e-3, ema_decay=0.99)
        opt.grads.enable_direct_accumulation()
        try:
            start = opt.flat.detach().clone()
            state0 = {k: getattr(opt, k).detach().clone() for k in ("exp_avg", "exp_avg_sq", "ema", "state")}

            def train_on(batch):
                target, weight = batch["total_energy"], batch["_graph_weight"]
                loss = ops.sq_error(model(batch)["total_energy"], target, weight, 1e3)
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss

            if collated:
                step = CollatedStep(DeviceLoader(ds, 48, seed=2), model.prepare_data, train_on, warmup=2)
            else:
                step = PipelinedBucketedStep(model.prepare_data, train_on, padded[0], warmup=2)
            with torch.no_grad():      # (the warm-ups and the captures took optimizer steps: rewind)
                opt.flat.copy_(start)
                for k, v in state0.items():
                    getattr(opt, k).copy_(v)
            losses = []
            for i in range(n_steps):
                if collated:
                    losses.append(float(step().detach()))
                    torch.cuda.synchronize()
                    _assert_same(step.last_static, padded[i], keys)
                else:
                    losses.append(float(step(padded[i], nxt=padded[i + 1] if i + 1 < n_steps else None).detach()))
            ops.join_side_streams()
            torch.cuda.synchronize()
            if collated:
                assert step.n_buckets == 1 and step.recaptures == 0
            return losses, opt.flat.detach().clone(), opt.ema.detach().clone(), start
        finally:
            opt.grads.disable_direct_accumulation()

    l_c, flat_c, ema_c, start = trajectory(True)
    l_p, flat_p, ema_p, _ = trajectory(False)
    for a, b in zip(l_c, l_p):
        assert abs(a - b) <= 2e-5 * abs(b), (l_c, l_p)
    assert rel_err(flat_c - start, flat_p - start) < 2e-3
    assert rel_err(ema_c, ema_p) < 1e-6


def test_one_epoch_collates_every_id_once(dev):
    from e3_layers_amd.data.device_store import DeviceDataset, DeviceLoader
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import CollatedStep

    store = synth_qm9(12, 64)
    ds = DeviceDataset(store, dev)
    loader = DeviceLoader(ds, 16, shuffle=True, seed=9, epochs=1)
    step = CollatedStep(loader, prepare=lambda b: None, fn=lambda b: b["total_energy"].reshape(-1) * 1.0, warmup=1)
    energy = store["total_energy"].reshape(-1).to(dev)
    seen = []
    for ids in loader.id_batches():
        got = step().clone()
        torch.cuda.synchronize()
        assert torch.equal(got[:16], energy[torch.tensor(ids, device=dev)]) and float(got[16]) == 0.0
        seen += ids
    with pytest.raises(StopIteration):
        step()
    assert sorted(seen) == list(range(64))


def test_collated_step_records_itself_again_after_a_guard_trips(dev, monkeypatch):
    """As ``test_pipelined_step_records_itself_again_after_a_guard_trips``: a tripped guard refines the knot tables; both buffers'
    preparation graphs (collation included) and steps record themselves again, and the replayed losses equal the eager model's on
    the host-padded batches afterwards."""
    import warnings

    from e3_layers_amd.backend import ops, radial_table
    from e3_layers_amd.data.device_store import DeviceDataset, DeviceLoader
    from e3_layers_amd.data.synthetic import synth_qm9
    from e3_layers_amd.run.graph_step import CollatedStep

    every = 2
    monkeypatch.setattr(radial_table, "GUARD_EVERY", every)
    knots0 = radial_table.KNOTS
    model = _energy_model(dev)
    store = synth_qm9(61, 3 * 128)
    ds = DeviceDataset(store, dev)
    loader = DeviceLoader(ds, 128, shuffle=False, epochs=None)      # batches 0, 1, 2, 0, 1, 2, ...
    n_cap, e_cap = loader.buckets[0]
    assert e_cap >= radial_table.MIN_EDGES_PER_KNOT * (2 * knots0 + 1)
    padded = [_padded(store, range(128 * k, 128 * (k + 1)), n_cap, e_cap, dev) for k in range(3)]

    def loss_on(batch):
        target, weight = batch["total_energy"], batch["_graph_weight"]
        loss = ops.sq_error(model(batch)["total_energy"], target, weight, 1e3)
        for p in model.parameters():
            p.grad = None
        loss.backward()
        return loss

    step = CollatedStep(loader, model.prepare_data, loss_on, warmup=2)
    i = 0
    for _ in range(4):
        step()
        i += 1
    torch.cuda.synchronize()
    assert step.recaptures == 0 and radial_table.REFINEMENTS == 0
    first = list(model.layer1.conv.fc.children())[0].weight
    key = radial_table.last_weight(model.layer1.conv.fc)
    scale = 1.0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        while step.recaptures == 0 and scale < 40.0:
            with torch.no_grad():
                first.mul_(1.25)
            scale *= 1.25
            for _ in range(2 * every + 2):
                step()
                i += 1
                torch.cuda.synchronize()
    assert radial_table.REFINEMENTS == 1 and radial_table.KNOTS == 2 * knots0 and radial_table.guard_ok(key), \
        (scale, [str(w.message)[:160] for w in caught])
    losses = []
    for _ in range(7):
        losses.append((i % 3, float(step().detach())))
        i += 1
        torch.cuda.synchronize()
    assert step.recaptures == 2 and step.n_buckets == 1
    (buffers,) = step._buffers.values()
    for b in range(2):
        assert set(radial_table.prepared_bins(buffers.static[b]["edge_length"])) == {radial_table.KNOTS}
    ops.join_side_streams()
    want = [float(loss_on(padded[k].clone()).detach()) for k in range(3)]
    for k, got in losses:
        assert abs(got - want[k]) <= 2e-5 * abs(want[k]), (k, got, want, losses)
