"""Conditional sampling on the CPU (run/sde_sampling.get_pc_sampler(fixed=...); run/sde_utils: the ``fixed`` / ``known`` arguments of
prior_sampling_counter, langevin_step_counter, reverse_step_counter, and replace_fixed): the float64 restatement the FIXED kernels of
csrc/e3k_sampler.hip are held to, against the unseeded sampler fed the same draws.

Set-up of tests/test_sampler_seeded_host.py: float64 as torch's default dtype, its affine stub model and batches, VPSDE(N=4,
beta_max=2) (that file says why a four-step schedule needs beta_max / N < 1).  The bound of the seeded / noise-fed comparison is that
file's 1e-9: the replacement adds m(t) x0 + s(t) z on both sides, exp and sqrt of the same lm up to the float64 roundings its
docstring already counts, and it overwrites rows -- it amplifies nothing."""
import pytest
import torch

from tests.test_sampler_seeded_host import KEYS, SEED, Affine, _batch, _sde
from tests.util import rel_err


@pytest.fixture(autouse=True)
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _masked(batch, mask, dtype=torch.int64, name="fixed"):
    batch.attrs[name] = ("node", "1x0e")
    batch[name] = torch.as_tensor(mask).to(dtype)
    return batch


def _mask(n):
    m = torch.zeros(n, dtype=torch.bool)
    m[2:6] = True      # the end of the first graph and the start of the second
    m[n - 1] = True    # the last node
    return m


def _samplers(**kwargs):
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, get_pc_sampler

    pred, corr = kwargs.pop("predictor", EulerMaruyamaPredictor), kwargs.pop("corrector", LangevinCorrector)
    return get_pc_sampler(_sde(), pred, corr, static_edges=True, **kwargs)


def _draw_bank(sde, n_nodes, steps, corrector=True, predictor=True):
    """the float64 draws in the order the unseeded conditioned loop asks for them: the prior per key, then per step the corrector's
    per key, its replacement's per key (block 2), the predictor's per key (block 1), its replacement's per key (block 3)"""
    from e3_layers_amd.data.compute_edge import normal_draw
    from e3_layers_amd.run.sde_utils import draw_words

    words, total = draw_words(sde)
    node = torch.arange(n_nodes).reshape(-1, 1)

    def z(draw, block, key):
        return normal_draw(SEED, draw, node, block * total + words[key] + torch.arange(sde.irreps[key]).reshape(1, -1), torch.float64)

    bank = [z(sde.N, 0, k) for k in sde.irreps]
    for i in range(steps):
        if corrector:
            bank += [z(i, 0, k) for k in sde.irreps] + [z(i, 2, k) for k in sde.irreps]
        if predictor:
            bank += [z(i, 1, k) for k in sde.irreps] + [z(i, 3, k) for k in sde.irreps]
    return bank


def test_seeded_conditioned_sampler_equals_the_unseeded_one_fed_the_same_draws():
    batch = _batch((5, 7, 3))
    n = batch["pos"].shape[0]
    mask = _mask(n)
    _masked(batch, mask)
    x0 = {k: batch[k].clone() for k in KEYS}
    model = Affine(KEYS)
    out_s, nfe = _samplers(seed=SEED, fixed="fixed")(model, batch)
    assert nfe == 8 and model.calls == 8
    bank = iter(_draw_bank(_sde(), n, 4))
    out_p, _ = _samplers(fixed="fixed")(Affine(KEYS), batch, noise_fn=lambda shape: next(bank))
    assert next(bank, None) is None      # every draw was asked for, in this order
    for k in KEYS:
        assert out_s[k].dtype == torch.float64 and torch.isfinite(out_s[k]).all()
        err = rel_err(out_s[k], out_p[k])
        print("conditioned: seeded vs noise-fed", k, err)
        assert err < 1e-9, (k, err)
        for out in (out_s, out_p):
            assert torch.equal(out[k][mask], x0[k][mask])                    # the fixed rows are x0, bit for bit
            assert not (out[k][~mask] == x0[k][~mask]).any()                 # ... and the free rows are not
    for k in KEYS:      # the input batch is untouched, the result carries the caller's fields only
        assert torch.equal(batch[k], x0[k])
    assert out_s["fixed"].dtype == torch.int64 and torch.equal(out_s["fixed"].reshape(-1), mask.long())
    assert not [k for k in out_s if k.startswith("known_")] and not [k for k in out_p if k.startswith("known_")]
    again, _ = _samplers(seed=SEED, fixed="fixed")(Affine(KEYS), batch)
    assert all(torch.equal(again[k], out_s[k]) for k in KEYS)
    # a bool, a float and a column mask are the same mask
    for dtype in (torch.bool, torch.float32, torch.uint8):
        other, _ = _samplers(seed=SEED, fixed="fixed")(Affine(KEYS), _masked(batch.clone(), mask.reshape(-1, 1), dtype))
        assert all(torch.equal(other[k], out_s[k]) for k in KEYS)
    # the caller's own known_<key> field comes back as it was
    own = _masked(batch.clone(), mask)
    own.attrs["known_pos"] = ("node", "1x1o")
    own["known_pos"] = torch.full((n, 3), 7.0)
    kept, _ = _samplers(seed=SEED, fixed="fixed")(Affine(KEYS), own)
    assert torch.equal(kept["known_pos"], torch.full((n, 3), 7.0)) and "known_aux" not in kept
    assert all(torch.equal(kept[k], out_s[k]) for k in KEYS)


def test_an_all_zero_mask_is_the_unconditioned_sampler_and_a_mask_moves_the_free_rows():
    batch = _batch((5, 7, 3))
    n = batch["pos"].shape[0]
    plain, _ = _samplers(seed=SEED)(Affine(KEYS), batch)
    zero, _ = _samplers(seed=SEED, fixed="fixed")(Affine(KEYS), _masked(batch.clone(), torch.zeros(n)))
    for k in KEYS:
        assert torch.equal(zero[k], plain[k])
    mask = _mask(n)
    cond, _ = _samplers(seed=SEED, fixed="fixed")(Affine(KEYS), _masked(batch.clone(), mask))
    # the free rows feel the fixed ones through the corrector's batch-wide norms
    err = rel_err(cond["pos"][~mask], plain["pos"][~mask])
    print("conditioned vs unconditioned, free rows", err)
    assert err > 1e-3, err
    # the unseeded pair: the same statement with a generator
    g = lambda: torch.Generator().manual_seed(3)      # noqa: E731
    plain_u, _ = _samplers()(Affine(KEYS), batch, generator=g())
    zero_u, _ = _samplers(fixed="fixed")(Affine(KEYS), _masked(batch.clone(), torch.zeros(n)), generator=g())
    assert rel_err(zero_u["pos"], plain_u["pos"]) > 1e-3      # (the replacement draws even when it replaces nothing: other noise)
    cond_u, _ = _samplers(fixed="fixed")(Affine(KEYS), _masked(batch.clone(), mask), generator=g())
    assert torch.equal(cond_u["pos"][mask], batch["pos"][mask]) and torch.isfinite(cond_u["pos"]).all()


def test_the_replacement_blocks_draw_apart():
    sde = _sde()
    bank = _draw_bank(sde, 200, 2)
    prior, steps = bank[:2], [bank[2 + 8 * i: 10 + 8 * i] for i in range(2)]
    blocks = []
    for st in steps:      # per step: corrector (block 0), its replacement (2), predictor (1), its replacement (3), two keys each
        blocks += [st[0:2], st[2:4], st[4:6], st[6:8]]
    everything = [prior] + blocks
    for i, a in enumerate(everything):
        for b in everything[i + 1:]:
            for x, y in zip(a, b):
                assert (x != y).all()
    c0, r2, p1, r3 = blocks[:4]
    # ... and across the keys: aux's two components against pos's first two, in and between the replacement blocks
    assert (r2[1] != r2[0][:, :2]).all() and (r3[1] != r3[0][:, :2]).all() and (r2[1] != r3[0][:, :2]).all()
    assert (r2[0][:, :2] != p1[1]).all() and (r3[0][:, :2] != r2[1]).all()      # a block's first words are not the previous block's last


def test_padded_batch_real_rows_equal_the_unpadded_run_and_ghost_rows_stay():
    plain, padded = _batch((5, 7, 3)), _batch((5, 7, 3), ghost=19)
    n = plain["pos"].shape[0]
    for k in KEYS:
        padded[k][:n] = plain[k]
    ghost_rows = {k: padded[k][n:].clone() for k in KEYS}
    mask = _mask(n)
    sampler = _samplers(seed=SEED, fixed="fixed")
    a, _ = sampler(Affine(KEYS), _masked(plain, mask))
    for ghost_byte in (0, 1):
        full = torch.cat([mask.long(), torch.full((19,), ghost_byte)])
        b, _ = sampler(Affine(KEYS), _masked(padded.clone(), full))
        for k in KEYS:
            assert torch.equal(b[k][:n], a[k])                      # exactly: the ghost rows enter nothing
            assert torch.equal(b[k][n:], ghost_rows[k])             # bit for bit, whatever their mask bytes hold
            assert torch.equal(b[k][:n][mask], plain[k][mask])


def test_none_classes_call_no_model_and_take_no_replacement_draw():
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector, NoneCorrector, NonePredictor

    batch = _batch((5, 7, 3))
    n = batch["pos"].shape[0]
    mask = _mask(n)
    _masked(batch, mask)
    for pred, corr, calls in ((EulerMaruyamaPredictor, NoneCorrector, 4), (NonePredictor, LangevinCorrector, 4), (NonePredictor, NoneCorrector, 0)):
        m = Affine(KEYS)
        out_s, _ = _samplers(predictor=pred, corrector=corr, seed=SEED, fixed="fixed")(m, batch)
        assert m.calls == calls                                    # as without a mask
        bank = iter(_draw_bank(_sde(), n, 4, corrector=corr is not NoneCorrector, predictor=pred is not NonePredictor))
        m = Affine(KEYS)
        out_p, _ = _samplers(predictor=pred, corrector=corr, fixed="fixed")(m, batch, noise_fn=lambda shape: next(bank))
        assert m.calls == calls and next(bank, None) is None       # no replacement draw behind a None class
        for k in KEYS:
            assert rel_err(out_s[k], out_p[k]) < 1e-9
            assert torch.equal(out_s[k][mask], batch[k][mask]) and torch.equal(out_p[k][mask], batch[k][mask])


def test_custom_classes_are_wrapped_without_a_seed():
    from e3_layers_amd.run.sde_sampling import EulerMaruyamaPredictor, LangevinCorrector

    class MyPredictor(EulerMaruyamaPredictor):
        pass

    class MyCorrector(LangevinCorrector):
        pass

    batch = _batch((5, 7, 3))
    n = batch["pos"].shape[0]
    _masked(batch, _mask(n))
    banks = [iter(_draw_bank(_sde(), n, 4)) for _ in range(2)]
    a, _ = _samplers(fixed="fixed")(Affine(KEYS), batch, noise_fn=lambda shape: next(banks[0]))
    b, _ = _samplers(predictor=MyPredictor, corrector=MyCorrector, fixed="fixed")(Affine(KEYS), batch, noise_fn=lambda shape: next(banks[1]))
    assert next(banks[1], None) is None and all(torch.equal(a[k], b[k]) for k in KEYS)


def test_step_functions_take_the_mask_and_the_known_values_directly():
    """The three counter functions with ``fixed`` a tensor and ``known`` a dict, not batch fields -- and their defaults unchanged."""
    from e3_layers_amd.run.sde_utils import langevin_step_counter, prior_sampling_counter, reverse_step_counter

    sde = _sde()
    batch = _batch((5, 7, 3))
    n = batch["pos"].shape[0]
    mask = _mask(n)
    known = {k: batch[k].clone() for k in KEYS}

    def run(**kw):
        b = batch.clone()
        b.attrs["t"] = ("graph", "1x0e")
        b["t"] = torch.full((3, 1), 0.5)
        b = prior_sampling_counter(sde, b, SEED, **kw)
        b = langevin_step_counter(sde, Affine(KEYS), b, SEED, 1, 0.16, **kw)
        return reverse_step_counter(sde, Affine(KEYS), b, SEED, 1, **kw)

    by_tensor = run(fixed=mask, known=known)
    in_batch = batch.clone()
    _masked(in_batch, mask)
    for k in KEYS:
        in_batch.attrs[f"known_{k}"] = in_batch.attrs[k]
        in_batch[f"known_{k}"] = known[k]
    sde2 = _sde()
    b = in_batch
    b.attrs["t"] = ("graph", "1x0e")
    b["t"] = torch.full((3, 1), 0.5)
    b = prior_sampling_counter(sde2, b, SEED, fixed="fixed")
    b = langevin_step_counter(sde2, Affine(KEYS), b, SEED, 1, 0.16, fixed="fixed")
    b = reverse_step_counter(sde2, Affine(KEYS), b, SEED, 1, fixed="fixed")
    free = run()
    lm = 0.5 * (-0.25 * (2.0 - 0.1) * 0.5 - 0.5 * 0.1)
    for k in KEYS:
        assert torch.equal(b[k], by_tensor[k])
        assert not torch.equal(by_tensor[k][~mask], free[k][~mask])
        # a fixed row is m x0 + s z'' of block 3 at t = 0.5: within s * 6 of m x0, and not x0 itself
        m, s = torch.exp(torch.tensor(lm)), torch.sqrt(-torch.expm1(torch.tensor(2 * lm)))
        dev = (by_tensor[k][mask] - m * known[k][mask]).abs()
        assert (dev > 0).all() and (dev < 6 * s).all()


def test_refusals():
    batch = _batch((4, 3))
    sampler = _samplers(seed=SEED, fixed="fixed")
    with pytest.raises(ValueError, match="no field"):
        sampler(Affine(KEYS), batch.clone())
    with pytest.raises(ValueError, match="no field"):
        _samplers(fixed="fixed")(Affine(KEYS), batch.clone())
    short = batch.clone()
    short.attrs["fixed"] = ("node", "1x0e")
    short.data["fixed"] = torch.zeros(6, 1)
    with pytest.raises(ValueError, match="7 nodes"):
        sampler(Affine(KEYS), short)
    wide = batch.clone()
    wide.attrs["fixed"] = ("node", "2x0e")
    wide.data["fixed"] = torch.zeros(7, 2)
    with pytest.raises(ValueError, match="7 nodes"):
        sampler(Affine(KEYS), wide)
    graphwise = batch.clone()
    graphwise.attrs["fixed"] = ("graph", "1x0e")
    graphwise.data["fixed"] = torch.zeros(2, 1)
    with pytest.raises(ValueError, match="per-node"):
        sampler(Affine(KEYS), graphwise)
    ok = _masked(batch.clone(), torch.tensor([1, 0, 0, 0, 0, 1, 0]))
    with pytest.raises(ValueError, match="generator"):
        sampler(Affine(KEYS), ok, generator=torch.Generator())
    with pytest.raises(ValueError, match="noise_fn"):
        sampler(Affine(KEYS), ok, noise_fn=lambda shape: torch.zeros(shape))
    out, _ = sampler(Affine(KEYS), ok)
    assert torch.equal(out["pos"][0], batch["pos"][0]) and torch.equal(out["pos"][5], batch["pos"][5])
