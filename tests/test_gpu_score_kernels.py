"""The kernels of csrc/e3k_score.hip and the vetoed optimizer step of csrc/e3k_optim.hip, called through the C ABI and held to
float64 element by element.

Perturbation (e3k_vpsde_perturb).  The oracle is the float64 form of run/sde_utils.sde_perturb_counter on the CPU.  u = 2^-24 is
half an fp32 ulp, relative.
  * The hashes are integers: u_g is exact, and t = fma(T - eps, u_g, eps) rounds once: |t - t64| <= u t64, with T - eps and eps the
    floats the kernel receives.
  * lm = t (q t + h) is one FMA and one product: the rounded t moves it by |2 q t + h| u t, the two roundings by 2 u |lm|: DLM.
  * a = expf(lm): a DLM + 2 u ULP_EXP a.   m = -expm1f(2 lm): 2 exp(2 lm) DLM + 2 u ULP_EXPM1 m.   s = sqrtf(m), correctly rounded:
    DS = Dm / (2 s) + u s.
  * z is within XI_BOUND (tests/test_gpu_md_integrator_kernels.py: the same draw, the same functions).
  * x_t = fma(a, x0, s z): Da |x0| + (DS + u s) (|z| + XI_BOUND) + s XI_BOUND + u |x_t|.
  ULP_EXP and ULP_EXPM1 are not constants of this file: they are measured through torch on the device on the case's own t grid (every
  lm the kernel forms, for the three plantings of t), as test_device_logf_is_within_ulp_log measures logf; the measurement must stay
  within OpenCL full profile's 3 ulp, and the bound uses the integer above it.
  t is planted through the kernel's own parameters: eps = T = 1e-5 puts every graph at t = eps (where 1 - exp(2 lm) would keep
  three digits), eps = T = 1 at t = 1, and (1e-5, 1) inside.

Denoising loss (e3k_denoise_loss): the running error analysis of tests/test_gpu_node_matrix.py (EV: a float64 value and a bound on
|fp32 result - value|, every operation adding its own rounding), as tests/test_gpu_train_matrix.py derives sq_reference's bounds: the
gradient elementwise, the loss as a sum in any order.  Rows of weight 0 get gradient exactly 0.

Vetoed step: bit comparisons only."""
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_edge_matrix import _worst_ulp
from tests.test_gpu_md_integrator_kernels import XI_BOUND
from tests.test_gpu_node_matrix import EV, sum_ev
from tests.util import record_measured

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
f32, f64 = np.float32, np.float64
SEED = (977 << 32) + 20241017      # both seed words in use
BETA_0, BETA_1 = 0.1, 20.0
CANARY = -7.25
PLANTED = {"inside": (1e-5, 1.0), "at_eps": (1e-5, 1e-5), "at_one": (1.0, 1.0)}      # (eps, T)
# (N real, G, D, ghost nodes, word0s)
PERTURB_CASES = [(1, 1, 3, 0, (0,)), (63, 2, 3, 0, (0,)), (65, 3, 3, 0, (0,)), (257, 4, 1, 0, (0,)), (110, 2, 3, 19, (0,)),
                 (65, 3, 3, 0, (0, 3))]


def _lib():
    from e3_layers_amd.backend import lib as L

    return L, L.load()


def _sizes(n, g, rng):
    cuts = np.sort(rng.choice(np.arange(1, n), g - 1, replace=False)) if g > 1 else np.array([], dtype=np.int64)
    return tuple(int(v) for v in np.diff(np.concatenate([[0], cuts, [n]])))


def _planted_sde(T, keys):
    from e3_layers_amd.run.sde_utils import VPSDE

    class Planted(VPSDE):
        T = property(lambda self: T)

    return Planted(keys, beta_min=BETA_0, beta_max=BETA_1)


def _perturb_batch(n, g, d, ghost, n_keys, rng):
    from e3_layers_amd.data import Batch

    sizes = _sizes(n, g, rng) + ((ghost,) if ghost else ())
    names = [f"k{j}" for j in range(n_keys)]
    attrs = {k: ("node", "1x1o" if d == 3 else f"{d}x0e") for k in names}
    lst = [dict({k: torch.from_numpy(rng.standard_normal((m, d)).astype(f32)) for k in names}, _n_nodes=torch.tensor([[m]])) for m in sizes]
    b = Batch.from_data_list(lst, attrs)
    if ghost:
        b["_graph_weight"] = torch.tensor([[1.0 / g]] * g + [[0.0]])
    return b, names


def _call_perturb(dev, x0, seg, n_graphs, eps, T, draw, word0):
    """e3k_vpsde_perturb on canaried output buffers -> (t [G + 1], x_t, z, std) as numpy, canaries checked"""
    L, lib = _lib()
    n, d = x0.shape
    xd, sd = x0.to(dev).contiguous(), seg.to(dev).contiguous()
    cell = torch.tensor([draw, 12345], dtype=torch.int64, device=dev)
    outs = [torch.full((size + 2,), CANARY, device=dev) for size in (n_graphs + 1, n * d, n * d, n)]
    rc = lib.e3k_vpsde_perturb(L.ptr(xd), L.ptr(sd), n, d, n_graphs, BETA_0, BETA_1, eps, T, SEED & 0xFFFFFFFF, SEED >> 32, L.ptr(cell),
                               word0, *(o.data_ptr() + 4 for o in outs), L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert cell.tolist() == [draw, 12345]      # read, not written
    got = []
    for o in outs:
        o = o.cpu().numpy()
        assert o[0] == f32(CANARY) and o[-1] == f32(CANARY)
        got.append(o[1:-1])
    return got[0], got[1].reshape(n, d), got[2].reshape(n, d), got[3]


def _lm32(t32):
    """the kernel's lm from its own t: one FMA (a float64 product and sum, rounded once), one product"""
    q, h = f32(-0.25) * (f32(BETA_1) - f32(BETA_0)), f32(-0.5) * f32(BETA_0)
    inner = (f64(q) * t32.astype(f64) + f64(h)).astype(f32)
    return (t32 * inner).astype(f32)


def _measure_exp_ulps(dev, t_grid):
    lm = _lm32(np.unique(t_grid.astype(f32)))
    two = (f32(2.0) * lm).astype(f32)
    exp_ulp = _worst_ulp(torch.exp(torch.from_numpy(lm).to(dev)).cpu().numpy(), np.exp(lm.astype(f64)))
    m1_ulp = _worst_ulp(torch.expm1(torch.from_numpy(two).to(dev)).cpu().numpy(), np.expm1(two.astype(f64)))
    return exp_ulp, m1_ulp


@pytest.mark.parametrize("planted", list(PLANTED))
@pytest.mark.parametrize("case", PERTURB_CASES, ids=lambda c: "N%d_G%d_D%d_ghost%d_keys%d" % (c[0], c[1], c[2], c[3], len(c[4])))
def test_perturb_against_the_float64_restatement(dev, case, planted):
    from e3_layers_amd.data.compute_edge import pair_hash
    from e3_layers_amd.run.sde_utils import sde_perturb_counter

    n, g, d, ghost, word0s = case
    eps, T = PLANTED[planted]
    rng = np.random.default_rng(1000 * n + 10 * g + d)
    batch, names = _perturb_batch(n, g, d, ghost, len(word0s), rng)
    seg = batch.nodeSegment()
    sde = _planted_sde(T, {k: d for k in names})
    draw = 41
    want, misc = sde_perturb_counter(sde, batch, SEED, draw, eps, dtype=torch.float64)
    # ---- t: the hashes are integers, u is exact; one rounding of the final multiply-add
    u = (pair_hash(SEED, draw, 0xFFFFFFFF, torch.arange(g)).numpy() >> 8).astype(f64) * 2.0 ** -24
    t64 = float(f32(eps)) + float(f32(T) - f32(eps)) * u
    assert np.array_equal(want["t"].numpy()[:g, 0], t64)
    if planted == "at_eps":
        assert (t64 == float(f32(1e-5))).all()
    if planted == "at_one":
        assert (t64 == 1.0).all()
    # ---- the device's exponentials on this case's grid: measured, asserted, used
    exp_ulp, m1_ulp = _measure_exp_ulps(dev, t64)
    print(f"device math library on the t grid of {planted}: expf {exp_ulp:.3f} ulp, expm1f {m1_ulp:.3f} ulp")
    record_measured("test_gpu_score_kernels", case=f"exp_{planted}_G{g}", expf_ulp=exp_ulp, expm1f_ulp=m1_ulp)
    assert exp_ulp <= 3 and m1_ulp <= 3, (exp_ulp, m1_ulp)      # (3: the OpenCL full-profile limit of both)
    ULP_EXP, ULP_EXPM1 = max(1, math.ceil(exp_ulp)), max(1, math.ceil(m1_ulp))
    q, h = float(f32(-0.25) * (f32(BETA_1) - f32(BETA_0))), float(f32(-0.5) * f32(BETA_0))
    lm = t64 * (q * t64 + h)
    a, m = np.exp(lm), -np.expm1(2.0 * lm)
    s = np.sqrt(m)
    dlm = np.abs(2.0 * q * t64 + h) * U * t64 + 2.0 * U * np.abs(lm)
    da = a * dlm + 2.0 * U * ULP_EXP * a
    dm = 2.0 * np.exp(2.0 * lm) * dlm + 2.0 * U * ULP_EXPM1 * m
    ds = dm / (2.0 * s) + U * s
    node_g = seg.numpy()[:n]
    worst = {}
    first_t = None
    for key, word0 in zip(names, word0s):
        x0 = batch[key]
        t, x_t, z, std = _call_perturb(dev, x0, seg, g, eps, T, draw, word0)
        assert (np.abs(t[:g].astype(f64) - t64) <= U * t64).all(), (t[:g], t64)
        assert t[g] == f32(0.5)
        if first_t is None:
            first_t = t
        assert np.array_equal(t, first_t)      # every key's call files the same t
        z64, x64, s64 = misc["zs"][key].numpy(), want[key].numpy(), misc["std"].numpy()[:, 0]
        assert np.array_equal(s64[:n], s[node_g])
        ez = np.abs(z[:n].astype(f64) - z64[:n])
        assert (ez <= XI_BOUND).all(), ez.max()
        es = np.abs(std[:n].astype(f64) - s64[:n])
        assert (es <= ds[node_g]).all(), (es / ds[node_g]).max()
        x0_64 = x0.numpy()[:n].astype(f64)
        bound = (da[node_g][:, None] * np.abs(x0_64) + (ds[node_g] + U * s[node_g])[:, None] * (np.abs(z64[:n]) + XI_BOUND)
                 + s[node_g][:, None] * XI_BOUND + U * np.abs(x64[:n]))
        ex = np.abs(x_t[:n].astype(f64) - x64[:n])
        assert (ex <= bound).all(), (ex / bound).max()
        worst[key] = (float(ez.max() / XI_BOUND), float((es / ds[node_g]).max()), float((ex / bound).max()))
        if ghost:      # bit for bit
            assert np.array_equal(x_t[n:].view(np.int32), x0.numpy()[n:].view(np.int32))
            assert not z[n:].view(np.int32).any() and (std[n:] == f32(1.0)).all()
        # the same (seed, draw) again: the same bits; draw + 1: every z differs
        t2, x2, z2, std2 = _call_perturb(dev, x0, seg, g, eps, T, draw, word0)
        assert all(np.array_equal(p.view(np.int32), r.view(np.int32)) for p, r in ((t, t2), (x_t, x2), (z, z2), (std, std2)))
        _, _, z3, _ = _call_perturb(dev, x0, seg, g, eps, T, draw + 1, word0)
        assert (z3[:n] != z[:n]).all()
    if len(word0s) == 2:      # the second key draws other words: its noise is not the first key's
        za = _call_perturb(dev, batch[names[0]], seg, g, eps, T, draw, 0)[2]
        zb = _call_perturb(dev, batch[names[0]], seg, g, eps, T, draw, 3)[2]
        assert (za != zb).all()
    print("perturb", case, planted, {k: tuple(round(v, 3) for v in w) for k, w in worst.items()}, "(z, std, x_t: worst error / bound)")
    record_measured("test_gpu_score_kernels", case=f"perturb_N{n}_G{g}_D{d}_{planted}", worst_x=max(w[2] for w in worst.values()))


def test_perturb_refuses_bad_arguments(dev):
    L, lib = _lib()
    x = torch.zeros(4, 3, device=dev)
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    cell = torch.zeros(1, dtype=torch.int64, device=dev)
    t, std = torch.zeros(2, device=dev), torch.zeros(4, device=dev)
    ok = dict(x0=L.ptr(x), seg=L.ptr(seg), N=4, D=3, G=1, b0=0.1, b1=20.0, eps=1e-5, T=1.0, draw=L.ptr(cell), t=L.ptr(t))

    def call(**over):
        a = dict(ok, **over)
        return lib.e3k_vpsde_perturb(a["x0"], a["seg"], a["N"], a["D"], a["G"], a["b0"], a["b1"], a["eps"], a["T"], 1, 2, a["draw"], 0, a["t"],
                                     L.ptr(torch.empty_like(x)), L.ptr(torch.empty_like(x)), L.ptr(std), L.stream_ptr())

    assert call() == 0
    for bad in (dict(D=0), dict(G=-1), dict(eps=2.0), dict(draw=None), dict(t=None), dict(x0=None), dict(b1=0.05), dict(N=-1)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
def _denoise_inputs(n, d, weights, rng):
    raw = rng.standard_normal((n, d)).astype(f32)
    x_t = rng.standard_normal((n, d)).astype(f32)
    z = rng.standard_normal((n, d)).astype(f32)
    std = (10.0 ** rng.uniform(-3, 0, n)).astype(f32)
    std[0] = f32(1e-3)
    w = None
    if weights == "uniform":
        w = np.full(n, f32(1.0) / f32(n), f32)
    elif weights == "zero_rows":
        w = rng.uniform(0.0, 2.0 / n, n).astype(f32)
        w[::3] = 0.0      # ghost rows of a padded batch
    return raw, x_t, z, std, w


def denoise_reference(raw, x_t, z, std, w):
    """(grad, loss) as (value, bound) pairs: err = (z - raw) - std x_t, wi = w_i (1 / D), grad = (-2 wi) err, loss = sum (wi err) err"""
    n, d = raw.shape
    wi = EV(np.full(n, float(f32(1.0) / f32(n))) if w is None else w.astype(f64)) * EV(float(f32(1.0) / f32(d)))
    err = (EV(z.astype(f64)) - EV(raw.astype(f64))) - EV(std.astype(f64)[:, None]) * EV(x_t.astype(f64))
    wi = EV(wi.v[:, None], wi.e[:, None])
    grad = (EV(-2.0) * wi) * err
    terms = (wi * err) * err
    loss = sum_ev(EV(terms.v.reshape(-1), terms.e.reshape(-1)), 0)
    return grad.pair(), loss.pair()


@pytest.mark.parametrize("weights", ["null", "uniform", "zero_rows"])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025])
def test_denoise_loss_against_float64(dev, n, d, weights):
    L, lib = _lib()
    rng = np.random.default_rng(7 * n + d)
    raw, x_t, z, std, w = _denoise_inputs(n, d, weights, rng)
    dt = [torch.from_numpy(v).to(dev) if v is not None else None for v in (raw, x_t, z, std, w)]
    loss = torch.full((3,), CANARY, device=dev)
    grad = torch.full((n * d + 2,), CANARY, device=dev)
    rc = lib.e3k_denoise_loss(*(L.ptr(v) for v in dt), n, d, loss.data_ptr() + 4, grad.data_ptr() + 4, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    assert loss[0] == loss[2] == f32(CANARY) and grad[0] == grad[-1] == f32(CANARY)
    (g64, gb), (l64, lb) = denoise_reference(raw, x_t, z, std, w)
    eg = np.abs(grad[1:-1].reshape(n, d).astype(f64) - g64)
    assert (eg <= gb).all(), (eg / np.where(gb > 0, gb, 1.0)).max()
    assert abs(float(loss[1]) - float(l64)) <= float(lb), (loss[1], l64, lb)
    if w is not None:
        assert not grad[1:-1].reshape(n, d)[w == 0].any()      # weight 0: gradient exactly 0
    plain = ((w if w is not None else np.full(n, 1.0 / n))[:, None] * ((-raw.astype(f64) - std.astype(f64)[:, None] * x_t + z) ** 2) / d).sum()
    assert abs(l64 - plain) <= 1e-6 * abs(plain) + 1e-12      # (the reference is the formula of the issue)
    # the same launch again: the same bits (one workgroup, fixed summation order)
    loss2, grad2 = torch.zeros(1, device=dev), torch.zeros(n * d, device=dev)
    assert lib.e3k_denoise_loss(*(L.ptr(v) for v in dt), n, d, L.ptr(loss2), L.ptr(grad2), L.stream_ptr()) == 0
    assert np.array_equal(loss2.cpu().numpy().view(np.int32), loss[1:2].view(np.int32))
    assert np.array_equal(grad2.cpu().numpy().view(np.int32), grad[1:-1].view(np.int32))
    print(f"denoise_loss N{n} D{d} {weights}: gradient worst error / bound {float((eg / np.where(gb > 0, gb, 1.0)).max()):.3f}, "
          f"loss {abs(float(loss[1]) - float(l64)) / float(lb):.3f}")


def test_denoise_loss_autograd_function(dev):
    from e3_layers_amd.backend import ops

    g = torch.Generator().manual_seed(5)
    raw = torch.randn(70, 3, generator=g).to(dev).requires_grad_(True)
    x_t, z = torch.randn(70, 3, generator=g).to(dev), torch.randn(70, 3, generator=g).to(dev)
    std = (0.1 + torch.rand(70, 1, generator=g)).to(dev)
    w = torch.rand(70, 1, generator=g).to(dev)
    w[::4] = 0
    loss = ops.denoise_loss(raw, x_t, z, std, w)
    (3.0 * loss).backward()
    r64 = raw.detach().double().requires_grad_(True)
    want = (w.double().reshape(-1) * ((-r64 - std.double() * x_t.double() + z.double()) ** 2).mean(-1)).sum()
    (3.0 * want).backward()
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    assert float((raw.grad.double() - r64.grad).abs().max()) <= 1e-5 * float(r64.grad.abs().max())
    with pytest.raises(RuntimeError):
        ops.denoise_loss(raw.detach().cpu(), x_t.cpu(), z.cpu(), std.cpu(), None)      # no CPU fallback


# ---------------------------------------------------------------------------------------------------------------------------------
HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, decay=0.999, use_num=1)


def _adam_buffers(dev, n, ema, seed):
    g = torch.Generator().manual_seed(seed)
    b = dict(p=torch.randn(n, generator=g), m=0.1 * torch.randn(n, generator=g), v=0.01 * torch.rand(n, generator=g))
    b["ema"] = torch.randn(n, generator=g) if ema else None
    b["state"] = torch.zeros(16)
    return {k: (t.to(dev).contiguous() if t is not None else None) for k, t in b.items()}


def _adam_call(dev, b, grad, clip, skip, veto=None):
    L, lib = _lib()
    args = (L.ptr(b["p"]), L.ptr(grad), L.ptr(b["m"]), L.ptr(b["v"]), L.ptr(b["ema"]), b["p"].numel(), HP["lr"], HP["b1"], HP["b2"], HP["eps"],
            HP["wd"], HP["decay"], HP["use_num"], clip, skip, L.ptr(b["state"]))
    rc = lib.e3k_adam_ema_step(*args, L.stream_ptr()) if veto is None else lib.e3k_adam_ema_step_vetoed(*args, L.ptr(veto), L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()


def _bits(b):
    return {k: t.clone().view(torch.int32) for k, t in b.items() if t is not None}


def _same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


@pytest.mark.parametrize("ema,clip,skip,nonfinite", [(False, 0.0, 0, False), (True, 0.0, 0, False), (True, 1.0, 0, False), (False, 0.5, 1, False),
                                                     (True, 0.0, 1, True), (True, 1.0, 1, False)])
@pytest.mark.parametrize("n", [1, 5, 7, 1027])
def test_vetoed_step_bits(dev, n, ema, clip, skip, nonfinite):
    gen = torch.Generator().manual_seed(100 + n)
    grads = [(3.0 * torch.randn(n, generator=gen)).to(dev) for _ in range(3)]
    if nonfinite:
        grads[2][n // 2] = float("inf")

    def fresh():
        b = _adam_buffers(dev, n, ema, 9 * n)
        for k in range(2):      # two plain steps first: the state block is in mid-run
            _adam_call(dev, b, grads[k], clip, skip)
        return b

    zero, three = torch.zeros(2, dtype=torch.int64, device=dev), torch.tensor([3, 0], dtype=torch.int64, device=dev)
    plain = fresh()
    before = _bits(plain)
    _adam_call(dev, plain, grads[2], clip, skip)
    plain = _bits(plain)
    # veto = 0: the bits of e3k_adam_ema_step, in every buffer and every state word
    open_ = fresh()
    assert _same(_bits(open_), before)
    _adam_call(dev, open_, grads[2], clip, skip, veto=zero)
    assert _same(_bits(open_), plain)
    if not nonfinite:
        assert not _same(plain, before, ("p",))      # (the step does move the weights)
    # veto = 3: nothing moves, neither counter advances
    held = fresh()
    _adam_call(dev, held, grads[2], clip, skip, veto=three)
    after = _bits(held)
    assert _same(after, before, [k for k in ("p", "m", "v", "ema") if k in before])
    st, st0 = held["state"].cpu(), before["state"].view(torch.float32).cpu()
    assert st[0] == st0[0] == 2.0 and st[8] == st0[8] and float(st[8]) == (2.0 if ema else 0.0)
    assert float(st[5]) == 0.0 and float(st[6]) == 1.0
    if ema:
        assert float(st[9]) == 1.0      # the effective EMA decay of the vetoed launch
    assert three.tolist() == [3, 0]      # read, not written
    # the veto cleared: the following step == a step taken from the pre-veto state, bit for bit
    _adam_call(dev, held, grads[2], clip, skip, veto=zero)
    assert _same(_bits(held), plain)
    # ... and two vetoed launches in a row change nothing either
    twice = fresh()
    _adam_call(dev, twice, grads[2], clip, skip, veto=three)
    _adam_call(dev, twice, grads[1], clip, skip, veto=three)
    _adam_call(dev, twice, grads[2], clip, skip, veto=zero)
    assert _same(_bits(twice), plain)


def test_vetoed_step_refuses_a_null_cell(dev):
    L, lib = _lib()
    b = _adam_buffers(dev, 8, True, 1)
    g = torch.zeros(8, device=dev)
    rc = lib.e3k_adam_ema_step_vetoed(L.ptr(b["p"]), L.ptr(g), L.ptr(b["m"]), L.ptr(b["v"]), L.ptr(b["ema"]), 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.999,
                                      1, 0.0, 0, L.ptr(b["state"]), None, L.stream_ptr())
    assert rc != 0


def test_fused_optimizer_takes_the_veto(dev):
    from e3_layers_amd.run.optim import FusedAdamEMA

    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(37, device=dev))
    opt = FusedAdamEMA([p], lr=1e-2, ema_decay=0.999, max_grad_norm=1.0)
    cell = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    start = opt.flat.clone()
    opt.grads.buffer.normal_()
    opt.step(veto=cell[1:])
    assert torch.equal(opt.flat, start) and opt.steps_taken == 0 and opt.ema_updates == 0
    opt.step(veto=cell[:1])
    assert not torch.equal(opt.flat, start) and opt.steps_taken == 1 and opt.ema_updates == 1
    with pytest.raises(ValueError):
        opt.step(veto=torch.zeros(1, device=dev))


# ---------------------------------------------------------------------------------------------------------------------------------
def test_step_record(dev):
    L, lib = _lib()
    W = 4
    cells = torch.tensor([0, -1], dtype=torch.int64, device=dev)
    over = torch.zeros(1, dtype=torch.int64, device=dev)
    ring = torch.full((W + 2,), CANARY, device=dev)
    loss = torch.zeros(1, device=dev)
    for s in range(6):
        loss.fill_(10.0 + s)
        if s == 3:
            over.fill_(1)      # the builder's counter goes up at step 3 and stays
        if s == 5:
            over.fill_(2)
        assert lib.e3k_score_step_record(L.ptr(loss), L.ptr(over), L.ptr(cells), ring.data_ptr() + 4, W, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [6, 3]                                   # six steps; the FIRST overflowed one is remembered
    assert ring.tolist() == [CANARY, 14.0, 15.0, 12.0, 13.0, CANARY]     # ring[s % W]
    assert over.tolist() == [2]
    assert lib.e3k_score_step_record(L.ptr(loss), L.ptr(over), L.ptr(cells), L.ptr(ring), 0, L.stream_ptr()) != 0
