"""The seeded sampler's kernels (csrc/e3k_sampler.hip: e3k_sampler_begin_step, e3k_sampler_langevin, e3k_sampler_reverse_em) called
through the C ABI on canaried buffers and held to float64, element by element.

The reference is the float64 form of the header's formulas on the floats the kernel receives, carried through the running error
analysis of tests/test_gpu_node_matrix.py (EV: a float64 value and a bound on |fp32 result - value|; every operation adds its own
rounding, so a product and a sum the compiler contracts into one FMA stay inside the bound of the two):
  * t is planted, exact.  lm = t fma(q, t, h): one FMA, one product.
  * m = -expm1f(2 lm): exp(2 lm) 2 D(lm) + 2 u ULP_EXPM1 m, with ULP_EXPM1 the device's expm1f measured through torch on the case's own
    t grid (tests/test_gpu_score_kernels.py's measurement; it must stay within OpenCL full profile's 3 ulp), s = sqrtf(m).
  * z is within XI_BOUND of normal_draw(..., float64) (tests/test_gpu_md_integrator_kernels.py: the same draw, the same functions).
  * the row norms are dot products and the two means sums of N terms in ANY order (dot_ev, sum_ev): the kernel's order is fixed but
    not part of its contract.  Phase 2 reads the kernel's own means: their bound travels on through the step size.
  * the table index k = (int64)((t (n_alpha - 1)) / T) is restated in numpy fp32, the same two operations: with n_alpha = 5 and T = 1 the
    plantings k / 4 and the float just below it must land on k and k - 1.
Ghost rows (segment G: outside [0, G)) are compared bit for bit."""
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_md_integrator_kernels import XI_BOUND
from tests.test_gpu_node_matrix import EV, dot_ev, fma, sum_ev
from tests.test_gpu_score_kernels import _measure_exp_ulps
from tests.util import record_measured

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
f32, f64 = np.float32, np.float64
SEED = (977 << 32) + 20241019      # both seed words in use
BETA_0, BETA_1 = 0.1, 20.0         # (the betas tests/test_gpu_score_kernels.py measures the exponentials at)
CANARY = -7.25
N_ALPHA, T_END, SNR, STEP = 5, 1.0, 0.16, 2


def _below(v):
    return float(np.nextafter(f32(v), f32(0.0)))


# per graph, in turn: both ends of the schedule, and every knot of the alphas table with the float just below it
PLANTED_T = [1e-3, 1.0, 0.25, _below(0.25), 0.5, _below(0.5), 0.75, _below(0.75)]
PLANTED_K = [0, 4, 1, 0, 2, 1, 3, 2]


def _lib():
    from e3_layers_amd.backend import lib as L

    return L, L.load()


def _case(n, d, ghost, g, rng, first_t=0):
    """x, raw [n + ghost, d] fp32, seg (ghost rows: segment g), t [g + 1] fp32 (the ghost graph's slot last), alphas [N_ALPHA]"""
    if n > g:
        cuts = np.sort(rng.choice(np.arange(1, n), g - 1, replace=False)) if g > 1 else np.array([], dtype=np.int64)
        sizes = np.diff(np.concatenate([[0], cuts, [n]]))
    else:
        sizes = np.array([n] + [0] * (g - 1))
    seg = np.concatenate([np.repeat(np.arange(g), sizes), np.full(ghost, g)]).astype(np.int64)
    x = rng.standard_normal((n + ghost, d)).astype(f32)
    raw = rng.standard_normal((n + ghost, d)).astype(f32)
    t = np.array([PLANTED_T[(first_t + j) % len(PLANTED_T)] for j in range(g)] + [0.5], dtype=f32)
    alphas = (1.0 - np.linspace(0.02, 0.6, N_ALPHA)).astype(f32)
    return x, raw, seg, t, alphas


def _std_ev(t32, ulp_expm1):
    """s(t) per graph as an EV, and the kernel's q, h"""
    dbeta = f32(BETA_1) - f32(BETA_0)
    q, h = f32(-0.25) * dbeta, f32(-0.5) * f32(BETA_0)
    t = EV(t32.astype(f64))
    lm = t * fma(float(q), t, float(h))
    m = -np.expm1(2.0 * lm.v)
    dm = 2.0 * np.exp(2.0 * lm.v) * lm.e + 2.0 * U * ulp_expm1 * m
    return EV(m, dm).sqrt(), float(dbeta)


def _draws(n, d, step, word0):
    from e3_layers_amd.data.compute_edge import normal_draw

    z = normal_draw(SEED, step, torch.arange(n).reshape(-1, 1), word0 + torch.arange(d).reshape(1, -1), torch.float64)
    return EV(z.numpy(), XI_BOUND)


def _rows(ev, seg):
    return EV(ev.v[seg][:, None], ev.e[seg][:, None])


def _expm1_ulp(dev, t32, tag):
    exp_ulp, m1_ulp = _measure_exp_ulps(dev, t32.astype(f64))
    assert exp_ulp <= 3 and m1_ulp <= 3, (exp_ulp, m1_ulp)      # (3: the OpenCL full-profile limit of both)
    return max(1, math.ceil(m1_ulp))


def langevin_reference(x, raw, seg, t32, alphas, n, word0, ulp):
    """((x' value, bound) over the real rows, (norms value, bound)) -- header formulas, EV arithmetic"""
    s_g, _ = _std_ev(t32, ulp)
    sg = seg[:n]
    s = _rows(s_g, sg)
    xr = EV(x[:n].astype(f64))
    score = -(EV(raw[:n].astype(f64)) / s) - xr
    z = _draws(n, x.shape[1], STEP, word0)
    gn, zn = dot_ev(score, score, 1).sqrt(), dot_ev(z, z, 1).sqrt()
    mean_g, mean_z = sum_ev(gn, 0) / EV(float(n)), sum_ev(zn, 0) / EV(float(n))
    ratio = (EV(float(f32(SNR))) * mean_z) / mean_g
    base = (ratio * ratio) * EV(2.0)
    tn = t32[sg]
    k = ((tn * f32(N_ALPHA - 1)).astype(f32) / f32(T_END)).astype(f32).astype(np.int64).clip(0, N_ALPHA - 1)
    step = base * EV(alphas.astype(f64)[k][:, None])
    amp = (step * EV(2.0)).sqrt()
    out = (xr + step * score) + amp * z
    norms = (np.array([mean_g.v, mean_z.v]), np.array([mean_g.e, mean_z.e]))
    return out.pair(), norms, k


def _call_langevin(dev, x, raw, seg, t, alphas, g, word0, alias):
    L, lib = _lib()
    n_all, d = x.shape
    xb = torch.full((n_all * d + 2,), CANARY, device=dev)
    xb[1:-1] = torch.from_numpy(x).reshape(-1).to(dev)
    ob = xb if alias else torch.full((n_all * d + 2,), CANARY, device=dev)
    nb = torch.full((4,), CANARY, device=dev)
    rd, sd, td, ad = (torch.from_numpy(v).to(dev).contiguous() for v in (raw, seg, t, alphas))
    cells = torch.tensor([STEP + 1, STEP], dtype=torch.int64, device=dev)
    rc = lib.e3k_sampler_langevin(ob.data_ptr() + 4, xb.data_ptr() + 4, L.ptr(rd), L.ptr(sd), L.ptr(td), L.ptr(ad), n_all, d, g, N_ALPHA,
                                  BETA_0, BETA_1, T_END, SNR, SEED & 0xFFFFFFFF, SEED >> 32, L.ptr(cells), word0, nb.data_ptr() + 4,
                                  L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [STEP + 1, STEP]      # read, not written
    ob, nb, xb = ob.cpu().numpy(), nb.cpu().numpy(), xb.cpu().numpy()
    assert ob[0] == ob[-1] == f32(CANARY) and nb[0] == nb[-1] == f32(CANARY) and xb[0] == xb[-1] == f32(CANARY)
    if not alias:
        assert np.array_equal(xb[1:-1].view(np.int32), x.reshape(-1).view(np.int32))      # the input is read only
    return ob[1:-1].reshape(n_all, d), nb[1:-1]


LANGEVIN_CASES = [(n, d, ghost, g, word0) for n in (1, 63, 64, 65, 1023, 1025, 2049) for d in (1, 3) for ghost in (0, 19)
                  for g, word0 in ((1, 0), (3, 3), (3, 0), (1, 3))]
LANGEVIN_CASES.append((130, 3, 19, 8, 0))      # every planting of t in one batch


@pytest.mark.parametrize("case", LANGEVIN_CASES, ids=lambda c: "N%d_D%d_ghost%d_G%d_word%d" % c)
def test_langevin_against_float64(dev, case):
    n, d, ghost, g, word0 = case
    rng = np.random.default_rng(100 * n + 10 * d + g + word0)
    first_t = (n + d + ghost + word0) % len(PLANTED_T)
    x, raw, seg, t, alphas = _case(n, d, ghost, g, rng, first_t)
    ulp = _expm1_ulp(dev, t[:g], case)
    (want, bound), (norms64, norms_b), k = langevin_reference(x, raw, seg, t, alphas, n, word0, ulp)
    assert np.array_equal(k, np.array([PLANTED_K[(first_t + j) % len(PLANTED_K)] for j in seg[:n]]))      # k and k - 1 at the knots
    got, norms = _call_langevin(dev, x, raw, seg, t, alphas, g, word0, alias=False)
    en = np.abs(norms.astype(f64) - norms64)
    assert (en <= norms_b).all(), (norms, norms64, norms_b)
    err = np.abs(got[:n].astype(f64) - want)
    assert np.isfinite(got).all() and (err <= bound).all(), (err / bound).max()
    assert np.array_equal(got[n:].view(np.int32), x[n:].view(np.int32))                     # ghost rows: bit for bit
    assert (got[:n] != x[:n]).any()                                                          # ... and the real rows moved
    again, norms2 = _call_langevin(dev, x, raw, seg, t, alphas, g, word0, alias=False)      # the same call: the same bits
    assert np.array_equal(again.view(np.int32), got.view(np.int32)) and np.array_equal(norms2.view(np.int32), norms.view(np.int32))
    aliased, norms3 = _call_langevin(dev, x, raw, seg, t, alphas, g, word0, alias=True)     # x_out = x: the same bits
    assert np.array_equal(aliased.view(np.int32), got.view(np.int32)) and np.array_equal(norms3.view(np.int32), norms.view(np.int32))
    worst = float((err / bound).max())
    print(f"langevin {case}: worst error / bound {worst:.3f}, norms {float((en / norms_b).max()):.3f}, expm1f {ulp} ulp")
    record_measured("test_gpu_sampler_kernels", case="langevin_N%d_D%d_ghost%d_G%d_word%d" % case, worst=worst)


def test_langevin_words_and_steps_draw_apart(dev):
    rng = np.random.default_rng(5)
    x, raw, seg, t, alphas = _case(65, 3, 0, 1, rng)
    a, _ = _call_langevin(dev, x, raw, seg, t, alphas, 1, 0, alias=False)
    b, _ = _call_langevin(dev, x, raw, seg, t, alphas, 1, 3, alias=False)
    assert (a != b).mean() >= 0.99


# ---------------------------------------------------------------------------------------------------------------------------------
N_SDE = 1000


def reverse_reference(x, raw, seg, t32, n, word0, ulp):
    s_g, dbeta = _std_ev(t32, ulp)
    sg = seg[:n]
    s = _rows(s_g, sg)
    xr = EV(x[:n].astype(f64))
    score = -(EV(raw[:n].astype(f64)) / s) - xr
    z = _draws(n, x.shape[1], STEP, word0)
    beta = fma(EV(t32.astype(f64)[sg][:, None]), dbeta, float(f32(BETA_0)))
    dt = float(f32(-1.0) / f32(N_SDE))
    mean = xr + ((EV(-0.5) * beta) * xr) * EV(dt)
    noised = mean + (beta.sqrt() * EV(abs(dt)).sqrt()) * z
    return (noised - (EV(dt) * beta) * score).pair()


def _call_reverse(dev, x, raw, seg, t, g, word0, alias, step=STEP):
    L, lib = _lib()
    n_all, d = x.shape
    xb = torch.full((n_all * d + 2,), CANARY, device=dev)
    xb[1:-1] = torch.from_numpy(x).reshape(-1).to(dev)
    ob = xb if alias else torch.full((n_all * d + 2,), CANARY, device=dev)
    rd, sd, td = (torch.from_numpy(v).to(dev).contiguous() for v in (raw, seg, t))
    cells = torch.tensor([step + 1, step], dtype=torch.int64, device=dev)
    rc = lib.e3k_sampler_reverse_em(ob.data_ptr() + 4, xb.data_ptr() + 4, L.ptr(rd), L.ptr(sd), L.ptr(td), n_all, d, g, BETA_0, BETA_1, N_SDE,
                                    SEED & 0xFFFFFFFF, SEED >> 32, L.ptr(cells), word0, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [step + 1, step]
    ob = ob.cpu().numpy()
    assert ob[0] == ob[-1] == f32(CANARY)
    return ob[1:-1].reshape(n_all, d)


REVERSE_CASES = [(n, d, ghost, g, word0) for n in (1, 63, 64, 65, 1023, 1025) for d in (1, 3) for ghost, g, word0 in ((0, 1, 3), (19, 3, 6))]


@pytest.mark.parametrize("case", REVERSE_CASES, ids=lambda c: "N%d_D%d_ghost%d_G%d_word%d" % c)
def test_reverse_em_against_float64(dev, case):
    n, d, ghost, g, word0 = case
    rng = np.random.default_rng(200 * n + 10 * d + g)
    x, raw, seg, t, _ = _case(n, d, ghost, g, rng, first_t=n % len(PLANTED_T))
    ulp = _expm1_ulp(dev, t[:g], case)
    want, bound = reverse_reference(x, raw, seg, t, n, word0, ulp)
    got = _call_reverse(dev, x, raw, seg, t, g, word0, alias=False)
    err = np.abs(got[:n].astype(f64) - want)
    assert np.isfinite(got).all() and (err <= bound).all(), (err / bound).max()
    assert np.array_equal(got[n:].view(np.int32), x[n:].view(np.int32))
    aliased = _call_reverse(dev, x, raw, seg, t, g, word0, alias=True)
    assert np.array_equal(aliased.view(np.int32), got.view(np.int32))
    assert np.array_equal(_call_reverse(dev, x, raw, seg, t, g, word0, alias=False).view(np.int32), got.view(np.int32))
    other = _call_reverse(dev, x, raw, seg, t, g, word0, alias=False, step=STEP + 1)      # the next step's noise is another
    assert (other[:n] != got[:n]).mean() >= 0.99
    worst = float((err / bound).max())
    print(f"reverse_em {case}: worst error / bound {worst:.3f}")
    record_measured("test_gpu_sampler_kernels", case="reverse_N%d_D%d_ghost%d_G%d_word%d" % case, worst=worst)


def test_predictor_noise_is_not_the_correctors_at_the_same_step(dev):
    """x = raw = 0 makes the score 0 and leaves sqrt(beta) sqrt(1 / N) z behind: the predictor's z itself, read back at words D + c,
    against the corrector's words c of the same step (the float64 draws of the layout)."""
    n, d = 65, 3
    rng = np.random.default_rng(3)
    x, raw, seg, t, _ = _case(n, d, 0, 1, rng)
    x[:], raw[:] = 0.0, 0.0
    pred = _call_reverse(dev, x, raw, seg, t, 1, d, alias=False)
    corr = _call_reverse(dev, x, raw, seg, t, 1, 0, alias=False)
    assert (pred != corr).all()
    beta = float(f32(BETA_0)) + float(t[0]) * float(f32(BETA_1) - f32(BETA_0))
    amp = math.sqrt(beta) * math.sqrt(1.0 / N_SDE)
    for got, word0 in ((pred, d), (corr, 0)):
        z = _draws(n, d, STEP, word0)
        assert (np.abs(got.astype(f64) / amp - z.v) <= XI_BOUND + 8 * U * np.abs(z.v)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g1", [1, 64, 300])
def test_begin_step_walks_the_table_and_stops(dev, g1):
    L, lib = _lib()
    times = torch.tensor([CANARY, 1.0, 0.75, 0.5, 0.25, CANARY], device=dev)
    cells = torch.tensor([-77, 0, 0, -77], dtype=torch.int64, device=dev)
    t = torch.full((g1 + 2,), CANARY, device=dev)
    for call in range(6):
        assert lib.e3k_sampler_begin_step(times.data_ptr() + 4, 4, cells.data_ptr() + 8, t.data_ptr() + 4, g1, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        k = min(call, 3)
        assert cells.tolist() == [-77, k + 1, k, -77]
        assert t[0] == CANARY and t[-1] == CANARY and (t[1:-1] == times[1 + k]).all()      # ... and does not move after the fourth
    assert cells.tolist() == [-77, 4, 3, -77]
    cells[1] = -1      # a negative step number is outside the table too
    assert lib.e3k_sampler_begin_step(times.data_ptr() + 4, 4, cells.data_ptr() + 8, t.data_ptr() + 4, g1, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [-77, -1, 3, -77] and (t[1:-1] == times[4]).all()


def test_the_entry_points_refuse_bad_arguments(dev):
    L, lib = _lib()
    x, raw = torch.zeros(4, 3, device=dev), torch.ones(4, 3, device=dev)
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    t, alphas, norms, out = torch.full((2,), 0.5, device=dev), torch.full((5,), 0.9, device=dev), torch.zeros(2, device=dev), torch.zeros(4, 3, device=dev)
    ok = dict(out=L.ptr(out), x=L.ptr(x), raw=L.ptr(raw), seg=L.ptr(seg), t=L.ptr(t), alphas=L.ptr(alphas), N=4, D=3, G=1, n_alpha=5, b0=0.1,
              b1=20.0, T=1.0, snr=0.16, cells=L.ptr(cells), norms=L.ptr(norms), n_sde=1000, times=L.ptr(alphas), n_times=5, G1=2)

    def langevin(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_langevin(a["out"], a["x"], a["raw"], a["seg"], a["t"], a["alphas"], a["N"], a["D"], a["G"], a["n_alpha"], a["b0"],
                                        a["b1"], a["T"], a["snr"], 1, 2, a["cells"], 0, a["norms"], L.stream_ptr())

    def reverse(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_reverse_em(a["out"], a["x"], a["raw"], a["seg"], a["t"], a["N"], a["D"], a["G"], a["b0"], a["b1"], a["n_sde"], 1, 2,
                                          a["cells"], 3, L.stream_ptr())

    def begin(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_begin_step(a["times"], a["n_times"], a["cells"], a["t"], a["G1"], L.stream_ptr())

    assert langevin() == 0 and reverse() == 0 and begin() == 0
    both = [dict(out=None), dict(x=None), dict(raw=None), dict(seg=None), dict(t=None), dict(cells=None), dict(N=0), dict(N=-1), dict(D=0),
            dict(D=1025), dict(G=-1), dict(b1=0.05), dict(b0=-1.0)]
    for bad in both + [dict(alphas=None), dict(norms=None), dict(n_alpha=0), dict(T=0.0), dict(snr=0.0), dict(G=0)]:
        assert langevin(**bad) == -1, bad
    for bad in both + [dict(n_sde=0)]:
        assert reverse(**bad) == -1, bad
    for bad in (dict(times=None), dict(cells=None), dict(t=None), dict(n_times=0), dict(G1=0)):
        assert begin(**bad) == -1, bad
    torch.cuda.synchronize()


def test_the_wrappers_refuse_host_tensors_and_bad_cells(dev):
    from e3_layers_amd.backend import diffusion_ops

    x, raw = torch.zeros(4, 3, device=dev), torch.ones(4, 3, device=dev)
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    t, alphas = torch.full((1, 1), 0.5, device=dev), torch.full((5,), 0.9, device=dev)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    out, norms = diffusion_ops.sampler_langevin(x, raw, seg, t, alphas, 1, 0.1, 20.0, 1.0, 0.16, 7, cells)
    assert out.shape == x.shape and norms.shape == (2,) and torch.isfinite(out).all()
    assert diffusion_ops.sampler_reverse_em(x, raw, seg, t, 1, 0.1, 20.0, 1000, 7, cells, 3, out=x) is x
    with pytest.raises(RuntimeError):
        diffusion_ops.sampler_langevin(x.cpu(), raw.cpu(), seg.cpu(), t.cpu(), alphas.cpu(), 1, 0.1, 20.0, 1.0, 0.16, 7, cells.cpu())      # no CPU fallback
    with pytest.raises(ValueError, match="cells"):
        diffusion_ops.sampler_reverse_em(x, raw, seg, t, 1, 0.1, 20.0, 1000, 7, cells[:1], 3)
    with pytest.raises(ValueError, match="times"):
        diffusion_ops.sampler_langevin(x, raw, seg, t, alphas, 2, 0.1, 20.0, 1.0, 0.16, 7, cells)
    with pytest.raises(ValueError, match="cells"):
        diffusion_ops.sampler_begin_step(alphas, cells.int(), t)
