"""The probability-flow ODE sampler's kernels (csrc/e3k_sampler.hip: e3k_sampler_ode_euler, e3k_sampler_ode_heun) called through the C
ABI on canaried buffers and held to float64, element by element.

The reference is the float64 form of the header's formulas on the floats the kernel receives, carried through the running error
analysis of tests/test_gpu_node_matrix.py (EV: a float64 value and a bound on |fp32 result - value|), as
tests/test_gpu_sampler_kernels.py does for the predictor-corrector kernels -- its s(t) (``_std_ev``: lm = t fma(q, t, h), the device's
expm1f at its measured ulps, one sqrtf) and its batch builder are used as they are:
  * the table is planted, exact: t_k = times[k], t_n = times[k + 1]; hs = t_n - t_k is one subtraction;
  * beta = fma(t, beta_1 - beta_0, beta_0); d = (0.5 beta) (raw / s); 0.5 beta is exact in fp32, the bound charges a rounding anyway;
  * x_out = fma(hs, d1, x) (Euler, stage A) and fma(0.5 hs, d1 + d2, x0) (stage B; d1 is an input there, exact).
Ghost rows (segment G: outside [0, G)), steps outside the table and everything "the same bits" are compared as int32.

Shapes: one thread per component in 256-thread blocks -- N D below, at and above one block and one wavefront, odd sizes, more than one
block (N = 1025 with D = 3 is 13 blocks), D = 1 (i = k) and D = 3 (i = k / 3)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_node_matrix import EV, fma
from tests.test_gpu_sampler_kernels import BETA_0, BETA_1, CANARY, _case, _expm1_ulp, _std_ev
from tests.util import record_measured

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
TIMES = np.array([1.0, 0.75, 0.5, 0.25, 1e-3], dtype=f32)      # five times, both ends of a run planted
N_STEPS = len(TIMES) - 1
STEPS = (0, 2, N_STEPS - 1)


def _lib():
    from e3_layers_amd.backend import lib as L

    return L, L.load()


def _drift_ev(raw, t32, ulp):
    """d(raw, t) = (0.5 beta(t)) (raw / s(t)) at one table entry"""
    s, dbeta = _std_ev(np.array([t32], dtype=f32), ulp)
    beta = fma(EV(f64(t32)), dbeta, float(f32(BETA_0)))
    return (EV(0.5) * beta) * (EV(raw.astype(f64)) / EV(s.v[0], s.e[0]))


def euler_reference(x, raw, n, k, ulp):
    d1 = _drift_ev(raw[:n], TIMES[k], ulp)
    hs = EV(f64(TIMES[k + 1])) - EV(f64(TIMES[k]))
    return fma(hs, d1, EV(x[:n].astype(f64))).pair(), d1.pair()


def heun_reference(x0, d1, raw2, n, k, ulp):
    d2 = _drift_ev(raw2[:n], TIMES[k + 1], ulp)
    hs = EV(f64(TIMES[k + 1])) - EV(f64(TIMES[k]))
    return fma(EV(0.5) * hs, EV(d1[:n].astype(f64)) + d2, EV(x0[:n].astype(f64))).pair()


def _canaried(dev, values):
    buf = torch.full((values.size + 2,), CANARY, device=dev)
    buf[1:-1] = torch.from_numpy(values).reshape(-1).to(dev)
    return buf


def _inner(buf, shape):
    host = buf.cpu().numpy()
    assert host[0] == host[-1] == f32(CANARY)
    return host[1:-1].reshape(shape)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _call_euler(dev, x, raw, seg, g, k, alias=False, want_d=True, g1=0, times=TIMES):
    """-> (x_out, d_out or None, t_out or None); the canaries, the read-only input and the cells are checked here"""
    L, lib = _lib()
    n_all, d = x.shape
    xb = _canaried(dev, x)
    ob = xb if alias else _canaried(dev, np.full_like(x, CANARY))
    db = _canaried(dev, np.full_like(x, CANARY)) if want_d else None
    tb = torch.full((g1 + 2,), CANARY, device=dev) if g1 else None
    rd, sd, td = (torch.from_numpy(v).to(dev).contiguous() for v in (raw, seg, times))
    cells = torch.tensor([k + 1, k], dtype=torch.int64, device=dev)
    rc = lib.e3k_sampler_ode_euler(ob.data_ptr() + 4, db.data_ptr() + 4 if want_d else None, xb.data_ptr() + 4, L.ptr(rd), L.ptr(sd), L.ptr(td),
                                   len(times), L.ptr(cells), tb.data_ptr() + 4 if g1 else None, g1, n_all, d, g, BETA_0, BETA_1,
                                   L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [k + 1, k]      # read, never written
    if not alias:
        assert _same(_inner(xb, x.shape), x)      # the input is read only
    return _inner(ob, x.shape), _inner(db, x.shape) if want_d else None, _inner(tb, (g1,)) if g1 else None


def _call_heun(dev, x0, d1, raw2, seg, g, k, alias=False, times=TIMES):
    L, lib = _lib()
    n_all, d = x0.shape
    xb = _canaried(dev, x0)
    ob = xb if alias else _canaried(dev, np.full_like(x0, CANARY))
    dd, rd, sd, td = (torch.from_numpy(v).to(dev).contiguous() for v in (d1, raw2, seg, times))
    cells = torch.tensor([k + 1, k], dtype=torch.int64, device=dev)
    rc = lib.e3k_sampler_ode_heun(ob.data_ptr() + 4, xb.data_ptr() + 4, L.ptr(dd), L.ptr(rd), L.ptr(sd), L.ptr(td), len(times), L.ptr(cells),
                                  n_all, d, g, BETA_0, BETA_1, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [k + 1, k]
    if not alias:
        assert _same(_inner(xb, x0.shape), x0)
    assert _same(dd.cpu().numpy(), d1)
    return _inner(ob, x0.shape)


CASES = [(n, d, ghost, g) for n in (1, 63, 64, 65, 255, 256, 257, 1025) for d in (1, 3) for ghost in (0, 19) for g in (1, 3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_D%d_ghost%d_G%d" % c)
def test_euler_against_float64(dev, case):
    n, d, ghost, g = case
    rng = np.random.default_rng(300 * n + 10 * d + ghost + g)
    x, raw, seg, _, _ = _case(n, d, ghost, g, rng)
    ulp = _expm1_ulp(dev, TIMES, case)
    worst = 0.0
    for k in STEPS:
        (want, bound), (want_d, bound_d) = euler_reference(x, raw, n, k, ulp)
        got, got_d, _ = _call_euler(dev, x, raw, seg, g, k)
        err, err_d = np.abs(got[:n].astype(f64) - want), np.abs(got_d[:n].astype(f64) - want_d)
        assert np.isfinite(got).all() and (err <= bound).all(), (k, (err / bound).max())
        assert (err_d <= bound_d).all(), (k, (err_d / bound_d).max())
        assert _same(got[n:], x[n:]) and (got_d[n:] == 0).all()            # ghost rows: bit for bit, no drift
        assert (got[:n] != x[:n]).any()                                     # ... and the real rows moved
        again, again_d, _ = _call_euler(dev, x, raw, seg, g, k)             # the same call: the same bits
        assert _same(again, got) and _same(again_d, got_d)
        aliased, aliased_d, _ = _call_euler(dev, x, raw, seg, g, k, alias=True)      # x_out = x
        assert _same(aliased, got) and _same(aliased_d, got_d)
        bare, none_d, none_t = _call_euler(dev, x, raw, seg, g, k, want_d=False)      # d_out null: the same x_out
        assert _same(bare, got) and none_d is None and none_t is None
        timed, timed_d, t_out = _call_euler(dev, x, raw, seg, g, k, g1=g + 1)        # ... and with t_out
        assert _same(timed, got) and _same(timed_d, got_d) and (t_out == TIMES[k + 1]).all()
        worst = max(worst, float((err / bound).max()), float((err_d / bound_d).max()))
    print(f"ode_euler {case}: worst error / bound {worst:.3f}, expm1f {ulp} ulp")
    record_measured("test_gpu_ode_kernels", case="euler_N%d_D%d_ghost%d_G%d" % case, worst=worst)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_D%d_ghost%d_G%d" % c)
def test_heun_against_float64(dev, case):
    n, d, ghost, g = case
    rng = np.random.default_rng(700 * n + 10 * d + ghost + g)
    x0, raw2, seg, _, _ = _case(n, d, ghost, g, rng)
    d1 = rng.standard_normal(x0.shape).astype(f32)
    ulp = _expm1_ulp(dev, TIMES, case)
    worst = 0.0
    for k in STEPS:
        want, bound = heun_reference(x0, d1, raw2, n, k, ulp)
        got = _call_heun(dev, x0, d1, raw2, seg, g, k)
        err = np.abs(got[:n].astype(f64) - want)
        assert np.isfinite(got).all() and (err <= bound).all(), (k, (err / bound).max())
        assert _same(got[n:], x0[n:]) and (got[:n] != x0[:n]).any()
        assert _same(_call_heun(dev, x0, d1, raw2, seg, g, k), got)                  # the same call: the same bits
        assert _same(_call_heun(dev, x0, d1, raw2, seg, g, k, alias=True), got)      # x_out = x0
        worst = max(worst, float((err / bound).max()))
    print(f"ode_heun {case}: worst error / bound {worst:.3f}, expm1f {ulp} ulp")
    record_measured("test_gpu_ode_kernels", case="heun_N%d_D%d_ghost%d_G%d" % case, worst=worst)


def test_stage_b_continues_stage_a(dev):
    """the two launches as the sampler chains them: stage B on stage A's own d_out is Heun's step of the float64 formulas"""
    n, d, g, k = 257, 3, 3, 2
    rng = np.random.default_rng(11)
    x, raw, seg, _, _ = _case(n, d, 19, g, rng)
    raw2 = rng.standard_normal(x.shape).astype(f32)
    ulp = _expm1_ulp(dev, TIMES, "chain")
    _, d1, _ = _call_euler(dev, x, raw, seg, g, k)
    got = _call_heun(dev, x, d1, raw2, seg, g, k)
    want, bound = heun_reference(x, d1, raw2, n, k, ulp)
    assert (np.abs(got[:n].astype(f64) - want) <= bound).all() and _same(got[n:], x[n:])


@pytest.mark.parametrize("g1", [1, 64, 300])
def test_t_out_takes_the_end_of_step_time(dev, g1):
    rng = np.random.default_rng(g1)
    x, raw, seg, _, _ = _case(65, 3, 19, 3, rng)
    for k in STEPS:
        _, _, t_out = _call_euler(dev, x, raw, seg, 3, k, g1=g1)      # (the canaries around [0, G1) are checked in the call)
        assert t_out.shape == (g1,) and (t_out == TIMES[k + 1]).all()


@pytest.mark.parametrize("k", [-1, len(TIMES) - 1, len(TIMES) + 5])
def test_steps_outside_the_table_stand_still(dev, k):
    rng = np.random.default_rng(17)
    x, raw, seg, _, _ = _case(257, 3, 19, 3, rng)
    d1 = rng.standard_normal(x.shape).astype(f32)
    for alias in (False, True):
        got, got_d, t_out = _call_euler(dev, x, raw, seg, 3, k, alias=alias, g1=64)
        assert _same(got, x) and (got_d == 0).all() and (t_out == f32(CANARY)).all()      # no time is written
        assert _same(_call_heun(dev, x, d1, raw, seg, 3, k, alias=alias), x)


def test_the_entry_points_refuse_bad_arguments(dev):
    L, lib = _lib()
    x, raw, d1 = torch.zeros(4, 3, device=dev), torch.ones(4, 3, device=dev), torch.ones(4, 3, device=dev)
    out, d_out = torch.zeros(4, 3, device=dev), torch.zeros(4, 3, device=dev)
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    times, t = torch.from_numpy(TIMES).to(dev), torch.zeros(2, device=dev)
    ok = dict(out=L.ptr(out), d=L.ptr(d_out), x=L.ptr(x), raw=L.ptr(raw), d1=L.ptr(d1), seg=L.ptr(seg), times=L.ptr(times), n_times=5,
              cells=L.ptr(cells), t=L.ptr(t), G1=2, N=4, D=3, G=1, b0=0.1, b1=20.0)

    def euler(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_ode_euler(a["out"], a["d"], a["x"], a["raw"], a["seg"], a["times"], a["n_times"], a["cells"], a["t"], a["G1"],
                                         a["N"], a["D"], a["G"], a["b0"], a["b1"], L.stream_ptr())

    def heun(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_ode_heun(a["out"], a["x"], a["d1"], a["raw"], a["seg"], a["times"], a["n_times"], a["cells"], a["N"], a["D"],
                                        a["G"], a["b0"], a["b1"], L.stream_ptr())

    assert euler() == 0 and heun() == 0
    assert euler(d=None) == 0 and euler(t=None, G1=0) == 0 and euler(out=ok["x"]) == 0 and heun(out=ok["x"]) == 0 and euler(G=0) == 0
    both = [dict(out=None), dict(x=None), dict(raw=None), dict(seg=None), dict(times=None), dict(cells=None), dict(N=0), dict(N=-1),
            dict(N=1 << 31), dict(D=0), dict(D=1025), dict(G=-1), dict(n_times=1), dict(n_times=0), dict(b1=0.05), dict(b0=-1.0),
            dict(N=(1 << 31) - 1, D=1024)]      # (N D >= 2^38)
    for bad in both + [dict(G1=0), dict(d=ok["out"]), dict(d=ok["x"])]:
        assert euler(**bad) == -1, bad
    for bad in both + [dict(d1=None), dict(d1=ok["out"])]:
        assert heun(**bad) == -1, bad
    torch.cuda.synchronize()


def test_the_wrappers_refuse_host_tensors_and_bad_cells(dev):
    from e3_layers_amd.backend import diffusion_ops

    rng = np.random.default_rng(23)
    x_np, raw_np, seg_np, _, _ = _case(65, 3, 19, 3, rng)
    x, raw, seg = (torch.from_numpy(v).to(dev) for v in (x_np, raw_np, seg_np))
    times = torch.from_numpy(TIMES).to(dev)
    cells = torch.tensor([3, 2], dtype=torch.int64, device=dev)
    t = torch.zeros(4, 1, device=dev)
    # the wrappers are the entry points: the same bits as the direct calls
    want, want_d, _ = _call_euler(dev, x_np, raw_np, seg_np, 3, 2)
    new, d1 = diffusion_ops.sampler_ode_euler(x, raw, seg, times, cells, 3, BETA_0, BETA_1, t_out=t)
    assert _same(new.cpu().numpy(), want) and _same(d1.cpu().numpy(), want_d) and (t == float(TIMES[3])).all()
    fin = diffusion_ops.sampler_ode_heun(x, d1, raw, seg, times, cells, 3, BETA_0, BETA_1)
    assert _same(fin.cpu().numpy(), _call_heun(dev, x_np, want_d, raw_np, seg_np, 3, 2))
    same, none = diffusion_ops.sampler_ode_euler(x.clone(), raw, seg, times, cells, 3, BETA_0, BETA_1, want_d=False)
    assert none is None and torch.equal(same, new)
    y = x.clone()
    assert diffusion_ops.sampler_ode_euler(y, raw, seg, times, cells, 3, BETA_0, BETA_1, out=y)[0] is y and torch.equal(y, new)
    with pytest.raises(RuntimeError):
        diffusion_ops.sampler_ode_euler(x.cpu(), raw.cpu(), seg.cpu(), times.cpu(), cells.cpu(), 3, BETA_0, BETA_1)      # no CPU fallback
    with pytest.raises(RuntimeError):
        diffusion_ops.sampler_ode_heun(x.cpu(), d1.cpu(), raw.cpu(), seg.cpu(), times.cpu(), cells.cpu(), 3, BETA_0, BETA_1)
    with pytest.raises(RuntimeError):
        diffusion_ops.sampler_ode_euler(x, raw, seg, times, cells, 3, BETA_0, BETA_1, t_out=t.cpu())
    for bad in (cells[:1], cells.int(), cells.repeat(2)[::2]):
        with pytest.raises(ValueError, match="cells"):
            diffusion_ops.sampler_ode_euler(x, raw, seg, times, bad, 3, BETA_0, BETA_1)
        with pytest.raises(ValueError, match="cells"):
            diffusion_ops.sampler_ode_heun(x, d1, raw, seg, times, bad, 3, BETA_0, BETA_1)
    with pytest.raises(ValueError, match="times"):
        diffusion_ops.sampler_ode_euler(x, raw, seg, times[:1], cells, 3, BETA_0, BETA_1)
    with pytest.raises(ValueError, match="times"):
        diffusion_ops.sampler_ode_heun(x, d1, raw, seg, times.double(), cells, 3, BETA_0, BETA_1)
    with pytest.raises(ValueError, match="t_out"):
        diffusion_ops.sampler_ode_euler(x, raw, seg, times, cells, 3, BETA_0, BETA_1, t_out=t.double())
    with pytest.raises(ValueError, match="d1"):
        diffusion_ops.sampler_ode_heun(x, d1, raw, seg, times, cells, 3, BETA_0, BETA_1, out=d1)
    with pytest.raises(ValueError, match="node_seg"):
        diffusion_ops.sampler_ode_heun(x, d1, raw[:, :2], seg, times, cells, 3, BETA_0, BETA_1)
