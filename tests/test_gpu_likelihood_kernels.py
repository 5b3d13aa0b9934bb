"""The likelihood's kernels (csrc/e3k_sampler.hip: e3k_sampler_probe, e3k_sampler_ode_div, e3k_sampler_prior_logp) called through the C
ABI inside NaN arenas and checked on every element, and the step kernels (e3k_sampler_begin_step, e3k_sampler_ode_euler,
e3k_sampler_ode_heun) on the ASCENDING table the likelihood runs them on.

e3k_sampler_probe: kind 0 equals data.compute_edge.rademacher_draw bit for bit; kind 1 is within XI_BOUND of normal_draw in float64
(tests/test_gpu_md_integrator_kernels.py: the same device function, the bound tests/test_gpu_sampler_kernels.py charges its draws).

e3k_sampler_ode_div: acc[g] = fma(coef, S, acc[g]), S = sum of (double)probe (double)vjp over the graph, coef = (w c(t)) scale.
  * The products are exact in double (24 x 24 bits).  A sum of n terms in ANY order is within gamma_{n-1} sum|terms| of the exact sum,
    gamma_n = n u / (1 - n u), u = 2^-53: the kernel's order is fixed but not part of its contract.
  * coef: beta = t db + b0 (2 roundings, or one as an FMA), lm = t (q t + hh) (3 roundings, no cancellation: q, hh <= 0), -expm1(2 lm)
    passes lm's relative error on with a factor |y e^y / expm1(y)| <= 1 and adds the device function's own error -- charged 3 ulp = 6 u,
    OpenCL's full-profile limit for the double expm1 --, sqrt halves what it receives and rounds once (correctly rounded: u), then one
    division and the two products (w c) scale; w = t_n - t_k is exact in double for fp32 entries a factor 2^29 apart at most:
        2 + (3 + 6) / 2 + 1 + 1 + 2 = 10.5 u, charged COEF_U = 12 u.
  * the final FMA rounds once: u |acc'|.
  So |acc' - exact| <= |coef| sum|terms| (gamma_{n-1} + COEF_U u) (1 + 2^-40) + u |acc'|, against numpy longdouble (64-bit mantissa).
  Small integers: S is exact, and a graph of one row with probe = vjp = 1 returns coef itself, so every other graph of the same launch
  must hold coef S to the bit -- c(t) divided out by the kernel's own unit response.

e3k_sampler_prior_logp: out[g] += -0.5 S - (0.5 n_g D) ln(2 pi) with S = sum x^2 (exact squares): gamma_{n-1} S / 2, one rounding of
the constant term, one of the difference, one of the sum into out."""
import numpy as np
import pytest
import torch

from tests.test_gpu_md_integrator_kernels import XI_BOUND
from tests.test_gpu_node_matrix import EV, fma
from tests.test_gpu_ode_kernels import _call_euler, _call_heun, _drift_ev, _same
from tests.test_gpu_sampler_kernels import BETA_0, BETA_1, _case, _expm1_ulp
from tests.util import record_measured

pytestmark = pytest.mark.gpu

f32, f64, ld = np.float32, np.float64, np.longdouble
U53 = 2.0 ** -53
COEF_U = 12
SEED = (977 << 32) + 20241019      # both seed words in use
ASC = np.array([1e-3, 0.25, 0.5, 0.75, 1.0], dtype=f32)      # an ascending table, both ends of a run planted
LN_2PI = float("1.8378770664093454835606594728112")
NAN = float("nan")


def _lib():
    from e3_layers_amd.backend import lib as L

    return L, L.load()


def _arena(dev, values, dtype):
    """the values between two NaN guards; -> the buffer (the operand starts one element in)"""
    buf = torch.full((values.size + 2,), NAN, device=dev, dtype=dtype)
    buf[1:-1] = torch.from_numpy(np.ascontiguousarray(values)).reshape(-1).to(dev)
    return buf


def _inner(buf, shape):
    host = buf.cpu().numpy()
    assert np.isnan(host[0]) and np.isnan(host[-1])      # nothing was written outside the operand
    return host[1:-1].reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------
# e3k_sampler_probe
# ---------------------------------------------------------------------------------------------------------------------
def _call_probe(dev, seg, d, g, draw, word0, kind):
    L, lib = _lib()
    n_all = seg.size
    out = _arena(dev, np.full((n_all, d), np.nan, dtype=f32), torch.float32)
    sd = torch.from_numpy(seg).to(dev)
    rc = lib.e3k_sampler_probe(out.data_ptr() + 4, L.ptr(sd), n_all, d, g, SEED & 0xFFFFFFFF, SEED >> 32, draw, word0, kind, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return _inner(out, (n_all, d))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
@pytest.mark.parametrize("d", [1, 3, 4])
def test_probe_equals_the_host_draws(dev, n, d):
    from e3_layers_amd.data.compute_edge import normal_draw, rademacher_draw

    rng = np.random.default_rng(10 * n + d)
    _, _, seg, _, _ = _case(n, d, 19, 3, rng)
    node, word0, draw = torch.arange(n).reshape(-1, 1), 5, 1001
    words = word0 + torch.arange(d).reshape(1, -1)
    got = _call_probe(dev, seg, d, 3, draw, word0, 0)
    want = rademacher_draw(SEED, draw, node, words, torch.float32).numpy()
    assert np.array_equal(got[:n], want) and set(np.unique(got[:n])) <= {-1.0, 1.0}
    assert (got[n:] == 0).all()                                   # ghost rows
    assert _same(_call_probe(dev, seg, d, 3, draw, word0, 0), got)
    if n * d >= 63:      # another draw index, another first word: other signs
        assert not np.array_equal(_call_probe(dev, seg, d, 3, draw + 1, word0, 0)[:n], want)
        assert not np.array_equal(_call_probe(dev, seg, d, 3, draw, word0 + 1, 0)[:n], want)
    gauss = _call_probe(dev, seg, d, 3, draw, word0, 1)
    z = normal_draw(SEED, draw, node, words, torch.float64).numpy()
    err = np.abs(gauss[:n].astype(f64) - z).max()
    assert err <= XI_BOUND, (err, XI_BOUND)
    assert (gauss[n:] == 0).all()
    record_measured("test_gpu_likelihood_kernels", case=f"probe_gaussian_N{n}_D{d}", worst=err / XI_BOUND)


# ---------------------------------------------------------------------------------------------------------------------
# e3k_sampler_ode_div and e3k_sampler_prior_logp
# ---------------------------------------------------------------------------------------------------------------------
ELEMENTS = (0, 1, 63, 64, 65, 255, 256, 257, 3075)      # n_g D per graph (0 and 1 rows; around a wavefront and the workgroup; 13 rounds)


def _graphs(g, d):
    """row counts of g real graphs, n_g d running through ELEMENTS (rounded up to whole rows), and a ghost graph of 19 rows behind"""
    counts = [-(-ELEMENTS[j % len(ELEMENTS)] // d) for j in range(g)]
    if g == 1:
        counts = [-(-3075 // d)]
    return np.array(counts + [19], dtype=np.int64)


def _row_ptr(dev, counts):
    L, lib = _lib()
    cd = torch.from_numpy(counts).to(dev)
    ptr = torch.empty(counts.size + 1, dtype=torch.int32, device=dev)
    assert lib.e3k_counts_to_ptr(L.ptr(cd), counts.size, L.ptr(ptr), L.stream_ptr()) == 0
    return ptr


def _coef_ld(k, stage, scale, times=ASC):
    """(w c(t)) scale in longdouble from the doubles of the fp32 parameters, as include/e3k.h states it"""
    tk, tn = ld(times[k]), ld(times[k + 1])
    w = tn - tk if stage == 0 else ld(0.5) * (tn - tk)
    t = tn if stage == 2 else tk
    b0, db = ld(f32(BETA_0)), ld(f32(BETA_1)) - ld(f32(BETA_0))
    lm = t * (ld(-0.25) * db * t + ld(-0.5) * b0)
    return w * (ld(0.5) * (t * db + b0)) / np.sqrt(-np.expm1(ld(2.0) * lm)) * ld(scale)


def _call_div(dev, acc0, probe, vjp, counts, g, k, stage, scale, times=ASC):
    """acc0: [g + 1] doubles, the ghost graph's slot last (it must come back as it went in)"""
    L, lib = _lib()
    n_all, d = probe.shape
    acc = _arena(dev, acc0, torch.float64)
    pd, vd, td = (torch.from_numpy(v).to(dev).contiguous() for v in (probe, vjp, times))
    ptr = _row_ptr(dev, counts)
    cells = torch.tensor([k + 1, k], dtype=torch.int64, device=dev)
    rc = lib.e3k_sampler_ode_div(acc.data_ptr() + 8, L.ptr(pd), L.ptr(vd), L.ptr(ptr), L.ptr(td), len(times), L.ptr(cells), n_all, d, g,
                                 stage, scale, BETA_0, BETA_1, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [k + 1, k] and _same(pd.cpu().numpy(), probe) and _same(vd.cpu().numpy(), vjp)      # read only
    out = _inner(acc, (g + 1,))
    assert np.array_equal(out[g:].view(np.int64), acc0[g:].view(np.int64))      # the ghost graph's slot: bit for bit
    return out


def _call_prior(dev, out0, x, counts, g):
    L, lib = _lib()
    n_all, d = x.shape
    out = _arena(dev, out0, torch.float64)
    xd = torch.from_numpy(x).to(dev).contiguous()
    rc = lib.e3k_sampler_prior_logp(out.data_ptr() + 8, L.ptr(xd), L.ptr(_row_ptr(dev, counts)), n_all, d, g, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert _same(xd.cpu().numpy(), x)
    res = _inner(out, (g + 1,))
    assert np.array_equal(res[g:].view(np.int64), out0[g:].view(np.int64))
    return res


def _per_graph(values, counts, g):
    """[(longdouble sum, longdouble sum of magnitudes, terms)] per real graph of values [N, D]"""
    ptr = np.concatenate([[0], np.cumsum(counts)])
    out = []
    for j in range(g):
        v = values[ptr[j]:ptr[j + 1]].reshape(-1).astype(ld)
        out.append((v.sum(), np.abs(v).sum(), v.size))
    return out


def _gamma(n):
    n = max(n - 1, 0)
    return n * U53 / (1.0 - n * U53)


CASES = [(g, d) for g in (1, 37) for d in (1, 3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "G%d_D%d" % c)
def test_ode_div_against_longdouble(dev, case):
    g, d = case
    rng = np.random.default_rng(100 * g + d)
    counts = _graphs(g, d)
    n_all = int(counts.sum())
    probe = rng.standard_normal((n_all, d)).astype(f32)
    vjp = rng.standard_normal((n_all, d)).astype(f32)
    terms = _per_graph(probe.astype(f64) * vjp.astype(f64), counts, g)      # (exact products)
    worst = 0.0
    for stage in (0, 1, 2):
        for k, scale, start in ((0, 1.0, 0.0), (2, 0.5, 1.0), (len(ASC) - 2, 1.0 / 3.0, -1.0)):
            acc0 = np.concatenate([start * rng.standard_normal(g), [NAN]]).astype(f64)      # (zero, or something to accumulate into)
            got = _call_div(dev, acc0, probe, vjp, counts, g, k, stage, scale)
            coef = _coef_ld(k, stage, scale)
            for j, (s, mag, n) in enumerate(terms):
                want = ld(acc0[j]) + coef * s
                bound = float(abs(coef) * mag) * (_gamma(n) + COEF_U * U53) * (1.0 + 2.0 ** -40) + U53 * abs(got[j])
                err = float(abs(ld(got[j]) - want))
                assert np.isfinite(got[j]) and err <= bound, (stage, k, j, n, err, bound)
                if n == 0:
                    assert got[j] == acc0[j] or (acc0[j] == 0 and got[j] == 0)      # a graph of no rows adds 0
                elif bound > 0:
                    worst = max(worst, err / bound)
            again = _call_div(dev, acc0, probe, vjp, counts, g, k, stage, scale)
            assert np.array_equal(again.view(np.int64), got.view(np.int64))      # the same call: the same bits
        # outside the table: acc is untouched, bit for bit
        acc0 = np.concatenate([rng.standard_normal(g), [NAN]]).astype(f64)
        for k in (-1, len(ASC) - 1):
            got = _call_div(dev, acc0, probe, vjp, counts, g, k, stage, 1.0)
            assert np.array_equal(got.view(np.int64), acc0.view(np.int64)), (stage, k)
    print(f"ode_div {case}: worst error / bound {worst:.3f}")
    record_measured("test_gpu_likelihood_kernels", case="ode_div_G%d_D%d" % case, worst=worst)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "G%d_D%d" % c)
def test_ode_div_small_integers_exactly(dev, case):
    """graph 0 is one row of ones in component 0: the launch's own coef; every other graph must hold coef S to the bit"""
    g, d = case
    rng = np.random.default_rng(7 * g + d)
    counts = np.concatenate([[1], _graphs(g, d)])
    n_all = int(counts.sum())
    probe = rng.choice(np.array([-1.0, 1.0], dtype=f32), (n_all, d))
    vjp = rng.integers(-8, 9, (n_all, d)).astype(f32)
    probe[0], vjp[0] = 0.0, 0.0
    probe[0, 0] = vjp[0, 0] = 1.0
    sums = [float(s) for s, _, _ in _per_graph(probe.astype(f64) * vjp.astype(f64), counts, g + 1)]
    assert any(s != 0 for s in sums[1:])
    for stage in (0, 1, 2):
        for k, scale in ((0, 1.0), (len(ASC) - 2, 0.5)):
            acc0 = np.concatenate([np.zeros(g + 1), [NAN]])
            got = _call_div(dev, acc0, probe, vjp, counts, g + 1, k, stage, scale)
            coef = got[0]
            ref = float(_coef_ld(k, stage, scale))
            assert coef > 0 and abs(coef - ref) <= (COEF_U + 1) * U53 * ref, (stage, k, coef, ref)
            for j in range(1, g + 1):
                assert got[j] == f64(coef) * f64(sums[j]), (stage, k, j, got[j], coef, sums[j])
    # the three stages weigh as they should: Euler's w is twice Heun A's at the same t, and Heun B reads the next time
    a, b, c = (_call_div(dev, np.concatenate([np.zeros(g + 1), [NAN]]), probe, vjp, counts, g + 1, 1, st, 1.0)[0] for st in (0, 1, 2))
    assert a == 2.0 * b and c != b


@pytest.mark.parametrize("case", CASES, ids=lambda c: "G%d_D%d" % c)
def test_prior_logp(dev, case):
    g, d = case
    rng = np.random.default_rng(900 * g + d)
    counts = _graphs(g, d)
    n_all = int(counts.sum())
    x = rng.standard_normal((n_all, d)).astype(f32)
    terms = _per_graph(x.astype(f64) ** 2, counts, g)
    worst = 0.0
    for start in (0.0, 1.0):
        out0 = np.concatenate([start * 50.0 * rng.standard_normal(g), [NAN]]).astype(f64)
        got = _call_prior(dev, out0, x, counts, g)
        for j, (s, _, n) in enumerate(terms):
            norm = ld(0.5) * ld(n) * ld(LN_2PI)
            want = ld(out0[j]) - ld(0.5) * s - norm
            bound = (0.5 * float(s) * _gamma(n) + U53 * float(norm) + U53 * float(ld(0.5) * s + norm)) * (1.0 + 2.0 ** -40) + U53 * abs(got[j])
            err = float(abs(ld(got[j]) - want))
            assert err <= bound, (j, n, err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
        assert np.array_equal(_call_prior(dev, out0, x, counts, g).view(np.int64), got.view(np.int64))
    # small integers: every operation of the kernel is exact or a single rounding that float64 numpy repeats
    xi = rng.integers(-8, 9, (n_all, d)).astype(f32)
    out0 = np.concatenate([rng.integers(-4, 5, g).astype(f64), [NAN]])
    got = _call_prior(dev, out0, xi, counts, g)
    for j, (s, _, n) in enumerate(_per_graph(xi.astype(f64) ** 2, counts, g)):
        want = f64(out0[j]) + (f64(-0.5) * f64(s) - f64(0.5 * n) * f64(LN_2PI))
        assert got[j] == want, (j, got[j], want)
    print(f"prior_logp {case}: worst error / bound {worst:.3f}")
    record_measured("test_gpu_likelihood_kernels", case="prior_logp_G%d_D%d" % case, worst=worst)


def test_keys_accumulate_into_one_accumulator(dev):
    """several keys are consecutive launches into the same acc, through the wrappers"""
    from e3_layers_amd.backend import diffusion_ops

    rng = np.random.default_rng(5)
    counts = _graphs(5, 1)
    n_all = int(counts.sum())
    ptr = diffusion_ops.graph_row_pointers(torch.from_numpy(counts).to(dev))
    assert ptr.cpu().tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    times, cells = torch.from_numpy(ASC).to(dev), torch.tensor([2, 1], dtype=torch.int64, device=dev)
    acc = torch.zeros(5, dtype=torch.float64, device=dev)
    want = np.zeros(5, dtype=ld)
    mags = np.zeros(5)
    for d in (3, 2):
        p, v = rng.standard_normal((n_all, d)).astype(f32), rng.standard_normal((n_all, d)).astype(f32)
        diffusion_ops.sampler_ode_div(acc, torch.from_numpy(p).to(dev), torch.from_numpy(v).to(dev), ptr, times, cells, 5, 2, 0.5, BETA_0, BETA_1)
        coef = _coef_ld(1, 2, 0.5)
        for j, (s, mag, n) in enumerate(_per_graph(p.astype(f64) * v.astype(f64), counts, 5)):
            want[j] += coef * s
            mags[j] += float(abs(coef) * mag) * (_gamma(n) + COEF_U * U53) + U53 * float(abs(want[j]))
    got = acc.cpu().numpy()
    assert (np.abs(got.astype(ld) - want).astype(f64) <= mags * (1.0 + 2.0 ** -40) + 1e-300).all()
    out = torch.zeros(5, dtype=torch.float64, device=dev)
    x = torch.from_numpy(rng.standard_normal((n_all, 3)).astype(f32)).to(dev)
    diffusion_ops.sampler_prior_logp(out, x, ptr, 5)
    first = out.clone()
    diffusion_ops.sampler_prior_logp(out, x, ptr, 5)
    assert torch.equal(out, first + first)      # (doubling is exact)
    with pytest.raises(RuntimeError):
        diffusion_ops.sampler_prior_logp(out.cpu(), x.cpu(), ptr.cpu(), 5)      # no CPU fallback
    with pytest.raises(ValueError, match="float64"):
        diffusion_ops.sampler_prior_logp(out.float(), x, ptr, 5)
    with pytest.raises(ValueError, match="row_ptr"):
        diffusion_ops.sampler_ode_div(acc, x, x, ptr.long(), times, cells, 5, 0, 1.0, BETA_0, BETA_1)
    with pytest.raises(ValueError, match="cells"):
        diffusion_ops.sampler_ode_div(acc, x, x, ptr, times, cells[:1], 5, 0, 1.0, BETA_0, BETA_1)
    with pytest.raises(ValueError, match="shape"):
        diffusion_ops.sampler_ode_div(acc, x, x[:, :2], ptr, times, cells, 5, 0, 1.0, BETA_0, BETA_1)


def test_the_entry_points_refuse_bad_arguments(dev):
    L, lib = _lib()
    x, p = torch.ones(4, 3, device=dev), torch.ones(4, 3, device=dev)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    ptr = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    times = torch.from_numpy(ASC).to(dev)
    ok = dict(acc=L.ptr(acc), p=L.ptr(p), x=L.ptr(x), seg=L.ptr(seg), ptr=L.ptr(ptr), times=L.ptr(times), n_times=5, cells=L.ptr(cells),
              N=4, D=3, G=1, stage=0, scale=1.0, b0=0.1, b1=20.0, kind=0)

    def probe(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_probe(a["x"], a["seg"], a["N"], a["D"], a["G"], 1, 2, 1001, 0, a["kind"], L.stream_ptr())

    def div(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_ode_div(a["acc"], a["p"], a["x"], a["ptr"], a["times"], a["n_times"], a["cells"], a["N"], a["D"], a["G"],
                                       a["stage"], a["scale"], a["b0"], a["b1"], L.stream_ptr())

    def prior(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_prior_logp(a["acc"], a["x"], a["ptr"], a["N"], a["D"], a["G"], L.stream_ptr())

    assert probe() == 0 and div() == 0 and prior() == 0 and probe(kind=1) == 0 and probe(G=0) == 0 and div(G=0) == 0 and prior(G=0) == 0
    shape = [dict(N=0), dict(N=-1), dict(N=1 << 31), dict(D=0), dict(D=1025), dict(G=-1), dict(N=(1 << 31) - 1, D=1024)]
    for bad in shape + [dict(x=None), dict(seg=None), dict(kind=2), dict(kind=-1)]:
        assert probe(**bad) == -1, bad
    for bad in shape + [dict(acc=None), dict(p=None), dict(x=None), dict(ptr=None), dict(times=None), dict(cells=None), dict(stage=3),
                        dict(stage=-1), dict(scale=0.0), dict(scale=-1.0), dict(n_times=1), dict(b1=0.05), dict(b0=-1.0)]:
        assert div(**bad) == -1, bad
    for bad in shape + [dict(acc=None), dict(x=None), dict(ptr=None)]:
        assert prior(**bad) == -1, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the step kernels on the ascending table: h > 0, under the bounds of tests/test_gpu_ode_kernels.py
# ---------------------------------------------------------------------------------------------------------------------
def _euler_reference(x, raw, n, k, ulp):
    d1 = _drift_ev(raw[:n], ASC[k], ulp)
    hs = EV(f64(ASC[k + 1])) - EV(f64(ASC[k]))
    return fma(hs, d1, EV(x[:n].astype(f64))).pair(), d1.pair()


def _heun_reference(x0, d1, raw2, n, k, ulp):
    d2 = _drift_ev(raw2[:n], ASC[k + 1], ulp)
    hs = EV(f64(ASC[k + 1])) - EV(f64(ASC[k]))
    return fma(EV(0.5) * hs, EV(d1[:n].astype(f64)) + d2, EV(x0[:n].astype(f64))).pair()


@pytest.mark.parametrize("case", [(65, 3, 19, 3), (257, 1, 0, 1), (1025, 3, 19, 3)], ids=lambda c: "N%d_D%d_ghost%d_G%d" % c)
def test_step_kernels_on_the_ascending_table(dev, case):
    n, d, ghost, g = case
    rng = np.random.default_rng(3 * n + d)
    x, raw, seg, _, _ = _case(n, d, ghost, g, rng)
    d1 = rng.standard_normal(x.shape).astype(f32)
    ulp = _expm1_ulp(dev, ASC, case)
    worst = 0.0
    for k in (0, 2, len(ASC) - 2):
        (want, bound), (want_d, bound_d) = _euler_reference(x, raw, n, k, ulp)
        got, got_d, t_out = _call_euler(dev, x, raw, seg, g, k, g1=g + 1, times=ASC)
        err, err_d = np.abs(got[:n].astype(f64) - want), np.abs(got_d[:n].astype(f64) - want_d)
        assert np.isfinite(got).all() and (err <= bound).all() and (err_d <= bound_d).all(), (k, (err / bound).max())
        assert _same(got[n:], x[n:]) and (got_d[n:] == 0).all() and (t_out == ASC[k + 1]).all()
        # h > 0: the state moves WITH the drift (the sampler's table moves it against)
        assert (np.sign(got[:n].astype(f64) - x[:n]) * np.sign(want_d) >= 0).all()
        want_h, bound_h = _heun_reference(x, d1, raw, n, k, ulp)
        got_h = _call_heun(dev, x, d1, raw, seg, g, k, times=ASC)
        err_h = np.abs(got_h[:n].astype(f64) - want_h)
        assert (err_h <= bound_h).all() and _same(got_h[n:], x[n:]), (k, (err_h / bound_h).max())
        worst = max(worst, float((err / bound).max()), float((err_d / bound_d).max()), float((err_h / bound_h).max()))
    for k in (-1, len(ASC) - 1):
        got, got_d, t_out = _call_euler(dev, x, raw, seg, g, k, g1=g + 1, times=ASC)
        assert _same(got, x) and (got_d == 0).all() and _same(_call_heun(dev, x, d1, raw, seg, g, k, times=ASC), x)
    record_measured("test_gpu_likelihood_kernels", case="ascending_N%d_D%d_ghost%d_G%d" % case, worst=worst)


def test_begin_step_walks_the_ascending_table(dev):
    L, lib = _lib()
    times = torch.from_numpy(ASC).to(dev)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    t = torch.full((6,), NAN, device=dev)
    n_steps = len(ASC) - 1      # (the loop hands the header the first n_steps entries)
    for k in range(n_steps + 2):
        assert lib.e3k_sampler_begin_step(L.ptr(times), n_steps, L.ptr(cells), t.data_ptr() + 4, 4, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        host = t.cpu().numpy()
        assert np.isnan(host[0]) and np.isnan(host[-1])
        if k < n_steps:
            assert cells.tolist() == [k + 1, k] and (host[1:-1] == ASC[k]).all()
        else:      # past the schedule: stands still
            assert cells.tolist() == [n_steps, n_steps - 1] and (host[1:-1] == ASC[n_steps - 1]).all()
