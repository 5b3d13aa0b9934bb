"""The conditional sampler's kernels (csrc/e3k_sampler.hip: e3k_sampler_langevin_fixed, e3k_sampler_reverse_em_fixed) called through
the C ABI on canaried buffers and held to float64, element by element, with the machinery of tests/test_gpu_sampler_kernels.py.

  * A FREE real row is the unconditioned update: it stays within langevin_reference / reverse_reference's bound, unchanged.
  * A FIXED real row is fmaf(m, x0, s z): t is planted and exact, lm = t fma(q, t, h) carries its two roundings, m = expf(lm) is within
    exp(lm) D(lm) + 2 u ULP_EXP m with ULP_EXP the device's expf measured on the case's own t grid (_measure_exp_ulps, asserted <= 3),
    s is _std_ev's, z is within XI_BOUND of normal_draw(..., float64) at the words word_fixed + c, the product s z rounds once and the
    FMA once (EV's fma).
  * The Langevin norms are those of the unconditioned entry point on the same inputs, bit for bit (phase 1 is the same code over all
    real rows, whatever the mask), and so is the whole output under an all-zero mask.
  * Ghost rows (segment G) are compared bit for bit with their mask bytes SET."""
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_node_matrix import EV, fma
from tests.test_gpu_sampler_kernels import (BETA_0, BETA_1, CANARY, N_ALPHA, N_SDE, PLANTED_T, SEED, SNR, STEP, T_END, U, _call_langevin,
                                            _call_reverse, _case, _draws, _lib, _rows, _std_ev, f32, f64, langevin_reference,
                                            reverse_reference)
from tests.test_gpu_score_kernels import _measure_exp_ulps
from tests.util import record_measured

pytestmark = pytest.mark.gpu

BYTE_CANARY = 0xA5


def _ulps(dev, t32):
    exp_ulp, m1_ulp = _measure_exp_ulps(dev, t32.astype(f64))
    assert exp_ulp <= 3 and m1_ulp <= 3, (exp_ulp, m1_ulp)      # (3: the OpenCL full-profile limit of both)
    return max(1, math.ceil(exp_ulp)), max(1, math.ceil(m1_ulp))


def _mean_ev(t32, ulp_exp):
    """m(t) = expf(lm) per graph as an EV: lm as _std_ev forms it, exp's own condition and the measured ulp"""
    dbeta = f32(BETA_1) - f32(BETA_0)
    q, h = f32(-0.25) * dbeta, f32(-0.5) * f32(BETA_0)
    t = EV(t32.astype(f64))
    lm = t * fma(float(q), t, float(h))
    m = np.exp(lm.v)
    return EV(m, m * lm.e + 2.0 * U * ulp_exp * m)


def fixed_reference(known, seg, t32, n, word_fixed, ulp_exp, ulp_expm1):
    """(value, bound) of fma(m, x0, s z) over the real rows"""
    s_g, _ = _std_ev(t32, ulp_expm1)
    sg = seg[:n]
    m, s = _rows(_mean_ev(t32, ulp_exp), sg), _rows(s_g, sg)
    z = _draws(n, known.shape[1], STEP, word_fixed)
    return fma(m, EV(known[:n].astype(f64)), s * z).pair()


def _patterns(n, ghost):
    """(name, mask uint8 [n + ghost]); the ghost rows' bytes are set in every pattern: they must not matter"""
    out = [("none", np.zeros(n, np.uint8)), ("all", np.ones(n, np.uint8))]
    if n > 1:
        out.append(("alternating", (np.arange(n) % 2 == 0).astype(np.uint8)))
        last = np.zeros(n, np.uint8)
        last[n - 1] = 1
        out.append(("last", last))
    if n >= 1028:
        stride = np.zeros(n, np.uint8)
        stride[1020:1028] = 1      # across the 1024 rows one pass of the Langevin workgroup covers
        out.append(("stride", stride))
    for name, m in out[2:]:
        assert m.any() and not m.all(), name
    return [(name, np.concatenate([m, np.full(ghost, 1 + i, np.uint8)])) for i, (name, m) in enumerate(out)]


def _planted(dev, host, canary):
    """a device buffer with one canary element at each end around ``host`` (flattened)"""
    flat = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
    buf = torch.full((flat.numel() + 2,), canary, dtype=flat.dtype, device=dev)
    buf[1:-1] = flat.to(dev)
    return buf


def _intact(buf, host, canary):
    got = buf.cpu().numpy()
    assert got[0] == canary and got[-1] == canary
    assert np.array_equal(got[1:-1].view(np.uint8), np.ascontiguousarray(host).reshape(-1).view(np.uint8))      # read only


def _call_fixed(dev, kind, x, raw, known, mask, seg, t, alphas, g, word0, word_fixed, alias):
    """either FIXED entry point -> (x' [n_all, d], norms [2] or None); every buffer canaried, every input checked unchanged"""
    L, lib = _lib()
    n_all, d = x.shape
    c = f32(CANARY)
    xb = _planted(dev, x, CANARY)
    ob = xb if alias else torch.full((n_all * d + 2,), CANARY, device=dev)
    kb, mb, rb = _planted(dev, known, CANARY), _planted(dev, mask, BYTE_CANARY), _planted(dev, raw, CANARY)
    sb, tb, ab = _planted(dev, seg, -99), _planted(dev, t, CANARY), _planted(dev, alphas, CANARY)
    nb = torch.full((4,), CANARY, device=dev)
    cells = torch.tensor([STEP + 1, STEP], dtype=torch.int64, device=dev)
    if kind == "langevin":
        rc = lib.e3k_sampler_langevin_fixed(ob.data_ptr() + 4, xb.data_ptr() + 4, rb.data_ptr() + 4, kb.data_ptr() + 4, mb.data_ptr() + 1,
                                            sb.data_ptr() + 8, tb.data_ptr() + 4, ab.data_ptr() + 4, n_all, d, g, N_ALPHA, BETA_0, BETA_1,
                                            T_END, SNR, SEED & 0xFFFFFFFF, SEED >> 32, L.ptr(cells), word0, word_fixed, nb.data_ptr() + 4,
                                            L.stream_ptr())
    else:
        rc = lib.e3k_sampler_reverse_em_fixed(ob.data_ptr() + 4, xb.data_ptr() + 4, rb.data_ptr() + 4, kb.data_ptr() + 4, mb.data_ptr() + 1,
                                              sb.data_ptr() + 8, tb.data_ptr() + 4, n_all, d, g, BETA_0, BETA_1, N_SDE, SEED & 0xFFFFFFFF,
                                              SEED >> 32, L.ptr(cells), word0, word_fixed, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [STEP + 1, STEP]
    for buf, host, canary in ((kb, known, c), (mb, mask, BYTE_CANARY), (rb, raw, c), (sb, seg, -99), (tb, t, c), (ab, alphas, c)):
        _intact(buf, host, canary)
    if not alias:
        _intact(xb, x, c)
    out, norms = ob.cpu().numpy(), nb.cpu().numpy()
    assert out[0] == c and out[-1] == c and norms[0] == c and norms[-1] == c
    if kind == "langevin":
        return out[1:-1].reshape(n_all, d), norms[1:-1]
    assert (norms == c).all()
    return out[1:-1].reshape(n_all, d), None


def _bits(a):
    return a.view(np.int32)


CASES = [(n, d, ghost, g, word0) for n in (1, 63, 64, 65, 1023, 1025, 2049) for d in (1, 3) for ghost in (0, 19) for g, word0 in ((1, 0), (3, 3))]


@pytest.mark.parametrize("kind", ["langevin", "reverse_em"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_D%d_ghost%d_G%d_word%d" % c)
def test_fixed_kernels_against_float64(dev, case, kind):
    n, d, ghost, g, word0 = case
    rng = np.random.default_rng(300 * n + 10 * d + g + word0 + (1 if kind == "langevin" else 2))
    x, raw, seg, t, alphas = _case(n, d, ghost, g, rng, first_t=(n + d + ghost) % len(PLANTED_T))
    known = rng.standard_normal(x.shape).astype(f32)
    total = word0 + d                                    # (the key is the layout's last: D_total = its first word + its width)
    ulp_exp, ulp_m1 = _ulps(dev, t[:g])
    if kind == "langevin":
        w_update, w_fixed = word0, 2 * total + word0
        (want, bound), _, _ = langevin_reference(x, raw, seg, t, alphas, n, w_update, ulp_m1)
        plain, plain_norms = _call_langevin(dev, x, raw, seg, t, alphas, g, w_update, alias=False)
    else:
        w_update, w_fixed = total + word0, 3 * total + word0
        want, bound = reverse_reference(x, raw, seg, t, n, w_update, ulp_m1)
        plain, plain_norms = _call_reverse(dev, x, raw, seg, t, g, w_update, alias=False), None
    want_f, bound_f = fixed_reference(known, seg, t, n, w_fixed, ulp_exp, ulp_m1)
    worst_free = worst_fixed = 0.0
    for name, mask in _patterns(n, ghost):
        got, norms = _call_fixed(dev, kind, x, raw, known, mask, seg, t, alphas, g, w_update, w_fixed, alias=False)
        rows = mask[:n].astype(bool)
        assert np.isfinite(got).all()
        err = np.abs(got[:n].astype(f64) - want)
        assert (err[~rows] <= bound[~rows]).all(), (name, (err[~rows] / bound[~rows]).max())
        err_f = np.abs(got[:n].astype(f64) - want_f)
        assert (err_f[rows] <= bound_f[rows]).all(), (name, (err_f[rows] / bound_f[rows]).max())
        # a free row is the unconditioned entry point's, bit for bit; a fixed one is not (its noise is another block's)
        assert np.array_equal(_bits(got[:n][~rows]), _bits(plain[:n][~rows])), name
        assert (got[:n][rows] != plain[:n][rows]).all(), name
        assert np.array_equal(_bits(got[n:]), _bits(x[n:])), name                           # ghost rows, mask bytes set: bit for bit
        if kind == "langevin":
            assert np.array_equal(_bits(norms), _bits(plain_norms)), (name, norms, plain_norms)
        if name == "none":
            assert np.array_equal(_bits(got), _bits(plain))
        again, norms2 = _call_fixed(dev, kind, x, raw, known, mask, seg, t, alphas, g, w_update, w_fixed, alias=False)
        aliased, norms3 = _call_fixed(dev, kind, x, raw, known, mask, seg, t, alphas, g, w_update, w_fixed, alias=True)
        assert np.array_equal(_bits(again), _bits(got)) and np.array_equal(_bits(aliased), _bits(got)), name
        if kind == "langevin":
            assert np.array_equal(_bits(norms2), _bits(norms)) and np.array_equal(_bits(norms3), _bits(norms)), name
        if (~rows).any():
            worst_free = max(worst_free, float((err[~rows] / bound[~rows]).max()))
        if rows.any():
            worst_fixed = max(worst_fixed, float((err_f[rows] / bound_f[rows]).max()))
    print(f"{kind}_fixed {case}: worst error / bound free {worst_free:.3f}, fixed {worst_fixed:.3f}, expf {ulp_exp} ulp, expm1f {ulp_m1} ulp")
    record_measured("test_gpu_sampler_fixed_kernels", case=kind + "_N%d_D%d_ghost%d_G%d_word%d" % case, worst_free=worst_free,
                    worst_fixed=worst_fixed)


def test_the_replacement_reads_its_own_words_and_the_known_values(dev):
    """x0 = 0 leaves s z behind: the replacement's z itself, read back at the words word_fixed + c; z = ... cannot be switched off, so
    the known values are checked through the difference of two calls: m (x0 - x0')."""
    n, d = 65, 3
    rng = np.random.default_rng(8)
    x, raw, seg, t, alphas = _case(n, d, 0, 1, rng)
    mask = np.ones(n, np.uint8)
    zero = np.zeros_like(x)
    ulp_exp, ulp_m1 = _ulps(dev, t[:1])
    s, m = _std_ev(t[:1], ulp_m1)[0], _mean_ev(t[:1], ulp_exp)
    for kind, w_update, w_fixed in (("langevin", 0, 6), ("reverse_em", 3, 9)):
        got, _ = _call_fixed(dev, kind, x, raw, zero, mask, seg, t, alphas, 1, w_update, w_fixed, alias=False)
        for words, same in ((w_fixed, True), (w_update, False), (w_fixed - 3, False)):
            z = _draws(n, d, STEP, words)
            close = np.abs(got.astype(f64) / s.v[0] - z.v) <= z.e + (s.e[0] / s.v[0] + 4 * U) * np.abs(z.v)
            assert close.all() if same else not close.any(), (kind, words)
        known = rng.standard_normal(x.shape).astype(f32)
        moved, _ = _call_fixed(dev, kind, x, raw, known, mask, seg, t, alphas, 1, w_update, w_fixed, alias=False)
        diff = moved.astype(f64) - got.astype(f64)
        assert (np.abs(diff - m.v[0] * known) <= m.e[0] * np.abs(known) + 4 * U * (np.abs(moved) + np.abs(got))).all(), kind


def test_the_fixed_entry_points_refuse_bad_arguments(dev):
    L, lib = _lib()
    x, raw, known = torch.zeros(4, 3, device=dev), torch.ones(4, 3, device=dev), torch.ones(4, 3, device=dev)
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    mask = torch.ones(4, dtype=torch.uint8, device=dev)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    t, alphas, norms = torch.full((2,), 0.5, device=dev), torch.full((5,), 0.9, device=dev), torch.full((2,), CANARY, device=dev)
    out = torch.full((4, 3), CANARY, device=dev)
    ok = dict(out=L.ptr(out), x=L.ptr(x), raw=L.ptr(raw), known=L.ptr(known), fixed=L.ptr(mask), seg=L.ptr(seg), t=L.ptr(t),
              alphas=L.ptr(alphas), N=4, D=3, G=1, n_alpha=5, b0=0.1, b1=20.0, T=1.0, snr=0.16, cells=L.ptr(cells), norms=L.ptr(norms),
              n_sde=1000)

    def langevin(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_langevin_fixed(a["out"], a["x"], a["raw"], a["known"], a["fixed"], a["seg"], a["t"], a["alphas"], a["N"], a["D"],
                                              a["G"], a["n_alpha"], a["b0"], a["b1"], a["T"], a["snr"], 1, 2, a["cells"], 0, 6, a["norms"],
                                              L.stream_ptr())

    def reverse(**over):
        a = dict(ok, **over)
        return lib.e3k_sampler_reverse_em_fixed(a["out"], a["x"], a["raw"], a["known"], a["fixed"], a["seg"], a["t"], a["N"], a["D"], a["G"],
                                                a["b0"], a["b1"], a["n_sde"], 1, 2, a["cells"], 3, 9, L.stream_ptr())

    both = [dict(known=None), dict(fixed=None), dict(out=L.ptr(known)), dict(out=None), dict(x=None), dict(raw=None), dict(seg=None),
            dict(t=None), dict(cells=None), dict(N=0), dict(N=-1), dict(D=0), dict(D=1025), dict(G=-1), dict(b1=0.05), dict(b0=-1.0)]
    for bad in both + [dict(alphas=None), dict(norms=None), dict(n_alpha=0), dict(T=0.0), dict(snr=0.0), dict(G=0)]:
        assert langevin(**bad) == -1, bad
    for bad in both + [dict(n_sde=0)]:
        assert reverse(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (norms == CANARY).all() and (known == 1.0).all()      # nothing was launched
    assert langevin() == 0 and reverse() == 0 and langevin(out=L.ptr(x)) == 0               # ... and x_out may be x
    torch.cuda.synchronize()


def test_the_fixed_wrappers_refuse_what_their_siblings_refuse(dev):
    from e3_layers_amd.backend import diffusion_ops

    x, raw, known = torch.zeros(4, 3, device=dev), torch.ones(4, 3, device=dev), torch.full((4, 3), 2.0, device=dev)
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    mask = torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device=dev)
    t, alphas = torch.full((1, 1), 0.5, device=dev), torch.full((5,), 0.9, device=dev)
    cells = torch.zeros(2, dtype=torch.int64, device=dev)
    lang = lambda **o: diffusion_ops.sampler_langevin(*[o.get(k, v) for k, v in dict(x=x, raw=raw, seg=seg, t=t, alphas=alphas).items()],  # noqa: E731
                                                      1, 0.1, 20.0, 1.0, 0.16, 7, o.get("cells", cells), 0, out=o.get("out"),
                                                      known=o.get("known", known), fixed=o.get("fixed", mask), word_fixed=6)
    rev = lambda **o: diffusion_ops.sampler_reverse_em(*[o.get(k, v) for k, v in dict(x=x, raw=raw, seg=seg, t=t).items()],  # noqa: E731
                                                       1, 0.1, 20.0, 1000, 7, o.get("cells", cells), 3, out=o.get("out"),
                                                       known=o.get("known", known), fixed=o.get("fixed", mask), word_fixed=9)
    out, norms = lang()
    plain, plain_norms = diffusion_ops.sampler_langevin(x, raw, seg, t, alphas, 1, 0.1, 20.0, 1.0, 0.16, 7, cells, 0)
    assert torch.equal(out[1:3], plain[1:3]) and torch.equal(norms, plain_norms) and (out[0] != plain[0]).all()
    assert rev(out=x) is x
    for call in (lang, rev):
        with pytest.raises(RuntimeError):
            call(known=known.cpu())                                        # no CPU fallback
        with pytest.raises(RuntimeError):
            call(fixed=mask.cpu())
        with pytest.raises(ValueError, match="uint8"):
            call(fixed=mask.bool())
        with pytest.raises(ValueError, match="uint8"):
            call(fixed=mask[:3])
        with pytest.raises(ValueError, match="uint8"):
            call(fixed=torch.ones(8, dtype=torch.uint8, device=dev)[::2])
        with pytest.raises(ValueError, match="known"):
            call(known=known[:, :2])
        with pytest.raises(ValueError, match="known"):
            call(out=known)
        with pytest.raises(ValueError, match="cells"):
            call(cells=cells[:1])
