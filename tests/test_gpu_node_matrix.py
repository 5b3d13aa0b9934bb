"""The node-side kernels of csrc/e3k_node.hip that tests/test_gpu_node_passes.py does not cover, every one against float64 on the CPU,
element by element: activations (and their two derivatives), NormActivation, the per-block RMS normalisation, sorted-segment sum,
relayout, one-hot rows, counts -> row pointers, the keyed self-connection weights with their multi-layer forms, and the double backward
of the Gate (its forward and first backward are held in tests/test_gpu_node_passes.py, whose segment tables these cases reuse).

``CASES`` is a plain table.  Each case makes C-ABI calls through backend/lib.py on buffers inside a NaN-filled arena with slack round
every buffer (the arena of tests/test_gpu_rtable_matrix.py, filled with NaN instead of random words), claims every word a call may
write with exactly one comparison and requires every other word of the arena to keep its bits.  tests/test_node_inventory.py holds the
table to the kernels the library ships and to the functions include/e3k.h declares, shows on the CPU that float32 models of the kernels
stay inside the bounds below, and that the bounds are sharp (planted mutants).  The input, reference and bound builders below run
without a GPU.

Bounds.  Per element, by running error analysis: ``EV`` carries a float64 value v and a bound e on |computed - v|, and every operation
of a kernel is replayed on it.  With u = 2^-24 and UR = u + 2^-52 (the float64 replay's own rounding),
    a + b:      e_a + e_b + UR |a + b|                      a * b:  |a| e_b + |b| e_a + e_a e_b + UR |a b|
    fma(a,b,c): |a| e_b + |b| e_a + e_a e_b + e_c + UR |a b + c|      (a contracted a * b + c errs by no more than the separate form)
    a / b:      (e_a + |a / b| e_b) / (|b| - e_b) + UR |a / b|        sqrt(a): e_a / (sqrt(a - e_a) + sqrt(a)) + UR sqrt(a)
(division and square root are correctly rounded: the library is built without fast-math flags), plus 2^-126 per operation for a
result that is flushed below the normal range.  A result that cancels therefore carries an ABSOLUTE bound by construction: ssp near 0,
act_bwd_from_output for negative x, s1 = (a' n - a) / n^2 of NormActivation at small n, the second-derivative coefficients of the
normalisation.  Primitives, as in the docstring of tests/test_gpu_node_passes.py:
    sigmoid(x) = rcp(1 + exp(-x)) on hardware transcendentals, tanhf:   relative E(x) = (1.5 |x| + 6) u
    precise expf (act_bwd_from_output):                                   2 ulp relative
    ssp(x) = max(x, 0) + log(1 + exp(-|x|)) - ln 2:  the exponential moves the logarithm's argument by at most 2u, the sum 1 + e
        by u, v_log_f32 of an argument in [1, 2] and its product with ln 2 err by 2u absolute, the two sums by u (|x| + 0.7) and
        u |y|, the constant ln 2 in fp32 by u:  ABSOLUTE (2 |x| + 8) u
  a primitive of an argument that itself carries e_x adds |f'(x)| e_x + c e_x^2 (c bounds |f''| / 2).
act'(x) replayed this way has the form of that docstring's D(x) = (2 x^2 + 10 |x| + 10) u: absolute, quadratic in |x|.
Sums that waves, LDS partials or atomics reduce in an order the test does not know get the order-independent
    gamma_n sum |terms|,  gamma_n = n u / (1 - n u),  n = the number of terms (the old value of an ACCUMULATED output counts as one):
any order of n - 1 additions of once-rounded products is inside it.  The sums are: sum x^2 over dim (NormActivation), over a block
(normalisation: 64 lanes, wave reduction), g_std over rows (registers, LDS, atomics), a segment's rows, V attributes (keyed forward),
K keys (g_W: tiles of 64 or 512, atomics between tiles) and all the columns (g_a: LDS chunks of 256, workspace rows, one wave).

Exact cases.  Keyed weights with a, W, g_M integers in [-4, 4] and the segment sum of integer rows are exact in fp32 in any order:
compared with ==, they catch any indexing error without a bound.  Relayout, one-hot and counts -> ptr are bit-exact anyway.

Uncovered columns.  NormActivation's three kernels store zero in a column no block covers (normact_bwd2_kernel stored nothing there
before these cases: na_bwd2_gap, na_bwd2_only_ggy and na_bwd2_only_gx read NaN in 30 of 125 outputs; fixed in csrc/e3k_node.hip).  The three normalisation kernels write the block columns only -- they walk blocks,
one wave per row, and a zero store would be a further pass over the row -- which include/e3k.h now says for all three; the gap
cases pin both: zero there, NaN (as handed over) here.

NormActivation on clamped channels and just above the clamp: s = act(n) / n and its slopes divide an absolute error of act by n, n^2,
n^3.  tests/test_gpu_ops.py::test_norm_activation leaves the clamped channels out; here NOTHING is left out: the bound says what fp32
resolves there (it is large on those channels only: tests/test_node_inventory.py shows that every element bound above 1e-4 lies in
a channel of norm below 0.5, and that the clamped channels are among the planted ones).

act_bwd_from_output computes 1 - 0.5 exp(-y / cst), which cancels for x below about -10 and may come out slightly negative.  Its
absolute bound (about 3.4 u |g_y| cst there) holds on the GPU against its own formula AND against g_y cst sigmoid(x) with the
conditioning term u |y| |g_y| added: inside the bound, not a defect; the factor is not clamped.

Worst error / bound per family on an MI355X (a record, not a threshold; printed by test_zz_worst_ratio_per_family): see MEASURED
below -- 0.48 .. 0.88 for the elementwise families (the float32 models of tests/test_node_inventory.py measure the same on the CPU),
0.98 for the keyed forward, 0.006 .. 0.21 for the keyed backward's long order-independent sums.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_node_passes import SPECS as GATE_SPECS, _out_view, _seg_array
from tests.test_gpu_rtable_matrix import Arena as _Arena, Check as _Check
from tests.util import record_measured

pytestmark = pytest.mark.gpu

# worst error / bound per family as printed by a full run on an MI355X
MEASURED = {
    "act_fwd": 0.640, "act_bwd": 0.499, "act_bwd2": 0.633, "act_out": 0.816, "act_out_from_x": 0.531,
    "gate_bwd2_g_gy": 0.483, "gate_bwd2_g_x": 0.480,
    "norm_act_fwd": 0.774, "norm_act_bwd": 0.656, "norm_act_bwd2": 0.652,
    "layernorm_fwd": 0.524, "layernorm_bwd": 0.719, "layernorm_bwd2": 0.876,
    "segment_sum": 0.498,
    # one FMA per output at V = 1: a single rounding against gamma_1 = u
    "keyed_weights_fwd": 0.976, "keyed_weights_multi_M": 0.774,
    # order-independent bounds over K + 1 and over (all columns) + 1 terms: far from attained by sums of random signs
    "keyed_weights_bwd_g_W": 0.214, "keyed_weights_multi_g_W": 0.187, "keyed_weights_bwd_g_a": 0.013, "keyed_weights_multi_g_a": 0.006,
}

E3K_OK, E3K_ERR_INVALID, E3K_ERR_UNSUPPORTED = 0, -1, -3
U = 2.0 ** -24
UR = U + 2.0 ** -52
FL = 2.0 ** -126
f32 = np.float32
NANF = np.float32(np.nan)
C1, C2, C3, C4 = 1.8, 1.6791767923989418, 1.1501944455736173, 1.5925374197228312
GRID_CAP = 8192 * 256      # elements one pass of a grid_for launch covers


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------------------------
# running error analysis
class EV:
    """float64 value v and a bound e on |fp32 result - v| (see the module docstring)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def of(x):
        return x if isinstance(x, EV) else EV(x)

    @staticmethod
    def _r(v, e):
        return EV(v, e + UR * np.abs(v) + FL)

    def __add__(self, o):
        o = EV.of(o)
        return EV._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = EV.of(o)
        return EV._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return EV.of(o) - self

    def __neg__(self):
        return EV(-self.v, self.e)

    def __mul__(self, o):
        o = EV.of(o)
        return EV._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = EV.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            den = np.abs(o.v) - o.e
            e = np.where(den > 0, (self.e + np.abs(v) * o.e) / np.where(den > 0, den, 1.0), np.inf)
        return EV._r(v, e)

    def __rtruediv__(self, o):
        return EV.of(o) / self

    def abs(self):
        return EV(np.abs(self.v), self.e)

    def sqrt(self):
        v = np.sqrt(self.v)
        lo = np.sqrt(np.maximum(self.v - self.e, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(lo + v > 0, self.e / np.where(lo + v > 0, lo + v, 1.0), np.sqrt(self.e))
        return EV._r(v, e)

    def pair(self, shape=None):
        v, e = (self.v, self.e) if shape is None else (np.broadcast_to(self.v, shape), np.broadcast_to(self.e, shape))
        return np.array(v), np.array(e)


def fma(a, b, c):
    a, b, c = EV.of(a), EV.of(b), EV.of(c)
    return EV._r(a.v * b.v + c.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + c.e)


def where(cond, a, b):
    a, b = EV.of(a), EV.of(b)
    return EV(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))


def dot_ev(a, b, axis, extra_terms=0):
    """sum over `axis` of a * b in any order: the inputs' own errors, and gamma_n sum |a b| for the n roundings"""
    a, b = EV.of(a), EV.of(b)
    p = a.v * b.v
    n = p.shape[axis]
    carried = np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e
    return EV(p.sum(axis), carried.sum(axis) + (gamma(n + extra_terms) + 2.0 ** -52 * n) * np.abs(p).sum(axis) + FL)


def sum_ev(t, axis, extra=None):
    """sum of already formed terms in any order (plus one more term `extra`, the old value of an accumulated output)"""
    t = EV.of(t)
    n = t.v.shape[axis] + (0 if extra is None else 1)
    v, e, a = t.v.sum(axis), t.e.sum(axis), np.abs(t.v).sum(axis)
    if extra is not None:
        v, a = v + extra, a + np.abs(extra)
    return EV(v, e + (gamma(n) + 2.0 ** -52 * n) * a + FL)


def E_(x):
    return (1.5 * np.abs(x) + 6.0) * U


def err_dact_doc(x):
    """D(x) of tests/test_gpu_node_passes.py"""
    return (2.0 * x * x + 10.0 * np.abs(x) + 10.0) * U


def sig_ev(x):
    x = EV.of(x)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x.v))
    return EV(s, E_(x.v) * s + s * (1.0 - s) * x.e + 0.1 * x.e ** 2 + FL)


def tanh_ev(x):
    x = EV.of(x)
    th = np.tanh(x.v)
    return EV(th, E_(x.v) * np.abs(th) + (1.0 - th * th) * x.e + 0.8 * x.e ** 2 + FL)


def exp_ev(x, ulps=2):
    x = EV.of(x)
    with np.errstate(over="ignore"):
        v = np.exp(x.v)
    return EV(v, v * (ulps * U + x.e + x.e ** 2) + FL)


def ssp64(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))) - np.log(2.0)


def sign_ev(x):
    return EV(np.sign(EV.of(x).v))


def act_ev(a, x, mutant=None):
    x = EV.of(x)
    if a == 1:
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-x.v))
        return EV(ssp64(x.v), (2.0 * np.abs(x.v) + 8.0) * U + s * x.e + 0.2 * x.e ** 2 + FL)
    if a == 2:
        return x * sig_ev(x)
    if a == 3:
        return tanh_ev(x) * x.abs()
    if a == 4:
        return tanh_ev(x)
    return x.abs() if a == 5 else x


def dact_ev(a, x, mutant=None):
    x = EV.of(x)
    if a == 1:
        return sig_ev(x)
    if a == 2:
        s = sig_ev(x)
        return s * (1.0 + x * (1.0 - s))
    if a == 3:
        th = tanh_ev(x)
        sg = sign_ev(x) if mutant != "tanhlu_sign" else EV(np.where(x.v != 0, 1.0, 0.0))
        return (1.0 - th * th) * x.abs() + th * sg
    if a == 4:
        th = tanh_ev(x)
        return 1.0 - th * th
    return sign_ev(x) if a == 5 else EV(np.ones_like(x.v))


def d2act_ev(a, x, mutant=None):
    x = EV.of(x)
    if a == 1:
        s = sig_ev(x)
        return s * (1.0 - s)
    if a == 2:
        s = sig_ev(x)
        inner = (2.0 + x * (1.0 - 2.0 * s)) if mutant != "silu_d2" else (2.0 + x)
        return s * (1.0 - s) * inner
    if a == 3:
        th = tanh_ev(x)
        return 2.0 * (1.0 - th * th) * (sign_ev(x) - th * x.abs())
    if a == 4:
        th = tanh_ev(x)
        return -2.0 * th * (1.0 - th * th)
    return EV(np.zeros_like(x.v))


# ---------------------------------------------------------------------------------------------------------------------------------
# the table's vocabulary
def _rng(c):
    return np.random.default_rng(zlib.crc32(c["id"].encode()))


def act(id_, why, op, a, n, cst=None, outs="both"):
    cst = {0: 1.0, 1: C1, 2: C2, 3: C3, 4: C4, 5: 1.25}[a] if cst is None else cst
    fn = {"fwd": "e3k_act_fwd", "bwd": "e3k_act_bwd", "bwd2": "e3k_act_bwd2", "out": "e3k_act_bwd_from_output"}[op]
    k = {"fwd": "act_fwd_kernel", "bwd": "act_bwd_kernel", "bwd2": "act_bwd2_kernel", "out": "act_bwd_out_kernel"}[op]
    return dict(id=id_, kind="act", why=why, op=op, act=a, n=n, cst=cst, outs=outs, fn=fn, funcs={fn}, kernels={k} if n and outs != "none" else set())


def na(id_, why, op, table, a, rows, eps=1e-4, normalize=1, outs="both"):
    fn = {"fwd": "e3k_norm_act_fwd", "bwd": "e3k_norm_act_bwd", "bwd2": "e3k_norm_act_bwd2"}[op]
    k = {"fwd": "normact_fwd_kernel", "bwd": "normact_bwd_kernel", "bwd2": "normact_bwd2_kernel"}[op]
    return dict(id=id_, kind="na", why=why, op=op, table=table, act=a, rows=rows, eps=eps, normalize=normalize, outs=outs, fn=fn, funcs={fn},
                kernels={k} if rows else set())


def ln(id_, why, op, table, rows, hs=True, outs="gxs"):
    fn = {"fwd": "e3k_layernorm_fwd", "bwd": "e3k_layernorm_bwd", "bwd2": "e3k_layernorm_bwd2"}[op]
    k = {"fwd": "layernorm_fwd_kernel", "bwd": "layernorm_bwd_kernel", "bwd2": "layernorm_bwd2_kernel"}[op]
    return dict(id=id_, kind="ln", why=why, op=op, table=table, rows=rows, hs=hs, outs=outs, fn=fn, funcs={fn}, kernels={k} if rows else set())


def seg(id_, why, sizes, dim, mean, exact=False):
    return dict(id=id_, kind="seg", why=why, sizes=list(sizes), dim=dim, mean=mean, exact=exact, fn="e3k_segment_sum", funcs={"e3k_segment_sum"},
                kernels={"segment_sum_kernel"} if len(sizes) else set())


def rl(id_, why, table, rows):
    return dict(id=id_, kind="rl", why=why, table=table, rows=rows, fn="e3k_relayout", funcs={"e3k_relayout"}, kernels={"relayout_kernel"})


def c2p(id_, why, G, zero=False):
    return dict(id=id_, kind="c2p", why=why, G=G, zero=zero, fn="e3k_counts_to_ptr", funcs={"e3k_counts_to_ptr"}, kernels={"counts_to_ptr_kernel"})


def oh(id_, why, rows, T, bad=(), flag=0, with_flag=True):
    return dict(id=id_, kind="oh", why=why, rows=rows, T=T, bad=list(bad), flag=flag, with_flag=with_flag, fn="e3k_onehot", funcs={"e3k_onehot"},
                kernels={"onehot_kernel"} if rows else set())


def kw(id_, why, op, instr, K, V, pad=0, exact=False, acc=0, outs="aw"):
    """instr: [(u, w_out)]; op fwd / bwd; outs: which of g_a ('a') and g_W ('w') the backward is asked for"""
    total = sum(u * w for u, w in instr)
    cb = (total + 255) // 256
    tiles = -(-K // (512 if cb >= 1024 else 64))
    if op == "fwd":
        fn, kernels = "e3k_keyed_weights_fwd", {"keyed_weights_kernel<0>"}
    else:
        fn, kernels = "e3k_keyed_weights_bwd", set()
        if "w" in outs:
            kernels |= {"keyed_weights_kernel<1>"} | ({"zero_words_kernel"} if tiles > 1 and not acc else set())
        if "a" in outs:
            kernels |= {"keyed_weights_bwd_a_kernel", "keyed_weights_bwd_a_reduce_kernel"}
    funcs = {fn} | ({"e3k_keyed_weights_bwd_workspace"} if op == "bwd" else set())
    return dict(id=id_, kind="kw", why=why, op=op, instr=list(instr), K=K, V=V, pad=pad, exact=exact, acc=acc, outs=outs, total=total, tiles=tiles,
                fn=fn, funcs=funcs, kernels=kernels)


def kwm(id_, why, layers, K, V, exact=False, null_w=None, acc=0):
    """layers: one instruction list per layer, sharing the attribute rows"""
    cb = (max(sum(u * w for u, w in ins) for ins in layers) + 255) // 256 * len(layers)
    tiles = -(-K // (512 if cb >= 1024 else 64))
    kernels = {"keyed_weights_multi_kernel<0>", "keyed_weights_multi_kernel<1>", "keyed_weights_bwd_a_multi_kernel", "keyed_weights_bwd_a_reduce_kernel"}
    if tiles > 1 and not acc:
        kernels |= {"zero_words_kernel"}
    return dict(id=id_, kind="kwm", why=why, layers=[list(l) for l in layers], K=K, V=V, exact=exact, null_w=null_w, acc=acc, tiles=tiles,
                fn="e3k_keyed_weights_fwd_multi", kernels=kernels,
                funcs={"e3k_keyed_weights_fwd_multi", "e3k_keyed_weights_bwd_multi", "e3k_keyed_weights_bwd_multi_workspace", "e3k_kw_args_create",
                       "e3k_kw_args_destroy", "e3k_keyed_weights_fwd", "e3k_keyed_weights_bwd", "e3k_keyed_weights_bwd_workspace"})


def gate2(id_, why, spec, cf, rows, outs="both"):
    kernels = ({"gate_bwd2_gy_kernel"} if outs != "gx" else set()) | ({"gate_bwd2_x_kernel"} if outs != "ggy" else set())
    return dict(id=id_, kind="gate2", why=why, spec=spec, cf=cf, rows=rows, outs=outs, fn="e3k_gate_bwd2", funcs={"e3k_gate_bwd2"},
                kernels=kernels if rows else set())


def refuse(id_, why, fn, rc, **over):
    return dict(id=id_, kind="refuse", why=why, fn="e3k_" + fn, rc=rc, over=over, kernels=set(), funcs={"e3k_" + fn})


# block tables: (off, mul, dim)
def _packed(md, gaps=()):
    out, off = [], 0
    for i, (m, d) in enumerate(md):
        off += dict(gaps).get(i, 0)
        out.append((off, m, d))
        off += m * d
    return out


TABLES = {
    # NormActivation: dim 1, 3, 5, 7 and mul 1, 3, 64
    "na_mixed": dict(blocks=_packed([(64, 1), (3, 3), (1, 5), (3, 7), (64, 3), (1, 1)]), row_dim=292),
    "na_gap": dict(blocks=_packed([(3, 3), (2, 5)], gaps={1: 4}), row_dim=25),      # columns 9..12 and 23..24 belong to no block
    "na_16": dict(blocks=_packed([(2, 3)] * 16), row_dim=96),
    "na_17": dict(blocks=_packed([(2, 3)] * 17), row_dim=102),
    # normalisation: block lengths 1, 63, 64, 65, 200, each with mul != len but the first and third
    "ln_mixed": dict(blocks=_packed([(1, 1), (21, 3), (64, 1), (13, 5), (40, 5)]), row_dim=393),
    "ln_gap": dict(blocks=_packed([(4, 3), (5, 1), (2, 5)], gaps={1: 3, 2: 1}), row_dim=33),      # 12..14, 20 and 31..32 uncovered
    "ln_16": dict(blocks=_packed([(3, 3), (70, 1)] * 8), row_dim=632),
    "ln_17": dict(blocks=_packed([(2, 3)] * 17), row_dim=102),
    # relayout: dim-1 blocks, a gap (copied through), mixed
    "rl_mixed": dict(blocks=_packed([(5, 1), (3, 3), (4, 5), (300, 3), (2, 7)], gaps={2: 3}), row_dim=5 + 9 + 3 + 20 + 900 + 14 + 2),
    "rl_wide": dict(blocks=_packed([(16, 3), (8, 5)]), row_dim=88),
}
ACT_NAMES = {0: "id", 1: "ssp", 2: "silu", 3: "tanhlu", 4: "tanh", 5: "abs"}
BIG_N = GRID_CAP + 257
KW_SMALL = [(3, 5), (2, 7)]                       # total 29
KW_257 = [(16, 8), (3, 43)]                        # total 257: the second instruction starts at column 128, inside the first 256-column block
KW_300 = [(10, 13), (17, 10)]                      # total 300: boundary at 130, different w_out on either side, two column blocks
KW_WIDE = [(512, 512)]                             # total 1024 * 256: 1024 column blocks, the key tile is 512

CASES = []
for _a in range(6):
    CASES += [act(f"act_fwd_{ACT_NAMES[_a]}", "values incl. 0, +-1e-6, a sweep of [-20, 20], +-88, +-104, +-1e4", "fwd", _a, 257),
              act(f"act_bwd_{ACT_NAMES[_a]}", "first derivative on the same values", "bwd", _a, 257),
              act(f"act_bwd2_{ACT_NAMES[_a]}", "second derivative on the same values, both outputs", "bwd2", _a, 257)]
for _n in (0, 1, 255, BIG_N):
    CASES += [act(f"act_fwd_n{_n}", "size: empty, one, under one workgroup, grid-stride wrap", "fwd", 2, _n),
              act(f"act_bwd_n{_n}", "size", "bwd", 3, _n),
              act(f"act_bwd2_n{_n}", "size", "bwd2", 1, _n)]
for _name in sorted(GATE_SPECS):
    for _cf in (0, 1):
        CASES.append(gate2(f"gate2_{_name}_{'cf' if _cf else 'e3nn'}", "the segment tables of the Gate passes: dims 1 3 5 7 9, gaps, segments out of row order",
                           _name, _cf, 7))
CASES += [gate2("gate2_rows0", "no rows", "layer", 1, 0), gate2("gate2_rows1", "one row", "odd_quads", 0, 1),
          gate2("gate2_layer_wrap", "4704 rows: grid.y (8192 / 5 column blocks) strides the rows", "layer", 1, 4704),
          gate2("gate2_only_ggy", "g_x and g_y NULL", "odd_quads", 1, 7, outs="ggy"), gate2("gate2_only_gx", "g_gy NULL", "in_gap", 0, 7, outs="gx")]
CASES += [
    act("act_bwd2_only_ggy", "g_x NULL (and g_y NULL with it)", "bwd2", 2, 257, outs="ggy"),
    act("act_bwd2_only_gx", "g_gy NULL", "bwd2", 3, 257, outs="gx"),
    act("act_bwd2_none", "both outputs NULL: refused", "bwd2", 2, 257, outs="none"),
] + [act(f"act_out_n{_n}", "ssp derivative from the output: own formula on the fp32 y, and against cst sigmoid(x)", "out", 1, _n) for _n in (0, 1, 255, 257, BIG_N)] + [
    act("act_out_cst0.3", "a small constant: -y / cst is scaled up", "out", 1, 257, cst=0.3),
]
for _s, (_eps, _nz) in {"norm": (1e-4, 1), "raw": (1e-4, 0), "sq": (0.0, 1)}.items():
    for _a in range(6):
        for _op in ("fwd", "bwd", "bwd2"):
            CASES.append(na(f"na_{_op}_{_s}_{ACT_NAMES[_a]}", "dims 1 3 5 7, muls 1 3 64; zero, 0.5 eps, 2 eps and 1e-3 channels", _op, "na_mixed", _a, 5, _eps, _nz))
for _op in ("fwd", "bwd", "bwd2"):
    CASES += [na(f"na_{_op}_rows0", "no rows", _op, "na_mixed", 2, 0), na(f"na_{_op}_rows1", "one row", _op, "na_mixed", 1, 1),
              na(f"na_{_op}_wrap", "rows * row_dim beyond 8192 * 256: grid-stride wrap", _op, "na_mixed", 2, 7200),
              na(f"na_{_op}_gap", "columns no block covers come out zero", _op, "na_gap", 2, 5),
              na(f"na_{_op}_16", "16 blocks", _op, "na_16", 3, 3)]
CASES += [na("na_bwd2_only_ggy", "g_x NULL", "bwd2", "na_gap", 2, 5, outs="ggy"), na("na_bwd2_only_gx", "g_gy NULL", "bwd2", "na_gap", 1, 5, outs="gx")]
for _op in ("fwd", "bwd", "bwd2"):
    CASES += [ln(f"ln_{_op}_rows{_r}", "lengths 1 63 64 65 200, mul != len, a zero block; rows round the four-row workgroup and the 512-workgroup cap",
                 _op, "ln_mixed", _r) for _r in (0, 1, 3, 4, 5, 2049)]
    CASES += [ln(f"ln_{_op}_gap", "uncovered columns stay as handed over", _op, "ln_gap", 5), ln(f"ln_{_op}_16", "16 blocks", _op, "ln_16", 7)]
CASES += [ln("ln_bwd2_no_hs", "h_std NULL", "bwd2", "ln_mixed", 5, hs=False),
          ln("ln_bwd2_no_gg", "g_gy NULL", "bwd2", "ln_mixed", 5, outs="xs"), ln("ln_bwd2_no_gx", "g_x NULL", "bwd2", "ln_mixed", 5, outs="gs"),
          ln("ln_bwd2_no_gs", "g_std NULL", "bwd2", "ln_mixed", 5, outs="gx")]
_SIZES = [0, 0, 3, 1, 0, 5000, 7, 0, 0, 2, 64, 0]
for _d in (1, 3, 64, 257):
    CASES += [seg(f"seg_sum_d{_d}", "empty segments first, in the middle and last; one of 5000 rows", _SIZES, _d, 0),
              seg(f"seg_mean_d{_d}", "mean; an empty segment gives 0", _SIZES, _d, 1)]
CASES += [seg("seg_none", "no segments", [], 3, 0), seg("seg_one", "one segment", [9], 3, 1), seg("seg_one_empty", "one empty segment", [0], 5, 1),
          seg("seg_exact", "integer rows: exact in any order", _SIZES, 257, 0, exact=True),
          seg("seg_many", "8200 segments of 257 columns: beyond the grid cap", [1, 0, 2] * 2734, 257, 1, exact=False)]
CASES += [rl(f"rl_mixed_rows{_r}", "dim-1 blocks, a gap, 953 columns: bit-exact both ways and the round trip", "rl_mixed", _r) for _r in (1, 3, 4, 5, 2100)]
CASES += [rl("rl_cap", "one column block: grid.y at its cap of 8192, rows run the four-row loop and its tail", "rl_wide", 8192 * 4 + 8192 * 2 + 5)]
CASES += [c2p(f"c2p_G{_g}", "chunks of 256 with a carry", _g) for _g in (0, 1, 255, 256, 257, 512, 513, 1000)] + [c2p("c2p_zero", "all counts zero", 300, zero=True)]
CASES += [oh("oh_plain", "1234 rows of 7 types", 1234, 7), oh("oh_bad", "an index past the end and a negative one: zero rows, bit 2", 1234, 7, bad=[(17, 7), (900, -1)]),
          oh("oh_T1", "one type", 300, 1), oh("oh_T1_bad", "one type, index 1", 300, 1, bad=[(5, 1)]),
          oh("oh_flag3", "a flag that holds 3 reads 7 afterwards", 50, 4, bad=[(0, -5)], flag=3),
          oh("oh_flag_kept", "no bad index: the flag keeps its 3", 50, 4, flag=3),
          oh("oh_no_flag", "bad_flag NULL", 50, 4, bad=[(3, 9)], with_flag=False), oh("oh_rows0", "no rows", 0, 4),
          oh("oh_wrap", "rows * T beyond the grid cap", GRID_CAP // 3 + 1000, 3, bad=[(GRID_CAP // 3 + 999, 3)])]
for _K in (1, 16, 17, 64, 65, 128, 129):
    CASES += [kw(f"kw_fwd_K{_K}", "exact integers; K round the key tile of 64", "fwd", KW_300, _K, 7, pad=5, exact=True),
              kw(f"kw_bwd_K{_K}", "exact integers; K round the tile of 64, the LDS chunk of 16 and the range of 128; pre-filled g_a", "bwd", KW_300, _K, 7, pad=5, exact=True)]
for _V in (1, 7, 32):
    CASES += [kw(f"kw_fwd_V{_V}", "float; padded rows (ld_m > total)", "fwd", KW_257, 17, _V, pad=3), kw(f"kw_bwd_V{_V}", "float; NaN in the padding of g_M", "bwd", KW_257, 17, _V, pad=3)]
CASES += [
    kw("kw_bwd_acc_1tile", "accumulate_w = 1 on a pre-filled g_W, one tile (stores)", "bwd", KW_300, 64, 7, acc=1),
    kw("kw_bwd_acc_tiles", "accumulate_w = 1 on a pre-filled g_W, three tiles (atomics)", "bwd", KW_300, 129, 7, acc=1),
    kw("kw_bwd_fill_tiles", "accumulate_w = 0 on a pre-filled g_W, three tiles: zero-filled first", "bwd", KW_300, 129, 7, acc=0),
    kw("kw_bwd_fill_exact", "the same with integers", "bwd", KW_SMALL, 200, 3, acc=0, exact=True),
    kw("kw_bwd_only_a", "g_W NULL", "bwd", KW_300, 65, 7, outs="a"), kw("kw_bwd_only_w", "g_a NULL (no workspace)", "bwd", KW_300, 65, 7, outs="w"),
    kw("kw_fwd_wide", "1024 column blocks, 80 keys: one tile of 512 (the protein net's form)", "fwd", KW_WIDE, 80, 4),
    kw("kw_bwd_wide", "the same, backward: g_W stored, not added", "bwd", KW_WIDE, 80, 4, acc=0),
    kw("kw_bwd_wide_K513", "two tiles of 512 add with atomics; exact integers", "bwd", KW_WIDE, 513, 2, exact=True, acc=0),
    kwm("kwm_1", "one layer", [KW_300], 17, 7), kwm("kwm_2", "two layers of different width", [KW_300, KW_SMALL], 65, 7),
    kwm("kwm_8", "eight layers", [KW_300, KW_SMALL, KW_257, KW_SMALL, KW_300, KW_257, KW_SMALL, KW_300], 17, 5, null_w=3),
    kwm("kwm_8_tiles", "eight layers, three key tiles: atomics between tiles, zero-fill first", [KW_300, KW_SMALL, KW_257, KW_SMALL, KW_300, KW_257, KW_SMALL, KW_300],
        130, 5, exact=True),
    kwm("kwm_2_acc", "accumulate_w = 1, tiles", [KW_300, KW_257], 129, 3, acc=1),
    refuse("act_fwd_6", "act = 6", "act_fwd", E3K_ERR_INVALID, act=6), refuse("act_fwd_m1", "act = -1", "act_fwd", E3K_ERR_INVALID, act=-1),
    refuse("act_bwd_6", "act = 6", "act_bwd", E3K_ERR_INVALID, act=6), refuse("act_bwd2_m1", "act = -1", "act_bwd2", E3K_ERR_INVALID, act=-1),
    refuse("act_out_silu", "only ssp has the from-output form", "act_bwd_from_output", E3K_ERR_INVALID, act=2),
    refuse("act_out_cst0", "cst = 0", "act_bwd_from_output", E3K_ERR_INVALID, act=1, cst=0.0),
    refuse("act_out_cst_neg", "cst < 0", "act_bwd_from_output", E3K_ERR_INVALID, act=1, cst=-1.0),
    refuse("na_fwd_17", "17 blocks", "norm_act_fwd", E3K_ERR_INVALID, table="na_17"), refuse("na_bwd_17", "17 blocks", "norm_act_bwd", E3K_ERR_INVALID, table="na_17"),
    refuse("na_bwd2_17", "17 blocks", "norm_act_bwd2", E3K_ERR_INVALID, table="na_17"), refuse("na_fwd_eps_neg", "epsilon < 0", "norm_act_fwd", E3K_ERR_INVALID, eps=-1e-3),
    refuse("ln_fwd_17", "17 blocks", "layernorm_fwd", E3K_ERR_INVALID, table="ln_17"), refuse("ln_bwd_17", "17 blocks", "layernorm_bwd", E3K_ERR_INVALID, table="ln_17"),
    refuse("ln_bwd2_17", "17 blocks", "layernorm_bwd2", E3K_ERR_INVALID, table="ln_17"),
    refuse("rl_17", "17 blocks", "relayout", E3K_ERR_INVALID, table="ln_17"),
    refuse("seg_dim0", "dim = 0", "segment_sum", E3K_ERR_INVALID, dim=0), refuse("c2p_neg", "n_seg < 0", "counts_to_ptr", E3K_ERR_INVALID, G=-1),
    refuse("oh_T0", "num_types = 0", "onehot", E3K_ERR_INVALID, T=0),
    refuse("kw_fwd_V33", "V = 33", "keyed_weights_fwd", E3K_ERR_UNSUPPORTED, V=33), refuse("kw_bwd_V33", "V = 33", "keyed_weights_bwd", E3K_ERR_UNSUPPORTED, V=33),
    refuse("kw_fwd_ld", "ld_m < total", "keyed_weights_fwd", E3K_ERR_INVALID, ld=-1),
    refuse("kwm_9", "nine layers", "keyed_weights_fwd_multi", E3K_ERR_INVALID, layers=9), refuse("kwm_bwd_9", "nine layers", "keyed_weights_bwd_multi", E3K_ERR_INVALID, layers=9),
    refuse("kwm_V", "layers of unequal V", "keyed_weights_fwd_multi", E3K_ERR_UNSUPPORTED, unequal=True),
    refuse("kwm_bwd_V", "layers of unequal V", "keyed_weights_bwd_multi", E3K_ERR_UNSUPPORTED, unequal=True),
]


def table_kernels():
    return set().union(*(c["kernels"] for c in CASES))


def table_functions():
    return set().union(*(c["funcs"] for c in CASES))


# ---------------------------------------------------------------------------------------------------------------------------------
# activations
SPECIAL = np.array([0.0, 1e-6, -1e-6, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4])


def act_inputs(c):
    rng, n = _rng(c), c["n"]
    base = np.concatenate([SPECIAL, np.linspace(-20.0, 20.0, 241)])
    x = rng.uniform(-20.0, 20.0, n)
    x[:min(n, len(base))] = base[:n]
    x = x.astype(f32)
    inp = dict(x=x, gy=rng.standard_normal(n).astype(f32), gh=rng.standard_normal(n).astype(f32))
    if c["op"] == "out":
        inp["y"] = (float(f32(c["cst"])) * ssp64(x.astype(np.float64))).astype(f32)
    return inp


def act_reference(c, inp, mutant=None):
    """name -> (want, bound) of what the call writes"""
    a, cst, x = c["act"], float(f32(c["cst"])), EV(inp["x"])
    gy, gh = EV(inp["gy"]), EV(inp["gh"])
    if c["op"] == "fwd":
        return dict(y=(cst * act_ev(a, x, mutant)).pair())
    if c["op"] == "bwd":
        return dict(gx=((gy * cst) * dact_ev(a, x, mutant)).pair())
    if c["op"] == "bwd2":
        h = gh * cst
        return dict(g_gy=(h * dact_ev(a, x, mutant)).pair(), g_x=((h * gy) * d2act_ev(a, x, mutant)).pair())
    y = EV(inp["y"])
    inv = EV._r(1.0 / cst, 0.0)
    fac = 1.0 - 0.5 * exp_ev((-y) * inv)
    own = ((gy * cst) * fac).pair()
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-x.v))
    # the same gradient from x: y is cst ssp(x) rounded to fp32, and d (cst factor) / d y = 0.5 exp(-y / cst) <= 1
    return dict(gx=own, gx_from_x=(gy.v * cst * sg, own[1] + U * np.abs(y.v) * np.abs(gy.v) + 2.0 ** -50 * np.abs(gy.v) * cst))


# ---------------------------------------------------------------------------------------------------------------------------------
# double backward of the Gate (formulas of include/e3k.h; the operation order of gate_bwd2_gy_kernel / gate_bwd2_x_kernel)
def gate2_inputs(c):
    rng, spec, rows = _rng(c), GATE_SPECS[c["spec"]], c["rows"]
    return dict(x=rng.standard_normal((rows, spec["in_dim"])).astype(f32), gy=rng.standard_normal((rows, spec["out_dim"])).astype(f32),
                h=rng.standard_normal((rows, spec["in_dim"])).astype(f32))


def gate2_reference(c, inp, mutant=None):
    spec, cf, rows = GATE_SPECS[c["spec"]], c["cf"], c["rows"]
    x, gy, h = inp["x"], inp["gy"], inp["h"]
    out = dict(g_gy=[np.zeros((rows, spec["out_dim"])), np.zeros((rows, spec["out_dim"]))], g_x=[np.zeros((rows, spec["in_dim"])), np.zeros((rows, spec["in_dim"]))])

    def put(name, sl, ev):
        out[name][0][:, sl], out[name][1][:, sl] = ev.pair()

    mid = lambda ev: EV(ev.v[:, None, :], ev.e[:, None, :])
    for kind, io, go, oo, mul, dim, a, cst in spec["segs"]:
        cst = float(f32(cst))
        if kind == 0:
            xs, hs, gs = EV(x[:, io:io + mul]), EV(h[:, io:io + mul]), EV(gy[:, oo:oo + mul])
            put("g_gy", slice(oo, oo + mul), (hs * cst) * dact_ev(a, xs))
            put("g_x", slice(io, io + mul), ((hs * gs) * cst) * d2act_ev(a, xs, mutant))
            continue
        xb, hb = EV(x[:, io:io + mul * dim].reshape(rows, dim, mul)), EV(h[:, io:io + mul * dim].reshape(rows, dim, mul))
        gt, hg = EV(x[:, go:go + mul]), EV(h[:, go:go + mul])
        g = EV(_out_view(gy[:, oo:oo + mul * dim], mul, dim, cf))
        sa, sda = cst * act_ev(a, gt), cst * dact_ev(a, gt)
        ggy = hb * mid(sa) + (mid(hg) * xb) * mid(sda)
        v, e = ggy.pair()
        if not cf:
            v, e = v.transpose(0, 2, 1), e.transpose(0, 2, 1)
        out["g_gy"][0][:, oo:oo + mul * dim], out["g_gy"][1][:, oo:oo + mul * dim] = v.reshape(rows, -1), e.reshape(rows, -1)
        dgh, dgx = dot_ev(g, hb, 1), dot_ev(g, xb, 1)
        put("g_x", slice(go, go + mul), cst * (dgh * dact_ev(a, gt) + (hg * dgx) * d2act_ev(a, gt, mutant)))
        v, e = ((mid(hg) * g) * mid(sda)).pair()
        out["g_x"][0][:, io:io + mul * dim], out["g_x"][1][:, io:io + mul * dim] = v.reshape(rows, -1), e.reshape(rows, -1)
    return {k: tuple(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# NormActivation
NA_KINDS = ("zero", "half_eps", "two_eps", "1e-3")


def na_channel_kind(r, k, u):
    """which channels of which rows carry a planted norm (index into NA_KINDS), -1: random"""
    t = (5 * r + 3 * k + u) % 9
    return t if t < 4 else -1


def na_inputs(c):
    rng, tb, rows = _rng(c), TABLES[c["table"]], c["rows"]
    x = rng.standard_normal((rows, tb["row_dim"]))
    eps = c["eps"] if c["eps"] > 0 else 1e-4
    planted = np.zeros((rows, tb["row_dim"]), bool)
    for k, (off, mul, dim) in enumerate(tb["blocks"]):
        X = x[:, off:off + mul * dim].reshape(rows, dim, mul)      # channel-fastest
        P = planted[:, off:off + mul * dim].reshape(rows, dim, mul)
        for r in range(min(rows, 9)):
            for u in range(mul):
                t = na_channel_kind(r, k, u)
                if t >= 0:
                    d = X[r, :, u] / np.linalg.norm(X[r, :, u])
                    X[r, :, u] = d * (0.0, 0.5 * eps, 2.0 * eps, 1e-3)[t]
                    P[r, :, u] = True
    return dict(x=x.astype(f32), gy=rng.standard_normal(x.shape).astype(f32), h=rng.standard_normal(x.shape).astype(f32), planted=planted)


def na_scales(c, n2, second, mutant=None):
    """normact_scale / normact_scale2 on the squared norms: s, d (and d2), and which channels the clamp holds"""
    a = c["act"]
    eps2 = float(f32(c["eps"]) * f32(c["eps"]))
    if eps2 > 0:
        thr = float(f32(c["eps"])) if mutant == "clamp_eps" else eps2
        clamped = n2.v < thr
        assert mutant or not (np.abs(n2.v - thr) <= 4 * n2.e).any(), "a channel sits on the clamp's comparison"
        n = where(clamped, thr, n2).sqrt()
        av, a1 = act_ev(a, n), dact_ev(a, n)
        if not second:
            if c["normalize"]:
                s, d = av / n, (a1 * n - av) / (n * n * n)
            else:
                s, d = av, a1 / n
            return s, where(clamped, 0.0, d), None, clamped
        a2 = d2act_ev(a, n)
        if c["normalize"]:
            s, s1, s2 = av / n, (a1 * n - av) / (n * n), (a2 * n * n - 2.0 * a1 * n + 2.0 * av) / (n * n * n)
        else:
            s, s1, s2 = av, a1, a2
        return s, where(clamped, 0.0, s1 / n), where(clamped, 0.0, (s2 * n - s1) / (n * n * n)), clamped
    clamped = np.zeros(n2.v.shape, bool)
    if not second:
        return act_ev(a, n2), 2.0 * dact_ev(a, n2), None, clamped
    return act_ev(a, n2), 2.0 * dact_ev(a, n2), 4.0 * d2act_ev(a, n2), clamped


def na_reference(c, inp, mutant=None):
    tb, rows, op = TABLES[c["table"]], c["rows"], c["op"]
    shape = (rows, tb["row_dim"])
    out = {k: [np.zeros(shape), np.zeros(shape)] for k in {"fwd": ["y"], "bwd": ["gx"], "bwd2": ["g_gy", "g_x"]}[op]}
    clamped_elems = 0

    def put(name, off, ev, cf):      # ev [rows, dim, mul]
        v, e = ev.pair()
        if not cf:
            v, e = v.transpose(0, 2, 1), e.transpose(0, 2, 1)
        out[name][0][:, off:off + v[0].size] = v.reshape(rows, -1)
        out[name][1][:, off:off + v[0].size] = e.reshape(rows, -1)

    for off, mul, dim in tb["blocks"]:
        sl = slice(off, off + mul * dim)
        X = EV(inp["x"][:, sl].reshape(rows, dim, mul))
        n2 = dot_ev(X, X, 1)
        s, d, d2, clamped = na_scales(c, n2, op == "bwd2", mutant)
        clamped_elems += int(clamped.sum()) * dim
        s, d = EV(s.v[:, None, :], s.e[:, None, :]), EV(d.v[:, None, :], d.e[:, None, :])
        if op == "fwd":
            put("y", off, s * X, cf=False)
            continue
        G = EV(inp["gy"][:, sl].reshape(rows, mul, dim).transpose(0, 2, 1))      # e3nn layout -> [rows, dim, mul]
        gx_ = dot_ev(G, X, 1)
        gx_ = EV(gx_.v[:, None, :], gx_.e[:, None, :])
        if op == "bwd":
            put("gx", off, fma(s, G, (d * gx_) * X), cf=True)
            continue
        H = EV(inp["h"][:, sl].reshape(rows, dim, mul))
        hx, hg = dot_ev(H, X, 1), dot_ev(H, G, 1)
        hx, hg = EV(hx.v[:, None, :], hx.e[:, None, :]), EV(hg.v[:, None, :], hg.e[:, None, :])
        d2 = EV(d2.v[:, None, :], d2.e[:, None, :])
        put("g_gy", off, fma(s, H, (d * hx) * X), cf=False)
        t2 = ((d2 * X) * hx) * gx_ if mutant != "no_d2" else EV(np.zeros_like(X.v))
        put("g_x", off, ((d * X) * hg + t2) + d * (H * gx_ + hx * G), cf=True)
    res = {k: (v[0], v[1]) for k, v in out.items()}
    res["clamped_elems"] = clamped_elems
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# per-block RMS normalisation
LN_EPS = float(f32(1e-6))


def ln_inputs(c):
    rng, tb, rows = _rng(c), TABLES[c["table"]], c["rows"]
    nb = len(tb["blocks"])
    x = rng.standard_normal((rows, tb["row_dim"])).astype(f32)
    if rows:
        off, mul, dim = tb["blocks"][1]
        x[0, off:off + mul * dim] = 0.0      # inv = 1 / sqrt(1e-6)
    inv = np.zeros((rows, nb))
    for k, (off, mul, dim) in enumerate(tb["blocks"]):
        X = x[:, off:off + mul * dim].astype(np.float64)
        inv[:, k] = 1.0 / np.sqrt((X * X).sum(1) / mul + LN_EPS)
    return dict(x=x, gy=rng.standard_normal(x.shape).astype(f32), h=rng.standard_normal(x.shape).astype(f32), std=rng.uniform(0.5, 1.5, nb).astype(f32),
                hs=rng.standard_normal(nb).astype(f32), inv=inv.astype(f32), old_gstd=rng.standard_normal(nb).astype(f32))


def ln_reference(c, inp, mutant=None):
    """name -> (want, bound); y / g_x / g_gy carry NaN where no block covers a column: written by nobody"""
    tb, rows, op = TABLES[c["table"]], c["rows"], c["op"]
    nb, shape = len(tb["blocks"]), (rows, tb["row_dim"])
    names = {"fwd": ["y"], "bwd": ["gx"], "bwd2": ["g_gy", "g_x"]}[op]
    out = {k: [np.full(shape, np.nan), np.zeros(shape)] for k in names}
    small = {k: [np.zeros((rows, nb)) if k == "inv" else np.zeros(nb), np.zeros((rows, nb)) if k == "inv" else np.zeros(nb)]
             for k in (["inv"] if op == "fwd" else ["g_std"])}
    eps = 1e-5 if mutant == "eps_1e-5" else LN_EPS
    col = lambda ev: EV(ev.v[:, None], ev.e[:, None])
    for k, (off, mul, dim) in enumerate(tb["blocks"]):
        sl = slice(off, off + mul * dim)
        m = float(mul * dim if mutant == "mean_over_len" else mul)
        X, sc = EV(inp["x"][:, sl]), float(inp["std"][k])
        if op == "fwd":
            inv = 1.0 / (dot_ev(X, X, 1) / m + eps).sqrt()
            small["inv"][0][:, k], small["inv"][1][:, k] = inv.pair()
            v, e = (X * col(inv * sc)).pair()
            out["y"][0][:, sl], out["y"][1][:, sl] = v, e
            continue
        G, v_ = EV(inp["gy"][:, sl]), EV(inp["inv"][:, k])
        D = dot_ev(G, X, 1)
        if op == "bwd":
            coef = ((D * v_) * v_) / m
            gv, ge = (col(sc * v_) * (G - X * col(coef))).pair()
            out["gx"][0][:, sl], out["gx"][1][:, sl] = gv, ge
            gs = sum_ev(D * v_, 0, extra=float(inp["old_gstd"][k]))
        else:
            H = EV(inp["h"][:, sl])
            A, B = dot_ev(H, G, 1), dot_ev(H, X, 1)
            hsk = float(inp["hs"][k]) if c["hs"] else 0.0
            v3 = (v_ * v_) * v_
            three = 2.0 if mutant == "v5_factor" else 3.0
            cg_x = ((-sc) * v3) * B / m + hsk * v_
            cx_x = (((-sc) * A) * v3) / m + (((((three * sc) * v3) * v_) * v_) * D) * B / (m * m) - ((hsk * D) * v3) / m
            cx_h = (((-sc) * v3) * D) / m
            gv, ge = fma(col(sc * v_), H, col(cg_x) * X).pair()
            out["g_gy"][0][:, sl], out["g_gy"][1][:, sl] = gv, ge
            gv, ge = fma(col(cx_x), X, fma(col(cg_x), G, col(cx_h) * H)).pair()
            out["g_x"][0][:, sl], out["g_x"][1][:, sl] = gv, ge
            gs = sum_ev(v_ * A - ((v3 * D) * B) / m, 0, extra=float(inp["old_gstd"][k]))
        small["g_std"][0][k], small["g_std"][1][k] = gs.v, gs.e
    res = {k: tuple(v) for k, v in out.items()}
    res.update({k: tuple(v) for k, v in small.items()})
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# segment sum
def seg_inputs(c):
    rng = _rng(c)
    n = int(np.sum(c["sizes"]))
    x = rng.integers(-50, 51, (n, c["dim"])).astype(f32) if c["exact"] else rng.standard_normal((n, c["dim"])).astype(f32)
    return dict(x=x, ptr=np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int32))


def seg_reference(c, inp, mutant=None):
    S = len(c["sizes"])
    want, bound = np.zeros((S, c["dim"])), np.zeros((S, c["dim"]))
    x = inp["x"].astype(np.float64)
    for s, n in enumerate(c["sizes"]):
        rowsx = x[inp["ptr"][s]:inp["ptr"][s + 1]]
        t = EV(rowsx.sum(0), (gamma(max(n, 1)) + 2.0 ** -52 * n) * np.abs(rowsx).sum(0))
        if c["mean"]:
            with np.errstate(divide="ignore", invalid="ignore"):
                t = t / float(n if mutant == "empty_div0" else max(n, 1))
        want[s], bound[s] = t.v, t.e
    return dict(out=(want, bound))


# ---------------------------------------------------------------------------------------------------------------------------------
# relayout, one-hot, counts -> ptr
def rl_reference(x, blocks, to_cf):
    y = x.copy()
    rows = x.shape[0]
    for off, mul, dim in blocks:
        b = x[:, off:off + mul * dim]
        y[:, off:off + mul * dim] = (b.reshape(rows, mul, dim) if to_cf else b.reshape(rows, dim, mul)).transpose(0, 2, 1).reshape(rows, -1)
    return y


def oh_inputs(c):
    idx = _rng(c).integers(0, c["T"], c["rows"]).astype(np.int64)
    for r, v in c["bad"]:
        idx[r] = v
    return idx


def oh_reference(c, idx):
    out = (idx[:, None] == np.arange(c["T"])[None, :]).astype(f32)
    return out, c["flag"] | (4 if len(c["bad"]) else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# keyed weights
def kw_layout(instr, V):
    """[(w_off, m_off, u, w_out)], the flat weight's size, the number of columns"""
    out, w_off, m_off = [], 0, 0
    for u, w in instr:
        out.append((w_off, m_off, u, w))
        w_off, m_off = w_off + u * V * w, m_off + u * w
    return out, w_off, m_off


def kw_inputs(c, instr=None, tag=""):
    instr = c["instr"] if instr is None else instr
    rng = np.random.default_rng(zlib.crc32((c["id"] + tag).encode()))
    lay, nW, total = kw_layout(instr, c["V"])
    K, V = c["K"], c["V"]
    if c["exact"]:
        draw = lambda *s: rng.integers(-4, 5, s, dtype=np.int8).astype(f32)
    else:
        draw = lambda *s: rng.standard_normal(s, dtype=f32)
    return dict(a=draw(K, V), W=draw(nW), gM=draw(K, total), old_ga=draw(K, V), old_gW=draw(nW))


def kw_reference(c, inp, instr=None, mutant=None, acc=None):
    """M, g_W, g_a as (want, bound); exact cases: float32 arithmetic on integers is exact, the bound is zero"""
    instr = c["instr"] if instr is None else instr
    acc = c.get("acc", 0) if acc is None else acc
    lay, nW, total = kw_layout(instr, c["V"])
    K, V = c["K"], c["V"]
    dt = f32 if c["exact"] else np.float64
    a, W, gM = inp["a"].astype(dt), inp["W"].astype(dt), inp["gM"].astype(dt)
    M = np.zeros((K, total), dt)
    Wc = np.zeros((total, V), dt)      # W as a [columns, V] matrix
    gW, gWa = np.zeros(nW, dt), np.zeros(nW, dt)
    for w_off, m_off, u, w in lay:
        blk = W[w_off:w_off + u * V * w]
        Wj = blk.reshape(u, V, w) if mutant != "uwv" else blk.reshape(u, w, V).transpose(0, 2, 1)
        Wc[m_off:m_off + u * w] = Wj.transpose(0, 2, 1).reshape(u * w, V)
        g = gM[:, m_off:m_off + u * w].reshape(K, u, w)
        gW[w_off:w_off + u * V * w] = np.einsum("tv,tuw->uvw", a, g).ravel()
        if not c["exact"]:
            gWa[w_off:w_off + u * V * w] = np.einsum("tv,tuw->uvw", np.abs(a), np.abs(g)).ravel()
    M = a @ Wc.T
    ga = gM @ Wc + inp["old_ga"].astype(dt)
    old_w = inp["old_gW"].astype(dt) * (1 if acc else 0)
    gW = gW + old_w
    if c["exact"]:
        z = lambda v: (v.astype(np.float64), np.zeros(v.shape))
        return dict(M=z(M), g_W=z(gW), g_a=z(ga))
    bM = gamma(V) * (np.abs(a) @ np.abs(Wc).T)
    bW = gamma(K + 1) * (gWa + np.abs(old_w))
    ba = gamma(total + 1) * (np.abs(gM) @ np.abs(Wc) + np.abs(inp["old_ga"]))
    return dict(M=(M, bM + FL), g_W=(gW, bW + FL), g_a=(ga, ba + FL))


def kw_workspace(instr, K, V):
    total = sum(u * w for u, w in instr)
    return (total + 255) // 256 * K * V


# ---------------------------------------------------------------------------------------------------------------------------------
# running the cases
class Arena(_Arena):
    """the arena of the radial-table matrix with every word NaN unless a buffer's initial values say otherwise"""

    def upload(self, dev):
        self.x0 = np.full(self.n + 32, np.nan, f32).view(np.int32)
        for name, init in self.inits:
            off, n = self.blocks[name]
            v = np.asarray(init)
            self.x0[off:off + n] = v.ravel().view(np.int32) if v.ndim else np.full(n, v).astype(v.dtype).view(np.int32)
        self.buf = torch.from_numpy(self.x0).to(dev)
        self.base = self.buf.data_ptr()
        assert self.base % 64 == 0
        return self

    def out(self, name, n):
        return self.alloc(name, n)


WORST = {}


class Check(_Check):
    def equal(self, name, want):
        """float outputs compared by value with == (exact cases)"""
        want = np.asarray(want, np.float64).ravel()
        self._claim(name, len(want))
        got = self.dev(name, np.float32)[:len(want)].astype(np.float64)
        bad = np.flatnonzero(~(got == want))
        assert len(bad) == 0, f"{name}: {len(bad)} of {len(want)} differ, first at {bad[:5]}: got {got[bad[:5]]}, want {want[bad[:5]]}"

    def finish(self):
        self.unchanged()
        for family, r in self.ratios.items():
            print(f"{self.case['id']}: {family} worst error / bound {r:.3f}")
            WORST[family] = max(WORST.get(family, 0.0), r)
            record_measured("test_gpu_node_matrix", case=self.case["id"], family=family, error_over_bound=r)


def _arena(c):
    return Arena(zlib.crc32(c["id"].encode()) ^ 0x5A5A)


def _blocks(L, blocks):
    arr = (L.Block * max(len(blocks), 1))()
    for i, (off, mul, dim) in enumerate(blocks):
        arr[i].off, arr[i].mul, arr[i].dim = off, mul, dim
    return arr


def _instr(L, instr, V):
    lay = kw_layout(instr, V)[0]
    arr = (L.KwInstr * len(lay))()
    for i, (w_off, m_off, u, w) in enumerate(lay):
        arr[i].w_off, arr[i].m_off, arr[i].u, arr[i].w_out = w_off, m_off, u, w
    return arr


def run_act(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp, n, op, a, cst = act_inputs(c), c["n"], c["op"], c["act"], c["cst"]
    ar = _arena(c)
    for k in ("x", "gy", "gh") + (("y",) if op == "out" else ()):
        ar.alloc(k, n, inp[k] if n else None)
    ar.out("o1", n).out("o2", n).upload(dev)
    if op == "fwd":
        rc, outs = lib.e3k_act_fwd(ar.p("x"), n, a, cst, ar.p("o1"), st), [("o1", "y")]
    elif op == "bwd":
        rc, outs = lib.e3k_act_bwd(ar.p("x"), ar.p("gy"), n, a, cst, ar.p("o1"), st), [("o1", "gx")]
    elif op == "out":
        rc, outs = lib.e3k_act_bwd_from_output(ar.p("y"), ar.p("gy"), n, a, cst, ar.p("o1"), st), [("o1", "gx")]
    else:
        o = c["outs"]
        rc = lib.e3k_act_bwd2(ar.p("x"), ar.p("gy") if o in ("both", "gx") else None, ar.p("gh"), n, a, cst, ar.p("o1") if o in ("both", "ggy") else None,
                              ar.p("o2") if o in ("both", "gx") else None, st)
        outs = [(b, k) for b, k, on in (("o1", "g_gy", o in ("both", "ggy")), ("o2", "g_x", o in ("both", "gx"))) if on]
    ck = Check(ar, c)
    if c["outs"] == "none":
        assert rc == E3K_ERR_INVALID
    else:
        assert rc == E3K_OK
        if n:
            ref = act_reference(c, inp)
            for b, k in outs:
                assert np.isfinite(ref[k][0]).all() and np.isfinite(ref[k][1]).all()
                ck.close(b, *ref[k], "act_" + op)
            if op == "out":
                got = ck.dev("o1", np.float32).astype(np.float64)
                want, bound = ref["gx_from_x"]
                assert (np.abs(got - want) <= bound).all(), "act_bwd_from_output against cst sigmoid(x)"
                ck.ratio("act_out_from_x", float((np.abs(got - want) / bound).max()))
    ck.finish()


def run_gate2(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp, spec, rows, o = gate2_inputs(c), GATE_SPECS[c["spec"]], c["rows"], c["outs"]
    ni, no = rows * spec["in_dim"], rows * spec["out_dim"]
    ar = _arena(c)
    ar.alloc("x", ni, inp["x"] if rows else None).alloc("gy", no, inp["gy"] if rows else None).alloc("h", ni, inp["h"] if rows else None)
    ar.out("g_gy", no).out("g_x", ni).upload(dev)
    rc = lib.e3k_gate_bwd2(ar.p("x"), ar.p("gy") if o != "ggy" else None, ar.p("h"), rows, spec["in_dim"], spec["out_dim"], _seg_array(L, spec["segs"]),
                           len(spec["segs"]), c["cf"], ar.p("g_gy") if o != "gx" else None, ar.p("g_x") if o != "ggy" else None, st)
    assert rc == E3K_OK
    ck = Check(ar, c)
    if rows:
        ref = gate2_reference(c, inp)
        for k, on in (("g_gy", o != "gx"), ("g_x", o != "ggy")):
            if on:
                ck.close(k, *ref[k], "gate_bwd2_" + k)
    ck.finish()


def run_na(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp, tb, rows, op = na_inputs(c), TABLES[c["table"]], c["rows"], c["op"]
    n = rows * tb["row_dim"]
    ar = _arena(c)
    for k in ("x", "gy", "h"):
        ar.alloc(k, n, inp[k] if n else None)
    ar.out("o1", n).out("o2", n).upload(dev)
    common = (rows, tb["row_dim"], _blocks(L, tb["blocks"]), len(tb["blocks"]), c["act"], c["eps"], c["normalize"])
    if op == "fwd":
        rc, outs = lib.e3k_norm_act_fwd(ar.p("x"), *common, ar.p("o1"), st), [("o1", "y")]
    elif op == "bwd":
        rc, outs = lib.e3k_norm_act_bwd(ar.p("x"), ar.p("gy"), *common, ar.p("o1"), st), [("o1", "gx")]
    else:
        o = c["outs"]
        rc = lib.e3k_norm_act_bwd2(ar.p("x"), ar.p("gy"), ar.p("h"), *common, ar.p("o1") if o != "gx" else None, ar.p("o2") if o != "ggy" else None, st)
        outs = [(b, k) for b, k, on in (("o1", "g_gy", o != "gx"), ("o2", "g_x", o != "ggy")) if on]
    assert rc == E3K_OK
    ck = Check(ar, c)
    if n:
        ref = na_reference(c, inp)
        for b, k in outs:
            assert np.isfinite(ref[k][0]).all() and np.isfinite(ref[k][1]).all()
            ck.close(b, *ref[k], "norm_act_" + op)      # (an uncovered column: want 0, bound 0)
    ck.finish()


def run_ln(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp, tb, rows, op = ln_inputs(c), TABLES[c["table"]], c["rows"], c["op"]
    nb, n = len(tb["blocks"]), rows * tb["row_dim"]
    ar = _arena(c)
    for k in ("x", "gy", "h"):
        ar.alloc(k, n, inp[k] if n else None)
    ar.alloc("std", nb, inp["std"]).alloc("hs", nb, inp["hs"]).alloc("inv", rows * nb, inp["inv"] if op != "fwd" and rows else None)
    ar.alloc("g_std", nb, inp["old_gstd"]).out("o1", n).out("o2", n).upload(dev)
    common = (rows, tb["row_dim"], _blocks(L, tb["blocks"]), nb, ar.p("std"))
    o = c["outs"]
    if op == "fwd":
        rc, outs = lib.e3k_layernorm_fwd(ar.p("x"), *common, ar.p("o1"), ar.p("inv"), st), [("o1", "y"), ("inv", "inv")]
    elif op == "bwd":
        rc, outs = lib.e3k_layernorm_bwd(ar.p("x"), ar.p("gy"), ar.p("inv"), *common, ar.p("o1"), ar.p("g_std"), st), [("o1", "gx"), ("g_std", "g_std")]
    else:
        rc = lib.e3k_layernorm_bwd2(ar.p("x"), ar.p("gy"), ar.p("h"), ar.p("hs") if c["hs"] else None, ar.p("inv"), *common,
                                    ar.p("o1") if "g" in o else None, ar.p("o2") if "x" in o else None, ar.p("g_std") if "s" in o else None, st)
        outs = [(b, k) for b, k, on in (("o1", "g_gy", "g" in o), ("o2", "g_x", "x" in o), ("g_std", "g_std", "s" in o)) if on]
    assert rc == E3K_OK
    ck = Check(ar, c)
    if rows:
        ref = ln_reference(c, inp)
        for b, k in outs:
            ck.close(b, *ref[k], "layernorm_" + op)      # (want NaN on uncovered columns: they must still be NaN)
    ck.finish()


def run_seg(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp, S, dim = seg_inputs(c), len(c["sizes"]), c["dim"]
    ar = _arena(c)
    ar.alloc("x", inp["x"].size, inp["x"] if inp["x"].size else None).alloc("ptr", S + 1, inp["ptr"]).out("out", S * dim).upload(dev)
    assert lib.e3k_segment_sum(ar.p("x"), ar.p("ptr"), S, dim, c["mean"], ar.p("out"), st) == E3K_OK
    ck = Check(ar, c)
    if S:
        want, bound = seg_reference(c, inp)["out"]
        if c["exact"]:
            assert np.abs(inp["x"]).sum(0).max() < 2 ** 24      # every partial sum is an integer fp32 holds
            ck.equal("out", want)
        else:
            ck.close("out", want, bound, "segment_sum")
    ck.finish()


def run_rl(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    tb, rows = TABLES[c["table"]], c["rows"]
    n = rows * tb["row_dim"]
    x = _rng(c).standard_normal((rows, tb["row_dim"])).astype(f32)
    ar = _arena(c)
    ar.alloc("x", n, x).out("cf", n).out("back", n).out("cf_of_x_as_cf", n).upload(dev)
    bl = (_blocks(L, tb["blocks"]), len(tb["blocks"]))
    assert lib.e3k_relayout(ar.p("x"), rows, tb["row_dim"], *bl, 1, ar.p("cf"), st) == E3K_OK
    assert lib.e3k_relayout(ar.p("cf"), rows, tb["row_dim"], *bl, 0, ar.p("back"), st) == E3K_OK
    assert lib.e3k_relayout(ar.p("x"), rows, tb["row_dim"], *bl, 0, ar.p("cf_of_x_as_cf"), st) == E3K_OK
    ck = Check(ar, c)
    ck.exact("cf", rl_reference(x, tb["blocks"], 1))
    ck.exact("back", x)
    ck.exact("cf_of_x_as_cf", rl_reference(x, tb["blocks"], 0))
    ck.finish()


def run_c2p(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    G = c["G"]
    counts = np.zeros(G, np.int64) if c["zero"] else _rng(c).integers(0, 40, G).astype(np.int64)
    ar = _arena(c)
    ar.alloc("counts", 2 * G, counts.view(np.int32) if G else None, align=2).alloc("ptr", G + 1, np.int32(-7)).upload(dev)
    assert lib.e3k_counts_to_ptr(ar.p("counts"), G, ar.p("ptr"), st) == E3K_OK
    ck = Check(ar, c)
    ck.exact("ptr", np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    ck.finish()


def run_oh(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    idx, rows, T = oh_inputs(c), c["rows"], c["T"]
    want, flag = oh_reference(c, idx)
    ar = _arena(c)
    ar.alloc("idx", 2 * rows, idx.view(np.int32) if rows else None, align=2).alloc("flag", 1, np.int32(c["flag"])).out("out", rows * T).upload(dev)
    assert lib.e3k_onehot(ar.p("idx"), rows, T, ar.p("out"), ar.p("flag") if c["with_flag"] else None, st) == E3K_OK
    ck = Check(ar, c)
    if rows:
        ck.exact("out", want)
        for r, _ in c["bad"]:
            assert not want[r].any()
    ck.exact("flag", np.int32(flag if c["with_flag"] else c["flag"]).reshape(1))
    ck.finish()


def _kw_padded(M, pad, fill=np.nan):
    """[K, total] -> [K, total + pad] with `fill` in the padding"""
    out = np.full((M.shape[0], M.shape[1] + pad), fill, f32)
    out[:, :M.shape[1]] = M
    return out


def run_kw(dev, c, L):
    lib, st = L.load(), L.stream_ptr()
    inp, K, V, total, pad = kw_inputs(c), c["K"], c["V"], c["total"], c["pad"]
    ld, nW = total + pad, len(inp["W"])
    ins = _instr(L, c["instr"], V)
    ws = lib.e3k_keyed_weights_bwd_workspace(ins, len(c["instr"]), K, V)
    assert ws == kw_workspace(c["instr"], K, V)
    ar = _arena(c)
    ar.alloc("a", K * V, inp["a"]).alloc("W", nW, inp["W"])
    ref = kw_reference(c, inp)
    if c["op"] == "fwd":
        ar.out("M", K * ld).upload(dev)
        assert lib.e3k_keyed_weights_fwd(ar.p("a"), ar.p("W"), ins, len(c["instr"]), K, V, ld, ar.p("M"), st) == E3K_OK
        ck = Check(ar, c)
        want, bound = _kw_padded(ref["M"][0], pad).astype(np.float64), _kw_padded(ref["M"][1], pad, 0.0).astype(np.float64)
        if c["exact"]:
            live = ~np.isnan(want).ravel()
            got = ck.dev("M", np.float32)
            assert np.isnan(got[~live]).all(), "the padding of M was written"
            assert (got[live].astype(np.float64) == want.ravel()[live]).all()
            ck._claim("M")
        else:
            ck.close("M", want, bound, "keyed_weights_fwd")      # (NaN wanted in the padding)
        ck.finish()
        return
    o = c["outs"]
    ar.alloc("gM", K * ld, _kw_padded(inp["gM"], pad)).alloc("g_a", K * V, inp["old_ga"]).alloc("g_W", nW, inp["old_gW"]).out("ws", ws).upload(dev)
    rc = lib.e3k_keyed_weights_bwd(ar.p("a"), ar.p("W"), ar.p("gM"), ins, len(c["instr"]), K, V, ld, ar.p("g_a") if "a" in o else None,
                                   ar.p("g_W") if "w" in o else None, c["acc"], ar.p("ws") if "a" in o else None, st)
    assert rc == E3K_OK
    ck = Check(ar, c)
    for name, on in (("g_a", "a" in o), ("g_W", "w" in o)):
        if on:
            ck.equal(name, ref[name][0]) if c["exact"] else ck.close(name, *ref[name], "keyed_weights_bwd_" + name)
    if "a" in o:
        ck.free("ws", ws)
    ck.finish()


def run_kwm(dev, c, L):
    """the multi-layer forms in the arena against float64, and against the single-layer calls on buffers of their own"""
    lib, st = L.load(), L.stream_ptr()
    K, V, nl = c["K"], c["V"], len(c["layers"])
    inps = [kw_inputs(c, ins, tag=f":{i}") for i, ins in enumerate(c["layers"])]
    a = inps[0]["a"]
    ar = _arena(c)
    ar.alloc("a", K * V, a).alloc("g_a", K * V, inps[0]["old_ga"])
    items, handles, tot = (L.KwMultiItem * nl)(), [], []
    for i, (ins, inp) in enumerate(zip(c["layers"], inps)):
        total = kw_layout(ins, V)[2]
        tot.append(total)
        ar.alloc(f"W{i}", len(inp["W"]), inp["W"]).out(f"M{i}", K * total).alloc(f"gM{i}", K * total, inp["gM"]).alloc(f"gW{i}", len(inp["W"]), inp["old_gW"])
        h = C.c_void_p()
        assert lib.e3k_kw_args_create(_instr(L, ins, V), len(ins), V, total, C.byref(h)) == E3K_OK
        handles.append(h)
    ws_want = sum((t + 255) // 256 for t in tot) * K * V
    ar.out("ws", ws_want).upload(dev)
    try:
        for i in range(nl):
            items[i].args, items[i].W, items[i].M, items[i].accumulate_w = handles[i], ar.p(f"W{i}"), ar.p(f"M{i}"), c["acc"]
            items[i].g_W = None if c["null_w"] == i else ar.p(f"gW{i}")
        assert lib.e3k_keyed_weights_bwd_multi_workspace(items, nl, K) == ws_want
        assert lib.e3k_keyed_weights_fwd_multi(items, nl, ar.p("a"), K, st) == E3K_OK
        for i in range(nl):
            items[i].M = ar.p(f"gM{i}")
        assert lib.e3k_keyed_weights_bwd_multi(items, nl, ar.p("a"), K, ar.p("g_a"), ar.p("ws"), st) == E3K_OK
        ck = Check(ar, c)
    finally:
        for h in handles:
            lib.e3k_kw_args_destroy(h)
    # float64: g_a accumulates over the layers on top of its old value
    ga, S = inps[0]["old_ga"].astype(np.float64), np.abs(inps[0]["old_ga"]).astype(np.float64)      # S: sum |terms| of the one reduction
    single = []
    ad = torch.from_numpy(a).to(dev)
    ga_single = torch.from_numpy(inps[0]["old_ga"]).to(dev)
    for i, (ins, inp) in enumerate(zip(c["layers"], inps)):
        ref = kw_reference(c, dict(inp, a=a, old_ga=np.zeros((K, V), f32)), ins, acc=c["acc"])
        ga, S = ga + ref["g_a"][0], S + (ref["g_a"][1] - FL) / gamma(tot[i] + 1) if not c["exact"] else S
        for name, key in ((f"M{i}", "M"), (f"gW{i}", "g_W")):
            if key == "g_W" and c["null_w"] == i:
                continue
            ck.equal(name, ref[key][0]) if c["exact"] else ck.close(name, *ref[key], "keyed_weights_multi_" + key)
        # the single-layer calls
        Wd, gMd = torch.from_numpy(inp["W"]).to(dev), torch.from_numpy(inp["gM"]).to(dev)
        Md, gWd = torch.full((K, tot[i]), float("nan"), device=dev), torch.from_numpy(inp["old_gW"]).to(dev)
        wsd = torch.empty(kw_workspace(ins, K, V), device=dev)
        arr = _instr(L, ins, V)
        assert lib.e3k_keyed_weights_fwd(L.ptr(ad), L.ptr(Wd), arr, len(ins), K, V, tot[i], L.ptr(Md), st) == E3K_OK
        assert lib.e3k_keyed_weights_bwd(L.ptr(ad), L.ptr(Wd), L.ptr(gMd), arr, len(ins), K, V, tot[i], L.ptr(ga_single), L.ptr(gWd), c["acc"], L.ptr(wsd), st) == E3K_OK
        single.append((Md.cpu().numpy(), gWd.cpu().numpy()))
    ck.equal("g_a", ga) if c["exact"] else ck.close("g_a", ga, gamma(sum(tot) + 1) * S + FL, "keyed_weights_multi_g_a")
    ck.free("ws", ws_want)
    for i in range(nl):
        assert np.array_equal(ck.dev(f"M{i}"), single[i][0].ravel().view(np.int32)), f"layer {i}: the multi forward differs in bits from the single call"
        if c["null_w"] != i and c["tiles"] == 1:      # both forms store: the same chain of FMAs over the keys
            assert np.array_equal(ck.dev(f"gW{i}"), single[i][1].ravel().view(np.int32)), f"layer {i}: the multi g_W differs in bits from the single call"
    ck.finish()


def run_refuse(dev, c, L):
    """a small valid problem of the entry point, one argument replaced: the return code, and the arena bit-identical"""
    lib, st = L.load(), L.stream_ptr()
    o = dict(act=2, cst=1.5, table="ln_gap", eps=1e-4, dim=3, G=4, T=4, V=3, ld=0, layers=2, unequal=False)
    if c["fn"].startswith("e3k_norm_act"):
        o["table"] = "na_gap"
    o.update(c["over"])
    tb = TABLES[o["table"]]
    rows, nb = 4, len(tb["blocks"])
    n = rows * tb["row_dim"]
    ar = _arena(c)
    for k in ("x", "gy", "h", "o1", "o2"):
        ar.alloc(k, n, np.ones(n, f32))
    ar.alloc("std", 17, np.ones(17, f32)).alloc("inv", rows * 17, np.ones(rows * 17, f32)).alloc("g_std", 17, np.zeros(17, f32))
    ar.alloc("ptr", 5, np.array([0, 1, 2, 3, 4], np.int32)).alloc("i64", 16, np.zeros(16, np.int32), align=2).alloc("flag", 1, np.int32(0))
    ins = KW_SMALL
    V = o["V"]
    lay, nW, total = kw_layout(ins, V)
    ar.alloc("a", 4 * 33, np.ones(4 * 33, f32)).alloc("W", nW, np.ones(nW, f32)).alloc("M", 4 * total).alloc("gW", nW).alloc("ga", 4 * 33, np.zeros(4 * 33, f32)).alloc("ws", 4 * 33 * 2)
    ar.upload(dev)
    p, fn = ar.p, c["fn"][4:]
    bl = (_blocks(L, tb["blocks"]), nb)
    nargs = (rows, tb["row_dim"], *bl, o["act"], o["eps"], 1)
    largs = (rows, tb["row_dim"], *bl, p("std"))
    handles = []
    if fn == "act_fwd":
        rc = lib.e3k_act_fwd(p("x"), n, o["act"], o["cst"], p("o1"), st)
    elif fn == "act_bwd":
        rc = lib.e3k_act_bwd(p("x"), p("gy"), n, o["act"], o["cst"], p("o1"), st)
    elif fn == "act_bwd2":
        rc = lib.e3k_act_bwd2(p("x"), p("gy"), p("h"), n, o["act"], o["cst"], p("o1"), p("o2"), st)
    elif fn == "act_bwd_from_output":
        rc = lib.e3k_act_bwd_from_output(p("x"), p("gy"), n, o["act"], o["cst"], p("o1"), st)
    elif fn == "norm_act_fwd":
        rc = lib.e3k_norm_act_fwd(p("x"), *nargs, p("o1"), st)
    elif fn == "norm_act_bwd":
        rc = lib.e3k_norm_act_bwd(p("x"), p("gy"), *nargs, p("o1"), st)
    elif fn == "norm_act_bwd2":
        rc = lib.e3k_norm_act_bwd2(p("x"), p("gy"), p("h"), *nargs, p("o1"), p("o2"), st)
    elif fn == "layernorm_fwd":
        rc = lib.e3k_layernorm_fwd(p("x"), *largs, p("o1"), p("inv"), st)
    elif fn == "layernorm_bwd":
        rc = lib.e3k_layernorm_bwd(p("x"), p("gy"), p("inv"), *largs, p("o1"), p("g_std"), st)
    elif fn == "layernorm_bwd2":
        rc = lib.e3k_layernorm_bwd2(p("x"), p("gy"), p("h"), None, p("inv"), *largs, p("o1"), p("o2"), p("g_std"), st)
    elif fn == "relayout":
        rc = lib.e3k_relayout(p("x"), rows, tb["row_dim"], *bl, 1, p("o1"), st)
    elif fn == "segment_sum":
        rc = lib.e3k_segment_sum(p("x"), p("ptr"), 4, o["dim"], 0, p("o1"), st)
    elif fn == "counts_to_ptr":
        rc = lib.e3k_counts_to_ptr(p("i64"), o["G"], p("ptr"), st)
    elif fn == "onehot":
        rc = lib.e3k_onehot(p("i64"), 4, o["T"], p("o1"), p("flag"), st)
    elif fn == "keyed_weights_fwd":
        rc = lib.e3k_keyed_weights_fwd(p("a"), p("W"), _instr(L, ins, V), len(ins), 4, V, total + o["ld"], p("M"), st)
    elif fn == "keyed_weights_bwd":
        rc = lib.e3k_keyed_weights_bwd(p("a"), p("W"), p("M"), _instr(L, ins, V), len(ins), 4, V, total, p("ga"), p("gW"), 0, p("ws"), st)
    else:
        nl = o["layers"]
        items = (L.KwMultiItem * nl)()
        try:
            for i in range(nl):
                Vi = V + 1 if o["unequal"] and i == 1 else V
                h = C.c_void_p()
                assert lib.e3k_kw_args_create(_instr(L, ins, Vi), len(ins), Vi, kw_layout(ins, Vi)[2], C.byref(h)) == E3K_OK
                handles.append(h)
                items[i].args, items[i].W, items[i].M, items[i].g_W = h, p("W"), p("M"), None
            if fn == "keyed_weights_fwd_multi":
                rc = lib.e3k_keyed_weights_fwd_multi(items, nl, p("a"), 4, st)
            else:
                assert fn == "keyed_weights_bwd_multi"
                assert lib.e3k_keyed_weights_bwd_multi_workspace(items, nl, 4) == 0
                rc = lib.e3k_keyed_weights_bwd_multi(items, nl, p("a"), 4, p("ga"), p("ws"), st)
        finally:
            for h in handles:
                lib.e3k_kw_args_destroy(h)
    assert rc == c["rc"], f"return code {rc}"
    Check(ar, c).finish()


RUNNERS = dict(act=run_act, gate2=run_gate2, na=run_na, ln=run_ln, seg=run_seg, rl=run_rl, c2p=run_c2p, oh=run_oh, kw=run_kw, kwm=run_kwm, refuse=run_refuse)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_node_case_against_float64(dev, c):
    from e3_layers_amd.backend import lib as L

    RUNNERS[c["kind"]](dev, c, L)


def test_workspace_rules_at_their_thresholds(dev):
    """what the two workspace functions expose of the host logic: ceil(total / 256) rows of K * V floats, per layer"""
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    for total, K, V in ((1, 1, 1), (256, 3, 2), (257, 3, 2), (512, 129, 32), (513, 1, 7)):
        ins = _instr(L, [(total, 1)], V)
        assert lib.e3k_keyed_weights_bwd_workspace(ins, 1, K, V) == (total + 255) // 256 * K * V
    ins = _instr(L, KW_SMALL, 3)
    assert lib.e3k_keyed_weights_bwd_workspace(ins, 2, 0, 3) == 0 and lib.e3k_keyed_weights_bwd_workspace(ins, 0, 4, 3) == 0
    assert lib.e3k_keyed_weights_bwd_workspace(None, 2, 4, 3) == 0 and lib.e3k_keyed_weights_bwd_workspace(ins, 2, 4, 0) == 0


def test_python_callers_hand_back_zero_on_uncovered_columns(dev):
    """ops.layer_norm (forward, backward) and ops.norm_activation's double backward on tables with a gap: the columns no block covers
    come back zero, also when the allocator hands out memory that held NaN"""
    from e3_layers_amd.backend import ops

    def poison(shape):      # the next allocations of this size are likely to reuse these bytes
        for _ in range(4):
            t = torch.full(shape, float("nan"), device=dev)
            del t

    tb = TABLES["ln_gap"]
    covered = np.zeros(tb["row_dim"], bool)
    for off, mul, dim in tb["blocks"]:
        covered[off:off + mul * dim] = True
    gap = torch.from_numpy(~covered).to(dev)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(5, tb["row_dim"], generator=gen).to(dev).requires_grad_(True)
    std = torch.rand(len(tb["blocks"]), generator=gen).add(0.5).to(dev).requires_grad_(True)
    poison(x.shape)
    y = ops.layer_norm(x, std, tb["blocks"])
    assert torch.isfinite(y).all() and float(y[:, gap].abs().max()) == 0.0
    poison(x.shape)
    gx, _ = torch.autograd.grad(y, [x, std], torch.ones_like(y))
    assert torch.isfinite(gx).all() and float(gx[:, gap].abs().max()) == 0.0
    tb = TABLES["na_gap"]
    covered = np.zeros(tb["row_dim"], bool)
    for off, mul, dim in tb["blocks"]:
        covered[off:off + mul * dim] = True
    gap = torch.from_numpy(~covered).to(dev)
    x = torch.randn(5, tb["row_dim"], generator=gen).to(dev).requires_grad_(True)
    y = ops.NormActFn.apply(x, tuple(tb["blocks"]), 2, 1e-4, True)
    seed = torch.randn(y.shape, generator=gen).to(dev).requires_grad_(True)
    (g,) = torch.autograd.grad(y, x, seed, create_graph=True)
    poison(x.shape)
    gg_x, gg_s = torch.autograd.grad((g * torch.randn(g.shape, generator=gen).to(dev)).sum(), [x, seed])
    for t in (y, g, gg_x, gg_s):
        assert torch.isfinite(t).all() and float(t[:, gap].abs().max()) == 0.0


def test_zz_worst_ratio_per_family(dev):
    """prints what the cases of this run measured (the module's MEASURED is a copy of a full run's)"""
    for family in sorted(WORST):
        print(f"worst error / bound, {family}: {WORST[family]:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
