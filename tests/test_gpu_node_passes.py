"""The node-side passes that have more than one form, every form against float64 on the CPU: the Gate kernels of csrc/e3k_node.hip
(scalar forms and 16-byte forms, both output layouts) and the fused hidden chain of the radial MLP of csrc/e3k_mlp.hip (64-row and
16-row tiles; its bounds are in the docstrings of its two reference functions below).

Gates.  Every case runs one C-ABI call on buffers that sit inside a NaN-filled arena with slack on both sides, compares what the call writes
with a float64 reference built from the formulas of include/e3k.h, and checks that the slack kept its bits.  A base pointer 4 bytes
past a 16-byte boundary ("mis") sends the same values through the scalar form; the two forms must then agree bit for bit (same
per-element arithmetic, same order of the dot over m).

Bounds, per element, from the count of rounded operations (u = 2^-24).

* sigmoid(x) = rcp(1 + exp(-x)) on hardware transcendentals: exp(-x) = exp2(-x log2 e), the rounded product moves the result by
  1.45 |x| u relative, v_exp_f32 and v_rcp_f32 are 1 ulp each, the sum one rounding: relative error below E(x) = (1.5 |x| + 6) u.
  tanhf is within 3 ulp, below E as well.
* act(x) (silu = x sigmoid, tanhlu = tanh |x|, tanh): one more product: |error| <= (E(x) + 2u) |act(x)|.
* act'(x): silu' = s (1 + x (1 - s)) and tanhlu' = (1 - th^2) |x| + th sign(x) cancel, so the bound is absolute.  1 - s and 1 - th^2
  carry (E + 2u) absolute, the product with x and the sum two roundings of at most (1 + |x|): below D(x) = (2 x^2 + 10 |x| + 10) u.
* forward: scalars y = c act(x): c (err_act + u |act|).  Gated y = x (c act(g)): |x| c (err_act(g) + 2u |act(g)|).
* backward, G = g_y + g_y2 (one rounding, u (|g_y| + |g_y2|)):
    scalars  G c act'(x):     u (|g_y| + |g_y2|) c |act'| + |G| c (D + 2u |act'|)
    gated    G (c act(g)):    u (|g_y| + |g_y2|) c |act| + |G| c (err_act + 2u |act|)
    gates    (sum_m G_m x_m) c act'(g): the FMA chain of dim terms errs by at most sum_m u (|g_y| + |g_y2|)_m |x_m| + dim u S with
             S = sum_m |G_m x_m|; then (that) c |act'| + S c (D + 2u |act'|).
A misplaced channel, component or segment moves an element by a whole term, about 1e6 times these bounds.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 1e-37      # room for results that underflow


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference of the activations and the error terms of their fp32 forms
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _ssp(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))) - np.log(2.0)


def _act(a, x):
    """activation ids of csrc/e3k_act.h: 0 identity, 1 ssp, 2 silu, 3 tanhlu, 4 tanh, 5 abs (only the one asked for is evaluated)"""
    return {0: lambda: x + 0.0, 1: lambda: _ssp(x), 2: lambda: x * _sig(x), 3: lambda: np.tanh(x) * np.abs(x), 4: lambda: np.tanh(x),
            5: lambda: np.abs(x)}[a]()


def _dact(a, x):
    if a in (0, 1, 5):
        return {0: lambda: np.ones_like(x), 1: lambda: _sig(x), 5: lambda: np.sign(x)}[a]()
    if a == 2:
        s = _sig(x)
        return s * (1.0 + x * (1.0 - s))
    th = np.tanh(x)
    return (1.0 - th * th) * np.abs(x) + th * np.sign(x) if a == 3 else 1.0 - th * th


def _err_act(a, x):
    """identity and abs are exact; ssp = max(x, 0) + log(1 + exp(-|x|)) - ln 2 cancels at 0: ABSOLUTE (2 |x| + 8) u (the derivation is
    in the docstring of tests/test_gpu_node_matrix.py); its derivative is the sigmoid, inside D(x) below like the others"""
    if a in (0, 5):
        return np.zeros_like(x)
    if a == 1:
        return (2.0 * np.abs(x) + 8.0) * U
    return ((1.5 * np.abs(x) + 6.0) * U + 2.0 * U) * np.abs(_act(a, x))


def _err_dact(x):
    return (2.0 * x * x + 10.0 * np.abs(x) + 10.0) * U


# ---------------------------------------------------------------------------------------------------------------------------------
# segment tables: (kind, in_off, gate_off, out_off, mul, dim, act, cst)
C2, C3, C4 = 1.6791767923989418, 1.1501944455736173, 1.5925374197228312
SPECS = {
    # the Gate of a config_energy layer at l_max 2: 64 channels everywhere
    "layer": dict(in_dim=1408, out_dim=1152, vec=(1, 1), segs=[
        (0, 0, 0, 0, 64, 1, 2, C2), (0, 64, 0, 64, 64, 1, 3, C3), (1, 384, 128, 128, 64, 3, 2, C2), (1, 576, 192, 320, 64, 3, 2, C2),
        (1, 768, 256, 512, 64, 5, 2, C2), (1, 1088, 320, 832, 64, 5, 2, C2)]),
    # channel counts whose quads are no power of two, a gated scalar (dim 1) and dim 7; the segments are listed out of row order
    "odd_quads": dict(in_dim=184, out_dim=148, vec=(1, 1), segs=[
        (1, 148, 24, 104, 12, 3, 2, C2), (0, 0, 0, 0, 8, 1, 4, C4), (1, 80, 12, 36, 8, 5, 3, C3), (1, 52, 8, 8, 4, 7, 2, C2),
        (1, 120, 20, 76, 4, 7, 4, C4), (1, 44, 36, 140, 8, 1, 2, C2)]),
    # 6 channels: nothing is 16-byte aligned, scalar forms both ways
    "mul6": dict(in_dim=66, out_dim=54, vec=(0, 0), segs=[
        (0, 0, 0, 0, 6, 1, 2, C2), (1, 18, 6, 6, 6, 3, 2, C2), (1, 36, 12, 24, 6, 5, 3, C3)]),
    # input columns 8..15 feed nothing (their gradient is zero): the backward stays scalar, the forward tiles its output row
    "in_gap": dict(in_dim=48, out_dim=32, vec=(1, 0), segs=[(0, 0, 0, 0, 8, 1, 2, C2), (1, 24, 16, 8, 8, 3, 2, C2)]),
    # output columns 8..11 are written by nobody (zero): the forward stays scalar, the backward tiles its input row
    "out_gap": dict(in_dim=40, out_dim=36, vec=(0, 1), segs=[(0, 0, 0, 0, 8, 1, 3, C3), (1, 16, 8, 12, 8, 3, 2, C2)]),
    # a gated block of dim 9 has no 16-byte form
    "dim9": dict(in_dim=44, out_dim=40, vec=(0, 0), segs=[(0, 0, 0, 0, 4, 1, 2, C2), (1, 8, 4, 4, 4, 9, 2, C2)]),
}
ROWS = (0, 1, 7, 4704)


def _seg_array(L, segs):
    arr = (L.GateSeg * len(segs))()
    for i, s in enumerate(segs):
        (arr[i].kind, arr[i].in_off, arr[i].gate_off, arr[i].out_off, arr[i].mul, arr[i].dim, arr[i].act, arr[i].cst) = s
    return arr


def _out_view(block, mul, dim, cf):
    """[rows, mul*dim] of an output row -> [rows, dim, mul]"""
    r = block.shape[0]
    return block.reshape(r, dim, mul) if cf else block.reshape(r, mul, dim).transpose(0, 2, 1)


def _ref_fwd(x, spec, cf):
    rows = x.shape[0]
    y = np.zeros((rows, spec["out_dim"]))
    bound = np.zeros_like(y)
    for kind, io, go, oo, mul, dim, act, cst in spec["segs"]:
        cst = float(np.float32(cst))      # the constant as the kernels hold it
        if kind == 0:
            xs = x[:, io:io + mul]
            y[:, oo:oo + mul] = cst * _act(act, xs)
            bound[:, oo:oo + mul] = cst * (_err_act(act, xs) + U * np.abs(_act(act, xs)))
        else:
            xb = x[:, io:io + mul * dim].reshape(rows, dim, mul)
            g = x[:, go:go + mul][:, None, :]
            v = xb * (cst * _act(act, g))
            b = np.abs(xb) * cst * (_err_act(act, g) + 2 * U * np.abs(_act(act, g)))
            if not cf:
                v, b = v.transpose(0, 2, 1), b.transpose(0, 2, 1)
            y[:, oo:oo + mul * dim] = v.reshape(rows, mul * dim)
            bound[:, oo:oo + mul * dim] = b.reshape(rows, mul * dim)
    return y, bound + TINY


def _ref_bwd(x, gy, gy2, spec, cf):
    rows = x.shape[0]
    gx = np.zeros((rows, spec["in_dim"]))
    bound = np.zeros_like(gx)
    G = gy if gy2 is None else gy + gy2
    Ga = np.abs(gy) if gy2 is None else np.abs(gy) + np.abs(gy2)      # what the one rounding of the sum is relative to
    ru = 0.0 if gy2 is None else U
    for kind, io, go, oo, mul, dim, act, cst in spec["segs"]:
        cst = float(np.float32(cst))      # the constant as the kernels hold it
        if kind == 0:
            xs, g, ga = x[:, io:io + mul], G[:, oo:oo + mul], Ga[:, oo:oo + mul]
            da = _dact(act, xs)
            gx[:, io:io + mul] = g * cst * da
            bound[:, io:io + mul] = ru * ga * cst * np.abs(da) + np.abs(g) * cst * (_err_dact(xs) + 2 * U * np.abs(da))
        else:
            xb = x[:, io:io + mul * dim].reshape(rows, dim, mul)
            gt = x[:, go:go + mul]
            g = _out_view(G[:, oo:oo + mul * dim], mul, dim, cf)
            ga = _out_view(Ga[:, oo:oo + mul * dim], mul, dim, cf)
            a, da = _act(act, gt), _dact(act, gt)
            gx[:, io:io + mul * dim] = (g * (cst * a)[:, None, :]).reshape(rows, mul * dim)
            bound[:, io:io + mul * dim] = (ru * ga * cst * np.abs(a)[:, None, :]
                                           + np.abs(g) * cst * (_err_act(act, gt) + 2 * U * np.abs(a))[:, None, :]).reshape(rows, mul * dim)
            S = (np.abs(g * xb)).sum(1)
            gx[:, go:go + mul] = (g * xb).sum(1) * cst * da
            bound[:, go:go + mul] = ((ru * ga * np.abs(xb)).sum(1) + dim * U * S) * cst * np.abs(da) \
                + S * cst * (_err_dact(gt) + 2 * U * np.abs(da))
    return gx, bound + TINY


class _Arena:
    """float32 buffers inside one NaN-filled allocation: 64 floats of slack around each, bases 16-byte aligned or 4 bytes past."""

    def __init__(self, dev, mis):
        self.dev, self.mis, self.items = dev, mis, []

    def add(self, values):
        self.items.append(np.ascontiguousarray(values, dtype=np.float32).ravel())
        return len(self.items) - 1

    def build(self):
        offs, at = [], 64
        for v in self.items:
            at = (at + 3) // 4 * 4 + (1 if self.mis else 0)
            offs.append(at)
            at += v.size + 64
        host = np.full(at + 4, np.nan, dtype=np.float32)
        for o, v in zip(offs, self.items):
            host[o:o + v.size] = v
        self.host, self.offs = host, offs
        self.buf = torch.from_numpy(host.copy()).to(self.dev)
        assert self.buf.data_ptr() % 16 == 0
        return self

    def ptr(self, i):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.offs[i])

    def read(self, i):
        self.after = self.buf.cpu().numpy()
        return self.after[self.offs[i]:self.offs[i] + self.items[i].size]

    def untouched_except(self, i):
        keep = np.ones(self.host.size, dtype=bool)
        keep[self.offs[i]:self.offs[i] + self.items[i].size] = False
        return np.array_equal(self.after[keep].view(np.uint32), self.host[keep].view(np.uint32))


def _inputs(name, rows, spec):
    rng = np.random.default_rng(zlib.crc32(f"{name}:{rows}".encode()))
    x = rng.standard_normal((rows, spec["in_dim"])).astype(np.float32)
    gy = rng.standard_normal((rows, spec["out_dim"])).astype(np.float32)
    gy2 = rng.standard_normal((rows, spec["out_dim"])).astype(np.float32)
    return x, gy, gy2


def _run_fwd(dev, L, spec, x, cf, mis):
    rows = x.shape[0]
    ar = _Arena(dev, mis)
    ix, iy = ar.add(x), ar.add(np.full((rows, spec["out_dim"]), np.nan, dtype=np.float32))
    ar.build()
    rc = L.load().e3k_gate_fwd(ar.ptr(ix), rows, spec["in_dim"], spec["out_dim"], _seg_array(L, spec["segs"]), len(spec["segs"]),
                               int(cf), ar.ptr(iy), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    y = ar.read(iy).reshape(rows, spec["out_dim"]).copy()
    assert ar.untouched_except(iy), "gate_fwd wrote outside its output"
    return y


def _run_bwd(dev, L, spec, x, gy, gy2, cf, mis):
    rows = x.shape[0]
    ar = _Arena(dev, mis)
    ix, ig = ar.add(x), ar.add(gy)
    ig2 = ar.add(gy2) if gy2 is not None else None
    io = ar.add(np.full((rows, spec["in_dim"]), np.nan, dtype=np.float32))
    ar.build()
    rc = L.load().e3k_gate_bwd(ar.ptr(ix), ar.ptr(ig), ar.ptr(ig2) if gy2 is not None else None, rows, spec["in_dim"],
                               spec["out_dim"], _seg_array(L, spec["segs"]), len(spec["segs"]), int(cf), ar.ptr(io), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    gx = ar.read(io).reshape(rows, spec["in_dim"]).copy()
    assert ar.untouched_except(io), "gate_bwd wrote outside its output"
    return gx


def _check(got, ref, bound, what):
    assert not np.isnan(got).any(), f"{what}: an element was not written"
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: max error / bound {worst:.3f}, max |error| {float(err.max()) if err.size else 0.0:.3e}")
    assert worst <= 1.0, f"{what}: error {worst:.2f} times the bound"


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cf", (0, 1), ids=("e3nn", "cf"))
@pytest.mark.parametrize("name", sorted(SPECS))
def test_gate_forward(dev, name, cf, rows):
    from e3_layers_amd.backend import lib as L

    spec = SPECS[name]
    assert L.load().e3k_gate_path(spec["in_dim"], spec["out_dim"], _seg_array(L, spec["segs"]), len(spec["segs"]), 0) == spec["vec"][0]
    x, _, _ = _inputs(name, rows, spec)
    ref, bound = _ref_fwd(x.astype(np.float64), spec, cf)
    got = {mis: _run_fwd(dev, L, spec, x, cf, mis) for mis in (False, True)}
    for mis in (False, True):
        _check(got[mis], ref, bound, f"gate_fwd {name} {'cf' if cf else 'e3nn'} rows {rows} {'misaligned' if mis else 'aligned'}")
    assert np.array_equal(got[False].view(np.uint32), got[True].view(np.uint32)), "the 16-byte and the scalar form differ in bits"


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("two", (False, True), ids=("gy", "gy+gy2"))
@pytest.mark.parametrize("cf", (0, 1), ids=("e3nn", "cf"))
@pytest.mark.parametrize("name", sorted(SPECS))
def test_gate_backward(dev, name, cf, two, rows):
    from e3_layers_amd.backend import lib as L

    spec = SPECS[name]
    assert L.load().e3k_gate_path(spec["in_dim"], spec["out_dim"], _seg_array(L, spec["segs"]), len(spec["segs"]), 1) == spec["vec"][1]
    x, gy, gy2 = _inputs(name, rows, spec)
    if not two:
        gy2 = None
    ref, bound = _ref_bwd(x.astype(np.float64), gy.astype(np.float64), None if gy2 is None else gy2.astype(np.float64), spec, cf)
    got = {mis: _run_bwd(dev, L, spec, x, gy, gy2, cf, mis) for mis in (False, True)}
    for mis in (False, True):
        _check(got[mis], ref, bound, f"gate_bwd {name} {'cf' if cf else 'e3nn'} rows {rows} {'misaligned' if mis else 'aligned'}")
    assert np.array_equal(got[False].view(np.uint32), got[True].view(np.uint32)), "the 16-byte and the scalar form differ in bits"


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused hidden chain of the radial MLP (csrc/e3k_mlp.hip): 64-row and 16-row tiles
MLP_SHAPES = {
    # (k0, h, hidden layers, act, cst)
    "radial": (8, 64, 3, 2, C2),          # config_energy: 8 radial basis functions, 64 hidden, silu
    "narrow": (10, 32, 2, 3, C3),         # k0 no multiple of 4 (scalar tile load, zero-padded k), two of the four waves idle
}
MLP_ROWS = (1, 63, 64, 65, 513, 16400, 70656)      # 16400 rows of one net: 257 tiles of 64, the last with 16 rows
LIP = 1.2      # |silu'| <= 1.0999, |tanhlu'| <= 1.2 (numerically: max over x of (1 - th^2)|x| + |th| is 1.1997 at |x| = 1.54)


def _mlp_forward_ref(x, Ws, alphas, act, cst):
    """float64 chain and, per layer, the bound on |z - z_ref| and |h - h_ref|: a sum of K products in fp32 FMA chains (two
    accumulators and the alpha scaling: K + 3 roundings) on inputs that carry the previous layer's error; h = cst act(z) moves by
    at most LIP times the error of z, plus the activation's own error and one product."""
    prev, dprev, zs, dzs = x, np.zeros_like(x), [], []
    for W, al in zip(Ws, alphas):
        K = W.shape[0]
        z = al * (prev @ W)
        dz = al * (dprev @ np.abs(W)) + (K + 3) * U * al * (np.abs(prev) @ np.abs(W)) + TINY
        zs.append(z), dzs.append(dz)
        prev = cst * _act(act, z)
        dprev = cst * (LIP * dz + _err_act(act, z) + U * np.abs(_act(act, z)))
    return zs, dzs, prev, dprev + TINY


def _mlp_backward_ref(x, Ws, alphas, act, cst, zs, g):
    """float64 backward FROM the fp32 pre-activations the kernel is given (inputs of the call), with bounds: gz = g cst act'(z)
    (the gate backward's terms), the input h_{l-1} = cst act(z_{l-1}) re-formed in fp32 (err_act + one product), weight gradients
    summed over R rows in MFMA chains and atomics (R + 4 roundings of sum |h| |gz|), dgrad over h columns (h + 3)."""
    L, R = len(Ws), x.shape[0]
    gWs, dgWs = [None] * L, [None] * L
    dg = np.zeros_like(g)
    for l in range(L - 1, -1, -1):
        W, al, z = Ws[l], alphas[l], zs[l]
        D = cst * _dact(act, z)
        eD = cst * (_err_dact(z) + U * np.abs(_dact(act, z)))
        gz = g * D
        dgz = dg * np.abs(D) + np.abs(g) * eD + U * np.abs(gz)
        if l > 0:
            H = cst * _act(act, zs[l - 1])
            eH = cst * (_err_act(act, zs[l - 1]) + U * np.abs(_act(act, zs[l - 1])))
        else:
            H, eH = x, np.zeros_like(x)
        gWs[l] = al * (H.T @ gz)
        dgWs[l] = al * (eH.T @ np.abs(gz) + np.abs(H).T @ dgz + (R + 4) * U * (np.abs(H).T @ np.abs(gz))) + TINY
        h = W.shape[1]
        g, dg = al * (gz @ W.T), al * (dgz @ np.abs(W).T + (h + 3) * U * (np.abs(gz) @ np.abs(W).T))
    return gWs, dgWs, g, dg + TINY


@pytest.mark.parametrize("nets", (1, 5))
@pytest.mark.parametrize("rows", MLP_ROWS)
@pytest.mark.parametrize("shape", sorted(MLP_SHAPES))
def test_mlp_hidden_chain(dev, shape, rows, nets):
    from e3_layers_amd.backend import lib as L

    k0, h, nl, act, cst = MLP_SHAPES[shape]
    lib = L.load()
    tiles64 = (rows + 63) // 64
    assert lib.e3k_mlp_tile_rows(rows, nets) == (16 if tiles64 * nets < 256 else 64)
    rng = np.random.default_rng(zlib.crc32(f"mlp:{shape}:{rows}:{nets}".encode()))
    x = rng.standard_normal((rows, k0)).astype(np.float32)
    alphas = [1.0 / np.sqrt(k0)] + [1.0 / np.sqrt(h)] * (nl - 1)
    alphas32 = (C.c_float * nl)(*alphas)
    alphas = [float(np.float32(a)) for a in alphas]
    cst32 = float(np.float32(cst))
    PAD = 8      # NaN rows behind every output: a tile's tail must not be written
    xd = torch.from_numpy(x).to(dev)

    def out_buf(cols):
        return torch.full((rows + PAD, cols), float("nan"), device=dev, dtype=torch.float32)

    nets_c = (L.MlpNet * nets)()
    Ws, zb, ob, gob, gwb, gxb = [], [], [], [], [], []
    for i in range(nets):
        W = [rng.standard_normal((k0 if l == 0 else h, h)).astype(np.float32) for l in range(nl)]
        Wd = [torch.from_numpy(w).to(dev) for w in W]
        Ws.append((W, Wd))
        zb.append([out_buf(h) for _ in range(nl)]), ob.append(out_buf(h))
        gob.append(torch.from_numpy(rng.standard_normal((rows, h)).astype(np.float32)).to(dev))
        gwb.append([torch.zeros_like(w) for w in Wd]), gxb.append(out_buf(k0))
        for l in range(nl):
            nets_c[i].weights[l], nets_c[i].z[l], nets_c[i].g_weights[l] = Wd[l].data_ptr(), zb[i][l].data_ptr(), gwb[i][l].data_ptr()
        nets_c[i].out, nets_c[i].g_out, nets_c[i].g_x = ob[i].data_ptr(), gob[i].data_ptr(), gxb[i].data_ptr()

    def ptrs(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    if nets == 1:      # the single-net entry points
        assert lib.e3k_mlp_hidden_fwd(L.ptr(xd), rows, k0, h, nl, ptrs(Ws[0][1]), alphas32, act, cst32, ptrs(zb[0]), L.ptr(ob[0]),
                                      L.stream_ptr()) == 0
        assert lib.e3k_mlp_hidden_bwd(L.ptr(xd), rows, k0, h, nl, ptrs(Ws[0][1]), alphas32, act, cst32, ptrs(zb[0]), L.ptr(gob[0]),
                                      ptrs(gwb[0]), L.ptr(gxb[0]), L.stream_ptr()) == 0
    else:
        assert lib.e3k_mlp_hidden_fwd_multi(nets_c, nets, L.ptr(xd), rows, k0, h, nl, alphas32, act, cst32, L.stream_ptr()) == 0
        assert lib.e3k_mlp_hidden_bwd_multi(nets_c, nets, L.ptr(xd), rows, k0, h, nl, alphas32, act, cst32, L.stream_ptr()) == 0
    torch.cuda.synchronize()

    x64 = x.astype(np.float64)
    for i in range(nets):
        W64 = [w.astype(np.float64) for w in Ws[i][0]]
        zs, dzs, out, dout = _mlp_forward_ref(x64, W64, alphas, act, cst32)
        tag = f"mlp {shape} rows {rows} net {i + 1}/{nets}"
        z_got = [b.cpu().numpy() for b in zb[i]]
        for l in range(nl):
            assert np.isnan(z_got[l][rows:]).all(), f"{tag}: z[{l}] written behind the last row"
            _check(z_got[l][:rows], zs[l], dzs[l], f"{tag} z[{l}]")
        o = ob[i].cpu().numpy()
        assert np.isnan(o[rows:]).all(), f"{tag}: out written behind the last row"
        _check(o[:rows], out, dout, f"{tag} out")
        gWs, dgWs, gx, dgx = _mlp_backward_ref(x64, W64, alphas, act, cst32, [z[:rows].astype(np.float64) for z in z_got],
                                               gob[i].cpu().numpy().astype(np.float64))
        for l in range(nl):
            _check(gwb[i][l].cpu().numpy(), gWs[l], dgWs[l], f"{tag} g_W[{l}]")
        gxg = gxb[i].cpu().numpy()
        assert np.isnan(gxg[rows:]).all(), f"{tag}: g_x written behind the last row"
        _check(gxg[:rows], gx, dgx, f"{tag} g_x")
