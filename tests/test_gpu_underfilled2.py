"""The kernels whose bodies were rescheduled so that their independent loads are in flight together -- the keyed self-connection
weights (forward, weight gradient, attribute gradient: csrc/e3k_node.hip), the knot bins' rank and scan passes and the table
gradient's combine (csrc/e3k_rtable.hip) -- through their C entries, BIT FOR BIT against numpy float32 models that sum in the
kernels' documented orders:

  keyed forward     M[t, c]   = fma chain over v ascending from 0                                  (every key on its own)
  keyed g_W         gv[c, v]  = fma chain over the keys ascending from 0; g_W = old + gv (accumulate) or gv.  Beyond one key tile
                    (65 keys: tiles of 33 and 32) the tiles meet in atomics: held to the float64 bound of tests/test_gpu_node_matrix.py
  keyed g_a         a workspace row per block of 256 columns: out[t, v] = fma chain over the block's columns ascending from 0 (zeros
                    past the last column); then per output lane r sums the rows r, r + 64, ..., the 64 lanes are added as a butterfly
                    (xor 32, 16, .. 1) and g_a += that.  The workspace rows are compared too: their layout is kept.
  bins              bin, coef (float32, operation for operation), the rank inside (chunk of 1 024 edges, knot), the chunk x knot counts
                    after the scan (edges of the knot in the chunks before), bin_ptr, bin_seg, bin_perm: all integers, all exact
  combine           g_T[j] = old or 0, then for k = 0 .. 3 the segments of knot j + 1 - k ascending: += P[segment][k], P read back from
                    the workspace the (unchanged) partial pass of the same call wrote

fma32 rounds once (the float64 product of two float32 is exact; the sum's double rounding is below 2^-52, as in the other models).
Sizes: the key loops take 8 gM values, 4 attribute rows and 4 attributes per block (KW_KB, KW_SB, KW_VC), hence the key counts round 4
and 8 and the attribute widths 1, 20 (five full chunks) and 32; the scan reads 16 chunks per block (E up to 17 chunks + 1); the combine
holds 4 segments per knot in flight (knots of 0, 1, 2, 4, 5 and 11 segments)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.test_gpu_node_matrix import FL, _instr, gamma, kw_layout
from tests.test_gpu_rtable_matrix import SENT, Arena, Check

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
E3K_OK = 0


def fma32(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# keyed weights
LAYERS = [[(3, 5), (1, 16), (7, 32)],      # 255 columns, two instruction boundaries inside the workgroup
          [(8, 32)],                       # 256
          [(1, 1), (8, 32)]]               # 257: a second workgroup with one column, a boundary after the first column


def kw_columns(W, instr, V):
    """W as a [columns, V] matrix"""
    lay, _, total = kw_layout(instr, V)
    Wc = np.zeros((total, V), f32)
    for w_off, m_off, u, w in lay:
        Wc[m_off:m_off + u * w] = W[w_off:w_off + u * V * w].reshape(u, V, w).transpose(0, 2, 1).reshape(u * w, V)
    return Wc


def kw_flat(Gc, instr, V):
    """a [columns, V] matrix in W's layout"""
    lay, nW, _ = kw_layout(instr, V)
    out = np.zeros(nW, Gc.dtype)
    for w_off, m_off, u, w in lay:
        out[w_off:w_off + u * V * w] = Gc[m_off:m_off + u * w].reshape(u, w, V).transpose(0, 2, 1).ravel()
    return out


def kw_model_fwd(a, Wc):
    acc = np.zeros((a.shape[0], Wc.shape[0]), f32)
    for v in range(a.shape[1]):
        acc = fma32(a[:, v:v + 1], Wc[None, :, v], acc)
    return acc


def kw_model_gw(a, gM, t0, t1):
    gv = np.zeros((gM.shape[1], a.shape[1]), f32)
    for t in range(t0, t1):
        gv = fma32(a[t][None, :], gM[t][:, None], gv)
    return gv


def kw_model_ws(gM, Wc):
    """[blocks of 256 columns, K * V]"""
    K, total = gM.shape
    V = Wc.shape[1]
    nb = (total + 255) // 256
    g = np.zeros((K, nb * 256), f32)
    w = np.zeros((nb * 256, V), f32)
    g[:, :total], w[:total] = gM, Wc
    rows = np.zeros((nb, K, V), f32)
    for b in range(nb):
        for col in range(256 * b, 256 * b + 256):
            rows[b] = fma32(g[:, col:col + 1], w[col][None, :], rows[b])
    return rows.reshape(nb, K * V)


def kw_model_ga(old, ws_rows):
    lanes = np.zeros((64, ws_rows.shape[1]), f32)
    for r in range(ws_rows.shape[0]):
        lanes[r % 64] = lanes[r % 64] + ws_rows[r]
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ off]
    return old.ravel() + lanes[0]


def _bits(x):
    return np.ascontiguousarray(x, f32).ravel().view(np.int32)


KW_KEYS = (1, 3, 4, 5, 7, 8, 9, 64, 65)


@pytest.mark.parametrize("V", (1, 20, 32))
@pytest.mark.parametrize("K", KW_KEYS)
def test_keyed_weights_bit_for_bit(dev, K, V):
    from e3_layers_amd.backend import lib as L

    lib, st = L.load(), L.stream_ptr()
    tiles = (K + 63) // 64
    for acc in (0, 1):
        null_w = 1 if (K + acc) % 2 else None      # a layer without g_W inside the multi-layer call
        rng = np.random.default_rng(zlib.crc32(f"kw:{K}:{V}:{acc}".encode()))
        draw = lambda *s: rng.standard_normal(s).astype(f32)
        a, old_ga = draw(K, V), draw(K, V)
        ar = Arena(zlib.crc32(f"kw-arena:{K}:{V}:{acc}".encode()))
        ar.alloc("a", K * V, a).alloc("g_a", K * V, old_ga).alloc("g_a_single", K * V, old_ga)
        lays, inp, handles = [], [], []
        nl = len(LAYERS)
        for i, ins in enumerate(LAYERS):
            _, nW, total = kw_layout(ins, V)
            lays.append((nW, total))
            inp.append(dict(W=draw(nW), gM=draw(K, total), old_gW=draw(nW)))
            ar.alloc(f"W{i}", nW, inp[i]["W"]).alloc(f"M{i}", K * total, f32(np.nan)).alloc(f"gM{i}", K * total, inp[i]["gM"])
            ar.alloc(f"gW{i}", nW, inp[i]["old_gW"])
        ws_rows = sum((t + 255) // 256 for _, t in lays)
        last = nl - 1      # the single-layer entries, on the last layer
        ar.alloc("ws", ws_rows * K * V, f32(np.nan)).alloc("M_single", K * lays[last][1], f32(np.nan)).alloc("gW_single", lays[last][0], inp[last]["old_gW"])
        ar.alloc("ws_single", (lays[last][1] + 255) // 256 * K * V, f32(np.nan)).upload(dev)
        items = (L.KwMultiItem * nl)()
        try:
            for i, ins in enumerate(LAYERS):
                h = C.c_void_p()
                assert lib.e3k_kw_args_create(_instr(L, ins, V), len(ins), V, lays[i][1], C.byref(h)) == E3K_OK
                handles.append(h)
                items[i].args, items[i].W, items[i].M, items[i].accumulate_w = h, ar.p(f"W{i}"), ar.p(f"M{i}"), acc
                items[i].g_W = None if null_w == i else ar.p(f"gW{i}")
            assert lib.e3k_keyed_weights_fwd_multi(items, nl, ar.p("a"), K, st) == E3K_OK
            for i in range(nl):
                items[i].M = ar.p(f"gM{i}")
            assert lib.e3k_keyed_weights_bwd_multi(items, nl, ar.p("a"), K, ar.p("g_a"), ar.p("ws"), st) == E3K_OK
            arr = _instr(L, LAYERS[last], V)
            assert lib.e3k_keyed_weights_fwd(ar.p("a"), ar.p(f"W{last}"), arr, len(LAYERS[last]), K, V, lays[last][1], ar.p("M_single"), st) == E3K_OK
            assert lib.e3k_keyed_weights_bwd(ar.p("a"), ar.p(f"W{last}"), ar.p(f"gM{last}"), arr, len(LAYERS[last]), K, V, lays[last][1],
                                             ar.p("g_a_single"), ar.p("gW_single"), acc, ar.p("ws_single"), st) == E3K_OK
            ck = Check(ar, dict(id=f"kw:{K}:{V}:{acc}"))
        finally:
            for h in handles:
                lib.e3k_kw_args_destroy(h)
        rows_all = []
        for i, ins in enumerate(LAYERS):
            Wc = kw_columns(inp[i]["W"], ins, V)
            ck.exact(f"M{i}", _bits(kw_model_fwd(a, Wc)))
            outs = [f"gW{i}"] if null_w != i else []
            if i == last:
                ck.exact("M_single", _bits(kw_model_fwd(a, Wc)))
                outs.append("gW_single")
            old = inp[i]["old_gW"]
            for name in outs:
                if tiles == 1:
                    gv = kw_flat(kw_model_gw(a, inp[i]["gM"], 0, K), ins, V)
                    ck.exact(name, _bits(old + gv if acc else gv))
                else:      # two key tiles add into the same element with atomics: the float64 bound of an order-free sum of K + 1 terms
                    a64, g64 = a.astype(f64), inp[i]["gM"].astype(f64)
                    want = kw_flat(g64.T @ a64, ins, V) + (old.astype(f64) if acc else 0.0)
                    mag = kw_flat(np.abs(g64).T @ np.abs(a64), ins, V) + (np.abs(old.astype(f64)) if acc else 0.0)
                    ck.close(name, want, gamma(K + 1) * mag + FL, "keyed_g_W_two_tiles")
            rows = kw_model_ws(inp[i]["gM"], Wc)
            rows_all.append(rows)
            if i == last:
                ck.exact("ws_single", _bits(rows))
                ck.exact("g_a_single", _bits(kw_model_ga(old_ga, rows)))
        rows_all = np.concatenate(rows_all)
        ck.exact("ws", _bits(rows_all))
        ck.exact("g_a", _bits(kw_model_ga(old_ga, rows_all)))
        ck.unchanged()      # (a layer without g_W keeps its old values; nothing else in the arena moved)


# ---------------------------------------------------------------------------------------------------------------------------------
# knot bins
def bins_model(r, key, nk, h_inv, K):
    """bin [E] (NaN radii: 1, checked apart), coef [E, 4] in float32 operation for operation, the flag bits"""
    one, h = f32(1), f32(h_inv)
    with np.errstate(invalid="ignore", over="ignore"):
        raw = r.astype(f32) * h
        x = np.where(raw < 0, f32(0), np.where(raw > f32(K), f32(K), raw)).astype(f32)
        i = np.clip(np.where(np.isnan(x), 1.0, np.floor(x.astype(f64))), 1, K - 2).astype(np.int64)
        t = x - i.astype(f32)
        tm1, tm2, tp1 = t - one, t - f32(2), t + one
        sixth, half = f32(1.0 / 6.0), f32(0.5)
        coef = np.stack([-t * tm1 * tm2 * sixth, tp1 * tm1 * tm2 * half, -tp1 * t * tm2 * half, tp1 * t * tm1 * sixth], 1).astype(f32)
    flag = 0
    if key is not None:
        good = (key >= 0) & (key < nk)
        i = i + np.where(good, key, 0) * (K + 1)
        flag = 0 if good.all() else 8
    return i, coef, flag


BINS_E = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 17 * 1024 + 1)
BINS_KINDS = ("uniform", "one_knot", "distinct", "keyed_bad", "nan")


@pytest.mark.parametrize("kind", BINS_KINDS)
@pytest.mark.parametrize("E", BINS_E)
def test_knot_bins_exact(dev, E, kind):
    from e3_layers_amd.backend import lib as L

    lib, st = L.load(), L.stream_ptr()
    K, h_inv = 96, 16.0
    nk = 3 if kind == "keyed_bad" else 1
    KT = nk * (K + 1) - 1
    rng = np.random.default_rng(zlib.crc32(f"bins:{E}:{kind}".encode()))
    h = 1.0 / h_inv
    if kind == "one_knot":
        r = (7 + rng.uniform(0.0, 1.0, E)) * h
    elif kind == "distinct":      # the 64 edges a wave ranks at a time all sit in different knots
        r = np.concatenate([rng.permutation(np.arange(1, K - 1))[:64] for _ in range(E // 64 + 1)])[:E] * h + rng.uniform(0.0, h, E)
    else:
        r = rng.uniform(-0.05, 1.08 * K * h, E)
    r = r.astype(f32)
    if kind == "nan" and E:
        r[rng.permutation(E)[:max(1, E // 50)]] = np.nan
    key = None
    if kind == "keyed_bad":
        key = rng.integers(0, nk, E).astype(np.int64)
        if E:
            key[rng.permutation(E)[:4]] = np.resize([-1, nk, -2 ** 40, 2 ** 33], min(E, 4))
    n_chunks = -(-E // 1024)
    ws_n = int(lib.e3k_rtable_bins_workspace_ints(E, KT))
    assert ws_n == E + n_chunks * (KT + 1)
    ar = Arena(zlib.crc32(f"bins-arena:{E}:{kind}".encode()))
    ar.alloc("r", E, r).alloc("bin", E, np.int32(SENT)).alloc("coef", 4 * E, f32(np.nan)).alloc("ptr", KT + 2, np.int32(SENT))
    ar.alloc("seg", KT + 2, np.int32(SENT)).alloc("perm", E, np.int32(SENT)).alloc("ws", ws_n, np.int32(SENT))
    if key is not None:
        ar.alloc("key", 2 * E, key.view(np.int32), align=2).alloc("flag", 1, np.int32(0x15))
    ar.upload(dev)
    nul = (lambda n: ar.p(n) if E > 0 else None)
    if key is not None:
        rc = lib.e3k_rtable_bins_keyed(nul("r"), nul("key"), nk, E, h_inv, K, nul("bin"), nul("coef"), ar.p("ptr"), ar.p("seg"), nul("perm"),
                                       nul("ws"), ar.p("flag"), st)
    else:
        rc = lib.e3k_rtable_bins(nul("r"), E, h_inv, K, nul("bin"), nul("coef"), ar.p("ptr"), ar.p("seg"), nul("perm"), nul("ws"), st)
    assert rc == E3K_OK
    ck = Check(ar, dict(id=f"bins:{E}:{kind}"))
    b, coef, flag = bins_model(r, key, nk, h_inv, K)
    nan = np.isnan(r)
    if nan.any():      # (the knot of a NaN radius is whatever the cast gives, clamped: any usable knot; its weights are NaN)
        got = ck.dev("bin").astype(np.int64)[nan]
        assert ((got >= 1) & (got <= K - 2)).all()
        b[nan] = got
        got_c = ck.dev("coef", f32).reshape(E, 4)
        assert np.isnan(got_c[nan]).all()
        coef[nan] = got_c[nan]
    ck.exact("bin", b.astype(np.int32))
    ck.exact("coef", coef.view(np.int32))
    if key is not None:
        ck.exact("flag", np.int32(0x15 | flag).reshape(1))
    cnt = np.bincount(b, minlength=KT + 1)
    ck.exact("ptr", np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
    ck.exact("seg", np.concatenate([[0], np.cumsum(-(-cnt // 64))]).astype(np.int32))
    perm = np.argsort(b, kind="stable")
    ck.exact("perm", perm.astype(np.int32))
    # the workspace: rank inside (chunk, knot), then per chunk the edges of every knot in the chunks before it
    chunk = np.arange(E) // 1024
    per_chunk = np.zeros((n_chunks, KT + 1), np.int64)
    np.add.at(per_chunk, (chunk, b), 1)
    before = np.cumsum(per_chunk, 0) - per_chunk
    pos = np.empty(E, np.int64)
    pos[perm] = np.arange(E) - np.cumsum(cnt)[b[perm]] + cnt[b[perm]]      # position inside the knot, edge ids ascending
    lrank = pos - before[chunk, b] if E else pos
    ck.exact("ws", np.concatenate([lrank, before.ravel()]).astype(np.int32))
    ck.unchanged()


# ---------------------------------------------------------------------------------------------------------------------------------
# the table gradient's combine
@pytest.mark.parametrize("accumulate", (0, 1))
@pytest.mark.parametrize("W", (192, 704, 1344))
def test_table_gradient_combine_bit_for_bit(dev, W, accumulate):
    from e3_layers_amd.backend import lib as L

    lib, st = L.load(), L.stream_ptr()
    K, h_inv = 16, 4.0
    rng = np.random.default_rng(zlib.crc32(f"combine:{W}:{accumulate}".encode()))
    # edges per knot -> segments of 64: 0, 1, 2 (65 edges), 4, 5 (one past the four in flight), 11 (two further blocks), next to each other
    per_knot = {2: 700, 3: 65, 4: 64, 6: 256, 7: 300, 9: 1, 13: 130, 14: 3}
    r = np.concatenate([(k + rng.uniform(0.0, 1.0, n)) / h_inv for k, n in per_knot.items()])
    r = rng.permutation(r).astype(f32)
    E = len(r)
    ws_n = int(lib.e3k_rtable_bins_workspace_ints(E, K))
    wsb_n = int(lib.e3k_rtable_bwd_workspace_floats(E, K, W))
    old = rng.standard_normal((K + 1) * W).astype(f32)
    ar = Arena(zlib.crc32(f"combine-arena:{W}:{accumulate}".encode()))
    ar.alloc("r", E, r).alloc("bin", E, np.int32(SENT)).alloc("coef", 4 * E, f32(np.nan)).alloc("ptr", K + 2, np.int32(SENT))
    ar.alloc("seg", K + 2, np.int32(SENT)).alloc("perm", E, np.int32(SENT)).alloc("ws", ws_n, np.int32(SENT))
    ar.alloc("gw", E * W).alloc("wsb", wsb_n, f32(np.nan)).alloc("gT", (K + 1) * W, old if accumulate else f32(np.nan)).upload(dev)
    assert lib.e3k_rtable_bins(ar.p("r"), E, h_inv, K, ar.p("bin"), ar.p("coef"), ar.p("ptr"), ar.p("seg"), ar.p("perm"), ar.p("ws"), st) == E3K_OK
    assert lib.e3k_rtable_interp_bwd(ar.p("gw"), ar.p("coef"), None, ar.p("ptr"), ar.p("seg"), ar.p("perm"), E, K, W, ar.p("wsb"), ar.p("gT"),
                                     accumulate, st) == E3K_OK
    ck = Check(ar, dict(id=f"combine:{W}:{accumulate}"))
    seg = ck.dev("seg").astype(np.int64)
    cnt = np.zeros(K + 1, np.int64)
    for k, n in per_knot.items():
        cnt[k] = n
    assert np.array_equal(seg, np.concatenate([[0], np.cumsum(-(-cnt // 64))]))
    assert sorted(set(np.diff(seg))) == [0, 1, 2, 3, 4, 5, 11]
    P = ck.dev("wsb", f32)[:seg[-1] * 4 * W].reshape(seg[-1], 4, W)
    assert np.isfinite(P).all()
    want = (old.reshape(K + 1, W) if accumulate else np.zeros((K + 1, W), f32)).copy()
    for j in range(K + 1):
        for k in range(4):
            b = j + 1 - k
            if 1 <= b <= K - 2:
                for s in range(seg[b], seg[b + 1]):
                    want[j] = want[j] + P[s, k]
    ck.exact("gT", _bits(want))
    for name in ("bin", "coef", "ptr", "seg", "perm", "ws", "wsb"):
        ck.free(name, ar.blocks[name][1])
    ck.unchanged()


# ---------------------------------------------------------------------------------------------------------------------------------
# rows grouped by key
GROUP_KINDS = ("mixed", "absent_key", "one_key", "bad_key")


@pytest.mark.parametrize("kind", GROUP_KINDS)
@pytest.mark.parametrize("R", (1, 1023, 1024, 1025, 4 * 1024 + 1))
def test_group_rows_exact(dev, R, kind):
    """perm: the rows by key, ascending row id inside a key (stable); bounds {start, count}; reps: a key's first row, 0 for an absent
    key; the flag: 1 when a key is outside [0, K) (such rows are placed nowhere).  R: up to one past the four keys a thread counts at a
    time (4 096 rows), and round the chunk of 1 024 rows whose successor's keys are requested ahead."""
    from e3_layers_amd.backend import lib as L

    lib, st = L.load(), L.stream_ptr()
    K = 7
    rng = np.random.default_rng(zlib.crc32(f"group:{R}:{kind}".encode()))
    key = rng.integers(0, K, R).astype(np.int64)
    if kind == "absent_key":
        key[key == 3] = 4
    elif kind == "one_key":
        key[:] = 5
    elif kind == "bad_key":
        key[rng.permutation(R)[:3]] = np.resize([-1, K, 2 ** 40], min(R, 3))
    ar = Arena(zlib.crc32(f"group-arena:{R}:{kind}".encode()))
    ar.alloc("key", 2 * R, key.view(np.int32), align=2).alloc("perm", R, np.int32(SENT)).alloc("bounds", 2 * K, np.int32(SENT))
    ar.alloc("reps", 2 * K, np.int32(SENT), align=2).alloc("bad", 1, np.int32(SENT)).upload(dev)
    assert lib.e3k_group_rows(ar.p("key"), R, K, ar.p("perm"), ar.p("bounds"), ar.p("reps"), ar.p("bad"), st) == E3K_OK
    ck = Check(ar, dict(id=f"group:{R}:{kind}"))
    good = (key >= 0) & (key < K)
    rows = np.flatnonzero(good)
    perm = rows[np.argsort(key[rows], kind="stable")]
    cnt = np.bincount(key[rows], minlength=K)
    start = np.cumsum(cnt) - cnt
    ck.exact("perm", perm.astype(np.int32))      # (the words behind the placed rows keep their bits: checked by `unchanged`)
    ck.exact("bounds", np.stack([start, cnt], 1).astype(np.int32))
    ck.exact("reps", np.where(cnt > 0, perm[np.minimum(start, max(len(perm) - 1, 0))] if len(perm) else 0, 0).astype(np.int64).view(np.int32))
    ck.exact("bad", np.int32(0 if good.all() else 1).reshape(1))
    ck.unchanged()
