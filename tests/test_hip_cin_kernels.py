"""Every kernel of the compressed interaction network (csrc/cin.hip, cin_bs.hip, cin_last.hip) ALONE against a float64
restatement of its operation, at the shapes where its tiling changes.

The bar is derived, not tuned.  Every output element e is a K-term sum of three-factor products; A[e] is the same sum
with every operand replaced by its absolute value (|G| = |g_out| + |g_pool|, |bias| added), computed in float64, and

    |got[e] - ref[e]|  <=  gamma * A[e],      gamma = 3 u + (K + 3) 2^-24

is the textbook worst case of a K-term fp32 accumulation of such products, u being the product error of the form
(include/rec_pangu_hip.h): 2^-23 for the f32 kernels, the per-channel bf16 ("bs") kernels, the collapsed last layer and
the pair kernels under bf16x6; 2^-16 for the pair kernels under bf16x3; 2^-8 under bf16.  K counts the terms of the
sum as written in _K below (a gradient that reaches X_0 in both roles counts both).  Each test prints
max(err / (gamma A)) per output.

Inputs: X_0 and X_{k-1} are drawn around 0.3 (pooled sums do not cancel), W is not symmetric in (h, m), bias / g_out /
g_pool are unrelated normals.  Rows live in wider buffers whose extra columns hold 1e6 on the input side (a kernel may
load them only against a zero weight) and NaN on the side of outputs written in place.

The CPU test at the end applies six small faults to the float64 references and asserts that the bar notices each one."""
import functools
import types

import pytest
import torch

from conftest import require_gpu

DEV = "cuda"
U_F32, U_X3, U_BF16 = 2.0 ** -23, 2.0 ** -16, 2.0 ** -8
PAIR_U = {"bf16x6": U_F32, "bf16x3": U_X3, "bf16": U_BF16}


@pytest.fixture(scope="module")
def hip():
    require_gpu()
    from rec_pangu_amd import hip as h
    h.lib()
    return h


def gamma(u: float, K: int) -> float:
    return 3.0 * u + (K + 3) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ float64 references
def _prod(X0, Xp):
    return X0.unsqueeze(2) * Xp.unsqueeze(1)  # [B, H, M, D]


def ref_fwd(X0, Xp, W, bias):
    """out[b,o,d] = bias[o] + sum_{h,m} W[o,h,m] X0[b,h,d] Xp[b,m,d];  pooled[b,o] = sum_d out[b,o,d]"""
    out = torch.einsum("ohm,bhmd->bod", W, _prod(X0, Xp))
    if bias is not None:
        out = out + bias.view(1, -1, 1)
    return out, out.sum(-1)


def ref_G(g_out, g_pool, D):
    if g_out is None:
        return g_pool.unsqueeze(-1).expand(-1, -1, D)
    return g_out if g_pool is None else g_out + g_pool.unsqueeze(-1)


def ref_bwd_x(X0, Xp, W, G):
    """dX0[b,h,d] = sum_{o,m} G W[o,h,m] Xp[b,m,d];  dXp[b,m,d] = sum_{o,h} G W[o,h,m] X0[b,h,d]"""
    U = torch.einsum("bod,ohm->bhmd", G, W)
    return torch.einsum("bhmd,bmd->bhd", U, Xp), torch.einsum("bhmd,bhd->bmd", U, X0)


def ref_bwd_w(X0, Xp, G):
    """dW[o,h,m] = sum_{b,d} G X0[b,h,d] Xp[b,m,d];  db[o] = sum_{b,d} G"""
    return torch.einsum("bod,bhmd->ohm", G, _prod(X0, Xp)), G.sum((0, 2))


def ref_last_fwd(X0, Xp, V):
    """p[b] = sum_{d,h,m} V[h,m] X0[b,h,d] Xp[b,m,d]"""
    return torch.einsum("hm,bhmd->b", V, _prod(X0, Xp))


def ref_last_bwd_x(X0, Xp, V, g):
    """dX0 = g[b] sum_m V[h,m] Xp;  dXp = g[b] sum_h V[h,m] X0"""
    gb = g.view(-1, 1, 1)
    return gb * torch.einsum("hm,bmd->bhd", V, Xp), gb * torch.einsum("hm,bhd->bmd", V, X0)


def ref_last_bwd_v(X0, Xp, g):
    """dV[h,m] = sum_{b,d} g[b] X0[b,h,d] Xp[b,m,d]"""
    return torch.einsum("b,bhmd->hm", g, _prod(X0, Xp))


def _abs(*ts):
    return [None if t is None else t.abs() for t in ts]


def _K(kind, B, H, M, O, D):
    """terms summed into one element of each output"""
    return {"out": H * M + 1, "pooled": D * (H * M + 1), "dx0": O * M, "dxp": O * H, "dx_both": 2 * O * H,
            "dw": B * D, "db": B * D, "p": D * H * M, "last_dx0": M, "last_dxp": H, "dv": B * D}[kind]


# ------------------------------------------------------------------------------------------------ inputs (CPU, shared)
@functools.lru_cache(maxsize=None)
def _case(B, H, M, O, D, same=False):
    """seeded fp32 operands of one layer, never modified; .d holds their float64 copies"""
    g = torch.Generator().manual_seed(((B * 131 + H) * 131 + M) * 131 * 131 + O * 131 + D + (7 if same else 0))
    c = types.SimpleNamespace(B=B, H=H, M=M, O=O, D=D, same=same)
    c.X0 = 0.3 + 0.5 * torch.randn(B, H, D, generator=g)
    c.Xp = c.X0 if same else 0.3 + 0.5 * torch.randn(B, M, D, generator=g)
    c.W = 0.5 * torch.randn(O, H, M, generator=g)
    c.bias = torch.randn(O, generator=g)
    c.g_out = torch.randn(B, O, D, generator=g)
    c.g_pool = torch.randn(B, O, generator=g)
    c.g = torch.randn(B, generator=g)             # the collapsed last layer's upstream gradient
    c.V = 0.5 * torch.randn(H, M, generator=g)    # ... and its weights
    c.d = types.SimpleNamespace(**{k: v.double() for k, v in vars(c).items() if torch.is_tensor(v)})
    if same:
        c.d.Xp = c.d.X0
    return c


GMODES = ("both", "g_out", "g_pool")


def _grads(c, gmode):
    """(g_out, g_pool) fp32 and the float64 G, |G| of a gradient mode"""
    go = None if gmode == "g_pool" else c.g_out
    gp = None if gmode == "g_out" else c.g_pool
    G = ref_G(None if go is None else c.d.g_out, None if gp is None else c.d.g_pool, c.D)
    Ga = ref_G(None if go is None else c.d.g_out.abs(), None if gp is None else c.d.g_pool.abs(), c.D)
    return go, gp, G, Ga


# the listed shapes (B, H, M, O, D): the smallest that reach each boundary
BS_FWD = [
    (9, 26, 26, 8, 64, True),      # two full workgroups of 4 samples + one tail sample (FULL + guarded launches)
    (3, 26, 16, 8, 64, False),     # tail only
    (17, 32, 32, 4, 32, False),    # both dimension limits, D = 32: 8 samples per workgroup, two FULL + one tail sample
    (8, 1, 1, 5, 32, False),       # O % 4 != 0: everything in the guarded instantiation
    (5, 7, 32, 137, 64, False),    # more than 128 channels, ragged last group of four
]
BS_BWD_X_RC = [(26, 16), (16, 26), (32, 1), (1, 32), (26, 26)]
BS_BWD_X_BD = [(3, 64), (9, 64), (17, 32)]
BS_BWD_X_O = (5, 8, 40)
# (B, H, M, O, D, xp is x0, want_bias, gradient mode): every listed value appears, not every combination
BS_BWD_W = [
    (1, 26, 26, 1, 64, True, True, "both"),
    (5, 26, 16, 16, 32, False, True, "g_out"),
    (257, 26, 26, 17, 64, True, True, "both"),      # 257: two samples per chunk, a one-sample last chunk
    (257, 7, 32, 16, 32, False, False, "g_pool"),
    (5, 32, 32, 137, 64, False, True, "both"),
    (1, 7, 32, 17, 64, False, False, "g_out"),
    (5, 26, 26, 137, 32, True, True, "g_pool"),
    (257, 32, 32, 1, 32, False, True, "both"),
]
PAIR_H = (1, 2, 7, 8, 15, 16, 26, 32)   # 1, 3, 28, 36, 120, 136, 351, 528 pairs: either side of 32 and of 128
PAIR_O = (1, 33, 127, 128)
PAIR_BD = [(1, 64), (3, 64), (5, 32)]   # half a 128-column workgroup, then a ragged one
PAIR_BF16 = [(3, 26, 26, 128, 64), (5, 7, 7, 33, 32)]
PAIR_BWD_W_CHUNK = (171, 26, 26, 16, 64)  # 512 / ntile = 170 chunks: the first batch with a two-sample chunk
# (B, H, M, O, D, xp is x0, one-channel form); S = samples per workgroup of (forward, backward-x) as cin_pick_plan and
# rp_cin_layer_bwd_x's search choose them (156 KB of LDS, half of it for S > 1 in the forward; S * ND <= 4 tiles per
# wave in the backward when O >= 4):
F32_CASES = [
    (5, 16, 16, 8, 40, True, False),     # S = (4, 2)
    (9, 26, 5, 7, 64, False, False),     # S = (4, 2)   odd M, H != M
    (3, 4, 4, 1, 80, True, True),        # S = (4, 4)   f32_1ch, three column tiles
    (5, 32, 40, 1, 80, False, True),     # S = (2, 4)   H*M = 1280 > 1024: W staged synchronously
    (2, 32, 32, 137, 64, False, False),  # S = (2, 2)
    (6, 26, 16, 16, 33, False, False),   # S = (4, 2)
    (5, 3, 3, 4, 8, True, False),        # S = (4, 4)   D = 8 (added: the list above has no D = 8)
    (3, 5, 6, 4, 80, False, False),      # S = (4, 1)   added: the backward's S = 1 (O >= 4 over three column tiles)
    (3, 32, 48, 1, 80, False, True),     # S = (1, 4)   added: the forward's S = 1 (two samples no longer fit 78 KB)
]
LAST_B = (1, 4, 5)
LAST_HMD = [(26, 128, 64, False), (26, 136, 64, False), (32, 5, 33, False), (1, 1, 1, False), (5, 5, 8, True),
            (7, 130, 32, False)]


# ------------------------------------------------------------------------------------------------ device helpers
def _rows(x3, pad, fill=1e6):
    """[B, R, D] (CPU) -> device [B, R*D + pad], the columns behind R*D filled"""
    B, n = x3.shape[0], x3[0].numel()
    buf = torch.full((B, n + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :n] = x3.reshape(B, n).to(DEV)
    return buf


def _check(tag, got, ref, A, u, K):
    """assert |got - ref| <= gamma A elementwise; prints and returns the largest ratio"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite values"
    bound = gamma(u, K) * A
    assert bool((bound > 0).all()), f"{tag}: a zero bound (degenerate inputs)"
    ratio = float(((got - ref).abs() / bound).max())
    print(f"{tag}: max err/(gamma A) = {ratio:.4f}  (K = {K}, gamma = {gamma(u, K):.3e})")
    assert ratio <= 1.0, f"{tag}: err / (gamma A) = {ratio:.3f} > 1"
    return ratio


def _tail_is(buf, n, what):
    """the columns behind n of a [B, >= n] buffer: all NaN ("nan") or all exactly zero ("zero")"""
    tail = buf[:, n:]
    assert tail.numel() > 0
    ok = torch.isnan(tail).all() if what == "nan" else (tail == 0).all()
    assert bool(ok), f"columns behind {n} are not all {what}"


# ------------------------------------------------------------------------------------------------ bs (per-channel bf16)
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,M,O,D,same", BS_FWD)
def test_cin_bs_fwd(hip, B, H, M, O, D, same):
    c = _case(B, H, M, O, D, same)
    x0 = _rows(c.X0, 13)
    xp = x0 if same else _rows(c.Xp, 13)
    wp = hip.bf16_pieces(c.W.to(DEV))
    for with_bias in (True, False):
        bd = c.d.bias if with_bias else None
        ro, rp = ref_fwd(c.d.X0, c.d.Xp, c.d.W, bd)
        ao, ap = ref_fwd(*_abs(c.d.X0, c.d.Xp, c.d.W, bd))
        if not with_bias:  # K counts the bias term; without one the bar must not be zero where the products vanish
            assert bool((ao > 0).all())
        for want_out, want_pool in ((True, True), (True, False), (False, True)):
            out, pooled = hip.cin_bs_fwd(x0, xp, wp, c.bias.to(DEV) if with_bias else None, H, M, O, D, want_out, want_pool)
            tag = f"cin_bs_fwd[{B},{H},{M},{O},{D} bias={int(with_bias)} out={int(want_out)} pool={int(want_pool)}]"
            assert (out is None) == (not want_out) and (pooled is None) == (not want_pool)
            if want_out:
                _check(tag + " out", out, ro, ao, U_F32, _K("out", B, H, M, O, D))
            if want_pool:
                _check(tag + " pooled", pooled, rp, ap, U_F32, _K("pooled", B, H, M, O, D))


BS_BWD_X = [(R, C, src, B, D) for (R, C) in BS_BWD_X_RC for src in (("W", "WT", "SYM") if R == C else ("W", "WT"))
            for (B, D) in BS_BWD_X_BD]


def _bs_bwd_x_ref(R, C, src, B, D, O, gmode):
    """-> (case, xk [B, C, D], weights [O, R, C] (fp32), ref, A, K) of one rp_cin_bs_bwd_x call.  src "W": the X_0-role
    gradient of a layer with (H, M) = (R, C); "WT": the X_{k-1}-role gradient of a layer with (H, M) = (C, R), weights
    W^T; "SYM": a first layer's whole gradient, weights W + W^T"""
    if src == "W":
        c = _case(B, R, C, O, D)
        _, _, G, Ga = _grads(c, gmode)
        ref = ref_bwd_x(c.d.X0, c.d.Xp, c.d.W, G)[0]
        A = ref_bwd_x(c.d.X0.abs(), c.d.Xp.abs(), c.d.W.abs(), Ga)[0]
        return c, c.Xp, c.W, ref, A, _K("dx0", B, R, C, O, D)
    if src == "WT":
        c = _case(B, C, R, O, D)
        _, _, G, Ga = _grads(c, gmode)
        ref = ref_bwd_x(c.d.X0, c.d.Xp, c.d.W, G)[1]
        A = ref_bwd_x(c.d.X0.abs(), c.d.Xp.abs(), c.d.W.abs(), Ga)[1]
        return c, c.X0, c.W.transpose(1, 2).contiguous(), ref, A, _K("dxp", B, C, R, O, D)
    c = _case(B, R, R, O, D, True)
    _, _, G, Ga = _grads(c, gmode)
    ref = sum(ref_bwd_x(c.d.X0, c.d.X0, c.d.W, G))
    A = sum(ref_bwd_x(c.d.X0.abs(), c.d.X0.abs(), c.d.W.abs(), Ga))
    return c, c.X0, None, ref, A, _K("dx_both", B, R, R, O, D)


@pytest.mark.gpu
@pytest.mark.parametrize("R,C,src,B,D", BS_BWD_X)
def test_cin_bs_bwd_x(hip, R, C, src, B, D):
    for O in BS_BWD_X_O:
        for gmode in GMODES:
            c, xk3, w3, ref, A, K = _bs_bwd_x_ref(R, C, src, B, D, O, gmode)
            go, gp, _, _ = _grads(c, gmode)
            xk = _rows(xk3, 13)
            if src == "SYM":  # formed on the device in fp32, as functional._CINLayer.backward forms it
                wd = c.W.to(DEV)
                wp = hip.bf16_pieces(wd + wd.transpose(1, 2))
            else:
                wp = hip.bf16_pieces(w3.to(DEV))
            go_d = None if go is None else go.to(DEV)
            gp_d = None if gp is None else gp.to(DEV)
            tag = f"cin_bs_bwd_x[{src} R={R} C={C} B={B} D={D} O={O} {gmode}]"
            like = torch.full((B, R * D + 13), float("nan"), dtype=torch.float32, device=DEV)
            dx = hip.cin_bs_bwd_x(xk, wp, go_d, gp_d, R, C, O, D, like=like)
            assert dx.shape == like.shape
            _tail_is(dx, R * D, "zero")
            _check(tag + " like", dx[:, :R * D], ref, A, U_F32, K)
            buf = torch.full((B, R * D + 13), float("nan"), dtype=torch.float32, device=DEV)
            buf[:, :R * D] = 0
            ret = hip.cin_bs_bwd_x(xk, wp, go_d, gp_d, R, C, O, D, like=None, out=buf[:, :R * D])
            assert ret.data_ptr() == buf.data_ptr()
            _tail_is(buf, R * D, "nan")
            _check(tag + " out=", buf[:, :R * D], ref, A, U_F32, K)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,M,O,D,same,want_bias,gmode", BS_BWD_W)
def test_cin_bs_bwd_w(hip, B, H, M, O, D, same, want_bias, gmode):
    c = _case(B, H, M, O, D, same)
    go, gp, G, Ga = _grads(c, gmode)
    rw, rb = ref_bwd_w(c.d.X0, c.d.Xp, G)
    aw, ab = ref_bwd_w(c.d.X0.abs(), c.d.Xp.abs(), Ga)
    x0 = _rows(c.X0, 16)
    xp = x0 if same else _rows(c.Xp, 16)
    assert x0.data_ptr() % 16 == 0 and xp.data_ptr() % 16 == 0 and x0.stride(0) % 4 == 0
    go_d = None if go is None else go.to(DEV)
    gp_d = None if gp is None else gp.to(DEV)
    dW, db = hip.cin_bs_bwd_w(x0, xp, go_d, gp_d, H, M, O, D, want_bias)
    tag = f"cin_bs_bwd_w[{B},{H},{M},{O},{D} {gmode}]"
    _check(tag + " dW", dW, rw, aw, U_F32, _K("dw", B, H, M, O, D))
    assert (db is None) == (not want_bias)
    if want_bias:
        _check(tag + " db", db, rb, ab, U_F32, _K("db", B, H, M, O, D))
    dW2, db2 = hip.cin_bs_bwd_w(x0, xp, go_d, gp_d, H, M, O, D, want_bias)  # fixed summation order
    assert torch.equal(dW, dW2) and (db is None or torch.equal(db, db2))


# ------------------------------------------------------------------------------------------------ pair (first layer)
def _pair_combos(H):
    return [(B, H, H, O, D) for O in PAIR_O for (B, D) in PAIR_BD]


def _with_mode(hip, mode, fn):
    hip.set_matmul_precision(mode)
    try:
        assert hip.get_matmul_precision() == mode
        fn()
    finally:
        hip.set_matmul_precision("auto")


def _pair_fwd(hip, shapes, mode):
    u = PAIR_U[mode]
    for k, (B, H, M, O, D) in enumerate(shapes):
        c = _case(B, H, H, O, D, True)
        with_bias, want_out, want_pool = [(True, True, True), (True, False, True), (False, True, False)][k % 3]
        bd = c.d.bias if with_bias else None
        ro, rp = ref_fwd(c.d.X0, c.d.X0, c.d.W, bd)
        ao, ap = ref_fwd(*_abs(c.d.X0, c.d.X0, c.d.W, bd))
        x0 = _rows(c.X0, 13)
        wsp = hip.cin_pair_pieces(c.W.to(DEV))
        out, pooled = hip.cin_pair_fwd(x0, wsp, c.bias.to(DEV) if with_bias else None, H, O, D, want_out, want_pool)
        tag = f"cin_pair_fwd[{mode} {B},{H},{O},{D} bias={int(with_bias)}]"
        assert (out is None) == (not want_out) and (pooled is None) == (not want_pool)
        if want_out:
            _check(tag + " out", out, ro, ao, u, _K("out", B, H, H, O, D))
        if want_pool:
            _check(tag + " pooled", pooled, rp, ap, u, _K("pooled", B, H, H, O, D))


def _pair_bwd_x(hip, shapes, mode):
    u = PAIR_U[mode]
    for k, (B, H, M, O, D) in enumerate(shapes):
        c = _case(B, H, H, O, D, True)
        gmode, use_into = [("both", False), ("g_out", True), ("g_pool", False), ("both", True)][k % 4]
        go, gp, G, Ga = _grads(c, gmode)
        ref = sum(ref_bwd_x(c.d.X0, c.d.X0, c.d.W, G))
        A = sum(ref_bwd_x(c.d.X0.abs(), c.d.X0.abs(), c.d.W.abs(), Ga))
        K = _K("dx_both", B, H, H, O, D)
        x0 = _rows(c.X0, 16)
        wst = hip.cin_pair_pieces(c.W.to(DEV), transposed=True)
        go_d = None if go is None else go.to(DEV)
        gp_d = None if gp is None else gp.to(DEV)
        assert go_d is None or go_d.data_ptr() % 16 == 0
        tag = f"cin_pair_bwd_x[{mode} {B},{H},{O},{D} {gmode}]"
        if use_into:  # ADDED to what is there; the columns behind H*D are not touched
            pre = torch.randn(B, H * D, generator=torch.Generator().manual_seed(k + H))
            buf = torch.full((B, H * D + 16), float("nan"), dtype=torch.float32, device=DEV)
            buf[:, :H * D] = pre.to(DEV)
            ret = hip.cin_pair_bwd_x(x0, wst, go_d, gp_d, H, O, D, like=None, into=buf)
            assert ret is buf
            _tail_is(buf, H * D, "nan")
            pre3 = pre.double().reshape(B, H, D)
            _check(tag + " into=", buf[:, :H * D], ref + pre3, A + pre3.abs(), u, K + 1)
        else:
            dx = hip.cin_pair_bwd_x(x0, wst, go_d, gp_d, H, O, D, like=x0)
            assert dx.shape == x0.shape
            _tail_is(dx, H * D, "zero")
            _check(tag + " like", dx[:, :H * D], ref, A, u, K)


def _pair_bwd_w(hip, shapes, mode):
    u = PAIR_U[mode]
    for k, (B, H, M, O, D) in enumerate(shapes):
        c = _case(B, H, H, O, D, True)
        gmode, want_bias = GMODES[k % 3], (k % 4 != 1)
        go, gp, G, Ga = _grads(c, gmode)
        rw, rb = ref_bwd_w(c.d.X0, c.d.X0, G)
        aw, ab = ref_bwd_w(c.d.X0.abs(), c.d.X0.abs(), Ga)
        x0 = _rows(c.X0, 16)
        go_d = None if go is None else go.to(DEV)
        gp_d = None if gp is None else gp.to(DEV)
        assert x0.data_ptr() % 16 == 0 and (go_d is None or go_d.data_ptr() % 16 == 0)
        dW, db = hip.cin_pair_bwd_w(x0, go_d, gp_d, H, O, D, want_bias)
        tag = f"cin_pair_bwd_w[{mode} {B},{H},{O},{D} {gmode}]"
        _check(tag + " dW", dW, rw, aw, u, _K("dw", B, H, H, O, D))
        assert (db is None) == (not want_bias)
        if want_bias:  # the bias gradient is a plain fp32 sum of G in every mode
            _check(tag + " db", db, rb, ab, U_F32, _K("db", B, H, H, O, D))
        if k % 2 == 0:  # fixed summation order
            dW2, db2 = hip.cin_pair_bwd_w(x0, go_d, gp_d, H, O, D, want_bias)
            assert torch.equal(dW, dW2) and (db is None or torch.equal(db, db2))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("H", PAIR_H)
def test_cin_pair_fwd(hip, H, mode):
    _with_mode(hip, mode, lambda: _pair_fwd(hip, _pair_combos(H), mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("H", PAIR_H)
def test_cin_pair_bwd_x(hip, H, mode):
    _with_mode(hip, mode, lambda: _pair_bwd_x(hip, _pair_combos(H), mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("H", PAIR_H)
def test_cin_pair_bwd_w(hip, H, mode):
    _with_mode(hip, mode, lambda: _pair_bwd_w(hip, _pair_combos(H), mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
def test_cin_pair_bwd_w_first_two_sample_chunk(hip, mode):
    _with_mode(hip, mode, lambda: _pair_bwd_w(hip, [PAIR_BWD_W_CHUNK], mode))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["fwd", "bwd_x", "bwd_w"])
def test_cin_pair_one_product_bf16(hip, kernel):
    """mode "bf16": the NPROD = 1 instantiations, held to u = 2^-8"""
    fn = {"fwd": _pair_fwd, "bwd_x": _pair_bwd_x, "bwd_w": _pair_bwd_w}[kernel]
    _with_mode(hip, "bf16", lambda: fn(hip, PAIR_BF16 + PAIR_BF16[::-1], "bf16"))


# ------------------------------------------------------------------------------------------------ f32 family
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,M,O,D,same,one_channel", F32_CASES)
def test_cin_layer_f32(hip, B, H, M, O, D, same, one_channel):
    """rp_cin_layer_fwd, _bwd_x and _bwd_w on rows that are not 16-byte aligned (the family is the fallback for them);
    one_channel: the f32_1ch form (want_out=False, g_out=None)"""
    c = _case(B, H, M, O, D, same)
    x0 = _rows(c.X0, 13)
    xp = x0 if same else _rows(c.Xp, 13)
    W2 = c.W.reshape(O, H * M).to(DEV)
    tag = f"cin_layer[{B},{H},{M},{O},{D}]"
    ro, rp = ref_fwd(c.d.X0, c.d.Xp, c.d.W, c.d.bias)
    ao, ap = ref_fwd(*_abs(c.d.X0, c.d.Xp, c.d.W, c.d.bias))
    out, pooled = hip.cin_layer_fwd(x0, xp, W2, c.bias.to(DEV), H, M, D, not one_channel, True)
    assert (out is None) == one_channel
    if out is not None:
        _check(tag + " fwd out", out, ro, ao, U_F32, _K("out", B, H, M, O, D))
    _check(tag + " fwd pooled", pooled, rp, ap, U_F32, _K("pooled", B, H, M, O, D))

    gmode = "g_pool" if one_channel else "both"
    go, gp, G, Ga = _grads(c, gmode)
    go_d = None if go is None else go.to(DEV)
    gpbuf = torch.full((B, O + 3), 1e6, dtype=torch.float32, device=DEV)  # g_pool arrives as a slice of a wider tensor
    gpbuf[:, :O] = gp.to(DEV)
    dx0, dxp, dW, db = hip.cin_layer_bwd(x0, xp, W2, H, M, D, go_d, gpbuf[:, :O], True)
    r0, r1 = ref_bwd_x(c.d.X0, c.d.Xp, c.d.W, G)
    a0, a1 = ref_bwd_x(c.d.X0.abs(), c.d.Xp.abs(), c.d.W.abs(), Ga)
    assert dx0.shape == x0.shape
    _tail_is(dx0, H * D, "zero")
    if same:
        assert dxp is None
        _check(tag + " bwd_x dx0 (both roles)", dx0[:, :H * D], r0 + r1, a0 + a1, U_F32, _K("dx_both", B, H, M, O, D))
    else:
        _check(tag + " bwd_x dx0", dx0[:, :H * D], r0, a0, U_F32, _K("dx0", B, H, M, O, D))
        _check(tag + " bwd_x dxp", dxp, r1, a1, U_F32, _K("dxp", B, H, M, O, D))
    rw, rb = ref_bwd_w(c.d.X0, c.d.Xp, G)
    aw, ab = ref_bwd_w(c.d.X0.abs(), c.d.Xp.abs(), Ga)
    _check(tag + " bwd_w dW", dW, rw, aw, U_F32, _K("dw", B, H, M, O, D))
    _check(tag + " bwd_w db", db, rb, ab, U_F32, _K("db", B, H, M, O, D))
    dW2, db2 = hip.cin_layer_bwd_w(x0, xp, W2, H, M, D, go_d, gpbuf[:, :O], True)  # alone, and in a fixed order
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


# ------------------------------------------------------------------------------------------------ collapsed last layer
@pytest.mark.gpu
@pytest.mark.parametrize("H,M,D,same", LAST_HMD)
def test_cin_last(hip, H, M, D, same):
    for B in LAST_B:
        c = _case(B, H, M, 1, D, same)
        vt = torch.zeros(M, 32, dtype=torch.float32, device=DEV)
        vt[:, :H] = c.V.t().to(DEV)
        x0 = _rows(c.X0, 13)
        xp = x0 if same else _rows(c.Xp, 13)
        g = c.g.to(DEV)
        tag = f"cin_last[{B},{H},{M},{D}]"
        p = hip.cin_last_fwd(x0, xp, vt, H, M, D)
        assert p.shape == (B, 1)
        _check(tag + " fwd p", p, ref_last_fwd(c.d.X0, c.d.Xp, c.d.V), ref_last_fwd(*_abs(c.d.X0, c.d.Xp, c.d.V)), U_F32,
               _K("p", B, H, M, 1, D))
        dx0, dxp, dV = hip.cin_last_bwd(x0, xp, vt, g, H, M, D)
        r0, r1 = ref_last_bwd_x(c.d.X0, c.d.Xp, c.d.V, c.d.g)
        a0, a1 = ref_last_bwd_x(*_abs(c.d.X0, c.d.Xp, c.d.V, c.d.g))
        assert dx0.shape == x0.shape and dxp.shape == xp.shape
        _tail_is(dx0, H * D, "zero")
        _tail_is(dxp, M * D, "zero")
        _check(tag + " bwd_x dx0", dx0[:, :H * D], r0, a0, U_F32, _K("last_dx0", B, H, M, 1, D))
        _check(tag + " bwd_x dxp", dxp[:, :M * D], r1, a1, U_F32, _K("last_dxp", B, H, M, 1, D))
        rv, av = ref_last_bwd_v(c.d.X0, c.d.Xp, c.d.g), ref_last_bwd_v(*_abs(c.d.X0, c.d.Xp, c.d.g))
        _check(tag + " bwd_v dV (unaligned rows)", dV, rv, av, U_F32, _K("dv", B, H, M, 1, D))
        # the same data on 16-byte aligned rows (the vector load path where D % 4 == 0), twice: a fixed summation order
        y0 = _rows(c.X0, 16 + (-H * D) % 4)
        yp = y0 if same else _rows(c.Xp, 16 + (-M * D) % 4)
        assert y0.stride(0) % 4 == 0 and yp.stride(0) % 4 == 0 and y0.data_ptr() % 16 == 0 and yp.data_ptr() % 16 == 0
        dVa = hip.cin_last_bwd(y0, yp, vt, g, H, M, D)[2]
        _check(tag + " bwd_v dV (aligned rows)", dVa, rv, av, U_F32, _K("dv", B, H, M, 1, D))
        assert torch.equal(dVa, hip.cin_last_bwd(y0, yp, vt, g, H, M, D)[2])


# ------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70 * 8 * 64])
def test_accumulate(hip, n):
    g = torch.Generator().manual_seed(n)
    dst, src = torch.randn(n, generator=g), torch.randn(n, generator=g)
    buf = torch.full((n + 5,), float("nan"), dtype=torch.float32, device=DEV)
    buf[:n] = dst.to(DEV)
    ret = hip.accumulate(buf[:n], src.to(DEV))
    assert ret.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:n].cpu(), dst + src)
    assert bool(torch.isnan(buf[n:]).all())


# ------------------------------------------------------------------------------------------------ host-side guards
@pytest.mark.gpu
def test_guards_refuse_before_any_launch(hip):
    """shapes and alignments the entry points check on the host (RP_REQUIRE / rp_fail ahead of every launch): each call
    raises the library's error and launches nothing"""
    def dev(*shape):
        return torch.zeros(shape, dtype=torch.float32, device=DEV)

    def refused(what, fn):
        n0 = hip.launch_count()
        with pytest.raises(RuntimeError, match=what):
            fn()
        assert hip.launch_count() == n0, what

    B = 2
    # cin_bs_fwd, D = 40: not 32 or 64
    wp = torch.zeros((4, 3, 32, 32), dtype=torch.bfloat16, device=DEV)
    refused("rp_cin_bs_fwd failed",
            lambda: hip.cin_bs_fwd(dev(B, 4 * 40), dev(B, 4 * 40), wp, None, 4, 4, 4, 40, True, True))
    # cin_pair_fwd, O = 129
    wsp = torch.zeros((3, 128, 32), dtype=torch.bfloat16, device=DEV)
    refused("rp_cin_pair_fwd failed", lambda: hip.cin_pair_fwd(dev(B, 4 * 32), wsp, None, 4, 129, 32, True, True))
    # cin_pair_bwd_x, g_out four bytes off alignment
    wst = torch.zeros((3, 128, 128), dtype=torch.bfloat16, device=DEV)
    g_out = dev(B * 8 * 32 + 1)[1:].view(B, 8, 32)
    assert g_out.data_ptr() % 16 == 4
    x0 = dev(B, 4 * 32)
    hip.cin_pair_lists(4, x0.device)  # (built once per H, ahead of the count)
    refused("rp_cin_pair_bwd_x failed", lambda: hip.cin_pair_bwd_x(x0, wst, g_out, None, 4, 8, 32, like=x0))
    # cin_bs_bwd_w, rows with ld % 4 != 0
    xu = dev(B, 4 * 32 + 13)
    refused("rp_cin_bs_bwd_w failed", lambda: hip.cin_bs_bwd_w(xu, xu, dev(B, 8, 32), None, 4, 4, 8, 32, True))
    # cin_last_fwd, D = 65
    refused("rp_cin_last_fwd failed", lambda: hip.cin_last_fwd(dev(B, 4 * 65), dev(B, 4 * 65), dev(4, 32), 4, 4, 65))
    # cin_layer_fwd, H = 33
    refused("rp_cin_layer_fwd failed",
            lambda: hip.cin_layer_fwd(dev(B, 33 * 8), dev(B, 4 * 8), dev(2, 33 * 4), None, 33, 4, 8, True, True))


# ------------------------------------------------------------------------------------------------ the bar has teeth (CPU)
def _breaks(ref, A, bad, K):
    """the faulty value is outside gamma A for u = 2^-23 and u = 2^-16, and the reference rounded to fp32 inside"""
    err = (bad - ref).abs()
    rounded = (ref.float().double() - ref).abs()
    for u in (U_F32, U_X3):
        assert bool((rounded <= gamma(u, K) * A).all())
        if not bool((err > gamma(u, K) * A).any()):
            return False
    return True


def _w_faults(c):
    """W with (1) one (h, m) term dropped from every sum, (2) W[o] of one channel read transposed — where that changes
    anything: not for a first layer (X_0 in both roles makes the sums symmetric in (h, m)) and not for a single row"""
    H, M = c.H, c.M
    W1 = c.d.W.clone()
    W1[:, H // 2, M // 2] = 0
    yield "term dropped", W1
    if not c.same and H > 1 and M > 1:
        W2 = c.d.W.clone()
        W2[c.O // 2] = c.d.W[c.O // 2].reshape(M, H).t()
        yield "W[o] transposed", W2


def _fwd_faults(c, log, tag, on="out"):
    """on: the output the faults are looked for in ("pooled" where the launch produces nothing else)"""
    d, i = c.d, ("out", "pooled").index(on)
    ref = ref_fwd(d.X0, d.Xp, d.W, d.bias)[i]
    A = ref_fwd(*_abs(d.X0, d.Xp, d.W, d.bias))[i]
    K = _K(on, c.B, c.H, c.M, c.O, c.D)
    for name, Wf, bf in [(n, Wf, d.bias) for n, Wf in _w_faults(c)] + [("bias omitted", d.W, None)]:
        if not _breaks(ref, A, ref_fwd(d.X0, d.Xp, Wf, bf)[i], K):
            log.append(f"{tag} forward: {name}")


def _bwd_x_faults(c, log, tag, gmode="both"):
    d = c.d
    _, _, G, Ga = _grads(c, gmode)
    refs, As = ref_bwd_x(d.X0, d.Xp, d.W, G), ref_bwd_x(d.X0.abs(), d.Xp.abs(), d.W.abs(), Ga)
    faults = [(n, Wf, G) for n, Wf in _w_faults(c)]
    faults.append(("g_pool omitted", d.W, d.g_out if gmode == "both" else torch.zeros_like(G)))
    for name, Wf, Gf in faults:
        bads = ref_bwd_x(d.X0, d.Xp, Wf, Gf)
        if c.same:
            ok = _breaks(sum(refs), sum(As), sum(bads), _K("dx_both", c.B, c.H, c.M, c.O, c.D))
        else:  # each role's gradient is an entry point's output of its own
            ok = all(_breaks(refs[i], As[i], bads[i], _K(("dx0", "dxp")[i], c.B, c.H, c.M, c.O, c.D)) for i in range(2))
        if not ok:
            log.append(f"{tag} bwd_x: {name}")


def _bwd_w_faults(c, gmode, log, tag):
    d = c.d
    _, _, G, Ga = _grads(c, gmode)
    rw, _ = ref_bwd_w(d.X0, d.Xp, G)
    aw, _ = ref_bwd_w(d.X0.abs(), d.Xp.abs(), Ga)
    K = _K("dw", c.B, c.H, c.M, c.O, c.D)
    bad = ref_bwd_w(d.X0[:-1], d.Xp[:-1], G[:-1])[0]
    if not _breaks(rw, aw, bad, K):
        log.append(f"{tag} bwd_w: last sample omitted")
    if c.B <= 5:
        G6 = G.clone()
        G6[c.B // 2, :, c.D - 8:] = 0  # the last 8-wide d octet of one sample contributes nothing
        if not _breaks(rw, aw, ref_bwd_w(d.X0, d.Xp, G6)[0], K):
            log.append(f"{tag} bwd_w: one d octet omitted")


# A forward whose only output is ONE number per (sample, channel) — the collapsed last layer's p[b], the f32_1ch form's
# pooled[b, 0] — sums K = D H M terms into it.  With H M >= 910 the bar's (K + 3) 2^-24 is wider than one of the H M terms
# of fault (1) (and, the weights being of random sign, than fault (2)): those (fault, shape) pairs are shown at the same
# (H, D) with M shrunk to 5.  The kernel tests keep the listed M.
SHRUNK_M = {(26, 128, 64): 5, (26, 136, 64): 5, (7, 130, 32): 5, (32, 40, 80): 5, (32, 48, 80): 5}


def _v_faults(c):
    V1 = c.d.V.clone()
    V1[c.H // 2, c.M // 2] = 0
    yield "term dropped", V1
    if not c.same and c.H > 1 and c.M > 1:
        yield "V transposed", c.d.V.reshape(c.M, c.H).t()


def _last_faults(B, H, M, D, same, log):
    c = _case(B, H, M, 1, D, same)
    d, tag = c.d, f"last[{B},{H},{M},{D}]"
    cf = _case(B, H, SHRUNK_M.get((H, M, D), M), 1, D, same)  # the forward's one number per sample: see SHRUNK_M
    rp_, ap_ = ref_last_fwd(cf.d.X0, cf.d.Xp, cf.d.V), ref_last_fwd(*_abs(cf.d.X0, cf.d.Xp, cf.d.V))
    for name, Vf in _v_faults(cf):
        if not _breaks(rp_, ap_, ref_last_fwd(cf.d.X0, cf.d.Xp, Vf), _K("p", B, cf.H, cf.M, 1, D)):
            log.append(f"{tag} forward (at M = {cf.M}): {name}")
    rx, ax = ref_last_bwd_x(d.X0, d.Xp, d.V, d.g), ref_last_bwd_x(*_abs(d.X0, d.Xp, d.V, d.g))
    for name, Vf in _v_faults(c):
        bx = ref_last_bwd_x(d.X0, d.Xp, Vf, d.g)
        if not all(_breaks(rx[i], ax[i], bx[i], _K(("last_dx0", "last_dxp")[i], B, H, M, 1, D)) for i in range(2)):
            log.append(f"{tag} bwd_x: {name}")
    rv, av = ref_last_bwd_v(d.X0, d.Xp, d.g), ref_last_bwd_v(*_abs(d.X0, d.Xp, d.g))
    K = _K("dv", B, H, M, 1, D)
    if not _breaks(rv, av, ref_last_bwd_v(d.X0[:-1], d.Xp[:-1], d.g[:-1]), K):
        log.append(f"{tag} bwd_v: last sample omitted")
    g6 = d.g.view(-1, 1, 1).expand(B, H, D).clone()
    g6[B // 2, :, max(D - 8, 0):] = 0
    if not _breaks(rv, av, torch.einsum("bhd,bmd->hm", g6 * d.X0, d.Xp), K):
        log.append(f"{tag} bwd_v: one d octet omitted")


def test_bar_catches_subtly_wrong_kernels():
    """Six faults applied to the float64 references, one at a time — (1) one (h, m) term dropped from every sum, (2) W[o]
    of one channel transposed, (3) bias omitted, (4) g_pool omitted, (5) the last sample left out of a weight gradient,
    (6) one 8-wide d octet of one sample left out of a weight gradient — break gamma A for u = 2^-23 and u = 2^-16 at
    the shapes of the kernel tests (1-4 at the forward / bwd_x shapes, 5 at the bwd_w shapes, 6 at those with B <= 5),
    while the unperturbed reference rounded to fp32 passes.  The pooled sums (K = D (H M + 1) terms) are wider than
    one term by construction: the faults are asserted on the [B, O, D] outputs the same launches produce."""
    missed = []
    for (B, H, M, O, D, same) in BS_FWD:
        _fwd_faults(_case(B, H, M, O, D, same), missed, f"bs[{B},{H},{M},{O},{D}]")
    for (R, C, src, B, D) in BS_BWD_X:
        for O in BS_BWD_X_O:
            c = _case(B, C, R, O, D) if src == "WT" else _case(B, R, C, O, D, src == "SYM")
            _bwd_x_faults(c, missed, f"bs[{src},{R},{C},{B},{D},{O}]")
    for (B, H, M, O, D, same, _, gmode) in BS_BWD_W:
        _bwd_w_faults(_case(B, H, M, O, D, same), gmode, missed, f"bs[{B},{H},{M},{O},{D}]")
    for shape in [s for H in PAIR_H for s in _pair_combos(H)] + PAIR_BF16:
        c = _case(*shape, True)
        _fwd_faults(c, missed, f"pair{list(shape)}")
        _bwd_x_faults(c, missed, f"pair{list(shape)}")
        _bwd_w_faults(c, "both", missed, f"pair{list(shape)}")
    _bwd_w_faults(_case(*PAIR_BWD_W_CHUNK, True), "both", missed, f"pair{list(PAIR_BWD_W_CHUNK)}")
    for (B, H, M, O, D, same, one_channel) in F32_CASES:
        c = _case(B, H, M, O, D, same)
        if one_channel:
            Ms = SHRUNK_M.get((H, M, D), M)
            _fwd_faults(_case(B, H, Ms, O, D, same), missed, f"f32[{B},{H},{M},{O},{D}] (at M = {Ms})", on="pooled")
        else:
            _fwd_faults(c, missed, f"f32[{B},{H},{M},{O},{D}]")
        gmode = "g_pool" if one_channel else "both"
        _bwd_x_faults(c, missed, f"f32[{B},{H},{M},{O},{D}]", gmode)
        _bwd_w_faults(c, gmode, missed, f"f32[{B},{H},{M},{O},{D}]")
    for (H, M, D, same) in LAST_HMD:
        for B in LAST_B:
            _last_faults(B, H, M, D, same, missed)
    assert missed == [], "the bar does not notice:\n" + "\n".join(missed)
