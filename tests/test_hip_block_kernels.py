"""Every entry point of the round 1-3 block kernels — csrc/cross.hip, mmoe.hip, norm.hip (FM pooling, the BatchNorm
family, the Dice gate, rp_accumulate), attn_core.hip and attn.hip — ALONE against a float64 restatement of its operation,
at the shapes where its launch code takes another path.  Built like tests/test_hip_cin_kernels.py.

Bars are derived, not tuned; each holds only float64 quantities of the case, u = 2^-23, eps = 2^-24 and term counts.

  sums of products   |got[e] - ref[e]| <= gamma(u, K) A[e],  gamma(u, K) = 3 u + (K + 3) 2^-24  (the CIN file's), A[e] the
                     same expression over absolute values in float64, K the roundings on the longest path into the element
                     (one per product, one per addition; a chained quantity carries its operand's count): the _K_* tables.
  nonlinear stages   first order: (bar of the stage's input) x |derivative in float64| + the stage's own rounding.
      exp            3 ulp = 3 u relative (OpenCL's bound for exp, which the device library's expf meets); an argument
                     s - m carries the bars of s and of m and the subtraction's (m - s) eps; exp's derivative is itself, so
                     an argument error is a relative error of the result.  A result under 2^-126 may be flushed: every
                     softmax bar has the absolute term TINY = 2^-125, and so has every
                     sum whose terms have such a factor (a product under 2^-126 is rounded in, or flushed from, the subnormal
                     range: an absolute error no relative bar covers), once per term.
      softmax row    p_j = e_j / sum e: rho = 2 max_k bar(s_k) + 3 u n_exp + (m - min s) eps + (2 n + 4) eps relative
                     (n_exp chained exp factors: 1 for the two-pass rows, T for the online form of attn_core, whose term j
                     is exp(s_j - m') times up to T - 1 rescalings exp(m' - m'') whose arguments add up to m - s_j; n
                     additions of the denominator, the division, and n more multiplications online).  The maximum's own
                     error cancels (softmax is shift invariant) but is counted: 2 max bar(s).
      rsqrt, sigmoid, ReLU: at the tests that use them.
  exact              masks / ReLU decisions further from zero than their bar, guard columns, copied values, counters.

Inputs: rows live in wider buffers.  Input padding holds 1e6 (NaN where the kernel is documented to load it and select it
away: CrossNet's VEC forms); outputs are prefilled with NaN: afterwards every owned element is finite and every other one
is still NaN.  FM fields sit around a common offset, BatchNorm has a column whose mean is hundreds of standard deviations
and a constant one, softmax rows come all-equal, one 80 above the rest, and spread over +-60, Dice's xhat reaches +-30.

The CPU test at the end applies the issue's eight faults to the float64 references and asserts the bars notice."""
import ctypes as C
import functools
import types

import pytest
import torch

from conftest import require_gpu

DEV = "cuda"
U = 2.0 ** -23
EPS = 2.0 ** -24
TINY = 2.0 ** -125
U_EXP = 3.0 * U
NAN = float("nan")
# The Dice gate's sigmoid is 1 / (1 + __expf(-xhat)) (the hardware exponential, no stated accuracy).  Measured once on an
# MI355X by test_dice_sigmoid_accuracy over 240001 points of [-30, 30] against float64: worst relative error 1.779e-6, at
# xhat = -29.65 (__expf scales its argument by log2 e in fp32, so its error grows with |xhat|: 5.3e-7 within |xhat| <= 10).
# The test prints the figure on every run.  The Dice bars use twice that as the sigmoid's relative error.
EXPF_SIGMOID_MEASURED = 1.779e-6
U_SIG = 2.0 * EXPF_SIGMOID_MEASURED


@pytest.fixture(scope="module")
def hip():
    require_gpu()
    from rec_pangu_amd import hip as h
    h.lib()
    return h


@pytest.fixture(autouse=True)
def _a_device_fault_ends_the_session():
    """the tests of this file launch kernels on buffers of their own: after a device fault nothing more is started"""
    yield
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:   # (pytest.exit is not an Exception: it leaves the session)
            pytest.exit(f"device fault, nothing more is run: {e}", returncode=3)


def gamma(u: float, K: int) -> float:
    return 3.0 * u + (K + 3) * 2.0 ** -24


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# =================================================================================================== float64 references
# ---------------------------------------------------------------------------------------------------------- CrossNet
def ref_cross_fwd(x0, W, Bv, wfc=None, bfc=None, drop=None, stale_bias=False):
    """X_{l+1} = X_l + (X_l . w_l) X_0 + b_l,  s_l = X_l . w_l,  logit = X_L . wfc + bfc   (cross.hip header).
    With absolute inputs it is the A of every output.  drop = (l, j): fault (a), term j left out of layer l's dot;
    stale_bias: fault (b), layer l >= 1 adds b_{l-1}."""
    X, s = x0, []
    for l in range(W.shape[0]):
        w = W[l]
        if drop is not None and drop[0] == l:
            w = w.clone()
            w[drop[1]] = 0
        sl = X @ w
        s.append(sl)
        X = X + sl[:, None] * x0 + Bv[l - 1 if (stale_bias and l >= 1) else l]
    logit = None if wfc is None else X @ wfc + (0 if bfc is None else bfc)
    return X, torch.stack(s, 1), logit


def _K_cross(kind, d, L, l=0):
    """x0, w, b exact (0).  s_l = sum_d X_l w: K(X_l) + d;  X_{l+1} = X_l + (s X_0 + b): K(s_l) + 3 = K(X_l) + d + 3, so
    K(X_l) = l (d + 3).  Backward (s_in exact): g_L = g_x + gl wfc: 2;  t_l = sum_d g_{l+1} X_0: K(g_{l+1}) + d;  g_l =
    g_{l+1} + t_l w_l: K(g_{l+1}) + d + 2, so K(g_l) = 2 + (L - l)(d + 2);  A_l = 1 + sum s peeled back: at most 2 L;
    dx0 = g_0 + sum_l s_l g_{l+1}: K(g_0) + L + 2.  Parameter gradients: prefix / suffix sums of L terms and one product."""
    return {"s": l * (d + 3) + d, "xout": L * (d + 3), "logit": L * (d + 3) + d + 1,
            "t": 2 + (L - 1 - l) * (d + 2) + d, "tA": 2 + (L - 1 - l) * (d + 2) + d + 2 * L + 1, "glA": L + 1,
            "dx0": 2 + L * (d + 2) + L + 2, "param": L + 2}[kind]


def ref_cross_bwd(x0, W, wfc, s, g_x, g_logit, ab=False):
    """the streaming backward as its comment states it -> dx0 [B, d], V [B, 2L+2] = [t_l A_l | gl A_L | t_l | gl].
    ab: operands are absolute values; then A_l is 1 + sum_k |s_k| over ALL k (the kernel peels a_run back by subtraction)"""
    B, L = s.shape
    gl = torch.zeros(B, dtype=x0.dtype) if g_logit is None else g_logit
    g = torch.zeros_like(x0) if g_x is None else g_x
    if g_logit is not None:
        g = g + gl[:, None] * wfc
    A = [1 + (s.sum(1) if ab else s[:, :l].sum(1)) for l in range(L + 1)]
    V = torch.zeros(B, 2 * L + 2, dtype=x0.dtype)
    V[:, L], V[:, 2 * L + 1] = gl * A[L], gl
    gx0 = torch.zeros_like(x0)
    for l in range(L - 1, -1, -1):
        t = (g * x0).sum(1)
        V[:, l], V[:, L + 1 + l] = t * A[l], t
        gx0 = gx0 + s[:, l:l + 1] * g
        g = g + t[:, None] * W[l]
    return gx0 + g, V


def ref_cross_param(P, cs, W, Bv, wfc, colg):
    """dW[l] = P[l] + C_l st_l;  dB[l] = sum_{k>l} w_k st_k + extra;  dwfc = P[L] + C_L sgl;  C_l = sum_{k<l} b_k,
    st_l = cs[L+1+l], sgl = cs[2L+1], extra = wfc sgl | colg | 0"""
    L, d = W.shape
    st, sgl = cs[L + 1:2 * L + 1], cs[2 * L + 1]
    Cp = torch.cat([torch.zeros(1, d, dtype=W.dtype), Bv.cumsum(0)])
    dW = P[:L, :d] + Cp[:L] * st[:, None]
    extra = wfc * sgl if wfc is not None else (colg if colg is not None else torch.zeros(d, dtype=W.dtype))
    wst = W * st[:, None]
    suffix = torch.cat([wst.flip(0).cumsum(0).flip(0)[1:], torch.zeros(1, d, dtype=W.dtype)])
    dB = suffix + extra
    dwfc = None if wfc is None else P[L, :d] + Cp[L] * sgl
    return dW, dB, dwfc


@functools.lru_cache(maxsize=None)
def _cross_case(B, d, L):
    g = _gen(1, B, d, L)
    c = _ns(B=B, d=d, L=L)
    c.x0 = torch.randn(B, d, generator=g)
    c.W = 0.5 * torch.randn(L, d, generator=g) / d   # |X_l| . |w_l| stays O(1): the A of a deep layer does not outgrow its value
    c.Bv = 0.1 * torch.randn(L, d, generator=g)
    c.wfc = torch.randn(d, generator=g) / d
    c.bfc = torch.randn(1, generator=g)
    c.g_x = torch.randn(B, d, generator=g)
    c.g_logit = torch.randn(B, generator=g)
    c.P = torch.randn(2 * L + 2, d, generator=g)
    c.cs = torch.randn(2 * L + 2, generator=g)
    c.colg = torch.randn(d, generator=g)
    c.d64 = _ns(**{k: v.double() for k, v in vars(c).items() if torch.is_tensor(v)})
    q = c.d64
    c.xout, c.s, c.logit = ref_cross_fwd(q.x0, q.W, q.Bv, q.wfc, q.bfc)
    c.a_xout, c.a_s, c.a_logit = ref_cross_fwd(q.x0.abs(), q.W.abs(), q.Bv.abs(), q.wfc.abs(), q.bfc.abs())
    c.s32 = c.s.float()   # what the backward is fed: the reference's s rounded to fp32
    return c


def _cross_bars(c):
    d, L = c.d, c.L
    bs = torch.stack([gamma(U, _K_cross("s", d, L, l)) * c.a_s[:, l] for l in range(L)], 1)
    return bs, gamma(U, _K_cross("xout", d, L)) * c.a_xout, gamma(U, _K_cross("logit", d, L)) * c.a_logit


def _cross_bwd_ref(c, gmode):
    """(dx0, V) and their bars for a gradient mode: "g_x", "g_logit" or "both" """
    q, d, L = c.d64, c.d, c.L
    gx = None if gmode == "g_logit" else q.g_x
    gl = None if gmode == "g_x" else q.g_logit
    s = c.s32.double()
    dx0, V = ref_cross_bwd(q.x0, q.W, q.wfc, s, gx, gl)
    adx0, aV = ref_cross_bwd(q.x0.abs(), q.W.abs(), q.wfc.abs(), s.abs(), None if gx is None else gx.abs(),
                             None if gl is None else gl.abs(), ab=True)
    bV = torch.zeros_like(V)
    for l in range(L):
        bV[:, l] = gamma(U, _K_cross("tA", d, L, l)) * aV[:, l]
        bV[:, L + 1 + l] = gamma(U, _K_cross("t", d, L, l)) * aV[:, L + 1 + l]
    bV[:, L] = gamma(U, _K_cross("glA", d, L)) * aV[:, L]   # (column 2L+1 is a copy of gl: bar 0, compared exactly)
    return dx0, V, gamma(U, _K_cross("dx0", d, L)) * adx0, bV


# (B, d, ld, L, misaligned) — the forward's <VEC, B_LDS> instantiation and what else the case reaches
CROSS_CASES = [
    (33, 5, 8, 2, False),        # <true, true>   one chunk, ld > d: the VEC select of loaded padding
    (7, 255, 256, 3, False),     # <true, true>   d one short of a chunk edge
    (7, 256, 260, 3, False),     # <true, true>   d at the edge; ld past dp: columns [dp, ld) stay untouched
    (9, 257, 264, 2, False),     # <true, true>   one column into the second chunk
    (5, 257, 259, 1, False),     # <false, true>  ld % 4 != 0
    (6, 5, 8, 6, True),          # <false, true>  row pointer 4 bytes off 16-byte alignment, L = CROSS_MAXL
    (5, 1800, 1800, 4, False),   # <true, false>  (2L+1) dp 4 = 73728 B > 64 KB: biases read from global memory
    (5, 1801, 1803, 4, False),   # <false, false> the same, unaligned
    (8192 + 5, 5, 8, 2, False),  # the persistent row loop and its register double buffer (B > 8192), VEC
    (8192 + 5, 257, 257, 1, False),  # the same, scalar form, two chunks
    (1, 1, 4, 1, False),
]
CROSS_PARAM = [(5, 2), (255, 3), (256, 6), (257, 1), (1, 1)]


# -------------------------------------------------------------------------------------------------------------- softmax
def softmax_bar(s, bs=0.0, n_exp=1):
    """-> (p, bar of p) over the last axis; s float64, bs the bar of s (tensor or number).  See the header."""
    n = s.shape[-1]
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True)
    bsm = bs.max(-1, keepdim=True).values if torch.is_tensor(bs) else bs
    rho = 2 * bsm + U_EXP * n_exp + (m - s.min(-1, keepdim=True).values) * EPS + (2 * n + 4) * EPS
    return p, p * rho + TINY


SOFTMAX_KINDS = ("normal", "equal", "top80", "pm60")


def _logits(kind, shape, g):
    """[..., n] logits of a softmax case"""
    n = shape[-1]
    if kind == "normal":
        return torch.randn(shape, generator=g)
    if kind == "equal":
        return torch.randn(shape[:-1] + (1,), generator=g).expand(shape).contiguous()
    if kind == "top80":   # the rest sits near 12: the top logit is past 88.7, where an unshifted fp32 exp overflows
        lg = 12.0 + 0.5 * torch.randn(shape, generator=g)
        top = torch.randint(0, n, shape[:-1] + (1,), generator=g)
        return lg.scatter(-1, top, lg.gather(-1, top) + 80.0)
    lg = torch.rand(shape, generator=g) * 120.0 - 60.0   # pm60: both ends present in every row with n >= 2
    if n >= 2:
        lg[..., 0], lg[..., n - 1] = 60.0, -60.0
    return lg


# ----------------------------------------------------------------------------------------------------------------- MMOE
def ref_mmoe_fwd(ze, lg):
    """ze [B, K, E], lg [B, T, E] -> out [T, B, K] = sum_e ze gate, gate [B, T, E] = softmax_e(lg), and their bars"""
    gate, bg = softmax_bar(lg)
    out = torch.einsum("bke,bte->tbk", ze, gate)
    E = ze.shape[2]
    bout = torch.einsum("bke,bte->tbk", ze.abs(), bg) + gamma(U, E) * torch.einsum("bke,bte->tbk", ze.abs(), gate) + E * TINY
    return out, gate, bout, bg


def ref_mmoe_bwd(ze, gate, dout, drop_dot=False):
    """dz[b,k,e] = sum_t dout[t,b,k] gate[b,t,e];  dgate = sum_k dout ze;  dlogit = gate (dgate - sum_e' gate dgate).
    Sums of products of exact inputs: K = T for the expert columns, K + E + 3 for the gate columns (dgate: K terms; the
    dot: E more and a product; a subtraction and a product).  drop_dot: fault (f)."""
    dze = torch.einsum("tbk,bte->bke", dout, gate)
    dgate = torch.einsum("tbk,bke->bte", dout, ze)
    dot = (gate * dgate).sum(-1, keepdim=True)
    return dze, gate * (dgate - (0 if drop_dot else dot))


def _mmoe_bwd_abs(ze, gate, dout):
    dze = torch.einsum("tbk,bte->bke", dout.abs(), gate)
    dgate = torch.einsum("tbk,bke->bte", dout.abs(), ze.abs())
    return dze, gate * (dgate + (gate * dgate).sum(-1, keepdim=True))


def _mmoe_bwd_bars(c, aze, alg):
    """(expert columns, gate columns): K = T and K + E + 3 (ref_mmoe_bwd), a TINY per term with the gate as a factor"""
    return gamma(U, c.T) * aze + c.T * TINY, gamma(U, c.K + c.E + 3) * alg + (c.E + 2) * TINY


@functools.lru_cache(maxsize=None)
def _mmoe_case(B, K, E, T, kind="normal"):
    g = _gen(2, B, K, E, T, SOFTMAX_KINDS.index(kind))
    c = _ns(B=B, K=K, E=E, T=T, kind=kind)
    c.ze = torch.randn(B, K, E, generator=g)
    c.lg = _logits(kind, (B, T, E), g)
    c.dout = torch.randn(T, B, K, generator=g)
    c.out, c.gate, c.b_out, c.b_gate = ref_mmoe_fwd(c.ze.double(), c.lg.double())
    c.gate32 = c.gate.float()
    return c


# (B, K, E, T, extra floats of ldz, pointer offset in floats, softmax kind)
MMOE_CASES = [
    (7, 1, 1, 1, 3, 0, "normal"),     # E = 1 (odd: scalar form); K below one wave stride
    (33, 63, 5, 3, 2, 0, "normal"),   # E = 5
    (33, 64, 6, 2, 0, 0, "normal"),   # E = 6, the 8-byte vector form (ldz = 396, even)
    (9, 65, 6, 2, 1, 0, "normal"),    # E = 6 with an odd ldz: the scalar form of an even E
    (5, 65, 7, 4, 1, 0, "pm60"),      # E = 7; K one past a wave stride
    (7, 64, 4, 8, 2, 0, "top80"),     # T = 8; E = 4 with ldz % 4 == 2: must not take the 16-byte path
    (7, 63, 4, 8, 0, 0, "equal"),     # E = 4, the 16-byte form (ldz = 284)
    (5, 65, 2, 1, 0, 1, "pm60"),      # E = 2, rows 4 bytes off 8-byte alignment: scalar form
    (3, 130, 8, 4, 0, 0, "top80"),    # E = 8, T E = 32 = MM_MAX_TE; a lane walks three k
    (262144 + 3, 1, 2, 1, 0, 0, "normal"),   # the row loop past the 65536-block cap
]


# ------------------------------------------------------------------------------------------------------------ FM pooling
def ref_fm_fwd(x):
    """x [B, F, D] -> bi [B, D] = 0.5 ((sum_f x)^2 - sum_f x^2), sum [B] = sum_d bi.  K: s F-1, s s 2F-1, q F, the
    difference 2F (the halving is exact); the row sum adds D."""
    s = x.sum(1)
    bi = 0.5 * (s * s - (x * x).sum(1))
    return bi, bi.sum(1)


def _fm_fwd_abs(x):
    s = x.abs().sum(1)
    bi = 0.5 * (s * s + (x * x).sum(1))
    return bi, bi.sum(1)


def _fm_g(x, g_sum, g_bi):
    g = torch.zeros(x.shape[0], x.shape[2], dtype=x.dtype)
    if g_sum is not None:
        g = g + g_sum[:, None]
    return g if g_bi is None else g + g_bi


def ref_fm_bwd(x, g_sum, g_bi, keep_x=True):
    """dx[b,f,:] = g (S - x[b,f,:]), g = g_sum[b] + g_bi[b,:].  K = F + 2.  keep_x False: fault (g), S in place of S - x"""
    return _fm_g(x, g_sum, g_bi)[:, None, :] * (x.sum(1, keepdim=True) - (x if keep_x else 0))


def _fm_bwd_abs(x, g_sum, g_bi):
    x = x.abs()
    g = _fm_g(x, None if g_sum is None else g_sum.abs(), None if g_bi is None else g_bi.abs())
    return g[:, None, :] * (x.sum(1, keepdim=True) + x)


@functools.lru_cache(maxsize=None)
def _fm_case(B, F, D):
    g = _gen(3, B, F, D)
    c = _ns(B=B, F=F, D=D)
    off = 3.0 * torch.randn(B, 1, D, generator=g)            # a common offset per (sample, column): s s and q nearly cancel
    c.x = off + 0.05 * torch.randn(B, F, D, generator=g)
    c.g_sum = torch.randn(B, generator=g)
    c.g_bi = torch.randn(B, D, generator=g)
    return c


# (B, F, D): TPR = lanes per sample
FM_CASES = [(65, 3, 4), (7, 5, 12), (33, 4, 260), (257, 7, 40), (1, 1, 8), (5, 2, 16)]
# D = 4: TPR 1; 8: TPR 2; 12: TPR 4 with 3 lanes busy; 16: TPR 4; 40: TPR 16 with 10 busy; 260: TPR 64, lane 0 walks two quads


# ------------------------------------------------------------------------------------------------------------- BatchNorm
BN_EPS = 1e-5


def ref_bn_stats(x, eps=BN_EPS):
    """x [M, N] float64 -> mean, biased var, rstd and their bars.
    mean: an M-term sum and the product with fl(1/M): gamma(u, M + 2) mean|x|.
    var:  the kernel's second pass around ITS fp32 mean mu^ = mu + dmu, |dmu| <= bar(mean).  Each term (x - mu^)^2 is off by
          at most 2 |x - mu| |dmu| + dmu^2 and carries three roundings relative to itself; the sum of M non-negative terms and
          the scaling add M + 1:   bar(var) = c + gamma(u, M + 4) (var + c),  c = 2 mean|x - mu| bar(mean) + bar(mean)^2.
          (An absolute-value bar over x^2 would hide the cancellation a one-pass E[x^2] - E[x]^2 suffers: fault (c).)
    rstd: d/dvar (var + eps)^-1/2 = -rstd^3 / 2, and an addition, a square root and a division of its own (4 u rstd)."""
    M = x.shape[0]
    mean = x.mean(0)
    b_mean = gamma(U, M + 2) * x.abs().mean(0)
    dev = (x - mean).abs()
    var = (dev * dev).mean(0)
    c = 2 * dev.mean(0) * b_mean + b_mean * b_mean
    b_var = c + gamma(U, M + 4) * (var + c)
    rstd = (var + eps) ** -0.5
    b_rstd = 0.5 * rstd ** 3 * b_var + 4 * U * rstd
    return _ns(mean=mean, var=var, rstd=rstd, b_mean=b_mean, b_var=b_var, b_rstd=b_rstd)


def ref_bn_apply(x, mean, rstd, gamma_, beta, b_mean=0.0, b_rstd=0.0):
    """y = (x - mean) (rstd gamma) + beta and its bar: |gamma| (rstd bar(mean) + |x - mean| bar(rstd)) from the statistics,
    and four roundings (difference, rstd gamma, product, sum) over |x - mean| rstd |gamma| + |beta|"""
    gm = 1.0 if gamma_ is None else gamma_
    bt = 0.0 if beta is None else beta
    dev = x - mean
    y = dev * (rstd * gm) + bt
    A = dev.abs() * rstd * abs(gm) + abs(bt)
    bar = abs(gm) * (rstd * b_mean + dev.abs() * b_rstd) + gamma(U, 4) * A
    return y, bar


def ref_bn_bwd_sums(x, dy, mean, rstd):
    """dbeta = sum_m dy (K = M);  dgamma = sum_m dy xhat, xhat = (x - mean) rstd (K = M + 3).  mean, rstd are inputs."""
    M = x.shape[0]
    xh = (x - mean) * rstd
    return (dy.sum(0), (dy * xh).sum(0), gamma(U, M) * dy.abs().sum(0), gamma(U, M + 3) * (dy * xh).abs().sum(0))


def ref_bn_bwd_apply(x, dy, mean, rstd, gamma_, mdy, mdyx, b_mdy=0.0, b_mdyx=0.0):
    """dx = gamma rstd (dy - mdy - xhat mdyx), six roundings over |gamma| rstd (|dy| + |mdy| + |xhat| |mdyx|), plus what the
    two means carry when the same call computed them"""
    gm = 1.0 if gamma_ is None else gamma_
    xh = (x - mean) * rstd
    k0 = abs(gm) * rstd
    dx = gm * rstd * (dy - mdy - xh * mdyx)
    bar = gamma(U, 6) * k0 * (dy.abs() + abs(mdy) + xh.abs() * abs(mdyx)) + k0 * (b_mdy + xh.abs() * b_mdyx)
    return dx, bar


def ref_bn_running(mean, var, rmean, rvar, tracked, momentum, M, unbias=True):
    """num_batches_tracked + 1;  m = momentum, or 1 / tracked when momentum < 0;  running = (1 - m) running + m stat, the
    variance times M / (M - 1) (1 when M = 1).  K = 5.  unbias False: fault (h)."""
    seen = (tracked if tracked is not None else 0) + 1
    m = momentum if momentum >= 0 else 1.0 / seen
    ub = M / (M - 1) if (M > 1 and unbias) else 1.0
    return ((1 - m) * rmean + m * mean, (1 - m) * rvar + m * var * ub,
            gamma(U, 5) * ((1 - m) * rmean.abs() + m * mean.abs()), gamma(U, 5) * ((1 - m) * rvar.abs() + m * var.abs() * ub), seen)


@functools.lru_cache(maxsize=None)
def _bn_case(M, N, offset_over_std=0.0):
    """column 0 is constant when N >= 5 (var = 0, rstd = 1 / sqrt(eps)); offset_over_std: every other column's mean / std"""
    g = _gen(4, M, N, int(offset_over_std))
    c = _ns(M=M, N=N)
    std = 0.5 + torch.rand(N, generator=g)
    base = offset_over_std * std if offset_over_std else 3.0 * torch.randn(N, generator=g)
    c.x = base + std * torch.randn(M, N, generator=g)
    if N >= 5:
        c.x[:, 0] = 1.7
    c.dy = torch.randn(M, N, generator=g)
    c.gamma = 1.0 + 0.5 * torch.randn(N, generator=g)
    c.beta = torch.randn(N, generator=g)
    c.st = ref_bn_stats(c.x.double())
    c.mean32, c.rstd32, c.var32 = c.st.mean.float(), c.st.rstd.float(), c.st.var.float()
    return c


# (M, N): bn_plan's shape and the finish kernel's nblk
BN_CASES = [
    (257, 1),     # one column, 256 rows per block row group; nblk = 1
    (257, 7),     # 8 columns x 32 rows; nblk = 3 (< 16)
    (70, 300),    # N >= 256: R = 1, two column blocks, rows = 4: nblk = 18 (> 16, 18 % 16 = 2)
    (33, 256),    # R = 1, one column block; nblk = 9
    (1, 5),       # M = 1
]
BN_OFFSET_CASE = (17, 5, 400.0)   # mean / std = 400: chosen on the CPU so that fault (c) misses bar(var) by >= 4x


def one_pass_var_fp32(x32):
    """fault (c): E[x^2] - E[x]^2 in fp32"""
    return ((x32 * x32).mean(0) - x32.mean(0) ** 2).double()


# ------------------------------------------------------------------------------------------------------------ Dice gate
def ref_dice(x, xhat, alpha, dy=None):
    """y = x (alpha + s (1 - alpha)), s = sigmoid(xhat);  dx_direct = dy (alpha + s (1 - alpha));  dxhat = dy x (1 - alpha)
    s (1 - s);  dal = dy x (1 - s).  The sigmoid is off by bs = U_SIG s (measured, see U_SIG); 1 - s by bs + eps; s (1 - s)
    by bs (1 - s) + s (bs + eps) <= bs + eps s.  Around that, 3-4 roundings of products over the absolute expression."""
    s = torch.sigmoid(xhat)
    bs = U_SIG * s
    k = alpha + s * (1 - alpha)
    ka = alpha.abs() + s * (1 - alpha).abs()
    r = _ns(s=s, y=x * k, b_y=x.abs() * ((1 - alpha).abs() * bs + gamma(U, 3) * ka))
    if dy is not None:
        r.dxd = dy * k
        r.b_dxd = dy.abs() * ((1 - alpha).abs() * bs + gamma(U, 3) * ka)
        gx = (dy * x).abs()
        r.dxh = dy * x * (1 - alpha) * s * (1 - s)
        r.b_dxh = gx * (1 - alpha).abs() * (bs + EPS * s + gamma(U, 5) * s * (1 - s))
        r.dal = dy * x * (1 - s)
        r.b_dal = gx * (bs + EPS + gamma(U, 3) * (1 - s))
    return r


@functools.lru_cache(maxsize=None)
def _dice_case(M, N):
    g = _gen(5, M, N)
    c = _ns(M=M, N=N)
    c.x = torch.randn(M, N, generator=g)
    c.xhat = torch.rand(M, N, generator=g) * 60.0 - 30.0
    c.xhat.view(-1)[0], c.xhat.view(-1)[-1] = -30.0, 30.0
    c.alpha = 0.25 + 0.5 * torch.randn(N, generator=g)
    c.dy = torch.randn(M, N, generator=g)
    return c


DICE_CASES = [(7, 5), (257, 33), (1, 1), ((16384 * 256) // 3 + 1, 3)]   # the last: M N = 4194306, two past the grid cap


# -------------------------------------------------------------------------------------------------------- attention
def _heads(m, H, a, raw=True):
    """[B, T, H a] -> [B, H, T, a].  raw: the reference's RAW view of the flat [T H a] buffer (head g, token t, dim j is
    flat element g T a + t a + j); raw False is fault (e), the [T, H, a] reshape a reader would expect"""
    B, T, _ = m.shape
    return m.reshape(B, H, T, a) if raw else m.reshape(B, T, H, a).transpose(1, 2)


def _unheads(h, raw=True):
    B, H, T, a = h.shape
    return h.reshape(B, T, H * a) if raw else h.transpose(1, 2).reshape(B, T, H * a)


def attn_ref(Q, K, V, R, H, a, scale, bQ=None, n_exp=1, raw=True, stats=None):
    """The T x T core in float64 with a bar for every stage.  Q, K, V, R: [B, T, H a] float64; bQ = (bar Q, bar K, bar V,
    bar R) or None when they are exact inputs; stats = (m, l) [B, H, T] given as inputs (the backward's recomputation
    P = exp(s - m) / l) instead of a softmax.  Bars, stage by stage (|.| absolute values, g(K) = gamma(u, K)):
      S  = Q K^T / scale         bS  = (g(a + 1) |Q||K|^T + bQ |K|^T + |Q| bK^T) / scale
      P  = softmax(S)            bP  = softmax_bar;   from stats: P (bS + 2 eps (|S| + |m|) + 3 u + |S - m| eps + 3 eps)
      O  = P V                   bO  = bP |V| + P bV + g(T + 2) P |V|
      Z  = O + R  (pre-ReLU)     bZ  = bO + bR + eps (|O| + |R|)"""
    B, T, _ = Q.shape
    z = torch.zeros_like(Q)
    bq, bk, bv, bR = (z, z, z, z) if bQ is None else bQ
    Qh, Kh, Vh = (_heads(t, H, a, raw) for t in (Q, K, V))
    bq, bk, bv = (_heads(t, H, a, raw) for t in (bq, bk, bv))
    inv = 1.0 / scale if scale > 0 else 1.0
    S = torch.einsum("bhic,bhjc->bhij", Qh, Kh) * inv
    bS = inv * (gamma(U, a + 1) * torch.einsum("bhic,bhjc->bhij", Qh.abs(), Kh.abs())
                + torch.einsum("bhic,bhjc->bhij", bq, Kh.abs()) + torch.einsum("bhic,bhjc->bhij", Qh.abs(), bk))
    if stats is None:
        P, bP = softmax_bar(S, bS, n_exp)
    else:
        m, l = stats[0].unsqueeze(-1), stats[1].unsqueeze(-1)
        P = torch.exp(S - m) / l
        bP = P * (bS + 2 * EPS * (S.abs() + m.abs()) + U_EXP + (S - m).abs() * EPS + 3 * EPS) + TINY
    Oh = torch.einsum("bhij,bhjc->bhic", P, Vh)
    bO = (torch.einsum("bhij,bhjc->bhic", bP, Vh.abs()) + torch.einsum("bhij,bhjc->bhic", P, bv)
          + gamma(U, T + 2) * torch.einsum("bhij,bhjc->bhic", P, Vh.abs()) + T * TINY)
    O, bO = _unheads(Oh, raw), _unheads(bO, raw)
    Z = O + R
    bZ = bO + bR + EPS * (O.abs() + R.abs())
    return _ns(Qh=Qh, Kh=Kh, Vh=Vh, bq=bq, bk=bk, bv=bv, S=S, bS=bS, P=P, bP=bP, O=O, Z=Z, bZ=bZ, inv=inv, H=H, a=a, T=T,
               raw=raw, out=Z.clamp_min(0.0), sure=Z.abs() > bZ)


def attn_ref_bwd(f, dZ):
    """Backward of the core from a forward record f and dZ [B, T, H a] = dout where the ReLU passed (exact).
      dP  = dO V^T                bdP = |dO| bV^T + g(a) |dO||V|^T                                   (dO = dZ)
      D   = sum_j P dP            bD  = sum_j (bP |dP| + P bdP) + g(T + 1) sum_j P |dP|
      dS  = P (dP - D) / scale    bdS = (bP |dP - D| + P (bdP + bD) + 3 eps P (|dP| + |D|)) / scale
      dV  = P^T dO                bdV = bP^T |dO| + g(T) P^T |dO|
      dQ  = dS K                  bdQ = bdS |K| + |dS| bK + g(T) |dS||K|         (dK the same with Q, transposed)
    -> dQ, dK, dV [B, T, H a] and their bars"""
    T, a = f.T, f.a
    dO = _heads(dZ, f.H, a, f.raw)
    aO = dO.abs()
    dP = torch.einsum("bhic,bhjc->bhij", dO, f.Vh)
    adP = torch.einsum("bhic,bhjc->bhij", aO, f.Vh.abs())
    bdP = torch.einsum("bhic,bhjc->bhij", aO, f.bv) + gamma(U, a) * adP
    D = (f.P * dP).sum(-1, keepdim=True)
    aD = (f.P * adP).sum(-1, keepdim=True)
    bD = (f.bP * dP.abs() + f.P * bdP).sum(-1, keepdim=True) + gamma(U, T + 1) * aD + T * TINY
    dS = f.P * (dP - D) * f.inv
    bdS = f.inv * (f.bP * (dP - D).abs() + f.P * (bdP + bD) + 3 * EPS * f.P * (adP + aD)) + 2 * TINY
    aS = dS.abs()
    dV = torch.einsum("bhij,bhic->bhjc", f.P, dO)
    bdV = torch.einsum("bhij,bhic->bhjc", f.bP, aO) + gamma(U, T) * torch.einsum("bhij,bhic->bhjc", f.P, aO) + T * TINY
    dQ = torch.einsum("bhij,bhjc->bhic", dS, f.Kh)
    bdQ = (torch.einsum("bhij,bhjc->bhic", bdS, f.Kh.abs()) + torch.einsum("bhij,bhjc->bhic", aS, f.bk)
           + gamma(U, T) * torch.einsum("bhij,bhjc->bhic", aS, f.Kh.abs()) + T * TINY)
    dK = torch.einsum("bhij,bhic->bhjc", dS, f.Qh)
    bdK = (torch.einsum("bhij,bhic->bhjc", bdS, f.Qh.abs()) + torch.einsum("bhij,bhic->bhjc", aS, f.bq)
           + gamma(U, T) * torch.einsum("bhij,bhic->bhjc", aS, f.Qh.abs()) + T * TINY)
    un = lambda t: _unheads(t, f.raw)
    return _ns(dQ=un(dQ), dK=un(dK), dV=un(dV), bdQ=un(bdQ), bdK=un(bdK), bdV=un(bdV))


def _score_inputs(kind, B, H, T, a, scale, g):
    """Q, K in head layout [B, H, T, a] whose scores Q K^T / scale are of a softmax kind: dimension 0 of q is 1 and of k the
    wanted logit (times scale), the other dimensions add a little noise ("equal": every key of a head is the same row)"""
    if kind == "normal":
        return torch.randn(B, H, T, a, generator=g), torch.randn(B, H, T, a, generator=g)
    Qh = 0.05 * torch.randn(B, H, T, a, generator=g)
    Kh = 0.05 * torch.randn(B, H, T, a, generator=g)
    if kind == "equal":
        return torch.randn(B, H, T, a, generator=g), Kh[:, :, :1].expand(B, H, T, a).contiguous()
    Qh[..., 0] = 1.0
    Kh[..., 0] = _logits(kind, (B, H, T), g) * (scale if scale > 0 else 1.0)
    return Qh, Kh


@functools.lru_cache(maxsize=None)
def _core_case(B, T, H, a, nproj, scaled, kind="normal"):
    """the split form's inputs: qkvr [B T, nproj H a] (+ xres when nproj = 3) and the reference with its bars"""
    g = _gen(6, B, T, H, a, nproj, int(scaled), SOFTMAX_KINDS.index(kind))
    HA = H * a
    scale = a ** 0.5 if scaled else 0.0
    c = _ns(B=B, T=T, H=H, a=a, HA=HA, nproj=nproj, scale=scale, kind=kind)
    Qh, Kh = _score_inputs(kind, B, H, T, a, scale, g)
    c.Q, c.K = Qh.reshape(B, T, HA), Kh.reshape(B, T, HA)   # the raw view back
    c.V = torch.randn(B, T, HA, generator=g)
    c.R = torch.randn(B, T, HA, generator=g)
    c.dout = torch.randn(B, T, HA, generator=g)
    c.f = attn_ref(c.Q.double(), c.K.double(), c.V.double(), c.R.double(), H, a, scale, n_exp=T)
    # what the backward is fed: the reference's out and a consistent (m, l), rounded to fp32
    c.out32 = c.f.out.float()
    m = c.f.S.max(-1).values
    c.m32 = m.float()
    c.l32 = torch.exp(c.f.S - c.m32.double().unsqueeze(-1)).sum(-1).float()
    return c


# (B, T, H, a, nproj, scaled, kind): samples per wave = 64 // (H T), 1 when H T >= 64
CORE_CASES = [
    (130, 1, 1, 1, 4, False, "normal"),    # H T = 1: 64 samples per wave, three waves, the last with 2; a = 1
    (23, 3, 2, 5, 4, True, "normal"),      # H T = 6: 10 samples on 60 lanes
    (5, 33, 1, 16, 4, True, "normal"),     # H T = 33: 1 sample on 33 lanes; a = AC_MAXA
    (5, 33, 1, 16, 3, False, "equal"),     # the same without W_res: the residual comes from xres
    (70, 1, 1, 16, 3, True, "normal"),     # a = 16 at 64 samples per wave, no W_res
    (7, 6, 1, 1, 3, False, "top80"),       # a = 1, no W_res
    (5, 13, 5, 3, 4, False, "pm60"),       # H T = 65 > 64: a second pass over the lanes; exp(s - m) underflows for most keys
    (9, 7, 2, 4, 4, True, "top80"),
    (9, 7, 2, 4, 3, True, "pm60"),
    (4, 26, 1, 8, 4, False, "equal"),      # two samples per wave (the shape the other tests use)
]


def _attn_nw(T, Din, H, a, has_res, bwd):
    """waves per workgroup as attn_plan chooses them (150 KB of LDS) — asserted by the cases below, not used by a kernel"""
    HA, nproj = H * a, 4 if has_res else 3
    o = T * (Din | 1) + 5 * T * HA + H * T * T + ((4 * T * HA + H * T * T) if bwd else 0)
    total, wpad, wlds = (o + 3) & ~3, (nproj * HA * Din + 3) & ~3, (nproj * HA * (Din | 1) + 3) & ~3
    for nw in (4, 3, 2, 1):
        if (wlds + (nw * wpad if bwd else 0) + nw * total) * 4 <= 150 * 1024:
            return nw
    return 0


def fused_ref(x, W, T, Din, H, a, has_res, scale, raw=True):
    """The one-launch layer: Q, K, V (, R) = X W_p^T, each a Din-term sum of products (bar g(Din) |X||W_p|^T), then the core;
    R = X itself without W_res (exact)"""
    HA = H * a
    Wp = W.reshape(-1, HA, Din)
    proj = [torch.einsum("btk,ck->btc", x, Wp[p]) for p in range(Wp.shape[0])]
    bars = [gamma(U, Din) * torch.einsum("btk,ck->btc", x.abs(), Wp[p].abs()) for p in range(Wp.shape[0])]
    if not has_res:
        proj.append(x)
        bars.append(torch.zeros_like(x))
    f = attn_ref(*proj, H, a, scale, bQ=tuple(bars), raw=raw)
    f.Wp, f.x = Wp, x
    return f


def fused_ref_bwd(f, gout, has_res):
    """dX = dQ Wq + dK Wk + dV Wv + dZ (Wres | I): nproj H a terms (+ 1);  dW_p[c, k] = sum_{b,t} d_p[b,t,c] X[b,t,k]: B T terms.
    Each with its operands' bars in front, as in attn_ref_bwd.  The ReLU decisions are taken from the reference: the caller
    gives a zero gout to the elements whose decision is not sure."""
    dZ = gout * (f.Z > 0)
    r = attn_ref_bwd(f, dZ)
    B, T, HA = dZ.shape
    ds = [(r.dQ, r.bdQ), (r.dK, r.bdK), (r.dV, r.bdV)] + ([(dZ, torch.zeros_like(dZ))] if has_res else [])
    n = len(ds) * HA + 1
    dx = sum(torch.einsum("btc,ck->btk", dv, f.Wp[p]) for p, (dv, _) in enumerate(ds))
    adx = sum(torch.einsum("btc,ck->btk", dv.abs(), f.Wp[p].abs()) for p, (dv, _) in enumerate(ds))
    bdx = sum(torch.einsum("btc,ck->btk", bv, f.Wp[p].abs()) for p, (_, bv) in enumerate(ds))
    if not has_res:
        dx, adx = dx + dZ, adx + dZ.abs()
    dW = torch.stack([torch.einsum("btc,btk->ck", dv, f.x) for dv, _ in ds])
    bdW = torch.stack([torch.einsum("btc,btk->ck", bv, f.x.abs())
                       + gamma(U, B * T) * torch.einsum("btc,btk->ck", dv.abs(), f.x.abs()) for dv, bv in ds])
    return _ns(dx=dx, bdx=bdx + gamma(U, n) * adx, dW=dW, bdW=bdW, dZ=dZ)


@functools.lru_cache(maxsize=None)
def _fused_case(B, T, Din, H, a, has_res, scaled, kind="normal"):
    g = _gen(7, B, T, Din, H, a, int(has_res), int(scaled), SOFTMAX_KINDS.index(kind))
    HA, nproj = H * a, 4 if has_res else 3
    scale = a ** 0.5 if scaled else 0.0
    c = _ns(B=B, T=T, Din=Din, H=H, a=a, HA=HA, has_res=has_res, scale=scale, nproj=nproj, kind=kind)
    c.x = torch.randn(B, T, Din, generator=g)
    c.W = torch.randn(nproj * HA, Din, generator=g) / Din ** 0.5
    if kind != "normal":   # H = 1 (the head split is then the identity): q[0] = x[0] = 1, k[0] = x[1] = the wanted logit
        assert H == 1 and Din >= 2 and has_res
        c.W = 0.05 * c.W
        if kind == "equal":
            c.W[:HA] = 0.0                                   # q = 0: every score is 0
        else:
            c.x[..., 0] = 1.0
            c.x[..., 1] = _logits(kind, (B, T), g) * (scale if scale > 0 else 1.0)
            c.W[0], c.W[HA] = 0.0, 0.0
            c.W[0, 0], c.W[HA, 1] = 1.0, 1.0
    c.gout = torch.randn(B, T, HA, generator=g)
    c.f = fused_ref(c.x.double(), c.W.double(), T, Din, H, a, has_res, scale)
    # The backward recomputes the forward, so a ReLU decision the reference cannot make (|Z| within its bar) would decide a
    # whole row of dx and every dW: those elements (at most 0.1 % of the case, asserted) get a zero upstream gradient, with
    # which either decision gives the same result
    c.left_out = int((~c.f.sure).sum())
    assert c.left_out <= EXCLUDED_CAP * c.f.Z.numel()
    c.gout[~c.f.sure] = 0.0
    return c


# (B, T, Din, H, a, has_res, scaled, kind)
FUSED_CASES = [
    (7, 17, 7, 4, 10, True, True, "normal"),     # odd Din (Dx = Din); the backward runs NW = 3 waves
    (9, 33, 16, 4, 8, True, False, "normal"),    # the forward runs NW = 3, the backward NW = 1
    (33, 1, 5, 1, 3, True, False, "normal"),     # T = 1
    (13, 7, 6, 3, 2, False, True, "normal"),     # no W_res (Din = H a): the residual is X
    (5, 9, 4, 1, 3, True, False, "equal"),
    (5, 9, 4, 1, 3, True, True, "top80"),
    (5, 9, 4, 1, 3, True, False, "pm60"),
    (2048 * 4 + 3, 2, 4, 1, 2, True, False, "normal"),   # the persistent loop: B > 2048 NW, each wave's LDS region reused
]
EXCLUDED_CAP = 1e-3   # at most 0.1 % of a case's elements may sit within their bar of the ReLU's zero


# =================================================================================================== device helpers
def _in(x2, ld=None, fill=1e6, off=0):
    """[R, n] (CPU) -> a device [R, n] view of rows ld floats apart, the columns behind n filled; off: floats by which the
    first row is off 16-byte alignment"""
    R, n = x2.shape
    ld = n if ld is None else ld
    flat = torch.full((off + R * ld + 4,), fill, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    buf = flat[off:off + R * ld].view(R, ld)
    buf[:, :n] = x2.to(DEV)
    return buf


def _vec(v):
    return v.reshape(-1).to(DEV).contiguous()


class _Out:
    """an output of R rows of n owned floats, ld apart, inside a NaN-filled buffer with 8 floats behind it and `off` before"""

    def __init__(self, R, n, ld=None, off=0, dtype=torch.float32):
        self.R, self.n, self.ld, self.off = R, n, (n if ld is None else ld), off
        self.flat = torch.full((off + R * self.ld + 8,), NAN, dtype=dtype, device=DEV)
        self.buf = self.flat[off:off + R * self.ld].view(R, self.ld)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def owned(self, tag, zero_to=None):
        """every owned element finite, everything else still NaN (columns [n, zero_to) exactly zero instead) -> [R, n]"""
        assert bool(torch.isnan(self.flat[:self.off]).all()) and bool(torch.isnan(self.flat[self.off + self.R * self.ld:]).all()), \
            f"{tag}: wrote outside its buffer"
        lo = self.n
        if zero_to is not None and zero_to > self.n:
            assert bool((self.buf[:, self.n:zero_to] == 0).all()), f"{tag}: columns [{self.n}, {zero_to}) are not exact zeros"
            lo = zero_to
        assert bool(torch.isnan(self.buf[:, lo:]).all()), f"{tag}: wrote into columns it does not own"
        own = self.buf[:, :self.n]
        assert bool(torch.isfinite(own).all()), f"{tag}: an owned element is not finite (left unwritten?)"
        return own


def _p(t):
    return None if t is None else (t.ptr if isinstance(t, _Out) else t.data_ptr())


def _rc(hip, name, *args):
    return getattr(hip.lib(), name)(*args, hip._stream())


def _ok(hip, name, *args):
    rc = _rc(hip, name, *args)
    assert rc == 0, f"{name}: code {rc}: {hip.lib().rp_last_error().decode()}"


def _bn_ws(hip, M, N):
    nb = C.c_size_t(0)
    assert hip.lib().rp_batchnorm_workspace_bytes(M, N, C.byref(nb)) == 0
    return torch.empty(nb.value, dtype=torch.uint8, device=DEV), nb.value


def _check(tag, got, ref, bar):
    """assert |got - ref| <= bar elementwise (exactly equal where the bar is 0); prints and returns max err / bar"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite values"
    bar = bar if torch.is_tensor(bar) else torch.full_like(ref, bar)
    bar = bar.expand_as(ref)
    err = (got - ref).abs()
    zero = bar == 0
    assert bool((err[zero] == 0).all()), f"{tag}: differs where the bar is zero"
    ratio = float((err[~zero] / bar[~zero]).max()) if bool((~zero).any()) else 0.0
    print(f"{tag}: max err/bar = {ratio:.4f}")
    assert ratio <= 1.0, f"{tag}: err / bar = {ratio:.3f} > 1"
    return ratio


def _check_relu(tag, got, f, cap=EXCLUDED_CAP):
    """an attention output: the ReLU's decision is exact and the value within bar(Z) wherever the reference's pre-activation
    is further from zero than bar(Z); the other elements (at most `cap` of the case) are left out"""
    got = got.detach().double().cpu().reshape(f.Z.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite values"
    left_out = int((~f.sure).sum())
    assert left_out <= cap * f.Z.numel(), f"{tag}: {left_out} of {f.Z.numel()} elements within their bar of zero"
    assert bool(((got > 0) == (f.Z > 0))[f.sure].all()), f"{tag}: a ReLU decision differs"
    return _check(tag, got[f.sure], f.out[f.sure], f.bZ[f.sure])


# =================================================================================================== CrossNet
@pytest.mark.gpu
@pytest.mark.parametrize("B,d,ld,L,mis", CROSS_CASES)
def test_crossnet_fwd(hip, B, d, ld, L, mis):
    """rp_crossnet_fwd alone: xout, logit and s_out in the three output combinations.  The VEC form loads the row's padding
    unconditionally and selects it away: there it holds NaN, elsewhere 1e6."""
    c = _cross_case(B, d, L)
    off = 1 if mis else 0
    vec = ld % 4 == 0 and not mis
    x0 = _in(c.x0, ld, NAN if vec else 1e6, off)
    W, Bv, wfc, bfc = _vec(c.W), _vec(c.Bv), _vec(c.wfc), _vec(c.bfc)
    bs, bx, bl = _cross_bars(c)
    for want_x, want_logit, want_s in ((True, False, True), (False, True, True), (True, True, False)):
        xout = _Out(B, d, ld, off) if want_x else None
        logit = _Out(1, B) if want_logit else None
        s = _Out(B, L) if want_s else None
        _ok(hip, "rp_crossnet_fwd", x0.data_ptr(), ld, d, L, W.data_ptr(), Bv.data_ptr(), wfc.data_ptr() if want_logit else None,
            bfc.data_ptr() if want_logit else None, _p(xout), ld, _p(logit), _p(s), B)
        tag = f"crossnet_fwd[{B},{d},{ld},{L}{' misaligned' if mis else ''} x={int(want_x)} logit={int(want_logit)}]"
        if want_x:
            _check(tag + " xout", xout.owned(tag), c.xout, bx)
        if want_logit:
            _check(tag + " logit", logit.owned(tag), c.logit, bl)
        if want_s:
            _check(tag + " s", s.owned(tag), c.s, bs)


@pytest.mark.gpu
@pytest.mark.parametrize("B,d,ld,L,mis", CROSS_CASES + [(5, 250, 260, 2, False)])
def test_crossnet_bwd_rows(hip, B, d, ld, L, mis):
    """rp_crossnet_bwd_rows alone, fed the reference's s rounded to fp32: dx0 and the 2L+2 columns of V, for g_x only, g_logit
    only and both.  The contract hip.crossnet_bwd_rows relies on is asserted: the VEC form leaves exact zeros in columns
    [d, min(ld, dp)) of dx0 and nothing in [dp, ld); the scalar form writes nothing past d."""
    c = _cross_case(B, d, L)
    off = 1 if mis else 0
    vec = ld % 4 == 0 and not mis
    dp = (d + 255) // 256 * 256
    x0 = _in(c.x0, ld, NAN if vec else 1e6, off)
    gx = _in(c.g_x, ld, NAN if vec else 1e6, off)
    W, wfc, s32, gl = _vec(c.W), _vec(c.wfc), _vec(c.s32), _vec(c.g_logit)
    for gmode in ("g_x", "g_logit", "both"):
        dx0r, Vr, bdx, bV = _cross_bwd_ref(c, gmode)
        dx0, V = _Out(B, d, ld, off), _Out(B, 2 * L + 2)
        _ok(hip, "rp_crossnet_bwd_rows", x0.data_ptr(), ld, d, L, W.data_ptr(), wfc.data_ptr(), s32.data_ptr(),
            None if gmode == "g_logit" else gx.data_ptr(), ld, None if gmode == "g_x" else gl.data_ptr(), dx0.ptr, ld, V.ptr, B)
        tag = f"crossnet_bwd_rows[{B},{d},{ld},{L}{' misaligned' if mis else ''} {gmode}]"
        _check(tag + " dx0", dx0.owned(tag, zero_to=min(ld, dp) if vec else None), dx0r, bdx)
        _check(tag + " V", V.owned(tag), Vr, bV)


@pytest.mark.gpu
@pytest.mark.parametrize("d,L", CROSS_PARAM)
def test_crossnet_param_grads(hip, d, L):
    """rp_crossnet_param_grads alone from a given P (rows 3 floats wider than d) and cs: with wfc (dwfc, extra = wfc sgl),
    with colg, and with neither"""
    c = _cross_case(5, d, L)
    q = c.d64
    P = _in(c.P, d + 3)
    cs, W, Bv, wfc, colg = _vec(c.cs), _vec(c.W), _vec(c.Bv), _vec(c.wfc), _vec(c.colg)
    g = gamma(U, _K_cross("param", d, L))
    for mode in ("wfc", "colg", "none"):
        w64, cg64 = (q.wfc if mode == "wfc" else None), (q.colg if mode == "colg" else None)
        ref = ref_cross_param(q.P, q.cs, q.W, q.Bv, w64, cg64)
        A = ref_cross_param(q.P.abs(), q.cs.abs(), q.W.abs(), q.Bv.abs(), None if w64 is None else w64.abs(),
                            None if cg64 is None else cg64.abs())
        dW, dB, dwfc = _Out(L, d), _Out(L, d), (_Out(1, d) if mode == "wfc" else None)
        _ok(hip, "rp_crossnet_param_grads", P.data_ptr(), d + 3, cs.data_ptr(), W.data_ptr(), Bv.data_ptr(),
            wfc.data_ptr() if mode == "wfc" else None, colg.data_ptr() if mode == "colg" else None, L, d, dW.ptr, dB.ptr, _p(dwfc))
        tag = f"crossnet_param_grads[{d},{L} {mode}]"
        _check(tag + " dW", dW.owned(tag), ref[0], g * A[0])
        if mode == "none" and L == 1:   # dB[L-1] is then an exact zero
            assert bool((dB.owned(tag) == 0).all())
        else:
            _check(tag + " dB", dB.owned(tag), ref[1], g * A[1])
        if dwfc is not None:
            _check(tag + " dwfc", dwfc.owned(tag), ref[2], g * A[2])


# =================================================================================================== MMOE
def _mmoe_z(c, extra, off):
    B, KE, TE = c.B, c.K * c.E, c.T * c.E
    return _in(torch.cat([c.ze.reshape(B, KE), c.lg.reshape(B, TE)], 1), KE + TE + extra, 1e6, off)


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,E,T,extra,off,kind", MMOE_CASES)
def test_mmoe_combine_fwd(hip, B, K, E, T, extra, off, kind):
    """rp_mmoe_combine_fwd alone: gate against the softmax bar, out = sum_e z gate with the gate's bar carried through;
    rows of gate sum to 1 within the sum of their bars"""
    c = _mmoe_case(B, K, E, T, kind)
    z = _mmoe_z(c, extra, off)
    out, gate = _Out(T * B, K), _Out(B, T * E)
    _ok(hip, "rp_mmoe_combine_fwd", z.data_ptr(), z.stride(0), K, E, T, out.ptr, gate.ptr, B)
    tag = f"mmoe_combine_fwd[{B},{K},{E},{T} +{extra} off={off} {kind}]"
    gt = gate.owned(tag)
    _check(tag + " gate", gt, c.gate, c.b_gate)
    _check(tag + " gate row sums", gt.double().cpu().view(B, T, E).sum(-1), torch.ones(B, T, dtype=torch.float64),
           c.b_gate.sum(-1) + E * EPS)
    _check(tag + " out", out.owned(tag), c.out, c.b_out)


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,E,T,extra,off,kind", MMOE_CASES)
def test_mmoe_combine_bwd(hip, B, K, E, T, extra, off, kind):
    """rp_mmoe_combine_bwd alone with the reference's gate (rounded to fp32) as input: the expert and the gate columns of dz"""
    c = _mmoe_case(B, K, E, T, kind)
    z = _mmoe_z(c, extra, off)
    gate, dout = _vec(c.gate32), _vec(c.dout)
    dz = _Out(B, K * E + T * E, z.stride(0), off)
    _ok(hip, "rp_mmoe_combine_bwd", z.data_ptr(), z.stride(0), K, E, T, gate.data_ptr(), dout.data_ptr(), dz.ptr, z.stride(0), B)
    g64 = c.gate32.double()
    dze, dlg = ref_mmoe_bwd(c.ze.double(), g64, c.dout.double())
    aze, alg = _mmoe_bwd_abs(c.ze.double(), g64, c.dout.double())
    tag = f"mmoe_combine_bwd[{B},{K},{E},{T} +{extra} off={off} {kind}]"
    got = dz.owned(tag)
    _check(tag + " dz experts", got[:, :K * E], dze, _mmoe_bwd_bars(c, aze, alg)[0])
    _check(tag + " dz gates", got[:, K * E:], dlg, _mmoe_bwd_bars(c, aze, alg)[1])


# =================================================================================================== FM pooling
@pytest.mark.gpu
@pytest.mark.parametrize("B,F,D", FM_CASES)
def test_fm_pool_fwd(hip, B, F, D):
    c = _fm_case(B, F, D)
    x = _in(c.x.reshape(B, F * D), F * D + 4)
    bi, sm = ref_fm_fwd(c.x.double())
    abi, asm = _fm_fwd_abs(c.x.double())
    for want_sum, want_bi in ((True, False), (False, True), (True, True)):
        o_sum, o_bi = (_Out(1, B) if want_sum else None), (_Out(B, D) if want_bi else None)
        _ok(hip, "rp_fm_pool_fwd", x.data_ptr(), F * D + 4, F, D, _p(o_sum), _p(o_bi), B)
        tag = f"fm_pool_fwd[{B},{F},{D} sum={int(want_sum)} bi={int(want_bi)}]"
        if want_bi:
            _check(tag + " bi", o_bi.owned(tag), bi, gamma(U, 2 * F) * abi)
        if want_sum:
            _check(tag + " sum", o_sum.owned(tag), sm, gamma(U, 2 * F + D) * asm)


@pytest.mark.gpu
@pytest.mark.parametrize("B,F,D", FM_CASES)
def test_fm_pool_bwd(hip, B, F, D):
    c = _fm_case(B, F, D)
    x = _in(c.x.reshape(B, F * D), F * D + 4)
    gs, gb = _vec(c.g_sum), _vec(c.g_bi)
    for use_sum, use_bi in ((True, False), (False, True), (True, True)):
        dx = _Out(B, F * D, F * D + 8)
        _ok(hip, "rp_fm_pool_bwd", x.data_ptr(), F * D + 4, F, D, gs.data_ptr() if use_sum else None,
            gb.data_ptr() if use_bi else None, dx.ptr, F * D + 8, B)
        s64, b64 = (c.g_sum.double() if use_sum else None), (c.g_bi.double() if use_bi else None)
        tag = f"fm_pool_bwd[{B},{F},{D} g_sum={int(use_sum)} g_bi={int(use_bi)}]"
        _check(tag + " dx", dx.owned(tag), ref_fm_bwd(c.x.double(), s64, b64).reshape(B, F * D),
               gamma(U, F + 2) * _fm_bwd_abs(c.x.double(), s64, b64).reshape(B, F * D))


# =================================================================================================== BatchNorm
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,ratio", [(M, N, 0.0) for M, N in BN_CASES] + [BN_OFFSET_CASE])
def test_batchnorm_train_fwd(hip, M, N, ratio):
    """rp_batchnorm_train_fwd alone: mean, var, rstd and y against ref_bn_stats / ref_bn_apply, with and without gamma / beta"""
    c = _bn_case(M, N, ratio)
    x = _in(c.x, N + 3)
    ws, nb = _bn_ws(hip, M, N)
    for affine in (True, False):
        y, mean, var, rstd = _Out(M, N, N + 2), _Out(1, N), _Out(1, N), _Out(1, N)
        gm, bt = (_vec(c.gamma), _vec(c.beta)) if affine else (None, None)
        _ok(hip, "rp_batchnorm_train_fwd", x.data_ptr(), N + 3, _p(gm), _p(bt), BN_EPS, y.ptr, N + 2, mean.ptr, var.ptr, rstd.ptr,
            M, N, ws.data_ptr(), nb)
        tag = f"batchnorm_train_fwd[{M},{N} mean/std={ratio:g} affine={int(affine)}]"
        st = c.st
        _check(tag + " mean", mean.owned(tag), st.mean.view(1, N), st.b_mean.view(1, N))
        _check(tag + " var", var.owned(tag), st.var.view(1, N), st.b_var.view(1, N))
        _check(tag + " rstd", rstd.owned(tag), st.rstd.view(1, N), st.b_rstd.view(1, N))
        yr, by = ref_bn_apply(c.x.double(), st.mean, st.rstd, c.gamma.double() if affine else None,
                              c.beta.double() if affine else None, st.b_mean, st.b_rstd)
        _check(tag + " y", y.owned(tag), yr, by)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,ratio", [(M, N, 0.0) for M, N in BN_CASES] + [BN_OFFSET_CASE])
def test_batchnorm_bwd_and_apply(hip, M, N, ratio):
    """rp_batchnorm_train_bwd, _bwd_sums, _bwd_apply (global means that differ from the local ones), _apply, _apply_bwd and
    _colsum (plain and centred), each alone, fed the reference's mean / rstd rounded to fp32 as exact inputs"""
    c = _bn_case(M, N, ratio)
    x, dy = _in(c.x, N + 3), _in(c.dy, N + 1)
    mean, rstd = _vec(c.mean32), _vec(c.rstd32)
    x64, dy64, m64, r64 = c.x.double(), c.dy.double(), c.mean32.double(), c.rstd32.double()
    ws, nb = _bn_ws(hip, M, N)
    dbr, dgr, b_db, b_dg = ref_bn_bwd_sums(x64, dy64, m64, r64)
    mdy, mdyx = dbr / M, dgr / M
    b_mdy, b_mdyx = b_db / M + 2 * EPS * mdy.abs(), b_dg / M + 2 * EPS * mdyx.abs()
    base = f"[{M},{N} mean/std={ratio:g}]"
    for affine in (True, False):
        gm, g64 = (_vec(c.gamma), c.gamma.double()) if affine else (None, None)
        bt, b64 = (_vec(c.beta), c.beta.double()) if affine else (None, None)
        tag = f"batchnorm_train_bwd{base[:-1]} affine={int(affine)}]"
        dx, dgamma, dbeta = _Out(M, N, N + 2), _Out(1, N), _Out(1, N)
        _ok(hip, "rp_batchnorm_train_bwd", x.data_ptr(), N + 3, dy.data_ptr(), N + 1, mean.data_ptr(), rstd.data_ptr(), _p(gm),
            dx.ptr, N + 2, dgamma.ptr, dbeta.ptr, M, N, ws.data_ptr(), nb)
        _check(tag + " dbeta", dbeta.owned(tag), dbr.view(1, N), b_db.view(1, N))
        _check(tag + " dgamma", dgamma.owned(tag), dgr.view(1, N), b_dg.view(1, N))
        _check(tag + " dx", dx.owned(tag), *ref_bn_bwd_apply(x64, dy64, m64, r64, g64, mdy, mdyx, b_mdy, b_mdyx))
        tag = f"batchnorm_bwd_apply{base[:-1]} affine={int(affine)}]"
        gdy, gdyx = (1.3 * mdy + 0.1).float(), (0.7 * mdyx - 0.2).float()   # another rank's share moved the means
        dx, gdy_d, gdyx_d = _Out(M, N, N + 2), _vec(gdy), _vec(gdyx)
        _ok(hip, "rp_batchnorm_bwd_apply", x.data_ptr(), N + 3, dy.data_ptr(), N + 1, mean.data_ptr(), rstd.data_ptr(), _p(gm),
            gdy_d.data_ptr(), gdyx_d.data_ptr(), dx.ptr, N + 2, M, N)
        _check(tag + " dx", dx.owned(tag), *ref_bn_bwd_apply(x64, dy64, m64, r64, g64, gdy.double(), gdyx.double()))
        tag = f"batchnorm_apply{base[:-1]} affine={int(affine)}]"
        y = _Out(M, N, N + 2)
        _ok(hip, "rp_batchnorm_apply", x.data_ptr(), N + 3, mean.data_ptr(), rstd.data_ptr(), _p(gm), _p(bt), y.ptr, N + 2, M, N)
        _check(tag + " y", y.owned(tag), *ref_bn_apply(x64, m64, r64, g64, b64))
        dx = _Out(M, N, N + 2)
        _ok(hip, "rp_batchnorm_apply_bwd", dy.data_ptr(), N + 1, rstd.data_ptr(), _p(gm), dx.ptr, N + 2, M, N)
        k0 = r64 * (g64 if affine else 1.0)
        _check(f"batchnorm_apply_bwd{base[:-1]} affine={int(affine)}] dx", dx.owned(tag), dy64 * k0, gamma(U, 2) * (dy64 * k0).abs())
    tag = f"batchnorm_bwd_sums{base}"
    dgamma, dbeta = _Out(1, N), _Out(1, N)
    _ok(hip, "rp_batchnorm_bwd_sums", x.data_ptr(), N + 3, dy.data_ptr(), N + 1, mean.data_ptr(), rstd.data_ptr(), dgamma.ptr,
        dbeta.ptr, M, N, ws.data_ptr(), nb)
    _check(tag + " dbeta", dbeta.owned(tag), dbr.view(1, N), b_db.view(1, N))
    _check(tag + " dgamma", dgamma.owned(tag), dgr.view(1, N), b_dg.view(1, N))
    tag = f"batchnorm_colsum{base}"
    out = _Out(1, N)
    _ok(hip, "rp_batchnorm_colsum", x.data_ptr(), N + 3, None, out.ptr, M, N, ws.data_ptr(), nb)
    _check(tag + " sum", out.owned(tag), x64.sum(0).view(1, N), (gamma(U, M) * x64.abs().sum(0)).view(1, N))
    center = (c.mean32 + 0.01 * c.mean32.abs() + 0.01).float()   # a global mean that is not the local one
    out, center_d = _Out(1, N), _vec(center)
    _ok(hip, "rp_batchnorm_colsum", x.data_ptr(), N + 3, center_d.data_ptr(), out.ptr, M, N, ws.data_ptr(), nb)
    sq = ((x64 - center.double()) ** 2).sum(0)
    _check(tag + " centred", out.owned(tag), sq.view(1, N), (gamma(U, M + 3) * sq).view(1, N))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,momentum,counter", [(257, 7, 0.1, 3), (257, 7, -1.0, 3), (1, 5, 0.1, 0), (70, 300, -1.0, 0),
                                                  (33, 256, 0.25, None), (33, 256, -1.0, None)])
def test_batchnorm_update_running(hip, M, N, momentum, counter):
    """rp_batchnorm_update_running alone: exponential and cumulative (momentum < 0) averages, the M / (M - 1) factor (1 at
    M = 1), a null counter (counts as the first batch); num_batches_tracked exactly"""
    c = _bn_case(M, N)
    g = _gen(8, M, N)
    rm0, rv0 = torch.randn(N, generator=g), 0.5 + torch.rand(N, generator=g)
    rm, rv = _Out(1, N), _Out(1, N)
    rm.buf[0], rv.buf[0] = rm0.to(DEV), rv0.to(DEV)
    tr = None
    if counter is not None:
        tr = torch.tensor([counter, -77], dtype=torch.int64, device=DEV)
    mean, var = _vec(c.mean32), _vec(c.var32)
    _ok(hip, "rp_batchnorm_update_running", mean.data_ptr(), var.data_ptr(), rm.ptr, rv.ptr, _p(tr), momentum, M, N)
    rmr, rvr, b_rm, b_rv, seen = ref_bn_running(c.mean32.double(), c.var32.double(), rm0.double(), rv0.double(), counter, momentum, M)
    tag = f"batchnorm_update_running[{M},{N} momentum={momentum} counter={counter}]"
    _check(tag + " running_mean", rm.owned(tag), rmr.view(1, N), b_rm.view(1, N))
    _check(tag + " running_var", rv.owned(tag), rvr.view(1, N), b_rv.view(1, N))
    if tr is not None:
        assert tr.tolist() == [seen, -77]


# =================================================================================================== Dice gate
@pytest.mark.gpu
def test_dice_sigmoid_accuracy(hip):
    """The gate's sigmoid alone (x = 1, alpha = 0 make y = s exactly) over 240001 points of [-30, 30] against float64: prints
    the worst relative error, which EXPF_SIGMOID_MEASURED records, and holds it under U_SIG = twice the recorded figure"""
    n = 240001
    xh = torch.linspace(-30.0, 30.0, n, dtype=torch.float64).float()
    y = _Out(n, 1)
    one, xh_d, zero = torch.ones(n, device=DEV), xh.to(DEV), torch.zeros(1, device=DEV)
    _ok(hip, "rp_dice_gate_fwd", one.data_ptr(), 1, xh_d.data_ptr(), 1, zero.data_ptr(), y.ptr, 1, n, 1)
    s = torch.sigmoid(xh.double())
    rel = (y.owned("dice sigmoid").double().cpu().view(-1) - s).abs() / s
    k = int(rel.argmax())
    print(f"dice sigmoid (__expf): worst relative error {float(rel[k]):.3e} at xhat = {float(xh[k]):.4f} "
          f"(recorded {EXPF_SIGMOID_MEASURED:.1e}, U_SIG = {U_SIG:.1e}); for |xhat| <= 10: {float(rel[xh.abs() <= 10].max()):.3e}")
    assert float(rel.max()) <= U_SIG


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", DICE_CASES)
def test_dice_gate(hip, M, N):
    """rp_dice_gate_fwd and rp_dice_gate_bwd alone, xhat out to +-30 (ref_dice has the bars)"""
    c = _dice_case(M, N)
    x, xh, dy, al = _in(c.x, N + 1), _in(c.xhat, N + 2), _in(c.dy, N + 3), _vec(c.alpha)
    r = ref_dice(c.x.double(), c.xhat.double(), c.alpha.double(), c.dy.double())
    y = _Out(M, N, N + 1)
    _ok(hip, "rp_dice_gate_fwd", x.data_ptr(), N + 1, xh.data_ptr(), N + 2, al.data_ptr(), y.ptr, N + 1, M, N)
    tag = f"dice_gate[{M},{N}]"
    _check(tag + " y", y.owned(tag), r.y, r.b_y)
    dxd, dxh, dal = _Out(M, N), _Out(M, N), _Out(M, N)
    _ok(hip, "rp_dice_gate_bwd", x.data_ptr(), N + 1, xh.data_ptr(), N + 2, al.data_ptr(), dy.data_ptr(), N + 3, dxd.ptr, dxh.ptr,
        dal.ptr, M, N)
    _check(tag + " dx_direct", dxd.owned(tag), r.dxd, r.b_dxd)
    _check(tag + " dxhat", dxh.owned(tag), r.dxh, r.b_dxh)
    _check(tag + " dal", dal.owned(tag), r.dal, r.b_dal)


# =================================================================================================== rp_accumulate
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 4100])
def test_accumulate(hip, n):
    """dst += src: the 16-byte form with its n % 4 tail, and the unaligned form (either pointer 4 bytes off: n4 = 0)"""
    g = _gen(9, n)
    a, b = torch.randn(1, n, generator=g), torch.randn(1, n, generator=g)
    for off_d, off_s in ((0, 0), (1, 0), (0, 1), (1, 1)):
        dst = _Out(1, n, off=off_d)
        dst.buf[0] = a[0].to(DEV)
        src = _in(b, n, 1e6, off_s)
        _ok(hip, "rp_accumulate", dst.ptr, src.data_ptr(), n)
        tag = f"accumulate[{n} off={off_d},{off_s}]"
        _check(tag + " dst", dst.owned(tag), a.double() + b.double(), gamma(U, 1) * (a.double().abs() + b.double().abs()))


# =================================================================================================== attention core
def _core_qkvr(c, pad):
    parts = [c.Q, c.K, c.V] + ([c.R] if c.nproj == 4 else [])
    return _in(torch.cat(parts, 2).reshape(c.B * c.T, c.nproj * c.HA), c.nproj * c.HA + pad)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,a,nproj,scaled,kind", CORE_CASES)
def test_attention_core_fwd(hip, B, T, H, a, nproj, scaled, kind):
    """rp_attention_core_fwd alone.  out through _check_relu; the statistics through P_ij = exp(s_ij - m_i) / l_i with the
    reference's s (not bit for bit: any (m, l) that describes the same row passes), rows of P summing to 1 within their bars,
    and m within the bar of the scores"""
    c = _core_case(B, T, H, a, nproj, scaled, kind)
    HA, HT, f = c.HA, H * T, c.f
    qkvr = _core_qkvr(c, 3)
    xres = _in(c.R.reshape(B * T, HA), HA + 1) if nproj == 3 else None
    out, stats = _Out(B * T, HA), _Out(B * HT, 2)
    _ok(hip, "rp_attention_core_fwd", qkvr.data_ptr(), qkvr.stride(0), nproj, _p(xres), HA + 1 if nproj == 3 else 0, T, H, a,
        c.scale, out.ptr, stats.ptr, B)
    tag = f"attention_core_fwd[{B},{T},{H},{a} nproj={nproj} scaled={int(scaled)} {kind}]"
    _check_relu(tag + " out", out.owned(tag), f)
    st = stats.owned(tag).double().cpu().view(B, H, T, 2)
    m, l = st[..., 0], st[..., 1]
    mr = f.S.max(-1).values
    _check(tag + " m", m, mr, f.bS.max(-1).values + EPS * mr.abs())
    P = torch.exp(f.S - m.unsqueeze(-1)) / l.unsqueeze(-1)
    _check(tag + " P from (m, l)", P, f.P, f.bP)
    _check(tag + " P row sums", P.sum(-1), torch.ones_like(m), f.bP.sum(-1))
    out2 = _Out(B * T, HA)   # the statistics are optional
    _ok(hip, "rp_attention_core_fwd", qkvr.data_ptr(), qkvr.stride(0), nproj, _p(xres), HA + 1 if nproj == 3 else 0, T, H, a,
        c.scale, out2.ptr, None, B)
    assert torch.equal(out2.owned(tag), out.buf)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,a,nproj,scaled,kind", CORE_CASES)
def test_attention_core_bwd(hip, B, T, H, a, nproj, scaled, kind):
    """rp_attention_core_bwd alone, fed the reference's out and a consistent (m, l), rounded to fp32: dQ, dK, dV within
    attn_ref_bwd's bars (P recomputed from the given statistics, as the kernel does), dR / dxres an exact masked copy"""
    c = _core_case(B, T, H, a, nproj, scaled, kind)
    HA, HT = c.HA, H * T
    qkvr = _core_qkvr(c, 3)
    f = attn_ref(c.Q.double(), c.K.double(), c.V.double(), c.R.double(), H, a, c.scale, stats=(c.m32.double(), c.l32.double()))
    dZ = c.dout.double() * (c.out32 > 0)
    r = attn_ref_bwd(f, dZ)
    stats = _vec(torch.stack([c.m32, c.l32], -1))
    dq = _Out(B * T, nproj * HA, nproj * HA + 2)
    dxres = _Out(B * T, HA, HA + 3) if nproj == 3 else None
    out_d, dout_d = _vec(c.out32), _vec(c.dout)
    _ok(hip, "rp_attention_core_bwd", qkvr.data_ptr(), qkvr.stride(0), nproj, out_d.data_ptr(), dout_d.data_ptr(),
        stats.data_ptr(), T, H, a, c.scale, dq.ptr, nproj * HA + 2, _p(dxres), HA + 3 if nproj == 3 else 0, B)
    tag = f"attention_core_bwd[{B},{T},{H},{a} nproj={nproj} scaled={int(scaled)} {kind}]"
    got = dq.owned(tag)
    for p, (name, ref, bar) in enumerate((("dQ", r.dQ, r.bdQ), ("dK", r.dK, r.bdK), ("dV", r.dV, r.bdV))):
        _check(f"{tag} {name}", got[:, p * HA:(p + 1) * HA], ref.reshape(B * T, HA), bar.reshape(B * T, HA))
    dres = got[:, 3 * HA:] if nproj == 4 else dxres.owned(tag)
    assert torch.equal(dres.cpu(), dZ.float().reshape(B * T, HA)), f"{tag}: the residual gradient is not the masked dout"


# =================================================================================================== fused attention layer
@pytest.mark.gpu
@pytest.mark.parametrize("B,T,Din,H,a,has_res,scaled,kind", FUSED_CASES)
def test_field_attention_fwd(hip, B, T, Din, H, a, has_res, scaled, kind):
    c = _fused_case(B, T, Din, H, a, has_res, scaled, kind)
    x = _in(c.x.reshape(B, T * Din), T * Din + 5)
    out, W = _Out(B, T * c.HA), _vec(c.W)
    _ok(hip, "rp_field_attention_fwd", x.data_ptr(), T * Din + 5, W.data_ptr(), T, Din, H, a, int(has_res), c.scale, out.ptr, B)
    tag = f"field_attention_fwd[{B},{T},{Din},{H},{a} res={int(has_res)} scaled={int(scaled)} {kind}]"
    _check_relu(tag + " out", out.owned(tag), c.f)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,Din,H,a,has_res,scaled,kind", FUSED_CASES)
def test_field_attention_bwd(hip, B, T, Din, H, a, has_res, scaled, kind):
    """rp_field_attention_bwd alone (it recomputes the forward): dx and dW.  Elements of Z = O + R within their bar of zero
    (at most 0.1 % of a case) carry a zero upstream gradient: see _fused_case"""
    c = _fused_case(B, T, Din, H, a, has_res, scaled, kind)
    f, HA = c.f, c.HA
    r = fused_ref_bwd(f, c.gout.double(), has_res)
    x = _in(c.x.reshape(B, T * Din), T * Din + 5)
    nb = C.c_size_t(0)
    assert hip.lib().rp_field_attention_bwd_workspace_bytes(B, T, Din, H, a, int(has_res), C.byref(nb)) == 0
    ws, W, gout = torch.empty(nb.value, dtype=torch.uint8, device=DEV), _vec(c.W), _vec(c.gout)
    tag = f"field_attention_bwd[{B},{T},{Din},{H},{a} res={int(has_res)} scaled={int(scaled)} {kind}]"
    for want_dx in (True, False):
        dx, dW = (_Out(B, T * Din, T * Din + 3) if want_dx else None), _Out(c.nproj * HA, Din)
        _ok(hip, "rp_field_attention_bwd", x.data_ptr(), T * Din + 5, W.data_ptr(), T, Din, H, a, int(has_res), c.scale,
            gout.data_ptr(), _p(dx), T * Din + 3, dW.ptr, B, ws.data_ptr(), nb.value)
        if want_dx:
            _check(tag + " dx", dx.owned(tag), r.dx.reshape(B, T * Din), r.bdx.reshape(B, T * Din))
        _check(tag + f" dW (dx={int(want_dx)})", dW.owned(tag), r.dW.reshape(c.nproj * HA, Din), r.bdW.reshape(c.nproj * HA, Din))


def test_attention_cases_reach_their_wave_counts():
    """the NW the fused-layer cases are listed for (CPU: a restatement of attn_plan's arithmetic)"""
    assert (_attn_nw(17, 7, 4, 10, True, False), _attn_nw(17, 7, 4, 10, True, True)) == (4, 3)
    assert (_attn_nw(33, 16, 4, 8, True, False), _attn_nw(33, 16, 4, 8, True, True)) == (3, 1)
    assert _attn_nw(2, 4, 1, 2, True, False) == 4 and _attn_nw(2, 4, 1, 2, True, True) == 4


# =================================================================================================== refused before a launch
@pytest.mark.gpu
def test_arguments_refused_before_any_launch(hip):
    """d = 2049, L = 7, T E = 33, a = 17, FM D = 6 and a no-W_res attention call with Din != H a return their documented error
    (RP_ERR_UNSUPPORTED = -3 for a shape no kernel was built for, RP_ERR_ARG = -1 for a malformed one), and B = 0 returns OK:
    all from host code, hip.launch_count() unchanged.  Every pointer is a valid buffer far larger than any of the shapes."""
    buf = torch.zeros(1 << 16, device=DEV)
    p = buf.data_ptr()
    n0 = hip.launch_count()
    UNS, ARG = -3, -1
    refused = [
        (UNS, "rp_crossnet_fwd", (p, 2052, 2049, 2, p, p, p, p, p, 2052, p, p, 4)),
        (UNS, "rp_crossnet_fwd", (p, 8, 5, 7, p, p, p, p, p, 8, p, p, 4)),
        (UNS, "rp_crossnet_bwd_rows", (p, 2052, 2049, 2, p, p, p, p, 2052, p, p, 2052, p, 4)),
        (UNS, "rp_crossnet_bwd_rows", (p, 8, 5, 7, p, p, p, p, 8, p, p, 8, p, 4)),
        (UNS, "rp_mmoe_combine_fwd", (p, 99, 2, 3, 11, p, p, 4)),
        (UNS, "rp_mmoe_combine_bwd", (p, 99, 2, 3, 11, p, p, p, 99, 4)),
        (UNS, "rp_attention_core_fwd", (p, 4 * 17, 4, None, 0, 3, 1, 17, 0.0, p, p, 4)),
        (UNS, "rp_attention_core_bwd", (p, 4 * 17, 4, p, p, p, 3, 1, 17, 0.0, p, 4 * 17, None, 0, 4)),
        (ARG, "rp_fm_pool_fwd", (p, 24, 3, 6, p, p, 4)),
        (ARG, "rp_fm_pool_bwd", (p, 24, 3, 6, p, p, p, 24, 4)),
        (ARG, "rp_field_attention_fwd", (p, 3 * 5, p, 3, 5, 2, 2, 0, 0.0, p, 4)),
        (ARG, "rp_field_attention_bwd", (p, 3 * 5, p, 3, 5, 2, 2, 0, 0.0, p, p, 3 * 5, p, 4, p, 1 << 18)),
    ]
    for code, name, args in refused:
        assert _rc(hip, name, *args) == code, f"{name}{args[1:]}: {hip.lib().rp_last_error().decode()}"
    empty = [
        ("rp_crossnet_fwd", (p, 8, 5, 2, p, p, p, p, p, 8, p, p, 0)),
        ("rp_crossnet_bwd_rows", (p, 8, 5, 2, p, p, p, p, 8, p, p, 8, p, 0)),
        ("rp_mmoe_combine_fwd", (p, 8, 2, 2, 2, p, p, 0)),
        ("rp_mmoe_combine_bwd", (p, 8, 2, 2, 2, p, p, p, 8, 0)),
        ("rp_fm_pool_fwd", (p, 24, 3, 8, p, p, 0)),
        ("rp_fm_pool_bwd", (p, 24, 3, 8, p, p, p, 24, 0)),
        ("rp_batchnorm_apply", (p, 8, p, p, p, p, p, 8, 0, 5)),
        ("rp_batchnorm_apply_bwd", (p, 8, p, p, p, 8, 0, 5)),
        ("rp_dice_gate_fwd", (p, 8, p, 8, p, p, 8, 0, 5)),
        ("rp_dice_gate_bwd", (p, 8, p, 8, p, p, 8, p, p, p, 0, 5)),
        ("rp_accumulate", (p, p, 0)),
        ("rp_attention_core_fwd", (p, 16, 4, None, 0, 3, 2, 2, 0.0, p, p, 0)),
        ("rp_attention_core_bwd", (p, 16, 4, p, p, p, 3, 2, 2, 0.0, p, 16, None, 0, 0)),
        ("rp_field_attention_fwd", (p, 12, p, 3, 4, 2, 2, 0, 0.0, p, 0)),
    ]
    for name, args in empty:
        assert _rc(hip, name, *args) == 0, f"{name} with an empty batch: {hip.lib().rp_last_error().decode()}"
    assert hip.launch_count() == n0
    assert bool((buf == 0).all())


# =================================================================================================== the bars have teeth (CPU)
def _outside(ref, bar, bad):
    """the faulty value leaves the bar somewhere (or is not finite) while the reference rounded to fp32 stays inside"""
    bar = bar if torch.is_tensor(bar) else torch.full_like(ref, bar)
    assert bool(((ref.float().double() - ref).abs() <= bar).all()), "the reference rounded to fp32 is outside its own bar"
    return (not bool(torch.isfinite(bad).all())) or bool(((bad - ref).abs() > bar).any())


def softmax_unshifted_fp32(lg32):
    """fault (d): exp(lg) / sum exp(lg) in fp32, no maximum subtracted"""
    e = torch.exp(lg32)
    return (e / e.sum(-1, keepdim=True)).double()


def test_bars_catch_subtly_wrong_kernels():
    """The issue's eight faults, applied to the float64 references at the committed cases, each leave their bar:
    (a) one term dropped from a CrossNet dot product; (b) the bias of layer l - 1 used in layer l; (c) a one-pass fp32
    variance, which misses bar(var) by at least 4x at BN_OFFSET_CASE; (d) a softmax without the maximum subtracted;
    (e) the attention head split as a [T, H, a] reshape instead of the raw view; (f) dgate without its - sum_e gate dgate
    term; (g) FM's dx with s in place of s - x; (h) the running variance without M / (M - 1).
    On (d): fp32 exp overflows past 88.7, so at logits spread over +-60 an unshifted fp32 softmax is neither non-finite nor
    less accurate than the shifted one (exp(60) = 1.1e26 is an ordinary fp32 number) and no bar derived from fp32 arithmetic
    can tell the two apart there: that is asserted below as what it is.  The fault is caught where it can exist, at the
    "80 above the rest" rows, whose top logit is 92: there it gives inf / inf."""
    missed = []
    for (B, d, ld, L, mis) in CROSS_CASES:
        c = _cross_case(B, d, L)
        q = c.d64
        bs, bx, bl = _cross_bars(c)
        for l in {0, L - 1}:   # the largest term of the first and of the last layer's dot, judged at the s it is summed into
            j = int((q.x0 * q.W[l]).abs().sum(0).argmax()) if l == 0 else int(q.W[l].abs().argmax())
            X, s, lo = ref_cross_fwd(q.x0, q.W, q.Bv, q.wfc, q.bfc, drop=(l, j))
            if not _outside(c.s, bs, s):
                missed.append(f"(a) cross[{B},{d},{L}] term {j} of layer {l}")
        if L >= 2:
            X, s, lo = ref_cross_fwd(q.x0, q.W, q.Bv, q.wfc, q.bfc, stale_bias=True)
            if not _outside(c.xout, bx, X):   # (judged at the rows it is added into)
                missed.append(f"(b) cross[{B},{d},{L}]")
    M, N, ratio = BN_OFFSET_CASE
    c = _bn_case(M, N, ratio)
    miss = (one_pass_var_fp32(c.x) - c.st.var).abs() / c.st.b_var
    assert float(miss[1:].max()) >= 4.0, f"(c) one-pass variance misses bar(var) by only {float(miss[1:].max()):.2f}x"
    for (Mb, Nb) in BN_CASES:   # ... and the two-pass variance in fp32 torch stays inside, there and everywhere
        cb = _bn_case(Mb, Nb)
        x32 = cb.x
        two_pass = ((x32 - x32.mean(0)) ** 2).mean(0).double()
        assert bool(((two_pass - cb.st.var).abs() <= cb.st.b_var).all())
    x32 = c.x
    assert bool(((((x32 - x32.mean(0)) ** 2).mean(0).double() - c.st.var).abs() <= c.st.b_var).all())
    for (B, K, E, T, extra, off, kind) in MMOE_CASES:
        c = _mmoe_case(B, K, E, T, kind)
        bad = softmax_unshifted_fp32(c.lg)
        caught = _outside(c.gate, c.b_gate, bad)
        if kind == "top80" and not caught:
            missed.append(f"(d) mmoe[{B},{K},{E},{T}] {kind}")
        if kind == "pm60":
            assert not caught, "an unshifted fp32 softmax at +-60 was expected to be indistinguishable (see the docstring)"
        g64 = c.gate32.double()
        dze, dlg = ref_mmoe_bwd(c.ze.double(), g64, c.dout.double())
        b_dlg = _mmoe_bwd_bars(c, *_mmoe_bwd_abs(c.ze.double(), g64, c.dout.double()))[1]
        if not _outside(dlg, b_dlg, ref_mmoe_bwd(c.ze.double(), g64, c.dout.double(), drop_dot=True)[1]):
            missed.append(f"(f) mmoe[{B},{K},{E},{T}] {kind}")
    for (B, T, H, a, nproj, scaled, kind) in CORE_CASES:
        c = _core_case(B, T, H, a, nproj, scaled, kind)
        f = c.f
        assert int((~f.sure).sum()) <= EXCLUDED_CAP * f.Z.numel(), f"core{(B, T, H, a, nproj, scaled, kind)}: too many left out"
        if kind in ("top80", "pm60"):
            bad = softmax_unshifted_fp32(f.S.float())
            caught = _outside(f.P, f.bP, bad)
            if kind == "top80" and not caught:
                missed.append(f"(d) core[{B},{T},{H},{a}] {kind}")
        if H > 1 and T > 1:
            g = attn_ref(c.Q.double(), c.K.double(), c.V.double(), c.R.double(), H, a, c.scale, n_exp=T, raw=False)
            if not _outside(f.Z, f.bZ, g.Z):
                missed.append(f"(e) core[{B},{T},{H},{a}] {kind}")
    for (B, T, Din, H, a, has_res, scaled, kind) in FUSED_CASES:
        c = _fused_case(B, T, Din, H, a, has_res, scaled, kind)
        assert c.left_out <= EXCLUDED_CAP * c.f.Z.numel(), f"fused{(B, T, Din, H, a)} {kind}: too many left out"
        if H > 1 and T > 1:
            g = fused_ref(c.x.double(), c.W.double(), T, Din, H, a, has_res, c.scale, raw=False)
            r, rg = fused_ref_bwd(c.f, c.gout.double(), has_res), fused_ref_bwd(g, c.gout.double(), has_res)
            if not (_outside(c.f.Z, c.f.bZ, g.Z) and _outside(r.dx, r.bdx, rg.dx) and _outside(r.dW, r.bdW, rg.dW)):
                missed.append(f"(e) fused[{B},{T},{Din},{H},{a}]")
    for (B, F, D) in FM_CASES:
        c = _fm_case(B, F, D)
        x, gs, gb = c.x.double(), c.g_sum.double(), c.g_bi.double()
        if not _outside(ref_fm_bwd(x, gs, gb), gamma(U, F + 2) * _fm_bwd_abs(x, gs, gb), ref_fm_bwd(x, gs, gb, keep_x=False)):
            missed.append(f"(g) fm[{B},{F},{D}]")
    for (M, N) in BN_CASES:
        if M > 1:
            c = _bn_case(M, N)
            rv0 = torch.ones(N, dtype=torch.float64)
            _, rvr, _, b_rv, _ = ref_bn_running(c.mean32.double(), c.var32.double(), rv0, rv0, 0, 0.1, M)
            if not _outside(rvr, b_rv, ref_bn_running(c.mean32.double(), c.var32.double(), rv0, rv0, 0, 0.1, M, unbias=False)[1]):
                missed.append(f"(h) bn[{M},{N}]")
    assert missed == [], "the bars do not notice:\n" + "\n".join(missed)
