"""rp_attention_wide_* (csrc/attn_wide.hip) alone, against float64 autograd over the formulas of include/rec_pangu_hip.h:
T in {2, 3, 4}; a = 20 (below a wave), 64 / 68 (exactly one pass of the lanes with dwordx4 columns' worth of scalar lanes / a
partial second one), 400 (AITM), 1024, and 67 (not a multiple of 4: the scalar-load kernels); B = 1, 5, 257 (65 workgroups) and
16389 (past the grid's 4096 workgroups of 4 samples: the sample-stride loop); both outputs (per token / summed over the tokens);
scale 0 and sqrt(a); xres as a row-strided view, once with a stride that is no multiple of 4 floats (scalar loads at a % 4 == 0).
The grid pairs the edges instead of taking their product.  The bar is the kernel tests' usual one: 1e-4 * max(1e-2, max|ref|).
Then the autograd node Fh.attention_wide (projection GEMM + core + the residual's gradient added by a library launch)."""
import functools
import math

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINK = 1e-5

# (T, a, B, sum_tokens, scaled, extra columns of the xres view)
CASES = [
    (2, 400, 257, True, False, 0),    # AITM's default
    (2, 400, 5, False, True, 16),
    (3, 20, 5, True, True, 0),
    (4, 20, 257, False, True, 4),
    (2, 20, 16389, True, False, 0),   # more samples than waves in the grid
    (4, 64, 257, False, False, 0),
    (3, 64, 1, True, True, 0),
    (2, 68, 1, True, False, 8),
    (3, 68, 257, False, True, 0),
    (2, 68, 5, False, False, 3),      # a % 4 == 0 but the residual's rows are not 16-byte aligned: scalar loads
    (3, 67, 5, True, True, 0),        # a % 4 != 0: scalar loads
    (4, 67, 257, False, False, 2),
    (3, 400, 5, True, False, 0),
    (4, 400, 1, False, True, 0),
    (3, 1024, 5, False, True, 0),
    (4, 1024, 1, True, False, 32),
    (2, 1024, 257, True, True, 0),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


def _close(got, ref, what):
    tol = 1e-4 * max(1e-2, float(ref.abs().max()))
    err = float((got.detach().cpu().double() - ref).abs().max())
    print(f"{what}: error {err:.3g}, bar {tol:.3g}")
    assert err <= tol, f"{what}: {err} > {tol}"


def pre_relu(qkv, xres, T, a, scale):
    """O + xres [B, T, a] of the formulas, in the dtype of the operands"""
    B = qkv.shape[0] // T
    q, k, v = (qkv[:, i * a:(i + 1) * a].reshape(B, T, a) for i in range(3))
    s = torch.einsum("bta,bsa->bts", q, k)
    if scale:
        s = s / scale
    return torch.einsum("bts,bsa->bta", torch.softmax(s, dim=2), v) + xres.reshape(B, T, a)


@functools.lru_cache(maxsize=None)
def _case(case):
    """operands (fp32, on the CPU; xres as a view with row stride a + extra), the cotangent and the float64 results: computed
    once, shared, left unchanged"""
    T, a, B, sum_tokens, scaled, extra = case
    g = torch.Generator().manual_seed(hash(case) % (1 << 31))
    qkv = torch.randn(B * T, 3 * a, generator=g)
    qkv[:, :2 * a] *= a ** -0.25  # scores of order 1
    xbuf = torch.randn(B * T, a + extra, generator=g)
    scale = math.sqrt(a) if scaled else 0.0
    # xres is an operand of its own here: push it away from the ReLU's kink where float64 puts O + xres within 1e-5 of it
    pre = pre_relu(qkv.double(), xbuf[:, :a].double(), T, a, scale).reshape(B * T, a)
    near = pre.abs() < KINK
    xbuf[:, :a] += torch.where(near, torch.where(pre >= 0, 2e-5, -2e-5), 0.0).float()
    xres = xbuf[:, :a]
    cot = torch.randn((B, a) if sum_tokens else (B, T, a), generator=g)
    q64, x64 = qkv.double().requires_grad_(True), xres.double().requires_grad_(True)
    pre = pre_relu(q64, x64, T, a, scale)
    assert float(pre.detach().abs().min()) >= KINK, "an element sits on the ReLU's kink"
    y = torch.relu(pre)
    out = y.sum(dim=1) if sum_tokens else y
    out.backward(cot.double())
    return dict(qkv=qkv, xres=xres, cot=cot, scale=scale, out=out.detach(), dqkv=q64.grad, dxres=x64.grad)


def _on_device(c):
    qkv = c["qkv"].to(DEV)
    xbuf = torch.empty((c["xres"].shape[0], c["xres"].stride(0)), device=DEV)
    xres = xbuf[:, :c["xres"].shape[1]]
    xres.copy_(c["xres"])
    return qkv, xres, c["cot"].to(DEV).contiguous()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T{}-a{}-B{}-{}-{}-ld+{}".format(c[0], c[1], c[2], "sum" if c[3] else "tokens",
                                                                                     "scaled" if c[4] else "unscaled", c[5]))
def test_forward_and_backward_against_float64(case):
    from rec_pangu_amd import hip
    T, a, B, sum_tokens, _, extra = case
    assert hip.attention_wide_fits(T, 1, a)
    c = _case(case)
    qkv, xres, cot = _on_device(c)
    assert xres.stride(0) == a + extra
    n0 = hip.launch_count()
    out = hip.attention_wide_fwd(qkv, xres, T, a, c["scale"], sum_tokens)
    dqkv, dxres = hip.attention_wide_bwd(qkv, xres, cot, T, a, c["scale"], sum_tokens)
    assert hip.launch_count() == n0 + 2
    assert out.shape == ((B, a) if sum_tokens else (B * T, a)) and dqkv.shape == (B * T, 3 * a) and dxres.shape == (B * T, a)
    _close(out.view(c["out"].shape), c["out"], "out")
    _close(dqkv, c["dqkv"], "dqkv")
    _close(dqkv[:, :a], c["dqkv"][:, :a], "dq")
    _close(dqkv[:, a:2 * a], c["dqkv"][:, a:2 * a], "dk")
    _close(dqkv[:, 2 * a:], c["dqkv"][:, 2 * a:], "dv")
    _close(dxres, c["dxres"], "dxres")
    out2 = hip.attention_wide_fwd(qkv, xres, T, a, c["scale"], sum_tokens)
    dqkv2, dxres2 = hip.attention_wide_bwd(qkv, xres, cot, T, a, c["scale"], sum_tokens)
    assert torch.equal(out, out2) and torch.equal(dqkv, dqkv2) and torch.equal(dxres, dxres2), "two runs differ"


@pytest.mark.parametrize("T,a,B,sum_tokens", [(2, 400, 33, True), (3, 68, 7, False)])
def test_the_autograd_node_against_float64(T, a, B, sum_tokens):
    """Fh.attention_wide: X [B, T, a] and the stacked weights [3a, a] -> the layer, with exact fp32 products in the projection
    GEMM; the gradient of X holds both of its uses (projection and residual)"""
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    g = torch.Generator().manual_seed(7 * T + a)
    X = torch.randn(B, T, a, generator=g)
    W = torch.randn(3 * a, a, generator=g) * a ** -0.5
    W[:2 * a] *= a ** -0.25
    cot = torch.randn((B, a) if sum_tokens else (B, T, a), generator=g)
    pre = pre_relu((X.double().reshape(B * T, a) @ W.double().t()), X.double().reshape(B * T, a), T, a, 0.0)
    X = X + torch.where(pre.abs() < 1e-4, 1e-3, 0.0).float()  # (X is the GEMM's input too: a coarser push, then the check)
    x64, w64 = X.double().requires_grad_(True), W.double().requires_grad_(True)
    pre = pre_relu(x64.reshape(B * T, a) @ w64.t(), x64.reshape(B * T, a), T, a, 0.0)
    assert float(pre.detach().abs().min()) >= KINK
    ref = torch.relu(pre).sum(dim=1) if sum_tokens else torch.relu(pre)
    ref.backward(cot.double())
    prev = hip.get_matmul_precision()
    hip.set_matmul_precision("fp32")
    try:
        xd, wd = X.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
        n_paths = hip.torch_path_count()
        out = Fh.attention_wide(xd, wd, T, a, 0.0, sum_tokens)
        out.backward(cot.to(DEV))
        assert hip.torch_path_count() == n_paths
    finally:
        hip.set_matmul_precision(prev)
    assert out.shape == ref.shape
    _close(out, ref.detach(), "out")
    _close(xd.grad, x64.grad, "dX")
    _close(wd.grad, w64.grad, "dW")
