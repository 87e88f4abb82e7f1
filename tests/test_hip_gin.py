"""rp_gin_fwd / rp_gin_bwd alone against a float64 restatement of the factorised layer (the four einsums of
include/rec_pangu_hip.h and their autograd), at the edges of the shape range.

A workgroup owns a tile of S = 256 / D samples (32, 12, 8, 4 for D = 8, 20, 32, 64), fewer where that many do not fit in LDS:
in the backward at F = P = 39, 10 at D = 20 and 3 at D = 64 (the case 39, 39, 1, 64, 37 runs that LDS-limited tile, a quarter
of the threads idle).  It walks the tiles with a stride of its grid: at most 512 workgroups forward, 256
backward.  B = 5000 is therefore 157 / 417 (500) / 625 / 1250 tiles: every backward launch at D >= 20 and every forward launch
at D >= 32 walks more than one tile per workgroup, which is where the per-workgroup partial of dalpha / dM is added to
instead of written.  5000 is a multiple of 8, 4 and 10, so the last tile of those walks is full; B = 5003 (one case more than
the grid of B = 1, 37, 5000) ends a multi-tile walk with a partial tile, as 37 does for a single one.  The kernels are fp32
FMA on the vector ALU: no matrix-core mode applies."""
import functools

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (F, P, O, D, B): every value of each dimension, and P == F as well as P < F at every D
CASES = [
    (5, 5, 3, 8, 37),
    (26, 26, 4, 32, 5000),
    (39, 39, 1, 64, 37),
    (39, 39, 3, 20, 5000),
    (26, 4, 4, 8, 5000),
    (26, 4, 3, 20, 37),
    (26, 4, 4, 32, 1),
    (7, 1, 1, 64, 5000),
    (1, 1, 3, 32, 37),
    (7, 1, 4, 8, 1),
    (26, 26, 4, 20, 37),
    (5, 5, 1, 64, 1),
    (26, 4, 4, 32, 5003),
]
IDS = ["F{}P{}O{}D{}B{}".format(*c) for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


def _forward64(x0, bi, W, alpha, h, F, P, O, D):
    B = x0.shape[0]
    M = W * h.view(O, 1, D)
    T = torch.einsum("ohd,bpd->boph", M, bi.view(B, P, D))
    U = torch.einsum("pfo,bfh->boph", alpha.view(P, F, O), x0.view(B, F, D))
    return (T * U).sum(dim=2).reshape(B, O * D)


@functools.lru_cache(maxsize=None)
def _case(F, P, O, D, B):
    """fp32 inputs (0.5 randn activations, Kaiming-normal parameters) and the float64 result and gradients, computed once"""
    gen = torch.Generator().manual_seed(1000 * F + 100 * P + 10 * O + D + B)
    x0 = 0.5 * torch.randn(B, F * D, generator=gen)
    bi = 0.5 * torch.randn(B, P * D, generator=gen)
    cot = torch.randn(B, O * D, generator=gen)
    W, alpha, h = torch.empty(O, D, D), torch.empty(P * F, O), torch.empty(O, D, 1)
    for p in (W, alpha, h):
        torch.nn.init.kaiming_normal_(p, generator=gen)
    leaves = [t.double().requires_grad_(True) for t in (x0, bi, W, alpha, h)]
    out = _forward64(*leaves, F, P, O, D)
    grads = torch.autograd.grad(out, leaves, cot.double())
    return dict(x0=x0, bi=bi, cot=cot, W=W, alpha=alpha, h=h, out=out.detach(), grads=[g.detach() for g in grads])


def _block(t, aligned):
    """t [B, n] as a column block of a wider device buffer: row stride a multiple of 4 from an aligned base, or an odd row
    stride starting one float in"""
    B, n = t.shape
    buf = torch.full((B, n + (16 if aligned else 13)), 7.0, device=DEV)
    view = buf[:, :n] if aligned else buf[:, 1:1 + n]
    view.copy_(t)
    assert view.stride(0) % 4 == (0 if aligned else 1)
    return view


def _grad_close(got, ref, what):
    tol = 1e-4 * max(1e-2, float(ref.abs().max()))
    err = float((got.double().cpu() - ref.reshape(got.shape)).abs().max())
    print(f"{what}: {err:.3g} (bar {tol:.3g})")
    assert err <= tol, f"{what}: {err} > {tol}"


@pytest.mark.parametrize("aligned", [False, True], ids=["odd_stride", "aligned"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_vs_float64(case, aligned):
    from rec_pangu_amd import hip
    F, P, O, D, B = case
    assert hip.gin_fits(F, P, O, D)
    c = _case(*case)
    x0, bi = _block(c["x0"], aligned), _block(c["bi"], aligned)
    W, alpha, h = c["W"].to(DEV), c["alpha"].to(DEV), c["h"].to(DEV)
    n0 = hip.launch_count()
    out = hip.gin_fwd(x0, bi, W, alpha, h, F)
    assert hip.launch_count() == n0 + 1 and out.shape == (B, O * D)
    print(f"out: {float((out.double().cpu() - c['out']).abs().max()):.3g}, max|ref| {float(c['out'].abs().max()):.3g}")
    torch.testing.assert_close(out.double().cpu(), c["out"], rtol=1e-4, atol=1e-5)
    dxbuf = torch.full((B, F * D + (16 if aligned else 13)), 3.0, device=DEV)
    dx0 = dxbuf[:, :F * D] if aligned else dxbuf[:, 1:1 + F * D]
    dbi, dW, dalpha, dh = hip.gin_bwd(_block(c["cot"], aligned), x0, bi, W, alpha, h, F, dx0, accumulate=False)
    assert hip.launch_count() == n0 + 3  # the tile walk and the finishing launch
    for got, ref, what in zip((dx0, dbi, dW, dalpha, dh), c["grads"], ("dx0", "dbi", "dW", "dalpha", "dh")):
        _grad_close(got, ref, what)
    outside = torch.ones(dxbuf.shape[1], dtype=torch.bool)
    outside[(0 if aligned else 1):(0 if aligned else 1) + F * D] = False
    assert torch.all(dxbuf[:, outside.to(DEV)] == 3.0), "dx0's neighbours in the wider buffer were written"


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[12]], ids=[IDS[0], IDS[4], IDS[12]])
def test_dx0_accumulates_onto_a_prefilled_buffer(case):
    from rec_pangu_amd import hip
    F, P, O, D, B = case
    c = _case(*case)
    dev = {k: c[k].to(DEV) for k in ("x0", "bi", "cot", "W", "alpha", "h")}
    pre = torch.randn(B, F * D, generator=torch.Generator().manual_seed(9))
    dx0 = pre.to(DEV)
    hip.gin_bwd(dev["cot"], dev["x0"], dev["bi"], dev["W"], dev["alpha"], dev["h"], F, dx0, accumulate=True)
    ref = pre.double() + c["grads"][0]
    tol = 1e-4 * max(1e-2, float(c["grads"][0].abs().max())) + 1e-6 * float(pre.abs().max())  # (+ the rounding of the sum)
    err = float((dx0.double().cpu() - ref).abs().max())
    assert err <= tol, f"accumulated dx0: {err} > {tol}"


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2], CASES[8]], ids=[IDS[0], IDS[1], IDS[2], IDS[8]])
def test_bi_aliasing_x0_sums_both_roles(case):
    """layer 0: B_i is B_0 itself — one tensor in both roles, its gradient the sum of the two"""
    from rec_pangu_amd import hip
    F, P, O, D, B = case
    assert F == P
    c = _case(*case)
    x64 = c["x0"].double().requires_grad_(True)
    params64 = [c[k].double().requires_grad_(True) for k in ("W", "alpha", "h")]
    out64 = _forward64(x64, x64, *params64, F, P, O, D)
    refs = torch.autograd.grad(out64, [x64] + params64, c["cot"].double())
    x0 = _block(c["x0"], False)
    W, alpha, h = c["W"].to(DEV), c["alpha"].to(DEV), c["h"].to(DEV)
    out = hip.gin_fwd(x0, x0, W, alpha, h, F)
    torch.testing.assert_close(out.double().cpu(), out64.detach(), rtol=1e-4, atol=1e-5)
    dx0 = torch.empty(B, F * D, device=DEV)
    dbi, dW, dalpha, dh = hip.gin_bwd(c["cot"].to(DEV), x0, x0, W, alpha, h, F, dx0, accumulate=False, bi_is_x0=True)
    assert dbi is None
    for got, ref, what in zip((dx0, dW, dalpha, dh), refs, ("dx0 (both roles)", "dW", "dalpha", "dh")):
        _grad_close(got, ref, what)


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[7]], ids=[IDS[1], IDS[3], IDS[7]])
def test_backward_is_bit_identical_from_run_to_run(case):
    from rec_pangu_amd import hip
    F, P, O, D, B = case
    c = _case(*case)
    dev = {k: c[k].to(DEV) for k in ("x0", "bi", "cot", "W", "alpha", "h")}
    runs = []
    for _ in range(2):
        dx0 = torch.empty(B, F * D, device=DEV)
        rest = hip.gin_bwd(dev["cot"], dev["x0"], dev["bi"], dev["W"], dev["alpha"], dev["h"], F, dx0, accumulate=False)
        runs.append((dx0,) + tuple(rest))
    for a, b, what in zip(runs[0], runs[1], ("dx0", "dbi", "dW", "dalpha", "dh")):
        assert torch.equal(a, b), what


def test_shapes_outside_the_range_are_refused():
    from rec_pangu_amd import hip
    x0 = torch.zeros(4, 3 * 10, device=DEV)
    W, alpha, h = torch.zeros(2, 10, 10, device=DEV), torch.zeros(9, 2, device=DEV), torch.zeros(2, 10, 1, device=DEV)
    assert not hip.gin_fits(3, 3, 2, 10)
    with pytest.raises(RuntimeError, match="rp_gin_fits"):
        hip.gin_fwd(x0, x0, W, alpha, h, 3)
