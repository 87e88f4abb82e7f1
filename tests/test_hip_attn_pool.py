"""The additive-attention pooling kernel alone on the GPU (csrc/attn_pool.hip): out, A, dX, dc, dW1 and dW2 against float64
autograd of tests/test_attn_pool_host.py's statement (the project's per-tensor bar 1e-4 max(1e-2, max |ref|)), bit-identical
runs, launch and torch-path counts, exact zeros at invalid positions, shapes just outside the declared geometry on the
counted torch path.

Shapes: L = 1 (64 samples per workgroup), 5 (12, a padded row tile), 20 (3), 50 (one, a padded tile); B = 1, 7 (a partial
last workgroup) and 300; D = 12 (a padded column tile), 64, 128 (the largest tile).  (Dh, K) = (D, 1), (4 D, 4), (40, 3): a
partial last chunk, and (4 D, 8) = (512, 8) at D = 128, the geometry's corner.  Modes: STAMP's form (sigmoid, mask, with
the per-sample bias) and ComirecSA's (tanh, softmax, none).  The first rows of every batch have lengths 1, L, 3, 2 and 0, row
5 has a hole in valid.  The float64 reference of every case is computed once per module."""
import functools
import warnings

import pytest
import torch

from conftest import require_gpu
from test_attn_pool_host import MODES, pool_f64, pool_grads, pool_inputs, within

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 64), (7, 1, 12), (7, 5, 12), (7, 5, 64), (300, 5, 12), (7, 20, 64), (300, 20, 64), (1, 20, 128), (7, 50, 12),
          (7, 50, 128), (1, 50, 64)]
NAMES = ("out", "A", "dx", "dc", "dw1", "dw2")


def hidden_shapes(Dx):
    return [(Dx, 1), (4 * Dx, 4), (40, 3)] + ([(4 * Dx, 8)] if Dx == 128 else [])


CASES = [(B, Lx, Dx, Dh, K, mode) for B, Lx, Dx in SHAPES for Dh, K in hidden_shapes(Dx) for mode in MODES]


@functools.lru_cache(maxsize=None)
def pool_case(B, Lx, Dx, Dh, K, mode, target_score=None):
    """inputs and float64 results: computed once, shared, left unchanged.  target_score: W2 rescaled so max |S| is that"""
    act, norm, with_c = MODES[mode]
    gen = torch.Generator().manual_seed(B * 1000 + Lx * 10 + Dx + Dh + K)
    x, w1, w2, valid, c, g = pool_inputs(B, Lx, Dx, Dh, K, with_c, gen)
    if target_score is not None:
        s = torch.tanh(x @ w1) @ w2
        w2 = w2 * (target_score / float(s.abs().max()))
    ref = pool_grads(pool_f64, x, w1, w2, valid, c, g, act, norm, torch.float64)
    return (x, w1, w2, valid, c, g), ref


def run_device(inputs, mode):
    from rec_pangu_amd import functional as Fh
    act, norm, _ = MODES[mode]
    x, w1, w2, valid, c, g = inputs
    xs, a1, a2 = (t.to(torch.float32).to(DEV).requires_grad_(True) for t in (x, w1, w2))
    cs = None if c is None else c.to(torch.float32).to(DEV).requires_grad_(True)
    out = Fh.attention_pool(xs, a1, a2, valid.to(DEV), bias=cs, act=act, norm=norm)
    A = out.grad_fn.saved_tensors[4]  # (the node keeps x, valid, w1, w2, A: the weights are what it saved)
    (out * g.to(torch.float32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return [None if t is None else t.detach().cpu() for t in (out, A, xs.grad, None if cs is None else cs.grad, a1.grad, a2.grad)]


@pytest.mark.parametrize("B,Lx,Dx,Dh,K,mode", CASES)
def test_forward_and_backward_against_float64(B, Lx, Dx, Dh, K, mode):
    require_gpu()
    from rec_pangu_amd import hip
    inputs, ref = pool_case(B, Lx, Dx, Dh, K, mode)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = run_device(inputs, mode)
    assert hip.launch_count() >= n0 + 2 + 3 + 1 and hip.torch_path_count() == t0
    worst = 0.0
    for name, a, b in zip(NAMES, got, ref):
        if b is None:
            assert a is None
            continue
        worst = max(worst, within(a, b, f"{name} at {(B, Lx, Dx, Dh, K, mode)}"))
    print(f"worst tensor: {worst:.3g} of its bar")
    valid = inputs[3]
    A, dx = got[1], got[2]
    masked = valid == 0
    if MODES[mode][1] == "softmax" and B > 4:
        torch.testing.assert_close(A[4], torch.full_like(A[4], 1.0 / Lx))  # no valid position: uniform
        masked[4] = False
    if masked.any():
        assert float(A[masked].abs().max()) == 0.0        # weight exactly 0 at invalid positions
        assert float(dx[masked].abs().max()) == 0.0       # no weight and no dPre: the row's gradient is exactly 0
    if MODES[mode][1] == "mask" and B > 4:
        assert float(got[0][4].abs().max()) == 0.0


def test_max_subtraction_matters_at_scores_near_twenty():
    require_gpu()
    B, Lx, Dx, Dh, K = 7, 20, 64, 256, 4
    inputs, ref = pool_case(B, Lx, Dx, Dh, K, "sa", 20.0)
    x, w1, w2 = inputs[:3]
    smax = float((torch.tanh(x @ w1) @ w2).abs().max())
    assert 15.0 < smax < 32.0
    got = run_device(inputs, "sa")
    for name, a, b in zip(NAMES, got, ref):
        if b is not None:
            within(a, b, f"{name} at max|S| = {smax:.3g}")


@pytest.mark.parametrize("B,Lx,Dx,Dh,K,mode", [(300, 20, 64, 256, 4, "sa"), (300, 5, 12, 12, 1, "stamp"), (7, 50, 128, 512, 8, "sa"),
                                               (7, 50, 128, 40, 3, "stamp")])
def test_two_runs_give_equal_bits(B, Lx, Dx, Dh, K, mode):
    require_gpu()
    inputs, _ = pool_case(B, Lx, Dx, Dh, K, mode)
    a, b = run_device(inputs, mode), run_device(inputs, mode)
    for name, u, v in zip(NAMES, a, b):
        assert (u is None and v is None) or torch.equal(u, v), name


@pytest.mark.parametrize("Lx,Dx,K", [(65, 12, 2), (5, 132, 2), (5, 12, 9)])
@pytest.mark.parametrize("mode", list(MODES))
def test_outside_the_geometry_takes_the_counted_torch_path(Lx, Dx, K, mode):
    require_gpu()
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    act, norm, with_c = MODES[mode]
    assert not hip.attn_pool_fits(Lx, Dx, 16, K)
    gen = torch.Generator().manual_seed(Lx + Dx + K)
    x, w1, w2, valid, c, g = pool_inputs(6, Lx, Dx, 16, K, with_c, gen)
    f = lambda t, d: None if t is None else t.to(torch.float32).to(d)  # noqa: E731
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = Fh.attention_pool(f(x, DEV), f(w1, DEV), f(w2, DEV), valid.to(DEV), bias=f(c, DEV), act=act, norm=norm)
    assert hip.launch_count() == n0 and hip.torch_path_count() == t0 + 1
    want = Fh.attention_pool_reference(f(x, "cpu"), f(w1, "cpu"), f(w2, "cpu"), valid, f(c, "cpu"), act, norm)
    within(got, want, "the counted torch path against the CPU path")
