"""rp_pair_loss_* (csrc/pair_loss.hip) through Fh.pair_loss, alone: both modes, logits and probabilities, the batch sizes around
one workgroup (255 / 256 / 257), one sample, several workgroups (5000) and the grid-stride loop (above 1024 workgroups of 256),
against a float64 restatement written here; the tie of AITM's constraint; saturated logits against torch's own fp32
composition; bit-identical repeats.  The bar is the kernel tests' usual one: 1e-4 * max(1e-2, max|ref|)."""
import functools

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINK = 1e-5
ESSM, AITM = 0, 1
COEF = {ESSM: 0.5, AITM: 0.6}
SEED_GRAD = 1.7  # the loss's incoming gradient: not 1, so that a kernel ignoring it shows
SIZES = [1, 255, 256, 257, 5000, 1024 * 256 + 300]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


def _close(got, ref, what):
    tol = 1e-4 * max(1e-2, float(ref.abs().max()))
    err = float((got.detach().cpu().double().reshape(-1) - ref.reshape(-1)).abs().max())
    print(f"{what}: error {err:.3g}, bar {tol:.3g}")
    assert err <= tol, f"{what}: {err} > {tol}"


def restatement(z1, z2, y1, y2, mode, coef, apply_sigmoid, dtype=torch.float64):
    """(p1, p2, loss, dz1, dz2) of the formulas in include/rec_pangu_hip.h, by autograd in `dtype`, the loss's gradient SEED_GRAD"""
    z1, z2 = z1.to(dtype).requires_grad_(True), z2.to(dtype).requires_grad_(True)
    y1, y2 = y1.to(dtype), y2.to(dtype)
    p1, p2 = (torch.sigmoid(z1), torch.sigmoid(z2)) if apply_sigmoid else (z1, z2)

    def bce(p, y):
        return -(y * torch.log(p).clamp(min=-100) + (1 - y) * torch.log1p(-p).clamp(min=-100)).mean()

    if mode == ESSM:
        loss = bce(p1 * p2, y2) + coef * bce(p1, y1)
    else:
        loss = bce(p1, y1) + bce(p2, y2) + coef * torch.maximum(p2 - p1, torch.zeros_like(p1)).sum()
    (loss * SEED_GRAD).backward()
    return p1.detach(), p2.detach(), loss.detach(), z1.grad, z2.grad


@functools.lru_cache(maxsize=None)
def _case(B, mode, apply_sigmoid):
    """inputs (fp32, on the CPU) and their float64 reference: computed once, shared, left unchanged"""
    g = torch.Generator().manual_seed(1000 * mode + 10 * B % 997 + int(apply_sigmoid))
    z1, z2 = (torch.rand(B, generator=g) * 16 - 8 for _ in range(2))
    y1, y2 = (torch.rand(B, generator=g) < 0.4).float(), (torch.rand(B, generator=g) < 0.2).float()
    if mode == AITM:  # no row on the kink of max(p2 - p1, 0): the comparison is total
        for _ in range(4):
            near = (torch.sigmoid(z2.double()) - torch.sigmoid(z1.double())).abs() < KINK
            z2 = torch.where(near, z2 - 0.5 * torch.sign(z2), z2)  # (towards 0: stays in [-8, 8], moves p2 by >= 1.6e-4)
        assert not bool(((torch.sigmoid(z2.double()) - torch.sigmoid(z1.double())).abs() < KINK).any())
    if not apply_sigmoid:  # the kernel's inputs are then the probabilities, as fp32 holds them
        z1, z2 = torch.sigmoid(z1), torch.sigmoid(z2)
        if mode == AITM:
            z2 = torch.where((z2.double() - z1.double()).abs() < KINK, z2 + 1e-4, z2)
            assert not bool(((z2.double() - z1.double()).abs() < KINK).any()) and float(z2.max()) < 1
    return (z1, z2, y1, y2), restatement(z1, z2, y1, y2, mode, COEF[mode], apply_sigmoid)


def _run(inputs, mode, coef, apply_sigmoid):
    from rec_pangu_amd import functional as Fh
    z1, z2, y1, y2 = (t.to(DEV) for t in inputs)
    z1.requires_grad_(True)
    z2.requires_grad_(True)
    p1, p2, loss = Fh.pair_loss(z1, z2, y1, y2, mode, coef, apply_sigmoid)
    (loss * SEED_GRAD).backward()
    return p1, p2, loss, z1.grad, z2.grad


@pytest.mark.parametrize("apply_sigmoid", [True, False], ids=["logits", "probs"])
@pytest.mark.parametrize("mode", [ESSM, AITM], ids=["essm", "aitm"])
@pytest.mark.parametrize("B", SIZES)
def test_against_float64(B, mode, apply_sigmoid):
    from rec_pangu_amd import hip
    inputs, ref = _case(B, mode, apply_sigmoid)
    n0 = hip.launch_count()
    got = _run(inputs, mode, COEF[mode], apply_sigmoid)
    assert hip.launch_count() >= n0 + 3  # forward, finish, backward
    assert got[0].shape == got[1].shape == (B,) and got[2].shape == ()
    for name, a, b in zip(("p1", "p2", "loss", "dz1", "dz2"), got, ref):
        _close(a, b, f"B={B} mode={mode} sigmoid={apply_sigmoid} {name}")
    again = _run(inputs, mode, COEF[mode], apply_sigmoid)
    for name, a, b in zip(("p1", "p2", "loss", "dz1", "dz2"), got, again):
        assert torch.equal(a, b), f"{name} differs between two runs on the same input"


def test_shapes_follow_the_inputs():
    """ESSM hands [B, 1] logits in and gets [B, 1] predictions and gradients back"""
    from rec_pangu_amd import functional as Fh
    inputs, ref = _case(257, ESSM, True)
    z1, z2, y1, y2 = (t.to(DEV) for t in inputs)
    z1, z2 = z1.view(-1, 1).requires_grad_(True), z2.view(-1, 1).requires_grad_(True)
    p1, p2, loss = Fh.pair_loss(z1, z2, y1, y2, ESSM, COEF[ESSM])
    (loss * SEED_GRAD).backward()
    assert p1.shape == p2.shape == z1.grad.shape == z2.grad.shape == (257, 1)
    for name, a, b in zip(("p1", "p2", "loss", "dz1", "dz2"), (p1, p2, loss, z1.grad, z2.grad), ref):
        _close(a, b, name)


def test_the_tie_of_the_constraint_splits_the_gradient():
    """p2 == p1 on purpose (probabilities in, no sigmoid): ATen's maximum backward gives each argument half — dp2 = bce' + c / 2,
    dp1 = bce' - c / 2 — and so does torch's own fp32 composition on the CPU"""
    B, c = 300, COEF[AITM]
    g = torch.Generator().manual_seed(5)
    p = torch.rand(B, generator=g) * 0.98 + 0.01
    y1, y2 = (torch.rand(B, generator=g) < 0.4).float(), (torch.rand(B, generator=g) < 0.2).float()
    got = _run((p, p.clone(), y1, y2), AITM, c, False)
    pd = p.double()
    dbce = lambda y: (pd - y.double()) / ((1 - pd) * pd).clamp(min=1e-12) / B  # noqa: E731
    _close(got[3], SEED_GRAD * (dbce(y1) - c * 0.5), "dp1 at the tie")
    _close(got[4], SEED_GRAD * (dbce(y2) + c * 0.5), "dp2 at the tie")
    cpu = restatement(p, p.clone(), y1, y2, AITM, c, False, dtype=torch.float32)
    _close(got[2], cpu[2].double(), "loss at the tie")
    _close(got[3], cpu[3].double(), "dp1 against torch's fp32 maximum backward")
    _close(got[4], cpu[4].double(), "dp2 against torch's fp32 maximum backward")


@pytest.mark.parametrize("mode", [ESSM, AITM], ids=["essm", "aitm"])
def test_saturated_logits_against_torch_fp32(mode):
    """z in {+-12, +-30, +-90} (away from the fp32 rounding edge of the sigmoid), every pair of them under every pair of labels:
    torch's own fp32 composition of the same formulas with autograd on the CPU.  Both finite; the loss within rtol 1e-5, the
    gradients within the bar."""
    vals = torch.tensor([12.0, -12.0, 30.0, -30.0, 90.0, -90.0])
    z1, z2, y1, y2 = (t.reshape(-1) for t in torch.meshgrid(vals, vals, torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0]),
                                                           indexing="ij"))
    z1, z2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    p1, p2 = torch.sigmoid(z1), torch.sigmoid(z2)
    bce = torch.nn.functional.binary_cross_entropy
    if mode == ESSM:
        loss = bce(p1 * p2, y2) + COEF[mode] * bce(p1, y1)
    else:
        loss = bce(p1, y1) + bce(p2, y2) + COEF[mode] * torch.sum(torch.maximum(p2 - p1, torch.zeros_like(y1)))
    (loss * SEED_GRAD).backward()
    got = _run((z1.detach(), z2.detach(), y1, y2), mode, COEF[mode], True)
    for t in (loss, z1.grad, z2.grad) + tuple(got):
        assert bool(torch.isfinite(t).all())
    print(f"mode {mode}: loss {float(got[2])} against {float(loss)}")
    torch.testing.assert_close(got[2].cpu(), loss.detach(), rtol=1e-5, atol=0)
    _close(got[0], p1.detach().double(), "p1")
    _close(got[1], p2.detach().double(), "p2")
    _close(got[3], z1.grad.double(), "dz1")
    _close(got[4], z2.grad.double(), "dz2")
