"""The logarithmic-net kernels (csrc/lognet.hip: rp_lognet_fwd / rp_lognet_bwd) alone against a float64 restatement of
ranking/afn.py:93-102, with batch statistics and with running statistics, at the edges of their work split, and the two-logit
head rp_pair_fc_*.

Tolerance: the project's bar 1e-4 max(1e-2, max |ref|) per compared tensor.  torch's own fp32 formulation of the block differs
from float64 by at most 3.3e-6 of the maximum (output and every gradient, both modes, shapes up to (1030, 39, 64, 8)) when both
clamp at float32(1e-5) and no input sits within 1e-7 of it, so the bar leaves about 30x room.  With batch statistics dbeta1 has
no real value (a shift of y_f scales c_l by a constant that BN2's batch statistics remove: the float64 value is ~1e-17 of the
other gradients): it is judged against the bar of dgamma1.  dx scales with 1 / |e|, so it is compared a second time as
dx max(|e|, 1e-5), where one tiny unclamped element cannot hide the others' errors.

Shapes (B, F, D, L): one sample of one field; two fields; odd sizes inside one workgroup; the Criteo field count at more than
one round per thread; a width that is no power of two (rows of 40 floats: a wave spans several samples); and F = 39, D = 64,
L = 8 at the smallest B for which every reduction has 17 partial workgroups — the finishing launch adds 16 slices of every
16th partial, so 17 is the first count at which a slice holds two.  Each at a row stride of exactly F D and at F D + 13 dense
columns padded to 64."""
import functools

import numpy as np
import pytest
import torch

from conftest import require_gpu

DEV = "cuda"
THR = float(np.float32(1e-5))  # the clamp of the kernels: float32(1e-5) < 1e-5
EPS, MOMENTUM = 1e-5, 0.1
SHAPES = [(1, 1, 4, 1), (3, 2, 4, 1), (65, 5, 8, 3), (257, 26, 16, 5), (300, 5, 40, 3), (513, 39, 64, 8)]
PLANTED = [0.0, 3e-6, -3e-6, 5e-6, -5e-6, 30.0, -12.0, 0.0]


def _ld(cols, pad=64):
    return (cols + pad - 1) // pad * pad


@functools.lru_cache(maxsize=None)
def make_case(B, F, D, L, stride, train, seed=0):
    """inputs of one case (CPU tensors, computed once, left unchanged).  x [B, stride]: e ~ N(0, 2 / D) in the first F D columns
    with planted exact zeros, +-3e-6, +-5e-6 (below the clamp), 30 and -12, nothing within 1e-7 of the clamp; behind them 13
    dense values and zero padding when the stride is wider.  bn1 / bn2: (gamma, beta, running mean, running var)"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * F + 7 * D + L + (1 if train else 0))
    n = F * D
    x = torch.zeros(B, stride)
    e = torch.randn(B, n, generator=g) * (2.0 / D) ** 0.5
    flat = e.view(-1)
    step = max(1, flat.numel() // 37)
    for j, pos in enumerate(range(1, flat.numel(), step)):
        if j % 2 == 0 or flat.numel() > 64:  # (the tiniest shapes keep every other planted value)
            flat[pos] = PLANTED[j % len(PLANTED)]
    near = (flat.abs() - THR).abs() < 1e-7
    flat[near] = 2e-5
    x[:, :n] = e
    if stride > n:
        x[:, n:n + 13] = torch.rand(B, 13, generator=g)
    W = torch.randn(L, F, generator=g) * (2.0 / F) ** 0.5
    bn1 = (1 + 0.1 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g), torch.full((F,), -2.3), torch.full((F,), 1.3))
    g2, b2 = 1 + 0.1 * torch.randn(L, generator=g), 0.1 * torch.randn(L, generator=g)
    # BN2's running statistics: those of c in float64 for this batch under BN1's running statistics
    xl = torch.log(torch.clamp(e.double().view(B, F, D).abs(), min=THR))
    y = (xl - (-2.3)) / (1.3 + EPS) ** 0.5 * bn1[0].double().view(1, F, 1) + bn1[1].double().view(1, F, 1)
    c = torch.exp(torch.einsum("lf,bfd->bld", W.double(), y))
    bn2 = (g2, b2, c.mean(dim=(0, 2)).float(), (c.var(dim=(0, 2), unbiased=False) + 1e-3).float())
    cot = torch.randn(B, _ld(L * D), generator=g)
    return dict(B=B, F=F, D=D, L=L, stride=stride, train=train, x=x, W=W, bn1=bn1, bn2=bn2, cot=cot)


def restate(c, thr=THR):
    """ranking/afn.py:93-102 and its gradients under the cotangent, in float64 with the clamp at thr = float32(1e-5) -> out [B, L D],
    dx [B, F D], dW, dg1, db1, dg2, db2, stats (mean1, var1, mean2, var2 used; biased) and, with batch statistics, run: the
    running buffers after the forward (momentum 0.1, unbiased variance, count B D)"""
    B, F, D, L, train = c["B"], c["F"], c["D"], c["L"], c["train"]
    E = c["x"][:, :F * D].double().view(B, F, D).requires_grad_(True)
    W = c["W"].double().requires_grad_(True)
    g1, b1, rm1, rv1 = (t.double() for t in c["bn1"])
    g2, b2, rm2, rv2 = (t.double() for t in c["bn2"])
    g1, b1, g2, b2 = (t.requires_grad_(True) for t in (g1, b1, g2, b2))
    a = E.abs()
    xl = torch.log(torch.where(a >= thr, a, torch.full_like(a, thr)))
    m1, v1 = (xl.mean(dim=(0, 2)), xl.var(dim=(0, 2), unbiased=False)) if train else (rm1, rv1)
    y = (xl - m1.view(1, F, 1)) / torch.sqrt(v1.view(1, F, 1) + EPS) * g1.view(1, F, 1) + b1.view(1, F, 1)
    z = torch.einsum("lf,bfd->bld", W, y)
    ce = torch.exp(z)
    m2, v2 = (ce.mean(dim=(0, 2)), ce.var(dim=(0, 2), unbiased=False)) if train else (rm2, rv2)
    out = ((ce - m2.view(1, L, 1)) / torch.sqrt(v2.view(1, L, 1) + EPS) * g2.view(1, L, 1) + b2.view(1, L, 1)).flatten(start_dim=1)
    (out * c["cot"][:, :L * D].double()).sum().backward()
    ref = dict(out=out.detach(), dx=E.grad.reshape(B, F * D), dW=W.grad, dg1=g1.grad, db1=b1.grad, dg2=g2.grad, db2=b2.grad,
               stats=tuple(t.detach() for t in (m1, v1, m2, v2)))
    if train:
        M = B * D
        unb = M / max(M - 1, 1)
        ref["run"] = ((1 - MOMENTUM) * rm1 + MOMENTUM * m1.detach(), (1 - MOMENTUM) * rv1 + MOMENTUM * v1.detach() * unb,
                      (1 - MOMENTUM) * rm2 + MOMENTUM * m2.detach(), (1 - MOMENTUM) * rv2 + MOMENTUM * v2.detach() * unb)
    return ref


@functools.lru_cache(maxsize=None)
def _reference(B, F, D, L, stride, train):
    return restate(make_case(B, F, D, L, stride, train))


def _close(got, ref, what, bar_of=None):
    bar = 1e-4 * max(1e-2, float((ref if bar_of is None else bar_of).abs().max()))
    err = float((got.detach().cpu().double() - ref).abs().max())
    print(f"{what}: max err {err:.3g}, bar {bar:.3g} ({err / bar:.3g})")
    assert err <= bar, f"{what}: {err} > {bar}"


def _cases():
    return [(s, wide, train) for s in SHAPES for wide in (False, True) for train in (True, False)]


def _id(v):
    return str(v).replace(" ", "")


def _direct(c, dx_buf=None):
    """one forward and one backward through the hip wrappers -> (out, z, stats, dx, dW, dg1, db1, dg2, db2)"""
    from rec_pangu_amd import hip
    F, D, L, train = c["F"], c["D"], c["L"], c["train"]
    x, W, cot = c["x"].to(DEV), c["W"].to(DEV), c["cot"].to(DEV)
    g1, b1, rm1, rv1 = (t.to(DEV) for t in c["bn1"])
    g2, b2, rm2, rv2 = (t.to(DEV) for t in c["bn2"])
    if train:
        stats = [torch.full((n,), float("nan"), device=DEV) for n in (F, F, L, L)]
    else:
        stats = [rm1, rv1, rm2, rv2]
    out = torch.full((c["B"], _ld(L * D)), 7.0, device=DEV)
    out, z = hip.lognet_fwd(x, F, D, W, g1, b1, stats[0], stats[1], EPS, g2, b2, stats[2], stats[3], EPS, train, out)
    res = hip.lognet_bwd(cot, x, z, F, D, W, g1, b1, stats[0], stats[1], EPS, g2, stats[2], stats[3], EPS, train, dx=dx_buf)
    torch.cuda.synchronize()
    return (out, z, stats) + tuple(res)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,wide,train", _cases(), ids=_id)
def test_kernels_against_float64(shape, wide, train):
    require_gpu()
    from rec_pangu_amd import functional as Fh, hip
    B, F, D, L = shape
    assert hip.lognet_fits(F, D, L)
    if shape == SHAPES[-1]:
        # the smallest B at which every reduction has 17 partial workgroups (the finish adds slices of every 16th partial)
        assert hip.lognet_plan(B, D)[0] == 17 and hip.lognet_plan(B - 1, D)[0] == 16
    stride = _ld(F * D + 13) if wide else F * D
    c = make_case(B, F, D, L, stride, train)
    ref = _reference(B, F, D, L, stride, train)
    n0 = hip.launch_count()
    out, z, stats, dx, dW, dg1, db1, dg2, db2 = _direct(c)
    assert hip.launch_count() - n0 == (10 if train else 6)
    tag = f"{_id(shape)} {'wide' if wide else 'exact'} {'batch' if train else 'running'}"
    _close(out[:, :L * D], ref["out"], f"{tag} out")
    assert bool((out[:, L * D:] == 7.0).all()), "the padding columns of the output were written"
    e = c["x"][:, :F * D].double()
    assert dx.shape == (B, F * D)
    _close(dx, ref["dx"], f"{tag} dx")
    scale = torch.clamp(e.abs(), min=1e-5)
    _close(dx.cpu().double() * scale, ref["dx"] * scale, f"{tag} dx |e|")
    below = e.abs() < THR
    assert int(below.sum()) >= 2 and bool((dx.cpu()[below] == 0).all()), "dx below the clamp must be exactly 0"
    _close(dW, ref["dW"], f"{tag} dW")
    _close(dg1, ref["dg1"], f"{tag} dgamma1")
    _close(db1, ref["db1"], f"{tag} dbeta1", bar_of=ref["dg1"] if train else None)
    _close(dg2, ref["dg2"], f"{tag} dgamma2")
    _close(db2, ref["db2"], f"{tag} dbeta2")
    if train:
        for name, got, want in zip(("mean1", "var1", "mean2", "var2"), stats, ref["stats"]):
            _close(got, want, f"{tag} {name}")
    # the autograd node on nn modules: the same launches (bit-identical), dx over the whole row buffer, the running buffers
    lin = torch.nn.Linear(F, L, bias=False).to(DEV)
    bn1, bn2 = torch.nn.BatchNorm1d(F, eps=EPS, momentum=MOMENTUM).to(DEV), torch.nn.BatchNorm1d(L, eps=EPS, momentum=MOMENTUM).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(c["W"])
        for bn, vals in ((bn1, c["bn1"]), (bn2, c["bn2"])):
            bn.weight.copy_(vals[0]), bn.bias.copy_(vals[1]), bn.running_mean.copy_(vals[2]), bn.running_var.copy_(vals[3])
    for m in (bn1, bn2):
        m.train(train)
    xd = c["x"].to(DEV).requires_grad_(True)
    o2 = Fh.logarithmic_net(xd, F, D, lin, bn1, bn2)
    assert o2.shape == (B, _ld(L * D)) and torch.equal(o2[:, :L * D], out[:, :L * D])
    o2.backward(c["cot"].to(DEV))
    assert xd.grad.shape == (B, stride) and torch.equal(xd.grad[:, :F * D], dx)
    assert bool((xd.grad[:, F * D:] == 0).all()), "columns beyond F D carry no gradient"
    for got, want in ((lin.weight.grad, dW), (bn1.weight.grad, dg1), (bn1.bias.grad, db1), (bn2.weight.grad, dg2), (bn2.bias.grad, db2)):
        assert torch.equal(got, want)
    if train:
        for name, got, want in zip(("running_mean1", "running_var1", "running_mean2", "running_var2"),
                                   (bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var), ref["run"]):
            _close(got, want, f"{tag} {name}")
        assert int(bn1.num_batches_tracked) == 1 and int(bn2.num_batches_tracked) == 1
    else:
        assert torch.equal(bn1.running_mean.cpu(), c["bn1"][2]) and torch.equal(bn2.running_var.cpu(), c["bn2"][3])
        assert int(bn1.num_batches_tracked) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("train", [True, False], ids=["batch", "running"])
def test_two_runs_are_bit_identical(train):
    require_gpu()
    B, F, D, L = SHAPES[-1]
    c = make_case(B, F, D, L, _ld(F * D + 13), train)
    a = _direct(c, dx_buf=torch.zeros(B, c["stride"], device=DEV))
    b = _direct(c, dx_buf=torch.zeros(B, c["stride"], device=DEV))
    flat = lambda r: [r[0], r[1], *r[2], *r[3:]]  # noqa: E731
    for k, (u, v) in enumerate(zip(flat(a), flat(b))):
        assert torch.equal(u, v), f"result {k} differs between two runs"


@pytest.mark.gpu
def test_shapes_outside_lognet_fits_are_refused_not_launched():
    require_gpu()
    from rec_pangu_amd import functional as Fh, hip
    lib = hip.lib()
    B, D = 8, 8
    for F, L in ((65, 3), (5, 9)):
        assert not hip.lognet_fits(F, D, L)
        x = torch.randn(B, F * D, device=DEV)
        W = torch.randn(L, F, device=DEV)
        v1, v2 = [torch.ones(F, device=DEV) for _ in range(4)], [torch.ones(L, device=DEV) for _ in range(4)]
        z, out = torch.zeros(B, L * D, device=DEV), torch.zeros(B, _ld(L * D), device=DEV)
        ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
        n0 = hip.launch_count()
        rc = lib.rp_lognet_fwd(x.data_ptr(), F * D, W.data_ptr(), *[t.data_ptr() for t in v1], EPS, *[t.data_ptr() for t in v2], EPS,
                               z.data_ptr(), out.data_ptr(), out.stride(0), B, F, D, L, 1, ws.data_ptr(), ws.numel(), None)
        assert rc == -3 and b"rp_lognet_fits" in lib.rp_last_error()  # RP_ERR_UNSUPPORTED
        rc = lib.rp_lognet_bwd(out.data_ptr(), out.stride(0), x.data_ptr(), F * D, z.data_ptr(), W.data_ptr(), v1[0].data_ptr(),
                               v1[1].data_ptr(), v1[2].data_ptr(), v1[3].data_ptr(), EPS, v2[0].data_ptr(), v2[2].data_ptr(),
                               v2[3].data_ptr(), EPS, x.data_ptr(), F * D, W.data_ptr(), v1[0].data_ptr(), v1[1].data_ptr(),
                               v2[0].data_ptr(), v2[1].data_ptr(), B, F, D, L, 1, ws.data_ptr(), ws.numel(), None)
        assert rc == -3 and hip.launch_count() == n0
        torch.cuda.synchronize()
        assert bool((out == 0).all())
        with pytest.raises(RuntimeError, match="lognet_fits"):
            Fh.logarithmic_net(x, F, D, torch.nn.Linear(F, L, bias=False).to(DEV), torch.nn.BatchNorm1d(F).to(DEV),
                               torch.nn.BatchNorm1d(L).to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 257, 1024 * 17 + 3])
def test_pair_fc_against_float64(B):
    """fc(cat[a, d]) for a Linear(2, 1): forward and the four gradients, at one sample, inside one workgroup and at 18 partial
    workgroups; two runs bit-identical"""
    require_gpu()
    from rec_pangu_amd import functional as Fh, hip
    assert hip.lib().rp_pair_fc_partials(B) == 3 * ((B + 1023) // 1024)
    g = torch.Generator().manual_seed(B)
    a, d, cot = (torch.randn(B, 1, generator=g) for _ in range(3))
    fc = torch.nn.Linear(2, 1)
    ref_fc = torch.nn.Linear(2, 1).double()
    ref_fc.load_state_dict({k: v.double() for k, v in fc.state_dict().items()})
    a64, d64 = a.double().requires_grad_(True), d.double().requires_grad_(True)
    ref = ref_fc(torch.cat([a64, d64], dim=-1))
    ref.backward(cot.double())
    fc = fc.to(DEV)
    runs = []
    for _ in range(2):
        fc.zero_grad()
        ad, dd = a.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
        out = Fh.pair_fc(ad, dd, fc)
        out.backward(cot.to(DEV))
        runs.append((out.detach(), ad.grad, dd.grad, fc.weight.grad.clone(), fc.bias.grad.clone()))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    out, da, dd_, dw, db = runs[0]
    assert out.shape == (B, 1) and dw.shape == (1, 2) and db.shape == (1,)
    _close(out, ref.detach(), f"pair_fc {B} out")
    _close(da, a64.grad, f"pair_fc {B} da")
    _close(dd_, d64.grad, f"pair_fc {B} dd")
    _close(dw, ref_fc.weight.grad, f"pair_fc {B} dw")
    _close(db, ref_fc.bias.grad, f"pair_fc {B} dbias")
