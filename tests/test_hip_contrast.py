"""The in-batch contrastive loss kernels (csrc/contrast.hip) alone on the GPU against float64 autograd of the host statement
Fh.contrastive_loss_reference (checked in tests/test_contrast_host.py against transcriptions of the reference's two losses).

Bar: the project's 1e-4 max(1e-2, max |ref|) per tensor: loss, lse, da and db, or the single gradient of the symmetric form.
The upstream gradient of every case is chosen (a power of two) so that the float64 gradient's max |.| is at least 1e-2, and
the test asserts it: the floor of the bar is never what passes.  Two kinds of case cannot be brought there:
- no row has a positive (distinct labels with the self pair excluded; n = 1 with it excluded): the float64 loss and gradient
  are zero identically, and the device must give exact zeros;
- the fp32 number format cannot: where each row's positive holds nearly all of its probability (n = 1, or 2 to 7 rows at
  T = 0.05), q = p - [positive] / c is a difference of two numbers near 1 that fp32 resolves to 2^-24 whatever evaluates
  it.  The criterion is not the kernel's: the composed fp32 statement (Fh.contrastive_loss_reference in float32, on the
  CPU) is run at the same upstream gradient, and only a case in which IT misses the scaled bar runs at upstream gradient 1,
  where the bar's floor bounds the absolute error by 1e-6.  Every case the composed statement resolves, the kernel must.

Shapes: n in {1, 2, 7, 33, 64, 300} symmetric (with and without exclude_self) and the asymmetric (7, 33), (300, 70) plus the
squares; d in {12, 64, 128}; T in {0.2, 0.05}; labels all distinct / three classes (asymmetric: one labels_a value absent
from labels_b, c_i = 0: that gradient row is exactly 0); rows normalised / scaled so that max |l| lies in [15, 32] / with one
all-zero row.  Every case runs twice and must give the same bits."""
import functools
import warnings

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.detach().abs().max()))


def frac(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max()) / bar(ref)


def check(tag, got, ref):
    for k in ref:
        print(f"{tag}: {k}: {frac(got[k], ref[k]):.3f} of the bar {bar(ref[k]):.3g}")
    for k in ref:
        assert got[k].shape == ref[k].shape and frac(got[k], ref[k]) <= 1.0, (tag, k, frac(got[k], ref[k]))


ROWS = ("normalised", "scaled", "zero_row")
LABELS = ("distinct", "three")
TEMPS = (0.2, 0.05)


def make_rows(n, d, kind, gen):
    x = torch.randn(n, d, generator=gen)
    if kind == "scaled":
        return x  # scaled below, once both operands are known
    x = torch.nn.functional.normalize(x, dim=-1)
    if kind == "zero_row" and n >= 2:
        x[n // 2] = 0
    return x


@functools.lru_cache(maxsize=None)
def case(n, m, d, T, labels, rows):
    """m = 0: the symmetric form -> (a, b | None, la, lb | None)"""
    gen = torch.Generator().manual_seed(((n * 1009 + m) * 131 + d) * 7 + int(T * 100) + 3 * LABELS.index(labels) + ROWS.index(rows))
    a = make_rows(n, d, rows, gen)
    b = make_rows(m, d, rows, gen) if m else None
    if rows == "scaled":
        top = float((a.double() @ (a if b is None else b).double().T).abs().max()) / T
        s = (24.0 / top) ** 0.5
        a = a * s
        b = None if b is None else b * s
        top = float((a.double() @ (a if b is None else b).double().T).abs().max()) / T
        assert 15.0 <= top <= 32.0, top
    if labels == "distinct":
        la, lb = torch.arange(n), (torch.arange(m) if m else None)
    else:
        la, lb = torch.arange(n) % 3, (torch.arange(m) % 3 if m else None)
        if m:
            la[0] = 99  # absent from labels_b: c_0 = 0
    return a, b, la, lb


def reference(a, b, la, lb, T, excl, scale):
    """float64 autograd of the host statement at upstream gradient 1"""
    from rec_pangu_amd import functional as Fh
    x = a.double().requires_grad_(True)
    y = None if b is None else b.double().requires_grad_(True)
    loss, lse = Fh.contrastive_loss_reference(x, y, la, lb, T, excl, scale, return_lse=True)
    loss.backward()
    ref = {"loss": loss.detach().view(1), "lse": lse, "da": x.grad}
    if y is not None:
        ref["db"] = y.grad
    return ref


def upstream(ref):
    """the power of two that brings the float64 gradient's max |.| to at least 1e-2"""
    top = max(float(ref[k].abs().max()) for k in ("da", "db") if k in ref)
    g = 1.0
    while top * g < 1e-2:
        g *= 2.0
    return g


def composed_fp32(a, b, la, lb, T, excl, scale, g):
    """the gradients of the host statement evaluated in float32 on the CPU at upstream gradient g"""
    from rec_pangu_amd import functional as Fh
    x = a.clone().requires_grad_(True)
    y = None if b is None else b.clone().requires_grad_(True)
    (Fh.contrastive_loss_reference(x, y, la, lb, T, excl, scale) * g).backward()
    return {"da": x.grad} if y is None else {"da": x.grad, "db": y.grad}


def device_run(a, b, la, lb, T, excl, scale, g):
    from rec_pangu_amd import functional as Fh, hip
    x = a.to(DEV).requires_grad_(True)
    y = None if b is None else b.to(DEV).requires_grad_(True)
    lad, lbd = la.to(DEV), (None if lb is None else lb.to(DEV))
    loss = Fh.contrastive_loss(x, y, lad, lbd, T, excl, scale)
    (loss * g).backward()
    loss2, lse, c = hip.contrast_fwd(x.detach(), None if y is None else y.detach(), lad, lbd, T, excl, scale)
    torch.cuda.synchronize()
    assert torch.equal(loss2.view(()), loss.detach())
    out = {"loss": loss.detach().view(1).cpu(), "lse": lse.cpu(), "da": x.grad.cpu(), "c": c.cpu()}
    if y is not None:
        out["db"] = y.grad.cpu()
    return out


def run_case(tag, a, b, la, lb, T, excl, scale):
    from rec_pangu_amd import hip
    ref = reference(a, b, la, lb, T, excl, scale)
    lbl = la if lb is None else lb
    eq = la.view(-1, 1) == lbl.view(1, -1)
    if excl:
        eq = eq & ~torch.eye(a.shape[0], dtype=torch.bool)
    counts = eq.sum(1)
    g = 1.0
    if int(counts.max()) == 0:  # no row has a positive: zero identically
        assert all(float(ref[k].abs().max()) == 0.0 for k in ("loss", "da", "db") if k in ref), tag
    else:
        g = upstream(ref)
        scaled = {k: ref[k] * g for k in ("da", "db") if k in ref}
        assert max(float(v.abs().max()) for v in scaled.values()) >= 1e-2, tag
        composed = composed_fp32(a, b, la, lb, T, excl, scale, g)
        if any(frac(composed[k], scaled[k]) > 1.0 for k in scaled):  # fp32 itself cannot: upstream gradient 1, on the floor
            print(f"{tag}: not resolved by the composed fp32 statement at upstream gradient {g:g}")
            g = 1.0
        else:
            ref.update(scaled)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = device_run(a, b, la, lb, T, excl, scale, g)
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0, tag
    assert torch.equal(got.pop("c"), counts.float()), tag
    check(tag, got, ref)
    empty = (counts == 0).nonzero().view(-1)
    if len(empty):  # a row without positives: its gradient row is exactly 0
        assert float(got["da"][empty].abs().max()) == 0.0 or b is None, tag
        if int(counts.max()) == 0:
            assert float(got["loss"].abs().max()) == 0.0 and all(float(got[k].abs().max()) == 0.0 for k in got if k[0] == "d"), tag
    again = device_run(a, b, la, lb, T, excl, scale, g)
    again.pop("c")
    for k in got:
        assert torch.equal(got[k], again[k]), (tag, k)


@pytest.mark.parametrize("d", [12, 64, 128])
@pytest.mark.parametrize("n", [1, 2, 7, 33, 64, 300])
def test_symmetric_form_against_float64_and_bit_identical(n, d):
    require_gpu()
    from rec_pangu_amd import hip
    geo = hip.contrast_geometry()
    assert (geo["TA"], geo["TB"], geo["max_d"]) == (32, 32, 128)  # the shapes sit around these
    for T in TEMPS:
        for labels in LABELS:
            for rows in ROWS:
                a, _, la, _ = case(n, 0, d, T, labels, rows)
                for excl in (False, True):
                    run_case(f"sym n={n} d={d} T={T} {labels} {rows} excl={int(excl)}", a, None, la, None, T, excl, T)


@pytest.mark.parametrize("d", [12, 64, 128])
@pytest.mark.parametrize("n,m", [(1, 1), (2, 2), (7, 7), (7, 33), (33, 33), (64, 64), (300, 70), (300, 300)])
def test_asymmetric_form_against_float64_and_bit_identical(n, m, d):
    require_gpu()
    for T in TEMPS:
        for labels in LABELS:
            for rows in ROWS:
                a, b, la, lb = case(n, m, d, T, labels, rows)
                run_case(f"asym n={n} m={m} d={d} T={T} {labels} {rows}", a, b, la, lb, T, False, 1.0)


def test_the_1e_10_inside_the_log_carries_the_result():
    """n = 2, symmetric with the self pair excluded, T = 0.05, the two rows at cosine below -0.5: the one remaining term of each
    row's sum is exp(l_01 - l_00) < 1e-10, so lse is m + log(1e-10) to fp32"""
    require_gpu()
    T = 0.05
    a = torch.nn.functional.normalize(torch.tensor([[1.0, 0.0, 0.0, 0.2], [-1.0, 0.3, 0.1, 0.0]]), dim=-1)
    la = torch.zeros(2, dtype=torch.int64)
    l = (a.double() @ a.double().T) / T
    assert float(a[0].double() @ a[1].double()) < -0.5
    for i in range(2):
        assert float(torch.exp(l[i, 1 - i] - l[i].max())) < 1e-10
    run_case("1e-10 carries", a, None, la, None, T, True, T)


def test_d_above_the_maximum_takes_the_counted_torch_path():
    require_gpu()
    from rec_pangu_amd import functional as Fh, hip
    d = hip.contrast_geometry()["max_d"] + 2
    assert not hip.contrast_fits(d) and hip.contrast_fits(d - 2) and not hip.contrast_fits(0)
    gen = torch.Generator().manual_seed(5)
    a = torch.nn.functional.normalize(torch.randn(9, d, generator=gen), dim=-1)
    la = torch.arange(9) % 3
    x = a.clone().requires_grad_(True)
    ref = Fh.contrastive_loss(x, None, la, None, 0.2, True, 0.2)
    ref.backward()
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    y = a.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = Fh.contrastive_loss(y, None, la.to(DEV), None, 0.2, True, 0.2)
    got.backward()
    assert hip.torch_path_count() == t0 + 1 and hip.launch_count() == n0
    assert abs(float(got) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    assert float((y.grad.cpu() - x.grad).abs().max()) <= 1e-5 * max(1e-2, float(x.grad.abs().max()))
    # the C entry point refuses the shape and launches nothing
    with pytest.raises(RuntimeError):
        hip.contrast_fwd(y.detach(), None, la.to(DEV), None, 0.2, True, 0.2)
    assert hip.launch_count() == n0
