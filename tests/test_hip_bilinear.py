"""rp_bilinear_fwd / rp_bilinear_bwd alone against a float64 restatement written here: T[b, p, :] = (W_w(p) E_i) * E_j formed
ONCE per pair, the second branch as A_i A_j T with A = relu(W2 relu(W1 mean_d E)), gradients by float64 autograd over that
form.  tests/test_fibinet_host.py pins the restatement to the layers' own (reference) formulation to 1e-12 and checks the
condition on the inputs that makes the comparison total: every SENET pre-activation of every case is, in float64, either
exactly 0 (a sum over an all-zero hidden layer) or at least 1e-5 away from 0, so no fp32 rounding can move a unit across its
ReLU kink, and active and inactive units both occur.  The seeds below were chosen for that (the first from 1 upward).  Every
output and gradient is compared, with the project's bar 1e-4 * max(1e-2, max |ref|)."""
import functools
from itertools import combinations

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINK = 1e-5

# (F, D, B, type, R): the smallest shapes at which each part can go wrong
CASES = [
    (2, 8, 1, "field_all", 0),               # one pair, one sample, no SENET
    (2, 16, 5, "field_interaction", 1),      # one pair with SENET
    (5, 8, 37, "field_all", 1),              # B not a multiple of any tile; shared weights summed over pairs
    (5, 8, 37, "field_each", 1),
    (5, 8, 37, "field_interaction", 1),
    (7, 64, 9, "field_interaction", 2),      # the widest D
    (26, 32, 70, "field_interaction", 8),    # the workload's geometry: more than one tile and one batch slice
    (40, 16, 3, "field_each", 13),           # the largest F
]
# sizes at which the launches take another path
EDGES = [
    (2, 8, 16384 + 37, "field_all", 1),      # more than one backward chunk of 16384 samples (partials added to)
    (2, 64, 2048 + 100, "field_interaction", 1),  # more than 512 tiles of 256 / D samples: a workgroup walks several
]
# the first seed from 1 upward that meets the condition AND gives the SENET a gradient that is not identically zero (with two
# fields and one hidden unit both entries of W2 have to be positive for any A_0 A_1 to be)
SEEDS = {c: 1 for c in CASES + EDGES}
SEEDS[CASES[1]] = 2
SEEDS[EDGES[0]] = 13


def case_id(c):
    return "F{}D{}B{}-{}-R{}".format(c[0], c[1], c[2], c[3][6:], c[4])


def weight_map(F, btype):
    pairs = list(combinations(range(F), 2))
    return pairs, [0 if btype == "field_all" else i if btype == "field_each" else p for p, (i, _) in enumerate(pairs)]


def n_weights(F, btype):
    return {"field_all": 1, "field_each": F, "field_interaction": F * (F - 1) // 2}[btype]


def draw(F, D, B, btype, R, n_dense=0, seed=1):
    """fp32 inputs of a case: x [B, F D + n_dense], the [D, D] matrices, (W1, W2) or None, the cotangent [B, width]"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * F + D + R)
    P = F * (F - 1) // 2
    x = torch.cat([0.5 * torch.randn(B, F * D, generator=g), torch.rand(B, n_dense, generator=g)], dim=1)
    Ws = [torch.randn(D, D, generator=g) / D ** 0.5 for _ in range(n_weights(F, btype))]
    senet = (2.0 * torch.randn(R, F, generator=g), torch.randn(F, R, generator=g) / R ** 0.5) if R > 0 else None
    cot = torch.randn(B, (2 if R else 1) * P * D + n_dense, generator=g)
    return x, Ws, senet, cot


def preactivations(x, senet, F, D):
    """(pre1 [B, R], pre2 [B, F]) of the SENET in float64"""
    Z = x[:, :F * D].double().view(-1, F, D).mean(dim=-1)
    pre1 = Z @ senet[0].double().t()
    return pre1, torch.relu(pre1) @ senet[1].double().t()


def restatement(x, Ws, senet, cot, F, D, btype, n_dense=0):
    """float64: out and the gradients of x's embedding columns, of the stacked matrices and of W1, W2 under `cot`"""
    pairs, wmap = weight_map(F, btype)
    I, J = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    E = x[:, :F * D].double().view(-1, F, D).requires_grad_(True)
    W = torch.stack(Ws).double().requires_grad_(True)
    T = torch.einsum("pdk,bpk->bpd", W[torch.tensor(wmap)], E[:, I]) * E[:, J]  # once per pair
    parts = [T.flatten(1)]
    leaves = [E, W]
    if senet is not None:
        W1, W2 = senet[0].double().requires_grad_(True), senet[1].double().requires_grad_(True)
        A = torch.relu(torch.relu(E.mean(dim=-1) @ W1.t()) @ W2.t())
        parts.append(((A[:, I] * A[:, J]).unsqueeze(-1) * T).flatten(1))
        leaves += [W1, W2]
    out = torch.cat(parts + [x[:, F * D:F * D + n_dense].double()], dim=1)
    grads = torch.autograd.grad(out, leaves, cot.double())
    res = {"out": out.detach(), "dx": grads[0].reshape(-1, F * D), "dW": grads[1]}
    if senet is not None:
        res["dW1"], res["dW2"] = grads[2], grads[3]
    return res


@functools.lru_cache(maxsize=None)
def _case(case, n_dense=0):
    """inputs and float64 reference of a case: computed once, shared by the tests that need it, left unchanged"""
    F, D, B, btype, R = case
    x, Ws, senet, cot = draw(F, D, B, btype, R, n_dense, SEEDS[case])
    return dict(x=x, Ws=Ws, senet=senet, cot=cot, ref=restatement(x, Ws, senet, cot, F, D, btype, n_dense))


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


def _dev(c):
    senet = None if c["senet"] is None else tuple(w.to(DEV) for w in c["senet"])
    return c["x"].to(DEV), [w.to(DEV) for w in c["Ws"]], senet, c["cot"].to(DEV)


def _check_grads(case, ref, dx, dW, dW1, dW2, what):
    F, D, B, btype, R = case
    _close(dx[:, :F * D], ref["dx"], f"{what} dx")
    _close(dW, ref["dW"], f"{what} dW")
    if btype == "field_each":
        assert not dW[F - 1].any(), "the last field opens no pair: its matrix has a zero gradient"
    if R > 0:
        _close(dW1, ref["dW1"], f"{what} dW1")
        _close(dW2, ref["dW2"], f"{what} dW2")
    else:
        assert dW1 is None and dW2 is None


@pytest.mark.parametrize("case", CASES + EDGES, ids=case_id)
def test_forward_and_backward_against_float64(case):
    from rec_pangu_amd import hip
    F, D, B, btype, R = case
    assert hip.bilinear_fits(F, D, R, btype)
    c = _case(case)
    x, Ws, senet, cot = _dev(c)
    out = hip.bilinear_fwd(x, F, D, Ws, btype, senet)
    assert out.shape == c["ref"]["out"].shape
    _close(out, c["ref"]["out"], f"{case_id(case)} out")
    dx, dW, dW1, dW2 = hip.bilinear_bwd(cot, x, F, D, Ws, btype, senet)
    assert dx.shape == (B, F * D) and dW.shape == (len(Ws), D, D)
    _check_grads(case, c["ref"], dx, dW, dW1, dW2, case_id(case))


WIDE = (5, 8, 37, "field_interaction", 1)


def test_dense_columns_are_copied_through():
    from rec_pangu_amd import hip
    F, D, B, btype, R = WIDE
    c = _case(WIDE, 3)
    x, Ws, senet, cot = _dev(c)
    out = hip.bilinear_fwd(x, F, D, Ws, btype, senet, n_dense=3)
    assert torch.equal(out[:, -3:].cpu(), c["x"][:, F * D:])
    _close(out, c["ref"]["out"], "out with dense columns")
    dx, dW, dW1, dW2 = hip.bilinear_bwd(cot, x, F, D, Ws, btype, senet, n_dense=3)
    _check_grads(WIDE, c["ref"], dx, dW, dW1, dW2, "with dense columns")


def test_leading_dimensions_larger_than_the_rows_and_untouched_padding():
    """source, destination and both gradient buffers wider than their rows: what lies behind the row is neither read (NaN there
    would spread) nor written (prefilled, compared)"""
    from rec_pangu_amd import hip
    F, D, B, btype, R = WIDE
    c = _case(WIDE, 3)
    _, Ws, senet, _ = _dev(c)
    width = c["ref"]["out"].shape[1]
    xw = torch.full((B, F * D + 3 + 5), float("nan"), device=DEV)
    xw[:, :F * D + 3] = c["x"].to(DEV)
    outw = torch.full((B, width + 7), 7.0, device=DEV)
    res = hip.bilinear_fwd(xw, F, D, Ws, btype, senet, n_dense=3, out=outw)
    assert res.data_ptr() == outw.data_ptr()
    _close(outw[:, :width], c["ref"]["out"], "wide out")
    assert bool((outw[:, width:] == 7.0).all()), "the forward wrote behind its columns"
    cotw = torch.full((B, width + 7), float("nan"), device=DEV)
    cotw[:, :width] = c["cot"].to(DEV)
    dxw = torch.full((B, F * D + 6), -3.0, device=DEV)
    dx, dW, dW1, dW2 = hip.bilinear_bwd(cotw, xw, F, D, Ws, btype, senet, n_dense=3, dx=dxw)
    assert dx.data_ptr() == dxw.data_ptr()
    _check_grads(WIDE, c["ref"], dxw, dW, dW1, dW2, "wide")
    assert bool((dxw[:, F * D:] == -3.0).all()), "the backward wrote behind the embedding columns of dx"
    # the embedding block of a wider row buffer as a strided view (what the model hands over)
    out2 = hip.bilinear_fwd(xw[:, :F * D + 3], F, D, Ws, btype, senet, n_dense=3)
    assert torch.equal(out2, outw[:, :width])


def test_dx_is_added_into_a_prefilled_buffer():
    from rec_pangu_amd import hip
    case = (5, 8, 37, "field_each", 1)
    F, D, B, btype, R = case
    c = _case(case)
    x, Ws, senet, cot = _dev(c)
    pre = torch.randn(B, F * D, generator=torch.Generator().manual_seed(3))
    dxa = pre.to(DEV)
    dx, dW, dW1, dW2 = hip.bilinear_bwd(cot, x, F, D, Ws, btype, senet, dx=dxa, accumulate=True)
    ref = dict(c["ref"], dx=c["ref"]["dx"] + pre.double())
    _check_grads(case, ref, dxa, dW, dW1, dW2, "accumulate")
    with pytest.raises(RuntimeError, match="accumulate"):
        hip.bilinear_bwd(cot, x, F, D, Ws, btype, senet, accumulate=True)


def test_backward_is_bit_identical_from_run_to_run():
    from rec_pangu_amd import hip
    case = (26, 32, 70, "field_interaction", 8)
    F, D, B, btype, R = case
    x, Ws, senet, cot = _dev(_case(case))
    a = hip.bilinear_bwd(cot, x, F, D, Ws, btype, senet)
    b = hip.bilinear_bwd(cot, x, F, D, Ws, btype, senet)
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    assert torch.equal(hip.bilinear_fwd(x, F, D, Ws, btype, senet), hip.bilinear_fwd(x, F, D, Ws, btype, senet))


def test_outside_the_range_is_refused_before_any_launch():
    import ctypes
    from rec_pangu_amd import hip
    lib = hip.lib()
    F, D, B = 3, 12, 4  # D = 12: outside rp_bilinear_fits
    x = torch.zeros(B, F * D, device=DEV)
    Ws = [torch.zeros(D, D, device=DEV) for _ in range(3)]
    assert not hip.bilinear_fits(F, D, 0, "field_interaction")
    n0 = hip.launch_count()
    with pytest.raises(RuntimeError, match="rp_bilinear_fits"):
        hip.bilinear_fwd(x, F, D, Ws, "field_interaction")
    tab = torch.tensor([w.data_ptr() for w in Ws], dtype=torch.int64, device=DEV)
    wmap = torch.arange(3, dtype=torch.int32, device=DEV)
    out = torch.zeros(B, 3 * D, device=DEV)
    rc = lib.rp_bilinear_fwd(x.data_ptr(), F * D, None, None, tab.data_ptr(), wmap.data_ptr(), out.data_ptr(), 3 * D, F, D, 0,
                             2, 0, B, None)
    assert rc == -3 and b"rp_bilinear_fits" in lib.rp_last_error()
    n = ctypes.c_size_t(0)
    assert lib.rp_bilinear_bwd_workspace_bytes(F, D, 0, 2, ctypes.byref(n)) == -3
    assert hip.launch_count() == n0
