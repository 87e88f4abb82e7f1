"""rp_ccpm_fwd / rp_ccpm_bwd alone against a float64 restatement of CCPM's conv stack written here (padded convolution along
the field axis, the rank-count selection with exact ties to the lower index, tanh, and autograd through the gather of the
selected positions), at the edges of the shape range.

A thread owns one (sample, column) pair, a workgroup 64 consecutive pairs of the B D; the backward's grid is capped at 512
workgroups (CAP_COLUMNS = 32768 columns), beyond which a workgroup walks several tiles and adds to its partial.

Near-ties.  k-max pooling is discontinuous: where the k-th and the (k+1)-th largest value of a conv line are closer than the
rounding difference of two correct fp32 evaluations, they may keep different positions.  The margin of a column is the minimum
over layers and channels with L_out > k of (k-th largest - (k+1)-th largest), computed in float64 from the test's own inputs.
Columns with a margin below 1e-5 (about 50 x the fp32 / fp64 difference of the conv outputs, which are of order 1: rows
N(0, 2 / D), Kaiming weights) are left out of the forward and the dx comparison and get a zero upstream gradient on both
sides, so the parameter gradients stay comparable; at most 2 % of a case's columns may be left out, which each test asserts."""
import ctypes
import functools

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 1e-5
CAP_COLUMNS = 512 * 64

# (F, D, channels, heights, B)
CASES = [
    (26, 32, (4, 4, 2), (6, 5, 3), 37),   # the Criteo geometry; B D not a multiple of the workgroup
    (5, 8, (4, 4, 2), (6, 5, 3), 24),     # kernel height >= input length at every layer
    (3, 4, (3,), (2,), 5),                # one layer, k = L_out - 1, D narrower than a wave
    (3, 16, (2,), (1,), 9),               # L_out = k: the selection is the identity, no padding
    (7, 20, (2, 3), (3, 2), 33),          # D not a power of two, C_out > C_in
    (40, 64, (4, 4, 2), (6, 5, 3), 9),    # the wide end of the range
]
IDS = ["F{}D{}c{}h{}B{}".format(F, D, "".join(map(str, c)), "".join(map(str, h)), B) for F, D, c, h, B in CASES]
BIG = (7, 8, (2, 3), (3, 2), 16384 + 3)   # B D >= 4 x CAP_COLUMNS: every partial of the capped grid, several tiles each


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


def k_schedule(F, n_layers):
    """ccpm.py:98-101"""
    return [max(3, int((1 - pow(float(i) / n_layers, n_layers - i)) * F)) if i < n_layers else 3
            for i in range(1, n_layers + 1)]


def stack64(x, Ws, bs, ks):
    """x [B, F, D], Ws[l] [C_out, C_in, kh, 1], bs[l] [C_out], all float64 -> (out [B, C_last k_last D] laid out as
    flatten(conv_out, 1), margin [B, D]).  Position i of a line is kept iff #{j: y_j > y_i or (y_j == y_i and j < i)} < k."""
    B, F, D = x.shape
    X = x.unsqueeze(1)
    margin = torch.full((B, D), float("inf"), dtype=torch.float64)
    for W, b, k in zip(Ws, bs, ks):
        kh, L = W.shape[2], X.shape[2]
        lout = L + kh - 1
        Xp = torch.nn.functional.pad(X, (0, 0, kh - 1, kh - 1))
        y = b.view(1, -1, 1, 1) + sum(torch.einsum("oc,bcld->bold", W[:, :, j, 0], Xp[:, :, j:j + lout]) for j in range(kh))
        yd = y.detach()
        yi, yj = yd.unsqueeze(3), yd.unsqueeze(2)  # [B, C, i, 1, D], [B, C, 1, j, D]
        pos = torch.arange(lout)
        lower = (pos.view(1, -1) < pos.view(-1, 1)).view(1, 1, lout, lout, 1)  # j < i
        rank = ((yj > yi) | ((yj == yi) & lower)).sum(dim=3)
        keep = rank < k
        assert bool((keep.sum(dim=2) == k).all())
        idx = torch.argsort((~keep).to(torch.int8), dim=2, stable=True)[:, :, :k]  # the kept positions, in their order
        if lout > k:
            s = yd.sort(dim=2, descending=True)[0]
            margin = torch.minimum(margin, (s[:, :, k - 1] - s[:, :, k]).min(dim=1)[0])
        X = torch.tanh(y.gather(2, idx))
    return X.flatten(start_dim=1), margin


def draw(F, D, channels, heights, B, seed):
    """fp32 inputs: rows N(0, 2 / D) (Kaiming-normal embedding tables), Kaiming-normal conv weights, Conv2d's own bias init"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F * D, generator=gen) * (2.0 / D) ** 0.5
    Ws, bs, cin = [], [], 1
    for co, kh in zip(channels, heights):
        W = torch.empty(co, cin, kh, 1)
        torch.nn.init.kaiming_normal_(W, generator=gen)
        bound = 1.0 / (cin * kh) ** 0.5
        Ws.append(W)
        bs.append((torch.rand(co, generator=gen) * 2 - 1) * bound)
        cin = co
    width = channels[-1] * 3 * D
    cot = torch.randn(B, width, generator=gen)
    return x, Ws, bs, cot


def reference(x, Ws, bs, cot, F, D, ks, use_margin=True):
    """float64 result and gradients; the upstream gradient of the columns below the margin is zeroed (returned as cot)"""
    B = x.shape[0]
    leaves = [x.double().view(B, F, D).requires_grad_(True)] + [t.double().requires_grad_(True) for t in Ws + bs]
    nl = len(Ws)
    out, margin = stack64(leaves[0], leaves[1:1 + nl], leaves[1 + nl:], ks)
    ok = (margin >= MARGIN) if use_margin else torch.ones_like(margin, dtype=torch.bool)
    cot = (cot.view(B, -1, D) * ok.view(B, 1, D)).reshape(B, -1)
    grads = torch.autograd.grad(out, leaves, cot.double())
    return dict(out=out.detach(), ok=ok, cot=cot, dx=grads[0].reshape(B, F * D), dW=grads[1:1 + nl], db=grads[1 + nl:])


@functools.lru_cache(maxsize=None)
def _case(F, D, channels, heights, B):
    ks = k_schedule(F, len(channels))
    x, Ws, bs, cot = draw(F, D, channels, heights, B, seed=100 * F + D + B)
    ref = reference(x, Ws, bs, cot, F, D, ks)
    return dict(x=x, Ws=Ws, bs=bs, ks=ks, **ref)


def _block(t, tight):
    """t [B, n] on the device: contiguous, or as a column block of a wider buffer with an odd row stride, one float in"""
    if tight:
        return t.to(DEV).contiguous()
    B, n = t.shape
    buf = torch.full((B, n + 13 + (n % 2)), 7.0, device=DEV)
    view = buf[:, 1:1 + n]
    view.copy_(t)
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 8 == 4
    return view


def _grad_close(got, ref, what):
    tol = 1e-4 * max(1e-2, float(ref.abs().max()))
    err = float((got.double().cpu() - ref.reshape(got.shape)).abs().max())
    print(f"{what}: {err:.3g} (bar {tol:.3g})")
    assert err <= tol, f"{what}: {err} > {tol}"


def _check_against(c, F, D, tight, what=""):
    from rec_pangu_amd import hip
    B = c["x"].shape[0]
    ok = c["ok"]
    excluded = int((~ok).sum())
    print(f"{what}columns below the margin: {excluded} of {ok.numel()}")
    assert excluded <= 0.02 * ok.numel(), "more than 2 % of the columns are near-ties: choose another seed"
    x = _block(c["x"], tight)
    Ws, bs = [w.to(DEV) for w in c["Ws"]], [b.to(DEV) for b in c["bs"]]
    n0 = hip.launch_count()
    out = hip.ccpm_fwd(x, Ws, bs, F, D, c["ks"])
    assert hip.launch_count() == n0 + 1, "the forward is one launch for the whole stack"
    assert out.shape == c["out"].shape
    okc = ok.view(B, 1, D)
    err = float(((out.double().cpu() - c["out"]).view(B, -1, D) * okc).abs().max())
    print(f"out: {err:.3g} (bar 1e-05)")
    assert err <= 1e-5
    dxbuf = torch.full((B, F * D + (0 if tight else 13)), 3.0, device=DEV)
    dxv = dxbuf if tight else dxbuf[:, 1:1 + F * D]
    dx, dWs, dbs = hip.ccpm_bwd(_block(c["cot"], tight), x, Ws, bs, F, D, c["ks"], dx=dxv)
    assert hip.launch_count() == n0 + 3  # the column walk and the finishing launch
    okx = ok.view(B, 1, D).expand(B, F, D).reshape(B, F * D)
    _grad_close(dx.double().cpu() * okx, c["dx"] * okx, "dx")
    for l, (dW, db) in enumerate(zip(dWs, dbs)):
        _grad_close(dW, c["dW"][l], f"dW{l}")
        _grad_close(db, c["db"][l], f"db{l}")
    if not tight:
        outside = torch.ones(dxbuf.shape[1], dtype=torch.bool)
        outside[1:1 + F * D] = False
        assert torch.all(dxbuf[:, outside.to(DEV)] == 3.0), "dx's neighbours in the wider buffer were written"
    return x, Ws, bs


@pytest.mark.parametrize("tight", [True, False], ids=["tight", "odd_offset"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_vs_float64(case, tight):
    from rec_pangu_amd import hip
    F, D, channels, heights, B = case
    c = _case(*case)
    assert hip.ccpm_fits(F, D, channels, heights, c["ks"])
    _check_against(c, F, D, tight)


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_backward_is_bit_identical_from_run_to_run(case):
    from rec_pangu_amd import hip
    F, D, channels, heights, B = case
    c = _case(*case)
    x, cot = c["x"].to(DEV), c["cot"].to(DEV)
    Ws, bs = [w.to(DEV) for w in c["Ws"]], [b.to(DEV) for b in c["bs"]]
    runs = []
    for _ in range(2):
        dx, dWs, dbs = hip.ccpm_bwd(cot, x, Ws, bs, F, D, c["ks"])
        runs.append([dx] + dWs + dbs)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_every_partial_of_the_capped_grid():
    """B D >= 4 x the cap's columns: each of the 512 workgroups walks at least four tiles, the last tile partial; parameter
    gradients (and everything else) against float64 with the same bars; two runs bit-identical"""
    from rec_pangu_amd import hip
    F, D, channels, heights, B = BIG
    assert B * D >= 4 * CAP_COLUMNS and (B * D) % 64 != 0
    c = _case(*BIG)
    x, Ws, bs = _check_against(c, F, D, True)
    cot = c["cot"].to(DEV)
    a = hip.ccpm_bwd(cot, x, Ws, bs, F, D, c["ks"])
    b = hip.ccpm_bwd(cot, x, Ws, bs, F, D, c["ks"])
    for p, q in zip([a[0]] + a[1] + a[2], [b[0]] + b[1] + b[2]):
        assert torch.equal(p, q)


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_exact_ties_go_to_the_lower_index(case):
    """rows of zeros: every conv line of layer 0 equals its bias, and so on up the stack — all ties.  The kept positions are
    the first k, so the gradient lands there: against the float64 restatement, which implements the lower-index rule (no
    margin rule here: every margin is zero)"""
    F, D, channels, heights, B = case
    ks = k_schedule(F, len(channels))
    _, Ws, bs, cot = draw(F, D, channels, heights, B, seed=77)
    x = torch.zeros(B, F * D)
    ref = reference(x, Ws, bs, cot, F, D, ks, use_margin=False)
    assert bool(ref["ok"].all())
    c = dict(x=x, Ws=Ws, bs=bs, ks=ks, **ref)
    _check_against(c, F, D, True, what="(ties) ")
    # db of layer 0 sees exactly the first k positions of each line: dW[co, 0, j] is zero (x is zero), db is not
    assert float(ref["db"][0].abs().max()) > 0


def test_a_shape_outside_the_range_is_refused():
    from rec_pangu_amd import hip
    lib = hip.lib()
    F, D, B = 6, 8, 4
    x = torch.zeros(B, F * D, device=DEV)
    W, b = torch.zeros(5, 1, 2, 1, device=DEV), torch.zeros(5, device=DEV)  # five channels: outside rp_ccpm_fits
    out = torch.zeros(B, 5 * 3 * D, device=DEV)
    assert not hip.ccpm_fits(F, D, [5], [2], [3])
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    ptrs = lambda *t: (ctypes.c_void_p * len(t))(*[u.data_ptr() for u in t])  # noqa: E731
    n0 = hip.launch_count()
    rc = lib.rp_ccpm_fwd(x.data_ptr(), F * D, ptrs(W), ptrs(b), out.data_ptr(), 5 * 3 * D, F, D, 1, ints(5), ints(2), ints(3),
                         B, None)
    assert rc == -3 and hip.launch_count() == n0  # RP_ERR_UNSUPPORTED, nothing launched
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    rc = lib.rp_ccpm_bwd(out.data_ptr(), 5 * 3 * D, x.data_ptr(), F * D, ptrs(W), ptrs(b), x.data_ptr(), F * D, ptrs(W),
                         ptrs(b), F, D, 1, ints(5), ints(2), ints(3), B, ws.data_ptr(), ws.numel(), None)
    assert rc == -3 and hip.launch_count() == n0
    with pytest.raises(RuntimeError, match="rp_ccpm_fits"):
        hip.ccpm_fwd(x, [W], [b], F, D, [3])
