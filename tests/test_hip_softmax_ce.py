"""The full-softmax loss kernels alone (rp_softmax_ce_fwd / _bwd) against float64, on the GPU.

Reference: cross_entropy(U.double() @ E.double().T, t) and its autograd on the CPU, with an upstream gradient g = 1.7.
Bar, per tensor (loss, lse, dU, dE): the project's 1e-4 max(1e-2, max |ref|).

What the bar leaves: torch's own fp32 formulation of the same loss (fp32 matmul, log_softmax, autograd, on the CPU) differs from
the float64 reference by at most 0.054 of that bar over the cases of this file (per tensor the worst case: loss 0.0018,
lse 0.002, dU 0.054 at scores_470, dE 0.03; measured with `python tests/test_hip_softmax_ce.py`, which needs no GPU) — about
20 times below it, so a kernel that keeps fp32 faith has room and one that drops to a single bf16 product does not.

Cases are named by the kernels' own geometry (hip.softmax_ce_geometry: TB rows of U per workgroup, TV rows of E per tile,
`slices` lanes per row in the finishing merge; hip.softmax_ce_splits: the split of V), not by guessed numbers."""
import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu

G_UP = 1.7


def _geom():
    from rec_pangu_amd import hip
    g = hip.softmax_ce_geometry()
    return g["TB"], g["TV"], g["slices"], g["max_d"]


def _smallest_v(B, pred):
    """the smallest V whose split (n, tiles per split) satisfies pred(V, n, per)"""
    from rec_pangu_amd import hip
    for V in range(1, 1 << 16):
        n, per = hip.softmax_ce_splits(B, V)
        if pred(V, n, per):
            return V
    raise AssertionError("no such V")


def _v_two_splits_partial_tail(B):
    TB, TV, _, _ = _geom()
    # two splits, the last of them holding exactly one tile, and that tile partial
    return _smallest_v(B, lambda V, n, per: n == 2 and 0 < V - per * TV < TV)


def _v_two_entries_per_slice(B):
    _, _, slices, _ = _geom()
    return _smallest_v(B, lambda V, n, per: n >= 2 * slices)


# name -> () -> dict(B, V, D, and optionally mult, ldu, targets, spike)
CASES = {
    "1x2x4": lambda: dict(B=1, V=2, D=4),
    "3x33x8": lambda: dict(B=3, V=33, D=8),
    "B=TB-1,V=TV-1": lambda: dict(B=_geom()[0] - 1, V=_geom()[1] - 1, D=16),
    "B=TB,V=TV+1": lambda: dict(B=_geom()[0], V=_geom()[1] + 1, D=16),
    "B=TB+1,V=TV+1": lambda: dict(B=_geom()[0] + 1, V=_geom()[1] + 1, D=16),
    "two_splits_partial_last_tile": lambda: dict(B=5, V=_v_two_splits_partial_tail(5), D=16),
    "two_entries_per_merge_slice": lambda: dict(B=_geom()[0] + 1, V=_v_two_entries_per_slice(_geom()[0] + 1), D=16),
    "D=40": lambda: dict(B=33, V=70, D=40),
    "D=20": lambda: dict(B=5, V=70, D=20),
    "D=64": lambda: dict(B=33, V=130, D=64),
    "D=70": lambda: dict(B=3, V=40, D=70),
    "D=100": lambda: dict(B=2, V=35, D=100),
    "D=max_d": lambda: dict(B=3, V=40, D=_geom()[3]),
    "ldu>D": lambda: dict(B=33, V=70, D=32, ldu=40),
    "ldu>D_unaligned": lambda: dict(B=7, V=70, D=16, ldu=19),
    "all_targets_equal": lambda: dict(B=35, V=67, D=16, targets="equal"),
    "targets_0_and_V-1": lambda: dict(B=34, V=67, D=16, targets="ends"),
    "scores_170": lambda: dict(B=65, V=515, D=64, mult=6.0, spike=True),
    "scores_470": lambda: dict(B=65, V=515, D=64, mult=10.0, spike=True),
    "V=70000": lambda: dict(B=33, V=70000, D=16),
}


def make_inputs(B, V, D, mult=1.0, ldu=None, targets=None, spike=False, seed=0):
    """CPU float32 (U [B, D] as a view of [B, ldu], E [V, D], t int64 [B])"""
    gen = torch.Generator().manual_seed(seed)
    E = torch.randn(V, D, generator=gen)
    wide = torch.randn(B, ldu or D, generator=gen) * mult
    U = wide[:, :D]
    if spike:  # row 0 peaks in the first tile of E, row 1 in the last
        U[0] = E[3] * mult
        U[1] = E[V - 2] * mult
    t = torch.randint(0, V, (B,), generator=gen)
    if targets == "equal":
        t[:] = V // 2
    elif targets == "ends":
        t[0::2] = 0
        t[1::2] = V - 1
    return U, E, t


def reference(U, E, t):
    """float64 on the CPU: (loss, lse [B], dU, dE) at the upstream gradient G_UP, and the scores"""
    U64, E64 = U.double().clone().requires_grad_(True), E.double().clone().requires_grad_(True)
    s = U64 @ E64.t()
    loss = torch.nn.functional.cross_entropy(s, t)
    (loss * G_UP).backward()
    return {"loss": loss.detach().reshape(1), "lse": torch.logsumexp(s.detach(), dim=1), "dU": U64.grad, "dE": E64.grad}, s.detach()


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def run_kernels(U, E, t):
    from rec_pangu_amd import hip
    dev = torch.device("cuda:0")
    wide = U._base if U._base is not None else U
    Ud = wide.to(dev)[:, :U.shape[1]]
    Ed, td = E.to(dev), t.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    loss, lse = hip.softmax_ce_fwd(Ud, Ed, td, flag)
    dU, dE = hip.softmax_ce_bwd(Ud, Ed, td, lse, torch.tensor([G_UP], device=dev))
    assert int(flag.item()) == 0
    return {"loss": loss.cpu(), "lse": lse.cpu(), "dU": dU.cpu(), "dE": dE.cpu()}


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_float64_and_bit_identical(name):
    require_gpu()
    spec = CASES[name]()
    U, E, t = make_inputs(**spec)
    ref, s = reference(U, E, t)
    if spec.get("spike"):
        TV = _geom()[1]
        assert int(s[0].argmax()) < TV and int(s[1].argmax()) >= (spec["V"] - 1) // TV * TV
        assert float(s.abs().max()) > 17 * spec["mult"]  # ±170 / ±470: exp overflows fp32 without the running maximum
    if name == "two_splits_partial_last_tile":
        from rec_pangu_amd import hip
        assert hip.softmax_ce_splits(spec["B"], spec["V"])[0] == 2 and hip.softmax_ce_splits(spec["B"], spec["V"] - 1)[0] == 1
    got = run_kernels(U, E, t)
    for k, want in ref.items():
        err = float((got[k].double() - want).abs().max())
        print(f"{name}: {k}: max err {err:.3g} against bar {bar(want):.3g}")
        assert got[k].shape == want.shape and err <= bar(want), (name, k, err, bar(want))
    again = run_kernels(U, E, t)
    for k in ref:
        assert torch.equal(got[k], again[k]), (name, k)


def _operand_error_bars(U, E, t, delta):
    """First-order bars, in float64, for kernels whose every matrix product carries a relative error of at most `delta` per
    term (split-bf16 operands: the pieces dropped by the split):  |s~ - s| <= A = delta |U| |E|^T, hence |lse~ - lse| <= max_v A
    (lse is 1-Lipschitz in the sup norm), |log p~ - log p| <= 2 max_v A, i.e. |dp| <= p (exp(2 max_v A) - 1); the second
    products add delta per term again:  |d dU| <= (g/B) (|dp| + delta |p'|) |E|,  |d dE| <= (g/B) (|dp| + delta |p'|)^T |U|."""
    U64, E64 = U.double(), E.double()
    s = U64 @ E64.t()
    A = delta * (U64.abs() @ E64.abs().t())
    amax = A.max(dim=1).values
    p = torch.softmax(s, dim=1)
    pp = p.clone()
    pp[torch.arange(len(t)), t] -= 1
    dp = p * torch.expm1(2 * amax)[:, None] + delta * pp.abs()
    gb = G_UP / len(t)
    return {"lse": amax, "loss": (amax + A[torch.arange(len(t)), t]).mean().reshape(1),
            "dU": gb * (dp @ E64.abs()), "dE": gb * (dp.t() @ U64.abs())}


@pytest.mark.parametrize("mode,delta", [("bf16x3", 2.0 ** -16), ("bf16", 2.0 ** -8 + 2.0 ** -17)])
@pytest.mark.parametrize("shape", [(33, 130, 64), (5, 70, 20), (3, 40, 128)])
def test_reduced_product_modes_stay_within_their_operand_error(mode, delta, shape):
    """rp_set_matmul_precision reaches the 3- and 1-product forms of every launch.  Per product term the split drops at most
    2 * 2^-18 + 2^-18 < 2^-16 (two round-to-nearest pieces per operand, the mid x mid term) / 2 * 2^-9 + 2^-18 (one piece);
    the bars are those figures carried through the loss to first order, plus the fp32 bar of the six-product form."""
    require_gpu()
    from rec_pangu_amd import hip
    U, E, t = make_inputs(*shape)
    ref, _ = reference(U, E, t)
    bars = _operand_error_bars(U, E, t, delta)
    hip.set_matmul_precision(mode)
    try:
        got, again = run_kernels(U, E, t), run_kernels(U, E, t)
    finally:
        hip.set_matmul_precision("auto")
    for k, want in ref.items():
        err = (got[k].double() - want).abs()
        allowed = bars[k] + bar(want)
        print(f"{mode} {shape}: {k}: max err {float(err.max()):.3g}, max allowed {float(allowed.max()):.3g}")
        assert bool((err <= allowed).all()), (mode, shape, k, float((err / allowed).max()))
        assert torch.equal(got[k], again[k])


def test_autograd_wrapper_and_upstream_gradient():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    U, E, t = make_inputs(33, 130, 64)
    ref, _ = reference(U, E, t)
    Ud, Ed = U.cuda().requires_grad_(True), E.cuda().requires_grad_(True)
    loss = Fh.full_softmax_ce(Ud, Ed, t.cuda())
    assert loss.dim() == 0
    (loss * G_UP).backward()
    for k, got in (("loss", loss.detach().reshape(1)), ("dU", Ud.grad), ("dE", Ed.grad)):
        assert float((got.cpu().double() - ref[k]).abs().max()) <= bar(ref[k]), k


def test_target_equal_to_v_raises_index_error_in_the_checked_mode():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    U, E, t = (x.cuda() for x in make_inputs(5, 33, 8))
    t[2] = 33
    with pytest.raises(IndexError):
        Fh.full_softmax_ce(U, E, t)
    t[2] = 32
    assert torch.isfinite(Fh.full_softmax_ce(U, E, t))  # the flag was cleared by the raise
    t[2] = -1
    loss = Fh.full_softmax_ce(U, E, t, check_indices="deferred")  # counted as item 0, the flag stays set
    assert torch.isfinite(loss) and int(Fh._seq_flag(U.device).item()) == 1
    Fh._seq_flag(U.device).zero_()


def test_d_above_the_budget_composes_from_torch_and_says_so():
    require_gpu()
    import warnings
    from rec_pangu_amd import functional as Fh, hip
    D = _geom()[3] + 8
    U, E, t = make_inputs(4, 20, D)
    ref, _ = reference(U, E, t)
    n0 = hip.torch_path_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = Fh.full_softmax_ce(U.cuda(), E.cuda(), t.cuda())
    assert hip.torch_path_count() == n0 + 1
    assert abs(float(loss) - float(ref["loss"])) <= bar(ref["loss"])


if __name__ == "__main__":
    # the measurement quoted in the module docstring: torch's fp32 formulation against the float64 reference, on the CPU
    worst = {}
    for name, spec in CASES.items():
        try:
            U, E, t = make_inputs(**spec())
        except RuntimeError as e:  # the geometry comes from the built library
            raise SystemExit(f"{name}: {e}")
        ref, _ = reference(U, E, t)
        U32, E32 = U.clone().requires_grad_(True), E.clone().requires_grad_(True)
        s = U32 @ E32.t()
        loss = torch.nn.functional.cross_entropy(s, t)
        (loss * G_UP).backward()
        got = {"loss": loss.detach().reshape(1), "lse": torch.logsumexp(s.detach(), dim=1), "dU": U32.grad, "dE": E32.grad}
        row = {k: float((got[k].double() - ref[k]).abs().max()) / bar(ref[k]) for k in ref}
        print(name, {k: round(v, 4) for k, v in row.items()})
        for k, v in row.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst fraction of the bar:", {k: round(v, 4) for k, v in worst.items()})
