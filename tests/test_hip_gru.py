"""The GRU recurrence kernels (csrc/gru.hip) and NARM's attention readout (csrc/narm.hip) alone on the GPU, against a float64
torch nn.GRU with the same weights.

Bar: the project's 1e-4 max(1e-2, max |ref|) per tensor (H_all, h_last, every dW / db, dX or dE).  Weights at kaiming scale
(std sqrt(2 / fan_in)), biases as nn.GRU draws them, inputs and table rows from N(0, 1), the arriving gradients from N(0, 1).
Shapes from rp_gru_geometry (TB = 32 rows per workgroup, 32 hidden columns per wave, contraction padded to 32): B = TB - 1,
TB, TB + 1 and two tiles plus a partial one (70); L = 1, 2, 7; H = 8, 20, 32, 64, 100, 128 with in != H, in = 128 with H = 8,
in = 6; one, two and three layers; with and without biases; id and dense input; both residencies of the weights (LDS up to
in = H = 64, L2 above).

Before relying on a case: torch's own fp32 nn.GRU on the CPU against the float64 reference, worst tensor, as a fraction of the
bar (test_the_cases_are_fair recomputes and asserts < 0.25):
  b31_l1_in6_h8 0.002   b32_l2_h20 0.004   b33_l7_h32_x3 0.005   b70_l7_h64_full 0.006   b33_l7_h100_full 0.009
  b33_l7_h128 0.010     b33_l2_in128_h8 0.007
"""
import functools

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu

#        name                (B, L, in, H, layers, bias, mode,     ids)
CASES = {
    "b31_l1_in6_h8":    (31, 1, 6, 8, 1, True, "packed", False),     # B = TB - 1, L = 1, no dwordx4 width, all lengths 1
    "b32_l2_h20":       (32, 2, 12, 20, 2, True, "packed", True),    # B = TB, mixed lengths
    "b33_l7_h32_x3":    (33, 7, 16, 32, 3, True, "packed0", True),   # B = TB + 1, three layers, one length 0
    "b70_l7_h64_full":  (70, 7, 40, 64, 2, False, "full", True),     # two tiles + a partial one, no biases, last = -1 / 0 / L - 1
    "b33_l7_h100_full": (33, 7, 64, 100, 2, True, "full", False),    # weights stay in L2 (Hp = 128)
    "b33_l7_h128":      (33, 7, 100, 128, 1, True, "packedL", False),  # the largest H, every length L
    "b33_l2_in128_h8":  (33, 2, 128, 8, 2, False, "packed", True),   # the widest input into the narrowest state
}
V = 41


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def frac(got, ref):
    return float((got.detach().cpu().double() - ref.double()).abs().max()) / bar(ref)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """everything of a case on the CPU in fp32: (rnn, E, ids, X, steps, last, G_all, G_last)"""
    B, L, n_in, H, layers, bias, mode, use_ids = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    torch.manual_seed(sum(map(ord, name)))
    rnn = torch.nn.GRU(n_in, H, layers, bias=bias, batch_first=True)
    for k, p in rnn.named_parameters():
        if p.dim() == 2:
            with torch.no_grad():
                p.copy_(torch.randn(p.shape, generator=gen) * (2.0 / p.shape[1]) ** 0.5)
    E = torch.randn(V, n_in, generator=gen)
    ids = torch.randint(1, V, (B, L), generator=gen)
    X = torch.randn(B, L, n_in, generator=gen)
    if mode == "full":
        steps = torch.full((B,), L)
        last = torch.randint(0, L, (B,), generator=gen)
        last[0], last[1], last[2] = -1, 0, L - 1
    else:
        steps = torch.randint(1, L + 1, (B,), generator=gen)
        if mode == "packedL":
            steps[:] = L
        steps[0], steps[1] = 1, L
        if mode == "packed0":
            steps[5] = 0
        last = steps - 1
    if use_ids:
        ids[:, 0] = 5                         # a hot id in every row
        if L > 2:
            ids[3, 1], steps[3] = 0, max(int(steps[3]), 3)  # an id 0 inside a sequence
            if mode != "full":
                last[3] = steps[3] - 1
            ids[4, -2:] = 0                   # a padded tail
            if mode != "full":
                steps[4], last[4] = L - 2, L - 3
    G_all = torch.randn(B, L, H, generator=gen)
    G_last = torch.randn(B, H, generator=gen)
    return rnn, E, ids, X, steps, last, G_all, G_last


def torch_run(name, dtype):
    """torch's nn.GRU in `dtype` on the CPU -> {tensor name: value}: H_all, h_last and every gradient"""
    B, L, n_in, H, layers, bias, mode, use_ids = CASES[name]
    rnn, E, ids, X, steps, last, G_all, G_last = inputs(name)
    net = torch.nn.GRU(n_in, H, layers, bias=bias, batch_first=True).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in rnn.state_dict().items()})
    leaf = (E if use_ids else X).to(dtype).clone().requires_grad_(True)
    x = torch.nn.functional.embedding(ids, leaf, padding_idx=0) if use_ids else leaf
    out, _ = net(x)  # (causal: the first steps[b] outputs of the full walk are the packed walk's)
    live = (torch.arange(L)[None, :] < steps[:, None]).to(dtype).unsqueeze(-1)
    h_all = out * live
    ok = ((last >= 0) & (last < steps)).to(dtype).unsqueeze(-1)
    h_last = h_all.gather(1, last.clamp(min=0).view(-1, 1, 1).expand(-1, 1, H)).squeeze(1) * ok
    ((h_all * G_all.to(dtype)).sum() + (h_last * G_last.to(dtype)).sum()).backward()
    res = {"H_all": h_all.detach(), "h_last": h_last.detach(), ("dE" if use_ids else "dX"): leaf.grad}
    res.update({"d" + k: p.grad for k, p in net.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def reference(name):
    return torch_run(name, torch.float64)


def device_run(name, freeze_input=False):
    from rec_pangu_amd import functional as Fh
    B, L, n_in, H, layers, bias, mode, use_ids = CASES[name]
    rnn, E, ids, X, steps, last, G_all, G_last = inputs(name)
    net = torch.nn.GRU(n_in, H, layers, bias=bias, batch_first=True)
    net.load_state_dict(rnn.state_dict())
    net = net.cuda()
    leaf = (E if use_ids else X).cuda().requires_grad_(not freeze_input)
    kw = dict(ids=ids.cuda(), item_weight=leaf) if use_ids else dict(x=leaf)
    h_all, h_last = Fh.gru_encode(net, steps.cuda(), last.cuda(), packed=mode != "full", **kw)
    kept = sum(t.numel() for t in h_all.grad_fn.saved_tensors if t is not None and t.dtype == torch.float32)
    ((h_all * G_all.cuda()).sum() + (h_last * G_last.cuda()).sum()).backward()
    res = {"H_all": h_all.detach().cpu(), "h_last": h_last.detach().cpu(),
           ("dE" if use_ids else "dX"): None if leaf.grad is None else leaf.grad.cpu()}
    res.update({"d" + k: p.grad.cpu() for k, p in net.named_parameters()})
    return res, kept - sum(p.numel() for p in net.parameters()) - leaf.numel()


def test_the_cases_are_fair():
    """torch's own fp32 nn.GRU stays under a quarter of the bar on every case (CPU only: no kernel runs here)"""
    for name in CASES:
        ref, got = reference(name), torch_run(name, torch.float32)
        worst = max(frac(got[k], ref[k]) for k in ref)
        print(f"{name}: torch fp32 at {worst:.3f} of the bar")
        assert worst < 0.25, (name, worst)


@pytest.mark.parametrize("name", list(CASES))
def test_gru_against_float64_and_bit_identical(name):
    require_gpu()
    from rec_pangu_amd import hip
    B, L, n_in, H, layers, bias, mode, use_ids = CASES[name]
    rnn, E, ids, X, steps, last, G_all, G_last = inputs(name)
    ref = reference(name)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got, kept = device_run(name)
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0
    assert set(got) == set(ref)
    for k in ref:
        f = frac(got[k], ref[k])
        print(f"{name}: {k}: {f:.3f} of the bar {bar(ref[k]):.3g}")
    for k in ref:
        assert got[k].shape == ref[k].shape and frac(got[k], ref[k]) <= 1.0, (name, k, frac(got[k], ref[k]))
    # exact zeros: behind steps[b], the empty row, the padding row's gradient
    dead = torch.arange(L)[None, :] >= steps[:, None]
    assert float(got["H_all"][dead].abs().sum()) == 0.0
    gone = (last < 0) | (last >= steps)
    assert float(got["h_last"][gone].abs().sum()) == 0.0
    if mode == "packed0":
        assert int(steps[5]) == 0 and float(got["h_last"][5].abs().max()) == 0.0 and float(got["H_all"][5].abs().max()) == 0.0
    if mode == "full":
        assert bool(gone[0]) and torch.equal(got["h_last"][1], got["H_all"][1, 0]) and torch.equal(got["h_last"][2], got["H_all"][2, -1])
    if use_ids:
        assert float(got["dE"][0].abs().max()) == 0.0
        if L > 2:
            assert int(ids[3, 1]) == 0 and int(steps[3]) > 1 and bool((ids[4, -2:] == 0).all()) and bool((ids == 5).any(1).all())
    # the only state kept between forward and backward: the hidden states, layers * B * L * H floats
    assert kept == layers * B * L * H
    again, _ = device_run(name)
    for k in got:
        assert torch.equal(got[k], again[k]), (name, k)  # two runs, the same bits


def test_an_id_outside_the_table_raises_and_reads_row_0():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    rnn, E, ids, X, steps, last, _, _ = inputs("b32_l2_h20")
    net = torch.nn.GRU(12, 20, 2, batch_first=True)
    net.load_state_dict(rnn.state_dict())
    net = net.cuda()
    bad, zero = ids.clone(), ids.clone()
    bad[2, 0], zero[2, 0] = V, 0
    with torch.no_grad():
        want = Fh.gru_encode(net, steps.cuda(), last.cuda(), ids=zero.cuda(), item_weight=E.cuda())
        got = Fh.gru_encode(net, steps.cuda(), last.cuda(), ids=bad.cuda(), item_weight=E.cuda(), check_indices="deferred")
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        with pytest.raises(IndexError):
            Fh.gru_encode(net, steps.cuda(), last.cuda(), ids=bad.cuda(), item_weight=E.cuda())
        Fh.gru_encode(net, steps.cuda(), last.cuda(), ids=zero.cuda(), item_weight=E.cuda())  # (the flag was cleared)


def test_a_gradient_nobody_needs_is_not_computed():
    require_gpu()
    from rec_pangu_amd import hip
    name = "b32_l2_h20"
    n0 = hip.launch_count()
    full, _ = device_run(name)
    n1 = hip.launch_count()
    frozen, _ = device_run(name, freeze_input=True)
    n2 = hip.launch_count()
    assert frozen["dE"] is None and n2 - n1 < n1 - n0  # no sort, no reduction into the table
    for k in full:
        if k != "dE":
            assert torch.equal(full[k], frozen[k]), k


def test_widths_above_the_kernels_take_the_torch_path_and_say_so_once():
    require_gpu()
    import warnings
    from rec_pangu_amd import functional as Fh, hip
    net = torch.nn.GRU(9, 160, 1, batch_first=True).cuda()
    x = torch.randn(3, 4, 9, device="cuda")
    steps = torch.tensor([4, 2, 1], device="cuda")
    t0 = hip.torch_path_count()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            h_all, h_last = Fh.gru_encode(net, steps, steps - 1, x=x)
    assert hip.torch_path_count() == t0 + 2 and len([w for w in seen if "gru_encode at in=9, H=160" in str(w.message)]) == 1
    want, _ = net(x)
    assert h_all.shape == (3, 4, 160) and torch.allclose(h_last[0], want[0, 3]) and float(h_all[1, 2:].detach().abs().sum()) == 0.0


# ---- NARM's attention readout alone -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narm_inputs(B, L, H):
    gen = torch.Generator().manual_seed(B * 1000 + L * 10 + H)
    t = {k: torch.randn(*s, generator=gen) for k, s in
         (("q1", (B, L, H)), ("q2", (B, H)), ("v", (1, H)), ("G", (B, L, H)), ("ht", (B, H)), ("dout", (B, 2 * H)))}
    ids = torch.randint(0, 3, (B, L), generator=gen)
    ids[0] = 0  # a row whose mask is all zero
    if B > 1:
        ids[1] = 1
    t["v"] = t["v"] * (2.0 / H) ** 0.5
    return t, ids


def narm_run(B, L, H, dtype, device):
    from rec_pangu_amd import functional as Fh
    t, ids = narm_inputs(B, L, H)
    leaves = {k: t[k].detach().clone().to(dtype).to(device).requires_grad_(True) for k in ("q1", "q2", "v", "G", "ht")}
    out = Fh.narm_attention(leaves["q1"], leaves["q2"], leaves["v"], ids.to(device), leaves["G"], leaves["ht"])
    (out * t["dout"].to(dtype).to(device)).sum().backward()
    res = {"out": out.detach().cpu()}
    res.update({"d" + k: p.grad.cpu() for k, p in leaves.items()})
    return res


@pytest.mark.parametrize("B,L,H", [(1, 1, 4), (67, 7, 12), (33, 5, 128)])
def test_narm_attention_against_float64_and_bit_identical(B, L, H):
    """torch's fp32 formula on the CPU against float64, worst tensor: 0.000, 0.008, 0.003 of the bar (asserted < 0.25)"""
    require_gpu()
    ref = narm_run(B, L, H, torch.float64, "cpu")
    fair = max(frac(v, ref[k]) for k, v in narm_run(B, L, H, torch.float32, "cpu").items())
    assert fair < 0.25, fair
    got = narm_run(B, L, H, torch.float32, "cuda")
    for k in ref:
        print(f"narm {B}x{L}x{H}: {k}: {frac(got[k], ref[k]):.3f} of the bar (torch fp32 worst {fair:.3f})")
    for k in ref:
        assert got[k].shape == ref[k].shape and frac(got[k], ref[k]) <= 1.0, (k, frac(got[k], ref[k]))
    assert float(got["out"][0, :H].abs().max()) == 0.0 and float(got["dq1"][0].abs().max()) == 0.0  # the all-zero mask row
    again = narm_run(B, L, H, torch.float32, "cuda")
    for k in got:
        assert torch.equal(got[k], again[k]), k  # dv included: a fixed-order two-stage sum
