"""The multi-interest kernels (csrc/capsule.hip) alone on the GPU against float64 autograd of the formulas: ComirecDR's
position-batched projection, the three routing rounds, the hard readout.

Bar: the project's 1e-4 max(1e-2, max |ref|) per tensor; every case runs twice and must give the same bits.
Projection shapes from rp_capsule_geometry (64 batch rows and 128 output columns per workgroup, 32 per wave; the backward's
contraction staged in chunks of 64; dW's batch split above 512 rows): B = 1, 63, 64, 65 and 1025 (three splits of 384 rows, the
last one short, a chunk of one row in it); L = 1, 2, 3; K D = 8, 40 (no multiple of 32), 150 (one full tile and a
partial one), 256, 2048 (the largest); D = 6, 16, 64, 100, 128.
Routing: B = 1, 3, 70; L = 1, 2, 7, 33; K = 1, 2, 4, 8; D = 8, 20, 64, 100, 128; rows read per interest (stride D) and shared
(stride 0); initial logits absent and given; stop_grad; masks full (row 0), a single valid position (row 1), fully masked
(row 2: exact zeros), a hole inside (row 3), padded tails (the rest); one case whose rows are scaled until |U v| passes 15
and the softmax saturates — torch's own fp32 formulation on the CPU stays under a quarter of the bar there (asserted)."""
import functools

import pytest
import torch

from conftest import require_gpu
from test_capsule_host import route64

pytestmark = pytest.mark.gpu


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.detach().abs().max()))


def frac(got, ref):
    return float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max()) / bar(ref)


def check(tag, got, ref):
    for k in ref:
        print(f"{tag}: {k}: {frac(got[k], ref[k]):.3f} of the bar {bar(ref[k]):.3g}")
    for k in ref:
        assert got[k].shape == ref[k].shape and frac(got[k], ref[k]) <= 1.0, (tag, k, frac(got[k], ref[k]))


# ---- (a) projection ---------------------------------------------------------------------------------------------------------
PROJECT = [(1, 1, 8, 6), (63, 3, 40, 64), (64, 3, 256, 100), (65, 1, 150, 128), (33, 2, 2048, 16), (65, 3, 256, 64),
           (1025, 2, 40, 16)]


def project_run(B, L, N, D, dtype, device):
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(B * 100000 + L * 10000 + N * 10 + D)
    x = torch.randn(B, L, D, generator=gen).to(dtype).to(device).requires_grad_(True)
    w = (torch.randn(1, L, N, D, generator=gen) * (2.0 / D) ** 0.5).to(dtype).to(device).requires_grad_(True)
    g = torch.randn(B, L, N, generator=gen).to(dtype).to(device)
    if device == "cpu":
        u = torch.einsum("lnd,bld->bln", w[0], x)  # (the formula itself: no [B, L, N, D] product in the test either)
    else:
        u = Fh.capsule_project(x, w)
    (u * g).sum().backward()
    return {"U": u.detach().cpu(), "dX": x.grad.cpu(), "dW": w.grad.cpu()}


@pytest.mark.parametrize("B,L,N,D", PROJECT)
def test_projection_against_float64_and_bit_identical(B, L, N, D):
    require_gpu()
    from rec_pangu_amd import hip
    geo = hip.capsule_geometry()
    assert (geo["proj_tb"], geo["proj_tn"]) == (64, 128)  # the shapes above are chosen around these
    ref = project_run(B, L, N, D, torch.float64, "cpu")
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = project_run(B, L, N, D, torch.float32, "cuda")
    split = hip.capsule_workspace_bytes(B, L, N, D) > 0  # (above 512 rows dW's batch is split: a second launch adds the parts)
    assert split == (B > 512) and hip.launch_count() == n0 + 3 + split and hip.torch_path_count() == t0  # forward, dX, dW
    check(f"project {B}x{L}x{N}x{D}", got, ref)
    again = project_run(B, L, N, D, torch.float32, "cuda")
    for k in got:
        assert torch.equal(got[k], again[k]), k


# ---- (b) routing ------------------------------------------------------------------------------------------------------------
#        name              (B, L, K, D, shared, b0, stop_grad, scale)
ROUTE = {
    "b1_l1_k1_d8":         (1, 1, 1, 8, False, False, False, 0.5),
    "b3_l2_k2_d20_sh":     (3, 2, 2, 20, True, True, False, 0.5),
    "b70_l7_k4_d64":       (70, 7, 4, 64, False, True, False, 0.5),
    "b70_l7_k4_d64_sh":    (70, 7, 4, 64, True, False, False, 0.5),
    "b3_l33_k8_d64_sh":    (3, 33, 8, 64, True, True, False, 0.5),
    "b70_l33_k4_d100":     (70, 33, 4, 100, False, False, False, 0.5),
    "b3_l33_k4_d128":      (3, 33, 4, 128, False, True, False, 0.5),
    "b5_l7_k2_d128_sh_sg": (5, 7, 2, 128, True, True, True, 0.5),
    "b70_l7_k8_d20_sg":    (70, 7, 8, 20, False, True, True, 0.5),
    "b1_l7_k1_d20_sh":     (1, 7, 1, 20, True, False, False, 0.5),
    "b5_l7_k2_d20_sat":    (5, 7, 2, 20, False, True, False, 6.0),
}


@functools.lru_cache(maxsize=None)
def route_inputs(name):
    B, L, K, D, shared, has_b0, stop_grad, scale = ROUTE[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    u = torch.randn(B, L, D if shared else K * D, generator=gen) * scale
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    mask = (torch.arange(L)[None] < lens[:, None]).long()
    mask[0] = 1                                   # full
    if B > 1:
        mask[1] = 0
        mask[1, min(1, L - 1)] = 1                # a single valid position
    if B > 2:
        mask[2] = 0                               # fully masked
    if B > 3 and L > 2:
        mask[3] = 1
        mask[3, 1] = 0                            # a hole inside
    b0 = torch.randn(B, K, L, generator=gen) if has_b0 else None
    g = torch.randn(B, K, D, generator=gen)
    return u, mask, b0, g


def route_run(name, dtype, device, formulas=False):
    """formulas: float64 autograd of the formulas as tests/test_capsule_host.py states them; otherwise Fh.capsule_route (on
    the CPU the reference's torch formulation, on the device the kernels)"""
    from rec_pangu_amd import functional as Fh
    B, L, K, D, shared, has_b0, stop_grad, scale = ROUTE[name]
    u, mask, b0, g = route_inputs(name)
    leaf = u.detach().clone().to(dtype).to(device).requires_grad_(True)  # (a fresh leaf: route_inputs is cached)
    b0 = None if b0 is None else b0.to(dtype).to(device)
    if formulas:
        U = leaf[:, None].expand(B, K, L, D) if shared else leaf.view(B, L, K, D).permute(0, 2, 1, 3)
        out = route64(U, mask, b0 if b0 is not None else torch.zeros(B, K, L, dtype=dtype), stop_grad)
    else:
        out = Fh.capsule_route(leaf, mask.to(device), K, b0=b0, shared=shared, stop_grad=stop_grad)
    (out * g.to(dtype).to(device)).sum().backward()
    return {"out": out.detach().cpu(), "dU": leaf.grad.cpu()}


@functools.lru_cache(maxsize=None)
def route_reference(name):
    return route_run(name, torch.float64, "cpu", formulas=True)


@pytest.mark.parametrize("name", list(ROUTE))
def test_routing_against_float64_and_bit_identical(name):
    require_gpu()
    from rec_pangu_amd import hip
    B, L, K, D, shared, has_b0, stop_grad, scale = ROUTE[name]
    u, mask, b0, g = route_inputs(name)
    assert hip.capsule_route_fits(K, L, D)
    ref = route_reference(name)
    fair = max(frac(v, ref[k]) for k, v in route_run(name, torch.float32, "cpu").items())
    print(f"route {name}: torch's fp32 formulation on the CPU at {fair:.3f} of the bar")
    assert fair < 0.25, (name, fair)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = route_run(name, torch.float32, "cuda")
    assert hip.launch_count() == n0 + 2 and hip.torch_path_count() == t0  # one launch each way
    check(f"route {name}", got, ref)
    if B > 2:  # the fully masked row: exact zeros, forward and backward
        assert int(mask[2].sum()) == 0 and float(got["out"][2].abs().max()) == 0.0 and float(got["dU"][2].abs().max()) == 0.0
    assert float(got["out"][0].abs().max()) > 0
    again = route_run(name, torch.float32, "cuda")
    for k in got:
        assert torch.equal(got[k], again[k]), (name, k)


def test_the_saturating_case_saturates():
    """|U v| passes 15 and the largest routing weight of round 2 is 1 to fp32 precision in some (b, k) (CPU, float64)"""
    name = "b5_l7_k2_d20_sat"
    B, L, K, D, shared, has_b0, stop_grad, scale = ROUTE[name]
    u, mask, b0, g = route_inputs(name)
    U = u.double().view(B, L, K, D).permute(0, 2, 1, 3)
    b, big = b0.double(), 0.0
    for i in range(2):
        c = torch.softmax(b, -1) * (mask != 0)[:, None, :]
        s = torch.einsum("bkl,bkld->bkd", c, U)
        n = (s * s).sum(-1, keepdim=True)
        delta = torch.einsum("bkld,bkd->bkl", U, s * n / (1 + n) / torch.sqrt(n + 1e-9))
        big = max(big, float(delta.abs().max()))
        b = b + delta
    assert big > 15 and float(torch.softmax(b, -1).max()) > 1 - 1e-7, (big, float(torch.softmax(b, -1).max()))


def test_stop_grad_cuts_rounds_0_and_1():
    """the same forward, another gradient — and with stop_grad the gradient is round 2's alone: c_2 ds_2^T"""
    require_gpu()
    from rec_pangu_amd import functional as Fh
    u, mask, b0, g = route_inputs("b70_l7_k8_d20_sg")
    res = {}
    for sg in (True, False):
        leaf = u.cuda().requires_grad_(True)
        out = Fh.capsule_route(leaf, mask.cuda(), 8, b0=b0.cuda(), stop_grad=sg)
        (out * g.cuda()).sum().backward()
        res[sg] = (out.detach().cpu(), leaf.grad.cpu())
    assert torch.equal(res[True][0], res[False][0]) and not torch.equal(res[True][1], res[False][1])


def test_saved_between_forward_and_backward():
    """routing: the projected rows, the mask and the initial logits, nothing else; projection: its two inputs; readout: one
    int32 per row"""
    require_gpu()
    from rec_pangu_amd import functional as Fh
    B, L, K, D, V = 9, 5, 3, 8, 11
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, L, D, generator=gen).cuda().requires_grad_(True)
    w = torch.randn(1, L, K * D, D, generator=gen).cuda().requires_grad_(True)
    mask, b0 = torch.ones(B, L, dtype=torch.long).cuda(), torch.randn(B, K, L, generator=gen).cuda()
    u = Fh.capsule_project(x, w)
    kept = [t for t in u.grad_fn.saved_tensors if t is not None]
    assert sorted(t.numel() for t in kept) == sorted([x.numel(), w.numel()])
    out = Fh.capsule_route(u, mask, K, b0=b0)
    kept = [t for t in out.grad_fn.saved_tensors if t is not None]
    assert sorted(t.numel() for t in kept) == sorted([u.numel(), mask.numel(), b0.numel()])
    plain = Fh.capsule_route(u, mask, K)  # (no logits: two tensors, and the rows are u itself, not a copy)
    kept = [t for t in plain.grad_fn.saved_tensors if t is not None]
    assert len(kept) == 2 and kept[0].data_ptr() == u.data_ptr()
    best = Fh.interest_pick(out, torch.randn(V, D, generator=gen).cuda(), torch.randint(0, V, (B,), generator=gen).cuda())
    kept = [t for t in best.grad_fn.saved_tensors if t is not None]
    assert len(kept) == 1 and kept[0].dtype == torch.int32 and kept[0].shape == (B,)


def test_comirecdr_never_holds_the_product():
    """(B, L, K, D) = (64, 8, 4, 64): the peak over forward + backward above the inputs stays under a quarter of the
    [B, L, K D, D] product's bytes — the product is D = 64 times the projected rows, so the bar is 16 of them"""
    require_gpu()
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.sequence import ComirecDR
    B, L, K, D, V = 64, 8, 4, 64, 500
    torch.manual_seed(0)
    model = ComirecDR({"item_id": {"vocab_size": V}}, {"embedding_dim": D, "max_length": L, "device": "cuda:0", "K": K,
                                                       "item_col": "item_id", "cate_cols": []}).cuda()
    gen = torch.Generator().manual_seed(1)
    batch = {"hist_item_list": torch.randint(1, V, (B, L), generator=gen).cuda(),
             "hist_mask_list": torch.ones(B, L, dtype=torch.long).cuda(),
             "target_item": torch.randint(0, V, (B, 1), generator=gen).cuda()}
    model(batch)["loss"].backward()  # (warm: the library, the flag word, the sort's buffers)
    model.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base, t0 = torch.cuda.memory_allocated(), hip.torch_path_count()
    model(batch)["loss"].backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    product = 4 * B * L * K * D * D
    print(f"ComirecDR {B}x{L}x{K}x{D}: peak {peak} bytes above the inputs = {peak / (product / D):.2f} projected-row tensors; "
          f"the product would be {product}")
    assert hip.torch_path_count() == t0 and 0 < peak < product // 4


# ---- (c) readout ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pick_inputs(B, K, D, V):
    """interests, table and targets whose float64 scores have a top-two gap of at least 1e-3 max |score| in EVERY row
    (asserted: no row is left out); rows that miss it are redrawn; targets 0 and V - 1 are there"""
    gen = torch.Generator().manual_seed(B * 1000 + K * 100 + D)
    inter, E = torch.randn(B, K, D, generator=gen), torch.randn(V, D, generator=gen)
    t = torch.randint(0, V, (B,), generator=gen)
    t[0], t[-1] = 0, V - 1

    def gaps():
        s = torch.bmm(inter.double(), E.double()[t].unsqueeze(-1)).squeeze(-1)
        top = torch.sort(s, dim=1, descending=True).values
        return s, (top[:, 0] - top[:, 1]) if K > 1 else torch.full((B,), float("inf"), dtype=torch.float64)

    for _ in range(100):
        s, gap = gaps()
        bad = gap < 2e-3 * float(s.abs().max())
        if not bool(bad.any()):
            break
        inter[bad] = torch.randn(int(bad.sum()), K, D, generator=gen)
    s, gap = gaps()
    assert float(gap.min()) >= 1e-3 * float(s.abs().max())
    return inter, E, t, torch.argmax(s, dim=1), torch.randn(B, D, generator=gen)


@pytest.mark.parametrize("B,K,D,V", [(1, 1, 8, 3), (70, 4, 20, 41), (5, 3, 130, 7), (33, 8, 64, 41)])
def test_pick_against_float64_argmax(B, K, D, V):
    require_gpu()
    from rec_pangu_amd import functional as Fh, hip
    inter, E, t, kk, g = pick_inputs(B, K, D, V)
    n0 = hip.launch_count()
    leaf = inter.cuda().requires_grad_(True)
    best = Fh.interest_pick(leaf, E.cuda(), t.cuda())
    assert torch.equal(best.grad_fn.saved_tensors[0].cpu(), kk.to(torch.int32))
    (best * g.cuda()).sum().backward()
    assert hip.launch_count() == n0 + 2
    assert torch.equal(best.detach().cpu(), inter[torch.arange(B), kk])  # a copy of the chosen row: the same bits
    want = torch.zeros(B, K, D)
    want[torch.arange(B), kk] = g
    assert torch.equal(leaf.grad.cpu(), want)  # exact zeros off the chosen interest


def test_pick_takes_the_lower_of_two_identical_interests():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    inter, E, t, kk, g = pick_inputs(70, 4, 20, 41)
    inter = inter.clone()
    for b, (lo, hi) in {3: (0, 2), 7: (1, 3), 11: (2, 3)}.items():
        inter[b, lo] = inter[b, hi] = 50.0 * E[t[b]]  # two bit-identical rows, far above the rest
    leaf = inter.cuda().requires_grad_(True)
    best = Fh.interest_pick(leaf, E.cuda(), t.cuda())
    k = best.grad_fn.saved_tensors[0].cpu()
    assert (int(k[3]), int(k[7]), int(k[11])) == (0, 1, 2)
    best.sum().backward()
    assert float(leaf.grad[3, 2].abs().max()) == 0.0 and float(leaf.grad[3, 0].min()) == 1.0


def test_pick_raises_for_a_target_outside_the_table_and_reads_row_0():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    inter, E, t, kk, g = pick_inputs(70, 4, 20, 41)
    bad, zero = t.clone(), t.clone()
    bad[5], zero[5] = 41, 0
    with torch.no_grad():
        want = Fh.interest_pick(inter.cuda(), E.cuda(), zero.cuda())
        got = Fh.interest_pick(inter.cuda(), E.cuda(), bad.cuda(), check_indices="deferred")
        assert torch.equal(got, want)
        with pytest.raises(IndexError):
            Fh.interest_pick(inter.cuda(), E.cuda(), bad.cuda())
        bad[5] = -1
        with pytest.raises(IndexError):
            Fh.interest_pick(inter.cuda(), E.cuda(), bad.cuda())
        Fh.interest_pick(inter.cuda(), E.cuda(), zero.cuda())  # (the flag was cleared)


# ---- outside the geometry ---------------------------------------------------------------------------------------------------
def test_a_size_outside_the_geometry_takes_the_torch_path_and_says_so_once():
    require_gpu()
    import warnings
    from rec_pangu_amd import functional as Fh, hip
    B, L, K, D = 4, 70, 2, 8  # L above the 64 positions a wave holds
    assert not hip.capsule_route_fits(K, L, D)
    gen = torch.Generator().manual_seed(0)
    u = torch.randn(B, L, K * D, generator=gen)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, 3:] = 0
    t0 = hip.torch_path_count()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            leaf = u.cuda().requires_grad_(True)
            out = Fh.capsule_route(leaf, mask.cuda(), K)
    assert hip.torch_path_count() == t0 + 2 and len([w for w in seen if "capsule_route at K=2, L=70" in str(w.message)]) == 1
    out.sum().backward()
    U = u.double().view(B, L, K, D).permute(0, 2, 1, 3)
    ref = route64(U, mask, torch.zeros(B, K, L, dtype=torch.float64))
    assert out.is_cuda and frac(out, ref) <= 1.0 and bool(torch.isfinite(leaf.grad).all())
