"""The masked multi-head attention core and the feed-forward activations (csrc/seq_attn.hip) alone on the GPU against float64
autograd of tests/test_sasrec_host.attention_f64 (checked there against torch's composed formulation).

Bar: the project's 1e-4 max(1e-2, max |ref|) per tensor (ctx, dqkv); every case runs twice and must give the same bits; one
library launch each way, no torch path.  Shapes around rp_seq_attn_geometry (64 query rows per wave, L <= 128; head widths
rounded up to 4, 8, 16, 32, 64 registers, dh <= 64): B = 1, 3, 70; L = 1, 2, 7, 33, 64, 65, 128; dh = 1, 4, 16, 20, 64; heads
= 1, 2, 4; L = 129 and dh = 65 take the counted torch path.  Masks: full, length 1, padded tails, a hole inside, with
mask[:, 0] = 1 in every compared row, so that every query has a visible key (a query without one is quantised at the fp32 ulp
of 1e6 in the reference and is compared nowhere; one such row runs for finiteness).  Last-row mode at the same shapes against
row qpos[b] of the full float64 result, qpos = 0, L - 1 and -1 among them.  Dropout at p = 0.1 and 0.5 with the decisions read
back through rp_seq_attn_keep_mask and fed to the float64 reference; the same decisions byte for byte from rp_dropout_fwd."""
import functools
import math

import pytest
import torch

from conftest import require_gpu
from test_sasrec_host import attention_f64, composed_fp32, masks

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


#       (B, L, heads, dh)
SHAPES = [(1, 1, 1, 1), (3, 2, 2, 4), (70, 7, 4, 16), (3, 33, 2, 20), (3, 64, 1, 64), (70, 65, 2, 16), (3, 65, 4, 20),
          (3, 128, 4, 4), (1, 128, 1, 64), (3, 63, 2, 1)]


@functools.lru_cache(maxsize=None)
def inputs(B, L, heads, dh, scale=1.0):
    """(qkv [B L, 3 D], mask [B, L], g [B L, D], qpos [B]); the float64 reference of a shape is computed once (reference())"""
    gen = torch.Generator().manual_seed(B * 1000003 + L * 10007 + heads * 101 + dh)
    D = heads * dh
    qkv = torch.randn(B * L, 3 * D, generator=gen)
    qkv[:, :2 * D] *= scale
    mask = masks(B, L, gen)
    g = torch.randn(B * L, D, generator=gen)
    qpos = torch.randint(0, L, (B,), generator=gen)
    qpos[0] = L - 1
    if B > 1:
        qpos[1] = 0
    if B > 2:
        qpos[2] = -1
    return qkv, mask, g, qpos


@functools.lru_cache(maxsize=None)
def reference(B, L, heads, dh, scale=1.0):
    qkv, mask, g, _ = inputs(B, L, heads, dh, scale)
    x = qkv.double().requires_grad_(True)
    ctx = attention_f64(x, mask, heads)
    (ctx * g.double()).sum().backward()
    return {"ctx": ctx.detach(), "dqkv": x.grad}


def device_run(qkv, mask, g, heads, p=0.0, training=False, qpos=None, q=None):
    from rec_pangu_amd import functional as Fh
    x = qkv.to(DEV).requires_grad_(True)
    qd = None if q is None else q.to(DEV).requires_grad_(True)
    ctx = Fh.seq_attention(x, mask.to(DEV), heads, p=p, training=training, qpos=None if qpos is None else qpos.to(DEV), q=qd)
    (ctx * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    out = {"ctx": ctx.detach().cpu(), "dqkv": x.grad.cpu()}
    if qd is not None:
        out["dq"] = qd.grad.cpu()
    return out


@pytest.mark.parametrize("B,L,heads,dh", SHAPES)
def test_full_mode_against_float64_and_bit_identical(B, L, heads, dh):
    require_gpu()
    from rec_pangu_amd import hip
    geo = hip.seq_attn_geometry()
    assert (geo["row_tile"], geo["max_l"], geo["max_dh"], geo["min_dh_tile"]) == (64, 128, 64, 4)  # the shapes sit around these
    qkv, mask, g, _ = inputs(B, L, heads, dh)
    assert bool((mask[:, 0] != 0).all())
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = device_run(qkv, mask, g, heads)
    assert hip.launch_count() == n0 + 2 and hip.torch_path_count() == t0  # one launch each way
    check(f"full {B}x{L}x{heads}x{dh}", got, reference(B, L, heads, dh))
    again = device_run(qkv, mask, g, heads)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    with_p0 = device_run(qkv, mask, g, heads, p=0.0, training=True)
    for k in got:
        assert torch.equal(got[k], with_p0[k]), k


@pytest.mark.parametrize("B,L,heads,dh", SHAPES)
def test_last_row_mode_against_the_full_float64_result(B, L, heads, dh):
    require_gpu()
    from rec_pangu_amd import hip
    qkv, mask, g, qpos = inputs(B, L, heads, dh)
    D = heads * dh
    rows, pick = torch.arange(B), qpos.clamp(min=0)
    live = (qpos >= 0)
    x = qkv.double().requires_grad_(True)
    full = attention_f64(x, mask, heads).view(B, L, D)
    gl = g.view(B, L, D)[rows, pick]
    (full[rows, pick] * gl.double() * live[:, None]).sum().backward()
    ref = {"ctx": (full[rows, pick] * live[:, None]).detach(), "dqkv": x.grad}
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = device_run(qkv, mask, gl, heads, qpos=qpos)
    assert hip.launch_count() == n0 + 2 and hip.torch_path_count() == t0
    check(f"last {B}x{L}x{heads}x{dh}", got, ref)
    for b in (~live).nonzero().view(-1).tolist():  # no history: exact zeros, zero gradients
        assert float(got["ctx"][b].abs().max()) == 0.0 and float(got["dqkv"].view(B, L, -1)[b].abs().max()) == 0.0
    dq = got["dqkv"].view(B, L, 3 * D)[:, :, :D].clone()
    dq[rows[live], pick[live]] = 0
    assert float(dq.abs().max()) == 0.0  # only the selected query row takes a dQ
    again = device_run(qkv, mask, gl, heads, qpos=qpos)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    # the query rows handed over as [B, D]: the same bits
    compact = device_run(qkv[:, D:].contiguous(), mask, gl, heads, qpos=qpos, q=qkv.view(B, L, 3 * D)[rows, pick, :D].contiguous())
    assert torch.equal(compact["ctx"], got["ctx"]) and torch.equal(compact["dqkv"], got["dqkv"][:, D:])
    assert torch.equal(compact["dq"], got["dqkv"].view(B, L, 3 * D)[rows, pick, :D] * live[:, None])


@pytest.mark.parametrize("B,L,heads,dh", [(2, 129, 1, 8), (2, 8, 1, 65)])
def test_shapes_outside_the_limits_take_the_counted_torch_path(B, L, heads, dh):
    require_gpu()
    import warnings
    from rec_pangu_amd import hip
    assert not hip.seq_attn_fits(L, heads, dh)
    qkv, mask, g, qpos = inputs(B, L, heads, dh)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = device_run(qkv, mask, g, heads)
        last = device_run(qkv, mask, g.view(B, L, -1)[:, 0].contiguous(), heads, qpos=qpos.clamp(min=0))
    assert hip.launch_count() == n0 and hip.torch_path_count() == t0 + 2
    ref = reference(B, L, heads, dh)
    check(f"torch path {B}x{L}x{heads}x{dh}", got, ref)
    want = ref["ctx"].view(B, L, -1)[torch.arange(B), qpos.clamp(min=0)]
    assert frac(last["ctx"], want) <= 1.0


def test_a_saturated_softmax():
    """Q and K scaled until the largest probability of most rows passes 1 - 1e-6; torch's own fp32 formulation on the CPU
    stays under a quarter of the bar there (asserted first)"""
    require_gpu()
    B, L, heads, dh, scale = 5, 33, 2, 16, 6.0
    qkv, mask, g, _ = inputs(B, L, heads, dh, scale)
    ref = reference(B, L, heads, dh, scale)
    D = heads * dh
    s = torch.einsum("bihd,bjhd->bhij", qkv[:, :D].double().view(B, L, heads, dh), qkv[:, D:2 * D].double().view(B, L, heads, dh))
    assert float((s / math.sqrt(dh)).abs().max()) > 100  # scores far apart: the softmax is saturated
    x = qkv.clone().requires_grad_(True)
    ctx = composed_fp32(x, mask, heads)
    (ctx * g).sum().backward()
    own = {"ctx": ctx.detach(), "dqkv": x.grad}
    for k in ref:
        print(f"torch fp32 on the CPU: {k}: {frac(own[k], ref[k]):.3f} of the bar")
        assert frac(own[k], ref[k]) <= 0.25, k
    check("saturated", device_run(qkv, mask, g, heads), ref)


def test_a_query_without_a_visible_key_stays_finite():
    require_gpu()
    B, L, heads, dh = 3, 7, 2, 4
    qkv, mask, g, _ = inputs(B, L, heads, dh)
    mask = mask.clone()
    mask[1] = 0  # no content at all
    mask[2, 0] = 0  # padding in front: query 0 sees nothing
    got = device_run(qkv, mask, g, heads)
    assert bool(torch.isfinite(got["ctx"]).all()) and bool(torch.isfinite(got["dqkv"]).all())
    x = qkv.double().requires_grad_(True)
    ctx = attention_f64(x, mask, heads)
    assert frac(got["ctx"].view(B, L, -1)[0], ctx.view(B, L, -1)[0]) <= 1.0  # the rows that have a visible key are untouched
    assert frac(got["ctx"].view(B, L, -1)[2, 1:], ctx.view(B, L, -1)[2, 1:]) <= 1.0
    last = device_run(qkv, mask, g.view(B, L, -1)[:, 0].contiguous(), heads, qpos=torch.tensor([L - 1, L - 1, 0]))
    assert bool(torch.isfinite(last["ctx"]).all()) and bool(torch.isfinite(last["dqkv"]).all())


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,L,heads,dh", [(70, 33, 2, 16), (3, 128, 4, 4), (5, 65, 1, 20)])
def test_attention_dropout(B, L, heads, dh, p):
    require_gpu()
    from rec_pangu_amd import hip
    qkv, mask, g, qpos = inputs(B, L, heads, dh)
    D = heads * dh
    torch.manual_seed(1000 + int(p * 10))
    gen = hip.device_generator(torch.device(DEV))
    seed, off = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, gen.get_offset()
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = device_run(qkv, mask, g, heads, p=p, training=True)
    assert hip.launch_count() == n0 + 2 and hip.torch_path_count() == t0
    assert gen.get_offset() == off + 4  # one call, one offset (torch's granularity is 4)
    keep = hip.seq_attn_keep_mask(B, heads, L, p, seed, off, torch.device(DEV)).cpu()
    assert keep.shape == (B, heads, L, L) and keep.dtype == torch.uint8 and set(keep.unique().tolist()) <= {0, 1}
    x = qkv.double().requires_grad_(True)
    ctx = attention_f64(x, mask, heads, keep, p)
    (ctx * g.double()).sum().backward()
    check(f"dropout {p} {B}x{L}x{heads}x{dh}", got, {"ctx": ctx.detach(), "dqkv": x.grad})
    # the same (seed, offset): the same bits; the next offset: another mask
    gen.set_offset(off)
    again = device_run(qkv, mask, g, heads, p=p, training=True)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    assert torch.equal(keep, hip.seq_attn_keep_mask(B, heads, L, p, seed, off, torch.device(DEV)).cpu())
    other = hip.seq_attn_keep_mask(B, heads, L, p, seed, off + 4, torch.device(DEV)).cpu()
    assert not torch.equal(keep, other)
    moved = device_run(qkv, mask, g, heads, p=p, training=True)  # (the generator now stands at off + 4)
    assert not torch.equal(moved["ctx"], got["ctx"])
    # the kept share over the visible entries
    visible = ((mask != 0)[:, None, None, :] & torch.ones(L, L, dtype=torch.bool).tril()[None, None]).expand(B, heads, L, L)
    n = int(visible.sum())
    share = float(keep[visible].double().mean())
    print(f"kept share {share:.5f} over {n} visible entries, 1 - p = {1 - p}")
    assert abs(share - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)
    # last-row mode draws row qpos[b] of the same decisions
    rows, pick, live = torch.arange(B), qpos.clamp(min=0), (qpos >= 0)
    gl = g.view(B, L, D)[rows, pick]
    gen.set_offset(off)
    last = device_run(qkv, mask, gl, heads, p=p, training=True, qpos=qpos)
    x = qkv.double().requires_grad_(True)
    full = attention_f64(x, mask, heads, keep, p).view(B, L, D)
    (full[rows, pick] * gl.double() * live[:, None]).sum().backward()
    check(f"dropout {p} last row", last, {"ctx": (full[rows, pick] * live[:, None]).detach(), "dqkv": x.grad})
    # p = 0 in training mode: the bits of a call without dropout, and no offset taken
    off2 = gen.get_offset()
    plain, p0 = device_run(qkv, mask, g, heads), device_run(qkv, mask, g, heads, p=0.0, training=True)
    assert gen.get_offset() == off2 and all(torch.equal(plain[k], p0[k]) for k in plain)


@pytest.mark.parametrize("name", ["gelu", "swish"])
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_seq_act_against_float64(name, N):
    require_gpu()
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    M = 37
    gen = torch.Generator().manual_seed(N)
    x = (torch.rand(M, N, generator=gen) * 16 - 8)
    x.view(-1)[:4] = torch.tensor([-8.0, 8.0, 0.0, 1e-3])[:min(4, M * N)]
    g = torch.randn(M, N, generator=gen)
    x64 = x.double().requires_grad_(True)
    y64 = x64 * 0.5 * (1.0 + torch.erf(x64 / math.sqrt(2.0))) if name == "gelu" else x64 * torch.sigmoid(x64)
    (y64 * g.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    yd = Fh.seq_act(xd, name)
    (yd * g.to(DEV)).sum().backward()
    assert hip.launch_count() == n0 + 2 and hip.torch_path_count() == t0
    check(f"{name} N={N}", {"y": yd, "dx": xd.grad}, {"y": y64.detach(), "dx": x64.grad})
    x3 = x.view(M, 1, N).to(DEV)  # any leading shape
    assert torch.equal(Fh.seq_act(x3, name).view(M, N), yd.detach())


def test_seq_take_is_the_selected_row_and_its_scatter():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    B, L, D = 9, 5, 7
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, L, D, generator=gen)
    qpos = torch.tensor([0, L - 1, -1, 2, 3, 1, -1, 4, 0])
    g = torch.randn(B, D, generator=gen)
    xd = x.to(DEV).requires_grad_(True)
    out = Fh.seq_take(xd, qpos.to(DEV))
    (out * g.to(DEV)).sum().backward()
    live = qpos >= 0
    want = x[torch.arange(B), qpos.clamp(min=0)] * live[:, None]
    dx = torch.zeros(B, L, D)
    dx[torch.arange(B)[live], qpos[live]] = g[live]
    assert torch.equal(out.detach().cpu(), want) and torch.equal(xd.grad.cpu(), dx)


@pytest.mark.parametrize("p", [0.3, 0.9])
@pytest.mark.parametrize("B,heads,L", [(2, 2, 5), (1, 3, 128)])  # a row that ends inside a Philox group; the kernel's limit
def test_attention_dropout_and_mlp_dropout_draw_from_one_generator(B, heads, L, p):
    """Element (m, n) of a 128-wide dropout matrix is in Philox group 32 m + n / 4; attention row m = (b heads + head) L + i,
    key n is in group 32 m + n / 4 too: at one (seed, offset) the two masks agree byte for byte on the first L columns."""
    require_gpu()
    from rec_pangu_amd import hip
    seed, offset = 20240611, 40
    rows = B * heads * L
    keep = hip.seq_attn_keep_mask(B, heads, L, p, seed, offset, torch.device(DEV)).view(rows, L)
    _, mask = hip.dropout_fwd(torch.ones(rows, 128, device=DEV), p, seed, offset)
    assert mask.dtype == keep.dtype == torch.uint8 and mask.shape == (rows, 128)
    assert torch.equal(keep.cpu(), mask[:, :L].cpu())
