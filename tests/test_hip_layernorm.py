"""rp_layernorm_fwd / rp_layernorm_bwd (csrc/layernorm.hip) against a float64 evaluation of the same formula.

Metric per tensor: max|got - ref| / max(1e-2, max|ref|); bar 1e-5.  torch's own fp32 CPU LayerNorm measures <= 1.5e-6 against
float64 on this metric at these shapes and both offsets (y, dx, dgamma, dbeta, dmul), so the kernels get about 7x that for
their different summation order; a one-pass variance (E[x^2] - mean^2) misses the off = 30 rows by more than an order of
magnitude.  Shapes: every register-resident width class (every 256 columns up to 2048), the looped path above it (4099),
widths that are no multiple of 4 (the scalar tail), ld = N (unaligned rows: per-element loads) and ld = ceil64(N) (dwordx4),
M = 1, 5, 300 and 2125 (> the backward's 2048 partial rows: the grid-stride loop and the two-stage reduction turn over)."""
import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-5
M_BIG = 2125  # the backward walks the rows with 512 blocks x 4 waves


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


def _err(got, ref):
    ref = ref.to(torch.float64)
    return float((got.detach().cpu().to(torch.float64) - ref).abs().max()) / max(1e-2, float(ref.abs().max()))


def _inputs(M, N, off, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(x=1.5 * torch.randn(M, N, generator=g) + off, dy=torch.randn(M, N, generator=g),
                mul=torch.randn(M, N, generator=g), gamma=1.0 + 0.5 * torch.randn(N, generator=g),
                beta=0.3 * torch.randn(N, generator=g), y0=torch.randn(M, N, generator=g), dx0=torch.randn(M, N, generator=g))


def _reference(t, use_mul, out_scale, dy_scale, accumulate, eps=1e-5):
    """float64, by autograd of the formula: y = out_scale * ((gamma (x - mu) r + beta) [* mul]) [+ y0]"""
    d = {k: v.to(torch.float64) for k, v in t.items()}
    x, gamma, beta, mul = (d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta", "mul"))
    mu = x.mean(dim=1, keepdim=True)
    r = 1.0 / torch.sqrt(((x - mu) ** 2).mean(dim=1, keepdim=True) + eps)
    n = gamma * ((x - mu) * r) + beta
    core = n * mul if use_mul else n
    core.backward(d["dy"] * dy_scale)
    out = dict(y=out_scale * core.detach() + (d["y0"] if accumulate else 0.0), dx=x.grad + (d["dx0"] if accumulate else 0.0),
               dgamma=gamma.grad, dbeta=beta.grad, mu=mu.detach().reshape(-1), r=r.detach().reshape(-1))
    if use_mul:
        out["dmul"] = mul.grad
    return out


def _padded(src, ld, fill=float("nan")):
    """src [M, N] inside a NaN-filled [M, ld] device buffer -> (buffer, the [M, N] view of it)"""
    buf = torch.full((src.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :src.shape[1]] = src.to(DEV)
    return buf, buf[:, :src.shape[1]]


def _run(t, ld, use_mul, out_scale, dy_scale, accumulate, stats=None):
    """the two launches on [M, ld] buffers whose padding columns hold NaN; y and dx are given N_pad = N + (ld - N) // 2"""
    from rec_pangu_amd import hip
    M, N = t["x"].shape
    n_pad = N + (ld - N) // 2
    _, x = _padded(t["x"], ld)
    _, dy = _padded(t["dy"], ld)
    mul = _padded(t["mul"], ld)[1] if use_mul else None
    gamma, beta = t["gamma"].to(DEV), t["beta"].to(DEV)
    ybuf, _ = _padded(t["y0"] if accumulate else torch.full((M, N), float("nan")), ld)
    dxbuf, _ = _padded(t["dx0"] if accumulate else torch.full((M, N), float("nan")), ld)
    n0 = hip.launch_count()
    _, st = hip.layernorm_fwd(x, gamma, beta, 1e-5, mul=mul, out=ybuf[:, :n_pad], out_scale=out_scale, accumulate=accumulate,
                              stats=stats, stats_given=stats is not None)
    _, dmul, dgamma, dbeta = hip.layernorm_bwd(dy, x, st, gamma, beta, mul=mul, dy_scale=dy_scale, dx=dxbuf[:, :n_pad],
                                               accumulate=accumulate)
    assert hip.launch_count() == n0 + 3  # forward, backward, the backward's finish
    return dict(ybuf=ybuf, dxbuf=dxbuf, stats=st, dmul=dmul, dgamma=dgamma, dbeta=dbeta, n_pad=n_pad)


def _check(got, ref, N, what):
    for name, buf in (("y", got["ybuf"]), ("dx", got["dxbuf"])):
        e = _err(buf[:, :N], ref[name])
        print(f"{what} {name}: {e:.3g}")
        assert e <= BAR, f"{what}: {name} off by {e}"
        pad = buf[:, N:got["n_pad"]]
        assert torch.count_nonzero(pad) == 0 and not torch.isnan(pad).any(), f"{what}: {name} padding up to N_pad must be zeros"
        assert torch.isnan(buf[:, got["n_pad"]:]).all(), f"{what}: {name} beyond N_pad must not be touched"
    for name in ("dgamma", "dbeta") + (("dmul",) if "dmul" in ref else ()):
        e = _err(got[name][..., :N], ref[name])
        print(f"{what} {name}: {e:.3g}")
        assert e <= BAR, f"{what}: {name} off by {e}"
    assert _err(got["stats"][:, 0], ref["mu"]) <= BAR and _err(got["stats"][:, 1], ref["r"]) <= BAR, f"{what}: statistics"


@pytest.mark.parametrize("N", [8, 43, 63, 64, 65, 257, 1677, 4099])
def test_layernorm_fwd_bwd_vs_float64(N):
    for M, off in [(1, 0.0), (1, 30.0), (5, 0.0), (5, 30.0), (300, 0.0), (300, 30.0), (M_BIG, 30.0)]:
        t = _inputs(M, N, off, seed=1000 * N + M + int(off))
        plain = _reference(t, use_mul=False, out_scale=1.0, dy_scale=1.0, accumulate=False)
        fused = _reference(t, use_mul=True, out_scale=0.25, dy_scale=0.5, accumulate=True)
        for ld in (N, (N + 63) // 64 * 64):
            what = f"N={N} M={M} off={off} ld={ld}"
            got = _run(t, ld, use_mul=False, out_scale=1.0, dy_scale=1.0, accumulate=False)
            _check(got, plain, N, what + " plain")
            # the statistics of the first launch handed back in (the parallel MaskBlocks normalise one x), the multiplier
            # inside the launch, out_scale + accumulate into y, dy_scale, accumulate into dx
            again = _run(t, ld, use_mul=True, out_scale=0.25, dy_scale=0.5, accumulate=True, stats=got["stats"].clone())
            _check(again, fused, N, what + " mul/accumulate")
            assert torch.equal(again["stats"], got["stats"])


@pytest.mark.parametrize("N", [513, 1000, 1100, 1500, 2048, 2049])
def test_layernorm_remaining_width_classes(N):
    """the kernels are instantiated per 256 columns of row held in registers (1 .. 8 quads per lane, then the looped path):
    the classes the shapes above leave out (3, 4, 5, 6 and 8 quads) and the first width past the register-resident limit"""
    t = _inputs(37, N, 30.0, seed=N)
    plain = _reference(t, use_mul=False, out_scale=1.0, dy_scale=1.0, accumulate=False)
    fused = _reference(t, use_mul=True, out_scale=0.25, dy_scale=0.5, accumulate=True)
    for ld in (N, (N + 63) // 64 * 64 + 64):
        got = _run(t, ld, use_mul=False, out_scale=1.0, dy_scale=1.0, accumulate=False)
        _check(got, plain, N, f"N={N} ld={ld} plain")
        again = _run(t, ld, use_mul=True, out_scale=0.25, dy_scale=0.5, accumulate=True, stats=got["stats"].clone())
        _check(again, fused, N, f"N={N} ld={ld} mul/accumulate")


@pytest.mark.parametrize("N,M", [(43, 300), (1677, M_BIG), (4099, M_BIG)])
def test_layernorm_bwd_is_bit_identical_from_run_to_run(N, M):
    t = _inputs(M, N, 30.0, seed=N)
    ld = (N + 63) // 64 * 64
    a = _run(t, ld, use_mul=True, out_scale=1.0, dy_scale=1.0, accumulate=False)
    b = _run(t, ld, use_mul=True, out_scale=1.0, dy_scale=1.0, accumulate=False)
    for k in ("stats", "dmul", "dgamma", "dbeta"):
        assert torch.equal(a[k][..., :N], b[k][..., :N]), k
    for k in ("ybuf", "dxbuf"):
        assert torch.equal(a[k][:, :a["n_pad"]], b[k][:, :b["n_pad"]]), k


def test_layernorm_unaligned_base_pointer():
    """rows a multiple of 4 floats apart but starting 4 bytes off a 16-byte boundary: the per-element path, same results"""
    from rec_pangu_amd import hip
    M, N, ld = 37, 43, 64
    t = _inputs(M, N, 30.0, seed=5)
    ref = _reference(t, use_mul=True, out_scale=1.0, dy_scale=1.0, accumulate=False)

    def shifted(src):
        flat = torch.full((M * ld + 1,), float("nan"), dtype=torch.float32, device=DEV)
        v = flat[1:].view(M, ld)[:, :N]
        v.copy_(src.to(DEV))
        return v

    x, dy, mul = shifted(t["x"]), shifted(t["dy"]), shifted(t["mul"])
    assert x.data_ptr() % 16 == 4
    gamma, beta = t["gamma"].to(DEV), t["beta"].to(DEV)
    y, st = hip.layernorm_fwd(x, gamma, beta, 1e-5, mul=mul, out=shifted(torch.zeros(M, N)))
    dx, dmul, dgamma, dbeta = hip.layernorm_bwd(dy, x, st, gamma, beta, mul=mul, dx=shifted(torch.zeros(M, N)))
    for name, got in (("y", y), ("dx", dx), ("dmul", dmul[:, :N]), ("dgamma", dgamma), ("dbeta", dbeta)):
        assert _err(got, ref[name]) <= BAR, name


def test_layernorm_width_one_is_finite():
    """N = 1: the variance is 0 and r = 1 / sqrt(eps) = 316 amplifies rounding, so no accuracy bar (the fp32 reference alone
    misses it there) — y = beta * mul exactly as x - mean = 0, and every gradient is finite"""
    from rec_pangu_amd import hip
    t = _inputs(9, 1, 30.0, seed=2)
    d = {k: v.to(DEV) for k, v in t.items()}
    y, st = hip.layernorm_fwd(d["x"], d["gamma"], d["beta"], 1e-5, mul=d["mul"])
    torch.testing.assert_close(y, d["beta"] * d["mul"], rtol=1e-6, atol=1e-7)
    outs = hip.layernorm_bwd(d["dy"], d["x"], st, d["gamma"], d["beta"], mul=d["mul"])
    assert all(torch.isfinite(o).all() for o in outs)


def test_layer_norm_function_vs_torch_autograd():
    """functional.layer_norm on the autograd tape (3-D input, with and without the multiplier) against torch's LayerNorm in
    float64"""
    from rec_pangu_amd import functional as Fh
    torch.manual_seed(0)
    ln = torch.nn.LayerNorm(43)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.5 * torch.randn(43))
        ln.bias.copy_(0.3 * torch.randn(43))
    x, mul, cot = torch.randn(4, 6, 43) + 3.0, torch.randn(4, 6, 43), torch.randn(4, 6, 43)
    for use_mul in (False, True):
        ref_ln = torch.nn.LayerNorm(43).double()
        ref_ln.load_state_dict(ln.state_dict())
        xr, mr = x.double().requires_grad_(True), mul.double().requires_grad_(True)
        yr = ref_ln(xr) * mr if use_mul else ref_ln(xr)
        yr.backward(cot.double())
        dev_ln = torch.nn.LayerNorm(43).to(DEV)
        dev_ln.load_state_dict(ln.state_dict())
        xd, md = x.to(DEV).requires_grad_(True), mul.to(DEV).requires_grad_(True)
        yd = Fh.layer_norm(xd, dev_ln, mul=md if use_mul else None)
        yd.backward(cot.to(DEV))
        assert yd.shape == x.shape
        pairs = [(yd, yr), (xd.grad, xr.grad), (dev_ln.weight.grad, ref_ln.weight.grad), (dev_ln.bias.grad, ref_ln.bias.grad)]
        if use_mul:
            pairs.append((md.grad, mr.grad))
        for got, ref in pairs:
            assert _err(got, ref.detach()) <= BAR
