"""ESSM and AITM on the HIP path: the reference's golden vectors in every matrix-core mode, a Criteo-shaped batch against the
model's own CPU path (pinned to the reference by tests/test_mtl_host.py), the default constructors without a torch path under
RP_STRICT_HIP, an attention configuration outside every HIP form on torch ops, the loss methods on device tensors, and the
captured training step — as a launch plan and as a hipGraph — bit-identical to the eager loop."""
import copy
import functools
import warnings

import pytest
import torch

from conftest import load_golden, require_gpu
from test_mtl_host import CASES, build

pytestmark = pytest.mark.gpu
DEV = "cuda"
CRITEO_CARD = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306,
               10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


@pytest.fixture(params=["auto", "bf16x6", "bf16x3"])
def matmul_mode(request):
    from rec_pangu_amd import hip
    prev = hip.get_matmul_precision()
    hip.set_matmul_precision(request.param)
    yield request.param
    hip.set_matmul_precision(prev)


def _to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _enc(n_dense, vocabs):
    enc = {f"I{i}": {"min": 0.0, "max": 1.0} for i in range(n_dense)}
    enc.update({f"C{i}": {"vocab_size": v} for i, v in enumerate(vocabs)})
    return enc


def _batches(enc, B, n, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        b = {k: (torch.rand(B, generator=gen) if "min" in v else torch.randint(0, v["vocab_size"] + 1, (B,), generator=gen))
             for k, v in enc.items()}
        b["task1_label"] = (torch.rand(B, generator=gen) < 0.3).float()
        b["task2_label"] = (torch.rand(B, generator=gen) < 0.1).float()
        out.append(b)
    return out


def _grad_close(got, ref, what):
    tol = 1e-4 * max(1e-2, float(ref.abs().max()))
    err = float((got.cpu() - ref).abs().max())
    assert err <= tol, f"{what}: {err} > {tol}"
    return err / tol


def _model(name, enc, **kw):
    from rec_pangu_amd.models import multi_task
    return getattr(multi_task, name)(enc_dict=enc, **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_forward_backward_adam_vs_reference(case, matmul_mode):
    from rec_pangu_amd import hip
    from rec_pangu_amd.optim import FusedAdam, make_adam
    g = load_golden(f"model_{case}.npz")
    model = build(case).to(DEV)
    n0, n_paths = hip.launch_count(), hip.torch_path_count()
    out = model(_to_dev(g["batch"]))
    assert hip.launch_count() > n0 and hip.torch_path_count() == n_paths, "the HIP kernels did not run"
    for k, v in g["out"].items():
        assert out[k].shape == v.shape, k
        print(f"{case} {matmul_mode} {k}: {float((out[k].detach().cpu() - v).abs().max()):.3g}")
        torch.testing.assert_close(out[k].detach().cpu(), v, rtol=1e-4, atol=1e-5, msg=lambda m: f"{case}:{k}: {m}")
    model.zero_grad()
    out["loss"].backward()
    params = dict(model.named_parameters())
    worst = 0.0
    for k, v in g["grad"].items():
        assert params[k].grad is not None, k
        worst = max(worst, _grad_close(params[k].grad, v, f"{case}: grad {k}"))
    print(f"{case} {matmul_mode} worst gradient error / bar: {worst:.3g}")
    # two FusedAdam steps, then the inference output
    model = build(case).to(DEV)
    opt = make_adam(model, 1e-2)
    assert isinstance(opt, FusedAdam)
    for _ in range(2):
        r = model(_to_dev(g["batch"]))
        r["loss"].backward()
        opt.step()
        model.zero_grad()
    sd = model.state_dict()
    worst = 0.0
    for k, v in g["adam2"].items():
        tol = 2e-4 * max(1e-2, float(v.abs().max()))
        err = float((sd[k].cpu() - v).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, f"{case}: {k} off by {err} after two Adam steps (tol {tol})"
    print(f"{case} {matmul_mode} worst weight error / bar: {worst:.3g}")
    model.eval()
    n_paths = hip.torch_path_count()
    with torch.no_grad():
        r = model(_to_dev(g["batch"]), is_training=False)
    assert "loss" not in r and hip.torch_path_count() == n_paths
    for k, v in g["adam2_out"].items():
        assert r[k].shape == v.shape, k
        torch.testing.assert_close(r[k].cpu(), v, rtol=1e-3, atol=1e-4)


@functools.lru_cache(maxsize=None)
def _criteo(name):
    """the Criteo-shaped CPU model with its default towers, its batch and the CPU result with every gradient: computed once per
    model, shared by the matrix-core modes, left unchanged"""
    enc = {f"I{i + 1}": {"min": 0.0, "max": 1.0} for i in range(13)}  # (present in the batch, read by neither model)
    enc.update({f"C{i + 1}": {"vocab_size": max(2, c // 64)} for i, c in enumerate(CRITEO_CARD)})
    torch.manual_seed(0)
    cpu = _model(name, enc, embedding_dim=32)
    first = cpu.ctr_layer if name == "ESSM" else cpu.click_tower
    assert first.net[0].weight.shape == ((128 if name == "ESSM" else 400), 26 * 32)
    cpu.eval()
    gen = torch.Generator().manual_seed(1)
    B = 256
    batch = {f"I{i + 1}": torch.rand(B, generator=gen) for i in range(13)}
    batch.update({f"C{i + 1}": torch.randint(0, enc[f"C{i + 1}"]["vocab_size"] + 1, (B,), generator=gen) for i in range(26)})
    batch["task1_label"] = (torch.rand(B, generator=gen) < 0.25).float()
    batch["task2_label"] = (torch.rand(B, generator=gen) < 0.1).float()
    ref = cpu(batch)
    ref["loss"].backward()
    return cpu, batch, {k: v.detach() for k, v in ref.items()}


@pytest.fixture(params=["auto", "bf16x6"])
def exact_matmul_mode(request):
    from rec_pangu_amd import hip
    prev = hip.get_matmul_precision()
    hip.set_matmul_precision(request.param)
    yield request.param
    hip.set_matmul_precision(prev)


@pytest.mark.parametrize("name", ["ESSM", "AITM"])
def test_criteo_shape_vs_the_cpu_path(name, exact_matmul_mode):
    """26 sparse fields (Criteo cardinalities / 64), D = 32, B = 256, the default hidden_dim / tower_dims (AITM: the wide attention
    form at T = 2, a = 400): predictions, loss and every gradient against a deepcopy of the model on the CPU, in eval().

    In the two modes whose products are fp32-faithful.  The bf16x3 mode (2^-16 per product) is pinned by the goldens above,
    whose seed keeps every ReLU pre-activation 1e-5 away from 0; this batch cannot: of the 716800 ReLU units of AITM's towers and
    info_layer here, 56 have a float64 pre-activation within 1e-5 of 0 and 4 within 1e-6 (counted on the CPU), so a product
    error of that size flips some — each flip changes one sample's gradient by a part in a few hundred, far above a 1e-4 bar,
    whatever the kernels do.  Measured on an
    MI355X in bf16x3: predictions within 1.1e-6 and the loss within 2.4e-7 of the CPU, the worst gradient (one embedding table's)
    2.9e-4 off at a scale of 7.7e-2."""
    matmul_mode = exact_matmul_mode
    from rec_pangu_amd import hip
    cpu, batch, ref = _criteo(name)
    model = copy.deepcopy(cpu).to(DEV)
    model.zero_grad()
    if name == "AITM":
        assert model.attention_layer._wide(2) and not hip.attention_core_fits(2, 1, 400)
    n0, n_paths = hip.launch_count(), hip.torch_path_count()
    out = model(_to_dev(batch))
    out["loss"].backward()
    assert hip.launch_count() > n0 and hip.torch_path_count() == n_paths
    for k in ("task1_pred", "task2_pred", "loss"):
        assert out[k].shape == ref[k].shape
        print(f"{name} {matmul_mode} {k}: {float((out[k].detach().cpu() - ref[k]).abs().max()):.3g}")
        torch.testing.assert_close(out[k].detach().cpu(), ref[k], rtol=1e-4, atol=1e-5)
    rgrads = {k: p.grad for k, p in cpu.named_parameters()}
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        rg = rgrads[k]
        assert p.grad is not None and rg is not None, k
        tol = 1e-4 * max(1e-2, float(rg.abs().max()))
        err = float((p.grad.cpu() - rg).abs().max())
        if err / tol > worst[1]:
            worst = (k, err / tol)
    print(f"{name} {matmul_mode} worst gradient error / bar: {worst[1]:.3g} ({worst[0]})")
    for k, p in model.named_parameters():
        _grad_close(p.grad, rgrads[k], f"grad {k}")


@pytest.mark.parametrize("name", ["ESSM", "AITM"])
def test_default_constructor_takes_no_torch_path(name, monkeypatch):
    from rec_pangu_amd import hip
    monkeypatch.setenv("RP_STRICT_HIP", "1")
    enc = _enc(3, [7, 3, 1000, 11, 90, 5])
    torch.manual_seed(0)
    model = _model(name, enc).to(DEV)
    model.train()
    n_paths, n0 = hip.torch_path_count(), hip.launch_count()
    batch = _to_dev(_batches(enc, 64, 1, seed=3)[0])
    out = model(batch)
    out["loss"].backward()
    assert hip.torch_path_count() == n_paths and hip.launch_count() > n0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    model.eval()
    with torch.no_grad():
        r = model(batch, is_training=False)
    assert hip.torch_path_count() == n_paths and "loss" not in r
    assert r["task1_pred"].shape == out["task1_pred"].shape == ((64, 1) if name == "ESSM" else (64,))


def test_an_attention_outside_every_form_runs_on_torch_ops_and_matches_the_cpu():
    """MultiHeadSelfAttention(36, num_heads=2, attention_dim=18) over 64 tokens: two heads (not the wide form), heads wider than
    16 (not the split form), Q/K/V of 64 tokens beside the weights beyond the one-launch layer's LDS.  The layer composes itself
    from device ops, says so (exactly one counted torch path), and agrees with its CPU copy"""
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.layers import MultiHeadSelfAttention
    T = 64
    assert not hip.attention_wide_fits(T, 2, 18) and not hip.attention_core_fits(T, 2, 18)
    assert not hip.field_attention_fits(T, 36, 2, 18, False)
    torch.manual_seed(4)
    cpu = MultiHeadSelfAttention(36, num_heads=2, attention_dim=18)
    assert cpu.W_res is None
    x = torch.randn(6, T, 36)
    cot = torch.randn(6, T, 36)
    xc = x.clone().requires_grad_(True)
    ref = cpu(xc)
    ref.backward(cot)
    layer = copy.deepcopy(cpu).to(DEV)
    layer.zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    n_paths = hip.torch_path_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = layer(xd)
    assert hip.torch_path_count() == n_paths + 1
    out.backward(cot.to(DEV))
    _grad_close(out.detach(), ref.detach(), "out")
    _grad_close(xd.grad, xc.grad, "dx")
    for k, p in layer.named_parameters():
        _grad_close(p.grad, dict(cpu.named_parameters())[k].grad, f"grad {k}")


def test_the_loss_methods_on_device_tensors():
    """ESSM.loss / AITM.loss keep their signatures on device tensors and equal the CPU formulas, value and gradients"""
    from rec_pangu_amd import hip
    enc = _enc(0, [7, 3])
    essm, aitm = _model("ESSM", enc, embedding_dim=4), _model("AITM", enc, embedding_dim=4)
    g = torch.Generator().manual_seed(0)
    B = 300
    p1, p2 = torch.rand(B, generator=g) * 0.98 + 0.01, torch.rand(B, generator=g) * 0.98 + 0.01
    y1, y2 = (torch.rand(B, generator=g) < 0.4).float(), (torch.rand(B, generator=g) < 0.2).float()
    for which in ("essm", "aitm"):
        res = {}
        for dev in ("cpu", DEV):
            a, b = (t.clone().to(dev).requires_grad_(True) for t in (p1, p2))  # (leaves on both devices)
            data = {"task1_label": y1.to(dev), "task2_label": y2.to(dev)}
            n_paths = hip.torch_path_count()
            if which == "essm":
                loss = essm.loss(a[:, None], (a * b)[:, None], data, weight=0.3)
            else:
                loss = aitm.loss(data["task1_label"], a, data["task2_label"], b, constraint_weight=0.7)
            assert hip.torch_path_count() == n_paths
            loss.backward()
            res[dev] = (loss.detach().cpu(), a.grad.cpu(), b.grad.cpu())
        torch.testing.assert_close(res[DEV][0], res["cpu"][0], rtol=1e-5, atol=1e-6)
        _grad_close(res[DEV][1], res["cpu"][1], f"{which}: dp1")
        _grad_close(res[DEV][2], res["cpu"][2], f"{which}: dp2")


@pytest.fixture(params=["plan", "hipgraph"])
def backend(request, monkeypatch):
    monkeypatch.setenv("RP_GRAPH_BACKEND", request.param)
    return request.param


@pytest.mark.parametrize("name", ["ESSM", "AITM"])
def test_graphed_step_is_bit_identical_to_the_eager_loop(name, backend):
    """the default constructors (dropout active: the step's dropout launches read the device clock, as in the MMOE graph tests) on 6
    sparse + 5 dense features, B = 384, 4 steps (two eager, two replayed, one per static batch): every prediction, loss, weight
    and optimizer moment of the replayed step equals the eager loop's; the step holds library launches only, so it replays as a
    launch plan, and no torch path is counted"""
    from rec_pangu_amd import hip
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    from rec_pangu_amd.optim import FusedAdam
    steps = 4
    enc = _enc(5, [3000, 17, 900, 4, 20000, 250])
    batches = [_to_dev(b) for b in _batches(enc, 384, steps + 1, seed=4)]
    results = {}
    n_paths = hip.torch_path_count()
    try:
        for mode in ("eager", "graph"):
            torch.manual_seed(0)
            model = _model(name, enc).to(DEV)
            for m in model.modules():
                if hasattr(m, "check_indices"):
                    m.check_indices = "deferred"
            model.train()
            opt = FusedAdam(model.parameters(), lr=1e-3, fuse_zero_grad=True, lazy_tables=True, replay="closed", defer=True)
            gstep = GraphedTrainStep(model, opt) if mode == "graph" else None
            preds, losses = [], []
            for i in range(steps):
                if gstep is not None:
                    out = gstep(batches[i], batches[i + 1])
                else:
                    model.prefetch(batches[i + 1])
                    out = model(batches[i])
                    out["loss"].backward()
                    opt.step()
                    model.zero_grad()
                preds.append((out["task1_pred"].detach().clone(), out["task2_pred"].detach().clone()))
                losses.append(out["loss"].detach().clone())
            if gstep is not None:
                assert gstep.replays == steps - 2, "every step after the two eager ones must have been a graph replay"
                if backend == "plan":
                    assert gstep.backend_used == "plan", (gstep.backend_used, gstep.why_not_plan)
                else:
                    assert gstep.backend_used == "hipgraph"
            model.embedding_layer.raise_if_bad_index()
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            osd = opt.state_dict()
            results[mode] = (preds, losses, sd,
                             [{k: v.clone() for k, v in st.items() if torch.is_tensor(v)} for st in osd["state"].values()])
    finally:
        EmbeddingLayer.unpin_sorts()
    assert hip.torch_path_count() == n_paths
    e, g = results["eager"], results["graph"]
    assert all(torch.isfinite(p).all() for pair in e[0] for p in pair)
    for (a1, a2), (b1, b2) in zip(e[0], g[0]):
        assert torch.equal(a1, b1) and torch.equal(a2, b2), "predictions differ"
    for a, b in zip(e[1], g[1]):
        assert torch.equal(a, b), "losses differ"
    for k in e[2]:
        assert torch.equal(e[2][k], g[2][k]), k
    for sa, sb in zip(e[3], g[3]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"optimizer state {k}"
