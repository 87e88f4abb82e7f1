"""FiBiNet and AFM on the HIP path: the reference's golden vectors in every matrix-core mode (the MLP's GEMMs; the SENET +
bilinear block is fp32 FMA), a Criteo-shaped batch against the model's own CPU path (pinned to the reference by
tests/test_fibinet_host.py), no torch path under RP_STRICT_HIP, an embedding width outside hip.bilinear_fits on torch ops, the
stand-alone BilinearInteractionLayer, and the captured training step — as a launch plan and as a hipGraph — bit-identical to
the eager loop."""
import copy
import functools
import warnings

import pytest
import torch

from conftest import load_golden, require_gpu
from test_fibinet_host import NAMES, build

pytestmark = pytest.mark.gpu
DEV = "cuda"


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
        b["label"] = (torch.rand(B, generator=gen) < 0.3).float()
        out.append(b)
    return out


def _grad_close(got, ref, what):
    tol = 1e-4 * max(1e-2, float(ref.abs().max()))
    err = float((got.cpu() - ref).abs().max())
    assert err <= tol, f"{what}: {err} > {tol}"
    return err / tol


@pytest.mark.parametrize("name", NAMES)
def test_forward_backward_adam_vs_reference(name, matmul_mode):
    from rec_pangu_amd import hip
    from rec_pangu_amd.optim import FusedAdam, make_adam
    g = load_golden("model_fibinet.npz")
    model = build(name).to(DEV)
    model.eval()
    n0, n_paths = hip.launch_count(), hip.torch_path_count()
    out = model(_to_dev(g["batch"]))
    assert hip.launch_count() > n0 and hip.torch_path_count() == n_paths, "the HIP kernels did not run"
    for k, v in g["out"].items():
        print(f"{name} {matmul_mode} {k}: {float((out[k].detach().cpu() - v).abs().max()):.3g}")
        torch.testing.assert_close(out[k].detach().cpu(), v, rtol=1e-4, atol=1e-5, msg=lambda m: f"{name}:{k}: {m}")
    model.zero_grad()
    out["loss"].backward()
    params = dict(model.named_parameters())
    worst = 0.0
    for k, v in g["grad"].items():
        assert params[k].grad is not None, k
        worst = max(worst, _grad_close(params[k].grad, v, f"{name}: grad {k}"))
    print(f"{name} {matmul_mode} worst gradient error / bar: {worst:.3g}")
    # two FusedAdam steps, then the inference output
    model = build(name).to(DEV)
    model.eval()
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
        assert err <= tol, f"{name}: {k} off by {err} after two Adam steps (tol {tol})"
    print(f"{name} {matmul_mode} worst weight error / bar: {worst:.3g}")
    n_paths = hip.torch_path_count()
    with torch.no_grad():
        r = model(_to_dev(g["batch"]), is_training=False)
    assert "loss" not in r and hip.torch_path_count() == n_paths
    for k, v in g["adam2_out"].items():
        torch.testing.assert_close(r[k].cpu(), v, rtol=1e-3, atol=1e-4)


@functools.lru_cache(maxsize=None)
def _criteo():
    """the Criteo-shaped CPU model, its batch and the CPU result with every gradient: computed once, shared by the matrix-core
    modes, left unchanged"""
    from rec_pangu_amd.models.ranking import FiBiNet
    card = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306,
            10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]
    enc = {f"I{i + 1}": {"min": 0.0, "max": 1.0} for i in range(13)}
    enc.update({f"C{i + 1}": {"vocab_size": max(2, c // 64)} for i, c in enumerate(card)})
    torch.manual_seed(0)
    cpu = FiBiNet(embedding_dim=32, enc_dict=enc)
    assert cpu.senet_layer.excitation[0].weight.shape == (8, 26) and cpu.dnn.net[0].weight.shape == (64, 26 * 25 * 32 + 13)
    cpu.eval()
    gen = torch.Generator().manual_seed(1)
    B = 256
    batch = {f"I{i + 1}": torch.rand(B, generator=gen) for i in range(13)}
    batch.update({f"C{i + 1}": torch.randint(0, enc[f"C{i + 1}"]["vocab_size"] + 1, (B,), generator=gen) for i in range(26)})
    batch["label"] = (torch.rand(B, generator=gen) < 0.25).float()
    ref = cpu(batch)
    ref["loss"].backward()
    return cpu, batch, {k: v.detach() for k, v in ref.items()}


def test_criteo_shape_vs_the_cpu_path(matmul_mode):
    """13 dense + 26 sparse (Criteo cardinalities / 64), D = 32, B = 256: 325 pairs, 8 SENET units, an MLP input of 20813
    columns.  pred, loss and every gradient against a deepcopy of the model on the CPU."""
    from rec_pangu_amd import hip
    cpu, batch, ref = _criteo()
    model = copy.deepcopy(cpu).to(DEV)
    model.zero_grad()
    n0, n_paths = hip.launch_count(), hip.torch_path_count()
    out = model(_to_dev(batch))
    out["loss"].backward()
    assert hip.launch_count() > n0 and hip.torch_path_count() == n_paths
    for k in ("pred", "loss"):
        print(f"{matmul_mode} {k}: {float((out[k].detach().cpu() - ref[k].detach()).abs().max()):.3g}")
        torch.testing.assert_close(out[k].detach().cpu(), ref[k].detach(), rtol=1e-4, atol=1e-5)
    rgrads = {k: p.grad for k, p in cpu.named_parameters()}
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        rg = rgrads[k]
        assert p.grad is not None and rg is not None, k
        tol = 1e-4 * max(1e-2, float(rg.abs().max()))
        err = float((p.grad.cpu() - rg).abs().max())
        if err / tol > worst[1]:
            worst = (k, err / tol)
    print(f"{matmul_mode} worst gradient error / bar: {worst[1]:.3g} ({worst[0]})")
    for k, p in model.named_parameters():
        _grad_close(p.grad, rgrads[k], f"grad {k}")


def test_default_constructor_takes_no_torch_path(monkeypatch):
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.ranking import FiBiNet
    monkeypatch.setenv("RP_STRICT_HIP", "1")
    enc = _enc(3, [7, 3, 1000, 11, 90, 5])
    torch.manual_seed(0)
    model = FiBiNet(enc_dict=enc).to(DEV)
    model.train()
    n_paths, n0 = hip.torch_path_count(), hip.launch_count()
    out = model(_to_dev(_batches(enc, 64, 1, seed=3)[0]))
    out["loss"].backward()
    assert hip.torch_path_count() == n_paths and hip.launch_count() > n0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_a_width_outside_the_range_runs_on_torch_ops_and_matches_the_cpu():
    """D = 12: outside hip.bilinear_fits.  The model composes the block from device ops, says so (exactly one counted torch
    path), and agrees with its CPU copy"""
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.ranking import FiBiNet
    enc = _enc(2, [7, 3, 1000, 11, 90])
    torch.manual_seed(2)
    cpu = FiBiNet(embedding_dim=12, enc_dict=enc)
    assert not cpu.hip_supported()
    cpu.eval()
    batch = _batches(enc, 48, 1, seed=5)[0]
    model = copy.deepcopy(cpu).to(DEV)
    ref = cpu(batch)
    ref["loss"].backward()
    n_paths = hip.torch_path_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = model(_to_dev(batch))
    assert hip.torch_path_count() == n_paths + 1
    out["loss"].backward()
    for k in ("pred", "loss"):
        torch.testing.assert_close(out[k].detach().cpu(), ref[k].detach(), rtol=1e-4, atol=1e-5)
    rgrads = {k: p.grad for k, p in cpu.named_parameters()}
    for k, p in model.named_parameters():
        _grad_close(p.grad, rgrads[k], f"grad {k}")


@pytest.mark.parametrize("btype", ["field_all", "field_each", "field_interaction"])
def test_the_stand_alone_bilinear_layer_equals_its_cpu_result(btype):
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.layers import BilinearInteractionLayer
    torch.manual_seed(3)
    cpu = BilinearInteractionLayer(6, 16, btype)
    x = torch.randn(21, 6, 16)
    cot = torch.randn(21, 15, 16)
    xc = x.clone().requires_grad_(True)
    ref = cpu(xc)
    ref.backward(cot)
    layer = copy.deepcopy(cpu).to(DEV)
    layer.zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    n0, n_paths = hip.launch_count(), hip.torch_path_count()
    out = layer(xd)
    out.backward(cot.to(DEV))
    assert hip.launch_count() > n0 and hip.torch_path_count() == n_paths
    assert out.shape == ref.shape
    _grad_close(out.detach(), ref.detach(), "out")
    _grad_close(xd.grad, xc.grad, "dx")
    for k, (w, rw) in enumerate(zip(layer.weights(), cpu.weights())):
        if rw.grad is None:
            assert w.grad is None, "a matrix no pair uses takes no gradient"
        else:
            _grad_close(w.grad, rw.grad, f"dW {k}")


@pytest.fixture(params=["plan", "hipgraph"])
def backend(request, monkeypatch):
    monkeypatch.setenv("RP_GRAPH_BACKEND", request.param)
    return request.param


def test_graphed_step_is_bit_identical_to_the_eager_loop(backend):
    """6 sparse + 5 dense, D = 16, B = 384, 4 steps (two eager, two replayed): every prediction, loss, weight and optimizer moment
    of the replayed step equals the eager loop's; the step holds library launches only, so it replays as a launch plan"""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    from rec_pangu_amd.models.ranking import FiBiNet
    from rec_pangu_amd.optim import FusedAdam
    steps = 4
    enc = _enc(5, [3000, 17, 900, 4, 20000, 250])
    batches = [_to_dev(b) for b in _batches(enc, 384, steps + 1, seed=4)]
    results = {}
    try:
        for mode in ("eager", "graph"):
            torch.manual_seed(0)
            model = FiBiNet(embedding_dim=16, enc_dict=enc).to(DEV)
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
                preds.append(out["pred"].detach().clone())
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
    e, g = results["eager"], results["graph"]
    assert all(torch.isfinite(p).all() for p in e[0])
    for a, b in zip(e[0], g[0]):
        assert torch.equal(a, b), "predictions differ"
    for a, b in zip(e[1], g[1]):
        assert torch.equal(a, b), "losses differ"
    for k in e[2]:
        assert torch.equal(e[2][k], g[2][k]), k
    for sa, sb in zip(e[3], g[3]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"optimizer state {k}"
