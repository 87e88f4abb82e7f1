"""MaskNet on the HIP path: the reference's golden vectors in every matrix-core mode, a Criteo-shaped batch against the model's
own CPU path (pinned to the reference by tests/test_masknet_host.py), no torch path under RP_STRICT_HIP, and the captured
training step — as a launch plan and as a hipGraph, parallel and serial blocks — bit-identical to the eager loop."""
import copy

import pytest
import torch

from conftest import load_golden, require_gpu
from test_masknet_host import CASES, build

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


@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_adam_vs_reference(name, matmul_mode):
    from rec_pangu_amd import hip
    from rec_pangu_amd.optim import FusedAdam, make_adam
    g = load_golden(f"model_{name}.npz")
    model = build(name).to(DEV)
    model.eval()
    n0 = hip.launch_count()
    out = model(_to_dev(g["batch"]))
    assert hip.launch_count() > n0, "the HIP kernels did not run"
    for k, v in g["out"].items():
        print(f"{name} {matmul_mode} {k}: {float((out[k].detach().cpu() - v).abs().max()):.3g}")
        torch.testing.assert_close(out[k].detach().cpu(), v, rtol=1e-4, atol=1e-5, msg=lambda m: f"{name}:{k}: {m}")
    model.zero_grad()
    out["loss"].backward()
    params = dict(model.named_parameters())
    worst = 0.0
    for k, v in g["grad"].items():
        assert params[k].grad is not None, k
        tol = 1e-4 * max(1e-2, float(v.abs().max()))
        err = float((params[k].grad.cpu() - v).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, f"{name}: grad {k} off by {err} (tol {tol})"
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
    with torch.no_grad():
        r = model(_to_dev(g["batch"]), is_training=False)
    assert "loss" not in r
    for k, v in g["adam2_out"].items():
        torch.testing.assert_close(r[k].cpu(), v, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("parallel", [True, False], ids=["parallel", "serial"])
def test_criteo_shape_vs_the_cpu_path(parallel, matmul_mode):
    """13 dense + 26 sparse (Criteo cardinalities / 64), D = 64: d = 1677, the mask bottleneck 503 wide — both odd.  B = 512,
    two blocks, eval mode; pred, loss and every gradient against a deepcopy of the model on the CPU."""
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.ranking import MaskNet
    card = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306,
            10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]
    enc = {f"I{i + 1}": {"min": 0.0, "max": 1.0} for i in range(13)}
    enc.update({f"C{i + 1}": {"vocab_size": max(2, c // 64)} for i, c in enumerate(card)})
    torch.manual_seed(0)
    cpu = MaskNet(embedding_dim=64, block_num=2, use_parallel=parallel, enc_dict=enc)
    assert cpu.input_dim == 1677 and cpu.mask_block_list[0]._mask_layer[0].out_features == 503
    cpu.eval()
    gen = torch.Generator().manual_seed(1)
    B = 512
    batch = {f"I{i + 1}": torch.rand(B, generator=gen) for i in range(13)}
    batch.update({f"C{i + 1}": torch.randint(0, enc[f"C{i + 1}"]["vocab_size"] + 1, (B,), generator=gen) for i in range(26)})
    batch["label"] = (torch.rand(B, generator=gen) < 0.25).float()
    model = copy.deepcopy(cpu).to(DEV)
    ref = cpu(batch)
    ref["loss"].backward()
    n0 = hip.launch_count()
    out = model(_to_dev(batch))
    out["loss"].backward()
    assert hip.launch_count() > n0
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
    print(f"{matmul_mode} parallel={parallel} worst gradient error / bar: {worst[1]:.3g} ({worst[0]})")
    for k, p in model.named_parameters():
        tol = 1e-4 * max(1e-2, float(rgrads[k].abs().max()))
        err = float((p.grad.cpu() - rgrads[k]).abs().max())
        assert err <= tol, f"grad {k}: {err} > {tol}"


@pytest.mark.parametrize("parallel", [True, False], ids=["parallel", "serial"])
def test_default_constructor_takes_no_torch_path(parallel, monkeypatch):
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.ranking import MaskNet
    monkeypatch.setenv("RP_STRICT_HIP", "1")
    enc = _enc(3, [7, 3, 1000, 11])
    torch.manual_seed(0)
    model = MaskNet(use_parallel=parallel, enc_dict=enc).to(DEV)
    model.train()
    n_paths, n0 = hip.torch_path_count(), hip.launch_count()
    out = model(_to_dev(_batches(enc, 64, 1, seed=3)[0]))
    out["loss"].backward()
    assert hip.torch_path_count() == n_paths and hip.launch_count() > n0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def _grad_close(got, ref, what):
    tol = 1e-4 * max(1e-2, float(ref.abs().max()))
    err = float((got.cpu() - ref).abs().max())
    assert err <= tol, f"{what}: {err} > {tol}"


@pytest.mark.parametrize("shared_input", [False, True], ids=["two_inputs", "one_input"])
def test_mask_block_layer_alone_vs_its_cpu_path(shared_input):
    """the layer outside MaskNet: input, mask input and output of different widths (all odd), 3-D tensors; with one tensor in
    both roles autograd adds the two gradients of it"""
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.layers import MaskBlock
    torch.manual_seed(5)
    din, dmask, dout = (43, 43, 29) if shared_input else (43, 21, 29)
    cpu = MaskBlock(din, dmask, dout, 0.3)
    with torch.no_grad():
        for p in cpu.parameters():
            p.copy_(0.3 * torch.randn_like(p) + (1.0 if p.dim() == 1 else 0.0))
    dev = copy.deepcopy(cpu).to(DEV)
    net = torch.randn(3, 7, din) + 2.0
    mask_in = net if shared_input else torch.randn(3, 7, dmask)
    cot = torch.randn(3, 7, dout)
    nc, nd = net.clone().requires_grad_(True), net.to(DEV).requires_grad_(True)
    mc, md = (nc, nd) if shared_input else (mask_in.clone().requires_grad_(True), mask_in.to(DEV).requires_grad_(True))
    ref = cpu(nc, mc)
    ref.backward(cot)
    n_paths, n0 = hip.torch_path_count(), hip.launch_count()
    out = dev(nd, md)
    out.backward(cot.to(DEV))
    assert hip.launch_count() >= n0 + 10 and hip.torch_path_count() == n_paths
    assert out.shape == ref.shape
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-4, atol=1e-5)
    _grad_close(nd.grad, nc.grad, "d net")
    if not shared_input:
        _grad_close(md.grad, mc.grad, "d mask_input")
    for (k, p), q in zip(dev.named_parameters(), cpu.parameters()):
        _grad_close(p.grad, q.grad, k)


@pytest.mark.parametrize("parallel", [True, False], ids=["parallel", "serial"])
def test_block_stack_on_an_unpadded_odd_width_input(parallel):
    """functional.mask_block_stack over a contiguous [B, 43] tensor (rows not 16-byte aligned, no padding columns): the result
    comes back 44 wide with a zero last column, the gradient of x 43 wide"""
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd.models.layers import MaskBlock
    torch.manual_seed(6)
    cpu = torch.nn.ModuleList(MaskBlock(43, 43, 43, 0.3) for _ in range(2))
    dev = copy.deepcopy(cpu).to(DEV)
    x, cot = torch.randn(37, 43) + 1.0, torch.randn(37, 43)
    xc, xd = x.clone().requires_grad_(True), x.to(DEV).requires_grad_(True)
    if parallel:
        ref = torch.stack([b(xc, xc) for b in cpu], dim=1).mean(dim=1)
    else:
        ref = xc
        for b in cpu:
            ref = b(ref, xc)
    ref.backward(cot)
    out = Fh.mask_block_stack(xd, dev, parallel)
    assert out.shape == (37, 44) and torch.count_nonzero(out[:, 43:]) == 0
    out.backward(torch.cat([cot, torch.zeros(37, 1)], dim=1).to(DEV))
    torch.testing.assert_close(out[:, :43].detach().cpu(), ref.detach(), rtol=1e-4, atol=1e-5)
    assert xd.grad.shape == (37, 43)
    _grad_close(xd.grad, xc.grad, "dx")
    for (k, p), q in zip(dev.named_parameters(), cpu.parameters()):
        _grad_close(p.grad, q.grad, k)


@pytest.fixture(params=["plan", "hipgraph"])
def backend(request, monkeypatch):
    monkeypatch.setenv("RP_GRAPH_BACKEND", request.param)
    return request.param


@pytest.mark.parametrize("parallel", [True, False], ids=["parallel", "serial"])
def test_graphed_step_is_bit_identical_to_the_eager_loop(parallel, backend):
    """default blocks and MLP (dropout 0.1 active), 40 steps: every prediction, loss, weight and optimizer moment of the
    replayed step equals the eager loop's; the step holds library launches only, so it replays as a launch plan"""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    from rec_pangu_amd.models.ranking import MaskNet
    from rec_pangu_amd.optim import FusedAdam
    steps = 40
    enc = _enc(5, [3000, 17, 900, 4, 20000, 250])
    batches = [_to_dev(b) for b in _batches(enc, 384, steps + 1, seed=4)]
    results = {}
    try:
        for mode in ("eager", "graph"):
            torch.manual_seed(0)
            model = MaskNet(embedding_dim=16, use_parallel=parallel, enc_dict=enc).to(DEV)
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
                if i % 7 == 0 or i > steps - 4:
                    preds.append(out["pred"].detach().clone())
                    losses.append(out["loss"].detach().clone())
            if gstep is not None:
                assert gstep.replays == steps - 2, "every step after the two eager ones must have been a graph replay"
                assert max(gstep._drop_calls) >= 1, "no dropout launch was captured"
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
