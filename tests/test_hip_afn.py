"""AFN on the HIP path: the reference's golden vectors in every matrix-core mode (the MLPs' GEMMs; the logarithmic net is fp32
FMA with logf / expf), a Criteo-shaped batch against the model's own CPU path (pinned to the reference by
tests/test_afn_host.py) with batch and with running statistics, no torch path, a neuron count outside hip.lognet_fits on torch
ops, and the captured training step — as a launch plan and as a hipGraph — bit-identical to the eager loop, parameters,
optimizer moments and both BatchNorms' buffers.

With batch statistics log_batch_norm.bias has no real gradient (tests/test_afn_host.py's docstring): that gradient is judged
against the bar of log_batch_norm.weight's gradient; the parameter, and exp_batch_norm's running buffers which a shift of it
scales, are left out of the after-Adam comparison; the after-Adam inference output is compared in the eval cases only."""
import copy
import functools
import warnings

import pytest
import torch

from conftest import load_golden, require_gpu
from test_afn_host import BN1_BIAS, CASES, TRAIN_SKIP, build

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


def _grad_close(got, ref, what, bar_of=None):
    tol = 1e-4 * max(1e-2, float((ref if bar_of is None else bar_of).abs().max()))
    err = float((got.cpu() - ref).abs().max())
    assert err <= tol, f"{what}: {err} > {tol}"
    return err / tol


def _grads_close(model, rgrads, train_mode, what):
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        assert p.grad is not None and rgrads[k] is not None, k
        r = _grad_close(p.grad, rgrads[k], f"{what}: grad {k}",
                        bar_of=rgrads["log_batch_norm.weight"] if (train_mode and k == BN1_BIAS) else None)
        if r > worst[1]:
            worst = (k, r)
    print(f"{what} worst gradient error / bar: {worst[1]:.3g} ({worst[0]})")


@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_adam_vs_reference(name, matmul_mode):
    from rec_pangu_amd import hip
    from rec_pangu_amd.optim import FusedAdam, make_adam
    train_mode = CASES[name][1]
    g = load_golden(f"model_{name}.npz")
    model = build(name).to(DEV)
    assert model.hip_supported()
    n0, n_paths = hip.launch_count(), hip.torch_path_count()
    out = model(_to_dev(g["batch"]))
    assert hip.launch_count() > n0 and hip.torch_path_count() == n_paths, "the HIP kernels did not run"
    for k, v in g["out"].items():
        print(f"{name} {matmul_mode} {k}: {float((out[k].detach().cpu() - v).abs().max()):.3g}")
        torch.testing.assert_close(out[k].detach().cpu(), v, rtol=1e-4, atol=1e-5, msg=lambda m: f"{name}:{k}: {m}")
    model.zero_grad()
    out["loss"].backward()
    assert set(g["grad"]) == {k for k, p in model.named_parameters() if p.grad is not None}
    _grads_close(model, g["grad"], train_mode, f"{name} {matmul_mode}")
    sd = model.state_dict()
    for k, v in g["after1"].items():
        if v.is_floating_point():
            _grad_close(sd[k], v, f"{name}: after1 {k}")
        else:
            assert int(sd[k]) == int(v), k
    # two FusedAdam steps, then the inference output
    model = build(name).to(DEV)
    opt = make_adam(model, 1e-2)
    assert isinstance(opt, FusedAdam)
    for _ in range(2):
        r = model(_to_dev(g["batch"]))
        r["loss"].backward()
        opt.step()
        model.zero_grad()
    sd = model.state_dict()
    assert list(sd) == list(g["adam2"])
    worst = 0.0
    for k, v in g["adam2"].items():
        if train_mode and k in TRAIN_SKIP:
            continue
        if not v.is_floating_point():
            assert int(sd[k]) == int(v), k
            continue
        tol = 2e-4 * max(1e-2, float(v.abs().max()))
        err = float((sd[k].cpu() - v).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, f"{name}: {k} off by {err} after two Adam steps (tol {tol})"
    print(f"{name} {matmul_mode} worst weight error / bar: {worst:.3g}")
    n_paths = hip.torch_path_count()
    model.eval()
    with torch.no_grad():
        r = model(_to_dev(g["batch"]), is_training=False)
    assert "loss" not in r and hip.torch_path_count() == n_paths
    if not train_mode:
        for k, v in g["adam2_out"].items():
            torch.testing.assert_close(r[k].cpu(), v, rtol=1e-3, atol=1e-4)


@functools.lru_cache(maxsize=None)
def _criteo(train_mode):
    """the Criteo-shaped CPU model (26 sparse fields, cardinalities / 64, D = 32, L = 5, dropout at 0), its batch of 512 and the
    CPU result with every gradient and the buffers after the step: computed once per mode, left unchanged.  Eval mode at the
    initial running statistics (0, 1) feeds an unnormalised log|e| into exp and saturates the prediction, so both BatchNorms
    first take their running statistics from one batch (momentum 1 for one training forward)."""
    from rec_pangu_amd.models.ranking import AFN
    card = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306,
            10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]
    enc = {f"I{i + 1}": {"min": 0.0, "max": 1.0} for i in range(13)}
    enc.update({f"C{i + 1}": {"vocab_size": max(2, c // 64)} for i, c in enumerate(card)})
    torch.manual_seed(0)
    cpu = AFN(enc_dict=enc)
    assert cpu.coefficient_W.weight.shape == (5, 26) and cpu.dense_layer.net[0].weight.shape == (64, 5 * 32)
    for m in cpu.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    gen = torch.Generator().manual_seed(1)
    B = 512
    batch = {f"I{i + 1}": torch.rand(B, generator=gen) for i in range(13)}
    batch.update({f"C{i + 1}": torch.randint(0, enc[f"C{i + 1}"]["vocab_size"] + 1, (B,), generator=gen) for i in range(26)})
    batch["label"] = (torch.rand(B, generator=gen) < 0.25).float()
    if not train_mode:
        cpu.train()
        for bn in (cpu.log_batch_norm, cpu.exp_batch_norm):
            bn.momentum = 1.0
        with torch.no_grad():
            cpu(batch)
        for bn in (cpu.log_batch_norm, cpu.exp_batch_norm):
            bn.momentum = 0.1
    cpu.train(train_mode)
    start = copy.deepcopy(cpu)
    ref = cpu(batch)
    ref["loss"].backward()
    ref = {k: v.detach() for k, v in ref.items()}
    assert 1e-3 < float(ref["pred"].min()) and float(ref["pred"].max()) < 1 - 1e-3
    return start, cpu, batch, ref


@pytest.mark.parametrize("train_mode", [True, False], ids=["train", "eval"])
def test_criteo_shape_vs_the_cpu_path(train_mode):
    """pred, loss, every gradient and both BatchNorms' buffers against the model's CPU path, in the library's default
    matrix-core mode (auto: exact products where a launch is bound by its traffic, as every GEMM of this step is).  Not in
    bf16x3: dE = dx / e makes the element with the smallest |e| the maximum of its table's gradient, so the bar measures the
    RELATIVE error of one element of the MLP's input gradient — a cancelling dot product that three bf16 products per flop
    (2^-16 each) do not carry to 1e-4 (measured: 0.35 of the bar with batch statistics, 1.33 with running statistics; 0.04 in
    auto and bf16x6).  The golden fixtures above run in all three modes."""
    from rec_pangu_amd import hip
    matmul_mode = hip.get_matmul_precision()
    start, cpu, batch, ref = _criteo(train_mode)
    model = copy.deepcopy(start).to(DEV)
    model.zero_grad()
    assert model.hip_supported() and model.training == train_mode
    n0, n_paths = hip.launch_count(), hip.torch_path_count()
    out = model(_to_dev(batch))
    out["loss"].backward()
    assert hip.launch_count() > n0 and hip.torch_path_count() == n_paths
    what = f"criteo {'train' if train_mode else 'eval'} {matmul_mode}"
    for k in ("pred", "loss"):
        print(f"{what} {k}: {float((out[k].detach().cpu() - ref[k]).abs().max()):.3g}")
        torch.testing.assert_close(out[k].detach().cpu(), ref[k], rtol=1e-4, atol=1e-5)
    _grads_close(model, {k: p.grad for k, p in cpu.named_parameters()}, train_mode, what)
    sd, rsd = model.state_dict(), cpu.state_dict()
    for k in rsd:
        if "running_" in k:
            _grad_close(sd[k], rsd[k], f"{what}: {k}")
        elif "num_batches" in k:
            assert int(sd[k]) == int(rsd[k]), k


def test_default_constructor_takes_no_torch_path(monkeypatch):
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.ranking import AFN
    monkeypatch.setenv("RP_STRICT_HIP", "1")
    enc = _enc(3, [7, 3, 1000, 11, 90, 5])
    torch.manual_seed(0)
    model = AFN(enc_dict=enc).to(DEV)
    model.train()
    n_paths, n0 = hip.torch_path_count(), hip.launch_count()
    out = model(_to_dev(_batches(enc, 64, 1, seed=3)[0]))
    out["loss"].backward()
    assert hip.torch_path_count() == n_paths and hip.launch_count() > n0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert int(model.log_batch_norm.num_batches_tracked) == 1 and int(model.exp_batch_norm.num_batches_tracked) == 1


def test_a_neuron_count_outside_the_range_runs_on_torch_ops_and_matches_the_cpu():
    """L = 9: outside hip.lognet_fits.  The model composes the logarithmic net from device ops, says so (exactly one counted
    torch path), and agrees with its CPU copy"""
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.ranking import AFN
    enc = _enc(2, [7, 3, 1000, 11, 90])
    torch.manual_seed(2)
    cpu = AFN(embedding_dim=8, dnn_hidden_units=[8], afn_hidden_units=[8], logarithmic_neurons=9, enc_dict=enc)
    assert not cpu.hip_supported()
    for m in cpu.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    cpu.train()
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
    _grads_close(model, {k: p.grad for k, p in cpu.named_parameters()}, True, "L = 9 on torch ops")


@pytest.fixture(params=["plan", "hipgraph"])
def backend(request, monkeypatch):
    monkeypatch.setenv("RP_GRAPH_BACKEND", request.param)
    return request.param


def test_graphed_step_is_bit_identical_to_the_eager_loop(backend):
    """6 sparse + 5 dense, D = 16, L = 5, B = 384, 5 steps (two eager, three replayed): every prediction, loss, weight, optimizer
    moment and BatchNorm buffer of the replayed step equals the eager loop's; the step holds library launches only, so it
    replays as a launch plan.  Dropout is active (the reference's 0.1, on the device clock) in the plan case and 0 in the
    hipGraph case."""
    from rec_pangu_amd import hip
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    from rec_pangu_amd.models.ranking import AFN
    from rec_pangu_amd.optim import FusedAdam
    steps = 5
    enc = _enc(5, [3000, 17, 900, 4, 20000, 250])
    batches = [_to_dev(b) for b in _batches(enc, 384, steps + 1, seed=4)]
    results = {}
    n_paths = hip.torch_path_count()
    try:
        for mode in ("eager", "graph"):
            torch.manual_seed(0)
            model = AFN(embedding_dim=16, enc_dict=enc).to(DEV)
            for m in model.modules():
                if hasattr(m, "check_indices"):
                    m.check_indices = "deferred"
                if isinstance(m, torch.nn.Dropout) and backend == "hipgraph":
                    m.p = 0.0
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
                    assert gstep.backend_used == "plan" and gstep.why_not_plan is None, (gstep.backend_used, gstep.why_not_plan)
                else:
                    assert gstep.backend_used == "hipgraph"
            model.embedding_layer.raise_if_bad_index()
            model.embedding_layer2.raise_if_bad_index()
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            osd = opt.state_dict()
            results[mode] = (preds, losses, sd,
                             [{k: v.clone() for k, v in st.items() if torch.is_tensor(v)} for st in osd["state"].values()])
    finally:
        EmbeddingLayer.unpin_sorts()
    assert hip.torch_path_count() == n_paths
    e, g = results["eager"], results["graph"]
    assert all(torch.isfinite(p).all() for p in e[0])
    assert int(e[2]["log_batch_norm.num_batches_tracked"]) == steps and int(e[2]["exp_batch_norm.num_batches_tracked"]) == steps
    for a, b in zip(e[0], g[0]):
        assert torch.equal(a, b), "predictions differ"
    for a, b in zip(e[1], g[1]):
        assert torch.equal(a, b), "losses differ"
    for k in e[2]:
        assert torch.equal(e[2][k], g[2][k]), k
    for sa, sb in zip(e[3], g[3]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"optimizer state {k}"
