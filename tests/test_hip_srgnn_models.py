"""SRGNN, NISER and GCSAN on the GPU: against the golden vectors of the reference (the CPU test's bars and checks,
tests/test_srgnn_host.py), each against its own CPU path at (B, V, D, L) = (300, 5000, 64, 20) with lengths 1, L, 3, 2 and 0
in the first rows (the project's 1e-4 max(1e-2, max |ref|) per tensor), the fused Adam against torch.optim.Adam on the CPU
path, NISER's item_dropout in train mode, and the launch / torch-path counts of the default configurations."""
import math

import pytest
import torch

from conftest import load_golden, require_gpu
from test_srgnn_host import CASES, UNUSED, check_against_golden, run_case, within

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODELS = {"SRGNN": {}, "SRGNN step 2": {"step": 2}, "NISER": {"item_dropout": 0.0}, "GCSAN": {"hidden_size": 64},
          "GCSAN step 2": {"hidden_size": 64, "step": 2, "weight": 0.4}}


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


@pytest.mark.parametrize("case", list(CASES))
def test_model_on_the_device_matches_the_reference(case):
    require_gpu()
    from rec_pangu_amd import hip
    g = load_golden(f"model_{case}.npz")
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    check_against_golden(g, *run_case(case, g, device=DEV))
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0


def _mid_batch(B, V, L, seed=0):
    """right-padded histories of 0 .. L items over a vocabulary small enough for repeats inside a session; row 0 has length
    1, row 1 length L, row 2 length 3, row 3 length 2, row 4 none"""
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(1, V, (B, L), generator=gen)
    hist[B // 2:] = torch.randint(1, 12, (B - B // 2, L), generator=gen)  # (the upper half: repeated items and transitions)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0], lens[1], lens[2], lens[3], lens[4] = 1, L, 3, 2, 0
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return {"hist_item_list": hist * mask, "hist_mask_list": mask, "target_item": torch.randint(0, V, (B, 1), generator=gen)}


def _mid_model(name, V, D, L, seed=3, **cfg):
    from rec_pangu_amd.models import sequence
    torch.manual_seed(seed)
    return getattr(sequence, name.split()[0])({"item_id": {"vocab_size": V}}, dict(
        {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}, **cfg))


def _grads(model):
    return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", list(MODELS))
def test_device_against_its_cpu_path(name):
    """the kernels, not a fallback, produce the numbers: the library's launch count rises, the torch-path count does not"""
    require_gpu()
    from rec_pangu_amd import hip
    B, V, D, L = 300, 5000, 64, 20
    batch = _mid_batch(B, V, L)
    cpu, dev = _mid_model(name, V, D, L, **MODELS[name]).eval(), _mid_model(name, V, D, L, **MODELS[name]).eval().to(DEV)
    rc = cpu({k: v.clone() for k, v in batch.items()})
    rc["loss"].backward()
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    rd = dev({k: v.to(DEV) for k, v in batch.items()})
    rd["loss"].backward()
    torch.cuda.synchronize()
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0
    within(rd["user_emb"], rc["user_emb"].detach(), "user_emb")
    within(rd["loss"].reshape(1), rc["loss"].detach().reshape(1), "loss")
    gc, gd = _grads(cpu), _grads(dev)
    unused = set(UNUSED) if name.startswith("GCSAN") else set()
    assert set(gc) == set(gd) == set(dict(cpu.named_parameters())) - unused
    for k, v in gc.items():
        if k.endswith("multi_head_attention.key.bias"):
            # exactly zero in exact arithmetic (tests/test_sasrec_host.py): rounding noise on both sides, held to the key
            # weight's scale
            ref = gc[k.replace("key.bias", "key.weight")]
            assert float((gd[k] - v).abs().max()) <= bar(ref), k
            continue
        within(gd[k], v, f"grad {k}")
    if name.startswith("GCSAN"):
        assert float(rd["user_emb"][4].abs().max()) == 0.0  # the row without history


@pytest.mark.parametrize("name", ["SRGNN", "NISER", "GCSAN"])
def test_two_fused_adam_steps_against_torch_adam_on_the_cpu(name):
    """Bound per element, derived as in tests/test_hip_gru_models.py: atol 1e-6 + rtol 1e-4 (equal gradients)
    plus what Adam makes of a gradient that differs within the project's bar d = 1e-4 max(1e-2, max |g|) of its tensor: step 1
    moves by lr g / (|g| + eps), insensitive to g's size; step 2 by lr f(g2 / g1) with |r f'(r)| < 1, so relative errors e1, e2
    of the two gradients shift it by at most lr (e1 + e2), e_i <= d_i / |g_i| — capped at 2 lr, the most two steps can differ."""
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    B, V, D, L, lr = 64, 500, 16, 7, 1e-2
    cfg = dict(MODELS[name], hidden_size=D) if name == "GCSAN" else MODELS[name]
    batch = _mid_batch(B, V, L)
    cpu, dev = _mid_model(name, V, D, L, **cfg).eval(), _mid_model(name, V, D, L, **cfg).eval().to(DEV)
    opt_c = torch.optim.Adam(cpu.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    opt_d = make_adam(dev, lr)
    slack = {k: torch.zeros_like(p) for k, p in cpu.named_parameters()}
    for _ in range(2):
        cpu({k: v.clone() for k, v in batch.items()})["loss"].backward()
        for k, p in cpu.named_parameters():
            if p.grad is not None:
                slack[k] += lr * bar(p.grad) / p.grad.abs().clamp(min=1e-30)
        opt_c.step()
        cpu.zero_grad()
        dev({k: v.to(DEV) for k, v in batch.items()})["loss"].backward()
        opt_d.step()
        dev.zero_grad()
    for (k, a), b in zip(cpu.state_dict().items(), dev.state_dict().values()):
        tol = 1e-6 + 1e-4 * a.abs() + slack[k].clamp(max=2 * lr)
        over = ((b.detach().cpu() - a).abs() - tol).max()
        print(f"{k}: worst excess over the bound {float(over):.3g}")
        assert float(over) <= 0, k


def test_niser_item_dropout_in_train_mode_is_reproducible_and_on_the_kernels():
    require_gpu()
    from rec_pangu_amd import hip
    batch = {k: v.to(DEV) for k, v in _mid_batch(64, 500, 20).items()}
    dev = _mid_model("NISER", 500, 32, 20, item_dropout=0.3).to(DEV).train()
    runs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        dev.zero_grad()
        n0, t0 = hip.launch_count(), hip.torch_path_count()
        res = dev({k: v.clone() for k, v in batch.items()})
        res["loss"].backward()
        torch.cuda.synchronize()
        assert hip.launch_count() > n0 and hip.torch_path_count() == t0 and math.isfinite(float(res["loss"]))
        runs.append([res["user_emb"].detach().clone(), res["loss"].detach().clone()] + list(_grads(dev).values()))
        assert all(bool(torch.isfinite(t).all()) for t in runs[-1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))  # equal generator state: equal bits
    assert not torch.equal(runs[0][0], runs[2][0])
    dev.eval()
    with torch.no_grad():
        a = dev(batch, is_training=False)["user_emb"]
        b = dev(batch, is_training=False)["user_emb"]
    assert torch.equal(a, b) and not torch.equal(a, runs[0][0])


@pytest.mark.parametrize("name", ["SRGNN", "NISER", "GCSAN"])
def test_the_default_configuration_uses_no_torch_path(name):
    require_gpu()
    from rec_pangu_amd import hip
    batch = {k: v.to(DEV) for k, v in _mid_batch(32, 200, 50).items()}
    dev = _mid_model(name, 200, 64, 50, **({"hidden_size": 64} if name == "GCSAN" else {})).to(DEV)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    res = dev(batch)
    res["loss"].backward()
    torch.cuda.synchronize()
    # the graph, the node rows, one cell step each way (2 + at least 6), the readout, the loss head
    assert hip.torch_path_count() == t0 and hip.launch_count() - n0 >= 1 + 1 + 2 + 6
    assert bool(torch.isfinite(res["user_emb"]).all())
    # the encoder alone: the graph 1 launch, a step 2 forward
    n0 = hip.launch_count()
    with torch.no_grad():
        alias, hidden = dev.node_rows(batch["hist_item_list"], False)
        n1 = hip.launch_count()
        dev.gnncell.encode(alias, hidden, 2)
    assert hip.launch_count() - n1 == 4 and hip.torch_path_count() == t0
