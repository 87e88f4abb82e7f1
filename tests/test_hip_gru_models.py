"""GRU4Rec and NARM on the GPU: against the golden vectors of the reference (the CPU test's bars, tests/test_gru_host.py),
against their own CPU path at (B, V, D, L) = (300, 5000, 64, 20) (the project's 1e-4 max(1e-2, max |ref|) per tensor), a batch
with an empty row, the fused Adam against torch.optim.Adam on the CPU path, the torch path above the kernels' widths, and a
SequenceTrainer epoch each."""
import math
import warnings

import pytest
import torch

from conftest import load_golden, require_gpu
from test_gru_host import CASES, run_case
from test_sequence_host import _tiny_loaders, check_against_golden

pytestmark = pytest.mark.gpu


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def within(got, ref, what):
    err = float((got.detach().cpu().double() - ref.double()).abs().max())
    print(f"{what}: max err {err:.3g} against bar {bar(ref):.3g}")
    assert got.shape == ref.shape and err <= bar(ref), (what, err, bar(ref))


@pytest.mark.parametrize("case", list(CASES))
def test_model_on_the_device_matches_the_reference(case):
    require_gpu()
    from rec_pangu_amd import hip
    g = load_golden(f"model_{case}.npz")
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    check_against_golden(g, *run_case(case, g, device="cuda:0"))
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0


@pytest.mark.parametrize("case", ["gru4rec", "narm_train"])
def test_model_with_the_fused_adam_matches_the_reference(case):
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    g = load_golden(f"model_{case}.npz")
    check_against_golden(g, *run_case(case, g, device="cuda:0", make_opt=lambda m: make_adam(m, 1e-2)))


def _mid_batch(B, V, L, narm, seed=0, empty_row=False):
    """right-padded histories of 1 .. L items (the CPU path raises for an empty one); row 0 has length 1, row 1 length L; for
    NARM an id 0 in front of len (row 2) and a non-zero id behind it (row 3)"""
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(1, V, (B, L), generator=gen)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0], lens[1], lens[2], lens[3] = 1, L, 3, 2
    if empty_row:
        lens[4] = 0
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    hist = hist * mask
    if narm:
        hist[2, 1], hist[3, 4] = 0, 7
    return {"hist_item_list": hist, "hist_mask_list": mask, "target_item": torch.randint(0, V, (B, 1), generator=gen)}


def _mid_model(name, V, D, L, seed=3, **cfg):
    from rec_pangu_amd.models import sequence
    torch.manual_seed(seed)
    return getattr(sequence, name)({"item_id": {"vocab_size": V}}, dict(
        {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}, **cfg))


MODELS = {"GRU4Rec": {}, "NARM": {"hidden_size": 32, "dropout_probs": [0, 0]}}


@pytest.mark.parametrize("name", list(MODELS))
def test_device_against_its_cpu_path(name):
    """the kernels, not a fallback, produce the numbers: the library's launch count rises, the torch-path count does not"""
    require_gpu()
    from rec_pangu_amd import hip
    B, V, D, L = 300, 5000, 64, 20
    batch = _mid_batch(B, V, L, name == "NARM")
    cpu = _mid_model(name, V, D, L, **MODELS[name])
    dev = _mid_model(name, V, D, L, **MODELS[name]).to("cuda:0")
    for (k, a), b in zip(cpu.state_dict().items(), dev.state_dict().values()):
        assert torch.equal(a, b.cpu()), k
    rc = cpu({k: v.clone() for k, v in batch.items()})
    rc["loss"].backward()
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    rd = dev({k: v.to("cuda:0") for k, v in batch.items()})
    rd["loss"].backward()
    torch.cuda.synchronize()
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0
    within(rd["user_emb"], rc["user_emb"].detach(), f"{name}: user_emb")
    within(rd["loss"].reshape(1), rc["loss"].detach().reshape(1), f"{name}: loss")
    grads = dict(dev.named_parameters())
    for k, p in cpu.named_parameters():
        within(grads[k].grad, p.grad, f"{name}: grad {k}")


@pytest.mark.parametrize("name", list(MODELS))
def test_a_row_without_history_gives_a_zero_user_emb(name):
    require_gpu()
    B, V, D, L = 40, 200, 16, 6
    batch = _mid_batch(B, V, L, name == "NARM", empty_row=True)
    assert int(batch["hist_mask_list"][4].sum()) == 0 and int(batch["hist_item_list"][4].abs().sum()) == 0
    dev = _mid_model(name, V, D, L, **MODELS[name]).to("cuda:0")
    res = dev({k: v.to("cuda:0") for k, v in batch.items()})
    res["loss"].backward()
    torch.cuda.synchronize()
    assert float(res["user_emb"][4].detach().abs().max()) == 0.0 and float(res["user_emb"][3].detach().abs().max()) > 0
    assert math.isfinite(float(res["loss"].detach())) and all(torch.isfinite(p.grad).all() for p in dev.parameters())


@pytest.mark.parametrize("name", list(MODELS))
def test_two_fused_adam_steps_against_torch_adam_on_the_cpu(name):
    """Bound per element: atol 1e-6 + rtol 1e-4 (tests/test_hip_sequence.py's, for equal gradients) plus what Adam makes of a
    gradient that differs within the project's bar d = 1e-4 max(1e-2, max |g|) of its tensor.  Step 1 moves by
    lr g / (|g| + eps), insensitive to g's size (d u / d g = lr eps / (|g| + eps)^2, below 1e-12 here).  Step 2 moves by
    lr f(g2 / g1) with f(r) = (0.4737 + 0.5263 r) / sqrt(0.49975 + 0.50025 r^2) and |r f'(r)| < 1, so a relative error e1, e2 of
    the two gradients shifts it by at most lr (e1 + e2), e_i <= d_i / |g_i| — capped at 2 lr, the most two steps can differ."""
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    B, V, D, L, lr = 64, 500, 16, 5, 1e-2
    batch = _mid_batch(B, V, L, name == "NARM")
    cpu, dev = _mid_model(name, V, D, L, **MODELS[name]), _mid_model(name, V, D, L, **MODELS[name]).to("cuda:0")
    opt_c = torch.optim.Adam(cpu.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    opt_d = make_adam(dev, lr)
    slack = {k: torch.zeros_like(p) for k, p in cpu.named_parameters()}
    for _ in range(2):
        cpu({k: v.clone() for k, v in batch.items()})["loss"].backward()
        for k, p in cpu.named_parameters():
            slack[k] += lr * bar(p.grad) / p.grad.abs().clamp(min=1e-30)
        opt_c.step()
        cpu.zero_grad()
        dev({k: v.to("cuda:0") for k, v in batch.items()})["loss"].backward()
        opt_d.step()
        dev.zero_grad()
    for (k, a), b in zip(cpu.state_dict().items(), dev.state_dict().values()):
        tol = 1e-6 + 1e-4 * a.abs() + slack[k].clamp(max=2 * lr)
        over = ((b.detach().cpu() - a).abs() - tol).max()
        tight = int(((b.detach().cpu() - a).abs() <= 1e-6 + 1e-4 * a.abs()).sum())
        print(f"{name}: {k}: {tight} of {a.numel()} elements within rtol 1e-4 / atol 1e-6, worst excess over the bound {float(over):.3g}")
        assert float(over) <= 0, k


def test_narm_with_its_default_dropouts_runs_on_the_kernels():
    """emb_dropout active: the rows go through the lookup launch and the library's dropout into the dense-input recurrence"""
    require_gpu()
    from rec_pangu_amd import hip
    batch = _mid_batch(64, 500, 5, True)
    dev = _mid_model("NARM", 500, 16, 5).to("cuda:0").train()
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    res = dev({k: v.to("cuda:0") for k, v in batch.items()})
    res["loss"].backward()
    torch.cuda.synchronize()
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0 and math.isfinite(float(res["loss"]))
    g = dev.item_emb.weight.grad  # (row 0 included: the loss head gives it a gradient, the lookup does not)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_a_hidden_width_of_160_takes_the_torch_path_and_says_so_once():
    require_gpu()
    from rec_pangu_amd import hip
    batch = _mid_batch(16, 50, 5, True)
    dev = _mid_model("NARM", 50, 8, 5, hidden_size=160, dropout_probs=[0, 0]).to("cuda:0")
    cpu = _mid_model("NARM", 50, 8, 5, hidden_size=160, dropout_probs=[0, 0])
    t0 = hip.torch_path_count()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            rd = dev({k: v.to("cuda:0") for k, v in batch.items()})
    said = [w for w in seen if "gru_encode at in=8, H=160" in str(w.message)]
    assert len(said) == 1 and hip.torch_path_count() >= t0 + 2
    within(rd["user_emb"], cpu(batch)["user_emb"].detach(), "H=160: user_emb")


@pytest.mark.parametrize("name", list(MODELS))
def test_sequence_trainer_epoch_on_the_device(name, tmp_path):
    require_gpu()
    from rec_pangu_amd import hip
    from rec_pangu_amd.models import sequence
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, test = _tiny_loaders()
    torch.manual_seed(0)
    model = getattr(sequence, name)(enc, dict(cfg, device="cuda:0"))
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    trainer.fit(model, train, valid, epoch=1, lr=1e-2, device=torch.device("cuda:0"), topk_list=[5, 10])
    assert hip.torch_path_count() == t0 and hip.launch_count() > n0
    assert model.item_emb.weight.is_cuda and len(trainer.log_df) == 1
    row = trainer.log_df.iloc[0]
    assert all(math.isfinite(float(row[k])) and 0.0 <= float(row[k]) <= 1.0 for k in ("recall@10", "ndcg@10", "hitrate@10"))
    metric = trainer.evaluate_model(model, test, torch.device("cuda:0"), topk_list=[5])
    assert all(math.isfinite(v) for k, v in metric.items() if k != "phase")
