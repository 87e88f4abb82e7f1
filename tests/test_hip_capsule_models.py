"""MIND and ComirecDR on the GPU: against the golden vectors of the reference (the CPU test's bars,
tests/test_capsule_host.py; MIND is fed the recorded initial logits), against their own CPU path at
(B, V, D, L, K) = (300, 5000, 64, 20, 4) on the same weights and logits (the project's 1e-4 max(1e-2, max |ref|) per
tensor), the fused Adam against torch.optim.Adam on the CPU path, a batch of one, and a SequenceTrainer epoch each with the
recall metrics of the multi-interest branch.

The readout picks one interest per row, and an fp32 rounding may pick another where the two best scores nearly tie.  Every
comparison here therefore runs on data whose top-two gap is at least 1e-3 max |score| in EVERY row, computed in float64 from
the CPU path's interests and ASSERTED in the test: gapped_batch redraws, from its seeded generator, the rows that miss twice
that (MIND's interests share their rows and differ by the initial logits alone, so among 300 random rows some always tie)."""
import functools
import math

import pytest
import torch

from conftest import load_golden, require_gpu
from test_capsule_host import CASES, feed_logits, run_case
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
    check_against_golden(g, *run_case(case, g, device="cuda:0", feed=True))
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0


@pytest.mark.parametrize("case", ["mind_train", "comirecdr"])
def test_model_with_the_fused_adam_matches_the_reference(case):
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    g = load_golden(f"model_{case}.npz")
    check_against_golden(g, *run_case(case, g, device="cuda:0", make_opt=lambda m: make_adam(m, 1e-2), feed=True))


def mid_model(name, V, D, L, K, seed=3):
    """the model as the reference initialises it — except ComirecDR's `w`: kaiming_normal_ takes the fan-in of the
    [1, L, K D, D] parameter for K D D, the projected rows come out near 1e-3 and the squashed interests near 1e-7, where the
    bar's floor (1e-4 * 1e-2) would pass anything.  Redrawn at std sqrt(2 / D) the interests are O(0.1) and the bar binds."""
    from rec_pangu_amd.models import sequence
    torch.manual_seed(seed)
    model = getattr(sequence, name)({"item_id": {"vocab_size": V}}, {"embedding_dim": D, "max_length": L, "device": "cpu",
                                                                      "item_col": "item_id", "cate_cols": [], "K": K})
    if name == "ComirecDR":
        with torch.no_grad():
            model.capsule.w.normal_(0.0, (2.0 / D) ** 0.5)
    return model


def row_gaps(model, res, batch):
    """(best - second best readout score) / max |score| of EVERY row, in float64 from the given interests"""
    e = model.item_emb.weight.detach().cpu().double()[batch["target_item"].view(-1)]
    s = torch.bmm(res["user_emb"].detach().cpu().double(), e.unsqueeze(-1)).squeeze(-1)
    top = torch.sort(s, dim=1, descending=True).values
    assert top.shape[0] == batch["target_item"].shape[0]
    return (top[:, 0] - top[:, 1]) / s.abs().max()


@functools.lru_cache(maxsize=None)
def gapped_batch(name, B, V, D, L, K, steps, seed=0):
    """Right-padded histories of 1 .. L items (row 0 has length 1, row 1 length L, row 2 an id 0 inside it), targets, and the
    initial logits MIND feeds to both paths, one set per training step.  The CPU path of mid_model(name, ...) is stepped
    `steps` times with torch's Adam (lr 1e-2); the history and the logits of every row whose top-two gap falls under
    2e-3 max |score| in any step are redrawn from the same generator until no row is left (the tests assert 1e-3 on their own
    CPU run, for all rows)."""
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(1, V, (B, L), generator=gen)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0], lens[1], lens[2] = 1, L, 3
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    hist = hist * mask
    hist[2, 1] = 0
    batch = {"hist_item_list": hist, "hist_mask_list": mask, "target_item": torch.randint(0, V, (B, 1), generator=gen)}
    logits = [torch.randn(B, K, L, generator=gen) for _ in range(steps)]
    for _ in range(200):
        cpu = mid_model(name, V, D, L, K)
        opt = torch.optim.Adam(cpu.parameters(), lr=1e-2)
        feed_logits(cpu, logits, "cpu")
        worst = torch.full((B,), float("inf"), dtype=torch.float64)
        for _ in range(steps):
            res = cpu({k: v.clone() for k, v in batch.items()})
            worst = torch.minimum(worst, row_gaps(cpu, res, batch))
            if steps > 1:
                res["loss"].backward()
                opt.step()
                cpu.zero_grad()
        bad = worst < 2e-3
        if not bool(bad.any()):
            return batch, logits
        n = int(bad.sum())
        hist[bad] = torch.randint(1, V, (n, L), generator=gen) * mask[bad]
        hist[2, 1] = 0
        for t in logits:
            t[bad] = torch.randn(n, K, L, generator=gen)
    raise AssertionError("no gapped batch found")


@pytest.mark.parametrize("name", ["MIND", "ComirecDR"])
def test_device_against_its_cpu_path(name):
    """the kernels, not a fallback, produce the numbers: the library's launch count rises, the torch-path count does not"""
    require_gpu()
    from rec_pangu_amd import hip
    B, V, D, L, K = 300, 5000, 64, 20, 4
    batch, logits = gapped_batch(name, B, V, D, L, K, 1)
    cpu, dev = mid_model(name, V, D, L, K), mid_model(name, V, D, L, K).to("cuda:0")
    for (k, a), b in zip(cpu.state_dict().items(), dev.state_dict().values()):
        assert torch.equal(a, b.cpu()), k
    feed_logits(cpu, logits, "cpu"), feed_logits(dev, logits, "cuda:0")
    rc = cpu({k: v.clone() for k, v in batch.items()})
    gap = float(row_gaps(cpu, rc, batch).min())
    print(f"{name}: top-two gap of the CPU path's readout scores, worst of {B} rows: {gap:.3g} of max |score|")
    assert gap >= 1e-3
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
        if p.grad is None:
            assert k == "capsule.relu.0.weight" and grads[k].grad is None
        else:
            within(grads[k].grad, p.grad, f"{name}: grad {k}")


@pytest.mark.parametrize("name", ["MIND", "ComirecDR"])
def test_two_fused_adam_steps_against_torch_adam_on_the_cpu(name):
    """Bound per element as in tests/test_hip_gru_models.py: atol 1e-6 + rtol 1e-4 (for equal gradients) plus what Adam makes
    of a gradient that differs within the project's bar d = 1e-4 max(1e-2, max |g|) of its tensor.  Step 1 moves by
    lr g / (|g| + eps), insensitive to g's size; step 2 by lr f(g2 / g1) with |r f'(r)| < 1, so a relative error e1, e2 of the
    two gradients shifts it by at most lr (e1 + e2), e_i <= d_i / |g_i| — capped at 2 lr, the most two steps can differ.  The
    top-two gap of the readout is asserted in front of both steps."""
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    B, V, D, L, K, lr = 64, 500, 16, 5, 3, 1e-2
    batch, logits = gapped_batch(name, B, V, D, L, K, 2)
    cpu, dev = mid_model(name, V, D, L, K), mid_model(name, V, D, L, K).to("cuda:0")
    feed_logits(cpu, logits, "cpu"), feed_logits(dev, logits, "cuda:0")
    opt_c = torch.optim.Adam(cpu.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    opt_d = make_adam(dev, lr)
    slack = {k: torch.zeros_like(p) for k, p in cpu.named_parameters()}
    for _ in range(2):
        rc = cpu({k: v.clone() for k, v in batch.items()})
        assert float(row_gaps(cpu, rc, batch).min()) >= 1e-3
        rc["loss"].backward()
        for k, p in cpu.named_parameters():
            if p.grad is not None:
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


@pytest.mark.parametrize("name", ["MIND", "ComirecDR"])
def test_a_batch_of_one_trains_on_the_device(name):
    require_gpu()
    from rec_pangu_amd import hip
    dev = mid_model(name, 50, 8, 6, 3).to("cuda:0")
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0]]),
            "target_item": torch.tensor([[5]])}
    t0 = hip.torch_path_count()
    res = dev({k: v.to("cuda:0") for k, v in data.items()})
    assert res["user_emb"].shape == (1, 3, 8) and res["loss"].dim() == 0
    res["loss"].backward()
    torch.cuda.synchronize()
    assert hip.torch_path_count() == t0 and math.isfinite(float(res["loss"].detach()))
    for k, p in dev.named_parameters():
        if k != "capsule.relu.0.weight":
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    with pytest.raises(ValueError, match="max_length"):
        dev({k: v[:, :5].to("cuda:0") if k != "target_item" else v.to("cuda:0") for k, v in data.items()})


def test_a_target_outside_the_table_raises_at_the_loss():
    require_gpu()
    dev = mid_model("ComirecDR", 50, 8, 6, 3).to("cuda:0")
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0]]),
            "target_item": torch.tensor([[50]])}
    with pytest.raises(IndexError):
        dev({k: v.to("cuda:0") for k, v in data.items()})
    data["target_item"][0, 0] = 49
    assert math.isfinite(float(dev({k: v.to("cuda:0") for k, v in data.items()})["loss"].detach()))  # (the flag was cleared)


@pytest.mark.parametrize("name", ["MIND", "ComirecDR"])
def test_sequence_trainer_epoch_on_the_device(name, tmp_path):
    require_gpu()
    from rec_pangu_amd import hip
    from rec_pangu_amd.models import sequence
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, test = _tiny_loaders()
    torch.manual_seed(0)
    model = getattr(sequence, name)(enc, dict(cfg, device="cuda:0", K=2))
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    trainer.fit(model, train, valid, epoch=1, lr=1e-2, device=torch.device("cuda:0"), topk_list=[5, 10])
    assert hip.torch_path_count() == t0 and hip.launch_count() > n0
    assert model.item_emb.weight.is_cuda and len(trainer.log_df) == 1
    row = trainer.log_df.iloc[0]
    assert all(math.isfinite(float(row[k])) and 0.0 <= float(row[k]) <= 1.0 for k in ("recall@10", "ndcg@10", "hitrate@10"))
    metric = trainer.evaluate_model(model, test, torch.device("cuda:0"), topk_list=[5])
    assert all(math.isfinite(v) for k, v in metric.items() if k != "phase")
