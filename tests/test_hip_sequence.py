"""The sequence-recall family on the GPU: the masked history mean alone against float64, YotubeDNN on the device against the
golden vectors of the reference and against its own CPU path, the fused Adam on a model without an EmbeddingLayer, the
device search of get_recall_predict against the CPU one, and a SequenceTrainer epoch.

Bars: the kernel-level and device-against-CPU comparisons use the project's 1e-4 max(1e-2, max |ref|) per tensor; the golden
comparison uses the CPU test's bars (tests/test_sequence_host.py)."""
import pytest
import torch

from conftest import load_golden, require_gpu
from test_sequence_host import (StubRecallModel, _tiny_loaders, check_against_golden, expected_preds, gapped_recall_data,
                                recall_loader, run_case)

pytestmark = pytest.mark.gpu


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def within(got, ref, what):
    err = float((got.detach().cpu().double() - ref.double()).abs().max())
    print(f"{what}: max err {err:.3g} against bar {bar(ref):.3g}")
    assert got.shape == ref.shape and err <= bar(ref), (what, err, bar(ref))


# ---- the masked history mean alone ------------------------------------------------------------------------------------------
def hist_inputs(case, seed=0):
    """(E [V, D], hist int64 [B, L], mask int64 [B, L]) on the CPU"""
    gen = torch.Generator().manual_seed(seed)
    if case == "L=1":
        V, D, B, L = 9, 8, 5, 1
    elif case == "D=6":
        V, D, B, L = 11, 6, 7, 5  # (no dwordx4 path)
    else:
        V, D, B, L = 41, 16, 67, 7
    E = torch.randn(V, D, generator=gen)
    hist = torch.randint(1, V, (B, L), generator=gen)
    mask = (torch.rand(B, L, generator=gen) < 0.7).long()
    if case == "L=1":
        hist[0, 0], mask[0, 0] = 0, 1
        mask[1, 0] = 0
    else:
        hist[:, 0], mask[:, 0] = 5, 1     # a hot id present in every bag
        mask[2] = 0                       # a fully masked row
        hist[3, 1], mask[3, 1] = 0, 1     # an unmasked id 0
        hist[4, -2:], mask[4, -2:] = 0, 0  # a padded tail
    return E, hist, mask


def hist_reference(E, hist, mask, G):
    E64 = E.double().clone().requires_grad_(True)
    e = torch.nn.functional.embedding(hist, E64, padding_idx=0)
    out = torch.mean(e * mask.unsqueeze(-1).double(), dim=1)
    (out * G.double()).sum().backward()
    return out.detach(), E64.grad


@pytest.mark.parametrize("case", ["L=1", "D=6", "mixed"])
def test_hist_mean_against_float64_and_bit_identical(case):
    require_gpu()
    from rec_pangu_amd import functional as Fh
    E, hist, mask = hist_inputs(case)
    G = torch.randn(hist.shape[0], E.shape[1], generator=torch.Generator().manual_seed(1))
    want_out, want_dE = hist_reference(E, hist, mask, G)
    if case == "mixed":
        assert bool(((hist == 0) & (mask == 1)).any()) and bool((mask.sum(1) == 0).any()) and bool((hist == 5).any(1).all())
    runs = []
    for _ in range(2):
        Ed = E.cuda().requires_grad_(True)
        out = Fh.hist_mean(Ed, hist.cuda(), mask.cuda())
        (out * G.cuda()).sum().backward()
        runs.append((out.detach().cpu(), Ed.grad.cpu()))
    within(runs[0][0], want_out, f"{case}: out")
    within(runs[0][1], want_dE, f"{case}: dE")
    assert float(runs[0][1][0].abs().max()) == 0.0  # no gradient to row 0, masked or not
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_hist_id_outside_the_table_raises_index_error():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    E, hist, mask = hist_inputs("D=6")
    hist[1, 1] = E.shape[0]
    with pytest.raises(IndexError):
        Fh.hist_mean(E.cuda(), hist.cuda(), mask.cuda())


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_yotubednn_on_the_device_matches_the_reference():
    require_gpu()
    from rec_pangu_amd import hip
    g = load_golden("model_yotubednn.npz")
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    check_against_golden(g, *run_case(g, device="cuda:0"))
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0


def test_yotubednn_with_the_fused_adam_matches_the_reference():
    require_gpu()
    from rec_pangu_amd.optim import FusedAdam, make_adam
    g = load_golden("model_yotubednn.npz")
    made = []

    def make(model):
        made.append(make_adam(model, 1e-2))
        return made[-1]

    check_against_golden(g, *run_case(g, device="cuda:0", make_opt=make))
    assert isinstance(made[0], FusedAdam)  # a model without an EmbeddingLayer: item_emb.weight is a dense parameter


def _mid_batch(B, V, L, seed=0):
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(1, V, (B, L), generator=gen)
    lens = torch.randint(0, L + 1, (B,), generator=gen)
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    hist = hist * mask
    hist[0, 0], mask[0, 0] = 0, 1
    return {"hist_item_list": hist, "hist_mask_list": mask, "target_item": torch.randint(0, V, (B, 1), generator=gen)}


def _mid_model(V, D, L, seed=3):
    from rec_pangu_amd.models.sequence import YotubeDNN
    torch.manual_seed(seed)
    return YotubeDNN({"item_id": {"vocab_size": V}},
                     {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []})


def test_yotubednn_device_against_its_cpu_path():
    require_gpu()
    B, V, D, L = 300, 5000, 64, 20
    batch = _mid_batch(B, V, L)
    cpu = _mid_model(V, D, L)
    dev = _mid_model(V, D, L).to("cuda:0")
    assert torch.equal(cpu.item_emb.weight.detach(), dev.item_emb.weight.detach().cpu())
    rc = cpu({k: v.clone() for k, v in batch.items()})
    rc["loss"].backward()
    rd = dev({k: v.to("cuda:0") for k, v in batch.items()})
    rd["loss"].backward()
    within(rd["user_emb"], rc["user_emb"].detach(), "user_emb")
    within(rd["loss"].reshape(1), rc["loss"].detach().reshape(1), "loss")
    within(dev.item_emb.weight.grad, cpu.item_emb.weight.grad, "item_emb.weight.grad")


def test_two_fused_adam_steps_against_torch_adam_on_the_cpu():
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    B, V, D, L = 64, 500, 16, 5
    batch = _mid_batch(B, V, L)
    cpu, dev = _mid_model(V, D, L), _mid_model(V, D, L).to("cuda:0")
    opt_c = torch.optim.Adam(cpu.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    opt_d = make_adam(dev, 1e-2)
    for _ in range(2):
        cpu({k: v.clone() for k, v in batch.items()})["loss"].backward()
        opt_c.step()
        cpu.zero_grad()
        dev({k: v.to("cuda:0") for k, v in batch.items()})["loss"].backward()
        opt_d.step()
        dev.zero_grad()
    torch.testing.assert_close(dev.item_emb.weight.detach().cpu(), cpu.item_emb.weight.detach(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("interests", [0, 3])
def test_get_recall_predict_on_the_device_equals_the_cpu_result(interests):
    require_gpu()
    from rec_pangu_amd.utils.evaluate import get_recall_predict
    n_users, n_items, dim, topN = 23, 301, 8, 20
    items, users, s = gapped_recall_data(n_users, n_items, dim, topN, interests)
    on_cpu = get_recall_predict(StubRecallModel(items, users), recall_loader(n_users, 7), torch.device("cpu"), topN=topN)
    on_dev = get_recall_predict(StubRecallModel(items, users).to("cuda:0"), recall_loader(n_users, 7), torch.device("cuda:0"),
                                topN=topN)
    assert on_cpu == expected_preds(s, n_users, topN, interests)
    assert set(on_dev) == set(on_cpu) and all(on_dev[u] == on_cpu[u] for u in on_cpu)


def test_sequence_trainer_epoch_on_the_device(tmp_path):
    require_gpu()
    import math
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.sequence import YotubeDNN
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, test = _tiny_loaders()
    torch.manual_seed(0)
    model = YotubeDNN(enc, dict(cfg, device="cuda:0"))
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    trainer.fit(model, train, valid, epoch=1, lr=1e-2, device=torch.device("cuda:0"), topk_list=[5, 10])
    assert hip.torch_path_count() == t0 and hip.launch_count() > n0
    assert model.item_emb.weight.is_cuda and len(trainer.log_df) == 1
    row = trainer.log_df.iloc[0]
    assert all(math.isfinite(float(row[k])) and 0.0 <= float(row[k]) <= 1.0 for k in ("recall@10", "ndcg@10", "hitrate@10"))
    metric = trainer.evaluate_model(model, test, torch.device("cuda:0"), topk_list=[5])
    assert all(math.isfinite(v) for k, v in metric.items() if k != "phase")
