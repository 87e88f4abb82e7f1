"""CLRec and ContraRec on the GPU: against the golden vectors of the reference (the CPU test's bars and rules,
tests/test_contrast_host.py), against their own CPU path at (B, V, D, L) = (300, 5000, 64, 20) with replayed augmentations (the
project's 1e-4 max(1e-2, max |ref|) per tensor), the 3 B-row batched encoder pass against three separate passes, a batch with
an empty row, the fused Adam against torch.optim.Adam on the CPU path, and the vectorised augmenter on the device."""
import math

import pytest
import torch

from conftest import require_gpu
from test_contrast_host import CASES, Replay, check_against_golden, check_augmenter, golden, run_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY_BIAS = "k_linear.bias"


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def within(got, ref, what, scale=None):
    """scale: the tensor whose bar applies instead of ref's own (see key_scale)"""
    err = float((got.detach().cpu().double() - ref.double()).abs().max())
    lim = bar(ref if scale is None else scale)
    print(f"{what}: max err {err:.3g} against bar {lim:.3g}")
    assert got.shape == ref.shape and err <= lim, (what, err, lim)


def key_scale(grads, k):
    """tests/test_hip_sasrec.key_scale: a key bias's gradient is zero in exact arithmetic, so its own max |ref| is rounding
    noise; the key WEIGHT's gradient sums the same dK rows against inputs of order one and gives the scale"""
    return grads[k[:-len("bias")] + "weight"] if k.endswith(KEY_BIAS) else None


@pytest.mark.parametrize("case", list(CASES))
def test_model_on_the_device_matches_the_reference(case):
    require_gpu()
    from rec_pangu_amd import hip
    g = golden(case)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    check_against_golden(g, *run_case(case, g, device=DEV))
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0


def _mid_batch(B, V, L, seed=0, empty_row=False):
    """right-padded histories of 1 .. L items; row 0 has length 1, row 1 length L; targets repeat (V_t = 40 values)"""
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(1, V - 1, (B, L), generator=gen)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0], lens[1], lens[2], lens[3] = 1, L, 3, 2
    if empty_row:
        lens[4] = 0
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return {"hist_item_list": hist * mask, "hist_mask_list": mask, "target_item": torch.randint(0, 40, (B, 1), generator=gen)}


def _mid_model(case, V, D, L, seed=3):
    from rec_pangu_amd.models import sequence
    name, cfg = CASES[case]
    torch.manual_seed(seed)
    return getattr(sequence, name)({"item_id": {"vocab_size": V}}, dict(
        {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}, **cfg)).train()


def _augmentations(model, hist, n, seed=5):
    """n results of the model's own augmenter on the CPU, to be replayed on both sides"""
    if not hasattr(model, "data_augmenter"):
        return []
    torch.manual_seed(seed)
    return [model.data_augmenter.augment(hist) for _ in range(n)]


def _pair(case, B, V, D, L, n_aug, empty_row=False):
    batch = _mid_batch(B, V, L, empty_row=empty_row)
    cpu, dev = _mid_model(case, V, D, L), _mid_model(case, V, D, L).to(DEV)
    for (k, a), b in zip(cpu.state_dict().items(), dev.state_dict().values()):
        assert torch.equal(a, b.cpu()), k
    augs = _augmentations(cpu, batch["hist_item_list"], n_aug)
    if augs:
        cpu.data_augmenter.augment = Replay(augs, "cpu")
        dev.data_augmenter.augment = Replay(augs, DEV)
    return batch, cpu, dev


@pytest.mark.parametrize("case", list(CASES))
def test_device_against_its_cpu_path(case):
    """the kernels, not a fallback, produce the numbers: the library's launch count rises, the torch-path count does not"""
    require_gpu()
    from rec_pangu_amd import hip
    B, V, D, L = 300, 5000, 64, 20
    batch, cpu, dev = _pair(case, B, V, D, L, 2)
    rc = cpu({k: v.clone() for k, v in batch.items()})
    rc["loss"].backward()
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    rd = dev({k: v.to(DEV) for k, v in batch.items()})
    rd["loss"].backward()
    torch.cuda.synchronize()
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0
    within(rd["user_emb"], rc["user_emb"].detach(), f"{case}: user_emb")
    within(rd["loss"].reshape(1), rc["loss"].detach().reshape(1), f"{case}: loss")
    grads = dict(dev.named_parameters())
    ref = {n: q.grad for n, q in cpu.named_parameters()}
    for k, p in cpu.named_parameters():
        within(grads[k].grad, p.grad, f"{case}: grad {k}", key_scale(ref, k))


def test_the_batched_encoder_pass_is_three_separate_passes():
    require_gpu()
    B, V, D, L = 70, 300, 32, 20
    batch = _mid_batch(B, V, L)
    dev = _mid_model("contrarec_bert", V, D, L).to(DEV)
    hist = batch["hist_item_list"]
    lens = batch["hist_mask_list"].sum(1).to(DEV)
    seqs = [hist.to(DEV)] + [a.to(DEV) for a in _augmentations(dev, hist, 2)]
    g = torch.randn(3 * B, D, generator=torch.Generator().manual_seed(1)).to(DEV)
    outs = {}
    for how in ("batched", "separate"):
        dev.zero_grad()
        if how == "batched":
            out = dev.encode(torch.cat(seqs, dim=0), lens.repeat(3))
        else:
            out = torch.cat([dev.encode(s, lens) for s in seqs], dim=0)
        (out * g).sum().backward()
        torch.cuda.synchronize()
        outs[how] = {"out": out.detach().cpu(), **{k: p.grad.cpu().clone() for k, p in dev.named_parameters()}}
    for k, ref in outs["separate"].items():
        within(outs["batched"][k], ref, f"batched encoder pass: {k}", key_scale(outs["separate"], k))


@pytest.mark.parametrize("case", ["clrec", "contrarec_bert"])
def test_a_row_without_history_gives_a_zero_user_emb(case):
    require_gpu()
    B, V, D, L = 40, 200, 16, 6
    batch = _mid_batch(B, V, L, empty_row=True)
    assert int(batch["hist_mask_list"][4].sum()) == 0 and int(batch["hist_item_list"][4].abs().sum()) == 0
    dev = _mid_model(case, V, D, L).to(DEV)
    res = dev({k: v.to(DEV) for k, v in batch.items()})
    res["loss"].backward()
    torch.cuda.synchronize()
    assert float(res["user_emb"][4].detach().abs().max()) == 0.0 and float(res["user_emb"][3].detach().abs().max()) > 0
    assert math.isfinite(float(res["loss"].detach())) and all(torch.isfinite(p.grad).all() for p in dev.parameters())


@pytest.mark.parametrize("case", ["clrec", "contrarec_bert"])
def test_two_fused_adam_steps_against_torch_adam_on_the_cpu(case):
    """Bound per element, derived as in tests/test_hip_sasrec.py: atol 1e-6 + rtol 1e-4 (equal gradients) plus what Adam makes
    of a gradient that differs within the project's bar d = 1e-4 max(1e-2, max |g|) of its tensor: step 1 moves by
    lr g / (|g| + eps), insensitive to g's size; step 2 by lr f(g2 / g1) with |r f'(r)| < 1, so relative errors e1, e2 of the two
    gradients shift it by at most lr (e1 + e2), e_i <= d_i / |g_i| -- capped at 2 lr, the most two steps can differ.  (The key
    biases, whose exact gradient is zero, sit at that cap.)"""
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    B, V, D, L, lr = 64, 500, 16, 5, 1e-2
    batch, cpu, dev = _pair(case, B, V, D, L, 4)
    opt_c = torch.optim.Adam(cpu.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    opt_d = make_adam(dev, lr)
    slack = {k: torch.zeros_like(p) for k, p in cpu.named_parameters()}
    for _ in range(2):
        cpu({k: v.clone() for k, v in batch.items()})["loss"].backward()
        for k, p in cpu.named_parameters():
            slack[k] += lr * bar(p.grad) / p.grad.abs().clamp(min=1e-30)
        opt_c.step()
        cpu.zero_grad()
        dev({k: v.to(DEV) for k, v in batch.items()})["loss"].backward()
        opt_d.step()
        dev.zero_grad()
    for (k, a), b in zip(cpu.state_dict().items(), dev.state_dict().values()):
        tol = 1e-6 + 1e-4 * a.abs() + slack[k].clamp(max=2 * lr)
        over = ((b.detach().cpu() - a).abs() - tol).max()
        tight = int(((b.detach().cpu() - a).abs() <= 1e-6 + 1e-4 * a.abs()).sum())
        print(f"{k}: {tight} of {a.numel()} elements within rtol 1e-4 / atol 1e-6, worst excess over the bound {float(over):.3g}")
        assert float(over) <= 0, k


def test_the_augmenter_on_the_device():
    require_gpu()
    check_augmenter(DEV)
