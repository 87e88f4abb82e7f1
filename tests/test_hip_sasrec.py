"""SASRec on the GPU: against the golden vectors of the reference (the CPU test's bars, tests/test_sasrec_host.py), against its own
CPU path at (B, V, D, L) = (300, 5000, 64, 20) with 2 layers and 4 heads (the project's 1e-4 max(1e-2, max |ref|) per tensor),
encode_last against the full encoder's gathered row, a batch with an empty row, the fused Adam against torch.optim.Adam on the
CPU path, train mode with the default dropouts, and the launch / torch-path counts of the default configuration."""
import math

import pytest
import torch

from conftest import load_golden, require_gpu
from test_sasrec_host import CASES, check_against_golden, run_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def within(got, ref, what, scale=None):
    """scale: the tensor whose bar applies instead of ref's own (see key_scale)"""
    err = float((got.detach().cpu().double() - ref.double()).abs().max())
    lim = bar(ref if scale is None else scale)
    print(f"{what}: max err {err:.3g} against bar {lim:.3g}")
    assert got.shape == ref.shape and err <= lim, (what, err, lim)


def key_scale(grads, k):
    """The gradient of a key bias is the column sum of dK over all B L rows and is ZERO in exact arithmetic (every query's
    score gradients add up to zero over its keys, so sum_j dK_j = sum_i (sum_j ds_ij) q_i = 0): max |ref| of that tensor is
    rounding noise and says nothing about the size of what was summed.  The key WEIGHT's gradient sums the same dK rows against
    inputs of order one (LayerNorm outputs, item rows), so its bar is the scale the sum's rounding lives on."""
    return grads[k[:-len("bias")] + "weight"] if k.endswith("multi_head_attention.key.bias") else None


@pytest.mark.parametrize("case", list(CASES))
def test_model_on_the_device_matches_the_reference(case):
    require_gpu()
    from rec_pangu_amd import hip
    g = load_golden(f"model_{case}.npz")
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    check_against_golden(g, *run_case(case, g, device=DEV))
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0


def _mid_batch(B, V, L, seed=0, empty_row=False):
    """right-padded histories of 1 .. L items (the CPU path raises for an empty one); row 0 has length 1, row 1 length L"""
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(1, V, (B, L), generator=gen)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0], lens[1], lens[2], lens[3] = 1, L, 3, 2
    if empty_row:
        lens[4] = 0
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return {"hist_item_list": hist * mask, "hist_mask_list": mask, "target_item": torch.randint(0, V, (B, 1), generator=gen)}


def _mid_model(V, D, L, seed=3, **cfg):
    from rec_pangu_amd.models.sequence import SASRec
    torch.manual_seed(seed)
    return SASRec({"item_id": {"vocab_size": V}}, dict(
        {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}, **cfg))


NO_DROP = {"hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0}


@pytest.mark.parametrize("act", ["gelu", "swish", "tanh"])
def test_device_against_its_cpu_path(act):
    """the kernels, not a fallback, produce the numbers: the library's launch count rises, the torch-path count does not"""
    require_gpu()
    from rec_pangu_amd import hip
    B, V, D, L = 300, 5000, 64, 20
    batch = _mid_batch(B, V, L)
    cfg = dict(NO_DROP, n_layers=2, n_heads=4, hidden_act=act)
    cpu, dev = _mid_model(V, D, L, **cfg), _mid_model(V, D, L, **cfg).to(DEV)
    for (k, a), b in zip(cpu.state_dict().items(), dev.state_dict().values()):
        assert torch.equal(a, b.cpu()), k
    rc = cpu({k: v.clone() for k, v in batch.items()})
    rc["loss"].backward()
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    rd = dev({k: v.to(DEV) for k, v in batch.items()})
    rd["loss"].backward()
    torch.cuda.synchronize()
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0
    within(rd["user_emb"], rc["user_emb"].detach(), f"{act}: user_emb")
    within(rd["loss"].reshape(1), rc["loss"].detach().reshape(1), f"{act}: loss")
    grads = dict(dev.named_parameters())
    for k, p in cpu.named_parameters():
        within(grads[k].grad, p.grad, f"{act}: grad {k}", key_scale({n: q.grad for n, q in cpu.named_parameters()}, k))


def test_encode_last_against_the_full_encoders_gathered_row():
    """the final layer in last-row mode against every layer full, both on the device, values and gradients, within the kernel
    bar; with a [B, 1, L, L] additive mask the encoder composes the result from torch ops and says so"""
    require_gpu()
    import warnings
    from rec_pangu_amd import hip
    B, V, D, L = 70, 300, 32, 33
    batch = _mid_batch(B, V, L)
    dev = _mid_model(V, D, L, **dict(NO_DROP, n_layers=2, n_heads=2)).to(DEV)
    mask = batch["hist_mask_list"].to(DEV)
    last = mask.sum(-1) - 1
    gen = torch.Generator().manual_seed(1)
    x0 = torch.randn(B, L, D, generator=gen)
    g = torch.randn(B, D, generator=gen).to(DEV)
    outs = {}
    for how in ("last", "full", "additive"):
        x = x0.to(DEV).requires_grad_(True)
        dev.zero_grad()
        n0, t0 = hip.launch_count(), hip.torch_path_count()
        if how == "last":
            out = dev.self_attention.encode_last(x, mask)
        elif how == "full":
            out = dev.gather_indexes(dev.self_attention(x, mask, output_all_encoded_layers=False)[-1], last)
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out = dev.gather_indexes(dev.self_attention(x, dev.get_attention_mask(mask))[-1], last)
        (out * g).sum().backward()
        torch.cuda.synchronize()
        assert (hip.torch_path_count() - t0) == (2 if how == "additive" else 0) and hip.launch_count() > n0
        outs[how] = {"out": out.detach().cpu(), "dx": x.grad.cpu(),
                     **{k: p.grad.cpu().clone() for k, p in dev.self_attention.named_parameters()}}
    for k, ref in outs["full"].items():
        within(outs["last"][k], ref, f"encode_last: {k}", key_scale(outs["full"], k))
        within(outs["additive"][k], ref, f"additive mask: {k}", key_scale(outs["full"], k))


def test_a_row_without_history_gives_a_zero_user_emb():
    require_gpu()
    B, V, D, L = 40, 200, 16, 6
    batch = _mid_batch(B, V, L, empty_row=True)
    assert int(batch["hist_mask_list"][4].sum()) == 0 and int(batch["hist_item_list"][4].abs().sum()) == 0
    dev = _mid_model(V, D, L, **NO_DROP).to(DEV)
    res = dev({k: v.to(DEV) for k, v in batch.items()})
    res["loss"].backward()
    torch.cuda.synchronize()
    assert float(res["user_emb"][4].detach().abs().max()) == 0.0 and float(res["user_emb"][3].detach().abs().max()) > 0
    assert math.isfinite(float(res["loss"].detach())) and all(torch.isfinite(p.grad).all() for p in dev.parameters())


def test_two_fused_adam_steps_against_torch_adam_on_the_cpu():
    """Bound per element, derived as in tests/test_hip_gru_models.py: atol 1e-6 + rtol 1e-4 (equal gradients) plus what Adam
    makes of a gradient that differs within the project's bar d = 1e-4 max(1e-2, max |g|) of its tensor: step 1 moves by
    lr g / (|g| + eps), insensitive to g's size; step 2 by lr f(g2 / g1) with |r f'(r)| < 1, so relative errors e1, e2 of the two
    gradients shift it by at most lr (e1 + e2), e_i <= d_i / |g_i| — capped at 2 lr, the most two steps can differ.  (The key
    biases, whose exact gradient is zero, sit at that cap: see tests/test_sasrec_host.py.)"""
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    B, V, D, L, lr = 64, 500, 16, 5, 1e-2
    batch = _mid_batch(B, V, L)
    cpu, dev = _mid_model(V, D, L, **NO_DROP), _mid_model(V, D, L, **NO_DROP).to(DEV)
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


def test_train_mode_with_the_default_dropouts_is_reproducible_and_on_the_kernels():
    require_gpu()
    from rec_pangu_amd import hip
    batch = {k: v.to(DEV) for k, v in _mid_batch(64, 500, 20).items()}
    dev = _mid_model(500, 32, 20).to(DEV).train()
    assert dev.attn_dropout_prob == 0.1 and dev.hidden_dropout_prob == 0.1 and dev.n_heads == 4
    runs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        dev.zero_grad()
        n0, t0 = hip.launch_count(), hip.torch_path_count()
        res = dev({k: v.clone() for k, v in batch.items()})
        res["loss"].backward()
        torch.cuda.synchronize()
        assert hip.launch_count() > n0 and hip.torch_path_count() == t0 and math.isfinite(float(res["loss"]))
        runs.append([res["user_emb"].detach().clone(), res["loss"].detach().clone()] +
                    [p.grad.detach().clone() for p in dev.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))  # equal generator state: equal bits
    assert not torch.equal(runs[0][0], runs[2][0])
    dev.eval()
    with torch.no_grad():
        a = dev(batch, is_training=False)["user_emb"]
        b = dev(batch, is_training=False)["user_emb"]
    assert torch.equal(a, b) and not torch.equal(a, runs[0][0])
