"""NextItNet on the GPU: against the golden vectors of the reference (the CPU test's bars, tests/test_nextitnet_host.py; the
batch with a row without history included), against its own CPU path at (B, V, D, L) = (300, 5000, 64, 20) in the default and
the one-masked configuration (the project's 1e-4 max(1e-2, max |ref|) per tensor), the final block in last mode against the
same block forced to full mode, the fused Adam against torch.optim.Adam on the CPU path, feat_drop in train mode, and the
launch / torch-path counts of the default configuration."""
import math

import pytest
import torch

from conftest import load_golden, require_gpu
from test_nextitnet_host import MODELS, check_against_golden, run_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def within(got, ref, what):
    err = float((got.detach().cpu().double() - ref.double()).abs().max())
    print(f"{what}: max err {err:.3g} against bar {bar(ref):.3g}")
    assert got.shape == ref.shape and err <= bar(ref), (what, err, bar(ref))


@pytest.mark.parametrize("case", list(MODELS))
def test_model_on_the_device_matches_the_reference(case):
    require_gpu()
    from rec_pangu_amd import hip
    g = load_golden(f"model_{case}.npz")
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    check_against_golden(g, *run_case(case, g, device=DEV))
    assert hip.launch_count() > n0 and hip.torch_path_count() == t0


def test_exact_zero_weight_gradients_stay_exact_on_the_device():
    """at L = 6 the default configuration's dilation-8 conv reads padding through every tap but the last: the device gives
    exact zeros there, as the reference does, so Adam leaves those entries where they were"""
    require_gpu()
    g = load_golden("model_nextitnet_default.npz")
    _, grads, adam2, _, _, _ = run_case("nextitnet_default", g, device=DEV)
    w8 = "nextit_layer.res_blocks.1.conv2.conv.weight"
    assert float(grads[w8][:, :, :2].abs().max()) == 0.0 and torch.equal(adam2[w8][:, :, :2], g["init"][w8][:, :, :2])
    assert "fc.weight" not in grads and torch.equal(adam2["fc.weight"], g["init"]["fc.weight"])


def _mid_batch(B, V, L, seed=0):
    """right-padded histories of 0 .. L items; row 0 has length 1, row 1 length L, row 4 none"""
    gen = torch.Generator().manual_seed(seed)
    hist = torch.randint(1, V, (B, L), generator=gen)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0], lens[1], lens[2], lens[3], lens[4] = 1, L, 3, 2, 0
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    return {"hist_item_list": hist * mask, "hist_mask_list": mask, "target_item": torch.randint(0, V, (B, 1), generator=gen)}


def _mid_model(V, D, L, seed=3, **cfg):
    from rec_pangu_amd.models.sequence import NextItNet
    torch.manual_seed(seed)
    return NextItNet({"item_id": {"vocab_size": V}}, dict(
        {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}, **cfg))


def _grads(model):
    return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("one_masked", [False, True])
def test_device_against_its_cpu_path(one_masked):
    """the kernels, not a fallback, produce the numbers: the library's launch count rises, the torch-path count does not"""
    require_gpu()
    from rec_pangu_amd import hip
    B, V, D, L = 300, 5000, 64, 20
    batch = _mid_batch(B, V, L)
    cpu, dev = _mid_model(V, D, L, one_masked=one_masked), _mid_model(V, D, L, one_masked=one_masked).to(DEV)
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
    assert set(gc) == set(gd) == set(dict(cpu.named_parameters())) - {"fc.weight"}
    for k, v in gc.items():
        within(gd[k], v, f"grad {k}")
    # the forward + backward of the encoder alone: per block 2 + 7 (two-masked) or 2 + 9 (one-masked) launches
    layer = dev.nextit_layer
    x = torch.randn(B, L, D, device=DEV, requires_grad=True)
    lens = batch["hist_mask_list"].sum(1).to(DEV)
    n0 = hip.launch_count()
    layer(x, lens).sum().backward()
    torch.cuda.synchronize()
    assert hip.launch_count() - n0 == len(layer.res_blocks) * (11 if one_masked else 9) and hip.torch_path_count() == t0


@pytest.mark.parametrize("one_masked", [False, True])
def test_last_mode_against_the_final_block_forced_to_full_mode(one_masked):
    require_gpu()
    from rec_pangu_amd import hip
    B, V, D, L = 70, 300, 32, 33
    batch = {k: v.to(DEV) for k, v in _mid_batch(B, V, L).items()}
    dev = _mid_model(V, D, L, one_masked=one_masked).to(DEV)
    outs = {}
    for how in ("last", "full"):
        dev.nextit_layer.last_mode = how == "last"
        dev.zero_grad()
        t0 = hip.torch_path_count()
        res = dev(batch)
        res["loss"].backward()
        torch.cuda.synchronize()
        assert hip.torch_path_count() == t0
        outs[how] = dict(_grads(dev), user_emb=res["user_emb"].detach().cpu())
    assert set(outs["last"]) == set(outs["full"])
    for k, ref in outs["full"].items():
        within(outs["last"][k], ref, f"last mode: {k}")


def test_two_fused_adam_steps_against_torch_adam_on_the_cpu():
    """Bound per element, derived as in tests/test_hip_gru_models.py: atol 1e-6 + rtol 1e-4 (equal gradients)
    plus what Adam makes of a gradient that differs within the project's bar d = 1e-4 max(1e-2, max |g|) of its tensor: step 1
    moves by lr g / (|g| + eps), insensitive to g's size; step 2 by lr f(g2 / g1) with |r f'(r)| < 1, so relative errors e1, e2
    of the two gradients shift it by at most lr (e1 + e2), e_i <= d_i / |g_i| — capped at 2 lr, the most two steps can differ."""
    require_gpu()
    from rec_pangu_amd.optim import make_adam
    B, V, D, L, lr = 64, 500, 16, 7, 1e-2
    batch = _mid_batch(B, V, L)
    cpu, dev = _mid_model(V, D, L), _mid_model(V, D, L).to(DEV)
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


def test_feat_drop_in_train_mode_is_reproducible_and_on_the_kernels():
    require_gpu()
    from rec_pangu_amd import hip
    batch = {k: v.to(DEV) for k, v in _mid_batch(64, 500, 20).items()}
    dev = _mid_model(500, 32, 20, feat_drop=0.1).to(DEV).train()
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
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))  # equal generator state: equal bits
    assert not torch.equal(runs[0][0], runs[2][0])
    dev.eval()
    with torch.no_grad():
        a = dev(batch, is_training=False)["user_emb"]
        b = dev(batch, is_training=False)["user_emb"]
    assert torch.equal(a, b) and not torch.equal(a, runs[0][0])


def test_the_default_configuration_uses_no_torch_path():
    require_gpu()
    from rec_pangu_amd import hip
    batch = {k: v.to(DEV) for k, v in _mid_batch(32, 200, 50).items()}
    dev = _mid_model(200, 64, 50).to(DEV)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    res = dev(batch)
    res["loss"].backward()
    torch.cuda.synchronize()
    assert hip.torch_path_count() == t0 and hip.launch_count() - n0 >= 2 * 9
    assert float(res["user_emb"][4].abs().max()) > 0  # the row without history: a function of the biases
