"""MaskNet on the CPU (plumbing, no GPU): state_dict contract, init RNG stream and forward / backward / Adam numerics against
the golden vectors produced by running the reference (tests/golden/make_golden_masknet.py), the constructor signature, the
trainer registry, and the argument validation of the LayerNorm entry points."""
import inspect

import pytest
import torch

from conftest import load_golden, small_enc_dict

torch.set_num_threads(1)

CASES = {
    "masknet_par3": dict(embedding_dim=8, block_num=3, use_parallel=True, hidden_units=[16, 8]),
    "masknet_ser2": dict(embedding_dim=8, block_num=2, use_parallel=False, hidden_units=[16, 8]),
}


def build(name, seed=1234):
    from rec_pangu_amd.models.ranking import MaskNet
    torch.manual_seed(seed)
    return MaskNet(enc_dict=small_enc_dict(), **CASES[name])


@pytest.mark.parametrize("name", list(CASES))
def test_init_stream_and_state_dict_contract(name):
    g = load_golden(f"model_{name}.npz")
    sd = build(name).state_dict()
    assert list(sd.keys()) == list(g["init"].keys())
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape, k
        assert torch.equal(sd[k], v), f"{name}: init of {k} differs from the reference's"
    per_block = ["_input_layer_norm.weight", "_input_layer_norm.bias", "_mask_layer.0.weight", "_mask_layer.0.bias",
                 "_mask_layer.2.weight", "_mask_layer.2.bias", "_hidden_layer.weight", "_hidden_layer.bias",
                 "_layer_norm.weight", "_layer_norm.bias"]
    block_keys = [k for k in sd if k.startswith("mask_block_list.")]
    assert block_keys == [f"mask_block_list.{b}.{p}" for b in range(CASES[name]["block_num"]) for p in per_block]
    assert sd["mask_block_list.0._mask_layer.0.weight"].shape == (12, 43)  # d = 5 * 8 + 3, agg = int(43 * 0.3)
    assert [k for k in sd if k.startswith("mlp.")] == [f"mlp.net.{i}.{p}" for i in (0, 3, 6) for p in ("weight", "bias")]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_adam_vs_reference(name):
    g = load_golden(f"model_{name}.npz")
    model = build(name)
    model.eval()  # (the MLP behind the blocks has Dropout(0.1); the fixtures are eval mode)
    out = model({k: v.clone() for k, v in g["batch"].items()})
    for k, v in g["out"].items():
        torch.testing.assert_close(out[k].detach(), v, rtol=1e-5, atol=1e-6, msg=lambda m: f"{name}:{k}: {m}")
    model.zero_grad()
    out["loss"].backward()
    params = dict(model.named_parameters())
    assert set(g["grad"]) == set(params)
    for k, v in g["grad"].items():
        torch.testing.assert_close(params[k].grad, v, rtol=1e-4, atol=1e-6, msg=lambda m: f"{name}:grad {k}: {m}")
    model = build(name)
    model.eval()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    for _ in range(2):
        r = model({k: v.clone() for k, v in g["batch"].items()})
        r["loss"].backward()
        opt.step()
        model.zero_grad()
    sd = model.state_dict()
    for k, v in g["adam2"].items():
        torch.testing.assert_close(sd[k], v, rtol=1e-4, atol=1e-6, msg=lambda m: f"{name}:adam2 {k}: {m}")
    with torch.no_grad():
        r = model({k: v.clone() for k, v in g["batch"].items()}, is_training=False)
    assert "loss" not in r
    for k, v in g["adam2_out"].items():
        torch.testing.assert_close(r[k], v, rtol=1e-5, atol=1e-6)


def test_constructor_signature_and_registry():
    """the signature as inspect.signature gives it for the reference's class (masknet.py:14-21)"""
    from rec_pangu_amd.models.ranking import MaskNet
    from rec_pangu_amd.benchmark_trainer import MODEL_REGISTRY
    from rec_pangu_amd.models.layers import MaskBlock
    sig = {k: v.default for k, v in inspect.signature(MaskNet.__init__).parameters.items() if k != "self"}
    assert sig == dict(embedding_dim=32, block_num=3, use_parallel=True, reduction_factor=0.3, hidden_units=[64, 64, 64],
                       loss_fun='torch.nn.BCELoss()', enc_dict=None)
    assert list(sig) == ["embedding_dim", "block_num", "use_parallel", "reduction_factor", "hidden_units", "loss_fun", "enc_dict"]
    assert MODEL_REGISTRY["MaskNet"] is MaskNet
    assert list(inspect.signature(MaskBlock.__init__).parameters)[1:] == ["input_dim", "mask_input_dim", "output_size",
                                                                         "reduction_factor"]


def test_mask_block_layer_on_cpu_with_unequal_widths():
    """the layer alone: input, mask input and output of different widths, against the formula written out"""
    from rec_pangu_amd.models.layers import MaskBlock
    torch.manual_seed(3)
    blk = MaskBlock(10, 7, 5, 0.5)
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn_like(p))
    net, x = torch.randn(6, 10), torch.randn(6, 7)
    F = torch.nn.functional
    mask = F.linear(F.relu(F.linear(x, blk._mask_layer[0].weight, blk._mask_layer[0].bias)), blk._mask_layer[2].weight,
                    blk._mask_layer[2].bias)
    n = F.layer_norm(net, (10,), blk._input_layer_norm.weight, blk._input_layer_norm.bias, 1e-5)
    ref = F.layer_norm(F.linear(n * mask, blk._hidden_layer.weight, blk._hidden_layer.bias), (5,), blk._layer_norm.weight,
                       blk._layer_norm.bias, 1e-5)
    assert blk._mask_layer[0].weight.shape == (3, 7)
    torch.testing.assert_close(blk(net, x), ref, rtol=1e-6, atol=1e-6)


def test_layernorm_argument_validation_needs_no_gpu():
    import ctypes
    from rec_pangu_amd import hip
    lib = hip.lib()
    assert lib.rp_version() == hip.ABI_VERSION == 108
    rc = lib.rp_layernorm_fwd(None, 0, None, None, 1e-5, None, 0, None, 0, 1, 1.0, 0, None, 0, 1, 1, None)
    assert rc == -1 and b"null" in lib.rp_last_error()
    rc = lib.rp_layernorm_bwd(None, 0, 1.0, None, 0, None, None, None, None, 0, None, 0, 1, 0, None, 0, None, None, 1, 1,
                              None, 0, None)
    assert rc == -1 and b"null" in lib.rp_last_error()
    n1, n2 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rp_layernorm_bwd_workspace_bytes(1677, ctypes.byref(n1)) == 0 and n1.value > 0
    assert lib.rp_layernorm_bwd_workspace_bytes(0, ctypes.byref(n2)) == -1
    # (the workspace takes no M: it cannot grow with the batch)
