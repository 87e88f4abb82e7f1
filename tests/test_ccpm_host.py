"""CCPM on the CPU (plumbing, no GPU): state_dict contract, init RNG stream and forward / backward / Adam numerics against
the golden vectors produced by running the reference (tests/golden/make_golden_ccpm.py), the constructor signature, the
trainer registry, KMaxPooling against hand-written expectations, the k schedule, the float64 restatement the GPU kernel tests
use against the model's own torch formulation, and the argument validation of the conv-stack entry points."""
import ctypes
import inspect

import pytest
import torch

from conftest import load_golden, small_enc_dict

torch.set_num_threads(1)

CASES = {
    "ccpm_default": dict(embedding_dim=8),
    "ccpm_c3h2": dict(embedding_dim=8, channels=[3], kernel_heights=[2]),
}
# the first model seed from 1234 upward whose every column margin is >= 1e-5 at the three recorded states, as
# tests/golden/make_golden_ccpm.py printed it
SEEDS = {"ccpm_default": 1235, "ccpm_c3h2": 1235}


def build(name):
    from rec_pangu_amd.models.ranking import CCPM
    torch.manual_seed(SEEDS[name])
    return CCPM(enc_dict=small_enc_dict(), **CASES[name])


@pytest.mark.parametrize("name", list(CASES))
def test_init_stream_and_state_dict_contract(name):
    g = load_golden(f"model_{name}.npz")
    model = build(name)
    sd = model.state_dict()
    assert list(sd.keys()) == list(g["init"].keys())
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape, k
        assert torch.equal(sd[k], v), f"{name}: init of {k} differs from the reference's"
    channels = CASES[name].get("channels", [4, 4, 2])
    heights = CASES[name].get("kernel_heights", [6, 5, 3])
    tail = [k for k in sd if not k.startswith("embedding_layer.")]
    assert tail == ([f"conv_layer.conv_layer.{4 * i + 1}.{p}" for i in range(len(channels)) for p in ("weight", "bias")]
                    + ["fc.weight", "fc.bias"])
    cin = 1
    for i, (co, kh) in enumerate(zip(channels, heights)):
        assert sd[f"conv_layer.conv_layer.{4 * i + 1}.weight"].shape == (co, cin, kh, 1)
        assert sd[f"conv_layer.conv_layer.{4 * i + 1}.bias"].shape == (co,)
        cin = co
    assert sd["fc.weight"].shape == (1, 3 * 8 * channels[-1])
    kinds = [type(m).__name__ for m in model.conv_layer.conv_layer]
    assert kinds == ["ZeroPad2d", "Conv2d", "KMaxPooling", "Tanh"] * len(channels)
    assert model.dnn_hidden_units == [64, 64, 64]
    assert model.conv_layer.ks == ([4, 3, 3] if len(channels) == 3 else [3])


@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_adam_vs_reference(name):
    g = load_golden(f"model_{name}.npz")
    model = build(name)
    model.eval()
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
    """the signatures as inspect.signature gives them for the reference's classes (ccpm.py:15-21, :82; sequence.py:69)"""
    from rec_pangu_amd.models.ranking import CCPM
    from rec_pangu_amd.models.ranking.ccpm import CCPM_ConvLayer
    from rec_pangu_amd.benchmark_trainer import MODEL_REGISTRY
    from rec_pangu_amd.models.layers import KMaxPooling
    sig = {k: v.default for k, v in inspect.signature(CCPM.__init__).parameters.items() if k != "self"}
    assert sig == dict(embedding_dim=32, hidden_units=[64, 64, 64], channels=[4, 4, 2], kernel_heights=[6, 5, 3],
                       loss_fun='torch.nn.BCELoss()', enc_dict=None)
    assert list(sig) == ["embedding_dim", "hidden_units", "channels", "kernel_heights", "loss_fun", "enc_dict"]
    assert MODEL_REGISTRY["CCPM"] is CCPM
    sig = {k: v.default for k, v in inspect.signature(CCPM_ConvLayer.__init__).parameters.items() if k != "self"}
    assert sig == dict(num_fields=inspect.Parameter.empty, channels=[3], kernel_heights=[3], activation="Tanh")
    assert list(inspect.signature(KMaxPooling.__init__).parameters)[1:] == ["k", "dim"]
    with pytest.raises(ValueError, match="same length"):
        CCPM_ConvLayer(5, channels=[3, 3], kernel_heights=[2])
    assert len(CCPM_ConvLayer(5, channels=[3, 3], kernel_heights=2).convs()) == 2  # a scalar height is repeated


def test_kmax_pooling_against_hand_written_expectations():
    from rec_pangu_amd.models.layers import KMaxPooling
    X = torch.tensor([[5., 1., 4., 2., 3.], [-1., -5., -2., -4., -3.]]).t().reshape(1, 1, 5, 2)  # two columns along dim 2
    out = KMaxPooling(3, dim=2)(X)
    assert out.shape == (1, 1, 3, 2)
    assert out[0, 0, :, 0].tolist() == [5., 4., 3.]      # the three largest, in their original order
    assert out[0, 0, :, 1].tolist() == [-1., -2., -3.]
    assert torch.equal(KMaxPooling(5, dim=2)(X), X)      # k = the length: the identity
    assert KMaxPooling(1, dim=2)(X)[0, 0, 0].tolist() == [5., -1.]
    seq = torch.tensor([[[1., 9.], [7., 2.], [3., 8.]]])  # [B, L, H] along dim 1, as the reference's docstring has it
    assert KMaxPooling(2, dim=1)(seq).tolist() == [[[7., 9.], [3., 8.]]]
    Xg = X.clone().requires_grad_(True)
    KMaxPooling(3, dim=2)(Xg).sum().backward()
    assert Xg.grad[0, 0, :, 0].tolist() == [1., 0., 1., 0., 1.]


@pytest.mark.parametrize("F,ks", [(3, [3, 3, 3]), (5, [4, 3, 3]), (26, [23, 8, 3]), (39, [34, 13, 3])])
def test_k_schedule(F, ks):
    from rec_pangu_amd.models.ranking.ccpm import CCPM_ConvLayer
    layer = CCPM_ConvLayer(F, channels=[4, 4, 2], kernel_heights=[6, 5, 3])
    formula = [max(3, int((1 - pow(float(i) / 3, 3 - i)) * F)) if i < 3 else 3 for i in (1, 2, 3)]
    assert layer.ks == formula == ks
    assert [m.k for m in layer.conv_layer if hasattr(m, "k")] == ks
    assert all(isinstance(k, int) for k in layer.ks)


@pytest.mark.parametrize("case", [(26, 32, (4, 4, 2), (6, 5, 3), 16), (7, 20, (2, 3), (3, 2), 33), (3, 16, (2,), (1,), 9)],
                         ids=["criteo", "c23", "identity"])
def test_the_float64_restatement_of_the_gpu_tests_against_the_torch_formulation(case):
    """tests/test_hip_ccpm_conv.py's stack64 (explicit padding, rank-count selection, ties to the lower index) and the
    module's topk -> sort -> gather formulation agree in float64 wherever no two values of a line are equal"""
    from rec_pangu_amd.models.ranking.ccpm import CCPM_ConvLayer
    from test_hip_ccpm_conv import draw, k_schedule, reference
    F, D, channels, heights, B = case
    x, Ws, bs, cot = draw(F, D, channels, heights, B, seed=5)
    layer = CCPM_ConvLayer(F, channels=list(channels), kernel_heights=list(heights)).double()
    assert layer.ks == k_schedule(F, len(channels))
    with torch.no_grad():
        for conv, W, b in zip(layer.convs(), Ws, bs):
            conv.weight.copy_(W)
            conv.bias.copy_(b)
    ref = reference(x, Ws, bs, cot, F, D, layer.ks, use_margin=False)
    xd = x.double().view(B, 1, F, D).requires_grad_(True)
    out = layer(xd).flatten(start_dim=1)
    torch.testing.assert_close(out.detach(), ref["out"], rtol=1e-12, atol=1e-12)
    out.backward(cot.double())
    torch.testing.assert_close(xd.grad.reshape(B, F * D), ref["dx"], rtol=1e-10, atol=1e-12)
    for conv, dW, db in zip(layer.convs(), ref["dW"], ref["db"]):
        torch.testing.assert_close(conv.weight.grad, dW, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(conv.bias.grad, db, rtol=1e-10, atol=1e-12)


def test_near_tie_cap_of_the_gpu_kernel_cases():
    """the float64 reference alone keeps every case of the GPU kernel tests under their 2 % cap of excluded columns"""
    from test_hip_ccpm_conv import BIG, CASES as KCASES, _case
    for case in KCASES + [BIG]:
        ok = _case(*case)["ok"]
        assert int((~ok).sum()) <= 0.02 * ok.numel(), case


def test_ccpm_argument_validation_needs_no_gpu():
    from rec_pangu_amd import hip
    lib = hip.lib()
    assert lib.rp_version() == hip.ABI_VERSION == 108  # (no existing prototype changed)
    for name in ("rp_ccpm_fits", "rp_ccpm_fwd", "rp_ccpm_bwd_workspace_bytes", "rp_ccpm_bwd"):
        assert name in hip.EXPORTED_SYMBOLS
    # the range: the GPU tests' grid is inside, L_out < k and everything beyond the limits outside
    assert hip.ccpm_fits(26, 32, [4, 4, 2], [6, 5, 3], [23, 8, 3]) and hip.ccpm_fits(40, 64, [4, 4, 2], [6, 5, 3], [35, 13, 3])
    assert hip.ccpm_fits(5, 8, [4, 4, 2], [6, 5, 3], [4, 3, 3]) and hip.ccpm_fits(3, 4, [3], [2], [3])
    assert hip.ccpm_fits(3, 16, [2], [1], [3]) and hip.ccpm_fits(7, 20, [2, 3], [3, 2], [3, 3])
    assert not hip.ccpm_fits(3, 4, [3], [2], [5])            # L_out = 4 < k = 5: the reference's topk raises
    assert not hip.ccpm_fits(26, 32, [4, 4, 2], [6, 5, 3], [23, 28, 3])  # the same at a later layer (L_out = 27)
    assert not hip.ccpm_fits(26, 32, [5], [2], [3]) and not hip.ccpm_fits(26, 32, [4], [9], [3])
    assert not hip.ccpm_fits(64, 32, [4], [2], [3]) and not hip.ccpm_fits(26, 32, [2] * 4, [2] * 4, [3] * 4)
    assert not hip.ccpm_fits(26, 0, [4], [2], [3]) and not hip.ccpm_fits(26, 32, [], [], [])
    # the wrappers' checks come before anything touches a device
    F, D, B = 5, 8, 4
    x = torch.zeros(B, F * D)
    W, b = torch.zeros(3, 1, 2, 1), torch.zeros(3)
    with pytest.raises(RuntimeError, match="float32"):
        hip.ccpm_fwd(x.double(), [W], [b], F, D, [3])
    with pytest.raises(RuntimeError, match="float32"):
        hip.ccpm_fwd(x, [W.half()], [b], F, D, [3])
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.ccpm_fwd(x, [torch.zeros(3, 1, 4, 1)[:, :, ::2]], [b], F, D, [3])
    with pytest.raises(RuntimeError, match="narrower"):
        hip.ccpm_fwd(x[:, :F * D - 1], [W], [b], F, D, [3])
    with pytest.raises(RuntimeError, match="narrower"):  # wide enough, but the rows overlap: row stride < F D
        hip.ccpm_fwd(torch.zeros(B * F * D).as_strided((B, F * D), (F * D - 1, 1)), [W], [b], F, D, [3])
    with pytest.raises(RuntimeError, match="topk would raise"):
        hip.ccpm_fwd(x, [W], [b], F, D, [7])
    with pytest.raises(RuntimeError, match="input channels"):
        hip.ccpm_bwd(torch.zeros(B, 3 * 3 * D), x, [torch.zeros(3, 2, 2, 1)], [b], F, D, [3])
    with pytest.raises(RuntimeError, match="HIP-device"):  # every host-side check passed: only now the device matters
        hip.ccpm_fwd(x, [W], [b], F, D, [3])
    # the C entry points: null pointers, a row stride smaller than the row, a stack outside the range (before any launch)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptrs = (ctypes.c_void_p * 1)(p.value)
    assert lib.rp_ccpm_fwd(None, 0, None, None, None, 0, 5, 8, 1, None, None, None, 1, None) == -1
    assert b"null" in lib.rp_last_error()
    assert lib.rp_ccpm_fwd(p, 39, ptrs, ptrs, p, 72, 5, 8, 1, ints(3), ints(2), ints(3), 1, None) == -1
    assert b"leading" in lib.rp_last_error()
    assert lib.rp_ccpm_fwd(p, 40, ptrs, ptrs, p, 71, 5, 8, 1, ints(3), ints(2), ints(3), 1, None) == -1
    assert lib.rp_ccpm_fwd(p, 40, ptrs, ptrs, p, 72, 5, 8, 1, ints(3), ints(2), ints(7), 1, None) == -3  # L_out = 6 < k = 7
    assert lib.rp_ccpm_bwd(p, 72, p, 40, ptrs, ptrs, p, 40, ptrs, ptrs, 5, 8, 1, ints(5), ints(2), ints(3), 1, p, 1 << 20,
                           None) == -3
    assert lib.rp_ccpm_bwd(p, 72, p, 40, ptrs, ptrs, p, 39, ptrs, ptrs, 5, 8, 1, ints(3), ints(2), ints(3), 1, p, 1 << 20,
                           None) == -1 and b"leading" in lib.rp_last_error()
    assert lib.rp_ccpm_bwd(p, 72, p, 40, ptrs, ptrs, p, 40, ptrs, ptrs, 5, 8, 1, ints(3), ints(2), ints(3), 1, p, 16,
                           None) == -1 and b"workspace" in lib.rp_last_error()
    # the workspace takes the stack and no batch size: it cannot grow with the batch
    assert len(lib.rp_ccpm_bwd_workspace_bytes.argtypes) == 4
    n = ctypes.c_size_t(0)
    assert lib.rp_ccpm_bwd_workspace_bytes(3, ints(4, 4, 2), ints(6, 5, 3), ctypes.byref(n)) == 0
    assert n.value == 512 * 138 * 4 + 256  # 138 parameters of the default stack, 512 partials
    assert lib.rp_ccpm_bwd_workspace_bytes(0, ints(4), ints(6), ctypes.byref(n)) == -1
