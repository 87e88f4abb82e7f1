"""NextItNet and its residual blocks on the CPU (plumbing, no GPU): the model against the three golden files produced by running
the reference (tests/golden/make_golden_nextitnet.py), its state_dict / init stream (the unused `fc` included), the config
defaults, the import surface, the float64 restatement of a block on a VIRTUAL SEQUENCE the GPU tests compare against (checked
here against the reference-formula CPU path, in both modes), the rule that padding rows are zero at the input of every conv,
the conditioning of every shape the GPU file compares, one SequenceTrainer epoch, and the declaration / binding / argument
checks of the new C entry points.

Bars of the model comparisons are tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, the other tolerance 1e-6,
the tighter of the two readings per element (the generator chose its seeds against a tenth of that).  Kernel comparisons use
the project's per-tensor bar 1e-4 max(1e-2, max |ref|) against float64.

Conditioning: a LayerNorm over exactly TWO channels is a sign function of their difference, and torch's own fp32 run is far
from its float64 run there.  Those widths (two-masked C = 2; one-masked C = 4, 5, whose middle width is 2) are compared
nowhere: ILL runs for finiteness and bit-identity only.  For every shape of CASES the fp32 CPU run of torch's own
formulation must sit under a quarter of the bar here, so that a badly conditioned shape fails on the host, not on the device."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from test_sequence_host import _tiny_loaders, close

torch.set_num_threads(1)

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
MODELS = {
    "nextitnet_default": {},
    "nextitnet_d12_k2": {"dilations": [1, 2], "kernel_size": 2},
    "nextitnet_one_masked": {"one_masked": True, "dilations": [1, 2], "kernel_size": 3},
}
LR = 1e-2

# (one_masked, C, k, dilation, L, B): what tests/test_hip_causal_conv.py compares, in full mode and in last mode
CASES = [
    (0, 3, 3, 1, 7, 3), (0, 8, 2, 2, 7, 70), (0, 20, 5, 1, 33, 3), (0, 33, 3, 4, 33, 70), (0, 64, 3, 1, 128, 3),
    (0, 64, 3, 4, 64, 70), (0, 128, 3, 2, 64, 3), (0, 64, 1, 1, 7, 1), (0, 8, 3, 9, 7, 3), (0, 64, 3, 1, 1, 3),
    (0, 20, 2, 1, 2, 70), (0, 64, 5, 2, 33, 1),
    (1, 3, 3, 1, 7, 3), (1, 8, 3, 2, 7, 70), (1, 9, 5, 1, 33, 3), (1, 64, 2, 4, 64, 70), (1, 128, 3, 1, 64, 1),
    (1, 64, 3, 2, 128, 3), (1, 8, 1, 1, 2, 3), (1, 16, 3, 40, 33, 3), (1, 64, 3, 1, 1, 3),
]
ILL = [(0, 2, 3, 1, 7, 3), (1, 4, 3, 1, 7, 3), (1, 5, 3, 2, 7, 70)]  # a LayerNorm over two channels: finiteness and bits only


def bar(ref):
    """the project's per-tensor bar against float64: 1e-4 max(1e-2, max |ref|)"""
    return 1e-4 * max(1e-2, float(ref.abs().max()))


# ---- the float64 restatement the GPU tests compare against ---------------------------------------------------------------------
def rows_of(k, one_masked):
    """virtual rows of a last-mode launch: the positions the read row depends on"""
    return k if one_masked else 3 * (k - 1) + 1


def block_f64(x, lens, params, stride, R, dilations, last=False, pad_every_conv=True):
    """One residual block on a virtual sequence, in the dtype of x (float64 in the tests), differentiable.
    x [B, L, C]; lens [B]; params: the block's 12 slots (conv weight 0..2 [Cout, Cin, taps], conv bias 0..2, LayerNorm gamma
    0..2, beta 0..2; a two-masked block has None in the third of each).  Row r of R stands for position
    pos = anchor - (R - 1 - r) stride, anchor = L - 1 (last: lens - 1, or L - 1 for an empty row); a row at pos >= lens is
    loaded as zero, a row at pos < 0 is padding: zero at the input of every conv (pad_every_conv False zeroes it at the
    first conv only: the mistake the rule is there to prevent).  dilations: the internal dilation of each conv, in rows.
    -> [B, R, C]: stages + the loaded rows."""
    B, Ls, C = x.shape
    anchor = torch.where(lens > 0, lens - 1, torch.full_like(lens, Ls - 1)) if last else torch.full_like(lens, Ls - 1)
    pos = anchor[:, None] - (R - 1 - torch.arange(R))[None, :] * stride  # [B, R]
    loaded = ((pos >= 0) & (pos < lens[:, None])).to(x.dtype)[..., None]
    v0 = x[torch.arange(B)[:, None], pos.clamp(0, Ls - 1)] * loaded
    alive = (pos >= 0).to(x.dtype)[..., None]
    one_masked = params[2] is not None

    def conv(v, w, b, dil):
        taps = w.shape[2]
        out = b.view(1, 1, -1).expand(B, R, -1)
        for j in range(taps):
            shift = (taps - 1 - j) * dil
            if shift >= R:
                continue
            moved = torch.cat([v.new_zeros(B, shift, v.shape[2]), v[:, :R - shift]], dim=1)
            out = out + moved @ w[:, :, j].t()
        return out

    def ln(v, g, be, first):
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
        y = torch.relu((v - mean) / torch.sqrt(var + 1e-5) * g.view(1, 1, -1) + be.view(1, 1, -1))
        return y * alive if (pad_every_conv or first) else y

    w, b, g, be = params[0:3], params[3:6], params[6:9], params[9:12]
    if one_masked:
        y = conv(ln(v0, g[0], be[0], True), w[0], b[0], dilations[0])
        y = conv(ln(y, g[1], be[1], False), w[1], b[1], dilations[1])
        y = conv(ln(y, g[2], be[2], False), w[2], b[2], dilations[2])
    else:
        y = ln(conv(v0, w[0], b[0], dilations[0]), g[0], be[0], False)
        y = ln(conv(y, w[1], b[1], dilations[1]), g[1], be[1], False)
    return y + v0


def block_modes(block, Ls):
    """(stride, R, dilations) of the block in full mode and in last mode"""
    k, d = block.kernel_size, block.dilation
    if block.one_masked:
        return (1, Ls, (1, d, 1)), (d, rows_of(k, True), (1, 1, 1))
    return (1, Ls, (d, 2 * d)), (d, rows_of(k, False), (1, 2))


def make_block(one_masked, C, k, d, seed=0):
    """a block with every parameter away from its default (gamma around 1, beta around 0, both random)"""
    from rec_pangu_amd.models.layers import ResBlockOneMasked, ResBlockTwoMasked
    torch.manual_seed(seed)
    block = (ResBlockOneMasked if one_masked else ResBlockTwoMasked)(C, k, d)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in block.named_parameters():
            if name.endswith("gamma"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=gen))
            elif name.endswith("beta") or name.endswith("bias"):
                p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    return block


def make_lens(B, Ls, gen):
    """per-row lengths: L, 0, 1, then random in [0, L]; a batch of one gets a length in the middle"""
    if B == 1:
        return torch.tensor([max(1, Ls // 2)])
    lens = torch.randint(0, Ls + 1, (B,), generator=gen)
    lens[0] = Ls
    lens[1] = 0
    if B > 2:
        lens[2] = 1
    return lens


def case_inputs(case):
    one, C, k, d, Ls, B = case
    gen = torch.Generator().manual_seed(1000 * C + 10 * Ls + B + k)
    x = torch.randn(B, Ls, C, generator=gen)
    lens = make_lens(B, Ls, gen)
    g_full = torch.randn(B, Ls, C, generator=gen)
    g_last = torch.randn(B, C, generator=gen)
    return make_block(one, C, k, d, seed=C + k), x, lens, g_full, g_last


_F64 = {}


def f64_results(case):
    """float64 autograd of the restatement, once per case: {'full' | 'last': {'out', 'dx', 'p0' .. 'p11'}}.  Last mode is the
    read row of the FULL float64 result (and the gradients of that row)."""
    if case in _F64:
        return _F64[case]
    block, x, lens, g_full, g_last = case_inputs(case)
    (stride, R, dil), _ = block_modes(block, x.shape[1])
    res = {}
    for mode in ("full", "last"):
        ps = [None if p is None else p.detach().double().requires_grad_(True) for p in block.stage_params()]
        xd = x.double().requires_grad_(True)
        out = block_f64(xd, lens, ps, stride, R, dil)
        if mode == "last":
            out = out[torch.arange(len(lens)), lens - 1]
        (out * (g_full if mode == "full" else g_last).double()).sum().backward()
        res[mode] = {"out": out.detach(), "dx": xd.grad}
        res[mode].update({f"p{i}": p.grad for i, p in enumerate(ps) if p is not None})
    _F64[case] = res
    return res


def run_block(case, mode, device="cpu", block_fn=None):
    """forward + backward of the library's block node on `device` -> {'out', 'dx', 'p0' .. 'p11'} (shared with the GPU tests)"""
    from rec_pangu_amd import functional as Fh
    block, x, lens, g_full, g_last = case_inputs(case)
    block = block.to(device)
    xd = x.to(device).requires_grad_(True)
    out = (block_fn or Fh.causal_conv_block)(xd, lens.to(device), block, mode == "last")
    (out * (g_full if mode == "full" else g_last).to(device)).sum().backward()
    got = {"out": out.detach().cpu(), "dx": xd.grad.cpu()}
    got.update({f"p{i}": p.grad.cpu() for i, p in enumerate(block.stage_params()) if p is not None})
    return got


@pytest.mark.parametrize("case", CASES, ids=str)
def test_fp32_on_the_cpu_sits_under_a_quarter_of_the_bar(case):
    ref = f64_results(case)
    for mode in ("full", "last"):
        got = run_block(case, mode)
        assert set(got) == set(ref[mode])
        for key, want in ref[mode].items():
            err = float((got[key].double() - want).abs().max())
            assert got[key].shape == want.shape and err <= bar(want) / 4, (mode, key, err, bar(want))


@pytest.mark.parametrize("one_masked,C,k,d,Ls", [(0, 5, 3, 1, 9), (0, 4, 2, 3, 6), (0, 6, 5, 2, 7), (1, 6, 3, 2, 9), (1, 8, 2, 1, 5),
                                                 (1, 7, 5, 4, 6), (0, 3, 1, 1, 4)])
def test_the_restatement_is_the_reference_formulas_in_both_modes(one_masked, C, k, d, Ls):
    """against NextItNetLayer's CPU path (the reference's torch ops) in float64, to 1e-12: full mode at every position, last mode
    at the read position, lengths 0, 1, L and in between"""
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd.models.layers import NextItNetLayer
    torch.manual_seed(3)
    layer = NextItNetLayer(C, [d], bool(one_masked), k).double().requires_grad_(False)
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.5)
    block = layer.res_blocks[0]
    gen = torch.Generator().manual_seed(Ls)
    B = 6
    x = torch.randn(B, Ls, C, generator=gen, dtype=torch.float64)
    lens = torch.tensor([0, 1, Ls, Ls - 1, 2 % (Ls + 1), Ls // 2])
    ps = [None if p is None else p.detach() for p in block.stage_params()]
    (stride, R, dil), (lstride, lR, ldil) = block_modes(block, Ls)
    full = block_f64(x, lens, ps, stride, R, dil)
    want_full = Fh.causal_conv_block(x, lens, block, False)  # the CPU path: the reference's formulas
    assert float((full - want_full).abs().max()) <= 1e-12
    last = block_f64(x, lens, ps, lstride, lR, ldil, last=True)[:, -1]
    want_last = layer(x, lens)
    assert torch.equal(want_last, Fh.causal_conv_block(x, lens, block, True))
    assert float((last - want_last).abs().max()) <= 1e-12
    assert float((full[torch.arange(B), lens - 1] - want_last).abs().max()) <= 1e-12


def test_padding_rows_are_zero_at_the_input_of_every_conv_not_only_the_first():
    """with padding rows zeroed at the first conv only, the bias and beta of an earlier stage leak into a later conv through
    rows the reference does not have: the restatement then misses the reference by far more than rounding"""
    from rec_pangu_amd.models.layers import NextItNetLayer
    torch.manual_seed(5)
    for one_masked in (False, True):
        layer = NextItNetLayer(6, [1], one_masked, 3).double().requires_grad_(False)
        for p in layer.parameters():
            torch.nn.init.normal_(p, std=0.5)
        block = layer.res_blocks[0]
        x = torch.randn(4, 8, 6, dtype=torch.float64)
        lens = torch.tensor([1, 2, 3, 8])  # short rows: most virtual rows of last mode are padding
        ps = [None if p is None else p.detach() for p in block.stage_params()]
        _, (stride, R, dil) = block_modes(block, 8)
        want = layer(x, lens)
        right = block_f64(x, lens, ps, stride, R, dil, last=True)[:, -1]
        wrong = block_f64(x, lens, ps, stride, R, dil, last=True, pad_every_conv=False)[:, -1]
        assert float((right - want).abs().max()) <= 1e-12
        assert float((wrong[:3] - want[:3]).abs().max()) > 1e-3  # the short rows break
        assert float((wrong[3] - want[3]).abs().max()) <= 1e-12  # the full row reaches back 6 positions at most: no padding row


def test_later_blocks_of_a_row_without_history_see_the_first_blocks_output():
    """the layer hands later blocks the length L for an empty row (NextItNetLayer._forward_hip); the same rule on the CPU
    formulas gives the reference's value"""
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd.models.layers import NextItNetLayer
    torch.manual_seed(7)
    layer = NextItNetLayer(6, [1, 2], False, 3).double().requires_grad_(False)
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.5)
    x = torch.randn(3, 5, 6, dtype=torch.float64)
    lens = torch.tensor([0, 3, 5])
    later = torch.where(lens > 0, lens, torch.full_like(lens, 5))
    y = Fh.causal_conv_block(x, lens, layer.res_blocks[0], False)
    got = Fh.causal_conv_block(y, later, layer.res_blocks[1], True)
    assert float((got - layer(x, lens)).abs().max()) <= 1e-12


# ---- the model -------------------------------------------------------------------------------------------------------------
def build(case, seed):
    from rec_pangu_amd.models.sequence import NextItNet
    torch.manual_seed(seed)
    return NextItNet(ENC, dict(CONFIG, **MODELS[case])).train()


def run_case(case, g, device="cpu", make_opt=None):
    """(out, grads, adam2, adam2_out, out2, grads2) of our model on `device`, as the generator runs the reference (shared with
    tests/test_hip_nextitnet.py); the last two are None without a batch2/ group"""
    seed = int(g["seed"])
    batch = {k: v.to(device) for k, v in g["batch"].items()}
    model = build(case, seed).to(device)
    res = model({k: v.clone() for k, v in batch.items()})
    model.zero_grad()
    res["loss"].backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
    out2 = grads2 = None
    if "batch2" in g:
        model.zero_grad()
        res = model({k: v.to(device) for k, v in g["batch2"].items()})
        res["loss"].backward()
        out2 = {k: v.detach().cpu() for k, v in res.items()}
        grads2 = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
    model = build(case, seed).to(device)
    opt = (make_opt(model) if make_opt is not None
           else torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999), eps=1e-08, weight_decay=0))
    for _ in range(2):
        model({k: v.clone() for k, v in batch.items()})["loss"].backward()
        opt.step()
        model.zero_grad()
    adam2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        r = model({k: v.clone() for k, v in batch.items()}, is_training=False)
    return out, grads, adam2, {k: v.detach().cpu() for k, v in r.items()}, out2, grads2


def check_against_golden(g, out, grads, adam2, adam2_out, out2, grads2, closer=close):
    assert set(out) == set(g["out"]) == {"user_emb", "loss"}
    for k, v in g["out"].items():
        closer("out", out[k], v, f"out {k}")
    assert set(grads) == set(g["grad"]) == set(g["init"]) - {"fc.weight"}  # (fc is never used: no gradient)
    for k, v in g["grad"].items():
        closer("grad", grads[k], v, f"grad {k}")
    assert list(adam2) == list(g["adam2"])
    for k, v in g["adam2"].items():
        closer("adam2", adam2[k], v, f"adam2 {k}")
    assert torch.equal(adam2["fc.weight"], g["init"]["fc.weight"])  # Adam never moves it
    assert set(adam2_out) == set(g["adam2_out"]) == {"user_emb"}
    for k, v in g["adam2_out"].items():
        closer("adam2_out", adam2_out[k], v, f"adam2_out {k}")
    if "batch2" in g:
        for k, v in g["out2"].items():
            closer("out", out2[k], v, f"out2 {k}")
        assert set(grads2) == set(g["grad2"])
        for k, v in g["grad2"].items():
            closer("grad", grads2[k], v, f"grad2 {k}")
    else:
        assert out2 is None


@pytest.mark.parametrize("case", list(MODELS))
def test_model_matches_the_reference_on_cpu(case):
    g = load_golden(f"model_{case}.npz")
    check_against_golden(g, *run_case(case, g))


def test_the_fixtures_hold_their_edge_cases():
    g = load_golden("model_nextitnet_default.npz")
    b = g["batch"]
    lens = b["hist_mask_list"].sum(1)
    assert 1 in lens.tolist() and L in lens.tolist() and any(1 < n < L for n in lens.tolist())
    assert int(g["batch2"]["hist_mask_list"].sum(1).min()) == 0  # the row without history
    empty = int(g["batch2"]["hist_mask_list"].sum(1).argmin())
    assert float(g["out2"]["user_emb"][empty].abs().max()) > 0  # a function of the biases, not zero
    # at L = 6 the dilation-8 conv reads padding through every tap but the last, the dilation-4 conv through its first:
    # exact zeros in the reference's fp32 gradient, and Adam leaves those entries where they were
    w8, w4 = "nextit_layer.res_blocks.1.conv2.conv.weight", "nextit_layer.res_blocks.1.conv1.conv.weight"
    assert float(g["grad"][w8][:, :, :2].abs().max()) == 0 and float(g["grad"][w8][:, :, 2].abs().max()) > 0
    assert float(g["grad"][w4][:, :, 0].abs().max()) == 0 and float(g["grad"][w4][:, :, 1].abs().max()) > 0
    assert torch.equal(g["adam2"][w8][:, :, :2], g["init"][w8][:, :, :2])
    for other in ("model_nextitnet_d12_k2.npz", "model_nextitnet_one_masked.npz"):
        o = load_golden(other)
        assert all(torch.equal(v, o["batch"][k]) for k, v in b.items()) and "batch2" not in o
        assert all(float(v.abs().amax(dim=(0, 1)).min()) > 0 for k, v in o["grad"].items() if k.endswith("conv.weight"))  # every tap is live
    assert load_golden("model_nextitnet_one_masked.npz")["init"]["nextit_layer.res_blocks.0.conv2.conv.weight"].shape == (4, 4, 3)


def block_keys(i, one_masked):
    if one_masked:
        names = ["layer_norm1.gamma", "layer_norm1.beta", "conv1.weight", "conv1.bias", "layer_norm2.gamma", "layer_norm2.beta",
                 "conv2.conv.weight", "conv2.conv.bias", "layer_norm3.gamma", "layer_norm3.beta", "conv3.weight", "conv3.bias"]
    else:
        names = ["conv1.conv.weight", "conv1.conv.bias", "layer_norm1.gamma", "layer_norm1.beta",
                 "conv2.conv.weight", "conv2.conv.bias", "layer_norm2.gamma", "layer_norm2.beta"]
    return [f"nextit_layer.res_blocks.{i}.{n}" for n in names]


@pytest.mark.parametrize("case", list(MODELS))
def test_state_dict_and_init_stream(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case, int(g["seed"]))
    sd = model.state_dict()
    one = MODELS[case].get("one_masked", False)
    assert list(sd) == list(g["init"]) == ["item_emb.weight"] + [k for i in range(2) for k in block_keys(i, one)] + ["fc.weight"]
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k  # same draws from the same stream
    assert sd["fc.weight"].shape == (D, D) and sd["nextit_layer.res_blocks.0.layer_norm1.gamma"].shape == (1, D, 1)
    assert not torch.equal(sd["nextit_layer.res_blocks.0.layer_norm1.gamma"], torch.ones(1, D, 1))  # Kaiming, like the reference


def test_config_keys_and_defaults_are_the_references():
    from rec_pangu_amd.models.layers import ResBlockOneMasked, ResBlockTwoMasked
    from rec_pangu_amd.models.sequence import NextItNet
    m = NextItNet(ENC, CONFIG)
    assert (m.dilations, m.one_masked, m.kernel_size, m.feat_drop) == (None, False, 3, 0)
    blocks = m.nextit_layer.res_blocks
    assert [type(b) for b in blocks] == [ResBlockTwoMasked] * 2 and [b.dilation for b in blocks] == [1, 4]
    assert blocks[1].conv1.conv.dilation == (4,) and blocks[1].conv2.conv.dilation == (8,) and blocks[1].conv2.padding == 16
    assert m.nextit_layer.feat_drop is None and blocks[0].layer_norm1.epsilon == 1e-5
    m = NextItNet(ENC, dict(CONFIG, one_masked=True, feat_drop=0.2))
    blocks = m.nextit_layer.res_blocks
    assert [type(b) for b in blocks] == [ResBlockOneMasked] * 3 and [b.dilation for b in blocks] == [1, 2, 4]
    assert blocks[2].conv1.weight.shape == (D // 2, D, 1) and blocks[2].conv2.conv.dilation == (4,)
    assert m.nextit_layer.feat_drop.p == 0.2


def test_the_model_and_the_layers_are_exported():
    import rec_pangu_amd  # noqa: F401
    import rec_pangu_amd.models as models
    from rec_pangu_amd.models import layers, sequence
    from rec_pangu_amd.models.layers import conv
    from rec_pangu_amd.models.sequence import NextItNet
    assert sequence.__all__ == ["YotubeDNN", "GRU4Rec", "NARM"]
    assert models.sequence.NextItNet is NextItNet and NextItNet.__module__ == "rec_pangu_amd.models.sequence.nextitnet"
    for name in ("NextItNetLayer", "ResBlockOneMasked", "ResBlockTwoMasked", "MaskedConv1d", "LayerNorm"):
        assert name in layers.__all__ and getattr(layers, name) is getattr(conv, name)
    assert "NextItNet" in rec_pangu_amd.__doc__


def test_a_batch_of_one_trains_and_a_row_without_history_does_not_raise():
    model = build("nextitnet_default", 1)
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1.0, 1, 0, 0, 0, 0]]),
            "target_item": torch.tensor([[5]])}
    res = model(data)
    assert res["user_emb"].shape == (1, D) and res["loss"].dim() == 0
    res["loss"].backward()
    assert model.fc.weight.grad is None and float(model.item_emb.weight.grad.abs().max()) > 0
    model.zero_grad()
    data = {"hist_item_list": torch.zeros(1, 6, dtype=torch.long), "hist_mask_list": torch.zeros(1, 6, dtype=torch.long),
            "target_item": torch.tensor([[5]])}
    res = model(data)
    res["loss"].backward()
    # gradients reach biases, gamma, beta and weights, and no embedding row but the target's (through the loss head)
    rows = model.item_emb.weight.grad.abs().sum(1)
    scores_only = torch.softmax(res["user_emb"].detach() @ model.item_emb.weight.detach().t(), -1)
    scores_only[0, 5] -= 1
    assert torch.allclose(model.item_emb.weight.grad, scores_only.t() @ res["user_emb"].detach(), atol=1e-6) and float(rows.min()) > 0
    assert float(model.nextit_layer.res_blocks[0].conv1.conv.bias.grad.abs().max()) > 0


def test_sequence_trainer_epoch(tmp_path):
    from rec_pangu_amd.models.sequence import NextItNet
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, _ = _tiny_loaders()
    torch.manual_seed(0)
    model = NextItNet(enc, cfg)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    trainer.fit(model, train, valid, epoch=1, lr=1e-2, device=torch.device("cpu"), topk_list=[5, 10])
    assert len(trainer.log_df) == 1
    assert all(torch.equal(before[k], v) == (k == "fc.weight") for k, v in model.state_dict().items())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rp_causal_conv_fits", "rp_causal_conv_geometry", "rp_causal_conv_workspace_bytes", "rp_causal_conv_fwd",
               "rp_causal_conv_bwd"]


def test_new_symbols_are_declared_bound_and_exported():
    from rec_pangu_amd import hip
    assert hip.ABI_VERSION == 108
    header = open(os.path.join(ROOT, "include", "rec_pangu_hip.h")).read()
    lib = hip.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in the header"
        assert name in hip.EXPORTED_SYMBOLS and len(hip._SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        getattr(lib, name)
    assert lib.rp_version() == 108


def test_fits_and_geometry_agree():
    from rec_pangu_amd import hip
    g = hip.causal_conv_geometry()
    assert {k: g[k] for k in ("max_c", "max_k", "max_l", "max_lc")} == {"max_c": 128, "max_k": 5, "max_l": 128, "max_lc": 8192}
    assert g["lds_bytes"] <= 160 * 1024
    for one in (False, True):
        # the region the kernel must cover: every C in 2 .. 128, k in 1 .. 5, L <= 128 with L C <= 8192
        for Cw in range(2, g["max_c"] + 1):
            Lmax = min(g["max_l"], g["max_lc"] // Cw)
            assert all(hip.causal_conv_fits(Ls, Cw, k, one) for Ls in (1, 2, 31, 32, 33, 64, 65, 96, 97, Lmax) if Ls <= Lmax
                       for k in (1, g["max_k"])), (Cw, one)
            assert not hip.causal_conv_fits(Lmax + 1, Cw, 3, one)
        assert not hip.causal_conv_fits(8, 1, 3, one) and not hip.causal_conv_fits(8, g["max_c"] + 1, 3, one)
        assert not hip.causal_conv_fits(0, 8, 3, one) and not hip.causal_conv_fits(8, 8, 0, one)
        assert not hip.causal_conv_fits(8, 8, g["max_k"] + 1, one) and not hip.causal_conv_fits(8, 0, 3, one)
    for case in CASES + ILL:
        assert hip.causal_conv_fits(case[4], case[1], case[2], bool(case[0])), case
    assert hip.causal_conv_rows(3, False) == rows_of(3, False) == 7 and hip.causal_conv_rows(5, True) == rows_of(5, True) == 5


def test_entry_points_reject_bad_arguments_without_a_launch():
    from rec_pangu_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    two = (ctypes.c_void_p * 12)(*[p, p, None, p, p, None, p, p, None, p, p, None])
    three = (ctypes.c_void_p * 12)(*([p] * 12))
    holes = (ctypes.c_void_p * 12)(*([p] * 11 + [None]))
    n0 = hip.launch_count()
    big = 1 << 40

    def fwd(Ls=8, Cw=8, k=3, d=1, one=0, last=0, x=p, lens=p, params=two, out=p, ws=p, nbytes=big):
        return lib.rp_causal_conv_fwd(x, lens, 2, Ls, Cw, k, d, one, last, params, out, ws, nbytes, None)

    def bwd(Ls=8, Cw=8, k=3, d=1, one=0, last=0, x=p, lens=p, dout=p, params=two, dx=p, grads=two, ws=p, nbytes=big):
        return lib.rp_causal_conv_bwd(x, lens, dout, 2, Ls, Cw, k, d, one, last, params, dx, grads, ws, nbytes, None)

    for f in (fwd, bwd):
        for last in (0, 1):
            for one, ok_params in ((0, two), (1, three)):
                kw = dict(one=one, last=last, params=ok_params)
                assert f(k=0, **kw) == -1 and f(Cw=0, **kw) == -1 and f(Ls=0, **kw) == -1 and f(d=0, **kw) == -1
                assert f(k=6, **kw) == -1 and f(Cw=129, **kw) == -1 and f(Ls=129, **kw) == -1 and f(Ls=128, Cw=65, **kw) == -1
                assert f(Cw=1, **kw) == -1 and f(d=-2, **kw) == -1
                assert f(x=None, **kw) == -1 and f(lens=None, **kw) == -1 and f(ws=None, **kw) == -1
                assert f(nbytes=16, **kw) == -1  # workspace too small
                assert f(one=one, last=last, params=None) == -1
        assert f(one=1, params=two) == -1 and f(one=1, params=holes) == -1  # a missing parameter of a stage the block has
    assert b"causal_conv" in lib.rp_last_error()
    assert fwd(out=None) == -1 and bwd(dout=None) == -1 and bwd(dx=None) == -1 and bwd(grads=None) == -1
    assert bwd(one=1, params=three, grads=holes) == -1
    n = ctypes.c_size_t(0)
    assert lib.rp_causal_conv_workspace_bytes(2, 8, 8, 3, 0, 0, 1, None) == -1
    assert lib.rp_causal_conv_workspace_bytes(2, 8, 8, 0, 0, 0, 1, ctypes.byref(n)) == -1
    assert lib.rp_causal_conv_workspace_bytes(-1, 8, 8, 3, 0, 0, 1, ctypes.byref(n)) == -1
    assert lib.rp_causal_conv_geometry(None, None, None, None, None) == -1
    # the backward's workspace holds the forward's; last mode needs less than full mode; an empty batch launches nothing
    sizes = {}
    for one in (0, 1):
        for last in (0, 1):
            for back in (0, 1):
                assert lib.rp_causal_conv_workspace_bytes(4096, 50, 64, 3, one, last, back, ctypes.byref(n)) == 0
                sizes[one, last, back] = n.value
        assert sizes[one, 0, 0] == sizes[one, 1, 0] < sizes[one, 1, 1] < sizes[one, 0, 1]
    assert lib.rp_causal_conv_fwd(p, p, 0, 8, 8, 3, 1, 0, 0, two, p, p, big, None) == 0
    assert lib.rp_causal_conv_bwd(p, p, p, 0, 8, 8, 3, 1, 0, 0, two, p, two, p, big, None) == 0
    assert hip.launch_count() == n0
