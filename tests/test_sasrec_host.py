"""SASRec and the TransformerEncoder on the CPU (plumbing, no GPU): the model against the three golden files produced by running
the reference (tests/golden/make_golden_sasrec.py), its state_dict / init stream, encode_last against the gathered row, the
reference's ValueError, the import surface, the float64 restatement of the masked attention the GPU tests use (checked here
against torch's composed fp32 formulation), and the declaration / binding / argument checks of the new C entry points.

Bars of the model comparisons are tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, the other tolerance 1e-6,
the tighter of the two readings per element (the generator chose its seeds against a tenth of that).

The key biases after Adam are the one exception, and not a matter of tolerance: their gradient is ZERO in exact arithmetic
(q_i . (k_j + b) shifts every score of a row by q_i . b, which the softmax does not see), the reference's fp32 gradient there
is rounding noise near 1e-9, and Adam normalises that noise into steps of the order of lr — the reference's own fp32 and
float64 runs differ by 1e4 bars in those entries at every seed (make_golden_sasrec.py).  So `grad/` holds them to the bar
like every gradient, `adam2_out/` (which does not depend on them) is compared in full, and in `adam2/` they are held to what
Adam guarantees instead: a step moves an entry by at most lr |m_hat| / sqrt(v_hat), which is lr at step 1 (m_hat = g,
v_hat = g^2) and, at step 2, lr |0.09 g1 + 0.1 g2| / 0.19 over sqrt((0.000999 g1^2 + 0.001 g2^2) / 0.001999) <= 1.002 lr by
Cauchy-Schwarz: |adam2 - init| <= 2.1 lr."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from test_sequence_host import close

torch.set_num_threads(1)

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
NO_DROP = {"hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0}
CASES = {
    "sasrec_train": (dict(NO_DROP, n_layers=2, n_heads=2, inner_size=16), True),
    "sasrec_eval": ({}, False),
    "sasrec_l1_relu": (dict(NO_DROP, n_layers=1, n_heads=1, hidden_act="relu"), True),
}
KEY_BIAS = "multi_head_attention.key.bias"
LR = 1e-2


def layer_keys(i):
    att = [f"{m}.{p}" for m in ("query", "key", "value", "dense", "LayerNorm") for p in ("weight", "bias")]
    ff = [f"{m}.{p}" for m in ("dense_1", "dense_2", "LayerNorm") for p in ("weight", "bias")]
    return [f"self_attention.layer.{i}.multi_head_attention.{k}" for k in att] + \
        [f"self_attention.layer.{i}.feed_forward.{k}" for k in ff]


def build(case, seed):
    from rec_pangu_amd.models.sequence import SASRec
    cfg, train = CASES[case]
    torch.manual_seed(seed)
    model = SASRec(ENC, dict(CONFIG, **cfg))
    return model.train() if train else model.eval()


def run_case(case, g, device="cpu", make_opt=None):
    """(out, grads, adam2, adam2_out) of our model on `device`, as the generator runs the reference (shared with
    tests/test_hip_sasrec.py)"""
    seed = int(g["seed"])
    batch = {k: v.to(device) for k, v in g["batch"].items()}
    model = build(case, seed).to(device)
    res = model({k: v.clone() for k, v in batch.items()})
    model.zero_grad()
    res["loss"].backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
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
    return out, grads, adam2, {k: v.detach().cpu() for k, v in r.items()}


def check_against_golden(g, out, grads, adam2, adam2_out, closer=close):
    """test_sequence_host.check_against_golden with the key biases' adam2 held to Adam's step bound (see the module's text);
    shared with tests/test_hip_sasrec.py, which passes what the HIP path computed and its own per-element `closer`"""
    assert set(out) == set(g["out"]) == {"user_emb", "loss"}
    for k, v in g["out"].items():
        closer("out", out[k], v, f"out {k}")
    assert set(grads) == set(g["grad"])
    for k, v in g["grad"].items():
        closer("grad", grads[k], v, f"grad {k}")
    assert list(adam2) == list(g["adam2"])
    n_key_bias = 0
    for k, v in g["adam2"].items():
        if k.endswith(KEY_BIAS):
            n_key_bias += 1
            assert float((adam2[k] - g["init"][k]).abs().max()) <= 2.1 * LR, k
            assert float((v - g["init"][k]).abs().max()) <= 2.1 * LR, k  # (the reference's own noise obeys the same bound)
        else:
            closer("adam2", adam2[k], v, f"adam2 {k}")
    assert n_key_bias == sum(k.endswith(KEY_BIAS) for k in g["init"]) >= 1
    assert set(adam2_out) == set(g["adam2_out"]) == {"user_emb"}
    for k, v in g["adam2_out"].items():
        closer("adam2_out", adam2_out[k], v, f"adam2_out {k}")


# ---- the float64 restatement the GPU tests compare against ---------------------------------------------------------------------
def attention_f64(qkv, mask, heads, keep=None, p=0.0):
    """softmax(Q K^T / sqrt(dh) + m) V per (b, head) in float64 from qkv [B L, 3 D] (Q | K | V, head h at columns
    [h dh, (h + 1) dh) of each) and mask [B, L] (non-zero = content): m = 0 where key j is content and j <= i, else -1e6;
    keep [B, heads, L, L] (explicit dropout decisions, None for none) multiplies the probabilities with 1 / (1 - p).
    -> ctx [B L, D] head-interleaved.  Differentiable: the GPU tests take float64 autograd of it."""
    B, Ls = mask.shape
    Dm = qkv.shape[1] // 3
    dh = Dm // heads
    x = qkv.double().view(B, Ls, 3, heads, dh)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(dh)
    tri = torch.ones(Ls, Ls, dtype=torch.bool, device=qkv.device).tril()
    visible = (mask != 0)[:, None, None, :] & tri[None, None]
    s = s + torch.where(visible, 0.0, -1e6).double()
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.double() / (1.0 - p)
    return torch.einsum("bhij,bjhd->bihd", pr, v).reshape(B * Ls, Dm)


def composed_fp32(qkv, mask, heads, keep=None, p=0.0):
    """the reference's ops (trainformer.py:70-92 behind the projections, base_model.py get_attention_mask) in the input's dtype"""
    from rec_pangu_amd.models.base_model import SequenceBaseModel
    B, Ls = mask.shape
    Dm = qkv.shape[1] // 3
    dh = Dm // heads
    add = SequenceBaseModel.get_attention_mask(None, mask.to(qkv.dtype))
    q, k, v = (qkv[:, i * Dm:(i + 1) * Dm].reshape(B, Ls, heads, dh) for i in range(3))
    scores = torch.matmul(q.permute(0, 2, 1, 3), k.permute(0, 2, 3, 1)) / math.sqrt(dh) + add
    probs = torch.softmax(scores, dim=-1)
    if keep is not None:
        probs = probs * keep.to(qkv.dtype) / (1.0 - p)
    return torch.matmul(probs, v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3).contiguous().view(B * Ls, Dm)


def bar(ref):
    """the project's per-tensor bar against float64: 1e-4 max(1e-2, max |ref|)"""
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def masks(B, Ls, gen):
    """[B, L] float masks with mask[:, 0] = 1: full, length 1, padded tails, a hole inside"""
    m = torch.ones(B, Ls)
    for b in range(B):
        kind = b % 4
        if kind == 1:
            m[b, 1:] = 0
        elif kind == 2:
            m[b, int(torch.randint(1, Ls + 1, (1,), generator=gen)):] = 0
        elif kind == 3 and Ls > 2:
            m[b, int(torch.randint(1, Ls - 1, (1,), generator=gen))] = 0
    return m


@pytest.mark.parametrize("B,Ls,heads,dh", [(1, 1, 1, 1), (3, 7, 2, 4), (5, 33, 4, 16), (2, 65, 1, 20)])
def test_the_float64_restatement_is_the_composed_formulation(B, Ls, heads, dh):
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(B * 1000 + Ls)
    qkv = torch.randn(B * Ls, 3 * heads * dh, generator=gen)
    mask = masks(B, Ls, gen)
    keep = (torch.rand(B, heads, Ls, Ls, generator=gen) >= 0.3)
    for kp, p in ((None, 0.0), (keep, 0.3)):
        ref = attention_f64(qkv, mask, heads, kp, p)
        assert float((composed_fp32(qkv.double(), mask, heads, kp, p) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
        assert float((composed_fp32(qkv, mask, heads, kp, p).double() - ref).abs().max()) <= bar(ref)
    ref = attention_f64(qkv, mask, heads)
    got = Fh.seq_attention(qkv, mask.long(), heads, p=0.5, training=False)  # (the CPU path; eval: no dropout; any mask dtype)
    assert got.dtype == torch.float32 and float((got.double() - ref).abs().max()) <= bar(ref)
    qpos = mask.sum(1).long() - 1
    qpos[0] = -1
    last = Fh.seq_attention(qkv, mask, heads, qpos=qpos)
    want = ref.view(B, Ls, -1)[torch.arange(B), qpos.clamp(min=0)] * (qpos >= 0)[:, None]
    assert float((last.double() - want).abs().max()) <= bar(ref) and float(last[0].abs().max()) == 0
    D_ = heads * dh
    compact = Fh.seq_attention(qkv[:, D_:], mask, heads, qpos=qpos, q=qkv.view(B, Ls, -1)[torch.arange(B), qpos.clamp(min=0), :D_])
    assert torch.equal(compact, last)


def test_seq_act_on_the_cpu_is_the_references_formula():
    from rec_pangu_amd import functional as Fh
    x = torch.linspace(-8, 8, 101).view(1, -1)
    assert torch.equal(Fh.seq_act(x, "gelu"), x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))))
    assert torch.equal(Fh.seq_act(x, "swish"), x * torch.sigmoid(x))
    with pytest.raises(KeyError):
        Fh.seq_act(x, "relu")


# ---- state, init, surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_state_dict_and_init_stream(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case, int(g["seed"]))
    sd = model.state_dict()
    n_layers = CASES[case][0].get("n_layers", 2)
    assert list(sd) == list(g["init"]) == ["item_emb.weight"] + [k for i in range(n_layers) for k in layer_keys(i)]
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k  # same draws from the same stream
    inner = CASES[case][0].get("inner_size", 32)
    assert sd["self_attention.layer.0.feed_forward.dense_1.weight"].shape == (inner, D)
    assert sd["self_attention.layer.0.multi_head_attention.query.weight"].shape == (D, D)


def test_config_keys_and_defaults_are_the_references():
    from rec_pangu_amd.models.sequence import SASRec
    m = SASRec(ENC, dict(CONFIG, hidden_size=999))
    assert (m.n_layers, m.n_heads, m.inner_size, m.hidden_dropout_prob, m.attn_dropout_prob, m.hidden_act, m.layer_norm_eps) == \
        (2, 4, 32, 0.1, 0.1, "gelu", 0.001)
    layer = m.self_attention.layer[1]
    att, ff = layer.multi_head_attention, layer.feed_forward
    assert (att.num_attention_heads, att.attention_head_size, att.attn_dropout.p, att.out_dropout.p) == (4, 2, 0.1, 0.1)
    assert att.query.in_features == D and att.LayerNorm.eps == 0.001 and ff.dropout.p == 0.1  # hidden_size is ignored
    assert m.self_attention.layer[0] is not layer and \
        m.self_attention.layer[0].feed_forward.dense_1.weight.data_ptr() != ff.dense_1.weight.data_ptr()  # deep copies


def test_the_model_and_the_layers_are_exported():
    import rec_pangu_amd  # noqa: F401
    import rec_pangu_amd.models as models
    from rec_pangu_amd.models import layers, sequence
    from rec_pangu_amd.models.sequence import SASRec
    from rec_pangu_amd.models.layers import transformer
    assert sequence.__all__ == ["YotubeDNN", "GRU4Rec", "NARM"]
    assert models.sequence.SASRec is SASRec and SASRec.__module__ == "rec_pangu_amd.models.sequence.sasrec"
    for name in ("FeedForward", "TransformerLayer", "TransformerEncoder"):
        assert name in layers.__all__ and getattr(layers, name) is getattr(transformer, name)
    assert transformer.MultiHeadAttention is not layers.MultiHeadAttention  # (layers' is the field attention of AutoInt)
    enc = layers.TransformerEncoder()
    assert len(enc.layer) == 2 and enc.layer[0].multi_head_attention.num_attention_heads == 2
    assert enc.layer[0].feed_forward.dense_1.weight.shape == (256, 64) and enc.layer[0].feed_forward.LayerNorm.eps == 1e-12
    assert [k for k in enc.state_dict() if k.startswith("layer.1.feed_forward.")] == \
        [f"layer.1.feed_forward.{m}.{p}" for m in ("dense_1", "dense_2", "LayerNorm") for p in ("weight", "bias")]


def test_a_width_the_heads_do_not_divide_raises_the_references_error():
    from rec_pangu_amd.models import layers
    from rec_pangu_amd.models.sequence import SASRec
    with pytest.raises(ValueError, match=r"The hidden size \(8\) is not a multiple of the number of attention heads \(3\)"):
        SASRec(ENC, dict(CONFIG, n_heads=3))
    with pytest.raises(ValueError):
        layers.TransformerEncoder(n_heads=5, hidden_size=64)
    with pytest.raises(KeyError):
        layers.TransformerEncoder(hidden_act="elu")


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_model_matches_the_reference_on_cpu(case):
    g = load_golden(f"model_{case}.npz")
    check_against_golden(g, *run_case(case, g))


@pytest.mark.parametrize("case", list(CASES))
def test_encode_last_is_the_gathered_row(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case, int(g["seed"]))
    hist, mask = g["batch"]["hist_item_list"], g["batch"]["hist_mask_list"]
    x = model.item_emb(hist)
    full = model.self_attention(x, model.get_attention_mask(mask), output_all_encoded_layers=True)
    assert len(full) == model.n_layers and len(model.self_attention(x, model.get_attention_mask(mask), False)) == 1
    want = model.gather_indexes(full[-1], mask.sum(-1) - 1)
    assert torch.equal(model.self_attention.encode_last(x, mask), want)
    assert torch.equal(model.self_attention.encode_last(x, mask.float()), want)  # any mask dtype
    assert torch.equal(model.self_attention(x, mask)[-1], full[-1])  # a [B, L] content mask is the same thing
    assert torch.equal(model({k: v for k, v in g["batch"].items()}, is_training=False)["user_emb"], want)


def test_the_fixture_batch_holds_its_edge_cases():
    b = load_golden("model_sasrec_train.npz")["batch"]
    hist, mask, tgt = b["hist_item_list"], b["hist_mask_list"], b["target_item"].view(-1)
    lens = mask.sum(1)
    assert hist.shape == (5, L) and torch.equal(mask, (torch.arange(L)[None] < lens[:, None]).long())  # right-padded
    assert 1 in lens.tolist() and L in lens.tolist() and any(1 < n < L for n in lens.tolist())
    assert int(lens.min()) >= 1  # no empty row: the reference raises there
    assert len(set(tgt.tolist())) < len(tgt) and 0 in tgt.tolist() and V - 1 in tgt.tolist()
    for other in ("model_sasrec_eval.npz", "model_sasrec_l1_relu.npz"):
        assert all(torch.equal(v, load_golden(other)["batch"][k]) for k, v in b.items())


def test_a_batch_of_one_trains_and_a_row_without_history_raises_like_the_reference():
    model = build("sasrec_train", 1)
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0]]),
            "target_item": torch.tensor([[5]])}
    res = model(data)
    assert res["user_emb"].shape == (1, D) and res["loss"].dim() == 0
    res["loss"].backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(model.item_emb.weight.grad.abs().max()) > 0
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0], [0] * 6]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0], [0] * 6]),
            "target_item": torch.tensor([[5], [6]])}
    with pytest.raises(RuntimeError):  # gather with index -1
        model(data)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rp_seq_attn_fits", "rp_seq_attn_geometry", "rp_seq_attn_fwd", "rp_seq_attn_fwd_dev", "rp_seq_attn_bwd",
               "rp_seq_attn_bwd_dev", "rp_seq_attn_keep_mask", "rp_seq_act_fwd", "rp_seq_act_bwd", "rp_seq_take_fwd",
               "rp_seq_take_bwd"]


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
    assert (hip.SEQ_ACT_GELU, hip.SEQ_ACT_SWISH) == (0, 1)


def test_fits_and_geometry_agree():
    from rec_pangu_amd import hip
    g = hip.seq_attn_geometry()
    assert g == {"max_l": 128, "max_dh": 64, "row_tile": 64, "min_dh_tile": 4}
    assert hip.seq_attn_fits(1, 1, 1) and hip.seq_attn_fits(g["max_l"], 7, g["max_dh"])
    assert not hip.seq_attn_fits(g["max_l"] + 1, 1, 8) and not hip.seq_attn_fits(8, 1, g["max_dh"] + 1)
    assert not hip.seq_attn_fits(0, 1, 8) and not hip.seq_attn_fits(8, 0, 8) and not hip.seq_attn_fits(8, 1, 0)


def test_entry_points_reject_bad_arguments_without_a_launch():
    from rec_pangu_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    n0 = hip.launch_count()
    fwd = lambda Ls, heads, dh, ldq=4096, ldkv=4096, q=p, drop=0.0, qpos=None, compact=0: lib.rp_seq_attn_fwd(  # noqa: E731
        q, ldq, compact, p, ldkv, p, qpos, 2, Ls, heads, dh, drop, 0, 0, p, p, None)
    bwd = lambda Ls, heads, dh, lddq=4096, lddkv=4096, dq=p: lib.rp_seq_attn_bwd(  # noqa: E731
        p, 4096, 0, p, 4096, p, None, p, p, p, 2, Ls, heads, dh, 0.0, 0, 0, dq, lddq, p, lddkv, None)
    for Ls, heads, dh in [(129, 1, 8), (0, 1, 8), (8, 0, 8), (8, 1, 65), (8, 1, 0)]:
        assert fwd(Ls, heads, dh) == -1 and bwd(Ls, heads, dh) == -1, (Ls, heads, dh)
    assert b"1 <= L <= 128" in lib.rp_last_error()
    assert fwd(8, 2, 8, ldq=15) == -1 and fwd(8, 2, 8, ldkv=31) == -1 and fwd(8, 2, 8, q=None) == -1
    assert fwd(8, 2, 8, drop=1.0) == -1 and fwd(8, 2, 8, drop=-0.1) == -1 and fwd(8, 2, 8, compact=1) == -1
    assert bwd(8, 2, 8, lddq=15) == -1 and bwd(8, 2, 8, lddkv=31) == -1 and bwd(8, 2, 8, dq=None) == -1
    assert lib.rp_seq_attn_fwd_dev(p, 64, 0, p, 64, p, None, 2, 8, 2, 8, 0.1, 0, 0, None, p, p, None) == -1
    assert lib.rp_seq_attn_bwd_dev(p, 64, 0, p, 64, p, None, p, p, p, 2, 8, 2, 8, 0.1, 0, 0, None, p, 64, p, 64, None) == -1
    assert lib.rp_seq_attn_keep_mask(2, 129, 2, 0.1, 0, 0, None, p, None) == -1
    assert lib.rp_seq_attn_keep_mask(2, 8, 2, 0.1, 0, 0, None, None, None) == -1
    assert lib.rp_seq_attn_geometry(None, None, None, None) == -1
    assert lib.rp_seq_act_fwd(p, 8, p, 8, 2, 8, 2, None) == -1 and lib.rp_seq_act_fwd(p, 7, p, 8, 2, 8, 0, None) == -1
    assert lib.rp_seq_act_bwd(p, 8, p, 8, p, 8, 2, 8, 5, None) == -1 and lib.rp_seq_act_bwd(p, 8, None, 8, p, 8, 2, 8, 1, None) == -1
    assert lib.rp_seq_take_fwd(p, 7, p, 2, 4, 8, p, None) == -1 and lib.rp_seq_take_bwd(p, None, 2, 4, 8, p, None) == -1
    # empty batches launch nothing
    assert lib.rp_seq_attn_fwd(p, 64, 0, p, 64, p, None, 0, 8, 2, 8, 0.0, 0, 0, p, p, None) == 0
    assert lib.rp_seq_act_fwd(p, 8, p, 8, 0, 8, 0, None) == 0 and lib.rp_seq_take_fwd(p, 8, p, 0, 4, 8, p, None) == 0
    assert hip.launch_count() == n0
