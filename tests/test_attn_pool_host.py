"""STAMP and ComirecSA on the host: against the golden vectors the reference wrote (tests/golden/make_golden_stamp_sa.py), their
state_dict / init stream (ComirecSA's unused W3 included), the config defaults and the import surface;
Fh.attention_pool_reference in fp32 against an INDEPENDENT float64 statement with autograd (what the GPU tests compare the
kernel against): both modes, both activations, with and without the per-sample bias, rows of length 0, 1 and L, a hole in
valid at a position with a non-zero id, the uniform pooling of an all-masked softmax row; STAMP's empty row through the
model; one SequenceTrainer epoch per model; the declaration / binding / argument checks of the new C entry points.

Bars of the model comparisons are tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, the other tolerance 1e-6,
the tighter of the two readings per element (the generator chose its seeds against a tenth of that).  Kernel-level
comparisons use the project's per-tensor bar 1e-4 max(1e-2, max |ref|) against float64."""
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
CASES = {  # (class name, config, train mode), as the generator's
    "stamp": ("STAMP", {}, False),
    "stamp_d12": ("STAMP", {"embedding_dim": 12}, True),
    "comirecsa_train": ("ComirecSA", {"K": 4}, True),
    "comirecsa_eval": ("ComirecSA", {"K": 4}, False),
    "comirecsa_k2_d12": ("ComirecSA", {"K": 2, "embedding_dim": 12}, True),
}
W3 = "multi_interest_sa.W3"
STAMP_KEYS = ["stamp_layer.fc_a.weight", "stamp_layer.fc_a.bias", "stamp_layer.fc_t.weight", "stamp_layer.fc_t.bias",
              "stamp_layer.attn_i.weight", "stamp_layer.attn_t.weight", "stamp_layer.attn_t.bias", "stamp_layer.attn_s.weight",
              "stamp_layer.attn_e.weight"]
SA_KEYS = ["multi_interest_sa.W1", "multi_interest_sa.W2", W3]
LR = 1e-2
ERR_ARG = -1  # RP_ERR_ARG


def build(case, seed):
    from rec_pangu_amd.models import sequence
    name, cfg, train = CASES[case]
    torch.manual_seed(seed)
    model = getattr(sequence, name)(ENC, dict(CONFIG, **cfg))
    return model.train() if train else model.eval()


def run_case(case, g, device="cpu", make_opt=None):
    """(out, grads, adam2, adam2_out) of our model on `device`, as the generator runs the reference (shared with
    tests/test_hip_attn_pool_models.py)"""
    seed = int(g["seed"])
    batch = {k: v.to(device) for k, v in g["batch"].items()}
    model = build(case, seed).to(device)
    res = model({k: v.clone() for k, v in batch.items()})
    model.zero_grad()
    res["loss"].backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
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
    assert set(out) == set(g["out"]) == {"user_emb", "loss"}
    for k, v in g["out"].items():
        closer("out", out[k], v, f"out {k}")
    assert set(grads) == set(g["grad"])
    for k, v in g["grad"].items():
        closer("grad", grads[k], v, f"grad {k}")
    assert list(adam2) == list(g["adam2"])
    for k, v in g["adam2"].items():
        closer("adam2", adam2[k], v, f"adam2 {k}")
    assert set(adam2_out) == set(g["adam2_out"]) == {"user_emb"}
    for k, v in g["adam2_out"].items():
        closer("adam2_out", adam2_out[k], v, f"adam2_out {k}")


# ---- the independent statement the kernel and the CPU path are compared against ------------------------------------------------
def pool_f64(x, w1, w2, valid, c, act, norm):
    """sample by sample in x's dtype (use float64) -> (out [B, K, D], A [B, L, K]).  Under "softmax" the score of a position
    with valid = 0 is the constant -1e9: the softmax runs over all L positions, a masked position has weight
    exp(-1e9 - max) = 0 unless every position is masked, which gives 1 / L each."""
    f = torch.sigmoid if act == "sigmoid" else torch.tanh
    outs, As = [], []
    for b in range(x.shape[0]):
        pre = x[b] @ w1                       # [L, Dh]
        if c is not None:
            pre = pre + c[b]
        s = f(pre) @ w2                       # [L, K]
        on = (valid[b] != 0).unsqueeze(-1).expand_as(s)
        if norm == "mask":
            A = torch.where(on, s, torch.zeros_like(s))
        else:
            z = torch.where(on, s, torch.full_like(s, -1e9))
            e = torch.exp(z - z.max(dim=0, keepdim=True).values)
            A = e / e.sum(dim=0, keepdim=True)
        As.append(A)
        outs.append(A.t() @ x[b])
    return torch.stack(outs), torch.stack(As)


def pool_inputs(B, Lx, Dx, Dh, K, with_c, gen, w2_scale=1.0, lens_head=(1, None, 3, 2, 0)):
    """float64 inputs: the first rows have lengths 1, L, 3, 2 and 0 (clamped to L), one later row has a hole in valid"""
    x = torch.randn(B, Lx, Dx, generator=gen, dtype=torch.float64)
    w1 = torch.randn(Dx, Dh, generator=gen, dtype=torch.float64) * (1.0 / Dx ** 0.5)
    w2 = torch.randn(Dh, K, generator=gen, dtype=torch.float64) * (w2_scale / Dh ** 0.5)
    c = torch.randn(B, Dh, generator=gen, dtype=torch.float64) * 0.5 if with_c else None
    lens = torch.randint(1, Lx + 1, (B,), generator=gen)
    for b, n in enumerate(lens_head[:B]):
        lens[b] = Lx if n is None else min(n, Lx)
    valid = (torch.arange(Lx)[None, :] < lens[:, None]).to(torch.float64)
    if B > 5 and Lx >= 3:
        lens[5] = Lx
        valid[5] = 1.0
        valid[5, 1] = 0.0  # a hole: the row of x there is what it is
    g = torch.randn(B, K, Dx, generator=gen, dtype=torch.float64)
    return x, w1, w2, valid, c, g


def pool_grads(fn, x, w1, w2, valid, c, g, act, norm, dtype):
    """(out, A, dx, dc | None, dw1, dw2) of fn in `dtype` for the arriving gradient g"""
    xs, a1, a2 = (t.to(dtype).clone().requires_grad_(True) for t in (x, w1, w2))
    cs = None if c is None else c.to(dtype).clone().requires_grad_(True)
    out, A = fn(xs, a1, a2, valid.to(dtype), cs, act, norm)
    (out * g.to(dtype)).sum().backward()
    return out.detach(), A.detach(), xs.grad, None if cs is None else cs.grad, a1.grad, a2.grad


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def within(got, ref, what):
    ref = ref.detach()
    err = float((got.detach().cpu().double() - ref.double()).abs().max())
    print(f"{what}: max err {err:.3g} against bar {bar(ref):.3g} ({err / bar(ref):.3g} of it)")
    assert got.shape == ref.shape and err <= bar(ref), (what, err, bar(ref))
    return err / bar(ref)


MODES = {"stamp": ("sigmoid", "mask", True), "sa": ("tanh", "softmax", False)}


# ---- the models against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_state_dict_and_init_stream(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case, int(g["seed"]))
    sd = model.state_dict()
    assert list(sd) == list(g["init"])
    for k, v in g["init"].items():
        assert torch.equal(sd[k], v), k
    assert list(sd) == ["item_emb.weight"] + (STAMP_KEYS if CASES[case][0] == "STAMP" else SA_KEYS)


@pytest.mark.parametrize("case", list(CASES))
def test_model_matches_the_reference_on_cpu(case):
    g = load_golden(f"model_{case}.npz")
    check_against_golden(g, *run_case(case, g))


def test_comirecsa_w3_takes_no_gradient_and_is_unmoved_by_adam():
    g = load_golden("model_comirecsa_train.npz")
    model = build("comirecsa_train", int(g["seed"]))
    model(dict(g["batch"]))["loss"].backward()
    params = dict(model.named_parameters())
    assert params[W3].grad is None and all(p.grad is not None for k, p in params.items() if k != W3)
    assert W3 not in g["grad"] and torch.equal(g["adam2"][W3], g["init"][W3])
    _, _, adam2, _ = run_case("comirecsa_train", g)
    assert torch.equal(adam2[W3], g["init"][W3])
    assert tuple(params[W3].shape) == (D, D) and tuple(params["multi_interest_sa.W1"].shape) == (D, 4 * D)


def test_config_keys_and_defaults_are_the_references():
    from rec_pangu_amd.models.layers import MultiInterestSelfAttention, STAMPLayer
    from rec_pangu_amd.models.sequence import STAMP, ComirecSA
    m = STAMP(ENC, dict(CONFIG))
    assert m.feat_drop == 0 and m.stamp_layer.feat_drop is None
    m = STAMP(ENC, dict(CONFIG, feat_drop=0.3))
    assert m.stamp_layer.feat_drop.p == 0.3
    with pytest.raises(KeyError):
        ComirecSA(ENC, dict(CONFIG))
    m = ComirecSA(ENC, dict(CONFIG, K=3))
    assert (m.multi_interest_sa.d, m.multi_interest_sa.num_attention_heads, m.multi_interest_sa.embedding_dim) == (4 * D, 3, D)
    assert MultiInterestSelfAttention(8, 2, d=40).W1.shape == (8, 40)
    assert [k for k, _ in STAMPLayer(4).named_parameters()] == [k[len("stamp_layer."):] for k in STAMP_KEYS]


def test_the_models_and_the_layers_are_exported():
    import rec_pangu_amd.models.layers as layers
    from rec_pangu_amd.models import sequence
    from rec_pangu_amd.models.layers import multi_interest
    from rec_pangu_amd.models.layers import sequence as seq_layers
    from rec_pangu_amd.models.sequence import comirec, stamp
    assert sequence.STAMP is stamp.STAMP and sequence.ComirecSA is comirec.ComirecSA and sequence.ComirecDR is comirec.ComirecDR
    assert "STAMPLayer" in layers.__all__ and layers.STAMPLayer is seq_layers.STAMPLayer
    assert "MultiInterestSelfAttention" in layers.__all__
    assert layers.MultiInterestSelfAttention is multi_interest.MultiInterestSelfAttention


def test_the_fixture_batch_holds_its_edge_cases():
    b = load_golden("model_stamp.npz")["batch"]
    hist, lens = b["hist_item_list"], b["hist_mask_list"].sum(1)
    assert int(lens.min()) == 1 and int(lens.max()) == hist.shape[1] == L
    assert any(len(set(r[r > 0].tolist())) < int((r > 0).sum()) for r in hist)  # a repeated item
    assert {0, V - 1} <= set(b["target_item"].view(-1).tolist())
    for case in CASES:
        assert torch.equal(load_golden(f"model_{case}.npz")["batch"]["hist_item_list"], hist)


# ---- the pooling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
@pytest.mark.parametrize("with_c", [False, True])
@pytest.mark.parametrize("B,Lx,Dx,Dh,K", [(7, 1, 4, 4, 1), (8, 5, 12, 40, 3), (6, 20, 8, 32, 4)])
def test_the_cpu_pooling_is_the_float64_statement(mode, act, with_c, B, Lx, Dx, Dh, K):
    from rec_pangu_amd import functional as Fh
    norm = MODES[mode][1]
    gen = torch.Generator().manual_seed(B * 1000 + Lx * 10 + K)
    x, w1, w2, valid, c, g = pool_inputs(B, Lx, Dx, Dh, K, with_c, gen)

    def ours(x_, w1_, w2_, valid_, c_, act_, norm_):
        return Fh.attention_pool_reference(x_, w1_, w2_, valid_, c_, act_, norm_, return_weights=True)

    want = pool_grads(pool_f64, x, w1, w2, valid, c, g, act, norm, torch.float64)
    got = pool_grads(ours, x, w1, w2, valid, c, g, act, norm, torch.float32)
    for name, a, b in zip(("out", "A", "dx", "dc", "dw1", "dw2"), got, want):
        if b is not None:
            within(a, b, name)
    out, A, dx = got[0], got[1], got[2]
    masked = valid == 0
    if norm == "softmax" and B > 4:
        masked[4] = False  # (the row without a valid position pools uniformly: below)
    assert float(A[masked].abs().max() if masked.any() else 0.0) == 0.0
    if B > 4:  # row 4 has no valid position
        if norm == "mask":
            assert float(out[4].abs().max()) == 0.0 and float(dx[4].abs().max()) == 0.0
        else:
            torch.testing.assert_close(A[4], torch.full_like(A[4], 1.0 / Lx))
            torch.testing.assert_close(out[4], x[4].float().mean(0, keepdim=True).expand(K, -1))
    # the public entry point on CPU tensors is the same function
    o2 = Fh.attention_pool(x.float(), w1.float(), w2.float(), valid, None if c is None else c.float(), act=act, norm=norm)
    assert torch.equal(o2, out)


def test_a_hole_in_valid_has_weight_zero_and_takes_no_gradient():
    """a position with valid = 0 and a non-zero row: weight exactly 0, no gradient to that row, whatever the row holds"""
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(3)
    x, w1, w2, valid, c, g = pool_inputs(7, 5, 6, 8, 2, True, gen)
    for act, norm, with_c in MODES.values():
        xa = x.float().clone().requires_grad_(True)
        out = Fh.attention_pool(xa, w1.float(), w2.float(), valid, c.float() if with_c else None, act=act, norm=norm)
        (out * g.float()).sum().backward()
        xb = x.float().clone()
        xb[5, 1] = 100.0
        out_b = Fh.attention_pool(xb, w1.float(), w2.float(), valid, c.float() if with_c else None, act=act, norm=norm)
        assert torch.equal(out_b[5], out[5]) and float(xa.grad[5, 1].abs().max()) == 0.0


def test_the_layers_run_the_functional_form():
    from rec_pangu_amd.models.layers import MultiInterestSelfAttention, STAMPLayer
    torch.manual_seed(0)
    sa = MultiInterestSelfAttention(6, 3, d=10)
    x = torch.randn(4, 5, 6)
    mask = (torch.arange(5)[None, :] < torch.tensor([5, 2, 1, 3])[:, None]).float()
    got = sa(x, mask.unsqueeze(-1))
    want = pool_f64(x.double(), sa.W1.double(), sa.W2.double(), mask.double(), None, "tanh", "softmax")[0]
    within(got, want, "interests")
    assert torch.equal(sa(x, mask), got)
    within(sa(x), pool_f64(x.double(), sa.W1.double(), sa.W2.double(), torch.ones(4, 5, dtype=torch.float64), None, "tanh", "softmax")[0],
           "no mask")
    st = STAMPLayer(6).double()
    lens = torch.tensor([5, 2, 1, 3])
    xd = x.double()
    sr = st(xd, lens)
    for b in range(4):  # the reference's formulas, row by row
        n = int(lens[b])
        rows = xd[b, :n]
        ms, xt = rows.sum(0) / n, rows[n - 1]
        e = st.attn_e(torch.sigmoid(st.attn_i(rows) + st.attn_t(xt) + st.attn_s(ms))).squeeze(-1)
        torch.testing.assert_close(sr[b], st.fc_a((e.unsqueeze(-1) * rows).sum(0)) * st.fc_t(xt), rtol=1e-12, atol=1e-12)


def test_stamp_empty_row_is_defined_and_takes_no_encoder_gradient():
    """lens = 0: the reference gives NaN; here m_s = x_t = 0, user_emb = fc_a.bias * fc_t.bias, no gradient to the rows"""
    from rec_pangu_amd.models.sequence import STAMP
    torch.manual_seed(1)
    model = STAMP(ENC, dict(CONFIG))
    with torch.no_grad():
        model.stamp_layer.fc_a.bias.uniform_(0.5, 1.0)
        model.stamp_layer.fc_t.bias.uniform_(0.5, 1.0)
    hist = torch.tensor([[7, 3, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [9, 0, 0, 0, 0, 0]])
    data = {"hist_item_list": hist, "hist_mask_list": (hist > 0).long(), "target_item": torch.tensor([[1], [2], [3]])}
    res = model(data)
    assert torch.isfinite(res["user_emb"]).all() and torch.isfinite(res["loss"])
    torch.testing.assert_close(res["user_emb"][1], model.stamp_layer.fc_a.bias * model.stamp_layer.fc_t.bias)
    only = model({k: v[1:2] for k, v in data.items()})
    only["loss"].backward()
    g = model.item_emb.weight.grad  # the loss head reads every item row; the encoder adds nothing for this row
    assert float(model.stamp_layer.attn_i.weight.grad.abs().max()) == 0.0
    assert float(model.stamp_layer.attn_e.weight.grad.abs().max()) == 0.0
    assert torch.isfinite(g).all()
    keep = torch.tensor([0, 2])
    u_all = model(data, is_training=False)["user_emb"]
    u_sub = model({k: v[keep] for k, v in data.items()}, is_training=False)["user_emb"]
    torch.testing.assert_close(u_all[keep], u_sub, rtol=1e-6, atol=1e-7)
    one = {k: v[:1] for k, v in data.items()}  # a batch of one trains
    model.zero_grad()
    model(one)["loss"].backward()
    assert torch.isfinite(model.item_emb.weight.grad).all()


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["STAMP", "ComirecSA"])
def test_sequence_trainer_epoch(name, tmp_path):
    from rec_pangu_amd.models import sequence
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, _ = _tiny_loaders()
    torch.manual_seed(0)
    model = getattr(sequence, name)(enc, dict(cfg, K=2))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    trainer.fit(model, train, valid, epoch=1, lr=1e-2, device=torch.device("cpu"), topk_list=[5, 10])
    assert len(trainer.log_df) == 1
    assert all(torch.equal(before[k], v) == (k == W3) for k, v in model.state_dict().items())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rp_attn_pool_geometry", "rp_attn_pool_fits", "rp_attn_pool_workspace_bytes", "rp_attn_pool_fwd", "rp_attn_pool_bwd"]


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
    for fn in ("attn_pool_fwd", "attn_pool_bwd", "attn_pool_fits", "attn_pool_geometry"):
        assert callable(getattr(hip, fn))


def test_fits_and_geometry_agree():
    from rec_pangu_amd import hip
    geo = hip.attn_pool_geometry()
    assert geo["max_d"] >= 128 and geo["max_dh"] >= 512 and geo["max_k"] >= 8 and geo["max_l"] >= 64
    assert geo["lds_bytes"] <= 160 * 1024
    for shape in ((1, 1, 1, 1), (50, 128, 512, 8), (64, 128, 512, 8), (20, 64, 256, 4), (5, 12, 40, 3), (50, 64, 64, 1)):
        assert hip.attn_pool_fits(*shape), shape
    for shape in ((65, 64, 64, 1), (20, 129, 64, 1), (20, 132, 64, 1), (20, 64, 513, 1), (20, 64, 64, 9), (0, 8, 8, 1), (8, 0, 8, 1),
                  (8, 8, 0, 1), (8, 8, 8, 0)):
        assert not hip.attn_pool_fits(*shape), shape


def test_entry_points_reject_bad_arguments_without_a_launch():
    from rec_pangu_amd import hip
    lib = hip.lib()
    n0 = hip.launch_count()
    nbytes = ctypes.c_size_t(0)
    for Lx, Dx, Dh, K in ((6, 129, 8, 1), (6, 8, 8, 9), (65, 8, 8, 1), (6, 8, 513, 1)):
        assert lib.rp_attn_pool_workspace_bytes(4, Lx, Dx, Dh, K, 0, ctypes.byref(nbytes)) == ERR_ARG
    assert lib.rp_attn_pool_workspace_bytes(4, 6, 8, 8, 1, 0, None) == ERR_ARG
    assert lib.rp_attn_pool_workspace_bytes(4, 6, 8, 32, 4, 0, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    fwd = nbytes.value
    assert lib.rp_attn_pool_workspace_bytes(4, 6, 8, 32, 4, 1, ctypes.byref(nbytes)) == 0 and nbytes.value > fwd
    act, norm = hip.ACT_TANH, hip.ATTN_POOL_SOFTMAX
    ws = ctypes.create_string_buffer(nbytes.value + 16)
    for Lx, Dx, Dh, K in ((6, 129, 8, 1), (6, 8, 8, 9), (65, 8, 8, 1)):
        assert lib.rp_attn_pool_fwd(ws, ws, ws, ws, None, 4, Lx, Dx, Dh, K, act, norm, ws, ws, ws, nbytes.value, None) == ERR_ARG
        assert lib.rp_attn_pool_bwd(ws, ws, ws, ws, None, ws, ws, 4, Lx, Dx, Dh, K, act, norm, ws, ws, ws, None, ws, nbytes.value,
                                    None) == ERR_ARG
    assert lib.rp_attn_pool_fwd(None, None, None, None, None, 4, 6, 8, 32, 4, act, norm, None, None, None, 0, None) == ERR_ARG
    assert b"null pointer" in lib.rp_last_error()
    assert lib.rp_attn_pool_bwd(None, None, None, None, None, None, None, 4, 6, 8, 32, 4, act, norm, None, None, None, None, None, 0,
                                None) == ERR_ARG
    assert lib.rp_attn_pool_fwd(ws, ws, ws, ws, None, 4, 6, 8, 32, 4, hip.ACT_RELU, norm, ws, ws, ws, nbytes.value, None) == ERR_ARG
    assert lib.rp_attn_pool_fwd(ws, ws, ws, ws, None, 4, 6, 8, 32, 4, act, 7, ws, ws, ws, nbytes.value, None) == ERR_ARG
    assert lib.rp_attn_pool_geometry(None, None, None, None, None, None) == ERR_ARG
    assert hip.launch_count() == n0
