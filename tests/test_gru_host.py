"""GRU4Rec and NARM on the CPU (plumbing, no GPU): both models against the golden vectors produced by running the reference
(tests/golden/make_golden_gru.py), their state_dict / init stream, the edge cases the fixture batches hold, a batch of one,
one SequenceTrainer epoch each, and the declaration / binding / argument checks / sizing of the new C entry points.

Bars of the model comparisons are tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, the other tolerance 1e-6,
the tighter of the two readings per element (the generator chose its seeds against a tenth of that)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from test_sequence_host import _tiny_loaders, check_against_golden

torch.set_num_threads(1)

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
CASES = {
    "gru4rec": ("GRU4Rec", {}, True),
    "narm_train": ("NARM", {"hidden_size": 12, "dropout_probs": [0, 0]}, True),
    "narm_eval": ("NARM", {"hidden_size": 12}, False),
}
GRU_KEYS = [f"{n}_{s}_l{k}" for k in range(2) for n in ("weight", "bias") for s in ("ih", "hh")]  # nn.GRU's own order


def build(case, seed):
    from rec_pangu_amd.models import sequence
    cls, cfg, train = CASES[case]
    torch.manual_seed(seed)
    model = getattr(sequence, cls)(ENC, dict(CONFIG, **cfg))
    return model.train() if train else model.eval()


def run_case(case, g, device="cpu", make_opt=None):
    """(out, grads, adam2, adam2_out) of our model on `device`, as the generator runs the reference (shared with
    tests/test_hip_gru_models.py)"""
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
           else torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0))
    for _ in range(2):
        model({k: v.clone() for k, v in batch.items()})["loss"].backward()
        opt.step()
        model.zero_grad()
    adam2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        r = model({k: v.clone() for k, v in batch.items()}, is_training=False)
    return out, grads, adam2, {k: v.detach().cpu() for k, v in r.items()}


# ---- state and init ---------------------------------------------------------------------------------------------------------
def test_gru4rec_state_dict_and_init_stream():
    g = load_golden("model_gru4rec.npz")
    model = build("gru4rec", int(g["seed"]))
    sd = model.state_dict()
    assert list(sd) == list(g["init"]) == ["item_emb.weight"] + ["gru.rnn." + k for k in GRU_KEYS] + ["gru.out.weight"]
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k  # same draws from the same stream
    assert sd["gru.rnn.weight_ih_l0"].shape == (3 * D, D) and sd["gru.rnn.bias_hh_l1"].shape == (3 * D,)
    assert isinstance(model.gru.rnn, torch.nn.GRU) and model.gru.rnn.num_layers == 2 and model.gru.rnn.batch_first
    assert float(sd["item_emb.weight"][0].abs().max()) > 0  # reset_parameters leaves the padding row non-zero


@pytest.mark.parametrize("case", ["narm_train", "narm_eval"])
def test_narm_state_dict_and_init_stream(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case, int(g["seed"]))
    sd = model.state_dict()
    want = ["item_emb.weight"] + [f"gru.weight_{s}_l{k}" for k in range(2) for s in ("ih", "hh")] + \
           ["a_1.weight", "a_2.weight", "v_t.weight", "b.weight"]
    assert list(sd) == list(g["init"]) == want
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k
    assert sd["gru.weight_ih_l0"].shape == (36, D) and sd["gru.weight_ih_l1"].shape == (36, 12) and sd["b.weight"].shape == (D, 24)


def test_config_keys_and_defaults_are_the_references():
    from rec_pangu_amd.models.sequence import NARM
    m = NARM(ENC, dict(CONFIG))
    assert (m.n_layers, m.dropout_probs, m.hidden_size) == (2, [0.1, 0.1], 32)
    assert m.emb_dropout.p == 0.1 and m.ct_dropout.p == 0.1 and m.gru.hidden_size == 32 and not m.gru.bias
    m = NARM(ENC, dict(CONFIG, n_layers=1, dropout_probs=[0.3, 0.0], hidden_size=5))
    assert m.gru.num_layers == 1 and m.emb_dropout.p == 0.3 and m.a_1.weight.shape == (5, 5)


def test_the_models_are_exported_where_yotubednn_is():
    import rec_pangu_amd.models as models
    from rec_pangu_amd.models import layers, sequence
    assert sequence.__all__ == ["YotubeDNN", "GRU4Rec", "NARM"]
    assert models.sequence.GRU4Rec is sequence.GRU4Rec and "GRU4RecEncoder" in layers.__all__
    enc = layers.GRU4RecEncoder(6)
    assert enc.rnn.hidden_size == 128 and enc.rnn.num_layers == 2 and list(enc.state_dict())[-1] == "out.weight"


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_model_matches_the_reference_on_cpu(case):
    g = load_golden(f"model_{case}.npz")
    check_against_golden(g, *run_case(case, g))


@pytest.mark.parametrize("case", list(CASES))
def test_the_fixture_batches_hold_their_edge_cases(case):
    b = load_golden(f"model_{case}.npz")["batch"]
    hist, mask, tgt = b["hist_item_list"], b["hist_mask_list"], b["target_item"].view(-1)
    lens = mask.sum(1)
    assert hist.shape == (5, L) and torch.equal(mask, (torch.arange(L)[None] < lens[:, None]).long())  # right-padded
    assert 1 in lens.tolist() and L in lens.tolist() and any(1 < n < L for n in lens.tolist())  # length 1, full, padded tail
    assert int(lens.min()) >= 1  # no empty row: the reference raises there
    assert len(set(tgt.tolist())) < len(tgt) and 0 in tgt.tolist() and V - 1 in tgt.tolist()
    if case.startswith("narm"):
        pos = torch.arange(L)[None]
        assert bool(((hist == 0) & (pos < lens[:, None])).any())  # an id 0 in front of len
        assert bool(((hist != 0) & (pos >= lens[:, None])).any())  # a non-zero id behind it


@pytest.mark.parametrize("case", ["gru4rec", "narm_train"])
def test_a_batch_of_one_trains(case):
    model = build(case, 1)
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0]]),
            "target_item": torch.tensor([[5]])}
    res = model(data)
    assert res["user_emb"].shape == (1, D) and res["loss"].dim() == 0
    res["loss"].backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert float(model.item_emb.weight.grad.abs().max()) > 0


def test_a_row_without_history_fails_on_the_cpu_like_the_reference():
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0], [0] * 6]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0], [0] * 6]),
            "target_item": torch.tensor([[5], [6]])}
    with pytest.raises(RuntimeError):  # pack_padded_sequence: a length must be positive
        build("gru4rec", 1)(data)
    with pytest.raises(RuntimeError):  # gather with index -1
        build("narm_train", 1)(data)


def test_functional_cpu_paths_are_the_torch_formulas():
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(0)
    rnn = torch.nn.GRU(4, 5, 2, batch_first=True)
    E = torch.randn(9, 4, generator=gen)
    ids = torch.tensor([[1, 2, 3], [4, 0, 0], [5, 6, 0]])
    lens = torch.tensor([3, 1, 2])
    h_all, h_last = Fh.gru_encode(rnn, lens, lens - 1, ids=ids, item_weight=E, packed=True)
    want, _ = rnn(torch.nn.functional.embedding(ids, E))
    for b, n in enumerate(lens.tolist()):
        torch.testing.assert_close(h_all[b, :n], want[b, :n], rtol=1e-6, atol=1e-6)
        assert float(h_all[b, n:].detach().abs().sum()) == 0 and torch.equal(h_last[b], h_all[b, n - 1])
    full, hl = Fh.gru_encode(rnn, torch.full((3,), 3), torch.tensor([2, -1, 0]), x=E[ids], packed=False)
    assert torch.equal(full, want) and float(hl[1].detach().abs().sum()) == 0 and torch.equal(hl[2], want[2, 0])
    q1, q2, v = torch.randn(3, 3, 5, generator=gen), torch.randn(3, 5, generator=gen), torch.randn(1, 5, generator=gen)
    got = Fh.narm_attention(q1, q2, v, ids, want, hl)
    alpha = ((ids > 0)[..., None] * torch.sigmoid(q1 + q2[:, None])) @ v.view(-1, 1)
    assert torch.equal(got, torch.cat([(alpha * want).sum(1), hl], 1))


# ---- trainer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["GRU4Rec", "NARM"])
def test_sequence_trainer_epoch(name, tmp_path):
    from rec_pangu_amd.models import sequence
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, _ = _tiny_loaders()
    torch.manual_seed(0)
    model = getattr(sequence, name)(enc, cfg)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    trainer.fit(model, train, valid, epoch=1, lr=1e-2, device=torch.device("cpu"), topk_list=[5, 10])
    assert len(trainer.log_df) == 1 and all(not torch.equal(before[k], v) for k, v in model.state_dict().items())


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rp_gru_geometry", "rp_gru_workspace_bytes", "rp_gru_fwd", "rp_gru_bwd", "rp_hist_rows_fwd", "rp_hist_rows_bwd",
               "rp_narm_attn_workspace_bytes", "rp_narm_attn_fwd", "rp_narm_attn_bwd"]


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


def _wgrad_ws(M, N, K):
    from rec_pangu_amd import hip
    n = ctypes.c_size_t(0)
    assert hip.lib().rp_linear_wgrad_workspace_bytes(M, N, K, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("B,Ls,n_in,H,ids", [(1, 1, 1, 1, True), (33, 7, 6, 20, True), (300, 20, 64, 64, False),
                                             (4096, 50, 128, 100, True)])
def test_gru_workspace_is_the_documented_formula(B, Ls, n_in, H, ids):
    """A(12 Hp Kp) + A(12 Hp Hp) + 2 A(12 B L H) + A(4 H ceil(B / TB)) + (id mode: A(4 B L in)) + A(the larger
    of the two weight-gradient GEMMs' workspaces), A = round up to 256, Hp / Kp = H / in rounded up to 32"""
    from rec_pangu_amd import hip
    geo = hip.gru_geometry()
    assert geo == {"TB": 32, "max_h": 128}
    A = lambda x: -(-x // 256) * 256  # noqa: E731
    Hp, Kp = -(-H // 32) * 32, -(-n_in // 32) * 32
    want = A(12 * Hp * Kp) + A(12 * Hp * Hp) + 2 * A(12 * B * Ls * H) + A(4 * H * -(-B // geo["TB"])) + \
        (A(4 * B * Ls * n_in) if ids else 0) + A(max(_wgrad_ws(B * Ls, 3 * H, n_in), _wgrad_ws(B * Ls, 3 * H, H)))
    assert hip.gru_workspace_bytes(B, Ls, n_in, H, ids) == want


def test_entry_points_reject_bad_arguments_without_a_launch():
    from rec_pangu_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    n = ctypes.c_size_t(0)
    n0 = hip.launch_count()
    for n_in, H, Ls in [(8, 129, 4), (129, 8, 4), (0, 8, 4), (8, 0, 4), (8, 8, 0)]:
        assert lib.rp_gru_workspace_bytes(4, Ls, n_in, H, 1, ctypes.byref(n)) == -1, (n_in, H, Ls)
        assert lib.rp_gru_fwd(None, None, 0, p, 4, Ls, n_in, H, p, p, None, None, p, p, p, p, None, p, 1 << 30, None) == -1
        assert lib.rp_gru_bwd(None, None, 0, p, 4, Ls, n_in, H, p, p, None, None, p, p, p, p, p, p, p, p, None, None, p, 1 << 30,
                              None) == -1
    assert b"1 <= in, H <= 128" in lib.rp_last_error()
    assert lib.rp_gru_workspace_bytes(4, 4, 8, 8, 0, None) == -1
    assert lib.rp_gru_geometry(None, None) == -1
    # null pointers, both inputs / neither input, an undersized workspace
    assert lib.rp_gru_fwd(None, None, 0, p, 4, 4, 8, 8, None, p, None, None, p, p, p, p, None, p, 1 << 30, None) == -1
    assert lib.rp_gru_fwd(None, None, 0, None, 4, 4, 8, 8, p, p, None, None, p, p, p, p, None, p, 1 << 30, None) == -1
    assert lib.rp_gru_fwd(p, p, 9, p, 4, 4, 8, 8, p, p, None, None, p, p, p, p, p, p, 1 << 30, None) == -1
    assert lib.rp_gru_fwd(p, None, 9, None, 4, 4, 8, 8, p, p, None, None, p, p, p, p, p, p, 1 << 30, None) == -1
    assert lib.rp_gru_fwd(None, None, 0, p, 4, 4, 8, 8, p, p, None, None, p, p, p, p, None, p, 16, None) == -1
    assert lib.rp_gru_bwd(None, None, 0, p, 4, 4, 8, 8, p, p, None, None, p, p, None, p, p, p, p, p, None, None, p, 1 << 30,
                          None) == -1
    assert lib.rp_gru_bwd(None, None, 0, p, 4, 4, 8, 8, p, p, None, None, p, p, p, p, p, p, p, None, None, None, p, 1 << 30,
                          None) == -1  # dW_ih without dW_hh
    assert lib.rp_hist_rows_fwd(p, 3, 0, p, 4, p, p, None) == -1 and lib.rp_hist_rows_fwd(None, 3, 4, p, 4, p, p, None) == -1
    assert lib.rp_hist_rows_bwd(p, p, 4, 4, 3, p, 2, p, None) == -1
    assert lib.rp_narm_attn_fwd(p, p, p, p, p, p, 2, 3, 129, p, p, None) == -1
    assert lib.rp_narm_attn_fwd(p, p, p, p, p, None, 2, 3, 8, p, p, None) == -1
    assert lib.rp_narm_attn_bwd(p, p, p, p, p, p, p, 2, 0, 8, p, p, p, p, p, p, 1 << 20, None) == -1
    assert lib.rp_narm_attn_workspace_bytes(5, 0, ctypes.byref(n)) == -1
    assert lib.rp_narm_attn_workspace_bytes(5, 8, ctypes.byref(n)) == 0 and n.value == 4 * 8 * 2
    assert lib.rp_narm_attn_workspace_bytes(10 ** 6, 8, ctypes.byref(n)) == 0 and n.value == 4 * 8 * 1024  # bounded slabs
    assert hip.launch_count() == n0
    assert hip.gru_fits(1, 128) and not hip.gru_fits(129, 8) and not hip.gru_fits(8, 0)
