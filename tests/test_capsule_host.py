"""MIND and ComirecDR on the CPU (plumbing, no GPU): both models against the golden vectors produced by running the reference
(tests/golden/make_golden_capsule.py), their state_dict / init stream / draw stream, a batch of one, CapsuleNetwork in all
three bilinear types with relu_layer and stop_grad against a float64 restatement written here, the ValueError for a history
of the wrong length, one SequenceTrainer epoch each (its validation goes through evaluate_recall's multi-interest branch),
and the declaration / binding / argument checks / sizing of the new C entry points.

Bars of the model comparisons are tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, the other tolerance 1e-6,
the tighter of the two readings per element (the generator chose its seeds against a tenth of that).  The layer against
float64: the project's 1e-4 max(1e-2, max |ref|) per tensor."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from test_sequence_host import _tiny_loaders, check_against_golden

torch.set_num_threads(1)

V, D, L, K = 37, 8, 6, 3
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": [], "K": K}
CASES = {"mind_train": ("MIND", True), "mind_eval": ("MIND", False), "comirecdr": ("ComirecDR", True)}
KEYS = {"MIND": ["item_emb.weight", "capsule.relu.0.weight", "capsule.linear.weight"],
        "ComirecDR": ["item_emb.weight", "capsule.w", "capsule.relu.0.weight"]}


def build(case, seed):
    from rec_pangu_amd.models import sequence
    cls, train = CASES[case]
    torch.manual_seed(seed)
    model = getattr(sequence, cls)(ENC, dict(CONFIG))
    return model.train() if train else model.eval()


def feed_logits(model, logits, device):
    """initial_logits replaced by the recorded draws, one per forward, in order"""
    queue = [t.to(device) for t in logits]
    model.capsule.initial_logits = lambda batch, dev: queue.pop(0)
    return queue


def run_case(case, g, device="cpu", make_opt=None, feed=False):
    """(out, grads, adam2, adam2_out) of our model on `device`, as the generator runs the reference (shared with
    tests/test_hip_capsule_models.py).  feed: MIND's initial logits come from the fixture instead of the generator — what the
    device needs, where torch.randn draws another stream."""
    seed = int(g["seed"])
    batch = {k: v.to(device) for k, v in g["batch"].items()}
    feed = feed and "logits" in g
    model = build(case, seed).to(device)
    if feed:
        feed_logits(model, [g["logits"]["out"]], device)
    res = model({k: v.clone() for k, v in batch.items()})
    model.zero_grad()
    res["loss"].backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
    model = build(case, seed).to(device)
    if feed:
        left = feed_logits(model, [g["logits"][k] for k in ("adam2_0", "adam2_1", "adam2_out")], device)
    opt = (make_opt(model) if make_opt is not None
           else torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0))
    for _ in range(2):
        model({k: v.clone() for k, v in batch.items()})["loss"].backward()
        opt.step()
        model.zero_grad()
    adam2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        r = model({k: v.clone() for k, v in batch.items()}, is_training=False)
    assert not feed or left == []
    return out, grads, adam2, {k: v.detach().cpu() for k, v in r.items()}


# ---- state and init ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_state_dict_and_init_stream(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case, int(g["seed"]))
    sd = model.state_dict()
    assert list(sd) == list(g["init"]) == KEYS[CASES[case][0]]
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k  # same draws from the same stream
    assert sd["capsule.relu.0.weight"].shape == (D, D)  # exists although relu_layer is off
    if CASES[case][0] == "MIND":
        assert sd["capsule.linear.weight"].shape == (D, D) and model.capsule.bilinear_type == 0
    else:
        assert sd["capsule.w"].shape == (1, L, K * D, D) and model.capsule.bilinear_type == 2
    c = model.capsule
    assert (c.hidden_size, c.seq_len, c.interest_num, c.routing_times, c.hard_readout, c.relu_layer, c.stop_grad) == \
        (D, L, K, 3, True, False, False)


def test_k_is_required_and_the_models_are_exported():
    from rec_pangu_amd.models import layers, sequence
    from rec_pangu_amd.models.sequence import MIND, ComirecDR
    assert sequence.MIND is MIND and sequence.ComirecDR is ComirecDR and "CapsuleNetwork" in layers.__all__
    cfg = {k: v for k, v in CONFIG.items() if k != "K"}
    for cls in (MIND, ComirecDR):
        with pytest.raises(KeyError):
            cls(ENC, cfg)
    assert layers.CapsuleNetwork(4, 5).bilinear_type == 2 and layers.CapsuleNetwork(4, 5).interest_num == 4  # the defaults
    assert list(layers.CapsuleNetwork(4, 5, bilinear_type=1, interest_num=3).state_dict()) == ["relu.0.weight", "linear.weight"]
    assert layers.CapsuleNetwork(4, 5, bilinear_type=1, interest_num=3).linear.weight.shape == (12, 4)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_model_matches_the_reference_on_cpu(case):
    """MIND draws its own logits here: the CPU generator's stream is the reference's"""
    g = load_golden(f"model_{case}.npz")
    check_against_golden(g, *run_case(case, g))


@pytest.mark.parametrize("case", ["mind_train", "mind_eval"])
def test_mind_draws_the_recorded_logits_in_the_references_order(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case, int(g["seed"]))
    assert set(g["logits"]) == {"out", "adam2_0", "adam2_1", "adam2_out"} and g["logits"]["out"].shape == (5, K, L)
    assert torch.equal(g["logits"]["out"], g["logits"]["adam2_0"])  # (the generator re-seeds in front of the Adam steps)
    assert torch.equal(model.capsule.initial_logits(5, "cpu"), g["logits"]["out"])
    model = build(case, int(g["seed"]))
    batch = {k: v.clone() for k, v in g["batch"].items()}
    model(batch)  # the training forward also draws the reference's torch.rand(B, D) placeholder behind the logits ...
    assert torch.equal(model.capsule.initial_logits(5, "cpu"), g["logits"]["adam2_1"])  # ... so the next forward's match
    check_against_golden(g, *run_case(case, g, feed=True))


@pytest.mark.parametrize("case", list(CASES))
def test_the_fixture_batches_hold_their_edge_cases(case):
    b = load_golden(f"model_{case}.npz")["batch"]
    hist, mask, tgt = b["hist_item_list"], b["hist_mask_list"], b["target_item"].view(-1)
    lens = mask.sum(1)
    assert hist.shape == (5, L) and torch.equal(mask, (torch.arange(L)[None] < lens[:, None]).long())  # right-padded
    assert 1 in lens.tolist() and L in lens.tolist() and any(1 < n < L for n in lens.tolist())  # length 1, full, padded tail
    assert int(lens.min()) >= 1  # no fully masked row: every interest would be zero, the readout an exact tie
    assert bool(((hist == 0) & (mask == 1) & (lens[:, None] == L)).any())  # an id 0 inside a full row
    assert len(set(tgt.tolist())) < len(tgt) and 0 in tgt.tolist() and V - 1 in tgt.tolist()


@pytest.mark.parametrize("case", ["mind_train", "comirecdr"])
def test_a_batch_of_one_trains(case):
    model = build(case, 1)
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0]]),
            "target_item": torch.tensor([[5]])}
    res = model(data)
    assert res["user_emb"].shape == (1, K, D) and res["loss"].dim() == 0
    res["loss"].backward()
    for k, p in model.named_parameters():
        if k != "capsule.relu.0.weight":
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert model(data, is_training=False)["user_emb"].shape == (1, K, D)


@pytest.mark.parametrize("case", ["mind_train", "comirecdr"])
def test_a_history_of_the_wrong_length_raises(case):
    model = build(case, 1)
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0]]),
            "target_item": torch.tensor([[5]])}
    with pytest.raises(ValueError, match="max_length"):
        model(data)
    with pytest.raises(ValueError, match="seq_len"):
        model.capsule(torch.zeros(1, L + 1, D), torch.ones(1, L + 1), "cpu")


# ---- the layer against float64 ------------------------------------------------------------------------------------------------
def route64(U, m, b0, stop_grad=False):
    """three routing rounds in float64, written from the formulas: U [B, K, L, D], m [B, L], b0 [B, K, L] -> [B, K, D]"""
    Ui = U.detach() if stop_grad else U
    b, v = b0, None
    for i in range(3):
        c = torch.softmax(b, dim=-1) * (m != 0)[:, None, :]  # softmax over all L positions, masked, not renormalised
        src = Ui if i < 2 else U
        s = torch.einsum("bkl,bkld->bkd", c, src)
        n = (s * s).sum(-1, keepdim=True)
        v = s * n / (1 + n) / torch.sqrt(n + 1e-9)
        if i < 2:
            b = b + torch.einsum("bkld,bkd->bkl", src, v)
    return v


def capsule64(params, btype, Kk, x, m, b0, relu_layer=False, stop_grad=False):
    """CapsuleNetwork in float64 from a {name: float64 tensor} parameter dict"""
    B, Ls, Dd = x.shape
    if btype == 0:
        U = (x @ params["linear.weight"].t())[:, None].expand(B, Kk, Ls, Dd)
    elif btype == 1:
        U = (x @ params["linear.weight"].t()).view(B, Ls, Kk, Dd).permute(0, 2, 1, 3)
    else:
        U = torch.einsum("lnd,bld->bln", params["w"][0], x).view(B, Ls, Kk, Dd).permute(0, 2, 1, 3)
    if b0 is None:
        b0 = torch.zeros(B, Kk, Ls, dtype=torch.float64, device=x.device)
    out = route64(U, m, b0, stop_grad)
    return torch.relu(out @ params["relu.0.weight"].t()) if relu_layer else out


def bar(ref):
    return 1e-4 * max(1e-2, float(ref.detach().abs().max()))


def within(got, ref, what, frac=1.0):
    err = float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max())
    print(f"{what}: max err {err:.3g} against bar {frac * bar(ref):.3g}")
    assert got.shape == ref.shape and err <= frac * bar(ref), (what, err, frac * bar(ref))


def layer_case(btype, relu_layer, stop_grad, device="cpu", B=7, Ls=5, Dd=6, Kk=3, seed=0):
    """a CapsuleNetwork on `device` and its float64 restatement on the same inputs -> [(what, got, ref)] for the output, the
    input's gradient and every used parameter's gradient"""
    from rec_pangu_amd.models.layers import CapsuleNetwork
    torch.manual_seed(seed)
    layer = CapsuleNetwork(Dd, Ls, bilinear_type=btype, interest_num=Kk, relu_layer=relu_layer)
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.5)
    layer.stop_grad = stop_grad
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, Ls, Dd, generator=gen)
    lens = torch.randint(1, Ls + 1, (B,), generator=gen)
    lens[0], lens[1] = Ls, 1
    mask = (torch.arange(Ls)[None] < lens[:, None]).long()
    b0 = torch.randn(B, Kk, Ls, generator=gen)
    g = torch.randn(B, Kk, Dd, generator=gen)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    ref = capsule64(p64, btype, Kk, x64, mask, b0.double() if btype == 0 else None, relu_layer, stop_grad)
    (ref * g.double()).sum().backward()
    layer = layer.to(device)
    layer.initial_logits = lambda batch, dev: b0.to(device)
    xd = x.to(device).requires_grad_(True)
    got = layer(xd, mask.to(device), device)
    (got * g.to(device)).sum().backward()
    out = [("out", got, ref), ("d item_eb", xd.grad, x64.grad)]
    for k, p in layer.named_parameters():
        if p64[k].grad is None:
            assert p.grad is None, k
        else:
            out.append((f"d {k}", p.grad, p64[k].grad))
    return out


@pytest.mark.parametrize("btype,relu_layer,stop_grad", [(0, False, False), (1, False, False), (2, False, False),
                                                        (0, True, False), (2, True, True), (1, False, True)])
def test_capsule_network_against_float64(btype, relu_layer, stop_grad):
    tag = f"type {btype}{' relu' if relu_layer else ''}{' stop_grad' if stop_grad else ''}"
    for what, got, ref in layer_case(btype, relu_layer, stop_grad):
        within(got, ref, f"{tag}: {what}")


def test_functional_cpu_paths_are_the_references_formulas():
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(0)
    x, w = torch.randn(3, 4, 5, generator=gen), torch.randn(1, 4, 10, 5, generator=gen)
    assert torch.equal(Fh.capsule_project(x, w), torch.sum(w[:, :4] * x.unsqueeze(2), dim=3))
    assert torch.equal(Fh.capsule_project(x, w[0]), Fh.capsule_project(x, w))
    inter, E = torch.randn(3, 4, 5, generator=gen, requires_grad=True), torch.randn(9, 5, generator=gen)
    inter.data[1, 2] = inter.data[1, 0]  # two identical interests: the lower index is picked
    t = torch.tensor([0, 8, 3])
    best = Fh.interest_pick(inter, E, t)
    kk = torch.argmax(torch.bmm(inter, E[t].unsqueeze(-1)), dim=1).view(-1)
    assert torch.equal(best, inter[torch.arange(3), kk])
    best.sum().backward()
    want = torch.zeros(3, 4, 5)
    want[torch.arange(3), kk] = 1
    assert torch.equal(inter.grad, want)
    m = torch.tensor([[1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]])
    u = torch.randn(3, 4, 10, generator=gen)
    out = Fh.capsule_route(u, m, 2)
    assert out.shape == (3, 2, 5) and float(out[1].abs().max()) == 0.0  # a fully masked row: exact zeros
    ref = route64(u.double().view(3, 4, 2, 5).permute(0, 2, 1, 3), m, torch.zeros(3, 2, 4, dtype=torch.float64))
    within(out, ref, "capsule_route on the CPU")
    with pytest.raises(ValueError):
        Fh.capsule_route(u, m, 2, rounds=0)


# ---- trainer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["MIND", "ComirecDR"])
def test_sequence_trainer_epoch(name, tmp_path):
    """the validation behind the epoch goes through get_recall_predict / evaluate_recall with a [B, K, D] user_emb"""
    from rec_pangu_amd.models import sequence
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, test = _tiny_loaders()
    torch.manual_seed(0)
    model = getattr(sequence, name)(enc, dict(cfg, K=2))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    trainer.fit(model, train, valid, epoch=1, lr=1e-2, device=torch.device("cpu"), topk_list=[5, 10])
    assert len(trainer.log_df) == 1
    assert all(not torch.equal(before[k], v) for k, v in model.state_dict().items() if k != "capsule.relu.0.weight")
    row = trainer.log_df.iloc[0]
    assert all(math.isfinite(float(row[k])) and 0.0 <= float(row[k]) <= 1.0 for k in ("recall@10", "ndcg@10", "hitrate@10"))
    batch = next(iter(test))
    assert model(batch, is_training=False)["user_emb"].dim() == 3
    metric = trainer.evaluate_model(model, test, torch.device("cpu"), topk_list=[5])
    assert all(math.isfinite(v) for k, v in metric.items() if k != "phase")


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rp_capsule_geometry", "rp_capsule_workspace_bytes", "rp_capsule_project_fwd", "rp_capsule_project_bwd_x", "rp_capsule_project_bwd_w",
               "rp_capsule_route_fwd", "rp_capsule_route_bwd", "rp_interest_pick_fwd", "rp_interest_pick_bwd"]


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
    assert [s for s in hip.EXPORTED_SYMBOLS if "capsule" in s and "workspace" in s] == ["rp_capsule_workspace_bytes"]  # one query


@pytest.mark.parametrize("B,Ls,N,Dd", [(1, 1, 8, 6), (512, 3, 40, 64), (513, 3, 40, 64), (1025, 2, 40, 16), (4096, 50, 256, 64),
                                       (16385, 20, 128, 32), (65536, 20, 128, 32)])
def test_workspace_is_the_documented_formula(B, Ls, N, Dd):
    """only dW takes a workspace — the partial sums of its batch splits.  S = min(32, max(1, ceil(B / 512)))
    splits of R = 64 ceil(ceil(B / S) / 64) rows, so ceil(B / R) of them; 4 ceil(B / R) L N D bytes, 0 when one split covers
    the batch"""
    from rec_pangu_amd import hip
    S = min(32, max(1, -(-B // 512)))
    R = 64 * -(-(-(-B // S)) // 64)
    n = -(-B // R)
    assert n <= 32 and (n - 1) * R < B <= n * R
    assert hip.capsule_workspace_bytes(B, Ls, N, Dd) == (4 * n * Ls * N * Dd if n > 1 else 0)
    assert (n > 1) == (B > 512)


def test_geometry_covers_the_sizes_the_models_are_used_at():
    from rec_pangu_amd import hip
    g = hip.capsule_geometry()
    assert g == {"proj_tb": 64, "proj_tn": 128, "max_k": 8, "max_l": 64, "max_d": 128, "lds_bytes": 144 * 1024}
    assert hip.capsule_route_fits(8, 64, 64) and hip.capsule_route_fits(4, 50, 128) and hip.capsule_route_fits(1, 1, 1)
    assert not hip.capsule_route_fits(9, 4, 8) and not hip.capsule_route_fits(4, 65, 8) and not hip.capsule_route_fits(4, 8, 129)
    assert not hip.capsule_route_fits(8, 64, 128) and not hip.capsule_route_fits(0, 4, 8)  # (the tiles would not fit the LDS)
    assert hip.capsule_project_fits(50, 2048, 128) and not hip.capsule_project_fits(50, 2049, 64)
    assert not hip.capsule_project_fits(50, 256, 129) and not hip.capsule_project_fits(0, 256, 64)


def test_entry_points_reject_bad_arguments_without_a_launch():
    from rec_pangu_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    n = ctypes.c_size_t(0)
    n0 = hip.launch_count()
    # (B, L, N, D): D = 129, D = 0, K D = 0 (K = 0), K D = 2049, L = 0
    for Ls, N, Dd in [(4, 258, 129), (4, 8, 0), (4, 0, 8), (4, 2049, 8), (0, 8, 8)]:
        assert lib.rp_capsule_project_fwd(p, p, 4, Ls, N, Dd, p, None) == -1, (Ls, N, Dd)
        assert lib.rp_capsule_project_bwd_x(p, p, 4, Ls, N, Dd, p, None) == -1, (Ls, N, Dd)
        assert lib.rp_capsule_project_bwd_w(p, p, 4, Ls, N, Dd, p, p, 1 << 30, None) == -1, (Ls, N, Dd)
        assert lib.rp_capsule_workspace_bytes(4, Ls, N, Dd, ctypes.byref(n)) == -1, (Ls, N, Dd)
    assert b"1 <= D <= 128" in lib.rp_last_error()
    for args in [(None, p, p), (p, None, p), (p, p, None)]:
        assert lib.rp_capsule_project_fwd(args[0], args[1], 4, 4, 8, 8, args[2], None) == -1
        assert lib.rp_capsule_project_bwd_x(args[0], args[1], 4, 4, 8, 8, args[2], None) == -1
        assert lib.rp_capsule_project_bwd_w(args[0], args[1], 4, 4, 8, 8, args[2], None, 0, None) == -1
    assert b"null" in lib.rp_last_error()
    assert lib.rp_capsule_workspace_bytes(4, 4, 8, 8, None) == -1
    assert lib.rp_capsule_project_bwd_w(p, p, 1025, 4, 8, 8, p, None, 0, None) == -1  # three splits and no workspace
    assert lib.rp_capsule_project_bwd_w(p, p, 1025, 4, 8, 8, p, p, 4 * 3 * 4 * 8 * 8 - 1, None) == -1 and b"workspace" in lib.rp_last_error()
    # routing (K, L, D): D = 129, K = 0, L = 0, K = 9, L = 65, tiles above the LDS budget
    for Kk, Ls, Dd in [(2, 4, 129), (0, 4, 8), (2, 0, 8), (9, 4, 8), (2, 65, 8), (8, 64, 128)]:
        assert lib.rp_capsule_route_fwd(p, Ls * Kk * Dd, Dd, Kk * Dd, p, None, 4, Kk, Ls, Dd, p, None) == -1, (Kk, Ls, Dd)
        assert lib.rp_capsule_route_bwd(p, Ls * Kk * Dd, Dd, Kk * Dd, p, None, p, 4, Kk, Ls, Dd, 0, p, None) == -1, (Kk, Ls, Dd)
    assert b"1 <= K <= 8" in lib.rp_last_error()
    assert lib.rp_capsule_route_fwd(None, 64, 8, 16, p, None, 4, 2, 4, 8, p, None) == -1
    assert lib.rp_capsule_route_fwd(p, 64, 8, 16, None, None, 4, 2, 4, 8, p, None) == -1
    assert lib.rp_capsule_route_fwd(p, 64, 8, 16, p, None, 4, 2, 4, 8, None, None) == -1
    assert lib.rp_capsule_route_fwd(p, 64, 4, 16, p, None, 4, 2, 4, 8, p, None) == -1  # interests overlap: 0 < sk < D
    assert lib.rp_capsule_route_bwd(p, 64, 8, 16, p, None, None, 4, 2, 4, 8, 0, p, None) == -1
    assert lib.rp_capsule_route_bwd(p, 64, 8, 16, p, None, p, 4, 2, 4, 8, 0, None, None) == -1
    assert lib.rp_interest_pick_fwd(p, p, 9, p, 4, 0, 8, p, p, p, None) == -1 and lib.rp_interest_pick_fwd(p, p, 9, p, 4, 2, 0, p, p, p, None) == -1
    assert lib.rp_interest_pick_fwd(p, p, 9, p, 4, 2, 8, p, p, None, None) == -1  # the flag is not optional
    assert lib.rp_interest_pick_fwd(None, p, 9, p, 4, 2, 8, p, p, p, None) == -1
    assert lib.rp_interest_pick_bwd(p, None, 4, 2, 8, p, None) == -1 and lib.rp_interest_pick_bwd(p, p, 4, 0, 8, p, None) == -1
    assert lib.rp_capsule_geometry(None, None, None, None, None, None) == -1
    assert hip.launch_count() == n0
