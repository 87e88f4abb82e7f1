"""AFN on the CPU (plumbing, no GPU): constructor signature, state_dict contract, init RNG stream and forward / backward /
running statistics / Adam numerics against the golden vectors produced by running the reference
(tests/golden/make_golden_afn.py), the trainer registry with one epoch of BenchmarkTrainer, the float64 restatement the GPU
kernel tests use against the model's own torch formulation, and the argument validation of the lognet entry points.

Train mode (batch statistics): log_batch_norm.bias has no real gradient — a shift of y_f scales c_l by a constant and
exp_batch_norm's batch statistics remove it — so the reference's own gradient there (1e-8 .. 4e-8) is fp32 rounding noise and
Adam turns it into steps of up to lr.  That gradient is judged against the bar of log_batch_norm.weight's gradient
(1e-4 max(1e-2, max |dgamma1|)); the parameter is left out of adam2/, and so are exp_batch_norm's running buffers there, which
the same shift scales (after1/ pins them before any Adam step); adam2_out/ is compared in the eval cases only."""
import ctypes
import inspect
import os

import pytest
import torch

from conftest import load_golden, small_enc_dict

torch.set_num_threads(1)

# per case, the first model seed from 1234 upward that tests/golden/make_golden_afn.py accepted (it prints them)
SEEDS = {"afn_eval": 1245, "afn_train": 1236, "afn_noens_eval": 1238}
CASES = {"afn_eval": (True, False), "afn_train": (True, True), "afn_noens_eval": (False, False)}  # ensemble_dnn, train mode
KW = dict(embedding_dim=8, dnn_hidden_units=[8, 4], afn_hidden_units=[8, 4], logarithmic_neurons=3)
BN1_BIAS = "log_batch_norm.bias"
TRAIN_SKIP = (BN1_BIAS, "exp_batch_norm.running_mean", "exp_batch_norm.running_var")  # of adam2/ in train mode


def build(name):
    from rec_pangu_amd.models.ranking import AFN
    ens, train_mode = CASES[name]
    torch.manual_seed(SEEDS[name])
    model = AFN(enc_dict=small_enc_dict(), ensemble_dnn=ens, **KW)
    if train_mode:
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    return model.train(train_mode)


def project_bar(ref):
    return 1e-4 * max(1e-2, float(ref.abs().max()))


def check_against_golden(name, g, out, grads, after1, adam2, adam2_out):
    """the comparisons of one case with the exemptions of the module docstring; shared with tests/test_hip_afn.py, which passes
    what the HIP path computed"""
    train_mode = CASES[name][1]
    for k, v in g["out"].items():
        torch.testing.assert_close(out[k], v, rtol=1e-5, atol=1e-6, msg=lambda m: f"{name}:{k}: {m}")
    assert set(g["grad"]) == set(grads)
    for k, v in g["grad"].items():
        if train_mode and k == BN1_BIAS:
            bar = project_bar(g["grad"]["log_batch_norm.weight"])
            err = float((grads[k] - v).abs().max())
            print(f"{name}: grad {k}: max err {err:.3g} against {bar:.3g}")
            assert err <= bar, (name, k, err, bar)
            continue
        torch.testing.assert_close(grads[k], v, rtol=1e-4, atol=1e-6, msg=lambda m: f"{name}:grad {k}: {m}")
    assert set(g["after1"]) == set(after1)
    for k, v in g["after1"].items():
        torch.testing.assert_close(after1[k], v, rtol=1e-4, atol=1e-6, msg=lambda m: f"{name}:after1 {k}: {m}")
    assert list(adam2) == list(g["adam2"])
    for k, v in g["adam2"].items():
        if train_mode and k in TRAIN_SKIP:
            continue
        torch.testing.assert_close(adam2[k], v, rtol=1e-4, atol=1e-6, msg=lambda m: f"{name}:adam2 {k}: {m}")
    if not train_mode:
        for k, v in g["adam2_out"].items():
            torch.testing.assert_close(adam2_out[k], v, rtol=1e-5, atol=1e-6, msg=lambda m: f"{name}:adam2_out {k}: {m}")


def run_case(name, g, device="cpu", make_opt=None):
    """(out, grads, after1, adam2, adam2_out) of our AFN on `device`, as make_golden.dump_model_case runs the reference"""
    batch = {k: v.to(device) for k, v in g["batch"].items()}
    train_mode = CASES[name][1]
    model = build(name).to(device)
    res = model({k: v.clone() for k, v in batch.items()})
    model.zero_grad()
    res["loss"].backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
    after1 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    model = build(name).to(device)
    opt = (make_opt(model) if make_opt is not None
           else torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0))
    for _ in range(2):
        r = model({k: v.clone() for k, v in batch.items()})
        r["loss"].backward()
        opt.step()
        model.zero_grad()
    adam2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model.eval()
    with torch.no_grad():
        r = model({k: v.clone() for k, v in batch.items()}, is_training=False)
    assert "loss" not in r
    model.train(train_mode)
    return out, grads, after1, adam2, {k: v.detach().cpu() for k, v in r.items()}


def test_constructor_signature_and_registry():
    """the signature as inspect.signature gives it for the reference's class (afn.py:15-22)"""
    from rec_pangu_amd.benchmark_trainer import MODEL_REGISTRY
    from rec_pangu_amd.models import ranking
    sig = {k: v.default for k, v in inspect.signature(ranking.AFN.__init__).parameters.items() if k != "self"}
    assert sig == dict(embedding_dim=32, dnn_hidden_units=[64, 64, 64], afn_hidden_units=[64, 64, 64], ensemble_dnn=True,
                       loss_fun='torch.nn.BCELoss()', logarithmic_neurons=5, enc_dict=None)
    assert list(sig) == ["embedding_dim", "dnn_hidden_units", "afn_hidden_units", "ensemble_dnn", "loss_fun",
                         "logarithmic_neurons", "enc_dict"]
    assert "AFN" in ranking.__all__ and MODEL_REGISTRY["AFN"] is ranking.AFN


@pytest.mark.parametrize("name", list(CASES))
def test_init_stream_and_state_dict_contract(name):
    g = load_golden(f"model_{name}.npz")
    model = build(name)
    sd = model.state_dict()
    assert list(sd.keys()) == list(g["init"].keys())
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
        assert torch.equal(sd[k], v), f"{name}: init of {k} differs from the reference's"
    tail = [k for k in sd if not k.startswith("embedding_layer.")]
    bn = lambda p: [f"{p}.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]  # noqa: E731
    head = (["coefficient_W.weight"] + [f"dense_layer.net.{i}.{s}" for i in (0, 3, 6) for s in ("weight", "bias")]
            + bn("log_batch_norm") + bn("exp_batch_norm"))
    assert tail[:len(head)] == head
    rest = tail[len(head):]
    if CASES[name][0]:
        emb2 = [k for k in rest if k.startswith("embedding_layer2.")]
        assert len(emb2) == 5 and rest == emb2 + [f"dnn.net.{i}.{s}" for i in (0, 3, 6) for s in ("weight", "bias")] + \
            ["fc.weight", "fc.bias"]
        assert sd["dnn.net.0.weight"].shape == (8, 5 * 8) and sd["fc.weight"].shape == (1, 2)
    else:
        assert rest == []
    assert sd["coefficient_W.weight"].shape == (3, 5) and sd["dense_layer.net.0.weight"].shape == (8, 3 * 8)
    assert sd["log_batch_norm.weight"].shape == (5,) and sd["exp_batch_norm.weight"].shape == (3,)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_running_statistics_adam_vs_reference(name):
    g = load_golden(f"model_{name}.npz")
    check_against_golden(name, g, *run_case(name, g))


def test_defaults_and_dropout_modules():
    from rec_pangu_amd.models.ranking import AFN
    model = AFN(enc_dict=small_enc_dict())
    assert model.coefficient_W.weight.shape == (5, 5) and model.coefficient_W.bias is None
    assert [type(m).__name__ for m in model.dense_layer.net] == ["Linear", "ReLU", "Dropout"] * 3 + ["Linear"]
    assert all(m.p == 0.1 for m in model.modules() if isinstance(m, torch.nn.Dropout))
    assert model.dense_layer.net[0].in_features == 32 * 5 and model.dnn.net[0].in_features == 32 * 5
    assert not hasattr(AFN(enc_dict=small_enc_dict(), ensemble_dnn=False), "fc")


def test_benchmark_trainer_runs_afn_for_one_epoch(tmp_path):
    """model_list=["AFN"] resolves through the registry (a NameError before) and trains on the sample loaders"""
    import pandas as pd
    from rec_pangu_amd.benchmark_trainer import BenchmarkTrainer
    from test_trainer_dataset import _loaders_in_reference_order
    _, train_loader, valid_loader, test_loader, enc, _ = _loaders_in_reference_order()
    csv = os.path.join(tmp_path, "bench.csv")
    torch.manual_seed(1)
    bt = BenchmarkTrainer(num_task=1, model_list=["AFN"], benchmark_res_path=csv, ckpt_root=os.path.join(tmp_path, "ck"))
    bt.run(train_loader, enc, valid_loader, test_loader, epoch=1, lr=1e-3, device=torch.device("cpu"))
    res = pd.read_csv(csv)
    assert list(res["model_name"]) == ["AFN"] and os.listdir(os.path.join(tmp_path, "ck")) == ["AFN"]
    assert {"roc_auc_score", "log_loss"} <= {c.replace("valid_", "").replace("test_", "") for c in res.columns}


@pytest.mark.parametrize("train", [True, False], ids=["batch", "running"])
def test_the_float64_restatement_of_the_gpu_tests_against_the_torch_formulation(train):
    """tests/test_hip_lognet.py's restatement and AFN.logarithmic_net (nn.BatchNorm1d, nn.Linear) agree in float64 to 1e-12,
    forward, every gradient and the running buffers, when both clamp at the same value: the model at the double 1e-5 here, the
    kernels (and the restatement in the GPU tests) at float32(1e-5) — no input sits between or within 1e-7 of them"""
    from rec_pangu_amd.models.ranking import AFN
    from test_hip_lognet import make_case, restate, THR
    B, F, D, L = 65, 5, 8, 3
    c = make_case(B, F, D, L, stride=F * D + 13, train=train)
    enc = {f"C{i}": {"vocab_size": 3} for i in range(F)}
    model = AFN(embedding_dim=D, dnn_hidden_units=[4], afn_hidden_units=[4], logarithmic_neurons=L, enc_dict=enc).double()
    model.train(train)
    with torch.no_grad():
        model.coefficient_W.weight.copy_(c["W"])
        for bn, (gm, be, rm, rv) in ((model.log_batch_norm, c["bn1"]), (model.exp_batch_norm, c["bn2"])):
            bn.weight.copy_(gm), bn.bias.copy_(be), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    E = c["x"][:, :F * D].double().view(B, F, D).requires_grad_(True)
    assert THR < 1e-5 and not bool(((E.detach().abs() - THR).abs() < 1e-7).any()) and bool((E.detach().abs() < THR).any())
    out = model.logarithmic_net(E)
    ref = restate(c, thr=1e-5)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)  # noqa: E731
    close(out.detach(), ref["out"])
    out.backward(c["cot"][:, :L * D].double())
    close(E.grad.reshape(B, F * D), ref["dx"])
    close(model.coefficient_W.weight.grad, ref["dW"])
    close(model.log_batch_norm.weight.grad, ref["dg1"]), close(model.log_batch_norm.bias.grad, ref["db1"])
    close(model.exp_batch_norm.weight.grad, ref["dg2"]), close(model.exp_batch_norm.bias.grad, ref["db2"])
    if train:
        close(model.log_batch_norm.running_mean, ref["run"][0]), close(model.log_batch_norm.running_var, ref["run"][1])
        close(model.exp_batch_norm.running_mean, ref["run"][2]), close(model.exp_batch_norm.running_var, ref["run"][3])


def test_lognet_argument_validation_needs_no_gpu():
    from rec_pangu_amd import hip
    lib = hip.lib()
    assert lib.rp_version() == hip.ABI_VERSION == 108  # (no existing prototype changed)
    for name in ("rp_lognet_fits", "rp_lognet_plan", "rp_lognet_workspace_bytes", "rp_lognet_fwd", "rp_lognet_bwd",
                 "rp_pair_fc_partials", "rp_pair_fc_fwd", "rp_pair_fc_bwd"):
        assert name in hip.EXPORTED_SYMBOLS
    assert hip.lognet_fits(26, 64, 5) and hip.lognet_fits(26, 32, 5) and hip.lognet_fits(39, 64, 8) and hip.lognet_fits(1, 4, 1)
    assert all(hip.lognet_fits(F, D, L) for F in (1, 26, 39, 64) for D in (1, 8, 40, 64, 256) for L in range(1, 9))
    assert not hip.lognet_fits(65, 8, 3) and not hip.lognet_fits(5, 8, 9) and not hip.lognet_fits(5, 257, 3)
    assert not hip.lognet_fits(0, 8, 3) and not hip.lognet_fits(5, 0, 3) and not hip.lognet_fits(5, 8, 0)
    # the plan: at most 512 partial workgroups, whole rounds of 2048 (sample, column) pairs
    assert hip.lognet_plan(1, 4) == (1, 2048) and hip.lognet_plan(512, 64) == (16, 2048) and hip.lognet_plan(513, 64) == (17, 2048)
    assert hip.lognet_plan(65536, 32) == (512, 4096) and hip.lognet_plan(65537, 32)[0] <= 512
    # the workspace takes the geometry and no batch size
    n = ctypes.c_size_t(0)
    assert len(lib.rp_lognet_workspace_bytes.argtypes) == 3
    assert lib.rp_lognet_workspace_bytes(26, 5, ctypes.byref(n)) == 0 and n.value == (512 * 26 * 7 + 26 * 7 + 10) * 4 + 256
    assert lib.rp_lognet_workspace_bytes(26, 5, None) == -1
    # the wrappers' checks come before anything touches a device
    B, F, D, L = 4, 3, 8, 2
    x, W = torch.zeros(B, F * D + 2), torch.zeros(L, F)
    v1, v2 = [torch.zeros(F) for _ in range(4)], [torch.zeros(L) for _ in range(4)]
    out = torch.zeros(B, 64)
    fwd = lambda x=x, W=W, v1=v1, v2=v2, out=out, D=D: hip.lognet_fwd(  # noqa: E731
        x, F, D, W, *v1, 1e-5, *v2, 1e-5, True, out)
    with pytest.raises(RuntimeError, match="float32"):
        fwd(x=x.double())
    with pytest.raises(RuntimeError, match=r"contiguous \[L, F\]"):
        fwd(W=torch.zeros(L, F + 1))
    with pytest.raises(RuntimeError, match="narrower"):
        fwd(x=x[:, :F * D - 1])
    with pytest.raises(RuntimeError, match="BatchNorm vector"):
        fwd(v1=[torch.zeros(F + 1)] + v1[1:])
    with pytest.raises(RuntimeError, match="narrower"):
        fwd(out=torch.zeros(B, L * D - 1))
    with pytest.raises(RuntimeError, match="rp_lognet_fits"):
        hip.lognet_fwd(x, F, D, torch.zeros(9, F), *v1, 1e-5, *[torch.zeros(9) for _ in range(4)], 1e-5, True, torch.zeros(B, 128))
    with pytest.raises(RuntimeError, match="HIP-device"):  # every host-side check passed: only now the device matters
        fwd()
    # the C entry points: null pointers, a row stride smaller than the row, a small workspace, a shape outside the range
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cf = lambda ldx, ldo, ws, F_=F, x_=p: lib.rp_lognet_fwd(  # noqa: E731
        x_, ldx, p, p, p, p, p, 1e-5, p, p, p, p, 1e-5, p, p, ldo, B, F_, D, L, 1, p, ws, None)
    assert cf(F * D, L * D, 1 << 30, x_=None) == -1 and b"null" in lib.rp_last_error()
    assert cf(F * D - 1, L * D, 1 << 30) == -1 and b"stride" in lib.rp_last_error()
    assert cf(F * D, L * D - 1, 1 << 30) == -1 and b"stride" in lib.rp_last_error()
    assert cf(F * D, L * D, 16) == -1 and b"workspace" in lib.rp_last_error()
    assert cf(65 * D, L * D, 1 << 30, F_=65) == -3 and b"rp_lognet_fits" in lib.rp_last_error()
    cb = lambda lddo, lddx, ws, L_=L, dx=p: lib.rp_lognet_bwd(  # noqa: E731
        p, lddo, p, F * D, p, p, p, p, p, p, 1e-5, p, p, p, 1e-5, dx, lddx, p, p, p, p, p, B, F, D, L_, 1, p, ws, None)
    assert cb(L * D, F * D, 1 << 30, dx=None) == -1 and b"null" in lib.rp_last_error()
    assert cb(L * D - 1, F * D, 1 << 30) == -1 and b"stride" in lib.rp_last_error()
    assert cb(L * D, F * D - 1, 1 << 30) == -1 and b"stride" in lib.rp_last_error()
    assert cb(L * D, F * D, 16) == -1 and b"workspace" in lib.rp_last_error()
    assert cb(9 * D, F * D, 1 << 30, L_=9) == -3
    assert lib.rp_pair_fc_fwd(None, p, p, p, p, 4, None) == -1 and lib.rp_pair_fc_bwd(p, p, p, p, p, p, p, p, None, 4, None) == -1
    assert lib.rp_pair_fc_partials(1) == 3 and lib.rp_pair_fc_partials(1 << 20) == 3 * 512
