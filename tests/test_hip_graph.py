"""The captured training step (rec_pangu_amd/graph_step.py: forward + backward + FusedAdam step + zero_grad captured once,
device-resident step counters, static double-buffered inputs, next batch's sort inside the capture) against the eager loop
on the same batches: every prediction, loss, weight and optimizer moment bit-identical — replayed as a LAUNCH PLAN
(csrc/plan.hip; the sort on the plan's side stream) and as a hipGraph."""
import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


@pytest.fixture(params=["plan", "hipgraph"])
def backend(request, monkeypatch):
    monkeypatch.setenv("RP_GRAPH_BACKEND", request.param)
    return request.param


def _enc(n_dense, vocabs):
    enc = {f"I{i}": {"min": 0.0, "max": 1.0} for i in range(n_dense)}
    enc.update({f"C{i}": {"vocab_size": v} for i, v in enumerate(vocabs)})
    return enc


def _batches(enc, B, n, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        b = {k: (torch.rand(B, generator=gen) if "min" in v else torch.randint(0, v["vocab_size"] + 1, (B,), generator=gen))
             for k, v in enc.items()}
        b["label"] = (torch.rand(B, generator=gen) < 0.3).float()
        b["task1_label"] = (torch.rand(B, generator=gen) < 0.3).float()
        b["task2_label"] = (torch.rand(B, generator=gen) < 0.1).float()
        out.append({k: v.to(DEV) for k, v in b.items()})
    return out


def _build(kind, enc):
    from rec_pangu_amd.models.ranking import DCN, DeepFM
    torch.manual_seed(0)
    if kind == "deepfm64":   # D = 64, [64, 64, 64]: the fused gather + Linear forward and the fused gather backward
        model = DeepFM(embedding_dim=64, hidden_units=[64, 64, 64], enc_dict=enc)
    elif kind == "deepfm32tail":  # the fused MLP tail behind a GENERIC first layer: nobody joins the tail's deferred second
        model = DeepFM(embedding_dim=32, hidden_units=[64, 64, 64], enc_dict=enc)  # stage but the step itself
    elif kind == "xdeepfm_dropout":  # the reference's default: dropout 0.1 inside the MLP — ACTIVE in the captured step
        from rec_pangu_amd.models.ranking import xDeepFM
        model = xDeepFM(embedding_dim=16, dnn_hidden_units=[32, 16], cin_layer_units=[8, 8], enc_dict=enc)
    elif kind == "xdeepfm64":  # BASELINE config 3's structure (CIN [128, 128] at D = 64: pair-form first layer + collapsed last
        from rec_pangu_amd.models.ranking import xDeepFM  # layer) — round 6: library launches only, replays as a launch plan
        model = xDeepFM(embedding_dim=64, dnn_hidden_units=[64, 64, 64], cin_layer_units=[128, 128], enc_dict=enc)
    elif kind == "mmoe":  # the reference's defaults: BatchNorm1d + Dropout(0.2) towers, two tasks (round 5: a launch plan)
        from rec_pangu_amd.models.multi_task import MMOE
        model = MMOE(enc_dict=enc, embedding_dim=16, device=None)
    elif kind == "autoint":  # the fields as tokens beside the MLP (Fh.token_view), dropout 0.1, the LR layer's own tables
        from rec_pangu_amd.models.ranking import AutoInt
        model = AutoInt(embedding_dim=16, dnn_hidden_units=[32, 16], attention_layers=1, num_heads=2, attention_dim=4, enc_dict=enc)
    elif kind == "deepfm16":
        model = DeepFM(embedding_dim=16, hidden_units=[32, 16], enc_dict=enc)
    else:
        model = DCN(embedding_dim=16, hidden_units=[32, 16], enc_dict=enc)
    model = model.to(DEV)
    for m in model.modules():
        if hasattr(m, "check_indices"):
            m.check_indices = "deferred"
    return model


def _eager_and_graphed(kind, enc, batches, steps, replay, defer, backend, after_call=None):
    """`steps` training steps on `batches`, once as the eager loop and once through a GraphedTrainStep (the learning rate is
    halved at steps 40 and 200) -> ({mode: (sampled predictions, losses, state dict, optimizer state, step counters)}, the
    GraphedTrainStep).  after_call(i, gstep): called behind the graphed run's call i."""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.optim import FusedAdam, LazyAdamRows, StepTables
    results = {}
    chunk, LazyAdamRows.TABLE_CHUNK = LazyAdamRows.TABLE_CHUNK, 100
    min_cap, StepTables.MIN_CAPACITY = StepTables.MIN_CAPACITY, 0  # (small tables: capacity doublings re-capture on the way)
    try:
        for mode in ("eager", "graph"):
            model = _build(kind, enc)
            opt = FusedAdam(model.parameters(), lr=1e-3, fuse_zero_grad=True, lazy_tables=True, replay=replay, defer=defer)
            gstep = GraphedTrainStep(model, opt) if mode == "graph" else None
            preds, losses = [], []
            for i in range(steps):
                if i in (40, 200):
                    for grp in opt.param_groups:
                        grp["lr"] *= 0.5
                if gstep is not None:
                    out = gstep(batches[i], batches[i + 1])
                    if after_call is not None:
                        after_call(i, gstep)
                else:
                    model.prefetch(batches[i + 1])
                    out = model(batches[i])
                    out["loss"].backward()
                    opt.step()
                    model.zero_grad()
                if i % 7 == 0 or i > steps - 4:
                    preds.append(out["pred" if "pred" in out else "task1_pred"].detach().clone())
                    losses.append(out["loss"].detach().clone())
            if gstep is not None:
                assert gstep.replays == steps - 2, "every step after the two eager ones must have been a graph replay"
                assert gstep.graphs[0] is not None and gstep.graphs[1] is not None
                if kind == "xdeepfm_dropout":
                    assert max(gstep._drop_calls) >= 1, "no dropout launch was captured: the model ran without active dropout"
                elif backend == "plan":
                    # DeepFM's step is library launches only: it must replay as a plan, the sort in the side section — and
                    # so are MMOE's and AutoInt's (BatchNorm statistics, loss sum, weight packing, token view: library
                    # launches) and DCN's since round 5 (the CrossNet's weight-space arithmetic is rp_crossnet_param_grads, its layer
                    # stack rp_multi_copy, the padding columns of dX_0 are written by the rows kernel)
                    assert gstep.backend_used == "plan" and gstep.plans[0].side >= 4, (gstep.backend_used, gstep.why_not_plan)
                else:
                    assert gstep.backend_used == "hipgraph"
            lz = model.embedding_layer._lazy
            assert lz.t == steps
            if mode == "graph":
                assert int(lz.tabs.t_dev.item()) == steps, "device and host step counters must agree"
            model.embedding_layer.raise_if_bad_index()
            sd = {k: v.clone() for k, v in model.state_dict().items()}  # (flushes the lazy rows: host counters must be right)
            osd = opt.state_dict()
            results[mode] = (preds, losses, sd, [{k: v.clone() for k, v in st.items() if torch.is_tensor(v)} for st in osd["state"].values()],
                             [g["_rp_step"] for g in osd["param_groups"]])
    finally:
        LazyAdamRows.TABLE_CHUNK = chunk
        StepTables.MIN_CAPACITY = min_cap
        from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
        EmbeddingLayer.unpin_sorts()
    return results, gstep


def _assert_bit_identical(e, g):
    for a, b in zip(e[0], g[0]):
        assert torch.equal(a, b), "predictions differ"
    for a, b in zip(e[1], g[1]):
        assert torch.equal(a, b), "losses differ"
    for k in e[2]:
        assert torch.equal(e[2][k], g[2][k]), k
    for sa, sb in zip(e[3], g[3]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), f"optimizer state {k}"
    assert e[4] == g[4]


@pytest.mark.parametrize("kind,replay,steps,defer", [("deepfm64", "closed", 330, False), ("deepfm64", "exact", 60, False),
                                                     ("deepfm16", "closed", 300, False), ("dcn", "closed", 60, False),
                                                     ("deepfm32tail", "closed", 40, True), ("xdeepfm_dropout", "closed", 40, True),
                                                     ("deepfm64", "closed", 300, True), ("mmoe", "closed", 40, True),
                                                     ("autoint", "closed", 40, True), ("xdeepfm64", "closed", 40, True)])
def test_graphed_step_is_bit_identical_to_the_eager_loop(kind, replay, steps, defer, backend):
    """(330 / 300 steps cross step 256, where the closed-form replay takes over, and — with TABLE_CHUNK = 100 — several
    in-place extensions of the step tables; the learning rate changes twice on the way)"""
    from rec_pangu_amd import hip
    enc = _enc(5, [3000, 17, 900, 4, 20000, 250])
    batches = _batches(enc, 384, steps + 1, seed=4)
    results, _ = _eager_and_graphed(kind, enc, batches, steps, replay, defer, backend)
    _assert_bit_identical(results["eager"], results["graph"])
    assert hip.launch_count() > 0


def test_a_recorded_first_layer_backward_holds_every_block_it_allocates(monkeypatch):
    """The plan's inline section runs BESIDE the launches recorded behind it, so no two tensors hip allocates between the
    backward's fork and its join may share memory: every allocation of the first capture made inside the backward's
    hip.holding() block is logged (address, bytes) and the blocks must be pairwise disjoint — a dropped temporary whose
    block the capture's allocator handed to the next launch would show here, where comparing results usually does not.
    The smallest shape with all three backward forms and both side sections: tables of [600, 5, 300, 3, 7, 1000] rows at
    B = 512 (tiny 1, 3, 4; big 0, 5; mid 2; RP_SMP_MIN_BATCH = 1: conftest).  Then twenty replays against the eager loop."""
    from rec_pangu_amd import hip
    monkeypatch.setenv("RP_GRAPH_BACKEND", "plan")
    enc = _enc(5, [r - 1 for r in (600, 5, 300, 3, 7, 1000)])
    steps = 3 + 20  # two eager calls, the call that captures, twenty more
    batches = _batches(enc, 512, steps + 1, seed=11)
    new, log = hip._new, []

    def logged(shape, dtype, device):
        t = new(shape, dtype, device)
        log.append((t.data_ptr(), t.numel() * t.element_size(), hip.holding.active()))
        return t

    def after_call(i, gstep):
        if i == 2:  # the first capture is done: later captures share its pool and may reuse what it dropped at its end
            assert gstep.replays == 1 and gstep.backend_used == "plan", (gstep.backend_used, gstep.why_not_plan)
            monkeypatch.setattr(hip, "_new", new)

    monkeypatch.setattr(hip, "_new", logged)
    results, gstep = _eager_and_graphed("deepfm64", enc, batches, steps, "closed", True, "plan", after_call)
    assert hip._new is new and gstep.backend_used == "plan" and gstep.plans[0].inline >= 1
    held = sorted((p, n) for p, n, active in log if active and n > 0)
    print(f"{len(log)} allocations logged, {len(held)} non-empty ones inside the holding block: {sorted(n for _, n in held)} bytes")
    # at least the workspaces of linear_wgrad, embed_grad_tiny, embed_grad_smp and embed_grad_ss
    assert len(held) >= 4
    for (p0, n0), (p1, _) in zip(held, held[1:]):
        assert p0 + n0 <= p1, f"two blocks held at once overlap: {p0:#x}+{n0} and {p1:#x}"
    _assert_bit_identical(results["eager"], results["graph"])


RECORDED_PLAN_SHAPE = [(36, 13, 11, 1), (36, 13, 11, 1)]  # (nodes, side, inline, streams) per static batch
RECORDED_LAUNCHES = [  # (kernel, section: 0 main stream, 1 side — the next batch's sort —, 2 inline side)
    ("lazy_cf_table_kernel", 0), ("void lazy_adam_catchup_wave_kernel", 0), ("transpose_kernel", 0),
    ("void embed_gather_linear_kernel", 0), ("void mlp_tail_fwd_kernel", 0), ("void mlp_tail_bwd_kernel", 0),
    ("void embed_grad_smp_kernel", 0), ("embed_grad_tiny_partial_kernel", 2), ("embed_grad_tiny_finish_kernel", 2),
    ("embed_grad_tiny_dw_kernel", 2), ("void embed_segsum_kernel", 0), ("void embed_ss_urows_kernel", 0),
    ("embed_ss_dw_kernel", 0), ("embed_grad_smp_dw_kernel", 2), ("void embed_grad_reduce_kernel", 2),
    ("void embed_grad_reduce_kernel", 2), ("void embed_grad_fix_kernel", 2), ("void linear_wgrad_bf16_kernel", 2),
    ("wgrad_reduce_kernel", 2), ("loss_finish_kernel", 2), ("mlp_tail_reduce_kernel", 2), ("void adam_kernel", 0),
    ("counters_add_kernel", 0), ("embed_keys_kernel", 1), ("sort_seg_hist_kernel", 1), ("sort_seg_scan_kernel", 1),
    ("sort_seg_scatter_kernel", 1), ("sort_seg_hist_kernel", 1), ("sort_seg_scan_kernel", 1),
    ("sort_seg_scatter_kernel", 1), ("embed_grad_smp_count_kernel", 1), ("embed_grad_smp_scan_kernel", 1),
    ("embed_grad_smp_mark_kernel", 1), ("embed_ss_count_kernel", 1), ("embed_ss_scan_kernel", 1),
    ("embed_ss_mark_kernel", 1)]


def test_the_recorded_step_keeps_its_launch_sequence():
    """What a capture records is pinned as literals: (nodes, side, inline, streams) of both static batches' plans and the
    (kernel, section) sequence of the recorded launches — DeepFM D = 64, [64, 64, 64] on _enc(5, [3000, 17, 900, 4, 20000,
    250]) at B = 384, two eager calls and two captured ones (RP_SMP_MIN_BATCH = 1: conftest).  The literals were recorded by
    running these very lines on the parent commit of the change that split GraphedTrainStep's capture into pieces."""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    from rec_pangu_amd.optim import FusedAdam
    enc = _enc(5, [3000, 17, 900, 4, 20000, 250])
    batches = _batches(enc, 384, 5, seed=4)
    try:
        model = _build("deepfm64", enc)
        opt = FusedAdam(model.parameters(), lr=1e-3, fuse_zero_grad=True, lazy_tables=True, replay="closed", defer=True)
        gstep = GraphedTrainStep(model, opt, backend="plan")
        for i in range(4):
            gstep(batches[i], batches[i + 1])
        torch.cuda.synchronize()
        assert gstep.backend_used == "plan", (gstep.backend_used, gstep.why_not_plan)
        shape = [(pl.nodes, pl.side, pl.inline, pl.streams) for pl in gstep.plans]
        launches = [(name.split("<")[0].split("(")[0], section) for name, section in gstep.launch_names()]
        print("plan shapes:", shape)
        print("launches:", launches)
        assert shape == RECORDED_PLAN_SHAPE
        assert launches == RECORDED_LAUNCHES
    finally:
        EmbeddingLayer.unpin_sorts()


def test_graphed_step_falls_back_to_eager_for_the_unannounced_and_the_last_batch(backend):
    """a batch that was not announced by the previous call is staged and sorted on the spot; a call without a next batch
    (end of an epoch) runs eagerly; the run continues on the graphs afterwards — all bit-identical to the eager loop"""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.optim import FusedAdam
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    enc = _enc(3, [500, 9, 4000])
    batches = _batches(enc, 256, 24, seed=9)
    order = [(i, i + 1) for i in range(8)] + [(8, None)] + [(12, 13), (13, 14), (20, 21), (14, 15), (15, None)]
    finals = {}
    try:
        for mode in ("eager", "graph"):
            model = _build("deepfm16", enc)
            opt = FusedAdam(model.parameters(), lr=2e-3, fuse_zero_grad=True, lazy_tables=True, replay="closed")
            gstep = GraphedTrainStep(model, opt) if mode == "graph" else None
            for cur, nxt in order:
                nb = batches[nxt] if nxt is not None else None
                if gstep is not None:
                    gstep(batches[cur], nb)
                else:
                    if nb is not None:
                        model.prefetch(nb)
                    model(batches[cur])["loss"].backward()
                    opt.step()
                    model.zero_grad()
            finals[mode] = {k: v.clone() for k, v in model.state_dict().items()}
            if gstep is not None:
                assert gstep.replays == len(order) - 2 - 2
    finally:
        EmbeddingLayer.unpin_sorts()
    for k in finals["eager"]:
        assert torch.equal(finals["eager"][k], finals["graph"][k]), k


def test_graphed_step_with_a_loader_that_refills_its_buffers_in_place():
    """a launch plan reads the caller's tensors when the replay RUNS, and the sort of a batch is made one call
    earlier from the same tensors.  A loader that recycles device buffers — here: the announced buffer is refilled in place
    with another batch between the call that announces it and the call that consumes it, every other step — must not make
    ids and sort disagree: the step sees the changed version counter and stages + re-sorts that batch.  Also: every input of
    the captured step has an argument site, and no recorded argument points inside an input."""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.optim import FusedAdam
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    enc = _enc(3, [500, 9, 4000])
    content = _batches(enc, 256, 16, seed=31)
    decoys = _batches(enc, 256, 16, seed=32)
    finals = {}
    try:
        for mode in ("eager", "graph"):
            model = _build("deepfm16", enc)
            opt = FusedAdam(model.parameters(), lr=2e-3, fuse_zero_grad=True, lazy_tables=True, replay="closed")
            if mode == "eager":
                for b in content[:-1]:
                    model(b)["loss"].backward()
                    opt.step()
                    model.zero_grad()
            else:
                gstep = GraphedTrainStep(model, opt, backend="plan")
                bufs = [{k: v.clone() for k, v in content[0].items()}, {k: torch.empty_like(v) for k, v in content[0].items()}]
                restaged = 0
                for i in range(len(content) - 1):
                    cur, nxt = bufs[i % 2], bufs[(i + 1) % 2]
                    late = i % 2 == 1
                    for k in nxt:  # the loader fills the buffer it announces ...
                        nxt[k].copy_((decoys if late else content)[i + 1][k])
                    before = gstep._staged_sig
                    gstep(cur, nxt)
                    if late:       # ... and, every other step, changes its mind afterwards: the same buffer, refilled in place
                        for k in nxt:
                            nxt[k].copy_(content[i + 1][k])
                        restaged += 1
                assert gstep.replays >= len(content) - 1 - 2 - 2 and restaged >= 6
                assert gstep.backend_used == "plan" and gstep.bind_report["interior"] == 0
                used = [k for k in gstep.bind_report["sites"]  # the step reads everything of its batch, the ids of the next one
                        if (k.startswith("cur:") and (k[4:] in enc or k == "cur:label")) or (k.startswith("next:C"))]
                assert used and all(gstep.bind_report["sites"][k] > 0 for k in used), gstep.bind_report
            finals[mode] = {k: v.clone() for k, v in model.state_dict().items()}
    finally:
        EmbeddingLayer.unpin_sorts()
    for k in finals["eager"]:
        assert torch.equal(finals["eager"][k], finals["graph"][k]), k


@pytest.mark.parametrize("kind", ["deepfm64", "deepfm16", "dcn"])
def test_replayed_step_with_everything_that_can_come_between_two_steps(kind, monkeypatch):
    """A replayed step (launch plan, deferred lazy table optimizer) next to everything a training loop does between two
    steps must leave the run bit-identical to the eager loop: an unannounced batch (staged and sorted on the spot), the last
    batch of an epoch (no next batch: an eager step), an evaluation forward of other rows, a state_dict() (flushes the lazy
    state), a change of the learning rate."""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.optim import FusedAdam
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    monkeypatch.setenv("RP_GRAPH_BACKEND", "plan")
    enc = _enc(3, [500, 9, 4000, 30, 12000])
    batches = _batches(enc, 320, 40, seed=11)
    # (current, announced next, what happens AFTER the step)
    order = [(i, i + 1, None) for i in range(6)] + [(6, 7, "eval"), (7, 8, None), (8, 9, "state_dict"), (9, 10, None),
             (10, 30, None),        # announces 30 ...
             (11, 12, None),        # ... but 11 arrives: it is staged and sorted on the spot
             (12, 13, "lr"), (13, 14, None), (14, None, None),  # end of an epoch
             (20, 21, None), (21, 22, "eval"), (22, 23, None), (23, 24, None)]
    finals, preds = {}, {}
    try:
        for mode in ("eager", "graph"):
            model = _build(kind, enc)
            opt = FusedAdam(model.parameters(), lr=2e-3, fuse_zero_grad=True, lazy_tables=True, replay="closed", defer=True)
            gstep = GraphedTrainStep(model, opt) if mode == "graph" else None
            seen = []
            for cur, nxt, after in order:
                nb = batches[nxt] if nxt is not None else None
                if gstep is not None:
                    out = gstep(batches[cur], nb)
                else:
                    if nb is not None:
                        model.prefetch(nb)
                    out = model(batches[cur])
                    out["loss"].backward()
                    opt.step()
                    model.zero_grad()
                seen.append(out["loss"].detach().clone())
                if after == "eval":
                    model.eval()
                    with torch.no_grad():
                        seen.append(model(batches[35])["pred"].detach().clone())
                    model.train()
                elif after == "state_dict":
                    seen.append(torch.cat([v.detach().reshape(-1).float()[:64] for v in model.state_dict().values()]))
                elif after == "lr":
                    for grp in opt.param_groups:
                        grp["lr"] *= 0.5
            finals[mode] = {k: v.clone() for k, v in model.state_dict().items()}
            preds[mode] = seen
            if gstep is not None:
                assert gstep.backend_used == "plan", (gstep.backend_used, gstep.why_not_plan)
                assert gstep.replays >= len(order) - 2 - 3
    finally:
        EmbeddingLayer.unpin_sorts()
    for i, (a, b) in enumerate(zip(preds["eager"], preds["graph"])):
        assert torch.equal(a, b), f"observation {i} differs"
    for k in finals["eager"]:
        assert torch.equal(finals["eager"][k], finals["graph"][k]), k


def test_graphed_step_above_a_million_pairs(backend):
    """1.2 M (sample, field) pairs per batch: the size at which rocPRIM's onesweep sort faulted under unsynchronised
    replays (GraphedTrainStep.MAX_PAIRS_ROCPRIM).  The own radix sort has no memset nodes: 60 replays without a
    synchronisation in between end in the same bits as the eager loop."""
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.optim import FusedAdam
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    from rec_pangu_amd.models.ranking import DeepFM
    enc = _enc(2, [3000000, 70000])
    batches = _batches(enc, 600000, 4, seed=4)
    finals = {}
    try:
        for mode in ("eager", "graph"):
            torch.manual_seed(0)
            model = DeepFM(embedding_dim=8, hidden_units=[16], enc_dict=enc).to(DEV)
            for m in model.modules():
                if hasattr(m, "check_indices"):
                    m.check_indices = "deferred"
            opt = FusedAdam(model.parameters(), lr=2e-3, fuse_zero_grad=True, lazy_tables=True, replay="closed")
            gstep = GraphedTrainStep(model, opt) if mode == "graph" else None
            for i in range(64):
                cur, nb = batches[i % 4], batches[(i + 1) % 4]
                if gstep is not None:
                    gstep(cur, nb)
                else:
                    model.prefetch(nb)
                    model(cur)["loss"].backward()
                    opt.step()
                    model.zero_grad()
            model.embedding_layer.raise_if_bad_index()
            finals[mode] = {k: v.clone() for k, v in model.state_dict().items()}
            if gstep is not None:
                assert gstep.replays >= 60
                del gstep
    finally:
        EmbeddingLayer.unpin_sorts()
    for k in finals["eager"]:
        assert torch.equal(finals["eager"][k], finals["graph"][k]), k


def test_graphed_step_refuses_what_it_cannot_capture():
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.ranking import DeepFM
    from rec_pangu_amd.optim import FusedAdam
    enc = _enc(2, [50, 7])
    torch.manual_seed(0)
    model = DeepFM(embedding_dim=8, hidden_units=[8], enc_dict=enc).to(DEV)  # check_indices is still "sync"
    opt = FusedAdam(model.parameters(), lr=1e-3, fuse_zero_grad=True, lazy_tables=True)
    with pytest.raises(RuntimeError, match="deferred"):
        GraphedTrainStep(model, opt)
    with pytest.raises(RuntimeError, match="FusedAdam"):
        GraphedTrainStep(model, torch.optim.Adam(model.parameters()))
    for m in model.modules():
        if hasattr(m, "check_indices"):
            m.check_indices = "deferred"
    # active dropout: the mask's (seed, offset) are launch arguments and would be frozen at capture
    from rec_pangu_amd import hip
    real = torch.cuda.is_current_stream_capturing
    torch.cuda.is_current_stream_capturing = lambda: True
    try:
        with pytest.raises(RuntimeError, match="dropout"):
            hip._dropout_seed_offset(torch.device(DEV))
    finally:
        torch.cuda.is_current_stream_capturing = real


# (force_a2a, ahead) -> (LaunchPlan.seg_tags, which host calls are the replay's own): recorded on the parent commit of the
# change that split GraphedTrainStep's capture into pieces
RECORDED_SEGMENTS = {(False, True): ([0, 1, 0, 0], [False, False, True]),
                     (True, True): ([0, 1, 1, 0, 0, 0, 0], [False, True, False, True, True, True]),
                     (True, False): ([0, 0, 0, 0, 0], [True, True, True, True])}


@pytest.mark.parametrize("force_a2a,ahead", [(False, True), (True, True), (True, False)])
def test_graphed_step_with_row_sharded_tables_single_rank(force_a2a, ahead, backend, monkeypatch):
    """The captured step WITH its collectives: a DeepFM whose tables are row-sharded under a 1-rank RCCL group — route,
    exchange (the identity, or RCCL self-copies with RP_FORCE_A2A=1), owner-side gather / reduce, dense all-reduce, deferred
    lazy Adam with device-resident counters — against the eager loop on the same batches: every prediction and the final
    weights bit-identical.  Replayed as a hipGraph (round 4: all_to_all_single as graph nodes) and, round 6, as a LAUNCH PLAN
    in segments: the plan is cut at every collective (rp_plan_host_mark) and the replay issues them itself in between —
    which needs the whole sharded step to consist of library launches (no ATen fill / cast / cat / scale left in it).  The
    plan's segments and the replay's own calls between them equal RECORDED_SEGMENTS."""
    import copy
    import socket
    import torch.distributed as dist
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.ranking import DeepFM
    from rec_pangu_amd.optim import make_adam
    from rec_pangu_amd.sharded import ShardedEmbeddingLayer, allreduce_dense_grads, shard_model_tables
    if force_a2a:
        monkeypatch.setenv("RP_FORCE_A2A", "1")
    if not ahead:  # (rounds 4-5: the route of a batch is built inside its own step — the path a step takes when the
        monkeypatch.setenv("RP_SHARD_AHEAD", "0")  # fixed-capacity buffers cannot be made)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0)
    try:
        enc = _enc(3, [3000, 17, 900, 20000, 6])
        batches = _batches(enc, 512, 41, seed=8)
        torch.manual_seed(0)
        base = DeepFM(embedding_dim=64, hidden_units=[64, 64, 64], enc_dict=enc).to(DEV)
        results = {}
        for mode in ("eager", "graph"):
            model = shard_model_tables(copy.deepcopy(base), 1, 0)
            assert isinstance(model.embedding_layer, ShardedEmbeddingLayer)
            for m in model.modules():
                if hasattr(m, "check_indices"):
                    m.check_indices = "deferred"
            opt = make_adam(model, 1e-3)
            gstep = GraphedTrainStep(model, opt, post_backward=lambda: allreduce_dense_grads(model)) if mode == "graph" else None
            preds = []
            for i in range(40):
                if gstep is not None:
                    out = gstep(batches[i], batches[i + 1])
                else:
                    model.prefetch(batches[i + 1])
                    out = model(batches[i])
                    out["loss"].backward()
                    allreduce_dense_grads(model)
                    opt.step()
                    model.zero_grad()
                preds.append(out["pred"].detach().clone())
            model.embedding_layer.raise_if_bad_index()
            if gstep is not None:
                assert gstep.replays >= 36 and gstep.backend_used == backend, (gstep.replays, gstep.backend_used, gstep.why_not_plan)
                if backend == "plan":
                    # the three exchanges (ids, rows, row gradients) and the dense all-reduce are the replay's own calls
                    pl = gstep.plans[0]
                    assert sum(1 for fn in pl.host_calls if fn is not None) == (4 if force_a2a else 1), pl.host_calls
                    # (round 6) the next batch's route, id exchange and owner-side sort are segments of the ahead stream
                    if ahead:
                        assert sum(pl.seg_tags) == (2 if force_a2a else 1) and pl.ahead_stream is not None, pl.seg_tags
                    else:
                        assert sum(pl.seg_tags) == 0 and pl.ahead_stream is None, pl.seg_tags
                    print("segments:", (force_a2a, ahead), pl.seg_tags, [fn is not None for fn in pl.host_calls])
                    assert (pl.seg_tags, [fn is not None for fn in pl.host_calls]) == RECORDED_SEGMENTS[force_a2a, ahead]
            results[mode] = (preds, {k: v.clone() for k, v in model.state_dict().items()})
            del gstep
        for a, b in zip(results["eager"][0], results["graph"][0]):
            assert torch.equal(a, b), "predictions differ"
        for k in results["eager"][1]:
            assert torch.equal(results["eager"][1][k], results["graph"][1][k]), k
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


def _defined_marks(smp, ss, B, n_smp, n_kept):
    """what the mark launches define of their buffers: the duplicate marks and list entirely, the block offsets up to their
    total, and of each kept field's unique-row list as many entries as the field has unique rows (the rest is never read)"""
    nbk = -(-B // 256)
    offs = ss[2][:n_kept * nbk + 1].tolist()
    out = [smp[0], smp[1], smp[2][:n_smp * nbk + 1], ss[2][:n_kept * nbk + 1]]
    for r in range(n_kept):
        u = offs[(r + 1) * nbk] - offs[r * nbk]
        assert 0 < u <= B
        out += [ss[0][r * B:r * B + u], ss[1][r * B:r * B + u]]
    return out


def test_marks_of_a_pinned_sort_stay_where_a_recorded_step_expects_them():
    """The duplicate marks / unique-row lists of a PINNED sort are read by recorded launches at fixed addresses: they must live
    exactly as long as the pinned sort, however many other marked sorts come and go (a cache of its own used to
    evict them at eight entries), and a re-sort in place must re-make them in the same buffers."""
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    B, vocabs = 512, [5000, 300, 3000, 40, 5, 2000]  # three big tables (rows >= B), one mid-size (the streaming form), two tiny
    enc = _enc(0, vocabs)
    torch.manual_seed(0)
    layer = EmbeddingLayer(enc_dict=enc, embedding_dim=64).to(DEV)
    layer.check_indices = "deferred"
    layer._marks_wanted = True  # (what the first three-form backward sets)
    smp = layer._smp_tables(B)
    assert [t[0] for t in smp] == [0, 2, 5] and [t[0] for t in layer._tiny_tables()] == [3, 4]
    skip = sum(1 << f for f in (0, 2, 3, 4, 5))

    def ids(seed):
        gen = torch.Generator().manual_seed(seed)
        return {f"C{i}": torch.randint(0, v + 1, (B,), generator=gen).to(DEV) for i, v in enumerate(vocabs)}

    def ptrs(look):
        return [t.data_ptr() for t in look.smp + look.ss[1]]

    keep = []
    try:
        X0 = ids(100)
        layer.pin_sort(X0)
        first = layer.pinned_sort(X0)
        assert first.pinned and first.smp_sig == (B, tuple(smp)) and first.ss[0] == skip
        before = ptrs(first)
        for i in range(8):  # eight more static batches ...
            X = ids(200 + i)
            layer.pin_sort(X)
            keep.append((X, layer.pinned_sort(X)))
            assert keep[-1][1] is not first and keep[-1][1].smp is not None
        for i in range(9):  # ... and marked eager sorts, all kept alive
            X = ids(300 + i)
            look = layer._sorted_keys(layer._idx_list(X), layer.row_base, layer.row_count, tuple(X[c] for c in layer.emb_feature))
            assert not look.pinned and look.smp is not None and look.ss is not None
            keep.append((X, look))
        assert len({p for _, look in keep for p in ptrs(look)} | set(before)) == 6 * (1 + len(keep))
        new = ids(101)
        for k in X0:  # the static batch is refilled in place and re-sorted in place
            X0[k].copy_(new[k])
        layer.pin_sort(X0)
        assert layer.pinned_sort(X0) is first
        assert ptrs(first) == before
        want_sk, want_sp = hip.sort_pairs(hip.embed_keys(layer.row_base, layer.row_count, layer._idx_list(new), layer.err_flag),
                                          end_bit=layer._meta()[3])
        assert torch.equal(first.sk, want_sk) and torch.equal(first.sp, want_sp)
        fresh = _defined_marks(hip.embed_grad_smp_mark(first.sk, first.sp, B, [t[0] for t in smp]),
                               hip.embed_grad_ss_mark(first.sk, B, skip), B, len(smp), 1)
        held = _defined_marks(first.smp, first.ss[1], B, len(smp), 1)
        assert len(fresh) == len(held) == 6
        for a, b in zip(held, fresh):
            assert a.shape == b.shape and torch.equal(a, b)
    finally:
        EmbeddingLayer.unpin_sorts()
