"""A whole training step — forward, backward, optimizer step, zero_grad — captured once and replayed: as a LAUNCH PLAN
(the library's own recorder, csrc/plan.hip: the recorded launches are re-issued with hipLaunchKernel — the device sees the
eager stream of kernels, the host spends a few microseconds per launch, and the next batch's row sort runs on a side stream
beside the step) when the captured step holds nothing but library launches, else as a hipGraph (backend="hipgraph", or a
step with ATen kernels / memsets in it: DCN's weight-space cumsum, a model with active dropout ...).

Why: the eager step of the headline configuration is 13 kernel launches + the 9 launches of the row sort behind autograd,
ctypes and torch.empty: ~1.0 ms of host time per step against ~1.3 ms on the device — and at the per-GPU batch of a
strong-scaling run (8192) the host IS the step time (1.10 ms eager against 0.32 ms replayed, profiles/microbench/probes/probe_graph.py).
Replaying a captured graph costs the host one launch (~0.1 ms) and the device no inter-kernel gaps of host origin.

What makes a step capturable here:
  * the STEP NUMBER lives on the device: every launch argument is frozen at capture, so the Adam kernels read the step from
    StepTables.t_dev (rp_adam_step / rp_lazy_adam_rows / rp_lazy_adam_cf_table with t_dev, rp_counter_add) and the
    per-step scalar tables are persistent buffers that the host extends in place (optim.StepTables);
  * STATIC INPUT BUFFERS, two sets: graph P reads the current batch from X[P] and its (keys, sorted keys, positions) from
    persistent tensors (EmbeddingLayer.pin_sort); the NEXT batch is copied into X[1-P] (one multi-tensor copy per dtype)
    before the launch and sorted at the END of graph P, on the same stream, into the tensors graph 1-P reads.  The sort
    is NOT overlapped with the step as the eager path does it (side stream): a fork inside one graph is replayed without
    overlap by this runtime, and a second graph on a second stream (measured 0.49 against 0.52 ms at b = 8192) died with
    memory access faults whenever the host ran more than a few steps ahead without a device-wide synchronisation
    (profiles/microbench/probes/probe_graph6.py) — one linear graph on one stream has run thousands of unsynchronised steps;
  * no host synchronisation inside the step: check_indices = "deferred" (raise_if_bad_index() after the run).

The captured launches are the eager path's own (same kernels, same order, same arguments except the step number's
source): results are bit-identical to the eager loop (tests/test_hip_graph.py).  Uses torch.cuda.CUDAGraph (= hipGraph
on ROCm) for the capture and for the allocator's graph-private pool; the first `eager_steps` calls run eagerly so that
optimizer state, gradient buffers and caches exist before the capture.
"""
import os
import time
from typing import Callable, Dict, Optional

import torch

from . import functional as _Fh
from . import hip
from .models.layers import embedding as _emb
from .sharded import route_stream, seed_scaled


def plan_refusal(n_kernel: int, n_other: int, plan_nodes: int, plan_streams: int) -> Optional[str]:
    """why a recording may not replay as a launch plan (None: it may) — the captured hipGraph's kernel / other node counts
    (hip.graph_node_counts) against what the plan recorded: a plan must hold every launch of the step, on one stream"""
    if n_other != 0:
        return f"the captured step holds {n_other} non-kernel node(s) (memset / memcpy)"
    if n_kernel != plan_nodes:
        return f"the captured step holds {n_kernel} kernel nodes, {plan_nodes} of them library launches"
    if plan_streams != 1:
        return f"the library launches were issued on {plan_streams} streams"
    return None


class _Capture:
    """What one capture produced: the hipGraph, the launch plan it replays as (None: as the hipGraph), the detached static
    outputs, the dropout launches in the step and the number of recorded argument words that point at the static inputs
    and are re-pointed at the caller's tensors (0: the step reads the static batches)."""

    def __init__(self, graph, plan, outs, drop_calls):
        self.graph, self.plan, self.outs, self.drop_calls, self.bind_sites = graph, plan, outs, drop_calls, 0

    def replay(self):
        (self.graph if self.plan is None else self.plan).replay()

    def destroy(self):  # (never under launches in flight: they read kernel arguments the graph executable owns)
        if self.plan is not None:
            self.plan.destroy()
        self.graph = self.plan = None


class _StaticBatch:
    """One of the two static batches (none allocated yet: batch None): the tensors X a captured step reads, the destination
    side of their staging copy (converted once), `valid` — X holds the content of the batch it stands for (false after a
    step that read the caller's tensors) —, `pin` — a row-sharded step's prepared lookup in persistent buffers — and the
    capture that reads X as its current batch."""

    def __init__(self, batch=None):
        self.X = {k: torch.zeros_like(v) for k, v in (batch or {}).items()}
        self.keys, self.tensors = list(self.X), list(self.X.values())
        self.copy_list = hip.CopyList(self.tensors)
        self.valid, self.pin, self.capture = False, None, None

    def fill(self, batch):
        src = [batch[k] for k in self.keys]
        # ONE launch for the ~40 columns of a batch: torch._foreach_copy_ issues a device-to-device copy per tensor here, and
        # 40 small copies cost the stream ~0.25 ms per step in dispatch gaps (rocprofv3: 42 x __amd_rocclr_copyBuffer per
        # step — what round 3 had read as "~10 us per graph node")
        if not self.copy_list(src) and not hip.multi_copy(self.tensors, src):
            torch._foreach_copy_(self.tensors, src)
        self.valid = True

    def drop_capture(self):
        if self.capture is not None:
            self.capture.destroy()
        self.capture = None


class GraphedTrainStep:
    """step = GraphedTrainStep(model, optimizer); out = step(batch, next_batch) in the training loop.

    `next_batch` is the batch of the following call (None at the end of an epoch: that step then runs eagerly).  The
    returned dict holds detached, STATIC tensors ('pred', 'loss', ...) that the next call on the same graph overwrites
    (do not keep an autograd graph of an earlier eager step alive across the first captured call: its AccumulateGrad nodes
    are bound to the eager stream).  `post_backward`: a hook run
    between backward and optimizer step (eager and captured alike).

    CONTRACT for the batches (launch plans re-point the recorded launches at the caller's own tensors, no staging copy):
    a batch handed in as `next_batch` is read TWICE — by that call's replay (its keys + row sort, a step ahead) and by the next
    call's (the step itself) — and both reads happen on the device after the calls have returned.  Its tensors must
    therefore stay alive and UNCHANGED from the call that announces them until MAX_IN_FLIGHT + 2 further calls have been
    made (the step holds references that long).  A loader that refills a device buffer in place is detected where torch can
    see it — the tensor's data pointer or version counter differs from what was announced — and the batch is then staged
    and re-sorted on the spot (correct, one copy + one sort slower); a refill torch cannot see (a raw kernel writing through
    data_ptr()) is the caller's responsibility.

    CONTRACT for the seed (row-sharded tables, world > 1): a step recorded as a launch plan seeds its backward with
    1 / world instead of 1, whatever `post_backward` is, and sharded.allreduce_dense_grads then skips its divide — the sum
    IS the mean.  A custom `post_backward` sees PRE-SCALED gradients there (unscaled ones in an eager step or in a step
    that replays as a hipGraph): one that divides by world itself, or clips before the reduce, must allow for it."""

    MAX_IN_FLIGHT = 6

    def __del__(self):
        try:
            if any(g is not None for g in self.graphs):
                torch.cuda.synchronize()
            for sb in self._batches:
                sb.drop_capture()
        except Exception:
            pass

    def __init__(self, model, optimizer, post_backward: Optional[Callable[[], None]] = None, eager_steps: int = 2,
                 backend: Optional[str] = None):
        if not getattr(model, "on_hip", False):
            raise RuntimeError("GraphedTrainStep needs a HIP-resident model")
        if not hasattr(optimizer, "set_device_clock"):
            raise RuntimeError("GraphedTrainStep needs rec_pangu_amd.optim.FusedAdam (device-resident step counters)")
        for m in model.modules():
            if getattr(m, "check_indices", "deferred") != "deferred":
                raise RuntimeError("GraphedTrainStep: set check_indices = 'deferred' on the embedding layers (a captured "
                                   "step cannot synchronise with the host; call raise_if_bad_index() after the run)")
        self.model, self.opt, self.post_backward = model, optimizer, post_backward
        # "plan": replay the captured step as a launch plan when it holds only library launches (checked against the
        # captured hipGraph's nodes), else as the hipGraph; "hipgraph": always the hipGraph
        self.backend = backend or os.environ.get("RP_GRAPH_BACKEND", "plan")
        if self.backend not in ("plan", "hipgraph"):
            raise ValueError("backend must be 'plan' or 'hipgraph'")
        # Row-sharded tables (sharded.ShardedEmbeddingLayer): the step is recorded as a launch plan too (round 6) — the
        # collectives are NOT issued under the capture, the plan is cut at each of them (sharded._recorded ->
        # rp_plan_host_mark) and a replay issues them itself between two segments — or captured WITH them as a hipGraph
        # (round 4): in the fixed-capacity exchange every split size is a constant, so RCCL's all-to-alls and the dense
        # all-reduce (post_backward = lambda: allreduce_dense_grads(model)) become graph nodes.  Every rank must capture and
        # replay in lockstep.  This is the one place where the kind of step is decided.
        self._sharded = not hasattr(model.embedding_layer, "pin_sort")
        if self._sharded and not hasattr(model.embedding_layer, "local_arena"):
            raise RuntimeError("GraphedTrainStep: unknown embedding layer type")
        # (sharded: the process group's watchdog thread polls the events of earlier, eager collectives while this thread
        # captures — legal only in thread-local capture mode; in the default global mode its hipEventQuery aborts the
        # process with hipErrorStreamCaptureUnsupported)
        self._error_mode = "thread_local" if self._sharded else "global"
        self._batches = (_StaticBatch(), _StaticBatch())  # graph P reads _batches[P], and prepares _batches[1 - P] for the next
        self.P = 0
        self.backend_used = None     # "plan" | "hipgraph" once the first step has been captured
        self.why_not_plan = None
        self.bind_report = None      # {"sites": {input: argument words}, "interior": derived pointers} of the last capture
        self.eager_left = eager_steps
        self._inflight, self._ev_pool = [], []  # completion events of the replays not yet known to have finished
        self._held = []          # the batches of the replays that may still be in flight (read from the caller's tensors)
        self._staged = None      # the caller's batch object whose content _batches[P] holds (sorted and pinned)
        self._staged_sig = None  # (data_ptr, version) of its tensors when it was announced (a recycled buffer re-stages)
        self._sig = self._pool = None
        self._dev = None         # host mirror of the device counters
        self._one = None         # the seed gradient of captured backward passes (see _seed_grad)
        self._seed = (None, None)  # (value, tensor): the cached seed of another value than 1
        # active dropout inside the step (the reference's default for xDeepFM / AutoInt / MMOE): the generator offset of a
        # step's start lives on the device (`_drop_clock`, advanced by the step's last launch), every dropout launch adds
        # its place in the step; the host generator is advanced after each replay, so eager and captured steps draw from
        # ONE stream of offsets (hip._dropout_seed_offset, csrc/dropout.hip: rp_dropout_fwd_dev)
        self._drop_clock = None
        self._drop_clock_host = None   # the value the device clock holds (will hold once the queued replays have run)
        self.replays = self.captures = 0
        # host time of the replay calls: `host_call_s` = inside __call__ WITHOUT the back-pressure wait (`host_wait_s`: the
        # host blocks there once MAX_IN_FLIGHT replays are queued — device time, not host work)
        self.host_call_s = self.host_wait_s = 0.0
        self.host_seg_max = {}         # slowest host time per part of a replay call (copy / prepare / replay / record / advance)
        self.host_call_max_s = 0.0     # the slowest single call (reset by the caller: bench.py's timed window)
        self._seg_t = 0.0
        self._last_plan = None

    # ---- what the two captures hold, as callers and tests read it (the replay path reads the records themselves) ---------
    graphs = property(lambda self: [sb.capture and sb.capture.graph for sb in self._batches])
    plans = property(lambda self: [sb.capture and sb.capture.plan for sb in self._batches])
    _drop_calls = property(lambda self: [sb.capture.drop_calls if sb.capture else 0 for sb in self._batches])

    # ---- pieces --------------------------------------------------------------------------------------------------------
    def _eager(self, batch, nxt):
        self._staged = None
        if nxt is not None:
            self.model.prefetch(nxt)
        out = self.model(batch)
        out["loss"].backward()
        if self.post_backward is not None:
            self.post_backward()
        self.opt.step()
        self.model.zero_grad()
        # detached: an autograd graph kept alive by a returned loss would keep its AccumulateGrad nodes (bound to THIS
        # stream) alive into the capture, which runs on another stream — that cross-stream dependency breaks the capture
        return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}

    def _alloc(self, batch):
        self._batches = (_StaticBatch(batch), _StaticBatch(batch))
        if not self._sharded:  # both static batches get their persistent sort buffers before anything is captured
            for sb in self._batches:  # (sharded: _sharded_pins, once the exchange capacity is known)
                self.model.embedding_layer.pin_sort(sb.X)
        self._one = torch.ones((), dtype=torch.float32, device=next(iter(batch.values())).device)
        self._drop_clock = torch.zeros((1,), dtype=torch.int64, device=self._one.device)
        self._held = []

    def _sig_of(self, batch):
        """what torch can see of a batch's buffers: (address, version counter) per tensor"""
        return [(t.data_ptr(), t._version) for t in batch.values()]

    def _stage_current(self, batch):
        cur = self._batches[self.P]
        cur.fill(batch)
        if not self._sharded:
            self.model.embedding_layer.pin_sort(cur.X)
        elif self._sharded_pins():
            # the route, id exchange and owner-side sort of the batch, eagerly (no replay prepared them beside the step before)
            self.model.embedding_layer.route_into(cur.X, cur.pin)
        self._staged = batch

    def _sharded_pins(self) -> bool:
        """round 6: a row-sharded step reads the part of its lookup that does not depend on the weights (route, requested rows,
        owner-side sort) from persistent buffers, filled by the replay of the step BEFORE it on the ahead stream
        (ShardedEmbeddingLayer.route_into inside the recording) — RP_SHARD_AHEAD=0: built inside the step itself (rounds 4-5)"""
        if os.environ.get("RP_SHARD_AHEAD", "1") == "0" or self.backend != "plan":
            return False
        emb, (a, b) = self.model.embedding_layer, self._batches
        if a.pin is not None and a.pin.capacity != emb._capacity:
            torch.cuda.synchronize()  # (the exchange capacity was re-measured: the recorded steps hold the old buffers)
            self._drop_captures()
            a.pin = b.pin = None
        if a.pin is None:
            pins = [emb.pinned_route(sb.X) for sb in (a, b)]
            if all(p is not None for p in pins):
                a.pin, b.pin = pins
        return a.pin is not None

    def _capture(self, P):
        """record the step of static batch P, judge whether it may replay as a launch plan, place the plan's streams"""
        cur, nxt = self._batches[P], self._batches[1 - P]
        if nxt.capture is None:
            # the flags describe the captures in use: with none left, a layer this capture no longer looks up must not keep
            # "a captured step rebuilds my window" from an earlier one (the capture below sets them again)
            for lz in self.opt._lazies():
                lz._cf_in_capture = False
        cap = self._record(cur, nxt, self.backend == "plan")
        if cap.plan is not None:
            why = plan_refusal(*hip.graph_node_counts(cap.graph.raw_cuda_graph()), cap.plan.nodes, cap.plan.streams)
            if why is not None:
                cap.plan.destroy()
                cap.plan, self.why_not_plan = None, why
                if self._sharded:
                    # plan refused and sharded: the recording holds foreign launches and no collective (the plan had taken
                    # them over) — once more, collectives included, as a plain hipGraph.  The refused graph goes first;
                    # self._pool is still what the first attempt got (None: a pool it opened dies with its graph, and the
                    # second attempt opens the one that is kept)
                    del cap
                    cap = self._record(cur, nxt, False)
        if self._pool is None:
            self._pool = cap.graph.pool()
        if cap.plan is not None:
            self._place(cap, cur, nxt)
        cur.capture = cap
        self.captures += 1
        self.backend_used = "plan" if cap.plan is not None else "hipgraph"

    def _record(self, cur, nxt, want_plan: bool) -> _Capture:
        """the python of one step on static batch `cur` under a stream capture (want_plan: and a plan recording) — no kernel
        runs; the next batch's look-ahead is recorded FIRST by a sharded step (_ahead_sharded) and LAST by an unsharded one"""
        world = getattr(self.model.embedding_layer, "world", 1) if self._sharded else 1
        seed = 1.0 / world if want_plan and world > 1 else 1.0  # (sharded._SEED_SCALED; the tensor is made outside the capture)
        if seed != 1.0 and self._seed[0] != seed:
            self._seed = (seed, torch.full_like(self._one, seed))
        # (keep_graph: the hipGraph_t stays inspectable — rp_graph_node_counts — and is only instantiated if it is replayed)
        g = torch.cuda.CUDAGraph(keep_graph=True) if want_plan else torch.cuda.CUDAGraph()
        plan = hip.LaunchPlan() if want_plan else None
        gen = hip.device_generator(self._drop_clock.device)
        drop = {"seed": gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, "clock": self._drop_clock, "calls": 0}
        self._dev = counters = self.opt.host_counters()
        self.opt.set_device_clock(True)
        try:
            torch.cuda.synchronize()
            hip.DROPOUT_CAPTURE[0] = drop
            if plan is not None:
                plan.begin()
            try:
                with torch.cuda.graph(g, pool=self._pool, capture_error_mode=self._error_mode), seed_scaled(seed != 1.0):
                    held = self._ahead_sharded(cur, nxt) if self._sharded else None
                    out = self.model(cur.X)  # (finds cur's pinned sort; nothing is announced inside the capture)
                    if plan is not None:
                        # the side section (the next batch's sort, recorded last) is forked here: beside the backward,
                        # where the eager path starts it too — beside the catch-up and the gather it costs more than it hides
                        plan.fork_here()
                    # the seed gradient is a persistent 1.0: loss.backward() would create it with an ATen fill kernel — the
                    # one launch of a DeepFM step that is not the library's (a launch plan must hold them all)
                    out["loss"].backward(gradient=self._seed_grad(out["loss"], seed))
                    if plan is not None:
                        hip.LaunchPlan.settle()
                    if self.post_backward is not None:
                        self.post_backward()
                    self.opt.step()
                    self.model.zero_grad()
                    if drop["calls"] > 0:  # the step's last launch on the main stream: the dropout clock of the next step
                        hip.counter_add_u64(self._drop_clock, 4 * drop["calls"])
                    if not self._sharded:
                        self._ahead_sort(nxt, plan)
            finally:  # (the plan's recording ends behind the capture; `held` lives until this function returns)
                hip.DROPOUT_CAPTURE[0] = None
                if plan is not None:
                    plan.end()
        finally:
            # the capture ran the python of one step without executing a kernel: put the host counters back
            self.opt.set_host_counters(counters)
            self.opt.set_device_clock(False)
        return _Capture(g, plan, {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, drop["calls"])

    def _ahead_sort(self, nxt, plan):
        """the next batch (already staged in its static tensors when the step is launched): keys + sort into its pinned
        tensors, recorded LAST.  It depends on nothing the step computes and touches persistent buffers only: a plan
        re-issues these launches on its side stream, beside the step (section 1)"""
        look = self.model.embedding_layer.pinned_sort(nxt.X)
        if look is None:
            raise RuntimeError("GraphedTrainStep: the static batch lost its pinned sort buffers")
        if plan is not None:
            plan.section(1)
        self.model.embedding_layer._sort_into(nxt.X, look)
        if plan is not None:
            plan.section(0)

    def _ahead_sharded(self, cur, nxt):
        """the NEXT batch's route, id exchange and owner-side sort into its persistent buffers: segments of the ahead stream
        (LaunchPlan.cut), forked at the start of a replay and joined at its end.  Recorded FIRST, every temporary held (the
        list returned) until the recording ends: they run BESIDE the step, whose temporaries must not land in memory the
        capture's allocator got back from them (hip.holding)"""
        if cur.pin is None:
            return None
        emb = self.model.embedding_layer
        hip.LaunchPlan.cut(1)
        with hip.holding() as held:
            emb.route_into(nxt.X, nxt.pin)
        hip.LaunchPlan.cut(0)
        emb.use_pinned(cur.pin)
        return held

    def _place(self, cap, cur, nxt):
        plan, dev = cap.plan, cur.tensors[0].device
        if self._sharded:
            # (no sections; the static inputs are filled by the staging copy.  Segments tagged for the ahead stream — the
            #  next batch's prepared lookup — run on the sharded path's own plain stream)
            if any(plan.seg_tags):
                plan.ahead_stream = route_stream(dev)
            return
        # the sections run on the very streams the eager path overlaps on (sort-ahead / first-layer weight gradient):
        # a stream of the plan's own may share the main stream's hardware queue (csrc/plan.hip)
        plan.set_streams(_emb._side_stream(dev), _Fh._side2_stream(dev))
        # Input rebinding: instead of copying every batch into a static input buffer, the recorded launch arguments that
        # point at those buffers are re-pointed at the batch's own tensors before each replay (rp_plan_bind_inputs /
        # _set_inputs).  ADVICE r5: an argument that points INSIDE a static input (a derived pointer: an offset view, a
        # column of a packed buffer) cannot be re-pointed — such a step keeps the staging copy.  (An input no launch reads
        # at all has no site and needs none; a launch that is not the library's would have refused the plan.)
        ins = cur.tensors + nxt.tensors
        sites, interior = plan.bind_report(ins)
        names = [f"cur:{k}" for k in cur.keys] + [f"next:{k}" for k in nxt.keys]
        self.bind_report = {"sites": dict(zip(names, sites)), "interior": interior}
        cap.bind_sites = plan.bind_inputs([t.data_ptr() for t in ins]) if interior == 0 else 0

    def _seed_grad(self, loss, value: float = 1.0):
        """the persistent 1.0 a captured backward starts from (created in _alloc, outside any capture); None — the default
        seed, an ATen fill — when the loss is not the float32 scalar every model here returns.  value = 1 / world: the seed of
        a row-sharded step recorded as a launch plan (sharded._SEED_SCALED), made in front of the capture"""
        one = self._one if value == 1.0 else (self._seed[1] if self._seed[0] == value else None)
        if one is not None and one.device == loss.device and one.dtype == loss.dtype and one.shape == loss.shape:
            return one
        return None

    def _sharded_capturable(self, batch) -> bool:
        """the fixed-capacity exchange is active for this batch size (measured by an earlier eager step): no split size
        comes back to the host inside the step"""
        emb = self.model.embedding_layer
        n = len(emb.emb_feature) * batch[emb.emb_feature[0]].numel()
        return emb.check_indices == "deferred" and emb._capacity is not None and n <= emb._capacity_n

    def _drop_captures(self):
        for lz in self.opt._lazies():  # (no capture in use rebuilds these states' closed-form windows any more)
            lz._cf_in_capture = False
        for sb in self._batches:
            sb.drop_capture()
        self._pool = None  # (the pool dies with its graphs)

    def reset(self):
        """drop the captured graphs (buffers they hold moved, the model or the batch shape changed)"""
        if torch.cuda.is_available():
            torch.cuda.synchronize()  # never destroy a graph executable that is still in flight
        self._drop_captures()
        if not self._sharded:
            for sb in self._batches:
                _emb.EmbeddingLayer.unpin_sorts(sb.X)
        self._batches, self._staged = (_StaticBatch(), _StaticBatch()), None

    # ---- live per-launch timing inside replayed steps (launch plans only) ------------------------------------------------
    def launch_names(self):
        """[(kernel name, section), ...] of the captured step's launches in recorded order (None unless it replays as a plan)"""
        pl = next((p for p in self.plans if p is not None), None)
        return None if pl is None else [pl.launch_name(k) for k in range(pl.nodes)]

    def set_probe(self, launch: int):
        for pl in self.plans:
            if pl is not None:
                pl.set_probe(launch)

    def last_probe_ms(self) -> float:
        return self._last_plan.probe_ms()

    # ---- the step ------------------------------------------------------------------------------------------------------
    def _fits(self, batch) -> bool:
        x = self._batches[0].X
        return batch.keys() == x.keys() and all(batch[k].shape == x[k].shape and batch[k].dtype == x[k].dtype and
                                                batch[k].device == x[k].device for k in x)

    def _seg(self, name):
        """slowest host time per part of the call (host_seg_max: where a stalled call stalled)"""
        t = time.perf_counter()
        if t - self._seg_t > self.host_seg_max.get(name, 0.0):
            self.host_seg_max[name] = t - self._seg_t
        self._seg_t = t

    def _choose_inputs(self, cap, cur, nxt, batch, next_batch):
        """where the replay reads its two batches: the caller's own tensors (a plan with re-bindable inputs, contiguous
        tensors) or the static batches, filled by the staging copy"""
        plan = cap.plan
        if (plan is not None and cap.bind_sites > 0 and all(t.is_contiguous() for t in batch.values())
                and all(t.is_contiguous() for t in next_batch.values())):
            # the replay reads this batch and sorts the next one straight from the caller's tensors: no staging copy
            plan.set_inputs([batch[k] for k in cur.keys] + [next_batch[k] for k in cur.keys])
            nxt.valid = False
            self._held.append((batch, next_batch))
            del self._held[:-(self.MAX_IN_FLIGHT + 2)]
            return
        if not cur.valid:  # (the step before read this batch from the caller's tensors: its static batch was never filled)
            cur.fill(batch)
        nxt.fill(next_batch)
        if plan is not None and cap.bind_sites > 0:
            plan.set_inputs(cur.tensors + nxt.tensors)

    def _wait_for_room(self):
        """bound how far the host runs ahead (a handful of launches in flight is all the overlap there is to win)"""
        if len(self._inflight) < self.MAX_IN_FLIGHT:
            return
        done = self._inflight.pop(0)
        t_w = time.perf_counter()
        done.synchronize()
        dt_w = time.perf_counter() - t_w
        self.host_wait_s += dt_w
        self.host_call_s -= dt_w  # (the wait is the device's time, not the host's)
        self._ev_pool.append(done)
        self._seg_t = time.perf_counter()

    def _advance_dropout_clock(self, gen, calls):
        off = gen.get_offset()
        if self._drop_clock_host != off:  # the first replay, or eager dropout calls since the last one
            self._drop_clock.fill_(off)
        gen.set_offset(off + 4 * calls)   # what `calls` eager dropout launches would have consumed
        self._drop_clock_host = off + 4 * calls

    def __call__(self, batch: Dict[str, torch.Tensor], next_batch: Optional[Dict[str, torch.Tensor]] = None):
        t_in = time.perf_counter()
        w0 = self.host_wait_s
        try:
            return self._call(batch, next_batch)
        finally:
            dt = time.perf_counter() - t_in
            self.host_call_s += dt
            own = dt - (self.host_wait_s - w0)  # (this call's time without its back-pressure wait)
            if own > self.host_call_max_s:
                self.host_call_max_s = own

    def _call(self, batch, next_batch):
        self._seg_t = time.perf_counter()
        if self.eager_left > 0 or next_batch is None:
            self.eager_left -= 1
            return self._eager(batch, next_batch)
        if not self._batches[0].X:
            self._alloc(batch)
        # a sharded batch outside the fixed-capacity exchange, or another shape than the captured one (the smaller last batch
        # of an epoch, or the batch before it, whose captured step would sort it): this step runs eagerly
        if (self._sharded and not self._sharded_capturable(batch)) or not (self._fits(batch) and self._fits(next_batch)):
            return self._eager(batch, next_batch)
        self._seg("fits")
        # not the batch announced by the previous call — or its tensors are not the ones (or no longer hold what) that call
        # sorted: stage and sort it now
        if self._staged is not batch or self._staged_sig != self._sig_of(batch):
            self._stage_current(batch)
        P = self.P
        cur, nxt = self._batches[P], self._batches[1 - P]
        gen = hip.device_generator(self._drop_clock.device)
        # (the dropout seed is a frozen launch argument: re-seeding re-captures)
        sig = self.opt.prepare_step() + (gen.initial_seed() & 0xFFFFFFFFFFFFFFFF,)
        if sig != self._sig:               # a table a graph points into has moved (capacity doubled, replay mode changed)
            if self._sig is not None:
                # launches of the old graphs may still be in flight (the host runs steps ahead): destroying a graph
                # executable under them frees the kernel arguments they read (observed: memory aperture violation)
                torch.cuda.synchronize()
                self._drop_captures()
            self._sig = sig
        if cur.capture is None:
            self._capture(P)
        self._seg("signature")
        cap = cur.capture  # (read here, behind the capture: a re-capture a few lines up may have replaced the one this call started with)
        self._choose_inputs(cap, cur, nxt, batch, next_batch)
        self._seg("copy")
        if self.opt.host_counters() != self._dev:  # eager steps ran in between
            self.opt.sync_device_clock()
        self._wait_for_room()
        self._seg("prepare")
        if cap.drop_calls > 0:
            self._advance_dropout_clock(gen, cap.drop_calls)
        cap.replay()
        if cap.plan is not None:
            self._last_plan = cap.plan
        self._seg("replay")
        ev = self._ev_pool.pop() if self._ev_pool else hip.Marker()
        ev.record()
        self._inflight.append(ev)
        self._seg("record")
        self.opt.advance_host()
        hip.bump_weight_epoch()
        self._dev = self.opt.host_counters()
        self._seg("advance")
        self.replays += 1
        self.P, self._staged, self._staged_sig = 1 - P, next_batch, self._sig_of(next_batch)
        return cap.outs
