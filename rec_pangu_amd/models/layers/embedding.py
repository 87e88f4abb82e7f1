"""EmbeddingLayer — drop-in for rec_pangu/models/layers/embedding.py:11-71, MI355X-first.

Same constructor, same `emb_feature` order (enc_dict key order of entries with 'vocab_size'),
same ModuleDict of nn.Embedding(vocab_size+1, D) and therefore the same state_dict keys
(`embedding_layer.<col>.weight`) and the same RNG draws at construction.

What is different is where the rows live: all tables of the layer are views into ONE contiguous
arena [sum(vocab+1), D] (HBM layout for the fused gather: a lookup is arena[row_base[f]+id]), and
their gradients are views into one dense gradient arena that the HIP backward writes in place.
`module.to()/cuda()/float()` move the arena once and re-point the per-table Parameters; anything
that replaces a table tensor behind our back (set_weights, external .data assignment) is detected
at the next forward and the arena is re-packed.

Device dispatch is by where the arena lives: a HIP-resident layer ALWAYS runs the HIP kernels
(rec_pangu_amd/hip.py raises if the library is missing — no fallback); a CPU-resident layer is
BASELINE.json config 0 ("plumbing, no GPU") and uses plain torch ops.
"""
import copy
import os
import weakref
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Union

import torch
from torch import nn

from ... import functional as Fh
from ...grad_arena import GradArena


class SortedLookup:
    """The sorted lookup of one batch and everything made from it: `keys` (arena row of every (field, sample) pair), their
    sort (`sk` sorted keys, `sp` positions), what identifies the batch (`src` id tensors, their `versions` at sort time,
    `sig` = (rows per table, device)), the side-stream `event` of a sort started ahead, and the marks the three-form backward
    wants: `smp` (rp_embed_grad_smp's duplicate marks, made for `smp_sig` = (B, big tables)) and `ss` = (skip mask,
    rp_embed_grad_ss's unique-row lists).  The marks live and die with the sort they describe.

    A PINNED lookup (graph_step.GraphedTrainStep) belongs to STATIC id tensors that are refilled in place: its tensors are
    persistent and re-sorted / re-marked IN PLACE (a recorded step holds all their addresses), it is matched by identity
    only (a refill bumps the versions) and carries no event (the order is the capture's).  `workspace`: its persistent sort
    workspace — a captured step's re-sort must not allocate (its launches may be re-issued on a side stream, where memory
    of the capture's pool could alias the step's temporaries); `want_marks`: whether a re-sort also re-makes the marks."""
    __slots__ = ("keys", "sk", "sp", "src", "versions", "sig", "event", "pinned", "workspace", "want_marks",
                 "smp_sig", "smp", "ss")

    def __init__(self, keys, sk, sp, src=None, sig=None, event=None, pinned=False, workspace=None, want_marks=True):
        self.keys, self.sk, self.sp, self.src, self.sig, self.event = keys, sk, sp, src, sig, event
        self.versions = None if src is None else tuple(t._version for t in src)
        self.pinned, self.workspace, self.want_marks = pinned, workspace, want_marks
        self.smp_sig = self.smp = self.ss = None

    def matches(self, src, sig) -> bool:
        """the sort of these very id tensors (identity) for this arena — and, unless pinned, of their current content"""
        return (self.sig == sig and len(self.src) == len(src) and all(a is b for a, b in zip(self.src, src))
                and (self.pinned or self.versions == tuple(t._version for t in src)))

    def wait_on(self, stream) -> None:
        """sorted ahead on the side stream: order `stream` behind it and tell the allocator who uses the tensors now"""
        if self.event is None:
            return
        stream.wait_event(self.event)
        for t in (self.keys, self.sk, self.sp) + (self.smp or ()) + (self.ss[1] if self.ss else ()):
            t.record_stream(stream)
        self.event = None

    def mark(self, B: int, smp, skip) -> None:
        """(re-)make the marks behind the sort, on the current stream: the duplicate marks of the big tables `smp` and — `skip`
        not None — the unique-row lists of the fields outside `skip`; in place where buffers of that signature are held"""
        from ... import hip
        sig = (B, tuple(smp))
        same = self.smp_sig == sig
        self.smp = hip.embed_grad_smp_mark(self.sk, self.sp, B, [t[0] for t in smp], out=self.smp if same else None)
        self.smp_sig = sig
        if skip is None:
            self.ss = None
        else:
            out = self.ss[1] if (same and self.ss is not None and self.ss[0] == skip) else None
            self.ss = (skip, hip.embed_grad_ss_mark(self.sk, B, skip, out=out))

    def ss_lists(self, skip: int):
        """the unique-row lists made with the sort for exactly these kept fields, or None (rp_embed_grad_ss makes its own)"""
        return self.ss[1] if (self.ss is not None and self.ss[0] == skip) else None


class GradForms(NamedTuple):
    """which form of the first layer's backward every table of a layer takes at one batch size (EmbeddingLayer._forms)"""
    tiny: Optional[list]  # [(field, first arena row, rows), ...] of rp_embed_grad_tiny's tables, or None
    big: Optional[list]   # ... of rp_embed_grad_smp's, or None
    skip: int             # bit f set: field f is one of those — the row-sorted form leaves its pairs out
    rest: bool            # mid-size fields remain for the row-sorted form ...
    ss: bool              # ... which is rp_embed_grad_ss (streaming) rather than rp_embed_grad_seg ...
    ss_ahead: bool        # ... with its unique-row lists made behind the sort


# the unpinned lookups of the last four batches (the batch in flight, the one whose sort was started ahead): two layers with
# the same vocabularies share one sort through it (EmbeddingLayer._sorted_keys / prefetch_sort)
_SORT_CACHE: list = []
_SORT_PINNED: list = []   # the pinned lookups (EmbeddingLayer.pin_sort): never evicted, dropped by unpin_sorts
_SIDE_STREAMS: dict = {}  # device -> the stream sorts started ahead run on


def _side_stream(dev):
    from ... import hip
    side = _SIDE_STREAMS.get(dev)
    if side is None:
        side = _SIDE_STREAMS[dev] = hip.make_side_stream(dev)  # (a high-priority stream measured no better)
    return side


def _find_sort(src, sig, cached: bool = True):
    """the pinned lookup of these id tensors, else (`cached`) the cached one of their current content, else None"""
    return next((look for look in (_SORT_PINNED + _SORT_CACHE if cached else _SORT_PINNED) if look.matches(src, sig)), None)


class DeferredGradView(torch.Tensor):
    """`.grad` of an embedding table while FusedAdam(defer=True) drives it (the contract was prose).

    Under the deferred execution a row's real optimizer step waits in the gradient arena until the row is next looked up, so
    between backward() and step() a table's gradient rows hold THIS step's gradients AND gradients of earlier steps that are
    still waiting — not the reference's dense gradient (rec_pangu/trainer.py:60-76 never reads it).  Anything that computes
    with such a tensor (gradient clipping, a norm, an in-place rescale) would silently read or damage waiting gradients:
    every torch operation on it RAISES instead.  Addresses, shapes and dtypes stay readable (the library checks that a
    table's .grad is still its arena view that way); `with rec_pangu_amd.models.layers.embedding.deferred_grad_reads():`
    opens the view for code that knows what the rows hold (tests, diagnostics); make_adam(..., defer=False) /
    RP_ADAM_DEFER=0 gives plain dense gradients."""
    _open = 0
    _META = {"data_ptr", "size", "stride", "dim", "numel", "nelement", "element_size", "is_contiguous", "storage_offset",
             "__get__", "__repr__", "__str__", "__format__", "__len__", "__hash__", "__reduce_ex__", "__deepcopy__",
             "is_floating_point", "is_complex", "get_device", "untyped_storage", "type", "requires_grad_", "_is_view"}

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        name = getattr(func, "__name__", "")
        if cls._open > 0 or name in cls._META:
            with torch._C.DisableTorchFunctionSubclass():
                out = func(*args, **(kwargs or {}))
            return out
        raise RuntimeError(
            f"torch.{name} on the .grad of an embedding table driven by FusedAdam(defer=True): its rows hold this step's "
            "gradients AND gradients of earlier steps whose optimizer step is still waiting (rec_pangu_amd/optim.py, deferred "
            "execution) — not a dense gradient.  Use make_adam(model, lr, defer=False) (or RP_ADAM_DEFER=0) when table gradients "
            "are read or rewritten between backward() and step() (gradient clipping), or wrap a knowing read in "
            "rec_pangu_amd.models.layers.embedding.deferred_grad_reads()")


class deferred_grad_reads:
    """context manager: table .grad views behave as plain tensors inside (see DeferredGradView)"""

    def __enter__(self):
        DeferredGradView._open += 1
        return self

    def __exit__(self, *exc):
        DeferredGradView._open -= 1
        return False


# set by rec_pangu_amd.sharded.sharded_construction(): models built inside it get row-sharded embedding layers that
# only ever allocate their own shard (see make_embedding_layer)
_SHARD_SPEC = None


def make_embedding_layer(enc_dict, embedding_dim: int):
    """What BaseModel / LR_Layer call to create their embedding layer: the arena-backed EmbeddingLayer, or — inside
    `sharded.sharded_construction(world, rank)` — a ShardedEmbeddingLayer holding rows r % world == rank, initialised
    with the very same RNG draws (table by table through a temporary) without ever allocating the full arena."""
    if _SHARD_SPEC is None:
        return EmbeddingLayer(enc_dict=enc_dict, embedding_dim=embedding_dim)
    from ...sharded import ShardedEmbeddingLayer
    return ShardedEmbeddingLayer.from_spec(enc_dict, embedding_dim, **_SHARD_SPEC)


class EmbeddingLayer(nn.Module):
    def __init__(self, enc_dict: Dict[str, Dict[str, Union[int, str]]], embedding_dim: int) -> None:
        super().__init__()
        self.enc_dict = enc_dict
        self.embedding_dim = embedding_dim
        self.embedding_layer = nn.ModuleDict()
        self.emb_feature: List[str] = []
        # "sync": raise IndexError right after the gather (one 4-byte D2H per forward, what the
        # reference's CPU nn.Embedding does); "deferred": only when raise_if_bad_index() is called.
        self.check_indices = "sync"

        rows = [enc_dict[c]["vocab_size"] + 1 for c in enc_dict.keys() if "vocab_size" in enc_dict[c].keys()]
        arena = torch.empty((sum(rows), embedding_dim))
        off = 0
        for col in self.enc_dict.keys():
            if "vocab_size" in self.enc_dict[col].keys():
                r = self.enc_dict[col]["vocab_size"] + 1
                self.emb_feature.append(col)
                emb = nn.Embedding(r, embedding_dim, _weight=arena[off:off + r])
                with torch.no_grad():
                    nn.init.normal_(emb.weight)  # the draw nn.Embedding.reset_parameters() would make
                self.embedding_layer.update({col: emb})
                off += r
        self._arena = arena
        self.grads = GradArena(overwrites=True)  # (every gradient launch of this layer writes ALL rows of its key list)
        self._dev_meta = None
        self._lazy = None        # optim.LazyAdamRows when the optimiser runs the exact lazy dense Adam
        self._presorted = None   # the SortedLookup of the batch being looked up
        self._fm_link = None     # functional.FMFold of the last gather that produced an FM term
        self._tag_tables()
        self.register_state_dict_pre_hook(lambda module, prefix, keep_vars: module.flush_lazy())
        # loading weights into a layer whose optimizer runs lazily: bring every row to the current step first, so that
        # no skipped zero-gradient step is replayed on top of the loaded values later
        self.register_load_state_dict_pre_hook(lambda module, *a, **k: module.flush_lazy())

    # ------------------------------------------------------------------ arena bookkeeping
    def _tables(self):
        """The per-table Parameters in field order.  Cached: walking the ModuleDict costs ~100 us per call at 26
        tables and this runs several times per step; the cache is dropped when a table Parameter object is replaced
        (set_weights, load with assign=True, ...), which the identity check below detects."""
        mods = self.__dict__.get("_tab_mods")
        tabs = self.__dict__.get("_tab_cache")
        if mods is not None:
            for m, p in zip(mods, tabs):
                if m._parameters["weight"] is not p:
                    mods = None
                    break
        if mods is None:
            mods = [self.embedding_layer[c] for c in self.emb_feature]
            tabs = [m.weight for m in mods]
            self.__dict__["_tab_mods"], self.__dict__["_tab_cache"] = mods, tabs
        return tabs

    def table_parameters(self):
        return self._tables()

    def _tag_tables(self):
        ref = weakref.ref(self)
        for p in self._tables():
            p._rp_store = ref  # lets FusedAdam find the arena behind a table Parameter

    def _point_at(self, arena: torch.Tensor):
        off = 0
        for p in self._tables():
            r = p.shape[0]
            p.data = arena[off:off + r]
            off += r
        self._arena = arena
        self._dev_meta = None
        self._tag_tables()

    def __deepcopy__(self, memo):
        """copy.deepcopy(model): nn.Parameter.__deepcopy__ clones every table into a storage of its own, which would
        tear the tables off the arena — and, with the lazy optimizer active, make the next forward re-pack the arena from
        table values that still owe their skipped steps while the moment arenas are stamped current.  The clone gets
        ONE copy of the arena (and of the gradient / moment arenas) and its tables are pointed back into it."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__setstate__({k: copy.deepcopy(v, memo) for k, v in self.__dict__.items()})
        new._point_at(new._arena)  # (same values: the arena copy and the table clones were taken from the same memory)
        if new.grads.buf is not None and self._grads_are_ours():
            new._attach_grads()
        return new

    def _apply(self, fn, recurse=True):
        # one move for the whole arena instead of one per table (module.to / .cuda / .float ...)
        self._ensure_packed()
        self.flush_lazy()
        self._point_at(fn(self._arena))
        if self._lazy is not None:
            self._lazy.apply(fn)
        self.grads.apply(fn)
        if self.grads.buf is not None:
            self._attach_grads()
        if self.__dict__.get("_shadow") is not None:
            self._shadow_stamp = None  # (rebuilt from the moved tables at the next training forward)
        return self

    def _ensure_packed(self):
        a, D = self._arena, self.embedding_dim
        off, ok = 0, True
        for p in self._tables():
            r = p.shape[0]
            if (p.device != a.device or p.dtype != a.dtype or p.dim() != 2 or p.shape[1] != D
                    or not p.is_contiguous() or off + r > a.shape[0]
                    or p.data_ptr() != a.data_ptr() + off * D * a.element_size()):
                ok = False
                break
            off += r
        if ok and off == a.shape[0]:
            tabs = self._tables()
            if tabs and (getattr(tabs[0], "_rp_store", None) is None or tabs[0]._rp_store() is not self):
                self._tag_tables()  # copy.deepcopy(model): the clone's tables still carried the original's weakref
            return
        # a table was replaced behind our back (set_weights, .data assignment, load with assign=True): re-pack.
        # Rows the lazy optimizer still owes steps to are brought up to date in the OLD arena first (the replaced table
        # is not in it any more, the others are); the moment arenas survive a same-shape re-pack with every row
        # stamped current, and are dropped (rebuilt by the optimizer) when the shape changed.
        if self._lazy is not None:
            self._lazy.flush(self)
        with torch.no_grad():
            tabs = self._tables()
            arena = torch.cat([p.detach().to(device=a.device, dtype=a.dtype).reshape(p.shape[0], -1) for p in tabs],
                              dim=0).contiguous()
        self.embedding_dim = arena.shape[1]
        self._point_at(arena)
        self.grads.drop()
        self._rows_sig_cache = None
        if self._lazy is not None and self._lazy.m.shape != arena.shape:
            self._lazy = None

    @property
    def arena(self) -> torch.Tensor:
        return self._arena

    def _meta(self):
        dev = self._arena.device
        if self._dev_meta is None or self._dev_meta[0].device != dev:
            rows = [p.shape[0] for p in self._tables()]
            base = [0]
            for r in rows[:-1]:
                base.append(base[-1] + r)
            self._dev_meta = (torch.tensor(base, dtype=torch.int64, device=dev),
                              torch.tensor(rows, dtype=torch.int64, device=dev),
                              torch.zeros((1,), dtype=torch.int32, device=dev),
                              max(1, int(sum(rows) - 1).bit_length()))
        return self._dev_meta

    row_base = property(lambda self: self._meta()[0])
    row_count = property(lambda self: self._meta()[1])
    err_flag = property(lambda self: self._meta()[2])

    def raise_if_bad_index(self):
        """Turn the device-side out-of-range flag into the reference's IndexError (synchronises)."""
        if self._dev_meta is not None and self._arena.is_cuda and int(self._dev_meta[2].item()) != 0:
            self._dev_meta[2].zero_()
            raise IndexError("index out of range in self")

    # ------------------------------------------------------------------ gradients (HIP path)
    def _attach_grads(self):
        off = 0
        guard = self._lazy is not None and bool(getattr(self._lazy, "defer", False))
        for p in self._tables():
            r = p.shape[0]
            if p.requires_grad:  # a frozen table (set_weights(trainable=False)) never shows a gradient
                view = self.grads.buf[off:off + r]
                # (deferred lazy Adam: the rows of other steps wait in this arena — computing with the view raises)
                p.grad = view.as_subclass(DeferredGradView) if guard else view
            off += r

    @property
    def grad_arena(self):
        return self.grads.buf

    def grads_are_arena(self) -> bool:
        """True when every table's .grad is the matching view of the gradient arena."""
        return self._grads_are_ours() and all(p.requires_grad for p in self._tables())

    def grads_were_zeroed(self):
        """FusedAdam(fuse_zero_grad) cleared the whole gradient arena."""
        self.grads.zeroed()

    def _grads_are_ours(self) -> bool:
        g, D = self.grads.buf, self.embedding_dim
        if g is None:
            return False
        off = 0
        for p in self._tables():
            if p.requires_grad and (p.grad is None or p.grad.data_ptr() != g.data_ptr() + off * D * 4
                                    or p.grad.shape != p.shape):
                return False
            off += p.shape[0]
        return True

    def flush_lazy(self):
        """Bring every row to the optimiser's current step (no-op unless the lazy Adam is active).  Called before
        anything reads the raw tables: state_dict(), .to(), checkpoints."""
        if self._lazy is not None:
            self._lazy.flush(self)

    def _tiny_tables(self):
        """[(field, first arena row, rows), ...] of the tables rp_embed_grad_tiny takes (whatever the batch size), or None"""
        return self._forms(0, big=False).tiny

    def _smp_tables(self, B: int):
        """[(field, first arena row, rows), ...] of the BIG tables rp_embed_grad_smp takes at batch size B, or None"""
        return self._forms(B).big

    def _forms(self, B: int, tiny: bool = True, big: bool = True) -> GradForms:
        """The form every table takes in the first layer's backward at batch size B: the ONE classification, read by the marks
        made behind a sort (_mark_sorted, possibly a step ahead on a side stream) and by the backward that consumes them
        (first_layer_grad).  tiny / big = False: for a call that form does not cover — its tables fall to the row-sorted form.
        Cached per (row signature, D, B); the switches are read when the record is made.
        TINY (rp_embed_grad_tiny): D = 64; each <= 254 rows, the smallest first while they fit 224 accumulator rows, at most
        16.
        BIG (round 6, rp_embed_grad_smp: the sample-major form): tables of at least B rows, where most runs of the sorted pair
        list are single pairs; not the tiny ones; < 2^24 rows each; the 16 largest; batches of RP_SMP_MIN_BATCH and more."""
        sig = self._rows_sig()
        key = (sig, self.embedding_dim, B, tiny, big)
        cache = self.__dict__.setdefault("_forms_cache", {})
        forms = cache.get(key)
        if forms is not None:
            return forms
        F = len(sig)
        fits = self.embedding_dim == 64 and F <= 64
        t = b = None
        if fits:
            pick, total = [], 0
            for f in sorted(range(F), key=lambda f: sig[f]):
                if sig[f] <= 254 and total + sig[f] <= 224 and len(pick) < 16:
                    pick.append(f)
                    total += sig[f]
            if total >= 1 and len(pick) >= 2:  # (a single tiny table is not worth two extra launches)
                t = [(f, sum(sig[:f]), sig[f]) for f in sorted(pick)]
        # (batches below RP_SMP_MIN_BATCH keep round 5's single row-sorted launch: the three-form backward is 16 launches more,
        #  and a b = 8192 step — the per-GPU batch of a strong-scaling run — is bound by launches: 0.50 ms against 0.43)
        if big and fits and B >= int(os.environ.get("RP_SMP_MIN_BATCH", "32768")):
            taken = {x[0] for x in t or ()}
            pick = sorted((f for f in range(F) if f not in taken and B <= sig[f] < (1 << 24)), key=lambda f: -sig[f])[:16]
            if pick and len(pick) * B < (1 << 24) and sum(sig) < (1 << 31):
                b = [(f, sum(sig[:f]), sig[f]) for f in sorted(pick)]
        t = t if tiny else None
        skip = sum(1 << x[0] for x in (t or []) + (b or []))
        rest = skip != (1 << F) - 1
        # the streaming form (rp_embed_grad_ss) only beside the sample-major one; its unique-row lists are made with the sort
        # unless RP_SS_MARK_AHEAD=0 (then rp_embed_grad_ss makes its own)
        ss = bool(b) and rest
        forms = cache[key] = GradForms(t, b, skip, rest, ss, ss and os.environ.get("RP_SS_MARK_AHEAD", "1") != "0")
        return forms

    def _mark_sorted(self, look: SortedLookup, force: bool = False) -> None:
        """behind a sort of this layer's pairs (on the stream that sorted them): the duplicate marks of the big tables and the
        unique-row lists of the mid-size ones (every field that is neither tiny nor big: rp_embed_grad_ss).  Only for a layer
        whose backward has taken the three-form path before (`_marks_wanted`, set by first_layer_grad) — DCN, xDeepFM, AutoInt and
        MMOE reduce through rp_embed_grad_reduce and made six launches' worth of marks per step for nobody."""
        if not (force or getattr(self, "_marks_wanted", False)):
            return
        F, n = len(self.emb_feature), look.sk.numel()
        forms = self._forms(n // F) if (n > 0 and n % F == 0) else None
        if forms is not None and forms.big:
            look.mark(n // F, forms.big, forms.skip if forms.ss_ahead else None)

    # The three backward passes below share their opening and closing: the protocol of the gradient arena (grad_arena.py).
    def _grad_begin(self, keys, presorted):
        """the gradient arena allocated or sparsely re-zeroed, the sort taken or made, the catch-up launch's promise settled
        -> (the SortedLookup, whether the tables' .grad views have to be attached at the end, whether the launches accumulate)"""
        from ... import hip
        fresh = not self._grads_are_ours()
        acc = self.grads.open(self._arena, fresh)
        look = presorted if presorted is not None else SortedLookup(keys, *hip.sort_pairs(keys, end_bit=self._meta()[3]))
        self.grads.settle(look.sk)
        return look, fresh, acc

    def _grad_end(self, sk, fresh: bool) -> None:
        self.grads.close(sk)
        if fresh:
            self._attach_grads()

    def accumulate_grad(self, keys, B: int, dx, gfm, ssum, presorted=None):
        """Called from the autograd node of the gather: dense table gradients, reference semantics
        (aten::embedding_dense_backward: every table gets a full [V+1, D] gradient, zeros where no
        sample looked) — the plain segmented reduce of dx [B, ldx]."""
        from ... import hip
        look, fresh, acc = self._grad_begin(keys, presorted)
        hip.embed_grad_reduce(look.sk, look.sp, B, self.embedding_dim, dx, gfm, ssum, self._arena, self.grads.buf,
                              accumulate=acc)
        self._grad_end(look.sk, fresh)

    def pool_grad(self, field: int, ids, g, inv, bag, L: int, presorted=None):
        """the backward of the pooled multi-id lookup of table `field`: g [B, D], inv = 1 / count or None, bag = the bag of
        every id or None, L ids per dense bag; the keys of its flat id list are made here unless their sort came along"""
        from ... import hip
        keys = None if presorted is not None else \
            hip.embed_keys(self.row_base[field:field + 1], self.row_count[field:field + 1], [ids], self.err_flag)
        look, fresh, acc = self._grad_begin(keys, presorted)
        hip.embed_pool_bwd(look.sk, look.sp, self.embedding_dim, g, inv, bag, L, self.grads.buf, accumulate=acc)
        self._grad_end(look.sk, fresh)

    def first_layer_grad(self, keys, B: int, dh, wt, gfm, ssum, presorted=None, dx=None, w=None, dw=None):
        """The backward of the lookup fused with the Linear that consumes x — its dgrad is formed inside the reduce from
        (dh, wt = W^T) — as NAMED LAUNCHES: this call only opens the pass (gradient arena, sort, the tables' forms); the autograd
        node issues `tiny`, `big`, `rest` or `gemm` in the order and on the plan section it wants and then `done`
        (functional._EmbedGatherLinear.backward: the one place that order is written down).
        w, dw ([64, K] each, both or neither): segment sums first, one matrix pass per run that also yields the embedding columns
        of the weight gradient dw — the forward stored no activation.  -> .forms (GradForms) and the launches:
          tiny    the tables of a few rows (Criteo: 8 fields, 31 % of the pairs): the sample-major one-hot path
          big(1)  round 6: the BIG tables (runs of the sorted list are mostly single pairs: the sort buys nothing and the
                  (field, row) order re-gathers every dH / S row once per field) go through the batch in sample order instead
                  (rp_embed_grad_smp): the marks if the sort had none, then its main launch -> the workspace `ws`
          big(2, ws)  the launches behind the sample-major one (the weight gradient's partial sums, the duplicate runs): other
                  rows than anything beside them
          rest    the row-sorted form over the remaining (mid-size) fields: rp_embed_grad_seg, or in two launches
                  rp_embed_grad_ss (a streaming segment-sum launch, then the matrix launch over the unique rows) with the
                  unique-row lists made with the sort — or just now, by big(1), for a sort nobody had marked
          gemm    (no w, dw) rp_embed_grad_gemm over every field that is not tiny, dx [B, ldx] added if given"""
        from ... import hip
        F, D = len(self.emb_feature), self.embedding_dim
        field_major = keys is not None and dx is None and keys.numel() == F * B
        if dw is not None and not field_major:
            raise RuntimeError("the fused first layer stored no activation, but its backward is not the field-major "
                               "single-device form rp_embed_grad_seg covers")
        look, fresh, acc = self._grad_begin(keys, presorted)
        # the tiny form only for the field-major all-fields call; the big one only with (w, dw) and where dh suits the kernel
        forms = self._forms(B, tiny=field_major, big=dw is not None and hip.embed_grad_smp_fits(D, 64, dh))
        to = (gfm, ssum, self._arena, self.grads.buf)

        def tiny():
            hip.embed_grad_tiny(keys, B, forms.tiny, dh, wt, *to, accumulate=acc, dw=dw)

        def big(phase, ws=None):
            if phase == 1:
                self._marks_wanted = True
                if look.smp_sig != (B, tuple(forms.big)):
                    self._mark_sorted(look, force=True)  # (a sort nobody marked: an eager backward that sorted for itself)
            return hip.embed_grad_smp(keys, look.smp, B, F, forms.big, dh, w, *to, accumulate=acc, dw=dw, phases=phase, ws=ws)

        def rest():
            launch, marks = (hip.embed_grad_ss, {"marks": look.ss_lists(forms.skip)}) if forms.ss else (hip.embed_grad_seg, {})
            launch(look.sk, look.sp, B, D, dh, w, *to, accumulate=acc, skip_fields=forms.skip, field_rows=self._rows_sig(),
                   dw=dw, **marks)

        def gemm():
            hip.embed_grad_gemm(look.sk, look.sp, B, D, dh, wt, dx, *to, accumulate=acc, skip_fields=forms.skip)

        return SimpleNamespace(forms=forms, tiny=tiny, big=big, rest=rest, gemm=gemm, done=lambda: self._grad_end(look.sk, fresh))

    # ------------------------------------------------------------------ reference API
    def set_weights(self, col_name: str, embedding_matrix: torch.Tensor, trainable: Optional[bool] = True) -> None:
        """embedding.py:36-47 — replace one table (re-packed into the arena at the next forward)."""
        self.embedding_layer[col_name].weight = nn.Parameter(embedding_matrix)
        if not trainable:
            self.embedding_layer[col_name].weight.requires_grad = False

    def _idx_list(self, X):
        out = []
        for c in self.emb_feature:
            t = X[c]
            if t.dtype is not torch.int64 or t.dim() != 1 or not t.is_contiguous():
                t = t.long().reshape(-1).contiguous()
            out.append(t)
        return out

    def gather_concat(self, X, dense: List[torch.Tensor], want_fm: bool, pad_to: int = 64):
        """HIP path: (x [B, ldx], fm [B,1] or None).  x = embeddings (F*D) | dense (ND) | zero pad."""
        self._ensure_packed()
        return self._gather(self._idx_list(X), None, dense, want_fm, pad_to, src=tuple(X[c] for c in self.emb_feature))

    def gather_linear_fits(self, n_dense: int, linear: nn.Linear, pad_to: int = 64) -> bool:
        """can lookup + concat + FM + `linear` (+ ReLU) run as the one fused launch (rp_embed_gather_linear_fwd)?"""
        from ... import hip
        F, D = len(self.emb_feature), self.embedding_dim
        d = F * D + n_dense
        ldx = Fh.padded(d, pad_to)
        w = linear.weight
        # (the answer only depends on shapes, alignment and the matrix-core mode: remembered per weight tensor — the check
        #  runs in every forward and used to stage the weight and cross the C ABI each time)
        key = (id(w), w.data_ptr() % 16, tuple(w.shape), F, D, n_dense, pad_to, self._arena.is_cuda, hip.get_matmul_precision())
        hit = self.__dict__.get("_glf_cache")
        if hit is not None and hit[0] == key:
            return hit[1]
        ok = (self._arena.is_cuda and D == 64 and linear.out_features == 64 and linear.in_features == d
              and hip.get_matmul_precision() != "fp32"
              and hip.embed_gather_linear_fits(D, F, n_dense, 64, ldx, Fh._rows16(w)))
        self.__dict__["_glf_cache"] = (key, ok)
        return ok

    def bf16_lookup(self, enable: bool = True) -> None:
        """bf16-STORAGE inference (SURVEY D6's secondary mode): snapshot the tables into a bf16 copy of the arena (half the
        bytes: 4.3 GB at Criteo shape) that no-grad forwards of the fused lookup + first layer then read instead of the fp32
        arena — half the gather traffic, fp32 accumulation, logits within 6e-2 of the fp32 tables' (measured 3.7e-2; bf16 rounding of every
        looked-up value; outside the 1e-4 parity gate, which the fp32 tables keep).  The snapshot is taken of the CURRENT
        weights (owed optimizer steps flushed first); training on makes it stale — a forward that would read a stale
        snapshot raises.  enable=False drops it."""
        if not enable:
            self._arena_bf16 = None
            return
        self._ensure_packed()
        self.flush_lazy()
        self._arena_bf16 = self._arena.detach().to(torch.bfloat16)
        self._bf16_stamp = self._bf16_stamp_now()

    def bf16_training(self, enable: bool = True) -> None:
        """bf16-STORAGE TRAINING (SURVEY D6's perf mode with a stated tolerance; never the parity path): the fused lookup +
        first layer gathers from a bf16 LOOKUP COPY of the tables (half the row bytes) and stores its activation as bf16
        (half the bytes the weight gradient reads); the fp32 tables stay the master the optimizer works on, moments and
        every accumulation stay fp32.  The deferred table optimizer keeps the copy current: whenever rp_lazy_adam_catchup /
        _flush_deferred write a parameter row they write its round-to-nearest-even bf16 image too (needs
        make_adam(defer=True), the default; other optimizers on the tables raise).  Anything that changes the tables through
        torch (load_state_dict, set_weights, .to()) is noticed and the copy rebuilt.  Tolerance: the looked-up values are
        bf16-rounded (2^-9 relative): logits within 6e-2 of the fp32 tables' (tests/test_hip_models.py)."""
        if not enable:
            self._shadow = None
            return
        self._ensure_packed()
        if not self._arena.is_cuda or self.embedding_dim != 64:
            raise RuntimeError("bf16_training: a HIP-resident layer with embedding_dim 64 (the fused lookup + first layer)")
        self._shadow_rebuild()

    def _shadow_rebuild(self):
        self.flush_lazy()
        self._shadow = self._arena.detach().to(torch.bfloat16)
        self._shadow_stamp = self._shadow_stamp_now()

    def _shadow_stamp_now(self):
        # (torch-side writes bump these counters; the fused optimizer writes through raw pointers and keeps the copy itself)
        return (self._arena.data_ptr(), self._arena._version, tuple(p._version for p in self._tables()))

    def _shadow_for_training(self):
        sh = self.__dict__.get("_shadow")
        if sh is None:
            return None
        if sh.device != self._arena.device or sh.shape != self._arena.shape or self._shadow_stamp != self._shadow_stamp_now():
            self._shadow_rebuild()
            sh = self._shadow
        return sh

    def _bf16_stamp_now(self):
        """what the snapshot is valid for: torch's version counter of the arena, the lazy optimizer's step AND the
        library's weight epoch — the fused optimizers write the arena through raw pointers, which torch's counter does
        not see (FusedAdam(lazy_tables=False), torch.optim.Adam on the table views: ADVICE r3)"""
        from ... import hip
        return (self._arena._version, None if self._lazy is None else self._lazy.t, hip.weight_epoch(),
                tuple(p._version for p in self._tables()))

    def _bf16_arena_for_inference(self):
        a = self.__dict__.get("_arena_bf16")
        if a is None or torch.is_grad_enabled():
            return None
        stamp = self._bf16_stamp_now()
        if stamp != self._bf16_stamp or a.device != self._arena.device:
            raise RuntimeError("the bf16 snapshot of the embedding tables is stale (the model was trained or moved since "
                               "bf16_lookup()): call bf16_lookup() again, or bf16_lookup(False) to read the fp32 tables")
        return a

    def gather_linear(self, X, dense: List[torch.Tensor], linear: nn.Linear, out_link, pad_to: int = 64):
        """HIP path: (h1 [B, 64] = relu(linear(cat(emb, dense))), fm [B,1]) in one launch; x is written for the backward
        but never re-read in the forward."""
        self._ensure_packed()
        idx = self._idx_list(X)
        a16 = self._bf16_arena_for_inference()
        if a16 is not None:
            from ... import hip
            dense = [t.float().reshape(-1).contiguous() for t in dense]
            out = hip.embed_gather_linear_fwd_bf16(a16, self.row_base, self.row_count, idx, dense, Fh._rows16(linear.weight),
                                                   linear.bias, self.err_flag)
            if self.check_indices == "sync":
                self.raise_if_bad_index()
            return out
        F, D = len(idx), self.embedding_dim
        d = F * D + len(dense)
        ldx = Fh.padded(d, pad_to)
        dense = [t if (t.dtype is torch.float32 and t.dim() == 1 and t.is_contiguous()) else t.float().reshape(-1).contiguous()
                 for t in dense]
        src = tuple(X[c] for c in self.emb_feature)
        self._presorted = None
        shadow = self._shadow_for_training()  # (before the replay below: a rebuild flushes)
        if self._lazy is not None and self._lazy.t > 0:
            self._presorted = self._sorted_keys(idx, self.row_base, self.row_count, src)
            self._lazy.replay(self, self._presorted.sk)
        elif torch.is_grad_enabled():
            self._presorted = self._sorted_keys(idx, self.row_base, self.row_count, src, lookup_only=True)
        out = Fh.embed_gather_linear(self, idx, dense, ldx, linear.weight, linear.bias, out_link, shadow=shadow)
        self._start_sort_ahead()
        if self.check_indices == "sync":
            self.raise_if_bad_index()
        return out

    def _sorted_keys(self, idx, row_base, row_count, src, lookup_only: bool = False):
        """The SortedLookup of this batch's row requests.  Two layers with the same vocabularies fed the same batch (a
        model's D-wide tables and its LR_Layer's 1-wide ones) ask for the same arena rows: the second one reuses the first
        one's sort.  The cache entry keeps the id tensors alive, so `is` + `_version` identify them."""
        from ... import hip
        sig = self._sort_sig()
        look = _find_sort(src, sig) if src is not None else None
        if look is not None:
            if look.event is not None:
                look.wait_on(torch.cuda.current_stream(self._arena.device))
            return look
        if lookup_only:
            return None
        keys = hip.embed_keys(row_base, row_count, idx, self.err_flag)
        sk, sp = self._sort_pairs(keys) if row_base is self.row_base else hip.sort_pairs(keys, end_bit=self._meta()[3])
        look = SortedLookup(keys, sk, sp, src, sig)
        if row_base is self.row_base and torch.is_grad_enabled():
            self._mark_sorted(look)
        if src is not None:
            self._cache_sort(look)
        return look

    def _sort_sig(self):
        return (self._rows_sig(), str(self._arena.device))

    @staticmethod
    def _cache_sort(look: SortedLookup) -> None:
        _SORT_CACHE.append(look)
        del _SORT_CACHE[:-4]

    def prefetch_sort(self, X) -> None:
        """Announce the batch of the NEXT step.  Its (arena row, position) sort is started on this layer's side stream
        right after this layer's next forward has been enqueued, so that it runs beside that step's backward and
        optimizer kernels: the radix sort is a chain of short latency-bound launches (0.17 ms at Criteo shape on a few %
        of the chip), the kernels beside it are HBM-bound.  `X` must hold the very tensors the later forward is given
        (identity is the cache key).  No effect on results: the same kernels on the same inputs, another stream."""
        if self._arena.is_cuda and all(X[c].device == self._arena.device for c in self.emb_feature):
            self._ahead = X

    def _start_sort_ahead(self) -> None:
        from ... import hip
        X, self._ahead = self.__dict__.get("_ahead"), None
        if X is None:
            return
        src = tuple(X[c] for c in self.emb_feature)
        look = _find_sort(src, self._sort_sig())
        if look is not None:
            if look.pinned:
                # static input buffers of a graphed step: re-sort into the persistent tensors, ON THIS STREAM — their readers
                # (a captured step's launches, eager forwards that match the pinned entry by identity) take no event from a
                # side stream (the side-stream form had no join back)
                self._sort_into(X, look)
            return
        dev = self._arena.device
        side = _side_stream(dev)
        main = torch.cuda.current_stream(dev)
        side.wait_stream(main)  # the id tensors (and whatever produced them) are ordered on the caller's stream
        with torch.cuda.stream(side):
            idx = self._idx_list(X)
            # 'sync' mode raises at the step that finds a bad id: the keys of the NEXT batch must not set this step's flag
            # (its own gather checks the same ids again when its turn comes) — they get a scratch flag
            keys = hip.embed_keys(self.row_base, self.row_count, idx, self._ahead_flag())
            look = SortedLookup(keys, *self._sort_pairs(keys), src, self._sort_sig())
            self._mark_sorted(look)
            look.event = torch.cuda.Event()
            look.event.record(side)
        for t in src:
            t.record_stream(side)
        self._cache_sort(look)

    def _ahead_flag(self):
        if self.check_indices != "sync":
            return self.err_flag
        f = self.__dict__.get("_scratch_flag")
        if f is None or f.device != self._arena.device:
            f = self.__dict__["_scratch_flag"] = torch.zeros((1,), dtype=torch.int32, device=self._arena.device)
        return f

    def _sort_pairs(self, keys, out=None, workspace=None):
        """the (arena row, position) sort of a pair list that covers ALL fields of this layer in order, B pairs each: field
        segment by field segment (rp_sort_pairs_fields_i32: a table of r rows needs log2 r key bits, not the arena's — the same
        result in 49 instead of 78 field-passes at Criteo shape); a list that is not F equal segments: the plain sort"""
        from ... import hip
        F = len(self.emb_feature)
        n = keys.numel()
        if n > 0 and n % F == 0:
            return hip.sort_pairs_fields(keys, n // F, self._rows_sig(), out=out, workspace=workspace)
        return hip.sort_pairs(keys, end_bit=self._meta()[3], out=out, workspace=workspace)

    def _sort_into(self, X, look: SortedLookup) -> None:
        """re-sort a pinned lookup in place from the current content of its static id tensors, on the current stream"""
        from ... import hip
        hip.embed_keys(self.row_base, self.row_count, self._idx_list(X), self.err_flag, out=look.keys)
        self._sort_pairs(look.keys, out=(look.sk, look.sp), workspace=look.workspace)
        # (a pinned entry keeps the choice made when it was pinned: marks that first appear inside a recorded step's side
        #  section would be allocated by the capture behind the step's temporaries and run beside them)
        if look.want_marks:
            self._mark_sorted(look, force=True)

    def pinned_sort(self, X) -> Optional[SortedLookup]:
        """the pinned lookup of the static batch X, or None"""
        return _find_sort(tuple(X[c] for c in self.emb_feature), self._sort_sig(), cached=False)

    def pin_sort(self, X) -> None:
        """graph_step: X holds STATIC id tensors (refilled in place from now on).  Sort their current content into
        persistent tensors on the current stream and pin the cache entry; later prefetch_sort(X) calls re-sort in place."""
        from ... import hip
        look = self.pinned_sort(X)
        if look is None:
            src = tuple(X[c] for c in self.emb_feature)
            n = sum(t.numel() for t in src)
            ws = hip.sort_workspace(n, self._arena.device)
            if n % len(src) == 0 and n > 0:  # (the field-segmented sort's histograms are per field: a few KB more)
                ws2 = hip.sort_fields_workspace(n // len(src), len(src), self._arena.device)
                ws = ws2 if ws2.numel() > ws.numel() else ws
            look = SortedLookup(*(torch.empty((n,), dtype=torch.int32, device=self._arena.device) for _ in range(3)),
                                src, self._sort_sig(), pinned=True, workspace=ws,
                                want_marks=bool(getattr(self, "_marks_wanted", False)))
        self._sort_into(X, look)
        if look not in _SORT_PINNED:
            _SORT_PINNED.append(look)

    @staticmethod
    def unpin_sorts(X=None) -> None:
        """drop the pinned entries of the static batch X (all of them when X is None)"""
        _SORT_PINNED[:] = [] if X is None else [e for e in _SORT_PINNED if not any(t is x for t in e.src for x in X.values())]

    def _rows_sig(self):
        if getattr(self, "_rows_sig_cache", None) is None:
            self._rows_sig_cache = tuple(int(t.shape[0]) for t in self._tables())
        return self._rows_sig_cache

    def _gather(self, idx, meta, dense, want_fm: bool, pad_to: int, src=None):
        """idx: one contiguous int64 [n] per addressed table; meta = (row_base, row_count) of those tables or None
        for all fields in order; src: the batch's id tensors (identity = sort cache key) or None."""
        F, D = len(idx), self.embedding_dim
        d = F * D + len(dense)
        ldx = Fh.padded(d, pad_to)
        dense = [t.float().reshape(-1).contiguous() for t in dense]
        row_base, row_count = meta if meta is not None else (self.row_base, self.row_count)
        self._presorted = None
        if self._lazy is not None and self._lazy.t > 0:
            # exact lazy dense Adam: the rows this batch reads must first replay the zero-gradient steps they
            # skipped.  The (row, position) sort the backward needs anyway is done here and reused there.
            self._presorted = self._sorted_keys(idx, row_base, row_count, src if meta is None else None)
            self._lazy.replay(self, self._presorted.sk)
        elif src is not None and meta is None and torch.is_grad_enabled():
            # no replay to do (dense Adam / first step): the backward sorts — unless another layer already has
            self._presorted = self._sorted_keys(idx, row_base, row_count, src, lookup_only=True)
        out = Fh.embed_gather(self, idx, dense, ldx, want_fm, meta)
        self._start_sort_ahead()
        if self.check_indices == "sync":
            self.raise_if_bad_index()
        return out if want_fm else (out, None)

    def table_range(self, field: int):
        """(first arena row, rows) of table `field` as python ints (cached with the row signature)"""
        sig = self._rows_sig()
        return sum(sig[:field]), sig[field]

    def lookup_pooled(self, X: Dict[str, torch.Tensor], name: str, pooling: str = "sum",
                      offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The multi-id lookup of a `_seq` column fused with its pooling: what the reference writes as
        `MaskedSumPooling()(emb(X, name=name))` / `MaskedAveragePooling()(...)` (embedding.py:64-71 +
        layers/sequence.py:13-59), without the [B, L, D] intermediate -> [B, D].

        X[name]: [B, L] ids (dense bags, padding ids included, as the reference takes them) or, with `offsets`
        (int64 [B + 1]), a flat [nnz] id list in CSR form (ragged bags).  pooling: "sum" | "average" (the masked average
        counts non-zero ELEMENTS per (sample, column), like the reference)."""
        if pooling not in ("sum", "average"):
            raise ValueError("pooling must be 'sum' or 'average'")
        self._ensure_packed()
        base_name = name.replace("_seq", "") if "seq" in name else name
        ids = X[name].long()
        if not self._arena.is_cuda:  # BASELINE config 0 (CPU plumbing): the reference's own composition
            table = self.embedding_layer[base_name]
            if offsets is None:
                e = table(ids if ids.dim() == 2 else ids.view(-1, 1))
                s = e.sum(dim=1)
                return s if pooling == "sum" else s / (e.ne(0).sum(dim=1).to(e.dtype) + 1e-16)
            rows = table(ids.view(-1))  # ragged bags: segment sums over the flat id list
            lens = offsets[1:] - offsets[:-1]
            bag = torch.repeat_interleave(torch.arange(lens.numel()), lens)
            s = torch.zeros((lens.numel(), rows.shape[1]), dtype=rows.dtype).index_add(0, bag, rows)
            if pooling == "sum":
                return s
            cnt = torch.zeros_like(s).index_add(0, bag, (rows != 0).to(rows.dtype))
            return s / (cnt + 1e-16)
        f = self.emb_feature.index(base_name)
        if offsets is None:
            if ids.dim() != 2:
                ids = ids.view(-1, 1)
            B, L = ids.shape
        else:
            offsets = offsets.long().contiguous()
            B, L = offsets.numel() - 1, 0
        flat = ids.reshape(-1).contiguous()
        presorted = None
        if self._lazy is not None and self._lazy.t > 0:
            # lazy dense Adam: the rows this lookup reads first replay the zero-gradient steps they skipped
            from ... import hip
            keys = hip.embed_keys(self.row_base[f:f + 1], self.row_count[f:f + 1], [flat], self.err_flag)
            sk, sp = hip.sort_pairs(keys, end_bit=self._meta()[3])
            self._lazy.replay(self, sk)
            presorted = SortedLookup(keys, sk, sp)
        out = Fh.embed_gather_pool(self, f, flat, offsets, L, B, pooling, presorted)
        if self.check_indices == "sync":
            self.raise_if_bad_index()
        return out

    def forward(self, X: Dict[str, torch.Tensor], name: Optional[str] = None) -> torch.Tensor:
        self._ensure_packed()
        if name is None:
            if self._arena.is_cuda:
                x, _ = self.gather_concat(X, [], want_fm=False, pad_to=1)
                return x.view(x.shape[0], len(self.emb_feature), self.embedding_dim)
            feature_emb_list = []
            for col in self.emb_feature:
                inp = X[col].long().view(-1, 1)
                feature_emb_list.append(self.embedding_layer[col](inp))
            return torch.stack(feature_emb_list, dim=1).squeeze(2)
        # single-field / sequence lookups (embedding.py:64-71): the same gather kernel over ONE table, every
        # (sample, position) of a `_seq` column being one row of the batch it sees
        base_name = name.replace("_seq", "") if "seq" in name else name
        if self._arena.is_cuda:
            i = self.emb_feature.index(base_name)
            ids = X[name].long()
            shape = tuple(ids.shape) if "seq" in name else (ids.numel(), 1)
            meta = (self.row_base[i:i + 1], self.row_count[i:i + 1])
            x, _ = self._gather([ids.reshape(-1).contiguous()], meta, [], False, 1)
            return x.view(*shape, self.embedding_dim)
        if "seq" in name:
            inp = X[name].long()
            fea = self.embedding_layer[name.replace("_seq", "")](inp)
        else:
            inp = X[name].long().view(-1, 1)
            fea = self.embedding_layer[name](inp)
        return fea
