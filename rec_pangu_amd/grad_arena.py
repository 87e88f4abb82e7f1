"""GradArena — the dense gradient buffer of an arena-backed embedding layer and the bookkeeping that keeps it cheap.

THE INVARIANT kept between steps: the buffer is zero everywhere except the rows named by the `touched` key list, so a fresh
gradient costs a sparse re-zero (rp_zero_rows over that list), not a fill of the whole buffer (8.6 GB at Criteo shape).
A gradient launch of the layer OVERWRITES the rows of its sorted key list while the arena is `clean` (nothing touched) and
accumulates into them otherwise.

THE NO-CLEAR PROMISE on top of it: the deferred catch-up launch in front of a training forward (rp_lazy_adam_catchup,
optim.LazyAdamRows.replay) applies the gradient rows that waited for the batch's rows and would clear them — 1 of its 8 row
transfers, dead when the backward that follows overwrites the very same rows.  With `mark = 2` it leaves them uncleared.
That is allowed only when the layer's gradient launches write EVERY row of their key list (`overwrites`), the arena is
clean and RP_ADAM_NOCLEAR is not 0 (`may_leave_uncleared`); the launch's key list is then recorded (`promise`).  The promise
is kept by the next gradient launch if it overwrites exactly that list — the same tensor, or the same memory and length
(`settle(written)` on a clean arena).  Whoever else comes first clears the rows (`settle()`): a second lookup, the optimizer
step, a flush, a switch of the execution mode, a backward over another key list or an accumulating one.

A backward pass is   accumulate = grads.open(parameter arena, fresh)   allocate, or re-zero what zero_grad() left behind
                     grads.settle(sorted keys)                         the promise: kept or cleared
                     the layer's own launch(es) into grads.buf         (accumulate: the flag they take)
                     grads.close(sorted keys)                          the rows are touched now
`fresh` (the layer's .grad no longer shows this buffer: zero_grad() dropped it) and attaching .grad afterwards are the
layer's business.  A fused optimizer step that cleared every gradient row says `zeroed()`.

THE STORE PROTOCOL — what optim.FusedAdam / LazyAdamRows ask of a layer that keeps its tables in one arena
(models.layers.EmbeddingLayer, sharded.ShardedEmbeddingLayer):
    arena, embedding_dim   the parameter rows [rows, D] (fp32)
    grads                  its GradArena;  grad_arena: grads.buf, read-only
    _lazy                  the layer's LazyAdamRows, or None
    _meta()[3]             bits of an arena row number (the end bit of a key sort)
    grads_are_arena()      every table's .grad is (a view of) grads.buf
    grads_were_zeroed()    the fused step cleared the gradients: grads.zeroed()
    flush_lazy()           bring every row to the optimizer's current step
    table_parameters()     the nn.Parameters that live in the arena, in arena order
"""
import os
from typing import Optional

import torch

from . import hip

# RP_ADAM_NOCLEAR=0: the catch-up launch always clears the gradient rows it applies (the round-3 behaviour)
NOCLEAR = os.environ.get("RP_ADAM_NOCLEAR", "1") != "0"


class GradArena:
    def __init__(self, overwrites: bool):
        self.overwrites = overwrites  # every gradient launch of the layer writes ALL rows of its key list
        self.buf: Optional[torch.Tensor] = None
        self.touched: Optional[torch.Tensor] = None  # keys written since the buffer was last all zero ...
        self.unsorted = False                        # ... concatenated from several backward passes
        self.promised: Optional[torch.Tensor] = None  # sorted keys of the catch-up launch that left its rows uncleared

    @property
    def clean(self) -> bool:
        """the buffer exists and is all zero (but for promised rows): the next gradient launch overwrites"""
        return self.buf is not None and self.touched is None

    @property
    def may_leave_uncleared(self) -> bool:
        return self.overwrites and self.clean and NOCLEAR

    def open(self, like: torch.Tensor, fresh: bool) -> bool:
        """a buffer shaped like `like`, holding nothing but gradients that count -> whether the pass's launches accumulate"""
        if self.buf is None or self.buf.shape != like.shape or self.buf.device != like.device:
            self.buf = torch.zeros_like(like)
            self.zeroed()
        elif fresh and self.touched is not None:
            hip.zero_rows(self.touched, self.buf.shape[1], self.buf)  # zero_grad() dropped the rows of earlier passes
            self.zeroed()
        return self.touched is not None

    def settle(self, written: Optional[torch.Tensor] = None) -> None:
        """an outstanding promise ends here.  written: the sorted keys a gradient launch is about to write — kept if it
        overwrites the promised list itself; in every other case the promised rows are cleared now"""
        keys, self.promised = self.promised, None
        if keys is None:
            return
        if written is not None and self.touched is None and (
                written is keys or (written.data_ptr() == keys.data_ptr() and written.numel() == keys.numel())):
            return
        hip.zero_rows(keys, self.buf.shape[1], self.buf)

    def close(self, keys: torch.Tensor) -> None:
        if self.touched is None:
            self.touched, self.unsorted = keys, False
        else:  # several backward passes before one optimizer step: the union is no longer sorted
            self.touched, self.unsorted = torch.cat([self.touched, keys]), True

    def promise(self, keys: torch.Tensor) -> None:
        self.promised = keys

    def zeroed(self) -> None:
        self.touched, self.unsorted = None, False

    def sorted_touched(self, end_bit: int) -> Optional[torch.Tensor]:
        if self.touched is not None and self.unsorted:
            return hip.sort_pairs(self.touched, end_bit=end_bit)[0]
        return self.touched

    def apply(self, fn) -> None:
        """module.to(): (the layer flushed first, which settles — there is no promise to move)"""
        self.buf = None if self.buf is None else fn(self.buf)
        self.touched = None if self.touched is None else fn(self.touched)

    def drop(self) -> None:
        self.buf = self.promised = None
        self.zeroed()
