"""torch.autograd.Function wrappers that put the HIP kernels (rec_pangu_amd/hip.py) on the autograd tape.

Everything here takes HIP-device fp32 tensors; nothing in this module computes on the CPU and
nothing falls back: a missing librecpangu_hip.so raises from hip.lib().
"""
import contextlib
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import hip

ACT_NONE, ACT_RELU, ACT_MASK = hip.ACT_NONE, hip.ACT_RELU, hip.ACT_MASK
ACT_TANH, ACT_SIGMOID, ACT_LEAKY = hip.ACT_TANH, hip.ACT_SIGMOID, hip.ACT_LEAKY


def act_code(module):
    """the GEMM-epilogue code of an activation module (rec_pangu/models/layers/activation.py:37-59 builds them by name),
    or None: ReLU, Tanh, Sigmoid, LeakyReLU at its default slope"""
    import torch.nn as nn
    if isinstance(module, nn.ReLU):
        return ACT_RELU
    if isinstance(module, nn.Tanh):
        return ACT_TANH
    if isinstance(module, nn.Sigmoid):
        return ACT_SIGMOID
    if isinstance(module, nn.LeakyReLU) and abs(module.negative_slope - 0.01) < 1e-12:
        return ACT_LEAKY
    return None


def _unit_inner(t: torch.Tensor) -> torch.Tensor:
    """Kernels take row-major 2-D views with unit inner stride (any leading dimension)."""
    if t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


def padded(width: int, pad_to: int) -> int:
    """width rounded up to a multiple of pad_to (pad_to <= 1: width itself): the leading dimension of a padded row buffer"""
    return width if pad_to <= 1 else (width + pad_to - 1) // pad_to * pad_to


def _wide_rows_grad(rows: torch.Tensor, used: int) -> Optional[torch.Tensor]:
    """the gradient buffer of a row buffer of which a block reads the first `used` columns only: zero-filled at full width
    when there are columns beyond them (they carry no gradient; the library's own fill), None when there are none (the
    wrapper then makes a [B, used] one)"""
    return hip.zeros(tuple(rows.shape), torch.float32, rows.device) if rows.shape[1] > used else None


# ----------------------------------------------------------------------------------------------
# K4  Linear (+bias, +ReLU)   — layers/deep.py:62-72
# ----------------------------------------------------------------------------------------------
def _rows16(w: torch.Tensor) -> torch.Tensor:
    """nn.Linear keeps W as [N, K] with row stride K; when K is not a multiple of 4 (DeepFM: 1677) its rows are not
    16-byte aligned and the GEMM would have to fetch W with scalar loads.  A [N, ceil4(K)] staging copy (a few
    hundred KB, one small launch) restores dwordx4 loads; the extra columns are never read (K is passed on)."""
    K = w.shape[1]
    if K % 4 == 0 or K <= 64 or not w.is_cuda:
        return w
    # one staging copy per weight VALUE: the key is torch's version counter plus hip.weight_epoch(), which the fused
    # optimizer kernels bump (they write parameters through raw pointers, invisibly to torch's counter).  DeepFM's forward
    # asks twice per step (the "does the fused launch fit" check and the launch itself).
    key = (w.data_ptr(), w._version, hip.weight_epoch(), torch.cuda.is_current_stream_capturing())
    hit = getattr(w, "_rp_rows16", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():  # (a cached tensor with a grad_fn would keep the weight's AccumulateGrad node alive)
        if w.dtype is torch.float32:
            out = hip.copy_rows(w.detach(), (K + 3) // 4 * 4)  # a library launch: part of a recorded launch plan
        else:
            buf = torch.empty((w.shape[0], (K + 3) // 4 * 4), dtype=w.dtype, device=w.device)
            buf[:, :K].copy_(w)
            out = buf[:, :K]
    if not key[3]:  # (inside a stream capture the copy must stay a node of every graph that uses it)
        try:
            w._rp_rows16 = (key, out)
        except AttributeError:
            pass
    return out


class FMFold:
    """Link between the gather node and the first Linear that consumes its output x (DeepFM): the FM part of the
    embedding gradient, g_fm[b] * S[b, :] added to every field's slice of dX[b], is folded into the dgrad GEMM that
    produces dX (rp_linear_fwd_rowadd) instead of being applied per (sample, field) pair in the segmented reduce.
    `dfm` is recorded by _GradTap (tap_fm_grad) when the loss backward produces it, before any Linear runs."""
    __slots__ = ("ssum", "ncols", "dfm", "folded", "dgrad", "D", "fused", "extra")

    def __init__(self, ssum, ncols, D=0):
        self.ssum, self.ncols, self.dfm, self.folded = ssum, ncols, None, False
        # the gradient of x[:, :ncols] from a consumer that read the embedding block as [B, F, D] tokens (token_view: AutoInt's
        # attention): left here by its backward, added into the other consumers' dX by the gather's backward
        self.extra = None
        # (dH, W^T) of the first Linear when its dgrad is left to the gather backward (rp_embed_grad_gemm): dX is then
        # never materialised; the Linear returns a stride-0 zero in its place
        self.dgrad, self.D, self.fused = None, D, False


class _TokenView(torch.autograd.Function):
    """x [B, ldx] (embedding block | dense | padding) -> a contiguous [B, F, D] copy of its first F*D columns (rp_copy_rows), for
    a consumer that reads the fields as tokens (AutoInt, autoint.py:44-46).  The slice + unflatten + reshape it replaces made a
    strided view whose re-pack was an ATen clone, and in the backward a zero-filled [B, ldx] slice gradient plus the ATen sum
    of the two consumers' gradients of x.  Here the token gradient is parked in the gather's link and the gather's backward
    adds it into the other consumer's dX with one library launch (rp_add_rows) — so x needs another consumer (the MLP)."""

    @staticmethod
    def forward(ctx, x, F: int, D: int, link):
        x = _unit_inner(x)
        out = torch.empty((x.shape[0], F * D), dtype=torch.float32, device=x.device)
        hip.copy_rows_to(x[:, :F * D], out)
        ctx.link = link
        return out.view(x.shape[0], F, D)

    @staticmethod
    def backward(ctx, dtok):
        ctx.link.extra = dtok.reshape(dtok.shape[0], -1).contiguous()
        return None, None, None, None


def token_view(x, F: int, D: int, link):
    return _TokenView.apply(x, F, D, link)


class _StackRows(torch.autograd.Function):
    """cat(ws, dim=0) of 2-D matrices with one column count, as ONE library launch (rp_multi_copy into the row blocks of a fresh
    buffer); the gradients leave as the row blocks (contiguous views) of the incoming one."""

    @staticmethod
    def forward(ctx, *ws):
        rows = [w.shape[0] for w in ws]
        out = torch.empty((sum(rows), ws[0].shape[1]), dtype=torch.float32, device=ws[0].device)
        dst, r0 = [], 0
        for r in rows:
            dst.append(out[r0:r0 + r])
            r0 += r
        src = [w.detach().contiguous() for w in ws]
        if not hip.multi_copy(dst, src):
            torch._foreach_copy_(dst, src)
        ctx.rows = rows
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        outs, r0 = [], 0
        for r in ctx.rows:
            outs.append(g[r0:r0 + r])
            r0 += r
        return tuple(outs)


def stack_rows(ws):
    return _StackRows.apply(*ws)


class _GradTap(torch.autograd.Function):
    """Identity whose backward records the incoming gradient in an FMFold.  Applied to the FM output AFTER the MLP
    forward, so that in the backward pass (later nodes run first) it fires before the MLP's first Linear computes dX.
    (A tensor hook would not do: hooks of a non-leaf tensor run only when its grad_fn — the gather, which also waits
    for dX — is about to execute.)"""

    @staticmethod
    def forward(ctx, t, link):
        ctx.link = link
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        ctx.link.dfm = g
        return g, None


def tap_fm_grad(fm, link):
    return _GradTap.apply(fm, link)


class ReluLink:
    """Hand-off between a Linear+ReLU (producer) and the Linear that consumes its output: the consumer's dgrad GEMM
    applies the producer's ReLU mask in its epilogue (RP_ACT_MASK with aux = its own input, y > 0 <=> pre > 0) and
    leaves the tensor here; the producer's backward skips its relu_bwd pass when the gradient it receives IS that
    tensor.  Holding the reference also keeps autograd from accumulating another consumer's gradient into it in
    place; a summed gradient is a different tensor and takes the ordinary path (masking twice is harmless)."""
    __slots__ = ("dx",)

    def __init__(self):
        self.dx = None


class _LinearAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act: int, fm_link=None, in_link=None, out_link=None):
        x = _unit_inner(x)
        K = weight.shape[1]
        y = hip.linear_fwd(x, _rows16(weight), bias, act, K=K)
        ctx.fm_link, ctx.in_link, ctx.out_link = fm_link, in_link, out_link
        ctx.act, ctx.K, ctx.has_bias = act, K, bias is not None
        ctx.save_for_backward(x, weight, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = _unit_inner(dy)
        dpre = dy
        if ctx.act == ACT_RELU:
            lk = ctx.out_link
            masked = lk is not None and lk.dx is not None and lk.dx.data_ptr() == dy.data_ptr() \
                and lk.dx.shape == dy.shape and lk.dx.stride() == dy.stride()
            if lk is not None:
                lk.dx = None
            if not masked:
                dpre = hip.relu_bwd(dy, y)
        elif ctx.act in (ACT_TANH, ACT_SIGMOID, ACT_LEAKY):
            dpre = hip.act_bwd(dy, y, ctx.act)  # through the activation's output: tanh 1 - y^2, sigmoid y (1 - y), leaky: sign
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # [ldx, N]: the dgrad GEMM is the same NT kernel on W^T; zero rows beyond K make it write the zeros of
            # x's padding columns itself (a strided fill of those columns costs more than the whole GEMM)
            wt = hip.transpose(weight, rows_out=x.shape[1])
            lk = ctx.fm_link
            if lk is not None and lk.D == 64 and weight.shape[0] == 64 and hip.get_matmul_precision() != "fp32" \
                    and hip.embed_grad_gemm_fits(lk.D, weight.shape[0], dpre, wt):
                # the consumer of this gradient is the embedding gather: its backward forms the dX rows it needs from
                # (dH, W^T) on the matrix core, inside the segmented reduce.  What flows back through autograd is a
                # stride-0 zero of the right shape (other consumers of x add their gradients to it as usual).
                lk.dgrad = (dpre, wt)
                # (the library's own fill: an ATen one would keep a recorded step from replaying as a launch plan)
                dx = hip.zeros((1, 1), x.dtype, x.device).expand(x.shape[0], x.shape[1])
                if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
                    dw, db = hip.linear_wgrad(dpre, x, ctx.K, want_bias=ctx.has_bias)
                return dx, dw, db, None, None, None, None
            dx = torch.empty_like(x)
            if lk is not None and lk.dfm is not None and lk.ssum is not None and hip.linear_fwd_rowadd(
                    dpre, wt, lk.dfm.reshape(-1).contiguous(), lk.ssum, lk.ncols, dx):
                lk.folded = True  # the gather backward now only applies the -g_fm * v part
            elif ctx.in_link is not None:
                hip.linear_fwd(dpre, wt, None, ACT_MASK, aux=x, out=dx)  # x = relu(...) of the producer: its mask
                ctx.in_link.dx = dx
            else:
                hip.linear_fwd(dpre, wt, None, ACT_NONE, out=dx)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = hip.linear_wgrad(dpre, x, ctx.K, want_bias=ctx.has_bias)
        return dx, dw, db, None, None, None, None


class _Activation(torch.autograd.Function):
    """an activation module as a launch of its own (rp_act_fwd / rp_act_bwd), for the places where it does not follow a Linear"""

    @staticmethod
    def forward(ctx, x, act: int):
        y = hip.act_fwd(_unit_inner(x), act)
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return hip.act_bwd(_unit_inner(dy), y, ctx.act), None


def activation(x, act: int):
    return _Activation.apply(x, act)


def linear_act(x, weight, bias=None, act: int = ACT_NONE, fm_link=None, in_link=None, out_link=None):
    """act(x[:, :K] @ weight^T + bias) for 2-D x; x may carry zero padding columns beyond K.
    in_link / out_link: ReluLink shared with the producing / consuming layer (see ReluLink)."""
    lead = None
    if x.dim() != 2:
        lead = x.shape[:-1]
        x = x.reshape(-1, x.shape[-1])
        in_link = None
    y = _LinearAct.apply(x, weight, bias, act, fm_link, in_link, out_link if lead is None else None)
    return y if lead is None else y.reshape(*lead, y.shape[-1])


class _MLPTail64(torch.autograd.Function):
    """hin [B,64] (output of a Linear+ReLU) -> [Linear 64x64 + ReLU] x L -> Linear 64 -> 1, ONE launch each way
    (rp_mlp_tail_fwd / rp_mlp_tail_bwd).  `in_link`: the ReluLink of the producing Linear+ReLU — the gradient that
    comes out is already masked by hin > 0, so that layer skips its relu_bwd pass."""

    @staticmethod
    def forward(ctx, hin, in_link, w_out, b_out, *wb):
        hin = _unit_inner(hin)
        L = len(wb) // 2
        Ws = [w.contiguous() for w in wb[:L]]
        bs = list(wb[L:])
        logit, hs = hip.mlp_tail_fwd(hin, Ws, bs, w_out.contiguous(), b_out)
        ctx.L, ctx.in_link, ctx.has_bias = L, in_link, [b is not None for b in bs] + [b_out is not None]
        ctx.save_for_backward(hin, w_out, *Ws, *hs)
        return logit

    @staticmethod
    def backward(ctx, dz):
        L = ctx.L
        hin, w_out, *rest = ctx.saved_tensors
        Ws, hs = rest[:L], rest[L:]
        dhin, dWs, dbs, dw_out, db_out = hip.mlp_tail_bwd(dz.reshape(-1).contiguous(), list(Ws), [hin] + list(hs),
                                                           w_out.contiguous())
        if ctx.in_link is not None:
            ctx.in_link.dx = dhin
        dbs = [d if hb else None for d, hb in zip(dbs, ctx.has_bias[:L])]
        return (dhin, None, dw_out.view_as(w_out), db_out if ctx.has_bias[L] else None, *dWs, *dbs)


class _MLPTail64BCE(torch.autograd.Function):
    """_MLPTail64 with the model's loss head inside both launches (rp_mlp_tail_fwd_bce / rp_mlp_tail_bwd_bce):
    forward(hin, in_link, label, p_eps, weight, n_add, w_out, b_out, *addends, *Ws, *bs) -> (pred [B,1], loss []).
    pred and every gradient are bit-identical to mlp_tail64 + sigmoid_bce (same arithmetic per row); the loss scalar is the
    same sum in another order.  A DeepFM step loses three launches of its critical path (sigmoid_bce_fwd, loss_finish,
    sigmoid_bce_bwd: 18 us of 0.87 ms at B = 65536)."""

    @staticmethod
    def forward(ctx, hin, in_link, label, p_eps: float, weight: float, n_add: int, w_out, b_out, *rest):
        ctx.set_materialize_grads(False)  # `pred` is normally not differentiated
        hin = _unit_inner(hin)
        addends, wb = rest[:n_add], rest[n_add:]
        L = len(wb) // 2
        Ws = [w.contiguous() for w in wb[:L]]
        bs = list(wb[L:])
        label = label.contiguous()
        pred, loss, hs = hip.mlp_tail_fwd_bce(hin, Ws, bs, w_out.contiguous(), b_out, [a.contiguous() for a in addends], label,
                                              p_eps, weight)
        ctx.cfg = (L, in_link, [b is not None for b in bs] + [b_out is not None], p_eps, weight, [tuple(a.shape) for a in addends])
        ctx.save_for_backward(hin, w_out, pred, label, *Ws, *hs)
        return pred, loss

    @staticmethod
    def backward(ctx, dpred, dloss):
        L, in_link, has_bias, p_eps, weight, shapes = ctx.cfg
        hin, w_out, pred, label, *rest = ctx.saved_tensors
        Ws, hs = rest[:L], rest[L:]
        n_add = len(shapes)
        if dloss is None and dpred is None:
            return (None,) * (8 + n_add + 2 * L)
        if dpred is not None or dloss is None:  # someone differentiated through `pred` itself (rare): the separate launches
            dz = None
            if dloss is not None:
                dz = hip.sigmoid_bce_bwd(pred, label, dloss, True, p_eps, weight)
            if dpred is not None:
                extra = dpred * (pred * (1 - pred))
                dz = extra if dz is None else dz + extra
            dz = dz.reshape(-1).contiguous()
            dhin, dWs, dbs, dw_out, db_out = hip.mlp_tail_bwd(dz, list(Ws), [hin] + list(hs), w_out.contiguous())
        else:
            dz = torch.empty((pred.shape[0],), dtype=torch.float32, device=pred.device) if n_add else None
            dhin, dWs, dbs, dw_out, db_out = hip.mlp_tail_bwd(None, list(Ws), [hin] + list(hs), w_out.contiguous(),
                                                               bce=(pred, label, dloss.contiguous(), p_eps, weight, dz))
        if in_link is not None:
            in_link.dx = dhin
        dbs = [d if hb else None for d, hb in zip(dbs, has_bias[:L])]
        dadds = [dz.reshape(sh) for sh in shapes]
        return (dhin, None, None, None, None, None, dw_out.view_as(w_out), db_out if has_bias[L] else None, *dadds, *dWs, *dbs)


def mlp_tail64_bce(hin, in_link, hidden, head, addends, label, p_eps: float = 0.0, weight: float = 1.0):
    """(pred [B,1], loss) = BCE(sigmoid(sum(addends) + tail(hin)), label): mlp_tail64 and sigmoid_bce as one launch each way"""
    Ws = [w for w, _ in hidden]
    bs = [b for _, b in hidden]
    return _MLPTail64BCE.apply(hin, in_link, label, float(p_eps), float(weight), len(addends), head[0], head[1], *addends, *Ws, *bs)


def mlp_tail64(hin, in_link, hidden, head):
    """hidden: [(weight [64,64], bias or None), ...] (1..3 layers, each followed by ReLU); head: (weight [1,64], bias)."""
    Ws = [w for w, _ in hidden]
    bs = [b for _, b in hidden]
    return _MLPTail64.apply(hin, in_link, head[0], head[1], *Ws, *bs)


# ----------------------------------------------------------------------------------------------
# K5  CrossNet (+ the fc that follows it in DCN)   — layers/interaction.py:119-141, ranking/dcn.py:64
# ----------------------------------------------------------------------------------------------
class _CrossNet(torch.autograd.Function):
    """forward(x0, wfc, bfc, L, w_0 .. w_{L-1}, b_0 .. b_{L-1}): the layers' parameters arrive one by one and are stacked by ONE
    library launch (rp_multi_copy) — torch.stack was two ATen cat launches per step —, their gradients leave as rows of the
    [L, d] results of rp_crossnet_param_grads.  A DCN step then holds library launches only (graph_step: launch plan)."""

    @staticmethod
    def forward(ctx, x0, wfc, bfc, L: int, *wb):
        x0 = _unit_inner(x0)
        d = wb[0].numel()
        stk = torch.empty((2 * L, d), dtype=torch.float32, device=x0.device)
        src = [t.detach().reshape(-1) for t in wb]
        if not hip.multi_copy([stk[i] for i in range(2 * L)], src):
            torch._foreach_copy_([stk[i] for i in range(2 * L)], src)
        W, Bv = stk[:L], stk[L:]
        wfc_c = None if wfc is None else wfc.contiguous()
        xout, logit, s = hip.crossnet_fwd(x0, d, W, Bv, wfc_c, bfc, want_x=wfc is None)
        ctx.d, ctx.L, ctx.fused_fc = d, L, wfc is not None
        ctx.shapes = [t.shape for t in wb]
        ctx.save_for_backward(x0, W, Bv, wfc_c, s)
        return logit if wfc is not None else xout

    @staticmethod
    def backward(ctx, g):
        """Streaming backward (rp_crossnet_bwd_rows): X_l = A_l X_0 + C_l, so the per-row kernel only emits dX_0 and
        2L+2 scalars per sample; the parameter gradients are one skinny wgrad GEMM V^T X_0 plus [L,d] arithmetic
        (rp_crossnet_param_grads)."""
        x0, W, Bv, wfc, s = ctx.saved_tensors
        g = g.contiguous()
        L, d = ctx.L, ctx.d
        fused = ctx.fused_fc
        dx0, V = hip.crossnet_bwd_rows(x0, d, W, wfc if fused else None, s, None if fused else g, g if fused else None)
        P, cs = hip.linear_wgrad(V, x0, d)                      # [2L+2, d], column sums of V
        colg = None
        if not fused:
            _, colg = hip.linear_wgrad(g, g, 1)                 # column sums of the incoming gradient
        dW, dB, dwfc = hip.crossnet_param_grads(P, cs, W, Bv, wfc.reshape(-1) if fused else None, colg)
        grads = [dW[i].view(ctx.shapes[i]) for i in range(L)] + [dB[i].view(ctx.shapes[L + i]) for i in range(L)]
        if fused:
            return (dx0, dwfc.view_as(wfc), cs[2 * L + 1:2 * L + 2], None) + tuple(grads)
        return (dx0, None, None, None) + tuple(grads)


def crossnet(x0, layer_w, layer_b, wfc=None, bfc=None):
    """x0 [B, >=d] -> X_L [B, d], or the fc logit [B,1] when (wfc [1,d], bfc [1]) are given.  layer_w / layer_b: the L
    layers' weight / bias parameters."""
    L = len(layer_w)
    return _CrossNet.apply(x0, wfc, bfc, L, *layer_w, *layer_b)


# ----------------------------------------------------------------------------------------------
# K6  xDeepFM CIN layer   — layers/interaction.py:164-168
# ----------------------------------------------------------------------------------------------
class CINLink:
    """Hand-off between the CIN's first layer and its collapsed last layer (both read X_0): the last layer's backward — which
    runs first — parks its gradient of X_0 here and the first layer's backward adds it into its own with one library launch
    (rp_add_rows), instead of autograd's ATen sum of the two [B, H D] gradients (a recorded step must hold none)."""
    __slots__ = ("dx0",)

    def __init__(self):
        self.dx0 = None


class CINForm(NamedTuple):
    """the kernel family that runs one CIN layer's forward, its gradient of X_0 / X_{k-1} and its weight gradient"""
    fwd: str
    bwd_x: str
    bwd_w: str


class CINPlan(NamedTuple):
    layers: Tuple[CINForm, ...]  # one per layer
    x0_contiguous: bool          # copy X_0 into 16-byte aligned rows first (the forms are then those of aligned rows)


def cin_forms(H: int, units, D: int, precision: Optional[str], rows_aligned: bool, n_outputs: int = 1) -> Optional[CINPlan]:
    """Which kernels run a CIN of `units` maps per layer over H fields of width D — the ONE place that decides it (the
    autograd functions below and CompressedInteractionNet._forward_hip execute what it returns).  precision: the
    matrix-core mode (None: the one in force); rows_aligned: x0.stride(0) % 4 == 0 and x0.data_ptr() % 16 == 0.
    None: no kernel form, the module composes the CIN from device ops — more than 32 fields, more than one output, or a
    WIDE middle layer (fed by more than 32 maps) without bf16.  bf16 below: precision is not "fp32" and D in {32, 64}.

      layer   fwd, bwd_x, bwd_w    condition                      launches
      first   pair, pair, pair     bf16, O <= 128, aligned rows   rp_cin_pair_pieces, rp_cin_pair_fwd; rp_cin_pair_bwd_x; _bwd_w
              pair, pair, f32      bf16, O <= 128, misaligned     ... but the weight gradient by rp_cin_layer_bwd_w
              bs, bs, bs           bf16, O > 128, aligned rows    rp_cin_bs_fwd; rp_cin_bs_bwd_x on W + W^T; rp_cin_bs_bwd_w
              bs, bs, f32          bf16, O > 128, misaligned      ... but the weight gradient by rp_cin_layer_bwd_w
              f32, f32, f32        no bf16                        rp_cin_layer_fwd; rp_cin_layer_bwd_x; rp_cin_layer_bwd_w
      middle  chunked (all three)  bf16, aligned rows             per chunk of <= 32 input maps rp_cin_bs_fwd (+ rp_accumulate);
                                                                  rp_cin_bs_bwd_x for X_0 and for X_{k-1}; rp_cin_bs_bwd_w
              f32, f32, f32        otherwise (<= 32 input maps)   as the first layer's
      last    head, last, last     L >= 2, rp_cin_last_fits       rp_cin_head_params_fwd + rp_cin_last_fwd + rp_add_scalars;
                                                                  rp_cin_last_bwd_x; rp_cin_last_bwd_v, rp_sum_all, _head_params_bwd
              last, last, last     L == 1, rp_cin_last_fits       rp_cin_last_* on X_{L-1} = X_0, weight-space arithmetic in torch
              f32_1ch, f32, f32    otherwise (D > 64)             the f32 form with the one output channel V = c . W_L

    (the bf16 operand pieces of bs and chunked come from hip.bf16_pieces, in front of each launch.)  A wide middle layer with
    misaligned rows sets x0_contiguous, and every layer takes its aligned-rows form.  X_1 .. X_{L-1} are the kernels' own
    allocations: always aligned.  The one run-time exception: a pair bwd_x whose g_out is not 16-byte aligned runs as bs
    bwd_x (_CINLayer.backward: _pair_reads)."""
    L = len(units)
    bf16 = (hip.get_matmul_precision() if precision is None else precision) != "fp32" and hip.cin_bs_fits(H, H, D)
    wide = any(u > 32 for u in units[:-2])
    if H > 32 or n_outputs != 1 or (wide and not bf16):
        return None
    aligned, f32, forms = rows_aligned or wide, CINForm("f32", "f32", "f32"), []
    if L >= 2:
        x = "pair" if hip.cin_pair_fits(H, units[0], D) else "bs"
        forms.append(CINForm(x, x, x if aligned else "f32") if bf16 else f32)
        forms += [CINForm("chunked", "chunked", "chunked") if bf16 and aligned else f32] * (L - 2)
    if hip.cin_last_fits(H, units[-2] if L >= 2 else H, D):
        forms.append(CINForm("head" if L >= 2 else "last", "last", "last"))
    else:
        forms.append(CINForm("f32_1ch", "f32", "f32"))
    return CINPlan(tuple(forms), wide and not rows_aligned)


def _pair_reads(g_out) -> bool:
    """rp_cin_pair_bwd_x loads g_out 16 bytes at a time"""
    return g_out is None or g_out.data_ptr() % 16 == 0


class _CINLayer(torch.autograd.Function):
    """A CIN layer in the pair, bs or f32 form (form.fwd "f32_1ch": f32 with want_out=False); xp None: X_{k-1} = X_0."""

    @staticmethod
    def forward(ctx, x0, xp, W, bias, H: int, M: int, D: int, want_out: bool, form: CINForm, link=None):
        x0 = _unit_inner(x0)
        same = xp is None
        xp_t = x0 if same else _unit_inner(xp)
        W = W.contiguous()
        O = W.shape[0]
        wst = None
        if form.fwd == "pair":  # one GEMM over the H(H+1)/2 pair products
            # (both layouts of the pair weights' bf16 pieces from one launch: the backward's is kept — the weights do not
            #  change between this forward and its backward)
            wsp, wst = hip.cin_pair_pieces(W.view(O, H, M), both=True)
            out, pooled = hip.cin_pair_fwd(x0, wsp, bias, H, O, D, want_out, True)
        elif form.fwd == "bs":
            out, pooled = hip.cin_bs_fwd(x0, xp_t, hip.bf16_pieces(W.view(O, H, M)), bias, H, M, O, D, want_out, True)
        else:
            out, pooled = hip.cin_layer_fwd(x0, xp_t, W, bias, H, M, D, want_out, True)
        ctx.cfg = (H, M, D, same, bias is not None, want_out, form)
        ctx.link = link
        ctx.save_for_backward(x0, None if same else xp_t, W, wst)
        if want_out:
            return out, pooled
        return pooled

    @staticmethod
    def backward(ctx, *grads):
        x0, xp, W, wst = ctx.saved_tensors
        H, M, D, same, has_bias, want_out, form = ctx.cfg
        g_out, g_pool = (grads if want_out else (None, grads[0]))
        g_out = None if g_out is None else g_out.contiguous()
        g_pool = None if g_pool is None else _unit_inner(g_pool)
        extra = None
        if ctx.link is not None and ctx.link.dx0 is not None:
            extra, ctx.link.dx0 = ctx.link.dx0, None
        if form.bwd_x == "f32":
            dx0, dxp, dW, db = hip.cin_layer_bwd(x0, x0 if same else xp, W, H, M, D, g_out, g_pool, has_bias)
        else:
            O, dxp = W.shape[0], None
            W3 = W.view(O, H, M)
            # X_0 enters in both roles: one pass with W[o,h,m] + W[o,m,h] gives its whole gradient
            gp = None if g_pool is None else g_pool.contiguous()  # [B, O] packed (it arrives as a slice of the cat)
            if form.bwd_x == "pair" and _pair_reads(g_out):
                # (the last layer's gradient of X_0, parked in the link: this launch adds its own into it)
                dx0 = hip.cin_pair_bwd_x(x0, wst, g_out, gp, H, O, D, like=x0, into=extra)
                extra = None
            else:
                dx0 = hip.cin_bs_bwd_x(x0, hip.bf16_pieces(W3 + W3.transpose(1, 2)), g_out, gp, H, M, O, D, like=x0)
        if extra is not None:
            hip.add_rows_to(extra, dx0[:, :extra.shape[1]])
        if form.bwd_w == "pair":  # symmetric pair form: products formed once, 2.9x fewer matrix-core passes
            dW, db = hip.cin_pair_bwd_w(x0, g_out, gp, H, O, D, has_bias)
        elif form.bwd_w == "bs":
            dW, db = hip.cin_bs_bwd_w(x0, x0, g_out, gp, H, M, O, D, has_bias)
        elif form.bwd_x != "f32":  # (misaligned rows; the f32 bwd_x above came with its weight gradient)
            dW, db = hip.cin_layer_bwd_w(x0, x0, W, H, M, D, g_out, g_pool, has_bias)
        return dx0, dxp, dW.view_as(W), db, None, None, None, None, None, None


class _CINLast(torch.autograd.Function):
    """The collapsed last CIN layer of a one-layer CIN (X_{L-1} = X_0, M = H): p[b] = sum_d sum_{h,m} V[h,m] X_0[b,h,d]
    X_0[b,m,d]  (rp_cin_last_*)."""

    @staticmethod
    def forward(ctx, x0, V, H: int, D: int):
        x0 = _unit_inner(x0)
        vt = torch.zeros((H, 32), dtype=torch.float32, device=x0.device)
        vt[:, :H] = V.reshape(H, H).t()
        ctx.cfg = (H, D)
        ctx.save_for_backward(x0, vt)
        return hip.cin_last_fwd(x0, x0, vt, H, H, D)

    @staticmethod
    def backward(ctx, gp):
        x0, vt = ctx.saved_tensors
        H, D = ctx.cfg
        dx0, dxp, dV = hip.cin_last_bwd(x0, x0, vt, gp.reshape(-1).contiguous(), H, H, D)
        return dx0 + dxp, dV.reshape(1, H * H), None, None  # (both roles are X_0, same row layout)


def cin_last(x0, V, H: int, D: int):
    """form "last": x0 [B, >=H*D], V [1, H*H] -> [B, 1]."""
    return _CINLast.apply(x0, V, H, D)


class _CINChunked(torch.autograd.Function):
    """A CIN layer whose second factor X_{k-1} is NOT X_0 (a middle layer), fed by any number of maps, on the bf16 matrix
    core: the sum over chunks of <= 32 maps of rp_cin_bs layers (interaction.py:164-168; include/rec_pangu_hip.h K6).
    X_k[b,o,:] = sum_c sum_{h, m in c} W[o,h,m] X_0[b,h,:] X_{k-1}[b,m,:] + bias[o]."""
    CHUNK = 32

    @staticmethod
    def forward(ctx, x0, xp, W, bias, H: int, M: int, D: int):
        x0, xp = _unit_inner(x0), _unit_inner(xp)
        O = W.shape[0]
        W3 = W.reshape(O, H, M)
        out = pooled = None
        for c0 in range(0, M, _CINChunked.CHUNK):
            c1 = min(M, c0 + _CINChunked.CHUNK)
            o_c, p_c = hip.cin_bs_fwd(x0, xp[:, c0 * D:c1 * D], hip.bf16_pieces(W3[:, :, c0:c1]), bias if c0 == 0 else None,
                                      H, c1 - c0, O, D, True, True)
            if out is None:
                out, pooled = o_c, p_c
            else:
                hip.accumulate(out, o_c)
                hip.accumulate(pooled, p_c)
        ctx.cfg = (H, M, D, bias is not None)
        ctx.save_for_backward(x0, xp, W3)
        return out, pooled

    @staticmethod
    def backward(ctx, g_out, g_pool):
        x0, xp, W3 = ctx.saved_tensors
        H, M, D, has_bias = ctx.cfg
        O = W3.shape[0]
        g_out = None if g_out is None else g_out.contiguous()
        gp = None if g_pool is None else g_pool.contiguous()  # packed [B, O]
        dx0 = None
        dxp = torch.empty((x0.shape[0], M * D), dtype=torch.float32, device=x0.device)
        dW = torch.empty((O, H, M), dtype=torch.float32, device=x0.device)
        db = None
        for c0 in range(0, M, _CINChunked.CHUNK):
            c1 = min(M, c0 + _CINChunked.CHUNK)
            mc = c1 - c0
            xc, Wc = xp[:, c0 * D:c1 * D], W3[:, :, c0:c1]
            # X_0-role gradient: rows h, contraction over the chunk's maps; X_{k-1}-role: rows m, contraction over h
            d0 = hip.cin_bs_bwd_x(xc, hip.bf16_pieces(Wc), g_out, gp, H, mc, O, D, like=x0)
            dx0 = d0 if dx0 is None else hip.accumulate(dx0, d0)
            hip.cin_bs_bwd_x(x0, hip.bf16_pieces(Wc.transpose(1, 2)), g_out, gp, mc, H, O, D, like=None,
                             out=dxp[:, c0 * D:c1 * D])
            dWc, dbc = hip.cin_bs_bwd_w(x0, xc, g_out, gp, H, mc, O, D, has_bias and c0 == 0)
            dW[:, :, c0:c1] = dWc.view(O, H, mc)
            if dbc is not None:
                db = dbc
        return dx0, dxp, dW.view(O, H * M), db, None, None, None


def cin_layer(x0, xp, W, bias, H: int, M: int, D: int, form: CINForm, want_out: bool = True, link=None):
    """One CIN layer in the form cin_forms chose: (X_k [B, O, D], pooled [B, O]), or pooled alone.  link: a CINLink shared
    with cin_head (the collapsed last layer's gradient of X_0 is added into the first layer's inside its backward)"""
    if form.fwd == "chunked":
        return _CINChunked.apply(x0, xp, W, bias, H, M, D)
    return _CINLayer.apply(x0, xp, W, bias, H, M, D, want_out, form, link)


class _CINHead(torch.autograd.Function):
    """The CIN's collapsed LAST layer with its weight-space arithmetic inside (round 6; models/layers/interaction.py has the
    algebra):  logit[b] = sum_d sum_{h,m} V[h,m] X_0[b,h,d] X_{L-1}[b,m,d] + D (c . b_L) + fc.bias,  V = c . W_L.
    One launch for (V^T, c . b_L), rp_cin_last_fwd, one launch for the two scalars; the backward's dW_L / db_L / dc from one
    launch.  What this replaces were two matmuls, four elementwise launches and their autograd counterparts per step."""

    @staticmethod
    def forward(ctx, x0, xp, WL, bL, c, fcb, H: int, M: int, D: int, link):
        x0 = _unit_inner(x0)
        xp = _unit_inner(xp)
        WL = WL.contiguous()
        c = c.reshape(-1).contiguous()
        vt, vb = hip.cin_head_params_fwd(WL, bL, c, H, M)
        out = hip.cin_last_fwd(x0, xp, vt, H, M, D)
        hip.add_scalars(out, vb, float(D), fcb)
        ctx.cfg, ctx.link = (H, M, D, bL is not None, fcb is not None, c.shape), link
        ctx.save_for_backward(x0, xp, vt, WL, bL, c)
        return out

    @staticmethod
    def backward(ctx, g):
        x0, xp, vt, WL, bL, c = ctx.saved_tensors
        H, M, D, has_b, has_fcb, cshape = ctx.cfg
        g = g.reshape(-1).contiguous()
        dx0, dxp, dV = hip.cin_last_bwd(x0, xp, vt, g, H, M, D)
        sg = hip.sum_all(g)
        dWL, dbL, dc = hip.cin_head_params_bwd(WL, bL, c, dV, sg, D, H, M)
        if ctx.link is not None:
            ctx.link.dx0, dx0 = dx0, None  # (added into the first layer's gradient of X_0 by its backward: CINLink)
        return dx0, dxp, dWL, dbL, dc.view(1, -1), (sg if has_fcb else None), None, None, None, None


def cin_head(x0, xp, WL, bL, c, fcb, H: int, M: int, D: int, link=None):
    """form "head": x0 [B, >= H D], xp = X_{L-1} [B, M D], WL [O, H M], bL [O] or None, c [1, O] (fc.weight's slice for the
    last layer's pooling), fcb [1] or None -> [B, 1]"""
    return _CINHead.apply(x0, xp, WL, bL, c, fcb, H, M, D, link)


class _RowSplit(torch.autograd.Function):
    """w [1, n] -> (w[:, :k], w[:, k:]) as tensors of their own that alias w's memory (no launch); the backward writes the two
    gradients into the halves of one [1, n] buffer with one library launch.  (Slicing a parameter leaves autograd a slice node
    per half: a zero fill and a copy each in the backward — ATen launches a recorded step must not hold.)"""

    @staticmethod
    def forward(ctx, w, k: int):
        ctx.k, ctx.n = k, w.shape[1]
        d = w.detach()
        return d[:, :k], d[:, k:]

    @staticmethod
    def backward(ctx, g1, g2):
        k, n = ctx.k, ctx.n
        ref = g1 if g1 is not None else g2
        g = torch.empty((1, n), dtype=torch.float32, device=ref.device)
        parts = []
        for gi, (a, b) in ((g1, (0, k)), (g2, (k, n))):
            parts.append((g[:, a:b], gi if gi is not None else hip.zeros((1, b - a), torch.float32, ref.device)))
        if not hip.multi_copy([p[0] for p in parts], [p[1].contiguous() for p in parts]):
            for dst, src in parts:
                hip.copy_rows_to(src, dst)
        return g, None


def row_split(w, k: int):
    return _RowSplit.apply(w, k)


class _TokenAlias(torch.autograd.Function):
    """_TokenView without the copy: the first F*D columns of x as a tensor of its own that aliases x's memory, for consumers that
    take a row stride (the CIN kernels).  The gradient takes the same road: parked in the gather's link, added into the other
    consumer's dX by the gather's backward (rp_add_rows)."""

    @staticmethod
    def forward(ctx, x, n: int, link):
        ctx.link = link
        return _unit_inner(x).detach()[:, :n]

    @staticmethod
    def backward(ctx, d):
        ctx.link.extra = d if d.is_contiguous() else d.contiguous()
        return None, None, None


def token_alias(x, n: int, link):
    return _TokenAlias.apply(x, n, link)



# ----------------------------------------------------------------------------------------------
# K7  AutoInt field self-attention layer   — layers/attention.py:63-101
# ----------------------------------------------------------------------------------------------
class _FieldAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, T: int, Din: int, H: int, a: int, has_res: bool, scale: float):
        x = _unit_inner(x)
        W = W.contiguous()
        out = hip.field_attention_fwd(x, W, T, Din, H, a, has_res, scale)
        ctx.cfg = (T, Din, H, a, has_res, scale)
        ctx.save_for_backward(x, W)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, W = ctx.saved_tensors
        T, Din, H, a, has_res, scale = ctx.cfg
        dx, dW = hip.field_attention_bwd(x, W, T, Din, H, a, has_res, scale, gout.contiguous(),
                                         ctx.needs_input_grad[0])
        return dx, dW, None, None, None, None, None, None


class _AttentionCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkvr, xres, T: int, H: int, a: int, scale: float):
        qkvr = qkvr.contiguous()
        nproj = qkvr.shape[1] // (H * a)
        xr = None if nproj == 4 else _unit_inner(xres)
        out, stats = hip.attention_core_fwd(qkvr, nproj, xr, T, H, a, scale)
        ctx.cfg = (nproj, T, H, a, scale)
        ctx.save_for_backward(qkvr, out, stats)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkvr, out, stats = ctx.saved_tensors
        nproj, T, H, a, scale = ctx.cfg
        dqkvr, dxres = hip.attention_core_bwd(qkvr, nproj, out, dout.contiguous(), stats, T, H, a, scale)
        return dqkvr, dxres, None, None, None, None


def field_attention_split(X, W, T: int, Din: int, H: int, a: int, has_res: bool, scale: float = 0.0):
    """Same layer as field_attention, split: ONE matrix-core GEMM for all projections of all B*T tokens
    (rp_linear_fwd; its dgrad / wgrad give dX and the weight gradients), then the T x T attention core per sample
    (rp_attention_core_*).  X [B, T, Din] -> [B, T, H*a]."""
    B = X.shape[0]
    x2 = X.reshape(B * T, Din)
    qkvr = linear_act(x2, W, None, ACT_NONE)                       # [B*T, (3|4)*H*a]
    out = _AttentionCore.apply(qkvr, None if has_res else x2, T, H, a, scale)
    return out.view(B, T, H * a)


class _AttentionWide(torch.autograd.Function):
    """The whole layer as ONE node, so that the two uses of its input (the projection GEMM and the residual) meet in a library
    launch (rp_add_rows) instead of autograd's ATen add: x2 [B*T, a] -> QKV (rp_linear_fwd on the stacked weights) -> the
    wide-head core (rp_attention_wide_fwd).  Saved: x2, W and the QKV the forward wrote; the backward recomputes the rest."""

    @staticmethod
    def forward(ctx, x2, W, T: int, a: int, scale: float, sum_tokens: bool):
        x2 = _unit_inner(x2)
        qkv = hip.linear_fwd(x2, _rows16(W), None, ACT_NONE, K=a)
        out = hip.attention_wide_fwd(qkv, x2, T, a, scale, sum_tokens)
        ctx.cfg = (T, a, scale, sum_tokens)
        ctx.save_for_backward(x2, W, qkv)
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, W, qkv = ctx.saved_tensors
        T, a, scale, sum_tokens = ctx.cfg
        dqkv, dxres = hip.attention_wide_bwd(qkv, x2, dout.contiguous(), T, a, scale, sum_tokens)
        dx = dW = None
        if ctx.needs_input_grad[0]:
            dx = hip.linear_fwd(dqkv, hip.transpose(W), None, ACT_NONE)  # [B*T, a]
            hip.add_rows_to(dxres, dx)                                     # + the residual's gradient
        if ctx.needs_input_grad[1]:
            dW, _ = hip.linear_wgrad(dqkv, x2, a, want_bias=False)
        return dx, dW, None, None, None, None


def attention_wide(X, W, T: int, a: int, scale: float = 0.0, sum_tokens: bool = False):
    """Self-attention over T <= 4 tokens with one head as wide as the input (no W_res), split form: X [B, T, a], W =
    stack_rows([Wq, Wk, Wv]) [3a, a] -> relu(softmax(Q K^T [/scale]) V + X) [B, T, a], or its sum over the tokens [B, a]
    (sum_tokens: AITM's torch.sum(ait, dim=1); the [B, T, a] tensor is then never written)."""
    B = X.shape[0]
    out = _AttentionWide.apply(X.reshape(B * T, a), W, T, a, float(scale), bool(sum_tokens))
    return out if sum_tokens else out.view(B, T, a)


class _FanOut(torch.autograd.Function):
    """x -> n aliases of it, one per consumer; the consumers' gradients are summed by library launches (rp_add_rows) instead of
    autograd's ATen adds, which would keep a recorded step from replaying as a launch plan.  2-D fp32 x (a shared tower input)."""

    @staticmethod
    def forward(ctx, x, n: int):
        x = _unit_inner(x)
        return tuple(x.detach() for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        total = _unit_inner(gs[0])
        for g in gs[1:]:
            hip.add_rows_to(_unit_inner(g), total)  # (in place: the first consumer's gradient buffer is this node's to keep)
        return total, None


def fan_out(x, n: int):
    return _FanOut.apply(x, n)


class _StackTokens(torch.autograd.Function):
    """n matrices [B, a] -> one [B, n, a] buffer (token i = matrix i), by rp_copy_rows into its row-strided slices: torch.cat of the
    unsqueezed matrices without the ATen launch; the gradients leave as the slices of the incoming one."""

    @staticmethod
    def forward(ctx, *xs):
        B, a = xs[0].shape
        out = torch.empty((B, len(xs), a), dtype=torch.float32, device=xs[0].device)
        for i, x in enumerate(xs):
            hip.copy_rows_to(_unit_inner(x), out[:, i, :])
        return out

    @staticmethod
    def backward(ctx, g):
        return tuple(g[:, i, :] for i in range(g.shape[1]))


def stack_tokens(xs):
    return _StackTokens.apply(*xs)


def field_attention(x, W, T: int, Din: int, H: int, a: int, has_res: bool, scale: float = 0.0):
    """x [B, >=T*Din] -> relu(attention + residual) [B, T, H*a];  W = cat(Wq, Wk, Wv[, Wres]) [(3|4)*H*a, Din]."""
    return _FieldAttention.apply(x, W, T, Din, H, a, has_res, scale)


# ----------------------------------------------------------------------------------------------
# K8  MMOE: one GEMM over [experts | gates] stored input-major ([h, N], as the reference keeps them),
#     then gate softmax + gate-weighted combine   — multi_task/mmoe.py:86-104
# ----------------------------------------------------------------------------------------------
class _LinearInputMajor(torch.autograd.Function):
    """z = x[:, :h] @ Wm + bias with Wm [h, N] (einsum 'ij,jk->ik' layout)."""

    @staticmethod
    def forward(ctx, x, Wm, bias):
        x = _unit_inner(x)
        Wm = Wm.contiguous()
        h = Wm.shape[0]
        z = hip.linear_fwd(x, hip.transpose(Wm), bias, ACT_NONE, K=h)
        ctx.h = h
        ctx.save_for_backward(x, Wm)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, Wm = ctx.saved_tensors
        dz = _unit_inner(dz)
        h, N = Wm.shape
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if x.shape[1] > h:  # zero rows appended to Wm: the GEMM writes the padding columns' zeros itself
                Wp = torch.empty((x.shape[1], Wm.shape[1]), dtype=Wm.dtype, device=Wm.device)
                Wp[:h].copy_(Wm)
                Wp[h:].zero_()
            else:
                Wp = Wm
            hip.linear_fwd(dz, Wp, None, ACT_NONE, out=dx)  # dz @ Wm^T
        if ctx.needs_input_grad[1]:
            dW, _ = hip.linear_wgrad(x[:, :h], dz, N, want_bias=False)  # roles swapped: x^T @ dz -> [h, N]
        if ctx.needs_input_grad[2]:
            # column sums of dz: the deterministic two-stage column-sum kernel (they rode on the wgrad kernel with K = 1 until
            # round 5: 0.137 ms at [65536, 520], 8x the time of streaming dz once)
            db = hip.batchnorm_colsum(dz)
        return dx, dW, db


class _MMOEProject(torch.autograd.Function):
    """z = x[:, :h] @ [experts | gate_1 | .. | gate_T] + [experts_bias | gate biases]  (multi_task/mmoe.py:86-104 as ONE GEMM)
    straight from the model's parameters: forward(x, pack, T, experts [h,K,E], experts_bias, *gates [h,E], *gate_biases [E]).
    `pack` [rows of x, N] is a persistent buffer of the model whose rows beyond h are zero (the dgrad's weight operand: it
    writes exact zeros into x's padding columns): the parameters are copied into their column blocks by rp_copy_rows /
    rp_multi_copy and their gradients leave as contiguous blocks the same way — torch.cat (x2), the padded copy and its
    zero fill, and autograd's strided-gradient clones were 6+ ATen launches per step."""

    @staticmethod
    def forward(ctx, x, pack, T: int, experts, experts_bias, *gw):
        x = _unit_inner(x)
        h, K, E = experts.shape
        gates, gbias = gw[:T], gw[T:]
        N = K * E + T * E
        hip.copy_rows_to(experts.detach().reshape(h, K * E), pack[:h, :K * E])
        for t in range(T):
            hip.copy_rows_to(gates[t].detach(), pack[:h, K * E + t * E:K * E + (t + 1) * E])
        bias = torch.empty((N,), dtype=torch.float32, device=x.device)
        dst = [bias[:K * E]] + [bias[K * E + t * E:K * E + (t + 1) * E] for t in range(T)]
        src = [experts_bias.detach().reshape(-1)] + [b.detach() for b in gbias]
        if not hip.multi_copy(dst, src):
            torch._foreach_copy_(dst, src)
        Wm = pack[:h]
        z = hip.linear_fwd(x, hip.transpose(Wm), bias, ACT_NONE, K=h)
        ctx.cfg = (h, K, E, T)
        ctx.save_for_backward(x, pack)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, pack = ctx.saved_tensors
        h, K, E, T = ctx.cfg
        dz = _unit_inner(dz)
        N = K * E + T * E
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            hip.linear_fwd(dz, pack, None, ACT_NONE, out=dx)  # dz @ Wm^T (the zero rows of pack give the padding columns of dx)
        need = ctx.needs_input_grad  # (x, pack, T, experts, experts_bias, gates.., gate biases..: the reference's gates are
        #                               plain tensors, not parameters — buffers here — and take no gradient)
        dexp, dgates = None, [None] * T
        if need[3] or any(need[5:5 + T]):
            dW, _ = hip.linear_wgrad(x[:, :h], dz, N, want_bias=False)  # roles swapped: x^T @ dz -> [h, N]
            if need[3]:
                dexp = hip.copy_rows_to(dW[:, :K * E], torch.empty((h, K * E), dtype=torch.float32, device=x.device)).view(h, K, E)
            for t in range(T):
                if need[5 + t]:
                    dgates[t] = hip.copy_rows_to(dW[:, K * E + t * E:K * E + (t + 1) * E],
                                                 torch.empty((h, E), dtype=torch.float32, device=x.device))
        dbe, dbias = None, [None] * T
        if need[4] or any(need[5 + T:5 + 2 * T]):
            db = hip.batchnorm_colsum(dz)
            dbe = db[:K * E].view(K, E) if need[4] else None
            dbias = [db[K * E + t * E:K * E + (t + 1) * E] if need[5 + T + t] else None for t in range(T)]
        return (dx, None, None, dexp, dbe, *dgates, *dbias)


def mmoe_project(x, pack, experts, experts_bias, gates, gate_biases):
    return _MMOEProject.apply(x, pack, len(gates), experts, experts_bias, *gates, *gate_biases)


def linear_input_major(x, Wm, bias):
    return _LinearInputMajor.apply(x, Wm, bias)


class _MMOECombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, K: int, E: int, T: int):
        z = _unit_inner(z)
        out, gate = hip.mmoe_combine_fwd(z, K, E, T)
        ctx.cfg = (K, E, T)
        ctx.save_for_backward(z, gate)
        ctx.set_materialize_grads(False)
        # T outputs, one per task (the rows of one [T, B, K] buffer): handed out as ONE tensor, the towers' slices came back
        # through autograd as T zero-filled [T, B, K] gradients plus their sum — 2T + 1 ATen launches over 67 MB each
        return tuple(out[t] for t in range(T))

    @staticmethod
    def backward(ctx, *douts):
        z, gate = ctx.saved_tensors
        K, E, T = ctx.cfg
        dout = torch.empty((T, z.shape[0], K), dtype=torch.float32, device=z.device)
        have = [t for t in range(T) if douts[t] is not None]
        for t in range(T):
            if douts[t] is None:
                dout[t].zero_()  # (a task whose mixture nobody used)
        if have and not hip.multi_copy([dout[t] for t in have], [douts[t].contiguous() for t in have]):
            torch._foreach_copy_([dout[t] for t in have], [douts[t] for t in have])
        dz = hip.mmoe_combine_bwd(z, K, E, T, gate, dout)
        if z.shape[1] != dz.shape[1]:
            full = torch.zeros_like(z)
            full[:, :dz.shape[1]] = dz
            dz = full
        return dz, None, None, None


def mmoe_combine(z, K: int, E: int, T: int):
    """z [B, K*E + T*E] (experts | gate logits) -> T gate-weighted expert mixtures [B, K] (the rows of one [T, B, K] buffer)."""
    return _MMOECombine.apply(z, K, E, T)


# ----------------------------------------------------------------------------------------------
# stand-alone FM pooling ([B,F,D] already materialised)   — layers/interaction.py:36-44
# ----------------------------------------------------------------------------------------------
class _FMPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, F: int, D: int, bi: bool):
        x2d = _unit_inner(x2d)
        out_sum, out_bi = hip.fm_pool_fwd(x2d, F, D, not bi, bi)
        ctx.cfg = (F, D, bi)
        ctx.save_for_backward(x2d)
        return out_bi if bi else out_sum

    @staticmethod
    def backward(ctx, g):
        (x2d,) = ctx.saved_tensors
        F, D, bi = ctx.cfg
        g = g.contiguous()
        return hip.fm_pool_bwd(x2d, F, D, None if bi else g, g if bi else None), None, None, None


def fm_pool(feature_emb, bi_interaction: bool = False):
    """feature_emb [B,F,D] (any row stride) -> product_sum_pooling [B,1] or Bi_interaction_pooling [B,D]."""
    B, F, D = feature_emb.shape
    return _FMPool.apply(feature_emb.reshape(B, F * D), F, D, bi_interaction)


# ----------------------------------------------------------------------------------------------
# K9  BatchNorm1d (MMOE towers)   — multi_task/mmoe.py:54
# ----------------------------------------------------------------------------------------------
class _BatchNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float):
        x = _unit_inner(x)
        y, mean, var, rstd = hip.batchnorm_train_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, mean, rstd, gamma)
        ctx.mark_non_differentiable(mean, var)
        ctx.set_materialize_grads(False)  # (the statistics' gradients were materialised as zero fills: 2 ATen launches per BN)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _gm, _gv):
        x, mean, rstd, gamma = ctx.saved_tensors
        if dy is None:
            return None, None, None, None
        dx, dgamma, dbeta = hip.batchnorm_train_bwd(x, _unit_inner(dy), mean, rstd, gamma)
        # (affine=False — Dice's BatchNorm — has neither: a gradient for a None input is an autograd error)
        return dx, (dgamma if gamma is not None else None), (dbeta if ctx.needs_input_grad[2] else None), None


class _BatchNormApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mean, rstd, gamma, beta):
        x = _unit_inner(x)
        ctx.save_for_backward(x, mean, rstd, gamma)
        return hip.batchnorm_apply(x, mean, rstd, gamma, beta)

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma = ctx.saved_tensors
        dy = _unit_inner(dy)
        dx = hip.batchnorm_apply_bwd(dy, rstd, gamma)
        dgamma = dbeta = None
        if gamma is not None and ctx.needs_input_grad[3]:
            dgamma = (dy * ((x - mean) * rstd)).sum(dim=0)  # eval-mode fine-tuning is off the hot path
        if ctx.needs_input_grad[4]:
            dbeta = dy.sum(dim=0)
        return dx, None, None, dgamma, dbeta


def batch_norm(x, bn: torch.nn.BatchNorm1d):
    """nn.BatchNorm1d semantics on the HIP kernels, including the running-statistics update in training mode."""
    use_batch = bn.training or not bn.track_running_stats or bn.running_mean is None
    if use_batch and type(bn) is not torch.nn.BatchNorm1d:
        return bn(x)  # sharded.SyncBatchNorm1d: global-batch statistics (torch ops + one all-reduce each way)
    if use_batch:
        y, mean, var = _BatchNormTrain.apply(x, bn.weight, bn.bias, bn.eps)
        if bn.training and bn.track_running_stats and bn.running_mean is not None:
            # one launch (six ATen launches per BatchNorm until round 5: 24 per MMOE step); in place, like nn.BatchNorm1d
            hip.batchnorm_update_running(mean, var, bn, x.shape[0])
        return y
    rstd = torch.rsqrt(bn.running_var + bn.eps)
    return _BatchNormApply.apply(x, bn.running_mean, rstd, bn.weight, bn.bias)


# ----------------------------------------------------------------------------------------------
# Dice   — layers/activation.py:10-34:  p = sigmoid(bn(x)),  y = p x + (1 - p) alpha x
# ----------------------------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    """nn.LayerNorm over the last dimension of a 2-D x, optionally times `mul` (rp_layernorm_fwd / _bwd)"""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float, mul):
        x = _unit_inner(x)
        mul = _unit_inner(mul) if mul is not None else None
        y, stats = hip.layernorm_fwd(x, gamma, beta, eps, mul=mul)
        ctx.save_for_backward(x, gamma, beta, mul, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mul, stats = ctx.saved_tensors
        dx, dmul, dg, db = hip.layernorm_bwd(_unit_inner(dy), x, stats, gamma, beta, mul=mul)
        return dx, dg, db, None, dmul


def layer_norm(x, ln: torch.nn.LayerNorm, mul=None):
    """ln(x) [* mul] for an affine nn.LayerNorm over the last dimension, as one launch each way; with `mul` (same shape as
    x) the product is formed inside the launch and the normalised tensor is never stored."""
    N = x.shape[-1]
    if tuple(ln.normalized_shape) != (N,) or ln.weight is None or ln.bias is None:
        raise RuntimeError(f"layer_norm: an affine LayerNorm over the last dimension ({N}), got {ln}")
    if mul is not None and mul.shape != x.shape:
        raise RuntimeError(f"layer_norm: mul {tuple(mul.shape)} against x {tuple(x.shape)}")
    y = _LayerNorm.apply(x.reshape(-1, N), ln.weight, ln.bias, float(ln.eps), mul.reshape(-1, N) if mul is not None else None)
    return y.reshape(x.shape)


class _MaskBlockStack(torch.autograd.Function):
    """MaskNet's whole stack of MaskBlocks (ranking/masknet.py:70-79 over layers/interaction.py:279-283) on one autograd node.
        block_k(net, x) = LN_out_k(Wh_k (LN_in_k(net) * (W2_k relu(W1_k x + c1_k) + c2_k)) + ch_k)
        parallel: v = mean_k block_k(x, x);   serial: v_0 = x, v_{k+1} = block_k(v_k, x), v = v_K
    x [B, W] (d = the blocks' width, columns beyond d are padding); params: per block (LN_in weight, bias, W1, c1, W2, c2, Wh,
    ch, LN_out weight, bias).  Returns v [B, ceil4(W)] with zeros beyond d.  Per block the forward is 5 launches (Linear+ReLU,
    Linear, LN_in * mask, Linear, LN_out — in parallel mode LN_out adds 1/K of its result into v, so the mean needs no launch)
    and keeps h = relu(.), the mask m, the hidden pre-norm z and the row statistics; LN_in(net) * m is recomputed in the
    backward.  x feeds every block's mask layer and (parallel) every LN_in: those gradients are summed here, in block
    order, by the LayerNorm backward's accumulate flag and rp_accumulate — autograd sees ONE gradient of x."""

    @staticmethod
    def forward(ctx, x, parallel: bool, eps_in, eps_out, *params):
        x = _unit_inner(x)
        nb = len(params) // 10
        d, agg = params[0].numel(), params[2].shape[0]
        B, dev = x.shape[0], x.device
        Wx, ag4 = (max(x.shape[1], d) + 3) // 4 * 4, (agg + 3) // 4 * 4

        def buf(w=Wx):
            return torch.empty((B, w), dtype=torch.float32, device=dev)

        v, net, st_in, kept = buf(), x, None, []
        for k in range(nb):
            g_in, b_in, W1, c1, W2, c2, Wh, ch, g_o, b_o = params[10 * k:10 * k + 10]
            h = buf(ag4)[:, :agg]
            hip.linear_fwd(x, _rows16(W1), c1, ACT_RELU, K=d, out=h)
            m = buf()
            hip.linear_fwd(h, _rows16(W2), c2, ACT_NONE, K=agg, out=m[:, :d])
            shared = parallel and k > 0  # every parallel block normalises the same x: one set of statistics
            nm, st_in = hip.layernorm_fwd(net, g_in, b_in, eps_in[k], mul=m, out=buf(), stats=st_in if shared else None,
                                          stats_given=shared)
            z = buf()
            hip.linear_fwd(nm, _rows16(Wh), ch, ACT_NONE, K=d, out=z[:, :d])
            if parallel:
                _, st_o = hip.layernorm_fwd(z, g_o, b_o, eps_out[k], out=v, out_scale=1.0 / nb, accumulate=k > 0)
                kept += [h, m, z, st_o]
            else:
                nxt = v if k == nb - 1 else buf()
                _, st_o = hip.layernorm_fwd(z, g_o, b_o, eps_out[k], out=nxt)
                kept += [h, m, z, st_o, net, st_in]
                net = nxt
        if parallel:
            kept.append(st_in)
        ctx.parallel, ctx.nb, ctx.eps_in, ctx.Wx = parallel, nb, eps_in, Wx
        ctx.save_for_backward(x, *params, *kept)
        return v

    @staticmethod
    def backward(ctx, dv):
        parallel, nb, Wx = ctx.parallel, ctx.nb, ctx.Wx
        saved = ctx.saved_tensors
        x, params, kept = saved[0], saved[1:1 + 10 * nb], saved[1 + 10 * nb:]
        d, agg = params[0].numel(), params[2].shape[0]
        B, dev = x.shape[0], x.device
        ag4 = (agg + 3) // 4 * 4
        grads = [None] * (10 * nb)
        g, dx = _unit_inner(dv), None
        per = 4 if parallel else 6
        for k in (range(nb) if parallel else reversed(range(nb))):
            g_in, b_in, W1, c1, W2, c2, Wh, ch, g_o, b_o = params[10 * k:10 * k + 10]
            h, m, z, st_o = kept[per * k:per * k + 4]
            net, st_in = (x, kept[-1]) if parallel else kept[per * k + 4:per * k + 6]
            dz, _, dgo, dbo = hip.layernorm_bwd(g, z, st_o, g_o, b_o, dy_scale=1.0 / nb if parallel else 1.0)
            nm, _ = hip.layernorm_fwd(net, g_in, b_in, ctx.eps_in[k], mul=m, stats=st_in, stats_given=True,
                                      out=torch.empty((B, Wx), dtype=torch.float32, device=dev))
            dWh, dch = hip.linear_wgrad(dz[:, :d], nm, d)
            dnm = hip.linear_fwd(dz, hip.transpose(Wh, rows_out=Wx), None, ACT_NONE)
            if parallel or k == 0:  # LN_in normalised x itself: its gradient joins the others' in dx
                dx, dm, dgi, dbi = hip.layernorm_bwd(dnm, net, st_in, g_in, b_in, mul=m, dx=dx, accumulate=dx is not None)
            else:
                g, dm, dgi, dbi = hip.layernorm_bwd(dnm, net, st_in, g_in, b_in, mul=m)
            dW2, dc2 = hip.linear_wgrad(dm[:, :d], h, agg)
            dh = torch.empty((B, ag4), dtype=torch.float32, device=dev)[:, :agg]
            hip.linear_fwd(dm, hip.transpose(W2), None, ACT_MASK, aux=h, out=dh)
            dW1, dc1 = hip.linear_wgrad(dh, x, d)
            dxm = hip.linear_fwd(dh, hip.transpose(W1, rows_out=x.shape[1]), None, ACT_NONE)
            dx = dxm if dx is None else hip.accumulate(dx, dxm)
            grads[10 * k:10 * k + 10] = [dgi, dbi, dW1, dc1, dW2, dc2, dWh, dch, dgo, dbo]
        return (dx if ctx.needs_input_grad[0] else None, None, None, None, *grads)


def mask_block_stack(x, blocks, parallel: bool):
    """the stack of MaskBlock modules `blocks` applied to the padded row buffer x (see _MaskBlockStack); -> [B, ceil4(W)]"""
    params = []
    for b in blocks:
        params += [b._input_layer_norm.weight, b._input_layer_norm.bias, b._mask_layer[0].weight, b._mask_layer[0].bias,
                   b._mask_layer[2].weight, b._mask_layer[2].bias, b._hidden_layer.weight, b._hidden_layer.bias,
                   b._layer_norm.weight, b._layer_norm.bias]
    eps_in = tuple(float(b._input_layer_norm.eps) for b in blocks)
    eps_out = tuple(float(b._layer_norm.eps) for b in blocks)
    return _MaskBlockStack.apply(x, bool(parallel), eps_in, eps_out, *params)


class _GINStack(torch.autograd.Function):
    """AOANet's whole GeneralizedInteractionNet (ranking/aoanet.py:81-115) on one autograd node:
        B_0 = x0,  B_{i+1} = layer_i(x0, B_i)   with layer_i the factorised contraction of rp_gin_fwd
    x0 [B, >= F D] with any row stride (the embedding block of the gather's row buffer); params: (W, alpha, h) per layer.
    Returns B_L [B, O D].  The forward is one launch per layer and keeps the layer outputs ([B, O D] each); T and U are
    rebuilt inside the backward launches.  x0 feeds every layer (layer 0 twice): those gradients are summed into ONE buffer
    by the kernel's accumulate flag, in reverse layer order — autograd sees one gradient of x0."""

    @staticmethod
    def forward(ctx, x0, F: int, D: int, *params):
        x0 = _unit_inner(x0)
        nl = len(params) // 3
        outs, bi = [], x0
        for i in range(nl):
            W, alpha, h = params[3 * i:3 * i + 3]
            bi = hip.gin_fwd(x0, bi, W, alpha, h, F)
            outs.append(bi)
        ctx.F, ctx.D, ctx.nl = F, D, nl
        ctx.save_for_backward(x0, *params, *outs[:-1])
        return outs[-1]

    @staticmethod
    def backward(ctx, dout):
        F, D, nl = ctx.F, ctx.D, ctx.nl
        saved = ctx.saved_tensors
        x0, params, outs = saved[0], saved[1:1 + 3 * nl], saved[1 + 3 * nl:]
        dx0 = _wide_rows_grad(x0, F * D)
        if dx0 is None:  # (rp_gin_bwd takes its dx0 from the caller either way)
            dx0 = torch.empty(tuple(x0.shape), dtype=torch.float32, device=x0.device)
        grads = [None] * (3 * nl)
        g = _unit_inner(dout)
        for i in reversed(range(nl)):
            W, alpha, h = params[3 * i:3 * i + 3]
            g, dW, dalpha, dh = hip.gin_bwd(g, x0, x0 if i == 0 else outs[i - 1], W, alpha, h, F, dx0,
                                            accumulate=i < nl - 1, bi_is_x0=i == 0)
            grads[3 * i:3 * i + 3] = [dW, dalpha, dh]
        return (dx0 if ctx.needs_input_grad[0] else None, None, None, *grads)


def gin_stack(x0_rows, F: int, D: int, layers):
    """the GeneralizedInteraction modules `layers` (the first over F input subspaces: B_0 in both roles) applied to the rows
    x0_rows [B, >= F D] (see _GINStack); -> [B, O D] of the last layer.  Every layer must satisfy hip.gin_fits."""
    params = []
    for i, l in enumerate(layers):
        P, O = l.input_subspaces, l.W.shape[0]
        if (i == 0 and P != F) or l.num_fields != F or l.embedding_dim != D or not hip.gin_fits(F, P, O, D):
            raise RuntimeError(f"gin_stack: layer {i} (F={l.num_fields}, P={P}, O={O}, D={l.embedding_dim}) over {F} fields of "
                               f"width {D}: no kernel form (hip.gin_fits)")
        params += [l.W, l.alpha, l.h]
    return _GINStack.apply(x0_rows, F, D, *params)


class _CCPMStack(torch.autograd.Function):
    """CCPM's whole conv stack (ranking/ccpm.py:77-107: [ZeroPad2d -> Conv2d (kh, 1) -> KMaxPooling -> Tanh] x L) on one
    autograd node, one launch each way.  x [B, >= F D] with any row stride (the gather's row buffer, read in place); params:
    every layer's conv weight, then every bias.  Returns [B, C_last k_last D] laid out as flatten(conv_out, 1).  Nothing but
    x and the parameters is saved: rp_ccpm_bwd rebuilds the activations and the selections per column."""

    @staticmethod
    def forward(ctx, x, F: int, D: int, ks, *params):
        x = _unit_inner(x)
        nl = len(params) // 2
        weights, biases = [w.contiguous() for w in params[:nl]], list(params[nl:])
        ctx.F, ctx.D, ctx.ks, ctx.nl = F, D, ks, nl
        ctx.save_for_backward(x, *weights, *biases)
        return hip.ccpm_fwd(x, weights, biases, F, D, ks)

    @staticmethod
    def backward(ctx, dout):
        F, D, nl = ctx.F, ctx.D, ctx.nl
        saved = ctx.saved_tensors
        x, weights, biases = saved[0], list(saved[1:1 + nl]), list(saved[1 + nl:])
        dx, dWs, dbs = hip.ccpm_bwd(_unit_inner(dout), x, weights, biases, F, D, ctx.ks, dx=_wide_rows_grad(x, F * D))
        return (dx if ctx.needs_input_grad[0] else None, None, None, None, *dWs, *dbs)


def ccpm_conv_stack(rows, F: int, D: int, conv_layer):
    """the CCPM_ConvLayer `conv_layer` applied to the rows [B, >= F D] (see _CCPMStack) -> [B, C_last k_last D].  The stack
    must satisfy hip.ccpm_fits (conv_layer.hip_supported)."""
    convs, ks = conv_layer.convs(), tuple(conv_layer.ks)
    channels, heights = [c.out_channels for c in convs], [c.kernel_size[0] for c in convs]
    if conv_layer.num_fields != F or not hip.ccpm_fits(F, D, channels, heights, ks):
        raise RuntimeError(f"ccpm_conv_stack: channels {channels}, heights {heights}, ks {list(ks)} over {F} fields of width "
                           f"{D}: no kernel form (hip.ccpm_fits)")
    return _CCPMStack.apply(rows, F, D, ks, *[c.weight for c in convs], *[c.bias for c in convs])


class _SenetBilinear(torch.autograd.Function):
    """FiBiNet's SENET + both bilinear branches + the cat with the dense columns (ranking/fibinet.py:60-67) on one autograd
    node: rows [B, >= F D + n_dense] with any row stride (the gather's row buffer, read in place) -> the MLP's input
    [B, ld] = T(E) | A_i A_j T(E) | dense | padding (not written).  params: W1, W2 of the SENET when R > 0, then the [D, D]
    matrices.  Nothing but the rows and the parameters is saved: rp_bilinear_bwd rebuilds A, U and T."""

    @staticmethod
    def forward(ctx, rows, F: int, D: int, R: int, btype: int, n_dense: int, ld: int, *params):
        rows = _unit_inner(rows)
        params = [p.contiguous() for p in params]
        senet, weights = (tuple(params[:2]), params[2:]) if R > 0 else (None, params)
        ctx.geom = (F, D, R, btype, n_dense)
        ctx.save_for_backward(rows, *params)
        out = hip._new((rows.shape[0], ld), torch.float32, rows.device)
        return hip.bilinear_fwd(rows, F, D, weights, btype, senet, n_dense, out=out)

    @staticmethod
    def backward(ctx, dout):
        F, D, R, btype, n_dense = ctx.geom
        rows, params = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        senet, weights = (tuple(params[:2]), params[2:]) if R > 0 else (None, params)
        dx, dW, dW1, dW2 = hip.bilinear_bwd(_unit_inner(dout), rows, F, D, weights, btype, senet, n_dense,
                                            dx=_wide_rows_grad(rows, F * D))
        # field_each: the last field opens no pair, its matrix takes no part (the reference leaves its .grad None)
        used = len(weights) - 1 if btype == hip.BILINEAR_TYPES["field_each"] else len(weights)
        grads = [dW[k] if k < used else None for k in range(len(weights))]
        return (dx if ctx.needs_input_grad[0] else None, None, None, None, None, None, None,
                *((dW1, dW2) if R > 0 else ()), *grads)


def senet_bilinear(rows, F: int, D: int, senet, bilinear, dense: int = 0, pad_to: int = 64):
    """the MLP input of FiBiNet from the rows [B, >= F D + dense] of the gather (embedding columns, then `dense` dense
    columns): bilinear(E) | bilinear(senet(E)) | dense, as [B, ld] with ld the width rounded up to pad_to (the padding
    columns are not written; the Linear that follows reads its in_features columns).  senet: a SENET_Layer or None (one
    branch); bilinear: a BilinearInteractionLayer.  The shape must satisfy hip.bilinear_fits."""
    btype = hip.BILINEAR_TYPES.get(bilinear.bilinear_type, -1)
    R = 0 if senet is None else senet.excitation[0].weight.shape[0]
    if not hip.bilinear_fits(F, D, R, btype):
        raise RuntimeError(f"senet_bilinear: {F} fields of width {D}, {R} SENET units, {bilinear.bilinear_type!r}: no kernel "
                           "form (hip.bilinear_fits)")
    width = (2 if R else 1) * (F * (F - 1) // 2) * D + dense
    ld = padded(width, pad_to)
    params = [] if senet is None else [senet.excitation[0].weight, senet.excitation[2].weight]
    return _SenetBilinear.apply(rows, F, D, R, btype, dense, ld, *params, *bilinear.weights())


class _LogarithmicNet(torch.autograd.Function):
    """AFN's logarithmic transformation layer with both BatchNorms (ranking/afn.py:93-102) on one autograd node: rows
    [B, >= F D] with any row stride (the gather's row buffer, read in place) -> the MLP's input [B, ld], L D columns written.
    stats: () with batch statistics — the node then also returns them (mean1, var1 [F], mean2, var2 [L], biased, not
    differentiable) for the running buffers — or the four running vectors.  Saved: the rows, z [B, L D], the statistics and the
    parameters; rp_lognet_bwd rebuilds y from the rows and c from z."""

    @staticmethod
    def forward(ctx, rows, F: int, D: int, ld: int, eps1: float, eps2: float, W, g1, b1, g2, b2, *stats):
        rows = _unit_inner(rows)
        W, g1, b1, g2, b2 = (t.contiguous() for t in (W, g1, b1, g2, b2))
        train = len(stats) == 0
        L, dev = W.shape[0], rows.device
        if train:
            stats = (hip._new((F,), torch.float32, dev), hip._new((F,), torch.float32, dev),
                     hip._new((L,), torch.float32, dev), hip._new((L,), torch.float32, dev))
        m1, v1, m2, v2 = stats
        out = hip._new((rows.shape[0], ld), torch.float32, dev)
        out, z = hip.lognet_fwd(rows, F, D, W, g1, b1, m1, v1, eps1, g2, b2, m2, v2, eps2, train, out)
        ctx.geom = (F, D, eps1, eps2, train)
        ctx.save_for_backward(rows, z, W, g1, b1, g2, m1, v1, m2, v2)
        if not train:
            return out
        ctx.mark_non_differentiable(m1, v1, m2, v2)
        ctx.set_materialize_grads(False)
        return out, m1, v1, m2, v2

    @staticmethod
    def backward(ctx, dout, *_):
        F, D, eps1, eps2, train = ctx.geom
        rows, z, W, g1, b1, g2, m1, v1, m2, v2 = ctx.saved_tensors
        if dout is None:
            return (None,) * (11 + (0 if train else 4))
        dx, dW, dg1, db1, dg2, db2 = hip.lognet_bwd(_unit_inner(dout), rows, z, F, D, W, g1, b1, m1, v1, eps1, g2, m2, v2, eps2,
                                                    train, dx=_wide_rows_grad(rows, F * D))
        return (dx if ctx.needs_input_grad[0] else None, None, None, None, None, None, dW, dg1, db1, dg2, db2,
                *(() if train else (None,) * 4))


def logarithmic_net(rows, F: int, D: int, coefficient_W, log_bn, exp_bn, pad_to: int = 64):
    """the input of AFN's dense_layer from the rows [B, >= F D] of the gather: exp_bn(exp(coefficient_W log_bn(log max(|E|,
    1e-5)))) flattened, as [B, ld] with ld = L D rounded up to pad_to (the padding columns are not written; the Linear that
    follows reads its in_features columns).  coefficient_W: the bias-free Linear(F, L); log_bn / exp_bn: affine
    nn.BatchNorm1d(F) / (L), whose running statistics are updated in training mode exactly like nn.BatchNorm1d's (the count
    is B D).  The shape must satisfy hip.lognet_fits."""
    W = coefficient_W.weight
    L = W.shape[0]
    if coefficient_W.bias is not None or W.shape[1] != F or not hip.lognet_fits(F, D, L):
        raise RuntimeError(f"logarithmic_net: {F} fields of width {D}, {L} neurons (bias: {coefficient_W.bias is not None}): "
                           "no kernel form (hip.lognet_fits)")
    for bn, n in ((log_bn, F), (exp_bn, L)):
        if type(bn) is not torch.nn.BatchNorm1d or bn.weight is None or bn.bias is None or bn.num_features != n:
            raise RuntimeError(f"logarithmic_net: an affine nn.BatchNorm1d({n}), got {bn}")
    batch = [bn.training or not bn.track_running_stats or bn.running_mean is None for bn in (log_bn, exp_bn)]
    if batch[0] != batch[1]:
        raise RuntimeError("logarithmic_net: one BatchNorm on batch statistics and one on running statistics")
    ld = padded(L * D, pad_to)
    head = (rows, F, D, ld, float(log_bn.eps), float(exp_bn.eps), W, log_bn.weight, log_bn.bias, exp_bn.weight, exp_bn.bias)
    if not batch[0]:
        return _LogarithmicNet.apply(*head, log_bn.running_mean, log_bn.running_var, exp_bn.running_mean, exp_bn.running_var)
    out, m1, v1, m2, v2 = _LogarithmicNet.apply(*head)
    M = rows.shape[0] * D
    for bn, m, v in ((log_bn, m1, v1), (exp_bn, m2, v2)):
        if bn.training and bn.track_running_stats and bn.running_mean is not None:
            hip.batchnorm_update_running(m, v, bn, M)
    return out


class _PairFC(torch.autograd.Function):
    """AFN's ensemble head fc(cat[a, d]) for a Linear(2, 1) (ranking/afn.py:81) without the cat: rp_pair_fc_*"""

    @staticmethod
    def forward(ctx, a, d, w, bias):
        a, d, w = a.contiguous(), d.contiguous(), w.contiguous()
        ctx.save_for_backward(a, d, w)
        return hip.pair_fc_fwd(a, d, w, bias)

    @staticmethod
    def backward(ctx, dz):
        a, d, w = ctx.saved_tensors
        da, dd, dw, db = hip.pair_fc_bwd(dz.contiguous(), a, d, w)
        return da.view(a.shape), dd.view(d.shape), dw, db


def pair_fc(a, d, fc: torch.nn.Linear):
    """fc(cat[a, d], dim=-1) for a, d [B, 1] and fc = nn.Linear(2, 1), as one launch each way plus the sums' finish"""
    return _PairFC.apply(a, d, fc.weight, fc.bias)


class _DiceGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, xhat, alpha):
        x, xhat = _unit_inner(x), _unit_inner(xhat)
        alpha = alpha.contiguous()
        ctx.save_for_backward(x, xhat, alpha)
        return hip.dice_gate_fwd(x, xhat, alpha)

    @staticmethod
    def backward(ctx, dy):
        x, xhat, alpha = ctx.saved_tensors
        dxd, dxh, dal = hip.dice_gate_bwd(x, xhat, alpha, _unit_inner(dy))
        dalpha = hip.batchnorm_colsum(dal) if ctx.needs_input_grad[2] else None  # deterministic two-stage column sums
        return dxd, dxh, dalpha


def dice(x, bn: torch.nn.BatchNorm1d, alpha):
    """Dice on the HIP kernels for 2-D x [M, N]: batch_norm (rp_batchnorm_*, running statistics updated in training
    mode exactly like nn.BatchNorm1d) + the gate (rp_dice_gate_*)."""
    return _DiceGate.apply(x, batch_norm(x, bn), alpha)


# ----------------------------------------------------------------------------------------------
# Dropout (training mode, p > 0)   — layers/deep.py:66-68, the multi-task towers
# ----------------------------------------------------------------------------------------------
class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p: float):
        x = _unit_inner(x)
        y, mask = hip.dropout_fwd(x, p)
        ctx.p = p
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return hip.dropout_bwd(_unit_inner(dy), mask, ctx.p), None


def dropout(x, p: float):
    """y = x * keep / (1 - p) on the HIP kernel (rp_dropout_*); x is [..., N], any leading shape."""
    if x.dim() == 2:
        return _Dropout.apply(x, float(p))
    lead = x.shape[:-1]
    return _Dropout.apply(x.reshape(-1, x.shape[-1]), float(p)).reshape(*lead, x.shape[-1])


# ----------------------------------------------------------------------------------------------
# K10  sum of logits -> sigmoid -> BCE(mean)   — ranking/deepfm.py:61-63, multi_task/mmoe.py:127
# ----------------------------------------------------------------------------------------------
class _SigmoidBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, label, apply_sigmoid: bool, p_eps: float, weight: float, *addends):
        ctx.set_materialize_grads(False)  # `pred` is normally not differentiated: no zero dpred, no dead arithmetic
        adds = [a.contiguous() for a in addends]
        label = label.contiguous()
        pred, loss = hip.sigmoid_bce_fwd(adds, label, apply_sigmoid, p_eps, weight)
        ctx.cfg = (apply_sigmoid, p_eps, weight, len(adds), [tuple(a.shape) for a in addends])
        ctx.save_for_backward(pred, label)
        return pred, loss

    @staticmethod
    def backward(ctx, dpred, dloss):
        pred, label = ctx.saved_tensors
        apply_sigmoid, p_eps, weight, n, shapes = ctx.cfg
        dz = None
        if dloss is not None:
            dz = hip.sigmoid_bce_bwd(pred, label, dloss, apply_sigmoid, p_eps, weight)
        if dpred is not None:  # someone differentiated through `pred` itself (rare): torch ops on device
            extra = dpred * (pred * (1 - pred) if apply_sigmoid else 1.0)
            dz = extra if dz is None else dz + extra
        outs = [None if dz is None else dz.reshape(s) for s in shapes]
        return (None, None, None, None, *outs)


def sigmoid_bce(addends: Sequence[torch.Tensor], label: torch.Tensor, apply_sigmoid=True, p_eps=0.0, weight=1.0):
    """pred [B,1] = sigmoid(sum(addends)); loss = weight * mean BCE(pred + p_eps, label)."""
    return _SigmoidBCE.apply(label, apply_sigmoid, p_eps, weight, *addends)


class _SigmoidBCEMulti(torch.autograd.Function):
    """The multi-task loss (multi_task/mmoe.py:127, towers.py): forward(T, apply_sigmoid, p_eps, weights, *labels, *logits) ->
    (pred_1 .. pred_T, loss) with loss = sum_i weights[i] * mean BCE(pred_i + p_eps, label_i): every task's launch adds its
    term to ONE device scalar, in task order — the fp32 additions of the reference's python sum without its ATen launches."""

    @staticmethod
    def forward(ctx, T: int, apply_sigmoid: bool, p_eps: float, weights, *rest):
        ctx.set_materialize_grads(False)
        labels = [t.contiguous() for t in rest[:T]]
        logits = [t.contiguous() for t in rest[T:]]
        preds, loss = [], None
        for i in range(T):
            pred, loss = hip.sigmoid_bce_fwd([logits[i]], labels[i], apply_sigmoid, p_eps, float(weights[i]), add_to=loss)
            preds.append(pred)
        ctx.cfg = (T, apply_sigmoid, p_eps, [float(w) for w in weights], [tuple(t.shape) for t in rest[T:]])
        ctx.save_for_backward(*preds, *labels)
        return (*preds, loss)

    @staticmethod
    def backward(ctx, *grads):
        T, apply_sigmoid, p_eps, weights, shapes = ctx.cfg
        saved = ctx.saved_tensors
        preds, labels = saved[:T], saved[T:]
        dloss = grads[T]
        outs = []
        for i in range(T):
            dz = None
            if dloss is not None:
                dz = hip.sigmoid_bce_bwd(preds[i], labels[i], dloss, apply_sigmoid, p_eps, weights[i])
            if grads[i] is not None:  # someone differentiated through a prediction itself (rare): torch ops on device
                extra = grads[i] * (preds[i] * (1 - preds[i]) if apply_sigmoid else 1.0)
                dz = extra if dz is None else dz + extra
            outs.append(None if dz is None else dz.reshape(shapes[i]))
        return (None, None, None, None) + (None,) * T + tuple(outs)


def sigmoid_bce_multi(logits: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], weights, apply_sigmoid=True, p_eps=0.0):
    """([pred_i [B,1]], loss) with loss = sum_i weights[i] * mean BCE(sigmoid(logits[i]) + p_eps, labels[i])"""
    T = len(logits)
    out = _SigmoidBCEMulti.apply(T, apply_sigmoid, float(p_eps), tuple(float(w) for w in weights), *labels, *logits)
    return list(out[:T]), out[T]


class _PairLoss(torch.autograd.Function):
    """The two-task loss heads that couple the tasks (rp_pair_loss_*): ESSM's BCE(p1 p2, y2) + w BCE(p1, y1) and AITM's
    BCE(p1, y1) + BCE(p2, y2) + c sum max(p2 - p1, 0), the sigmoids included when the inputs are logits."""

    @staticmethod
    def forward(ctx, z1, z2, y1, y2, mode: int, coef: float, apply_sigmoid: bool):
        ctx.set_materialize_grads(False)  # the predictions are normally not differentiated
        y1, y2 = y1.reshape(-1).contiguous(), y2.reshape(-1).contiguous()
        p1, p2, loss = hip.pair_loss_fwd(z1.reshape(-1).contiguous(), z2.reshape(-1).contiguous(), y1, y2, mode, coef,
                                         apply_sigmoid)
        ctx.cfg = (mode, coef, apply_sigmoid, tuple(z1.shape), tuple(z2.shape))
        ctx.save_for_backward(p1, p2, y1, y2)
        return p1.view(z1.shape), p2.view(z2.shape), loss

    @staticmethod
    def backward(ctx, dp1, dp2, dloss):
        p1, p2, y1, y2 = ctx.saved_tensors
        mode, coef, apply_sigmoid, s1, s2 = ctx.cfg
        dz1 = dz2 = None
        if dloss is not None:
            dz1, dz2 = hip.pair_loss_bwd(p1, p2, y1, y2, dloss, mode, coef, apply_sigmoid)
        for k, (dp, p) in enumerate(((dp1, p1), (dp2, p2))):
            if dp is not None:  # someone differentiated through a prediction itself (rare): torch ops on device
                extra = dp.reshape(-1) * (p * (1 - p) if apply_sigmoid else 1.0)
                if k == 0:
                    dz1 = extra if dz1 is None else dz1 + extra
                else:
                    dz2 = extra if dz2 is None else dz2 + extra
        return (None if dz1 is None else dz1.view(s1), None if dz2 is None else dz2.view(s2), None, None, None, None, None)


def pair_loss(z1, z2, y1, y2, mode: int, coef: float, apply_sigmoid: bool = True):
    """(p1, p2, loss): p = sigmoid(z) (apply_sigmoid) or z, shaped like z1 / z2; mode hip.PAIR_ESSM: loss = BCE(p1 p2, y2) +
    coef BCE(p1, y1); hip.PAIR_AITM: loss = BCE(p1, y1) + BCE(p2, y2) + coef sum_b max(p2 - p1, 0)"""
    return _PairLoss.apply(z1, z2, y1, y2, int(mode), float(coef), bool(apply_sigmoid))


class _SigmoidSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *addends):
        pred, _ = hip.sigmoid_bce_fwd([a.contiguous() for a in addends], None, True)
        ctx.shapes = [tuple(a.shape) for a in addends]
        ctx.save_for_backward(pred)
        return pred

    @staticmethod
    def backward(ctx, dpred):
        (pred,) = ctx.saved_tensors
        dz = dpred * pred * (1 - pred)
        return tuple(dz.reshape(s) for s in ctx.shapes)


def sigmoid_sum(addends: Sequence[torch.Tensor]):
    return _SigmoidSum.apply(*addends)


# ----------------------------------------------------------------------------------------------
# K1/K2/K3  multi-table gather (+dense concat, +FM)   — layers/embedding.py:59-63 etc.
# `store` is the arena-backed EmbeddingLayer; its per-table Parameters are passed only so that the
# node is connected to the graph: their gradients are written by the kernel straight into the
# layer's dense gradient arena (exposed as each Parameter's .grad), not returned through autograd.
# ----------------------------------------------------------------------------------------------
class _EmbedGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, store, idx: List[torch.Tensor], dense: List[torch.Tensor], ldx: int, want_fm: bool, meta,
                *tables):
        need_grad = any(ctx.needs_input_grad[6:])
        pre = store._presorted  # the batch's SortedLookup where the lazy-Adam replay (or another layer) already sorted it
        store._presorted = None
        row_base, row_count = meta if meta is not None else (store.row_base, store.row_count)
        x, fm, ssum, keys = hip.embed_gather_fwd(store.arena, row_base, row_count, idx, dense, ldx,
                                                 want_fm, want_fm and need_grad, need_grad and pre is None,
                                                 store.err_flag)
        ctx.store, ctx.want_fm, ctx.B = store, want_fm, idx[0].shape[0]
        # link to the first Linear that consumes x (DeepFM passes it on as `fm_link`): FM fold / fused dgrad
        ctx.link = store._fm_link = FMFold(ssum, len(idx) * store.embedding_dim, store.embedding_dim) \
            if (need_grad and meta is None) else None
        ctx.presorted = pre if need_grad else None
        if pre is not None:
            keys = pre.keys if need_grad else None
        ctx.save_for_backward(keys, ssum)
        if want_fm:
            return x, fm
        return x

    @staticmethod
    def backward(ctx, dx, dfm=None):
        keys, ssum = ctx.saved_tensors
        store = ctx.store
        fused = None
        if ctx.link is not None and ctx.link.dgrad is not None:
            fused, ctx.link.dgrad = ctx.link.dgrad, None
            ctx.link.fused = True
            if dx is not None and dx.dim() == 2 and dx.stride(0) == 0 and dx.stride(1) == 0:
                dx = None  # the placeholder of the fused Linear: no other consumer of x contributed
        if dx is not None:
            dx = _unit_inner(dx)
        if ctx.link is not None and ctx.link.extra is not None:
            extra, ctx.link.extra = ctx.link.extra, None
            if fused is not None and dx is None and extra.shape[1] == len(store.emb_feature) * store.embedding_dim:
                # the first Linear left its dgrad to this backward (rp_embed_grad_gemm forms the dX rows it needs from (dH, W^T)
                # inside the segmented reduce): the token consumer's gradient IS the dx operand of that launch — no dX, no add
                dx = extra
            elif dx is None or fused is not None:
                raise RuntimeError("token_view: the gathered activation needs a consumer that materialises its gradient")
            else:
                hip.add_rows_to(extra, dx[:, :extra.shape[1]])
        gfm = dfm.contiguous() if (ctx.want_fm and dfm is not None) else None
        if ctx.link is not None and ctx.link.folded:
            ssum = None  # g_fm * S is already inside dx (rp_linear_fwd_rowadd)
        if fused is None:
            store.accumulate_grad(keys, ctx.B, dx, gfm, ssum, presorted=ctx.presorted)
        else:  # (dH, W^T) of the Linear that consumes x: its dgrad is formed inside the reduce
            g = store.first_layer_grad(keys, ctx.B, *fused, gfm, ssum, presorted=ctx.presorted, dx=dx)
            if g.forms.tiny:
                g.tiny()
            g.gemm()
            g.done()
        return (None,) * (6 + len(store.emb_feature))


_WGRAD_STREAMS: dict = {}


def _side2_stream(device):
    st = _WGRAD_STREAMS.get(device)
    if st is None:
        st = _WGRAD_STREAMS[device] = hip.make_side_stream(device)
    return st


def _masked_by_consumer(lk, dy) -> bool:
    """does dy already carry the ReLU mask of the activation it belongs to — is it the very gradient the consumer of that
    activation left in the ReluLink `lk`?  (The link's gradient is used up either way.)"""
    masked = lk is not None and lk.dx is not None and lk.dx.data_ptr() == dy.data_ptr() and lk.dx.shape == dy.shape
    if lk is not None:
        lk.dx = None
    return masked


def _wgrad_stream(device):
    """the stream the first layer's weight gradient runs on beside the gather backward (RP_WGRAD_OVERLAP=0: none); never
    inside a stream capture (a fork inside a captured graph is replayed without overlap anyway)"""
    if os.environ.get("RP_WGRAD_OVERLAP", "1") == "0" or torch.cuda.is_current_stream_capturing():
        return None
    return _side2_stream(device)


class _EmbedGatherLinear(torch.autograd.Function):
    """rp_embed_gather_linear_fwd: lookup + dense concat + FM + the first Linear (+ ReLU) of the MLP in one launch; the
    backward is the weight gradient (x is still written for it) and rp_embed_grad_gemm (dX never exists).  `out_link`: the
    ReluLink shared with the consumer of h1 (the fused MLP tail hands back a gradient that is already masked)."""

    @staticmethod
    def forward(ctx, store, idx, dense, ldx: int, weight, bias, out_link, shadow, *tables):
        pre = store._presorted
        store._presorted = None
        need_grad = any(ctx.needs_input_grad[8:])
        need_w = ctx.needs_input_grad[4] or (bias is not None and ctx.needs_input_grad[5])
        B, K, Kg = idx[0].shape[0], weight.shape[1], len(idx) * store.embedding_dim
        wt = None
        if need_grad and weight.is_cuda and weight.dtype is torch.float32 and K % 4 != 0 and K > 64:
            # the backward will want W^T (rp_embed_grad_gemm) and this forward wants the aligned copy of W: one launch makes
            # both from one read of W, in front of the forward, and the transpose leaves the backward's critical path
            with torch.no_grad():
                wt, w16 = hip.transpose_copy(weight.detach(), rows_out=ldx, ld_copy=(K + 3) // 4 * 4)
        else:
            w16 = _rows16(weight)
        ctx.wt = wt
        if shadow is not None:
            # bf16-storage training (EmbeddingLayer.bf16_training): rows from the bf16 lookup copy, the activation stored as
            # bf16 for the weight gradient (rp_linear_wgrad_xbf16); everything else as below
            want_keys = pre is None
            # round 5: like the fp32 tables' path, no activation is stored when the tables get gradients — the embedding columns
            # of the weight gradient come from rp_embed_grad_seg over the fp32 MASTER rows (the forward used their bf16 images:
            # a 2^-9-relative inconsistency inside the mode's stated tolerance, and closer to the fp32 reference);
            # RP_GRAD_SEG=0: the stored bf16 activation + rp_linear_wgrad_xbf16 (round 4)
            seg16 = (need_grad and need_w and K > Kg and len(idx) <= 64 and os.environ.get("RP_GRAD_SEG", "1") != "0"
                     and weight.shape[0] == 64 and store.embedding_dim == 64)  # (what rp_embed_grad_seg_fits asks for: ADVICE r5)
            x, h1, fm, ssum, keys = hip.embed_gather_linear_fwd_bf16(shadow, store.row_base, store.row_count, idx, dense, w16, bias,
                                                                     store.err_flag, train_ldx=ldx, want_keys=want_keys,
                                                                     dense_only=seg16)
            ctx.store, ctx.B, ctx.K, ctx.out_link, ctx.has_bias = store, B, K, out_link, bias is not None
            ctx.ldx, ctx.x_mode, ctx.Kg, ctx.need_tables = ldx, ("seg" if seg16 else "bf16"), Kg, need_grad
            ctx.presorted = pre if need_grad else None
            if pre is not None:
                keys = pre.keys
            ctx.save_for_backward(keys, ssum, x, h1, weight)
            store._fm_link = None
            return h1, fm
        # x exists only for the weight gradient; inference stores none.
        # "seg" (round 5, the default where it fits): NO activation is stored at all — the embedding columns of the weight
        # gradient come out of the gather backward itself (rp_embed_grad_seg: one matrix pass per run of equal rows over the
        # table rows it reads anyway), the dense columns from a small weight gradient over xd.  RP_GRAD_SEG=0: the stored x.
        if not need_w:
            x_mode = "none"
        elif (need_grad and K > Kg and len(idx) <= 64 and os.environ.get("RP_GRAD_SEG", "1") != "0"
              and store.embedding_dim == 64 and weight.shape[0] == 64):
            x_mode = "seg"
        else:
            x_mode = "full"
        want_keys = need_grad and pre is None
        x, h1, fm, ssum, keys = hip.embed_gather_linear_fwd(store.arena, store.row_base, store.row_count, idx, dense, ldx, w16,
                                                            bias, True, need_grad, want_keys, store.err_flag,
                                                            x_mode="dense" if x_mode == "seg" else x_mode)
        ctx.store, ctx.B, ctx.K, ctx.out_link, ctx.has_bias = store, B, K, out_link, bias is not None
        ctx.ldx, ctx.x_mode, ctx.Kg, ctx.need_tables = ldx, x_mode, Kg, need_grad
        ctx.presorted = pre if need_grad else None
        if pre is not None:
            keys = pre.keys if need_grad else None
        ctx.save_for_backward(keys, ssum, x, h1, weight)
        store._fm_link = None
        return h1, fm

    @staticmethod
    def backward(ctx, dh1, dfm):
        keys, ssum, x, h1, weight = ctx.saved_tensors
        store = ctx.store
        dh1 = _unit_inner(dh1)
        dpre = dh1 if _masked_by_consumer(ctx.out_link, dh1) else hip.relu_bwd(dh1, h1)
        dw = db = None
        need_w = ctx.needs_input_grad[4] or (ctx.has_bias and ctx.needs_input_grad[5])
        need_t = keys is not None and ctx.need_tables
        if need_w and ctx.x_mode == "none":
            raise RuntimeError("the fused lookup + first layer stored no activation (the forward ran without gradients for the "
                               "layer's weight)")
        # "seg": the weight gradient's three column groups come from three launches: the dense columns (+ the bias gradient)
        # from rp_linear_wgrad over xd, the tiny tables' from rp_embed_grad_tiny and the other tables' from the big / rest
        # launches of the gather backward (store.first_layer_grad), all into dw_seg
        seg = need_w and ctx.x_mode == "seg"
        dw_seg = torch.empty((64, ctx.K), dtype=torch.float32, device=dpre.device) if seg else None

        def wgrad():
            if ctx.x_mode == "seg":    # x holds the dense columns only (xd [B, 64]); their columns of dw and the bias gradient
                return dw_seg, hip.linear_wgrad(dpre, x, ctx.K - ctx.Kg, dw=dw_seg[:, ctx.Kg:], want_bias=ctx.has_bias)[1]
            if ctx.x_mode == "bf16":   # the activation was stored as bf16 (bf16-storage training)
                return hip.linear_wgrad_xbf16(dpre, x, ctx.K, want_bias=ctx.has_bias)
            return hip.linear_wgrad(dpre, x, ctx.K, want_bias=ctx.has_bias)

        # The weight gradient (streams x: 0.15 ms at Criteo shape) and the fused gather backward (bound by its random row
        # gathers, ~1 TB/s of HBM: 0.30 ms) both depend only on dpre and are independent of each other: the weight gradient
        # runs on a second stream BESIDE the gather backward instead of in front of it.  Same kernels, same inputs: bit-identical.
        wstream = _wgrad_stream(dpre.device) if (need_w and need_t) else None
        # ... and while a LAUNCH PLAN is being recorded (a captured step: one stream), the side launches are marked as an
        # inline section (plan.side2): the replay issues them on the plan's second side stream, joined after the gather
        # backward; until that join hip.holding() keeps every tensor hip allocates (launches that run BESIDE others: hip.py).
        plan = hip.LaunchPlan
        in_plan = (wstream is None and need_w and need_t
                   and os.environ.get("RP_WGRAD_OVERLAP", "1") != "0" and plan.is_recording())

        def side_wgrad():
            with plan.side2(in_plan):
                out = wgrad()
                if in_plan:
                    plan.run_deferred()  # (e.g. the MLP tail's second stage: behind the weight gradient, not in front)
            return out

        # THE ISSUE ORDER of the first layer's backward: {a plan is recording} x {dw's embedding columns come from the gather
        # backward (seg)}.  Except when both hold, the weight gradient goes first: in front, or beside on the second stream.
        with hip.holding() if in_plan else contextlib.nullcontext():
            if wstream is not None:
                main = torch.cuda.current_stream(dpre.device)
                wstream.wait_stream(main)
                with torch.cuda.stream(wstream):
                    dw, db = wgrad()
            elif need_w and not (in_plan and seg):
                dw, db = side_wgrad()
            if need_t:
                wt = ctx.wt if ctx.wt is not None else hip.transpose(weight, rows_out=ctx.ldx)
                gfm = dfm.contiguous() if dfm is not None else None
                g = store.first_layer_grad(keys, ctx.B, dpre, wt, gfm, ssum if gfm is not None else None, presorted=ctx.presorted,
                                           w=weight if seg else None, dw=dw_seg)
                f = g.forms
                if not seg:  # (recording or not) the tiny tables on the side, one row-sorted launch for all others
                    if f.tiny:
                        with plan.side2(in_plan):
                            g.tiny()
                    g.gemm()
                elif not in_plan:  # the caller's stream: tiny, sample-major, row-sorted, the launches behind the sample-major one
                    if f.tiny:
                        g.tiny()
                    ws = g.big(1) if f.big else None
                    if f.rest:
                        g.rest()
                    if f.big:
                        g.big(2, ws)
                else:
                    # (round 5) the LONG main-stream launch is issued first and the short side launches behind it, all forked from
                    # the same point (plan.fork2_mark) — issued the other way round the side launches filled every CU and
                    # rp_embed_grad_seg (77 KB of LDS per workgroup) started 58 us late (profiles/r05_trace_step.txt)
                    # Measured (profiles/r05 lines, alternating runs on one box): 0.946 / 0.947 ms with the main launch first
                    # against 0.929 / 0.932 the other way round (long-run means equal, 0.906-0.916): the side launches then stretch
                    # to twice their time and the join comes later
                    # (re-measured at the end of round 5, after the loss head moved into the MLP tail and the side streams went to
                    #  the lowest priority: main launch first 0.8324 / 0.8375 ms against 0.8369 / 0.8384 in the 20-step window,
                    #  0.8086 / 0.8099 against 0.8152 / 0.8161 over 600 steps)
                    # (round 6) with big tables the sample-major launch is that long launch; the tiny tables' launches are forked IN
                    # FRONT of it and run beside it on the second stream, and the launches behind the sample-major one follow them
                    # there (plan.side2_sync: that stream waits for the sample-major launch at that point); without tiny tables the
                    # fork is marked behind the sample-major launch
                    if f.tiny or not f.big:
                        plan.fork2_mark()
                    if f.big:
                        ws = g.big(1)
                        if f.tiny:
                            with plan.side2():
                                g.tiny()
                            plan.side2_sync()
                        else:
                            plan.fork2_mark()
                    # (the streaming segment-sum launch uses no LDS, but it cannot run BESIDE the sample-major launch on a second
                    #  stream: 4 x 112 and 2 x 240 registers per SIMD lane do not fit the file of 512 together — one after the
                    #  other on the main stream)
                    if f.rest:
                        g.rest()
                    if f.big:
                        # on the second stream beside the row-sorted form's launches; in ISSUE order behind those: issued in front
                        # of them, the 4096 short workgroups of the duplicate reduce held the segment-sum launch up by 56 us
                        # (profiles/r06 trace notes)
                        with plan.side2():
                            g.big(2, ws)
                    elif f.tiny:  # (no sample-major launch: behind the long main-stream launch in issue order)
                        with plan.side2():
                            g.tiny()
                g.done()
            if in_plan:
                if seg:
                    dw, db = side_wgrad()
                plan.join()
        if wstream is not None:
            main.wait_stream(wstream)  # whoever consumes dw / db (AccumulateGrad, the optimizer) is ordered behind them
            dw.record_stream(main)     # (allocated under the second stream, consumed and freed on the main one)
            if db is not None:
                db.record_stream(main)
        return (None, None, None, None, dw, db, None, None) + (None,) * len(store.emb_feature)


def embed_gather_linear(store, idx, dense, ldx: int, weight, bias, out_link, shadow=None):
    tables = [store.embedding_layer[c].weight for c in store.emb_feature]
    return _EmbedGatherLinear.apply(store, idx, dense, ldx, weight, bias, out_link, shadow, *tables)


def embed_gather(store, idx, dense, ldx: int, want_fm: bool, meta=None):
    """`meta` = (row_base, row_count) of the tables `idx` addresses when that is a subset of the store's fields
    (single-field / sequence lookups); None = all fields in order."""
    tables = [store.embedding_layer[c].weight for c in store.emb_feature]
    return _EmbedGather.apply(store, idx, dense, ldx, want_fm, meta, *tables)


# ----------------------------------------------------------------------------------------------
# pooled multi-id lookup (north_star's CSR / segmented gather + sum-pool): embedding.py:64-71 (`_seq`) followed by
# layers/sequence.py:13-59 (MaskedAveragePooling / MaskedSumPooling) as ONE launch each way
# ----------------------------------------------------------------------------------------------
class _EmbedGatherPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, store, field: int, ids, offsets, L: int, B: int, mode: str, presorted, *tables):
        need_grad = any(ctx.needs_input_grad[8:])
        base, count = store.table_range(field)
        out, inv, bag = hip.embed_gather_pool_fwd(store.arena, base, count, ids, offsets, L, B, mode, store.err_flag,
                                                  need_grad)
        ctx.store, ctx.field, ctx.L, ctx.presorted = store, field, L, presorted
        ctx.save_for_backward(ids, inv, bag)
        return out

    @staticmethod
    def backward(ctx, g):
        ids, inv, bag = ctx.saved_tensors
        store = ctx.store
        store.pool_grad(ctx.field, ids, g.contiguous(), inv, bag, ctx.L, presorted=ctx.presorted)
        return (None,) * (8 + len(store.emb_feature))


def embed_gather_pool(store, field: int, ids, offsets, L: int, B: int, mode: str, presorted=None):
    tables = [store.embedding_layer[c].weight for c in store.emb_feature]
    return _EmbedGatherPool.apply(store, field, ids, offsets, L, B, mode, presorted, *tables)


class _SeqPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, mode: str):
        out, inv = hip.seq_pool_fwd(e, mode, ctx.needs_input_grad[0])
        ctx.L = e.shape[1]
        ctx.save_for_backward(inv)
        return out

    @staticmethod
    def backward(ctx, g):
        (inv,) = ctx.saved_tensors
        return hip.seq_pool_bwd(g.contiguous(), inv, ctx.L), None


def seq_pool(e, mode: str):
    """MaskedSumPooling ("sum") / MaskedAveragePooling ("average") of an explicit [B, L, D] HIP tensor"""
    return _SeqPool.apply(e.float().contiguous(), mode)


# ----------------------------------------------------------------------------------------------
# sequence recall: the full-softmax loss head (models/base_model.py:124-138 of the reference) and the masked history mean
# (models/sequence/yotubednn.py:34-36).  No [B, V] and no [B, L, D] tensor exists on the HIP path.
# ----------------------------------------------------------------------------------------------
_SEQ_FLAGS: dict = {}


def _seq_flag(device) -> torch.Tensor:
    """the device word the sequence kernels raise on an id / target outside its table (one per device)"""
    flag = _SEQ_FLAGS.get(device)
    if flag is None:
        flag = _SEQ_FLAGS[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return flag


def _raise_if_flagged(device, what: str):
    flag = _seq_flag(device)
    if int(flag.item()) != 0:  # (one 4-byte copy: what the reference's CPU ops check on the host)
        flag.zero_()
        raise IndexError(what)


class _SoftmaxCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user_emb, item_weight, target):
        u, e = _unit_inner(user_emb), item_weight.contiguous()
        loss, lse = hip.softmax_ce_fwd(u, e, target, _seq_flag(u.device))
        # the inputs themselves plus lse [B]: no logits, no softmax
        ctx.save_for_backward(u, e, target, lse)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        u, e, target, lse = ctx.saved_tensors
        du, de = hip.softmax_ce_bwd(u, e, target, lse, g.reshape(1).float().contiguous(), ctx.needs_input_grad[0],
                                    ctx.needs_input_grad[1])
        return du, de, None


def full_softmax_ce(user_emb: torch.Tensor, item_weight: torch.Tensor, target: torch.Tensor, check_indices: str = "sync"):
    """CrossEntropyLoss()(user_emb @ item_weight.T, target), the scalar mean over the batch (reference
    models/base_model.py:135-137).  user_emb [B, D], item_weight [V, D], target int64 [B].  On the HIP device the fused
    kernels (no [B, V] tensor; the backward recomputes from lse); check_indices "sync" raises IndexError for a target outside
    [0, V) right after the forward, as the reference's CPU loss does, "deferred" leaves the flag set.  On CPU tensors the
    reference's torch formula."""
    if not user_emb.is_cuda:
        return torch.nn.functional.cross_entropy(torch.matmul(user_emb, item_weight.transpose(1, 0)), target)
    target = target.contiguous()
    if user_emb.dtype != torch.float32 or item_weight.dtype != torch.float32 or not hip.softmax_ce_fits(user_emb.shape[1]):
        hip.note_torch_path(f"full_softmax_ce at D={user_emb.shape[1]}, {user_emb.dtype} (the kernels take fp32 up to "
                            f"D={hip.softmax_ce_geometry()['max_d']})")
        return torch.nn.functional.cross_entropy(torch.matmul(user_emb, item_weight.transpose(1, 0)), target)
    loss = _SoftmaxCE.apply(user_emb, item_weight, target)
    if check_indices == "sync":
        _raise_if_flagged(user_emb.device, f"Target out of bounds: every target must lie in [0, {item_weight.shape[0]})")
    return loss


class _HistMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, item_weight, hist, mask):
        e = item_weight.contiguous()
        out = hip.hist_mean_fwd(e, hist, mask, _seq_flag(e.device))
        ctx.save_for_backward(hist, mask)
        ctx.rows = e.shape
        return out

    @staticmethod
    def backward(ctx, g):
        hist, mask = ctx.saved_tensors
        de = torch.zeros(ctx.rows, dtype=torch.float32, device=g.device)
        hip.hist_mean_bwd(hist, mask, _unit_inner(g), de)
        return de, None, None


def hist_mean(item_weight: torch.Tensor, hist: torch.Tensor, mask: torch.Tensor, check_indices: str = "sync"):
    """mean over dim 1 of item_emb(hist) * mask[..., None] with item_emb = nn.Embedding(V, D, padding_idx=0) (reference
    models/sequence/yotubednn.py:34-36): out[b] = (1/L) sum_l mask[b, l] item_weight[hist[b, l]] — the divisor is L, not the
    mask count — and no gradient reaches row 0 through it, whatever the mask.  hist int64 [B, L], mask [B, L] of any dtype.
    On the HIP device one launch each way and no [B, L, D] tensor; on CPU tensors the reference's torch formula."""
    if not item_weight.is_cuda:
        e = torch.nn.functional.embedding(hist, item_weight, padding_idx=0)
        return torch.mean(e * mask.unsqueeze(-1).float(), dim=1)
    if item_weight.dtype != torch.float32:
        hip.note_torch_path(f"hist_mean over a {item_weight.dtype} table (the kernels take fp32)")
        e = torch.nn.functional.embedding(hist, item_weight, padding_idx=0)
        return torch.mean(e * mask.unsqueeze(-1).float(), dim=1)
    out = _HistMean.apply(item_weight, hist.contiguous(), mask.float().contiguous())
    if check_indices == "sync":
        _raise_if_flagged(item_weight.device, "index out of range in self")
    return out


# ----------------------------------------------------------------------------------------------
# sequence recall: the GRU encoder of GRU4Rec / NARM (models/layers/sequence.py:231-251, models/sequence/narm.py:49) and
# NARM's attention readout (narm.py:52-61).  One launch per layer and direction; only the hidden states are saved.
# ----------------------------------------------------------------------------------------------
def _gru_layers(rnn):
    """[(W_ih, W_hh, b_ih, b_hh)] per layer of an nn.GRU (biases None without them)"""
    out = []
    for k in range(rnn.num_layers):
        b = (getattr(rnn, f"bias_ih_l{k}"), getattr(rnn, f"bias_hh_l{k}")) if rnn.bias else (None, None)
        out.append((getattr(rnn, f"weight_ih_l{k}"), getattr(rnn, f"weight_hh_l{k}")) + b)
    return out


class _HistRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, item_weight, hist):
        e = item_weight.contiguous()
        ctx.save_for_backward(hist)
        ctx.rows = e.shape
        return hip.hist_rows_fwd(e, hist, _seq_flag(e.device))

    @staticmethod
    def backward(ctx, g):
        (hist,) = ctx.saved_tensors
        de = hip.zeros(ctx.rows, torch.float32, g.device)
        hip.hist_rows_bwd(hist, g.contiguous(), de)
        return de, None


class _GRUEncode(torch.autograd.Function):
    """inputs: item_weight | None, x | None, ids | None, steps, last, layers, has_bias, then each layer's parameters"""

    @staticmethod
    def forward(ctx, item_weight, x, ids, steps, last, n_layers: int, has_bias: bool, *params):
        ctx.set_materialize_grads(False)  # (GRU4Rec reads h_last only, NARM both: no zero-filled [B, L, H] gradient)
        per = 4 if has_bias else 2
        layers = [tuple(p.contiguous() for p in params[k * per:(k + 1) * per]) + ((None, None) if not has_bias else ())
                  for k in range(n_layers)]
        e = item_weight.contiguous() if ids is not None else None
        inp, hs, h_last = x, [], None
        for k, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
            first_ids = k == 0 and ids is not None
            h_all, h_last = hip.gru_fwd(ids if first_ids else None, e if first_ids else None, None if first_ids else inp,
                                        w_ih, w_hh, b_ih, b_hh, steps, last, _seq_flag(w_ih.device) if first_ids else None)
            hs.append(h_all)
            inp = h_all
        ctx.n_layers, ctx.has_bias, ctx.per = n_layers, has_bias, per
        ctx.e_shape = None if e is None else e.shape
        # saved between forward and backward: the inputs themselves and layers * B * L * H floats of hidden states
        ctx.save_for_backward(e, x, ids, steps, last, *hs, *[p for lay in layers for p in lay[:per]])
        return hs[-1], h_last

    @staticmethod
    def backward(ctx, dh_all, dh_last):
        n, per = ctx.n_layers, ctx.per
        saved = ctx.saved_tensors
        e, x, ids, steps, last = saved[:5]
        hs, flat = saved[5:5 + n], saved[5 + n:]
        need = ctx.needs_input_grad
        grads = [None] * (n * per)
        d_in = None
        dh_all = None if dh_all is None else dh_all.contiguous()
        dh_last = None if dh_last is None else dh_last.contiguous()
        for k in range(n - 1, -1, -1):
            p = flat[k * per:(k + 1) * per]
            w_ih, w_hh = p[0], p[1]
            b_ih, b_hh = (p[2], p[3]) if ctx.has_bias else (None, None)
            first_ids = k == 0 and ids is not None
            want_dx = k > 0 or (need[0] if first_ids else need[1])
            want_dw = any(need[7 + k * per:7 + (k + 1) * per])
            if not (want_dx or want_dw):
                break  # (nothing below this layer asks for a gradient either)
            got = hip.gru_bwd(ids if first_ids else None, e if first_ids else None,
                              None if first_ids else (x if k == 0 else hs[k - 1]), w_ih, w_hh, b_ih, b_hh, steps, last, hs[k],
                              dh_all, dh_last if k == n - 1 else None, want_dx, want_dw)
            dh_all = got[0]
            if want_dw:
                grads[k * per:(k + 1) * per] = got[1:1 + per]
            if k == 0:
                d_in = got[0]
        de = dx = None
        if ids is not None and need[0] and d_in is not None:
            de = hip.zeros(tuple(ctx.e_shape), torch.float32, d_in.device)
            hip.hist_rows_bwd(ids, d_in, de)
        elif ids is None and need[1]:
            dx = d_in
        return (de, dx, None, None, None, None, None, *grads)


def _gru_torch(rnn, e, steps, last, packed: bool):
    """torch's nn.GRU over e [B, L, in]: the reference's pack / unpack when packed (a zero length raises, as there)"""
    L = e.shape[1]
    if packed:
        seq = torch.nn.utils.rnn.pack_padded_sequence(e, steps.cpu().to(torch.int64), batch_first=True, enforce_sorted=False)
        out, _ = rnn(seq, None)
        h_all, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=L)
    else:
        h_all, _ = rnn(e)
    ok = (last >= 0) & (last < steps)
    idx = last.clamp(min=0).to(torch.int64).view(-1, 1, 1).expand(-1, 1, h_all.shape[-1])
    h_last = h_all.gather(1, idx).squeeze(1) * ok.unsqueeze(-1).to(h_all.dtype)
    return h_all, h_last


def gru_encode(rnn, steps: torch.Tensor, last: torch.Tensor, x: torch.Tensor = None, ids: torch.Tensor = None,
               item_weight: torch.Tensor = None, packed: bool = True, check_indices: str = "sync"):
    """A multi-layer, one-direction nn.GRU `rnn` (the parameter holder) over a batch of histories, h_0 = 0 ->
    (H_all [B, L, H], h_last [B, H]) of the top layer.  Input: either ids int64 [B, L] + item_weight [V, in] (the rows of
    nn.Embedding(padding_idx=0), gathered inside the kernel: no [B, L, in] tensor) or a dense x [B, L, in].  steps [B]: row b
    takes steps[b] steps (packed: its length, H_all zero behind it; full: L); h_last[b] = H_all[b, last[b]], zero where
    last[b] < 0 or >= steps[b].  On the HIP device one rp_gru_fwd / rp_gru_bwd launch per layer; on CPU tensors torch's nn.GRU
    (packed: the reference's pack / unpack, which raises for a zero length)."""
    dev_t = x if x is not None else item_weight
    layers = _gru_layers(rnn)
    if rnn.bidirectional or (rnn.dropout and rnn.training) or getattr(rnn, "proj_size", 0):
        raise NotImplementedError("gru_encode: one direction, no dropout between the layers, no projection")
    if not dev_t.is_cuda:
        e = x if x is not None else torch.nn.functional.embedding(ids, item_weight, padding_idx=0)
        return _gru_torch(rnn, e, steps, last, packed)
    n_in, H = layers[0][0].shape[1], rnn.hidden_size
    if dev_t.dtype != torch.float32 or not hip.gru_fits(n_in, H):
        hip.note_torch_path(f"gru_encode at in={n_in}, H={H}, {dev_t.dtype} (the kernels take fp32 up to "
                            f"{hip.gru_geometry()['max_h']} columns)")
        e = x if x is not None else torch.nn.functional.embedding(ids, item_weight, padding_idx=0)
        return _gru_torch(rnn, e, steps, last, packed)
    per = 4 if rnn.bias else 2
    flat = [p for lay in layers for p in lay[:per]]
    steps32, last32 = steps.to(torch.int32).contiguous(), last.to(torch.int32).contiguous()
    h_all, h_last = _GRUEncode.apply(item_weight if ids is not None else None, None if x is None else x.contiguous(),
                                     None if ids is None else ids.contiguous(), steps32, last32, rnn.num_layers, bool(rnn.bias),
                                     *flat)
    if ids is not None and check_indices == "sync":
        _raise_if_flagged(dev_t.device, "index out of range in self")
    return h_all, h_last


def hist_rows(item_weight: torch.Tensor, hist: torch.Tensor, check_indices: str = "sync"):
    """nn.Embedding(V, D, padding_idx=0)(hist) as a [B, L, D] tensor: the lookup on its own (row 0 takes no gradient)"""
    if not item_weight.is_cuda or item_weight.dtype != torch.float32:
        if item_weight.is_cuda:
            hip.note_torch_path(f"hist_rows over a {item_weight.dtype} table (the kernels take fp32)")
        return torch.nn.functional.embedding(hist, item_weight, padding_idx=0)
    out = _HistRows.apply(item_weight, hist.contiguous())
    if check_indices == "sync":
        _raise_if_flagged(item_weight.device, "index out of range in self")
    return out


class _NarmAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q1, q2, v, ids, gru_out, ht):
        q1, q2, v, g, ht = q1.contiguous(), q2.contiguous(), v.contiguous().view(-1), gru_out.contiguous(), ht.contiguous()
        out, alpha = hip.narm_attn_fwd(q1, q2, v, ids, g, ht)
        ctx.save_for_backward(q1, q2, v, ids, g, alpha)
        ctx.v_shape = v.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        q1, q2, v, ids, g, alpha = ctx.saved_tensors
        dq1, dq2, dv, dg, dht = hip.narm_attn_bwd(q1, q2, v, ids, g, alpha, dout.contiguous())
        return dq1, dq2, dv, None, dg, dht


def narm_attention(q1: torch.Tensor, q2: torch.Tensor, v: torch.Tensor, ids: torch.Tensor, gru_out: torch.Tensor,
                   ht: torch.Tensor):
    """NARM's readout (reference models/sequence/narm.py:54-61): alpha = (mask * sigmoid(q1 + q2[:, None])) @ v with
    mask = ids > 0, c_local = sum_l alpha * gru_out -> cat([c_local, ht], 1) [B, 2H].  q1, gru_out [B, L, H]; q2, ht [B, H];
    v [H] (v_t.weight.view(-1)); ids int64 [B, L].  On the HIP device one launch each way plus dv's finishing sum."""
    H = gru_out.shape[-1]
    if not gru_out.is_cuda or gru_out.dtype != torch.float32 or not hip.narm_attn_fits(H):
        if gru_out.is_cuda:
            hip.note_torch_path(f"narm_attention at H={H}, {gru_out.dtype} (the kernels take fp32 up to H=128)")
        mask = ids.gt(0).unsqueeze(2).expand_as(gru_out)
        alpha = torch.matmul(mask * torch.sigmoid(q1 + q2.unsqueeze(1).expand_as(q1)), v.view(-1, 1))
        return torch.cat([torch.sum(alpha.expand_as(gru_out) * gru_out, 1), ht], 1)
    return _NarmAttention.apply(q1, q2, v.view(-1), ids.contiguous(), gru_out, ht)


# ----------------------------------------------------------------------------------------------
# sequence recall: the multi-interest encoder of MIND / ComirecDR (models/layers/multi_interest.py:96-161 of the reference) and
# the hard readout (models/sequence/mind.py:44-49).  Saved between forward and backward: the projected rows, the mask and the
# initial logits of the routing, one int32 per row of the readout.  No [B, L, K D, D] tensor exists on the HIP path.
# ----------------------------------------------------------------------------------------------
class _CapsuleProject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x = x.contiguous()
        w3 = w.reshape(w.shape[-3], w.shape[-2], w.shape[-1]).contiguous()
        ctx.save_for_backward(x, w3)
        ctx.w_shape = w.shape
        return hip.capsule_project_fwd(x, w3)

    @staticmethod
    def backward(ctx, du):
        x, w3 = ctx.saved_tensors
        dx, dw = hip.capsule_project_bwd(du.contiguous(), x, w3, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, None if dw is None else dw.view(ctx.w_shape)


def capsule_project(x: torch.Tensor, w: torch.Tensor):
    """ComirecDR's per-position projection (reference multi_interest.py:103-105): sum(w[:, :L] * x.unsqueeze(2), dim=3) with
    x [B, L, D] and w [1, L, K D, D] (or [L, K D, D]) -> [B, L, K D].  On the HIP device one launch each for the forward, dX and
    dW on the exact-fp32 matrix core and no [B, L, K D, D] product; on CPU tensors the reference's formula."""
    L = x.shape[1]
    w4 = w if w.dim() == 4 else w.unsqueeze(0)
    if not x.is_cuda:
        return torch.sum(w4[:, :L, :, :] * torch.unsqueeze(x, dim=2), dim=3)
    N, D = w4.shape[2], w4.shape[3]
    if x.dtype != torch.float32 or w.dtype != torch.float32 or not hip.capsule_project_fits(L, N, D):
        hip.note_torch_path(f"capsule_project at K D={N}, D={D}, {x.dtype} (the kernels take fp32, D <= 128, K D <= 2048)")
        return torch.einsum("lnd,bld->bln", w4[0, :L], x)
    return _CapsuleProject.apply(x, w4[:, :L])


class _CapsuleRoute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u_hat, mask, b0, K: int, shared: bool, stop_grad: bool):
        u_hat = u_hat.contiguous()
        ctx.save_for_backward(u_hat, mask, b0)  # the inputs themselves: the backward recomputes the three rounds
        ctx.cfg = (K, shared, stop_grad)
        return hip.capsule_route_fwd(u_hat, mask, b0, K, shared)

    @staticmethod
    def backward(ctx, dout):
        u_hat, mask, b0 = ctx.saved_tensors
        K, shared, stop_grad = ctx.cfg
        return hip.capsule_route_bwd(u_hat, mask, b0, dout.contiguous(), K, shared, stop_grad), None, None, None, None, None


def _capsule_route_torch(u_hat, mask, K: int, b0, shared: bool, stop_grad: bool, rounds: int = 3):
    """the reference's formulation, op for op (multi_interest.py:99, 107-156)"""
    B, L, W = u_hat.shape
    D = W if shared else W // K
    item_eb_hat = u_hat.repeat(1, 1, K) if shared else u_hat
    item_eb_hat = torch.reshape(item_eb_hat, (-1, L, K, D))
    item_eb_hat = torch.transpose(item_eb_hat, 1, 2).contiguous()
    item_eb_hat_iter = item_eb_hat.detach() if stop_grad else item_eb_hat
    capsule_weight = torch.zeros(B, K, L, device=u_hat.device, dtype=u_hat.dtype) if b0 is None else b0
    interest_capsule = None
    for i in range(rounds):
        atten_mask = torch.unsqueeze(mask, 1).repeat(1, K, 1)
        paddings = torch.zeros_like(atten_mask, dtype=u_hat.dtype)
        c = torch.nn.functional.softmax(capsule_weight, dim=-1)
        c = torch.unsqueeze(torch.where(torch.eq(atten_mask, 0), paddings, c), 2)
        src = item_eb_hat_iter if i < 2 else item_eb_hat
        interest_capsule = torch.matmul(c, src)
        cap_norm = torch.sum(torch.square(interest_capsule), -1, True)
        interest_capsule = cap_norm / (1 + cap_norm) / torch.sqrt(cap_norm + 1e-9) * interest_capsule
        if i < 2:
            delta = torch.matmul(src, torch.transpose(interest_capsule, 2, 3).contiguous())
            capsule_weight = capsule_weight + torch.reshape(delta, (-1, K, L))
    return torch.reshape(interest_capsule, (-1, K, D))


def capsule_route(u_hat: torch.Tensor, mask: torch.Tensor, K: int, b0: torch.Tensor = None, shared: bool = False,
                  stop_grad: bool = False, rounds: int = 3):
    """Three rounds of dynamic routing (reference multi_interest.py:125-154) -> the interest capsules [B, K, D].
    u_hat: the projected history rows, [B, L, K D] (interest k reads the columns [k D, k D + D)) or, shared, [B, L, D] read by
    all K interests (MIND: the reference's .repeat(1, 1, K) is a stride here).  mask [B, L] (0 = padding, any dtype);
    b0 [B, K, L]: the initial routing logits, None for zeros; it takes no gradient.  The softmax runs over all L positions and
    the masked weights are not renormalised; a fully masked row gives zeros.  stop_grad: rounds 0 and 1 read a detached
    u_hat.  rounds: the reference's routing_times; the logits stop changing after round 1, so every count from 3 up gives
    round 2's capsules.  On the HIP device one launch each way (the backward recomputes the rounds); outside
    rp_capsule_geometry's limits, or with fewer than 3 rounds, the composed torch formulas on the device, counted; on CPU
    tensors the reference's formulas."""
    if rounds < 1:
        raise ValueError("capsule_route: at least one routing round")
    if b0 is not None:
        b0 = b0.detach().to(u_hat.device)
    if not u_hat.is_cuda:
        return _capsule_route_torch(u_hat, mask, K, b0, shared, stop_grad, rounds)
    B, L, W = u_hat.shape
    D = W if shared else W // K
    if u_hat.dtype != torch.float32 or rounds < 3 or not hip.capsule_route_fits(K, L, D):
        g = hip.capsule_geometry()
        hip.note_torch_path(f"capsule_route at K={K}, L={L}, D={D}, {rounds} rounds, {u_hat.dtype} (the kernel takes fp32, "
                            f"3 rounds, K <= {g['max_k']}, L <= {g['max_l']}, D <= {g['max_d']} and 4 max(K, 2) L (D + 1) <= "
                            f"{g['lds_bytes']} bytes)")
        return _capsule_route_torch(u_hat, mask, K, b0, shared, stop_grad, rounds)
    b0 = None if b0 is None else b0.float().contiguous()
    return _CapsuleRoute.apply(u_hat, mask.float().contiguous(), b0, K, shared, stop_grad)


class _InterestPick(torch.autograd.Function):
    @staticmethod
    def forward(ctx, interests, item_weight, target):
        best, kidx = hip.interest_pick_fwd(interests.contiguous(), item_weight.contiguous(), target, _seq_flag(interests.device))
        ctx.save_for_backward(kidx)
        ctx.K = interests.shape[1]
        return best

    @staticmethod
    def backward(ctx, dbest):
        (kidx,) = ctx.saved_tensors
        return hip.interest_pick_bwd(dbest.contiguous(), kidx, ctx.K), None, None


def interest_pick(interests: torch.Tensor, item_weight: torch.Tensor, target: torch.Tensor, check_indices: str = "sync"):
    """The hard readout of the multi-interest models (reference mind.py:44-49): per row the interest that scores highest
    against the target's item row, interests [B, K, D], item_weight [V, D], target int64 [B] -> [B, D].  The first maximum
    wins, as torch.argmax; no gradient flows through the scores.  On the HIP device one launch each way instead of the
    reference's Python loop over the batch; check_indices as in full_softmax_ce."""
    if not interests.is_cuda or interests.dtype != torch.float32 or item_weight.dtype != torch.float32:
        if interests.is_cuda:
            hip.note_torch_path(f"interest_pick over {interests.dtype} / {item_weight.dtype} (the kernels take fp32)")
        item_e = torch.nn.functional.embedding(target, item_weight, padding_idx=0)
        k_index = torch.argmax(torch.bmm(interests, item_e.unsqueeze(-1)), dim=1)
        return interests.gather(1, k_index.view(-1, 1, 1).expand(-1, 1, interests.shape[2])).squeeze(1)
    best = _InterestPick.apply(interests, item_weight, target.contiguous())
    if check_indices == "sync":
        _raise_if_flagged(interests.device, f"Target out of bounds: every target must lie in [0, {item_weight.shape[0]})")
    return best


# ----------------------------------------------------------------------------------------------
# sequence recall: SASRec's masked multi-head self-attention core (models/layers/trainformer.py:70-92 of the reference) and
# the feed-forward activations the GEMM epilogue lacks (trainformer.py:133-145).  Saved between forward and backward: the
# projected rows, the mask, the output and one float per (b, head, query); no [B, heads, L, L] tensor exists on the HIP path.
# ----------------------------------------------------------------------------------------------
def _seq_attention_keypad_reference(q, kv, mask, heads: int, qpos, compact: bool):
    """seq_attention_reference's key-padding mode: layers/sequence.py MultiHeadAttention.scaled_dot_product_attention of the
    reference under masked_fill(mask == 0, -inf), with the maximum subtracted per row (the reference subtracts the maximum
    of the whole batch tensor: equal unless a row's own maximum lies ~87 below it) and its NaN -> 0 for a sample without a
    content key written as a guarded division, so that such a sample passes zero gradients instead of NaN."""
    B, L = mask.shape
    D = kv.shape[1] // 2
    dh = D // heads
    content = (mask != 0).view(B, 1, 1, L)
    key_layer = kv[:, :D].reshape(B, L, heads, dh).permute(0, 2, 3, 1)
    value_layer = kv[:, D:].reshape(B, L, heads, dh).permute(0, 2, 1, 3)
    if qpos is None:
        query_layer = q.reshape(B, L, heads, dh).permute(0, 2, 1, 3)
    else:
        q_rows = q if compact else q.reshape(B, L, -1)[torch.arange(B, device=q.device), qpos.clamp(0, L - 1)]
        query_layer = q_rows[:, :D].reshape(B, 1, heads, dh).permute(0, 2, 1, 3)
    scores = (torch.matmul(query_layer, key_layer) / (dh ** 0.5)).masked_fill(~content, float("-inf"))
    top = scores.detach().max(dim=-1, keepdim=True).values
    e = torch.exp(scores - torch.where(torch.isinf(top), torch.zeros_like(top), top))
    den = e.sum(dim=-1, keepdim=True)
    probs = e / torch.where(den > 0, den, torch.ones_like(den))
    context_layer = torch.matmul(probs, value_layer).permute(0, 2, 1, 3).contiguous()
    if qpos is None:
        return context_layer.view(B * L, D)
    return context_layer.view(B, D) * (qpos >= 0).to(q.dtype).view(B, 1)


def seq_attention_reference(q, kv, mask, heads: int, keep=None, scale: float = 1.0, qpos=None, compact: bool = False,
                            causal: bool = True):
    """The composed formulation, op for op as the reference's MultiHeadAttention.forward between its projections and `dense`,
    in the dtype of its inputs: q [B L, D] (or, with qpos and compact, [B, D]: one row per
    sample), kv [B L, 2 D] (K | V), mask [B, L] -> ctx [B L, D], or [B, D] with qpos (a zero row where qpos[b] < 0).
    keep: the dropout decisions [B, heads, L, L] (any dtype; None: no dropout), scale: 1 / (1 - p).
    causal False: the key-padding mode (every query over every content key, a masked key has probability 0, a sample
    without a content key gives zero rows); no dropout there."""
    if not causal:
        if keep is not None:
            raise ValueError("seq_attention_reference: the key-padding mode has no dropout")
        return _seq_attention_keypad_reference(q, kv, mask, heads, qpos, compact)
    B, L = mask.shape
    D = kv.shape[1] // 2
    dh = D // heads
    content = (mask != 0).to(q.dtype)
    causal = torch.tril(torch.ones(L, L, dtype=q.dtype, device=q.device))
    add = (1.0 - content.view(B, 1, 1, L) * causal.view(1, 1, L, L)) * -1e6  # get_attention_mask: [B, 1, L, L]
    key_layer = kv[:, :D].reshape(B, L, heads, dh).permute(0, 2, 3, 1)
    value_layer = kv[:, D:].reshape(B, L, heads, dh).permute(0, 2, 1, 3)
    if qpos is None:
        query_layer = q.reshape(B, L, heads, dh).permute(0, 2, 1, 3)
    else:
        rows = torch.arange(B, device=q.device)
        idx = qpos.clamp(0, L - 1)
        q_rows = q if compact else q.reshape(B, L, -1)[rows, idx]
        query_layer = q_rows[:, :D].reshape(B, 1, heads, dh).permute(0, 2, 1, 3)
        add = add[rows, 0, idx].view(B, 1, 1, L)
        if keep is not None:
            keep = keep[rows, :, idx].view(B, heads, 1, L)
    attention_scores = torch.matmul(query_layer, key_layer) / (dh ** 0.5) + add
    attention_probs = torch.softmax(attention_scores, dim=-1)
    if keep is not None:
        attention_probs = attention_probs * keep.to(q.dtype) * scale
    context_layer = torch.matmul(attention_probs, value_layer).permute(0, 2, 1, 3).contiguous()
    if qpos is None:
        return context_layer.view(B * L, D)
    return context_layer.view(B, D) * (qpos >= 0).to(q.dtype).view(B, 1)


class _SeqAttention(torch.autograd.Function):
    """inputs: rows = the stacked [B L, 3 D] buffer (q is None) or the [B L, 2 D] K | V buffer (q [B, D]: one query per sample)"""

    @staticmethod
    def forward(ctx, rows, q, mask, qpos, heads: int, p: float, causal: bool = True):
        rows = _unit_inner(rows)
        stacked = q is None
        D = rows.shape[1] // (3 if stacked else 2)
        qv = rows if stacked else _unit_inner(q)
        kv = rows[:, D:] if stacked else rows
        rng = hip.seq_attn_seed_offset(rows.device) if p > 0.0 else None
        out, lse = hip.seq_attn_fwd(qv, kv, mask, heads, p, rng, qpos, compact=not stacked, causal=causal)
        # (the key-padding backward forms its delta from the recomputed probabilities: the output is not kept)
        ctx.save_for_backward(rows, None if stacked else qv, mask, qpos, out if causal else None, lse)
        ctx.cfg = (heads, p, rng, D, causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        rows, q, mask, qpos, out, lse = ctx.saved_tensors
        heads, p, rng, D, causal = ctx.cfg
        if q is None:  # dqkv [B L, 3 D]: dQ | dK | dV, written in place by the one launch
            drows = hip._new((rows.shape[0], 3 * D), torch.float32, rows.device)
            hip.seq_attn_bwd(rows, rows[:, D:], mask, out, dout.contiguous(), lse, heads, p, rng, qpos, dq=drows, dkv=drows[:, D:],
                             causal=causal)
            return drows, None, None, None, None, None, None
        dq, dkv = hip.seq_attn_bwd(q, rows, mask, out, dout.contiguous(), lse, heads, p, rng, qpos, compact=True, causal=causal)
        return dkv, dq, None, None, None, None, None


def seq_attention(qkv: torch.Tensor, mask: torch.Tensor, heads: int, p: float = 0.0, training: bool = False,
                  qpos: torch.Tensor = None, q: torch.Tensor = None, causal: bool = True):
    """The masked multi-head attention core of the reference's TransformerEncoder on already-projected rows:
    qkv [B L, 3 D] (Q | K | V, biases added, head h at columns [h dh, (h + 1) dh) of each), mask [B, L] (non-zero = content, any
    dtype) -> ctx [B L, D], head-interleaved: softmax(Q K^T / sqrt(dh) + m) V per (b, head) with m = 0 where the key is content
    and not behind the query, else -1e6, and dropout (p, when training) on the probabilities.
    qpos int64 [B]: last-row mode, one query position per sample -> ctx [B, D]; qpos[b] < 0 gives a zero row and no gradient.
    With q [B, D] (the query rows themselves, one per sample; needs qpos) qkv holds K | V only, [B L, 2 D].
    On the HIP device one launch each way (rp_seq_attn_*: nothing of size L x L is stored, the backward recomputes the
    probabilities and regenerates the dropout decisions from one offset of the device generator's Philox stream); outside
    rp_seq_attn_fits (L <= 128, dh <= 64) the composed torch formulation on the device, counted; on CPU tensors the same
    formulation.
    causal False: the key-padding mode of the reference's BERT4RecEncoder (rp_seq_attn_keypad_*): every query row attends to
    every content key, a masked key has probability exactly 0 (skipped, no additive score), a sample without a content key
    gets zero rows and passes zero gradients.  That layer has no dropout on the probabilities: p > 0 while training raises
    ValueError."""
    if q is not None and qpos is None:
        raise ValueError("seq_attention: q (one query row per sample) needs qpos")
    B, L = mask.shape
    D = qkv.shape[1] // (3 if q is None else 2)
    if D % heads:
        raise ValueError(f"seq_attention: {D} columns do not split into {heads} heads")
    p = float(p) if training else 0.0
    if not causal and p > 0.0:
        raise ValueError("seq_attention: the key-padding mode (causal=False) has no attention dropout")
    fits = qkv.is_cuda and qkv.dtype == torch.float32 and (q is None or q.dtype == torch.float32) and \
        hip.seq_attn_fits(L, heads, D // heads)
    if not fits:
        if qkv.is_cuda:
            g = hip.seq_attn_geometry()
            hip.note_torch_path(f"seq_attention at L={L}, dh={D // heads}, {qkv.dtype} (the kernel takes fp32, L <= {g['max_l']}, "
                                f"dh <= {g['max_dh']})")
        qr, kv = (qkv[:, :D], qkv[:, D:]) if q is None else (q, qkv)
        keep = None
        if p > 0.0:
            keep = torch.nn.functional.dropout(torch.ones(B, heads, L, L, dtype=qkv.dtype, device=qkv.device), p, True)
        return seq_attention_reference(qr, kv, mask, heads, keep=keep, scale=1.0, qpos=qpos, compact=q is not None, causal=causal)
    if qpos is not None:
        qpos = qpos.to(torch.int64).contiguous()
    return _SeqAttention.apply(qkv, q, mask.to(torch.float32).contiguous(), qpos, heads, p, bool(causal))


SEQ_ACTS = {"gelu": hip.SEQ_ACT_GELU, "swish": hip.SEQ_ACT_SWISH}


class _SeqAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act: int):
        x = _unit_inner(x)
        ctx.act = act
        ctx.save_for_backward(x)
        return hip.seq_act_fwd(x, act)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return hip.seq_act_bwd(_unit_inner(dy), x, ctx.act), None


def seq_act(x: torch.Tensor, name: str):
    """The two feed-forward activations of the reference's FeedForward the GEMM epilogue lacks: 'gelu' (erf form,
    x 0.5 (1 + erf(x / sqrt 2))) and 'swish' (x sigmoid(x)); x [..., N].  On the HIP device one launch each way; on CPU
    tensors the reference's formulas."""
    if name not in SEQ_ACTS:
        raise KeyError(name)
    if not x.is_cuda or x.dtype != torch.float32:
        if x.is_cuda:
            hip.note_torch_path(f"seq_act over {x.dtype} (the kernels take fp32)")
        return x * 0.5 * (1.0 + torch.erf(x / (2.0 ** 0.5))) if name == "gelu" else x * torch.sigmoid(x)
    return _SeqAct.apply(x.reshape(-1, x.shape[-1]), SEQ_ACTS[name]).reshape(x.shape)


class _SeqTake(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, qpos, B: int, L: int):
        ctx.save_for_backward(qpos)
        ctx.dims = (B, L)
        return hip.seq_take_fwd(_unit_inner(x), qpos, B, L)

    @staticmethod
    def backward(ctx, dout):
        (qpos,) = ctx.saved_tensors
        return hip.seq_take_bwd(dout.contiguous(), qpos, *ctx.dims), None, None, None


def seq_take(x: torch.Tensor, qpos: torch.Tensor):
    """x [B, L, D], qpos int64 [B] -> x[b, qpos[b]] as [B, D]; on the HIP device a zero row (and no gradient) where
    qpos[b] < 0, on CPU tensors the reference's gather (SequenceBaseModel.gather_indexes), which raises there."""
    B, L, D = x.shape
    if not x.is_cuda or x.dtype != torch.float32:
        if x.is_cuda:
            hip.note_torch_path(f"seq_take over {x.dtype} (the kernels take fp32)")
        return x.gather(dim=1, index=qpos.view(-1, 1, 1).expand(-1, -1, D)).squeeze(1)
    return _SeqTake.apply(x.reshape(B * L, D), qpos.to(torch.int64).contiguous(), B, L)


# ----------------------------------------------------------------------------------------------
# sequence recall: one residual block of NextItNet (models/layers/conv.py: ResBlockTwoMasked / ResBlockOneMasked) as ONE
# autograd node; the forward keeps the block's input and nothing else (csrc/causal_conv.hip)
# ----------------------------------------------------------------------------------------------
class _CausalConvBlock(torch.autograd.Function):
    """inputs: x, lens, k, dilation, one_masked, last, then the block's 12 parameter slots (None where it has none)"""

    @staticmethod
    def forward(ctx, x, lens, k: int, dilation: int, one_masked: bool, last: bool, *params):
        x = x.contiguous()
        ps = [None if p is None else p.contiguous() for p in params]
        ctx.cfg = (k, dilation, one_masked, last)
        ctx.have = [p is not None for p in ps]
        ctx.save_for_backward(x, lens, *[p for p in ps if p is not None])
        return hip.causal_conv_fwd(x, lens, ps, k, dilation, one_masked, last)

    @staticmethod
    def backward(ctx, dout):
        x, lens, *held = ctx.saved_tensors
        it = iter(held)
        ps = [next(it) if h else None for h in ctx.have]
        dx, grads = hip.causal_conv_bwd(x, lens, dout.contiguous(), ps, *ctx.cfg)
        return (dx, None, None, None, None, None, *grads)


def causal_conv_block_reference(x, lens, block, last: bool):
    """the block in torch ops (the reference's formulas, any device and dtype): rows at positions >= lens read as zero"""
    B, L, _ = x.shape
    behind = torch.arange(L, device=x.device).unsqueeze(0) >= lens.unsqueeze(-1)
    y = block(torch.masked_fill(x, behind.unsqueeze(-1), 0).transpose(1, 2))
    if last:
        return y[torch.arange(B, device=x.device), :, lens - 1]  # (lens = 0 reads position L - 1)
    return y.transpose(1, 2)


def causal_conv_block(x: torch.Tensor, lens: torch.Tensor, block, last: bool):
    """One residual block of NextItNet over x [B, L, C] with lengths lens int64 [B] (rows at positions >= lens[b] are read as
    zero; the residual adds the row as read).  last = False -> [B, L, C], every position; last = True -> [B, C], the block's
    output at position lens[b] - 1 (L - 1 for lens[b] = 0), computed on the HIP device from the few rows it depends on.
    `block`: a ResBlockTwoMasked / ResBlockOneMasked (the parameter holder).  One rp_causal_conv_fwd / _bwd per call on the
    HIP device inside the kernel's limits; the torch formulas on CPU tensors and, counted, outside the limits."""
    if not x.is_cuda:
        return causal_conv_block_reference(x, lens, block, last)
    B, L, Cw = x.shape
    lens = lens.to(torch.int64).contiguous()
    k, d = block.kernel_size, block.dilation
    if x.dtype != torch.float32 or d < 1 or not hip.causal_conv_fits(L, Cw, k, block.one_masked):
        hip.note_torch_path(f"causal_conv_block at L={L}, C={Cw}, k={k}, {x.dtype} (the kernel takes fp32 inside "
                            f"{hip.causal_conv_geometry()})")
        return causal_conv_block_reference(x, lens.clamp(0, L), block, last)
    return _CausalConvBlock.apply(x, lens, int(k), int(d), bool(block.one_masked), bool(last), *block.stage_params())


# ----------------------------------------------------------------------------------------------
# sequence recall: the session graphs of SRGNN / NISER / GCSAN (models/utils.py: generate_graph), their gated graph cell
# (models/layers/graph.py: SRGNNConv, SRGNNCell) and the row L2 normalisation of NISER (csrc/session_graph.hip).
# Sample b keeps its nodes in its own L slots: node v is row b L + v of [B, L, ...].  A step is ONE autograd node that keeps
# its input and nothing else; the graph is the alias list.
# ----------------------------------------------------------------------------------------------
def session_graph(hist: torch.Tensor):
    """hist int64 [B, L] -> (nodes int64 [B, L], alias int32 [B, L], count int32 [B], indeg int32 [B, L], outdeg int32 [B, L]).
    Per sample, over its items with id > 0 in order s_0 .. s_{n-1}: nodes = the distinct ids ascending (torch.unique's order), 0
    behind the node count; alias[l] = the node number of s_l, -1 for l >= n; transition l is alias[l] -> alias[l + 1], and the
    degrees count the multiset of the n - 1 transitions.  On the HIP device one rp_session_graph launch (no host copy of the
    lengths); on CPU tensors, and counted beyond the kernel's L, batched torch ops that give the same integers."""
    if hist.dim() != 2:
        raise RuntimeError(f"session_graph: hist must be [B, L], got {tuple(hist.shape)}")
    L = hist.shape[1]
    if hist.is_cuda:
        if L <= hip.session_graph_geometry()["max_l"]:
            return hip.session_graph(hist.to(torch.int64).contiguous())
        hip.note_torch_path(f"session_graph at L={L} (the kernel takes L <= {hip.session_graph_geometry()['max_l']})")
    return session_graph_reference(hist)


def session_graph_reference(hist: torch.Tensor):
    """session_graph in batched torch ops (any device): a stable sort moves the items with id > 0 to the front, a node number
    is the count of smaller first occurrences, degrees are scatter_adds of integers"""
    B, L = hist.shape
    hist = hist.to(torch.int64)
    dev = hist.device
    valid = hist > 0
    n = valid.sum(1)
    pos = torch.arange(L, device=dev).unsqueeze(0)
    order = torch.sort((~valid).to(torch.int8), dim=1, stable=True).indices  # the items with id > 0 first, in order
    inside = pos < n.unsqueeze(1)
    s = torch.where(inside, hist.gather(1, order), torch.zeros_like(hist))
    same = (s.unsqueeze(2) == s.unsqueeze(1)) & torch.ones(L, L, dtype=torch.bool, device=dev).tril(-1)  # [b, j, k]: k < j
    first = inside & ~same.any(2)
    rank = ((s.unsqueeze(1) < s.unsqueeze(2)) & first.unsqueeze(1)).sum(2)  # [b, i] = #{j first: s_j < s_i}
    alias = torch.where(inside, rank, torch.full_like(rank, -1))
    nodes = torch.zeros(B, L + 1, dtype=torch.int64, device=dev)
    nodes.scatter_(1, torch.where(first, rank, torch.full_like(rank, L)), s)  # (column L collects what is no first occurrence)
    nodes = nodes[:, :L].contiguous()
    a = alias.clamp(min=0)
    leaves = (pos < (n - 1).unsqueeze(1)).to(torch.int64)  # position l starts a transition
    ends = (inside & (pos > 0)).to(torch.int64)            # position l ends one
    outdeg = torch.zeros(B, L, dtype=torch.int64, device=dev).scatter_add_(1, a, leaves)
    indeg = torch.zeros(B, L, dtype=torch.int64, device=dev).scatter_add_(1, a, ends)
    return nodes, alias.to(torch.int32), first.sum(1).to(torch.int32), indeg.to(torch.int32), outdeg.to(torch.int32)


def _cell_params(cell):
    return [cell.incomming_conv.lin.weight, cell.incomming_conv.lin.bias, cell.outcomming_conv.lin.weight,
            cell.outcomming_conv.lin.bias, cell.lin_ih.weight, cell.lin_ih.bias, cell.lin_hh.weight, cell.lin_hh.bias]


def ggnn_cell_reference(h, alias, params, final: bool):
    """one step of the cell in torch ops over the padded [B, L, D] layout (any device and dtype): the reference's formulas with
    the message passing written as gather / scatter_add over the sample's transitions"""
    w_in, b_in, w_out, b_out, w_ih, b_ih, w_hh, b_hh = params
    B, L, D = h.shape
    dev = h.device
    a = alias.clamp(min=0).to(torch.int64)
    n = (alias >= 0).sum(1)
    cnt = (alias.max(dim=1).values.to(torch.int64) + 1).clamp(min=0)
    pos = torch.arange(L, device=dev).unsqueeze(0)
    node = (pos < cnt.unsqueeze(1)).to(h.dtype).unsqueeze(-1)
    h = h * node
    src, dst = a[:, :-1], a[:, 1:]
    em = (pos[:, :L - 1] < (n - 1).unsqueeze(1)).to(h.dtype)
    outdeg = torch.zeros(B, L, dtype=h.dtype, device=dev).scatter_add(1, src, em)
    indeg = torch.zeros(B, L, dtype=h.dtype, device=dev).scatter_add(1, dst, em)
    src_d, dst_d = src.unsqueeze(-1).expand(-1, -1, D), dst.unsqueeze(-1).expand(-1, -1, D)
    p_in = torch.nn.functional.linear(h, w_in, b_in)
    p_out = torch.nn.functional.linear(h, w_out, b_out)
    m_in = p_in.gather(1, src_d) * (em / outdeg.gather(1, src).clamp(min=1)).unsqueeze(-1)
    m_out = p_out.gather(1, dst_d) * (em / indeg.gather(1, dst).clamp(min=1)).unsqueeze(-1)
    agg_in = torch.zeros_like(h).scatter_add(1, dst_d, m_in)
    agg_out = torch.zeros_like(h).scatter_add(1, src_d, m_out)
    gi = torch.nn.functional.linear(torch.cat([agg_in, agg_out], dim=-1), w_ih, b_ih)
    gh = torch.nn.functional.linear(h, w_hh, b_hh)
    i_r, i_i, i_n = gi.chunk(3, -1)
    h_r, h_i, h_n = gh.chunk(3, -1)
    reset_gate = torch.sigmoid(i_r + h_r)
    input_gate = torch.sigmoid(i_i + h_i)
    new_gate = torch.tanh(i_n + reset_gate * h_n)
    hy = ((1 - input_gate) * h + input_gate * new_gate) * node
    if not final:
        return hy
    seq = hy.gather(1, a.unsqueeze(-1).expand(-1, -1, D)) * (alias >= 0).to(h.dtype).unsqueeze(-1)
    ht = seq.gather(1, (n - 1).clamp(min=0).view(-1, 1, 1).expand(-1, 1, D)).squeeze(1) * (n > 0).to(h.dtype).unsqueeze(-1)
    return seq, ht


class _GGNNCell(torch.autograd.Function):
    """inputs: h, alias, final, then the cell's 8 parameters; saved: h, alias and the parameters themselves"""

    @staticmethod
    def forward(ctx, h, alias, final: bool, *params):
        ctx.set_materialize_grads(False)
        h = h.contiguous()
        ps = [p.contiguous() for p in params]
        ctx.final = final
        ctx.save_for_backward(h, alias, *ps)
        return hip.ggnn_cell_fwd(h, alias, ps, final)

    @staticmethod
    def backward(ctx, *douts):
        h, alias, *ps = ctx.saved_tensors
        douts = [None if d is None else d.contiguous() for d in douts]
        if all(d is None for d in douts):
            return (None,) * (3 + len(ps))
        if ctx.final:
            dh, grads = hip.ggnn_cell_bwd(h, alias, ps, dseq=douts[0], dht=douts[1])
        else:
            dh, grads = hip.ggnn_cell_bwd(h, alias, ps, dhout=douts[0])
        return (dh, None, None, *grads)


def ggnn_cell(h: torch.Tensor, alias: torch.Tensor, cell, final: bool = False):
    """One step of the session-graph gated cell (`cell`: an SRGNNCell, the parameter holder) over node states h [B, L, D]
    (node v of sample b at row v of its L slots, rows behind the node count read as zero) on the graphs alias int32 [B, L]
    describes (session_graph's).  final = False -> h' [B, L, D], zero behind the node count; final = True -> the last step's
    read-back in sequence order: (seq_hidden [B, L, D] with row l = h'[alias[l]] and ZERO rows at padding, ht [B, D] =
    seq_hidden at the last item, zero for a sample without items).  One rp_ggnn_cell_fwd / _bwd per call on the HIP device
    inside the kernel's limits; ggnn_cell_reference on CPU tensors and, counted, outside the limits."""
    params = _cell_params(cell)
    if not h.is_cuda:
        return ggnn_cell_reference(h, alias, params, final)
    B, L, D = h.shape
    if h.dtype != torch.float32 or not hip.ggnn_fits(L, D):
        hip.note_torch_path(f"ggnn_cell at L={L}, D={D}, {h.dtype} (the kernel takes fp32 inside {hip.ggnn_geometry()})")
        return ggnn_cell_reference(h, alias, params, final)
    return _GGNNCell.apply(h, alias.to(torch.int32).contiguous(), bool(final), *params)


class _L2Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return hip.l2norm_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return hip.l2norm_bwd(x, dy.contiguous())


def l2_normalize(x: torch.Tensor, eps: float = 1e-12):
    """F.normalize(x, dim=-1): x / max(|x|_2, eps) over the last axis, any leading shape.  A row of zeros stays zero and passes a
    ZERO gradient (F.normalize passes dy / eps there: the padded node rows of a session are such rows, and nothing reads
    them).  On the HIP device rp_l2norm_fwd / _bwd (eps is the kernel's 1e-12); torch ops on CPU tensors."""
    if not x.is_cuda or x.dtype != torch.float32 or eps != 1e-12:
        if x.is_cuda:
            hip.note_torch_path(f"l2_normalize over {x.dtype}, eps={eps} (the kernels take fp32 at eps 1e-12)")
        nrm = x.norm(dim=-1, keepdim=True)
        return x * torch.where(nrm > 0, 1.0 / nrm.clamp_min(eps), torch.zeros_like(nrm))
    return _L2Normalize.apply(x.reshape(-1, x.shape[-1])).reshape(x.shape)


# ----------------------------------------------------------------------------------------------
# sequence recall: two-layer additive attention over the history's rows + pooling of those rows — STAMPLayer's attention
# (models/layers/sequence.py:131-137) and MultiInterestSelfAttention (models/layers/multi_interest.py:37-51) as ONE autograd
# node (csrc/attn_pool.hip).  Saved between forward and backward: the inputs and the weights A [B, L, K];
# the hidden tensor [B, L, Dh] exists on neither side.
# ----------------------------------------------------------------------------------------------
_ATTN_POOL_ACTS = {"sigmoid": ACT_SIGMOID, "tanh": ACT_TANH}
_ATTN_POOL_NORMS = {"mask": hip.ATTN_POOL_MASK, "softmax": hip.ATTN_POOL_SOFTMAX}


def attention_pool_reference(x, w1, w2, valid, bias=None, act: str = "tanh", norm: str = "softmax", return_weights: bool = False):
    """attention_pool in torch ops (any device and dtype): materialises the hidden tensor [B, L, Dh].  The score of a
    position with valid = 0 is the constant -1e9 under norm = "softmax" (what the reference's fp32 `S + -1e9` rounds to
    for |S| < 32), so no gradient passes to S there."""
    if act not in _ATTN_POOL_ACTS or norm not in _ATTN_POOL_NORMS:
        raise ValueError(f"attention_pool: act must be one of {sorted(_ATTN_POOL_ACTS)} and norm of {sorted(_ATTN_POOL_NORMS)}")
    pre = torch.matmul(x, w1)
    if bias is not None:
        pre = pre + bias.unsqueeze(1)
    hidden = torch.sigmoid(pre) if act == "sigmoid" else torch.tanh(pre)
    s = torch.matmul(hidden, w2)  # [B, L, K]
    v = valid.to(x.dtype).unsqueeze(-1)
    if norm == "mask":
        a = s * v
    else:
        a = torch.softmax(torch.where(v != 0, s, torch.full_like(s, -1e9)), dim=1)
    out = torch.matmul(a.transpose(1, 2), x)
    return (out, a) if return_weights else out


class _AttentionPool(torch.autograd.Function):
    """inputs: x, valid, w1, w2, bias | None, act, norm; saved: those tensors and A"""

    @staticmethod
    def forward(ctx, x, valid, w1, w2, bias, act: int, norm: int):
        x, valid, w1, w2 = x.contiguous(), valid.contiguous(), w1.contiguous(), w2.contiguous()
        bias = None if bias is None else bias.contiguous()
        out, A = hip.attn_pool_fwd(x, valid, w1, w2, bias, act, norm)
        ctx.cfg = (act, norm, bias is not None)
        ctx.save_for_backward(x, valid, w1, w2, A, *(() if bias is None else (bias,)))
        return out

    @staticmethod
    def backward(ctx, dout):
        act, norm, has_bias = ctx.cfg
        x, valid, w1, w2, A, *rest = ctx.saved_tensors
        bias = rest[0] if has_bias else None
        dx, dw1, dw2, dc = hip.attn_pool_bwd(x, valid, w1, w2, bias, A, dout.contiguous(), act, norm)
        return dx, None, dw1, dw2, dc, None, None


def attention_pool(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, valid: torch.Tensor, bias=None, act: str = "tanh",
                   norm: str = "softmax"):
    """out[b, k, :] = sum_l A[b, l, k] x[b, l, :] with S = act(x w1 + bias[:, None]) w2 and A = S valid (norm "mask") or the
    softmax over l of (valid ? S : -1e9) (norm "softmax"): x [B, L, D], w1 [D, Dh], w2 [Dh, K], valid [B, L] of 0 / 1 (any
    dtype), bias [B, Dh] or None, act "sigmoid" | "tanh" -> [B, K, D].  Rows of x at valid = 0 are read as they are.  Under
    "mask" a sample without a valid position gives zeros; under "softmax" it pools uniformly over all L rows (the
    reference's behaviour) and passes no gradient to the scores.  One rp_attn_pool_fwd / _bwd per call on the HIP device
    inside the kernel's limits; attention_pool_reference on CPU tensors and, counted, outside the limits."""
    if act not in _ATTN_POOL_ACTS or norm not in _ATTN_POOL_NORMS:
        raise ValueError(f"attention_pool: act must be one of {sorted(_ATTN_POOL_ACTS)} and norm of {sorted(_ATTN_POOL_NORMS)}")
    if not x.is_cuda:
        return attention_pool_reference(x, w1, w2, valid, bias, act, norm)
    B, L, D = x.shape
    Dh, K = w2.shape
    if x.dtype != torch.float32 or not hip.attn_pool_fits(L, D, Dh, K):
        hip.note_torch_path(f"attention_pool at L={L}, D={D}, Dh={Dh}, K={K}, {x.dtype} (the kernel takes fp32 inside "
                            f"{hip.attn_pool_geometry()})")
        return attention_pool_reference(x, w1, w2, valid, bias, act, norm)
    return _AttentionPool.apply(x, valid.to(torch.float32), w1, w2, bias, _ATTN_POOL_ACTS[act], _ATTN_POOL_NORMS[norm])


# ----------------------------------------------------------------------------------------------
# sequence recall: the in-batch contrastive loss of CLRec (models/sequence/clrec.py:65-102 of the reference) and ContraRec
# (contrarec.py:93-144) as ONE autograd node (csrc/contrast.hip).  Saved between forward and backward: the
# inputs, lse [n] (float64) and the positive counts c [n]; no [n, m] tensor exists on the HIP path.
# ----------------------------------------------------------------------------------------------
def contrastive_loss_reference(a, b, labels_a, labels_b, temperature: float, exclude_self: bool = False, scale: float = 1.0,
                               return_lse: bool = False):
    """contrastive_loss in torch ops, op for op as the reference's two ContraLoss modules (any device and dtype):
    materialises the [n, m] matrix several times.  b None: the symmetric form (b = a, labels_b = labels_a)."""
    if b is None:
        b, labels_b = a, labels_a
    elif exclude_self:
        raise ValueError("contrastive_loss: exclude_self belongs to the symmetric form (b=None)")
    n, m = a.shape[0], b.shape[0]
    dot = torch.matmul(a, b.transpose(0, 1)) / temperature
    logits_max, _ = torch.max(dot, dim=1, keepdim=True)
    logits = dot - logits_max.detach()
    mask = torch.eq(labels_a.view(-1, 1), labels_b.view(1, -1)).to(a.dtype)
    logits_mask = torch.ones_like(mask)
    if exclude_self:
        logits_mask = torch.scatter(logits_mask, 1, torch.arange(n, device=a.device).view(-1, 1), 0)
    mask = mask * logits_mask
    exp_logits = torch.exp(logits) * logits_mask
    log_denominator = torch.log(exp_logits.sum(1, keepdim=True) + 1e-10)
    log_prob = logits - log_denominator
    mean_log_prob_pos = (mask * log_prob).sum(1) / (mask.sum(1) + 1e-10)
    loss = (-scale * mean_log_prob_pos).mean()
    if return_lse:
        return loss, (logits_max + log_denominator).view(-1).detach()
    return loss


class _ContrastiveLoss(torch.autograd.Function):
    """inputs: a, b | None, labels_a, labels_b | None; saved: those, lse and c"""

    @staticmethod
    def forward(ctx, a, b, la, lb, temperature: float, exclude_self: bool, scale: float):
        a = _unit_inner(a)
        b = None if b is None else _unit_inner(b)
        loss, lse, c = hip.contrast_fwd(a, b, la, lb, temperature, exclude_self, scale)
        ctx.cfg = (temperature, exclude_self, scale, b is not None)
        ctx.save_for_backward(a, la, lse, c, *(() if b is None else (b, lb)))
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        temperature, exclude_self, scale, has_b = ctx.cfg
        a, la, lse, c, *rest = ctx.saved_tensors
        b, lb = rest if has_b else (None, None)
        da, db = hip.contrast_bwd(a, b, la, lb, lse, c, g.reshape(1).float().contiguous(), temperature, exclude_self, scale,
                                  ctx.needs_input_grad[0], has_b and ctx.needs_input_grad[1])
        return da, db, None, None, None, None, None


def contrastive_loss(a: torch.Tensor, b, labels_a: torch.Tensor, labels_b, temperature: float, exclude_self: bool = False,
                     scale: float = 1.0):
    """The in-batch contrastive loss: with l_ij = (a_i . b_j) / temperature, N_i = all j (exclude_self: all j != i),
    P_i = { j in N_i : labels_a[i] == labels_b[j] } and c_i = |P_i|,
        lse_i = m_i + log(sum_{j in N_i} exp(l_ij - m_i) + 1e-10),  m_i = max_j l_ij over all j,
        loss  = (scale / n) sum_i -(sum_{j in P_i} (l_ij - lse_i)) / (c_i + 1e-10)      (a row without positives adds 0).
    a [n, D], b [m, D], labels int64 [n] / [m]; b = None (then labels_b = None too) is the symmetric form over a's own rows,
    the only one that takes exclude_self.  CLRec: a = user rows, b = target rows, labels arange(B), scale 1; ContraRec:
    symmetric over cat(view1, view2), labels cat(target, target), exclude_self, scale = temperature.
    On the HIP device rp_contrast_fwd / _bwd (no [n, m] tensor, the backward recomputes from lse; bit-identical runs) for
    fp32 rows up to D = 128; outside, the composed torch formulation on the device, counted; on CPU tensors the same
    formulation (contrastive_loss_reference)."""
    if b is None:
        if labels_b is not None:
            raise ValueError("contrastive_loss: the symmetric form (b=None) takes no labels_b")
    elif exclude_self:
        raise ValueError("contrastive_loss: exclude_self belongs to the symmetric form (b=None)")
    if not (temperature > 0):
        raise ValueError("contrastive_loss: the temperature must be positive")
    if not a.is_cuda:
        return contrastive_loss_reference(a, b, labels_a, labels_b, temperature, exclude_self, scale)
    D = a.shape[1]
    if a.dtype != torch.float32 or (b is not None and b.dtype != torch.float32) or not hip.contrast_fits(D):
        hip.note_torch_path(f"contrastive_loss at D={D}, {a.dtype} (the kernels take fp32 up to "
                            f"D={hip.contrast_geometry()['max_d']})")
        return contrastive_loss_reference(a, b, labels_a, labels_b, temperature, exclude_self, scale)
    la = labels_a.reshape(-1).to(torch.int64).contiguous()
    lb = None if b is None else labels_b.reshape(-1).to(torch.int64).contiguous()
    return _ContrastiveLoss.apply(a, b, la, lb, float(temperature), bool(exclude_self), float(scale))
