"""TransformerEncoder and its parts — drop-ins for rec_pangu/models/layers/trainformer.py: the same constructor signatures,
attributes, state_dict keys (`layer.{i}.multi_head_attention.{query,key,value,dense,LayerNorm}.*`,
`layer.{i}.feed_forward.{dense_1,dense_2,LayerNorm}.*`) and init RNG stream (one TransformerLayer is built and deep-copied
n_layers times).

What the mask argument is decides the path:
  - a [B, 1, L, L] additive mask (the reference's get_attention_mask output): the reference's torch formulas, op for op —
    on the CPU that is the path, on the HIP device it is the composed formulation, counted in hip.torch_path_count();
  - a [B, L] content mask (non-zero = content, any dtype), on the HIP device: per layer ONE GEMM on stack_rows([Wq, Wk, Wv])
    with the three biases, Fh.seq_attention (the causal + padding mask, the softmax, the attention dropout and P V as one
    launch each way, nothing of size L x L in memory), `dense`, Fh.dropout, the residual and Fh.layer_norm; then dense_1 with
    its activation (the GEMM epilogue for relu / tanh / sigmoid, Fh.seq_act for gelu / swish), dense_2, dropout, residual,
    LayerNorm.  On the CPU the same mask is turned into the additive one first.

encode_last(x, mask) returns only output[b, len_b - 1] ([B, D], len_b = sum(mask[b])): what SASRec reads.  On the HIP device
its FINAL layer runs in last-row mode: K and V are projected for all positions, but Q, the attention row, `dense`, both
LayerNorms and the feed-forward run for B rows instead of B L.  A sample with len_b = 0 gives a zero row there and takes no
gradient; on the CPU the gather raises, as the reference's does.
"""
import copy
import math

import torch
from torch import nn
import torch.nn.functional as fn

from ... import functional as Fh

_EPILOGUE_ACTS = {"relu": Fh.ACT_RELU, "tanh": Fh.ACT_TANH, "sigmoid": Fh.ACT_SIGMOID}


def additive_attention_mask(mask: torch.Tensor) -> torch.Tensor:
    """[B, L] content mask -> the reference's [B, 1, L, L] additive mask (base_model.py:164-193): 0 where key j <= i is
    content, -1e6 elsewhere"""
    extended = mask.unsqueeze(1).unsqueeze(2)
    max_len = mask.size(-1)
    subsequent = torch.triu(torch.ones((1, max_len, max_len), dtype=torch.uint8), diagonal=1)
    subsequent = (subsequent == 0).unsqueeze(1).type_as(mask)
    return (1.0 - extended * subsequent) * -1e6


def _stack_bias(linears):
    return Fh.stack_rows([m.bias.view(-1, 1) for m in linears]).view(-1)


class MultiHeadAttention(nn.Module):
    """Multi-head self-attention with dropout on the probabilities, `dense`, dropout, residual, LayerNorm."""

    def __init__(self, n_heads, hidden_size, hidden_dropout_prob, attn_dropout_prob, layer_norm_eps):
        super(MultiHeadAttention, self).__init__()
        if hidden_size % n_heads != 0:
            raise ValueError(
                "The hidden size (%d) is not a multiple of the number of attention "
                "heads (%d)" % (hidden_size, n_heads)
            )

        self.num_attention_heads = n_heads
        self.attention_head_size = int(hidden_size / n_heads)
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        self.sqrt_attention_head_size = math.sqrt(self.attention_head_size)

        self.query = nn.Linear(hidden_size, self.all_head_size)
        self.key = nn.Linear(hidden_size, self.all_head_size)
        self.value = nn.Linear(hidden_size, self.all_head_size)

        self.softmax = nn.Softmax(dim=-1)
        self.attn_dropout = nn.Dropout(attn_dropout_prob)

        self.dense = nn.Linear(hidden_size, hidden_size)
        self.LayerNorm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        self.out_dropout = nn.Dropout(hidden_dropout_prob)

    def transpose_for_scores(self, x):
        new_x_shape = x.size()[:-1] + (self.num_attention_heads, self.attention_head_size)
        return x.view(*new_x_shape)

    def _forward_torch(self, input_tensor, attention_mask):
        """trainformer.py:65-97"""
        query_layer = self.transpose_for_scores(self.query(input_tensor)).permute(0, 2, 1, 3)
        key_layer = self.transpose_for_scores(self.key(input_tensor)).permute(0, 2, 3, 1)
        value_layer = self.transpose_for_scores(self.value(input_tensor)).permute(0, 2, 1, 3)
        attention_scores = torch.matmul(query_layer, key_layer)
        attention_scores = attention_scores / self.sqrt_attention_head_size
        attention_scores = attention_scores + attention_mask
        attention_probs = self.softmax(attention_scores)
        attention_probs = self.attn_dropout(attention_probs)
        context_layer = torch.matmul(attention_probs, value_layer)
        context_layer = context_layer.permute(0, 2, 1, 3).contiguous()
        context_layer = context_layer.view(*(context_layer.size()[:-2] + (self.all_head_size,)))
        hidden_states = self.dense(context_layer)
        hidden_states = self.out_dropout(hidden_states)
        return self.LayerNorm(hidden_states + input_tensor)

    def _finish_hip(self, context, residual):
        hidden_states = Fh.linear_act(context, self.dense.weight, self.dense.bias)
        if self.training and self.out_dropout.p > 0:
            hidden_states = Fh.dropout(hidden_states, self.out_dropout.p)
        return Fh.layer_norm(hidden_states + residual, self.LayerNorm)

    def forward(self, input_tensor, attention_mask, qpos=None):
        """input_tensor [B, L, D]; attention_mask: [B, 1, L, L] additive or [B, L] content (see the module's text).  qpos
        (int64 [B], HIP device and a content mask only): one query position per sample -> [B, D]."""
        if attention_mask.dim() != 2 or not input_tensor.is_cuda:
            if qpos is not None:
                raise ValueError("MultiHeadAttention: qpos needs a [B, L] content mask on the HIP device")
            if attention_mask.dim() == 2:
                attention_mask = additive_attention_mask(attention_mask)
            elif input_tensor.is_cuda:
                Fh.hip.note_torch_path("MultiHeadAttention with a [B, 1, L, L] additive mask (the kernel takes the [B, L] "
                                       "content mask)")
            return self._forward_torch(input_tensor, attention_mask)
        B, L, D = input_tensor.shape
        heads, p = self.num_attention_heads, self.attn_dropout.p
        rows = input_tensor.reshape(B * L, D)
        if qpos is None:
            qkv = Fh.linear_act(rows, Fh.stack_rows([self.query.weight, self.key.weight, self.value.weight]),
                                _stack_bias([self.query, self.key, self.value]))
            context = Fh.seq_attention(qkv, attention_mask, heads, p, self.training)
            return self._finish_hip(context, rows).reshape(B, L, D)
        kv = Fh.linear_act(rows, Fh.stack_rows([self.key.weight, self.value.weight]), _stack_bias([self.key, self.value]))
        last = Fh.seq_take(input_tensor, qpos)
        q = Fh.linear_act(last, self.query.weight, self.query.bias)
        context = Fh.seq_attention(kv, attention_mask, heads, p, self.training, qpos=qpos, q=q)
        return self._finish_hip(context, last)


class FeedForward(nn.Module):
    """Point-wise feed-forward layer: two dense layers, dropout, residual, LayerNorm."""

    def __init__(self, hidden_size, inner_size, hidden_dropout_prob, hidden_act, layer_norm_eps):
        super(FeedForward, self).__init__()
        self.dense_1 = nn.Linear(hidden_size, inner_size)
        self.hidden_act = hidden_act
        self.intermediate_act_fn = self.get_hidden_act(hidden_act)

        self.dense_2 = nn.Linear(inner_size, hidden_size)
        self.LayerNorm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)
        self.dropout = nn.Dropout(hidden_dropout_prob)

    def get_hidden_act(self, act):
        ACT2FN = {
            "gelu": self.gelu,
            "relu": fn.relu,
            "swish": self.swish,
            "tanh": torch.tanh,
            "sigmoid": torch.sigmoid,
        }
        return ACT2FN[act]

    def gelu(self, x):
        """the erf form (OpenAI GPT's tanh form gives slightly different results)"""
        return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))

    def swish(self, x):
        return x * torch.sigmoid(x)

    def forward(self, input_tensor):
        if not input_tensor.is_cuda:
            hidden_states = self.dense_1(input_tensor)
            hidden_states = self.intermediate_act_fn(hidden_states)
            hidden_states = self.dense_2(hidden_states)
            hidden_states = self.dropout(hidden_states)
            return self.LayerNorm(hidden_states + input_tensor)
        code = _EPILOGUE_ACTS.get(self.hidden_act)
        if code is not None:
            hidden_states = Fh.linear_act(input_tensor, self.dense_1.weight, self.dense_1.bias, act=code)
        else:
            hidden_states = Fh.seq_act(Fh.linear_act(input_tensor, self.dense_1.weight, self.dense_1.bias), self.hidden_act)
        hidden_states = Fh.linear_act(hidden_states, self.dense_2.weight, self.dense_2.bias)
        if self.training and self.dropout.p > 0:
            hidden_states = Fh.dropout(hidden_states, self.dropout.p)
        return Fh.layer_norm(hidden_states + input_tensor, self.LayerNorm)


class TransformerLayer(nn.Module):
    """One transformer layer: a multi-head self-attention sublayer and a point-wise feed-forward sublayer."""

    def __init__(self, n_heads, hidden_size, intermediate_size, hidden_dropout_prob, attn_dropout_prob, hidden_act,
                 layer_norm_eps):
        super(TransformerLayer, self).__init__()
        self.multi_head_attention = MultiHeadAttention(
            n_heads, hidden_size, hidden_dropout_prob, attn_dropout_prob, layer_norm_eps
        )
        self.feed_forward = FeedForward(hidden_size, intermediate_size, hidden_dropout_prob, hidden_act, layer_norm_eps)

    def forward(self, hidden_states, attention_mask, qpos=None):
        if qpos is None:
            attention_output = self.multi_head_attention(hidden_states, attention_mask)
        else:
            attention_output = self.multi_head_attention(hidden_states, attention_mask, qpos=qpos)
        return self.feed_forward(attention_output)


class TransformerEncoder(nn.Module):
    r"""n_layers TransformerLayers (the reference's defaults: 2 layers, 2 heads, hidden_size 64, inner_size 256, both dropouts
    0.5, 'gelu' of 'gelu', 'relu', 'swish', 'tanh', 'sigmoid', layer_norm_eps 1e-12)."""

    def __init__(self, n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=0.5, attn_dropout_prob=0.5,
                 hidden_act="gelu", layer_norm_eps=1e-12):
        super(TransformerEncoder, self).__init__()
        layer = TransformerLayer(n_heads, hidden_size, inner_size, hidden_dropout_prob, attn_dropout_prob, hidden_act,
                                 layer_norm_eps)
        self.layer = nn.ModuleList([copy.deepcopy(layer) for _ in range(n_layers)])

    def forward(self, hidden_states, attention_mask, output_all_encoded_layers=True):
        """-> the list of all layers' outputs, or of the last one only"""
        all_encoder_layers = []
        for layer_module in self.layer:
            hidden_states = layer_module(hidden_states, attention_mask)
            if output_all_encoded_layers:
                all_encoder_layers.append(hidden_states)
        if not output_all_encoded_layers:
            all_encoder_layers.append(hidden_states)
        return all_encoder_layers

    def encode_last(self, hidden_states, mask):
        """hidden_states [B, L, D], mask [B, L] (non-zero = content) -> output[b, len_b - 1] of the last layer, [B, D]"""
        last = torch.sum(mask, dim=-1).to(torch.int64) - 1
        if not hidden_states.is_cuda or len(self.layer) == 0:
            output = self.forward(hidden_states, mask, output_all_encoded_layers=False)[-1]
            index = last.view(-1, 1, 1).expand(-1, -1, output.shape[-1])
            return output.gather(dim=1, index=index).squeeze(1)
        for layer_module in self.layer[:-1]:
            hidden_states = layer_module(hidden_states, mask)
        output = self.layer[-1](hidden_states, mask, qpos=last)
        # a sample without history: the attention row is zero there, but `dense`, the LayerNorms and the feed-forward would
        # turn it into their biases' image; the row is defined as zero and takes no gradient
        return output * (last >= 0).to(output.dtype).view(-1, 1)
