"""NextItNet's encoder — drop-in for rec_pangu/models/layers/conv.py (constructor signatures, parameter names, shapes and
creation order as there, so state_dict keys and the init stream match).

    NextItNetLayer(emb_seqs [B, L, C], lens [B]) -> [B, C]: rows at positions >= lens zeroed, a stack of residual blocks of
    dilated causal convolutions on [B, C, L], the row at lens - 1 (lens = 0 reads position L - 1, as indexing with -1 does).

On the HIP device every block is one Fh.causal_conv_block node (csrc/causal_conv.hip): every block but the
final one in full mode, the final one in last mode — it computes the one row per sample that is read from the few rows it
depends on.  `last_mode = False` on the layer forces the final block to full mode too (tests and the microbenchmark).  On the
CPU, and on the device outside the kernel's limits (counted, hip.note_torch_path), the reference's torch formulas.
"""
from typing import List

import torch
from torch import nn

from ... import functional as Fh


class LayerNorm(nn.Module):
    """over the channel axis of [B, C, L] at each position, biased variance; gamma / beta are [1, C, 1]"""

    def __init__(self, channels: int, epsilon: float = 1e-5) -> None:
        super().__init__()
        self.gamma = nn.Parameter(torch.ones([1, channels, 1], dtype=torch.float32))
        self.beta = nn.Parameter(torch.zeros([1, channels, 1], dtype=torch.float32))
        self.epsilon = epsilon

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        var, mean = torch.var_mean(x, dim=1, keepdim=True, unbiased=False)
        x = (x - mean) / torch.sqrt(var + self.epsilon)
        return x * self.gamma + self.beta


class MaskedConv1d(nn.Module):
    """nn.Conv1d behind (kernel_size - 1) * dilation zeros in front of its own input: output t reads inputs <= t"""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, dilation: int = 1) -> None:
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, dilation=dilation)
        self.padding = (kernel_size - 1) * dilation

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.conv(torch.nn.functional.pad(x, [self.padding, 0]))


class ResBlockOneMasked(nn.Module):
    one_masked = True

    def __init__(self, channels: int, kernel_size: int, dilation: int):
        super().__init__()
        mid_channels = channels // 2
        self.layer_norm1 = LayerNorm(channels)
        self.conv1 = nn.Conv1d(channels, mid_channels, kernel_size=1)
        self.layer_norm2 = LayerNorm(mid_channels)
        self.conv2 = MaskedConv1d(mid_channels, mid_channels, kernel_size=kernel_size, dilation=dilation)
        self.layer_norm3 = LayerNorm(mid_channels)
        self.conv3 = nn.Conv1d(mid_channels, channels, kernel_size=1)
        self.channels, self.kernel_size, self.dilation = channels, kernel_size, dilation

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.conv1(torch.relu(self.layer_norm1(x)))
        y = self.conv2(torch.relu(self.layer_norm2(y)))
        y = self.conv3(torch.relu(self.layer_norm3(y)))
        return y + x

    def stage_params(self):
        """the kernel's 12 slots: conv weight 0..2, conv bias 0..2, LayerNorm gamma 0..2, beta 0..2 in stage order"""
        convs = (self.conv1, self.conv2.conv, self.conv3)
        lns = (self.layer_norm1, self.layer_norm2, self.layer_norm3)
        return [c.weight for c in convs] + [c.bias for c in convs] + [n.gamma for n in lns] + [n.beta for n in lns]


class ResBlockTwoMasked(nn.Module):
    one_masked = False

    def __init__(self, channels: int, kernel_size: int, dilation: int):
        super().__init__()
        self.conv1 = MaskedConv1d(channels, channels, kernel_size, dilation)
        self.layer_norm1 = LayerNorm(channels)
        self.conv2 = MaskedConv1d(channels, channels, kernel_size, 2 * dilation)
        self.layer_norm2 = LayerNorm(channels)
        self.channels, self.kernel_size, self.dilation = channels, kernel_size, dilation

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.relu(self.layer_norm1(self.conv1(x)))
        y = torch.relu(self.layer_norm2(self.conv2(y)))
        return y + x

    def stage_params(self):
        convs, lns = (self.conv1.conv, self.conv2.conv), (self.layer_norm1, self.layer_norm2)
        return [c.weight for c in convs] + [None] + [c.bias for c in convs] + [None] + \
            [n.gamma for n in lns] + [None] + [n.beta for n in lns] + [None]


class NextItNetLayer(nn.Module):
    def __init__(self, channels: int, dilations: List[int], one_masked: bool, kernel_size: int, feat_drop: float = 0.0):
        super().__init__()
        if one_masked:
            ResBlock = ResBlockOneMasked
            if dilations is None:
                dilations = [1, 2, 4]
        else:
            ResBlock = ResBlockTwoMasked
            if dilations is None:
                dilations = [1, 4]
        self.feat_drop = nn.Dropout(feat_drop) if feat_drop > 0 else None
        self.res_blocks = nn.ModuleList([ResBlock(channels, kernel_size, dilation) for dilation in dilations])
        self.last_mode = True

    def forward(self, emb_seqs, lens):
        batch_size, max_len, _ = emb_seqs.size()
        if emb_seqs.is_cuda and len(self.res_blocks) > 0:
            return self._forward_hip(emb_seqs, lens)
        mask = torch.arange(max_len, device=lens.device).unsqueeze(0).expand(batch_size, max_len) >= lens.unsqueeze(-1)
        emb_seqs = torch.masked_fill(emb_seqs, mask.unsqueeze(-1), 0)
        if self.feat_drop is not None:
            emb_seqs = self.feat_drop(emb_seqs)
        x = torch.transpose(emb_seqs, 1, 2)  # (B, C, L)
        for res_block in self.res_blocks:
            x = res_block(x)
        return x[torch.arange(len(lens)), :, lens - 1]  # (lens = 0 reads position L - 1)

    def _forward_hip(self, x, lens):
        B, L, _ = x.shape
        lens = lens.to(torch.int64).clamp(0, L).contiguous()
        if self.feat_drop is not None and self.training:
            # (the reference zeroes the rows behind lens first; a dropped zero is a zero, and the first block reads those
            #  rows as zero whatever they hold)
            x = Fh.dropout(x, self.feat_drop.p)
        # A block reads rows at positions >= lens as zero.  That IS the masked_fill for the first block; the later blocks
        # never look behind lens - 1 from the read position, except in a row without history, whose read position is
        # L - 1 and whose later blocks must see the first block's output everywhere: their length is L.
        later = torch.where(lens > 0, lens, torch.full_like(lens, L))
        n = len(self.res_blocks)
        for i, block in enumerate(self.res_blocks):
            final = i == n - 1
            x = Fh.causal_conv_block(x, lens if i == 0 else later, block, last=final and self.last_mode)
            if final and not self.last_mode:
                x = Fh.seq_take(x, later - 1)
        return x
