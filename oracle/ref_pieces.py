"""Torch formulation of the operand format of the CIN pair kernels — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What rec_pangu_amd.hip.cin_pair_pieces (rp_cin_pair_pieces) is checked against, bit for bit: the same fp32 adds and
round-to-nearest-even conversions, as the product itself computed the pieces before that launch existed.
"""
import torch


def bf16_split3(full):
    """fp32 -> [3, ...] bf16 (hi, mid, lo) with full = hi + mid + lo (+ 2^-24 |full|)"""
    hi = full.to(torch.bfloat16)
    r1 = full - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack((hi, mid, lo)).contiguous()


def cin_pair_ws(W3):
    """W [O, H, H] -> Ws[o, (h <= m)] = W[o,h,m] + W[o,m,h] (W[o,h,h] on the diagonal), row-major upper triangle"""
    O, H, _ = W3.shape
    iu = torch.triu_indices(H, H, device=W3.device)
    return W3[:, iu[0], iu[1]] + W3[:, iu[1], iu[0]] * (iu[0] != iu[1]).to(W3.dtype)


def cin_pair_pieces(W3, transposed: bool = False):
    """[3, 128, pairs rounded up to 32] (rp_cin_pair_fwd's wsp) or, transposed, [3, pairs rounded up to 128, 128]
    (rp_cin_pair_bwd_x's wst), zero padded"""
    O = W3.shape[0]
    ws = cin_pair_ws(W3)
    npair = ws.shape[1]
    if transposed:
        full = torch.zeros(((npair + 127) // 128 * 128, 128), dtype=torch.float32, device=W3.device)
        full[:npair, :O] = ws.t()
    else:
        full = torch.zeros((128, (npair + 31) // 32 * 32), dtype=torch.float32, device=W3.device)
        full[:O, :npair] = ws
    return bf16_split3(full)
