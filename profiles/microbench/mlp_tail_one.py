"""The MLP tail's launches alone (HIP events over `reps` launches after warm-up): mlp_tail_one.py [M] [L] [reps]
   -> one JSON line: us per launch of the fused-BCE forward, the backward's first launch (parts = 1) and its second stage
   (parts = 2).  RP_LIB_PATH selects the library, so two builds are timed on one box in one session."""
import ctypes as C
import json
import os
import sys
import torch
sys.path.insert(0, '.')
from rec_pangu_amd import hip

M = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
L = int(sys.argv[2]) if len(sys.argv) > 2 else 2
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
lib = hip.lib()
torch.manual_seed(0)
dev = 'cuda'
hin = torch.relu(torch.randn(M, 64, device=dev))
Ws = [torch.randn(64, 64, device=dev) / 8 for _ in range(L)]
bs = [torch.randn(64, device=dev) / 8 for _ in range(L)]
w_out, b_out = torch.randn(1, 64, device=dev) / 8, torch.randn(1, device=dev)
fm = torch.randn(M, device=dev)
label = (torch.rand(M, device=dev) < 0.3).float()
pred, loss, hs = hip.mlp_tail_fwd_bce(hin, Ws, bs, w_out, b_out, [fm], label)
acts = [hin] + hs
dz = torch.randn(M, device=dev) / M
dhin = torch.empty(M, 64, device=dev)
grads = torch.empty(L * 4160 + 65, device=dev)
nbytes = C.c_size_t(0)
assert lib.rp_mlp_tail_bwd_workspace_bytes(M, L, C.byref(nbytes)) == 0
ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
stream = torch.cuda.current_stream().cuda_stream


def bwd(parts):
    rc = lib.rp_mlp_tail_bwd_parts(dz.data_ptr(), L, hip._ptr_array(Ws), hip._i64_array([64] * L), hip._ptr_array(acts), 64,
                                   w_out.data_ptr(), dhin.data_ptr(), 64, grads.data_ptr(), M, ws.data_ptr(), nbytes.value,
                                   parts, stream)
    assert rc == 0


partial = torch.empty(lib.rp_mlp_tail_loss_partials(M), device=dev)


def fwd():
    rc = lib.rp_mlp_tail_fwd_bce(hin.data_ptr(), 64, L, hip._ptr_array(Ws), hip._i64_array([64] * L), hip._opt_ptr_array(bs),
                                 hip._ptr_array(hs), w_out.data_ptr(), b_out.data_ptr(), hip._ptr_array([fm]), 1,
                                 label.data_ptr(), 0.0, pred.data_ptr(), partial.data_ptr(), M, stream)
    assert rc == 0


def timed(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):  # five windows: the spread of the figure itself
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1) * 1e3 / reps, 2))
    return out


res = {"lib": os.path.basename(os.path.dirname(hip.LIB_PATH)) + "/" + os.path.basename(hip.LIB_PATH), "M": M, "L": L, "reps": reps,
       "fwd_bce_us": timed(fwd),
       "bwd_part1_us": timed(lambda: bwd(1)),
       "bwd_part2_us": timed(lambda: bwd(2))}
print(json.dumps(res))
