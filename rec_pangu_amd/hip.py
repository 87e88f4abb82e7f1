"""ctypes binding of librecpangu_hip.so (C ABI: include/rec_pangu_hip.h).

This is the only place Python touches the kernels.  PyTorch is plumbing here: it owns device
memory (`tensor.data_ptr()`), and the current HIP stream (`torch.cuda.current_stream()`); no
torch type crosses the ABI.  There is NO fallback: if the shared object is missing or a call
fails, a RuntimeError is raised — a CUDA(HIP)-resident tensor never silently takes another path.
"""
import contextlib
import ctypes as C
import os
import re
from typing import List, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "rec_pangu_hip.h")  # (csrc/Makefile: ../../include from csrc)
LIB_PATH = os.environ.get("RP_LIB_PATH") or os.path.join(_HERE, "lib", "librecpangu_hip.so")  # (override: A/B builds)

_lib = None

_i64, _i32, _f32, _vp, _sz = C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_size_t
_f64 = C.c_double
_C_TYPES = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "rp_stream_t": C.c_void_p}
_PROTOTYPE = re.compile(r"([A-Za-z_][\w\s]*?[\s*]+)(rp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def parse_header(text: str):
    """-> ({entry point: (restype, [argtypes])} in header order, {RP_* constant: int}) from the text of the C header: every
    `ret rp_name(params);` outside comments and preprocessor lines, every `#define RP_NAME <integer>`.  A scalar maps to
    its ctypes type, rp_stream_t and every pointer (host out-parameters included: byref(...), ctypes arrays and string
    buffers all pass) to c_void_p, a `const char *` result to c_char_p.  Anything else raises, naming the prototype."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    consts = {m.group(1): int(m.group(2), 0) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(RP_\w+)[ \t]+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def ctype(decl: str, proto: str, result: bool = False):
        words = decl.replace("*", " * ").split()
        if "[" in decl:
            raise RuntimeError(f"C header: array parameter {decl.strip()!r} in `{proto}` has no ctypes mapping")
        if "*" in words:
            if result and words != ["const", "char", "*"]:
                raise RuntimeError(f"C header: result type {decl.strip()!r} of `{proto}` has no ctypes mapping")
            return C.c_char_p if result else C.c_void_p
        words = [w for w in words if w != "const"]
        if not result and len(words) == 2:  # `type name`
            words = words[:1]
        if len(words) != 1 or words[0] not in _C_TYPES:
            raise RuntimeError(f"C header: type {decl.strip()!r} in `{proto}` has no ctypes mapping")
        return _C_TYPES[words[0]]

    sigs = {}
    for m in _PROTOTYPE.finditer(text):
        ret, name, params = m.groups()
        proto = " ".join(m.group(0).split())
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (ctype(ret, proto, result=True), [ctype(p, proto) for p in params])
    calls = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", text))
    if calls != set(sigs):
        raise RuntimeError(f"C header: not parsed as prototypes: {sorted(calls - set(sigs))}")
    return sigs, consts


with open(HEADER_PATH) as _f:
    _SIGNATURES, _RP = parse_header(_f.read())
ABI_VERSION = _RP["RP_ABI_VERSION"]  # rp_version(): bumped with every change of the entry points' prototypes
MAX_FIELDS = _RP["RP_MAX_FIELDS"]
ACT_NONE, ACT_RELU, ACT_MASK, ACT_TANH, ACT_SIGMOID, ACT_LEAKY = (
    _RP["RP_ACT_" + n] for n in ("NONE", "RELU", "MASK", "TANH", "SIGMOID", "LEAKY"))
EXPORTED_SYMBOLS = tuple(_SIGNATURES.keys())


def lib():
    """Load the shared object once; raise loudly if it is not there (no CPU stand-in exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `make -C rec_pangu_amd/csrc` "
                "(or __graft_entry__.build()). The HIP path has no fallback.")
        handle = C.CDLL(LIB_PATH)
        handle.rp_version.restype = C.c_int
        if handle.rp_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} is version {handle.rp_version()} of the C ABI, these bindings are for {ABI_VERSION}: "
                               "rebuild it (`make -C rec_pangu_amd/csrc`, or __graft_entry__.build())")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
        mode = os.environ.get("RP_MATMUL_PRECISION")  # fp32 | bf16 | bf16x3 | bf16x6 | auto (library default)
        if mode:
            if handle.rp_set_matmul_precision(MATMUL_MODES[mode]) != 0:
                raise RuntimeError(f"RP_MATMUL_PRECISION={mode}: rejected by the library")
    return _lib


def available() -> bool:
    return os.path.exists(LIB_PATH)


def launch_count() -> int:
    return int(lib().rp_launch_count())


# ---- HIP-resident modules that take a torch (ATen) path: counted and warned about once, never silent ----------------
_torch_paths: dict = {}


def note_torch_path(what: str) -> None:
    """A module whose tensors live on the HIP device is about to compose its result from torch device ops instead of the
    library's kernels (a configuration no kernel covers: a masked / cross attention, a CIN over more than 32 fields, a
    non-ReLU activation module inside an MLP ...).  Results are the same; the launch is not ours.  Counted per reason
    (torch_path_count / torch_paths) and warned about once per reason; RP_STRICT_HIP=1 turns it into an error."""
    n = _torch_paths.get(what, 0)
    _torch_paths[what] = n + 1
    if os.environ.get("RP_STRICT_HIP", "0") == "1":
        raise RuntimeError(f"RP_STRICT_HIP=1: a HIP-resident module took a torch path: {what}")
    if n == 0:
        import warnings
        warnings.warn(f"rec_pangu_amd: HIP-resident module on a torch (ATen) path, not on the library's kernels: {what} "
                      "(reported once; hip.torch_paths() has the counts)", RuntimeWarning, stacklevel=3)


def torch_path_count() -> int:
    return sum(_torch_paths.values())


def torch_paths() -> dict:
    return dict(_torch_paths)


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().rp_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def _stream() -> int:
    # raw handle of torch's current stream: torch.cuda.current_stream() builds a Stream object (~10 us per call,
    # dozens of launches per step)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"expected a HIP-device tensor, got one on {t.device}")
    return t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a HIP-device tensor, got {t.device}")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")


def _rowmajor(t: torch.Tensor, name: str) -> int:
    """2-D tensor with unit inner stride -> leading dimension."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"{name}: need a 2-D tensor with unit inner stride, got {tuple(t.shape)}/{t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _rows(t: torch.Tensor, name: str, cols: int, B: Optional[int] = None) -> int:
    """The contract of a row buffer a kernel reads or writes in place — float32 [B, >= cols], unit inner stride, rows that
    do not overlap — checked in that order -> leading dimension.  Host-side only: a validator runs every such check first
    and the device checks (_req) last, so a refusal never depends on where the tensor lives."""
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected torch.float32, got {t.dtype}")
    if t.dim() != 2:
        raise RuntimeError(f"{name}: need a 2-D tensor, got {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise RuntimeError(f"{name}: need unit inner stride, got {tuple(t.shape)}/{t.stride()}")
    if t.shape[1] < cols:
        raise RuntimeError(f"{name} {tuple(t.shape)}: rows narrower than {cols}")
    if t.shape[0] > 1 and t.stride(0) < cols:
        raise RuntimeError(f"{name} {tuple(t.shape)} / strides {t.stride()}: rows overlap, row stride narrower than {cols}")
    if B is not None and t.shape[0] != B:
        raise RuntimeError(f"{name} {tuple(t.shape)}: expected {B} rows")
    return _rowmajor(t, name)


def _params(named) -> None:
    """(name, tensor) pairs of a parameter list: float32 and contiguous (host-side, like _rows)"""
    for name, t in named:
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: expected torch.float32, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")


# ---- device memory: ONE allocator, and one rule for recorded steps ----------------------------------------------------
# Every device tensor this module allocates — outputs, workspaces, internal scratch — comes from `_new`; while a
# `holding()` block is open, `_new` keeps it referenced by the block's list.  Why: inside a stream capture the allocator
# hands a freed block to the NEXT allocation of the same capture — fine for launches that replay in recorded order on one
# stream, wrong for launches the replay runs BESIDE others (a plan's inline section between its fork and its join, the
# row-sharded step's look-ahead segments): a temporary one of them dropped would be overwritten by its neighbour on
# every replay.  Whoever records such launches opens the block around them and everything they run beside.
_HOLDING = None


class holding:
    """with holding() as items: ...  (nestable: an inner block collects its own tensors; closed behind an exception too)"""

    def __enter__(self):
        global _HOLDING
        self.prev, self.items = _HOLDING, []
        _HOLDING = self.items
        return self.items

    def __exit__(self, *exc):
        global _HOLDING
        _HOLDING = self.prev
        return False

    @staticmethod
    def active() -> bool:
        return _HOLDING is not None


def _new(shape, dtype, device):
    t = torch.empty(shape, dtype=dtype, device=device)
    if _HOLDING is not None:
        _HOLDING.append(t)
    return t


def _new_like(t):
    return _new(t.shape, t.dtype, t.device)


def _workspace(query: str, *dims, device, given=None):
    """-> (uint8 workspace, bytes) of the size rp_<query>_workspace_bytes(*dims) asks for; given: a caller's persistent
    workspace, taken instead of a fresh one when it is on the device and large enough"""
    name, nbytes = f"rp_{query}_workspace_bytes", _sz(0)
    _check(getattr(lib(), name)(*dims, C.byref(nbytes)), name)
    if given is not None and given.numel() >= nbytes.value and given.device == device:
        return given, nbytes.value
    return _new((nbytes.value,), torch.uint8, device), nbytes.value


# ---- optional per-entry-point timing with HIP events on the launch stream (bench.py's roofline) ----
_timing = None


def enable_timing(on: bool = True, only=None):
    """Record a HIP-event pair around every C-ABI call (`only`: just the named entry points).  An event record is
    a barrier packet in the queue: timing every launch of a step serialises kernels that would otherwise overlap
    and costs host time, so a throughput measurement should restrict it to the few launches it reports."""
    global _timing, _timing_only
    _timing = {} if on else None
    _timing_only = None if only is None else frozenset(only)


_timing_only = None
_timing_paused = False


def pause_timing(paused: bool):
    """Keep the recorded events but stop/resume recording new ones (lets a benchmark sample every n-th step)."""
    global _timing_paused
    _timing_paused = bool(paused)


class _Timed:
    """`tag`: a launch-shape suffix (bench.py then reports one row per kernel shape instead of one per entry point);
    `nbytes` / `flops`: algorithmic bytes moved / flops of this launch where the entry point knows them itself."""
    __slots__ = ("name", "key", "ev", "meta")

    def __init__(self, name, tag=None, nbytes=0, flops=0):
        self.name = name
        self.key = name if tag is None else f"{name}[{tag}]"
        self.meta = (nbytes, flops)

    def __enter__(self):
        self.ev = None
        if _timing is not None and not _timing_paused and (_timing_only is None or self.name in _timing_only):
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
            _timing.setdefault(self.key, []).append(self.ev)
            if self.meta != (0, 0):
                _timing_meta[self.key] = self.meta
        return False


_timing_meta = {}


def timing_summary():
    """{entry point[shape tag]: (calls, mean milliseconds)} for the calls recorded since enable_timing(True)."""
    out = {}
    for name, evs in (_timing or {}).items():
        ms = [a.elapsed_time(b) for a, b in evs]
        out[name] = (len(ms), sum(ms) / max(len(ms), 1))
    return out


def timing_meta():
    """{entry point[shape tag]: (algorithmic bytes, flops) per launch} for the rows that carry them (the GEMMs)."""
    return dict(_timing_meta)


_PTR_ARRAYS: dict = {}  # tuple of device addresses -> the ctypes array holding them (the same lists recur every step)


def _ptr_array(tensors: Sequence[torch.Tensor]):
    """HOST array of the tensors' device addresses for a `*_ptrs` argument (copied into the launch packet by the
    library).  Built once per distinct address tuple: the element-wise fill of a ctypes array was the largest single item
    of the host's time per step (10 calls x up to 39 tensors: ~0.25 ms of a ~1.0 ms enqueue, host_profile.py)."""
    ptrs = tuple([t.data_ptr() for t in tensors])
    arr = _PTR_ARRAYS.get(ptrs)
    if arr is None:
        for i, t in enumerate(tensors):
            if not t.is_cuda:  # a host pointer inside a launch packet is a GPU memory fault, not an exception
                raise RuntimeError(f"Expected all tensors to be on the same device: input {i} is on {t.device} but the "
                                   "model is on the HIP device (move the batch with .to(device))")
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        if len(_PTR_ARRAYS) >= 512:
            _PTR_ARRAYS.clear()
        _PTR_ARRAYS[ptrs] = arr
    return arr


# ----------------------------------------------------------------------------------------------
def embed_gather_fwd(arena, row_base, row_count, idx: List[torch.Tensor], dense: List[torch.Tensor], ldx: int,
                     want_fm: bool, want_sum: bool, want_keys: bool, err_flag: torch.Tensor):
    _req(arena, torch.float32, "arena")
    F, ND = len(idx), len(dense)
    B, D = idx[0].shape[0], arena.shape[1]
    for t in idx:
        _req(t, torch.int64, "index")
        if t.dim() != 1 or t.shape[0] != B or not t.is_contiguous():
            raise RuntimeError("index tensors must be contiguous int64 [B]")
    for t in dense:
        _req(t, torch.float32, "dense")
        if t.dim() != 1 or t.shape[0] != B or not t.is_contiguous():
            raise RuntimeError("dense tensors must be contiguous float32 [B]")
    dev = arena.device
    x = _new((B, ldx), torch.float32, dev)
    fm = _new((B, 1), torch.float32, dev) if want_fm else None
    ssum = _new((B, D), torch.float32, dev) if want_sum else None
    keys = _new((F * B,), torch.int32, dev) if want_keys else None
    with _Timed("embed_gather_fwd", f"D={D}"):
        _check(lib().rp_embed_gather_fwd(arena.data_ptr(), row_base.data_ptr(), row_count.data_ptr(), _ptr_array(idx), F,
                                     _ptr_array(dense), ND, B, D, x.data_ptr(), ldx, _ptr(fm), _ptr(ssum), _ptr(keys),
                                     err_flag.data_ptr(), _stream()), "rp_embed_gather_fwd")
    return x, fm, ssum, keys


def embed_gather_linear_fits(D: int, F: int, ND: int, hidden: int, ldx: int, W) -> bool:
    return F <= 32 and bool(lib().rp_embed_gather_linear_fits(D, ND, hidden, ldx, _rowmajor(W, "W"))) and W.data_ptr() % 16 == 0


def embed_gather_linear_fwd(arena, row_base, row_count, idx: List[torch.Tensor], dense: List[torch.Tensor], ldx: int, W, bias,
                            want_fm: bool, want_sum: bool, want_keys: bool, err_flag: torch.Tensor, x_mode: str = "full"):
    """the gather fused with the 64-wide Linear + ReLU that consumes it -> (x, h1 [B, 64], fm, ssum, keys).
    x_mode: "full" = x [B, ldx] is stored; "dense" = only the dense columns, as xd [B, 64] (the embedding columns of the
    weight gradient come from the gather backward: rp_embed_grad_seg); "none" = nothing is stored (inference)."""
    _req(arena, torch.float32, "arena")
    _req(W, torch.float32, "W")
    F, ND = len(idx), len(dense)
    B, D = idx[0].shape[0], arena.shape[1]
    for t in idx:
        _req(t, torch.int64, "index")
        if t.dim() != 1 or t.shape[0] != B or not t.is_contiguous():
            raise RuntimeError("index tensors must be contiguous int64 [B]")
    for t in dense:
        _req(t, torch.float32, "dense")
        if t.dim() != 1 or t.shape[0] != B or not t.is_contiguous():
            raise RuntimeError("dense tensors must be contiguous float32 [B]")
    dev = arena.device
    assert x_mode in ("full", "dense", "none")
    x = _new((B, ldx), torch.float32, dev) if x_mode == "full" else None
    xd = _new((B, 64), torch.float32, dev) if x_mode == "dense" else None
    h1 = _new((B, 64), torch.float32, dev)
    fm = _new((B, 1), torch.float32, dev) if want_fm else None
    ssum = _new((B, D), torch.float32, dev) if want_sum else None
    keys = _new((F * B,), torch.int32, dev) if want_keys else None
    K = F * D + ND
    # algorithmic bytes (rows + ids read, the [B, F*D+ND] output written — counted whether or not the launch
    # stores it, the figure the gather is priced on) + h1
    with _Timed("embed_gather_linear_fwd", f"D={D}", B * (F * (D * 4 + 8) + (F * D + ND) * 4 + 64 * 4), 2 * B * K * 64):
        _check(lib().rp_embed_gather_linear_fwd(arena.data_ptr(), row_base.data_ptr(), row_count.data_ptr(), _ptr_array(idx), F,
                                                _ptr_array(dense), ND, B, D, _ptr(x), ldx, W.data_ptr(), _rowmajor(W, "W"),
                                                _ptr(bias), h1.data_ptr(), _ptr(fm), _ptr(ssum), _ptr(keys),
                                                err_flag.data_ptr(), _ptr(xd), _stream()), "rp_embed_gather_linear_fwd")
    return (x if x_mode == "full" else xd), h1, fm, ssum, keys


def embed_gather_linear_fwd_bf16(arena_bf16, row_base, row_count, idx: List[torch.Tensor], dense: List[torch.Tensor], W, bias,
                                 err_flag: torch.Tensor, train_ldx: int = 0, want_keys: bool = False, dense_only: bool = False):
    """bf16-storage: the fused lookup + FM + first Linear over a bf16 copy of the arena -> (h1 [B, 64], fm [B, 1]);
    train_ldx > 0 (the bf16-storage TRAINING mode): -> (x_bf16 [B, train_ldx] bfloat16, h1, fm, ssum [B, 64], keys or None);
    dense_only (round 5, with train_ldx > 0): no activation is stored — x is xd [B, 64] fp32, the dense columns"""
    _req(arena_bf16, torch.bfloat16, "arena_bf16")
    _req(W, torch.float32, "W")
    F, ND = len(idx), len(dense)
    B, D = idx[0].shape[0], arena_bf16.shape[1]
    dev = arena_bf16.device
    h1 = _new((B, 64), torch.float32, dev)
    fm = _new((B, 1), torch.float32, dev)
    K = F * D + ND
    if train_ldx:
        x16 = None if dense_only else _new((B, train_ldx), torch.bfloat16, dev)
        xd = _new((B, 64), torch.float32, dev) if dense_only else None
        ssum = _new((B, D), torch.float32, dev)
        keys = _new((F * B,), torch.int32, dev) if want_keys else None
        # algorithmic bytes: bf16 rows + ids read, the bf16 activation "written" (SURVEY 8d's figure, whether or not the launch
        # stores it), h1 + the field sums
        with _Timed("embed_gather_linear_fwd_bf16", f"D={D}", B * (F * (D * 2 + 8) + (F * D + ND) * 2 + 64 * 4 + D * 4), 2 * B * K * 64):
            _check(lib().rp_embed_gather_linear_fwd_bf16(arena_bf16.data_ptr(), row_base.data_ptr(), row_count.data_ptr(),
                                                         _ptr_array(idx), F, _ptr_array(dense), ND, B, D, W.data_ptr(),
                                                         _rowmajor(W, "W"), _ptr(bias), h1.data_ptr(), fm.data_ptr(),
                                                         _ptr(x16), train_ldx, ssum.data_ptr(), _ptr(keys),
                                                         err_flag.data_ptr(), _ptr(xd), _stream()), "rp_embed_gather_linear_fwd_bf16")
        return (xd if dense_only else x16), h1, fm, ssum, keys
    # algorithmic bytes: SURVEY 8d's bf16 figure — bf16 rows + int64 ids read, the [B, F*D] bf16 output "written" (it is
    # consumed in registers here) = F * (2 D + 8) + 2 F D per sample (6 864 B at Criteo shape) — plus h1
    with _Timed("embed_gather_linear_fwd_bf16", f"D={D}", B * (F * (D * 2 + 8) + F * D * 2 + 64 * 4), 2 * B * K * 64):
        _check(lib().rp_embed_gather_linear_fwd_bf16(arena_bf16.data_ptr(), row_base.data_ptr(), row_count.data_ptr(),
                                                     _ptr_array(idx), F, _ptr_array(dense), ND, B, D, W.data_ptr(),
                                                     _rowmajor(W, "W"), _ptr(bias), h1.data_ptr(), fm.data_ptr(),
                                                     None, 0, None, None, err_flag.data_ptr(), None, _stream()),
               "rp_embed_gather_linear_fwd_bf16")
    return h1, fm


def sort_workspace(n: int, device) -> torch.Tensor:
    """a workspace rp_sort_pairs_i32 accepts for n pairs (callers that must not allocate per call keep one)"""
    return _workspace("sort", n, device=device)[0]


def sort_pairs(keys: torch.Tensor, end_bit: int = 32, out=None, workspace=None):
    """out = (sorted keys, positions) to write into (persistent buffers of the captured-step path; either may be None), else
    fresh tensors; workspace: a persistent sort_workspace(n) (else one is allocated per call)"""
    _req(keys, torch.int32, "keys")
    n = keys.numel()
    ws, nbytes = _workspace("sort", n, device=keys.device, given=workspace)
    assert workspace is None or ws is workspace
    ko, po = (_new_like(keys) if t is None else t for t in (out or (None, None)))
    assert ko.shape == keys.shape and po.shape == keys.shape and ko.dtype == po.dtype == torch.int32
    with _Timed("sort_pairs_i32"):
        _check(lib().rp_sort_pairs_i32(ws.data_ptr(), nbytes, keys.data_ptr(), ko.data_ptr(), po.data_ptr(), n,
                                   end_bit, _stream()), "rp_sort_pairs_i32")
    return ko, po


METRIC_AUC, METRIC_LOGLOSS = _RP["RP_METRIC_AUC"], _RP["RP_METRIC_LOGLOSS"]
# the launches of rp_binary_metrics in issue order: name -> RP_METRICS_STAGE_* bit (a measurement issues them one by one)
METRICS_STAGES = {s: _RP["RP_METRICS_STAGE_" + s.upper()]
                  for s in ("key", "sort", "tile_sums", "tile_scan", "group_neg", "rank", "finish")}


def metrics_workspace(n: int, device) -> torch.Tensor:
    return _workspace("metrics", n, device=device)[0]


def metrics_stage_bytes(n: int, flags: int = METRIC_AUC | METRIC_LOGLOSS) -> dict:
    """algorithmic bytes of each launch group of rp_binary_metrics over n elements (csrc/metrics.hip; T = tiles of 4096)"""
    T = -(-n // 4096)
    auc = bool(flags & METRIC_AUC)
    out = {"key": n * (8 + (4 if auc else 0)) + 20 * T, "finish": (20 + (8 if auc else 0)) * T + 40}
    if auc:
        # the sort: 4 digit passes, each reads the keys twice (histogram, scatter) and the values once (implicit in the
        # first pass) and writes both columns
        out.update({"sort": n * 4 * (4 * 2 + 3 + 4 * 2), "tile_sums": n * (4 + 4 + 4 + 1) + 8 * T, "tile_scan": 16 * T,
                    "group_neg": n * (4 + 1 + 4) + 8 * T, "rank": n * (4 + 1 + 4) + 12 * T})
    return out


def binary_metrics(pred: torch.Tensor, label: torch.Tensor, flags: int = METRIC_AUC | METRIC_LOGLOSS, eps: float = 1e-7,
                   workspace=None, result=None, stages=None) -> torch.Tensor:
    """rp_binary_metrics over float32 [n] device tensors -> the DEVICE result, int64 [5] = (two_u, P, N, unsupported, the
    bits of the float64 log-loss sum); nothing here waits for the device — the caller's one copy of the 40 bytes does.
    stages: names from METRICS_STAGES, issued as one call each under their own timing rows (measurements; needs the same
    workspace and result across the calls)."""
    _req(pred, torch.float32, "pred")
    _req(label, torch.float32, "label")
    n = pred.numel()
    if label.numel() != n or not pred.is_contiguous() or not label.is_contiguous():
        raise RuntimeError("binary_metrics: pred and label must be contiguous and of one length")
    ws, _ = _workspace("metrics", n, device=pred.device, given=workspace)
    res = _new((5,), torch.int64, pred.device) if result is None else result
    sizes = metrics_stage_bytes(n, flags)
    for tag, bits in ([(None, 0)] if stages is None else [(s, METRICS_STAGES[s]) for s in stages]):
        with _Timed("binary_metrics", tag, sizes.get(tag, 0) if tag else sum(sizes.values())):
            _check(lib().rp_binary_metrics(ws.data_ptr(), ws.numel(), pred.data_ptr(), label.data_ptr(), n, eps, flags | bits,
                                           res.data_ptr(), _stream()), "rp_binary_metrics")
    return res


_SORT_FIELDS: dict = {}


def sort_fields_workspace(B: int, F: int, device) -> torch.Tensor:
    return _workspace("sort_pairs_fields", B, F, device=device)[0]


def sort_pairs_fields(keys: torch.Tensor, B: int, field_rows, out=None, workspace=None):
    """rp_sort_pairs_fields_i32: the pair list of one lookup (keys[f * B + b] = arena row, the tables back to back in field
    order with `field_rows` rows each) sorted field segment by field segment — the result of sort_pairs(keys, bits of the arena),
    bit for bit, in 49 instead of 78 field-passes at Criteo shape.  out / workspace as sort_pairs."""
    _req(keys, torch.int32, "keys")
    F = len(field_rows)
    assert keys.numel() == F * B
    ck = tuple(int(r) for r in field_rows)
    arrs = _SORT_FIELDS.get(ck)
    if arrs is None:
        if len(_SORT_FIELDS) > 64:
            _SORT_FIELDS.clear()
        base, acc = [], 0
        for r in ck:
            base.append(acc)
            acc += r
        arrs = _SORT_FIELDS[ck] = ((C.c_int64 * F)(*base), (C.c_int64 * F)(*ck))
    ws, _ = _workspace("sort_pairs_fields", B, F, device=keys.device, given=workspace)
    ko, po = (_new_like(keys) if t is None else t for t in (out or (None, None)))
    assert ko.shape == keys.shape and po.shape == keys.shape and ko.dtype == po.dtype == torch.int32
    with _Timed("sort_pairs_i32"):  # (the same row of the per-kernel table as the plain sort: it is that sort)
        _check(lib().rp_sort_pairs_fields_i32(ws.data_ptr(), ws.numel(), keys.data_ptr(), ko.data_ptr(), po.data_ptr(), B, F,
                                              arrs[0], arrs[1], _stream()), "rp_sort_pairs_fields_i32")
    return ko, po


def embed_grad_reduce(sorted_keys, sorted_pos, B: int, D: int, dx, gfm, sum_in, arena, grad_arena, accumulate: bool):
    _req(grad_arena, torch.float32, "grad_arena")
    ldx = 0
    if dx is not None:
        _req(dx, torch.float32, "dx")
        ldx = _rowmajor(dx, "dx")
    ws, nbytes = _workspace("embed_grad_reduce", sorted_keys.numel(), D, device=grad_arena.device)
    with _Timed("embed_grad_reduce", f"D={D}"):
        _check(lib().rp_embed_grad_reduce(sorted_keys.data_ptr(), sorted_pos.data_ptr(), sorted_keys.numel(), B, D,
                                      _ptr(dx), ldx, _ptr(gfm), _ptr(sum_in), _ptr(arena), grad_arena.data_ptr(),
                                      int(accumulate), ws.data_ptr(), nbytes, _stream()), "rp_embed_grad_reduce")


def embed_grad_gemm_fits(D: int, hidden: int, dh, wt) -> bool:
    return bool(lib().rp_embed_grad_gemm_fits(D, hidden, _rowmajor(dh, "dh"), _rowmajor(wt, "wt"))) \
        and dh.data_ptr() % 16 == 0 and wt.data_ptr() % 16 == 0


def embed_grad_tiny(keys, B: int, tiny, dh, wt, gfm, sum_in, arena, grad_arena, accumulate: bool, dw=None):
    """rp_embed_grad_tiny: the gradient rows of the tiny tables `tiny` = [(field, first arena row, rows), ...] from the
    unsorted pair keys [F * B] (sample-major one-hot GEMMs).  dw [64, K]: the tiny tables' columns of the first layer's
    weight gradient are written into it as well (the companion of embed_grad_seg)."""
    _req(keys, torch.int32, "keys")
    _req(dh, torch.float32, "dh")
    n = len(tiny)
    ckey = tuple(tiny)
    arrs = _TINY_ARRAYS.get(ckey)
    if arrs is None:
        arrs = _TINY_ARRAYS[ckey] = ((C.c_int32 * n)(*[t[0] for t in tiny]), (C.c_int64 * n)(*[t[1] for t in tiny]),
                                     (C.c_int32 * n)(*[t[2] for t in tiny]))
    ws, nbytes = _workspace("embed_grad_tiny", B, device=grad_arena.device)
    with _Timed("embed_grad_tiny", f"{n} tables", B * (64 * 8 + 4 + 4 * n)):
        _check(lib().rp_embed_grad_tiny(keys.data_ptr(), B, arrs[0], arrs[1], arrs[2], n, dh.data_ptr(), _rowmajor(dh, "dh"),
                                        wt.data_ptr(), _rowmajor(wt, "wt"), _ptr(gfm), _ptr(sum_in), _ptr(arena),
                                        grad_arena.data_ptr(), int(accumulate), _ptr(dw),
                                        _rowmajor(dw, "dw") if dw is not None else 0, ws.data_ptr(), nbytes, _stream()),
               "rp_embed_grad_tiny")


_TINY_ARRAYS: dict = {}


def embed_grad_gemm(sorted_keys, sorted_pos, B: int, D: int, dh, wt, dx, gfm, sum_in, arena, grad_arena, accumulate: bool,
                    skip_fields: int = 0):
    """rp_embed_grad_gemm: the segmented reduce with the consuming Linear's dgrad formed inside (dh [B,64], wt = W1^T).
    skip_fields: bit f set = the pairs of field f are left out (field-major positions only; embed_grad_tiny's tables)."""
    _req(grad_arena, torch.float32, "grad_arena")
    _req(dh, torch.float32, "dh")
    _req(wt, torch.float32, "wt")
    ldx = _rowmajor(dx, "dx") if dx is not None else 0
    ws, nbytes = _workspace("embed_grad_reduce", sorted_keys.numel(), D, device=grad_arena.device)
    with _Timed("embed_grad_gemm", f"D={D}"):
        _check(lib().rp_embed_grad_gemm(sorted_keys.data_ptr(), sorted_pos.data_ptr(), sorted_keys.numel(), B, D,
                                        dh.data_ptr(), _rowmajor(dh, "dh"), wt.data_ptr(), _rowmajor(wt, "wt"), _ptr(dx), ldx,
                                        _ptr(gfm), _ptr(sum_in), _ptr(arena), grad_arena.data_ptr(), int(accumulate),
                                        skip_fields, ws.data_ptr(), nbytes, _stream()), "rp_embed_grad_gemm")


def embed_grad_seg_fits(D: int, hidden: int, dh) -> bool:
    return bool(lib().rp_embed_grad_seg_fits(D, hidden, _rowmajor(dh, "dh"))) and dh.data_ptr() % 16 == 0


_SEG_ROWS: dict = {}


def _seg_rows(field_rows):
    """the table sizes per field as a ctypes array (None stays None), built once per distinct tuple"""
    if field_rows is None:
        return None
    ck = tuple(field_rows)
    fr = _SEG_ROWS.get(ck)
    if fr is None:
        fr = _SEG_ROWS[ck] = (C.c_int64 * len(ck))(*ck)
    return fr


def embed_grad_seg(sorted_keys, sorted_pos, B: int, D: int, dh, w, gfm, sum_in, arena, grad_arena, accumulate: bool,
                   skip_fields: int = 0, field_rows=None, dw=None):
    """rp_embed_grad_seg: the first layer's whole backward on the embedding columns, segment-sum first — the table
    gradient rows (dgrad of `w` [64, K] formed per run of equal keys + the FM term) AND, with dw [64, K], the embedding
    columns of the layer's weight gradient from the table rows the launch reads anyway (no stored activation).
    field_rows: table sizes per field (scheduling only).  Field-major positions (the single-device path)."""
    _req(grad_arena, torch.float32, "grad_arena")
    _req(dh, torch.float32, "dh")
    _req(w, torch.float32, "w")
    n = sorted_keys.numel()
    fr = _seg_rows(field_rows)
    ws, nbytes = _workspace("embed_grad_seg", n, B, D, device=grad_arena.device)
    with _Timed("embed_grad_seg", f"D={D}"):  # (algorithmic bytes / flops: bench.py knows the unique-row count)
        _check(lib().rp_embed_grad_seg(sorted_keys.data_ptr(), sorted_pos.data_ptr(), n, B, D, dh.data_ptr(), _rowmajor(dh, "dh"),
                                       w.data_ptr(), _rowmajor(w, "w"), _ptr(gfm), _ptr(sum_in), arena.data_ptr(),
                                       grad_arena.data_ptr(), int(accumulate), skip_fields, fr, _ptr(dw),
                                       _rowmajor(dw, "dw") if dw is not None else 0, ws.data_ptr(), nbytes, _stream()),
               "rp_embed_grad_seg")


_SMP_FIELDS: dict = {}


def embed_grad_smp_fits(D: int, hidden: int, dh) -> bool:
    return bool(lib().rp_embed_grad_smp_fits(D, hidden, _rowmajor(dh, "dh"))) and dh.data_ptr() % 16 == 0


def _smp_fields(fields):
    """`fields` = [(field, first arena row, rows), ...] (or plain field indices for the mark launch) -> ctypes arrays"""
    ck = tuple((int(f[0]), int(f[1]), int(f[2])) if isinstance(f, (tuple, list)) else (int(f), 0, 0) for f in fields)
    arr = _SMP_FIELDS.get(ck)
    if arr is None:
        n = len(ck)
        arr = _SMP_FIELDS[ck] = ((C.c_int32 * n)(*[t[0] for t in ck]), (C.c_int64 * n)(*[t[1] for t in ck]),
                                 (C.c_int64 * n)(*[t[2] for t in ck]))
    return arr


def embed_grad_smp_mark(sorted_keys, sorted_pos, B: int, fields, out=None):
    """rp_embed_grad_smp_mark: (dupq, dupkeys, scratch) — which pairs of the big tables `fields` share their table row with
    another pair of the batch, numbered compactly in sorted order, from the sorted pair list (depends on the batch's ids only)."""
    _req(sorted_keys, torch.int32, "sorted_keys")
    _req(sorted_pos, torch.int32, "sorted_pos")
    nf = len(fields)
    if out is None:
        nsc = _sz(0)
        _check(lib().rp_embed_grad_smp_mark_scratch(B, nf, C.byref(nsc)), "rp_embed_grad_smp_mark_scratch")
        out = (_new((nf * B,), torch.int32, sorted_keys.device),
               _new((nf * B,), torch.int32, sorted_keys.device),
               _new((nsc.value,), torch.int32, sorted_keys.device))
    with _Timed("embed_grad_smp_mark", f"{nf} fields", 16 * nf * B):
        _check(lib().rp_embed_grad_smp_mark(sorted_keys.data_ptr(), sorted_pos.data_ptr(), sorted_keys.numel(), B,
                                            _smp_fields(fields)[0], nf, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                            _stream()), "rp_embed_grad_smp_mark")
    return out


def embed_grad_smp(keys, marks, B: int, F: int, fields, dh, w, gfm, sum_in, arena, grad_arena, accumulate: bool, dw=None,
                   phases: int = 3, ws=None):
    """rp_embed_grad_smp: the first layer's backward on the embedding columns of the big tables `fields`, sample-major (the
    table rows' gradient incl. the FM term + those fields' columns of dw [64, K]); `fields` = [(field, first arena row,
    rows), ...] ascending; `marks` = embed_grad_smp_mark's pair.  phases = 1: the main launch only, 2: the launches behind
    it (same `ws`, returned by the phase-1 call), 3: both.  -> the workspace."""
    _req(keys, torch.int32, "keys")
    _req(dh, torch.float32, "dh")
    _req(w, torch.float32, "w")
    _req(grad_arena, torch.float32, "grad_arena")
    nf = len(fields)
    ws, nbytes = _workspace("embed_grad_smp", B, nf, device=grad_arena.device, given=ws)
    fa = _smp_fields(fields)
    with _Timed("embed_grad_smp" if phases & 1 else "embed_grad_smp_behind", f"{nf} fields"):
        _check(lib().rp_embed_grad_smp(keys.data_ptr(), marks[0].data_ptr(), marks[1].data_ptr(), B, F, fa[0], fa[1], fa[2], nf,
                                       dh.data_ptr(), _rowmajor(dh, "dh"), w.data_ptr(), _rowmajor(w, "w"), _ptr(gfm),
                                       _ptr(sum_in), arena.data_ptr(), grad_arena.data_ptr(), int(accumulate), _ptr(dw),
                                       _rowmajor(dw, "dw") if dw is not None else 0, phases, ws.data_ptr(), nbytes, _stream()),
               "rp_embed_grad_smp")
    return ws


def embed_grad_reduce_rows(keys, rows, grad_arena, accumulate: bool):
    """rp_embed_grad_reduce_rows: grad_arena[key] (+)= the sum of rows[i] over a key-sorted list (key -1: no entry)"""
    _req(keys, torch.int32, "keys")
    _req(rows, torch.float32, "rows")
    n, D = keys.numel(), rows.shape[1]
    ws, nbytes = _workspace("embed_grad_reduce", n, D, device=grad_arena.device)
    _check(lib().rp_embed_grad_reduce_rows(keys.data_ptr(), rows.data_ptr(), n, D, grad_arena.data_ptr(), int(accumulate),
                                           ws.data_ptr(), nbytes, _stream()), "rp_embed_grad_reduce_rows")


def embed_grad_ss_mark(sorted_keys, B: int, skip_fields: int, out=None):
    """rp_embed_grad_ss_mark: (ustart, ukey, offs) — the unique-row lists of the fields rp_embed_grad_ss keeps (every field
    whose bit in skip_fields is clear), from the sorted keys alone"""
    _req(sorted_keys, torch.int32, "sorted_keys")
    n = sorted_keys.numel()
    F = n // B
    kept = sum(1 for f in range(F) if not (skip_fields >> f) & 1)
    if out is None:
        nr, no = _sz(0), _sz(0)
        _check(lib().rp_embed_grad_ss_mark_sizes(B, kept, C.byref(nr), C.byref(no)), "rp_embed_grad_ss_mark_sizes")
        out = (_new((nr.value,), torch.int32, sorted_keys.device),
               _new((nr.value,), torch.int32, sorted_keys.device),
               _new((no.value,), torch.int32, sorted_keys.device))
    with _Timed("embed_grad_ss_mark", f"{kept} fields", 12 * kept * B):
        _check(lib().rp_embed_grad_ss_mark(sorted_keys.data_ptr(), n, B, skip_fields, out[0].data_ptr(), out[1].data_ptr(),
                                           out[2].data_ptr(), _stream()), "rp_embed_grad_ss_mark")
    return out


def embed_grad_ss(sorted_keys, sorted_pos, B: int, D: int, dh, w, gfm, sum_in, arena, grad_arena, accumulate: bool,
                  skip_fields: int = 0, field_rows=None, dw=None, phases: int = 3, ws=None, marks=None):
    """rp_embed_grad_ss: embed_grad_seg's work as a streaming segment-sum launch + a matrix launch over the unique rows (the
    mid-size tables' share of the first layer's backward); same arguments and results up to fp32 summation order.
    marks: embed_grad_ss_mark's triple for this sort and skip_fields (None: made inside the call).
    phases = 1: the segment-sum launch only, 2: the launches behind it (same `ws`), 3: both.  -> the workspace."""
    _req(grad_arena, torch.float32, "grad_arena")
    _req(dh, torch.float32, "dh")
    _req(w, torch.float32, "w")
    n = sorted_keys.numel()
    fr = _seg_rows(field_rows)
    ws, nbytes = _workspace("embed_grad_ss", n, B, D, skip_fields, device=grad_arena.device, given=ws)
    with _Timed("embed_grad_ss" if phases & 2 else "embed_grad_segsum", f"D={D}"):
        _check(lib().rp_embed_grad_ss(sorted_keys.data_ptr(), sorted_pos.data_ptr(), n, B, D, dh.data_ptr(), _rowmajor(dh, "dh"),
                                      w.data_ptr(), _rowmajor(w, "w"), _ptr(gfm), _ptr(sum_in), arena.data_ptr(),
                                      grad_arena.data_ptr(), int(accumulate), skip_fields, fr, _ptr(dw),
                                      _rowmajor(dw, "dw") if dw is not None else 0,
                                      None if marks is None else marks[0].data_ptr(), None if marks is None else marks[1].data_ptr(),
                                      None if marks is None else marks[2].data_ptr(), phases, ws.data_ptr(), nbytes, _stream()),
               "rp_embed_grad_ss")
    return ws


def zeros(shape, dtype, device):
    """torch.zeros through the library's own fill launch (rp_fill_words): inside a recorded step an ATen fill kernel would
    keep the step from replaying as a launch plan"""
    t = _new(shape, dtype, device)
    nb = t.numel() * t.element_size()
    if nb % 4 != 0 or t.data_ptr() % 16 != 0:
        return t.zero_()
    if nb:
        _check(lib().rp_fill_words(t.data_ptr(), nb // 4, 0, _stream()), "rp_fill_words")
    return t


def zero_rows(keys, D: int, grad_arena):
    with _Timed("zero_rows"):
        _check(lib().rp_zero_rows(keys.data_ptr(), keys.numel(), D, grad_arena.data_ptr(), _stream()), "rp_zero_rows")


def linear_fwd(a, w, bias, act: int = ACT_NONE, aux=None, K: Optional[int] = None, out=None):
    """out[M,N] = act(a[:, :K] @ w[N,K]^T + bias). `a` may be wider than K (padded rows)."""
    _req(a, torch.float32, "a")
    _req(w, torch.float32, "w")
    lda, ldw = _rowmajor(a, "a"), _rowmajor(w, "w")
    M, N = a.shape[0], w.shape[0]
    K = w.shape[1] if K is None else K
    if a.shape[1] < K:
        raise RuntimeError(f"linear_fwd: a has {a.shape[1]} columns, need {K}")
    if out is None:
        out = _new((M, N), torch.float32, a.device)
    ldo = _rowmajor(out, "out")
    ldaux = _rowmajor(aux, "aux") if aux is not None else 0
    with _Timed("linear_fwd", f"{M}x{N}x{K}", 4 * (M * K + N * K + M * N * (2 if aux is not None else 1)), 2 * M * N * K):
        _check(lib().rp_linear_fwd(a.data_ptr(), lda, w.data_ptr(), ldw, _ptr(bias), out.data_ptr(), ldo, M, N, K, act,
                               _ptr(aux), ldaux, _stream()), "rp_linear_fwd")
    return out


def linear_fwd_rowadd(a, w, row_scale, row_add, add_cols: int, out) -> bool:
    """out = a @ w^T + row_scale[:, None] * tile(row_add)[:, :add_cols]; False when the fused kernel does not cover
    the shape (nothing was launched)."""
    M, K = a.shape
    N = w.shape[0]
    if not (get_matmul_precision() != "fp32" and K <= 64 and K % 4 == 0 and M % 128 == 0 and M >= 128 and N % 64 == 0
            and add_cols % 64 == 0 and 0 < add_cols <= N and row_add.shape[1] == 64 and a.stride(0) % 4 == 0
            and w.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and out.shape[1] >= N):
        return False
    with _Timed("linear_fwd", f"{M}x{N}x{K}+rowadd", 4 * (M * K + N * K + M * N + M * 65), 2 * M * N * K):
        _check(lib().rp_linear_fwd_rowadd(a.data_ptr(), _rowmajor(a, "a"), w.data_ptr(), _rowmajor(w, "w"), out.data_ptr(),
                                          _rowmajor(out, "out"), M, N, K, row_scale.data_ptr(), row_add.data_ptr(),
                                          _rowmajor(row_add, "row_add"), add_cols, _stream()), "rp_linear_fwd_rowadd")
    return True


def linear_wgrad(dy, x, K: int, dw=None, db=None, accumulate: bool = False, want_bias: bool = True):
    """dw[N,K] = dy[M,N]^T @ x[:, :K]; db[N] = colsum(dy)."""
    _req(dy, torch.float32, "dy")
    _req(x, torch.float32, "x")
    M, N = dy.shape
    lddy, ldx = _rowmajor(dy, "dy"), _rowmajor(x, "x")
    if dw is None:
        dw = _new((N, K), torch.float32, dy.device)
    if db is None and want_bias:
        db = _new((N,), torch.float32, dy.device)
    ws, nbytes = _workspace("linear_wgrad", M, N, K, device=dy.device)
    with _Timed("linear_wgrad", f"{M}x{N}x{K}", 4 * (M * N + M * K + N * K), 2 * M * N * K):
        _check(lib().rp_linear_wgrad(dy.data_ptr(), lddy, x.data_ptr(), ldx, dw.data_ptr(), _rowmajor(dw, "dw"), _ptr(db),
                                 M, N, K, int(accumulate), ws.data_ptr(), nbytes, _stream()), "rp_linear_wgrad")
    return dw, db


def linear_wgrad_xbf16(dy, x16, K: int, want_bias: bool = True):
    """rp_linear_wgrad_xbf16: dw[N, K] = dy^T @ x16[:, :K] with the activation stored as bfloat16 (bf16-storage training)"""
    _req(dy, torch.float32, "dy")
    _req(x16, torch.bfloat16, "x16")
    M, N = dy.shape
    dw = _new((N, K), torch.float32, dy.device)
    db = _new((N,), torch.float32, dy.device) if want_bias else None
    ws, nbytes = _workspace("linear_wgrad", M, N, K, device=dy.device)
    with _Timed("linear_wgrad_xbf16", f"{M}x{N}x{K}", 4 * (M * N + N * K) + 2 * M * K, 2 * M * N * K):
        _check(lib().rp_linear_wgrad_xbf16(dy.data_ptr(), _rowmajor(dy, "dy"), x16.data_ptr(), _rowmajor(x16, "x16"),
                                           dw.data_ptr(), K, _ptr(db), M, N, K, 0, ws.data_ptr(), nbytes, _stream()),
               "rp_linear_wgrad_xbf16")
    return dw, db


GEMM_FWD_FAMILIES = {_RP["RP_GEMM_FWD_" + n.upper()]: n for n in ("f32", "shortk", "colsplit", "wide", "tiled")}
GEMM_TILES = {_RP["RP_GEMM_TILE_128X128"]: "128x128", _RP["RP_GEMM_TILE_128X64_8W"]: "128x64x8w",
              _RP["RP_GEMM_TILE_128X64_4W"]: "128x64x4w"}
GEMM_SK_LAUNCHES = {_RP["RP_GEMM_SK_" + n.upper()]: n for n in ("interior", "right", "bottom", "guarded")}
GEMM_WGRAD_FAMILIES = {_RP["RP_GEMM_WGRAD_" + n.upper()]: n for n in ("f32", "narrow", "wide", "xbf16")}


def linear_fwd_form(M: int, N: int, K: int, lda: int, ldw: int, a_aligned16: bool = True, w_aligned16: bool = True,
                    act: int = ACT_NONE) -> dict:
    """The launch form rp_linear_fwd chooses for this shape under the matmul precision in force (rp_linear_fwd_form: a host
    function, no GPU): family, nprod, tile, vec_a, vec_w, sk (the short-K launches, a tuple of names), per, grid, post_act,
    split_nb."""
    o = (C.c_int * _RP["RP_GEMM_FORM_INTS"])()
    _check(lib().rp_linear_fwd_form(M, N, K, lda, ldw, int(a_aligned16), int(w_aligned16), act, o), "rp_linear_fwd_form")
    family = GEMM_FWD_FAMILIES[o[_RP["RP_GEMM_FAMILY"]]]
    bits = o[_RP["RP_GEMM_FWD_SK_LAUNCHES"]]
    return {"family": family, "nprod": o[_RP["RP_GEMM_NPROD"]],
            "tile": GEMM_TILES[o[_RP["RP_GEMM_FWD_TILE"]]] if family == "tiled" else None,
            "vec_a": bool(o[_RP["RP_GEMM_FWD_VEC_A"]]), "vec_w": bool(o[_RP["RP_GEMM_FWD_VEC_W"]]),
            "sk": tuple(n for b, n in sorted(GEMM_SK_LAUNCHES.items()) if bits & b), "per": o[_RP["RP_GEMM_FWD_SK_PER"]],
            "grid": (o[_RP["RP_GEMM_FWD_GRID_X"]], o[_RP["RP_GEMM_FWD_GRID_Y"]]),
            "post_act": bool(o[_RP["RP_GEMM_FWD_POST_ACT"]]), "split_nb": o[_RP["RP_GEMM_FWD_SPLIT_NB"]]}


def linear_wgrad_form(M: int, N: int, K: int, lddy: int, ldx: int, dy_aligned16: bool = True, x_align_bytes: int = 16,
                      x_is_bf16: bool = False) -> Optional[dict]:
    """The launch form rp_linear_wgrad (x_is_bf16: rp_linear_wgrad_xbf16) chooses (rp_linear_wgrad_form: a host function, no
    GPU): family, nprod, na, vec_x, vec_y, S, rows, grid; None where rp_linear_wgrad_xbf16 refuses the shape."""
    o = (C.c_int * _RP["RP_GEMM_FORM_INTS"])()
    rc = lib().rp_linear_wgrad_form(M, N, K, lddy, ldx, int(dy_aligned16), x_align_bytes, int(x_is_bf16), o)
    if rc == _RP["RP_ERR_UNSUPPORTED"]:
        return None
    _check(rc, "rp_linear_wgrad_form")
    return {"family": GEMM_WGRAD_FAMILIES[o[_RP["RP_GEMM_FAMILY"]]], "nprod": o[_RP["RP_GEMM_NPROD"]],
            "na": o[_RP["RP_GEMM_WGRAD_NA"]], "vec_x": bool(o[_RP["RP_GEMM_WGRAD_VEC_X"]]),
            "vec_y": bool(o[_RP["RP_GEMM_WGRAD_VEC_Y"]]), "S": o[_RP["RP_GEMM_WGRAD_S"]], "rows": o[_RP["RP_GEMM_WGRAD_ROWS"]],
            "grid": (o[_RP["RP_GEMM_WGRAD_GRID_X"]], o[_RP["RP_GEMM_WGRAD_GRID_Y"]], o[_RP["RP_GEMM_WGRAD_GRID_Z"]])}


def transpose(w, rows_out: Optional[int] = None):
    """w [R, C] -> [C, R]; with rows_out > C the result has rows_out rows, the extra ones zero (a dgrad GEMM on it
    then writes exact zeros into the padding columns of a padded activation gradient)."""
    _req(w, torch.float32, "w")
    R, Cc = w.shape
    R4 = (R + 3) // 4 * 4  # 16-byte aligned rows (the GEMM then fetches them with dwordx4, unguarded)
    rows = max(Cc, rows_out or 0)
    out = _new((rows, R4), torch.float32, w.device)[:, :R]
    with _Timed("transpose", f"{R}x{Cc}", 4 * (R * Cc + rows * R)):
        _check(lib().rp_transpose(w.data_ptr(), _rowmajor(w, "w"), out.data_ptr(), R4, R, Cc, rows, _stream()),
               "rp_transpose")
    return out


def transpose_copy(w, rows_out: int, ld_copy: int):
    """(transpose(w, rows_out), copy_rows(w, ld_copy)) from one launch (rp_transpose_copy)"""
    _req(w, torch.float32, "w")
    R, Cc = w.shape
    R4 = (R + 3) // 4 * 4
    rows = max(Cc, rows_out or 0)
    out = _new((rows, R4), torch.float32, w.device)[:, :R]
    buf = _new((R, ld_copy), torch.float32, w.device)
    with _Timed("transpose_copy", f"{R}x{Cc}", 4 * (2 * R * Cc + rows * R)):
        _check(lib().rp_transpose_copy(w.data_ptr(), _rowmajor(w, "w"), out.data_ptr(), R4, R, Cc, rows, buf.data_ptr(), ld_copy,
                                       _stream()), "rp_transpose_copy")
    return out, buf[:, :Cc]


def pieces_ld(K: int, np_: int) -> int:
    """bf16 elements per row of the interleaved-pieces layout (include/rec_pangu_hip.h: rp_pieces_ld)"""
    return int(lib().rp_pieces_ld(int(K), int(np_)))


def pieces_pack(x, np_: int = 2, K: Optional[int] = None, out=None):
    """fp32 [M, >=K] -> bf16 pieces [M, rp_pieces_ld(K, np)] in the interleaved layout (rp_pieces_pack)"""
    _req(x, torch.float32, "x")
    M = x.shape[0]
    K = x.shape[1] if K is None else K
    ldo = pieces_ld(K, np_)
    if out is None:
        out = _new((M, ldo), torch.bfloat16, x.device)
    with _Timed("pieces_pack", f"{M}x{K}x{np_}", 4 * M * K + 2 * M * ldo):
        _check(lib().rp_pieces_pack(x.data_ptr(), _rowmajor(x, "x"), M, K, np_, out.data_ptr(), _rowmajor(out, "out"), _stream()),
               "rp_pieces_pack")
    return out


def linear_fwd_pieces(a_pc, w_pc, bias, K: int, np_: int = 2, act: int = ACT_NONE, aux=None, out=None):
    """out[M,N] = act(a . w^T + bias) on pre-split operands (pieces_pack layout); np = 2 is bit-identical to linear_fwd under
    RP_MATMUL_BF16X3, np = 1 is the plain-bf16 product"""
    _req(a_pc, torch.bfloat16, "a_pc")
    _req(w_pc, torch.bfloat16, "w_pc")
    M, N = a_pc.shape[0], w_pc.shape[0]
    if out is None:
        out = _new((M, N), torch.float32, a_pc.device)
    ldaux = _rowmajor(aux, "aux") if aux is not None else 0
    with _Timed("linear_fwd_pieces", f"{M}x{N}x{K}x{np_}", 2 * (M + N) * pieces_ld(K, np_) + 4 * M * N * (2 if aux is not None else 1),
                2 * M * N * K):
        _check(lib().rp_linear_fwd_pieces(a_pc.data_ptr(), _rowmajor(a_pc, "a_pc"), w_pc.data_ptr(), _rowmajor(w_pc, "w_pc"),
                                          _ptr(bias), out.data_ptr(), _rowmajor(out, "out"), M, N, K, np_, act, _ptr(aux), ldaux,
                                          _stream()), "rp_linear_fwd_pieces")
    return out


def copy_rows(w, ld_out: int):
    """a copy of the 2-D tensor w with row stride ld_out >= w.shape[1] (rp_copy_rows); returns the [R, C] view of it"""
    _req(w, torch.float32, "w")
    R, Cc = w.shape
    buf = _new((R, ld_out), torch.float32, w.device)
    with _Timed("copy_rows", f"{R}x{Cc}", 8 * R * Cc):
        _check(lib().rp_copy_rows(w.data_ptr(), _rowmajor(w, "w"), buf.data_ptr(), ld_out, R, Cc, _stream()), "rp_copy_rows")
    return buf[:, :Cc]


def copy_rows_to(src, dst):
    """dst[r, :] = src[r, :] for 2-D fp32 tensors of one shape with unit inner stride, any row strides (rp_copy_rows): packs a
    matrix into a column block of a wider one, or a column block out into a contiguous matrix"""
    _req(src, torch.float32, "src")
    _req(dst, torch.float32, "dst")
    if src.dim() != 2 or src.shape != dst.shape or src.stride(1) != 1 or dst.stride(1) != 1:
        raise RuntimeError("copy_rows_to: two 2-D tensors of one shape with unit inner stride")
    R, Cc = src.shape
    with _Timed("copy_rows", f"{R}x{Cc}", 8 * R * Cc):
        _check(lib().rp_copy_rows(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), R, Cc, _stream()), "rp_copy_rows")
    return dst


def add_rows_to(src, dst):
    """dst[r, :] += src[r, :] for 2-D fp32 tensors of one shape with unit inner stride, any row strides (rp_add_rows)"""
    _req(src, torch.float32, "src")
    _req(dst, torch.float32, "dst")
    if src.dim() != 2 or src.shape != dst.shape or src.stride(1) != 1 or dst.stride(1) != 1:
        raise RuntimeError("add_rows_to: two 2-D tensors of one shape with unit inner stride")
    R, Cc = src.shape
    with _Timed("add_rows", f"{R}x{Cc}", 12 * R * Cc):
        _check(lib().rp_add_rows(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), R, Cc, _stream()), "rp_add_rows")
    return dst


class Marker:
    """Completion marker on the current stream (rp_marker_*): an event without timing and without a default event's
    system-scope fence.  The host may wait for it; it must not read device memory on its strength."""

    def __init__(self):
        h = _vp()
        _check(lib().rp_marker_create(C.byref(h)), "rp_marker_create")
        self._h = h

    def record(self):
        _check(lib().rp_marker_record(self._h, _stream()), "rp_marker_record")

    def synchronize(self):
        _check(lib().rp_marker_wait(self._h), "rp_marker_wait")

    def __del__(self):
        try:
            if self._h is not None:
                lib().rp_marker_destroy(self._h)
        except Exception:
            pass


# ---- launch plans (csrc/plan.hip; used by graph_step.GraphedTrainStep) -------------------------------------------------
class LaunchPlan:
    """A recorded sequence of the library's kernel launches (rp_plan_*).  `with plan.recording(): ...` records every
    launch issued inside — from any thread — and `plan.replay()` re-issues them on the current stream."""

    def __init__(self):
        self._h = None
        self._streams = None
        self.nodes = self.side = self.streams = self.inline = 0
        self.host_calls = []  # what the caller issues itself between two segments of the replay (host marks); None = a cut
        self.seg_tags = [0]   # per segment: 0 = the replay's stream, 1 = the ahead stream (cut)
        self._tag = 0
        self.ahead_stream = None  # torch stream of the tag-1 segments (set by the owner of the plan)
        self._ev_fork = self._ev_join = None

    _recording = None  # the plan being recorded (host_call appends to it)

    def begin(self):
        h = _vp()
        _check(lib().rp_plan_begin(C.byref(h)), "rp_plan_begin")
        self._h = h
        LaunchPlan._recording = self

    @classmethod
    def host_call(cls, fn) -> bool:
        """Inside a recording: `fn` is work the library does not launch (a collective of the row-sharded path) — it is NOT
        issued now; the plan is cut here (rp_plan_host_mark) and every replay calls fn() between the two segments, on the
        stream of the segments around it.  -> True when the call was taken over (the caller skips issuing it), False outside
        a recording.  fn None: a plain cut (see cut)."""
        pl = cls._recording
        if pl is None or not cls.is_recording():
            return False
        k = _i32()
        _check(lib().rp_plan_host_mark(C.byref(k)), "rp_plan_host_mark")
        assert k.value == len(pl.host_calls)
        pl.host_calls.append(fn)
        pl.seg_tags.append(pl._tag)
        return True

    @classmethod
    def cut(cls, tag: int) -> bool:
        """Inside a recording of a plan that replays in segments (a row-sharded step): the segments recorded from here on —
        and the host calls between them — belong to stream `tag`: 0 = the replay's stream, 1 = the AHEAD stream (the next
        batch's route, id exchange and owner-side sort: work that depends on nothing the step computes; the replay forks it
        at its start and joins it at its end, LaunchPlan.replay)."""
        pl = cls._recording
        if pl is None or not cls.is_recording():
            return False
        pl._tag = int(tag)
        return cls.host_call(None)

    def end(self):
        LaunchPlan._recording = None
        if LaunchPlan._deferred and LaunchPlan.is_recording():
            LaunchPlan.join()  # (nobody joined the inline section after the last deferred launch was queued)
        LaunchPlan._deferred, LaunchPlan._kept = [], []
        _check(lib().rp_plan_end(self._h), "rp_plan_end")
        a, b, c = _i32(), _i32(), _i32()
        _check(lib().rp_plan_info(self._h, C.byref(a), C.byref(b), C.byref(c)), "rp_plan_info")
        self.nodes, self.side, self.streams = a.value, b.value, c.value
        _check(lib().rp_plan_inline_count(self._h, C.byref(a)), "rp_plan_inline_count")
        self.inline = a.value

    def set_streams(self, side, side2):
        """torch streams the side / inline sections are re-issued on (kept alive by the caller)"""
        self._streams = (side, side2)
        _check(lib().rp_plan_set_streams(self._h, _vp(side.cuda_stream) if side is not None else None,
                                         _vp(side2.cuda_stream) if side2 is not None else None), "rp_plan_set_streams")

    @staticmethod
    def section(k: int):
        _check(lib().rp_plan_section(k), "rp_plan_section")

    @classmethod
    @contextlib.contextmanager
    def side2(cls, enabled: bool = True):
        """with LaunchPlan.side2(): the launches issued inside are recorded on the inline section (2: the replay issues them
        on the plan's second side stream); back on the main section afterwards, also behind an exception.  enabled=False
        (no plan is recording): nothing"""
        if enabled:
            cls.section(2)
        try:
            yield
        finally:
            if enabled:
                cls.section(0)

    @staticmethod
    def fork_here():
        _check(lib().rp_plan_fork_here(), "rp_plan_fork_here")

    @staticmethod
    def fork2_mark():
        """the inline section's launches recorded from here on depend on the main stream as it is NOW (rp_plan_fork2_mark)"""
        _check(lib().rp_plan_fork2_mark(), "rp_plan_fork2_mark")

    # launches a recording step wants on the inline section (2) but has no hurry with: issued behind the next launches
    # recorded there (run_deferred), at the latest in front of the section's join.  `_kept` holds the callables until then
    # (join / end), and through their closures the tensors they touch: the capture's allocator would hand that memory to
    # the launches recorded in between
    _deferred: list = []
    _kept: list = []

    @classmethod
    def defer_side(cls, fn):
        cls._deferred.append(fn)
        cls._kept.append(fn)

    @classmethod
    def run_deferred(cls):
        """issue the deferred launches now, on the inline section (the caller may already be inside it)"""
        if not cls._deferred:
            return
        todo, cls._deferred = cls._deferred, []
        with cls.side2():
            for fn in todo:
                fn()

    @classmethod
    def settle(cls):
        """after the backward of a recording step: launches still waiting for the inline section are issued and joined NOW
        (their results are the optimizer's inputs; a step without the fused first-layer node never joined them)"""
        if cls._deferred and cls.is_recording():
            cls.join()

    @classmethod
    def join(cls):
        cls.run_deferred()
        _check(lib().rp_plan_join(), "rp_plan_join")
        cls._kept = []

    @staticmethod
    def side2_sync():
        """the inline section waits here for what the main stream holds at this point (rp_plan_side2_sync)"""
        _check(lib().rp_plan_side2_sync(), "rp_plan_side2_sync")

    @staticmethod
    def is_recording() -> bool:
        return bool(lib().rp_plan_is_recording())

    def replay(self):
        if self.host_calls:  # segments, the caller's own work (collectives) in between
            s = _stream()
            tags, calls, nseg = self.seg_tags, self.host_calls, len(self.host_calls) + 1
            side = self.ahead_stream if any(tags) else None
            if any(tags) and side is None:
                tags = [0] * nseg  # (no ahead stream given: everything in recorded order on the replay's stream)
            if side is not None:
                # fork: the ahead segments depend on what was enqueued BEFORE this replay only (the next batch's staged ids,
                # the previous replay's reads of the buffers they rewrite)
                main = torch.cuda.current_stream()
                if self._ev_fork is None:
                    self._ev_fork, self._ev_join = torch.cuda.Event(), torch.cuda.Event()
                self._ev_fork.record(main)
                side.wait_event(self._ev_fork)
                s1 = _vp(side.cuda_stream)
                # the ahead segments in front of their first host call (the route: launches only) are issued first — beside
                # the step from its start; their collectives follow the step's own (RCCL runs collectives in issue order: an
                # id exchange waiting for the route must not sit in front of the row / gradient exchanges of the step)
                first_side = next(k for k in range(nseg) if tags[k] == 1)
                rc = lib().rp_plan_replay_segment(self._h, first_side, s1)
                if rc != 0:
                    _check(rc, "rp_plan_replay_segment")
            else:
                first_side = -1
            for k in range(nseg):  # the replay's own stream: segments and the host calls between two of them
                if tags[k] == 0:
                    rc = lib().rp_plan_replay_segment(self._h, k, s)
                    if rc != 0:
                        _check(rc, "rp_plan_replay_segment")
                    if k < nseg - 1 and tags[k + 1] == 0 and calls[k] is not None:
                        calls[k]()
            if side is not None:
                with torch.cuda.stream(side):
                    for k in range(first_side, nseg):
                        if tags[k] != 1:
                            continue
                        if k > first_side:
                            if calls[k - 1] is not None and tags[k - 1] == 1:
                                calls[k - 1]()
                            rc = lib().rp_plan_replay_segment(self._h, k, s1)
                            if rc != 0:
                                _check(rc, "rp_plan_replay_segment")
                self._ev_join.record(side)
                main.wait_event(self._ev_join)
            return
        rc = lib().rp_plan_replay(self._h, _stream())
        if rc != 0:
            _check(rc, "rp_plan_replay")

    # ---- live timing of one launch inside replayed steps (bench.py: a replay runs no python between its launches) ------
    def set_probe(self, launch: int):
        """bracket launch `launch` (0 .. nodes - 1, recorded order; -1 = off) of the following replays with a timing-event pair"""
        _check(lib().rp_plan_set_probe(self._h, launch), "rp_plan_set_probe")

    def probe_ms(self) -> float:
        ms = C.c_float(0)
        _check(lib().rp_plan_probe_ms(self._h, C.byref(ms)), "rp_plan_probe_ms")
        return ms.value

    def bind_inputs(self, addrs) -> int:
        """remember where the recorded launch arguments hold the addresses `addrs` (the static input buffers the step was
        recorded on); -> number of argument words found (rp_plan_bind_inputs)"""
        arr = (C.c_uint64 * len(addrs))(*addrs)
        n = _i32()
        _check(lib().rp_plan_bind_inputs(self._h, arr, len(addrs), C.byref(n)), "rp_plan_bind_inputs")
        self._n_inputs = len(addrs)
        self._in_arr = (C.c_uint64 * len(addrs))()
        return n.value

    def bind_report(self, tensors):
        """(sites per input, interior words): how often the recorded launch arguments hold exactly tensors[i].data_ptr(), and
        how many hold an address INSIDE one of the tensors — derived pointers that set_inputs cannot re-point
        (rp_plan_bind_report)"""
        n = len(tensors)
        addrs = (C.c_uint64 * n)(*[t.data_ptr() for t in tensors])
        sizes = (C.c_uint64 * n)(*[t.numel() * t.element_size() for t in tensors])
        sites = (C.c_int32 * n)()
        inner = _i32()
        _check(lib().rp_plan_bind_report(self._h, addrs, sizes, n, sites, C.byref(inner)), "rp_plan_bind_report")
        return list(sites), inner.value

    def set_inputs(self, tensors):
        """the next replays read input i from tensors[i] (rp_plan_set_inputs)"""
        a = self._in_arr
        for i, t in enumerate(tensors):
            a[i] = t.data_ptr()
        _check(lib().rp_plan_set_inputs(self._h, a, self._n_inputs), "rp_plan_set_inputs")

    def slowest_call(self, reset: bool = True):
        """(kind, node, ms) of the slowest HIP call the replays issued since the last reset (kind: launch / record / wait)"""
        k, n, ms = C.c_int(-1), C.c_int(-1), C.c_double(0)
        _check(lib().rp_plan_slowest_call(self._h, C.byref(k), C.byref(n), C.byref(ms), 1 if reset else 0), "rp_plan_slowest_call")
        return (("launch", "record", "wait")[k.value] if k.value >= 0 else None), n.value, ms.value

    def launch_name(self, launch: int):
        """(kernel name as rocprofv3 prints it, section: 0 main stream, 1 side (next batch's sort), 2 inline side)"""
        buf, sec = C.create_string_buffer(512), _i32()
        _check(lib().rp_plan_launch_name(self._h, launch, buf, 512, C.byref(sec)), "rp_plan_launch_name")
        return buf.value.decode("utf-8", "replace"), sec.value

    def destroy(self):
        if self._h is not None and _lib is not None:
            _lib.rp_plan_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


_COPY_PLANS: dict = {}


def make_side_stream(device) -> "torch.cuda.Stream":
    """a stream for work that runs BESIDE the main stream (the next batch's sort, the side work of the first layer's backward):
    of the LOWEST priority the device offers (rp_stream_create_low, wrapped as an ExternalStream), so that the main stream's
    launches are dispatched first — measured in alternating runs on one box: 0.912 / 0.912 -> 0.903 / 0.887 ms per step in the
    20-step window, 0.879 -> 0.866 over 600 steps."""
    with torch.cuda.device(device):
        h = _vp()
        _check(lib().rp_stream_create_low(C.byref(h)), "rp_stream_create_low")
    return torch.cuda.ExternalStream(h.value, device=device)


def multi_copy(dst: Sequence[torch.Tensor], src: Sequence[torch.Tensor]) -> bool:
    """dst[i].copy_(src[i]) for every i in ONE launch (rp_multi_copy).  Only for same-shape, same-dtype, contiguous
    tensors on the current device — returns False (nothing done) otherwise, the caller then copies tensor by tensor."""
    n = len(dst)
    for d, s_ in zip(dst, src):
        if not (d.is_cuda and s_.is_cuda and d.device == s_.device and d.dtype == s_.dtype and d.shape == s_.shape
                and d.is_contiguous() and s_.is_contiguous()):
            return False
    # (the byte counts are part of the key: a re-allocation at the same addresses with another shape or dtype must not
    #  find the old sizes — ADVICE r4)
    key = (tuple(t.data_ptr() for t in dst) + tuple(t.data_ptr() for t in src)
           + tuple(t.numel() * t.element_size() for t in dst))
    arrs = _COPY_PLANS.get(key)
    if arrs is None:
        if len(_COPY_PLANS) >= 256:
            _COPY_PLANS.clear()
        arrs = ((C.c_void_p * n)(*[t.data_ptr() for t in dst]), (C.c_void_p * n)(*[t.data_ptr() for t in src]),
                (C.c_uint64 * n)(*[t.numel() * t.element_size() for t in dst]))
        _COPY_PLANS[key] = arrs
    _check(lib().rp_multi_copy(arrs[0], arrs[1], arrs[2], n, _stream()), "rp_multi_copy")
    return True


class CopyList:
    """rp_multi_copy into a FIXED set of destination tensors (a captured step's static input buffers): the destination
    pointers and byte counts are converted once, a call only fills the source pointers (the general multi_copy validates and
    keys ~40 tensor pairs per call: a third of the host time of a replayed step)."""

    def __init__(self, dst: Sequence[torch.Tensor]):
        self.n = len(dst)
        self.shapes = [(t.shape, t.dtype) for t in dst]
        self.dst = (C.c_void_p * self.n)(*[t.data_ptr() for t in dst])
        self.bytes = (C.c_uint64 * self.n)(*[t.numel() * t.element_size() for t in dst])
        self.src = (C.c_void_p * self.n)()
        self.ok = all(t.is_cuda and t.is_contiguous() for t in dst)

    def __call__(self, src: Sequence[torch.Tensor]) -> bool:
        """copy src[i] into the i-th destination; False (nothing done) unless every source is a contiguous device tensor of the
        destination's shape and dtype"""
        if not self.ok or len(src) != self.n:
            return False
        a = self.src
        for i, t in enumerate(src):
            if not (t.is_cuda and t.is_contiguous() and (t.shape, t.dtype) == self.shapes[i]):
                return False
            a[i] = t.data_ptr()
        _check(lib().rp_multi_copy(self.dst, a, self.bytes, self.n, _stream()), "rp_multi_copy")
        return True


def graph_node_counts(raw_graph: int):
    """(kernel nodes, other nodes) of a captured hipGraph (torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph())"""
    k, o = _i32(), _i32()
    _check(lib().rp_graph_node_counts(_vp(raw_graph), C.byref(k), C.byref(o)), "rp_graph_node_counts")
    return k.value, o.value


def relu_bwd(dy, act_out):
    M, N = dy.shape
    out = _new((M, N), torch.float32, dy.device)
    with _Timed("relu_bwd", f"{M}x{N}", 12 * M * N):
        _check(lib().rp_relu_bwd(dy.data_ptr(), _rowmajor(dy, "dy"), act_out.data_ptr(), _rowmajor(act_out, "act_out"),
                             out.data_ptr(), N, M, N, _stream()), "rp_relu_bwd")
    return out


def act_bwd(dy, act_out, act: int):
    """dy * act'(.) through the activation's output (rp_act_bwd; act = ACT_RELU / TANH / SIGMOID / LEAKY)"""
    M, N = dy.shape
    out = _new((M, N), torch.float32, dy.device)
    with _Timed("act_bwd", f"{M}x{N}", 12 * M * N):
        _check(lib().rp_act_bwd(dy.data_ptr(), _rowmajor(dy, "dy"), act_out.data_ptr(), _rowmajor(act_out, "act_out"),
                                out.data_ptr(), N, M, N, act, _stream()), "rp_act_bwd")
    return out


def act_fwd(x, act: int):
    """act(x) as a launch of its own (rp_act_fwd), 2-D x"""
    M, N = x.shape
    out = _new((M, N), torch.float32, x.device)
    with _Timed("act_fwd", f"{M}x{N}", 8 * M * N):
        _check(lib().rp_act_fwd(x.data_ptr(), _rowmajor(x, "x"), out.data_ptr(), N, M, N, act, _stream()), "rp_act_fwd")
    return out


def crossnet_fwd(x0, d: int, W, Bv, wfc=None, bfc=None, want_x: bool = True):
    """X_L (and/or logit = X_L . wfc + bfc) of the L-layer CrossNet; returns (xout, logit, s)."""
    _req(x0, torch.float32, "x0")
    B, L = x0.shape[0], W.shape[0]
    dev = x0.device
    xout = _new((B, d), torch.float32, dev) if want_x else None
    logit = _new((B, 1), torch.float32, dev) if wfc is not None else None
    s = _new((B, L), torch.float32, dev)
    with _Timed("crossnet_fwd"):
        _check(lib().rp_crossnet_fwd(x0.data_ptr(), _rowmajor(x0, "x0"), d, L, W.data_ptr(), Bv.data_ptr(), _ptr(wfc),
                                     _ptr(bfc), _ptr(xout), d, _ptr(logit), s.data_ptr(), B, _stream()),
               "rp_crossnet_fwd")
    return xout, logit, s


def crossnet_bwd_rows(x0, d: int, W, wfc, s, g_x, g_logit):
    """-> dx0 [B, x0.shape[1]] (columns >= d zeroed), V [B, 2L+2] (see rp_crossnet_bwd_rows)."""
    B, L = x0.shape[0], W.shape[0]
    dx0 = _new_like(x0)
    ldg = _rowmajor(g_x, "g_x") if g_x is not None else 0
    # the vectorised kernel writes whole dwordx4 up to the leading dimension (exact zeros beyond d); only the unaligned form
    # leaves the padding columns to a fill (an ATen launch: it kept a DCN step from replaying as a launch plan)
    vec = (x0.stride(0) % 4 == 0 and dx0.stride(0) % 4 == 0 and x0.data_ptr() % 16 == 0 and dx0.data_ptr() % 16 == 0
           and (g_x is None or (ldg % 4 == 0 and g_x.data_ptr() % 16 == 0)) and x0.shape[1] <= (d + 255) // 256 * 256)
    if x0.shape[1] > d and not vec:
        dx0[:, d:].zero_()
    V = _new((B, 2 * L + 2), torch.float32, x0.device)
    with _Timed("crossnet_bwd_rows"):
        _check(lib().rp_crossnet_bwd_rows(x0.data_ptr(), _rowmajor(x0, "x0"), d, L, W.data_ptr(), _ptr(wfc),
                                          s.data_ptr(), _ptr(g_x), ldg, _ptr(g_logit), dx0.data_ptr(),
                                          _rowmajor(dx0, "dx0"), V.data_ptr(), B, _stream()), "rp_crossnet_bwd_rows")
    return dx0, V


def crossnet_param_grads(P, cs, W, Bv, wfc, colg):
    """(dW [L, d], dB [L, d], dwfc [d] or None) of the CrossNet from the skinny weight gradient P = V^T X_0 and the column
    sums cs of V (rp_crossnet_param_grads)"""
    L, d = W.shape
    dW = _new((L, d), torch.float32, W.device)
    dB = _new((L, d), torch.float32, W.device)
    dwfc = _new((d,), torch.float32, W.device) if wfc is not None else None
    with _Timed("crossnet_param_grads", f"{L}x{d}"):
        _check(lib().rp_crossnet_param_grads(P.data_ptr(), _rowmajor(P, "P"), cs.data_ptr(), W.data_ptr(), Bv.data_ptr(), _ptr(wfc),
                                             _ptr(colg), L, d, dW.data_ptr(), dB.data_ptr(), _ptr(dwfc), _stream()),
               "rp_crossnet_param_grads")
    return dW, dB, dwfc


def cin_layer_fwd(x0, xp, W, bias, H: int, M: int, D: int, want_out: bool, want_pool: bool):
    """One CIN layer.  x0 [B, >=H*D], xp [B, >=M*D] (pass the same tensor for the first layer), W [O, H*M].
    -> (out [B,O,D] or None, pooled [B,O] or None)."""
    _req(x0, torch.float32, "x0")
    _req(xp, torch.float32, "xp")
    B, O = x0.shape[0], W.shape[0]
    out = _new((B, O, D), torch.float32, x0.device) if want_out else None
    pooled = _new((B, O), torch.float32, x0.device) if want_pool else None
    with _Timed("cin_layer_fwd"):
        _check(lib().rp_cin_layer_fwd(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"),
                                      W.data_ptr(), _ptr(bias), _ptr(out), _ptr(pooled), O, H, M, O, D, B, _stream()),
               "rp_cin_layer_fwd")
    return out, pooled


def cin_layer_bwd(x0, xp, W, H: int, M: int, D: int, g_out, g_pool, want_bias: bool):
    """Gradients of one CIN layer: -> (dx0 like x0, dxp [B, M*D] or None when xp is x0, dW like W, dbias [O] or None)."""
    B, O = x0.shape[0], W.shape[0]
    same = xp is x0
    dx0 = _new_like(x0)
    if x0.shape[1] > H * D:
        dx0[:, H * D:].zero_()
    dxp = None if same else _new((B, M * D), torch.float32, x0.device)
    ldgp = _rowmajor(g_pool, "g_pool") if g_pool is not None else 0
    with _Timed("cin_layer_bwd_x"):
        _check(lib().rp_cin_layer_bwd_x(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"),
                                        W.data_ptr(), _ptr(g_out), _ptr(g_pool), ldgp, dx0.data_ptr(),
                                        _rowmajor(dx0, "dx0"), 0, _ptr(dxp), M * D, H, M, O, D, B, _stream()),
               "rp_cin_layer_bwd_x")
    return (dx0, dxp) + cin_layer_bwd_w(x0, xp, W, H, M, D, g_out, g_pool, want_bias)


def field_attention_fits(T: int, Din: int, H: int, a: int, has_res: bool) -> bool:
    return bool(lib().rp_field_attention_fits(T, Din, H, a, int(has_res)))


def field_attention_fwd(x, W, T: int, Din: int, H: int, a: int, has_res: bool, scale: float):
    """x [B, >=T*Din] (tokens contiguous per sample) -> out [B, T, H*a]."""
    _req(x, torch.float32, "x")
    _req(W, torch.float32, "W")
    B = x.shape[0]
    out = _new((B, T, H * a), torch.float32, x.device)
    with _Timed("field_attention_fwd"):
        _check(lib().rp_field_attention_fwd(x.data_ptr(), _rowmajor(x, "x"), W.data_ptr(), T, Din, H, a, int(has_res),
                                            scale, out.data_ptr(), B, _stream()), "rp_field_attention_fwd")
    return out


def field_attention_bwd(x, W, T: int, Din: int, H: int, a: int, has_res: bool, scale: float, gout, want_dx: bool):
    B = x.shape[0]
    dx = None
    if want_dx:
        dx = _new_like(x)
        if x.shape[1] > T * Din:
            dx[:, T * Din:].zero_()
    dW = _new_like(W)
    ws, nbytes = _workspace("field_attention_bwd", B, T, Din, H, a, int(has_res), device=x.device)
    with _Timed("field_attention_bwd"):
        _check(lib().rp_field_attention_bwd(x.data_ptr(), _rowmajor(x, "x"), W.data_ptr(), T, Din, H, a, int(has_res),
                                            scale, gout.data_ptr(), _ptr(dx), _rowmajor(dx, "dx") if want_dx else 0,
                                            dW.data_ptr(), B, ws.data_ptr(), nbytes, _stream()),
               "rp_field_attention_bwd")
    return dx, dW


def cin_bs_fits(H: int, M: int, D: int) -> bool:
    return bool(lib().rp_cin_bs_fits(H, M, D))


def bf16_pieces(w3: torch.Tensor) -> torch.Tensor:
    """[O, R, C] fp32 (R, C <= 32) -> [O, 3, 32, 32] bf16: (hi, mid, lo) with w = hi + mid + lo (+ 2^-24 |w|), zero
    padded — the operand format of the split-bf16 matrix-core kernels (round-to-nearest-even conversions, exactly
    what v_cvt_pk_bf16_f32 does in the kernels that split on the fly)."""
    O, R, Cc = w3.shape
    pad = _new((O, 32, 32), torch.float32, w3.device).zero_()
    pad[:, :R, :Cc] = w3
    hi = pad.to(torch.bfloat16)
    r1 = pad - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo], dim=1).contiguous()


def cin_bs_fwd(x0, xp, wp, bias, H: int, M: int, O: int, D: int, want_out: bool, want_pool: bool):
    B = x0.shape[0]
    out = _new((B, O, D), torch.float32, x0.device) if want_out else None
    pooled = _new((B, O), torch.float32, x0.device) if want_pool else None
    with _Timed("cin_bs_fwd"):
        _check(lib().rp_cin_bs_fwd(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"), wp.data_ptr(),
                                   _ptr(bias), H, M, O, D, _ptr(out), _ptr(pooled), B, _stream()), "rp_cin_bs_fwd")
    return out, pooled


def accumulate(dst, src):
    """dst += src (contiguous fp32 tensors of one size; rp_accumulate)"""
    _req(dst, torch.float32, "dst")
    _req(src, torch.float32, "src")
    assert dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel()
    with _Timed("accumulate", None, 12 * dst.numel()):
        _check(lib().rp_accumulate(dst.data_ptr(), src.data_ptr(), dst.numel(), _stream()), "rp_accumulate")
    return dst


def cin_bs_bwd_x(xk, wp, g_out, g_pool, R: int, Cn: int, O: int, D: int, like, out=None):
    """-> dx shaped like `like` ([B, >= R*D], zero beyond R*D), or written into `out` ([B, R*D] view, any leading
    dimension)."""
    B = xk.shape[0]
    dx = out if out is not None else _new_like(like)
    if out is None and like.shape[1] > R * D:
        dx[:, R * D:].zero_()
    with _Timed("cin_bs_bwd_x"):
        _check(lib().rp_cin_bs_bwd_x(xk.data_ptr(), _rowmajor(xk, "xk"), wp.data_ptr(), _ptr(g_out), _ptr(g_pool), R, Cn, O,
                                     D, dx.data_ptr(), _rowmajor(dx, "dx"), B, _stream()), "rp_cin_bs_bwd_x")
    return dx


def cin_bs_bwd_w(x0, xp, g_out, g_pool, H: int, M: int, O: int, D: int, want_bias: bool):
    """dW [O, H*M], dbias [O] or None on the bf16 matrix core (rp_cin_bs_bwd_w); g_pool must be packed [B, O]."""
    B = x0.shape[0]
    dW = _new((O, H * M), torch.float32, x0.device)
    db = _new((O,), torch.float32, x0.device) if want_bias else None
    ws, nbytes = _workspace("cin_bs_bwd_w", B, O, device=x0.device)
    with _Timed("cin_bs_bwd_w"):
        _check(lib().rp_cin_bs_bwd_w(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"), _ptr(g_out),
                                     _ptr(g_pool), H, M, O, D, dW.data_ptr(), _ptr(db), B, ws.data_ptr(), nbytes,
                                     _stream()), "rp_cin_bs_bwd_w")
    return dW, db


def cin_pair_fits(H: int, O: int, D: int) -> bool:
    return bool(lib().rp_cin_pair_fits(H, O, D))


def cin_pair_pieces(W3, transposed: bool = False, both: bool = False):
    """W [O, H, H] -> the symmetric pair weights Ws[o, (h<=m)] = W[o,h,m] + W[o,m,h] (W[o,h,h] on the diagonal) as bf16
    pieces: [3, 128, KP] (rp_cin_pair_fwd's wsp, KP = pairs rounded up to 32) or, transposed, [3, KPT, 128]
    (rp_cin_pair_bwd_x's wst, KPT = pairs rounded up to 128); both: (wsp, wst) from ONE launch (rp_cin_pair_pieces, round 6:
    the fold + split were ~18 torch launches per layout and step)."""
    _req(W3, torch.float32, "W")
    O, H = W3.shape[0], W3.shape[1]
    W3 = W3.contiguous()
    npair = H * (H + 1) // 2
    dev = W3.device
    wsp = _new((3, 128, (npair + 31) // 32 * 32), torch.bfloat16, dev) if (both or not transposed) else None
    wst = _new((3, (npair + 127) // 128 * 128, 128), torch.bfloat16, dev) if (both or transposed) else None
    _check(lib().rp_cin_pair_pieces(W3.data_ptr(), O, H, _ptr(wsp), _ptr(wst), _stream()), "rp_cin_pair_pieces")
    return (wsp, wst) if both else (wst if transposed else wsp)


def cin_head_params_fwd(WL, bL, c, H: int, M: int):
    """-> (vt [M, 32], vb [1]): V^T = (c . W_L)^T zero padded and c . b_L of the collapsed last CIN layer (rp_cin_head_params_fwd)"""
    O = WL.shape[0]
    vt = _new((M, 32), torch.float32, WL.device)
    vb = _new((1,), torch.float32, WL.device)
    _check(lib().rp_cin_head_params_fwd(WL.data_ptr(), _ptr(bL), c.data_ptr(), O, H, M, vt.data_ptr(), vb.data_ptr(), _stream()),
           "rp_cin_head_params_fwd")
    return vt, vb


def cin_head_params_bwd(WL, bL, c, dV, sg, D: int, H: int, M: int):
    """-> (dWL [O, H M], dbL [O] or None, dc [O]) of the collapsed last layer's weights from dV [H, M] and sg = sum g
    (rp_cin_head_params_bwd)"""
    O = WL.shape[0]
    dWL = _new((O, H * M), torch.float32, WL.device)
    dbL = _new((O,), torch.float32, WL.device) if bL is not None else None
    dc = _new((O,), torch.float32, WL.device)
    _check(lib().rp_cin_head_params_bwd(WL.data_ptr(), _ptr(bL), c.data_ptr(), dV.data_ptr(), sg.data_ptr(), float(D), O, H, M,
                                        dWL.data_ptr(), _ptr(dbL), dc.data_ptr(), _stream()), "rp_cin_head_params_bwd")
    return dWL, dbL, dc


def add_scalars(out, a, scale: float, b0=None):
    """out[i] += scale * a[0] + (b0[0] if b0 is given), in place (rp_add_scalars)"""
    assert out.is_contiguous() and out.dtype == torch.float32
    _check(lib().rp_add_scalars(out.data_ptr(), out.numel(), a.data_ptr(), float(scale), _ptr(b0), _stream()), "rp_add_scalars")
    return out


def sum_all(x):
    """-> [1] = the sum of x's elements in a fixed order (rp_sum_all)"""
    assert x.is_contiguous() and x.dtype == torch.float32
    out = _new((1,), torch.float32, x.device)
    _check(lib().rp_sum_all(x.data_ptr(), x.numel(), out.data_ptr(), _stream()), "rp_sum_all")
    return out


_PAIR_LISTS = {}


def cin_pair_lists(H: int, device):
    """(lstart, lent) of rp_cin_pair_bwd_x for H fields, built once per (H, device)."""
    key = (H, str(device))
    if key not in _PAIR_LISTS:
        pairs = [(h, m) for h in range(H) for m in range(h, H)]  # row-major upper triangle
        ntile = (len(pairs) + 127) // 128
        lstart, lent = [0], []
        for tile in range(ntile):
            for half in range(2):
                lo = tile * 128 + half * 64
                loc = {}
                for pl, (h, m) in enumerate(pairs[lo:lo + 64]):
                    loc.setdefault(h, []).append(pl | (m << 8))
                    loc.setdefault(m, []).append(pl | (h << 8))  # (h == m: the diagonal pair twice)
                for h in range(H):
                    lent.extend(loc.get(h, []))
                    lstart.append(len(lent))
        _PAIR_LISTS[key] = (torch.tensor(lstart, dtype=torch.int32, device=device),
                            torch.tensor(lent if lent else [0], dtype=torch.int32, device=device))
    return _PAIR_LISTS[key]


def cin_pair_bwd_x(x0, wst, g_out, g_pool, H: int, O: int, D: int, like, into=None):
    """-> dX_0 shaped like `like` ([B, >= H*D], zero beyond H*D) in the pair form (rp_cin_pair_bwd_x).  into: a [B, >= H*D]
    tensor the gradient is ADDED to and that is returned (the collapsed last layer's gradient of X_0: no pass of its own)"""
    B = x0.shape[0]
    if into is not None:
        _req(into, torch.float32, "into")
        assert into.shape[0] == B and into.shape[1] >= H * D and into.stride(1) == 1
        dx = into
    else:
        dx = _new_like(like)
        if like.shape[1] > H * D:
            dx[:, H * D:].zero_()
    lstart, lent = cin_pair_lists(H, x0.device)
    with _Timed("cin_pair_bwd_x"):
        _check(lib().rp_cin_pair_bwd_x(x0.data_ptr(), _rowmajor(x0, "x0"), wst.data_ptr(), _ptr(g_out), _ptr(g_pool),
                                       lstart.data_ptr(), lent.data_ptr(), H, O, D, dx.data_ptr(), _rowmajor(dx, "dx"), B,
                                       1 if into is not None else 0, _stream()), "rp_cin_pair_bwd_x")
    return dx


def cin_pair_fwd(x0, wsp, bias, H: int, O: int, D: int, want_out: bool, want_pool: bool):
    B = x0.shape[0]
    out = _new((B, O, D), torch.float32, x0.device) if want_out else None
    pooled = _new((B, O), torch.float32, x0.device) if want_pool else None
    with _Timed("cin_pair_fwd"):
        _check(lib().rp_cin_pair_fwd(x0.data_ptr(), _rowmajor(x0, "x0"), wsp.data_ptr(), _ptr(bias), H, O, D, _ptr(out),
                                     _ptr(pooled), B, _stream()), "rp_cin_pair_fwd")
    return out, pooled


def cin_pair_bwd_w(x0, g_out, g_pool, H: int, O: int, D: int, want_bias: bool):
    """first-layer dW [O, H*H], dbias [O] or None in the symmetric pair form (rp_cin_pair_bwd_w); O <= 128."""
    B = x0.shape[0]
    dW = _new((O, H * H), torch.float32, x0.device)
    db = _new((O,), torch.float32, x0.device) if want_bias else None
    ws, nbytes = _workspace("cin_pair_bwd_w", B, H, O, device=x0.device)
    with _Timed("cin_pair_bwd_w"):
        _check(lib().rp_cin_pair_bwd_w(x0.data_ptr(), _rowmajor(x0, "x0"), _ptr(g_out), _ptr(g_pool), H, O, D, dW.data_ptr(),
                                       _ptr(db), B, ws.data_ptr(), nbytes, _stream()), "rp_cin_pair_bwd_w")
    return dW, db


def cin_layer_bwd_w(x0, xp, W, H: int, M: int, D: int, g_out, g_pool, want_bias: bool):
    """dW like W, dbias [O] or None (rp_cin_layer_bwd_w alone)."""
    B, O = x0.shape[0], W.shape[0]
    ldgp = _rowmajor(g_pool, "g_pool") if g_pool is not None else 0
    dW = _new_like(W)
    db = _new((O,), torch.float32, x0.device) if want_bias else None
    ws, nbytes = _workspace("cin_layer_bwd_w", B, H, M, O, device=x0.device)
    with _Timed("cin_layer_bwd_w"):
        _check(lib().rp_cin_layer_bwd_w(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"),
                                        _ptr(g_out), _ptr(g_pool), ldgp, dW.data_ptr(), _ptr(db), H, M, O, D, B,
                                        ws.data_ptr(), nbytes, _stream()), "rp_cin_layer_bwd_w")
    return dW, db


def cin_last_fits(H: int, M: int, D: int) -> bool:
    return bool(lib().rp_cin_last_fits(H, M, D))


def cin_last_fwd(x0, xp, vt, H: int, M: int, D: int):
    """x0 [B, >=H*D], xp [B, >=M*D], vt [M, 32] (V^T zero padded) -> pooled [B, 1]."""
    _req(x0, torch.float32, "x0")
    B = x0.shape[0]
    pooled = _new((B, 1), torch.float32, x0.device)
    with _Timed("cin_last_fwd"):
        _check(lib().rp_cin_last_fwd(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"), vt.data_ptr(),
                                     H, M, D, pooled.data_ptr(), B, _stream()), "rp_cin_last_fwd")
    return pooled


def cin_last_bwd(x0, xp, vt, g, H: int, M: int, D: int):
    """-> dx0 (shape of x0, zero beyond H*D), dxp (shape of xp), dV [H, M]."""
    B = x0.shape[0]
    dx0, dxp = _new_like(x0), _new_like(xp)
    if x0.shape[1] > H * D:
        dx0[:, H * D:].zero_()
    if xp.shape[1] > M * D:
        dxp[:, M * D:].zero_()
    with _Timed("cin_last_bwd_x"):
        _check(lib().rp_cin_last_bwd_x(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"),
                                       vt.data_ptr(), g.data_ptr(), H, M, D, dx0.data_ptr(), _rowmajor(dx0, "dx0"),
                                       dxp.data_ptr(), _rowmajor(dxp, "dxp"), B, _stream()), "rp_cin_last_bwd_x")
    dV = _new((H, M), torch.float32, x0.device)
    ws, nbytes = _workspace("cin_last_bwd_v", B, H, M, device=x0.device)
    with _Timed("cin_last_bwd_v"):
        _check(lib().rp_cin_last_bwd_v(x0.data_ptr(), _rowmajor(x0, "x0"), xp.data_ptr(), _rowmajor(xp, "xp"), g.data_ptr(),
                                       H, M, D, dV.data_ptr(), B, ws.data_ptr(), nbytes, _stream()),
               "rp_cin_last_bwd_v")
    return dx0, dxp, dV


def attention_core_fits(T: int, H: int, a: int) -> bool:
    return bool(lib().rp_attention_core_fits(T, H, a))


def attention_core_fwd(qkvr, nproj: int, xres, T: int, H: int, a: int, scale: float):
    """qkvr [B*T, nproj*H*a] (Q|K|V|R), xres [B*T, H*a] when nproj == 3 -> out [B*T, H*a], stats [B, H*T, 2]."""
    _req(qkvr, torch.float32, "qkvr")
    BT = qkvr.shape[0]
    B = BT // T
    out = _new((BT, H * a), torch.float32, qkvr.device)
    stats = _new((B, H * T, 2), torch.float32, qkvr.device)
    with _Timed("attention_core_fwd"):
        _check(lib().rp_attention_core_fwd(qkvr.data_ptr(), _rowmajor(qkvr, "qkvr"), nproj, _ptr(xres),
                                           _rowmajor(xres, "xres") if xres is not None else 0, T, H, a, scale,
                                           out.data_ptr(), stats.data_ptr(), B, _stream()), "rp_attention_core_fwd")
    return out, stats


def attention_core_bwd(qkvr, nproj: int, out, dout, stats, T: int, H: int, a: int, scale: float):
    BT = qkvr.shape[0]
    dqkvr = _new_like(qkvr)
    dxres = _new((BT, H * a), torch.float32, qkvr.device) if nproj == 3 else None
    with _Timed("attention_core_bwd"):
        _check(lib().rp_attention_core_bwd(qkvr.data_ptr(), _rowmajor(qkvr, "qkvr"), nproj, out.data_ptr(), dout.data_ptr(),
                                           stats.data_ptr(), T, H, a, scale, dqkvr.data_ptr(), _rowmajor(dqkvr, "dqkvr"),
                                           _ptr(dxres), H * a if dxres is not None else 0, BT // T, _stream()),
               "rp_attention_core_bwd")
    return dqkvr, dxres


def attention_wide_fits(T: int, H: int, a: int) -> bool:
    """the few-token, one-wide-head form of the attention core (rp_attention_wide_*): H == 1, 2 <= T <= 4, a <= 65536"""
    return bool(lib().rp_attention_wide_fits(T, H, a))


def _attention_wide_dims(qkv, xres, T: int, a: int):
    ldq = _rows(qkv, "attention_wide: qkv", 3 * a)
    BT = qkv.shape[0]
    ldr = _rows(xres, "attention_wide: xres", a, BT)
    if BT % T != 0 or BT == 0:
        raise RuntimeError(f"attention_wide: qkv {tuple(qkv.shape)} does not hold B*{T} token rows")
    _req(qkv, torch.float32, "qkv")
    _req(xres, torch.float32, "xres")
    return BT // T, ldq, ldr


def attention_wide_fwd(qkv, xres, T: int, a: int, scale: float, sum_tokens: bool):
    """qkv [B*T, >=3a] (Q|K|V), xres [B*T, >=a] -> relu(softmax(Q K^T [/scale]) V + xres): [B*T, a], or its sum over the
    tokens [B, a] when sum_tokens"""
    B, ldq, ldr = _attention_wide_dims(qkv, xres, T, a)
    out = _new((B if sum_tokens else B * T, a), torch.float32, qkv.device)
    with _Timed("attention_wide_fwd", f"{B}x{T}x{a}", 4 * (4 * B * T * a + out.numel())):
        _check(lib().rp_attention_wide_fwd(qkv.data_ptr(), ldq, xres.data_ptr(), ldr, T, 1, a, scale, int(sum_tokens),
                                           out.data_ptr(), B, _stream()), "rp_attention_wide_fwd")
    return out


def attention_wide_bwd(qkv, xres, dout, T: int, a: int, scale: float, sum_tokens: bool):
    """-> (dqkv [B*T, 3a], dxres [B*T, a]) from the cotangent dout (shaped like attention_wide_fwd's result, contiguous)"""
    B, ldq, ldr = _attention_wide_dims(qkv, xres, T, a)
    _req(dout, torch.float32, "dout")
    if not dout.is_contiguous() or dout.numel() != (B if sum_tokens else B * T) * a:
        raise RuntimeError("attention_wide_bwd: dout must be contiguous and shaped like the forward's result")
    dqkv = _new((B * T, 3 * a), torch.float32, qkv.device)
    dxres = _new((B * T, a), torch.float32, qkv.device)
    with _Timed("attention_wide_bwd", f"{B}x{T}x{a}", 4 * (6 * B * T * a + dout.numel() + 4 * B * T * a)):
        _check(lib().rp_attention_wide_bwd(qkv.data_ptr(), ldq, xres.data_ptr(), ldr, dout.data_ptr(), T, 1, a, scale,
                                           int(sum_tokens), dqkv.data_ptr(), 3 * a, dxres.data_ptr(), a, B, _stream()),
               "rp_attention_wide_bwd")
    return dqkv, dxres


def mmoe_combine_fwd(z, K: int, E: int, T: int):
    """z [B, >=K*E+T*E] -> (out [T,B,K], gate [B,T*E])."""
    _req(z, torch.float32, "z")
    B = z.shape[0]
    out = _new((T, B, K), torch.float32, z.device)
    gate = _new((B, T * E), torch.float32, z.device)
    with _Timed("mmoe_combine_fwd"):
        _check(lib().rp_mmoe_combine_fwd(z.data_ptr(), _rowmajor(z, "z"), K, E, T, out.data_ptr(), gate.data_ptr(), B,
                                         _stream()), "rp_mmoe_combine_fwd")
    return out, gate


def mmoe_combine_bwd(z, K: int, E: int, T: int, gate, dout):
    """dout [T,B,K] -> dz [B, K*E+T*E]."""
    B = z.shape[0]
    dz = _new((B, K * E + T * E), torch.float32, z.device)
    with _Timed("mmoe_combine_bwd"):
        _check(lib().rp_mmoe_combine_bwd(z.data_ptr(), _rowmajor(z, "z"), K, E, T, gate.data_ptr(), dout.data_ptr(),
                                         dz.data_ptr(), K * E + T * E, B, _stream()), "rp_mmoe_combine_bwd")
    return dz


MATMUL_MODES = {m: _RP["RP_MATMUL_" + m.upper()] for m in ("fp32", "bf16", "auto", "bf16x3", "bf16x6")}


def set_matmul_precision(mode: str):
    """GEMM matrix-core mode: 'auto' (default: per launch 'bf16x3' when matrix-core bound, 'bf16x6' when HBM-bound),
    'bf16x6' (fp32-faithful split-bf16), 'bf16x3', 'bf16', 'fp32' (f32 MFMA)."""
    _check(lib().rp_set_matmul_precision(MATMUL_MODES[mode]), "rp_set_matmul_precision")


def get_matmul_precision() -> str:
    v = lib().rp_get_matmul_precision()
    return {n: k for k, n in MATMUL_MODES.items()}[v]


def fm_pool_fwd(x2d, F: int, D: int, want_sum: bool, want_bi: bool):
    """x2d [B, >=F*D] -> (sum [B,1] or None, bi [B,D] or None)."""
    _req(x2d, torch.float32, "x")
    B = x2d.shape[0]
    out_sum = _new((B, 1), torch.float32, x2d.device) if want_sum else None
    out_bi = _new((B, D), torch.float32, x2d.device) if want_bi else None
    with _Timed("fm_pool_fwd"):
        _check(lib().rp_fm_pool_fwd(x2d.data_ptr(), _rowmajor(x2d, "x"), F, D, _ptr(out_sum), _ptr(out_bi), B,
                                    _stream()), "rp_fm_pool_fwd")
    return out_sum, out_bi


def fm_pool_bwd(x2d, F: int, D: int, g_sum, g_bi):
    dx = _new_like(x2d)
    if x2d.shape[1] > F * D:
        dx[:, F * D:].zero_()
    with _Timed("fm_pool_bwd"):
        _check(lib().rp_fm_pool_bwd(x2d.data_ptr(), _rowmajor(x2d, "x"), F, D, _ptr(g_sum), _ptr(g_bi), dx.data_ptr(),
                                    _rowmajor(dx, "dx"), x2d.shape[0], _stream()), "rp_fm_pool_bwd")
    return dx


def batchnorm_train_fwd(x, gamma, beta, eps: float):
    """-> y, mean [N], var [N] (biased), rstd [N]"""
    _req(x, torch.float32, "x")
    M, N = x.shape
    dev = x.device
    y = _new((M, N), torch.float32, dev)
    mean, var, rstd = (_new((N,), torch.float32, dev) for _ in range(3))
    ws, nb = _workspace("batchnorm", M, N, device=dev)
    with _Timed("batchnorm_train_fwd", f"{M}x{N}", 16 * M * N):  # 3 reads + 1 write
        _check(lib().rp_batchnorm_train_fwd(x.data_ptr(), _rowmajor(x, "x"), _ptr(gamma), _ptr(beta), eps, y.data_ptr(),
                                            N, mean.data_ptr(), var.data_ptr(), rstd.data_ptr(), M, N, ws.data_ptr(),
                                            nb, _stream()), "rp_batchnorm_train_fwd")
    return y, mean, var, rstd


def batchnorm_train_bwd(x, dy, mean, rstd, gamma):
    M, N = x.shape
    dev = x.device
    dx = _new((M, N), torch.float32, dev)
    dgamma, dbeta = (_new((N,), torch.float32, dev) for _ in range(2))
    ws, nb = _workspace("batchnorm", M, N, device=dev)
    with _Timed("batchnorm_train_bwd", f"{M}x{N}", 20 * M * N):  # x, dy twice + dx
        _check(lib().rp_batchnorm_train_bwd(x.data_ptr(), _rowmajor(x, "x"), dy.data_ptr(), _rowmajor(dy, "dy"),
                                            mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), dx.data_ptr(), N,
                                            dgamma.data_ptr(), dbeta.data_ptr(), M, N, ws.data_ptr(), nb, _stream()),
               "rp_batchnorm_train_bwd")
    return dx, dgamma, dbeta


def batchnorm_apply(x, mean, rstd, gamma, beta):
    M, N = x.shape
    y = _new((M, N), torch.float32, x.device)
    with _Timed("batchnorm_apply", f"{M}x{N}", 8 * M * N):
        _check(lib().rp_batchnorm_apply(x.data_ptr(), _rowmajor(x, "x"), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma),
                                        _ptr(beta), y.data_ptr(), N, M, N, _stream()), "rp_batchnorm_apply")
    return y


def layernorm_fwd(x, gamma, beta, eps: float, mul=None, out=None, out_scale: float = 1.0, accumulate: bool = False,
                  stats=None, stats_given: bool = False):
    """-> (y, stats).  y = out_scale * (LayerNorm(x[:, :N]) [* mul[:, :N]]) over the N = gamma.numel() leading columns of the
    2-D x, written (accumulate: added) into `out` [M, >= N] (default: a fresh [M, N]); out's columns from N on are written
    as zeros.  stats [M, 2] = (mean, 1 / sqrt(var + eps)) per row: made here or, with stats_given, read."""
    N = gamma.numel()
    ldx = _rows(x, "layernorm_fwd: x", N)
    M = x.shape[0]
    ldmul = _rows(mul, "layernorm_fwd: mul", N, M) if mul is not None else 0
    if beta.numel() != N:
        raise RuntimeError(f"layernorm_fwd: beta of {beta.numel()} elements against {N} normalised columns")
    if out is not None:
        _rows(out, "layernorm_fwd: out", N, M)
    if stats is None and stats_given:
        raise RuntimeError("layernorm_fwd: stats_given without stats")
    _req(x, torch.float32, "x")
    _req(gamma, torch.float32, "gamma")
    _req(beta, torch.float32, "beta")
    if out is None:
        out = _new((M, N), torch.float32, x.device)
    if stats is None:
        stats = _new((M, 2), torch.float32, x.device)
    with _Timed("layernorm_fwd", f"{M}x{N}" + ("*mul" if mul is not None else "") + ("+=" if accumulate else ""),
                4 * M * N * (2 + (mul is not None) + bool(accumulate))):
        _check(lib().rp_layernorm_fwd(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), eps, _ptr(mul), ldmul,
                                      out.data_ptr(), _rowmajor(out, "out"), out.shape[1], out_scale, int(accumulate),
                                      _ptr(stats), int(stats_given), M, N, _stream()), "rp_layernorm_fwd")
    return out, stats


def layernorm_bwd(dy, x, stats, gamma, beta, mul=None, dy_scale: float = 1.0, dx=None, accumulate: bool = False):
    """-> (dx, dmul, dgamma, dbeta) of layernorm_fwd for the incoming dy [M, >= N] (times dy_scale).  dx [M, x.shape[1]]
    (fresh, or the given one; accumulate: added to it), zeros in its columns from N on; dmul [M, mul.shape[1]] (columns
    from N on are not written) or None."""
    N = gamma.numel()
    _rows(x, "layernorm_bwd: x", N)
    M, dev = x.shape[0], x.device
    for name, buf in (("dy", dy), ("mul", mul), ("dx", dx)):
        if buf is not None:
            _rows(buf, "layernorm_bwd: " + name, N, M)
    _req(dy, torch.float32, "dy")
    _req(x, torch.float32, "x")
    if dx is None:
        if accumulate:
            raise RuntimeError("layernorm_bwd: accumulate without dx")
        dx = _new((M, x.shape[1]), torch.float32, dev)
    dmul = _new((M, mul.shape[1]), torch.float32, dev) if mul is not None else None
    dgamma, dbeta = (_new((N,), torch.float32, dev) for _ in range(2))
    if M == 0:
        return dx, dmul, dgamma.zero_(), dbeta.zero_()
    ws, nbytes = _workspace("layernorm_bwd", N, device=dev)
    with _Timed("layernorm_bwd", f"{M}x{N}" + ("*mul" if mul is not None else "") + ("+=" if accumulate else ""),
                4 * M * N * (3 + 2 * (mul is not None) + bool(accumulate))):
        _check(lib().rp_layernorm_bwd(dy.data_ptr(), _rowmajor(dy, "dy"), dy_scale, x.data_ptr(), _rowmajor(x, "x"),
                                      stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(mul),
                                      _rowmajor(mul, "mul") if mul is not None else 0, dx.data_ptr(), _rowmajor(dx, "dx"),
                                      dx.shape[1], int(accumulate), _ptr(dmul), _rowmajor(dmul, "dmul") if dmul is not None else 0,
                                      dgamma.data_ptr(), dbeta.data_ptr(), M, N, ws.data_ptr(), nbytes, _stream()),
               "rp_layernorm_bwd")
    return dx, dmul, dgamma, dbeta


def gin_fits(F: int, P: int, O: int, D: int) -> bool:
    """do rp_gin_fwd / rp_gin_bwd cover a generalized interaction layer over F fields, P input and O output subspaces of
    width D?  (rp_gin_fits: D in {8, 16, 20, 32, 64}, F and P up to 64, O up to 16)"""
    return bool(lib().rp_gin_fits(F, P, O, D))


def _gin_dims(x0, bi, W, alpha, h, F: int, wide=()):
    """the checks that need no GPU (shapes, dtypes, contiguity, row widths), then the device check; -> P, O, D.
    wide: (name, tensor, columns) of the row buffers besides x0 and bi"""
    O, D = W.shape[0], W.shape[1]
    P = alpha.shape[0] // F
    if W.shape != (O, D, D) or alpha.shape != (P * F, O) or h.numel() != O * D:
        raise RuntimeError(f"gin: W {tuple(W.shape)} / alpha {tuple(alpha.shape)} / h {tuple(h.shape)} over {F} fields")
    _params((("gin: W", W), ("gin: alpha", alpha), ("gin: h", h)))
    _rows(x0, "gin: x0", F * D)
    bufs = (("bi", bi, P * D), *wide)
    for name, buf, cols in bufs:
        _rows(buf, "gin: " + name, cols, x0.shape[0])
    for name, t in (("x0", x0), ("W", W), ("alpha", alpha), ("h", h), *[(name, buf) for name, buf, _ in bufs]):
        _req(t, torch.float32, name)
    return P, O, D


def gin_fwd(x0, bi, W, alpha, h, F: int):
    """-> out [B, O D] of one generalized interaction layer (rp_gin_fwd): x0 [B, >= F D] and bi [B, >= P D] with any row
    strides, W [O, D, D], alpha [P F, O], h [O, D, 1]"""
    P, O, D = _gin_dims(x0, bi, W, alpha, h, F)
    B = x0.shape[0]
    out = _new((B, O * D), torch.float32, x0.device)
    with _Timed("gin_fwd", f"{B}x{F}.{P}.{O}.{D}", 4 * B * (F * D + P * D + O * D), 2 * B * O * P * D * (D + F + 1)):
        _check(lib().rp_gin_fwd(x0.data_ptr(), _rowmajor(x0, "x0"), bi.data_ptr(), _rowmajor(bi, "bi"), W.data_ptr(),
                                alpha.data_ptr(), h.data_ptr(), out.data_ptr(), O * D, F, P, O, D, B, _stream()), "rp_gin_fwd")
    return out


def gin_bwd(dout, x0, bi, W, alpha, h, F: int, dx0, accumulate: bool, bi_is_x0: bool = False):
    """-> (dbi, dW, dalpha, dh) of gin_fwd for the incoming dout [B, >= O D]; the gradient of x0 is written (accumulate: added)
    into the given dx0 [B, >= F D].  bi_is_x0 (layer 0: bi is the very tensor x0): bi's gradient joins dx0 and dbi is None."""
    P, O, D = _gin_dims(x0, bi, W, alpha, h, F, wide=[("dout", dout, W.shape[0] * W.shape[1]), ("dx0", dx0, F * W.shape[1])])
    B, dev = x0.shape[0], x0.device
    dbi = None if bi_is_x0 else _new((B, P * D), torch.float32, dev)
    dW, dalpha, dh = _new_like(W), _new_like(alpha), _new_like(h)
    ws, nbytes = _workspace("gin_bwd", F, P, O, D, device=dev)
    with _Timed("gin_bwd", f"{B}x{F}.{P}.{O}.{D}", 4 * B * (2 * F * D + 2 * P * D + O * D + bool(accumulate) * F * D),
                2 * B * O * P * D * (3 * D + 3 * F + 2)):
        _check(lib().rp_gin_bwd(dout.data_ptr(), _rowmajor(dout, "dout"), x0.data_ptr(), _rowmajor(x0, "x0"), bi.data_ptr(),
                                _rowmajor(bi, "bi"), W.data_ptr(), alpha.data_ptr(), h.data_ptr(), dx0.data_ptr(),
                                _rowmajor(dx0, "dx0"), int(accumulate), _ptr(dbi), P * D if dbi is not None else 0,
                                dW.data_ptr(), dalpha.data_ptr(), dh.data_ptr(), F, P, O, D, B, ws.data_ptr(), nbytes,
                                _stream()), "rp_gin_bwd")
    return dbi, dW, dalpha, dh


def _ccpm_ints(vals):
    return (C.c_int * max(len(vals), 1))(*[int(v) for v in vals])


def ccpm_fits(F: int, D: int, channels, heights, ks) -> bool:
    """do rp_ccpm_fwd / rp_ccpm_bwd cover a CCPM conv stack over F fields of width D with these output channels, kernel
    heights and pooling sizes per layer?  (rp_ccpm_fits: 1 to 3 layers, channels 1..4, heights 1..8, F <= 64, D <= 65536,
    every conv line L_out = L_in + kh - 1 <= 64 with 1 <= k <= L_out — L_out < k, where the reference's topk raises, is
    refused — and the working set of a wave within 144 KiB of LDS)"""
    n = len(channels)
    if n == 0 or len(heights) != n or len(ks) != n:
        return False
    return bool(lib().rp_ccpm_fits(int(F), int(D), n, _ccpm_ints(channels), _ccpm_ints(heights), _ccpm_ints(ks)))


def _ccpm_dims(x, weights, biases, F: int, D: int, ks, dout=None, dx=None):
    """the checks that need no GPU (shapes, dtypes, contiguity, widths, the range), then the device check; -> channels,
    heights.  dout: [B, >= C_last k_last D], dx: [B, >= F D] (the backward's row buffers)"""
    n = len(weights)
    if n == 0 or len(biases) != n or len(ks) != n:
        raise RuntimeError(f"ccpm: {n} weights / {len(biases)} biases / {len(ks)} pooling sizes")
    channels, heights, cin = [], [], 1
    for l, (w, b) in enumerate(zip(weights, biases)):
        if w.dim() not in (3, 4) or w.shape[1] != cin or (w.dim() == 4 and w.shape[3] != 1) or b.shape != (w.shape[0],):
            raise RuntimeError(f"ccpm: layer {l}: weight {tuple(w.shape)} / bias {tuple(b.shape)} over {cin} input channels "
                               "(need [C_out, C_in, kh, 1] and [C_out])")
        _params(((f"ccpm: layer {l} weight", w), (f"ccpm: layer {l} bias", b)))
        channels.append(w.shape[0])
        heights.append(w.shape[2])
        cin = w.shape[0]
    _rows(x, "ccpm: x", F * D)
    bufs = [(name, buf, cols) for name, buf, cols in (("dout", dout, channels[-1] * int(ks[-1]) * D), ("dx", dx, F * D))
            if buf is not None]
    for name, buf, cols in bufs:
        _rows(buf, "ccpm: " + name, cols, x.shape[0])
    lin = F
    for l, (kh, k) in enumerate(zip(heights, ks)):
        if lin + kh - 1 < k:
            raise RuntimeError(f"ccpm: layer {l}: L_out = {lin} + {kh} - 1 < k = {k} (topk would raise)")
        lin = k
    if not ccpm_fits(F, D, channels, heights, ks):
        raise RuntimeError(f"ccpm: F={F} D={D} channels={channels} heights={heights} ks={list(ks)}: outside rp_ccpm_fits")
    _req(x, torch.float32, "x")
    for t in list(weights) + list(biases):
        _req(t, torch.float32, "ccpm parameter")
    for name, buf, _ in bufs:
        _req(buf, torch.float32, name)
    return channels, heights


def _ccpm_cost(B, F, D, channels, heights, ks):
    """(bytes, flops) of the forward: x in, the last layer out; 2 flops per conv FMA"""
    lin, cin, fma = F, 1, 0
    for co, kh, k in zip(channels, heights, ks):
        fma += co * cin * kh * (lin + kh - 1)
        lin, cin = k, co
    return 4 * B * D * (F + channels[-1] * ks[-1]), 2 * B * D * fma


def ccpm_fwd(x, weights, biases, F: int, D: int, ks):
    """-> out [B, C_last k_last D] of the whole CCPM conv stack in one launch (rp_ccpm_fwd): x [B, >= F D] with any row
    stride, weights[l] [C_out, C_in, kh, 1], biases[l] [C_out], ks[l] the pooling size of layer l"""
    channels, heights = _ccpm_dims(x, weights, biases, F, D, ks)
    B, n = x.shape[0], len(weights)
    width = channels[-1] * int(ks[-1]) * D
    out = _new((B, width), torch.float32, x.device)
    nbytes, flops = _ccpm_cost(B, F, D, channels, heights, ks)
    with _Timed("ccpm_fwd", f"{B}x{F}.{D}", nbytes, flops):
        _check(lib().rp_ccpm_fwd(x.data_ptr(), _rowmajor(x, "x"), _ptr_array(weights), _ptr_array(biases), out.data_ptr(),
                                 width, F, D, n, _ccpm_ints(channels), _ccpm_ints(heights), _ccpm_ints(ks), B, _stream()),
               "rp_ccpm_fwd")
    return out


def ccpm_bwd(dout, x, weights, biases, F: int, D: int, ks, dx=None):
    """-> (dx, dWs, dbs) of ccpm_fwd for the incoming dout [B, >= C_last k_last D], rebuilt from x alone (rp_ccpm_bwd).  dx: a
    [B, >= F D] buffer to write the first F D columns of (the others are left alone); a fresh [B, F D] one otherwise."""
    channels, heights = _ccpm_dims(x, weights, biases, F, D, ks, dout=dout, dx=dx)
    B, n, dev = x.shape[0], len(weights), x.device
    if dx is None:
        dx = _new((B, F * D), torch.float32, dev)
    dWs, dbs = [_new_like(w) for w in weights], [_new_like(b) for b in biases]
    ws, wbytes = _workspace("ccpm_bwd", n, _ccpm_ints(channels), _ccpm_ints(heights), device=dev)
    nbytes, flops = _ccpm_cost(B, F, D, channels, heights, ks)
    with _Timed("ccpm_bwd", f"{B}x{F}.{D}", nbytes + 4 * B * D * 2 * F, 4 * flops):
        _check(lib().rp_ccpm_bwd(dout.data_ptr(), _rowmajor(dout, "dout"), x.data_ptr(), _rowmajor(x, "x"), _ptr_array(weights),
                                 _ptr_array(biases), dx.data_ptr(), _rowmajor(dx, "dx"), _ptr_array(dWs), _ptr_array(dbs), F, D,
                                 n, _ccpm_ints(channels), _ccpm_ints(heights), _ccpm_ints(ks), B, ws.data_ptr(), wbytes,
                                 _stream()), "rp_ccpm_bwd")
    return dx, dWs, dbs


BILINEAR_TYPES = {"field_" + t: _RP["RP_BILINEAR_" + t.upper()] for t in ("all", "each", "interaction")}
_BIL_TABLES: dict = {}
_BIL_WMAPS: dict = {}


def _bilinear_type(bilinear_type) -> int:
    """the RP_BILINEAR_* code of a type given by name or code; -1 for one the library does not know"""
    if isinstance(bilinear_type, str):
        return BILINEAR_TYPES.get(bilinear_type, -1)
    return int(bilinear_type) if int(bilinear_type) in BILINEAR_TYPES.values() else -1


def bilinear_fits(F: int, D: int, R: int, bilinear_type) -> bool:
    """do rp_bilinear_fwd / rp_bilinear_bwd cover F fields of width D with a SENET of R hidden units (0: none) and this weight
    sharing?  (rp_bilinear_fits: 2 <= F <= 40, D in {8, 16, 32, 64}, 0 <= R <= F, field_all / field_each / field_interaction)"""
    t = _bilinear_type(bilinear_type)
    return t >= 0 and bool(lib().rp_bilinear_fits(int(F), int(D), int(R), t))


def bilinear_weight_count(F: int, bilinear_type) -> int:
    t = _bilinear_type(bilinear_type)
    return {0: 1, 1: F, 2: F * (F - 1) // 2}[t]


def _bilinear_tables(weights, F: int, t: int, device):
    """(device array of the matrices' addresses, device array pair -> matrix), each built once: per address tuple (the
    parameters stay where they are from step to step, so a recorded step holds the array's address) / per (F, type)"""
    key = (F, t, str(device))
    wmap = _BIL_WMAPS.get(key)
    if wmap is None:
        pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]  # itertools.combinations order
        wmap = _BIL_WMAPS[key] = torch.tensor([0 if t == 0 else i if t == 1 else p for p, (i, _) in enumerate(pairs)],
                                              dtype=torch.int32, device=device)
    ptrs = (str(device),) + tuple([w.data_ptr() for w in weights])
    tab = _BIL_TABLES.get(ptrs)
    if tab is None:
        if len(_BIL_TABLES) >= 4096:  # (a few KB each; a recorded step replays with its array's address, so they are kept)
            _BIL_TABLES.clear()
        tab = _BIL_TABLES[ptrs] = torch.tensor(list(ptrs[1:]), dtype=torch.int64, device=device)
    return tab, wmap


def _bilinear_dims(x, F: int, D: int, weights, bilinear_type, senet, n_dense: int, wide=(), dx=None):
    """the checks that need no GPU (dtypes, contiguity, shapes, row widths, the range), then the device check; -> (type
    code, R, P, columns of the output).  wide: (name, tensor) pairs that must hold [B, >= width]; dx: [B, >= F D]"""
    t = _bilinear_type(bilinear_type)
    if t < 0:
        raise RuntimeError(f"bilinear: unknown bilinear_type {bilinear_type!r}")
    R = 0 if senet is None else int(senet[0].shape[0])
    params = list(weights) + ([] if senet is None else list(senet))
    _params((f"bilinear: parameter {k}", w) for k, w in enumerate(params))
    _rows(x, "bilinear: x", F * D + n_dense)
    if F < 2 or len(weights) != bilinear_weight_count(F, t) or any(tuple(w.shape) != (D, D) for w in weights):
        raise RuntimeError(f"bilinear: {len(weights)} matrices for F = {F}, D = {D}, type {bilinear_type!r} "
                           "(need 1 / F / F (F - 1) / 2 of shape [D, D])")
    if senet is not None and (tuple(senet[0].shape) != (R, F) or tuple(senet[1].shape) != (F, R)):
        raise RuntimeError(f"bilinear: SENET weights {tuple(senet[0].shape)} / {tuple(senet[1].shape)} for F = {F} "
                           "(need [R, F] and [F, R])")
    if not bilinear_fits(F, D, R, t):
        raise RuntimeError(f"bilinear: F={F} D={D} R={R} type={bilinear_type!r}: outside rp_bilinear_fits")
    P = F * (F - 1) // 2
    width = (2 if R else 1) * P * D + n_dense
    for name, buf, cols in [(n, b, width) for n, b in wide] + ([("dx", dx, F * D)] if dx is not None else []):
        _rows(buf, "bilinear: " + name, cols, x.shape[0])
    _req(x, torch.float32, "x")
    for w in params:
        _req(w, torch.float32, "bilinear parameter")
    for name, buf in list(wide) + ([("dx", dx)] if dx is not None else []):
        _req(buf, torch.float32, name)
    return t, R, P, width


def bilinear_fwd(x, F: int, D: int, weights, bilinear_type, senet=None, n_dense: int = 0, out=None):
    """-> out [B, P D | P D | n_dense]: the bilinear products of the field pairs, the same scaled by A_i A_j of the SENET
    (senet = (W1 [R, F], W2 [F, R]); None: that branch is absent), and the dense columns, in one launch (rp_bilinear_fwd).
    x [B, >= F D + n_dense] with any row stride, weights: the [D, D] matrices (1 / F / P of them for field_all / field_each /
    field_interaction).  out: a [B, >= width] buffer whose first `width` columns are written."""
    t, R, P, width = _bilinear_dims(x, F, D, weights, bilinear_type, senet, n_dense,
                                    wide=[("out", out)] if out is not None else [])
    B, dev = x.shape[0], x.device
    if out is None:
        out = _new((B, width), torch.float32, dev)
    tab, wmap = _bilinear_tables(weights, F, t, dev)
    w1, w2 = (None, None) if senet is None else senet
    with _Timed("bilinear_fwd", f"{B}x{F}.{D}.{R}", 4 * (B * (F * D + 2 * n_dense + width - n_dense) + len(weights) * D * D),
                B * P * D * (2 * D + (3 if R else 1))):
        _check(lib().rp_bilinear_fwd(x.data_ptr(), _rowmajor(x, "x"), _ptr(w1), _ptr(w2), tab.data_ptr(), wmap.data_ptr(),
                                     out.data_ptr(), _rowmajor(out, "out"), F, D, R, t, n_dense, B, _stream()),
               "rp_bilinear_fwd")
    return out


def bilinear_bwd(dout, x, F: int, D: int, weights, bilinear_type, senet=None, n_dense: int = 0, dx=None,
                 accumulate: bool = False):
    """-> (dx, dW [NW, D, D], dW1, dW2) of bilinear_fwd for the incoming dout [B, >= width], rebuilt from x alone
    (rp_bilinear_bwd).  dx: a [B, >= F D] buffer whose first F D columns are written, or added to with accumulate (the others
    are left alone); a fresh [B, F D] one otherwise.  dW1 / dW2 are None without a SENET."""
    if dx is None and accumulate:
        raise RuntimeError("bilinear_bwd: accumulate needs the dx buffer to add to")
    t, R, P, width = _bilinear_dims(x, F, D, weights, bilinear_type, senet, n_dense, wide=[("dout", dout)], dx=dx)
    B, dev = x.shape[0], x.device
    if dx is None:
        dx = _new((B, F * D), torch.float32, dev)
    dW = _new((len(weights), D, D), torch.float32, dev)
    dW1, dW2 = (None, None) if senet is None else (_new_like(senet[0]), _new_like(senet[1]))
    tab, wmap = _bilinear_tables(weights, F, t, dev)
    w1, w2 = (None, None) if senet is None else senet
    ws, wbytes = _workspace("bilinear_bwd", F, D, R, t, device=dev)
    with _Timed("bilinear_bwd", f"{B}x{F}.{D}.{R}", 4 * (B * (2 * F * D + width - n_dense) + 2 * len(weights) * D * D),
                B * P * D * (6 * D + (8 if R else 3))):
        _check(lib().rp_bilinear_bwd(dout.data_ptr(), _rowmajor(dout, "dout"), x.data_ptr(), _rowmajor(x, "x"), _ptr(w1),
                                     _ptr(w2), tab.data_ptr(), wmap.data_ptr(), dx.data_ptr(), _rowmajor(dx, "dx"),
                                     int(bool(accumulate)), dW.data_ptr(), _ptr(dW1), _ptr(dW2), F, D, R, t, n_dense, B,
                                     ws.data_ptr(), wbytes, _stream()), "rp_bilinear_bwd")
    return dx, dW, dW1, dW2


def lognet_fits(F: int, D: int, L: int) -> bool:
    """do rp_lognet_fwd / rp_lognet_bwd cover F fields of width D and L logarithmic neurons?  (rp_lognet_fits: 1 <= F <= 64,
    1 <= D <= 256, 1 <= L <= 8 — the shapes whose kernels compile without scratch)"""
    return bool(lib().rp_lognet_fits(int(F), int(D), int(L)))


def lognet_plan(B: int, D: int):
    """-> (partial workgroups of every reduction of rp_lognet_* over the B D (sample, column) pairs, pairs per workgroup)"""
    nblk, chunk = C.c_int(0), _i64(0)
    _check(lib().rp_lognet_plan(int(B), int(D), C.byref(nblk), C.byref(chunk)), "rp_lognet_plan")
    return nblk.value, chunk.value


def _lognet_dims(x, F: int, D: int, W, vecs1, vecs2, wide=()):
    """the checks rp_lognet_fwd / rp_lognet_bwd share (shapes and types first, the device last) -> L"""
    if W.dim() != 2 or W.shape[1] != F or not W.is_contiguous():
        raise RuntimeError(f"lognet: W {tuple(W.shape)} for F = {F}: expected a contiguous [L, F]")
    L = W.shape[0]
    _params([("lognet: W", W)] + [("lognet: a BatchNorm vector", v) for v in (*vecs1, *vecs2)])
    _rows(x, "lognet: x", F * D)
    for n, vecs in ((F, vecs1), (L, vecs2)):
        for v in vecs:
            if v.numel() != n:
                raise RuntimeError(f"lognet: a BatchNorm vector of {v.numel()} elements, expected {n}")
    for name, buf, cols in wide:
        _rows(buf, "lognet: " + name, cols, x.shape[0])
    if not lognet_fits(F, D, L):
        raise RuntimeError(f"lognet: F={F} D={D} L={L}: outside rp_lognet_fits")
    for t in (x, W, *vecs1, *vecs2, *[buf for _, buf, _ in wide]):
        _req(t, torch.float32, "lognet")
    return L


def lognet_fwd(x, F: int, D: int, W, gamma1, beta1, mean1, var1, eps1: float, gamma2, beta2, mean2, var2, eps2: float,
               train: bool, out):
    """AFN's logarithmic net on the rows x [B, >= F D] (read in place): out[:, :L D] = BN2(exp(W BN1(log max(|x|, 1e-5)))) and
    z [B, L D] (for the backward).  train: mean1 / var1 [F] and mean2 / var2 [L] are WRITTEN with the batch statistics
    (biased variances); otherwise they are read.  rp_lognet_fwd: 5 launches with batch statistics, 1 without."""
    L = _lognet_dims(x, F, D, W, (gamma1, beta1, mean1, var1), (gamma2, beta2, mean2, var2), wide=[("out", out, W.shape[0] * D)])
    B, dev = x.shape[0], x.device
    z = _new((B, L * D), torch.float32, dev)
    ws, wbytes = _workspace("lognet", F, L, device=dev)
    with _Timed("lognet_fwd", f"{B}x{F}.{D}.{L}", 4 * B * (F * D + L * D)):
        _check(lib().rp_lognet_fwd(x.data_ptr(), _rowmajor(x, "x"), W.data_ptr(), gamma1.data_ptr(), beta1.data_ptr(),
                                   mean1.data_ptr(), var1.data_ptr(), eps1, gamma2.data_ptr(), beta2.data_ptr(), mean2.data_ptr(),
                                   var2.data_ptr(), eps2, z.data_ptr(), out.data_ptr(), _rowmajor(out, "out"), B, F, D, L,
                                   int(train), ws.data_ptr(), wbytes, _stream()), "rp_lognet_fwd")
    return out, z


def lognet_bwd(dout, x, z, F: int, D: int, W, gamma1, beta1, mean1, var1, eps1: float, gamma2, mean2, var2, eps2: float,
               train: bool, dx=None):
    """-> (dx, dW [L, F], dgamma1, dbeta1 [F], dgamma2, dbeta2 [L]) of lognet_fwd with the statistics it used (rp_lognet_bwd).
    dx: a [B, >= F D] buffer whose first F D columns are written (the others are the caller's)."""
    L = _lognet_dims(x, F, D, W, (gamma1, beta1, mean1, var1), (gamma2, mean2, var2),
                     wide=[("dout", dout, W.shape[0] * D)] + ([("dx", dx, F * D)] if dx is not None else []))
    B, dev = x.shape[0], x.device
    if z.shape != (B, L * D) or not z.is_contiguous():
        raise RuntimeError(f"lognet_bwd: z {tuple(z.shape)} for B = {B}, L D = {L * D}")
    if dx is None:
        dx = _new((B, F * D), torch.float32, dev)
    dW = _new((L, F), torch.float32, dev)
    dg1, db1 = _new((F,), torch.float32, dev), _new((F,), torch.float32, dev)
    dg2, db2 = _new((L,), torch.float32, dev), _new((L,), torch.float32, dev)
    ws, wbytes = _workspace("lognet", F, L, device=dev)
    with _Timed("lognet_bwd", f"{B}x{F}.{D}.{L}", 4 * B * (2 * F * D + 2 * L * D)):
        _check(lib().rp_lognet_bwd(dout.data_ptr(), _rowmajor(dout, "dout"), x.data_ptr(), _rowmajor(x, "x"), z.data_ptr(),
                                   W.data_ptr(), gamma1.data_ptr(), beta1.data_ptr(), mean1.data_ptr(), var1.data_ptr(), eps1,
                                   gamma2.data_ptr(), mean2.data_ptr(), var2.data_ptr(), eps2, dx.data_ptr(), _rowmajor(dx, "dx"),
                                   dW.data_ptr(), dg1.data_ptr(), db1.data_ptr(), dg2.data_ptr(), db2.data_ptr(), B, F, D, L,
                                   int(train), ws.data_ptr(), wbytes, _stream()), "rp_lognet_bwd")
    return dx, dW, dg1, db1, dg2, db2


def pair_fc_fwd(a, d, w, bias):
    """z [B, 1] = w[0, 0] a + w[0, 1] d + bias: nn.Linear(2, 1) over cat[a, d] without the cat (rp_pair_fc_fwd)"""
    B = _pair_vectors((a, d), ("a", "d"))
    _req(w, torch.float32, "pair_fc: weight")
    _req(bias, torch.float32, "pair_fc: bias")
    if w.numel() != 2 or bias.numel() != 1 or not w.is_contiguous():
        raise RuntimeError(f"pair_fc: weight {tuple(w.shape)} / bias {tuple(bias.shape)}: expected a Linear(2, 1)")
    z = _new((B, 1), torch.float32, a.device)
    with _Timed("pair_fc_fwd"):
        _check(lib().rp_pair_fc_fwd(a.data_ptr(), d.data_ptr(), w.data_ptr(), bias.data_ptr(), z.data_ptr(), B, _stream()),
               "rp_pair_fc_fwd")
    return z


def pair_fc_bwd(dz, a, d, w):
    """-> (da [B, 1], dd [B, 1], dw [1, 2], dbias [1]) of pair_fc_fwd (rp_pair_fc_bwd: deterministic two-stage sums)"""
    B = _pair_vectors((dz, a, d), ("dz", "a", "d"))
    dev = a.device
    da, dd = _new((B, 1), torch.float32, dev), _new((B, 1), torch.float32, dev)
    dw, db = _new((1, 2), torch.float32, dev), _new((1,), torch.float32, dev)
    partial = _new((lib().rp_pair_fc_partials(B),), torch.float32, dev)
    with _Timed("pair_fc_bwd"):
        _check(lib().rp_pair_fc_bwd(dz.data_ptr(), a.data_ptr(), d.data_ptr(), w.data_ptr(), da.data_ptr(), dd.data_ptr(),
                                    dw.data_ptr(), db.data_ptr(), partial.data_ptr(), B, _stream()), "rp_pair_fc_bwd")
    return da, dd, dw, db


def dice_gate_fwd(x, xhat, alpha):
    """y = x * (alpha + sigmoid(xhat) * (1 - alpha))  (rp_dice_gate_fwd)"""
    _req(x, torch.float32, "x")
    _req(xhat, torch.float32, "xhat")
    _req(alpha, torch.float32, "alpha")
    M, N = x.shape
    y = _new((M, N), torch.float32, x.device)
    with _Timed("dice_gate_fwd", f"{M}x{N}", 12 * M * N):
        _check(lib().rp_dice_gate_fwd(x.data_ptr(), _rowmajor(x, "x"), xhat.data_ptr(), _rowmajor(xhat, "xhat"),
                                      alpha.data_ptr(), y.data_ptr(), N, M, N, _stream()), "rp_dice_gate_fwd")
    return y


def dice_gate_bwd(x, xhat, alpha, dy):
    """-> (dx_direct, dxhat, dal) packed [M, N] each (rp_dice_gate_bwd); dalpha = column sums of dal"""
    M, N = x.shape
    dxd, dxh, dal = (_new((M, N), torch.float32, x.device) for _ in range(3))
    with _Timed("dice_gate_bwd", f"{M}x{N}", 24 * M * N):
        _check(lib().rp_dice_gate_bwd(x.data_ptr(), _rowmajor(x, "x"), xhat.data_ptr(), _rowmajor(xhat, "xhat"),
                                      alpha.data_ptr(), dy.data_ptr(), _rowmajor(dy, "dy"), dxd.data_ptr(), dxh.data_ptr(),
                                      dal.data_ptr(), M, N, _stream()), "rp_dice_gate_bwd")
    return dxd, dxh, dal


def batchnorm_apply_bwd(dy, rstd, gamma):
    M, N = dy.shape
    dx = _new((M, N), torch.float32, dy.device)
    with _Timed("batchnorm_apply_bwd", f"{M}x{N}", 8 * M * N):
        _check(lib().rp_batchnorm_apply_bwd(dy.data_ptr(), _rowmajor(dy, "dy"), rstd.data_ptr(), _ptr(gamma),
                                            dx.data_ptr(), N, M, N, _stream()), "rp_batchnorm_apply_bwd")
    return dx


def sigmoid_bce_fwd(addends: Sequence[torch.Tensor], label: Optional[torch.Tensor], apply_sigmoid: bool = True,
                    p_eps: float = 0.0, weight: float = 1.0, add_to: Optional[torch.Tensor] = None):
    B = addends[0].numel()
    for z in addends:
        _req(z, torch.float32, "logit")
        if z.numel() != B or not z.is_contiguous():
            raise RuntimeError("logit addends must be contiguous with B elements")
    dev = addends[0].device
    pred = _new((B, 1), torch.float32, dev)
    loss = partial = None
    if label is not None:
        _req(label, torch.float32, "label")
        if label.numel() != B or not label.is_contiguous():
            raise RuntimeError("label must be contiguous float32 with B elements")
        partial = _new((lib().rp_loss_partials(B),), torch.float32, dev)
        loss = _new((), torch.float32, dev) if add_to is None else add_to
    elif add_to is not None:
        raise RuntimeError("sigmoid_bce_fwd: add_to needs a label")
    with _Timed("sigmoid_bce_fwd"):
        # add_to: the loss scalar of the tasks before this one (a multi-task loss): this launch ADDS its weighted mean
        fn = lib().rp_sigmoid_bce_fwd if add_to is None else lib().rp_sigmoid_bce_fwd_accum
        _check(fn(_ptr_array(addends), len(addends), int(apply_sigmoid), _ptr(label), B, p_eps, weight, pred.data_ptr(),
                  _ptr(partial), _ptr(loss), _stream()), "rp_sigmoid_bce_fwd")
    return pred, loss


def sigmoid_bce_bwd(pred, label, gloss, apply_sigmoid: bool = True, p_eps: float = 0.0, weight: float = 1.0):
    B = pred.numel()
    dz = _new((B, 1), torch.float32, pred.device)
    gloss = gloss.reshape(1).contiguous()
    with _Timed("sigmoid_bce_bwd"):
        _check(lib().rp_sigmoid_bce_bwd(pred.data_ptr(), label.data_ptr(), gloss.data_ptr(), B, p_eps, weight,
                                    int(apply_sigmoid), dz.data_ptr(), _stream()), "rp_sigmoid_bce_bwd")
    return dz


PAIR_ESSM, PAIR_AITM = _RP["RP_PAIR_ESSM"], _RP["RP_PAIR_AITM"]


def _pair_vectors(tensors, names):
    B = tensors[0].numel()
    for t, name in zip(tensors, names):
        _req(t, torch.float32, name)
        if t.numel() != B or not t.is_contiguous():
            raise RuntimeError(f"pair_loss: {name} must be contiguous with B = {B} elements")
    if B < 1:
        raise RuntimeError("pair_loss: empty batch")
    return B


def pair_loss_fwd(z1, z2, y1, y2, mode: int, coef: float, apply_sigmoid: bool = True):
    """-> (p1 [B], p2 [B], loss []): RP_PAIR_ESSM BCE(p1 p2, y2) + coef BCE(p1, y1); RP_PAIR_AITM BCE(p1, y1) + BCE(p2, y2) +
    coef sum_b max(p2 - p1, 0), with p = sigmoid(z) or z itself"""
    B = _pair_vectors((z1, z2, y1, y2), ("z1", "z2", "y1", "y2"))
    dev = z1.device
    p1, p2 = _new((B,), torch.float32, dev), _new((B,), torch.float32, dev)
    partial = _new((3 * lib().rp_loss_partials(B),), torch.float32, dev)
    loss = _new((), torch.float32, dev)
    with _Timed("pair_loss_fwd"):
        _check(lib().rp_pair_loss_fwd(z1.data_ptr(), z2.data_ptr(), y1.data_ptr(), y2.data_ptr(), B, mode, coef,
                                      int(apply_sigmoid), p1.data_ptr(), p2.data_ptr(), partial.data_ptr(), loss.data_ptr(),
                                      _stream()), "rp_pair_loss_fwd")
    return p1, p2, loss


def pair_loss_bwd(p1, p2, y1, y2, gloss, mode: int, coef: float, apply_sigmoid: bool = True):
    B = _pair_vectors((p1, p2, y1, y2), ("p1", "p2", "y1", "y2"))
    dz1, dz2 = _new((B,), torch.float32, p1.device), _new((B,), torch.float32, p1.device)
    gloss = gloss.reshape(1).contiguous()
    with _Timed("pair_loss_bwd"):
        _check(lib().rp_pair_loss_bwd(p1.data_ptr(), p2.data_ptr(), y1.data_ptr(), y2.data_ptr(), gloss.data_ptr(), B, mode,
                                      coef, int(apply_sigmoid), dz1.data_ptr(), dz2.data_ptr(), _stream()), "rp_pair_loss_bwd")
    return dz1, dz2


_weight_epoch = 0


def weight_epoch() -> int:
    """bumped by every optimizer launch of this module: parameters change through raw pointers there, which torch's
    tensor version counters do not see (caches of derived weight layouts key on this)"""
    return _weight_epoch


def bump_weight_epoch() -> None:
    """a captured step was replayed: its optimizer kernels ran without any python"""
    global _weight_epoch
    _weight_epoch += 1


def counters_add(counters, delta: int = 1):
    """*c += delta for every device counter in `counters` (1..8 int32[1] tensors) in ONE launch (rp_counters_add)"""
    if len(counters) == 1:
        return counter_add(counters[0], delta)
    _check(lib().rp_counters_add(_ptr_array(counters), len(counters), delta, _stream()), "rp_counters_add")


def counter_add(counter, delta: int = 1):
    """*counter += delta on the current stream (device-resident step counters, see rp_counter_add)"""
    _check(lib().rp_counter_add(counter.data_ptr(), delta, _stream()), "rp_counter_add")


def adam_step(params, grads, ms, vs, lr, beta1, beta2, eps, step: int, zero_grad: bool, scalars=None, t_dev=None):
    """One fused launch per <=64 tensors; tensors must be contiguous fp32 on the same device.  t_dev (device int32[1],
    completed steps) + scalars (the per-step float2 table): the step number is read on the device (hipGraph replays)."""
    global _weight_epoch
    _weight_epoch += 1
    for i in range(0, len(params), MAX_FIELDS):
        ps, gs = params[i:i + MAX_FIELDS], grads[i:i + MAX_FIELDS]
        mm, vv = ms[i:i + MAX_FIELDS], vs[i:i + MAX_FIELDS]
        for t in (*ps, *gs, *mm, *vv):
            _req(t, torch.float32, "adam tensor")
            if not t.is_contiguous():
                raise RuntimeError("adam tensors must be contiguous")
        sizes = (C.c_int64 * len(ps))(*[p.numel() for p in ps])
        with _Timed("adam_step"):
            _check(lib().rp_adam_step(_ptr_array(ps), _ptr_array(gs), _ptr_array(mm), _ptr_array(vv), sizes, len(ps), lr,
                                  beta1, beta2, eps, step, int(zero_grad), _ptr(scalars), _ptr(t_dev), _stream()),
                   "rp_adam_step")


# ---- exact lazy dense Adam (arena rows) ---------------------------------------------------------------
def embed_keys(row_base, row_count, idx: List[torch.Tensor], err_flag, out=None):
    F, B = len(idx), idx[0].shape[0]
    keys = out if out is not None else _new((F * B,), torch.int32, idx[0].device)
    assert keys.numel() == F * B and keys.dtype == torch.int32
    with _Timed("embed_keys"):
        _check(lib().rp_embed_keys(row_base.data_ptr(), row_count.data_ptr(), _ptr_array(idx), F, B, keys.data_ptr(),
                                   err_flag.data_ptr(), _stream()), "rp_embed_keys")
    return keys


def shard_keys(row_base, row_count, idx: List[torch.Tensor], world: int, lbits: int, err_flag):
    """composite (owner << lbits | local row) int32 keys of a batch's row requests, p = f*B + b (rp_shard_keys)."""
    F, B = len(idx), idx[0].shape[0]
    keys = _new((F * B,), torch.int32, idx[0].device)
    with _Timed("shard_keys"):
        _check(lib().rp_shard_keys(row_base.data_ptr(), row_count.data_ptr(), _ptr_array(idx), F, B, world, lbits,
                                   keys.data_ptr(), err_flag.data_ptr(), _stream()), "rp_shard_keys")
    return keys


def route_build(sorted_keys, sorted_pos, world: int, lbits: int, out=None):
    """-> (slot_sorted int32 [n], slot_of_pair int64 [n], uniq_rows int64 [n] (first counts[world] valid),
    counts int64 [world+1]) from the sorted composite keys (rp_route_build).  out = (slot_sorted, slot_of_pair): persistent
    buffers to write into (the prepared lookup of a recorded step's static batch)"""
    n = sorted_keys.numel()
    dev = sorted_keys.device
    if out is not None:
        slot_sorted, slot_of_pair = out
        assert slot_sorted.shape == (n,) and slot_sorted.dtype == torch.int32 and slot_of_pair.shape == (n,) \
            and slot_of_pair.dtype == torch.int64
    else:
        slot_sorted = _new((n,), torch.int32, dev)
        slot_of_pair = _new((n,), torch.int64, dev)
    uniq_rows = _new((n,), torch.int64, dev)
    counts = _new((world + 1,), torch.int64, dev)
    ws, nbytes = _workspace("route", n, world, device=dev)
    with _Timed("route_build"):
        _check(lib().rp_route_build(ws.data_ptr(), nbytes, sorted_keys.data_ptr(), sorted_pos.data_ptr(), n, world,
                                    lbits, slot_sorted.data_ptr(), slot_of_pair.data_ptr(), uniq_rows.data_ptr(),
                                    counts.data_ptr(), _stream()), "rp_route_build")
    return slot_sorted, slot_of_pair, uniq_rows, counts


def route_pad(sorted_keys, sorted_pos, world: int, lbits: int, capacity: int, counts, slot_sorted, slot_of_pair, err_flag,
              out=None):
    """fixed-capacity form of a route (rp_route_pad): slot_sorted / slot_of_pair are rewritten in place / overwritten;
    -> rows_padded int64 [world * capacity] (local rows to ask each owner for, unused slots 0); out: a persistent buffer for it"""
    if out is not None:
        assert out.shape == (world * capacity,) and out.dtype == torch.int64
        rows_padded = out
        _check(lib().rp_fill_words(rows_padded.data_ptr(), rows_padded.numel() * 2, 0, _stream()), "rp_fill_words")
    else:
        rows_padded = zeros((world * capacity,), torch.int64, sorted_keys.device)
    with _Timed("route_pad"):
        _check(lib().rp_route_pad(sorted_keys.data_ptr(), sorted_pos.data_ptr(), sorted_keys.numel(), world, lbits, capacity,
                                  counts.data_ptr(), slot_sorted.data_ptr(), slot_of_pair.data_ptr(),
                                  rows_padded.data_ptr(), err_flag.data_ptr(), _stream()), "rp_route_pad")
    return rows_padded


def route_field_major(sorted_keys, sorted_pos, slot_sorted, B: int, world: int, lbits: int, out=None):
    """-> (slot_fm, pos_fm): the route's sorted (slot, position) list moved into FIELD-major order (rp_route_field_major) —
    what rp_embed_grad_seg takes as its sorted pair list when the rows came from more than one owner"""
    n = sorted_keys.numel()
    dev = sorted_keys.device
    if out is not None:
        slot_fm, pos_fm = out
        assert slot_fm.shape == (n,) and pos_fm.shape == (n,) and slot_fm.dtype == pos_fm.dtype == torch.int32
    else:
        slot_fm = _new((n,), torch.int32, dev)
        pos_fm = _new((n,), torch.int32, dev)
    delta = _new((world * (n // B),), torch.int64, dev)
    with _Timed("route_field_major"):
        _check(lib().rp_route_field_major(sorted_keys.data_ptr(), sorted_pos.data_ptr(), slot_sorted.data_ptr(), n, B, world, lbits,
                                          slot_fm.data_ptr(), pos_fm.data_ptr(), delta.data_ptr(), _stream()),
               "rp_route_field_major")
    return slot_fm, pos_fm


def batchnorm_update_running(mean, var, bn, M: int):
    """bn.running_mean / running_var / num_batches_tracked after one training forward over M rows (rp_batchnorm_update_running)"""
    for t in (mean, var, bn.running_mean, bn.running_var):
        _req(t, torch.float32, "statistics")
    nbt = bn.num_batches_tracked
    if nbt is not None and (nbt.dtype is not torch.int64 or not nbt.is_cuda):
        raise RuntimeError("batchnorm_update_running: num_batches_tracked must be an int64 device tensor")
    _check(lib().rp_batchnorm_update_running(mean.data_ptr(), var.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                             _ptr(nbt), -1.0 if bn.momentum is None else float(bn.momentum), M, mean.numel(),
                                             _stream()), "rp_batchnorm_update_running")


def batchnorm_colsum(x, center=None):
    """column sums of x, or of (x - center)^2 (rp_batchnorm_colsum) -> [N]"""
    _req(x, torch.float32, "x")
    M, N = x.shape
    out = _new((N,), torch.float32, x.device)
    ws, nb = _workspace("batchnorm", M, N, device=x.device)
    with _Timed("batchnorm_colsum", f"{M}x{N}", 4 * M * N):
        _check(lib().rp_batchnorm_colsum(x.data_ptr(), _rowmajor(x, "x"), _ptr(center), out.data_ptr(), M, N, ws.data_ptr(),
                                         nb, _stream()), "rp_batchnorm_colsum")
    return out


def batchnorm_bwd_sums(x, dy, mean, rstd):
    """-> (dgamma [N] = sum dy * xhat, dbeta [N] = sum dy) over the local rows (rp_batchnorm_bwd_sums)"""
    M, N = x.shape
    dgamma, dbeta = (_new((N,), torch.float32, x.device) for _ in range(2))
    ws, nb = _workspace("batchnorm", M, N, device=x.device)
    with _Timed("batchnorm_bwd_sums", f"{M}x{N}", 8 * M * N):
        _check(lib().rp_batchnorm_bwd_sums(x.data_ptr(), _rowmajor(x, "x"), dy.data_ptr(), _rowmajor(dy, "dy"),
                                           mean.data_ptr(), rstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), M, N,
                                           ws.data_ptr(), nb, _stream()), "rp_batchnorm_bwd_sums")
    return dgamma, dbeta


def batchnorm_bwd_apply(x, dy, mean, rstd, gamma, mean_dy, mean_dyx):
    M, N = x.shape
    dx = _new((M, N), torch.float32, x.device)
    with _Timed("batchnorm_bwd_apply", f"{M}x{N}", 12 * M * N):
        _check(lib().rp_batchnorm_bwd_apply(x.data_ptr(), _rowmajor(x, "x"), dy.data_ptr(), _rowmajor(dy, "dy"),
                                            mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), mean_dy.data_ptr(),
                                            mean_dyx.data_ptr(), dx.data_ptr(), N, M, N, _stream()),
               "rp_batchnorm_bwd_apply")
    return dx


def mlp_tail_fits(n_hidden: int, width: int, hin) -> bool:
    return bool(lib().rp_mlp_tail_fits(n_hidden, width, _rowmajor(hin, "hin"))) and hin.data_ptr() % 16 == 0


def _i64_array(vals):
    return (C.c_int64 * max(len(vals), 1))(*vals)


def _opt_ptr_array(tensors):
    arr = (C.c_void_p * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else _ptr(t)
    return arr


def mlp_tail_fwd(hin, Ws, bs, w_out, b_out):
    """hin [M,64] -> (logit [M,1], hidden outputs [M,64] x len(Ws)) in one launch (rp_mlp_tail_fwd)."""
    _req(hin, torch.float32, "hin")
    M, L = hin.shape[0], len(Ws)
    hs = [_new((M, 64), torch.float32, hin.device) for _ in range(L)]
    logit = _new((M, 1), torch.float32, hin.device)
    with _Timed("mlp_tail_fwd", f"{M}x64x{L}", 4 * M * (64 * (L + 1) + 1), 2 * M * (64 * 64 * L + 64)):
        _check(lib().rp_mlp_tail_fwd(hin.data_ptr(), _rowmajor(hin, "hin"), L, _ptr_array(Ws), _i64_array([_rowmajor(w, "W") for w in Ws]),
                                     _opt_ptr_array(bs), _ptr_array(hs), w_out.data_ptr(), _ptr(b_out), logit.data_ptr(), M,
                                     _stream()), "rp_mlp_tail_fwd")
    return logit, hs


def mlp_tail_fwd_bce(hin, Ws, bs, w_out, b_out, addends, label, p_eps: float = 0.0, weight: float = 1.0):
    """the tail's forward with the loss head inside (rp_mlp_tail_fwd_bce): -> (pred [M,1], loss [] , hidden outputs).
    The scalar is the only thing the partial sums are for and nobody on the device reads it: inside a recorded launch plan
    rp_loss_finish is issued on the plan's inline side section (deferred behind the next launches recorded there)."""
    _req(hin, torch.float32, "hin")
    _req(label, torch.float32, "label")
    M, L = hin.shape[0], len(Ws)
    dev = hin.device
    hs = [_new((M, 64), torch.float32, dev) for _ in range(L)]
    pred = _new((M, 1), torch.float32, dev)
    n_part = lib().rp_mlp_tail_loss_partials(M)
    partial = _new((n_part,), torch.float32, dev)
    loss = _new((), torch.float32, dev)
    for t in addends:
        _req(t, torch.float32, "addend")
        if t.numel() != M or not t.is_contiguous():
            raise RuntimeError("mlp_tail_fwd_bce: every addend is a contiguous [M] / [M, 1] logit")
    if label.numel() != M or not label.is_contiguous():
        raise RuntimeError("mlp_tail_fwd_bce: label must be a contiguous [M]")
    with _Timed("mlp_tail_fwd", f"{M}x64x{L}+bce", 4 * M * (64 * (L + 1) + 3), 2 * M * (64 * 64 * L + 64)):
        _check(lib().rp_mlp_tail_fwd_bce(hin.data_ptr(), _rowmajor(hin, "hin"), L, _ptr_array(Ws),
                                         _i64_array([_rowmajor(w, "W") for w in Ws]), _opt_ptr_array(bs), _ptr_array(hs),
                                         w_out.data_ptr(), _ptr(b_out), _ptr_array(addends) if addends else None, len(addends),
                                         label.data_ptr(), p_eps, pred.data_ptr(), partial.data_ptr(), M, _stream()),
               "rp_mlp_tail_fwd_bce")

    def finish():
        _check(lib().rp_loss_finish(partial.data_ptr(), n_part, weight / M, loss.data_ptr(), _stream()), "rp_loss_finish")

    if LaunchPlan.is_recording():
        LaunchPlan.defer_side(finish)
    else:
        finish()
    return pred, loss, hs


def mlp_tail_bwd(dz, Ws, acts, w_out, bce=None):
    """-> (dhin [M,64] masked by hin > 0, [dW_l], [db_l], dw_out [1,64], db_out [1]) (rp_mlp_tail_bwd).
    bce = (pred, label, gloss, p_eps, weight, dz_out): the loss head's backward inside the launch (rp_mlp_tail_bwd_bce) —
    `dz` is then None and the logit's gradient is written to dz_out [M] for the other logit addends."""
    M, L = (dz.shape[0] if bce is None else bce[0].shape[0]), len(Ws)
    dev = dz.device if bce is None else bce[0].device
    dhin = _new((M, 64), torch.float32, dev)
    grads = _new((L * 4096 + L * 64 + 65,), torch.float32, dev)
    ws, nbytes = _workspace("mlp_tail_bwd", M, L, device=dev)
    def launch(parts):
        if bce is not None:
            pred, label, gloss, p_eps, weight, dz_out = bce
            _check(lib().rp_mlp_tail_bwd_bce(pred.data_ptr(), label.data_ptr(), gloss.data_ptr(), p_eps, weight, _ptr(dz_out), L,
                                             _ptr_array(Ws), _i64_array([_rowmajor(w, "W") for w in Ws]), _ptr_array(acts),
                                             _rowmajor(acts[0], "hin"), w_out.data_ptr(), dhin.data_ptr(), 64, grads.data_ptr(),
                                             M, ws.data_ptr(), nbytes, parts, _stream()), "rp_mlp_tail_bwd_bce")
            return
        _check(lib().rp_mlp_tail_bwd_parts(dz.data_ptr(), L, _ptr_array(Ws), _i64_array([_rowmajor(w, "W") for w in Ws]),
                                           _ptr_array(acts), _rowmajor(acts[0], "hin"), w_out.data_ptr(), dhin.data_ptr(), 64,
                                           grads.data_ptr(), M, ws.data_ptr(), nbytes, parts, _stream()),
               "rp_mlp_tail_bwd")

    with _Timed("mlp_tail_bwd", f"{M}x64x{L}", 4 * M * (64 * (L + 2) + 1), 2 * M * (2 * 64 * 64 * L + 128)):
        if LaunchPlan.is_recording():
            # a captured step: the second stage (workspace -> grads, ~20 us of latency) reads nothing the following
            # launches write and nobody needs `grads` before the optimizer: it joins the plan's inline section (the second
            # side stream) behind the next launches recorded there, instead of standing between this launch and the first
            # layer's backward.  The plan keeps the closure, and with it the workspace, until that section is joined.
            launch(1)
            LaunchPlan.defer_side(lambda: launch(2))
        else:
            launch(3)
    dWs = [grads[l * 4096:(l + 1) * 4096].view(64, 64) for l in range(L)]
    dbs = [grads[L * 4096 + l * 64:L * 4096 + (l + 1) * 64] for l in range(L)]
    return dhin, dWs, dbs, grads[L * 4160:L * 4160 + 64].view(1, 64), grads[L * 4160 + 64:L * 4160 + 65]


_drop_calls = 0
# the dropout state of the GraphedTrainStep whose capture is running: {"seed", "clock": int64[1] device tensor, "calls"}
DROPOUT_CAPTURE = [None]


def _dropout_seed_offset(device):
    """(seed, offset) for one dropout call, tied to torch's RNG state: the seed is the device generator's (set by
    torch.manual_seed), the offset its Philox offset, advanced by 4 per call (the granularity torch accepts) so that
    other torch random ops interleave consistently.  Falls back to a process-wide call counter if this torch build does
    not expose generator offsets."""
    global _drop_calls
    if torch.cuda.is_current_stream_capturing():
        st = DROPOUT_CAPTURE[0]
        if st is None:
            raise RuntimeError("dropout inside a stream capture that is not a GraphedTrainStep's: its (seed, offset) are launch "
                               "arguments and would be frozen (every replay would draw the same mask)")
        # a captured step: the offset is read on the device (st['clock'] = the generator offset of the step's start) plus
        # this call's place in the step; the step's last launch advances the clock (graph_step.GraphedTrainStep)
        delta = 4 * st["calls"]
        st["calls"] += 1
        return st["seed"], delta, st["clock"]
    try:
        gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
        seed, off = gen.initial_seed(), gen.get_offset()
        gen.set_offset(off + 4)
        return seed & 0xFFFFFFFFFFFFFFFF, off, None
    except (AttributeError, RuntimeError):
        _drop_calls += 1
        return torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, 4 * _drop_calls, None


def dropout_fwd(x, p: float, seed: Optional[int] = None, offset: Optional[int] = None):
    """-> (y, mask uint8 [M, N]); seed / offset default to torch's device generator state (advanced)."""
    _req(x, torch.float32, "x")
    M, N = x.shape
    clock = None
    if seed is None:
        seed, offset, clock = _dropout_seed_offset(x.device)
    y = _new((M, N), torch.float32, x.device)
    mask = _new((M, N), torch.uint8, x.device)
    with _Timed("dropout_fwd", f"{M}x{N}", 9 * M * N):
        if clock is not None:
            _check(lib().rp_dropout_fwd_dev(x.data_ptr(), _rowmajor(x, "x"), y.data_ptr(), N, mask.data_ptr(), M, N, p, seed,
                                            offset, clock.data_ptr(), _stream()), "rp_dropout_fwd_dev")
        else:
            _check(lib().rp_dropout_fwd(x.data_ptr(), _rowmajor(x, "x"), y.data_ptr(), N, mask.data_ptr(), M, N, p, seed, offset,
                                        _stream()), "rp_dropout_fwd")
    return y, mask


def counter_add_u64(counter, delta: int):
    """*counter += delta (uint64 / int64 device scalar) on the current stream (rp_counter_add_u64)"""
    _check(lib().rp_counter_add_u64(counter.data_ptr(), int(delta), _stream()), "rp_counter_add_u64")


def device_generator(device):
    """torch's default generator of a HIP device"""
    return torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]


def dropout_bwd(dy, mask, p: float):
    M, N = dy.shape
    dx = _new((M, N), torch.float32, dy.device)
    with _Timed("dropout_bwd", f"{M}x{N}", 9 * M * N):
        _check(lib().rp_dropout_bwd(dy.data_ptr(), _rowmajor(dy, "dy"), mask.data_ptr(), dx.data_ptr(), N, M, N, p, _stream()),
               "rp_dropout_bwd")
    return dx


def adam_step_scalars(lr: float, beta1: float, beta2: float, step: int, eps: float = 1e-8):
    """the two per-step scalars of the Adam kernels (see rp_adam_step_scalars): one row of the lazy step table"""
    a, b = C.c_float(0), C.c_float(0)
    _check(lib().rp_adam_step_scalars(lr, beta1, beta2, eps, step, C.byref(a), C.byref(b)), "rp_adam_step_scalars")
    return a.value, b.value


def adam_step_scalars_range(lr: float, beta1: float, beta2: float, step0: int, n: int, eps: float = 1e-8) -> torch.Tensor:
    """[n, 2] float32 HOST tensor: row i = adam_step_scalars(.., step0 + i) — one C call (rp_adam_step_scalars_range)"""
    out = torch.empty((n, 2), dtype=torch.float32)
    _check(lib().rp_adam_step_scalars_range(lr, beta1, beta2, eps, step0, n, out.data_ptr()), "rp_adam_step_scalars_range")
    return out


def lazy_adam_rows(sorted_keys, D: int, p, g, m, v, last, scalars, t_target: int, real_step: bool, zero_grad: bool,
                   beta1: float, beta2: float, eps: float, cf_table=None, cf_from: int = 0, t_dev=None):
    """cf_table (from lazy_adam_cf_table, built for the end step of this call's replay) selects the closed-form replay
    of the steps after `cf_from`; None = the bit-exact serial replay"""
    with _Timed("lazy_adam_rows_step" if real_step else "lazy_adam_rows_replay", f"D={D}"):
        _check(lib().rp_lazy_adam_rows(sorted_keys.data_ptr(), sorted_keys.numel(), D, p.data_ptr(), _ptr(g),
                                       m.data_ptr(), v.data_ptr(), last.data_ptr(), scalars.data_ptr(), t_target,
                                       int(real_step), int(zero_grad), beta1, beta2, eps, _ptr(cf_table), cf_from,
                                       _ptr(t_dev), _stream()),
               "rp_lazy_adam_rows")


def lazy_adam_flush(rows: int, D: int, p, m, v, last, scalars, t_target: int, beta1: float, beta2: float, eps: float,
                    cf_table=None, cf_from: int = 0):
    with _Timed("lazy_adam_flush", f"D={D}"):
        _check(lib().rp_lazy_adam_flush(rows, D, p.data_ptr(), m.data_ptr(), v.data_ptr(), last.data_ptr(),
                                        scalars.data_ptr(), t_target, beta1, beta2, eps, _ptr(cf_table), cf_from,
                                        _stream()),
               "rp_lazy_adam_flush")


def lazy_adam_catchup(sorted_keys, D: int, p, g, m, v, last, scalars, t_done: int, mark, beta1: float,
                      beta2: float, eps: float, cf_table=None, cf_from: int = 0, t_dev=None, shadow=None):
    """deferred execution (rp_lazy_adam_catchup): everything the unique rows of sorted_keys are owed through step t_done —
    their pending real step, then the zero-gradient steps — and, with mark, the stamp 'gradient of step t_done+1 coming'.
    mark = 2: stamp, and leave the applied gradient rows uncleared (the caller's backward overwrites them).
    shadow: the bf16 lookup copy of the tables (bf16-storage training), written wherever a parameter row is"""
    with _Timed("lazy_adam_catchup", f"D={D}"):
        _check(lib().rp_lazy_adam_catchup(sorted_keys.data_ptr(), sorted_keys.numel(), D, p.data_ptr(), _ptr(g),
                                          m.data_ptr(), v.data_ptr(), last.data_ptr(), scalars.data_ptr(), t_done,
                                          int(mark), beta1, beta2, eps, _ptr(cf_table), cf_from, _ptr(t_dev), _ptr(shadow),
                                          _stream()), "rp_lazy_adam_catchup")


def lazy_adam_flush_deferred(rows: int, D: int, p, g, m, v, last, scalars, t_target: int, beta1: float, beta2: float,
                             eps: float, cf_table=None, cf_from: int = 0, shadow=None):
    with _Timed("lazy_adam_flush", f"D={D}"):
        _check(lib().rp_lazy_adam_flush_deferred(rows, D, p.data_ptr(), _ptr(g), m.data_ptr(), v.data_ptr(),
                                                 last.data_ptr(), scalars.data_ptr(), t_target, beta1, beta2, eps,
                                                 _ptr(cf_table), cf_from, _ptr(shadow), _stream()),
               "rp_lazy_adam_flush_deferred")


def rows_to_bf16(sorted_keys, D: int, p, shadow):
    """shadow[row] = bf16(p[row]) for the unique rows of sorted_keys (rp_rows_to_bf16)"""
    _req(shadow, torch.bfloat16, "shadow")
    with _Timed("rows_to_bf16"):
        _check(lib().rp_rows_to_bf16(sorted_keys.data_ptr(), sorted_keys.numel(), D, p.data_ptr(), shadow.data_ptr(), _stream()),
               "rp_rows_to_bf16")


def lazy_adam_cf_table(ns_d, t_end: int, cf_from: int, beta1: float, beta2: float, cf_table, built_to: int = -1, t_dev=None):
    """bring the closed-form replay table to replays ending at step t_end (see rp_lazy_adam_cf_table): ns_d [>= t_end + 1, 2]
    float64 device table by step, cf_table [capacity > t_end, 8] float32 (written in place).  built_to: the t_end of the
    previous call on this buffer (only the stamps that were not final then are rebuilt), -1 = a fresh buffer."""
    assert ns_d.dtype == torch.float64 and ns_d.is_contiguous() and (t_dev is not None or ns_d.shape[0] > t_end)
    assert cf_table.dtype == torch.float32 and cf_table.is_contiguous() and (t_dev is not None or cf_table.shape[0] > t_end)
    with _Timed("lazy_adam_cf_table"):
        _check(lib().rp_lazy_adam_cf_table(ns_d.data_ptr(), t_end, cf_from, beta1, beta2, cf_table.data_ptr(), cf_table.shape[0],
                                           built_to, _ptr(t_dev), _stream()), "rp_lazy_adam_cf_table")


POOL_MODES = {"sum": 0, "average": 1}


def embed_gather_pool_fwd(arena, row_base: int, row_count: int, ids, offsets, L: int, B: int, mode: str, err_flag,
                          want_bwd: bool):
    """rp_embed_gather_pool_fwd: pooled multi-id lookup of ONE table.  ids: flat int64 [nnz] (dense bags: nnz = B * L,
    offsets None; CSR: offsets int64 [B + 1]).  Returns (out [B, D], inv [B, D] or None, bag_of int32 [nnz] or None)."""
    _req(arena, torch.float32, "arena")
    D = arena.shape[1]
    out = _new((B, D), torch.float32, arena.device)
    inv = _new((B, D), torch.float32, arena.device) if (want_bwd and mode == "average") else None
    bag = _new((ids.numel(),), torch.int32, arena.device) if (want_bwd and offsets is not None) else None
    nnz = ids.numel()
    with _Timed("embed_gather_pool_fwd", f"D={D}", nnz * (D * 4 + 8) + B * D * 4):
        _check(lib().rp_embed_gather_pool_fwd(arena.data_ptr(), row_base, row_count, ids.data_ptr(), _ptr(offsets), L, B, D,
                                              POOL_MODES[mode], out.data_ptr(), D, _ptr(inv), _ptr(bag), err_flag.data_ptr(),
                                              _stream()), "rp_embed_gather_pool_fwd")
    return out, inv, bag


def embed_pool_bwd(sorted_keys, sorted_pos, D: int, g, scale, bag_of, L: int, grad_arena, accumulate: bool):
    _req(grad_arena, torch.float32, "grad_arena")
    _req(g, torch.float32, "g")
    n = sorted_keys.numel()
    ws, nbytes = _workspace("embed_grad_reduce", n, D, device=grad_arena.device)
    with _Timed("embed_pool_bwd", f"D={D}", n * (D * 4 + 8)):
        _check(lib().rp_embed_pool_bwd(sorted_keys.data_ptr(), sorted_pos.data_ptr(), n, D, g.data_ptr(), _rowmajor(g, "g"),
                                       _ptr(scale), _ptr(bag_of), L, grad_arena.data_ptr(), int(accumulate), ws.data_ptr(),
                                       nbytes, _stream()), "rp_embed_pool_bwd")


def seq_pool_fwd(e, mode: str, want_bwd: bool):
    """MaskedSumPooling / MaskedAveragePooling of an explicit contiguous [B, L, D] tensor -> (out [B, D], inv or None)"""
    _req(e, torch.float32, "e")
    B, L, D = e.shape
    out = _new((B, D), torch.float32, e.device)
    inv = _new((B, D), torch.float32, e.device) if (want_bwd and mode == "average") else None
    with _Timed("seq_pool_fwd", f"{B}x{L}x{D}", (B * L * D + B * D) * 4):
        _check(lib().rp_seq_pool_fwd(e.data_ptr(), B, L, D, POOL_MODES[mode], out.data_ptr(), _ptr(inv), _stream()),
               "rp_seq_pool_fwd")
    return out, inv


def seq_pool_bwd(g, inv, L: int):
    _req(g, torch.float32, "g")
    B, D = g.shape
    de = _new((B, L, D), torch.float32, g.device)
    with _Timed("seq_pool_bwd", f"{B}x{L}x{D}", (B * L * D + B * D) * 4):
        _check(lib().rp_seq_pool_bwd(g.data_ptr(), _ptr(inv), B, L, D, de.data_ptr(), _stream()), "rp_seq_pool_bwd")
    return de


# ---- sequence recall: the full-softmax loss head and the masked history mean (csrc/softmax_ce.hip, csrc/pool.hip) --------
def softmax_ce_geometry() -> dict:
    """{"TB": rows of U per workgroup, "TV": rows of E per tile, "max_d": largest D the kernels take, "slices": lanes per row
    of the finishing merge (slice q merges the splits q, q + slices, ... in ascending order)}"""
    v = [_i32(0) for _ in range(4)]
    _check(lib().rp_softmax_ce_geometry(*[C.byref(x) for x in v]), "rp_softmax_ce_geometry")
    return dict(zip(("TB", "TV", "max_d", "slices"), (x.value for x in v)))


def softmax_ce_splits(B: int, V: int):
    """(number of splits of V, tiles of E per split) of the forward and dU launches for a batch of B rows"""
    n, per = _i32(0), _i64(0)
    _check(lib().rp_softmax_ce_splits(B, V, C.byref(n), C.byref(per)), "rp_softmax_ce_splits")
    return n.value, per.value


def softmax_ce_workspace_bytes(B: int, V: int, D: int) -> int:
    n = _sz(0)
    _check(lib().rp_softmax_ce_workspace_bytes(B, V, D, C.byref(n)), "rp_softmax_ce_workspace_bytes")
    return n.value


def softmax_ce_fits(D: int) -> bool:
    return 1 <= D <= softmax_ce_geometry()["max_d"]


def _sce_args(u, e, target):
    _req(u, torch.float32, "user_emb")
    _req(e, torch.float32, "item_weight")
    _req(target, torch.int64, "target")
    B, D = u.shape
    V = e.shape[0]
    if e.dim() != 2 or e.shape[1] != D or not e.is_contiguous():
        raise RuntimeError(f"softmax_ce: item_weight must be a contiguous [V, {D}] tensor, got {tuple(e.shape)}/{e.stride()}")
    if target.shape != (B,) or not target.is_contiguous():
        raise RuntimeError(f"softmax_ce: target must be a contiguous [{B}] tensor, got {tuple(target.shape)}")
    return B, V, D, _rowmajor(u, "user_emb")


def softmax_ce_fwd(u, e, target, err_flag):
    """rp_softmax_ce_fwd -> (loss float32 [1], lse float32 [B]); u [B, D] (unit inner stride), e [V, D], target int64 [B]"""
    B, V, D, ldu = _sce_args(u, e, target)
    ws, nbytes = _workspace("softmax_ce", B, V, D, device=u.device)
    lse, loss = _new((B,), torch.float32, u.device), _new((1,), torch.float32, u.device)
    with _Timed("softmax_ce_fwd", f"{B}x{V}x{D}", 4 * (B * D + V * D), 2 * B * V * D):
        _check(lib().rp_softmax_ce_fwd(u.data_ptr(), ldu, e.data_ptr(), target.data_ptr(), B, V, D, lse.data_ptr(),
                                       loss.data_ptr(), err_flag.data_ptr(), ws.data_ptr(), nbytes, _stream()),
               "rp_softmax_ce_fwd")
    return loss, lse


def softmax_ce_bwd(u, e, target, lse, gloss, want_du: bool = True, want_de: bool = True):
    """rp_softmax_ce_bwd -> (dU [B, D] or None, dE [V, D] or None); gloss: device float32 [1].  The two gradients are two
    launches, issued (and timed) as one call each."""
    B, V, D, ldu = _sce_args(u, e, target)
    _req(lse, torch.float32, "lse")
    _req(gloss, torch.float32, "gloss")
    ws, nbytes = _workspace("softmax_ce", B, V, D, device=u.device)
    du = _new((B, D), torch.float32, u.device) if want_du else None
    de = _new((V, D), torch.float32, u.device) if want_de else None
    for tag, out, nbytes_moved in (("dU", du, 4 * (2 * B * D + V * D)), ("dE", de, 4 * (B * D + 2 * V * D))):
        if out is None:
            continue
        with _Timed("softmax_ce_bwd", f"{tag} {B}x{V}x{D}", nbytes_moved, 4 * B * V * D):
            _check(lib().rp_softmax_ce_bwd(u.data_ptr(), ldu, e.data_ptr(), target.data_ptr(), lse.data_ptr(), gloss.data_ptr(),
                                           B, V, D, _ptr(du) if tag == "dU" else None, D, _ptr(de) if tag == "dE" else None,
                                           ws.data_ptr(), nbytes, _stream()), "rp_softmax_ce_bwd")
    return du, de


def hist_mean_fwd(e, hist, mask, err_flag):
    """rp_hist_mean_fwd: out[b] = (1/L) sum_l mask[b, l] e[hist[b, l]]; e [V, D], hist int64 [B, L], mask float32 [B, L]"""
    _req(e, torch.float32, "item_weight")
    _req(hist, torch.int64, "hist")
    _req(mask, torch.float32, "mask")
    B, L = hist.shape
    V, D = e.shape
    if not (e.is_contiguous() and hist.is_contiguous() and mask.is_contiguous()) or mask.shape != hist.shape:
        raise RuntimeError("hist_mean: item_weight, hist and mask must be contiguous, hist and mask of one shape")
    out = _new((B, D), torch.float32, e.device)
    with _Timed("hist_mean_fwd", f"D={D}", B * L * (D * 4 + 12) + B * D * 4):
        _check(lib().rp_hist_mean_fwd(e.data_ptr(), V, D, hist.data_ptr(), mask.data_ptr(), B, L, out.data_ptr(), D,
                                      err_flag.data_ptr(), _stream()), "rp_hist_mean_fwd")
    return out


def hist_mean_bwd(hist, mask, g, de):
    """rp_hist_mean_bwd: de[hist[b, l]] += (mask[b, l] / L) g[b] for every position whose id is not 0 (de [V, D], added into)"""
    _req(g, torch.float32, "g")
    _req(de, torch.float32, "dE")
    B, L = hist.shape
    V, D = de.shape
    assert de.is_contiguous() and g.shape == (B, D)
    # (all 32 bits: an id outside the table, skipped by the kernel, must not land inside another id's run)
    sk, sp = sort_pairs(hist.reshape(-1).to(torch.int32))
    with _Timed("hist_mean_bwd", f"D={D}", B * L * (D * 4 + 12)):
        _check(lib().rp_hist_mean_bwd(sk.data_ptr(), sp.data_ptr(), B * L, L, D, V, mask.data_ptr(), g.data_ptr(),
                                      _rowmajor(g, "g"), de.data_ptr(), _stream()), "rp_hist_mean_bwd")
    return de


# ---- sequence recall: the GRU recurrence (csrc/gru.hip) and NARM's attention readout (csrc/narm.hip) ----------------------
def gru_geometry() -> dict:
    """{"TB": batch rows per workgroup, "max_h": largest input / hidden width the kernels take}"""
    tb, mh = _i32(0), _i32(0)
    _check(lib().rp_gru_geometry(C.byref(tb), C.byref(mh)), "rp_gru_geometry")
    return {"TB": tb.value, "max_h": mh.value}


def gru_fits(n_in: int, H: int) -> bool:
    mh = gru_geometry()["max_h"]
    return 1 <= n_in <= mh and 1 <= H <= mh


def gru_workspace_bytes(B: int, L: int, n_in: int, H: int, ids_mode: bool) -> int:
    n = _sz(0)
    _check(lib().rp_gru_workspace_bytes(B, L, n_in, H, int(ids_mode), C.byref(n)), "rp_gru_workspace_bytes")
    return n.value


def _gru_args(ids, e, x, w_ih, w_hh, b_ih, b_hh, steps, last):
    H = w_hh.shape[1]
    named = [("W_ih", w_ih), ("W_hh", w_hh)] + ([("b_ih", b_ih), ("b_hh", b_hh)] if b_ih is not None else [])
    _params(named)
    if (ids is None) == (x is None) or (b_ih is None) != (b_hh is None):
        raise RuntimeError("gru: give either ids (+ item_weight) or x, and both biases or neither")
    if ids is not None:
        _params([("item_weight", e)])
        _req(ids, torch.int64, "ids")
        _req(e, torch.float32, "item_weight")
        (B, L), (V, n_in) = ids.shape, e.shape
        src = ids
    else:
        _req(x, torch.float32, "x")
        B, L, n_in = x.shape
        V, src = 0, x
    if not src.is_contiguous() or w_ih.shape != (3 * H, n_in) or w_hh.shape != (3 * H, H) or \
            (b_ih is not None and (b_ih.shape != (3 * H,) or b_hh.shape != (3 * H,))):
        raise RuntimeError(f"gru: need a contiguous input, W_ih [3H, {n_in}], W_hh [3H, H] and biases [3H], H = {H}")
    for name, t in (("steps", steps), ("last", last)):
        _req(t, torch.int32, name)
        if t.shape != (B,) or not t.is_contiguous():
            raise RuntimeError(f"gru: {name} must be a contiguous int32 [{B}] tensor")
    for name, t in named:
        _req(t, torch.float32, name)
    return B, L, V, n_in, H


def gru_fwd(ids, e, x, w_ih, w_hh, b_ih, b_hh, steps, last, err_flag=None):
    """rp_gru_fwd, one layer -> (H_all [B, L, H], h_last [B, H]); ids int64 [B, L] + e [V, in], or x [B, L, in]"""
    B, L, V, n_in, H = _gru_args(ids, e, x, w_ih, w_hh, b_ih, b_hh, steps, last)
    ws, nbytes = _workspace("gru", B, L, n_in, H, int(ids is not None), device=w_ih.device)
    h_all, h_last = _new((B, L, H), torch.float32, w_ih.device), _new((B, H), torch.float32, w_ih.device)
    with _Timed("gru_fwd", f"{B}x{L}x{n_in}x{H}", 4 * B * L * (n_in + H), 6 * B * L * H * (n_in + H)):
        _check(lib().rp_gru_fwd(_ptr(ids), _ptr(e) if ids is not None else None, V, _ptr(x), B, L, n_in, H, w_ih.data_ptr(),
                                w_hh.data_ptr(), _ptr(b_ih), _ptr(b_hh), steps.data_ptr(), last.data_ptr(), h_all.data_ptr(),
                                h_last.data_ptr(), _ptr(err_flag), ws.data_ptr(), nbytes, _stream()), "rp_gru_fwd")
    return h_all, h_last


def gru_bwd(ids, e, x, w_ih, w_hh, b_ih, b_hh, steps, last, h_all, dh_all, dh_last, want_dx: bool, want_dw: bool):
    """rp_gru_bwd, one layer -> (dX [B, L, in] or None, dW_ih, dW_hh, db_ih, db_hh; the last four None unless want_dw,
    the biases' None without biases)"""
    B, L, V, n_in, H = _gru_args(ids, e, x, w_ih, w_hh, b_ih, b_hh, steps, last)
    dev = w_ih.device
    for name, t, shape in (("H_all", h_all, (B, L, H)), ("dH_all", dh_all, (B, L, H)), ("dh_last", dh_last, (B, H))):
        if t is not None:
            _req(t, torch.float32, name)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError(f"gru_bwd: {name} must be a contiguous {shape} tensor, got {tuple(t.shape)}/{t.stride()}")
    ws, nbytes = _workspace("gru", B, L, n_in, H, int(ids is not None), device=dev)
    dx = _new((B, L, n_in), torch.float32, dev) if want_dx else None
    dwi = _new((3 * H, n_in), torch.float32, dev) if want_dw else None
    dwh = _new((3 * H, H), torch.float32, dev) if want_dw else None
    dbi = _new((3 * H,), torch.float32, dev) if (want_dw and b_ih is not None) else None
    dbh = _new((3 * H,), torch.float32, dev) if (want_dw and b_ih is not None) else None
    with _Timed("gru_bwd", f"{B}x{L}x{n_in}x{H}", 4 * B * L * (n_in + 8 * H), 18 * B * L * H * (n_in + H)):
        _check(lib().rp_gru_bwd(_ptr(ids), _ptr(e) if ids is not None else None, V, _ptr(x), B, L, n_in, H, w_ih.data_ptr(),
                                w_hh.data_ptr(), _ptr(b_ih), _ptr(b_hh), steps.data_ptr(), last.data_ptr(), h_all.data_ptr(),
                                _ptr(dh_all), _ptr(dh_last), _ptr(dx), _ptr(dwi), _ptr(dwh), _ptr(dbi), _ptr(dbh),
                                ws.data_ptr(), nbytes, _stream()), "rp_gru_bwd")
    return dx, dwi, dwh, dbi, dbh


def hist_rows_fwd(e, hist, err_flag):
    """rp_hist_rows_fwd: e [V, D], hist int64 [B, L] -> e[hist] as a [B, L, D] tensor"""
    _req(e, torch.float32, "item_weight")
    _req(hist, torch.int64, "hist")
    if not (e.is_contiguous() and hist.is_contiguous()):
        raise RuntimeError("hist_rows: item_weight and hist must be contiguous")
    (B, L), (V, D) = hist.shape, e.shape
    out = _new((B, L, D), torch.float32, e.device)
    with _Timed("hist_rows_fwd", f"D={D}", B * L * (D * 8 + 8)):
        _check(lib().rp_hist_rows_fwd(e.data_ptr(), V, D, hist.data_ptr(), B * L, out.data_ptr(), err_flag.data_ptr(), _stream()),
               "rp_hist_rows_fwd")
    return out


def hist_rows_bwd(hist, g, de):
    """rp_hist_rows_bwd: de[hist[b, l]] += g[b, l] for every position whose id is not 0 (g [B, L, D], de [V, D], added into)"""
    _req(g, torch.float32, "g")
    _req(de, torch.float32, "dE")
    B, L = hist.shape
    V, D = de.shape
    assert de.is_contiguous() and g.is_contiguous() and g.shape == (B, L, D)
    sk, sp = sort_pairs(hist.reshape(-1).to(torch.int32))
    with _Timed("hist_rows_bwd", f"D={D}", B * L * (D * 4 + 8)):
        _check(lib().rp_hist_rows_bwd(sk.data_ptr(), sp.data_ptr(), B * L, D, V, g.data_ptr(), D, de.data_ptr(), _stream()),
               "rp_hist_rows_bwd")
    return de


def narm_attn_fits(H: int) -> bool:
    return 1 <= H <= 128


def _narm_args(q1, q2, v, ids, g, ht):
    B, L, H = g.shape
    for name, t, shape in (("q1", q1, (B, L, H)), ("q2", q2, (B, H)), ("v", v, (H,)), ("gru_out", g, (B, L, H)),
                           ("ht", ht, (B, H))):
        _req(t, torch.float32, name)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"narm_attention: {name} must be a contiguous {shape} tensor, got {tuple(t.shape)}/{t.stride()}")
    _req(ids, torch.int64, "ids")
    if tuple(ids.shape) != (B, L) or not ids.is_contiguous():
        raise RuntimeError(f"narm_attention: ids must be a contiguous int64 [{B}, {L}] tensor")
    return B, L, H


def narm_attn_fwd(q1, q2, v, ids, g, ht):
    """rp_narm_attn_fwd -> (out [B, 2H], alpha [B, L])"""
    B, L, H = _narm_args(q1, q2, v, ids, g, ht)
    out, alpha = _new((B, 2 * H), torch.float32, g.device), _new((B, L), torch.float32, g.device)
    with _Timed("narm_attn_fwd", f"{B}x{L}x{H}", 8 * B * L * H):
        _check(lib().rp_narm_attn_fwd(q1.data_ptr(), q2.data_ptr(), v.data_ptr(), ids.data_ptr(), g.data_ptr(), ht.data_ptr(),
                                      B, L, H, alpha.data_ptr(), out.data_ptr(), _stream()), "rp_narm_attn_fwd")
    return out, alpha


def narm_attn_bwd(q1, q2, v, ids, g, alpha, dout):
    """rp_narm_attn_bwd -> (dq1, dq2, dv, dG, dht)"""
    B, L, H = g.shape
    _req(dout, torch.float32, "dout")
    if tuple(dout.shape) != (B, 2 * H) or not dout.is_contiguous():
        raise RuntimeError(f"narm_attention: the gradient must be a contiguous [{B}, {2 * H}] tensor")
    dev = g.device
    dq1, dg = _new((B, L, H), torch.float32, dev), _new((B, L, H), torch.float32, dev)
    dq2, dht, dv = _new((B, H), torch.float32, dev), _new((B, H), torch.float32, dev), _new((H,), torch.float32, dev)
    ws, nbytes = _workspace("narm_attn", B, H, device=dev)
    with _Timed("narm_attn_bwd", f"{B}x{L}x{H}", 16 * B * L * H):
        _check(lib().rp_narm_attn_bwd(q1.data_ptr(), q2.data_ptr(), v.data_ptr(), ids.data_ptr(), g.data_ptr(),
                                      alpha.data_ptr(), dout.data_ptr(), B, L, H, dq1.data_ptr(), dq2.data_ptr(), dg.data_ptr(),
                                      dht.data_ptr(), dv.data_ptr(), ws.data_ptr(), nbytes, _stream()), "rp_narm_attn_bwd")
    return dq1, dq2, dv, dg, dht


# ---- sequence recall: the multi-interest encoder of MIND / ComirecDR and the hard readout (csrc/capsule.hip) -------------
def capsule_geometry() -> dict:
    """{"proj_tb", "proj_tn": batch rows / output columns per workgroup of the projection's forward; "max_k", "max_l",
    "max_d", "lds_bytes": the routing launch takes K <= max_k, L <= max_l, D <= max_d with 4 max(K, 2) L (D + 1) <= lds_bytes}"""
    v = [_i32(0) for _ in range(6)]
    _check(lib().rp_capsule_geometry(*[C.byref(x) for x in v]), "rp_capsule_geometry")
    return dict(zip(("proj_tb", "proj_tn", "max_k", "max_l", "max_d", "lds_bytes"), (x.value for x in v)))


def capsule_project_fits(L: int, N: int, D: int) -> bool:
    return 1 <= D <= 128 and 1 <= N <= 2048 and 1 <= L <= 65535


def capsule_workspace_bytes(B: int, L: int, N: int, D: int) -> int:
    n = _sz(0)
    _check(lib().rp_capsule_workspace_bytes(B, L, N, D, C.byref(n)), "rp_capsule_workspace_bytes")
    return n.value


def capsule_route_fits(K: int, L: int, D: int) -> bool:
    g = capsule_geometry()
    return 1 <= K <= g["max_k"] and 1 <= L <= g["max_l"] and 1 <= D <= g["max_d"] and \
        4 * max(K, 2) * L * (D + 1) <= g["lds_bytes"]


def _capsule_dense(named):
    for name, t, shape in named:
        _req(t, torch.float32, name)
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise RuntimeError(f"capsule: {name} must be a contiguous {tuple(shape)} tensor, got {tuple(t.shape)}/{t.stride()}")


def capsule_project_fwd(x, w):
    """rp_capsule_project_fwd: x [B, L, D], w [L, N, D] -> U [B, L, N]"""
    B, L, D = x.shape
    N = w.shape[1]
    _capsule_dense([("x", x, (B, L, D)), ("w", w, (L, N, D))])
    u = _new((B, L, N), torch.float32, x.device)
    with _Timed("capsule_project_fwd", f"{B}x{L}x{N}x{D}", 4 * (B * L * (D + N) + L * N * D), 2 * B * L * N * D):
        _check(lib().rp_capsule_project_fwd(x.data_ptr(), w.data_ptr(), B, L, N, D, u.data_ptr(), _stream()),
               "rp_capsule_project_fwd")
    return u


def capsule_project_bwd(du, x, w, want_dx: bool, want_dw: bool):
    """rp_capsule_project_bwd_x / _bwd_w -> (dX [B, L, D] or None, dW [L, N, D] or None)"""
    B, L, D = x.shape
    N = w.shape[1]
    _capsule_dense([("dU", du, (B, L, N)), ("x", x, (B, L, D)), ("w", w, (L, N, D))])
    dx = dw = None
    if want_dx:
        dx = _new((B, L, D), torch.float32, x.device)
        with _Timed("capsule_project_bwd_x", f"{B}x{L}x{N}x{D}", 4 * (B * L * (D + N) + L * N * D), 2 * B * L * N * D):
            _check(lib().rp_capsule_project_bwd_x(du.data_ptr(), w.data_ptr(), B, L, N, D, dx.data_ptr(), _stream()),
                   "rp_capsule_project_bwd_x")
    if want_dw:
        dw = _new((L, N, D), torch.float32, x.device)
        ws, nbytes = _workspace("capsule", B, L, N, D, device=x.device)
        with _Timed("capsule_project_bwd_w", f"{B}x{L}x{N}x{D}", 4 * (B * L * (D + N) + L * N * D), 2 * B * L * N * D):
            _check(lib().rp_capsule_project_bwd_w(du.data_ptr(), x.data_ptr(), B, L, N, D, dw.data_ptr(),
                                                  ws.data_ptr() if nbytes else None, nbytes, _stream()),
                   "rp_capsule_project_bwd_w")
    return dx, dw


def _capsule_route_args(u_hat, mask, b0, K: int, shared: bool):
    """u_hat [B, L, D] (shared) or [B, L, K D] -> (B, L, D, batch / interest / position strides in floats)"""
    B, L, W = u_hat.shape
    D = W if shared else W // K
    if not shared and D * K != W:
        raise RuntimeError(f"capsule_route: the rows of u_hat ({W} wide) do not split into {K} interests")
    _capsule_dense([("u_hat", u_hat, (B, L, W)), ("mask", mask, (B, L))] + ([("b0", b0, (B, K, L))] if b0 is not None else []))
    return B, L, D, L * W, 0 if shared else D, W


def capsule_route_fwd(u_hat, mask, b0, K: int, shared: bool):
    """rp_capsule_route_fwd -> out [B, K, D]"""
    B, L, D, sb, sk, sl = _capsule_route_args(u_hat, mask, b0, K, shared)
    out = _new((B, K, D), torch.float32, u_hat.device)
    with _Timed("capsule_route_fwd", f"{B}x{K}x{L}x{D}", 4 * B * (u_hat.shape[2] * L + K * D)):
        _check(lib().rp_capsule_route_fwd(u_hat.data_ptr(), sb, sk, sl, mask.data_ptr(), _ptr(b0), B, K, L, D, out.data_ptr(),
                                          _stream()), "rp_capsule_route_fwd")
    return out


def capsule_route_bwd(u_hat, mask, b0, dout, K: int, shared: bool, stop_grad: bool):
    """rp_capsule_route_bwd -> dU with u_hat's shape"""
    B, L, D, sb, sk, sl = _capsule_route_args(u_hat, mask, b0, K, shared)
    _capsule_dense([("dout", dout, (B, K, D))])
    du = _new_like(u_hat)
    with _Timed("capsule_route_bwd", f"{B}x{K}x{L}x{D}", 4 * B * (2 * u_hat.shape[2] * L + K * D)):
        _check(lib().rp_capsule_route_bwd(u_hat.data_ptr(), sb, sk, sl, mask.data_ptr(), _ptr(b0), dout.data_ptr(), B, K, L, D,
                                          int(stop_grad), du.data_ptr(), _stream()), "rp_capsule_route_bwd")
    return du


def interest_pick_fwd(interests, e, target, err_flag):
    """rp_interest_pick_fwd: interests [B, K, D], e [V, D], target int64 [B] -> (best [B, D], kidx int32 [B])"""
    B, K, D = interests.shape
    _capsule_dense([("interests", interests, (B, K, D)), ("item_weight", e, (e.shape[0], D))])
    _req(target, torch.int64, "target")
    if tuple(target.shape) != (B,) or not target.is_contiguous():
        raise RuntimeError(f"interest_pick: target must be a contiguous int64 [{B}] tensor")
    best, kidx = _new((B, D), torch.float32, e.device), _new((B,), torch.int32, e.device)
    with _Timed("interest_pick_fwd", f"{B}x{K}x{D}", 4 * B * D * (K + 2)):
        _check(lib().rp_interest_pick_fwd(interests.data_ptr(), e.data_ptr(), e.shape[0], target.data_ptr(), B, K, D,
                                          best.data_ptr(), kidx.data_ptr(), err_flag.data_ptr(), _stream()),
               "rp_interest_pick_fwd")
    return best, kidx


def interest_pick_bwd(dbest, kidx, K: int):
    """rp_interest_pick_bwd -> dout [B, K, D]: dbest[b] at kidx[b], zeros elsewhere"""
    B, D = dbest.shape
    _capsule_dense([("dbest", dbest, (B, D))])
    dout = _new((B, K, D), torch.float32, dbest.device)
    with _Timed("interest_pick_bwd", f"{B}x{K}x{D}", 4 * B * D * (K + 1)):
        _check(lib().rp_interest_pick_bwd(dbest.data_ptr(), kidx.data_ptr(), B, K, D, dout.data_ptr(), _stream()),
               "rp_interest_pick_bwd")
    return dout


# ---- sequence recall: SASRec's masked multi-head self-attention core and the feed-forward activations (csrc/seq_attn.hip) --
SEQ_ACT_GELU, SEQ_ACT_SWISH = _RP["RP_SEQ_ACT_GELU"], _RP["RP_SEQ_ACT_SWISH"]


def seq_attn_geometry() -> dict:
    """{"max_l", "max_dh": the fused path takes L <= max_l and dh <= max_dh; "row_tile": query rows per wave; "min_dh_tile":
    dh is rounded up to min_dh_tile * 2^k registers per row}"""
    v = [_i32(0) for _ in range(4)]
    _check(lib().rp_seq_attn_geometry(*[C.byref(x) for x in v]), "rp_seq_attn_geometry")
    return dict(zip(("max_l", "max_dh", "row_tile", "min_dh_tile"), (x.value for x in v)))


def seq_attn_fits(L: int, heads: int, dh: int) -> bool:
    return bool(lib().rp_seq_attn_fits(L, heads, dh))


def seq_attn_seed_offset(device):
    """(seed, offset, clock) of one attention-dropout call: one offset of the device generator's stream, as a dropout call"""
    return _dropout_seed_offset(device)


def _seq_attn_args(q, kv, mask, qpos, heads: int, compact: bool):
    """q: [B L, >= D] rows (full mode, or last-row mode on the stacked buffer) or [B, >= D] (compact); kv [B L, >= 2 D]: K | V;
    mask float [B, L]; qpos int64 [B] or None -> (B, L, D, dh)"""
    B, L = mask.shape
    _req(mask, torch.float32, "mask")
    if not mask.is_contiguous():
        raise RuntimeError("seq_attn: mask must be contiguous")
    if kv.shape[1] % 2 or (kv.shape[1] // 2) % heads:
        raise RuntimeError(f"seq_attn: K | V rows of {kv.shape[1]} columns do not split into 2 x {heads} heads")
    D = kv.shape[1] // 2
    _req(q, torch.float32, "q")
    _req(kv, torch.float32, "kv")
    _rows(kv, "kv", 2 * D, B * L)
    if compact and qpos is None:
        raise RuntimeError("seq_attn: query rows as [B, D] need qpos")
    _rows(q, "q", D, B if compact else B * L)
    if qpos is not None:
        _req(qpos, torch.int64, "qpos")
        if tuple(qpos.shape) != (B,) or not qpos.is_contiguous():
            raise RuntimeError(f"seq_attn: qpos must be a contiguous int64 [{B}] tensor")
    return B, L, D, D // heads


def seq_attn_fwd(q, kv, mask, heads: int, p: float = 0.0, rng=None, qpos=None, compact: bool = False, causal: bool = True):
    """rp_seq_attn_fwd(_dev) -> (ctx [B L, D] or, with qpos, [B, D]; lse [B, heads, L] or [B, heads]).  rng: (seed, offset,
    clock) from seq_attn_seed_offset when p > 0; compact: q holds one row per sample, [B, D] (needs qpos).  causal False:
    rp_seq_attn_keypad_fwd, every query over every content key (no dropout there)."""
    B, L, D, dh = _seq_attn_args(q, kv, mask, qpos, heads, compact)
    rows = B if qpos is not None else B * L
    ctx = _new((rows, D), torch.float32, q.device)
    lse = _new((B, heads) if qpos is not None else (B, heads, L), torch.float32, q.device)
    if not causal:
        if p > 0.0:
            raise RuntimeError("seq_attn: the key-padding mode has no dropout")
        with _Timed("seq_attn_keypad_fwd", f"{B}x{heads}x{L}x{dh}", 4 * (B * L * 3 * D + rows * D), 4 * B * heads * L * L * dh):
            _check(lib().rp_seq_attn_keypad_fwd(q.data_ptr(), _rowmajor(q, "q"), int(compact), kv.data_ptr(), _rowmajor(kv, "kv"),
                                                mask.data_ptr(), _ptr(qpos), B, L, heads, dh, ctx.data_ptr(), lse.data_ptr(),
                                                _stream()), "rp_seq_attn_keypad_fwd")
        return ctx, lse
    seed, offset, clock = rng if (p > 0.0 and rng is not None) else (0, 0, None)
    head = (q.data_ptr(), _rowmajor(q, "q"), int(compact), kv.data_ptr(), _rowmajor(kv, "kv"), mask.data_ptr(), _ptr(qpos), B, L,
            heads, dh, p, seed, offset)
    with _Timed("seq_attn_fwd", f"{B}x{heads}x{L}x{dh}", 4 * (B * L * 3 * D + rows * D), 4 * B * heads * L * L * dh):
        if clock is not None:
            _check(lib().rp_seq_attn_fwd_dev(*head, clock.data_ptr(), ctx.data_ptr(), lse.data_ptr(), _stream()),
                   "rp_seq_attn_fwd_dev")
        else:
            _check(lib().rp_seq_attn_fwd(*head, ctx.data_ptr(), lse.data_ptr(), _stream()), "rp_seq_attn_fwd")
    return ctx, lse


def seq_attn_bwd(q, kv, mask, ctx, dctx, lse, heads: int, p: float = 0.0, rng=None, qpos=None, compact: bool = False, dq=None,
                 dkv=None, causal: bool = True):
    """rp_seq_attn_bwd(_dev) -> (dq with q's rows x D, dkv [B L, 2 D]); dq / dkv: row buffers to write into (the column
    blocks of one [B L, 3 D] buffer, for instance).  causal False: rp_seq_attn_keypad_bwd, which takes no ctx (pass None)."""
    B, L, D, dh = _seq_attn_args(q, kv, mask, qpos, heads, compact)
    rows = B if qpos is not None else B * L
    if ctx is None:
        if causal:
            raise RuntimeError("seq_attn_bwd: the causal backward needs ctx")
        ctx = dctx  # (the key-padding backward does not read it: only the checks below see it)
    _rows(ctx, "ctx", D, rows)
    _rows(dctx, "dctx", D, rows)
    if not (ctx.is_contiguous() and dctx.is_contiguous() and lse.is_contiguous()):
        raise RuntimeError("seq_attn_bwd: ctx, dctx and lse must be contiguous")
    _req(ctx, torch.float32, "ctx")
    _req(dctx, torch.float32, "dctx")
    _req(lse, torch.float32, "lse")
    if dq is None:
        dq = _new((q.shape[0], D), torch.float32, q.device)
    if dkv is None:
        dkv = _new((B * L, 2 * D), torch.float32, q.device)
    _rows(dq, "dq", D, q.shape[0])
    _rows(dkv, "dkv", 2 * D, B * L)
    if not causal:
        with _Timed("seq_attn_keypad_bwd", f"{B}x{heads}x{L}x{dh}", 4 * (B * L * 6 * D + 2 * rows * D), 7 * B * heads * L * L * dh):
            _check(lib().rp_seq_attn_keypad_bwd(q.data_ptr(), _rowmajor(q, "q"), int(compact), kv.data_ptr(), _rowmajor(kv, "kv"),
                                                mask.data_ptr(), _ptr(qpos), dctx.data_ptr(), lse.data_ptr(), B, L,
                                                heads, dh, dq.data_ptr(), _rowmajor(dq, "dq"), dkv.data_ptr(),
                                                _rowmajor(dkv, "dkv"), _stream()), "rp_seq_attn_keypad_bwd")
        return dq, dkv
    seed, offset, clock = rng if (p > 0.0 and rng is not None) else (0, 0, None)
    head = (q.data_ptr(), _rowmajor(q, "q"), int(compact), kv.data_ptr(), _rowmajor(kv, "kv"), mask.data_ptr(), _ptr(qpos),
            ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), B, L, heads, dh, p, seed, offset)
    tail = (dq.data_ptr(), _rowmajor(dq, "dq"), dkv.data_ptr(), _rowmajor(dkv, "dkv"), _stream())
    with _Timed("seq_attn_bwd", f"{B}x{heads}x{L}x{dh}", 4 * (B * L * 6 * D + 2 * rows * D), 14 * B * heads * L * L * dh // 2):
        if clock is not None:
            _check(lib().rp_seq_attn_bwd_dev(*head, clock.data_ptr(), *tail), "rp_seq_attn_bwd_dev")
        else:
            _check(lib().rp_seq_attn_bwd(*head, *tail), "rp_seq_attn_bwd")
    return dq, dkv


def seq_attn_keep_mask(B: int, heads: int, L: int, p: float, seed: int, offset: int, device) -> torch.Tensor:
    """the keep decisions of an attention-dropout call at (seed, offset): uint8 [B, heads, L, L] (rp_seq_attn_keep_mask)"""
    keep = _new((B, heads, L, L), torch.uint8, device)
    _check(lib().rp_seq_attn_keep_mask(B, L, heads, p, seed, offset, None, keep.data_ptr(), _stream()), "rp_seq_attn_keep_mask")
    return keep


def seq_act_fwd(x, act: int):
    """rp_seq_act_fwd: erf-GELU / swish of a 2-D x"""
    _req(x, torch.float32, "x")
    M, N = x.shape
    y = _new((M, N), torch.float32, x.device)
    with _Timed("seq_act_fwd", f"{M}x{N}", 8 * M * N):
        _check(lib().rp_seq_act_fwd(x.data_ptr(), _rowmajor(x, "x"), y.data_ptr(), N, M, N, act, _stream()), "rp_seq_act_fwd")
    return y


def seq_act_bwd(dy, x, act: int):
    """rp_seq_act_bwd: dy * act'(x) from the saved input"""
    _req(dy, torch.float32, "dy")
    M, N = x.shape
    dx = _new((M, N), torch.float32, x.device)
    with _Timed("seq_act_bwd", f"{M}x{N}", 12 * M * N):
        _check(lib().rp_seq_act_bwd(dy.data_ptr(), _rowmajor(dy, "dy"), x.data_ptr(), _rowmajor(x, "x"), dx.data_ptr(), N, M, N,
                                    act, _stream()), "rp_seq_act_bwd")
    return dx


def seq_take_fwd(x, qpos, B: int, L: int):
    """rp_seq_take_fwd: x [B L, D], qpos int64 [B] -> [B, D], row qpos[b] of each sample (zeros where qpos[b] < 0)"""
    D = x.shape[1]
    _rows(x, "x", D, B * L)
    _req(x, torch.float32, "x")
    _req(qpos, torch.int64, "qpos")
    out = _new((B, D), torch.float32, x.device)
    with _Timed("seq_take_fwd", f"{B}x{L}x{D}", 8 * B * D):
        _check(lib().rp_seq_take_fwd(x.data_ptr(), _rowmajor(x, "x"), qpos.data_ptr(), B, L, D, out.data_ptr(), _stream()),
               "rp_seq_take_fwd")
    return out


def seq_take_bwd(dout, qpos, B: int, L: int):
    """rp_seq_take_bwd -> dx [B L, D]: dout[b] at row qpos[b], zeros elsewhere"""
    D = dout.shape[1]
    _req(dout, torch.float32, "dout")
    if tuple(dout.shape) != (B, D) or not dout.is_contiguous():
        raise RuntimeError(f"seq_take_bwd: dout must be a contiguous [{B}, {D}] tensor")
    dx = _new((B * L, D), torch.float32, dout.device)
    with _Timed("seq_take_bwd", f"{B}x{L}x{D}", 4 * B * D * (L + 1)):
        _check(lib().rp_seq_take_bwd(dout.data_ptr(), qpos.data_ptr(), B, L, D, dx.data_ptr(), _stream()), "rp_seq_take_bwd")
    return dx


# ---- sequence recall: NextItNet's residual blocks of dilated causal convolutions (csrc/causal_conv.hip) ------------------------
def causal_conv_geometry() -> dict:
    v = [_i32(0) for _ in range(5)]
    _check(lib().rp_causal_conv_geometry(*[C.byref(x) for x in v]), "rp_causal_conv_geometry")
    return dict(zip(("max_c", "max_k", "max_l", "max_lc", "lds_bytes"), (x.value for x in v)))


def causal_conv_fits(L: int, Cw: int, k: int, one_masked: bool) -> bool:
    return bool(lib().rp_causal_conv_fits(L, Cw, k, int(one_masked)))


def causal_conv_rows(k: int, one_masked: bool) -> int:
    """virtual rows per sample of a last-mode launch: the positions the read row depends on"""
    return k if one_masked else 3 * (k - 1) + 1


def causal_conv_stages(Cw: int, k: int, one_masked: bool):
    """-> ([(Cin, Cout, taps)] per conv, [width] per LayerNorm) in stage order"""
    mid = Cw // 2
    if one_masked:
        return [(Cw, mid, 1), (mid, mid, k), (mid, Cw, 1)], [Cw, mid, mid]
    return [(Cw, Cw, k), (Cw, Cw, k)], [Cw, Cw]


def _causal_conv_args(x, lens, params, k: int, one_masked: bool):
    """params: 12 entries, conv weight 0..2, conv bias 0..2, LayerNorm gamma 0..2, beta 0..2 (None where the block has none)"""
    if x.dim() != 3:
        raise RuntimeError(f"causal_conv: x must be [B, L, C], got {tuple(x.shape)}")
    B, L, Cw = x.shape
    _rows(x.view(B * L, Cw) if x.is_contiguous() else x.reshape(B * L, Cw), "x", Cw, B * L)
    if not x.is_contiguous():
        raise RuntimeError("causal_conv: x must be contiguous")
    convs, lns = causal_conv_stages(Cw, k, one_masked)
    if len(params) != 12:
        raise RuntimeError("causal_conv: params holds 12 entries")
    named = []
    for c in range(3):
        want = convs[c] if c < len(convs) else None
        for slot, shape in ((c, None if want is None else (want[1], want[0], want[2])), (3 + c, None if want is None else (want[1],))):
            t = params[slot]
            if (t is None) != (shape is None) or (t is not None and tuple(t.shape) != shape):
                raise RuntimeError(f"causal_conv: parameter {slot} must be {shape}, got {None if t is None else tuple(t.shape)}")
            if t is not None:
                named.append((f"param{slot}", t))
        n = lns[c] if c < len(lns) else None
        for slot in (6 + c, 9 + c):
            t = params[slot]
            if (t is None) != (n is None) or (t is not None and t.numel() != n):
                raise RuntimeError(f"causal_conv: parameter {slot} must hold {n} elements")
            if t is not None:
                named.append((f"param{slot}", t))
    _params(named)
    if lens.dtype != torch.int64 or tuple(lens.shape) != (B,) or not lens.is_contiguous():
        raise RuntimeError(f"causal_conv: lens must be a contiguous int64 [{B}] tensor")
    _req(x, torch.float32, "x")
    _req(lens, torch.int64, "lens")
    for name, t in named:
        _req(t, torch.float32, name)
    return B, L, Cw


def _ptrs12(ts):
    return (C.c_void_p * 12)(*[None if t is None else t.data_ptr() for t in ts])


def _causal_conv_cost(B, R, Cw, k, one_masked):
    convs, _ = causal_conv_stages(Cw, k, one_masked)
    return 2 * B * R * sum(ci * co * t for ci, co, t in convs), 4 * sum(ci * co * t + co for ci, co, t in convs)


def causal_conv_fwd(x, lens, params, k: int, dilation: int, one_masked: bool, last: bool):
    """rp_causal_conv_fwd, one block -> out [B, L, C] (full mode) or [B, C] (last mode: the row at lens - 1)"""
    B, L, Cw = _causal_conv_args(x, lens, params, k, one_masked)
    R = causal_conv_rows(k, one_masked) if last else L
    ws, nbytes = _workspace("causal_conv", B, L, Cw, k, int(one_masked), int(last), 0, device=x.device)
    out = _new((B, Cw) if last else (B, L, Cw), torch.float32, x.device)
    flops, wbytes = _causal_conv_cost(B, R, Cw, k, one_masked)
    with _Timed("causal_conv_fwd", f"{B}x{R}x{Cw}k{k}{'o' if one_masked else 't'}", 4 * (2 * B * R * Cw + out.numel()) + wbytes, flops):
        _check(lib().rp_causal_conv_fwd(x.data_ptr(), lens.data_ptr(), B, L, Cw, k, int(dilation), int(one_masked), int(last),
                                        _ptrs12(params), out.data_ptr(), ws.data_ptr(), nbytes, _stream()), "rp_causal_conv_fwd")
    return out


def causal_conv_bwd(x, lens, dout, params, k: int, dilation: int, one_masked: bool, last: bool):
    """rp_causal_conv_bwd -> (dx [B, L, C], 12 gradients in the order of params, None where params has None)"""
    B, L, Cw = _causal_conv_args(x, lens, params, k, one_masked)
    _req(dout, torch.float32, "dout")
    if tuple(dout.shape) != ((B, Cw) if last else (B, L, Cw)) or not dout.is_contiguous():
        raise RuntimeError(f"causal_conv_bwd: dout must be a contiguous {(B, Cw) if last else (B, L, Cw)} tensor, got {tuple(dout.shape)}")
    R = causal_conv_rows(k, one_masked) if last else L
    ws, nbytes = _workspace("causal_conv", B, L, Cw, k, int(one_masked), int(last), 1, device=x.device)
    dx = _new((B, L, Cw), torch.float32, x.device)
    grads = [None if p is None else _new(tuple(p.shape), torch.float32, x.device) for p in params]
    flops, wbytes = _causal_conv_cost(B, R, Cw, k, one_masked)
    with _Timed("causal_conv_bwd", f"{B}x{R}x{Cw}k{k}{'o' if one_masked else 't'}", nbytes + 4 * (2 * B * R * Cw + B * L * Cw) + 2 * wbytes, 4 * flops):
        _check(lib().rp_causal_conv_bwd(x.data_ptr(), lens.data_ptr(), dout.data_ptr(), B, L, Cw, k, int(dilation), int(one_masked),
                                        int(last), _ptrs12(params), dx.data_ptr(), _ptrs12(grads), ws.data_ptr(), nbytes,
                                        _stream()), "rp_causal_conv_bwd")
    return dx, grads


# ---- sequence recall: session graphs, the gated graph cell and the row L2 normalisation (csrc/session_graph.hip) --------------
def session_graph_geometry() -> dict:
    v = [_i32(0) for _ in range(2)]
    _check(lib().rp_session_graph_geometry(*[C.byref(x) for x in v]), "rp_session_graph_geometry")
    return dict(zip(("max_l", "samples_per_workgroup"), (x.value for x in v)))


def session_graph(hist):
    """rp_session_graph: hist int64 [B, L] -> (nodes int64 [B, L], alias int32 [B, L], count int32 [B], indeg, outdeg int32 [B, L])"""
    if hist.dim() != 2 or hist.dtype != torch.int64 or not hist.is_contiguous():
        raise RuntimeError(f"session_graph: hist must be a contiguous int64 [B, L] tensor, got {hist.dtype} {tuple(hist.shape)}")
    _req(hist, torch.int64, "hist")
    B, L = hist.shape
    dev = hist.device
    nodes = _new((B, L), torch.int64, dev)
    alias, indeg, outdeg = (_new((B, L), torch.int32, dev) for _ in range(3))
    count = _new((B,), torch.int32, dev)
    with _Timed("session_graph", f"{B}x{L}", 8 * B * L + 20 * B * L):
        _check(lib().rp_session_graph(hist.data_ptr(), B, L, nodes.data_ptr(), alias.data_ptr(), count.data_ptr(), indeg.data_ptr(),
                                      outdeg.data_ptr(), _stream()), "rp_session_graph")
    return nodes, alias, count, indeg, outdeg


def ggnn_geometry() -> dict:
    v = [_i32(0) for _ in range(4)]
    _check(lib().rp_ggnn_geometry(*[C.byref(x) for x in v]), "rp_ggnn_geometry")
    return dict(zip(("max_d", "max_l", "rows_per_workgroup", "lds_bytes"), (x.value for x in v)))


def ggnn_fits(L: int, D: int) -> bool:
    return bool(lib().rp_ggnn_fits(L, D))


def _ggnn_args(h, alias, params):
    """params: W_in, b_in, W_out, b_out, W_ih, b_ih, W_hh, b_hh"""
    if h.dim() != 3:
        raise RuntimeError(f"ggnn_cell: h must be [B, L, D], got {tuple(h.shape)}")
    B, L, D = h.shape
    if h.dtype != torch.float32 or not h.is_contiguous():
        raise RuntimeError("ggnn_cell: h must be a contiguous float32 tensor")
    if alias.dtype != torch.int32 or tuple(alias.shape) != (B, L) or not alias.is_contiguous():
        raise RuntimeError(f"ggnn_cell: alias must be a contiguous int32 [{B}, {L}] tensor")
    shapes = [(D, D), (D,), (D, D), (D,), (3 * D, 2 * D), (3 * D,), (3 * D, D), (3 * D,)]
    if len(params) != 8 or any(tuple(p.shape) != s for p, s in zip(params, shapes)):
        raise RuntimeError(f"ggnn_cell: params must have the shapes {shapes}, got {[tuple(p.shape) for p in params]}")
    named = [(f"param{i}", p) for i, p in enumerate(params)]
    _params(named)
    _req(h, torch.float32, "h")
    _req(alias, torch.int32, "alias")
    for name, t in named:
        _req(t, torch.float32, name)
    return B, L, D


def _ptrs8(ts):
    return (C.c_void_p * 8)(*[t.data_ptr() for t in ts])


def ggnn_cell_fwd(h, alias, params, final: bool):
    """rp_ggnn_cell_fwd, one step -> h' [B, L, D], or with final (seq_hidden [B, L, D], ht [B, D]): the alias read-back"""
    B, L, D = _ggnn_args(h, alias, params)
    ws, nbytes = _workspace("ggnn_cell", B, L, D, 0, device=h.device)
    if final:
        outs = (_new((B, L, D), torch.float32, h.device), _new((B, D), torch.float32, h.device))
        ptrs = (None, outs[0].data_ptr(), outs[1].data_ptr())
    else:
        outs = _new((B, L, D), torch.float32, h.device)
        ptrs = (outs.data_ptr(), None, None)
    with _Timed("ggnn_cell_fwd", f"{B}x{L}x{D}", 8 * B * L * D + 4 * 11 * D * D, 2 * B * L * 11 * D * D):
        _check(lib().rp_ggnn_cell_fwd(h.data_ptr(), alias.data_ptr(), B, L, D, _ptrs8(params), *ptrs, ws.data_ptr(), nbytes,
                                      _stream()), "rp_ggnn_cell_fwd")
    return outs


def ggnn_cell_bwd(h, alias, params, dhout=None, dseq=None, dht=None):
    """rp_ggnn_cell_bwd -> (dh [B, L, D], the 8 gradients in the order of params); each arriving gradient may be None"""
    B, L, D = _ggnn_args(h, alias, params)
    for name, t, shape in (("dhout", dhout, (B, L, D)), ("dseq", dseq, (B, L, D)), ("dht", dht, (B, D))):
        if t is not None:
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError(f"ggnn_cell_bwd: {name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
            _req(t, torch.float32, name)
    ws, nbytes = _workspace("ggnn_cell", B, L, D, 1, device=h.device)
    dh = _new((B, L, D), torch.float32, h.device)
    grads = [_new(tuple(p.shape), torch.float32, h.device) for p in params]
    with _Timed("ggnn_cell_bwd", f"{B}x{L}x{D}", nbytes + 16 * B * L * D, 6 * B * L * 11 * D * D):
        _check(lib().rp_ggnn_cell_bwd(h.data_ptr(), alias.data_ptr(), _ptr(dhout), _ptr(dseq), _ptr(dht), B, L, D, _ptrs8(params),
                                      dh.data_ptr(), _ptrs8(grads), ws.data_ptr(), nbytes, _stream()), "rp_ggnn_cell_bwd")
    return dh, grads


def l2norm_fwd(x):
    """rp_l2norm_fwd: x [M, D] contiguous -> x / max(|x|_2, 1e-12) per row"""
    _req(x, torch.float32, "x")
    if x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError(f"l2norm_fwd: x must be a contiguous 2-D tensor, got {tuple(x.shape)}")
    M, D = x.shape
    y = _new((M, D), torch.float32, x.device)
    with _Timed("l2norm_fwd", f"{M}x{D}", 8 * M * D):
        _check(lib().rp_l2norm_fwd(x.data_ptr(), y.data_ptr(), M, D, _stream()), "rp_l2norm_fwd")
    return y


def l2norm_bwd(x, dy):
    """rp_l2norm_bwd -> dx from the saved input and dy (both [M, D] contiguous)"""
    _req(x, torch.float32, "x")
    _req(dy, torch.float32, "dy")
    if x.dim() != 2 or x.shape != dy.shape or not x.is_contiguous() or not dy.is_contiguous():
        raise RuntimeError(f"l2norm_bwd: x and dy must be contiguous [M, D] tensors, got {tuple(x.shape)}, {tuple(dy.shape)}")
    M, D = x.shape
    dx = _new((M, D), torch.float32, x.device)
    with _Timed("l2norm_bwd", f"{M}x{D}", 12 * M * D):
        _check(lib().rp_l2norm_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), M, D, _stream()), "rp_l2norm_bwd")
    return dx


# ---- sequence recall: two-layer additive attention + pooling of the same rows (csrc/attn_pool.hip) ---------------------------
ATTN_POOL_MASK, ATTN_POOL_SOFTMAX = _RP["RP_ATTN_POOL_MASK"], _RP["RP_ATTN_POOL_SOFTMAX"]


def attn_pool_geometry() -> dict:
    v = [_i32(0) for _ in range(6)]
    _check(lib().rp_attn_pool_geometry(*[C.byref(x) for x in v]), "rp_attn_pool_geometry")
    return dict(zip(("max_d", "max_dh", "max_k", "max_l", "rows_per_workgroup", "lds_bytes"), (x.value for x in v)))


def attn_pool_fits(L: int, D: int, Dh: int, K: int) -> bool:
    return bool(lib().rp_attn_pool_fits(L, D, Dh, K))


def _attn_pool_args(x, valid, w1, w2, c, act, norm):
    if x.dim() != 3:
        raise RuntimeError(f"attn_pool: x must be [B, L, D], got {tuple(x.shape)}")
    B, L, D = x.shape
    if w1.dim() != 2 or w2.dim() != 2 or w1.shape[0] != D or w2.shape[0] != w1.shape[1]:
        raise RuntimeError(f"attn_pool: w1 must be [{D}, Dh] and w2 [Dh, K], got {tuple(w1.shape)}, {tuple(w2.shape)}")
    Dh, K = w2.shape
    if tuple(valid.shape) != (B, L):
        raise RuntimeError(f"attn_pool: valid must be [{B}, {L}], got {tuple(valid.shape)}")
    if c is not None and tuple(c.shape) != (B, Dh):
        raise RuntimeError(f"attn_pool: the bias must be [{B}, {Dh}], got {tuple(c.shape)}")
    if act not in (ACT_SIGMOID, ACT_TANH) or norm not in (ATTN_POOL_MASK, ATTN_POOL_SOFTMAX):
        raise RuntimeError(f"attn_pool: act must be ACT_SIGMOID / ACT_TANH and norm ATTN_POOL_MASK / _SOFTMAX, got {act}, {norm}")
    named = [("x", x), ("valid", valid), ("w1", w1), ("w2", w2)] + ([("bias", c)] if c is not None else [])
    _params(named)
    for name, t in named:
        _req(t, torch.float32, name)
    return B, L, D, Dh, K


def attn_pool_fwd(x, valid, w1, w2, c, act: int, norm: int):
    """rp_attn_pool_fwd -> (out [B, K, D], A [B, L, K]); c [B, Dh] or None"""
    B, L, D, Dh, K = _attn_pool_args(x, valid, w1, w2, c, act, norm)
    ws, nbytes = _workspace("attn_pool", B, L, D, Dh, K, 0, device=x.device)
    out, A = _new((B, K, D), torch.float32, x.device), _new((B, L, K), torch.float32, x.device)
    with _Timed("attn_pool_fwd", f"{B}x{L}x{D}h{Dh}k{K}", 4 * (B * L * D + B * K * D + B * L * K + D * Dh), 2 * B * L * Dh * (D + K) + 2 * B * L * K * D):
        _check(lib().rp_attn_pool_fwd(x.data_ptr(), valid.data_ptr(), w1.data_ptr(), w2.data_ptr(), _ptr(c), B, L, D, Dh, K, act, norm,
                                      out.data_ptr(), A.data_ptr(), ws.data_ptr(), nbytes, _stream()), "rp_attn_pool_fwd")
    return out, A


def attn_pool_bwd(x, valid, w1, w2, c, A, dout, act: int, norm: int):
    """rp_attn_pool_bwd -> (dx [B, L, D], dw1 [D, Dh], dw2 [Dh, K], dc [B, Dh] or None) from the inputs, the kept A and dout"""
    B, L, D, Dh, K = _attn_pool_args(x, valid, w1, w2, c, act, norm)
    for name, t, shape in (("A", A, (B, L, K)), ("dout", dout, (B, K, D))):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"attn_pool_bwd: {name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
        _req(t, torch.float32, name)
    ws, nbytes = _workspace("attn_pool", B, L, D, Dh, K, 1, device=x.device)
    dx, dw1, dw2 = (_new(s, torch.float32, x.device) for s in ((B, L, D), (D, Dh), (Dh, K)))
    dc = None if c is None else _new((B, Dh), torch.float32, x.device)
    with _Timed("attn_pool_bwd", f"{B}x{L}x{D}h{Dh}k{K}", nbytes + 4 * (2 * B * L * D + B * K * D + B * L * K), 6 * B * L * Dh * (D + K) + 4 * B * L * K * D):
        _check(lib().rp_attn_pool_bwd(x.data_ptr(), valid.data_ptr(), w1.data_ptr(), w2.data_ptr(), _ptr(c), A.data_ptr(),
                                      dout.data_ptr(), B, L, D, Dh, K, act, norm, dx.data_ptr(), dw1.data_ptr(), dw2.data_ptr(),
                                      _ptr(dc), ws.data_ptr(), nbytes, _stream()), "rp_attn_pool_bwd")
    return dx, dw1, dw2, dc


# ---- sequence recall: the in-batch contrastive loss of CLRec and ContraRec (csrc/contrast.hip) -------------------------------
def contrast_geometry() -> dict:
    """{"TA", "TB": rows of a / b per tile, "max_d": largest D the kernels take, "max_splits": most splits of b's rows}"""
    v = [_i32(0) for _ in range(4)]
    _check(lib().rp_contrast_geometry(*[C.byref(x) for x in v]), "rp_contrast_geometry")
    return dict(zip(("TA", "TB", "max_d", "max_splits"), (x.value for x in v)))


def contrast_fits(D: int) -> bool:
    return bool(lib().rp_contrast_fits(D))


def contrast_workspace_bytes(n: int, m: int, D: int) -> int:
    nb = _sz(0)
    _check(lib().rp_contrast_workspace_bytes(n, m, D, C.byref(nb)), "rp_contrast_workspace_bytes")
    return nb.value


def _contrast_args(a, b, la, lb):
    """a [n, D], b [m, D] or None (symmetric form), la int64 [n], lb int64 [m] or None -> (n, m, D, lda, ldb)"""
    n, D = a.shape
    lda = _rows(a, "a", D)
    _req(a, torch.float32, "a")
    _req(la, torch.int64, "labels_a")
    if tuple(la.shape) != (n,) or not la.is_contiguous():
        raise RuntimeError(f"contrast: labels_a must be a contiguous int64 [{n}] tensor")
    if b is None:
        if lb is not None:
            raise RuntimeError("contrast: the symmetric form (b None) takes no labels_b")
        return n, n, D, lda, 0
    m = b.shape[0]
    ldb = _rows(b, "b", D)
    if b.shape[1] != D:
        raise RuntimeError(f"contrast: b rows of {b.shape[1]} columns against a's {D}")
    _req(b, torch.float32, "b")
    _req(lb, torch.int64, "labels_b")
    if tuple(lb.shape) != (m,) or not lb.is_contiguous():
        raise RuntimeError(f"contrast: labels_b must be a contiguous int64 [{m}] tensor")
    return n, m, D, lda, ldb


def contrast_fwd(a, b, la, lb, temperature: float, exclude_self: bool = False, scale: float = 1.0):
    """rp_contrast_fwd -> (loss float32 [1], lse float64 [n], c float32 [n]); b / lb None: the symmetric form"""
    n, m, D, lda, ldb = _contrast_args(a, b, la, lb)
    ws, nbytes = _workspace("contrast", n, m, D, device=a.device)
    lse = _new((n,), torch.float64, a.device)
    c, loss = (_new((k,), torch.float32, a.device) for k in (n, 1))
    with _Timed("contrast_fwd", f"{n}x{m}x{D}", 4 * (n * D + m * D), 2 * n * m * D):
        _check(lib().rp_contrast_fwd(a.data_ptr(), lda, _ptr(b), ldb, la.data_ptr(), _ptr(lb), n, m, D, temperature,
                                     int(exclude_self), scale, lse.data_ptr(), c.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                     nbytes, _stream()), "rp_contrast_fwd")
    return loss, lse, c


def contrast_bwd(a, b, la, lb, lse, c, gloss, temperature: float, exclude_self: bool = False, scale: float = 1.0,
                 want_da: bool = True, want_db: bool = True):
    """rp_contrast_bwd -> (da [n, D] or None, db [m, D] or None); gloss: device float32 [1].  Symmetric form (b None):
    (da + db, None)."""
    n, m, D, lda, ldb = _contrast_args(a, b, la, lb)
    _req(lse, torch.float64, "lse")
    _req(c, torch.float32, "c")
    _req(gloss, torch.float32, "gloss")
    ws, nbytes = _workspace("contrast", n, m, D, device=a.device)
    sym = b is None
    da = _new((n, D), torch.float32, a.device) if (want_da or sym) else None
    db = _new((m, D), torch.float32, a.device) if (want_db and not sym) else None
    if da is None and db is None:
        return None, None
    with _Timed("contrast_bwd", f"{n}x{m}x{D}", 4 * (2 * n * D + 2 * m * D), 8 * n * m * D):
        _check(lib().rp_contrast_bwd(a.data_ptr(), lda, _ptr(b), ldb, la.data_ptr(), _ptr(lb), lse.data_ptr(), c.data_ptr(),
                                     gloss.data_ptr(), n, m, D, temperature, int(exclude_self), scale, _ptr(da), D, _ptr(db), D,
                                     ws.data_ptr(), nbytes, _stream()), "rp_contrast_bwd")
    return da, db
