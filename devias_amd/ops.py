"""Tensor-level wrappers over the C ABI (include/devias_amd.h).  PyTorch supplies device memory and the current
HIP stream; every bit of arithmetic happens in libdevias_amd.so.  No function here has a CPU or eager fallback."""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ACT_DGELU, ACT_DRELU, ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, BF16, F32  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16}
_workspaces = {}


def dt_code(t: torch.dtype) -> int:
    try:
        return _DT[t]
    except KeyError:
        raise TypeError(f"devias_amd kernels support float32 and bfloat16 tensors, got {t}") from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: devias_amd kernels need a GPU tensor (HIP extension only; no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous, got strides {t.stride()}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


def _chk_each(who: str, dtype, *items) -> None:
    """_chk with `dtype` and the shape of every (name, tensor, shape) whose tensor is not None"""
    for n, t, shape in items:
        if t is not None:
            _chk(t, f"{who}.{n}", dtype)
            assert tuple(t.shape) == tuple(shape), (n, tuple(t.shape), shape)


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only fp32 scratch buffer per (device, stream): kernels of one stream are ordered, so a buffer is never shared by
    two launches in flight (the weight-gradient side stream gets its own)."""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    n = (int(nbytes) + 3) // 4
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < n:
        ws = torch.empty(max(n, 1 << 20), dtype=torch.float32, device=device)
        _workspaces[key] = ws
    return ws


def attach_workspace(a, nbytes: int, device) -> None:
    """point an argument struct's ws / ws_bytes at the stream's workspace of at least `nbytes`.  A backward passes a.ws_bytes: the stream's workspace may have been
    re-allocated larger since the struct was filled"""
    ws = workspace(nbytes, device)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4


def get_option(name: str) -> int:
    """devias_get_option: the current value of a process-wide option (to restore it after a temporary change)"""
    v = ctypes.c_int32(0)
    _lib.check(_lib.load().devias_get_option(name.encode(), ctypes.byref(v)), "devias_get_option")
    return int(v.value)


def set_option(name: str, value: int) -> None:
    """devias_set_option: change a process-wide option (names, environment variables, defaults and meanings: the option block of include/devias_amd.h)"""
    _lib.check(_lib.load().devias_set_option(name.encode(), int(value)), "devias_set_option")


def option_names() -> Tuple[str, ...]:
    """devias_option_name: every option's name, in the library's table order"""
    lib, names = _lib.load(), []
    while (n := lib.devias_option_name(len(names))) is not None:
        names.append(n.decode())
    return tuple(names)


@contextlib.contextmanager
def options(**changes: int):
    """Scope for option changes: snapshots EVERY option, applies `changes` (an unknown name raises before anything is changed) and on exit -- normal or by an
    exception -- restores the whole snapshot, so set_option calls inside the block are undone too.  Nests."""
    saved = {n: get_option(n) for n in option_names()}
    unknown = sorted(set(changes) - set(saved))
    if unknown:
        raise ValueError(f"unknown option(s) {unknown}; the library has {sorted(saved)}")
    try:
        for n, v in changes.items():
            set_option(n, v)
        yield
    finally:
        for n, v in saved.items():
            set_option(n, v)


def release_gemm_queue_stream(stream=None) -> None:
    """devias_gemm_release_queue_stream: the dynamic tile queues of the persistent GEMM (option gemm_dynamic) live in one ring per device that belongs to the FIRST
    stream that launched a dynamic-queue GEMM; launches on any other stream walk static tile lists (same bits, slower beside concurrent kernels).  A host that moves
    its step to another stream calls this -- after every dynamic-queue launch of the old stream has completed -- to hand the ring to `stream` (default: the current one)."""
    st = torch.cuda.current_stream() if stream is None else stream
    _lib.check(_lib.load().devias_gemm_release_queue_stream(st.cuda_stream), "devias_gemm_release_queue_stream")


def counters(reset: bool = False) -> dict:
    """launch counts per kernel family since the last reset (devias_counter): tests assert WHICH kernels served a step"""
    lib = _lib.load()
    out = {k: int(lib.devias_counter(i)) for k, i in _lib.COUNTERS.items()}
    if reset:
        lib.devias_counters_reset()
    return out


def region_counters() -> dict:
    """calls per fused region / loss entry point of the second counter bank (devias_region_counter) since the last reset; counters(reset=True) resets both banks"""
    lib = _lib.load()
    return {k: int(lib.devias_region_counter(i)) for k, i in _lib.REGION_COUNTERS.items()}


def pool_head_args(B: int, Nt: int, pool: int, eps: float, W: torch.Tensor, bias: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor,
                   drop_mask: Optional[torch.Tensor] = None) -> "_lib.PoolHeadArgs":
    """devias_pool_head_args for head weight W [C, D] in the compute dtype and fp32 bias / LayerNorm vectors; the workspace is the stream's.  The caller keeps the
    tensors alive while the struct is in use (it holds raw pointers)."""
    lib = _lib.load()
    C, D = W.shape
    dt = dt_code(W.dtype)
    _chk(W, "pool_head.W")
    _chk_each("pool_head", torch.float32, ("bias", bias, (C,)), ("ln_w", ln_w, (D,)), ("ln_b", ln_b, (D,)), ("drop_mask", drop_mask, (B, D)))
    a = _lib.PoolHeadArgs()
    a.struct_size = ctypes.sizeof(_lib.PoolHeadArgs)
    a.B, a.Nt, a.D, a.C, a.dtype, a.pool, a.eps = B, Nt, D, C, dt, pool, eps
    a.W, a.bias, a.ln_w, a.ln_b, a.drop_mask = (_p(t) for t in (W, bias, ln_w, ln_b, drop_mask))
    nws = lib.devias_pool_head_workspace_bytes(B, Nt, D, C, dt)
    if nws <= 0:
        raise NotImplementedError(f"devias_pool_head: unsupported dims B={B} Nt={Nt} D={D} C={C} (D in 384 / 768 / 1024, B, Nt >= 1, C >= 2)")
    attach_workspace(a, nws, W.device)
    return a


def pool_head_fwd(a: "_lib.PoolHeadArgs", h: torch.Tensor, save: bool = True):
    """devias_pool_head_fwd: h [B*Nt, D] -> (token [B, D], logits [B, C], the save arena as a uint8 tensor or None)"""
    lib = _lib.load()
    _chk(h, "pool_head.h")
    assert tuple(h.shape) == (a.B * a.Nt, a.D) and dt_code(h.dtype) == a.dtype
    attach_workspace(a, a.ws_bytes, h.device)
    arena = torch.empty((lib.devias_pool_head_save_bytes(a.B, a.D, a.dtype),), dtype=torch.uint8, device=h.device) if save else None
    token = torch.empty((a.B, a.D), dtype=h.dtype, device=h.device)
    logits = torch.empty((a.B, a.C), dtype=h.dtype, device=h.device)
    _lib.check(lib.devias_pool_head_fwd(ctypes.byref(a), h.data_ptr(), token.data_ptr(), logits.data_ptr(), _p(arena), _stream()), "devias_pool_head_fwd")
    return token, logits, arena


def pool_head_bwd(a: "_lib.PoolHeadArgs", arena: torch.Tensor, dlogits: torch.Tensor, dtoken: Optional[torch.Tensor], dx: torch.Tensor, grads) -> None:
    """devias_pool_head_bwd: writes every row of dx [B*Nt, D] and the four fp32 gradients `grads` = (dW [C, D], db [C], dln_w [D], dln_b [D])"""
    lib = _lib.load()
    _chk(dlogits, "pool_head.dlogits"); _chk(dx, "pool_head.dx")
    assert tuple(dlogits.shape) == (a.B, a.C) and tuple(dx.shape) == (a.B * a.Nt, a.D) and dt_code(dx.dtype) == a.dtype and dlogits.dtype == dx.dtype
    _chk_each("pool_head", dx.dtype, ("dtoken", dtoken, (a.B, a.D)))
    _chk_each("pool_head", torch.float32, *zip(("grad",) * 4, grads, ((a.C, a.D), (a.C,), (a.D,), (a.D,))))
    g = _lib.PoolHeadGrads()
    g.struct_size = ctypes.sizeof(_lib.PoolHeadGrads)
    g.dW, g.db, g.dln_w, g.dln_b = [t.data_ptr() for t in grads]
    attach_workspace(a, a.ws_bytes, dx.device)
    _lib.check(lib.devias_pool_head_bwd(ctypes.byref(a), arena.data_ptr(), dlogits.data_ptr(), _p(dtoken), dx.data_ptr(), ctypes.byref(g), _stream()),
               "devias_pool_head_bwd")


def pool_head_launches() -> int:
    """devias_pool_head_fwd / _bwd calls that launched since the last reset (devias_pool_head_launches: a counter of its own, both banks are closed);
    counters(reset=True) resets it too"""
    return int(_lib.load().devias_pool_head_launches())


def two_token_head_args(B: int, Nt: int, eps: float, Wa: torch.Tensor, ba: torch.Tensor, Ws: Optional[torch.Tensor], bs: Optional[torch.Tensor], ln_w: torch.Tensor,
                        ln_b: torch.Tensor, mask_a: Optional[torch.Tensor] = None, mask_s: Optional[torch.Tensor] = None) -> "_lib.TwoTokenHeadArgs":
    """devias_two_token_head_args for head weights Wa [Ca, D], Ws [Cs, D] in the compute dtype and fp32 bias / LayerNorm vectors; Ws = bs = None is the unified head
    (both tokens through Wa).  The workspace is the stream's.  The caller keeps the tensors alive while the struct is in use (it holds raw pointers)."""
    lib = _lib.load()
    unified = Ws is None
    if unified != (bs is None):
        raise ValueError("two_token_head: Ws and bs are given together (separate heads) or not at all (unified head)")
    Ca, D = Wa.shape
    Cs = Ca if unified else Ws.shape[0]
    dt = dt_code(Wa.dtype)
    _chk(Wa, "two_token_head.Wa")
    if not unified:
        _chk(Ws, "two_token_head.Ws", Wa.dtype)
        assert Ws.shape[1] == D
    _chk_each("two_token_head", torch.float32, ("ba", ba, (Ca,)), ("bs", bs, (Cs,)), ("ln_w", ln_w, (D,)), ("ln_b", ln_b, (D,)), ("mask_a", mask_a, (B, D)),
              ("mask_s", mask_s, (B, D)))
    a = _lib.TwoTokenHeadArgs()
    a.struct_size = ctypes.sizeof(_lib.TwoTokenHeadArgs)
    a.B, a.Nt, a.D, a.Ca, a.Cs, a.dtype, a.unified, a.eps = B, Nt, D, Ca, Cs, dt, int(unified), eps
    a.Wa, a.Ws, a.ba, a.bs, a.ln_w, a.ln_b, a.mask_a, a.mask_s = (_p(t) for t in (Wa, Ws, ba, bs, ln_w, ln_b, mask_a, mask_s))
    nws = lib.devias_two_token_head_workspace_bytes(B, Nt, D, Ca, Cs, int(unified), dt)
    if nws <= 0:
        raise NotImplementedError(f"devias_two_token_head: unsupported dims B={B} Nt={Nt} D={D} Ca={Ca} Cs={Cs} (D in 384 / 768 / 1024, B >= 1, Nt >= 2, Ca, Cs >= 2)")
    attach_workspace(a, nws, Wa.device)
    return a


def two_token_head_fwd(a: "_lib.TwoTokenHeadArgs", h: torch.Tensor, save: bool = True):
    """devias_two_token_head_fwd: h [B*Nt, D] -> (token_a [B, D], token_s [B, D], logits_a [B, Ca], logits_s [B, Cs], the save arena as a uint8 tensor or None).
    Unified head: the two logits are the halves of ONE [2B, Ca] tensor (the library's single GEMM writes it)."""
    lib = _lib.load()
    _chk(h, "two_token_head.h")
    assert tuple(h.shape) == (a.B * a.Nt, a.D) and dt_code(h.dtype) == a.dtype
    attach_workspace(a, a.ws_bytes, h.device)
    arena = torch.empty((lib.devias_two_token_head_save_bytes(a.B, a.D, a.dtype),), dtype=torch.uint8, device=h.device) if save else None
    token_a = torch.empty((a.B, a.D), dtype=h.dtype, device=h.device)
    token_s = torch.empty((a.B, a.D), dtype=h.dtype, device=h.device)
    if a.unified:
        both = torch.empty((2 * a.B, a.Ca), dtype=h.dtype, device=h.device)
        logits_a, logits_s = both[:a.B], both[a.B:]
    else:
        logits_a = torch.empty((a.B, a.Ca), dtype=h.dtype, device=h.device)
        logits_s = torch.empty((a.B, a.Cs), dtype=h.dtype, device=h.device)
    _lib.check(lib.devias_two_token_head_fwd(ctypes.byref(a), h.data_ptr(), token_a.data_ptr(), token_s.data_ptr(), logits_a.data_ptr(),
                                             None if a.unified else logits_s.data_ptr(), _p(arena), _stream()), "devias_two_token_head_fwd")
    return token_a, token_s, logits_a, logits_s, arena


def two_token_head_bwd(a: "_lib.TwoTokenHeadArgs", arena: torch.Tensor, dlogits_a: torch.Tensor, dlogits_s: torch.Tensor, dtoken_a: Optional[torch.Tensor],
                       dtoken_s: Optional[torch.Tensor], dx: torch.Tensor, grads) -> None:
    """devias_two_token_head_bwd: writes every row of dx [B*Nt, D] and the fp32 gradients `grads` = (dWa [Ca, D], dba [Ca], dWs [Cs, D], dbs [Cs], dln_w [D], dln_b [D]);
    unified head: dWs = dbs = None"""
    lib = _lib.load()
    _chk(dx, "two_token_head.dx")
    assert tuple(dx.shape) == (a.B * a.Nt, a.D) and dt_code(dx.dtype) == a.dtype
    _chk_each("two_token_head", dx.dtype, ("dlogits_a", dlogits_a, (a.B, a.Ca)), ("dlogits_s", dlogits_s, (a.B, a.Cs)), ("dtoken_a", dtoken_a, (a.B, a.D)),
              ("dtoken_s", dtoken_s, (a.B, a.D)))
    _chk_each("two_token_head", torch.float32, *zip(("grad",) * 6, grads, ((a.Ca, a.D), (a.Ca,), (a.Cs, a.D), (a.Cs,), (a.D,), (a.D,))))
    g = _lib.TwoTokenHeadGrads()
    g.struct_size = ctypes.sizeof(_lib.TwoTokenHeadGrads)
    g.dWa, g.dba, g.dWs, g.dbs, g.dln_w, g.dln_b = [_p(t) for t in grads]
    attach_workspace(a, a.ws_bytes, dx.device)
    _lib.check(lib.devias_two_token_head_bwd(ctypes.byref(a), arena.data_ptr(), dlogits_a.data_ptr(), dlogits_s.data_ptr(), _p(dtoken_a), _p(dtoken_s), dx.data_ptr(),
                                             ctypes.byref(g), _stream()), "devias_two_token_head_bwd")


def two_token_head_launches() -> int:
    """devias_two_token_head_fwd / _bwd calls that launched since the last reset (devias_two_token_head_launches); counters(reset=True) resets it too"""
    return int(_lib.load().devias_two_token_head_launches())


def mixup_clips(x: torch.Tensor, table) -> torch.Tensor:
    """devias_mixup_clips: x [B, ..., H, W] (fp32 or bf16, B even) mixed IN PLACE from `table`, a ctypes array of B _lib.MixupRow (host memory: the rows travel as
    kernel arguments, nothing is copied to the device ahead of the launch); clip i pairs with clip B-1-i"""
    _chk(x, "mixup_clips.x")
    if x.dim() < 3 or x.shape[0] < 2 or x.shape[0] % 2 or x.numel() == 0:
        raise ValueError(f"mixup_clips: x [B, ..., H, W] with an even B >= 2 expected, got {tuple(x.shape)}")
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    if len(table) != B:
        raise ValueError(f"mixup_clips: the table has {len(table)} rows for {B} clips")
    _lib.check(_lib.load().devias_mixup_clips(x.data_ptr(), B, x[0].numel() // (H * W), H, W, dt_code(x.dtype), table, _stream()), "devias_mixup_clips")
    return x


def mixup_target(target: torch.Tensor, num_classes: int, on: float, off: float, w_self, w_other) -> torch.Tensor:
    """devias_mixup_target: int64 labels [B] -> fp32 [B, C], row b = fl(v(y_b) w_self[b]) + fl(v(y_{B-1-b}) w_other[b]) with v = `on` at the label and `off` elsewhere;
    w_self / w_other are HOST sequences of B floats.  A label outside [0, C) makes its row and the partner row NaN."""
    _chk(target, "mixup_target.target", torch.int64)
    B = target.shape[0] if target.dim() == 1 else 0
    if B == 0 or len(w_self) != B or len(w_other) != B or int(num_classes) < 2:
        raise ValueError(f"mixup_target: target [B], B weights each and num_classes >= 2 expected, got {tuple(target.shape)}, {len(w_self)}, {len(w_other)}, {num_classes}")
    out = torch.empty((B, int(num_classes)), dtype=torch.float32, device=target.device)
    fa = ctypes.c_float * B
    _lib.check(_lib.load().devias_mixup_target(target.data_ptr(), B, int(num_classes), float(on), float(off), fa(*w_self), fa(*w_other), out.data_ptr(), _stream()),
               "devias_mixup_target")
    return out


def clip_ingest(src: torch.Tensor, table: torch.Tensor, rows, T: int, out: torch.Tensor) -> torch.Tensor:
    """devias_clip_ingest: src a flat uint8 device buffer, table the fp32 [3, 256] device tap table, rows a ctypes array of B _lib.IngestRow (host memory: the rows
    travel as kernel arguments), out [B, 3, T, S_h, S_w] fp32 or bf16 (any base alignment: a view into a larger allocation is served by the scalar kernel)"""
    _chk(src, "clip_ingest.src", torch.uint8)
    _chk(table, "clip_ingest.table", torch.float32)
    _chk(out, "clip_ingest.out")
    if src.dim() != 1 or table.numel() != 768 or out.dim() != 5 or out.shape[0] != len(rows) or out.shape[1] != 3 or out.shape[2] != int(T):
        raise ValueError(f"clip_ingest: a flat src, a 768-entry table and out [B={len(rows)}, 3, T={T}, S_h, S_w] expected, got {tuple(src.shape)}, {tuple(table.shape)}, {tuple(out.shape)}")
    _lib.check(_lib.load().devias_clip_ingest(src.data_ptr(), src.numel(), table.data_ptr(), rows, out.shape[0], int(T), out.shape[3], out.shape[4], dt_code(out.dtype),
                                              out.data_ptr(), _stream()), "devias_clip_ingest")
    return out


def _chk_randaug(who, buf, rows, T, stats):
    _chk(buf, who + ".buf", torch.uint8)
    _chk(stats, who + ".stats", torch.uint8)
    if buf.dim() != 1 or stats.dim() != 1 or stats.numel() < len(rows) * int(T) * _lib.RANDAUG_STATS_BYTES:
        raise ValueError(f"{who}: a flat buf and flat stats of at least B * T * {_lib.RANDAUG_STATS_BYTES} = {len(rows) * int(T) * _lib.RANDAUG_STATS_BYTES} bytes expected, "
                         f"got {tuple(buf.shape)} and {tuple(stats.shape)}")


def randaug_stats(buf: torch.Tensor, rows, T: int, stats: torch.Tensor) -> torch.Tensor:
    """devias_randaug_stats: the tables / grey levels that the AutoContrast, Equalize and Contrast rows of one layer need, into stats (flat uint8, B * T *
    _lib.RANDAUG_STATS_BYTES); rows a ctypes array of B _lib.RandaugRow (host memory: the rows travel as kernel arguments)"""
    _chk_randaug("randaug_stats", buf, rows, T, stats)
    _lib.check(_lib.load().devias_randaug_stats(buf.data_ptr(), buf.numel(), rows, len(rows), int(T), stats.data_ptr(), _stream()), "devias_randaug_stats")
    return stats


def randaug_apply(buf: torch.Tensor, rows, T: int, stats: torch.Tensor) -> torch.Tensor:
    """devias_randaug_apply: one RandAugment layer on the clips of the flat uint8 device buffer `buf`, IN the buffer: every row's op reads its clip at row.src and
    writes it at row.dst (the same place for a point op)"""
    _chk_randaug("randaug_apply", buf, rows, T, stats)
    _lib.check(_lib.load().devias_randaug_apply(buf.data_ptr(), buf.numel(), rows, len(rows), int(T), stats.data_ptr(), _stream()), "devias_randaug_apply")
    return buf


def randaug_launches() -> int:
    """kernel launches of devias_randaug_stats / devias_randaug_apply since the last reset (devias_randaug_launches: a counter of its own, both banks are closed);
    counters(reset=True) resets it"""
    return int(_lib.load().devias_randaug_launches())


def _chk_soft_ce(who, logits, target):
    _chk(logits, who + ".logits")
    _chk(target, who + ".target", torch.float32)
    if logits.dim() != 2 or target.shape != logits.shape or logits.shape[0] == 0:
        raise ValueError(f"{who}: logits [B, C] and a soft target [B, C] expected, got {tuple(logits.shape)} and {tuple(target.shape)}")
    return logits.shape


def soft_ce_fwd(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """devias_soft_ce_fwd: mean_b sum_c -t[b, c] log_softmax(z)[b, c] of logits [B, C] (fp32 or bf16) against fp32 soft targets [B, C] -> fp32 loss [1]"""
    B, C = _chk_soft_ce("soft_ce_fwd", logits, target)
    lib = _lib.load()
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    ws = workspace(lib.devias_soft_ce_workspace_bytes(B), logits.device)
    _lib.check(lib.devias_soft_ce_fwd(logits.data_ptr(), target.data_ptr(), B, C, dt_code(logits.dtype), loss.data_ptr(), ws.data_ptr(), _stream()), "devias_soft_ce_fwd")
    return loss


def soft_ce_bwd(logits: torch.Tensor, target: torch.Tensor, g_loss: torch.Tensor) -> torch.Tensor:
    """devias_soft_ce_bwd: g_loss is the fp32 DEVICE scalar arriving on the loss"""
    B, C = _chk_soft_ce("soft_ce_bwd", logits, target)
    _chk(g_loss, "soft_ce_bwd.g_loss", torch.float32)
    dz = torch.empty_like(logits)
    _lib.check(_lib.load().devias_soft_ce_bwd(logits.data_ptr(), target.data_ptr(), B, C, dt_code(logits.dtype), g_loss.data_ptr(), dz.data_ptr(), _stream()), "devias_soft_ce_bwd")
    return dz


def _chk_distill(who, student, teacher):
    _chk(student, who + ".student")
    _chk(teacher, who + ".teacher", torch.float32)
    if student.dim() != 2 or teacher.dim() != 2 or teacher.shape[0] != student.shape[0] or student.shape[0] == 0 or teacher.shape[1] > student.shape[1]:
        raise ValueError(f"{who}: student [B, C] and teacher [B, Ct <= C] expected, got {tuple(student.shape)} and {tuple(teacher.shape)}")
    return student.shape[0], student.shape[1], teacher.shape[1]


def distill_fwd(student: torch.Tensor, teacher: torch.Tensor, mode: int, weight: float = 1.0):
    """devias_distill_fwd: student logits [B, C] (fp32 or bf16) against fp32 teacher logits [B, Ct], left-padded with C - Ct columns of (its global minimum - 1)
    -> (fp32 loss [1], the device scalar that holds the minimum, or None without a pad)"""
    B, C, Ct = _chk_distill("distill_fwd", student, teacher)
    lib = _lib.load()
    loss = torch.empty((1,), dtype=torch.float32, device=student.device)
    tmin = torch.empty((1,), dtype=torch.float32, device=student.device) if C > Ct else None
    ws = workspace(lib.devias_distill_workspace_bytes(B), student.device)
    _lib.check(lib.devias_distill_fwd(student.data_ptr(), teacher.data_ptr(), B, C, Ct, dt_code(student.dtype), int(mode), float(weight), _p(tmin), loss.data_ptr(),
                                      ws.data_ptr(), _stream()), "devias_distill_fwd")
    return loss, tmin


def distill_bwd(student: torch.Tensor, teacher: torch.Tensor, tmin: Optional[torch.Tensor], g_loss: torch.Tensor, mode: int, weight: float = 1.0) -> torch.Tensor:
    """devias_distill_bwd: g_loss is the fp32 DEVICE scalar arriving on the loss, tmin the forward's"""
    B, C, Ct = _chk_distill("distill_bwd", student, teacher)
    _chk(g_loss, "distill_bwd.g_loss", torch.float32)
    dz = torch.empty_like(student)
    _lib.check(_lib.load().devias_distill_bwd(student.data_ptr(), teacher.data_ptr(), B, C, Ct, dt_code(student.dtype), int(mode), float(weight), _p(tmin),
                                              g_loss.data_ptr(), dz.data_ptr(), _stream()), "devias_distill_bwd")
    return dz


def auto_split_k(M: int, N: int, K: int, bk: int = 64) -> int:
    """Split the long reduction of a weight-gradient GEMM so that (tiles x splits) is just under ONE full round of the kernel that will run it:
    2 slots per CU for the bf16 256x256 kernel counted in 256x128 halves (512 on MI355X), 3 per CU for the 128x128 kernel (768); the CU count
    is the library's (device CUs minus the option gemm_reserve_cus), the same number the fused regions use (csrc/regions.hip)."""
    cus = _lib.load().devias_policy_gemm_cus()
    if bk == 64 and M % 256 == 0 and N % 128 == 0:
        tiles, slots = (M // 256) * (N // 128), 2 * cus
    else:
        tiles, slots = ((M + 127) // 128) * ((N + 127) // 128), 3 * cus
    if tiles >= slots or K < 8 * bk:
        return 1
    return max(1, min(slots // tiles, K // (4 * bk), 64))


def gemm(A: torch.Tensor, B: torch.Tensor, *, trans_a: bool = False, trans_b: bool = False,
         bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, aux_in: Optional[torch.Tensor] = None,
         aux_out: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, res_mod: int = 0,
         out: Optional[torch.Tensor] = None, out_f32: bool = False, beta: float = 0.0, split_k: int = 1,
         colsum: Optional[torch.Tensor] = None, colsum_beta: float = 0.0,
         row_scale: Optional[torch.Tensor] = None, rows_per_scale: int = 0) -> torch.Tensor:
    """C[M,N] = epilogue(op(A) @ op(B)); see devias_gemm in include/devias_amd.h.
    A: [M,K] (or [K,M] if trans_a); B: [N,K] nn.Linear layout (or [K,N] if trans_b)."""
    _chk(A, "gemm.A"); _chk(B, "gemm.B", A.dtype)
    assert A.dim() == 2 and B.dim() == 2
    M, K = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    N, Kb = (B.shape[1], B.shape[0]) if trans_b else (B.shape[0], B.shape[1])
    if K != Kb:
        raise ValueError(f"gemm: reduction mismatch {K} vs {Kb}")
    cdt = torch.float32 if out_f32 else A.dtype
    if out is None:
        if beta != 0.0:
            raise ValueError("gemm: beta needs an existing `out`")
        out = torch.empty((M, N), dtype=cdt, device=A.device)
    else:
        _chk(out, "gemm.out", cdt)
        assert out.shape == (M, N)
    a = _lib.GemmArgs()
    a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    a.M, a.N, a.K = M, N, K
    a.lda, a.ldb, a.ldc = A.shape[1], B.shape[1], N
    a.trans_a, a.trans_b = int(trans_a), int(trans_b)
    a.dtype = dt_code(A.dtype)
    a.c_f32 = int(cdt == torch.float32)
    a.bias = _p(_chk(bias, "gemm.bias", torch.float32)) if bias is not None else None
    a.act = act
    a.ld_aux = N
    if aux_in is not None:
        _chk(aux_in, "gemm.aux_in", A.dtype); assert aux_in.shape == (M, N)
        a.aux_in = aux_in.data_ptr()
    if aux_out is not None:
        _chk(aux_out, "gemm.aux_out", A.dtype); assert aux_out.shape == (M, N)
        a.aux_out = aux_out.data_ptr()
    if res is not None:
        _chk(res, "gemm.res", A.dtype)
        assert res.shape[-1] == N and res.numel() // N == (res_mod if res_mod > 0 else M)
        a.res, a.ldr, a.res_mod = res.data_ptr(), N, res_mod
    a.beta = beta
    if row_scale is not None:
        _chk(row_scale, "gemm.row_scale", torch.float32); assert rows_per_scale > 0 and row_scale.numel() * rows_per_scale >= M
        a.row_scale, a.rows_per_scale = row_scale.data_ptr(), rows_per_scale
    if split_k == 1 and M <= 256 and K >= 512 and not trans_a:
        # small-M (B*S-row slot MLP) GEMMs are latency bound on a handful of tiles: split K to fill the chip
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        split_k = max(1, min(K // 128, (256 + tiles - 1) // tiles))
    if colsum is not None:            # bias gradient folded into the epilogue (needs the un-split kernel)
        _chk(colsum, "gemm.colsum", torch.float32); assert colsum.numel() == N
        split_k = 1
        a.colsum, a.colsum_beta = colsum.data_ptr(), colsum_beta
        nbytes = max(((M + 127) // 128) * N * 4, _lib.load().devias_colsum_workspace_bytes(M, N))
        a.ws = workspace(nbytes, A.device).data_ptr()
    a.split_k = split_k
    if split_k > 1:
        nbytes = _lib.load().devias_gemm_workspace_bytes(M, N, split_k)
        a.ws = workspace(nbytes, A.device).data_ptr()
    _lib.check(_lib.load().devias_gemm(ctypes.byref(a), _stream()), "devias_gemm")
    return out


def wgrad(dY: torch.Tensor, X: torch.Tensor, out: Optional[torch.Tensor] = None, beta: float = 0.0) -> torch.Tensor:
    """dW[N,K] (fp32) = dY[M,N]^T @ X[M,K]   (weight gradient of Y = X W^T); split-K over the long M reduction."""
    M, N = dY.shape
    K = X.shape[1]
    sk = auto_split_k(N, K, M, bk=64 if dY.dtype == torch.bfloat16 else 16)     # C is [N, K], the reduction runs over M
    return gemm(dY, X, trans_a=True, trans_b=True, out=out, out_f32=True, beta=beta, split_k=sk)


# ---- grouped weight gradients (devias_wgrad_group) ------------------------------------------------------------------------------------------------
# An encoder block's backward leaves its four weight-gradient products (dW2, dW1, dWp, dWqkv) to ONE queue; when WGRAD_GROUP blocks are pending -- and, for the
# rest, in a callback the autograd engine runs before backward() returns -- the queue runs them as one grouped split-K launch + one combine.  The fused region and the
# per-kernel Function enqueue the same jobs in the same order, so both paths keep the same bits.  The queue's references keep the operands alive (the block's
# incoming gradient, its saved activations, dhpre / dqkv / dx1); the gradient tensors are returned to autograd at once and filled later on the same stream.
# What this rests on: between a Function's return and the flush NOTHING reads the returned gradient tensor.  That holds when AccumulateGrad adopts it unread (the
# parameter has no .grad, the tensor object is unshared -- the queue keeps storages, never tensors --, grad mode is off), and it is checked per weight by
# wgrad_deferrable: no .grad, no tensor hooks, no post-accumulate hooks, no grad mode inside backward (create_graph), no anomaly mode (it scans every returned
# gradient).  NOT checked, because Python cannot see them: a weight used twice in one graph (the engine sums its two gradients before AccumulateGrad -- the encoder
# uses each weight once) and hooks registered on the AccumulateGrad NODE itself (torch's DistributedDataParallel does that; this project's GradSync uses
# post-accumulate hooks, which are seen).  A host that needs either sets WGRAD_GROUP = 0.
WGRAD_GROUP = int(os.environ.get("DEVIAS_WGRAD_GROUP", "4"))      # blocks per grouped launch (measured: profiles/wgrad_group.txt); 0 = every product at once, as before
_WGRAD_MAX_JOBS = 64


class _WgradQueue:
    def __init__(self, stream):
        self.stream, self.jobs, self.keep, self.blocks = stream, [], [], 0


_wgrad_queues = {}       # (device index, stream handle) -> _WgradQueue
_wgrad_ws = {}           # the grouped launch's partial tiles, grow-only per (device index, stream handle)
_keep_free = {}          # (device index, bytes) -> retention buffers (dhpre | dqkv | dx1 of a region's backward) not lent out
_keep_made = [0]


def wgrad_job(dY: torch.Tensor, X: torch.Tensor, dW: torch.Tensor, beta: float = 0.0) -> "_lib.WgradJob":
    _chk(dY, "wgrad_job.dY", torch.bfloat16); _chk(X, "wgrad_job.X", torch.bfloat16); _chk(dW, "wgrad_job.dW", torch.float32)
    assert dY.shape[0] == X.shape[0] and dW.shape == (dY.shape[1], X.shape[1])
    return _lib.WgradJob(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), dY.shape[0], dY.shape[1], X.shape[1], dY.shape[1], X.shape[1], beta)


def wgrad_group_plan(job_tiles, k_tiles: int, cus: int):
    """devias_policy_wgrad_group_plan (no GPU needed): ([(tiles, split) per round], [(job, tile, first K-tile, K-tiles, partial index, round) per (round, workgroup)])"""
    lib = _lib.load()
    jt = (ctypes.c_int32 * len(job_tiles))(*job_tiles)
    rounds = (ctypes.c_int32 * 128)()
    n = lib.devias_policy_wgrad_group_plan(jt, len(job_tiles), k_tiles, cus, rounds, 64, None, 0)
    if n < 0:
        raise ValueError(lib.devias_last_error().decode())
    units = (ctypes.c_int32 * (6 * n * cus))()
    assert lib.devias_policy_wgrad_group_plan(jt, len(job_tiles), k_tiles, cus, rounds, 64, units, n * cus) == n
    return [(rounds[2 * i], rounds[2 * i + 1]) for i in range(n)], [tuple(units[6 * i:6 * i + 6]) for i in range(n * cus)]


def wgrad_group(jobs, cus: int = 0, device=None, stream: Optional[int] = None) -> None:
    """devias_wgrad_group: dW_j = beta_j dW_j + dY_j^T X_j for every job (ops.wgrad_job) in one grouped launch; an ineligible list raises"""
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    stream = _stream() if stream is None else stream
    arr = (_lib.WgradJob * len(jobs))(*jobs)
    nbytes = lib.devias_wgrad_group_workspace_bytes(arr, len(jobs), cus)
    if nbytes < 0:
        raise ValueError(lib.devias_last_error().decode())
    key = (device.index or 0, stream)
    ws = _wgrad_ws.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        _wgrad_ws.pop(key, None)
        ws = _wgrad_ws[key] = torch.empty((max(nbytes // 4, 64),), dtype=torch.float32, device=device)
    _lib.check(lib.devias_wgrad_group(arr, len(jobs), cus, ws.data_ptr(), ws.numel() * 4, stream), "devias_wgrad_group")


def wgrad_deferrable(p: Optional[torch.Tensor]) -> bool:
    """a weight's gradient may be filled after its Function has returned only if nothing can read it before the queue is flushed: no gradient yet (autograd then adopts
    the returned tensor without reading it), no tensor hooks, no post-accumulate hooks (GradSync's)"""
    return (WGRAD_GROUP > 0 and p is not None and p.grad is None and not getattr(p, "_backward_hooks", None) and not getattr(p, "_post_accumulate_grad_hooks", None)
            and not torch.is_grad_enabled() and not torch.is_anomaly_enabled())


def wgrad_defer_mask(params, dtype: torch.dtype, M: int, D: int, hid: int, plain: bool) -> int:
    """bit i set = the i-th weight gradient of an encoder block (dW2, dW1, dWp, dWqkv) goes through the queue; 0 where the grouped kernel cannot serve the block's
    shapes (it needs whole 256 x 256 tiles of bf16 and the option gemm256) or the caller says so (`plain` False: element dropout masks, which only the per-kernel path has)"""
    if WGRAD_GROUP <= 0 and _keep_free:
        _keep_made[0] -= sum(len(v) for v in _keep_free.values())
        _keep_free.clear()                                 # switched off: give the retention buffers back
    if not (WGRAD_GROUP > 0 and plain and dtype == torch.bfloat16 and D % 256 == 0 and hid % 256 == 0 and M % 64 == 0 and get_option("gemm256") != 0):
        return 0
    return sum(1 << i for i, p in enumerate(params) if wgrad_deferrable(p))


def keep_buffer(nbytes: int, device) -> torch.Tensor:
    """a retention buffer for one region backward's dhpre | dqkv | dx1: lent until the queue has launched the block's weight gradients (wgrad_flush gives it back)"""
    free = _keep_free.setdefault((torch.device(device).index or 0, int(nbytes)), [])
    if free:
        return free.pop()
    _keep_made[0] += 1
    return torch.empty((int(nbytes),), dtype=torch.uint8, device=device)


def wgrad_enqueue(jobs, keep, device, lent=None) -> None:
    """called from a block's backward: `jobs` run at the next flush; `keep` is whatever must stay alive until then, `lent` a keep_buffer to give back"""
    key = (torch.device(device).index or 0, _stream())
    q = _wgrad_queues.get(key)
    if q is None:
        q = _wgrad_queues[key] = _WgradQueue(key[1])
    if len(q.jobs) + len(jobs) > _WGRAD_MAX_JOBS:
        _wgrad_flush_queue(key, q)
    q.jobs += list(jobs)
    q.keep.append((keep, lent))
    q.blocks += 1
    if q.blocks >= WGRAD_GROUP:
        _wgrad_flush_queue(key, q)
    else:
        torch.autograd.Variable._execution_engine.queue_callback(wgrad_flush)       # runs before backward() returns; a no-op when nothing is pending


def _wgrad_flush_queue(key, q) -> None:
    jobs, keep = q.jobs, q.keep
    q.jobs, q.keep, q.blocks = [], [], 0
    if not jobs:
        return
    device = torch.device("cuda", key[0])
    try:
        wgrad_group(jobs, device=device, stream=q.stream)      # (wgrad_defer_mask admitted only jobs the grouped kernel takes: a refusal here is an error)
    finally:
        for _, lent in keep:
            if lent is not None:
                free = _keep_free.setdefault((key[0], lent.numel()), [])
                if len(free) < WGRAD_GROUP:                # (the pool never holds more than a group's worth: a host that lowers WGRAD_GROUP gets the memory back)
                    free.append(lent)
                else:
                    _keep_made[0] -= 1


def wgrad_flush() -> None:
    """launch everything that is pending (every stream's queue, each on its own stream)"""
    for key, q in list(_wgrad_queues.items()):
        _wgrad_flush_queue(key, q)


def wgrad_pending() -> int:
    return sum(len(q.jobs) for q in _wgrad_queues.values())


def wgrad_keep_stats() -> Tuple[int, int]:
    """(retention buffers alive, of those currently free)"""
    return _keep_made[0], sum(len(v) for v in _keep_free.values())


def encoder_block_infer(x: torch.Tensor, x2: torch.Tensor, B: int, N: int, H: int, eps: float, norms, weights, biases, qscaled=None) -> torch.Tensor:
    """devias_encoder_block_infer: one encoder block's forward with nothing kept for a backward, x [rows, D] -> x2 [rows, D] (rows >= B * N: LayerNorm and the GEMMs
    run over all rows, the attention over (B, N) on the first B * N).  norms = fp32 (n1w, n1b, n2w, n2b); weights = (Wqkv, Wp, W1, W2) in x's dtype, nn.Linear
    layout; biases = fp32 (q_bias | 0 | v_bias, proj, fc1, fc2); qscaled = (WqkvS, qkv_biasS) or None (devias_block_args.WqkvS).  Every intermediate lives in the
    stream's workspace (ops.workspace): one buffer, reused by all blocks of all models on that stream."""
    _chk(x, "encoder_block_infer.x"); _chk(x2, "encoder_block_infer.x2", x.dtype)
    assert x.dim() == 2 and x2.shape == x.shape
    lib = _lib.load()
    rows, D = x.shape
    hid = weights[2].shape[0]
    for t in norms + biases:
        _chk(t, "encoder_block_infer.norms / biases", torch.float32)
    for t in weights:
        _chk(t, "encoder_block_infer.weights", x.dtype)
    a = _lib.BlockArgs()
    a.B, a.N, a.D, a.H, a.hidden, a.dtype, a.eps = B, N, D, H, hid, dt_code(x.dtype), eps
    (a.n1w, a.n1b, a.n2w, a.n2b) = [t.data_ptr() for t in norms]
    (a.Wqkv, a.Wp, a.W1, a.W2) = [t.data_ptr() for t in weights]
    (a.qkv_bias, a.pb, a.b1, a.b2) = [t.data_ptr() for t in biases]
    if qscaled is not None:
        _chk(qscaled[0], "encoder_block_infer.WqkvS", x.dtype); _chk(qscaled[1], "encoder_block_infer.qkv_biasS", torch.float32)
        a.WqkvS, a.qkv_biasS = qscaled[0].data_ptr(), qscaled[1].data_ptr()
    ws = workspace(lib.devias_encoder_block_infer_workspace_bytes(B, N, rows, D, H, hid, a.dtype), x.device)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _lib.check(lib.devias_encoder_block_infer(ctypes.byref(a), x.data_ptr(), x2.data_ptr(), rows, _stream()), "devias_encoder_block_infer")
    return x2


def cast(src: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> torch.Tensor:
    """out = (dtype) src, or (dtype)(scale * src) when `scale` is given (out may be src for fp32 -> fp32)."""
    _chk(src, "cast.src")
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    _chk(out, "cast.out", dtype)
    if scale is not None:
        _lib.check(_lib.load().devias_cast_scale(src.data_ptr(), dt_code(src.dtype), out.data_ptr(), dt_code(dtype), src.numel(), float(scale), _stream()),
                   "devias_cast_scale")
        return out
    _lib.check(_lib.load().devias_cast(src.data_ptr(), dt_code(src.dtype), out.data_ptr(), dt_code(dtype), src.numel(), _stream()),
               "devias_cast")
    return out


def patch_im2col(x: torch.Tensor, tubelet: int, patch: int, dtype: torch.dtype) -> torch.Tensor:
    _chk(x, "patch_im2col.x")
    B, C, T, H, W = x.shape
    n_tok = (T // tubelet) * (H // patch) * (W // patch)
    out = torch.empty((B * n_tok, C * tubelet * patch * patch), dtype=dtype, device=x.device)
    _lib.check(_lib.load().devias_patch_im2col(x.data_ptr(), dt_code(x.dtype), out.data_ptr(), dt_code(dtype), B, C, T, H, W,
                                               tubelet, patch, _stream()), "devias_patch_im2col")
    return out


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, beta: float = 0.0, cols: Optional[tuple] = None) -> torch.Tensor:
    """out[n] = beta * out[n] + sum_m x[m, n]; `cols = (first, count)` sums only that column range of the row-major matrix (row stride = its full width)"""
    _chk(x, "colsum.x")
    M, ld = x.shape
    c0, N = cols if cols is not None else (0, ld)
    assert 0 <= c0 and c0 + N <= ld
    if out is None:
        assert beta == 0.0
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
    ws = workspace(_lib.load().devias_colsum_workspace_bytes(M, N), x.device)
    _lib.check(_lib.load().devias_colsum(x.data_ptr() + c0 * x.element_size(), dt_code(x.dtype), M, N, ld, out.data_ptr(), beta, ws.data_ptr(), _stream()),
               "devias_colsum")
    return out


def rows_reduce_mod(x: torch.Tensor, mod: int) -> torch.Tensor:
    _chk(x, "rows_reduce_mod.x")
    M, N = x.shape
    out = torch.empty((mod, N), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().devias_rows_reduce_mod(x.data_ptr(), dt_code(x.dtype), M, N, mod, out.data_ptr(), _stream()),
               "devias_rows_reduce_mod")
    return out


def rows_broadcast(src: torch.Tensor, M: int, dtype: torch.dtype) -> torch.Tensor:
    _chk(src, "rows_broadcast.src", torch.float32)
    mod, N = src.shape
    out = torch.empty((M, N), dtype=dtype, device=src.device)
    _lib.check(_lib.load().devias_rows_broadcast(src.data_ptr(), mod, N, out.data_ptr(), dt_code(dtype), M, _stream()),
               "devias_rows_broadcast")
    return out


def act_bwd(dy: torch.Tensor, y: torch.Tensor, act: int) -> torch.Tensor:
    _chk(dy, "act_bwd.dy"); _chk(y, "act_bwd.y", dy.dtype)
    dx = torch.empty_like(dy)
    _lib.check(_lib.load().devias_act_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), act, dt_code(dy.dtype), dy.numel(), _stream()),
               "devias_act_bwd")
    return dx


def mul_mask(a: torch.Tensor, mask: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = a * mask (+ b): element-wise dropout with a caller-drawn fp32 mask of 0 / (1/keep) (devias_mul_mask)"""
    _chk(a, "mul_mask.a"); _chk(mask, "mul_mask.mask", torch.float32)
    assert mask.numel() == a.numel()
    if b is not None:
        _chk(b, "mul_mask.b", a.dtype)
    y = torch.empty_like(a)
    _lib.check(_lib.load().devias_mul_mask(a.data_ptr(), mask.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), dt_code(a.dtype), a.numel(), _stream()),
               "devias_mul_mask")
    return y


def row_scale(x: torch.Tensor, scale: torch.Tensor, rows_per_scale: int) -> torch.Tensor:
    _chk(x, "row_scale.x"); _chk(scale, "row_scale.scale", torch.float32)
    M, N = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.load().devias_row_scale(x.data_ptr(), scale.data_ptr(), rows_per_scale, y.data_ptr(), dt_code(x.dtype), M, N, _stream()),
               "devias_row_scale")
    return y


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _chk(a, "add.a"); _chk(b, "add.b", a.dtype)
    y = torch.empty_like(a)
    _lib.check(_lib.load().devias_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), dt_code(a.dtype), a.numel(), _stream()), "devias_add")
    return y


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    _chk(x, "layernorm_fwd.x"); _chk(gamma, "gamma", torch.float32); _chk(beta, "beta", torch.float32)
    M, D = x.shape
    y = torch.empty_like(x)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().devias_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                rstd.data_ptr(), M, D, eps, dt_code(x.dtype), _stream()), "devias_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None, dgamma=None, dbeta=None, beta_acc: float = 0.0, dx_colsum=None):
    _chk(dy, "layernorm_bwd.dy"); _chk(x, "layernorm_bwd.x", dy.dtype)
    M, D = x.shape
    dx = torch.empty_like(x)
    if dgamma is None or dbeta is None:
        assert beta_acc == 0.0
        dgamma = dgamma if dgamma is not None else torch.empty((D,), dtype=torch.float32, device=x.device)
        dbeta = dbeta if dbeta is not None else torch.empty((D,), dtype=torch.float32, device=x.device)
    _chk(dgamma, "layernorm_bwd.dgamma", torch.float32); _chk(dbeta, "layernorm_bwd.dbeta", torch.float32)
    if dres is not None:
        _chk(dres, "layernorm_bwd.dres", dy.dtype)
    ws = workspace(_lib.load().devias_layernorm_bwd_workspace_bytes(M, D), x.device)
    _lib.check(_lib.load().devias_layernorm_bwd(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                _p(dres), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), beta_acc, _p(dx_colsum), M, D,
                                                dt_code(x.dtype), ws.data_ptr(), _stream()), "devias_layernorm_bwd")
    return dx, dgamma, dbeta


def mhsa_fwd(qkv: torch.Tensor, B: int, N: int, H: int, scale: float, out: Optional[torch.Tensor] = None, drop=None, q_prescaled: bool = False):
    """drop = (keep, seed): nn.Dropout(1 - keep) on the softmax matrix, mask = the library's hash of (seed, b, h, i, j) (include/devias_amd.h)"""
    _chk(qkv, "mhsa_fwd.qkv")
    assert qkv.numel() == B * N * 3 * H * 64, "mhsa: head dim must be 64"
    if out is None:
        o = torch.empty((B * N, H * 64), dtype=qkv.dtype, device=qkv.device)
    else:
        o = _chk(out, "mhsa_fwd.out", qkv.dtype)
        assert o.shape == (B * N, H * 64)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    assert not (q_prescaled and drop is not None and float(drop[0]) < 1.0), "mhsa_fwd: q_prescaled is not offered with attention dropout"
    if drop is not None and float(drop[0]) < 1.0:
        _lib.check(_lib.load().devias_mhsa_fwd_dropout(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, scale, dt_code(qkv.dtype),
                                                       float(drop[0]), int(drop[1]) & 0xFFFFFFFFFFFFFFFF, _stream()), "devias_mhsa_fwd_dropout")
        return o, lse
    if q_prescaled:          # the q third of qkv holds q * scale * log2(e) (DEVIAS_ATTN_Q_PRESCALED, bf16; not with attention dropout)
        _lib.check(_lib.load().devias_mhsa_fwd_flags(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, scale, dt_code(qkv.dtype), _lib.ATTN_Q_PRESCALED, _stream()),
                   "devias_mhsa_fwd_flags")
        return o, lse
    _lib.check(_lib.load().devias_mhsa_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, scale, dt_code(qkv.dtype), _stream()),
               "devias_mhsa_fwd")
    return o, lse


def mhsa_bwd_dv_from_do(dtype: torch.dtype, drop=None) -> bool:
    """True where the v_bias gradient is the column sum of d_o (devias_mhsa_bwd_bias_dv_from_do: bf16, no attention dropout, one-wave-per-SIMD dK / dV kernel):
    the caller asks the GEMM that produces d_o for its column sums and passes bias_out = (dbq, None)"""
    keep = float(drop[0]) if drop is not None else 1.0
    return bool(_lib.load().devias_mhsa_bwd_bias_dv_from_do(dt_code(dtype), keep))


def mhsa_bwd(qkv, o, d_o, lse, B: int, N: int, H: int, scale: float, drop=None, bias_out=None, q_prescaled: bool = False):
    """bias_out = (dbq, dbv): fp32 [H * 64] destinations of the q_bias / v_bias gradients (column sums of dQ / dV over all rows), produced by the same call
    (devias_mhsa_bwd_bias: from the kernels' accumulators in bf16, by two column-sum passes in fp32)"""
    _chk(qkv, "mhsa_bwd.qkv"); _chk(o, "mhsa_bwd.o", qkv.dtype); _chk(d_o, "mhsa_bwd.d_o", qkv.dtype)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    if bias_out is not None:
        dbq, dbv = (None if t is None else _chk(t, "mhsa_bwd.bias_out", torch.float32) for t in bias_out)
        assert dbq.numel() == H * 64 and (dbv is None or dbv.numel() == H * 64)      # (dbv = None: only where mhsa_bwd_dv_from_do() says the caller has it from colsum(d_o))
        wsb = int(_lib.load().devias_mhsa_bwd_bias_workspace_bytes(B, N, H))
        ws = torch.empty((2, (wsb + 3) // 4), dtype=torch.float32, device=qkv.device)
        keep, seed = (float(drop[0]), int(drop[1]) & 0xFFFFFFFFFFFFFFFF) if drop is not None else (1.0, 0)
        if q_prescaled:
            _lib.check(_lib.load().devias_mhsa_bwd_bias_flags(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, N, H, scale,
                                                              dt_code(qkv.dtype), keep, seed, dbq.data_ptr(), None if dbv is None else dbv.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(),
                                                              _lib.ATTN_Q_PRESCALED, _stream()), "devias_mhsa_bwd_bias_flags")
            return dqkv
        _lib.check(_lib.load().devias_mhsa_bwd_bias(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, N, H, scale,
                                                    dt_code(qkv.dtype), keep, seed, dbq.data_ptr(), None if dbv is None else dbv.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), _stream()),
                   "devias_mhsa_bwd_bias")
        return dqkv
    assert not (q_prescaled and drop is not None and float(drop[0]) < 1.0), "mhsa_bwd: q_prescaled is not offered with attention dropout"
    if drop is not None and float(drop[0]) < 1.0:
        _lib.check(_lib.load().devias_mhsa_bwd_dropout(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(),
                                                       B, N, H, scale, dt_code(qkv.dtype), float(drop[0]), int(drop[1]) & 0xFFFFFFFFFFFFFFFF, _stream()),
                   "devias_mhsa_bwd_dropout")
        return dqkv
    wsb = int(_lib.load().devias_mhsa_bwd_workspace_bytes(B, N, H))      # row statistics of the one-wave-per-SIMD dK / dV kernel (bf16)
    ws = torch.empty(((wsb + 3) // 4,), dtype=torch.float32, device=qkv.device)
    if q_prescaled:
        _lib.check(_lib.load().devias_mhsa_bwd_flags(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                                     dqkv.data_ptr(), B, N, H, scale, dt_code(qkv.dtype), ws.data_ptr(), _lib.ATTN_Q_PRESCALED, _stream()), "devias_mhsa_bwd_flags")
        return dqkv
    _lib.check(_lib.load().devias_mhsa_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                           dqkv.data_ptr(), B, N, H, scale, dt_code(qkv.dtype), ws.data_ptr(), _stream()), "devias_mhsa_bwd")
    return dqkv


def slot_attn_fwd(q, kv, B, S, N, h, dh, scale, attn_out=None, rsum_out=None):
    _chk(q, "slot_attn_fwd.q"); _chk(kv, "slot_attn_fwd.kv", q.dtype)
    dev = q.device
    attn = attn_out if attn_out is not None else torch.empty((B * h, S, N), dtype=torch.float32, device=dev)
    rsum = rsum_out if rsum_out is not None else torch.empty((B * h, S), dtype=torch.float32, device=dev)
    o = torch.empty((B * S, h * dh), dtype=q.dtype, device=dev)
    ws = workspace(_lib.load().devias_slot_attn_workspace_bytes(B, S, N, h, dh), dev)
    _lib.check(_lib.load().devias_slot_attn_fwd(q.data_ptr(), kv.data_ptr(), attn.data_ptr(), rsum.data_ptr(), o.data_ptr(), B, S, N,
                                                h, dh, scale, dt_code(q.dtype), ws.data_ptr(), _stream()), "devias_slot_attn_fwd")
    return attn, rsum, o


def slot_attn_bwd(q, kv, attn, rsum, o, d_o, d_attn_ext, B, S, N, h, dh, scale, ds_out=None):
    dev = q.device
    _chk(d_o, "slot_attn_bwd.d_o", q.dtype)
    dq = torch.empty_like(q)
    ds = ds_out if ds_out is not None else torch.empty((B * h, S, N), dtype=torch.float32, device=dev)
    if d_attn_ext is not None:
        _chk(d_attn_ext, "slot_attn_bwd.d_attn_ext", torch.float32)
    ws = workspace(_lib.load().devias_slot_attn_workspace_bytes(B, S, N, h, dh), dev)
    _lib.check(_lib.load().devias_slot_attn_bwd(q.data_ptr(), kv.data_ptr(), attn.data_ptr(), rsum.data_ptr(), o.data_ptr(),
                                                d_o.data_ptr(), _p(d_attn_ext), dq.data_ptr(), ds.data_ptr(), B, S, N, h, dh, scale,
                                                dt_code(q.dtype), ws.data_ptr(), _stream()), "devias_slot_attn_bwd")
    return dq, ds


def slot_attn_kv_grad(q_stack, do_stack, ds_stack, attn_stack, rsum_stack, L, B, S, N, h, dh, scale):
    for t, n in ((q_stack, "q_stack"), (do_stack, "do_stack"), (ds_stack, "ds_stack"), (attn_stack, "attn_stack"),
                 (rsum_stack, "rsum_stack")):
        _chk(t, "slot_attn_kv_grad." + n)
    dkv = torch.empty((B * N, 2 * h * dh), dtype=q_stack.dtype, device=q_stack.device)
    _lib.check(_lib.load().devias_slot_attn_kv_grad(q_stack.data_ptr(), do_stack.data_ptr(), ds_stack.data_ptr(), attn_stack.data_ptr(),
                                                    rsum_stack.data_ptr(), dkv.data_ptr(), L, B, S, N, h, dh, scale,
                                                    dt_code(q_stack.dtype), _stream()), "devias_slot_attn_kv_grad")
    return dkv


def gemm_batched(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, *, lda: int, ldb: int, ldc: int,
                 stride_a: int, stride_b: int, stride_c: int, batch: int, trans_a: bool = False, trans_b: bool = False,
                 a_off: int = 0, b_off: int = 0, c_off: int = 0) -> torch.Tensor:
    """`batch` independent C_i[M,N] = op(A_i) @ op(B_i) in one launch (devias_gemm with batch > 1): problem i reads A + a_off + i*stride_a ...
    (element offsets / strides into the given tensors, which only supply base pointers and dtypes).  C may be fp32 with bf16 operands."""
    _chk(A, "gemm_batched.A"); _chk(B, "gemm_batched.B", A.dtype); _chk(C, "gemm_batched.C")
    if C.dtype not in (A.dtype, torch.float32):
        raise TypeError("gemm_batched: C must have the operand dtype or float32")
    a = _lib.GemmArgs()
    es, ec = A.element_size(), C.element_size()
    a.A, a.B, a.C = A.data_ptr() + a_off * es, B.data_ptr() + b_off * es, C.data_ptr() + c_off * ec
    a.M, a.N, a.K = M, N, K
    a.lda, a.ldb, a.ldc = lda, ldb, ldc
    a.trans_a, a.trans_b = int(trans_a), int(trans_b)
    a.dtype = dt_code(A.dtype)
    a.c_f32 = int(C.dtype == torch.float32)
    a.split_k = 1
    a.batch, a.stride_a, a.stride_b, a.stride_c = batch, stride_a, stride_b, stride_c
    _lib.check(_lib.load().devias_gemm(ctypes.byref(a), _stream()), "devias_gemm(batched)")
    return C


def slotf_fwd(qp, ctx, B, S, N, h, D, scale, attn_out=None, rsum_out=None):
    """folded slot attention forward (devias_slotf_fwd): qp [B*S, h*D], ctx [B*N, D] -> attn fp32 [B*h,S,N], rsum fp32 [B*h,S], z [B*S, h*D]"""
    _chk(qp, "slotf_fwd.qp"); _chk(ctx, "slotf_fwd.ctx", qp.dtype)
    dev = qp.device
    attn = attn_out if attn_out is not None else torch.empty((B * h, S, N), dtype=torch.float32, device=dev)
    rsum = rsum_out if rsum_out is not None else torch.empty((B * h, S), dtype=torch.float32, device=dev)
    z = torch.empty((B * S, h * D), dtype=qp.dtype, device=dev)
    ws = workspace(_lib.load().devias_slotf_workspace_bytes(B, S, N, h, D), dev)
    _lib.check(_lib.load().devias_slotf_fwd(qp.data_ptr(), ctx.data_ptr(), attn.data_ptr(), rsum.data_ptr(), z.data_ptr(), B, S, N, h, D,
                                            scale, dt_code(qp.dtype), ws.data_ptr(), _stream()), "devias_slotf_fwd")
    return attn, rsum, z


def slotf_bwd(ctx, attn, rsum, z, dz, d_attn_ext, B, S, N, h, D, scale, ds_out=None):
    _chk(ctx, "slotf_bwd.ctx"); _chk(z, "slotf_bwd.z", ctx.dtype); _chk(dz, "slotf_bwd.dz", ctx.dtype)
    dev = ctx.device
    dqp = torch.empty((B * S, h * D), dtype=ctx.dtype, device=dev)
    ds = ds_out if ds_out is not None else torch.empty((B * h, S, N), dtype=torch.float32, device=dev)
    if d_attn_ext is not None:
        _chk(d_attn_ext, "slotf_bwd.d_attn_ext", torch.float32)
    ws = workspace(_lib.load().devias_slotf_workspace_bytes(B, S, N, h, D), dev)
    _lib.check(_lib.load().devias_slotf_bwd(ctx.data_ptr(), attn.data_ptr(), rsum.data_ptr(), z.data_ptr(), dz.data_ptr(), _p(d_attn_ext),
                                            dqp.data_ptr(), ds.data_ptr(), B, S, N, h, D, scale, dt_code(ctx.dtype), ws.data_ptr(), _stream()),
               "devias_slotf_bwd")
    return dqp, ds


def slotf_context_grad(attn_stack, rsum_stack, ds_stack, dz_stack, qp_stack, L, B, S, N, h, D, scale):
    """dc [B*N, D] of L stacked folded layers that share the context rows: devias_slotf_pack + one batched [N,K] x [K,D] GEMM per clip"""
    for t, n in ((attn_stack, "attn_stack"), (rsum_stack, "rsum_stack"), (ds_stack, "ds_stack"), (dz_stack, "dz_stack"), (qp_stack, "qp_stack")):
        _chk(t, "slotf_context_grad." + n)
    dt, dev = qp_stack.dtype, qp_stack.device
    K = 2 * L * h * S
    Np = (N + 7) // 8 * 8
    coef = torch.empty((B, K, Np), dtype=dt, device=dev)
    vec = torch.empty((B, K, D), dtype=dt, device=dev)
    _lib.check(_lib.load().devias_slotf_pack(attn_stack.data_ptr(), rsum_stack.data_ptr(), ds_stack.data_ptr(), dz_stack.data_ptr(),
                                             qp_stack.data_ptr(), coef.data_ptr(), vec.data_ptr(), L, B, S, N, Np, h, D, scale, dt_code(dt),
                                             _stream()), "devias_slotf_pack")
    dc = torch.empty((B * N, D), dtype=dt, device=dev)
    gemm_batched(coef, vec, dc, N, D, K, lda=Np, ldb=D, ldc=D, stride_a=K * Np, stride_b=K * D, stride_c=N * D, batch=B,
                 trans_a=True, trans_b=True)
    return dc


def slot_select(slots_head: torch.Tensor, B: int, S: int, nb: int) -> torch.Tensor:
    _chk(slots_head, "slot_select.slots_head")
    C = slots_head.shape[-1]
    idx = torch.empty((B, 2), dtype=torch.int32, device=slots_head.device)
    _lib.check(_lib.load().devias_slot_select(slots_head.data_ptr(), dt_code(slots_head.dtype), B, S, C, nb, idx.data_ptr(), _stream()),
               "devias_slot_select")
    return idx


def _loss_dims(slots_head, slots, maskp, attn, B, nb, ns, w_scene, w_mp, w_md, scene_ce=False):
    d = _lib.LossDims()
    d.B = B
    d.S = slots_head.shape[0] // B
    d.C = slots_head.shape[1]
    d.nb, d.ns = nb, ns
    d.D, d.G, d.N = slots.shape[1], maskp.shape[1], attn.shape[2]
    d.nh = attn.shape[0] // B
    d.w_scene, d.w_mask_pred, d.w_mask_distill = w_scene, w_mp, w_md
    d.dtype = dt_code(slots_head.dtype)
    d.scene_ce = 1 if scene_ce else 0
    return d


def _chk_loss(who, slots_head, slots, maskp, attn, scene, labels, target, fg, fgN, nb):
    """The kernels index every tensor from B, S, C, nb, D, G, N and nh alone, so tensors whose rows disagree are refused here, before anything is launched,
    rather than read out of bounds on the device.  `scene` is the int64 labels [B] if `labels`, else the teacher's fp32 logits [B, C - nb]."""
    sname = "scene_target" if labels else "teacher"
    for t, n, dt in ((slots_head, "slots_head", None), (slots, "slots", slots_head.dtype), (maskp, "maskp", slots_head.dtype),
                     (attn, "attn", torch.float32), (target, "target", torch.int64), (scene, sname, torch.int64 if labels else torch.float32),
                     (fg, "fg", torch.float32), (fgN, "fgN", torch.float32)):
        _chk(t, who + "." + n, dt)
    B, rows = target.shape[0], slots_head.shape[0]
    if target.dim() != 1 or scene.shape != ((B,) if labels else (B, slots_head.shape[1] - nb)) or B == 0 or rows % B or slots.shape[0] != rows \
            or maskp.shape[0] != rows or attn.dim() != 3 or attn.shape[0] % B or attn.shape[1] != rows // B or fg.shape != (B, maskp.shape[1]) \
            or fgN.shape != (B, attn.shape[2]):
        raise ValueError(f"{who}: inconsistent shapes slots_head {tuple(slots_head.shape)} slots {tuple(slots.shape)} maskp {tuple(maskp.shape)} attn {tuple(attn.shape)} "
                         f"target {tuple(target.shape)} {sname} {tuple(scene.shape)} fg {tuple(fg.shape)} fgN {tuple(fgN.shape)} nb {nb}")
    return B


def _loss_entry(direction, slots_head, slots, maskp, attn, scene, target, fg, fgN, nb, w_scene, w_mp, w_md, scene_ce):
    """The one place that branches on the recipe, by the scene source's dtype (the kernels' LABELS flag): int64 labels go to the label entry points, which
    take (target, scene_target) where the teacher ones take (teacher, target) and ignore w_scene.  -> (who, B, dims, the ten leading arguments)"""
    labels = scene.dtype == torch.int64
    who = ("head_match_loss_labels_" if labels else "head_match_loss_") + direction
    B = _chk_loss(who, slots_head, slots, maskp, attn, scene, labels, target, fg, fgN, nb)
    d = _loss_dims(slots_head, slots, maskp, attn, B, nb, slots_head.shape[1] - nb, 0.0 if labels else w_scene, w_mp, w_md, scene_ce)
    lead = (slots_head, slots, maskp, attn) + ((target, scene) if labels else (scene, target)) + (fg, fgN)
    return who, B, d, (ctypes.byref(d),) + tuple(t.data_ptr() for t in lead)


def _head_match_loss_fwd(slots_head, slots, maskp, attn, scene, target, fg, fgN, nb, w_scene, w_mp, w_md, scene_ce=False):
    who, B, d, lead = _loss_entry("fwd", slots_head, slots, maskp, attn, scene, target, fg, fgN, nb, w_scene, w_mp, w_md, scene_ce)
    dev = slots_head.device
    losses = torch.empty((6,), dtype=torch.float32, device=dev)
    match = torch.empty((B, 2), dtype=torch.int32, device=dev)
    logits = torch.empty((B, d.C), dtype=slots_head.dtype, device=dev)
    ws = workspace(_lib.load().devias_head_match_loss_workspace_bytes(B), dev)
    _lib.check(getattr(_lib.load(), "devias_" + who)(*lead, losses.data_ptr(), match.data_ptr(), logits.data_ptr(), ws.data_ptr(), _stream()), "devias_" + who)
    return losses, match, logits


def _head_match_loss_bwd(slots_head, slots, maskp, attn, scene, target, fg, fgN, match, g_total, nb, w_scene, w_mp, w_md, scene_ce=False):
    who, B, d, lead = _loss_entry("bwd", slots_head, slots, maskp, attn, scene, target, fg, fgN, nb, w_scene, w_mp, w_md, scene_ce)
    _chk(g_total, who + ".g_total", torch.float32)
    _chk(match, who + ".match", torch.int32)
    dZ = torch.empty_like(slots_head)
    dslots = torch.empty_like(slots)
    dmask = torch.empty_like(maskp)
    dattn = torch.empty_like(attn)
    _lib.check(getattr(_lib.load(), "devias_" + who)(*lead, match.data_ptr(), g_total.data_ptr(), dZ.data_ptr(), dslots.data_ptr(), dmask.data_ptr(),
                                                     dattn.data_ptr(), _stream()), "devias_" + who)
    return dZ, dslots, dmask, dattn


# the four public wrappers pin their scene argument's dtype (so a mistyped one is a TypeError, not the other recipe) and forward
def head_match_loss_fwd(slots_head, slots, maskp, attn, teacher, target, fg, fgN, nb, w_scene, w_mp, w_md, scene_ce=False):
    _chk(teacher, "head_match_loss_fwd.teacher", torch.float32)
    return _head_match_loss_fwd(slots_head, slots, maskp, attn, teacher, target, fg, fgN, nb, w_scene, w_mp, w_md, scene_ce)


def head_match_loss_bwd(slots_head, slots, maskp, attn, teacher, target, fg, fgN, match, g_total, nb, w_scene, w_mp, w_md, scene_ce=False):
    _chk(teacher, "head_match_loss_bwd.teacher", torch.float32)
    return _head_match_loss_bwd(slots_head, slots, maskp, attn, teacher, target, fg, fgN, match, g_total, nb, w_scene, w_mp, w_md, scene_ce)


def head_match_loss_labels_fwd(slots_head, slots, maskp, attn, target, scene_target, fg, fgN, nb, w_mp, w_md, scene_ce=False):
    """devias_head_match_loss_labels_fwd: the 'matching' loss against ground-truth scene labels (int64 [B] in [0, C - nb), not offset by nb)"""
    _chk(scene_target, "head_match_loss_labels_fwd.scene_target", torch.int64)
    return _head_match_loss_fwd(slots_head, slots, maskp, attn, scene_target, target, fg, fgN, nb, 0.0, w_mp, w_md, scene_ce)


def head_match_loss_labels_bwd(slots_head, slots, maskp, attn, target, scene_target, fg, fgN, match, g_total, nb, w_mp, w_md, scene_ce=False):
    _chk(scene_target, "head_match_loss_labels_bwd.scene_target", torch.int64)
    return _head_match_loss_bwd(slots_head, slots, maskp, attn, scene_target, target, fg, fgN, match, g_total, nb, 0.0, w_mp, w_md, scene_ce)


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """devias_adamw_step.  beta1 / beta2 cross the C ABI as doubles (here and in adamw_multi / adamw_ema_multi): the library forms `1 - beta` in double and rounds
    once, as torch does and as ema_factors does for the EMA decay; 1.0f - fl32(0.999) would be 1.3e-5 off 0.001."""
    for t, n in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, "adamw_step." + n, torch.float32)
    _lib.check(_lib.load().devias_adamw_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param.numel(),
                                             lr, beta1, beta2, eps, weight_decay, step, grad_scale, _stream()), "devias_adamw_step")


def grad_sumsq_multi(table, chunk_tensor, chunk_index, partials):
    """devias_grad_sumsq_multi: table uint8 [n_tensors, 64] (devias_opt_tensor records), chunk lists int32, partials fp32."""
    _chk(table, "grad_sumsq_multi.table", torch.uint8); _chk(partials, "grad_sumsq_multi.partials", torch.float32)
    _chk(chunk_tensor, "grad_sumsq_multi.chunk_tensor", torch.int32); _chk(chunk_index, "grad_sumsq_multi.chunk_index", torch.int32)
    _lib.check(_lib.load().devias_grad_sumsq_multi(table.data_ptr(), chunk_tensor.data_ptr(), chunk_index.data_ptr(), chunk_tensor.numel(),
                                                   partials.data_ptr(), _stream()), "devias_grad_sumsq_multi")


def clip_coef(partials, n_chunks, max_norm, out):
    _chk(partials, "clip_coef.partials", torch.float32); _chk(out, "clip_coef.out", torch.float32)
    _lib.check(_lib.load().devias_clip_coef(partials.data_ptr(), n_chunks, float(max_norm), out.data_ptr(), _stream()), "devias_clip_coef")


def adamw_multi(table, chunk_tensor, chunk_index, beta1, beta2, eps, grad_scale=1.0, grad_scale_dev=None):
    _chk(table, "adamw_multi.table", torch.uint8)
    _chk(chunk_tensor, "adamw_multi.chunk_tensor", torch.int32); _chk(chunk_index, "adamw_multi.chunk_index", torch.int32)
    if grad_scale_dev is not None:
        _chk(grad_scale_dev, "adamw_multi.grad_scale_dev", torch.float32)
    _lib.check(_lib.load().devias_adamw_multi(table.data_ptr(), chunk_tensor.data_ptr(), chunk_index.data_ptr(), chunk_tensor.numel(),
                                              beta1, beta2, eps, grad_scale, _p(grad_scale_dev), _stream()), "devias_adamw_multi")


def ema_factors(decay: float):
    """(decay, 1 - decay) as the two fp32 factors of the shadow update.  The second is `1. - decay` in double, rounded once: what torch computes for
    `(1. - decay) * model_v`; 1.0f - fl32(decay) differs from it in the last bit for 0.9999 and 0.99."""
    d = float(decay)
    if not 0.0 <= d <= 1.0:                    # a NaN fails the comparison too
        raise ValueError(f"model EMA decay must lie in [0, 1], got {decay!r}")
    return d, 1.0 - d


def adamw_ema_multi(table, chunk_tensor, chunk_index, beta1, beta2, eps, ema_decay, grad_scale=1.0, grad_scale_dev=None):
    """devias_adamw_ema_multi: adamw_multi, and the shadow weights of every record whose `ema` word is set, in the same launch."""
    _chk(table, "adamw_ema_multi.table", torch.uint8)
    _chk(chunk_tensor, "adamw_ema_multi.chunk_tensor", torch.int32); _chk(chunk_index, "adamw_ema_multi.chunk_index", torch.int32)
    if grad_scale_dev is not None:
        _chk(grad_scale_dev, "adamw_ema_multi.grad_scale_dev", torch.float32)
    d, o = ema_factors(ema_decay)
    _lib.check(_lib.load().devias_adamw_ema_multi(table.data_ptr(), chunk_tensor.data_ptr(), chunk_index.data_ptr(), chunk_tensor.numel(),
                                                  beta1, beta2, eps, grad_scale, _p(grad_scale_dev), d, o, _stream()), "devias_adamw_ema_multi")


def ema_multi(table, chunk_tensor, chunk_index, ema_decay):
    """devias_ema_multi: ema <- ema * decay + (1 - decay) * param for every record of the table whose `ema` word is set; reads nothing else of a record."""
    _chk(table, "ema_multi.table", torch.uint8)
    _chk(chunk_tensor, "ema_multi.chunk_tensor", torch.int32); _chk(chunk_index, "ema_multi.chunk_index", torch.int32)
    d, o = ema_factors(ema_decay)
    _lib.check(_lib.load().devias_ema_multi(table.data_ptr(), chunk_tensor.data_ptr(), chunk_index.data_ptr(), chunk_tensor.numel(), d, o, _stream()),
               "devias_ema_multi")


def _chk_ce(who, logits, target):
    _chk(logits, who + ".logits")
    _chk(target, who + ".target", torch.int64)
    if logits.dim() != 2 or target.shape != (logits.shape[0],) or logits.shape[0] == 0:
        raise ValueError(f"{who}: logits [B, C] and target [B] expected, got {tuple(logits.shape)} and {tuple(target.shape)}")
    return logits.shape


def softmax_ce_fwd(logits: torch.Tensor, target: torch.Tensor, smoothing: float = 0.0) -> torch.Tensor:
    """devias_softmax_ce_fwd: label-smoothing cross-entropy of logits [B, C] (fp32 or bf16) against int64 targets [B] -> fp32 loss [1]"""
    B, C = _chk_ce("softmax_ce_fwd", logits, target)
    lib = _lib.load()
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    ws = workspace(lib.devias_softmax_ce_workspace_bytes(B), logits.device)
    _lib.check(lib.devias_softmax_ce_fwd(logits.data_ptr(), target.data_ptr(), B, C, dt_code(logits.dtype), float(smoothing), loss.data_ptr(), ws.data_ptr(), _stream()),
               "devias_softmax_ce_fwd")
    return loss


def softmax_ce_bwd(logits: torch.Tensor, target: torch.Tensor, g_loss: torch.Tensor, smoothing: float = 0.0) -> torch.Tensor:
    """devias_softmax_ce_bwd: g_loss is the fp32 DEVICE scalar arriving on the loss"""
    B, C = _chk_ce("softmax_ce_bwd", logits, target)
    _chk(g_loss, "softmax_ce_bwd.g_loss", torch.float32)
    dz = torch.empty_like(logits)
    _lib.check(_lib.load().devias_softmax_ce_bwd(logits.data_ptr(), target.data_ptr(), B, C, dt_code(logits.dtype), float(smoothing), g_loss.data_ptr(), dz.data_ptr(), _stream()),
               "devias_softmax_ce_bwd")
    return dz
