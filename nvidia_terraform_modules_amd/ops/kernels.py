"""Python entry points for the gfx950 validation kernels (K1, K2, K3).

All functions launch on the current PyTorch stream and never synchronise, so
they can be captured in a ``torch.cuda.CUDAGraph`` (HIP graph on ROCm).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from ._lib import check, lib, lib_experimental, stream_handle
from .mcore import MCORE_FORMATS, mcore_format, mcore_format_id, mcore_shape_ok
from .mx import MX_BLOCK, mx_bits, mx_format_id, mx_shape_ok
from .mxq import MXQ_ROUNDING
from . import wave as _wave

BM = BN = 256
BK = 64


def gemm_shape_ok(m: int, n: int, k: int) -> bool:
    """True iff the 256x256x64 MFMA kernel tiles (M, N, K) exactly."""
    return m > 0 and n > 0 and k >= 2 * BK and m % BM == 0 and n % BN == 0 and k % BK == 0


def _require(t: torch.Tensor, name: str, dtype: torch.dtype) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be 2-D with unit inner stride")


GEMM_VARIANTS = {"default": 0, "pingpong8": 1, "pingpong8b": 4,
                 "pingpong8c": 5, "pingpong8cw": 10, "pingpong8cwe": 11,
                 "pingpong8cwn": 12, "pingpong8cwne": 13, "tile128": 15,
                 "tile256x128": 16, "tile160": 17, "tile256x160": 18, "tile128w4": 19,
                 "tile256x128w4": 20, "tile160w4": 21, "pingpong8cm": 22, "tile160x128": 23,
                 "tile128x160": 24, "tile128x256": 26, "pingpong8o": 25,
                 "pp8o_g128": 41, "pp8o_g128_nostore": 42, "pp8o_nostore": 43,
                 "pingpong8om": 47, "pingpong8od": 48, "pingpong8s": 49,
                 "pingpong8omd": 51, "pp192x256": 27, "pp256x192": 28,
                 "pp224x256": 29, "pp192x256s": 54, "pp256x192s": 55,
                 "dma4k_d3": 39}


# variants built only into libntm_experimental.so (tests / tools): never selected
# by the default dispatch, not present in the shipping library or Job binary
EXPERIMENTAL_VARIANTS = frozenset({"pingpong8", "pingpong8cw",
                                   "pingpong8cwe", "pingpong8cwn", "pingpong8cwne",
                                   "tile128w4", "tile256x128w4", "tile160w4",
                                   "pp8o_g128", "pp8o_g128_nostore", "pp8o_nostore",
                                   "pingpong8od", "pingpong8omd", "pingpong8om", "pp224x256"})

# (TM, TN) of the 4-wave tile kernels (gemm_bf16_t128.hpp)
TILE_SHAPES = {"tile128": (128, 128), "tile256x128": (256, 128), "tile160": (160, 160),
               "tile256x160": (256, 160), "tile128w4": (128, 128), "tile256x128w4": (256, 128),
               "tile160w4": (160, 160), "tile160x128": (160, 128), "tile128x160": (128, 160),
               "tile128x256": (128, 256)}


# wave-specialised tile kernels: any M, N % 4, K % 8 (edge tiles and the K tail masked)
MASKED_TILES = frozenset({"tile128", "tile256x128", "tile160", "tile160x128", "tile128x160",
                          "tile128x256"})


def _tile128_shape_ok(m: int, n: int, k: int, tm: int = 128, tn: int = 128,
                      masked: bool = False) -> bool:
    if masked:
        return m > 0 and n > 0 and n % 4 == 0 and k > 0 and k % 8 == 0
    return m > 0 and n > 0 and m % tm == 0 and n % tn == 0 and k >= 128 and k % 128 == 0


def k1_plan(m: int, n: int, k: int) -> tuple[int, str, str]:
    """The default dispatch's plan: (rows of C on the top kernel, top kernel,
    kernel of the remaining rows) - host-side, no GPU needed. The top kernel is
    the 256x256 one ("pingpong8c" / "pingpong8b") or a small tile; the rest is
    a small tile (ignored when the top takes every row). Raises ValueError
    when no combination of the K1 kernels tiles (M, N, K)."""
    top, tv, rest = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib().ntm_k1_plan(m, n, k, ctypes.byref(top), ctypes.byref(tv), ctypes.byref(rest))
    if rc != 0:
        raise ValueError(f"shape ({m},{n},{k}) not tiled by the K1 kernels")
    names = {v: kname for kname, v in GEMM_VARIANTS.items()}
    return top.value, names[tv.value], names[rest.value]


def k1_splitk_plan(m: int, n: int, k: int) -> tuple[int, str, str, int]:
    """The default dispatch's plan with split-K allowed (what ``gemm_bf16``
    runs): ``k1_plan``'s triple plus the number of K slices (1 = unsplit; > 1 =
    all of C on the top kernel, a masked small tile, in that many K slices)."""
    top, tv, rest, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib().ntm_k1_plan_splitk(m, n, k, ctypes.byref(top), ctypes.byref(tv),
                                  ctypes.byref(rest), ctypes.byref(sp))
    if rc != 0:
        raise ValueError(f"shape ({m},{n},{k}) not tiled by the K1 kernels")
    names = {v: kname for kname, v in GEMM_VARIANTS.items()}
    return top.value, names[tv.value], names[rest.value], sp.value


# (M, N, K) -> split-K workspace bytes of the default plan (0 = unsplit); a
# plan is validated once per shape
_DEFAULT_WS: dict[tuple[int, int, int], int] = {}


# (M, N, K) -> the stream-K variant of a stream-K default plan
_DEFAULT_SK: dict[tuple[int, int, int], str] = {}

# stream-K split mode on the 192-wide ping-pong tiles (gemm_bf16_skh.hpp)
SKH_VARIANTS = ("pp192x256s", "pp256x192s")
SK_VARIANTS = ("pingpong8s",) + SKH_VARIANTS


def k1_candidates(m: int, n: int, k: int, lda: int | None = None, ldb: int | None = None,
                  ldc: int | None = None) -> list[str]:
    """K1 builds worth timing on the box itself for an (m, n, k) GEMM: the default
    plan, plus the 4-wave ``dma4k_d3`` where its shape rule holds (M, N % 256,
    K % 128, K >= 256, rows 16-byte aligned, operands < 2 GiB). Under the power
    limit the two trade places box by box (profiles/r6_w4kh), so bench.py times
    both after its pre-warm and runs the faster (bench.select_k1)."""
    lda, ldb, ldc = lda or k, ldb or k, ldc or n
    ok = (m % 256 == 0 and n % 256 == 0 and k % 128 == 0 and k >= 256 and
          not (lda % 8 or ldb % 8 or ldc % 8) and m * lda * 2 < (1 << 31) and
          n * ldb * 2 < (1 << 31))
    return ["default", "dma4k_d3"] if ok else ["default"]


def set_plan_pp_tiles(on: bool = True, split: bool | None = None) -> None:
    """A/B knob for tools (tools/k1_ab.py pp-tiles): let the plan use the 192x256 /
    256x192 ping-pong tiles on all of C (``on``) and in stream-K split mode
    (``split``, default: as ``on``). The shipping plan has both. Process-wide."""
    split = on if split is None else split
    lib().ntm_set_plan_pp_tiles((1 if on else 0) | (2 if split else 0))
    _DEFAULT_WS.clear()
    _DEFAULT_SK.clear()
    _FP8_WS.clear()


def set_plan_splitk(margin: float = 0.0, long_slice_k: int = -1, fp8: bool = True) -> None:
    """A/B knob for tools (tools/k1_ab.py margin): the factor by which a split-K
    plan whose slices keep at least ``long_slice_k`` of K must beat the unsplit
    plan's predicted time (shorter slices, and any split against stream-K, keep
    1.1). margin <= 0 / long_slice_k < 0: the shipping 1.03 / 1024 (K1-fp8:
    1152 pairs of e4m3 values); margin 1.1 = round 4's plan. ``fp8`` False keeps
    K1-fp8's split-K at 1.1. Process-wide."""
    lib().ntm_set_plan_splitk(float(margin), int(long_slice_k), 1 if fp8 else 0)
    _DEFAULT_WS.clear()
    _DEFAULT_SK.clear()
    _FP8_WS.clear()


def set_plan_splitk_ragged(on: bool = True) -> None:
    """A/B knob for tools (tools/k1_ab.py margin): price long-slice split-K
    against the ragged-scaled unsplit time (the shipping plan, ``on``) or with
    round 4's rule. Process-wide; clears the per-shape plan memos here so no
    later default-dispatch call runs a stale decision."""
    lib().ntm_set_plan_splitk_ragged(1 if on else 0)
    _DEFAULT_WS.clear()
    _DEFAULT_SK.clear()
    _FP8_WS.clear()


def set_cus_override(cus: int = 0) -> None:
    """Host-only test knob: plan for ``cus`` CUs instead of the device's own (0 =
    the device's). Never set around real launches. Clears the plan memos."""
    lib().ntm_set_cus_override(int(cus))
    _DEFAULT_WS.clear()
    _DEFAULT_SK.clear()
    _FP8_WS.clear()


def skh_ws_bytes(variant: str, m: int, n: int, k: int) -> int:
    """Workspace of stream-K split mode on a 192-wide tile ("pp192x256s" /
    "pp256x192s") for (M, N, K) on this device; 0 when it does not serve it."""
    if m <= 0 or n <= 0 or k <= 0:
        return 0
    return int(lib().ntm_skh_ws_bytes(GEMM_VARIANTS[variant], m, n, k))


def _default_ws_bytes(m: int, n: int, k: int) -> int:
    """Split-K workspace bytes of the default plan; -1 when the plan is stream-K
    (its workspace is the per-stream cached one, ``_sk_workspace``)."""
    key = (m, n, k)
    wsb = _DEFAULT_WS.get(key)
    if wsb is None:
        _, top, _, sp = k1_splitk_plan(m, n, k)  # raises if no kernel serves the shape
        if top in SK_VARIANTS:
            # stream-K only where its own launch serves the shape (the plan and the
            # launch size for the same CUs; belt and braces): else the unsplit plan
            ok = (sk_ws_bytes(m, n, k) if top == "pingpong8s" else skh_ws_bytes(top, m, n, k)) > 0
            wsb = -1 if ok else 0
            if ok:
                _DEFAULT_SK[key] = top
        else:
            wsb = lib().ntm_splitk_ws_bytes(m, n, k, sp) if sp > 1 else 0
        _DEFAULT_WS[key] = wsb
    return wsb


def gemm_bf16(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
              variant: str = "default", splits: int = 1) -> torch.Tensor:
    """K1: ``out = a @ b.T`` in bf16 with fp32 accumulation on MFMA.

    a: [M, K] bf16, b: [N, K] bf16 (both K-contiguous), out: [M, N] bf16.
    ``variant``: "default" = the tile shape with the smallest predicted time
    (rounds of 256 CUs x tile area / efficiency, ``k1_plan``; split-K on a small
    tile when C cannot fill the chip and K is long, ``k1_splitk_plan``): "tile128" /
    "tile256x128" / "tile160" / "tile256x160" (128x128 / 256x128 / 160x160 /
    256x160 tiles, K % 128; the first three with 4 LDS-DMA producer + 4 MFMA
    consumer waves and masked edge tiles (any M, N % 4), 256x160 with 4 waves
    and whole tiles) for small, mid-size and ragged C,
    else "pingpong8c" when K % 128 == 0, else "pingpong8b" (8 waves, two per SIMD, staggered, balanced 8/4/8/4 LDS read
    schedule; 8c adds parity-alternating B buffers and a tail-free K loop),
    "pingpong8" (the first 12/4/8/0 schedule), "dma4k_d3" (4 waves x 128x128 per
    wave on 256x256 tiles, off the plan; bench.select_k1 times it against the plan
    on each box) - see validation/include.
    ``splits`` > 1 (masked tiles only): split-K into that many K slices, fp32
    partials in a workspace from PyTorch's allocator, then one reduction kernel.
    """
    _require(a, "a", torch.bfloat16)
    _require(b, "b", torch.bfloat16)
    m, k = a.shape
    n, kb = b.shape
    if k != kb:
        raise ValueError(f"K mismatch: a has {k}, b has {kb}")
    if variant in TILE_SHAPES:
        tm, tn = TILE_SHAPES[variant]
        if not _tile128_shape_ok(m, n, k, tm, tn, masked=variant in MASKED_TILES):
            raise ValueError(f"shape ({m},{n},{k}) not served by the {tm}x{tn} kernel "
                             "(masked tiles: N % 4, K % 8; others: whole tiles, K % 128)")
    elif variant == "default":
        _default_ws_bytes(m, n, k)  # the native plan is the one authority on what it serves
    elif variant in SKH_VARIANTS:
        if not skh_ws_bytes(variant, m, n, k):
            raise ValueError(f"shape ({m},{n},{k}) not served by {variant} (N % 8, K % 8, "
                             "K >= 128; at most half a round of its tiles, >= 2 K slices each)")
    elif variant in ("pingpong8s", "pingpong8s_rev", "pingpong8s_nopair"):  # stream-K
        if not sk_ws_bytes(m, n, k):
            raise ValueError(f"shape ({m},{n},{k}) not served by stream-K (N % 8, K % 8, K >= 128; "
                             "256x256 tiles: more than the CUs and not a multiple of them, or "
                             "few enough for >= 2 K slices per tile in one round)")
    elif variant in ("pingpong8cm", "pingpong8om", "pingpong8omd", "pp192x256", "pp256x192",
                     "pp224x256"):
        # 8-wave ping-pong tiles with masked edges (+ K tail)
        if not (m > 0 and n > 0 and n % 8 == 0 and k > 0 and k % 8 == 0):
            raise ValueError(f"shape ({m},{n},{k}) not served by {variant} (N % 8, K % 8)")
    elif not gemm_shape_ok(m, n, k):
        raise ValueError(f"shape ({m},{n},{k}) not tiled by the 256x256x64 kernel")
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    _require(out, "out", torch.bfloat16)
    if tuple(out.shape) != (m, n):
        raise ValueError("out has the wrong shape")
    if variant in ("pingpong8s", "pingpong8s_rev", "pingpong8s_nopair"):
        return _gemm_bf16_sk(a, b, out, rev=variant == "pingpong8s_rev",
                             nopair=variant == "pingpong8s_nopair")
    if variant in SKH_VARIANTS:
        return _gemm_bf16_sk(a, b, out, sk_variant=variant)
    if splits > 1:
        if variant not in MASKED_TILES:
            raise ValueError(f"split-K runs on {sorted(MASKED_TILES)}, not {variant}")
        ws_bytes = lib().ntm_splitk_ws_bytes(m, n, k, splits)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=a.device)
        rc = lib().ntm_gemm_bf16_splitk(
            GEMM_VARIANTS[variant], splits, a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
            a.stride(0), b.stride(0), out.stride(0), ws.data_ptr(), ws_bytes, stream_handle())
        check(rc, "ntm_gemm_bf16_splitk")
        return out
    if variant.startswith("knob"):            # experimental tuning sweep: "knob<N>"
        rc = lib_experimental().ntm_gemm_bf16_knob(
            int(variant[4:]), a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, a.stride(0),
            b.stride(0), out.stride(0), stream_handle())
        check(rc, "ntm_gemm_bf16_knob")
        return out
    if variant in EXPERIMENTAL_VARIANTS:
        rc = lib_experimental().ntm_gemm_bf16_experimental(
            GEMM_VARIANTS[variant], a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
            a.stride(0), b.stride(0), out.stride(0), stream_handle())
        check(rc, "ntm_gemm_bf16_experimental")
        return out
    if variant == "default" and _default_ws_bytes(m, n, k) < 0:
        return _gemm_bf16_sk(a, b, out, sk_variant=_DEFAULT_SK[(m, n, k)])
    if variant == "default" and _default_ws_bytes(m, n, k):
        wsb = _default_ws_bytes(m, n, k)
        ws = torch.empty((wsb + 3) // 4, dtype=torch.float32, device=a.device)
        rc = lib().ntm_gemm_bf16_ex(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
                                    a.stride(0), b.stride(0), out.stride(0), ws.data_ptr(), wsb,
                                    stream_handle())
        check(rc, "ntm_gemm_bf16_ex")
        return out
    rc = lib().ntm_gemm_bf16_variant(
        GEMM_VARIANTS[variant], a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
        a.stride(0), b.stride(0), out.stride(0), stream_handle())
    check(rc, "ntm_gemm_bf16")
    return out


def sk_ws_bytes(m: int, n: int, k: int) -> int:
    """Workspace of the stream-K build ("pingpong8s") for (M, N, K) on this
    device; 0 when it does not serve the shape. It serves two-round mode (more
    256x256 tiles than CUs, not a multiple of them) and split mode (each XCD's
    tiles fit its CUs at least twice: S >= 2 K slices per tile, one round)."""
    if m <= 0 or n <= 0 or k <= 0:
        return 0
    return int(lib().ntm_sk_ws_bytes(m, n, k))


# (device index, stream handle) -> the stream-K workspace of that stream: its
# counter block is zeroed once here and every completed launch leaves it zero,
# so calls on one stream reuse it with no memset dispatch
_SK_WS: dict[tuple[int, int], torch.Tensor] = {}


def _sk_workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    key = (dev.index if dev.index is not None else torch.cuda.current_device(),
           int(stream_handle() or 0))
    ws = _SK_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        _SK_WS[key] = ws
    return ws


def sk_xcc_error(device=None, clear: bool = True) -> int:
    """The XCD-placement error word of this stream's stream-K workspace
    (synchronises): 0 while every split tile's parts ran on one XCD, else the
    first violation a combiner saw (0x80000000 | mode << 28 | tile << 8 |
    combiner's XCC << 4 | other's XCC; gemm_bf16_sk.hpp). ``clear`` resets it."""
    dev = torch.device(device) if device is not None else torch.device(
        "cuda", torch.cuda.current_device())
    key = (dev.index if dev.index is not None else torch.cuda.current_device(),
           int(stream_handle() or 0))
    ws = _SK_WS.get(key)
    if ws is None:
        return 0
    i = lib().ntm_sk_error_word_index()
    word = ws.view(torch.int32)[i:i + 1]
    v = int(word.item()) & 0xFFFFFFFF
    if clear and v:
        word.zero_()
    return v


class SkPlacementError(RuntimeError):
    """A stream-K launch saw parts of a split tile on different XCDs: the
    write-through / L1-only-acquire protocol's invariant broke, so C is not
    trusted (gemm_bf16_sk.hpp). Raised by the default dispatch under
    ``NTM_SK_CHECK=1`` (bench.py sets it; the validation Job checks the word
    itself)."""


def sk_check_enabled() -> bool:
    """``NTM_SK_CHECK=1``: every stream-K launch of ``gemm_bf16`` reads (and
    clears) this stream's placement error word afterwards and raises
    :class:`SkPlacementError` when it is set. Costs one host sync per stream-K
    launch, so it is opt-in; the plain 256x256 / small-tile paths are unaffected."""
    import os

    return os.environ.get("NTM_SK_CHECK", "0") not in ("", "0")


def set_sk_fault_inject(on: bool = True) -> None:
    """Fault injection for the placement check (tests): while on, the head /
    slice 0 of every split tile claims a wrong XCC, so every stream-K launch
    sets the error word. Process-wide."""
    lib().ntm_set_sk_fault_inject(1 if on else 0)


def _sk_checked(dev: torch.device, out: torch.Tensor) -> torch.Tensor:
    if sk_check_enabled():
        w = sk_xcc_error(dev, clear=True)
        if w:
            raise SkPlacementError(
                f"stream-K placement violation (error word 0x{w:08x}: tile {(w >> 8) & 0xFFFF}, "
                f"combiner XCC {(w >> 4) & 0xF}, other XCC {w & 0xF}); C is not trusted")
    return out


def _gemm_bf16_sk(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, rev: bool = False,
                  nopair: bool = False, sk_variant: str = "pingpong8s") -> torch.Tensor:
    """Stream-K (gemm_bf16_sk.hpp; sk_variant "pp192x256s" / "pp256x192s": split
    mode on the 192-wide tiles, gemm_bf16_skh.hpp): fp32 partials of the split
    tiles and one counter per split in this stream's cached workspace
    (_sk_workspace). rev / nopair: experimental builds (segments reversed; split
    mode's S-partial protocol also at S = 2)."""
    m, k = a.shape
    n = b.shape[0]
    if sk_variant in SKH_VARIANTS:
        wsb = skh_ws_bytes(sk_variant, m, n, k)
        ws = _sk_workspace(a.device, wsb)
        rc = lib().ntm_gemm_bf16_skh(GEMM_VARIANTS[sk_variant], a.data_ptr(), b.data_ptr(),
                                     out.data_ptr(), m, n, k, a.stride(0), b.stride(0),
                                     out.stride(0), ws.data_ptr(), wsb, stream_handle())
        check(rc, "ntm_gemm_bf16_skh")
        return _sk_checked(a.device, out)
    wsb = sk_ws_bytes(m, n, k)
    ws = _sk_workspace(a.device, wsb)
    fn = (lib_experimental().ntm_gemm_bf16_sk_rev if rev else
          lib_experimental().ntm_gemm_bf16_sk_nopair if nopair else lib().ntm_gemm_bf16_sk)
    rc = fn(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, a.stride(0), b.stride(0),
            out.stride(0), ws.data_ptr(), wsb, stream_handle())
    check(rc, "ntm_gemm_bf16_sk")
    return _sk_checked(a.device, out)


def gemm_fp8_shape_ok(m: int, n: int, k: int) -> bool:
    return bool(lib().ntm_gemm_fp8_shape_ok(m, n, k))


# K1-fp8 variants: the 256x256 kernel and the wave-specialised tiles with the fp8 consumer
FP8_VARIANTS = ("default", "pingpong8c", "pingpong8o", "pingpong8cm", "tile128", "tile256x128",
                "tile160", "tile160x128", "tile128x160", "tile128x256")


def k1_fp8_plan(m: int, n: int, k: int) -> tuple[int, str, str]:
    """K1-fp8's default plan, as ``k1_plan`` (the same tile and row-split model
    with K counted in pairs of e4m3 values, over the tiles that have an fp8
    build). Raises ValueError for shapes the fp8 kernels do not serve."""
    top, tv, rest = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib().ntm_k1_fp8_plan(m, n, k, ctypes.byref(top), ctypes.byref(tv), ctypes.byref(rest))
    if rc != 0:
        raise ValueError(f"shape ({m},{n},{k}) not served by the fp8 kernels (N % 8, K % 16)")
    names = {v: kname for kname, v in GEMM_VARIANTS.items()}
    return top.value, names[tv.value], names[rest.value]


def k1_fp8_splitk_plan(m: int, n: int, k: int) -> tuple[int, str, str, int]:
    """K1-fp8's plan with split-K allowed (what ``gemm_fp8`` runs): ``k1_fp8_plan``'s
    triple plus the number of K slices (> 1: all of C on a masked small tile)."""
    top, tv, rest, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib().ntm_k1_fp8_plan_splitk(m, n, k, ctypes.byref(top), ctypes.byref(tv),
                                      ctypes.byref(rest), ctypes.byref(sp))
    if rc != 0:
        raise ValueError(f"shape ({m},{n},{k}) not served by the fp8 kernels (N % 8, K % 16)")
    names = {v: kname for kname, v in GEMM_VARIANTS.items()}
    return top.value, names[tv.value], names[rest.value], sp.value


_FP8_WS: dict[tuple[int, int, int], int] = {}


def _fp8_ws_bytes(m: int, n: int, k: int) -> int:
    key = (m, n, k)
    wsb = _FP8_WS.get(key)
    if wsb is None:
        sp = k1_fp8_splitk_plan(m, n, k)[3]
        wsb = lib().ntm_fp8_splitk_ws_bytes(m, n, k, sp) if sp > 1 else 0
        _FP8_WS[key] = wsb
    return wsb


def gemm_fp8(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
             knob: int = 0, variant: str = "default", splits: int = 1) -> torch.Tensor:
    """K1-fp8: ``out = a @ b.T`` with OCP e4m3 operands (``torch.float8_e4m3fn``),
    fp32 accumulation on the f8f6f4 MFMA (unit scales), bf16 output.

    a: [M, K], b: [N, K] (K-contiguous, rows 16-byte aligned), out: [M, N] bf16;
    N % 8, K % 16. ``variant``: "default" = ``k1_fp8_plan`` (256x256 tiles, or
    the wave-specialised 128x128 / 256x128 / 160x160 / 160x128 / 128x160 tiles
    and row splits where they fill the chip better); "pingpong8c" = the 256x256
    kernel (the bf16 default's schedule and LDS image, twice the MFMA rate per
    clock); "pingpong8o" = its persistent build with the C stores of one tile
    overlapping the next tile's K loop, on VGPR accumulators (whole 256x256
    tiles, K % 256, K >= 512; the plan's choice there); "tile*" = one tile shape. The default splits K over a masked small
    tile for skinny C with a long K (``k1_fp8_splitk_plan``; fp32 partials in a
    workspace from PyTorch's allocator); ``splits`` > 1 forces that on a "tile*"
    variant. ``knob`` != 0 selects an experimental schedule of the 256x256
    kernel (gemm_fp8_diag.hpp).
    """
    _require(a, "a", torch.float8_e4m3fn)
    _require(b, "b", torch.float8_e4m3fn)
    m, k = a.shape
    n, kb = b.shape
    if k != kb:
        raise ValueError(f"K mismatch: a has {k}, b has {kb}")
    if not gemm_fp8_shape_ok(m, n, k):
        raise ValueError(f"shape ({m},{n},{k}) not served by the fp8 kernel (N % 8, K % 16)")
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    _require(out, "out", torch.bfloat16)
    if tuple(out.shape) != (m, n):
        raise ValueError("out has the wrong shape")
    if knob:
        rc = lib_experimental().ntm_gemm_fp8_knob(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
                                     a.stride(0), b.stride(0), out.stride(0), int(knob),
                                     stream_handle())
    elif splits > 1 or (variant == "default" and _fp8_ws_bytes(m, n, k)):
        if splits > 1 and variant not in MASKED_TILES:
            raise ValueError(f"fp8 split-K runs on {sorted(MASKED_TILES)}, not {variant}")
        wsb = (lib().ntm_fp8_splitk_ws_bytes(m, n, k, splits) if splits > 1
               else _fp8_ws_bytes(m, n, k))
        ws = torch.empty((wsb + 3) // 4, dtype=torch.float32, device=a.device)
        if splits > 1:
            rc = lib().ntm_gemm_fp8_splitk(GEMM_VARIANTS[variant], splits, a.data_ptr(),
                                           b.data_ptr(), out.data_ptr(), m, n, k, a.stride(0),
                                           b.stride(0), out.stride(0), ws.data_ptr(), wsb,
                                           stream_handle())
        else:
            rc = lib().ntm_gemm_fp8_ex(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
                                       a.stride(0), b.stride(0), out.stride(0), ws.data_ptr(), wsb,
                                       stream_handle())
    else:
        if variant not in FP8_VARIANTS:
            raise ValueError(f"fp8 variant {variant!r} not in {FP8_VARIANTS}")
        rc = lib().ntm_gemm_fp8_variant(GEMM_VARIANTS[variant], a.data_ptr(), b.data_ptr(),
                                        out.data_ptr(), m, n, k, a.stride(0), b.stride(0),
                                        out.stride(0), stream_handle())
    check(rc, "ntm_gemm_fp8")
    return out


def gemm_bf16_rowsum(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
                     rowsum: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """K1 with the fused ABFT epilogue: returns ``(out, rowsum)`` where
    ``rowsum[m]`` is the fp32 sum over n of the accumulators of row m (the
    default kernel; ``rowsum`` is zeroed here, stream-ordered)."""
    _require(a, "a", torch.bfloat16)
    _require(b, "b", torch.bfloat16)
    m, k = a.shape
    n = b.shape[0]
    if b.shape[1] != k or not gemm_shape_ok(m, n, k):
        raise ValueError(f"shape ({m},{n},{k}) not tiled by the 256x256x64 kernel")
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    _require(out, "out", torch.bfloat16)
    if rowsum is None:
        rowsum = torch.empty(m, dtype=torch.float32, device=a.device)
    if rowsum.dtype != torch.float32 or rowsum.numel() < m or not rowsum.is_contiguous():
        raise ValueError("rowsum must be a contiguous fp32 tensor of >= M entries")
    rowsum.zero_()
    rc = lib().ntm_gemm_bf16_rowsum(a.data_ptr(), b.data_ptr(), out.data_ptr(), rowsum.data_ptr(),
                                    m, n, k, a.stride(0), b.stride(0), out.stride(0),
                                    stream_handle())
    check(rc, "ntm_gemm_bf16_rowsum")
    return out, rowsum


def gemm_fp8_rowsum(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
                    rowsum: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """K1-fp8 with the fused ABFT epilogue (the 256x256 fp8 build, M, N, K %
    256): returns ``(out, rowsum)`` as ``gemm_bf16_rowsum`` does; check it with
    ``abft_check`` on the same e4m3 operands."""
    _require(a, "a", torch.float8_e4m3fn)
    _require(b, "b", torch.float8_e4m3fn)
    m, k = a.shape
    n = b.shape[0]
    if b.shape[1] != k or m % 256 or n % 256 or k % 256:
        raise ValueError(f"shape ({m},{n},{k}) not tiled by the 256x256 fp8 kernel (M, N, K % 256)")
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    _require(out, "out", torch.bfloat16)
    if rowsum is None:
        rowsum = torch.empty(m, dtype=torch.float32, device=a.device)
    if rowsum.dtype != torch.float32 or rowsum.numel() < m or not rowsum.is_contiguous():
        raise ValueError("rowsum must be a contiguous fp32 tensor of >= M entries")
    rowsum.zero_()
    rc = lib().ntm_gemm_fp8_rowsum(a.data_ptr(), b.data_ptr(), out.data_ptr(), rowsum.data_ptr(),
                                   m, n, k, a.stride(0), b.stride(0), out.stride(0),
                                   stream_handle())
    check(rc, "ntm_gemm_fp8_rowsum")
    return out, rowsum


@dataclass
class AbftReport:
    rows: int
    bad_acc: int        # rows whose fused fp32 checksum disagrees with A . colsum(B)
    bad_store: int      # rows whose stored bf16 sum disagrees with the checksum
    max_rel_acc: float  # max |err| / ||C_m||_2
    max_rel_store: float

    @property
    def ok(self) -> bool:
        return self.bad_acc == 0 and self.bad_store == 0

    def as_dict(self) -> dict:
        return {"rows": self.rows, "bad_acc": self.bad_acc, "bad_store": self.bad_store,
                "max_rel_acc": self.max_rel_acc, "max_rel_store": self.max_rel_store,
                "ok": self.ok}


def abft_check(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor,
               rowsum: torch.Tensor) -> AbftReport:
    """K3: O(MK + NK + MN) ABFT check of ``c = a @ b.T`` against the fused
    row checksum (see aux_kernels.hpp); ``a`` / ``b`` bf16 (K1) or e4m3
    (K1-fp8). Synchronises to read the result."""
    m, k = a.shape
    n = b.shape[0]
    if c.shape != (m, n) or c.dtype != torch.bfloat16 or c.stride(1) != 1:
        raise ValueError("c must be [M, N] bf16 with unit inner stride")
    if a.dtype != b.dtype or a.dtype not in (torch.bfloat16, torch.float8_e4m3fn):
        raise ValueError("a and b must both be bf16 or both float8_e4m3fn")
    fn = lib().ntm_abft_check if a.dtype == torch.bfloat16 else lib().ntm_abft_check_fp8
    scratch = torch.empty(k, dtype=torch.float64, device=a.device)
    res = torch.empty(lib().ntm_abft_result_bytes(), dtype=torch.uint8, device=a.device)
    rc = fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), rowsum.data_ptr(),
            m, n, k, a.stride(0), b.stride(0), c.stride(0),
            scratch.data_ptr(), res.data_ptr(), stream_handle())
    check(rc, "ntm_abft_check")
    raw = res.cpu().numpy().tobytes()
    return AbftReport(
        rows=m, bad_acc=int.from_bytes(raw[0:8], "little"),
        bad_store=int.from_bytes(raw[8:16], "little"),
        max_rel_acc=ctypes.c_float.from_buffer_copy(raw[16:20]).value,
        max_rel_store=ctypes.c_float.from_buffer_copy(raw[20:24]).value)


def fill_uniform_(t: torch.Tensor, seed: int, scale: float = 1.0) -> torch.Tensor:
    """K3: fill a bf16 (or OCP e4m3, ``torch.float8_e4m3fn``) tensor in place
    with ``scale * U[-1, 1)`` (hash RNG; e4m3 rounds to nearest even)."""
    if t.dtype not in (torch.bfloat16, torch.float8_e4m3fn) or not t.is_cuda or \
            not t.is_contiguous():
        raise ValueError("fill_uniform_ needs a contiguous bf16 or float8_e4m3fn GPU tensor")
    fn = lib().ntm_fill_uniform_bf16 if t.dtype == torch.bfloat16 else lib().ntm_fill_uniform_e4m3
    rc = fn(t.data_ptr(), t.numel(), seed & (2**64 - 1), float(scale), stream_handle())
    check(rc, "ntm_fill_uniform")
    return t


def ref_gemm_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """K3: independent fp32-FMA reference ``a @ b.T`` (no MFMA, no hipBLASLt) for
    bf16 or OCP e4m3 operands (both of the same dtype)."""
    dt = a.dtype if a.dtype in (torch.bfloat16, torch.float8_e4m3fn) else torch.bfloat16
    _require(a, "a", dt)
    _require(b, "b", dt)
    m, k = a.shape
    n = b.shape[0]
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    fn = lib().ntm_ref_gemm_f32 if dt == torch.bfloat16 else lib().ntm_ref_gemm_f32_e4m3
    rc = fn(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, a.stride(0), b.stride(0),
            out.stride(0), stream_handle())
    check(rc, "ntm_ref_gemm_f32")
    return out


@dataclass
class VerifyReport:
    n: int
    bad: int
    max_abs_err: float
    rel_rms_err: float

    @property
    def ok(self) -> bool:
        return self.bad == 0

    def as_dict(self) -> dict:
        return {"n": self.n, "bad": self.bad, "max_abs_err": self.max_abs_err,
                "rel_rms_err": self.rel_rms_err, "ok": self.ok}


def verify_bf16(c: torch.Tensor, ref: torch.Tensor, atol: float, rtol: float) -> VerifyReport:
    """K3: element-wise ``|c - ref| <= atol + rtol*|ref|`` on device (synchronises)."""
    if c.dtype != torch.bfloat16 or ref.dtype != torch.float32:
        raise ValueError("verify_bf16 expects bf16 c and fp32 ref")
    if c.shape != ref.shape or not c.is_contiguous() or not ref.is_contiguous():
        raise ValueError("c and ref must be contiguous and of equal shape")
    nbytes = lib().ntm_verify_result_bytes()
    res = torch.zeros(nbytes, dtype=torch.uint8, device=c.device)
    rc = lib().ntm_verify_bf16(c.data_ptr(), ref.data_ptr(), c.numel(), float(atol), float(rtol),
                               res.data_ptr(), stream_handle())
    check(rc, "ntm_verify_bf16")
    raw = res.cpu().numpy().tobytes()
    bad = int.from_bytes(raw[0:8], "little")
    max_err = ctypes.c_float.from_buffer_copy(raw[8:12]).value
    sse = ctypes.c_double.from_buffer_copy(raw[16:24]).value
    ssr = ctypes.c_double.from_buffer_copy(raw[24:32]).value
    rel = (sse / ssr) ** 0.5 if ssr > 0 else float("inf")
    return VerifyReport(n=c.numel(), bad=bad, max_abs_err=max_err, rel_rms_err=rel)


# (unroll, policy, grid) of the block-tiled K2 kernels; policy bit0 =
# nontemporal loads, bit1 = nontemporal stores, bit2 = software-pipelined
# copy, bit3 = chunked; grid 0 = one block per tile (no grid-stride loop);
# unroll 1 = the original grid-stride kernel. Chosen by tools/hbm_sweep.py on
# MI355X, interleaved rounds (profiles/r2_k2/): (2, 7, 0) - 2 float4 per lane,
# nontemporal load + store, one 8 KiB tile per block, so the dispatcher keeps
# every CU's wave slots full - 6.37 TB/s at 2 GiB and 6.05 at 4 GiB, against
# 5.81 / 5.41 for the earlier (8, 7, 512) grid-stride pipeline and 4.97 / 4.78
# for a plain grid-stride float4 copy on the same box. Grids <= 1024 blocks
# (at most 16 waves per CU) were all that the round-1 sweeps tried.
#   read  (8, 1, 1024) 7.08-7.13 TB/s at 1 GiB (grid-stride 6.11)
STREAM_COPY_CONFIG: tuple[int, int, int] = (2, 7, 0)
STREAM_READ_CONFIG: tuple[int, int, int] = (8, 1, 1024)


def stream_copy(src: torch.Tensor, dst: torch.Tensor,
                config: tuple[int, int, int] | None | str = "tuned") -> None:
    """K2: float4 HBM copy of ``src`` into ``dst`` (byte-identical)."""
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() < nbytes or nbytes % 16:
        raise ValueError("stream_copy needs 16-byte multiple sizes and a large enough dst")
    cfg = STREAM_COPY_CONFIG if config == "tuned" else (config or (1, 0, 0))
    rc = lib().ntm_stream_copy_ex(src.data_ptr(), dst.data_ptr(), nbytes, *cfg, stream_handle())
    check(rc, "ntm_stream_copy")


def stream_read(src: torch.Tensor, sink: torch.Tensor,
                config: tuple[int, int, int] | None | str = "tuned") -> None:
    """K2: read-only HBM sweep of ``src`` (``sink`` only written on NaN/inf)."""
    nbytes = src.numel() * src.element_size()
    if nbytes % 16:
        raise ValueError("stream_read needs a 16-byte multiple size")
    cfg = STREAM_READ_CONFIG if config == "tuned" else (config or (1, 0, 0))
    rc = lib().ntm_stream_read_ex(src.data_ptr(), nbytes, sink.data_ptr(), *cfg,
                                  stream_handle())
    check(rc, "ntm_stream_read")


# K4: HBM pattern test (validation/include/ntm/hbm_pattern.hpp). Pattern ids of the C ABI.
HBM_PATTERN_ADDR = 0
HBM_PATTERN_HASH = 1
HBM_PATTERNS = {"addr": HBM_PATTERN_ADDR, "hash": HBM_PATTERN_HASH}


def hbm_pattern_id(pattern: int | str) -> int:
    p = HBM_PATTERNS.get(pattern.lower()) if isinstance(pattern, str) else pattern
    if p not in (HBM_PATTERN_ADDR, HBM_PATTERN_HASH):
        raise ValueError(f"unknown HBM pattern {pattern!r} (addr = 0, hash = 1)")
    return p


def hbm_pattern_check_args(t: torch.Tensor, base: int) -> int:
    """Bytes of ``t``; raises unless it is contiguous and size and base are 16-byte multiples."""
    nbytes = t.numel() * t.element_size()
    if not t.is_contiguous() or nbytes % 16 or base % 16 or base < 0 or base + nbytes > 2**64:
        raise ValueError("HBM pattern needs a contiguous tensor, bytes % 16 == 0 and base % 16 == 0")
    return nbytes


@dataclass
class HbmPatternReport:
    bad_words: int                 # 8-byte words that differ from the pattern
    bad_bits: int                  # OR of expected ^ got over them (64 bit)
    first_bad_offset: int | None   # smallest base + byte offset of one
    records: list                  # up to 4 of {"offset", "expected", "got"}

    @property
    def ok(self) -> bool:
        return self.bad_words == 0

    def as_dict(self) -> dict:
        return {"bad_words": self.bad_words, "bad_bits": self.bad_bits,
                "first_bad_offset": self.first_bad_offset, "records": self.records, "ok": self.ok}


def hbm_pattern_write(t: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                      base: int = 0) -> torch.Tensor:
    """K4: fill ``t``'s bytes with the ADDR (0) or HASH (1) pattern of the logical
    byte range ``base .. base + nbytes`` (formulas: validation/README.md)."""
    nbytes = hbm_pattern_check_args(t, base)
    if not t.is_cuda:
        raise ValueError("hbm_pattern_write needs a GPU tensor")
    rc = lib().ntm_hbm_pattern_write(t.data_ptr(), nbytes, base, hbm_pattern_id(pattern),
                                     seed & (2**64 - 1), int(bool(invert)), stream_handle())
    check(rc, "ntm_hbm_pattern_write")
    return t


def hbm_pattern_verify(t: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                       base: int = 0, invert_after: bool = False) -> HbmPatternReport:
    """K4: compare ``t``'s bytes with the pattern on the device (synchronises).
    ``invert_after`` also leaves the complement of the expected pattern in ``t``."""
    nbytes = hbm_pattern_check_args(t, base)
    if not t.is_cuda:
        raise ValueError("hbm_pattern_verify needs a GPU tensor")
    n = lib().ntm_hbm_pattern_result_bytes()
    res = torch.zeros(n // 8, dtype=torch.int64, device=t.device)
    res[2] = -1                                     # first_bad_offset: all ones
    rc = lib().ntm_hbm_pattern_verify(t.data_ptr(), nbytes, base, hbm_pattern_id(pattern),
                                      seed & (2**64 - 1), int(bool(invert)),
                                      int(bool(invert_after)), res.data_ptr(), stream_handle())
    check(rc, "ntm_hbm_pattern_verify")
    return read_pattern_result(res)


def new_pattern_result(device) -> torch.Tensor:
    """An initialised ntm::hbm::PatternResult (128 bytes) in device memory."""
    res = torch.zeros(lib().ntm_hbm_pattern_result_bytes() // 8, dtype=torch.int64, device=device)
    res[2] = -1                                     # first_bad_offset: all ones
    return res


def read_pattern_result(res: torch.Tensor) -> HbmPatternReport:
    """Copies the record to the host (synchronises) and decodes it."""
    raw = res.cpu().numpy().tobytes()
    u64 = lambda o: int.from_bytes(raw[o:o + 8], "little")  # noqa: E731
    bad = u64(0)
    nrec = min(int.from_bytes(raw[24:28], "little"), 4)
    recs = [{"offset": u64(32 + 24 * i), "expected": u64(40 + 24 * i), "got": u64(48 + 24 * i)}
            for i in range(nrec)]
    return HbmPatternReport(bad_words=bad, bad_bits=u64(8),
                            first_bad_offset=u64(16) if bad else None,
                            records=sorted(recs, key=lambda r: r["offset"]))


# K6: host-link (PCIe) check (validation/include/ntm/host_link.hpp, host_link_plan.hpp).
HOST_LINK_SLOT_BYTES = 64      # one chase slot: the next index (8 bytes) + padding
HOST_LINK_MAX_BLOCKS = 65536
HOST_LINK_UNROLLS = (1, 2, 4, 8)


def host_link_check_args(host: torch.Tensor, pattern, base: int, blocks, multiple: int = 16) -> int:
    """Bytes of ``host``; ValueError unless the pattern is known, size and base are
    ``multiple``-byte multiples and ``host`` is a contiguous pinned CPU tensor."""
    if pattern is not None:
        hbm_pattern_id(pattern)
    if not isinstance(host, torch.Tensor):
        raise ValueError("host link needs a pinned CPU tensor")
    nbytes = host.numel() * host.element_size()
    if nbytes % multiple or base % 16 or base < 0 or base + nbytes > 2**64:
        raise ValueError(f"host link needs bytes % {multiple} == 0 and base % 16 == 0")
    if blocks is not None and not 1 <= int(blocks) <= HOST_LINK_MAX_BLOCKS:
        raise ValueError(f"blocks must be in 1 .. {HOST_LINK_MAX_BLOCKS}")
    if host.is_cuda or not host.is_contiguous() or not host.is_pinned():
        raise ValueError("host link needs a contiguous pinned CPU tensor (is_pinned())")
    return nbytes


def host_link_default_blocks(pull: bool = False) -> int:
    """Blocks of the persistent push (``pull``: pull) kernel when ``blocks`` is None."""
    return lib().ntm_host_link_default_blocks(int(bool(pull)))


def host_link_tile_bytes(pull: bool = False) -> int:
    """Bytes a block moves per loop trip in the default push (``pull``: pull) build."""
    return lib().ntm_host_link_tile_bytes(int(bool(pull)))


def _host_link_knobs(config):
    if config is None:
        return None
    unroll, nt = config
    if unroll not in HOST_LINK_UNROLLS:
        raise ValueError(f"unroll must be one of {HOST_LINK_UNROLLS}")
    return int(unroll), int(bool(nt))


def host_link_push(host: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                   base: int = 0, blocks: int | None = None, config=None) -> torch.Tensor:
    """K6, device->host: the current GPU writes the ADDR (0) or HASH (1) pattern of the
    logical byte range ``base .. base + nbytes`` into the pinned CPU tensor ``host``
    (stream-ordered: synchronise before reading it on the host). ``config`` =
    (unroll, nontemporal) selects a sweep build instead of the measured default."""
    nbytes = host_link_check_args(host, pattern, base, blocks)
    knobs = _host_link_knobs(config)
    args = (host.data_ptr(), nbytes, base, hbm_pattern_id(pattern), seed & (2**64 - 1),
            int(bool(invert)), int(blocks or 0))
    if knobs is None:
        rc = lib().ntm_host_link_push(*args, stream_handle())
    else:
        rc = lib().ntm_host_link_push_ex(*args, *knobs, stream_handle())
    check(rc, "ntm_host_link_push")
    return host


def host_link_pull(host: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                   base: int = 0, dst: torch.Tensor | None = None, blocks: int | None = None,
                   config=None, result: torch.Tensor | None = None):
    """K6, host->device: the current GPU reads the pinned CPU tensor ``host`` and compares
    it with the pattern on the device (synchronises; returns the report). ``dst`` (a GPU
    tensor of the same size) also receives the bytes read. With ``result`` (from an earlier
    call's ``new_pattern_result``) the call only enqueues and returns None."""
    nbytes = host_link_check_args(host, pattern, base, blocks)
    knobs = _host_link_knobs(config)
    if dst is not None and (not dst.is_cuda or not dst.is_contiguous()
                            or dst.numel() * dst.element_size() != nbytes):
        raise ValueError("dst must be a contiguous GPU tensor of host's size")
    res = new_pattern_result(dst.device if dst is not None else "cuda") if result is None else result
    args = (host.data_ptr(), nbytes, base, hbm_pattern_id(pattern), seed & (2**64 - 1),
            int(bool(invert)), dst.data_ptr() if dst is not None else None, int(blocks or 0))
    if knobs is None:
        rc = lib().ntm_host_link_pull(*args, res.data_ptr(), stream_handle())
    else:
        rc = lib().ntm_host_link_pull_ex(*args, *knobs, res.data_ptr(), stream_handle())
    check(rc, "ntm_host_link_pull")
    return read_pattern_result(res) if result is None else None


def host_link_chase(host: torch.Tensor, hops: int, start: int = 0) -> tuple[int, float]:
    """K6, read round trip: one lane follows the chain in the pinned CPU tensor ``host``
    (64-byte slots, the first 8 bytes of slot i = the index of the next slot;
    ``reference.host_link_chase_table``) for ``hops`` dependent loads from slot ``start``.
    Returns (final slot index, nanoseconds per hop); synchronises. An index that is no
    slot ends the walk early and raises."""
    nbytes = host_link_check_args(host, None, 0, None, multiple=HOST_LINK_SLOT_BYTES)
    nslots = nbytes // HOST_LINK_SLOT_BYTES
    if nslots < 1 or not 0 <= start < nslots or not 1 <= hops < 2**32:
        raise ValueError("host_link_chase needs >= 1 slot, 0 <= start < slots and 1 <= hops < 2^32")
    dev = torch.cuda.current_device()
    khz = lib().ntm_host_link_clock_khz(dev)
    if khz <= 0:
        raise RuntimeError("cannot read the device's wall clock rate")
    out = torch.zeros(3, dtype=torch.int64, device=torch.device("cuda", dev))
    rc = lib().ntm_host_link_chase(host.data_ptr(), nslots, start, hops, out.data_ptr(), stream_handle())
    check(rc, "ntm_host_link_chase")
    final, ticks, done = (int(v) for v in out.cpu())
    if done != hops:
        raise RuntimeError(f"host_link_chase read {final}, not a slot index, after {done} hops")
    return final, ticks / khz * 1e6 / hops


# K7: MX block-scaled matrix check (validation/include/ntm/mx_gemm.hpp, mx_plan.hpp). The
# host side (formats, packing, generators, bound, exact reference) is numpy: ops/mx.py.
@dataclass
class MxCompareReport:
    count: int                 # 32-bit words that differ
    first_index: int | None    # smallest flat index of one
    expected: int | None       # the words at first_index
    got: int | None

    @property
    def ok(self) -> bool:
        return self.count == 0

    def as_dict(self) -> dict:
        return {"count": self.count, "first_index": self.first_index, "expected": self.expected,
                "got": self.got, "ok": self.ok}


def mx_check_args(a, b, sa, sb, fmt, out=None, need_cuda: bool = True) -> tuple[int, int, int, int]:
    """(format code, M, N, K) of one MX product; ValueError unless a / b / sa / sb are
    contiguous uint8 matrices (on one GPU when ``need_cuda``) whose shapes agree, with M, N
    and K multiples of 128, and ``out`` (if given) a contiguous fp32 [M, N] beside them."""
    f = mx_format_id(fmt)
    bits = mx_bits(f)
    for name, t in (("a", a), ("b", b), ("sa", sa), ("sb", sb)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"MX check: {name} must be a contiguous 2-D uint8 tensor")
        if need_cuda and not t.is_cuda:
            raise ValueError("MX check needs GPU tensors")
        if t.device != a.device:
            raise ValueError("MX check: all tensors must be on one device")
    M, N = a.shape[0], b.shape[0]
    K = a.shape[1] * 8 // bits
    if (a.shape[1] * 8) % bits or b.shape[1] != a.shape[1] or not mx_shape_ok(M, N, K):
        raise ValueError("MX check needs a [M, K*bits/8], b [N, K*bits/8] with M, N, K multiples of 128")
    if tuple(sa.shape) != (M, K // MX_BLOCK) or tuple(sb.shape) != (N, K // MX_BLOCK):
        raise ValueError("MX check needs sa [M, K/32] and sb [N, K/32]")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32
                            or tuple(out.shape) != (M, N) or not out.is_contiguous()
                            or out.device != a.device):
        raise ValueError("MX check: out must be a contiguous fp32 [M, N] tensor on the operands' device")
    return f, M, N, K


def _mx_product(entry: str, a, b, sa, sb, fmt, out):
    f, M, N, K = mx_check_args(a, b, sa, sb, fmt, out)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = getattr(lib(), entry)(f, a.data_ptr(), b.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                   out.data_ptr(), M, N, K, stream_handle())
    check(rc, entry)
    return out


def mx_gemm(a: torch.Tensor, b: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, fmt,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """K7: C [M, N] fp32 = A @ B.T on the block-scaled f8f6f4 matrix instruction. ``a`` / ``b``:
    packed uint8 rows of format ``fmt`` (``mx_pack``), ``sa`` / ``sb``: E8M0 scale bytes
    [rows, K/32]. M, N and K must be multiples of 128. Stream-ordered."""
    return _mx_product("ntm_mx_gemm", a, b, sa, sb, fmt, out)


def mx_reference_gpu(a: torch.Tensor, b: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, fmt,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """K7: the same product without the matrix cores (integer decode, ldexpf, an fp32 FMA
    chain in k order); exact under ``mx_dense_exact``. Stream-ordered."""
    return _mx_product("ntm_mx_reference", a, b, sa, sb, fmt, out)


def mx_compare(expected: torch.Tensor, got: torch.Tensor) -> MxCompareReport:
    """K7: bitwise compare of two GPU tensors of 32-bit elements on the device
    (synchronises)."""
    for t in (expected, got):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("mx_compare needs GPU tensors")
        if t.element_size() != 4 or not t.is_contiguous():
            raise ValueError("mx_compare needs contiguous tensors of 32-bit elements")
    if expected.numel() != got.numel() or expected.device != got.device:
        raise ValueError("mx_compare needs two tensors of one size on one device")
    res = torch.zeros(lib().ntm_mx_mismatch_bytes() // 8, dtype=torch.int64, device=got.device)
    res[1] = -1                                     # first_index: all ones
    with torch.cuda.device(got.device):
        rc = lib().ntm_mx_compare(expected.data_ptr(), got.data_ptr(), expected.numel(),
                                  res.data_ptr(), stream_handle())
    check(rc, "ntm_mx_compare")
    raw = res.cpu().numpy().tobytes()
    count = int.from_bytes(raw[0:8], "little")
    if count == 0:
        return MxCompareReport(0, None, None, None)
    return MxCompareReport(count, int.from_bytes(raw[8:16], "little"),
                           int.from_bytes(raw[16:20], "little"), int.from_bytes(raw[20:24], "little"))


# K11: MX quantise / dequantise on the device (validation/include/ntm/mxq.hpp, mxq_plan.hpp).
# The host side (rules, generators) is numpy: ops/mxq.py.
_MXQ_DTYPE = {torch.float32: 0, torch.bfloat16: 1}


def _mxq_rounding(rounding, seed) -> tuple[int, int]:
    if rounding not in MXQ_ROUNDING:
        raise ValueError(f"rounding must be one of {MXQ_ROUNDING}")
    if rounding == "stochastic" and seed is None:
        raise ValueError("stochastic rounding needs a seed")
    return MXQ_ROUNDING.index(rounding), int(seed or 0) & (2**64 - 1)


def _mxq_source(x) -> tuple[int, int, int]:
    """(R, K, ldx) of a 2-D fp32 / bf16 GPU tensor whose rows are contiguous."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _MXQ_DTYPE or x.dim() != 2 or not x.is_cuda:
        raise ValueError("MX quantise needs a 2-D fp32 or bf16 GPU tensor")
    if x.shape[1] and x.stride(1) != 1:
        raise ValueError("MX quantise needs rows of contiguous elements")
    return x.shape[0], x.shape[1], x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


def _mxq_down(entry: str, x, fmt, scales, packed, rounding="rne", seed=None):
    f = mx_format_id(fmt)
    R, K, ldx = _mxq_source(x)
    given = entry.endswith("cvt")
    KB = K // MX_BLOCK
    if given:
        if (not isinstance(scales, torch.Tensor) or scales.dtype != torch.uint8 or tuple(scales.shape) != (R, KB)
                or not scales.is_contiguous() or scales.device != x.device):
            raise ValueError("mxq_cvt needs contiguous uint8 scales [R, K/32] on the source's device")
    elif scales is None:
        scales = torch.empty((R, max(KB, 0)), dtype=torch.uint8, device=x.device)
    if packed is None:
        packed = torch.empty((R, K * mx_bits(f) // 8), dtype=torch.uint8, device=x.device)
    args = [f, _MXQ_DTYPE[x.dtype], x.data_ptr()]
    args += [scales.data_ptr(), packed.data_ptr()] if given else [packed.data_ptr(), scales.data_ptr()]
    args += [R, K, ldx]
    if "reference" not in entry:
        args += list(_mxq_rounding(rounding, seed))
    elif rounding != "rne":
        raise ValueError("the reference kernels round to nearest even only")
    with torch.cuda.device(x.device):
        rc = getattr(lib(), entry)(*args, stream_handle())
    check(rc, entry)
    return packed, scales


def mx_quantize(x: torch.Tensor, fmt, rounding: str = "rne", seed: int | None = None, packed=None, scales=None):
    """K11: quantise ``x`` [R, K] (fp32 or bf16, K a multiple of 32, row stride >= K) to MX format
    ``fmt`` on the device with the scaled-conversion instructions -> (packed uint8 [R, K*bits/8],
    scales uint8 [R, K/32]) laid out as ``mx_gemm`` takes them. OCP MX v1.0: scale byte =
    clamp(floor(log2(amax)) - emax_elem + 127, 1, 254), 127 for a zero block; elements round to
    nearest even and saturate. ``rounding="stochastic"`` (e2m1, e4m3) needs ``seed``: the random
    word of element i is ``hash32(seed, 11, i)``. Not judged: Inf / NaN inputs saturate, fp32
    denormals are whatever the instruction makes of them. Stream-ordered."""
    return _mxq_down("ntm_mxq_quantize", x, fmt, scales, packed, rounding, seed)


def mx_quantize_reference_gpu(x: torch.Tensor, fmt, packed=None, scales=None):
    """K11: ``mx_quantize`` by integer bit arithmetic only (no conversion instruction)."""
    return _mxq_down("ntm_mxq_reference_quantize", x, fmt, scales, packed)


def mxq_cvt(x: torch.Tensor, scales: torch.Tensor, fmt, rounding: str = "rne", seed: int | None = None,
            reference: bool = False, packed=None) -> torch.Tensor:
    """K11: the element-level form: convert ``x`` [R, K] with the given scale bytes [R, K/32]
    (1 .. 254) -> packed codes. ``reference=True`` runs the integer kernel."""
    return _mxq_down("ntm_mxq_reference_cvt" if reference else "ntm_mxq_cvt", x, fmt, scales, packed, rounding, seed)[0]


def _mxq_up(entry: str, packed, scales, fmt, dtype, out):
    f = mx_format_id(fmt)
    bits = mx_bits(f)
    for name, t in (("packed", packed), ("scales", scales)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"MX dequantise: {name} must be a contiguous 2-D uint8 GPU tensor")
    if dtype not in _MXQ_DTYPE:
        raise ValueError("MX dequantise: dtype must be torch.float32 or torch.bfloat16")
    R, K = packed.shape[0], packed.shape[1] * 8 // bits
    if (packed.shape[1] * 8) % bits or tuple(scales.shape) != (R, K // MX_BLOCK) or scales.device != packed.device:
        raise ValueError("MX dequantise needs packed [R, K*bits/8] and scales [R, K/32] on one device")
    if out is None:
        out = torch.empty((R, K), dtype=dtype, device=packed.device)
    elif out.dtype != dtype or out.dim() != 2 or tuple(out.shape) != (R, K) or out.stride(1) != 1 or out.device != packed.device:
        raise ValueError("MX dequantise: out must be [R, K] of the asked dtype with contiguous rows")
    ldx = out.stride(0) if R > 1 else max(out.stride(0), K)
    with torch.cuda.device(packed.device):
        rc = getattr(lib(), entry)(f, _MXQ_DTYPE[dtype], packed.data_ptr(), scales.data_ptr(), out.data_ptr(), R, K, ldx,
                                   stream_handle())
    check(rc, entry)
    return out


def mx_dequantize(packed: torch.Tensor, scales: torch.Tensor, fmt, dtype=torch.float32, out=None) -> torch.Tensor:
    """K11: the inverse of ``mx_quantize`` on the device: code value * 2^(byte - 127) as fp32, or
    that rounded to nearest even as bf16. Not judged: results outside the normal fp32 range and
    the NaN / Inf codes of e4m3 / e5m2 come out as the instruction makes them. Stream-ordered."""
    return _mxq_up("ntm_mxq_dequantize", packed, scales, fmt, dtype, out)


def mx_dequantize_reference_gpu(packed: torch.Tensor, scales: torch.Tensor, fmt, dtype=torch.float32, out=None):
    """K11: ``mx_dequantize`` by integer bit arithmetic only."""
    return _mxq_up("ntm_mxq_reference_dequantize", packed, scales, fmt, dtype, out)


def mxq_to_device(bits, device, bf16: bool = False) -> torch.Tensor:
    """fp32 bit patterns (numpy uint32, any strides kept as a dense copy) -> an fp32 GPU tensor,
    or with ``bf16`` their upper halves as a bf16 tensor."""
    import numpy as np
    b = np.ascontiguousarray(bits, dtype=np.uint32)
    if bf16:
        return torch.from_numpy((b >> np.uint32(16)).astype(np.uint16).view(np.int16)).to(device).view(torch.bfloat16)
    return torch.from_numpy(b.view(np.int32)).to(device).view(torch.float32)


# K10: fp64 / fp32 / fp16 / int8 / 2:4-sparse matrix-core check (validation/include/ntm/mcore.hpp,
# mcore_plan.hpp). The host side (format table, packers, generators, bound, exact reference) is
# numpy: ops/mcore.py.
@dataclass
class McoreCompareReport:
    count: int                 # result words that differ
    first_index: int | None    # smallest flat index of one
    expected: int | None       # the words at first_index
    got: int | None

    @property
    def ok(self) -> bool:
        return self.count == 0

    def as_dict(self) -> dict:
        return {"count": self.count, "first_index": self.first_index, "expected": self.expected,
                "got": self.got, "ok": self.ok}


_MCORE_TORCH = {"f64": (torch.float64,), "f32": (torch.float32,), "f16": (torch.float16,), "i8": (torch.int8,),
                "sp_bf16": (torch.bfloat16, torch.int16), "sp_i8": (torch.int8,)}
_MCORE_ACC = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float32, "i8": torch.int32,
              "sp_bf16": torch.float32, "sp_i8": torch.int32}


def mcore_to_device(inputs: dict, device) -> dict:
    """``mcore_make_inputs``' numpy arrays as GPU tensors (bf16 bit patterns become bfloat16)."""
    import numpy as np

    def t(x):
        if x is None:
            return None
        if x.dtype == np.uint16:
            return torch.from_numpy(x.view(np.int16).copy()).to(device).view(torch.bfloat16)
        return torch.from_numpy(x.copy()).to(device)
    return {**inputs, "a": t(inputs["a"]), "ai": t(inputs["ai"]), "b": t(inputs["b"])}


def mcore_check_args(a, b, fmt, ai=None, out=None, need_cuda: bool = True) -> tuple[int, int, int, int]:
    """(format code, M, N, K) of one matrix-core product; ValueError unless a / b (/ ai) are
    contiguous matrices of the format's element type (on one GPU when ``need_cuda``) whose
    shapes agree, with M, N and K multiples of 128, and ``out`` (if given) a contiguous [M, N]
    tensor of the accumulator's type beside them."""
    f = mcore_format(fmt)
    name = f["name"]
    tensors = [("a", a, _MCORE_TORCH[name]), ("b", b, _MCORE_TORCH[name])]
    if f["sparse"]:
        tensors.append(("ai", ai, (torch.uint8,)))
    for label, t, dtypes in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"matrix-core check: {label} must be a contiguous 2-D tensor of {dtypes[0]}")
        if need_cuda and not t.is_cuda:
            raise ValueError("matrix-core check needs GPU tensors")
        if t.device != a.device:
            raise ValueError("matrix-core check: all tensors must be on one device")
    M, N, K = a.shape[0], b.shape[0], b.shape[1]
    if a.shape[1] != (K // 2 if f["sparse"] else K) or not mcore_shape_ok(M, N, K):
        raise ValueError("matrix-core check needs a [M, K] (sparse: [M, K/2]) and b [N, K] with M, N, K multiples of 128")
    if f["sparse"] and tuple(ai.shape) != (M, K // 4):
        raise ValueError("matrix-core check needs ai [M, K/4]")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != _MCORE_ACC[name]
                            or tuple(out.shape) != (M, N) or not out.is_contiguous() or out.device != a.device):
        raise ValueError(f"matrix-core check: out must be a contiguous {_MCORE_ACC[name]} [M, N] tensor on the operands' device")
    return mcore_format_id(fmt), M, N, K


def _mcore_product(entry: str, a, b, fmt, ai, out):
    f, M, N, K = mcore_check_args(a, b, fmt, ai, out)
    if out is None:
        out = torch.empty((M, N), dtype=_MCORE_ACC[MCORE_FORMATS[f]], device=a.device)
    with torch.cuda.device(a.device):
        rc = getattr(lib(), entry)(f, a.data_ptr(), ai.data_ptr() if ai is not None else None, b.data_ptr(),
                                   out.data_ptr(), M, N, K, stream_handle())
    check(rc, entry)
    return out


def mcore_gemm(a: torch.Tensor, b: torch.Tensor, fmt, ai: torch.Tensor | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """K10: C [M, N] = A @ B.T on the format's matrix instruction (``MCORE_FORMATS``): fp64,
    fp32, fp16 or int8 MFMA, or a 2:4-sparse SMFMAC with ``a`` = Ac [M, K/2] and ``ai`` [M, K/4].
    M, N and K must be multiples of 128. Stream-ordered."""
    return _mcore_product("ntm_mcore_gemm", a, b, fmt, ai, out)


def mcore_reference_gpu(a: torch.Tensor, b: torch.Tensor, fmt, ai: torch.Tensor | None = None,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """K10: the same product with no matrix instruction (one thread per element, an fma or
    integer multiply-add loop in k order); exact under ``mcore_exact``. Stream-ordered."""
    return _mcore_product("ntm_mcore_reference", a, b, fmt, ai, out)


def mcore_compare(expected: torch.Tensor, got: torch.Tensor) -> McoreCompareReport:
    """K10: bitwise compare of two GPU tensors of 4- or 8-byte elements on the device
    (synchronises)."""
    for t in (expected, got):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("mcore_compare needs GPU tensors")
        if t.element_size() not in (4, 8) or not t.is_contiguous():
            raise ValueError("mcore_compare needs contiguous tensors of 4- or 8-byte elements")
    if expected.numel() != got.numel() or expected.device != got.device or expected.element_size() != got.element_size():
        raise ValueError("mcore_compare needs two tensors of one size and word width on one device")
    res = torch.zeros(lib().ntm_mcore_mismatch_bytes() // 8, dtype=torch.int64, device=got.device)
    res[1] = -1                                     # first_index: all ones
    with torch.cuda.device(got.device):
        rc = lib().ntm_mcore_compare(expected.data_ptr(), got.data_ptr(), expected.numel(), expected.element_size(),
                                     res.data_ptr(), stream_handle())
    check(rc, "ntm_mcore_compare")
    raw = res.cpu().numpy().tobytes()
    count = int.from_bytes(raw[0:8], "little")
    if count == 0:
        return McoreCompareReport(0, None, None, None)
    return McoreCompareReport(count, int.from_bytes(raw[8:16], "little"), int.from_bytes(raw[16:24], "little"),
                              int.from_bytes(raw[24:32], "little"))


# K5: per-CU compute sweep (validation/include/ntm/cu_sweep.hpp, cu_sweep_plan.hpp).
CU_SWEEP_SUBTESTS = ("lds", "valu", "mfma_bf16", "mfma_fp8")
CU_SWEEP_MAGIC = 0x4B355357
CU_SWEEP_MAX_LAUNCHES = 8      # cap of the coverage loop
CU_SWEEP_GRID_PER_CU = 4       # workgroups per CU and launch
CU_SWEEP_FAULT_OFF = 0xFFFFFFFF


def cu_sweep_record_dtype():
    """numpy dtype of the 64-byte per-workgroup record (ntm::cus::Record)."""
    import numpy as np
    dt = np.dtype([("hw_id", "<u4"), ("xcc_id", "<u4"), ("simd", "u1", (4,)), ("magic", "<u4"),
                   ("wg", "<u4"), ("bad", "<u4", (4,)), ("first", "<u4"), ("first_round", "<u4"),
                   ("first_elem", "<u4"), ("expected", "<u8"), ("got", "<u8")])
    assert dt.itemsize == 64
    return dt


def cu_sweep_subtest_id(subtest: int | str) -> int:
    s = CU_SWEEP_SUBTESTS.index(subtest) if subtest in CU_SWEEP_SUBTESTS else subtest
    if s not in (0, 1, 2, 3):
        raise ValueError(f"unknown CU sweep sub-test {subtest!r} {CU_SWEEP_SUBTESTS}")
    return s


def cu_sweep_max_lds_bytes(device=None) -> int:
    """The per-block LDS maximum the runtime reports for ``device``: the default ``lds_bytes``."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = lib().ntm_cu_sweep_max_lds_bytes(dev.index if dev.index is not None else torch.cuda.current_device())
    if n <= 0:
        raise RuntimeError("cannot read the device's per-block LDS maximum")
    return n


def cu_sweep(device=None, iters: int = 2, lds_bytes: int | None = None, grid: int | None = None,
             seed: int = 0, fault_key: int | None = None, fault_subtest: int | str | None = None):
    """K5: one launch of the per-CU compute sweep; returns the workgroups' records (a numpy
    structured array, ``cu_sweep_record_dtype``). ``lds_bytes`` defaults to the device's
    per-block maximum, ``grid`` to 4 workgroups per CU. ``fault_key`` (a packed CU key of
    ``cu_sweep_decode``) makes the workgroups on that CU flip one bit of one computed value of
    ``fault_subtest`` before the compare. Expected values come from ``reference.cu_sweep_expected``."""
    import numpy as np
    from .reference import cu_sweep_expected

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("cu_sweep needs a GPU device")
    limit = cu_sweep_max_lds_bytes(dev)
    lds_bytes = limit if lds_bytes is None else int(lds_bytes)
    if lds_bytes < 16 or lds_bytes % 16 or lds_bytes > limit:
        raise ValueError(f"lds_bytes must be a multiple of 16 in 16 .. {limit}, got {lds_bytes}")
    if grid is None:
        grid = CU_SWEEP_GRID_PER_CU * torch.cuda.get_device_properties(dev).multi_processor_count
    if grid < 1 or not 1 <= iters <= 1024:
        raise ValueError("cu_sweep needs grid >= 1 and 1 <= iters <= 1024")
    if (fault_key is None) != (fault_subtest is None):
        raise ValueError("fault_key and fault_subtest go together")
    key = CU_SWEEP_FAULT_OFF if fault_key is None else int(fault_key) & 0xFFFFFFFF
    sub = 0 if fault_subtest is None else cu_sweep_subtest_id(fault_subtest)
    table = cu_sweep_expected(iters, seed, lds_bytes)["table"]
    with torch.cuda.device(dev):
        exp = torch.from_numpy(table.view(np.int32).copy()).to(dev)
        rec = torch.empty(grid * 16, dtype=torch.int32, device=dev)
        rc = lib().ntm_cu_sweep_launch(rec.data_ptr(), exp.data_ptr(), grid, iters, lds_bytes,
                                       seed & 0xFFFFFFFF, key, sub, stream_handle())
        check(rc, "ntm_cu_sweep_launch")
        raw = rec.cpu().numpy()            # synchronises; exp stays alive until here
    return raw.view(cu_sweep_record_dtype()).copy()


def cu_sweep_decode(hw_id: int, xcc_id: int) -> dict:
    """HW_REG_HW_ID / HW_REG_XCC_ID words -> xcd, se, sh, cu, simd and the packed CU key."""
    out = (ctypes.c_uint * 6)()
    lib().ntm_cu_sweep_decode(int(hw_id) & 0xFFFFFFFF, int(xcc_id) & 0xFFFFFFFF, out)
    return dict(zip(("xcd", "se", "sh", "cu", "simd", "key"), (int(v) for v in out)))


def cu_sweep_summarize(records, cus: int, launches: int = 1, gpu: int = 0) -> dict:
    """Aggregate records (of one or more launches, concatenated) per CU: coverage, workgroups
    per CU, the bad CUs with their first mismatch, ``ok`` and the Job's failure ``message``."""
    import json

    import numpy as np
    recs = np.ascontiguousarray(records, dtype=cu_sweep_record_dtype())
    buf = recs.tobytes()
    n = lib().ntm_cu_sweep_summarize(buf, len(recs), cus, launches, gpu, None, 0)
    out = ctypes.create_string_buffer(n + 1)
    lib().ntm_cu_sweep_summarize(buf, len(recs), cus, launches, gpu, out, n + 1)
    return json.loads(out.value.decode())


# K8: per-XCD sweep (validation/include/ntm/xcd_sweep.hpp, xcd_sweep_plan.hpp).
XCD_SWEEP_MAGIC = 0x4B385843
XCD_SWEEP_LEVELS = ("l2", "mall", "hbm", "mfma")
XCD_SWEEP_MODES = ("alone", "together")
XCD_SWEEP_TILE_BYTES = 64 * 1024
XCD_SWEEP_CUS_PER_XCD = 32
XCD_SWEEP_MFMA_PER_BATCH = 512     # per wave; a workgroup is 4 waves


def xcd_sweep_record_dtype():
    """numpy dtype of the 64-byte per-workgroup record (ntm::xcs::Record)."""
    import numpy as np
    dt = np.dtype([("magic", "<u4"), ("hw_id", "<u4"), ("xcc_id", "<u4"), ("wg", "<u4"),
                   ("tiles", "<u4"), ("bad_words", "<u4"), ("rt_ticks", "<u4"), ("cycles", "<u4"),
                   ("rt_start", "<u8"), ("first_off", "<u8"), ("expected", "<u8"), ("got", "<u8")])
    assert dt.itemsize == 64
    return dt


def xcd_sweep_gated(level: int | str, mode: int | str) -> bool:
    """Whether the Job's rate rule judges this cell (mall / together and hbm / together are
    reported only: profiles/xcd_sweep/README.md)."""
    lv = XCD_SWEEP_LEVELS.index(level) if level in XCD_SWEEP_LEVELS else level
    md = XCD_SWEEP_MODES.index(mode) if mode in XCD_SWEEP_MODES else mode
    return bool(lib().ntm_xcd_sweep_gated(lv, md))


def xcd_sweep_xcds(device=None) -> int:
    """XCDs the sweep expects on ``device``: its CU count / 32."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.cuda.get_device_properties(dev).multi_processor_count // XCD_SWEEP_CUS_PER_XCD


def _xcd_sweep_slow(slow_xcd, slow_factor):
    if slow_xcd is None:
        return -1, 1
    if not 0 <= int(slow_xcd) < 16 or not 1 <= int(slow_factor) <= 64:
        raise ValueError("slow_xcd must be in 0 .. 15 and slow_factor in 1 .. 64")
    return int(slow_xcd), int(slow_factor)


def _xcd_sweep_records(rec: torch.Tensor):
    raw = rec.cpu().numpy()            # synchronises
    return raw.view(xcd_sweep_record_dtype()).copy()


def xcd_sweep_read(buf: torch.Tensor, pattern: int | str, seed: int, xcd_mask: int, passes: int,
                   wg_per_cu: int = 2, slow_xcd: int | None = None, slow_factor: int = 1):
    """K8: one launch of the verified per-XCD read; returns the workgroups' records (a numpy
    structured array, ``xcd_sweep_record_dtype``). ``buf`` is ``xcds`` equal slices (a
    multiple of 64 KiB each) that ``hbm_pattern_write(buf, pattern, seed)`` filled; slice x
    is read by the workgroups that find themselves on XCD x, ``passes`` times over, when bit
    x of ``xcd_mask`` is set. ``slow_xcd`` / ``slow_factor``: fault injection, the workgroups
    on that XCD sleep until each tile took ``slow_factor`` times its own duration."""
    if not buf.is_cuda or not buf.is_contiguous():
        raise ValueError("xcd_sweep_read needs a contiguous GPU tensor")
    xcds = xcd_sweep_xcds(buf.device)
    nbytes = buf.numel() * buf.element_size()
    if xcds < 1 or nbytes % xcds or (nbytes // xcds) % XCD_SWEEP_TILE_BYTES or nbytes == 0:
        raise ValueError(f"the buffer must be {xcds} slices, each a multiple of 64 KiB; got {nbytes} bytes")
    slice_bytes = nbytes // xcds
    if passes < 1 or passes * (slice_bytes // XCD_SWEEP_TILE_BYTES) >= 2**31 or wg_per_cu < 1:
        raise ValueError("xcd_sweep_read needs passes >= 1, passes * tiles < 2^31 and wg_per_cu >= 1")
    sx, sf = _xcd_sweep_slow(slow_xcd, slow_factor)
    grid = xcds * XCD_SWEEP_CUS_PER_XCD * int(wg_per_cu)
    with torch.cuda.device(buf.device):
        heads = torch.empty(lib().ntm_xcd_sweep_heads_bytes() // 4, dtype=torch.int32, device=buf.device)
        rec = torch.zeros(grid * 16, dtype=torch.int32, device=buf.device)
        rc = lib().ntm_xcd_sweep_read_launch(buf.data_ptr(), slice_bytes, xcds, int(xcd_mask) & 0xFFFFFFFF,
                                             int(passes), hbm_pattern_id(pattern), seed & (2**64 - 1), grid,
                                             sx, sf, heads.data_ptr(), rec.data_ptr(), stream_handle())
        check(rc, "ntm_xcd_sweep_read_launch")
        return _xcd_sweep_records(rec)


def xcd_sweep_mfma(device=None, batches: int = 64, seed: int = 7, xcd_mask: int | None = None,
                   wg_per_cu: int = 1, slow_xcd: int | None = None, slow_factor: int = 1):
    """K8: one launch of the per-XCD clock probe under matrix load: one 4-wave workgroup per
    CU (``wg_per_cu``), each wave running ``batches`` x 512 back-to-back bf16 MFMAs between
    two stamp pairs. Returns the records; ``tiles`` is the workgroup's MFMA count."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("xcd_sweep_mfma needs a GPU device")
    xcds = xcd_sweep_xcds(dev)
    if xcds < 1 or not 1 <= batches <= 65536 or wg_per_cu < 1:
        raise ValueError("xcd_sweep_mfma needs 1 <= batches <= 65536 and wg_per_cu >= 1")
    sx, sf = _xcd_sweep_slow(slow_xcd, slow_factor)
    mask = (1 << xcds) - 1 if xcd_mask is None else int(xcd_mask) & 0xFFFFFFFF
    grid = xcds * XCD_SWEEP_CUS_PER_XCD * int(wg_per_cu)
    with torch.cuda.device(dev):
        sink = torch.zeros(1, dtype=torch.float32, device=dev)
        rec = torch.zeros(grid * 16, dtype=torch.int32, device=dev)
        rc = lib().ntm_xcd_sweep_mfma_launch(grid, int(batches), seed & 0xFFFFFFFF, xcds, mask, sx, sf,
                                             rec.data_ptr(), sink.data_ptr(), stream_handle())
        check(rc, "ntm_xcd_sweep_mfma_launch")
        return _xcd_sweep_records(rec)


def xcd_sweep_summarize(records, level: int | str, mode: int | str, xcds: int, ratio: float = 0.0,
                        gpu: int = 0, expected_tiles: int = 0, xcd_mask: int | None = None) -> dict:
    """Aggregate records (one launch, or launches with disjoint masks concatenated) per XCD:
    workgroups, CUs, tiles, bytes, span over the XCD's own stamps, rate, clock; conservation
    against ``expected_tiles`` (passes x tiles per slice; 0 = not checked); the rule
    ``rate < ratio x median`` when ``ratio > 0`` and at least 3 XCDs are judged; ``ok``,
    ``failures`` and the Job's one-line ``message``. No GPU needed."""
    import json

    import numpy as np
    lv = XCD_SWEEP_LEVELS.index(level) if level in XCD_SWEEP_LEVELS else level
    md = XCD_SWEEP_MODES.index(mode) if mode in XCD_SWEEP_MODES else mode
    if lv not in range(4) or md not in range(2):
        raise ValueError(f"level is one of {XCD_SWEEP_LEVELS}, mode one of {XCD_SWEEP_MODES}")
    if not 1 <= xcds <= 16:
        raise ValueError("xcds must be in 1 .. 16")
    mask = (1 << xcds) - 1 if xcd_mask is None else int(xcd_mask) & 0xFFFFFFFF
    recs = np.ascontiguousarray(records, dtype=xcd_sweep_record_dtype())
    buf = recs.tobytes()
    args = (buf, len(recs), lv, md, xcds, mask, int(expected_tiles), float(ratio), gpu)
    n = lib().ntm_xcd_sweep_summarize(*args, None, 0)
    out = ctypes.create_string_buffer(n + 1)
    lib().ntm_xcd_sweep_summarize(*args, out, n + 1)
    return json.loads(out.value.decode())


# K9: atomics and cross-XCD hand-off check (validation/include/ntm/atomics.hpp, atomics_plan.hpp).
ATOMIC_OPS = ("add_u32", "add_u64", "and_u32", "or_u32", "xor_u32", "min_i32", "max_i32", "max_u64",
              "cas_u32", "add_f32", "add_f64", "add_bf16x2", "add_f16x2")
ATOMICS_MAGIC = 0x4B394154
ATOMICS_SLAB_WORDS = 256           # 16-byte words of a 4 KiB slab
ATOMICS_SENTINEL = 0xFFFFFFFF
_ATOMICS_OFF = 0xFFFFFFFF          # no injection


def _atomic_op(op) -> int:
    if op in ATOMIC_OPS:
        return ATOMIC_OPS.index(op)
    if isinstance(op, int) and 0 <= op < len(ATOMIC_OPS):
        return op
    raise ValueError(f"op is one of {ATOMIC_OPS}")


def _atomics_device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the atomics check needs a GPU device")
    return dev


def atomics_exact(op, adds_per_slot: int, max_abs: int) -> bool:
    """Whether ``adds_per_slot`` adds of integers up to ``max_abs`` in size are exact in any
    order for ``op``: adds x max_abs < 2^24 (fp32), < 2^53 (fp64), <= 255 (bf16), <= 2047
    (fp16); a packed slot is two cells that take every second add. Integer ops: always."""
    if adds_per_slot < 0 or max_abs < 0 or adds_per_slot >= 2**64 or max_abs >= 2**64:
        return False
    return bool(lib().ntm_atomics_exact(_atomic_op(op), int(adds_per_slot), int(max_abs)))


def atomics_record_dtype():
    """numpy dtype of the 96-byte per-workgroup hand-off record (ntm::atm::Record)."""
    import numpy as np
    names = ("magic", "hw_id", "xcc_id", "wg", "episode", "episodes_read", "words_checked", "bad_words",
             "stale_words", "writer_mask", "warm_bad", "first_class", "writer_hw", "writer_xcc", "writer_wg",
             "first_off")
    dt = np.dtype([(n, "<u4") for n in names] + [("expected", "<u8"), ("got", "<u8"), ("ticket", "<u4"),
                                                ("sleeps", "<u4"), ("pad0", "<u4"), ("pad1", "<u4")])
    assert dt.itemsize == 96
    return dt


def _atomics_rmw(fn, what, op, slots, grid, iters, seed, max_abs, device):
    import numpy as np
    o, dev = _atomic_op(op), _atomics_device(device)
    if not lib().ntm_atomics_rmw_shape_ok(o, int(slots), int(grid), int(iters), int(max_abs)):
        raise ValueError(f"{what}: {ATOMIC_OPS[o]} refuses slots={slots}, grid={grid}, iters={iters}, "
                         f"max_abs={max_abs} (grid x 256 x iters must be a multiple of slots and below 2^32; "
                         "float adds must stay exact: atomics_exact)")
    wide = lib().ntm_atomics_slot_bytes(o) == 8
    with torch.cuda.device(dev):
        table = torch.empty(int(slots), dtype=torch.int64 if wide else torch.int32, device=dev)
        check(fn(o, table.data_ptr(), int(slots), int(grid), int(iters), seed & (2**64 - 1), int(max_abs),
                 stream_handle()), what)
        return table.cpu().numpy().view(np.uint64 if wide else np.uint32).copy()


def atomics_rmw(op, slots: int, grid: int, iters: int, seed: int = 0x4B39, max_abs: int = 1, device=None):
    """K9: ``grid`` x 256 threads x ``iters`` non-returning agent-scope atomics of kind ``op``;
    operation ``k = gid * iters + it`` hits slot ``k % slots``. Returns the table (numpy uint32,
    or uint64 for the 8-byte ops; ``cas_u32``: claim word low, success count high)."""
    return _atomics_rmw(lib().ntm_atomics_rmw_launch, "ntm_atomics_rmw_launch", op, slots, grid, iters, seed,
                        max_abs, device)


def atomics_rmw_reference(op, slots: int, grid: int, iters: int, seed: int = 0x4B39, max_abs: int = 1,
                          device=None):
    """The table ``atomics_rmw`` must produce, from a GPU kernel that uses no atomic: one
    thread per slot folds its operations in order."""
    return _atomics_rmw(lib().ntm_atomics_rmw_reference_launch, "ntm_atomics_rmw_reference_launch", op, slots,
                        grid, iters, seed, max_abs, device)


def atomics_rmw_expected(op, slots: int, total: int, seed: int = 0x4B39, max_abs: int = 1):
    """The same table computed on the host. No GPU needed."""
    import numpy as np
    o = _atomic_op(op)
    out = np.zeros(int(slots), dtype=np.uint64 if lib().ntm_atomics_slot_bytes(o) == 8 else np.uint32)
    if lib().ntm_atomics_expected(o, int(slots), int(total), seed & (2**64 - 1), int(max_abs), out.ctypes.data):
        raise ValueError("atomics_rmw_expected: refused arguments")
    return out


def atomics_tickets(heads: int, grid: int, iters: int, device=None, inject: int | None = None) -> dict:
    """K9: every thread draws ``iters`` tickets with a returning fetch-add, head
    ``(gid + it) % heads``, and stores its gid into ``claim[head][ticket]``. Returns
    ``counters`` (one per head, as the device holds them: 32 words apart), ``claim``
    (heads x tickets per head) and the shape. ``inject``: that thread writes its first
    ticket one entry too high (fault injection)."""
    dev = _atomics_device(device)
    nbytes = lib().ntm_atomics_ticket_claim_bytes(int(heads), int(grid), int(iters))
    if not nbytes:
        raise ValueError("atomics_tickets needs 1 <= heads <= 1024 dividing grid x 256, and iters >= 1")
    with torch.cuda.device(dev):
        counters = torch.empty(lib().ntm_atomics_counter_bytes(int(heads)) // 4, dtype=torch.int32, device=dev)
        claim = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        check(lib().ntm_atomics_ticket_launch(counters.data_ptr(), claim.data_ptr(), int(heads), int(grid),
                                              int(iters), _ATOMICS_OFF if inject is None else int(inject),
                                              stream_handle()), "ntm_atomics_ticket_launch")
        import numpy as np
        return {"counters": counters.cpu().numpy().view(np.uint32).copy(),
                "claim": claim.cpu().numpy().view(np.uint32).reshape(int(heads), -1).copy(),
                "heads": int(heads), "grid": int(grid), "iters": int(iters)}


def atomics_handoff(episodes: int, episode_size: int, rounds: int = 1, seed: int = 0x4B39, device=None,
                    inject: tuple[int, int] | None = None):
    """K9: ``rounds`` launches of the cross-XCD hand-off on ``episodes`` episodes of
    ``episode_size`` workgroups; round r finds the slabs holding round r - 1. Returns the
    records of all rounds, concatenated (``atomics_record_dtype``). ``inject = (round, wg)``:
    in that round (1-based) that workgroup leaves one 64-byte line of its slab at last
    round's pattern (fault injection: a lost write-back)."""
    import numpy as np
    dev = _atomics_device(device)
    nbytes = lib().ntm_atomics_handoff_slab_bytes(int(episodes), int(episode_size))
    if not nbytes or rounds < 1:
        raise ValueError("atomics_handoff needs episodes >= 1, 2 <= episode_size <= 64 and rounds >= 1")
    grid = int(episodes) * int(episode_size)
    with torch.cuda.device(dev):
        slabs = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        counters = torch.empty(lib().ntm_atomics_counter_bytes(int(episodes)) // 4, dtype=torch.int32, device=dev)
        check(lib().ntm_atomics_handoff_init(slabs.data_ptr(), int(episodes), int(episode_size),
                                             seed & (2**64 - 1), 0, stream_handle()), "ntm_atomics_handoff_init")
        out = []
        for r in range(1, int(rounds) + 1):
            rec = torch.zeros(grid * 24, dtype=torch.int32, device=dev)
            wg = int(inject[1]) if inject is not None and int(inject[0]) == r else _ATOMICS_OFF
            check(lib().ntm_atomics_handoff_launch(slabs.data_ptr(), counters.data_ptr(), rec.data_ptr(),
                                                   int(episodes), int(episode_size), seed & (2**64 - 1), r, wg,
                                                   stream_handle()), "ntm_atomics_handoff_launch")
            out.append(rec.cpu().numpy().view(atomics_record_dtype()).copy())
        return np.concatenate(out)


def atomics_summarize(kind: str, gpu: int = 0, **kw) -> dict:
    """The Job's verdict on one sub-test, no GPU needed: ``ok``, the counts, ``failures`` and
    the one-line ``message``.

    ``"rmw"``: ``op``, ``got``, ``expected`` (tables) - names op, slot, expected, got, bad bits.
    ``"tickets"``: ``counters``, ``claim``, ``grid``, ``iters`` (``atomics_tickets``' result) -
    names head and ticket as missing, duplicate or invalid, and a counter that is short.
    ``"handoff"``: ``records``, ``episodes``, ``episode_size``, ``xcds``, ``launches`` - names
    reader and writer of a stale or corrupt word; one reader per episode and launch, all words
    checked, and at least one cross-XCD pair on a device with more than one XCD."""
    import json

    import numpy as np
    L = lib()
    if kind == "rmw":
        o = _atomic_op(kw["op"])
        dt = np.uint64 if L.ntm_atomics_slot_bytes(o) == 8 else np.uint32
        got, exp = np.ascontiguousarray(kw["got"], dtype=dt), np.ascontiguousarray(kw["expected"], dtype=dt)
        if got.shape != exp.shape:
            raise ValueError("got and expected differ in shape")
        call = lambda out, cap: L.ntm_atomics_summarize_rmw(o, got.ctypes.data, exp.ctypes.data, got.size, gpu, out, cap)
    elif kind == "tickets":
        counters = np.ascontiguousarray(kw["counters"], dtype=np.uint32)
        claim = np.ascontiguousarray(kw["claim"], dtype=np.uint32)
        heads = claim.shape[0]
        if claim.nbytes != L.ntm_atomics_ticket_claim_bytes(heads, kw["grid"], kw["iters"]) or \
                counters.nbytes < L.ntm_atomics_counter_bytes(heads):
            raise ValueError("counters / claim do not fit heads, grid and iters")
        call = lambda out, cap: L.ntm_atomics_summarize_tickets(counters.ctypes.data, claim.ctypes.data, heads,
                                                                kw["grid"], kw["iters"], gpu, out, cap)
    elif kind == "handoff":
        recs = np.ascontiguousarray(kw["records"], dtype=atomics_record_dtype())
        buf = recs.tobytes()
        call = lambda out, cap: L.ntm_atomics_summarize_handoff(buf, len(recs), kw["episodes"], kw["episode_size"],
                                                                kw["xcds"], kw.get("launches", 1), gpu, out, cap)
    else:
        raise ValueError('kind is "rmw", "tickets" or "handoff"')
    n = call(None, 0)
    if not n:
        raise ValueError(f"atomics_summarize({kind!r}): refused arguments")
    out = ctypes.create_string_buffer(n + 1)
    call(out, n + 1)
    return json.loads(out.value.decode())


def gemm_tolerance(k: int) -> tuple[float, float]:
    """(atol, rtol) for bf16-rounded output of an fp32-accumulated K-term dot product
    of U[-1,1) operands: bf16 output rounding (2^-8 relative) dominates; the fp32
    summation-order difference grows ~sqrt(K) * 2^-24 * |terms|."""
    atol = 1e-3 + 4.0 * (k ** 0.5) * 2.0 ** -20
    return atol, 2.0 ** -7


def clock_probe_ghz(device=None, iters: int = 20000, grid: int = 256) -> dict:
    """Shader clock this GPU holds under a dense bf16 MFMA load on random
    operands (``clock_probe_kernel``: Delta s_memtime / Delta s_memrealtime per
    wave, one 4-wave block per CU). Returns the median / min / max GHz over
    waves and the probe's wall time. Run it right after a timed loop: it reads
    the power / thermal state that loop left, which is what tells a
    power-limited GPU apart from a slow one in a multi-GPU run."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.zeros(grid * 4 * 2, dtype=torch.int64, device=dev)
    sink = torch.zeros(1, dtype=torch.float32, device=dev)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    check(lib().ntm_clock_probe(grid, iters, out.data_ptr(), sink.data_ptr(), stream_handle()),
          "ntm_clock_probe")
    t1.record()
    t1.synchronize()
    v = out.view(-1, 2).double()
    res = _ghz_summary(v[:, 0] / v[:, 1] * 0.1)
    res["probe_ms"] = round(t0.elapsed_time(t1), 3)
    res["waves"] = res.pop("n")
    return res


def _ghz_summary(ghz: torch.Tensor) -> dict:
    """median / p10 / min / max of per-wave (or per-workgroup) clocks; None
    fields when no finite sample is left (a caller in a collective must not
    raise on one rank)."""
    ghz = ghz[torch.isfinite(ghz) & (ghz > 0)]
    if ghz.numel() == 0:
        return {"median_GHz": None, "p10_GHz": None, "min_GHz": None, "max_GHz": None, "n": 0}
    q = torch.quantile(ghz, torch.tensor([0.1, 0.5], dtype=ghz.dtype, device=ghz.device))
    return {"median_GHz": round(float(q[1]), 4), "p10_GHz": round(float(q[0]), 4),
            "min_GHz": round(float(ghz.min()), 4), "max_GHz": round(float(ghz.max()), 4),
            "n": int(ghz.numel())}


def gemm_clock_ghz(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
                   steps: int = 1, prequeue=None, prequeue_launches: int = 0) -> dict:
    """K1's OWN clock: ``steps`` back-to-back launches
    of the shipping pingpong8o build with a start / end s_memtime +
    s_memrealtime stamp per workgroup and the XCC_ID register of the XCD that
    ran it (gemm_bf16_pp6.hpp STAMP 1; C is the real product). Per workgroup
    and launch, clock = d(shader cycles) / d(100 MHz ticks).

    Returns median / p10 / min / max GHz over all workgroups, per-XCD medians
    keyed by the REAL XCC id, whether the dispatcher's ``blockIdx & 7`` round
    robin matched those ids, and ``bound_GHz``: per launch the slowest XCD's
    median clock (the tiles are split evenly over the XCDs, so the slowest
    one sets the launch time), median over launches. Needs whole 256x256
    tiles, K % 128, K >= 256. The MFMA-only ``clock_probe_ghz`` reads the clock
    of a different load (no LDS or HBM traffic): under shared power the two
    can differ by 15-20 %. ``prequeue`` (a launch callable) is called
    ``prequeue_launches`` times right before the stamped launches, with no host
    sync between, so they start in the steady state of a loaded GPU."""
    _require(a, "a", torch.bfloat16)
    _require(b, "b", torch.bfloat16)
    m, k = a.shape
    n = b.shape[0]
    grid = lib().ntm_gemm_bf16_clock_grid(m, n)
    if grid <= 0 or k % 128 or k < 256 or b.shape[1] != k:
        raise ValueError(f"shape ({m},{n},{k}) not served by the clock build (M, N % 256, K % 128, K >= 256)")
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    _require(out, "out", torch.bfloat16)
    words = lib().ntm_gemm_bf16_clock_words()
    stamps = torch.zeros((steps, grid, words), dtype=torch.int64, device=a.device)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    for _ in range(prequeue_launches if prequeue is not None else 0):
        prequeue()
    t0.record()
    for i in range(steps):
        check(lib().ntm_gemm_bf16_clock(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
                                        a.stride(0), b.stride(0), out.stride(0),
                                        stamps[i].data_ptr(), stream_handle()),
              "ntm_gemm_bf16_clock")
    t1.record()
    t1.synchronize()
    return clock_summary(stamps.cpu(), t0.elapsed_time(t1) / steps)


CLOCK_DRIFT_MAX = 0.03
CLOCK_MAX_BATCHES = 3


def gemm_clock_stable(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
                      steps: int = 20, prequeue=None, prequeue_launches: int = 40,
                      max_batches: int = CLOCK_MAX_BATCHES,
                      drift_max: float = CLOCK_DRIFT_MAX) -> dict:
    """``gemm_clock_ghz`` with a self-check: a batch whose
    per-launch stamp windows (``per_launch_window_us_median``) drift by more
    than ``drift_max`` (max / min - 1) caught a clock transient and is stamped
    again - each batch queued behind ``prequeue_launches`` plain launches with
    no host sync - up to ``max_batches``. Returns the first stable batch (else
    the least drifted) with ``clock_batches``, ``clock_batch_drift_pct`` (per
    batch) and ``clock_stable``."""
    best, drifts = None, []
    for _ in range(max(1, max_batches)):
        r = gemm_clock_ghz(a, b, out, steps=steps, prequeue=prequeue,
                           prequeue_launches=prequeue_launches)
        w = [x for x in r["per_launch_window_us_median"] if x > 0]
        d = (max(w) / min(w) - 1.0) if w else float("inf")
        drifts.append(round(100 * d, 2) if d != float("inf") else None)
        if best is None or d < best[0]:
            best = (d, r)
        if d <= drift_max:
            break
    r = best[1]
    r["clock_batches"] = len(drifts)
    r["clock_batch_drift_pct"] = drifts
    r["clock_stable"] = best[0] <= drift_max
    return r


def clock_summary(stamps: torch.Tensor, ms_per_launch: float) -> dict:
    """Summary of a [launches, workgroups, words] record of the clock build
    (host-side; see ``gemm_clock_ghz``)."""
    steps, grid = stamps.shape[0], stamps.shape[1]
    sv = stamps.double()
    ghz = (sv[:, :, 2] - sv[:, :, 0]) / (sv[:, :, 3] - sv[:, :, 1]) * 0.1   # [steps, grid]
    res = _ghz_summary(ghz.reshape(-1))
    res["workgroups"] = res.pop("n")
    # the XCD that really ran each workgroup (XCC_ID register) ...
    xcc = (stamps[:, :, 4] & 0xF).long()
    ids = sorted(set(xcc.reshape(-1).tolist()))
    res["xcc_ids"] = ids
    res["per_xcc_median_GHz"] = {str(x): _ghz_summary(ghz[xcc == x])["median_GHz"] for x in ids}
    # ... against the dispatcher's round robin, blockIdx & 7 (what stream-K's
    # per-XCD tile lists and its write-through / L1-only-acquire protocol assume)
    resid = torch.arange(grid) & 7
    seen = {r: sorted(set(xcc[:, resid == r].reshape(-1).tolist())) for r in range(min(8, grid))}
    one_each = all(len(v) == 1 for v in seen.values())
    res["xcc_of_blockidx_mod_8"] = {str(r): v for r, v in seen.items()}
    res["blockidx_mod_8_is_xcc"] = bool(one_each and len({v[0] for v in seen.values()}) == len(seen))
    # kept for continuity with earlier rounds' JSON: groups by b & 7
    res["per_xcd_group_median_GHz"] = [_ghz_summary(ghz[:, r::8].reshape(-1))["median_GHz"]
                                       for r in range(min(8, grid))]
    res["ms_per_launch"] = round(ms_per_launch, 4)
    res["launches"] = steps
    # per launch: medians over workgroups of the shader cycles and of the wall
    # window (us) between a workgroup's two stamps - to set against a profiler's
    # per-dispatch duration and cycle counters (tools/clock_check.py)
    cyc = (sv[:, :, 2] - sv[:, :, 0]).median(dim=1).values
    win = ((sv[:, :, 3] - sv[:, :, 1]) / 100.0).median(dim=1).values
    # the median workgroup's cycles over the median workgroup's window, median
    # over launches (2.0 / 2.7 % below GRBM_GUI_ACTIVE / 8 XCDs / duration on the
    # same dispatches, profiles/r4_clock/)
    lg = cyc / (win * 1e3)
    lg = lg[torch.isfinite(lg) & (lg > 0)]
    res["launch_GHz"] = round(float(lg.median()), 4) if lg.numel() else None
    # the launch-bounding clock: every XCD gets the same number of tiles, so the
    # slowest XCD's workgroups finish last and set the launch time
    bound, spread = [], []
    for i in range(steps):
        per = [float(ghz[i][xcc[i] == x].median()) for x in ids if bool((xcc[i] == x).any())]
        per = [v for v in per if v == v and v > 0]
        if per:
            bound.append(min(per))
            spread.append(max(per) / min(per) - 1.0)
    res["bound_GHz"] = round(sorted(bound)[len(bound) // 2], 4) if bound else None
    res["xcc_clock_spread_pct"] = round(100 * sorted(spread)[len(spread) // 2], 2) if spread else None
    # when each XCD's last workgroup ended, after the launch's first start (us,
    # median over launches): the gap between the first and the last XCD to finish
    # is how long the faster XCDs idle at the end of every launch
    rt0 = sv[:, :, 1].min(dim=1).values                      # [steps]
    fin = {x: [] for x in ids}
    for i in range(steps):
        for x in ids:
            sel = xcc[i] == x
            if bool(sel.any()):
                fin[x].append(float((sv[i, :, 3][sel].max() - rt0[i]) / 100.0))
    res["per_xcc_finish_us"] = {str(x): round(sorted(v)[len(v) // 2], 2) for x, v in fin.items() if v}
    idle = []
    for i in range(steps):
        ends = [float((sv[i, :, 3][xcc[i] == x].max() - rt0[i]) / 100.0)
                for x in ids if bool((xcc[i] == x).any())]
        if ends:
            idle.append(max(ends) - min(ends))
    res["xcc_finish_spread_us"] = round(sorted(idle)[len(idle) // 2], 2) if idle else None
    res["per_launch_cycles_median"] = [int(x) for x in cyc.tolist()]
    res["per_launch_window_us_median"] = [round(x, 2) for x in win.tolist()]
    return res


# K12: wave data paths and the special-function unit (validation/include/ntm/wave_paths.hpp,
# wave_paths_plan.hpp). The host side (op list, maps, generators, brackets) is numpy: ops/wave.py.
def _wave_words(t, name, device=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.element_size() != 4 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous GPU tensor of 32-bit elements")
    if device is not None and t.device != device:
        raise ValueError(f"{name} must be on {device}")
    return t


def wave_to_device(words, device) -> torch.Tensor:
    """numpy uint32 words -> an int32 GPU tensor of the same bits."""
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).to(device)


def _wave_lane(reference, op, ctrl, x, old):
    if isinstance(op, str):
        op = _wave.wave_lane_op_index(op if ctrl is None else f"{op} {ctrl}")
    op = int(op)
    x, old = _wave_words(x, "x"), _wave_words(old, "old", x.device)
    if x.numel() != old.numel():
        raise ValueError("x and old must have one size")
    out = torch.zeros_like(x, dtype=torch.int32)
    with torch.cuda.device(x.device):
        rc = lib().ntm_wave_lane(int(reference), op, 1, x.data_ptr(), old.data_ptr(), out.data_ptr(), x.numel(), stream_handle())
    check(rc, "ntm_wave_lane")
    return out


def wave_lane(op, ctrl, x: torch.Tensor, old: torch.Tensor) -> torch.Tensor:
    """K12: one op of the ``lane`` family on the words ``x`` (and ``old``: the DPP old value, the
    second register of a swap), a multiple of 256 words, each 64 one wave. ``op`` is an index
    into ``wave_lane_ops()`` or the op's name (``"row_shr:3"`` with ``ctrl="bound_ctrl:0"``, or
    the whole name with ``ctrl=None``). A bad op or size raises and launches nothing."""
    return _wave_lane(False, op, ctrl, x, old)


def wave_lane_reference_gpu(op, ctrl, x: torch.Tensor, old: torch.Tensor) -> torch.Tensor:
    """K12: ``wave_lane`` through LDS by the plan's lane map, with no cross-lane instruction."""
    return _wave_lane(True, op, ctrl, x, old)


def _wave_tr(reference, bits, image, stride):
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous():
        raise ValueError("the image must be a contiguous uint8 GPU tensor")
    stride = int(stride)
    rows = image.numel() // stride if stride > 0 else 0
    n = lib().ntm_wave_tr_out_words(int(bits), rows, stride) if stride > 0 and rows * stride == image.numel() else 0
    if n == 0:
        raise ValueError("bad transposed-read shape (rows a multiple of the block's, stride a multiple of 8 - 16 for "
                         "6-bit - and at least 32, image within 16 KiB)")
    out = torch.zeros(n, dtype=torch.int32, device=image.device)
    with torch.cuda.device(image.device):
        rc = lib().ntm_wave_tr_read(int(reference), int(bits), image.data_ptr(), rows, stride, out.data_ptr(), stream_handle())
    check(rc, "ntm_wave_tr_read")
    return out


def wave_tr_read(bits: int, image: torch.Tensor, stride: int) -> torch.Tensor:
    """K12: one workgroup reads ``image`` (uint8, rows x ``stride`` bytes, 16-byte aligned) through
    the ``bits``-wide transposed LDS read -> int32 words in the layout of
    ``wave_expected_tr_read``. A misaligned image or a bad stride raises and launches nothing."""
    return _wave_tr(False, bits, image, stride)


def wave_tr_read_reference_gpu(bits: int, image: torch.Tensor, stride: int) -> torch.Tensor:
    """K12: ``wave_tr_read`` with byte reads and shifts by the plan's map."""
    return _wave_tr(True, bits, image, stride)


def _sfu_id(op) -> int:
    if isinstance(op, str):
        if op not in _wave.WAVE_SFU_OPS:
            raise ValueError(f"op must be one of {_wave.WAVE_SFU_OPS}")
        return _wave.WAVE_SFU_OPS.index(op)
    return int(op)


def wave_sfu(op, x: torch.Tensor) -> torch.Tensor:
    """K12: the raw result words of one fp32 transcendental instruction on the words ``x``."""
    x = _wave_words(x, "x")
    y = torch.zeros_like(x, dtype=torch.int32)
    with torch.cuda.device(x.device):
        rc = lib().ntm_wave_sfu(_sfu_id(op), x.data_ptr(), y.data_ptr(), x.numel(), stream_handle())
    check(rc, "ntm_wave_sfu")
    return y


def wave_sfu_distance(op, x: torch.Tensor, y: torch.Tensor, bound: int | None = None) -> dict:
    """K12: the ordered-integer distance of the results ``y`` of ``op`` on ``x`` from the host's
    brackets (``ops.wave_sfu_brackets``), computed on the device in integers: ``max_d``,
    ``max_index``, and with a ``bound`` the count ``beyond`` it and ``first_beyond``."""
    import numpy as np
    x, y = _wave_words(x, "x"), _wave_words(y, "y", x.device)
    lo, hi = _wave.wave_sfu_brackets(_sfu_id(op), x.cpu().numpy().view(np.uint32))
    dlo, dhi = wave_to_device(lo, x.device), wave_to_device(hi, x.device)
    res = torch.tensor([0, -1, 0, -1], dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().ntm_wave_sfu_distance(y.data_ptr(), dlo.data_ptr(), dhi.data_ptr(), x.numel(),
                                         0xFFFFFFFF if bound is None else int(bound), res.data_ptr(), stream_handle())
    check(rc, "ntm_wave_sfu_distance")
    r = res.cpu().numpy().view(np.uint32)
    return {"max_d": int(r[0]), "max_index": None if r[0] == 0 else int(r[1]), "beyond": int(r[2]),
            "first_beyond": None if r[2] == 0 else int(r[3])}


def wave_valu(op: str, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor | None = None, reference: bool = False) -> torch.Tensor:
    """K12: ``op="bitop3"``: v_bitop3_b32 of a, b, c under all 256 truth tables -> [256, n];
    ``op="cvt_pk_bf16"``: v_cvt_pk_bf16_f32 of the fp32 words a (low half) and b (high half) -> [n].
    ``reference=True`` evaluates the table bit by bit / rounds in integers."""
    if op not in ("bitop3", "cvt_pk_bf16"):
        raise ValueError("op must be 'bitop3' or 'cvt_pk_bf16'")
    a, b = _wave_words(a, "a"), _wave_words(b, "b", a.device)
    if op == "bitop3":
        c = _wave_words(c, "c", a.device)
    n = a.numel()
    if b.numel() != n or (op == "bitop3" and c.numel() != n):
        raise ValueError("the operands must have one size")
    out = torch.zeros((256, n) if op == "bitop3" else (n,), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib().ntm_wave_valu(int(reference), 0 if op == "bitop3" else 1, a.data_ptr(), b.data_ptr(),
                                 c.data_ptr() if op == "bitop3" else None, out.data_ptr(), n, stream_handle())
    check(rc, "ntm_wave_valu")
    return out


def wave_sweep(family: str, inputs: torch.Tensor, layout, expected: torch.Tensor | None, grid: int,
               fault_wg: int | None = None, fault_index: int = 0):
    """K12: the per-CU form of one family: ``grid`` workgroups each run it against ``expected``
    and leave one record -> a numpy structured array (``hw_id``, ``xcc_id``, ``simd``, ``magic``,
    ``wg``, ``bad``, ``first`` (complement of the smallest bad index, 0 = none), ``expected``,
    ``got``, ``digest`` [7]). Layout of ``inputs``: wave_paths.hpp. For ``"sfu"`` ``fault_wg`` is the
    key of a CU (``wave_cu_key``) whose workgroups flip bit 10 of word ``fault_index`` of v_exp_f32."""
    import ctypes
    import numpy as np
    fam = _wave.WAVE_FAMILIES.index(family)
    inputs = _wave_words(inputs, "inputs")
    nb = lib().ntm_wave_record_bytes()
    rec = torch.zeros(int(grid) * nb // 8, dtype=torch.int64, device=inputs.device)
    lay = (ctypes.c_uint * max(len(layout or ()), 1))(*(layout or (0,)))
    with torch.cuda.device(inputs.device):
        rc = lib().ntm_wave_sweep(fam, inputs.data_ptr(), inputs.numel(), ctypes.cast(lay, ctypes.c_void_p) if layout else None,
                                  expected.data_ptr() if expected is not None else None, rec.data_ptr(), int(grid),
                                  0xFFFFFFFF if fault_wg is None else int(fault_wg), int(fault_index), stream_handle())
    check(rc, "ntm_wave_sweep")
    dt = _wave_record_dtype()
    assert dt.itemsize == nb
    return rec.cpu().numpy().view(dt)


def wave_sfu_digest(device, grid: int):
    """K12: every workgroup of ``grid`` runs the whole input list of the seven transcendentals;
    -> (records, digests uint64 [grid, 7])."""
    import numpy as np
    lists = [_wave.wave_sfu_inputs(op)[0] for op in range(7)]
    recs = wave_sweep("sfu", wave_to_device(np.concatenate(lists), device), [len(v) for v in lists], None, grid)
    return recs, recs["digest"]


def wave_sfu_locate(op, x: torch.Tensor, cu_key: int, on_key: bool, grid: int, max_launches: int = 8,
                    fault_key: int | None = None, fault_index: int = 0):
    """K12: the second, small launch behind an inconsistent digest. Of ``grid`` workgroups the first
    that runs on the CU ``cu_key`` (``on_key``; else on any other CU) stores the result words of
    instruction ``op`` on ``x`` -> (words int32 tensor, its record) or ``None`` when no workgroup
    landed there within ``max_launches`` launches (a cap, not a retry)."""
    import numpy as np
    x = _wave_words(x, "x")
    nb = lib().ntm_wave_record_bytes()
    y = torch.zeros_like(x, dtype=torch.int32)
    for _ in range(max_launches):
        side = torch.zeros(8 + nb // 8, dtype=torch.int64, device=x.device)
        with torch.cuda.device(x.device):
            rc = lib().ntm_wave_sfu_locate(_sfu_id(op), x.data_ptr(), x.numel(), int(cu_key), int(bool(on_key)), side.data_ptr(),
                                           y.data_ptr(), side.data_ptr() + 64, int(grid),
                                           0xFFFFFFFF if fault_key is None else int(fault_key), int(fault_index), stream_handle())
        check(rc, "ntm_wave_sfu_locate")
        raw = side.cpu().numpy()
        if raw[0] & 0xFFFFFFFF:
            return y, raw[8:].view(_wave_record_dtype())[0]
    return None


def _wave_record_dtype():
    import numpy as np
    return np.dtype([("hw_id", "<u4"), ("xcc_id", "<u4"), ("simd", "u1", 4), ("magic", "<u4"), ("wg", "<u4"), ("bad", "<u4"),
                     ("first", "<u4"), ("expected", "<u4"), ("got", "<u4"), ("pad", "<u4"), ("digest", "<u8", 7)])


def wave_cu_key(rec) -> int:
    """(xcc, se, sh, cu) of a record packed as the header's ``cu_key``."""
    h, x = int(rec["hw_id"]), int(rec["xcc_id"])
    return ((x & 15) << 8) | (((h >> 13) & 7) << 5) | (((h >> 12) & 1) << 4) | ((h >> 8) & 15)
