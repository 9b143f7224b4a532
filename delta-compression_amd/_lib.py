"""ctypes binding of libdeltagpu.so (include/delta_gpu.h).

Device buffers are passed as integer device addresses (e.g. a torch tensor's
``data_ptr()``) and streams as integer ``hipStream_t`` handles (e.g.
``torch.cuda.current_stream().cuda_stream``).  No torch type crosses the C ABI.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
# DG_LIB_VARIANT=prof selects the profiling build (make prof); never a CPU path
_VARIANT = os.environ.get("DG_LIB_VARIANT", "")
LIB_PATH = os.path.join(HERE, "lib", "libdeltagpu%s.so" % ("_" + _VARIANT if _VARIANT else ""))

ALGO_GREEDY, ALGO_ONEPASS, ALGO_CORRECTING = 0, 1, 2
SEED_LEN = 16
TABLE_SIZE = 1048573
MAX_TABLE_SIZE = 1073741827
BUF_CAP = 256
OPT_VERBOSE, OPT_SPLAY, OPT_INPLACE, OPT_POLICY_CONSTANT = 0, 1, 2, 3
POLICIES = {"localmin": 0, "constant": 1}
CMD_COPY, CMD_ADD = 0, 1   # DG_CMD_COPY / DG_CMD_ADD
SKETCH_BINS = 256
SKETCH_EMPTY = 0xFFFFFFFFFFFFFFFF
MATCH_NONE = 0xFFFFFFFF
MATCH_ALL, MATCH_NOT_SELF, MATCH_EARLIER = 0, 1, 2
_MATCH_MODES = {"all": MATCH_ALL, "not_self": MATCH_NOT_SELF, "earlier": MATCH_EARLIER}

_ALGOS = {"greedy": ALGO_GREEDY, "onepass": ALGO_ONEPASS, "correcting": ALGO_CORRECTING}

STATUS = {
    0: "DG_OK", 1: "DG_ERR_INVALID_ARG", 2: "DG_ERR_UNSUPPORTED", 3: "DG_ERR_TOO_LARGE",
    4: "DG_ERR_NO_DEVICE", 5: "DG_ERR_HIP", 6: "DG_ERR_NOMEM", 7: "DG_ERR_CAPACITY",
    8: "DG_ERR_MALFORMED", 9: "DG_ERR_SRC_CRC", 10: "DG_ERR_DST_CRC", 11: "DG_ERR_TABLE_POOL", 12: "DG_ERR_INTERNAL",
}
LIMIT_TABLE_POOL_BYTES = 0
LIMIT_ONEPASS_MEMBERS = 1
MEMBERS_AUTO, MEMBERS_ON, MEMBERS_OFF = 0, 1, 2


class DeltaError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        self.code = code
        super().__init__(f"{STATUS.get(code, code)}: {msg}" if msg else STATUS.get(code, str(code)))


class DiffOptions(C.Structure):
    """delta_diff_options_t (src/c/delta.h:248-257)."""
    _fields_ = [("p", C.c_size_t), ("q", C.c_size_t), ("buf_cap", C.c_size_t),
                ("max_table", C.c_size_t), ("flags", C.c_uint64)]

    @classmethod
    def make(cls, p: int = SEED_LEN, q: int = TABLE_SIZE, buf_cap: int = BUF_CAP,
             max_table: int = MAX_TABLE_SIZE, flags: int = 0) -> "DiffOptions":
        return cls(p, q, buf_cap, max_table, flags)


class Buffer(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("len", C.c_size_t)]


class Pair(C.Structure):
    _fields_ = [("r_off", C.c_uint64), ("r_len", C.c_uint64),
                ("v_off", C.c_uint64), ("v_len", C.c_uint64)]


class Span(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint64)]


class DecodeDesc(C.Structure):
    _fields_ = [("ref_off", C.c_uint64), ("ref_len", C.c_uint64),
                ("delta_off", C.c_uint64), ("delta_len", C.c_uint64),
                ("out_off", C.c_uint64), ("out_cap", C.c_uint64)]


class InplaceDesc(C.Structure):   # dg_inplace_desc_t
    _fields_ = [("ref_off", C.c_uint64), ("ref_len", C.c_uint64),
                ("delta_off", C.c_uint64), ("delta_cap", C.c_uint64)]


class UpdateDesc(C.Structure):   # dg_update_desc_t
    _fields_ = [("buf_off", C.c_uint64), ("buf_cap", C.c_uint64), ("ref_len", C.c_uint64),
                ("delta_off", C.c_uint64), ("delta_len", C.c_uint64)]


class ComposeDesc(C.Structure):   # dg_compose_desc_t
    _fields_ = [("a_off", C.c_uint64), ("a_cap", C.c_uint64), ("b_off", C.c_uint64), ("b_cap", C.c_uint64)]


class InvertDesc(C.Structure):   # dg_invert_desc_t
    _fields_ = [("ref_off", C.c_uint64), ("ref_len", C.c_uint64),
                ("delta_off", C.c_uint64), ("delta_cap", C.c_uint64)]


class ReadStream(C.Structure):   # dg_read_stream_t
    _fields_ = [("ref_off", C.c_uint64), ("ref_len", C.c_uint64),
                ("delta_off", C.c_uint64), ("delta_len", C.c_uint64)]


class ReadReq(C.Structure):   # dg_read_req_t
    _fields_ = [("stream", C.c_uint32), ("off", C.c_uint32), ("len", C.c_uint32), ("reserved", C.c_uint32),
                ("out_off", C.c_uint64)]


class Match(C.Structure):   # dg_match_t
    _fields_ = [("best", C.c_uint32), ("equal", C.c_uint32), ("used", C.c_uint32), ("reserved", C.c_uint32)]


class InplaceStats(C.Structure):
    _fields_ = [("already_inplace", C.c_int), ("num_copies", C.c_uint64), ("num_adds", C.c_uint64),
                ("copy_bytes", C.c_uint64), ("add_bytes", C.c_uint64)]


class DeltaInfo(C.Structure):
    _fields_ = [("inplace", C.c_int), ("version_size", C.c_uint64),
                ("src_crc", C.c_uint8 * 8), ("dst_crc", C.c_uint8 * 8),
                ("num_commands", C.c_uint64), ("num_copies", C.c_uint64),
                ("num_adds", C.c_uint64), ("copy_bytes", C.c_uint64),
                ("add_bytes", C.c_uint64)]


class PlacedCommandC(C.Structure):   # dg_placed_command_t
    _fields_ = [("tag", C.c_uint32), ("src", C.c_uint64), ("dst", C.c_uint64), ("length", C.c_uint64),
                ("data", C.POINTER(C.c_uint8))]


class Commands(C.Structure):         # dg_commands_t
    _fields_ = [("data", C.POINTER(PlacedCommandC)), ("len", C.c_size_t), ("storage", C.c_void_p)]


def _share_torch_runtime() -> None:
    """One HIP runtime per process.

    PyTorch-ROCm ships its own libamdhip64/libhsa-runtime64.  If libdeltagpu.so
    were loaded first it would bind /opt/rocm's runtime and torch would then
    load a second one, which cannot open the device again ("No HIP GPUs are
    available").  Importing torch first makes the dynamic linker satisfy our
    libamdhip64.so.7 dependency with torch's already-loaded copy, so device
    pointers and streams are shared by construction.
    """
    try:
        import torch  # noqa: F401
    except Exception:  # torch absent: /opt/rocm's runtime is used
        pass


def _load() -> C.CDLL:
    _share_torch_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C delta-compression_amd` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u8p, sz, u32, u64, i32 = C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_uint32, C.c_uint64, C.c_int32
    sig = {
        "dg_abi_version": (C.c_int, []),
        "dg_diff_options_default": (None, [C.POINTER(DiffOptions)]),
        "dg_buffer_free": (None, [C.POINTER(Buffer)]),
        "dg_context_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "dg_context_destroy": (None, [vp]),
        "dg_context_stream": (vp, [vp]),
        "dg_context_set_limit": (C.c_int, [vp, C.c_int, u64]),
        "dg_status_string": (C.c_char_p, [C.c_int]),
        "dg_last_error": (C.c_char_p, [vp]),
        "dg_encode_plan_create": (C.c_int, [vp, C.c_int, C.POINTER(Pair), u32, C.POINTER(DiffOptions), C.POINTER(vp)]),
        "dg_encode_plan_output_bound": (u64, [vp]),
        "dg_encode_plan_num_pairs": (u32, [vp]),
        "dg_encode_plan_flags": (u32, [vp]),
        "dg_encode_plan_run_modes": (C.c_int, [vp, C.POINTER(u64), C.POINTER(u64)]),
        "dg_encode_plan_table_size": (u64, [vp, u32]),
        "dg_encode_plan_run": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, vp]),
        "dg_encode_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_encode_plan_set_timing_mode": (C.c_int, [vp, C.c_int]),
        "dg_encode_plan_set_timing_every": (C.c_int, [vp, C.c_int]),
        "dg_encode_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_encode_plan_copy_counts_device": (vp, [vp]),
        "dg_encode_plan_destroy": (None, [vp]),
        "dg_encode": (C.c_int, [vp, C.c_int, u8p, sz, u8p, sz, C.POINTER(DiffOptions), C.POINTER(Buffer)]),
        "dg_encode_batch": (C.c_int, [vp, C.c_int, C.POINTER(u8p), C.POINTER(sz), C.POINTER(u8p),
                                      C.POINTER(sz), u32, C.POINTER(DiffOptions), C.POINTER(Buffer),
                                      C.POINTER(i32)]),
        "dg_encode_pipelined": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(Pair), u32, C.POINTER(DiffOptions), u64,
                                          vp, u64, C.POINTER(u64), C.POINTER(i32)]),
        "dg_encode_pipelined_multi": (C.c_int, [C.POINTER(vp), u32, C.c_int, vp, vp, C.POINTER(Pair), u32,
                                                C.POINTER(DiffOptions), u64, vp, u64, C.POINTER(u64), C.POINTER(i32)]),
        "dg_host_alloc": (C.c_int, [vp, u64, C.POINTER(vp)]),
        "dg_host_free": (None, [vp]),
        "dg_crc64_xz": (C.c_int, [vp, u8p, sz, C.c_uint8 * 8]),
        "dg_crc64_xz_batch_device": (C.c_int, [vp, vp, C.POINTER(Span), u32, vp, vp]),
        "dg_decode": (C.c_int, [vp, u8p, sz, u8p, sz, C.c_int, C.POINTER(Buffer)]),
        "dg_decode_batch_device": (C.c_int, [vp, vp, vp, C.POINTER(DecodeDesc), u32, C.c_int, vp, vp, vp, vp]),
        "dg_decode_plan_create": (C.c_int, [vp, C.POINTER(DecodeDesc), u32, C.c_int, C.POINTER(vp)]),
        "dg_decode_plan_run": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "dg_decode_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_decode_plan_set_timing_every": (C.c_int, [vp, C.c_int]),
        "dg_decode_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_decode_plan_destroy": (None, [vp]),
        "dg_delta_info": (C.c_int, [u8p, sz, C.POINTER(DeltaInfo)]),
        "dg_diff": (C.c_int, [vp, C.c_int, u8p, sz, u8p, sz, C.POINTER(DiffOptions), C.POINTER(Commands)]),
        "dg_delta_decode": (C.c_int, [u8p, sz, C.POINTER(Commands), C.POINTER(DeltaInfo)]),
        "dg_encode_commands": (C.c_int, [C.POINTER(PlacedCommandC), sz, C.c_int, u64, C.c_uint8 * 8,
                                         C.c_uint8 * 8, C.POINTER(Buffer)]),
        "dg_commands_free": (None, [C.POINTER(Commands)]),
        "dg_make_inplace": (C.c_int, [u8p, sz, u8p, sz, C.c_int, C.POINTER(Buffer), C.POINTER(InplaceStats)]),
        "dg_inplace_plan_create": (C.c_int, [vp, C.POINTER(InplaceDesc), u32, C.c_int, C.POINTER(vp)]),
        "dg_inplace_plan_create_for": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp)]),
        "dg_inplace_plan_output_bound": (u64, [vp]),
        "dg_inplace_plan_run": (C.c_int, [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]),
        "dg_inplace_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_inplace_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_inplace_plan_destroy": (None, [vp]),
        "dg_make_inplace_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz), C.POINTER(u8p), C.POINTER(sz), u32,
                                            C.c_int, C.POINTER(Buffer), C.POINTER(i32)]),
        "dg_update_plan_create": (C.c_int, [vp, C.POINTER(UpdateDesc), u32, C.c_int, C.POINTER(vp)]),
        "dg_update_plan_run": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "dg_update_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_update_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_update_plan_destroy": (None, [vp]),
        "dg_update_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz), C.POINTER(sz), C.POINTER(u8p), C.POINTER(sz),
                                      u32, C.c_int, C.POINTER(sz), C.POINTER(i32)]),
        "dg_compose": (C.c_int, [u8p, sz, u8p, sz, C.c_int, C.POINTER(Buffer)]),
        "dg_compose_plan_create": (C.c_int, [vp, C.POINTER(ComposeDesc), u32, C.c_int, C.POINTER(vp)]),
        "dg_compose_plan_create_for": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(vp)]),
        "dg_compose_plan_run": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]),
        "dg_compose_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_compose_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_compose_plan_destroy": (None, [vp]),
        "dg_compose_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz), C.POINTER(u8p), C.POINTER(sz), u32,
                                       C.c_int, C.POINTER(Buffer), C.POINTER(i32)]),
        "dg_invert": (C.c_int, [u8p, sz, u8p, sz, C.POINTER(Buffer)]),
        "dg_invert_plan_create": (C.c_int, [vp, C.POINTER(InvertDesc), u32, C.POINTER(vp)]),
        "dg_invert_plan_create_for": (C.c_int, [vp, vp, C.POINTER(vp)]),
        "dg_invert_plan_output_bound": (u64, [vp]),
        "dg_invert_plan_run": (C.c_int, [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]),
        "dg_invert_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_invert_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_invert_plan_destroy": (None, [vp]),
        "dg_invert_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz), C.POINTER(u8p), C.POINTER(sz), u32,
                                      C.POINTER(Buffer), C.POINTER(i32)]),
        "dg_segment_pairs": (C.c_int, [C.POINTER(Pair), u32, u64, u64, C.POINTER(Pair), u64, C.POINTER(u32)]),
        "dg_splice": (C.c_int, [C.POINTER(Pair), C.POINTER(Pair), u32, C.POINTER(u8p), C.POINTER(sz), C.POINTER(i32),
                                C.c_uint8 * 8, C.POINTER(Buffer)]),
        "dg_splice_plan_create": (C.c_int, [vp, C.POINTER(Pair), u32, C.POINTER(Pair), C.POINTER(u32), u32,
                                            C.POINTER(u64), C.POINTER(vp)]),
        "dg_splice_plan_create_for": (C.c_int, [vp, vp, C.POINTER(Pair), C.POINTER(u32), u32, C.POINTER(vp)]),
        "dg_splice_plan_output_bound": (u64, [vp]),
        "dg_splice_plan_run": (C.c_int, [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]),
        "dg_splice_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_splice_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_splice_plan_destroy": (None, [vp]),
        "dg_splice_batch": (C.c_int, [vp, C.POINTER(Pair), u32, C.POINTER(Pair), C.POINTER(u32), C.POINTER(u8p),
                                      C.POINTER(sz), C.POINTER(i32), u8p, C.POINTER(Buffer), C.POINTER(i32)]),
        "dg_encode_large": (C.c_int, [vp, C.c_int, u8p, sz, u8p, sz, C.POINTER(DiffOptions), u64, u64,
                                      C.POINTER(Buffer)]),
        "dg_read": (C.c_int, [u8p, sz, u8p, sz, u64, u64, C.POINTER(Buffer)]),
        "dg_read_plan_create": (C.c_int, [vp, C.POINTER(ReadStream), u32, u32, C.POINTER(vp)]),
        "dg_read_plan_index": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "dg_read_plan_run": (C.c_int, [vp, vp, vp, vp, u32, vp, vp, vp, vp]),
        "dg_read_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_read_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_read_plan_destroy": (None, [vp]),
        "dg_read_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz), C.POINTER(u8p), C.POINTER(sz), u32,
                                    C.POINTER(ReadReq), u32, C.POINTER(Buffer), C.POINTER(i32)]),
        "dg_read_plan_chunk_index": (C.c_int, [vp, u32]),
        "dg_read_plan_index_chunked": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "dg_read_plan_index_get": (C.c_int, [vp, u32, vp, u64, C.POINTER(u64)]),
        "dg_read_plan_index_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_read_plan_index_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_tile_requests": (C.c_int, [u32, u32, C.POINTER(ReadReq), u32, C.POINTER(u32)]),
        "dg_decode_large": (C.c_int, [vp, u8p, sz, u8p, sz, C.c_int, u32, u32, C.POINTER(Buffer)]),
        "dg_read_lineage": (C.c_int, [u8p, sz, C.POINTER(u8p), C.POINTER(sz), u32, u64, u64, C.POINTER(Buffer)]),
        "dg_lineage_work_items": (u32, []),
        "dg_lineage_plan_create": (C.c_int, [vp, C.POINTER(u32), u32, C.POINTER(vp)]),
        "dg_lineage_plan_run": (C.c_int, [vp, vp, vp, vp, u32, vp, vp, vp, vp]),
        "dg_lineage_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_lineage_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_lineage_plan_destroy": (None, [vp]),
        "dg_read_lineage_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz), C.POINTER(u8p), C.POINTER(sz),
                                            C.POINTER(u32), u32, C.POINTER(ReadReq), u32, C.POINTER(Buffer),
                                            C.POINTER(i32)]),
        "dg_sketch": (C.c_int, [u8p, sz, u32, u32, C.POINTER(u64)]),
        "dg_sketch_match": (C.c_int, [C.POINTER(u64), u32, C.POINTER(u64), u32, u32, C.c_int, u32, u32,
                                      C.POINTER(Match)]),
        "dg_sketch_plan_create": (C.c_int, [vp, C.POINTER(Span), u32, u32, u32, C.POINTER(vp)]),
        "dg_sketch_plan_chunk_bytes": (u32, [vp]),
        "dg_sketch_plan_run": (C.c_int, [vp, vp, vp, vp]),
        "dg_sketch_plan_set_timing": (C.c_int, [vp, C.c_int]),
        "dg_sketch_plan_stage_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.c_int]),
        "dg_sketch_plan_destroy": (None, [vp]),
        "dg_sketch_match_device": (C.c_int, [vp, vp, u32, vp, u32, u32, C.c_int, u32, u32, vp, vp]),
        "dg_sketch_batch": (C.c_int, [vp, C.POINTER(u8p), C.POINTER(sz), u32, u32, u32, C.POINTER(u64)]),
        "dg_synth_edit_pairs_device": (C.c_int, [vp, vp, vp, u32, u64, u64, u64, vp]),
        "dg_synth_shift_pairs_device": (C.c_int, [vp, u64, u32, u64, u64, u32, C.POINTER(Pair),
                                                  C.POINTER(u64), C.POINTER(u64), vp, vp, vp]),
        "dg_synth_transpose_pairs_device": (C.c_int, [vp, u64, u32, u64, u32, C.POINTER(Pair),
                                                      C.POINTER(u64), C.POINTER(u64), vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if os.environ.get("DG_LIB_VARIANT"):   # an older A/B baseline build
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    return L


lib = _load()


def _set_every(fn, plan, every):
    if fn is not None:
        plan.ctx.check(fn(plan.handle, int(every)), "timing stride")
    elif every != 1:   # (older A/B variant builds lack it)
        raise RuntimeError("this library build records events on every run only")


def status_string(code: int) -> str:
    return lib.dg_status_string(code).decode()


def _u8(b: bytes):
    return C.cast(C.c_char_p(b), C.POINTER(C.c_uint8)) if b else None


def _opts(p=SEED_LEN, q=TABLE_SIZE, buf_cap=BUF_CAP, max_table=MAX_TABLE_SIZE, flags=0,
          verbose=False, splay=False, inplace=False, policy="localmin") -> DiffOptions:
    f = flags | (verbose << OPT_VERBOSE) | (splay << OPT_SPLAY) | (inplace << OPT_INPLACE)
    f |= POLICIES[policy] << OPT_POLICY_CONSTANT
    return DiffOptions.make(p, q, buf_cap, max_table, f)


def _algo(a) -> int:
    if isinstance(a, str):
        if a not in _ALGOS:
            raise ValueError(f"Unknown algorithm: {a}")
        return _ALGOS[a]
    return int(a)


class Context:
    """A HIP device + stream + constant tables (dg_context_t)."""

    def __init__(self, device: int = -1):
        h = C.c_void_p()
        rc = lib.dg_context_create(device, C.byref(h))
        if rc:
            raise DeltaError(rc, "dg_context_create")
        self.handle = h
        # live plan handles -> their destroy function.  A plan's destroy uses its
        # context, and the collector finalises a context and its plans in any
        # order once they are garbage together, so the context, closed first,
        # destroys them (_Plan.close then finds nothing left to do)
        self._plans = {}

    def close(self):
        if self.handle:
            for h, destroy in list(self._plans.items()):
                destroy(C.c_void_p(h))
            self._plans.clear()
            lib.dg_context_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return lib.dg_context_stream(self.handle) or 0

    def set_limit(self, limit: int, value: int):
        """dg_context_set_limit (e.g. LIMIT_TABLE_POOL_BYTES; 0 = automatic)."""
        self.check(lib.dg_context_set_limit(self.handle, int(limit), int(value)), "set_limit")

    def check(self, rc: int, what: str = ""):
        if rc:
            raise DeltaError(rc, f"{what}: {lib.dg_last_error(self.handle).decode()}")


_default_ctx: Optional[Context] = None
_ctx_lock = threading.Lock()


def default_context() -> Context:
    global _default_ctx
    with _ctx_lock:
        if _default_ctx is None:
            _default_ctx = Context(-1)
        return _default_ctx


class _Plan:
    """What the plan classes share: the handle's lifetime and the stage timing
    of dg_<_prefix>_set_timing / _stage_times / _destroy."""

    _prefix = ""   # the plan's C function prefix, e.g. "dg_encode_plan"
    handle = None

    def set_timing(self, slots: int = 1):
        self.ctx.check(getattr(lib, self._prefix + "_set_timing")(self.handle, int(slots)), "set_timing")

    def stage_times(self):
        ms = (C.c_float * 8)()
        names = (C.c_char_p * 8)()
        k = getattr(lib, self._prefix + "_stage_times")(self.handle, ms, names, 8)
        return {names[i].decode(): ms[i] for i in range(k)}

    def _own(self, h):
        """Take the created handle; the context destroys it if it closes first."""
        self.handle = h
        self.ctx._plans[h.value] = getattr(lib, self._prefix + "_destroy")

    def close(self):
        if self.handle:
            destroy = self.ctx._plans.pop(self.handle.value, None)
            if destroy is not None:   # (None: the context closed before this plan and took it along)
                destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EncodePlan(_Plan):
    """Device-resident batch (dg_encode_plan_t): fixed pair geometry + options.

    ``pairs`` is a sequence of (r_off, r_len, v_off, v_len) into two device
    arenas.  ``run`` takes device addresses and an optional stream handle.
    """

    _prefix = "dg_encode_plan"

    def __init__(self, ctx: Context, algorithm, pairs: Sequence[Tuple[int, int, int, int]],
                 **opt_kw):
        self.ctx = ctx
        n = len(pairs)
        arr = (Pair * max(n, 1))(*[Pair(*p) for p in pairs])
        o = _opts(**opt_kw)
        h = C.c_void_p()
        ctx.check(lib.dg_encode_plan_create(ctx.handle, _algo(algorithm), arr, n, C.byref(o),
                                            C.byref(h)), "dg_encode_plan_create")
        self._own(h)
        self.n = n

    @property
    def output_bound(self) -> int:
        return lib.dg_encode_plan_output_bound(self.handle)

    @property
    def members(self) -> bool:
        """True when onepass runs through verified diagonal members."""
        fn = getattr(lib, "dg_encode_plan_flags", None)   # (absent from older A/B baselines)
        return bool(fn(self.handle) & 1) if fn else False

    @property
    def run_modes(self) -> tuple:
        """(runs in member mode, runs as a plain plan) so far: automatic member
        mode runs a batch whose every pair it routed to the plain chain as a
        plain plan between member-mode probes (dg_encode_plan_run_modes)."""
        fn = getattr(lib, "dg_encode_plan_run_modes", None)   # (absent from older A/B baselines)
        if not fn:
            return (0, 0)
        m, p = C.c_uint64(), C.c_uint64()
        self.ctx.check(fn(self.handle, C.byref(m), C.byref(p)), "dg_encode_plan_run_modes")
        return (m.value, p.value)

    def table_size(self, i: int) -> int:
        return lib.dg_encode_plan_table_size(self.handle, i)

    def set_timing(self, slots: int = 1, dominant_only: bool = False, every: int = 1):
        """Record per-stage events for the next runs (ring of `slots` sets);
        dominant_only: only the events around the dominant kernel(s);
        every: only every `every`-th run records them."""
        mode = getattr(lib, "dg_encode_plan_set_timing_mode", None)   # (older A/B variant builds lack it)
        if mode is not None:
            self.ctx.check(mode(self.handle, 1 if dominant_only else 0), "timing mode")
        _set_every(getattr(lib, "dg_encode_plan_set_timing_every", None), self, every)
        self.ctx.check(lib.dg_encode_plan_set_timing(self.handle, int(slots)), "set_timing")

    def copy_counts_ptr(self) -> int:
        return lib.dg_encode_plan_copy_counts_device(self.handle) or 0

    def run(self, d_ref: int, d_ver: int, d_out: int, out_cap: int, d_offsets: int,
            d_status: int, stream: int = 0):
        self.ctx.check(lib.dg_encode_plan_run(self.handle, d_ref, d_ver, d_out, out_cap, d_offsets,
                                              d_status, stream or None), "dg_encode_plan_run")


class DecodePlan(_Plan):
    """dg_decode_plan_t: batched device decode + CRC verify (C5)."""

    _prefix = "dg_decode_plan"

    def __init__(self, ctx: Context, descs: Sequence[Tuple[int, int, int, int, int, int]],
                 ignore_hash: bool = False):
        self.ctx = ctx
        n = len(descs)
        arr = (DecodeDesc * max(n, 1))(*[DecodeDesc(*d) for d in descs])
        h = C.c_void_p()
        ctx.check(lib.dg_decode_plan_create(ctx.handle, arr, n, int(ignore_hash), C.byref(h)),
                  "dg_decode_plan_create")
        self._own(h)
        self.n = n

    def run(self, d_ref: int, d_delta: int, d_out: int, d_out_len: int, d_status: int,
            stream: int = 0):
        self.ctx.check(lib.dg_decode_plan_run(self.handle, d_ref, d_delta, d_out, d_out_len, d_status,
                                              stream or None), "dg_decode_plan_run")

    def set_timing(self, slots: int = 1, every: int = 1):
        """Events around the kernel on every `every`-th run (ring of `slots`)."""
        _set_every(getattr(lib, "dg_decode_plan_set_timing_every", None), self, every)
        self.ctx.check(lib.dg_decode_plan_set_timing(self.handle, int(slots)), "set_timing")


class InplacePlan(_Plan):
    """dg_inplace_plan_t: a batch of standard deltas converted to in-place form
    on the device.  descs: (ref_off, ref_len, delta_off, delta_cap) per delta, or
    for_plan: an EncodePlan whose packed output the run converts (pass its
    offsets and status to run)."""

    _prefix = "dg_inplace_plan"

    def __init__(self, ctx: Context, descs: Optional[Sequence[Tuple[int, int, int, int]]] = None,
                 policy: str = "localmin", for_plan: Optional["EncodePlan"] = None):
        self.ctx = ctx
        h = C.c_void_p()
        if for_plan is not None:
            ctx.check(lib.dg_inplace_plan_create_for(ctx.handle, for_plan.handle, POLICIES[policy], C.byref(h)),
                      "dg_inplace_plan_create_for")
            self.n = for_plan.n
        else:
            n = len(descs)
            arr = (InplaceDesc * max(n, 1))(*[InplaceDesc(*d) for d in descs])
            ctx.check(lib.dg_inplace_plan_create(ctx.handle, arr, n, POLICIES[policy], C.byref(h)),
                      "dg_inplace_plan_create")
            self.n = n
        self._own(h)

    @property
    def output_bound(self) -> int:
        return lib.dg_inplace_plan_output_bound(self.handle)

    def run(self, d_ref: int, d_delta: int, d_out: int, out_cap: int, d_out_offsets: int, d_status: int,
            d_delta_offsets: int = 0, d_delta_status: int = 0, stream: int = 0):
        self.ctx.check(lib.dg_inplace_plan_run(self.handle, d_ref, d_delta, d_delta_offsets or None,
                                               d_delta_status or None, d_out, out_cap, d_out_offsets, d_status,
                                               stream or None), "dg_inplace_plan_run")


class UpdatePlan(_Plan):
    """dg_update_plan_t: a batch of in-place deltas applied in place on the
    device: each stream's buffer, which holds R, becomes V.  descs: (buf_off,
    buf_cap, ref_len, delta_off, delta_len) per stream.  A stream that fails
    validation (status other than 0 and 10) keeps every byte."""

    _prefix = "dg_update_plan"

    def __init__(self, ctx: Context, descs: Sequence[Tuple[int, int, int, int, int]], ignore_hash: bool = False):
        self.ctx = ctx
        n = len(descs)
        arr = (UpdateDesc * max(n, 1))(*[UpdateDesc(*d) for d in descs])
        h = C.c_void_p()
        ctx.check(lib.dg_update_plan_create(ctx.handle, arr, n, int(ignore_hash), C.byref(h)),
                  "dg_update_plan_create")
        self._own(h)
        self.n = n

    def run(self, d_buf: int, d_delta: int, d_out_len: int, d_status: int, d_delta_offsets: int = 0,
            d_delta_status: int = 0, stream: int = 0):
        self.ctx.check(lib.dg_update_plan_run(self.handle, d_buf, d_delta, d_delta_offsets or None,
                                              d_delta_status or None, d_out_len, d_status, stream or None),
                       "dg_update_plan_run")


class ComposePlan(_Plan):
    """dg_compose_plan_t: a batch of delta pairs composed on the device,
    delta(R -> V1) and delta(V1 -> V2) giving delta(R -> V2).  descs: (a_off,
    a_cap, b_off, b_cap) per pair, or for_plans: the two EncodePlans whose
    packed outputs the run composes (pass their offsets and statuses to run).
    A run with d_out = 0 and out_cap = 0 is the sizing run."""

    _prefix = "dg_compose_plan"

    def __init__(self, ctx: Context, descs: Optional[Sequence[Tuple[int, int, int, int]]] = None,
                 ignore_hash: bool = False, for_plans: Optional[Tuple["EncodePlan", "EncodePlan"]] = None):
        self.ctx = ctx
        h = C.c_void_p()
        if for_plans is not None:
            ctx.check(lib.dg_compose_plan_create_for(ctx.handle, for_plans[0].handle, for_plans[1].handle,
                                                     int(ignore_hash), C.byref(h)), "dg_compose_plan_create_for")
            self.n = for_plans[0].n
        else:
            n = len(descs)
            arr = (ComposeDesc * max(n, 1))(*[ComposeDesc(*d) for d in descs])
            ctx.check(lib.dg_compose_plan_create(ctx.handle, arr, n, int(ignore_hash), C.byref(h)),
                      "dg_compose_plan_create")
            self.n = n
        self._own(h)

    def run(self, d_a: int, d_b: int, d_out: int, out_cap: int, d_out_offsets: int, d_status: int,
            d_a_offsets: int = 0, d_a_status: int = 0, d_b_offsets: int = 0, d_b_status: int = 0, stream: int = 0):
        self.ctx.check(lib.dg_compose_plan_run(self.handle, d_a, d_a_offsets or None, d_a_status or None,
                                               d_b, d_b_offsets or None, d_b_status or None, d_out or None, out_cap,
                                               d_out_offsets, d_status, stream or None), "dg_compose_plan_run")


class InvertPlan(_Plan):
    """dg_invert_plan_t: a batch of standard deltas inverted on the device, R
    and delta(R -> V) giving delta(V -> R).  descs: (ref_off, ref_len,
    delta_off, delta_cap) per delta, or for_plan: an EncodePlan whose packed
    output the run inverts (pass its offsets and status to run)."""

    _prefix = "dg_invert_plan"

    def __init__(self, ctx: Context, descs: Optional[Sequence[Tuple[int, int, int, int]]] = None,
                 for_plan: Optional["EncodePlan"] = None):
        self.ctx = ctx
        h = C.c_void_p()
        if for_plan is not None:
            ctx.check(lib.dg_invert_plan_create_for(ctx.handle, for_plan.handle, C.byref(h)),
                      "dg_invert_plan_create_for")
            self.n = for_plan.n
        else:
            n = len(descs)
            arr = (InvertDesc * max(n, 1))(*[InvertDesc(*d) for d in descs])
            ctx.check(lib.dg_invert_plan_create(ctx.handle, arr, n, C.byref(h)), "dg_invert_plan_create")
            self.n = n
        self._own(h)

    @property
    def output_bound(self) -> int:
        return lib.dg_invert_plan_output_bound(self.handle)

    def run(self, d_ref: int, d_delta: int, d_out: int, out_cap: int, d_out_offsets: int, d_status: int,
            d_delta_offsets: int = 0, d_delta_status: int = 0, stream: int = 0):
        self.ctx.check(lib.dg_invert_plan_run(self.handle, d_ref, d_delta, d_delta_offsets or None,
                                              d_delta_status or None, d_out, out_cap, d_out_offsets, d_status,
                                              stream or None), "dg_invert_plan_run")


def encode(R: bytes, V: bytes, algorithm="onepass", p: int = SEED_LEN, q: int = TABLE_SIZE,
           buf_cap: int = BUF_CAP, max_table: int = MAX_TABLE_SIZE, splay: bool = False,
           inplace: bool = False, policy: str = "localmin",
           ctx: Optional[Context] = None) -> bytes:
    """One pair, host bytes in, DLT\\x03 bytes out (src/c/main.c:257-292)."""
    ctx = ctx or default_context()
    out = Buffer()
    o = _opts(p, q, buf_cap, max_table, splay=splay, inplace=inplace, policy=policy)
    rc = lib.dg_encode(ctx.handle, _algo(algorithm), _u8(R), len(R), _u8(V), len(V), C.byref(o),
                       C.byref(out))
    ctx.check(rc, "dg_encode")
    res = C.string_at(out.data, out.len)
    lib.dg_buffer_free(C.byref(out))
    return res


def encode_batch(pairs: Sequence[Tuple[bytes, bytes]], algorithm="onepass", p: int = SEED_LEN,
                 q: int = TABLE_SIZE, buf_cap: int = BUF_CAP, max_table: int = MAX_TABLE_SIZE,
                 ctx: Optional[Context] = None, splay: bool = False) -> List[bytes]:
    """Many pairs through the batched device path (host buffers in and out).
    splay: greedy's tie-break among the longest matches (smallest offset)."""
    ctx = ctx or default_context()
    n = len(pairs)
    if n == 0:
        return []
    keep = [(bytes(r), bytes(v)) for r, v in pairs]
    rp = (C.POINTER(C.c_uint8) * n)(*[_u8(r) for r, _ in keep])
    vp = (C.POINTER(C.c_uint8) * n)(*[_u8(v) for _, v in keep])
    rl = (C.c_size_t * n)(*[len(r) for r, _ in keep])
    vl = (C.c_size_t * n)(*[len(v) for _, v in keep])
    outs = (Buffer * n)()
    st = (C.c_int32 * n)()
    o = _opts(p, q, buf_cap, max_table, splay=splay)
    ctx.check(lib.dg_encode_batch(ctx.handle, _algo(algorithm), rp, rl, vp, vl, n, C.byref(o), outs,
                                  st), "dg_encode_batch")
    res = []
    for i in range(n):
        if st[i]:
            raise DeltaError(st[i], f"pair {i}")
        res.append(C.string_at(outs[i].data, outs[i].len))
        lib.dg_buffer_free(C.byref(outs[i]))
    return res


def encode_pipelined(pairs: Sequence[Tuple[bytes, bytes]], algorithm="onepass", p: int = SEED_LEN,
                     q: int = TABLE_SIZE, buf_cap: int = BUF_CAP, max_table: int = MAX_TABLE_SIZE,
                     chunk_bytes: int = 0, pinned: bool = False, align: int = 16, out_cap: Optional[int] = None,
                     ctx: Optional[Context] = None, ctxs: Optional[Sequence[Context]] = None,
                     splay: bool = False, inplace: bool = False, policy: str = "localmin") -> List[bytes]:
    """Many pairs host-to-host through dg_encode_pipelined (chunked, two chunks in
    flight).  The pairs are laid out in host arenas `align` bytes apart, pinned
    (dg_host_alloc) or pageable (bytearray).  ctxs: one context per device,
    through dg_encode_pipelined_multi (byte-balanced pair ranges, one host
    thread per device, deltas packed in pair order).  inplace: every chunk is
    converted to in-place deltas on the device after its encode (policy)."""
    ctx = ctx or (ctxs[0] if ctxs else default_context())
    n = len(pairs)
    if n == 0:
        return []
    lay, rt, vt = [], 0, 0
    for r, v in pairs:   # each pair at the next multiple of `align` (1: packed, unaligned)
        ro, vo = (rt + align - 1) // align * align, (vt + align - 1) // align * align
        lay.append((ro, len(r), vo, len(v)))
        rt, vt = ro + len(r), vo + len(v)
    cap = out_cap if out_cap is not None else (2 if inplace else 1) * sum(len(v) for _, v in pairs) + 64 * n + 64
    bufs = []

    def host(nbytes):
        if pinned:
            h = C.c_void_p()
            ctx.check(lib.dg_host_alloc(ctx.handle, max(nbytes, 1), C.byref(h)), "dg_host_alloc")
            bufs.append(h)
            return h.value
        b = (C.c_uint8 * max(nbytes, 1))()
        bufs.append(b)
        return C.addressof(b)

    try:
        hr, hv, ho = host(rt), host(vt), host(cap)
        for (r, v), (ro, _, vo, _) in zip(pairs, lay):
            C.memmove(hr + ro, bytes(r), len(r))
            C.memmove(hv + vo, bytes(v), len(v))
        pa = (Pair * n)(*[Pair(*x) for x in lay])
        offs = (C.c_uint64 * (n + 1))()
        st = (C.c_int32 * n)()
        o = _opts(p, q, buf_cap, max_table, splay=splay, inplace=inplace, policy=policy)
        if ctxs:
            hs = (C.c_void_p * len(ctxs))(*[c.handle for c in ctxs])
            ctx.check(lib.dg_encode_pipelined_multi(hs, len(ctxs), _algo(algorithm), hr, hv, pa, n, C.byref(o),
                                                    chunk_bytes, ho, cap, offs, st), "dg_encode_pipelined_multi")
        else:
            ctx.check(lib.dg_encode_pipelined(ctx.handle, _algo(algorithm), hr, hv, pa, n, C.byref(o), chunk_bytes,
                                              ho, cap, offs, st), "dg_encode_pipelined")
        res = []
        for i in range(n):
            if st[i]:
                raise DeltaError(st[i], f"pair {i}")
            res.append(C.string_at(ho + offs[i], offs[i + 1] - offs[i]))
        return res
    finally:
        if pinned:
            for h in bufs:
                lib.dg_host_free(h)


def make_inplace(R: bytes, delta: bytes, policy: str = "localmin", stats: bool = False):
    """main.c `inplace` (:427-480): standard delta -> in-place delta, host only."""
    out = Buffer()
    st = InplaceStats()
    rc = lib.dg_make_inplace(_u8(R), len(R), _u8(delta), len(delta), POLICIES[policy], C.byref(out),
                             C.byref(st))
    if rc:
        raise DeltaError(rc, "dg_make_inplace")
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    if stats:
        return res, {k: getattr(st, k) for k, _ in InplaceStats._fields_}
    return res


def make_inplace_batch(items: Sequence[Tuple[bytes, bytes]], policy: str = "localmin",
                       ctx: Optional[Context] = None) -> List[bytes]:
    """(R, standard delta) pairs -> in-place deltas, converted on the device in
    one batch (dg_make_inplace_batch); equal to make_inplace item by item."""
    ctx = ctx or default_context()
    n = len(items)
    if n == 0:
        return []
    keep = [(bytes(r), bytes(d)) for r, d in items]
    rp = (C.POINTER(C.c_uint8) * n)(*[_u8(r) for r, _ in keep])
    dp = (C.POINTER(C.c_uint8) * n)(*[_u8(d) for _, d in keep])
    rl = (C.c_size_t * n)(*[len(r) for r, _ in keep])
    dl = (C.c_size_t * n)(*[len(d) for _, d in keep])
    outs = (Buffer * n)()
    st = (C.c_int32 * n)()
    ctx.check(lib.dg_make_inplace_batch(ctx.handle, rp, rl, dp, dl, n, POLICIES[policy], outs, st),
              "dg_make_inplace_batch")
    res, bad = [], None
    for i in range(n):
        if st[i] and bad is None:
            bad = i
        res.append(C.string_at(outs[i].data, outs[i].len) if outs[i].len else b"")
        lib.dg_buffer_free(C.byref(outs[i]))
    if bad is not None:
        raise DeltaError(st[bad], f"delta {bad}")
    return res


def compose(A: bytes, B: bytes, ignore_hash: bool = False) -> bytes:
    """delta(R -> V1) and delta(V1 -> V2) -> delta(R -> V2) in normal form
    (dg_compose): host only, and none of R, V1 or V2 is needed."""
    out = Buffer()
    rc = lib.dg_compose(_u8(A), len(A), _u8(B), len(B), int(ignore_hash), C.byref(out))
    if rc:
        raise DeltaError(rc, "dg_compose")
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    return res


def compose_batch(items: Sequence[Tuple[bytes, bytes]], ignore_hash: bool = False,
                  ctx: Optional[Context] = None, status: bool = False):
    """(A, B) delta pairs composed on the device in one batch
    (dg_compose_batch); equal to compose item by item.  Raises DeltaError for
    the first failing item; with status=True returns (results, statuses)
    instead, a failed item's result being b""."""
    ctx = ctx or default_context()
    n = len(items)
    if n == 0:
        return ([], []) if status else []
    keep = [(bytes(a), bytes(b)) for a, b in items]
    ap = (C.POINTER(C.c_uint8) * n)(*[_u8(a) for a, _ in keep])
    bp = (C.POINTER(C.c_uint8) * n)(*[_u8(b) for _, b in keep])
    al = (C.c_size_t * n)(*[len(a) for a, _ in keep])
    bl = (C.c_size_t * n)(*[len(b) for _, b in keep])
    outs = (Buffer * n)()
    st = (C.c_int32 * n)()
    ctx.check(lib.dg_compose_batch(ctx.handle, ap, al, bp, bl, n, int(ignore_hash), outs, st), "dg_compose_batch")
    res = []
    for i in range(n):
        res.append(C.string_at(outs[i].data, outs[i].len) if outs[i].len else b"")
        lib.dg_buffer_free(C.byref(outs[i]))
    if status:
        return res, list(st)
    for i in range(n):
        if st[i]:
            raise DeltaError(st[i], f"pair {i}")
    return res


def invert(R: bytes, A: bytes) -> bytes:
    """R and A = delta(R -> V) -> delta(V -> R) in normal form (dg_invert):
    host only, and V is not needed."""
    out = Buffer()
    rc = lib.dg_invert(_u8(R), len(R), _u8(A), len(A), C.byref(out))
    if rc:
        raise DeltaError(rc, "dg_invert")
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    return res


def invert_batch(items: Sequence[Tuple[bytes, bytes]], ctx: Optional[Context] = None, status: bool = False):
    """(R, delta(R -> V)) pairs inverted on the device in one batch
    (dg_invert_batch); equal to invert item by item.  Raises DeltaError for
    the first failing item; with status=True returns (results, statuses)
    instead, a failed item's result being b""."""
    ctx = ctx or default_context()
    n = len(items)
    if n == 0:
        return ([], []) if status else []
    keep = [(bytes(r), bytes(d)) for r, d in items]
    rp = (C.POINTER(C.c_uint8) * n)(*[_u8(r) for r, _ in keep])
    dp = (C.POINTER(C.c_uint8) * n)(*[_u8(d) for _, d in keep])
    rl = (C.c_size_t * n)(*[len(r) for r, _ in keep])
    dl = (C.c_size_t * n)(*[len(d) for _, d in keep])
    outs = (Buffer * n)()
    st = (C.c_int32 * n)()
    ctx.check(lib.dg_invert_batch(ctx.handle, rp, rl, dp, dl, n, outs, st), "dg_invert_batch")
    res = []
    for i in range(n):
        res.append(C.string_at(outs[i].data, outs[i].len) if outs[i].len else b"")
        lib.dg_buffer_free(C.byref(outs[i]))
    if status:
        return res, list(st)
    for i in range(n):
        if st[i]:
            raise DeltaError(st[i], f"delta {i}")
    return res


# ── one large pair: segments, windows and the splice of the segments' deltas ──

def _pairs(items):
    n = len(items)
    return (Pair * max(n, 1))(*[Pair(*map(int, p)) for p in items])


def segment_pairs(wholes, seg_bytes: int = 1 << 20, window_bytes: int = 1 << 20):
    """The fixed segmentation rule (dg_segment_pairs, host only).  wholes: one
    (r_off, r_len, v_off, v_len) or a sequence of them; returns (segments,
    seg_first): the segments of every group as (r_off, r_len, v_off, v_len),
    group after group, and each group's first segment (n_groups + 1 entries)."""
    if wholes and isinstance(wholes[0], int):
        wholes = [wholes]
    n = len(wholes)
    wa = _pairs(wholes)
    first = (C.c_uint32 * (n + 1))()
    rc = lib.dg_segment_pairs(wa, n, seg_bytes, window_bytes, None, 0, first)
    if rc:
        raise DeltaError(rc, "dg_segment_pairs")
    total = first[n]
    segs = (Pair * max(total, 1))()
    rc = lib.dg_segment_pairs(wa, n, seg_bytes, window_bytes, segs, total, first)
    if rc:
        raise DeltaError(rc, "dg_segment_pairs")
    return [(s.r_off, s.r_len, s.v_off, s.v_len) for s in segs[:total]], list(first)


def splice(segments, deltas: Sequence[bytes], whole, src_crc: bytes, seg_status=None) -> bytes:
    """The deltas of one group's segments -> one standard delta of the whole
    pair, in normal form (dg_splice): host only, and none of R or V is needed.
    src_crc: the 8 header bytes of CRC-64/XZ(R)."""
    n = len(segments)
    keep = [bytes(d) for d in deltas]
    if len(keep) != n or len(src_crc) != 8:
        raise ValueError("one delta per segment and an 8-byte src_crc")
    dp = (C.POINTER(C.c_uint8) * max(n, 1))(*[_u8(d) for d in keep])
    dl = (C.c_size_t * max(n, 1))(*[len(d) for d in keep])
    st = (C.c_int32 * max(n, 1))(*seg_status) if seg_status is not None else None
    out = Buffer()
    rc = lib.dg_splice(_pairs([whole]), _pairs(segments), n, dp, dl, st, (C.c_uint8 * 8)(*src_crc), C.byref(out))
    if rc:
        raise DeltaError(rc, "dg_splice")
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    return res


class SplicePlan(_Plan):
    """dg_splice_plan_t: the segment deltas of a batch of large pairs spliced on
    the device into one standard delta per pair.  segments, wholes: (r_off,
    r_len, v_off, v_len); seg_first: n_groups + 1 entries; caps: the most bytes
    each segment's delta may have (None: no bound), or for_plan: the EncodePlan
    that encodes the segments (pass its offsets and status to run)."""

    _prefix = "dg_splice_plan"

    def __init__(self, ctx: Context, wholes, seg_first, segments=None, caps=None,
                 for_plan: Optional["EncodePlan"] = None):
        self.ctx = ctx
        h = C.c_void_p()
        ng = len(wholes)
        fa = (C.c_uint32 * (ng + 1))(*seg_first)
        if for_plan is not None:
            ctx.check(lib.dg_splice_plan_create_for(ctx.handle, for_plan.handle, _pairs(wholes), fa, ng, C.byref(h)),
                      "dg_splice_plan_create_for")
            self.n_seg = for_plan.n
        else:
            ns = len(segments)
            ca = (C.c_uint64 * max(ns, 1))(*caps) if caps is not None else None
            ctx.check(lib.dg_splice_plan_create(ctx.handle, _pairs(segments), ns, _pairs(wholes), fa, ng, ca, C.byref(h)),
                      "dg_splice_plan_create")
            self.n_seg = ns
        self._own(h)
        self.n = ng

    @property
    def output_bound(self) -> int:
        return lib.dg_splice_plan_output_bound(self.handle)

    def run(self, d_deltas: int, d_offsets: int, d_src_crc: int, d_out: int, out_cap: int, d_out_offsets: int,
            d_status: int, d_seg_status: int = 0, stream: int = 0):
        self.ctx.check(lib.dg_splice_plan_run(self.handle, d_deltas or None, d_offsets or None, d_seg_status or None,
                                              d_src_crc or None, d_out or None, out_cap, d_out_offsets, d_status,
                                              stream or None), "dg_splice_plan_run")


def splice_batch(groups, ctx: Optional[Context] = None, status: bool = False):
    """Groups of (segments, deltas, whole, src_crc[, seg_status]) spliced on the
    device in one batch (dg_splice_batch); equal to splice group by group.
    Raises DeltaError for the first failing group; with status=True returns
    (results, statuses) instead, a failed group's result being b""."""
    ctx = ctx or default_context()
    ng = len(groups)
    if ng == 0:
        return ([], []) if status else []
    segs, keep, first, sst, any_st = [], [], [0], [], False
    for grp in groups:
        segs += list(grp[0])
        keep += [bytes(d) for d in grp[1]]
        if len(grp) > 4 and grp[4] is not None:
            sst += list(grp[4])
            any_st = True
        else:
            sst += [0] * len(grp[0])
        first.append(len(segs))
    if len(keep) != len(segs):
        raise ValueError("one delta per segment")
    ns = len(segs)
    dp = (C.POINTER(C.c_uint8) * max(ns, 1))(*[_u8(d) for d in keep])
    dl = (C.c_size_t * max(ns, 1))(*[len(d) for d in keep])
    crc = b"".join(bytes(grp[3]) for grp in groups)
    outs = (Buffer * ng)()
    st = (C.c_int32 * ng)()
    ctx.check(lib.dg_splice_batch(ctx.handle, _pairs([grp[2] for grp in groups]), ng, _pairs(segs),
                                  (C.c_uint32 * (ng + 1))(*first), dp, dl,
                                  (C.c_int32 * max(ns, 1))(*sst) if any_st else None, _u8(crc), outs, st),
              "dg_splice_batch")
    res = []
    for i in range(ng):
        res.append(C.string_at(outs[i].data, outs[i].len) if outs[i].len else b"")
        lib.dg_buffer_free(C.byref(outs[i]))
    if status:
        return res, list(st)
    for i in range(ng):
        if st[i]:
            raise DeltaError(st[i], f"group {i}")
    return res


def sketch_windows(R: bytes, V: bytes, seg_bytes: int = 1 << 20, window_bytes: int = 1 << 20, host: bool = False,
                   p: int = SEED_LEN, k: int = SKETCH_BINS, ctx: Optional[Context] = None):
    """The segments of (R, V) with each window chosen by resemblance instead of
    by position, for drift: an insertion longer than the window starves every
    later fixed window.  Candidate windows R[max(0, cS - W), min(|R|, cS + S + W))
    for c = 0 .. ceil(|R| / S) - 1 are sketched, V's segments are the targets,
    matched with mode "all"; a target without a match keeps the fixed rule's
    window.  host=True sketches and matches with the host functions.  Returns
    the segments as segment_pairs does."""
    S, W = seg_bytes, window_bytes
    segs, _ = segment_pairs((0, len(R), 0, len(V)), S, W)
    cands = [(max(0, c * S - W), min(len(R), c * S + S + W)) for c in range((len(R) + S - 1) // S)]
    if not cands:
        return segs
    bufs = [R[a:b] for a, b in cands] + [V[vo:vo + vl] for _, _, vo, vl in segs]
    if host:
        sk = [sketch(b, p, k) for b in bufs]
        best = match_sketches(sk[len(cands):], sk[:len(cands)], k, "all")
    else:
        ctx = ctx or default_context()
        sk = sketch_batch(bufs, p, k, ctx)
        best = match_sketches(sk[len(cands):], sk[:len(cands)], k, "all")
    out = []
    for seg, (b, _, _) in zip(segs, best):
        if b == MATCH_NONE:
            out.append(seg)
        else:
            out.append((cands[b][0], cands[b][1] - cands[b][0], seg[2], seg[3]))
    return out


def encode_large(R: bytes, V: bytes, algorithm="onepass", seg_bytes: int = 1 << 20, window_bytes: int = 1 << 20,
                 windows: str = "fixed", p: int = SEED_LEN, q: int = TABLE_SIZE, buf_cap: int = BUF_CAP,
                 max_table: int = MAX_TABLE_SIZE, splay: bool = False, inplace: bool = False,
                 policy: str = "localmin", ctx: Optional[Context] = None) -> bytes:
    """One large pair encoded as segments of V against windows of R, the
    segment deltas spliced on the device into one standard delta (every wave
    of the device at work instead of one).  windows="fixed": the rule of
    segment_pairs, all on the device (dg_encode_large); "sketch" /
    "sketch_host": windows chosen by sketch_windows, the segments encoded as
    one batch and spliced on the device."""
    ctx = ctx or default_context()
    if windows == "fixed":
        out = Buffer()
        o = _opts(p, q, buf_cap, max_table, splay=splay, inplace=inplace, policy=policy)
        ctx.check(lib.dg_encode_large(ctx.handle, _algo(algorithm), _u8(R), len(R), _u8(V), len(V), C.byref(o),
                                      seg_bytes, window_bytes, C.byref(out)), "dg_encode_large")
        res = C.string_at(out.data, out.len)
        lib.dg_buffer_free(C.byref(out))
        return res
    if windows not in ("sketch", "sketch_host"):
        raise ValueError(f"Unknown window rule: {windows}")
    segs = sketch_windows(R, V, seg_bytes, window_bytes, host=windows == "sketch_host", p=p, ctx=ctx)
    deltas = encode_batch([(R[ro:ro + rl], V[vo:vo + vl]) for ro, rl, vo, vl in segs], algorithm, p, q, buf_cap,
                          max_table, ctx, splay)
    d = splice_batch([(segs, deltas, (0, len(R), 0, len(V)), crc64_xz(R, ctx))], ctx)[0]
    return make_inplace(R, d, policy) if inplace else d


class ReadPlan(_Plan):
    """dg_read_plan_t: byte ranges of versions kept as R plus a standard delta,
    read on the device without rebuilding the versions.  streams: (ref_off,
    ref_len, delta_off, delta_len) per stream.  index() parses every stream
    once (again whenever the delta bytes change); run() serves a device array
    of ReadReq, one block per request."""

    _prefix = "dg_read_plan"

    def __init__(self, ctx: Context, streams: Sequence[Tuple[int, int, int, int]], max_requests: int):
        self.ctx = ctx
        n = len(streams)
        arr = (ReadStream * max(n, 1))(*[ReadStream(*s) for s in streams])
        h = C.c_void_p()
        ctx.check(lib.dg_read_plan_create(ctx.handle, arr, n, int(max_requests), C.byref(h)), "dg_read_plan_create")
        self._own(h)
        self.n = n
        self.max_requests = int(max_requests)

    def index(self, d_delta: int, d_stream_status: int = 0, d_delta_offsets: int = 0, d_delta_status: int = 0,
              stream: int = 0):
        self.ctx.check(lib.dg_read_plan_index(self.handle, d_delta, d_delta_offsets or None, d_delta_status or None,
                                              d_stream_status or None, stream or None), "dg_read_plan_index")

    def run(self, d_ref: int, d_delta: int, d_reqs: int, n_req: int, d_out: int, d_out_len: int, d_status: int,
            stream: int = 0):
        self.ctx.check(lib.dg_read_plan_run(self.handle, d_ref or None, d_delta or None, d_reqs or None, int(n_req),
                                            d_out or None, d_out_len or None, d_status or None, stream or None),
                       "dg_read_plan_run")

    def chunk_index(self, chunk_bytes: int = 0):
        """Once per plan: fixes the chunk size (a multiple of 4096; 0: the
        default) and allocates the chunked index pass's work memory."""
        self.ctx.check(lib.dg_read_plan_chunk_index(self.handle, int(chunk_bytes)), "dg_read_plan_chunk_index")

    def index_chunked(self, d_delta: int, d_stream_status: int = 0, d_delta_offsets: int = 0, d_delta_status: int = 0,
                      stream: int = 0):
        """index() with every stream cut into chunks and parsed by many blocks; the same index."""
        self.ctx.check(lib.dg_read_plan_index_chunked(self.handle, d_delta, d_delta_offsets or None,
                                                      d_delta_status or None, d_stream_status or None, stream or None),
                       "dg_read_plan_index_chunked")

    def index_get(self, i: int) -> bytes:
        """Stream i's index as the last pass left it: the 32-byte head and, for a
        stream whose status is 0, its entries (for comparing passes; the layout is private)."""
        need = C.c_uint64(0)
        rc = lib.dg_read_plan_index_get(self.handle, int(i), None, 0, C.byref(need))
        if rc != 7:   # DG_ERR_CAPACITY: the size
            self.ctx.check(rc or 12, "dg_read_plan_index_get")
        buf = (C.c_uint8 * need.value)()
        self.ctx.check(lib.dg_read_plan_index_get(self.handle, int(i), buf, need.value, C.byref(need)),
                       "dg_read_plan_index_get")
        return bytes(buf[:need.value])

    def set_index_timing(self, slots: int = 1):
        self.ctx.check(lib.dg_read_plan_index_set_timing(self.handle, int(slots)), "dg_read_plan_index_set_timing")

    def index_stage_times(self) -> dict:
        """Mean milliseconds of the chunked passes' stages: map, resolve, fill, total."""
        ms = (C.c_float * 8)()
        names = (C.c_char_p * 8)()
        k = lib.dg_read_plan_index_stage_times(self.handle, ms, names, 8)
        return {names[j].decode(): float(ms[j]) for j in range(k)}


def tile_requests(version_size: int, tile_bytes: int = 0) -> List[Tuple[int, int, int]]:
    """The (off, length, out_off) read requests of stream 0 that tile
    [0, version_size) (dg_tile_requests): host arithmetic, no GPU."""
    n = C.c_uint32(0)
    rc = lib.dg_tile_requests(int(version_size), int(tile_bytes), None, 0, C.byref(n))
    if rc not in (0, 7):
        raise DeltaError(rc, "dg_tile_requests")
    arr = (ReadReq * max(n.value, 1))()
    rc = lib.dg_tile_requests(int(version_size), int(tile_bytes), arr, n.value, C.byref(n))
    if rc:
        raise DeltaError(rc, "dg_tile_requests")
    return [(arr[j].off, arr[j].len, arr[j].out_off) for j in range(n.value)]


def decode_large(R: bytes, delta: bytes, ignore_hash: bool = False, chunk_bytes: int = 0, tile_bytes: int = 0,
                 ctx: Optional[Context] = None) -> bytes:
    """decode() of one delta by the whole GPU (dg_decode_large): a chunked
    index of the stream, then V read as tiles; the same bytes and statuses."""
    ctx = ctx or default_context()
    out = Buffer()
    rc = lib.dg_decode_large(ctx.handle, _u8(R), len(R), _u8(delta), len(delta), int(ignore_hash), int(chunk_bytes),
                             int(tile_bytes), C.byref(out))
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    ctx.check(rc, "dg_decode_large")
    return res


def read_range(R: bytes, delta: bytes, off: int, length: int) -> bytes:
    """Bytes [off, off + length) of the version delta makes of R, clipped to the
    version (dg_read): host only, no CRC check."""
    out = Buffer()
    rc = lib.dg_read(_u8(R), len(R), _u8(delta), len(delta), int(off), int(length), C.byref(out))
    if rc:
        raise DeltaError(rc, "dg_read")
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    return res


def _read_batch(items, parents, requests, ctx, status):
    """read_ranges (parents None: dg_read_batch; every R is bytes) and
    read_lineage_batch (dg_read_lineage_batch; an R may be None): the items and
    the requests to C arrays, the call, the results out of the library's
    buffers; raises, or returns the statuses."""
    ctx = ctx or default_context()
    n, m = len(items), len(requests)
    if m == 0:
        return ([], []) if status else []
    keep = [(bytes(r if parents is None else r or b""), bytes(d)) for r, d in items]
    rp = (C.POINTER(C.c_uint8) * max(n, 1))(*[_u8(r) for r, _ in keep])
    dp = (C.POINTER(C.c_uint8) * max(n, 1))(*[_u8(d) for _, d in keep])
    rl = (C.c_size_t * max(n, 1))(*[len(r) for r, _ in keep])
    dl = (C.c_size_t * max(n, 1))(*[len(d) for _, d in keep])
    rq = (ReadReq * m)(*[ReadReq(int(s), int(o), int(ln), 0, 0) for s, o, ln in requests])
    outs = (Buffer * m)()
    st = (C.c_int32 * m)()
    if parents is None:
        rc, what = lib.dg_read_batch(ctx.handle, rp, rl, dp, dl, n, rq, m, outs, st), "dg_read_batch"
    else:
        par = (C.c_uint32 * max(n, 1))(*[int(p) for p in parents])
        rc = lib.dg_read_lineage_batch(ctx.handle, rp, rl, dp, dl, par, n, rq, m, outs, st)
        what = "dg_read_lineage_batch"
    ctx.check(rc, what)
    res = []
    for j in range(m):
        res.append(C.string_at(outs[j].data, outs[j].len) if outs[j].len else b"")
        lib.dg_buffer_free(C.byref(outs[j]))
    if status:
        return res, list(st)
    for j in range(m):
        if st[j]:
            raise DeltaError(st[j], f"request {j}")
    return res


def read_ranges(items: Sequence[Tuple[bytes, bytes]], requests: Sequence[Tuple[int, int, int]],
                ctx: Optional[Context] = None, status: bool = False):
    """requests (stream, off, length) read from the (R, delta) items on the
    device in one batch (dg_read_batch); equal to read_range request by
    request.  Raises DeltaError for the first failing request; with
    status=True returns (results, statuses) instead, a failed request's result
    being b""."""
    return _read_batch(items, None, requests, ctx, status)


LINEAGE_BASE = 0xFFFFFFFF   # DG_LINEAGE_BASE
LINEAGE_MAX_DEPTH = 64      # DG_LINEAGE_MAX_DEPTH


def lineage_work_items() -> int:
    """Work items of a lineage request's stack on the device (dg_lineage_work_items)."""
    return int(lib.dg_lineage_work_items())


class LineagePlan(_Plan):
    """dg_lineage_plan_t: byte ranges of versions that are several standard
    deltas away from a whole buffer, read on the device without rebuilding any
    version.  reads: the ReadPlan whose streams these are and whose index
    passes index them (it must outlive this plan); parents[i]: LINEAGE_BASE or
    the stream that makes stream i's reference.  run() serves a device array of
    ReadReq, one block per request, as ReadPlan.run does."""

    _prefix = "dg_lineage_plan"

    def __init__(self, reads: "ReadPlan", parents: Sequence[int], max_requests: int):
        self.ctx = reads.ctx
        self.reads = reads
        n = len(parents)
        arr = (C.c_uint32 * max(n, 1))(*[int(p) for p in parents])
        h = C.c_void_p()
        self.ctx.check(lib.dg_lineage_plan_create(reads.handle, arr, int(max_requests), C.byref(h)),
                       "dg_lineage_plan_create")
        self._own(h)
        self.max_requests = int(max_requests)

    def run(self, d_ref: int, d_delta: int, d_reqs: int, n_req: int, d_out: int, d_out_len: int, d_status: int,
            stream: int = 0):
        self.ctx.check(lib.dg_lineage_plan_run(self.handle, d_ref or None, d_delta or None, d_reqs or None, int(n_req),
                                               d_out or None, d_out_len or None, d_status or None, stream or None),
                       "dg_lineage_plan_run")


def read_lineage(R: bytes, deltas: Sequence[bytes], off: int, length: int) -> bytes:
    """Bytes [off, off + length) of the version that deltas[0] on R, deltas[1]
    on that version, ... make, clipped to it (dg_read_lineage): host only, no
    CRC check, no version rebuilt."""
    keep = [bytes(d) for d in deltas]
    k = len(keep)
    dp = (C.POINTER(C.c_uint8) * max(k, 1))(*[_u8(d) for d in keep])
    dl = (C.c_size_t * max(k, 1))(*[len(d) for d in keep])
    out = Buffer()
    rc = lib.dg_read_lineage(_u8(R), len(R), dp, dl, k, int(off), int(length), C.byref(out))
    if rc:
        raise DeltaError(rc, "dg_read_lineage")
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    return res


def read_lineage_batch(items: Sequence[Tuple[Optional[bytes], bytes]], parents: Sequence[int],
                       requests: Sequence[Tuple[int, int, int]], ctx: Optional[Context] = None, status: bool = False):
    """requests (stream, off, length) read on the device in one batch
    (dg_read_lineage_batch) from items (R or None, delta): stream i's delta
    applies to R where parents[i] is LINEAGE_BASE, else to the version of
    stream parents[i] (its R is ignored).  Equal to read_lineage request by
    request.  Raises DeltaError for the first failing request; with
    status=True returns (results, statuses) instead, a failed request's result
    being b""."""
    return _read_batch(items, parents, requests, ctx, status)


class SketchPlan(_Plan):
    """dg_sketch_plan_t: the resemblance sketches of a batch of spans of one
    device arena.  spans: (off, len) per buffer; run writes span i's k words
    at d_sketch + 8 k i."""

    _prefix = "dg_sketch_plan"

    def __init__(self, ctx: Context, spans: Sequence[Tuple[int, int]], p: int = SEED_LEN, k: int = SKETCH_BINS):
        self.ctx = ctx
        n = len(spans)
        arr = (Span * max(n, 1))(*[Span(*s) for s in spans])
        h = C.c_void_p()
        ctx.check(lib.dg_sketch_plan_create(ctx.handle, arr, n, p, k, C.byref(h)), "dg_sketch_plan_create")
        self._own(h)
        self.n, self.p, self.k = n, p, k

    @property
    def chunk_bytes(self) -> int:
        return lib.dg_sketch_plan_chunk_bytes(self.handle)

    def run(self, d_arena: int, d_sketch: int, stream: int = 0):
        self.ctx.check(lib.dg_sketch_plan_run(self.handle, d_arena or None, d_sketch or None, stream or None),
                       "dg_sketch_plan_run")


def _match_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in _MATCH_MODES:
            raise ValueError(f"Unknown match mode: {mode}")
        return _MATCH_MODES[mode]
    return int(mode)


def sketch(data: bytes, p: int = SEED_LEN, k: int = SKETCH_BINS) -> List[int]:
    """The resemblance sketch of one buffer (dg_sketch): k words, host only."""
    out = (C.c_uint64 * max(k, 1))()
    rc = lib.dg_sketch(_u8(data), len(data), p, k, out)
    if rc:
        raise DeltaError(rc, "dg_sketch")
    return list(out)


def sketch_batch(buffers: Sequence[bytes], p: int = SEED_LEN, k: int = SKETCH_BINS,
                 ctx: Optional[Context] = None) -> List[List[int]]:
    """The sketches of many buffers, computed on the device in one batch
    (dg_sketch_batch); equal to sketch buffer by buffer."""
    ctx = ctx or default_context()
    n = len(buffers)
    keep = [bytes(b) for b in buffers]
    bp = (C.POINTER(C.c_uint8) * max(n, 1))(*[_u8(b) for b in keep])
    bl = (C.c_size_t * max(n, 1))(*[len(b) for b in keep])
    out = (C.c_uint64 * max(n * k, 1))()
    ctx.check(lib.dg_sketch_batch(ctx.handle, bp, bl, n, p, k, out), "dg_sketch_batch")
    return [list(out[i * k:(i + 1) * k]) for i in range(n)]


def match_sketches(targets: Sequence[Sequence[int]], cands: Sequence[Sequence[int]], k: int = SKETCH_BINS,
                   mode="all", target_base: int = 0, min_equal: int = 1) -> List[Tuple[int, int, int]]:
    """(best, equal, used) per target sketch among the candidate sketches
    (dg_sketch_match, host only); best is MATCH_NONE when nothing is eligible."""
    n_t, n_c = len(targets), len(cands)
    ta = (C.c_uint64 * max(n_t * k, 1))(*[w for s in targets for w in s])
    ca = (C.c_uint64 * max(n_c * k, 1))(*[w for s in cands for w in s])
    out = (Match * max(n_t, 1))()
    rc = lib.dg_sketch_match(ta, n_t, ca, n_c, k, _match_mode(mode), target_base, min_equal, out)
    if rc:
        raise DeltaError(rc, "dg_sketch_match")
    return [(out[i].best, out[i].equal, out[i].used) for i in range(n_t)]


def match_sketches_device(ctx: Context, d_targets: int, n_t: int, d_cands: int, n_c: int, d_out: int,
                          k: int = SKETCH_BINS, mode="all", target_base: int = 0, min_equal: int = 1, stream: int = 0):
    """match_sketches on device arrays (dg_sketch_match_device): one launch on
    the stream; d_out receives n_t dg_match_t (four uint32 each)."""
    ctx.check(lib.dg_sketch_match_device(ctx.handle, d_targets or None, n_t, d_cands or None, n_c, k, _match_mode(mode),
                                         target_base, min_equal, d_out or None, stream or None),
              "dg_sketch_match_device")


def pick_bases(buffers: Sequence[bytes], mode="earlier", p: int = SEED_LEN, k: int = SKETCH_BINS,
               min_equal: int = 1, ctx: Optional[Context] = None) -> List[Tuple[Optional[int], int, int]]:
    """For every buffer the most resembling other one as its base: (best | None,
    equal, used).  The sketches and the matching run on the device; in
    "earlier" mode a base always comes before its buffer, so the assignment has
    no cycle."""
    import numpy as np
    import torch
    ctx = ctx or default_context()
    n = len(buffers)
    if n == 0:
        return []
    words = np.array(sketch_batch(buffers, p, k, ctx), dtype=np.uint64).view(np.int64)
    sk = torch.from_numpy(words).cuda()
    out = torch.zeros(n * 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()   # (torch filled the buffers on its own stream)
    match_sketches_device(ctx, sk.data_ptr(), n, sk.data_ptr(), n, out.data_ptr(), k, mode, 0, min_equal)
    torch.cuda.ExternalStream(ctx.stream).synchronize()
    res = (out.cpu().view(n, 4).to(torch.int64) & 0xFFFFFFFF).tolist()
    return [(None if b == MATCH_NONE else b, e, u) for b, e, u, _ in res]


def update_batch(items: Sequence[Tuple[bytes, bytes]], ignore_hash: bool = False,
                 ctx: Optional[Context] = None, status: bool = False):
    """(R, in-place delta) pairs -> V, each applied on the device in a buffer of
    max(|R|, version size) bytes that holds R (dg_update_batch).  Raises
    DeltaError for the first failing item, as make_inplace_batch does; with
    status=True returns (results, statuses) instead, a result being None where
    the item's buffer was left as it was (every status but 0 and 10)."""
    ctx = ctx or default_context()
    n = len(items)
    if n == 0:
        return ([], []) if status else []
    keep = [(bytes(r), bytes(d)) for r, d in items]
    caps = []
    for r, d in keep:
        vs = int.from_bytes(d[5:9], "big") if len(d) >= 25 else 0
        caps.append(max(len(r), vs, 1))
    bufs = [(C.c_uint8 * cap)() for cap in caps]
    for b, (r, _) in zip(bufs, keep):
        C.memmove(b, r, len(r))
    bp = (C.POINTER(C.c_uint8) * n)(*[C.cast(b, C.POINTER(C.c_uint8)) for b in bufs])
    dp = (C.POINTER(C.c_uint8) * n)(*[_u8(d) for _, d in keep])
    rl = (C.c_size_t * n)(*[len(r) for r, _ in keep])
    bc = (C.c_size_t * n)(*caps)
    dl = (C.c_size_t * n)(*[len(d) for _, d in keep])
    ol = (C.c_size_t * n)()
    st = (C.c_int32 * n)()
    ctx.check(lib.dg_update_batch(ctx.handle, bp, rl, bc, dp, dl, n, int(ignore_hash), ol, st), "dg_update_batch")
    res = [bytes(bufs[i][:ol[i]]) if st[i] in (0, 10) else None for i in range(n)]
    if status:
        return res, list(st)
    for i in range(n):
        if st[i]:
            raise DeltaError(st[i], f"delta {i}")
    return res


def crc64_xz(data: bytes, ctx: Optional[Context] = None) -> bytes:
    """CRC-64/XZ, 8 bytes big-endian (src/c/delta.h:294-322), on the GPU."""
    ctx = ctx or default_context()
    out = (C.c_uint8 * 8)()
    ctx.check(lib.dg_crc64_xz(ctx.handle, _u8(data), len(data), out), "dg_crc64_xz")
    return bytes(out)


def decode(R: bytes, delta: bytes, ignore_hash: bool = False,
           ctx: Optional[Context] = None) -> bytes:
    """Apply a delta to R on the GPU (src/c/main.c:323-400)."""
    ctx = ctx or default_context()
    out = Buffer()
    rc = lib.dg_decode(ctx.handle, _u8(R), len(R), _u8(delta), len(delta), int(ignore_hash),
                       C.byref(out))
    res = C.string_at(out.data, out.len) if out.len else b""
    lib.dg_buffer_free(C.byref(out))
    ctx.check(rc, "dg_decode")
    return res


def info(delta: bytes) -> dict:
    """Header and command summary (src/c/main.c:402-425)."""
    d = DeltaInfo()
    rc = lib.dg_delta_info(_u8(delta), len(delta), C.byref(d))
    if rc:
        raise DeltaError(rc, "dg_delta_info")
    return {
        "inplace": bool(d.inplace), "version_size": d.version_size,
        "src_crc": bytes(d.src_crc), "dst_crc": bytes(d.dst_crc),
        "num_commands": d.num_commands, "num_copies": d.num_copies, "num_adds": d.num_adds,
        "copy_bytes": d.copy_bytes, "add_bytes": d.add_bytes,
    }


# ── command lists (src/python/delta.py:44-96, 854-1000; delta.h:94-137) ──────

@dataclass
class CopyCmd:
    """Copy R[offset : offset+length] to the output (delta.py:44-51)."""
    offset: int
    length: int


@dataclass
class AddCmd:
    """Append literal bytes (delta.py:54-62)."""
    data: bytes


@dataclass
class PlacedCopy:
    """COPY with explicit source and destination (delta.py:72-80)."""
    src: int
    dst: int
    length: int


@dataclass
class PlacedAdd:
    """ADD at an explicit destination (delta.py:83-92)."""
    dst: int
    data: bytes


def _placed_list(cl: Commands) -> list:
    out = []
    for i in range(cl.len):
        c = cl.data[i]
        if c.tag == CMD_COPY:
            out.append(PlacedCopy(c.src, c.dst, c.length))
        else:
            out.append(PlacedAdd(c.dst, C.string_at(c.data, c.length) if c.length else b""))
    return out


def diff(R: bytes, V: bytes, algorithm="onepass", p: int = SEED_LEN, q: int = TABLE_SIZE,
         buf_cap: int = BUF_CAP, max_table: int = MAX_TABLE_SIZE, verbose: bool = False,
         ctx: Optional[Context] = None, splay: bool = False) -> list:
    """delta_diff / diff_greedy / diff_onepass / diff_correcting (delta.py:376,
    576): the algorithm's commands (CopyCmd / AddCmd), computed by the GPU
    encoder (dg_diff).  splay: greedy only."""
    return unplace_commands(diff_placed(R, V, algorithm, p, q, buf_cap, max_table, verbose, ctx, splay))


def diff_placed(R: bytes, V: bytes, algorithm="onepass", p: int = SEED_LEN, q: int = TABLE_SIZE,
                buf_cap: int = BUF_CAP, max_table: int = MAX_TABLE_SIZE, verbose: bool = False,
                ctx: Optional[Context] = None, splay: bool = False) -> list:
    """place_commands(diff(...)) in one call (dg_diff returns the placed form)."""
    ctx = ctx or default_context()
    cl = Commands()
    o = _opts(p, q, buf_cap, max_table, verbose=verbose, splay=splay)
    ctx.check(lib.dg_diff(ctx.handle, _algo(algorithm), _u8(R), len(R), _u8(V), len(V), C.byref(o),
                          C.byref(cl)), "dg_diff")
    try:
        return _placed_list(cl)
    finally:
        lib.dg_commands_free(C.byref(cl))


def diff_greedy(R: bytes, V: bytes, p: int = SEED_LEN, splay: bool = False, **kw) -> list:
    """delta_diff_greedy (greedy.c:88-267): the longest match at every position;
    splay picks the smallest offset among the longest instead of the largest."""
    return diff(R, V, "greedy", p=p, splay=splay, **kw)


def diff_onepass(R: bytes, V: bytes, p: int = SEED_LEN, q: int = TABLE_SIZE, **kw) -> list:
    return diff(R, V, "onepass", p=p, q=q, **kw)


def diff_correcting(R: bytes, V: bytes, p: int = SEED_LEN, q: int = TABLE_SIZE,
                    buf_cap: int = BUF_CAP, **kw) -> list:
    return diff(R, V, "correcting", p=p, q=q, buf_cap=buf_cap, **kw)


def output_size(commands: list) -> int:
    """delta.py:848-851."""
    return sum(c.length if isinstance(c, CopyCmd) else len(c.data) for c in commands)


def place_commands(commands: list) -> list:
    """Sequential destinations (delta.py:854-865, apply.c:136-164)."""
    out, dst = [], 0
    for c in commands:
        if isinstance(c, CopyCmd):
            out.append(PlacedCopy(c.offset, dst, c.length))
            dst += c.length
        else:
            out.append(PlacedAdd(dst, bytes(c.data)))
            dst += len(c.data)
    return out


def unplace_commands(placed: list) -> list:
    """Placed -> algorithm commands in destination order, stable
    (delta.py:868-895, apply.c:168-225)."""
    order = sorted(range(len(placed)), key=lambda i: placed[i].dst)
    return [CopyCmd(placed[i].src, placed[i].length) if isinstance(placed[i], PlacedCopy)
            else AddCmd(placed[i].data) for i in order]


def encode_delta(commands: list, *, inplace: bool = False, version_size: int, src_crc: bytes,
                 dst_crc: bytes) -> bytes:
    """Placed commands -> DLT\\x03 bytes (delta.py:939-964) via dg_encode_commands."""
    if len(src_crc) != 8 or len(dst_crc) != 8:
        raise ValueError("src_crc and dst_crc must be 8 bytes")
    n = len(commands)
    arr = (PlacedCommandC * max(n, 1))()
    keep = []
    for i, c in enumerate(commands):
        if isinstance(c, PlacedCopy):
            arr[i] = PlacedCommandC(CMD_COPY, c.src, c.dst, c.length, None)
        else:
            b = bytes(c.data)
            keep.append(b)
            arr[i] = PlacedCommandC(CMD_ADD, 0, c.dst, len(b), _u8(b))
    out = Buffer()
    rc = lib.dg_encode_commands(arr, n, int(inplace), version_size, (C.c_uint8 * 8)(*src_crc),
                                (C.c_uint8 * 8)(*dst_crc), C.byref(out))
    if rc:
        raise DeltaError(rc, "dg_encode_commands")
    try:
        return C.string_at(out.data, out.len)
    finally:
        lib.dg_buffer_free(C.byref(out))


def decode_delta(data: bytes):
    """delta.py:967-999's name and return value (commands, inplace,
    version_size, src_crc, dst_crc), via dg_delta_decode.  Malformed input
    follows the C decoder (encoding.c:111-178), not delta.py: an unknown
    command type or a COPY/ADD cut short by the buffer end raises
    DeltaError (code 8) where delta.py skips unknown types and returns
    truncated ADD data.  tests/test_format_cpu.py::test_decode_errors pins
    this choice."""
    cl, hdr = Commands(), DeltaInfo()
    rc = lib.dg_delta_decode(_u8(data), len(data), C.byref(cl), C.byref(hdr))
    if rc:
        raise DeltaError(rc, "dg_delta_decode")
    try:
        return (_placed_list(cl), bool(hdr.inplace), hdr.version_size, bytes(hdr.src_crc),
                bytes(hdr.dst_crc))
    finally:
        lib.dg_commands_free(C.byref(cl))
