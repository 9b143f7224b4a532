"""delta_compression_amd — MI355X-native batched delta codec (host mirror).

Python view of the C ABI in ``include/delta_gpu.h`` (``lib/libdeltagpu.so``).
Names and argument meanings follow the reference's interface for this path:

* ``encode(R, V, algorithm, p, q)``  — ``delta encode`` (src/c/main.c:257-292;
  src/python/delta.py:1579-1629): CRC-64/XZ of both buffers, onepass or
  correcting differencing, placement, DLT\\x03 serialisation.
* ``encode_batch(pairs, ...)``      — the same for many pairs at once.
* ``encode_pipelined(pairs, ...)``  — host arenas in chunks, H2D / encode / D2H overlapped.
* ``EncodePlan``                    — device-resident batches (the hot path).
* ``crc64_xz(data)``                — ``delta_crc64_xz`` (src/c/delta.h:294).
* ``decode(R, delta)``              — ``delta decode`` (main.c:323-400).
* ``UpdatePlan`` / ``update_batch`` — an in-place delta applied in the buffer
  that holds R (apply.c:253-284), validated whole before the first store.
* ``compose(A, B)`` / ``ComposePlan`` / ``compose_batch`` — delta(R -> V1) and
  delta(V1 -> V2) joined into delta(R -> V2) without R, V1 or V2 (no reference
  counterpart; the normal form is stated in ``include/delta_gpu.h``).
* ``invert(R, A)`` / ``InvertPlan`` / ``invert_batch`` — R and delta(R -> V)
  turned into delta(V -> R) without V (no reference counterpart; the normal
  form is stated in ``include/delta_gpu.h``).
* ``segment_pairs`` / ``SplicePlan`` / ``splice`` / ``splice_batch`` /
  ``encode_large`` — one large pair cut into segments of V against windows of
  R, encoded as an ordinary batch, the segment deltas spliced into one
  standard delta (no reference counterpart; rule, contract and normal form are
  stated in ``include/delta_gpu.h``).
* ``read_range(R, delta, off, length)`` / ``ReadPlan`` / ``read_ranges`` — bytes
  [off, off + length) of the version a standard delta makes of R, without
  rebuilding the version (no reference counterpart: the replay of
  apply.c:229-249, sliced).  ``ReadPlan.chunk_index`` / ``index_chunked`` index
  one large delta with the whole GPU (the same index), and ``decode_large(R,
  delta)`` is ``decode`` as that index plus ``tile_requests`` tiles of V.
* ``read_lineage(R, deltas, off, length)`` / ``LineagePlan`` /
  ``read_lineage_batch`` — the same read of a version that is several deltas
  away from R (a delta on a delta on ... R), without rebuilding any version.
* ``sketch`` / ``SketchPlan`` / ``sketch_batch`` / ``match_sketches`` /
  ``pick_bases`` — which buffer to encode against: min-wise resemblance
  sketches over the encoders' fingerprints and base selection by the exact
  integer rule of ``include/delta_gpu.h`` (no reference counterpart).
* ``info(delta)``                   — ``delta info`` (main.c:402-425).
* ``diff`` / ``diff_greedy`` / ``diff_onepass`` / ``diff_correcting``, ``place_commands``,
  ``unplace_commands``, ``encode_delta``, ``decode_delta`` — the command-list
  level of src/python/delta.py:376-999 (the differencing on the GPU, the
  container walk in the library's host code).

Everything runs on the GPU.  Importing this package without the built
library, or calling it without a visible GPU, raises — there is no CPU
fallback.
"""
from __future__ import annotations

from ._lib import (  # noqa: F401
    ALGO_CORRECTING,
    ALGO_GREEDY,
    ALGO_ONEPASS,
    BUF_CAP,
    MAX_TABLE_SIZE,
    SEED_LEN,
    TABLE_SIZE,
    AddCmd,
    Context,
    CopyCmd,
    PlacedAdd,
    PlacedCopy,
    DeltaError,
    DiffOptions,
    EncodePlan,
    DecodePlan,
    InplacePlan,
    UpdatePlan,
    ComposeDesc,
    ComposePlan,
    InvertDesc,
    InvertPlan,
    SplicePlan,
    ReadPlan,
    ReadReq,
    ReadStream,
    SketchPlan,
    SKETCH_BINS,
    SKETCH_EMPTY,
    MATCH_NONE,
    MATCH_ALL,
    MATCH_NOT_SELF,
    MATCH_EARLIER,
    LIB_PATH,
    LIMIT_ONEPASS_MEMBERS,
    LIMIT_TABLE_POOL_BYTES,
    MEMBERS_AUTO,
    MEMBERS_OFF,
    MEMBERS_ON,
    crc64_xz,
    decode,
    decode_delta,
    default_context,
    diff,
    diff_correcting,
    diff_greedy,
    diff_onepass,
    diff_placed,
    encode,
    encode_batch,
    encode_delta,
    encode_pipelined,
    info,
    lib,
    make_inplace,
    make_inplace_batch,
    update_batch,
    compose,
    compose_batch,
    invert,
    invert_batch,
    segment_pairs,
    splice,
    splice_batch,
    sketch_windows,
    encode_large,
    read_range,
    read_ranges,
    LineagePlan,
    read_lineage,
    read_lineage_batch,
    lineage_work_items,
    LINEAGE_BASE,
    LINEAGE_MAX_DEPTH,
    tile_requests,
    decode_large,
    sketch,
    sketch_batch,
    match_sketches,
    match_sketches_device,
    pick_bases,
    output_size,
    place_commands,
    status_string,
    unplace_commands,
)

__all__ = [
    "ALGO_ONEPASS", "ALGO_CORRECTING", "ALGO_GREEDY", "SEED_LEN", "TABLE_SIZE",
    "MAX_TABLE_SIZE", "BUF_CAP", "Context", "DeltaError", "DiffOptions", "EncodePlan", "DecodePlan", "InplacePlan", "UpdatePlan",
    "ComposeDesc", "ComposePlan", "compose", "compose_batch",
    "InvertDesc", "InvertPlan", "invert", "invert_batch",
    "SplicePlan", "segment_pairs", "splice", "splice_batch", "sketch_windows", "encode_large",
    "ReadPlan", "ReadReq", "ReadStream", "read_range", "read_ranges", "tile_requests", "decode_large",
    "LineagePlan", "read_lineage", "read_lineage_batch", "lineage_work_items", "LINEAGE_BASE", "LINEAGE_MAX_DEPTH",
    "SketchPlan", "sketch", "sketch_batch", "match_sketches", "match_sketches_device", "pick_bases", "SKETCH_BINS", "SKETCH_EMPTY",
    "MATCH_NONE", "MATCH_ALL", "MATCH_NOT_SELF", "MATCH_EARLIER",
    "crc64_xz", "decode", "default_context", "encode", "encode_batch", "encode_pipelined", "info", "lib",
    "make_inplace", "make_inplace_batch", "update_batch", "status_string", "LIB_PATH", "LIMIT_TABLE_POOL_BYTES",
    "LIMIT_ONEPASS_MEMBERS", "MEMBERS_AUTO", "MEMBERS_ON", "MEMBERS_OFF",
    "CopyCmd", "AddCmd", "PlacedCopy", "PlacedAdd", "diff", "diff_greedy", "diff_onepass", "diff_correcting",
    "diff_placed", "place_commands", "unplace_commands", "output_size", "encode_delta", "decode_delta",
]
