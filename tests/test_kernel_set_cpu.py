"""CPU: the default library ships exactly the kernels the product launches
(no kernel the product never launches).

The gfx950 code objects are extracted from lib/libdeltagpu.so as
test_isa_serialize.py does, and only their symbol tables are read: every kernel
has one kernel descriptor symbol, `<mangled name>.kd`.  A kernel added to or
removed from the product changes EXPECTED below in the same commit; a kernel
kept for an experiment belongs in a variant build, not here.
"""
from __future__ import annotations

import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "delta-compression_amd", "lib", "libdeltagpu.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# (Itanium-mangled, as in the symbol table; the readable name beside each group)
EXPECTED = {
    # dg_kernels.hip: scan_sizes, crc_rows<byte|five>, crc_rows_wide<1024>, crc_finalize, crc_patch,
    # serialize_wave, decode, and the synthetic-input kernels
    "_ZN2dg17scan_sizes_kernelEPKmPmjPjS3_",
    "_ZN2dg15crc_rows_kernelILi0EEEvNS_7CrcArgsE",
    "_ZN2dg15crc_rows_kernelILi1EEEvNS_7CrcArgsE",
    "_ZN2dg20crc_rows_wide_kernelILj1024EEEvNS_7CrcArgsE",
    "_ZN2dg19crc_finalize_kernelENS_7CrcArgsE",
    "_ZN2dg16crc_patch_kernelEPhPKmS2_PKij",
    "_ZN2dg21serialize_wave_kernelENS_7SerArgsE",
    "_ZN2dg13decode_kernelENS_10DecodeArgsE",
    "_ZN2dg19synth_random_kernelEPhS0_mmm",
    "_ZN2dg18synth_edits_kernelEPhjmmm",
    "_ZN2dg19synth_stream_kernelEPhPKNS_9SynthSpanEj",
    "_ZN2dg17synth_copy_kernelEPhPKhPKNS_9SynthCopyEj",
    "_ZN2dg18synth_shift_kernelEPhPKhPKNS_9SynthSpanEPKmjmj",
    # dg_onepass.hip: onepass16<plain | routed | members>, onepass<p = any | 16> from HBM
    "_ZN2dg16onepass16_kernelILb0ELb0EEEvNS_10EncodeArgsE",
    "_ZN2dg16onepass16_kernelILb0ELb1EEEvNS_10EncodeArgsE",
    "_ZN2dg16onepass16_kernelILb1ELb0EEEvNS_10EncodeArgsE",
    "_ZN2dg14onepass_kernelILi0EEEvNS_10EncodeArgsE",
    "_ZN2dg14onepass_kernelILi16EEEvNS_10EncodeArgsE",
    # dg_members.hip: member_chunk, member_serialize
    "_ZN2dg19member_chunk_kernelENS_8SpecArgsEj",
    "_ZN2dg23member_serialize_kernelENS_10MemSerArgsEjj",
    # dg_correcting.hip: class, clear, stats, build (global), build_lds<CRC off | on>, scan
    "_ZN2dg23correcting_class_kernelENS_10EncodeArgsE",
    "_ZN2dg23correcting_clear_kernelENS_10EncodeArgsE",
    "_ZN2dg23correcting_stats_kernelENS_10EncodeArgsE",
    "_ZN2dg23correcting_build_kernelENS_10EncodeArgsEjj",
    "_ZN2dg27correcting_build_lds_kernelILb0EEEvNS_10EncodeArgsEj",
    "_ZN2dg27correcting_build_lds_kernelILb1EEEvNS_10EncodeArgsEj",
    "_ZN2dg22correcting_scan_kernelENS_10EncodeArgsE",
    # dg_greedy.hip: heads, build<splay off | on>, match
    "_ZN2dg12_GLOBAL__N_119greedy_heads_kernelENS_10GreedyArgsE",
    "_ZN2dg12_GLOBAL__N_119greedy_build_kernelILb0EEEvNS_10GreedyArgsEj",
    "_ZN2dg12_GLOBAL__N_119greedy_build_kernelILb1EEEvNS_10GreedyArgsEj",
    "_ZN2dg12_GLOBAL__N_119greedy_match_kernelENS_10GreedyArgsE",
}


def _gfx950_kernels():
    """Names of the kernel descriptor symbols of the library's gfx950 code objects."""
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        with open(LIB, "rb") as src, open(so, "wb") as dst:
            dst.write(src.read())
        subprocess.run([OBJDUMP, "--offloading", so], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            r = subprocess.run([OBJDUMP, "-t", os.path.join(tmp, f)], check=True, capture_output=True, text=True)
            for line in r.stdout.splitlines():
                sym = line.split()[-1] if line.split() else ""
                if sym.endswith(".kd"):
                    names.add(sym[:-3])
    return names


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(OBJDUMP), reason="library or llvm-objdump missing")
def test_library_ships_exactly_the_launched_kernels():
    got = _gfx950_kernels()
    assert got == EXPECTED, {"unexpected": sorted(got - EXPECTED), "missing": sorted(EXPECTED - got)}
