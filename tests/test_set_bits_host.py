"""CPU: what the dense set similarity kernels share with the host (cms_set_bits.h, built as
tests/cpp/set_bits_host_shim.hip): the expansion of bits into e2m1 nibbles and the bit matrix's geometry."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "set_bits_host_shim.hip")
DEPS = [SRC] + [os.path.join(HERE, "..", "mahout_amd", "csrc", f) for f in ("cms_set_bits.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libset_bits_host_shim.so")


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17",
                               "-I/opt/rocm/include", SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    for name, nargs in (("sb_stage", 0), ("sb_padded_k", 1), ("sb_seg_stages", 1), ("sb_segments", 2),
                        ("sb_matrix_bytes", 2), ("sb_word_off", 3)):
        getattr(lib, name).restype = ctypes.c_int64
        getattr(lib, name).argtypes = [ctypes.c_int64] * nargs
    lib.sb_expand8.restype = ctypes.c_uint32
    return lib


def test_expand_every_byte(shim):
    """Nibble j of the dword is 0x2 (e2m1 1.0) iff bit j of the byte is set, and nothing above the byte is read."""
    for b in range(256):
        exp = sum(0x2 << (4 * j) for j in range(8) if b >> j & 1)
        assert shim.sb_expand8(b) == exp == shim.sb_expand8(b | 0xABCDEF00), b


def test_padded_k_and_segments(shim):
    st = shim.sb_stage()
    assert st % 64 == 0 and (1 << 24) % st == 0
    for num, stages in ((1, 1), (st - 1, 1), (st, 1), (st + 1, 2), (2 * st + 1, 3), (2 ** 31 - 1, 2 ** 31 // st)):
        assert shim.sb_padded_k(num) == stages * st
        assert shim.sb_segments(num, 1) == stages and shim.sb_segments(num, 2) == (stages + 1) // 2
        assert shim.sb_matrix_bytes(129, num) == 256 * stages * st // 8  # rows padded to whole blocks of 128
    # CMS_SET_BITS_KSEG: whole stages, at least one, at most 2^24 cross indices
    assert [shim.sb_seg_stages(a) for a in (0, 1, st, 2 * st + 5, 2 ** 24, 2 ** 30)] == \
        [2 ** 24 // st, 1, 1, 2, 2 ** 24 // st, 2 ** 24 // st]
    assert shim.sb_segments(2 ** 31 - 1, shim.sb_seg_stages(0)) == 128


def test_word_offsets_tile_the_matrix(shim):
    """Every (row, word) of a 3-stage, 130-row matrix has a word of its own inside the padded matrix, and a stage of
    a block's rows is one contiguous run."""
    st, stages = shim.sb_stage(), 3
    offs = {shim.sb_word_off(r, w, stages) for r in range(130) for w in range(stages * st // 32)}
    assert len(offs) == 130 * stages * st // 32 and max(offs) < shim.sb_matrix_bytes(130, 3 * st) // 4 and min(offs) == 0
    run = [shim.sb_word_off(r, st // 32 + w, stages) for r in range(128) for w in range(st // 32)]
    assert run == list(range(run[0], run[0] + len(run)))
