"""CPU: the subtraction's mass rule on the host alone -- no device call
anywhere here.  check_subtract_masses of cms_checkpoint.cpp through
tests/cpp/subtract_host_shim.cpp: live_mass[r] >= image mass[r] for every
row, compared as the 64-bit values they are."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mahout_amd import checkpoint as ck

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "subtract_host_shim.cpp")
LIB_SRC = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.cpp")
LIB_HDR = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.h")
OUT = os.path.join(HERE, "cpp", "_build", "libsubtract_host_shim.so")

F = {name: i for i, name in enumerate(ck.ROW_FORMS)}


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    newest = max(os.path.getmtime(p) for p in (SRC, LIB_SRC, LIB_HDR))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17",
                               "-I/opt/rocm/include", SRC, LIB_SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.host_check_subtract_masses.restype = ctypes.c_char_p
    return lib


def _header(n, counter_type=0):
    hd = np.zeros(1, ck.HEADER)
    h = hd[0]
    h["depth"], h["width"], h["num_owners"], h["counter_type"] = 4, 128, n, counter_type
    return hd


def _dir(masses, form="u16"):
    dire = np.zeros(len(masses), ck.DIR_ENTRY)
    dire["form"] = F[form]
    dire["mass"] = np.asarray(masses, np.uint64)
    return dire


def _ptr(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _masses(shim, dire, live, counter_type=0):
    live = None if live is None else np.asarray(live, np.uint64)
    return shim.host_check_subtract_masses(_ptr(_header(dire.size, counter_type)), _ptr(dire), _ptr(live),
                                           ctypes.c_int64(dire.size))


IMAGE = [5, 0, 70000, 1, 9]


def test_equal_masses_are_accepted(shim):
    assert _masses(shim, _dir(IMAGE), IMAGE) is None
    assert _masses(shim, _dir(IMAGE), [6, 3, 70001, 1, 10]) is None


@pytest.mark.parametrize("row", [0, 2, 4], ids=["first", "middle", "last"])
def test_a_mass_one_below_the_images_is_refused(shim, row):
    live = list(IMAGE)
    live[row] -= 1
    msg = _masses(shim, _dir(IMAGE), live)
    assert msg is not None and b"below zero" in msg


def test_a_hot_row_one_below_is_refused(shim):
    dire = _dir([3, 2 ** 20, 4])
    dire["form"][1] = F["u32"]  # form 7
    assert int(dire["form"][1]) == 7
    assert _masses(shim, dire, [3, 2 ** 20, 4]) is None
    assert _masses(shim, dire, [3, 2 ** 20 - 1, 4]) is not None


def test_an_empty_live_table(shim):
    assert _masses(shim, _dir([0, 0, 0]), None) is None  # (no live masses: an empty handle)
    assert _masses(shim, _dir([0, 0, 0]), [0, 0, 0]) is None
    for r in range(3):
        image = [0, 0, 0]
        image[r] = 1
        assert _masses(shim, _dir(image), None) is not None
        assert _masses(shim, _dir(image), [0, 0, 0]) is not None


def test_masses_near_2_32_do_not_wrap(shim):
    top = 2 ** 32 - 1
    assert _masses(shim, _dir([top, top - 1, 1]), [top, top, top]) is None
    assert _masses(shim, _dir([top, 0, 0]), [top - 1, 0, 0]) is not None
    assert _masses(shim, _dir([top, 0, 0]), [0, 0, 0]) is not None  # (0 - top is 1 mod 2^32: no wrapped difference passes)
    assert _masses(shim, _dir([1, 0, 0]), [top, 0, 0]) is None
    # 64-bit values as they are: 2^32 + 1 live against 2 in the image passes, the reverse is refused
    assert _masses(shim, _dir([2, 0, 0]), [2 ** 32 + 1, 0, 0]) is None
    assert _masses(shim, _dir([2 ** 32 + 1, 0, 0]), [2, 0, 0]) is not None
    assert _masses(shim, _dir([2 ** 63, 0, 0]), [2 ** 63 - 1, 0, 0]) is not None


def test_fp64_counters_do_not_subtract(shim):
    assert _masses(shim, _dir([0, 0, 0], "f64"), [0, 0, 0], counter_type=1) is not None
