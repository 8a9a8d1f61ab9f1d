"""CPU: k_common_item_estimate's shape (cms_common_item.h through tests/cpp/common_item_host_shim.hip) -- cell bytes,
default tiles, the CMS_COMMON_EST_TILE rounding -- and the attach rules the GPU test's fallback models rely on."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import common_item_ref as CI

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mahout_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "common_item_host_shim.hip")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("cms_common_item.h", "cms_common.h", "cms_exact.h", "cms_hash.h")]
OUT = os.path.join(HERE, "cpp", "_build", "libcommon_item_host_shim.so")


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-I/opt/rocm/include", SRC, "-o", OUT])
    return ctypes.CDLL(OUT)


# measure (CMS_SIM_*: uncentered, Pearson, Euclidean), kind (weighted, boolean), cell bytes, default tile
@pytest.mark.parametrize("measure,kind,cell,tile", [(2, 0, 32, 2048), (0, 0, 48, 1344), (1, 0, 64, 1024),
                                                    (2, 1, 24, 2688), (0, 1, 40, 1600), (1, 1, 56, 1152)])
def test_shape(shim, measure, kind, cell, tile):
    assert shim.cih_cell_bytes(measure, kind) == cell and shim.cih_tile_default(measure, kind) == tile
    assert tile % 64 == 0 and tile * cell <= 65536 < (tile + 64) * cell  # the largest multiple of 64 within 64 KiB
    for asked, got in ((0, tile), (-5, tile), (1, 64), (64, 64), (65, 128), (tile - 1, tile), (tile, tile),
                       (tile + 1, tile), (1 << 30, tile)):
        assert shim.cih_tile_for(measure, kind, asked) == got, asked


def test_fallback_models(shim):
    """(a) has a shift and one item at U = 2^51, (b) no shift at all; the plain model neither."""
    lib = shim
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    shifts = {}
    for variant in (None, "big", "noshift"):
        m, _, vals = CI.model(65, variant=variant)
        allv = np.ascontiguousarray(np.concatenate(vals), np.float32)
        s = shifts[variant] = lib.cih_shift(p(allv), ctypes.c_int64(allv.size))
        if s >= 0:
            inel = [i for i, (_, v) in enumerate(m.lists["key"])
                    if not lib.cih_eligible(p(np.array(v, np.float32)), ctypes.c_int64(len(v)), s)]
            assert inel == ([65 // 3] if variant == "big" else []) and (variant != "big" or len(m.lists["key"][21][0]) == 2)
    assert shifts == {None: 1, "big": 0, "noshift": -1}
