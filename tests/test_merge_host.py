"""CPU: the merge's header-level compatibility rules on the host alone -- no
device call anywhere here.

  * check_merge_params / check_merge_masses / merge_increment of
    cms_checkpoint.cpp through tests/cpp/merge_host_shim.cpp: the hash
    parameters in use, the owner-ID sections, and the overflow rule the
    ingest uses (old + inc >= 2^32);
  * the same rules through the pure-numpy specification
    mahout_amd.checkpoint.sum_counters on the golden fixture.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mahout_amd import checkpoint as ck

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "merge_host_shim.cpp")
LIB_SRC = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.cpp")
LIB_HDR = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.h")
OUT = os.path.join(HERE, "cpp", "_build", "libmerge_host_shim.so")
GOLDEN = os.path.join(HERE, "golden", "ckpt_v1_small.bin")

F = {name: i for i, name in enumerate(ck.ROW_FORMS)}
DEPTH = 4


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    newest = max(os.path.getmtime(p) for p in (SRC, LIB_SRC, LIB_HDR))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17",
                               "-I/opt/rocm/include", SRC, LIB_SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    lib.host_check_merge_params.restype = ctypes.c_char_p
    lib.host_check_merge_masses.restype = ctypes.c_char_p
    lib.host_merge_increment.restype = ctypes.c_uint64
    return lib


def _header(n=3, counter_type=0):
    hd = np.zeros(1, ck.HEADER)
    h = hd[0]
    h["depth"], h["width"], h["num_owners"], h["counter_type"] = DEPTH, 128, n, counter_type
    h["a"][:DEPTH] = np.arange(1, DEPTH + 1) * 1000003
    h["b"][:DEPTH] = np.arange(1, DEPTH + 1) * 7919
    return hd


def _ptr(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _params(shim, hd, a, b, live_ids=None, image_ids=None):
    return shim.host_check_merge_params(_ptr(hd), _ptr(a), _ptr(b), _ptr(live_ids), _ptr(image_ids))


def _live(hd):
    """The live handle's a[32], b[32] equal to the header's in use (rows >=
    depth hold what another depth-32 draw would: not in use)."""
    a = np.array(hd[0]["a"], np.int64)
    b = np.array(hd[0]["b"], np.int64)
    a[DEPTH:] = 99
    b[DEPTH:] = 77
    return a, b


# ---- hash parameters ----

def test_equal_hash_parameters_pass(shim):
    hd = _header()
    a, b = _live(hd)
    assert _params(shim, hd, a, b) is None


@pytest.mark.parametrize("which", ["a", "b"])
def test_a_difference_at_the_last_row_in_use_is_refused(shim, which):
    hd = _header()
    a, b = _live(hd)
    (a if which == "a" else b)[DEPTH - 1] += 1
    assert _params(shim, hd, a, b) is not None


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("index", [DEPTH, 31])
def test_a_difference_past_the_depth_passes(shim, which, index):
    hd = _header()
    a, b = _live(hd)
    (a if which == "a" else b)[index] += 12345
    assert _params(shim, hd, a, b) is None


# ---- owner-ID sections ----

def test_id_sections(shim):
    hd = _header()
    a, b = _live(hd)
    ids = np.array([3, 5, 8], np.int64)
    assert _params(shim, hd, a, b, None, None) is None  # absent / absent
    assert _params(shim, hd, a, b, ids, ids.copy()) is None  # identical
    assert _params(shim, hd, a, b, ids, None) is not None  # present / absent
    assert _params(shim, hd, a, b, None, ids) is not None  # absent / present
    other = ids.copy()
    other[1] = 6  # one ID differs
    assert _params(shim, hd, a, b, ids, other) is not None


# ---- the overflow rule ----

def _dir(masses, form="u16"):
    dire = np.zeros(len(masses), ck.DIR_ENTRY)
    dire["form"] = F[form]
    dire["mass"] = np.asarray(masses, np.uint64)
    return dire


def _masses(shim, hd, dire, live):
    live = None if live is None else np.asarray(live, np.uint64)
    return shim.host_check_merge_masses(_ptr(hd), _ptr(dire), _ptr(live), ctypes.c_int64(dire.size))


@pytest.mark.parametrize("live,image", [(2 ** 32 - 2, 1), (1, 2 ** 32 - 2), (2 ** 31, 2 ** 31 - 1), (0, 2 ** 32 - 1)])
def test_masses_summing_to_2_32_minus_1_are_accepted(shim, live, image):
    hd = _header()
    assert _masses(shim, hd, _dir([5, image, 0]), [7, live, 0]) is None


@pytest.mark.parametrize("live,image", [(2 ** 32 - 1, 1), (1, 2 ** 32 - 1), (2 ** 31, 2 ** 31), (0, 2 ** 32),
                                        (2 ** 63, 2 ** 63)])
def test_masses_summing_to_2_32_are_refused(shim, live, image):
    hd = _header()
    msg = _masses(shim, hd, _dir([5, 0, image]), [7, 0, live])
    assert msg is not None and b"2^32" in msg  # the ingest's wording (cms_api.hip flags_error)


def test_an_empty_live_table_and_fp64_counters(shim):
    hd = _header()
    assert _masses(shim, hd, _dir([2 ** 32 - 1, 0, 9]), None) is None  # (no live masses: an empty handle)
    assert _masses(shim, hd, _dir([2 ** 32, 0, 9]), None) is not None
    assert _masses(shim, _header(counter_type=1), _dir([2 ** 40, 0, 9], "f64"), [2 ** 40, 1, 1]) is None


# ---- the per-row increment bound ----

@pytest.mark.parametrize("form,length,cbound,mass,want", [
    ("zero", 0, 0, 0, 0),
    ("list", 2, 0, 0, 0),            # a list of no entries
    ("list", 2 + 8 * 5, 2, 5, 2),    # min(cbound, mass)
    ("list", 2 + 8 * 5, 9, 5, 5),
    ("list", 2 + 8 * 300, 300, 300, 300),    # every key in one bucket: the loader bounds the length, not a bucket
    ("list", 2 + 8 * 1024, 0, 2000, 1024),   # no cbound: the longest list there is
    ("u1", 64, 1, 40, 1),
    ("u2", 128, 3, 2, 2),
    ("u4", 256, 9, 1000, 9),
    ("u8", 512, 200, 100, 100),
    ("u8", 512, 200, 0, 0),          # mass 0: every stored counter is zero
    ("u16", 1024, 300, 60000, 60000),  # a u16 row's cbound is not maintained by in-place adds: the mass bounds it
    ("u16", 1024, 300, 10 ** 6, 65535),
    ("u32", 2048, 0, 70000, 70000),
    ("f64", 4096, 0, 12, 12),
])
def test_merge_increment(shim, form, length, cbound, mass, want):
    e = np.zeros(1, ck.DIR_ENTRY)
    e[0]["form"], e[0]["len"], e[0]["cbound"], e[0]["mass"] = F[form], length, cbound, mass
    assert shim.host_merge_increment(_ptr(e)) == want


# ---- the numpy specification on the golden fixture ----

def test_golden_merged_with_itself_is_twice_its_counters():
    c = ck.read_checkpoint(GOLDEN)
    got = ck.sum_counters([GOLDEN, GOLDEN])
    assert got.shape == (c.num_owners, c.depth, c.width)
    assert np.array_equal(got, 2 * c.counters())
    assert np.array_equal(ck.sum_counters([c, GOLDEN, c]), 3 * c.counters())
    assert np.array_equal(ck.sum_counters([c]), c.counters())


def _patched(tmp_path, name, patch):
    img = bytearray(open(GOLDEN, "rb").read())
    hd = np.frombuffer(bytes(img[:ck.HEADER_BYTES]), ck.HEADER).copy()
    patch(hd[0])
    img[:ck.HEADER_BYTES] = hd.tobytes()
    path = tmp_path / name
    path.write_bytes(img)
    return str(path)


def test_sum_counters_refuses_other_hash_parameters(tmp_path):
    d = ck.read_checkpoint(GOLDEN).depth

    def last_in_use(h):
        h["b"][d - 1] += 1

    def past_depth(h):
        h["a"][d] += 1

    with pytest.raises(ValueError):
        ck.sum_counters([GOLDEN, _patched(tmp_path, "b.ckpt", last_in_use)])
    ok = ck.sum_counters([GOLDEN, _patched(tmp_path, "c.ckpt", past_depth)])  # not in use
    assert np.array_equal(ok, 2 * ck.read_checkpoint(GOLDEN).counters())


@pytest.mark.parametrize("field", ["frac_bits", "seed"])
def test_sum_counters_shape_rules(tmp_path, field):
    def patch(h):
        h[field] += 1

    path = _patched(tmp_path, "p.ckpt", patch)
    if field == "seed":  # the seed alone decides nothing: the parameters in use do
        assert np.array_equal(ck.sum_counters([GOLDEN, path]), 2 * ck.read_checkpoint(GOLDEN).counters())
    else:
        with pytest.raises(ValueError):
            ck.sum_counters([GOLDEN, path])
