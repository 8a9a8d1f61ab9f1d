"""CPU: the compaction's target-form rule and its no-GPU specification -- no
device call anywhere here.

  * ckpt::compact_form (cms_checkpoint.cpp, built for the CPU through
    tests/cpp/compact_host_shim.cpp) against mahout_amd.checkpoint.compact_form
    over every capacity edge, masses around 2^16, shapes with and without
    forms and lists, frac_bits, the list limits and the list's own edges;
  * checkpoint.compact_checkpoint on the golden fixture and on images designed
    with deliberately wide forms: counters, masses, IDs, hash parameters and
    pairs_ingested unchanged, the result valid to the loader's host checks,
    idempotent, and never larger.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from mahout_amd import checkpoint as ck

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "compact_host_shim.cpp")
LIB_SRC = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.cpp")
LIB_HDR = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.h")
OUT = os.path.join(HERE, "cpp", "_build", "libcompact_host_shim.so")
GOLDEN = os.path.join(HERE, "golden", "ckpt_v1_small.bin")

F = {name: i for i, name in enumerate(ck.ROW_FORMS)}
CMAX = (0, 1, 2, 3, 4, 15, 16, 255, 256, 65535, 65536)
SHAPES = ((4, 128), (5, 96), (3, 100), (32, 4096))


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    newest = max(os.path.getmtime(p) for p in (SRC, LIB_SRC, LIB_HDR))
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17",
                               "-I/opt/rocm/include", SRC, LIB_SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    for fn in ("host_check_header", "host_check_directory", "host_check_owner_ids"):
        getattr(lib, fn).restype = ctypes.c_char_p
    lib.host_compact_form.restype = ctypes.c_int
    lib.host_compact_form.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_uint64)]
    return lib


def _host(shim, cmax, mass, sums, d, w, frac_bits, list_keys, forms):
    """(form name, stored bytes) by the library's rule."""
    arr = None if sums is None else (ctypes.c_uint64 * d)(*[int(s) for s in sums])
    ln = ctypes.c_uint64()
    f = shim.host_compact_form(cmax, mass, arr, d, w, frac_bits, list_keys, int(forms), ctypes.byref(ln))
    return ck.ROW_FORMS[f], int(ln.value)


def _both(shim, cmax, mass, sums, d, w, frac_bits=0, list_keys=256, forms=True):
    """The form both statements of the rule give, and the stored length agreeing with it."""
    name, ln = _host(shim, cmax, mass, sums, d, w, frac_bits, list_keys, forms)
    spec = ck.compact_form(cmax, mass, sums, d, w, frac_bits=frac_bits, list_keys=list_keys, forms=forms)
    assert name == spec, (cmax, mass, sums, d, w, frac_bits, list_keys, forms, name, spec)
    assert ln == ck.row_length(F[name], d, w, mass if name == "list" else 0)
    return name


def test_rule_grid(shim):
    seen = set()
    for (d, w), cmax, frac_bits, list_keys, forms in itertools.product(SHAPES, CMAX, (0, 1), (0, 256, 1024), (True, False)):
        for mass in sorted({cmax, cmax + 1, 4 * cmax, 65535, 65536, 65537}):
            if mass < cmax:
                continue
            for sums in (None, [mass] * d, [mass] * (d - 1) + [mass + 1]):
                name = _both(shim, cmax, mass, sums, d, w, frac_bits, list_keys, forms)
                seen.add(name)
                # what the rule promises, whatever both implementations say
                if cmax == 0:
                    assert name == "zero"
                elif mass >= 65536 or cmax >= 65536:
                    assert name == "u32"
                else:
                    assert name != "u32" and name != "zero"
                    if name == "list":
                        assert frac_bits == 0 and forms and list_keys and sums == [mass] * d and ck.shape_has_form("list", d, w)
                        assert cmax <= 255
                    else:
                        assert cmax < 1 << ck._BITS[name]
                        assert ck.shape_has_form(name, d, w) and (forms or name == "u16")
    assert seen == {"zero", "list", "u1", "u2", "u4", "u8", "u16", "u32"}


def test_list_edges(shim):
    # the list limit: m = L is a list, m = L + 1 is not
    assert _both(shim, 20, 256, [256] * 8, 8, 1024, list_keys=256) == "list"
    assert _both(shim, 20, 257, [257] * 8, 8, 1024, list_keys=256) == "u8"
    assert _both(shim, 20, 257, [257] * 8, 8, 1024, list_keys=1024) == "list"
    assert _both(shim, 20, 1024, [1024] * 4, 4, 4096, list_keys=1024) == "list"
    assert _both(shim, 20, 1025, [1025] * 4, 4, 4096, list_keys=1024) == "u8"
    assert _both(shim, 20, 1025, [1025] * 4, 4, 4096, list_keys=4096) == "u8"  # (1024 bounds every list)
    assert _both(shim, 20, 5, [5] * 4, 4, 4096, list_keys=0) == "u8"
    # d m = 8192 is the last list, d m = 8224 is dense (d = 32, list_keys = 1024)
    assert _both(shim, 128, 256, [256] * 32, 32, 1024, list_keys=1024) == "list"
    assert _both(shim, 129, 257, [257] * 32, 32, 1024, list_keys=1024) == "u8"
    # no list holds a bucket more than 255 times (the writers re-count list entries in u8): 256 keys of one
    # bucket stay dense, at the default limit too, though the list would be the shorter
    assert _both(shim, 255, 255, [255] * 4, 4, 1024) == "list"
    assert _both(shim, 256, 256, [256] * 4, 4, 1024) == "u16"
    assert _both(shim, 256, 256, [256] * 5, 5, 8192) == "u16"
    assert _both(shim, 256, 256, [256] * 32, 32, 1024, list_keys=1024) == "u16"
    assert _both(shim, 300, 300, [300] * 4, 4, 1024, list_keys=1024) == "u16"
    assert _both(shim, 255, 256, [256] * 4, 4, 1024) == "list"
    # ... and at the grid's (32, 4096), whose u16 row passes 80 KiB, nothing is a list
    assert _both(shim, 256, 256, [256] * 32, 32, 4096, list_keys=1024) == "u16"
    assert _both(shim, 256, 257, [257] * 32, 32, 4096, list_keys=1024) == "u16"
    assert _both(shim, 1, 3, [3] * 32, 32, 4096, list_keys=1024) == "u1"
    # a list exactly as long as its dense alternative is stored dense: 2 + 2 * 7 == 128 / 8
    assert _both(shim, 1, 6, [6], 1, 128) == "list"
    assert _both(shim, 1, 7, [7], 1, 128) == "u1"
    assert _both(shim, 3, 14, [14], 1, 128) == "list"
    assert _both(shim, 3, 15, [15], 1, 128) == "u2"  # 2 + 2 * 15 == 128 / 4
    # sketch rows that disagree, or whose sum is not the mass: dense
    assert _both(shim, 1, 5, [5, 5, 5, 4], 4, 128) == "u1"
    assert _both(shim, 1, 6, [5, 5, 5, 5], 4, 128) == "u1"
    assert _both(shim, 1, 5, None, 4, 128) == "u1"
    assert _both(shim, 1, 5, [5] * 4, 4, 128) == "list"
    # fixed-point counters and handles without forms store no lists
    assert _both(shim, 1, 5, [5] * 4, 4, 128, frac_bits=1) == "u1"
    assert _both(shim, 1, 5, [5] * 4, 4, 128, forms=False) == "u16"


HASH = (np.arange(1, 33, dtype=np.int64) * 1000003, np.arange(1, 33, dtype=np.int64) * 7919)


def designed_image():
    """(4, 128), every row stored wider than it needs: counters <= 1 as u16 and
    as u32, a list stored dense (u8) and as an unsorted list, an all-zero u8
    row, a demotable hot row, a row that stays hot, a row that stays u16."""
    d, w = 4, 128
    rng = np.random.Generator(np.random.PCG64(7))
    c = np.zeros((10, d, w), np.uint64)
    forms, lists, masses = [None] * 10, {}, np.zeros(10, np.uint64)

    def keys(r, m, reps=1):
        for i in range(d):
            np.add.at(c[r, i], rng.integers(0, w, m), reps)
        masses[r] = m * reps

    c[0, :, 3] = 1; masses[0] = 1; forms[0] = "u16"            # -> list (10 bytes)
    c[1, :, 9] = 1; masses[1] = 1; forms[1] = "u32"            # -> list
    for i in range(d):                                          # 40 distinct buckets per sketch row, sums agree:
        c[2, i, rng.permutation(w)[:40]] = 1                    # list of 322 bytes > the 64 of its 1-bit row -> u1
    masses[2] = 40; forms[2] = "u8"
    forms[3] = "u8"                                             # all zero -> zero
    keys(4, 3); forms[4] = "u8"                                 # sums agree, m = 3 -> list (26 bytes)
    ent = np.stack([rng.integers(0, w, 6) for _ in range(d)])[:, ::-1]
    for i in range(d):
        np.add.at(c[5, i], ent[i], 1)
    lists[5] = ent; masses[5] = 6                               # unsorted list -> the sorted list
    c[6, 0, 5] = 200; c[6, 1, 6] = 100; masses[6] = 200; forms[6] = "u32"   # sums disagree -> u8
    c[7, :, 1] = 70000; masses[7] = 70000                       # stays u32
    c[8, :, 2] = 300; masses[8] = 70000; forms[8] = "u32"       # mass keeps it u32
    c[9, :, 2] = 300; masses[9] = 300; forms[9] = "u16"         # list of 2402 bytes > 1024 -> stays u16
    ids = np.arange(10, dtype=np.int64) * 3 + 100
    return ck.build_checkpoint(c, *HASH, seed=42, owner_ids=ids, forms=forms, lists=lists, masses=masses,
                               pairs_ingested=12345), c


def _valid(shim, data):
    c = ck.Checkpoint(data)
    hd = np.frombuffer(data[:ck.HEADER_BYTES], ck.HEADER).copy()
    assert shim.host_check_header(hd.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(len(data))) is None
    dire = np.ascontiguousarray(c.directory)
    assert shim.host_check_directory(hd.ctypes.data_as(ctypes.c_void_p), dire.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.c_int64(c.num_owners)) is None
    if c.owner_ids is not None:
        ids = np.ascontiguousarray(c.owner_ids)
        assert shim.host_check_owner_ids(ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_int64(ids.size)) is None
    return c


def _check_compacted(shim, data, **kw):
    """(kw: a handle that holds every form of the input is never left with a
    larger payload; one without lists or forms is not asked that)"""
    before = ck.Checkpoint(data)
    out = ck.compact_checkpoint(data, **kw)
    after = _valid(shim, out)
    assert np.array_equal(after.counters(), before.counters())
    assert np.array_equal(after.masses, before.masses)
    assert (after.owner_ids is None) == (before.owner_ids is None)
    assert before.owner_ids is None or np.array_equal(after.owner_ids, before.owner_ids)
    assert np.array_equal(after.a, before.a) and np.array_equal(after.b, before.b)
    assert (after.pairs_ingested, after.seed, after.frac_bits) == (before.pairs_ingested, before.seed, before.frac_bits)
    assert ck.compact_checkpoint(out, **kw) == out
    assert ck.compact_checkpoint(ck.Checkpoint(out), **kw) == out
    assert kw or after.payload_bytes <= before.payload_bytes
    return before, after


def test_compact_checkpoint_golden(shim):
    data = open(GOLDEN, "rb").read()
    before, after = _check_compacted(shim, data)
    # the fixture holds every form; its sparse owners are lists again unless a
    # dense form of theirs is no longer
    assert after.form_counts().get("list", 0) > 0 and before.form_counts().get("list", 0) > 0
    _, nl = _check_compacted(shim, data, list_keys=0)
    assert "list" not in nl.form_counts()
    b2, a2 = _check_compacted(shim, data, forms=False)
    assert set(a2.form_counts()) <= {"zero", "u16", "u32"}


def test_compact_checkpoint_designed(shim):
    data, c = designed_image()
    before, after = _check_compacted(shim, data)
    got = [ck.ROW_FORMS[f] for f in after.forms]
    assert got == ["list", "list", "u1", "zero", "list", "list", "u8", "u32", "u32", "u16"], got
    assert after.payload_bytes < before.payload_bytes
    ent = after.list_entries(5)
    assert np.array_equal(ent, np.sort(before.list_entries(5), axis=1))  # ascending, repeats kept
    assert np.array_equal(after.bounds, [1, 1, 1, 0, int(c[4].max()), int(c[5].max()), 200, 0, 0, 300])
    assert np.array_equal(after.classes, [0, 0, 1, 0, 0, 0, 4, 0, 0, 5])
    # a handle without lists, and one without forms
    _, nl = _check_compacted(shim, data, list_keys=0)
    dense = [ck.default_form(int(c[r].max()), int(before.masses[r]), 4, 128) for r in (4, 5)]
    assert [ck.ROW_FORMS[f] for f in nl.forms] == ["u1", "u1", "u1", "zero"] + dense + ["u8", "u32", "u32", "u16"]
    _, nf = _check_compacted(shim, data, forms=False)
    assert [ck.ROW_FORMS[f] for f in nf.forms] == ["u16", "u16", "u16", "zero", "u16", "u16", "u16", "u32", "u32", "u16"]


def test_compact_checkpoint_refuses_fp64():
    data = ck.build_checkpoint(np.ones((2, 2, 64), np.float64), *HASH)
    with pytest.raises(ValueError):
        ck.compact_checkpoint(data)
