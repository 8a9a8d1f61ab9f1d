"""CPU: build_checkpoint / write_checkpoint (mahout_amd.checkpoint), the
checkpoint format's numpy writer, against the three things that define the
format:

  * the golden fixture tests/golden/ckpt_v1_small.bin, which the GPU saver
    wrote: decoded and re-encoded it gives the same bytes;
  * the numpy reader: default-form images decode to the designed counters, in
    the forms the documented rule gives;
  * the host validator of cms_checkpoint.cpp (the CPU build of
    tests/test_checkpoint_host.py): every image the writer returns passes it,
    and what it would refuse the writer refuses with ValueError.
"""
import ctypes

import numpy as np
import pytest

from mahout_amd import checkpoint as ck
from test_checkpoint_host import GOLDEN, shim  # noqa: F401 -- the existing CPU build of the host validator

SHAPES = [(4, 128), (5, 96), (3, 100), (2, 64)]
A = np.arange(1, 33, dtype=np.int64) * 1000003
B = np.arange(1, 33, dtype=np.int64) * 7919


def _validate(shim, image):  # noqa: F811
    """The host validator's verdict on a whole image (None: accepted)."""
    hd = np.frombuffer(image[:ck.HEADER_BYTES], ck.HEADER).copy()
    msg = shim.host_check_header(hd.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(len(image)))
    if msg is not None:
        return msg
    n = int(hd[0]["num_owners"])
    do = int(hd[0]["dir_off"])
    dire = np.frombuffer(image[do:do + 32 * n], ck.DIR_ENTRY).copy()
    msg = shim.host_check_directory(hd.ctypes.data_as(ctypes.c_void_p), dire.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.c_int64(n))
    if msg is None and int(hd[0]["flags"]) & ck.FLAG_OWNER_IDS:
        ids = np.frombuffer(image[ck.HEADER_BYTES:ck.HEADER_BYTES + 8 * n], "<i8").copy()
        msg = shim.host_check_owner_ids(ids.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n))
    return msg


def _table(d, w, seed=0):
    """One or more owners for every default form: largest counters 0, 1, 3, 4,
    15, 16, 255, 256, 65535 (u16), 65536 and 2^32 - 1 (u32), and a row of
    small counters whose row sum passes 2^16 (u32 by mass)."""
    rng = np.random.Generator(np.random.PCG64(seed + 131 * d + w))
    tops = [0, 1, 1, 3, 4, 15, 16, 255, 256, 65535, 65536, 2 ** 32 - 1, 40000]
    c = np.zeros((len(tops) + 1, d, w), np.uint64)
    for r, top in enumerate(tops):
        if top == 0:
            continue
        nz = rng.random((d, w)) < 0.1
        c[r][nz] = rng.integers(1, min(top, 50) + 1, size=int(nz.sum()))
        i = rng.integers(0, d)
        if top >= 256:  # alone in its sketch row, so that the counter and not the row sum decides the form
            c[r, i] = 0
        c[r, i, rng.integers(0, w)] = top
    c[-1] = 700  # row sums 700 w >= 2^16 for w >= 94: u32 by mass at w = 96, 100, 128
    return c


def _expected_form(row, d, w):
    cmax, mass = int(row.max()), int(row.sum(axis=1).max())
    if mass >= 2 ** 16 or cmax >= 2 ** 16:
        return "u32"
    if cmax <= 1 and w % 128 == 0:
        return "u1"
    if cmax <= 3 and w % 64 == 0:
        return "u2"
    if cmax <= 15 and w % 32 == 0:
        return "u4"
    if cmax <= 255 and w % 32 == 0:
        return "u8"
    return "u16"


def test_golden_reencodes_to_the_same_bytes(shim):  # noqa: F811
    raw = open(GOLDEN, "rb").read()
    c = ck.Checkpoint(raw)
    assert c.frac_bits == 0 and c.owner_ids is None
    counters = np.stack([c.row_counters(r) for r in range(c.num_owners)])
    lists = {r: c.list_entries(r) for r in np.flatnonzero(c.forms == ck.ROW_FORMS.index("list")).tolist()}
    assert lists  # the fixture holds list rows
    again = ck.build_checkpoint(counters, c.a, c.b, seed=c.seed, frac_bits=c.frac_bits, forms=c.forms,
                                classes=c.classes, bounds=c.bounds, masses=c.masses, lists=lists,
                                pairs_ingested=c.pairs_ingested)
    assert again == raw
    assert _validate(shim, again) is None


@pytest.mark.parametrize("d,w", SHAPES)
def test_default_forms_round_trip(shim, tmp_path, d, w):  # noqa: F811
    c = _table(d, w)
    n = c.shape[0]
    image = ck.build_checkpoint(c, A[:d], B[:d], seed=42)
    assert _validate(shim, image) is None
    got = ck.Checkpoint(image)
    assert np.array_equal(got.counters(), c.astype(np.float64))
    want = [_expected_form(c[r], d, w) for r in range(n)]
    assert [ck.ROW_FORMS[f] for f in got.forms] == want
    assert "u32" in want and "u16" in want and (w % 32 != 0 or "u8" in want)
    assert np.array_equal(got.masses, c.sum(axis=2).max(axis=1))
    hot = np.array(want) == "u32"
    assert np.array_equal(got.bounds, np.where(hot, 0, c.reshape(n, -1).max(axis=1)))
    cls = {"u1": 1, "u2": 2, "u4": 3, "u8": 4, "u16": 5, "u32": 0}
    assert got.classes.tolist() == [cls[f] for f in want]
    assert np.array_equal(got.a, A[:d]) and np.array_equal(got.b, B[:d]) and got.seed == 42
    assert got.pairs_ingested == int(got.masses.sum())
    assert np.all(got.offsets % 16 == 0)
    path = tmp_path / "t.ckpt"
    assert ck.write_checkpoint(path, c, A[:d], B[:d], seed=42) == len(image)
    assert path.read_bytes() == image


def test_lists_zero_rows_ids_and_fractions(shim):  # noqa: F811
    d, w, n = 4, 128, 6
    rng = np.random.Generator(np.random.PCG64(9))
    ent = {1: rng.integers(0, w, size=(d, 7)), 3: np.zeros((d, 0), np.int64), 4: np.full((d, 3), w - 1)}
    c = np.zeros((n, d, w), np.uint64)
    for r, e in ent.items():
        for i in range(d):
            c[r, i] = np.bincount(e[i], minlength=w)
    c[5, 2, 17] = 6
    image = ck.build_checkpoint(c, A, B, frac_bits=1, owner_ids=[2, 3, 5, 7, 11, 13], lists=ent,
                                forms=["zero", None, None, "list", None, "u16"], pairs_ingested=99)
    assert _validate(shim, image) is None
    got = ck.Checkpoint(image)
    assert [ck.ROW_FORMS[f] for f in got.forms] == ["zero", "list", "u1", "list", "list", "u16"]
    assert got.lengths.tolist() == [0, 2 + 2 * d * 7, d * w // 8, 2, 2 + 2 * d * 3, 2 * d * w]
    assert np.array_equal(got.counters(), c / 2.0)  # preference units at frac_bits 1
    assert got.owner_ids.tolist() == [2, 3, 5, 7, 11, 13] and got.pairs_ingested == 99
    assert np.array_equal(got.list_entries(1), ent[1]) and got.classes.tolist() == [0, 0, 1, 0, 0, 5]
    assert got.bounds.tolist() == [0, int(c[1].max()), 0, 0, 3, 6]


def test_fp64_table(shim):  # noqa: F811
    c = np.random.Generator(np.random.PCG64(3)).normal(size=(3, 2, 7))
    image = ck.build_checkpoint(c, A, B)
    assert _validate(shim, image) is None
    got = ck.Checkpoint(image)
    assert got.counter_type == 1 and [ck.ROW_FORMS[f] for f in got.forms] == ["f64"] * 3
    assert np.array_equal(got.counters(), c)


def _refusals():
    z = lambda n=2, d=4, w=128: np.zeros((n, d, w), np.uint64)  # noqa: E731

    def over_capacity():
        c = z()
        c[1, 0, 0] = 16
        return dict(counters=c, forms=["u4", "u4"])

    def one_bit_at_w64():
        return dict(counters=z(w=64), forms=["u1", None])

    def two_bit_at_w96():
        return dict(counters=z(w=96), forms=["u2", None])

    def narrow_at_w100():
        return dict(counters=z(w=100), forms=["u8", None])

    def list_at_w100():
        return dict(counters=z(w=100), lists={0: np.zeros((4, 0), np.int64)})

    def list_too_long():
        c = z()
        c[0, :, 0] = 1025
        return dict(counters=c, lists={0: np.zeros((4, 1025), np.int64)})

    def list_longer_than_a_slot():  # 2 + 2 d m > 2 d w
        c = z(d=2, w=32)
        c[0, :, 0] = 32
        return dict(counters=c, lists={0: np.zeros((2, 32), np.int64)})

    def list_entry_outside():
        c = z()
        return dict(counters=c, lists={0: np.full((4, 1), 128)})

    def list_disagrees():
        c = z()
        c[0, :, 5] = 1
        return dict(counters=c, lists={0: np.full((4, 1), 6)})

    def ids_not_ascending():
        return dict(counters=z(), owner_ids=[4, 4])

    def narrow_class():
        c = z()
        c[0, 0, 0] = 200
        return dict(counters=c, classes=[3, 1])

    def hot_with_place():
        c = z()
        c[0, 0, 0] = 70000
        return dict(counters=c, classes=[5, 1])

    def zero_with_counters():
        c = z()
        c[0, 0, 0] = 1
        return dict(counters=c, forms=["zero", None])

    def mass_2_32():
        return dict(counters=z(), masses=[2 ** 32, 0])

    def f64_row_in_u32_table():
        return dict(counters=z(), forms=["f64", None])

    def unknown_form():
        return dict(counters=z(), forms=[9, None])

    def depth_33():
        return dict(counters=np.zeros((1, 33, 32), np.uint64), a=np.ones(33, np.int64), b=np.ones(33, np.int64))

    return [over_capacity, one_bit_at_w64, two_bit_at_w96, narrow_at_w100, list_at_w100, list_too_long,
            list_longer_than_a_slot, list_entry_outside, list_disagrees, ids_not_ascending, narrow_class,
            hot_with_place, zero_with_counters, mass_2_32, f64_row_in_u32_table, unknown_form, depth_33]


@pytest.mark.parametrize("case", _refusals(), ids=lambda f: f.__name__)
def test_writer_refuses_what_the_loader_would(case):
    kw = case()
    kw.setdefault("a", A)
    kw.setdefault("b", B)
    with pytest.raises(ValueError):
        ck.build_checkpoint(kw.pop("counters"), kw.pop("a"), kw.pop("b"), **kw)
