"""CPU: the per-row decisions of widen_rows (mahout_amd/csrc/cms_forms.h, the
functions k_widen_mark and k_widen_rows call) compiled for the host and
enumerated over their whole domain: every source form (an owner on the shared
zero row included), every bound at and around each form's capacity, both
values of to_u16, every class of the row's current place, and shapes with and
without forms, 1-bit and 2-bit rows.

The rule is restated here in plain Python; the shim is only asked what the
library decides and what its pack / unpack steps store.

  * fit: the bytes the chosen rewrite stores for the whole row never exceed
    the place the row was given (its own when it stays, the mover's new one);
  * target: the form equals the restated rule, is wider than the source,
    holds the bound, and is 1-bit / 2-bit only at the widths that allow it;
  * round trip: unpack then pack at every reachable width reproduces the
    counters and stores exactly the bytes of the lane's 16 counters;
  * place classes: a place of a class's size is read back as at least that
    class, and no 1-bit place exists below 16 counters.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "forms_host_shim.hip")
HDR = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_forms.h")
OUT = os.path.join(HERE, "cpp", "_build", "libforms_host_shim.so")

SOURCES = ("zero", "list", "u1", "u2", "u4", "u8", "u16")
BITS = {"zero": 0, "list": 0, "u1": 1, "u2": 2, "u4": 4, "u8": 8, "u16": 16}
CAP = {0: 0, 1: 1, 2: 3, 4: 15, 8: 255, 16: 65535}  # largest counter of a form, by its bits
NBS = (0, 1, 2, 3, 4, 15, 16, 255, 256, 65535, 65536)
CLASS_BITS = (0, 1, 2, 4, 8, 16)  # kCapNone, kCapU1 .. kCapU16: the bits of the widest form a place holds
SHAPES = ((1, 1), (1, 16), (32, 16), (2, 48), (4, 96), (1, 128), (4, 192), (3, 1000), (4, 1024), (5, 1024),
          (9, 1024), (5, 8192), (2, 32768))
ROW_ALIGN = 64  # u16 units


@pytest.fixture(scope="module")
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", SRC, "-o",
                               OUT])
    lib = ctypes.CDLL(OUT)
    ll, i, vp = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p
    lib.fh_form_cap.restype = ctypes.c_uint
    lib.fh_class_units.restype = ll
    lib.fh_class_units.argtypes = [i, ll]
    lib.fh_class_of_units.argtypes = [ll, ll]
    lib.fh_widen_needed.argtypes = [i, i, ctypes.c_ulonglong, i]
    lib.fh_widen_target.argtypes = [i, i, ctypes.c_uint, i, i]
    lib.fh_rewrite_extent.restype = ll
    lib.fh_rewrite_extent.argtypes = [i, i, i, i]
    lib.fh_unpack_row.restype = None
    lib.fh_unpack_row.argtypes = [i, vp, ll, vp]
    lib.fh_pack16.argtypes = [i, vp, vp, ll]
    lib.fh_pack_counts_word.restype = None
    lib.fh_pack_counts_word.argtypes = [i, vp, vp, ll, i, i]
    names = ("u16", "u8", "u4", "u2", "u1", "list")
    lib.form = {nm: lib.fh_const(k) for k, nm in enumerate(names)}  # form name -> the library's code
    lib.form["zero"] = lib.form["u16"]  # an owner on the zero row reads as u16
    lib.bits_of = {lib.form[nm]: BITS[nm] for nm in names}
    lib.cls = {b: lib.fh_const(6 + k) for k, b in enumerate(CLASS_BITS)}  # class bits -> kCap code
    lib.cls_bits = {v: k for k, v in lib.cls.items()}
    assert lib.fh_const(12) == ROW_ALIGN
    return lib


# ---- the rule, restated ----

def units_of(cbits, dw):
    """u16 units of a place of the class whose widest form has cbits bits."""
    raw = dw if cbits == 16 else dw * cbits // 16
    return (raw + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN


def target_bits(src, nb, to_u16, w):
    sb = BITS[src]
    if to_u16 or w % 32:  # an accumulate build; no forms at this width
        return 16
    for tb, align in ((1, 128), (2, 64), (4, 1), (8, 1)):
        if sb < tb and nb <= CAP[tb] and w % align == 0:
            return tb
    return 16


def plan(src, nb, to_u16, cbits, d, w):
    """(target bits, stays in place, bits of the place's class, re-count branch, bytes stored)."""
    dw = d * w
    tb = target_bits(src, nb, to_u16, w)
    stays = src != "zero" and cbits >= tb
    place = cbits if stays else (16 if tb >= 8 else 8)  # a mover: a u8 place below u8, else a whole slot
    recount = src in ("zero", "list")
    stored = d * (w // (32 // tb)) * 4 if recount else (dw + 15) // 16 * 16 * tb // 8
    return tb, stays, place, recount, stored


def domain():
    for d, w in SHAPES:
        for src in SOURCES:
            for nb in NBS:
                for to_u16 in (0, 1):
                    for cbits in CLASS_BITS:
                        yield src, nb, to_u16, cbits, d, w


def lib_plan(shim, src, nb, to_u16, cbits, d, w, extents):
    f, zero = shim.form[src], int(src == "zero")
    tf = shim.fh_widen_target(f, zero, nb, to_u16, w)
    stays = bool(shim.fh_widen_in_place(zero, shim.cls[cbits], tf))
    place = cbits if stays else shim.cls_bits[shim.fh_widen_move_class(tf)]
    recount = bool(shim.fh_widen_recount(f, zero))
    key = (recount, shim.bits_of[tf], d, w)
    if key not in extents:
        extents[key] = shim.fh_rewrite_extent(int(recount), shim.bits_of[tf], d, w)
    return shim.bits_of[tf], stays, place, recount, extents[key]


def test_rewrite_fits_its_place(shim):
    """No (source, bound, to_u16, place class, shape) makes the rewrite store
    more bytes than the place the row was given, and none reaches a pack width
    the dense pack refuses.  (Before the zero-row rule moved into
    widen_recount, a zero-row owner with nb <= 1 at w % 128 == 0 was packed as
    u16 into a u8 place: 2 dw bytes into dw.)"""
    extents, seen = {}, 0
    for case in domain():
        src, nb, to_u16, cbits, d, w = case
        tb, stays, place, recount, stored = lib_plan(shim, *case, extents)
        assert stored >= 0, ("the dense pack has no case for", case, tb)
        room = 2 * shim.fh_class_units(shim.cls[place], d * w)
        assert room == 2 * units_of(place, d * w), case
        assert stored <= room, (case, tb, stays, place, stored, room)
        assert (tb, stays, place, recount, stored) == plan(*case), case
        seen += 1
    assert seen == len(SHAPES) * len(SOURCES) * len(NBS) * 2 * len(CLASS_BITS)


def test_target_rules(shim):
    for src, nb, to_u16, cbits, d, w in domain():
        if cbits:
            continue  # (the target does not depend on the place)
        f, zero = shim.form[src], int(src == "zero")
        tb = shim.bits_of[shim.fh_widen_target(f, zero, nb, to_u16, w)]
        case = (src, nb, to_u16, d, w)
        assert tb == target_bits(src, nb, to_u16, w), case
        sb = BITS[src]
        assert tb > sb or tb == 16, case  # strictly wider; u16 is the widest narrow form
        if not to_u16 and w % 32 == 0 and tb < 16:
            # the narrowest such form: the next narrower one is the source's, misses nb, or needs another width
            for nb2, align in ((1, 128), (2, 64), (4, 1), (8, 1)):
                if nb2 < tb:
                    assert nb2 <= sb or nb > CAP[nb2] or w % align, case
        # the form holds the bound (a row whose bound reaches 2^16 is promoted
        # to a u32 slot before widen_rows sees it: nb = 65536 only checks u16)
        assert CAP[tb] >= min(nb, 65535), case
        if tb == 1:
            assert w % 128 == 0 and d * w >= 16, case
        if tb == 2:
            assert w % 64 == 0, case
        # a touched row is rewritten when its form cannot hold nb, on the zero row, or by an accumulate build
        for all_touched in (0, 1):
            want = bool(all_touched) or src == "zero" or nb > CAP[sb]
            assert bool(shim.fh_widen_needed(f, zero, nb, all_touched)) == want, case
        assert bool(shim.fh_widen_recount(f, zero)) == (src in ("zero", "list")), case
    for nm, b in BITS.items():
        if nm != "zero":
            assert shim.fh_form_bits(shim.form[nm]) == b and shim.fh_form_cap(shim.form[nm]) == CAP[b]


def _encode(counters, bits):
    """counter j in bits bits*(j % (8/bits)) of byte j*bits/8 (u16: little-endian) -- cms_internal.h."""
    c = np.asarray(counters, np.uint64)
    if bits == 16:
        return c.astype("<u2").view(np.uint8).copy()
    per = 8 // bits
    c = c.reshape(-1, per)
    return (c << (np.arange(per, dtype=np.uint64) * np.uint64(bits))).sum(axis=1).astype(np.uint8)


def _decode(raw, bits, count):
    raw = np.asarray(raw, np.uint8)
    if bits == 16:
        return raw.view("<u2")[:count].astype(np.uint32)
    per = 8 // bits
    sh = (np.arange(per) * bits).astype(np.uint8)
    return ((raw[:, None] >> sh) & ((1 << bits) - 1)).reshape(-1)[:count].astype(np.uint32)


def _aligned(nbytes, fill):
    buf = np.full(nbytes + 64, fill, np.uint8)
    o = (-buf.ctypes.data) % 64
    return buf[o:o + nbytes]


@pytest.mark.parametrize("sb", [1, 2, 4, 8, 16])
def test_dense_round_trip(shim, sb):
    """unpack16 reads what the form's layout stores, and pack16_bits at every
    reachable width stores exactly bytes [j tb / 8, (j + 16) tb / 8) -- words
    [j tb / 32, (j + 16) tb / 32) -- holding the same counters."""
    lanes = 37
    n = lanes * 16
    rng = np.random.Generator(np.random.PCG64(sb))
    counters = rng.integers(0, CAP[sb] + 1, n).astype(np.uint32)
    counters[:4] = (CAP[sb], 0, CAP[sb], 1)
    f = {v: k for k, v in shim.bits_of.items()}[sb]
    row = _aligned(n * sb // 8, 0)
    row[:] = _encode(counters, sb)
    got = np.zeros(n, np.uint32)
    shim.fh_unpack_row(f, row.ctypes.data, lanes, got.ctypes.data)
    assert np.array_equal(got, counters)
    reachable = [tb for tb in (2, 4, 8, 16) if tb > sb or tb == 16]
    for tb in (1, 2, 4, 8, 16):
        out = _aligned(n * tb // 8 + 64, 0xA5)
        for lane in range(lanes):
            j = lane * 16
            before = out.copy()
            ok = shim.fh_pack16(tb, got[j:j + 16].ctypes.data, out.ctypes.data, j)
            if tb == 1:
                assert not ok and np.array_equal(out, before)  # refused: nothing stored
                continue
            assert ok
            lo, hi = j * tb // 8, (j + 16) * tb // 8
            assert lo % 4 == 0 and hi % 4 == 0 and (lo // 4, hi // 4) == (j * tb // 32, (j + 16) * tb // 32)
            assert np.array_equal(out[:lo], before[:lo]) and np.array_equal(out[hi:], before[hi:])
        if tb == 1:
            continue
        assert np.all(out[n * tb // 8:] == 0xA5)
        if tb in reachable:
            assert np.array_equal(_decode(out[:n * tb // 8], tb, n), counters), (sb, tb)


@pytest.mark.parametrize("src", ["list", "zero"])
@pytest.mark.parametrize("d,w", [(3, 128), (2, 192), (4, 96)])
def test_recount_round_trip(shim, src, d, w):
    """The list re-count's pack (a list row's counters are < 2^8; a zero-row
    owner's are all 0) at every target width the shape allows: word q of
    sketch row rr goes to word rr w tb / 32 + q and nowhere else."""
    rng = np.random.Generator(np.random.PCG64(w))
    for tb in (1, 2, 4, 8, 16):
        if (tb == 1 and w % 128) or (tb == 2 and w % 64):
            continue
        counts = rng.integers(0, min(CAP[tb], 255) + 1, (d, w)).astype(np.uint8)
        if src == "zero":
            counts[:] = 0
        nbytes = d * w * tb // 8
        out = _aligned(nbytes + 64, 0xA5)
        cpw = 32 // tb
        for rr in range(d):
            c8 = _aligned(w, 0)
            c8[:] = counts[rr]
            for q in range(w // cpw):
                before = out.copy()
                shim.fh_pack_counts_word(tb, c8.ctypes.data, out.ctypes.data, rr, w, q)
                at = 4 * (rr * w // cpw + q)
                assert np.array_equal(out[:at], before[:at]) and np.array_equal(out[at + 4:], before[at + 4:])
        assert np.all(out[nbytes:] == 0xA5)
        assert np.array_equal(_decode(out[:nbytes], tb, d * w), counts.reshape(-1)), (src, tb)


def test_place_classes(shim):
    for d, w in SHAPES:
        dw = d * w
        for cbits in CLASS_BITS:
            u = shim.fh_class_units(shim.cls[cbits], dw)
            assert u == units_of(cbits, dw) and u % ROW_ALIGN == 0
            assert shim.fh_class_of_units(u, dw) >= shim.cls[cbits], (d, w, cbits)
            if cbits == 16 or w % 32 == 0:  # (narrow forms exist only at w % 32 == 0)
                assert 2 * u >= (dw + 15) // 16 * 16 * cbits // 8  # the place holds its class's widest form
        if dw < 16:
            for u in range(0, 4 * ROW_ALIGN + 1, ROW_ALIGN):
                assert shim.fh_class_of_units(u, dw) != shim.cls[1], (d, w, u)
    for nm in ("u1", "u2", "u4", "u8", "u16", "list"):
        assert shim.cls_bits[shim.fh_form_class(shim.form[nm])] == BITS[nm]
        want = 16 if nm in ("u8", "u16") else 8
        if nm != "list":
            assert shim.cls_bits[shim.fh_widen_move_class(shim.form[nm])] == want
