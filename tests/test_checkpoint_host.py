"""CPU: the checkpoint image (format version 1, DESIGN.md 3 "Checkpoint
image") on the host alone -- no device call anywhere here.

  * cms_checkpoint_info on files written by numpy from the documented layout;
  * the host validation of header and directory (cms_checkpoint.cpp) through
    tests/cpp/checkpoint_host_shim.cpp, every refusal the loader relies on;
  * the golden fixture tests/golden/ckpt_v1_small.bin, saved once on the GPU
    (tests/golden/make_ckpt_golden.py), decoded by the pure-numpy reader
    (mahout_amd.checkpoint) to exactly the oracle's table of the generator's
    seeded stream: the format stays readable as version 1.
"""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from mahout_amd import checkpoint as ck

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "checkpoint_host_shim.cpp")
LIB_SRC = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.cpp")
LIB_HDR = os.path.join(HERE, "..", "mahout_amd", "csrc", "cms_checkpoint.h")
OUT = os.path.join(HERE, "cpp", "_build", "libcheckpoint_host_shim.so")
GOLDEN = os.path.join(HERE, "golden", "ckpt_v1_small.bin")

CMS_E_PARAM = 1
F = {name: i for i, name in enumerate(ck.ROW_FORMS)}


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
    return lib


@pytest.fixture(scope="module")
def lib():
    from mahout_amd import build_lib, _lib
    build_lib.build()
    return _lib.load()


def make_image(n=6, d=4, w=128, rows=None, ids=None, counter_type=0, frac_bits=0, pairs=17, seed=42):
    """An image written from the documented layout alone.  rows: per owner
    (form name, place class, stored bytes); default: one row of several forms."""
    dw = d * w
    if rows is None:
        lst = np.concatenate([[2], np.arange(2 * d) % w]).astype("<u2").tobytes()  # m = 2
        rows = [("zero", 0, b""), ("list", 0, lst), ("u1", 4, bytes(dw // 8)), ("u4", 4, bytes([0x21]) * (dw // 2)),
                ("u16", 5, np.arange(dw, dtype="<u2").tobytes()), ("u32", 0, np.full(dw, 70000, "<u4").tobytes())][:n]
    assert len(rows) == n
    hd = np.zeros(1, ck.HEADER)
    ids_off, ids_bytes, dir_off, dir_bytes, payload_off = ck.section_layout(n, ids is not None)
    dire = np.zeros(n, ck.DIR_ENTRY)
    payload = bytearray()
    for r, (form, cls, raw) in enumerate(rows):
        dire[r] = (F[form], cls, 0, 3, len(raw), 5 * r, len(payload))
        payload += raw + bytes(-len(raw) % 16)
    h = hd[0]
    h["magic"], h["version"], h["header_bytes"] = ck.MAGIC, ck.VERSION, ck.HEADER_BYTES
    h["depth"], h["width"], h["counter_type"], h["frac_bits"] = d, w, counter_type, frac_bits
    h["num_owners"], h["pairs_ingested"], h["seed"] = n, pairs, seed
    h["flags"], h["dir_entry_bytes"] = (1 if ids is not None else 0), 32
    h["ids_off"], h["ids_bytes"], h["dir_off"], h["dir_bytes"] = ids_off, ids_bytes, dir_off, dir_bytes
    h["payload_off"], h["payload_bytes"] = payload_off, len(payload)
    h["checksum"] = ck.payload_checksum(bytes(payload))
    h["file_bytes"] = payload_off + len(payload)
    h["a"][:d] = np.arange(1, d + 1) * 1000003
    h["b"][:d] = np.arange(1, d + 1) * 7919
    out = bytearray(hd.tobytes())
    if ids is not None:
        out += np.asarray(ids, "<i8").tobytes()
    out += bytes(dir_off - len(out)) + dire.tobytes() + payload
    assert len(out) == int(h["file_bytes"])
    return out, hd, dire


def info(lib, path):
    from mahout_amd._lib import CmsParams
    p = CmsParams()
    nbytes = ctypes.c_int64()
    rc = lib.cms_checkpoint_info(os.fsencode(str(path)), ctypes.byref(p), ctypes.byref(nbytes))
    return rc, p, nbytes.value


# ---- cms_checkpoint_info ----

def test_info_returns_the_parameters(lib, tmp_path):
    img, _, _ = make_image(ids=[3, 5, 8, 13, 21, 34], frac_bits=2, seed=-7)
    path = tmp_path / "a.ckpt"
    path.write_bytes(img)
    rc, p, nbytes = info(lib, path)
    assert rc == 0, lib.cms_last_error()
    assert (p.struct_size, p.depth, p.width, p.counter_type, p.seed, p.num_owners, p.frac_bits) == (48, 4, 128, 0, -7, 6, 2)
    assert (p.weighting, p.device, p.flags) == (0, -1, 0)
    assert nbytes == len(img)
    c = ck.read_checkpoint(path)  # the two implementations agree on the same bytes
    assert (c.depth, c.width, c.num_owners, c.frac_bits, c.seed, c.pairs_ingested) == (4, 128, 6, 2, -7, 17)
    assert c.owner_ids.tolist() == [3, 5, 8, 13, 21, 34]
    assert [ck.ROW_FORMS[f] for f in c.forms] == ["zero", "list", "u1", "u4", "u16", "u32"]
    got = c.counters() * 4  # (preference units at frac_bits 2 -> counter units)
    assert got[0].sum() == 0 and got[2].sum() == 0
    assert np.all(got[3] == np.tile([1, 2], 256).reshape(4, 128))
    assert np.all(got[4].reshape(-1) == np.arange(512)) and np.all(got[5] == 70000)
    want = np.zeros((4, 128))
    for i, b in enumerate(np.arange(8) % 128):
        want[i // 2, b] += 1
    assert np.all(got[1] == want)


@pytest.mark.parametrize("case", ["magic", "version", "short", "section", "long", "missing"])
def test_info_refuses(lib, tmp_path, case):
    img, hd, _ = make_image()
    path = tmp_path / "bad.ckpt"
    if case == "magic":
        img[0:8] = b"NOTACKPT"
    elif case == "version":
        hd[0]["version"] = 2
        img[:ck.HEADER_BYTES] = hd.tobytes()
    elif case == "short":  # shorter than its header claims
        img = img[:-16]
    elif case == "section":  # a section past the end
        hd[0]["payload_off"] = len(img) + 64
        img[:ck.HEADER_BYTES] = hd.tobytes()
    elif case == "long":
        img = img + bytes(16)
    if case != "missing":
        path.write_bytes(img)
    rc, _, _ = info(lib, path)
    assert rc == CMS_E_PARAM
    assert lib.cms_last_error()


def test_info_refuses_a_truncated_header(lib, tmp_path):
    img, _, _ = make_image()
    path = tmp_path / "head.ckpt"
    path.write_bytes(img[:100])
    assert info(lib, path)[0] == CMS_E_PARAM


# ---- host validation of header and directory ----

def _check(shim, hd, dire):
    msg = shim.host_check_header(hd.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(int(hd[0]["file_bytes"])))
    if msg is not None:
        return msg
    return shim.host_check_directory(hd.ctypes.data_as(ctypes.c_void_p), dire.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.c_int64(dire.size))


def test_struct_sizes_match_the_documented_layout(shim):
    assert shim.host_header_bytes() == ck.HEADER_BYTES == ck.HEADER.itemsize
    assert shim.host_dir_entry_bytes() == ck.DIR_ENTRY.itemsize == 32
    hd = np.zeros(1, ck.HEADER)
    hd[0]["num_owners"], hd[0]["flags"] = 1000, 1
    shim.host_layout_sections(hd.ctypes.data_as(ctypes.c_void_p))
    got = tuple(int(hd[0][f]) for f in ("ids_off", "ids_bytes", "dir_off", "dir_bytes", "payload_off"))
    assert got == ck.section_layout(1000, True)


def test_valid_image_passes(shim):
    _, hd, dire = make_image()
    assert _check(shim, hd, dire) is None
    _, hd, dire = make_image(n=3, d=3, w=100, rows=[("u16", 5, bytes(600)), ("zero", 0, b""), ("u32", 0, bytes(1200))])
    assert _check(shim, hd, dire) is None
    _, hd, dire = make_image(n=2, d=2, w=7, counter_type=1, rows=[("f64", 0, bytes(112)), ("zero", 0, b"")])
    assert _check(shim, hd, dire) is None


def _mutations():
    def length(hd, dire):  # a length that disagrees with form and shape
        dire[3]["len"] = 128

    def list_length(hd, dire):  # not 2 + 2 d m for any m
        dire[1]["len"] = 20

    def list_long(hd, dire):  # m = 1025: past the longest list a build stores
        dire[1]["len"] = 2 + 2 * 4 * 1025

    def form(hd, dire):  # an unknown form
        dire[2]["form"] = 9

    def narrow_class(hd, dire):  # a place class narrower than the form
        dire[3]["cls"] = 2

    def u16_class(hd, dire):
        dire[4]["cls"] = 4

    def zero_place(hd, dire):
        dire[0]["cls"] = 5

    def descending(hd, dire):  # offsets not ascending
        dire[3]["off"], dire[4]["off"] = dire[4]["off"], dire[3]["off"]

    def unaligned(hd, dire):  # not 16-byte aligned
        dire[2]["off"] += 8

    def overlap(hd, dire):
        dire[5]["off"] -= 16

    def past_end(hd, dire):
        dire[5]["off"] += 16

    def reserved(hd, dire):
        dire[1]["rsv"] = 1

    def f64_row(hd, dire):  # an fp64 row in a u32 table
        dire[0]["form"], dire[0]["len"] = 8, 8 * 512

    return [length, list_length, list_long, form, narrow_class, u16_class, zero_place, descending, unaligned, overlap,
            past_end, reserved, f64_row]


@pytest.mark.parametrize("mutate", _mutations(), ids=lambda f: f.__name__)
def test_directory_refusals(shim, mutate):
    _, hd, dire = make_image()
    mutate(hd, dire)
    assert _check(shim, hd, dire) is not None


@pytest.mark.parametrize("form,w", [("u1", 64), ("u2", 32), ("u4", 48), ("u8", 100), ("list", 100)])
def test_forms_the_shape_cannot_hold_are_refused(shim, form, w):
    """1-bit rows need w % 128 == 0, 2-bit rows w % 64 == 0, any narrow form
    and list rows w % 32 == 0: the loader never hands such a row to a kernel."""
    d = 4
    dw = d * w
    raw = {"u1": bytes(dw // 8), "u2": bytes(dw // 4), "u4": bytes(dw // 2), "u8": bytes(dw),
           "list": np.array([1] + [0] * d, "<u2").tobytes()}[form]
    _, hd, dire = make_image(n=1, d=d, w=w, rows=[(form, 5, raw)])
    assert _check(shim, hd, dire) is not None


@pytest.mark.parametrize("field,value", [("depth", 0), ("depth", 33), ("width", 0), ("width", 40000), ("counter_type", 2),
                                         ("frac_bits", 32), ("num_owners", 0), ("flags", 2), ("payload_bytes", 8),
                                         ("dir_off", 0), ("ids_bytes", 8), ("header_bytes", 512)])
def test_header_refusals(shim, field, value):
    _, hd, dire = make_image()
    hd[0][field] = value
    assert _check(shim, hd, dire) is not None


def test_owner_ids_must_ascend(shim):
    ok = np.array([1, 2, 9], np.int64)
    bad = np.array([1, 9, 9], np.int64)
    assert shim.host_check_owner_ids(ok.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(3)) is None
    assert shim.host_check_owner_ids(bad.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(3)) is not None


def test_reader_refuses_what_the_library_refuses(tmp_path):
    img, _, _ = make_image()
    img[-1] ^= 0x40  # one payload byte flipped
    with pytest.raises(ValueError):
        ck.Checkpoint(bytes(img))
    img, _, _ = make_image()
    with pytest.raises(ValueError):
        ck.Checkpoint(bytes(img[:-16]))


# ---- the golden fixture ----

def test_golden_fixture_decodes_to_the_oracle_table(lib, oracle):
    spec = importlib.util.spec_from_file_location("make_ckpt_golden", os.path.join(HERE, "golden", "make_ckpt_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    rc, p, nbytes = info(lib, GOLDEN)
    assert rc == 0 and nbytes == os.path.getsize(GOLDEN)
    assert (p.num_owners, p.depth, p.width, p.seed, p.counter_type, p.frac_bits) == (gen.N, gen.D, gen.W, gen.SEED, 0, 0)
    c = ck.read_checkpoint(GOLDEN)
    # every form a built table holds side by side (zero-row owners: tests/test_gpu_checkpoint.py)
    assert set(c.form_counts()) == set(ck.ROW_FORMS) - {"f64", "zero"}, c.form_counts()
    batches = gen.golden_stream()
    a, b = oracle.hash_params(gen.SEED, gen.D)
    assert np.array_equal(c.a, a) and np.array_equal(c.b, b)
    rows = np.concatenate([x[0] for x in batches])
    vals = np.concatenate([np.ones(x[0].size, np.float32) if x[2] is None else x[2] for x in batches])
    exp = oracle.build_table(gen.N, gen.D, gen.W, a, b, rows, np.concatenate([x[1] for x in batches]), vals)
    got = c.counters()
    assert np.array_equal(got, exp), np.flatnonzero((got != exp).any(axis=(1, 2)))
    assert c.pairs_ingested == rows.size
    mass = np.zeros(gen.N)
    np.add.at(mass, rows, vals)
    assert np.array_equal(c.masses.astype(np.float64), mass)
    assert c.owner_ids is None
