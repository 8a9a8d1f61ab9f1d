"""read_checkpoint / write_checkpoint: a pure-numpy reader and writer of the
checkpoint image (format version 1, DESIGN.md 3 "Checkpoint image") -- no GPU
and no library.

The format's independent second implementation (the tests decode what the GPU
wrote with the reader, and load tables designed counter by counter through the
writer: build_checkpoint) and an inspection tool:

    python -m mahout_amd.checkpoint table.ckpt

Layout, little-endian throughout:

    [0, 640)        header (HEADER below)
    [640, +8 n)     owner IDs, i64 [n] -- only with header flag bit 0
    dir_off         row directory, one 32-byte DIR_ENTRY per owner row
    payload_off     every row's stored bytes in row order, each row on a
                    16-byte boundary, pad bytes zero
"""
import numpy as np

MAGIC = b"MCMSCKPT"
VERSION = 1
HEADER_BYTES = 640
FLAG_OWNER_IDS = 1

HEADER = np.dtype([
    ("magic", "S8"), ("version", "<u4"), ("header_bytes", "<u4"),
    ("depth", "<i4"), ("width", "<i4"), ("counter_type", "<i4"), ("frac_bits", "<i4"),
    ("num_owners", "<i8"), ("pairs_ingested", "<i8"), ("seed", "<i8"),
    ("flags", "<u4"), ("dir_entry_bytes", "<u4"),
    ("ids_off", "<u8"), ("ids_bytes", "<u8"), ("dir_off", "<u8"), ("dir_bytes", "<u8"),
    ("payload_off", "<u8"), ("payload_bytes", "<u8"), ("checksum", "<u8"), ("file_bytes", "<u8"),
    ("a", "<i8", (32,)), ("b", "<i8", (32,)),
])
assert HEADER.itemsize == HEADER_BYTES

DIR_ENTRY = np.dtype([
    ("form", "u1"), ("cls", "u1"), ("rsv", "<u2"), ("cbound", "<u4"),
    ("len", "<u8"), ("mass", "<u8"), ("off", "<u8"),
])
assert DIR_ENTRY.itemsize == 32

# stored forms (DirEntry.form)
ROW_FORMS = ("zero", "list", "u1", "u2", "u4", "u8", "u16", "u32", "f64")
_BITS = {"u1": 1, "u2": 2, "u4": 4, "u8": 8, "u16": 16, "u32": 32, "f64": 64}


def payload_checksum(payload):
    """Sum modulo 2^64 of the payload read as little-endian u64 words."""
    words = np.frombuffer(payload, "<u8")
    return int(np.add.reduce(words, dtype=np.uint64)) if words.size else 0


def section_layout(num_owners, has_ids):
    """(ids_off, ids_bytes, dir_off, dir_bytes, payload_off) of an image."""
    ids_bytes = 8 * num_owners if has_ids else 0
    dir_off = (HEADER_BYTES + ids_bytes + 15) // 16 * 16
    dir_bytes = DIR_ENTRY.itemsize * num_owners
    return HEADER_BYTES, ids_bytes, dir_off, dir_bytes, dir_off + dir_bytes


def row_length(form, depth, width, m=0):
    """Stored bytes of a row of this form (m: a list row's key count)."""
    name = ROW_FORMS[form]
    if name == "zero":
        return 0
    if name == "list":
        return 2 + 2 * depth * m
    return depth * width * _BITS[name] // 8


class Checkpoint:
    """A decoded image: the header fields as attributes, `owner_ids` (None
    without explicit IDs), per-row `forms` (indices into ROW_FORMS),
    `classes`, `bounds`, `masses`, `lengths`, `offsets`, and counters(rows)."""

    def __init__(self, data):
        buf = memoryview(data)
        if len(buf) < HEADER_BYTES:
            raise ValueError("shorter than a checkpoint header")
        hd = np.frombuffer(buf[:HEADER_BYTES], HEADER)[0]
        if bytes(hd["magic"]).ljust(8, b"\0") != MAGIC:
            raise ValueError("not a checkpoint image (bad magic)")
        if int(hd["version"]) != VERSION:
            raise ValueError("unknown checkpoint format version %d" % int(hd["version"]))
        self.header = hd
        for f in ("depth", "width", "counter_type", "frac_bits", "num_owners", "pairs_ingested", "seed", "flags",
                  "payload_off", "payload_bytes", "checksum", "file_bytes"):
            setattr(self, f, int(hd[f]))
        n, d = self.num_owners, self.depth
        has_ids = bool(self.flags & FLAG_OWNER_IDS)
        want = section_layout(n, has_ids)
        got = tuple(int(hd[f]) for f in ("ids_off", "ids_bytes", "dir_off", "dir_bytes", "payload_off"))
        if got != want or int(hd["header_bytes"]) != HEADER_BYTES or int(hd["dir_entry_bytes"]) != DIR_ENTRY.itemsize:
            raise ValueError("section offsets disagree with the shape")
        if self.file_bytes != self.payload_off + self.payload_bytes or len(buf) != self.file_bytes:
            raise ValueError("length disagrees with the header")
        self.a = np.array(hd["a"][:d], np.int64)
        self.b = np.array(hd["b"][:d], np.int64)
        ids_off, ids_bytes, dir_off, dir_bytes, _ = want
        self.owner_ids = np.frombuffer(buf[ids_off:ids_off + ids_bytes], "<i8").copy() if has_ids else None
        self.directory = np.frombuffer(buf[dir_off:dir_off + dir_bytes], DIR_ENTRY)
        self.forms = self.directory["form"].astype(np.int32)
        self.classes = self.directory["cls"].astype(np.int32)
        self.bounds = self.directory["cbound"].astype(np.uint32)
        self.masses = self.directory["mass"].astype(np.uint64)
        self.lengths = self.directory["len"].astype(np.int64)
        self.offsets = self.directory["off"].astype(np.int64)
        self.payload = buf[self.payload_off:self.payload_off + self.payload_bytes]
        if self.forms.size and int(self.forms.max()) >= len(ROW_FORMS):
            raise ValueError("unknown row form")
        ends = self.offsets + (self.lengths + 15) // 16 * 16
        starts = np.concatenate([[0], ends[:-1]]) if n else ends
        if np.any(self.offsets != starts) or (n and int(ends[-1]) != self.payload_bytes):
            raise ValueError("payload offsets do not tile the payload in row order")
        if payload_checksum(self.payload) != self.checksum:
            raise ValueError("payload checksum mismatch")

    def row_bytes(self, r):
        o, ln = int(self.offsets[r]), int(self.lengths[r])
        return np.frombuffer(self.payload[o:o + ln], np.uint8)

    def row_counters(self, r):
        """Counters [d][w] of owner row r in counter units: uint64 for a u32
        table, float64 for an fp64 one."""
        d, w = self.depth, self.width
        name = ROW_FORMS[int(self.forms[r])]
        raw = self.row_bytes(r)
        if name != "zero" and raw.size != row_length(int(self.forms[r]), d, w, (raw.size - 2) // (2 * d)):
            raise ValueError("row %d: length disagrees with its form" % r)
        if name == "zero":
            return np.zeros((d, w), np.float64 if self.counter_type == 1 else np.uint64)
        if name == "list":
            e = raw.view("<u2")
            m = int(e[0])
            if e.size != 1 + d * m:
                raise ValueError("row %d: list key count disagrees with its length" % r)
            out = np.zeros((d, w), np.uint64)
            ent = e[1:].reshape(d, m).astype(np.int64)
            if m and int(ent.max()) >= w:
                raise ValueError("row %d: list entry outside the sketch row" % r)
            for i in range(d):
                out[i] = np.bincount(ent[i], minlength=w)
            return out
        if name == "f64":
            return raw.view("<f8").reshape(d, w).copy()
        bits = _BITS[name]
        if bits >= 8:
            return raw.view("<u%d" % (bits // 8)).astype(np.uint64).reshape(d, w)
        per = 8 // bits  # counter j in bits (j % per) * bits of byte j // per
        sh = (np.arange(per, dtype=np.uint8) * bits)[None, :]
        vals = (raw[:, None] >> sh) & np.uint8((1 << bits) - 1)
        return vals.reshape(-1).astype(np.uint64).reshape(d, w)

    def counters(self, rows=None):
        """[len(rows)][d][w] float64 in preference units, as read_counters()
        returns them (all rows when rows is None)."""
        rows = np.arange(self.num_owners) if rows is None else np.asarray(rows, np.int64)
        out = np.zeros((rows.size, self.depth, self.width), np.float64)
        for i, r in enumerate(rows.tolist()):
            out[i] = self.row_counters(r)
        if self.counter_type == 0 and self.frac_bits:
            out = np.ldexp(out, -self.frac_bits)
        return out

    def list_entries(self, r):
        """The stored entries [d][m] (u16 buckets, in stored order) of list row r."""
        if ROW_FORMS[int(self.forms[r])] != "list":
            raise ValueError("row %d is not a list row" % r)
        e = self.row_bytes(r).view("<u2")
        m = int(e[0])
        if e.size != 1 + self.depth * m:
            raise ValueError("row %d: list key count disagrees with its length" % r)
        return e[1:].reshape(self.depth, m).copy()

    def form_counts(self):
        return {ROW_FORMS[f]: int(c) for f, c in enumerate(np.bincount(self.forms, minlength=len(ROW_FORMS))) if c}


def read_checkpoint(path):
    """Decode a checkpoint file (ValueError when it is not a valid image)."""
    with open(path, "rb") as f:
        return Checkpoint(f.read())


# ---- the writer ----

_FORM = {name: i for i, name in enumerate(ROW_FORMS)}
_NARROW = ("u1", "u2", "u4", "u8", "u16")           # place classes 1..5
LIST_MAX_KEYS, LIST_MAX_ENTRIES = 1024, 8192        # the longest list a build stores (kListMaxKeys/Entries)
MAX_DEPTH, MAX_OWNERS = 32, 1 << 24


def shape_has_form(name, depth, width):
    """Whether a u32 table of this shape stores rows of this form: 1-bit rows
    need w % 128 == 0, 2-bit rows w % 64 == 0, any narrow form and lists
    w % 32 == 0, lists a u16 row of at most 80 KiB as well."""
    forms = width % 32 == 0
    if name == "u1":
        return forms and width % 128 == 0
    if name == "u2":
        return forms and width % 64 == 0
    if name in ("u4", "u8"):
        return forms
    if name == "list":
        return forms and 2 * depth * width <= 80 * 1024
    return name in ("zero", "u16", "u32")


def default_form(cmax, mass, depth, width):
    """The form (a ROW_FORMS name) a row with largest counter cmax and mass
    `mass` is stored in: u32 from 2^16 on, else the narrowest dense form that
    holds cmax among those the shape has."""
    if mass >= 1 << 16 or cmax >= 1 << 16:
        return "u32"
    for name in _NARROW:
        if cmax < 1 << _BITS[name] and shape_has_form(name, depth, width):
            return name
    return "u16"


def _pack_dense(c, name):
    """Rows [k][d*w] (uint64) of one dense form -> their stored bytes [k][len]."""
    bits = _BITS[name]
    if bits >= 8:
        return np.ascontiguousarray(c.astype("<u%d" % (bits // 8))).view(np.uint8).reshape(c.shape[0], -1)
    per = 8 // bits  # counter j in bits (j % per) * bits of byte j // per
    v = c.astype(np.uint8).reshape(c.shape[0], -1, per)
    sh = (np.arange(per, dtype=np.uint8) * bits)[None, None, :]
    return np.bitwise_or.reduce(v << sh, axis=2).astype(np.uint8)


def build_checkpoint(counters, a, b, *, seed=0, frac_bits=0, owner_ids=None, forms=None, classes=None, bounds=None,
                     masses=None, lists=None, pairs_ingested=None):
    """The checkpoint image (bytes) of a designed table: the format's writer.

    counters: [n][d][w] unsigned integers in counter units (a u32 table), or a
    float64 array (an fp64 table: every row form f64).  a, b: the hash
    parameters in use, at least d each.  The per-row arguments are sequences
    of n entries, or None for the defaults, which are what a saving handle
    writes:

      forms    ROW_FORMS names or indices; None or -1 for a row: u32 when the
               row's mass or a counter reaches 2^16, else the narrowest dense
               form the shape has that holds the largest counter (an all-zero
               row is a dense row of zeros; form "zero" only when asked for)
      classes  place classes; default the form's own (u1..u16 = 1..5), 0 for
               list, zero, u32 and f64 rows
      bounds   cbound; default the row's largest counter, 0 for u32/f64 rows
      masses   default the owner's largest row sum (0 in an fp64 table)
      lists    {row: entries [d][m]} or a sequence with None: the row is
               stored as that list, which must count to counters[row]
      pairs_ingested  default the sum of the masses

    ValueError for what the loader would refuse: a counter above its form's
    capacity, a form the shape lacks, a place class narrower than the form, a
    list past the stored limits or with an entry outside the row, a mass of
    2^32 or more (u32 counters), owner IDs that do not strictly ascend."""
    counters = np.asarray(counters)
    if counters.ndim != 3:
        raise ValueError("counters must be [n][d][w]")
    n, d, w = counters.shape
    f64 = counters.dtype.kind == "f"
    if not f64 and counters.dtype.kind not in "ui":
        raise ValueError("counters must be unsigned integers or float64")
    if not f64 and counters.dtype.kind == "i" and counters.size and int(counters.min()) < 0:
        raise ValueError("negative counter")
    if not 1 <= d <= MAX_DEPTH or not 1 <= w <= (1 << 20 if f64 else 1 << 15) or not 1 <= n <= MAX_OWNERS:
        raise ValueError("shape outside what a handle holds")
    if not 0 <= frac_bits <= 31:
        raise ValueError("frac_bits outside [0, 31]")
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.size < d or b.size < d or a.size > 32 or b.size > 32:
        raise ValueError("one (a, b) per sketch row")
    if owner_ids is not None:
        owner_ids = np.asarray(owner_ids, np.int64)
        if owner_ids.shape != (n,) or np.any(np.diff(owner_ids) <= 0):
            raise ValueError("owner IDs must be n strictly ascending values")
    dw = d * w
    flat = counters.reshape(n, dw)
    if f64:
        flat = flat.astype(np.float64)
        cmax = np.zeros(n, np.uint64)
        mass_def = np.zeros(n, np.uint64)
    else:
        flat = flat.astype(np.uint64)
        if flat.size and int(flat.max()) >= 1 << 32:
            raise ValueError("a counter of 2^32 or more")
        cmax = flat.max(axis=1)
        mass_def = counters.astype(np.uint64).sum(axis=2).max(axis=1)
    mass = mass_def if masses is None else np.asarray(masses, np.uint64)
    if mass.shape != (n,):
        raise ValueError("one mass per owner")
    if not f64 and np.any(mass >= np.uint64(1 << 32)):
        raise ValueError("a row mass of 2^32 or more (u32 counters)")
    if isinstance(lists, dict):
        lists = [lists.get(r) for r in range(n)]
    if lists is not None and len(lists) != n:
        raise ValueError("one list (or None) per owner")

    # -- forms --
    form = np.full(n, -1, np.int32)
    if forms is not None:
        if len(forms) != n:
            raise ValueError("one form per owner")
        for r, f in enumerate(forms):
            if f is None:
                continue
            f = _FORM.get(f, f) if isinstance(f, str) else int(f)
            if not isinstance(f, int) or not -1 <= f < len(ROW_FORMS):
                raise ValueError("row %d: unknown row form" % r)
            form[r] = f
    if lists is not None:
        for r, ent in enumerate(lists):
            if ent is None:
                continue
            if form[r] not in (-1, _FORM["list"]):
                raise ValueError("row %d: list entries for a row of another form" % r)
            form[r] = _FORM["list"]
    todo = np.flatnonzero(form < 0)
    if f64:
        form[todo] = _FORM["f64"]
    elif todo.size:
        # (vectorised default_form)
        pick = np.full(todo.size, _FORM["u16"], np.int32)
        for name in reversed(_NARROW[:-1]):
            if shape_has_form(name, d, w):
                pick[cmax[todo] < np.uint64(1 << _BITS[name])] = _FORM[name]
        pick[(mass[todo] >= np.uint64(1 << 16)) | (cmax[todo] >= np.uint64(1 << 16))] = _FORM["u32"]
        form[todo] = pick

    # -- every check the loader makes, and the counters against their forms --
    need_cls = np.zeros(n, np.int32)
    length = np.zeros(n, np.int64)
    list_raw = {}
    for fi, name in enumerate(ROW_FORMS):
        rows = np.flatnonzero(form == fi)
        if rows.size == 0:
            continue
        if f64 != (name == "f64") and name != "zero":
            raise ValueError("row %d: a %s row in %s table" % (rows[0], name, "an fp64" if f64 else "a u32"))
        if not f64 and not shape_has_form(name, d, w):
            raise ValueError("row %d: a %s row in a shape that has none" % (rows[0], name))
        if name == "zero":
            if np.any(flat[rows] != 0):
                raise ValueError("a zero row with counters")
        elif name == "list":
            for r in rows.tolist():
                ent = None if lists is None else lists[r]
                if ent is None:
                    raise ValueError("row %d: a list row needs its entries" % r)
                ent = np.asarray(ent)
                if ent.ndim != 2 or ent.shape[0] != d:
                    raise ValueError("row %d: list entries must be [d][m]" % r)
                m = ent.shape[1]
                ln = 2 + 2 * d * m
                if m > LIST_MAX_KEYS or m * d > LIST_MAX_ENTRIES or ln > 2 * dw:
                    raise ValueError("row %d: list row too long" % r)
                if m and (int(ent.min()) < 0 or int(ent.max()) >= w):
                    raise ValueError("row %d: list entry outside the sketch row" % r)
                cnt = np.stack([np.bincount(ent[i].astype(np.int64), minlength=w) for i in range(d)]) if m else 0
                if np.any(flat[r].reshape(d, w) != cnt):
                    raise ValueError("row %d: the list does not count to the row's counters" % r)
                list_raw[r] = np.concatenate([[m], ent.reshape(-1)]).astype("<u2").view(np.uint8)
                length[r] = ln
        else:
            if name in _NARROW:
                need_cls[rows] = 1 + _NARROW.index(name)
            if not f64 and _BITS[name] < 64 and np.any(cmax[rows] >= np.uint64(1) << np.uint64(_BITS[name])):
                bad = rows[cmax[rows] >= np.uint64(1) << np.uint64(_BITS[name])][0]
                raise ValueError("row %d: a counter above the capacity of form %s" % (bad, name))
            length[rows] = dw * _BITS[name] // 8
    cls = need_cls.copy() if classes is None else np.asarray(classes, np.int32)
    if cls.shape != (n,) or np.any(cls < need_cls) or np.any(cls > 5):
        raise ValueError("a place class narrower than the row's form, or unknown")
    no_place = np.isin(form, [_FORM["zero"], _FORM["u32"], _FORM["f64"]])
    if np.any(cls[no_place] != 0):
        raise ValueError("zero, u32 and f64 rows have no arena place")
    if bounds is None:
        cb = np.where(no_place & (form != _FORM["zero"]), 0, cmax).astype(np.uint64)
    else:
        cb = np.asarray(bounds, np.uint64)
    if cb.shape != (n,) or np.any(cb >= np.uint64(1 << 32)):
        raise ValueError("one u32 cbound per owner")

    # -- layout and payload --
    padded = (length + 15) // 16 * 16
    off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    payload = np.zeros(int(padded.sum()), np.uint8)
    for fi, name in enumerate(ROW_FORMS):
        rows = np.flatnonzero(form == fi)
        if rows.size == 0 or name in ("zero", "list"):
            continue
        raw = (np.ascontiguousarray(flat[rows].astype("<f8")).view(np.uint8).reshape(rows.size, -1) if name == "f64"
               else _pack_dense(flat[rows], name))
        payload[off[rows][:, None] + np.arange(raw.shape[1])[None, :]] = raw
    for r, raw in list_raw.items():
        payload[off[r]:off[r] + raw.size] = raw
    payload = payload.tobytes()

    dire = np.zeros(n, DIR_ENTRY)
    dire["form"], dire["cls"], dire["cbound"] = form, cls, cb
    dire["len"], dire["mass"], dire["off"] = length, mass, off
    hd = np.zeros(1, HEADER)
    h = hd[0]
    ids_off, ids_bytes, dir_off, dir_bytes, payload_off = section_layout(n, owner_ids is not None)
    h["magic"], h["version"], h["header_bytes"] = MAGIC, VERSION, HEADER_BYTES
    h["depth"], h["width"], h["counter_type"], h["frac_bits"] = d, w, int(f64), frac_bits
    h["num_owners"], h["seed"] = n, seed
    h["pairs_ingested"] = int(mass.sum(dtype=np.uint64)) if pairs_ingested is None else int(pairs_ingested)
    if int(h["pairs_ingested"]) < 0:
        raise ValueError("negative pairs_ingested")
    h["flags"], h["dir_entry_bytes"] = (FLAG_OWNER_IDS if owner_ids is not None else 0), DIR_ENTRY.itemsize
    h["ids_off"], h["ids_bytes"], h["dir_off"], h["dir_bytes"] = ids_off, ids_bytes, dir_off, dir_bytes
    h["payload_off"], h["payload_bytes"] = payload_off, len(payload)
    h["checksum"] = payload_checksum(payload)
    h["file_bytes"] = payload_off + len(payload)
    h["a"][:d], h["b"][:d] = a[:d], b[:d]
    out = bytearray(hd.tobytes())
    if owner_ids is not None:
        out += owner_ids.astype("<i8").tobytes()
    out += bytes(dir_off - len(out)) + dire.tobytes() + payload
    assert len(out) == int(h["file_bytes"])
    return bytes(out)


def write_checkpoint(path, counters, a, b, **kw):
    """build_checkpoint(...) written to `path`; returns the byte count."""
    data = build_checkpoint(counters, a, b, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def sum_counters(paths_or_checkpoints):
    """The counters [n][d][w] (as Checkpoint.counters()) of the images' streams
    together: the no-GPU specification of SketchTable.merge.  A count-min
    sketch is linear, so tables built with the same hash functions add counter
    by counter.  The images must agree in shape, counter type, frac_bits, the
    hash parameters in use (a_i, b_i for i < depth) and their owner IDs (all
    absent, or all identical), and -- u32 counters -- no row's summed mass may
    reach 2^32: ValueError otherwise, as the library refuses the merge."""
    cks = [c if isinstance(c, Checkpoint) else read_checkpoint(c) for c in paths_or_checkpoints]
    if not cks:
        raise ValueError("no checkpoint to sum")
    first = cks[0]
    total = first.counters()
    mass = first.masses.copy()
    for c in cks[1:]:
        for f in ("depth", "width", "num_owners", "counter_type", "frac_bits"):
            if getattr(c, f) != getattr(first, f):
                raise ValueError("checkpoints differ in %s" % f)
        if not (np.array_equal(c.a, first.a) and np.array_equal(c.b, first.b)):
            raise ValueError("checkpoints were built with different hash parameters")
        if (c.owner_ids is None) != (first.owner_ids is None) or (
                c.owner_ids is not None and not np.array_equal(c.owner_ids, first.owner_ids)):
            raise ValueError("checkpoints differ in their owner IDs")
        if first.counter_type == 0:
            if np.any(mass >= 2 ** 32) or np.any(c.masses >= 2 ** 32) or np.any(mass + c.masses >= 2 ** 32):
                raise ValueError("a row's total increment reached 2^32 (u32 counters)")
        mass = mass + c.masses
        total = total + c.counters()
    return total


def diff_counters(minuend, subtrahend):
    """(counters [n][d][w] as Checkpoint.counters(), masses [n] uint64) of the
    minuend's stream without the subtrahend's: the no-GPU specification of
    SketchTable.subtract and the counterpart of sum_counters.  Both are paths
    or Checkpoint objects.  ValueError, as the library refuses the call, when
    the images differ in shape, counter type, frac_bits, the hash parameters in
    use or their owner IDs, when either holds fp64 counters ((a + b) - b is
    not a there), and when a row's mass or any single counter would fall below
    zero."""
    a, b = (c if isinstance(c, Checkpoint) else read_checkpoint(c) for c in (minuend, subtrahend))
    for f in ("depth", "width", "num_owners", "counter_type", "frac_bits"):
        if getattr(a, f) != getattr(b, f):
            raise ValueError("checkpoints differ in %s" % f)
    if a.counter_type != 0:
        raise ValueError("fp64 counters do not subtract")
    if not (np.array_equal(a.a, b.a) and np.array_equal(a.b, b.b)):
        raise ValueError("checkpoints were built with different hash parameters")
    if (a.owner_ids is None) != (b.owner_ids is None) or (
            a.owner_ids is not None and not np.array_equal(a.owner_ids, b.owner_ids)):
        raise ValueError("checkpoints differ in their owner IDs")
    if np.any(a.masses < b.masses):
        raise ValueError("row %d: the mass would fall below zero" % int(np.flatnonzero(a.masses < b.masses)[0]))
    out = np.zeros((a.num_owners, a.depth, a.width), np.float64)
    for r in range(a.num_owners):
        x, y = a.row_counters(r), b.row_counters(r)  # uint64, counter units
        if np.any(x < y):
            raise ValueError("row %d: a counter would fall below zero" % r)
        out[r] = x - y
    if a.frac_bits:
        out = np.ldexp(out, -a.frac_bits)
    return out, a.masses - b.masses


def compact_form(cmax, mass, row_sums, depth, width, frac_bits=0, list_keys=256, forms=True):
    """The form (a ROW_FORMS name) SketchTable.compact re-stores a u32 row in:
    the numpy twin of ckpt::compact_form (cms_checkpoint.cpp).  cmax: the
    row's largest counter; mass: its row mass; row_sums: the sums of its
    `depth` sketch rows (None: not known, which rules a list out); list_keys:
    the handle's list limit (CMS_LIST_KEYS; 0: no lists); forms: False for a
    handle that stores only zero / u16 / u32 rows (CMS_NO_FORMS).  In order:

      1. cmax == 0: "zero";
      2. mass >= 2^16 or cmax >= 2^16: "u32";
      3. D = the narrowest dense form the handle stores that holds cmax
         (default_form);
      4. "list" instead of D only when frac_bits == 0, the handle stores lists,
         every sketch row sums to the mass m, 1 <= m <= min(list_keys, 1024),
         depth * m <= 8192, 2 + 2 * depth * m < D's stored bytes, and
         cmax <= 255: no list holds a bucket more than 255 times, as no built
         list does (the library's writers re-count list entries in u8
         counters, so a fuller bucket would wrap at the next write)."""
    cmax, mass = int(cmax), int(mass)
    if cmax == 0:
        return "zero"
    if mass >= 1 << 16 or cmax >= 1 << 16:
        return "u32"
    dense = default_form(cmax, mass, depth, width) if forms else "u16"
    m = mass
    if (frac_bits == 0 and forms and list_keys > 0 and cmax <= 255 and shape_has_form("list", depth, width)
            and row_sums is not None
            and len(row_sums) == depth and all(int(s) == m for s in row_sums)
            and 1 <= m <= min(int(list_keys), LIST_MAX_KEYS) and depth * m <= LIST_MAX_ENTRIES
            and 2 + 2 * depth * m < row_length(_FORM[dense], depth, width)):
        return "list"
    return dense


def compact_checkpoint(ckpt_or_bytes, list_keys=256, forms=True):
    """The image (bytes) of the same table with every row in the form
    compact_form gives it, default place classes and bounds, the image's own
    masses, owner IDs, hash parameters, seed and pairs_ingested: the no-GPU
    specification of SketchTable.compact (save_device() after compact() is
    compact_checkpoint(save_device() before), with the handle's list_keys and
    forms).  A list row's entries are, per sketch row, the buckets in
    ascending order, bucket j repeated c[j] times.  u32 tables only."""
    c = ckpt_or_bytes if isinstance(ckpt_or_bytes, Checkpoint) else Checkpoint(ckpt_or_bytes)
    if c.counter_type != 0:
        raise ValueError("fp64 counters are stored in one form: there is nothing to narrow")
    n, d, w = c.num_owners, c.depth, c.width
    counters = np.zeros((n, d, w), np.uint64)
    names, lists = [], {}
    for r in range(n):
        x = c.row_counters(r)
        counters[r] = x
        name = compact_form(int(x.max()), int(c.masses[r]), x.sum(axis=1), d, w, c.frac_bits, list_keys, forms)
        if name == "list":
            lists[r] = np.stack([np.repeat(np.arange(w), x[i].astype(np.int64)) for i in range(d)])
        names.append(name)
    return build_checkpoint(counters, c.a, c.b, seed=c.seed, frac_bits=c.frac_bits, owner_ids=c.owner_ids, forms=names,
                            lists=lists, masses=c.masses, pairs_ingested=c.pairs_ingested)


def fold_checkpoint(ckpt_or_bytes, width, list_keys=256, forms=True):
    """The image (bytes) of the same stream's table at the narrower width
    `width`, a divisor of the image's: the no-GPU specification of
    SketchTable.fold_device.  The hash is ((a key + b) mod p)
    mod w and (s mod w) mod w' = s mod w' for every divisor w' of w, so

        T'[r][i][j'] = sum of T[r][i][j] over j = j' (mod w')

    is, counter for counter, the table the stream builds at width w' with the
    same hash parameters.  Every folded row is stored in the form compact_form
    gives it at shape (depth, width), with default place classes and bounds, as
    compact_checkpoint stores them; masses, owner IDs, hash parameters, seed,
    frac_bits and pairs_ingested are the image's own.  fold_checkpoint(img, w)
    at the image's own width is compact_checkpoint(img).  ValueError for a
    width that does not divide the image's, for an fp64 image (a folded fp64
    sum is not the reference's sequential chain in ingest order: no stream's
    table) and for a folded counter of 2^32 or more."""
    c = ckpt_or_bytes if isinstance(ckpt_or_bytes, Checkpoint) else Checkpoint(ckpt_or_bytes)
    if c.counter_type != 0:
        raise ValueError("fp64 counters do not fold: the folded sum would be no stream's table")
    n, d, w = c.num_owners, c.depth, c.width
    width = int(width)
    if not 1 <= width <= w or w % width:
        raise ValueError("width %d does not divide the image's width %d" % (width, w))
    counters = np.zeros((n, d, width), np.uint64)
    names, lists = [], {}
    for r in range(n):
        x = c.row_counters(r).reshape(d, w // width, width).sum(axis=1, dtype=np.uint64)  # (at most 2^15 u32 terms)
        if int(x.max()) >= 1 << 32:
            raise ValueError("row %d: a folded counter reaches 2^32" % r)
        counters[r] = x
        name = compact_form(int(x.max()), int(c.masses[r]), x.sum(axis=1), d, width, c.frac_bits, list_keys, forms)
        if name == "list":
            lists[r] = np.stack([np.repeat(np.arange(width), x[i].astype(np.int64)) for i in range(d)])
        names.append(name)
    return build_checkpoint(counters, c.a, c.b, seed=c.seed, frac_bits=c.frac_bits, owner_ids=c.owner_ids, forms=names,
                            lists=lists, masses=c.masses, pairs_ingested=c.pairs_ingested)


if __name__ == "__main__":
    import sys
    c = read_checkpoint(sys.argv[1])
    print("checkpoint v%d: n=%d d=%d w=%d counters=%s frac_bits=%d pairs=%d seed=%d ids=%s" % (
        VERSION, c.num_owners, c.depth, c.width, "f64" if c.counter_type else "u32", c.frac_bits, c.pairs_ingested,
        c.seed, "yes" if c.owner_ids is not None else "no"))
    print("file %d bytes, payload %d bytes, rows by form: %s" % (c.file_bytes, c.payload_bytes, c.form_counts()))
