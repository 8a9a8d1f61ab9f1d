"""read_checkpoint: a pure-numpy reader of the checkpoint image (format
version 1, DESIGN.md 3 "Checkpoint image") -- no GPU and no library.

The format's independent second implementation (the tests decode what the GPU
wrote with it) and an inspection tool:

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

    def form_counts(self):
        return {ROW_FORMS[f]: int(c) for f, c in enumerate(np.bincount(self.forms, minlength=len(ROW_FORMS))) if c}


def read_checkpoint(path):
    """Decode a checkpoint file (ValueError when it is not a valid image)."""
    with open(path, "rb") as f:
        return Checkpoint(f.read())


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


if __name__ == "__main__":
    import sys
    c = read_checkpoint(sys.argv[1])
    print("checkpoint v%d: n=%d d=%d w=%d counters=%s frac_bits=%d pairs=%d seed=%d ids=%s" % (
        VERSION, c.num_owners, c.depth, c.width, "f64" if c.counter_type else "u32", c.frac_bits, c.pairs_ingested,
        c.seed, "yes" if c.owner_ids is not None else "no"))
    print("file %d bytes, payload %d bytes, rows by form: %s" % (c.file_bytes, c.payload_bytes, c.form_counts()))
