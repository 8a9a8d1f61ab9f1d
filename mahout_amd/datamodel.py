"""DataModel inputs of the sketch path.

GenericDataModel / FileDataModel reduced to what CosineCM reads: the sorted
owner-ID universe and each owner's preferences sorted by key, in the SoA
layout of GenericUserPreferenceArray (long[] ids, float[] values,
T/impl/model/GenericUserPreferenceArray.java:52-54) -- here one CSR
(offsets, keys, values) over all owners, which is exactly what
cms_ingest_csr consumes.
"""
import re

import numpy as np


class NoSuchUserException(KeyError):
    """org.apache.mahout.cf.taste.common.NoSuchUserException"""


class GenericDataModel:
    """T/impl/model/GenericDataModel.java:80-137: per-user preferences sorted
    by item (:91), item IDs sorted (:120), user IDs sorted (:134)."""

    def __init__(self, user_prefs):
        # user_prefs: {userID: {itemID: float}}
        self.user_ids = np.array(sorted(user_prefs), dtype=np.int64)
        items = set()
        offsets = [0]
        keys, vals = [], []
        for u in self.user_ids:
            prefs = user_prefs[int(u)]
            for it in sorted(prefs):
                keys.append(it)
                vals.append(np.float32(prefs[it]))
                items.add(it)
            offsets.append(len(keys))
        self.item_ids = np.array(sorted(items), dtype=np.int64)
        self.offsets = np.array(offsets, dtype=np.int64)
        self.keys = np.array(keys, dtype=np.int64)
        self.values = np.array(vals, dtype=np.float32)

    @classmethod
    def from_csr(cls, user_ids, offsets, keys, values):
        self = cls.__new__(cls)
        self.user_ids = np.ascontiguousarray(user_ids, np.int64)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.keys = np.ascontiguousarray(keys, np.int64)
        self.values = None if values is None else np.ascontiguousarray(values, np.float32)
        self.item_ids = np.unique(self.keys)
        return self

    def transposed(self):
        """The model with users and items swapped: its "users" are this
        model's items (ascending), each with the users that hold it as keys,
        ascending, and the same values -- the orientation an ItemSimilarity's
        CosineCM is built over (FileDataModel's transpose, :414-418).  A user
        without preferences has no place in it, so transposing twice drops
        such users."""
        users = np.repeat(self.user_ids, np.diff(self.offsets))
        order = np.lexsort((users, self.keys))  # by item, then by user
        items, counts = np.unique(self.keys, return_counts=True)
        off = np.zeros(items.size + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        return GenericDataModel.from_csr(items, off, users[order], None if self.values is None else self.values[order])

    def getUserIDs(self):
        return self.user_ids

    def getItemIDs(self):
        return self.item_ids

    def getNumUsers(self):
        return int(self.user_ids.size)

    def getNumItems(self):
        return int(self.item_ids.size)

    def hasPreferenceValues(self):
        return self.values is not None

    def getMinPreference(self):
        """Smallest preference value (GenericDataModel.java:87-116); +inf when
        empty; NaN without values (AbstractDataModel.java:31-34)."""
        if self.values is None:
            return float("nan")
        return float(self.values.min()) if self.values.size else float("inf")

    def getMaxPreference(self):
        if self.values is None:
            return float("nan")
        return float(self.values.max()) if self.values.size else float("-inf")

    def getPreferenceValue(self, user_id, item_id):
        """GenericDataModel.getPreferenceValue (:244-253): the value, or None."""
        keys, vals = self.getPreferencesFromUser(user_id)
        j = np.searchsorted(keys, item_id)
        if j < keys.size and keys[j] == item_id:
            return None if vals is None else float(vals[j])
        return None

    def getPreferencesFromUser(self, user_id):
        """(item IDs ascending, float values) -- GenericDataModel.java:210-216."""
        i = np.searchsorted(self.user_ids, user_id)
        if i >= self.user_ids.size or self.user_ids[i] != user_id:
            raise NoSuchUserException(user_id)
        lo, hi = self.offsets[i], self.offsets[i + 1]
        v = None if self.values is None else self.values[lo:hi]
        return self.keys[lo:hi], v


_JAVA_DEC = re.compile(r"[+-]?(?:NaN|Infinity|(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?[fFdD]?)")
_JAVA_HEX = re.compile(r"([+-]?)0[xX]([0-9a-fA-F]*)\.?([0-9a-fA-F]*)[pP]([+-]?\d+)[fFdD]?")
_LONG = re.compile(r"[+-]?\d+")


def _round_to_f32(q):
    """The float32 nearest the exact rational q (ties to even), as IEEE 754
    round-to-nearest does for Float.parseFloat (JLS: "rounded to type float
    by the usual round-to-nearest rule")."""
    from fractions import Fraction
    try:
        x = float(q)  # correctly rounded to double (int / int true division)
    except OverflowError:
        return np.float32(np.inf if q > 0 else -np.inf)
    with np.errstate(over="ignore", under="ignore"):
        f = np.float32(x)
    if float(f) == x:  # q is within half a double ulp of a float32: that one
        return f
    # decimal -> double -> float rounds twice; only a double that lands
    # exactly on a float32 midpoint can end on the wrong side: resolve it from q
    up = x > float(f) if np.isfinite(f) else x < 0
    if not np.isfinite(f):  # x beyond FLT_MAX: f is inf, its neighbour FLT_MAX
        g = np.float32(np.finfo(np.float32).max) * np.float32(1 if x > 0 else -1)
        f, g = g, f
        up = not up
    with np.errstate(over="ignore"):
        g = np.nextafter(f, np.float32(np.inf) if up else np.float32(-np.inf))
    gv = Fraction(float(g)) if np.isfinite(g) else Fraction(2 ** 128) * (1 if up else -1)
    mid = (Fraction(float(f)) + gv) / 2
    if Fraction(x) != mid:
        return np.float32(f) if abs(Fraction(x) - Fraction(float(f))) < abs(Fraction(x) - gv) else g
    if q == mid:  # an exact tie: the even significand (inf counts as even past FLT_MAX)
        return f if (int(np.float32(f).view(np.uint32)) & 1) == 0 else g
    return g if (q > mid) == up else f


_F32_CACHE = {}


def java_parse_float(s):
    """java.lang.Float.parseFloat: surrounding whitespace (chars <= ' ')
    trimmed, optional sign, NaN / Infinity, decimal or hexadecimal
    significand, optional f/F/d/D suffix; the exact value rounded once to
    float32.  Raises ValueError (NumberFormatException) otherwise."""
    r = _F32_CACHE.get(s)
    if r is not None:
        return r
    from fractions import Fraction
    t = s.strip("".join(chr(c) for c in range(33)))
    if _JAVA_DEC.fullmatch(t):
        body = t.rstrip("fFdD") if t[-1:] in "fFdD" and "Infinity" not in t else t
        neg = body.startswith("-")
        core = body.lstrip("+-")
        if core == "NaN":
            r = np.float32(np.nan)
        elif core == "Infinity":
            r = np.float32(-np.inf if neg else np.inf)
        else:
            q = Fraction(core)
            r = _round_to_f32(-q if neg else q)
            if neg and r == 0:
                r = np.float32(-0.0)
    else:
        m = _JAVA_HEX.fullmatch(t)
        if not m or not (m.group(2) or m.group(3)):
            raise ValueError(f"For input string: \"{s}\"")
        digits = (m.group(2) or "") + (m.group(3) or "")
        q = Fraction(int(digits, 16), 16 ** len(m.group(3) or "")) * Fraction(2) ** int(m.group(4))
        r = _round_to_f32(-q if m.group(1) == "-" else q)
        if m.group(1) == "-" and r == 0:
            r = np.float32(-0.0)
    if len(_F32_CACHE) < 65536:
        _F32_CACHE[s] = r
    return r


def java_parse_long(s):
    """java.lang.Long.parseLong (FileDataModel.readUserIDFromString /
    readItemIDFromString): decimal digits with an optional sign, no
    whitespace, within the long range; ValueError otherwise."""
    if not _LONG.fullmatch(s):
        raise ValueError(f"For input string: \"{s}\"")
    v = int(s)
    if not -2 ** 63 <= v < 2 ** 63:
        raise ValueError(f"For input string: \"{s}\"")
    return v


class FileDataModel(GenericDataModel):
    """T/impl/model/file/FileDataModel.java: one data file and, with
    update_files=True, the reference's update files (:92-101, :239-334) --
    files beside the data file whose names share its name up to the first
    period, not older than it, read after it in ascending modification time
    with the same line rules, so a later line deletes or replaces an earlier
    preference.  refresh() re-reads everything.  The default reads the data
    file alone:

    - the delimiter is ',' if the first data line (blank and '#' lines
      skipped) holds one, else tab (determineDelimiter, :344-352); every
      line is split on that single character, empty tokens kept (Guava
      Splitter.on, :201);
    - the file has preference values when that first line has a non-empty
      third token (:210-214); otherwise it is a boolean model
      (processLineWithoutID, :560-603; hasPreferenceValues() is false);
    - IDs are Long.parseLong, values Float.parseFloat (:411-412, :455);
    - transpose swaps user and item (:414-418);
    - a repeated (user, item) keeps the LAST value (:511-527);
    - `user,item,` (empty value, no timestamp) removes the preference
      (:493-508) -- the user stays in the model even with no preferences left
      (GenericDataModel.toDataMap keeps the emptied collection, :160-168).
    """

    def __init__(self, path, transpose=False, update_files=False):
        self._path = path
        self._transpose = transpose
        self._update_files = update_files
        self._load()

    def refresh(self, alreadyRefreshed=None):
        """Refreshable.refresh: re-read the data file (and, with
        update_files, every update file).  The model's arrays are replaced,
        never changed in place."""
        self._load()

    def _find_update_files(self):
        """findUpdateFilesAfter(dataFile.lastModified()) (:313-334): the plain
        files of the data file's directory whose names start with the data
        file's name up to its first period, other than the data file, not
        older than it -- in ascending modification time (a TreeMap keyed by
        it: of two files with one time the later listed replaces the other)."""
        import os
        name = os.path.basename(self._path)
        start = name.split(".", 1)[0]
        parent = os.path.dirname(os.path.abspath(self._path))
        t0 = os.stat(self._path).st_mtime_ns
        by_time = {}
        for fn in sorted(os.listdir(parent)):
            p = os.path.join(parent, fn)
            if os.path.isdir(p) or not fn.startswith(start) or fn == name:
                continue
            t = os.stat(p).st_mtime_ns
            if t >= t0:
                by_time[t] = p
        return [by_time[t] for t in sorted(by_time)]

    def _load(self):
        path, transpose = self._path, self._transpose
        with open(path) as f:
            lines = [ln.rstrip("\n").rstrip("\r") for ln in f]
        first = next((ln for ln in lines if ln and ln[0] != "#"), None)
        if first is None:
            raise ValueError("dataFile is empty")
        if "," in first:
            delim = ","
        elif "\t" in first:
            delim = "\t"
        else:
            raise ValueError("Did not find a delimiter in first line")
        ftok = first.split(delim)
        has_values = len(ftok) >= 3 and ftok[2] != ""
        if self._update_files:  # processed after the data file, with its delimiter and line rules (:260-262)
            for up in self._find_update_files():
                with open(up) as f:
                    lines.extend(ln.rstrip("\n").rstrip("\r") for ln in f)
        prefs = {}
        for line in lines:
            if not line or line[0] == "#":
                continue
            tok = line.split(delim)
            if len(tok) < 2 or (has_values and len(tok) < 3):
                raise ValueError(f"NoSuchElementException: too few fields in line {line!r}")
            u, it = java_parse_long(tok[0]), java_parse_long(tok[1])
            has_pref = len(tok) >= 3
            pref_s = tok[2] if has_pref else ""
            has_ts = len(tok) >= 4
            if transpose:
                u, it = it, u
            if (has_values or has_pref) and not has_ts and pref_s == "":
                if u in prefs:
                    prefs[u].pop(it, None)
                continue
            if has_values:
                prefs.setdefault(u, {})[it] = float(java_parse_float(pref_s))
            else:
                prefs.setdefault(u, {})[it] = 1.0
        super().__init__(prefs)
        if not has_values:
            self.values = None  # GenericBooleanPrefDataModel


def preference_delta(old, new):
    """What turns `old`'s sketches into `new`'s, for two models over the same
    user IDs: ((users, items, values) to retract, (users, items, values) to
    ingest) as COO arrays, users by ID.  Retracted are the removed
    preferences and the changed ones at their OLD values; ingested the added
    preferences and the changed ones at their NEW values (a boolean model's
    values count as 1.0).  ValueError when the user IDs differ."""
    if not np.array_equal(old.user_ids, new.user_ids):
        raise ValueError("preference_delta: the models differ in their user IDs")

    def coo(m):
        u = np.repeat(np.asarray(m.user_ids, np.int64), np.diff(m.offsets))
        v = np.ones(m.keys.size, np.float32) if m.values is None else np.asarray(m.values, np.float32)
        return u, np.asarray(m.keys, np.int64), v

    uo, ko, vo = coo(old)
    un, kn, vn = coo(new)
    u = np.concatenate([uo, un])
    k = np.concatenate([ko, kn])
    v = np.concatenate([vo, vn])
    src = np.concatenate([np.zeros(uo.size, np.int8), np.ones(un.size, np.int8)])
    order = np.lexsort((src, k, u))  # a preference of both models: old then new, adjacent
    u, k, v, src = u[order], k[order], v[order], src[order]
    both = (u[:-1] == u[1:]) & (k[:-1] == k[1:]) & (src[:-1] == 0) & (src[1:] == 1)
    same = both & (v[:-1] == v[1:])
    keep_old = np.ones(u.size, bool)  # the old side of an unchanged preference leaves, and its new side
    keep_new = np.ones(u.size, bool)
    keep_old[:-1] &= ~same
    keep_new[1:] &= ~same
    r = (src == 0) & keep_old
    a = (src == 1) & keep_new
    return (u[r], k[r], v[r]), (u[a], k[a], v[a])
