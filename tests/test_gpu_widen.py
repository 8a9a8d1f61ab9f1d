"""GPU: widen_rows (cms_table.hip k_widen_mark / k_widen_rows, the decisions of
cms_forms.h) form by form, in the compact layout, every comparison over the
WHOLE table against the oracle's rebuild
(`T/impl/common/DoubleCountMinSketch.java:72-80`).

  * first-touch rows among real movers: owners on the shared zero row that a
    batch touches for the first time (bound 1: they become 1-bit rows in u8
    places) side by side with 4-bit rows in u8 places that the same batch
    lifts past 255 (they move to whole u16 slots) -- through every route onto
    the zero row: a fresh handle, reset(), owners a row build left without
    keys, and a merged table (a one-rank transport communicator takes the
    packed merge and still accepts COO ingest);
  * the same batch through the owner-grouped path (k_ingest_sorted);
  * the transition matrix: owners landed in every form (by first-touch weight
    and by a Zipf row build), then one small batch that lifts a few of each
    source form to each wider target and leaves a few below their capacity;
    the forms afterwards equal the rule restated here in Python.

tests/test_forms_host.py enumerates the same decisions on the CPU.
"""
import numpy as np
import pytest

from mahout_amd import SketchTable
from mahout_amd.synth import zipf_stream

pytestmark = pytest.mark.gpu

FORMS = SketchTable.FORMS  # ("u32", "u16", "u8", "u4", "u2", "u1", "list")
BITS = {"list": 0, "u1": 1, "u2": 2, "u4": 4, "u8": 8, "u16": 16}
NAME = {b: f for f, b in BITS.items()}
CAP = {0: 0, 1: 1, 2: 3, 4: 15, 8: 255, 16: 65535}
N_KEYS = 20000


@pytest.fixture(autouse=True)
def _compact(monkeypatch):
    monkeypatch.setenv("CMS_NO_COMPACT", "0")


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


class Stream:
    """What went into a table, for the oracle's rebuild."""

    def __init__(self):
        self.r, self.k, self.v = [], [], []

    def add(self, t, rows, keys, vals=None):
        rows = np.asarray(rows, np.int64)
        keys = np.asarray(keys, np.int64)
        vals = np.ones(rows.size, np.float32) if vals is None else np.asarray(vals, np.float32)
        t.ingest(rows, keys, vals)
        self.r.append(rows), self.k.append(keys), self.v.append(vals)

    def table(self, oracle, n, d, w, seed=42):
        a, b = oracle.hash_params(seed, d)
        return oracle.build_table(n, d, w, a, b, np.concatenate(self.r), np.concatenate(self.k),
                                  np.concatenate(self.v))


def _check_table(t, oracle, exp, queries):
    got = t.read_counters()
    bad = np.flatnonzero((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, ("owners whose counters differ from the oracle", bad[:20], bad.size)
    n = exp.shape[0]
    for q in queries:
        ref = oracle.similarities_row(exp, int(q))
        ref[q] = oracle.cosine_cm(exp[q], exp[q])
        assert _same(t.similarities(int(q), np.arange(n)), ref), q


# ---- a / c: first-touch rows among real movers ----

N_A, D_A, W_A = 4096, 4, 1024


def _first_touch(t, oracle, s, fresh, grouped=False):
    """Batch 1: every even owner one pair of weight 10 (4-bit rows in u8
    places).  Batch 2: weight 300 on the same key (bound 310: a whole u16
    slot) and one unit pair for every odd owner (first touch, bound 1: a
    1-bit row in a u8 place).  fresh: the owners that were on the zero row
    before batch 1.  grouped: batch 2 is padded past 32768 pairs with unit
    pairs on eight owners batch 1 made hot, and goes into a finalized table."""
    n = N_A
    hot = np.arange(n - 8, n) if grouped else np.zeros(0, np.int64)
    ev = np.setdiff1d(np.arange(0, n, 2), hot)
    od = np.setdiff1d(np.arange(1, n, 2), hot)
    k_ev, k_od = (ev * 31 + 5) % N_KEYS, (od * 17 + 3) % N_KEYS
    s.add(t, np.concatenate([ev, hot]), np.concatenate([k_ev, hot]),
          np.concatenate([np.full(ev.size, 10), np.full(hot.size, 70000)]))
    if grouped:
        t.finalize()  # a live table with current norms
    rng = np.random.Generator(np.random.PCG64(12))
    pad = 32768 if grouped else 0
    rows = np.concatenate([ev, od, rng.choice(hot, pad) if pad else hot])
    keys = np.concatenate([k_ev, k_od, rng.integers(0, N_KEYS, pad)])
    vals = np.concatenate([np.full(ev.size, 300), np.ones(od.size + pad)])
    assert (rows.size >= 32768) == grouped
    s.add(t, rows, keys, vals)
    t.finalize()
    _check_table(t, oracle, s.table(oracle, n, D_A, W_A), (0, 1, n // 2 + 1, n - 1))
    form, bound = t.owner_forms()
    fo, fe = np.intersect1d(od, fresh), np.intersect1d(ev, fresh)
    assert fo.size > 1000 and fe.size > 1000
    assert np.all(form[fo] == FORMS.index("u1")) and np.all(bound[fo] == 1), np.unique(form[fo])
    assert np.all(form[fe] == FORMS.index("u16")), np.unique(form[fe])
    assert np.all(form[hot] == FORMS.index("u32"))


def _one_rank_transport(t):
    """A communicator of one rank: the sum over ranks leaves the words as they
    are, the gather copies the rank's bytes (staged through the host)."""
    from mahout_amd import transport
    calls = {"allreduce": 0, "allgather": 0}

    def allreduce(ptr, count):
        calls["allreduce"] += 1

    def allgather(send, recv, nbytes):
        calls["allgather"] += 1
        host = np.empty(nbytes, np.uint8)
        transport._d2h(host, send, nbytes)
        transport._h2d(recv, host, nbytes)
    t.comm_init_transport(0, 1, allreduce, allgather)
    return calls


@pytest.mark.parametrize("route", ["fresh", "reset", "build", "merged"])
def test_first_touch_rows_among_real_movers(oracle, route):
    n, d, w = N_A, D_A, W_A
    items, users = zipf_stream(N_KEYS, n // 2, 300_000, seed=41)  # a row build over the lower half of the owners
    with SketchTable(n, depth=d, width=w, seed=42, collective_single_rank=route == "merged") as t:
        s = Stream()
        fresh = np.arange(n)
        calls = None
        if route == "reset":
            t.ingest(items, users)
            t.finalize()
            t.reset()
        elif route in ("build", "merged"):
            if route == "merged":
                calls = _one_rank_transport(t)
            s.add(t, items, users)
            t.finalize()  # merged: the packed merge lays the rows out anew; owners without keys stay on the zero row
            fresh = np.arange(n // 2, n)
            assert t.stats()["world"] == 1
        _first_touch(t, oracle, s, fresh)
        if calls is not None:  # the packed merge ran, and the batches went through the merged table's delta log
            assert calls["allreduce"] > 0 and calls["allgather"] > 0, calls


def test_first_touch_rows_grouped_path(oracle):
    """The same second batch with >= 32768 pairs into a live table with current
    norms: k_ingest_sorted, the other caller of widen_rows with bounds."""
    with SketchTable(N_A, depth=D_A, width=W_A, seed=42) as t:
        t.set_timing(True)
        _first_touch(t, oracle, Stream(), np.arange(N_A), grouped=True)
        assert t.timing("ingest_sorted")[1] == 1 and t.timing("ingest_atomic")[1] == 1  # batch 2, batch 1
        assert t.timing("widen_rows")[1] == 2


# ---- b: the transition matrix ----

def _target_bits(sb, nb, w):
    """cms_forms.h widen_target, restated: the narrowest form wider than the
    source's (sb bits; 0: a list row or the zero row) that holds nb; 2-bit
    rows need w % 64 == 0, 1-bit rows w % 128 == 0, any form w % 32 == 0."""
    if w % 32:
        return 16
    for tb, align in ((1, 128), (2, 64), (4, 1), (8, 1)):
        if sb < tb and nb <= CAP[tb] and w % align == 0:
            return tb
    return 16


def _expected_forms(form, bound, rowmax, mass, zero, delta, w):
    """Forms after one small batch adding delta[r] (mass) to owner r: a row
    whose mass reaches 2^16 is promoted to u32; a touched narrow row is
    rewritten when it sits on the zero row or its new bound -- its tracked
    largest counter (never above the accumulated bound) plus the batch's mass
    -- passes its form's capacity; a u16 row stays u16."""
    out = form.copy()
    for r in np.flatnonzero(delta > 0):
        f = FORMS[form[r]]
        if f == "u32" or mass[r] + delta[r] >= 65536:
            out[r] = FORMS.index("u32")
        elif f == "u16" and not zero[r]:
            pass
        else:
            sb = 0 if zero[r] else BITS[f]
            nb = min(int(bound[r]), int(rowmax[r])) + int(delta[r])
            if zero[r] or nb > CAP[sb]:
                out[r] = FORMS.index(NAME[_target_bits(sb, nb, w)])
    return out


@pytest.mark.parametrize("d,w", [(4, 96), (4, 192), (3, 1000), (4, 1024), (5, 1024), (9, 1024), (32, 16)])
def test_transition_matrix(oracle, d, w):
    n, built = 1536, 1024
    rng = np.random.Generator(np.random.PCG64(d * w))
    items, users = zipf_stream(N_KEYS, built, 300_000, seed=d + w)  # the row build: owners 0..1023
    with SketchTable(n, depth=d, width=w, seed=42) as t:
        s = Stream()
        s.add(t, items, users)
        t.finalize()
        mass = np.bincount(items, minlength=n).astype(np.int64)
        zero = mass == 0  # owners without keys: on the zero row
        # first-touch weights: 1-bit, 2-bit, 4-bit rows in u8 places, u8 and u16 rows in whole slots, one hot owner
        fresh = np.arange(built, n)
        wts = np.array([1, 2, 10, 200, 1000])[np.arange(fresh.size) % 5]
        wts[-1] = 70000
        form, bound = t.owner_forms()
        exp = s.table(oracle, n, d, w)
        delta = np.zeros(n, np.int64)
        delta[fresh] = wts
        want = _expected_forms(form, bound, exp.max(axis=(1, 2)), mass, zero, delta, w)
        s.add(t, fresh, fresh % N_KEYS, wts)
        t.finalize()
        form, bound = t.owner_forms()
        assert np.array_equal(form, want), [(r, FORMS[form[r]], FORMS[want[r]]) for r in np.flatnonzero(form != want)[:10]]
        if w % 128 == 0:
            assert {FORMS[f] for f in form[fresh]} == {"u1", "u2", "u4", "u8", "u16", "u32"}
        mass = mass + delta
        zero = mass == 0
        assert not zero[fresh].any()
        exp = s.table(oracle, n, d, w)
        _check_table(t, oracle, exp, ())
        # the lifting batch: from every source form a few owners to each
        # strictly wider target (one pair whose weight puts the new bound just
        # past the next narrower form), a few left within their capacity
        rowmax = exp.max(axis=(1, 2)).astype(np.int64)
        cur = np.minimum(bound.astype(np.int64), rowmax)
        delta = np.zeros(n, np.int64)
        planned = set()
        for src in ("list", "u1", "u2", "u4", "u8", "u16"):
            own = [r for r in np.flatnonzero((form == FORMS.index(src)) & ~zero) if mass[r] < 30000]
            rng.shuffle(own)
            sb = BITS[src]
            targets = [tb for tb in (1, 2, 4, 8, 16) if tb > sb] + ["keep", "u32"]
            for tgt in targets:
                took = 0
                for r in own:
                    if delta[r] or took == 3:
                        continue
                    if tgt == "keep":
                        wt = 1 if cur[r] + 1 <= CAP[sb] else 0
                    elif tgt == "u32":
                        wt = 65536 - mass[r]
                    else:
                        below = max(CAP[sb], max(CAP[b] for b in (0, 1, 2, 4, 8) if b < tgt), cur[r])
                        wt = below + 1 - cur[r] if below + 1 <= CAP[tgt] else 0
                    if wt > 0:
                        delta[r] = wt
                        took += 1
                        planned.add((src, tgt))
        rows = np.flatnonzero(delta)
        assert rows.size >= 6  # (without forms: three u16 rows kept, three promoted)
        want = _expected_forms(form, bound, rowmax, mass, zero, delta, w)
        s.add(t, rows, (rows * 7 + 1) % N_KEYS, delta[rows])
        t.finalize()
        got, _ = t.owner_forms()
        assert np.array_equal(got, want), [(r, FORMS[form[r]], FORMS[got[r]], FORMS[want[r]])
                                           for r in np.flatnonzero(got != want)[:10]]
        moved = {(FORMS[form[r]], FORMS[got[r]]) for r in rows}
        if w % 128 == 0:  # every dense source reached every wider form, and some kept theirs
            for a, src in enumerate(("u1", "u2", "u4", "u8", "u16")):
                for tgt in ("u2", "u4", "u8", "u16", "u32")[a:]:
                    assert (src, tgt) in moved, (src, tgt, sorted(moved), sorted(planned, key=str))
                # (a 1-bit row cannot keep its form: any added mass lifts its bound to 2)
                assert src == "u1" or (src, src) in moved, (src, sorted(moved))
        if w % 32:
            assert set(got[rows]) <= {FORMS.index("u16"), FORMS.index("u32")}
        _check_table(t, oracle, s.table(oracle, n, d, w), list(rows[:6]) + [0, n - 1])
