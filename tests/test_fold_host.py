"""CPU: checkpoint.fold_checkpoint, the no-GPU specification of the fold
 -- no device call anywhere here.

The identity itself is checked against the oracle: the image of the table a
stream builds at width w, folded to a divisor w', decodes to the table the same
stream builds at w' with the same hash parameters, counter for counter, for
power-of-two widths and others alike.  Then the forms (compact_form at the new
shape), the identity fold (= compact_checkpoint) and every refusal.
"""
import numpy as np
import pytest

from mahout_amd import checkpoint as ck

N, KEYS, PAIRS = 64, 5000, 6000
CASES = [(4, 1024, (512, 256, 32, 16, 1)), (3, 96, (48, 32, 24, 3))]


def _stream(d, w):
    """A seeded stream: most owners a handful of keys, a few repeated pairs,
    one owner with weights that pass 2^16."""
    rng = np.random.Generator(np.random.PCG64(100 * d + w))
    rows = np.minimum(rng.zipf(1.3, PAIRS) - 1, N - 5).astype(np.int64)  # (the last four owners have no keys)
    keys = rng.integers(0, KEYS, PAIRS).astype(np.int64)
    vals = np.ones(PAIRS, np.float32)
    vals[rows == 5] = 40.0
    rows = np.concatenate([rows, np.full(4, 7)])
    keys = np.concatenate([keys, np.array([11, 11, 12, 13])])
    vals = np.concatenate([vals, np.array([40000, 40000, 3, 1], np.float32)])
    return rows, keys, vals


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "d%d-w%d" % c[:2])
def built(request, oracle):
    d, w, divisors = request.param
    a, b = oracle.hash_params(42, d)
    rows, keys, vals = _stream(d, w)
    table = oracle.build_table(N, d, w, a, b, rows, keys, vals)
    ids = np.arange(N, dtype=np.int64) * 3 + 100
    image = ck.build_checkpoint(table.astype(np.uint64), a, b, seed=42, owner_ids=ids, pairs_ingested=rows.size)
    narrow = {wf: oracle.build_table(N, d, wf, a, b, rows, keys, vals) for wf in divisors}
    return d, w, divisors, image, narrow


def test_the_folded_image_is_the_narrow_table(built):
    d, w, divisors, image, narrow = built
    src = ck.Checkpoint(image)
    for wf in divisors:
        got = ck.Checkpoint(ck.fold_checkpoint(image, wf))
        assert (got.depth, got.width, got.num_owners) == (d, wf, N)
        assert np.array_equal(got.counters(), narrow[wf]), wf
        assert np.array_equal(got.masses, src.masses) and np.array_equal(got.owner_ids, src.owner_ids)
        assert np.array_equal(got.a, src.a) and np.array_equal(got.b, src.b)
        assert (got.seed, got.frac_bits, got.pairs_ingested, got.counter_type) == (src.seed, src.frac_bits,
                                                                                   src.pairs_ingested, 0)


def test_every_row_is_in_its_compact_form(built):
    d, w, divisors, image, narrow = built
    seen = set()
    for wf in divisors:
        got = ck.Checkpoint(ck.fold_checkpoint(image, wf))
        for r in range(N):
            x = narrow[wf][r].astype(np.uint64)
            want = ck.compact_form(int(x.max()), int(got.masses[r]), x.sum(axis=1), d, wf)
            assert ck.ROW_FORMS[got.forms[r]] == want, (wf, r)
            seen.add(want)
        named = np.array([ck.ROW_FORMS[f] for f in got.forms])
        assert np.all(got.bounds[named == "u32"] == 0)
        rest = named != "u32"
        assert np.array_equal(got.bounds[rest], narrow[wf].max(axis=(1, 2)).astype(np.uint32)[rest])
    assert {"zero", "list", "u16", "u32"} <= seen, seen
    # under CMS_NO_FORMS the image holds zero / u16 / u32 rows only
    got = ck.Checkpoint(ck.fold_checkpoint(image, divisors[0], forms=False))
    assert {ck.ROW_FORMS[f] for f in got.forms} <= {"zero", "u16", "u32"}
    assert np.array_equal(got.counters(), narrow[divisors[0]])
    got = ck.Checkpoint(ck.fold_checkpoint(image, divisors[0], list_keys=0))
    assert "list" not in {ck.ROW_FORMS[f] for f in got.forms}


def test_folding_to_the_own_width_is_the_compaction(built):
    d, w, divisors, image, narrow = built
    assert ck.fold_checkpoint(image, w) == ck.compact_checkpoint(image)
    assert ck.fold_checkpoint(image, w, list_keys=16, forms=False) == ck.compact_checkpoint(image, list_keys=16, forms=False)
    # a fold of a fold is the fold: w -> w1 -> w2 = w -> w2
    w1, w2 = (256, 32) if w == 1024 else (48, 24)
    assert ck.fold_checkpoint(ck.fold_checkpoint(image, w1), w2) == ck.fold_checkpoint(image, w2)


def test_refusals(built, oracle):
    d, w, divisors, image, narrow = built
    for bad in (0, -1, w + 1, 2 * w, 5, w - 1):
        with pytest.raises(ValueError):
            ck.fold_checkpoint(image, bad)
    a, b = oracle.hash_params(42, d)
    f64 = ck.build_checkpoint(np.ones((2, d, w), np.float64), a, b)
    with pytest.raises(ValueError, match="fp64"):
        ck.fold_checkpoint(f64, w // 2)


def overflowing_image(oracle, d=2, w=64):
    """Two counters of 2^31 in one residue class of w / 2 (explicit masses: no
    stream builds it, a loaded image can hold it)."""
    a, b = oracle.hash_params(42, d)
    c = np.zeros((3, d, w), np.uint64)
    c[1, 1, 3] = c[1, 1, 3 + w // 2] = 1 << 31
    c[2, 0, 5] = 7
    return ck.build_checkpoint(c, a, b, seed=42, masses=np.array([0, (1 << 32) - 1, 7], np.uint64))


def test_a_folded_counter_of_2_32_is_refused(oracle):
    image = overflowing_image(oracle)
    with pytest.raises(ValueError, match="2\\^32"):
        ck.fold_checkpoint(image, 32)
    with pytest.raises(ValueError, match="2\\^32"):
        ck.fold_checkpoint(image, 1)
    assert ck.fold_checkpoint(image, 64) == ck.compact_checkpoint(image)  # nothing folds: nothing overflows
