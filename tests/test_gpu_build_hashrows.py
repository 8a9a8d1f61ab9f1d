"""GPU: the branch-free row hash (RowHash, cms_hash.h) in the split owners'
slice build (k_build_slices<D>) and the streamed mid owners' one-pass build
(k_build_mid<2, D, 512>), D = 4 and 5 at power-of-two widths.

Both kernels hash a key's D rows at once and take ONE redo per key, for a key
with a row in the fp64 quotient's margin, a key that is no u32 below 2^32 - 2
and, behind the COO partition, an escaped token.  The owners here are sized at
the kernels' loop edges (the slice loop steps 8 x 512 keys, the streamed one
2 x 512) and carry the keys the host build of the same helper redoes
(tests/test_hash_rows_host.py), placed so that every key slot of a step and the
last, partial step meet one; one split and one streamed owner also hold keys
in [2^31, 2^32), at and above 2^32 and negative ones.

Counters are compared bit for bit with the oracle through read_counters();
norms and maxima through similarities() against the oracle's rows and against a
CMS_NO_FORMS=1 handle built from the same pairs.  CMS_SPLIT_KEYS = 5001 keeps a
split owner cheap; every case stays under 200K pairs but the COO one (286720:
the smallest COO batches that take the row build have 262144).
"""
import os

import numpy as np
import pytest

from mahout_amd import SketchTable
from test_hash_rows_host import load_shim, redo_keys

pytestmark = pytest.mark.gpu

SPLIT = 5001    # CMS_SPLIT_KEYS: more keys make a split owner
T = 512         # threads of either kernel
SLICE = 65535   # keys of a slice


def _same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _handle(n, d, w, env=None):
    """A handle created under the given tunables (read once, at creation)."""
    env = dict(env or {})
    env.setdefault("CMS_SPLIT_KEYS", str(SPLIT))
    names = ("CMS_NO_FORMS", "CMS_NO_COMPACT", "CMS_MID_U8_KEYS", "CMS_MID_U4_KEYS", "CMS_SPLIT_KEYS")
    saved = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(env)
    try:
        return SketchTable(n, depth=d, width=w, seed=42)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _pairs(owners):
    rows = np.concatenate([np.full(k.size, i, np.int64) for i, k in enumerate(owners)])
    return rows, np.concatenate(owners).astype(np.int64)


def _csr(owners):
    off = np.zeros(len(owners) + 1, np.int64)
    off[1:] = np.cumsum([k.size for k in owners])
    return off, np.concatenate(owners).astype(np.int64)


def _positions(m, per):
    """Where an owner of m keys gets its planted keys: 64 spread evenly, one in
    every key slot of the first step, the first and the last key of the last
    step (index m - 1: the lone key of a second slice, or of a step of one)."""
    step = per * T
    pos = set(int(x) for x in np.linspace(0, m - 1, 64).astype(np.int64))
    pos |= {u * T + 5 for u in range(per) if u * T + 5 < m}
    last = ((m - 1) // step) * step
    pos |= {last, m - 1}
    pos = np.array(sorted(pos), np.int64)
    slots = set(((pos % step) // T).tolist())
    assert slots == set(range(min(per, (m + T - 1) // T))), (m, slots)
    assert np.any(pos >= last)
    return pos


def _owner(rng, m, per, planted, wide=False):
    """m keys below 2^22, the planted (redo) keys at _positions; wide: a
    quarter each of keys in [2^31, 2^32), from 2^32 up and negative ones."""
    keys = rng.permutation(1 << 22)[:m].astype(np.int64)
    if wide:
        q = m // 4
        idx = rng.permutation(m)
        keys[idx[:q]] = (1 << 31) + rng.permutation(1 << 20)[:q]
        keys[idx[q:2 * q]] = (1 << 32) + rng.permutation(1 << 20)[:q]
        keys[idx[2 * q:3 * q]] = -1 - rng.permutation(1 << 20)[:q]
        keys[idx[3 * q:3 * q + 6]] = [1 << 31, (1 << 32) - 1, (1 << 32) - 2, (1 << 32) - 3, 1 << 32, (1 << 62) + 5]
    if planted is not None:
        pos = _positions(m, per)
        assert pos.size >= 64
        keys[pos] = rng.choice(planted, pos.size, replace=False)
    return keys


def _owners(rng, planted):
    """(owners, number of split owners).  Split: SPLIT + 1, 4096 k +- 1 keys,
    65536 keys (two slices, the second of one key) and one with wide keys;
    streamed: 1025, 1024 k + 1, 5001 keys and one with wide keys."""
    split = [SPLIT + 1, 2 * 4096 + 1, 2 * 4096 - 1, SLICE + 1]
    streamed = [1025, 2 * 1024 + 1, SPLIT]
    owners = [_owner(rng, m, 8, planted) for m in split] + [_owner(rng, 6000, 8, planted, wide=True)]
    owners += [_owner(rng, m, 2, planted) for m in streamed] + [_owner(rng, 3000, 2, planted, wide=True)]
    return owners, len(split) + 1


def _check(oracle, t, plain, owners, exp, queries=None):
    n = len(owners)
    assert np.array_equal(t.read_counters(), exp)
    ids = np.arange(n)
    for q in (range(n) if queries is None else queries):
        s = t.similarities(q, ids)
        if plain is not None:
            assert _same(s, plain.similarities(q, ids)), q
        ref = oracle.similarities_row(exp, q)
        ref[q] = oracle.cosine_cm(exp[q], exp[q])
        assert _same(s, ref), q


@pytest.fixture(scope="module")
def shim():
    return load_shim()


@pytest.mark.parametrize("d,w", [(5, 8192), (4, 1024)])
def test_hash_rows_csr(oracle, shim, d, w):
    a, b = oracle.hash_params(42, d)
    planted = redo_keys(shim, a, b, w)
    assert planted.size >= 100
    rng = np.random.Generator(np.random.PCG64(d * 1009 + w))
    owners, nsplit = _owners(rng, planted)
    n = len(owners)
    off, keys = _csr(owners)
    assert keys.size < 200_000
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    with _handle(n, d, w) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            x.ingest_csr(off, keys)
            x.finalize()
        assert t.stats()["hot_rows"] == nsplit, t.stats()
        _check(oracle, t, plain, owners, exp)


def test_hash_rows_tokens(oracle, shim):
    """Behind the COO partition: a key in [0, 2^31) is its own u32 token, any
    other travels as an index into the batch's keys and is resolved in the
    redo, in the slice kernel and in the streamed one."""
    d, w = 5, 8192
    a, b = oracle.hash_params(42, d)
    planted = redo_keys(shim, a, b, w)
    rng = np.random.Generator(np.random.PCG64(31))
    owners = [_owner(rng, 2 * 4096 + 1, 8, planted, wide=True)]
    owners += [_owner(rng, m, 2, planted, wide=True) for m in (1025, 2 * 1024 + 1, SPLIT)]
    rest = 286_720 - sum(k.size for k in owners)
    owners += [_owner(rng, 5000, 2, planted) for _ in range(rest // 5000)]
    owners += [_owner(rng, rest % 5000, 2, None)]
    n = len(owners)
    rows, keys = _pairs(owners)
    assert keys.size == 286_720
    order = rng.permutation(rows.size)
    exp = oracle.build_table(n, d, w, a, b, rows[order], keys[order])
    with _handle(n, d, w) as t:
        t.ingest(rows[order], keys[order])
        t.finalize()
        assert t.stats()["hot_rows"] == 1, t.stats()
        _check(oracle, t, None, owners, exp, queries=(0, 1, 2, 3, n - 1))


@pytest.mark.parametrize("d,w", [(3, 96), (8, 16384)])
def test_generic_shapes_untouched(oracle, d, w):
    """A depth the kernels do not unroll, at a width that is no power of two
    and at one whose images exceed the LDS: the same owners (no planted keys:
    the helper has no say here) through each_bucket."""
    a, b = oracle.hash_params(42, d)
    rng = np.random.Generator(np.random.PCG64(d * 1009 + w))
    owners, nsplit = _owners(rng, None)
    n = len(owners)
    off, keys = _csr(owners)
    exp = oracle.build_table(n, d, w, a, b, *_pairs(owners))
    with _handle(n, d, w) as t, _handle(n, d, w, {"CMS_NO_FORMS": "1"}) as plain:
        for x in (t, plain):
            x.ingest_csr(off, keys)
            x.finalize()
        assert t.stats()["hot_rows"] == nsplit, t.stats()
        _check(oracle, t, plain, owners, exp)
