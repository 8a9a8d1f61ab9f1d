"""CPU: mahout_amd.checkpoint.diff_counters, the no-GPU specification of
SketchTable.subtract, on tables written by build_checkpoint."""
import numpy as np
import pytest

from mahout_amd import checkpoint as ck

N, D, W = 12, 3, 128
HA = np.arange(1, D + 1, dtype=np.int64) * 1000003
HB = np.arange(1, D + 1, dtype=np.int64) * 7919


def _table(seed, hot_row=None):
    """[N][D][W] counters: rows of every magnitude (0/1, < 4, < 16, < 256, u16, one u32 row), the last row zero."""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.zeros((N, D, W), np.uint64)
    tops = [2, 2, 4, 4, 16, 16, 256, 256, 60000, 3, 1 << 20]
    for r, top in enumerate(tops):
        c[r] = rng.integers(0, top, (D, W)) * (rng.random((D, W)) < 0.3)
    return c


def _image(c, **kw):
    return ck.Checkpoint(ck.build_checkpoint(c, HA, HB, **kw))


def test_the_sum_minus_one_summand_is_the_other():
    ca, cb = _table(1), _table(2)
    a, b = _image(ca), _image(cb)
    both = ck.sum_counters([a, b])
    s = _image(both.astype(np.uint64), masses=a.masses + b.masses)
    got, mass = ck.diff_counters(s, b)
    assert np.array_equal(got, a.counters()) and np.array_equal(got, ca.astype(np.float64))
    assert mass.dtype == np.uint64 and np.array_equal(mass, a.masses)
    got, mass = ck.diff_counters(s, a)
    assert np.array_equal(got, cb.astype(np.float64)) and np.array_equal(mass, b.masses)
    zero, mass = ck.diff_counters(a, a)
    assert not zero.any() and not mass.any()


def test_paths_and_list_rows(tmp_path):
    ca, cb = _table(3), _table(4)
    ent = np.array([[5, 5, 9], [0, 127, 127], [64, 64, 64]])  # [d][m], repeats allowed
    cb[9] = np.stack([np.bincount(e, minlength=W) for e in ent])
    pa, pb = str(tmp_path / "s.ckpt"), str(tmp_path / "b.ckpt")
    ck.write_checkpoint(pb, cb, HA, HB, lists={9: ent})
    ck.write_checkpoint(pa, ca + cb, HA, HB)
    got, mass = ck.diff_counters(pa, pb)
    assert np.array_equal(got, ca.astype(np.float64))
    assert np.array_equal(mass, ck.read_checkpoint(pa).masses - ck.read_checkpoint(pb).masses)


def test_frac_bits_scale_the_difference():
    ca, cb = _table(5), _table(6)
    got, _ = ck.diff_counters(_image(ca + cb, frac_bits=2), _image(cb, frac_bits=2))
    assert np.array_equal(got, ca / 4.0)


def _refused(a, b):
    with pytest.raises(ValueError):
        ck.diff_counters(a, b)


def test_mismatching_shapes_are_refused():
    ca = _table(7)
    a = _image(ca)
    _refused(a, _image(ca[:N - 1]))                      # num_owners
    _refused(a, _image(ca[:, :D - 1], ))                 # depth
    _refused(a, _image(ca[:, :, :W // 2]))               # width
    _refused(a, _image(ca, frac_bits=1))                 # frac_bits


def test_other_hash_parameters_are_refused():
    ca = _table(8)
    hb2 = HB.copy()
    hb2[D - 1] += 1
    _refused(_image(ca), ck.Checkpoint(ck.build_checkpoint(ca, HA, hb2)))
    ha2 = HA.copy()
    ha2[0] += 1
    _refused(_image(ca), ck.Checkpoint(ck.build_checkpoint(ca, ha2, HB)))


def test_differing_owner_ids_are_refused():
    ca = _table(9)
    ids = np.arange(N, dtype=np.int64) * 3 + 7
    other = ids.copy()
    other[N // 2] += 1
    _refused(_image(ca, owner_ids=ids), _image(ca))
    _refused(_image(ca), _image(ca, owner_ids=ids))
    _refused(_image(ca, owner_ids=ids), _image(ca, owner_ids=other))
    got, _ = ck.diff_counters(_image(ca, owner_ids=ids), _image(ca, owner_ids=ids))
    assert not got.any()


def test_a_mass_underflow_is_refused():
    ca = _table(10)
    a = _image(ca)
    m = a.masses.copy()
    m[4] += 1
    _refused(a, _image(ca, masses=m))


def test_a_counter_underflow_the_masses_do_not_show_is_refused():
    """The same owner with equal mass over different keys."""
    ca = np.zeros((N, D, W), np.uint64)
    cb = ca.copy()
    ca[3, :, 10] = 5
    cb[3, :, 11] = 5
    a, b = _image(ca), _image(cb)
    assert np.array_equal(a.masses, b.masses)
    _refused(a, b)
    cb[3, :, 11] = 0
    cb[3, :, 10] = 5
    cb[3, 1, 10] = 6  # one counter one too high, the mass (the largest row sum) declared equal
    _refused(a, _image(cb, masses=a.masses))


def test_fp64_images_are_refused():
    c = np.zeros((N, D, W), np.float64)
    c[0, 0, 0] = 1.5
    f = _image(c)
    _refused(f, f)
    _refused(f, _image(_table(11)))
    _refused(_image(_table(11)), f)
