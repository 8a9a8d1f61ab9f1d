"""CPU: the host side of the threshold neighbourhoods -- cms_fastidset_to_array
(the library's FastIDSet, `T/impl/common/FastIDSet.java:125-166`) against
taste.FastIDSet, the two prototypes in the binding, and the constructor checks
of taste.ThresholdUserNeighborhood
(`T/impl/neighborhood/ThresholdUserNeighborhood.java:68-75`).  No device call."""
import numpy as np
import pytest

from mahout_amd import _lib, taste
from mahout_amd.sketch import fastidset_to_array


@pytest.fixture(scope="module", autouse=True)
def lib():
    from mahout_amd import build_lib
    build_lib.build()
    return _lib.load()


def _expected(ids):
    s = taste.FastIDSet()
    for i in np.asarray(ids, np.int64).tolist():
        s.add(i)
    return s.toList()


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 100, 5000])  # 3: the first rehash of a size-2 set
@pytest.mark.parametrize("kind", ["ascending", "random", "negative"])
def test_fastidset_to_array_matches_taste(n, kind):
    rng = _rng(1000 + n)
    if kind == "ascending":
        ids = np.cumsum(rng.integers(1, 9, n)).astype(np.int64)
    elif kind == "random":
        ids = rng.permutation(np.unique(rng.integers(0, 2 ** 40, 2 * n + 1)))[:n].astype(np.int64)
    else:
        ids = -rng.permutation(np.unique(rng.integers(1, 2 ** 40, 2 * n + 1)))[:n].astype(np.int64)
    assert ids.size == n and np.unique(ids).size == n
    got = fastidset_to_array(ids)
    assert got.tolist() == _expected(ids)
    assert sorted(got.tolist()) == sorted(ids.tolist())


def test_fastidset_every_size_across_the_first_rehash():
    """A new FastIDSet() holds nextTwinPrime(3) = 5 slots and grows at the add
    that finds numSlotsUsed * 1.5f >= 5: every prefix length up to and past
    that add follows the model's order."""
    seq = (7, 12, 3, 9, 20, 15)
    s = taste.FastIDSet()
    sizes = []
    for i in seq:
        s.add(i)
        sizes.append(len(s.keys))
    assert sizes[0] == 5 and sizes[-1] > 5  # the rehash happens inside this range
    for m in range(len(seq) + 1):
        ids = np.array(seq[:m], np.int64)
        assert fastidset_to_array(ids).tolist() == _expected(ids)


def test_fastidset_repeated_id_is_added_once():
    ids = np.array([5, 9, 5, 5, 1 << 33, 9, -4], np.int64)
    got = fastidset_to_array(ids)
    assert got.size == 4 and got.tolist() == _expected(ids)


@pytest.mark.parametrize("sentinel", [-2 ** 63, 2 ** 63 - 1])
def test_fastidset_refuses_the_sentinels(sentinel):
    with pytest.raises(_lib.CmsError) as ei:
        fastidset_to_array(np.array([1, sentinel, 2], np.int64))
    assert ei.value.code == _lib.CMS_E_PARAM


def test_prototypes_are_bound(lib):
    for name in ("cms_threshold_neighbors", "cms_fastidset_to_array"):
        assert name in _lib.EXPORTS and name in _lib._SIGS
        assert getattr(lib, name).argtypes == _lib._SIGS[name][1]
    assert (_lib.CMS_NEIGHBOR_ORDER_ID, _lib.CMS_NEIGHBOR_ORDER_FASTIDSET) == (0, 1)
    assert len(_lib._SIGS["cms_threshold_neighbors"][1]) == 10


def test_threshold_neighbors_null_arguments_need_no_device(lib):
    """The argument checks come before the handle is touched."""
    import ctypes
    total = ctypes.c_int64()
    off = np.zeros(1, np.int64)
    p = off.ctypes.data_as(ctypes.c_void_p)
    assert lib.cms_threshold_neighbors(None, None, 0, 0.5, 0, p, None, None, 0, ctypes.byref(total)) == _lib.CMS_E_PARAM
    assert lib.cms_fastidset_to_array(None, 0, None, None) == _lib.CMS_E_PARAM


def test_threshold_user_neighborhood_constructor_errors():
    sim, model = object(), object()
    with pytest.raises(ValueError, match="NaN"):
        taste.ThresholdUserNeighborhood(float("nan"), sim, model)
    for rate in (0.5, 0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="samplingRate"):
            taste.ThresholdUserNeighborhood(0.7, sim, model, rate)
    with pytest.raises(ValueError):
        taste.ThresholdUserNeighborhood(0.7, None, model)
    for t in (0.7, float("inf"), float("-inf"), -3.0):
        nb = taste.ThresholdUserNeighborhood(t, sim, model)
        assert nb.threshold == t
    assert taste.ThresholdUserNeighborhood(0.7, sim, model, samplingRate=1.0).threshold == 0.7
