"""GPU: the anonymous-profile queries (cms_anonymous_similarities,
cms_anonymous_most_similar, cms_anonymous_estimate_preferences: k_anon_sketch,
k_anon_rows, k_anon_cosine) against the oracle -- the profile's sketch from
oracle.build_table (CosineCM.exportProfile, `T/impl/similarity/CosineCM.java:41-58`),
its similarity with every owner from oracle.cosine_cm (`:83-96`,
`T/impl/common/DoubleCountMinSketch.java:114-149`), the lists from
oracle.top_users (`T/impl/recommender/TopItems.java:91-136`) and the estimates
from oracle.estimate_preference
(`T/impl/recommender/GenericUserBasedRecommender.java:134-184`).  Bit for bit,
NaN matching NaN; no tolerance anywhere.

The tables of sections 1-3 are DESIGNED: counters chosen in numpy, written by
mahout_amd.checkpoint.build_checkpoint with the stored form of every owner
named, installed with SketchTable.load_device.  Every stored form is present
by construction, and each test asserts on the CPU, before the GPU is used,
that the cases it is about occur in its design.

  1  every stored form (list, u1 .. u16, u32, zero) x six profiles, at
     w = 128, 64 and 30 (the w % 4 != 0 path), weighted and unweighted
  2  the 2^53 switch, all four (profile, owner) combinations
  3  top-k: ties decided by ID, NaN owners, k above the candidates, padding,
     n = 1, batch edges (Q = 1, B, B + 1, 3 B + 2), a handle without forms
  4  a hashed stream: a profile equal to an owner's pairs scores as that owner
  5  estimates and taste.PlusAnonymousUserDataModel's recommend(TEMP_USER_ID)
  6  the calls change nothing of the handle; the states that refuse them
"""
import os

import numpy as np
import pytest

from mahout_amd import SketchTable, _lib, checkpoint as ck, taste
from mahout_amd.datamodel import GenericDataModel
from mahout_amd.synth import movielens_like, zipf_stream

pytestmark = pytest.mark.gpu

SEED = 42


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def load_design(c, a, b, owner_ids=None, forms=None, lists=None, weighted=False, env=None):
    """A finalized handle holding the designed table c [n][d][w]."""
    import torch

    n, d, w = c.shape
    image = ck.build_checkpoint(c, a, b, seed=SEED, owner_ids=owner_ids, forms=forms, lists=lists)
    saved = {k: os.environ.pop(k, None) for k in ("CMS_NO_FORMS",)}
    os.environ.update(env or {})
    try:  # (the tunables are read once, at creation)
        t = SketchTable(n, depth=d, width=w, seed=SEED, weighted=weighted)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    try:
        dev = torch.device("cuda", t.device)
        t.load_device(torch.frombuffer(bytearray(image), dtype=torch.uint8).to(dev))
        t.finalize()
        assert np.array_equal(t.read_counters(), c.astype(np.float64))
    except BaseException:
        t.close()
        raise
    return t


def profile_sketch(oracle, d, w, a, b, keys, vals=None):
    keys = np.ascontiguousarray(keys, np.int64)
    return oracle.build_table(1, d, w, a, b, np.zeros(keys.size, np.int64), keys, vals)[0]


def expected_row(oracle, psk, table, weighted=False):
    return np.array([oracle.cosine_cm(psk, table[r], weighted) for r in range(table.shape[0])], np.float64)


# ------------------------------------------------------------ 1. forms ----

FORM_NAMES = ("list", "u1", "u2", "u4", "u8", "u16", "u32")
TWIN_KEYS = np.array([5, 9, 9, 1000, -7, 123456, 77, 5, 31, 2 ** 40], np.int64)
TWIN_VALS = np.array([1, 2, 3, 1, 4, 1, 2, 2, 5, 1], np.float32)


def forms_design(oracle, d, w, seed):
    """72 owners: ten of each form the shape has (the others' counters in u16
    rows), an all-zero owner, a `zero`-form owner, and one owner holding the
    sketch of (TWIN_KEYS, TWIN_VALS).  Returns (counters, forms, lists, ids)."""
    rng = _rng(seed)
    a, b = oracle.hash_params(SEED, d)
    rows, forms, lists = [], [], {}
    for name in FORM_NAMES:
        for _ in range(10):
            c = np.zeros((d, w), np.uint64)
            has = ck.shape_has_form(name, d, w)
            if name == "list":
                m = int(rng.integers(1, 41))
                ent = rng.integers(0, w, (d, m))
                for i in range(d):
                    c[i] = np.bincount(ent[i], minlength=w)
                if has:
                    lists[len(rows)] = ent
            elif name == "u32":
                for i in range(d):
                    c[i, rng.choice(w, 6, replace=False)] = rng.integers(1, 1 << 20, 6)
                c[0, 0] = 70000 + len(rows)
            elif name == "u16":
                for i in range(d):
                    c[i, rng.choice(w, 5, replace=False)] = rng.integers(256, 12000, 5)
            else:
                cap = {"u1": 1, "u2": 3, "u4": 15, "u8": 255}[name]
                c = (rng.integers(0, cap + 1, (d, w)) * (rng.random((d, w)) < 0.4)).astype(np.uint64)
                c[0, 1] = cap
            rows.append(c)
            forms.append(name if has else "u16")
    rows.append(np.zeros((d, w), np.uint64))
    forms.append(None)
    rows.append(np.zeros((d, w), np.uint64))
    forms.append("zero")
    rows.append(profile_sketch(oracle, d, w, a, b, TWIN_KEYS, TWIN_VALS).astype(np.uint64))
    forms.append(None)
    n = len(rows)
    ids = np.cumsum(rng.integers(1, 50, n)) - 1000  # explicit, non-contiguous, some negative
    return np.stack(rows), forms, lists, ids.astype(np.int64)


def form_profiles(w):
    rng = _rng(w)
    # 4 w keys with values up to 300: counters past u8 everywhere; past u16 as
    # well where 4 w x 300 can reach 2^16 (a key repeated 240 times), and in a
    # profile of its own at every width
    rep = 240 if 4 * w > 240 else 0
    big_k = np.concatenate([rng.integers(0, 10 ** 6, 4 * w - rep), np.full(rep, 4242)])
    big_v = np.concatenate([rng.integers(0, 301, 4 * w - rep), np.full(rep, 300)]).astype(np.float32)
    return {
        "past u16": (np.array([8, 9, 8, 10], np.int64), np.array([70000, 3, 2, 65535], np.float32)),
        "empty": (np.zeros(0, np.int64), None),
        "one key": (np.array([17], np.int64), None),
        "5 keys": (np.array([3, -4, 2 ** 33, 99, 3], np.int64), np.array([1, 2, 1, 7, 1], np.float32)),
        "w keys": (rng.integers(-10 ** 9, 10 ** 9, w), None),
        "4w keys": (big_k, big_v),
        "twin": (TWIN_KEYS, TWIN_VALS),
    }


@pytest.mark.parametrize("w", [128, 64, 30])
def test_every_stored_form(oracle, w):
    d = 5
    a, b = oracle.hash_params(SEED, d)
    c, forms, lists, ids = forms_design(oracle, d, w, 100 + w)
    n = c.shape[0]
    assert n == 73
    # the design holds what the shape can: every form at 128, no 1-bit rows at 64, u16 / u32 only at 30
    present = {f for f in forms if f}
    want = {f for f in FORM_NAMES if ck.shape_has_form(f, d, w)} | {"zero", "u16"}
    assert present == want, (present, want)
    assert (w == 128) == ("u1" in present) and (w == 30) == (present == {"u16", "u32", "zero"})
    assert bool(lists) == (w != 30)
    table = c.astype(np.float64)
    profs = form_profiles(w)
    sketches = {k: profile_sketch(oracle, d, w, a, b, *p) for k, p in profs.items()}
    assert sketches["empty"].max() == 0 and sketches["one key"].sum() == d
    assert np.sum(sketches["4w keys"] > 255) > 1 and (w == 30 or sketches["4w keys"].max() >= 65536)  # past u8, past u16
    assert sketches["past u16"].max() >= 65536 and profs["4w keys"][0].size == 4 * w
    twin_row = n - 1
    assert np.array_equal(sketches["twin"], table[twin_row])
    for weighted in (False, True):
        t = load_design(c, a, b, owner_ids=ids, forms=forms, lists=lists, weighted=weighted)
        try:
            assert t.stats()["list_rows"] == (10 if lists else 0)
            for name, (keys, vals) in profs.items():
                exp = expected_row(oracle, sketches[name], table, weighted)
                got = t.anonymous_similarities(keys, vals, ids)
                assert _same(got, exp), (w, weighted, name, np.flatnonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp)))))
                if name == "empty":
                    assert np.isnan(got).all()
                else:
                    assert np.isnan(got[n - 3]) and np.isnan(got[n - 2])  # the all-zero and zero-form owners
                    assert np.count_nonzero(~np.isnan(got)) >= n // 2 or name == "one key"
                if name == "twin":
                    assert got[twin_row] == oracle.cosine_cm(table[twin_row], table[twin_row], weighted)
                    assert got[twin_row] == t.similarities(ids[twin_row], ids[twin_row:twin_row + 1])[0]
                # a subset in another order, repeats included
                sub = np.array([ids[5], ids[n - 1], ids[5], ids[0], ids[61]], np.int64)
                assert _same(t.anonymous_similarities(keys, vals, sub), exp[[5, n - 1, 5, 0, 61]])
            with pytest.raises(_lib.CmsError) as ei:
                t.anonymous_similarities([1], None, [int(ids[0]) - 1])
            assert ei.value.code == _lib.CMS_E_NO_SUCH_ID
        finally:
            t.close()


# ---------------------------------------------------- 2. the 2^53 switch ----

def test_switch_at_2_53(oracle):
    d, w = 3, 64
    a, b = oracle.hash_params(SEED, d)
    K = 777
    big = np.float32(2.0 ** 27)
    others_k = np.array([1, 2, 3, 4, 5, 6, 8], np.int64)
    others_v = np.array([3, 5, 7, 9, 11, 13, 1001], np.float32)

    def stream(kval, scale):
        return np.concatenate([[K], others_k]), np.concatenate([[kval], others_v * np.float32(scale)]).astype(np.float32)

    owners = [stream(big, 1), stream(3, 1), stream(big, 3), stream(1, 2)]
    c = np.stack([profile_sketch(oracle, d, w, a, b, *s) for s in owners]).astype(np.uint64)
    table = c.astype(np.float64)
    norms = (table * table).sum(axis=2)
    assert (norms[0] >= 2.0 ** 53).all() and (norms[2] >= 2.0 ** 53).all()
    assert (norms[1] < 2.0 ** 53).all() and (norms[3] < 2.0 ** 53).all() and (norms[1] > 0).all()
    assert c.max() >= 2 ** 27
    profiles = {"at or above": stream(big, 5), "below": stream(2, 7)}
    t = load_design(c, a, b)
    try:
        for name, (keys, vals) in profiles.items():
            psk = profile_sketch(oracle, d, w, a, b, keys, vals)
            pn = (psk * psk).sum(axis=1)
            assert (pn >= 2.0 ** 53).all() if name == "at or above" else (pn < 2.0 ** 53).all()
            exp = expected_row(oracle, psk, table)
            assert not np.isnan(exp).any()
            got = t.anonymous_similarities(keys, vals, np.arange(4))
            assert _same(got, exp), (name, got, exp)
        # both regimes inside one batch of the list call
        ids, sc, cnt = t.anonymous_most_similar([profiles["below"], profiles["at or above"]], 4)
        for q, name in enumerate(("below", "at or above")):
            psk = profile_sketch(oracle, d, w, a, b, *profiles[name])
            ei, es = oracle.top_users(np.arange(4), expected_row(oracle, psk, table), 4)
            assert cnt[q] == ei.size and ids[q, :cnt[q]].tolist() == ei.tolist() and _same(sc[q, :cnt[q]], es)
    finally:
        t.close()


# ----------------------------------------------------------- 3. top-k ----

N3, D3, W3 = 513, 3, 64


def topk_design(seed):
    """513 owners: 40 distinct patterns shared by groups of identical owners
    (ties on every score, IDs deciding), 60 all-zero owners (NaN)."""
    rng = _rng(seed)
    pats = (rng.integers(0, 9, (40, D3, W3)) * (rng.random((40, D3, W3)) < 0.3)).astype(np.uint64)
    pats[:, :, 0] += 1
    which = rng.integers(0, 40, N3)
    c = pats[which]
    zero = rng.choice(N3, 60, replace=False)
    c[zero] = 0
    return c, which, zero


@pytest.fixture(scope="module")
def topk_case(oracle):
    a, b = oracle.hash_params(SEED, D3)
    c, which, zero = topk_design(9)
    table = c.astype(np.float64)
    rng = _rng(10)
    profs = []
    for q in range(26):
        m = int(rng.integers(3, 40))
        profs.append((rng.integers(0, 5000, m), rng.integers(1, 6, m).astype(np.float32)))
    profs[9] = (np.array([11, 12, 11], np.int64), np.array([40000, 5, 40000], np.float32))  # a counter past u16
    profs[20] = (np.zeros(0, np.int64), np.zeros(0, np.float32))                              # an empty profile
    sims = np.stack([expected_row(oracle, profile_sketch(oracle, D3, W3, a, b, *p), table) for p in profs])
    return a, b, c, zero, profs, sims


def check_lists(oracle, got, owner_ids, sims, k):
    ids, sc, cnt = got
    assert ids.shape == sc.shape == (sims.shape[0], k)
    for q in range(sims.shape[0]):
        ei, es = oracle.top_users(owner_ids, sims[q], k)
        m = int(cnt[q])
        assert m == ei.size, (q, m, ei.size)
        assert ids[q, :m].tolist() == ei.tolist(), q
        assert _same(sc[q, :m], es), q
        assert (ids[q, m:] == -1).all() and (sc[q, m:].view(np.uint64) == np.uint64(2 ** 64 - 1)).all(), q


def test_top_k_lists(oracle, topk_case):
    a, b, c, zero, profs, sims = topk_case
    owner_ids = np.arange(N3, dtype=np.int64)
    valid = N3 - zero.size
    assert valid < 512  # k = 512 is above the candidates of every profile
    assert np.isnan(sims[:, zero]).all() and np.isnan(sims[20]).all()
    q0 = sims[0][~np.isnan(sims[0])]
    assert np.unique(q0).size <= 40 < q0.size  # groups of equal scores: the IDs decide
    t = load_design(c, a, b)
    try:
        B = t.anonymous_batch(2)
        assert B == 8 and t.anonymous_batch(4) == 8
        for Q in (1, B, B + 1, 3 * B + 2):  # a batch edge is crossed from B + 1 on; profile 9 makes a u32 batch
            for k in (1, 7, 512):
                if Q > 1 and k == 7 and Q != 3 * B + 2:
                    continue
                check_lists(oracle, t.anonymous_most_similar(profs[:Q], k), owner_ids, sims[:Q], k)
        # the CSR form of the same batch
        off = np.zeros(27, np.int64)
        np.cumsum([p[0].size for p in profs], out=off[1:])
        csr = (off, np.concatenate([p[0] for p in profs]), np.concatenate([p[1] for p in profs]))
        check_lists(oracle, t.anonymous_most_similar(csr, 7), owner_ids, sims, 7)
        ids, sc, cnt = t.anonymous_most_similar([], 3)
        assert ids.shape == (0, 3) and cnt.size == 0
        for bad_k in (0, 513):
            with pytest.raises(_lib.CmsError) as ei:
                t.anonymous_most_similar(profs[:1], bad_k)
            assert ei.value.code == _lib.CMS_E_PARAM
    finally:
        t.close()


def test_top_k_without_forms(oracle, topk_case):
    a, b, c, zero, profs, sims = topk_case
    t = load_design(c, a, b, env={"CMS_NO_FORMS": "1"})
    try:
        st = t.stats()
        assert st["u8_rows"] == st["nibble_rows"] == st["crumb_rows"] == st["bit_rows"] == st["list_rows"] == 0
        check_lists(oracle, t.anonymous_most_similar(profs[:11], 7), np.arange(N3, dtype=np.int64), sims[:11], 7)
    finally:
        t.close()


def test_top_k_of_one_owner(oracle, topk_case):
    a, b, c, zero, profs, sims = topk_case
    r = int(np.setdiff1d(np.arange(N3), zero)[0])
    ids1 = np.array([77], np.int64)
    t = load_design(c[r:r + 1], a, b, owner_ids=ids1)
    try:
        check_lists(oracle, t.anonymous_most_similar(profs[:3], 5), ids1, sims[:3, r:r + 1], 5)
    finally:
        t.close()


# ------------------------------------------- 4. twin of a hashed stream ----

def test_twin_of_an_owner(oracle):
    d, w, n = 5, 256, 300
    owners, keys = zipf_stream(2000, n, 6000, seed=3)
    with SketchTable(n, depth=d, width=w, seed=SEED) as t:
        t.ingest(owners, keys)
        t.finalize()
        all_ids = np.arange(n, dtype=np.int64)
        k = 10
        picked = [int(o) for o in np.unique(owners)[:: max(1, np.unique(owners).size // 20)][:20]]
        assert len(picked) == 20
        for o in picked:
            mine = keys[owners == o]
            assert mine.size > 0
            want = t.similarities(o, all_ids)
            assert _same(t.anonymous_similarities(mine, None, all_ids), want), o
            # most_similar(o) with o itself inserted at its own score
            oi, os_ = t.most_similar(o, k)
            cand = sorted([(-float(s), int(i)) for i, s in zip(oi, os_)] + [(-float(want[o]), o)])[:k]
            ids, sc, cnt = t.anonymous_most_similar([(mine, None)], k)
            assert cnt[0] == len(cand)
            assert ids[0, :cnt[0]].tolist() == [i for _, i in cand], o
            assert sc[0, :cnt[0]].tolist() == [-s for s, _ in cand], o


# ------------------------------------- 5. estimates and the Taste route ----

D5, W5, NN5, HOW5 = 4, 1024, 15, 10


def test_recommend_for_the_temporary_user(oracle):
    users, items, ratings = movielens_like(n_users=60, n_items=300, n_ratings=3000, seed=5)
    uid_all = np.unique(users)
    T = taste.PlusAnonymousUserDataModel.TEMP_USER_ID
    a, b = oracle.hash_params(SEED, D5)
    for gone, capped in ((int(uid_all[7]), True), (int(uid_all[41]), False)):
        keep = users != gone
        u2, i2, r2 = users[keep], items[keep], ratings[keep]
        uid = np.unique(u2)
        rows = np.searchsorted(uid, u2)
        order = np.lexsort((i2, rows))
        rows, i2, r2 = rows[order], i2[order], r2[order]
        off = np.zeros(uid.size + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=uid.size), out=off[1:])
        base = GenericDataModel.from_csr(uid, off, i2, r2)
        if not capped:  # a model without min / max has no capper (GenericUserBasedRecommender.java:209-216)
            base.getMinPreference = lambda: float("nan")
            base.getMaxPreference = lambda: float("nan")
        model = taste.PlusAnonymousUserDataModel(base)
        tk, tv = items[users == gone], ratings[users == gone].astype(np.float32)
        assert tk.size >= 20
        # the oracle's table with the profile's sketch in front: row -1 of ext[1:]
        ext = np.concatenate([profile_sketch(oracle, D5, W5, a, b, tk, tv)[None],
                              oracle.build_table(uid.size, D5, W5, a, b, rows, i2, r2)])
        table = ext[1:]
        sim = taste.CosineCM(model, taste.FixedShapeConfig(D5, W5), taste.HashFunctionBuilder(SEED))
        try:
            nbh = taste.NearestNUserNeighborhood(NN5, sim, model)
            rec = taste.GenericUserBasedRecommender(model, nbh, sim)
            assert (rec._capper is not None) == capped
            with pytest.raises(taste.NoSuchUserException):
                rec.recommend(T, HOW5)  # no temporary preferences yet
            model.setTempPrefs(tk, tv)
            sims = expected_row(oracle, ext[0], table)
            assert _same([sim.userSimilarity(T, int(u)) for u in uid[:5]], sims[:5])
            assert sim.userSimilarity(int(uid[3]), T) == sims[3]
            nb, _ = oracle.top_users(uid, sims, NN5)
            assert nbh.getUserNeighborhood(T).tolist() == nb.tolist()
            cand = rec.getAllOtherItems(nb, T).toList()
            assert len(cand) > HOW5 and not set(cand) & set(tk.tolist())
            nb_rows = np.searchsorted(uid, nb)
            est = np.array([oracle.estimate_preference(table, a, b, -1, nb_rows, it, capper=rec._capper)
                            for it in cand], np.float32)
            assert np.array_equal(rec.doEstimatePreferences(T, nb, cand), est, equal_nan=True)
            want = taste.get_top_items(HOW5, cand, est)
            got = rec.recommend(T, HOW5)
            assert [i for i, _ in got] == [i for i, _ in want]
            assert [float(v) for _, v in got] == [float(v) for _, v in want]
            assert len(got) == min(HOW5, int(np.sum(~np.isnan(est)))) > 0
            # estimatePreference: the temporary user's own value, else the estimate
            assert rec.estimatePreference(T, int(tk[0])) == tv[0]
            assert np.array_equal(np.float32(rec.estimatePreference(T, cand[0])), est[0], equal_nan=True)
            # every other ID is served as before
            u = int(uid[0])
            assert sim.userSimilarity(u, int(uid[1])) == oracle.cosine_cm(table[0], table[1])
            with pytest.raises(_lib.CmsError) as ei:
                sim.table.anonymous_estimate_preferences(tk, tv, [int(uid[0]), gone], cand[:3])
            assert ei.value.code == _lib.CMS_E_NO_SUCH_ID
            model.clearTempPrefs()
            with pytest.raises(taste.NoSuchUserException):
                sim.userSimilarity(T, u)
        finally:
            sim.close()


# ------------------------------------------------- 6. non-interference ----

def test_calls_change_nothing_and_states_refuse(oracle):
    d, w, n = 4, 128, 200
    owners, keys = zipf_stream(500, n, 5000, seed=8)
    prof = (np.array([1, 2, 3, 2], np.int64), np.array([1, 2, 1, 1], np.float32))
    ids = np.arange(n, dtype=np.int64)
    with SketchTable(n, depth=d, width=w, seed=SEED) as t:
        t.ingest(owners[:4000], keys[:4000])
        with pytest.raises(_lib.CmsError) as ei:  # not finalized
            t.anonymous_similarities(*prof, ids)
        assert ei.value.code == _lib.CMS_E_STATE
        t.finalize()
        first = t.top_k_refresh(5)
        t.ingest(owners[4000:], keys[4000:])  # touched marks for the next refresh
        t.finalize()
        before = (t.read_counters(), t.stats(), t.refresh_stats())
        out0 = np.full(n, 7.0)
        for bad, code in (((prof[0], np.array([1, -2, 1, 1], np.float32)), _lib.CMS_E_VALUE),
                          ((prof[0], np.array([1, 0.5, 1, 1], np.float32)), _lib.CMS_E_VALUE),
                          ((prof[0], np.array([2.0 ** 31] * 4, np.float32)), _lib.CMS_E_OVERFLOW)):
            with pytest.raises(_lib.CmsError) as ei:
                t.anonymous_similarities(*bad, ids)
            assert ei.value.code == code
            with pytest.raises(_lib.CmsError) as ei:
                t.anonymous_most_similar([prof, bad], 3)  # the whole batch is validated first
            assert ei.value.code == code
        # a refused call writes no output
        import ctypes
        k_, v_ = np.array([1], np.int64), np.array([-1.0], np.float32)
        rc = t._lib.cms_anonymous_similarities(t._h, k_.ctypes.data_as(ctypes.c_void_p), v_.ctypes.data_as(ctypes.c_void_p),
                                               1, ids.ctypes.data_as(ctypes.c_void_p), n,
                                               out0.ctypes.data_as(ctypes.c_void_p))
        assert rc == _lib.CMS_E_VALUE and (out0 == 7.0).all()
        with pytest.raises(_lib.CmsError) as ei:
            t.anonymous_most_similar((np.array([0, 3, 2]), prof[0], prof[1]), 3)
        assert ei.value.code == _lib.CMS_E_PARAM
        # a mix of the new calls
        s = t.anonymous_similarities(*prof, ids)
        t.anonymous_most_similar([prof, (keys[:50], None), (np.zeros(0, np.int64), None)], 9)
        e = t.anonymous_estimate_preferences(*prof, ids[:20], np.arange(30))
        assert s.shape == (n,) and e.shape == (30,)
        assert np.isnan(t.anonymous_estimate_preferences(np.zeros(0, np.int64), None, ids[:20], np.arange(5))).all()
        after = (t.read_counters(), t.stats(), t.refresh_stats())
        assert np.array_equal(before[0], after[0])
        assert {k: v for k, v in before[1].items() if k != "topk_redo"} == \
               {k: v for k, v in after[1].items() if k != "topk_redo"}
        assert before[2] == after[2]
        assert _same(t.similarities(3, ids), t.similarities(3, ids))  # still finalized
        # a following refresh is what it is on a handle that never saw the calls
        got = t.top_k_refresh(5)
        rs = t.refresh_stats()
    with SketchTable(n, depth=d, width=w, seed=SEED) as u:
        u.ingest(owners[:4000], keys[:4000])
        u.finalize()
        first_u = u.top_k_refresh(5)
        u.ingest(owners[4000:], keys[4000:])
        u.finalize()
        want = u.top_k_refresh(5)
        assert u.refresh_stats() == rs
    for x, y in zip(first + got, first_u + want):
        assert np.array_equal(x, y, equal_nan=True)
    # handles of the other modes refuse
    with SketchTable(n, depth=d, width=w, seed=SEED, counters="f64") as f:
        f.ingest(owners, keys)
        f.finalize()
        with pytest.raises(_lib.CmsError) as ei:
            f.anonymous_similarities(*prof, ids)
        assert ei.value.code == _lib.CMS_E_STATE and "fp64" in str(ei.value)
    off = np.zeros(n + 1, np.int64)
    order = np.argsort(owners, kind="stable")
    np.cumsum(np.bincount(owners, minlength=n), out=off[1:])
    with SketchTable.per_owner_shapes(n, seed=SEED) as p:
        p.ingest_csr(off, keys[order], np.ones(keys.size, np.float32))
        p.configure_owner_shapes(0.5, 500)
        p.finalize()
        for call in (lambda: p.anonymous_similarities(*prof, ids), lambda: p.anonymous_most_similar([prof], 3),
                     lambda: p.anonymous_estimate_preferences(*prof, ids[:4], [1, 2])):
            with pytest.raises(_lib.CmsError) as ei:
                call()
            assert ei.value.code == _lib.CMS_E_STATE and "per-owner" in str(ei.value)
