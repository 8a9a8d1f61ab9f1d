"""SketchTable: a handle to the device-resident count-min-sketch table.

Thin, typed wrapper over the C ABI (include/mahout_cms.h).  One table holds
the [num_owners][depth][width] u32 sketches of every owner; the reference
builds the same sketches one DoubleCountMinSketch at a time
(T/impl/common/DoubleCountMinSketch.java, T/impl/similarity/CosineCM.java:41-67).
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import check


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dev_ptr(x):
    """Device pointer from an int or a torch tensor (None passes through)."""
    if x is None:
        return None
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    return ctypes.c_void_p(x.data_ptr())


def _torch_stream(*xs):
    """Current torch stream (hipStream_t) of the first device tensor (0: the
    legacy default stream), or None when no input is a device tensor."""
    import torch

    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return torch.cuda.current_stream(x.device).cuda_stream
    return None


def shape_from_delta_epsilon(delta, epsilon):
    """AbstractCountMinSketch(delta, epsilon) shape rule -> (width, depth)."""
    lib = _lib.load()
    w = ctypes.c_int32()
    d = ctypes.c_int32()
    check(lib.cms_shape_from_delta_epsilon(delta, epsilon, ctypes.byref(w), ctypes.byref(d)))
    return w.value, d.value


def frac_bits_for(values, max_bits=31):
    """Smallest frac_bits with every value * 2^frac_bits an integer (the
    preference granularity a u32 handle needs); ValueError when none <= max_bits."""
    v = np.asarray(values, np.float32).astype(np.float64)
    if v.size == 0:
        return 0
    for fb in range(max_bits + 1):
        x = np.ldexp(v, fb)
        if np.all(x == np.floor(x)):
            return fb
    raise ValueError("preference values need more than %d fractional bits" % max_bits)


def shard_of_key(key, world):
    return _lib.load().cms_shard_of_key(int(key), int(world))


def comm_unique_id():
    buf = (ctypes.c_uint8 * 128)()
    check(_lib.load().cms_comm_unique_id(buf))
    return bytes(buf)


class SketchTable:
    def __init__(self, num_owners, depth=5, width=4096, seed=42, weighted=False, device=-1, owner_ids=None,
                 per_owner=False, frac_bits=0, counters="u32", collective_single_rank=False):
        """counters: "u32" (exact integer counters in units of 2^-frac_bits) or
        "f64" (DoubleCountMinSketch's fp64 counters for any float preference).
        collective_single_rank: CMS_FLAG_COLLECTIVE_SINGLE_RANK (a one-rank
        comm_init still takes the multi-rank data path)."""
        lib = _lib.load()
        p = _lib.CmsParams()
        check(lib.cms_params_init(ctypes.byref(p)))
        p.counter_type = {"u32": _lib.CMS_COUNTER_U32, "f64": _lib.CMS_COUNTER_F64}[counters]
        p.depth = depth
        p.width = width
        p.seed = seed
        p.num_owners = num_owners
        p.weighting = _lib.CMS_WEIGHTED if weighted else _lib.CMS_UNWEIGHTED
        p.device = device
        p.frac_bits = frac_bits
        p.flags = _lib.CMS_FLAG_COLLECTIVE_SINGLE_RANK if collective_single_rank else 0
        h = ctypes.c_void_p()
        create = lib.cms_create_per_owner if per_owner else lib.cms_create
        check(create(ctypes.byref(p), ctypes.byref(h)))
        self.per_owner = per_owner
        self.counters = counters
        self._lib = lib
        self._h = h
        if device < 0:  # the device the library chose (hipGetDevice at creation), not torch's guess
            device = self.stats()["device"]
        self.device = int(device)
        self.num_owners = num_owners
        self.depth = depth
        self.width = width
        self.seed = seed
        self.weighted = bool(weighted)
        self.frac_bits = frac_bits
        self.hash_rows = 32 if per_owner else depth  # CMS_MAX_DEPTH rows for per-owner handles
        if owner_ids is not None:
            self.set_owner_ids(owner_ids)

    # -- lifecycle --
    def close(self):
        if self._h:
            self._lib.cms_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- setup --
    def set_owner_ids(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        check(self._lib.cms_set_owner_ids(self._h, _ptr(ids), ids.size))
    def hash_params(self):
        """(a_i, b_i) of every hash row: depth rows, or all CMS_MAX_DEPTH (32)
        rows of a per-owner handle (any owner's shape may use them)."""
        a = np.zeros(self.hash_rows, np.int64)
        b = np.zeros(self.hash_rows, np.int64)
        check(self._lib.cms_hash_params(self._h, _ptr(a), _ptr(b)))
        return a, b

    def set_hash_params(self, a, b):
        """Install a HashFunctionBuilder's drawn (a_i, b_i) (cms_set_hash_params);
        one pair per sketch row of the handle (32 for per-owner handles)."""
        a = np.ascontiguousarray(a, np.int64)
        b = np.ascontiguousarray(b, np.int64)
        if a.shape != b.shape:
            raise ValueError("a and b differ in length")
        check(self._lib.cms_set_hash_params(self._h, _ptr(a), _ptr(b), int(a.size)))

    def hash_keys(self, keys):
        keys = np.ascontiguousarray(keys, np.int64)
        out = np.zeros((keys.size, self.depth), np.int32)
        check(self._lib.cms_hash_keys(self._h, _ptr(keys), keys.size, _ptr(out)))
        return out

    # -- ingest --
    def ingest(self, owner, key, val=None):
        owner = np.ascontiguousarray(owner, np.int64)
        key = np.ascontiguousarray(key, np.int64)
        v = None if val is None else np.ascontiguousarray(val, np.float32)
        if owner.size != key.size or (v is not None and v.size != key.size):
            raise ValueError("owner/key/val length mismatch")
        check(self._lib.cms_ingest(self._h, _ptr(owner), _ptr(key), _ptr(v), owner.size))

    def ingest_device_rows(self, d_row, d_key, d_val, n):
        # stream-ordered both ways (no host wait): the library's stream waits
        # for the producers on torch's current stream, and torch's stream waits
        # for the ingest, so the inputs may be freed once this returns.  The
        # library stream is a blocking stream, so against torch's legacy
        # default stream (s == 0) that ordering is implicit.
        s = _torch_stream(d_row, d_key, d_val)
        if s:
            check(self._lib.cms_wait_stream(self._h, ctypes.c_void_p(s)))
        check(self._lib.cms_ingest_device_rows(self._h, _dev_ptr(d_row), _dev_ptr(d_key), _dev_ptr(d_val), int(n)))
        if s:
            check(self._lib.cms_release_to_stream(self._h, ctypes.c_void_p(s)))
        elif s is None:
            self.synchronize()

    def retract(self, owner, key, val=None):
        """Take pairs that were ingested out of the live table (cms_retract):
        DoubleCountMinSketch.update(key, -val) per pair, owners by ID.  All or
        nothing: CMS_E_OVERFLOW (nothing written) when an owner's batch mass
        exceeds its mass or a counter's summed decrements exceed it.  The
        table needs finalize() before the next query."""
        owner = np.ascontiguousarray(owner, np.int64)
        key = np.ascontiguousarray(key, np.int64)
        v = None if val is None else np.ascontiguousarray(val, np.float32)
        if owner.size != key.size or (v is not None and v.size != key.size):
            raise ValueError("owner/key/val length mismatch")
        check(self._lib.cms_retract(self._h, _ptr(owner), _ptr(key), _ptr(v), owner.size))

    def retract_device_rows(self, d_row, d_key, d_val, n):
        """retract() for pairs resident on the device, owners by row index
        (cms_retract_device_rows).  Blocking, unlike ingest_device_rows: the
        library's stream waits for the producers on torch's current stream,
        and the table has changed (or the call was refused) on return."""
        s = _torch_stream(d_row, d_key, d_val)
        if s:
            check(self._lib.cms_wait_stream(self._h, ctypes.c_void_p(s)))
        check(self._lib.cms_retract_device_rows(self._h, _dev_ptr(d_row), _dev_ptr(d_key), _dev_ptr(d_val), int(n)))

    def ingest_csr(self, offsets, keys, vals=None):
        offsets = np.ascontiguousarray(offsets, np.int64)
        keys = np.ascontiguousarray(keys, np.int64)
        v = None if vals is None else np.ascontiguousarray(vals, np.float32)
        if offsets.size != self.num_owners + 1:
            raise ValueError("offsets must have num_owners + 1 entries")
        check(self._lib.cms_ingest_csr(self._h, _ptr(offsets), _ptr(keys), _ptr(v)))

    def ingest_csr_device(self, d_offsets, d_keys, d_vals=None):
        s = _torch_stream(d_offsets, d_keys, d_vals)
        if s:
            check(self._lib.cms_wait_stream(self._h, ctypes.c_void_p(s)))
        check(self._lib.cms_ingest_csr_device(self._h, _dev_ptr(d_offsets), _dev_ptr(d_keys), _dev_ptr(d_vals)))
        if s:
            check(self._lib.cms_release_to_stream(self._h, ctypes.c_void_p(s)))
        elif s is None:
            self.synchronize()

    def reset(self):
        check(self._lib.cms_reset(self._h))

    def comm_init(self, unique_id, rank, world):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        check(self._lib.cms_comm_init(self._h, buf, rank, world))

    def comm_init_transport(self, rank, world, allreduce, allgather):
        """cms_comm_init_transport: a caller-supplied communicator in place of
        RCCL.  allreduce(d_ptr, count) sums `count` u64 words at device address
        d_ptr over all ranks in place; allgather(d_send, d_recv, nbytes) writes
        every rank's `nbytes` bytes at d_send, in rank order, to d_recv.  See
        mahout_amd.transport for a torch.distributed implementation."""
        def ar(ptr, count, _user):
            try:
                allreduce(int(ptr), int(count))
                return 0
            except Exception:  # noqa: BLE001 -- reported as a status code
                import traceback
                traceback.print_exc()
                return 1

        def ag(send, recv, nbytes, _user):
            try:
                allgather(int(send), int(recv), int(nbytes))
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1
        # the C side keeps the function pointers: hold the thunks for the handle's life
        self._transport = (_lib.ALLREDUCE_FN(ar), _lib.ALLGATHER_FN(ag))
        check(self._lib.cms_comm_init_transport(self._h, int(rank), int(world), self._transport[0],
                                                self._transport[1], None))

    def finalize(self):
        check(self._lib.cms_finalize(self._h))

    def finalize_with(self, allreduce):
        """cms_finalize_with: merge through a caller collective.
        allreduce(d_ptr, count) must sum `count` u64 words at device address
        d_ptr over all ranks, in place."""
        def thunk(ptr, count, _user):
            try:
                allreduce(int(ptr), int(count))
                return 0
            except Exception:  # noqa: BLE001 -- reported as a status code
                import traceback
                traceback.print_exc()
                return 1
        cb = _lib.ALLREDUCE_FN(thunk)
        check(self._lib.cms_finalize_with(self._h, cb, None))

    def synchronize(self):
        check(self._lib.cms_synchronize(self._h))

    # -- queries --
    def similarity(self, id1, id2):
        out = ctypes.c_double()
        check(self._lib.cms_similarity(self._h, int(id1), int(id2), ctypes.byref(out)))
        return out.value

    def similarities(self, id1, ids2):
        ids2 = np.ascontiguousarray(ids2, np.int64)
        out = np.zeros(ids2.size, np.float64)
        check(self._lib.cms_similarities(self._h, int(id1), _ptr(ids2), ids2.size, _ptr(out)))
        return out

    def point_query(self, owner_id, key):
        out = ctypes.c_double()
        check(self._lib.cms_point_query(self._h, int(owner_id), int(key), ctypes.byref(out)))
        return out.value

    def most_similar(self, owner_id, k):
        ids = np.zeros(k, np.int64)
        sc = np.zeros(k, np.float64)
        cnt = ctypes.c_int32()
        check(self._lib.cms_most_similar(self._h, int(owner_id), int(k), _ptr(ids), _ptr(sc), ctypes.byref(cnt)))
        return ids[:cnt.value], sc[:cnt.value]

    def top_k_rows(self, row_begin, row_count, k):
        ids = np.zeros((row_count, k), np.int64)
        sc = np.zeros((row_count, k), np.float64)
        cnt = np.zeros(row_count, np.int32)
        check(self._lib.cms_top_k_rows(self._h, int(row_begin), int(row_count), int(k), _ptr(ids), _ptr(sc),
                                       _ptr(cnt)))
        return ids, sc, cnt

    _NEIGHBOR_ORDERS = {"id": _lib.CMS_NEIGHBOR_ORDER_ID, "fastidset": _lib.CMS_NEIGHBOR_ORDER_FASTIDSET}

    def threshold_neighbors(self, owner_ids, threshold, order="id", scores=True, capacity=None):
        """ThresholdUserNeighborhood lists of many owners (cms_threshold_neighbors):
        every other owner whose similarity is not NaN and >= threshold.
        order "id": ascending owner ID; "fastidset": FastIDSet.toArray() order,
        what getUserNeighborhood returns.  Returns (offsets [nq + 1], ids,
        scores or None): owner_ids[q]'s list is ids[offsets[q]:offsets[q + 1]].
        One call with a guessed capacity (or `capacity` entries), and one
        more with the exact total when that was short."""
        q = np.ascontiguousarray(owner_ids, np.int64).reshape(-1)
        nq, n = q.size, self.num_owners
        off = np.zeros(nq + 1, np.int64)
        total = ctypes.c_int64()
        cap = min(nq * (n - 1), max(1 << 20, 64 * nq)) if capacity is None else max(0, int(capacity))
        for attempt in range(2):
            ids = np.zeros(max(cap, 1), np.int64)
            sc = np.zeros(max(cap, 1), np.float64) if scores else None
            rc = self._lib.cms_threshold_neighbors(self._h, _ptr(q), nq, float(threshold), self._NEIGHBOR_ORDERS[order],
                                                   _ptr(off), _ptr(ids), _ptr(sc), cap, ctypes.byref(total))
            if rc == _lib.CMS_E_PARAM and attempt == 0 and total.value > cap and off[-1] == total.value:
                cap = total.value  # refused for room alone: the exact size is known now
                continue
            check(rc)
            break
        t = total.value
        return off, ids[:t], (sc[:t] if scores else None)

    def threshold_neighbor_counts(self, owner_ids, threshold):
        """The list lengths threshold_neighbors would return (count-only call)."""
        q = np.ascontiguousarray(owner_ids, np.int64).reshape(-1)
        off = np.zeros(q.size + 1, np.int64)
        total = ctypes.c_int64()
        check(self._lib.cms_threshold_neighbors(self._h, _ptr(q), q.size, float(threshold), _lib.CMS_NEIGHBOR_ORDER_ID,
                                                _ptr(off), None, None, 0, ctypes.byref(total)))
        return np.diff(off)

    def estimate_preferences(self, user_id, neighbor_ids, item_keys, capper=None):
        """doEstimatePreference(user, neighbourhood, item) for every item key
        (CosineCM point-query path); capper = (min, max) or None."""
        nb = np.ascontiguousarray(neighbor_ids, np.int64)
        it = np.ascontiguousarray(item_keys, np.int64)
        out = np.zeros(it.size, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_estimate_preferences(self._h, int(user_id), _ptr(nb), nb.size, _ptr(it), it.size,
                                                 int(capper is not None), float(lo), float(hi), _ptr(out)))
        return out

    # -- the exact CosineSimilarity over an attached DataModel --
    def attach_exact(self, offsets, keys=None, vals=None):
        """The owners' DataModel for the exact cosine (cms_exact_attach_csr):
        a CSR over the table's owner rows (keys strictly ascending within a
        row), or a GenericDataModel whose users are the owners.  The sketch
        table is neither read nor written; a second call replaces the model."""
        if keys is None and hasattr(offsets, "offsets"):
            model = offsets
            if not model.hasPreferenceValues():
                raise ValueError("DataModel doesn't have preference values")
            offsets, keys, vals = model.offsets, model.keys, model.values
        offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        keys = np.ascontiguousarray(keys, np.int64).reshape(-1)
        vals = np.ascontiguousarray(vals, np.float32).reshape(-1)
        if offsets.size != self.num_owners + 1:
            raise ValueError("offsets needs num_owners + 1 entries")
        if keys.size != vals.size or (offsets.size and int(offsets.max()) > keys.size):
            raise ValueError("offsets reach past the keys, or keys and vals differ in length")
        check(self._lib.cms_exact_attach_csr(self._h, _ptr(offsets), _ptr(keys), _ptr(vals)))

    def owner_rows(self, owner_ids):
        """The owner rows of owner IDs (cms_owner_rows; CMS_E_NO_SUCH_ID for an unknown one)."""
        ids = np.ascontiguousarray(owner_ids, np.int64).reshape(-1)
        rows = np.zeros(ids.size, np.int64)
        check(self._lib.cms_owner_rows(self._h, _ptr(ids), ids.size, _ptr(rows)))
        return rows

    def detach_exact(self):
        check(self._lib.cms_exact_detach(self._h))

    def exact_similarities(self, id1, ids2):
        """CosineSimilarity.userSimilarity(id1, ids2[t]) over the attached model."""
        ids2 = np.ascontiguousarray(ids2, np.int64).reshape(-1)
        out = np.zeros(ids2.size, np.float64)
        check(self._lib.cms_exact_similarities(self._h, int(id1), _ptr(ids2), ids2.size, _ptr(out)))
        return out

    def exact_pairs(self, ids1, ids2):
        """CosineSimilarity.userSimilarity(ids1[t], ids2[t]), element-wise."""
        ids1 = np.ascontiguousarray(ids1, np.int64).reshape(-1)
        ids2 = np.ascontiguousarray(ids2, np.int64).reshape(-1)
        if ids1.size != ids2.size:
            raise ValueError("ids1 and ids2 differ in length")
        out = np.zeros(ids1.size, np.float64)
        check(self._lib.cms_exact_pairs(self._h, _ptr(ids1), _ptr(ids2), ids1.size, _ptr(out)))
        return out

    def exact_top_k_rows(self, rows, k):
        """The k most similar owners of each owner row under the exact cosine:
        ids [nq][k], scores [nq][k] (padding: ID -1, NaN) and counts [nq],
        ordered as top_k_rows orders them."""
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1)
        ids = np.zeros((rows.size, k), np.int64)
        sc = np.zeros((rows.size, k), np.float64)
        cnt = np.zeros(rows.size, np.int32)
        check(self._lib.cms_exact_top_k_rows(self._h, _ptr(rows), rows.size, int(k), _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def exact_most_similar(self, owner_id, k):
        """mostSimilarUserIDs(owner_id, k) under the exact cosine: (ids, scores)."""
        ids = np.zeros(k, np.int64)
        sc = np.zeros(k, np.float64)
        cnt = ctypes.c_int32()
        check(self._lib.cms_exact_most_similar(self._h, int(owner_id), int(k), _ptr(ids), _ptr(sc), ctypes.byref(cnt)))
        return ids[:cnt.value], sc[:cnt.value]

    def exact_estimate_preferences(self, user_id, neighbor_ids, item_keys, capper=None):
        """doEstimatePreference(user, neighbourhood, item) for every item key
        over the attached model's raw preferences and the exact cosine (the
        reference's path for a similarity that is no CosineCM); capper =
        (min, max) or None.  A batch of one user."""
        nb = np.ascontiguousarray(neighbor_ids, np.int64).reshape(-1)
        it = np.ascontiguousarray(item_keys, np.int64).reshape(-1)
        return self.exact_estimate_preferences_batch([user_id], [0, nb.size], nb, [0, it.size], it, capper)

    def exact_estimate_preferences_batch(self, user_ids, nb_offsets, neighbor_ids, item_offsets, item_keys,
                                         capper=None):
        """exact_estimate_preferences for many users in one call
        (cms_exact_estimate_preferences_batch), shaped as
        estimate_preferences_batch; item keys may repeat, come in any order
        and be unknown to the model (NaN)."""
        us, nbo, nb, ito, it = SketchTable._estimate_batch_args(user_ids, nb_offsets, neighbor_ids, item_offsets,
                                                                item_keys)
        out = np.zeros(it.size, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_exact_estimate_preferences_batch(self._h, us.size, _ptr(us), _ptr(nbo), _ptr(nb),
                                                             _ptr(ito), _ptr(it), int(capper is not None), float(lo),
                                                             float(hi), _ptr(out)))
        return out

    def exact_recommend_batch(self, user_ids, nb_offsets, neighbor_ids, how_many, include_known=False, capper=None):
        """cms_exact_recommend_batch: GenericUserBasedRecommender.recommend
        over exact_estimate_preferences for every user of user_ids at once,
        shaped as recommend_batch with the attached model as the DataModel.
        Returns (counts [n], items [n][how_many], values [n][how_many] float32)."""
        us = np.ascontiguousarray(user_ids, np.int64).reshape(-1)
        nbo = np.ascontiguousarray(nb_offsets, np.int64).reshape(-1)
        nb = np.ascontiguousarray(neighbor_ids, np.int64).reshape(-1)
        if nbo.size != us.size + 1 or nbo[0] != 0 or nbo[-1] != nb.size or bool(np.any(np.diff(nbo) < 0)):
            raise ValueError("nb_offsets must hold len(user_ids) + 1 non-decreasing entries from 0 to len(neighbor_ids)")
        if how_many < 1:
            raise ValueError("howMany must be at least 1")
        counts = np.zeros(us.size, np.int32)
        items = np.full((us.size, how_many), -1, np.int64)
        vals = np.full((us.size, how_many), np.nan, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_exact_recommend_batch(self._h, us.size, _ptr(us), _ptr(nbo), _ptr(nb), int(how_many),
                                                  int(bool(include_known)), int(capper is not None), float(lo),
                                                  float(hi), _ptr(counts), _ptr(items), _ptr(vals)))
        return counts, items, vals

    # -- anonymous profiles: preferences that are no row of the table --
    @staticmethod
    def _profile(keys, vals):
        keys = np.ascontiguousarray(keys, np.int64).reshape(-1)
        if vals is not None:
            vals = np.ascontiguousarray(vals, np.float32).reshape(-1)
            if vals.size != keys.size:
                raise ValueError("keys and vals differ in length")
        return keys, vals

    def anonymous_similarities(self, keys, vals, ids2):
        """CosineCM.userSimilarity(TEMP_USER_ID, ids2[i]) for the temporary
        preferences (keys, vals; vals None = 1.0 each)."""
        keys, vals = self._profile(keys, vals)
        ids2 = np.ascontiguousarray(ids2, np.int64)
        out = np.zeros(ids2.size, np.float64)
        check(self._lib.cms_anonymous_similarities(self._h, _ptr(keys), _ptr(vals), keys.size, _ptr(ids2), ids2.size,
                                                   _ptr(out)))
        return out

    def anonymous_most_similar(self, profiles, k):
        """mostSimilarUserIDs(TEMP_USER_ID, k) for many profiles at once.
        profiles: (offsets, keys, vals) in CSR form (vals may be None), or a
        list of (keys, vals) pairs.  Returns ids [nq][k], scores [nq][k]
        (padding: ID -1, NaN) and counts [nq], as top_k_rows does."""
        if isinstance(profiles, tuple) and len(profiles) == 3 and not isinstance(profiles[0], tuple):
            offsets, keys, vals = profiles
            offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
            keys, vals = self._profile(keys, vals)
        else:
            plist = [self._profile(kk, vv) for kk, vv in profiles]
            offsets = np.zeros(len(plist) + 1, np.int64)
            np.cumsum([p[0].size for p in plist], out=offsets[1:])
            keys = np.concatenate([p[0] for p in plist]) if plist else np.zeros(0, np.int64)
            with_vals = [p[1] is not None for p in plist]
            if any(with_vals):  # a profile without values reads as 1.0 each
                vals = np.concatenate([p[1] if p[1] is not None else np.ones(p[0].size, np.float32) for p in plist])
            else:
                vals = None
        if offsets.size < 1:
            raise ValueError("offsets needs nq + 1 entries")
        nq = offsets.size - 1
        if nq > 0 and (keys.size < int(offsets.max()) or (vals is not None and vals.size != keys.size)):
            raise ValueError("offsets reach past the keys")
        ids = np.zeros((nq, k), np.int64)
        sc = np.zeros((nq, k), np.float64)
        cnt = np.zeros(nq, np.int32)
        check(self._lib.cms_anonymous_most_similar(self._h, nq, _ptr(offsets), _ptr(keys), _ptr(vals), int(k),
                                                   _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def anonymous_estimate_preferences(self, keys, vals, neighbor_ids, item_keys, capper=None):
        """doEstimatePreference(TEMP_USER_ID, neighbourhood, item) for every
        item key; capper = (min, max) or None."""
        keys, vals = self._profile(keys, vals)
        nb = np.ascontiguousarray(neighbor_ids, np.int64)
        it = np.ascontiguousarray(item_keys, np.int64)
        out = np.zeros(it.size, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_anonymous_estimate_preferences(self._h, _ptr(keys), _ptr(vals), keys.size, _ptr(nb),
                                                           nb.size, _ptr(it), it.size, int(capper is not None),
                                                           float(lo), float(hi), _ptr(out)))
        return out

    def anonymous_batch(self, elem_bytes=2):
        """Profiles the similarity kernel serves per read of an owner's row."""
        b = ctypes.c_int32()
        check(self._lib.cms_anonymous_batch(self._h, int(elem_bytes), ctypes.byref(b)))
        return b.value

    @staticmethod
    def _estimate_batch_args(user_ids, nb_offsets, neighbor_ids, item_offsets, item_keys):
        """The arrays of an estimate batch as contiguous int64, checked."""
        us = np.ascontiguousarray(user_ids, np.int64)
        nbo = np.ascontiguousarray(nb_offsets, np.int64)
        nb = np.ascontiguousarray(neighbor_ids, np.int64)
        ito = np.ascontiguousarray(item_offsets, np.int64)
        it = np.ascontiguousarray(item_keys, np.int64)
        if nbo.size != us.size + 1 or ito.size != us.size + 1:
            raise ValueError("offset arrays need len(user_ids) + 1 entries")
        # the library reads neighbor_ids / item_keys up to the last offsets and
        # writes item_offsets[-1] estimates: the offsets must describe exactly
        # these arrays, or the call would run past the host buffers
        for name, o, arr in (("nb_offsets", nbo, nb), ("item_offsets", ito, it)):
            if o[0] != 0 or o[-1] != arr.size or (o.size > 1 and bool(np.any(np.diff(o) < 0))):
                raise ValueError(f"{name} must start at 0, never decrease and end at the length of its array")
        return us, nbo, nb, ito, it

    def estimate_preferences_batch(self, user_ids, nb_offsets, neighbor_ids, item_offsets, item_keys, capper=None):
        """estimate_preferences for many users in one call
        (cms_estimate_preferences_batch): user u's neighbourhood is
        neighbor_ids[nb_offsets[u]:nb_offsets[u+1]], its candidates
        item_keys[item_offsets[u]:item_offsets[u+1]]; returns one float32
        estimate per candidate."""
        us, nbo, nb, ito, it = SketchTable._estimate_batch_args(user_ids, nb_offsets, neighbor_ids, item_offsets,
                                                                item_keys)
        out = np.zeros(it.size, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_estimate_preferences_batch(self._h, us.size, _ptr(us), _ptr(nbo), _ptr(nb), _ptr(ito),
                                                       _ptr(it), int(capper is not None), float(lo), float(hi),
                                                       _ptr(out)))
        return out

    def recommend_batch(self, user_ids, nb_offsets, neighbor_ids, model_user_ids, pref_offsets, pref_items,
                        how_many, include_known=False, capper=None):
        """cms_recommend_batch: GenericUserBasedRecommender.recommend for every
        user of user_ids at once. User u's neighbourhood is
        neighbor_ids[nb_offsets[u]:nb_offsets[u+1]] (IDs); the DataModel is
        model_user_ids (ascending) with row r's item IDs
        pref_items[pref_offsets[r]:pref_offsets[r+1]]. Returns (counts [n],
        items [n][how_many], values [n][how_many] float32)."""
        us = np.ascontiguousarray(user_ids, np.int64)
        nbo = np.ascontiguousarray(nb_offsets, np.int64)
        nb = np.ascontiguousarray(neighbor_ids, np.int64)
        mu = np.ascontiguousarray(model_user_ids, np.int64)
        po = np.ascontiguousarray(pref_offsets, np.int64)
        pi = np.ascontiguousarray(pref_items, np.int64)
        # the library reads every array up to its last offset: they must match
        if nbo.size != us.size + 1 or nbo[0] != 0 or nbo[-1] != nb.size or bool(np.any(np.diff(nbo) < 0)):
            raise ValueError("nb_offsets must hold len(user_ids) + 1 non-decreasing entries from 0 to len(neighbor_ids)")
        if po.size != mu.size + 1 or po[0] != 0 or po[-1] != pi.size or bool(np.any(np.diff(po) < 0)):
            raise ValueError("pref_offsets must hold len(model_user_ids) + 1 non-decreasing entries from 0 to "
                             "len(pref_items)")
        if how_many < 1:
            raise ValueError("howMany must be at least 1")
        counts = np.zeros(us.size, np.int32)
        items = np.full((us.size, how_many), -1, np.int64)
        vals = np.full((us.size, how_many), np.nan, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_recommend_batch(self._h, us.size, _ptr(us), _ptr(nbo), _ptr(nb), mu.size, _ptr(mu),
                                            _ptr(po), _ptr(pi), int(how_many), int(bool(include_known)),
                                            int(capper is not None), float(lo), float(hi), _ptr(counts),
                                            _ptr(items), _ptr(vals)))
        return counts, items, vals

    # -- item-based recommender: owners are items --
    def similarity_block(self, ids1, ids2):
        """cms_similarity_block: the [n1][n2] float64 block of the similarity
        matrix, row i equal to similarities(ids1[i], ids2) bit for bit; one
        read of each ids1 row serves all of ids2.  IDs may repeat."""
        a = np.ascontiguousarray(ids1, np.int64).reshape(-1)
        b = np.ascontiguousarray(ids2, np.int64).reshape(-1)
        out = np.zeros((a.size, b.size), np.float64)
        check(self._lib.cms_similarity_block(self._h, _ptr(a), a.size, _ptr(b), b.size, _ptr(out)))
        return out

    @staticmethod
    def _csr(name, offsets, n, *arrays):
        o = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        # the library reads every array up to its last offset: they must match
        if o.size != n + 1 or o[0] != 0 or bool(np.any(np.diff(o) < 0)) or any(a.size != o[-1] for a in arrays):
            raise ValueError(f"{name} must hold {n + 1} non-decreasing entries from 0 to the length of its arrays")
        return o

    def item_estimates_batch(self, pref_offsets, pref_items, pref_vals, cand_offsets, cand_items, capper=None):
        """cms_item_estimates_batch: GenericItemBasedRecommender's
        doEstimatePreference for many users over a table whose owners are
        items.  User u's preferences are pref_items / pref_vals
        [pref_offsets[u]:pref_offsets[u+1]] in PreferenceArray order, its
        candidates cand_items[cand_offsets[u]:cand_offsets[u+1]]; returns one
        float32 estimate per candidate.  capper = (min, max) or None."""
        pi = np.ascontiguousarray(pref_items, np.int64).reshape(-1)
        pv = np.ascontiguousarray(pref_vals, np.float32).reshape(-1)
        ci = np.ascontiguousarray(cand_items, np.int64).reshape(-1)
        n = np.asarray(pref_offsets).size - 1
        po = self._csr("pref_offsets", pref_offsets, n, pi, pv)
        co = self._csr("cand_offsets", cand_offsets, n, ci)
        out = np.zeros(ci.size, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_item_estimates_batch(self._h, n, _ptr(po), _ptr(pi), _ptr(pv), _ptr(co), _ptr(ci),
                                                 int(capper is not None), float(lo), float(hi), _ptr(out)))
        return out

    ITEM_STRATEGIES = {"preferred": 0, "all_unknown": 1}

    def item_recommend_batch(self, user_ids, model_user_ids, pref_offsets, pref_items, pref_vals, how_many,
                             strategy="preferred", include_known=False, capper=None):
        """cms_item_recommend_batch: GenericItemBasedRecommender.recommend for
        every user of user_ids over a table whose owners are the model's
        items.  The DataModel is model_user_ids (ascending) with row r's
        preferences pref_items / pref_vals [pref_offsets[r]:pref_offsets[r+1]].
        strategy: "preferred" (PreferredItemsNeighborhoodCandidateItemsStrategy)
        or "all_unknown".  Returns (counts [n], items [n][how_many], values
        [n][how_many] float32)."""
        us = np.ascontiguousarray(user_ids, np.int64).reshape(-1)
        mu = np.ascontiguousarray(model_user_ids, np.int64).reshape(-1)
        pi = np.ascontiguousarray(pref_items, np.int64).reshape(-1)
        pv = np.ascontiguousarray(pref_vals, np.float32).reshape(-1)
        po = self._csr("pref_offsets", pref_offsets, mu.size, pi, pv)
        if how_many < 1:
            raise ValueError("howMany must be at least 1")
        counts = np.zeros(us.size, np.int32)
        items = np.full((us.size, how_many), -1, np.int64)
        vals = np.full((us.size, how_many), np.nan, np.float32)
        lo, hi = capper if capper is not None else (0.0, 0.0)
        check(self._lib.cms_item_recommend_batch(self._h, us.size, _ptr(us), mu.size, _ptr(mu), _ptr(po), _ptr(pi),
                                                 _ptr(pv), int(self.ITEM_STRATEGIES.get(strategy, strategy)),
                                                 int(how_many), int(bool(include_known)), int(capper is not None),
                                                 float(lo), float(hi), _ptr(counts), _ptr(items), _ptr(vals)))
        return counts, items, vals

    def write_similar_items(self, path, k, as_float=True):
        """cms_top_k_all in FileSimilarItemsWriter's CSV format."""
        check(self._lib.cms_write_similar_items(self._h, os.fsencode(path), int(k), int(as_float)))

    def write_similarities(self, path, k, fmt, threshold=None):
        """cms_write_similarities: fmt 'item_similarity_job' (MR ItemSimilarityJob
        text result) or 'spark_itemsimilarity' (TextDelimitedIndexedDatasetWriter);
        threshold: RowSimilarityJob's --threshold (cms_write_similarities_threshold)."""
        code = {"item_similarity_job": _lib.CMS_FORMAT_ITEM_SIMILARITY_JOB,
                "spark_itemsimilarity": _lib.CMS_FORMAT_SPARK_ITEMSIMILARITY}[fmt]
        if threshold is None:
            check(self._lib.cms_write_similarities(self._h, os.fsencode(path), int(k), code))
        else:
            check(self._lib.cms_write_similarities_threshold(self._h, os.fsencode(path), int(k), code,
                                                             float(threshold)))

    def top_k_all_partial(self, k, shard, nshards):
        n = self.num_owners
        ids = np.zeros((n, k), np.int64)
        sc = np.zeros((n, k), np.float64)
        cnt = np.zeros(n, np.int32)
        check(self._lib.cms_top_k_all_partial(self._h, int(k), int(shard), int(nshards), _ptr(ids), _ptr(sc),
                                              _ptr(cnt)))
        return ids, sc, cnt

    def top_k_merge(self, k, parts):
        """parts: list of (ids, scores, counts) partial lists."""
        n = self.num_owners
        ids = np.ascontiguousarray(np.stack([p[0] for p in parts]), np.int64)
        sc = np.ascontiguousarray(np.stack([p[1] for p in parts]), np.float64)
        cnt = np.ascontiguousarray(np.stack([p[2] for p in parts]), np.int32)
        oi = np.zeros((n, k), np.int64)
        os_ = np.zeros((n, k), np.float64)
        oc = np.zeros(n, np.int32)
        check(self._lib.cms_top_k_merge(self._h, int(k), len(parts), _ptr(ids), _ptr(sc), _ptr(cnt), _ptr(oi),
                                        _ptr(os_), _ptr(oc)))
        return oi, os_, oc

    def top_k_all(self, k):
        """mostSimilar lists of every owner, [num_owners][k] by owner row
        (symmetric streaming all-pairs pass)."""
        n = self.num_owners
        # uninitialised on purpose: the library defines every cell (ID -1 and a
        # NaN score past a row's count)
        ids = np.empty((n, k), np.int64)
        sc = np.empty((n, k), np.float64)
        cnt = np.empty(n, np.int32)
        check(self._lib.cms_top_k_all(self._h, int(k), _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def _device_lists(self, k):
        import torch
        dev = torch.device("cuda", self.device)
        n = self.num_owners
        return (torch.empty((n, k), dtype=torch.int64, device=dev), torch.empty((n, k), dtype=torch.float64, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev))

    def top_k_all_device(self, k):
        """top_k_all(k) with the lists left on the handle's GPU as torch
        tensors (cms_top_k_all_device): (ids [n][k], scores [n][k], counts [n])."""
        out = self._device_lists(k)
        check(self._lib.cms_top_k_all_device(self._h, int(k), *[ctypes.c_void_p(x.data_ptr()) for x in out]))
        return out

    def top_k_refresh_device(self, k):
        """top_k_refresh(k) into device tensors (cms_top_k_refresh_device)."""
        out = self._device_lists(k)
        check(self._lib.cms_top_k_refresh_device(self._h, int(k), *[ctypes.c_void_p(x.data_ptr()) for x in out]))
        return out

    def top_k_refresh(self, k):
        """The same lists as top_k_all(k), recomputing only the pairs with an
        owner touched by COO ingests since the previous refresh (the first
        call runs the whole job and keeps 2k-deep lists on the device)."""
        n = self.num_owners
        ids = np.empty((n, k), np.int64)
        sc = np.empty((n, k), np.float64)
        cnt = np.empty(n, np.int32)
        check(self._lib.cms_top_k_refresh(self._h, int(k), _ptr(ids), _ptr(sc), _ptr(cnt)))
        return ids, sc, cnt

    def refresh_stats(self):
        """(owners touched, lists recomputed whole, whole jobs) of the last refresh."""
        v = [ctypes.c_int64(0) for _ in range(3)]
        check(self._lib.cms_refresh_stats(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def refresh_classes(self):
        """{class: (owners, touched)} of the last refresh's job, classes
        "multi" (multi-limb), "int8" and "fp4" (cms_refresh_classes)."""
        v = (ctypes.c_int64 * 6)()
        check(self._lib.cms_refresh_classes(self._h, v))
        return {c: (int(v[i]), int(v[3 + i])) for i, c in enumerate(("multi", "int8", "fp4"))}

    # -- per-owner shapes (CountMinSketchConfig) --
    @classmethod
    def per_owner_shapes(cls, num_owners, seed=42, weighted=False, device=-1, owner_ids=None, frac_bits=0):
        """A handle whose owners each carry their own (d, w): CosineCM with
        its CountMinSketchConfig (cms_create_per_owner)."""
        return cls(num_owners, seed=seed, weighted=weighted, device=device, owner_ids=owner_ids, per_owner=True,
                   frac_bits=frac_bits)

    def configure_owner_shapes(self, q, num_keys):
        """CountMinSketchConfig(q).configure(dataModel) on the GPU."""
        check(self._lib.cms_configure_owner_shapes(self._h, float(q), int(num_keys)))

    def set_owner_delta_epsilon(self, delta, epsilon):
        de = np.ascontiguousarray(delta, np.float64)
        ep = np.ascontiguousarray(epsilon, np.float64)
        if de.size != self.num_owners or ep.size != self.num_owners:
            raise ValueError("one (delta, epsilon) per owner")
        check(self._lib.cms_set_owner_delta_epsilon(self._h, _ptr(de), _ptr(ep)))

    def owner_shapes(self):
        """(delta, epsilon, width, depth) per owner row."""
        n = self.num_owners
        de, ep = np.zeros(n, np.float64), np.zeros(n, np.float64)
        w, d = np.zeros(n, np.int32), np.zeros(n, np.int32)
        check(self._lib.cms_get_owner_shapes(self._h, _ptr(de), _ptr(ep), _ptr(w), _ptr(d)))
        return de, ep, w, d

    def read_owner_sketch(self, owner_id):
        """getExportedCMProfile(owner_id): [depth][width] fp64."""
        w = ctypes.c_int32()
        d = ctypes.c_int32()
        check(self._lib.cms_read_owner_sketch(self._h, int(owner_id), None, 0, ctypes.byref(w), ctypes.byref(d)))
        out = np.zeros((d.value, w.value), np.float64)
        check(self._lib.cms_read_owner_sketch(self._h, int(owner_id), _ptr(out), out.size, ctypes.byref(w),
                                              ctypes.byref(d)))
        return out

    def read_counters(self, row_begin=0, row_count=None):
        if row_count is None:
            row_count = self.num_owners - row_begin
        out = np.zeros((row_count, self.depth, self.width), np.float64)
        check(self._lib.cms_read_counters(self._h, int(row_begin), int(row_count), _ptr(out)))
        return out

    FORMS = ("u32", "u16", "u8", "u4", "u2", "u1", "list")

    def owner_forms(self, row_begin=0, row_count=None):
        """(form code per owner -- an index into FORMS --, the counter bound
        each narrow form was chosen for) of owners [row_begin, +row_count)
        (cms_owner_forms)."""
        if row_count is None:
            row_count = self.num_owners - row_begin
        form = np.zeros(row_count, np.int32)
        bound = np.zeros(row_count, np.uint32)
        check(self._lib.cms_owner_forms(self._h, int(row_begin), int(row_count), _ptr(form), _ptr(bound)))
        return form, bound

    def read_counters_device(self, row_begin=0, row_count=None, out=None):
        """Counters [row_count][d][w] on the handle's device, in counter units
        (cms_read_counters_device).  The tensor is torch.int32 holding the u32
        bits (torch's integer reductions work on it); a counter at or above
        2^31 reads negative -- use .view(torch.uint32) or mask with 0xFFFFFFFF
        in int64 where such counters can occur."""
        import torch
        if row_count is None:
            row_count = self.num_owners - row_begin
        if out is None:
            out = torch.empty((row_count, self.depth, self.width), dtype=torch.int32,
                              device=torch.device("cuda", self.device))
        if out.device != torch.device("cuda", self.device) or out.element_size() != 4 or not out.is_contiguous():
            raise ValueError("out must be a contiguous 4-byte tensor on cuda:%d" % self.device)
        if out.numel() < row_count * self.depth * self.width:
            raise ValueError("out holds fewer than row_count * depth * width counters")
        check(self._lib.cms_read_counters_device(self._h, int(row_begin), int(row_count), ctypes.c_void_p(out.data_ptr())))
        s = torch.cuda.current_stream(out.device).cuda_stream
        if s:  # later torch work on this stream waits for the copy
            check(self._lib.cms_release_to_stream(self._h, ctypes.c_void_p(s)))
        return out

    # -- checkpoint and restore (DESIGN.md 3 "Checkpoint image") --
    def checkpoint_size(self):
        """Bytes save() would write / save_device() returns (cms_checkpoint_size)."""
        b = ctypes.c_int64()
        check(self._lib.cms_checkpoint_size(self._h, ctypes.byref(b)))
        return int(b.value)

    def save(self, path):
        """The table as a checkpoint file: every row in its stored form
        (cms_save_table; written as path + ".tmp", then renamed)."""
        check(self._lib.cms_save_table(self._h, os.fsencode(path)))

    def load(self, path):
        """A checkpoint file into this (empty) handle; finalize() afterwards
        derives the norms (cms_load_table)."""
        check(self._lib.cms_load_table(self._h, os.fsencode(path)))

    def save_device(self):
        """The checkpoint image as a torch uint8 tensor on the handle's device
        (cms_save_table_device): the same bytes save() writes."""
        import torch
        size = self.checkpoint_size()
        out = torch.empty(size, dtype=torch.uint8, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(out.device).synchronize()  # (the allocation is the tensor's alone)
        b = ctypes.c_int64()
        check(self._lib.cms_save_table_device(self._h, ctypes.c_void_p(out.data_ptr()), size, ctypes.byref(b)))
        return out[:b.value]

    def load_device(self, image):
        """A checkpoint image (uint8 tensor on the handle's device) into this
        (empty) handle (cms_load_table_device)."""
        import torch
        if image.device != torch.device("cuda", self.device) or image.dtype != torch.uint8 or not image.is_contiguous():
            raise ValueError("image must be a contiguous uint8 tensor on cuda:%d" % self.device)
        torch.cuda.current_stream(image.device).synchronize()  # its producers are done
        check(self._lib.cms_load_table_device(self._h, ctypes.c_void_p(image.data_ptr()), int(image.numel())))

    def merge(self, path):
        """A checkpoint file added into this table, counter by counter
        (cms_merge_table): the table of both streams together.  The handle may
        be empty or populated; shape, counter type, hash parameters and owner
        IDs must equal the file's.  A refused merge changes nothing;
        finalize() afterwards re-derives the norms."""
        check(self._lib.cms_merge_table(self._h, os.fsencode(path)))

    def merge_device(self, image):
        """merge() of a checkpoint image (uint8 tensor on the handle's device,
        as save_device() returns it; cms_merge_table_device)."""
        import torch
        if image.device != torch.device("cuda", self.device) or image.dtype != torch.uint8 or not image.is_contiguous():
            raise ValueError("image must be a contiguous uint8 tensor on cuda:%d" % self.device)
        torch.cuda.current_stream(image.device).synchronize()  # its producers are done
        check(self._lib.cms_merge_table_device(self._h, ctypes.c_void_p(image.data_ptr()), int(image.numel())))

    def subtract(self, path):
        """A checkpoint file subtracted from this table, counter by counter
        (cms_subtract_table): the table of the stream that remains, when the
        file's stream is a part of this table's.  u32 counters only; the rules
        of merge() apply, and no row mass and no counter may fall below zero
        (CMS_E_OVERFLOW).  A refused subtraction changes nothing; finalize()
        afterwards re-derives the norms."""
        check(self._lib.cms_subtract_table(self._h, os.fsencode(path)))

    def subtract_device(self, image):
        """subtract() of a checkpoint image (uint8 tensor on the handle's
        device, as save_device() returns it; cms_subtract_table_device)."""
        import torch
        if image.device != torch.device("cuda", self.device) or image.dtype != torch.uint8 or not image.is_contiguous():
            raise ValueError("image must be a contiguous uint8 tensor on cuda:%d" % self.device)
        torch.cuda.current_stream(image.device).synchronize()  # its producers are done
        check(self._lib.cms_subtract_table_device(self._h, ctypes.c_void_p(image.data_ptr()), int(image.numel())))

    def compact(self):
        """Every owner row re-stored in the narrowest form its counters need
        now, and the table laid out anew (cms_compact_table): what merges and
        subtractions widened shrinks back.  No counter, mass or query result
        changes and the handle's state is kept (no finalize() is needed).
        Returns the number of owners whose stored form or place class changed.
        checkpoint.compact_checkpoint is the no-GPU specification."""
        changed = ctypes.c_int64()
        check(self._lib.cms_compact_table(self._h, ctypes.byref(changed)))
        return int(changed.value)

    def fold_size(self, width):
        """Bytes save_folded() would write / fold_device() returns (cms_fold_size)."""
        b = ctypes.c_int64()
        check(self._lib.cms_fold_size(self._h, int(width), ctypes.byref(b)))
        return int(b.value)

    def fold_device(self, width):
        """The checkpoint image of this table folded to `width`, a divisor of
        its own, as a torch uint8 tensor on the handle's device
        (cms_fold_table_device): counter j of every sketch row added into
        counter j mod width, which is the table the same stream builds at that
        width with the same hash parameters.  This handle is only read.  The
        image loads into a handle of the new width and merges into or subtracts
        from a live one; checkpoint.fold_checkpoint is the no-GPU
        specification.  u32 counters only."""
        import torch
        size = self.fold_size(width)
        out = torch.empty(size, dtype=torch.uint8, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(out.device).synchronize()  # (the allocation is the tensor's alone)
        b = ctypes.c_int64()
        check(self._lib.cms_fold_table_device(self._h, int(width), ctypes.c_void_p(out.data_ptr()), size, ctypes.byref(b)))
        return out[:b.value]

    def save_folded(self, path, width):
        """fold_device(width) written to a checkpoint file (cms_fold_table;
        written as path + ".tmp", then renamed)."""
        check(self._lib.cms_fold_table(self._h, int(width), os.fsencode(path)))

    def folded(self, width, device=None, weighted=None):
        """A new SketchTable of width `width` holding this table folded to it
        (fold_device, then load_device), on this handle's device and with its
        weighting unless given.  Not finalized, as after from_checkpoint."""
        import torch
        image = self.fold_device(width)
        device = self.device if device is None else int(device)
        if device != self.device:
            image = image.to(torch.device("cuda", device))
        t = SketchTable(self.num_owners, depth=self.depth, width=int(width), seed=self.seed,
                        weighted=self.weighted if weighted is None else weighted, device=device,
                        frac_bits=self.frac_bits, counters=self.counters)
        try:
            t.load_device(image)
        except Exception:
            t.close()
            raise
        return t

    @classmethod
    def from_checkpoint(cls, path, device=-1, weighted=False):
        """A new handle of the file's shape (cms_checkpoint_info), loaded from it."""
        lib = _lib.load()
        p = _lib.CmsParams()
        check(lib.cms_checkpoint_info(os.fsencode(path), ctypes.byref(p), None))
        t = cls(p.num_owners, depth=p.depth, width=p.width, seed=p.seed, weighted=weighted, device=device,
                frac_bits=p.frac_bits, counters="f64" if p.counter_type == _lib.CMS_COUNTER_F64 else "u32")
        try:
            t.load(path)
        except Exception:
            t.close()
            raise
        return t

    def release_scratch(self):
        """cms_release_scratch: ingest/query scratch and the kept refresh lists
        go back to the allocator (the next refresh is a whole job)."""
        check(self._lib.cms_release_scratch(self._h))

    # -- instrumentation --
    def stats(self):
        s = _lib.CmsStats()
        s.struct_size = ctypes.sizeof(s)
        check(self._lib.cms_get_stats(self._h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def set_timing(self, enabled=True, level=2):
        """HIP-event timing of the library's kernel scopes.  level 1 brackets
        only the roofline kernels (cheap enough for timed steps), level 2 every
        phase scope as well (each event costs the stream a few us)."""
        check(self._lib.cms_set_timing(self._h, int(level) if enabled else 0))

    def timing(self, name):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        check(self._lib.cms_get_timing(self._h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def reset_timing(self):
        check(self._lib.cms_reset_timing(self._h))


def fastidset_to_array(ids):
    """toArray() of a new FastIDSet() after add(ids[i]) in order
    (cms_fastidset_to_array: the library's own FastIDSet, host only)."""
    ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
    out = np.zeros(max(ids.size, 1), np.int64)
    cnt = ctypes.c_int64()
    check(_lib.load().cms_fastidset_to_array(_ptr(ids), ids.size, _ptr(out), ctypes.byref(cnt)))
    return out[:cnt.value]


def shard_of_keys(keys, world):
    """Vectorised cms_shard_of_key (splitmix64 finalizer mod world) for host
    arrays -- used to route a stream's pairs to their rank before ingest."""
    z = np.asarray(keys, np.int64).astype(np.uint64)
    if world <= 1:
        return np.zeros(z.shape, np.int32)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(world)).astype(np.int32)


def java_double_to_string(v):
    """Java Double.toString(v) as the library writes it (cms_format_java_double)."""
    buf = ctypes.create_string_buffer(64)
    n = _lib.load().cms_format_java_double(float(v), buf, 64)
    if n < 0:
        raise ValueError(v)
    return buf.value.decode()
