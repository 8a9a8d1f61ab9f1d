"""Host-side mirror of the reference's plugin surface for the sketch path.

``CosineCM`` keeps the names, argument meaning and error behaviour of
org.apache.mahout.cf.taste.impl.similarity.CosineCM
(T/impl/similarity/CosineCM.java) and of the two plugin interfaces it
serves, UserSimilarity (T/similarity/UserSimilarity.java:31-58) and
ItemSimilarity (T/similarity/ItemSimilarity.java:31-64); every similarity
is computed by libmahout_cms.so on the GPU.

Shape: the reference sizes each owner's sketch from CountMinSketchConfig's
(delta, epsilon) (CosineCM.java:63,86).  ``CountMinSketchConfig`` keeps that
per-owner mode (u1 hashed at u2's shape on the GPU).  The fixed-shape configs of this
path (d, w for every owner) are expressed by ``FixedShapeConfig``, whose
getDelta/getEpsilon return exp(-d) and e/w -- the subclass override the
reference allows (CountMinSketchConfig.getDelta/getEpsilon are public,
non-final) -- and the shape actually used is the one
AbstractCountMinSketch(delta, epsilon) derives from them.
"""
import math

import numpy as np

from . import _lib
from .datamodel import GenericDataModel, NoSuchUserException, preference_delta
from .sketch import SketchTable, frac_bits_for, shape_from_delta_epsilon


class TasteException(Exception):
    """org.apache.mahout.cf.taste.common.TasteException"""


class NoSuchItemException(TasteException, KeyError):
    """org.apache.mahout.cf.taste.common.NoSuchItemException"""


class Weighting:
    UNWEIGHTED = "UNWEIGHTED"
    WEIGHTED = "WEIGHTED"


class HashFunctionBuilder:
    """HashFunctionBuilder(long seed) (T/impl/common/HashFunctionBuilder.java:23-29)."""

    def __init__(self, seed):
        self.seed = int(seed)


class FixedShapeConfig:
    """Every owner gets the same (depth, width)."""

    def __init__(self, depth, width):
        self.depth = int(depth)
        self.width = int(width)

    def getDelta(self, owner_id=None):
        return math.exp(-float(self.depth))

    def getEpsilon(self, owner_id=None):
        return math.e / float(self.width)

    def shape(self):
        """(width, depth) that new DoubleCountMinSketch(delta, epsilon, ...) builds."""
        return shape_from_delta_epsilon(self.getDelta(), self.getEpsilon())


class CountMinSketchConfig:
    """CountMinSketchConfig(q) (T/impl/common/CountMinSketchConfig.java:57-60):
    per-owner (delta, epsilon) chosen by the Fmeasure search.  configure()
    runs computeConfig (:120-158) on the GPU when the CosineCM that owns the
    data is built; setConfig() takes (delta, epsilon) arrays computed
    elsewhere (the ser/ cache of :74-95 in the reference).  getDelta /
    getEpsilon before configuration raise TasteException, as :230-251 do."""

    def __init__(self, q):
        self.q = float(q)
        self._explicit = None
        self._result = None  # (owner ids, delta, epsilon) once configured

    def setConfig(self, delta, epsilon):
        self._explicit = (np.asarray(delta, np.float64), np.asarray(epsilon, np.float64))

    def _configure(self, table, dataModel):
        if self._explicit is not None:
            table.set_owner_delta_epsilon(*self._explicit)
        else:
            table.configure_owner_shapes(self.q, dataModel.getNumItems())
        de, ep, _, _ = table.owner_shapes()
        self._result = (dataModel.getUserIDs(), de, ep)

    def _lookup(self, arr, userID):
        if self._result is None:
            raise TasteException("delta is null, call configure method first")
        ids = self._result[0]
        i = np.searchsorted(ids, userID)
        return float(arr[i]) if i < ids.size and ids[i] == userID else 0.0  # trove: missing key -> 0.0

    def getDelta(self, userID):
        return self._lookup(self._result[1] if self._result else None, userID)

    def getEpsilon(self, userID):
        return self._lookup(self._result[2] if self._result else None, userID)


def counter_units(offsets, values):
    """(frac_bits, counters) for a DataModel: exact u32 counters in units of
    2^-frac_bits when every preference is a non-negative multiple of
    2^-frac_bits and every owner's total stays below 2^32 such units (the
    integer fast paths, bit-identical similarities); otherwise
    DoubleCountMinSketch's own fp64 counters, filled in DataModel order."""
    if values is None:
        return 0, "u32"
    v = np.asarray(values, np.float32)
    if v.size and (not np.all(np.isfinite(v)) or (v < 0).any()):
        return 0, "f64"
    try:
        fb = frac_bits_for(v)
    except ValueError:
        return 0, "f64"
    off = np.asarray(offsets, np.int64)
    if v.size:
        mass = np.add.reduceat(np.ldexp(v.astype(np.float64), fb), off[:-1].clip(max=v.size - 1))
        mass[off[1:] == off[:-1]] = 0.0
        if (mass >= 2.0 ** 32).any():
            return 0, "f64"
    return fb, "u32"


def _map_error(e, owner_kind="user"):
    if e.code == _lib.CMS_E_NO_SUCH_ID:
        return NoSuchUserException(str(e)) if owner_kind == "user" else NoSuchItemException(str(e))
    if e.code in (_lib.CMS_E_PARAM, _lib.CMS_E_SHAPE):
        return ValueError(str(e))  # IllegalArgumentException
    return TasteException(str(e))


class PlusAnonymousUserDataModel:
    """PlusAnonymousUserDataModel(delegate)
    (T/impl/model/PlusAnonymousUserDataModel.java:74-137): the delegate's
    users plus one temporary user, TEMP_USER_ID, whose preferences are set
    for the length of a request -- recommender.recommend(TEMP_USER_ID, n)
    then serves a user the model does not hold.  Over such a model CosineCM
    keeps the delegate's sketch table and answers for TEMP_USER_ID with the
    anonymous-profile calls (SketchTable.anonymous_*); the temporary
    preferences take the table's own frac_bits scaling, and values it cannot
    hold raise TasteException."""

    TEMP_USER_ID = -2 ** 63  # Long.MIN_VALUE

    def __init__(self, delegate):
        self._delegate = delegate
        self._temp = None  # (item IDs, float32 values) as given

    def getDelegate(self):
        return self._delegate

    def setTempPrefs(self, itemIDs, values):
        keys = np.ascontiguousarray(itemIDs, np.int64).reshape(-1)
        vals = np.ascontiguousarray(values, np.float32).reshape(-1)
        if keys.size == 0 or keys.size != vals.size:
            raise ValueError("prefs is null or empty")
        self._temp = (keys, vals)

    def clearTempPrefs(self):
        self._temp = None

    def _temp_prefs(self):
        if self._temp is None:
            raise NoSuchUserException(self.TEMP_USER_ID)
        return self._temp

    def getUserIDs(self):
        ids = self._delegate.getUserIDs()
        if self._temp is None:
            return ids
        return np.concatenate([np.array([self.TEMP_USER_ID], np.int64), np.asarray(ids, np.int64)])

    def getPreferencesFromUser(self, user_id):
        if user_id == self.TEMP_USER_ID:
            return self._temp_prefs()
        return self._delegate.getPreferencesFromUser(user_id)

    def getItemIDsFromUser(self, user_id):
        if user_id == self.TEMP_USER_ID:
            return self._temp_prefs()[0]
        return self._delegate.getPreferencesFromUser(user_id)[0]

    def getPreferenceValue(self, user_id, item_id):
        if user_id == self.TEMP_USER_ID:
            keys, vals = self._temp_prefs()
            hit = np.nonzero(keys == item_id)[0]
            return float(vals[hit[0]]) if hit.size else None
        return self._delegate.getPreferenceValue(user_id, item_id)

    def getItemIDs(self):
        return self._delegate.getItemIDs()

    def getNumItems(self):
        return self._delegate.getNumItems()

    def getNumUsers(self):
        return self._delegate.getNumUsers() + (0 if self._temp is None else 1)

    def hasPreferenceValues(self):
        return self._delegate.hasPreferenceValues()

    def getMinPreference(self):
        return self._delegate.getMinPreference()

    def getMaxPreference(self):
        return self._delegate.getMaxPreference()


class CosineCM:
    """CosineCM(DataModel, [Weighting,] CountMinSketchConfig, HashFunctionBuilder).

    Owners are the DataModel's users (sketches keyed by item ID).  Over a
    transposed DataModel the owners are items and userSimilarity /
    itemSimilarity are the sketch-cosine ItemSimilarity.  Over a
    PlusAnonymousUserDataModel the owners are the delegate's users, and
    TEMP_USER_ID is answered from the temporary preferences.
    """

    def __init__(self, dataModel, conf, hfBuilder, weighting=Weighting.UNWEIGHTED, device=-1, sketches=None,
                 counters=None):
        """sketches: a checkpoint file written by saveSketches(); the sketches
        are loaded from it instead of being built from the DataModel (fixed
        shapes only; the file's shape, owners and counter type must be the
        ones this DataModel and conf would build).  counters="f64" asks for
        DoubleCountMinSketch's own fp64 counters even where the preferences
        would fit exact u32 units (counter_units decides otherwise)."""
        if counters not in (None, "f64"):
            raise ValueError('counters must be None (chosen from the preferences) or "f64"')
        self._counters = counters
        if not dataModel.hasPreferenceValues():  # CosineCM.java:38
            raise ValueError("DataModel doesn't have preference values")
        self._per_owner = isinstance(conf, CountMinSketchConfig)
        if sketches is not None and self._per_owner:
            raise ValueError("sketches= needs a fixed-shape configuration (per-owner shapes keep the DataModel)")
        self._sketches = sketches
        if self._per_owner:
            width = depth = None  # each owner has its own shape
        else:
            width, depth = conf.shape() if hasattr(conf, "shape") else (conf.width, conf.depth)
        # the table holds the delegate's users; the temporary user is sketched per call
        self._anon = dataModel if isinstance(dataModel, PlusAnonymousUserDataModel) else None
        if self._anon is not None:
            dataModel = self._anon.getDelegate()
        self._model = dataModel
        self._conf = conf
        self._hfb = hfBuilder
        self._weighted = weighting == Weighting.WEIGHTED
        self._device = device
        self.depth, self.width = depth, width
        self._inferrer = None
        self._build()

    def _build(self):
        m = self._model
        fb, counters = (0, "f64") if self._counters == "f64" else counter_units(m.offsets, m.values)
        try:
            if self._per_owner:
                self._table = SketchTable(m.getNumUsers(), seed=self._hfb.seed, weighted=self._weighted,
                                          device=self._device, owner_ids=m.getUserIDs(), per_owner=True,
                                          frac_bits=fb, counters=counters)
                self._table.ingest_csr(m.offsets, m.keys, m.values)
                self._conf._configure(self._table, m)
            else:
                self._table = SketchTable(m.getNumUsers(), depth=self.depth, width=self.width, seed=self._hfb.seed,
                                          weighted=self._weighted, device=self._device, owner_ids=m.getUserIDs(),
                                          frac_bits=fb, counters=counters)
                if self._sketches is not None:
                    self._table.load(self._sketches)  # (installs the file's hash parameters and owner IDs)
                else:
                    self._table.ingest_csr(m.offsets, m.keys, m.values)
            self._table.finalize()
        except _lib.CmsError as e:
            raise _map_error(e)
        # what the table was built from (the model's arrays are replaced, never
        # changed in place): refresh() applies the difference to a changed model
        self._built = None if self._sketches is not None or self._per_owner else (
            m.user_ids, m.offsets, m.keys, m.values, fb, counters)

    def setDataModel(self, dataModel):
        """The DataModel the next refresh() reads (the sketches still hold the
        previous one until then)."""
        if not dataModel.hasPreferenceValues():
            raise ValueError("DataModel doesn't have preference values")
        self._anon = dataModel if isinstance(dataModel, PlusAnonymousUserDataModel) else None
        self._model = self._anon.getDelegate() if self._anon is not None else dataModel

    def _refresh_in_place(self):
        """The changed model's difference (datamodel.preference_delta) applied
        to the live table as retract + ingest + finalize: counter for counter
        the table a rebuild gives.  False when the table has to be rebuilt:
        nothing changed since the build, per-owner shapes or fp64 counters, or
        another user-ID universe or counter unit."""
        b, m = self._built, self._model
        if b is None or b[5] != "u32":
            return False
        if m.offsets is b[1] and m.keys is b[2] and m.values is b[3]:
            return False
        if not np.array_equal(m.user_ids, b[0]):
            return False
        fb, counters = counter_units(m.offsets, m.values)
        if counters != "u32" or fb != b[4]:
            return False
        (ru, rk, rv), (au, ak, av) = preference_delta(GenericDataModel.from_csr(b[0], b[1], b[2], b[3]), m)
        try:
            if ru.size:
                self._table.retract(ru, rk, rv)
            if au.size:
                self._table.ingest(au, ak, av)
            self._table.finalize()
        except _lib.CmsError:
            return False  # (the rebuild closes this table)
        self._built = (m.user_ids, m.offsets, m.keys, m.values, fb, counters)
        return True

    @property
    def table(self):
        return self._table

    # ---- the temporary user of a PlusAnonymousUserDataModel ----
    def _is_temp(self, userID):
        return self._anon is not None and userID == PlusAnonymousUserDataModel.TEMP_USER_ID

    def _temp_prefs(self):
        """The temporary preferences (NoSuchUserException when unset)."""
        return self._anon.getPreferencesFromUser(PlusAnonymousUserDataModel.TEMP_USER_ID)

    def anonymousEstimates(self, theNeighborhood, itemIDs, capper=None):
        """doEstimatePreference(TEMP_USER_ID, neighbourhood, item) per item."""
        keys, vals = self._temp_prefs()
        try:
            return self._table.anonymous_estimate_preferences(keys, vals, theNeighborhood, itemIDs, capper)
        except _lib.CmsError as e:
            raise _map_error(e, "user")

    # ---- UserSimilarity ----
    def userSimilarity(self, userID1, userID2):
        try:
            if self._is_temp(userID1) or self._is_temp(userID2):
                other = userID2 if self._is_temp(userID1) else userID1
                if self._is_temp(other):
                    raise ValueError("userSimilarity of the temporary user with itself")
                keys, vals = self._temp_prefs()
                return float(self._table.anonymous_similarities(keys, vals, [other])[0])
            return self._table.similarity(userID1, userID2)
        except _lib.CmsError as e:
            raise _map_error(e, "user")

    def setPreferenceInferrer(self, inferrer):
        if inferrer is None:
            raise ValueError("inferrer is null")
        self._inferrer = inferrer  # unused by the sketch cosine, as in CosineCM

    # ---- ItemSimilarity (owners are items in the transposed orientation) ----
    def itemSimilarity(self, itemID1, itemID2):
        try:
            return self._table.similarity(itemID1, itemID2)
        except _lib.CmsError as e:
            raise _map_error(e, "item")

    def itemSimilarities(self, itemID1, itemID2s):
        try:
            return self._table.similarities(itemID1, itemID2s)
        except _lib.CmsError as e:
            raise _map_error(e, "item")

    def allSimilarItemIDs(self, itemID):
        """AbstractItemSimilarity.allSimilarItemIDs: every owner whose
        similarity is not NaN (T/impl/similarity/AbstractItemSimilarity.java:48-58)."""
        ids = self._model.getUserIDs()
        sims = self.itemSimilarities(itemID, ids)
        return ids[~np.isnan(sims)]

    # ---- recommender-side consumers ----
    def mostSimilarUserIDs(self, userID, howMany):
        """GenericUserBasedRecommender.mostSimilarUserIDs (:119-127) with
        TopItems.getTopUsers (TopItems.java:91-136)."""
        if howMany < 1:
            raise ValueError("howMany must be at least 1")
        try:
            if self._is_temp(userID):
                ids, _, cnt = self._table.anonymous_most_similar([self._temp_prefs()], howMany)
                return ids[0, :int(cnt[0])]
            ids, _ = self._table.most_similar(userID, howMany)
        except _lib.CmsError as e:
            raise _map_error(e, "user")
        return ids

    def nearestNeighborhoods(self, userIDs, n, dataModel):
        """NearestNUserNeighborhood(n).getUserNeighborhood for many users:
        (offsets, neighbour IDs) from one all-owners top-n pass (cms_top_k_all:
        the same lists as mostSimilarUserIDs, each unordered pair scored once)."""
        ids, _, cnt = self._table.top_k_all(n)
        owners = dataModel.getUserIDs()
        users = np.ascontiguousarray(userIDs, np.int64)
        rows = np.searchsorted(owners, users)
        if np.any(rows >= owners.size) or np.any(owners[np.minimum(rows, owners.size - 1)] != users):
            bad = users[(rows >= owners.size) | (owners[np.minimum(rows, owners.size - 1)] != users)][0]
            raise NoSuchUserException(int(bad))
        c = cnt[rows].astype(np.int64)
        off = np.zeros(users.size + 1, np.int64)
        np.cumsum(c, out=off[1:])
        sel = ids[rows]
        nb = sel[np.arange(n)[None, :] < c[:, None]]
        return off, np.ascontiguousarray(nb, np.int64)

    def estimatePreferences(self, theUserID, theNeighborhood, itemIDs, capper=None):
        """doEstimatePreference(user, neighbourhood, item) per item with the
        sketch point query (GenericUserBasedRecommender.java:153-158)."""
        return self._table.estimate_preferences(theUserID, theNeighborhood, itemIDs, capper)

    def recommendBatch(self, userIDs, nb_offsets, neighborIDs, modelCSR, howMany, includeKnownItems=False, capper=None):
        """recommend for many users (cms_recommend_batch) over the DataModel
        modelCSR = (user IDs ascending, offsets, item IDs): (counts, items, values)."""
        mu, po, pi = modelCSR
        return self._table.recommend_batch(userIDs, nb_offsets, neighborIDs, mu, po, pi, howMany, includeKnownItems,
                                           capper)

    def getExportedCMProfileEstimate(self, userID, itemID):
        """DoubleCountMinSketch.get(itemID) on userID's sketch, the point query
        GenericUserBasedRecommender.doEstimatePreference uses (:153-158)."""
        try:
            return self._table.point_query(userID, itemID)
        except _lib.CmsError as e:
            raise _map_error(e, "user")

    def refresh(self, alreadyRefreshed=None):
        """Refreshable.refresh: every sketch is the data model's again.  A
        model that changed since the build (FileDataModel.refresh(), or
        setDataModel) over the same users is applied in place, its removed and
        changed preferences retracted and its new ones ingested; otherwise
        every sketch is rebuilt, as the reference does."""
        if self._refresh_in_place():
            return
        self._table.close()
        self._sketches = None  # (a refresh reads the DataModel, as the reference's does)
        self._build()

    def saveSketches(self, path):
        """Every owner's sketch as one checkpoint file (SketchTable.save);
        CosineCM(..., sketches=path) loads it instead of ingesting."""
        if self._per_owner:
            raise ValueError("saveSketches needs a fixed-shape configuration")
        try:
            self._table.save(path)
        except _lib.CmsError as e:
            raise _map_error(e)

    def compactSketches(self):
        """Every sketch re-stored in the narrowest form its counters need now
        (SketchTable.compact): what in-place refreshes widened shrinks back.
        No similarity or estimate changes.  Returns the owners re-stored."""
        try:
            return self._table.compact()
        except _lib.CmsError as e:
            raise _map_error(e)

    def close(self):
        self._table.close()


class CosineSimilarity:
    """CosineSimilarity(DataModel[, Weighting]) (T/impl/similarity/CosineSimilarity.java:32-103):
    the full-norm cosine over the raw preferences, the quantity CosineCM's
    sketch cosine approximates, computed on the GPU (cms_exact_*) with the
    reference's values bit for bit.

    Owners are the DataModel's users.  Over a transposed DataModel the owners
    are items and itemSimilarity / itemSimilarities / allSimilarItemIDs are
    this cosine between their rating vectors, in the sense in which CosineCM
    offers them.  The object owns a minimal handle whose sketch table is never
    ingested; only the attached model is used."""

    def __init__(self, dataModel, weighting=Weighting.UNWEIGHTED, device=-1):
        if not dataModel.hasPreferenceValues():  # CosineSimilarity.java:41
            raise ValueError("DataModel doesn't have preference values")
        self._model = dataModel
        self._table = SketchTable(dataModel.getNumUsers(), depth=1, width=32, weighted=weighting == Weighting.WEIGHTED,
                                  device=device, owner_ids=dataModel.getUserIDs())
        try:
            self._table.attach_exact(dataModel)
        except _lib.CmsError as e:
            self._table.close()
            raise _map_error(e)

    @property
    def table(self):
        return self._table

    def userSimilarity(self, userID1, userID2):
        try:
            return float(self._table.exact_similarities(userID1, [userID2])[0])
        except _lib.CmsError as e:
            raise _map_error(e, "user")

    def userSimilarities(self, userID1, userID2s):
        try:
            return self._table.exact_similarities(userID1, userID2s)
        except _lib.CmsError as e:
            raise _map_error(e, "user")

    def itemSimilarity(self, itemID1, itemID2):
        try:
            return float(self._table.exact_similarities(itemID1, [itemID2])[0])
        except _lib.CmsError as e:
            raise _map_error(e, "item")

    def itemSimilarities(self, itemID1, itemID2s):
        try:
            return self._table.exact_similarities(itemID1, itemID2s)
        except _lib.CmsError as e:
            raise _map_error(e, "item")

    def allSimilarItemIDs(self, itemID):
        """AbstractItemSimilarity.allSimilarItemIDs: every owner whose
        similarity is not NaN (T/impl/similarity/AbstractItemSimilarity.java:48-58)."""
        ids = self._model.getUserIDs()
        sims = self.itemSimilarities(itemID, ids)
        return ids[~np.isnan(sims)]

    def mostSimilarUserIDs(self, userID, howMany):
        """GenericUserBasedRecommender.mostSimilarUserIDs (:119-127) with
        TopItems.getTopUsers (TopItems.java:91-136)."""
        if howMany < 1:
            raise ValueError("howMany must be at least 1")
        try:
            ids, _ = self._table.exact_most_similar(userID, howMany)
        except _lib.CmsError as e:
            raise _map_error(e, "user")
        return ids

    def nearestNeighborhoods(self, userIDs, n, dataModel):
        """NearestNUserNeighborhood(n).getUserNeighborhood for many users:
        (offsets, neighbour IDs), the lists of exact_top_k_rows over the
        users' owner rows (the same lists as mostSimilarUserIDs)."""
        users = np.ascontiguousarray(userIDs, np.int64).reshape(-1)
        try:
            ids, _, cnt = self._table.exact_top_k_rows(self._table.owner_rows(users), n)
        except _lib.CmsError as e:
            raise _map_error(e, "user")
        c = cnt.astype(np.int64)
        off = np.zeros(users.size + 1, np.int64)
        np.cumsum(c, out=off[1:])
        return off, np.ascontiguousarray(ids[np.arange(n)[None, :] < c[:, None]], np.int64)

    def estimatePreferences(self, theUserID, theNeighborhood, itemIDs, capper=None):
        """doEstimatePreference(user, neighbourhood, item) per item with the
        DataModel's own preference values (GenericUserBasedRecommender.java:159-161)."""
        return self._table.exact_estimate_preferences(theUserID, theNeighborhood, itemIDs, capper)

    def recommendBatch(self, userIDs, nb_offsets, neighborIDs, modelCSR, howMany, includeKnownItems=False, capper=None):
        """recommend for many users (cms_exact_recommend_batch): the attached
        model is the DataModel, modelCSR is not read.  (counts, items, values)."""
        return self._table.exact_recommend_batch(userIDs, nb_offsets, neighborIDs, howMany, includeKnownItems, capper)

    def refresh(self, alreadyRefreshed=None):
        """Refreshable.refresh: the attached model is the DataModel's again."""
        try:
            self._table.attach_exact(self._model)
        except _lib.CmsError as e:
            raise _map_error(e)

    def close(self):
        self._table.close()


class NearestNUserNeighborhood:
    """NearestNUserNeighborhood(n, similarity, model): the n most similar
    users (T/impl/neighborhood/NearestNUserNeighborhood.java) -- TopItems
    .getTopUsers with minSimilarity -inf and sampling rate 1, i.e. the same
    order as mostSimilarUserIDs."""

    def __init__(self, n, userSimilarity, dataModel):
        if n < 1:
            raise ValueError("n must be at least 1")
        self.n = n
        self._sim = userSimilarity
        self._model = dataModel

    def getUserNeighborhood(self, userID):
        return self._sim.mostSimilarUserIDs(userID, self.n)

    def getUserNeighborhoods(self, userIDs):
        """getUserNeighborhood for many users: (offsets, neighbour IDs), the
        same lists as mostSimilarUserIDs, from the similarity's one device
        pass (CosineCM: cms_top_k_all; CosineSimilarity: cms_exact_top_k_rows)."""
        return self._sim.nearestNeighborhoods(userIDs, self.n, self._model)


class ThresholdUserNeighborhood:
    """ThresholdUserNeighborhood(threshold, similarity, model[, samplingRate]):
    every other user whose similarity is not NaN and at least the threshold
    (T/impl/neighborhood/ThresholdUserNeighborhood.java:77-97), in the order
    the reference returns them: toArray() of the FastIDSet the users were added
    to in getUserIDs() order.  One device selection per call
    (SketchTable.threshold_neighbors) instead of a userSimilarity per pair."""

    def __init__(self, threshold, userSimilarity, dataModel, samplingRate=1.0):
        if userSimilarity is None or dataModel is None:
            raise ValueError("userSimilarity or dataModel is null")
        if np.isnan(threshold):
            raise ValueError("threshold must not be NaN")
        if not samplingRate == 1.0:
            # the reference samples users with its own random generator
            # (SamplingLongPrimitiveIterator); a rate below 1 has no defined
            # answer to reproduce, and rates outside (0, 1] it refuses itself
            raise ValueError("samplingRate must be 1.0: the reference's random user sampling is not reproduced")
        self.threshold = float(threshold)
        self._sim = userSimilarity
        self._model = dataModel

    def _lists(self, userIDs):
        try:
            off, ids, _ = self._sim.table.threshold_neighbors(userIDs, self.threshold, order="fastidset", scores=False)
        except _lib.CmsError as e:
            raise _map_error(e, "user")
        return off, ids

    def getUserNeighborhood(self, userID):
        if userID == PlusAnonymousUserDataModel.TEMP_USER_ID and isinstance(self._model, PlusAnonymousUserDataModel):
            # the temporary user is no row of the table: its similarities with
            # every owner, then the reference's loop on the host
            keys, vals = self._model.getPreferencesFromUser(userID)
            owners = np.asarray(self._model.getDelegate().getUserIDs(), np.int64)
            try:
                sims = self._sim.table.anonymous_similarities(keys, vals, owners)
            except _lib.CmsError as e:
                raise _map_error(e, "user")
            keep = FastIDSet()
            for o in owners[~np.isnan(sims) & (sims >= self.threshold)].tolist():
                keep.add(o)
            return np.array(keep.toList(), np.int64)
        return self._lists([userID])[1]

    def getUserNeighborhoods(self, userIDs):
        """getUserNeighborhood for many users: (offsets, neighbour IDs), each
        list in FastIDSet order (one cms_threshold_neighbors call)."""
        return self._lists(np.ascontiguousarray(userIDs, np.int64))


class GenericUserBasedRecommender:
    """GenericUserBasedRecommender(model, neighborhood, similarity)
    (T/impl/recommender/GenericUserBasedRecommender.java:108-116, 134-184):
    with a CosineCM the estimate path with the sketch point query, with a
    CosineSimilarity the one over the DataModel's own values (sim == null),
    capped by EstimatedPreferenceCapper when the model has min/max (:209-216).
    The similarity serves the neighbourhoods, the estimates and the batch
    recommend (nearestNeighborhoods, estimatePreferences, recommendBatch)."""

    def __init__(self, dataModel, neighborhood, similarity):
        self._model = dataModel
        self._nb = neighborhood
        self._sim = similarity
        lo, hi = dataModel.getMinPreference(), dataModel.getMaxPreference()
        self._capper = None if (np.isnan(lo) and np.isnan(hi)) else (lo, hi)

    def estimatePreference(self, userID, itemID):
        actual = self._model.getPreferenceValue(userID, itemID)
        if actual is not None:
            return np.float32(actual)
        return self.doEstimatePreferences(userID, self._nb.getUserNeighborhood(userID), [itemID])[0]

    def doEstimatePreferences(self, theUserID, theNeighborhood, itemIDs):
        """doEstimatePreference for many items at once (one GPU launch)."""
        if len(theNeighborhood) == 0:
            return np.full(len(itemIDs), np.nan, np.float32)
        if theUserID == PlusAnonymousUserDataModel.TEMP_USER_ID and isinstance(self._model, PlusAnonymousUserDataModel):
            return self._sim.anonymousEstimates(theNeighborhood, itemIDs, self._capper)
        try:
            return self._sim.estimatePreferences(theUserID, theNeighborhood, itemIDs, self._capper)
        except _lib.CmsError as e:
            raise _map_error(e, "user")

    def getAllOtherItems(self, theNeighborhood, theUserID, includeKnownItems=False):
        """getAllOtherItems (GenericUserBasedRecommender.java:187-198): the
        neighbours' items as a FastIDSet, the user's own removed."""
        possible = FastIDSet()
        for u in theNeighborhood:
            possible.addAll(self._item_set(u))
        if not includeKnownItems:
            possible.removeAll(self._item_set(theUserID))
        return possible

    def _item_set(self, userID):
        """GenericDataModel.getItemIDsFromUser (GenericDataModel.java:219-227)."""
        keys, _ = self._model.getPreferencesFromUser(userID)
        s = FastIDSet(len(keys))
        for k in keys.tolist():
            s.add(k)
        return s

    def _model_csr(self):
        """The DataModel as (user IDs ascending, offsets, item IDs in
        getPreferencesFromUser order), built once."""
        if getattr(self, "_csr", None) is None:
            m = self._model
            if all(hasattr(m, a) for a in ("user_ids", "offsets", "keys")):
                self._csr = (m.user_ids, m.offsets, m.keys)
            else:
                uids = np.asarray(m.getUserIDs(), np.int64)
                parts = [np.asarray(m.getPreferencesFromUser(int(u))[0], np.int64) for u in uids]
                off = np.zeros(uids.size + 1, np.int64)
                np.cumsum([p.size for p in parts], out=off[1:])
                self._csr = (uids, off, np.concatenate(parts) if parts else np.zeros(0, np.int64))
        return self._csr

    def recommend_all(self, userIDs, howMany, includeKnownItems=False):
        """recommend(userID, howMany) for every user of userIDs in one native
        call (cms_recommend_batch, or cms_exact_recommend_batch over a
        CosineSimilarity): the neighbourhoods from one device pass, the
        candidates in FastIDSet order and TopItems.getTopItems on the host
        side of the library, every estimate in one device batch.
        Returns one [(itemID, float value)] list per user, equal to recommend()."""
        if howMany < 1:
            raise ValueError("howMany must be at least 1")
        users = np.ascontiguousarray(userIDs, np.int64)
        nb_off, nb = self._nb.getUserNeighborhoods(users)
        try:
            cnt, items, vals = self._sim.recommendBatch(users, nb_off, nb, self._model_csr(), howMany,
                                                        includeKnownItems, self._capper)
        except _lib.CmsError as e:
            raise _map_error(e, "user")
        return [[(int(items[u, j]), vals[u, j]) for j in range(int(cnt[u]))] for u in range(users.size)]

    def recommend(self, userID, howMany, includeKnownItems=False):
        """recommend(userID, howMany) (GenericUserBasedRecommender.java:84-105):
        the neighbourhood, the candidate items in FastIDSet iteration order,
        their estimates (one GPU call), then TopItems.getTopItems
        (TopItems.java:47-88) -- a JDK PriorityQueue under the reversed
        ByValueRecommendedItemComparator and a stable sort, so tied values
        come out in the reference's order.  [(itemID, float value)]."""
        if howMany < 1:
            raise ValueError("howMany must be at least 1")
        nb = self._nb.getUserNeighborhood(userID)
        if len(nb) == 0:
            return []
        items = self.getAllOtherItems(nb, userID, includeKnownItems).toList()
        est = self.doEstimatePreferences(userID, nb, items) if items else np.zeros(0, np.float32)
        return get_top_items(howMany, items, est)


# ---- the item-based recommender ------------------------------------------------

def build_capper(dataModel):
    """GenericItemBasedRecommender.buildCapper (:271-278): no capper when the
    model's min and max preference are both NaN, else (min, max) as floats."""
    lo, hi = np.float32(dataModel.getMinPreference()), np.float32(dataModel.getMaxPreference())
    return None if (np.isnan(lo) and np.isnan(hi)) else (float(lo), float(hi))


def item_estimate(sims, prefs, capper=None):
    """GenericItemBasedRecommender.doEstimatePreference (:231-259) restated:
    sims[i] = itemSimilarity(candidate, the user's i-th item), prefs[i] that
    item's float value.  NaN similarities are skipped; preference += sim *
    pref and total += sim in order (fp64); fewer than two points give NaN;
    (float)(preference / total), then the capper.  np.float32."""
    preference = np.float64(0.0)
    total = np.float64(0.0)
    count = 0
    for s, p in zip(np.asarray(sims, np.float64).tolist(), np.asarray(prefs, np.float32).tolist()):
        if s != s:
            continue
        preference = preference + np.float64(s) * np.float64(p)
        total = total + np.float64(s)
        count += 1
    if count <= 1:
        return np.float32(np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.float32(preference / total)
    if capper is not None:  # EstimatedPreferenceCapper.capEstimate
        lo, hi = np.float32(capper[0]), np.float32(capper[1])
        if e > hi:
            e = hi
        elif e < lo:
            e = lo
    return e


class FullRunningAverage:
    """T/impl/common/FullRunningAverage.java:30-55: NaN until the first datum,
    then average * (count - 1) / count + datum / count."""

    def __init__(self):
        self.count = 0
        self.average = float("nan")

    def addDatum(self, datum):
        self.count += 1
        if self.count == 1:
            self.average = float(datum)
        else:
            c = float(self.count)
            self.average = self.average * float(self.count - 1) / c + float(datum) / c

    def getAverage(self):
        return self.average

    def getCount(self):
        return self.count


def multi_most_similar_estimate(similarities, excludeItemIfNotSimilarToAll=True):
    """MultiMostSimilarEstimator.estimate (:334-354) with no rescorer:
    similarities = itemSimilarities(candidate, toItemIDs).  NaN enters the
    average when excludeItemIfNotSimilarToAll (and makes it NaN); an average
    of 0 becomes NaN."""
    avg = FullRunningAverage()
    for s in np.asarray(similarities, np.float64).tolist():
        if excludeItemIfNotSimilarToAll or s == s:
            avg.addDatum(s)
    a = avg.getAverage()
    return float("nan") if a == 0 else a


class _CandidateItemsStrategy:
    """AbstractCandidateItemsStrategy (T/impl/recommender/AbstractCandidateItemsStrategy.java):
    both strategy interfaces over doGetCandidateItems."""

    native = None  # cms_item_recommend_batch's strategy number

    def __init__(self):
        self._side = None  # (the model's arrays, its transposed model)

    def _item_side(self, dataModel):
        """getPreferencesForItem's view of a GenericDataModel: its transpose, kept per model."""
        key = (dataModel.offsets, dataModel.keys)
        if self._side is None or self._side[0][0] is not key[0] or self._side[0][1] is not key[1]:
            self._side = (key, dataModel.transposed())
        return self._side[1]

    def getCandidateItems(self, *args):
        """(userID, preferencesFromUser, dataModel, includeKnownItems) for
        recommend, (itemIDs, dataModel) for mostSimilarItems."""
        if len(args) == 2:
            return self.doGetCandidateItems(args[0], args[1], False)
        _, prefs, dataModel, includeKnownItems = args
        return self.doGetCandidateItems(prefs[0], dataModel, includeKnownItems)

    def refresh(self, alreadyRefreshed=None):
        pass


class PreferredItemsNeighborhoodCandidateItemsStrategy(_CandidateItemsStrategy):
    """Every item of every user who holds one of the preferred items
    (T/impl/recommender/PreferredItemsNeighborhoodCandidateItemsStrategy.java:31-46)."""

    native = 0

    def doGetCandidateItems(self, preferredItemIDs, dataModel, includeKnownItems=False):
        side = self._item_side(dataModel)
        possible = FastIDSet()
        for item in np.asarray(preferredItemIDs, np.int64).tolist():
            try:
                raters, _ = side.getPreferencesFromUser(item)  # getPreferencesForItem: ascending user ID
            except NoSuchUserException:
                raise NoSuchItemException(item)
            for u in raters.tolist():
                keys, _ = dataModel.getPreferencesFromUser(u)
                s = FastIDSet(len(keys))  # getItemIDsFromUser
                for k in keys.tolist():
                    s.add(k)
                possible.addAll(s)
        if not includeKnownItems:
            for item in np.asarray(preferredItemIDs, np.int64).tolist():  # removeAll(long[])
                possible.remove(item)
        return possible


class AllUnknownItemsCandidateItemsStrategy(_CandidateItemsStrategy):
    """Every item of the model but the preferred ones
    (T/impl/recommender/AllUnknownItemsCandidateItemsStrategy.java:28-40)."""

    native = 1

    def doGetCandidateItems(self, preferredItemIDs, dataModel, includeKnownItems=False):
        possible = FastIDSet(dataModel.getNumItems())
        for item in np.asarray(dataModel.getItemIDs(), np.int64).tolist():
            possible.add(item)
        if not includeKnownItems:
            for item in np.asarray(preferredItemIDs, np.int64).tolist():
                possible.remove(item)
        return possible


class GenericItemBasedRecommender:
    """GenericItemBasedRecommender(dataModel, similarity[, candidateItemsStrategy,
    mostSimilarItemsCandidateItemsStrategy]) (T/impl/recommender/
    GenericItemBasedRecommender.java).  dataModel is the user-oriented model,
    similarity an ItemSimilarity -- a CosineCM over dataModel.transposed() puts
    every estimate of a recommend() into one device batch
    (SketchTable.item_recommend_batch / item_estimates_batch /
    similarity_block).  Any other ItemSimilarity, and a CosineCM whose table
    those calls refuse (per-owner shapes, fp64 counters), is served through
    itemSimilarities per candidate and item_estimate on the host."""

    def __init__(self, dataModel, similarity, candidateItemsStrategy=None, mostSimilarItemsCandidateItemsStrategy=None):
        if similarity is None:
            raise ValueError("similarity is null")
        self._model = dataModel
        self._sim = similarity
        self._strategy = candidateItemsStrategy or PreferredItemsNeighborhoodCandidateItemsStrategy()
        self._ms_strategy = mostSimilarItemsCandidateItemsStrategy or PreferredItemsNeighborhoodCandidateItemsStrategy()
        self._capper = build_capper(dataModel)
        self._csr = None

    def getSimilarity(self):
        return self._sim

    def _table(self):
        """The similarity's sketch table when the device calls serve it, else None."""
        s = self._sim
        if isinstance(s, CosineCM) and not s._per_owner and s.table.counters == "u32":
            return s.table
        return None

    def _model_csr(self):
        """(user IDs ascending, offsets, item IDs, float values) in getPreferencesFromUser order, built once."""
        if self._csr is None:
            m = self._model
            if all(hasattr(m, a) for a in ("user_ids", "offsets", "keys", "values")) and m.values is not None:
                self._csr = (m.user_ids, m.offsets, m.keys, m.values)
            else:
                uids = np.asarray(m.getUserIDs(), np.int64)
                parts = [m.getPreferencesFromUser(int(u)) for u in uids]
                off = np.zeros(uids.size + 1, np.int64)
                np.cumsum([len(p[0]) for p in parts], out=off[1:])
                keys = np.concatenate([np.asarray(p[0], np.int64) for p in parts]) if parts else np.zeros(0, np.int64)
                vals = (np.concatenate([np.ones(len(p[0]), np.float32) if p[1] is None else np.asarray(p[1], np.float32)
                                        for p in parts]) if parts else np.zeros(0, np.float32))
                self._csr = (uids, off, keys, vals)
        return self._csr

    def _prefs(self, userID):
        keys, vals = self._model.getPreferencesFromUser(userID)
        vals = np.ones(len(keys), np.float32) if vals is None else np.asarray(vals, np.float32)
        return np.asarray(keys, np.int64), vals

    # ---- estimates ----
    def doEstimatePreferences(self, userID, itemIDs):
        """doEstimatePreference(userID, preferencesFromUser, item) for every item (float32)."""
        keys, vals = self._prefs(userID)
        items = np.ascontiguousarray(itemIDs, np.int64).reshape(-1)
        t = self._table()
        if t is not None:
            try:
                return t.item_estimates_batch([0, keys.size], keys, vals, [0, items.size], items, self._capper)
            except _lib.CmsError as e:
                raise _map_error(e, "item")
        return np.array([item_estimate(self._sim.itemSimilarities(int(i), keys), vals, self._capper)
                         for i in items.tolist()], np.float32).reshape(-1)

    def estimatePreference(self, userID, itemID):
        """The user's own value when the user has the item (:142-149), else the estimate."""
        keys, vals = self._prefs(userID)
        hit = np.nonzero(keys == itemID)[0]
        if hit.size:
            return np.float32(vals[hit[0]])
        return self.doEstimatePreferences(userID, [itemID])[0]

    # ---- recommend ----
    def getAllOtherItems(self, userID, includeKnownItems=False):
        """AbstractRecommender.getAllOtherItems: the candidate strategy's FastIDSet."""
        return self._strategy.getCandidateItems(userID, self._prefs(userID), self._model, includeKnownItems)

    def _native_strategy(self):
        s = self._strategy
        return s.native if isinstance(s, _CandidateItemsStrategy) and self._table() is not None else None

    def recommend(self, userID, howMany, includeKnownItems=False):
        """recommend(userID, howMany, null, includeKnownItems) (:120-139): [(itemID, float32 value)]."""
        return self.recommend_all([userID], howMany, includeKnownItems)[0]

    def recommend_all(self, userIDs, howMany, includeKnownItems=False):
        """recommend() for every user of userIDs: with a device-served CosineCM
        and one of the two built-in strategies, one native call
        (cms_item_recommend_batch); otherwise user by user on the host around
        doEstimatePreferences.  One [(itemID, float32 value)] list per user."""
        if howMany < 1:
            raise ValueError("howMany must be at least 1")
        users = np.ascontiguousarray(userIDs, np.int64).reshape(-1)
        native = self._native_strategy()
        if native is not None:
            mu, po, pi, pv = self._model_csr()
            rows = np.minimum(np.searchsorted(mu, users), max(mu.size - 1, 0))
            bad = mu[rows] != users if mu.size else np.ones(users.size, bool)
            if bad.any():
                raise NoSuchUserException(int(users[bad][0]))
            try:
                cnt, items, vals = self._sim.table.item_recommend_batch(users, mu, po, pi, pv, howMany, native,
                                                                        includeKnownItems, self._capper)
            except _lib.CmsError as e:
                raise _map_error(e, "item")
            return [[(int(items[u, j]), vals[u, j]) for j in range(int(cnt[u]))] for u in range(users.size)]
        out = []
        for u in users.tolist():
            keys, _ = self._prefs(u)
            if keys.size == 0:
                out.append([])
                continue
            items = self.getAllOtherItems(u, includeKnownItems).toList()
            est = self.doEstimatePreferences(u, items) if items else np.zeros(0, np.float32)
            out.append(get_top_items(howMany, items, est))
        return out

    # ---- most similar items ----
    def _block(self, ids1, ids2):
        """itemSimilarity(ids1[i], ids2[j]) as [n1][n2]: one device block, or itemSimilarities per row."""
        t = self._table()
        if t is not None:
            try:
                return t.similarity_block(ids1, ids2)
            except _lib.CmsError as e:
                raise _map_error(e, "item")
        return np.array([self._sim.itemSimilarities(int(a), ids2) for a in ids1], np.float64).reshape(len(ids1), len(ids2))

    def mostSimilarItems(self, itemIDs, howMany, excludeItemIfNotSimilarToAll=True):
        """mostSimilarItems(itemID | itemIDs, howMany[, excludeItemIfNotSimilarToAll])
        (:162-204): one item ranks the candidates by itemSimilarity(itemID, .);
        several by MultiMostSimilarEstimator, the FullRunningAverage of
        itemSimilarities(candidate, itemIDs).  [(itemID, float32 value)]."""
        if howMany < 1:
            raise ValueError("howMany must be at least 1")
        single = np.ndim(itemIDs) == 0
        to = np.ascontiguousarray([itemIDs] if single else itemIDs, np.int64).reshape(-1)
        cands = self._ms_strategy.getCandidateItems(to, self._model).toList()
        if not cands:
            return []
        if single:
            est = self._block(to, cands)[0]
        else:
            est = [multi_most_similar_estimate(row, excludeItemIfNotSimilarToAll) for row in self._block(cands, to)]
        return get_top_items(howMany, cands, est)

    def recommendedBecause(self, userID, itemID, howMany):
        """recommendedBecause (:206-222): the user's other items ranked by
        (1.0 + itemSimilarity(itemID, item)) * preference."""
        if howMany < 1:
            raise ValueError("howMany must be at least 1")
        keys, vals = self._prefs(userID)
        own = FastIDSet(keys.size)
        for k in keys.tolist():
            own.add(k)
        own.remove(itemID)
        items = own.toList()
        if not items:
            return []
        sims = self._block([itemID], items)[0]
        pref = {int(k): float(v) for k, v in zip(keys.tolist(), vals.tolist())}
        est = [(1.0 + float(s)) * pref[i] for i, s in zip(items, sims)]
        return get_top_items(howMany, items, est)

    def refresh(self, alreadyRefreshed=None):
        self._capper = build_capper(self._model)
        self._csr = None


def _is_prime(n):
    """Primality of n < 2^63 (deterministic Miller-Rabin bases)."""
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _next_prime(n):
    """commons-math3 Primes.nextPrime(n): the smallest prime >= n."""
    n = max(n, 2)
    while not _is_prime(n):
        n += 1
    return n


def next_twin_prime(n):
    """RandomUtils.nextTwinPrime (math/.../common/RandomUtils.java:86-98): the
    larger of the first twin-prime pair whose smaller member is >= n."""
    if n > 2147482949:
        raise ValueError(n)
    if n <= 3:
        return 5
    nxt = _next_prime(n)
    while not _is_prime(nxt + 2):
        nxt = _next_prime(nxt + 4)
    return nxt + 2


class FastIDSet:
    """T/impl/common/FastIDSet.java: open addressing with double hashing
    (hash = (int) key & 0x7FFFFFFF, jump = 1 + hash % (size - 2)), REMOVED
    markers, twin-prime table sizes and float load-factor arithmetic -- what
    fixes its iteration order (the order TopItems.getTopItems sees the
    candidates in, hence the order of tied recommendations)."""

    NULL = -(1 << 63)
    REMOVED = (1 << 63) - 1

    def __init__(self, size=2, loadFactor=1.5):
        self.lf = np.float32(loadFactor)
        self.keys = [self.NULL] * next_twin_prime(int(self.lf * np.float32(size)))
        self.numEntries = 0
        self.numSlotsUsed = 0

    def _probe(self, key, for_add):
        h = (key & 0xFFFFFFFF) & 0x7FFFFFFF  # (int) key & 0x7FFFFFFF
        keys = self.keys
        n = len(keys)
        jump = 1 + h % (n - 2)
        index = h % n
        cur = keys[index]
        if not for_add:
            while cur != self.NULL and key != cur:
                index -= jump - n if index < jump else jump
                cur = keys[index]
            return index
        while cur != self.NULL and cur != self.REMOVED and key != cur:
            index -= jump - n if index < jump else jump
            cur = keys[index]
        if cur != self.REMOVED:
            return index
        add_index = index
        while cur != self.NULL and key != cur:
            index -= jump - n if index < jump else jump
            cur = keys[index]
        return index if key == cur else add_index

    def add(self, key):
        key = int(key)
        if np.float32(self.numSlotsUsed) * self.lf >= np.float32(len(self.keys)):
            if np.float32(self.numEntries) * self.lf >= np.float32(self.numSlotsUsed):
                self._rehash(next_twin_prime(int(self.lf * np.float32(len(self.keys)))))
            else:
                self._rehash(next_twin_prime(int(self.lf * np.float32(self.numEntries))))
        index = self._probe(key, True)
        old = self.keys[index]
        if old != key:
            self.keys[index] = key
            self.numEntries += 1
            if old == self.NULL:
                self.numSlotsUsed += 1
            return True
        return False

    def remove(self, key):
        key = int(key)
        if key in (self.NULL, self.REMOVED):
            return False
        index = self._probe(key, False)
        if self.keys[index] == self.NULL:
            return False
        self.keys[index] = self.REMOVED
        self.numEntries -= 1
        return True

    def _rehash(self, new_size):
        old = self.keys
        self.numEntries = 0
        self.numSlotsUsed = 0
        self.keys = [self.NULL] * new_size
        for k in old:
            if k != self.NULL and k != self.REMOVED:
                self.add(k)

    def _live(self):
        return [k for k in self.keys if k != self.NULL and k != self.REMOVED]

    def addAll(self, other):
        changed = False
        for k in other._live():
            changed |= self.add(k)
        return changed

    def removeAll(self, other):
        changed = False
        for k in other._live():
            changed |= self.remove(k)
        return changed

    def toList(self):
        """Iteration order (KeyIterator: table positions, NULL and REMOVED skipped)."""
        return self._live()

    def __len__(self):
        return self.numEntries


def _cmp_by_value_reversed(a, b):
    """Collections.reverseOrder(ByValueRecommendedItemComparator): the queue
    head is the lowest float value (ByValueRecommendedItemComparator.java:37-41)."""
    return -1 if a[1] < b[1] else 1 if a[1] > b[1] else 0


def get_top_items(howMany, itemIDs, estimates):
    """TopItems.getTopItems (TopItems.java:47-88) with no rescorer: a
    PriorityQueue of howMany + 1, items kept while their (double) estimate
    beats the head once full, then the queue's array order stably sorted by
    float value descending.  [(itemID, float32 value)]."""
    q = _JavaPriorityQueue(_cmp_by_value_reversed)
    full = False
    lowest = float("-inf")
    for item, e in zip(itemIDs, estimates):
        pref = float(e)
        if pref != pref or (full and not pref > lowest):
            continue
        q.add((int(item), np.float32(pref)))
        if full:
            q.poll()
        elif len(q) > howMany:
            full = True
            q.poll()
        lowest = float(q.peek()[1])
    out = list(q.q)
    out.sort(key=lambda x: -float(x[1]))  # Collections.sort is stable, as is list.sort
    return out


# ---- the precomputed-similarity consumer ----------------
# GenericItemSimilarity(Iterable<ItemItemSimilarity>) is how Taste consumes
# precomputed item-item similarities (T/impl/similarity/GenericItemSimilarity.java:71-95,
# 172-236); the all-pairs lists of cms_top_k_all / cms_top_k_refresh feed it
# through ``similarities_from_top_k``.

class ItemItemSimilarity:
    """GenericItemSimilarity.ItemItemSimilarity (:251-315): value must lie in
    [-1, 1] (NaN rejected, as Preconditions.checkArgument does, :264-266)."""

    __slots__ = ("itemID1", "itemID2", "value")

    def __init__(self, itemID1, itemID2, value):
        value = float(value)
        if not (-1.0 <= value <= 1.0):
            raise ValueError("Illegal value: %r. Must be: -1.0 <= value <= 1.0" % value)
        self.itemID1 = int(itemID1)
        self.itemID2 = int(itemID2)
        self.value = value

    def getItemID1(self):
        return self.itemID1

    def getItemID2(self):
        return self.itemID2

    def getValue(self):
        return self.value

    def __repr__(self):
        return "ItemItemSimilarity[%d,%d:%r]" % (self.itemID1, self.itemID2, self.value)


def _cmp_item_item(a, b):
    """ItemItemSimilarity.compareTo (:296-300): highest value first."""
    return -1 if a.value > b.value else 1 if a.value < b.value else 0


class _JavaPriorityQueue:
    """java.util.PriorityQueue with a comparator: a binary min-heap with the
    JDK's siftUp / siftDown (offer, poll, peek), so ties leave the queue in
    the same order the reference's does."""

    def __init__(self, cmp):
        self.q = []
        self.cmp = cmp

    def add(self, x):
        q, cmp = self.q, self.cmp
        k = len(q)
        q.append(x)
        while k > 0:  # siftUpUsingComparator
            parent = (k - 1) >> 1
            e = q[parent]
            if cmp(x, e) >= 0:
                break
            q[k] = e
            k = parent
        q[k] = x

    def peek(self):
        return self.q[0]

    def poll(self):
        q, cmp = self.q, self.cmp
        result = q[0]
        x = q.pop()
        n = len(q)
        if n:
            k, half = 0, n >> 1
            while k < half:  # siftDownUsingComparator
                child = 2 * k + 1
                c = q[child]
                right = child + 1
                if right < n and cmp(c, q[right]) > 0:
                    child = right
                    c = q[child]
                if cmp(x, c) <= 0:
                    break
                q[k] = c
                k = child
            q[k] = x
        return result

    def __len__(self):
        return len(self.q)


def get_top_item_item_similarities(howMany, allSimilarities):
    """TopItems.getTopItemItemSimilarities (T/impl/recommender/TopItems.java:145-174):
    a PriorityQueue in reverse compareTo order (lowest value at the head), a
    strict '>' admission once full, then Collections.sort (stable) of the
    queue's array order."""
    import functools
    pq = _JavaPriorityQueue(lambda a, b: -_cmp_item_item(a, b))  # Collections.reverseOrder()
    full = False
    lowest = -math.inf
    for s in allSimilarities:
        v = s.value
        if not math.isnan(v) and (not full or v > lowest):
            pq.add(s)
            if full:
                pq.poll()
            elif len(pq) > howMany:
                full = True
                pq.poll()
            lowest = pq.peek().value
    result = list(pq.q)
    result.sort(key=functools.cmp_to_key(_cmp_item_item))  # stable, as Collections.sort
    return result


class GenericItemSimilarity:
    """org.apache.mahout.cf.taste.impl.similarity.GenericItemSimilarity over
    precomputed similarities: ordered (smaller ID first) pair map where a later
    value wins, a pair of an item with itself skipped (assumed 1.0), and the
    per-item index of similar items (:172-205)."""

    def __init__(self, similarities, maxToKeep=None):
        if maxToKeep is not None:
            similarities = get_top_item_item_similarities(int(maxToKeep), similarities)
        self._maps = {}
        self._index = {}
        for s in similarities:
            a, b = s.itemID1, s.itemID2
            if a == b:
                continue
            lo, hi = (a, b) if a < b else (b, a)
            self._maps.setdefault(lo, {})[hi] = s.value
            self._index.setdefault(lo, set()).add(hi)
            self._index.setdefault(hi, set()).add(lo)

    @classmethod
    def from_similarity(cls, otherSimilarity, itemIDs, maxToKeep=None):
        """GenericItemSimilarity(ItemSimilarity, DataModel[, maxToKeep])
        (:126-160): every pair i < j of the item IDs in ascending order, NaN
        pairs skipped, as DataModelSimilaritiesIterator enumerates them
        (:317-353); one batched itemSimilarities call per item on the GPU."""
        ids = [int(x) for x in sorted(itemIDs)]

        def pairs():
            for i, a in enumerate(ids[:-1]):
                rest = ids[i + 1:]
                vals = otherSimilarity.itemSimilarities(a, rest)
                for b, v in zip(rest, vals):
                    if not math.isnan(v):  # the iterator skips NaN pairs (:341)
                        yield ItemItemSimilarity(a, b, v)
        return cls(pairs(), maxToKeep)

    def itemSimilarity(self, itemID1, itemID2):
        """(:219-236): 1.0 for an item with itself, NaN for a pair never given."""
        if itemID1 == itemID2:
            return 1.0
        lo, hi = (itemID1, itemID2) if itemID1 < itemID2 else (itemID2, itemID1)
        return self._maps.get(lo, {}).get(hi, math.nan)

    def itemSimilarities(self, itemID1, itemID2s):
        return np.array([self.itemSimilarity(itemID1, int(b)) for b in itemID2s], np.float64)

    def allSimilarItemIDs(self, itemID):
        """(:248-251).  The reference returns its FastIDSet's hash order; this
        returns the same IDs in ascending order (order unpinned)."""
        return np.array(sorted(self._index.get(int(itemID), ())), np.int64)

    def refresh(self, alreadyRefreshed=None):
        pass  # (:254-256) does nothing


def similarities_from_top_k(ids, scores, counts, owner_ids=None):
    """ItemItemSimilarity records of the all-pairs lists (cms_top_k_all /
    cms_top_k_refresh: [n][k] partner IDs and scores, counts[n]) in owner order
    then list order -- the iterable GenericItemSimilarity(Iterable) takes."""
    n = len(counts)
    for r in range(n):
        a = int(owner_ids[r]) if owner_ids is not None else r
        for i in range(int(counts[r])):
            yield ItemItemSimilarity(a, int(ids[r, i]), float(scores[r, i]))
