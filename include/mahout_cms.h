/*
 * mahout_cms.h -- C ABI of the MI355X-native count-min-sketch ingest and
 * sketch-cosine similarity path (libmahout_cms.so, gfx950).
 *
 * This is the drop-in boundary for Mahout Taste's CosineCM path.  Every entry
 * point below names the reference interface it replaces; "T/" abbreviates
 * mr/src/main/java/org/apache/mahout/cf/taste/ in jalhajj/mahout.
 *
 * Vocabulary (reference domain terms):
 *   owner  -- the entity a sketch belongs to.  CosineCM sketches a Taste
 *             "user" (T/impl/similarity/CosineCM.java:41-58); over a
 *             transposed DataModel (FileDataModel transpose=true,
 *             T/impl/model/file/FileDataModel.java:166,414-418) the owner is an
 *             item and this path is the sketch-cosine ItemSimilarity.
 *   key    -- the ID hashed into the sketch (the owner's preference IDs).
 *   row    -- dense index of an owner in the sorted owner-ID universe.
 *   depth d / width w -- sketch shape; counters are [d][w] row-major per
 *             owner (T/impl/common/DoubleCountMinSketch.java:62-64).
 *
 * Conventions:
 *   - every function is extern "C", noexcept, and returns int status
 *     (CMS_OK = 0) unless stated; the message of the last failure on the
 *     calling thread is cms_last_error().
 *   - pointers named h_* / plain are HOST memory, copied during the call and
 *     never retained; pointers named d_* are DEVICE memory on the handle's GPU.
 *   - similarity values are the reference's: in [-1, 1] or NaN ("unknown").
 *     NaN is a value, never an error.
 *   - the handle serialises ingest/finalize with an internal mutex; queries
 *     after cms_finalize are reentrant.
 */
#ifndef MAHOUT_CMS_H
#define MAHOUT_CMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMS_ABI_VERSION 2 /* 2: cms_stats leads with struct_size */

/* ---- status codes (mapped to Java exceptions by the JNI shim) ---------- */
#define CMS_OK 0
#define CMS_E_PARAM 1      /* IllegalArgumentException / CMException (AbstractCountMinSketch.java:71-76) */
#define CMS_E_SHAPE 2      /* checkArgument w/d mismatch (DoubleCountMinSketch.java:117-118) */
#define CMS_E_NO_SUCH_ID 3 /* NoSuchUserException / NoSuchItemException (GenericDataModel.java:210-215) */
#define CMS_E_STATE 4      /* call-order violation (query before finalize, ...) */
#define CMS_E_VALUE 5      /* increment not a non-negative multiple of 2^-frac_bits below 2^(32-frac_bits) */
#define CMS_E_OVERFLOW 6   /* a counter could exceed the counter type or fall below zero */
#define CMS_E_HIP 7        /* HIP runtime error */
#define CMS_E_RCCL 8       /* RCCL error */
#define CMS_E_OOM 9        /* device or host allocation failed */
#define CMS_E_SKETCH 10    /* TasteException: CMException inside exportProfile (CosineCM.java:45-46) or no
                              configuration solution (CountMinSketchConfig.java:145-147) */

/* ---- parameters ----------------------------------------------------------- */
#define CMS_COUNTER_U32 0 /* exact integer counters (non-negative integer increments) */
#define CMS_COUNTER_F64 1 /* fp64 counters: DoubleCountMinSketch's own type, any float preference
                             (negative, non-dyadic); increments are applied per owner in ingest
                             order (the DataModel order CosineCM.exportProfile uses) and every sum
                             is the reference's sequential fp64 chain.  Single-GPU; fixed shapes
                             up to width 2^20, and per-owner shapes (cms_create_per_owner);
                             owners are built by CSR ingest or host COO ingest (stable by
                             owner), not by cms_ingest_device_rows. */

#define CMS_UNWEIGHTED 0 /* org.apache.mahout.cf.taste.common.Weighting */
#define CMS_WEIGHTED 1

typedef struct cms_params {
  uint32_t struct_size; /* = sizeof(cms_params); filled by cms_params_init */
  int32_t depth;        /* d, 1..32 (AbstractCountMinSketch.java:34-44 init; bound of this build) */
  int32_t width;        /* w: 1..32768 with CMS_COUNTER_U32, 1..2^20 with CMS_COUNTER_F64 */
  int32_t counter_type; /* CMS_COUNTER_* */
  int64_t seed;         /* HashFunctionBuilder(long seed) (HashFunctionBuilder.java:23) */
  int64_t num_owners;   /* n: rows of the sketch table */
  int32_t weighting;    /* CMS_UNWEIGHTED | CMS_WEIGHTED (CosineCM.java:33) */
  int32_t device;       /* HIP device ordinal; -1 = current device */
  int32_t frac_bits;    /* 0..31: preferences are multiples of 2^-frac_bits (1 for half-star
                           ratings); counters hold pref * 2^frac_bits.  Similarities are
                           scale-invariant bit for bit; point queries / counters read back
                           in preference units.  0 = integer preferences. */
  int32_t flags;        /* CMS_FLAG_* bits (0 = defaults) */
} cms_params;

/* cms_params.flags:
 * CMS_FLAG_COLLECTIVE_SINGLE_RANK -- a one-rank job still takes the multi-rank
 *   data path: cms_comm_init(h, uid, 0, 1) creates a real one-rank RCCL
 *   communicator (and cms_comm_init_transport(h, 0, 1, ...) attaches the
 *   caller's transport), so cms_finalize merges through the packed all-reduce,
 *   later COO batches go through the delta log and its all-gather, and
 *   cms_top_k_all through the collective merge -- each with one participant,
 *   so the results equal the plain single-GPU path bit for bit.  Without the
 *   flag a world of 1 detaches any communicator (the fast single-GPU path).
 *   Not with CMS_COUNTER_F64 (CMS_E_PARAM). */
#define CMS_FLAG_COLLECTIVE_SINGLE_RANK 0x1

typedef struct cms_handle cms_handle;

/* Defaults: d=5, w=4096, u32, seed=42, n=0, unweighted, device -1, frac_bits 0. */
int cms_params_init(cms_params* p);

/* AbstractCountMinSketch(double delta, double epsilon, ...) shape rule
 * (T/impl/common/AbstractCountMinSketch.java:69-83): w = ceil(e/eps),
 * d = ceil(ln(1/delta)); CMS_E_PARAM for the CMException ranges. */
int cms_shape_from_delta_epsilon(double delta, double epsilon, int32_t* width, int32_t* depth);

/* new DoubleCountMinSketch(width, depth, hfBuilder) for every owner at once
 * (T/impl/common/DoubleCountMinSketch.java:32-42) plus the CosineCM instance
 * state (CosineCM.java:26-39).  Counters start at zero.
 *
 * Tunables.  The library reads these environment variables once, here, and
 * never again (a handle's behaviour is fixed at creation); none changes any
 * result, only the storage or kernel a result comes from:
 *   CMS_NO_FORMS=1        narrow rows stay u16 (no 1/2/4/8-bit row forms)
 *   CMS_NO_COMPACT=1      every narrow row keeps a whole u16 slot (no compact row layout)
 *   CMS_NO_VMM=1          the compact row arena as one hipMalloc grown by copying
 *                         (no reserved virtual range mapped in chunks)
 *   CMS_BIT_KEYS=<n>      byte-class owners of <= n keys try 1-bit rows first (64)
 *   CMS_CRUMB_KEYS=<n>    ... of <= n keys 2-bit rows (256)
 *   CMS_LIST_KEYS=<n>     ... of <= n keys, unit increments: sparse list rows (256; 0 = none)
 *   CMS_NO_HOT_ROUTING=1  the COO partition sends every owner through both passes
 *   CMS_NO_FP4=1          no e2m1 operand image: every single-limb pair on int8 MFMA
 *   CMS_NO_MLS=1          multi-limb slabs on the 128-row tile kernel instead of k_cosine_mls
 *   CMS_THRESHOLD_SLAB_ROWS=<rows>  query rows per slab of cms_threshold_neighbors, rounded up to
 *                         whole 128-row tiles (default: the top-k's slab budget)
 *   CMS_EXACT_TILE=<rows> candidate rows per workgroup of the exact cosine's tile kernel, rounded up
 *                         to a multiple of 64 (default and most: 8192, 64 KiB of LDS cells) */
int cms_create(const cms_params* p, cms_handle** out);
void cms_destroy(cms_handle* h);
const char* cms_last_error(void);
int cms_abi_version(void);

/* Owner-ID universe: strictly ascending IDs, row i <-> ids[i] (the order of
 * DataModel.getUserIDs(), GenericDataModel.java:128-134).  Without this call
 * owner IDs are the row indices 0..n-1. */
int cms_set_owner_ids(cms_handle* h, const int64_t* ids, int64_t n);

/* The d hash parameters (a_i, b_i) of HashFunctionBuilder(seed)
 * (HashFunctionBuilder.java:40-61). */
int cms_hash_params(cms_handle* h, int64_t* a, int64_t* b);
/* Install a caller's HashFunctionBuilder parameters instead of the ones
 * drawn from p->seed: (a_i, b_i) = (randomParamA[i], randomParamB[i]) as the
 * builder drew them (HashFunctionBuilder.java:40-61) -- for a builder whose
 * seed is unknown (new HashFunctionBuilder() seeds from the clock).  count
 * must be the handle's depth (CMS_MAX_DEPTH = 32 for a per-owner handle: the
 * rows any owner's shape may use).  Before the first ingest only
 * (CMS_E_STATE otherwise; cms_reset allows it again). */
int cms_set_hash_params(cms_handle* h, const int64_t* a, const int64_t* b, int32_t count);

/* HashFunction.hash(key) for every row i < d, computed on the GPU
 * (HashFunction.java:31-34): out[k*d + i] = h_i(keys[k]). */
int cms_hash_keys(cms_handle* h, const int64_t* keys, int64_t n, int32_t* out);

/* ---- ingest: DoubleCountMinSketch.update(key, inc) for many owners --------
 * (DoubleCountMinSketch.java:72-80; CosineCM.exportProfile :41-58 feeds it the
 * owner's PreferenceArray).  val may be NULL (every increment 1.0, the
 * implicit-feedback stream).  With CMS_COUNTER_U32 every val must be a
 * non-negative integer (CMS_E_VALUE otherwise).  Duplicate (owner, key) pairs
 * ADD, as repeated update() calls do. */

/* COO pairs from host memory, owners by ID. */
int cms_ingest(cms_handle* h, const int64_t* owner, const int64_t* key, const float* val, int64_t n);
/* COO pairs already resident on the device, owners by row index. Asynchronous
 * on the handle's stream (use cms_synchronize).  The handle's stream is a
 * BLOCKING stream: it is ordered after work already queued on the device's
 * legacy default stream and before work queued there later.  Buffers written
 * on any other stream must be complete before the call, and every device
 * input must stay allocated until cms_synchronize (or a blocking call) returns. */
int cms_ingest_device_rows(cms_handle* h, const int64_t* d_row, const int64_t* d_key, const float* d_val,
                           int64_t n);
/* DoubleCountMinSketch.update(key, -val) for pairs that WERE ingested: the table of the
 * remaining stream, counter for counter -- table[owner][i][h_i(key)] -= val * 2^frac_bits
 * for every sketch row i, and the owner's mass falls by the same amount.  What
 * FileDataModel's update files state as removed or changed preferences
 * (FileDataModel.java:493-527), applied to the live table instead of a rebuild.
 * Owners by ID, host memory.
 *   Values: val NULL means 1.0 each; duplicate pairs add; a zero value is a no-op; values
 * are validated exactly as a host ingest validates them (CMS_E_VALUE).  An unknown owner ID
 * is CMS_E_NO_SUCH_ID.  n == 0 returns CMS_OK and changes nothing; a batch holds fewer than
 * 2^31 pairs (CMS_E_PARAM).
 *   States: fixed shape, CMS_COUNTER_U32, no communicator; before or after cms_finalize.
 * CMS_E_STATE for an fp64 handle ((a + b) - b is not a in fp64), a per-owner handle (it keeps
 * the DataModel: a new CSR ingest replaces it) and a handle with a communicator (the delta
 * log is additive).  A pending device-ingest error is reported first, as cms_synchronize would.
 *   Rules, all checked for the whole batch before the first write: for every owner the
 * batch's summed decrement is at most its mass; for every counter (owner, sketch row,
 * bucket) the batch's decrements SUMMED PER COUNTER -- duplicates of a pair, and distinct
 * keys that share a bucket of that row -- are at most the live counter.  Either violation is
 * CMS_E_OVERFLOW, the message naming an offending owner; so is any non-zero batch against an
 * empty handle.  A refused call leaves the handle bit for bit as it was.
 *   A sketch cannot prove that a pair was ever ingested: the rules are NECESSARY, NOT
 * SUFFICIENT.  The result is some stream's table only if the batch is a sub-stream of what
 * was ingested; a batch that merely fits the counters leaves a table no stream built.
 *   On success pairs_ingested falls by n (saturating at 0) and the handle is "ingested, not
 * finalized", as after cms_subtract_table: queries return CMS_E_STATE until cms_finalize
 * re-derives norms and row maxima.  With kept cms_top_k_refresh lists the batch's owners are
 * marked touched: the next refresh is incremental.  Dense rows keep their form and place
 * (nothing narrows or returns to the shared zero row); a live list row that loses entries
 * is rewritten densely first. */
int cms_retract(cms_handle* h, const int64_t* owner, const int64_t* key, const float* val, int64_t n);
/* The same for pairs resident on the device, owners by row index (a row outside
 * [0, num_owners) is CMS_E_PARAM).  BLOCKING and all-or-nothing (unlike
 * cms_ingest_device_rows): the check's verdict is needed before the first write. */
int cms_retract_device_rows(cms_handle* h, const int64_t* d_row, const int64_t* d_key, const float* d_val,
                            int64_t n);
/* CSR from host memory: the owner at row r has keys[offsets[r] .. offsets[r+1])
 * -- the DataModel layout (one PreferenceArray per owner,
 * GenericUserPreferenceArray.java:52-54).  offsets has num_owners+1 entries. */
int cms_ingest_csr(cms_handle* h, const int64_t* offsets, const int64_t* keys, const float* vals);
/* CSR resident on the device.  The offsets are checked on the device before
 * any counter is touched (offsets[0] == 0, non-decreasing; CMS_E_PARAM
 * otherwise), so the build reads keys[0 .. offsets[num_owners]) only; d_keys
 * (and d_vals) must hold that many entries.  Asynchronous after that check.
 *
 * Device ingests are not all-or-nothing for the VALUES (unlike the host
 * ingests, which validate the whole batch first): a pair whose row is outside
 * [0, num_owners) (COO) or whose increment the counter type cannot take is
 * skipped, the others are applied, and the next synchronising call
 * (cms_synchronize / cms_finalize) reports CMS_E_PARAM / CMS_E_VALUE. */
int cms_ingest_csr_device(cms_handle* h, const int64_t* d_offsets, const int64_t* d_keys, const float* d_vals);

/* Forget all counters (next ingest rebuilds the table from zero). */
int cms_reset(cms_handle* h);

/* Return the handle's ingest/query scratch to the device allocator (the
 * table, norms and the all-pairs operands stay).  For 288 GB budgets: a
 * 1M-owner d=5 w=8192 table is 164 GB on its own. */
int cms_release_scratch(cms_handle* h);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ----------------------
 * The interaction stream is sharded by key (user) hash; each rank ingests its
 * shard into a full-shape partial table and cms_finalize sums the tables with
 * RCCL.  Counters are integers, so the merged table is bit-identical for any
 * rank count. */
int cms_comm_unique_id(void* out /* 128 bytes, ncclUniqueId */);
int cms_comm_init(cms_handle* h, const void* unique_id, int32_t rank, int32_t world);
/* The sharding function: rank that owns `key` among `world` ranks. */
int32_t cms_shard_of_key(int64_t key, int32_t world);

/* Merge (RCCL all-reduce when a communicator is attached), then derive the
 * per-(owner,row) norms the cosine needs.  Queries require it.
 * The merge is counter-width adaptive: one all-reduce of (row mass, largest
 * local counter) per owner bounds every merged counter of that owner, and the
 * counters then travel as bit fields of exactly that width packed into u64
 * words whose u64 sums cannot carry between fields -- the merged table is
 * bit-identical to a u32 all-reduce at a fraction of the xGMI bytes. */
int cms_finalize(cms_handle* h);
/* The same merge through a caller-supplied collective instead of RCCL (an MPI,
 * torch.distributed or Spark transport): fn(d_buf, count, user) must replace
 * the count u64 words at device pointer d_buf (on the handle's device; the
 * handle's stream is idle) by their sum over all ranks, and return 0.  It is
 * called a fixed number of times, with identical counts on every rank.  The
 * merged table takes no further ingest until cms_reset (CMS_E_STATE). */
typedef int (*cms_allreduce_fn)(void* d_buf, int64_t count, void* user);
int cms_finalize_with(cms_handle* h, cms_allreduce_fn fn, void* user);
/* A whole multi-rank communicator supplied by the caller instead of RCCL (an
 * MPI, torch.distributed or Spark transport).  After this call the handle
 * behaves exactly as after cms_comm_init: cms_finalize merges through
 * `allreduce` (as cms_finalize_with), later COO batches go into the delta log
 * and the next cms_finalize exchanges the logs through `allgather`, and
 * cms_top_k_all is collective (partial lists gathered through `allgather`,
 * merged exactly).  allgather(d_send, d_recv, bytes, user) must write the
 * `bytes` bytes of every rank's d_send, concatenated in rank order, to d_recv
 * (world * bytes, device memory on the handle's device; the handle's stream
 * is idle during the call) and return 0.  Every rank makes the same sequence
 * of calls with identical sizes.  world == 1 detaches any communicator. */
typedef int (*cms_allgather_fn)(const void* d_send, void* d_recv, int64_t bytes, void* user);
int cms_comm_init_transport(cms_handle* h, int32_t rank, int32_t world, cms_allreduce_fn allreduce,
                            cms_allgather_fn allgather, void* user);
int cms_synchronize(cms_handle* h);
/* Stream ordering without a host wait (stream: a hipStream_t of the handle's
 * device, e.g. the caller's current torch stream; NULL = legacy default).
 * cms_wait_stream: the handle's later work waits for everything queued on
 * `stream` so far (inputs written there are complete before they are read).
 * cms_release_to_stream: later work queued on `stream` waits for the handle's
 * work queued so far (device inputs may then be freed / reused on `stream`). */
int cms_wait_stream(cms_handle* h, void* stream);
int cms_release_to_stream(cms_handle* h, void* stream);

/* ---- queries (after cms_finalize) ---------------------------------------- */

/* CosineCM.userSimilarity(id1, id2) (CosineCM.java:83-96): min over the d rows
 * of the per-row cosine (DoubleCountMinSketch.cosine :114-149), then
 * normalizeWeightResult(r, 1, 0) (AbstractSimilarity.java:313-330).
 * CMS_E_NO_SUCH_ID for unknown owners. */
int cms_similarity(cms_handle* h, int64_t id1, int64_t id2, double* out);
/* ItemSimilarity.itemSimilarities(id1, ids2[]) (ItemSimilarity.java:58) as
 * one batched GPU call. */
int cms_similarities(cms_handle* h, int64_t id1, const int64_t* ids2, int64_t n, double* out);
/* DoubleCountMinSketch.get(key) of owner `id` (DoubleCountMinSketch.java:94-103),
 * the point query GenericUserBasedRecommender uses (:153-158). */
int cms_point_query(cms_handle* h, int64_t id, int64_t key, double* out);
/* GenericUserBasedRecommender.doEstimatePreference(user, neighbourhood, item)
 * with the CosineCM point query (GenericUserBasedRecommender.java:134-184) for
 * q items at once: out[i] is the float estimate for item_keys[i], NaN when
 * fewer than two neighbours carry data.  neighbor_ids is the neighbourhood in
 * the caller's order (NearestNUserNeighborhood order); use_capper applies
 * EstimatedPreferenceCapper(cap_min, cap_max) (:209-216).  The DataModel's own
 * preference short cut of estimatePreference (:108-116) stays with the caller. */
int cms_estimate_preferences(cms_handle* h, int64_t user_id, const int64_t* neighbor_ids, int64_t m,
                             const int64_t* item_keys, int64_t q, int32_t use_capper, float cap_min, float cap_max,
                             float* out);
/* cms_estimate_preferences for n users in one call -- the estimate phase of
 * GenericUserBasedRecommender.recommend (:84-105) for a whole user batch:
 * user u's neighbourhood is neighbor_ids[nb_offsets[u] .. nb_offsets[u+1])
 * (in NearestNUserNeighborhood order) and its candidate items
 * item_keys[item_offsets[u] .. item_offsets[u+1]); out is parallel to
 * item_keys.  Both offset arrays hold n + 1 non-decreasing entries from 0.
 * Every estimate equals the single-user call's (same order of fp64 sums). */
int cms_estimate_preferences_batch(cms_handle* h, int64_t n, const int64_t* user_ids, const int64_t* nb_offsets,
                                   const int64_t* neighbor_ids, const int64_t* item_offsets, const int64_t* item_keys,
                                   int32_t use_capper, float cap_min, float cap_max, float* out);
/* GenericUserBasedRecommender.recommend(userID, how_many) for n users at
 * once (GenericUserBasedRecommender.java:84-105), replacing one
 * Recommender.recommend call per user.  The caller supplies each user's
 * neighbourhood (nb_offsets / neighbor_ids: IDs in NearestNUserNeighborhood
 * order, e.g. from cms_top_k_all) and the DataModel's item IDs per user
 * (model_user_ids ascending; row r's items pref_items[pref_offsets[r] ..
 * pref_offsets[r + 1]) in getPreferencesFromUser order).  Per user: the
 * candidates are getAllOtherItems (:187-198) in FastIDSet iteration order,
 * their estimates come from one cms_estimate_preferences_batch over all
 * users, and the list is TopItems.getTopItems (TopItems.java:47-88) with the
 * JDK PriorityQueue's order for ties.  out_counts[n] (<= how_many, 0 for an
 * empty neighbourhood), out_items / out_values [n][how_many] (float values,
 * as RecommendedItem.getValue()).  A user or neighbour missing from the model
 * is CMS_E_NO_SUCH_ID (NoSuchUserException). */
int cms_recommend_batch(cms_handle* h, int64_t n, const int64_t* user_ids, const int64_t* nb_offsets,
                        const int64_t* neighbor_ids, int64_t n_model_users, const int64_t* model_user_ids,
                        const int64_t* pref_offsets, const int64_t* pref_items, int32_t how_many,
                        int32_t include_known, int32_t use_capper, float cap_min, float cap_max, int32_t* out_counts,
                        int64_t* out_items, float* out_values);

/* ---- item-based recommender: blocks of the similarity matrix -------------
 * Fixed-shape u32 handles, after cms_finalize; a per-owner-shape or fp64
 * handle is CMS_E_STATE.  The calls read the table as cms_similarities does
 * (concurrent readers, nothing is changed).  With timing on they run on the
 * handle's stream under the scopes "item_block" / "item_estimate".
 *
 * out[i * n2 + j] = userSimilarity(ids1[i], ids2[j]): row i equals
 * cms_similarities(h, ids1[i], ids2, n2, .) bit for bit.  IDs may repeat.  An
 * unknown ID is CMS_E_NO_SUCH_ID and nothing is written.  One workgroup per
 * ids1[i] images that owner's sketch row in LDS once for all of ids2 (widths
 * above 8192 go pair by pair through the kernel of cms_similarities). */
int cms_similarity_block(cms_handle* h, const int64_t* ids1, int64_t n1, const int64_t* ids2, int64_t n2, double* out);
/* GenericItemBasedRecommender.doEstimatePreference (:231-259) for n users
 * over a handle whose owners are ITEMS: user u's preferences are pref_items /
 * pref_vals [pref_offsets[u], pref_offsets[u + 1]) in PreferenceArray order,
 * its candidates cand_items [cand_offsets[u], cand_offsets[u + 1]); out
 * (floats) is parallel to cand_items.  Per candidate: the similarities with
 * the preferred items, NaN skipped, preference += sim * pref and total += sim
 * in preference order, NaN for fewer than two, (float)(preference / total),
 * then the EstimatedPreferenceCapper clamp when use_capper.  Both offset arrays
 * hold n + 1 non-decreasing entries from 0. */
int cms_item_estimates_batch(cms_handle* h, int64_t n, const int64_t* pref_offsets, const int64_t* pref_items,
                             const float* pref_vals, const int64_t* cand_offsets, const int64_t* cand_items,
                             int32_t use_capper, float cap_min, float cap_max, float* out);
/* GenericItemBasedRecommender.recommend(userID, howMany, null, includeKnownItems)
 * (:120-139) for n users of the DataModel given as a CSR (model_user_ids
 * strictly ascending; row r holds pref_items / pref_vals [pref_offsets[r],
 * pref_offsets[r + 1])), over a handle whose owners are the model's items.
 * strategy 0: PreferredItemsNeighborhoodCandidateItemsStrategy (the default),
 * 1: AllUnknownItemsCandidateItemsStrategy.  The candidates come in FastIDSet
 * iteration order, every estimate from one device batch, the ranking is
 * TopItems.getTopItems with the JDK heap order.  out_counts[n] (0 for a user
 * without preferences), out_items / out_values [n][how_many].  A user missing
 * from the model is CMS_E_NO_SUCH_ID. */
int cms_item_recommend_batch(cms_handle* h, int64_t n, const int64_t* user_ids, int64_t n_model_users,
                             const int64_t* model_user_ids, const int64_t* pref_offsets, const int64_t* pref_items,
                             const float* pref_vals, int32_t strategy, int32_t how_many, int32_t include_known,
                             int32_t use_capper, float cap_min, float cap_max, int32_t* out_counts, int64_t* out_items,
                             float* out_values);
/* GenericUserBasedRecommender.mostSimilarUserIDs(id, k) with the CosineCM
 * estimator (:119-127, :231-247) and TopItems.getTopUsers (TopItems.java:91-136):
 * the first k other owners under (similarity desc, ID asc), NaN excluded.
 * Writes *count <= k entries; scores are the fp64 similarities. */
int cms_most_similar(cms_handle* h, int64_t id, int32_t k, int64_t* out_ids, double* out_scores, int32_t* count);
/* mostSimilar for every owner in rows [row_begin, row_begin+row_count): the
 * all-pairs top-k pass (config 4).  ids/scores are [row_count][k]; counts[row_count]. */
int cms_top_k_rows(cms_handle* h, int64_t row_begin, int64_t row_count, int32_t k, int64_t* ids,
                   double* scores, int32_t* counts);
/* ThresholdUserNeighborhood.getUserNeighborhood(id) for nq owners at once
 * (T/impl/neighborhood/ThresholdUserNeighborhood.java:77-97): every OTHER
 * owner whose similarity s = userSimilarity(id, other) -- the value
 * cms_similarities returns, after normalizeWeightResult -- passes
 * !Double.isNaN(s) && s >= threshold (:88-90), as one CSR: the list of ids[q]
 * is out_ids / out_scores [offsets[q], offsets[q + 1]).  The sampling rate is
 * 1: every owner is considered (SamplingLongPrimitiveIterator's random
 * sampling is not reproduced).  On a per-owner-shape handle the similarity is
 * the asymmetric userSimilarity(id, other): the query's preferences at the
 * other's shape (CosineCM.java:83-96), so v may be in u's list and u not in v's.
 *
 * order: CMS_NEIGHBOR_ORDER_ID lists ascending owner ID, the getUserIDs()
 * order in which the reference adds the neighbours (:86-92);
 * CMS_NEIGHBOR_ORDER_FASTIDSET lists what it returns, neighborhood.toArray()
 * of a new FastIDSet() after those adds (:81, :96; FastIDSet.java:157-166),
 * scores travelling with their IDs.  ids may repeat and come in any order;
 * each entry gets its own list.
 *
 * Capacity protocol: offsets [nq + 1] and *total are complete on every
 * accepted call, whether or not the lists fit.  out_ids == NULL (capacity 0)
 * only counts.  With out_ids != NULL and *total > capacity the call returns
 * CMS_E_PARAM (as cms_save_table_device does for a short buffer) and the
 * contents of out_ids / out_scores are unspecified: call again with *total.
 * out_scores may be NULL.  nq == 0 writes offsets[0] = 0, *total = 0.
 *
 * CMS_E_STATE before cms_finalize; CMS_E_PARAM for a NaN threshold (the
 * constructor's checkArgument, :73; any other double is taken, infinities
 * included), a bad order or a null offsets / total; CMS_E_NO_SUCH_ID for an
 * unknown ID, before any device work; CMS_E_SKETCH on a per-owner handle with
 * an owner whose (delta, epsilon) raise CMException; CMS_E_OOM when a chunk's
 * staging buffer cannot be had.  The call changes nothing in the table; a
 * merged multi-rank handle answers locally, with no collective. */
#define CMS_NEIGHBOR_ORDER_ID 0        /* ascending owner ID: the order the reference adds them */
#define CMS_NEIGHBOR_ORDER_FASTIDSET 1 /* FastIDSet.toArray() of new FastIDSet() after those adds:
                                          what getUserNeighborhood returns, and the order
                                          doEstimatePreference sums in */
int cms_threshold_neighbors(cms_handle* h, const int64_t* ids, int64_t nq, double threshold, int32_t order,
                            int64_t* offsets /* nq + 1 */, int64_t* out_ids, double* out_scores /* may be NULL */,
                            int64_t capacity, int64_t* total);
/* Host only, no handle: out = toArray() of a new FastIDSet() after
 * add(ids[0..n)) in order (FastIDSet.java:125-166; default size 2, load factor
 * 1.5); *count <= n (a repeated ID is added once).  An ID equal to FastIDSet's
 * NULL or REMOVED sentinel (Long.MIN_VALUE, Long.MAX_VALUE) is CMS_E_PARAM,
 * add's checkArgument (:126).  The implementation is the one
 * cms_recommend_batch orders getAllOtherItems with. */
int cms_fastidset_to_array(const int64_t* ids, int64_t n, int64_t* out, int64_t* count);
/* mostSimilar for EVERY owner (config 4, the suggested cms_topk_all of the
 * scope table): the same lists as cms_top_k_rows(h, 0, num_owners, ...), but
 * each unordered pair's similarity is computed once and streamed into both
 * owners' lists (no n x n slab).  ids/scores are [num_owners][k] by owner
 * row, counts[num_owners]; k <= 512.  Entries past counts[r] in row r are
 * padding with a defined value: ID -1 and a NaN score (every byte 0xFF), for
 * this call and for cms_top_k_refresh and the _device variants below. */
int cms_top_k_all(cms_handle* h, int32_t k, int64_t* ids, double* scores, int32_t* counts);
/* cms_top_k_all with the lists left on the device: d_ids / d_scores
 * [num_owners][k] and d_counts [num_owners] on the handle's GPU (no host copy
 * of the 1.6 GB answer at 1M owners, k = 100).  Returns when they are written. */
int cms_top_k_all_device(cms_handle* h, int32_t k, int64_t* d_ids, double* d_scores, int32_t* d_counts);
/* With a communicator (cms_comm_init, world G > 1) cms_top_k_all is collective:
 * rank r computes shard r of the pairs, the partial lists are all-gathered
 * over RCCL and merged exactly; every rank receives the full result
 * (G * k <= 1024).  The two pieces are also exported: */
/* The partial lists of shard `shard` of `nshards` ([num_owners][k] IDs and
 * scores, counts): every pair is computed by exactly one shard. */
int cms_top_k_all_partial(cms_handle* h, int32_t k, int32_t shard, int32_t nshards, int64_t* ids, double* scores,
                          int32_t* counts);
/* Exact merge of nparts partial lists laid out [nparts][num_owners][k] (counts
 * [nparts][num_owners]) into the final lists (nparts * k <= 1024). */
int cms_top_k_merge(cms_handle* h, int32_t k, int32_t nparts, const int64_t* ids, const double* scores,
                    const int32_t* counts, int64_t* out_ids, double* out_scores, int32_t* out_counts);
/* The periodic top-k refresh of a streaming table (config 5; the Refreshable
 * contract of the precomputed similarities, T/common/Refreshable.java:51,
 * feeding GenericItemSimilarity): returns exactly what cms_top_k_all returns
 * for the current table.  The first call (or one with another k, or after a
 * CSR ingest, cms_reset or the first multi-rank merge) runs the whole job and
 * keeps every owner's list 2k deep on the device; later calls recompute only
 * the pairs with an owner a COO ingest touched since, fold them into the kept
 * lists, and recompute whole any list that lost its exactness margin.
 * Collective like cms_top_k_all with a communicator. */
int cms_top_k_refresh(cms_handle* h, int32_t k, int64_t* ids, double* scores, int32_t* counts);
/* cms_top_k_refresh into device buffers (layout and padding as
 * cms_top_k_all_device). */
int cms_top_k_refresh_device(cms_handle* h, int32_t k, int64_t* d_ids, double* d_scores, int32_t* d_counts);
/* Statistics of the last cms_top_k_refresh: owners touched (num_owners for a
 * whole job), lists recomputed whole, whole jobs so far. */
int cms_refresh_stats(cms_handle* h, int64_t* touched, int64_t* redone, int64_t* full_jobs);
/* Operand classes of the last cms_top_k_refresh's all-pairs job: out6 =
 * {multi-limb owners, int8 owners, fp4 owners, touched multi-limb, touched
 * int8, touched fp4} (a whole job counts every owner as touched).  Each class
 * has its own pair cost (k_cosine_mls limb passes, int8 and fp4 symmetric
 * waves), so the work a refresh must redo follows from these six counts.
 * Zeros for per-owner and fp64 handles (no operand classes). */
int cms_refresh_classes(cms_handle* h, int64_t* out6);

/* cms_top_k_all written as FileSimilarItemsWriter does
 * (T/impl/similarity/precompute/FileSimilarItemsWriter.java:50-61): one line
 * "itemID,similarItemID,similarity" per similar item, owners in ascending ID
 * order, each list most similar first; similarity as Java's
 * String.valueOf(double), narrowed to float first when as_float (the
 * RecommendedItem values SimilarItems carries, SimilarItems.java:36-47). */
int cms_write_similar_items(cms_handle* h, const char* path, int32_t k, int32_t as_float);
/* The same all-pairs lists in the output formats of the other similarity
 * drivers a sketch cosine can stand in for:
 *   CMS_FORMAT_ITEM_SIMILARITY_JOB -- ItemSimilarityJob's text result
 *     (T/hadoop/similarity/item/ItemSimilarityJob.java:181-233): each pair of
 *     a list once as "aID\tbID\tsimilarity" with aID < bID, sorted by (aID, bID)
 *     (EntityEntityWritable.java:64-71); for a pair listed by both owners the
 *     lower ID's value is kept.
 *   CMS_FORMAT_SPARK_ITEMSIMILARITY -- spark-itemsimilarity's
 *     TextDelimitedIndexedDatasetWriter, default schema
 *     (spark/src/main/scala/org/apache/mahout/drivers/TextDelimitedReaderWriter.scala:244-303):
 *     "ID\tID1:s1 ID2:s2 ..." per owner, non-zero similarities by strength
 *     descending; a bare "ID" when the list is empty.
 * Values print as Java's Double.toString (fp64). */
#define CMS_FORMAT_ITEM_SIMILARITY_JOB 1
#define CMS_FORMAT_SPARK_ITEMSIMILARITY 2
int cms_write_similarities(cms_handle* h, const char* path, int32_t k, int32_t format);
/* cms_write_similarities with RowSimilarityJob's --threshold: pairs whose
 * similarity is below `threshold` are left out (of the lists before the top-k,
 * which for a top-k list is the same as dropping them afterwards;
 * RowSimilarityJob.java, ItemSimilarityJob.java:128-129).  In the
 * ItemSimilarityJob format a pair also needs similarity > Double.MIN_VALUE,
 * the TopSimilarItemsQueue sentinel (TopSimilarItemsQueue.java:50-58,
 * ItemSimilarityJob.java:203-209). */
int cms_write_similarities_threshold(cms_handle* h, const char* path, int32_t k, int32_t format, double threshold);
/* Java Double.toString(v) into buf (NUL-terminated); returns the length or -1. */
int cms_format_java_double(double v, char* buf, int32_t cap);

/* Counters of rows [row_begin, row_begin+row_count) as fp64 (the reference's
 * counter type), [row_count][d][w]. */
int cms_read_counters(cms_handle* h, int64_t row_begin, int64_t row_count, double* out);
/* The same counters without leaving the device: u32 in counter units (the
 * preference times 2^frac_bits), [row_count][d][w], written to d_out on the
 * handle's stream (asynchronous, like the device ingests) -- for a device-side
 * consumer of the sketches (getExportedCMProfile for many owners,
 * CosineCM.java:60-67) and for whole-table checks at sizes the host cannot hold. */
int cms_read_counters_device(cms_handle* h, int64_t row_begin, int64_t row_count, uint32_t* d_out);
/* How each owner's counters are stored (no reference counterpart: the
 * reference keeps every sketch as fp64): out_form[i] is one of CMS_FORM_*,
 * out_bound[i] the proven bound on the owner's counters the form was chosen
 * for (0 for u32 rows; either output may be NULL).  For capacity checks. */
#define CMS_FORM_U32 0  /* hot row: u32 slot */
#define CMS_FORM_U16 1
#define CMS_FORM_U8 2
#define CMS_FORM_U4 3
#define CMS_FORM_U2 4
#define CMS_FORM_U1 5
#define CMS_FORM_LIST 6 /* sparse key-bucket list */
int cms_owner_forms(cms_handle* h, int64_t row_begin, int64_t row_count, int32_t* out_form, uint32_t* out_bound);

/* ---- anonymous profiles: queries for a user the table does not hold ---------
 * PlusAnonymousUserDataModel (T/impl/model/PlusAnonymousUserDataModel.java:74-137,
 * TEMP_USER_ID = Long.MIN_VALUE) lets recommender.recommend(TEMP_USER_ID, n)
 * serve temporary preferences -- a visitor's session, a new user, a basket.
 * With CosineCM that call sketches the preferences with exportProfile
 * (CosineCM.java:41-58) and compares the sketch with every owner's (:83-96).
 * These calls take the preferences themselves: (keys[i], vals[i]) pairs,
 * update(key, val) each in order, duplicate keys adding; vals NULL = 1.0 each.
 *
 * The handle must be finalized (CMS_E_STATE), with a fixed shape and
 * CMS_COUNTER_U32: per-owner-shape handles and fp64 handles return CMS_E_STATE
 * (both need kernel families of their own, not built yet).  A merged
 * multi-rank handle answers locally -- every rank holds the whole table, no
 * collective is issued.  The calls hold the handle exclusively, as
 * cms_most_similar does, and change nothing of it: not the table, the norms,
 * the kept refresh lists or touched marks, pairs_ingested or any cms_stats
 * field (topk_redo aside, when the top-k's radix fallback runs).
 *
 * Values are validated as a host ingest validates them -- a non-negative
 * multiple of 2^-frac_bits below 2^(32-frac_bits), else CMS_E_VALUE; a profile
 * whose total in counter units reaches 2^32 is CMS_E_OVERFLOW -- for the whole
 * batch before any device work: a refused call writes no output.  An empty
 * profile is legal: every similarity NaN, an empty list, every estimate NaN.
 * A width whose sketch row does not fit a compute unit's LDS as u32 counters
 * (above 32768) is CMS_E_PARAM.
 *
 * Every similarity equals, bit for bit, what cms_similarities returns for a
 * twin owner holding the same stream (DoubleCountMinSketch.cosine :114-149,
 * then normalizeWeightResult). */

/* CosineCM.userSimilarity(TEMP_USER_ID, ids2[i]) for the temporary preferences
 * (keys[0..m), vals[0..m) or NULL = 1.0 each).  CMS_E_NO_SUCH_ID for an
 * unknown owner. */
int cms_anonymous_similarities(cms_handle* h, const int64_t* keys, const float* vals, int64_t m,
                               const int64_t* ids2, int64_t n, double* out);
/* GenericUserBasedRecommender.mostSimilarUserIDs(TEMP_USER_ID, k) (:119-127)
 * with TopItems.getTopUsers (TopItems.java:91-136) for nq profiles at once:
 * profile q is keys/vals[offsets[q] .. offsets[q+1]) (nq + 1 offsets from 0,
 * non-decreasing, else CMS_E_PARAM); ids/scores [nq][k], counts[nq].  Every
 * owner is a candidate -- there is no self to exclude, an owner identical to
 * the profile is listed at its score -- in the order similarity descending,
 * owner ID ascending, NaN excluded.  k <= 512; entries past counts[q] are
 * padded as cms_top_k_all pads them (ID -1, all-ones NaN).  Each owner's
 * stored row is read once per batch of profiles, not once per profile. */
int cms_anonymous_most_similar(cms_handle* h, int64_t nq, const int64_t* offsets, const int64_t* keys,
                               const float* vals, int32_t k, int64_t* ids, double* scores, int32_t* counts);
/* doEstimatePreference(TEMP_USER_ID, neighbourhood, item)
 * (GenericUserBasedRecommender.java:134-184) for q items: the similarities of
 * the temporary preferences with neighbor_ids[0..mn) in the caller's order,
 * then cms_estimate_preferences' sums.  The temporary user is never in its own
 * neighbourhood.  CMS_E_NO_SUCH_ID for an unknown neighbour. */
int cms_anonymous_estimate_preferences(cms_handle* h, const int64_t* keys, const float* vals, int64_t m,
                                       const int64_t* neighbor_ids, int64_t mn, const int64_t* item_keys, int64_t q,
                                       int32_t use_capper, float cap_min, float cap_max, float* out);
/* How many profiles the similarity kernel serves per read of an owner's row at
 * this handle's width: *batch for sketch-row images of elem_bytes (2: every
 * counter of the batch below 2^16, else 4) -- the largest power of two up to
 * 8 whose [width][batch] image fits 128 KiB of LDS.  For tests and sizing. */
int cms_anonymous_batch(cms_handle* h, int32_t elem_bytes, int32_t* batch);

/* ---- per-owner sketch shapes: CosineCM with its CountMinSketchConfig --------
 * The reference sizes every owner's sketch separately.  CountMinSketchConfig
 * (T/impl/common/CountMinSketchConfig.java:120-158) picks (d, w) per owner and
 * stores delta = exp(-d), epsilon = e/w; CosineCM.userSimilarity(u1, u2)
 * builds u1's sketch with u2's (delta, epsilon) and compares it with u2's own
 * cached sketch (T/impl/similarity/CosineCM.java:60-67,83-96), so the
 * similarity is asymmetric.  A per-owner handle keeps the DataModel (one
 * cms_ingest_csr / cms_ingest_csr_device call; a later call replaces it)
 * resident on the GPU; cms_finalize builds every owner's own sketch, and the
 * similarity kernels hash u1's preferences at u2's shape on the fly.
 * p->depth / p->width are ignored.  cms_similarity(ies), cms_point_query,
 * cms_estimate_preferences, cms_most_similar, cms_top_k_rows, cms_top_k_all
 * and cms_write_similar_items work as for fixed shapes; the COO ingests,
 * cms_read_counters, cms_hash_keys and cms_top_k_all_partial return
 * CMS_E_STATE.  Several GPUs: every rank ingests the whole DataModel (u1's
 * preferences are hashed at each candidate's shape) and, after
 * cms_comm_init / cms_comm_init_transport, cms_top_k_all splits the QUERY
 * rows over the ranks (256-row chunks round-robin) and all-gathers the lists,
 * so every rank returns the single-GPU answer. */
int cms_create_per_owner(const cms_params* p, cms_handle** out);
/* CountMinSketchConfig(q).configure(dataModel) -> computeConfig on the GPU:
 * per owner n = its CSR row length (PreferenceArray.length()), u = num_keys
 * (dataModel.getNumItems()); maximise Fmeasure(w, d, n, u, q) (:210-219) over
 * d in [1, 25), w in [d, n], ties to the last (>=, :137); delta = exp(-d),
 * epsilon = e/w.  Needs the DataModel first.  CMS_E_SKETCH for an owner with
 * no solution (the TasteException of :145-147). */
int cms_configure_owner_shapes(cms_handle* h, double q, int64_t num_keys);
/* Caller-supplied configuration: the getDelta(id) / getEpsilon(id) values of
 * a CountMinSketchConfig (:230-251), in owner-row order.  An owner whose pair
 * is outside the CMException ranges (AbstractCountMinSketch.java:71-76; e.g.
 * the 0.0 trove returns for a missing owner) fails, with CMS_E_SKETCH, exactly
 * the calls that need its shape with CMS_E_SKETCH (exportProfile, CosineCM.java:41-58).  Shapes
 * beyond this build (depth > 32, width > 2^24) are refused here. */
int cms_set_owner_delta_epsilon(cms_handle* h, const double* delta, const double* epsilon);
/* The configuration and the shape new DoubleCountMinSketch(delta, epsilon, ...)
 * derives from it (width = depth = 0: CMException).  Outputs may be NULL. */
int cms_get_owner_shapes(cms_handle* h, double* delta, double* epsilon, int32_t* width, int32_t* depth);
/* getExportedCMProfile(id) (CosineCM.java:60-67): the owner's own sketch as
 * fp64 [depth][width] (capacity in doubles; out NULL returns the shape only). */
int cms_read_owner_sketch(cms_handle* h, int64_t id, double* out, int64_t capacity, int32_t* width, int32_t* depth);

/* ---- checkpoint and restore of the sketch table ------------------------------
 * The reference has no counterpart: CosineCM rebuilds every sketch from the
 * DataModel (its own persistence is the CountMinSketchConfig's delta/epsilon
 * cache).  A checkpoint image carries every owner row in the form the table
 * stores it in (list / 1 / 2 / 4 / 8 / 16-bit rows, u32 hot rows, fp64), so it
 * is about cms_stats.stored_bytes long; the format (version 1, little-endian)
 * is documented byte for byte in DESIGN.md 3 "Checkpoint image" and read
 * without the library by mahout_amd/checkpoint.py.  A file is the image; a
 * device image is the same bytes.
 *
 * Saving: fixed-shape handles (CMS_E_STATE on a per-owner handle), before or
 * after cms_finalize; on a multi-rank handle only once merged and with no COO
 * batch ingested since the last cms_finalize (every rank then holds the whole
 * table; CMS_E_STATE otherwise).  The call synchronises and
 * reports a pending device-ingest error as cms_synchronize would; it writes
 * only on CMS_OK.
 *
 * Loading: the handle must be empty (new, or after cms_reset), fixed-shape and
 * without a communicator (CMS_E_STATE otherwise), and its depth, width,
 * num_owners, counter type and frac_bits must equal the image's (CMS_E_PARAM).
 * The image's hash parameters and owner IDs are installed as
 * cms_set_hash_params / cms_set_owner_ids would, pairs_ingested is restored,
 * and the handle is left "ingested, not finalized": cms_finalize derives the
 * norms (the image stores none), later ingests behave as on the saving handle.
 * Header, directory and section bounds are checked on the host before the
 * device sees anything, the payload checksum and every list row's entries on
 * the device while copying; on any failure the call returns CMS_E_PARAM and
 * the handle is empty and usable, as after cms_reset.  The restored rows are
 * laid out anew (no holes where rows moved), in whatever layout the handle
 * has: CMS_NO_COMPACT / CMS_NO_VMM / CMS_NO_FORMS handles load any image. */

/* Bytes cms_save_table would write / cms_save_table_device needs. */
int cms_checkpoint_size(cms_handle* h, int64_t* bytes);
/* The image to path: written as path + ".tmp", then renamed, so a crash never
 * leaves a half file under the real name. */
int cms_save_table(cms_handle* h, const char* path);
int cms_load_table(cms_handle* h, const char* path);
/* The image into / out of device memory on the handle's GPU (16-byte aligned).
 * *bytes = the image's length; CMS_E_PARAM when capacity is smaller (*bytes is
 * still set).  Blocking: the image is complete when the call returns. */
int cms_save_table_device(cms_handle* h, void* d_buf, int64_t capacity, int64_t* bytes);
int cms_load_table_device(cms_handle* h, const void* d_buf, int64_t bytes);
/* Merging: a count-min sketch is linear, so an image adds counter by counter
 * into a live table built with the same hash functions: table[r][i][j] +=
 * image[r][i][j], row_mass[r] += the image's, pairs_ingested += the image's.
 * The handle is fixed-shape and without a communicator (CMS_E_STATE otherwise),
 * empty or populated, before or after cms_finalize; afterwards it is
 * "ingested, not finalized", exactly as after a COO batch (cms_finalize
 * re-derives the norms; kept cms_top_k_refresh lists stay, the image's
 * non-empty rows marked touched).  Depth, width, num_owners, counter type and
 * frac_bits, the hash parameters in use (a_i, b_i for i < depth, drawn or
 * installed) and the owner-ID sections (both absent, or identical) must equal
 * the image's: CMS_E_PARAM.  u32 counters: no row's mass + image mass may reach
 * 2^32 (CMS_E_OVERFLOW).  A pending device-ingest error is reported first, as
 * cms_synchronize would.  Every check -- header, directory, payload checksum,
 * pad bytes and every list row's entries, over the WHOLE image -- precedes
 * every write: a refused merge leaves the live table bit for bit as it was.
 * The file is staged whole in device memory first (CMS_E_OOM when it does not
 * fit beside the table). */
int cms_merge_table(cms_handle* h, const char* path);
int cms_merge_table_device(cms_handle* h, const void* d_buf, int64_t bytes);
/* Subtracting: the other half of the merge.  If the image was built with the
 * same hash functions and its stream is a sub-stream of the live table's,
 * table - image is, counter for counter, the table of the remaining stream
 * (merge today's delta, subtract the delta from N days ago: a sliding window).
 * table[r][i][j] -= image[r][i][j], row_mass[r] -= the image's,
 * pairs_ingested -= the image's (saturating at 0: instrumentation only).
 * Accepted under the merge's rules, in the merge's order, and: u32 counters
 * only -- an fp64 handle returns CMS_E_STATE, since (a + b) - b is not a in
 * fp64 and the result would be no stream's table; no row mass may fall below
 * zero (live mass >= image mass for every row, so an empty handle accepts
 * only an image whose masses are all 0) and no single counter may fall below
 * zero (live >= image for every (r, i, j); a device pass over the whole image
 * against the live rows in whatever form they are in): CMS_E_OVERFLOW, the
 * message naming an offending owner row.  Every check precedes every write: a
 * refused subtraction leaves every counter, place, form, bound, mass and
 * pairs_ingested bit for bit as they were.  Afterwards the handle is
 * "ingested, not finalized" as after a merge; the rows the image subtracts
 * from are marked for cms_top_k_refresh.  Dense live rows keep form and place
 * (nothing narrows, demotes or returns to the shared zero row); a live list
 * row that loses entries is rewritten densely first. */
int cms_subtract_table(cms_handle* h, const char* path);
int cms_subtract_table_device(cms_handle* h, const void* d_buf, int64_t bytes);
/* Compacting: every writer above widens, promotes or moves a row and none
 * narrows one, so after merges and subtractions a table stores far more than
 * its counters need.  Re-store every owner row in the narrowest form its
 * counters need now and lay the table out anew.  *rows_changed (may be NULL) =
 * owners whose stored form or place class differs afterwards.
 * The target form of a row with largest counter cmax and mass M, in order:
 * cmax == 0: no storage (the shared zero row); M >= 2^16 or cmax >= 2^16: u32;
 * else the narrowest of 1-/2-/4-/8-/16-bit rows the handle stores that holds
 * cmax -- or a sorted list of M keys where frac_bits == 0, the handle stores
 * lists, every sketch row sums to M, M <= min(CMS_LIST_KEYS, 1024),
 * depth * M <= 8192, the list's 2 + 2 * depth * M bytes are strictly fewer
 * than the dense row's, and cmax <= 255 (no list holds a bucket more than 255
 * times, as no built list does: the writers re-count list entries in u8).  Place classes are the forms' own and the bounds the
 * rows' largest counters (0 for u32 rows), as a checkpoint of defaults records.
 * No counter, row mass, owner ID or hash parameter changes, nor does
 * pairs_ingested, and the handle's state is carried over: a finalized handle
 * stays finalized and every query returns the bits it returned before, without
 * a new cms_finalize; "ingested, not finalized" stays so; kept
 * cms_top_k_refresh lists and touched marks survive (scores do not depend on
 * storage).  Without the compact layout (CMS_NO_COMPACT=1) rows keep whole
 * slots: stored_bytes falls, table_bytes need not.
 * The handle is fixed-shape, CMS_COUNTER_U32 and without a communicator, before
 * or after cms_finalize: CMS_E_STATE for an fp64 handle (one form: nothing to
 * narrow), a per-owner handle and a handle with a communicator.  A pending
 * device-ingest error is reported first, as cms_synchronize would.  An empty
 * handle returns CMS_OK and 0.  The call holds the handle exclusively.
 * Failure: the re-formed rows are packed into a transient buffer of about the
 * new stored bytes beside the old table and verified there; a state error, a
 * pending ingest error or CMS_E_OOM for that buffer is returned before the
 * first change and leaves the handle bit for bit as it was.  If a HIP call
 * fails after the old rows have been given up, the table is lost: the handle
 * is left empty and usable, as after cms_reset, and the call returns CMS_E_HIP
 * with a message that says so. */
int cms_compact_table(cms_handle* h, int64_t* rows_changed);
/* Folding: the table of the same stream at a narrower width, without the
 * stream.  The hash is ((a key + b) mod p) mod width and (s mod w) mod w' =
 * s mod w' for every divisor w' of w, so
 *   T'[r][i][j'] = sum of T[r][i][j] over j = j' (mod new_width)
 * is, counter for counter, the table the stream builds at new_width with the
 * same hash parameters.  The result is an ordinary checkpoint image of width
 * new_width -- a file, or device memory -- for cms_load_table into a handle of
 * that width or cms_merge_table / cms_subtract_table into a live one: depth,
 * counter type, frac_bits, seed, hash parameters, owner IDs, row masses and
 * pairs_ingested are the source's; every folded row is stored in the form
 * cms_compact_table's rule gives it at shape (depth, new_width) under the
 * handle's CMS_LIST_KEYS / CMS_NO_FORMS, with the forms' own place classes and
 * the folded largest counters as bounds (0 for u32 rows); a list row's entries
 * are its buckets ascending, bucket j' repeated T'[r][i][j'] times.
 * new_width: 1 <= new_width <= width and width % new_width == 0, CMS_E_PARAM
 * otherwise; new_width == width yields the image of the compacted table.
 * Accepted exactly where cms_save_table is (fixed shape, before or after
 * cms_finalize, a multi-rank handle under the save's rule), and u32 counters
 * only: an fp64 handle returns CMS_E_STATE (a folded fp64 sum is not the
 * sequential chain in ingest order, so it would be no stream's table).  A
 * pending device-ingest error is reported first, as cms_synchronize would.
 * The call holds the handle exclusively and only reads it: no counter, form,
 * place, mass, norm, kept cms_top_k_refresh list, touched mark, pairs_ingested
 * or finalized state changes.  A folded counter that would reach 2^32 (only a
 * loaded image can hold one: a stream's sketch rows sum to a mass below 2^32)
 * returns CMS_E_OVERFLOW naming the owner row, and nothing is written.  The
 * table is never expanded: two passes read every stored row once each.
 * The reference has no counterpart. */
/* Bytes cms_fold_table would write / cms_fold_table_device needs (runs the
 * scan: the size depends on each folded row's form). */
int cms_fold_size(cms_handle* h, int32_t new_width, int64_t* bytes);
/* The folded image to path: written as path + ".tmp", then renamed. */
int cms_fold_table(cms_handle* h, int32_t new_width, const char* path);
/* The folded image into device memory on the handle's GPU (16-byte aligned).
 * *bytes = the image's length, set whenever the fold itself is accepted;
 * CMS_E_PARAM when capacity is smaller, and then the buffer is untouched.
 * Blocking: the image is complete when the call returns. */
int cms_fold_table_device(cms_handle* h, int32_t new_width, void* d_buf, int64_t capacity, int64_t* bytes);
/* The parameters a handle needs to load the file (host only: no device call):
 * depth, width, counter type, seed, num_owners and frac_bits from its header;
 * weighting unweighted, device -1, flags 0.  CMS_E_PARAM for a file that is
 * not a checkpoint, has an unknown version, or is shorter or longer than its
 * header claims.  file_bytes may be NULL. */
int cms_checkpoint_info(const char* path, cms_params* out, int64_t* file_bytes);

/* ---- the exact CosineSimilarity ------------------------------------------------
 * CosineSimilarity.userSimilarity (T/impl/similarity/CosineSimilarity.java:44-103)
 * over the owners' raw preferences: the quantity the sketch cosine
 * approximates.  sumX2, sumXY and sumY2 are the reference's sequential fp64
 * sums (sumXY over the common items, in id1's preference order); NaN when
 * either list is empty or Math.sqrt(sumX2) * Math.sqrt(sumY2) == 0.0; else
 * sumXY / denominator and normalizeWeightResult(result, count, count) with
 * count = the two list lengths' sum (AbstractSimilarity.java:313-330) under the
 * handle's weighting.  Every result equals the reference's bit for bit.
 *
 * The DataModel of the handle's num_owners rows as a host CSR (row i <->
 * cms_set_owner_ids' ids[i]): offsets [n + 1] from 0, never decreasing; a
 * row's keys strictly ascending, as GenericDataModel gives them; vals the
 * preference values (any float).  CMS_E_PARAM otherwise, and then the handle
 * keeps what it had.  Works on every handle kind, before or after
 * cms_finalize, and neither reads nor writes the sketch table; a second call
 * replaces the model.  Timing scope "exact_attach". */
int cms_exact_attach_csr(cms_handle* h, const int64_t* offsets, const int64_t* keys, const float* vals);
/* Frees the model (cms_destroy does too).  The calls below return
 * CMS_E_STATE while no model is attached. */
int cms_exact_detach(cms_handle* h);
/* out[t] = userSimilarity(id1, ids2[t]); owner IDs as cms_similarities takes
 * them (CMS_E_NO_SUCH_ID).  Timing scope "exact_pairs". */
int cms_exact_similarities(cms_handle* h, int64_t id1, const int64_t* ids2, int64_t m, double* out);
/* out[t] = userSimilarity(ids1[t], ids2[t]). */
int cms_exact_pairs(cms_handle* h, const int64_t* ids1, const int64_t* ids2, int64_t m, double* out);
/* The k most similar owners of each owner ROW rows[q] (any order, repeats
 * allowed), laid out and ordered as cms_top_k_rows: TopItems.getTopUsers, NaN
 * skipped, the row itself excluded, similarity descending then owner ID
 * ascending; ids / scores [nq][k] (padding: ID -1, NaN), counts [nq]; scores
 * may be NULL.  k in [1, 512].  Timing scopes "exact_tile", "exact_pairs",
 * "top_k". */
int cms_exact_top_k_rows(cms_handle* h, const int64_t* rows, int64_t nq, int32_t k, int64_t* ids, double* scores,
                         int32_t* counts);
/* rows[i] = the owner row of ids[i] (cms_set_owner_ids, or the IDs a loaded
 * checkpoint installed); CMS_E_NO_SUCH_ID for an unknown ID.  Host only. */
int cms_owner_rows(cms_handle* h, const int64_t* ids, int64_t m, int64_t* rows);
/* The same list for one owner ID, as cms_most_similar returns it. */
int cms_exact_most_similar(cms_handle* h, int64_t id, int32_t k, int64_t* out_ids, double* out_scores, int32_t* count);
/* GenericUserBasedRecommender.doEstimatePreference over a similarity that is
 * no CosineCM (GenericUserBasedRecommender.java:134-184, sim == null) for n
 * users, shaped as cms_estimate_preferences_batch: a neighbour's preference is
 * the attached model's raw float for the item -- an absent item is no data
 * point, a present 0.0 is one -- and theSimilarity is this section's
 * userSimilarity(user, neighbour), skipped when NaN; the neighbours are taken
 * in the caller's order, the user itself skipped; fewer than two data points
 * give NaN, else (float)(preference / totalSimilarity) and the capper.  A key
 * the model lacks gives NaN; keys may repeat and come in any order.  Every
 * estimate equals the reference's bit for bit.  One user is a batch of one.
 * Argument rules and errors as cms_estimate_preferences_batch; CMS_E_STATE
 * without a model.  The sketch table is neither read nor written.  Timing
 * scopes "exact_pairs", "exact_estimate". */
int cms_exact_estimate_preferences_batch(cms_handle* h, int64_t n, const int64_t* user_ids, const int64_t* nb_offsets,
                                         const int64_t* neighbor_ids, const int64_t* item_offsets,
                                         const int64_t* item_keys, int32_t use_capper, float cap_min, float cap_max,
                                         float* out);
/* GenericUserBasedRecommender.recommend for n users over that estimate, shaped
 * as cms_recommend_batch with the attached model as the DataModel (owner rows
 * are its rows): getAllOtherItems in FastIDSet order on host threads, one
 * estimate batch, TopItems.getTopItems.  out_counts[n] (0 for an empty
 * neighbourhood), out_items / out_values [n][how_many].  An unknown user or
 * neighbour ID is CMS_E_NO_SUCH_ID, and nothing is written. */
int cms_exact_recommend_batch(cms_handle* h, int64_t n, const int64_t* user_ids, const int64_t* nb_offsets,
                              const int64_t* neighbor_ids, int32_t how_many, int32_t include_known, int32_t use_capper,
                              float cap_min, float cap_max, int32_t* out_counts, int64_t* out_items,
                              float* out_values);

/* ---- instrumentation ------------------------------------------------------- */
typedef struct cms_stats {
  uint32_t struct_size;     /* sizeof(cms_stats) as the caller compiled it: only fields that fit are written */
  int64_t pairs_ingested;   /* update() calls applied on this rank */
  int64_t num_owners;
  int32_t depth, width;
  int32_t exact_norms;      /* 1 if every (owner,row) norm is < 2^53 (bit-exact fast path) */
  int32_t world, rank;
  int64_t table_bytes;       /* the narrow rows' arena as laid out (zero row + every row's place) + the hot owners' u32 rows */
  int64_t multi_limb_owners; /* owners with a counter >= 128 (all-pairs limb split; -1 before the first all-pairs call) */
  int64_t topk_redo;         /* top-k rows that needed the radix-select fallback */
  int64_t deep_limb_owners;  /* of those, owners with a counter >= 2^14 (3+ limbs); -1 before */
  int64_t fp4_owners;        /* single-limb owners with every counter <= 4 (fp4 MFMA operands); -1 before */
  int64_t merge_words;       /* u64 words the last multi-rank merge all-reduced (packed counters) */
  int64_t hot_rows;          /* owners whose counters are stored as u32 (the others narrow) */
  int64_t stored_bytes;      /* bytes of counters as stored: what one whole-table build writes */
  int64_t u8_rows;           /* narrow owners stored as u8 (every counter < 2^8) */
  int64_t nibble_rows;       /* narrow owners stored as 4-bit counters (every counter < 2^4) */
  int64_t crumb_rows;        /* narrow owners stored as 2-bit counters (every counter < 2^2) */
  int64_t bit_rows;          /* narrow owners stored as 1-bit counters (every counter 0 or 1) */
  int64_t collective_calls;  /* all-reduce / all-gather calls made through the communicator so far */
  int32_t comm_kind;         /* 0 none (single-GPU path), 1 RCCL (cms_comm_init), 2 caller transport */
  int32_t device;            /* HIP device ordinal of the handle */
  int64_t list_rows;         /* narrow owners stored as sparse key-bucket lists (2 + 2 d m bytes, m keys) */
  int64_t po_wide_pairs;     /* per-owner top-k: (query, wide owner) pairs given the row-0 bound so far */
  int64_t po_wide_exact;     /* of those, pairs the bound could not rule out (computed exactly) */
} cms_stats;
/* out->struct_size must be set (at least through pairs_ingested); an ABI-2
 * caller whose cms_stats is shorter (built before later fields were appended)
 * receives the fields it knows. ABI-1 structs had no struct_size: bindings
 * compare cms_abi_version() with CMS_ABI_VERSION at load time (mahout_amd/_lib.py,
 * the JNI shim's JNI_OnLoad) and refuse a mismatch. */
int cms_get_stats(cms_handle* h, cms_stats* out);

/* Per-kernel HIP-event timing on the handle's stream (off by default).
 * level 1: the roofline kernels' scopes only ("build_rows", "ingest_atomic",
 * "allreduce", the cosine / top-k families); level >= 2: every scope, the
 * ingest phases ("partition", "build_plan", "hot_norms", "norms", merge
 * phases) included -- each recorded event costs the stream a few us. */
int cms_set_timing(cms_handle* h, int32_t enabled);
/* Accumulated (total ms, launches) for a kernel family name, e.g.
 * "build_rows", "partition", "norms", "allreduce", "cosine".  Process-wide
 * host counters, whatever the timing switch (cleared by cms_reset_timing):
 * "host_alloc" = ms in the library's hipMalloc calls (launches = calls),
 * "host_free" = ms in the hipFree of a growing buffer (it waits for queued
 * device work), "host_alloc_bytes" = bytes allocated (in total_ms),
 * "host_alloc_max" = the slowest single hipMalloc (ms; its bytes in launches). */
int cms_get_timing(cms_handle* h, const char* name, double* total_ms, int64_t* launches);
int cms_reset_timing(cms_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* MAHOUT_CMS_H */
