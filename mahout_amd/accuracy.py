"""How far the sketch cosine is from the cosine it approximates.

``sketch_accuracy`` compares, for a set of query owners, the top-k list of
CosineCM's sketch cosine (SketchTable.top_k_rows) with the top-k list of the
exact CosineSimilarity over the attached DataModel
(SketchTable.exact_top_k_rows), and the two similarities at both lists' pairs.
Every similarity comes from the library; only the reduction is numpy.
"""
import numpy as np


def _runs(rows):
    """Maximal runs of consecutive values in rows: (start index, length)."""
    out, i = [], 0
    while i < rows.size:
        j = i + 1
        while j < rows.size and rows[j] == rows[j - 1] + 1:
            j += 1
        out.append((i, j - i))
        i = j
    return out


def _errors(sketch, exact):
    """The error figures of sketch minus exact over one list's pairs."""
    nan = np.isnan(sketch) | np.isnan(exact)
    e = (sketch - exact)[~nan]
    none = float("nan")
    return {
        "pairs": int(e.size),
        "nan_pairs": int(nan.sum()),
        "abs_err_mean": float(np.abs(e).mean()) if e.size else none,
        "abs_err_max": float(np.abs(e).max()) if e.size else none,
        "signed_err_mean": float(e.mean()) if e.size else none,
    }


def sketch_accuracy(table, owner_ids, k):
    """The accuracy of a finalized table's sketch cosine for the query owners
    owner_ids (IDs of the table's owner universe, nq of them) at list length k.
    The table needs an attached model (attach_exact).

    Returns a dict.  With S = the sketch lists and E = the exact lists
    (ids [nq][k], scores [nq][k], counts [nq]; entry t of query q is valid for
    t < counts[q]):

      sketch_ids, sketch_scores, sketch_counts   S, as top_k_rows returns it (padding: ID -1, NaN)
      exact_ids, exact_scores, exact_counts      E, as exact_top_k_rows returns it
      recall_at_k [nq]   |{E.ids[q, :E.counts[q]]} & {S.ids[q, :S.counts[q]]}| / E.counts[q];
                         1.0 when E.counts[q] == 0
      sketch_list        over the pairs (owner_ids[q], S.ids[q, t]), t < S.counts[q], in
                         (q, t) order, with s = S.scores[q, t] and x = exact_pairs of the
                         pair, e = s - x over the pairs where neither is NaN:
                           pairs            how many such pairs
                           nan_pairs        pairs left out (s or x is NaN)
                           abs_err_mean     np.abs(e).mean()
                           abs_err_max      np.abs(e).max()
                           signed_err_mean  e.mean()
                         (the three figures are NaN when pairs == 0)
      exact_list         the same over the pairs (owner_ids[q], E.ids[q, t]), t < E.counts[q],
                         with x = E.scores[q, t] and s = similarities(owner_ids[q], ...) of the pair
    """
    ids = np.ascontiguousarray(owner_ids, np.int64).reshape(-1)
    rows = table.owner_rows(ids)
    nq = ids.size
    s_ids = np.full((nq, k), -1, np.int64)
    s_sc = np.full((nq, k), np.nan, np.float64)
    s_cnt = np.zeros(nq, np.int32)
    for i, m in _runs(rows):  # top_k_rows takes a row range
        a, b, c = table.top_k_rows(int(rows[i]), m, k)
        s_ids[i:i + m], s_sc[i:i + m], s_cnt[i:i + m] = a, b, c
    e_ids, e_sc, e_cnt = table.exact_top_k_rows(rows, k)

    recall = np.ones(nq, np.float64)
    for q in range(nq):
        ce = int(e_cnt[q])
        if ce:
            recall[q] = np.intersect1d(e_ids[q, :ce], s_ids[q, :int(s_cnt[q])]).size / ce

    s_valid = np.arange(k)[None, :] < s_cnt[:, None]
    e_valid = np.arange(k)[None, :] < e_cnt[:, None]
    s_ids[~s_valid], s_sc[~s_valid] = -1, np.nan  # padding as exact_top_k_rows pads
    qid = np.broadcast_to(ids[:, None], (nq, k))
    # the exact cosine at the sketch lists' pairs
    x_at_s = table.exact_pairs(qid[s_valid], s_ids[s_valid])
    # the sketch cosine at the exact lists' pairs, query by query
    s_at_e = np.concatenate([table.similarities(int(ids[q]), e_ids[q, :int(e_cnt[q])]) for q in range(nq)]
                            + [np.zeros(0, np.float64)])
    return {
        "sketch_ids": s_ids, "sketch_scores": s_sc, "sketch_counts": s_cnt,
        "exact_ids": e_ids, "exact_scores": e_sc, "exact_counts": e_cnt,
        "recall_at_k": recall,
        "sketch_list": _errors(s_sc[s_valid], x_at_s),
        "exact_list": _errors(s_at_e, e_sc[e_valid]),
    }


def _estimates_at(recommender, users, lists):
    """The recommender's own estimate (doEstimatePreferences with its own
    neighbourhood) at every (users[u], item of lists[u]) in (user, list) order."""
    off, nb = recommender._nb.getUserNeighborhoods(users)  # the lists getUserNeighborhood gives, in one pass
    parts = []
    for u, lst in enumerate(lists):
        if lst:
            est = recommender.doEstimatePreferences(int(users[u]), nb[off[u]:off[u + 1]], [i for i, _ in lst])
            parts.append(np.asarray(est, np.float64))
    return np.concatenate(parts + [np.zeros(0, np.float64)])


def _values(lists):
    return np.array([v for lst in lists for _, v in lst], np.float64)


def recommendation_accuracy(sketch_recommender, exact_recommender, user_ids, how_many):
    """What the sketch does to what a user is shown: the recommendations of a
    taste.GenericUserBasedRecommender over a CosineCM (sketch_recommender)
    against those of one over a taste.CosineSimilarity (exact_recommender),
    both over the same DataModel, for the users user_ids (nu of them) at list
    length how_many.  Every list and estimate comes from the library; only the
    reduction is numpy.

    Returns a dict.  With S_u = sketch_recommender.recommend_all(user_ids,
    how_many)[u] and E_u = exact_recommender.recommend_all(user_ids,
    how_many)[u], each a [(itemID, float32 value)] list:

      sketch_lists, exact_lists   S and E
      precision_at_n [nu]   |{items of S_u} & {items of E_u}| / len(E_u); 1.0 when E_u is empty
      exact_list         over the pairs (u, item of E_u) in (user, list) order, with x = the
                         exact list's value and s = sketch_recommender.doEstimatePreferences(u,
                         its own neighbourhood of u, items of E_u), e = s - x over the pairs
                         where neither is NaN:
                           pairs            how many such pairs
                           nan_pairs        pairs left out (s or x is NaN)
                           abs_err_mean     np.abs(e).mean()
                           abs_err_max      np.abs(e).max()
                           signed_err_mean  e.mean()
                         (the three figures are NaN when pairs == 0)
      sketch_list        the same over the pairs (u, item of S_u), with s = the sketch list's
                         value and x = exact_recommender.doEstimatePreferences(u, its own
                         neighbourhood of u, items of S_u)
    """
    users = np.ascontiguousarray(user_ids, np.int64).reshape(-1)
    s_lists = sketch_recommender.recommend_all(users, how_many)
    e_lists = exact_recommender.recommend_all(users, how_many)
    precision = np.ones(users.size, np.float64)
    for u, (s, e) in enumerate(zip(s_lists, e_lists)):
        if e:
            precision[u] = len({i for i, _ in s} & {i for i, _ in e}) / len(e)
    return {
        "sketch_lists": s_lists, "exact_lists": e_lists,
        "precision_at_n": precision,
        "exact_list": _errors(_estimates_at(sketch_recommender, users, e_lists), _values(e_lists)),
        "sketch_list": _errors(_values(s_lists), _estimates_at(exact_recommender, users, s_lists)),
    }
