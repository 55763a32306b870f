"""Host model of the recall statement of ``cdml_amd.knn.export(audit_rows=m)``: plain numpy over the
fp64 exact search of oracle/knn.py and the greedy rule of tests/test_knn_desim_host.py.  Plain module: it imports nothing of
the package, touches no GPU and holds no pytest configuration.

The sample is given (``cdml_amd.knn.audit_sample``: the first m entries of a seeded CPU ``torch.randperm(n)``, sorted).
  (a) the exact embedding lists of the sample's rows (cross mode: every row against its own side, ids global);
      e_hits = sum over rows of |I[r] & I_exact[r]| over the valid exact entries, e_possible = the number of those;
  (b) U = the sample and every id of its exact lists; the exact raw-feature lists of U;
  (c) f_hits / f_possible on the sample's rows, as (a);
  (d) a [n, k_f] table that holds the exact rows of U and -1 elsewhere -- the greedy rule reads only rows of ids in the
      query's own list -- and desim(I_exact[sample], table, query_ids = sample);
  (e) desim_rows_equal = the sampled rows whose SET of kept ids equals the export's; desim_kept_intersection / _union = the
      Jaccard numerator and denominator summed over the sample."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_knn_desim_host import greedy_desim  # noqa: E402

from oracle import knn as oknn  # noqa: E402

COUNT_KEYS = ("audit_rows", "union_rows", "e_hits", "e_possible", "f_hits", "f_possible", "desim_rows_equal",
              "desim_kept_intersection", "desim_kept_union")


def exact_lists(emb, doc_location, rows, k):
    """(D, I, d) of the exact search of ``rows`` (global ids; -1 / inf where a side runs out) and their full distance rows
    against the searched side; strict when not 0 < doc_location < n"""
    emb = np.asarray(emb, dtype=np.float32)
    n = emb.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    if not 0 < doc_location < n:
        return oknn.calc_knn_exact(emb, emb[rows], k)
    D = np.full((len(rows), k), np.inf)
    I = np.full((len(rows), k), -1, dtype=np.int64)
    d = [None] * len(rows)
    for sel, base, shift in ((rows < doc_location, emb[doc_location:], doc_location), (rows >= doc_location, emb[:doc_location], 0)):
        if sel.any():
            Ds, Is, ds = oknn.calc_knn_exact(base, emb[rows[sel]], k)
            D[sel], I[sel] = Ds, np.where(Is >= 0, Is + shift, Is)
            for t, r in enumerate(np.nonzero(sel)[0]):
                d[r] = ds[t]
    return D, I, d


def set_counts(got, want):
    hits = possible = 0
    for g, w in zip(np.asarray(got).tolist(), np.asarray(want).tolist()):
        w = set(x for x in w if x >= 0)
        hits += len(w & set(x for x in g if x >= 0))
        possible += len(w)
    return hits, possible


def audit_counts(emb, feats, doc_location, sample, I, fI, I_desim, k, k_f, thr=1.4, fI_end=31):
    """the audit's integer counts (COUNT_KEYS) for an export whose arrays are I, fI, I_desim ([n, .] ndarrays)"""
    emb, feats = np.asarray(emb, dtype=np.float32), np.asarray(feats, dtype=np.float32)
    sample = np.asarray(sample, dtype=np.int64)
    n = emb.shape[0]
    _, ex, _ = exact_lists(emb, doc_location, sample, k)
    e_hits, e_possible = set_counts(np.asarray(I)[sample], ex)
    U = np.unique(np.concatenate([sample, ex[ex >= 0]]))
    fDx, fIx, _ = oknn.calc_knn_exact(feats, feats[U], k_f)
    at = np.searchsorted(U, sample)
    f_hits, f_possible = set_counts(np.asarray(fI)[sample], fIx[at])
    full_i = np.full((n, k_f), -1, dtype=np.int64)
    full_d = np.full((n, k_f), np.inf, dtype=np.float32)
    full_i[U], full_d[U] = fIx, fDx.astype(np.float32)
    dx = greedy_desim(ex, full_i, full_d, thr, min(fI_end, k_f), query_ids=sample)
    rows_equal = inter = union = 0
    for g, w in zip(np.asarray(I_desim)[sample].tolist(), dx.tolist()):
        g, w = set(x for x in g if x >= 0), set(x for x in w if x >= 0)
        rows_equal += int(g == w)
        inter += len(g & w)
        union += len(g | w)
    return {"audit_rows": int(len(sample)), "union_rows": int(len(U)), "e_hits": e_hits, "e_possible": e_possible,
            "f_hits": f_hits, "f_possible": f_possible, "desim_rows_equal": rows_equal, "desim_kept_intersection": inter,
            "desim_kept_union": union}
