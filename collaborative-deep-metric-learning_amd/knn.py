"""Exact k-nearest-neighbour export behind the reference's ``calc_knn`` signature
(faiss_knn.py:82-131).

The reference l2-normalises the embeddings, builds a faiss ``IndexHNSWFlat`` and
returns ``D`` (squared L2 distances, ascending) and ``I`` (int64 ids; the query
itself is its own first neighbour -- "51 = 50 neighbours + the query").  HNSW is an
approximation of the exact answer; this module computes the exact one by brute
force on the GPU: blocks of inner products ``Q @ Bᵀ`` from the plane kernels
(the headline path's arithmetic, ``ops.gemm_bf16x3_nt``; or the fp32 MFMA GEMM,
``ops.fc_bwd_data`` without a mask), folded into per-query candidate lists by
``ops.knn_merge`` while the 128-MiB score block is still in the Infinity Cache.  Ties are ordered by id.  ``M``,
``efConstruction`` and ``efSearch`` are accepted for call compatibility and ignored.
"""
import numpy as np
import torch

from . import ops

Q_BLOCK = 4096      # query rows per GEMM; 4096 x 8192 scores = 128 MiB stay in the 256 MiB Infinity Cache
B_BLOCK = 8192
# Round 6 (precision "f32x3"): only the FIRST block of the catalogue goes through score blocks -- it gives every query a k-th
# best distance tau -- and the rest through ONE launch of the plane GEMM whose epilogue appends every element within tau to
# its query's candidate list (cdml_knn_filter_x3): no score matrix.  An element of the rest passes with probability
# ~ k / FIRST_BLOCK for exchangeable rows, so a query collects ~ k * (n - FIRST_BLOCK) / FIRST_BLOCK candidates; the lists
# have four times that many slots, and a list that overflows anyway (rows sorted so that later ones are closer) sends the
# whole search back through the score blocks -- nothing is silently lost.
FIRST_BLOCK = 32768


def _round_up(x, m):
    return (x + m - 1) // m * m


def _device_matrix(a, device, row_multiple, col_multiple=32):
    """[n, D] -> zero-padded fp32 device matrix [n_pad, Dp] (Dp % col_multiple == 0)."""
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32)
    n, D = t.shape
    out = torch.zeros((_round_up(n, row_multiple), _round_up(D, col_multiple)), dtype=torch.float32, device=device)
    out[:n, :D] = t
    return out


def _planes(x, Dp):
    out = torch.empty((x.shape[0], 3 * Dp), dtype=torch.bfloat16, device=x.device)
    ops.split_f32_bf16x3(x, out, Dp)
    return out


def _planes_h2(x, Dp):
    """two fp16 planes of x * 2^s, s from the tensor's maximum (a host read: the export is not a step path); (planes, scale)"""
    from .engine_f16x2 import pow2_for
    scale = pow2_for(float(x.abs().amax()), 2.0 ** 13) or 1.0
    out = torch.empty((x.shape[0], 2 * Dp), dtype=torch.float16, device=x.device)
    ops.split_f32_f16x2(x, out, Dp, scale)
    return out, scale


def knn_search(base, queries, k, l2_norm=True, device="cuda:0", q_block=Q_BLOCK, b_block=B_BLOCK, precision="f32x3",
               fused=True, first_block=FIRST_BLOCK, q_chunk=262144, c_chunk=1048576):
    """Device tensors (D [nq,k] fp32 squared L2 ascending, I [nq,k] int64; -1 where
    the catalogue has fewer than k rows).  ``precision``: "f32x3" (default; round 6) = the inner products on the plane
    kernels -- the headline path's arithmetic: every fp32 operand as three exact bf16 planes, six plane products per fp32
    product on the bf16 MFMA (csrc/gemm_bf16x3.hip), errors those of the fp32 kernels -- "f16x2" = two fp16 planes per
    operand under one scale per tensor, three products on the fp16 MFMA (csrc/gemm_f16x2_256.hip; unit rows need no range
    management) -- or "f32" = the fp32 MFMA.
    ``fused`` (precision "f32x3", catalogues of more than two first blocks): everything after the first ``first_block``
    catalogue rows through the filter epilogue instead of score blocks (False: score blocks throughout, the round-5 form);
    ``q_chunk`` queries x ``c_chunk`` catalogue rows per filter launch (operands inside a descriptor's 2 GiB window, candidate
    buffer q_chunk x list capacity x 8 B), the lists merged -- and every query's threshold tightened -- after each.
    Non-finite input: a catalogue row with a NaN coordinate is nobody's neighbour (its distances are NaN, the kernels' clamp
    at 0 keeps a NaN, and a NaN passes no compare); a row with an infinite coordinate has distance NaN or +inf, so it is
    nobody's neighbour either wherever at least k finite rows exist (+inf can still fill a list that would otherwise be
    short).  A non-finite query gets I = -1, D = +inf throughout.  The other results are those of the finite rows alone --
    bit for bit on "f32x3" and "f32"; on "f16x2" the tensor's maximum is then not finite and the planes are split at scale 1
    instead (_planes_h2), which loses precision for rows far below fp16's range."""
    if precision not in ("f32x3", "f32", "f16x2"):
        raise ValueError("precision must be 'f32x3', 'f16x2' or 'f32'")
    h2 = precision == "f16x2"
    x3 = precision == "f32x3" or h2                          # (the plane forms)
    cap = ops.knn_list_capacity()
    if not 1 <= k <= cap:
        raise ValueError("nearest_num must be in [1, %d]" % cap)
    nb, D = base.shape
    nq = queries.shape[0]
    if queries.shape[1] != D:
        raise ValueError("query / catalogue dimension mismatch")
    b_block = _round_up(min(b_block, _round_up(nb, 64)), 256 if x3 else 64)
    colm = 128 if h2 else 64 if x3 else 32
    B = _device_matrix(base, device, b_block, colm)
    same = queries is base
    Q = B if same else _device_matrix(queries, device, 1, colm)
    Dp = B.shape[1]
    if l2_norm:                                              # faiss_knn.py:99-104
        ops.l2norm_fwd(B[:nb], Dp, B)
        if not same:
            ops.l2norm_fwd(Q[:nq], Dp, Q)
    b_sq = torch.zeros(B.shape[0], dtype=torch.float32, device=device)
    ops.row_sqnorm(B[:nb], Dp, b_sq)
    if same:
        q_sq = b_sq
    else:
        q_sq = torch.zeros(nq, dtype=torch.float32, device=device)
        ops.row_sqnorm(Q[:nq], Dp, q_sq)
    best_d = torch.empty((nq, cap), dtype=torch.float32, device=device)
    best_i = torch.empty((nq, cap), dtype=torch.int32, device=device)
    q_block = min(q_block, nq)
    scores = torch.empty((q_block, b_block), dtype=torch.float32, device=device)
    if h2:
        B3, sb = _planes_h2(B, Dp)
        Q3, sq = (B3, sb) if same else _planes_h2(Q, Dp)
        osc = 1.0 / (sq * sb)
    elif x3:
        B3 = _planes(B, Dp)
        Q3 = B3 if same else _planes(Q, Dp)
    n_pad = B.shape[0]
    first_cols = n_pad
    use_filter = x3 and fused and first_block % b_block == 0 and first_block >= 4 * k and nb > 2 * first_block
    if use_filter:
        # a catalogue so long that a query would collect more than ~512 candidates behind a 32 768-row first block gets a
        # longer first block (k n / 512 rows: a 10 M-row catalogue sends 10 % of its rows through score blocks)
        first_cols = min(max(first_block, _round_up(k * nb // 512, b_block)), n_pad)
        use_filter = first_cols + 256 <= n_pad
        if not use_filter:
            first_cols = n_pad
    # queries and catalogue in chunks: a chunk's operands stay inside the 2 GiB window of a buffer descriptor, and the
    # candidate lists of a query chunk inside a bounded buffer
    q_chunk = _round_up(min(q_chunk, nq), q_block) if use_filter else nq
    c_chunk = _round_up(c_chunk, 256)
    lim = (2 ** 31) // (3 * Dp * 2) - 512
    q_chunk, c_chunk = min(q_chunk, lim // q_block * q_block), min(c_chunk, lim // 256 * 256)
    if use_filter:
        list_cap = 64
        expect = k * min(nb - first_cols, c_chunk) / float(first_cols)     # per catalogue chunk: merged and tau tightened after each
        while list_cap < 4 * expect:
            list_cap *= 2
        cnt = torch.zeros(q_chunk, dtype=torch.int32, device=device)
        cand = torch.empty((q_chunk, list_cap, 2), dtype=torch.int32, device=device)
        overflow = torch.zeros(1, dtype=torch.int32, device=device)
    for qs in range(0, nq, q_chunk):
        mq = min(q_chunk, nq - qs)
        for q0 in range(qs, qs + mq, q_block):
            m = min(q_block, qs + mq - q0)
            for c0 in range(0, first_cols, b_block):
                # scores[m, b_block] = Q[q0:q0+m] @ B[c0:c0+b_block]^T
                if h2:
                    ops.gemm_f16x2_nt(ops.BE_F32, Q3[q0:q0 + m], Dp, B3[c0:c0 + b_block], Dp, scores, m, b_block, Dp, osc)
                elif x3:
                    ops.gemm_bf16x3_nt(ops.BE_F32, Q3[q0:q0 + m], Dp, B3[c0:c0 + b_block], Dp, scores, m, b_block, Dp)
                else:
                    ops.fc_bwd_data(Q[q0:q0 + m], B[c0:c0 + b_block], None, scores, m, b_block, Dp)
                ops.knn_merge(scores, m, b_block, c0, nb, q_sq[q0:q0 + m], b_sq[c0:c0 + b_block], k,
                              best_d[q0:q0 + m], best_i[q0:q0 + m], first=(c0 == 0))
        if not use_filter:
            continue
        for c0 in range(first_cols, n_pad, c_chunk):
            nc = min(c_chunk, n_pad - c0)
            tau = best_d[qs:qs + mq, k - 1].contiguous()     # the k-th best so far: every merged chunk tightens it
            if h2:
                ops.knn_filter_h2(Q3[qs:qs + mq], Dp, B3[c0:c0 + nc], Dp, mq, nc, Dp, osc, q_sq[qs:qs + mq], b_sq[c0:c0 + nc], tau, c0,
                                  nb, cnt, cand, list_cap)
            else:
                ops.knn_filter_x3(Q3[qs:qs + mq], Dp, B3[c0:c0 + nc], Dp, mq, nc, Dp, q_sq[qs:qs + mq], b_sq[c0:c0 + nc], tau, c0, nb,
                                  cnt, cand, list_cap)
            ops.knn_merge_list(cand, cnt, list_cap, mq, k, best_d[qs:qs + mq], best_i[qs:qs + mq], overflow)
    if use_filter and int(overflow.item()):                  # (a sync; the export is not a step path)
        return knn_search(base, queries, k, l2_norm=l2_norm, device=device, q_block=q_block, b_block=b_block,
                          precision=precision, fused=False)
    I = best_i[:, :k].to(torch.int64)
    I[I == 0x7fffffff] = -1
    return best_d[:, :k].contiguous(), I


def calc_knn(embeddings, q_embeddings=None, nearest_num=51, l2_norm=True, M=80, efConstruction=64,
             efSearch=32, device="cuda:0", precision="f32x3"):
    """(D, I) ndarrays as faiss ``index.search(q, nearest_num)`` returns them
    (faiss_knn.py:128).  Like the reference, queries default to the catalogue."""
    emb = embeddings if torch.is_tensor(embeddings) else np.asarray(embeddings, dtype=np.float32)
    q = emb if q_embeddings is None else q_embeddings
    D, I = knn_search(emb, q, int(nearest_num), l2_norm=l2_norm, device=device, precision=precision)
    return D.cpu().numpy(), I.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------------
# The rest of faiss_knn.main (faiss_knn.py:134-400): the raw-feature kNN, the cross search, near-duplicate suppression
# ("desim") on the device (csrc/knn_desim.hip) and the text writer.

DESIM_THRESHOLD = 1.4       # faiss_knn.py:187 fD_threshold
DESIM_FI_END = 31           # faiss_knn.py:187 fI_end


def _dev_tensor(a, dtype, device):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype).contiguous()


def _like(out, ref):
    """out (a device tensor) in the kind of ``ref``: a tensor (ref's dtype and device) or an ndarray (ref's dtype)."""
    if torch.is_tensor(ref):
        return out.to(device=ref.device, dtype=ref.dtype)
    return out.cpu().numpy().astype(np.asarray(ref).dtype, copy=False)


def desim(eI, fI, fD, fD_threshold=DESIM_THRESHOLD, fI_end=DESIM_FI_END, query_ids=None, device="cuda:0"):
    """Near-duplicate suppression of kNN lists, the rule of the reference's ``iter_desim_mp`` (faiss_knn.py:187-244) on the
    GPU.  ``eI`` [nq, ke <= 128]: embedding-neighbour ids per query row; ``fI`` / ``fD`` [n_f, kf]: the raw-feature kNN of
    the whole catalogue (ids / squared distances, ``calc_knn(features, ...)``).  Per row, left to right, a neighbour j that
    is still kept removes every LATER kept neighbour found among fI[j, :fI_end] with fD <= fD_threshold (a float32 compare;
    j itself and -1 entries excluded); the query's own id -- ``query_ids[i]``, by default the row index i, the global row
    order of a strict or a cross list -- is removed at the end.  Removed entries become -1.  Ids < 0 or >= n_f in eI are
    never kept.  Returns the kind and dtype of ``eI``."""
    if eI.ndim != 2 or fI.ndim != 2 or tuple(fI.shape) != tuple(fD.shape):
        raise ValueError("eI [nq, ke], fI and fD [n_f, kf] of one shape")
    nq, ke = eI.shape
    n_f, kf = fI.shape
    fI_end = min(int(fI_end), kf)                         # fI[...][:, :f_end] (faiss_knn.py:174)
    if not 1 <= ke <= ops.knn_list_capacity():
        raise ValueError("desim takes at most %d columns" % ops.knn_list_capacity())
    if not 1 <= fI_end <= 64:
        raise ValueError("fI_end must be in [1, 64]")
    if nq == 0:
        return _like(torch.empty((0, ke), dtype=torch.int32), eI)
    e = _dev_tensor(eI, torch.int64, device).clamp(-1, 2 ** 31 - 1).to(torch.int32)
    int32 = fI.dtype == torch.int32 if torch.is_tensor(fI) else np.asarray(fI).dtype == np.int32
    fi = _dev_tensor(fI, torch.int32 if int32 else torch.int64, device)            # (both id types read as they are)
    fd = _dev_tensor(fD, torch.float32, device)
    kp = 32 if fI_end <= 32 else 64
    ff = torch.empty((n_f, kp), dtype=torch.int32, device=device)
    ops.knn_desim_prep(fi, fd, fI_end, float(np.float32(fD_threshold)), ff)
    qid = None if query_ids is None else _dev_tensor(query_ids, torch.int32, device)
    out = torch.empty((nq, ke), dtype=torch.int32, device=device)
    ops.knn_desim(e, ff, out, query_id=qid)
    return _like(out, eI)


def iter_desim_mp(eI, fI, fD, fD_threshold=DESIM_THRESHOLD, fI_end=DESIM_FI_END, process_num=22):
    """The reference's signature (faiss_knn.py:187); ``process_num`` is accepted and ignored (one launch does every row)."""
    return desim(eI, fI, fD, fD_threshold=fD_threshold, fI_end=fI_end)


IVF_STORAGES = ("f32", "f16", "pq")      # IVFIndex.STORAGES / IVFIndex.SCANS, named here for the checks that run before the class exists
IVF_SCANS = ("buffer", "filter")


PQ_M_MIN, PQ_M_MAX, PQ_CODEWORDS = 8, 64, 256     # include/cdml_ivf_pq.h
PQ4_CODEWORDS = 16                                # include/cdml_ivf_pq4.h
PQ_BITS = (4, 8)


def _check_pq_m(storage, pq_m, Dp=None, what="pq_m"):
    """``pq_m`` of an index with ``storage``: None for "f32" / "f16" (anything else is refused), a multiple of 8 in [8, 64]
    that divides ``Dp`` (where known) for "pq".  Pure host arithmetic."""
    if storage != "pq":
        if pq_m is not None:
            raise ValueError("%s belongs to storage=\"pq\" (got storage=%r)" % (what, storage))
        return None
    if pq_m is None:
        raise ValueError("storage=\"pq\" needs pq_m: the bytes per listed row, a multiple of 8 in [%d, %d] that divides Dp"
                         % (PQ_M_MIN, PQ_M_MAX))
    m = int(pq_m)
    if m != pq_m or not PQ_M_MIN <= m <= PQ_M_MAX or m % 8:
        raise ValueError("%s must be a multiple of 8 in [%d, %d], got %r" % (what, PQ_M_MIN, PQ_M_MAX, pq_m))
    if Dp is not None and Dp % m:
        raise ValueError("%s = %d does not divide the padded dimension Dp = %d" % (what, m, Dp))
    return m


def _check_pq_residual(storage, pq_residual):
    """``pq_residual`` of an index with ``storage``: the refusal, by name"""
    if pq_residual and storage != "pq":
        raise ValueError("pq_residual belongs to storage=\"pq\" (got storage=%r)" % (storage,))
    return bool(pq_residual)


def pq_codewords(bits):
    """256 or 16: the codewords of a subspace under ``pq_bits``"""
    return PQ4_CODEWORDS if int(bits) == 4 else PQ_CODEWORDS


def _check_pq_bits(storage, pq_bits, pq_m=None, Dp=None, pq_residual=False):
    """``pq_bits`` of an index with ``storage``: 8 (include/cdml_ivf_pq.h) or 4 (include/cdml_ivf_pq4.h: two codes a byte, 2
    ``pq_m`` subspaces of 16 codewords).  The refusals, by name; pure host arithmetic."""
    if isinstance(pq_bits, bool) or pq_bits not in PQ_BITS:
        raise ValueError("pq_bits must be one of %s, got %r" % (PQ_BITS, pq_bits))
    bits = int(pq_bits)
    if bits != 8 and storage != "pq":
        raise ValueError("pq_bits belongs to storage=\"pq\" (got storage=%r)" % (storage,))
    if bits == 4:
        if pq_residual:
            raise ValueError("pq_bits=4 with pq_residual=True is not built (residual 4-bit codes: DESIGN.md section 10): use "
                             "pq_bits=8 or pq_residual=False")
        if pq_m is not None and Dp is not None and Dp % (2 * int(pq_m)):
            raise ValueError("pq_bits=4 has 2 pq_m = %d subspaces: they do not divide the padded dimension Dp = %d"
                             % (2 * int(pq_m), Dp))
    return bits


def _check_ivf_options(storage, refine, scan, ks=(), pq_m=None, pq_residual=False):
    """The refusals of the IVF options the export's call sites share, by name, before any device work.  ``ks``: the list
    lengths the searches will ask for (a re-rank must keep at least that many)."""
    if storage not in IVF_STORAGES:
        raise ValueError("storage must be one of %s, got %r" % (IVF_STORAGES, storage))
    _check_pq_residual(storage, pq_residual)
    if scan not in IVF_SCANS:
        raise ValueError("scan must be one of %s, got %r" % (IVF_SCANS, scan))
    _check_pq_m(storage, pq_m)
    if storage == "pq" and scan == "filter":
        raise ValueError("scan=\"filter\" (DESIGN.md section 9f.2) has no launch for storage=\"pq\": use scan=\"buffer\"")
    r = int(refine)
    if r != refine or r < 0:
        raise ValueError("refine must be an integer >= 0, got %r" % (refine,))
    if r and storage == "f32":
        raise ValueError("refine belongs to storage=\"f16\" or \"pq\" (the distances of storage=\"f32\" are exact already)")
    if r and ks and not max(ks) <= r <= ops.knn_list_capacity():
        raise ValueError("refine must be 0 or in [k = %d, %d], got %d" % (max(ks), ops.knn_list_capacity(), r))
    return r


def _check_ivf_lists(what, nlist, nprobe, n_rows):
    """(nlist, nprobe) of one index over ``n_rows`` rows: both 0 (the exact search), or 1 <= nprobe <= nlist <= n_rows."""
    nlist, nprobe = int(nlist), int(nprobe)
    if nlist < 0 or nprobe < 0:
        raise ValueError("%snlist and %snprobe must be >= 0, got %d and %d" % (what, what, nlist, nprobe))
    if nlist == 0:
        if nprobe:
            raise ValueError("%snprobe = %d without %snlist: the exact search probes nothing (set %snlist > 0)"
                             % (what, nprobe, what, what))
        return 0, 0
    if nlist > n_rows:
        raise ValueError("%snlist = %d exceeds the %d rows of its index" % (what, nlist, n_rows))
    if not 1 <= nprobe <= nlist:
        raise ValueError("%snprobe must be in [1, %snlist = %d], got %d" % (what, what, nlist, nprobe))
    return nlist, nprobe


def ivf_knn(base, queries=None, k=51, nlist=1024, nprobe=16, l2_norm=True, storage="f32", refine=0, scan="buffer", iters=10,
            seed=0, device="cuda:0", precision="f32x3", index=None, stats=None, pq_m=None, pq_residual=False, pq_bits=8):
    """Device (D, I) of ``IVFIndex.search``, shaped and typed like ``knn_search``'s: the index of ``base`` (built here with
    ``nlist`` lists, ``iters`` Lloyd iterations and ``seed``, or taken as ``index=``), every query's ``nprobe`` nearest lists
    scanned exactly.  ``queries=None`` is the self-search.  ``refine>0`` (storage "f16" or "pq"; "pq" takes ``pq_m``, the
    bytes per listed row, ``pq_residual``: codes of the row minus its list's centroid, DESIGN.md section 9f.4, and ``pq_bits``: 8, or 4 for two 16-codeword codes a byte, section 9f.5) re-ranks the ``refine`` best against the fp32 rows ``index.prepare(base)``.  The one place the export's approximate searches go through; its launches are
    those of DESIGN.md sections 9f-9f.3.  ``stats`` (a dict, optional) receives ``IVFIndex.search``'s."""
    if index is None:
        _check_ivf_options(storage, refine, scan, (int(k),), pq_m, pq_residual)
        _check_pq_bits(storage, pq_bits, pq_m, _round_up(int(base.shape[1]), 32), pq_residual)
        index = IVFIndex.build(base, int(nlist), iters=iters, seed=seed, l2_norm=l2_norm, device=device, precision=precision,
                               storage=storage, pq_m=pq_m, pq_residual=pq_residual, pq_bits=pq_bits)
    q = base if queries is None else queries
    kw = {"refine": int(refine), "base": index.prepare(base)} if int(refine) > 0 else {}
    return index.search(q, int(k), int(nprobe), stats=stats, scan=scan, **kw)


def cross_nlist(nlist, n_side, n):
    """max(1, ceil(nlist n_side / n)): the lists of one side's index of a cross search, so that a list of either side is as
    long on average as a list of ``nlist`` over the whole catalogue.  Pure host arithmetic."""
    nlist, n_side, n = int(nlist), int(n_side), int(n)
    if nlist < 1 or n_side < 1 or n < n_side:
        raise ValueError("cross_nlist needs nlist >= 1 and 1 <= n_side <= n, got %d, %d, %d" % (nlist, n_side, n))
    return max(1, -(-nlist * n_side // n))


def _check_cross_lists(nlist, nprobe, doc_location, n):
    """(nlist, nprobe) of a cross search checked for the whole catalogue and for either side, before any device work"""
    nlist, nprobe = _check_ivf_lists("", nlist, nprobe, n)
    if nlist:
        for n_side in (doc_location, n - doc_location):
            if n_side < 1 or cross_nlist(nlist, n_side, n) > n_side:
                raise ValueError("nlist = %d gives a side of %d rows more lists than rows" % (nlist, n_side))
    return nlist, nprobe


def cross_knn(embeddings, doc_location, nearest_num=81, precision="f32x3", device="cuda:0", nlist=0, nprobe=0, storage="f32",
              refine=0, scan="buffer", ivf_iters=10, ivf_seed=0, stats=None, pq_m=None, pq_residual=False, pq_bits=8):
    """(crossD, crossI) as faiss_knn.py:325-336 builds them: rows [0, doc_location) (videos) search the documents, their
    ids offset by ``doc_location`` into global ids; rows [doc_location, n) (documents) search the videos.  Rows are in
    global order, so the query of row r is r.  The exact search (``knn_search``) stands for the reference's HNSW.  A -1
    ("no neighbour": a side with fewer than nearest_num rows) stays -1 instead of taking the offset.  Returns the kind
    of ``embeddings``.
    ``nlist > 0``: either side is searched through an ``IVFIndex`` of its own (``ivf_knn``) with ``cross_nlist(nlist, n_side,
    n)`` lists, of which min(nprobe, that many) are probed; ``storage``, ``pq_m``, ``pq_residual``, ``pq_bits``, ``refine``, ``scan``, ``ivf_iters`` and ``ivf_seed`` go
    to both.  ``stats`` (a dict, optional) receives the two searches' under "video_to_doc" and "doc_to_video"."""
    t = embeddings if torch.is_tensor(embeddings) else torch.from_numpy(np.asarray(embeddings, dtype=np.float32))
    if int(nlist) or int(nprobe):
        n = t.shape[0]
        nlist, nprobe = _check_cross_lists(nlist, nprobe, int(doc_location), n)
        _check_ivf_options(storage, refine, scan, (int(nearest_num),), pq_m, pq_residual)
        _check_pq_bits(storage, pq_bits, pq_m, _round_up(int(t.shape[1]), 32), pq_residual)
        video, doc = t[:doc_location], t[doc_location:]
        out = []
        for name, base, q in (("video_to_doc", doc, video), ("doc_to_video", video, doc)):
            nl = cross_nlist(nlist, base.shape[0], n)
            st = None if stats is None else stats.setdefault(name, {})
            out.append(ivf_knn(base, q, int(nearest_num), nlist=nl, nprobe=min(nprobe, nl), storage=storage, refine=refine,
                               scan=scan, iters=ivf_iters, seed=ivf_seed, device=device, precision=precision, stats=st,
                               pq_m=pq_m, pq_residual=pq_residual, pq_bits=pq_bits))
        (vdD, vdI), (dvD, dvI) = out
        vdI = torch.where(vdI >= 0, vdI + doc_location, vdI)
        D, I = torch.cat([vdD, dvD]), torch.cat([vdI, dvI])
        if torch.is_tensor(embeddings):
            return D, I
        return D.cpu().numpy(), I.cpu().numpy()
    _check_ivf_options(storage, refine, scan, pq_m=pq_m, pq_residual=pq_residual)
    _check_pq_bits(storage, pq_bits, pq_residual=pq_residual)
    if storage != "f32" or int(refine) or scan != "buffer":
        raise ValueError("storage, refine and scan belong to nlist > 0 (this search is exact)")
    video, doc = t[:doc_location], t[doc_location:]
    vdD, vdI = knn_search(doc, video, int(nearest_num), device=device, precision=precision)
    vdI = torch.where(vdI >= 0, vdI + doc_location, vdI)
    dvD, dvI = knn_search(video, doc, int(nearest_num), device=device, precision=precision)
    D, I = torch.cat([vdD, dvD]), torch.cat([vdI, dvI])
    if torch.is_tensor(embeddings):
        return D, I
    return D.cpu().numpy(), I.cpu().numpy()


def load_decode_map(path):
    """(decode_map {int row: guid}, encode_map {guid: int row}) from the export's JSON (faiss_knn.py:52-61)."""
    import json
    with open(path, "r") as f:
        index2guid = json.load(f)
    decode_map, encode_map = {}, {}
    for k, v in index2guid.items():
        decode_map[int(k)] = v
        encode_map[v] = int(k)
    return decode_map, encode_map


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


WRITERS = ("host", "device")
WRITER_BUFFER_BYTES = 1 << 30   # the device writer's output buffer: a part longer than this goes out in row ranges of at most so many bytes


def _part_text_host(D, I, b, e, decode_map, row0=None):
    """the text of rows [b, e) of D / I as write_knn writes them, formatted on the host (one numpy str() pass for the part);
    the rows are rows ``row0`` (default b) and up of the catalogue"""
    row0 = b if row0 is None else row0
    Dt = D[b:e, 1:].astype(np.float32, copy=False)
    It = I[b:e, 1:].astype(np.int64, copy=False)
    m = (It > 0) & (Dt > np.float32(0.0)) & (Dt < np.float32(1.4))        # the float32 compares numpy makes
    ds = Dt[m].astype(str).tolist()                  # one call for the part: numpy's str of a float32 is its shortest repr
    ids = It[m].tolist()
    ends = np.cumsum(m.sum(1)).tolist()
    lines, p = [], 0
    for r, q in zip(range(row0, row0 + e - b), ends):
        lines.append(decode_map[r] + "," + "".join([decode_map[ids[t]] + "#" + ds[t] + "<" for t in range(p, q)]) + "\n")
        p = q
    return "".join(lines)


def guid_table(decode_map, device="cuda:0"):
    """(guid_bytes uint8 [total + 1], guid_off int64 [n + 1]) on ``device``: the utf-8 bytes of decode_map[0 .. n - 1], one
    after the other, and where each starts (include/cdml_knn_writer.h; the last byte is a pad, so that a table of empty
    guids still has an address).  ``decode_map``: a sequence, or a dict whose keys are exactly 0 .. n - 1."""
    n = len(decode_map)
    try:
        enc = [decode_map[i].encode("utf-8") for i in range(n)]
    except (KeyError, IndexError):
        raise ValueError("writer=\"device\" needs a decode_map with the keys 0 .. %d" % (n - 1))
    off = np.zeros(n + 1, dtype=np.int64)
    if n:
        off[1:] = np.cumsum(np.fromiter((len(b) for b in enc), dtype=np.int64, count=n))
    data = np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(data).to(device), torch.from_numpy(off).to(device)


def _write_knn_device(out_dir, D, I, decode_map, split_num, prefix, device, buffer_bytes, stats):
    import os
    n, k = D.shape
    if not 1 <= k <= ops.knn_list_capacity():
        raise ValueError("writer=\"device\" takes at most %d columns, got %d" % (ops.knn_list_capacity(), k))
    gbytes, goff = guid_table(decode_map, device)
    n_guid = goff.numel() - 1
    if n > n_guid:
        raise ValueError("decode_map names %d rows, the lists have %d" % (n_guid, n))
    Dd = _dev_tensor(D, torch.float32, device)
    Id = _dev_tensor(I, torch.int64, device)
    patch = n // split_num
    host_parts = launches = 0
    for s in range(split_num):
        b = s * patch
        e = n if s == split_num - 1 else (s + 1) * patch
        path = os.path.join(out_dir, prefix + str(s))
        if e <= b:
            open(path, "wb").close()
            continue
        Dp, Ip = Dd[b:e], Id[b:e]
        sizes = torch.empty(e - b, dtype=torch.int64, device=device)
        flags = torch.empty(e - b, dtype=torch.int32, device=device)
        ops.knn_line_sizes(Dp, Ip, b, goff, gbytes.numel(), sizes, flags)
        off = torch.zeros(e - b + 1, dtype=torch.int64, device=device)
        off[1:] = torch.cumsum(sizes, 0)
        lost = ((Ip[:, 1:] >= n_guid) & (Dp[:, 1:] > 0.0) & (Dp[:, 1:] < float(np.float32(1.4)))).any()
        n_flag, n_lost = torch.stack([flags.sum(), lost.to(torch.int64)]).tolist()       # the host read
        if n_lost:
            raise ValueError("a kept neighbour id is not in decode_map (%d guids)" % n_guid)
        if n_flag:              # a kept distance below the digit routine's range: this part is formatted on the host
            host_parts += 1
            with open(path, "w", encoding="utf-8", newline="\n") as f:
                f.write(_part_text_host(Dp.cpu().numpy(), Ip.cpu().numpy(), 0, e - b, decode_map, row0=b))
            continue
        off_h = off.cpu().numpy()
        with open(path, "wb") as f:
            r0 = 0
            while r0 < e - b:
                # the longest row range from r0 within the buffer (one row at least: a longer line gets a buffer of its own)
                r1 = int(np.searchsorted(off_h, off_h[r0] + int(buffer_bytes), side="right")) - 1
                r1 = min(max(r1, r0 + 1), e - b)
                nbytes = int(off_h[r1] - off_h[r0])
                out = torch.empty(nbytes, dtype=torch.uint8, device=device)
                ops.knn_line_write(Dp[r0:r1], Ip[r0:r1], b + r0, gbytes, goff,
                                   off if (r0, r1) == (0, e - b) else (off[r0:r1 + 1] - off[r0]).contiguous(), out)
                launches += 1
                f.write(memoryview(out.cpu().numpy()))
                r0 = r1
    if stats is not None:
        stats.update(writer="device", host_parts=host_parts, write_launches=launches)


def write_knn(out_dir, D, I, decode_map, split_num=10, prefix="knn_result", writer="host", device="cuda:0",
              buffer_bytes=WRITER_BUFFER_BYTES, stats=None):
    """The text lists of faiss_knn.py:267-305 (``write_knn`` / ``write_process``), byte for byte: ``split_num`` files
    ``prefix + str(index)``, parts of ``n // split_num`` rows, the remainder in the last one.  A line is
    ``decode_map[row] + "," + "".join(decode_map[id] + "#" + str(d) + "<")`` over columns 1.. where id > 0 and
    0.0 < d < 1.4 (d a float32, printed as its shortest repr).  Reproduced as the reference has them: column 0 is skipped
    in every mode (in a cross list it is a real neighbour), and catalogue row 0 never appears as a neighbour (id > 0).
    ``decode_map`` is an argument (the reference's workers read a global its ``main`` never sets).
    ``writer="device"`` (csrc/knn_writer.hip) writes the same bytes: per part, one launch sizes
    every line, an int64 scan places them, one launch formats them into a byte buffer (at most ``buffer_bytes`` per launch)
    and the part is copied out and written as it is.  A part with a kept distance outside the digit routine's range
    (below 2^-64) is formatted on the host instead.  ``stats`` (a dict, optional) receives ``host_parts`` and
    ``write_launches``."""
    import os
    if writer not in WRITERS:
        raise ValueError("writer must be one of %s, got %r" % (WRITERS, writer))
    if writer == "device":
        D, I = (a if torch.is_tensor(a) else np.asarray(a) for a in (D, I))
        if tuple(D.shape) != tuple(I.shape) or len(D.shape) != 2:
            raise ValueError("D and I of one shape [n, k]")
        os.makedirs(out_dir, exist_ok=True)
        return _write_knn_device(out_dir, D, I, decode_map, int(split_num), prefix, device, buffer_bytes, stats)
    D, I = _host(D), _host(I)
    if D.shape != I.shape or D.ndim != 2:
        raise ValueError("D and I of one shape [n, k]")
    os.makedirs(out_dir, exist_ok=True)
    n = D.shape[0]
    patch = n // split_num
    for s in range(split_num):
        b = s * patch
        e = n if s == split_num - 1 else (s + 1) * patch
        with open(os.path.join(out_dir, prefix + str(s)), "w", encoding="utf-8", newline="\n") as f:
            f.write(_part_text_host(D, I, b, e, decode_map))


def audit_sample(n, audit_rows, audit_seed=0):
    """The rows the export's audit looks at: the first ``audit_rows`` entries of a seeded CPU ``torch.randperm(n)``, sorted
    (int64, CPU)."""
    g = torch.Generator()
    g.manual_seed(int(audit_seed))
    return torch.sort(torch.randperm(int(n), generator=g)[:int(audit_rows)]).values


def _set_counts(got, want):
    """(hits, possible) = (sum over rows of |got[r] & want[r]|, the number of entries of want) over the entries >= 0"""
    hits = possible = 0
    for g, w in zip(got.tolist(), want.tolist()):
        w = set(x for x in w if x >= 0)
        hits += len(w & set(x for x in g if x >= 0))
        possible += len(w)
    return hits, possible


def _export_audit(emb, features, doc_location, cross, sample, I, fI, I_desim, k, k_f, fD_threshold, fI_end, precision, device):
    """The recall statement of an export, integer counts only: what the export's lists of the
    ``sample`` rows share with the exact search's, for the embedding lists, the raw-feature lists and the desimmed lists."""
    n = emb.shape[0]
    smp = sample.to(device)
    if cross:
        ex = torch.full((smp.numel(), k), -1, dtype=torch.int64, device=device)
        is_video = smp < doc_location
        for rows, base, shift in ((is_video, emb[doc_location:], doc_location), (~is_video, emb[:doc_location], 0)):
            if bool(rows.any()):
                _, Ie = knn_search(base, emb[smp[rows]], k, device=device, precision=precision)
                ex[rows] = torch.where(Ie >= 0, Ie + shift, Ie)
    else:
        _, ex = knn_search(emb, emb[smp], k, device=device, precision=precision)
    e_hits, e_possible = _set_counts(I[smp].cpu(), ex.cpu())
    U = torch.unique(torch.cat([smp, ex[ex >= 0]]))                     # sorted
    feats = features if torch.is_tensor(features) else torch.from_numpy(np.asarray(features, dtype=np.float32))
    fDx, fIx = knn_search(feats, feats[U.to(feats.device)], k_f, device=device, precision=precision)
    at = torch.searchsorted(U, smp)                                     # the sample's rows of U
    f_hits, f_possible = _set_counts(_dev_tensor(fI, torch.int64, device)[smp].cpu(), fIx[at].cpu())
    full_i = torch.full((n, k_f), -1, dtype=torch.int64, device=device)
    full_d = torch.full((n, k_f), float("inf"), dtype=torch.float32, device=device)
    full_i[U], full_d[U] = fIx, fDx
    dx = desim(ex, full_i, full_d, fD_threshold=fD_threshold, fI_end=fI_end, query_ids=smp, device=device)
    rows_equal = inter = union = 0
    for g, w in zip(I_desim[smp].cpu().tolist(), dx.cpu().tolist()):
        g, w = set(x for x in g if x >= 0), set(x for x in w if x >= 0)
        rows_equal += int(g == w)
        inter += len(g & w)
        union += len(g | w)
    return {"audit_rows": int(smp.numel()), "union_rows": int(U.numel()), "e_hits": e_hits, "e_possible": e_possible,
            "f_hits": f_hits, "f_possible": f_possible, "desim_rows_equal": rows_equal, "desim_kept_intersection": inter,
            "desim_kept_union": union}


def _load_feature_knn(feature_knn, n):
    """(fD, fI) of ``feature_knn`` -- a pair of arrays, or a directory that holds fD.npy and fI.npy -- checked by name"""
    import os
    if isinstance(feature_knn, (str, os.PathLike)):
        feature_knn = (np.load(os.path.join(feature_knn, "fD.npy")), np.load(os.path.join(feature_knn, "fI.npy")))
    try:
        fD, fI = feature_knn
        shapes = (tuple(fD.shape), tuple(fI.shape))
    except (TypeError, ValueError, AttributeError):
        raise ValueError("feature_knn must be a pair (fD, fI) of arrays or a directory that holds fD.npy and fI.npy")
    if shapes[0] != shapes[1] or len(shapes[0]) != 2 or shapes[0][0] != n or shapes[0][1] < 1:
        raise ValueError("feature_knn must be two [n = %d, >= 1] arrays of one shape, got %s and %s" % (n, shapes[0], shapes[1]))
    return fD, fI


def _scalars(st):
    """the host numbers of an ``IVFIndex.search`` stats dict (its device tensors stay out of a report)"""
    out = {}
    for key, v in st.items():
        if isinstance(v, dict):
            out[key] = _scalars(v)
        elif key == "chunks":
            out["n_chunks"] = len(v)
        elif isinstance(v, (int, float, str)):
            out[key] = v
    return out


def export(embeddings, features, decode_map, out_dir, doc_location=343455, nearest_num=81, desim_nearest_num=26,
           fD_threshold=DESIM_THRESHOLD, fI_end=DESIM_FI_END, precision="f32x3", device="cuda:0", split_num=10,
           nlist=0, nprobe=0, feature_nlist=0, feature_nprobe=0, storage="f32", refine=0, scan="buffer", ivf_iters=10,
           ivf_seed=0, feature_knn=None, writer="host", audit_rows=0, audit_seed=0, stats=None, pq_m=None, feature_pq_m=None,
           pq_residual=False, pq_bits=8):
    """faiss_knn.main (faiss_knn.py:359-400) with explicit arguments: the raw-feature kNN (fD, fI; k = min(desim_nearest_num,
    nearest_num)), then -- cross mode when 0 < doc_location < n, strict mode otherwise -- the embedding kNN, desim and the
    text lists.  Writes fD.npy, fI.npy, {strict,cross}D.npy, {strict,cross}I.npy, {strict,cross}I_desim.npy, the
    ``split_num`` text files {strict,cross}_knn<i> and decode_map.json.  The text lists are written from the DESIMMED ids
    in both modes (the reference's cross branch writes the un-desimmed crossI: faiss_knn.py:350, marked TODO; crossI.npy
    keeps those).  Returns (D, I_desim) as device tensors.

    At catalogue scale; every default keeps the exact path and its bytes:
    ``nlist`` / ``nprobe``: the embedding search through ``ivf_knn`` (strict) or ``cross_knn(nlist=...)`` (cross: an index per
    side).  ``feature_nlist`` / ``feature_nprobe``: the raw-feature search through ``ivf_knn``, independently.  ``storage``,
    ``refine``, ``scan``, ``ivf_iters``, ``ivf_seed`` go to every index; with ``storage="pq"`` the embedding indexes take ``pq_m``
    and the raw-feature index ``feature_pq_m`` (default: ``pq_m``), and ``pq_residual`` and ``pq_bits`` go to every pq index.  ``feature_knn``: (fD, fI) or a directory holding
    fD.npy / fI.npy of an earlier export -- raw features do not change when the model is retrained -- written as given, no
    feature search (``features`` may then be None unless the audit needs them).  ``writer``: "host" | "device"
    (``write_knn``).  ``audit_rows = m > 0``: the recall statement -- for the rows ``audit_sample(n, m, audit_seed)`` the
    exact searches are run and the export's lists compared with them; integer counts, written to export_audit.json and
    ``stats["audit"]``, no threshold.  ``stats`` (a dict, optional): per stage {"seconds", "max_memory_allocated"} and the
    ``IVFIndex.search`` numbers.  Bad combinations are ValueErrors raised before any device work."""
    import json
    import os
    import time
    n = embeddings.shape[0]
    k, k_f = int(nearest_num), min(int(desim_nearest_num), int(nearest_num))
    cross = 0 < doc_location < n
    # ---- the refusals, before any device work ----
    if writer not in WRITERS:
        raise ValueError("writer must be one of %s, got %r" % (WRITERS, writer))
    nlist, nprobe = _check_cross_lists(nlist, nprobe, int(doc_location), n) if cross else _check_ivf_lists("", nlist, nprobe, n)
    feature_nlist, feature_nprobe = _check_ivf_lists("feature_", feature_nlist, feature_nprobe, n)
    refine = _check_ivf_options(storage, refine, scan, ((k,) if nlist else ()) + ((k_f,) if feature_nlist else ()), pq_m,
                                pq_residual)
    pq_bits = _check_pq_bits(storage, pq_bits, pq_residual=pq_residual)
    feature_pq_m = _check_pq_m(storage, pq_m if feature_pq_m is None else feature_pq_m, what="feature_pq_m")
    if nlist:                                                 # (2 pq_m subspaces must divide either index's padded dimension)
        _check_pq_bits(storage, pq_bits, pq_m, _round_up(int(embeddings.shape[1]), 32), pq_residual)
    if feature_nlist and features is not None and feature_knn is None:
        _check_pq_bits(storage, pq_bits, feature_pq_m, _round_up(int(features.shape[1]), 32), pq_residual)
    if not (nlist or feature_nlist) and (storage != "f32" or refine or scan != "buffer"):
        raise ValueError("storage, refine and scan belong to an IVF search: set nlist or feature_nlist (both are 0)")
    if feature_knn is not None:
        if feature_nlist:
            raise ValueError("feature_knn and feature_nlist > 0 exclude each other: the given lists are written as they are")
        feature_knn = _load_feature_knn(feature_knn, n)
    elif features is None:
        raise ValueError("features is None and no feature_knn was given")
    audit_rows = int(audit_rows)
    if not 0 <= audit_rows <= n:
        raise ValueError("audit_rows must be in [0, n = %d], got %d" % (n, audit_rows))
    if audit_rows and features is None:
        raise ValueError("the audit runs the exact raw-feature search: it needs features")
    ivf = {"storage": storage, "refine": refine, "scan": scan}
    pq = {"pq_m": int(pq_m), "feature_pq_m": feature_pq_m} if storage == "pq" else {}
    pqr = {"pq_residual": True} if pq_residual else {}        # (absent when off: the stats of a plain export keep their keys)
    if int(pq_bits) != 8:
        pqr["pq_bits"] = int(pq_bits)                         # (absent at 8, for the same reason)

    def stage(name, t0, extra=None):
        if stats is not None:
            torch.cuda.synchronize(device)
            stats[name] = dict(extra or {}, seconds=time.perf_counter() - t0,
                               max_memory_allocated=torch.cuda.max_memory_allocated(device))
        return time.perf_counter()

    os.makedirs(out_dir, exist_ok=True)
    t0 = time.perf_counter()
    if feature_knn is not None:
        fD, fI = feature_knn
    elif feature_nlist:
        st = {}
        fD, fI = ivf_knn(features, None, k_f, nlist=feature_nlist, nprobe=feature_nprobe, iters=ivf_iters, seed=ivf_seed,
                         device=device, precision=precision, stats=st, pq_m=pq.get("feature_pq_m"), **ivf, **pqr)
        t0 = stage("feature_knn", t0, {"ivf": _scalars(st)})
    else:
        fD, fI = knn_search(features, features, k_f, device=device, precision=precision)
        t0 = stage("feature_knn", t0)
    np.save(os.path.join(out_dir, "fD.npy"), _host(fD))
    np.save(os.path.join(out_dir, "fI.npy"), _host(fI))
    emb = embeddings if torch.is_tensor(embeddings) else torch.from_numpy(np.asarray(embeddings, dtype=np.float32))
    t0 = time.perf_counter()
    st = {}
    if cross:
        mode = "cross"
        if nlist:
            D, I = cross_knn(emb.to(device), doc_location, nearest_num=nearest_num, precision=precision, device=device,
                             nlist=nlist, nprobe=nprobe, ivf_iters=ivf_iters, ivf_seed=ivf_seed, stats=st, pq_m=pq.get("pq_m"),
                             **ivf, **pqr)
        else:
            D, I = cross_knn(emb.to(device), doc_location, nearest_num=nearest_num, precision=precision, device=device)
    else:
        mode = "strict"
        if nlist:
            D, I = ivf_knn(emb, None, k, nlist=nlist, nprobe=nprobe, iters=ivf_iters, seed=ivf_seed, device=device,
                           precision=precision, stats=st, pq_m=pq.get("pq_m"), **ivf, **pqr)
        else:
            D, I = knn_search(emb, emb, int(nearest_num), device=device, precision=precision)
    t0 = stage("embedding_knn", t0, {"ivf": _scalars(st)} if nlist else None)
    np.save(os.path.join(out_dir, mode + "D.npy"), D.cpu().numpy())
    np.save(os.path.join(out_dir, mode + "I.npy"), I.cpu().numpy())
    t0 = time.perf_counter()
    I_desim = desim(I, fI, fD, fD_threshold=fD_threshold, fI_end=fI_end, device=device)
    t0 = stage("desim", t0)
    np.save(os.path.join(out_dir, mode + "I_desim.npy"), I_desim.cpu().numpy())
    t0 = time.perf_counter()
    if writer == "host":
        write_knn(out_dir, D, I_desim, decode_map, split_num=split_num, prefix=mode + "_knn")
        t0 = stage("write", t0, {"writer": "host"})
    else:
        st = {}
        write_knn(out_dir, D, I_desim, decode_map, split_num=split_num, prefix=mode + "_knn", writer=writer, device=device,
                  stats=st)
        t0 = stage("write", t0, st)
    dm = decode_map if isinstance(decode_map, dict) else dict(enumerate(decode_map))
    with open(os.path.join(out_dir, "decode_map.json"), "w") as f:
        json.dump({str(k): v for k, v in dm.items()}, f)
    if audit_rows:
        t0 = time.perf_counter()
        counts = _export_audit(emb.to(device), features, int(doc_location), cross, audit_sample(n, audit_rows, audit_seed), I, fI,
                               I_desim, k, k_f, fD_threshold, fI_end, precision, device)
        report = dict(counts, mode=mode, n=n, doc_location=int(doc_location), nearest_num=k, desim_nearest_num=k_f,
                      fD_threshold=float(fD_threshold), fI_end=int(fI_end), precision=precision, nlist=nlist, nprobe=nprobe,
                      feature_nlist=feature_nlist, feature_nprobe=feature_nprobe, ivf_iters=int(ivf_iters), ivf_seed=int(ivf_seed),
                      feature_knn_given=feature_knn is not None, audit_seed=int(audit_seed), **ivf, **pq, **pqr)
        with open(os.path.join(out_dir, "export_audit.json"), "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
        stage("audit", t0)
        if stats is not None:
            stats["audit"].update(report)
    return D, I_desim


# ----------------------------------------------------------------------------------------------------------------------------
# The approximate path: an inverted-file (IVF-Flat) index (include/cdml_ivf.h, csrc/ivf.hip).  k-means
# cuts the catalogue into nlist lists; a query is scored only against the rows of its nprobe nearest lists.  ``calc_knn``
# stays exact and keeps ignoring its HNSW arguments.

IVF_TILE = 128              # slots x rows per work item of the grouped score product (csrc/ivf.hip kTile)
IVF_SCORE_BYTES = 1 << 30   # default budget of a query chunk's ragged score buffer: 1 GiB, or ...
IVF_SCORE_SLOTS = 512       # ... IVF_SCORE_SLOTS score rows per list and chunk (4 B x 512 x n_listed), whichever is more: a chunk of
#                             B score bytes holds B / (4 n_listed) slots per list whatever nlist and nprobe are, and a 128-slot tile of
#                             the scan is as full as that allows (1 GiB at 10 M rows: 27 slots, four fifths of the product padding)


def ivf_plan_chunks(costs, score_bytes, max_queries=None):
    """Query chunks [(q0, q1), ...] in order, each chunk's scores within ``score_bytes``: ``costs[q]`` = the score FLOATS of
    query q (the padded lengths of its probed lists).  Every query is in exactly one chunk; a chunk holds at most
    ``max_queries`` queries; a query whose own scores exceed the budget is refused.  Pure host arithmetic."""
    c = np.asarray(costs, dtype=np.int64).reshape(-1)
    budget = int(score_bytes) // 4
    if c.size and int(c.max()) > budget:
        q = int(c.argmax())
        raise ValueError("score_bytes = %d is less than the %d bytes of query %d's own scores: raise score_bytes or lower nprobe"
                         % (int(score_bytes), 4 * int(c[q]), q))
    cum = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(c)])
    chunks, q0, n = [], 0, int(c.size)
    while q0 < n:
        q1 = int(np.searchsorted(cum, cum[q0] + budget, side="right")) - 1    # the last q1 with cum[q1] - cum[q0] <= budget
        if max_queries is not None:
            q1 = min(q1, q0 + int(max_queries))
        q1 = min(max(q1, q0 + 1), n)
        chunks.append((q0, q1))
        q0 = q1
    return chunks


def ivf_tables(probe, list_len, tile_slots=IVF_TILE, tile_rows=IVF_TILE):
    """The slot, tile and offset tables of one query chunk (plumbing: torch calls on ``probe``'s device, ONE host read).
    probe int32 [m, nprobe] (-1 = no list); list_len int64 [nlist].  A slot is one (query, probed list) pair; slots are
    sorted by list (stably: by query inside a list).  Returns a dict: n_slots, n_floats, n_tiles (ints), slot_query int32
    [n_slots], slot_start int32 [nlist + 1], slot_off int64 [n_slots], slot_of int32 [m, nprobe] (-1 for a -1 probe), tiles
    int32 [n_tiles, 4] = (list, first slot in the list's block, first row in the list, 0), ordered by list.  A tile is
    ``tile_slots`` x ``tile_rows`` (the MFMA scans' 128 x 128; the PQ scan's ``ops.ivf_pq_tile(M)``)."""
    tile_slots, tile_rows = int(tile_slots), int(tile_rows)
    m, nprobe = probe.shape
    nlist = list_len.numel()
    dev = probe.device
    flat = probe.reshape(-1).to(torch.int64)
    key = torch.where(flat >= 0, flat, torch.full_like(flat, nlist))
    skey, order = torch.sort(key, stable=True)
    cnt = torch.bincount(key, minlength=nlist + 1)[:nlist]
    slot_start = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
    slot_start[1:] = torch.cumsum(cnt, 0)
    ld = (list_len + 3) // 4 * 4
    blk = cnt * ld                                            # floats of list c's score block [cnt][ld]
    blk_off = torch.cumsum(blk, 0) - blk
    tn = (list_len + tile_rows - 1) // tile_rows
    nt = (cnt + tile_slots - 1) // tile_slots * tn
    tile_start = torch.cumsum(nt, 0) - nt
    n_slots, n_floats, n_tiles = torch.stack([slot_start[-1], blk.sum(), nt.sum()]).tolist()      # the host read
    slot_list = skey[:n_slots]
    slot_of = torch.full((m * nprobe,), -1, dtype=torch.int32, device=dev)
    slot_of[order[:n_slots]] = torch.arange(n_slots, dtype=torch.int32, device=dev)
    slot_off = blk_off[slot_list] + (torch.arange(n_slots, device=dev) - slot_start[slot_list]) * ld[slot_list]
    tc = torch.repeat_interleave(torch.arange(nlist, device=dev), nt, output_size=n_tiles)
    loc = torch.arange(n_tiles, device=dev) - tile_start[tc]
    tnc = tn[tc].clamp(min=1)
    tiles = torch.stack([tc, loc // tnc * tile_slots, loc % tnc * tile_rows, torch.zeros_like(tc)], 1).to(torch.int32).contiguous()
    return {"n_slots": n_slots, "n_floats": n_floats, "n_tiles": n_tiles,
            "slot_query": (order[:n_slots] // nprobe).to(torch.int32), "slot_start": slot_start.to(torch.int32),
            "slot_off": slot_off, "slot_of": slot_of.view(m, nprobe), "tiles": tiles}


def pq_query_floats(pq_m, nprobe=0, bits=8):
    """256 M (``bits=4``: 2 M tables of 16 = 32 M): the floats of one query's lookup table, what a query of a pq index costs a
    chunk beside its scores; a residual index (``pq_residual``) adds its ``nprobe`` slot scalars"""
    return (2 * PQ4_CODEWORDS if int(bits) == 4 else PQ_CODEWORDS) * int(pq_m) + int(nprobe)


PQ_TRAIN_ROWS = 65536       # default training rows of pq_train (256 per codeword)
PQ4_TRAIN_ROWS = 4096       # ... with bits=4 (256 per codeword again)


def _check_pq_train(n_finite, iters, train_rows, bits=8):
    """(n_train, iters) of ``pq_train``: the refusals, by name"""
    iters = int(iters)
    K = pq_codewords(bits)
    if iters < 0:
        raise ValueError("pq_iters must be >= 0, got %d" % iters)
    if n_finite < K:
        raise ValueError("storage=\"pq\" needs at least %d finite rows to start its codebooks from, got %d" % (K, n_finite))
    n_train = min(n_finite, PQ4_TRAIN_ROWS if K == PQ4_CODEWORDS else PQ_TRAIN_ROWS) if train_rows is None else int(train_rows)
    if not K <= n_train <= n_finite:
        raise ValueError("pq_train_rows must be in [%d, the number of finite rows = %d], got %d" % (K, n_finite, n_train))
    return n_train, iters


def pq_train(X_prepared, pq_m, iters=10, seed=0, train_rows=None, centroids=None, assign=None):
    """(codebooks fp32 [M, 256, Dp / M] on X's device, pq_objective float64 [M, iters] on the CPU): the deterministic Lloyd's of
    ``IVFIndex.build`` per subspace (include/cdml_ivf_pq.h).  ``X_prepared``: the fp32 device matrix [n, Dp] of
    ``IVFIndex.prepare``.  The training rows are the (sorted) first ``train_rows`` ids of the seeded CPU permutation of the
    finite rows (default min(n_finite, 65 536)); every subspace's 256 initial codewords are the sub-vectors of the sorted
    first 256 ids.  An iteration encodes the training rows (``ops.pq_encode``) and replaces every non-empty codeword by the
    mean of its rows (``ops.ivf_centroid_sums``, rows ordered by (code, id)); an empty codeword keeps its value.
    pq_objective[m, t] = the sum of iteration t's attained distances in subspace m.
    ``centroids`` (fp32 [nlist, Dp], the padded matrix) and ``assign`` (int64 [n]) together: the same Lloyd's on the
    RESIDUALS x - centroids[assign] of the same rows (include/cdml_ivf_pqr.h; one fp32 subtract per column, materialised
    for the training rows only); every finite row then needs an assign in [0, nlist)."""
    return _pq_lloyd(X_prepared, pq_m, iters, seed, train_rows, centroids, assign, 8)


def pq4_train(X_prepared, pq_m, iters=10, seed=0, train_rows=None):
    """``pq_train`` for ``pq_bits=4`` (include/cdml_ivf_pq4.h): the same deterministic Lloyd's over Ms = 2 ``pq_m`` subspaces of 16
    codewords -- (codebooks fp32 [2 M, 16, Dp / (2 M)], pq_objective float64 [2 M, iters]); the initial codewords are the
    sub-vectors of the sorted first 16 ids of the seeded permutation, the default training rows min(n_finite, 4 096) (256 per
    codeword, as 65 536 is for 256), at least 16 finite rows are needed, the encoder is ``ops.pq4_encode``, an empty codeword
    keeps its value.  Plain codebooks only: residual 4-bit codes are not built."""
    return _pq_lloyd(X_prepared, pq_m, iters, seed, train_rows, None, None, 4)


def _pq_lloyd(X_prepared, pq_m, iters, seed, train_rows, centroids, assign, bits):
    """``pq_train`` (bits = 8) and ``pq4_train`` (bits = 4)"""
    X = X_prepared
    if (centroids is None) != (assign is None):
        raise ValueError("pq_train takes centroids and assign together (residual codebooks) or neither (plain codebooks)")
    if not torch.is_tensor(X) or X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1:
        raise ValueError("pq_train takes the prepared fp32 [n, Dp] matrix (IVFIndex.prepare)")
    n, Dp = X.shape
    M = _check_pq_m("pq", pq_m, Dp)
    _check_pq_bits("pq", bits, M, Dp)
    K = pq_codewords(bits)
    Ms = 2 * M if bits == 4 else M                        # subspaces; M stays the bytes per row
    dsub = Dp // Ms
    dev = X.device
    fin = torch.nonzero(torch.isfinite(X).all(1)).flatten().cpu()
    n_finite = int(fin.numel())
    n_train, iters = _check_pq_train(n_finite, iters, train_rows, bits)
    g = torch.Generator()
    g.manual_seed(int(seed))
    perm = torch.randperm(n_finite, generator=g)
    init_rows = torch.sort(fin[perm[:K]]).values
    train_ids = torch.sort(fin[perm[:n_train]]).values
    Xt = X if n_train == n else X.index_select(0, train_ids.to(dev))
    X0 = X.index_select(0, init_rows.to(dev))
    if centroids is not None:
        Cp, a = centroids, assign
        if not torch.is_tensor(Cp) or Cp.dtype != torch.float32 or Cp.dim() != 2 or Cp.shape[1] != Dp \
                or not torch.is_tensor(a) or a.dtype != torch.int64 or tuple(a.shape) != (n,):
            raise ValueError("pq_train takes centroids fp32 [nlist, Dp = %d] and assign int64 [n = %d]" % (Dp, n))
        Cp, a = Cp.to(dev), a.to(dev)
        a_fin = a.index_select(0, fin.to(dev))
        if int(a_fin.min()) < 0 or int(a_fin.max()) >= Cp.shape[0]:
            raise ValueError("pq_train: every finite row needs an assign in [0, nlist = %d)" % Cp.shape[0])
        Xt = X.index_select(0, train_ids.to(dev)) - Cp.index_select(0, a.index_select(0, train_ids.to(dev)))
        X0 = X0 - Cp.index_select(0, a.index_select(0, init_rows.to(dev)))
    cb = X0.view(K, Ms, dsub).permute(1, 0, 2).contiguous()
    codes = torch.empty((n_train, M), dtype=torch.uint8, device=dev)
    dist = torch.empty((n_train, Ms), dtype=torch.float32, device=dev)
    objective = torch.zeros((Ms, iters), dtype=torch.float64)
    for it in range(iters):
        if bits == 4:
            ops.pq4_encode(Xt, cb, codes, dist)
        else:
            ops.pq_encode(Xt, cb, codes, dist)
        objective[:, it] = dist.double().sum(0).cpu()
        sub = pq_unpack(codes) if bits == 4 else codes
        for m in range(Ms):
            key = sub[:, m].to(torch.int64)
            order = torch.argsort(key, stable=True).to(torch.int32)       # by (code, id)
            start = torch.zeros(K + 1, dtype=torch.int64, device=dev)
            start[1:] = torch.cumsum(torch.bincount(key, minlength=K), 0)
            ops.ivf_centroid_sums(Xt[:, m * dsub:(m + 1) * dsub], order, start.to(torch.int32), cb[m], dsub)
    return cb, objective


def pq_unpack(codes):
    """uint8 [n, 2 M]: the per-subspace codes of 4-bit ``codes`` (uint8 [n, M]; byte b = code(2b) | code(2b + 1) << 4)"""
    return torch.stack((codes & 15, codes >> 4), dim=2).reshape(codes.shape[0], -1)


class IVFIndex:
    """IVF-Flat index over a catalogue (the contract: include/cdml_ivf.h).  ``build`` runs Lloyd's k-means on the device and
    ``from_assignment`` takes centroids and an assignment as they are; ``search`` returns EXACTLY the k best listed rows of
    every query's ``nprobe`` nearest lists under the key (distance, id).  Attributes (device tensors): ``centroids`` fp32
    [nlist, D], ``assign`` int64 [n] (-1 = unlisted: a row with a non-finite coordinate), ``ids`` int32 [n_listed] sorted by
    (assign, id), ``list_start`` int32 [nlist + 1], ``rows`` fp32 [n_listed, Dp] and ``r_sq`` [n_listed] in that order;
    ``init_rows`` and ``train_ids`` (int64, CPU, sorted: the rows the centroids started from and the rows k-means ran on),
    ``objective`` (float64, CPU: one entry per Lloyd iteration), ``n_unlisted``.

    ``storage="f16"`` (include/cdml_ivf_f16.h): ``rows`` is the fp16 image of the prepared rows (half
    the bytes; the fp32 prepared matrix is not kept), ``r_sq`` the fp32 squared norms of the rounded values, a row whose
    image overflows is unlisted; k-means, ``assign``, ``centroids`` and the probes are those of the fp32 index.  ``search``
    then scans on the fp16 MFMA, and ``refine=r`` re-scores the r best candidates against fp32 rows (``base=``).

    ``storage="pq"`` (include/cdml_ivf_pq.h): product-quantised lists.  ``codes`` uint8 [n_listed,
    pq_m] stands where ``rows`` stood (there is no ``rows``), ``codebooks`` fp32 [pq_m, 256, Dp / pq_m] (``pq_train``, or given),
    ``pq_objective`` float64 [pq_m, pq_iters] (CPU), ``r_sq`` the norms of the decoded rows, ``decode(positions)`` the decoded
    rows.  ``search`` scans by table lookup (one lookup table per query); ``refine=r`` re-ranks as for "f16".
    ``pq_residual=True`` (include/cdml_ivf_pqr.h): the codes describe the row minus its list's
    centroid, a decoded row is centroid + codewords, and a score starts from the slot's <query, centroid>.
    ``pq_bits=4`` (include/cdml_ivf_pq4.h): the same ``pq_m`` bytes per row hold two 4-bit codes each
    (the even subspace in the low nibble), ``codebooks`` is fp32 [2 pq_m, 16, Dp / (2 pq_m)], a query's lookup table 32 ``pq_m``
    floats instead of 256 ``pq_m``.  Not with ``pq_residual``.

    ``search(..., scan="filter")`` (include/cdml_ivf_filter.h) is the same search, bit for bit, with a
    score buffer for the first ``seed_probes`` probe columns only: the other columns append what is within the seeded
    threshold to ``filter_cap`` candidate slots per query.

    The index can change after it is born (include/cdml_ivf_update.h): ``train`` (``build`` on a sample,
    then ``reset``) gives an index that lists no row, ``add(rows)`` appends rows under new ids in blocks and merges them into the
    lists in one launch, ``remove(ids)`` unlists rows (ids are stable: ``n_rows`` stays), ``locate`` / ``reconstruct`` find an
    id's position and what is stored for it, and ``state_dict(lists=True)`` / ``load_state_dict(state)`` carry the lists
    themselves, so that no step needs the whole catalogue as one fp32 matrix.  After any sequence of these the index equals
    ``from_assignment`` of all rows ever added with its own ``assign``, bit for bit."""

    STORAGES = ("f32", "f16", "pq")
    _NORM_ROWS = 1 << 20        # rows per fp32 temporary when the squared norms of fp16 rows are taken

    def __init__(self):
        raise TypeError("use IVFIndex.build, IVFIndex.train, IVFIndex.from_assignment or IVFIndex.load_state_dict")

    # ---- construction ----
    @staticmethod
    def _as_tensor(a):
        t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float32))
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("the catalogue must be a non-empty [n, D] matrix")
        return t

    @staticmethod
    def _prepared(t, device, l2_norm):
        """[n, D] -> the fp32 device matrix [n, Dp] the index works on: zero-padded to Dp % 32 == 0, l2-normalised if asked."""
        X = _device_matrix(t, device, 1, 32)
        if l2_norm:
            ops.l2norm_fwd(X, X.shape[1], X)
        return X

    def prepare(self, base):
        """The fp32 device matrix [n, Dp] this index works on for ``base`` ([n, D]): zero-padded to Dp % 32 == 0 and
        l2-normalised when the index is; what ``search(..., refine=r, base=)`` re-ranks against."""
        t = base if torch.is_tensor(base) else torch.as_tensor(np.asarray(base, dtype=np.float32))
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError("catalogue / index dimension mismatch: base must be [n, D = %d], got %s" % (self.dim, tuple(t.shape)))
        return self._prepared(t, self.device, self.l2_norm)

    @classmethod
    def _check_storage(cls, storage):
        if storage not in cls.STORAGES:
            raise ValueError("storage must be one of %s, got %r" % (cls.STORAGES, storage))
        return storage

    @classmethod
    def _sqnorm_f16(cls, rows):
        """fp32 |row|^2 of fp16 rows (the rounded values), through fp32 temporaries of at most _NORM_ROWS rows"""
        out = torch.zeros(rows.shape[0], dtype=torch.float32, device=rows.device)
        for r0 in range(0, rows.shape[0], cls._NORM_ROWS):
            part = rows[r0:r0 + cls._NORM_ROWS].float()
            ops.row_sqnorm(part, part.shape[1], out[r0:r0 + cls._NORM_ROWS])
        return out

    @classmethod
    def _blank(cls, nlist, D, l2_norm, device, precision, storage="f32", pq_m=None, pq_residual=False, pq_bits=8):
        self = object.__new__(cls)
        self.pq_residual = _check_pq_residual(storage, pq_residual)
        self.pq_bits = _check_pq_bits(storage, pq_bits, pq_m, _round_up(int(D), 32), pq_residual)
        self.nlist, self.dim, self.l2_norm, self.device, self.precision = int(nlist), int(D), bool(l2_norm), torch.device(device), precision
        self.storage = cls._check_storage(storage)
        if storage == "pq":
            self.pq_m = int(pq_m)
            self.pq_objective = torch.empty((self.pq_m * (2 if self.pq_bits == 4 else 1), 0), dtype=torch.float64)
        self.init_rows = self.train_ids = torch.empty(0, dtype=torch.int64)
        self.objective = torch.empty(0, dtype=torch.float64)
        return self

    def _set_lists(self, X, C, assign):
        """the cluster-major lists of (X, assign); rows with a non-finite coordinate are unlisted whatever ``assign`` says"""
        n = X.shape[0]
        self._C = C
        payload, r_sq, a = self._encode_block(X, assign.to(device=X.device))  # (an unlisted row's payload is computed and dropped)
        key = torch.where(a >= 0, a, torch.full_like(a, self.nlist))
        order = torch.argsort(key, stable=True)               # ids ascend inside a list
        cnt = torch.bincount(key, minlength=self.nlist + 1)
        n_listed = n - int(cnt[self.nlist])
        if n_listed < 1:
            raise ValueError("assign lists no finite row")
        start = torch.zeros(self.nlist + 1, dtype=torch.int64, device=X.device)
        start[1:] = torch.cumsum(cnt[:self.nlist], 0)
        self.assign = a
        self.ids = order[:n_listed].to(torch.int32)
        self.list_start = start.to(torch.int32)
        self.list_len = cnt[:self.nlist].contiguous()
        setattr(self, self._payload_name(), payload.index_select(0, order[:n_listed]))
        self.r_sq = r_sq.index_select(0, order[:n_listed])
        self.centroids = C[:, :self.dim]
        self.n_rows, self.n_listed, self.n_unlisted = n, n_listed, n - n_listed
        return self

    def decode(self, positions):
        """fp32 [len, Dp]: the decoded rows (the concatenated codewords; with ``pq_residual`` the list's centroid + them, one
        fp32 add; with ``pq_bits=4`` the 2 pq_m codewords of the unpacked nibbles) at ``positions`` of the cluster-major lists (plumbing: a torch gather).  storage "pq" only."""
        if self.storage != "pq":
            raise ValueError("decode belongs to an index with storage=\"pq\" (this one is %r)" % self.storage)
        pos = positions.to(device=self.device, dtype=torch.int64)
        lst = None
        if self.pq_residual:                              # the list of a position: the last c with list_start[c] <= position
            lst = torch.searchsorted(self.list_start[1:].to(torch.int64), pos, right=True)
        return self._decode_codes(self.codes.index_select(0, pos), lst)

    def _decode_codes(self, codes, lists):
        """``decode`` of given code rows (uint8 [len, pq_m]); ``lists`` (int64 [len]; residual indexes only): each row's list"""
        c = (pq_unpack(codes) if self.pq_bits == 4 else codes).to(torch.int64)
        m = torch.arange(c.shape[1], device=self.device)
        out = self.codebooks[m[None, :], c].reshape(c.shape[0], -1)
        if self.pq_residual:
            out = self._C.index_select(0, lists) + out
        return out

    @staticmethod
    def _check_codebooks(codebooks, Dp, pq_bits=None):
        """(codebooks as a CPU-or-device fp32 tensor, M, bits): the refusals of a given ``codebooks``, by name.  [M, 256, Dp / M]
        is an 8-bit set, [2 M, 16, Dp / (2 M)] a 4-bit one; ``pq_bits`` (None = whatever the shape says) must agree."""
        cb = codebooks if torch.is_tensor(codebooks) else torch.as_tensor(np.asarray(codebooks))
        if pq_bits is not None:
            _check_pq_bits("pq", pq_bits)
        bits = 4 if cb.dim() == 3 and cb.shape[1] == PQ4_CODEWORDS else 8
        if cb.dtype != torch.float32 or cb.dim() != 3 or cb.shape[1] != pq_codewords(bits) or cb.shape[0] % (2 if bits == 4 else 1) \
                or cb.shape[0] * cb.shape[2] != Dp:
            raise ValueError("codebooks must be a float32 [M, %d, Dp / M] (or, 4-bit, [2 M, %d, Dp / (2 M)]) tensor with M dsub = "
                             "Dp = %d, got %s %s" % (PQ_CODEWORDS, PQ4_CODEWORDS, Dp, tuple(cb.shape), cb.dtype))
        if pq_bits is not None and int(pq_bits) != bits:
            raise ValueError("pq_bits=%d contradicts codebooks of shape %s (a %d-bit set)" % (int(pq_bits), tuple(cb.shape), bits))
        return cb, _check_pq_m("pq", cb.shape[0] // (2 if bits == 4 else 1), Dp, what="the codebooks' M"), bits

    @classmethod
    def from_assignment(cls, base, centroids, assign, l2_norm=True, device="cuda:0", precision="f32x3", storage="f32",
                        codebooks=None, pq_residual=False, pq_bits=None):
        """The index of given ``centroids`` ([nlist, D]) and an arbitrary ``assign`` (int [n], values in [-1, nlist); -1 =
        unlisted): the search contract does not need the assignment to be the nearest centroid.  ``storage="pq"`` takes
        ``codebooks`` (fp32 [M, 256, Dp / M]) as they are; with ``pq_residual=True`` they are codebooks of residuals.
        ``pq_bits`` (default: 8, or what the codebooks say) -- codebooks of shape [2 M, 16, Dp / (2 M)] make a 4-bit index; a
        ``pq_bits`` that contradicts the codebooks' shape is refused."""
        cls._check_storage(storage)
        _check_pq_residual(storage, pq_residual)
        t = cls._as_tensor(base)
        pq_m = None
        bits = 8
        if storage == "pq":
            if codebooks is None:
                raise ValueError("from_assignment(storage=\"pq\") needs codebooks= (fp32 [M, 256, Dp / M]; knn.pq_train)")
            codebooks, pq_m, bits = cls._check_codebooks(codebooks, _round_up(t.shape[1], 32), pq_bits)
            _check_pq_bits(storage, bits, pq_m, _round_up(t.shape[1], 32), pq_residual)
        elif pq_bits is not None:
            _check_pq_bits(storage, pq_bits)
        if storage != "pq" and codebooks is not None:
            raise ValueError("codebooks belongs to storage=\"pq\" (got storage=%r)" % storage)
        c = centroids if torch.is_tensor(centroids) else torch.as_tensor(np.asarray(centroids, dtype=np.float32))
        a = assign if torch.is_tensor(assign) else torch.as_tensor(np.asarray(assign))
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != t.shape[1]:
            raise ValueError("centroid / catalogue dimension mismatch: centroids must be [nlist >= 1, D = %d]" % t.shape[1])
        if a.dim() != 1 or a.shape[0] != t.shape[0] or a.is_floating_point():
            raise ValueError("assign must be an integer vector with one entry per catalogue row (%d)" % t.shape[0])
        nlist = c.shape[0]
        if a.numel() and (int(a.min()) < -1 or int(a.max()) >= nlist):
            raise ValueError("assign must lie in [-1, nlist = %d)" % nlist)
        self = cls._blank(nlist, t.shape[1], l2_norm, device, precision, storage, pq_m, pq_residual, bits)
        if storage == "pq":
            self.codebooks = codebooks.detach().to(self.device).contiguous().clone()
        X = cls._prepared(t, self.device, l2_norm)
        return self._set_lists(X, _device_matrix(c, self.device, 1, 32), a)

    @classmethod
    def build(cls, base, nlist, iters=10, seed=0, train_rows=None, l2_norm=True, device="cuda:0", precision="f32x3",
              storage="f32", pq_m=None, pq_iters=None, pq_seed=None, pq_train_rows=None, pq_residual=False, pq_bits=8):
        """Lloyd's k-means, deterministic (include/cdml_ivf.h BUILD).  ``precision`` is that of the coarse ``knn_search`` calls
        (every assignment step, and ``probes``).  ``storage`` ("f32" | "f16" | "pq") is the format of the lists alone: k-means
        runs on the fp32 rows either way, so (base, seed) gives the same ``assign`` and the same probes for all three.
        ``storage="pq"``: ``pq_m`` bytes per row; the codebooks come from ``pq_train(X, pq_m, pq_iters (default 10), pq_seed
        (default ``seed``), pq_train_rows)`` on the prepared rows; with ``pq_residual=True`` on their residuals against the
        final centroids and assignment; ``pq_bits=4``: 2 ``pq_m`` subspaces of 16 codewords (``pq4_train``)."""
        cls._check_storage(storage)
        _check_pq_residual(storage, pq_residual)
        t = cls._as_tensor(base)
        pq_m = _check_pq_m(storage, pq_m, _round_up(t.shape[1], 32))
        pq_bits = _check_pq_bits(storage, pq_bits, pq_m, _round_up(t.shape[1], 32), pq_residual)
        if storage != "pq" and (pq_iters is not None or pq_seed is not None or pq_train_rows is not None):
            raise ValueError("pq_iters, pq_seed and pq_train_rows belong to storage=\"pq\" (got storage=%r)" % storage)
        nlist, iters = int(nlist), int(iters)
        n_finite = int(torch.isfinite(t).all(1).sum())
        if not 1 <= nlist <= n_finite:
            raise ValueError("nlist must be in [1, the number of finite rows = %d], got %d" % (n_finite, nlist))
        if iters < 0:
            raise ValueError("iters must be >= 0, got %d" % iters)
        n_train = min(n_finite, 256 * nlist) if train_rows is None else int(train_rows)
        if not nlist <= n_train <= n_finite:
            raise ValueError("train_rows must be in [nlist = %d, the number of finite rows = %d], got %d" % (nlist, n_finite, n_train))
        if storage == "pq":
            _check_pq_train(n_finite, 10 if pq_iters is None else pq_iters, pq_train_rows, pq_bits)
        self = cls._blank(nlist, t.shape[1], l2_norm, device, precision, storage, pq_m, pq_residual, pq_bits)
        dev = self.device
        X = cls._prepared(t, dev, l2_norm)
        n, Dp = X.shape
        finite = torch.isfinite(X).all(1)
        fin = torch.nonzero(finite).flatten().cpu()
        if fin.numel() != n_finite:
            raise ValueError("rows became non-finite under l2 normalisation (%d of %d finite rows left)" % (fin.numel(), n_finite))
        g = torch.Generator()
        g.manual_seed(int(seed))
        perm = torch.randperm(n_finite, generator=g)
        init_rows = torch.sort(fin[perm[:nlist]]).values
        train_ids = torch.sort(fin[perm[:n_train]]).values
        Xt = X if n_train == n else X.index_select(0, train_ids.to(dev))
        C = X.index_select(0, init_rows.to(dev)).contiguous()
        objective = []
        for _ in range(iters):
            Dt, It = knn_search(C, Xt, 1, l2_norm=False, device=dev, precision=precision)
            a = It[:, 0]
            ok = a >= 0
            objective.append(torch.where(ok, Dt[:, 0], torch.zeros_like(Dt[:, 0])).double().sum())
            key = torch.where(ok, a, torch.full_like(a, nlist))
            order = torch.argsort(key, stable=True).to(torch.int32)
            start = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
            start[1:] = torch.cumsum(torch.bincount(key, minlength=nlist + 1)[:nlist], 0)
            ops.ivf_centroid_sums(Xt, order, start.to(torch.int32), C, Dp)
        _, Ia = knn_search(C, X, 1, l2_norm=False, device=dev, precision=precision)
        if storage == "pq":
            res = {"centroids": C, "assign": Ia[:, 0].to(torch.int64)} if pq_residual else {}
            train = pq4_train if pq_bits == 4 else pq_train
            self.codebooks, self.pq_objective = train(X, pq_m, iters=10 if pq_iters is None else pq_iters,
                                                      seed=seed if pq_seed is None else pq_seed, train_rows=pq_train_rows, **res)
        self._set_lists(X, C, Ia[:, 0])
        self.init_rows, self.train_ids = init_rows, train_ids
        self.objective = torch.stack(objective).cpu() if objective else torch.empty(0, dtype=torch.float64)
        return self

    def state_dict(self, lists=False):
        """centroids + assign + the flags (CPU tensors); the lists are re-derived from the catalogue on load, bit for bit.
        An f16 index adds ``"storage": "f16"``; an f32 index's keys are what they were (a missing key loads as "f32").
        ``lists=True`` adds the lists themselves -- ``n_rows``, ``ids``, ``list_start``, ``r_sq`` and ``rows`` or ``codes`` -- so
        that ``load_state_dict(state, base=None)`` needs no catalogue (an index built by ``add`` may never have had one)."""
        state = {"centroids": self.centroids.detach().cpu().clone(), "assign": self.assign.cpu().clone(), "l2_norm": self.l2_norm,
                 "precision": self.precision, "init_rows": self.init_rows.clone(), "objective": self.objective.clone()}
        if self.storage != "f32":
            state["storage"] = self.storage
        if self.storage == "pq":
            state["pq_m"] = self.pq_m
            state["codebooks"] = self.codebooks.detach().cpu().clone()
            if self.pq_residual:
                state["pq_residual"] = True
            if self.pq_bits == 4:                             # (absent at 8: the state of an 8-bit index keeps its keys)
                state["pq_bits"] = 4
        if lists:
            state["n_rows"] = int(self.n_rows)
            state["ids"], state["list_start"], state["r_sq"] = self.ids.cpu().clone(), self.list_start.cpu().clone(), self.r_sq.cpu().clone()
            payload = "codes" if self.storage == "pq" else "rows"
            state[payload] = getattr(self, payload).cpu().clone()
        return state

    @classmethod
    def load_state_dict(cls, state, base=None, device="cuda:0", storage=None):
        """The index of ``state_dict()`` over the same catalogue ``base``.  ``storage`` (default: the state's, "f32" where
        it names none) may re-derive the lists in another format: centroids and assign do not depend on it.  "pq" needs
        the state's codebooks (a state of a pq index); its codes are re-derived from ``base``, bit for bit.
        ``base=None``: the lists are taken from the state as they are (``state_dict(lists=True)``), in the state's format;
        a state without lists is refused by name."""
        if base is None:
            return cls._load_lists(state, device, storage)
        storage = cls._check_storage(state.get("storage", "f32") if storage is None else storage)
        kw = {}
        if storage == "pq":
            if "codebooks" not in state:
                raise ValueError("this state holds no codebooks (it is not the state of a storage=\"pq\" index): it cannot be "
                                 "loaded as \"pq\"")
            kw["codebooks"] = state["codebooks"]
            kw["pq_residual"] = bool(state.get("pq_residual", False))
            kw["pq_bits"] = state.get("pq_bits")              # (None: what the codebooks' shape says)
        self = cls.from_assignment(base, state["centroids"], state["assign"], l2_norm=state["l2_norm"], device=device,
                                   precision=state["precision"], storage=storage, **kw)
        self.init_rows, self.objective = state["init_rows"].clone(), state["objective"].clone()
        return self

    @classmethod
    def _load_lists(cls, state, device, storage):
        """``load_state_dict(state, base=None)``: the refusals by name, then the state's lists as they are"""
        own = cls._check_storage(state.get("storage", "f32"))
        payload = "codes" if own == "pq" else "rows"
        missing = [k for k in ("n_rows", "ids", "list_start", "r_sq", payload) if k not in state]
        if missing:
            raise ValueError("load_state_dict(base=None) needs a state that carries its lists (state_dict(lists=True)): this one "
                             "lacks %s; give base= (the catalogue) instead" % ", ".join(missing))
        if storage is not None and cls._check_storage(storage) != own:
            raise ValueError("load_state_dict(base=None) takes the lists in the state's format (%r): storage=%r needs base= to "
                             "re-derive them" % (own, storage))
        c = state["centroids"]
        pq_m = bits = None
        if own == "pq":
            _, pq_m, bits = cls._check_codebooks(state["codebooks"], _round_up(c.shape[1], 32), state.get("pq_bits"))
        self = cls._blank(c.shape[0], c.shape[1], state["l2_norm"], device, state["precision"], own, pq_m,
                          bool(state.get("pq_residual", False)), 8 if bits is None else bits)
        dev = self.device
        if own == "pq":
            self.codebooks = state["codebooks"].detach().to(dev).contiguous().clone()
        self._C = _device_matrix(c, dev, 1, 32)
        self.centroids = self._C[:, :self.dim]
        self.assign = state["assign"].to(device=dev, dtype=torch.int64).clone()
        self.ids = state["ids"].to(device=dev, dtype=torch.int32).clone()
        self.list_start = state["list_start"].to(device=dev, dtype=torch.int32).clone()
        self.list_len = (self.list_start[1:] - self.list_start[:-1]).to(torch.int64).contiguous()
        self.r_sq = state["r_sq"].to(device=dev, dtype=torch.float32).clone()
        setattr(self, payload, state[payload].to(dev).contiguous().clone())
        self.n_rows, self.n_listed = int(state["n_rows"]), int(self.ids.numel())
        self.n_unlisted = self.n_rows - self.n_listed
        if tuple(self.assign.shape) != (self.n_rows,) or tuple(self.list_start.shape) != (self.nlist + 1,) \
                or self.r_sq.numel() != self.n_listed or getattr(self, payload).shape[0] != self.n_listed:
            raise ValueError("the state's lists disagree with each other (n_rows = %d, n_listed = %d)" % (self.n_rows, self.n_listed))
        self.init_rows, self.objective = state["init_rows"].clone(), state["objective"].clone()
        return self

    # ---- train / add / remove (include/cdml_ivf_update.h) ----
    @classmethod
    def train(cls, sample, nlist, iters=10, seed=0, train_rows=None, l2_norm=True, device="cuda:0", precision="f32x3",
              storage="f32", pq_m=None, pq_iters=None, pq_seed=None, pq_train_rows=None, pq_residual=False, pq_bits=8):
        """``build(sample, nlist, ...)`` followed by ``reset()``: an index that knows its centroids (and codebooks) and lists no
        row yet; ``add`` fills it.  ``train(sample, ...).add(sample)`` IS ``build(sample, ...)``, attribute for attribute."""
        return cls.build(sample, nlist, iters=iters, seed=seed, train_rows=train_rows, l2_norm=l2_norm, device=device,
                         precision=precision, storage=storage, pq_m=pq_m, pq_iters=pq_iters, pq_seed=pq_seed,
                         pq_train_rows=pq_train_rows, pq_residual=pq_residual, pq_bits=pq_bits).reset()

    def _payload_name(self):
        return "codes" if self.storage == "pq" else "rows"

    def _row_shape(self):
        """(columns, dtype) of one payload row"""
        Dp = _round_up(self.dim, 32)
        return (self.pq_m, torch.uint8) if self.storage == "pq" else (Dp, torch.float16 if self.storage == "f16" else torch.float32)

    def reset(self):
        """Drop every row: n_rows = n_listed = 0, empty ids / payload / r_sq / assign, list_start all zero.  Centroids,
        codebooks, init_rows, train_ids and the objectives stay.  Returns the index."""
        dev = self.device
        cols, dt = self._row_shape()
        setattr(self, self._payload_name(), torch.empty((0, cols), dtype=dt, device=dev))
        self.ids = torch.empty(0, dtype=torch.int32, device=dev)
        self.r_sq = torch.empty(0, dtype=torch.float32, device=dev)
        self.assign = torch.empty(0, dtype=torch.int64, device=dev)
        self.list_start = torch.zeros(self.nlist + 1, dtype=torch.int32, device=dev)
        self.list_len = torch.zeros(self.nlist, dtype=torch.int64, device=dev)
        self.n_rows = self.n_listed = self.n_unlisted = 0
        return self

    def _check_listed(self):
        if getattr(self, "n_listed", None) == 0:
            raise ValueError("the index lists no row: add rows first (IVFIndex.add)")

    def _check_ids(self, ids, what):
        """int64 ids on the index's device; an id outside [0, n_rows) is refused by name (checked where the ids live)"""
        q = ids if torch.is_tensor(ids) else torch.as_tensor(np.asarray(ids))
        if q.dim() != 1 or q.is_floating_point() or q.dtype == torch.bool:
            raise ValueError("%s takes an integer vector of catalogue ids" % what)
        q = q.to(torch.int64)
        if q.numel() and (int(q.min()) < 0 or int(q.max()) >= self.n_rows):
            raise ValueError("%s: an id is outside [0, n_rows = %d) (got ids in [%d, %d])"
                             % (what, self.n_rows, int(q.min()), int(q.max())))
        return q.to(self.device).contiguous()

    def _encode_block(self, X, a, stages=None):
        """(payload [b, row], r_sq fp32 [b], a int64 [b] with -1 for an unlisted row) of one prepared block ``X`` whose nearest
        centroids are ``a``: what the index stores per row, a function of the row and of the centroids / codebooks alone (which is
        why ``_set_lists`` may take it for the whole catalogue and ``add`` chunk by chunk)"""
        b, Dp = X.shape
        dev = X.device
        mark = (lambda name: None) if stages is None else stages
        Xh = X.to(torch.float16) if self.storage == "f16" else None           # round to nearest even; overflow -> inf
        finite = torch.isfinite(X if Xh is None else Xh).all(1)
        a = torch.where(finite, a.to(torch.int64), torch.full((b,), -1, dtype=torch.int64, device=dev))
        if self.storage == "pq":
            codes = torch.empty((b, self.pq_m), dtype=torch.uint8, device=dev)
            if self.pq_residual:
                ops.pqr_encode(X, self._C, a, self.codebooks, codes)
            elif self.pq_bits == 4:
                ops.pq4_encode(X, self.codebooks, codes)
            else:
                ops.pq_encode(X, self.codebooks, codes)
            mark("encode")
            r_sq = torch.zeros(b, dtype=torch.float32, device=dev)
            for r0 in range(0, b, self._NORM_ROWS):
                lst = a[r0:r0 + self._NORM_ROWS].clamp(min=0) if self.pq_residual else None      # (an unlisted row's norm is dropped)
                part = self._decode_codes(codes[r0:r0 + self._NORM_ROWS], lst)
                ops.row_sqnorm(part, Dp, r_sq[r0:r0 + self._NORM_ROWS])
            mark("r_sq")
            return codes, r_sq, a
        if self.storage == "f16":
            mark("encode")
            r_sq = self._sqnorm_f16(Xh)
            mark("r_sq")
            return Xh, r_sq, a
        mark("encode")
        r_sq = torch.zeros(b, dtype=torch.float32, device=dev)
        ops.row_sqnorm(X, Dp, r_sq)
        mark("r_sq")
        return X, r_sq, a

    def _move(self, old_pos, kept_start, payload, r_sq, order, add_start, id0, n_rows):
        """the one launch of an update: new lists from the kept old rows (``old_pos``: None = all of them, in place) and the
        chunk (``payload`` / ``r_sq`` / ``order`` / ``add_start``; None for a removal); ``n_rows`` = the ids consumed after it.
        Out of place: the old arrays are freed when this returns, so the peak is twice the list bytes.  The index changes only
        after the launch has been enqueued: an allocation that fails leaves it as it was."""
        dev = self.device
        name = self._payload_name()
        cols, dt = self._row_shape()
        zeros = torch.zeros(self.nlist + 1, dtype=torch.int32, device=dev)
        add_start = zeros if add_start is None else add_start
        new_start = kept_start + add_start
        n_new = int(new_start[-1])                            # the host read
        new_rows = torch.empty((n_new, cols), dtype=dt, device=dev)
        new_ids = torch.empty(n_new, dtype=torch.int32, device=dev)
        new_r_sq = torch.empty(n_new, dtype=torch.float32, device=dev)
        if n_new:
            ops.ivf_lists_move(getattr(self, name), self.ids, self.r_sq, old_pos, payload, r_sq, order, id0, kept_start, add_start,
                               new_start, new_rows, new_ids, new_r_sq)
        setattr(self, name, new_rows)
        self.ids, self.r_sq, self.list_start = new_ids, new_r_sq, new_start
        self.list_len = (new_start[1:] - new_start[:-1]).to(torch.int64).contiguous()
        self.n_rows, self.n_listed, self.n_unlisted = n_rows, n_new, n_rows - n_new

    def add(self, rows, block_rows=1 << 20, stages=None):
        """Append ``rows`` ([m, D]; numpy, CPU or device tensor) as catalogue ids n_rows .. n_rows + m - 1; returns the first
        new id.  In blocks of at most ``block_rows`` rows (the fp32 temporaries are block_rows x Dp) the rows are prepared,
        assigned to their nearest centroid (``build``'s final assignment call), rounded / encoded and their r_sq taken as
        ``from_assignment`` does; the chunk's payload is kept in the list format, and ONE launch (``ops.ivf_lists_move``)
        merges it into the lists: a list = its old rows, then its new rows in chunk order.  A row with a non-finite
        coordinate (storage "f16": an overflowing image) consumes its id and is unlisted.  The index then equals
        ``from_assignment`` of all rows ever added with ``self.assign``, bit for bit.  Only the m keys of the chunk are sorted;
        the lists are written out of place (peak: twice the list bytes).  ``stages`` (a callable, optional; tools/ivf_add_bench.py)
        is called with a stage's name when its work has been enqueued."""
        t = rows if torch.is_tensor(rows) else torch.as_tensor(np.asarray(rows, dtype=np.float32))
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError("add: row / index dimension mismatch: rows must be [m, D = %d], got %s" % (self.dim, tuple(t.shape)))
        m, block_rows = int(t.shape[0]), int(block_rows)
        if m < 1:
            raise ValueError("add needs m >= 1 rows, got %d" % m)
        if block_rows < 1:
            raise ValueError("block_rows must be >= 1, got %d" % block_rows)
        id0 = int(self.n_rows)
        if id0 + m > 2 ** 31 - 1:
            raise ValueError("add: n_rows + m = %d exceeds 2^31 - 1 (catalogue ids are int32)" % (id0 + m))
        dev = self.device
        mark = (lambda name: None) if stages is None else stages
        cols, dt = self._row_shape()
        payload = torch.empty((m, cols), dtype=dt, device=dev)
        r_sq = torch.empty(m, dtype=torch.float32, device=dev)
        a = torch.empty(m, dtype=torch.int64, device=dev)
        for b0 in range(0, m, block_rows):
            b1 = min(b0 + block_rows, m)
            Xb = t[b0:b1].to(device=dev, dtype=torch.float32)
            mark("copy_in")
            X = self._prepared(Xb, dev, self.l2_norm)
            mark("prepare")
            _, Ia = knn_search(self._C, X, 1, l2_norm=False, device=dev, precision=self.precision)
            mark("assign")
            payload[b0:b1], r_sq[b0:b1], a[b0:b1] = self._encode_block(X, Ia[:, 0], stages)
        key = torch.where(a >= 0, a, torch.full_like(a, self.nlist))
        order = torch.argsort(key, stable=True)               # the chunk alone: m keys
        cnt = torch.bincount(key, minlength=self.nlist + 1)
        add_start = torch.zeros(self.nlist + 1, dtype=torch.int32, device=dev)
        add_start[1:] = torch.cumsum(cnt[:self.nlist], 0)
        n_add = m - int(cnt[self.nlist])                      # the host read
        assign = torch.cat([self.assign, a])
        mark("tables")
        self._move(None, self.list_start, payload, r_sq, order[:n_add].to(torch.int32), add_start, id0, id0 + m)
        self.assign = assign
        mark("move")
        return id0

    def locate(self, ids):
        """int32 [len]: the position of every id of ``ids`` in the cluster-major lists (``ids[position] == id``), -1 for an
        unlisted id.  An id outside [0, n_rows) is refused by name."""
        q = self._check_ids(ids, "locate")
        pos = torch.full((q.numel(),), -1, dtype=torch.int32, device=self.device)
        if q.numel() and self.n_listed:
            ops.ivf_locate(q, self.assign, self.ids, self.list_start, pos)
        return pos

    def reconstruct(self, ids):
        """fp32 [len, Dp]: what the index stores for ``ids`` -- the listed row (fp16 widened), or for storage "pq" the
        decoded row ``decode(locate(ids))``.  An unlisted id is refused by name."""
        q = self._check_ids(ids, "reconstruct")
        gone = self.assign.index_select(0, q.to(self.assign.device)) < 0
        if bool(gone.any()):
            raise ValueError("reconstruct: id %d is unlisted (removed, or a row with a non-finite coordinate): the index stores "
                             "nothing for it" % int(q[torch.nonzero(gone)[0, 0]]))
        pos = self.locate(q).to(torch.int64)
        if self.storage == "pq":
            return self.decode(pos)
        return self.rows.index_select(0, pos).float()

    def remove(self, ids):
        """Unlist ``ids`` (an integer vector; duplicates and already-unlisted ids are allowed, an id outside [0, n_rows) is
        refused by name); returns how many rows were listed and are no longer.  Ids are stable: n_rows stays, assign[id]
        becomes -1, and the lists close up in ONE launch (``ops.ivf_lists_move`` over the kept positions).  The index then
        equals ``from_assignment`` of the catalogue with the new ``assign``."""
        q = self._check_ids(ids, "remove")
        if q.numel() == 0 or self.n_listed == 0:
            return 0
        dev = self.device
        pos = self.locate(q)
        keep = torch.ones(self.n_listed, dtype=torch.bool, device=dev)
        keep[pos[pos >= 0].to(torch.int64)] = False
        cs = torch.zeros(self.n_listed + 1, dtype=torch.int64, device=dev)
        cs[1:] = torch.cumsum(keep, 0)
        kept_start = cs.index_select(0, self.list_start.to(torch.int64)).to(torch.int32)
        n_removed = self.n_listed - int(cs[-1])               # the host read
        if n_removed == 0:
            return 0
        self._move(torch.nonzero(keep).flatten().to(torch.int32), kept_start, None, None, None, None, 0, self.n_rows)
        self.assign[q] = -1
        return n_removed

    # ---- search ----
    def _check_queries(self, queries, nprobe, k=None):
        cap = ops.knn_list_capacity()
        if k is not None and not 1 <= int(k) <= cap:
            raise ValueError("k must be in [1, %d], got %d" % (cap, int(k)))
        if not 1 <= int(nprobe) <= min(self.nlist, cap):
            raise ValueError("nprobe must be in [1, min(nlist = %d, %d)], got %d" % (self.nlist, cap, int(nprobe)))
        shape = tuple(queries.shape)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError("query / index dimension mismatch: queries must be [nq, D = %d], got %s" % (self.dim, shape))

    def _check_probe(self, probe, nq, nprobe):
        """a given probe table as a tensor (None stays None): the refusals, by name"""
        if probe is None:
            return None
        probe = torch.as_tensor(probe)
        if tuple(probe.shape) != (nq, nprobe) or probe.is_floating_point():
            raise ValueError("probe must be an integer [nq = %d, nprobe = %d] table" % (nq, nprobe))
        if probe.numel() and (int(probe.min()) < -1 or int(probe.max()) >= self.nlist):
            raise ValueError("probe ids must lie in [-1, nlist = %d)" % self.nlist)
        return probe

    def _probes(self, Q, nprobe):
        _, I = knn_search(self._C, Q, int(nprobe), l2_norm=False, device=self.device, precision=self.precision)
        return I

    def probes(self, queries, nprobe):
        """int64 [nq, nprobe]: every query's nprobe nearest centroids, nearest first (the exact search; -1 throughout for a
        non-finite query)."""
        self._check_queries(queries, nprobe)
        t = queries if torch.is_tensor(queries) else torch.as_tensor(np.asarray(queries, dtype=np.float32))
        return self._probes(self._prepared(t, self.device, self.l2_norm), nprobe)

    def scanned_share(self, probe):
        """The mean share of the listed rows that a query of ``probe`` ([nq, nprobe] list ids, -1 = none) scores."""
        self._check_listed()
        p = probe.to(device=self.device, dtype=torch.int64)
        rows = torch.where(p >= 0, self.list_len[p.clamp(min=0)], torch.zeros_like(p)).sum(1)
        return float(rows.double().mean()) / self.n_listed

    def default_score_bytes(self):
        """max(1 GiB, 4 B x 512 x n_listed): the default ``score_bytes`` of ``search``"""
        return max(IVF_SCORE_BYTES, 4 * IVF_SCORE_SLOTS * self.n_listed)

    def _check_refine(self, k, refine, base):
        """(r, base) of ``search``: the refusals, by name, before any device work"""
        r = int(refine)
        if self.storage == "f32":
            if r != 0 or base is not None:
                raise ValueError("refine and base belong to an index with storage=\"f16\" or \"pq\" (this one is \"f32\": its distances are exact already)")
            return 0, None
        if r == 0:
            if base is not None:
                raise ValueError("base is read only with refine > 0")
            return 0, None
        cap = ops.knn_list_capacity()
        if not int(k) <= r <= cap:
            raise ValueError("refine must be 0 or in [k = %d, %d], got %d" % (int(k), cap, r))
        Dp = _round_up(self.dim, 32)
        if base is None:
            raise ValueError("refine > 0 needs base=: the fp32 rows to re-rank against (IVFIndex.prepare(catalogue))")
        if not torch.is_tensor(base) or base.dtype != torch.float32 or base.dim() != 2 or base.stride(1) != 1 \
                or tuple(base.shape) != (self.n_rows, Dp) or base.device.type != self.device.type \
                or (self.device.index is not None and base.device.index != self.device.index):
            raise ValueError("base must be an fp32 [n_rows = %d, Dp = %d] matrix on %s (IVFIndex.prepare(catalogue)), got %s"
                             % (self.n_rows, Dp, self.device,
                                (tuple(base.shape), base.dtype, str(base.device)) if torch.is_tensor(base) else type(base).__name__))
        return r, base

    SCANS = ("buffer", "filter")
    FILTER_CAP_MIN, FILTER_CAP_MAX = 64, 65536

    def default_seed_probes(self, keep, nprobe):
        """min(nprobe, max(1, ceil(4 keep nlist / n_listed))): the probe columns whose lists hold 4 keep rows on average, so
        that short lists do not leave the seeded threshold at +inf.  Pure host arithmetic."""
        self._check_listed()
        keep, nprobe = int(keep), int(nprobe)
        return min(nprobe, max(1, -(-4 * keep * self.nlist // self.n_listed)))

    @classmethod
    def default_filter_cap(cls, keep):
        """the smallest power of two >= 4 keep, at least 64: the candidate slots per query of ``scan="filter"``"""
        cap = cls.FILTER_CAP_MIN
        while cap < 4 * int(keep):
            cap *= 2
        return cap

    def filter_costs(self, probe, seed_probes, filter_cap):
        """int64 ndarray [nq]: a query's floats in a chunk of ``scan="filter"`` = the padded lengths of its SEED lists (the
        first ``seed_probes`` columns of ``probe``, -1 = none) + 2 ``filter_cap`` (its candidate slots, 8 B each); what
        ``ivf_plan_chunks`` plans that search with."""
        p = probe[:, :int(seed_probes)].to(torch.int64)
        ld = (self.list_len + 3) // 4 * 4
        return (torch.where(p >= 0, ld[p.clamp(min=0)], torch.zeros_like(p)).sum(1) + 2 * int(filter_cap)).cpu().numpy()

    def _check_scan(self, scan, filter_cap, seed_probes, nprobe):
        """the refusals of ``search``'s scan arguments, by name, before any device work"""
        if scan not in self.SCANS:
            raise ValueError("scan must be one of %s, got %r" % (self.SCANS, scan))
        if scan == "filter" and self.storage == "pq":
            raise ValueError("scan=\"filter\" (DESIGN.md section 9f.2) has no launch for storage=\"pq\": use scan=\"buffer\"")
        if scan == "buffer":
            if filter_cap is not None or seed_probes is not None:
                raise ValueError("filter_cap and seed_probes belong to scan=\"filter\" (this search is scan=\"buffer\")")
            return
        if filter_cap is not None:
            c = int(filter_cap)
            if c != filter_cap or not self.FILTER_CAP_MIN <= c <= self.FILTER_CAP_MAX or c & (c - 1):
                raise ValueError("filter_cap must be a power of two in [%d, %d], got %r"
                                 % (self.FILTER_CAP_MIN, self.FILTER_CAP_MAX, filter_cap))
        if seed_probes is not None and (int(seed_probes) != seed_probes or not 1 <= int(seed_probes) <= int(nprobe)):
            raise ValueError("seed_probes must be in [1, nprobe = %d], got %r" % (int(nprobe), seed_probes))

    def _scan_buffered(self, Q, q_sq, probe, k, refine, base, score_bytes, best_d, best_i, cand_d, cand_i):
        """The buffered search of prepared queries ``Q`` over ``probe`` (int32 [nq, nprobe]) into best_d / best_i (and cand_d /
        cand_i, the merge's lists, when they are other tensors: ``refine``): per chunk the slot tables, the grouped product
        into the ragged score buffer, the merge, the re-rank.  Returns (chunks, n_tiles, n_floats)."""
        f16, pq = self.storage == "f16", self.storage == "pq"
        Dp = Q.shape[1]
        nprobe = probe.shape[1]
        ld = (self.list_len + 3) // 4 * 4
        p = probe.to(torch.int64)
        costs = torch.where(p >= 0, ld[p.clamp(min=0)], torch.zeros_like(p)).sum(1).cpu().numpy()
        tile = {}
        if pq:                                            # a chunk's scores AND lookup tables fit score_bytes together
            costs = costs + (pq_query_floats(self.pq_m, bits=4) if self.pq_bits == 4
                             else pq_query_floats(self.pq_m, nprobe if self.pq_residual else 0))
            tile["tile_slots"], tile["tile_rows"] = (ops.ivf_pq4_tile if self.pq_bits == 4 else ops.ivf_pq_tile)(self.pq_m)
        chunks = ivf_plan_chunks(costs, score_bytes, max_queries=(2 ** 31 - 1) // nprobe)
        n_tiles = n_floats = 0
        keep = refine or k                                # entries the merge must get right
        for q0, q1 in chunks:
            pc = probe[q0:q1].contiguous()
            tb = ivf_tables(pc, self.list_len, **tile)
            n_tiles += tb["n_tiles"]
            n_floats += tb["n_floats"]
            if tb["n_slots"] == 0:                        # nothing probed (non-finite queries only)
                best_d[q0:q1] = float("inf")
                best_i[q0:q1] = 0x7fffffff
                if refine:
                    cand_i[q0:q1] = 0x7fffffff
                continue
            scores = torch.empty(max(tb["n_floats"], 4), dtype=torch.float32, device=Q.device)
            if f16:
                Qh = Q[q0:q1].to(torch.float16)
                ops.row_sqnorm(Qh.float(), Dp, q_sq[q0:q1])
                if tb["n_tiles"]:
                    ops.ivf_scan_f16(Qh, tb["slot_query"], tb["slot_start"], tb["slot_off"], self.rows, self.list_start,
                                     tb["tiles"], scores)
            elif pq and self.pq_bits == 4:
                if tb["n_tiles"]:
                    lut = torch.empty((q1 - q0, 2 * self.pq_m, PQ4_CODEWORDS), dtype=torch.float32, device=Q.device)
                    ops.pq4_lut(Q[q0:q1], self.codebooks, lut)
                    ops.ivf_scan_pq4(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], self.codes, self.list_start,
                                     tb["tiles"], scores)
            elif pq:
                if tb["n_tiles"]:
                    lut = torch.empty((q1 - q0, self.pq_m, PQ_CODEWORDS), dtype=torch.float32, device=Q.device)
                    ops.pq_lut(Q[q0:q1], self.codebooks, lut)
                    if self.pq_residual:
                        slot_base = torch.empty(tb["n_slots"], dtype=torch.float32, device=Q.device)
                        ops.ivf_slot_dots(Q[q0:q1], self._C, tb["slot_query"], tb["slot_start"], slot_base)
                        ops.ivf_scan_pqr(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], slot_base, self.codes,
                                         self.list_start, tb["tiles"], scores)
                    else:
                        ops.ivf_scan_pq(lut, tb["slot_query"], tb["slot_start"], tb["slot_off"], self.codes, self.list_start,
                                        tb["tiles"], scores)
            elif tb["n_tiles"]:
                ops.ivf_scan_f32(Q[q0:q1], tb["slot_query"], tb["slot_start"], tb["slot_off"], self.rows, self.list_start,
                                 tb["tiles"], scores)
            ops.ivf_merge(scores, tb["slot_off"], tb["slot_of"], pc, self.list_start, self.ids, self.r_sq, q_sq[q0:q1], keep,
                          cand_d[q0:q1], cand_i[q0:q1])
            if refine:
                ops.ivf_refine(Q[q0:q1], base, cand_i[q0:q1], refine, k, best_d[q0:q1], best_i[q0:q1])
        return chunks, n_tiles, n_floats

    def _scan_filtered(self, Q, q_sq, probe, k, refine, base, score_bytes, best_d, best_i, cand_d, cand_i, s, cap_f, stats):
        """``scan="filter"`` (include/cdml_ivf_filter.h): per chunk, the first ``s`` probe columns through the buffered launches
        (every query's list and its keep-th distance tau), the other columns through ONE filter launch that writes no score
        and appends what is within tau to the query's ``cap_f`` candidate slots, ``knn_merge_list``, the re-rank.  A query
        whose count exceeded ``cap_f`` is searched again through ``_scan_buffered`` over its whole probe row."""
        f16 = self.storage == "f16"
        dev = Q.device
        Dp = Q.shape[1]
        nq, nprobe = probe.shape
        keep = refine or k
        ld = (self.list_len + 3) // 4 * 4
        seed_p, rest_p = probe.clone(), probe.clone()
        seed_p[:, s:] = -1                                    # a list is scanned by the seed or by the filter, never by both
        rest_p[:, :s] = -1
        chunks = ivf_plan_chunks(self.filter_costs(probe, s, cap_f), score_bytes, max_queries=(2 ** 31 - 1) // nprobe)
        n_tiles = n_floats = n_appended = 0
        redo = []
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        for q0, q1 in chunks:
            m = q1 - q0
            pc = seed_p[q0:q1].contiguous()
            tb = ivf_tables(pc, self.list_len)
            n_tiles += tb["n_tiles"]
            n_floats += tb["n_floats"]
            Qc = Q[q0:q1]
            if f16:
                Qc = Qc.to(torch.float16)
                ops.row_sqnorm(Qc.float(), Dp, q_sq[q0:q1])
            if tb["n_slots"] == 0:                        # nothing seeded: the lists ivf_merge leaves for no row
                cand_d[q0:q1] = float("inf")
                cand_i[q0:q1] = 0x7fffffff
            else:
                scores = torch.empty(max(tb["n_floats"], 4), dtype=torch.float32, device=dev)
                if tb["n_tiles"]:
                    (ops.ivf_scan_f16 if f16 else ops.ivf_scan_f32)(Qc, tb["slot_query"], tb["slot_start"], tb["slot_off"], self.rows,
                                                                   self.list_start, tb["tiles"], scores)
                ops.ivf_merge(scores, tb["slot_off"], tb["slot_of"], pc, self.list_start, self.ids, self.r_sq, q_sq[q0:q1], keep,
                              cand_d[q0:q1], cand_i[q0:q1])
                del scores
            if s < nprobe:
                tr = ivf_tables(rest_p[q0:q1].contiguous(), self.list_len)
                n_tiles += tr["n_tiles"]
                if tr["n_tiles"]:
                    tau = cand_d[q0:q1, keep - 1].contiguous()            # +inf where fewer than keep rows were seeded
                    cnt = torch.zeros(m, dtype=torch.int32, device=dev)
                    cand = torch.empty((m, cap_f, 2), dtype=torch.int32, device=dev)
                    (ops.ivf_filter_f16 if f16 else ops.ivf_filter_f32)(Qc, tr["slot_query"], tr["slot_start"], q_sq[q0:q1], tau, cnt,
                                                                       self.rows, self.list_start, self.r_sq, self.ids, tr["tiles"],
                                                                       cand, cap_f)
                    over = cnt > cap_f                        # (before the merge puts cnt back to 0)
                    n_over, n_app = torch.stack([over.sum(), cnt.sum()]).tolist()         # the host read
                    n_appended += n_app
                    ops.knn_merge_list(cand, cnt, cap_f, m, keep, cand_d[q0:q1], cand_i[q0:q1], overflow)
                    if n_over:
                        redo.append(torch.nonzero(over).flatten() + q0)
            if refine:
                ops.ivf_refine(Q[q0:q1], base, cand_i[q0:q1], refine, k, best_d[q0:q1], best_i[q0:q1])
        n_redo = 0
        if redo:                                              # candidates were dropped: these queries go through the score buffer
            idx = torch.cat(redo)
            n_redo = int(idx.numel())
            po = probe.index_select(0, idx)
            pl = po.to(torch.int64)
            own = int(torch.where(pl >= 0, ld[pl.clamp(min=0)], torch.zeros_like(pl)).sum(1).max())
            bd = torch.empty((n_redo, best_d.shape[1]), dtype=torch.float32, device=dev)
            bi = torch.empty((n_redo, best_i.shape[1]), dtype=torch.int32, device=dev)
            cd = torch.empty_like(bd) if refine else bd
            ci = torch.empty_like(bi) if refine else bi
            # (the budget covers one such query's own scores even where ``score_bytes`` is below them)
            self._scan_buffered(Q.index_select(0, idx), q_sq.index_select(0, idx), po, k, refine, base, max(int(score_bytes), 4 * own),
                                bd, bi, cd, ci)
            best_d[idx], best_i[idx] = bd, bi
            if refine:
                cand_d[idx], cand_i[idx] = cd, ci
        if stats is not None:
            stats.update(scan="filter", seed_probes=s, filter_cap=cap_f, n_appended=int(n_appended), refiltered=n_redo)
        return chunks, n_tiles, n_floats

    def search(self, queries, k, nprobe, score_bytes=None, stats=None, probe=None, refine=0, base=None, scan="buffer",
               filter_cap=None, seed_probes=None):
        """(D [nq, k] fp32 squared L2 ascending, I [nq, k] int64; +inf / -1 where fewer than k rows were probed), device
        tensors shaped and typed like ``knn_search``'s.  Queries go in chunks whose ragged score buffer fits ``score_bytes``
        (default ``default_score_bytes()``: 1 GiB, or 2 KiB per listed row where that is more -- 20 GB at 10 M rows;
        ``ivf_plan_chunks``); the result does not depend on the chunking.  ``stats`` (a dict, optional)
        receives the chunk list, the tile count and the score floats.  ``probe`` (int [nq, nprobe], values in [-1, nlist),
        a query's lists distinct; default: ``probes(queries, nprobe)``): the lists to scan, as given.
        On an index with storage "f16" a chunk's queries are rounded to fp16 as the rows were and the distances are those
        of the rounded values (a query whose image is non-finite probes nothing); ``refine=r`` (k <= r <= 128, with
        ``base`` = the fp32 matrix of ``prepare(catalogue)``) keeps the r best of them and returns the k best under the fp32
        distances sum (q - x)^2 of the fp32 rows (include/cdml_ivf_f16.h).
        On an index with storage "pq" (include/cdml_ivf_pq.h) the distances are those of the decoded rows to the unrounded
        query, scored by table lookup; a chunk holds its queries' lookup tables (256 ``pq_m`` floats each) beside its scores
        within ``score_bytes``; ``refine=r`` re-ranks as for "f16"; ``scan="filter"`` is refused.
        ``scan="filter"`` (include/cdml_ivf_filter.h) writes scores only for the first ``seed_probes``
        probe columns (default ``default_seed_probes(refine or k, nprobe)``): they give every query a keep-th distance tau
        (keep = refine or k), and one launch over the other columns appends what is within tau to ``filter_cap`` candidate
        slots per query (a power of two in [64, 65536]; default ``default_filter_cap(keep)``).  (D, I) are those of
        ``scan="buffer"`` bit for bit, for either storage and any refine, chunking, query order, ``filter_cap`` and
        ``seed_probes`` (the merged lists agree in their first keep entries; what lies behind them is not promised): a query
        that collects more than ``filter_cap`` candidates is searched again through the score buffer over its whole probe
        row (with the budget raised to its own scores where ``score_bytes`` is below them), so nothing is lost.  A chunk then
        holds the SEED lists' scores plus 8 B x ``filter_cap`` per query within ``score_bytes``: a query whose own probed
        lists exceed the budget is accepted whenever its seed lists fit.  ``stats`` gains ``scan``, ``seed_probes``,
        ``filter_cap``, ``n_appended`` (candidates counted over all chunks, dropped ones included) and ``refiltered`` (queries
        searched again); ``n_floats`` is the seed floats, ``n_tiles`` the tiles of the seed and filter scans."""
        self._check_queries(queries, nprobe, k)
        k, nprobe = int(k), int(nprobe)
        refine, base = self._check_refine(k, refine, base)
        self._check_scan(scan, filter_cap, seed_probes, nprobe)
        self._check_listed()
        probe = self._check_probe(probe, queries.shape[0], nprobe)
        t = queries if torch.is_tensor(queries) else torch.as_tensor(np.asarray(queries, dtype=np.float32))
        dev = self.device
        f16 = self.storage == "f16"
        Q = self._prepared(t, dev, self.l2_norm)
        nq, Dp = Q.shape
        cap = ops.knn_list_capacity()
        best_d = torch.empty((nq, cap), dtype=torch.float32, device=dev)
        best_i = torch.empty((nq, cap), dtype=torch.int32, device=dev)
        if nq:
            q_sq = torch.zeros(nq, dtype=torch.float32, device=dev)
            if not f16:
                ops.row_sqnorm(Q, Dp, q_sq)
            probe = (self._probes(Q, nprobe) if probe is None else probe.to(dev)).to(torch.int32).contiguous()
            if f16:                                           # a query with no finite fp16 image probes nothing
                lost = (Q.abs() >= 65520.0).any(1)            # (fp32 -> fp16 rounds to inf from 65520 on; NaN queries have -1 probes already)
                probe = torch.where(lost[:, None], torch.full_like(probe, -1), probe)
            budget = self.default_score_bytes() if score_bytes is None else score_bytes
            keep = refine or k                                # entries the merge must get right
            cand_d = torch.empty_like(best_d) if refine else best_d
            cand_i = torch.empty_like(best_i) if refine else best_i
            if scan == "filter":
                chunks, n_tiles, n_floats = self._scan_filtered(
                    Q, q_sq, probe, k, refine, base, budget, best_d, best_i, cand_d, cand_i,
                    self.default_seed_probes(keep, nprobe) if seed_probes is None else int(seed_probes),
                    self.default_filter_cap(keep) if filter_cap is None else int(filter_cap), stats)
            else:
                chunks, n_tiles, n_floats = self._scan_buffered(Q, q_sq, probe, k, refine, base, budget, best_d, best_i, cand_d,
                                                                cand_i)
            if stats is not None:
                stats.update(chunks=chunks, n_tiles=n_tiles, n_floats=n_floats, probe=probe)
                if refine:
                    stats.update(candidates=cand_i[:, :refine])
        I = best_i[:, :k].to(torch.int64)
        I[I == 0x7fffffff] = -1
        return best_d[:, :k].contiguous(), I

    # ---- range search ----
    RANGE_CAP = 256             # default candidate slots per query of ``range_search``'s first pass (a tuning choice, not a gate)

    def _check_range_cap(self, range_cap):
        if range_cap is None:
            return self.RANGE_CAP
        c = int(range_cap)
        if isinstance(range_cap, bool) or c != range_cap or not self.FILTER_CAP_MIN <= c <= self.FILTER_CAP_MAX or c & (c - 1):
            raise ValueError("range_cap must be a power of two in [%d, %d], got %r"
                             % (self.FILTER_CAP_MIN, self.FILTER_CAP_MAX, range_cap))
        return c

    def range_costs(self, nq, nprobe, cap):
        """int64 ndarray [nq]: a query's floats in a chunk of ``range_search`` = 2 ``cap`` (its candidate slots, 8 B each) and,
        on storage "pq", its lookup table (and the ``nprobe`` slot scalars of a residual index).  Pure host arithmetic."""
        own = 2 * int(cap)
        if self.storage == "pq":
            own += pq_query_floats(self.pq_m, int(nprobe) if self.pq_residual else 0)
        return np.full(int(nq), own, dtype=np.int64)

    def _range_plan(self, nq, nprobe, cap, result_bytes):
        """the chunks of one pass of ``range_search`` over ``nq`` queries with ``cap`` slots each; a budget below one query's own
        bytes is refused by name, before the launch"""
        costs = self.range_costs(nq, nprobe, cap)
        if nq and 4 * int(costs[0]) > int(result_bytes):
            raise ValueError("result_bytes = %d is less than the %d bytes of one query's %d candidate slots%s: raise result_bytes"
                             % (int(result_bytes), 4 * int(costs[0]), int(cap),
                                " and lookup table" if self.storage == "pq" else ""))
        return ivf_plan_chunks(costs, result_bytes, max_queries=(2 ** 31 - 1) // int(nprobe))

    def _range_filter(self, Qc, q_sq, pc, tau, cap):
        """ONE filter launch over the probe rows ``pc`` of the prepared queries ``Qc`` with tau = the radii: (cnt int32 [m],
        cand int32 [m, cap, 2], tiles).  ``q_sq``: the norms of fp32 queries (fp16 lists take them of the rounded queries here)."""
        dev = Qc.device
        m = Qc.shape[0]
        pq = self.storage == "pq"
        tile = dict(zip(("tile_slots", "tile_rows"), ops.ivf_pq_tile(self.pq_m))) if pq else {}
        tb = ivf_tables(pc, self.list_len, **tile)
        cnt = torch.zeros(m, dtype=torch.int32, device=dev)
        cand = torch.empty((m, cap, 2), dtype=torch.int32, device=dev)
        if not tb["n_tiles"]:                             # nothing probed, or empty lists only
            return cnt, cand, 0
        if pq:
            lut = torch.empty((m, self.pq_m, PQ_CODEWORDS), dtype=torch.float32, device=dev)
            ops.pq_lut(Qc, self.codebooks, lut)
            if self.pq_residual:
                slot_base = torch.empty(tb["n_slots"], dtype=torch.float32, device=dev)
                ops.ivf_slot_dots(Qc, self._C, tb["slot_query"], tb["slot_start"], slot_base)
                ops.ivf_filter_pqr(lut, tb["slot_query"], tb["slot_start"], slot_base, q_sq, tau, cnt, self.codes, self.list_start,
                                   self.r_sq, self.ids, tb["tiles"], cand, cap)
            else:
                ops.ivf_filter_pq(lut, tb["slot_query"], tb["slot_start"], q_sq, tau, cnt, self.codes, self.list_start, self.r_sq,
                                  self.ids, tb["tiles"], cand, cap)
        elif self.storage == "f16":
            Qh = Qc.to(torch.float16)
            q_sq = torch.zeros(m, dtype=torch.float32, device=dev)
            ops.row_sqnorm(Qh.float(), Qc.shape[1], q_sq)
            ops.ivf_filter_f16(Qh, tb["slot_query"], tb["slot_start"], q_sq, tau, cnt, self.rows, self.list_start, self.r_sq, self.ids,
                               tb["tiles"], cand, cap)
        else:
            ops.ivf_filter_f32(Qc, tb["slot_query"], tb["slot_start"], q_sq, tau, cnt, self.rows, self.list_start, self.r_sq, self.ids,
                               tb["tiles"], cand, cap)
        return cnt, cand, tb["n_tiles"]

    def range_search(self, queries, radius, nprobe, probe=None, range_cap=None, result_bytes=None, stats=None):
        """(lims int64 [nq + 1], D fp32 [total], I int64 [total]), device tensors: query q owns D[lims[q]:lims[q + 1]] and the
        same span of I, sorted by (d, id) ascending -- EVERY listed row of the query's ``nprobe`` probed lists with
        d <= radius[q], where d is the distance ``search(..., scan="buffer")`` forms for that (query, row), bit for bit.
        ``radius``: a float or an [nq] tensor, in the squared-L2 units of ``search``; a negative or NaN radius returns nothing
        for its query, +inf every probed listed row; a NaN query returns nothing.  ``probe`` as ``search`` takes it.
        There is no re-rank: on storage "f16" the distances are those of the rounded rows to the rounded query, on "pq" those
        of the decoded rows, as in ``search`` without ``refine``.  An index with ``pq_bits=4`` is refused (its scan has no filter
        launch).
        Per chunk of queries: the slot tables, the lookup tables of a pq index, ONE filter launch (include/cdml_ivf_filter.h,
        include/cdml_ivf_range.h) with tau = radius into ``range_cap`` candidate slots per query (a power
        of two in [64, 65536], default 256) and one host read of the counts.  A chunk holds 8 B x ``range_cap`` per query (and
        a pq query's lookup table) within ``result_bytes`` (default ``default_score_bytes()``).  The queries that counted more
        than ``range_cap`` go through the launch ONCE more with the smallest power of two that holds the largest count; when
        ``result_bytes`` cannot hold one such query, a ValueError says how many bytes it needs.  The result does not depend
        on ``range_cap``, ``result_bytes``, the chunking or the order of the queries.  ``stats`` (a dict, optional) receives
        ``chunks``, ``n_tiles``, ``range_cap``, ``n_results``, ``second_pass`` (queries) and ``second_cap``."""
        self._check_queries(queries, nprobe)
        nprobe = int(nprobe)
        if self.storage == "pq" and self.pq_bits == 4:
            raise ValueError("range_search has no launch for pq_bits=4 (the 4-bit scan has no filter form: DESIGN.md section 10): "
                             "use pq_bits=8")
        cap = self._check_range_cap(range_cap)
        nq = int(queries.shape[0])
        if torch.is_tensor(radius) or isinstance(radius, np.ndarray):
            radius = torch.as_tensor(radius)
            if tuple(radius.shape) != (nq,):
                raise ValueError("radius must be a float or an [nq = %d] tensor, got shape %s" % (nq, tuple(radius.shape)))
        else:
            radius = float(radius)
        self._check_listed()
        probe = self._check_probe(probe, nq, nprobe)
        t = queries if torch.is_tensor(queries) else torch.as_tensor(np.asarray(queries, dtype=np.float32))
        dev = self.device
        budget = self.default_score_bytes() if result_bytes is None else int(result_bytes)
        chunks = self._range_plan(nq, nprobe, cap, budget)
        Q = self._prepared(t, dev, self.l2_norm)
        Dp = Q.shape[1]
        st = dict(chunks=chunks, n_tiles=0, range_cap=cap, n_results=0, second_pass=0, second_cap=0)
        if stats is not None:
            stats.update(st)
        if not nq:
            z = torch.zeros(1, dtype=torch.int64, device=dev)
            return z, torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
        tau = (radius.to(device=dev, dtype=torch.float32) if torch.is_tensor(radius)
               else torch.full((nq,), radius, dtype=torch.float32, device=dev)).contiguous()
        q_sq = torch.zeros(nq, dtype=torch.float32, device=dev)
        if self.storage != "f16":
            ops.row_sqnorm(Q, Dp, q_sq)
        probe = (self._probes(Q, nprobe) if probe is None else probe.to(dev)).to(torch.int32).contiguous()
        if self.storage == "f16":                         # a query with no finite fp16 image probes nothing, as in ``search``
            lost = (Q.abs() >= 65520.0).any(1)
            probe = torch.where(lost[:, None], torch.full_like(probe, -1), probe)
        parts, redo, redo_cnt = [], [], []
        for q0, q1 in chunks:
            cnt, cand, nt = self._range_filter(Q[q0:q1], q_sq[q0:q1], probe[q0:q1].contiguous(), tau[q0:q1], cap)
            st["n_tiles"] += nt
            cnt_h = cnt.cpu()                             # the host read
            over = cnt_h > cap
            if bool(over.any()):                          # these queries lost candidates: none of theirs is kept from this pass
                idx = torch.nonzero(over).flatten()
                redo.append(idx + q0)
                redo_cnt.append(cnt_h[idx])
                cnt = torch.where(over.to(dev), torch.zeros_like(cnt), cnt)
            parts.append(range_compact(cand, cnt, cap))
            del cand
        n1 = torch.cat([p[0][1:] - p[0][:-1] for p in parts])
        D1, I1 = torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])
        if not redo:
            lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            lims[1:] = torch.cumsum(n1, 0)
            st["n_results"] = int(D1.numel())
            if stats is not None:
                stats.update(st)
            return lims, D1, I1
        # the second pass, once: the queries over capacity with room for the largest count
        idx = torch.cat(redo).to(dev)
        want = torch.cat(redo_cnt)
        cap2 = 1 << (int(want.max()) - 1).bit_length()
        chunks2 = self._range_plan(int(idx.numel()), nprobe, cap2, budget)
        Q2, s2, p2, t2 = Q.index_select(0, idx), q_sq.index_select(0, idx), probe.index_select(0, idx), tau.index_select(0, idx)
        parts2 = []
        for q0, q1 in chunks2:
            cnt, cand, nt = self._range_filter(Q2[q0:q1], s2[q0:q1], p2[q0:q1].contiguous(), t2[q0:q1], cap2)
            st["n_tiles"] += nt
            if not torch.equal(cnt.cpu(), want[q0:q1]):
                raise RuntimeError("range_search: the second launch counted other candidates than the first")
            parts2.append(range_compact(cand, cnt, cap2))
            del cand
        D2, I2 = torch.cat([p[1] for p in parts2]), torch.cat([p[2] for p in parts2])
        n2 = want.to(device=dev, dtype=torch.int64)
        n = n1.clone()
        n[idx] = n2
        lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        lims[1:] = torch.cumsum(n, 0)
        D = torch.empty(int(lims[-1]), dtype=torch.float32, device=dev)
        I = torch.empty(int(lims[-1]), dtype=torch.int64, device=dev)
        for Dx, Ix, nx, owner in ((D1, I1, n1, torch.arange(nq, device=dev)), (D2, I2, n2, idx)):
            start = torch.cumsum(nx, 0) - nx                  # where each query's span begins in this pass's output
            own = torch.repeat_interleave(torch.arange(nx.numel(), device=dev), nx)
            dest = lims[owner[own]] + (torch.arange(Dx.numel(), device=dev) - start[own])
            D[dest], I[dest] = Dx, Ix
        st.update(n_results=int(D.numel()), second_pass=int(idx.numel()), second_cap=cap2)
        if stats is not None:
            stats.update(st)
        return lims, D, I


def range_compact(cand, cnt, cap):
    """(lims int64 [m + 1], D fp32 [total], I int64 [total]) of the candidate lists a filter launch filled: ``cand`` int32
    [m, cap, 2] pairs (the bits of d, id), ``cnt`` int32 [m] the candidates counted.  The first min(cnt, cap) slots of every query
    are kept and sorted by (d, id) ascending.  d is never negative and never NaN there, so its bits order as integers.  Plain
    torch on the tensors' device (CPU tensors too)."""
    cap = int(cap)
    m = int(cnt.numel())
    dev = cand.device
    c = cand.reshape(-1)[:2 * m * cap].view(m, cap, 2)
    n = cnt.to(torch.int64).clamp(min=0, max=cap)
    lims = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    lims[1:] = torch.cumsum(n, 0)
    keep = torch.arange(cap, device=dev)[None, :] < n[:, None]
    owner = torch.repeat_interleave(torch.arange(m, device=dev), n)       # ascending: the mask selects row by row
    key = (c[..., 0][keep].to(torch.int64) << 32) | c[..., 1][keep].to(torch.int64)       # d's bits < 2^31, id in [0, 2^31)
    key, order = torch.sort(key)
    key = key[torch.sort(owner[order], stable=True)[1]]                   # back into the queries' spans, (d, id) kept inside
    D = (key >> 32).to(torch.int32).view(torch.float32)
    return lims, D, key & 0xffffffff


def ivf_range(base, queries=None, radius=None, nlist=1024, nprobe=16, l2_norm=True, storage="f32", iters=10, seed=0,
              device="cuda:0", precision="f32x3", index=None, stats=None, pq_m=None, pq_residual=False, range_cap=None,
              result_bytes=None):
    """Device (lims, D, I) of ``IVFIndex.range_search``: the index of ``base`` (built here as ``ivf_knn`` builds it, or taken as
    ``index=``), every listed row of a query's ``nprobe`` nearest lists within ``radius`` (a float or an [nq] tensor, squared
    L2).  ``queries=None`` searches the catalogue against itself.  No re-rank: the distances of storage "f16" / "pq" are
    those of the stored values."""
    if radius is None:
        raise ValueError("ivf_range needs radius: a float or an [nq] tensor of squared-L2 radii")
    if index is None:
        if storage not in IVF_STORAGES:
            raise ValueError("storage must be one of %s, got %r" % (IVF_STORAGES, storage))
        _check_pq_residual(storage, pq_residual)
        _check_pq_m(storage, pq_m)
        index = IVFIndex.build(base, int(nlist), iters=iters, seed=seed, l2_norm=l2_norm, device=device, precision=precision,
                               storage=storage, pq_m=pq_m, pq_residual=pq_residual)
    return index.range_search(base if queries is None else queries, radius, int(nprobe), range_cap=range_cap,
                              result_bytes=result_bytes, stats=stats)
