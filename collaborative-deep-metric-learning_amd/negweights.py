"""The proposal distribution of the weighted negatives as integer tables (include/cdml_negweights.h; build-defined).

``NegativeWeights`` turns one weight per catalogue row -- e.g. the unigram^0.75 of word2vec (Mikolov et al. 2013) over the
co-watch degree counts, or its mixture with uniform -- into what sampler mode 3 reads: every row owns ``quanta[v]`` of the
2^32 values of a 32-bit word, so a draw is one Philox word and a search, exact and counter-based like the other sampler
modes, and ``lq[v] = log(quanta[v] / 2^32)`` is exactly the log-probability the sampler used (the importance correction
of the sampled softmax, Bengio & Senecal 2008).  Host numpy, off the step path.

The quantisation rule, with P the rows of positive weight and T = 2^32:
    base[v] = 1 + floor(w[v] / sum(w) * (T - |P|))        in float64, 0 for a row of weight 0
    R = T - sum(base) is spread one quantum each (+1 if R > 0, -1 if R < 0) over the |R| largest entries of base, ties to
    the lower id (repeated while |R| > |P|, which no input has needed; an entry is never taken below 1)
so sum(quanta) = 2^32 EXACTLY, quanta[v] = 0 exactly where w[v] = 0, and every positive entry ends within 2 quanta of
1 + w / sum(w) * (T - |P|).
"""
import collections
import math

import numpy as np
import torch

TOTAL = 1 << 32
MIN_POSITIVE, MAX_POSITIVE = 3, 1 << 31
MIN_BITS, MAX_BITS, DEFAULT_BITS = 8, 24, 16

# the device tables of one distribution: start int32 (uint32 bits), coarse int32 [2^bits + 1], lq fp32 [n_rows]; n_live = the
# length of start the sampler clamps its search to
NegTables = collections.namedtuple("NegTables", "start coarse lq bits n_live")


def check_weights(w, n_rows=None):
    """The refusals of a weight vector, by name; returns it as a float64 ndarray."""
    if torch.is_tensor(w):
        w = w.detach().cpu().numpy()
    w = np.asarray(w)
    if w.ndim != 1 or (n_rows is not None and w.shape[0] != int(n_rows)):
        raise ValueError("negative_weights needs one weight per catalogue row%s, got shape %s"
                         % ("" if n_rows is None else " (%d)" % int(n_rows), tuple(w.shape)))
    if w.dtype.kind not in "fiu":
        raise ValueError("negative_weights must be real numbers, got dtype %s" % w.dtype)
    w = w.astype(np.float64)
    if not np.isfinite(w).all():
        raise ValueError("negative_weights must be finite")
    if (w < 0).any():
        raise ValueError("negative_weights must be >= 0 (a negative weight at row %d)" % int(np.flatnonzero(w < 0)[0]))
    n_pos = int((w > 0).sum())
    if n_pos < MIN_POSITIVE or n_pos > MAX_POSITIVE:
        raise ValueError("negative_weights needs at least %d and at most 2^31 positive entries, got %d" % (MIN_POSITIVE, n_pos))
    return w


def quantise(w):
    """int64 [n] quanta of the weights ``w`` (float64, checked): the rule of the module's docstring."""
    pos = w > 0
    n_pos = int(pos.sum())
    ids = np.flatnonzero(pos)
    share = w[ids] / w[ids].sum()
    base = 1 + np.floor(share * float(TOTAL - n_pos)).astype(np.int64)
    rest = TOTAL - int(base.sum())
    if rest:
        order = np.lexsort((ids, -base))                  # the largest entries first, ties to the lower id
        while rest:
            sign = 1 if rest > 0 else -1
            take = order[:min(abs(rest), n_pos)]
            if sign < 0:
                take = take[base[take] > 1]
                if not len(take):
                    raise ValueError("negative_weights cannot be quantised to 2^32 quanta")
            base[take] += sign
            rest -= sign * len(take)
    q = np.zeros(len(w), dtype=np.int64)
    q[ids] = base
    return q


class NegativeWeights:
    """The tables of one distribution over ``n_rows`` catalogue rows (CPU tensors):

    ``quanta`` int64 [n_rows], sum = 2^32, 0 exactly for the rows of weight 0; ``n_live`` = 1 + the last positive row;
    ``start`` int32 [n_live] holding the uint32 exclusive prefix sums of quanta (rows at or after n_live own nothing and are
    outside the search: their prefix, 2^32, does not fit); ``coarse`` int32 [2^bits + 1] with coarse[b] = owner(b << (32 -
    bits)) and coarse[2^bits] = n_live - 1; ``lq`` fp32 [n_rows] = log(max(quanta, 1)) - 32 ln 2 (float64, rounded once;
    finite for the rows of weight 0, which only the sampler's uniform fall-back can draw).
    owner(r) = the largest v < n_live with start[v] <= r."""

    def __init__(self, quanta, bits=DEFAULT_BITS):
        q = quanta.detach().cpu().numpy() if torch.is_tensor(quanta) else np.asarray(quanta)
        bits = int(bits)
        if not MIN_BITS <= bits <= MAX_BITS:
            raise ValueError("bits must be in [%d, %d], got %d" % (MIN_BITS, MAX_BITS, bits))
        if q.ndim != 1 or q.dtype.kind not in "iu" or (q < 0).any() or int(q.astype(np.int64).sum()) != TOTAL:
            raise ValueError("quanta must be a 1-D vector of non-negative integers that sum to 2^32")
        q = q.astype(np.int64)
        n_pos = int((q > 0).sum())
        if n_pos < MIN_POSITIVE:
            raise ValueError("negative_weights needs at least %d positive entries, got %d" % (MIN_POSITIVE, n_pos))
        self.n_rows, self.bits = len(q), bits
        self.n_live = int(np.flatnonzero(q)[-1]) + 1
        prefix = np.cumsum(q) - q                                           # exclusive, int64
        start = prefix[:self.n_live]
        edges = np.arange(1 << bits, dtype=np.int64) << (32 - bits)
        coarse = np.empty((1 << bits) + 1, dtype=np.int32)
        coarse[:-1] = np.searchsorted(start, edges, side="right") - 1
        coarse[-1] = self.n_live - 1
        lq = np.log(np.maximum(q, 1).astype(np.float64)) - 32.0 * math.log(2.0)
        self.quanta = torch.from_numpy(q)
        self.start = torch.from_numpy(start.astype(np.uint32).view(np.int32).copy())
        self.coarse = torch.from_numpy(coarse)
        self.lq = torch.from_numpy(lq.astype(np.float32))

    @classmethod
    def from_weights(cls, w, bits=DEFAULT_BITS):
        """``w``: 1-D tensor or array of finite weights >= 0, at least 3 (and at most 2^31) of them positive."""
        return cls(quantise(check_weights(w)), bits)

    @classmethod
    def from_counts(cls, counts, power=0.75, uniform_mix=0.0, bits=DEFAULT_BITS):
        """w = (1 - uniform_mix) * c^power / sum(c^power) + uniform_mix / n over the counts c (e.g. the degree counts of
        parse_data.cowatch_graph): the unigram^power family and its mixtures with uniform."""
        power, lam = float(power), float(uniform_mix)
        if not (0.0 <= power < float("inf")):
            raise ValueError("power must be finite and >= 0, got %r" % (power,))
        if not 0.0 <= lam <= 1.0:
            raise ValueError("uniform_mix must be in [0, 1], got %r" % (uniform_mix,))
        c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
        c = c.astype(np.float64)
        if c.ndim != 1 or not np.isfinite(c).all() or (c < 0).any():
            raise ValueError("counts must be a 1-D vector of finite numbers >= 0")
        cp = np.where(c > 0, np.power(np.maximum(c, 1e-300), power), 0.0)
        total = cp.sum()
        if not total > 0 and lam < 1.0:
            raise ValueError("counts must have a positive entry")
        w = lam / len(c) + ((1.0 - lam) * cp / total if total > 0 else 0.0)
        return cls.from_weights(w, bits)

    def owner(self, r):
        """owner(r) of 32-bit words ``r`` (int or integer array): the host definition, by a search over all of start."""
        start = self.start.numpy().view(np.uint32).astype(np.int64)
        return np.searchsorted(start, np.asarray(r, dtype=np.int64), side="right") - 1

    def tables(self, device, pad_to=None):
        """The device copies the sampler and ``ops.negw_bias`` read.  ``pad_to`` (>= n_live): ``start`` padded with
        0xFFFFFFFF to that length and ``n_live`` reported as that length -- a buffer that later distributions over the same
        rows can be copied into; the draw is unchanged, since coarse[] never brackets a padded row."""
        start, n_live = self.start, self.n_live
        if pad_to is not None:
            if int(pad_to) < n_live:
                raise ValueError("pad_to must be >= n_live = %d, got %d" % (n_live, int(pad_to)))
            start = torch.full((int(pad_to),), -1, dtype=torch.int32)
            start[:n_live] = self.start
            n_live = int(pad_to)
        return NegTables(start.to(device).contiguous(), self.coarse.to(device).contiguous(), self.lq.to(device).contiguous(),
                         self.bits, n_live)


def as_negative_weights(w, n_rows, bits=DEFAULT_BITS):
    """``w`` as a NegativeWeights over ``n_rows`` rows: one already, or a weight vector (checked by name)."""
    if isinstance(w, NegativeWeights):
        if w.n_rows != int(n_rows):
            raise ValueError("negative_weights needs one weight per catalogue row (%d), got %d" % (int(n_rows), w.n_rows))
        return w
    return NegativeWeights(quantise(check_weights(w, n_rows)), bits)
