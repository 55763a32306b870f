"""Losses behind the reference's loss plug-in API (losses.py)."""
import torch

from . import ops


class BaseLoss(object):
    """Inherit from this class when implementing new losses (losses.py:4-18)."""

    def calculate_loss(self, unused_triplets, **unused_params):
        raise NotImplementedError()


class _HingeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, triplets, margin):
        B, C, D = triplets.shape
        e = triplets.contiguous().view(B * 3, D)
        dev = e.device
        pos, neg, hinge = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        de = torch.empty_like(e) if triplets.requires_grad else None
        ops.triplet_hinge(e, B, D, margin, pos, neg, hinge, stats, de)
        ctx.de = de
        ctx.shape = triplets.shape
        ctx.mark_non_differentiable(pos, neg, hinge, stats)
        return stats[0].clone(), pos, neg, hinge, stats

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        return (ctx.de * g_loss).view(ctx.shape), None


class HingeLoss(BaseLoss):
    def calculate_loss(self, triplets, margin=0.1):
        """losses.py:20-49.  triplets: float32 [batch, 3, embedding] device tensor
        (anchor, positive, negative).  Returns the reference's dict; distances are
        SQUARED L2 and keep tf.split's channel axis ([batch, 1])."""
        if triplets.dim() != 3 or triplets.shape[1] != 3:
            raise ValueError("triplets must be [batch, 3, embedding]")
        if triplets.shape[2] % 4:
            raise ValueError("embedding size must be a multiple of 4")
        triplets = triplets.to(torch.float32)
        loss, pos, neg, hinge, stats = _HingeFunction.apply(triplets, float(margin))
        self.summary = {"mean_pos_dist": stats[1], "mean_neg_dist": stats[2]}   # losses.py:40-41
        return {"hinge_loss": loss,
                "anchors": triplets[:, 0:1, :],
                "positives": triplets[:, 1:2, :],
                "negatives": triplets[:, 2:3, :],
                "pos_dist": pos.view(-1, 1),
                "neg_dist": neg.view(-1, 1),
                "hinge_dist": hinge.view(-1, 1)}


class _NPairFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pairs, temperature, symmetric, ids, logq=None):
        B, _, D = pairs.shape
        dev = pairs.device
        # the chain's tile rules: B up to a multiple of 256 pairs, D up to a multiple of 64 columns, zero rows / columns
        # (a zero pair has no video id of its own: it is never read past B)
        tile = ops.NPAIR_TILE["f32x3"]
        Bp, Dp = (B + tile - 1) // tile * tile, (D + 63) // 64 * 64
        e = torch.zeros((2 * Bp, Dp), dtype=torch.float32, device=dev)
        e[:2 * B, :D] = pairs.reshape(2 * B, D)
        rows = None
        if ids is not None:
            rows = torch.zeros(2 * Bp, dtype=torch.int32, device=dev)
            rows[:2 * B] = ids.reshape(-1).to(device=dev, dtype=torch.int32)
        ws = ops.NPairWorkspace(Bp, Dp, "f32x3", dev)
        de = torch.zeros_like(e) if pairs.requires_grad else None
        stats = torch.zeros(4, dtype=torch.float32, device=dev)
        bias = None
        if logq is not None:                              # each row's lq, laid out like rows (padded pairs: 0)
            bias = torch.zeros(2 * Bp, dtype=torch.float32, device=dev)
            bias[:2 * B] = logq.reshape(-1).to(device=dev, dtype=torch.float32)
        ops.npair_loss(e, rows, B, Dp, temperature, symmetric, "f32x3", de=de, stats=stats, ws=ws, logq=bias)
        part = ws.ws[:4 * B].view(B, 4)                   # per anchor: loss term, 2 - 2 <a, p>, negatives' sum, their count
        pos = part[:, 1].clone()
        neg = part[:, 2] / part[:, 3].clamp(min=1.0)
        ctx.de = None if de is None else de[:2 * B, :D].reshape(B, 2, D)
        ctx.mark_non_differentiable(pos, neg, stats)
        return stats[0].clone(), pos, neg, stats

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        return ctx.de * g_loss, None, None, None, None


class _NPairMixedFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pairs, negatives, temperature, symmetric, ids, logq, negative_ids, negative_logq):
        B, _, D = pairs.shape
        dev = pairs.device
        Dp = (D + 63) // 64 * 64                          # zero columns up to the chain's width; the batch is not padded
        e = torch.zeros((3 * B, Dp), dtype=torch.float32, device=dev)
        e3 = e.view(B, 3, Dp)
        e3[:, :2, :D] = pairs
        e3[:, 2, :D] = negatives
        rows = None
        if ids is not None:
            rows = torch.empty((B, 3), dtype=torch.int32, device=dev)
            rows[:, :2] = ids.reshape(B, 2).to(device=dev, dtype=torch.int32)
            rows[:, 2] = negative_ids.reshape(B).to(device=dev, dtype=torch.int32)
            rows = rows.view(-1)
        ws = ops.NPairMixed(B, Dp, "f32x3", dev)
        need = pairs.requires_grad or negatives.requires_grad
        de = torch.zeros_like(e) if need else None
        stats = torch.zeros(4, dtype=torch.float32, device=dev)
        bias = None if logq is None else logq.reshape(-1).to(device=dev, dtype=torch.float32)
        vec = isinstance(negative_logq, torch.Tensor)     # one log-probability per negative: the chain's vector path
        nb = negative_logq.reshape(-1).to(device=dev, dtype=torch.float32).contiguous() if vec and bias is not None else None
        ops.npair_mixed_loss(e, rows, B, Dp, temperature, symmetric, "f32x3", de=de, stats=stats, ws=ws, logq=bias,
                             lq_u=negative_logq if bias is not None and not vec else 0.0, neg_bias=nb)
        part = ws.ws[:4 * B].view(B, 4)
        pos = part[:, 1].clone()
        neg = part[:, 2] / part[:, 3].clamp(min=1.0)
        ctx.de = None if de is None else de.view(B, 3, Dp)[:, :, :D]
        ctx.mark_non_differentiable(pos, neg, stats)
        return stats[0].clone(), pos, neg, stats

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        return ctx.de[:, :2] * g_loss, ctx.de[:, 2] * g_loss, None, None, None, None, None, None


class NPairLoss(BaseLoss):
    def calculate_loss(self, pairs, temperature=0.1, symmetric=True, ids=None, logq=None, negatives=None, negative_ids=None,
                       negative_logq=None):
        """Multi-class N-pair (in-batch softmax) loss -- build-defined, the reference has no such loss.  pairs: float32
        [batch, 2, embedding] device tensor of unit rows (anchor, positive); every other pair's positive is a negative of
        an anchor, and with ``symmetric`` every other anchor a negative of a positive.  ``ids`` (int [batch, 2] video ids of
        the rows, optional): a negative that is the same video as the anchor or its positive does not count.
        ``temperature`` 0.1 and ``symmetric`` True are the build's defaults.  Distances are SQUARED L2 of unit rows:
        pos_dist = |a_i - p_i|^2, neg_dist = the mean over anchor i's counted negatives ([batch, 1]).  ``logq`` (float
        [batch, 2], optional): each row's log sampling probability -- the sampling-bias correction of Yi et al. 2019, every
        logit less its candidate's logq (the anchor's in the column term, the positive's in the row term).
        ``negatives`` (float [batch, embedding] unit rows, optional): mixed negative sampling -- one uniformly drawn
        catalogue negative per pair; every anchor's softmax then also runs over all of them, and they receive a gradient
        (the returned dict gains "negatives").  The batch must be a multiple of 256 pairs (a padding row would be a
        negative).  ``negative_ids`` (int [batch], required with ``ids``): a negative that is the anchor's or its positive's
        video does not count; ``negative_logq`` (with ``logq``; default 0): one float -- the uniform draw's log probability
        -- or a float tensor [batch], the log sampling probability of each negative (a non-uniform proposal)."""
        if pairs.dim() != 3 or pairs.shape[1] != 2:
            raise ValueError("pairs must be [batch, 2, embedding]")
        if negatives is None and (negative_ids is not None or negative_logq is not None):
            raise ValueError("negative_ids and negative_logq go with negatives")
        if negatives is not None:
            B, tile = pairs.shape[0], ops.NPAIR_TILE["f32x3"]
            if negatives.dim() != 2 or tuple(negatives.shape) != (B, pairs.shape[2]):
                raise ValueError("negatives must be [batch, embedding], one row per pair")
            if B % tile:
                raise ValueError("with negatives the batch must be a multiple of %d pairs (got %d)" % (tile, B))
            if (ids is None) != (negative_ids is None):
                raise ValueError("ids and negative_ids go together (one video id per row)")
            if negative_ids is not None and negative_ids.numel() != B:
                raise ValueError("negative_ids must hold one video id per negative ([batch])")
            if negative_logq is not None:
                if logq is None:
                    raise ValueError("negative_logq goes with logq (without one no logit is corrected)")
                if isinstance(negative_logq, torch.Tensor) and negative_logq.numel() != 1:
                    if negative_logq.numel() != B or not bool(torch.isfinite(negative_logq).all()):
                        raise ValueError("a negative_logq tensor must hold one finite log-probability per negative ([batch])")
                else:
                    negative_logq = float(negative_logq)
                    if not (float("-inf") < negative_logq < float("inf")):
                        raise ValueError("negative_logq must be a finite float")
        if ids is not None and ids.numel() != 2 * pairs.shape[0]:
            raise ValueError("ids must hold one video id per row ([batch, 2])")
        if logq is not None:
            if logq.numel() != 2 * pairs.shape[0]:
                raise ValueError("logq must hold one log-probability per row ([batch, 2])")
            if not bool(torch.isfinite(logq).all()):
                raise ValueError("every logq entry must be finite")
        pairs = pairs.to(torch.float32)
        if negatives is not None:
            negatives = negatives.to(torch.float32)
            loss, pos, neg, stats = _NPairMixedFunction.apply(pairs, negatives, float(temperature), bool(symmetric), ids, logq,
                                                              negative_ids, 0.0 if negative_logq is None else negative_logq)
            self.summary = {"mean_pos_dist": stats[1], "mean_neg_dist": stats[2]}
            return {"npair_loss": loss,
                    "anchors": pairs[:, 0:1, :],
                    "positives": pairs[:, 1:2, :],
                    "negatives": negatives[:, None, :],
                    "pos_dist": pos.view(-1, 1),
                    "neg_dist": neg.view(-1, 1)}
        loss, pos, neg, stats = _NPairFunction.apply(pairs, float(temperature), bool(symmetric), ids, logq)
        self.summary = {"mean_pos_dist": stats[1], "mean_neg_dist": stats[2]}
        return {"npair_loss": loss,
                "anchors": pairs[:, 0:1, :],
                "positives": pairs[:, 1:2, :],
                "pos_dist": pos.view(-1, 1),
                "neg_dist": neg.view(-1, 1)}
